"""Shared by tests/test_rebalance_edges.py (CPU) and tests/test_rebalance_edges_gpu.py: the committed vectors of the rebalancers' edge
cases (tests/golden/ref_rebalance_edges.npz), the cases themselves, and the two restatements' answers in the vectors' layout."""
import os

import numpy as np

from oracle import bind as ob
from oracle import py_rebalance as pr
from tests import ref_fleets as rf

GOLDEN_REBALANCE_EDGES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_rebalance_edges.npz")
NAMES = [str(n) for n in np.load(GOLDEN_REBALANCE_EDGES)["names"]]
SCALE_FIELDS = ("action", "copies", "timestamp", "new_i1", "new_i2", "heavy")
CONC_FIELDS = ("threshold", "reset", "new_prior_sum", "new_prior_count")
INFO_FIELDS = ("size_estimate", "free_count", "total_count", "n_candidates", "n_selected", "error", "space_to_fill", "cutoff")
STAT_FIELDS = ("total_capacity", "total_free", "global_lru", "instance_count", "model_copy_count")


def tier_names(tier):
    return [n for n in NAMES if rf.rebalance_edge_tier(n) == tier]


def load_cases():
    """(the vectors, {name: (tier, case)}): built once per module, shared, left unchanged."""
    return np.load(GOLDEN_REBALANCE_EDGES), {name: (tier, case) for name, tier, case in rf.rebalance_edge_cases()}


def sd(st):
    return {n: int(st[n]) for n in st.dtype.names}


def py_registry(fleet):
    out = []
    for m in fleet.models:
        o, k, f = int(m["ent_off"]), int(m["n_loaded"]), int(m["n_failed"])
        out.append(dict(type=int(m["type"]), last_used=int(m["last_used"]),
                        loaded=[(int(fleet.ent_pod[o + i]), int(fleet.ent_time[o + i])) for i in range(k)],
                        failed=[(int(fleet.ent_pod[o + k + i]), int(fleet.ent_time[o + k + i])) for i in range(f)]))
    return out


def py_rows(rows):
    return [{k: int(r[k]) for k in rows.dtype.names} for r in rows]


def py_table(fleet):
    return [dict(rpm=int(r["rpm"]), shutting_down=bool(r["flags"] & 1), in_table=not bool(r["flags"] & 4)) for r in fleet.pods]


def scale_matrix(outs):
    return np.stack([np.asarray(outs[f]).astype(np.int64) for f in SCALE_FIELDS], 1).reshape(-1, len(SCALE_FIELDS))


def conc_matrix(couts):
    return np.stack([np.asarray(couts[f]).astype(np.int64) for f in CONC_FIELDS], 1).reshape(-1, len(CONC_FIELDS))


def c_rate(case):
    """-> dict(scale, rpm, overloaded, skipped[, conc, average_model_parallelism, model_parallelism_sum]) by oracle/mm_rebalance_oracle.c"""
    fleet, _, entries, conc, sp, cp, _ = case
    if conc is None:
        outs, ov, sk = ob.scaleup_plan(fleet, entries, sp.view(ob.ORC_SCALEUP_PARAMS))
        return dict(scale=scale_matrix(outs), rpm=outs["rpm"].astype(np.int64), overloaded=ov, skipped=int(sk))
    outs, couts, ov, sk, res = ob.scaleup_plan_conc(fleet, entries, conc, sp.view(ob.ORC_SCALEUP_PARAMS), cp)
    return dict(scale=scale_matrix(outs), rpm=outs["rpm"].astype(np.int64), overloaded=ov, skipped=int(sk), conc=conc_matrix(couts),
                average_model_parallelism=float(res["average_model_parallelism"]), model_parallelism_sum=int(res["model_parallelism_sum"]))


def py_rate(case):
    """The same by oracle/py_rebalance.py."""
    fleet, _, entries, conc, sp, cp, _ = case
    orc = ob.OracleFleet(fleet)
    args = (py_table(fleet), [int(x) for x in orc.order], sd(orc.stats()), [sd(t) for t in ob.type_set_stats(fleet)], bool(fleet.n_types),
            py_registry(fleet), py_rows(entries), {n: int(sp[n][0]) for n in sp.dtype.names})
    if conc is None:
        outs, ov, early = pr.scaleup(*args)
        res = None
    else:
        outs, ov, early, res = pr.scaleup(*args, py_rows(conc), dict(dynamic_rpm_scale_constant=int(cp["dynamic_rpm_scale_constant"][0]),
                                                                  average_model_parallelism=float(cp["average_model_parallelism"][0])))
    mask = np.zeros(fleet.n_pods, np.uint8)
    mask[sorted(ov)] = 1
    out = dict(scale=np.array([[o[f] for f in SCALE_FIELDS] for o in outs], np.int64).reshape(-1, 6), rpm=np.array([o["rpm"] for o in outs], np.int64),
               overloaded=mask, skipped=int(early))
    if res is not None:
        out["conc"] = np.array([[o[f] for f in CONC_FIELDS] for o in outs], np.int64).reshape(-1, 4)
        out["average_model_parallelism"], out["model_parallelism_sum"] = res["average_model_parallelism"], res["model_parallelism_sum"]
    return out


def check_rate(name, got, ref, who=""):
    """Every field of every row against the vectors; the overloaded set where the reference's run shows it (a scale-up happened)."""
    want = ref[f"{name}/scale"]
    bad = np.argwhere(got["scale"] != want)
    assert len(bad) == 0, (name, who, "first differing row", int(bad[0][0]), SCALE_FIELDS[bad[0][1]], got["scale"][bad[0][0]], want[bad[0][0]])
    if np.any(want[:, 0] == 2):
        assert np.array_equal(np.asarray(got["overloaded"]).astype(np.uint8), ref[f"{name}/overloaded"]), (name, who, "overloaded")
    if f"{name}/conc" in ref:
        wc = ref[f"{name}/conc"]
        bad = np.argwhere(got["conc"] != wc)
        assert len(bad) == 0, (name, who, "first differing row", int(bad[0][0]), CONC_FIELDS[bad[0][1]], got["conc"][bad[0][0]], wc[bad[0][0]])
        assert got["average_model_parallelism"] == float(ref[f"{name}/average_model_parallelism"][0]), (name, who)


def c_janitor(case):
    fleet, _, entries, conc, dp, dyn, _ = case
    if conc is None:
        return ob.scaledown_plan(fleet, entries, dp.view(ob.ORC_SCALEDOWN_PARAMS))
    return ob.scaledown_plan_conc(fleet, entries, conc, dp.view(ob.ORC_SCALEDOWN_PARAMS), dyn)


def py_janitor(case):
    fleet, _, entries, conc, dp, dyn, _ = case
    orc = ob.OracleFleet(fleet)
    pos_of = {int(p): i for i, p in enumerate(orc.order)}
    st = {n: int(v) for n, v in zip(ob.ORC_STATS.names, ob.instance_set_stats(fleet, int(dp["self_pod"][0]), orc)[0])}
    got = pr.scaledown(py_table(fleet), {p: pos_of.get(p, 2**31 - 1) for p in range(fleet.n_pods)}, st, py_registry(fleet), py_rows(entries),
                       {n: int(dp[n][0]) for n in dp.dtype.names}, None if conc is None else py_rows(conc), dyn)
    return np.array(got, np.uint8)


def check_janitor(name, got, ref, who=""):
    bad = np.flatnonzero(np.asarray(got) != ref[f"{name}/removed"])
    assert bad.size == 0, (name, who, "first differing row", int(bad[0]), int(got[bad[0]]), int(ref[f"{name}/removed"][bad[0]]))


def plan_subsets(fleet, partitioned):
    """[(partition or -1, its stats, instance in subset, prohibited type rows)] as the reaper walks them"""
    g = sd(ob.OracleFleet(fleet).stats())
    if not partitioned:
        return g, [(-1, g, None, None)]
    pts, sets, pst = ob.partition_stats(fleet)
    return g, [(k, sd(pst[k]), [int(x) == k for x in pts], set(int(t) for t in sets[k])) for k in range(len(sets))]


def py_plan(case):
    """-> (calls (model, lastUsed, subset), [info per subset]) by oracle/py_rebalance.py"""
    fleet, _, units, partitioned, _ = case
    pods = [dict(capacity=int(r["capacity"]), used=int(r["used"]), loading_threads=int(r["loading_threads"]),
                 loading_in_progress=int(r["loading_in_progress"]), shutting_down=bool(r["flags"] & 5)) for r in fleet.pods]
    models = [dict(type=int(m["type"]), last_used=int(m["last_used"]), loaded=list(range(int(m["n_loaded"]))), failed=list(range(int(m["n_failed"]))))
              for m in fleet.models]
    g, subsets = plan_subsets(fleet, partitioned)
    calls, infos, taken = [], [], set()
    for k, st, in_subset, prohibited in subsets:
        sel, info = pr.proactive(pods, g, st, in_subset, prohibited, taken if k >= 0 else None, models, units, fleet.now)
        assert sel is not None, "sizeEstimate == 0: the generator refuses such a case"
        calls += [(i, lu, max(k, 0)) for i, lu in sel]
        taken |= {i for i, _ in sel}
        infos.append(info)
    return np.array(calls, np.int64).reshape(-1, 3), infos


def device_plan(plan, fleet, units, partitioned, n_parts):
    """(calls, [info per subset]) from plan(partition, skip) -> (models, last_used, info), as tests/test_ref_vectors.py:plan_calls walks it."""
    from tests.test_ref_vectors import plan_calls
    infos = []

    def keep(k, skip):
        m, lu, info = plan(k, skip)
        infos.append(info)
        return m, lu, info
    return plan_calls(keep, fleet, units, partitioned, n_parts), infos


def check_plan(name, calls, ref, who=""):
    want = ref[f"{name}/proactive"]
    assert calls.shape == want.shape, (name, who, "calls", len(calls), len(want), calls[:3], want[:3])
    bad = np.argwhere(calls != want)
    assert len(bad) == 0, (name, who, "first differing call", int(bad[0][0]), calls[bad[0][0]], want[bad[0][0]])


def check_infos(name, got, want):
    assert len(got) == len(want), name
    for k, (g, w) in enumerate(zip(got, want)):
        for f in INFO_FIELDS:
            assert int(g[f]) == int(w[f]), (name, "subset", k, f, int(g[f]), int(w[f]))
