"""GPU: the type-constraint kernels (row a18) against tests/golden/ref_type_edges.npz — what TypeConstraintManager's own text answers
on the cases of tests/ref_type_edges.py (see tests/test_type_edges.py, which asserts the premises and holds the restatements to the
same vectors).  Every comparison is exact.  Every case goes through every route that reaches type_sets_kernel / type_prefer_kernel
(the caller's label words; the resident ones behind 64 label names), stage_partitions and the stats kernels (fused into the commit;
by delta commit; with no partition over a table of tombstones; stand-alone over a table without rows and on pod-axis shards), and the wide tables through two of their consumers."""
import numpy as np
import pytest

from modelmesh_amd.solver import Solver
from oracle import bind as ob
from oracle.bind import unpack_bitmap
from tests import ref_fleets as rf
from tests import ref_type_edges as te
from tests import type_edge_helpers as h
from tests.test_ref_vectors import STAT_FIELDS, check_type_tables
from tests.type_edge_helpers import CASES, NAMES

pytestmark = pytest.mark.gpu

LABEL_NAMES = [f"l{i:02d}" for i in range(64)]
STATS_NAMES = h.tier_names("stats")
BASES = [n for n in STATS_NAMES if CASES[n][6]["after"]]
SHARDED = [f"type_edges_stats_wide_{T}" for T in te.WIDE_T] + ["type_edges_stats_many_513"]
WIDE_CONSUMED = ("type_edges_stats_wide_64", "type_edges_stats_wide_128")  # 65 and 129 type rows


@pytest.fixture(scope="module")
def ref():
    return h.load()


def device_tables(al, pf, ha, hp, P):
    A, F = unpack_bitmap(al, P).astype(bool), unpack_bitmap(pf, P).astype(bool)
    return lambda t: (set(np.nonzero(A[t])[0].tolist()) if ha[t] else None, set(np.nonzero(F[t])[0].tolist()) if hp[t] else None)


def read_back(s, T):
    """mmp_pod_partitions, mmp_partition_count, mmp_partition_stats with every word, mmp_type_stats of every row, mmp_cluster_stats"""
    pts, parts = s.partitions()
    parts = [(tuple(int(st[x]) for x in STAT_FIELDS), frozenset(t for t in range(T + 1) if (pr >> t) & 1)) for st, pr in parts]
    g = tuple(int(s.stats()[x]) for x in STAT_FIELDS)
    ts = [tuple(int(s.type_stats(t)[x]) for x in STAT_FIELDS) for t in range(T + 1)]
    return (pts, parts), (lambda t: g if t is None else ts[t]), g


def check_rows(name, ref, route, al, pf, ha, hp):
    """rows 0 ... T word for word: has_allowed, has_prefer, the allowed and the preferred bitmap (zero where the set is null)"""
    rows = ref[f"{name}/rows"]
    W = (rows.shape[1] - 2) // 2
    assert np.array_equal(ha, rows[:, 0]) and np.array_equal(hp, rows[:, 1]), (name, route, ha, rows[:, 0], hp, rows[:, 1])
    assert np.array_equal(np.asarray(al, np.uint64), rows[:, 2: 2 + W].astype(np.uint64)), (name, route, "allowed")
    assert np.array_equal(np.asarray(pf, np.uint64), rows[:, 2 + W:].astype(np.uint64)), (name, route, "preferred")


def commit_and_check(name, ref, s, fleet, T, tables, route):
    s.load_replaced_rs(fleet.replaced_rs)
    s.load_models(fleet.models, fleet.ent_pod, fleet.ent_time)
    s.commit()
    partitions, type_stats, g = read_back(s, T)
    check_type_tables(name, ref, fleet, T, tables, partitions, type_stats)
    want = ob.OracleFleet(fleet).stats()
    assert g == tuple(int(want[x]) for x in STAT_FIELDS), (name, route, "cluster stats")
    n_parts = len(ref[f"{name}/part_types_len"])
    assert len(partitions[1]) == n_parts, (name, route)
    return partitions, type_stats


@pytest.mark.parametrize("name", NAMES)
def test_label_routes_commit_and_read_back(ref, name):
    """mmp_types_from_labels with the caller's words and mmp_types_from_pod_labels with the same words resident (behind
    mmp_label_names_load with 64 names and mmp_pod_labels_set), each followed by a commit and the read-back; then the reference's own
    tables through mmp_types_load and the same read-back."""
    _, fleet, ids, pod_bits, req, pref, meta = CASES[name]
    P, T = fleet.n_pods, len(req)
    for route in ("caller", "resident", "loaded"):
        s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
        try:
            if route == "resident":
                s.label_names_load(LABEL_NAMES)
            s.load_pods(fleet.pods)
            if route == "caller":
                al, pf, ha, hp = s.types_from_labels(req, pref, pod_bits)
            elif route == "resident":
                s.pod_labels_set(np.arange(P, dtype=np.int32), pod_bits, [bin(int(b)).count("1") for b in pod_bits])
                words, _ = s.pod_labels_get()
                assert np.array_equal(words, pod_bits), name
                al, pf, ha, hp = s.types_from_pod_labels(req, pref)
            else:
                f = h.with_tables(fleet, T, h.ref_tables(ref, name, P))
                al, pf, ha, hp = f.allowed, f.prefer, f.has_allowed, f.has_prefer
                s.load_types(T + 1, al, pf, ha, hp)
            check_rows(name, ref, route, al, pf, ha, hp)
            partitions, _ = commit_and_check(name, ref, s, fleet, T, device_tables(al, pf, ha, hp, P), route)
            if "n_parts" in meta:  # what ran: 513 and 600 partitions leave LDS (kPtsLds = 512)
                assert len(partitions[1]) == meta["n_parts"] and (len(partitions[1]) > 512) == (meta["n_parts"] in (513, 600)), name
            if "tw" in meta:
                assert (T + 1 + 63) // 64 == meta["tw"] == {62: 1, 63: 1, 64: 2, 127: 2, 128: 3}[T], name
        finally:
            s.close()


@pytest.mark.parametrize("name", BASES)
def test_after_tables_by_delta_commit_and_from_scratch(ref, name):
    """the twin in which six instances moved across a threshold: reached by mmp_pods_upsert + commit from the committed base, which
    re-ranks by insertion (delta_commits() == 1) wherever the table has two instances or more, and from scratch"""
    _, fleet, ids, pod_bits, req, pref, meta = CASES[name]
    after = meta["after"]
    f2 = CASES[after][1]
    P, T = fleet.n_pods, len(req)
    idx = np.array([p for p in range(P) if fleet.pods[p] != f2.pods[p]], np.int32)
    assert len(idx) == min(6, P), name
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    try:
        s.load_pods(fleet.pods)
        al, pf, ha, hp = s.types_from_labels(req, pref, pod_bits)
        tables = device_tables(al, pf, ha, hp, P)
        commit_and_check(name, ref, s, fleet, T, tables, "base")
        s.upsert_pods(idx, f2.pods[idx])
        s.commit()
        assert s.delta_commits() == (1 if P >= 2 else 0), (name, s.delta_commits())
        partitions, type_stats, g = read_back(s, T)
        check_type_tables(after, ref, f2, T, tables, partitions, type_stats)
        want = ob.OracleFleet(f2).stats()
        assert g == tuple(int(want[x]) for x in STAT_FIELDS), (after, "cluster stats after the delta commit", g)
    finally:
        s.close()
    s = Solver(f2.min_space_units, f2.min_churn_age_ms)
    try:
        s.load_pods(f2.pods)
        al, pf, ha, hp = s.types_from_labels(req, pref, pod_bits)
        check_rows(after, ref, "scratch", al, pf, ha, hp)
        commit_and_check(after, ref, s, f2, T, device_tables(al, pf, ha, hp, P), "scratch")
        assert s.delta_commits() == 0
    finally:
        s.close()


@pytest.mark.parametrize("name", [n for n in STATS_NAMES if "twin_of" not in CASES[n][6]])
def test_the_same_type_table_over_a_table_of_tombstones(ref, name):
    """every instance tombstoned.  The table still has its rows (P > 0), so the commit runs the kernels fused into it, with no
    partition (NP = 0) — NOT the stand-alone launch_subset_stats, which a commit takes only for a table without rows (below) and on
    a pod-axis shard.  No partition; every type's stats are empty with lru Long.MAX_VALUE.  Held to oracle.bind."""
    _, fleet, ids, pod_bits, req, pref, meta = CASES[name]
    P, T = fleet.n_pods, len(req)
    f = h.with_tables(fleet, T, h.ref_tables(ref, name, P))
    f.pods = fleet.pods.copy()
    f.pods["flags"] = 4
    s = Solver(f.min_space_units, f.min_churn_age_ms)
    try:
        s.load_fleet(f)
        (pts, parts), type_stats, g = read_back(s, T)
        assert len(parts) == 0 and (pts < 0).all(), name
        want_g = ob.OracleFleet(f).stats()
        assert g == tuple(int(want_g[x]) for x in STAT_FIELDS) == (0, 0, 2**63 - 1, 0, 0), (name, g)
        tss = ob.type_set_stats(f)
        for t in range(T + 1):
            assert type_stats(t) == tuple(int(tss[t][x]) for x in STAT_FIELDS) == (0, 0, 2**63 - 1, 0, 0), (name, t, type_stats(t))
    finally:
        s.close()


@pytest.mark.parametrize("name", [f"type_edges_stats_wide_{T}" for T in te.WIDE_T] + ["type_edges_stats_items_base"])
def test_the_same_type_table_over_a_table_without_rows(ref, name):
    """mmp_pods_load with no row, the case's T + 1 type rows (no bitmap word: W = 0) through mmp_types_load, a commit: the one commit
    that takes the stand-alone launch_subset_stats.  With P == 0 it launches subset_stats_finish_kernel alone (256-thread blocks,
    NP = 0): no partition, no instance, and every type row — constrained or not — answers the empty cluster's stats,
    InstanceSetStatsTracker's EMPTY_STATS with lru Long.MAX_VALUE."""
    _, fleet, ids, pod_bits, req, pref, meta = CASES[name]
    T = len(req)
    rows = ref[f"{name}/rows"]
    ha, hp = rows[:, 0].astype(np.uint8), rows[:, 1].astype(np.uint8)
    assert ha.any() and (T + 1 + 63) // 64 == meta.get("tw", 1), name
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    try:
        s.load_pods(fleet.pods[:0])
        s.load_types(T + 1, np.zeros((T + 1, 0), np.uint64), np.zeros((T + 1, 0), np.uint64), ha, hp)
        s.load_models(fleet.models, fleet.ent_pod, fleet.ent_time)
        s.commit()
        (pts, parts), type_stats, g = read_back(s, T)
        assert len(parts) == 0 and len(pts) == 0, name
        assert g == (0, 0, 2**63 - 1, 0, 0), (name, g)
        for t in range(T + 1):
            assert type_stats(t) == (0, 0, 2**63 - 1, 0, 0), (name, t, type_stats(t))
    finally:
        s.close()


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("name", SHARDED)
def test_pod_axis_shards_hold_the_same_partitions_and_stats(ref, name, G):
    """the wide cases and the 513-partition case on a group of G pod-axis shards over the thread transport: the shard commit runs the
    stand-alone stats kernels (partition_stats_kernel and subset_stats_finish_kernel, 256-thread blocks: the only route on which
    they see a type-constraint case with instances) over the whole table, and every shard answers mmp_pod_partitions, mmp_partition_stats, mmp_type_stats
    and mmp_cluster_stats as the single context does (no shard refuses them)."""
    from tests.test_shard_edges_gpu import run_group
    _, fleet, ids, pod_bits, req, pref, meta = CASES[name]
    P, T = fleet.n_pods, len(req)
    tables = h.ref_tables(ref, name, P)
    f = h.with_tables(fleet, T, tables)
    res = run_group(f, G, lambda s, g: read_back(s, T))
    assert len(res) == G
    for g, (partitions, type_stats, gstats) in enumerate(res):
        check_type_tables(name, ref, fleet, T, tables, partitions, type_stats)
        want = ob.OracleFleet(f).stats()
        assert gstats == tuple(int(want[x]) for x in STAT_FIELDS), (name, G, g)


def consumer_fleet(ref, name):
    """a wide case with the reference's tables installed and a registry on it: per type row 0, 63, 64, 65 and T (the rows on either side
    of the type-word edges, and the row of unconfigured types) models without a copy (the reaper's candidates) and with two"""
    _, fleet, ids, pod_bits, req, pref, meta = CASES[name]
    P, T = fleet.n_pods, len(req)
    f = h.with_tables(fleet, T, h.ref_tables(ref, name, P))
    f.pods = fleet.pods.copy()
    types = sorted({t for t in (0, 63, 64, 65, T) if t <= T})
    rf._set_models(f, [(t, lp, ()) for t in types for lp in ((), (), (1, 2))])
    f.models["last_used"] = f.now - 1_000 * (1 + np.arange(len(f.models)))
    return f, T, types


@pytest.mark.parametrize("name", WIDE_CONSUMED)
def test_a_guard_batch_reads_the_wide_type_stats(ref, name):
    """mmp_gate_batch with models of type rows 0, 63, 64, 65 and T: loadLocal's sizing and the reload rule read typeSetStats(type),
    held to oracle.bind on the same fleet (tests/test_type_edges.py holds oracle.bind's stats to the reference on exactly this case)"""
    from tests.gate_helpers import oracle_gates
    f, T, types = consumer_fleet(ref, name)
    rng = np.random.default_rng(77)
    model = np.repeat(np.arange(f.n_models), 12)
    r, xp, xt, expl = rf._with_lists(rf._edge_rows(f, rng, model, rng.integers(0, f.n_pods, len(model))), [[]] * len(model), [[]] * len(model))
    r["size_hint"] = 0  # the estimate from the type's stats decides the initial size
    tss = ob.type_set_stats(f)
    # (row T and an unconstrained row share the cluster's stats: every other row has its own)
    assert len({tuple(int(tss[t][x]) for x in STAT_FIELDS) for t in types}) >= len(types) - 1, (name, "the rows' stats do not tell them apart")
    want = oracle_gates(f, r, xp, xt, expl, 450_000)
    s = Solver(f.min_space_units, f.min_churn_age_ms)
    try:
        s.load_fleet(f)
        got = s.gates(r, xp, xt, expl, f.now)
    finally:
        s.close()
    assert np.array_equal(got["bits"], want[:, 0].astype(np.uint32)), name
    sized = (got["bits"] & 32) == 0
    assert sized.sum() >= len(r) // 4 and np.array_equal(got["initial_size"][sized], want[sized, 1]), name
    by_type = {t: set(got["initial_size"][sized & (f.models["type"][model] == t)].tolist()) for t in types}
    assert len({frozenset(v) for v in by_type.values()}) >= 2, (name, by_type)


@pytest.mark.parametrize("name", WIDE_CONSUMED)
def test_the_proactive_plan_excludes_by_the_wide_prohibited_rows(ref, name):
    """mmp_proactive_plan_subset for the partitions that are prohibited nothing, row 63 alone and row 64 alone: held to oracle.bind; the
    candidates of type rows 63 / 64 are in the plan of every such partition but the one that prohibits their row"""
    f, T, types = consumer_fleet(ref, name)
    pts, sets, pst = ob.partition_stats(f)
    ks = {r: sets.index(frozenset(r)) for r in ((), (63,), (64,)) if frozenset(r) in sets}
    assert len(ks) == (3 if T >= 127 else 2), (name, ks)
    plans = {}
    s = Solver(f.min_space_units, f.min_churn_age_ms)
    try:
        s.load_fleet(f)
        _, parts = s.partitions()
        for r, k in ks.items():
            assert parts[k][1] == sum(1 << t for t in r), (name, r, "the device numbers the partitions as the oracle does")
            gm, gl, ginfo = s.proactive_plan(6400, f.now, f.n_models, partition=k)
            wm, wl_, winfo = ob.proactive_plan(f, 6400, f.now, f.n_models, partition=k)
            assert np.array_equal(gm, wm) and np.array_equal(gl, wl_), (name, r, gm, wm)
            assert all(int(ginfo[x]) == int(winfo[x]) for x in ginfo.dtype.names), (name, r, ginfo, winfo)
            plans[r] = {int(f.models["type"][m]) for m in gm}
    finally:
        s.close()
    assert {63, 64} <= plans[()] and 63 not in plans[(63,)] and 64 in plans[(63,)], (name, plans)
    if (64,) in plans:
        assert 64 not in plans[(64,)] and 63 in plans[(64,)], (name, plans)


def test_load_targets_with_an_empty_but_present_preferred_set(ref):
    """the default row of the all-negative case: has_prefer == 1 with a zero bitmap.  A handful of load-target requests for models of
    that row decide as OracleFleet.place decides them on the same tables, and as the reference's own getNext text did (the place
    mode of the harness over the same tables: empty_pref/place in the vectors)."""
    from tests.test_ref_vectors import check_place
    f, ids, reqs = te.empty_pref_place(ref)
    rows = ref[f"{te.EMPTY_PREF}/rows"]
    assert rows[-1][1] == 1 and not rows[-1][2:].any() and f.has_prefer[-1] == 1 and not f.prefer[-1].any()
    assert rf.digest(rf.input_blob(f, ids, reqs, None)) == bytes(ref["empty_pref/digest"]).decode()
    want = ob.OracleFleet(f).place(reqs, np.zeros(0, np.int32), f.now)
    s = Solver(f.min_space_units, f.min_churn_age_ms)
    try:
        s.load_fleet(f)
        got = s.place(reqs, None, f.now)
    finally:
        s.close()
    for x in ("chosen", "best", "n_candidates", "hash"):
        assert np.array_equal(got[x], want[x]), x
    check_place("empty_pref", f, reqs, got, ref["empty_pref/place"])
    assert (got["chosen"] >= 0).sum() >= 10
