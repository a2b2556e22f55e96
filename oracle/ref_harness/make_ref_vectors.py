#!/usr/bin/env python3
"""Generates tests/golden/ref_getnext.npz: what the REFERENCE'S OWN TEXT decides (oracle/_ref/ref_harness, built by
build.sh from /root/reference) on the fleets of tests/ref_fleets.py.  Run in the build container (the GPU box has no
reference tree and only reads the committed file).

Per load-target case: the clusterState iteration order, and per request (chosen, candidates.size(), survivors of the rpm
filter, audit hash of the shortlist).  Per serve-target case: (chosen, chosenTimeStamp).  Per guard case: (MMP_GATE_* bits,
loadLocal's initial size).  Plus a digest of each case's inputs.
tests/golden/ref_gate_edges.npz: the guard cases at the edges of their value domain (gate_edge_vectors below).
tests/golden/ref_place_edges.npz: the load-target cases at the edges of theirs (place_edge_vectors below).
tests/golden/ref_rebalance_edges.npz: the rate task, the janitor's scale-down and the reaper's proactive loads at the edges of theirs
(rebalance_edge_vectors below).
tests/golden/ref_type_edges.npz: TypeConstraintManager's static computation at the edges of its value domain (type_edge_vectors below).
usage: python oracle/ref_harness/make_ref_vectors.py [--gate-edges | --place-edges | --rebalance-edges | --serve-edges | --type-edges]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import ref_fleets as rf  # noqa: E402

# MMP_REF_HARNESS / MMP_REF_OUT: run another build of the harness (tools/ref_coverage.sh: the --coverage build) without
# touching the committed vectors
HARNESS = os.environ.get("MMP_REF_HARNESS") or os.path.join(ROOT, "oracle", "_ref", "ref_harness")
OUT = os.environ.get("MMP_REF_OUT") or os.path.join(ROOT, "tests", "golden", "ref_getnext.npz")
EDGE_OUT = os.environ.get("MMP_REF_EDGE_OUT") or os.path.join(ROOT, "tests", "golden", "ref_gate_edges.npz")
PLACE_EDGE_OUT = os.environ.get("MMP_REF_PLACE_EDGE_OUT") or os.path.join(ROOT, "tests", "golden", "ref_place_edges.npz")
REBALANCE_EDGE_OUT = os.environ.get("MMP_REF_REBALANCE_EDGE_OUT") or os.path.join(ROOT, "tests", "golden", "ref_rebalance_edges.npz")


def proactive_inputs(fleet, units, partitioned):
    """What the harness is GIVEN for a reaper run (rows a5 / a18 produce them in a mesh): the cluster's stats and, with type
    constraints, per ProhibitedTypeSet partition its stats, its prohibited type rows and its instances."""
    from oracle import bind as ob
    g = np.zeros(1, dtype=ob.ORC_STATS)
    g[0] = ob.OracleFleet(fleet).stats()
    if not partitioned:
        return units, g, np.zeros(0, dtype=ob.ORC_STATS), [], None
    pts, sets, pst = ob.partition_stats(fleet)
    return units, g, pst, [sorted(s) for s in sets], pts


def run(blob: bytes, n_place: int, n_serve: int, n_gate: int = 0, n_scale: int = -1, n_pods: int = 0, n_sd: int = -1, proactive: bool = False,
        events: bool = False, upgrade: int = -1, types=None, migration: int = -1, conc: bool = False, env=None):
    """env: one of the harness' CONTEXT switches (harness.cc: MMP_REF_EXC_CONTEXT, MMP_REF_SEND_DEST, MMP_REF_MIGRATION_FAULTS) for
    a second pass over a case: state around the decision that the reference's text consults for side effects only."""
    with tempfile.TemporaryDirectory() as td:
        fin, fout = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        open(fin, "wb").write(blob)
        subprocess.run([HARNESS, fin, fout], check=True, env=dict(os.environ, **env) if env else None)
        raw = open(fout, "rb").read()
    n_present = int(np.frombuffer(raw, "<i8", 1)[0])
    off = 8
    order = np.frombuffer(raw, "<i4", n_present, off).copy()
    off += 4 * n_present
    place = np.frombuffer(raw, "<i4", 4 * n_place, off).reshape(n_place, 4).copy()
    off += 16 * n_place
    serve = np.frombuffer(raw, "<i8", 2 * n_serve, off).reshape(n_serve, 2).copy()
    off += 16 * n_serve
    gate = np.frombuffer(raw, "<i4", 2 * n_gate, off).reshape(n_gate, 2).copy()
    off += 8 * n_gate
    if migration >= 0:
        bits = np.frombuffer(raw, "u1", migration, off).copy()
        assert off + migration == len(raw)
        return bits
    if types is not None:  # (T, P): see harness.cc "a18"
        T, P = types
        W = (P + 63) // 64
        w = np.frombuffer(raw, "<i8", (len(raw) - off) // 8, off)
        i = 0
        rows = np.zeros((T + 1, 2 + 2 * W), np.int64)
        for t in range(T + 1):
            rows[t] = w[i: i + 2 + 2 * W]
            i += 2 + 2 * W
        pod_part = w[i: i + P].copy()
        i += P
        n_part = int(w[i])
        i += 1
        part_types, part_stats = [], []
        for _ in range(n_part):
            k = int(w[i])
            part_types.append(w[i + 1: i + 1 + k].copy())
            part_stats.append(w[i + 1 + k: i + 6 + k].copy())
            i += 6 + k
        order = w[i: i + n_part].copy()
        i += n_part
        tstats = w[i: i + 6 * T].reshape(T, 6).copy()
        assert i + 6 * T == len(w)
        return rows, pod_part, part_types, np.array(part_stats).reshape(n_part, 5), order, tstats
    if upgrade >= 0:  # after every call: n, then n x (replica set, expiry)
        w = np.frombuffer(raw, "<i8", (len(raw) - off) // 8, off)
        maps, i = [], 0
        for _ in range(upgrade):
            n = int(w[i])
            maps.append(w[i + 1: i + 1 + 2 * n].reshape(n, 2).copy())
            i += 1 + 2 * n
        assert i == len(w)
        return maps
    if events:  # per checkpoint: 5 stats words, n, n instance indices (clusterState order); then 4 counters
        w = np.frombuffer(raw, "<i8", (len(raw) - off) // 8, off)
        n_ck, i = int(w[0]), 1
        stats, orders = [], []
        for _ in range(n_ck):
            stats.append(w[i: i + 5].copy())
            n = int(w[i + 5])
            orders.append(w[i + 6: i + 6 + n].astype(np.int32))
            i += 6 + n
        assert i + 4 == len(w)
        return np.array(stats).reshape(n_ck, 5), orders, w[i: i + 4].copy()
    if proactive:
        n_calls = int(np.frombuffer(raw, "<i8", 1, off)[0])
        calls = np.frombuffer(raw, "<i8", 3 * n_calls, off + 8).reshape(n_calls, 3).copy()
        assert off + 8 + 24 * n_calls == len(raw)
        return calls
    if n_sd >= 0:
        removed = np.frombuffer(raw, "u1", n_sd, off).copy()
        assert off + n_sd == len(raw)
        return removed
    if n_scale < 0:
        assert off == len(raw)
        return order, place, serve, gate
    scale = np.frombuffer(raw, "<i8", 6 * n_scale, off).reshape(n_scale, 6).copy()
    off += 48 * n_scale
    called = int(np.frombuffer(raw, "<i8", 1, off)[0])
    off += 8
    ov = np.frombuffer(raw, "u1", n_pods, off).copy()
    off += n_pods
    if conc:  # per entry (threshold, resets, priorSum, priorCount), then the bits of averageModelParallelism
        co = np.frombuffer(raw, "<i8", 4 * n_scale + 1, off).copy()
        assert off + 8 * (4 * n_scale + 1) == len(raw)
        return order, place, serve, gate, scale, called, ov, co[:-1].reshape(n_scale, 4), co[-1:].view(np.float64)
    assert off == len(raw)
    return order, place, serve, gate, scale, called, ov


GUARDS = ["goLocal", "failures", "locations", "notAllowed", "churn", "earlyReject", "reload", "publish"]


def gate_edge_vectors():
    """tests/golden/ref_gate_edges.npz: the guards at the edges of their value domain (tests/ref_fleets.py:gate_edge_cases).  A case
    that does not hold what it is there for is REFUSED: the assertions below read the inputs and the reference's own outputs."""
    from oracle import bind as ob
    out, names = {}, []
    tier_bits, tier_rows, tier_sizing = {}, {}, {}
    for name, fleet, ids, reqs, xp, xt, expl, expiry in rf.gate_edge_cases():
        tier = rf.gate_edge_tier(name)
        assert tier in rf.GATE_EDGE_TIERS and fleet.n_pods in (8, 24, 64, 65) and fleet.n_models <= 60 and len(reqs) <= 2000, name
        tstats = np.ascontiguousarray(ob.type_set_stats(fleet))
        blob = rf.input_blob(fleet, ids, gates=(reqs, xp, xt, expl, expiry, tstats))
        _, _, _, gate = run(blob, 0, 0, len(reqs))
        assert np.array_equal(run(blob, 0, 0, len(reqs), env={"MMP_REF_EXC_CONTEXT": "1"})[3], gate), name
        bits = gate[:, 0].astype(np.uint32)
        sized = (bits & 32) == 0
        assert sized.mean() >= 0.5, (name, "the initial size is observable in fewer than half of the rows", sized.mean())
        if tier == "timed":
            want = {(x, e, k) for x in (False, True) for e in (False, True) for k in ("equal", "off", "any")}
            assert rf.timed_combinations(fleet, reqs, xp, xt) == want, name
            # ... and they decide: the same rows with every exclusion's time erased (a key exclude) go another way somewhere
            any_time = np.full(len(xt), rf._lib.ANY_TIME, np.int64)
            g2 = run(rf.input_blob(fleet, ids, gates=(reqs, xp, any_time, expl, expiry, tstats)), 0, 0, len(reqs))[3]
            assert ((g2[:, 0] ^ gate[:, 0]) & 1).sum() >= 20, (name, "the exclusions' times decide too few rows")
        outcome = rf.sizing_outcomes(fleet, reqs, tstats)
        seen = tier_sizing.setdefault(tier, {})
        for i in np.nonzero(sized)[0]:
            q, o, v = reqs[i], outcome[i], int(gate[i, 1])
            if o is None:
                assert v == q["loader_predicted"], (name, i)
                continue
            ok = {"hint": v == q["size_hint"], "negative estimate": v < -1, "positive estimate": v > 0, "estimate -1": v == -1,
                  "estimate 0: loader_predicted": v == q["loader_predicted"]}[o]
            assert ok, (name, int(i), o, v)
            seen[o] = seen.get(o, 0) + 1
        if tier == "totals":
            eng = [int(s["total_capacity"] - s["total_free"]) for s in tstats[1:10]]
            c = int(tstats[1]["model_copy_count"])
            assert eng == [2**31 - 1, 2**31, 2**31 + 5, 2**32 - 2 * c, 2**32 - c - 1, 2**32 - 1, 2**32, 2**32 + 99, 10**10], (name, eng)
            assert all(int(s["model_copy_count"]) == c for s in tstats[1:]), name
            assert [int(s["instance_count"]) for s in tstats[10:13]] == [1, 2, 2], name
            assert 20 * int(tstats[10]["total_free"]) == int(tstats[10]["total_capacity"]), name
            assert 20 * int(tstats[11]["total_free"]) == int(tstats[11]["total_capacity"]), name
            assert 20 * int(tstats[12]["total_free"]) == int(tstats[12]["total_capacity"]) - 1, name
        tier_bits.setdefault(tier, []).append(bits)
        tier_rows[tier] = tier_rows.get(tier, 0) + len(reqs)
        out[f"{name}/gate"] = gate
        out[f"{name}/digest"] = np.frombuffer(rf.digest(blob).encode(), np.uint8)
        names.append(name)
        print(f"{name}: {len(reqs)} guard evaluations, {100 * sized.mean():.0f} % sized; fired: " +
              " ".join(f"{b}:{int(((bits >> k) & 1).sum())}" for k, b in enumerate(GUARDS)))
    for tier in rf.GATE_EDGE_TIERS:
        bits = np.concatenate(tier_bits[tier])
        assert int(np.bitwise_or.reduce(bits)) == 255 and int(np.bitwise_and.reduce(bits)) == 0, (tier, "a guard bit is never set or never clear")
        print(f"tier {tier}: {tier_rows[tier]} rows; sizing outcomes among the sized rows: {tier_sizing[tier]}")
    assert all(tier_sizing["totals"].get(o, 0) > 0 for o in rf.SIZING_OUTCOMES), tier_sizing["totals"]
    out["names"] = np.array(names)
    np.savez_compressed(EDGE_OUT, **out)
    print(f"wrote {EDGE_OUT}: {os.path.getsize(EDGE_OUT) / 1e6:.2f} MB, {len(names)} cases")


def place_edge_vectors():
    """tests/golden/ref_place_edges.npz: getNext at the edges of its value domain (tests/ref_fleets.py:place_edge_cases).  As above, a
    case that does not hold what it is there for is REFUSED, on the evidence of the inputs and the reference's own outputs."""
    out, names = {}, []
    seen = {t: dict(rows=0, pairs=0, outcomes=set(), sizes=set(), kinds=set(), rpm={}) for t in rf.PLACE_EDGE_TIERS}
    orders = {}
    for name, fleet, ids, reqs, extra in rf.place_edge_cases():
        tier, meta = rf.place_edge_tier(name), rf.place_edge_meta(name)
        assert tier in rf.PLACE_EDGE_TIERS and fleet.n_pods in (8, 64, 65, 200, 700) and 0 < len(reqs) <= 3000, name
        blob = rf.input_blob(fleet, ids, reqs, extra)
        order, place, _, _ = run(blob, len(reqs), 0)
        for a, b, off in meta["pairs"]:  # one row inside, one outside a threshold: the reference must decide them differently
            if off == 0:  # the same first instance: the same walk but for the threshold
                assert not np.array_equal(place[a, :3], place[b, :3]), (name, "the reference decides a pair alike", a, b, place[a], place[b], reqs[a], reqs[b])
            else:  # first instances `off` positions apart: lists of different length anyway — they must END at different instances
                assert place[a, 1] > 0 and place[b, 1] > 0 and place[a, 1] != place[b, 1] + off, \
                    (name, "the two lists of a pair end at the same instance", a, b, off, place[a], place[b])
        if meta["caller"]:
            for f in rf._lib.PLACE_CALLER.names:
                assert np.all(reqs[f] == reqs[f][0]), (name, "not one caller's batch", f)
            assert len(meta["pairs"]) > 0 or tier == "order", name  # (the order tier is about the table: it has no pairs)
        st = seen[tier]
        st["rows"] += len(reqs)
        st["pairs"] += len(meta["pairs"])
        st["outcomes"] |= {"remote" if c >= 0 else "self" if c == -2 else "none" for c in place[:, 0]}
        st["sizes"] |= set(int(n) for n in place[:, 1])
        st["kinds"] |= set(rf.place_row_kinds(fleet, order, reqs, extra))
        for i in np.nonzero(place[:, 1] >= 2)[0]:
            gone = int(place[i, 1] - place[i, 2])
            how = "0" if gone == 0 else "all but one" if gone == place[i, 1] - 1 else "some"
            st["rpm"].setdefault(rf.rpm_class(fleet, int(reqs["last_used"][i])), {}).setdefault(how, 0)
            st["rpm"][rf.rpm_class(fleet, int(reqs["last_used"][i]))][how] += 1
        orders[name] = order
        out[f"{name}/order"], out[f"{name}/place"] = order, place
        out[f"{name}/digest"] = np.frombuffer(rf.digest(blob).encode(), np.uint8)
        names.append(name)
        print(f"{name}: {len(order)} instances, {len(reqs)} decisions, {len(meta['pairs'])} pairs: "
              f"{int((place[:, 0] >= 0).sum())} remote, {int((place[:, 0] == -2).sum())} self, {int((place[:, 0] == -1).sum())} none; "
              f"shortlists {int(place[:, 1].min())} ... {int(place[:, 1].max())}")
    assert len(names) <= 16
    for tier in rf.PLACE_EDGE_TIERS:
        assert any(rf.place_edge_meta(n)["caller"] for n in names if rf.place_edge_tier(n) == tier), (tier, "no one-caller case")
    for name in names:
        after = rf.place_edge_meta(name)["after"]
        if after is not None:
            assert not np.array_equal(orders[name], orders[after]), (name, "the changed rows do not move in the order")
    for tier in rf.PLACE_EDGE_TIERS:
        st = seen[tier]
        assert st["outcomes"] == {"remote", "self", "none"}, (tier, st["outcomes"])
        print(f"tier {tier}: {st['rows']} rows, {st['pairs']} pairs; kinds " + ", ".join(sorted(f"{k}{' (full)' if f else ''}" for k, f in st["kinds"])) +
              f"; shortlists of 1: {1 in st['sizes']}, of >= 65: {max(st['sizes']) >= 65}; filtered by rpm class: " +
              "; ".join(f"{c} {st['rpm'].get(c, {})}" for c in rf.RPM_CLASSES))
    sizes = set().union(*(seen[t]["sizes"] for t in rf.PLACE_EDGE_TIERS))
    assert 1 in sizes and max(sizes) >= 65, sizes
    # case (a) exists only with a first instance that is not full and case (b) only with a full one (:4828); the simple case in both
    assert seen["breaks"]["kinds"] >= {("simple", False), ("simple", True), ("a found", False), ("a replay", False), ("b found", True),
                                       ("b replay", True), ("none", False)}, seen["breaks"]["kinds"]
    assert {("simple", True), ("b found", True)} <= seen["rpm"]["kinds"], seen["rpm"]["kinds"]
    for c in rf.RPM_CLASSES[:4]:  # beyond a day no clause applies (:4972): class `none` filters nothing
        assert set(seen["rpm"]["rpm"].get(c, {})) == {"0", "some", "all but one"}, (c, seen["rpm"]["rpm"].get(c))
    assert set(seen["rpm"]["rpm"]["none"]) == {"0"}, seen["rpm"]["rpm"]["none"]
    out["names"] = np.array(names)
    np.savez_compressed(PLACE_EDGE_OUT, **out)
    print(f"wrote {PLACE_EDGE_OUT}: {os.path.getsize(PLACE_EDGE_OUT) / 1e3:.0f} kB, {len(names)} cases")


def run_rebalance(tier, case, blob):
    """One rebalance edge case through the harness -> {field: array}: rate: scale (action, copies, timestamp, i1, i2, heavy per entry),
    overloaded, exclude_set_built, with MaxConcCacheEntry rows also conc + average_model_parallelism; janitor: removed; plan: proactive."""
    fleet = case[0]
    if tier == "rate":
        n, latency = len(case[2]), case[3] is not None
        got = run(blob, 0, 0, 0, n, fleet.n_pods, conc=latency)
        out = dict(scale=got[4], exclude_set_built=np.array([got[5]]), overloaded=got[6])
        if latency:
            out["conc"], out["average_model_parallelism"] = got[7], got[8]
        return out
    if tier == "janitor":
        return dict(removed=run(blob, 0, 0, 0, -1, 0, len(case[2])))
    return dict(proactive=run(blob, 0, 0, proactive=True))


def rebalance_answer(tier, out, row):
    """What the reference answered for one row of a case (row -1: for the run as a whole)."""
    if tier == "rate":
        a = out["scale"] if row < 0 else out["scale"][row]
        if "conc" in out:
            a = np.concatenate([np.ravel(a), np.ravel(out["conc"] if row < 0 else out["conc"][row])])
        return np.ravel(a)
    if tier == "janitor":
        return np.ravel(out["removed"] if row < 0 else out["removed"][row])
    calls = out["proactive"]
    return np.ravel(calls[:, :2]) if row < 0 else np.array([int(np.any(calls[:, 0] == row))])


def rebalance_throws(tier, case):
    """The rows on which the Java would throw, from the inputs alone (the harness is C++ and traps there): a reason, or None."""
    from oracle import bind as ob
    fleet = case[0]
    if tier == "rate":
        sp = case[4]
        if int(sp["now"][0]) == int(sp["last_check_time"][0]):
            return "timeDelta == 0"
        if case[3] is None and int(sp["scale_up_rpm_threshold"][0]) == 0:
            return "scaleUpRpms == 0"
        rows = list(ob.type_set_stats(fleet)) + [ob.OracleFleet(fleet).stats()]
        if any(int(s["instance_count"]) >= 2 and int(s["total_capacity"]) == 0 for s in rows):
            return "totalCapacity == 0 at the fullness clause"
        return None
    if tier == "janitor":
        dp = case[4]
        return "timeSinceLastCheck == 0" if int(dp["now"][0]) == int(dp["last_check_time"][0]) else None
    units, partitioned = case[2], case[3]
    stats = list(ob.partition_stats(fleet)[2]) if partitioned else [ob.OracleFleet(fleet).stats()]
    for s in stats:
        tc, tf, c = int(s["total_capacity"]), int(s["total_free"]), int(s["model_copy_count"])
        if tc > 0 and tf > 0 and c >= 3:
            avg = rf._tdiv(rf._i32(tc - tf), c)
            if (avg if c > 10 else rf._tdiv(rf._i32(avg + units), 2)) == 0:
                return "sizeEstimate == 0"
        if tc > 0 and tf > 0 and c < 3 and units == 0:
            return "sizeEstimate == 0"
    return None


def rebalance_edge_vectors():
    """tests/golden/ref_rebalance_edges.npz: the rate task, the janitor's scale-down and the reaper's proactive loads at the edges of
    their value domain (tests/ref_fleets.py:rebalance_edge_cases).  A case that does not hold what it is there for is REFUSED, on
    the evidence of the inputs and the reference's own outputs: both rows of every pair must be answered differently."""
    out, names, outs, tiers = {}, [], {}, {}
    seen = {t: dict(cases=0, rows=0, pairs=0, run_pairs=0, sizes=set(), lens=set(), what={}) for t in rf.REBALANCE_EDGE_TIERS}

    def count(tier, what, n=1):
        if n:
            seen[tier]["what"][what] = seen[tier]["what"].get(what, 0) + int(n)

    for name, tier, case in rf.rebalance_edge_cases():
        fleet, meta = case[0], case[-1]
        assert tier == rf.rebalance_edge_tier(name) and fleet.n_pods in (8, 64, 65) and fleet.n_models <= 600, name
        assert rebalance_throws(tier, case) is None, (name, rebalance_throws(tier, case))
        blob = rf.rebalance_blob(tier, case)
        got = run_rebalance(tier, case, blob)
        n_rows = fleet.n_models if tier == "plan" else len(case[2])
        assert 0 < n_rows <= 600, name
        for a, b, what in meta["pairs"]:
            assert not np.array_equal(rebalance_answer(tier, got, a), rebalance_answer(tier, got, b)), \
                (name, "the reference answers a pair alike", a, b, what, rebalance_answer(tier, got, a))
        st = seen[tier]
        st["cases"], st["rows"], st["pairs"] = st["cases"] + 1, st["rows"] + n_rows, st["pairs"] + len(meta["pairs"])
        st["sizes"].add(fleet.n_pods)
        st["lens"].add(n_rows)
        if tier == "rate":
            sc, sp = got["scale"], case[4]
            early = int(sp["now"][0] - sp["last_check_time"][0]) * 5 < int(sp["rate_check_interval_ms"][0]) * 3
            few = int((fleet.pods["flags"] & 5 == 0).sum()) < 2
            assert (early or few) == (not sc[:, 0].any() and np.array_equal(sc[:, 3:5], np.stack(
                [case[2]["earlier_use_iteration"], case[2]["last_used_iteration"]], 1))), (name, "an early return that leaves no trace")
            count(tier, "exit: timeDelta too short", early)
            count(tier, "exit: fewer than two instances", few and not early)
            for k, a in enumerate(("none", "second copy", "scale-up")):
                count(tier, a, (sc[:, 0] == k).sum())
            count(tier, "heavy", sc[:, 5].sum())
            count(tier, "markers moved", (sc[:, 4] != case[2]["last_used_iteration"]).sum())
            count(tier, "overloaded instances", got["overloaded"].sum())
            if "overloaded" in meta:
                assert sorted(np.flatnonzero(got["overloaded"])) == sorted(meta["overloaded"]), (name, np.flatnonzero(got["overloaded"]))
            if "conc" in got:
                count(tier, "counter resets", got["conc"][:, 1].sum())
                assert not np.any((got["conc"][:, 0] == 0) & (sc[:, 0] == 2)), (name, "scaleUpRpms == 0 reached")
        elif tier == "janitor":
            count(tier, "removed", got["removed"].sum())
            count(tier, "kept", (got["removed"] == 0).sum())
            count(tier, "exit: shutting down", int(case[4]["shutting_down"][0]))
        else:
            count(tier, "loads", len(got["proactive"]))
            count(tier, "runs without a load", len(got["proactive"]) == 0)
        for k, v in got.items():
            out[f"{name}/{k}"] = v
        out[f"{name}/pairs"] = np.array([(a, b) for a, b, _ in meta["pairs"]], np.int32).reshape(-1, 2)
        out[f"{name}/digest"] = np.frombuffer(rf.digest(blob).encode(), np.uint8)
        names.append(name)
        outs[name], tiers[name] = got, tier
        print(f"{name}: {fleet.n_pods} instances, {n_rows} rows, {len(meta['pairs'])} pairs")
    for a, ra, b, rb in rf.rebalance_run_pairs():  # the same row of two runs one unit apart
        assert tiers[a] == tiers[b] and not np.array_equal(rebalance_answer(tiers[a], outs[a], ra), rebalance_answer(tiers[b], outs[b], rb)), \
            ("the reference answers a pair of runs alike", a, ra, b, rb)
        seen[tiers[a]]["run_pairs"] += 1
    for tier in rf.REBALANCE_EDGE_TIERS:
        st = seen[tier]
        assert st["sizes"] >= ({8, 64, 65} if tier != "plan" else {8, 64}), (tier, st["sizes"])
        if tier != "plan":
            assert st["lens"] >= {255, 256, 257}, (tier, sorted(st["lens"]))
        print(f"tier {tier}: {st['cases']} cases, {st['rows']} rows, {st['pairs']} pairs of rows, {st['run_pairs']} pairs of runs; " +
              ", ".join(f"{k}: {v}" for k, v in sorted(st["what"].items())))
    w = seen["rate"]["what"]
    assert all(w.get(k, 0) > 0 for k in ("none", "second copy", "scale-up", "heavy", "exit: timeDelta too short", "exit: fewer than two instances",
                                         "overloaded instances", "counter resets")), w
    w = seen["janitor"]["what"]
    assert all(w.get(k, 0) > 0 for k in ("removed", "kept", "exit: shutting down")), w
    w = seen["plan"]["what"]
    assert all(w.get(k, 0) > 0 for k in ("loads", "runs without a load")), w
    out["names"] = np.array(names)
    out["run_pairs"] = np.array([f"{a}:{ra}:{b}:{rb}" for a, ra, b, rb in rf.rebalance_run_pairs()])
    np.savez_compressed(REBALANCE_EDGE_OUT, **out)
    print(f"wrote {REBALANCE_EDGE_OUT}: {os.path.getsize(REBALANCE_EDGE_OUT) / 1e3:.0f} kB, {len(names)} cases")


SERVE_EDGE_OUT = os.environ.get("MMP_REF_SERVE_EDGE_OUT") or os.path.join(ROOT, "tests", "golden", "ref_serve_edges.npz")


def serve_edge_vectors():
    """tests/golden/ref_serve_edges.npz: ForwardingLB.getNext on rf.serve_edge_cases().  Refused: a pair the reference decides
    alike in chosen and chosenTimeStamp, a case without each outcome and each branch of the loop."""
    out, names = {}, []
    n_rows = n_pairs = 0
    for name, fleet, ids, reqs, in_use, last_used, xp, xt, meta in rf.serve_edge_cases():
        blob = rf.input_blob(fleet, ids, serve=(reqs, in_use, last_used, xp, xt))
        _, _, serve, _ = run(blob, 0, len(reqs))
        for p in meta["pairs"]:
            if tuple(serve[p["a"]]) == tuple(serve[p["b"]]):
                sys.exit(f"{name}: pair '{meta['pair_names'][p['name']]}' is decided alike by the reference: refused")
        missing = [k for k, ok in rf.serve_edge_occurrence(fleet, reqs, xp, xt, serve).items() if not ok]
        if missing:
            sys.exit(f"{name}: does not occur: {missing}")
        out[f"{name}/serve"] = serve
        out[f"{name}/digest"] = np.frombuffer(rf.digest(blob).encode(), np.uint8)
        names.append(name)
        n_rows, n_pairs = n_rows + len(reqs), n_pairs + len(meta["pairs"])
        print(f"{name}: {fleet.n_pods} instances, {len(reqs)} rows, {len(meta['pairs'])} pairs: {int((serve[:, 0] >= 0).sum())} remote, "
              f"{int((serve[:, 0] == -2).sum())} self, {int((serve[:, 0] == -1).sum())} none")
    out["names"] = np.array(names)
    np.savez_compressed(SERVE_EDGE_OUT, **out)
    print(f"wrote {SERVE_EDGE_OUT}: {os.path.getsize(SERVE_EDGE_OUT) / 1e3:.0f} kB, {len(names)} cases, {n_rows} rows, {n_pairs} pairs")


TYPE_EDGE_OUT = os.environ.get("MMP_REF_TYPE_EDGE_OUT") or os.path.join(ROOT, "tests", "golden", "ref_type_edges.npz")


def type_edge_vectors():
    """tests/golden/ref_type_edges.npz: TypeConstraintManager's static computation on rf.type_edge_cases() (tests/ref_type_edges.py).
    Refused: a pair the reference answers alike in the field it is there for (a pair marked alike: one it answers differently there), a case or a
    tier without what it is there for — all on the evidence of the inputs and the reference's own output."""
    import time
    from tests import ref_type_edges as te
    out, names, metas, not_pinned = {}, [], {}, []
    seen = {t: dict(cases=0, rows=0, pairs=0, what=set()) for t in te.TYPE_EDGE_TIERS}
    slowest = (0.0, None)
    for name, fleet, ids, pod_bits, req_bits, pref_bits, meta in rf.type_edge_cases():
        tier, P, T = meta["tier"], fleet.n_pods, len(req_bits)
        W = (P + 63) // 64
        blob = rf.input_blob(fleet, ids, types=(pod_bits, req_bits, pref_bits))
        t0 = time.time()
        rows, pod_part, part_types, part_stats, order, tstats = run(blob, 0, 0, types=(T, P))
        slowest = max(slowest, (time.time() - t0, name))
        out[f"{name}/rows"], out[f"{name}/pod_part"], out[f"{name}/part_stats"] = rows, pod_part, part_stats
        out[f"{name}/part_types_len"] = np.array([len(x) for x in part_types], np.int32)
        out[f"{name}/part_types"] = np.concatenate(part_types) if part_types else np.zeros(0, np.int64)
        out[f"{name}/order"], out[f"{name}/tstats"] = order, tstats
        out[f"{name}/pairs"] = np.array([f"{k}:{a}:{b}:{w}:{f}" for k, a, b, w, f in meta["pairs"]])
        out[f"{name}/digest"] = np.frombuffer(rf.digest(blob).encode(), np.uint8)
        names.append(name)
        metas[name] = meta
        st = seen[tier]
        st["cases"], st["rows"], st["pairs"] = st["cases"] + 1, st["rows"] + T + 1, st["pairs"] + len(meta["pairs"])
        for kind, a, b, what, field in meta["pairs"]:  # ... in the ONE field the pair is there for
            ans = te.field_inst if kind == "inst" else te.field_type
            if ans(out, name, a, field) == ans(out, name, b, field):
                sys.exit(f"{name}: the reference answers pair {kind} {a} / {b} ({what}) alike in {field}: refused")
        for kind, a, b, what, field in meta["alike"]:
            ans = te.field_inst if kind == "inst" else te.field_type
            if ans(out, name, a, field) != ans(out, name, b, field):
                sys.exit(f"{name}: the reference answers pair {kind} {a} / {b} ({what}), marked alike, differently in {field}: refused")
            not_pinned.append(f"{name}:{kind}:{a}:{b}:{what}:{field}")
        sig = te.signatures(out, name)
        sets = lambda t, which: te.set_of(rows[t], W, which)  # noqa: E731
        present = [p for p in range(P) if not fleet.pods["flags"][p] & 5]
        assert [p for p in range(P) if pod_part[p] >= 0] == present, name
        if tier == "sets":
            for p in meta["absent"]:  # shutting down / tombstoned, and would match type 0: in no set, in no partition
                assert not any(te.answer_inst(out, name, p)[0]) and pod_part[p] < 0, (name, p, "an absent instance is in a set")
            s0 = te.sets_blocks(P)[0]
            assert {0, 62, P - 1} <= set(meta["engineered"]) and (P < 65 or {63, 64} <= set(meta["engineered"])), name
            assert s0 + 8 in sets(5, 0) and s0 + 8 not in (sets(5, 1) or set()), (name, "required and preferred: allowed, NOT preferred")
            assert s0 + 9 not in sets(5, 0) and s0 + 9 in sets(5, 1), (name, "preferred only: preferred and prohibited")
            assert rows[6][0] == 0 and sets(6, 1) == sets(T, 1), (name, "a type with neither constrains nothing")
            assert s0 + 1 not in sets(0, 0) and not any(te.answer_inst(out, name, s0 + 1)[0][0::2]), (name, "no label: allowed nowhere")
            if meta["with_all"]:
                assert s0 + 10 in sets(3, 0) and s0 + 11 not in sets(3, 0), name
                st["what"].add("an instance with all 64 labels")
            else:
                assert rows[7][0] == 1 and sets(7, 0) == set() and sets(7, 1), (name, "nobody meets it: empty, not null; configured preference")
                assert rows[8][0] == 1 and sets(8, 0) == set() and sets(8, 1) is None, name
                st["what"].add("a requirement nobody meets")
        elif tier == "infer":
            if meta["want"] is None:
                assert sets(meta["row"], 1) is None, (name, "the inference is not null", sets(meta["row"], 1))
            else:
                assert sets(meta["row"], 1) == set(meta["want"]), (name, sets(meta["row"], 1), meta["want"])
            st["what"].add(meta["item"] + (" EMPTY non-null" if meta["want"] == [] else ""))
            if meta["item"] == "configured":
                assert sets(meta["twin_row"], 1) == set(meta["twin_want"]) != sets(meta["row"], 1), (name, "inference would not differ")
                assert sets(meta["row"], 0) == sets(meta["twin_row"], 0)
            for t in range(T):  # no requirement, a configured preference: the DEFAULT preferred set (:709-710), whatever was configured
                if req_bits[t] == 0 and pref_bits[t] != 0:
                    assert rows[t][0] == 0 and sets(t, 1) == sets(T, 1), (name, t)
        else:
            if "n_parts" in meta:
                assert len(sig) == meta["n_parts"] == len(set(sig)), (name, len(sig))
            if "rows" in meta:
                assert meta["tw"] == {62: 1, 63: 1, 64: 2, 127: 2, 128: 3}[T], name
                for r in meta["rows"]:
                    assert frozenset([r]) in sig and frozenset() in sig, (name, "no pair of partitions that differ in row", r)
                assert all(s <= set(meta["rows"]) for s in sig), name
            if meta.get("variant") == "base" and "twin_of" not in meta:
                hosts = lambda t: [k for k in range(len(sig)) if t not in sig[k]]  # noqa: E731
                assert len(hosts(4)) == 1 and len(hosts(1)) == 0 and len(hosts(2)) == len(sig) == 4, name
                assert tuple(tstats[1]) == (1, 0, 0, 2**63 - 1, 0, 0), (name, tstats[1])
                by = {tuple(sorted(sig[k])): part_stats[k] for k in range(len(sig))}
                assert by[(1, 3, 4)][1] == by[(0, 1, 4)][1] and by[(1, 3, 4)][0] != by[(0, 1, 4)][0], (name, "equal totalFree, unequal capacity")
                assert by[(1,)][1] == te.MIN_SPACE, name
            if meta.get("variant") == "hostile" and "twin_of" not in meta:
                assert (part_stats[:, 0] < 0).any() and (part_stats[:, 4] < 0).any() and (tstats[:, 1] < 0).any() and (tstats[:, 5] < 0).any(), \
                    (name, "no sum wraps")
                assert fleet.pods["count"].min() >= 0 and fleet.pods["capacity"].min() >= 0 and fleet.pods["used"].min() >= 0
            if meta.get("variant") == "nolru" and "twin_of" not in meta:
                assert (part_stats[:, 2] == 2**63 - 1).all(), name
            st["what"].add(f"{len(sig)} partitions")
        print(f"{name}: {P} instances, {T} types, {len(sig)} partitions, {len(meta['pairs'])} pairs")
    for name in names:  # the twins: the same case after six instances moved
        if metas[name]["after"]:
            assert te.answer_case(out, name) != te.answer_case(out, metas[name]["after"]), (name, "the moved instances change nothing")
    run_pairs, alike = [], []
    for a, b, p, what, field, same in te.type_edge_run_pairs():
        if (te.field_case(out, a, field) == te.field_case(out, b, field)) != same:
            sys.exit(f"{a} / {b}: instance {p} ({what}) is answered {'differently' if same else 'alike'} in {field} by the reference: refused")
        (alike if same else run_pairs).append(f"{a}:{b}:{p}:{what}:{field}")
        seen[metas[a]["tier"]]["pairs"] += 0 if same else 1
    for t in te.TYPE_EDGE_TIERS:
        print(f"tier {t}: {seen[t]['cases']} cases, {seen[t]['rows']} type rows, {seen[t]['pairs']} pairs; " + ", ".join(sorted(seen[t]["what"])))
    assert seen["sets"]["what"] == {"an instance with all 64 labels", "a requirement nobody meets"}
    assert {"allneg EMPTY non-null", "tie44", "single", "configured", "t0", "p1", "w256"} <= seen["infer"]["what"], seen["infer"]["what"]
    assert {"1 partitions", "2 partitions", "512 partitions", "513 partitions", "600 partitions"} <= seen["stats"]["what"]
    alike = not_pinned + alike
    print(f"NOT pinned (answered alike, as they must be): {alike}")
    print(f"slowest case: {slowest[1]} {slowest[0]:.1f} s in the harness")
    # a preferred set that is EMPTY but present, in front of getNext (the place mode of the harness): has_prefer = 1 with a zero row
    rows = out[f"{te.EMPTY_PREF}/rows"]
    assert rows[-1][1] == 1 and not rows[-1][2:].any(), "the default row of the all-negative case is not empty and present"
    f, ids, reqs = te.empty_pref_place(out)
    blob = rf.input_blob(f, ids, reqs, None)
    _, place, _, _ = run(blob, len(reqs), 0)
    assert (place[:, 0] >= 0).sum() >= 10 and (place[:, 1] >= 2).any(), place
    out["empty_pref/place"], out["empty_pref/digest"] = place, np.frombuffer(rf.digest(blob).encode(), np.uint8)
    out["names"], out["run_pairs"], out["alike"] = np.array(names), np.array(run_pairs), np.array(alike)
    np.savez_compressed(TYPE_EDGE_OUT, **out)
    print(f"wrote {TYPE_EDGE_OUT}: {os.path.getsize(TYPE_EDGE_OUT) / 1e3:.0f} kB, {len(names)} cases")


REGISTRY_EDGE_OUT = os.environ.get("MMP_REF_REGISTRY_EDGE_OUT") or os.path.join(ROOT, "tests", "golden", "ref_registry_edges.npz")
REGISTRY_HARNESS = os.environ.get("MMP_REG_HARNESS") or os.path.join(ROOT, "oracle", "_ref", "registry_harness")


def save_npz_fixed(path, arrays):
    """an .npz whose bytes depend on the arrays alone: members in the order given, a fixed member time, deflate"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def registry_edge_vectors():
    """tests/golden/ref_registry_edges.npz: the janitor's cache and registry loops and pruneModelRegistry, the reference's own text
    (oracle/_ref/registry_harness), on the cases of tests/ref_registry_edges.py.  Refused: a pair the text answers alike in what it is
    there for (a pair marked alike: one it answers differently), a case or a tier in which a named exit does not occur, a case
    without its digest — all on the evidence of the inputs and the text's recorded calls."""
    import json
    from tests import ref_registry_edges as re_
    from tests import registry_prune_model as rp
    out, names, runs_of, inputs = {}, [], {}, {}
    seen = {t: dict(cases=0, rows=0, records=0, pairs=0, alike=0, exits={}) for t in re_.TIERS}
    for c in re_.cases():
        name, meta, fleet, reg = c["name"], c["meta"], c["fleet"], c["reg"]
        pods = fleet.pods
        if meta["kind"] == "janitor":
            text = re_.janitor_input(pods, reg, c["entries"], c["states"], c["prm"])
        else:
            text = re_.prune_input(pods, reg, meta["self_pod"], meta["runs"])
        res = subprocess.run([REGISTRY_HARNESS], input=text.encode(), stdout=subprocess.PIPE, check=True)
        parsed = re_.parse(res.stdout.decode(), pods)
        assert len(parsed) == (1 if meta["kind"] == "janitor" else len(meta["runs"])), name
        out[f"{name}/pods"] = pods
        out[f"{name}/models"], out[f"{name}/ent_pod"], out[f"{name}/ent_time"] = rp.registry_to_arrays(reg)
        if meta["kind"] == "janitor":
            out[f"{name}/entries"], out[f"{name}/states"], out[f"{name}/prm"] = c["entries"], c["states"], c["prm"]
        for k, run in enumerate(parsed):
            for key, arr in re_.pack_run(run, c.get("entries")).items():
                out[f"{name}/r{k}/{key}"] = arr
        out[f"{name}/meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
        out[f"{name}/digest"] = np.frombuffer(re_.digest(text).encode(), np.uint8)
        names.append(name)
        inputs[name] = c
    save_npz_fixed(REGISTRY_EDGE_OUT, dict(out, names=np.array(names)))
    z = np.load(REGISTRY_EDGE_OUT)  # everything below reads what the file holds
    for name in names:
        c, meta = inputs[name], inputs[name]["meta"]
        st = seen[meta["tier"]]
        reg = rp.registry_from_arrays(z[f"{name}/models"], z[f"{name}/ent_pod"], z[f"{name}/ent_time"])
        if f"{name}/digest" not in z.files:
            sys.exit(f"{name}: no digest: refused")
        st["cases"], st["records"] = st["cases"] + 1, st["records"] + len(reg)
        if meta["kind"] == "janitor":
            run, entries, prm = re_.Run(z, f"{name}/r0/"), z[f"{name}/entries"], z[f"{name}/prm"]
            runs_of[name] = (run, entries, reg)
            st["rows"] += len(entries)
            for kind, a, b, what in meta["pairs"]:
                if re_.answer(run, entries, kind, a, reg) == re_.answer(run, entries, kind, b, reg):
                    sys.exit(f"{name}: the text answers pair {kind} {a} / {b} ({what}) alike: refused")
            for kind, a, b, what in meta["alike"]:
                if re_.answer(run, entries, kind, a, reg) != re_.answer(run, entries, kind, b, reg):
                    sys.exit(f"{name}: the text answers pair {kind} {a} / {b} ({what}), marked alike, differently: refused")
            st["pairs"], st["alike"] = st["pairs"] + len(meta["pairs"]), st["alike"] + len(meta["alike"])
            shown = re_.exits_of(run, reg, entries, prm)
        else:
            runs = [re_.Run(z, f"{name}/r{k}/") for k in range(len(meta["runs"]))]
            runs_of[name] = (runs, None, reg)
            st["rows"] += len(runs)
            for want_same, pairs in ((False, meta["pairs"]), (True, meta["alike"])):
                for kind, a, b, what in pairs:
                    if (re_.prune_rec_answer(runs, reg, a) == re_.prune_rec_answer(runs, reg, b)) != want_same:
                        sys.exit(f"{name}: the text answers pair {kind} {a} / {b} ({what}) {'differently' if want_same else 'alike'}: refused")
            st["pairs"], st["alike"] = st["pairs"] + len(meta["pairs"]), st["alike"] + len(meta["alike"])
            shown = re_.prune_exits_of(runs, reg, meta) if meta["domain"] else set()
        missing = set(meta["exits"]) - shown
        if missing:
            sys.exit(f"{name}: the case does not show {sorted(missing)} (it shows {sorted(shown)}): refused")
        for e in shown:
            st["exits"][e] = st["exits"].get(e, 0) + 1
        print(f"{name}: {len(reg)} records, {len(z[name + '/entries']) if meta['kind'] == 'janitor' else len(meta['runs'])} rows / runs, "
              f"{len(meta['pairs'])} pairs, {len(meta['alike'])} alike; shows {sorted(shown)}")
    for a, b, kind, what, alike in re_.run_pairs():
        if kind == "row":
            at = inputs[b]["meta"]["stop_at"]
            same = re_.answer(*runs_of[a][:2], "row", at, runs_of[a][2]) == re_.answer(*runs_of[b][:2], "row", at, runs_of[b][2])
        else:
            same = re_.prune_answer(runs_of[a][0], runs_of[a][2], inputs[a]["meta"]) == re_.prune_answer(runs_of[b][0], runs_of[b][2], inputs[b]["meta"])
        if same != alike:
            sys.exit(f"{a} / {b} ({what}): the text answers them {'alike' if same else 'differently'}: refused")
        seen[inputs[a]["meta"]["tier"]]["alike" if alike else "pairs"] += 1
    for t in re_.TIERS:
        lacking = set(re_.TIER_EXITS[t]) - set(seen[t]["exits"])
        if lacking:
            sys.exit(f"tier {t}: no case shows {sorted(lacking)}: refused")
        s = seen[t]
        print(f"tier {t}: {s['cases']} cases, {s['records']} records, {s['rows']} cache rows / runs, {s['pairs']} pairs, {s['alike']} alike; exits " +
              ", ".join(f"{k} x{v}" for k, v in sorted(s["exits"].items())))
    print(f"wrote {REGISTRY_EDGE_OUT}: {os.path.getsize(REGISTRY_EDGE_OUT)} bytes, {len(names)} cases")


def main():
    if not os.environ.get("MMP_REF_HARNESS"):
        subprocess.run(["bash", os.path.join(ROOT, "oracle", "ref_harness", "build.sh")], check=True)
    if "--registry-edges" in sys.argv[1:]:  # only the janitor's loops and the registry prune
        return registry_edge_vectors()
    if "--type-edges" in sys.argv[1:]:  # only the type-constraint edge cases
        return type_edge_vectors()
    if "--gate-edges" in sys.argv[1:]:  # only the guard edge cases: ref_getnext.npz stays as it is
        return gate_edge_vectors()
    if "--place-edges" in sys.argv[1:]:  # only the load-target edge cases
        return place_edge_vectors()
    if "--serve-edges" in sys.argv[1:]:  # only the serve choice's edge cases
        return serve_edge_vectors()
    if "--rebalance-edges" in sys.argv[1:]:  # only the rebalancers' edge cases
        return rebalance_edge_vectors()
    out = {}
    names = []
    for name, fleet, ids, reqs, extra in rf.place_cases():
        blob = rf.input_blob(fleet, ids, reqs, extra)
        order, place, _, _ = run(blob, len(reqs), 0)
        if name in ("fuzz_None_3", "fuzz_prefer_5"):  # the same decisions with the destination id sent along (:4997-4999)
            o2, p2, _, _ = run(blob, len(reqs), 0, env={"MMP_REF_SEND_DEST": "1"})
            assert np.array_equal(o2, order) and np.array_equal(p2, place), name
        out[f"{name}/order"], out[f"{name}/place"] = order, place
        out[f"{name}/digest"] = np.frombuffer(rf.digest(blob).encode(), np.uint8)
        names.append(name)
        print(f"{name}: {len(order)} instances in clusterState, {len(reqs)} decisions: "
              f"{int((place[:, 0] >= 0).sum())} remote, {int((place[:, 0] == -2).sum())} self, {int((place[:, 0] == -1).sum())} none; "
              f"mean shortlist {place[:, 1].mean():.1f}")
    for name, fleet, ids, reqs, extra in rf.caller_place_cases():
        blob = rf.input_blob(fleet, ids, reqs, extra)
        order, place, _, _ = run(blob, len(reqs), 0)
        out[f"{name}/order"], out[f"{name}/place"] = order, place
        out[f"{name}/digest"] = np.frombuffer(rf.digest(blob).encode(), np.uint8)
        names.append(name)
        print(f"{name}: one caller (instance {int(reqs['self_pod'][0])}), {len(reqs)} decisions: "
              f"{int((place[:, 0] >= 0).sum())} remote, {int((place[:, 0] == -2).sum())} self, {int((place[:, 0] == -1).sum())} none; "
              f"mean shortlist {place[:, 1].mean():.1f}")
    for name, fleet, ids, reqs, in_use, last_used, xp, xt in rf.serve_cases():
        blob = rf.input_blob(fleet, ids, serve=(reqs, in_use, last_used, xp, xt))
        _, _, serve, _ = run(blob, 0, len(reqs))
        if name.endswith("_0"):  # ... and the serve target's (:4386-4388)
            assert np.array_equal(run(blob, 0, len(reqs), env={"MMP_REF_SEND_DEST": "1"})[2], serve), name
        out[f"{name}/serve"] = serve
        out[f"{name}/digest"] = np.frombuffer(rf.digest(blob).encode(), np.uint8)
        names.append(name)
        print(f"{name}: {len(reqs)} serve decisions: {int((serve[:, 0] >= 0).sum())} remote, {int((serve[:, 0] == -2).sum())} self")
    from oracle import bind as ob
    for name, fleet, ids, reqs, xp, xt, expl, expiry in rf.gate_cases():
        tstats = np.ascontiguousarray(ob.type_set_stats(fleet))  # an INPUT of the guards (rows a5 / a18 are pinned separately)
        blob = rf.input_blob(fleet, ids, gates=(reqs, xp, xt, expl, expiry, tstats))
        _, _, _, gate = run(blob, 0, 0, len(reqs))
        # which exception flies when a guard refuses (one seen earlier in the request, or a new one: :4019-4031, :4598-4601,
        # :4618-4621) is not part of the decision: the same bits with failures "seen before" and for internal requests
        assert np.array_equal(run(blob, 0, 0, len(reqs), env={"MMP_REF_EXC_CONTEXT": "1"})[3], gate), name
        out[f"{name}/gate"] = gate
        out[f"{name}/digest"] = np.frombuffer(rf.digest(blob).encode(), np.uint8)
        names.append(name)
        bits = gate[:, 0].astype(np.uint32)
        print(f"{name}: {len(reqs)} guard evaluations; fired: " + " ".join(f"{b}:{int(((bits >> k) & 1).sum())}" for k, b in enumerate(
            ["goLocal", "failures", "locations", "notAllowed", "churn", "earlyReject", "reload", "publish"])))
    for name, fleet, ids, entries, sp in rf.scaleup_cases():
        cstats = np.zeros(1, dtype=ob.ORC_STATS)
        cstats[0] = ob.OracleFleet(fleet).stats()  # clusterStats / typeSetStats: INPUTS of the planner (rows a5 / a18)
        blob = rf.input_blob(fleet, ids, scaleup=(entries, sp, cstats, np.ascontiguousarray(ob.type_set_stats(fleet))))
        *_, scale, called, ov = run(blob, 0, 0, 0, len(entries), fleet.n_pods)
        out[f"{name}/scale"], out[f"{name}/overloaded"] = scale, ov
        out[f"{name}/exclude_set_built"] = np.array([called])
        out[f"{name}/digest"] = np.frombuffer(rf.digest(blob).encode(), np.uint8)
        names.append(name)
        print(f"{name}: {len(entries)} cache entries: {int((scale[:, 0] == 1).sum())} second copies, {int((scale[:, 0] == 2).sum())} scale-ups, "
              f"{int(scale[:, 5].sum())} heavy, {int(ov.sum())} overloaded instances")
    for name, fleet, ids, entries, sp in rf.scaleup_edge_cases():
        cstats = np.zeros(1, dtype=ob.ORC_STATS)
        cstats[0] = ob.OracleFleet(fleet).stats()
        blob = rf.input_blob(fleet, ids, scaleup=(entries, sp, cstats, np.ascontiguousarray(ob.type_set_stats(fleet))))
        *_, scale, called, ov = run(blob, 0, 0, 0, len(entries), fleet.n_pods)
        out[f"{name}/scale"], out[f"{name}/overloaded"] = scale, ov
        out[f"{name}/exclude_set_built"] = np.array([called])
        out[f"{name}/digest"] = np.frombuffer(rf.digest(blob).encode(), np.uint8)
        names.append(name)
        print(f"{name}: {len(entries)} cache entries: {int((scale[:, 0] == 1).sum())} second copies, {int((scale[:, 0] == 2).sum())} scale-ups, "
              f"{int(ov.sum())} overloaded instances, exclude set built: {called}")
    for name, fleet, ids, entries, conc, sp, cp in rf.scaleup_conc_cases():
        cstats = np.zeros(1, dtype=ob.ORC_STATS)
        cstats[0] = ob.OracleFleet(fleet).stats()
        blob = rf.input_blob(fleet, ids, scaleup=(entries, sp, cstats, np.ascontiguousarray(ob.type_set_stats(fleet))), conc=(conc, cp))
        *_, scale, called, ov, cout, avg = run(blob, 0, 0, 0, len(entries), fleet.n_pods, conc=True)
        out[f"{name}/scale"], out[f"{name}/overloaded"] = scale, ov
        out[f"{name}/exclude_set_built"] = np.array([called])
        out[f"{name}/conc"], out[f"{name}/average_model_parallelism"] = cout, avg
        out[f"{name}/digest"] = np.frombuffer(rf.digest(blob).encode(), np.uint8)
        names.append(name)
        print(f"{name}: {len(entries)} MaxConcCacheEntry entries: {int((scale[:, 0] == 1).sum())} second copies, {int((scale[:, 0] == 2).sum())} scale-ups, "
              f"{int(scale[:, 5].sum())} heavy, {int(cout[:, 1].sum())} counter resets, {len(np.unique(cout[:, 0]))} distinct thresholds, "
              f"{int(ov.sum())} overloaded instances; averageModelParallelism {float(cp['average_model_parallelism'][0])} -> {float(avg[0])!r}")
    for name, fleet, ids, entries, conc, dp, dyn in rf.scaledown_conc_cases():
        istats = ob.instance_set_stats(fleet, int(dp["self_pod"][0]))
        cp = np.zeros(1, dtype=rf._lib.CONC_PARAMS)
        cp["dynamic_rpm_scale_constant"], cp["average_model_parallelism"] = dyn, 1.0
        blob = rf.input_blob(fleet, ids, scaledown=(entries, dp, istats), conc=(conc, cp))
        removed = run(blob, 0, 0, 0, -1, 0, len(entries))
        out[f"{name}/removed"] = removed
        out[f"{name}/digest"] = np.frombuffer(rf.digest(blob).encode(), np.uint8)
        names.append(name)
        print(f"{name}: {len(entries)} MaxConcCacheEntry candidates: {int(removed.sum())} local copies removed")
    for name, fleet, ids, entries, dp in rf.scaledown_edge_cases():
        istats = ob.instance_set_stats(fleet, int(dp["self_pod"][0]))
        blob = rf.input_blob(fleet, ids, scaledown=(entries, dp, istats))
        removed = run(blob, 0, 0, 0, -1, 0, len(entries))
        out[f"{name}/removed"] = removed
        out[f"{name}/digest"] = np.frombuffer(rf.digest(blob).encode(), np.uint8)
        names.append(name)
        print(f"{name}: {len(entries)} candidates: {int(removed.sum())} local copies removed")
    for name, fleet, ids, entries, dp in rf.scaledown_cases():
        istats = ob.instance_set_stats(fleet, int(dp["self_pod"][0]))  # instanceSetStats(): an INPUT (rows a5 / a18)
        blob = rf.input_blob(fleet, ids, scaledown=(entries, dp, istats))
        removed = run(blob, 0, 0, 0, -1, 0, len(entries))
        out[f"{name}/removed"] = removed
        out[f"{name}/digest"] = np.frombuffer(rf.digest(blob).encode(), np.uint8)
        names.append(name)
        print(f"{name}: {len(entries)} candidates: {int(removed.sum())} local copies removed")
    for name, fleet, ids, units, partitioned in rf.proactive_cases():
        blob = rf.input_blob(fleet, ids, proactive=proactive_inputs(fleet, units, partitioned))
        calls = run(blob, 0, 0, proactive=True)
        out[f"{name}/proactive"] = calls
        out[f"{name}/digest"] = np.frombuffer(rf.digest(blob).encode(), np.uint8)
        names.append(name)
        print(f"{name}: {fleet.n_models} registry rows: {len(calls)} proactive loads over {len(np.unique(calls[:, 2])) if len(calls) else 0} instance subset(s)")
    for name, fleet, ids, ev, ck, tables in rf.table_event_cases():
        blob = rf.input_blob(fleet, ids, events=(ev, ck))
        stats, orders, counters = run(blob, 0, 0, events=True)
        assert len(orders) == len(tables)
        out[f"{name}/stats"] = stats
        out[f"{name}/order_len"] = np.array([len(o) for o in orders], np.int32)
        out[f"{name}/orders"] = np.concatenate(orders) if orders else np.zeros(0, np.int32)
        out[f"{name}/counters"] = counters
        out[f"{name}/digest"] = np.frombuffer(rf.digest(blob).encode(), np.uint8)
        names.append(name)
        print(f"{name}: {len(ev)} listener events, {len(orders)} checkpoints; upgradeTracker added/removed {counters[0]}/{counters[1]}, "
              f"housekeepings {counters[2]}")
    for name, fleet, ids, pod_bits, req_bits, pref_bits in rf.type_constraint_cases():
        blob = rf.input_blob(fleet, ids, types=(pod_bits, req_bits, pref_bits))
        rows, pod_part, part_types, part_stats, order, tstats = run(blob, 0, 0, types=(len(req_bits), fleet.n_pods))
        out[f"{name}/rows"], out[f"{name}/pod_part"], out[f"{name}/part_stats"] = rows, pod_part, part_stats
        out[f"{name}/part_types_len"] = np.array([len(x) for x in part_types], np.int32)
        out[f"{name}/part_types"] = np.concatenate(part_types) if part_types else np.zeros(0, np.int64)
        out[f"{name}/order"], out[f"{name}/tstats"] = order, tstats
        out[f"{name}/digest"] = np.frombuffer(rf.digest(blob).encode(), np.uint8)
        names.append(name)
        print(f"{name}: {len(req_bits)} types over {fleet.n_pods} instances: {len(part_types)} ProhibitedTypeSet partitions, "
              f"{int(rows[:-1, 0].sum())} types with requirements, {int(rows[:, 1].sum())} rows with preferred instances")
    for name, fleet, ids, entries, self_pod, now in rf.migration_cases():
        blob = rf.input_blob(fleet, ids, migration=(entries, self_pod, now))
        bits = run(blob, 0, 0, migration=len(entries))
        # aborted loads (deregistered at once, :7027-7030) and copies that fail to load elsewhere (:7033-7036): the same copies
        # are triggered; the shutdown does not wait for a copy that failed
        b2 = run(blob, 0, 0, migration=len(entries), env={"MMP_REF_MIGRATION_FAULTS": "1"})
        assert np.array_equal(b2 & 1, bits & 1) and np.all((b2 >> 1) <= (bits >> 1)) and (b2 >> 1).sum() < (bits >> 1).sum(), name
        out[f"{name}/migration"] = bits
        out[f"{name}/digest"] = np.frombuffer(rf.digest(blob).encode(), np.uint8)
        names.append(name)
        print(f"{name}: {len(entries)} cache entries: {int((bits & 1).sum())} copies triggered elsewhere, the shutdown waits for {int((bits >> 1).sum())}")
    small = rf.wl.fuzz_fleet(1, pods=4, models=4)  # the harness wants a fleet in every input; the tracker never looks at it
    small_ids = rf.string_ids(small, 1)
    for name, ev in rf.upgrade_event_cases():
        blob = rf.input_blob(small, small_ids, upgrade=ev)
        maps = run(blob, 0, 0, upgrade=len(ev))
        out[f"{name}/map_len"] = np.array([len(m) for m in maps], np.int32)
        out[f"{name}/maps"] = np.concatenate(maps) if maps else np.zeros((0, 2), np.int64)
        out[f"{name}/digest"] = np.frombuffer(rf.digest(blob).encode(), np.uint8)
        names.append(name)
        print(f"{name}: {len(ev)} tracker calls; the likely-replaced map is non-empty after {int((out[f'{name}/map_len'] > 0).sum())} of them, "
              f"up to {int(out[f'{name}/map_len'].max())} replica sets")
    out["names"] = np.array(names)
    out["manifest"] = np.array(open(os.path.join(ROOT, "oracle", "_ref", "gen", "MANIFEST.txt")).read())
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1e6:.2f} MB, {len(names)} cases")
    gate_edge_vectors()
    place_edge_vectors()
    rebalance_edge_vectors()


if __name__ == "__main__":
    main()
