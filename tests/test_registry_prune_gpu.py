"""mmp_registry_prune on the device against the Python restatement of pruneModelRegistry (tests/registry_prune_model.py):
edits, removed lists, every info field and the missing map, bit-exact over sequences of reaper runs; the resident registry
after an apply; the proactive plan, load-target and serve decisions that follow it without a commit; truncation, dry runs,
concurrency with decisions, the missing map's lifetime, and the JNI veneer."""
import copy
import threading
import time

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd import workload as wl
from modelmesh_amd.solver import MmpError, Solver
from oracle import bind as ob
from oracle.bind import OracleFleet
from tests import registry_prune_model as rp
from tests.registry_prune_model import GONE_AFTER_MS as GONE, LONG_MAX, REAPER_FREQ_MS, Reaper
from tests.util import assert_same_decisions

pytestmark = pytest.mark.gpu

INFO_FIELDS = ("n_edits", "n_removed", "n_repaired", "n_unresolved", "n_missing_pods", "n_new_missing", "truncated")


def prune_fleet(seed, pods, models, base=None):
    """The recipe: entry ages on both sides of gone-after, some ids not in the pod table (-1), 1 % Long.MAX records; and three
    groups of instances (~5 % of the table together) that leave at different times, so that before the first measured run a
    third of them holds a mark older than gone-after, a third a younger one and a third none."""
    rng = np.random.default_rng(77_000 + seed)
    fleet = base if base is not None else wl.fuzz_fleet(seed + 900, pods=pods, models=models)
    now, P, M = fleet.now, fleet.n_pods, fleet.n_models
    fleet.pods["flags"] = np.where(fleet.pods["flags"] & _lib.POD_TOMBSTONE, _lib.POD_LIVE, fleet.pods["flags"])  # all present first
    n_ent = len(fleet.ent_pod)
    fleet.ent_time = (now - rng.choice([1_000, GONE - 1, GONE, GONE + 1, 2 * GONE, 4 * GONE, 86_400_000], n_ent)).astype(np.int64)
    fleet.ent_pod = np.where(rng.random(n_ent) < 0.01, -1, fleet.ent_pod).astype(np.int32)
    fleet.models["last_used"] = np.where(rng.random(M) < 0.01, LONG_MAX, fleet.models["last_used"])
    gone = rng.choice(P, size=max(3, int(round(0.05 * P))), replace=False)
    groups = [np.sort(g).astype(np.int32) for g in np.array_split(gone, 3)]
    fleet.ent_pod[: min(3, n_ent)] = -1  # (tiny fleets: the 1 % may be empty)
    if M:
        fleet.models["last_used"][M // 2] = LONG_MAX
    return fleet, groups


def same_registry(s, reg):
    got = rp.compact(*s.get_models())
    want = rp.registry_to_arrays(reg)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def one_run(s, reaper, reg, self_pod, now, apply=True, **kw):
    """The same run on both sides; asserts every output equal; returns the restatement's (edits, removed, info, candidates)."""
    flags = s.get_pods()["flags"]  # (staged == committed: the callers commit before they run)
    e, rm, info = s.prune_registry(self_pod, now, apply=apply, **kw)
    # (apply=False: the map advances, the resident registry is the caller's to edit — here: it stays as it is)
    we, wrm, winfo, cand = reaper.run(flags, reg if apply else copy.deepcopy(reg), self_pod, now)
    print(f"run at {now}: device {dict((f, int(info[f])) for f in INFO_FIELDS)}  restatement {winfo}")
    assert np.array_equal(e, we), (e[:5], we[:5])
    assert np.array_equal(rm, wrm), (rm[:5], wrm[:5])
    for f in INFO_FIELDS:
        assert int(info[f]) == winfo[f], (f, info, winfo)
    assert s.missing_instances() == reaper.missings
    return we, wrm, winfo, cand


def seeded(fleet, groups, self_pod=0):
    """Solver + restatement after the two seeding runs: group 0 left at now - gone_after - 1 min (its mark is OLDER than
    gone-after at `now`), group 1 at now - gone_after / 2 (younger), group 2 has just left (no mark yet)."""
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    s.load_fleet(fleet)
    reg = rp.registry_from_arrays(fleet.models, fleet.ent_pod, fleet.ent_time)
    reaper = Reaper()
    for g, t in ((groups[0], fleet.now - GONE - 60_000), (groups[1], fleet.now - GONE // 2)):
        s.remove_pods(g)
        s.commit()
        e, _, _, _ = one_run(s, reaper, reg, self_pod, t, apply=False)  # (the registry keeps its Long.MAX records for the runs under test)
        assert len(e[e["n_removed"] > 0]) == 0  # first sightings only
    s.remove_pods(groups[2])
    s.commit()
    assert (s.get_pods()["flags"][np.concatenate(groups)] & _lib.POD_TOMBSTONE).all()
    old = sum(1 for v in reaper.missings.values() if fleet.now - v > GONE)
    young = len(reaper.missings) - old
    assert old >= 1 and young >= 1, (old, young)
    return s, reaper, reg


@pytest.mark.parametrize("seed,pods,models", [(0, 8, 300), (1, 40, 600), (2, 300, 2000), (3, 2000, 20000), (4, 10_000, 100_000)])
def test_four_runs_equal_the_restatement(seed, pods, models):
    base = wl.make_fleet("C3") if models == 100_000 else None
    fleet, groups = prune_fleet(seed, pods, models, base)
    assert (fleet.n_pods, fleet.n_models) == (pods, models)
    s, reaper, reg = seeded(fleet, groups)
    try:
        seen = dict(partial=0, freed=0, failed=0, first=0, unresolved=0, repaired=0)
        for run in range(4):
            now = fleet.now + run * REAPER_FREQ_MS
            e, rm, info, cand = one_run(s, reaper, reg, 0, now)
            cand = set(cand)
            for ed in e:
                if ed["n_removed"] and ed["n_loaded_after"] + ed["n_failed_after"] > 0:
                    seen["partial"] += 1
                if ed["n_removed"] and ed["n_loaded_after"] == 0 and int(ed["model"]) in cand and \
                        any(not x["failed"] for x in rm[ed["removed_off"]: ed["removed_off"] + ed["n_removed"]]):
                    seen["freed"] += 1
            seen["failed"] += int(rm["failed"].sum())
            seen["first"] += info["n_new_missing"]
            seen["unresolved"] += info["n_unresolved"]
            seen["repaired"] += info["n_repaired"]
            if pods <= 300 or run == 3:
                same_registry(s, reg)
        assert all(v > 0 for v in seen.values()), seen  # the fleet exercised every kind of outcome
        assert reaper.missings == {} or max(reaper.missings.values()) <= now
    finally:
        s.close()


def test_resident_registry_after_apply_and_a_second_run():
    fleet, groups = prune_fleet(10, 120, 3000)
    s, reaper, reg = seeded(fleet, groups)
    try:
        e, rm, info, _ = one_run(s, reaper, reg, 0, fleet.now)
        assert info["n_removed"] > 0 and info["n_repaired"] > 0
        same_registry(s, reg)  # rows and per-model entry order preserved
        e2, rm2, info2 = s.prune_registry(0, fleet.now)
        assert len(e2) == 0 and len(rm2) == 0 and int(info2["n_edits"]) == 0
        same_registry(s, reg)
    finally:
        s.close()


def _plan_base(seed, pods, models):
    """A fleet with free space (the plan has a budget) whose unloaded-or-freed models are recent enough to qualify."""
    fleet = wl.make_fleet("C1", models=models, pods=pods)
    fleet.pods["used"] = fleet.pods["capacity"] // 4
    return fleet


def test_the_plan_after_a_prune_selects_what_the_prune_freed():
    fleet, groups = prune_fleet(20, 64, 2000, _plan_base(20, 64, 2000))
    s, reaper, reg = seeded(fleet, groups)
    twin = Solver(fleet.min_space_units, fleet.min_churn_age_ms)  # the same table and registry, never pruned
    try:
        now = fleet.now
        reg0 = copy.deepcopy(reg)
        e, rm, info, _ = one_run(s, reaper, reg, 0, now)
        f2 = copy.copy(fleet)
        f2.pods = s.get_pods()
        f2.models, f2.ent_pod, f2.ent_time = rp.registry_to_arrays(reg)
        gm, gl, gi = s.proactive_plan(6400, now, fleet.n_models)
        wm, wl_, wi = ob.proactive_plan(f2, 6400, now, fleet.n_models)
        for f in ("size_estimate", "free_count", "total_count", "n_candidates", "n_selected", "error", "space_to_fill", "cutoff"):
            assert int(gi[f]) == int(wi[f]), (f, gi, wi)
        assert np.array_equal(gm, wm) and np.array_equal(gl, wl_)
        freed = {int(ed["model"]) for ed in e if ed["n_removed"] and ed["n_loaded_after"] == 0 and len(reg0[ed["model"]].loaded) > 0}
        hit = freed & set(gm.tolist())
        print(f"plan: {len(gm)} selected, {len(freed)} models freed by the prune, {len(hit)} of them selected")
        assert hit, "no selected model is one the prune freed"
        f0 = copy.copy(f2)
        f0.models, f0.ent_pod, f0.ent_time = rp.registry_to_arrays(reg0)
        twin.load_fleet(f0)
        tm, _, _ = twin.proactive_plan(6400, now, fleet.n_models)
        assert not (hit & set(tm.tolist())), "the plan selects the freed models without the prune as well"
    finally:
        s.close()
        twin.close()


def _serve_check(s, fleet, rng, models_of_interest, n=300):
    P, now = fleet.n_pods, fleet.now
    reqs = np.zeros(n, dtype=_lib.SERVE_REQ)
    reqs["model"] = rng.choice(models_of_interest, n)
    reqs["self_pod"] = rng.integers(-1, P, n)
    reqs["flags"] = rng.integers(0, 4, n)
    reqs["assume_completed_ms"] = 3000
    reqs["last_invoke_time"] = now - 10
    in_use = rng.integers(0, 3, P).astype(np.int32)
    last_used = (now - rng.choice([0, 5, 100, 10_000], P)).astype(np.int64)
    got = s.serve(reqs, in_use, last_used, np.zeros(0, np.int32), np.zeros(0, np.int64), now)
    live = np.ascontiguousarray(((fleet.pods["flags"] & 2) != 0).astype(np.uint8))
    for i in range(n):
        r, mm = reqs[i], fleet.models[reqs[i]["model"]]
        pods = fleet.ent_pod[mm["ent_off"]: mm["ent_off"] + mm["n_loaded"]]
        times = fleet.ent_time[mm["ent_off"]: mm["ent_off"] + mm["n_loaded"]]
        ch, ts = ob.serve(r["self_pod"], r["flags"] & 1, r["flags"] & 2, pods, times, now, r["assume_completed_ms"],
                          r["local_in_flight"], r["last_invoke_time"], live, in_use, last_used)
        assert got[i]["chosen"] == ch and (ch == -1 or got[i]["chosen_load_start"] == ts), (i, got[i], ch, ts)


@pytest.mark.parametrize("seed,pods,models", [(30, 60, 1500), (31, 600, 8000)])
def test_decisions_on_pruned_models_without_a_commit(seed, pods, models):
    fleet, groups = prune_fleet(seed, pods, models)
    s, reaper, reg = seeded(fleet, groups)
    try:
        e, rm, info, _ = one_run(s, reaper, reg, 0, fleet.now)
        pruned = e["model"][e["n_removed"] > 0]
        assert len(pruned) > 0
        f2 = copy.copy(fleet)
        f2.pods = s.get_pods()
        f2.models, f2.ent_pod, f2.ent_time = rp.registry_to_arrays(reg)
        rng = np.random.default_rng(seed)
        for n in (700, 6000):  # the latency slots and the batch path
            reqs, extra = wl.fuzz_requests(f2, seed + n, n)
            reqs["model"][::2] = rng.choice(pruned, len(reqs["model"][::2]))
            want = OracleFleet(f2).place(reqs, extra, f2.now, threads=4)
            assert_same_decisions(f2, reqs, s.place(reqs, extra, f2.now), want)
        _serve_check(s, f2, rng, pruned)
    finally:
        s.close()


def test_truncation_and_dry_run_change_nothing():
    fleet, groups = prune_fleet(40, 100, 2500)
    s, reaper, reg = seeded(fleet, groups)
    try:
        now = fleet.now
        flags = s.get_pods()["flags"]
        we, wrm, winfo, _ = Reaper(dict(reaper.missings)).run(flags, copy.deepcopy(reg), 0, now)
        assert len(we) > 4 and len(wrm) > 4
        marks = dict(reaper.missings)
        for flg in (_lib.PRUNE_APPLY, 0):
            for me, mr in ((3, len(wrm)), (len(we), 2), (0, 0)):
                e, rm, info = s.prune_registry_raw(0, now, GONE, rp.LASTUSED_AGE_ON_ADD_MS, flg, me, mr)
                assert int(info["truncated"]) == 1
                assert np.array_equal(e, we[:me]) and np.array_equal(rm, wrm[:mr])  # the prefix
                for f in INFO_FIELDS[:-1]:
                    assert int(info[f]) == winfo[f], (f, info, winfo)  # the totals
                same_registry(s, reg)
                assert s.missing_instances() == marks
        e, rm, info = s.prune_registry(0, now, dry=True)
        assert np.array_equal(e, we) and np.array_equal(rm, wrm) and int(info["truncated"]) == 0
        for f in INFO_FIELDS:
            assert int(info[f]) == winfo[f], (f, info, winfo)
        same_registry(s, reg)
        assert s.missing_instances() == marks
        # flags = 0: the map advances, the resident registry is the caller's to edit
        e, rm, info = s.prune_registry(0, now, apply=False)
        assert np.array_equal(e, we)
        same_registry(s, reg)
        reaper.run(flags, copy.deepcopy(reg), 0, now)
        assert s.missing_instances() == reaper.missings != marks
        with pytest.raises(MmpError):
            s.prune_registry_raw(0, now, GONE, 0, _lib.PRUNE_APPLY | _lib.PRUNE_DRY, 10, 10)
        with pytest.raises(MmpError):
            s.prune_registry_raw(0, 0, GONE, 0, 0, 10, 10)  # the clock is a wall-clock time
    finally:
        s.close()


def test_the_python_veneer_regrows_its_buffers():
    fleet, groups = prune_fleet(41, 100, 2500)
    s, reaper, reg = seeded(fleet, groups)
    try:
        one_run(s, reaper, reg, 0, fleet.now, max_edits=2, max_removed=1)
        same_registry(s, reg)
    finally:
        s.close()


def test_a_prune_during_place_batches_is_never_seen_half_applied():
    """Batches decided while the rows are rewritten equal the oracle on the registry before or after, per model.  (The removed
    entries sit on instances that are gone and therefore ineligible either way, so the two registries mostly decide alike: what
    this catches is a row seen half rewritten — new offset with old counts, or the reverse — which excludes the wrong instances.)"""
    fleet, groups = prune_fleet(50, 200, 6000)
    s, reaper, reg = seeded(fleet, groups)
    try:
        now = fleet.now
        f0 = copy.copy(fleet)
        f0.pods = s.get_pods()
        f0.models, f0.ent_pod, f0.ent_time = rp.registry_to_arrays(reg)
        reg1 = copy.deepcopy(reg)
        we, _, _, _ = Reaper(dict(reaper.missings)).run(f0.pods["flags"], reg1, 0, now)
        f1 = copy.copy(f0)
        f1.models, f1.ent_pod, f1.ent_time = rp.registry_to_arrays(reg1)
        pruned = we["model"][we["n_removed"] > 0]
        assert len(pruned) > 10
        rng = np.random.default_rng(5)
        batches = []
        for n in (300, 300, 3000, 9000):
            reqs, extra = wl.fuzz_requests(f0, 50 + n + len(batches), n)
            reqs["model"][::2] = rng.choice(pruned, len(reqs["model"][::2]))
            batches.append((reqs, extra, OracleFleet(f0).place(reqs, extra, now, threads=4), OracleFleet(f1).place(reqs, extra, now, threads=4)))
        results, stop, errors = [], threading.Event(), []

        def decide():
            try:
                k = 0
                while not stop.is_set() or k < 8:
                    b = k % len(batches)
                    results.append((b, s.place(batches[b][0], batches[b][1], now)))
                    k += 1
            except Exception as ex:  # noqa: BLE001
                errors.append(ex)

        th = threading.Thread(target=decide)
        th.start()
        while len(results) < 3 and not errors:
            time.sleep(0.001)
        e, rm, info = s.prune_registry(0, now)
        n_at_prune = len(results)
        while len(results) < n_at_prune + 3 and not errors:
            time.sleep(0.001)
        stop.set()
        th.join()
        assert not errors, errors
        assert np.array_equal(e, we)
        sides = set()
        for b, got in results:
            reqs, _, w0, w1 = batches[b]
            eq0 = np.ones(len(reqs), bool)
            eq1 = np.ones(len(reqs), bool)
            for f in ("chosen", "best", "n_candidates", "hash"):
                eq0 &= got[f] == w0[f]
                eq1 &= got[f] == w1[f]
            assert (eq0 | eq1).all(), "a decision equals neither registry"
            # per model: all of its decisions in the batch agree with ONE of the two registries
            for m in np.unique(reqs["model"][~(eq0 & eq1)]):
                rows = reqs["model"] == m
                assert eq0[rows].all() or eq1[rows].all(), f"model {m} was decided against a mixture"
            sides.add("before" if eq0.all() else "after" if eq1.all() else "both")
        print(f"{len(results)} batches decided, {n_at_prune} before the prune returned: {sorted(sides)}")
        b, got = results[-1]
        assert_same_decisions(f1, batches[b][0], got, batches[b][3])  # the last batch started after the prune had returned
        same_registry(s, reg1)
    finally:
        s.close()


def test_the_missing_map_lifetime():
    fleet, groups = prune_fleet(60, 50, 800)
    s, reaper, reg = seeded(fleet, groups)
    try:
        marks = s.missing_instances()
        assert marks and s.missing_slots() == fleet.n_pods
        # kept by pod index; survives a reload of the same index space
        s.load_pods(s.get_pods())
        s.commit()
        assert s.missing_instances() == marks
        # grows when pods are appended: the old marks stay, the new slots carry none
        row = np.zeros(2, dtype=_lib.POD_ROW)  # two empty instances
        row["capacity"], row["lru_time"], row["version"] = fleet.pods["capacity"][0], LONG_MAX, fleet.pods["version"][0]
        row["id_order"], row["loading_threads"], row["flags"] = [fleet.n_pods, fleet.n_pods + 1], 8, _lib.POD_LIVE
        s.upsert_pods(np.array([fleet.n_pods, fleet.n_pods + 1], np.int32), row)
        s.commit()
        one_run(s, reaper, reg, 0, fleet.now - GONE // 2 + 1)
        assert s.missing_slots() == fleet.n_pods + 2
        grown = s.missing_instances()
        assert all(grown.get(p) == t for p, t in marks.items()) and len(grown) > len(marks)
        assert all(p < fleet.n_pods for p in grown)
        # a leader change
        s.reset_missing_instances()
        assert s.missing_instances() == {} and s.missing_slots() == fleet.n_pods + 2
        reaper.clear()
        one_run(s, reaper, reg, 0, fleet.now)
        assert s.missing_instances()
        # mmp_pod_ids_load redefines the index space: the map is cleared
        s.load_pod_ids(["%06x-%05x" % (0, i) for i in range(fleet.n_pods + 2)])
        assert s.missing_instances() == {} and s.missing_slots() == 0
    finally:
        s.close()


def test_prune_needs_a_committed_snapshot():
    s = Solver(6553, 60_000)
    try:
        with pytest.raises(MmpError) as ei:
            s.prune_registry(0, 1_700_000_000_000)
        assert ei.value.code == _lib.MMP_ESTATE
    finally:
        s.close()


def test_the_veneer_entry_runs_under_the_mock_jvm(tmp_path):
    from tests import jni_mock as jm
    from tests.test_jni_veneer import _java_natives
    veneer = jm.Veneer(jm.build(tmp_path), _java_natives())
    env = veneer.env
    fleet, groups = prune_fleet(70, 40, 900)
    h = veneer.call("create", 0, fleet.min_space_units, fleet.min_churn_age_ms)
    assert h != 0 and env.pending() is None
    try:
        gone = np.concatenate(groups)
        fleet.pods["flags"][gone] = _lib.POD_TOMBSTONE
        assert veneer.call("podsLoad", h, jm.ByteBuffer(fleet.pods), fleet.n_pods) == 0
        assert veneer.call("modelsLoad", h, jm.ByteBuffer(fleet.models), fleet.n_models, jm.ByteBuffer(fleet.ent_pod),
                           jm.ByteBuffer(fleet.ent_time), len(fleet.ent_pod)) == 0
        assert veneer.call("commit", h) == 0
        reg = rp.registry_from_arrays(fleet.models, fleet.ent_pod, fleet.ent_time)
        reaper = Reaper()
        for now in (fleet.now, fleet.now + GONE + 1):
            we, wrm, winfo, _ = reaper.run(fleet.pods["flags"], reg, 0, now)
            edits = jm.ByteBuffer(np.zeros(max(len(we), 1), dtype=_lib.PRUNE_EDIT))
            removed = jm.ByteBuffer(np.zeros(max(len(wrm), 1), dtype=_lib.PRUNE_REMOVED))
            info = jm.ByteBuffer(np.zeros(1, dtype=_lib.PRUNE_INFO))
            rc = veneer.call("registryPrune", h, 0, now, GONE, rp.LASTUSED_AGE_ON_ADD_MS, _lib.PRUNE_APPLY, edits, len(we), removed,
                             len(wrm), info)
            assert rc == 0 and env.pending() is None
            assert np.array_equal(edits.arr[: len(we)], we) and np.array_equal(removed.arr[: len(wrm)], wrm)
            for f in INFO_FIELDS:
                assert int(info.arr[0][f]) == winfo[f], f
            since = jm.ByteBuffer(np.zeros(fleet.n_pods, np.int64))
            n = jm.ByteBuffer(np.zeros(1, np.int32))
            assert veneer.call("registryMissingGet", h, since, fleet.n_pods, n) == 0 and int(n.arr[0]) == fleet.n_pods
            assert {int(p): int(since.arr[p]) for p in np.nonzero(since.arr)[0]} == reaper.missings
        assert winfo["n_removed"] > 0
        # a short buffer is refused before the library is called
        env.clear()
        short = jm.ByteBuffer(np.zeros(2, dtype=_lib.PRUNE_EDIT))
        assert veneer.call("registryPrune", h, 0, now, GONE, 0, 0, short, 3, removed, 1, info) == -1
        assert env.pending()[0] == "java/lang/IllegalArgumentException" and "editsOut shorter" in env.pending()[1]
        env.clear()
        assert veneer.call("registryMissingReset", h) == 0
        assert veneer.call("registryMissingGet", h, since, fleet.n_pods, n) == 0 and not since.arr.any()
    finally:
        veneer.call("destroy", h)
