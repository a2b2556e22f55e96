"""pruneModelRegistry (MM.java:6524-6609) restated: hand-worked cases on the sequential form (tests/registry_prune_model.py),
the vectorised closed rule held against it on random fleets over consecutive runs, and the new C boundary."""
import copy
import os
import re

import numpy as np

from modelmesh_amd import _lib
from modelmesh_amd._lib import POD_LIVE, POD_SHUTTING_DOWN, POD_TOMBSTONE
from tests import registry_prune_model as rp
from tests.registry_prune_model import GONE_AFTER_MS as GONE, LONG_MAX, REAPER_FREQ_MS, Reaper, Record

T0 = 1_700_000_000_000  # the first reaper run
OLD = T0 - 3_600_000    # a load time well past gone-after
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flags(n, tomb=(), shutting=()):
    f = np.full(n, POD_LIVE, np.uint32)
    f[list(tomb)] = POD_TOMBSTONE
    f[list(shutting)] |= POD_SHUTTING_DOWN
    return f


def test_marked_at_run_1_untouched_at_run_2_pruned_at_run_3():
    """Runs every 7 minutes, gone-after 10: the first run only marks, the second (7 min) waits, the third (14 min) prunes
    and drops the mark."""
    flags = _flags(4, tomb=[2])
    reg = [Record(0, [(1, OLD), (2, OLD)], [], T0 - 5)]
    r = Reaper()
    e, rm, info, _ = r.run(flags, reg, 0, T0)
    assert len(e) == 0 and r.missings == {2: T0} and info["n_new_missing"] == 1 and info["n_missing_pods"] == 1
    e, rm, info, _ = r.run(flags, reg, 0, T0 + REAPER_FREQ_MS)
    assert len(e) == 0 and r.missings == {2: T0} and info["n_new_missing"] == 0
    assert reg[0].loaded == [(1, OLD), (2, OLD)]
    e, rm, info, _ = r.run(flags, reg, 0, T0 + 2 * REAPER_FREQ_MS)
    assert e.tolist() == [(0, 1, 0, 0, 0, 1, T0 - 5)] and rm.tolist() == [(2, 0, OLD)]
    assert reg[0].loaded == [(1, OLD)]
    assert r.missings == {} and info["n_missing_pods"] == 0 and info["n_removed"] == 1


def test_both_boundaries_are_strict():
    flags = _flags(3, tomb=[1])
    # :6761: an entry aged exactly gone_after is examined (only `<` skips) ...
    r = Reaper()
    r.run(flags, [Record(0, [(1, T0 - GONE)], [], 5)], 0, T0)
    assert r.missings == {1: T0}
    # ... one millisecond younger is not
    r = Reaper()
    r.run(flags, [Record(0, [(1, T0 - GONE + 1)], [], 5)], 0, T0)
    assert r.missings == {}
    # :6777: a mark aged exactly gone_after does not prune (only `>` does), and the cleanup keeps it (:6604 is `>` too)
    r = Reaper({1: T0 - GONE})
    reg = [Record(0, [(1, OLD)], [], 5)]
    e, _, _, _ = r.run(flags, reg, 0, T0)
    assert len(e) == 0 and r.missings == {1: T0 - GONE}
    e, rm, _, _ = r.run(flags, reg, 0, T0 + 1)
    assert e["n_removed"].tolist() == [1] and reg[0].loaded == [] and r.missings == {}


def test_self_is_never_examined():
    flags = _flags(3, tomb=[1])  # the table does not even hold the caller (:6765 comes before the lookup)
    r = Reaper({1: T0 - GONE - 1})
    reg = [Record(0, [(1, OLD)], [], 5)]
    e, _, info, _ = r.run(flags, reg, 1, T0)
    assert len(e) == 0 and reg[0].loaded == [(1, OLD)]


def test_a_failed_entry_is_pruned():
    flags = _flags(4, tomb=[3])
    r = Reaper({3: T0 - GONE - 1})
    reg = [Record(0, [(0, OLD)], [(2, OLD), (3, OLD)], 5)]
    e, rm, _, _ = r.run(flags, reg, 0, T0)
    assert e.tolist() == [(0, 1, 1, 0, 0, 1, 5)] and rm.tolist() == [(3, 1, OLD)]
    assert reg[0].failed == [(2, OLD)]


def test_a_returning_pod_drops_its_mark():
    r = Reaper({2: T0 - 1000})
    reg = [Record(0, [(2, OLD)], [], 5)]
    e, _, info, _ = r.run(_flags(4), reg, 0, T0)
    assert len(e) == 0 and r.missings == {} and info["n_missing_pods"] == 0


def test_a_shutting_down_pod_is_present():
    flags = _flags(4, shutting=[2])
    r = Reaper({2: T0 - GONE - 1})
    reg = [Record(0, [(2, OLD)], [], 5)]
    e, _, _, _ = r.run(flags, reg, 0, T0)
    assert len(e) == 0 and reg[0].loaded == [(2, OLD)] and r.missings == {}


def test_unresolved_entries_are_counted_and_left_alone():
    r = Reaper()
    reg = [Record(0, [(-1, OLD), (7, OLD)], [(-1, OLD)], 5)]
    e, _, info, _ = r.run(_flags(4), reg, 0, T0)
    assert len(e) == 0 and info["n_unresolved"] == 3 and r.missings == {}


def test_candidate_rule_after_the_prune():
    """:6574: a model emptied by the prune becomes a candidate in the same run; one left with two failures does not."""
    flags = _flags(5, tomb=[4])
    r = Reaper({4: T0 - GONE - 1})
    reg = [Record(0, [(4, OLD)], [(1, OLD)], T0 - 5),             # emptied, one failure: candidate
           Record(0, [(4, OLD)], [(1, OLD), (2, OLD)], T0 - 5),   # emptied, two failures: not
           Record(0, [(3, OLD), (4, OLD)], [], T0 - 5),           # partially pruned: still loaded
           Record(0, [], [], T0 - 5)]                             # never loaded: candidate, no edit
    before = copy.deepcopy(reg)
    _, _, _, cand_dry = Reaper({4: T0 - GONE - 1}).run(flags, before, 0, T0, dry=True)
    e, _, _, cand = r.run(flags, reg, 0, T0)
    assert cand == [0, 3] and cand_dry == [0, 3] and e["model"].tolist() == [0, 1, 2]
    # without the prune (no mark: first sighting) only the never-loaded model qualifies
    _, _, _, cand0 = Reaper().run(flags, copy.deepcopy(before), 0, T0)
    assert cand0 == [3]
    # the cluster-full form of the rule: lastUsed must be later than the global LRU
    _, _, _, cand_full = Reaper({4: T0 - GONE - 1}).run(flags, copy.deepcopy(before), 0, T0, global_lru=T0)
    assert cand_full == []


def test_long_max_last_used_is_repaired_before_the_candidate_rule():
    r = Reaper()
    reg = [Record(0, [], [], LONG_MAX), Record(0, [(1, OLD)], [], LONG_MAX)]
    want = T0 - 3 * rp.LASTUSED_AGE_ON_ADD_MS
    e, rm, info, cand = r.run(_flags(3), reg, 0, T0, global_lru=want)  # repaired value == globalLru: `>` fails
    assert e.tolist() == [(0, 0, 0, 1, 0, 0, want), (1, 1, 0, 1, 0, 0, want)] and len(rm) == 0 and info["n_repaired"] == 2
    assert reg[0].last_used == want and cand == []
    _, _, info, cand = r.run(_flags(3), reg, 0, T0, global_lru=want - 1)
    assert cand == [0] and info["n_edits"] == 0


def test_a_dry_run_changes_nothing():
    flags = _flags(4, tomb=[2])
    r = Reaper({2: T0 - GONE - 1})
    reg = [Record(0, [(2, OLD)], [], LONG_MAX)]
    e, rm, info, _ = r.run(flags, reg, 0, T0, dry=True)
    assert len(e) == 1 and len(rm) == 1 and reg[0].loaded == [(2, OLD)] and reg[0].last_used == LONG_MAX
    assert r.missings == {2: T0 - GONE - 1} and info["n_missing_pods"] == 0


def random_fleet(rng, n_pods, n_models, now):
    """A registry with entry ages on both sides of gone-after, unresolved ids, Long.MAX records; ~8 % tombstones."""
    flags = np.full(n_pods, POD_LIVE, np.uint32)
    tomb = rng.random(n_pods) < 0.08
    flags[tomb] = POD_TOMBSTONE
    flags[rng.random(n_pods) < 0.03] |= POD_SHUTTING_DOWN
    reg = []
    for _ in range(n_models):
        k, f = int(rng.choice([0, 1, 1, 2, 3, 6])), int(rng.choice([0, 0, 0, 1, 2, 3]))
        pods = rng.choice(n_pods, size=min(k + f, n_pods), replace=False).tolist()
        ents = [(-1 if rng.random() < 0.03 else (n_pods + 3 if rng.random() < 0.01 else p),
                 int(now - rng.choice([0, GONE - 1, GONE, GONE + 1, 5 * GONE, 100 * GONE]))) for p in pods]
        k = min(k, len(ents))
        lu = LONG_MAX if rng.random() < 0.05 else int(now - rng.integers(0, 10**8))
        reg.append(Record(int(rng.integers(0, 3)), sorted(ents[:k]), sorted(ents[k:]), lu))
    return flags, reg


def test_the_vectorised_rule_equals_the_sequential_one():
    for seed in range(12):
        rng = np.random.default_rng(8800 + seed)
        n_pods, n_models = int(rng.choice([3, 40, 300])), int(rng.choice([1, 50, 700]))
        now = T0
        flags, reg = random_fleet(rng, n_pods, n_models, now)
        tomb = np.nonzero(flags & POD_TOMBSTONE)[0]
        r = Reaper({int(p): int(now - rng.choice([1, GONE, GONE + 1, 3 * GONE])) for p in tomb if rng.random() < 0.6})
        since = np.zeros(n_pods + 2, np.int64)
        for p, t in r.missings.items():
            since[p] = t
        self_pod = int(rng.integers(-1, n_pods))
        seen_edit = 0
        for run in range(5):
            models, ep, et = rp.registry_to_arrays(reg)
            if run % 2:  # rows anywhere in an arena with garbage: the closed form follows ent_off
                pad = 5
                ep, et = np.concatenate([np.full(pad, 99, np.int32), ep]), np.concatenate([np.zeros(pad, np.int64), et])
                models["ent_off"] += pad
            e2, rm2, info2, since, keep = rp.closed_rule(flags, models, ep, et, since, self_pod, now)
            e1, rm1, info1, _ = r.run(flags, reg, self_pod, now)
            assert np.array_equal(e1, e2) and np.array_equal(rm1, rm2), (seed, run)
            assert info1 == info2, (seed, run, info1, info2)
            assert {int(p): int(since[p]) for p in np.nonzero(since)[0]} == r.missings, (seed, run)
            # the kept entries are the edited registry
            used = np.zeros(len(ep), bool)
            for m in models:
                used[m["ent_off"]: m["ent_off"] + m["n_loaded"] + m["n_failed"]] = True
            want = rp.registry_to_arrays(reg)
            assert np.array_equal(ep[keep & used], want[1]) and np.array_equal(et[keep & used], want[2])
            seen_edit += len(e1)
            now += REAPER_FREQ_MS
            if run == 2:  # an instance comes back, another one goes
                if len(tomb):
                    flags[tomb[0]] = POD_LIVE
                flags[int(rng.integers(0, n_pods))] = POD_TOMBSTONE
        assert seen_edit > 0 or n_models == 1


def test_the_boundary_declares_and_binds_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "mmplace.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for sym in ("mmp_registry_prune", "mmp_registry_missing_get", "mmp_registry_missing_reset"):
        assert re.search(r"\b%s\s*\(" % sym, code), sym
        assert sym in bound, sym
    for name in ("mmp_prune_edit", "mmp_prune_removed", "mmp_prune_info", "MMP_PRUNE_APPLY", "MMP_PRUNE_DRY"):
        assert name in code, name
    assert "#define MMP_ABI_VERSION 3" in code
    assert _lib.PRUNE_EDIT.itemsize == 32 and _lib.PRUNE_REMOVED.itemsize == 16 and _lib.PRUNE_INFO.itemsize == 32
    # the scope the header promises to state
    for word in ("readOnlyMode", "loadFailureInfos", "cleanLeaselessEtcdInstanceRecords", "janitor", "committed snapshot",
                 "mmp_pod_ids_load"):
        assert word in hdr, word
