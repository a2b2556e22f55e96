"""The janitor restatement (tests/janitor_model.py) by hand at every boundary, its two forms against each other over
consecutive runs, the recipe's visibility condition for every fleet the GPU tests use, and the join with the scale-down."""
import copy

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd._lib import (JAN_EDIT_REGISTERED, JAN_EDIT_REM_FAILED, JAN_EDIT_REM_LOADED, JAN_EDIT_REPAIRED,
                                JAN_EDIT_TIMESTAMP_MISMATCH, JAN_EDIT_TOUCHED, JAN_EDIT_UNLOAD_SET, JAN_EXPIRED, JAN_IN_ORDER, JAN_NONE,
                                JAN_REFRESHED, JAN_REGISTERED, JAN_REMOVED, JAN_REPAIRED, JANITOR_ENTRY, JE_DONE, JE_FAILED, JE_STATE_LIVE)
from tests import janitor_model as jm
from tests import registry_prune_model as rp
from tests.registry_prune_model import LONG_MAX, Record

NOW = 1_700_000_000_000
SELF = 2
ID_ORDER = np.array([0, 1, 2, 3, 4, 5], np.uint32)
LIVE = JE_DONE | JE_STATE_LIVE
FAILED = JE_DONE | JE_FAILED
OLD = NOW - 2_000_000
RECENT_WINDOW = 360 * 2000 + 240_000
PINNED_REMOVALS = [138, 156]  # of 483 and 523 candidates: what the scale-down oracle removes in the two runs of
                              # test_the_candidates_feed_the_scale_down (seed 12), recorded once


def entry(model, last_used, lt=0, lct=0, flags=LIVE, luat=-1, weight=10):
    e = np.zeros(1, dtype=JANITOR_ENTRY)
    e[0] = (model, weight, last_used, lt, lct, luat, 3, NOW - 9_000_000, 0, 1, 2, flags, 0)
    return e


def run(reg, entries, **kw):
    """Both forms on the same input; asserts them equal; returns the sequential form's outputs (and leaves `reg` edited)."""
    entries = np.concatenate(entries) if isinstance(entries, list) else entries
    prm = jm.params(SELF, NOW, **kw)
    arrays = rp.registry_to_arrays(reg)
    closed = jm.closed_rule(*arrays, entries, prm, ID_ORDER)
    seq = jm.Janitor().run(reg, entries, prm, ID_ORDER)
    same(seq, closed)
    return seq


def same(a, b):
    for x, y, what in zip(a[:4], b[:4], ("actions", "edits", "candidates", "rows")):
        assert np.array_equal(x, y), (what, x, y)
    assert a[4] == b[4], (a[4], b[4])


def test_recently_used_is_strict():
    for age, want in ((RECENT_WINDOW - 1, JAN_NONE), (RECENT_WINDOW, JAN_REGISTERED)):
        reg = [Record(0, [(0, 5)], [], NOW - 100)]
        a, e, c, rows, info = run(reg, [entry(0, NOW - age, lt=77)])
        assert a[0] == want
        assert (len(e) == 1 and e[0]["flags"] & JAN_EDIT_REGISTERED and reg[0].loaded == [(0, 5), (SELF, 77)]) == (want == JAN_REGISTERED)


def test_min_stale_age_is_inclusive_and_only_raises():
    for gap, want in ((999, JAN_IN_ORDER), (1000, JAN_REFRESHED)):
        reg = [Record(0, [(SELF, 77)], [], OLD - gap)]
        a, e, *_ = run(reg, [entry(0, OLD, lt=77)], min_stale_age_ms=1000)
        assert a[0] == want and (len(e) == 1) == (want == JAN_REFRESHED)
        if len(e):
            assert e[0]["flags"] == JAN_EDIT_TOUCHED and e[0]["last_used_after"] == OLD == reg[0].last_used
    # the recently-used branch refreshes too; a record ahead of the cache is left alone
    reg = [Record(0, [(SELF, 77)], [], NOW - 5000), Record(0, [(SELF, 78)], [], NOW)]
    a, e, *_ = run(reg, [entry(0, NOW - 10, lt=1), entry(1, NOW - 20, lt=78)], min_stale_age_ms=1000)
    assert list(a) == [JAN_REFRESHED, JAN_NONE] and list(e["model"]) == [0]


def test_unload_attempt_age_and_age_of_zero():
    # age(0) == 0: "just attempted"; -1 (never) is ages ago; the bound is strict
    for luat, want in ((0, JAN_REMOVED), (-1, JAN_REGISTERED), (NOW - 599_999, JAN_REMOVED), (NOW - 600_000, JAN_REGISTERED)):
        reg = [Record(0, [(SELF, 5)], [], OLD)]
        a, e, c, *_ = run(reg, [entry(0, OLD, lt=6, luat=luat)])
        assert a[0] == want, luat
        if want == JAN_REGISTERED:
            assert e[0]["flags"] == JAN_EDIT_REGISTERED | JAN_EDIT_TIMESTAMP_MISMATCH and reg[0].loaded == [(SELF, 6)]
            assert e[0]["inserted_pos"] == 0 and e[0]["inserted_time"] == 6 and len(c) == 1
        else:
            assert len(e) == 0 and len(c) == 0  # the registration stays (the entry is not failed), but it is no candidate: not in the cache


def test_both_expiries_are_strict_and_the_switch_is_at_three_minutes():
    def expired(failed_age, used_age):
        reg = [Record(0, [], [(SELF, NOW - failed_age)], NOW)]
        ents = [entry(0, NOW - used_age, lct=NOW - failed_age, flags=FAILED)]
        a, e, *_ = run(reg, ents)
        return a[0] == JAN_EXPIRED and len(e) == 1 and e[0]["flags"] == JAN_EDIT_REM_FAILED and reg[0].failed == []

    assert not expired(450_000, 1000) and expired(450_001, 1000)            # 7.5 minutes, strict
    assert expired(450_001, 179_999) and not expired(450_001, 180_000)      # used exactly 3 minutes ago: the full rule
    assert not expired(900_000, 180_000) and expired(900_001, 180_000)      # 15 minutes, strict
    # no cache entry at all: lastUsed = -1, the full rule
    for age, gone in ((900_000, False), (900_001, True)):
        reg = [Record(0, [(0, 1)], [(SELF, NOW - age)], NOW)]
        a, e, *_ = run(reg, np.zeros(0, JANITOR_ENTRY))
        assert (len(e) == 1) == gone
    # a live copy under a failure record: the record goes at once (:6042) and the entry is registered before that (:5980)
    reg = [Record(0, [], [(SELF, NOW - 5)], OLD - 1)]
    a, e, c, *_ = run(reg, [entry(0, OLD, lt=9)])
    assert a[0] == JAN_REGISTERED and e[0]["flags"] == JAN_EDIT_REGISTERED | JAN_EDIT_TOUCHED and reg[0].failed == [] and len(c) == 1


def test_last_unload_time_two_against_three_copies_left():
    for others, want in (([(0, 1), (1, 1)], 0), ([(0, 1), (1, 1), (3, 1)], NOW)):
        reg = [Record(0, sorted(others + [(SELF, 7)]), [], OLD)]
        a, e, c, *_ = run(reg, np.zeros(0, JANITOR_ENTRY))
        assert e[0]["flags"] == JAN_EDIT_REM_LOADED | JAN_EDIT_UNLOAD_SET and e[0]["last_unload_after"] == want
        assert e[0]["n_loaded_after"] == len(others) and reg[0].loaded == others and e[0]["entry"] == -1 and len(c) == 0


def test_two_candidates_with_equal_last_used_the_first_in_registry_order_stays():
    reg = [Record(0, [(SELF, 10 + m)], [], NOW) for m in range(4)]
    ents = [entry(3, OLD + 5, lt=13, weight=33), entry(1, OLD, lt=11, weight=11), entry(2, OLD, lt=12, weight=22), entry(0, OLD - 5, lt=10)]
    a, e, c, rows, info = run(reg, ents)
    assert list(a) == [JAN_IN_ORDER] * 4 and len(e) == 0
    assert list(c["model"]) == [0, 1, 3] and list(rows) == [3, 1, 0] and list(c["last_used"]) == [OLD - 5, OLD, OLD + 5]
    assert info["n_candidates"] == 3 and info["n_ties"] == 1 and list(c["weight"]) == [10, 11, 33]


@pytest.mark.parametrize("at", [0, 2, 4])
def test_the_long_max_stop(at):
    reg = [Record(0, [(SELF, 10 + m)], [], LONG_MAX if m == at else OLD) for m in range(5)]
    ents = [entry(m, LONG_MAX if m == at else OLD - m, lt=99) for m in range(5)]
    a, e, c, rows, info = run(reg, ents)
    assert info["stopped_at"] == at and len(c) == 0 and info["n_candidates"] == 0
    assert list(a) == [JAN_REGISTERED] * at + [JAN_REPAIRED] + [JAN_NONE] * (4 - at)
    assert list(e["model"]) == list(range(at + 1)) and e[at]["flags"] == JAN_EDIT_REPAIRED
    assert e[at]["last_used_after"] == NOW - 3 * jm.LASTUSED_AGE_ON_ADD_MS == reg[at].last_used
    assert all(r.loaded == [(SELF, 99)] for r in reg[:at]) and all(r.loaded == [(SELF, 10 + m)] for m, r in enumerate(reg) if m >= at)
    # a row that is not done does not stop the run
    reg = [Record(0, [(SELF, 10)], [], OLD)]
    a, e, c, rows, info = run(reg, [entry(0, LONG_MAX, lt=10, flags=JE_STATE_LIVE)])
    assert info["stopped_at"] == -1 and a[0] == JAN_NONE and len(c) == 1


def test_an_entry_the_cache_loop_removed_meets_the_registry_loop():
    # failed entry, failure record under ANOTHER timestamp: removed from the cache (:5970); the registry loop still finds it
    # in the snapshot (ce != null, failed), but getLastUsedTime gives -1: the full rule, no updateLastUsed, no second removal
    reg = [Record(0, [], [(SELF, NOW - 900_001)], OLD - 50), Record(0, [], [(SELF, NOW - 900_000)], OLD - 50)]
    ents = [entry(0, OLD, lct=1, flags=FAILED), entry(1, OLD - 1, lct=1, flags=FAILED)]
    a, e, c, rows, info = run(reg, ents)
    assert list(a) == [JAN_REMOVED, JAN_REMOVED]
    assert len(e) == 1 and e[0]["model"] == 0 and e[0]["flags"] == JAN_EDIT_REM_FAILED and e[0]["last_used_after"] == OLD - 50
    assert info["n_action"][JAN_REMOVED] == 2 and info["n_action"][JAN_EXPIRED] == 0
    # a live-looking entry removed for a recent unload attempt keeps its registration and is NOT a candidate
    reg = [Record(0, [(SELF, 5)], [], NOW)]
    a, e, c, *_ = run(reg, [entry(0, OLD, lt=6, luat=NOW - 1)])
    assert a[0] == JAN_REMOVED and len(e) == 0 and len(c) == 0 and reg[0].loaded == [(SELF, 5)]


def test_shutting_down_does_nothing():
    reg = [Record(0, [(SELF, 5)], [(SELF, 1)], OLD)]
    before = copy.deepcopy(reg)
    a, e, c, rows, info = run(reg, [entry(0, OLD, lt=6), entry(-1, OLD - 1)], shutting_down=1)
    assert not a.any() and len(e) == 0 and len(c) == 0 and info["n_action"][0] == 2 and info["stopped_at"] == -1
    assert reg == before


def test_where_a_registered_entry_goes():
    # in front of the first resolved entry with a greater id; unresolved ones keep their place and are not compared
    order = np.array([5, 4, 3, 2, 1, 0], np.uint32)  # pod 0 has the greatest id
    for loaded, want in (([(4, 1), (-1, 2), (1, 3)], [(4, 1), (-1, 2), (SELF, 9), (1, 3)]), ([(-1, 2), (5, 3)], [(-1, 2), (5, 3), (SELF, 9)]),
                         ([(9, 2), (0, 3)], [(9, 2), (SELF, 9), (0, 3)])):
        reg = [Record(0, list(loaded), [], OLD)]
        prm = jm.params(SELF, NOW)
        ents = entry(0, OLD, lt=9)
        closed = jm.closed_rule(*rp.registry_to_arrays(reg), ents, prm, order)
        seq = jm.Janitor().run(reg, ents, prm, order)
        same(seq, closed)
        assert reg[0].loaded == want and seq[1][0]["inserted_pos"] == want.index((SELF, 9))


def test_check_entries():
    assert jm.check_entries(np.concatenate([entry(0, 1), entry(-1, 1), entry(-1, 1), entry(4, 1)]), 5)
    assert not jm.check_entries(np.concatenate([entry(0, 1), entry(0, 1)]), 5)
    assert not jm.check_entries(entry(5, 1), 5) and not jm.check_entries(entry(-2, 1), 5)


def sequence(seed, pods, models, base=None, runs=3):
    """Consecutive runs 6 minutes apart; the registry and cache edits of one run are in place before the next (the cache is
    rebuilt from the edited registry).  Yields per run (registry before, entries, params, sequential outputs)."""
    fleet, self_pod, reg = jm.janitor_fleet(seed, pods, models, base)
    for k in range(runs):
        now = int(fleet.now) + k * jm.RUN_EVERY_MS
        entries = jm.make_cache(fleet, reg, self_pod, 1000 * seed + k, now)
        assert jm.check_entries(entries, fleet.n_models)
        prm = jm.params(self_pod, now)
        before = copy.deepcopy(reg)
        out = jm.Janitor().run(reg, entries, prm, fleet.pods["id_order"])
        yield fleet, self_pod, before, reg, entries, prm, out


@pytest.mark.parametrize("seed,pods,models", [(s, p, m) for s, p, m in jm.GPU_FLEETS if m <= 20000] + [(11, 30, 500), (12, 64, 1500)])
def test_the_two_forms_agree_over_consecutive_runs(seed, pods, models):
    for fleet, self_pod, before, reg, entries, prm, out in sequence(seed, pods, models):
        closed = jm.closed_rule(*rp.registry_to_arrays(before), entries, prm, fleet.pods["id_order"])
        same(out, closed)
        # and on an arena with garbage between the rows
        m, ep, et = rp.registry_to_arrays(before)
        m2 = m.copy()
        m2["ent_off"] += 3
        closed = jm.closed_rule(m2, np.concatenate([[7, 7, 7], ep]).astype(np.int32), np.concatenate([[1, 1, 1], et]).astype(np.int64), entries, prm,
                                fleet.pods["id_order"])
        same(out, closed)


def _shown(seed, pods, models, base=None):
    seen = {}
    for fleet, self_pod, before, reg, entries, prm, out in sequence(seed, pods, models, base):
        v = jm.visibility(before, out[1], out[0], out[4], int(prm[0]["now"]))
        v["short_expiry"], v["full_expiry"], v["failure_stays"] = jm.expiry_kinds(before, reg, entries, self_pod, prm)
        for k, x in v.items():
            seen[k] = seen.get(k, 0) + x
    return seen


@pytest.mark.parametrize("seed,pods,models", jm.GPU_FLEETS)
def test_the_recipe_shows_every_outcome_for_every_gpu_fleet(seed, pods, models):
    from modelmesh_amd import workload as wl
    seen = _shown(seed, pods, models, wl.make_fleet("C3") if models == 100_000 else None)
    print(seen)
    assert all(v > 0 for v in seen.values()), seen


def test_the_candidates_feed_the_scale_down():
    """The run's candidate rows go to the scale-down restatement unchanged: they are the candidates the sequential form built
    (registry order filtered, then oldest first without ties), and the removals that follow are the oracle's on those rows."""
    from oracle import bind as ob
    removed, n_cands = [], []
    for fleet, self_pod, before, reg, entries, prm, (actions, edits, cands, rows, info) in sequence(12, 64, 1500, runs=2):
        assert len(cands) > 20 and cands.dtype == _lib.CACHE_ENTRY
        # rebuilt independently from the edited registry and the surviving cache: loaded on self_pod, still cached, not failed
        alive = {int(entries[r]["model"]): r for r in range(len(entries))
                 if actions[r] not in (JAN_REMOVED, JAN_EXPIRED) and entries[r]["model"] >= 0 and entries[r]["last_used"] > 0
                 and not entries[r]["flags"] & JE_FAILED}
        want, seen_times = [], set()
        for m, rec in enumerate(reg):
            if m in alive and any(p == self_pod for p, _ in rec.loaded) and int(entries[alive[m]]["last_used"]) not in seen_times:
                seen_times.add(int(entries[alive[m]]["last_used"]))
                want.append((int(entries[alive[m]]["last_used"]), alive[m]))
        want.sort()
        assert [r for _, r in want] == list(rows) and [t for t, _ in want] == list(cands["last_used"])
        assert np.all(np.diff(cands["last_used"]) > 0)
        f2 = copy.copy(fleet)
        f2.models, f2.ent_pod, f2.ent_time = rp.registry_to_arrays(reg)
        f2.pods = fleet.pods.copy()
        f2.pods["used"] = f2.pods["capacity"] - f2.pods["capacity"] // 50  # the cluster is close to full (:6229), or nothing is scaled down
        f2.pods["lru_time"] = int(prm[0]["now"]) - 5_000_000  # a young cache: a second copy unused for 17 minutes is old enough (:6253-6258)
        sp = np.zeros(1, dtype=_lib.SCALEDOWN_PARAMS)
        sp[0] = (self_pod, 0, int(prm[0]["now"]), int(prm[0]["now"]) - 11_000, 10_000, 2_000_000, 2000, 0)
        rem = ob.scaledown_plan(f2, cands, sp)
        # the same removals from rows built here from the cache rows alone, in the order worked out above
        indep = np.zeros(len(want), dtype=_lib.CACHE_ENTRY)
        for k, (t, r) in enumerate(want):
            indep[k]["model"], indep[k]["last_used"] = entries[r]["model"], t
            for f in jm.CAND_FIELDS:
                indep[k][f] = entries[r][f]
        assert np.array_equal(indep, cands)
        assert np.array_equal(ob.scaledown_plan(f2, indep, sp), rem)
        n_cands.append(cands)
        removed.append(sorted(int(m) for m in cands["model"][rem != 0]))
        # removeModelCopies' conditions that can be read off the record (:6223, :6233-6248, :6258, :6265-6270): a removed model has
        # another copy on an instance that is in the table and not shutting down; with two copies it was unused for longer than a
        # tenth of the cache's age; with more, no copy was unloaded within 8 rate intervals or loaded within 30 minutes
        now_ = int(prm[0]["now"])
        for c in cands[rem != 0]:
            rec = reg[c["model"]]
            others = [p for p, _ in rec.loaded if p != self_pod]
            assert len(rec.loaded) >= 2 and any(0 <= p < fleet.n_pods and not f2.pods["flags"][p] & 5 for p in others)
            if len(rec.loaded) == 2:
                assert now_ - int(c["last_used"]) > 5_000_000 // 10
            else:
                assert not (c["last_unload_time"] > 0 and now_ - int(c["last_unload_time"]) < 8 * 10_000)
                assert not any(t > now_ - 1_800_000 for _, t in rec.loaded)
    assert [len(c) for c in n_cands] == [483, 523]
    assert all(len(x) > 0 for x in removed)
    assert [len(x) for x in removed] == PINNED_REMOVALS, removed
