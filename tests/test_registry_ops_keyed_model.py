"""tests/registry_ops_keyed_model.py: every boundary of the fifth kind (MM.java:3682-3687) and of the lookup by id (:2481, :2945)
worked by hand through BOTH forms, then the closed per-op form held against the sequential one on batches constructed from an
8 x 300 fleet to take every named exit."""
import copy

import numpy as np
import pytest

from modelmesh_amd import workload as wl
from modelmesh_amd._lib import (ROP_DEREGISTER, ROP_DROP_LOCAL, ROP_EDIT_REM_LOADED, ROP_EDIT_TOUCHED, ROP_EDIT_UNLOAD_SET, ROP_EDITED,
                                ROP_NO_RECORD, ROP_REGISTER, ROP_SCALE_DOWN, ROPF_MATCH_TIME, ROPF_SHUTTING_DOWN)
from tests import registry_ops_keyed_model as rk
from tests import registry_ops_model as ro
from tests.registry_ops_keyed_model import KeyedRegistry
from tests.registry_ops_model import LONG_MAX, InvalidOps, ModelRecord, op_row, ops_array

NOW = 1_700_000_000_000
ID_ORDER = np.array([30, 10, 50, 20, 40, 60], np.uint32)  # instance index -> place of its id among the ids
KEY = b"model-a"


def both_forms(kreg, ops, keys, now=NOW, dry=False):
    """One batch through the sequential form and the closed form (on the arrays of the registry as it stood, behind the
    resolution), every output equal; the arrays rebuilt from the edits equal the records the sequential form left.  Returns
    (model_idx, status, edits, info)."""
    before = copy.deepcopy(kreg)
    arrays = ro.registry_to_arrays(before.records_by_row())
    staged = rk.staged_ops(before, ops, keys)
    cst, ced, cinfo = rk.closed_rule_k(*arrays, staged, now, kreg.id_order)
    idx, st, ed, info = kreg.run(ops, keys, now, dry=dry)
    assert np.array_equal(st, cst) and np.array_equal(ed, ced) and info == cinfo, (st, cst, ed, ced, info, cinfo)
    assert [int(i) for i in idx] == [before.row(k) for k in keys]
    if not dry:
        got = ro.registry_from_arrays(*ro.apply_edits(*arrays, staged, ced))
        want = kreg.records_by_row()
        for g, w in zip(got, want):  # (the arrays carry no lastUnloadTime)
            assert g == ModelRecord(w.type, w.instance_ids, w.load_failed_instance_ids, w.last_used)
    return idx, st, ed, info


def drop(record, pod, last_used=0, now=NOW, op=ROP_DROP_LOCAL, **kw):
    """One op on one record under KEY: (record after, status, edit or None)."""
    kreg = KeyedRegistry([KEY], [copy.deepcopy(record)], ID_ORDER)
    idx, st, ed, info = both_forms(kreg, ops_array([op_row(99, pod, op, last_used=last_used, **kw)]), [KEY], now)
    assert idx[0] == 0 and info["n_edits"] + info["n_unchanged"] + info["n_no_record"] == 1
    return kreg.registry[KEY], int(st[0]), (ed[0] if len(ed) else None)


def rec(loaded=(), failed=(), last_used=NOW - 1000, last_unload=0):
    return ModelRecord(0, list(loaded), list(failed), last_used, last_unload)


def loaded(r):
    return list(r.instance_ids.items())


def failed(r):
    return list(r.load_failed_instance_ids.items())


# ---- DROP_LOCAL: the entry --------------------------------------------------------------------------------------------------

def test_drop_local_with_the_entry_present_removes_it_whatever_its_time():
    r, st, e = drop(rec([(1, 4), (0, 5), (2, 6)]), 0, last_used=NOW)
    assert st == ROP_EDITED and loaded(r) == [(1, 4), (2, 6)]
    assert e["flags"] == ROP_EDIT_REM_LOADED | ROP_EDIT_TOUCHED and e["inserted_pos"] == -1 and e["model"] == 0 and e["op_index"] == 0
    assert (e["n_loaded_after"], e["n_failed_after"], e["last_used_after"], e["last_unload_after"]) == (2, 0, NOW, 0)
    # load_time / load_complete_time are not read: the same op with any times is the same edit
    r2, _, e2 = drop(rec([(1, 4), (0, 5), (2, 6)]), 0, last_used=NOW, load_time=-9, load_complete_time=77)
    assert r2 == r and e2.tobytes() == e.tobytes()


def test_drop_local_with_the_entry_absent_is_still_an_edit():
    before = rec([(1, 4), (2, 6)], [(3, 7)])
    r, st, e = drop(before, 0, last_used=NOW - 2000)           # nothing to remove, lastUsed not raised: submitted all the same (:3687)
    assert st == ROP_EDITED and e is not None and e["flags"] == 0 and r == before
    assert (e["n_loaded_after"], e["n_failed_after"], e["last_used_after"], e["inserted_pos"]) == (2, 1, NOW - 1000, -1)
    r, st, e = drop(before, 0, last_used=0)
    assert st == ROP_EDITED and e["flags"] == ROP_EDIT_TOUCHED and r.last_used == NOW and loaded(r) == loaded(before)
    r, st, e = drop(rec(), 4, last_used=NOW - 2000)            # a record without any entry
    assert st == ROP_EDITED and e["flags"] == 0 and (e["n_loaded_after"], e["n_failed_after"]) == (0, 0)


@pytest.mark.parametrize("copies", [1, 2, 3, 4])
def test_drop_local_never_touches_last_unload_in_contrast_to_deregister(copies):
    pods = [1, 3, 0, 4][:copies]                               # in id order: 10, 20, 30, 40
    before = rec([(p, 100 + p) for p in pods], last_unload=4242)
    r, st, e = drop(before, pods[-1], last_used=NOW - 2000)
    assert st == ROP_EDITED and loaded(r) == [(p, 100 + p) for p in pods[:-1]]
    assert r.last_unload_time == 4242 and not e["flags"] & ROP_EDIT_UNLOAD_SET and e["last_unload_after"] == 0
    assert e["flags"] == ROP_EDIT_REM_LOADED and e["n_loaded_after"] == copies - 1
    d, dst, de = drop(before, pods[-1], last_used=NOW - 2000, op=ROP_DEREGISTER)   # the same record, the older kind
    assert dst == ROP_EDITED and de["flags"] == ROP_EDIT_REM_LOADED | ROP_EDIT_UNLOAD_SET
    assert d.last_unload_time == (NOW if copies - 1 > 2 else 0) and de["last_unload_after"] == d.last_unload_time
    assert loaded(d) == loaded(r)


def test_drop_local_leaves_the_failure_record_of_the_same_instance():
    before = rec([(1, 4), (0, 5)], [(3, 7), (0, 8)])
    r, st, e = drop(before, 0, last_used=NOW)
    assert loaded(r) == [(1, 4)] and failed(r) == [(3, 7), (0, 8)]
    assert e["flags"] == ROP_EDIT_REM_LOADED | ROP_EDIT_TOUCHED and (e["n_loaded_after"], e["n_failed_after"]) == (1, 2)
    r, st, e = drop(rec([(1, 4)], [(0, 8)]), 0, last_used=NOW)  # only the failure record is there: nothing is removed
    assert loaded(r) == [(1, 4)] and failed(r) == [(0, 8)] and e["flags"] == ROP_EDIT_TOUCHED


def test_drop_local_beside_an_unresolved_entry():
    before = rec([(3, 1), (-1, 2), (9, 3), (2, 4)])            # -1 and 9 are not in the instance table
    r, st, e = drop(before, 2, last_used=NOW)
    assert loaded(r) == [(3, 1), (-1, 2), (9, 3)] and e["n_loaded_after"] == 3
    r, st, e = drop(before, 5, last_used=NOW)                   # absent: the unresolved ones are no match for anybody
    assert loaded(r) == loaded(before) and e["flags"] == ROP_EDIT_TOUCHED


# ---- DROP_LOCAL: lastUsed ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lu,want,touched", [(0, NOW, True), (NOW - 1001, NOW - 1000, False), (NOW - 1000, NOW - 1000, False),
                                             (NOW - 999, NOW - 999, True)])
def test_drop_local_last_used_zero_lower_equal_higher(lu, want, touched):
    r, st, e = drop(rec([(0, 5)]), 0, last_used=lu)
    assert r.last_used == want == e["last_used_after"] and bool(e["flags"] & ROP_EDIT_TOUCHED) == touched


def test_drop_local_on_a_record_at_long_max():
    for lu in (0, NOW, LONG_MAX):
        r, st, e = drop(rec([(0, 5)], last_used=LONG_MAX), 0, last_used=lu)
        assert r.last_used == LONG_MAX == e["last_used_after"] and e["flags"] == ROP_EDIT_REM_LOADED


def test_drop_local_admits_no_flag_bit():
    for flags in (ROPF_SHUTTING_DOWN, ROPF_MATCH_TIME, 4):
        with pytest.raises(InvalidOps):
            drop(rec([(0, 5)]), 0, flags=flags)
    with pytest.raises(InvalidOps):
        drop(rec([(0, 5)]), 0, op=5)
    with pytest.raises(InvalidOps):
        drop(rec([(0, 5)]), 6)


# ---- NO_RECORD --------------------------------------------------------------------------------------------------------------

def small_world():
    ids = [b"a", b"b", b"c", b"d"]
    recs = [rec([(0, 5)]), rec([(1, 6)], [(2, 7)]), rec([(3, 8), (0, 9)]), rec()]
    return KeyedRegistry(ids, recs, ID_ORDER)


@pytest.mark.parametrize("kind", [ROP_REGISTER, 1, ROP_DEREGISTER, ROP_SCALE_DOWN, ROP_DROP_LOCAL])
def test_an_unknown_id_a_deleted_id_and_an_id_registered_again(kind):
    k = small_world()
    op = lambda pod: op_row(0, pod, kind, last_used=0, load_time=6)  # noqa: E731
    idx, st, ed, info = both_forms(k, ops_array([op(1)]), [b"nope"])
    assert (idx[0], st[0], len(ed)) == (-1, ROP_NO_RECORD, 0) and info["n_no_record"] == 1 and info["n_unchanged"] == 0
    assert info["n_unchanged_op"] == [0] * 8 and info["n_edited_op"] == [0] * 8
    before = copy.deepcopy(k.registry)
    k.delete(b"b")
    idx, st, ed, info = both_forms(k, ops_array([op(1)]), [b"b"])
    assert (idx[0], st[0], len(ed)) == (1, ROP_NO_RECORD, 0)       # the row is still the table's, the record is gone
    assert k.get(b"b") is None and k.registry == {x: before[x] for x in (b"a", b"c", b"d")}
    k.put(b"b", rec([(4, 1)]))                                      # registered again: the same row, and now it edits
    idx, st, ed, info = both_forms(k, ops_array([op_row(0, 4, ROP_DROP_LOCAL, last_used=0)]), [b"b"])
    assert (idx[0], st[0]) == (1, ROP_EDITED) and ed[0]["model"] == 1 and loaded(k.registry[b"b"]) == []


def test_the_all_zero_record_is_the_deleted_one():
    k = KeyedRegistry([b"z", b"y"], [ModelRecord(0, [], [], 0), ModelRecord(0, [], [], 1)], ID_ORDER)
    idx, st, ed, info = both_forms(k, ops_array([op_row(0, 1, ROP_REGISTER, load_time=5), op_row(0, 1, ROP_REGISTER, load_time=5)]), [b"z", b"y"])
    assert list(idx) == [0, 1] and list(st) == [ROP_NO_RECORD, ROP_EDITED] and list(ed["model"]) == [1] and list(ed["op_index"]) == [1]


def test_duplicates_are_two_positions_on_one_live_record_only():
    k = small_world()
    two = ops_array([op_row(0, 0, ROP_DROP_LOCAL), op_row(0, 3, ROP_DROP_LOCAL)])
    before = copy.deepcopy(k.registry)
    with pytest.raises(InvalidOps):
        k.run(two, [b"c", b"c"], NOW)
    with pytest.raises(InvalidOps):
        rk.closed_rule_k(*ro.registry_to_arrays(k.records_by_row()), rk.staged_ops(k, two, [b"c", b"c"]), NOW, ID_ORDER)
    assert k.registry == before
    idx, st, ed, info = both_forms(k, two, [b"nope", b"nope"])       # no record under the key: nothing to name twice
    assert list(st) == [ROP_NO_RECORD] * 2 and info["n_no_record"] == 2 and info["n_edits"] == 0 and k.registry == before
    k.delete(b"a")
    idx, st, ed, info = both_forms(k, two, [b"a", b"a"])
    assert list(st) == [ROP_NO_RECORD] * 2 and list(idx) == [0, 0]


def test_retired_rows_renumber_the_table_and_the_ids_still_name_their_records():
    k = small_world()
    k.delete(b"a")
    k.retire([0])
    idx, st, ed, info = both_forms(k, ops_array([op_row(0, 0, ROP_DROP_LOCAL, last_used=NOW), op_row(0, 1, ROP_DROP_LOCAL)]), [b"c", b"a"])
    assert list(idx) == [1, -1] and list(st) == [ROP_EDITED, ROP_NO_RECORD] and ed[0]["model"] == 1
    assert loaded(k.registry[b"c"]) == [(3, 8)] and loaded(k.registry[b"b"]) == [(1, 6)]


def test_a_dry_run_changes_nothing():
    k = small_world()
    before = copy.deepcopy(k.registry)
    idx, st, ed, info = both_forms(k, ops_array([op_row(0, 0, ROP_DROP_LOCAL), op_row(0, 1, ROP_DEREGISTER)]), [b"a", b"b"], dry=True)
    assert list(st) == [ROP_EDITED, ROP_EDITED] and k.registry == before


# ---- the two forms on constructed batches -----------------------------------------------------------------------------------

def fleet_world(seed, pods=8, models=300):
    """An 8 x 300 fuzz fleet with the shapes of ro.seed_shapes, named m<i>; every 29th record deleted."""
    fleet = wl.fuzz_fleet(seed + 1300, pods=pods, models=models)
    rng = np.random.default_rng(95_000 + seed)
    recs = ro.registry_from_arrays(fleet.models, fleet.ent_pod, fleet.ent_time)
    ro.seed_shapes(recs, fleet.pods["id_order"], int(fleet.now), rng)
    k = KeyedRegistry([b"m%d" % i for i in range(models)], recs, fleet.pods["id_order"].copy())
    shaped = {id(r) for r in recs if r.last_used in (0, LONG_MAX) or any(p < 0 for p in r.instance_ids)}
    for i in range(5, models, 29):
        if id(recs[i]) not in shaped:
            k.delete(b"m%d" % i)
    return k, int(fleet.now), rng


@pytest.mark.parametrize("seed,n", [(0, 120), (1, 257), (2, 64)])
def test_the_closed_form_equals_the_sequential_one_and_every_exit_occurs(seed, n):
    k, now, rng = fleet_world(seed)
    seen_k, seen_old = set(), set()
    for batch in range(3):
        ops, keys = rk.draw_ops_k(k, now + batch, rng, n)
        assert len(ops) == n
        before = copy.deepcopy(k)
        idx, st, ed, info = both_forms(k, ops, keys, now + batch)
        by_op = {int(e["op_index"]): e for e in ed}
        for i, (o, key) in enumerate(zip(ops, keys)):
            seen_k.update(rk.classify_k(before, o, key, st[i]))
            if before.get(key) is not None and o["op"] != ROP_DROP_LOCAL:
                seen_old.update(ro.classify(before.get(key), o, st[i], by_op.get(i)))
        assert info["n_edits"] + info["n_unchanged"] + info["n_no_record"] == n and info["n_no_record"] >= 4
        assert info["n_edited_op"][ROP_DROP_LOCAL] > 0 and info["n_unchanged_op"][ROP_DROP_LOCAL] == 0
    assert seen_k == set(rk.EXITS_K), set(rk.EXITS_K) - seen_k
    if n >= 120:
        assert len(seen_old) >= 20, sorted(set(ro.EXITS) - seen_old)   # (the older kinds' own file asserts each of theirs)
