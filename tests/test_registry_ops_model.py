"""tests/registry_ops_model.py: every boundary of the four Java sites worked by hand on the sequential form, the closed per-op
form held against it on batches constructed to take every exit, and the census moving by exactly the entries put and removed."""
import copy

import numpy as np
import pytest

from modelmesh_amd import workload as wl
from modelmesh_amd._lib import (ROP_DEREGISTER, ROP_EDIT_PUT_FAILED, ROP_EDIT_PUT_LOADED, ROP_EDIT_REM_FAILED, ROP_EDIT_REM_LOADED,
                                ROP_EDIT_REPLACED, ROP_EDIT_TOUCHED, ROP_EDIT_UNLOAD_SET, ROP_EDITED, ROP_LOAD_FAILED, ROP_REGISTER,
                                ROP_SCALE_DOWN, ROP_UNCHANGED, ROPF_MATCH_TIME, ROPF_SHUTTING_DOWN)
from tests import registry_census_model as rc
from tests import registry_ops_model as ro
from tests.registry_ops_model import LONG_MAX, ModelRecord, Registry, op_row, ops_array

NOW = 1_700_000_000_000
ID_ORDER = np.array([30, 10, 50, 20, 40, 60], np.uint32)  # instance index -> place of its id among the ids: 1 < 3 < 0 < 4 < 2 < 5


def run_one(record, row, now=NOW, id_order=ID_ORDER):
    """One op on one record (model 0), through BOTH forms; returns (record after, status, edit or None)."""
    reg = Registry([copy.deepcopy(record)], id_order)
    arrays = ro.registry_to_arrays(reg.records)
    ops = ops_array([op_row(0, *row[0:2], **row[2])])
    cst, ced, cinfo = ro.closed_rule(*arrays, ops, now, id_order)
    st, ed, info = reg.run(ops, now)
    assert np.array_equal(st, cst) and np.array_equal(ed, ced) and info == cinfo
    got = ro.registry_from_arrays(*ro.apply_edits(*arrays, ops, ced))
    assert got[0] == ModelRecord(reg.records[0].type, reg.records[0].instance_ids, reg.records[0].load_failed_instance_ids,
                                 reg.records[0].last_used)  # (the arrays carry no lastUnloadTime)
    return reg.records[0], int(st[0]), (ed[0] if len(ed) else None)


def rec(loaded=(), failed=(), last_used=NOW - 1000):
    return ModelRecord(0, list(loaded), list(failed), last_used)


def loaded(r):
    return list(r.instance_ids.items())


def failed(r):
    return list(r.load_failed_instance_ids.items())


# ---- REGISTER ----------------------------------------------------------------------------------------------------------

def test_register_onto_an_empty_record():
    r, st, e = run_one(rec(), (0, ROP_REGISTER, dict(last_used=NOW - 5, load_time=NOW - 9)))
    assert st == ROP_EDITED and loaded(r) == [(0, NOW - 9)] and failed(r) == []
    assert e["flags"] == ROP_EDIT_PUT_LOADED | ROP_EDIT_TOUCHED and e["inserted_pos"] == 0
    assert (e["n_loaded_after"], e["n_failed_after"], e["last_used_after"], e["last_unload_after"]) == (1, 0, NOW - 5, 0)


@pytest.mark.parametrize("time", [NOW - 7, NOW + 3])
def test_register_over_an_existing_key_replaces_in_place(time):
    before = rec([(1, NOW - 8), (0, NOW - 7), (2, NOW - 6)])
    r, st, e = run_one(before, (0, ROP_REGISTER, dict(last_used=NOW - 2000, load_time=time)))
    assert st == ROP_EDITED  # the record is always submitted, also when nothing in it moved
    assert loaded(r) == [(1, NOW - 8), (0, time), (2, NOW - 6)]
    assert e["flags"] == ROP_EDIT_PUT_LOADED | ROP_EDIT_REPLACED and e["inserted_pos"] == 1 and e["n_loaded_after"] == 3


@pytest.mark.parametrize("pod,want_pos", [(1, 0), (0, 2), (5, 4)])
def test_register_in_id_order_beside_an_unresolved_entry(pod, want_pos):
    # ids in order: 3 (20), -1 (never compared), 4 (40), 2 (50)
    before = rec([(3, 1), (-1, 2), (4, 3), (2, 4)])
    r, st, e = run_one(before, (pod, ROP_REGISTER, dict(last_used=NOW, load_time=77)))
    want = [(3, 1), (-1, 2), (4, 3), (2, 4)]
    want.insert(want_pos, (pod, 77))
    assert loaded(r) == want and e["inserted_pos"] == want_pos and not e["flags"] & ROP_EDIT_REPLACED
    # first: 10 < 20 goes in front; middle: 30 goes behind the unresolved entry, in front of 40; last: 60 at the end


def test_register_behind_a_leading_unresolved_entry():
    r, _, e = run_one(rec([(-1, 2), (6, 5)]), (1, ROP_REGISTER, dict(last_used=NOW, load_time=77)))
    assert loaded(r) == [(-1, 2), (6, 5), (1, 77)] and e["inserted_pos"] == 2  # (6 lies beyond the table: unresolved too)


def test_register_removes_the_failure_record():
    r, st, e = run_one(rec([(1, 5)], [(3, 6), (0, 7)]), (0, ROP_REGISTER, dict(last_used=NOW, load_time=9)))
    assert loaded(r) == [(1, 5), (0, 9)] and failed(r) == [(3, 6)]
    assert e["flags"] == ROP_EDIT_PUT_LOADED | ROP_EDIT_REM_FAILED | ROP_EDIT_TOUCHED and (e["n_loaded_after"], e["n_failed_after"]) == (2, 1)


def test_register_last_used_zero_is_now_and_is_never_lowered():
    r, _, e = run_one(rec(last_used=NOW - 1), (0, ROP_REGISTER, dict(last_used=0, load_time=1)))
    assert r.last_used == NOW and e["flags"] & ROP_EDIT_TOUCHED
    r, _, e = run_one(rec(last_used=NOW - 1), (0, ROP_REGISTER, dict(last_used=NOW - 2, load_time=1)))
    assert r.last_used == NOW - 1 and not e["flags"] & ROP_EDIT_TOUCHED
    r, _, e = run_one(rec(last_used=NOW - 1), (0, ROP_REGISTER, dict(last_used=NOW - 1, load_time=1)))
    assert r.last_used == NOW - 1 and not e["flags"] & ROP_EDIT_TOUCHED  # `>`: an equal time does not count as raised
    r, _, e = run_one(rec(last_used=LONG_MAX), (0, ROP_REGISTER, dict(last_used=0, load_time=1)))
    assert r.last_used == LONG_MAX and e["last_used_after"] == LONG_MAX and not e["flags"] & ROP_EDIT_TOUCHED


# ---- LOAD_FAILED -------------------------------------------------------------------------------------------------------

def test_load_failed_time_mismatch_or_absent_leaves_everything():
    before = rec([(0, 5), (2, 6)], [(4, 7)])
    for pod, lt in ((0, 4), (1, 5), (4, 7)):  # wrong time; not loaded; only in the failed list
        r, st, e = run_one(before, (pod, ROP_LOAD_FAILED, dict(last_used=NOW, load_time=lt, load_complete_time=9)))
        assert st == ROP_UNCHANGED and e is None and r == before


def test_load_failed_writes_the_failure_in_id_order():
    before = rec([(1, 4), (0, 5), (2, 6)], [(3, 7), (4, 8)])
    r, st, e = run_one(before, (0, ROP_LOAD_FAILED, dict(last_used=NOW, load_time=5, load_complete_time=99)))
    assert loaded(r) == [(1, 4), (2, 6)] and failed(r) == [(3, 7), (0, 99), (4, 8)]
    assert e["flags"] == ROP_EDIT_REM_LOADED | ROP_EDIT_PUT_FAILED | ROP_EDIT_TOUCHED and e["inserted_pos"] == 1
    assert (e["n_loaded_after"], e["n_failed_after"], e["last_unload_after"]) == (2, 3, 0)  # (no updateLastUnloadTime at this site)


def test_load_failed_shutting_down_writes_no_failure():
    r, st, e = run_one(rec([(0, 5)], [(3, 7)]), (0, ROP_LOAD_FAILED, dict(flags=ROPF_SHUTTING_DOWN, last_used=NOW, load_time=5, load_complete_time=9)))
    assert st == ROP_EDITED and loaded(r) == [] and failed(r) == [(3, 7)]
    assert e["flags"] == ROP_EDIT_REM_LOADED | ROP_EDIT_TOUCHED and e["inserted_pos"] == -1


def test_load_failed_over_an_existing_failed_key():
    r, _, e = run_one(rec([(0, 5)], [(3, 7), (0, 8), (4, 9)]), (0, ROP_LOAD_FAILED, dict(last_used=NOW, load_time=5, load_complete_time=99)))
    assert failed(r) == [(3, 7), (0, 99), (4, 9)] and e["n_failed_after"] == 3
    assert e["flags"] == ROP_EDIT_REM_LOADED | ROP_EDIT_PUT_FAILED | ROP_EDIT_REPLACED | ROP_EDIT_TOUCHED and e["inserted_pos"] == 1


@pytest.mark.parametrize("op_lu", [-1, 0])
@pytest.mark.parametrize("rec_lu,want", [(0, NOW), (NOW - 50, NOW - 50)])
def test_load_failed_last_used_from_the_record(op_lu, rec_lu, want):
    # lu <= 0 takes the record's; a record at 0 hands 0 on, which updateLastUsed reads as now
    r, _, e = run_one(rec([(0, 5)], last_used=rec_lu), (0, ROP_LOAD_FAILED, dict(last_used=op_lu, load_time=5, load_complete_time=9)))
    assert r.last_used == want and bool(e["flags"] & ROP_EDIT_TOUCHED) == (rec_lu == 0)


# ---- DEREGISTER --------------------------------------------------------------------------------------------------------

BOTH = dict(loaded=[(1, 4), (0, 5), (2, 6), (5, 3)], failed=[(3, 7), (0, 8)])


@pytest.mark.parametrize("lt,lct,rem_l,rem_f", [(5, 9, True, False), (4, 8, False, True), (5, 8, True, True), (4, 9, False, False)])
def test_deregister_with_match_time(lt, lct, rem_l, rem_f):
    before = rec(**BOTH)
    r, st, e = run_one(before, (0, ROP_DEREGISTER, dict(flags=ROPF_MATCH_TIME, last_used=NOW - 1, load_time=lt, load_complete_time=lct)))
    if not (rem_l or rem_f):
        assert st == ROP_UNCHANGED and e is None and r == before
        return
    assert loaded(r) == [x for x in BOTH["loaded"] if not (rem_l and x[0] == 0)]
    assert failed(r) == [x for x in BOTH["failed"] if not (rem_f and x[0] == 0)]
    want = (ROP_EDIT_REM_LOADED | ROP_EDIT_UNLOAD_SET if rem_l else 0) | (ROP_EDIT_REM_FAILED if rem_f else 0) | ROP_EDIT_TOUCHED
    assert e["flags"] == want and e["inserted_pos"] == -1
    assert e["last_unload_after"] == (NOW if rem_l else 0) and r.last_unload_time == (NOW if rem_l else 0)  # 3 copies are left


@pytest.mark.parametrize("pod,rem_l,rem_f", [(1, True, False), (3, False, True), (0, True, True), (4, False, False)])
def test_deregister_without_match_time(pod, rem_l, rem_f):
    before = rec(**BOTH)
    r, st, e = run_one(before, (pod, ROP_DEREGISTER, dict(last_used=0, load_time=-1, load_complete_time=-1)))  # (times not looked at)
    assert st == (ROP_EDITED if rem_l or rem_f else ROP_UNCHANGED)
    if e is None:
        assert r == before
        return
    assert (e["n_loaded_after"], e["n_failed_after"]) == (4 - rem_l, 2 - rem_f)
    assert bool(e["flags"] & ROP_EDIT_REM_LOADED) == rem_l and bool(e["flags"] & ROP_EDIT_REM_FAILED) == rem_f
    assert r.last_used == NOW and e["flags"] & ROP_EDIT_TOUCHED  # :4513 passes 0 = now


@pytest.mark.parametrize("n_before,want", [(3, 0), (4, NOW), (1, 0)])
def test_deregister_last_unload_time_is_zero_up_to_two_copies_left(n_before, want):
    before = rec([(p, 10 + p) for p in range(n_before)])
    before.last_unload_time = 12345
    r, _, e = run_one(before, (0, ROP_DEREGISTER, dict(last_used=0)))
    assert e["n_loaded_after"] == n_before - 1 and e["flags"] & ROP_EDIT_UNLOAD_SET
    assert e["last_unload_after"] == want and r.last_unload_time == want


def test_deregister_of_a_failure_alone_does_not_set_the_unload_time():
    before = rec([(1, 4), (2, 5), (4, 6), (5, 7)], [(0, 8)])
    before.last_unload_time = 12345
    r, _, e = run_one(before, (0, ROP_DEREGISTER, dict(last_used=0)))
    assert e["flags"] == ROP_EDIT_REM_FAILED | ROP_EDIT_TOUCHED and e["last_unload_after"] == 0
    assert r.last_unload_time == 12345 and failed(r) == []


# ---- SCALE_DOWN --------------------------------------------------------------------------------------------------------

def test_scale_down_absent_mismatch_match():
    before = rec([(1, 4), (0, 5), (2, 6), (4, 7)], [(0, 8)], last_used=NOW - 10)
    for pod, lt in ((3, 5), (0, 6)):
        r, st, e = run_one(before, (pod, ROP_SCALE_DOWN, dict(last_used=NOW, load_time=lt)))
        assert st == ROP_UNCHANGED and e is None and r == before
    r, st, e = run_one(before, (0, ROP_SCALE_DOWN, dict(last_used=NOW - 20, load_time=5)))
    assert st == ROP_EDITED and loaded(r) == [(1, 4), (2, 6), (4, 7)]
    assert failed(r) == [(0, 8)]  # the failed entry of the same instance survives
    assert e["flags"] == ROP_EDIT_REM_LOADED | ROP_EDIT_UNLOAD_SET and e["last_unload_after"] == NOW and r.last_used == NOW - 10
    r, _, e = run_one(rec([(1, 4), (0, 5), (2, 6)]), (0, ROP_SCALE_DOWN, dict(last_used=0, load_time=5)))
    assert e["last_unload_after"] == 0 and e["flags"] == ROP_EDIT_REM_LOADED | ROP_EDIT_UNLOAD_SET | ROP_EDIT_TOUCHED and r.last_used == NOW


# ---- validation --------------------------------------------------------------------------------------------------------

def test_what_is_refused():
    reg = Registry([rec([(0, 5)]), rec()], ID_ORDER)
    good = op_row(0, 0, ROP_DEREGISTER)
    for bad in (op_row(2, 0, 0), op_row(-1, 0, 0), op_row(0, 6, 0), op_row(0, -1, 0), op_row(0, 0, 4), op_row(0, 0, -1), op_row(0, 0, 0, flags=4),
                op_row(0, 1, ROP_REGISTER)):  # the last: a second op on model 0
        before = copy.deepcopy(reg.records)
        for form in (lambda o: reg.run(o, NOW), lambda o: ro.closed_rule(*ro.registry_to_arrays(reg.records), o, NOW, ID_ORDER)):
            with pytest.raises(ro.InvalidOps):
                form(ops_array([good, bad]))
        assert reg.records == before
    with pytest.raises(ro.InvalidOps):
        reg.run(ops_array([good]), 0)
    st, ed, info = reg.run(ops_array([]), NOW)
    assert len(st) == 0 and len(ed) == 0 and info["n_edits"] == 0 and info["n_unchanged"] == 0


# ---- the two forms on constructed batches ------------------------------------------------------------------------------

def fuzz_registry(seed, pods, models):
    fleet = wl.fuzz_fleet(seed + 1300, pods=pods, models=models)
    rng = np.random.default_rng(91_000 + seed)
    reg = Registry(ro.registry_from_arrays(fleet.models, fleet.ent_pod, fleet.ent_time), fleet.pods["id_order"].copy())
    ro.seed_shapes(reg.records, reg.id_order, fleet.now, rng)
    return fleet, reg, rng


@pytest.mark.parametrize("seed,pods,models,n", [(0, 8, 300, 120), (1, 300, 2000, 700)])
def test_the_two_forms_agree_and_every_exit_occurs(seed, pods, models, n):
    fleet, reg, rng = fuzz_registry(seed, pods, models)
    n_types = int(fleet.models["type"].max()) + 1
    for batch in range(3):
        now = fleet.now + batch * 1000
        ops = ro.draw_ops(reg.records, reg.id_order, now, rng, n)
        assert len(ops) == n and len(set(ops["model"].tolist())) == n
        arrays = ro.registry_to_arrays(reg.records)
        before = copy.deepcopy(reg.records)
        census0 = rc.census_sequential(ro.to_prune_records(before), pods, n_types)
        cst, ced, cinfo = ro.closed_rule(*arrays, ops, now, reg.id_order)
        dst, ded, dinfo = reg.run(ops, now, dry=True)
        assert reg.records == before  # a dry run changes nothing
        st, ed, info = reg.run(ops, now)
        assert np.array_equal(st, cst) and np.array_equal(ed, ced) and info == cinfo
        assert np.array_equal(st, dst) and np.array_equal(ed, ded) and info == dinfo
        assert list(ed["op_index"]) == sorted(ed["op_index"])  # op order
        # the closed form's rebuild of the edited records equals what the sequential form left
        after = ro.registry_to_arrays(ro.registry_from_arrays(*ro.apply_edits(*arrays, ops, ced)))
        for g, w in zip(after, ro.registry_to_arrays(reg.records)):
            assert np.array_equal(g, w)
        # every exit of the four sites occurred: a condition on the recipe
        by_op = {int(e["op_index"]): e for e in ed}
        seen = set()
        for i, o in enumerate(ops):
            seen.update(ro.classify(before[o["model"]], o, st[i], by_op.get(i)))
        assert seen == set(ro.EXITS), sorted(set(ro.EXITS) - seen)
        assert info["n_edits"] + info["n_unchanged"] == n and all(info["n_edited_op"]) and all(info["n_unchanged_op"][1:])
        assert info["n_unchanged_op"][ROP_REGISTER] == 0
        # the census moved by exactly the entries put and removed, per instance and list
        census1 = rc.census_sequential(ro.to_prune_records(reg.records), pods, n_types)
        d_loaded, d_failed = np.zeros(pods, np.int64), np.zeros(pods, np.int64)
        for e in ed:
            pod, f = int(ops[e["op_index"]]["pod"]), int(e["flags"])
            d_loaded[pod] += bool(f & ROP_EDIT_PUT_LOADED and not f & ROP_EDIT_REPLACED) - bool(f & ROP_EDIT_REM_LOADED)
            d_failed[pod] += bool(f & ROP_EDIT_PUT_FAILED and not f & ROP_EDIT_REPLACED) - bool(f & ROP_EDIT_REM_FAILED)
        assert np.array_equal(census1[1] - census0[1], d_loaded) and np.array_equal(census1[2] - census0[2], d_failed)
        assert d_loaded.any() and d_failed.any()
        assert int(d_loaded.sum() + d_failed.sum()) == info["n_entries_added"] - info["n_entries_removed"]
        rc.assert_same_census(rc.census_closed(*after[:2], pods, n_types), census1)
        ro.seed_shapes(reg.records, reg.id_order, now + 1000, rng)  # the shapes the next batch draws from
