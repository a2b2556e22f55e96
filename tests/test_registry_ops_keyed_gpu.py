"""mmp_registry_ops_k on the device, every comparison exact: against the two-call sequence it replaces (model_ids_resolve +
registry_ops on a second context in the same state), against the sequential restatement (tests/registry_ops_keyed_model.py) for
the fifth kind and the lookup, and on its own: NO_RECORD, duplicates, the window a retirement opens between the two calls, keys
(empty, UTF-8, beyond the LDS staging region, offsets that do not start at 0), buffers and refusals, what follows an applied batch
without a commit, answers beside a writer, run-to-run identity.  Small fleets: 8 x 300 and one of 64 x 2000."""
import copy
import os
import re
import threading

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd import workload as wl
from modelmesh_amd._lib import (ROP_DEREGISTER, ROP_DROP_LOCAL, ROP_EDIT_REM_LOADED, ROP_EDIT_TOUCHED, ROP_EDIT_UNLOAD_SET, ROP_EDITED,
                                ROP_NO_RECORD, ROP_REGISTER, ROPS_APPLY, ROPS_DRY)
from modelmesh_amd.solver import MmpError, Solver
from tests import registry_ops_keyed_model as rk
from tests import registry_ops_model as ro
from tests import registry_prune_model as rp
from tests import test_status_by_id_gpu as sbg
from tests.registry_ops_keyed_model import KeyedRegistry
from tests.registry_ops_model import LONG_MAX, InvalidOps, ModelRecord, op_row, ops_array

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5
M, P = 300, 8
LONG_ID = b"L" * 17_000                         # one key longer than the 16 KB a workgroup stages
WIDE = b"W" * 200                               # 256 of these in one workgroup are 51 200 key bytes
IDS = [b"", "modèle-é".encode(), LONG_ID, b"k" * 15, b"k" * 16, b"k" * 17] + [b"m%d" % i for i in range(6, M)]
SHARED = ("n_edits", "n_unchanged", "truncated", "n_entries_added", "n_entries_removed")


def block_sizes():
    """kRopsBlock and kIdTabBlock as the source states them."""
    csrc = os.path.join(ROOT, "modelmesh_amd", "csrc")
    text = "".join(open(os.path.join(csrc, f)).read() for f in ("registry_ops_kernels.hpp", "rebalance_kernels.hpp", "pod_events_kernels.hpp",
                                                                "keyed_kernels.hpp"))
    val = lambda name: re.search(r"constexpr int " + name + r" = (\w+);", text).group(1)  # noqa: E731
    rops = val("kRopsBlock")
    return int(val(rops) if not rops.isdigit() else rops), int(val("kIdTabBlock")), int(val("kKeyedLdsBytes"))


ROPS_BLOCK, IDTAB_BLOCK, LDS_BYTES = block_sizes()
SIZES = sorted({0, 1, 63, 64, 65, ROPS_BLOCK - 1, ROPS_BLOCK, ROPS_BLOCK + 1, IDTAB_BLOCK - 1, IDTAB_BLOCK, IDTAB_BLOCK + 1})


def test_the_block_sizes_are_the_ones_the_sizes_were_chosen_for():
    assert (ROPS_BLOCK, IDTAB_BLOCK, LDS_BYTES) == (256, 256, 16384) == (_lib.ROPS_BLOCK, 256, 16384)
    assert SIZES == [0, 1, 63, 64, 65, 255, 256, 257] and len(LONG_ID) > LDS_BYTES and 256 * len(WIDE) > LDS_BYTES


# ---- the world by row: the fuzz fleet of the older file, its rows named by IDS ------------------------------------------------

def row_world(seed=0, pods=P, models=M, ids=None):
    fleet = wl.fuzz_fleet(seed + 1300, pods=pods, models=models)
    rng = np.random.default_rng(97_000 + seed)
    recs = ro.registry_from_arrays(fleet.models, fleet.ent_pod, fleet.ent_time)
    ro.seed_shapes(recs, fleet.pods["id_order"], int(fleet.now), rng)
    for i in (9, 38, 67):                         # three deleted records: the empty row
        recs[i] = ModelRecord(0, [], [], 0)
    fleet.models, fleet.ent_pod, fleet.ent_time = ro.registry_to_arrays(recs)
    ids = ids if ids is not None else (IDS if models == M else [b"id-%d" % i for i in range(models)])
    return fleet, KeyedRegistry(ids, recs, fleet.pods["id_order"].copy()), rng


def loaded(fleet, ids):
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    s.load_fleet(fleet)
    s.model_ids_load(ids)
    return s


def untouched(x):
    """An output buffer still holds nothing but the fill byte."""
    return set(x.tobytes()) <= {FILL}


def same_registry(s, k):
    got = rp.compact(*s.get_models())
    want = ro.registry_to_arrays(k.records_by_row())
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def same_contexts(s1, s2):
    for a, b in zip(rp.compact(*s1.get_models()), rp.compact(*s2.get_models())):
        assert a.tobytes() == b.tobytes()


def same_as_model(got, want, what=""):
    (idx, st, ed, info), (widx, wst, wed, winfo) = got, want
    assert np.array_equal(idx, widx), (what, idx[:8], widx[:8])
    assert st.dtype == wst.dtype and np.array_equal(st, wst), (what, st[:8], wst[:8])
    assert ed.dtype == wed.dtype and ed.tobytes() == wed.tobytes(), (what, ed[:4], wed[:4])
    for f in SHARED + ("n_no_record",):
        assert int(info[f]) == winfo[f], (what, f, info, winfo)
    assert list(info["n_edited_op"]) == winfo["n_edited_op"] and list(info["n_unchanged_op"]) == winfo["n_unchanged_op"], (what, info, winfo)


def one_batch(s, k, ops, keys, now, apply=True, **kw):
    """The same batch on the device and in the restatement (which edits `k` when the device applies); every output equal."""
    got = s.registry_ops_k(ops, keys, now, apply=apply, **kw)
    want = k.run(ops, keys, now, dry=not apply)
    same_as_model(got, want)
    return got


@pytest.fixture(scope="module")
def small():
    return row_world()


# ---- equality with the two-call sequence --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pair(small):
    """Two contexts in the same state: `a` gets the one call, `b` the two calls it replaces; both advance together."""
    fleet, k0, _ = small
    a, b = loaded(fleet, IDS), loaded(fleet, IDS)
    yield a, b, copy.deepcopy(k0), int(fleet.now)
    a.close()
    b.close()


def two_calls(s, ops, keys, now, flags):
    """model_ids_resolve, then registry_ops on the rows it answered (live ones: a host skips what it knows to be deleted)."""
    ops = ops.copy()
    ops["model"] = s.model_ids_resolve(keys)
    return ops["model"].copy(), s.registry_ops_raw(ops, now, flags, max(len(ops), 1))


@pytest.mark.parametrize("n", SIZES)
def test_the_call_with_keys_equals_resolve_plus_registry_ops(pair, n):
    a, b, k, now = pair
    rng = np.random.default_rng(1000 + n)
    live = [i for i, key in enumerate(k.ids) if k.get(key) is not None]
    for flags in (0, ROPS_DRY, ROPS_APPLY):
        old = ro.draw_ops([k.registry[k.ids[i]] for i in live], k.id_order, now, rng, n)   # kinds 0..3 on live records
        assert len(old) == n
        keys = [k.ids[live[int(o["model"])]] for o in old]
        ops = old.copy()
        ops["model"] = -12345                                                              # by key the field is ignored
        idx, st, ed, info, rc = a.registry_ops_k_raw(ops, keys, now, flags, max(n, 1), fill=FILL)
        assert rc == 0
        widx, (wst, wed, winfo) = two_calls(b, old, keys, now, flags)
        assert np.array_equal(idx, widx) and st.tobytes() == wst.tobytes() and ed.tobytes() == wed.tobytes()
        for f in SHARED:
            assert int(info[f]) == int(winfo[f]), (f, info, winfo)
        assert list(info["n_edited_op"][:4]) == list(winfo["n_edited_op"]) and list(info["n_unchanged_op"][:4]) == list(winfo["n_unchanged_op"])
        assert not info["n_edited_op"][4:].any() and not info["n_unchanged_op"][4:].any() and int(info["n_no_record"]) == 0
        assert n < 63 or int(info["n_edits"]) > 0
        same_as_model((idx, st, ed, info), k.run(ops, keys, now, dry=flags != ROPS_APPLY), (n, flags))
        same_contexts(a, b)
        same_registry(a, k)
        # the by-row form (keys NULL) passes the same comparison
        rows = ops.copy()
        rows["model"] = widx
        ridx, rst, red, rinfo, rc = a.registry_ops_k_raw(rows, None, now + 1, flags, max(n, 1), fill=FILL)
        assert rc == 0
        bst, bed, binfo = b.registry_ops_raw(rows, now + 1, flags, max(n, 1))
        assert np.array_equal(ridx, widx) and rst.tobytes() == bst.tobytes() and red.tobytes() == bed.tobytes()
        for f in SHARED:
            assert int(rinfo[f]) == int(binfo[f])
        assert list(rinfo["n_edited_op"][:4]) == list(binfo["n_edited_op"]) and int(rinfo["n_no_record"]) == 0
        same_as_model((ridx, rst, red, rinfo), k.run(ops, keys, now + 1, dry=flags != ROPS_APPLY), (n, flags, "by row"))
        same_contexts(a, b)


def test_the_old_call_still_refuses_kind_four_and_by_row_the_new_one_takes_it(small):
    fleet, k0, _ = small
    k, now = copy.deepcopy(k0), int(fleet.now)
    s = loaded(fleet, IDS)
    try:
        row = next(i for i, key in enumerate(k.ids) if k.get(key) is not None and k.get(key).instance_ids)
        pod = next(iter(k.get(k.ids[row]).instance_ids))
        ops = ops_array([op_row(row, pod, ROP_DROP_LOCAL, last_used=0)])
        with pytest.raises(MmpError) as ei:
            s.registry_ops_raw(ops, now, ROPS_APPLY, 4)
        assert ei.value.code == _lib.MMP_EINVAL
        same_registry(s, k)
        idx, st, ed, info = s.registry_ops_k(ops, None, now)             # by row: the fifth kind for a host with an id map
        same_as_model((idx, st, ed, info), k.run(ops, [k.ids[row]], now))
        assert ed[0]["flags"] & ROP_EDIT_REM_LOADED and not ed[0]["flags"] & ROP_EDIT_UNLOAD_SET
        same_registry(s, k)
        # by row an empty row is an ordinary record, as in mmp_registry_ops: it is edited, not NO_RECORD
        idx, st, ed, info = s.registry_ops_k(ops_array([op_row(9, 1, ROP_DROP_LOCAL, last_used=5)]), None, now, apply=False)
        assert list(st) == [ROP_EDITED] and ed[0]["last_used_after"] == 5 and int(info["n_no_record"]) == 0
    finally:
        s.close()


# ---- DROP_LOCAL against the sequential model ----------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 120, 257])
def test_drop_local_alone_and_mixed_with_the_four_other_kinds(small, n):
    fleet, k0, _ = small
    k, now, rng = copy.deepcopy(k0), int(fleet.now), np.random.default_rng(n)
    s = loaded(fleet, IDS)
    try:
        seen = set()
        live = [key for key in k.ids if k.get(key) is not None]
        for batch in range(2):
            ops, keys = rk.draw_ops_k(k, now + batch, rng, n)
            before = copy.deepcopy(k) if n > 1 else k
            idx, st, ed, info = one_batch(s, k, ops, keys, now + batch)
            if n > 1:
                for i, (o, key) in enumerate(zip(ops, keys)):
                    seen.update(rk.classify_k(before, o, key, st[i]))
                assert all(int(x) > 0 for x in info["n_edited_op"][:5]) and int(info["n_no_record"]) >= 4
            same_registry(s, k)
        alone = ops_array([op_row(0, int(rng.integers(0, P)), ROP_DROP_LOCAL, last_used=int(rng.choice([0, now - 50, now]))) for _ in range(n)])
        got = one_batch(s, k, alone, [live[int(i)] for i in rng.permutation(len(live))[:n]], now, max_edits=4)
        assert got[1].all() and int(got[3]["n_edited_op"][ROP_DROP_LOCAL]) == n and not (got[2]["flags"] & ROP_EDIT_UNLOAD_SET).any()
        same_registry(s, k)
        assert n == 1 or seen == set(rk.EXITS_K), set(rk.EXITS_K) - seen
    finally:
        s.close()


def hand_world():
    """The records of the by-hand boundaries (tests/test_registry_ops_keyed_model.py), one per id, on a 6-instance table."""
    now = 1_700_000_000_000
    rec = lambda l=(), f=(), lu=now - 1000: ModelRecord(0, list(l), list(f), lu)  # noqa: E731
    recs = {b"present": rec([(1, 4), (0, 5), (2, 6)]), b"absent": rec([(1, 4), (2, 6)], [(3, 7)]), b"bare": rec(),
            b"c1": rec([(1, 101)]), b"c2": rec([(1, 101), (3, 103)]), b"c3": rec([(1, 101), (3, 103), (0, 100)]),
            b"c4": rec([(1, 101), (3, 103), (0, 100), (4, 104)]),
            b"d1": rec([(1, 101)]), b"d2": rec([(1, 101), (3, 103)]), b"d3": rec([(1, 101), (3, 103), (0, 100)]),
            b"d4": rec([(1, 101), (3, 103), (0, 100), (4, 104)]),
            b"failure": rec([(1, 4), (0, 5)], [(3, 7), (0, 8)]), b"only-failure": rec([(1, 4)], [(0, 8)]),
            b"unresolved": rec([(3, 1), (-1, 2), (9, 3), (2, 4)]),
            b"lu-zero": rec([(0, 5)]), b"lu-lower": rec([(0, 5)]), b"lu-equal": rec([(0, 5)]), b"lu-higher": rec([(0, 5)]),
            b"at-max": rec([(0, 5)], lu=LONG_MAX), b"deleted": rec(lu=0)}
    fleet = wl.fuzz_fleet(1300, pods=6, models=1)
    fleet.pods["id_order"] = np.array([30, 10, 50, 20, 40, 60], np.uint32)
    fleet.models, fleet.ent_pod, fleet.ent_time = ro.registry_to_arrays(list(recs.values()))
    return fleet, KeyedRegistry(list(recs), list(recs.values()), fleet.pods["id_order"].copy()), now


def test_every_by_hand_boundary_is_replayed_on_the_device():
    fleet, k, now = hand_world()
    s = loaded(fleet, k.ids)
    try:
        if not np.array_equal(s.get_pods()["id_order"], k.id_order):
            k.id_order = s.get_pods()["id_order"].copy()   # (the committed order is the library's to state; no op here inserts)
        d = lambda pod, lu=0, kind=ROP_DROP_LOCAL: op_row(0, pod, kind, last_used=lu)  # noqa: E731
        cases = [(b"present", d(0, now)), (b"absent", d(0, now - 2000)), (b"bare", d(4, now - 2000)),
                 (b"c1", d(1, now - 2000)), (b"c2", d(3, now - 2000)), (b"c3", d(0, now - 2000)), (b"c4", d(4, now - 2000)),
                 (b"d1", d(1, now - 2000, ROP_DEREGISTER)), (b"d2", d(3, now - 2000, ROP_DEREGISTER)), (b"d3", d(0, now - 2000, ROP_DEREGISTER)),
                 (b"d4", d(4, now - 2000, ROP_DEREGISTER)),
                 (b"failure", d(0, now)), (b"only-failure", d(0, now)), (b"unresolved", d(2, now)),
                 (b"lu-zero", d(0, 0)), (b"lu-lower", d(0, now - 1001)), (b"lu-equal", d(0, now - 1000)), (b"lu-higher", d(0, now - 999)),
                 (b"at-max", d(0, 0)), (b"deleted", d(1, now)), (b"never-registered", d(1, now))]
        ops, keys = ops_array([c[1] for c in cases]), [c[0] for c in cases]
        idx, st, ed, info = one_batch(s, k, ops, keys, now)
        by_key = {keys[int(e["op_index"])]: e for e in ed}
        assert list(st) == [ROP_EDITED] * 19 + [ROP_NO_RECORD] * 2 and list(idx[-2:]) == [len(k.ids) - 1, -1]
        assert by_key[b"present"]["flags"] == ROP_EDIT_REM_LOADED | ROP_EDIT_TOUCHED and by_key[b"absent"]["flags"] == 0
        assert by_key[b"bare"]["flags"] == 0 and (by_key[b"bare"]["n_loaded_after"], by_key[b"bare"]["n_failed_after"]) == (0, 0)
        for c in (1, 2, 3, 4):                    # the only copy, one of 2 / 3 / 4: lastUnloadTime only under DEREGISTER
            e, de = by_key[b"c%d" % c], by_key[b"d%d" % c]
            assert e["flags"] == ROP_EDIT_REM_LOADED and e["last_unload_after"] == 0 and e["n_loaded_after"] == c - 1
            assert de["flags"] == ROP_EDIT_REM_LOADED | ROP_EDIT_UNLOAD_SET and de["last_unload_after"] == (now if c - 1 > 2 else 0)
        assert (by_key[b"failure"]["n_loaded_after"], by_key[b"failure"]["n_failed_after"]) == (1, 2)
        assert by_key[b"only-failure"]["flags"] == ROP_EDIT_TOUCHED and by_key[b"unresolved"]["n_loaded_after"] == 3
        assert [int(by_key[x]["last_used_after"]) for x in (b"lu-zero", b"lu-lower", b"lu-equal", b"lu-higher", b"at-max")] == \
            [now, now - 1000, now - 1000, now - 999, LONG_MAX]
        assert [bool(by_key[x]["flags"] & ROP_EDIT_TOUCHED) for x in (b"lu-zero", b"lu-lower", b"lu-equal", b"lu-higher", b"at-max")] == \
            [True, False, False, True, False]
        assert (ed["inserted_pos"] == -1).all() and int(info["n_entries_removed"]) == 16 and int(info["n_entries_added"]) == 0
        same_registry(s, k)
    finally:
        s.close()


# ---- NO_RECORD, the window: worlds by key, where events and retirements can follow ----------------------------------------------

def key_world(n=40):
    """n records by key over the 8 instances of the status file's wire world, lists in id order, entries at distinct times."""
    io = sbg.W.fleet.pods["id_order"]
    order = sorted(range(P), key=lambda p: io[p])
    ids = [b"key-%d" % i for i in range(n)]
    recs = [ModelRecord(0, [(p, 1000 * i + j) for j, p in enumerate(order) if (i + j) % 3 == 0],
                        [(order[(i + 5) % P], 1000 * i + 500)] if i % 4 == 0 else [], i + 1) for i in range(n)]
    s = sbg.W.solver()
    status, _ = s.ingest_models_json([sbg.value_of(r) for r in recs])
    assert not status.any()
    s.model_ids_load(ids)
    return s, KeyedRegistry(ids, recs, io.copy())


def event(s, k, key, mr):
    """One registry event on both sides; mr None: ENTRY_DELETED."""
    s.models_events_json([key], [sbg.value_of(mr) if mr else ""], np.array([mr is None], np.uint8), True)
    k.delete(key) if mr is None else k.put(key, copy.deepcopy(mr))


def test_an_unknown_id_a_deleted_id_and_the_same_id_registered_again():
    s, k = key_world()
    try:
        now = 5_000_000
        same_registry(s, k)
        pod = next(iter(k.get(b"key-6").instance_ids))
        op = ops_array([op_row(0, pod, ROP_DROP_LOCAL, last_used=0)])
        idx, st, ed, info = one_batch(s, k, op, [b"never-seen"], now)
        assert (idx[0], st[0], len(ed), int(info["n_no_record"]), int(info["n_unchanged"])) == (-1, ROP_NO_RECORD, 0, 1, 0)
        event(s, k, b"key-6", None)
        idx, st, ed, info = one_batch(s, k, op, [b"key-6"], now)
        assert (idx[0], st[0], len(ed)) == (6, ROP_NO_RECORD, 0)
        same_registry(s, k)
        event(s, k, b"key-6", ModelRecord(0, [(pod, 77)], [], 9))
        idx, st, ed, info = one_batch(s, k, op, [b"key-6"], now)
        assert (idx[0], st[0], int(ed[0]["model"]), int(ed[0]["n_loaded_after"])) == (6, ROP_EDITED, 6, 0)
        same_registry(s, k)
        # a batch that is all NO_RECORD: no edits, registry untouched, and the next call works (the map is clean)
        event(s, k, b"key-7", None)
        n = ROPS_BLOCK + 3
        keys = [b"key-7", b"ghost", b"ghost"] + [b"ghost-%d" % i for i in range(n - 3)]
        ops = ops_array([op_row(i % 40, i % P, i % 5, last_used=0) for i in range(n)])
        resident = [a.copy() for a in s.get_models()]
        idx, st, ed, info = one_batch(s, k, ops, keys, now)
        assert (st == ROP_NO_RECORD).all() and len(ed) == 0 and int(info["n_no_record"]) == n and int(info["n_edits"]) == 0
        assert not info["n_edited_op"].any() and not info["n_unchanged_op"].any() and idx[0] == 7 and (idx[1:] == -1).all()
        for x, y in zip(resident, s.get_models()):
            assert x.tobytes() == y.tobytes()
        live = [key for key in k.ids if k.get(key) is not None]
        one_batch(s, k, ops_array([op_row(0, i % P, i % 5, last_used=0, load_time=3) for i in range(len(live))]), live, now)
        same_registry(s, k)
    finally:
        s.close()


def test_two_positions_on_one_row_are_refused_and_colliding_hashes_are_not(monkeypatch):
    fleet, k0, _ = row_world()
    k, now = copy.deepcopy(k0), int(fleet.now)
    s = loaded(fleet, IDS)
    try:
        live = [key for key in k.ids if k.get(key) is not None]
        good = [op_row(0, i % P, ROP_DROP_LOCAL, last_used=0) for i in range(281)]
        resident = [a.copy() for a in s.get_models()]
        for keys in (live[:280] + [live[3]], live[:5] + [live[2]], [live[0], live[0]]):   # two workgroups apart; in one wave; alone
            for flags in (ROPS_APPLY, 0):
                assert len(good[:len(keys)]) == len(keys)
                out = s.registry_ops_k_raw(ops_array(good[:len(keys)]), keys, now, flags, 1024, fill=FILL)
                assert out[4] == _lib.MMP_EINVAL and all(untouched(a) for a in out[:4])
            with pytest.raises(InvalidOps):
                k.run(ops_array(good[:len(keys)]), keys, now)
        for x, y in zip(resident, s.get_models()):
            assert x.tobytes() == y.tobytes()
        one_batch(s, k, ops_array(good[:280]), live[:280], now)          # the next call is correct: the map was left clean
        same_registry(s, k)
    finally:
        s.close()
    monkeypatch.setenv("MMP_MODEL_ID_HASH_BITS", "0")                    # every id shares one hash: told apart by their bytes
    k = copy.deepcopy(k0)
    s = loaded(fleet, IDS)
    try:
        live = [key for key in k.ids if k.get(key) is not None]
        idx, st, ed, info = one_batch(s, k, ops_array(good[:280]), live[:280], now)
        assert len(set(idx.tolist())) == 280 and int(info["n_edits"]) == 280
        ops, keys = rk.draw_ops_k(k, now, np.random.default_rng(8), 257)
        one_batch(s, k, ops, keys, now)
        same_registry(s, k)
    finally:
        s.close()


def test_ops_by_key_follow_the_renumbering_of_a_retirement():
    s, k = key_world()
    try:
        now = 5_000_000
        gone = [b"key-2", b"key-3", b"key-11", b"key-30"]
        for key in gone:
            event(s, k, key, None)
        rows = [k.row(key) for key in gone]
        remap = s.models_retire(rows)
        k.retire(rows)
        assert remap[4] == 2 and remap[39] == 35 and len(k.ids) == 36
        keys = [b"key-4", b"key-39", b"key-2", b"key-12", b"key-0", b"key-31"]
        ops = ops_array([op_row(4, next(iter(k.get(key).instance_ids), 0) if k.get(key) else 0, kind, last_used=0, load_time=1)
                         for key, kind in zip(keys, (ROP_DROP_LOCAL, ROP_DROP_LOCAL, ROP_DROP_LOCAL, ROP_REGISTER, ROP_DEREGISTER, ROP_DROP_LOCAL))])
        idx, st, ed, info = one_batch(s, k, ops, keys, now)
        assert idx.tolist() == [2, 35, -1, 9, 0, 27] and st[2] == ROP_NO_RECORD
        assert ed["model"].tolist() == [2, 35, 9, 0, 27]               # the records the ids name under the new numbering
        same_registry(s, k)
    finally:
        s.close()


# ---- keys ----------------------------------------------------------------------------------------------------------------------

def test_the_empty_key_utf8_keys_beyond_the_lds_region_and_offsets_that_do_not_start_at_zero(small):
    fleet, k0, _ = small
    k, now = copy.deepcopy(k0), int(fleet.now)
    s = loaded(fleet, IDS)
    try:
        drop = lambda i: op_row(0, i % P, ROP_DROP_LOCAL, last_used=0)  # noqa: E731
        keys = [b"", "modèle-é".encode(), "modèle-e".encode(), b"k" * 14, b"k" * 15, b"k" * 16, b"k" * 17, b"k" * 18]
        idx, st, ed, info = one_batch(s, k, ops_array([drop(i) for i in range(8)]), keys, now)
        assert idx.tolist() == [0, 1, -1, -1, 3, 4, 5, -1] and (st[[2, 3, 7]] == ROP_NO_RECORD).all() and (st[[0, 1, 4, 5, 6]] == ROP_EDITED).all()
        # one key longer than the staging region: its workgroup reads in place, the next one stages
        live = [key for key in k.ids if k.get(key) is not None and key != LONG_ID]
        keys = [LONG_ID] + live[:IDTAB_BLOCK + 20]
        idx, st, ed, info = one_batch(s, k, ops_array([drop(i) for i in range(len(keys))]), keys, now + 1)
        assert idx[0] == 2 and st.all() and (st == ROP_EDITED).all()
        # a workgroup whose keys together exceed it (unknown ids: no record, not duplicates), beside one that fits; then the same
        # live keys in a batch small enough to be staged: the same rows, the same evaluation
        keys = [WIDE] * 200 + live[100:156] + live[160:200]
        ops = ops_array([drop(i) for i in range(len(keys))])
        in_place = one_batch(s, k, ops, keys, now + 2, apply=False)
        assert (in_place[1][:200] == ROP_NO_RECORD).all() and (in_place[1][200:] == ROP_EDITED).all()
        staged = one_batch(s, k, ops[200:], keys[200:], now + 2, apply=False)
        assert np.array_equal(staged[0], in_place[0][200:]) and np.array_equal(staged[1], in_place[1][200:])
        a, b = staged[2].copy(), in_place[2].copy()
        b["op_index"] -= 200
        assert a.tobytes() == b.tobytes()
        # key_off[0] != 0: the bytes in front belong to somebody else
        blob = b"junk-in-front" + b"".join(live[:3])
        off = np.cumsum([13] + [len(x) for x in live[:3]]).astype(np.int32)
        ops = ops_array([drop(i) for i in range(3)])
        idx, st, ed, info, rc = s.registry_ops_k_raw(ops, live[:3], now + 3, 0, 8, key_off=off, blob=blob)
        assert rc == 0
        same_as_model((idx, st, ed, info), k.run(ops, live[:3], now + 3, dry=True))
        same_registry(s, k)
    finally:
        s.close()


# ---- buffers, refusals -----------------------------------------------------------------------------------------------------------

def test_truncation_null_buffers_and_every_refusal_of_the_header(small):
    fleet, k0, rng0 = small
    k, now = copy.deepcopy(k0), int(fleet.now)
    s = loaded(fleet, IDS)
    try:
        ops, keys = rk.draw_ops_k(k, now, np.random.default_rng(4), 200)
        widx, wst, wed, winfo = k.run(ops, keys, now, dry=True)
        assert len(wed) > 40
        for flags in (ROPS_APPLY, 0):
            for cap in (3, len(wed) - 1, 0):                 # too small, one short, no buffer: the prefix, the totals, nothing applied
                idx, st, ed, info, rc = s.registry_ops_k_raw(ops, keys, now, flags, cap)
                assert rc == 0 and int(info["truncated"]) == 1 and ed.tobytes() == wed[:cap].tobytes()
                same_as_model((idx, st, wed, info), (widx, wst, wed, dict(winfo, truncated=1)))
                same_registry(s, k)
        idx, st, ed, info, rc = s.registry_ops_k_raw(ops, keys, now, 0, len(wed), fill=FILL, null_status=True, null_idx=True)
        assert rc == 0 and (st == FILL).all() and (idx.view(np.uint8) == FILL).all()
        same_as_model((widx, wst, ed, info), (widx, wst, wed, winfo))
        for cap in (0, 4):                                   # n = 0: a valid call with empty outputs, by key and by row
            for kk in ([], None):
                idx, st, ed, info, rc = s.registry_ops_k_raw(ops[:0], kk, now, ROPS_APPLY, cap, fill=FILL)
                assert rc == 0 and len(st) == 0 and len(ed) == 0 and not info.tobytes().strip(b"\0")
        one_batch(s, k, ops, keys, now, max_edits=2)         # the veneer regrows from 2
        same_registry(s, k)

        resident = [a.copy() for a in s.get_models()]
        live = [key for key in k.ids if k.get(key) is not None]
        good, gk = [op_row(0, i % P, ROP_DROP_LOCAL, last_used=0) for i in range(270)], live[:270]
        E, A0 = _lib.MMP_EINVAL, dict(now=now, flags=ROPS_APPLY, max_edits=512)
        mono = np.arange(272, dtype=np.int32)
        mono[100] = 98
        refusals = [
            ("a pod beyond the table", dict(ops=good + [op_row(0, P, 0)], keys=gk + [live[270]])),
            ("a negative pod", dict(ops=good + [op_row(0, -1, 0)], keys=gk + [live[270]])),
            ("kind 5", dict(ops=good + [op_row(0, 0, 5)], keys=gk + [live[270]])),
            ("kind -1", dict(ops=good + [op_row(0, 0, -1)], keys=gk + [live[270]])),
            ("an unknown flag bit", dict(ops=good + [op_row(0, 0, 0, flags=4)], keys=gk + [live[270]])),
            ("SHUTTING_DOWN on DROP_LOCAL", dict(ops=good + [op_row(0, 0, ROP_DROP_LOCAL, flags=1)], keys=gk + [live[270]])),
            ("MATCH_TIME on DROP_LOCAL", dict(ops=good + [op_row(0, 0, ROP_DROP_LOCAL, flags=2)], keys=gk + [live[270]])),
            ("now = 0", dict(ops=good, keys=gk, now=0)), ("now < 0", dict(ops=good, keys=gk, now=-5)),
            ("APPLY | DRY", dict(ops=good, keys=gk, flags=ROPS_APPLY | ROPS_DRY)), ("an unknown call flag", dict(ops=good, keys=gk, flags=4)),
            ("offsets not monotone", dict(ops=good + [op_row(0, 0, 0)], keys=gk + [live[270]], key_off=mono)),
            ("keys without key_off", dict(ops=good, keys=gk, null_off=True)),
            ("key_off without keys", dict(ops=good, keys=gk, null_keys=True)),
            ("two keys on one live row", dict(ops=good + [op_row(0, 1, ROP_DEREGISTER)], keys=gk + [gk[7]])),
            ("a NULL info", dict(ops=good, keys=gk, null_info=True)), ("NULL ops with n > 0", dict(ops=good, keys=gk, null_ops=True)),
            ("a negative capacity", dict(ops=good, keys=gk, max_edits=-1)),
            ("by row: a model beyond the registry", dict(ops=[op_row(M, 0, 0)], keys=None)),
            ("by row: a negative model", dict(ops=[op_row(-1, 0, ROP_DROP_LOCAL)], keys=None)),
            ("by row: one model twice", dict(ops=[op_row(20, 0, 0), op_row(20, 1, ROP_DROP_LOCAL)], keys=None)),
        ]
        for what, kw in refusals:
            a = dict(A0, **kw)
            out = s.registry_ops_k_raw(ops_array(a.pop("ops")), a.pop("keys"), a.pop("now"), a.pop("flags"), a.pop("max_edits"), fill=FILL, **a)
            assert out[4] == E, what
            assert all(untouched(x) for x in out[:4]), what                         # nothing written
            for x, y in zip(resident, s.get_models()):
                assert x.tobytes() == y.tobytes(), what                             # nothing changed
        one_batch(s, k, ops_array(good), gk, now)                                    # the map was left all -1
        same_registry(s, k)
    finally:
        s.close()
    for keys, want in (([b"a"], _lib.MMP_ESTATE), (None, _lib.MMP_ESTATE)):         # before the first commit
        s = Solver(6553, 60_000)
        try:
            assert s.registry_ops_k_raw(ops_array([op_row(0, 0, 0)]), keys, 1_700_000_000_000, 0, 4)[4] == want
        finally:
            s.close()
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)                        # committed, but no model ids
    try:
        s.load_fleet(fleet)
        assert s.registry_ops_k_raw(ops_array([op_row(0, 0, 0)]), [b"a"], now, 0, 4)[4] == _lib.MMP_ESTATE
        assert s.registry_ops_k_raw(ops_array([op_row(0, 0, ROP_DROP_LOCAL)]), None, now, 0, 4)[4] == 0   # by row needs none
    finally:
        s.close()


# ---- downstream, writer, rerun -------------------------------------------------------------------------------------------------

def test_after_an_apply_the_census_and_status_by_id_see_the_edited_records():
    fleet, k, rng = row_world(5, 64, 2000)
    s = loaded(fleet, k.ids)
    try:
        now = int(fleet.now)
        before = s.registry_census()
        ops, keys = rk.draw_ops_k(k, now, rng, 700)
        idx, st, ed, info = one_batch(s, k, ops, keys, now)
        assert int(info["n_edits"]) > 300 and int(info["n_entries_removed"]) > 50 and int(info["n_entries_added"]) > 20
        after = s.registry_census()
        moved = int(after[1].sum() + after[2].sum()) - int(before[1].sum() + before[2].sum())
        assert moved == int(info["n_entries_added"]) - int(info["n_entries_removed"])
        same_registry(s, k)
        edited = [keys[int(e["op_index"])] for e in ed]
        ridx, rows, copies = s.models_status_k(edited, now)
        assert np.array_equal(ridx, ed["model"])
        for e, key, r in zip(ed, edited, rows):
            mr = k.registry[key]
            pods = sorted(copies["pod"][r["copy_off"]: r["copy_off"] + r["n_not_checked"] + r["n_failed"]].tolist())
            assert (int(r["n_not_checked"]), int(r["n_failed"])) == (int(e["n_loaded_after"]), int(e["n_failed_after"]))
            assert pods == sorted(list(mr.instance_ids) + list(mr.load_failed_instance_ids))
    finally:
        s.close()


def test_two_hundred_calls_beside_a_writer_that_joins_new_ids():
    s, k = key_world()
    try:
        now, stop, errors = 5_000_000, threading.Event(), []
        joiner_rec = ModelRecord(0, [(1, 5)], [], 3)

        def writer():
            try:
                i = 0
                while not stop.is_set() and i < 2000:
                    s.models_events_json([b"joined-%d" % i], [sbg.value_of(joiner_rec)], np.zeros(1, np.uint8), True)
                    i += 1
            except Exception as e:  # noqa: BLE001
                errors.append(e)
        t = threading.Thread(target=writer)
        t.start()
        try:
            rng = np.random.default_rng(3)
            base = list(k.ids)
            for call in range(200):                          # joining ids never renumber existing rows: the model knows the answer
                pick = [base[int(i)] for i in rng.permutation(len(base))[:12]] + [b"never-joins"]
                ops = ops_array([op_row(0, int(rng.integers(0, P)), int(rng.integers(0, 5)), last_used=0, load_time=int(rng.integers(0, 3)))
                                 for _ in pick])
                got = s.registry_ops_k(ops, pick, now + call, apply=call % 2 == 0)
                same_as_model(got, k.run(ops, pick, now + call, dry=call % 2 != 0), call)
        finally:
            stop.set()
            t.join()
        assert not errors, errors
        rows = rp.compact(*s.get_models())[0]
        assert len(rows) > len(k.ids)                        # the writer did get in between
        want = ro.registry_to_arrays(k.records_by_row())[0]
        for f in ("n_loaded", "n_failed", "last_used"):
            assert np.array_equal(rows[f][:len(want)], want[f]), f
    finally:
        s.close()


def test_the_same_batch_on_the_same_state_twice_is_byte_identical(small):
    fleet, k0, _ = small
    now = int(fleet.now)
    s = loaded(fleet, IDS)
    try:
        ops, keys = rk.draw_ops_k(k0, now, np.random.default_rng(21), 257)
        a = s.registry_ops_k_raw(ops, keys, now, 0, 300, fill=FILL)
        b = s.registry_ops_k_raw(ops, keys, now, 0, 300, fill=0x3C)
        assert a[4] == b[4] == 0 and int(a[3]["n_edits"]) > 50
        for x, y in zip(a[:4], b[:4]):
            assert x.tobytes() == y.tobytes()
        same_registry(s, k0)
    finally:
        s.close()
