"""mmp_vmodels_write_json on the device against tests/vmodel_write_model.py, byte for byte on values, offsets and rows, over a
small fleet loaded by key (8 instances x 300 models) whose ids and records are read back from the device: batches of 0, 1, 63,
64, 65 and 257 requests, stored values on both sides of the 2 048-byte tile at every dword alignment, values of 63 .. 130 members,
compared and rendered ids of 0 .. 200 bytes that differ in their first, last and 64th byte, request strings that need every
escape, the parser's own verdict on the malformed and edge lists of tests/vmodel_fixtures.py, both id hashes masked to 0 and 4
bits, one value 64 times in a call, every rendered value fed back through mmp_vmodels_events_json, the dec spans against the old
values and the rows against mmp_model_ids_resolve, the sizing protocol, every refusal with the outputs untouched, two runs, 200
calls beside a thread that sends registry events, and the reference's own vmodel tests (tests/golden/vmodel_kats.json) through
tests/vmodel_minimesh.py with the device answering.  The batches are tests/vmodel_write_fixtures.py's; tests/test_vmodel_write_model.py
asserts, without a device, that each holds every class, op and flag."""
import ctypes as C
import json
import os
import threading

import numpy as np
import pytest

from modelmesh_amd import _lib
from tests import vmodel_fixtures as vf
from tests import vmodel_minimesh as minimesh
from tests import vmodel_model as vm
from tests import vmodel_write_fixtures as fx
from tests import vmodel_write_model as wm
from tests.ingest_model import REJECT
from tests.model_events_fixtures import World

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -5
FILL = 0xA5
WORLD = World(0)
REG_VALUES = vf.registry_values(WORLD.pod_ids, fx.M)[0]


def start():
    """A committed 8-instance context whose registry holds the 300 records by key."""
    s = WORLD.solver()
    assert not len(s.ingest_models_json([])[0])
    s.model_ids_load([])
    status, rows, _, n_app = s.models_events_json(fx.MIDS, REG_VALUES, None, True)
    assert not status.any() and n_app == fx.M and list(rows) == list(range(fx.M))
    return s


def registry_of(s):
    rows = s.get_models()[0]
    return vm.Registry(s.model_ids_get(), [(r["n_loaded"], r["n_failed"], r["last_used"], r["type"]) for r in rows])


def reqs_of(b):
    return np.array(b.reqs, dtype=_lib.VMODEL_WRITE_REQ) if len(b.reqs) else np.zeros(0, _lib.VMODEL_WRITE_REQ)


def call(s, b, now=fx.NOW, age=fx.AGE, owner=fx.DEFAULT_OWNER):
    return s.vmodels_write_json(reqs_of(b), b.strs, b.olds, now, age, owner)


def raw(s, b, cap, now=fx.NOW, age=fx.AGE, owner=fx.DEFAULT_OWNER, reqs=None, **kw):
    return s.vmodels_write_json_raw(reqs_of(b) if reqs is None else reqs, b.strs, b.olds, now, age, owner, cap, fill=FILL, **kw)


def rows_of(model_rows):
    out = np.zeros(len(model_rows), _lib.VMODEL_WRITE_ROW)
    for i, r in enumerate(model_rows):
        out[i] = (r.cls, r.flags, r.model, r.target_copy_count, r.dec_model, r.dec_off, r.dec_len, r.last_used)
    return out


def check(s, b, reg, **kw):
    """The call equals the model on batch b: rows and bytes (the offsets are the values' lengths).  -> (values, rows)."""
    want, want_rows = wm.write_batch(b.reqs, b.strs, b.olds, reg, kw.get("now", fx.NOW), kw.get("age", fx.AGE),
                                     kw.get("owner", fx.DEFAULT_OWNER))
    vals, rows = call(s, b, **kw)
    exp = rows_of(want_rows)
    bad = [i for i in range(len(rows)) if rows[i].tobytes() != exp[i].tobytes()]
    assert not bad, [(i, rows[i], exp[i], b.reqs[i], b.strs[i], b.olds[i][:200]) for i in bad[:4]]
    for i, (g, x) in enumerate(zip(vals, want)):
        assert g == x, (i, b.reqs[i], len(b.olds[i]), g, x)
    return vals, rows


@pytest.fixture(scope="module")
def ctx():
    s = start()
    reg = registry_of(s)
    assert reg.ids == fx.MIDS and reg.recs == [tuple(r) for r in fx.RECS]  # the device holds what the CPU tests assumed
    yield s, reg
    s.close()


@pytest.mark.parametrize("n", fx.SIZES)
def test_batch_sizes_against_the_model(ctx, n):
    s, reg = ctx
    b = fx.sized_batch(n)
    assert len(b.reqs) == n
    check(s, b, reg)


def test_n_1_once_per_class_and_op(ctx):
    s, reg = ctx
    singles = fx.single_batches()
    assert {b.reqs[0][0] for b in singles} == set(wm.OPS)
    for b, want in zip(singles, wm.CLASSES):
        assert list(check(s, b, reg)[1]["cls"]) == [want]


def test_tile_edges_at_every_dword_alignment(ctx):
    """2 046 .. 2 048 bytes take the tile, 2 049 and 2 050 the serial walk: both equal the model, so they agree."""
    s, reg = ctx
    check(s, fx.tile_edge_batch(), reg)


def test_values_of_63_to_130_members(ctx):
    s, reg = ctx
    check(s, fx.member_batch(), reg)
    check(s, fx.member_batch(True), reg)


def test_ids_across_the_lanes(ctx):
    s, reg = ctx
    check(s, fx.string_batch(), reg)


def test_request_strings_that_need_every_escape(ctx):
    s, reg = ctx
    vals, _ = check(s, fx.escape_batch(), reg)
    assert any(b'"amid":"q\\" b\\\\ nl\\u000a tab\\u0009 \\u0001\\u001f del\x7f e-acute \xc3\xa9"' in v for v in vals if v)


def test_one_stored_value_64_times(ctx):
    s, reg = ctx
    check(s, fx.repeated_batch(), reg)


def test_the_last_used_arithmetic_wraps(ctx):
    s, reg = ctx
    b = fx.sized_batch(65)
    for now, age in ((5, (1 << 63) - 1), (1, 1 << 62), (fx.NOW, 0), ((1 << 63) - 1, 1)):
        check(s, b, reg, now=now, age=age)


def test_without_a_default_owner(ctx):
    s, reg = ctx
    vals, _ = check(s, fx.sized_batch(63), reg, owner=b"")
    assert vals[0] == b'{"o":"owner-a","amid":"m8","tmid":"m8"}'
    b = fx.Batch([(wm.SET, 0)], [(fx.A, b"", b"")], [b""])
    assert check(s, b, reg, owner=b"")[0] == [b'{"amid":"m8","tmid":"m8"}']
    assert check(s, b, reg)[0] == [b'{"o":"default-owner","amid":"m8","tmid":"m8"}']


def test_malformed_exactly_where_the_parser_says_status_1(ctx):
    """The malformed and edge lists of tests/vmodel_fixtures.py, each as the stored value of the four ops."""
    s, reg = ctx
    values = fx.corpus_values()
    assert sum(vm.classify(v)[0] == REJECT for v in values) > 30 and len(values) > 100
    _, rows = check(s, fx.corpus_batch(), reg)
    t = WORLD.solver()
    try:
        pst = t.vmodels_events_json([b"c%d" % i for i in range(len(values))], values)[0]
    finally:
        t.close()
    got = (rows["cls"][len(fx.head()):].reshape(-1, 4) == wm.MALFORMED)
    assert all(np.array_equal(got[:, k], pst == 1) for k in range(4))


def test_dec_spans_slice_the_ids_and_rows_equal_model_ids_resolve(ctx):
    s, reg = ctx
    n_dec = 0
    for b in fx.every_batch():
        _, rows = check(s, b, reg)
        ids, at = [], []
        for i, r in enumerate(rows):
            for k in range(2):
                if r["dec_len"][k] >= 0:
                    o = int(r["dec_off"][k])
                    span = b.olds[i][o:o + int(r["dec_len"][k])]
                    assert b.olds[i][o - 1:o] == b'"' and b.olds[i][o + len(span):o + len(span) + 1] == b'"'
                    row = vm.classify(b.olds[i])[1]
                    assert span in (row.amid, row.tmid)
                    ids.append(span)
                    at.append((i, k))
        want = s.model_ids_resolve(ids)
        assert [int(rows[i]["dec_model"][k]) for i, k in at] == list(want)
        n_dec += len(ids)
        sets = [i for i, r in enumerate(rows) if r["cls"] in (wm.CREATED, wm.UPDATED, wm.UNCHANGED, wm.NEEDS_TARGET_STATUS) and b.reqs[i][0] == wm.SET]
        assert list(rows["model"][sets]) == list(s.model_ids_resolve([b.strs[i][0] for i in sets]))
    assert n_dec > 300


@pytest.mark.parametrize("bits", [0, 4])
def test_both_id_hashes_masked(monkeypatch, bits):
    monkeypatch.setenv("MMP_MODEL_ID_HASH_BITS", str(bits))
    monkeypatch.setenv("MMP_VMODEL_ID_HASH_BITS", str(bits))
    s = start()
    try:
        reg = registry_of(s)
        check(s, fx.sized_batch(257), reg)
        check(s, fx.string_batch(), reg)
    finally:
        s.close()


def test_rendered_values_through_the_read_side(ctx):
    """Every CREATED and UPDATED value of every batch, as an event of a key of its own: the table then carries the record the
    model intends, read back through mmp_vmodels_get, and mmp_vmodels_resolve answers from it."""
    s, reg = ctx
    t = start()
    try:
        keys, values, want = [], [], []
        for b in fx.every_batch():
            vals, rows = check(s, b, reg)
            for i, v in enumerate(vals):
                if v is not None:
                    keys.append(b"w%d" % len(keys))
                    values.append(v)
                    want.append(vm.classify(v))
        assert len(keys) > 400 and all(c[1] is not None for c in want)
        status, idx, n_app = t.vmodels_events_json(keys, values)
        assert not status.any() and n_app == len(keys)
        m = vm.VModels()
        m.events(keys, values)
        ids, flags, strings = t.vmodels_get()
        assert ids == m.ids and np.array_equal(flags, m.flags()) and strings == m.strings()
        assert strings == [(r.amid, r.tmid, r.owner) for _, r in want]
        ans = t.vmodels_resolve(keys)
        assert [tuple(int(x) for x in a) for a in ans] == [tuple(a) for a in m.resolve_many(registry_of(t), keys)]
    finally:
        t.close()


def test_sizing_a_small_buffer_writes_nothing(ctx):
    s, reg = ctx
    b = fx.sized_batch(65)
    want, want_rows = fx.run_model(b, reg)
    total = sum(len(v) for v in want if v is not None)
    offs = np.concatenate([[0], np.cumsum([len(v) if v is not None else 0 for v in want])])
    for cap, null_out in ((0, True), (0, False), (total - 1, False), (total - 1, True)):
        out, off, rows, tot, rc = raw(s, b, cap, null_out=null_out)
        assert rc == 0 and tot == total and rows.tobytes() == rows_of(want_rows).tobytes() and np.array_equal(off, offs)
        assert (out == FILL).all()
    for cap in (total, total + 3):
        out, off, rows, tot, rc = raw(s, b, cap)
        assert rc == 0 and tot == total and bytes(out[:total]) == b"".join(v for v in want if v is not None)
        assert (out[total:] == FILL).all()


def test_refusals_leave_the_outputs_untouched(ctx):
    s, reg = ctx
    b = fx.sized_batch(63)

    def refused(rc_want, on=s, **kw):
        out, off, rows, tot, rc = raw(on, b, 4096, **kw)
        assert rc == rc_want, (rc, kw)
        assert tot == -1 and all((a.view(np.uint8) == FILL).all() for a in (out, off, rows))

    refused(EINVAL, flags=1)
    refused(EINVAL, now=0)
    refused(EINVAL, now=-5)
    refused(EINVAL, age=-1)
    for field, value in (("op", 4), ("op", 1 << 31), ("flags", 128), ("flags", 1 << 31), ("flags", wm.TARGET_LOADED | wm.TARGET_NOT_LOADED)):
        r = reqs_of(b)
        r[field][40] = value
        refused(EINVAL, reqs=r)
    lens = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])])  # noqa: E731
    off = lens(b.olds).astype(np.int64)
    off[30] = off[31] + 1
    refused(EINVAL, old_off=off)
    soff = lens([x for t in b.strs for x in t]).astype(np.int32)
    soff[3 * 20 + 2] = soff[3 * 20 + 3] + 1
    refused(EINVAL, str_off=soff)
    for i in (0, 9):  # a SET and a COMPLETE with an empty id_a, the offsets still monotone
        assert b.reqs[i][0] in (wm.SET, wm.COMPLETE)
        soff = lens([x for t in b.strs for x in t]).astype(np.int32)
        soff[3 * i + 1:] -= soff[3 * i + 1] - soff[3 * i]
        refused(EINVAL, str_off=soff)
    # NULL required buffers, negative sizes
    L, total = s.lib, C.c_int64(-1)
    req, soff1, off1 = np.zeros(1, _lib.VMODEL_WRITE_REQ), np.array([0, 1, 1, 1], np.int32), np.array([0, 2], np.int64)
    o, rw = np.full(2, -1, np.int64), np.full(1, 0xFF, _lib.VMODEL_WRITE_ROW)
    rw.view(np.uint8)[:] = FILL
    P = _lib.ptr
    full = [s.h, P(req), 1, b"a", P(soff1), None, 0, b"{}", P(off1), fx.NOW, fx.AGE, 0, None, 0, P(o), P(rw), C.byref(total)]
    for hole in (1, 3, 4, 7, 8, 14, 15, 16):
        args = list(full)
        args[hole] = None
        assert L.mmp_vmodels_write_json(*args) == EINVAL, hole
    for at, value in ((6, -1), (6, 3), (13, -1)):  # a negative owner length, an owner length without bytes, a negative capacity
        args = list(full)
        args[at] = value
        assert L.mmp_vmodels_write_json(*args) == EINVAL, at
    assert total.value == -1 and list(o) == [-1, -1] and (rw.view(np.uint8) == FILL).all()
    assert L.mmp_vmodels_write_json(*full) == 0 and total.value == 23 and rw["cls"][0] == wm.UPDATED  # {} takes a target
    # MMP_ESTATE: no model-id table
    fresh = WORLD.solver()
    try:
        refused(ESTATE, on=fresh)
    finally:
        fresh.close()
    assert len(check(s, b, reg)[0]) == 63  # and the context still answers


def test_n_0_is_valid(ctx):
    s, _ = ctx
    out, off, rows, tot, rc = raw(s, fx.to_batch([]), 16)
    assert rc == 0 and tot == 0 and list(off) == [0] and (out == FILL).all()


def test_two_runs_are_byte_identical(ctx):
    s, _ = ctx
    b = fx.sized_batch(257)
    a1, a2 = call(s, b), call(s, b)
    assert a1[0] == a2[0] and a1[1].tobytes() == a2[1].tobytes()


def test_200_calls_beside_a_thread_sending_registry_events(ctx):
    """A writer flips the previous active model's record between one loaded copy and none: every answer equals the model's over one
    state or the other, and both are seen to differ."""
    s, _ = ctx
    t = start()
    try:
        key = fx.A
        row = fx.MIDS.index(key)
        states = (REG_VALUES[row], REG_VALUES[fx.MIDS.index(fx.C)])  # loaded1 / not_loaded
        b = fx.sized_batch(65)
        answers = []
        for v in states:
            assert not t.models_events_json([key], [v], None, False)[0].any()
            vals, rows = fx.run_model(b, registry_of(t))
            answers.append((vals, rows_of(rows).tobytes()))
        assert answers[0] != answers[1]
        stop, errors, sent = threading.Event(), [], []

        def writer():
            try:
                while not stop.is_set() or len(sent) < 2:
                    assert not t.models_events_json([key], [states[len(sent) % 2]], None, False)[0].any()
                    sent.append(1)
            except Exception as ex:  # noqa: BLE001
                errors.append(ex)

        th = threading.Thread(target=writer)
        th.start()
        seen = set()
        try:
            for _ in range(200):
                out, off, rows, tot, rc = raw(t, b, 1 << 16)  # (one call: the sizes and the bytes of one state)
                assert rc == 0 and tot <= 1 << 16
                vals = [bytes(out[off[i]:off[i + 1]]) if rows["cls"][i] in wm.RENDERED else None for i in range(len(rows))]
                got = (vals, rows.tobytes())
                assert got in answers
                seen.add(answers.index(got))
        finally:
            stop.set()
            th.join()
        assert not errors, errors
    finally:
        t.close()


class DeviceAnswers:
    """tests/vmodel_minimesh.py's two calls answered by the device, over a context that follows the mesh's two tables through the
    listeners' events (mmp_models_events_json / mmp_vmodels_events_json) after every commit."""

    def __init__(self, mesh):
        self.mesh = mesh
        self.s = s = WORLD.solver()
        assert not len(s.ingest_models_json([])[0])
        s.model_ids_load([])

    def write(self, op, flags, strs, old):
        vals, rows = self.s.vmodels_write_json(np.array([(op, flags)], _lib.VMODEL_WRITE_REQ), [strs], [old], self.mesh.now, self.mesh.age,
                                               self.mesh.default_owner)
        r = rows[0]
        return vals[0], wm.Row(int(r["cls"]), int(r["flags"]), int(r["model"]), int(r["target_copy_count"]), tuple(map(int, r["dec_model"])),
                               tuple(map(int, r["dec_off"])), tuple(map(int, r["dec_len"])), int(r["last_used"]))

    def refs(self, flags, last_used, info, old):
        vals, cls, refs = self.s.models_refs_json(np.array([(flags, 0, last_used)], _lib.REFS_REQ), [old], None if info is None else [info])
        return vals[0], int(cls[0]), int(refs[0])

    def committed(self, reg, vms):
        if reg:
            keys = list(reg)
            st = self.s.models_events_json(keys, [reg[k] or b"" for k in keys], [reg[k] is None for k in keys], True)[0]
            assert not st.any()
        if vms:
            keys = list(vms)
            assert not self.s.vmodels_events_json(keys, [vms[k] or b"" for k in keys], np.array([vms[k] is None for k in keys], np.uint8))[0].any()


@pytest.mark.parametrize("name", ["vModelsTest", "vModelOwnerTest"])
def test_the_references_own_tests_with_the_device_answering(name):
    """tests/golden/vmodel_kats.json through tests/vmodel_minimesh.py, every assertion of the reference test holding; after every
    step the resident tables are asked — mmp_vmodels_resolve, mmp_vmodels_transitions, mmp_models_status — and say what the mesh's
    own two tables say."""
    kats = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vmodel_kats.json")))
    mesh = minimesh.MiniVMesh(fx.NOW, fx.AGE, b"", DeviceAnswers, WORLD.pod_ids[0])
    s = mesh.answers.s
    asked = []

    def after(m, st):
        vmids = [b"test-vmodel-a", b"test-vmodel-b", b"test-vmodel-owner1"]
        ans = s.vmodels_resolve(vmids)
        ids = s.model_ids_get()
        for k, a in zip(vmids, ans):
            want = m.vmodel_status(k)
            assert (a["cls"] == vm.OK) == (want["status"] != "NOT_FOUND"), (st, k, a)
            if a["cls"] == vm.OK:
                assert ids[a["model"]].decode() == want["active"] and ids[a["target_model"]].decode() == want["target"]
                assert (a["vstatus"] == vm.DEFINED) == (want["status"] == "DEFINED")
        rows, info = s.vmodels_transitions(fx.NOW, fx.AGE)
        moving = sorted(k for k in m.vmodels if m.vmodel_status(k)["status"] == "TRANSITIONING")
        assert info["n_listed"] == len(moving) and info["n_host_skipped"] == 0
        models = [b"myModel", b"myNextModel3", b"myNextModel4", b"another-model"]
        rows_of_ids = s.model_ids_resolve(models)
        known = [(k, r) for k, r in zip(models, rows_of_ids) if r >= 0]
        if known:
            reqs = np.zeros(len(known), _lib.STATUS_REQ)
            reqs["model"], reqs["fail_pod"] = [r for _, r in known], -1
            status = s.models_status(reqs, fx.NOW)[0]
            reg = registry_of(s)
            for (k, r), row in zip(known, status):  # (a deleted record leaves the empty row: the id keeps its number)
                assert (not reg.empty(int(r))) == m.model_found(k), (st, k, row)
                assert (row["cls"] == _lib.MST_ASK) == m.is_loaded(k) and row["cls"] != _lib.MST_NOT_FOUND, (st, k, row)
        assert all(not m.model_found(k) for k, r in zip(models, rows_of_ids) if r < 0)
        asked.append(st["at"])

    try:
        minimesh.run_scenario(mesh, kats[name]["steps"], after)
    finally:
        s.close()
    assert len(asked) == len(kats[name]["steps"])
