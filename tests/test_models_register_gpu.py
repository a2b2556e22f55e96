"""mmp_models_register_json on the device against tests/model_register_model.py, byte for byte on values, offsets, classes and
last_used: batches of 0, 1, 63, 64, 65 and 257 requests, stored values on both sides of the 2 048-byte tile at every dword
alignment, compared strings of 0 .. 200 bytes that differ in their first, last and 64th byte, values of 63 .. 130 members, the
parser's own verdict on the malformed and edge lists of tests/ingest_corpus.py, request strings that need every escape, every
rendered value fed back through mmp_models_events_json, the rows against mmp_model_ids_resolve (also with colliding hashes), the
sizing protocol, every refusal with the outputs untouched, two runs, a run beside a census reader.  The batches are
tests/model_register_fixtures.py's; tests/test_model_register_model.py asserts, without a device, that each holds all nine classes."""
import ctypes as C
import threading

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd.solver import Solver
from tests import model_register_fixtures as fx
from tests import model_register_model as mm
from tests import registry_prune_model as rp
from tests.ingest_model import REJECT, model_bean, model_class
from tests.model_events_fixtures import World, make_model_ids

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -5
FILL = 0xA5
N_BASE = 40


def reqs_of(b):
    r = np.zeros(len(b.reqs), _lib.REGISTER_REQ)
    for i, (f, t) in enumerate(b.reqs):
        r[i] = (f, 0, t)
    return r


def call(s, b, keys=False):
    return s.models_register_json(reqs_of(b), b.infos, b.olds, fx.NOW, fx.AGE, b.keys if keys else None)


def raw(s, b, cap, keys=False, now=fx.NOW, age=fx.AGE, reqs=None, **kw):
    return s.models_register_json_raw(reqs_of(b) if reqs is None else reqs, b.infos, b.olds, now, age, b.keys if keys else None, cap,
                                      fill=FILL, **kw)


def check(s, b):
    """The call equals the model on batch b: classes, last_used, bytes (the offsets are the values' lengths).  -> (values, classes)."""
    want, want_cls, want_lu = fx.run_model(b)
    vals, cls, lu, rows = call(s, b)
    assert rows is None
    bad = np.nonzero(np.array(cls) != np.array(want_cls, np.int32))[0]
    assert not len(bad), [(int(i), int(cls[i]), want_cls[i], b.reqs[i], b.infos[i], b.olds[i][:200]) for i in bad[:4]]
    assert list(lu) == want_lu
    for i, (g, x) in enumerate(zip(vals, want)):
        assert g == x, (i, b.reqs[i], len(b.olds[i]), g, x)
    return vals, cls


@pytest.fixture(scope="module")
def ctx():
    """(world, s, ids): a committed 8-instance context whose registry holds N_BASE stored values named ids."""
    w = World(0)
    s = w.solver()
    ids = make_model_ids(np.random.default_rng(5), N_BASE)
    assert not s.ingest_models_json(w.values[:N_BASE])[0].any()
    s.model_ids_load(ids)
    yield w, s, ids
    s.close()


@pytest.mark.parametrize("n", fx.SIZES)
def test_batch_sizes_against_the_model(ctx, n):
    _, s, _ = ctx
    b = fx.sized_batch(n)
    assert len(b.reqs) == n
    check(s, b)


def test_n_1_once_per_class(ctx):
    _, s, _ = ctx
    for b, want in zip(fx.single_batches(), mm.CLASSES):
        assert list(check(s, b)[1]) == [want]


def test_tile_edges_at_every_dword_alignment(ctx):
    """2 046 .. 2 048 bytes take the tile, 2 049 and 2 050 the serial walk: both equal the model, so they agree."""
    _, s, _ = ctx
    check(s, fx.tile_edge_batch())


def test_compared_strings_across_the_lanes(ctx):
    _, s, _ = ctx
    check(s, fx.string_batch())


def test_values_of_63_to_130_members(ctx):
    _, s, _ = ctx
    check(s, fx.member_batch())


def test_the_member_layouts_padded_past_the_tile(ctx):
    """The serial walk over 63 .. 130 members with a repeated compared name, each value as a touch and as a delete."""
    _, s, _ = ctx
    check(s, fx.padded_member_batch())


def test_request_strings_that_need_every_escape(ctx):
    _, s, _ = ctx
    vals, _ = check(s, fx.escape_batch())
    assert b'"encKey":"q\\" b\\\\ nl\\u000a tab\\u0009 \\u0001\\u001f del\x7f e-acute \xc3\xa9"' in vals[9]


def test_malformed_exactly_where_the_parser_says_status_1(ctx):
    """The malformed and edge lists of tests/ingest_corpus.py, each as the stored value of a register and of a delete."""
    _, s, _ = ctx
    values = fx.corpus_values()
    assert sum(model_class(v) == REJECT for v in values) > 100 and len(values) > 1000
    b = fx.corpus_batch(values)
    _, cls = check(s, b)
    t = Solver(1, 1)
    try:
        t.load_pod_ids(["i-0"])
        pst, _ = t.upsert_models_json(values, np.arange(len(values), dtype=np.int32))
    finally:
        t.close()
    got = np.array(cls[9:]).reshape(-1, 2) == mm.MALFORMED
    assert np.array_equal(got[:, 0], pst == 1) and np.array_equal(got[:, 1], pst == 1)
    assert [int(x) for x in got[:, 0]] == [int(model_class(v) == REJECT) for v in values]


def test_rendered_values_through_the_read_side(ctx):
    """Every CREATED and TOUCHED value of every batch, as an event of a key of its own with MMP_MEV_APPEND: the records then carry
    the request's type, the intended lu and the old value's entries."""
    w, s, _ = ctx
    t = w.solver()
    try:
        assert not len(t.ingest_models_json([])[0])
        t.model_ids_load([])
        first = 0
        for b in fx.every_batch():
            vals, cls = check(s, b)
            _, _, want_lu = fx.run_model(b)
            idx = [i for i in range(len(vals)) if vals[i] is not None]
            assert idx and {int(cls[i]) for i in idx} == {mm.CREATED, mm.TOUCHED}
            status, rows, _, n_app = t.models_events_json([b"reg-%d-%d" % (first, i) for i in idx], [vals[i] for i in idx], None, True)
            assert not status.any() and n_app == len(idx) and list(rows) == list(range(first, first + len(idx)))
            recs = rp.registry_from_arrays(*t.get_models())
            for r, i in zip(rows, idx):
                typ = b.infos[i][0].decode()
                ts = want_lu[i]
                old = model_bean(b.olds[i], w.pod_ids, w.type_names, 0) if cls[i] == mm.TOUCHED else None
                lu = ts if old is None else max(old.lu, ts if ts else fx.NOW)
                rec = recs[int(r)]
                assert rec.type == (w.type_names.index(typ) if typ in w.type_names else 0) and rec.last_used == lu, (i, vals[i])
                assert (list(rec.loaded), list(rec.failed)) == (([], []) if old is None else (old.loaded, old.failed))
            first += len(idx)
    finally:
        t.close()


@pytest.mark.parametrize("bits", [None, 0, 4])
def test_rows_against_model_ids_resolve(monkeypatch, bits):
    if bits is not None:
        monkeypatch.setenv("MMP_MODEL_ID_HASH_BITS", str(bits))
    w = World(0)
    s = w.solver()
    try:
        ids = make_model_ids(np.random.default_rng(5), N_BASE)
        assert not s.ingest_models_json(w.values[:N_BASE])[0].any()
        s.model_ids_load(ids)
        b = fx.sized_batch(65)
        keys = [ids[(3 * i) % N_BASE] if i % 4 else b"unknown-%d" % i for i in range(65)]
        b = b._replace(keys=keys)
        want = s.model_ids_resolve(keys)
        assert (want < 0).sum() == 17 and len(set(want)) > 20
        vals, cls, lu, rows = call(s, b, keys=True)
        assert np.array_equal(rows, want)
        plain = call(s, b)
        assert vals == plain[0] and np.array_equal(cls, plain[1]) and np.array_equal(lu, plain[2])
    finally:
        s.close()


def test_sizing_a_small_buffer_writes_nothing(ctx):
    _, s, _ = ctx
    b = fx.sized_batch(65)
    want, want_cls, want_lu = fx.run_model(b)
    total = sum(len(v) for v in want if v is not None)
    offs = np.concatenate([[0], np.cumsum([len(v) if v is not None else 0 for v in want])])
    for cap, null_out in ((0, True), (0, False), (total - 1, False), (total - 1, True)):
        out, off, cls, lu, rows, tot, rc = raw(s, b, cap, null_out=null_out)
        assert rc == 0 and tot == total and list(cls) == want_cls and list(lu) == want_lu and np.array_equal(off, offs)
        assert (out == FILL).all()
    out, off, cls, lu, rows, tot, rc = raw(s, b, total + 3)
    assert rc == 0 and tot == total and bytes(out[:total]) == b"".join(v for v in want if v is not None)
    assert (out[total:] == FILL).all()


def test_refusals_leave_the_outputs_untouched(ctx):
    _, s, _ = ctx
    b = fx.sized_batch(63)
    n = 63

    def refused(rc_want, on=s, keys=False, **kw):
        out, off, cls, lu, rows, tot, rc = raw(on, b, 4096, keys=keys, **kw)
        assert rc == rc_want, (rc, kw)
        assert tot == -1 and all((a.view(np.uint8) == FILL).all() for a in (out, off, cls, lu))
        assert rows is None or (rows.view(np.uint8) == FILL).all()

    refused(EINVAL, flags=1)
    refused(EINVAL, now=0)
    refused(EINVAL, now=-5)
    refused(EINVAL, age=-1)
    for field, value in (("flags", 4), ("flags", 1 << 31), ("reserved", 1)):
        r = reqs_of(b)
        r[field][40] = value
        refused(EINVAL, reqs=r)
    lens = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])])  # noqa: E731
    off = lens(b.olds).astype(np.int64)
    off[30] = off[31] + 1
    refused(EINVAL, old_off=off)
    ioff = lens([x for t in b.infos for x in t]).astype(np.int32)
    ioff[3 * 20 + 2] = ioff[3 * 20 + 3] + 1
    refused(EINVAL, info_off=ioff)
    koff = lens(b.keys).astype(np.int32)
    koff[6] = koff[7] + 1
    refused(EINVAL, keys=True, key_off=koff)
    ioff = lens([x for t in b.infos for x in t]).astype(np.int32)
    ioff[3 * 1 + 1:] -= ioff[3 * 1 + 1] - ioff[3 * 1]  # request 1 (a register) with an empty type, the offsets still monotone
    refused(EINVAL, info_off=ioff)
    # NULL required buffers
    L, total = s.lib, C.c_int64(-1)
    req, ioff1, off1 = np.zeros(1, _lib.REGISTER_REQ), np.array([0, 1, 1, 1], np.int32), np.array([0, 2], np.int64)
    o, cl, lu = np.full(2, -1, np.int64), np.full(1, -1, np.int32), np.full(1, -1, np.int64)
    P = _lib.ptr
    full = [s.h, P(req), 1, None, None, b"t", P(ioff1), b"{}", P(off1), fx.NOW, fx.AGE, 0, None, 0, P(o), P(cl), P(lu), None, C.byref(total)]
    for hole in (1, 5, 6, 7, 8, 14, 15, 16, 18):
        args = list(full)
        args[hole] = None
        assert L.mmp_models_register_json(*args) == EINVAL, hole
    args = list(full)
    args[17] = P(np.zeros(1, np.int32))  # model_idx_out without key_off
    assert L.mmp_models_register_json(*args) == EINVAL
    assert total.value == -1 and list(o) == [-1, -1] and list(cl) == [-1] and list(lu) == [-1]
    assert L.mmp_models_register_json(*full) == 0 and total.value == 0 and list(cl) == [mm.CONFLICT]  # {} reads as the default type
    # MMP_ESTATE: no instance ids (the parser's condition); rows asked of a context without a model-id table
    fresh = Solver(1, 1)
    try:
        refused(ESTATE, on=fresh)
        fresh.load_pod_ids(["i-0"])
        refused(ESTATE, on=fresh, keys=True)
        out, off, cls, lu, rows, tot, rc = raw(fresh, b, 1 << 20)  # ... and without keys no id table is needed
        assert rc == 0 and list(cls) == fx.run_model(b)[1]
    finally:
        fresh.close()
    assert n == len(check(s, b)[0])  # and the context still answers


def test_n_0_is_valid(ctx):
    _, s, _ = ctx
    b = fx.to_batch([])
    out, off, cls, lu, rows, tot, rc = raw(s, b, 16, keys=True)
    assert rc == 0 and tot == 0 and list(off) == [0] and (out == FILL).all()


def test_two_runs_are_byte_identical(ctx):
    _, s, _ = ctx
    b = fx.sized_batch(257)
    a1, a2 = call(s, b, keys=True), call(s, b, keys=True)
    assert a1[0] == a2[0] and all(np.array_equal(x, y) for x, y in zip(a1[1:], a2[1:]))


def test_beside_a_census_reader(ctx):
    _, s, _ = ctx
    b = fx.sized_batch(257)
    want = call(s, b)
    census0 = s.registry_census()
    stop, errors, reads = threading.Event(), [], []

    def reader():
        try:
            while not stop.is_set() or len(reads) < 2:
                reads.append(s.registry_census())
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    th = threading.Thread(target=reader)
    th.start()
    try:
        for _ in range(6):
            got = call(s, b)
            assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    finally:
        stop.set()
        th.join()
    assert not errors, errors
    for c in reads:
        for x, y in zip(c, census0):
            assert np.array_equal(x, y)
