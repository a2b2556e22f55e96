"""mmp_models_refs_json on the device against tests/model_refs_model.py, byte for byte on values, offsets, classes and counts:
batches of 0, 1, 63, 64, 65 and 257 requests, stored values on both sides of the 2 048-byte tile at every dword alignment (padded
by an unknown member and by a long kept string), every refs value against every autoDel value, values of 63 .. 130 members, one
value 64 times in a call, the parser's own verdict on the malformed and edge lists of tests/ingest_corpus.py, created records whose
strings need every escape, every rendered value fed back through mmp_models_events_json, the sizing protocol, every refusal with
the outputs untouched, two runs, 200 calls beside a thread that sends registry events.  The batches are
tests/model_refs_fixtures.py's; tests/test_model_refs_model.py asserts, without a device, that each holds all seven classes."""
import ctypes as C
import threading

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd.solver import Solver
from tests import model_refs_fixtures as fx
from tests import model_refs_model as mr
from tests import registry_prune_model as rp
from tests.ingest_model import REJECT, model_bean, model_class
from tests.model_events_fixtures import World, make_model_ids

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -5
FILL = 0xA5
N_BASE = 40


def reqs_of(b):
    r = np.zeros(len(b.reqs), _lib.REFS_REQ)
    for i, (f, t) in enumerate(b.reqs):
        r[i] = (f, 0, t)
    return r


def call(s, b, infos=True):
    return s.models_refs_json(reqs_of(b), b.olds, b.infos if infos else None)


def raw(s, b, cap, reqs=None, infos=True, **kw):
    return s.models_refs_json_raw(reqs_of(b) if reqs is None else reqs, b.olds, b.infos if infos else None, cap, fill=FILL, **kw)


def check(s, b):
    """The call equals the model on batch b: classes, counts, bytes (the offsets are the values' lengths).  -> (values, classes)."""
    want, want_cls, want_refs = fx.run_model(b)
    vals, cls, refs = call(s, b)
    bad = np.nonzero(np.array(cls) != np.array(want_cls, np.int32))[0]
    assert not len(bad), [(int(i), int(cls[i]), want_cls[i], b.reqs[i], b.infos[i], b.olds[i][:200]) for i in bad[:4]]
    assert list(refs) == want_refs
    for i, (g, x) in enumerate(zip(vals, want)):
        assert g == x, (i, b.reqs[i], len(b.olds[i]), g, x)
    return vals, cls


@pytest.fixture(scope="module")
def ctx():
    """(world, s, ids): a committed 8-instance context whose registry holds the world's 300 stored values, N_BASE of them named."""
    w = World(0)
    s = w.solver()
    assert not s.ingest_models_json(w.values)[0].any()
    ids = make_model_ids(np.random.default_rng(5), len(w.values))
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
    for b, want in zip(fx.single_batches(), mr.CLASSES):
        assert list(check(s, b)[1]) == [want]


def test_the_fleets_own_stored_values(ctx):
    """The 300 stored values of the fleet, read as the store holds them: each takes a referent, and gives it back."""
    w, s, _ = ctx
    olds = [v if isinstance(v, bytes) else v.encode() for v in w.values]
    up = fx.Batch([(mr.INC, fx.NOW + i) for i in range(len(olds))], [fx.NO_INFO] * len(olds), olds)
    vals, cls = check(s, up)
    assert set(cls) == {mr.SET}
    down = fx.Batch([(0, 0)] * len(olds), [fx.NO_INFO] * len(olds), vals)
    assert set(check(s, down)[1]) == {mr.SET}


def test_refs_and_auto_del_at_their_value_edges(ctx):
    _, s, _ = ctx
    check(s, fx.boundary_batch())


def test_tile_edges_at_every_dword_alignment(ctx):
    """2 046 .. 2 048 bytes take the tile, 2 049 and 2 050 the serial walk: both equal the model, so they agree."""
    _, s, _ = ctx
    check(s, fx.tile_edge_batch())


def test_values_of_63_to_130_members(ctx):
    _, s, _ = ctx
    check(s, fx.member_batch())


def test_the_member_layouts_padded_past_the_tile(ctx):
    _, s, _ = ctx
    check(s, fx.padded_member_batch())


def test_one_stored_value_64_times(ctx):
    _, s, _ = ctx
    vals, _ = check(s, fx.repeated_batch())
    assert len(set(vals[7::2])) == 32 and len(set(vals[8::2])) == 1  # (an INC renders its own last_used, a DEC the same bytes)


def test_created_records_and_strings_that_need_every_escape(ctx):
    _, s, _ = ctx
    b = fx.created_batch()
    vals, _ = check(s, b)
    assert any(b'"encKey":"q\\" b\\\\ nl\\u000a tab\\u0009 \\u0001\\u001f del\x7f e-acute \xc3\xa9"' in v for v in vals if v)


def test_without_info_every_creation_is_not_found(ctx):
    _, s, _ = ctx
    b = fx.created_batch()
    want, want_cls, want_refs = mr.refs_batch(b.reqs, None, b.olds)
    vals, cls, refs = call(s, b, infos=False)
    assert vals == want and list(cls) == want_cls and list(refs) == want_refs and mr.CREATED not in want_cls


def test_malformed_exactly_where_the_parser_says_status_1(ctx):
    """The malformed and edge lists of tests/ingest_corpus.py, each as the stored value of an INC and of a DEC."""
    _, s, _ = ctx
    values = fx.corpus_values()
    assert sum(model_class(v) == REJECT for v in values) > 100 and len(values) > 1000
    _, cls = check(s, fx.corpus_batch(values))
    t = Solver(1, 1)
    try:
        t.load_pod_ids(["i-0"])
        pst, _ = t.upsert_models_json(values, np.arange(len(values), dtype=np.int32))
    finally:
        t.close()
    got = np.array(cls[7:]).reshape(-1, 2) == mr.MALFORMED
    assert np.array_equal(got[:, 0], pst == 1) and np.array_equal(got[:, 1], pst == 1)
    assert [int(x) for x in got[:, 0]] == [int(model_class(v) == REJECT) for v in values]


def test_rendered_values_through_the_read_side(ctx):
    """Every SET and CREATED value of every batch, as an event of a key of its own with MMP_MEV_APPEND: the records then carry
    the intended type and lu and the old value's entries."""
    w, s, _ = ctx
    t = w.solver()
    try:
        assert not len(t.ingest_models_json([])[0])
        t.model_ids_load([])
        first = 0
        for b in fx.every_batch():
            vals, cls = check(s, b)
            idx = [i for i in range(len(vals)) if vals[i] is not None]
            assert idx and {int(cls[i]) for i in idx} == {mr.SET, mr.CREATED}
            status, rows, _, n_app = t.models_events_json([b"ref-%d-%d" % (first, i) for i in idx], [vals[i] for i in idx], None, True)
            assert not status.any() and n_app == len(idx) and list(rows) == list(range(first, first + len(idx)))
            recs = rp.registry_from_arrays(*t.get_models())
            for r, i in zip(rows, idx):
                flags, lu = b.reqs[i]
                rec = recs[int(r)]
                if cls[i] == mr.CREATED:
                    typ = b.infos[i][0].decode()
                    want = (w.type_names.index(typ) if typ in w.type_names else 0, lu, [], [])
                else:
                    old = model_bean(b.olds[i], w.pod_ids, w.type_names, 0)
                    want = (old.type, lu if flags & mr.INC else old.lu, old.loaded, old.failed)
                assert (rec.type, rec.last_used, list(rec.loaded), list(rec.failed)) == want, (i, vals[i])
            first += len(idx)
    finally:
        t.close()


def test_sizing_a_small_buffer_writes_nothing(ctx):
    _, s, _ = ctx
    b = fx.sized_batch(65)
    want, want_cls, want_refs = fx.run_model(b)
    total = sum(len(v) for v in want if v is not None)
    offs = np.concatenate([[0], np.cumsum([len(v) if v is not None else 0 for v in want])])
    for cap, null_out in ((0, True), (0, False), (total - 1, False), (total - 1, True)):
        out, off, cls, refs, tot, rc = raw(s, b, cap, null_out=null_out)
        assert rc == 0 and tot == total and list(cls) == want_cls and list(refs) == want_refs and np.array_equal(off, offs)
        assert (out == FILL).all()
    for cap in (total, total + 3):  # an exact fit, and room to spare
        out, off, cls, refs, tot, rc = raw(s, b, cap)
        assert rc == 0 and tot == total and bytes(out[:total]) == b"".join(v for v in want if v is not None)
        assert (out[total:] == FILL).all()


def test_refusals_leave_the_outputs_untouched(ctx):
    _, s, _ = ctx
    b = fx.sized_batch(63)

    def refused(rc_want, on=s, **kw):
        out, off, cls, refs, tot, rc = raw(on, b, 4096, **kw)
        assert rc == rc_want, (rc, kw)
        assert tot == -1 and all((a.view(np.uint8) == FILL).all() for a in (out, off, cls, refs))

    refused(EINVAL, flags=1)
    for field, value in (("flags", 4), ("flags", 1 << 31), ("reserved", 1), ("reserved", -1)):
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
    # NULL required buffers, a negative capacity
    L, total = s.lib, C.c_int64(-1)
    req, off1 = np.zeros(1, _lib.REFS_REQ), np.array([0, 2], np.int64)
    o, cl, rf = np.full(2, -1, np.int64), np.full(1, -1, np.int32), np.full(1, -1, np.int32)
    P = _lib.ptr
    full = [s.h, P(req), 1, None, None, b"{}", P(off1), 0, None, 0, P(o), P(cl), P(rf), C.byref(total)]
    for hole in (1, 5, 6, 10, 11, 12, 13):
        args = list(full)
        args[hole] = None
        assert L.mmp_models_refs_json(*args) == EINVAL, hole
    args = list(full)
    args[9] = -1
    assert L.mmp_models_refs_json(*args) == EINVAL
    args = list(full)
    args[4] = P(np.array([0, 1, 1, 1], np.int32))  # info bytes asked for, and no info
    assert L.mmp_models_refs_json(*args) == EINVAL
    assert total.value == -1 and list(o) == [-1, -1] and list(cl) == [-1] and list(rf) == [-1]
    assert L.mmp_models_refs_json(*full) == 0 and total.value == 2 and list(cl) == [mr.SET] and list(o) == [0, 2]  # a DEC of {}
    # MMP_ESTATE: no instance ids (the parser's condition)
    fresh = Solver(1, 1)
    try:
        refused(ESTATE, on=fresh)
        fresh.load_pod_ids(["i-0"])
        out, off, cls, refs, tot, rc = raw(fresh, b, 1 << 20)  # ... and no id table is needed
        assert rc == 0 and list(cls) == fx.run_model(b)[1]
    finally:
        fresh.close()
    assert len(check(s, b)[0]) == 63  # and the context still answers


def test_n_0_is_valid(ctx):
    _, s, _ = ctx
    b = fx.to_batch([])
    for infos in (True, False):
        out, off, cls, refs, tot, rc = raw(s, b, 16, infos=infos)
        assert rc == 0 and tot == 0 and list(off) == [0] and (out == FILL).all()


def test_two_runs_are_byte_identical(ctx):
    _, s, _ = ctx
    b = fx.sized_batch(257)
    a1, a2 = call(s, b), call(s, b)
    assert a1[0] == a2[0] and all(np.array_equal(x, y) for x, y in zip(a1[1:], a2[1:]))


def test_200_calls_beside_a_thread_sending_registry_events(ctx):
    """The answer is a function of the arguments alone: beside a writer that flips a record between two values, every answer
    equals the model's — which is the answer in one state and in the other."""
    w, s, ids = ctx
    b = fx.sized_batch(65)
    want = fx.run_model(b)
    key, states = ids[3], (w.values[3], w.values[4])
    stop, errors, sent = threading.Event(), [], []

    def writer():
        try:
            while not stop.is_set() or len(sent) < 2:
                status, rows, _, n_app = s.models_events_json([key], [states[len(sent) % 2]], None, False)
                assert not status.any() and n_app == 0 and list(rows) == [3]
                sent.append(1)
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    th = threading.Thread(target=writer)
    th.start()
    try:
        for _ in range(200):
            vals, cls, refs = call(s, b)
            assert vals == want[0] and list(cls) == want[1] and list(refs) == want[2]
    finally:
        stop.set()
        th.join()
    assert not errors, errors
    assert not s.models_events_json([key], [states[0]], None, False)[0].any()  # the registry as the other tests found it
