"""mmp_models_rewrite_json on the device against tests/model_rewrite_model.py, byte for byte: batches of 0, 1, 63, 64, 65, 256 and
257 values over an 8 x 300 fleet loaded by key, rows of 0 .. 130 entries, old values on both sides of the 2 048-byte tile at every
dword alignment, one row 64 times in a call, the rendered values fed back through mmp_models_upsert_json into a twin context,
the parser's own verdict on the malformed and edge lists of tests/ingest_corpus.py, the registry after applied ops, a prune, a
join and a retire, the sizing protocol, every refusal with the outputs untouched, two runs, a run beside a census reader.
The batches are tests/model_rewrite_fixtures.py's; tests/test_model_rewrite_model.py asserts, without a device, that each holds
every status and every owned member present and omitted."""
import ctypes as C
import threading

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd.solver import Solver
from tests import ingest_corpus as ic
from tests import model_rewrite_fixtures as fx
from tests import registry_prune_model as rp
from tests.ingest_model import REJECT, UNSPECIFIED, model_class
from tests.model_events_fixtures import same_registry, start, to_arrays

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -5
FILL = 0xA5


def recs_of(s):
    return [(r.type, r.last_used, tuple(r.loaded), tuple(r.failed)) for r in rp.registry_from_arrays(*s.get_models())]


def start_rewrite(w):
    """(s, t, recs): s holds the world's registry with the setup events applied, by key; t is a twin with 300 empty rows."""
    s, twin, _ = start(w, w.base_ids)
    t = twin.s
    status = s.models_events_json([w.base_ids[r] for r, _, _ in w.setup], [v for _, v, _ in w.setup],
                                  np.array([g for _, _, g in w.setup], np.uint8), False)[0]
    assert not status.any()
    recs = fx.recs_after_setup(w)
    same_registry(rp.compact(*s.get_models()), to_arrays(recs), "setup")
    assert not t.ingest_models_json(["{}"] * len(w.stored))[0].any()
    return s, t, recs


def rewrite(s, b, lul=True):
    return s.models_rewrite_json(b.rows, b.olds, b.last_unload if lul else None, (b.fail_pod, b.msgs))


def check(s, b, recs, pod_ids, lul=True):
    """The call equals the model on batch b: statuses and bytes.  Returns (values, status)."""
    want, want_st = fx.run_model(b, recs, pod_ids, lul)
    vals, st = rewrite(s, b, lul)
    assert list(st) == want_st, np.nonzero(np.array(st) != np.array(want_st))[0][:8]
    for i, (g, x) in enumerate(zip(vals, want)):
        assert g == x, (i, int(b.rows[i]), len(b.olds[i]), g, x)
    return vals, st


@pytest.fixture(scope="module")
def ctx():
    w = fx.rewrite_world(0)
    s, t, recs = start_rewrite(w)
    yield w, s, t, recs
    s.close()
    t.close()


@pytest.mark.parametrize("n", fx.SIZES)
def test_batch_sizes_against_the_model_and_the_twin(ctx, n):
    w, s, t, recs = ctx
    b = fx.sized_batch(w, recs, n)
    assert len(b.olds) == n
    vals, st = check(s, b, recs, w.pod_ids)
    check(s, b, recs, w.pod_ids, lul=False)  # lul as an ordinary kept member
    # the rendered values are what the read side takes: through mmp_models_upsert_json into the twin, record by record
    ok = [i for i in range(n) if st[i] == 0]
    if ok:
        tst, tlul = t.upsert_models_json([vals[i] for i in ok], b.rows[ok])
        assert not tst.any() and np.array_equal(tlul, b.last_unload[ok])
        trecs = recs_of(t)
        same_registry(to_arrays([trecs[int(b.rows[i])] for i in ok]), to_arrays([recs[int(b.rows[i])] for i in ok]), "twin")


def test_n_1_once_per_status(ctx):
    w, s, _, recs = ctx
    for b, want in zip(fx.single_batches(w), (0, 1, 2)):
        assert list(check(s, b, recs, w.pod_ids)[1]) == [want]


def test_tile_edges_at_every_dword_alignment(ctx):
    """2 046 .. 2 048 bytes take the tile, 2 049 and 2 050 the serial walk: both equal the model, so they agree."""
    w, s, _, recs = ctx
    for b in fx.tile_edge_batches(w):
        check(s, b, recs, w.pod_ids)


def test_one_row_64_times_under_different_fail_pods(ctx):
    w, s, _, recs = ctx
    vals, st = check(s, fx.same_row_batch(w), recs, w.pod_ids)
    assert len(set(vals[8:])) > 8 and not any(st[8:])
    same_registry(rp.compact(*s.get_models()), to_arrays(recs), "read-only")


def test_fails_members_around_the_64_member_round_on_both_routes(ctx):
    """`fails` at member 0, 63, 64 and last of 63 .. 130 members, two `fails` inside and across a round, objects and not: on the
    tile, and padded past it."""
    w, s, _, recs = ctx
    for b in fx.member_batches(w):
        check(s, b, recs, w.pod_ids)


def test_rows_of_0_to_130_entries():
    ids, stored, recs = fx.entry_world()
    s = Solver(1, 1)
    try:
        s.load_pod_ids(ids)
        assert not s.ingest_models_json(stored)[0].any()
        same_registry(rp.compact(*s.get_models()), to_arrays(recs), "entry world")
        b = fx.entry_batch(ids, stored, recs)
        assert max(len(v) for v in b.olds) > fx.TILE  # both routes
        check(s, b, recs, ids)
        check(s, b, recs, ids, lul=False)
    finally:
        s.close()


def test_status_1_exactly_where_the_parser_gives_it(ctx):
    """The malformed and edge lists of tests/ingest_corpus.py: status 1 here exactly where mmp_models_upsert_json gives it — and
    every other value, escaped strings across the chunk edges included, rewritten as the model rewrites it."""
    w, s, t, recs = ctx
    values = list(ic.model_corpus()) + ic.chunk_edge_models() + ic.tile_edge_models()[0]
    values = [v if isinstance(v, bytes) else v.encode() for v in values]
    values = [v for v in values if model_class(v) != UNSPECIFIED]
    assert sum(model_class(v) == REJECT for v in values) > 100 and len(values) > 1000
    b = fx.to_batch([(6, v, 3, -1, b"") for v in values])
    _, st = check(s, b, recs, w.pod_ids)
    pst, _ = t.upsert_models_json(values, b.rows)
    assert np.array_equal(st == 1, pst == 1)
    assert [int(x == 1) for x in st] == [int(model_class(v) == REJECT) for v in values]


def test_after_applied_registry_ops(ctx):
    w, _, _, _ = ctx
    s, t, recs = start_rewrite(w)
    try:
        now = int(w.fleet.now)
        with_copy = [r for r in range(10, len(recs)) if recs[r][2]]  # rows with a loaded copy
        ra = next(r for r in range(10, len(recs)) if len(recs[r][2]) + len(recs[r][3]) < 8 and r not in with_copy[:3])
        rb, rc, rd = with_copy[:3]
        free = next(p for p in range(8) if p not in {q for q, _ in recs[ra][2] + recs[ra][3]})
        ops = np.zeros(4, _lib.REGISTRY_OP)
        ops["model"] = (ra, rb, rc, rd)
        ops["pod"] = (free, recs[rb][2][0][0], recs[rc][2][0][0], recs[rd][2][0][0])
        ops["op"] = (_lib.ROP_REGISTER, _lib.ROP_LOAD_FAILED, _lib.ROP_DEREGISTER, _lib.ROP_SCALE_DOWN)
        ops["last_used"], ops["load_complete_time"] = now - 5, now
        ops["load_time"] = (now - 1000, recs[rb][2][0][1], 0, recs[rd][2][0][1])  # the failed load and the scale-down name their copy
        st, edits, info = s.registry_ops(ops, now)
        assert int(info["n_edits"]) == 4 and list(edits["model"]) == [ra, rb, rc, rd]
        recs2 = recs_of(s)
        failed_pod = int(ops["pod"][1])
        assert free in {p for p, _ in recs2[ra][2]} and failed_pod in {p for p, _ in recs2[rb][3]}
        assert len(recs2[rc][2]) == len(recs[rc][2]) - 1 and len(recs2[rd][2]) == len(recs[rd][2]) - 1
        items = fx.head(w) + [(ra, w.stored[ra], 0, -1, b""), (rb, w.stored[rb], 0, failed_pod, b'OOM "x"'),
                              (rc, w.stored[rc], int(edits[2]["last_unload_after"]), -1, b""),
                              (rd, w.stored[rd], int(edits[3]["last_unload_after"]), -1, b"")]
        b = fx.to_batch(items)
        fx.check_conditions(*fx.run_model(b, recs2, w.pod_ids))
        vals, _ = check(s, b, recs2, w.pod_ids)
        assert b'"%s":' % w.pod_ids[free].encode() in vals[8]
        assert b'"%s":{"msg":"OOM \\"x\\""}' % w.pod_ids[failed_pod].encode() in vals[9]
    finally:
        s.close()
        t.close()


def test_after_an_applied_prune(ctx):
    w, _, _, _ = ctx
    s, t, recs = start_rewrite(w)
    try:
        now, gone = int(w.fleet.now), 5
        s.remove_pods(np.array([gone], np.int32))
        s.commit()
        s.prune_registry(0, now)
        _, _, info = s.prune_registry(0, now + 700_000)
        recs2 = recs_of(s)
        touched = [r for r in range(5, len(recs)) if recs2[r] != recs[r]]
        assert touched and int(info["n_edits"]) >= len(touched)
        assert all(gone not in {p for p, _ in recs2[r][2] + recs2[r][3]} for r in touched)
        b = fx.to_batch(fx.head(w) + [(r, w.stored[r], r, gone, b"gone") for r in touched[:64]])
        fx.check_conditions(*fx.run_model(b, recs2, w.pod_ids))
        vals, st = check(s, b, recs2, w.pod_ids)
        assert not any(st[8:])
    finally:
        s.close()
        t.close()


def test_ids_joined_since_the_load_are_rendered(ctx):
    w, _, _, _ = ctx
    s, t, recs = start_rewrite(w)
    try:
        check(s, fx.to_batch(fx.head(w)), recs, w.pod_ids)  # (the device copy of the id store exists before the join)
        s.append_pod_ids(["late-joiner"])
        ids = list(w.pod_ids) + ["late-joiner"]
        v = b'{"mPath":"m20","instanceIds":{"late-joiner":11,"%s":12},"failedIn":{"late-joiner":13}}' % w.pod_ids[1].encode()
        assert not s.upsert_models_json([v], np.array([20], np.int32))[0].any()
        recs2 = recs_of(s)
        assert recs2[20][2] == ((8, 11), (1, 12)) and recs2[20][3] == ((8, 13),)
        b = fx.to_batch(fx.head(w) + [(20, v, 0, 8, b"late failure")])
        vals, st = check(s, b, recs2, ids)
        assert st[8] == 0 and b'"late-joiner":{"msg":"late failure"}' in vals[8]
    finally:
        s.close()
        t.close()


def test_after_pods_retire_the_new_numbering_and_status_2(ctx):
    w, _, _, _ = ctx
    s, t, recs = start_rewrite(w)
    try:
        gone = 3
        check(s, fx.to_batch(fx.head(w)), recs, w.pod_ids)  # (the device copy of the id store exists before the retire)
        remap, turned = s.pods_retire(np.array([gone], np.int32))
        assert turned > 0 and list(remap) == [0, 1, 2, -1, 3, 4, 5, 6]
        ids = [x for p, x in enumerate(w.pod_ids) if p != gone]
        recs2 = recs_of(s)
        named = [r for r in range(5, len(recs)) if gone in {p for p, _ in recs[r][2] + recs[r][3]}]
        moved = [r for r in range(5, len(recs)) if r not in named and any(p > gone for p, _ in recs[r][2] + recs[r][3])]
        assert named and moved
        b = fx.to_batch(fx.head(w) + [(r, w.stored[r], 1, -1, b"") for r in named[:20] + moved[:40]])
        vals, st = check(s, b, recs2, ids)
        assert all(x == 2 for x in st[8:8 + len(named[:20])]) and not any(st[8 + len(named[:20]):])
    finally:
        s.close()
        t.close()


def test_sizing_a_small_buffer_writes_nothing(ctx):
    w, s, _, recs = ctx
    b = fx.sized_batch(w, recs, 65)
    want, want_st = fx.run_model(b, recs, w.pod_ids)
    total = sum(len(v) for v in want if v is not None)
    args = (b.rows, b.olds, b.last_unload, (b.fail_pod, b.msgs))
    offs = np.concatenate([[0], np.cumsum([len(v) if v is not None else 0 for v in want])])
    for cap, null_out in ((0, True), (0, False), (total - 1, False), (total - 1, True)):
        out, off, st, tot, rc = s.models_rewrite_json_raw(*args, cap, fill=FILL, null_out=null_out)
        assert rc == 0 and tot == total and list(st) == want_st and np.array_equal(off, offs)
        assert (out == FILL).all()
    out, off, st, tot, rc = s.models_rewrite_json_raw(*args, total + 3, fill=FILL)
    assert rc == 0 and tot == total and bytes(out[:total]) == b"".join(v for v in want if v is not None)
    assert (out[total:] == FILL).all()


def test_refusals_leave_the_outputs_untouched(ctx):
    w, s, _, recs = ctx
    b = fx.sized_batch(w, recs, 63)
    fail = (b.fail_pod, b.msgs)

    def refused(rc_want, rows=b.rows, olds=b.olds, lul=b.last_unload, fail=fail, on=s, **kw):
        out, off, st, tot, rc = on.models_rewrite_json_raw(rows, olds, lul, fail, 4096, fill=FILL, **kw)
        assert rc == rc_want, (rc, kw)
        assert tot == -1 and (out == FILL).all() and (off.view(np.uint8) == FILL).all() and (st.view(np.uint8) == FILL).all()

    refused(EINVAL, flags=1)
    for bad_row in (-1, len(recs)):
        rows = b.rows.copy()
        rows[40] = bad_row
        refused(EINVAL, rows=rows)
    for bad_pod in (-2, len(w.pod_ids)):
        fp = b.fail_pod.copy()
        fp[62] = bad_pod
        refused(EINVAL, fail=(fp, b.msgs))
    off = np.concatenate([[0], np.cumsum([len(v) for v in b.olds])]).astype(np.int64)
    off[30] = off[31] + 1
    refused(EINVAL, old_off=off)
    moff = np.concatenate([[0], np.cumsum([len(m) for m in b.msgs])]).astype(np.int32)
    moff[6] = moff[7] + 1
    refused(EINVAL, msg_off=moff)
    refused(EINVAL, no_msgs=True)  # fail_pod without the two message arrays
    # NULL required buffers
    L, total = s.lib, C.c_int64(-1)
    o, st = np.full(2, -1, np.int64), np.full(1, -1, np.int32)
    one = (np.zeros(1, np.int32), np.array([0, 2], np.int64))
    assert L.mmp_models_rewrite_json(s.h, None, 1, b"{}", _lib.ptr(one[1]), None, None, None, None, 0, None, 0, _lib.ptr(o), _lib.ptr(st),
                                     C.byref(total)) == EINVAL
    assert L.mmp_models_rewrite_json(s.h, _lib.ptr(one[0]), 1, b"{}", _lib.ptr(one[1]), None, None, None, None, 0, None, 0, None,
                                     _lib.ptr(st), C.byref(total)) == EINVAL
    assert L.mmp_models_rewrite_json(s.h, _lib.ptr(one[0]), 1, b"{}", _lib.ptr(one[1]), None, None, None, None, 0, None, 0, _lib.ptr(o),
                                     _lib.ptr(st), None) == EINVAL
    assert total.value == -1 and list(o) == [-1, -1] and list(st) == [-1]
    # MMP_ESTATE: no id store; an instance table resized behind the id store's back
    fresh = Solver(1, 1)
    try:
        refused(ESTATE, on=fresh)
    finally:
        fresh.close()
    s2, t2, _ = start_rewrite(w)
    try:
        s2.load_pods(np.concatenate([w.fleet.pods, w.fleet.pods[:1]]))
        refused(ESTATE, on=s2)
    finally:
        s2.close()
        t2.close()
    check(s, b, recs, w.pod_ids)  # and the context still answers


def test_two_runs_are_byte_identical(ctx):
    w, s, _, recs = ctx
    b = fx.sized_batch(w, recs, 257)
    a1, a2 = rewrite(s, b), rewrite(s, b)
    assert a1[0] == a2[0] and np.array_equal(a1[1], a2[1])


def test_beside_a_census_reader(ctx):
    w, s, _, recs = ctx
    b = fx.sized_batch(w, recs, 256)
    want = rewrite(s, b)
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
            got = rewrite(s, b)
            assert got[0] == want[0] and np.array_equal(got[1], want[1])
    finally:
        stop.set()
        th.join()
    assert not errors, errors
    for c in reads:
        for x, y in zip(c, census0):
            assert np.array_equal(x, y)
