"""tests/model_register_model.py pinned without a device: on values worked out by hand from ModelMesh.java:3088-3147 / :3181-3203,
against `json`, and through tests/ingest_model.py (the read side's oracle).  And, from the model alone, that every batch
tests/test_models_register_gpu.py sends holds all nine classes."""
import json

import pytest

from tests import model_register_fixtures as fx
from tests import model_register_model as mm
from tests.ingest_model import model_bean

NOW, AGE = 1_000_000, 1_000
MAX = (1 << 63) - 1
T1 = (b"t1", b"", b"")


def reg(old, info=T1, flags=0, ict=0, now=NOW, age=AGE):
    return mm.register(flags, ict, info, old, now, age)


def test_every_class_on_the_head():
    b = fx.to_batch(fx.head())
    vals, classes, lus = fx.run_model(b)
    assert classes == list(mm.CLASSES)
    ts = fx.NOW - 6 * fx.AGE
    assert vals[mm.CREATED] == b'{"type":"type-1","encKey":"k","mPath":"p","lu":%d}' % ts
    assert vals[mm.TOUCHED] == b'{"type":"type-1","mPath":"p","instanceIds":{"i-0":5},"lu":%d}' % ts
    assert [v is None for v in vals] == [False, False] + [True] * 7
    assert lus == [ts, ts, fx.NOW - fx.AGE, ts, 0, 0, 0, ts, ts]


@pytest.mark.parametrize("ict,load_now,want", [
    (0, False, NOW - 6 * AGE), (0, True, NOW - AGE),  # :3101 6x older if we're not loading now
    (1, False, 1), (1, True, 1), (NOW - 1, False, NOW - 1), (NOW - 1, True, NOW - 1),  # :3099 ict > 0
    (NOW, False, NOW), (NOW, True, NOW), (NOW + 1, False, NOW), (NOW + 1, True, NOW),  # :3098 ict >= now
    (-5, False, NOW - 6 * AGE)])
def test_last_used_timestamp(ict, load_now, want):
    flags = mm.LOAD_NOW if load_now else 0
    assert mm.last_used_timestamp(flags, ict, NOW, AGE) == want
    v, c, t = reg(b"", flags=flags, ict=ict)
    assert (c, t) == (mm.CREATED, want) and v == b'{"type":"t1","lu":%d}' % want
    assert reg(b"", flags=mm.DELETE | flags, ict=ict) == (None, mm.ABSENT, 0)


def test_the_product_and_the_difference_wrap():
    assert mm.last_used_timestamp(0, 0, 5, MAX) == mm.jlong(5 - mm.jlong(MAX * 6)) == 11  # MAX * 6 wraps to -6
    assert mm.last_used_timestamp(mm.LOAD_NOW, 0, 5, MAX) == 5 - MAX


def test_the_touch_rule_at_its_edge():
    ts = NOW - 6 * AGE
    for lu, want in ((ts - AGE - 1, mm.TOUCHED), (ts - AGE, mm.EXISTS), (ts - AGE + 1, mm.EXISTS)):
        old = b'{"type":"t1","lu":%d,"refs":1}' % lu
        v, c, t = reg(old)
        assert (c, t) == (want, ts), lu
        assert v == (b'{"type":"t1","refs":1,"lu":%d}' % ts if want == mm.TOUCHED else None)
        assert reg(old, flags=mm.LOAD_NOW)[1:] == (mm.EXISTS, NOW - AGE)  # :3120 !loadNow
    # the same edge with an explicit timestamp
    assert reg(b'{"type":"t1","lu":%d}' % (500 - AGE - 1), ict=500) == (b'{"type":"t1","lu":500}', mm.TOUCHED, 500)
    assert reg(b'{"type":"t1","lu":%d}' % (500 - AGE), ict=500) == (None, mm.EXISTS, 500)


def test_lu_at_long_max_the_sum_wraps_and_lu_stays():
    old = b'{"type":"t1","lu":%d,"autoDel":true}' % MAX
    assert reg(old) == (b'{"type":"t1","autoDel":true,"lu":%d}' % MAX, mm.TOUCHED, NOW - 6 * AGE)


def test_a_timestamp_of_zero_means_now():
    now, age = 6_000, 1_000  # now == age * 6
    assert mm.last_used_timestamp(0, 0, now, age) == 0
    assert mm.register(0, 0, T1, b"", now, age) == (b'{"type":"t1"}', mm.CREATED, 0)  # lu at its default: omitted
    assert mm.register(0, 0, T1, b'{"type":"t1","lu":-1001}', now, age) == (b'{"type":"t1","lu":6000}', mm.TOUCHED, 0)
    assert mm.register(0, 0, T1, b'{"type":"t1","lu":-1000}', now, age) == (None, mm.EXISTS, 0)
    assert mm.register(0, 0, T1, b'{"type":"t1"}', now, age) == (None, mm.EXISTS, 0)


def test_the_three_attributes():
    old = b'{"type":"t1","encKey":"k","mPath":"p","lu":%d}' % NOW
    assert reg(old, (b"t1", b"k", b"p"))[1] == mm.EXISTS
    for info in ((b"t2", b"k", b"p"), (b"t1", b"K", b"p"), (b"t1", b"k", b"pp"), (b"t1", b"", b"p"), (b"t1", b"k", b""), (b"t", b"k", b"p")):
        assert reg(old, info)[1] == mm.CONFLICT, info
    # null against null, and a stored "" is not the request's null (:3094-3095 map the REQUEST's "" to null, not the record's)
    assert reg(b'{"type":"t1","encKey":null,"lu":%d}' % NOW)[1] == mm.EXISTS
    assert reg(b'{"type":"t1","encKey":"","lu":%d}' % NOW)[1] == mm.CONFLICT
    assert reg(b'{"type":"t1","mPath":"","lu":%d}' % NOW)[1] == mm.CONFLICT
    assert reg(b'{"type":"t1","mPath":"","lu":%d}' % NOW, (b"t1", b"", b"x"))[1] == mm.CONFLICT


def test_type_absent_and_null_read_as_the_default():
    for old in (b'{"lu":%d}' % NOW, b'{"type":null,"lu":%d}' % NOW, b'{"type":"t1","type":null,"lu":%d}' % NOW, b"{}"):
        assert reg(old, (b"NLCLASSIFIER", b"", b""))[1] in (mm.EXISTS, mm.TOUCHED), old
        assert reg(old, T1)[1] == mm.CONFLICT, old
    assert reg(b"{}", (b"NLCLASSIFIER", b"", b"")) == (b'{"lu":%d}' % (NOW - 6 * AGE), mm.TOUCHED, NOW - 6 * AGE)
    assert reg(b" { } ", (b"NLCLASSIFIER", b"", b""))[0] == b'{"lu":%d}' % (NOW - 6 * AGE)


def test_the_last_occurrence_decides():
    assert reg(b'{"type":"t1","encKey":"a","lu":%d,"encKey":"b"}' % NOW, (b"t1", b"b", b""))[1] == mm.EXISTS
    assert reg(b'{"type":"t1","encKey":"a","lu":%d,"encKey":"b"}' % NOW, (b"t1", b"a", b""))[1] == mm.CONFLICT
    assert reg(b'{"type":"t1","encKey":"a\\\\b","lu":5,"encKey":null}')[1] == mm.TOUCHED  # the escaped one lost
    assert reg(b'{"type":"t1","encKey":null,"lu":5,"encKey":"a\\\\b"}')[1] == mm.HOST
    assert reg(b'{"lu":%d,"type":"t1","lu":5}' % NOW) == (b'{"type":"t1","lu":%d}' % (NOW - 6 * AGE), mm.TOUCHED, NOW - 6 * AGE)
    assert reg(b'{"refs":1,"refs":0}', flags=mm.DELETE)[1] == mm.DELETABLE
    assert reg(b'{"refs":0,"refs":1}', flags=mm.DELETE)[1] == mm.REFERENCED


def test_the_host_decides():
    for member in (b'"encKey":"a\\"b"', b'"mPath":"a\\u0041"', b'"encKey":5', b'"mPath":{"a":1}', b'"mPath":true', b'"encKey":["k"]'):
        assert reg(b'{"type":"t1",%s}' % member)[1] == mm.HOST, member
        assert reg(b'{"type":"t2",%s}' % member)[1] == mm.HOST, member  # (before the conflict: the device does not compare at all)
        assert reg(b'{"type":"t1",%s}' % member, flags=mm.DELETE)[1] == mm.DELETABLE  # a delete does not compare them


@pytest.mark.parametrize("refs,want", [(b"0", mm.DELETABLE), (b"1", mm.REFERENCED), (b"-1", mm.DELETABLE), (None, mm.DELETABLE),
                                       (b"2147483647", mm.REFERENCED), (b"2147483648", mm.HOST), (b"-2147483648", mm.DELETABLE),
                                       (b"-2147483649", mm.HOST), (b'"1"', mm.HOST), (b"1.0", mm.HOST), (b"null", mm.HOST)])
def test_refs(refs, want):
    old = b'{"type":"t1"}' if refs is None else b'{"type":"t1", "refs" : %s ,"lu":3}' % refs
    assert reg(old, flags=mm.DELETE, ict=99) == (None, want, 0)  # :3188 getRefCount() > 0
    assert reg(old)[1] == mm.TOUCHED  # a register does not look at refs


def test_malformed_is_the_parsers_verdict():
    for old in (b" ", b"{", b'{"type":"t1"', b'{"type":"t1"} x', b'{"lu":"5"}', b'{"instanceIds":{"a":"b"}}', b"[]", b'{"type":"t1",}'):
        assert reg(old)[1] == mm.MALFORMED and reg(old, flags=mm.DELETE)[1:] == (mm.MALFORMED, 0), old
    with pytest.raises(ValueError):
        reg(b'{"type":"t\\u0031"}')


def _rendered(batch):
    vals, classes, lus = fx.run_model(batch)
    return [(i, v, c, t) for i, (v, c, t) in enumerate(zip(vals, classes, lus)) if c in (mm.CREATED, mm.TOUCHED)]


@pytest.fixture(scope="module")
def batches():
    return fx.every_batch()


def test_against_json(batches):
    seen = set()
    for b in batches:
        for i, v, c, ts in _rendered(b):
            doc = json.loads(v.decode("utf-8", "surrogateescape"), object_pairs_hook=list)
            typ, enc, path = (x.decode("utf-8", "surrogateescape") for x in b.infos[i])
            if c == mm.CREATED:  # exactly the four members, in the bean's order, each omitted at null / 0
                want = [("type", typ)] + [("encKey", enc)] * bool(enc) + [("mPath", path)] * bool(path) + [("lu", ts)] * bool(ts)
                assert doc == want, (i, v)
            else:  # the old one with lu replaced
                old = json.loads(b.olds[i].decode("utf-8", "surrogateescape"), object_pairs_hook=list)
                lu = dict(old).get("lu", 0)
                lu2 = max(lu, ts if ts else fx.NOW)
                assert doc == [(k, x) for k, x in old if k != "lu"] + [("lu", lu2)] * bool(lu2), (i, v)
                assert ts > mm.jlong(lu + fx.AGE)
            seen.add(c)
    assert seen == {mm.CREATED, mm.TOUCHED}


def test_through_the_read_sides_oracle(batches):
    ids, names = ["i-%d" % p for p in range(8)], ["NLCLASSIFIER", "type-1", "type-2"]
    n = 0
    for b in batches:
        for i, v, c, ts in _rendered(b):
            got = model_bean(v, ids, names, 3)
            typ = b.infos[i][0].decode()
            assert got.status == 0 and got.type == (names.index(typ) if typ in names else 3), (i, v)
            if c == mm.CREATED:
                assert (got.lu, got.lul, got.loaded, got.failed) == (ts, 0, [], [])
            else:
                old = model_bean(b.olds[i], ids, names, 3)
                assert got.lu == max(old.lu, ts if ts else fx.NOW)
                assert (got.type, got.lul, got.loaded, got.failed) == (old.type, old.lul, old.loaded, old.failed)
            n += 1
    assert n > 100  # (not vacuous)


def test_every_batch_the_gpu_test_sends_holds_all_nine_classes():
    values = fx.corpus_values()
    assert len(values) > 1000
    for b in fx.every_batch(values):
        assert len(b.reqs) >= 9 and fx.has_every_class(b)
    assert [fx.run_model(b)[1] for b in fx.single_batches()] == [[c] for c in mm.CLASSES]
    # beyond the head: the drawn requests of the largest batch bring every class on their own, and both sides of the tile
    drawn = fx.to_batch(fx.drawn_items(248, 257))
    assert set(fx.run_model(drawn)[1]) == set(mm.CLASSES)
    lens = [len(o) for o in fx.tile_edge_batch().olds]
    assert {fx.TILE - 2, fx.TILE - 1, fx.TILE, fx.TILE + 1, fx.TILE + 2} <= set(lens)
    classes = fx.run_model(fx.string_batch())[1]
    assert classes.count(mm.CONFLICT) > 40 and classes.count(mm.TOUCHED) == 3 * (len(fx.STRING_LENGTHS) - 1) + 1  # (length 0: a stored "" equals nothing)


def test_the_padded_member_layouts_answer_as_the_tile_sized_ones():
    """The same class and last_used from either, on every class a layout is meant to reach, and values equal up to the pad."""
    tile, padded = fx.member_batch(), fx.padded_member_batch()
    (tv, tc, tl), (pv, pc, pl) = fx.run_model(tile), fx.run_model(padded)
    assert (tc, tl) == (pc, pl) and len(tc) == 9 + 2 * 5 * len(fx.MEMBER_COUNTS)
    assert {c for c in tc[9:]} == {mm.TOUCHED, mm.CONFLICT, mm.REFERENCED, mm.DELETABLE}
    for i in range(9, len(tc)):
        told, pold = tile.olds[i], padded.olds[i]
        assert len(told) <= fx.TILE < len(pold)
        drop_pad = lambda v: [(k, x) for k, x in json.loads(v, object_pairs_hook=list) if k != "pad"]  # noqa: E731
        assert drop_pad(pold) == json.loads(told, object_pairs_hook=list)
        assert (tv[i] is None) == (pv[i] is None) == (tc[i] != mm.TOUCHED)
        if tv[i] is not None:
            assert drop_pad(pv[i]) == json.loads(tv[i], object_pairs_hook=list), i
