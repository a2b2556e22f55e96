"""tests/model_refs_model.py pinned without a device: on values worked out by hand from VModelManager.java:294-302 / :475-489 and
ModelRecord.java:213-222, against `json`, and through tests/ingest_model.py (the read side's oracle).  And, from the model alone,
that every batch tests/test_models_refs_gpu.py sends holds all seven classes and both flags set and clear."""
import json

import pytest

from tests import model_refs_fixtures as fx
from tests import model_refs_model as mr
from tests.ingest_model import model_bean

INT_MAX, INT_MIN = (1 << 31) - 1, -(1 << 31)
LONG_MIN = -(1 << 63)
T1 = (b"t1", b"", b"")


def dec(old):
    return mr.refs_step(0, 0, None, old)


def inc(old, lu=0, info=None, flags=0):
    return mr.refs_step(mr.INC | flags, lu, info, old)


def test_every_class_on_the_head():
    b = fx.to_batch(fx.head())
    vals, classes, counts = fx.run_model(b)
    assert classes == list(mr.CLASSES)
    assert vals[mr.SET] == b'{"type":"type-1","mPath":"p","lu":1000,"instanceIds":{"i-0":5},"refs":1}'
    assert vals[mr.CREATED] == b'{"type":"type-1","encKey":"k","mPath":"p","refs":1,"autoDel":true,"lu":%d}' % fx.NOW
    assert [v is None for v in vals] == [False, False] + [True] * 5
    assert counts == [1, 1, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("stored,field,ret", [(None, 0, 0), (0, 0, 0), (1, 0, 0), (2, 1, 1), (-1, -1, 0), (INT_MAX, INT_MAX - 1, INT_MAX - 1),
                                              (INT_MIN, INT_MIN, 0)])
def test_dec(stored, field, ret):
    """ModelRecord.java:214 refCount > 0 ? --refCount : 0: the field moves only above 0, the return value is 0 at and below it."""
    old = b'{"type":"t"}' if stored is None else b'{"refs": %d ,"type":"t"}' % stored
    want = b'{"type":"t","refs":%d}' % field if field else b'{"type":"t"}'
    assert dec(old) == (want, mr.SET, ret)
    assert dec(old[:-1] + b',"autoDel":false}') == (want[:-1].replace(b',"refs"', b',"autoDel":false,"refs"') + b"}"
                                                    if field else b'{"type":"t","autoDel":false}', mr.SET, ret)
    # with autoDel the RETURN value decides (:478): from 1, from 0 and from below 0 the record goes
    assert dec(old[:-1] + b',"autoDel":true}')[1] == (mr.DELETE if ret == 0 else mr.SET)


@pytest.mark.parametrize("stored,after", [(None, 1), (0, 1), (1, 2), (2, 3), (-1, 0), (INT_MAX, INT_MIN), (INT_MIN, INT_MIN + 1)])
def test_inc(stored, after):
    """ModelRecord.java:221 ++refCount as a Java int; :301 setLastUsed sets unconditionally, lu is omitted at 0."""
    old = b'{"type":"t","lu":77}' if stored is None else b'{"refs":%d,"type":"t","lu":77}' % stored
    refs = b',"refs":%d' % after if after else b""
    assert inc(old, 5) == (b'{"type":"t"%s,"lu":5}' % refs, mr.SET, after)
    assert inc(old, 0) == (b'{"type":"t"%s}' % refs, mr.SET, after)
    assert inc(old, LONG_MIN) == (b'{"type":"t"%s,"lu":-9223372036854775808}' % refs, mr.SET, after)
    assert inc(old[:-1] + b',"autoDel":1}', 5)[1] == mr.SET  # an INC does not read autoDel


@pytest.mark.parametrize("raw", [b"2147483648", b"-2147483649", b"1.0", b'"1"', b"null", b"true", b"[1]", b"1e3"])
def test_refs_the_host_decides(raw):
    old = b'{"type":"t","refs":%s}' % raw
    assert dec(old) == (None, mr.HOST, 0) and inc(old, 5) == (None, mr.HOST, 0)
    assert dec(b'{"refs":%s,"type":"t","refs":2}' % raw) == (b'{"type":"t","refs":1}', mr.SET, 1)  # the first occurrence lost


def test_a_losing_first_occurrence_of_refs_is_dropped_too():
    assert dec(b'{"refs":7,"type":"t","refs":1}') == (b'{"type":"t"}', mr.SET, 0)
    assert inc(b'{"refs":7,"lu":1,"type":"t","lu":2,"refs":1}', 9) == (b'{"type":"t","refs":2,"lu":9}', mr.SET, 2)
    assert dec(b'{"refs":7,"lu":1,"type":"t","lu":2,"refs":1}') == (b'{"lu":1,"type":"t","lu":2}', mr.SET, 0)  # a DEC keeps lu


@pytest.mark.parametrize("auto,want", [(b"true", mr.DELETE), (b"false", mr.SET), (None, mr.SET), (b"null", mr.HOST), (b"1", mr.HOST),
                                       (b'"true"', mr.HOST)])
def test_auto_del(auto, want):
    old = b'{"refs":1}' if auto is None else b'{"refs":1,"autoDel":%s}' % auto
    assert dec(old)[1:] == (want, 0)
    assert inc(old, 0)[1:] == (mr.SET, 2)
    if want == mr.SET:
        assert dec(old)[0] == (b"{}" if auto is None else b'{"autoDel":false}')


def test_a_duplicate_auto_del_the_last_decides_and_all_stay():
    assert dec(b'{"autoDel":true,"refs":1,"autoDel":false}') == (b'{"autoDel":true,"autoDel":false}', mr.SET, 0)
    assert dec(b'{"autoDel":false,"refs":1,"autoDel":true}') == (None, mr.DELETE, 0)
    assert dec(b'{"autoDel":7,"refs":1,"autoDel":true}')[1] == mr.DELETE and dec(b'{"autoDel":true,"refs":1,"autoDel":7}')[1] == mr.HOST


def test_dec_to_zero_with_and_without_auto_del():
    assert dec(b'{"type":"t","refs":1,"autoDel":true}') == (None, mr.DELETE, 0)
    assert dec(b'{"type":"t","refs":1}') == (b'{"type":"t"}', mr.SET, 0)
    assert dec(b'{"type":"t","refs":2,"autoDel":true}') == (b'{"type":"t","autoDel":true,"refs":1}', mr.SET, 1)
    for refs in (0, -1):  # the return value is 0 although the field is not touched
        assert dec(b'{"type":"t","refs":%d,"autoDel":true}' % refs) == (None, mr.DELETE, 0)


def test_no_stored_value():
    assert dec(b"") == (None, mr.ENSURE_ABSENT, 0)
    assert mr.refs_step(mr.AUTO_DELETE, 9, T1, b"") == (None, mr.ENSURE_ABSENT, 0)
    assert inc(b"") == (None, mr.NOT_FOUND, 0) and inc(b"", 5, (b"", b"k", b"p")) == (None, mr.NOT_FOUND, 0)
    assert inc(b"", 0, T1) == (b'{"type":"t1","refs":1}', mr.CREATED, 1)
    assert inc(b"", 5, T1) == (b'{"type":"t1","refs":1,"lu":5}', mr.CREATED, 1)
    assert inc(b"", LONG_MIN, T1, mr.AUTO_DELETE) == (b'{"type":"t1","refs":1,"autoDel":true,"lu":-9223372036854775808}', mr.CREATED, 1)
    assert inc(b"", 5, (b"t1", b"k", b""))[0] == b'{"type":"t1","encKey":"k","refs":1,"lu":5}'
    assert inc(b"", 5, (b"t1", b"", b"/p"))[0] == b'{"type":"t1","mPath":"/p","refs":1,"lu":5}'
    assert inc(b"", 5, (b"t1", b'a"b', b"c\\d\n"), mr.AUTO_DELETE)[0] == \
        b'{"type":"t1","encKey":"a\\"b","mPath":"c\\\\d\\u000a","refs":1,"autoDel":true,"lu":5}'


def test_malformed_is_the_parsers_verdict():
    for old in (b" ", b"{", b'{"type":"t1"', b'{"type":"t1"} x', b'{"lu":"5"}', b'{"instanceIds":{"a":"b"}}', b"[]", b'{"type":"t1",}'):
        assert dec(old) == (None, mr.MALFORMED, 0) and inc(old, 5) == (None, mr.MALFORMED, 0), old
    with pytest.raises(ValueError):
        dec(b'{"type":"t\\u0031"}')


def test_unknown_members_of_every_json_type_stay_verbatim():
    kept = b'"a" : [1, {"refs":5}] , "b":{"refs":1,"lu":2},"c":"x\\"refs\\"", "d":-1.5e3,"e":true,"f":null'
    old = b' { "refs":3, ' + kept + b' , "lu" : 6 } '
    same = kept.replace(b" , ", b",").replace(b'"x\\"refs\\"", ', b'"x\\"refs\\"",')
    assert dec(old) == (b"{" + same + b',"lu" : 6,"refs":2}', mr.SET, 2)
    assert inc(old, 8) == (b"{" + same + b',"refs":4,"lu":8}', mr.SET, 4)


def _rendered(batch):
    vals, classes, counts = fx.run_model(batch)
    return [(i, v, c, r) for i, (v, c, r) in enumerate(zip(vals, classes, counts)) if c in mr.RENDERED]


@pytest.fixture(scope="module")
def batches():
    return fx.every_batch()


def _loads(v):
    return json.loads(v.decode("utf-8", "surrogateescape"), object_pairs_hook=list)


def test_against_json(batches):
    """The new value means the old one with the owned keys replaced."""
    seen = set()
    for b in batches:
        for i, v, c, r in _rendered(b):
            doc = _loads(v)
            flags, lu = b.reqs[i]
            if c == mr.CREATED:
                typ, enc, path = (x.decode("utf-8", "surrogateescape") for x in b.infos[i])
                want = [("type", typ)] + [("encKey", enc)] * bool(enc) + [("mPath", path)] * bool(path) + [("refs", 1)] + \
                       [("autoDel", True)] * bool(flags & mr.AUTO_DELETE) + [("lu", lu)] * bool(lu)
                assert doc == want and r == 1, (i, v)
                seen.add((c, bool(flags & mr.AUTO_DELETE)))
                continue
            old = _loads(b.olds[i])
            refs = dict(old).get("refs", 0)
            if flags & mr.INC:
                after = mr.jint(refs + 1)
                assert r == after
                assert doc == [(k, x) for k, x in old if k not in ("refs", "lu")] + [("refs", after)] * bool(after) + [("lu", lu)] * bool(lu)
            else:
                after = refs - 1 if refs > 0 else refs
                assert r == max(after, 0) and not (r == 0 and dict(old).get("autoDel", False))
                assert doc == [(k, x) for k, x in old if k != "refs"] + [("refs", after)] * bool(after), (i, v)
            seen.add((c, bool(flags & mr.INC)))
    assert seen == {(mr.SET, False), (mr.SET, True), (mr.CREATED, False), (mr.CREATED, True)}


def test_through_the_read_sides_oracle(batches):
    """The new value parses back to the intended record: the type, the entries and lul of the old one, lu as the step sets it."""
    ids, names = ["i-%d" % p for p in range(8)], ["NLCLASSIFIER", "type-1", "type-2"]
    n = 0
    for b in batches:
        for i, v, c, _r in _rendered(b):
            got = model_bean(v, ids, names, 3)
            flags, lu = b.reqs[i]
            assert got.status == 0, (i, v)
            if c == mr.CREATED:
                typ = b.infos[i][0].decode()
                assert (got.type, got.lu, got.lul, got.loaded, got.failed) == (names.index(typ) if typ in names else 3, lu, 0, [], [])
            else:
                old = model_bean(b.olds[i], ids, names, 3)
                assert got.lu == (lu if flags & mr.INC else old.lu)
                assert (got.type, got.lul, got.loaded, got.failed) == (old.type, old.lul, old.loaded, old.failed)
            n += 1
    assert n > 300  # (not vacuous)


def test_every_batch_the_gpu_test_sends_holds_every_class_and_flag():
    values = fx.corpus_values()
    assert len(values) > 1000
    for b in fx.every_batch(values):
        assert len(b.reqs) >= 7 and fx.holds_everything(b)
    assert [fx.run_model(b)[1] for b in fx.single_batches()] == [[c] for c in mr.CLASSES]
    drawn = fx.Batch(*zip(*[((f, t), i, o) for f, t, i, o in fx.drawn_items(250, 257)]))
    assert set(fx.run_model(drawn)[1]) == set(mr.CLASSES)  # the drawn requests bring every class on their own
    lens = [len(o) for o in fx.tile_edge_batch().olds]
    assert all(lens.count(n) == 8 for n in range(fx.TILE - 2, fx.TILE + 3))
    assert fx.run_model(fx.repeated_batch())[1][7:] == [mr.SET] * 64
    classes = fx.run_model(fx.boundary_batch())[1]
    assert classes.count(mr.HOST) > 60 and classes.count(mr.DELETE) > 5


def test_a_generator_refuses_a_batch_that_lacks_a_class_or_a_flag():
    head = fx.head()
    for k in range(len(head)):
        with pytest.raises(ValueError):
            fx.to_batch(head[:k] + head[k + 1:] + [head[(k + 1) % len(head)]])
    no_auto = [(f & ~mr.AUTO_DELETE, t, i, o) for f, t, i, o in head]
    with pytest.raises(ValueError):
        fx.to_batch(no_auto)


def test_the_padded_member_layouts_answer_as_the_tile_sized_ones():
    tile, padded = fx.member_batch(), fx.padded_member_batch()
    (tv, tc, tr), (pv, pc, pr) = fx.run_model(tile), fx.run_model(padded)
    assert (tc, tr) == (pc, pr) and len(tc) == 7 + 2 * 5 * len(fx.MEMBER_COUNTS)
    assert set(tc[7:]) == {mr.SET, mr.DELETE}
    drop_pad = lambda v: [(k, x) for k, x in json.loads(v, object_pairs_hook=list) if k != "pad"]  # noqa: E731
    for i in range(7, len(tc)):
        assert len(tile.olds[i]) <= fx.TILE < len(padded.olds[i])
        assert (tv[i] is None) == (pv[i] is None)
        if tv[i] is not None:
            assert drop_pad(pv[i]) == json.loads(tv[i], object_pairs_hook=list), i
