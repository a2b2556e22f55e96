"""tests/model_rewrite_model.py on values worked by hand — the model is the oracle of the rewrite kernels, so its own rule is
pinned here without a device — its semantics against json, its round trip through the parser's model, the entry point of the
C ABI and of the veneer, and the conditions every batch of tests/test_models_rewrite_gpu.py meets (from the model alone)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from modelmesh_amd import _lib
from tests import model_rewrite_fixtures as fx
from tests.ingest_model import model_bean
from tests.model_rewrite_model import HOST, MALFORMED, OK, escape, members, rewrite

IDS = ["a-1", "b-2", "c-3"]
EMPTY = (0, 0, (), ())
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rw(old, rec, lul=None, fail=None, **kw):
    val, st = rewrite(old.encode() if isinstance(old, str) else old, rec, IDS, lul, fail, **kw)
    assert st == OK
    return val


# ---- hand-worked values ---------------------------------------------------------------------------------------------------

def test_every_owned_member_present():
    old = '{"type":"t","instanceIds":{"zz":1},"failedIn":null,"fails":{"b-2":{"msg":"old"}},"lu":5,"lul":6,"refs":2}'
    rec = (0, 77, ((0, 10),), ((1, -1),))
    assert rw(old, rec, 9) == (b'{"type":"t","refs":2,"instanceIds":{"a-1":10},"failedIn":{"b-2":-1},'
                               b'"fails":{"b-2":{"msg":"old"}},"lu":77,"lul":9}')


def test_every_owned_member_absent_or_defaulted():
    assert rw('{"type":"t"}', EMPTY, 0) == b'{"type":"t"}'
    assert rw("{}", EMPTY, 0) == b"{}"
    assert rw('{"instanceIds":{"a-1":1},"failedIn":{"b-2":2},"fails":{"b-2":{"msg":"m"}},"lu":3,"lul":4}', EMPTY, 0) == b"{}"
    assert rw("{}", (0, 5, ((2, 1),), ()), 0) == b'{"instanceIds":{"c-3":1},"lu":5}'
    assert rw('{"mPath":"p"}', (0, 0, (), ((2, 1),)), 0) == b'{"mPath":"p","failedIn":{"c-3":1}}'


def test_duplicates_of_kept_and_of_owned_members():
    assert rw('{"a":1,"a":2,"lu":1,"lu":2,"a":3}', (0, 9, (), ())) == b'{"a":1,"a":2,"a":3,"lu":9}'
    assert rw('{"instanceIds":{"a-1":1},"k":null,"instanceIds":null}', (0, 0, ((1, 4), (0, 5)), ())) == \
        b'{"k":null,"instanceIds":{"b-2":4,"a-1":5}}'


def test_an_escaped_spelling_of_an_owned_name_is_some_other_member():
    # (names are matched by their raw bytes; the parsers' model calls an escaped KNOWN name unspecified, hence strict=False)
    assert rw('{"l\\u0075":4,"lu":5}', (0, 6, (), ()), strict=False) == b'{"l\\u0075":4,"lu":6}'
    assert rw('{"f\\u0061ils":{"a-1":1},"fails":{"a-1":{"msg":"m"}}}', (0, 0, (), ((0, 1),))) == \
        b'{"f\\u0061ils":{"a-1":1},"failedIn":{"a-1":1},"fails":{"a-1":{"msg":"m"}}}'


def test_fails_null_absent_doubled_stale_and_escaped():
    rec = (0, 0, (), ((0, 1),))
    want = b'{"failedIn":{"a-1":1}}'
    assert rw('{"fails":null,"failedIn":{"a-1":1}}', rec) == want
    assert rw('{"failedIn":{"a-1":1}}', rec) == want
    assert rw('{"fails":{}}', rec) == want
    assert rw('{"fails":{"a-1":{"msg":"1"}},"fails":{"a-1":{"msg":"2"}}}', rec) == want[:-1] + b',"fails":{"a-1":{"msg":"2"}}}'
    assert rw('{"fails":{"a-1":{"msg":"1"}},"fails":null}', rec) == want[:-1] + b',"fails":{"a-1":{"msg":"1"}}}'  # the last OBJECT
    assert rw('{"fails":{"zz":{"msg":"s"},"a-1":{"msg":"k", "t" : 5},"b-2":{"msg":"t"}}}', rec) == \
        want[:-1] + b',"fails":{"a-1":{"msg":"k", "t" : 5}}}'
    assert rw('{"fails":{"\\u0061-1":{"msg":"e"},"a-1":{"msg":"r"}}}', rec) == want[:-1] + b',"fails":{"a-1":{"msg":"r"}}}'
    assert rw('{"fails":{"\\u0061-1":{"msg":"e"}}}', rec) == want


def test_fail_pod_replace_remove_absent_and_escaping():
    old = '{"fails":{"a-1":{"msg":"o1"},"b-2":{"msg":"o2"}}}'
    rec = (0, 0, (), ((0, 1), (1, 2)))
    head = b'{"failedIn":{"a-1":1,"b-2":2},"fails":{'
    assert rw(old, rec, None, (0, b"new")) == head + b'"b-2":{"msg":"o2"},"a-1":{"msg":"new"}}}'      # replace
    assert rw(old, rec, None, (0, b"")) == head + b'"b-2":{"msg":"o2"}}}'                              # remove
    assert rw(old, rec, None, (2, b"m")) == head + b'"a-1":{"msg":"o1"},"b-2":{"msg":"o2"}}}'          # not in the failed list
    assert rw(old, rec, None, (-1, b"m")) == head + b'"a-1":{"msg":"o1"},"b-2":{"msg":"o2"}}}'
    assert rw("{}", rec, None, (1, b"first")) == b'{"failedIn":{"a-1":1,"b-2":2},"fails":{"b-2":{"msg":"first"}}}'
    assert rw("{}", (0, 0, ((1, 1),), ()), None, (1, b"loaded, not failed")) == b'{"instanceIds":{"b-2":1}}'
    msg = b'a"b\\c\nd\xc3\xa9\x1f'
    assert escape(msg) == b'a\\"b\\\\c\\u000ad\xc3\xa9\\u001f'
    assert rw(old, rec, None, (1, msg)) == head + b'"a-1":{"msg":"o1"},"b-2":{"msg":"a\\"b\\\\c\\u000ad\xc3\xa9\\u001f"}}}'
    assert json.loads(rw(old, rec, None, (1, msg)))["fails"]["b-2"]["msg"] == msg.decode()


def test_last_unload_null_zero_and_set():
    old = '{"lul":4,"x":1}'
    assert rw(old, EMPTY, None) == b'{"lul":4,"x":1}'
    assert rw(old, EMPTY, 0) == b'{"x":1}'
    assert rw(old, EMPTY, 8) == b'{"x":1,"lul":8}'


def test_whitespace_in_the_three_separator_styles():
    rec = (0, 3, (), ())
    assert rw('{"a":[1,2],"lu":1,"b":"x y"}', rec) == b'{"a":[1,2],"b":"x y","lu":3}'
    assert rw('{"a": [1, 2], "lu": 1, "b": "x y"}', rec) == b'{"a": [1, 2],"b": "x y","lu":3}'
    assert rw(' {"a" :\t[1 ,\n 2] ,\n "lu" :\t1 ,\n "b" :\t"x y" }\n', rec) == b'{"a" :\t[1 ,\n 2],"b" :\t"x y","lu":3}'
    assert rw("\n{ }\t", EMPTY) == b"{}"


def test_the_times():
    rec = (0, I64_MIN, ((0, 0), (1, -1), (2, 9)), ((0, 10), (1, 10**18), (2, I64_MAX)))
    assert rw("{}", rec, I64_MAX) == (b'{"instanceIds":{"a-1":0,"b-2":-1,"c-3":9},"failedIn":{"a-1":10,"b-2":1000000000000000000,'
                                      b'"c-3":9223372036854775807},"lu":-9223372036854775808,"lul":9223372036854775807}')


def test_the_statuses():
    assert rewrite(b'{"a":1', EMPTY, IDS) == (None, MALFORMED)
    assert rewrite(b"", EMPTY, IDS) == (None, MALFORMED)
    assert rewrite(b'{"lu":"3"}', EMPTY, IDS) == (None, MALFORMED)
    assert rewrite(b"{}", (0, 0, ((-1, 1),), ()), IDS) == (None, HOST)
    assert rewrite(b"{}", (0, 0, (), ((3, 1),)), IDS) == (None, HOST)
    assert rewrite(b'{"a":1', (0, 0, ((-1, 1),), ()), IDS) == (None, MALFORMED)  # malformed first
    for bad in ('q"', "b\\", "t\t", "é"):
        assert rewrite(b"{}", (0, 0, ((1, 1),), ()), ["a", bad]) == (None, HOST), bad
        assert rewrite(b"{}", (0, 0, ((0, 1),), ()), ["a", bad])[1] == OK  # (an id nobody renders is nobody's problem)
    with pytest.raises(ValueError):
        rewrite(b'{"x":1 2}', EMPTY, IDS)


# ---- semantics, round trip ------------------------------------------------------------------------------------------------

def _worlds():
    w = fx.rewrite_world(0)
    return w, fx.recs_after_setup(w)


def test_semantics_against_json_and_round_trip_through_the_parser():
    w, recs = _worlds()
    pod_of = {s: i for i, s in enumerate(w.pod_ids)}
    seen = 0
    for r, old in enumerate(w.stored):
        ty, lu, loaded, failed = recs[r]
        lul = (r * 7919) % 5 * 1000
        new, st = rewrite(old, recs[r], w.pod_ids, lul)
        if st == HOST:
            continue
        seen += 1
        want = {k: v for k, v in json.loads(old).items() if k not in ("instanceIds", "failedIn", "fails", "lu", "lul")}
        if loaded:
            want["instanceIds"] = {w.pod_ids[p]: t for p, t in loaded}
        if failed:
            want["failedIn"] = {w.pod_ids[p]: t for p, t in failed}
        fails = {k: v for k, v in (json.loads(old).get("fails") or {}).items() if k in {w.pod_ids[p] for p, _ in failed}}
        if fails:
            want["fails"] = fails
        if lu:
            want["lu"] = lu
        if lul:
            want["lul"] = lul
        got = json.loads(new)
        assert got == want, r
        assert list(got) == list(want), r  # the kept members in document order, the owned ones behind them in theirs
        b = model_bean(new, pod_of, w.type_names, 0)
        assert (b.status, b.type, b.lu, b.lul, tuple(b.loaded), tuple(b.failed)) == (0, ty, lu, lul, loaded, failed), r
    assert seen >= len(w.stored) - 2


# ---- the entry point ------------------------------------------------------------------------------------------------------

def test_the_entry_point_is_declared_bound_and_in_the_veneer():
    header = open(os.path.join(ROOT, "include", "mmplace.h")).read()
    assert "int mmp_models_rewrite_json(mmp_ctx *ctx" in header
    assert "mmp_models_rewrite_json" in {name for name, _, _ in _lib.SYMBOLS}
    for line, value in (("#define MMP_MRW_OK 0", _lib.MRW_OK), ("#define MMP_MRW_MALFORMED 1", _lib.MRW_MALFORMED),
                        ("#define MMP_MRW_HOST 2", _lib.MRW_HOST)):
        assert line in header and value == int(line.split()[-1])
    assert (OK, MALFORMED, HOST) == (_lib.MRW_OK, _lib.MRW_MALFORMED, _lib.MRW_HOST)
    assert "Java_com_ibm_watson_modelmesh_MmPlace_modelsRewriteJson" in open(os.path.join(ROOT, "integration", "mmplace_jni.cc")).read()
    assert "static native int modelsRewriteJson(" in open(os.path.join(ROOT, "integration", "GpuPlacementLB.java")).read()


def test_the_entry_point_refuses_a_null_context():
    L = _lib.load()
    total = C.c_int64(7)
    off, st, rows = np.full(2, 7, np.int64), np.full(1, 7, np.int32), np.zeros(1, np.int32)
    old = np.array([0, 2], np.int64)
    assert L.mmp_models_rewrite_json(None, _lib.ptr(rows), 1, b"{}", _lib.ptr(old), None, None, None, None, 0, None, 0,
                                     _lib.ptr(off), _lib.ptr(st), C.byref(total)) == -1  # MMP_EINVAL
    assert total.value == 7 and list(off) == [7, 7] and list(st) == [7]


# ---- the batches of the GPU tests -----------------------------------------------------------------------------------------

def test_every_gpu_batch_meets_the_fixture_conditions():
    w, recs = _worlds()
    batches = [fx.sized_batch(w, recs, n) for n in fx.SIZES if n >= 2] + [fx.same_row_batch(w)] + fx.tile_edge_batches(w) + fx.member_batches(w)
    for b in batches:
        fx.check_conditions(*fx.run_model(b, recs, w.pod_ids))
    # (n = 0 and n = 1 cannot hold three statuses: n = 1 runs once per status instead)
    assert [fx.run_model(b, recs, w.pod_ids)[1] for b in fx.single_batches(w)] == [[OK], [MALFORMED], [HOST]]
    ids, stored, erecs = fx.entry_world()
    fx.check_conditions(*fx.run_model(fx.entry_batch(ids, stored, erecs), erecs, ids))


def test_the_tile_edge_values_have_their_sizes_and_alignments():
    w, _ = _worlds()
    for a, b in enumerate(fx.tile_edge_batches(w)):
        assert len(b.olds[0]) % 4 == a  # the filler: the padded values behind it start at every dword alignment in turn
        sizes = [len(v) for v in b.olds[1:6]]
        assert sizes == [2046, 2047, 2048, 2049, 2050], sizes
        for v in b.olds[1:-8]:
            assert {k for k, _, _, _ in members(v, 0)} >= {b"type", b"fails", b"x", b"zz"}


def test_the_member_layouts_reach_what_they_are_meant_to_reach():
    """From the model alone: the last `fails` OBJECT decides wherever it stands, a `fails` that is no object is dropped and
    decides nothing, every value parses, and the padded value of a layout is the tile-sized one up to the pad."""
    w, recs = _worlds()
    p0, p2 = w.pod_ids[0], w.pod_ids[2]
    assert [p for p, _ in recs[1][3]] == [0, 2]
    layouts = fx.member_layouts(w)
    tile, padded = fx.member_batches(w)
    (tv, ts), (pv, ps) = (fx.run_model(b, recs, w.pod_ids) for b in (tile, padded))
    assert ts == ps and not any(ts[8:]) and len(tv) == 8 + len(layouts)
    assert {n for _, n, _ in layouts} == set(fx.MEMBER_COUNTS) and {0, 62, 63, 64, 129} <= {a for _, _, at in layouts for a in at}
    for (name, n, at), told, pold, t, p, fp, msg in zip(layouts, tile.olds[8:], padded.olds[8:], tv[8:], pv[8:], tile.fail_pod[8:],
                                                         tile.msgs[8:]):
        assert len(told) <= fx.TILE < len(pold) and len(members(told, 0)) == n and len(members(pold, 0)) == n + 1
        assert p.replace(fx.PAD, b"") == t and fx.PAD in p, name
        doc, old = json.loads(t), json.loads(told)
        assert json.loads(p)["pad"] == "p" * fx.TILE
        kept = [k for k in doc if k not in ("failedIn", "fails", "lul")]
        assert kept == [k for k in old if k != "fails"] and len(kept) == n - len(at), name  # no `fails` is ever kept
        objs = [v for _, v in sorted(at.items()) if v[:1] == b"{"]
        want = {}
        if objs:
            tag = json.loads(objs[-1])[p0]["msg"][:-2]
            assert tag == ("second" if name.startswith("obj-obj") else "first" if name.startswith("obj-") else "only")
            want = {p0: {"msg": tag + "-0"}, p2: {"msg": tag + "-2"}}
        if fp >= 0:
            want.pop(w.pod_ids[fp], None)
            want[w.pod_ids[fp]] = {"msg": msg.decode()}
        assert doc.get("fails", {}) == want, name
        assert ("fails" in doc) == (bool(objs) or fp >= 0) and (fp >= 0) == ("-msg" in name or (bool(objs) and fp == 2)), name
    names = [name for name, _, _ in layouts]  # non-objects only: no `fails` without a message, one for the message alone
    assert all("fails" not in json.loads(tv[8 + names.index(x)]) for x in ("non-20", "non-70"))
    assert all(list(json.loads(tv[8 + names.index(x)])["fails"]) == [p0] for x in ("non-msg-20", "non-msg-70"))
