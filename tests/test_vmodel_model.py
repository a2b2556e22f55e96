"""tests/vmodel_model.py worked by hand — the resolve classes, the parser's rules, the transition prologue — and, from the model
alone, the coverage of the batches tests/test_vmodels_gpu.py sends: a corpus that lacks a class is an error of the test."""
import json

import numpy as np
import pytest

from tests import vmodel_fixtures as fx
from tests import vmodel_model as vm
from tests.ingest_model import ACCEPT, REJECT, UNSPECIFIED

REG = vm.Registry([b"act", b"tgt", b"failed-only", b"gone", b"three", b"lu0", b"lumax", b"lu1"],
                  [(1, 0, 50, 0), (1, 0, 60, 0), (0, 2, 70, 0), (0, 0, 0, 0), (3, 1, 80, 0), (1, 0, 0, 0), (2, 0, fx.LONG_MAX, 0), (1, 0, 1, 0)])


def table(*records):
    m = vm.VModels()
    st, idx, n = m.events([b"v%d" % i for i in range(len(records))], list(records))
    assert not st.any() and list(idx) == list(range(len(records))) and n == len(records)
    return m


def test_resolve_first_phase():
    m = table('{"amid":"act","tmid":"tgt","o":"me"}')
    A = vm.Answer
    ok = A(vm.OK, vm.ACTIVE, 0, 0, 1, vm.TRANSITIONING, vm.T_LOADING, 0)
    assert m.resolve(REG, b"v0") == ok  # :575 notFoundModelId == null
    assert m.resolve(REG, b"v0", nf=b"") == ok  # empty is null
    assert m.resolve(REG, b"v0", nf=b"tgt") == ok  # differs from active
    assert m.resolve(REG, b"v0", nf=b"ac") == ok and m.resolve(REG, b"v0", nf=b"acT") == ok
    assert m.resolve(REG, b"v0", nf=b"act") == ok._replace(cls=vm.STRONG_READ, model=-1)  # :582
    assert m.resolve(REG, b"nope") == A(vm.NOT_FOUND, 0, -1, -1, -1, 0, 0, 0)  # :570-573


def test_resolve_after_the_strong_read():
    m = table('{"amid":"act","tmid":"tgt"}', '{"amid":"act","tmid":"act"}', '{"amid":"act"}', '{"tmid":"act"}')
    r = lambda k, nf: m.resolve(REG, k, nf=nf, after_strong=True)  # noqa: E731
    assert r(b"v0", b"other")[:4] == (vm.OK, vm.ACTIVE, 0, 0)  # nf equal to neither: :587
    assert r(b"v0", b"tgt")[:4] == (vm.OK, vm.ACTIVE, 0, 0)  # nf == target only: active still differs
    assert r(b"v0", b"act")[:4] == (vm.OK, vm.TARGET, 0, 1)  # nf == active: the target, :591
    assert r(b"v1", b"act")[:4] == (vm.TARGET_NOT_FOUND, 0, 1, -1)  # nf == both: :594
    assert r(b"v1", None)[:4] == (vm.OK, vm.ACTIVE, 1, 0) and r(b"v1", b"")[:4] == (vm.OK, vm.ACTIVE, 1, 0)
    # a null id equals nothing: nf == active, target null -> the Java returns null
    a = r(b"v2", b"act")
    assert a[:5] == (vm.OK, vm.TARGET, 2, -1, -1) and a.flags == vm.NULL_ID and a.vstatus == vm.TRANSITIONING and a.target_status == vm.T_NOT_FOUND
    a = r(b"v3", b"act")  # active null: differs from any nf
    assert a[:5] == (vm.OK, vm.ACTIVE, 3, -1, 0) and a.flags == vm.NULL_ID
    assert m.resolve(REG, b"v3", nf=b"act").cls == vm.OK  # ... in the first phase too


def test_owner_rule():
    m = table('{"amid":"act","tmid":"act","o":"owner"}', '{"amid":"act","tmid":"act"}', '{"amid":"act","tmid":"act","o":""}')
    found = lambda k, o: m.resolve(REG, k, owner=o).cls == vm.OK  # noqa: E731
    assert found(b"v0", None) and found(b"v0", b"") and found(b"v0", b"owner")  # absent, empty (emptyToNull), equal
    assert not found(b"v0", b"ownes") and not found(b"v0", b"owne") and not found(b"v0", b"owner2")  # last byte, shorter, longer
    assert found(b"v1", None) and not found(b"v1", b"owner")  # given against OWNER_NULL
    assert not found(b"v2", b"x") and found(b"v2", None)  # a stored "" is not null: it differs from "x"
    assert m.resolve(REG, b"v0", owner=b"ownes") == vm.Answer(vm.NOT_FOUND, 0, -1, -1, -1, 0, 0, 0)


def test_status_classes():
    m = table('{"amid":"act","tmid":"act"}', '{"amid":"act","tmid":"tgt"}', '{"amid":"act","tmid":"tgt","failed":true}',
              '{"amid":"act","tmid":"failed-only","failed":true}', '{"amid":"act","tmid":"failed-only"}',
              '{"amid":"act","tmid":"gone","failed":true}', '{"amid":"act","tmid":"unheard-of"}', '{"amid":"act","tmid":"three","failed":true}',
              '{}', '{"amid":"a\\\\b","tmid":"act"}')
    want = [(vm.DEFINED, vm.T_NONE, 0), (vm.TRANSITIONING, vm.T_LOADING, 1), (vm.TRANSITION_FAILED, vm.T_LOADING, 1),
            (vm.TRANSITION_FAILED, vm.T_LOADING_FAILED, 2), (vm.TRANSITIONING, vm.T_LOADING, 2), (vm.TRANSITION_FAILED, vm.T_NOT_FOUND, 3),
            (vm.TRANSITIONING, vm.T_NOT_FOUND, -1), (vm.TRANSITION_FAILED, vm.T_LOADING, 4), (vm.DEFINED, vm.T_NONE, -1)]
    for i, (vs, ts, tm) in enumerate(want):
        a = m.resolve(REG, b"v%d" % i)
        assert (a.cls, a.vstatus, a.target_status, a.target_model) == (vm.OK, vs, ts, tm), i
    assert m.resolve(REG, b"v9") == vm.Answer(vm.HOST, 0, 9, -1, -1, 0, 0, 0)
    assert m.resolve(REG, b"v8").flags == vm.NULL_ID and m.flags()[8] == vm.F_ACTIVE_NULL | vm.F_TARGET_NULL | vm.F_OWNER_NULL


def test_parser_rules():
    p = vm.parse
    assert p('{"amid":"a","tmid":"b","failed":true}') == (0, vm.Row(b"a", b"b", None, True, False))
    assert p('{"amid":"a","failed":false}')[1].failed is False and p('{"amid":"a"}')[1].failed is False
    assert p('{"amid":"a","amid":null}')[1].amid is None  # a later null wins over an earlier string
    assert p('{"amid":null,"amid":"a"}')[1].amid == b"a"
    assert p('{"amid":7,"amid":"a"}') == (1, None)  # an earlier duplicate of the wrong type is malformed
    assert p('{"failed":"no","failed":true}') == (1, None) and p('{"failed":null}') == (1, None)
    for unknown in ("1", "-2.5e3", '"s"', "true", "false", "null", "[1,[2]]", '{"amid":7}'):  # unknown members of every JSON type
        assert p('{"later":%s,"amid":"a","x":%s}' % (unknown, unknown)) == (0, vm.Row(b"a", None, None, False, False)), unknown
    assert p('{"o":"a\\"b"}')[1] == vm.Row(None, None, b'a\\"b', False, True)  # raw bytes, flagged HOST
    assert p('{"amid":"é"}')[1].amid == "é".encode()
    assert p('{"amid":"a"} ')[0] == 0 and p('{"amid":"a"} x')[0] == 1 and p("")[0] == 1
    assert vm.classify('{"x":1 2,"amid":"a"}')[0] == UNSPECIFIED and vm.classify('{"\\u0061mid":"a"}')[0] == UNSPECIFIED
    with pytest.raises(ValueError):
        p('{"x":01}')


def test_events_apply_in_order():
    m = vm.VModels()
    st, idx, n = m.events([b"a", b"b", b"a", b"c", b"a", b"d", b"d"], ['{"amid":"1"}', "", '{"amid":"2"', '{"amid":"3"}', "", "{", '{"o":"x"}'],
                          [0, 1, 0, 0, 1, 0, 0])
    assert list(st) == [0, 2, 1, 0, 0, 1, 0] and list(idx) == [0, -1, 0, 1, 0, 2, 2] and n == 3
    assert m.rows == [None, vm.Row(b"3", None, None, False, False), vm.Row(None, None, b"x", False, False)]
    st, idx, n = m.events([b"a", b"e", b"b"], ['{"amid":"again"}', "{}", "{}"], None, append=False)  # set again: its old row back
    assert list(st) == [0, 2, 2] and list(idx) == [0, -1, -1] and n == 0 and m.rows[0].amid == b"again"
    assert m.info() == (3, 3, 7)


def test_transition_prologue():
    m = table('{"amid":"gone","tmid":"tgt"}', '{"amid":"act","tmid":"tgt","failed":true}', '{"amid":"three","tmid":"gone"}',
              '{"amid":"lu0","tmid":"tgt"}', '{"amid":"lumax","tmid":"nowhere"}', '{"amid":"lu1","tmid":"tgt"}', '{"amid":"act","tmid":"act"}',
              '{"amid":"a\\\\","tmid":"tgt"}', '{"tmid":"tgt"}', '{"amid":"failed-only","tmid":"tgt"}')
    m.events([b"dead"], [""], [0])
    m.events([b"dead"], [""], [1])
    rows, info = m.transitions(REG, 1000, 300)
    T = vm.Transition
    assert rows == [T(0, 3, 1, 0, vm.PROMOTE, vm.XF_FROM_EMPTY, 0),  # target_count 0
                    T(1, 0, 1, 1, vm.ENSURE_LOADED, vm.XF_FAILED, 50),  # 1
                    T(2, 4, 3, 3, vm.ENSURE_LOADED, vm.XF_TO_EMPTY, 80),  # 3
                    T(3, 5, 1, 1, vm.ENSURE_LOADED, 0, 700),  # last_used 0 -> now - age
                    T(4, 6, -1, 2, vm.ENSURE_LOADED, 0, fx.LONG_MAX),  # Long.MAX_VALUE stays
                    T(5, 7, 1, 1, vm.ENSURE_LOADED, 0, 1),  # 1 is not 0
                    T(8, -1, 1, 0, vm.PROMOTE, 0, 0),  # active null: curActive == null
                    T(9, 2, 1, 0, vm.PROMOTE, 0, 0)]  # failed copies are not instanceIds
    assert info == (8, 3, 5, 1)
    assert m.transitions(REG, 100, 300)[0][3].last_used == -200  # now_ms - age negative
    assert m.transitions(REG, -(1 << 63), 1)[0][3].last_used == fx.LONG_MAX  # Java long arithmetic wraps


def _numpy_inputs(m, reg):
    rows = m.rows
    listed = np.array([r is not None and not r.host and vm.in_transition(r) for r in rows])
    arow = np.array([reg.row(r.amid) if r else -1 for r in rows], np.int32)
    trow = np.array([reg.row(r.tmid) if r else -1 for r in rows], np.int32)
    failed = np.array([bool(r and r.failed) for r in rows])
    recs = np.array(reg.recs, np.int64).reshape(-1, 4)
    return listed, arow, trow, failed, recs[:, 0], recs[:, 2], np.array([reg.empty(i) for i in range(len(reg.ids))])


def _world():
    mids = fx.model_ids(300)
    vals, recs = fx.registry_values(["pod-%d" % i for i in range(8)], 300)
    return mids, vm.Registry(mids, recs)


def test_the_numpy_form_equals_the_loop():
    mids, reg = _world()
    m = vm.VModels()
    m.events(*fx.scenario(257, mids))
    for now, age in ((fx.NOW, fx.AGE), (100, 300), (-(1 << 63), 1)):
        rows, _ = m.transitions(reg, now, age)
        got = vm.transitions_numpy(*_numpy_inputs(m, reg), now, age)
        assert [tuple(int(x) for x in g) for g in got] == [tuple(t) for t in rows]


def test_corpora_are_classified_as_the_gpu_test_assumes():
    for v in fx.MALFORMED:
        assert vm.classify(v)[0] == REJECT, v
        ok = True
        try:
            ok = isinstance(json.loads(v), dict)
        except ValueError:
            ok = False
        # json.loads refuses it, or it is not an object, or it holds a known member of the wrong type
        assert not ok or any(k in v for k in ('"amid":7', '"amid":true', '"amid":[', '"amid":{', '"tmid":1.5', '"o":false', '"o":{}',
                                               '"failed":"', '"failed":1', '"failed":0', '"failed":null')), v
    for v in fx.EDGE:
        assert vm.classify(v)[0] == ACCEPT, v
        assert isinstance(json.loads(v), dict), v
    for total in range(2046, 2051):
        for by_owner in (True, False):
            assert vm.classify(fx.padded(total, by_owner))[0] == ACCEPT
    assert vm.parse(fx.template_across_chunks(5))[1] == vm.Row(b"active-model", b"target", b"owner\\\\x", True, True)


@pytest.mark.parametrize("n_vm", [63, 64, 65, 257])
def test_every_gpu_batch_holds_every_class(n_vm):
    """The scenario batches of tests/test_vmodels_gpu.py (n = 0 and 1 hold what they can: nothing, one applied event)."""
    mids, reg = _world()
    m = vm.VModels()
    keys, values, deleted = fx.scenario(n_vm, mids)
    st, idx, n_app = m.events(keys, values, deleted)
    assert {int(x) for x in st} == {0, 1, 2} and n_app == len(m.ids) > n_vm * 9 // 10
    flags = m.flags()
    for bit in (vm.F_FAILED, vm.F_ABSENT, vm.F_ACTIVE_NULL, vm.F_TARGET_NULL, vm.F_OWNER_NULL, vm.F_HOST):
        assert (flags & bit).any() and not (flags & bit).all(), bit
    ans = m.resolve_many(reg, *fx.questions(m))
    assert {a.cls for a in ans} == {vm.NOT_FOUND, vm.OK, vm.STRONG_READ, vm.TARGET_NOT_FOUND, vm.HOST}
    assert {a.which for a in ans if a.cls == vm.OK} == {vm.ACTIVE, vm.TARGET}
    assert {a.vstatus for a in ans} == {vm.DEFINED, vm.TRANSITIONING, vm.TRANSITION_FAILED}
    assert {a.target_status for a in ans} == {vm.T_NONE, vm.T_LOADING, vm.T_LOADING_FAILED, vm.T_NOT_FOUND}
    assert {a.flags for a in ans} == {0, vm.NULL_ID}
    assert any(a.cls == vm.OK and a.model < 0 and not a.flags for a in ans) and any(a.model >= 0 for a in ans)
    rows, info = m.transitions(reg, fx.NOW, fx.AGE)
    assert {t.cls for t in rows} == {vm.PROMOTE, vm.ENSURE_LOADED} and info[3] > 0
    assert {0, 1, 3} <= {t.target_count for t in rows}
    assert {t.flags for t in rows} >= {0, vm.XF_FAILED, vm.XF_FROM_EMPTY, vm.XF_TO_EMPTY}
    lus = {t.last_used for t in rows if t.cls == vm.ENSURE_LOADED}
    assert {fx.NOW - fx.AGE, 1, fx.LONG_MAX} <= lus
    assert any(t.from_model < 0 for t in rows) and any(t.to_model < 0 for t in rows)
