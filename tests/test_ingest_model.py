"""tests/ingest_model.py — the plain-Python statement of what a stored value means to the two beans — checked by hand, and the
corpora of tests/ingest_corpus.py checked for values the parsers are not specified on.  No GPU."""
import pytest

from tests import ingest_corpus as ic
from tests import ingest_model as im
from tests.test_ingest_gpu import MALFORMED_MODELS, WELL_FORMED_MODELS
from tests.test_registry_upsert_json_gpu import parse_value

IDS = ["p%d" % i for i in range(8)]
NAMES = ["NLCLASSIFIER", "t1"]


def bean(v, unknown=0):
    return im.model_bean(v.encode() if isinstance(v, str) else v, IDS, NAMES, unknown)


def test_the_malformed_list_is_rejected():
    for v in MALFORMED_MODELS:
        assert im.model_class(v.encode()) == im.REJECT, v
        assert bean(v) == (1, None, 0, 0, [], []), v


def test_the_well_formed_list_by_hand():
    for v, (ty, nl, nf, lu) in WELL_FORMED_MODELS:
        b = bean(v)
        assert im.model_class(v.encode()) == im.ACCEPT, v
        assert (b.status, b.type, len(b.loaded), len(b.failed), b.lu) == (0, ty, nl, nf, lu), v
    by_hand = {
        '{"instanceIds":{"p1":1},"instanceIds":{"p2":2,"p3":3}}': (0, 0, 0, 0, [(2, 2), (3, 3)], []),
        '{"fails":{"p1":{"msg":"}{][","t":5}},"failedIn":{"p1":4}}': (0, 0, 0, 0, [], [(1, 4)]),
        '{"type":"t1","mPath":"a\\\\","lu":-3}': (0, 1, -3, 0, [], []),
        # the duplicate-map values of the parsers' tests: only the last occurrence of a map leaves entries
        ic.DUPLICATE_MODELS[0]: (0, 0, 0, 0, [(5, 9)], [(1, 4)]),
        ic.DUPLICATE_MODELS[1]: (0, 0, 0, 0, [(1, 4)], [(5, 9)]),
        ic.DUPLICATE_MODELS[3]: (0, 0, 0, 0, [], [(3, 3)]),
        '{"type":"nobody","lul":7,"instanceIds":{"p7":1,"p8":2,"":3,"p7":4}}': (0, 9, 0, 7, [(7, 1), (-1, 2), (-1, 3), (7, 4)], []),
        ic.five_byte_record(3).decode(): (0, 0, 0, 0, [(-1, 0), (-1, 1), (-1, 2)], []),
    }
    assert {v for v, _ in WELL_FORMED_MODELS} >= set(list(by_hand)[:3])
    for v, want in by_hand.items():
        assert bean(v, unknown=9) == want, v
    assert bean('{"lu":1}', unknown=5).type == 0 and im.model_bean(b'{"lu":1}', IDS, ["t0"], 5).type == 5  # no NLCLASSIFIER loaded


def test_integer_extremes():
    lo64, hi64, lo32, hi32 = -9223372036854775808, 9223372036854775807, -2147483648, 2147483647
    assert bean('{"lu":-9223372036854775808,"lul":9223372036854775807}')[:4] == (0, 0, lo64, hi64)
    assert bean('{"lu":2147483647,"lul":-2147483648}')[:4] == (0, 0, hi32, lo32)
    assert bean('{"instanceIds":{"p1":-9223372036854775808},"failedIn":{"p2":9223372036854775807}}')[4:] == ([(1, lo64)], [(2, hi64)])
    assert im.pod_bean(b'{"count":2147483647,"rpm":-2147483648,"cap":9223372036854775807,"lruTime":-9223372036854775808}') == \
        (0, (lo64, hi32, hi64, 0, 0, 0, lo32, False, 0, 0))
    assert im.pod_bean(b'{"shutdown":true,"startTime":5,"vers":6,"lThreads":1,"lInProg":2,"used":3}') == \
        (0, (0, 0, 0, 3, 1, 2, 0, True, 5, 6))
    # one past an extreme is not specified (the parsers wrap, Jackson refuses), and neither is the int range on a long
    for v in ('{"lu":9223372036854775808}', '{"lul":-9223372036854775809}', '{"failedIn":{"p1":9223372036854775808}}'):
        assert im.model_class(v.encode()) == im.UNSPECIFIED, v
    for v in ('{"count":2147483648}', '{"rpm":-2147483649}', '{"cap":9223372036854775808}'):
        assert im.pod_class(v.encode()) == im.UNSPECIFIED, v
    assert im.pod_class(b'{"cap":2147483648}') == im.ACCEPT


def test_the_three_classes():
    unspecified = ['{"x": 1 2}', '{"x": [1,2}}', '{"x": tru}', '{"lu": 05}', '{"lu": -007, "x": 1}', '{"type": 5}', '{"type": {}}',
                   '{"l\\u0075": 5}', '{"type": "t\\u0031"}', '{"instanceIds": {"p\\u0031": 5}}', '{"x": "\\q"}', '{"x": NaN}']
    for v in unspecified:
        assert im.model_class(v.encode()) == im.UNSPECIFIED, v
        with pytest.raises(ValueError):
            bean(v)
    reject = ['{"lu": 5}x', '{"lu": 5}\n}', 'x{"lu": 5}', '{"lu": null}', '{"lu": true}', '{"lu": 5 2}', '{"lu": 05 2}',
              '{"lu": NaN}', '{"instanceIds": {"p1": null}}', '{"instanceIds": {"p1": true}}', '{"instanceIds": "x"}', '{,}',
              '{"x": 1,}', '{"x" 1}', '{"x": [1, 2}', '{"x": "a}', '{"lu": 5}' + " " * 3000 + "}", ic.overclaiming_record(40).decode(),
              '{"x": 1 2, "lu": }']
    for v in reject:
        assert im.model_class(v.encode()) == im.REJECT, v
    accept = ['{"x": "\\u00e9\\n\\"", "lu": 5}', ' \t\r\n{"lu": 5}\n', '{"type": "unheard-of"}', '{"x": 1.5e3, "y": [null, true]}']
    for v in accept:
        assert im.model_class(v.encode()) == im.ACCEPT, v
    assert im.model_class('{"x": "é"}'.encode()[:-3]) == im.REJECT  # cut inside a character: truncated all the same
    assert [im.pod_class(v.encode()) for v in ic.POD_VALUES] == \
        [im.ACCEPT, im.REJECT, im.REJECT, im.REJECT, im.ACCEPT, im.REJECT, im.ACCEPT, im.ACCEPT, im.REJECT, im.REJECT, im.REJECT]


def test_no_corpus_holds_an_unspecified_value():
    """Every builder, every form: no value of the UNSPECIFIED class, the forms of a value are of its class, and the strict
    prefixes are all rejected.  The corpora hold both other classes."""
    for corpus, cls_of in ((ic.model_corpus(), im.model_class), (ic.pod_corpus(), im.pod_class)):
        seen = set()
        for v in corpus:
            c = cls_of(v)
            assert c != im.UNSPECIFIED, v
            seen.add(c)
            for w in ic.forms(v, c):
                assert cls_of(w) == c, (v, w[:40])
                assert len(w) > ic.TILE or w is v
        assert seen == {im.ACCEPT, im.REJECT}
    assert all(im.model_class(v) == im.REJECT for v in ic.model_corpus()[-100:])
    assert all(im.pod_class(v) == im.REJECT for v in ic.pod_corpus()[-40:])
    for v in ic.planted_models(4096) + ic.chunk_edge_models() + ic.tile_edge_models()[0]:
        assert im.model_class(v) != im.UNSPECIFIED, v[:80]
    for v in ic.planted_pods(4096) + ic.chunk_edge_pods():
        assert im.pod_class(v) != im.UNSPECIFIED, v[:80]
    assert im.model_class(ic.five_byte_record(40)) == im.ACCEPT and im.model_class(ic.overclaiming_record(40)) == im.REJECT


def test_the_upsert_tests_own_parser_agrees_on_the_corpus():
    """tests/test_registry_upsert_json_gpu.py derives what its twin registry receives with parse_value; on this corpus it says
    what the reference says, so its twin-context checks are checks against the reference.  (It reads a dict, so it cannot see an
    EARLIER duplicate of the wrong type: the two such values are left out of the event run and named here.)"""
    default = ic.TYPE_NAMES.index("NLCLASSIFIER")
    type_of = {s: i for i, s in enumerate(ic.TYPE_NAMES)}
    assert all(im.model_class(v) == im.REJECT and parse_value(v, ic.POD_OF, type_of, ic.UNKNOWN_TYPE, default) for v in ic.TWIN_BLIND)
    for v in ic.model_corpus():
        if v in ic.TWIN_BLIND:
            continue
        for w in ic.forms(v, im.model_class(v)):
            a, p = ic.model_answer(v), parse_value(w, ic.POD_OF, type_of, ic.UNKNOWN_TYPE, default)
            if a.status:
                assert p is None, v
            else:
                assert p == ((a.type, a.lu, tuple(a.loaded), tuple(a.failed)), a.lul), v
