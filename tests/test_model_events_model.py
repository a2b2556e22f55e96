"""tests/model_events_model.py pinned on hand-worked cases (no GPU), and the four entry points named in the header and in
_lib.SYMBOLS."""
import os

import pytest

from modelmesh_amd import _lib
from tests.model_events_model import APPLIED, EMPTY, MALFORMED, UNKNOWN, ModelEventsModel

PODS = ["aaaaaa-1", "bbbbbb-1"]
TYPES = ["NLCLASSIFIER", "t1"]
GOOD = '{"type": "t1", "lu": 7, "lul": 3, "instanceIds": {"bbbbbb-1": 5, "gone-1": 6}}'
GOOD_REC = (1, 7, ((1, 5), (-1, 6)), ())
OTHER = '{"lu": 9, "failedIn": {"aaaaaa-1": 2}}'
OTHER_REC = (0, 9, (), ((0, 2),))
BAD = '{"lu": 5,}'


def fresh(ids=()):
    m = ModelEventsModel(PODS, TYPES, 0)
    m.recs = [EMPTY] * len(ids)
    m.load(ids)
    return m


def test_delete_put_delete_of_an_unknown_key():
    m = fresh()
    st, idx, lul, n = m.events(["K", "K", "K"], ["", GOOD, ""], [1, 0, 1])
    assert list(st) == [UNKNOWN, APPLIED, APPLIED] and list(idx) == [-1, 0, 0] and list(lul) == [0, 3, 0] and n == 1
    assert m.recs == [EMPTY] and m.ids == [b"K"]  # deleted, but still named


def test_the_same_with_append_off():
    m = fresh()
    st, idx, _, n = m.events(["K", "K", "K"], ["", GOOD, ""], [1, 0, 1], append=False)
    assert list(st) == [UNKNOWN] * 3 and list(idx) == [-1] * 3 and n == 0 and m.recs == [] and m.ids == []


def test_a_malformed_first_event_of_a_new_id_leaves_an_empty_row():
    m = fresh(["old"])
    st, idx, lul, n = m.events(["new"], [BAD])
    assert list(st) == [MALFORMED] and list(idx) == [1] and list(lul) == [0] and n == 1
    assert m.recs == [EMPTY, EMPTY] and list(m.resolve(["new", "old", "x"])) == [1, 0, -1]
    st, idx, _, n = m.events(["new"], [GOOD])  # ... which the next event fills
    assert list(st) == [APPLIED] and list(idx) == [1] and n == 0 and m.recs[1] == GOOD_REC


def test_two_new_ids_interleaved():
    m = fresh(["old"])
    st, idx, lul, n = m.events(["a", "b", "a", "old", "b"], [GOOD, OTHER, BAD, OTHER, GOOD])
    assert list(st) == [0, 0, 1, 0, 0] and list(idx) == [1, 2, 1, 0, 2] and list(lul) == [3, 0, 0, 0, 3] and n == 2
    assert m.recs == [OTHER_REC, GOOD_REC, GOOD_REC] and m.get() == [b"old", b"a", b"b"]


def test_an_id_re_added_after_a_deletion_keeps_its_row():
    m = fresh(["x", "y"])
    m.events(["y"], [GOOD])
    st, idx, _, n = m.events(["y"], [""], [1])
    assert list(st) == [APPLIED] and list(idx) == [1] and n == 0 and m.recs[1] == EMPTY
    st, idx, _, n = m.events(["y"], [OTHER])
    assert list(st) == [APPLIED] and list(idx) == [1] and n == 0 and m.recs[1] == OTHER_REC and m.n_models == 2


def test_the_empty_key_is_a_key():
    m = fresh(["x"])
    st, idx, _, n = m.events(["", "x", ""], [GOOD, OTHER, OTHER])
    assert list(st) == [0, 0, 0] and list(idx) == [1, 0, 1] and n == 1 and m.recs == [OTHER_REC, OTHER_REC]
    assert list(m.resolve([b""])) == [1] and m.get(1, 1) == [b""]


def test_a_key_with_bytes_from_0x80_on():
    k1, k2 = "modèle-é".encode(), b"\xff\x80raw"
    m = fresh([k1])
    st, idx, _, n = m.events([k2, k1, "modèle-é"], [GOOD, OTHER, GOOD])  # a str key is its UTF-8 bytes
    assert list(st) == [0, 0, 0] and list(idx) == [1, 0, 0] and n == 1 and m.get() == [k1, k2]


def test_a_key_that_is_a_prefix_of_another():
    m = fresh(["model"])
    st, idx, _, n = m.events(["model-1", "mode", "model", "model-1"], [GOOD, OTHER, GOOD, ""], [0, 0, 0, 1])
    assert list(st) == [0, 0, 0, 0] and list(idx) == [1, 2, 0, 1] and n == 2
    assert m.recs == [GOOD_REC, EMPTY, OTHER_REC] and list(m.resolve(["mod", "model-", "model-1"])) == [-1, -1, 1]


def test_load_checks_count_and_repeats():
    m = fresh(["a", "b"])
    with pytest.raises(ValueError):
        m.load(["a", "a"])
    with pytest.raises(RuntimeError):
        m.load(["a"])
    assert m.ids == [b"a", b"b"]
    with pytest.raises(RuntimeError):
        ModelEventsModel().events(["a"], [GOOD])


def test_the_four_entry_points_are_declared_and_bound():
    names = ("mmp_model_ids_load", "mmp_model_ids_resolve", "mmp_model_ids_get", "mmp_models_events_json")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmplace.h")).read()
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for name in names:
        assert name in bound, name
        assert "int %s(mmp_ctx *ctx" % name in header, name
    assert "#define MMP_MEV_APPEND 1u" in header and _lib.MEV_APPEND == 1
