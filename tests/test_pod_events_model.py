"""tests/pod_events_model.py on cases worked by hand: the model is the oracle of mmp_pod_ids_append / mmp_pods_events_json, so
its own rules are pinned here without a device."""
import numpy as np
import pytest

from modelmesh_amd._lib import POD_LIVE, POD_SHUTTING_DOWN, POD_TOMBSTONE
from tests.pod_events_model import APPLIED, MALFORMED, UNKNOWN, PodEventsModel

GOOD = '{"count": 3, "cap": 100, "used": 40, "lruTime": 77, "startTime": 1234, "vers": 9}'
GOOD2 = '{"count": 5, "cap": 200, "startTime": 99, "shutdown": true}'
BAD = '{"count": 3, "cap": '


def _model(ids=("bbbbbb-1", "dddddd-1")):
    m = PodEventsModel()
    m.load(list(ids))
    return m


def test_unknown_id_with_and_without_the_flag():
    m = _model()
    st, idx, start, n = m.events(["cccccc-1"], [GOOD], append=False)
    assert (list(st), list(idx), list(start), n) == ([UNKNOWN], [-1], [0], 0) and m.n_pods == 2
    st, idx, start, n = m.events(["cccccc-1"], [GOOD], append=True)
    assert (list(st), list(idx), list(start), n) == ([APPLIED], [2], [1234], 1) and m.n_pods == 3
    r = m.rows[2]
    assert (r["count"], r["capacity"], r["used"], r["lru_time"], r["version"], r["flags"]) == (3, 100, 40, 77, 9, POD_LIVE)
    assert list(m.rows["id_order"]) == [0, 2, 1] and list(m.rows["replica_set"]) == [0, 1, 2]


def test_deletion_of_an_unknown_id_never_appends():
    m = _model()
    for flag in (False, True):
        st, idx, _, n = m.events(["zzzzzz-9"], [""], deleted=[1], append=flag)
        assert (list(st), list(idx), n) == ([UNKNOWN], [-1], 0) and m.n_pods == 2
    # ... also when the same call makes the id join LATER: the deletion came first
    st, idx, _, n = m.events(["zzzzzz-9", "zzzzzz-9", "zzzzzz-9"], ["", GOOD, ""], deleted=[1, 0, 1])
    assert (list(st), list(idx), n) == ([UNKNOWN, APPLIED, APPLIED], [-1, 2, 2], 1)
    assert m.rows["flags"][2] == POD_TOMBSTONE and m.rows["count"][2] == 3


def test_the_same_new_id_twice_in_one_call():
    m = _model()
    st, idx, start, n = m.events(["aaaaaa-1", "aaaaaa-1"], [BAD, GOOD])  # malformed, then good
    assert (list(st), list(idx), list(start), n) == ([MALFORMED, APPLIED], [2, 2], [0, 1234], 1)
    assert m.rows["flags"][2] == POD_LIVE and m.rows["count"][2] == 3
    st, idx, start, n = m.events(["aaaaaa-2", "aaaaaa-2"], [GOOD, ""], deleted=[0, 1])  # good, then deleted
    assert (list(st), list(idx), list(start), n) == ([APPLIED, APPLIED], [3, 3], [1234, 0], 1)
    assert m.rows["flags"][3] == POD_TOMBSTONE and m.rows["count"][3] == 3  # the row keeps what the good event wrote
    # a join whose only value is malformed: the index is handed out, the row stays a tombstone
    st, idx, _, n = m.events(["aaaaaa-3"], [BAD])
    assert (list(st), list(idx), n) == ([MALFORMED], [4], 1)
    assert m.rows["flags"][4] == POD_TOMBSTONE and m.rows["count"][4] == 0 and m.rows["replica_set"][4] == 2


def test_a_known_pod_deleted_then_added_again_in_one_call():
    m = _model()
    m.events(["bbbbbb-1"], [GOOD])
    st, idx, start, n = m.events(["bbbbbb-1", "bbbbbb-1"], ["", GOOD2], deleted=[1, 0], live=[1, 0])
    assert (list(st), list(idx), list(start), n) == ([APPLIED, APPLIED], [0, 0], [0, 99], 0)
    r = m.rows[0]
    assert (r["count"], r["capacity"], r["used"], r["lru_time"], r["flags"]) == (5, 200, 0, 0, POD_SHUTTING_DOWN)  # not live, no tombstone


def test_rank_of_a_new_id_first_last_middle_and_prefix():
    m = _model(["bbbbbb-1", "dddddd-1"])
    io, rs = m.append(["aaaaaa-1"])  # sorts first
    assert list(io) == [1, 2, 0] and list(rs) == [0, 1, 2]
    io, rs = m.append(["eeeeee-1"])  # last
    assert list(io) == [1, 2, 0, 3] and list(rs) == [0, 1, 2, 3]
    io, rs = m.append(["cccccc-1"])  # middle
    assert list(io) == [1, 3, 0, 4, 2] and list(rs) == [0, 1, 2, 3, 4]
    io, rs = m.append(["bbbbbb-"])  # a prefix of an existing id: in front of it, and of its replica set
    assert list(io) == [2, 4, 0, 5, 3, 1] and list(rs) == [0, 1, 2, 3, 4, 0]
    io, rs = m.append(["bbbbbb-10", "B"])  # behind the id it extends; upper case sorts in front of lower case (bytes)
    assert list(io) == [3, 6, 1, 7, 5, 2, 4, 0] and list(rs) == [0, 1, 2, 3, 4, 0, 0, -1]


def test_ids_of_length_0_6_and_7():
    m = PodEventsModel()
    io, rs = m.load(["abcdefg", "", "abcdef"])
    assert list(io) == [2, 0, 1] and list(rs) == [0, -1, -1]  # |id| < 7: no replica set; "" sorts first
    io, rs = m.append(["abcdefh", "abcde"])
    assert list(io) == [3, 0, 2, 4, 1] and list(rs) == [0, -1, -1, 0, -1]
    st, idx, _, n = m.events(["", "abcdef", "abcdefg"], [GOOD, GOOD, GOOD])
    assert (list(st), list(idx), n) == ([APPLIED] * 3, [1, 2, 0], 0)


def test_refusals_change_nothing():
    m = PodEventsModel()
    with pytest.raises(RuntimeError):
        m.append(["x"])
    with pytest.raises(RuntimeError):
        m.events(["x"], [GOOD])
    m.load([])  # a load of no ids is a valid start
    m.append(["aaaaaa-1", "aaaaaa-2"])
    before = m.rows.copy()
    for dup in (["aaaaaa-1"], ["cccccc-1", "cccccc-1"], ["cccccc-1", "bbbbbb-1", "cccccc-1"]):
        with pytest.raises(ValueError):
            m.append(dup)
        assert np.array_equal(m.rows, before) and len(m.ids) == 2 and len(m.index) == 2
    assert m.append([])[0].tolist() == [0, 1]


def test_a_load_keeps_the_rows_it_finds_and_renumbers_them():
    m = _model(["bbbbbb-1", "dddddd-1"])
    m.events(["dddddd-1"], [GOOD])
    m.load(["dddddd-2", "aaaaaa-1", "cccccc-1"])
    assert list(m.rows["count"]) == [0, 3, 0] and list(m.rows["id_order"]) == [2, 0, 1] and list(m.rows["replica_set"]) == [0, 1, 2]
    assert list(m.rows["flags"]) == [POD_TOMBSTONE, POD_LIVE, POD_TOMBSTONE]
