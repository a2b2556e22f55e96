"""tests/pod_retire_model.py on hand-worked cases (no GPU): the remap, the ranks of the survivors, the kept interning, the squeezed
label / type / missing lists, the rewritten records and the count, the two guards on both sides, a retired id that rejoins."""
import copy

import numpy as np
import pytest

from modelmesh_amd._lib import POD_LIVE, POD_TOMBSTONE
from tests.pod_events_model import APPLIED, UNKNOWN, PodEventsModel
from tests.pod_retire_model import PodRetireState, retire

IDS = [b"rsaaaa-00003", b"rsbbbb-00001", b"p4", b"rsaaaa-00001", b"rsbbbb-00002", b"rscccc-00009"]
VALUE = '{"lruTime":5,"cap":100,"used":10,"count":1}'


def fleet(ids=IDS):
    st = PodRetireState()
    st.pods.load(list(ids))
    n = len(ids)
    st.pods.rows["flags"] = POD_LIVE
    st.pods.rows["capacity"] = 100 + np.arange(n)  # a row can be told from its neighbours
    st.label_words, st.label_counts = [1 << p for p in range(n)], [p + 1 for p in range(n)]
    st.allowed, st.prefer = [[p % 2 for p in range(n)], [1] * n], [[(p // 2) % 2 for p in range(n)], [0] * n]
    st.missing = [1000 + p if p % 2 else 0 for p in range(n)]
    return st


def snapshot(st):
    m = st.pods
    return copy.deepcopy((m.ids, m.index, m.rows.tobytes(), m._intern, st.label_words, st.label_counts, st.allowed, st.prefer, st.missing,
                          st.records))


def test_ranks_and_replica_sets_of_the_start():
    st = fleet()
    # bytes order: p4 < rsaaaa-00001 < rsaaaa-00003 < rsbbbb-00001 < rsbbbb-00002 < rscccc-00009
    assert list(st.pods.rows["id_order"]) == [2, 3, 0, 1, 4, 5]
    assert list(st.pods.rows["replica_set"]) == [0, 1, -1, 0, 1, 2]


@pytest.mark.parametrize("pods,remap", [
    ([], [0, 1, 2, 3, 4, 5]),
    ([0], [-1, 0, 1, 2, 3, 4]),
    ([5], [0, 1, 2, 3, 4, -1]),
    ([0, 1, 2, 3, 4, 5], [-1] * 6),
    ([5, 0, 1, 2, 4], [-1, -1, -1, 0, -1, -1]),
    ([3, 1, 3, 3], [0, -1, 1, -1, 2, 3]),  # named twice (and more): retired once
])
def test_remap_and_squeezed_lists(pods, remap):
    st = fleet()
    before = fleet()
    got, count = retire(st, pods)
    assert got.dtype == np.int32 and list(got) == remap and count == 0
    keep = [p for p in range(6) if remap[p] >= 0]
    assert st.pods.n_pods == len(keep) and st.pods.ids == [IDS[p] for p in keep]
    assert st.pods.index == {IDS[p]: remap[p] for p in keep}
    assert list(st.pods.rows["capacity"]) == [100 + p for p in keep]
    assert st.label_words == [1 << p for p in keep] and st.label_counts == [p + 1 for p in keep]
    assert st.allowed == [[p % 2 for p in keep], [1] * len(keep)] and st.prefer == [[(p // 2) % 2 for p in keep], [0] * len(keep)]
    assert st.missing == [before.missing[p] for p in keep]
    assert list(st.pods.rows["replica_set"]) == [before.pods.rows["replica_set"][p] for p in keep]  # nothing renumbered
    want_rank = {p: r for r, p in enumerate(sorted(keep, key=lambda p: IDS[p]))}
    assert list(st.pods.rows["id_order"]) == [want_rank[p] for p in keep]


@pytest.mark.parametrize("gone,ranks", [
    (2, [1, 2, 0, 3, 4]),   # the lowest id (p4) leaves: everyone moves down one
    (0, [2, 0, 1, 3, 4]),   # a middle id (rsaaaa-00003, rank 2): the ranks above it move down
    (5, [2, 3, 0, 1, 4]),   # the highest id leaves: no rank changes
])
def test_ranks_after_the_lowest_a_middle_and_the_highest_id_leave(gone, ranks):
    st = fleet()
    retire(st, [gone])
    assert list(st.pods.rows["id_order"]) == ranks


def test_the_type_word_count_drops_at_65_64_63():
    ids = [b"rsaaaa-%05d" % i for i in range(65)]
    st = fleet(ids)
    words = lambda: (st.pods.n_pods + 63) // 64  # noqa: E731
    assert words() == 2 and len(st.allowed[0]) == 65
    retire(st, [64])
    assert words() == 1 and len(st.allowed[0]) == 64 and st.allowed[0] == [p % 2 for p in range(64)]
    retire(st, [0])
    assert words() == 1 and len(st.allowed[0]) == 63 and st.allowed[0] == [p % 2 for p in range(1, 64)]
    assert st.missing == [1000 + p if p % 2 else 0 for p in range(1, 64)]


def records():
    # instance 1 is retired.  only / first / middle / last entry on it; beside an unresolved entry (-1) and one >= P0 (9); a failed one
    return [([[1, 10]], []),
            ([[1, 11], [0, 12], [3, 13]], []),
            ([[0, 14], [1, 15], [3, 16]], []),
            ([[0, 17], [3, 18], [1, 19]], []),
            ([[-1, 20], [1, 21], [9, 22]], []),
            ([[4, 23]], [[1, 24]]),
            ([], []),
            ([[5, 25], [2, 26]], [[0, 27]])]


def test_records_are_rewritten_where_they_stand():
    st = fleet()
    st.records = records()
    assert st.n_unresolved() == 2
    remap, count = retire(st, [1])
    assert list(remap) == [0, -1, 1, 2, 3, 4] and count == 6
    assert st.records == [([[-1, 10]], []),
                          ([[-1, 11], [0, 12], [2, 13]], []),
                          ([[0, 14], [-1, 15], [2, 16]], []),
                          ([[0, 17], [2, 18], [-1, 19]], []),
                          ([[-1, 20], [-1, 21], [9, 22]], []),  # 9 stays 9, although the table now has 5 rows
                          ([[3, 23]], [[-1, 24]]),
                          ([], []),
                          ([[4, 25], [1, 26]], [[0, 27]])]
    assert st.n_unresolved() == 2 + count


def test_gone_only_on_both_sides():
    st = fleet()
    st.pods.events([IDS[1], IDS[4]], ["", ""], deleted=[1, 1])
    before = snapshot(st)
    with pytest.raises(ValueError, match="instance 3 is not"):
        retire(st, [4, 5, 3, 1], gone_only=True)  # 3 and 5 are live: the lowest is named
    assert snapshot(st) == before
    st.pods.rows["flags"][4] |= POD_LIVE  # a tombstone flag beside a live one is no tombstone
    with pytest.raises(ValueError, match="instance 4 is not"):
        retire(st, [4, 1], gone_only=True)
    st.pods.rows["flags"][4] &= ~np.uint32(POD_LIVE)
    remap, _ = retire(st, [4, 1], gone_only=True)
    assert list(remap) == [0, -1, 1, 2, -1, 3]
    assert not (st.pods.rows["flags"] & POD_TOMBSTONE).any()


def test_unreferenced_on_both_sides():
    st = fleet()
    st.records = records()
    before = snapshot(st)
    with pytest.raises(ValueError, match="instance 1 is still"):
        retire(st, [4, 1], unreferenced=True)  # 4 is loaded in record 5, 1 all over: the lowest
    with pytest.raises(ValueError, match="instance 0 is still"):
        retire(st, [0], unreferenced=True)  # a failed entry counts (record 7)
    assert snapshot(st) == before
    st.records = [r for r in st.records if all(e[0] not in (1, 4) for e in r[0] + r[1])]
    remap, count = retire(st, [4, 1], unreferenced=True)
    assert count == 0 and list(remap) == [0, -1, 1, 2, -1, 3]
    assert st.records == [([], []), ([[3, 25], [1, 26]], [[0, 27]])]


def test_refusals_change_nothing():
    st = fleet()
    st.records = records()
    before = snapshot(st)
    for bad in ([6], [-1], [0, 1, 7]):
        with pytest.raises(ValueError):
            retire(st, bad)
    st.pods.rows = st.pods.rows[:5]  # resized by index behind the id store's back
    with pytest.raises(RuntimeError):
        retire(st, [0])
    st.pods.rows = np.frombuffer(before[2], st.pods.rows.dtype).copy()
    assert snapshot(st) == before


def test_a_retired_id_rejoins_at_the_end_and_keeps_its_replica_set():
    st = fleet()
    m = st.pods
    retire(st, [5, 1])  # rscccc (number 2, its only member) and one of rsbbbb
    status, idx, _, n_app = m.events([IDS[5], IDS[1]], [VALUE, VALUE], append=False)
    assert list(status) == [UNKNOWN, UNKNOWN] and list(idx) == [-1, -1] and n_app == 0 and m.n_pods == 4
    status, idx, _, n_app = m.events([IDS[5], b"rsdddd-00001", IDS[1]], [VALUE] * 3)
    assert list(status) == [APPLIED] * 3 and list(idx) == [4, 5, 6] and n_app == 3
    assert list(m.rows["replica_set"]) == [0, -1, 0, 1, 2, 3, 1]  # rscccc is 2 again, the new prefix gets the next number
    order = sorted(range(7), key=lambda i: m.ids[i])
    assert [int(m.rows["id_order"][i]) for i in order] == list(range(7))


def test_without_ids_the_rows_keep_their_id_order():
    st = PodRetireState(PodEventsModel())
    st.pods.rows = np.zeros(4, st.pods.rows.dtype)
    st.pods.rows["id_order"] = [7, 3, 9, 1]
    remap, _ = retire(st, [1])
    assert list(remap) == [0, -1, 1, 2] and list(st.pods.rows["id_order"]) == [7, 9, 1]
