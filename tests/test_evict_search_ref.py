"""CPU: the linear form of tests/evict_search_ref.py against `walk`, the definition, every field of every row; and the premise of
the reference-text run of tests/test_evict_search_edges_gpu.py, counted from tests/golden/ref_clhm_edges.npz alone."""
import os

import numpy as np
import pytest

from tests import evict_search_ref as er
from tests import ref_clhm_cases as rc
from tests.evict_search_ref import T0, linear, walk
from tests.test_ref_clhm_edges_gpu import EVICT_CASES, GOLDEN, _evict_states

EDGE_CAPS = (0, -1, 2**62, -2**62, -2**63, 2**63 - 1)


def same(caches, reqs):
    n = 0
    for k, w, ts in reqs:
        if 0 <= k < len(caches) and len(caches[k][0]) <= er.WALKABLE:
            assert linear(*caches[k], w, ts) == walk(*caches[k], w, ts), (k, w, ts, caches[k][2])
            n += 1
    return n


def test_mixed_lengths():
    for label, caches, reqs, named in er.mixed_cases():
        assert same(caches, reqs) == len(reqs) - 2, label
        for i, v in named:  # (the cases are the ones named)
            assert walk(*caches[reqs[i][0]], *reqs[i][1:])[1] == v, (label, i)


def test_every_position_of_one_deque():
    caches, reqs = er.exhaustive_case()
    assert same(caches, reqs) == len(reqs) > 15 * er.EXHAUSTIVE


@pytest.mark.parametrize("name", sorted(er.defect_cases()))
def test_defects_at_the_chunk_edges(name):
    (lu, wt), ok = er.defect_cases()[name]
    assert er.searchable(lu, wt) == ok
    caches, reqs = er.defect_load(name)
    assert same(caches, reqs) == len(reqs)


@pytest.mark.parametrize("E", [17, 1025])
def test_values(E):
    caches, reqs = er.value_case(E)
    assert same(caches, reqs) == len(reqs)
    assert set(EDGE_CAPS) <= {c[2] for c in caches} and {w for _, w, _ in reqs} == {0, 3}


def test_the_default_threshold_loads():
    for lengths, unordered in (([20, 1023, 1024, 1025], ()), ([1025, 2000, 20], (0,))):
        caches, reqs = er.threshold_case(lengths, unordered)
        assert same(caches, reqs) == len(reqs)


def test_the_store_of_the_call_path_cases():
    caches = er.small_store()
    reqs = er.small_reqs(caches, 808) +[(8, 3, er.stamp_at(caches[8][0][0], p)) for p in (10, 60)]
    assert same(caches, reqs) == len(reqs) and len(set(reqs)) == len(reqs)
    assert [er.searchable(lu, wt) for lu, wt, _ in caches] == [True] * 8 + [False]


@pytest.mark.parametrize("E", [0, 1, 2, 16, 17, 18, 290, 2049])
def test_unordered_deques_zero_and_negative_weights_and_the_capacities_at_the_ends(E):
    rng = np.random.default_rng(E)
    lu = T0 + rng.integers(0, 40, E).astype(np.int64)  # unordered, with ties
    wt = rng.integers(-3, 4, E).astype(np.int32)  # zero and negative
    total = int(wt.sum())
    for w in (0, 3, -5):
        for ts in (T0 - 1, T0, T0 + 20, T0 + 39, T0 + 40, 0):
            for cap in EDGE_CAPS + (total, total + w, total + w - 1, total // 2, -total):
                assert linear(lu, wt, cap, w, ts) == walk(lu, wt, cap, w, ts), (w, ts, cap)
                assert linear(np.sort(lu), np.abs(wt), cap, w, ts) == walk(np.sort(lu), np.abs(wt), cap, w, ts), (w, ts, cap)


def test_the_recorded_inserts_of_the_reference_text_reach_the_search():
    """Conditions of the reference-text run with every deque searched, counted from the committed file: 216 recorded inserts over
    the five cases, 215 of them on a non-empty deque in time order with no negative weight (these the device must search at
    MMP_EVICT_SEARCH_FROM=0), 26 of those with victims."""
    assert os.path.getsize(GOLDEN) > 0
    vec = np.load(GOLDEN)
    inserts = searched = with_victims = 0
    for name, _ in EVICT_CASES:
        v = rc.load_edge_case(vec, name)
        rows, states = _evict_states(v)
        inserts += len(rows)
        for (c, i), (_, _, wt, lu) in zip(rows, states):
            if len(lu) and er.searchable(lu, wt) and v["ops"][i]["arg"] >= 0:
                searched += 1
                with_victims += int(v["outs"][i]["n_evicted"] > 0)
    assert (inserts, searched, with_victims) == (216, 215, 26)
