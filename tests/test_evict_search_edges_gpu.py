"""GPU: the prefix scan and the search of evict_tree_kernels.hpp at their edges, every field of every row exact against the linear
form of tests/evict_search_ref.py (held to the walk in tests/test_evict_search_ref.py), and n_above / n_searchable / rows_searched
of every load and batch against what the inputs say.  What tests/test_evict_search_gpu.py leaves out: caches of different lengths
and empty caches in one table, four and five search steps, a cache of more than 256 chunks, a defect at a chunk edge and a
negative stored weight, zero weights and the capacities at the ends of int64, the staged call path and the counter's ring, the
default threshold with caches on both sides of it, and the reference's own recorded inserts with every deque searched."""
import threading

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd.solver import Solver
from tests import evict_search_ref as er
from tests import ref_clhm_cases as rc
from tests import test_ref_clhm_edges_gpu as edges
from tests.evict_search_ref import NOW
from tests.test_evict_search_gpu import FIELDS, walk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vec():
    return np.load(edges.GOLDEN)


@pytest.fixture
def solver(monkeypatch):
    monkeypatch.setenv("MMP_EVICT_SEARCH_FROM", "0")
    s = Solver(100, 1000)
    yield s
    s.close()


def load(s, caches):
    s.load_caches(np.cumsum([0] + [len(c[0]) for c in caches]), np.concatenate([c[0] for c in caches] + [np.zeros(0, np.int64)]),
                  np.concatenate([c[1] for c in caches] + [np.zeros(0, np.int32)]), [c[2] for c in caches])


def ask(s, reqs, want):
    """one batch, every field of every row against `want`; -> the rows"""
    got = s.evict(np.array(reqs, dtype=_lib.EVICT_REQ), NOW)
    have = np.stack([got[f].astype(np.int64) for f in FIELDS], axis=1)
    bad = np.nonzero((have != np.array(want, dtype=np.int64).reshape(len(reqs), len(FIELDS))).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), [(int(i), reqs[i], tuple(have[i]), want[i]) for i in bad[:5]])
    return got


def run(s, caches, reqs, search_from=0, want=None):
    """load, one batch against the reference, and the three counts against the inputs; -> (rows, info)"""
    load(s, caches)
    got = ask(s, reqs, er.reference(caches, reqs) if want is None else want)
    info = s.evict_search_info()
    assert (info["n_above"], info["n_searchable"], info["rows_searched"]) == er.expected_info(caches, reqs, search_from), info
    return got, info


# ---- the reference text through the search --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,team", edges.EVICT_CASES)
def test_the_reference_text_with_every_deque_searched(vec, solver, name, team):
    """The five cases of test_stateless_eviction_equals_the_reference_text_at_the_edges, the same rows and comparisons, in a
    context that searches every non-empty deque: 215 of the 216 recorded inserts (tests/test_evict_search_ref.py counts them)."""
    rows, states = edges._check_evict_case(vec, solver, name, team)
    v = rc.load_edge_case(vec, name)
    ok = [len(lu) > 0 and er.searchable(lu, wt) for _, _, wt, lu in states]
    info = solver.evict_search_info()
    assert (info["search_from"], info["n_above"], info["n_searchable"]) == (0, sum(len(lu) > 0 for _, _, _, lu in states), sum(ok))
    assert info["rows_searched"] == sum(1 for (_, i), k in zip(rows, ok) if k and v["ops"][i]["arg"] >= 0) > 0


# ---- a. mixed lengths -----------------------------------------------------------------------------------------------------------
def test_caches_of_different_lengths_and_empty_caches_in_one_load(solver):
    for label, caches, reqs, named in er.mixed_cases():
        got, info = run(solver, caches, reqs)
        assert (info["n_above"], info["n_searchable"]) == (6, 6), label
        assert [int(got[i]["n_victims"]) for i, _ in named] == [v for _, v in named], label  # (the cases are the ones named)
        none = [i for i, r in enumerate(reqs) if not 0 <= r[0] < len(caches)]
        assert len(none) == 2 and all(tuple(int(got[i][f]) for f in FIELDS) == (0, 0, 0, 0, -1) for i in none), label


# ---- b. search depth ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", er.DEPTH_LENGTHS)
def test_three_four_and_five_search_steps(solver, E):
    caches, reqs, victims = er.depth_case(E)
    got, info = run(solver, caches, reqs)
    assert info["rows_searched"] == len(reqs) > 2048 and np.array_equal(got["n_victims"], victims)


def test_every_position_of_one_deque(solver):
    caches, reqs = er.exhaustive_case()
    _, info = run(solver, caches, reqs)
    assert info["rows_searched"] == len(reqs) > 15 * er.EXHAUSTIVE


# ---- c. more than 256 chunks --------------------------------------------------------------------------------------------------
def test_a_cache_of_more_than_256_chunks(solver):
    """256, 257 and 258 chunks in one load, every weight 2^31 - 1.  The carry of a chunk sums the chunk totals to its left 256 a
    trip: the second trip runs from the cache's 258th chunk on, the "in order" pass over all chunks from its 257th."""
    for k, caches, reqs in er.wide_cases():
        got, info = run(solver, caches, reqs)
        assert (info["n_searchable"], info["rows_searched"]) == (3, len(reqs)), k
        last = [E + 1 - k for E in er.WIDE_LENGTHS]  # E + 1 entries of one weight, k of them fit
        assert [int(g["n_victims"]) for g in got] == [last[c] for c, _, _ in reqs], k


# ---- d. unsearchable caches ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(er.defect_cases()))
def test_one_defect_at_a_chunk_edge(solver, name):
    caches, reqs = er.defect_load(name)
    stays = er.defect_cases()[name][1]
    want = [walk(*caches[k], w, ts) for k, w, ts in reqs]  # the walk itself: the defective cache must take it
    _, info = run(solver, caches, reqs, want=want)
    assert (info["n_above"], info["n_searchable"]) == (6, 6 if stays else 3)
    assert info["rows_searched"] == (len(reqs) if stays else len(reqs) // 2)


# ---- e. values ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [17, 1025])
def test_zero_weights_and_the_capacities_at_the_ends(solver, E):
    caches, reqs = er.value_case(E)
    assert set(er.NAMED_CAPS) <= {c[2] for c in caches}
    _, info = run(solver, caches, reqs)
    assert info["rows_searched"] == len(reqs)


# ---- f. call paths and the counter --------------------------------------------------------------------------------------------
def test_the_counter_over_more_calls_than_its_ring_has_slots(solver):
    caches = er.small_store()
    load(solver, caches)
    pool = er.small_reqs(caches, 7) + [(8, 3, er.stamp_at(caches[8][0][0], p)) for p in (10, 60)]
    want = er.reference(caches, pool)

    def call(i):
        rows = list(range(i % 7 + 1)) + [7, 8]  # i % 7 + 1 searched, 2 on the unordered cache
        ask(solver, [pool[j] for j in rows], [want[j] for j in rows])
    for i in range(40):
        call(i)
        assert solver.evict_search_info()["rows_searched"] == i % 7 + 1, i
    for i in range(40, 60):
        call(i)
    assert solver.evict_search_info()["rows_searched"] == 59 % 7 + 1


@pytest.mark.parametrize("n", [2048, 2049, 20000])
def test_batches_on_either_side_of_the_latency_slots(solver, n):
    caches = er.small_store()
    reqs = er.small_reqs(caches, n)
    _, info = run(solver, caches, reqs)
    assert (info["n_above"], info["n_searchable"], info["rows_searched"]) == (9, 8, n)


def test_four_threads_on_one_context(solver):
    caches = er.small_store()
    load(solver, caches)
    reqs = [er.small_reqs(caches, 64, 200 * t) for t in range(4)]
    want = [er.reference(caches, r) for r in reqs]
    failed = []

    def work(t):
        try:
            for _ in range(50):
                ask(solver, reqs[t], want[t])
        except BaseException as e:  # (an assertion in a thread reaches nobody)
            failed.append((t, e))
    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not failed, failed[:1]  # (no count is read here: which call was the last one is not defined)


# ---- g. default threshold and reloads -------------------------------------------------------------------------------------------
def test_the_default_threshold_and_what_a_reload_leaves(monkeypatch):
    monkeypatch.delenv("MMP_EVICT_SEARCH_FROM", raising=False)
    s = Solver(100, 1000)

    def step(lengths, unordered=()):
        return run(s, *er.threshold_case(lengths, unordered), search_from=1024)[1]
    try:
        info = step([20, 1023, 1024, 1025])
        assert (info["search_from"], info["n_above"], info["rows_searched"], info["generation"]) == (1024, 1, 4, 1)
        info = step([20, 1023, 1024])
        assert (info["n_above"], info["rows_searched"], info["generation"]) == (0, 0, 1)
        info = step([1025, 2000, 20])
        assert (info["n_above"], info["n_searchable"], info["rows_searched"], info["generation"]) == (2, 2, 8, 2)
        info = step([1025, 2000, 20], unordered=(0,))
        assert (info["n_above"], info["n_searchable"], info["rows_searched"], info["generation"]) == (2, 1, 4, 3)
        for gen, lengths in enumerate(([5000], [1025, 1025, 1025, 3000, 10], [1100], [1025, 2000, 20]), 4):
            info = step(lengths)
            assert (info["n_searchable"], info["generation"]) == (sum(E > 1024 for E in lengths), gen)
    finally:
        s.close()
