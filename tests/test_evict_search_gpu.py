"""GPU: mmp_evict_batch by search over prefix weights (evict_tree_kernels.hpp) against a plain walk in Python integers, every
field of every row exact.  MMP_EVICT_SEARCH_FROM=0 sends the shortest deques to the search; the lengths sit on the edges of the
search (TEAM = 16 lanes, 17-fold narrowing) and of the scan (chunks of 1 024 entries).

Case 5 reloads: mmp_cache_replay writes the STATEFUL store (mmp_caches_load_keyed), which mmp_evict_batch never read; the store it
reads has one writer, mmp_caches_load.  The replayed deque, read back with mmp_cache_read, reaches it through that call, and the
table must follow it there."""
import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd.solver import Solver

pytestmark = pytest.mark.gpu
NOW, T0 = 1_760_000_000_000, 1_700_000_000_000
TEAM, CHUNK = 16, 1024
LENGTHS = [0, 1, 2, TEAM - 1, TEAM, TEAM + 1, (TEAM + 1) ** 2 - 1, (TEAM + 1) ** 2, (TEAM + 1) ** 2 + 1, CHUNK - 1, CHUNK, CHUNK + 1,
           2 * CHUNK + 1]
FIELDS = ("insert_pos", "n_victims", "self_evicted", "weighted_size", "oldest_time")


def walk(lu, wt, cap, w, ts):
    """clhm insert + evict on one deque: (insert_pos, n_victims, self_evicted, weighted_size, oldest_time)"""
    ts = ts or NOW
    pos = len(lu)
    while pos > 0 and lu[pos - 1] > ts:  # from the tail to the first lastUsed <= ts
        pos -= 1
    dq = [(int(t), int(x)) for t, x in zip(lu, wt)]
    dq.insert(pos, (int(ts), int(w)))
    size, head = sum(x for _, x in dq), 0
    while size > cap and head < len(dq):  # poll the head while weightedSize > capacity
        size -= dq[head][1]
        head += 1
    return pos, head, int(head > pos), size, dq[head][0] if head < len(dq) else -1


def deque_of(E):
    """E entries in time order, weights 1 .. 5; runs of four equal stamps across the first splitter of the search and the chunk edge"""
    lu = T0 + 10 * np.arange(E, dtype=np.int64)
    for a in runs(E):
        lu[a:a + 4] = lu[a]
    return lu, (1 + (7 * np.arange(E)) % 5).astype(np.int32)


def runs(E):
    """where deque_of's runs start: the first step's first probe is entry s - 1, s = E // 17 + 1; a chunk ends at 1 023"""
    return [a for a in (max(E // (TEAM + 1) - 2, 0), CHUNK - 2) if a < E]


def check(s, caches, reqs, searched=None):
    """load `caches` = [(lu, wt, cap)], send reqs = [(cache, weight, ts)] as one batch, compare with the walk; returns the info"""
    s.load_caches(np.cumsum([0] + [len(c[0]) for c in caches]), np.concatenate([c[0] for c in caches] + [np.zeros(0, np.int64)]),
                  np.concatenate([c[1] for c in caches] + [np.zeros(0, np.int32)]), [c[2] for c in caches])
    got = s.evict(np.array(reqs, dtype=_lib.EVICT_REQ), NOW)
    for i, (k, w, ts) in enumerate(reqs):
        assert tuple(int(got[i][f]) for f in FIELDS) == walk(*caches[k], w, ts), (i, k, w, ts)
    info = s.evict_search_info()
    assert info["rows_searched"] == (len(reqs) if searched is None else searched)
    return info


@pytest.fixture
def solver(monkeypatch):
    monkeypatch.setenv("MMP_EVICT_SEARCH_FROM", "0")
    s = Solver(100, 1000)
    yield s
    s.close()


@pytest.mark.parametrize("E", LENGTHS)
def test_lengths_and_stamps(solver, E):
    lu, wt = deque_of(E)
    caches = [(lu, wt, int(wt.sum()) // 2), (lu, wt, int(wt.sum()) + 100)]
    stamps = [T0 - 5, T0 + 10 * (E // 2) + 5, T0 + 10 * E + 5, 0] + [int(lu[a]) for a in runs(E)]
    check(solver, caches, [(k, 3, ts) for k in (0, 1) for ts in stamps], searched=None if E else 0)  # (no entries: nothing to search)


@pytest.mark.parametrize("E", LENGTHS)
def test_victim_counts_and_the_capacities_beside_them(solver, E):
    lu, wt = T0 + 10 * np.arange(E, dtype=np.int64), deque_of(E)[1]
    pos, w = E // 2, 3
    ts = T0 + 10 * pos - 5
    merged = [int(x) for x in wt[:pos]] + [w] + [int(x) for x in wt[pos:]]
    counts = sorted({0, 1, pos, pos + 1, E + 1})
    caps = [sum(merged[v:]) + d for v in counts for d in (0, -1, 1)]  # `v` victims leave exactly sum(merged[v:])
    check(solver, [(lu, wt, cap) for cap in caps], [(k, w, ts) for k in range(len(caps))], searched=None if E else 0)
    assert [walk(lu, wt, caps[3 * i], w, ts)[1] for i in range(len(counts))] == counts  # (the cases are the ones named)


@pytest.mark.parametrize("E", [5, CHUNK + 1])
def test_sums_beyond_32_bits(solver, E):
    lu, wt = T0 + 10 * np.arange(E, dtype=np.int64), np.full(E, 2**31 - 1, np.int32)
    caches = [(lu, wt, cap) for cap in (2**31 - 1, 2**31, 2**40)]
    check(solver, caches, [(k, 2**31 - 1, ts) for k in range(3) for ts in (0, T0 + 10 * (E // 2) + 5, T0 + 10 * (E - 1) + 5)])


@pytest.mark.parametrize("E", [TEAM + 1, CHUNK + 1])
def test_rows_that_take_the_walk_inside_the_search_kernel(solver, E):
    lu, wt = deque_of(E)
    swapped = lu.copy()
    swapped[[E // 2, E // 2 + 1]] = swapped[[E // 2 + 1, E // 2]]  # one entry out of time order, loaded as it is
    caches = [(lu, wt, int(wt.sum()) // 2), (swapped, wt, int(wt.sum()) // 2)]
    stamps = (T0 - 5, T0 + 10 * (E // 2) + 5, int(swapped[E // 2]), 0)
    reqs = [(k, w, ts) for ts in stamps for k, w in ((0, 3), (1, 3), (0, -5))]  # the three kinds side by side in a wavefront
    info = check(solver, caches, reqs, searched=len(stamps))
    assert (info["n_above"], info["n_searchable"]) == (2, 1)


def test_the_table_follows_the_store(solver):
    E = CHUNK + 1
    lu, wt = deque_of(E)
    cap = int(wt.sum())
    reqs = [(0, 3, ts) for ts in (T0 - 5, T0 + 10 * (E // 2) + 5, 0)]
    gen = check(solver, [(lu, wt, cap)], reqs)["generation"]
    solver.load_caches_keyed([0, E], lu, wt, np.arange(E), [cap])
    op = np.zeros(1, dtype=_lib.CACHE_OP)
    op["op"], op["key"], op["arg"], op["time"] = _lib.COP_PUT_IF_ABSENT, E, 7, T0 + 10 * (E // 2) + 5  # inserts in the middle, evicts
    outs, _ = solver.cache_replay(op, NOW)
    assert outs["result"][0] == 1 and outs["n_evicted"][0] > 0
    after = solver.cache_read(0, 4096)
    assert len(after["weight"]) == E + 1 - outs["n_evicted"][0]
    assert check(solver, [(after["last_used"], after["weight"], cap)], reqs)["generation"] == gen + 1


def test_short_caches_keep_the_walk_at_the_default_threshold(monkeypatch):
    monkeypatch.delenv("MMP_EVICT_SEARCH_FROM", raising=False)
    s = Solver(100, 1000)
    try:
        lu, wt = deque_of(20)
        info = check(s, [(lu, wt, 30), (lu, wt, 1000)], [(k, 3, ts) for k in (0, 1) for ts in (T0 - 5, T0 + 105, 0)], searched=0)
        assert info["generation"] == 0 and info["n_above"] == 0
    finally:
        s.close()
