"""GPU: the replay of caches beyond the 2 047 slots of the LDS tile (mmp_cache_slots_limit, cache_wide_kernels.hpp: the deque
blocked in global memory).  The reference's own vectors (tests/golden/ref_clhm_edges.npz) through the blocked kernel with
MMP_CACHE_WIDE_FROM=0; then sizes up to the limit against the C oracle, operation by operation: result, victims in listener order,
buffer weight, weightedSize, oldestTime, and the deque after every call.  Every comparison is exact.

The script of the sizes runs as two calls, because a call's slots are its entries + its inserts and 262 143 entries leave room for
one: call A holds the reads, ONE insert (older than everything), a removal and the three evicting weight updates, call B the 130
equal-stamped inserts, the insert "now" and the manager's operations, on the cache A left (1 130 entries shorter)."""
import ctypes as C

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd.solver import MmpError, Solver
from oracle import bind as ob
from tests import ref_clhm_cases as rc
from tests import test_ref_clhm_edges_gpu as edges

pytestmark = pytest.mark.gpu
NOW = rc.NOW
T0 = NOW - 10_000_000
W, RESERVED = 3, 6000
LIBC = C.CDLL(None)
LIBC.realloc.restype, LIBC.realloc.argtypes = C.c_void_p, [C.c_void_p, C.c_size_t]


@pytest.mark.parametrize("name", edges.NAMES)
def test_reference_vectors_through_the_blocked_kernel(monkeypatch, name):
    monkeypatch.setenv("MMP_CACHE_WIDE_FROM", "0")
    v = rc.load_edge_case(np.load(edges.GOLDEN), name)
    last = len(v["bounds"]) - 1
    s = Solver(100, 1000)
    try:
        edges._replay(s, v, [0, last])
        edges._replay(s, v, list(range(last + 1)))
    finally:
        s.close()


def _oracle(E, managed, slack=W):
    """keys 1 .. E, weight W, lastUsed ascending from T0 in steps of 10, `slack` units free; a managed cache's pinned entry behind
    them.  Written into the oracle's node array: a put per entry would read the whole deque E times."""
    h = ob.CCache(W * E + slack + (RESERVED if managed else 0), RESERVED if managed else None, NOW)
    lu, wt, key = h.nodes()
    nodes = np.zeros(E + len(key), ob.ORC_NODE)
    nodes["last_used"] = np.concatenate([T0 + 10 * np.arange(E), lu])
    nodes["weight"] = np.concatenate([np.full(E, W), wt])
    nodes["key"] = np.concatenate([1 + np.arange(E), key])
    h.c.nodes = LIBC.realloc(h.c.nodes, max(nodes.nbytes, 16))
    C.memmove(h.c.nodes, nodes.ctypes.data, nodes.nbytes)
    h.c.n = h.c.cap_nodes = len(nodes)
    h.c.weighted_size = int(nodes["weight"].sum())
    h.c.oldest_time = int(nodes["last_used"][0]) if len(nodes) else -1
    if managed:
        h.u.total_occupancy = W * E
    return h


def _load(s, caches):
    seg = np.concatenate([[0], np.cumsum([h.c.n for h in caches])]).astype(np.int32)
    cols = [np.concatenate(x) for x in zip(*(h.nodes() for h in caches))]
    ubm = np.zeros(len(caches), dtype=_lib.UBM_STATE)
    for i, h in enumerate(caches):
        ubm[i] = (h.u.reserved, h.u.total_unloading, h.u.total_occupancy, h.u.cache_deficit, 0) if h.u is not None else (-1, 0, 0, 0, 0)
    s.load_caches_keyed(seg, *cols, np.array([h.c.capacity for h in caches], np.int64), ubm)


def _oracle_call(caches, ops):
    """the operations on the oracle: per operation (result, victims, buffer weight, weightedSize, oldestTime)"""
    want = []
    for o in ops:
        h = caches[o["cache"]]
        res, ev = h.apply(int(o["op"]), int(o["key"]), int(o["arg"]), int(o["time"]), int(o["flag"]), NOW)
        if h.u is not None:
            assert h.u.n_evicted <= 1024  # ORC_UBM_MAX_EVICTED: the record held every victim
            h.u.n_evicted = 0
        want.append((res, ev, h.lib.orc_ubm_buffer_weight(C.byref(h.u)) if h.u is not None else 0, h.c.weighted_size, h.oldest_time()))
    return want


def _check_call(s, caches, rows):
    ops = np.array(rows, dtype=_lib.CACHE_OP)
    want = _oracle_call(caches, ops)
    outs, ev = s.cache_replay(ops, NOW)
    for i, (o, w) in enumerate(zip(outs, want)):
        got = (o["result"], list(ev[o["evicted_off"]: o["evicted_off"] + o["n_evicted"]]), o["buffer_weight"], o["weighted_size"], o["oldest_time"])
        assert got == w, (i, ops[i])
    for c, h in enumerate(caches):
        st = s.cache_read(c, max_entries=h.c.n + 1)
        lu, wt, key = h.nodes()
        assert np.array_equal(st["key"], key) and np.array_equal(st["last_used"], lu) and np.array_equal(st["weight"], wt), c
        assert (st["capacity"], st["weighted_size"]) == (h.c.capacity, h.c.weighted_size)
        if h.u is not None:
            u = st["ubm"]
            assert (u["total_unloading"], u["total_occupancy"], u["cache_deficit"]) == (h.u.total_unloading, h.u.total_occupancy, h.u.cache_deficit)
    return outs


def _call_a(c, managed, E):
    put, rem = (4, 10) if managed else (0, 3)
    mid, hot = E // 2, E - 1  # hot: the key whose weight grows (near the tail: it stays)
    stamps = (0, T0 + 10 * mid + 5, 0, T0 + 10 * (E - 1), 0, T0 + 7, 0)  # "now", into the middle, a tie with the tail, no move
    rows = [(c, 1, p + 1, 0, t, 0, 0) for p, t in zip((0, 63, 64, 127, 128, mid, E - 1), stamps)]
    rows += [(c, put, E + 1, W, T0 - 5, 0, 0), (c, rem, mid + 8, 0, 0, 0, 0)]
    # the cache is W short of full: +4 evicts 1 and leaves 2 free, +389 evicts 129, +3000 evicts 1000
    return rows + [(c, 2, hot, W + 4, -1, 0, 0), (c, 2, hot, W + 393, -1, 0, 0), (c, 2, hot, W + 3393, -1, 0, 0)]


def _call_b(c, managed, E):
    put = 4 if managed else 0
    rows = [(c, put, E + 2 + i, W, T0 + 10 * (E // 2 + 300) + 3, 0, 0) for i in range(130)]  # one block fills: the cache re-spreads
    rows += [(c, put, E + 200, W, 0, 0, 0)]
    if managed:  # a failed unload shrinks the capacity (100 victims reach the listener), a finished one, an insert that evicts 14
        rows += [(c, 9, 0, 300, 0, 0, 0), (c, 9, 0, 30, 0, 1, 0), (c, 4, E + 201, 40, 0, 0, 0)]
    return rows


@pytest.mark.parametrize("E", [2046, 2047, 5000, 65600, 262143])
def test_sizes_equal_the_oracle(E):
    caches = [_oracle(E, False), _oracle(E - 1, True)]  # E entries each: the manager's pinned one is the managed cache's last
    s = Solver(100, 1000)
    try:
        s.cache_slots_limit(262144)
        _load(s, caches)
        outs = _check_call(s, caches, _call_a(0, False, E) + _call_a(1, True, E - 1))
        assert list(outs["n_evicted"][9:12]) == [1, 129, 1000]
        _check_call(s, caches, _call_b(0, False, E) + _call_b(1, True, E - 1))
    finally:
        s.close()


def test_four_team_lists_in_one_call():
    caches = [_oracle(n, False, slack=0) for n in (10, 100, 1000, 3000)]
    s = Solver(100, 1000)
    try:
        s.cache_slots_limit(4096)
        _load(s, caches)
        rows = []
        for c, h in enumerate(caches):
            n = h.c.n
            rows += [(c, 1, 1, 0, 0, 0, 0), (c, 0, n + 1, W, 0, 0, 0), (c, 0, n + 2, W, T0 - 5, 0, 0), (c, 2, n, 3 * W + 1, -1, 0, 0), (c, 3, 5, 0, 0, 0, 0)]
        _check_call(s, caches, rows)
    finally:
        s.close()


def test_victims_last_used_through_replay_kt():
    E = 5000
    ids = [b"m%05d" % i for i in range(E + 3)]  # key k is row k
    h = _oracle(E, False)
    s = Solver(100, 1000)
    try:
        s.cache_slots_limit(8192)
        s.load_pod_ids(["aaaaaa-1"])
        reg = np.zeros(len(ids), _lib.MODEL_ROW)
        reg["last_used"] = 1
        s.load_models(reg, np.zeros(0, np.int32), np.zeros(0, np.int64))
        s.model_ids_load(ids)
        lu, wt, key = h.nodes()
        s.load_caches_keyed_k([0, E], lu, wt, [ids[k] for k in key], [h.c.capacity])
        ops = np.array([(0, 1, 3, 0, T0 + 10 * 4000 + 1, 0, 0), (0, 0, E + 1, W, 0, 0, 0), (0, 2, E, W + 600, -1, 0, 0),
                        (0, 0, E + 2, W, T0 + 10 * 2500 + 5, 0, 0)], dtype=_lib.CACHE_OP)
        want = []
        for o in ops:
            before = dict(zip(h.nodes()[2].tolist(), h.nodes()[0].tolist()))
            _, ev = h.apply(int(o["op"]), int(o["key"]), int(o["arg"]), int(o["time"]), 0, NOW)
            want.append((ev, [before[k] for k in ev]))
        outs, rows, _, _, _, times = s.cache_replay_kt(ops, [ids[k] for k in ops["key"]], NOW)
        got = [(list(rows[o["evicted_off"]: o["evicted_off"] + o["n_evicted"]]), list(times[o["evicted_off"]: o["evicted_off"] + o["n_evicted"]]))
               for o in outs]
        assert got == want and [len(e) for e, _ in want] == [0, 0, 200, 1]
        st = s.cache_read(0, max_entries=E + 2)
        assert np.array_equal(st["key"], h.nodes()[2]) and np.array_equal(st["last_used"], h.nodes()[0])
    finally:
        s.close()


def test_the_limit():
    E = 262144
    lus, wts, keys = T0 + np.arange(E, dtype=np.int64), np.full(E, W, np.int32), 1 + np.arange(E, dtype=np.int32)
    put = np.array([(0, 0, E + 1, W, 0, 0, 0)], dtype=_lib.CACHE_OP)
    s = Solver(100, 1000)
    try:
        for bad in (2046, 262145):
            with pytest.raises(MmpError) as e:
                s.cache_slots_limit(bad)
            assert e.value.code == _lib.MMP_EINVAL
        s.load_caches_keyed([0, 2047], lus[:2047], wts[:2047], keys[:2047], [10**9])
        with pytest.raises(MmpError) as e:  # a context that never raised it: 2 048 slots are refused
            s.cache_replay(put, NOW)
        assert e.value.code == _lib.MMP_EINVAL
        s.cache_slots_limit(262144)
        assert s.cache_replay(put, NOW)[0]["result"][0] == 1
        s.load_caches_keyed([0, E, E + 2], np.append(lus, [5, 6]), np.append(wts, [W, W]), np.append(keys, [1, 2]), [10**9, 10**9])
        with pytest.raises(MmpError) as e:
            s.cache_replay(np.array([(1, 1, 1, 0, 0, 0, 0), put[0]], dtype=_lib.CACHE_OP), NOW)
        assert e.value.code == _lib.MMP_EINVAL and b"262144" in s.lib.mmp_last_error(s.h)
        st, small = s.cache_read(0, max_entries=E), s.cache_read(1)
        assert np.array_equal(st["key"], keys) and np.array_equal(st["last_used"], lus) and st["weighted_size"] == W * E
        assert list(small["key"]) == [1, 2] and list(small["last_used"]) == [5, 6]
    finally:
        s.close()
