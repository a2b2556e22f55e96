"""GPU: mmp_evict_batch_k, eviction evaluations on the resident caches by model id (evict_resident_kernels.hpp).  Every comparison
is exact.  Two references: for every row a SECOND context that holds one copy of the asked cache per row (read back from the
context under test) and applies the rows with one mmp_cache_replay_k, one operation per copy; for unmanaged inserts also the plain
walk of tests/evict_search_ref.py.  The last test holds the managed cascade to the reference's own recorded answers."""
import os

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd.solver import MmpError, Solver  # noqa: F401
from tests import ref_clhm_cases as rc
from tests.evict_search_ref import linear
from tests.test_cache_keyed_gpu import ctx
from tests.test_evict_search_gpu import NOW, T0, deque_of, runs

pytestmark = pytest.mark.gpu
UB, I64_MAX = _lib.UNLOADBUF_KEY, 2**63 - 1
PUT, NEW = _lib.COP_PUT_IF_ABSENT, _lib.COP_UBM_INSERT_NEW_ENTRY
STATE = ("n_evicted", "buffer_weight", "weighted_size", "oldest_time")
MAXE = 8192


def ids_of(m):
    return [b"m%d" % r for r in range(m)]


def op_rows(rows):
    """[(cache, op, arg, time)] -> CACHE_OP rows (the key field is never read)"""
    ops = np.zeros(len(rows), _lib.CACHE_OP)
    for i, (c, op, arg, t) in enumerate(rows):
        ops[i] = (c, op, -7, arg, t, 0, 0)
    return ops


def load(s, ids, lu, wt, cap, reserved=-1, tu=0):
    """one cache: entry j is row j; managed (reserved >= 0): the pinned entry at the tail, weight = the reserve"""
    n, m = len(lu), int(reserved >= 0)
    ubm = np.zeros(1, _lib.UBM_STATE)
    ubm["reserved"], ubm["total_unloading"], ubm["total_occupancy"] = reserved, tu, int(np.sum(wt))
    s.load_caches_keyed_k([0, n + m], np.append(lu, [I64_MAX] * m), np.append(wt, [reserved] * m), ids[:n] + [b"x"] * m, [cap], ubm,
                          is_unloadbuf=np.append(np.zeros(n, np.uint8), [1] * m))


def snap(s, n_caches):
    out = []
    for c in range(n_caches):
        st = s.cache_read_k(c, MAXE)
        out.append((st["row"].tobytes(), st["weight"].tobytes(), st["last_used"].tobytes(), st["capacity"], st["weighted_size"],
                    st["ubm"].tobytes()))
    return out


def check(s, n_caches, ids, ops, keys, empty=(), limit=None):
    """ask `ops` of s; nothing may change; every row against the replay of that one op on a copy of its cache, and its victims
    against the head of the deque as s reads it back"""
    before = snap(s, n_caches)
    got = s.evict_batch_k(ops, keys, NOW)
    assert snap(s, n_caches) == before
    valid = [i for i in range(len(ops)) if 0 <= ops[i]["cache"] < n_caches]
    states = {int(c): s.cache_read_k(int(c), MAXE) for c in set(ops["cache"][valid])}
    b = ctx(ids, empty)
    if limit:
        b.cache_slots_limit(limit)
    sts = [states[int(ops[i]["cache"])] for i in valid]
    b.load_caches_keyed_k(np.cumsum([0] + [len(st["row"]) for st in sts]), np.concatenate([st["last_used"] for st in sts]),
                          np.concatenate([st["weight"] for st in sts]), [k or b"x" for st in sts for k in st["ids"]],
                          [st["capacity"] for st in sts], np.array([st["ubm"] for st in sts], _lib.UBM_STATE),
                          is_unloadbuf=np.concatenate([st["row"] == UB for st in sts]).astype(np.uint8))
    ops2 = ops[valid].copy()
    ops2["cache"] = np.arange(len(valid))
    outs, ev, _, status, rows = b.cache_replay_k(ops2, [keys[i] for i in valid], NOW)
    b.close()
    for j, i in enumerate(valid):
        g, o, st = got[i], outs[j], sts[j]
        assert (g["key_status"], g["row"]) == (status[j], rows[j]), i
        assert g["result"] == (-1 if status[j] == _lib.CKEY_UNKNOWN else o["result"]), (i, ops[i])
        assert tuple(g[f] for f in STATE) == tuple(o[f] for f in STATE), (i, ops[i], g, o)
        victims = sorted(int(r) for r in ev[o["evicted_off"]: o["evicted_off"] + o["n_evicted"]])
        head = s.cache_read_k(int(ops[i]["cache"]), max(int(g["n_evicted"] - g["self_evicted"]), 1))["row"]
        assert victims == sorted([int(r) for r in head[: g["n_evicted"] - g["self_evicted"]]] + [int(rows[j])] * int(g["self_evicted"])), i
        if st["ubm"]["reserved"] < 0 and g["result"] == 1:
            want = linear(st["last_used"], st["weight"], st["capacity"], int(ops[i]["arg"]), int(ops[i]["time"]))
            assert tuple(int(g[f]) for f in ("insert_pos", "n_evicted", "self_evicted", "weighted_size", "oldest_time")) == want, i
    for i in set(range(len(ops))) - set(valid):
        assert got[i]["result"] == -1 and got[i]["oldest_time"] == -1 and not any(got[i][f] for f in STATE[:3])
    return got


@pytest.fixture(params=["0", None], ids=["from0", "default"])
def threshold(request, monkeypatch):
    if request.param is None:
        monkeypatch.delenv("MMP_EVICT_SEARCH_FROM", raising=False)
    else:
        monkeypatch.setenv("MMP_EVICT_SEARCH_FROM", request.param)


@pytest.mark.parametrize("managed", [False, True], ids=["plain", "managed"])
@pytest.mark.parametrize("E", [0, 1, 15, 16, 17, 1023, 1024, 1025, 2049])
def test_lengths_stamps_weights(threshold, E, managed):
    """stamps at the head, at the tail, now and on a run of four ties; weights that evict 0, 1, 64, 65 and all entries and the
    new entry itself (at the tail P[v] + 1 evicts v entries under a capacity of the total + 1)"""
    ids = ids_of(E + 3)
    lu, wt = deque_of(E)
    P = np.concatenate([[0], np.cumsum(wt.astype(np.int64))])
    R = 7 if managed else -1
    cap = int(P[E]) + 1 + max(R, 0)
    s = ctx(ids)
    load(s, ids, lu, wt, cap, R)
    weights = [int(P[v]) + 1 for v in sorted({0, 1, 64, 65, E}) if v <= E] + [cap + 1]
    stamps = [T0 - 5, T0 + 10 * E + 5, 0] + [int(lu[a]) for a in runs(E)]
    rows = [(0, op, w, ts) for op in ((PUT, NEW) if managed else (PUT,)) for w in weights for ts in stamps]
    got = check(s, 1, ids, op_rows(rows), [ids[E]] * len(rows), limit=MAXE)
    assert {int(n) for n in got["n_evicted"]} >= {v for v in (0, 1, 64, 65, E) if v <= E}
    s.close()


def _home(key, cells):
    x = (key & 0xFFFFFFFF) + 0x9E3779B97F4A7C15 & (2**64 - 1)
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & (2**64 - 1)
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & (2**64 - 1)
    return ((x ^ (x >> 31)) & 0xFFFFFFFF) & (cells - 1)


@pytest.mark.parametrize("E,managed", [(17, False), (2049, False), (2049, True)])
def test_keys(E, managed, monkeypatch):
    """present at the head and at the tail (a hit now, and one stamped older than the entry), an absent key whose cell run wraps
    the end of the index, a deleted record's row, an unknown id, a cache index out of range"""
    monkeypatch.delenv("MMP_EVICT_SEARCH_FROM", raising=False)
    M = 6000
    ids = ids_of(M)
    cells = 64
    while cells < 2 * (E + managed):
        cells *= 2
    wrap = next(r for r in range(E + 1, M) if _home(r, cells) > cells - 16)
    lu, wt = deque_of(E)
    s = ctx(ids, empty=(E,))
    load(s, ids, lu, wt, int(wt.sum()) + 20, 9 if managed else -1)
    keys, rows = [], []
    for op in (PUT, NEW):
        for k, c in ((ids[0], 0), (ids[E - 1], 0), (ids[wrap], 0), (ids[E], 0), (b"no such model", 0), (ids[wrap], 1), (ids[wrap], -1)):
            for ts in (0, T0 - 100):
                keys.append(k)
                rows.append((c, op, 40, ts))
    got = check(s, 1, ids, op_rows(rows), keys, empty=(E,), limit=MAXE)
    assert list(got["result"][:14]) == [0, 0, 0, 0, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1]
    assert list(got["key_status"][6:10]) == [_lib.CKEY_EMPTY_ROW] * 2 + [_lib.CKEY_UNKNOWN] * 2
    assert list(got["insert_pos"][:4]) == [0, 0, E - 1, E - 1]
    for bad in (_lib.COP_GET, _lib.COP_UBM_INSERT_FAILED_PLACEHOLDER):
        with pytest.raises(MmpError) as e:
            s.evict_batch_k(op_rows([(0, bad, 1, 0)]), [ids[0]], NOW)
        assert e.value.code == _lib.MMP_EINVAL
    s.close()


@pytest.mark.parametrize("E,kind", [(1500, "hit"), (1500, "put"), (1500, "remove"), (5000, "put")])
def test_fresh_after_every_writer(E, kind, monkeypatch):
    """ask, replay, ask again: the second answer is the new state's.  Then across mmp_models_retire with a renumbered key, and
    MMP_ESTATE behind mmp_model_ids_load.  5 000 entries: behind mmp_cache_slots_limit, the replay on the blocked route."""
    monkeypatch.delenv("MMP_EVICT_SEARCH_FROM", raising=False)
    ids = ids_of(E + 4)
    lu, wt = deque_of(E)
    s = ctx(ids)
    s.cache_slots_limit(MAXE)
    load(s, ids, lu, wt, int(wt.sum()) + 3)
    s.cache_replay_k(op_rows([(0, _lib.COP_REMOVE, 0, 0)]), [ids[0]], NOW)  # (row 0 leaves the cache: it is retired below)
    ask = op_rows([(0, PUT, w, ts) for w in (1, 200) for ts in (0, T0 + 5, T0 + 10 * E // 2)] + [(0, PUT, 1, 0)])
    keys = [ids[E]] * 6 + [ids[1]]
    first = check(s, 1, ids, ask, keys, limit=MAXE)
    step = {"hit": (_lib.COP_GET, ids[1], 0), "put": (PUT, ids[E + 1], 300), "remove": (_lib.COP_REMOVE, ids[E // 2], 0)}[kind]
    s.cache_replay_k(op_rows([(0, step[0], step[2], 0)]), [step[1]], NOW)
    second = check(s, 1, ids, ask, keys, limit=MAXE)
    assert first.tobytes() != second.tobytes()
    remap = s.models_retire([0])
    assert remap[E] == E - 1
    third = check(s, 1, ids[1:], ask, keys, limit=MAXE)
    assert list(third["row"]) == [r - 1 for r in second["row"]]
    assert [tuple(r[f] for f in STATE) for r in third] == [tuple(r[f] for f in STATE) for r in second]
    s.model_ids_load(ids[1:])
    with pytest.raises(MmpError) as e:
        s.evict_batch_k(ask, keys, NOW)
    assert e.value.code == _lib.MMP_ESTATE
    s.close()


@pytest.mark.parametrize("search_from", ["0", None], ids=["from0", "default"])
def test_managed_cascade_recorded(search_from, monkeypatch):
    """the mass_managed runs of the reference's own vectors: the state in front of each probe (a put or an insertNewEntry), the
    row against the recorded answer — among them the cascade that evicts down to the pinned entry alone"""
    if search_from is None:
        monkeypatch.delenv("MMP_EVICT_SEARCH_FROM", raising=False)
    else:
        monkeypatch.setenv("MMP_EVICT_SEARCH_FROM", search_from)
    v = rc.load_edge_case(np.load(os.path.join(os.path.dirname(__file__), "golden", "ref_clhm_edges.npz")), "mass_managed")
    j, last = len(v["bounds"]) - 2, len(v["bounds"]) - 1
    probes = [int(rc.run_rows(v, c)[1][0]) for c in range(len(v["caps"]))]
    assert all(len(rc.run_rows(v, c)[1]) == 1 for c in range(len(v["caps"]))) and set(v["ops"]["op"][probes]) == {PUT, NEW}
    hdr = v[f"b{j}/hdr"]
    names = sorted({int(k) for k in v[f"b{j}/key"]} | {int(k) for k in v["ops"]["key"][probes]} - {UB})
    row_of = {k: r for r, k in enumerate(k for k in names if k != UB)}
    ids = ids_of(len(row_of))
    ubm = np.zeros(len(hdr), _lib.UBM_STATE)
    ubm["reserved"], ubm["total_unloading"], ubm["total_occupancy"], ubm["cache_deficit"] = v["reserved"], hdr[:, 3], hdr[:, 4], hdr[:, 5]
    key = v[f"b{j}/key"]
    s = ctx(ids)
    s.load_caches_keyed_k(np.cumsum(np.append(0, hdr[:, 0])), v[f"b{j}/last_used"], v[f"b{j}/weight"],
                          [b"x" if k == UB else ids[row_of[int(k)]] for k in key], hdr[:, 1], ubm, is_unloadbuf=(key == UB))
    ops = v["ops"][probes].astype(_lib.CACHE_OP)
    got = s.evict_batch_k(ops, [ids[row_of[int(k)]] for k in ops["key"]], rc.NOW)
    want = v["outs"][probes]
    for f in ("result",) + STATE:
        assert list(got[f]) == list(want[f]), f
    after = v[f"b{last}/hdr"]
    assert any(after[c, 0] == 1 and want[c]["n_evicted"] > 1 for c in range(len(hdr)))  # down to the pinned entry alone
    s.close()
