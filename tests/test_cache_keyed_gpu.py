"""GPU: the stateful caches by model id (mmp_caches_load_keyed_k, mmp_cache_replay_k, mmp_cache_evicted_ids, mmp_cache_read_k) and
mmp_models_retire carrying bound caches, against tests/cache_keyed_model.py and against the plain calls.  Every comparison is exact.

The reference through the keyed path: every case of tests/golden/ref_clhm_edges.npz (the reference's own local-cache text, read as
tests/test_ref_clhm_edges_gpu.py reads it) with each vector key k renamed to the id of registry row perm[k], perm a seeded
permutation under which no row equals its vector key.  Keyed equals resolve + plain + ids_get on a second context, at the
wavefront and kIdTabBlock edges of the op count."""
import threading

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd.solver import MmpError, Solver
from oracle import bind as ob
from tests import ref_clhm_cases as rc
from tests.cache_keyed_model import IdTable, Refused
from tests.test_cache_replay_gpu import _export, _mk_caches, _random_ops, ops_res

pytestmark = pytest.mark.gpu
NOW = 1_760_000_000_000
UB = _lib.UNLOADBUF_KEY
NAMES = ("lengths_plain", "lengths_managed", "lengths_big", "mass_plain", "mass_managed", "clhm", "manager", "wide")
OUT_FIELDS = ["result", "n_evicted", "buffer_weight", "weighted_size", "oldest_time"]


def make_ids(rng, n, lo=1, hi=40):
    """n distinct ids of lo..hi bytes (any byte value)"""
    out, seen = [], set()
    while len(out) < n:
        b = rng.integers(0, 256, int(rng.integers(lo, hi + 1)), dtype=np.uint8).tobytes()
        if b not in seen:
            seen.add(b)
            out.append(b)
    return out


def ctx(ids, empty=()):
    """a context whose registry has one row per id: live rows, but the `empty` ones (what a deletion leaves)"""
    s = Solver(100, 1000)
    s.load_pod_ids(["aaaaaa-1"])
    rows = np.zeros(len(ids), _lib.MODEL_ROW)
    rows["last_used"] = 1
    rows["last_used"][list(empty)] = 0
    s.load_models(rows, np.zeros(0, np.int32), np.zeros(0, np.int64))
    s.model_ids_load(ids)
    return s


def snapshot(s, n_caches):
    """every cache as the plain read shows it, as bytes"""
    out = []
    for c in range(n_caches):
        st = s.cache_read(c)
        out.append((st["key"].tobytes(), st["weight"].tobytes(), st["last_used"].tobytes(), st["capacity"], st["weighted_size"],
                    st["ubm"].tobytes()))
    return out


def ev_of(outs, ev, i):
    return list(ev[outs[i]["evicted_off"]: outs[i]["evicted_off"] + outs[i]["n_evicted"]])


def code_of(e):
    return e.value.code


# ---- the reference through the keyed path ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def vec():
    import os
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "ref_clhm_edges.npz"))


def _renamed(v, seed):
    """vector key -> row (never equal), the ids of the rows, and the case's ops as the keyed call takes them"""
    last = len(v["bounds"]) - 1
    ks = set(int(k) for k in v["ops"]["key"]) | {int(k) for j in range(1, last + 1) for k in v[f"b{j}/key"]}
    ks = sorted(k for k in ks if k != UB)
    assert all(k >= 0 for k in ks)
    rng = np.random.default_rng(seed)
    M = len(ks) + 7
    while True:
        perm = rng.permutation(M)[: len(ks)]
        if not np.any(perm == np.array(ks)):
            break
    row_of = {k: int(r) for k, r in zip(ks, perm)}
    ids = make_ids(rng, M)
    ops = v["ops"].astype(_lib.CACHE_OP)
    keys = []
    for i in range(len(ops)):
        k = int(ops[i]["key"])
        if k == UB:
            ops[i]["reserved"] = _lib.COPK_RAW_KEY
            keys.append(b"not read")
        elif int(ops[i]["op"]) in _lib.COP_KEYLESS:
            keys.append(b"not read either")
        else:
            ops[i]["key"] = -12345  # never read
            keys.append(ids[row_of[k]])
    return row_of, ids, ops, keys


def _check_case(s, v, row_of, ids, ops, keys, cut_at):
    seg, lus, wts, k0 = rc.initial_state(v["caps"], v["reserved"])
    ubm = np.zeros(len(v["caps"]), dtype=_lib.UBM_STATE)
    ubm["reserved"] = v["reserved"]
    assert (k0 == UB).all()
    got_rows = s.load_caches_keyed_k(seg, lus, wts, [b"x"] * len(k0), v["caps"], ubm, is_unloadbuf=np.ones(len(k0), np.uint8))
    assert (got_rows == UB).all()
    back = {r: k for k, r in row_of.items()}
    for j0, j1 in zip(cut_at[:-1], cut_at[1:]):
        a, b = int(v["bounds"][j0]), int(v["bounds"][j1])
        outs, ev, ev_ids, status, rows = s.cache_replay_k(ops[a:b], keys[a:b], rc.NOW)
        assert not status.any()
        for i in range(b - a):
            o, g = v["outs"][a + i], outs[i]
            want_ev = [int(k) for k in v["evicted"][o["evicted_off"]: o["evicted_off"] + o["n_evicted"]]]
            sl = slice(g["evicted_off"], g["evicted_off"] + g["n_evicted"])
            assert tuple(g[f] for f in OUT_FIELDS) == tuple(o[f] for f in OUT_FIELDS), (v["name"], a + i, ops[a + i])
            assert [back[int(r)] for r in ev[sl]] == want_ev, (v["name"], a + i)
            assert ev_ids[sl] == [ids[row_of[k]] for k in want_ev], (v["name"], a + i)
        used = np.zeros(len(ev), bool)
        for g in outs:
            used[g["evicted_off"]: g["evicted_off"] + g["n_evicted"]] = True
        assert (ev[~used] == -1).all() and all(x == b"" for x, u in zip(ev_ids, used) if not u)
        for c in range(len(v["caps"])):
            hdr, ck, cw, cl = rc.edge_state(v, j1, c)
            st = s.cache_read_k(c)
            assert list(st["row"]) == [UB if k == UB else row_of[int(k)] for k in ck], (v["name"], j1, c)
            assert st["ids"] == [b"" if k == UB else ids[row_of[int(k)]] for k in ck], (v["name"], j1, c)
            assert np.array_equal(st["weight"], cw) and np.array_equal(st["last_used"], cl), (v["name"], j1, c)
            assert (st["capacity"], st["weighted_size"]) == (hdr[1], hdr[2]), (v["name"], j1, c)
            if v["reserved"][c] >= 0:
                u = st["ubm"]
                assert (u["total_unloading"], u["total_occupancy"], u["cache_deficit"]) == (hdr[3], hdr[4], hdr[5]), (v["name"], j1, c)


@pytest.mark.parametrize("name", NAMES)
def test_the_reference_text_through_the_keyed_path(vec, name):
    v = rc.load_edge_case(vec, name)
    row_of, ids, ops, keys = _renamed(v, 4100 + NAMES.index(name))
    last = len(v["bounds"]) - 1
    s = ctx(ids)
    try:
        _check_case(s, v, row_of, ids, ops, keys, [0, last])                  # one call
        _check_case(s, v, row_of, ids, ops, keys, list(range(last + 1)))      # cut at every recorded boundary
    finally:
        s.close()


def test_the_vectors_bring_the_edges_through_the_resolver_and_the_gather(vec):
    """all three team widths, 2 046 entries, and one op evicting 1, 63, 64, 65 and 257 entries"""
    n_ev, widths, entries = set(), set(), set()
    for name in NAMES:
        v = rc.load_edge_case(vec, name)
        n_ev |= set(int(x) for x in v["outs"]["n_evicted"])
        last = len(v["bounds"]) - 1
        n0 = (v["reserved"] >= 0).astype(np.int64)
        ins = np.bincount(v["ops"]["cache"][np.isin(v["ops"]["op"], _lib.COP_INSERTING)], minlength=len(n0))
        widths |= {rc.team_width(int(x)) for x in n0 + ins}
        entries |= set(int(x) for j in range(1, last + 1) for x in v[f"b{j}/hdr"][:, 0])
    assert {1, 63, 64, 65, 257} <= n_ev and widths == {8, 16, 64} and 2046 in entries


# ---- keyed = resolve + plain + ids_get ----------------------------------------------------------------------------------------------

def _world(seed, n_caches=5):
    """oracle caches as tests/test_cache_replay_gpu.py makes them, whose keys are renamed to rows of a registry"""
    rng = np.random.default_rng(seed)
    managed = rng.random(n_caches) < 0.6
    caches = _mk_caches(rng, n_caches, managed)
    return rng, managed, caches


class Renamer:
    """oracle key -> row, assigned on first sight from a seeded permutation; ids by row"""

    def __init__(self, seed, M):
        rng = np.random.default_rng(seed)
        self.perm = [int(x) for x in rng.permutation(M)]
        self.ids = make_ids(rng, M)
        self.row = {}

    def __call__(self, k):
        k = int(k)
        if k == UB:
            return UB
        if k not in self.row:
            self.row[k] = self.perm[len(self.row)]
        return self.row[k]


def _two_contexts(R, caches):
    seg, lu, wt, key, cap, ubm = _export(caches)
    rows = np.array([R(k) for k in key], np.int32)
    s1, s2 = ctx(R.ids), ctx(R.ids)
    got = s1.load_caches_keyed_k(seg, lu, wt, [b"" if r == UB else R.ids[r] for r in rows], cap, ubm, is_unloadbuf=(rows == UB))
    assert np.array_equal(got, rows)
    s2.load_caches_keyed(seg, lu, wt, rows, cap, ubm)
    return s1, s2


def _keyed_ops(R, ops):
    """(ops for the keyed call, keys, the same ops by row for the plain call)"""
    by_row = ops.copy()
    by_row["key"] = [R(k) if int(o) not in _lib.COP_KEYLESS else k for k, o in zip(ops["key"], ops["op"])]
    keyed = ops.copy()
    keyed["key"] = 77
    keys = [b"-" if int(o) in _lib.COP_KEYLESS else R.ids[r] for r, o in zip(by_row["key"], ops["op"])]
    return keyed, keys, by_row


@pytest.mark.parametrize("n_ops", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_keyed_equals_resolve_then_plain_then_ids_get(n_ops):
    rng, managed, caches = _world(8800 + n_ops)
    R = Renamer(n_ops, 4000)
    ops_res.clear()
    ops = _random_ops(rng, caches, managed, n_ops, 0)
    ops_res.clear()
    keyed, keys, by_row = _keyed_ops(R, ops)
    s1, s2 = _two_contexts(R, _world(8800 + n_ops)[2])  # the same caches as they were before the ops
    try:
        outs, ev, ev_ids, status, rows = s1.cache_replay_k(keyed, keys, NOW)
        res = s2.model_ids_resolve(keys)
        plain = by_row.copy()
        plain["key"] = [r if int(o) not in _lib.COP_KEYLESS else k for r, o, k in zip(res, ops["op"], by_row["key"])]
        assert np.array_equal(plain, by_row)
        outs2, ev2 = s2.cache_replay(plain, NOW)
        assert outs.tobytes() == outs2.tobytes() and len(ev) == len(ev2)
        assert not status.any() and list(rows) == [-1 if int(o) in _lib.COP_KEYLESS else r for r, o in zip(by_row["key"], ops["op"])]
        for i in range(n_ops):
            e = ev_of(outs2, ev2, i)
            assert ev_of(outs, ev, i) == e
            sl = slice(outs[i]["evicted_off"], outs[i]["evicted_off"] + outs[i]["n_evicted"])
            assert ev_ids[sl] == [s2.model_ids_get(int(r), 1)[0] for r in e]
        assert snapshot(s1, len(caches)) == snapshot(s2, len(caches))
        for c, h in enumerate(caches):  # and both equal the oracle
            assert list(s1.cache_read_k(c)["row"]) == [R(k) for k in h.nodes()[2]]
    finally:
        s1.close()
        s2.close()


# ---- keys ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [None, 0])
def test_id_lengths_utf8_a_workgroup_beyond_the_lds_region_offsets_not_from_zero_and_colliding_hashes(monkeypatch, bits):
    if bits is not None:
        monkeypatch.setenv("MMP_MODEL_ID_HASH_BITS", str(bits))  # every id shares one hash: told apart by their bytes
    rng = np.random.default_rng(5)
    edge = [b"", b"a", b"b" * 15, b"c" * 16, b"d" * 17, b"e" * 31, b"f" * 32, b"g" * 33, b"h" * 200, "modèle-é".encode(), "模型-1".encode()]
    long_ids = [b"L%03d" % i + bytes(rng.integers(97, 123, 76, dtype=np.uint8)) for i in range(256)]  # 256 x 80 bytes > kKeyedLdsBytes
    short = [b"s%d" % i for i in range(40)]
    ids = long_ids + edge + short   # ops 0..255: a workgroup whose keys do not fit the LDS region; the next one's do
    assert sum(len(x) for x in long_ids) > 16384 > sum(len(x) for x in edge + short)
    t = IdTable(ids)
    s = ctx(ids)
    try:
        h = ob.CCache(10**9, None, NOW)
        s.load_caches_keyed_k([0, 0], [], [], [], [10**9])
        n = len(ids)
        ops = np.zeros(2 * n, dtype=_lib.CACHE_OP)
        ops["op"] = [_lib.COP_PUT_IF_ABSENT] * n + [_lib.COP_GET] * n
        ops["arg"], ops["time"] = 3, NOW - 50 + np.arange(2 * n) % 7
        keys = ids + ids[::-1]
        want, _ = t.replay([h], ops, keys, NOW)
        blob, off = Solver.pack_keys(keys)
        r = s.cache_replay_k_raw(ops, None, NOW, 64, key_off=off + 5, blob=b"\xffjunk" + blob)  # key_off[0] != 0
        assert list(r["status"]) == [0] * (2 * n) and list(r["rows"]) == [w["key"] for w in want]
        assert list(r["outs"]["result"]) == [w["result"] for w in want] == [1] * (2 * n)
        st = s.cache_read_k(0)
        assert list(st["row"]) == list(h.nodes()[2]) and st["ids"] == [ids[k] for k in h.nodes()[2]]
    finally:
        s.close()


# ---- statuses -------------------------------------------------------------------------------------------------------------------------

IDS5 = [b"a", b"bb", b"", "é".encode(), b"gone", b"spare"]


def _small(managed=True, empty=(4,)):
    """one managed and one plain cache over IDS5: rows 0, 1 and the deleted record's row 4 in cache 0; row 2 in cache 1"""
    s = ctx(IDS5, empty)
    seg = [0, 4 if managed else 3, (4 if managed else 3) + 1]
    ids = ([b"zz"] if managed else []) + [b"a", b"bb", b"gone", b""]
    isu = ([1] if managed else []) + [0, 0, 0, 0]
    lu = ([np.iinfo(np.int64).max] if managed else []) + [NOW - 400, NOW - 300, NOW - 200, NOW - 100]
    if managed:  # the pinned entry is the deque's last node
        ids, isu, lu = ids[1:4] + ids[:1] + ids[4:], isu[1:4] + isu[:1] + isu[4:], lu[1:4] + lu[:1] + lu[4:]
    wt = [10, 10, 10, 100, 5] if managed else [10, 10, 10, 5]
    ubm = np.zeros(2, dtype=_lib.UBM_STATE)
    ubm["reserved"] = [100 if managed else -1, -1]
    ubm["total_occupancy"] = [30 if managed else 0, 0]
    rows = s.load_caches_keyed_k(seg, lu, wt, ids, [1000, 1000], ubm, is_unloadbuf=isu)
    return s, rows


def cop(cache, code, arg=0, time=0, flag=0, key=0, reserved=0):
    return (cache, code, key, arg, time, flag, reserved)


def test_all_three_statuses_and_the_entry_of_a_deleted_record_is_read_and_removed():
    s, rows = _small()
    try:
        assert list(rows) == [0, 1, 4, UB, 2]
        ops = np.array([cop(0, _lib.COP_GET), cop(0, _lib.COP_GET), cop(0, _lib.COP_GET), cop(0, _lib.COP_UBM_REMOVE_ENTRY),
                        cop(0, _lib.COP_GET, key=UB, reserved=1), cop(0, _lib.COP_UBM_SPACE_IS_READY, 1)], dtype=_lib.CACHE_OP)
        outs, ev, ids, status, krow = s.cache_replay_k(ops, [b"a", b"gone", b"nobody", b"gone", b"nobody", b"nobody"], NOW)
        assert list(status) == [_lib.CKEY_LIVE, _lib.CKEY_EMPTY_ROW, _lib.CKEY_UNKNOWN, _lib.CKEY_EMPTY_ROW, _lib.CKEY_LIVE, _lib.CKEY_LIVE]
        assert list(krow) == [0, 4, _lib.CACHE_KEY_UNKNOWN, 4, UB, -1]
        assert list(outs["result"][:5]) == [1, 1, 0, 10, 1]          # removeEntry answers the weight
        st = s.cache_read_k(0)
        assert 4 not in st["row"] and b"gone" not in st["ids"] and st["ids"][list(st["row"]).index(UB)] == b""
        assert s.cache_read_k(1)["ids"] == [b""] and list(s.cache_read_k(1)["row"]) == [2]  # the empty id is not the pseudo-entry
    finally:
        s.close()


@pytest.mark.parametrize("code,arg", [(_lib.COP_GET, 0), (_lib.COP_REMOVE, 0), (_lib.COP_UBM_REMOVE_ENTRY, 0), (_lib.COP_UPDATE_WEIGHT, 7),
                                      (_lib.COP_UBM_ADJUST_SPACE_REQUEST, 639), (_lib.COP_UBM_ADJUST_AFTER_LOAD, 700)])
def test_a_non_inserting_op_under_an_unknown_id_equals_the_plain_call_on_a_key_no_cache_holds(code, arg):
    (s1, _), (s2, _) = _small(), _small()
    try:
        ops = np.array([cop(0, code, arg, NOW - 1)], dtype=_lib.CACHE_OP)
        outs, ev, ids, status, krow = s1.cache_replay_k(ops, [b"nobody"], NOW)
        ops["key"] = 424242
        outs2, ev2 = s2.cache_replay(ops, NOW)
        assert outs.tobytes() == outs2.tobytes() and status[0] == _lib.CKEY_UNKNOWN and krow[0] == _lib.CACHE_KEY_UNKNOWN
        assert ev_of(outs, ev, 0) == ev_of(outs2, ev2, 0)
        assert snapshot(s1, 2) == snapshot(s2, 2)
    finally:
        s1.close()
        s2.close()


@pytest.mark.parametrize("pos", [0, 1, 2])
@pytest.mark.parametrize("code", _lib.COP_INSERTING)
def test_an_inserting_op_under_an_unknown_id_is_not_run(code, pos):
    """first, middle and last of a cache's three ops: every cache byte-identical to a run without it, its out row what a GET of
    an absent key writes — result 0, nothing evicted, the state as the preceding op left it"""
    (s1, _), (s2, _) = _small(), _small()
    try:
        others = [cop(0, _lib.COP_GET, 0, NOW - 3), cop(0, _lib.COP_UBM_ADJUST_AFTER_LOAD, 20)]
        rows = others[:]
        rows.insert(pos, cop(0, code, 900, NOW - 2))
        keys = [b"a", b"bb"]
        keys.insert(pos, b"nobody")
        before = s1.cache_read(0)
        outs, ev, ids, status, krow = s1.cache_replay_k(np.array(rows, dtype=_lib.CACHE_OP), keys, NOW)
        outs2, _, _, _, _ = s2.cache_replay_k(np.array(others, dtype=_lib.CACHE_OP), [b"a", b"bb"], NOW)
        assert snapshot(s1, 2) == snapshot(s2, 2)
        assert [tuple(o[f] for f in OUT_FIELDS) for o in np.delete(outs, pos)] == [tuple(o[f] for f in OUT_FIELDS) for o in outs2]
        g = outs[pos]
        assert (g["result"], g["n_evicted"], status[pos], krow[pos]) == (0, 0, _lib.CKEY_UNKNOWN, _lib.CACHE_KEY_UNKNOWN)
        if pos:
            assert tuple(g[f] for f in OUT_FIELDS[2:]) == tuple(outs[pos - 1][f] for f in OUT_FIELDS[2:])
        else:
            assert (g["buffer_weight"], g["weighted_size"]) == (100, before["weighted_size"])
        assert all(x == b"" for x in ids) and (ev == -1).all()
    finally:
        s1.close()
        s2.close()


# ---- the eviction record ------------------------------------------------------------------------------------------------------------

def _evicting():
    """a plain cache of capacity 30 holding a, bb, gone (10 each): a put of 25 evicts all three"""
    s, _ = _small(managed=False)
    ops = np.array([cop(0, _lib.COP_PUT_IF_ABSENT, 25, NOW - 1)], dtype=_lib.CACHE_OP)
    return s, ops, ["é"]


def test_the_eviction_record_short_buffers_the_context_keeps_it_and_a_retirement_cannot_change_it():
    s, ops, keys = _evicting()
    s.close()
    want_ids = [b"a", b"bb", b"gone", b""]  # 3 entries + 1 insert = 4 slots, three used
    need = sum(len(x) for x in want_ids)
    for room in (0, need - 1, need, need + 9):
        s, _ = _small(managed=False)
        try:
            s.load_caches_keyed_k([0, 3], [NOW - 400, NOW - 300, NOW - 200], [10, 10, 10], [b"a", b"bb", b"gone"], [30])
            r = s.cache_replay_k_raw(ops, keys, NOW, room, fill=0x5A)
            assert r["need"] == need and list(r["evicted_rows"]) == [0, 1, 4, -1] and list(r["id_off"]) == [0, 1, 3, 7, 7]
            if room >= need:
                assert r["id_bytes"][:need].tobytes() == b"".join(want_ids)
            else:
                assert set(r["id_bytes"].tobytes()) <= {0x5A}              # the bytes are not written
            assert list(s.cache_read_k(0)["row"]) == [3]                   # the replay was applied all the same
            assert s.cache_evicted_ids() == want_ids
            remap = s.models_retire([0, 1, 4])                             # the evicted rows: no longer keys of live entries
            assert list(remap) == [-1, -1, 0, 1, -1, 2]
            assert s.cache_evicted_ids() == want_ids                       # bytes, not rows
            st = s.cache_read_k(0)
            assert list(st["row"]) == [1] and st["ids"] == ["é".encode()]
            # replaced by the next keyed replay: no eviction at all, one slot (1 entry, no insert), unused
            outs, ev, ids, status, krow = s.cache_replay_k(np.array([cop(0, _lib.COP_GET)], dtype=_lib.CACHE_OP), ["é"], NOW)
            assert (outs[0]["result"], list(ev), ids, list(krow)) == (1, [-1], [b""], [1])
            assert s.cache_evicted_ids() == [b""]
            s.cache_replay_k(np.zeros(0, dtype=_lib.CACHE_OP), [], NOW)    # n_ops == 0 is valid
            assert s.cache_evicted_ids() == []
        finally:
            s.close()


def test_the_wrapper_falls_back_to_the_kept_record_when_its_buffer_was_short():
    s, ops, keys = _evicting()
    try:
        s.load_caches_keyed_k([0, 3], [NOW - 400, NOW - 300, NOW - 200], [10, 10, 10], [b"a", b"bb", b"gone"], [30])
        outs, ev, ids, status, krow = s.cache_replay_k(ops, keys, NOW, id_bytes_hint=2)
        assert ids == [b"a", b"bb", b"gone", b""] and ev_of(outs, ev, 0) == [0, 1, 4]
    finally:
        s.close()


# ---- the retirement -------------------------------------------------------------------------------------------------------------------

def _registry_bytes(s):
    return [x.tobytes() for x in s.get_models()] + [s.model_ids_get()]


def test_retirement_renumbers_bound_caches_and_refuses_a_live_key():
    ids = [b"id-%d" % i for i in range(12)]
    t = IdTable(ids)
    s = ctx(ids)
    try:
        # cache 0 managed holds rows 3, 7 and the pseudo-entry; cache 1 holds rows 5, 9; cache 2 is empty
        ubm = np.zeros(3, dtype=_lib.UBM_STATE)
        ubm["reserved"] = [50, -1, -1]
        ubm["total_occupancy"] = [20, 0, 0]
        s.load_caches_keyed_k([0, 3, 5, 5], [NOW - 9, NOW - 8, np.iinfo(np.int64).max, NOW - 7, NOW - 6], [10, 10, 50, 4, 4],
                              [ids[3], ids[7], b"", ids[5], ids[9]], [500, 500, 500], ubm, is_unloadbuf=[0, 0, 1, 0, 0])
        live = [[3, 7, UB], [5, 9], []]
        reg, caches = _registry_bytes(s), snapshot(s, 3)
        # a row that is a live key is refused, the lowest one named, nothing changed
        with pytest.raises(Refused) as me:
            IdTable(ids).retire([11, 9, 0, 5], live)
        with pytest.raises(MmpError) as e:
            s.models_retire([11, 9, 0, 5])
        assert code_of(e) == _lib.MMP_EINVAL and me.value.index == 5 and "row 5 " in str(e.value)
        assert _registry_bytes(s) == reg and snapshot(s, 3) == caches and s.n_models == 12
        # below, between and above the keys
        remap = s.models_retire([0, 4, 6, 11, 4])
        assert list(remap) == t.retire([0, 4, 6, 11, 4], live)
        for c in range(3):
            st = s.cache_read_k(c)
            assert list(st["row"]) == IdTable.renumber(live[c], list(remap))
            assert st["ids"] == [b"" if k == UB else ids[k] for k in live[c]]   # the ids are unchanged, the pseudo-entry keeps its key
        live = [IdTable.renumber(k, list(remap)) for k in live]
        # the next keyed replays equal the model.  A replay writes the other of the two layouts: after this read-only one the
        # layout the retirement renumbered keeps id-9's row in cache 1's second slot ...
        outs, _, _, _, krow = s.cache_replay_k(np.array([cop(1, _lib.COP_GET)], dtype=_lib.CACHE_OP), [ids[5]], NOW)
        assert (outs[0]["result"], krow[0]) == (1, t.resolve(ids[5])[1])
        # ... and the one that removes id-9's entry by id writes one entry in front of it: the stale slot lies behind n[c]
        outs, ev, evids, status, krow = s.cache_replay_k(np.array([cop(1, _lib.COP_REMOVE), cop(0, _lib.COP_GET)], dtype=_lib.CACHE_OP),
                                                         [ids[9], ids[7]], NOW)
        assert list(outs["result"]) == [1, 1] and list(krow) == [t.resolve(ids[9])[1], t.resolve(ids[7])[1]]
        r9 = t.resolve(ids[9])[1]
        live[1].remove(r9)
        remap2 = s.models_retire([r9])                                           # the same row, retired once the entry is gone
        assert list(remap2) == t.retire([r9], live)
        assert list(s.cache_read_k(1)["row"]) == [remap2[live[1][0]]] and s.cache_read_k(1)["ids"] == [ids[5]]
        assert s.model_ids_resolve([ids[9]])[0] == -1
    finally:
        s.close()


@pytest.mark.parametrize("shape", ["no caches", "one empty cache", "2046 entries"])
def test_retirement_over_context_shapes(shape):
    n = 2046
    ids = [b"m%d" % i for i in range(n + 10)]
    s = ctx(ids)
    try:
        if shape == "one empty cache":
            s.load_caches_keyed_k([0, 0], [], [], [], [100])
        if shape == "2046 entries":
            rows = np.arange(5, n + 5)
            s.load_caches_keyed_k([0, n], NOW - n + np.arange(n), np.ones(n, np.int32), [ids[r] for r in rows], [10**9])
        remap = s.models_retire([0, 3, n + 7])
        want = IdTable(ids).retire([0, 3, n + 7], [[]])
        assert list(remap) == want and s.n_models == n + 7
        if shape == "2046 entries":
            st = s.cache_read_k(0, max_entries=n)
            assert list(st["row"]) == [want[r] for r in rows] and st["ids"] == [ids[r] for r in rows]
            with pytest.raises(MmpError) as e:
                s.models_retire([n + 2, int(want[rows[-1]]), int(want[rows[0]])])
            assert code_of(e) == _lib.MMP_EINVAL and "row %d " % want[rows[0]] in str(e.value)
    finally:
        s.close()


def test_unbound_caches_are_not_touched_by_a_retirement():
    ids = [b"u%d" % i for i in range(8)]
    s, s0 = ctx(ids), ctx(ids)
    try:
        s.load_caches_keyed([0, 2], [NOW - 2, NOW - 1], [1, 1], [5, 2], [100], None)  # the host's own keys: row 2 may be retired
        before = snapshot(s, 1)
        assert list(s.models_retire([2, 6])) == list(s0.models_retire([2, 6]))
        assert snapshot(s, 1) == before and _registry_bytes(s) == _registry_bytes(s0)
    finally:
        s.close()
        s0.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

def test_refusals_change_nothing():
    s, _ = _small()
    try:
        L, C = s.lib, _lib.C
        good = np.array([cop(0, _lib.COP_GET), cop(1, _lib.COP_PUT_IF_ABSENT, 3, NOW - 1)], dtype=_lib.CACHE_OP)
        gk = [b"a", b"spare"]
        state, reg = snapshot(s, 2), _registry_bytes(s)

        def raw(ops, keys, **kw):
            try:
                s.cache_replay_k_raw(np.array(ops, dtype=_lib.CACHE_OP), keys, NOW, 64, **kw)
            except MmpError as e:
                return e.code
            return 0

        blob, off = Solver.pack_keys(gk)
        E = _lib.MMP_EINVAL
        assert raw([cop(2, _lib.COP_GET)], [b"a"]) == E                                      # what mmp_cache_replay refuses
        assert raw([cop(0, 13)], [b"a"]) == E and raw([cop(-1, _lib.COP_GET)], [b"a"]) == E
        assert raw(good, gk, max_evicted=1) == E                                              # evicted_rows too small
        assert raw(good, None, blob=blob, key_off=np.array([0, 3, 1], np.int32)) == E         # offsets not monotone
        assert raw([cop(0, _lib.COP_GET, reserved=2)], [b"a"]) == E and raw([cop(0, _lib.COP_GET, reserved=-1)], [b"a"]) == E
        assert raw([cop(0, _lib.COP_GET, key=3, reserved=1)], [b"a"]) == E                    # a raw key that is not the pseudo-entry's
        used, need = C.c_int32(0), C.c_int32(0)
        outs = np.zeros(2, dtype=_lib.CACHE_OP_OUT)
        ev = np.zeros(16, np.int32)
        p = _lib.ptr
        assert L.mmp_cache_replay_k(s.h, p(good), 2, blob, None, NOW, None, None, p(outs), p(ev), 16, C.byref(used), None, 0, None,
                                    C.byref(need)) == E                                        # keys without key_off
        assert L.mmp_cache_replay_k(s.h, p(good), 2, None, p(off), NOW, None, None, p(outs), p(ev), 16, C.byref(used), None, 0, None,
                                    C.byref(need)) == E                                        # and the reverse
        assert L.mmp_cache_replay_k(s.h, p(good), 2, blob, p(off), NOW, None, None, None, p(ev), 16, C.byref(used), None, 0, None,
                                    C.byref(need)) == E                                        # NULL outs
        # a load with an unknown id: the lowest entry named, the caches loaded before stay
        with pytest.raises(MmpError) as e:
            s.load_caches_keyed_k([0, 3], [1, 2, 3], [1, 1, 1], [b"a", b"x", b"y"], [10])
        assert code_of(e) == E and "entry 1 " in str(e.value)
        with pytest.raises(MmpError) as e:
            s.load_caches_keyed_k([0, 1], [1], [1], None, [10], blob=b"ab", key_off=np.array([2, 1], np.int32))
        assert code_of(e) == E
        assert snapshot(s, 2) == state and _registry_bytes(s) == reg
        outs_ok, _, _, st_ok, _ = s.cache_replay_k(good, gk, NOW)                              # still bound, still working
        assert list(outs_ok["result"]) == [1, 1] and not st_ok.any()
    finally:
        s.close()


def _estate(s):
    codes = []
    for call in (lambda: s.cache_replay_k(np.array([cop(0, _lib.COP_GET)], dtype=_lib.CACHE_OP), [b"a"], NOW),
                 lambda: s.cache_read_k(0), lambda: s.cache_evicted_ids()):
        with pytest.raises(MmpError) as e:
            call()
        codes.append(code_of(e))
    return codes


def test_estate_for_unbound_caches_after_an_id_load_and_after_a_resize_by_index():
    s, _ = _small()
    try:
        state = snapshot(s, 2)
        s.model_ids_load(IDS5)                                   # the binding goes, the contents stay
        assert _estate(s) == [_lib.MMP_ESTATE] * 3 and snapshot(s, 2) == state
        s.load_caches_keyed_k([0, 1], [NOW], [1], [b"a"], [10])  # ... until the next keyed load
        assert list(s.cache_read_k(0)["row"]) == [0]
        s.load_caches_keyed([0, 1], [NOW], [1], [0], [10], None)  # unbound
        assert _estate(s) == [_lib.MMP_ESTATE] * 3
        assert list(s.cache_read(0)["key"]) == [0]               # the plain calls go on
        s.load_caches_keyed_k([0, 1], [NOW], [1], [b"a"], [10])
        s.load_models(np.zeros(3, _lib.MODEL_ROW), np.zeros(0, np.int32), np.zeros(0, np.int64))  # resized by index
        assert _estate(s) == [_lib.MMP_ESTATE] * 3
        with pytest.raises(MmpError) as e:
            s.load_caches_keyed_k([0, 1], [NOW], [1], [b"a"], [10])
        assert code_of(e) == _lib.MMP_ESTATE
    finally:
        s.close()


# ---- the loop by id, beside a writer, determinism -----------------------------------------------------------------------------------

def test_evictions_go_straight_into_deregister_ops_by_id():
    from tests.registry_ops_model import op_row, ops_array
    from tests.test_registry_ops_keyed_gpu import IDS, loaded, row_world
    fleet, k, _ = row_world()
    now = int(fleet.now)
    s1, s2 = loaded(fleet, IDS), loaded(fleet, IDS)
    try:
        held = [r for r in range(len(IDS)) if fleet.models["n_loaded"][r] > 0][:6]
        assert len(held) == 6
        pods = [int(fleet.ent_pod[fleet.models["ent_off"][r]]) for r in held]
        n = len(held)
        lu, wt = NOW - 100 + np.arange(n), np.full(n, 10, np.int32)
        s1.load_caches_keyed_k([0, n], lu, wt, [IDS[r] for r in held], [10 * n])
        s2.load_caches_keyed([0, n], lu, wt, held, [10 * n], None)
        spare = next(r for r in range(len(IDS)) if r not in held and fleet.models["last_used"][r] != 0)
        put = np.array([cop(0, _lib.COP_PUT_IF_ABSENT, 35, NOW, key=spare)], dtype=_lib.CACHE_OP)
        outs, ev, ev_ids, _, _ = s1.cache_replay_k(put, [IDS[spare]], NOW)
        victims = ev_of(outs, ev, 0)
        vids = ev_ids[outs[0]["evicted_off"]: outs[0]["evicted_off"] + outs[0]["n_evicted"]]
        assert victims == held[:4] and vids == [IDS[r] for r in victims]
        dereg = ops_array([op_row(0, pods[i], _lib.ROP_DEREGISTER, last_used=now - 5) for i in range(len(victims))])
        idx1, st1, ed1, info1 = s1.registry_ops_k(dereg, vids, now)       # no row on the host in between
        outs2, ev2 = s2.cache_replay(put, NOW)
        by_row = dereg.copy()
        by_row["model"] = ev_of(outs2, ev2, 0)
        idx2, st2, ed2, info2 = s2.registry_ops_k(by_row, None, now)
        assert list(idx1) == victims and st1.tobytes() == st2.tobytes() and ed1.tobytes() == ed2.tobytes() and len(ed1) == 4
        assert [x.tobytes() for x in s1.get_models()] == [x.tobytes() for x in s2.get_models()]
    finally:
        s1.close()
        s2.close()


def test_keyed_replays_beside_a_writer_that_joins_new_ids():
    """200 keyed replays on one thread while models_events_json with MMP_MEV_APPEND joins new ids on another: rows only join at the
    end, so every answer is the model's."""
    ids = [b"w%d" % i for i in range(20)]
    t = IdTable(ids)
    s = ctx(ids)
    try:
        s.load_caches_keyed_k([0, 0], [], [], [], [40])
        h = ob.CCache(40, None, NOW)
        errors = []

        def writer():
            try:
                for i in range(40):
                    s.models_events_json([b"joined-%d" % i], ['{"type":"t","lastUsed":1}'], None, append=True)
            except Exception as ex:  # noqa: BLE001
                errors.append(ex)

        th = threading.Thread(target=writer)
        th.start()
        try:
            rng = np.random.default_rng(3)
            for i in range(200):
                key = ids[int(rng.integers(0, 20))] if rng.random() < 0.9 else b"never-%d" % i
                code = int(rng.choice([_lib.COP_PUT_IF_ABSENT, _lib.COP_GET, _lib.COP_REMOVE]))
                ops = np.array([cop(0, code, 10, NOW - 1000 + i)], dtype=_lib.CACHE_OP)
                want, (wrows, wids) = t.replay([h], ops, [key], NOW)
                outs, ev, evids, status, krow = s.cache_replay_k(ops, [key], NOW)
                assert (outs[0]["result"], status[0], krow[0], ev_of(outs, ev, 0)) == \
                    (want[0]["result"], want[0]["status"], want[0]["key"], want[0]["evicted_rows"]), i
                assert list(ev) == wrows and evids == wids, i
        finally:
            th.join()  # the writer is inside the context: it ends before the context may be closed, whatever failed above
        assert not errors and s.model_ids_resolve([b"joined-39"])[0] >= 20
        assert list(s.cache_read_k(0)["row"]) == list(h.nodes()[2])
    finally:
        s.close()


def test_two_runs_over_the_same_state_are_byte_identical():
    runs = []
    for _ in range(2):
        rng, managed, caches = _world(31337)
        R = Renamer(9, 4000)
        ops_res.clear()
        ops = _random_ops(rng, caches, managed, 300, 0)
        ops_res.clear()
        keyed, keys, _ = _keyed_ops(R, ops)
        s1, s2 = _two_contexts(R, _world(31337)[2])
        try:
            r = s1.cache_replay_k_raw(keyed, keys, NOW, 1 << 16, fill=0x11)
            reads = [s1.cache_read_k(c) for c in range(len(caches))]
            rows_named = sorted({int(x) for st in reads for x in st["row"] if x >= 0})
            free = [x for x in range(4000) if x not in rows_named][:50]
            remap = s1.models_retire(free)
            after = [s1.cache_read_k(c) for c in range(len(caches))]
            runs.append(([r[k].tobytes() for k in ("outs", "evicted_rows", "status", "rows", "id_off", "id_bytes")], r["need"],
                         [(st["row"].tobytes(), st["ids"]) for st in reads + after], remap.tobytes()))
        finally:
            s1.close()
            s2.close()
    assert runs[0] == runs[1]
