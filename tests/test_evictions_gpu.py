"""GPU: the eviction record with times (mmp_cache_replay_kt, mmp_cache_evicted_times) against tests/evictions_model.py part (a) and
against mmp_cache_replay_k on a second context.  Every comparison is exact.

Every case of tests/golden/ref_clhm_edges.npz and every stream of tests/golden/ref_clhm.npz goes through mmp_cache_replay_kt with its
keys renamed to ids (as tests/test_cache_keyed_gpu.py renames them): every output mmp_cache_replay_k has is byte-equal to that call's
on a second context, the times are the model's, and mmp_cache_evicted_times returns them — also when the caller passed NULL.

What the vectors hold of the shapes at which the third stack column can go wrong is asserted from their inputs
(test_the_vectors_bring_...).  They do NOT hold an eviction at exactly 48 / 49 and 160 / 161 slots or on the full 2 048-slot tile
(their probe calls at those sizes evict nothing: the capacity there is 10^9), nor a victim whose time is 1 or Long.MAX_VALUE - 1;
those are built by hand below (test_an_eviction_at_the_team_and_tile_edges, test_victims_at_the_ends_of_long)."""
import os

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd.solver import MmpError, Solver
from tests import evictions_model as em
from tests import ref_clhm_cases as rc
from tests.test_cache_keyed_gpu import NAMES, UB, _renamed, _small, code_of, cop, ctx, make_ids

pytestmark = pytest.mark.gpu
NOW = 1_760_000_000_000
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
SAME = ("outs", "evicted_rows", "status", "rows", "id_off", "id_bytes")
I64_MAX = 2**63 - 1


@pytest.fixture(scope="module")
def vec():
    return np.load(os.path.join(GOLDEN, "ref_clhm_edges.npz"))


@pytest.fixture(scope="module")
def streams():
    return np.load(os.path.join(GOLDEN, "ref_clhm.npz"))


def _load_both(s1, s2, caps, reserved):
    seg, lus, wts, k0 = rc.initial_state(caps, reserved)
    ubm = np.zeros(len(caps), dtype=_lib.UBM_STATE)
    ubm["reserved"] = reserved
    for s in (s1, s2):
        s.load_caches_keyed_k(seg, lus, wts, [b"x"] * len(k0), caps, ubm, is_unloadbuf=np.ones(len(k0), np.uint8))


def _kt_against_k_and_the_model(s1, s2, ops, keys, per_op, row_of, cuts, what):
    """s1: mmp_cache_replay_kt, s2: mmp_cache_replay_k, call by call; per_op: model (a) for the whole stream, by vector key.
    Calls alternate between a times buffer and NULL (the context alone keeps them)."""
    for n_call, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        mode = "ctx" if n_call % 2 else "out"
        r1 = s1.cache_replay_k_raw(ops[a:b], keys[a:b], rc.NOW, 1 << 17, fill=0x5A, times=mode)
        r2 = s2.cache_replay_k_raw(ops[a:b], keys[a:b], rc.NOW, 1 << 17, fill=0x5A)
        assert r1["need"] == r2["need"] <= 1 << 17, what
        for f in SAME:
            assert r1[f].tobytes() == r2[f].tobytes(), (what, a, b, f)
        n_slots = len(r1["evicted_rows"])
        want_keys, want_times = em.flat_times(r1["outs"], per_op[a:b], n_slots)
        assert [(-1 if k == -1 else UB if k == UB else row_of[int(k)]) for k in want_keys] == list(r1["evicted_rows"]), (what, a, b)
        kept = s1.cache_evicted_times()
        assert np.array_equal(kept, want_times), (what, a, b)  # an unused slot holds 0 (the buffer was filled with 0x5A)
        if mode == "out":
            assert np.array_equal(r1["last_used"], want_times), (what, a, b)
        assert s1.cache_evicted_ids() == s2.cache_evicted_ids()


@pytest.mark.parametrize("name", NAMES)
def test_every_edge_case_of_the_reference_text_with_times(vec, name):
    v = rc.load_edge_case(vec, name)
    row_of, ids, ops, keys = _renamed(v, 5200 + NAMES.index(name))
    per_op = em.victim_times(v["caps"], v["reserved"], v["ops"], rc.NOW)
    last = len(v["bounds"]) - 1
    for cut_at in ([0, last], list(range(last + 1))):  # one call; cut at every recorded boundary
        s1, s2 = ctx(ids), ctx(ids)
        try:
            _load_both(s1, s2, v["caps"], v["reserved"])
            _kt_against_k_and_the_model(s1, s2, ops, keys, per_op, row_of, [int(v["bounds"][j]) for j in cut_at], name)
        finally:
            s1.close()
            s2.close()


def _rename_stream(ops_in, seed):
    ks = sorted({int(k) for k, o in zip(ops_in["key"], ops_in["op"]) if int(o) not in _lib.COP_KEYLESS and int(k) != UB})
    rng = np.random.default_rng(seed)
    perm = rng.permutation(len(ks) + 5)[: len(ks)]
    row_of = {k: int(r) for k, r in zip(ks, perm)}
    ids = make_ids(rng, len(ks) + 5)
    ops = ops_in.astype(_lib.CACHE_OP)
    keys = []
    for i in range(len(ops)):
        if int(ops[i]["op"]) in _lib.COP_KEYLESS:
            keys.append(b"-")
        else:
            keys.append(ids[row_of[int(ops[i]["key"])]])
            ops[i]["key"] = -4242  # never read
    return row_of, ids, ops, keys


STREAMS = ["kat_basic_eviction", "kat_concurrent_eviction", "kat_standalone_lru", "head_reads"] + [f"stream{k:02d}" for k in range(36)]


def test_the_stream_list_is_the_files(streams):
    assert STREAMS == [str(n) for n in streams["names"]]


@pytest.mark.parametrize("name", STREAMS)
def test_every_stream_of_the_reference_text_with_times(streams, name):
    caps, reserved, ops_in = (streams[f"{name}/{k}"] for k in ("caps", "reserved", "ops"))
    row_of, ids, ops, keys = _rename_stream(ops_in, 77 + STREAMS.index(name))
    per_op = em.victim_times(caps, reserved, ops_in, rc.NOW)
    for pieces in (1, 5):
        s1, s2 = ctx(ids), ctx(ids)
        try:
            _load_both(s1, s2, caps, reserved)
            cuts = [int(x) for x in np.linspace(0, len(ops), pieces + 1).astype(int)]
            _kt_against_k_and_the_model(s1, s2, ops, keys, per_op, row_of, cuts, name)
        finally:
            s1.close()
            s2.close()


def test_the_vectors_bring_the_shapes_the_third_stack_column_can_go_wrong_at(vec):
    """from the inputs and the reference's own answers: probe calls on both sides of both team thresholds and on the full tile (the
    LDS layout of the new instantiations at all three widths and at 64 KiB); among operations that EVICT: all three team widths, one
    operation evicting 1, 2, 63, 64, 65, 129 and 257 entries on a plain and on a managed cache (2 pending is the smallest reversal),
    the cascade, a plain put on a managed cache, the entry that evicts itself, and call cuts at every recorded boundary"""
    occ = {}
    for name in NAMES:
        v = rc.load_edge_case(vec, name)
        occ.update({f"{name}: {k}": x for k, x in rc.edge_occurrence(v, v["tier"], name).items()})
        assert len(v["bounds"]) >= 4, name  # cuts inside the prefix and in front of the probes
    for name in ("lengths_plain", "lengths_managed"):
        for tw, s in ((8, 48), (16, 49), (16, 160), (64, 161)):
            assert occ[f"{name}: {tw} lanes at {s} slots"]
    assert occ["lengths_big: 2047 slots"]
    for N in (1, 2, 63, 64, 65, 129, 257):
        assert occ[f"mass_plain: evict: {N} evicted by one operation"] and occ[f"mass_managed: pending: {N} evicted by one operation"]
        if N >= 2:
            assert occ[f"mass_managed: cascade: {N} evicted by one operation"]
    assert occ["clhm: a put that evicts itself"]
    v = rc.load_edge_case(vec, "mass_managed")
    evicting = v["outs"]["n_evicted"] > 0
    assert ((v["ops"]["op"] == 0) & (v["reserved"][v["ops"]["cache"]] >= 0) & evicting).any()  # a plain put on a managed cache
    widths = set()
    for name in ("mass_plain", "mass_managed"):
        v = rc.load_edge_case(vec, name)
        for r in v["runs"]:  # the probe call of the cut run: the entries the cache holds, the pinned one, one insert
            widths.add(rc.team_width(int(r["entries"]) + int(r["managed"]) + 1))
    assert widths == {8, 16, 64}


def _one_cache(entries, cap, managed, ids):
    """a context with one cache holding `entries` [(id, lastUsed, weight)] in deque order (the pinned entry last when managed)"""
    s = ctx(ids)
    keys = [e[0] for e in entries] + ([b"pinned"] if managed else [])
    lu = [e[1] for e in entries] + ([I64_MAX] if managed else [])
    wt = [e[2] for e in entries] + ([1] if managed else [])
    isu = [0] * len(entries) + ([1] if managed else [])
    ubm = np.zeros(1, dtype=_lib.UBM_STATE)
    ubm["reserved"] = 1 if managed else -1
    ubm["total_occupancy"] = sum(wt[: len(entries)]) if managed else 0
    s.load_caches_keyed_k([0, len(keys)], lu, wt, keys, [cap], ubm, is_unloadbuf=isu)
    return s


@pytest.mark.parametrize("managed", [False, True])
@pytest.mark.parametrize("slots", [48, 49, 160, 161, 2048])
def test_an_eviction_at_the_team_and_tile_edges(slots, managed):
    """one put that evicts three entries on a cache whose replay takes exactly `slots` slots (entries + the pinned one + the insert
    + 1): 8 lanes at 48, 16 at 49 and 160, the wavefront at 161, and the full tile — the 65 536-byte launch — at 2 048.  Managed:
    the three go through the pending stack (a reversal of three)."""
    L = slots - 2 - int(managed)
    ids = [b"m%d" % i for i in range(L + 1)]
    T0 = NOW - 10_000_000
    s = _one_cache([(ids[i], T0 + 7 * i, 10) for i in range(L)], 10 * L + int(managed), managed, ids)
    try:
        assert rc.team_width(slots - 1) == {48: 8, 49: 16, 160: 16, 161: 64, 2048: 64}[slots]
        code = _lib.COP_UBM_INSERT_NEW_ENTRY if managed else _lib.COP_PUT_IF_ABSENT
        outs, ev, ev_ids, _, _, lu = s.cache_replay_kt(np.array([cop(0, code, 21, NOW)], dtype=_lib.CACHE_OP), [ids[L]], NOW, 1 << 16)
        sl = slice(int(outs[0]["evicted_off"]), int(outs[0]["evicted_off"]) + int(outs[0]["n_evicted"]))
        assert list(ev[sl]) == [0, 1, 2] and list(lu[sl]) == [T0, T0 + 7, T0 + 14] and ev_ids[sl] == ids[:3]
        assert len(ev) == slots - 1 and (np.delete(lu, np.arange(sl.start, sl.stop)) == 0).all()
        assert np.array_equal(s.cache_evicted_times(), lu)
    finally:
        s.close()


@pytest.mark.parametrize("managed", [False, True])
def test_victims_at_the_ends_of_long(managed):
    """lastUsed 1 and Long.MAX_VALUE - 1 come back as they are"""
    ids = [b"one", b"mid", b"top", b"new"]
    s = _one_cache([(b"one", 1, 10), (b"mid", NOW, 10), (b"top", I64_MAX - 1, 10)], 30 + int(managed), managed, ids)
    try:
        code = _lib.COP_UBM_INSERT_NEW_ENTRY if managed else _lib.COP_PUT_IF_ABSENT
        outs, ev, _, _, _, lu = s.cache_replay_kt(np.array([cop(0, code, 30, I64_MAX)], dtype=_lib.CACHE_OP), [b"new"], NOW)
        assert list(ev[:3]) == [0, 1, 2] and list(lu[:3]) == [1, NOW, I64_MAX - 1] and lu[3] == 0
    finally:
        s.close()


@pytest.mark.parametrize("stamp,want", [(NOW - 99, NOW - 99), (NOW - 500, NOW - 400), (0, NOW), (-1, NOW - 400)])
def test_an_own_key_victim_after_a_stamped_weight_update_that_evicts_its_own_entry(stamp, want):
    """UpdateTask stamps before it evicts (clhm :646-647): newer keeps the stamp, older keeps lastUsed (max, :1358), 0 is now, quiet
    leaves it.  A weight of 31 cannot stay in a cache of 30 whatever else leaves first."""
    s, _ = _small(managed=False)
    try:
        s.load_caches_keyed_k([0, 3], [NOW - 400, NOW - 300, NOW - 200], [10, 10, 10], [b"a", b"bb", b"gone"], [30])
        ops = np.array([cop(0, _lib.COP_UPDATE_WEIGHT, 31, stamp)], dtype=_lib.CACHE_OP)
        outs, ev, ev_ids, _, _, lu = s.cache_replay_kt(ops, [b"a"], NOW)
        got = dict(zip(ev_ids[: outs[0]["n_evicted"]], (int(x) for x in lu)))
        assert got[b"a"] == want
        assert all(got[k] == t for k, t in ((b"bb", NOW - 300), (b"gone", NOW - 200)) if k in got)
        model = em.victim_times(np.array([30]), np.array([-1]), np.array(
            [(0, 0, 1, 10, NOW - 400, 0, 0), (0, 0, 2, 10, NOW - 300, 0, 0), (0, 0, 3, 10, NOW - 200, 0, 0), (0, 2, 1, 31, stamp, 0, 0)],
            dtype=rc.CACHE_OP), NOW)[3]
        assert [t for _, t in model] == [int(x) for x in lu[: len(model)]]
    finally:
        s.close()


def test_an_inserting_op_under_an_unknown_id_writes_no_time_and_an_unused_slot_holds_0():
    s, _ = _small()
    try:
        ops = np.array([cop(0, _lib.COP_UBM_INSERT_NEW_ENTRY, 5000, NOW)], dtype=_lib.CACHE_OP)
        r = s.cache_replay_k_raw(ops, [b"nobody"], NOW, 64, fill=0x5A, times="out")
        assert r["status"][0] == _lib.CKEY_UNKNOWN and r["outs"][0]["n_evicted"] == 0
        assert len(r["last_used"]) > 0 and (r["last_used"] == 0).all() and (r["evicted_rows"] == -1).all()
        assert (s.cache_evicted_times() == 0).all() and len(s.cache_evicted_times()) == len(r["last_used"])
    finally:
        s.close()


def test_evicted_times_answers_estate_when_the_last_replay_recorded_none():
    s, _ = _small(managed=False)
    try:
        def estate():
            with pytest.raises(MmpError) as e:
                s.cache_evicted_times()
            return code_of(e) == _lib.MMP_ESTATE
        get = np.array([cop(0, _lib.COP_GET)], dtype=_lib.CACHE_OP)
        assert estate()                                              # no replay yet
        s.cache_replay_kt(get, [b"a"], NOW)
        assert len(s.cache_evicted_times()) == len(s.cache_evicted_ids())
        s.cache_replay_k(get, [b"a"], NOW)                           # a plain keyed replay records none
        assert estate()
        s.cache_replay_kt(np.zeros(0, dtype=_lib.CACHE_OP), [], NOW)  # n_ops == 0: the empty record, with times
        assert len(s.cache_evicted_times()) == 0
        s.cache_replay_kt(get, [b"a"], NOW)
        s.load_caches_keyed_k([0, 1], [NOW], [1], [b"a"], [10])     # a cache load ends the record
        assert estate()
    finally:
        s.close()


# ======================================================== mmp_evictions_k ========================================================
# against tests/evictions_model.py part (b), and against the composition it replaces on a second context in the same state:
# mmp_registry_ops_k with the ops spelled out (status, edits, registry byte-equal) and mmp_gate_batch with loaded_time from the model
# (MMP_GATE_RELOAD_ELSEWHERE; times >= 0 only, where the gate's -1 convention is unambiguous).

import copy  # noqa: E402
import threading  # noqa: E402

from modelmesh_amd import workload as wl  # noqa: E402
from modelmesh_amd._lib import ROPS_APPLY, ROPS_DRY  # noqa: E402
from oracle import bind as ob  # noqa: E402
from tests import registry_ops_model as ro  # noqa: E402
from tests import registry_prune_model as rp  # noqa: E402
from tests import test_registry_ops_keyed_gpu as rg  # noqa: E402
from tests.registry_ops_keyed_model import KeyedRegistry  # noqa: E402
from tests.registry_ops_model import ModelRecord, op_row, ops_array  # noqa: E402

EV_FILL = 0xA5
GATE_ENTRY_FAILED = 16
WORLDS = {"rows": (0, rg.P, rg.M), "8": (21, 8, 400), "64": (22, 64, 400), "65": (23, 65, 400)}


@pytest.fixture(scope="module")
def worlds():
    out = {}
    for name, (seed, pods, models) in WORLDS.items():
        fleet, k, rng = rg.row_world(seed, pods, models)
        out[name] = (fleet, k, ob.type_set_stats(fleet))
    return out


def draw_victims(k, fleet, rng, n, self_pod):
    """n victims on distinct live records (as far as they go) plus unknown and deleted ids: load times equal to / one off the
    registered ones, failed entries, last_used around the record's; and a load timeout that splits the registered times"""
    now = int(fleet.now)
    live = [key for key in k.ids if k.get(key) is not None]
    dead = [key for key in k.ids if k.get(key) is None]
    mine = [key for key in live if self_pod in k.get(key).instance_ids or self_pod in k.get(key).load_failed_instance_ids]
    rest = [key for key in live if key not in mine]
    keys = (mine + [rest[i] for i in rng.permutation(len(rest))])[: max(n - 3, 0)] + dead[:1] + [b"never-seen", b"never-seen"]
    keys = [keys[i] for i in rng.permutation(len(keys))][:n]
    while len(keys) < n:
        keys.append(b"unknown-%d" % len(keys))
    entries = np.zeros(n, dtype=_lib.EVICTED_ENTRY)
    ages = []
    for i, key in enumerate(keys):
        mr = k.get(key)
        lt = lct = int(rng.integers(0, 5))
        lu = int(rng.choice([0, 1, now - 50, now, now + 9]))
        if mr is not None:
            lt = mr.instance_ids.get(self_pod, lt) + int(rng.choice([0, 0, 0, 1, -1]))
            lct = mr.load_failed_instance_ids.get(self_pod, lct) + int(rng.choice([0, 0, 1]))
            lu = int(rng.choice([lu, mr.last_used, mr.last_used + 1, mr.last_used - 1]))
            ages += [now - t for t in (mr.instance_ids.get(self_pod), mr.load_failed_instance_ids.get(self_pod)) if t is not None]
        entries[i] = tuple(em.jsub(x, 0) for x in (lu, lt, lct)) + (int(rng.integers(1, 9000)), int(rng.random() < 0.2))  # (as Java longs)
    timeout = int(np.median(ages)) // 2 if ages else 30_000
    return entries, keys, timeout


def spelled_out(entries, self_pod):
    return ops_array([op_row(-1, self_pod, _lib.ROP_DEREGISTER, flags=_lib.ROPF_MATCH_TIME, last_used=int(e["last_used"]),
                             load_time=int(e["load_time"]), load_complete_time=int(e["load_complete_time"])) for e in entries])


def same_as_model_b(got, want, what=""):
    (idx, outs, st, ed, info), (widx, wouts, wst, wed, winfo) = got, want
    assert np.array_equal(idx, widx), what
    assert outs.tobytes() == wouts.tobytes(), (what, outs[:6], wouts[:6])
    assert np.array_equal(st, wst) and ed.tobytes() == wed.tobytes(), what
    for f in ("n_in_registry", "n_attempt_reload", "n_reload", "n_log", "n_no_record"):
        assert int(info[f]) == winfo[f], (what, f)
    rg.same_as_model((idx, st, ed, info["ops"]), (widx, wst, wed, winfo["ops"]), what)


def check_against_both(s1, s2, k, fleet, stats, entries, keys, self_pod, timeout, apply=True):
    now = int(fleet.now)
    before = copy.deepcopy(k)
    want = em.evictions_run(k, entries, keys, self_pod, now, timeout, stats, dry=not apply)
    got = s1.evictions_k(entries, keys, self_pod, now, timeout, apply=apply)
    same_as_model_b(got, want)
    rg.same_registry(s1, k)
    # the composition, on the second context
    ops = spelled_out(entries, self_pod)
    idx2, st2, ed2, info2 = s2.registry_ops_k(ops, keys, now, apply=apply)
    assert np.array_equal(idx2, got[0]) and st2.tobytes() == got[2].tobytes() and ed2.tobytes() == got[3].tobytes()
    assert info2.tobytes() == got[4]["ops"].tobytes()
    rg.same_contexts(s1, s2)
    outs = want[1]
    ask = [i for i in range(len(keys)) if before.get(keys[i]) is not None and (int(outs[i]["loaded_time"]) >= 0 or entries[i]["flags"])]
    if ask:
        reqs = np.zeros(len(ask), dtype=_lib.GATE_REQ)
        reqs["model"] = [before.row(keys[i]) for i in ask]
        reqs["self_pod"] = self_pod
        reqs["flags"] = [GATE_ENTRY_FAILED if entries[i]["flags"] else 0 for i in ask]
        reqs["loaded_time"] = [int(outs[i]["loaded_time"]) for i in ask]
        reqs["load_timeout_ms"] = timeout
        # (the registry the gate reads has been edited by the apply above; the reload rule reads the record's type and the stats only)
        bits = s2.gates(reqs, [], [], [], now)["bits"]
        assert [bool(b & _lib.GATE_RELOAD_ELSEWHERE) for b in bits] == [bool(outs[i]["flags"] & _lib.EVO_RELOAD) for i in ask]
    return got


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
@pytest.mark.parametrize("world", list(WORLDS))
def test_evictions_k_equals_the_model_and_the_composition(worlds, world, n):
    fleet, k0, stats = worlds[world]
    k = copy.deepcopy(k0)
    P = len(k.id_order)
    rng = np.random.default_rng(1000 * n + P)
    self_pod = int(rng.integers(0, P))
    entries, keys, timeout = draw_victims(k, fleet, rng, n, self_pod)
    s1, s2 = rg.loaded(fleet, k.ids), rg.loaded(fleet, k.ids)
    try:
        for flags in (0, ROPS_DRY):   # change nothing
            want = em.evictions_run(k, entries, keys, self_pod, int(fleet.now), timeout, stats, dry=True)
            r = s1.evictions_k_raw(entries, keys, self_pod, int(fleet.now), timeout, flags, max(n, 1))
            assert r[5] == 0
            same_as_model_b(r[:5], want, flags)
            rg.same_registry(s1, k)
        got = check_against_both(s1, s2, k, fleet, stats, entries, keys, self_pod, timeout)
        if n >= 63 and world in ("rows", "8"):
            f = got[1]["flags"]
            assert all((f & b).any() for b in (1, 2, 4, 8)), f   # every flag occurs
            assert len(got[3]) > 0 and (got[2] == _lib.ROP_NO_RECORD).any() and (got[2] == _lib.ROP_UNCHANGED).any()
    finally:
        s1.close()
        s2.close()


@pytest.mark.parametrize("copies", [1, 63, 64, 65, 1025])
def test_rows_of_many_copies_with_self_pod_first_last_and_absent(copies):
    Pn = 1100
    fleet = wl.fuzz_fleet(77, pods=Pn, models=8)
    order = np.argsort(fleet.pods["id_order"])                      # TreeMap order of the instance ids
    now = int(fleet.now)
    old = now - 10_000_000
    recs, cases = [], []
    for where in ("first", "last", "absent"):
        for lst in ("loaded", "failed"):
            pods = [int(p) for p in order[:copies + 1]]
            self_pod = {"first": pods[0], "last": pods[-2], "absent": pods[-1]}[where]
            ents = [(p, old + j) for j, p in enumerate(pods[:-1])]
            recs.append(ModelRecord(0, ents if lst == "loaded" else [], ents if lst == "failed" else [], 5))
            cases.append((where, lst, self_pod))
    ids = [b"r%d" % i for i in range(len(recs))]
    fleet.models, fleet.ent_pod, fleet.ent_time = ro.registry_to_arrays(recs)
    stats = ob.type_set_stats(fleet)
    # one self_pod per call: the six records are asked in three calls of two
    s1, s2 = rg.loaded(fleet, ids), rg.loaded(fleet, ids)
    k = KeyedRegistry(ids, recs, fleet.pods["id_order"].copy())
    try:
        for j in range(0, 6, 2):
            (where, _, self_pod), keys = cases[j], ids[j:j + 2]
            entries = np.zeros(2, dtype=_lib.EVICTED_ENTRY)
            for q, key in enumerate(keys):
                mr = k.get(key)
                entries[q] = (now - 3, mr.instance_ids.get(self_pod, 0), mr.load_failed_instance_ids.get(self_pod, 0), 10, 0)
            got = check_against_both(s1, s2, k, fleet, stats, entries, keys, self_pod, 1000)
            if where == "absent":
                assert (got[1]["flags"] == 0).all() and (got[2] == _lib.ROP_UNCHANGED).all()
            else:
                assert (got[1]["flags"] & 3 == 3).all() and (got[2] == _lib.ROP_EDITED).all()
                assert list(got[1]["loaded_time"]) == [old + (0 if where == "first" else copies - 1)] * 2
    finally:
        s1.close()
        s2.close()


def test_every_by_hand_boundary_of_the_model_on_the_device():
    """the records of tests/test_evictions_model.py's boundaries as one registry: the time rule at 2 * timeout / + 1, both lists
    (the first wins), a failed entry, MATCH_TIME one off on either list, a wrapped now - last_used"""
    fleet = wl.fuzz_fleet(78, pods=8, models=4)
    now, T, me = int(fleet.now), 30_000, 1
    old, new = now - 10 * T, now - 5
    rows = [
        (ModelRecord(0, [(me, now - 2 * T)], [], 5), (now - 10, now - 2 * T, 0, 1, 0)),
        (ModelRecord(0, [(me, now - 2 * T - 1)], [], 5), (now - 10, now - 2 * T - 1, 0, 1, 0)),
        (ModelRecord(0, [], [(me, old)], 5), (now - 10, 0, old, 1, 0)),
        (ModelRecord(0, [(me, new)], [(me, old)], 5), (now - 10, new, old, 1, 0)),
        (ModelRecord(0, [(me, old)], [(me, new)], 5), (now - 10, old + 1, new - 1, 1, 0)),
        (ModelRecord(0, [(0, old)], [(2, old)], 5), (now - 10, old, old, 1, 0)),
        (ModelRecord(0, [(me, old), (0, 7)], [], 5), (now - 10, old, 0, 1, _lib.EVF_FAILED)),
        (ModelRecord(0, [(me, old)], [], 5), (-(2**63), old, 0, 1, 0)),
        (ModelRecord(0, [(me, now + 10 * T)], [], 5), (now + 77, 0, 0, 1, 0)),
        (ModelRecord(0, [], [], 0), (now, 0, 0, 1, _lib.EVF_FAILED)),                  # the empty row
    ]
    recs = [r for r, _ in rows]
    ids = [b"h%d" % i for i in range(len(rows))]
    fleet.models, fleet.ent_pod, fleet.ent_time = ro.registry_to_arrays(recs)
    entries = np.array([e for _, e in rows], dtype=_lib.EVICTED_ENTRY)
    k = KeyedRegistry(ids, recs, fleet.pods["id_order"].copy())
    s1, s2 = rg.loaded(fleet, ids), rg.loaded(fleet, ids)
    try:
        got = check_against_both(s1, s2, k, fleet, ob.type_set_stats(fleet), entries, ids, me, T)
        f = got[1]["flags"]
        assert not f[0] & 2 and f[1] & 2 and f[2] & 3 == 3 and f[3] & 3 == 1 and f[4] & 3 == 3 and f[5] == 0 and f[6] == 8 and f[9] == 0
        assert list(got[2]) == [1, 1, 1, 1, 0, 0, 1, 1, 0, 2]
        assert got[1]["millis_since_last_used"][7] == now - 2**63 and got[1]["millis_since_last_used"][8] == -77
    finally:
        s1.close()
        s2.close()


def test_truncation_and_every_refusal_leave_the_registry_and_the_id_map_clean(worlds):
    fleet, k0, stats = worlds["rows"]
    k, now = copy.deepcopy(k0), int(fleet.now)
    rng = np.random.default_rng(5)
    self_pod = 3
    entries, keys, timeout = draw_victims(k, fleet, rng, 200, self_pod)
    s = rg.loaded(fleet, k.ids)
    try:
        want = em.evictions_run(k, entries, keys, self_pod, now, timeout, stats, dry=True)
        assert len(want[3]) > 5
        for flags in (ROPS_APPLY, 0):
            for cap in (3, len(want[3]) - 1, 0):     # the prefix and the totals; nothing applied
                idx, outs, st, ed, info, rc = s.evictions_k_raw(entries, keys, self_pod, now, timeout, flags, cap)
                assert rc == 0 and int(info["ops"]["truncated"]) == 1 and ed.tobytes() == want[3][:cap].tobytes()
                assert outs.tobytes() == want[1].tobytes() and np.array_equal(st, want[2])
                rg.same_registry(s, k)
        resident = [a.copy() for a in s.get_models()]
        live = [key for key in k.ids if k.get(key) is not None]
        good = np.zeros(70, dtype=_lib.EVICTED_ENTRY)
        bad_flag = good.copy()
        bad_flag["flags"][69] = 2
        mono = np.arange(71, dtype=np.int32)
        mono[30] = 28
        A0 = dict(entries=good, keys=live[:70], self_pod=self_pod, now=now, flags=ROPS_APPLY, max_edits=128)
        refusals = [("two victims on one live row", dict(keys=live[:69] + [live[7]])), ("self_pod beyond the table", dict(self_pod=rg.P)),
                    ("a negative self_pod", dict(self_pod=-1)), ("an unknown entry flag", dict(entries=bad_flag)), ("now = 0", dict(now=0)),
                    ("APPLY | DRY", dict(flags=ROPS_APPLY | ROPS_DRY)), ("an unknown call flag", dict(flags=4)),
                    ("a negative capacity", dict(max_edits=-1)), ("offsets not monotone", dict(key_off=mono))]
        for what, kw in refusals:
            a = dict(A0, **kw)
            out = s.evictions_k_raw(a["entries"], a["keys"], a["self_pod"], a["now"], timeout, a["flags"], a["max_edits"], fill=EV_FILL,
                                    key_off=a.get("key_off"))
            assert out[5] == _lib.MMP_EINVAL, what
            assert all(set(x.tobytes()) <= {EV_FILL} for x in out[:5]), what
            for x, y in zip(resident, s.get_models()):
                assert x.tobytes() == y.tobytes(), what
        got = s.evictions_k(entries, keys, self_pod, now, timeout, max_edits=2)        # the map was left all -1; the veneer regrows
        same_as_model_b(got, em.evictions_run(k, entries, keys, self_pod, now, timeout, stats))
        rg.same_registry(s, k)
    finally:
        s.close()
    s = Solver(6553, 60_000)                                                          # before the first commit: as mmp_gate_batch
    try:
        assert s.evictions_k_raw(np.zeros(1, dtype=_lib.EVICTED_ENTRY), [b"a"], 0, 1_700_000_000_000, 1, 0, 4)[5] == _lib.MMP_ESTATE
        with pytest.raises(MmpError) as e:
            s.gates(np.zeros(1, dtype=_lib.GATE_REQ), [], [], [], 1_700_000_000_000)
        assert code_of(e) == _lib.MMP_ESTATE
    finally:
        s.close()


# ---- the loop end to end ---------------------------------------------------------------------------------------------------------------

def _loop_world():
    from tests.test_registry_ops_keyed_gpu import IDS
    fleet, k, _ = rg.row_world()
    held = [r for r in range(len(IDS)) if fleet.models["n_loaded"][r] > 0][:6]
    assert len(held) == 6
    return fleet, k, IDS, held


def test_the_eviction_loop_in_two_calls_with_the_records_own_times_and_a_retirement_in_between():
    """the scenario of tests/test_cache_keyed_gpu.py::test_evictions_go_straight_into_deregister_ops_by_id, rebuilt: cache_replay_kt ->
    evictions_k, last_used taken from the record — and it IS the victims' true lastUsed (what the parent could not know) — with an
    unrelated mmp_models_retire between the two calls: the record holds ids and times, not rows"""
    fleet, k, IDS, held = _loop_world()
    now = int(fleet.now)
    stats = ob.type_set_stats(fleet)
    s = rg.loaded(fleet, IDS)
    try:
        self_pod = int(fleet.ent_pod[fleet.models["ent_off"][held[0]]])
        n = len(held)
        lu = NOW - 100 + 7 * np.arange(n)
        s.load_caches_keyed_k([0, n], lu, np.full(n, 10, np.int32), [IDS[r] for r in held], [10 * n])
        spare = next(r for r in range(len(IDS)) if r not in held and fleet.models["last_used"][r] != 0)
        put = np.array([cop(0, _lib.COP_PUT_IF_ABSENT, 35, NOW, key=spare)], dtype=_lib.CACHE_OP)
        outs, ev, ev_ids, _, _, ev_lu = s.cache_replay_kt(put, [IDS[spare]], NOW)
        m = int(outs[0]["n_evicted"])
        assert m == 4 and list(ev[:m]) == held[:4] and ev_ids[:m] == [IDS[r] for r in held[:4]]
        assert list(ev_lu[:m]) == list(lu[:4])                                # the victims' true lastUsed: cannot pass on the parent
        gone = [r for r in (9, 38, 67) if r not in held]                      # the three deleted records' rows, unrelated to the victims
        remap = s.models_retire(gone)
        k.retire(gone)
        assert all(remap[r] != r for r in held if r > min(gone))             # the victims' rows did move
        vids = ev_ids[:m]
        entries = np.zeros(m, dtype=_lib.EVICTED_ENTRY)
        for i, key in enumerate(vids):
            mr = k.get(key)
            entries[i] = (int(ev_lu[i]), mr.instance_ids.get(self_pod, 0), mr.load_failed_instance_ids.get(self_pod, 0), 10, 0)
        want = em.evictions_run(k, entries, vids, self_pod, now, 1000, stats)
        got = s.evictions_k(entries, vids, self_pod, now, 1000)
        same_as_model_b(got, want)
        rg.same_registry(s, k)
        assert (got[2] == _lib.ROP_EDITED).any() and list(got[0]) == [k.row(key) for key in vids]
        assert np.array_equal(s.cache_evicted_times()[:m], lu[:4])            # the record outlives the retirement
    finally:
        s.close()


def test_the_loop_beside_a_writer_that_joins_new_ids():
    """200 iterations of replay_kt -> evictions_k on one thread while models_events_json joins ids on another (rows only join at the
    end, so every answer is the model's)"""
    from tests import test_status_by_id_gpu as sbg
    s, k = rg.key_world(20)
    ids, fleet = list(k.ids), sbg.W.fleet
    stats = ob.type_set_stats(fleet)
    now = 5_000_000
    me = min(range(rg.P), key=lambda p: fleet.pods["id_order"][p])            # in instanceIds of every third record
    joiner = ModelRecord(0, [(1, 5)], [], 3)
    try:
        s.load_caches_keyed_k([0, 0], [], [], [], [20])
        h = ob.CCache(20, None, NOW)
        errors = []

        def writer():
            try:
                for i in range(40):
                    s.models_events_json([b"joined-%d" % i], [sbg.value_of(joiner)], np.zeros(1, np.uint8), True)
            except Exception as ex:  # noqa: BLE001
                errors.append(ex)

        th = threading.Thread(target=writer)
        th.start()
        n_edits = 0
        try:
            rng = np.random.default_rng(4)
            for i in range(200):
                r = int(rng.integers(0, 20))
                t = NOW - 1000 + i
                lu_b, _, key_b = h.nodes()
                before = dict(zip((int(x) for x in key_b), (int(x) for x in lu_b)))
                _, evk = h.apply(0, r, 10, t, 0, NOW)
                outs, ev, evids, _, _, ev_lu = s.cache_replay_kt(np.array([cop(0, _lib.COP_PUT_IF_ABSENT, 10, t)], dtype=_lib.CACHE_OP),
                                                                  [ids[r]], NOW)
                m = int(outs[0]["n_evicted"])
                assert list(ev[:m]) == evk and [int(x) for x in ev_lu[:m]] == [before[v] for v in evk], i
                if not m:
                    continue
                entries = np.zeros(m, dtype=_lib.EVICTED_ENTRY)
                for q, v in enumerate(evk):
                    entries[q] = (int(ev_lu[q]), k.get(ids[v]).instance_ids.get(me, 0), 0, 10, 0)
                got = s.evictions_k(entries, evids[:m], me, now + i, 500)
                same_as_model_b(got, em.evictions_run(k, entries, evids[:m], me, now + i, 500, stats), i)
                n_edits += len(got[3])
        finally:
            th.join()
        assert not errors and s.model_ids_resolve([b"joined-39"])[0] >= 20 and n_edits > 0
        rows = rp.compact(*s.get_models())[0]
        want = ro.registry_to_arrays(k.records_by_row())[0]
        for f in ("n_loaded", "n_failed", "last_used"):
            assert np.array_equal(rows[f][:len(want)], want[f]), f
    finally:
        s.close()
