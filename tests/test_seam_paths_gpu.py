"""GPU: the two paths of the seven host-pointer request calls (mmp_place_batch, _place_batch_c, _serve_batch, _gate_batch,
_miss_batch, _route_batch, _evict_batch) answer alike, and refuse alike.

A call rides a latency slot while every count it brings is within the slot layout table (mmplace.hip, beside FastSlot) and is
staged through device scratch beyond it.  The cases send the same rows down both paths — one row past each request limit against
calls of at most the limit, and four requests whose pool is padded one entry past its capacity against the same four with the pool
trimmed — and require equal output fields.  Which path a call took is read from what the library exposes: after profile(True) a
staged call leaves last_kernel_ms() >= 0, a slot call leaves it negative.  (mmp_miss_batch has no staged path of its own: past its
slot it is mmp_gate_batch + mmp_place_batch, which ride slots of their own for these shapes.)

The refusals are decided on the host, before any state is looked at: MMP_EINVAL on a committed and on an uncommitted context."""
import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd import workload as wl
from modelmesh_amd._lib import MMP_EINVAL, MMP_ESTATE, MMP_OK, ptr
from modelmesh_amd.solver import Solver

pytestmark = pytest.mark.gpu
INT_MAX = 2**31 - 1
# the request limits and pool capacities of the slot layout table
LIMIT = {"place": 4096, "place_c": 4096, "serve": 1024, "gate": 4096 * 64 // 144, "evict": 4096 * 16 // 32}
POOLS = {"place": {"extra": 16384}, "serve": {"counters": 8192, "excl": 4096}, "gate": {"excl": 4096, "explicit": 4096},
         "miss": {"extra": 2048, "excl": 2048, "explicit": 2048}, "route": {"counters": 4096, "excl": 4096, "explicit": 4096}}
OUTS = {"place": ("pouts",), "place_c": ("pouts",), "serve": ("souts",), "gate": ("gouts",), "miss": ("gouts", "pouts"),
        "route": ("gouts", "souts"), "evict": ("eouts",)}
OUT_DTYPE = {"pouts": _lib.PLACE_OUT, "souts": _lib.SERVE_OUT, "gouts": _lib.GATE_OUT, "eouts": _lib.EVICT_OUT}
assert LIMIT["gate"] == 1820 and LIMIT["evict"] == 2048 and _lib.GATE_REQ.itemsize == 144 and _lib.EVICT_OUT.itemsize == 32


@pytest.fixture(scope="module")
def fleet():
    return wl.make_fleet("C1")


@pytest.fixture(scope="module")
def mesh(fleet):
    """a committed context with caches loaded"""
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    s.load_fleet(fleet)
    cs = wl.ChurnStream(fleet, 0xC5)
    s.load_caches(cs.seg_off, cs.cache_lu, cs.cache_wt, cs.cache_cap)
    yield s
    s.close()


@pytest.fixture(scope="module")
def bare(fleet):
    """an uncommitted context without caches (the registry is loaded: serve_counters reads its host mirror)"""
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    s.load_fleet(fleet, commit=False)
    yield s
    s.close()


def _ranges(rng, n, frac):
    """[off, off + cnt) of a pool for each of n requests: none for some, one to three entries for the others (request 0 has two)"""
    cnt = np.where(rng.random(n) < frac, rng.integers(1, 4, n), 0).astype(np.int32)
    if n and frac:
        cnt[0] = 2
    off = np.zeros(n + 1, np.int64)
    np.cumsum(cnt, out=off[1:])
    return off[:-1].astype(np.int32), cnt, int(off[-1])


def make_args(fleet, s, seed, n, pools=True):
    """Consistent arguments of all seven calls for n requests: request i of every call names model i % M from instance i % P.
    pools: about half the requests bring exclusion pairs / explicit members / extras of their own, the others none."""
    rng = np.random.default_rng(seed)
    M, P, now = fleet.n_models, fleet.n_pods, fleet.now
    frac = 0.5 if pools else 0.0
    a = {"n": n, "now": now}
    g = np.zeros(n, dtype=_lib.GATE_REQ)
    g["model"], g["self_pod"] = np.arange(n) % M, np.arange(n) % P
    g["flags"] = rng.integers(0, 512, n)
    g["excl_off"], g["n_excl"], n_excl = _ranges(rng, n, frac)
    g["explicit_off"], g["n_explicit"], n_explicit = _ranges(rng, n, frac)
    g["size_hint"] = rng.integers(0, 20_000, n)
    g["last_used_time"] = now - rng.integers(0, 10_000_000, n)
    g["cache_capacity"] = 8_388_608
    g["cache_weighted_size"] = rng.integers(0, 9_000_000, n)
    g["cache_oldest_time"] = np.where(rng.random(n) < 0.1, -1, now - rng.integers(0, 10_000_000, n))
    g["loader_predicted"], g["loading_count"], g["weight_predict_cutoff"] = rng.integers(0, 20_000, n), rng.integers(0, 13, n), 10
    g["loaded_time"] = np.where(rng.random(n) < 0.3, -1, now - rng.integers(0, 1_000_000, n))
    g["load_timeout_ms"] = 240_000
    sp = fleet.pods[g["self_pod"]]
    g["fresh_lru"], g["fresh_capacity"], g["fresh_used"], g["fresh_count"] = sp["lru_time"], sp["capacity"], sp["used"], sp["count"]
    g["fresh_loading_threads"], g["fresh_in_progress"], g["fresh_rpm"] = 8, rng.integers(0, 3, n), rng.integers(0, 500, n)
    g["last_published"] = now - rng.integers(0, 10_000, n)
    a["greqs"] = g
    a["xp"], a["xt"], a["n_excl"] = rng.integers(0, P, n_excl).astype(np.int32), (now - rng.integers(0, 100_000, n_excl)).astype(np.int64), n_excl
    a["expl"], a["n_explicit"] = rng.integers(0, P, n_explicit).astype(np.int32), n_explicit
    sr = np.zeros(n, dtype=_lib.SERVE_REQ)
    sr["model"], sr["self_pod"] = g["model"], g["self_pod"]
    sr["flags"], sr["local_in_flight"] = rng.integers(0, 4, n), rng.integers(0, 3, n)
    sr["last_invoke_time"], sr["assume_completed_ms"] = now - rng.choice([0, 10, 1000], n), rng.choice([3000, 30_000], n)
    sr["excl_off"], sr["n_excl"] = g["excl_off"], g["n_excl"]  # one MapFilteringSet for both halves of a route
    in_use = rng.integers(0, 3, P).astype(np.int32)
    last_used = (now - rng.choice([0, 5, 5, 100, 10_000], P)).astype(np.int64)
    a["sreqs"], a["counters"] = s.serve_counters(sr, in_use, last_used)
    a["n_counters"] = len(a["counters"])
    pr = wl.make_requests(fleet, seed, n=max(n, 1), extra_frac=0.0)[0][:n].copy()
    assert np.array_equal(pr["model"], g["model"])
    pr["extra_off"], pr["n_extra"], n_extra = _ranges(rng, n, frac)
    a["preqs"], a["extra"], a["n_extra"] = pr, rng.integers(0, P, n_extra).astype(np.int32), n_extra
    one = pr.copy()  # the single-caller form: every row from instance 1
    row = fleet.pods[1]
    one["self_pod"], one["flags"], one["fresh_rpm"] = 1, 0, 0
    one["fresh_lru"], one["fresh_capacity"], one["fresh_used"], one["fresh_count"] = row["lru_time"], row["capacity"], row["used"], row["count"]
    a["caller"], a["creqs"] = _lib.split_caller(one)
    ev = np.zeros(n, dtype=_lib.EVICT_REQ)
    ev["cache"], ev["weight"] = np.arange(n) % P, rng.integers(1, 200_000, n)
    ev["last_used"] = np.where(rng.random(n) < 0.5, 0, now - rng.integers(0, 1_000_000, n))
    a["ereqs"] = ev
    for name, dt in OUT_DTYPE.items():
        a[name] = np.zeros(n, dtype=dt)
    return a


def raw(s, kind, a):
    """The call on the arguments as they stand (an array may be None, a length anything): -> return code."""
    L, h, n, now, p = s.lib, s.h, a["n"], a["now"], lambda k: ptr(a[k]) if a[k] is not None and len(a[k]) else None
    if kind == "place":
        return L.mmp_place_batch(h, p("preqs"), n, p("extra"), a["n_extra"], now, p("pouts"))
    if kind == "place_c":
        return L.mmp_place_batch_c(h, ptr(a["caller"]), p("creqs"), n, p("extra"), a["n_extra"], now, p("pouts"))
    if kind == "serve":
        return L.mmp_serve_batch(h, p("sreqs"), n, p("counters"), a["n_counters"], p("xp"), p("xt"), a["n_excl"], now, p("souts"))
    if kind == "gate":
        return L.mmp_gate_batch(h, p("greqs"), n, p("xp"), p("xt"), a["n_excl"], p("expl"), a["n_explicit"], now, 450_000, p("gouts"))
    if kind == "miss":
        return L.mmp_miss_batch(h, p("greqs"), p("preqs"), n, p("xp"), p("xt"), a["n_excl"], p("expl"), a["n_explicit"], p("extra"),
                                a["n_extra"], now, 450_000, p("gouts"), p("pouts"))
    if kind == "route":
        return L.mmp_route_batch(h, p("greqs"), p("sreqs"), n, p("counters"), a["n_counters"], p("xp"), p("xt"), a["n_excl"], p("expl"),
                                 a["n_explicit"], now, 450_000, p("gouts"), p("souts"))
    assert kind == "evict"
    return L.mmp_evict_batch(h, p("ereqs"), n, now, p("eouts"))


ROWS = ("greqs", "sreqs", "preqs", "creqs", "ereqs") + tuple(OUT_DTYPE)


def run(s, kind, a, lo, hi, staged):
    """Rows [lo, hi) of `a` in one call, with the whole pools; proves the path it took.  -> {output name: rows}"""
    b = dict(a)
    for k in ROWS:
        b[k] = np.ascontiguousarray(a[k][lo:hi]).copy()
    b["n"] = hi - lo
    s.profile(True)
    assert raw(s, kind, b) == MMP_OK, (kind, lo, hi, s.lib.mmp_last_error(s.h))
    ms = s.last_kernel_ms()
    assert (ms >= 0) if staged else (ms < 0), (kind, lo, hi, "staged" if staged else "slot", ms)
    return {k: b[k] for k in OUTS[kind]}


def assert_same(kind, got, want, what):
    for k in OUTS[kind]:
        for f in OUT_DTYPE[k].names:
            if f != "pad":
                assert np.array_equal(got[k][f], want[k][f]), (kind, what, k, f, np.nonzero(got[k][f] != want[k][f])[0][:5])


@pytest.mark.parametrize("kind", ["place", "place_c", "gate", "serve", "evict"])
def test_one_row_past_the_slot_equals_slot_sized_calls(fleet, mesh, kind):
    n = LIMIT[kind] + 1
    a = make_args(fleet, mesh, 11, n)
    for pool, cap in POOLS.get("place" if kind == "place_c" else kind, {}).items():
        assert a["n_" + pool] <= cap, (kind, pool)  # the pools fit a slot: the row count alone decides the path
    for rep, cut in enumerate((n - 1, 1, n // 2)):  # (the slots are reused: sequence numbers, rows of the call before)
        whole = run(mesh, kind, a, 0, n, staged=True)
        parts = [run(mesh, kind, a, 0, cut, staged=False), run(mesh, kind, a, cut, n, staged=False)]
        assert_same(kind, {k: np.concatenate([p[k] for p in parts]) for k in OUTS[kind]}, whole, (rep, cut))


@pytest.mark.parametrize("kind,pool", [(k, p) for k, ps in POOLS.items() for p in ps])
def test_a_pool_one_entry_past_the_slot_equals_the_trimmed_pool(fleet, mesh, kind, pool):
    a = make_args(fleet, mesh, 23, 4)
    assert a["n_excl"] and a["n_explicit"] and a["n_extra"] and a["n_counters"]
    b = dict(a)
    arrays = {"extra": ("extra",), "counters": ("counters",), "excl": ("xp", "xt"), "explicit": ("expl",)}[pool]
    cap = POOLS[kind][pool]
    for k in arrays:  # entries no request references
        pad = np.zeros(cap + 1 - len(a[k]), dtype=a[k].dtype)
        b[k] = np.concatenate([a[k], pad])
    b["n_" + pool] = cap + 1
    for rep in range(3):
        padded = run(mesh, kind, b, 0, 4, staged=kind != "miss")  # (miss past its slot: the two calls, on slots of their own)
        trimmed = run(mesh, kind, a, 0, 4, staged=False)
        assert_same(kind, padded, trimmed, (pool, rep))


# every pool range of a call: (call, request array, offset field, count field, the pool's length)
RANGES = [("place", "preqs", "extra_off", "n_extra", "n_extra"), ("place_c", "creqs", "extra_off", "n_extra", "n_extra"),
          ("serve", "sreqs", "excl_off", "n_excl", "n_excl"), ("serve", "sreqs", "cnt_off", "n_cnt", "n_counters"),
          ("gate", "greqs", "excl_off", "n_excl", "n_excl"), ("gate", "greqs", "explicit_off", "n_explicit", "n_explicit"),
          ("miss", "greqs", "excl_off", "n_excl", "n_excl"), ("miss", "greqs", "explicit_off", "n_explicit", "n_explicit"),
          ("miss", "preqs", "extra_off", "n_extra", "n_extra"),
          ("route", "greqs", "excl_off", "n_excl", "n_excl"), ("route", "greqs", "explicit_off", "n_explicit", "n_explicit"),
          ("route", "sreqs", "excl_off", "n_excl", "n_excl"), ("route", "sreqs", "cnt_off", "n_cnt", "n_counters")]
# the arrays of a call that must not be null: requests and outputs (n > 0), pools (positive length)
REQS = {"place": ("preqs",), "place_c": ("creqs",), "serve": ("sreqs",), "gate": ("greqs",), "miss": ("greqs", "preqs"),
        "route": ("greqs", "sreqs"), "evict": ("ereqs",)}
POOL_ARRAYS = {"place": ("extra",), "place_c": ("extra",), "serve": ("counters", "xp", "xt"), "gate": ("xp", "xt", "expl"),
               "miss": ("xp", "xt", "expl", "extra"), "route": ("counters", "xp", "xt", "expl"), "evict": ()}


def small_args(fleet, s):
    """two requests without ranges of their own, every pool four entries long"""
    a = make_args(fleet, s, 5, 2, pools=False)
    a["sreqs"]["cnt_off"], a["sreqs"]["n_cnt"] = 0, 0
    a["counters"] = np.zeros(4, dtype=_lib.SERVE_COUNTER)
    a["xp"], a["xt"], a["expl"], a["extra"] = np.zeros(4, np.int32), np.zeros(4, np.int64), np.zeros(4, np.int32), np.zeros(4, np.int32)
    a["n_counters"] = a["n_excl"] = a["n_explicit"] = a["n_extra"] = 4
    return a


@pytest.mark.parametrize("ctx", ["mesh", "bare"])
def test_ranges_outside_their_pool_are_refused_before_the_state_check(request, fleet, ctx):
    s = request.getfixturevalue(ctx)
    base = small_args(fleet, s)
    for kind in REQS:
        assert raw(s, kind, base) == (MMP_OK if ctx == "mesh" else MMP_ESTATE), kind  # (what is refused below is the range alone)
    for kind, arr, off_f, cnt_f, len_k in RANGES:
        for off, cnt in [(-1, 1), (0, -1), (INT_MAX, 1), (INT_MAX, INT_MAX), (base[len_k], 1)]:
            a = dict(base)
            a[arr] = base[arr].copy()
            a[arr][off_f][1], a[arr][cnt_f][1] = off, cnt
            assert raw(s, kind, a) == MMP_EINVAL, (kind, arr, off_f, off, cnt)
            msg = (s.lib.mmp_last_error(s.h) or b"").decode()
            assert ("mmp_place_batch_c" if kind == "place_c" else "mmp_%s_batch" % kind) in msg and "request 1" in msg, msg


@pytest.mark.parametrize("ctx", ["mesh", "bare"])
def test_null_arrays_and_two_models_are_refused_before_the_state_check(request, fleet, ctx):
    s = request.getfixturevalue(ctx)
    base = small_args(fleet, s)
    for kind in REQS:
        for k in REQS[kind] + OUTS[kind] + POOL_ARRAYS[kind]:
            a = dict(base)
            a[k] = None
            assert raw(s, kind, a) == MMP_EINVAL, (kind, k)
    for kind, other in (("miss", "preqs"), ("route", "sreqs")):
        a = dict(base)
        a[other] = base[other].copy()
        a[other]["model"][1] = (base["greqs"]["model"][1] + 1) % fleet.n_models
        assert raw(s, kind, a) == MMP_EINVAL, kind


def test_empty_calls_and_state_answers(fleet, mesh, bare):
    empty = make_args(fleet, mesh, 1, 0)
    for kind in REQS:
        assert raw(mesh, kind, empty) == MMP_OK, kind
        assert raw(bare, kind, empty) == (MMP_OK if kind in ("miss", "evict") else MMP_ESTATE), kind
    assert raw(bare, "evict", make_args(fleet, bare, 1, 1)) == MMP_ESTATE  # no caches loaded


def test_route_refuses_a_pod_axis_shard_context_on_both_paths(fleet):
    """A shard's snapshot holds a slice of the instances: the route is refused whether the call would ride a slot (5) or be
    staged (257)."""
    import torch
    from modelmesh_amd import dist as mdist
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    try:
        s.load_fleet(fleet, commit=False)
        placer = mdist.PodShardedPlacer(mdist.SolverShardBackend(s, 0, 1, torch.device("cuda", 0)), speculative=True)
        mdist.run_lockstep([placer.commit_steps()])
        for n in (5, 257):
            assert raw(s, "route", make_args(fleet, s, n, n)) == MMP_ESTATE, n
    finally:
        s.close()
