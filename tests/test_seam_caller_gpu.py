"""GPU: the single-caller forms of the route and miss seams (mmp_route_batch_c / mmp_miss_batch_c; route_batch_c_kernel and
gate_batch_c_kernel, modelmesh_amd/csrc/seam_caller_kernels.hpp).

Their answers are DEFINED as those of mmp_route_batch / mmp_miss_batch on the rows tests/seam_caller_model.py expands, so every
comparison here is of bytes: (1) fuzz fleets at the row counts where the path or the last wavefront's fill changes, (2) every
selected row of the guard edge cases as the caller of a 300-row batch, held to the reference's own rows
(tests/golden/ref_gate_edges.npz) as well, (3) the refusals, (4) beside other calls and a commit, (5) twice."""
import dataclasses
import threading

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd import workload as wl
from modelmesh_amd._lib import MMP_EINVAL, MMP_ESTATE, MMP_OK, ptr
from modelmesh_amd.solver import Solver
from tests import ref_fleets as rf
from tests import seam_caller_model as scm
from tests.gate_helpers import GOLDEN_GATE_EDGES, gate_edge_inputs

pytestmark = pytest.mark.gpu

# 0 .. 256: written out as full rows for the existing calls' slots; 257 ..: the new kernels, whose last wavefront holds
# 1 (257, 321, 513), 63 (319, 511), 64 (320, 512) or 40 (1 000) rows
NS = (0, 1, 63, 64, 65, 255, 256, 257, 319, 320, 321, 511, 512, 513, 1000)
N_MAX = max(NS)
ROUTE_SLOT = {"n": 256, "counters": 4096, "excl": 4096, "explicit": 4096}  # RouteSlot (mmplace.hip)
MISS_SLOT = {"n": 256, "extra": 2048, "excl": 2048, "explicit": 2048}      # MissSlot
EXPIRY = 450_000
BATCH = 300  # the calls of parts 2 to 4: past the slots; two workgroups, four full wavefronts and one of 44 rows


def with_long_copy_lists(fleet, seed, k_models=12):
    """The fuzz fleets give a model at most three copies; the kernels prefetch four.  k_models models get 5 to 9 copies on
    different instances and 0 to 5 failure records, in instance-id order as the registry lists them."""
    rng = np.random.default_rng(seed)
    P = fleet.n_pods
    models, ent_pod, ent_time = fleet.models.copy(), [fleet.ent_pod], [fleet.ent_time]
    off = len(fleet.ent_pod)
    chosen = rng.choice(fleet.n_models, k_models, replace=False)
    for m in chosen:
        k, nf = int(rng.integers(5, 10)), int(rng.integers(0, 6))
        pods = rng.choice(P, k + nf, replace=False).astype(np.int32)
        order = fleet.pods["id_order"]
        lp, fp = pods[:k][np.argsort(order[pods[:k]])], pods[k:][np.argsort(order[pods[k:]])]
        ent_pod.append(np.concatenate([lp, fp]))
        ent_time.append((fleet.now - rng.integers(1_000, 600_000, k + nf)).astype(np.int64))
        models["ent_off"][m], models["n_loaded"][m], models["n_failed"][m] = off, k, nf
        off += k + nf
    return dataclasses.replace(fleet, models=models, ent_pod=np.concatenate(ent_pod), ent_time=np.concatenate(ent_time)), chosen


def _ranges(rng, n, long_every):
    """[off, off + cnt) per request: none for half, 1-3 entries for most others, 5-7 for every long_every-th"""
    cnt = np.where(rng.random(n) < 0.5, rng.integers(1, 4, n), 0).astype(np.int32)
    cnt[::long_every] = rng.integers(5, 8, len(cnt[::long_every]))
    off = np.zeros(n + 1, np.int64)
    np.cumsum(cnt, out=off[1:])
    return off[:-1].astype(np.int32), cnt, int(off[-1])


def make_caller(fleet, rng, self_pod):
    now = fleet.now
    c = np.zeros(1, dtype=_lib.SEAM_CALLER)
    c["self_pod"] = self_pod
    c["gate_flags"] = int(rng.choice([0, 1, 1 | 64, 256, 128 | 8]))
    c["loading_count"], c["weight_predict_cutoff"] = int(rng.integers(0, 13)), 10
    c["cache_capacity"], c["cache_weighted_size"] = 8_388_608, int(rng.integers(8_000_000, 9_000_000))
    c["cache_oldest_time"] = now - int(rng.integers(0, 1_000_000))
    c["load_timeout_ms"] = 240_000
    row = fleet.pods[max(self_pod, 0)]
    c["fresh_lru"], c["fresh_capacity"], c["fresh_used"], c["fresh_count"] = row["lru_time"], row["capacity"], row["used"], row["count"]
    c["fresh_loading_threads"], c["fresh_in_progress"], c["fresh_rpm"] = row["loading_threads"], int(rng.integers(0, 3)), int(row["rpm"])
    c["last_published"] = now - int(rng.choice([500, 3_000, 38_000, 45_000, 170_000]))
    c["local_in_flight"], c["last_invoke_time"] = int(rng.integers(0, 3)), now - int(rng.choice([0, 10, 1000]))
    pc = np.zeros(1, dtype=_lib.PLACE_CALLER)
    pc["self_pod"], pc["flags"] = self_pod, int(rng.integers(0, 2))
    pc["fresh_lru"], pc["fresh_capacity"], pc["fresh_used"] = row["lru_time"], row["capacity"], row["used"]
    pc["fresh_count"], pc["fresh_rpm"] = row["count"], int(rng.choice([0, 120, 400]))
    return c, pc


def make_batch(fleet, s, seed, n, self_pod, long_models):
    """One caller's batch of n requests with their pools: dict of the arguments of route_c and miss_c."""
    rng = np.random.default_rng(seed)
    M, P, now = fleet.n_models, fleet.n_pods, fleet.now
    a = {"now": now}
    a["caller"], a["pcaller"] = make_caller(fleet, rng, self_pod)
    g = np.zeros(n, dtype=_lib.GATE_REQ_C)
    g["model"] = rng.integers(0, M, n)
    g["model"][1::7] = long_models[np.arange(len(g["model"][1::7])) % len(long_models)]  # copy lists longer than the prefetch
    g["model"][5::31] = -1
    g["flags"] = rng.integers(0, 512, n)
    g["excl_off"], g["n_excl"], n_excl = _ranges(rng, n, 9)
    g["explicit_off"], g["n_explicit"], n_explicit = _ranges(rng, n, 11)
    g["size_hint"], g["loader_predicted"] = rng.integers(0, 20_000, n), rng.integers(0, 20_000, n)
    g["last_used_time"] = now - rng.integers(0, 10_000_000, n)
    g["loaded_time"] = np.where(rng.random(n) < 0.3, -1, now - rng.integers(0, 1_000_000, n))
    # exclusions that bite: a copy of the request's model with its load time, one millisecond off, or any time
    xp, xt = rng.integers(0, P, n_excl).astype(np.int32), (now - rng.integers(0, 100_000, n_excl)).astype(np.int64)
    for i in np.nonzero((g["n_excl"] > 0) & (g["model"] >= 0))[0]:
        m = fleet.models[g["model"][i]]
        if m["n_loaded"]:
            for j in range(int(g["n_excl"][i])):
                e = int(m["ent_off"]) + int(rng.integers(0, m["n_loaded"]))
                xp[g["excl_off"][i] + j] = fleet.ent_pod[e]
                xt[g["excl_off"][i] + j] = int(rng.choice([fleet.ent_time[e], fleet.ent_time[e] + 1, _lib.ANY_TIME]))
    a["greqs"], a["xp"], a["xt"], a["expl"] = g, xp, xt, rng.integers(0, P, n_explicit).astype(np.int32)
    sr = np.zeros(n, dtype=_lib.SERVE_REQ)
    sr["model"], sr["self_pod"] = g["model"], self_pod
    sr["flags"], sr["assume_completed_ms"] = rng.integers(0, 4, n), rng.choice([3000, 30_000], n)
    in_use = rng.integers(0, 3, P).astype(np.int32)
    last_used = (now - rng.choice([0, 5, 5, 100, 10_000], P)).astype(np.int64)
    sr, a["counters"] = s.serve_counters(sr, in_use, last_used)
    a["sreqs"] = scm.serve_request_side(sr)
    p = np.zeros(n, dtype=_lib.PLACE_REQ_C)
    p["model"], p["pick"] = g["model"], rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    p["last_used"] = np.where(rng.random(n) < 0.2, 0, now - rng.integers(0, 90_000_000, n))
    p["extra_off"], p["n_extra"], n_extra = _ranges(rng, n, 13)
    a["preqs"], a["extra"] = p, rng.integers(0, P, n_extra).astype(np.int32)
    return a


def head(a, n):
    """the first n requests of a batch with the whole pools"""
    b = dict(a)
    for k in ("greqs", "sreqs", "preqs"):
        b[k] = np.ascontiguousarray(a[k][:n])
    return b


def route_both(s, a):
    """-> (route_c's outputs, route's outputs on the expanded rows)"""
    got = s.route_c(a["caller"], a["greqs"], a["sreqs"], a["counters"], a["xp"], a["xt"], a["expl"], a["now"], EXPIRY)
    fg, fs = scm.expand_route(a["caller"], a["greqs"], a["sreqs"])
    want = s.route(fg, fs, a["counters"], a["xp"], a["xt"], a["expl"], a["now"], EXPIRY)
    return got, want


def miss_both(s, a):
    got = s.miss_c(a["caller"], a["pcaller"], a["greqs"], a["preqs"], a["xp"], a["xt"], a["expl"], a["extra"], a["now"], EXPIRY)
    fg, fp = scm.expand_miss(a["caller"], a["pcaller"], a["greqs"], a["preqs"])
    want = s.miss(fg, fp, a["xp"], a["xt"], a["expl"], a["extra"], a["now"], EXPIRY)
    return got, want


def assert_bytes(got, want, what):
    for k, (x, y) in enumerate(zip(got, want)):
        assert x.dtype == y.dtype and len(x) == len(y), what
        if x.tobytes() != y.tobytes():
            bad = [i for i in range(len(x)) if x[i] != y[i]]
            raise AssertionError((what, "output", k, len(bad), [(i, x[i], y[i]) for i in bad[:4]]))


# ---- 1. equal to the existing calls ------------------------------------------------------------------------------------------
FLEETS = {"65 instances": (5, 65, None), "200 instances, type constraints": (1, 200, "typed")}


@pytest.fixture(scope="module", params=list(FLEETS))
def mesh(request):
    seed, pods, profile = FLEETS[request.param]
    fleet, long_models = with_long_copy_lists(wl.fuzz_fleet(seed, pods=pods, models=300, profile=profile), seed)
    assert (fleet.n_types > 0 and fleet.has_allowed.any()) == (profile is not None)
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    s.load_fleet(fleet)
    yield fleet, long_models, s
    s.close()


def check_contents(fleet, a, long_models):
    g = a["greqs"]
    named = fleet.models["n_loaded"][g["model"][g["model"] >= 0]]
    assert (named > 4).sum() >= 20 and (g["n_excl"] > 4).sum() >= 20 and (g["n_explicit"] > 4).sum() >= 20
    assert (g["model"] == -1).sum() >= 5 and (a["sreqs"]["n_cnt"] > 4).sum() >= 5


@pytest.mark.parametrize("self_pod", [3, -1])
def test_route_c_equals_route_on_the_expanded_rows(mesh, self_pod):
    fleet, long_models, s = mesh
    a = make_batch(fleet, s, 101 + self_pod, N_MAX, self_pod, long_models)
    check_contents(fleet, a, long_models)
    assert len(a["counters"]) <= ROUTE_SLOT["counters"] and len(a["xp"]) <= ROUTE_SLOT["excl"] and len(a["expl"]) <= ROUTE_SLOT["explicit"]
    staged = set()
    for n in NS:
        b = head(a, n)
        s.profile(True)
        got, want = route_both(s, b)
        assert len(got[0]) == n and len(got[1]) == n
        assert_bytes(got, want, ("route", n, self_pod))
        s.profile(True)
        s.route_c(b["caller"], b["greqs"], b["sreqs"], b["counters"], b["xp"], b["xt"], b["expl"], b["now"], EXPIRY)
        if s.last_kernel_ms() >= 0:  # a staged call leaves its kernel time, a slot call does not
            staged.add(n)
    assert staged == {n for n in NS if n > ROUTE_SLOT["n"]}  # the row count alone decided the path
    s.profile(False)


@pytest.mark.parametrize("self_pod", [3, -1])
def test_miss_c_equals_miss_on_the_expanded_rows(mesh, self_pod):
    fleet, long_models, s = mesh
    a = make_batch(fleet, s, 202 + self_pod, N_MAX, self_pod, long_models)
    check_contents(fleet, a, long_models)
    assert max(len(a["xp"]), len(a["expl"]), len(a["extra"])) <= MISS_SLOT["excl"]
    for n in NS:
        got, want = miss_both(s, head(a, n))
        assert len(got[0]) == n and len(got[1]) == n
        assert_bytes(got, want, ("miss", n, self_pod))


@pytest.mark.parametrize("n", [1, 64])
def test_a_pool_past_the_slot_sends_few_rows_to_the_new_kernels(mesh, n):
    fleet, long_models, s = mesh
    a = head(make_batch(fleet, s, 303, 64, 3, long_models), n)
    pad = 4097 - len(a["xp"])
    assert pad > 0
    a["xp"] = np.concatenate([a["xp"], np.zeros(pad, np.int32)])  # pairs no request references
    a["xt"] = np.concatenate([a["xt"], np.zeros(pad, np.int64)])
    assert len(a["xp"]) > max(ROUTE_SLOT["excl"], MISS_SLOT["excl"])
    s.profile(True)
    got = s.route_c(a["caller"], a["greqs"], a["sreqs"], a["counters"], a["xp"], a["xt"], a["expl"], a["now"], EXPIRY)
    assert s.last_kernel_ms() >= 0  # staged: route_batch_c_kernel
    s.profile(False)
    fg, fs = scm.expand_route(a["caller"], a["greqs"], a["sreqs"])
    assert_bytes(got, s.route(fg, fs, a["counters"], a["xp"], a["xt"], a["expl"], a["now"], EXPIRY), ("route, long pool", n))
    got, want = miss_both(s, a)
    assert_bytes(got, want, ("miss, long pool", n))


# ---- 5. determinism ----------------------------------------------------------------------------------------------------------
def test_two_runs_of_the_largest_call_are_byte_identical(mesh):
    fleet, long_models, s = mesh
    a = make_batch(fleet, s, 100, N_MAX, 3, long_models)  # (the largest call of part 1)
    runs = [(s.route_c(a["caller"], a["greqs"], a["sreqs"], a["counters"], a["xp"], a["xt"], a["expl"], a["now"], EXPIRY),
             s.miss_c(a["caller"], a["pcaller"], a["greqs"], a["preqs"], a["xp"], a["xt"], a["expl"], a["extra"], a["now"], EXPIRY))
            for _ in range(2)]
    assert_bytes(runs[0][0], runs[1][0], "route_c twice")
    assert_bytes(runs[0][1], runs[1][1], "miss_c twice")


# ---- 2. held to the reference text -------------------------------------------------------------------------------------------
NAMES = [str(n) for n in np.load(GOLDEN_GATE_EDGES)["names"]]
BIT_NAMES = ("GO_LOCAL", "FAILURES_BREACHED", "LOCATIONS_BREACHED", "LOCAL_NOT_ALLOWED", "CHURN_REJECT", "EARLY_REJECT",
             "RELOAD_ELSEWHERE", "SHOULD_PUBLISH")


def single_rows(name, r):
    """The row selection of tests/test_gate_edges_gpu.py:single_rows, restated: every timed row with a fifth-or-later exclusion,
    every engineered row of the totals fleets, every row of the thresholds fleets, and 64 rows spread over the case."""
    tier = rf.gate_edge_tier(name)
    spread = np.linspace(0, len(r) - 1, 64).astype(np.int64)
    if tier == "timed":
        spread = np.union1d(spread, np.nonzero(r["n_excl"] >= 5)[0])
    elif tier == "totals":
        spread = np.union1d(spread, np.arange(len(r) - rf.N_TOTALS_PLAIN))
    elif tier == "thresholds":
        spread = np.arange(len(r))
    return spread


@pytest.fixture(scope="module")
def edges():
    ref = np.load(GOLDEN_GATE_EDGES)
    return ref, {c[0]: c for c in gate_edge_inputs(ref)}


def test_the_selected_rows_set_and_clear_every_guard_in_every_tier(edges):
    """From the golden file alone (and the selection): what part 2 holds to the reference covers both values of every guard."""
    ref, cases = edges
    total = {}
    for name in NAMES:
        rows = single_rows(name, cases[name][3])
        assert 64 <= len(rows) <= 1121 and len(np.unique(rows)) == len(rows), name
        total.setdefault(rf.gate_edge_tier(name), []).append(ref[f"{name}/gate"][rows, 0].astype(np.uint32))
    assert set(total) == set(rf.GATE_EDGE_TIERS)
    for tier, parts in total.items():
        bits = np.concatenate(parts)
        for k, bit in enumerate(BIT_NAMES):
            n_set = int(((bits >> k) & 1).sum())
            if (tier, bit) == ("totals", "FAILURES_BREACHED"):
                assert (n_set, len(bits)) == (0, 4484)  # the one guard a tier's selection never sets
                continue
            assert n_set >= 2 and len(bits) - n_set >= 36, (tier, bit, n_set, len(bits))


@pytest.mark.parametrize("name", NAMES)
def test_guard_edges_through_the_single_caller_calls(edges, name):
    ref, cases = edges
    _, fleet, ids, r, xp, xt, expl, expiry, _ = cases[name]
    want = ref[f"{name}/gate"]
    rows = single_rows(name, r)
    rng = np.random.default_rng(len(name) + fleet.n_pods)
    N, P, now = len(r), fleet.n_pods, fleet.now
    assert N >= 2 * BATCH
    none = np.zeros(0, np.int32)
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    try:
        s.load_fleet(fleet)
        # the request sides of every row once, laid out twice so that rows i .. i + 299 (wrapping round) are one slice
        sr = np.zeros(N, dtype=_lib.SERVE_REQ)
        sr["model"], sr["self_pod"] = r["model"], r["self_pod"]
        sr["flags"], sr["assume_completed_ms"] = rng.integers(0, 4, N), rng.choice([3000, 30_000], N)
        in_flight, last_invoke = rng.integers(0, 3, N), now - rng.choice([0, 10, 1000], N)
        sr, counters = s.serve_counters(sr, rng.integers(0, 3, P).astype(np.int32),
                                        (now - rng.choice([0, 5, 5, 100, 10_000], P)).astype(np.int64))
        pr = wl.make_requests(fleet, 5, n=N, extra_frac=0.0)[0]
        pr["model"], pr["self_pod"], pr["n_extra"], pr["extra_off"] = r["model"], r["self_pod"], 0, 0
        G, S = np.tile(scm.request_side(r), 2), np.tile(scm.serve_request_side(sr), 2)
        PQ = np.zeros(N, dtype=_lib.PLACE_REQ_C)
        for f in _lib.PLACE_REQ_C.names:
            PQ[f] = pr[f]
        PQ = np.tile(PQ, 2)
        done = np.zeros(N, bool)
        for i in rows:
            caller, row = scm.split_gate(r[i], in_flight[i], last_invoke[i])
            assert row[0] == G[i]
            pcaller = np.zeros(1, dtype=_lib.PLACE_CALLER)
            for f in _lib.PLACE_CALLER.names:
                pcaller[f] = pr[f][i]
            g, sq, pq = G[i:i + BATCH], S[i:i + BATCH], PQ[i:i + BATCH]
            got_r = s.route_c(caller, g, sq, counters, xp, xt, expl, now, expiry)
            got_m = s.miss_c(caller, pcaller, g, pq, xp, xt, expl, none, now, expiry)
            for what, o in (("route_c", got_r[0]), ("miss_c", got_m[0])):  # position 0 is row i itself: the reference's row
                assert int(o["bits"][0]) == int(want[i, 0]), (name, what, int(i), bin(int(o["bits"][0])), bin(int(want[i, 0])))
                # (the initial size is observable where loadLocal does not return early, MM.java:5195)
                assert (int(want[i, 0]) & 32) or int(o["initial_size"][0]) == int(want[i, 1]), (name, what, int(i))
            fg, fs = scm.expand_route(caller, g, sq)
            assert fg[:1].tobytes() == r[i:i + 1].tobytes()
            assert_bytes(got_r, s.route(fg, fs, counters, xp, xt, expl, now, expiry), (name, "route", int(i)))
            fp = _lib.join_caller(pcaller, pq)  # (expand_miss's rows: the gate rows are the route's)
            assert_bytes(got_m, s.miss(fg, fp, xp, xt, expl, none, now, expiry), (name, "miss", int(i)))
            done[i] = True
        assert done[rows].all() and int(done.sum()) == len(rows)  # no selected row was left out
    finally:
        s.close()


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------
def raw_route(s, a, n):
    p = lambda k: ptr(a[k]) if a[k] is not None and len(a[k]) else None  # noqa: E731
    return s.lib.mmp_route_batch_c(s.h, p("caller"), p("greqs"), p("sreqs"), n, p("counters"), a["n_counters"], p("xp"), p("xt"),
                                   a["n_excl"], p("expl"), a["n_explicit"], a["now"], EXPIRY, p("gouts"), p("souts"))


def raw_miss(s, a, n):
    p = lambda k: ptr(a[k]) if a[k] is not None and len(a[k]) else None  # noqa: E731
    return s.lib.mmp_miss_batch_c(s.h, p("caller"), p("pcaller"), p("greqs"), p("preqs"), n, p("xp"), p("xt"), a["n_excl"], p("expl"),
                                  a["n_explicit"], p("extra"), a["n_extra"], a["now"], EXPIRY, p("gouts"), p("pouts"))


def refusal_args(fleet, s, n, long_models):
    a = head(make_batch(fleet, s, 404, max(n, 1), 3, long_models), n)
    a["n_counters"], a["n_excl"], a["n_explicit"], a["n_extra"] = len(a["counters"]), len(a["xp"]), len(a["expl"]), len(a["extra"])
    assert min(a["n_counters"], a["n_excl"], a["n_explicit"], a["n_extra"]) > 0
    for k, dt in (("gouts", _lib.GATE_OUT), ("souts", _lib.SERVE_OUT), ("pouts", _lib.PLACE_OUT)):
        a[k] = np.frombuffer(bytes([0xA5]) * (dt.itemsize * n), dtype=dt).copy()
    return a


def einval_cases(a, n, kind):
    """(what, arguments, n) of every refusal of include/mmplace.h for one call"""
    INT_MAX = 2**31 - 1
    own = ("sreqs", "souts", "counters") if kind == "route" else ("preqs", "pouts", "extra", "pcaller")
    for k in ("caller", "greqs", "gouts", "xp", "xt", "expl") + own:
        yield "null " + k, dict(a, **{k: None}), n
    yield "n < 0", a, -1
    for k in ("n_excl", "n_explicit") + (("n_counters",) if kind == "route" else ("n_extra",)):
        yield k + " < 0", dict(a, **{k: -1}), n
    ranges = [("greqs", "excl_off", "n_excl", "n_excl"), ("greqs", "explicit_off", "n_explicit", "n_explicit")]
    ranges.append(("sreqs", "cnt_off", "n_cnt", "n_counters") if kind == "route" else ("preqs", "extra_off", "n_extra", "n_extra"))
    for arr, off_f, cnt_f, len_k in ranges:
        for off, cnt in [(-1, 1), (0, -1), (INT_MAX, 1), (INT_MAX, INT_MAX), (a[len_k], 1)]:
            b = dict(a)
            b[arr] = a[arr].copy()
            b[arr][off_f][n - 1], b[arr][cnt_f][n - 1] = off, cnt
            yield f"{arr}.{off_f} = {off}, {cnt_f} = {cnt}", b, n
    if kind == "miss":
        b = dict(a)
        b["preqs"] = a["preqs"].copy()
        b["preqs"]["model"][n - 1] = (int(a["greqs"]["model"][n - 1]) + 1) % 300  # the LAST row names two models
        yield "two models in the last row", b, n


@pytest.mark.parametrize("n", [2, BATCH])
def test_refusals_leave_the_outputs_as_they_were(mesh, n):
    fleet, long_models, s = mesh
    a = refusal_args(fleet, s, n, long_models)
    assert a["greqs"]["model"][n - 1] >= 0
    before = {k: a[k].tobytes() for k in ("gouts", "souts", "pouts")}
    for kind, raw in (("route", raw_route), ("miss", raw_miss)):
        for what, b, nn in einval_cases(a, n, kind):
            assert raw(s, b, nn) == MMP_EINVAL, (kind, what)
            assert ("mmp_%s_batch_c" % kind) in (s.lib.mmp_last_error(s.h) or b"").decode(), (kind, what)
            for k in before:
                assert a[k].tobytes() == before[k], (kind, what, k)
    assert raw_route(s, a, n) == MMP_OK and raw_miss(s, a, n) == MMP_OK  # (what was refused above was the one argument alone)
    assert a["gouts"].tobytes() != before["gouts"]


@pytest.mark.parametrize("n", [2, BATCH])
def test_before_the_first_commit_the_answer_is_estate(mesh, n):
    fleet, long_models, _ = mesh
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    try:
        s.load_fleet(fleet, commit=False)
        a = refusal_args(fleet, s, n, long_models)
        before = {k: a[k].tobytes() for k in ("gouts", "souts", "pouts")}
        assert raw_route(s, a, n) == MMP_ESTATE and raw_miss(s, a, n) == MMP_ESTATE
        assert {k: a[k].tobytes() for k in before} == before
        b = dict(a)
        b["greqs"] = a["greqs"].copy()
        b["greqs"]["n_excl"][n - 1] = -1
        assert raw_route(s, b, n) == MMP_EINVAL and raw_miss(s, b, n) == MMP_EINVAL  # the arguments are looked at first
    finally:
        s.close()


# ---- 4. beside other work ----------------------------------------------------------------------------------------------------
def test_four_callers_beside_a_commit_answer_as_alone(mesh):
    fleet, long_models, s = mesh
    batches = [make_batch(fleet, s, 500 + t, BATCH, (7 * t + 2) % fleet.n_pods, long_models) for t in range(4)]

    def call(a):
        return s.route_c(a["caller"], a["greqs"], a["sreqs"], a["counters"], a["xp"], a["xt"], a["expl"], a["now"], EXPIRY)
    alone = [call(a) for a in batches]
    for t, a in enumerate(batches):  # ... which is the existing call's answer
        assert_bytes(alone[t], route_both(s, a)[1], ("alone", t))
    errors, cond, state = [], threading.Condition(), {"calls": 0, "done": 0, "commits": 0}

    def caller_thread(t):
        try:
            for rep in range(50):
                assert_bytes(call(batches[t]), alone[t], ("thread", t, rep))
                with cond:
                    state["calls"] += 1
                    cond.notify_all()
        except BaseException as e:  # noqa: BLE001
            errors.append(e)
        finally:
            with cond:
                state["done"] += 1
                cond.notify_all()

    def commit_thread():
        # one commit of the unchanged table per answered call, for as long as a caller runs (a commit loop without that pace
        # holds the batch lock back to back and the callers wait behind it)
        try:
            seen = -1
            while True:
                with cond:
                    cond.wait_for(lambda: state["calls"] != seen or state["done"] == 4)
                    if state["done"] == 4:
                        return
                    seen = state["calls"]
                s.commit()
                state["commits"] += 1
        except BaseException as e:  # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=caller_thread, args=(t,)) for t in range(4)]
    committer = threading.Thread(target=commit_thread)
    committer.start()
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    committer.join()
    assert not errors, errors[:2]
    assert state["calls"] == 200 and state["commits"] >= 10
