"""GPU: batches — of one caller and of request rows — decided with the per-type shortlists a commit records (place_kernel.hpp:
TypeMemo, memo_try; include/mmplace.h: mmp_shortlists, mmp_split_batches) equal the oracle AND the same context with the shortlists
switched off (MMP_NO_MEMO=1: every request on the ordinary lane path) — on the bench configuration, on fuzzed fleets of every profile;
on batches built so that EVERY request has a position of its own inside its shortlist (the calling instance, a model's loaded
instance, a request's own exclusion: the check takes excluded candidates out of the recorded list and treats the caller as one more
candidate, and leaves what changes the walk itself to the ordinary path); and across commits and registry events that move the
shortlists (the registry's per-model words are rebuilt).  Every test runs in BOTH forms the library has for such batches, at every
batch size (by default they take launches that fill the chip): "one launch" = the check in front of the lane phase of the same kernel
(place_batch_m_kernel / place_batch_c_m_kernel: MMP_MEMO_FROM=0, MMP_NO_SPLIT=1) and "split" = the check alone in a first launch, the
rest in a dense tail launch (place_memo_kernel + place_tail_kernel: MMP_SPLIT_FROM=0)."""
import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd import workload as wl
from modelmesh_amd.solver import Solver
from oracle.bind import OracleFleet
from tests.util import covered_share

pytestmark = pytest.mark.gpu
FIELDS = ("chosen", "best", "n_candidates", "hash")


@pytest.fixture(autouse=True, params=["one launch", "split"])
def _every_batch_through_the_shortlists(request, monkeypatch):
    monkeypatch.setenv("MMP_MEMO_FROM", "0")
    if request.param == "split":
        monkeypatch.setenv("MMP_SPLIT_FROM", "0")
    else:
        monkeypatch.setenv("MMP_NO_SPLIT", "1")
    return request.param


def _solver(fleet):
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    s.load_fleet(fleet)
    return s


def _same(got, want, what):
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f, int(np.flatnonzero(got[f] != want[f])[0]))


def one_caller(fleet, reqs, pod, *, favour=0, drift=0, rpm=0, lru=None):
    """The batch as ONE instance issues it: self = pod (-1: not in the table), its fresh record = its row (+ drift)."""
    out = reqs.copy()
    row = fleet.pods[max(pod, 0)]
    out["self_pod"] = pod
    out["flags"] = favour
    out["fresh_lru"] = row["lru_time"] if lru is None else lru
    out["fresh_capacity"] = row["capacity"]
    out["fresh_used"] = row["used"] + drift
    out["fresh_count"] = int(row["count"]) + (1 if drift else 0)
    out["fresh_rpm"] = rpm
    return out


def place_as_caller(s, orc, fleet, reqs, extra, what):
    caller, rc = _lib.split_caller(reqs)
    got = s.place_c(caller, rc, extra, fleet.now)
    _same(got, orc.place(reqs, extra, fleet.now, threads=8), what)
    return got


def test_bench_configuration_is_covered_and_exact(_every_batch_through_the_shortlists):
    """C3, one decision per model from one caller: all four type rows have both shortlists, they answer > 97 % of the requests
    (the rest carry a position of their own inside the list), and every decision equals the oracle's; so do batches that are not
    a whole number of workgroups, callers that favour themselves, are absent from the table, or bring a drifted fresh record."""
    fleet = wl.make_fleet("C3")
    orc = OracleFleet(fleet)
    reqs, extra = wl.make_requests(fleet, 7)
    s = _solver(fleet)
    try:
        rows = s.shortlists()
        assert len(rows) == 8 and rows["valid"].all(), rows
        assert (rows["lo"] >= 0).all() and (rows["hi"] > rows["lo"]).all() and (rows["n_candidates"] >= 1).all()
        one = one_caller(fleet, reqs, 4711)
        assert covered_share(s, fleet, orc, one, extra) > 0.97
        place_as_caller(s, orc, fleet, one, extra, "caller 4711")
        place_as_caller(s, orc, fleet, one_caller(fleet, reqs, -1, rpm=250), extra, "caller not in the table")
        place_as_caller(s, orc, fleet, one_caller(fleet, reqs, 77, favour=1, drift=150_000), extra, "favourSelf, drifted record")
        place_as_caller(s, orc, fleet, one_caller(fleet, reqs, 9000, drift=10**9), extra, "a caller that is full by its fresh record")
        for n in (70_001, 1500):
            place_as_caller(s, orc, fleet, one[:n], extra, f"n={n}")
        # request rows, a caller per request (place_batch_m_kernel)
        assert covered_share(s, fleet, orc, reqs, extra) > 0.97
        _same(s.place(reqs, extra, fleet.now), orc.place(reqs, extra, fleet.now, threads=8), "request rows")
        _same(s.place(reqs[:70_001], extra, fleet.now), orc.place(reqs[:70_001], extra, fleet.now, threads=8), "request rows, n=70001")
        n_split, off = s.split_batches()
        if _every_batch_through_the_shortlists == "split":
            assert n_split >= 7 and not off, (n_split, off)  # every batch above (but the one of 1500: a latency slot) took the two launches; no tail was large
        else:
            assert n_split == 0
    finally:
        s.close()


@pytest.mark.parametrize("profile", [None, "full", "prefer"])
@pytest.mark.parametrize("seed", [3, 11, 29])
def test_fuzzed_fleets_with_and_without_the_shortlists(seed, profile, monkeypatch):
    fleet = wl.fuzz_fleet(seed, pods=700, models=900, profile=profile)
    orc = OracleFleet(fleet)
    reqs, extra = wl.fuzz_requests(fleet, seed * 7 + 1, 6000)
    rng = np.random.default_rng(seed)
    callers = [int(orc.order[0]), int(orc.order[min(5, len(orc.order) - 1)]), int(rng.integers(0, fleet.n_pods)), -1]
    batches = [one_caller(fleet, reqs, p, favour=j & 1, drift=(0, 90_000)[j >> 1 & 1], rpm=(0, 180)[j % 3 == 0],
                          lru=None if j % 2 else fleet.now - 50_000) for j, p in enumerate(callers)]
    batches.append(reqs)  # and the rows as they came: a caller per request
    want = [orc.place(b, extra, fleet.now, threads=8) for b in batches]
    for env in ({}, {"MMP_NO_MEMO": "1"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        s = _solver(fleet)
        try:
            for b, w in zip(batches[:-1], want[:-1]):
                caller, rc = _lib.split_caller(b)
                _same(s.place_c(caller, rc, extra, fleet.now), w, env or "shortlists")
            _same(s.place(batches[-1], extra, fleet.now), want[-1], ("rows", env or "shortlists"))
        finally:
            s.close()


@pytest.mark.parametrize("how", ["self", "loaded", "extra", "mixed"])
def test_requests_with_a_position_inside_their_shortlist_take_the_ordinary_path(how):
    """Every request of the batch names an instance from the head of the order — as the calling instance, as an instance that
    already holds the model, as one of the request's own exclusions: none may be answered from the recorded list."""
    fleet = wl.make_fleet("C2")
    orc = OracleFleet(fleet)
    head = orc.order[:48].astype(np.int32)  # the shortlists live here
    rng = np.random.default_rng(5)
    reqs, extra = wl.make_requests(fleet, 3, n=20_000, extra_frac=0.0)
    n = len(reqs)
    callers = [int(rng.integers(0, fleet.n_pods))]
    if how in ("self", "mixed"):
        callers = [int(p) for p in rng.choice(head, 3, replace=False)]
    if how in ("extra", "mixed"):
        ne = rng.integers(1, 5, n).astype(np.int32)
        off = np.zeros(n + 1, np.int64)
        np.cumsum(ne, out=off[1:])
        reqs["extra_off"], reqs["n_extra"] = off[:-1], ne
        extra = rng.choice(head, int(off[-1])).astype(np.int32)
    if how in ("loaded", "mixed"):  # the models' first loaded instance moves to the head of the order
        fleet.ent_pod = fleet.ent_pod.copy()
        m = fleet.models
        has = m["n_loaded"] > 0
        fleet.ent_pod[m["ent_off"][has]] = rng.choice(head, int(has.sum()))
        # (entries of a model must stay distinct: drop the models where the new head instance repeats another entry)
        for i in np.flatnonzero(has):
            e = fleet.ent_pod[m["ent_off"][i]: m["ent_off"][i] + m["n_loaded"][i] + m["n_failed"][i]]
            if len(set(e.tolist())) != len(e):
                fleet.models["n_loaded"][i] = 0
                fleet.models["n_failed"][i] = 0
        orc = OracleFleet(fleet)
    s = _solver(fleet)
    try:
        for j, p in enumerate(callers):
            place_as_caller(s, orc, fleet, one_caller(fleet, reqs, p, favour=j & 1), extra, (how, p))
        if how in ("self", "mixed"):  # rows: every request (self) / every second one (mixed) called by an instance at the head
            sel = np.ones(n, bool) if how == "self" else rng.random(n) < 0.5
            reqs["self_pod"] = np.where(sel, rng.choice(head, n), reqs["self_pod"])
            row = fleet.pods[reqs["self_pod"]]
            for f, g in (("fresh_lru", "lru_time"), ("fresh_capacity", "capacity"), ("fresh_used", "used"), ("fresh_count", "count")):
                reqs[f] = row[g]
            # the caller's own entry inside the list is answered by the check itself (memo_try): every class of the rpm rule, favourSelf
            reqs["fresh_rpm"] = rng.choice(np.array([0, 0, 150, 900, 5000, 2_000_000], np.int32), n)
            reqs["flags"] = (rng.random(n) < 0.3).astype(np.uint32)
            reqs["fresh_used"] += np.where(rng.random(n) < 0.3, rng.integers(0, 4_000_000, n), 0)  # (some callers full by their fresh record)
        _same(s.place(reqs, extra, fleet.now), orc.place(reqs, extra, fleet.now, threads=8), (how, "rows"))
    finally:
        s.close()


def test_shortlists_follow_commits_and_registry_events():
    """Instance rows change (the head of the order moves), models gain and lose copies at the head: after every commit /
    upsert the batch equals a fresh oracle."""
    fleet = wl.make_fleet("C2")
    rng = np.random.default_rng(9)
    s = _solver(fleet)
    try:
        seen = set()
        for step in range(6):
            orc = OracleFleet(fleet)
            reqs, extra = wl.make_requests(fleet, 100 + step, n=12_000)
            place_as_caller(s, orc, fleet, one_caller(fleet, reqs, int(rng.integers(0, fleet.n_pods))), extra, f"step {step}")
            seen.add(tuple(s.shortlists()["hi"].tolist()))
            head = orc.order[:40]
            if step % 2 == 0:  # a few instances at the head fill up / empty: the shortlists move
                idx = rng.choice(head, 6, replace=False).astype(np.int32)
                rows = fleet.pods[idx].copy()
                rows["used"] = np.where(rng.random(6) < 0.5, rows["capacity"] - 1, rows["capacity"] // 8)
                rows["count"] = rng.integers(0, 30, 6)
                fleet.pods[idx] = rows
                s.upsert_pods(idx, rows)
                s.commit()
            else:  # registry events: models whose only copy now sits at the head of the order
                mi = rng.choice(fleet.n_models, 300, replace=False).astype(np.int32)
                new_pod = rng.choice(head, 300).astype(np.int32)
                new_time = np.full(300, fleet.now - 5000, np.int64)
                rows = fleet.models[mi].copy()
                rows["n_loaded"], rows["n_failed"] = 1, 0
                rows["ent_off"] = np.arange(300)  # (indexing the arrays of this call)
                s.upsert_models(mi, rows, new_pod, new_time)
                rows["ent_off"] = len(fleet.ent_pod) + np.arange(300)  # the oracle's view: entries appended
                fleet.ent_pod = np.concatenate([fleet.ent_pod, new_pod])
                fleet.ent_time = np.concatenate([fleet.ent_time, new_time])
                fleet.models[mi] = rows
        assert len(seen) > 1, "the write stream never moved a shortlist"
    finally:
        s.close()


@pytest.mark.parametrize("blocks", [1, 3, 16, 64])
def test_the_tail_deals_its_requests_out_whatever_its_size(blocks, monkeypatch, _every_batch_through_the_shortlists):
    """The split form's second launch (place_tail_kernel) with 1 / 3 / 16 / 64 workgroups, on a batch that is not a whole number of
    wavefronts and in which every third request has a position of its own at the head of the order: a few thousand undecided
    requests, several passes per workgroup when there are few of them — every row equals the oracle's."""
    if _every_batch_through_the_shortlists != "split":
        pytest.skip("the split form only")
    monkeypatch.setenv("MMP_TAIL_BLOCKS", str(blocks))
    fleet = wl.make_fleet("C2")
    orc = OracleFleet(fleet)
    rng = np.random.default_rng(blocks)
    reqs, extra = wl.make_requests(fleet, 21, n=30_011)
    n = len(reqs)
    head = orc.order[:8].astype(np.int32)
    sel = rng.random(n) < 0.33
    reqs["self_pod"] = np.where(sel, rng.choice(head, n), reqs["self_pod"])
    row = fleet.pods[reqs["self_pod"]]
    for f, g in (("fresh_lru", "lru_time"), ("fresh_capacity", "capacity"), ("fresh_used", "used"), ("fresh_count", "count")):
        reqs[f] = row[g]
    s = _solver(fleet)
    try:
        _same(s.place(reqs, extra, fleet.now), orc.place(reqs, extra, fleet.now, threads=8), f"{blocks} workgroups")
        assert s.split_batches()[0] == 1
    finally:
        s.close()


def test_a_batch_the_records_do_not_fit_switches_the_split_off_until_the_next_commit(_every_batch_through_the_shortlists):
    """Every request called by the type's best instance without favourSelf: the check decides none of them, the tail all — right, but
    slowly — and reports it; the batches after it go through one launch until a commit gives the split another chance."""
    if _every_batch_through_the_shortlists != "split":
        pytest.skip("the split form only")
    fleet = wl.make_fleet("C2")
    orc = OracleFleet(fleet)
    reqs, extra = wl.make_requests(fleet, 33, n=20_000, extra_frac=0.0)
    hostile = reqs.copy()
    hostile["self_pod"] = orc.order[0]
    hostile["flags"] = 0
    row = fleet.pods[hostile["self_pod"]]
    for f, g in (("fresh_lru", "lru_time"), ("fresh_capacity", "capacity"), ("fresh_used", "used"), ("fresh_count", "count")):
        hostile[f] = row[g]
    s = _solver(fleet)
    try:
        _same(s.place(hostile, extra, fleet.now), orc.place(hostile, extra, fleet.now, threads=8), "hostile")
        assert s.split_batches() == (1, False)  # (the report is read by the NEXT split batch of the stream)
        _same(s.place(reqs, extra, fleet.now), orc.place(reqs, extra, fleet.now, threads=8), "after")
        n_split, off = s.split_batches()
        assert off and n_split == 1, (n_split, off)
        _same(s.place(reqs, extra, fleet.now), orc.place(reqs, extra, fleet.now, threads=8), "unsplit")
        assert s.split_batches() == (1, True)
        s.commit()
        assert s.split_batches() == (1, False)
        _same(s.place(reqs, extra, fleet.now), orc.place(reqs, extra, fleet.now, threads=8), "after the commit")
        assert s.split_batches() == (2, False)
    finally:
        s.close()


def test_more_exclusions_than_the_lane_phase_takes_next_to_requests_the_check_leaves(_every_batch_through_the_shortlists):
    """in the kernels without a workgroup barrier a wavefront's general path (a model with more than 8 excluded
    instances: place_one, two tiles of the whole table in LDS) ran while other wavefronts of the workgroup were still in their lane
    phase on per-lane LDS scratch that overlapped those tiles.  Every wavefront now owns its region (place_wave_lds).  A batch that
    mixes both kinds in every workgroup, 5 000 instances (tiles of 1.3 KB over the scratch columns), decided three times."""
    fleet = wl.make_fleet("C3", models=40_000, pods=5_000)
    rng = np.random.default_rng(77)
    # a sixth of the models get 9-12 loaded instances spread over the table
    m = fleet.models
    big = rng.random(fleet.n_models) < 0.16
    k = np.where(big, rng.integers(9, 13, fleet.n_models), m["n_loaded"] + m["n_failed"]).astype(np.int64)
    off = np.zeros(fleet.n_models + 1, np.int64)
    np.cumsum(k, out=off[1:])
    ent = np.zeros(int(off[-1]), np.int32)
    for i in range(fleet.n_models):
        if big[i]:
            ent[off[i]:off[i + 1]] = np.sort(rng.choice(fleet.n_pods, int(k[i]), replace=False))
        else:
            ent[off[i]:off[i + 1]] = fleet.ent_pod[m["ent_off"][i]: m["ent_off"][i] + k[i]]
    fleet.ent_pod, fleet.ent_time = ent, np.full(len(ent), fleet.now - 10_000, np.int64)
    fleet.models["ent_off"] = off[:-1]
    fleet.models["n_loaded"] = np.where(big, k, m["n_loaded"])
    fleet.models["n_failed"] = np.where(big, 0, m["n_failed"])
    orc = OracleFleet(fleet)
    reqs, extra = wl.make_requests(fleet, 5)
    head = orc.order[:40].astype(np.int32)
    sel = rng.random(len(reqs)) < 0.2  # ... and a fifth of the callers stand at the head of the order (the lane phase runs in every workgroup)
    reqs["self_pod"] = np.where(sel, rng.choice(head, len(reqs)), reqs["self_pod"])
    row = fleet.pods[reqs["self_pod"]]
    for f, g in (("fresh_lru", "lru_time"), ("fresh_capacity", "capacity"), ("fresh_used", "used"), ("fresh_count", "count")):
        reqs[f] = row[g]
    want = orc.place(reqs, extra, fleet.now, threads=8)
    s = _solver(fleet)
    try:
        for rep in range(3):
            _same(s.place(reqs, extra, fleet.now), want, f"rep {rep}")
    finally:
        s.close()
