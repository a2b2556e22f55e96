"""GPU: the split form's first launch decides the rows its shortlist check leaves wherever the ordinary lane phase can, in the wavefront
that found them (place_kernel.hpp: place_memo_body -> lane_phase); only what that phase hands on reaches the tail's lists
(place_tail_kernel), and the tail reports the rows the check left, not the lengths of its lists.

Every batch here takes the split route (MMP_MEMO_FROM=0, MMP_SPLIT_FROM=0) from device memory, so that a batch of any size gets the
batch kernels, and every row — all four fields — is compared with the oracle.  The result buffers start as 0xFF bytes: a row nobody
wrote cannot pass."""
import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd import workload as wl
from modelmesh_amd.solver import Solver
from oracle.bind import OracleFleet
from tests.util import covered_share

pytestmark = pytest.mark.gpu
FIELDS = ("chosen", "best", "n_candidates", "hash")
SIZES = (1, 63, 64, 65, 255, 256, 257, 1021)
FRESH = (("fresh_lru", "lru_time"), ("fresh_capacity", "capacity"), ("fresh_used", "used"), ("fresh_count", "count"))


@pytest.fixture(autouse=True)
def _every_batch_split(monkeypatch):
    monkeypatch.setenv("MMP_MEMO_FROM", "0")
    monkeypatch.setenv("MMP_SPLIT_FROM", "0")


def _solver(fleet):
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    s.load_fleet(fleet)
    return s


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        a = np.zeros(1, np.int32)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(torch.device("cuda", 0))


def _place(s, reqs, extra, now, how="place_dev", stream=None):
    """One batch from device memory on `stream` (a new one if none is given), waited for: the result rows."""
    import torch
    n = len(reqs)
    st = stream or torch.cuda.Stream()
    d_x = _dev(extra)
    d_o = torch.full((n * _lib.PLACE_OUT.itemsize,), 0xFF, dtype=torch.uint8, device="cuda:0")
    x = d_x.data_ptr() if len(extra) else 0
    if how == "place_c_dev":
        caller, rc = _lib.split_caller(reqs)
        d_r = _dev(rc)
        s.place_c_dev(caller, d_r.data_ptr(), n, x, len(extra), now, d_o.data_ptr(), st.cuda_stream)
    elif how == "place_dev2":
        d_r = _dev(reqs)
        s.place_dev2(d_r.data_ptr(), n, x, len(extra), now, d_o.data_ptr(), st.cuda_stream)
    else:
        d_r = _dev(reqs)
        s.place_dev(d_r.data_ptr(), n, x, now, d_o.data_ptr(), st.cuda_stream)
    torch.cuda.synchronize()
    return np.frombuffer(d_o.cpu().numpy().tobytes(), dtype=_lib.PLACE_OUT)[:n]


def _same(got, want, what):
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f, int(np.flatnonzero(got[f] != want[f])[0]))


def _callers_to(reqs, fleet, sel, pods):
    """The rows `sel` as instance `pods` issues them: self = the instance, the fresh record = its table row."""
    out = reqs.copy()
    out["self_pod"] = np.where(sel, pods, out["self_pod"])
    row = fleet.pods[out["self_pod"]]
    for f, g in FRESH:
        out[f] = np.where(sel, row[g], out[f])
    return out


def _third_at_the_head(fleet, orc, seed, n):
    """n request rows, a third of them called by one of the first instances of the placement order (the shortlists live there): most
    wavefronts hold rows the check leaves next to rows it decides."""
    rng = np.random.default_rng(seed)
    reqs, extra = wl.make_requests(fleet, seed, n=n)
    head = orc.order[: min(8, len(orc.order))].astype(np.int32)
    reqs = _callers_to(reqs, fleet, rng.random(n) < 1 / 3, rng.choice(head, n))
    return reqs, extra


@pytest.fixture(scope="module")
def mixed():
    """Per configuration: the fleet, its oracle, 1 021 mixed rows and the oracle's answer (decisions are independent: a prefix of the
    batch has the prefix of the answer)."""
    out = {}
    for name in ("C1", "C2"):
        fleet = wl.make_fleet(name)
        orc = OracleFleet(fleet)
        reqs, extra = _third_at_the_head(fleet, orc, 41, max(SIZES))
        out[name] = (fleet, orc, reqs, extra, orc.place(reqs, extra, fleet.now, threads=8))
    return out


@pytest.mark.parametrize("name", ["C1", "C2"])
def test_rows_the_check_leaves_next_to_rows_it_decides(mixed, name):
    fleet, orc, reqs, extra, want = mixed[name]
    s = _solver(fleet)
    try:
        for k, n in enumerate(SIZES):
            _same(_place(s, reqs[:n], extra, fleet.now), want[:n], (name, n))
            assert s.split_batches()[0] == k + 1, (name, n)
    finally:
        s.close()


def _hostile(fleet, orc, seed, n):
    """Every row called by the first instance of the order without favourSelf: the check decides none of them."""
    reqs, extra = wl.make_requests(fleet, seed, n=n, extra_frac=0.0)
    reqs = _callers_to(reqs, fleet, np.ones(n, bool), np.full(n, orc.order[0], np.int32))
    reqs["flags"] = 0
    return reqs, extra


def _calm(fleet, seed, n):
    """Rows from callers outside the table, without exclusions of their own: only a model's own copies can lie inside a shortlist."""
    reqs, extra = wl.make_requests(fleet, seed, n=n, extra_frac=0.0)
    reqs["self_pod"] = -1
    return reqs, extra


@pytest.mark.parametrize("n", [65, 4099])
def test_a_batch_the_check_leaves_whole_then_a_normal_one(n):
    """The tail reports the rows the check LEFT (here: all of them, though the first launch decided them itself and the lists stayed
    empty), which switches the split off as tests/test_shortlist_memo_gpu.py has it; and it zeroes those words: after a commit the
    next batches' reports are their own — a stale word of n rows would be more than 1/32 of the 1 500-row batches that follow."""
    import torch
    fleet = wl.make_fleet("C2")
    orc = OracleFleet(fleet)
    bad, bad_x = _hostile(fleet, orc, 33, n)
    calm, calm_x = _calm(fleet, 34, 1500)
    want_bad, want_calm = orc.place(bad, bad_x, fleet.now, threads=8), orc.place(calm, calm_x, fleet.now, threads=8)
    s = _solver(fleet)
    st = torch.cuda.Stream()
    try:
        left = round((1.0 - covered_share(s, fleet, orc, calm, calm_x)) * len(calm))
        assert left * 32 <= len(calm) < n * 32, ("the calm batch is not calm", left)
        _same(_place(s, bad, bad_x, fleet.now, stream=st), want_bad, "every row left")
        assert s.split_batches() == (1, False)  # (the report is read by the NEXT split batch of the stream)
        _same(_place(s, calm, calm_x, fleet.now, stream=st), want_calm, "after")
        assert s.split_batches() == (1, True)
        s.commit()
        assert s.split_batches() == (1, False)
        for k in range(3):  # split, reports its own rows; the next one reads that report
            _same(_place(s, calm, calm_x, fleet.now, stream=st), want_calm, f"after the commit, {k}")
            assert s.split_batches() == (2 + k, False), k
    finally:
        s.close()


def _many_exclusions(types):
    """tests/test_shortlist_memo_gpu.py::test_more_exclusions_than_the_lane_phase_takes_next_to_requests_the_check_leaves: a sixth of
    the models with 9-12 loaded instances on a 5 000-pod table (the general path), a fifth of the callers at the head of the order."""
    fleet = wl.make_fleet("C3", models=40_000, pods=5_000)
    if types == 8:
        # 8 type rows: the staged records (4 KB) are the larger part of a wavefront's region; 4 rows: the scratch.  (A quarter of the
        # instances may host each new type: few enough for another shortlist, too many for the commit to take the table for a sparse one,
        # which would send every batch to the prefix-table kernels.)
        wl.add_sparse_types(fleet, k=fleet.n_pods // 4)
    rng = np.random.default_rng(77)
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
    reqs = reqs[:4099]
    head = orc.order[:40].astype(np.int32)
    reqs = _callers_to(reqs, fleet, rng.random(len(reqs)) < 0.2, rng.choice(head, len(reqs)))
    return fleet, orc, reqs, extra


@pytest.mark.parametrize("types", [4, 8])
def test_general_path_rows_still_reach_the_tail(types):
    """Rows only the general path decides (more exclusions than a lane takes), rows the cold lane phase decides and covered rows in
    every workgroup, three times over: the tail still decides its rows, and a wavefront's lane scratch stays inside its own region
    — with 4 type rows the 3 072 bytes of scratch are more than the staged records (2 KB), and the stride rule alone keeps the
    neighbouring wavefront's records apart."""
    fleet, orc, reqs, extra = _many_exclusions(types)
    assert fleet.n_types == types
    tot = (fleet.models["n_loaded"] + fleet.models["n_failed"])[reqs["model"]]
    assert np.count_nonzero(tot > 8) > len(reqs) // 10  # rows for the tail, in every workgroup
    want = orc.place(reqs, extra, fleet.now, threads=8)
    s = _solver(fleet)
    try:
        for rep in range(3):
            _same(_place(s, reqs, extra, fleet.now), want, (types, rep))
        assert s.split_batches()[0] == 3
    finally:
        s.close()


def test_an_empty_tail_then_a_batch_with_rest_on_the_same_stream(mixed):
    import torch
    fleet, orc, reqs, extra, want = mixed["C2"]
    calm, calm_x = _calm(fleet, 35, 4096)
    # rows whose model has no copy and no failure anywhere: nothing of their own can lie inside a shortlist
    m = fleet.models[calm["model"]]
    calm = calm[(m["n_loaded"] + m["n_failed"]) == 0][:256]
    assert len(calm) == 256
    s = _solver(fleet)
    st = torch.cuda.Stream()
    try:
        assert covered_share(s, fleet, orc, calm, calm_x) == 1.0
        _same(_place(s, calm, calm_x, fleet.now, stream=st), orc.place(calm, calm_x, fleet.now, threads=8), "fully covered")
        _same(_place(s, reqs[:257], extra, fleet.now, stream=st), want[:257], "257 mixed rows behind it")
        assert s.split_batches()[0] == 2
    finally:
        s.close()


def test_a_bad_range_row_in_a_wavefront_with_a_cold_lane(mixed):
    fleet, orc, reqs, extra, want = mixed["C2"]
    reqs = reqs[:257].copy()
    assert len(extra) > 0
    cold, bad = 69, 70  # (two lanes of the second wavefront)
    reqs[cold] = _callers_to(reqs[cold:cold + 1], fleet, np.ones(1, bool), np.full(1, orc.order[0], np.int32))[0]
    reqs["flags"][cold] = 0  # the caller is the first instance of the order, no favourSelf: the check leaves it
    reqs["extra_off"][bad], reqs["n_extra"][bad] = len(extra) - 1, 3  # runs off the pool's end
    ok = np.arange(len(reqs)) != bad
    want = orc.place(reqs[ok], extra, fleet.now, threads=8)
    s = _solver(fleet)
    try:
        got = _place(s, reqs, extra, fleet.now, how="place_dev2")
        assert got["best"][bad] == _lib.MMP_BAD_REQUEST and got["chosen"][bad] == _lib.MMP_NONE, got[bad]
        _same(got[ok], want, "the rows beside the bad one")
        assert s.split_batches()[0] == 1
    finally:
        s.close()


@pytest.mark.parametrize("n", [65, 1021])
def test_the_single_caller_form(n):
    """One caller at the head of the order for the whole batch (the check leaves what that caller's own entry would change), and one
    far from it."""
    fleet = wl.make_fleet("C2")
    orc = OracleFleet(fleet)
    reqs, extra = wl.make_requests(fleet, 43, n=n)
    s = _solver(fleet)
    try:
        for k, pod in enumerate((int(orc.order[0]), int(orc.order[3]), int(orc.order[len(orc.order) // 2]))):
            one = _callers_to(reqs, fleet, np.ones(n, bool), np.full(n, pod, np.int32))
            one["flags"], one["fresh_rpm"] = 0, 0
            _same(_place(s, one, extra, fleet.now, how="place_c_dev"), orc.place(one, extra, fleet.now, threads=8), (n, pod))
            assert s.split_batches()[0] == k + 1
    finally:
        s.close()
