"""GPU: the split form's tail launch as workgroups of ONE wavefront (place_kernel.hpp: place_tail_body, place_block<..., NOBAR, LIST>),
gated by one line of the stream's buffer: a tail wavefront reads the call's gate word, leaves if the first launch appended nothing, and
otherwise decides its lists 64 entries a pass; the report comes from the same word, and the word of the stream's NEXT call is zeroed by
this call's tail.

Every batch takes the split route (MMP_MEMO_FROM=0, MMP_SPLIT_FROM=0) from device memory, the result buffers start as 0xFF bytes, and
all four fields of every row are compared with the oracle.  Rows reach the tail's lists as in tests/test_split_rest_in_wave_gpu.py:
their model has more loaded instances than a lane takes exclusions (8), so only the general path decides them."""
import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd import workload as wl
from modelmesh_amd.solver import Solver
from oracle.bind import OracleFleet
from tests.util import covered_share

pytestmark = pytest.mark.gpu
FIELDS = ("chosen", "best", "n_candidates", "hash")
SIZES = (1, 63, 64, 65, 255, 256, 257, 1021, 4097)
HOWS = ("place_dev", "place_c_dev")
FRESH = (("fresh_lru", "lru_time"), ("fresh_capacity", "capacity"), ("fresh_used", "used"), ("fresh_count", "count"))
# instances: neither a multiple of 64.  5 000: a wavefront's 64 scratch columns (3 072 bytes) are more than the general path's two
# tiles (2 x 80 words); 20 011: the tiles (2 x 314 words = 5 024 bytes) are the larger part of the one-wavefront LDS region.
PODS = (5_000, 20_011)


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


class _Batch:
    """A batch in device memory (uploaded and waited for), its result buffer prefilled with 0xFF; go() enqueues it and waits for
    nothing."""

    def __init__(self, reqs, extra, how):
        import torch
        self.n, self.how, self.n_extra = len(reqs), how, len(extra)
        self.caller = None
        if how == "place_c_dev":
            self.caller, reqs = _lib.split_caller(reqs)
        self.d_r, self.d_x = _dev(reqs), _dev(extra)
        self.d_o = torch.full((self.n * _lib.PLACE_OUT.itemsize,), 0xFF, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()

    def go(self, s, now, st):
        x = self.d_x.data_ptr() if self.n_extra else 0
        if self.how == "place_c_dev":
            s.place_c_dev(self.caller, self.d_r.data_ptr(), self.n, x, self.n_extra, now, self.d_o.data_ptr(), st.cuda_stream)
        else:
            s.place_dev(self.d_r.data_ptr(), self.n, x, now, self.d_o.data_ptr(), st.cuda_stream)
        return self

    def rows(self):
        """(after a device-wide wait) the result rows"""
        import torch
        torch.cuda.synchronize()
        return np.frombuffer(self.d_o.cpu().numpy().tobytes(), dtype=_lib.PLACE_OUT)[:self.n]


def _place(s, reqs, extra, now, how, stream=None):
    import torch
    return _Batch(reqs, extra, how).go(s, now, stream or torch.cuda.Stream()).rows()


def _same(got, want, what):
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f, int(np.flatnonzero(got[f] != want[f])[0]))


def _one_caller(reqs, fleet, pod):
    """The rows as instance `pod` issues them all (the single-caller form takes one caller per batch)."""
    out = reqs.copy()
    out["self_pod"] = pod
    for f, g in FRESH:
        out[f] = fleet.pods[pod][g] if pod >= 0 else 0  # (a caller outside the table has no row)
    out["flags"], out["fresh_rpm"] = 0, 0
    return out


class _Case:
    """A C3-shaped fleet of `pods` instances in which a sixth of the models have 9-12 loaded instances (the general path), with: `mixed`
    — 4 097 rows, a fifth of the callers at the head of the placement order (rows the check leaves and the head window decides), a
    sixth for the lists, the rest the check's; `lists` — 4 097 rows that ALL reach the lists; `calm` — 4 097 rows of which none does
    (callers outside the table, no exclusions, models without a copy anywhere).  Each with the oracle's answer, computed once; the
    single-caller form's rows are the same with one caller for the batch."""

    def __init__(self, pods):
        fleet = wl.make_fleet("C3", models=40_000, pods=pods)
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
        self.fleet, self.orc = fleet, OracleFleet(fleet)
        self.tot = fleet.models["n_loaded"] + fleet.models["n_failed"]
        n = max(SIZES)
        every, extra = wl.make_requests(fleet, 5)
        self.extra = extra
        head = self.orc.order[:40].astype(np.int32)
        mixed = every[:n].copy()
        sel = rng.random(n) < 0.2
        mixed["self_pod"] = np.where(sel, rng.choice(head, n), mixed["self_pod"])
        for f, g in FRESH:
            mixed[f] = np.where(sel, fleet.pods[mixed["self_pod"]][g], mixed[f])
        lists = every[self.tot[every["model"]] > 8][:n].copy()
        quiet, _ = wl.make_requests(fleet, 6, extra_frac=0.0)
        quiet["self_pod"] = -1
        calm = quiet[self.tot[quiet["model"]] == 0][:n].copy()
        # the CPU's word on what the batches hold: rows for the lists in every workgroup of `mixed`, nothing else in `lists`, none in `calm`
        assert len(lists) == n and len(calm) == n, (len(lists), len(calm))
        assert np.all(self.tot[lists["model"]] > 8) and np.all(self.tot[calm["model"]] == 0)
        per_wg = np.add.reduceat((self.tot[mixed["model"]] > 8).astype(np.int64), np.arange(0, n, 256))
        assert per_wg[:-1].min() >= 8, per_wg
        self.batches = {}
        for name, rows in (("mixed", mixed), ("lists", lists), ("calm", calm)):
            self.batches[name, "place_dev"] = rows
            # one caller for the batch: the second instance of the order (its own entry lies inside the shortlists)
            self.batches[name, "place_c_dev"] = _one_caller(rows, fleet, int(self.orc.order[1])) if name != "calm" else _one_caller(rows, fleet, -1)
        self.want = {key: self.orc.place(rows, extra, fleet.now, threads=8) for key, rows in self.batches.items()}

    def lists_reached(self, name, how, n):
        """rows of the batch's first n that only the general path decides"""
        return int(np.count_nonzero(self.tot[self.batches[name, how]["model"][:n]] > 8))


_cases = {}


@pytest.fixture(scope="module", params=PODS)
def case(request):
    if request.param not in _cases:
        _cases[request.param] = _Case(request.param)
    return _cases[request.param]


@pytest.fixture(scope="module")
def narrow():
    if PODS[0] not in _cases:
        _cases[PODS[0]] = _Case(PODS[0])
    return _cases[PODS[0]]


@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("name", ["calm", "mixed", "lists"])
def test_every_size_on_both_fleets(case, name, how):
    """Nothing in the lists / rows for the lists next to rows the check and the head window decide / every row in the lists, at every
    size, on a table whose one-wavefront LDS region is its scratch columns and on one where it is the general path's tiles."""
    reqs, want = case.batches[name, how], case.want[name, how]
    assert case.fleet.n_pods % 64 != 0
    s = _solver(case.fleet)
    try:
        if name == "calm" and how == "place_dev" and case.fleet.n_pods == PODS[0]:
            # (the narrow table: the check itself decides every calm row.  On the wide one the commit records no valid shortlist, the
            # check leaves every row and the cold branch asks the head window: rows without an exclusion of their own.)
            assert covered_share(s, case.fleet, case.orc, reqs, case.extra) == 1.0
        for k, n in enumerate(SIZES):
            if name != "mixed":
                assert case.lists_reached(name, how, n) == (n if name == "lists" else 0)
            _same(_place(s, reqs[:n], case.extra, case.fleet.now, how), want[:n], (case.fleet.n_pods, name, how, n))
            assert s.split_batches()[0] == k + 1, (name, how, n)
    finally:
        s.close()


@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("blocks", ["64", "16", "5", "1"])
def test_a_list_longer_than_a_pass_and_a_wavefront_with_several_lists(narrow, monkeypatch, blocks, how):
    """4 097 rows that all reach the lists: 65 wavefronts of the first launch, so list 0 holds 65 entries — two passes of 64 — and with
    16 / 5 / 1 tail wavefronts each owns 4 / 13 / 64 lists and walks them entry by entry (no entry skipped: a row nobody decided is
    0xFF bytes)."""
    monkeypatch.setenv("MMP_TAIL_BLOCKS", blocks)
    c = narrow
    reqs, want = c.batches["lists", how], c.want["lists", how]
    n = len(reqs)
    assert c.lists_reached("lists", how, n) == n == 4097
    s = _solver(c.fleet)
    try:
        _same(_place(s, reqs, c.extra, c.fleet.now, how), want, (blocks, how))
        _same(_place(s, reqs[:1021], c.extra, c.fleet.now, how), want[:1021], (blocks, how, 1021))
        assert s.split_batches()[0] == 2
    finally:
        s.close()


def _few_for_the_lists(c, how, seed):
    """4 097 rows, 100 of them for the lists (scattered), the others fully covered: the check leaves 100 rows — not more than 1/32 of the
    batch, while the rows of TWO such batches together are."""
    n = 4097
    rng = np.random.default_rng(seed)
    at = np.sort(rng.choice(n, 100, replace=False))
    calm = c.batches["calm", how]
    rows, want = calm.copy(), c.want["calm", how].copy()
    src = rng.choice(n, 100, replace=False)
    from_lists = c.batches["lists", how][src]
    if how == "place_c_dev":  # (one caller for the batch: the calm batch's)
        from_lists = _one_caller(from_lists, c.fleet, -1)
        w = c.orc.place(from_lists, c.extra, c.fleet.now, threads=8)
    else:
        w = c.want["lists", how][src]
    rows[at], want[at] = from_lists, w
    assert 100 * 32 <= n < 200 * 32
    return rows, want


@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("streams", [1, 2])
def test_back_to_back_rows_none_rows_and_the_report(narrow, how, streams):
    """Three batches on a stream with no host wait between them — rows in the lists, none, rows — on one stream and on two alternately:
    a gate word that is not zero again when the stream's next first launch appends would show as rows of an EARLIER batch in a later
    report (two batches' rows together are more than 1/32 of a batch: the split would be switched off), one zeroed before its tail has
    read it as rows nobody decided."""
    import torch
    c = narrow
    a, want_a = _few_for_the_lists(c, how, 1)
    b, want_b = c.batches["calm", how][:1021], c.want["calm", how][:1021]
    d, want_d = _few_for_the_lists(c, how, 2)
    s = _solver(c.fleet)
    sts = [torch.cuda.Stream() for _ in range(streams)]
    try:
        assert covered_share(s, c.fleet, c.orc, c.batches["calm", "place_dev"], c.extra) == 1.0
        outs = [(_Batch(rows, c.extra, how), want) for rows, want in ((a, want_a), (b, want_b), (d, want_d)) for st in sts]
        for k, (bt, want) in enumerate(outs):  # a, a', b, b', d, d': per stream rows, none, rows
            bt.go(s, c.fleet.now, sts[k % streams])
        for k, (bt, want) in enumerate(outs):
            _same(bt.rows(), want, (how, streams, k))
        assert s.split_batches() == (3 * streams, False)
        # the third tails' reports, read by the streams' next split batches: their own 100 rows, not 200
        for rows, want, count in ((b, want_b, 4), (a, want_a, 5)):
            more = [_Batch(rows, c.extra, how) for st in sts]
            for bt, st in zip(more, sts):
                bt.go(s, c.fleet.now, st)
            for bt in more:
                _same(bt.rows(), want, (how, streams, count))
            assert s.split_batches() == (count * streams, False)
    finally:
        s.close()
