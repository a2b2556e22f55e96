"""GPU: split batches (include/mmplace.h: mmp_split_batches) from several host threads, on many streams, and with work in flight.

A split batch is two launches on the call's stream: the first (place_memo_kernel) appends the indices it leaves undecided to lists
in a buffer the context keeps per stream, the second (place_tail_kernel) decides them and zeroes the lists for the stream's next
batch.  The pair must follow each other on the stream: between two threads that share one, a tail would decide the other batch's
indices with its own requests, and the other tail would find its lists empty — rows never written.  The cases here put threads on
one stream (every entry point, the NULL stream, submission threads next to direct calls, and a full cluster, whose batches are never
split), pass hipStreamPerThread (refused: it is another stream in every thread), use more streams over a context's life than it
keeps buffers for (mmp_stream_retire returns them), and grow a stream's buffer while earlier pairs are still queued.  Every result
buffer starts as 0xFF bytes (a row nobody wrote cannot pass) and every row is compared with the oracle bit for bit.

Every split batch the threads share a stream with is one the records cover (fewer than 1/32 of its rows undecided, checked first):
two or more batches' undecided indices then fit one batch's lists, and all batches of a case have the same length, so even a library
that interleaves the pairs only loses rows, never reads or writes out of bounds."""
import ctypes as C
import threading

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd import workload as wl
from modelmesh_amd.solver import Solver
from oracle.bind import OracleFleet
from tests.util import assert_same_decisions, covered_share

pytestmark = pytest.mark.gpu
EINVAL = -1
N = 65_536      # rows per batch of the threaded cases
THREADS = 4
CALLS = 24      # per thread


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _dev(a):
    torch, dev = _torch()
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)


def _outs(n):
    torch, dev = _torch()
    return torch.full((n * 16,), 0xFF, dtype=torch.uint8, device=dev)


def _rows(t):
    return np.frombuffer(t.cpu().numpy().tobytes(), dtype=_lib.PLACE_OUT)


def _one_caller(fleet, reqs, pod):
    out = reqs.copy()
    row = fleet.pods[pod]
    out["self_pod"], out["flags"], out["fresh_rpm"] = pod, 0, 0
    out["fresh_lru"], out["fresh_capacity"], out["fresh_used"], out["fresh_count"] = row["lru_time"], row["capacity"], row["used"], row["count"]
    return out


class Batch:
    """One request set on the device: rows (or a caller + 24-byte rows), its exclusion pool, the oracle's answer."""

    def __init__(self, fleet, orc, reqs, extra, one_caller=False):
        self.reqs, self.extra, self.n = reqs, extra, len(reqs)
        self.want = orc.place(reqs, extra, fleet.now, threads=8)
        self.caller = None
        if one_caller:
            self.caller, rc = _lib.split_caller(reqs)
            self.d_reqs = _dev(rc)
        else:
            self.d_reqs = _dev(reqs)
        self.d_extra = _dev(extra if len(extra) else np.zeros(1, np.int32))

    def launch(self, s, how, d_out, stream, now):
        r, e, n = self.d_reqs.data_ptr(), self.d_extra.data_ptr(), self.n
        if how == "place_dev":
            s.place_dev(r, n, e, now, d_out.data_ptr(), stream)
        elif how == "place_dev2":
            s.place_dev2(r, n, e, len(self.extra), now, d_out.data_ptr(), stream)
        else:
            assert how == "place_c_dev" and self.caller is not None
            s.place_c_dev(self.caller, r, n, e, len(self.extra), now, d_out.data_ptr(), stream)


def _check(fleet, b, out, what):
    got = _rows(out)
    assert (got["n_candidates"] >= 0).all(), (what, "rows never written", int(np.count_nonzero(got["n_candidates"] < 0)))
    assert_same_decisions(fleet, b.reqs, got, b.want)


@pytest.mark.parametrize("case", ["place_dev", "place_dev2", "place_c_dev", "null stream", "full cluster unsplit", "issue threads"])
def test_threads_sharing_one_stream_get_every_row(case, monkeypatch):
    """4 threads released together by a barrier each enqueue 24 split batches of 65 536 rows on ONE stream without synchronising
    (ctypes lets go of the GIL in the call: the launches interleave); every call writes a buffer of its own."""
    torch, dev = _torch()
    full = case == "full cluster unsplit"
    if full:  # the default route: place_batch_long_kernel
        fleet = wl.make_full_cluster(wl.make_fleet("C3"))
    else:
        monkeypatch.setenv("MMP_MEMO_FROM", "0")
        monkeypatch.setenv("MMP_SPLIT_FROM", "0")
        fleet = wl.make_fleet("C3")
    orc = OracleFleet(fleet)
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    try:
        s.load_fleet(fleet)
        sets = []
        for k in range(THREADS):
            reqs, extra = wl.make_requests(fleet, 0x5EED + 17 * k, n=N)
            if case == "place_c_dev":  # a different caller per thread, far from the head of the order (where the shortlists are)
                reqs = _one_caller(fleet, reqs, int(orc.order[-1 - 97 * k]))
            if not full:
                share = covered_share(s, fleet, orc, reqs, extra)
                assert share > 1 - 1 / 32, (k, share)  # (the safety premise of this test: see the module's docstring)
            sets.append(Batch(fleet, orc, reqs, extra, one_caller=case == "place_c_dev"))
        how = {"place_dev": "place_dev", "place_c_dev": "place_c_dev"}.get(case, "place_dev2")
        stream = 0 if case == "null stream" else torch.cuda.Stream(dev).cuda_stream
        n0 = s.split_batches()[0]
        outs = [[_outs(N) for _ in range(CALLS)] for _ in range(THREADS)]
        torch.cuda.synchronize()
        if case == "issue threads":
            assert s.lib.mmp_issue_threads(s.h, 2) == 0
        bar = threading.Barrier(THREADS)
        errors = []

        def worker(k):
            try:
                # submission threads: half the callers go through the ring (place_dev), half launch directly (place_dev2)
                mine = ("place_dev" if k % 2 == 0 else "place_dev2") if case == "issue threads" else how
                bar.wait()
                for j in range(CALLS):
                    sets[k].launch(s, mine, outs[k][j], stream, fleet.now)
            except BaseException as e:  # noqa: BLE001
                errors.append((k, e))
                bar.abort()

        ts = [threading.Thread(target=worker, args=(k,)) for k in range(THREADS)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        if case == "issue threads":
            assert s.lib.mmp_issue_flush(s.h) == 0
        torch.cuda.synchronize()
        assert not errors, errors
        for k in range(THREADS):
            for j in range(CALLS):
                _check(fleet, sets[k], outs[k][j], (case, k, j))
        n_split, off = s.split_batches()
        if full:
            assert n_split == 0, n_split
        else:
            assert n_split - n0 == THREADS * CALLS and not off, (n_split - n0, off)
    finally:
        if case == "issue threads":
            s.lib.mmp_issue_threads(s.h, 0)
        s.close()


def test_hipStreamPerThread_is_refused_by_every_entry_point_that_takes_a_stream():
    """Handle 2 names the calling thread's per-thread stream: another stream in every thread.  Every entry point refuses it with
    MMP_EINVAL before it launches anything, and says why."""
    torch, dev = _torch()
    from modelmesh_amd import dist as mdist
    per_thread = C.c_void_p(2)
    fleet = wl.make_fleet("C2")
    reqs, extra = wl.make_requests(fleet, 3, n=4096)
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    try:
        s.load_fleet(fleet)
        L = s.lib
        d_r, d_e, d_o = _dev(reqs), _dev(extra if len(extra) else np.zeros(1, np.int32)), _outs(len(reqs))
        caller, rc_rows = _lib.split_caller(_one_caller(fleet, reqs, 5))
        cp = np.ascontiguousarray(caller, dtype=_lib.PLACE_CALLER).reshape(1)
        d_rc = _dev(rc_rows)
        n = len(reqs)
        P = C.c_void_p
        arr = (P * 1)(P(d_r.data_ptr()))
        outs1 = (P * 1)(P(d_o.data_ptr()))
        ex1 = (P * 1)(P(d_e.data_ptr()))
        ns = (C.c_int32 * 1)(n)
        calls = {
            "mmp_place_batch_dev": lambda: L.mmp_place_batch_dev(s.h, P(d_r.data_ptr()), n, P(d_e.data_ptr()), fleet.now, P(d_o.data_ptr()), per_thread),
            "mmp_place_batch_dev2": lambda: L.mmp_place_batch_dev2(s.h, P(d_r.data_ptr()), n, P(d_e.data_ptr()), len(extra), fleet.now,
                                                                   P(d_o.data_ptr()), per_thread),
            "mmp_place_batch_c_dev": lambda: L.mmp_place_batch_c_dev(s.h, _lib.ptr(cp), P(d_rc.data_ptr()), n, P(d_e.data_ptr()), len(extra),
                                                                     fleet.now, P(d_o.data_ptr()), per_thread),
            "mmp_place_multi_dev": lambda: L.mmp_place_multi_dev(s.h, 1, arr, ns, ex1, fleet.now, outs1, per_thread),
            "mmp_stream_retire": lambda: L.mmp_stream_retire(s.h, per_thread),
        }
        for name, call in calls.items():
            assert call() == EINVAL, name
            msg = (L.mmp_last_error(s.h) or b"").decode()
            assert "hipStreamPerThread" in msg and name in msg, (name, msg)
        torch.cuda.synchronize()
        assert (_rows(d_o)["n_candidates"] == -1).all(), "a refused call wrote result rows"
        assert s.split_batches()[0] == 0
        # the context still answers on a stream of its own
        st = torch.cuda.Stream(dev)
        s.place_dev2(d_r.data_ptr(), n, d_e.data_ptr(), len(extra), fleet.now, d_o.data_ptr(), st.cuda_stream)
        torch.cuda.synchronize()
        assert_same_decisions(fleet, reqs, _rows(d_o), OracleFleet(fleet).place(reqs, extra, fleet.now))
        assert L.mmp_stream_retire(s.h, P(st.cuda_stream)) == 0
    finally:
        s.close()
    # the pod-axis shard calls, on a committed one-shard context
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    try:
        s.load_fleet(fleet, commit=False)
        placer = mdist.PodShardedPlacer(mdist.SolverShardBackend(s, 0, 1, dev), speculative=True)
        mdist.run_lockstep([placer.commit_steps()])
        L = s.lib
        xchg = [torch.zeros(n * max(L.mmp_shard_xchg_slots(k + 1, 1), 1), dtype=torch.int64, device=dev) for k in range(6)]
        d_x = (P * 6)(*[P(t.data_ptr()) for t in xchg])
        d_xf = torch.zeros(n * L.mmp_shard_fast_slots(), dtype=torch.int64, device=dev)
        d_o = _outs(n)
        n_rest, rr, ro = C.c_int32(0), P(), P()
        calls = {
            "mmp_shard_place_phase_dev": lambda: L.mmp_shard_place_phase_dev(s.h, 1, P(d_r.data_ptr()), n, P(d_e.data_ptr()), fleet.now, d_x,
                                                                             P(d_o.data_ptr()), per_thread),
            "mmp_shard_place_fast_dev": lambda: L.mmp_shard_place_fast_dev(s.h, P(d_r.data_ptr()), n, P(d_e.data_ptr()), fleet.now,
                                                                           P(d_xf.data_ptr()), per_thread),
            "mmp_shard_place_fast_finish_dev": lambda: L.mmp_shard_place_fast_finish_dev(s.h, P(d_r.data_ptr()), n, P(d_xf.data_ptr()),
                                                                                         P(d_o.data_ptr()), per_thread, C.byref(n_rest),
                                                                                         C.byref(rr), C.byref(ro)),
            "mmp_shard_place_fast_scatter_dev": lambda: L.mmp_shard_place_fast_scatter_dev(s.h, 0, P(d_o.data_ptr()), per_thread),
        }
        for name, call in calls.items():
            assert call() == EINVAL, name
            msg = (L.mmp_last_error(s.h) or b"").decode()
            assert "hipStreamPerThread" in msg and name in msg, (name, msg)
        torch.cuda.synchronize()
        assert (_rows(d_o)["n_candidates"] == -1).all(), "a refused call wrote result rows"
        assert not d_xf.any().item(), "a refused call wrote the exchange buffer"
    finally:
        s.close()


def test_streams_beyond_the_buffers_a_context_keeps_split_again_after_retire(monkeypatch):
    """70 streams, a split batch on each: the first 64 get a buffer and split, the rest go unsplit (same rows).  After every stream
    is retired (and destroyed), 8 new streams split again: retire gave the buffers back."""
    torch, dev = _torch()
    monkeypatch.setenv("MMP_MEMO_FROM", "0")
    monkeypatch.setenv("MMP_SPLIT_FROM", "0")
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    fleet = wl.make_fleet("C3")
    orc = OracleFleet(fleet)
    reqs, extra = wl.make_requests(fleet, 0x57EA, n=40_000)
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    made = []

    def new_stream():
        h = C.c_void_p()
        assert hip.hipStreamCreateWithFlags(C.byref(h), 1) == 0  # hipStreamNonBlocking
        made.append(h.value)
        return h.value

    try:
        s.load_fleet(fleet)
        assert covered_share(s, fleet, orc, reqs, extra) > 1 - 1 / 32
        b = Batch(fleet, orc, reqs, extra)
        streams = [new_stream() for _ in range(70)]
        assert len(set(streams)) == 70
        for i, st in enumerate(streams):
            o = _outs(b.n)
            b.launch(s, "place_dev2", o, st, fleet.now)
            torch.cuda.synchronize()
            _check(fleet, b, o, ("stream", i))
        assert s.split_batches() == (64, False), s.split_batches()
        for st in streams:
            assert s.lib.mmp_stream_retire(s.h, C.c_void_p(st)) == 0
        # (the retired streams are destroyed only after the new ones exist: no new handle can repeat a retired one's)
        fresh = [new_stream() for _ in range(8)]
        assert not set(fresh) & set(streams)
        for st in streams:
            assert hip.hipStreamDestroy(C.c_void_p(st)) == 0
            made.remove(st)
        for i, st in enumerate(fresh):
            o = _outs(b.n)
            b.launch(s, "place_dev2", o, st, fleet.now)
            torch.cuda.synchronize()
            _check(fleet, b, o, ("new stream", i))
        assert s.split_batches() == (64 + 8, False), s.split_batches()
        for st in fresh:
            assert s.lib.mmp_stream_retire(s.h, C.c_void_p(st)) == 0
    finally:
        s.close()
        torch.cuda.synchronize()
        for st in made:
            hip.hipStreamDestroy(C.c_void_p(st))


@pytest.mark.parametrize("env", ["default", "split from 0"])
def test_a_stream_buffer_grows_while_earlier_pairs_are_queued(env, monkeypatch):
    """One stream, one thread, no synchronisation: 50 000, 400 000, 60 000 and 800 000 rows, each into a buffer of its own.  The
    stream's buffer is reallocated for the larger batches while the pairs in front of them still read the old one."""
    torch, dev = _torch()
    if env != "default":
        monkeypatch.setenv("MMP_SPLIT_FROM", "0")
        monkeypatch.setenv("MMP_MEMO_FROM", "0")
    fleet = wl.make_fleet("C3")
    orc = OracleFleet(fleet)
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    try:
        s.load_fleet(fleet)
        batches = []
        for k, n in enumerate((50_000, 400_000, 60_000, 800_000)):
            parts, ex_parts, off = [], [], 0
            for j in range(-(-n // fleet.n_models)):
                rq, ex = wl.make_requests(fleet, seed=0x6000 + 10 * k + j)
                rq = rq.copy()
                rq["extra_off"] += off
                off += len(ex)
                parts.append(rq)
                ex_parts.append(ex)
            reqs, extra = np.concatenate(parts)[:n], np.concatenate(ex_parts)
            assert covered_share(s, fleet, orc, reqs, extra) > 1 - 1 / 32
            batches.append(Batch(fleet, orc, reqs, extra))
        st = torch.cuda.Stream(dev)
        outs = [_outs(b.n) for b in batches]
        torch.cuda.synchronize()
        for b, o in zip(batches, outs):
            b.launch(s, "place_dev2", o, st.cuda_stream, fleet.now)
        torch.cuda.synchronize()
        for b, o in zip(batches, outs):
            _check(fleet, b, o, (env, b.n))
        n_split, off = s.split_batches()
        assert not off
        assert n_split == (4 if env != "default" else 2), n_split  # (by default: the batches from 393 216 rows)
        assert s.lib.mmp_stream_retire(s.h, C.c_void_p(st.cuda_stream)) == 0
    finally:
        s.close()
