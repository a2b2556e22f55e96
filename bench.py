#!/usr/bin/env python
"""bench.py — placement decisions/sec on the BASELINE.json headline config.

A "step" is one pass of the hot path over one batch: 100k load-target decisions
(one per model, CacheMissForwardingLB.getNext semantics) against a committed
10k-pod snapshot (config C3), with requests, model table and outputs already
resident in HBM.  The timed steps rotate through --batches DISTINCT request
batches (default 48 x 6.4 MB of requests + 48 x 1.6 MB of results = 384 MB, more
than the 256 MiB Infinity Cache), each with its own result buffer, issued
round-robin on --streams HIP streams: a step's requests come from HBM, not from
a cache the previous step warmed.  Every stream and every batch is used once
before the warm-up steps (setup, untimed), so the timed region does not depend
on --warmup.  N>1 (torch.distributed.run, one rank per GPU): decisions are
independent, so ranks shard the model axis with no data-path collective and the
line reports weak scaling (100k decisions per rank per step).

Prints ONE JSON line on rank 0 (contract in the task statement).  A plain run
does only what the headline needs: set-up, warm-up, the timed steps and the
line (`value`, `ms_per_step`, `config`).  `--full` adds everything else the
bench measures or checks: the kernel-duration passes and `roofline`, the parity
gate against the CPU oracle, and the additional legs (`pod_axis`, latency,
`churn`, `full_cluster`, per-kernel `kernels`, `cpu_baseline`, ...).
`--dump-outputs DIR` writes the result rows of the last timed step as
DIR/<field>.npy (float64).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# HIP maps streams onto a pool of hardware queues (4 by default), and the library's own streams take part in the
# rotation: with the default pool the 4 streams of the timed region shared ~2 queues (4.86 us per step); with 8 queues
# they each get one (3.64 us).  Must be in the environment before the HIP runtime initialises (measured, round 2:
# pool 2 / 4 / 8 / 16 -> 4.88 / 4.86 / 3.64 / 3.67 us per step at 4 streams; INTEGRATION.md recommends the same to hosts).
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def algorithmic_bytes(fleet, reqs) -> int:
    """bytes(d) = 32*P + (24 + 12*(k+f) + 4*e) + 16 summed over the batch."""
    m = fleet.models[reqs["model"]]
    per = 32 * fleet.n_pods + 24 + 12 * (m["n_loaded"].astype(np.int64) + m["n_failed"]) + 4 * reqs["n_extra"] + 16
    return int(per.sum())


def kernel_bytes(fleet, reqs) -> int:
    """What a launch asks the memory system for per batch: request (64 B) + model row (24 B) + the
    model's instanceIds / failedIn / per-request exclusions (4 B each, plus a 4 B rank-position lookup
    each) + result (16 B).  Only the request and the result are STREAMS (hbm_stream_bytes): the registry view is a 3.2 MB table
    on C3 that every launch re-reads — L2 misses on it are served by the Infinity Cache (the FETCH_SIZE counter includes them,
    VERDICT r4 weak 2), not by HBM.  The rank-ordered bitmaps and per-pod columns a decision touches (a few 64-pod
    words near the head of the order) are shared by all decisions and stay in L2."""
    m = fleet.models[reqs["model"]]
    per = 64 + 24 + 8 * (m["n_loaded"].astype(np.int64) + m["n_failed"] + reqs["n_extra"]) + 16
    return int(per.sum())


def hbm_stream_bytes(n_decisions: int, request_bytes: int = 64) -> int:
    """The bytes of a launch that can only come from / go to HBM: the request stream and the result rows (16 B)."""
    return int(n_decisions) * (request_bytes + 16)


class NodeBarrier:
    """Barrier across the ranks of ONE node through a page of shared memory (/dev/shm): rank r publishes the number of
    the barrier it has reached in a cache line of its own and waits until every rank has published at least that number.
    A few microseconds, against 30-60 us for `dist.barrier()` on the RCCL backend (a one-element all-reduce launched on
    the device plus a stream wait) — which matters when the region it closes is 400 us.  The driver's contract is one
    node (`--nnodes=1`); `create()` returns None when the ranks are not all local or /dev/shm is unusable, and the caller
    keeps `dist.barrier()`.  A wait that lasts 60 s raises instead of spinning forever."""
    STRIDE = 8  # int64 slots per rank: one 64-byte line each

    def __init__(self, mm, rank, world, path):
        self.mm, self.rank, self.world, self.path, self.epoch = mm, rank, world, path, 0
        self.view = mm[:world * self.STRIDE:self.STRIDE]

    @classmethod
    def create(cls, rank, world, dist_mod):
        try:
            if int(os.environ.get("LOCAL_WORLD_SIZE", str(world))) != world or not os.path.isdir("/dev/shm"):
                return None
            path = f"/dev/shm/mmp_bench_barrier_{os.environ.get('MASTER_PORT', '0')}"  # one rendezvous port = one job on this node
            if rank == 0:
                np.zeros(world * cls.STRIDE, np.int64).tofile(path)
            dist_mod.barrier()  # the file exists and is zeroed before anybody maps it
            ok = os.path.exists(path)
            mm = np.memmap(path, dtype=np.int64, mode="r+", shape=(world * cls.STRIDE,)) if ok else None
            flags = [None] * world
            dist_mod.all_gather_object(flags, bool(ok))  # all or nothing: a rank without the page sends everybody back to dist.barrier()
            if all(flags):
                return cls(mm, rank, world, path)
            if rank == 0 and ok:
                os.unlink(path)
            return None
        except Exception:
            return None

    def wait(self):
        self.epoch += 1
        e = self.epoch
        self.mm[self.rank * self.STRIDE] = e
        view = self.view
        if view.min() >= e:
            return
        t0 = time.perf_counter()
        spins = 0
        while view.min() < e:
            spins += 1
            if (spins & 0xFFFF) == 0 and time.perf_counter() - t0 > 60.0:
                raise RuntimeError(f"NodeBarrier: rank {self.rank} waited 60 s at barrier {e}: {view.tolist()}")

    def close(self):
        try:
            del self.view, self.mm
            if self.rank == 0:
                os.unlink(self.path)
        except Exception:
            pass


def make_step_batch(fleet, seeds):
    """One step's batch: a request set (one load-target decision per model, wl.make_requests) per seed, concatenated;
    the exclusion-pool offsets of a set move behind the pools of the sets before it.  Returns (requests, pool, length of
    the first set's pool) — the first `fleet.n_models` requests with the first `length` pool entries are set 0 unchanged."""
    from modelmesh_amd import workload as wl
    parts, ex_parts, off = [], [], 0
    for seed in seeds:
        rq, ex = wl.make_requests(fleet, seed=seed)
        if off:
            rq = rq.copy()
            rq["extra_off"] += off
        parts.append(rq)
        ex_parts.append(ex)
        off += len(ex)
    if len(parts) == 1:
        return parts[0], ex_parts[0], len(ex_parts[0])
    return np.concatenate(parts), np.concatenate(ex_parts), len(ex_parts[0])


DUMP_LIMIT_BYTES = 64_000_000 - 4096  # 64 MB in all, with room for the .npy headers


def dump_outputs(out_dir: str, rows) -> None:
    """`rows`: the PLACE_OUT result rows of one step.  One float64 array per field (32-bit integers: exact in float64); above
    DUMP_LIMIT_BYTES a fixed seeded sample of rows, whose indices go to row.npy."""
    names = rows.dtype.names
    if len(rows) * 8 * len(names) > DUMP_LIMIT_BYTES:
        k = DUMP_LIMIT_BYTES // (8 * (len(names) + 1))
        idx = np.sort(np.random.default_rng(0).choice(len(rows), k, replace=False))
        rows = rows[idx]
    else:
        idx = None
    os.makedirs(out_dir, exist_ok=True)
    for f in names:
        np.save(os.path.join(out_dir, f"{f}.npy"), rows[f].astype(np.float64))
    if idx is not None:
        np.save(os.path.join(out_dir, "row.npy"), idx.astype(np.float64))


def measured_traffic(workload: str, decisions_per_launch: int, kernel: str = "place_batch_kernel", tag: str = ""):
    """HBM bytes per place_batch_kernel launch from the committed rocprofv3 PMC passes of this same
    command (profiles/rNN/pmc_place_batch_<workload>*.json, written by tools/pmc_summary.py), and where the figure comes
    from.  A summary counts only if (a) it was taken AT THIS LAUNCH SIZE (its write bytes are the 16-byte result rows of
    one launch, which identifies the size) and (b) it is stamped with the hash of the kernel sources of THIS tree
    (tools/kernel_hash.py): a kernel change that alters the traffic must not keep an old number.  -> (bytes | None, provenance)"""
    import glob
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_hash import kernel_source_hash
    now_hash = kernel_source_hash()
    best, prov = None, f"no PMC summary for {workload} at {decisions_per_launch} decisions per launch under profiles/"
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", f"pmc_place_batch_{workload}{tag}*.json"))):
        try:
            j = json.load(open(f))
        except Exception:
            continue
        if j.get("kernel", kernel) != kernel:
            continue
        if tag:  # a tagged summary names its launch size itself (its writes are not only result rows)
            if not f.endswith(f"{tag}_{decisions_per_launch // 1000}k.json"):
                continue
        elif abs(j.get("write_bytes", 0) / 16 - decisions_per_launch) > 0.02 * decisions_per_launch:
            continue
        rel = os.path.relpath(f, ROOT)
        if j.get("kernel_source_hash") != now_hash:
            if best is None:
                prov = (f"{rel} was taken on other kernel sources ({j.get('kernel_source_hash', 'unstamped')} != {now_hash}): "
                        "not used, the compulsory streams stand in")
            continue
        best, prov = j.get("traffic_bytes_per_launch"), f"{rel} (rocprofv3 FETCH_SIZE x 2 + WRITE_SIZE, kernel sources {now_hash})"
    return best, prov


def cpu_baseline(fleet, reqs, extra, budget_s: float = 6.0):
    """The reference ALGORITHM on this box's host cores: oracle/mm_oracle.c:orc_place_lean — the getNext
    restatement (lazy walk of the PLACEMENT_ORDER list with the filter, sequential breaks, rpm rule) without the
    checker's audit machinery (no per-call allocation, no pos_of rebuild, no shortlist hash) — rebuilt here with
    gcc -O2 -march=native, on a persistent worker pool (one thread / all cores).  Not the JVM."""
    from oracle.bind import OracleFleet
    orc = OracleFleet(fleet)
    hw_threads = os.cpu_count() or 1
    # the threads this process may actually RUN: the affinity mask, capped by the CPU time its cgroup grants (the GPU box
    # shows 256 hardware threads and grants 16 CPUs' worth: 256 workers fighting over that quota measured 5x one thread)
    affinity = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else hw_threads
    quota = _cgroup_cpu_limit()
    cores = usable_cpus()
    out, flags = {}, ""
    lat = None
    for label, th in (("single", 1), ("all", cores)):
        pool = orc.lean_pool(th)
        flags = pool.flags
        try:
            pool(reqs[:2000], extra, fleet.now)  # threads started, code and tables touched
            # one pool call = one wake-up of every worker: give each at least ~8k decisions per call (the 100k batch
            # repeated), or the condition-variable round trip is what gets timed on a many-core host
            rep = max(1, -(-th * 8192 // len(reqs)))
            work = np.tile(reqs, rep) if rep > 1 else reqs
            n_done, t0 = 0, time.perf_counter()
            while True:
                pool(work, extra, fleet.now)
                n_done += len(work)
                dt = time.perf_counter() - t0
                if dt >= budget_s:
                    break
            out[label] = n_done / dt
            if th == 1:
                _, lat = pool(reqs[:20000], extra, fleet.now, latencies=True)
        finally:
            pool.close()
    return {
        "value": out["all"], "unit": "decisions/s", "cores": cores, "kind": "port",
        "sample": f"{len(reqs)} C3 decisions repeated for ~{budget_s:.0f}s per leg (1 thread, then {cores} threads on a "
                  f"persistent pool, >= 8k decisions per thread per call); CPU port of the reference algorithm (oracle/mm_oracle.c:orc_place_lean, gcc {flags}), "
                  "not the JVM",
        "single_thread_value": out["single"],
        "scaling_vs_single_thread": out["all"] / out["single"] if out["single"] else None,
        "p50_us": float(np.percentile(lat, 50) / 1e3), "p99_us": float(np.percentile(lat, 99) / 1e3),
        # `cores` = worker threads used = min(affinity mask, cgroup CPU quota); the box's hardware threads are listed apart
        "hw_threads": hw_threads, "cgroup_cpu_limit": quota, "affinity_cpus": affinity,
    }


def usable_cpus() -> int:
    """Threads this process can actually run at once: the affinity mask capped by the cgroup's CPU quota."""
    affinity = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = _cgroup_cpu_limit()
    return max(1, min(affinity, int(np.ceil(quota)) if quota else affinity))


def _cgroup_cpu_limit():
    """CPUs' worth of time the container's cgroup grants (cpu.max quota / period); None: unlimited or not readable"""
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        return None if quota == "max" else float(quota) / float(period)
    except Exception:
        return None


def pod_axis_leg(workload: str, rank: int, world: int, dev, steps: int, warmup: int, fence):
    """The same decisions with the POD axis sharded across the ranks (BASELINE.json
    config C4): every rank sees the whole batch and owns 1/world of the PLACEMENT_ORDER positions.  A
    batch takes the speculative form first — every shard decides on its own slice, ONE RCCL
    all-reduce(MIN) of 2 int64 per decision picks the lowest shard holding an eligible pod — and the
    decisions that shard could not finish alone take the six-exchange protocol as a compacted sub-batch
    (modelmesh_amd.dist.PodShardedPlacer).  Strong scaling of the pod table, not of the batch: value =
    decisions of ONE batch / time."""
    import torch
    import torch.distributed as dist

    from modelmesh_amd import dist as mdist
    from modelmesh_amd import workload as wl
    from modelmesh_amd._lib import PLACE_OUT
    from modelmesh_amd.solver import Solver

    fleet = wl.make_fleet(workload)
    reqs, extra = wl.make_requests(fleet, seed=0xBE7C0)  # identical on every rank
    n = len(reqs)
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms, device=dev.index)
    s.load_fleet(fleet, commit=False)
    placer = mdist.PodShardedPlacer(mdist.SolverShardBackend(s, rank, world, dev))
    t0 = time.perf_counter()
    placer.commit()
    commit_ms = (time.perf_counter() - t0) * 1e3
    d_reqs = torch.from_numpy(reqs.view(np.uint8).reshape(-1)).to(dev)
    d_extra = torch.from_numpy(np.ascontiguousarray(extra if len(extra) else np.zeros(1, np.int32))).to(dev)
    d_outs = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    for _ in range(warmup):
        placer.place(d_reqs, n, d_extra, fleet.now, d_outs)
    fence()
    t0 = time.perf_counter()
    for _ in range(steps):
        placer.place(d_reqs, n, d_extra, fleet.now, d_outs)
    fence()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    got = np.frombuffer(d_outs.cpu().numpy().tobytes(), dtype=PLACE_OUT)
    out = None
    if rank == 0:
        from oracle.bind import OracleFleet
        want = OracleFleet(fleet).place(reqs, extra, fleet.now, threads=os.cpu_count() or 1)
        parity = bool(all(np.array_equal(got[f], want[f]) for f in ("chosen", "best", "n_candidates", "hash")))
        slots = sum(s.shard_xchg_slots(ph) for ph in range(1, 7))
        n_rest = placer.last_n_rest
        out = {"workload": f"{workload}: {fleet.n_models} models x {fleet.n_pods} pods", "n_shards": world,
               "value": n * steps / elapsed, "unit": "decisions/s", "ms_per_step": elapsed / steps * 1e3,
               "decisions_per_step": n, "scaling": "strong (pod table split, batch replicated)",
               "collective": ("1 x all_reduce(MIN, 2 int64 per decision) + 6 x all_reduce(int64; MIN x5, SUM x1) over the "
                              "undecided rest, via torch.distributed (RCCL)") if world > 1 else "none (1 shard)",
               "decided_by_the_single_exchange": n - n_rest, "took_the_six_phase_protocol": n_rest,
               "allreduce_bytes_per_step": 8 * s.shard_fast_slots() * n + 8 * slots * n_rest,
               "allreduce_bytes_per_step_six_phase_only": 8 * slots * n, "sharded_commit_ms": commit_ms,
               "parity_vs_oracle": parity}
    s.close()
    return out


def _gloo_exchange_callback():
    """mmp_exchange_fn over torch.distributed's (gloo) process group: what lets SEVERAL ranks on ONE device run the in-library
    group protocol (RCCL refuses two ranks on one device) — the driver's 8-GPU run takes RCCL instead; this exists so that every
    other line of the N-rank control flow has executed on a 1-GPU box before it."""
    import ctypes as C

    import torch
    import torch.distributed as dist
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    xfn = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p)

    def fn(_user, dev_buf, count, elem64, op_min, stream):
        try:
            t = torch.empty(int(count), dtype=torch.int64 if elem64 else torch.int32)
            nbytes = t.numel() * t.element_size()
            if hip.hipStreamSynchronize(stream) != 0 or hip.hipMemcpy(t.data_ptr(), dev_buf, nbytes, 2) != 0:
                return 1
            dist.all_reduce(t, op=dist.ReduceOp.MIN if op_min else dist.ReduceOp.SUM)
            return 0 if hip.hipMemcpy(dev_buf, t.data_ptr(), nbytes, 1) == 0 else 1
        except Exception:  # noqa: BLE001 (a C callback must not raise)
            return 1
    return xfn(fn)


def pod_axis_lib_leg(workload: str, rank: int, world: int, dev, steps: int, warmup: int, fence, exchange: str = "rccl"):
    """The same pod-axis batch with the collectives INSIDE libmmplace (include/mmplace.h: mmp_shard_group_init /
    mmp_shard_commit / mmp_shard_place_batch_dev): ncclCommInitRank from a unique id that rank 0 creates through the
    library and torch.distributed only broadcasts; every ncclAllReduce runs on the library's own stream, and the rest
    count of the speculative form never leaves the device.  This is the path a Java mesh reaches through JNI."""
    import torch
    import torch.distributed as dist

    from modelmesh_amd import workload as wl
    from modelmesh_amd._lib import PLACE_OUT
    from modelmesh_amd.solver import Solver

    fleet = wl.make_fleet(workload)
    reqs, extra = wl.make_requests(fleet, seed=0xBE7C0)  # identical on every rank
    n = len(reqs)
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms, device=dev.index)
    cb = None
    try:
        if exchange == "gloo":  # the host moves the exchange words (mmp_shard_group_set_exchange): several ranks on one device
            import ctypes as C
            cb = _gloo_exchange_callback()
            rc = s.lib.mmp_shard_group_set_exchange(s.h, C.cast(cb, C.c_void_p), None)
            if rc != 0:
                raise RuntimeError(f"mmp_shard_group_set_exchange: {rc}")
            s.shard_group_init(None, rank, world)
        else:
            idt = torch.zeros(128, dtype=torch.uint8, device=dev)
            if rank == 0:
                idt.copy_(torch.frombuffer(bytearray(s.shard_unique_id()), dtype=torch.uint8))
            if world > 1:
                dist.broadcast(idt, src=0)
            torch.cuda.synchronize(dev)
            s.shard_group_init(bytes(idt.cpu().numpy().tobytes()), rank, world)
        s.load_fleet(fleet, commit=False)
        t0 = time.perf_counter()
        s.shard_commit()
        commit_ms = (time.perf_counter() - t0) * 1e3
        d_reqs = torch.from_numpy(reqs.view(np.uint8).reshape(-1)).to(dev)
        d_extra = torch.from_numpy(np.ascontiguousarray(extra if len(extra) else np.zeros(1, np.int32))).to(dev)
        d_outs = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        n_rest = 0
        for _ in range(warmup):
            n_rest = s.shard_place_dev(d_reqs.data_ptr(), n, d_extra.data_ptr(), fleet.now, d_outs.data_ptr())
        fence()
        t0 = time.perf_counter()
        for _ in range(steps):
            n_rest = s.shard_place_dev(d_reqs.data_ptr(), n, d_extra.data_ptr(), fleet.now, d_outs.data_ptr())
        fence()
        elapsed = time.perf_counter() - t0
        # the same batches without the host synchronisation at the end of each (mmp_shard_place_batch_async_dev: a batch is
        # completed — its rest count read, the six phases run if there is a rest — when the next one is issued; one wait at the end)
        fence()
        t0 = time.perf_counter()
        for _ in range(steps):
            s.shard_place_async_dev(d_reqs.data_ptr(), n, d_extra.data_ptr(), fleet.now, d_outs.data_ptr())
        n_rest_async = s.shard_wait()
        fence()
        elapsed_async = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([elapsed, elapsed_async], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed, elapsed_async = float(t[0].item()), float(t[1].item())
        got = np.frombuffer(d_outs.cpu().numpy().tobytes(), dtype=PLACE_OUT)
        out = None
        if rank == 0:
            from oracle.bind import OracleFleet
            want = OracleFleet(fleet).place(reqs, extra, fleet.now, threads=os.cpu_count() or 1)
            parity = bool(all(np.array_equal(got[f], want[f]) for f in ("chosen", "best", "n_candidates", "hash")))
            slots = sum(s.shard_xchg_slots(ph) for ph in range(1, 7))
            out = {"workload": f"{workload}: {fleet.n_models} models x {fleet.n_pods} pods", "n_shards": world,
                   "value": n * steps / elapsed, "unit": "decisions/s", "ms_per_step": elapsed / steps * 1e3,
                   "decisions_per_step": n, "scaling": "strong (pod table split, batch replicated)",
                   "collective": ("inside libmmplace on its own stream: ncclAllReduce(MIN, 2 int64 per decision), then 5 x MIN + 1 x SUM over "
                                  "the undecided rest only when the (host-read) count of it is not zero (RCCL bound at run time)") if exchange == "rccl"
                   else "the library's group protocol with the exchange words moved by the host (mmp_shard_group_set_exchange): gloo, through host memory",
                   "took_the_six_phase_protocol": int(n_rest),
                   "ms_per_step_async": elapsed_async / steps * 1e3, "value_async": n * steps / elapsed_async,
                   "took_the_six_phase_protocol_async": int(n_rest_async),
                   "allreduce_bytes_per_step": 8 * s.shard_fast_slots() * n + 8 * slots * int(n_rest),
                   "sharded_commit_ms": commit_ms, "parity_vs_oracle": parity}
        s.shard_group_destroy()
        return out
    finally:
        s.close()


def churn_pod_axis_leg(workload: str, rank: int, world: int, dev, fence, slices: int = 6, events: int = 20_000):
    """Config C5 on the pod-axis layout (BASELINE.json configs[4]: streaming churn over 8 GPUs): every rank holds
    one shard; per 2 s slice every shard takes the changed InstanceRecords / ModelRecords, the shards re-commit
    together (all-reduce SUM of the rank slices) and decide the slice's load targets (speculative exchange).
    The stream is generated identically on every rank (same seed), so the shards stay in lock step.  Cache
    evictions are per pod and need no exchange; rank 0 evaluates the slice's evictions on its own context."""
    import torch

    from modelmesh_amd import dist as mdist
    from modelmesh_amd import workload as wl
    from modelmesh_amd._lib import PLACE_OUT
    from modelmesh_amd.solver import Solver

    fleet = wl.make_fleet(workload)
    cs = wl.ChurnStream(fleet, 0xC5, events_per_slice=events)
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms, device=dev.index)
    s.load_fleet(cs.fleet, commit=False)
    placer = mdist.PodShardedPlacer(mdist.SolverShardBackend(s, rank, world, dev))
    s.load_caches(cs.seg_off, cs.cache_lu, cs.cache_wt, cs.cache_cap)
    d_extra = torch.zeros(1, dtype=torch.int32, device=dev)
    busy, n_ev = 0.0, 0
    for it in range(slices + 1):
        f = cs.fleet
        ev = cs.model_events() if it else None
        fence()
        t0 = time.perf_counter()
        if it:
            s.upsert_pods(cs.changed_pods, f.pods[cs.changed_pods])
            s.upsert_models(*ev)
        placer.commit()
        sl = cs.next_slice()
        reqs = sl["place_reqs"]
        n = len(reqs)
        d_reqs = torch.from_numpy(np.ascontiguousarray(reqs).view(np.uint8).reshape(-1)).to(dev)
        d_outs = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
        placer.place(d_reqs, n, d_extra, f.now, d_outs)
        got = np.frombuffer(d_outs.cpu().numpy().tobytes(), dtype=PLACE_OUT)
        if rank == 0:
            s.evict(sl["evict_reqs"], f.now)
        fence()
        if it:  # slice 0 is the warm-up
            busy += time.perf_counter() - t0
            n_ev += events
        cs.apply(sl, got)
    s.close()
    if rank != 0:
        return None
    return {"workload": f"C5 on the pod axis: {events} events per 2 s slice over {fleet.n_models} models x {fleet.n_pods} pods, "
                        f"{world} shard(s), sharded commit per slice", "events_per_s": n_ev / busy, "slices": slices,
            "ms_per_slice": busy / slices * 1e3, "required_events_per_s": 10_000, "headroom_x": n_ev / busy / 10_000}


def full_cluster_leg(workload: str, device: int, dev):
    """The same batch on the steady state of a mesh: EVERY instance full and all caches about equally old (global
    LRU eviction) — getNext is then in its LRU-window mode (MM.java:4911-4917) and most shortlists are the whole
    table.  The library picks place_batch_long_kernel for such a snapshot."""
    import torch

    from modelmesh_amd import workload as wl
    from modelmesh_amd._lib import PLACE_OUT
    from modelmesh_amd.solver import Solver
    from oracle.bind import OracleFleet
    fleet = wl.make_fleet(workload)
    rng = np.random.default_rng(5)
    P = fleet.n_pods
    fleet.pods["used"] = fleet.pods["capacity"] - rng.integers(0, 40_000, P)
    fleet.pods["lru_time"] = fleet.now - (36_000_000 * (1 + rng.uniform(-0.04, 0.04, P))).astype(np.int64)
    reqs, extra = wl.make_requests(fleet, seed=0xBE7C0)
    n = len(reqs)
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms, device=device)
    try:
        s.load_fleet(fleet)
        d_reqs = torch.from_numpy(reqs.view(np.uint8).reshape(-1)).to(dev)
        d_extra = torch.from_numpy(np.ascontiguousarray(extra if len(extra) else np.zeros(1, np.int32))).to(dev)
        d_outs = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
        st = torch.cuda.Stream(dev)
        for _ in range(3):
            s.place_dev(d_reqs.data_ptr(), n, d_extra.data_ptr(), fleet.now, d_outs.data_ptr(), st.cuda_stream)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(20):
            s.place_dev(d_reqs.data_ptr(), n, d_extra.data_ptr(), fleet.now, d_outs.data_ptr(), st.cuda_stream)
        torch.cuda.synchronize(dev)
        dt = (time.perf_counter() - t0) / 20
        got = np.frombuffer(d_outs.cpu().numpy().tobytes(), dtype=PLACE_OUT)
        # the same launches alternating on two streams (the shape of the headline's timed region: one launch's ramp-up and tail
        # under the other's body), each stream with its own result buffer
        st2 = torch.cuda.Stream(dev)
        d_outs2 = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
        pairs = ((st, d_outs), (st2, d_outs2))
        for i in range(4):
            q, o = pairs[i & 1]
            s.place_dev(d_reqs.data_ptr(), n, d_extra.data_ptr(), fleet.now, o.data_ptr(), q.cuda_stream)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for i in range(40):
            q, o = pairs[i & 1]
            s.place_dev(d_reqs.data_ptr(), n, d_extra.data_ptr(), fleet.now, o.data_ptr(), q.cuda_stream)
        torch.cuda.synchronize(dev)
        dt2 = (time.perf_counter() - t0) / 40
        got2 = np.frombuffer(d_outs2.cpu().numpy().tobytes(), dtype=PLACE_OUT)
        # ONE decision on this fleet through the host-pointer ABI (n = 1: the call a request thread makes) — the regime in which the
        # reference's own loop walks the whole table (MM.java:4890-4938) and the GPU path wins a SINGLE request:
        # the load target alone (mmp_place_batch) and the cache-miss route (mmp_miss_batch: guards + load target)
        import ctypes as C

        from modelmesh_amd import _lib as L
        from modelmesh_amd._lib import ptr as _ptr
        orc = OracleFleet(fleet)
        k1 = 1200
        one = reqs[:1].copy()
        one_out = np.zeros(1, dtype=PLACE_OUT)
        g1 = np.zeros(1, dtype=L.GATE_REQ)
        g1["cache_capacity"], g1["loader_predicted"] = 8_388_608, 6400
        go1 = np.zeros(1, dtype=L.GATE_OUT)
        a_place = (s.h, _ptr(one), C.c_int32(1), None, C.c_int32(0), C.c_int64(fleet.now), _ptr(one_out))
        z = C.c_int32(0)
        a_miss = (s.h, _ptr(g1), _ptr(one), C.c_int32(1), None, None, z, None, z, None, z, C.c_int64(fleet.now), C.c_int64(450_000), _ptr(go1),
                  _ptr(one_out))
        lat1 = {"place": [], "miss": []}
        got1 = np.zeros(k1, dtype=PLACE_OUT)
        for name, fn, a in (("place", s.lib.mmp_place_batch, a_place), ("miss", s.lib.mmp_miss_batch, a_miss)):
            for i in range(k1 + 200):
                one[0] = reqs[(i * 37) % n]
                one["extra_off"] = 0
                one["n_extra"] = 0
                g1["model"], g1["self_pod"] = one["model"], one["self_pod"]
                t1 = time.perf_counter()
                rc = fn(*a)
                dt1 = time.perf_counter() - t1
                if rc != 0:
                    raise RuntimeError(f"full cluster, single {name}: rc {rc}")
                if i >= 200:
                    lat1[name].append(dt1)
                    if name == "place":
                        got1[i - 200] = one_out[0]
        single_reqs = reqs[[(i * 37) % n for i in range(200, k1 + 200)]].copy()
        single_reqs["extra_off"] = 0
        single_reqs["n_extra"] = 0
    finally:
        s.close()
    want1 = orc.place(single_reqs, None, fleet.now, threads=usable_cpus())
    single_parity = bool(all(np.array_equal(got1[f], want1[f]) for f in ("chosen", "best", "n_candidates", "hash")))
    # the CPU port of the reference algorithm on the SAME fleet: decisions/s on the granted cores and per-decision latency on one
    # (a bounded sample: a decision walks thousands of instances here, ~80 us each on one core)
    cores = usable_cpus()
    cpu = {}
    for label, th in (("single", 1), ("all", cores)):
        pool = orc.lean_pool(th)
        try:
            sample = reqs[: 4000 * th]
            pool(sample[:200], extra, fleet.now)
            n_done, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < 3.0:
                pool(sample, extra, fleet.now)
                n_done += len(sample)
            cpu[label] = n_done / (time.perf_counter() - t0)
            if th == 1:
                _, cl = pool(reqs[:3000], extra, fleet.now, latencies=True)
                cpu["p50_us"], cpu["p99_us"] = float(np.percentile(cl, 50) / 1e3), float(np.percentile(cl, 99) / 1e3)
        finally:
            pool.close()
    want = orc.place(reqs, extra, fleet.now, threads=usable_cpus())
    parity = bool(all(np.array_equal(g[f], want[f]) for g in (got, got2) for f in ("chosen", "best", "n_candidates", "hash")))
    # roofline of place_batch_long_kernel on this fleet.  What a decision MUST move is what it moves on any fleet (request, model
    # row, its lists, result): the shortlist's per-type prefix tables (candidate count, hash sum, rpm-rule survivors over the
    # shortlist order; built at commit) are shared by all decisions and L2-resident.  The walk they replace would have read a
    # 16 B record per shortlisted instance (MM.java:4880-4935): kept beside it as `walk_equivalent_bytes`, not as traffic.
    comp = kernel_bytes(fleet, reqs)
    traffic, prov = measured_traffic(workload, n, "place_batch_long_kernel", "_full_cluster")
    use = traffic or comp
    roof = {"bound": "hbm", "kernel": "place_batch_long_kernel", "achieved": use / dt / 1e9, "peak": 8000.0, "unit": "GB/s",
            "frac": use / dt / 8e12, "traffic": traffic, "traffic_provenance": prov, "bytes_per_launch": use,
            "compulsory_bytes_per_launch": comp, "walk_equivalent_bytes": int(got["n_candidates"].astype(np.int64).sum()) * 16,
            "note": "launch time here = wall time of 20 back-to-back launches on one stream / 20"}
    return {"workload": f"{workload} with every instance full, lruTimes within +-4 % of 10 h", "value": n / dt, "unit": "decisions/s",
            "ms_per_step": dt * 1e3, "note": "value / ms_per_step: launches back to back on ONE stream (what rounds 1-2 reported)",
            "value_two_streams": n / dt2, "ms_per_step_two_streams": dt2 * 1e3,
            "mean_shortlist": float(got["n_candidates"].mean()), "parity_vs_oracle": parity, "roofline": roof,
            # one request at a time on this fleet: the GPU path through the C ABI against the CPU port of the reference algorithm
            "single_decision": {
                "gpu_place_n1": {"p50_us": float(np.percentile(lat1["place"], 50) * 1e6), "p99_us": float(np.percentile(lat1["place"], 99) * 1e6)},
                "gpu_miss_route_n1": {"p50_us": float(np.percentile(lat1["miss"], 50) * 1e6), "p99_us": float(np.percentile(lat1["miss"], 99) * 1e6)},
                "cpu_port_one_core": {"p50_us": cpu["p50_us"], "p99_us": cpu["p99_us"]},
                "parity_vs_oracle": single_parity,
                "note": "mmp_place_batch / mmp_miss_batch with n = 1 (host pointers, launch + PCIe inclusive, ctypes) against "
                        "orc_place_lean on one core: with every instance full the reference's loop walks the table"},
            "cpu_baseline": {"value": cpu["all"], "unit": "decisions/s", "cores": cores, "kind": "port", "single_thread_value": cpu["single"],
                             "p50_us": cpu["p50_us"], "p99_us": cpu["p99_us"],
                             "sample": f"~3 s per leg of the same full-cluster batch (4000 decisions per thread per call); "
                                       "oracle/mm_oracle.c:orc_place_lean, not the JVM"}}


def single_caller_leg(fleet, solver, dev, sets: int = 8):
    """The single-caller request form (mmp_place_batch_c: the caller's side once per call, 24 bytes per decision — the shape of
    every batch the reference itself issues: rate task, janitor, reaper, preShutdown run on ONE instance): `sets` request sets
    of one caller in one launch against the same decisions as 64-byte rows; launch time on one stream between an event pair,
    4 rotating buffers; then the host-pointer call (PCIe inclusive).  Parity: both forms against the oracle."""
    import ctypes as C

    import torch

    from modelmesh_amd import _lib as L
    from modelmesh_amd import workload as wl
    from modelmesh_amd._lib import PLACE_OUT
    from modelmesh_amd._lib import ptr as _ptr
    from oracle.bind import OracleFleet
    solver.load_fleet(fleet)
    sp = 4321 % fleet.n_pods
    row = fleet.pods[sp]
    bufs, hosts = [], []
    for b in range(4):
        parts, ex_parts, off = [], [], 0
        for k in range(sets):
            rq, ex = wl.make_requests(fleet, seed=0xCA11E + b * 31 + k)
            rq = rq.copy()
            rq["extra_off"] += off
            off += len(ex)
            parts.append(rq)
            ex_parts.append(ex)
        rq = np.concatenate(parts)
        ex = np.concatenate(ex_parts)
        rq["self_pod"], rq["flags"] = sp, 0
        rq["fresh_lru"], rq["fresh_capacity"], rq["fresh_used"] = row["lru_time"], row["capacity"], row["used"] + 1000
        rq["fresh_count"], rq["fresh_rpm"] = row["count"], 0
        caller, rc = L.split_caller(rq)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
        n = len(rq)
        bufs.append((up(rq), up(rc), up(ex), len(ex), torch.zeros(n * 16, dtype=torch.uint8, device=dev),
                     torch.zeros(n * 16, dtype=torch.uint8, device=dev)))
        hosts.append((rq, rc, ex))
    st = torch.cuda.Stream(dev)
    K, ms = 200, {}
    for form in ("rows", "caller"):
        if form == "rows":
            fn = solver.lib.mmp_place_batch_dev
            args = [(solver.h, C.c_void_p(r.data_ptr()), C.c_int32(n), C.c_void_p(e.data_ptr()), C.c_int64(fleet.now), C.c_void_p(o.data_ptr()),
                     C.c_void_p(st.cuda_stream)) for r, _, e, _, o, _ in bufs]
        else:
            fn = solver.lib.mmp_place_batch_c_dev
            args = [(solver.h, _ptr(caller), C.c_void_p(r.data_ptr()), C.c_int32(n), C.c_void_p(e.data_ptr()), C.c_int32(ne), C.c_int64(fleet.now),
                     C.c_void_p(o.data_ptr()), C.c_void_p(st.cuda_stream)) for _, r, e, ne, _, o in bufs]
        for i in range(20):
            if fn(*args[i % 4]) != 0:
                raise RuntimeError(solver.lib.mmp_last_error(solver.h))
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for i in range(K):
            fn(*args[i % 4])
        e1.record(st)
        torch.cuda.synchronize(dev)
        ms[form] = e0.elapsed_time(e1) / K
    # the single-caller launches round-robin on four streams, as the timed region issues its steps: wall time per launch
    sts4 = [st] + [torch.cuda.Stream(dev) for _ in range(3)]
    args4 = [tuple(list(a[:-1]) + [C.c_void_p(sts4[i % 4].cuda_stream)]) for i, a in enumerate(args)]
    for i in range(20):
        fn(*args4[i % 4])
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(4 * K):
        fn(*args4[i % 4])
    torch.cuda.synchronize(dev)
    ms4 = (time.perf_counter() - t0) * 1e3 / (4 * K)
    rq0, rc0, ex0 = hosts[0]
    want = OracleFleet(fleet).place(rq0, ex0, fleet.now, threads=usable_cpus())
    got_r = np.frombuffer(bufs[0][4].cpu().numpy().tobytes(), dtype=PLACE_OUT)
    got_c = np.frombuffer(bufs[0][5].cpu().numpy().tobytes(), dtype=PLACE_OUT)
    parity = bool(all(np.array_equal(g[f], want[f]) for g in (got_r, got_c) for f in ("chosen", "best", "n_candidates", "hash")))
    # the host boundary: the same batch through host pointers (H2D of the requests + launch + D2H of the results)
    t_host = {}
    for form in ("rows", "caller"):
        ts = []
        for _ in range(6):
            t0 = time.perf_counter()
            if form == "rows":
                solver.place(rq0, ex0, fleet.now)
            else:
                solver.place_c(caller, rc0, ex0, fleet.now)
            ts.append(time.perf_counter() - t0)
        t_host[form] = float(np.median(ts[1:]))
    return {"decisions_per_launch": n, "request_sets": sets, "caller": int(sp),
            "kernel_ms_rows_64B": ms["rows"], "kernel_ms_single_caller_24B": ms["caller"],
            "decisions_per_s_single_caller": n / (ms["caller"] * 1e-3),
            "ms_per_launch_single_caller_4_streams": ms4, "decisions_per_s_single_caller_4_streams": n / (ms4 * 1e-3),
            "shortlists": {"kernel": "place_memo_c_kernel + place_tail_c_kernel from 524288 rows on (two launches on the call's stream: "
                                     "the type's recorded shortlist checked by a lane per request, the undecided ones in a dense "
                                     "tail; place_kernel.hpp: TypeMemo, memo_try, place_tail_body); place_batch_c_m_kernel (one "
                                     "launch, the check in front of the lane phase) from 262144 rows on; `kernel_ms_*` = the whole "
                                     "call on ONE stream",
                           "rows": [[int(v) for v in r] for r in solver.shortlists()]},
            "hbm_bytes_per_decision": {"rows": 80, "single_caller": 40},
            "hbm_only_frac": {"rows": hbm_stream_bytes(n) / (ms["rows"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                              "single_caller": hbm_stream_bytes(n, 24) / (ms["caller"] * 1e-3) / 1e9 / HBM_PEAK_GBS},
            "host_boundary_decisions_per_s": {"rows": n / t_host["rows"], "single_caller": n / t_host["caller"]},
            "parity_vs_oracle": parity,
            "note": "mmp_place_batch_c_dev / mmp_place_batch_c: self and getFreshInstanceRecord() belong to the calling instance "
                    "(MM.java:5369-5386) and travel once per call; the launch is bound by the instructions of a decision, not by "
                    "the request stream (profiles/r5/place_experiments/README.md, profiles/r5/shortlist_experiments/README.md): "
                    "halving the bytes bought 14 %, the shortlists in front of the lane phase another 10-12 %; round 6: split into "
                    "two launches, four streams with a hardware queue each 8.1-8.4 us per 800k rows (profiles/r6/README.md)"}


def multi_entry_leg(fleet, solver, dev, k: int = 8):
    """A host that holds k batches the size of ONE request set (one decision per model): k launches (mmp_place_batch_dev each)
    against one launch over the k arrays (mmp_place_multi_dev), same stream, same buffers, results compared."""
    import torch

    from modelmesh_amd import workload as wl
    from modelmesh_amd._lib import PLACE_OUT
    solver.load_fleet(fleet)  # (the churn leg left its own fleet in the context)
    sets = [wl.make_requests(fleet, seed=0x3A00 + i) for i in range(k)]
    n = len(sets[0][0])
    d_reqs = [torch.from_numpy(r.view(np.uint8).reshape(-1)).to(dev) for r, _ in sets]
    d_extra = [torch.from_numpy(np.ascontiguousarray(x if len(x) else np.zeros(1, np.int32))).to(dev) for _, x in sets]
    d_a = [torch.zeros(n * 16, dtype=torch.uint8, device=dev) for _ in range(k)]
    d_b = [torch.zeros(n * 16, dtype=torch.uint8, device=dev) for _ in range(k)]
    st = torch.cuda.Stream(dev)
    rp, xp = [t.data_ptr() for t in d_reqs], [t.data_ptr() for t in d_extra]
    ap, bp = [t.data_ptr() for t in d_a], [t.data_ptr() for t in d_b]

    def separate():
        for i in range(k):
            solver.place_dev(rp[i], n, xp[i], fleet.now, ap[i], st.cuda_stream)

    def one_launch():
        solver.place_multi_dev(rp, [n] * k, xp, fleet.now, bp, st.cuda_stream)
    out = {}
    for name, fn in (("separate_launches", separate), ("one_launch", one_launch)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(20):
            fn()
        torch.cuda.synchronize(dev)
        out[name + "_us"] = (time.perf_counter() - t0) / 20 * 1e6
    same = all(bool((a == b).all().item()) for a, b in zip(d_a, d_b))
    return {"arrays": k, "decisions_per_array": n, **out, "decisions_per_s_one_launch": k * n / (out["one_launch_us"] * 1e-6),
            "identical_results": same,
            "note": "k x mmp_place_batch_dev vs one mmp_place_multi_dev over the same k request arrays, one stream, wall time of 20 "
                    "repetitions incl. the host's issue time"}


def seam_latency_leg(fleet, solver, reps: int = 2000):
    """What invokeModel costs per request at the boundary: the cache-hit route (guards + serve target) and the cache-miss route
    (guards + load target), each as ONE call (mmp_route_batch / mmp_miss_batch, n = 1) and as the two calls it replaces.
    Arguments marshalled once; wall time per call through ctypes."""
    import ctypes as C

    from modelmesh_amd import _lib
    from modelmesh_amd._lib import ptr
    solver.load_fleet(fleet)
    now = fleet.now
    lib, h = solver.lib, solver.h
    rng = np.random.default_rng(7)
    g = np.zeros(1, dtype=_lib.GATE_REQ)
    g["model"], g["self_pod"], g["cache_capacity"], g["loader_predicted"] = 12345 % fleet.n_models, 17 % fleet.n_pods, 8_388_608, 6400
    go = np.zeros(1, dtype=_lib.GATE_OUT)
    sr = np.zeros(1, dtype=_lib.SERVE_REQ)
    sr["model"], sr["self_pod"], sr["assume_completed_ms"] = g["model"], g["self_pod"], 3000
    in_use = rng.integers(0, 3, fleet.n_pods).astype(np.int32)
    last_used = (now - rng.integers(0, 10_000, fleet.n_pods)).astype(np.int64)
    sr, cnt = solver.serve_counters(sr, in_use, last_used)
    if len(cnt) == 0:
        cnt = np.zeros(1, dtype=_lib.SERVE_COUNTER)
    so = np.zeros(1, dtype=_lib.SERVE_OUT)
    nc = C.c_int32(int(sr["n_cnt"].sum()))
    pr, _ = wl_requests(fleet, 1)
    pr["model"], pr["self_pod"] = g["model"], g["self_pod"]
    po = np.zeros(1, dtype=_lib.PLACE_OUT)
    one = C.c_int32(1)
    z = C.c_int32(0)
    calls = {
        "gates": (lib.mmp_gate_batch, (h, ptr(g), one, None, None, z, None, z, C.c_int64(now), C.c_int64(450_000), ptr(go))),
        "serve": (lib.mmp_serve_batch, (h, ptr(sr), one, ptr(cnt), nc, None, None, z, C.c_int64(now), ptr(so))),
        "place": (lib.mmp_place_batch, (h, ptr(pr), one, None, z, C.c_int64(now), ptr(po))),
        "route": (lib.mmp_route_batch, (h, ptr(g), ptr(sr), one, ptr(cnt), nc, None, None, z, None, z, C.c_int64(now), C.c_int64(450_000),
                                        ptr(go), ptr(so))),
        "miss": (lib.mmp_miss_batch, (h, ptr(g), ptr(pr), one, None, None, z, None, z, None, z, C.c_int64(now), C.c_int64(450_000), ptr(go),
                                      ptr(po))),
    }
    out = {}
    for name, (fn, a) in calls.items():
        for _ in range(200):
            fn(*a)
        t = np.zeros(reps)
        for i in range(reps):
            t0 = time.perf_counter()
            rc = fn(*a)
            t[i] = time.perf_counter() - t0
            if rc != 0:
                raise RuntimeError(f"{name}: rc {rc}")
        out[name] = {"p50_us": float(np.percentile(t, 50) * 1e6), "p99_us": float(np.percentile(t, 99) * 1e6)}
    return {"cache_hit_route_one_call": out["route"], "cache_hit_as_two_calls_p50_us": out["gates"]["p50_us"] + out["serve"]["p50_us"],
            "cache_miss_route_one_call": out["miss"], "cache_miss_as_two_calls_p50_us": out["gates"]["p50_us"] + out["place"]["p50_us"],
            "single_calls": {k: out[k] for k in ("gates", "serve", "place")},
            "note": "n = 1 through the C ABI (ctypes, arguments marshalled once): mmp_route_batch = request guards + serve target, "
                    "mmp_miss_batch = request guards + load target, one launch each"}


def seam_tail_cpp(reps: int = 8000):
    """The four n = 1 seam calls issued round-robin from a plain C++ thread (tools/micro/seam_tail.cc, built here): percentiles
    without the interpreter's noise, and WHEN the slow calls happen — by kind and in bursts (profiles/r5/seam_tail.txt: they
    fall on every kind alike; the tail is not a property of one call path)."""
    import re
    import subprocess
    import tempfile
    exe = os.path.join(tempfile.gettempdir(), f"mmp_seam_tail_{os.getpid()}")
    libdir = os.path.join(ROOT, "modelmesh_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "micro", "seam_tail.cc"),
                    "-L" + libdir, "-lmmplace", "-Wl,-rpath," + libdir, "-lpthread", "-o", exe], check=True, capture_output=True)
    def parse(stdout, what):
        out = {}
        for m in re.finditer(r"^(\w+)\s+n=1\s+p50\s+([\d.]+)\s+p90\s+([\d.]+)\s+p99\s+([\d.]+)\s+p99\.9\s+([\d.]+)\s+max\s+([\d.]+)", stdout, re.M):
            out[m.group(1)] = {"p50_us": float(m.group(2)), "p90_us": float(m.group(3)), "p99_us": float(m.group(4)), "p99_9_us": float(m.group(5)),
                               "max_us": float(m.group(6))}
        m = re.search(r"slow calls .*?: (\d+) of (\d+) = ([\d.]+) %; by kind: place (\d+) serve (\d+) gates (\d+) route (\d+)", stdout)
        if m:
            out["slow_calls"] = {"share_pct": float(m.group(3)), "by_kind": {"place": int(m.group(4)), "serve": int(m.group(5)), "gates": int(m.group(6)),
                                                                           "route": int(m.group(7))}}
        m = re.search(r"(\d+) of (\d+) directly behind another slow call", stdout)
        if m and "slow_calls" in out:
            out["slow_calls"]["directly_behind_another"] = int(m.group(1))
        m = re.search(r"calling thread: (.*?); while measuring: (\d+) voluntary and (\d+) involuntary context switches", stdout)
        if m:
            out["calling_thread"] = {"state": m.group(1), "voluntary_context_switches": int(m.group(2)), "involuntary_context_switches": int(m.group(3))}
        out["note"] = f"{reps} calls of each kind, round-robin, one C++ thread, {what}; slow = more than 1.6 x the kind's p50"
        return out

    # round 6: the same run with the calling thread left to the scheduler and PINNED to one CPU of the process's mask.
    # On the 256-thread host behind a 16-CPU quota the unpinned thread is moved around (hundreds of context switches per run) and 0.5 %
    # of its calls are slow, in bursts, on every kind alike; pinned, it is switched a handful of times and the tail goes with it
    # (profiles/r6/seam_tail_pinning.txt).  A mesh's request threads are the host's to pin; the line carries both.
    try:
        cpus = sorted(os.sched_getaffinity(0))
        pin = cpus[len(cpus) // 2]
        runs = {}
        for label, extra_args, what in (("pinned_to_one_cpu", ["pin", str(pin)], f"pinned to CPU {pin}"), ("unpinned", [], "not pinned")):
            r = subprocess.run([exe, str(reps)] + extra_args, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise RuntimeError(f"seam_tail exit {r.returncode}: {r.stderr[-300:]}")
            runs[label] = parse(r.stdout, what)
    finally:
        try:
            os.unlink(exe)
        except OSError:
            pass
    out = dict(runs["pinned_to_one_cpu"])  # (the percentiles at the top level of the object are the pinned run's)
    out["unpinned"] = runs["unpinned"]
    return out


def wl_requests(fleet, n):
    from modelmesh_amd import workload as wl
    r, x = wl.make_requests(fleet, 3, n=max(n, 1), extra_frac=0.0)
    return r[:n].copy(), x


def _single_prober():
    """tools/micro/single_prober.c built with gcc (None when no compiler is at hand: the leg then reports no latencies)"""
    import ctypes as C
    import subprocess
    import tempfile
    src = os.path.join(ROOT, "tools", "micro", "single_prober.c")
    so = os.path.join(tempfile.gettempdir(), f"mmp_single_prober_{os.getpid()}.so")
    try:
        subprocess.run(["gcc", "-O2", "-shared", "-fPIC", src, "-o", so, "-lpthread"], check=True, capture_output=True, timeout=120)
        lib = C.CDLL(so)
    except Exception:
        return None
    lib.prober_start.restype = C.c_int
    lib.prober_start.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64]
    lib.prober_stop.restype = C.c_int64
    lib.prober_stop.argtypes = [C.c_void_p, C.c_int64]
    return lib


def churn_leg(fleet, solver, slices: int = 8, events: int = 20_000):
    """Config C5 on this rank's solver: per 2 s slice of simulated time apply the changed InstanceRecords and
    the changed ModelRecords (mmp_pods_upsert / mmp_models_upsert), re-rank on the device, decide the slice's load targets and evaluate its
    cache evictions (host-pointer C ABI, PCIe inclusive).  Only the library calls are timed; the event
    generation / bookkeeping between slices (numpy) is not part of the path."""
    import ctypes as C
    from modelmesh_amd import workload as wl
    cs = wl.ChurnStream(fleet, 0xC5)
    solver.load_caches(cs.seg_off, cs.cache_lu, cs.cache_wt, cs.cache_cap)
    busy, commit_s, n_ev = 0.0, 0.0, 0
    # BASELINE.md config 5 asks for the p99 DECISION latency of the sustained stream: a second host thread (C:
    # tools/micro/single_prober.c — a Python thread's samples would include its waits for the interpreter lock) issues single
    # load-target decisions, mmp_place_batch(n = 1), back to back for the whole leg and records each call's wall time
    single, _ = wl.make_requests(fleet, seed=0xC51, n=256)
    single = np.ascontiguousarray(single)
    single["n_extra"] = 0
    single["extra_off"] = 0
    prober = _single_prober()
    for it in range(slices + 1):
        f = cs.fleet
        ev = cs.model_events() if it else None  # building the event batch is the host mesh's work, not timed
        t0 = time.perf_counter()
        if it:
            solver.upsert_pods(cs.changed_pods, f.pods[cs.changed_pods])
            solver.upsert_models(*ev)  # the ModelRecords the previous slice changed (registry listener events)
            t1 = time.perf_counter()
            solver.commit()
            commit_s += time.perf_counter() - t1
        sl = cs.next_slice()
        got = solver.place(sl["place_reqs"], sl["extra"], f.now)
        solver.evict(sl["evict_reqs"], f.now)
        if it:  # slice 0 is the warm-up
            busy += time.perf_counter() - t0
            n_ev += events
        elif prober is not None:  # (after the warm-up slice: a committed snapshot exists)
            prober.prober_start(C.cast(solver.lib.mmp_place_batch, C.c_void_p), solver.h, single.ctypes.data_as(C.c_void_p), len(single),
                                C.c_int64(int(fleet.now)), C.c_int64(4_000_000))
        cs.apply(sl, got)
    lat, why_none = np.zeros(0), "tools/micro/single_prober.c could not be built (no gcc?)"
    if prober is not None:
        buf = np.zeros(4_000_000, np.uint32)
        got_n = int(prober.prober_stop(buf.ctypes.data_as(C.c_void_p), C.c_int64(len(buf))))
        lat = buf[100:got_n].astype(np.float64) / 1e3 if got_n > 200 else np.zeros(0)
        why_none = f"the prober thread returned {got_n} (negative: calls that failed; small: too few samples)"
    return {"single_decisions_during_churn": {"error": why_none} if not len(lat) else {
                "calls": int(len(lat)), "p50_us": float(np.percentile(lat, 50)), "p99_us": float(np.percentile(lat, 99)),
                "p999_us": float(np.percentile(lat, 99.9)), "max_us": float(lat.max()),
                "note": "mmp_place_batch(n = 1) from a second host thread (C, tools/micro/single_prober.c) for the whole leg, across its "
                        "upserts, registry events and commits (a decision takes the published snapshot; a commit swaps a pointer)"},
            "workload": f"C5: {events} events per 2 s slice (45% load decisions, 45% eviction evaluations, 10% "
                        f"republishes) over {fleet.n_models} models x {fleet.n_pods} pods, commit per slice",
            "events_per_s": n_ev / busy, "slices": slices, "ms_per_slice": busy / slices * 1e3,
            "commit_ms": commit_s / slices * 1e3,
            "required_events_per_s": 10_000, "headroom_x": n_ev / busy / 10_000}


def secondary_kernels_leg(fleet, solver, device: int, workload: str = "C3", reps: int = 5):
    """Every other kernel of the path on C3-sized inputs: device
    time from the library's own HIP-event bracket around the kernels of one host-pointer call
    (mmp_profile / mmp_last_kernel_ms: events on the stream the kernels are launched on), median of
    `reps` calls, against the algorithmic bytes of SURVEY.md §8(d) / DESIGN.md §4."""
    from modelmesh_amd import _lib
    from modelmesh_amd import wire
    from modelmesh_amd import workload as wl
    from modelmesh_amd.solver import Solver
    rng = np.random.Generator(np.random.PCG64(0x5EC0))
    P, M, now = fleet.n_pods, fleet.n_models, fleet.now
    m = fleet.models
    k_of = (m["n_loaded"] + m["n_failed"]).astype(np.int64)
    out = []

    def timed(name, fn, alg_bytes, units, unit_name, note=None, s=solver):
        ms, wall = [], []
        for i in range(reps + 1):
            t0 = time.perf_counter()
            fn()
            if i:
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(s.last_kernel_ms())
        t = float(np.median(ms))
        row = {"kernel": name, "kernel_ms": t, "call_wall_ms": float(np.median(wall)), "units": int(units), "unit": unit_name,
               "units_per_s": units / (t * 1e-3) if t > 0 else None}
        if alg_bytes is not None:
            row["algorithmic_bytes"] = int(alg_bytes)
            row["achieved_GBs"] = alg_bytes / (t * 1e-3) / 1e9 if t > 0 else None
            row["frac_hbm_peak"] = row["achieved_GBs"] / HBM_PEAK_GBS if t > 0 else None
        if note:
            row["note"] = note
        out.append(row)

    solver.load_fleet(fleet)  # the churn leg left its own fleet in the context
    solver.profile(True)
    try:
        # a5 / a4: commit = rank (all pairs, literal comparator) + scatter + bitmaps + stats
        def commit_from_scratch():
            solver.load_pods(fleet.pods)  # a replaced table: the commit ranks every row
            solver.commit()
        timed("snapshot_commit (rank + scatter + build_ge + build_masks + cluster_stats)", commit_from_scratch,
              None, P, "pods ranked", "from scratch: ranks by sampling + counting with the literal PLACEMENT_ORDER comparator from 8192 pods "
              "on (rank_sample.hpp: no comparison sort; all-pairs kernel below that, or when the order is not provably total); a commit "
              "after a few changed rows re-ranks by insertion (snapshot_commit_after_16_rows)")
        # the same commit after 16 republished InstanceRecords: re-rank by insertion (delta_scatter_kernel), same tables after it
        d_rng = np.random.default_rng(16)
        d_idx = np.sort(d_rng.choice(P, size=min(16, P), replace=False)).astype(np.int32)
        flip = [0]

        def commit_after_16_rows():
            rows = fleet.pods[d_idx].copy()
            flip[0] ^= 1
            rows["count"] += flip[0]          # each of the 16 rows moves in the order, and back on the next repetition
            rows["rpm"] += 7 * flip[0]
            solver.upsert_pods(d_idx, rows)
            solver.commit()
        n0 = solver.delta_commits()
        timed("snapshot_commit after 16 changed rows (insertion re-rank + the same table builds)", commit_after_16_rows,
              None, P, "pods in the table", "the K <= 16 changed rows are placed by binary search with the literal comparator "
              "on the host's mirror of the order; one kernel re-ranks and scatters every row; bitmaps / windows / stats as above")
        out[-1]["commits_by_insertion"] = solver.delta_commits() - n0
        solver.load_pods(fleet.pods)
        solver.commit()

        # a12 stateless eviction evaluations over one clhm deque per pod
        cs = wl.ChurnStream(fleet, 0xC5)
        solver.load_caches(cs.seg_off, cs.cache_lu, cs.cache_wt, cs.cache_cap)
        # the same three kernels at two launch sizes: 100k units (391 workgroups: the launch lasts one dependent chain, like the
        # 100k place launch) and 800k (3125 workgroups: the size of a bench step, which covers the chip)
        def per_request_kernels(n, tag):
            ev = np.zeros(n, dtype=_lib.EVICT_REQ)
            ev["cache"] = rng.integers(0, P, n)
            ev["weight"] = np.minimum(cs.size_units[rng.integers(0, M, n)], 2**31 - 1)
            ev["last_used"] = np.where(rng.random(n) < 0.7, 0, now - rng.integers(1, 7_200_000, n))
            e_of = np.diff(cs.seg_off).astype(np.int64)[ev["cache"]]
            timed("evict_batch_kernel" + tag, lambda: solver.evict(ev, now), int((12 * e_of + 16).sum()), n,
                  "eviction evaluations", "SURVEY 8(d): 12*E + 16 bytes per evaluation; the deques (2.4 MB) are L2 resident")

            # a9 serve-target decisions
            sr = np.zeros(n, dtype=_lib.SERVE_REQ)
            sr["model"] = rng.integers(0, M, n)
            sr["self_pod"] = rng.integers(0, P, n)
            sr["flags"] = rng.integers(0, 4, n)
            sr["local_in_flight"] = rng.integers(0, 3, n)
            sr["last_invoke_time"] = now - rng.choice([0, 10, 1000], n)
            sr["assume_completed_ms"] = 3000
            in_use = rng.integers(0, 3, P).astype(np.int32)
            last_used = (now - rng.integers(0, 10_000, P)).astype(np.int64)
            kk = m["n_loaded"][sr["model"]].astype(np.int64)
            z32, z64 = np.zeros(0, np.int32), np.zeros(0, np.int64)
            srk, counters = solver.serve_counters(sr, in_use, last_used)  # what the host assembles: one entry per listed copy
            timed("serve_batch_kernel" + tag, lambda: solver.serve_k(srk, counters, z32, z64, now),
                  int((48 + 16 + 24 + 28 * kk).sum()), n, "serve-target decisions",
                  "request 48 B + model row 24 B + (entry 12 B + counter 16 B) per copy + result 16 B; nothing indexed by the instance table")
            # the seam the LB uses: one request per call (ForwardingLB.getNext, MM.java:4315) through a latency slot
            lat = []
            one, cnt1 = srk[:1].copy(), counters[int(srk["cnt_off"][0]): int(srk["cnt_off"][0]) + int(srk["n_cnt"][0])].copy()
            one["cnt_off"] = 0
            for _ in range(200 if not tag else 0):
                solver.serve_k(one, cnt1, z32, z64, now)
            for _ in range(3000 if not tag else 0):
                t0 = time.perf_counter_ns()
                solver.serve_k(one, cnt1, z32, z64, now)
                lat.append(time.perf_counter_ns() - t0)
            if lat:
                out.append({"kernel": "serve_single", "p50_us": float(np.percentile(lat, 50)) / 1e3, "p99_us": float(np.percentile(lat, 99)) / 1e3,
                            "bytes_in": int(48 + 16 * len(cnt1)), "unit": "serve-target decision",
                            "note": "mmp_serve_batch(n = 1) through a latency slot: 48 B + 16 B per listed copy cross the boundary (round 2: two P-sized arrays)"})

            # a10 / a11 / a14 / a20 request guards
            g = np.zeros(n, dtype=_lib.GATE_REQ)
            g["model"] = rng.integers(0, M, n)
            g["self_pod"] = rng.integers(0, P, n)
            g["flags"] = rng.integers(0, 512, n)
            g["size_hint"] = rng.choice([0, 6400], n)
            g["cache_capacity"] = 8_388_608
            g["cache_weighted_size"] = rng.integers(0, 8_388_608, n)
            g["cache_oldest_time"] = now - rng.integers(1, 5_000_000, n)
            g["loader_predicted"] = 6400
            g["loading_count"] = rng.integers(0, 20, n)
            g["weight_predict_cutoff"] = 10
            g["loaded_time"] = now - rng.integers(1, 5_000_000, n)
            g["load_timeout_ms"] = 90_000
            cur = fleet.pods[g["self_pod"]]
            for a, b in (("fresh_lru", "lru_time"), ("fresh_capacity", "capacity"), ("fresh_used", "used"),
                         ("fresh_count", "count"), ("fresh_loading_threads", "loading_threads"),
                         ("fresh_in_progress", "loading_in_progress"), ("fresh_rpm", "rpm")):
                g[a] = cur[b]
            g["last_published"] = now - rng.integers(500, 170_000, n)
            timed("gate_batch_kernel" + tag, lambda: solver.gates(g, z32, z64, z32, now),
                  int((144 + 8 + 24 + 12 * k_of[g["model"]]).sum()), n, "guarded requests",
                  "request 144 B + model row 24 B + 12 B per entry + result 8 B")
            # the cache-hit route of one request = its guards + its serve target: ONE launch (mmp_route_batch) for what the two
            # kernels above do in two (the serve half on the gate requests' models)
            sr2 = srk.copy()
            sr2["model"], sr2["self_pod"] = g["model"], g["self_pod"]
            sr2, counters2 = solver.serve_counters(sr2, in_use, last_used)
            kk2 = m["n_loaded"][sr2["model"]].astype(np.int64)
            timed("route_batch_kernel (guards + serve target, one launch)" + tag,
                  lambda: solver.route(g, sr2, counters2, z32, z64, z32, now),
                  int((144 + 48 + 24 + 8 + 16 + 12 * k_of[g["model"]] + 16 * kk2).sum()), n, "routed requests",
                  "both requests 144 + 48 B + model row 24 B + 12 B per entry + 16 B per listed copy's counter + both results 24 B")

        per_request_kernels(100_000, "")
        per_request_kernels(800_000, " (800k per launch)")

        # a17 leader proactive-load plan over the whole registry
        timed("proactive_plan (space reduction + key-range buckets + ranks by counting + distinct top-K)",
              lambda: solver.proactive_plan(6400, now, 4096), 3 * 24 * M, M, "registry rows scanned",
              "device span of eight dependent launches, no host read in the middle (round 3: 102 us with one); bytes = the three "
              "passes over the model rows (qualify, histogram, bin)")

        # a12 + a13 stateful keyed caches: one clhm put + one read per cache (10k caches)
        keys = np.concatenate([np.arange(c, dtype=np.int32) for c in np.diff(cs.seg_off)]) if len(cs.cache_lu) else z32
        e_cache = np.diff(cs.seg_off).astype(np.int64)
        ops = np.zeros(2 * P, dtype=_lib.CACHE_OP)
        ops["cache"] = np.repeat(np.arange(P, dtype=np.int32), 2)
        ops["op"] = np.tile([_lib.COP_PUT_IF_ABSENT, _lib.COP_GET], P)
        ops["key"] = np.where(ops["op"] == _lib.COP_PUT_IF_ABSENT, 1_000_000, 0)
        ops["arg"] = 6400
        ops["time"] = 0

        def replay():
            # same starting state every repetition (the replay mutates the caches)
            solver.load_caches_keyed(cs.seg_off, cs.cache_lu, cs.cache_wt, keys, cs.cache_cap)
            solver.cache_replay(ops, now)
        timed("cache_replay_kernel", replay, int((32 * e_cache + 16).sum() + 64 * len(ops)), len(ops),
              "cache operations", "16 B per deque entry read + 16 B written, 32 B per operation in + 32 B out; caches of up to 48 / 160 "
              "deque slots are replayed by 8- / 16-lane teams (8 / 4 caches per wavefront), larger ones by a wavefront each: a chain of "
              "dependent steps per cache (table row -> entries + operation -> LDS deque -> result), not a stream.  Every repetition "
              "reloads the caches first (the replay mutates them), so the kernel reads the deques COLD, from HBM: 16-17 us here against "
              "13 us for a replay of resident caches (profiles/r5/README.md) — the same kernel")

        # f-1 KV wire format: Jackson JSON of the instance table and of the registry, parsed on device
        ids = wire.make_ids(rng, P)
        wf = wl.make_fleet(workload, models=min(M, 50_000))  # registry sample: the JSON is generated in Python
        wire.adopt_ids(wf, ids)
        pv = wire.pod_values(wf, rng, np.full(P, now - 1000, np.int64))
        mv = wire.model_values(wf, ids, ["NLCLASSIFIER"] + ["type-%d" % t for t in range(1, max(wf.n_types, 1))], rng,
                               np.zeros(wf.n_models, np.int64))
        js = Solver(wf.min_space_units, wf.min_churn_age_ms, device=device)  # a context of its own: ids replace the table
        try:
            js.load_pod_ids(ids)
            js.profile(True)
            live = np.ones(P, np.uint8)
            pb = sum(len(v) for v in pv)
            timed("ingest_pods_kernel", lambda: js.ingest_pods_json(pv, np.arange(P, dtype=np.int32), live),
                  pb + 64 * P, pb, "JSON bytes", "InstanceRecord JSON read once + 64 B row written; call_wall_ms is mostly the Python "
                  "packer in front of the C call (solver.py:_pack joins the values into one blob), not the library", s=js)
            js.load_type_names(["NLCLASSIFIER"] + ["type-%d" % t for t in range(1, max(wf.n_types, 1))], 0)
            mb = sum(len(v) for v in mv)
            timed("ingest_models_kernel + rocprim scan + compact_entries_kernel", lambda: js.ingest_models_json(mv),
                  mb + 24 * wf.n_models + 36 * len(wf.ent_pod), mb, "JSON bytes",
                  "ModelRecord JSON read once + rows written + entries parked, read back and written to the CSR "
                  f"arrays (12 B x 3 per entry); {wf.n_models} of the {M} registry values; call_wall_ms is mostly the Python packer "
                  "in front of the C call (solver.py:_pack)", s=js)
        finally:
            js.close()
    finally:
        solver.profile(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--workload", default="C3", choices=["C1", "C2", "C3", "C4"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-pod-axis", action="store_true", help="skip the pod-axis sharded leg")
    ap.add_argument("--no-secondary", action="store_true", help="skip the per-kernel leg (evict / serve / gates / ...)")
    ap.add_argument("--decisions-per-step", type=int, default=800_000,
                    help="decisions of one step = one launch of place_batch_kernel, rounded to whole request sets of one "
                         "decision per model (C3: 8 sets = 800k decisions = 3125 workgroups on 256 CUs; a 100k launch is "
                         "1.5 workgroups per CU and latency-bound: DESIGN.md 11)")
    ap.add_argument("--batches", type=int, default=0,
                    help="distinct request batches the steps rotate through; 0 = as many as put requests + results above "
                         "384 MB (> the 256 MiB Infinity Cache: a timed step reads its requests from HBM), at least 3")
    ap.add_argument("--ramp", type=int, default=3000,
                    help="untimed launches in setup that bring the device out of its idle power state (not warm-up steps)")
    ap.add_argument("--issuers", type=int, default=1, help="host threads issuing the timed steps")
    ap.add_argument("--issue-threads", type=int, default=0,
                    help="submission threads inside the library (mmp_issue_threads): the timed loop then only appends "
                         "descriptors and the helpers launch in parallel, one per stream; 0 = the calling thread launches.  "
                         "Measured (round 2): the host's share of a step drops from 3.15 to 0.4 us, the step time does not move "
                         "(3.25 us: with the round-2 kernel the timed region is bound by the GPU, not by the launch path), so the "
                         "default leaves the helpers off")
    ap.add_argument("--streams", type=int, default=0,
                    help="HIP streams the timed steps are issued on round-robin; 0 = 4 (profiles/r2/place_sweep_C3.csv: a second "
                         "launch in flight covers the first one's start-up and tail — 800k decisions: 26.2 us on one stream, 17.9 us per "
                         "step on two, 17.9 on four, 20.2 on eight over long regions; round 4, the driver's 20-step region, six alternating "
                         "runs each: two streams 38.6-41.3 G decisions/s (median 40.4), four 37.6-44.0 (median 43.2); "
                         "a 100k launch is 1564 wavefronts, too few to cover its own latency chain on 256 CUs: 8.2 us on one "
                         "stream, 3.3 us per step on four; the closing synchronize costs per stream)")
    ap.add_argument("--leg-timeout", type=float, default=420.0,
                    help="watchdog for the additional legs (pod axis, latency, churn, per-kernel, cpu baseline): when "
                         "it fires rank 0 prints the line with the legs completed so far and every rank exits 0")
    ap.add_argument("--full-cluster", action="store_true",
                    help="profiling variant: every instance full and all caches equally old (the fleet of the line's `full_cluster` "
                         "object); use with --kernel-only")
    ap.add_argument("--kernel-only", action="store_true",
                    help="skip the n=1 latency / host-boundary legs (used under rocprofv3 so that every "
                         "place_batch_kernel dispatch in the trace is a full batch)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: kernel-duration passes and roofline, the parity gate against the CPU oracle and "
                         "the additional legs (the --no-* / --kernel-only options select among them)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the result rows of the last timed step as DIR/<field>.npy (float64)")
    args = ap.parse_args()

    # stdout carries ONE JSON line and nothing else: native libraries write banners to file descriptor 1 (RCCL prints
    # its version block there on communicator creation), so fd 1 is pointed at stderr for the whole run and the line
    # is written to the saved descriptor.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    # A HIP stream is served by one of GPU_MAX_HW_QUEUES hardware queues (4 unless the host says otherwise), handed out round-robin
    # over ALL streams of the process — the library's own included — and two streams that share a queue run strictly one after the
    # other.  A split batch (first launch + tail) hides its tail only behind launches of OTHER queues: with the
    # default 4 queues two of the four bench streams shared one (profiles/r6/streams.txt: 17.5 us per step; 12.9 with a queue per
    # stream).  A host's choice, like the stream count; set before the runtime initialises, reported in config.hw_queues.
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

    import torch
    import torch.distributed as dist

    from modelmesh_amd import workload as wl
    from modelmesh_amd.solver import Solver

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: libmmplace has no CPU path")
    # MMP_BENCH_ONE_DEVICE=1 (with MMP_BENCH_BACKEND=gloo) lets several ranks share cuda:0 — only for
    # exercising the N>1 code path on a 1-GPU box; the driver's runs use one GPU per rank over RCCL.
    if os.environ.get("MMP_BENCH_ONE_DEVICE") == "1":
        local_rank = 0
    backend = os.environ.get("MMP_BENCH_BACKEND", "nccl")
    torch.cuda.set_device(local_rank)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)

    # the barrier of the timed region's brackets: shared memory on one node, dist.barrier() otherwise (MMP_BENCH_DIST_BARRIER=1 forces it)
    node_barrier = None
    if world > 1 and os.environ.get("MMP_BENCH_DIST_BARRIER") != "1":
        node_barrier = NodeBarrier.create(rank, world, dist)

    fleet = wl.make_fleet(args.workload)
    if args.full_cluster:  # profiling variant (tools/gpu_profile.sh): the fleet of full_cluster_leg — every instance full, equally old
        frng = np.random.default_rng(5)
        fleet.pods["used"] = fleet.pods["capacity"] - frng.integers(0, 40_000, fleet.n_pods)
        fleet.pods["lru_time"] = fleet.now - (36_000_000 * (1 + frng.uniform(-0.04, 0.04, fleet.n_pods))).astype(np.int64)
    solver = Solver(fleet.min_space_units, fleet.min_churn_age_ms, device=local_rank)
    solver.load_fleet(fleet)
    dev = torch.device("cuda", local_rank)

    # model-axis shard: every rank owns its own batches of one-decision-per-model requests.  R distinct batches
    # (their requests + results exceed the 256 MiB Infinity Cache) so that a timed step reads its requests from HBM.
    sets_per_step = max(1, round(args.decisions_per_step / fleet.n_models))  # request sets (one decision per model) per step
    n_batches = args.batches if args.batches > 0 else max(3, -(-384_000_000 // (sets_per_step * fleet.n_models * 80)))
    n_streams = args.streams if args.streams > 0 else 4
    import ctypes as C
    batches = []  # (reqs, extra) on the host, for the parity gate
    d_bufs = []   # device tensors, kept alive
    for b in range(n_batches):
        rq, ex, pool0 = make_step_batch(fleet, [0xBE7C0 + 100_000 * rank + b * sets_per_step + j for j in range(sets_per_step)])
        if b == 0:
            first_set_pool = pool0
        batches.append((rq, ex))
        d_bufs.append((torch.from_numpy(rq.view(np.uint8).reshape(-1)).to(dev),
                       torch.from_numpy(np.ascontiguousarray(ex if len(ex) else np.zeros(1, np.int32))).to(dev),
                       torch.zeros(len(rq) * 16, dtype=torch.uint8, device=dev)))
    reqs, extra = batches[0]
    n = len(reqs)

    # bind the C calls once: at a few us of GPU work per step the ctypes argument marshalling would otherwise be
    # what is measured.  The timed steps go to streams of their own; torch's current stream is the legacy null
    # stream, whose launches order against every blocking stream of the process.
    _fn = solver.lib.mmp_place_batch_dev
    _prio = os.environ.get("MMP_BENCH_STREAM_PRIO")  # (experiments: "alt" = every second stream at high priority)
    streams = [torch.cuda.Stream(dev, priority=(-1 if _prio == "alt" and i % 2 == 0 else 0)) for i in range(n_streams)]

    def call_args(b, st):
        r_, e_, o_ = d_bufs[b]
        return (solver.h, C.c_void_p(r_.data_ptr()), C.c_int32(n), C.c_void_p(e_.data_ptr()), C.c_int64(fleet.now),
                C.c_void_p(o_.data_ptr()), C.c_void_p(st.cuda_stream))

    # step i decides batch i mod R on stream i mod S (lcm(R, S) distinct pairings)
    import math
    period = n_batches * n_streams // math.gcd(n_batches, n_streams)
    _args = [call_args(i % n_batches, streams[i % n_streams]) for i in range(period)]

    _done = [torch.cuda.Event() for _ in streams]
    _last_stream = [n_streams - 1]  # index of the stream that got the most recent launch
    _fence_t = [0.0]  # when the last fence knew the device was done (before its closing synchronize)
    _fence_default = ["last"]

    def fence():
        # Closing a region (tools/region_anatomy.py, 20 steps on 4 streams, device-side span 73 us): torch.cuda.synchronize()
        # alone parks the host on one marker round trip per stream that had launches (+45 us); polling one event per stream in
        # ISSUE order costs more (+83 us: every query of an unfinished event makes the runtime do work on that queue);
        # polling them in REVERSE order — the stream that got the last launch first, by then the others are done — gets the
        # host there in +26 us, and the synchronize that closes the region finds nothing left to wait for (+7 us).
        # (round 6) "streams": every stream synchronised in turn, then the device — each call retires its stream's finished commands
        # while the other streams still run; with two launches per step (a split batch) the synchronize that closes a region of 40
        # kernels otherwise spends 60 us retiring them (tools/r6/host_issue.py: 20 kernels 6 us, 40 kernels 45-60 us, whatever the kernels)
        _mode = os.environ.get("MMP_BENCH_FENCE", _fence_default[0])  # (experiments: "sync" = synchronize only, "spin" = issue order)
        if _mode == "streams":
            for st_ in streams:
                st_.synchronize()
        elif _mode != "sync":
            for e_, st_ in zip(_done, streams):
                e_.record(st_)
            for k_ in range(len(_done)):
                e_ = _done[k_] if _mode == "spin" else _done[(_last_stream[0] - k_) % len(_done)]
                while not e_.query():
                    # (round 6) hipStreamQuery on the other streams while waiting: the runtime retires their finished commands NOW,
                    # beside the device's work, instead of all of them inside the closing synchronize (a split batch is two launches
                    # per step: 40 commands + 4 markers to retire cost that synchronize 50-60 us of a 350 us region)
                    if _mode == "last":
                        for st_ in streams:
                            st_.query()
        _fence_t[0] = time.perf_counter()
        torch.cuda.synchronize(dev)
        if world > 1:
            if node_barrier is not None:
                node_barrier.wait()
            else:
                dist.barrier()
            torch.cuda.synchronize(dev)

    def check(rc):
        if rc != 0:
            raise RuntimeError(solver.lib.mmp_last_error(solver.h))

    # setup (untimed, not a warm-up step): every batch decided once and every stream used once, so that neither the
    # first use of a stream nor a never-touched buffer falls into the timed region whatever --warmup says
    for i in range(max(n_batches, n_streams)):
        check(_fn(*_args[i % period]))
    fence()
    if solver.split_batches()[0] > 0:
        _fence_default[0] = "streams"
    # ... and the device brought out of its idle power state: the host spent seconds generating the batches above, and
    # a 20-step region (~90 us) right after that was measured anywhere between 89 and 184 us.  ~10 ms of the same
    # launches first; none of it is timed and none of it replaces a warm-up step.
    import gc
    gc.collect()
    gc.disable()  # a collection inside a ~90 us region would be most of it (enabled again behind the region)
    for i in range(args.ramp):
        _fn(*_args[i % period])
    fence()
    # ... and the host: the first region of this shape a process runs was measured at 200 us against 86-93 us for the next
    # ones (its 20 launches take the host 112 us instead of 56, the closing synchronize 43 us instead of 7) — code and
    # data of the launch path are not in the host's caches yet.  Two untimed rehearsals of the region's shape (at most 1000
    # steps each: a longer region no longer feels that first-region cost, and the rehearsals would double the run's length).
    rehearsal = min(args.steps, 1000)
    for rep_ in range(2 if args.ramp else 0):
        for i in range(rehearsal):
            _fn(*_args[i % period])
        _last_stream[0] = (rehearsal - 1) % n_streams
        fence()
    n_helpers = max(0, min(args.issue_threads, n_streams))
    _flush = solver.lib.mmp_issue_flush
    if n_helpers:
        check(solver.lib.mmp_issue_threads(solver.h, n_helpers))
    pos = 0
    # (the timed steps' argument tuples are picked before the warm-up so that nothing but the fence lies between the
    # last warm-up step and the region)
    sched = [_args[(args.warmup + i) % period] for i in range(args.steps)]
    for i in range(args.warmup):
        check(_fn(*_args[pos % period]))
        pos += 1
    check(_flush(solver.h))
    _last_stream[0] = (pos - 1) % n_streams
    fence()
    # timed region: exactly K steps (the loop body is the bare C call: at ~4 us of launch work per step a Python
    # function frame is measurable); --issuers > 1 splits the schedule over host threads (ctypes drops the GIL)
    pos += args.steps
    _last_stream[0] = (pos - 1) % n_streams
    n_issuers = max(1, min(args.issuers, args.steps))
    issue_s = None
    if n_issuers == 1:
        rcs = 0
        t0 = time.perf_counter()
        for a in sched:
            rcs |= _fn(*a)
        t_issued = time.perf_counter()
        rcs |= _flush(solver.h)  # (submission threads) everything appended has been handed to the streams
        fence()
        elapsed = time.perf_counter() - t0
        issue_s = t_issued - t0
        if os.environ.get("MMP_BENCH_REPEAT"):  # experiments: the anatomy of this region and of further ones (stderr only)
            print(f"region 0: issue {issue_s * 1e6:.1f} us, known done {(_fence_t[0] - t0) * 1e6:.1f} us, total {elapsed * 1e6:.1f} us",
                  file=sys.stderr)
            for rep_ in range(int(os.environ["MMP_BENCH_REPEAT"])):
                sched_ = [_args[(pos + i) % period] for i in range(args.steps)]
                pos += args.steps
                _last_stream[0] = (pos - 1) % n_streams
                t0_ = time.perf_counter()
                for a in sched_:
                    _fn(*a)
                t1_ = time.perf_counter()
                _flush(solver.h)
                fence()
                t2_ = time.perf_counter()
                print(f"region {rep_ + 1}: issue {(t1_ - t0_) * 1e6:.1f} us, known done {(_fence_t[0] - t0_) * 1e6:.1f} us, "
                      f"total {(t2_ - t0_) * 1e6:.1f} us", file=sys.stderr)
    else:
        import threading as _th
        parts = [sched[j::n_issuers] for j in range(n_issuers)]
        rc_box = [0] * n_issuers
        gate = _th.Barrier(n_issuers + 1)

        def issue(j):
            gate.wait()
            rc = 0
            for a in parts[j]:
                rc |= _fn(*a)
            rc_box[j] = rc
        ths = [_th.Thread(target=issue, args=(j,)) for j in range(n_issuers)]
        for t_ in ths:
            t_.start()
        t0 = time.perf_counter()
        gate.wait()
        for t_ in ths:
            t_.join()
        rc_box.append(_flush(solver.h))
        fence()
        elapsed = time.perf_counter() - t0
        rcs = 0
        for v in rc_box:
            rcs |= v
    gc.enable()
    check(rcs)
    if n_helpers:
        check(solver.lib.mmp_issue_threads(solver.h, 0))  # the passes below bracket launches with events: issued in line
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    from modelmesh_amd._lib import PLACE_OUT
    if args.dump_outputs and rank == 0:
        # the last timed step decided batch (warmup + steps - 1) mod R; every step on that batch writes the same rows
        last_b = (args.warmup + args.steps - 1) % n_batches
        dump_outputs(args.dump_outputs, np.frombuffer(d_bufs[last_b][2].cpu().numpy().tobytes(), dtype=PLACE_OUT))

    line = None
    if rank == 0:
        line = {
            "metric": "placement decisions/sec at 100k models x 10k pods; p99 decision latency",
            "value": n * args.steps * world / elapsed, "unit": "decisions/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "i64", "data": "synthetic",
            "config": {"workload": f"{args.workload}: {fleet.n_models} models x {fleet.n_pods} pods, {sets_per_step} load-target "
                                   f"decision(s) per model per step = {n} decisions per launch (SURVEY.md §8d synthetic fleet)",
                       "decisions_per_step_per_gpu": n, "request_sets_per_step": sets_per_step,
                       "sharding": "model axis, no collective",
                       "region_barrier": None if world == 1 else ("shared memory, one node (NodeBarrier)" if node_barrier is not None
                                                                  else "dist.barrier()"),
                       "streams": n_streams, "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "distinct_batches": n_batches, "issuers": n_issuers,
                       "library_submission_threads": n_helpers,
                       "resident_input_bytes": int(n_batches * n * (64 + 16)),
                       "host_issue_us_per_step": None if issue_s is None else issue_s / args.steps * 1e6},
        }

    def close():
        solver.close()
        if world > 1:
            if node_barrier is not None:
                dist.barrier()  # nobody is still inside a wait() when rank 0 removes the page
                node_barrier.close()
            dist.destroy_process_group()

    if not args.full:
        if rank == 0:
            os.write(real_stdout, (json.dumps(line) + "\n").encode())
        close()
        return

    # the kernel's own launch duration: K back-to-back launches on ONE stream (rotating through the batches like the
    # timed region) between a HIP event pair recorded on that stream — region time / K is what
    # rocprofv3 --kernel-trace reports as the kernel's average duration for the same single-stream command ...
    stream = streams[0]  # events must be recorded on the stream the kernel is launched on
    one_stream = [call_args(i % n_batches, stream) for i in range(n_batches)]
    k_steps = max(args.steps, 200)
    for i in range(min(20, n_batches)):
        check(_fn(*one_stream[i % n_batches]))
    fence()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record(stream)
    for i in range(k_steps):
        _fn(*one_stream[i % n_batches])
    ev1.record(stream)
    fence()
    gpu_ms_per_step = ev0.elapsed_time(ev1) / k_steps
    # A split batch is two kernels per call: the figure above is the PAIR's.  The dominant kernel's own duration — what rocprofv3
    # reports as place_memo_kernel's average for this single-stream command — comes from a second context with the tail launch
    # switched off (MMP_SPLIT_NOTAIL=1, a diagnostic: such a context leaves the undecided requests undecided), the same K launches back
    # to back on the same stream between one event pair.  The rows it leaves untouched are the tail's share of the batch.
    first_ms, tail_share = None, None
    if solver.split_batches()[0] > 0:
        os.environ["MMP_SPLIT_NOTAIL"] = "1"
        try:
            s2 = Solver(fleet.min_space_units, fleet.min_churn_age_ms, device=local_rank)
            s2.load_fleet(fleet)
        finally:
            del os.environ["MMP_SPLIT_NOTAIL"]
        scratch_out = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
        s2_args = [(s2.h,) + a[1:5] + (C.c_void_p(scratch_out.data_ptr()), a[6]) for a in one_stream]
        for i in range(min(20, n_batches)):
            check(_fn(*s2_args[i % n_batches]))
        fence()
        ev0.record(stream)
        for i in range(k_steps):
            _fn(*s2_args[i % n_batches])
        ev1.record(stream)
        fence()
        first_ms = ev0.elapsed_time(ev1) / k_steps
        scratch_out.zero_()
        check(_fn(*s2_args[0]))
        fence()
        tail_share = float((scratch_out.view(-1, 16) == 0).all(dim=1).sum().item()) / n  # (a decided row is never all zero)
        s2.close()
        del scratch_out
    # ... and an event pair around every single launch (adds ~2 us of event granularity)
    n_pairs = min(k_steps, 200)
    starts = [torch.cuda.Event(enable_timing=True) for _ in range(n_pairs)]
    ends = [torch.cuda.Event(enable_timing=True) for _ in range(n_pairs)]
    for i in range(n_pairs):
        starts[i].record(stream)
        _fn(*one_stream[i % n_batches])
        ends[i].record(stream)
    fence()
    kern_ms = float(np.mean([s_.elapsed_time(e_) for s_, e_ in zip(starts, ends)]))

    # the same kernel on ONE request set per launch (one decision per model: the launch size rounds 1 and 2 quoted),
    # rotating through every set of every batch (the same 384 MB, so still from HBM), one stream, one event pair
    set_ms = None
    if sets_per_step > 1 and not args.kernel_only:  # (--kernel-only is the command the rocprofv3 summaries are taken from: one launch size)
        M_, rsz = fleet.n_models, batches[0][0].dtype.itemsize
        set_args = []
        for b in range(n_batches):
            r_, e_, o_ = d_bufs[b]
            for j in range(sets_per_step):
                set_args.append((solver.h, C.c_void_p(r_.data_ptr() + j * M_ * rsz), C.c_int32(M_), C.c_void_p(e_.data_ptr()),
                                 C.c_int64(fleet.now), C.c_void_p(o_.data_ptr() + j * M_ * 16), C.c_void_p(stream.cuda_stream)))
        for i in range(20):
            check(_fn(*set_args[i % len(set_args)]))
        fence()
        ev0.record(stream)
        for i in range(400):
            _fn(*set_args[i % len(set_args)])
        ev1.record(stream)
        fence()
        set_ms = ev0.elapsed_time(ev1) / 400

    # every batch the GPU decided must equal the oracle's answer (parity gate before any number)
    parity, want = None, None
    if rank == 0:
        from oracle.bind import OracleFleet
        orc0 = OracleFleet(fleet)
        cores = usable_cpus()
        n_check = n_batches if cores >= 16 else min(n_batches, 4)  # the checker makes ~20k decisions/s per core
        parity = True
        for b in range(n_check):
            got_b = np.frombuffer(d_bufs[b][2].cpu().numpy().tobytes(), dtype=PLACE_OUT)
            want_b = orc0.place(batches[b][0], batches[b][1], fleet.now, threads=cores)
            if b == 0:
                want = want_b
            parity = parity and bool(all(np.array_equal(got_b[f], want_b[f]) for f in ("chosen", "best", "n_candidates", "hash")))
        del orc0

    # The headline is complete here.  Everything below is an additional leg; a watchdog makes sure the
    # ONE JSON line is still printed (with the legs finished so far) if a leg hangs — e.g. a collective
    # of the pod-axis leg on a node whose RCCL setup misbehaves — instead of losing the measurement.
    if rank == 0:
        alg = int(np.mean([algorithmic_bytes(fleet, bq[0]) for bq in batches[:4]]))
        kb = int(np.mean([kernel_bytes(fleet, bq[0]) for bq in batches[:4]]))
        # launches from 393 216 decisions on are SPLIT: the per-type shortlists checked in a launch of its own (place_memo_kernel, the
        # dominant kernel: every request and result row passes through it), the rest decided by a tail launch (place_kernel.hpp:
        # kSplitFrom); MMP_NO_SPLIT=1: one launch with the check in front (place_batch_m_kernel); MMP_NO_MEMO=1: place_batch_kernel
        n_split, split_off = solver.split_batches()
        split_on = n_split > 0
        kname = ("place_memo_kernel" if split_on else
                 "place_batch_m_kernel" if n >= 262_144 and os.environ.get("MMP_NO_MEMO") != "1" else "place_batch_kernel")  # (kMemoFrom)
        traffic, traffic_prov = measured_traffic(args.workload, n, kernel=kname)
        # roofline of the dominant kernel: bytes it has to move per launch (measured by the PMC passes when a
        # summary is committed, else the compulsory streams) / its average launch duration / the HBM peak
        if split_on:
            # what place_memo_kernel asks the memory system for: the request and result streams, the model's word (4 B of an array of its
            # own, not the 32-byte registry row), the caller's position (4 B), the request's own exclusions and their positions
            kb = int(np.mean([80 * len(bq[0]) + 8 * len(bq[0]) + 8 * int(bq[0]["n_extra"].sum()) for bq in batches[:4]]))
        moved = traffic if traffic else kb
        pair_ms = gpu_ms_per_step  # one call on one stream: the kernel alone, or first launch + tail of a split batch
        if first_ms is not None:
            gpu_ms_per_step = first_ms  # the dominant kernel's own duration
        achieved = moved / (gpu_ms_per_step * 1e-3) / 1e9
        line.update({
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_provenance": traffic_prov,
                         "kernel": kname, "kernel_ms": gpu_ms_per_step,
                         "kernel_ms_per_launch_event_pairs": kern_ms,
                         "split": None if first_ms is None else {
                             "first_launch": "place_memo_kernel", "first_launch_ms": first_ms,
                             "tail_launch": "place_tail_kernel", "tail_share_of_the_batch": tail_share,
                             "call_ms_one_stream": pair_ms, "tail_ms_one_stream": pair_ms - first_ms,
                             "batches_split": n_split, "switched_off": split_off,
                             "note": "one mmp_place_batch_dev call = two launches on the caller's stream; `kernel_ms` / `frac` / `hbm_only` "
                                     "are the first launch's (every request and result row passes through it: the dominant kernel), "
                                     "`call_ms_one_stream` is both back to back on ONE stream; in the timed region the tail runs beside "
                                     "the first launches of the other streams (`ms_per_step`)"},
                         "bytes_per_launch": moved,
                         "bytes_per_launch_source": "rocprofv3 FETCH_SIZE x 2 + WRITE_SIZE (profiles/)" if traffic else
                                                    ("compulsory streams (request 64 B + the model's word 4 B + the caller's position 4 B + own exclusions + result 16 B)" if split_on else
                                                     "compulsory streams (request 64 B + resolved model row + exclusions + result 16 B)"),
                         "kernel_bytes_per_launch": kb,
                         # HBM ONLY: request stream + result rows over the kernel's own duration.  `frac` above is the counter
                         # figure, which counts the launch's L2 misses on the 3.2 MB registry view — Infinity Cache hits — as
                         # fetched bytes (profiles/r5/place_experiments/README.md: with every row fetched by ONE XCD the counter
                         # drops to 56.9 MB per launch and the launch is no faster).
                         "hbm_only": {"bytes_per_launch": hbm_stream_bytes(n), "bytes_per_decision": 80,
                                      "achieved": hbm_stream_bytes(n) / (gpu_ms_per_step * 1e-3) / 1e9,
                                      "frac": hbm_stream_bytes(n) / (gpu_ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                      "frac_timed_region": hbm_stream_bytes(n) * args.steps / elapsed / 1e9 / HBM_PEAK_GBS},
                         "frac_timed_region": moved * args.steps / elapsed / 1e9 / HBM_PEAK_GBS,
                         "launch_of_one_request_set": None if set_ms is None else (lambda tb: {
                             "decisions": fleet.n_models, "kernel_ms": set_ms, "bytes_per_launch": tb,
                             "frac": tb / (set_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                             "note": "one decision per model per launch (the launch size of rounds 1-2): 1564 wavefronts on "
                                     "256 CUs, bound by its own latency chain, not by bandwidth — DESIGN.md 4.1 / 11"})(
                             measured_traffic(args.workload, fleet.n_models)[0] or kb // sets_per_step),
                         "scan_equivalent": {
                             "note": "SURVEY.md §8(d) algorithmic bytes (32 B x P per decision: the scan the reference "
                                     "logically performs over every pod); this kernel does not perform that scan, so the "
                                     "figure is not traffic and is kept out of `frac`",
                             "algorithmic_bytes_per_launch": alg,
                             "rate_GBs": alg / (gpu_ms_per_step * 1e-3) / 1e9}},
            "parity_vs_oracle": parity,
        })
        if parity is False:
            line["invalid"] = "parity_vs_oracle is false: the numbers of this line describe a wrong kernel"

    # the additional legs below work on the first request set of batch 0 (one decision per model; its exclusion-pool
    # offsets start at 0, so the batch's pool serves it unchanged)
    reqs = reqs[:fleet.n_models]
    extra = extra[:first_set_pool]
    n = len(reqs)
    if rank == 0:
        want = want[:n]

    import threading
    emit_lock = threading.Lock()
    emitted = [False]

    def emit(note=None):
        with emit_lock:
            if emitted[0]:
                return
            emitted[0] = True
            if rank == 0:
                if note:
                    line["watchdog"] = note
                os.write(real_stdout, (json.dumps(line) + "\n").encode())

    def on_timeout():
        emit(f"an additional leg did not finish within {args.leg_timeout:.0f} s; the line carries the legs completed so far")
        os._exit(0)

    # several ranks: a collective that hangs on one rank hangs all of them; keep the wait short so that the line (with the
    # headline and the legs finished so far) still appears well inside any driver-side limit
    if world > 1:
        args.leg_timeout = min(args.leg_timeout, 240.0)
    dog = threading.Timer(args.leg_timeout, on_timeout)
    dog.daemon = True
    dog.start()

    # pod-axis sharded leg (all ranks take part; reported next to the model-axis headline)
    pod_axis = []
    if not args.no_pod_axis and not args.kernel_only:
        legs = [args.workload] + (["C4"] if world >= 8 and args.workload != "C4" else [])
        for wname in legs:
            try:
                pod_axis.append(pod_axis_leg(wname, rank, world, dev, min(max(args.steps, 20), 200), min(max(args.warmup // 10, 2), 5), fence))
            except Exception as e:  # the headline line must still be printed
                pod_axis.append({"workload": wname, "error": f"{type(e).__name__}: {e}"})
            if rank == 0:
                line["pod_axis"] = list(pod_axis)
        pod_axis_lib = []
        one_device = os.environ.get("MMP_BENCH_ONE_DEVICE") == "1" and world > 1
        for wname in legs:
            try:  # (RCCL refuses two ranks on one device: there the group's exchange goes through the host's gloo group)
                pod_axis_lib.append(pod_axis_lib_leg(wname, rank, world, dev, min(max(args.steps, 20), 200),
                                                     min(max(args.warmup // 10, 2), 5), fence, exchange="gloo" if one_device else "rccl"))
            except Exception as e:  # the headline line must still be printed
                pod_axis_lib.append({"workload": wname, "error": f"{type(e).__name__}: {e}"})
            if rank == 0:
                line["pod_axis_in_library_rccl"] = list(pod_axis_lib)
        try:
            cpa = churn_pod_axis_leg(args.workload, rank, world, dev, fence)
        except Exception as e:
            cpa = {"error": f"{type(e).__name__}: {e}"}
        if rank == 0:
            line["churn_pod_axis"] = cpa

    if rank == 0:
        line["pod_axis"] = pod_axis
        # single-decision latency through the host-pointer C ABI (n=1, PCIe + launch inclusive)
        # (the C ABI call with its arguments marshalled once, as a JNI caller holding direct ByteBuffers would;
        # `..._via_python_wrapper` adds what modelmesh_amd.solver.Solver.place spends on numpy / ctypes per call)
        lat, lat_py = [], []
        one = reqs[:1].copy()
        one_out = np.zeros(1, dtype=PLACE_OUT)
        from modelmesh_amd._lib import ptr as _ptr
        _one_args = (solver.h, _ptr(one), C.c_int32(1), None, C.c_int32(0), C.c_int64(fleet.now), _ptr(one_out))
        _place = solver.lib.mmp_place_batch
        # (round 6) the calling thread pinned to one CPU for the single-request loops, as a mesh's request threads can be: on this host
        # (256 hardware threads behind a 16-CPU quota) an unpinned thread is migrated a few hundred times per 80 000 calls and 0.5 % of
        # its calls are slow — the whole of the p99 (profiles/r6/seam_tail_pinning.txt)
        _aff = None
        try:
            _aff = os.sched_getaffinity(0)
            _pin = sorted(_aff)[len(_aff) // 2]
            os.sched_setaffinity(0, {_pin})
            line["single_decision_thread"] = f"pinned to CPU {_pin} (sched_setaffinity) for the n = 1 latency loops"
        except (AttributeError, OSError):
            _aff = None
        for i in range(0 if args.kernel_only else 2000):
            one[0] = reqs[i % n]
            one["extra_off"] = 0
            one["n_extra"] = 0
            t1 = time.perf_counter()
            rc = _place(*_one_args)
            lat.append(time.perf_counter() - t1)
            if rc != 0 or (reqs[i % n]["n_extra"] == 0 and (one_out[0]["chosen"] != want[i % n]["chosen"] or
                                                          one_out[0]["hash"] != want[i % n]["hash"])):
                raise RuntimeError(f"latency path: decision {i % n} differs from the oracle (rc {rc})")
        for i in range(0 if args.kernel_only else 300):
            one[0] = reqs[i % n]
            one["extra_off"] = 0
            one["n_extra"] = 0
            t1 = time.perf_counter()
            solver.place(one, None, fleet.now)
            lat_py.append(time.perf_counter() - t1)
        if _aff is not None:
            try:
                os.sched_setaffinity(0, _aff)
            except OSError:
                pass
        if lat:
            lat = np.array(lat[200:]) * 1e6
            line["p50_decision_latency_us"] = float(np.percentile(lat, 50))
            line["p99_decision_latency_us"] = float(np.percentile(lat, 99))
            line["p50_decision_latency_us_via_python_wrapper"] = float(np.percentile(np.array(lat_py[50:]) * 1e6, 50))
            t1 = time.perf_counter()
            for _ in range(5):
                solver.place(reqs, extra, fleet.now)
            line["host_boundary_decisions_per_s"] = 5 * n / (time.perf_counter() - t1)
            # SURVEY.md §8(d) latency metric: per-batch wall time through the host-pointer ABI for B in {1k, 64k}
            batches = {}
            for B in (1_000, 64_000):
                sub = reqs[: min(B, n)]
                ts = []
                for _ in range(60):
                    t1 = time.perf_counter()
                    solver.place(sub, extra, fleet.now)
                    ts.append(time.perf_counter() - t1)
                ts = np.array(ts[10:]) * 1e6
                batches[str(len(sub))] = {"p50_us": float(np.percentile(ts, 50)), "p99_us": float(np.percentile(ts, 99)),
                                          "p99_us_per_decision": float(np.percentile(ts, 99)) / len(sub)}
            line["host_boundary_batch_latency"] = batches
        if not args.kernel_only:
            try:
                line["churn"] = churn_leg(fleet, solver)
                sd = line["churn"].get("single_decisions_during_churn", {})
                if "p99_us" in sd:  # BASELINE.md's second criterion: decision latency while the mesh churns
                    line["p50_decision_latency_us_under_churn"], line["p99_decision_latency_us_under_churn"] = sd["p50_us"], sd["p99_us"]
            except Exception as e:
                line["churn"] = {"error": f"{type(e).__name__}: {e}"}
        if not args.kernel_only:
            try:
                line["full_cluster"] = full_cluster_leg(args.workload, local_rank, dev)
            except Exception as e:
                line["full_cluster"] = {"error": f"{type(e).__name__}: {e}"}
        if not args.kernel_only:
            try:
                line["multi_batch_entry"] = multi_entry_leg(fleet, solver, dev)
            except Exception as e:
                line["multi_batch_entry"] = {"error": f"{type(e).__name__}: {e}"}
        if not args.kernel_only:
            try:
                line["single_caller"] = single_caller_leg(fleet, solver, dev, sets_per_step)
                solver.load_fleet(fleet)
            except Exception as e:
                line["single_caller"] = {"error": f"{type(e).__name__}: {e}"}
        if not args.kernel_only:
            try:
                line["per_request_seams"] = seam_latency_leg(fleet, solver)
                line["per_request_seams"]["from_a_cpp_host"] = seam_tail_cpp()
            except Exception as e:
                line["per_request_seams"] = {"error": f"{type(e).__name__}: {e}"}
        if not args.kernel_only and not args.no_secondary:
            try:
                line["kernels"] = secondary_kernels_leg(fleet, solver, local_rank, args.workload)
            except Exception as e:
                line["kernels"] = {"error": f"{type(e).__name__}: {e}"}
        if world == 1 and not args.no_cpu_baseline and not args.kernel_only:
            line["cpu_baseline"] = cpu_baseline(fleet, reqs, extra)
        # the three regimes of the load-target kernel, read together: 8 request sets per launch (`value`),
        # one request set per launch, and the full cluster (getNext's LRU-window mode, whole-table shortlists)
        one_set = (line.get("roofline") or {}).get("launch_of_one_request_set") or {}
        fc = line.get("full_cluster") if isinstance(line.get("full_cluster"), dict) else {}
        line["roofline_frac_by_regime"] = {
            "value_launch": (line.get("roofline") or {}).get("frac"),
            "value_launch_hbm_only": ((line.get("roofline") or {}).get("hbm_only") or {}).get("frac"),
            "launch_of_one_request_set": one_set.get("frac"),
            "full_cluster": (fc.get("roofline") or {}).get("frac")}
        # the regime in which one request at a time is FASTER on the GPU path than the reference algorithm on a core
        sdl = fc.get("single_decision") or {}
        if sdl:
            line["full_cluster_single_decision_us"] = {"gpu_p50": (sdl.get("gpu_place_n1") or {}).get("p50_us"),
                                                       "gpu_p99": (sdl.get("gpu_place_n1") or {}).get("p99_us"),
                                                       "cpu_port_p50": (sdl.get("cpu_port_one_core") or {}).get("p50_us"),
                                                       "cpu_port_p99": (sdl.get("cpu_port_one_core") or {}).get("p99_us")}
    if rank == 0:
        # the scalars a reader of the driver's record needs, inside objects the driver keeps whole
        fcsd = line.get("full_cluster_single_decision_us") or {}
        line["config"]["results"] = {
            "parity_vs_oracle": line.get("parity_vs_oracle"),
            "p50_decision_latency_us": line.get("p50_decision_latency_us"), "p99_decision_latency_us": line.get("p99_decision_latency_us"),
            "p50_decision_latency_us_under_churn": line.get("p50_decision_latency_us_under_churn"),
            "p99_decision_latency_us_under_churn": line.get("p99_decision_latency_us_under_churn"),
            "full_cluster_single_decision_us": fcsd or None,
            "churn_events_per_s": (line.get("churn") or {}).get("events_per_s") if isinstance(line.get("churn"), dict) else None,
            "pod_axis_ms_per_batch": [{k: pa.get(k) for k in ("workload", "shards", "ms_per_batch", "parity_vs_oracle") if k in pa}
                                      for pa in (line.get("pod_axis") or []) if isinstance(pa, dict)],
            "full_cluster_decisions_per_s": (line.get("full_cluster") or {}).get("value") if isinstance(line.get("full_cluster"), dict) else None,
        }
        line["roofline"]["parity_vs_oracle"] = line.get("parity_vs_oracle")
    emit()
    if world > 1:
        # the other ranks wait for rank 0's single-process legs here, still under the watchdog
        dist.barrier()
    dog.cancel()

    close()
    if rank == 0 and parity is False:
        sys.exit(3)


if __name__ == "__main__":
    main()
