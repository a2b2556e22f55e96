#!/usr/bin/env python
"""Wall and device time of the registry ops by id (mmp_registry_ops_k) against the two-call sequence it replaces
(mmp_model_ids_resolve + mmp_registry_ops), at n = 1, 256 and 4096 ops on C3, with MMP_ROPS_APPLY and with flags 0; and at n = 1
beside a thread that issues 800 000-row place batches on the same context (what the calls queue behind on the batch lock).

usage: tools/registry_ops_keyed_time.py [--parent-lib PATH] [--reps R] [--out FILE.jsonl]
The two-call sequence runs in processes of their own against --parent-lib (a libmmplace.so built from the parent commit; default:
this tree's library, whose two calls compute the same), the new call against this tree's library: two processes each,
alternating.  One jsonl row per (process, call, n, flags, contended): p50 and p99 wall in us, median device span in us
(mmp_last_kernel_ms, summed over the two calls of the sequence).  The ops alternate between REGISTER and DEREGISTER of one instance on the same records, so
that an applied series neither grows the records nor runs out of entries and every pair of repetitions does the same work.
Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NS = (1, 256, 4096)
NEW = ("mmp_registry_ops_k",)
BIG = 800_000


def world():
    import numpy as np

    from modelmesh_amd import _lib
    from modelmesh_amd import workload as wl
    from modelmesh_amd.solver import Solver
    fleet = wl.make_fleet("C3")
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    s.load_fleet(fleet)
    ids = [b"model-%06d" % i for i in range(fleet.n_models)]
    s.model_ids_load(ids)
    return s, _lib, np, fleet, ids


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def worker(mode, reps):
    from modelmesh_amd import _lib
    if mode == "compose":
        _lib.SYMBOLS = [x for x in _lib.SYMBOLS if x[0] not in NEW]
    s, _lib, np, fleet, ids = world()
    s.lib.mmp_profile(s.h, 1)
    span = lambda: s.lib.mmp_last_kernel_ms(s.h)  # noqa: E731
    now = int(fleet.now)
    rng = np.random.default_rng(5)
    pod = 3

    def new_call(ops, keys, flags):
        out = s.registry_ops_k_raw(ops, keys, now, flags, len(ops))
        assert out[4] == 0
        return span()

    def two_calls(ops, keys, flags):
        ops = ops.copy()
        ops["model"] = s.model_ids_resolve(keys)
        d = span()
        s.registry_ops_raw(ops, now, flags, len(ops))
        return d + span()

    fn = new_call if mode == "new" else two_calls
    name = "registry_ops_k" if mode == "new" else "resolve+registry_ops"

    def series(n, flags, reps, contended):
        rows = rng.permutation(fleet.n_models)[:n]
        keys = [ids[int(r)] for r in rows]
        put = np.zeros(n, _lib.REGISTRY_OP)            # (model: by key it is ignored, by row the resolve fills it in)
        put["pod"], put["op"], put["last_used"], put["load_time"] = pod, _lib.ROP_REGISTER, now, now
        rem = put.copy()
        rem["op"] = _lib.ROP_DEREGISTER
        for _ in range(3):                             # warm-up: buffers grown, code resident
            fn(put, keys, flags)
            fn(rem, keys, flags)
        wall, dev = [], []
        for r in range(reps):
            ops = put if r % 2 == 0 else rem
            t0 = time.perf_counter()
            d = fn(ops, keys, flags)
            wall.append((time.perf_counter() - t0) * 1e6)
            dev.append(d * 1e3)
        if reps % 2:
            fn(rem, keys, flags)
        print(json.dumps({"mode": mode, "call": name, "n": n, "flags": flags, "contended": contended, "reps": reps,
                          "wall_p50_us": round(pct(wall, 0.5), 1), "wall_p99_us": round(pct(wall, 0.99), 1),
                          "device_us": round(statistics.median(dev), 1), "pid": os.getpid()}), flush=True)

    for n in NS:
        for flags in (_lib.ROPS_APPLY, 0):
            series(n, flags, reps, False)
    # n = 1 beside 800 000-row batches: every call of either form queues behind the batch that holds the lock
    from modelmesh_amd import workload as wl
    reqs, extra = wl.make_requests(fleet, 7, BIG)
    stop = threading.Event()

    def batches():
        while not stop.is_set():
            s.place(reqs, extra, fleet.now)
    s.place(reqs, extra, fleet.now)
    t = threading.Thread(target=batches)
    t.start()
    try:
        for flags in (_lib.ROPS_APPLY, 0):
            series(1, flags, max(reps, 60), True)
    finally:
        stop.set()
        t.join()
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker")
    ap.add_argument("--parent-lib")
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.reps)
    lines = []
    for _ in range(2):  # two processes each, alternating
        for mode in ("new", "compose"):
            env = dict(os.environ)
            if mode == "compose" and a.parent_lib:
                env["MMP_LIB_PATH"] = os.path.abspath(a.parent_lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", mode, "--reps", str(a.reps)], env=env, text=True,
                               stdout=subprocess.PIPE, check=True, timeout=280)
            sys.stdout.write(p.stdout)
            sys.stdout.flush()
            lines.append(p.stdout)
    if a.out:
        with open(a.out, "w") as f:
            f.write("".join(lines))


if __name__ == "__main__":
    main()
