"""Call wall and device span of mmp_evict_batch_k on one bound cache of 2 000, 8 192 and 65 536 entries, n = 1, 256 and 4 096 rows,
against what it replaces: mmp_cache_read_k of the whole deque + mmp_caches_load of it + mmp_evict_batch of the same questions (the
three calls are the parent commit's own; this tree did not change them).

    python tools/evict_resident_time.py [--calls 20] [--processes 2]

Routes, timed in turn inside each child so that they alternate:
  fresh    a one-operation mmp_cache_replay_k (a read of an absent id: the store generation moves, the deque does not) in front of
           every timed call, outside the timed window: the call builds its tables
  repeat   the call again on the unchanged store: the tables are reused
  three    read_k + caches_load + evict_batch
Wall is closed by each call's own synchronise; device_us is mmp_last_kernel_ms of the evaluation call (for `three`: of
mmp_evict_batch, -1 where it rides a latency slot).  The cache is full (capacity = the sum of the weights); stamps are spread over
the deque, three in ten "now"; every row asks an absent id.  Medians over `calls` calls after 3 warm-up calls; `processes` children
run one after the other: the spread between them is the run-to-run band.  One JSON line per figure and process."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

NOW = 1_760_000_000_000
WARM = 3
SIZES, BATCHES = (2000, 8192, 65536), (1, 256, 4096)
med = lambda xs: round(float(np.median(xs)), 1)  # noqa: E731


def child(calls):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from modelmesh_amd import _lib
    from modelmesh_amd.solver import Solver
    E_max = max(SIZES)
    ids = [b"model-%07d" % r for r in range(E_max + 1)]
    s = Solver(100, 1000)
    s.profile(True)
    s.load_pod_ids(["aaaaaa-1"])
    rows = np.zeros(len(ids), _lib.MODEL_ROW)
    rows["last_used"] = 1
    s.load_models(rows, np.zeros(0, np.int32), np.zeros(0, np.int64))
    s.model_ids_load(ids)
    s.cache_slots_limit(262144)
    touch = np.zeros(1, dtype=_lib.CACHE_OP)
    touch["op"] = _lib.COP_GET
    for E in SIZES:
        lu = (NOW - 10 * E + 10 * np.arange(E)).astype(np.int64)
        wt = (1 + (7 * np.arange(E)) % 5).astype(np.int32)
        cap = int(wt.sum())
        s.load_caches_keyed_k([0, E], lu, wt, ids[:E], [cap])
        rng = np.random.default_rng(E)
        for n in BATCHES:
            ops = np.zeros(n, dtype=_lib.CACHE_OP)
            ops["op"], ops["arg"] = _lib.COP_PUT_IF_ABSENT, 3
            ops["time"] = np.where(rng.random(n) < 0.3, 0, NOW - rng.integers(0, 10 * E + 10, n))
            blob, off = s.pack_keys([ids[E_max]] * n)
            reqs = np.zeros(n, dtype=_lib.EVICT_REQ)
            reqs["weight"], reqs["last_used"] = 3, ops["time"]
            t = {r: ([], []) for r in ("fresh", "repeat", "three")}
            for k in range(WARM + calls):
                s.cache_replay_k(touch, [ids[E_max]], NOW)
                for r in ("fresh", "repeat"):
                    t0 = time.perf_counter()
                    got = s.evict_batch_k(ops, None, NOW, key_off=off, blob=blob)
                    t[r][0].append(1e6 * (time.perf_counter() - t0)), t[r][1].append(1e3 * s.last_kernel_ms())
                t0 = time.perf_counter()
                st = s.cache_read_k(0, E)
                s.load_caches([0, E], st["last_used"], st["weight"], [st["capacity"]])
                old = s.evict(reqs, NOW)
                t["three"][0].append(1e6 * (time.perf_counter() - t0)), t["three"][1].append(1e3 * s.last_kernel_ms() if n > 2048 else -1)
            same = bool((got["n_evicted"] == old["n_victims"]).all() and (got["weighted_size"] == old["weighted_size"]).all())
            for r, (wall, dev) in t.items():
                print(json.dumps({"route": r, "pid": os.getpid(), "entries": E, "n": n, "wall_us": med(wall[WARM:]),
                                  "device_us": med(dev[WARM:]), "same_answers": same}), flush=True)
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--processes", type=int, default=2)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.calls)
    for _ in range(a.processes):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(a.calls)], capture_output=True, text=True,
                             check=True, timeout=400).stdout
        sys.stdout.write(out)


if __name__ == "__main__":
    main()
