"""Call wall and device span of mmp_cache_replay on ONE cache of 2 047, 8 192 and 65 536 deque slots: what the blocked deque in
global memory (cache_wide_kernels.hpp) costs per operation, and what it costs beside the LDS kernel where both can run.

    python tools/cache_wide_time.py [--calls 30] [--processes 2]
    python tools/cache_wide_time.py --one-op        (20 one-operation calls at 65 536 entries: the run to put under a kernel trace)

Two streams of n = 1, 256 and 4 096 operations:
  get   reads of random live keys stamped "now": every one unlinks an entry from the middle and links it at the tail
  put   putIfAbsent of new keys stamped "now" on a full cache of unit weights: every one evicts the head
The cache has `slots` entries for the get stream and slots - n entries for the put stream (a call's slots are its entries + its
inserts; 4 096 puts do not fit 2 047 slots and are left out there).  The state is loaded again before every call (not timed), so
every call of a series does the same work.  At 2 047 slots the series runs twice: by default through cache_replay_kernel<64> (LDS),
and in a child with MMP_CACHE_WIDE_FROM=0 through the blocked kernels.

Wall is closed by the call's own synchronise; the device span is mmp_last_kernel_ms (spread + replay + compact on the blocked
route).  Medians over `calls` calls after 3 warm-up calls.  The series runs in `processes` fresh child processes per route, one
after the other: the spread of a figure between them is the run-to-run band.  One JSON line per figure and process, then the
comparisons."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modelmesh_amd import _lib  # noqa: E402
from modelmesh_amd.solver import Solver  # noqa: E402

NOW = 1_760_000_000_000
WARM = 3


def series(s, route, slots, n, stream, calls):
    E = slots if stream == "get" else slots - n
    lu = (NOW - 10 * E + 10 * np.arange(E)).astype(np.int64)
    wt, keys = np.ones(E, np.int32), np.arange(E, dtype=np.int32)
    rng = np.random.default_rng(slots + n)
    ops = np.zeros(n, dtype=_lib.CACHE_OP)
    if stream == "get":
        ops["op"], ops["key"] = _lib.COP_GET, rng.integers(0, E, n)
    else:
        ops["op"], ops["key"], ops["arg"] = _lib.COP_PUT_IF_ABSENT, E + np.arange(n), 1
    wall, dev = [], []
    for k in range(WARM + calls):
        s.load_caches_keyed([0, E], lu, wt, keys, [E])
        t0 = time.perf_counter()
        outs, ev = s.cache_replay(ops, NOW)
        t1 = time.perf_counter()
        assert (outs["result"] == 1).all() and len(ev) >= (n if stream == "put" else 0)
        if k >= WARM:
            wall.append(1e6 * (t1 - t0)), dev.append(1e3 * s.last_kernel_ms())
    med = lambda xs: round(float(np.median(xs)), 1)  # noqa: E731
    print(json.dumps({"route": route, "pid": os.getpid(), "slots": slots, "stream": stream, "n": n, "calls": calls, "wall_us": med(wall),
                      "device_us": med(dev), "device_us_per_op": round(med(dev) / n, 2)}), flush=True)


def child(route, calls):
    s = Solver(100, 1000)
    s.profile(True)
    s.cache_slots_limit(262144)
    for slots in ((2047,) if route == "wide@2047" else (2047, 8192, 65536)):
        for stream in ("get", "put"):
            for n in (1, 256, 4096):
                if stream == "get" or n < slots:
                    series(s, route if slots == 2047 else "wide", slots, n, stream, calls)
    s.close()


def one_op():
    s = Solver(100, 1000)
    s.cache_slots_limit(262144)
    for _ in range(20):
        series(s, "wide", 65536, 1, "get", 1)
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--processes", type=int, default=2)
    ap.add_argument("--child", default=None)
    ap.add_argument("--one-op", action="store_true")
    a = ap.parse_args()
    if a.one_op:
        return one_op()
    if a.child:
        return child(a.child, a.calls)
    rows = []
    for _ in range(a.processes):  # one after the other: each a fresh process with a context of its own
        for route in ("lds", "wide@2047"):
            env = dict(os.environ, **({"MMP_CACHE_WIDE_FROM": "0"} if route != "lds" else {}))
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", route, "--calls", str(a.calls)], capture_output=True,
                                 text=True, check=True, env=env).stdout
            sys.stdout.write(out)
            rows += [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]
    pick = lambda **kw: [r["device_us"] for r in rows if all(r[k] == v for k, v in kw.items())]  # noqa: E731
    for stream in ("get", "put"):
        for n in (1, 256, 4096):
            lds, wide = pick(route="lds", slots=2047, stream=stream, n=n), pick(route="wide@2047", slots=2047, stream=stream, n=n)
            if lds:
                print(json.dumps({"what": "blocked / LDS at 2047 slots", "stream": stream, "n": n, "lds_device_us": lds, "wide_device_us": wide,
                                  "ratio": round(float(np.median(wide) / np.median(lds)), 2)}), flush=True)
            a8, a64 = pick(route="wide", slots=8192, stream=stream, n=n), pick(route="wide", slots=65536, stream=stream, n=n)
            print(json.dumps({"what": "65536 / 8192 slots, blocked", "stream": stream, "n": n, "device_us_8192": a8, "device_us_65536": a64,
                              "ratio": round(float(np.median(a64) / np.median(a8)), 2)}), flush=True)


if __name__ == "__main__":
    main()
