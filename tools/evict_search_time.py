"""Call wall and device span of mmp_evict_batch on caches of 20, 1 024, 8 192 and 65 536 entries, by the walk and by the search over
prefix weights (evict_tree_kernels.hpp); what building the tables adds to mmp_caches_load; and a one-operation mmp_cache_replay on
65 536 entries (the replay writes another store and builds nothing: the figure is there to show it).

    python tools/evict_search_time.py [--calls 30] [--processes 2] [--parent TREE]

n = 1, 256 and 2 048 evaluations ride a latency slot, 16 384 are staged.  Caches are full (capacity = the sum of the weights), so an
insert evicts one or two entries; stamps are spread over the deque, three in ten are "now".  The 20-entry shape is 10 000 caches,
the others one cache.  Routes, each a fresh child process with a context of its own:
  walk     MMP_EVICT_SEARCH_FROM=1000000   evict_batch_kernel, as before
  search   MMP_EVICT_SEARCH_FROM=0         evict_search_kernel, every cache searched
  default  no switch
  parent   the same series run from TREE, a built checkout of the commit before (it has no search: its walk, its load)
Wall is closed by the call's own synchronise (the slot's completion word, or the staged batch's hipStreamSynchronize).  The device
span is mmp_last_kernel_ms, which the latency slots do not take: it is there for the staged size, -1 elsewhere.  Medians over
`calls` calls after 3 warm-up calls; the children of a route run `processes` times, alternating with the other routes: the spread
of a figure between them is the run-to-run band.  One JSON line per figure and process, then the comparisons."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

NOW = 1_760_000_000_000
WARM = 3
SIZES, BATCHES = (20, 1024, 8192, 65536), (1, 256, 2048, 16384)
ROUTES = {"walk": "1000000", "search": "0", "default": None, "parent": None}
med = lambda xs: round(float(np.median(xs)), 1)  # noqa: E731


def child(route, calls, root):
    sys.path.insert(0, root)
    from modelmesh_amd import _lib
    from modelmesh_amd.solver import Solver
    s = Solver(100, 1000)
    s.profile(True)
    out = lambda **kw: print(json.dumps({"route": route, "pid": os.getpid(), "calls": calls, **kw}), flush=True)  # noqa: E731
    for E in SIZES:
        nc = 10_000 if E == 20 else 1
        lu = np.tile(NOW - 10 * E + 10 * np.arange(E), nc).astype(np.int64)
        wt = np.tile(1 + (7 * np.arange(E)) % 5, nc).astype(np.int32)
        seg, cap = E * np.arange(nc + 1), np.full(nc, int(wt[:E].sum()))
        wall, dev = [], []
        for k in range(WARM + 5):
            t0 = time.perf_counter()
            s.load_caches(seg, lu, wt, cap)
            wall.append(1e6 * (time.perf_counter() - t0)), dev.append(1e3 * s.last_kernel_ms())
        out(what="load", entries=E, caches=nc, wall_us=med(wall[WARM:]), build_device_us=med(dev[WARM:]))
        rng = np.random.default_rng(E)
        for n in BATCHES:
            reqs = np.zeros(n, dtype=_lib.EVICT_REQ)
            reqs["cache"], reqs["weight"] = rng.integers(0, nc, n), 3
            reqs["last_used"] = np.where(rng.random(n) < 0.3, 0, NOW - rng.integers(0, 10 * E + 10, n))
            wall, dev = [], []
            for k in range(WARM + calls):
                t0 = time.perf_counter()
                got = s.evict(reqs, NOW)
                wall.append(1e6 * (time.perf_counter() - t0)), dev.append(1e3 * s.last_kernel_ms() if n > 2048 else -1)
            out(what="evict", entries=E, n=n, wall_us=med(wall[WARM:]), device_us=med(dev[WARM:]),
                sum=int(got["n_victims"].sum() + got["insert_pos"].sum() + got["weighted_size"].sum() % 1000003))
    E = 65536
    s.cache_slots_limit(262144)
    op = np.zeros(1, dtype=_lib.CACHE_OP)
    op["op"], op["key"] = _lib.COP_GET, E // 2
    wall = []
    for k in range(WARM + 10):
        s.load_caches_keyed([0, E], NOW - 10 * E + 10 * np.arange(E), np.ones(E, np.int32), np.arange(E), [E])
        t0 = time.perf_counter()
        s.cache_replay(op, NOW)
        wall.append(1e6 * (time.perf_counter() - t0))
    out(what="replay, one get", entries=E, wall_us=med(wall[WARM:]))
    s.close()


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--processes", type=int, default=2)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--child", nargs=2, default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.calls, a.child[1])
    rows = []
    for _ in range(a.processes):
        for route, sw in ROUTES.items():
            if route == "parent" and not a.parent:
                continue
            env = {k: v for k, v in os.environ.items() if k != "MMP_EVICT_SEARCH_FROM"}
            env.update({"MMP_EVICT_SEARCH_FROM": sw} if sw else {})
            root = os.path.abspath(a.parent) if route == "parent" else here
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", route, root, "--calls", str(a.calls)],
                                 capture_output=True, text=True, check=True, env=env, timeout=240).stdout
            sys.stdout.write(out)
            rows += [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]
    pick = lambda f, **kw: [r[f] for r in rows if all(r.get(k) == v for k, v in kw.items())]  # noqa: E731
    for E in SIZES:
        for n in BATCHES:
            sums = set(pick("sum", what="evict", entries=E, n=n))
            print(json.dumps({"what": "evict by route", "entries": E, "n": n, "same_answers": len(sums) == 1,
                              **{f"{r}_wall_us": pick("wall_us", what="evict", route=r, entries=E, n=n) for r in ROUTES},
                              **{f"{r}_device_us": pick("device_us", what="evict", route=r, entries=E, n=n) for r in ROUTES}}), flush=True)
        print(json.dumps({"what": "load by route", "entries": E, **{f"{r}_wall_us": pick("wall_us", what="load", route=r, entries=E) for r in ROUTES},
                          "build_device_us": pick("build_device_us", what="load", route="search", entries=E)}), flush=True)
    print(json.dumps({"what": "replay by route", **{f"{r}_wall_us": pick("wall_us", what="replay, one get", route=r) for r in ROUTES}}), flush=True)


if __name__ == "__main__":
    main()
