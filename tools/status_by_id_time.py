#!/usr/bin/env python
"""Wall and device time of the status calls by id (mmp_models_status_k, mmp_vmodels_status) against the multi-call compositions
they replace (model_ids_resolve + models_status; vmodels_resolve + models_status on two rows per vmodel + vmodels_get once per
distinct row, stitched on the host), at n = 1, 256, 4096 and 20000 keys.

usage: tools/status_by_id_time.py [--parent-lib PATH] [--reps R] [--out FILE.jsonl]
The compositions run in processes of their own against --parent-lib (a libmmplace.so built from the parent commit; default: this
tree's library, whose composed calls are unchanged), the new calls against this tree's library: two processes each, alternating.
One jsonl row per (process, call, n): median wall in us, median device span in us (mmp_last_kernel_ms, summed over a composition's
calls; vmodels_get is copies only and has none).  Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NS = (1, 256, 4096, 20000)
NEW = ("mmp_models_status_k", "mmp_vmodels_status")
M, V, P, NOW = 4096, 512, 8, 1_700_000_000_000


def world():
    import numpy as np

    from modelmesh_amd import _lib
    from modelmesh_amd import workload as wl
    from modelmesh_amd.solver import Solver
    fleet = wl.fuzz_fleet(77, pods=P, models=M)
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    s.load_fleet(fleet)
    ids = [b"model-%05d" % i for i in range(M)]
    s.model_ids_load(ids)
    vids = [b"vmodel-%04d" % v for v in range(V)]
    vals = ['{"o":"owner-%d","amid":"%s","tmid":"%s"%s}' % (v % 7, ids[(37 * v) % M].decode(), ids[(37 * v + v % 3) % M].decode(),
                                                          ',"failed":true' if v % 5 == 0 else "") for v in range(V)]
    s.vmodels_events_json(vids, vals)
    rng = np.random.default_rng(5)
    return s, _lib, np, ids, vids, rng


def worker(mode, reps):
    from modelmesh_amd import _lib
    if mode == "compose":
        _lib.SYMBOLS = [x for x in _lib.SYMBOLS if x[0] not in NEW]
    s, _lib, np, ids, vids, rng = world()
    s.lib.mmp_profile(s.h, 1)
    span = lambda: s.lib.mmp_last_kernel_ms(s.h)

    def new_models(keys):
        s.models_status_k(keys, NOW)
        return span()

    def new_vmodels(keys):
        s.vmodels_status(keys, NOW)
        return span()

    def compose_models(keys):
        idx = s.model_ids_resolve(keys)
        d = span()
        reqs = np.zeros(len(keys), _lib.STATUS_REQ)
        reqs["model"], reqs["fail_pod"] = idx, -1
        s.models_status(reqs, NOW)
        return d + span()

    def compose_vmodels(keys):
        a = s.vmodels_resolve(keys)
        d = span()
        reqs = np.zeros(2 * len(keys), _lib.STATUS_REQ)
        reqs["fail_pod"] = -1
        reqs["model"][0::2] = a["model"]
        reqs["model"][1::2] = np.where(a["vstatus"] != 0, a["target_model"], -1)
        s.models_status(reqs, NOW)
        d += span()
        got = {}
        for v in np.unique(a["vmodel"]):
            if v >= 0:
                got[int(v)] = s.vmodels_get(int(v), 1)
        return d

    calls = {"new": (("models_status_k", new_models, ids), ("vmodels_status", new_vmodels, vids)),
             "compose": (("resolve+status", compose_models, ids), ("resolve+status+get", compose_vmodels, vids))}[mode]
    for name, fn, pool in calls:
        for n in NS:
            keys = [pool[int(i)] for i in rng.integers(0, len(pool), n)]
            fn(keys)
            wall, dev = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                d = fn(keys)
                wall.append((time.perf_counter() - t0) * 1e6)
                dev.append(d * 1e3)
            print(json.dumps({"mode": mode, "call": name, "n": n, "reps": reps, "wall_us": round(statistics.median(wall), 1),
                              "device_us": round(statistics.median(dev), 1), "pid": os.getpid()}), flush=True)
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker")
    ap.add_argument("--parent-lib")
    ap.add_argument("--reps", type=int, default=30)
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
                               stdout=subprocess.PIPE, check=True, timeout=300)
            sys.stdout.write(p.stdout)
            lines.append(p.stdout)
    if a.out:
        with open(a.out, "w") as f:
            f.write("".join(lines))


if __name__ == "__main__":
    main()
