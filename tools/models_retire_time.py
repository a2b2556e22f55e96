"""Device span and call wall of mmp_models_retire on C3 (10k pods x 100k models) with 1 %, 10 % and 50 % of the rows retired,
beside the route a host had for the same result before it:

    mmp_models_retire of the rows    beside    mmp_models_ingest_json + mmp_model_ids_load of the survivors

    python tools/models_retire_time.py [--repeats 5]

The retired rows are drawn at random; before every timed retire the whole registry and its ids are loaded again (not timed), so
every repeat compacts the same state.  The reload route is timed at the C boundary with the survivors' values and ids already
packed — the host work of holding and packing them, which the retire takes away, is not in its wall.

One JSON line per route and share: medians over `repeats` calls after 1 warm-up call, device span (mmp_profile /
mmp_last_kernel_ms, the two calls of the reload route added) and wall time of the call(s), both in microseconds."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modelmesh_amd import wire  # noqa: E402
from modelmesh_amd import workload as wl  # noqa: E402
from modelmesh_amd._lib import ptr  # noqa: E402
from modelmesh_amd.solver import Solver  # noqa: E402


def median_us(xs):
    return round(float(np.median(xs)), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    rng = np.random.default_rng(0xC3)
    fleet = wl.make_fleet("C3")
    M, P = fleet.n_models, fleet.n_pods
    ids = wire.make_ids(rng, P)
    wire.adopt_ids(fleet, ids)
    type_names = ["NLCLASSIFIER"] + ["type-%d" % t for t in range(1, max(fleet.n_types, 1))]
    mv = [v.encode() for v in wire.model_values(fleet, ids, type_names, rng, np.zeros(M, np.int64))]
    mids = [b"model-%07d-%05x" % (i, int(x)) for i, x in enumerate(rng.integers(0, 16**5, M))]

    s, t = (Solver(fleet.min_space_units, fleet.min_churn_age_ms) for _ in range(2))
    for ctx in (s, t):
        ctx.profile(True)
        ctx.load_pod_ids(ids)
        ctx.load_type_names(type_names, 0)
    L = s.lib
    for share in (0.01, 0.10, 0.50):
        rows = np.sort(rng.choice(M, int(M * share), replace=False)).astype(np.int32)
        keep = np.ones(M, bool)
        keep[rows] = False
        blob, off = Solver._pack([mv[i] for i in np.nonzero(keep)[0]])
        kblob, koff = Solver._pack([mids[i] for i in np.nonzero(keep)[0]])
        koff32, n_keep = koff.astype(np.int32), int(keep.sum())
        lul, status = np.zeros(n_keep, np.int64), np.zeros(n_keep, np.int32)
        span, wall, rspan, rwall = [], [], [], []
        for k in range(1 + a.repeats):
            assert not s.ingest_models_json(mv)[0].any()
            s.model_ids_load(mids)
            t0 = time.perf_counter()
            remap = s.models_retire(rows)
            t1 = time.perf_counter()
            ms = s.last_kernel_ms()
            assert s.n_models == n_keep and int((remap >= 0).sum()) == n_keep
            t2 = time.perf_counter()
            rc1 = L.mmp_models_ingest_json(t.h, blob, ptr(off), n_keep, ptr(lul), ptr(status))
            ms1 = t.last_kernel_ms()
            rc2 = L.mmp_model_ids_load(t.h, kblob, ptr(koff32), n_keep)
            t3 = time.perf_counter()
            ms2 = t.last_kernel_ms()
            assert rc1 == 0 and rc2 == 0 and not status.any()
            if k:
                span.append(1e3 * ms if ms >= 0 else -1.0)
                wall.append(1e6 * (t1 - t0))
                rspan.append(1e3 * (ms1 + ms2) if ms1 >= 0 and ms2 >= 0 else -1.0)
                rwall.append(1e6 * (t3 - t2))
        for route, sp, wa in (("mmp_models_retire", span, wall), ("mmp_models_ingest_json + mmp_model_ids_load", rspan, rwall)):
            print(json.dumps({"route": route, "fleet": "C3", "rows": M, "retired": len(rows), "device_us": median_us(sp),
                              "wall_us": median_us(wa)}), flush=True)
    s.close()
    t.close()


if __name__ == "__main__":
    main()
