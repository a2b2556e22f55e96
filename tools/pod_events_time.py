"""Device span and call wall of the instance-side entry points on C3 (10k pods x 100k models), each beside the route there was
before it:

    mmp_pod_ids_append of 1 and of 16 ids        beside  mmp_pod_ids_load of the whole list
    mmp_pods_events_json of 1 / 256 events       beside  mmp_pods_ingest_json of the same values by index
    mmp_registry_unresolved (max_models = M)     beside  mmp_registry_census

    python tools/pod_events_time.py [--repeats 7]

One JSON line per route: medians over `repeats` calls after 2 warm-up calls, device span (mmp_profile / mmp_last_kernel_ms; -1
where the call brackets none, as the load) and wall time of the call, both in microseconds.  Every append adds ids for good, so
the table grows by (2 + repeats) * 17 ids over the run: nothing against 10k."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modelmesh_amd import wire  # noqa: E402
from modelmesh_amd import workload as wl  # noqa: E402
from modelmesh_amd.solver import Solver  # noqa: E402


def timed(s, fn, repeats, warmup=2):
    wall, span = [], []
    for k in range(warmup + repeats):
        t0 = time.perf_counter()
        fn(k)
        t1 = time.perf_counter()
        if k >= warmup:
            wall.append(1e6 * (t1 - t0))
            span.append(1e3 * s.last_kernel_ms())
    return round(float(np.median(span)), 1), round(float(np.median(wall)), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    rng = np.random.default_rng(0xC3)
    fleet = wl.make_fleet("C3")
    M, P = fleet.n_models, fleet.n_pods
    ids = wire.make_ids(rng, P)
    wire.adopt_ids(fleet, ids)
    type_names = ["NLCLASSIFIER"] + ["type-%d" % t for t in range(1, max(fleet.n_types, 1))]
    pv = [v.encode() for v in wire.pod_values(fleet, rng, np.full(P, 1000, np.int64))]
    mv = [v.encode() for v in wire.model_values(fleet, ids, type_names, rng, np.zeros(M, np.int64))]
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    s.profile(True)

    def line(route, n, span, wall):
        print(json.dumps({"route": route, "fleet": "C3", "n": n, "device_us": span, "wall_us": wall}), flush=True)

    line("mmp_pod_ids_load", P, *timed(s, lambda k: s.load_pod_ids(ids), a.repeats))
    s.load_type_names(type_names, 0)
    assert not s.ingest_pods_json(pv, np.arange(P))[0].any()
    assert not s.ingest_models_json(mv)[0].any()
    for n in (1, 16):
        line("mmp_pod_ids_append", n, *timed(s, lambda k: s.append_pod_ids(["joiner-%d-%d-%d" % (n, k, j) for j in range(n)]), a.repeats))
    for n in (1, 256):
        idx = rng.permutation(P)[:n].astype(np.int32)
        keys, vals = [ids[i] for i in idx], [pv[(i + 1) % P] for i in idx]
        line("mmp_pods_events_json", n, *timed(s, lambda k: s.pods_events_json(keys, vals), a.repeats))
        line("mmp_pods_ingest_json", n, *timed(s, lambda k: s.ingest_pods_json(vals, idx), a.repeats))
    # (room for every row, so that the list kernel runs; the C3 registry names known ids only, so it lists nothing: the figure
    # is count + scan + the list pass over M rows, without the copy of a list)
    line("mmp_registry_unresolved", M, *timed(s, lambda k: s.registry_unresolved(M), a.repeats))
    line("mmp_registry_census", M, *timed(s, lambda k: s.registry_census_raw(0, 0), a.repeats))
    s.close()


if __name__ == "__main__":
    main()
