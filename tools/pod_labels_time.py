"""Device span and call wall of the two instance JSON calls on C3 (10k pods), with the label table loaded and without:

    mmp_pods_ingest_json over the 10 000 instance values
    mmp_pods_events_json of 1 / 256 / 10 000 events

    python tools/pod_labels_time.py [--repeats 7] [--no-table-only]

C3's values hold `"labels":["gpu","l<k>"]`; the table loaded here names "gpu", "l0" .. "l3" and 59 labels no value holds, so a
lookup probes a full-width table.  One JSON line per route and mode: medians over `repeats` calls after 2 warm-up calls, device
span (mmp_profile / mmp_last_kernel_ms: with a table it covers the second launch, ingest_pod_labels_kernel) and wall time of the
call, both in microseconds, and min / max of the span as the run-to-run spread.  A library that has no label entry points (a
commit before them) reports the `no table` lines alone: the lines to hold the later ones against."""
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

NAMES = ["gpu", "l0", "l1", "l2", "l3"] + ["label-%d" % i for i in range(5, 64)]


def timed(s, fn, repeats, warmup=2):
    wall, span = [], []
    for k in range(warmup + repeats):
        t0 = time.perf_counter()
        fn(k)
        t1 = time.perf_counter()
        if k >= warmup:
            wall.append(1e6 * (t1 - t0))
            span.append(1e3 * s.last_kernel_ms())
    return (round(float(np.median(span)), 1), round(float(np.median(wall)), 1), round(float(np.min(span)), 1),
            round(float(np.max(span)), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-table-only", action="store_true", help="skip the runs with a label table (to count launches under a profiler)")
    a = ap.parse_args()
    rng = np.random.default_rng(0xC3)
    fleet = wl.make_fleet("C3")
    P = fleet.n_pods
    ids = wire.make_ids(rng, P)
    wire.adopt_ids(fleet, ids)
    pv = [v.encode() for v in wire.pod_values(fleet, rng, np.full(P, 1000, np.int64))]
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    s.profile(True)
    s.load_pod_ids(ids)
    modes = [("no table", None)] + ([("table", NAMES)] if hasattr(s, "label_names_load") and not a.no_table_only else [])
    picks = {n: rng.permutation(P)[:n].astype(np.int32) for n in (1, 256, P)}

    def line(route, mode, n, span, wall, lo, hi):
        print(json.dumps({"route": route, "labels": mode, "fleet": "C3", "n": n, "device_us": span, "wall_us": wall,
                          "device_us_min": lo, "device_us_max": hi}), flush=True)

    for mode, names in modes:
        if names is not None:
            s.label_names_load(names)
        status, _ = s.ingest_pods_json(pv, np.arange(P))
        assert not status.any()
        if names is not None:
            words, counts = s.pod_labels_get()
            assert (counts == 2).all() and all(int(words[p]) == 1 | (2 << (p % 4)) for p in range(0, P, 97))
        line("mmp_pods_ingest_json", mode, P, *timed(s, lambda k: s.ingest_pods_json(pv, np.arange(P)), a.repeats))
        for n, idx in picks.items():
            keys, vals = [ids[i] for i in idx], [pv[i] for i in idx]
            line("mmp_pods_events_json", mode, n, *timed(s, lambda k: s.pods_events_json(keys, vals), a.repeats))
    s.close()


if __name__ == "__main__":
    main()
