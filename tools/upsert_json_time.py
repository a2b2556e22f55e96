"""Device span and call wall of mmp_models_upsert_json for bursts of registry events on C3 (10k pods x 100k models), beside the
two routes there were for the same bytes: a full mmp_models_ingest_json of the registry, and mmp_models_upsert of pre-parsed
rows (the floor: the same apply with the parsing left out and the entries crossing from the host).

    python tools/upsert_json_time.py [--bursts 1,256,4096,100000] [--repeats 7]

A burst of n events names n distinct rows and carries the stored values (modelmesh_amd.wire.model_values) of n other models, so
every event rewrites its row.  One JSON line per burst and one for the full reload: medians over `repeats` calls after 2 warm-up
calls, device span (mmp_profile / mmp_last_kernel_ms) and wall time of the call, both in microseconds."""
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
        fn()
        t1 = time.perf_counter()
        if k >= warmup:
            wall.append(1e6 * (t1 - t0))
            span.append(1e3 * s.last_kernel_ms())
    return round(float(np.median(span)), 1), round(float(np.median(wall)), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bursts", default="1,256,4096,100000")
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    rng = np.random.default_rng(0xC3)
    fleet = wl.make_fleet("C3")
    M, P = fleet.n_models, fleet.n_pods
    ids = wire.make_ids(rng, P)
    wire.adopt_ids(fleet, ids)
    type_names = ["NLCLASSIFIER"] + ["type-%d" % t for t in range(1, max(fleet.n_types, 1))]
    values = [v.encode() for v in wire.model_values(fleet, ids, type_names, rng, np.zeros(M, np.int64))]
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    s.load_pod_ids(ids)
    s.load_pods(fleet.pods)
    s.load_types(fleet.n_types, fleet.allowed, fleet.prefer, fleet.has_allowed, fleet.has_prefer)
    s.load_type_names(type_names, 0)
    s.commit()
    s.profile(True)

    def reload():
        status, _ = s.ingest_models_json(values)
        assert not status.any()
    span, wall = timed(s, reload, a.repeats)
    print(json.dumps({"route": "mmp_models_ingest_json", "fleet": "C3", "records": M, "bytes": sum(map(len, values)),
                      "device_us": span, "wall_us": wall}), flush=True)
    for n in (int(x) for x in a.bursts.split(",")):
        n = min(n, M)
        rows = rng.permutation(M)[:n].astype(np.int32)
        src = (rows + 1 + rng.integers(0, M - 1, n)) % M
        vals = [values[k] for k in src]

        def events():
            status, _ = s.upsert_models_json(vals, rows)
            assert not status.any()
        j_span, j_wall = timed(s, events, a.repeats)
        # the same records pre-parsed: rows with their entries, as mmp_models_upsert takes them
        m = fleet.models[src].copy()
        cnt = (m["n_loaded"] + m["n_failed"]).astype(np.int64)
        off = np.zeros(n + 1, np.int64)
        np.cumsum(cnt, out=off[1:])
        seg = np.repeat(np.arange(n), cnt)
        take = m["ent_off"][seg] + (np.arange(int(off[-1])) - off[seg])
        ep, et = fleet.ent_pod[take], fleet.ent_time[take]
        m["ent_off"] = off[:-1]
        u_span, u_wall = timed(s, lambda: s.upsert_models(rows, m, ep, et), a.repeats)
        print(json.dumps({"route": "burst", "fleet": "C3", "events": n, "bytes": sum(map(len, vals)), "entries": int(off[-1]),
                          "upsert_json_device_us": j_span, "upsert_json_wall_us": j_wall,
                          "upsert_rows_device_us": u_span, "upsert_rows_wall_us": u_wall}), flush=True)
    s.close()


if __name__ == "__main__":
    main()
