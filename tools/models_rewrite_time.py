"""Device span and call wall of mmp_models_rewrite_json on C3 (10k pods x 100k models) at n = 64, 4 096 and the whole registry,
beside mmp_models_upsert_json over the same records in the same run: the rewrite reads the same bytes and writes about as many.

    python tools/models_rewrite_time.py [--sizes 64,4096,100000] [--repeats 7]

The registry is loaded from the stored values (modelmesh_amd.wire.model_values); a batch of n names n distinct rows with their
own stored values, a last_unload for each and a load failure on one row in sixteen.  The rewrite is timed as its write call
(size pass + scan + write pass, the buffer sized by one call before) and as its sizes-only call (parser + size pass + scan), so
that the two passes can be told apart; the upsert writes the same values back into their own rows.  One JSON line per size:
medians over `repeats` calls after 2 warm-up calls, device span (mmp_profile / mmp_last_kernel_ms) and wall time in
microseconds, and the ratio of the two device spans."""
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
    ap.add_argument("--sizes", default="64,4096,100000")
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
    status, _ = s.ingest_models_json(values)
    assert not status.any()
    s.profile(True)
    for n in (int(x) for x in a.sizes.split(",")):
        n = min(n, M)
        rows = np.sort(rng.permutation(M)[:n]).astype(np.int32)
        vals = [values[k] for k in rows]
        lul = rng.integers(0, 2, n) * rng.integers(1, 10**12, n)
        fail_pod = np.where(np.arange(n) % 16 == 0, fleet.ent_pod[np.minimum(fleet.models["ent_off"][rows], len(fleet.ent_pod) - 1)], -1)
        fail_pod = np.where((fail_pod >= 0) & (fail_pod < P), fail_pod, -1).astype(np.int32)
        msgs = [b"load failed: out of memory" if p >= 0 else b"" for p in fail_pod]
        args = (rows, vals, lul, (fail_pod, msgs))
        _, _, st, total, rc = s.models_rewrite_json_raw(*args, 0)
        assert rc == 0 and not st.any()

        def write():
            assert s.models_rewrite_json_raw(*args, total)[4] == 0

        def sizes():
            assert s.models_rewrite_json_raw(*args, 0, null_out=True)[4] == 0

        def upsert():
            status, _ = s.upsert_models_json(vals, rows)
            assert not status.any()
        w_span, w_wall = timed(s, write, a.repeats)
        z_span, z_wall = timed(s, sizes, a.repeats)
        u_span, u_wall = timed(s, upsert, a.repeats)
        print(json.dumps({"fleet": "C3", "values": n, "bytes_in": sum(map(len, vals)), "bytes_out": int(total),
                          "rewrite_device_us": w_span, "rewrite_wall_us": w_wall, "rewrite_sizes_only_device_us": z_span,
                          "rewrite_sizes_only_wall_us": z_wall, "upsert_json_device_us": u_span, "upsert_json_wall_us": u_wall,
                          "device_ratio": round(w_span / u_span, 2) if u_span > 0 else None}), flush=True)
    s.close()


if __name__ == "__main__":
    main()
