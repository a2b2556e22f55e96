"""Device span and call wall of mmp_models_register_json on C3 (10k pods x 100k models) at n = 64, 4 096 and the whole registry,
beside mmp_models_rewrite_json over the same stored values in the same run: the rewrite is the nearest call with the same pass
structure (parser, size pass, scan, one read-back, write pass).

    python tools/models_register_time.py [--sizes 64,4096,100000] [--repeats 7]

The registry is loaded from the stored values (modelmesh_amd.wire.model_values) and its rows are named.  A batch of n names n
distinct rows: one third creations (no stored value), one third touches (the stored value of the row, its type asked for, lu far
enough behind) and one third exists (the same with loadNow), every request with its key, so that the by-key stage runs too.  The
call is timed as its write call (the buffer sized by one call before) and as its sizes-only call, so that the two passes can be
told apart; the rewrite renders the same stored values with a last_unload each.  One JSON line per size: medians over `repeats`
calls after 2 warm-up calls, device span (mmp_profile / mmp_last_kernel_ms) and wall time in microseconds, and the ratio of the two
device spans."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modelmesh_amd import _lib  # noqa: E402
from modelmesh_amd import wire  # noqa: E402
from modelmesh_amd import workload as wl  # noqa: E402
from modelmesh_amd.solver import Solver  # noqa: E402

AGE = 3_600_000


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
    keys = [b"model-%06d" % k for k in range(M)]
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    s.load_pod_ids(ids)
    s.load_pods(fleet.pods)
    s.load_types(fleet.n_types, fleet.allowed, fleet.prefer, fleet.has_allowed, fleet.has_prefer)
    s.load_type_names(type_names, 0)
    s.commit()
    status, _ = s.ingest_models_json(values)
    assert not status.any()
    s.model_ids_load(keys)
    now = int(fleet.models["last_used"].max()) + 100 * AGE  # every stored lu lies more than 6 ages behind: a register touches
    s.profile(True)
    for n in (int(x) for x in a.sizes.split(",")):
        n = min(n, M)
        rows = np.sort(rng.permutation(M)[:n]).astype(np.int32)
        vals = [values[k] for k in rows]
        kind = np.arange(n) % 3  # 0 creation, 1 touch, 2 exists
        reqs = np.zeros(n, _lib.REGISTER_REQ)
        reqs["flags"] = np.where(kind == 2, _lib.MREG_LOAD_NOW, 0)
        infos = [(type_names[int(fleet.models["type"][r])].encode(), b"", b"s3://bucket/m%d" % r) for r in rows]  # (as wire.model_values)
        olds = [b"" if kind[i] == 0 else vals[i] for i in range(n)]
        bkeys = [keys[r] for r in rows]
        args = (reqs, infos, olds, now, AGE, bkeys)
        r = s.models_register_json_raw(*args, 0)
        total = r[5]
        counts = np.bincount(r[2], minlength=9)
        assert r[6] == 0 and np.array_equal(r[4], rows), "the rows of the keys"
        assert counts[_lib.MREG_CREATED] + counts[_lib.MREG_TOUCHED] + counts[_lib.MREG_EXISTS] == n, counts
        lul = rng.integers(1, 10**12, n)
        rw_args = (rows, vals, lul, None)
        _, _, st, rw_total, rc = s.models_rewrite_json_raw(*rw_args, 0)
        assert rc == 0 and not st.any()

        def write():
            assert s.models_register_json_raw(*args, total)[6] == 0

        def sizes():
            assert s.models_register_json_raw(*args, 0, null_out=True)[6] == 0

        def rewrite():
            assert s.models_rewrite_json_raw(*rw_args, rw_total)[4] == 0

        def rewrite_sizes():
            assert s.models_rewrite_json_raw(*rw_args, 0, null_out=True)[4] == 0
        w_span, w_wall = timed(s, write, a.repeats)
        z_span, z_wall = timed(s, sizes, a.repeats)
        r_span, r_wall = timed(s, rewrite, a.repeats)
        rz_span, rz_wall = timed(s, rewrite_sizes, a.repeats)
        print(json.dumps({"fleet": "C3", "requests": n, "created": int(counts[_lib.MREG_CREATED]), "touched": int(counts[_lib.MREG_TOUCHED]),
                          "exists": int(counts[_lib.MREG_EXISTS]), "conflict": int(counts[_lib.MREG_CONFLICT]),
                          "bytes_in": sum(map(len, olds)), "bytes_out": int(total),
                          "register_device_us": w_span, "register_wall_us": w_wall, "register_sizes_only_device_us": z_span,
                          "register_sizes_only_wall_us": z_wall, "rewrite_bytes_in": sum(map(len, vals)), "rewrite_bytes_out": int(rw_total),
                          "rewrite_device_us": r_span, "rewrite_wall_us": r_wall, "rewrite_sizes_only_device_us": rz_span,
                          "rewrite_sizes_only_wall_us": rz_wall,
                          "device_ratio": round(w_span / r_span, 2) if r_span > 0 else None}), flush=True)
    s.close()


if __name__ == "__main__":
    main()
