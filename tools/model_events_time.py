"""Device span and call wall of registry events by key on C3 (10k pods x 100k models), beside the route there was before it:

    mmp_models_events_json of 1k / 100k events    beside  a Python dict from id to row, then mmp_models_upsert_json by index
    mmp_model_ids_load of the 100k ids, mmp_model_ids_resolve of 1k / 100k keys, mmp_model_ids_get of all rows

    python tools/model_events_time.py [--repeats 5] [--new 0.1]

The events of one call are the same on both routes: a share `--new` of them carries an id nobody has seen (fresh ones in every
repeat, so every repeat joins as many rows), the rest update known rows drawn with repeats.  The dict route runs on a second
context over the same registry; its wall includes the dict lookups, which is the work the by-key call takes off the host.

One JSON line per route: medians over `repeats` calls after 1 warm-up call, device span (mmp_profile / mmp_last_kernel_ms; -1
where the call brackets none) and wall time of the Solver call, both in microseconds."""
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


def timed(s, fn, repeats, warmup=1):
    wall, span = [], []
    for k in range(warmup + repeats):
        t0 = time.perf_counter()
        fn(k)
        t1 = time.perf_counter()
        if k >= warmup:
            wall.append(1e6 * (t1 - t0))
            ms = s.last_kernel_ms()
            span.append(1e3 * ms if ms >= 0 else -1.0)
    return round(float(np.median(span)), 1), round(float(np.median(wall)), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--new", type=float, default=0.1)
    a = ap.parse_args()
    rng = np.random.default_rng(0xC3)
    fleet = wl.make_fleet("C3")
    M, P = fleet.n_models, fleet.n_pods
    ids = wire.make_ids(rng, P)
    wire.adopt_ids(fleet, ids)
    type_names = ["NLCLASSIFIER"] + ["type-%d" % t for t in range(1, max(fleet.n_types, 1))]
    mv = [v.encode() for v in wire.model_values(fleet, ids, type_names, rng, np.zeros(M, np.int64))]
    mids = [b"model-%07d-%05x" % (i, int(x)) for i, x in enumerate(rng.integers(0, 16**5, M))]

    def line(route, n, span, wall):
        print(json.dumps({"route": route, "fleet": "C3", "n": n, "device_us": span, "wall_us": wall}), flush=True)

    s, t = (Solver(fleet.min_space_units, fleet.min_churn_age_ms) for _ in range(2))
    for ctx in (s, t):
        ctx.profile(True)
        ctx.load_pod_ids(ids)
        ctx.load_type_names(type_names, 0)
        assert not ctx.ingest_models_json(mv)[0].any()
    line("mmp_model_ids_load", M, *timed(s, lambda k: s.model_ids_load(mids), a.repeats))
    row_of = {k: i for i, k in enumerate(mids)}  # the map the dict route keeps on the host
    for n in (1000, 100000):
        n_new = int(n * a.new)
        src = rng.integers(0, M, n)
        vals = [mv[i] for i in rng.integers(0, M, n)]
        fresh_at = rng.choice(n, n_new, replace=False)

        def keys_of(k, route):
            keys = [mids[i] for i in src]
            for j, at in enumerate(fresh_at):
                keys[at] = b"joiner-%s-%d-%d-%d" % (route, n, k, j)
            return keys

        def by_key(k):
            s.models_events_json(keys_of(k, b"k"), vals)

        def by_dict(k):
            idx = np.zeros(n, np.int32)
            for i, key in enumerate(keys_of(k, b"d")):
                r = row_of.get(key)
                if r is None:
                    r = row_of[key] = len(row_of)
                idx[i] = r
            t.upsert_models_json(vals, idx)

        line("mmp_models_events_json", n, *timed(s, by_key, a.repeats))
        line("dict + mmp_models_upsert_json", n, *timed(t, by_dict, a.repeats))
        keys = [mids[i] for i in src]
        line("mmp_model_ids_resolve", n, *timed(s, lambda k: s.model_ids_resolve(keys), a.repeats))
    line("mmp_model_ids_get", s.n_models, *timed(s, lambda k: s.model_ids_get(), a.repeats))
    s.close()
    t.close()


if __name__ == "__main__":
    main()
