"""Device span and call wall of the single-caller route and miss calls beside the full-row calls on the same requests, on C3
(10k pods x 100k models) with ONE calling instance, at 100 000 and 800 000 requests per call.

    python tools/seam_caller_time.py [--sizes 100000,800000] [--repeats 7]

The request halves are drawn as bench.py draws them for its gate / serve / route legs (the same distributions, restated here:
bench.py keeps them inside its kernel table); what describes the calling instance is drawn once.  The full rows are the
expansion of the compact rows (tests/seam_caller_model.py), so both forms decide the same requests, and their outputs are
compared in the same run.  Per size and run:

  mmp_route_batch   (144 + 48 B per request)  against  mmp_route_batch_c   (48 + 24 B)
  mmp_gate_batch    (144 B per request)       against  the gate half of mmp_miss_batch_c (48 B)

mmp_miss_batch_c's device span is the sum of its two launches' brackets (the guards on the compact rows, then the load targets
as mmp_place_batch_c); its gate half is that span minus the span of mmp_place_batch_c alone on the same load-target rows, both
medians of the same run.  Medians over `repeats` calls after 2 warm-up calls, device span (mmp_profile / mmp_last_kernel_ms) and
wall time in microseconds; the whole is run twice, and the last line says whether each compact span at the largest size stays
within the full-row span plus what the two runs of the full-row call differ by."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modelmesh_amd import _lib  # noqa: E402
from modelmesh_amd import workload as wl  # noqa: E402
from modelmesh_amd.solver import Solver  # noqa: E402
from tests import seam_caller_model as scm  # noqa: E402


def timed(s, fn, repeats, warmup=2):
    wall, span, out = [], [], None
    for k in range(warmup + repeats):
        t0 = time.perf_counter()
        out = fn()
        t1 = time.perf_counter()
        if k >= warmup:
            wall.append(1e6 * (t1 - t0))
            span.append(1e3 * s.last_kernel_ms())
    return round(float(np.median(span)), 1), round(float(np.median(wall)), 1), out


def requests(fleet, s, rng, n, self_pod):
    """One instance's n requests: (caller, place caller, gate rows, serve rows, counters, place rows)."""
    M, P, now = fleet.n_models, fleet.n_pods, fleet.now
    cur = fleet.pods[self_pod]
    c = np.zeros(1, dtype=_lib.SEAM_CALLER)
    c["self_pod"], c["gate_flags"] = self_pod, 0
    c["loading_count"], c["weight_predict_cutoff"] = int(rng.integers(0, 20)), 10
    c["cache_capacity"], c["cache_weighted_size"] = 8_388_608, int(rng.integers(0, 8_388_608))
    c["cache_oldest_time"], c["load_timeout_ms"] = now - int(rng.integers(1, 5_000_000)), 90_000
    for a, b in (("fresh_lru", "lru_time"), ("fresh_capacity", "capacity"), ("fresh_used", "used"), ("fresh_count", "count"),
                 ("fresh_loading_threads", "loading_threads"), ("fresh_in_progress", "loading_in_progress"), ("fresh_rpm", "rpm")):
        c[a] = cur[b]
    c["last_published"] = now - int(rng.integers(500, 170_000))
    c["local_in_flight"], c["last_invoke_time"] = int(rng.integers(0, 3)), now - int(rng.choice([0, 10, 1000]))
    g = np.zeros(n, dtype=_lib.GATE_REQ_C)
    g["model"] = rng.integers(0, M, n)
    g["flags"] = rng.integers(0, 512, n)
    g["size_hint"], g["loader_predicted"] = rng.choice([0, 6400], n), 6400
    g["loaded_time"] = now - rng.integers(1, 5_000_000, n)
    sr = np.zeros(n, dtype=_lib.SERVE_REQ)
    sr["model"], sr["self_pod"] = g["model"], self_pod
    sr["flags"], sr["assume_completed_ms"] = rng.integers(0, 4, n), 3000
    in_use = rng.integers(0, 3, P).astype(np.int32)
    last_used = (now - rng.integers(0, 10_000, P)).astype(np.int64)
    sr, counters = s.serve_counters(sr, in_use, last_used)
    pr = wl.make_requests(fleet, int(rng.integers(1, 1 << 30)), n=n, extra_frac=0.0)[0]
    pr["model"], pr["self_pod"], pr["flags"], pr["extra_off"], pr["n_extra"] = g["model"], self_pod, 0, 0, 0
    for a, b in (("fresh_lru", "lru_time"), ("fresh_capacity", "capacity"), ("fresh_used", "used"), ("fresh_count", "count"),
                 ("fresh_rpm", "rpm")):
        pr[a] = cur[b]
    pc, pq = _lib.split_caller(pr)
    return c, pc, g, scm.serve_request_side(sr), counters, pq


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,800000")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--fleet", default="C3")
    a = ap.parse_args()
    rng = np.random.default_rng(0xC3)
    fleet = wl.make_fleet(a.fleet)
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    s.load_fleet(fleet)
    s.profile(True)
    z32, z64, now = np.zeros(0, np.int32), np.zeros(0, np.int64), fleet.now
    sizes = [int(x) for x in a.sizes.split(",")]
    sets = {n: requests(fleet, s, rng, n, 1) for n in sizes}
    runs = []
    for run in (1, 2):
        for n in sizes:
            c, pc, g, sq, counters, pq = sets[n]
            fg, fs = scm.expand_route(c, g, sq)
            r_span, r_wall, r_out = timed(s, lambda: s.route(fg, fs, counters, z32, z64, z32, now), a.repeats)
            rc_span, rc_wall, rc_out = timed(s, lambda: s.route_c(c, g, sq, counters, z32, z64, z32, now), a.repeats)
            g_span, g_wall, g_out = timed(s, lambda: s.gates(fg, z32, z64, z32, now), a.repeats)
            m_span, m_wall, m_out = timed(s, lambda: s.miss_c(c, pc, g, pq, z32, z64, z32, z32, now), a.repeats)
            p_span, p_wall, p_out = timed(s, lambda: s.place_c(pc, pq, None, now), a.repeats)
            row = {"fleet": a.fleet, "run": run, "requests": n,
                   "route_bytes_per_request": {"full": 144 + 48, "compact": 48 + 24},
                   "gate_bytes_per_request": {"full": 144, "compact": 48},
                   "route_batch_device_us": r_span, "route_batch_wall_us": r_wall,
                   "route_batch_c_device_us": rc_span, "route_batch_c_wall_us": rc_wall,
                   "gate_batch_device_us": g_span, "gate_batch_wall_us": g_wall,
                   "miss_batch_c_device_us": m_span, "miss_batch_c_wall_us": m_wall,
                   "place_batch_c_device_us": p_span, "place_batch_c_wall_us": p_wall,
                   "miss_batch_c_gate_half_device_us": round(m_span - p_span, 1),
                   "route_outputs_equal": same(r_out, rc_out),
                   "gate_outputs_equal": g_out.tobytes() == m_out[0].tobytes(),
                   "place_outputs_equal": p_out.tobytes() == m_out[1].tobytes()}
            assert row["route_outputs_equal"] and row["gate_outputs_equal"] and row["place_outputs_equal"], row
            runs.append(row)
            print(json.dumps(row), flush=True)
    big = [r for r in runs if r["requests"] == max(sizes)]
    verdict = {"requests": max(sizes)}
    for full, compact, key in (("route_batch_device_us", "route_batch_c_device_us", "route"),
                               ("gate_batch_device_us", "miss_batch_c_gate_half_device_us", "gate")):
        spread = abs(big[0][full] - big[1][full])
        verdict[key] = {"full_us": [r[full] for r in big], "compact_us": [r[compact] for r in big], "full_run_to_run_us": round(spread, 1),
                        "compact_within_full_plus_spread": all(r[compact] <= r[full] + spread for r in big)}
    print(json.dumps(verdict), flush=True)
    s.close()


if __name__ == "__main__":
    main()
