"""Wall time of the request seams by model id (mmp_route_batch_ck / mmp_miss_batch_ck / mmp_place_batch_ck) beside the two-call
sequence they replace — mmp_model_ids_resolve, then the _c call on the rows it answered — on C3 (10k pods x 100k models):

    python tools/keyed_seam_time.py [--iters 3000] [--rounds 4] [--events-repeats 5]
    python tools/keyed_seam_time.py --events-only [--label parent]      (runs on a library without the keyed calls as well)

  seams   n = 1 and n = 256 requests per call, (a) on an idle context and (b) while a second thread issues 800 000-row
          host-pointer mmp_place_batch_c batches back to back (they are staged: the batch lock is held for the whole call).
          p50 / p99 of the call's wall time in microseconds, the calling thread pinned to one CPU as bench.py pins it for its
          n = 1 loops; both forms are called through ctypes on arguments prepared once, in alternating blocks (`rounds` blocks of
          `iters` calls each), and their outputs are compared.  The two-call sequence includes writing the resolved rows into the
          request rows, as its caller must.  Beside them the _c call ALONE on rows already known (what a caller with a host id
          map pays): keyed minus that is what the resolution costs inside the call.
  events  wall time of mmp_models_events_json for the registry events of one churn slice (the batch tools/upsert_time.py sends by
          index), by key: once as updates only, once with a tenth of the keys replaced by ids nobody has seen — those join, the id
          table is swapped and the call drains the latency slots behind the swap.  Median, minimum and maximum over
          `events-repeats` calls after one warm-up call.  Run it on the parent commit and on this one (--label) to compare.

One JSON line per measurement."""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))
from modelmesh_amd import _lib  # noqa: E402
from modelmesh_amd import wire  # noqa: E402
from modelmesh_amd import workload as wl  # noqa: E402
from modelmesh_amd._lib import ptr  # noqa: E402
from modelmesh_amd.solver import Solver  # noqa: E402

EXPIRY = 450_000
BIG = 800_000


def world():
    rng = np.random.default_rng(0xC3)
    fleet = wl.make_fleet("C3")
    pod_ids = wire.make_ids(rng, fleet.n_pods)
    wire.adopt_ids(fleet, pod_ids)
    mids = [b"model-%07d-%05x" % (i, int(x)) for i, x in enumerate(rng.integers(0, 16**5, fleet.n_models))]
    return rng, fleet, pod_ids, mids


def percentiles(ns):
    a = np.asarray(ns, np.float64) / 1e3
    return round(float(np.percentile(a, 50)), 2), round(float(np.percentile(a, 99)), 2)


def block(fn, iters, out):
    clock = time.perf_counter_ns
    for _ in range(iters):
        t0 = clock()
        fn()
        out.append(clock() - t0)


def seam_calls(s, lib, fleet, mids, rng, n):
    """{call: (keyed fn, two-call fn, the _c call alone, outputs of the first two)} on arguments prepared once"""
    from seam_caller_time import requests
    c, pc, g, sq, counters, pq = requests(fleet, s, rng, n, 1)
    keys = [mids[int(m)] for m in g["model"]]
    keys[n // 2] = b"an id nobody loaded"  # one miss per call (n = 1: the call's one key is a hit)
    if n == 1:
        keys[0] = mids[int(g["model"][0])]
    blob, off = Solver.pack_keys(keys)
    blob = np.frombuffer(blob, np.uint8).copy()
    now, h = C.c_int64(int(fleet.now)), s.h
    exp = C.c_int64(EXPIRY)
    nc = len(counters)

    def bufs(*dts):
        return [np.zeros(n, dt) for dt in dts]

    calls = {}
    # route
    kg, ks_, kidx = bufs(_lib.GATE_OUT, _lib.SERVE_OUT, np.int32)
    tg, ts_, tidx = bufs(_lib.GATE_OUT, _lib.SERVE_OUT, np.int32)
    g2 = g.copy()
    A = (h, ptr(c), ptr(g), ptr(sq), n, ptr(blob), ptr(off), ptr(counters) if nc else None, nc, None, None, 0, None, 0, now, exp,
         ptr(kg), ptr(ks_), ptr(kidx))
    R = (h, ptr(blob), ptr(off), n, ptr(tidx))
    B = (h, ptr(c), ptr(g2), ptr(sq), n, ptr(counters) if nc else None, nc, None, None, 0, None, 0, now, exp, ptr(tg), ptr(ts_))

    def route_keyed():
        assert lib.mmp_route_batch_ck(*A) == 0

    def route_two():
        assert lib.mmp_model_ids_resolve(*R) == 0
        g2["model"] = tidx
        assert lib.mmp_route_batch_c(*B) == 0

    def route_alone():  # (the rows the last two-call sequence left in g2)
        assert lib.mmp_route_batch_c(*B) == 0
    calls["route"] = (route_keyed, route_two, route_alone, lambda: (kg, ks_, kidx), lambda: (tg, ts_, tidx))
    # miss
    mkg, mkp, mkidx = bufs(_lib.GATE_OUT, _lib.PLACE_OUT, np.int32)
    mtg, mtp, mtidx = bufs(_lib.GATE_OUT, _lib.PLACE_OUT, np.int32)
    g3, p3 = g.copy(), pq.copy()
    MA = (h, ptr(c), ptr(pc), ptr(g), ptr(pq), n, ptr(blob), ptr(off), None, None, 0, None, 0, None, 0, now, exp, ptr(mkg), ptr(mkp), ptr(mkidx))
    MR = (h, ptr(blob), ptr(off), n, ptr(mtidx))
    MB = (h, ptr(c), ptr(pc), ptr(g3), ptr(p3), n, None, None, 0, None, 0, None, 0, now, exp, ptr(mtg), ptr(mtp))

    def miss_keyed():
        assert lib.mmp_miss_batch_ck(*MA) == 0

    def miss_two():
        assert lib.mmp_model_ids_resolve(*MR) == 0
        g3["model"] = mtidx
        p3["model"] = mtidx
        assert lib.mmp_miss_batch_c(*MB) == 0

    def miss_alone():
        assert lib.mmp_miss_batch_c(*MB) == 0
    calls["miss"] = (miss_keyed, miss_two, miss_alone, lambda: (mkg, mkp, mkidx), lambda: (mtg, mtp, mtidx))
    # place
    pko, pkidx = bufs(_lib.PLACE_OUT, np.int32)
    pto, ptidx = bufs(_lib.PLACE_OUT, np.int32)
    p4 = pq.copy()
    PA = (h, ptr(pc), ptr(pq), n, ptr(blob), ptr(off), None, 0, now, ptr(pko), ptr(pkidx))
    PR = (h, ptr(blob), ptr(off), n, ptr(ptidx))
    PB = (h, ptr(pc), ptr(p4), n, None, 0, now, ptr(pto))

    def place_keyed():
        assert lib.mmp_place_batch_ck(*PA) == 0

    def place_two():
        assert lib.mmp_model_ids_resolve(*PR) == 0
        p4["model"] = ptidx
        assert lib.mmp_place_batch_c(*PB) == 0

    def place_alone():
        assert lib.mmp_place_batch_c(*PB) == 0
    calls["place"] = (place_keyed, place_two, place_alone, lambda: (pko, pkidx), lambda: (pto, ptidx))
    keep = (c, pc, g, sq, counters, pq, blob, off, g2, g3, p3, p4)  # (the pointers above outlive this frame through these)
    return calls, keep


def seams(a, rng, fleet, mids):
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    s.load_fleet(fleet)
    s.model_ids_load(mids)
    lib = s.lib
    full = os.sched_getaffinity(0)
    pin = sorted(full)[len(full) // 2]
    big = wl.make_requests(fleet, 0xB16, n=BIG, extra_frac=0.0)[0]
    big["self_pod"], big["flags"] = 1, 0  # one calling instance
    for f, col in (("fresh_lru", "lru_time"), ("fresh_capacity", "capacity"), ("fresh_used", "used"), ("fresh_count", "count"),
                   ("fresh_rpm", "rpm")):
        big[f] = fleet.pods[1][col]
    big_pc, big_pq = _lib.split_caller(big)
    stop = threading.Event()
    n_big = [0]

    def big_batches():
        os.sched_setaffinity(0, full - {pin} or full)  # (this thread only: the caller keeps its CPU to itself)
        while not stop.is_set():
            s.place_c(big_pc, big_pq, None, fleet.now)
            n_big[0] += 1

    sets = {n: seam_calls(s, lib, fleet, mids, rng, n) for n in (1, 256)}
    for case in ("idle", "beside_800k_batches"):
        th = None
        if case != "idle":
            th = threading.Thread(target=big_batches)
            th.start()
        os.sched_setaffinity(0, {pin})
        try:
            for n in (1, 256):
                calls, _ = sets[n]
                iters = a.iters if n == 1 else max(a.iters // 3, 100)
                if case != "idle":  # (the two-call sequence waits for the batch lock: milliseconds per call)
                    iters = max(iters // 10, 100)
                for name, (keyed, two, alone, k_out, t_out) in calls.items():
                    for fn in (keyed, two, alone):  # warm-up: every shape of the timed window
                        for _ in range(200):
                            fn()
                    tk, tt, ta = [], [], []
                    for _ in range(a.rounds):  # alternating blocks
                        block(keyed, iters, tk)
                        block(two, iters, tt)
                        block(alone, iters, ta)
                    equal = all(x.tobytes() == y.tobytes() for x, y in zip(k_out(), t_out()))
                    kp50, kp99 = percentiles(tk)
                    tp50, tp99 = percentiles(tt)
                    ap50, ap99 = percentiles(ta)
                    print(json.dumps({"measure": "seam", "case": case, "call": name, "n": n, "calls_each": len(tk),
                                      "keyed_p50_us": kp50, "keyed_p99_us": kp99, "two_call_p50_us": tp50, "two_call_p99_us": tp99,
                                      "c_call_alone_p50_us": ap50, "c_call_alone_p99_us": ap99,
                                      "outputs_equal": equal, "pinned_cpu": pin, "big_batches_so_far": n_big[0]}), flush=True)
                    assert equal
        finally:
            os.sched_setaffinity(0, full)
            if th:
                stop.set()
                th.join()
    s.close()


def events(a, rng, fleet, pod_ids, mids):
    """mmp_models_events_json on the registry events of one churn slice, by key"""
    M = fleet.n_models
    type_names = ["NLCLASSIFIER"] + ["type-%d" % t for t in range(1, max(fleet.n_types, 1))]
    # the slice and its events, as tools/upsert_time.py draws them
    d = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    d.load_fleet(fleet)
    cs = wl.ChurnStream(fleet, 0xC5)
    sl = cs.next_slice()
    cs.apply(sl, d.place(sl["place_reqs"], sl["extra"], cs.fleet.now))
    idx, rows, ent_pod, ent_time = cs.model_events()
    d.close()
    part = types.SimpleNamespace(models=rows, ent_pod=ent_pod, ent_time=ent_time)
    vals = [v.encode() for v in wire.model_values(part, pod_ids, type_names, rng, np.zeros(len(rows), np.int64))]
    n = len(idx)
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    s.load_pod_ids(pod_ids)
    s.load_type_names(type_names, 0)
    mv = [v.encode() for v in wire.model_values(fleet, pod_ids, type_names, rng, np.zeros(M, np.int64))]
    assert not s.ingest_models_json(mv)[0].any()
    s.model_ids_load(mids)
    fresh_at = rng.choice(n, n // 10, replace=False)
    for what in ("updates only", "a tenth of the keys join"):
        wall = []
        for k in range(1 + a.events_repeats):
            keys = [mids[int(i)] for i in idx]
            if what != "updates only":
                for j, at in enumerate(fresh_at):
                    keys[at] = b"joiner-%d-%d" % (k, j)
            t0 = time.perf_counter()
            st, _, _, n_app = s.models_events_json(keys, vals)
            t1 = time.perf_counter()
            assert not st.any() and n_app == (0 if what == "updates only" else len(fresh_at))
            if k:
                wall.append(1e6 * (t1 - t0))
        print(json.dumps({"measure": "mmp_models_events_json", "label": a.label, "events": n, "batch": what, "calls": len(wall),
                          "wall_us_median": round(float(np.median(wall)), 1), "wall_us_min": round(min(wall), 1),
                          "wall_us_max": round(max(wall), 1)}), flush=True)
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3000)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--events-repeats", type=int, default=5)
    ap.add_argument("--events-only", action="store_true")
    ap.add_argument("--seams-only", action="store_true")
    ap.add_argument("--label", default="this commit")
    a = ap.parse_args()
    rng, fleet, pod_ids, mids = world()
    if not a.events_only:
        seams(a, rng, fleet, mids)
    if not a.seams_only:
        events(a, rng, fleet, pod_ids, mids)


if __name__ == "__main__":
    main()
