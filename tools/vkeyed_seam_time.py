"""Wall time of the request seams by vmodel id (mmp_route_batch_cv / mmp_miss_batch_cv / mmp_place_batch_cv) on C3 (10k pods x
100k models, one defined vmodel per model) beside what a host has without them:

    python tools/vkeyed_seam_time.py [--iters 3000] [--rounds 4]

  two calls   mmp_vmodels_resolve (staged, under the batch lock), the answered rows written into the request rows, then the _c call
  _ck alone   the call by MODEL id on the ids the vmodels name: what a host pays that resolved the vmodel some other way; _cv minus
              that is what resolveVModelId costs inside the call

for one route, one miss and one load target (n = 1) and for 256 routes, (a) on an idle context and (b) while a second thread issues
800 000-row host-pointer mmp_place_batch_c batches back to back (they are staged: the batch lock is held for the whole call).  p50 /
p99 of the call's wall time in microseconds, the calling thread pinned to one CPU; the forms are called through ctypes on arguments
prepared once, in alternating blocks (`rounds` blocks of `iters` calls each), and their outputs are compared.  Every request names
a defined vmodel except one per 256 (an id nobody has seen); nf is empty, as on the first attempt of callModel.

The writer's side — what the copy-on-write rows and the drain behind every swap cost mmp_vmodels_events_json — is measured with
tools/vmodels_time.py on this tree and on its parent commit, two processes each, alternating.

One JSON line per measurement."""
import argparse
import ctypes as C
import json
import os
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))
from keyed_seam_time import BIG, EXPIRY, block, percentiles, world  # noqa: E402
from modelmesh_amd import _lib  # noqa: E402
from modelmesh_amd import workload as wl  # noqa: E402
from modelmesh_amd._lib import ptr  # noqa: E402
from modelmesh_amd.solver import Solver  # noqa: E402


def vid_of(i):
    return b"vmodel-%07d" % i


def seam_calls(s, lib, fleet, mids, rng, n, names):
    """{call: (_cv fn, two-call fn, _ck fn, outputs of the first two)} on arguments prepared once"""
    from seam_caller_time import requests
    c, pc, g, sq, counters, pq = requests(fleet, s, rng, n, 1)
    vkeys = [vid_of(int(m)) for m in g["model"]]
    mkeys = [mids[int(m)] for m in g["model"]]
    if n > 1:
        vkeys[n // 2] = b"a vmodel nobody defined"
        mkeys[n // 2] = b"an id nobody loaded"
    vblob, voff = Solver.pack_keys(vkeys)
    mblob, moff = Solver.pack_keys(mkeys)
    vblob, mblob = np.frombuffer(vblob, np.uint8).copy(), np.frombuffer(mblob, np.uint8).copy()
    now, h, exp, nc = C.c_int64(int(fleet.now)), s.h, C.c_int64(EXPIRY), len(counters)
    cnt = ptr(counters) if nc else None
    ans = np.zeros(n, _lib.VMODEL_ANSWER)
    RES = (h, ptr(vblob), ptr(voff), n, None, None, None, None, None, ptr(ans))

    def bufs(*dts):
        return [np.zeros(n, dt) for dt in dts]

    def rows_of():  # what the two-call host passes on: the row when the class is OK, else -1
        return np.where(ans["cls"] == _lib.VMR_OK, ans["model"], -1)

    calls = {}

    def route():
        vg, vs_, vvm = bufs(_lib.GATE_OUT, _lib.SERVE_OUT, _lib.VSEAM_ROW)
        tg, ts_ = bufs(_lib.GATE_OUT, _lib.SERVE_OUT)
        kg, ks_, kidx = bufs(_lib.GATE_OUT, _lib.SERVE_OUT, np.int32)
        g2 = g.copy()
        V = (h, ptr(c), ptr(g), ptr(sq), n, ptr(vblob), ptr(voff), None, None, None, cnt, nc, None, None, 0, None, 0, now, exp,
             ptr(vg), ptr(vs_), ptr(vvm))
        B = (h, ptr(c), ptr(g2), ptr(sq), n, cnt, nc, None, None, 0, None, 0, now, exp, ptr(tg), ptr(ts_))
        K = (h, ptr(c), ptr(g), ptr(sq), n, ptr(mblob), ptr(moff), cnt, nc, None, None, 0, None, 0, now, exp, ptr(kg), ptr(ks_), ptr(kidx))

        def route_cv():
            assert lib.mmp_route_batch_cv(*V) == 0

        def route_two():
            assert lib.mmp_vmodels_resolve(*RES) == 0
            g2["model"] = rows_of()
            assert lib.mmp_route_batch_c(*B) == 0

        def route_ck():
            assert lib.mmp_route_batch_ck(*K) == 0
        return (route_cv, route_two, route_ck, lambda: (vg, vs_, vvm["model"]), lambda: (tg, ts_, rows_of()), (g2, vg, vs_, vvm, tg, ts_, kg, ks_, kidx))

    def miss():
        vg, vp, vvm = bufs(_lib.GATE_OUT, _lib.PLACE_OUT, _lib.VSEAM_ROW)
        tg, tp = bufs(_lib.GATE_OUT, _lib.PLACE_OUT)
        kg, kp, kidx = bufs(_lib.GATE_OUT, _lib.PLACE_OUT, np.int32)
        g3, p3 = g.copy(), pq.copy()
        V = (h, ptr(c), ptr(pc), ptr(g), ptr(pq), n, ptr(vblob), ptr(voff), None, None, None, None, None, 0, None, 0, None, 0, now, exp,
             ptr(vg), ptr(vp), ptr(vvm))
        B = (h, ptr(c), ptr(pc), ptr(g3), ptr(p3), n, None, None, 0, None, 0, None, 0, now, exp, ptr(tg), ptr(tp))
        K = (h, ptr(c), ptr(pc), ptr(g), ptr(pq), n, ptr(mblob), ptr(moff), None, None, 0, None, 0, None, 0, now, exp, ptr(kg), ptr(kp), ptr(kidx))

        def miss_cv():
            assert lib.mmp_miss_batch_cv(*V) == 0

        def miss_two():
            assert lib.mmp_vmodels_resolve(*RES) == 0
            g3["model"] = p3["model"] = rows_of()
            assert lib.mmp_miss_batch_c(*B) == 0

        def miss_ck():
            assert lib.mmp_miss_batch_ck(*K) == 0
        return (miss_cv, miss_two, miss_ck, lambda: (vg, vp, vvm["model"]), lambda: (tg, tp, rows_of()), (g3, p3, vg, vp, vvm, tg, tp, kg, kp, kidx))

    def place():
        vo, vvm = bufs(_lib.PLACE_OUT, _lib.VSEAM_ROW)
        to, = bufs(_lib.PLACE_OUT)
        ko, kidx = bufs(_lib.PLACE_OUT, np.int32)
        p4 = pq.copy()
        V = (h, ptr(pc), ptr(pq), n, ptr(vblob), ptr(voff), None, None, None, None, 0, now, ptr(vo), ptr(vvm))
        B = (h, ptr(pc), ptr(p4), n, None, 0, now, ptr(to))
        K = (h, ptr(pc), ptr(pq), n, ptr(mblob), ptr(moff), None, 0, now, ptr(ko), ptr(kidx))

        def place_cv():
            assert lib.mmp_place_batch_cv(*V) == 0

        def place_two():
            assert lib.mmp_vmodels_resolve(*RES) == 0
            p4["model"] = rows_of()
            assert lib.mmp_place_batch_c(*B) == 0

        def place_ck():
            assert lib.mmp_place_batch_ck(*K) == 0
        return (place_cv, place_two, place_ck, lambda: (vo, vvm["model"]), lambda: (to, rows_of()), (p4, vo, vvm, to, ko, kidx))
    for name, build in (("route", route), ("miss", miss), ("place", place)):  # (a scope each: the closures keep their own buffers)
        if name in names:
            calls[name] = build()
    keep = (c, pc, g, sq, counters, pq, vblob, voff, mblob, moff, ans)  # (the pointers above outlive this frame through these)
    return calls, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3000)
    ap.add_argument("--rounds", type=int, default=4)
    a = ap.parse_args()
    rng, fleet, _, mids = world()
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    s.load_fleet(fleet)
    s.model_ids_load(mids)
    M = fleet.n_models
    st, _, n_app = s.vmodels_events_json([vid_of(i) for i in range(M)], [b'{"amid":"%s","tmid":"%s"}' % (m, m) for m in mids])
    assert not st.any() and n_app == M
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

    sets = {1: seam_calls(s, lib, fleet, mids, rng, 1, ("route", "miss", "place")), 256: seam_calls(s, lib, fleet, mids, rng, 256, ("route",))}
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
                for name, (cv, two, ck, v_out, t_out, _) in calls.items():
                    for fn in (cv, two, ck):  # warm-up: every shape of the timed window
                        for _ in range(200 if case == "idle" else 20):
                            fn()
                    tv, tt, tc = [], [], []
                    for _ in range(a.rounds):  # alternating blocks
                        block(cv, iters, tv)
                        block(two, iters, tt)
                        block(ck, iters, tc)
                    equal = all(np.asarray(x).tobytes() == np.asarray(y).astype(np.asarray(x).dtype).tobytes() for x, y in zip(v_out(), t_out()))
                    vp50, vp99 = percentiles(tv)
                    tp50, tp99 = percentiles(tt)
                    cp50, cp99 = percentiles(tc)
                    print(json.dumps({"measure": "vseam", "case": case, "call": name, "n": n, "calls_each": len(tv),
                                      "cv_p50_us": vp50, "cv_p99_us": vp99, "two_call_p50_us": tp50, "two_call_p99_us": tp99,
                                      "ck_alone_p50_us": cp50, "ck_alone_p99_us": cp99, "outputs_equal": equal, "pinned_cpu": pin,
                                      "big_batches_so_far": n_big[0]}), flush=True)
                    assert equal
        finally:
            os.sched_setaffinity(0, full)
            if th:
                stop.set()
                th.join()
    s.close()


if __name__ == "__main__":
    main()
