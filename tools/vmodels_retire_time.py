"""Device span and call wall of mmp_vmodels_retire on a C3-sized vmodel table (20 000 vmodels over the ids of 100 000 models) with
a tenth and half of the rows retired, beside the only other route to the same state, measured in the same run:

    mmp_vmodels_retire of the rows    beside    a fresh context that takes the survivors as one mmp_vmodels_events_json batch

    python tools/vmodels_retire_time.py [--repeats 5]

The retired rows are drawn at random and deleted first, as the listener would have (the retire runs with ABSENT_ONLY); before every
timed retire the table is emptied and the whole batch sent again (not timed), so every repeat compacts the same state.  The rebuild
route is timed at the C boundary with the survivors' ids and values already packed — the host work of holding and packing them,
which the retire takes away, is not in its wall — on a context created (not timed) for that repeat.  Neither route reads the
registry: the table is loaded without one.

One JSON line per route and share: medians over `repeats` calls after 1 warm-up call, device span (mmp_profile /
mmp_last_kernel_ms) and wall time of the call, both in microseconds."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modelmesh_amd import _lib  # noqa: E402
from modelmesh_amd import workload as wl  # noqa: E402
from modelmesh_amd._lib import ptr  # noqa: E402
from modelmesh_amd.solver import Solver  # noqa: E402
from tests import vmodel_model as vm  # noqa: E402


def median_us(xs):
    return round(float(np.median(xs)), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--vmodels", type=int, default=20000)
    a = ap.parse_args()
    rng = np.random.default_rng(0xC3)
    fleet = wl.make_fleet("C3")
    M, V = fleet.n_models, a.vmodels
    mids = [b"model-%07d-%05x" % (i, int(x)) for i, x in enumerate(rng.integers(0, 16**5, M))]
    vids = [b"vmodel-%06d-%04x" % (i, int(x)) for i, x in enumerate(rng.integers(0, 16**4, V))]
    active = rng.integers(0, M, V)
    target = np.where(rng.random(V) < 0.1, rng.integers(0, M, V), active)  # a tenth in transition
    values = [vm.render(mids[active[v]].decode(), mids[target[v]].decode(), "owner-%d" % (v % 97), failed=bool(v % 31 == 0)).encode()
              for v in range(V)]

    def context():
        c = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
        c.profile(True)
        return c

    s = context()
    L = s.lib
    for share in (0.10, 0.50):
        rows = np.sort(rng.choice(V, int(V * share), replace=False)).astype(np.int32)
        keep = np.ones(V, bool)
        keep[rows] = False
        kept = np.nonzero(keep)[0]
        kblob, koff = Solver._pack([vids[i] for i in kept])
        blob, off = Solver._pack([values[i] for i in kept])
        koff32, n_keep = koff.astype(np.int32), len(kept)
        idx, status, n_app = np.zeros(n_keep, np.int32), np.zeros(n_keep, np.int32), _lib.C.c_int32(0)
        span, wall, rspan, rwall = [], [], [], []
        for k in range(1 + a.repeats):
            s.vmodels_retire(np.arange(int(s.vmodels_info()["n_rows"]), dtype=np.int32))  # (empties the table)
            st, _, n = s.vmodels_events_json(vids, values)
            assert not st.any() and n == V
            st, _, _ = s.vmodels_events_json([vids[i] for i in rows], [b""] * len(rows), np.ones(len(rows), np.uint8))
            assert not st.any()
            t0 = time.perf_counter()
            remap, n_after = s.vmodels_retire(rows, absent_only=True)
            t1 = time.perf_counter()
            ms = s.last_kernel_ms()
            assert n_after == n_keep and int((remap >= 0).sum()) == n_keep
            t = context()
            t2 = time.perf_counter()
            rc = L.mmp_vmodels_events_json(t.h, kblob, ptr(koff32), blob, ptr(off), n_keep, None, _lib.VMEV_APPEND, ptr(idx), ptr(status),
                                           _lib.C.byref(n_app))
            t3 = time.perf_counter()
            rms = t.last_kernel_ms()
            assert rc == 0 and not status.any() and n_app.value == n_keep
            if k == a.repeats:  # both routes end in the same table
                assert s.vmodels_get()[0] == t.vmodels_get()[0] and s.vmodels_get()[2] == t.vmodels_get()[2]
                assert s.vmodels_info().tobytes() == t.vmodels_info().tobytes()
            t.close()
            if k:
                span.append(1e3 * ms if ms >= 0 else -1.0)
                wall.append(1e6 * (t1 - t0))
                rspan.append(1e3 * rms if rms >= 0 else -1.0)
                rwall.append(1e6 * (t3 - t2))
        for route, sp, wa in (("mmp_vmodels_retire", span, wall), ("fresh context + mmp_vmodels_events_json", rspan, rwall)):
            print(json.dumps({"route": route, "fleet": "C3", "vmodels": V, "retired": len(rows), "device_us": median_us(sp),
                              "wall_us": median_us(wa)}), flush=True)
    s.close()


if __name__ == "__main__":
    main()
