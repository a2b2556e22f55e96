"""Device span and call wall of mmp_models_status beside the only other way a host has to the same answers: mmp_models_get of
the whole registry plus the vectorised numpy form of the rule (tests/model_status_model.status_closed) on the same box
(mmp_profile / mmp_last_kernel_ms).

    python tools/status_time.py [--cases C3:4096,C3:100000] [--repeats 10]

A case is fleet:n.  The n requests draw models of the fleet uniformly (repeating), -1 for one in fifty; two in five carry a
fail_pod — half of those an instance the record names — and half the MISS flag.  The call is timed with exactly the room it needs
(the sizes come from an untimed call), and its answer is compared with the numpy form's once.  One JSON line per case: medians
over `repeats` calls after 3 warm-up calls, with the min..max band of the device span; the read-back and the numpy form are timed
separately (the read-back moves the whole registry whatever n is)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from modelmesh_amd import _lib  # noqa: E402
from modelmesh_amd import workload as wl  # noqa: E402
from modelmesh_amd.solver import Solver  # noqa: E402
from tests import model_status_model as sm  # noqa: E402


def draw(fleet, n, rng):
    M, P = fleet.n_models, fleet.n_pods
    reqs = np.zeros(n, dtype=_lib.STATUS_REQ)
    reqs["model"] = np.where(rng.random(n) < 0.02, -1, rng.integers(0, M, n))
    m = np.maximum(reqs["model"], 0)
    named = fleet.ent_pod[np.minimum(fleet.models["ent_off"][m], len(fleet.ent_pod) - 1)]
    has = (reqs["model"] >= 0) & (fleet.models["n_loaded"][m] + fleet.models["n_failed"][m] > 0) & (named >= 0) & (named < P)
    fp = np.where(has & (rng.random(n) < 0.5), named, rng.integers(0, P, n))
    reqs["fail_pod"] = np.where(rng.random(n) < 0.4, fp, -1)
    reqs["flags"] = rng.random(n) < 0.5
    return reqs


def med(v):
    return round(float(np.median(v)), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="C3:4096,C3:100000")
    ap.add_argument("--repeats", type=int, default=10)
    a = ap.parse_args()
    cases = {}
    for c in a.cases.split(","):
        name, n = c.split(":")
        cases.setdefault(name, []).append(int(n))
    for name, sizes in cases.items():
        fleet = wl.make_fleet(name)
        now = int(fleet.now)
        s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
        try:
            s.load_fleet(fleet)
            s.profile(True)
            for n in sizes:
                reqs = draw(fleet, n, np.random.default_rng(n))
                total = s.models_status_raw(reqs, now, 0)[2]
                dev, wall, get_wall, np_wall = [], [], [], []
                for k in range(3 + a.repeats):
                    t0 = time.perf_counter()
                    rows, copies, got_total, rc = s.models_status_raw(reqs, now, total)
                    w = (time.perf_counter() - t0) * 1e6
                    d = s.last_kernel_ms() * 1000.0
                    assert rc == 0 and got_total == total
                    t0 = time.perf_counter()
                    models, ep, et = s.get_models()
                    gw = (time.perf_counter() - t0) * 1e6
                    t0 = time.perf_counter()
                    want = sm.status_closed(models, ep, et, fleet.pods["id_order"], reqs, now)
                    nw = (time.perf_counter() - t0) * 1e6
                    if k == 0:
                        sm.assert_same_status((rows, copies), want, f"{name}:{n}")
                    if k >= 3:
                        dev.append(d), wall.append(w), get_wall.append(gw), np_wall.append(nw)
                print(json.dumps(dict(fleet=name, pods=fleet.n_pods, models=fleet.n_models, n=n, copies=total,
                                      status=dict(device_median_us=med(dev), device_min_us=round(min(dev), 1), device_max_us=round(max(dev), 1),
                                                  wall_median_us=med(wall)),
                                      models_get_wall_median_us=med(get_wall), numpy_closed_wall_median_us=med(np_wall),
                                      host_route_over_status_wall=round((med(get_wall) + med(np_wall)) / med(wall), 1))), flush=True)
        finally:
            s.close()


if __name__ == "__main__":
    main()
