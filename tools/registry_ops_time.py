"""Device span and call wall of an applied mmp_registry_ops beside the route it replaces, mmp_models_upsert of the same edited
records, and beside one mmp_registry_prune pass over the same registry (mmp_profile / mmp_last_kernel_ms).

    python tools/registry_ops_time.py [--cases C3:1,C3:8,C3:64,C3:2000,ONE:2000,C4:8] [--repeats 10]

A case is fleet:n.  C3: 10k pods x 100k models; C4: 50k pods x 1M models; ONE: 2 000 models that all stand on one instance of 8.
The n ops name n distinct models and the instance of each model's first copy; calls alternate between DEREGISTER (the copy
goes) and REGISTER (it is put back), so every op of every call edits its record.  After each applied call the n records are read
back (untimed) and sent through mmp_models_upsert, timed alone: the host-side rebuild of the records is not counted against it.
One JSON line per case: medians over `repeats` calls after 3 or 4 warm-up calls (an even number of calls in all, so that a case
leaves the registry as it found it), with the min..max band of the device span."""
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


def one_instance_fleet():
    """8 instances, 2 000 models, every model with a copy on instance 3 (the shape preShutdown meets)."""
    fleet = wl.fuzz_fleet(1320, pods=8, models=2000)
    M = fleet.n_models
    others = np.where(np.arange(M) % 2 == 0, 1, 5).astype(np.int32)
    fleet.models["ent_off"], fleet.models["n_loaded"], fleet.models["n_failed"] = 2 * np.arange(M), 2, 0
    order = fleet.pods["id_order"]
    pair = np.stack([np.full(M, 3, np.int32), others], axis=1)
    swap = order[pair[:, 0]] > order[pair[:, 1]]  # entries stand in id order
    pair[swap] = pair[swap][:, ::-1]
    fleet.ent_pod = pair.reshape(-1).astype(np.int32)
    fleet.ent_time = (fleet.now - 10_000 - np.arange(2 * M)).astype(np.int64)
    return fleet


def stats(dev, wall):
    return dict(median_us=round(float(np.median(dev)), 2), min_us=round(min(dev), 2), max_us=round(max(dev), 2),
                wall_median_us=round(float(np.median(wall)), 1))


def records_of(s, models):
    """(rows with offsets from 0, ent_pod, ent_time) of these models as the device holds them."""
    rows, ep, et = s.get_models()
    sub = rows[models].copy()
    n = sub["n_loaded"] + sub["n_failed"]
    idx = np.concatenate([np.arange(o, o + k) for o, k in zip(sub["ent_off"], n)]) if len(sub) else np.zeros(0, np.int64)
    sub["ent_off"] = np.cumsum(n) - n
    return sub, ep[idx].copy(), et[idx].copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="C3:1,C3:8,C3:64,C3:2000,ONE:2000,C4:8")
    ap.add_argument("--repeats", type=int, default=10)
    a = ap.parse_args()
    cases = {}
    for c in a.cases.split(","):
        name, n = c.split(":")
        cases.setdefault(name, []).append(int(n))
    for name, sizes in cases.items():
        fleet = one_instance_fleet() if name == "ONE" else wl.make_fleet(name)
        now, P, M = int(fleet.now), fleet.n_pods, fleet.n_models
        s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
        try:
            s.load_fleet(fleet)
            s.profile(True)
            with_copy = np.nonzero(fleet.models["n_loaded"] > 0)[0]
            for _ in range(3):
                s.prune_registry(0, now, dry=True, max_edits=M, max_removed=len(fleet.ent_pod))
            pdev, pwall = [], []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                s.prune_registry(0, now, dry=True, max_edits=M, max_removed=len(fleet.ent_pod))
                pwall.append((time.perf_counter() - t0) * 1e6)
                pdev.append(s.last_kernel_ms() * 1000.0)
            for n in sizes:
                models = with_copy[np.linspace(0, len(with_copy) - 1, n).astype(np.int64)].astype(np.int32)
                assert len(set(models.tolist())) == n
                ops = np.zeros(n, dtype=_lib.REGISTRY_OP)
                ops["model"] = models
                ops["pod"] = fleet.ent_pod[fleet.models["ent_off"][models]]
                ops["load_time"] = fleet.ent_time[fleet.models["ent_off"][models]]
                odev, owall, udev, uwall = [], [], [], []
                warm = 3 + (3 + a.repeats) % 2
                for k in range(warm + a.repeats):
                    ops["op"] = _lib.ROP_DEREGISTER if k % 2 == 0 else _lib.ROP_REGISTER
                    t0 = time.perf_counter()
                    _, ed, info = s.registry_ops_raw(ops, now + k, _lib.ROPS_APPLY, n, want_status=False)
                    w = (time.perf_counter() - t0) * 1e6
                    d = s.last_kernel_ms() * 1000.0
                    assert int(info["n_edits"]) == n and not int(info["truncated"])
                    rows, ep, et = records_of(s, models)
                    t0 = time.perf_counter()
                    s.upsert_models(models, rows, ep, et)
                    uw = (time.perf_counter() - t0) * 1e6
                    ud = s.last_kernel_ms() * 1000.0
                    if k >= warm:
                        odev.append(d), owall.append(w), udev.append(ud), uwall.append(uw)
                ro, up = stats(odev, owall), stats(udev, uwall)
                print(json.dumps(dict(fleet=name, pods=P, models=M, n=n, ops_applied=ro, upsert_same_records=up,
                                      prune_scan=stats(pdev, pwall), wall_ops_over_upsert=round(ro["wall_median_us"] / up["wall_median_us"], 3))),
                      flush=True)
        finally:
            s.close()


if __name__ == "__main__":
    main()
