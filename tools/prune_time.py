"""Device span of mmp_registry_prune against mmp_proactive_plan on the same fleets (mmp_profile / mmp_last_kernel_ms).

    python tools/prune_time.py [--fleets C3,C4] [--repeats 10]

Per fleet (C3: 10k pods x 100k models; C4: 50k pods x 1M models) and per state of the instance table — nothing missing, 1 %
of the pods at first sighting, 1 % of the pods due — one JSON line: the plan's span over `repeats` runs (median and the
min..max band), the prune's (dry runs, so that every repeat sees the same state), the span of ONE applied prune where there is
something to apply, and the byte ratio (the plan streams the 24-byte model rows once; the prune reads 12 bytes per entry more)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modelmesh_amd import workload as wl  # noqa: E402
from modelmesh_amd.solver import Solver  # noqa: E402

GONE = 600_000


def spans(fn, s, repeats):
    out = []
    for _ in range(repeats):
        fn()
        out.append(s.last_kernel_ms() * 1000.0)
    return dict(median_us=round(float(np.median(out)), 2), min_us=round(min(out), 2), max_us=round(max(out), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fleets", default="C3,C4")
    ap.add_argument("--repeats", type=int, default=10)
    a = ap.parse_args()
    for name in a.fleets.split(","):
        fleet = wl.make_fleet(name)
        now, P, M = fleet.now, fleet.n_pods, fleet.n_models
        n_ent = len(fleet.ent_pod)
        ratio = (24 * M + 12 * n_ent) / (24 * M)
        gone = np.random.default_rng(1).choice(P, size=P // 100, replace=False).astype(np.int32)
        for state in ("nothing_missing", "first_sighting", "due"):
            s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
            try:
                s.load_fleet(fleet)
                s.profile(True)
                if state != "nothing_missing":
                    s.remove_pods(gone)
                    s.commit()
                if state == "due":
                    s.prune_registry(0, now - GONE - 1, apply=False)  # the marks, older than gone-after at `now`
                for _ in range(3):  # warm-up
                    s.proactive_plan(6400, now, 1024)
                    s.prune_registry(0, now, dry=True, max_edits=M, max_removed=n_ent)
                plan = spans(lambda: s.proactive_plan(6400, now, 1024), s, a.repeats)
                holder = {}

                def dry():
                    holder["r"] = s.prune_registry(0, now, dry=True, max_edits=M, max_removed=n_ent)
                prune = spans(dry, s, a.repeats)
                info = holder["r"][2]
                row = dict(fleet=name, pods=P, models=M, entries=n_ent, state=state, plan=plan, prune_scan=prune,
                           byte_ratio=round(ratio, 3), scan_over_plan=round(prune["median_us"] / plan["median_us"], 3),
                           n_edits=int(info["n_edits"]), n_removed=int(info["n_removed"]), n_new_missing=int(info["n_new_missing"]))
                s.prune_registry(0, now, apply=True, max_edits=M, max_removed=n_ent)
                row["prune_applied_us"] = round(s.last_kernel_ms() * 1000.0, 2)
                print(json.dumps(row), flush=True)
            finally:
                s.close()


if __name__ == "__main__":
    main()
