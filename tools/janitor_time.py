"""Call wall and device span of mmp_janitor_plan, beside mmp_registry_prune on the same fleets (mmp_profile / mmp_last_kernel_ms).

    python tools/janitor_time.py [--fleets C3,C4] [--caches 1000,4000,16000] [--repeats 10]

Per fleet (C3: 10k pods x 100k models; C4: 50k pods x 1M models) and cache size one JSON line: the plan's wall time and device
span over `repeats` dry runs (median and the min..max band; dry, so that every repeat sees the same registry), wall and span
of ONE applied plan, and the prune's dry span on the same resident registry — the same-shaped pass over all M models, and the
only existing number this can be set against.  The cache: `n` models on which pod 0 is registered; 80 % of the rows agree with
the registry (they become candidates, ranked), 10 % carry another load timestamp (registered again), 10 % of the models have no
row (deregistered)."""
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

SELF = 0


def measure(fn, s, repeats):
    wall, span = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e6)
        span.append(s.last_kernel_ms() * 1000.0)

    def band(x):
        return dict(median_us=round(float(np.median(x)), 2), min_us=round(min(x), 2), max_us=round(max(x), 2))
    return dict(wall=band(wall), device=band(span))


def cache_for(fleet, n, rng):
    """Registers SELF on n models (in place of their first copy) and returns the cache rows for them, MRU first."""
    now = int(fleet.now)
    has = np.nonzero(fleet.models["n_loaded"] > 0)[0]
    chosen = rng.choice(has, size=min(n, len(has)), replace=False)
    first = fleet.models["ent_off"][chosen]
    fleet.ent_pod[first] = SELF
    fleet.ent_time[first] = now - 5_000_000
    kind = rng.random(len(chosen))
    keep = kind >= 0.1
    e = np.zeros(int(keep.sum()), dtype=_lib.JANITOR_ENTRY)
    e["model"] = chosen[keep]
    e["weight"] = 100
    e["last_used"] = now - 1_000_000 - 3 * rng.permutation(len(e))
    e["load_timestamp"] = fleet.ent_time[first[keep]] + (kind[keep] < 0.2)
    e["last_unload_attempt_time"] = -1
    e["last_heavy_time"] = now - 7_000_000
    e["flags"] = _lib.JE_DONE | _lib.JE_STATE_LIVE
    return e[np.argsort(-e["last_used"], kind="stable")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fleets", default="C3,C4")
    ap.add_argument("--caches", default="1000,4000,16000")
    ap.add_argument("--repeats", type=int, default=10)
    a = ap.parse_args()
    for name in a.fleets.split(","):
        for n in (int(x) for x in a.caches.split(",")):
            fleet = wl.make_fleet(name)
            M, now = fleet.n_models, int(fleet.now)
            # SELF only where the cache puts it.  (A record may then name pod 1 twice: no valid TreeMap image, harmless for timing —
            # nothing here reads pod 1's entries.)
            mine = fleet.ent_pod == SELF
            fleet.ent_pod[mine] = 1
            entries = cache_for(fleet, n, np.random.default_rng(n))
            prm = np.zeros(1, dtype=_lib.JANITOR_PARAMS)
            prm[0] = (SELF, 0, now, 360, 240_000, 6 * 3_600_000, 900_000, 180_000, 600_000, 3_600_000)
            s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
            try:
                s.load_fleet(fleet)
                s.profile(True)
                cap = len(entries) + n
                for _ in range(3):  # warm-up
                    s.janitor_plan(entries, prm, dry=True, max_edits=cap, max_candidates=cap)
                    s.prune_registry(SELF, now, dry=True, max_edits=1024, max_removed=1024)
                holder = {}

                def dry():
                    holder["r"] = s.janitor_plan(entries, prm, dry=True, max_edits=cap, max_candidates=cap)
                plan = measure(dry, s, a.repeats)
                prune = measure(lambda: s.prune_registry(SELF, now, dry=True, max_edits=1024, max_removed=1024), s, a.repeats)
                info = holder["r"][4]
                row = dict(fleet=name, pods=fleet.n_pods, models=M, entries=len(fleet.ent_pod), cache_rows=len(entries), plan=plan,
                           prune=prune, plan_over_prune=round(plan["device"]["median_us"] / prune["device"]["median_us"], 2),
                           n_edits=int(info["n_edits"]), n_candidates=int(info["n_candidates"]), n_ties=int(info["n_ties"]))
                t0 = time.perf_counter()
                s.janitor_plan_raw(entries, prm, _lib.JANITOR_APPLY, cap, cap)  # (the raw form: without the mirror's read-back)
                row["applied_wall_us"] = round((time.perf_counter() - t0) * 1e6, 2)
                row["applied_device_us"] = round(s.last_kernel_ms() * 1000.0, 2)
                print(json.dumps(row), flush=True)
            finally:
                s.close()


if __name__ == "__main__":
    main()
