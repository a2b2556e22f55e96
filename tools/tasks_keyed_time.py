#!/usr/bin/env python
"""Wall and device time of the periodic tasks by id (mmp_scaleup_plan_k, mmp_scaledown_plan_k, mmp_migration_plan_k,
mmp_janitor_plan_k without and with its scale-down) against the calls each replaces (mmp_model_ids_resolve + the by-row call; for
the janitor with its scale-down, + mmp_scaledown_plan on the candidates), at n = 1, 256 and 4096 entries on C3, idle and beside a
thread that issues 800 000-row place batches on the same context (what the calls queue behind on the batch lock).

usage: tools/tasks_keyed_time.py [--parent-lib PATH] [--reps R] [--out FILE.jsonl]
The replaced calls run in processes of their own against --parent-lib (a libmmplace.so built from the parent commit; default: this
tree's library, whose by-row calls compute the same), the new calls against this tree's library: two processes each, alternating.
One jsonl row per (process, call, n, contended): p50 and p99 wall in us, median device span in us (mmp_last_kernel_ms, summed over
the calls of a sequence), and for the janitor n_candidates and n_edits of the last call.

The world at size n: C3 with instance SELF's registrations taken out and put back on exactly n models that have three copies, and
the n cache entries are those models — old, live, done, their loadTimestamp the registry's, distinct lastUsed times.  So the cache
is the whole cache of the instance (an applied run finds no lost copy to deregister and edits nothing: every repetition does the
same work) and EVERY entry is a scale-down candidate: the chained form runs its gather / decide / budget kernels on n candidates,
and the replaced sequence makes its third call on n rows.  The janitor alone runs with flags 0, the chained form with
MMP_JANITOR_APPLY.  Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NS = (1, 256, 4096)
NEW = ("mmp_scaleup_plan_k", "mmp_scaledown_plan_k", "mmp_migration_plan_k", "mmp_janitor_plan_k")
BIG = 800_000
SELF = 3


def world(n_self):
    import numpy as np

    from modelmesh_amd import _lib
    from modelmesh_amd import workload as wl
    from modelmesh_amd.solver import Solver
    fleet = wl.make_fleet("C3")
    now = int(fleet.now)
    m, ep, et, io = fleet.models, fleet.ent_pod, fleet.ent_time, fleet.pods["id_order"]

    def resort(row):                                    # instanceIds is in id order
        o, nl = int(m["ent_off"][row]), int(m["n_loaded"][row])
        order = np.argsort(io[ep[o:o + nl]], kind="stable")
        ep[o:o + nl], et[o:o + nl] = ep[o:o + nl][order], et[o:o + nl][order]

    for x in np.nonzero(ep == SELF)[0]:                 # SELF's own registrations go to a neighbour the record does not name
        row = int(np.searchsorted(m["ent_off"], x, side="right")) - 1
        o, k = int(m["ent_off"][row]), int(m["n_loaded"][row] + m["n_failed"][row])
        ep[x] = next(q for q in range(SELF + 1, fleet.n_pods) if q not in ep[o:o + k])
        resort(row)
    three = np.nonzero((m["n_loaded"] == 3) & (m["n_failed"] == 0))[0]
    held = np.random.default_rng(17).permutation(three)[:n_self]
    assert len(held) == n_self
    for r, row in enumerate(held):                      # ... and come back on n_self models with two other, old copies
        o = int(m["ent_off"][row])
        ep[o], et[o:o + 3] = SELF, (now - 40_000_000 - r, now - 50_000_000, now - 60_000_000)
        m["last_used"][row] = now - 3_000_000
        resort(row)
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    s.load_fleet(fleet)
    ids = [b"model-%06d" % i for i in range(fleet.n_models)]
    s.model_ids_load(ids)
    load_time = {int(row): now - 40_000_000 - r for r, row in enumerate(held)}
    return s, _lib, np, fleet, ids, held, load_time


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def worker(mode, reps):
    from modelmesh_amd import _lib
    if mode == "compose":
        _lib.SYMBOLS = [x for x in _lib.SYMBOLS if x[0] not in NEW]
    new = mode == "new"
    for n in NS:
        at_size(mode, new, n, reps)


def at_size(mode, new, n, reps):
    s, _lib, np, fleet, ids, held, load_time = world(n)
    s.lib.mmp_profile(s.h, 1)
    span = lambda: s.lib.mmp_last_kernel_ms(s.h)  # noqa: E731
    now = int(fleet.now)
    last = {}                                          # the janitor's n_candidates / n_edits of the last call

    sp = np.zeros(1, _lib.SCALEUP_PARAMS)
    sp["self_pod"], sp["iteration_counter"], sp["second_copy_max_age_iters"], sp["second_copy_min_age_iters"] = SELF, 130, 240, 42
    sp["scale_up_rpm_threshold"], sp["our_rpm"], sp["now"], sp["last_check_time"], sp["rate_check_interval_ms"] = 2000, 100, now, now - 10_000, 10_000
    sp["second_copy_lru_threshold_ms"], sp["assume_completed_ms"] = 72_000_000, 30_000
    dp = np.zeros(1, _lib.SCALEDOWN_PARAMS)
    dp["self_pod"], dp["now"], dp["last_check_time"], dp["rate_check_interval_ms"] = SELF, now, now - 7_000, 10_000
    dp["adjusted_cache_capacity"], dp["scale_up_rpm_threshold"] = 10_000_000, 2000
    jp = np.zeros(1, _lib.JANITOR_PARAMS)
    jp[0] = (SELF, 0, now, 360, 240_000, 6 * 3_600_000, 900_000, 180_000, 600_000, 3_600_000)

    def resolved(e, keys):
        e = e.copy()
        e["model"] = s.model_ids_resolve(keys)
        return e, span()

    def scaleup(e, j, keys):
        if new:
            assert s.scaleup_plan_k_raw(e, keys, sp)[-1] == 0
            return span()
        e, d = resolved(e, keys)
        s.scaleup_plan(e, sp)
        return d + span()

    def scaledown(e, j, keys):
        if new:
            assert s.scaledown_plan_k_raw(e, keys, dp)[-1] == 0
            return span()
        e, d = resolved(e, keys)
        s.scaledown_plan(e, dp)
        return d + span()

    def migration(e, j, keys):
        if new:
            assert s.migration_plan_k_raw(e, keys, SELF, now)[-1] == 0
            return span()
        e, d = resolved(e, keys)
        s.migration_plan(e, SELF, now)
        return d + span()

    def janitor(e, j, keys):
        if new:
            out = s.janitor_plan_k_raw(j, keys, jp, 0, len(j), len(j))
            assert out[-1] == 0
            last["info"] = out[6]
            return span()
        j, d = resolved(j, keys)
        last["info"] = s.janitor_plan_raw(j, jp, 0, len(j), len(j))[4]
        return d + span()

    def janitor_chain(e, j, keys):
        if new:
            out = s.janitor_plan_k_raw(j, keys, jp, _lib.JANITOR_APPLY, len(j), len(j), dp)
            assert out[-1] == 0
            last["info"] = out[6]
            return span()
        j, d = resolved(j, keys)
        out = s.janitor_plan_raw(j, jp, _lib.JANITOR_APPLY, len(j), len(j))
        last["info"] = out[4]
        d += span()
        s.scaledown_plan(out[2], dp)                    # the candidates it returned: n of them
        return d + span()

    calls = (("scaleup", scaleup), ("scaledown", scaledown), ("migration", migration), ("janitor", janitor), ("janitor+scaledown", janitor_chain))
    keys = [ids[int(r)] for r in held]
    e = np.zeros(n, _lib.CACHE_ENTRY)                   # (model: by key it is ignored, by row the resolve fills it in)
    e["weight"], e["last_used"], e["interval_count"] = 100, now - 5_000_000 - np.arange(n), 3
    j = np.zeros(n, _lib.JANITOR_ENTRY)                 # old, live, done, in order with the registry: every entry a candidate
    j["weight"], j["last_used"], j["last_unload_attempt_time"], j["flags"] = 100, now - 2_000_000 - 10 * np.arange(n), -1, _lib.JE_DONE | _lib.JE_STATE_LIVE
    j["load_timestamp"], j["last_heavy_time"] = [load_time[int(r)] for r in held], now - 30_000_000

    def series(name, fn, reps, contended):
        last.clear()
        for _ in range(4):                              # warm-up: buffers grown, code resident
            fn(e, j, keys)
        wall, dev = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            d = fn(e, j, keys)
            wall.append((time.perf_counter() - t0) * 1e6)
            dev.append(d * 1e3)
        info = last.get("info")
        if info is not None:                            # what the series is FOR: every entry a candidate, nothing to edit
            assert int(info["n_candidates"]) == n and int(info["n_edits"]) == 0, (name, n, info)
        print(json.dumps({"mode": mode, "call": name + ("_k" if new else " (resolve + by row)"), "n": n, "contended": contended, "reps": reps,
                          "wall_p50_us": round(pct(wall, 0.5), 1), "wall_p99_us": round(pct(wall, 0.99), 1),
                          "device_us": round(statistics.median(dev), 1),
                          "n_candidates": None if info is None else int(info["n_candidates"]),
                          "n_edits": None if info is None else int(info["n_edits"]), "pid": os.getpid()}), flush=True)

    for name, fn in calls:
        series(name, fn, reps, False)
    # beside 800 000-row batches: every call of either form queues behind the batch that holds the lock
    from modelmesh_amd import workload as wl
    reqs, extra = wl.make_requests(fleet, 7, BIG)
    stop = threading.Event()

    def batches():
        while not stop.is_set():
            s.place(reqs, extra, fleet.now)
    s.place(reqs, extra, fleet.now)
    t = threading.Thread(target=batches)
    t.start()
    try:
        for name, fn in calls:
            series(name, fn, reps, True)
    finally:
        stop.set()
        t.join()
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker")
    ap.add_argument("--parent-lib")
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.reps)
    lines = []
    for _ in range(2):  # two processes each, alternating
        for mode in ("new", "compose"):
            env = dict(os.environ)
            if mode == "compose" and a.parent_lib:
                env["MMP_LIB_PATH"] = os.path.abspath(a.parent_lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", mode, "--reps", str(a.reps)], env=env, text=True,
                               stdout=subprocess.PIPE, check=True, timeout=280)
            sys.stdout.write(p.stdout)
            sys.stdout.flush()
            lines.append(p.stdout)
    if a.out:
        with open(a.out, "w") as f:
            f.write("".join(lines))


if __name__ == "__main__":
    main()
