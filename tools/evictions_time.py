"""Call wall and device span of the two calls of the eviction loop by id beside the calls they stand next to.

    python tools/evictions_time.py [--calls 200] [--processes 2]

Replay.  mmp_cache_replay_kt against mmp_cache_replay_k on the same streams: n = 1, 256 and 4 096 ops on 64 caches of 16 entries at
capacity, every op a putIfAbsent of an id its cache does not hold, so every op evicts one entry (the shape of
tools/cache_keyed_time.py).  Two contexts hold the same state and the two forms alternate call by call.

Evictions.  mmp_evictions_k against mmp_gate_batch + mmp_registry_ops_k at n = 1, 64 and 4 096 victims on a registry of 8 192
records with 4 copies each, one of them this instance's (flags 0: computed, nothing applied, so every call sees the same state).
The replaced form gets loaded_time from the host — which the host of a binding without an id map does not have; it is timed as the
floor of what the one call replaces.

Wall is closed by the call's own synchronise; the device span is mmp_last_kernel_ms (summed over the calls of a form that launch
kernels).  Medians over `calls` calls after 10 warm-up calls.  The whole series runs in `processes` fresh child processes one after
the other: the spread of one form's median between them is the run-to-run band the other form is read against.  One JSON line per
figure and process, then one line per comparison."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modelmesh_amd import _lib  # noqa: E402
from modelmesh_amd import workload as wl  # noqa: E402
from modelmesh_amd.solver import Solver  # noqa: E402

NOW = 1_760_000_000_000
ENTRIES = 16


def med(xs):
    return round(float(np.median(xs)), 1)


def context(ids):
    s = Solver(100, 1000)
    s.profile(True)
    s.load_pod_ids(["aaaaaa-1"])
    rows = np.zeros(len(ids), _lib.MODEL_ROW)
    rows["last_used"] = 1
    s.load_models(rows, np.zeros(0, np.int32), np.zeros(0, np.int64))
    s.model_ids_load(ids)
    return s


def replay_series(nc, n, calls):
    per = -(-n // nc)
    K = ENTRIES + 2 * per + 2
    ids = [b"model-%05d-%04d" % (c, k) for c in range(nc) for k in range(K)]
    a, b = context(ids), context(ids)
    seg = np.arange(nc + 1, dtype=np.int32) * ENTRIES
    lu = np.tile(NOW - 1000 + np.arange(ENTRIES), nc).astype(np.int64)
    wt = np.ones(nc * ENTRIES, np.int32)
    rows0 = (np.repeat(np.arange(nc), ENTRIES) * K + np.tile(np.arange(ENTRIES), nc)).astype(np.int32)
    cap = np.full(nc, ENTRIES, np.int64)
    for s in (a, b):
        s.load_caches_keyed_k(seg, lu, wt, [ids[r] for r in rows0], cap)
    cursor = np.full(nc, ENTRIES, np.int64)
    w, d = {"kt": [], "k": []}, {"kt": [], "k": []}
    for k in range(10 + calls):
        ops = np.zeros(n, dtype=_lib.CACHE_OP)
        ops["cache"] = np.arange(n) % nc
        ops["op"], ops["arg"], ops["time"] = _lib.COP_PUT_IF_ABSENT, 1, NOW + k * 10
        which = (cursor[ops["cache"]] + np.arange(n) // nc) % K
        np.add.at(cursor, ops["cache"], 1)
        blob, koff = Solver.pack_keys([ids[int(c) * K + int(x)] for c, x in zip(ops["cache"], which)])
        res = {}
        for form, s, times in ((("kt", a, "out"), ("k", b, None)) if k % 2 else (("k", b, None), ("kt", a, "out"))):
            t0 = time.perf_counter()
            res[form] = s.cache_replay_k_raw(ops, None, NOW, 32 * n, key_off=koff, blob=blob, times=times)
            t1 = time.perf_counter()
            if k >= 10:
                w[form].append(1e6 * (t1 - t0)), d[form].append(1e3 * s.last_kernel_ms())
        if k == 10:  # the two forms answer alike, and the times are the victims'
            assert all(res["kt"][f].tobytes() == res["k"][f].tobytes() for f in ("outs", "evicted_rows", "id_off", "id_bytes"))
            assert int((res["kt"]["last_used"] != 0).sum()) == n
    a.close()
    b.close()
    for form, name in (("kt", "mmp_cache_replay_kt"), ("k", "mmp_cache_replay_k")):
        print(json.dumps({"what": "replay", "form": name, "pid": os.getpid(), "caches": nc, "n": n, "calls": calls, "wall_us": med(w[form]),
                          "device_us": med(d[form])}), flush=True)


def evictions_series(n, calls):
    M, P, me = 8192, 8, 3
    fleet = wl.fuzz_fleet(5, pods=P, models=16)
    ids = [b"model-%05d" % i for i in range(M)]
    models = np.zeros(M, _lib.MODEL_ROW)
    models["ent_off"], models["n_loaded"], models["last_used"] = 4 * np.arange(M), 4, 5
    order = [int(p) for p in np.argsort(fleet.pods["id_order"])]
    four = sorted([me] + [p for p in order if p != me][:3], key=order.index)
    fleet.models, fleet.ent_pod = models, np.tile(np.array(four, np.int32), M)
    fleet.ent_time = (NOW - 10_000_000 + np.arange(4 * M)).astype(np.int64)
    a, b = (Solver(fleet.min_space_units, fleet.min_churn_age_ms) for _ in range(2))
    for s in (a, b):
        s.profile(True)
        s.load_fleet(fleet)
        s.model_ids_load(ids)
    now = int(fleet.now)
    rng = np.random.default_rng(n)
    w, d = {"one": [], "two": []}, {"one": [], "two": []}
    for k in range(10 + calls):
        rows = rng.permutation(M)[:n]
        keys = [ids[r] for r in rows]
        loaded = fleet.ent_time[4 * rows + four.index(me)]
        entries = np.zeros(n, dtype=_lib.EVICTED_ENTRY)
        entries["last_used"], entries["load_time"], entries["weight"] = now - 5, loaded, 10
        ops = np.zeros(n, dtype=_lib.REGISTRY_OP)
        ops["pod"], ops["op"], ops["flags"] = me, _lib.ROP_DEREGISTER, _lib.ROPF_MATCH_TIME
        ops["last_used"], ops["load_time"] = now - 5, loaded
        reqs = np.zeros(n, dtype=_lib.GATE_REQ)
        reqs["model"], reqs["self_pod"], reqs["loaded_time"], reqs["load_timeout_ms"] = rows, me, loaded, 1000
        t0 = time.perf_counter()
        one = a.evictions_k_raw(entries, keys, me, now, 1000, 0, n)
        t1 = time.perf_counter()
        ms_one = a.last_kernel_ms()
        t2 = time.perf_counter()
        bits = b.gates(reqs, [], [], [], now)["bits"]
        ms1 = b.last_kernel_ms()
        two = b.registry_ops_k_raw(ops, keys, now, 0, n)
        t3 = time.perf_counter()
        ms2 = b.last_kernel_ms()
        assert one[5] == 0 and two[4] == 0
        if k == 10:
            assert one[3].tobytes() == two[2].tobytes() and len(one[3]) == n
            assert [bool(x & _lib.GATE_RELOAD_ELSEWHERE) for x in bits] == [bool(x & _lib.EVO_RELOAD) for x in one[1]["flags"]]
        if k >= 10:
            w["one"].append(1e6 * (t1 - t0)), w["two"].append(1e6 * (t3 - t2))
            d["one"].append(1e3 * ms_one), d["two"].append(1e3 * (max(ms1, 0) + ms2))
    a.close()
    b.close()
    for form, name in (("one", "mmp_evictions_k"), ("two", "mmp_gate_batch + mmp_registry_ops_k")):
        print(json.dumps({"what": "evictions", "form": name, "pid": os.getpid(), "n": n, "calls": calls, "wall_us": med(w[form]),
                          "device_us": med(d[form])}), flush=True)


def child(calls):
    for n in (1, 256, 4096):
        replay_series(64, n, calls)
    for n in (1, 64, 4096):
        evictions_series(n, calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--processes", type=int, default=2)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.calls)
    rows = []
    for _ in range(a.processes):  # one after the other: each a fresh process with a context of its own
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(a.calls)], capture_output=True, text=True,
                             check=True).stdout
        sys.stdout.write(out)
        rows += [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]
    pairs = {"replay": ("mmp_cache_replay_kt", "mmp_cache_replay_k"), "evictions": ("mmp_evictions_k", "mmp_gate_batch + mmp_registry_ops_k")}
    for what, (new, old) in pairs.items():
        for n in sorted({r["n"] for r in rows if r["what"] == what}):
            for metric in ("device_us", "wall_us"):
                o = [r[metric] for r in rows if r["what"] == what and r["n"] == n and r["form"] == old]
                v = [r[metric] for r in rows if r["what"] == what and r["n"] == n and r["form"] == new]
                band = round(max(o) - min(o), 1)
                added = round(float(np.median(v) - np.median(o)), 1)
                print(json.dumps({"what": what + " compared", "n": n, "metric": metric, "new": v, "old": o, "old_band": band, "added": added,
                                  "within_band": bool(added <= band)}), flush=True)


if __name__ == "__main__":
    main()
