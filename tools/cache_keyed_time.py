"""Call wall and device span of mmp_cache_replay_k beside the calls it replaces, and of mmp_models_retire with and without bound
caches.

    python tools/cache_keyed_time.py [--calls 200] [--series 2] [--retire-repeats 20] [--retire-only]

Replay.  n = 1, 256 and 4 096 ops on 64 and 2 000 caches of 16 entries at capacity: every op is a putIfAbsent of an id its cache
does not hold, so every op evicts one entry and the caches keep their size.  Two contexts hold the same state; the two forms
alternate call by call in one process:

    one call     mmp_cache_replay_k (ids in, evicted ids out)
    replaced     mmp_model_ids_resolve, mmp_cache_replay, then mmp_model_ids_get of every victim's row (one call per victim: the
                 rows are scattered, and a host without an id map has no other way back from a row to its id)

Wall is closed by the call's own synchronise (every call returns with its results on the host); the device span is
mmp_last_kernel_ms, summed over the calls of the replaced form that launch kernels (mmp_model_ids_get launches none).  Medians
over `calls` calls after 10 warm-up calls, for each of `series` repeated series.

Retirement.  A registry of 120 000 rows, 1 000 rows retired that no cache names: with bound caches of 100 000 entries (50 x
2 000), with the same caches unbound, and with no caches (the last two take the path the call always took: no new launch).
--retire-only skips the replay series.  State is reloaded before every timed call.  One JSON line per figure."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modelmesh_amd import _lib  # noqa: E402
from modelmesh_amd._lib import ptr  # noqa: E402
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


def replay_series(nc, n, calls, series):
    per = -(-n // nc)
    K = ENTRIES + 2 * per + 2                     # ids per cache: the one inserted was evicted long before it comes round again
    ids = [b"model-%05d-%04d" % (c, k) for c in range(nc) for k in range(K)]
    a, b = context(ids), context(ids)
    seg = np.arange(nc + 1, dtype=np.int32) * ENTRIES
    lu = np.tile(NOW - 1000 + np.arange(ENTRIES), nc).astype(np.int64)
    wt = np.ones(nc * ENTRIES, np.int32)
    rows0 = (np.repeat(np.arange(nc), ENTRIES) * K + np.tile(np.arange(ENTRIES), nc)).astype(np.int32)
    cap = np.full(nc, ENTRIES, np.int64)
    a.load_caches_keyed_k(seg, lu, wt, [ids[r] for r in rows0], cap)
    b.load_caches_keyed(seg, lu, wt, rows0, cap)
    cursor = np.full(nc, ENTRIES, np.int64)
    L = b.lib
    one = np.zeros(1, np.uint8).repeat(64)
    off1 = np.zeros(2, np.int32)
    nb = C.c_int32(0)
    out = []
    for sidx in range(series):
        wa, wb, da, db = [], [], [], []
        for k in range(10 + calls):
            ops = np.zeros(n, dtype=_lib.CACHE_OP)
            ops["cache"] = np.arange(n) % nc
            ops["op"], ops["arg"], ops["time"] = _lib.COP_PUT_IF_ABSENT, 1, NOW + (sidx * (10 + calls) + k) * 10
            rank = np.arange(n) // nc
            which = (cursor[ops["cache"]] + rank) % K
            np.add.at(cursor, ops["cache"], 1)
            keys = [ids[int(c) * K + int(w)] for c, w in zip(ops["cache"], which)]
            blob, koff = Solver.pack_keys(keys)
            t0 = time.perf_counter()
            r = a.cache_replay_k_raw(ops, None, NOW, 32 * n, key_off=koff, blob=blob)
            t1 = time.perf_counter()
            ms_a = a.last_kernel_ms()
            t2 = time.perf_counter()
            rows = b.model_ids_resolve(keys)
            ms1 = b.last_kernel_ms()
            ops["key"] = rows
            outs, ev = b.cache_replay(ops, NOW)
            ms2 = b.last_kernel_ms()
            got = []
            for o in outs:
                for row in ev[o["evicted_off"]: o["evicted_off"] + o["n_evicted"]]:
                    rc = L.mmp_model_ids_get(b.h, int(row), 1, ptr(one), 64, ptr(off1), C.byref(nb))
                    assert rc == 0
                    got.append(one[: nb.value].tobytes())
            t3 = time.perf_counter()
            assert r["need"] <= 32 * n and int(r["outs"]["n_evicted"].sum()) == n == len(got)
            if k == 10:  # the two forms answer alike
                raw = r["id_bytes"].tobytes()
                mine = [raw[r["id_off"][o["evicted_off"]]: r["id_off"][o["evicted_off"] + 1]] for o in r["outs"]]
                assert mine == got and r["outs"].tobytes() == outs.tobytes()
            if k >= 10:
                wa.append(1e6 * (t1 - t0)), wb.append(1e6 * (t3 - t2))
                da.append(1e3 * ms_a), db.append(1e3 * (ms1 + ms2))
        out.append((med(wa), med(da), med(wb), med(db)))
    a.close()
    b.close()
    for form, i in (("mmp_cache_replay_k", 0), ("resolve + mmp_cache_replay + ids_get per victim", 2)):
        print(json.dumps({"what": "replay", "form": form, "caches": nc, "n_ops": n, "calls": calls,
                          "wall_us_by_series": [o[i] for o in out], "device_us_by_series": [o[i + 1] for o in out]}), flush=True)


def retire_series(repeats, keyed):
    M, nc, per = 120_000, 50, 2_000
    ids = [b"model-%06d" % i for i in range(M)]
    rows = np.arange(nc * per, dtype=np.int32)
    seg = np.arange(nc + 1, dtype=np.int32) * per
    lu = (NOW - nc * per + np.arange(nc * per)).astype(np.int64)
    wt = np.ones(nc * per, np.int32)
    cap = np.full(nc, 10**9, np.int64)
    entry_ids = [ids[r] for r in rows]
    retired = np.arange(M - 1_000, M, dtype=np.int32)
    for shape in (("bound caches", "unbound caches", "no caches") if keyed else ("unbound caches", "no caches")):
        wall, dev = [], []
        for k in range(1 + repeats):
            s = context(ids)
            if shape == "bound caches":
                s.load_caches_keyed_k(seg, lu, wt, entry_ids, cap, want_rows=False)
            elif shape == "unbound caches":
                s.load_caches_keyed(seg, lu, wt, rows, cap)
            t0 = time.perf_counter()
            remap = s.models_retire(retired)
            t1 = time.perf_counter()
            ms = s.last_kernel_ms()
            assert s.n_models == M - 1_000 and remap[M - 1] == -1
            s.close()
            if k:
                wall.append(1e6 * (t1 - t0)), dev.append(1e3 * ms)
        print(json.dumps({"what": "retire", "lib": os.path.basename(_lib.LIB_PATH), "shape": shape, "rows": M, "retired": 1_000,
                          "cache_entries": 0 if shape == "no caches" else nc * per, "repeats": repeats, "wall_us": med(wall),
                          "device_us": med(dev), "wall_us_min_max": [round(min(wall), 1), round(max(wall), 1)]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--series", type=int, default=2)
    ap.add_argument("--retire-repeats", type=int, default=20)
    ap.add_argument("--retire-only", action="store_true")
    a = ap.parse_args()
    if not a.retire_only:
        for nc in (64, 2000):
            for n in (1, 256, 4096):
                replay_series(nc, n, a.calls, a.series)
    retire_series(a.retire_repeats, keyed=not a.retire_only)


if __name__ == "__main__":
    main()
