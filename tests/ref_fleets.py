"""Fleets and requests of the reference-text vectors (tests/golden/ref_getnext.npz, ref_gate_edges.npz, ref_place_edges.npz,
ref_rebalance_edges.npz): built here, deterministically from
seeds, so that the generator (oracle/ref_harness/make_ref_vectors.py — needs /root/reference) and the tests that consume
the committed vectors (CPU: the oracle; GPU: the HIP path) construct byte-identical inputs.  A digest of the inputs is stored
with the vectors and checked by the tests.

The harness runs the reference's own Java text, which orders instances by their id STRINGS (String.compareTo, MM.java:4696)
and derives the replica set from id.substring(0, 6) (MM.java:4770).  The fuzz fleets of modelmesh_amd.workload draw
`id_order` and `replica_set` independently, which no set of strings can realise — so every fleet here first gets real ids
("%06x-..." prefixes per replica set, short ids for instances without one) and `id_order` := the rank of its id, and
the registry entries (instanceIds / loadFailedInstanceIds iterate in id order) are re-sorted accordingly."""
from __future__ import annotations

import functools
import hashlib
import struct

import numpy as np

from modelmesh_amd import _lib
from modelmesh_amd import workload as wl

B36 = "0123456789abcdefghijklmnopqrstuvwxyz"


def _b36(i: int, width: int) -> str:
    s = ""
    for _ in range(width):
        s = B36[i % 36] + s
        i //= 36
    return s


def string_ids(fleet, seed: int):
    """Give every instance an id consistent with its replica set; id_order := String.compareTo rank; registry entries re-sorted."""
    rng = np.random.default_rng(0x1D5 + seed)
    P = fleet.n_pods
    tag = rng.permutation(P)  # decouples the id order from the pod index
    ids = []
    for p in range(P):
        rs = int(fleet.pods["replica_set"][p])
        ids.append(f"{rs:06x}-{_b36(int(tag[p]), 5)}" if rs >= 0 else "s" + _b36(int(tag[p]), 4))  # |id| < 7: no replica set (:4769)
    assert len(set(ids)) == P
    order = sorted(range(P), key=lambda p: ids[p])  # ASCII: Python's str order == String.compareTo's
    rank = np.empty(P, np.uint32)
    rank[order] = np.arange(P, dtype=np.uint32)
    fleet.pods["id_order"] = rank
    # instanceIds (a TreeMap) and loadFailedInstanceIds iterate in id order
    ep, et = fleet.ent_pod.copy(), fleet.ent_time.copy()
    for m in fleet.models:
        for a, k in ((int(m["ent_off"]), int(m["n_loaded"])), (int(m["ent_off"] + m["n_loaded"]), int(m["n_failed"]))):
            if k > 1:
                o = np.argsort(rank[fleet.ent_pod[a:a + k]], kind="stable")
                ep[a:a + k], et[a:a + k] = fleet.ent_pod[a:a + k][o], fleet.ent_time[a:a + k][o]
    fleet.ent_pod, fleet.ent_time = ep, et
    return ids


def place_cases():
    """(name, fleet, ids, reqs, extra): the fuzz fleets x profiles of the GPU parity tests, the scenario fleets, C1, C2."""
    for profile in (None, "full", "prefer"):
        for seed in range(16):
            pods = int(np.random.default_rng(seed).choice([1, 7, 63, 64, 65, 200, 700, 5000]))
            fleet = wl.fuzz_fleet(seed, pods=pods, profile=profile)
            ids = string_ids(fleet, seed)
            reqs, extra = wl.fuzz_requests(fleet, seed, 2000)
            yield f"fuzz_{profile}_{seed}", fleet, ids, reqs, extra
    for name, fleet, reqs, extra in wl.scenario_fleets():
        ids = string_ids(fleet, 99)
        yield f"scenario_{name}", fleet, ids, reqs, extra
    for cfg, seed in (("C1", 11), ("C2", 12)):
        fleet = wl.make_fleet(cfg)
        ids = string_ids(fleet, seed)
        reqs, extra = wl.make_requests(fleet, seed)
        yield cfg, fleet, ids, reqs, extra
    yield from big_place_cases()


def caller_place_cases():
    """(name, fleet, ids, reqs, extra): batches issued by ONE instance — every request of a batch carries the same self /
    favourSelf / getFreshInstanceRecord() (MM.java:5369-5386), as the batches of the rate task, the janitor, the reaper and
    preShutdown do.  The harness decides them as ordinary getNext calls; the device in the single-caller form
    (mmp_place_batch_c: 24-byte rows, tests/test_ref_vectors_gpu.py)."""
    for k, (seed, profile, pods) in enumerate(((3, None, 200), (5, "full", 700), (8, "prefer", 300), (12, "full", 5000), (14, None, 65))):
        fleet = wl.fuzz_fleet(seed, pods=pods, profile=profile)
        ids = string_ids(fleet, 200 + k)
        rng = np.random.default_rng(900 + k)
        for j in range(3):
            reqs, extra = wl.fuzz_requests(fleet, 70 * k + j, 3000)
            sp = -1 if (k + j) % 5 == 4 else int(rng.integers(0, pods))
            row = fleet.pods[max(sp, 0)]
            reqs["self_pod"], reqs["flags"] = sp, (j == 1)
            reqs["fresh_lru"] = row["lru_time"] if j != 2 else fleet.now - 130_000
            reqs["fresh_capacity"] = row["capacity"]
            reqs["fresh_used"] = row["used"] if j == 0 else int(row["capacity"] * [0.2, 0.8, 0.99][(k + j) % 3])
            reqs["fresh_count"] = int(row["count"]) + j
            reqs["fresh_rpm"] = 0 if j < 2 else 120
            yield f"caller_{k}_{j}", fleet, ids, reqs, extra
    fleet = wl.make_full_cluster(wl.make_fleet("C3"))
    ids = string_ids(fleet, 14)
    reqs, extra = wl.make_requests(fleet, seed=0xBE7C1)
    reqs = wl.sample_requests(reqs, 4000, 5)
    row = fleet.pods[4321]
    reqs["self_pod"], reqs["flags"] = 4321, 0
    reqs["fresh_lru"], reqs["fresh_capacity"], reqs["fresh_used"] = row["lru_time"], row["capacity"], row["used"]
    reqs["fresh_count"], reqs["fresh_rpm"] = row["count"], 0
    yield "caller_C3_full_cluster", fleet, ids, reqs, extra


def big_place_cases():
    """The configurations the bench quotes (BASELINE.json configs[2], [3]) and the two regimes with paths of their own on the
    device: the whole 10k / 50k-instance order and a seeded sample of the one-decision-per-model batch.  C3 as it is (window
    path); C3 with every instance full — the bench's `full_cluster` fleet and batch (prefix tables, case (b) from the whole-window
    tables); C3 with types only a dozen instances may host (next-non-empty-word tables); C4's 50k-instance table."""
    fleet = wl.make_fleet("C3")
    ids = string_ids(fleet, 13)
    reqs, extra = wl.make_requests(fleet, 13)
    yield "C3_table", fleet, ids, wl.sample_requests(reqs, 20000, 1), extra
    fleet = wl.make_full_cluster(wl.make_fleet("C3"))
    ids = string_ids(fleet, 14)
    reqs, extra = wl.make_requests(fleet, seed=0xBE7C0)
    yield "C3_full_cluster", fleet, ids, wl.sample_requests(reqs, 6000, 2), extra
    fleet = wl.add_sparse_types(wl.make_fleet("C3"))
    ids = string_ids(fleet, 15)
    reqs, extra = wl.make_requests(fleet, seed=0xBE7C0)
    sparse = np.nonzero(fleet.models["type"][reqs["model"]] >= 4)[0]
    pick = np.sort(np.concatenate([sparse[:: max(1, len(sparse) // 2000)][:2000], np.random.default_rng(3).choice(len(reqs), 2000, replace=False)]))
    yield "C3_sparse_types", fleet, ids, np.ascontiguousarray(reqs[np.unique(pick)]), extra
    fleet = wl.make_fleet("C4")
    ids = string_ids(fleet, 16)
    reqs, extra = wl.make_requests(fleet, 16)
    yield "C4_table", fleet, ids, wl.sample_requests(reqs, 10000, 4), extra


def serve_cases():
    """(name, fleet, ids, reqs, in_use, last_used, excl_pod, excl_time): serve-target requests on fuzz fleets — load-start times
    that straddle the assume-completed cutoff and collide, models with many copies, tried pairs and key excludes."""
    for seed in range(6):
        rng = np.random.default_rng(1000 + seed)
        fleet = wl.fuzz_fleet(seed, pods=int(rng.choice([8, 64, 300])), models=400)
        P, now = fleet.n_pods, fleet.now
        fleet.ent_time[:] = now - rng.choice([500, 2_999, 3_000, 3_001, 10_000, 10_000, 60_000], len(fleet.ent_time))
        if P >= 8:
            ent_pod, ent_time = list(fleet.ent_pod), list(fleet.ent_time)
            for i in np.nonzero(rng.random(fleet.n_models) < 0.1)[0]:
                k = int(rng.integers(5, 9))
                fleet.models["ent_off"][i], fleet.models["n_loaded"][i], fleet.models["n_failed"][i] = len(ent_pod), k, 0
                ent_pod += list(rng.choice(P, size=k, replace=False))
                ent_time += list(now - rng.choice([500, 2_999, 3_000, 3_001, 10_000, 60_000], k))
            fleet.ent_pod = np.array(ent_pod, np.int32)
            fleet.ent_time = np.array(ent_time, np.int64)
        ids = string_ids(fleet, 50 + seed)
        n = 3000
        reqs = np.zeros(n, dtype=_lib.SERVE_REQ)
        reqs["model"] = rng.integers(0, fleet.n_models, n)
        reqs["self_pod"] = np.where(rng.random(n) < 0.1, -1, rng.integers(0, P, n))
        m = fleet.models[reqs["model"]]
        has = m["n_loaded"] > 0
        pickc = (m["ent_off"] + rng.integers(0, 8, n) % np.maximum(m["n_loaded"], 1)).clip(0, max(len(fleet.ent_pod) - 1, 0))
        if len(fleet.ent_pod):
            reqs["self_pod"] = np.where(has & (rng.random(n) < 0.5), fleet.ent_pod[pickc], reqs["self_pod"])
        reqs["flags"] = rng.integers(0, 4, n)
        reqs["local_in_flight"] = rng.integers(0, 3, n)
        reqs["last_invoke_time"] = now - rng.choice([0, 10, 1000], n)
        reqs["assume_completed_ms"] = rng.choice([3000, 30_000], n)
        in_use = rng.integers(0, 3, P).astype(np.int32)
        last_used = (now - rng.choice([0, 5, 5, 100, 10_000], P)).astype(np.int64)
        ne = np.where(rng.random(n) < 0.3, rng.integers(1, 8, n), 0).astype(np.int32)
        off = np.zeros(n + 1, np.int64)
        np.cumsum(ne, out=off[1:])
        reqs["excl_off"], reqs["n_excl"] = off[:-1], ne
        excl_pod = np.zeros(int(off[-1]), np.int32)
        excl_time = np.zeros(int(off[-1]), np.int64)
        for i in np.nonzero(ne)[0]:
            mm = fleet.models[reqs["model"][i]]
            for j in range(ne[i]):
                if mm["n_loaded"] > 0 and rng.random() < 0.8:
                    e = mm["ent_off"] + rng.integers(0, mm["n_loaded"])
                    excl_pod[off[i] + j] = fleet.ent_pod[e]
                    excl_time[off[i] + j] = _lib.ANY_TIME if rng.random() < 0.5 else fleet.ent_time[e] + rng.integers(0, 2)
                else:
                    excl_pod[off[i] + j] = rng.integers(0, P)
                    excl_time[off[i] + j] = _lib.ANY_TIME
        yield f"serve_{seed}", fleet, ids, reqs, in_use, last_used, excl_pod, excl_time


def gate_cases():
    """(name, fleet, ids, reqs, excl_pod, excl_time, explicit, in_use_expiry): the request-level guards (mmp_gate_req) on fuzz
    fleets — models with many copies / failures so that the count guards trigger, fresh rows near and far from the table's."""
    for seed in range(4):
        rng = np.random.default_rng(3000 + seed)
        fleet = wl.fuzz_fleet(seed + 40, pods=int(rng.choice([8, 64, 300])), models=300, profile=None if seed % 2 else "prefer")
        P, now = fleet.n_pods, fleet.now
        fleet.ent_time[:] = now - rng.choice([100, 1_400, 1_600, 449_000, 451_000, 3_000_000], len(fleet.ent_time))
        m = fleet.models
        big = np.nonzero(rng.random(len(m)) < 0.1)[0]
        ent_pod, ent_time = list(fleet.ent_pod), list(fleet.ent_time)
        for i in big:
            k, f = int(rng.integers(4, min(8, P) + 1)) if P >= 5 else min(P, 2), int(rng.integers(0, min(8, P)))
            f = min(f, P - k) if P - k > 0 else 0
            pods = rng.choice(P, size=k + f, replace=False)
            m["ent_off"][i], m["n_loaded"][i], m["n_failed"][i] = len(ent_pod), k, f
            ent_pod += list(pods)
            ent_time += list(now - rng.choice([100, 449_000, 451_000], k + f))
        fleet.ent_pod = np.array(ent_pod, np.int32)
        fleet.ent_time = np.array(ent_time, np.int64)
        ids = string_ids(fleet, 70 + seed)
        n = 3000
        r = np.zeros(n, dtype=_lib.GATE_REQ)
        r["model"] = rng.integers(0, fleet.n_models, n)
        r["self_pod"] = rng.integers(0, P, n)
        mm = m[r["model"]]
        has = mm["n_loaded"] > 0
        pick = (mm["ent_off"] + rng.integers(0, 8, n) % np.maximum(mm["n_loaded"], 1)).clip(0, len(fleet.ent_pod) - 1)
        r["self_pod"] = np.where(has & (rng.random(n) < 0.6), fleet.ent_pod[pick], r["self_pod"])
        r["flags"] = rng.integers(0, 512, n)
        r["size_hint"] = rng.choice([0, 1, 6400, 2_000_000], n)
        r["last_used_time"] = rng.choice([0, now - 5_000, now - 4_000_000], n)
        r["cache_capacity"] = rng.choice([131072, 1_000_000], n)
        r["cache_weighted_size"] = (r["cache_capacity"] * rng.choice([0.1, 0.96, 0.999, 1.0], n)).astype(np.int64)
        r["cache_oldest_time"] = rng.choice([-1, _lib.JAVA_LONG_MAX, now - 1_000, now - 4_500_000, now - 700_000], n)
        r["loader_predicted"] = rng.choice([6400, 1, 200_000], n)
        r["loading_count"] = rng.integers(0, 20, n)
        r["weight_predict_cutoff"] = 10
        r["loaded_time"] = rng.choice([-1, now - 1_000, now - 200_000, now - 5_000_000], n)
        r["load_timeout_ms"] = rng.choice([90_000, 720_000], n)
        cur = fleet.pods[r["self_pod"]]
        near = rng.random(n) < 0.6
        r["fresh_lru"] = np.where(near, cur["lru_time"], cur["lru_time"] - rng.choice([0, 10_000, 30_000], n))
        r["fresh_lru"] = np.where(rng.random(n) < 0.04, -1, r["fresh_lru"])  # an empty cache: oldestTime() == -1, read as Long.MAX_VALUE (:5423-5425)
        r["fresh_capacity"] = np.where(near, cur["capacity"], cur["capacity"] - rng.choice([0, 100, 50_000], n))
        r["fresh_used"] = np.where(near, cur["used"], (cur["used"] * rng.choice([1.0, 1.1, 1.3], n)).astype(np.int64))
        r["fresh_count"] = cur["count"] + rng.choice([0, 0, 1, 2, 10], n)
        r["fresh_loading_threads"] = np.where(rng.random(n) < 0.9, cur["loading_threads"], 3)
        r["fresh_in_progress"] = cur["loading_in_progress"] + rng.choice([0, 0, 1, 3], n)
        r["fresh_rpm"] = cur["rpm"] + rng.choice([0, 0, 5, 99, 100, 1000], n)
        r["last_published"] = now - rng.choice([500, 2_500, 38_000, 39_500, 100_000, 170_000], n)
        ne = np.where(rng.random(n) < 0.3, rng.integers(1, 8, n), 0).astype(np.int32)
        off = np.zeros(n + 1, np.int64)
        np.cumsum(ne, out=off[1:])
        r["excl_off"], r["n_excl"] = off[:-1], ne
        excl_pod = rng.integers(0, P, int(off[-1])).astype(np.int32)
        excl_time = np.full(int(off[-1]), _lib.ANY_TIME, np.int64)
        nx = np.where(rng.random(n) < 0.4, rng.integers(1, 8, n), 0).astype(np.int32)
        xoff = np.zeros(n + 1, np.int64)
        np.cumsum(nx, out=xoff[1:])
        r["explicit_off"], r["n_explicit"] = xoff[:-1], nx
        explicit = rng.integers(0, P, int(xoff[-1])).astype(np.int32)
        yield f"gates_{seed}", fleet, ids, r, excl_pod, excl_time, explicit, 450_000


INT_MIN, INT_MAX, LONG_MIN, LONG_MAX = -(2**31), 2**31 - 1, -(2**63), 2**63 - 1
GATE_EDGE_TIERS = ("timed", "totals", "thresholds", "wrap")
GATE_EXPIRY = 450_000
GATE_CUTOFF = 10  # weight_predict_cutoff of the engineered rows
N_TOTALS_PLAIN = 300  # ordinary rows behind the engineered ones of a gate_totals case


def _edge_fleet(P, seed, groups=()):
    """An orderly fleet (one version, every instance live and present, nothing full) that the tiers below then bend where they
    need to.  groups: type t + 1 may only be placed on the instances groups[t]; type 0 is unconstrained."""
    rng = np.random.default_rng(0xE06E + seed)
    now = wl.NOW_MS
    rows = np.zeros(P, dtype=_lib.POD_ROW)
    rows["capacity"] = 1_000_000
    rows["used"] = rng.choice([200_000, 500_000, 900_000], P)
    rows["count"] = rng.integers(1, 30, P)
    rows["lru_time"] = now - rng.integers(400_000, 9_000_000, P)
    rows["rpm"] = rng.choice([0, 50, 500, 5000], P)
    rows["loading_threads"] = 8
    rows["loading_in_progress"] = rng.integers(0, 3, P)
    rows["version"] = 7
    rows["id_order"] = rng.permutation(P)
    rows["replica_set"] = rng.integers(0, 3, P)
    rows["flags"] = _lib_flag_live()
    fleet = wl.Fleet(pods=rows, models=np.zeros(0, _lib.MODEL_ROW), ent_pod=np.zeros(0, np.int32), ent_time=np.zeros(0, np.int64),
                     min_space_units=6553, min_churn_age_ms=600_000, now=now)
    if groups:
        T = len(groups) + 1
        al = np.zeros((T, P), bool)
        al[0] = True
        for t, g in enumerate(groups):
            al[t + 1, list(g)] = True
        fleet.n_types = T
        fleet.allowed, fleet.prefer = wl.bitmap_from_bool(al), wl.bitmap_from_bool(np.zeros((T, P), bool))
        fleet.has_allowed, fleet.has_prefer = np.array([0] + [1] * len(groups), np.uint8), np.zeros(T, np.uint8)
    return fleet, rng


def _set_models(fleet, specs):
    """specs: [(type, copies, failed)] -> the registry, each list in instance-id order (as instanceIds / loadFailedInstanceIds
    iterate; string_ids has run, so id_order IS that order).  Times are set by the caller, by POSITION."""
    rank = fleet.pods["id_order"]
    rows = np.zeros(len(specs), dtype=_lib.MODEL_ROW)
    ent = []
    for i, (ty, lp, fp) in enumerate(specs):
        lp = sorted((int(p) for p in lp), key=lambda p: rank[p])
        fp = sorted((int(p) for p in fp), key=lambda p: rank[p])
        rows[i] = (ty, len(ent), len(lp), len(fp), fleet.now - 5_000)
        ent += lp + fp
    fleet.models = rows
    fleet.ent_pod = np.array(ent, np.int32)
    fleet.ent_time = np.full(len(ent), fleet.now - 3_000_000, np.int64)


def _copies(fleet, i):
    m = fleet.models[i]
    a, k, f = int(m["ent_off"]), int(m["n_loaded"]), int(m["n_failed"])
    return fleet.ent_pod[a:a + k], fleet.ent_time[a:a + k], fleet.ent_pod[a + k:a + k + f], fleet.ent_time[a + k:a + k + f]


def _count_specs(rng, P, n_types):
    """A few models with enough copies / failure records for the two caps (the tiers that are about something else still have to
    see every guard both ways)."""
    out = []
    for k, f in ((5, 3), (6, 0), (2, 5), (4, 2)):
        pods = rng.choice(P, size=min(k + f, P), replace=False)
        out.append((int(rng.integers(0, max(n_types, 1))), list(pods[:min(k, P)]), list(pods[min(k, P):])))
    return out


def _edge_rows(fleet, rng, model, self_pod):
    """Ordinary values in every field of a guard request (as gate_cases draws them), no exclusions; the tiers overwrite what
    they are about."""
    n, now = len(model), fleet.now
    r = np.zeros(n, dtype=_lib.GATE_REQ)
    r["model"], r["self_pod"] = model, self_pod
    r["flags"] = rng.integers(0, 512, n)
    r["size_hint"] = rng.choice([0, 1, 6400, 2_000_000], n)
    r["last_used_time"] = rng.choice([0, now - 5_000, now - 4_000_000], n)
    r["cache_capacity"] = rng.choice([131072, 1_000_000], n)
    r["cache_weighted_size"] = (r["cache_capacity"] * rng.choice([0.1, 0.96, 0.999, 1.0], n)).astype(np.int64)
    r["cache_oldest_time"] = rng.choice([-1, LONG_MAX, now - 1_000, now - 4_500_000, now - 700_000], n)
    r["loader_predicted"] = rng.choice([6400, 1, 200_000], n)
    r["loading_count"] = rng.integers(0, 20, n)
    r["weight_predict_cutoff"] = GATE_CUTOFF
    r["loaded_time"] = rng.choice([-1, now - 1_000, now - 200_000, now - 5_000_000], n)
    r["load_timeout_ms"] = rng.choice([90_000, 720_000], n)
    cur = fleet.pods[r["self_pod"]]
    near = rng.random(n) < 0.6
    r["fresh_lru"] = np.where(near, cur["lru_time"], cur["lru_time"] - rng.choice([0, 10_000, 30_000], n))
    r["fresh_capacity"] = np.where(near, cur["capacity"], cur["capacity"] - rng.choice([0, 100, 50_000], n))
    r["fresh_used"] = np.where(near, cur["used"], (cur["used"] * rng.choice([1.0, 1.1, 1.3], n)).astype(np.int64))
    r["fresh_count"] = cur["count"] + rng.choice([0, 0, 1, 2, 10], n)
    r["fresh_loading_threads"] = np.where(rng.random(n) < 0.9, cur["loading_threads"], 3)
    r["fresh_in_progress"] = cur["loading_in_progress"] + rng.choice([0, 0, 1, 3], n)
    r["fresh_rpm"] = cur["rpm"] + rng.choice([0, 0, 5, 99, 100, 1000], n)
    r["last_published"] = now - rng.choice([500, 2_500, 38_000, 39_500, 100_000, 170_000], n)
    return r


def _publish_row(fleet, rng, p, lp=50_000, flags=0, **over):
    """One row of caller p whose fresh record EQUALS the table's (published lp ms ago: checked, not old, nothing to publish), with
    the fields in `over` moved: that field alone decides publishInstanceRecord."""
    q = _edge_rows(fleet, rng, np.array([0]), np.array([p]))
    cur = fleet.pods[p]
    q["flags"] = (q["flags"] & np.uint32(63)) | flags | (256 if cur["flags"] & 1 else 0)
    q["fresh_lru"], q["fresh_capacity"], q["fresh_used"], q["fresh_count"] = cur["lru_time"], cur["capacity"], cur["used"], cur["count"]
    q["fresh_loading_threads"], q["fresh_in_progress"], q["fresh_rpm"] = cur["loading_threads"], cur["loading_in_progress"], cur["rpm"]
    q["last_published"] = fleet.now - lp
    for k, v in over.items():
        q[k] = v
    return q


def _i32(x):
    return (int(x) + 2**31) % 2**32 - 2**31


def _i64(x):
    return (int(x) + 2**63) % 2**64 - 2**63


def _random_rows(fleet, rng, n):
    """n ordinary rows: the caller is one of the model's copies more often than not; short lists of key excludes and explicit
    excludes on some."""
    P = fleet.n_pods
    model = rng.integers(0, fleet.n_models, n)
    self_pod = rng.integers(0, P, n)
    for i in range(n):
        lp = _copies(fleet, model[i])[0]
        if len(lp) and rng.random() < 0.6:
            self_pod[i] = lp[rng.integers(0, len(lp))]
    r = _edge_rows(fleet, rng, model, self_pod)
    excl = [[(int(rng.integers(0, P)), _lib.ANY_TIME) for _ in range(int(rng.integers(1, 8)))] if rng.random() < 0.3 else [] for _ in range(n)]
    expl = [[int(x) for x in rng.integers(0, P, int(rng.integers(1, 8)))] if rng.random() < 0.4 else [] for _ in range(n)]
    return r, excl, expl


def _with_lists(r, excl, expl):
    """excl: per row [(instance, time)]; expl: per row [instance] -> (rows with the offsets set, excl_pod, excl_time, explicit)."""
    r = r.copy()
    ne, nx = np.array([len(x) for x in excl], np.int64), np.array([len(x) for x in expl], np.int64)
    r["excl_off"], r["n_excl"] = np.cumsum(ne) - ne, ne
    r["explicit_off"], r["n_explicit"] = np.cumsum(nx) - nx, nx
    excl_pod = np.array([p for x in excl for p, _ in x], np.int32)
    excl_time = np.array([t for x in excl for _, t in x], np.int64)
    explicit = np.array([p for x in expl for p in x], np.int32)
    return r, excl_pod, excl_time, explicit


def _cat(parts):
    rows = np.concatenate([p[0] for p in parts])
    return rows, [x for p in parts for x in p[1]], [x for p in parts for x in p[2]]


def timed_combinations(fleet, r, excl_pod, excl_time):
    """{(exclusion at index >= 4, copy at index >= 4, 'equal' | 'off' | 'any')}: which pairs of an exclusion and a copy of the
    same instance a set of rows holds ('off': the exclusion's time is the copy's + 1, so it must NOT filter)."""
    seen = set()
    for q in r:
        lp, lt, _, _ = _copies(fleet, q["model"])
        for x in range(q["n_excl"]):
            p, t = excl_pod[q["excl_off"] + x], excl_time[q["excl_off"] + x]
            for e in np.nonzero(lp == p)[0]:
                kind = "any" if t == _lib.ANY_TIME else "equal" if t == lt[e] else "off" if t == lt[e] + 1 else None
                if kind:
                    seen.add((x >= 4, bool(e >= 4), kind))
    return seen


def _timed_case(P, seed, typed):
    fleet, rng = _edge_fleet(P, seed, [range(0, P, 2), range(P // 2, P)] if typed else ())
    ids = string_ids(fleet, 300 + seed)
    now = fleet.now
    specs = []
    for k in range(1, 9):
        for j in range(6):
            pods = rng.choice(P, size=k, replace=False)
            if P > 64 and j < 3 and P - 1 not in pods:
                pods[0] = P - 1  # the caller of the second bitmap word holds copies too
            specs.append((int(rng.integers(0, fleet.n_types)) if typed else 0, list(pods), []))
    specs += _count_specs(rng, P, fleet.n_types)
    _set_models(fleet, specs)
    fleet.ent_time[:] = now - rng.choice([0, 1499, 1500, 50_000], len(fleet.ent_time))
    model, self_pod, flags, excl = [], [], [], []
    lo, hi = [(1, 0), (4, 3), (9, 0), (3, 1)], [(5, 4), (9, 8), (7, 5), (9, 4)]  # (list length, index of the pair that matters)
    c = 0

    def filler(lp, lt, others):
        if len(others) and rng.random() < 0.5:
            return int(rng.choice(others)), _lib.ANY_TIME  # not a copy of the model
        q = int(rng.integers(0, len(lp)))
        return int(lp[q]), int(lt[q]) + 1 + int(rng.integers(0, 2))  # a copy, at another time: filters nothing
    for i in range(48):
        lp, lt, _, _ = _copies(fleet, i)
        k = len(lp)
        others = np.setdiff1d(np.arange(P), lp)
        for e in range(k):
            for kind in range(3):
                for where in (lo, hi):
                    L, x = where[c % 4]
                    lst = [filler(lp, lt, others) for _ in range(L)]
                    lst[x] = (int(lp[e]), [_lib.ANY_TIME, int(lt[e]), int(lt[e]) + 1][kind])
                    model.append(i)
                    self_pod.append(int([lp[e], lp[(e + 1) % k], rng.integers(0, P)][c % 3]))  # its own copy excluded: has_local flips
                    flags.append(3 if c % 2 == 0 else int(rng.integers(0, 8)))
                    excl.append(lst)
                    c += 1
        for keep in (0, k - 1) if k >= 2 else ():  # every copy but one excluded: filteredCount == 1
            lst = [(int(lp[e]), _lib.ANY_TIME if (e + c) % 2 else int(lt[e])) for e in range(k) if e != keep]
            model.append(i)
            self_pod.append(int(lp[keep] if c % 2 else lp[(keep + 1) % k]))
            flags.append(int(rng.integers(0, 8)))
            excl.append([lst[j] for j in rng.permutation(len(lst))])
            c += 1
    r = _edge_rows(fleet, rng, np.array(model), np.array(self_pod))
    r["flags"] = (r["flags"] & ~np.uint32(7)) | np.array(flags, np.uint32)
    expl = [[int(x) for x in rng.integers(0, P, int(rng.integers(1, 8)))] if rng.random() < 0.3 else [] for _ in range(len(r))]
    rows, excl, expl = _cat([(r, excl, expl), _random_rows(fleet, rng, 200)])
    return (fleet, ids) + _with_lists(rows, excl, expl) + (GATE_EXPIRY,)


def estimate_of(total_capacity, total_free, copy_count):
    """loadLocal's -(1 + (int) (totalCapacity - totalFree) / copyCount) in Java's arithmetic (MM.java:5170-5175) — used to AIM
    the engineered rows (cache sizes on either side of |initialSize|) and to name the sizing outcome of a row; the expected
    outputs come from the reference."""
    d = (total_capacity - total_free) & 0xFFFFFFFF
    d -= (d >> 31) << 32
    q = abs(d) // copy_count * (1 if d >= 0 else -1)
    e = (-(1 + q)) & 0xFFFFFFFF
    return e - ((e >> 31) << 32)


def totals_plan(P, c):
    """The instance groups of a gate_totals fleet: [(instances, capacity - free or None, copies, what)]; type t + 1 <-> group t."""
    used = [2**31 - 1, 2**31, 2**31 + 5, 2**32 - 2 * c, 2**32 - c - 1, 2**32 - 1, 2**32, 2**32 + 99]
    plan = [(list(range(5 * i, 5 * i + 5)), d, c, "used") for i, d in enumerate(used)]
    plan.append((list(range(40, 52)), 10**10, c, "used"))
    plan.append(([52], None, c, "one instance, 20 * free == capacity"))
    plan.append(([53, 54], None, c, "20 * free == capacity"))
    plan.append(([55, P - 1], None, c, "20 * free == capacity - 1"))
    return plan


def _totals_case(P, c, seed):
    plan = totals_plan(P, c)
    fleet, rng = _edge_fleet(P, seed, [g for g, _, _, _ in plan])
    ids = string_ids(fleet, 320 + seed)
    now, pods = fleet.now, fleet.pods
    for g, d, copies, what in plan:
        k = len(g)
        pods["count"][g] = copies // k
        pods["count"][g[0]] += copies - copies // k * k
        if d is not None:  # nothing full: capacity - free = the sum of `used`
            pods["capacity"][g] = 2**29 if d // k < 2**29 - 2**20 else 2**30
            pods["used"][g] = d // k
            pods["used"][g[0]] += d - d // k * k
        else:
            free = [6_710_886, 13_421_772][:k] if k == 2 else [6_710_886]
            for p, f in zip(g, free):
                pods["capacity"][p], pods["used"][p] = 20 * f, 19 * f
            if what.endswith("- 1"):
                pods["capacity"][g[1]] += 1
                pods["used"][g[1]] += 1
    T = fleet.n_types
    specs = []
    for t in range(T):
        g = plan[t - 1][0] if t else list(range(P))
        specs += [(t, [], []), (t, [g[0]], []), (t, list(g[:2]), [g[-1]] if len(g) > 2 else [])]
    specs += [(T + 3, [56], []), (-1, [57, 58], [])]  # no such type row: answered from row 0
    specs += _count_specs(rng, P, T)
    _set_models(fleet, specs)
    fleet.ent_time[:] = now - rng.choice([100, 449_000, 451_000, 3_000_000], len(fleet.ent_time))
    n_eng = len(specs) - 4
    model = np.repeat(np.arange(n_eng), 27)
    lc, hint, pred = (np.tile(a.reshape(-1), n_eng) for a in np.meshgrid([GATE_CUTOFF - 1, GATE_CUTOFF, GATE_CUTOFF + 1], [0, 1, 2], [0, 1, 6400],
                                                                         indexing="ij"))
    n = len(model)
    self_pod = np.where(np.arange(n) % 4 == 0, P - 1, rng.integers(0, P, n))
    r = _edge_rows(fleet, rng, model, self_pod)
    r["loading_count"], r["loader_predicted"] = lc, pred
    r["flags"] = np.where(hint > 0, r["flags"] | 32, r["flags"] & ~np.uint32(32))
    r["size_hint"] = np.where(hint == 1, 0, 6400)
    # the early reject on either side of equality: |initialSize| against the cache's capacity, then against its free space
    pods_present = (pods["flags"] & 5) == 0
    rem = np.maximum(pods["capacity"] - pods["used"], 0)
    al = np.ones((max(T, 1), P), bool)
    for t, (g, _, _, _) in enumerate(plan):
        al[t + 1] = np.isin(np.arange(P), g)
    for i in range(n):
        ty = int(fleet.models["type"][model[i]])
        sel = al[ty if 0 <= ty < T else 0] & pods_present
        cap, free = int(pods["capacity"][sel].sum()), int(rem[sel & (rem >= fleet.min_space_units)].sum())
        copies = int(pods["count"][sel].sum())
        size = 6400 if hint[i] == 2 else 0
        if not hint[i] and lc[i] > GATE_CUTOFF and copies >= 10:
            size = estimate_of(cap, free, copies)
        size = abs(size or int(pred[i]))
        how, d = int(rng.integers(0, 3)), int(rng.integers(-1, 2))
        r["flags"][i] = (r["flags"][i] & ~np.uint32(8)) | (8 if how else 0)
        if how == 1:
            r["cache_capacity"][i], r["cache_weighted_size"][i] = size + d, 0
        elif how == 2:
            r["cache_capacity"][i], r["cache_weighted_size"][i] = 2**40, 2**40 - (size + d)
            r["last_used_time"][i], r["cache_oldest_time"][i] = now - 5_000, now - 1_000
        # onEviction: now - loadedTime against 2 * loadTimeoutMs, around equality
        r["flags"][i] &= ~np.uint32(16)
        r["load_timeout_ms"][i], r["loaded_time"][i] = 90_000, now - (180_000 + int(rng.integers(-1, 2)))
    excl, expl = [[] for _ in range(n)], [[] for _ in range(n)]
    rows, excl, expl = _cat([(r, excl, expl), _random_rows(fleet, rng, N_TOTALS_PLAIN)])
    return (fleet, ids) + _with_lists(rows, excl, expl) + (GATE_EXPIRY,)


def _thresholds_case(P, seed, typed):
    # three small groups that are about 20 * free / capacity (onEviction), as in the totals fleets
    plan = [([52], "one instance"), ([53, 54], "20 * free == capacity"), ([55, 56], "20 * free == capacity - 1")] if typed else []
    fleet, rng = _edge_fleet(P, seed, [g for g, _ in plan])
    ids = string_ids(fleet, 340 + seed)
    now, pods, msu = fleet.now, fleet.pods, fleet.min_space_units
    for g, what in plan:
        for p, f in zip(g, [6_710_886, 13_421_772]):
            pods["capacity"][p], pods["used"][p] = 20 * f, 19 * f
        if what.endswith("- 1"):
            pods["capacity"][g[1]] += 1
            pods["used"][g[1]] += 1
    byrank = np.argsort(pods["id_order"])
    mid = P // 2 + (byrank[P // 2] == P - 1)
    tomb = int(byrank[mid])  # a tombstone in the middle of the id order: a copy list can hold it at any position
    A, B, Cc, Dd, Fs = [p for p in (P - 1, 1, 2, 3, 4, 6, 7, 5) if p != tomb][:5]  # A = the last instance: the second bitmap word of 65
    for p, (used, count, age, rpm, inprog) in ((A, (500_000, 40, 5_000_000, 5000, 5)), (B, (500_000, 1000, 160_000, 500, 8)),
                                               (Dd, (1_000_000 - msu, 20, 3_000_000, 50, 1)), (Fs, (500_000, 10, 3_000_000, 50, 1))):
        pods["capacity"][p], pods["used"][p], pods["count"][p], pods["lru_time"][p] = 1_000_000, used, count, now - age
        pods["rpm"][p], pods["loading_in_progress"][p], pods["loading_threads"][p] = rpm, inprog, 8
    pods["capacity"][Cc], pods["used"][Cc], pods["count"][Cc], pods["lru_time"][Cc] = 1_000_000, 0, 0, LONG_MAX  # an empty cache
    pods["rpm"][Cc], pods["loading_in_progress"][Cc] = 0, 0
    pods["flags"][tomb] = 4
    pods["flags"][Fs] = 3  # announced its shutdown, still in the table
    lower = [int(p) for p in byrank[:mid] if p != Fs]
    upper = [int(p) for p in byrank[mid + 1:] if p != Fs]
    r_, e_, o_ = now - GATE_EXPIRY + 1, now - GATE_EXPIRY, now - GATE_EXPIRY - 1  # failure times: > cutoff, at it, before it
    fail_pat = [[r_, r_, r_], [r_, r_, e_, r_], [r_, e_, r_, o_, r_], [r_, r_, e_, o_, e_], [r_, r_, o_], [e_, e_, e_], [r_, o_, r_, e_, o_, r_],
                [e_, o_, r_, r_, r_], [o_, o_, o_, o_, r_, r_]]
    # copy lists by position: L an instance of the table, T the tombstone, X an instance the request excludes explicitly
    loc_pat = ["LLLL", "LLLLL", "TLLLL", "TLLLLL", "LLLLT", "LLLLTL", "LLXLL", "LLXLLL", "LLLLXL", "LLLLLX", "LLTLXLL", "XLLLL"]
    specs, loc_x = [], []
    for times in fail_pat:
        specs.append((0, [], list(rng.choice(P, size=len(times), replace=False))))
    for pat in loc_pat:
        t_at = pat.find("T")
        if t_at >= 0:
            cp = lower[:t_at] + [tomb] + upper[:len(pat) - t_at - 1]
        else:
            cp = upper[:len(pat)]
        specs.append((0, cp, []))
    go_times = [[100, 1499], [100, 1500], [1499, 100], [1500, 100], [1499, 1499, 100], [1500, 3000, 100], [0, 1500], [100, 100]]
    for times in go_times:
        specs.append((0, list(rng.choice(upper, size=len(times), replace=False)), []))
    n_spec = len(specs)
    specs += [(t + 1, [g[0]], []) for t, (g, _) in enumerate(plan)]
    specs += _count_specs(rng, P, fleet.n_types)
    _set_models(fleet, specs)
    for i, times in enumerate(fail_pat):
        m = fleet.models[i]
        fleet.ent_time[m["ent_off"]: m["ent_off"] + m["n_failed"]] = times
    for i, times in enumerate(go_times):
        m = fleet.models[len(fail_pat) + len(loc_pat) + i]
        fleet.ent_time[m["ent_off"]: m["ent_off"] + m["n_loaded"]] = now - np.array(times)
    parts = []
    # ---- the caps and goLocal's 1500 ms, by every caller kind
    model, self_pod, expl = [], [], []
    for i in range(n_spec):
        lp = _copies(fleet, i)[0]
        pat = loc_pat[i - len(fail_pat)] if len(fail_pat) <= i < len(fail_pat) + len(loc_pat) else ""
        for rep in range(4):
            model.append(i)
            self_pod.append(int(lp[rep % len(lp)]) if len(lp) and rep < 3 else A)
            x = [int(lp[j]) for j, ch in enumerate(pat) if ch == "X"]
            pad = [int(p) for p in lower[:6] if p not in lp]
            # the excluded copy sits before / after the explicit list's fourth entry
            expl.append((pad[:rep + 2] + x + pad[rep + 2:rep + 3]) if x else (pad[:rep] if rep % 2 else []))
    r = _edge_rows(fleet, rng, np.array(model), np.array(self_pod))
    r["flags"] = (r["flags"] & ~np.uint32(7)) | 3  # favourSelfForHits, a cache entry that is not done: oldest() decides
    parts.append((r, [[] for _ in range(len(r))], expl))

    # ---- publishInstanceRecord: a fresh record equal to the table's, one field moved to just inside / outside its threshold
    prow = []

    def pub(p, lp=50_000, flags=0, **over):
        prow.append(_publish_row(fleet, rng, p, lp, flags, **over))
    cap, lru = 1_000_000, int(pods["lru_time"][A])
    d_in = max(d for d in range(19_000, 21_000) if d < (cap - d) // 50)  # |cur - cap| < cap / 50, cap being the FRESH capacity
    u_in = max(d for d in range(19_000, 21_000) if d < (cap + d) // 50)
    for p in (A, B, Cc, Dd, Fs):
        for lp, flags in ((1_999, 64), (2_000, 64), (38_999, 0), (39_000, 0), (1_999, 128), (500, 64 | 128)):
            pub(p, lp, flags, fresh_count=int(pods["count"][p]) + 20)
        for lp in (160_000, 160_001):
            pub(p, lp, fresh_in_progress=int(pods["loading_in_progress"][p]) + 1 if p in (A, Cc) else int(pods["loading_in_progress"][p]))
            pub(p, lp, fresh_used=int(pods["used"][p]) + 1)
        pub(p, fresh_loading_threads=7)
        pub(p, flags=256)
        pub(p)
    for d in (d_in, d_in + 1):
        pub(A, fresh_capacity=cap - d)
    for d in (u_in, u_in + 1):
        pub(A, fresh_capacity=cap + d)
    for d in (19_999, 20_000, -19_999, -20_000):
        pub(A, fresh_lru=lru - d)
    for d in (9_999, 10_000, -9_999, -10_000):  # (now - lruTime) / 16 = 10 000 for B
        pub(B, fresh_lru=int(pods["lru_time"][B]) - d)
    for cnt in (45, 46, 35, 34, 49, 50):  # 15 % of 40, then the ten copies
        pub(A, fresh_count=cnt)
    for cnt in (1009, 1010, 991, 990):
        pub(B, fresh_count=cnt)
    for used in (599_999, 600_000, 400_001, 400_000):
        pub(A, fresh_used=used)
    for rpm in (5099, 5100, 4901, 4900):
        pub(A, fresh_rpm=rpm)
    for rpm in (554, 555, 446, 445, 599, 600):  # 10 % of 500
        pub(B, fresh_rpm=rpm)
    for rpm in (0, 1):
        pub(Cc, fresh_rpm=rpm)
    for ip in (7, 8, 3, 2, 9):  # +-3 loads; 9 also crosses loadingThreads
        pub(A, fresh_in_progress=ip)
    for ip in (9, 7, 11, 5):
        pub(B, fresh_in_progress=ip)
    for ip in (0, 2, 3, 4):
        pub(Dd, fresh_in_progress=ip)
    for ip in (0, 1, 3):
        pub(Cc, fresh_in_progress=ip)
    for used in (1_000_000 - msu, 1_000_000 - msu + 1, 1_000_000 - msu - 1):  # isFull on either side
        pub(Dd, fresh_used=used)
    for lp in (50_000, 200_000):  # an empty cache: oldestTime() == -1 is Long.MAX_VALUE, the table's value
        for fl in (-1, LONG_MAX, now - 1_000, 0):
            pub(Cc, lp, fresh_lru=fl)
        pub(A, lp, fresh_lru=-1)
    for lp, flags in ((50_000, 0), (50_000, 256), (1_000, 256), (200_000, 256), (200_000, 0), (1_000, 128), (1_000, 128 | 256)):
        pub(tomb, lp, flags)  # no record of the caller in the table: created unless it is shutting down
    pr = np.concatenate(prow)
    parts.append((pr, [[] for _ in range(len(pr))], [[] for _ in range(len(pr))]))

    # ---- the churn guard and onEviction
    n_c = 0
    crow = []
    for space in (msu - 1, msu, msu + 1):
        for oldest in (now - fleet.min_churn_age_ms + 1, now - fleet.min_churn_age_ms, now - fleet.min_churn_age_ms - 1, now, -1, 0, 1, LONG_MAX,
                       LONG_MAX - 1):
            q = _edge_rows(fleet, rng, np.array([n_c % n_spec]), np.array([A]))
            q["cache_capacity"], q["cache_weighted_size"], q["cache_oldest_time"] = 1_000_000, 1_000_000 - space, oldest
            crow.append(q)
            n_c += 1
    ev_models = [n_spec + j for j in range(len(plan))]  # the engineered groups' models
    for mi in ev_models + [0, len(fail_pat)]:
        for timeout in (90_000, 720_000):
            for d in (-1, 0, 1):
                for failed, lt in ((0, now - 2 * timeout - d), (16, now - 2 * timeout - 1), (0, -1), (0, 0)):
                    q = _edge_rows(fleet, rng, np.array([mi]), np.array([B]))
                    q["flags"] = (q["flags"] & ~np.uint32(16)) | failed
                    q["load_timeout_ms"], q["loaded_time"] = timeout, lt
                    crow.append(q)
    cr = np.concatenate(crow)
    parts.append((cr, [[] for _ in range(len(cr))], [[] for _ in range(len(cr))]))
    parts.append(_random_rows(fleet, rng, 300))
    rows, excl, expl = _cat(parts)
    return (fleet, ids) + _with_lists(rows, excl, expl) + (GATE_EXPIRY,)


def _wrap_case(P, seed, typed):
    """HOSTILE values: no mesh produces them.  What is pinned is that the device, like Java, wraps."""
    fleet, rng = _edge_fleet(P, seed, [range(0, P, 3), range(1, P), [5, 7]] if typed else ())
    ids = string_ids(fleet, 360 + seed)
    now, pods = fleet.now, fleet.pods
    if typed:  # two instances whose free space times 20 leaves 64 bits (onEviction's 20 * totalFree): only type 1 keeps small totals
        pods["capacity"][[5, 7]], pods["used"][[5, 7]] = 2**61, 0
    i32 = [0, 1, -1, 99, 100, 101, 2**30, INT_MAX, INT_MIN, INT_MIN + 1]
    i64 = [0, 1, -1, now, 2**62, -(2**62), LONG_MAX, LONG_MIN, LONG_MIN + 1]
    # the table's rows keep to the non-negative values in most places; `count` in all: PLACEMENT_ORDER subtracts counts
    # (MM.java:4676), negative ones would make it no order at all, and the instance order is not what is tested here
    odd = rng.random(P) < 0.5
    for f in ("count", "rpm", "loading_threads", "loading_in_progress"):
        pods[f] = np.where(odd, rng.choice([0, 1, 99, 100, 101, 2**30, INT_MAX], P), pods[f])
    neg = [1, 2, 3, 4, 6, P - 1]  # rows whose rpm / loads in progress / loading threads are negative (compared, never subtracted, by the order)
    pods["rpm"][neg[:3]] = [-1, INT_MIN, INT_MIN + 1]
    pods["loading_in_progress"][neg[3:]] = [-1, INT_MIN, INT_MIN + 1]
    pods["loading_threads"][neg[4]] = -1
    pods["lru_time"] = np.where(rng.random(P) < 0.3, rng.choice([1, now, 2**62, LONG_MAX], P), pods["lru_time"])
    specs = []
    for _ in range(50):
        k, f = int(rng.integers(0, min(8, P) + 1)), int(rng.integers(0, 7))
        f = min(f, P - k)
        ps = rng.choice(P, size=k + f, replace=False)
        specs.append((int(rng.integers(0, max(fleet.n_types, 1))), list(ps[:k]), list(ps[k:])))
    specs += _count_specs(rng, P, fleet.n_types)
    _set_models(fleet, specs)
    fleet.ent_time[:] = np.where(rng.random(len(fleet.ent_time)) < 0.5, rng.choice(i64, len(fleet.ent_time)),
                                 now - rng.choice([100, 1499, 1500, 449_999, 450_000, 450_001], len(fleet.ent_time)))
    n = 1300
    r, _, expl = _random_rows(fleet, rng, n)
    for f in ("size_hint", "loader_predicted", "loading_count", "weight_predict_cutoff", "fresh_count", "fresh_loading_threads",
              "fresh_in_progress", "fresh_rpm"):
        r[f] = rng.choice(i32, n)
    for f in ("last_used_time", "cache_capacity", "cache_weighted_size", "cache_oldest_time", "loaded_time", "load_timeout_ms", "fresh_lru",
              "fresh_capacity", "fresh_used", "last_published"):
        r[f] = rng.choice(i64, n)
    excl = []
    for i in range(n):
        lp, lt, _, _ = _copies(fleet, r["model"][i])
        lst = []
        for _ in range(int(rng.integers(0, 10)) if rng.random() < 0.5 else 0):
            if len(lp) and rng.random() < 0.7:
                e = int(rng.integers(0, len(lp)))
                lst.append((int(lp[e]), int(rng.choice([int(lt[e]), int(lt[e]), LONG_MIN] + i64))))
            else:
                lst.append((int(rng.integers(0, P)), int(rng.choice(i64))))
        excl.append(lst)
    # a difference of exactly MIN_VALUE, whose Math.abs stays negative and passes every "<": one field at a time, the rest of the
    # fresh record equal to the table's; and |difference| * 100 leaving 64 bits
    aimed = []
    for p in range(P):
        cur = pods[p]
        for over in (dict(fresh_count=_i32(int(cur["count"]) + INT_MIN)), dict(fresh_rpm=_i32(int(cur["rpm"]) + INT_MIN)),
                     dict(fresh_in_progress=_i32(int(cur["loading_in_progress"]) + INT_MIN)), dict(fresh_lru=_i64(int(cur["lru_time"]) + LONG_MIN)),
                     dict(fresh_used=_i64(int(cur["used"]) - 2**62)), dict(fresh_used=_i64(int(cur["used"]) + LONG_MIN)),
                     dict(fresh_capacity=_i64(int(cur["capacity"]) + LONG_MIN)), dict(fresh_count=_i32(int(cur["count"]) + INT_MIN + 1)),
                     dict(fresh_used=_i64(int(cur["used"]) - 2**62 + 1)), dict(fresh_rpm=INT_MAX), dict(fresh_rpm=INT_MAX - 1), dict(fresh_rpm=0),
                     dict(fresh_in_progress=INT_MAX), dict(fresh_in_progress=0))[(0 if P <= 8 or p in neg else p % 3)::1 if P <= 8 or p in neg else 3]:
            aimed.append(_publish_row(fleet, rng, p, **over))
    aimed = np.concatenate(aimed)
    none = [[] for _ in range(len(aimed))]
    rows, excl, expl = _cat([(r, excl, expl), (aimed, none, none), _random_rows(fleet, rng, 200)])
    return (fleet, ids) + _with_lists(rows, excl, expl) + (GATE_EXPIRY,)


def gate_edge_cases():
    """(name, fleet, ids, reqs, excl_pod, excl_time, explicit, in_use_expiry) as gate_cases, at the EDGES of the guards' value
    domain; name = gate_<tier>_<case>.  timed: (instance, loadStart) exclusions as a cache-hit retry leaves them, matching and
    off by one, before and behind the device's four-entry prefetch.  totals: fleets whose per-type totalCapacity - totalFree is
    engineered around 2^31 and 2^32 (loadLocal's estimate narrows it to int first), 20 * totalFree at totalCapacity.  thresholds:
    one row just inside, one just outside every threshold of the publish / reload / churn / cap rules.  wrap: hostile values."""
    for P, typed in ((8, False), (24, True), (64, False), (65, True)):
        yield (f"gate_timed_{P}",) + _timed_case(P, P, typed)
    for P, c in ((64, 9), (65, 10), (64, 12), (65, 300)):
        yield (f"gate_totals_c{c}",) + _totals_case(P, c, c)
    for P, typed in ((24, False), (65, True)):
        yield (f"gate_thresholds_{P}",) + _thresholds_case(P, P, typed)
    for P, typed in ((8, False), (65, True)):
        yield (f"gate_wrap_{P}",) + _wrap_case(P, P, typed)


def gate_edge_tier(name):
    return name.split("_")[1]


SIZING_OUTCOMES = ("hint", "negative estimate", "positive estimate", "estimate -1", "estimate 0: loader_predicted")


def sizing_outcomes(fleet, r, tstats):
    """Per row, which way loadLocal's sizing goes (MM.java:5159-5178) — one of SIZING_OUTCOMES, or None where neither a hint nor
    the estimate applies (or the hint is 0).  tstats: typeSetStats per type row."""
    out = []
    for q in r:
        ty = int(fleet.models["type"][q["model"]])
        st = tstats[ty if 0 <= ty < len(tstats) else 0]
        what = None
        if q["flags"] & 32:
            what = "hint" if q["size_hint"] else None
        elif q["loading_count"] > q["weight_predict_cutoff"] and st["model_copy_count"] >= 10:
            e = estimate_of(int(st["total_capacity"]), int(st["total_free"]), int(st["model_copy_count"]))
            what = SIZING_OUTCOMES[1] if e < -1 else SIZING_OUTCOMES[2] if e > 0 else SIZING_OUTCOMES[3] if e == -1 else SIZING_OUTCOMES[4]
        out.append(what)
    return out


PLACE_EDGE_TIERS = ("breaks", "rpm", "order")
RPM_CLASSES = ("m11", "m15", "m3", "m4", "none")  # the strictest clause of :4966-4972 that applies to a request's lastUsedAgo


def place_edge_tier(name):
    return name.split("_")[1]


def place_edge_meta(name):
    """What a place-edge case was built for: pairs [(row inside, row outside, offset)] of requests on either side of one threshold
    — offset 0: the two rows walk from the same first instance; else the outside row's first instance stands that many eligible
    positions behind (negative: in front of) the inside row's, and what must differ is where the two lists END —, caller (the case
    is one caller's batch), after (the name of the case that holds the same table after a few rows changed)."""
    return _place_edge_all()[name][4]


def rpm_class(fleet, last_used):
    ago = 0 if last_used == 0 else fleet.now - int(last_used)
    return "m11" if ago < -1000 else "m15" if ago < 5000 else "m3" if ago < 720_000 else "m4" if ago < 86_400_000 else "none"


def cluster_order(fleet):
    """The instances in PLACEMENT_ORDER, by the Python restatement: used to AIM the engineered rows (which instance is a model's
    first candidate); the expected outputs come from the reference."""
    from oracle import py_oracle as po
    return po.Mesh(fleet.min_space_units, fleet.min_churn_age_ms, fleet.now).sorted_cluster_state(py_pods(fleet))


def py_pods(fleet):
    """The instance table as oracle/py_oracle.py takes it."""
    return [dict(lru_time=int(r["lru_time"]), capacity=int(r["capacity"]), used=int(r["used"]), version=int(r["version"]), count=int(r["count"]),
                 loading_threads=int(r["loading_threads"]), loading_in_progress=int(r["loading_in_progress"]), rpm=int(r["rpm"]),
                 id_order=int(r["id_order"]), replica_set=int(r["replica_set"]), shutting_down=bool(r["flags"] & 5)) for r in fleet.pods]


def _set_types(fleet, allowed, prefer):
    """Per type row the instances it may be placed on / prefers (None: no such set)."""
    T, P = len(allowed), fleet.n_pods
    al, pf = np.ones((T, P), bool), np.zeros((T, P), bool)
    for t in range(T):
        if allowed[t] is not None:
            al[t] = np.isin(np.arange(P), list(allowed[t]))
        if prefer[t] is not None:
            pf[t] = np.isin(np.arange(P), list(prefer[t]))
    fleet.n_types = T
    fleet.allowed, fleet.prefer = wl.bitmap_from_bool(al), wl.bitmap_from_bool(pf)
    fleet.has_allowed = np.array([a is not None for a in allowed], np.uint8)
    fleet.has_prefer = np.array([p is not None for p in prefer], np.uint8)


class _PlaceRows:
    """Load-target requests of one case.  A row's fresh record is the table's row of its caller (a stand-in for a caller that is
    not in the table) unless the keywords lru / capacity / used / count / rpm move a field; ago: lastUsedAgo (a day and more by
    default: the rpm rule filters nothing)."""

    def __init__(self, fleet, seed):
        self.fleet, self.rng = fleet, np.random.default_rng(0x91ACE + seed)
        self.rows, self.extra, self.pairs = [], [], []

    def add(self, model, self_pod=-1, favour=0, pick=None, ago=100_000_000, last_used=None, extra=(), **fresh):
        f = self.fleet
        q = np.zeros(1, dtype=_lib.PLACE_REQ)
        q["model"], q["self_pod"], q["flags"] = model, self_pod, favour
        q["pick"] = int(self.rng.integers(0, 2**32)) if pick is None else pick
        q["last_used"] = f.now - ago if last_used is None else last_used
        q["extra_off"], q["n_extra"] = len(self.extra), len(extra)
        self.extra += [int(p) for p in extra]
        if self_pod >= 0:
            cur = f.pods[self_pod]
            vals = dict(lru=cur["lru_time"], capacity=cur["capacity"], used=cur["used"], count=cur["count"], rpm=cur["rpm"])
        else:
            vals = dict(lru=f.now - 1_000_000, capacity=1_000_000, used=500_000, count=5, rpm=0)
        vals.update(fresh)
        q["fresh_lru"], q["fresh_capacity"], q["fresh_used"] = vals["lru"], vals["capacity"], vals["used"]
        q["fresh_count"], q["fresh_rpm"] = vals["count"], vals["rpm"]
        self.rows.append(q)
        return len(self.rows) - 1

    def pair(self, inside, outside, offset=0):
        self.pairs.append((inside, outside, offset))

    def done(self):
        return np.concatenate(self.rows), np.array(self.extra, np.int32)


def _one_caller(rows, self_pod, **fresh):
    """The same requests as ONE instance's batch: every row carries this caller and its fresh record."""
    for q in rows.rows:
        q["self_pod"], q["flags"] = self_pod, 0
        q["fresh_lru"], q["fresh_capacity"], q["fresh_used"] = fresh["lru"], fresh["capacity"], fresh["used"]
        q["fresh_count"], q["fresh_rpm"] = fresh["count"], fresh["rpm"]


def _age(now, t):
    return 0 if t == 0 else now - t


def _tdiv(a, b):
    return abs(a) // b * (1 if a >= 0 else -1)  # Java's '/': toward zero


def _breaks_full_case(P, seed, typed, future=False, zero_oldest=False, caller=False, mixed=False):
    """Every instance full: the LRU break (:4913-4917) and case (b)'s window (:4864).  Instances are named by their role; a model
    whose copies are the instances in front of X in the order has X as its first candidate.  mixed: a sixth of the instances are
    NOT full and no type may use them — the same walks, on a table that is no full cluster (the device picks its kernels by that)."""
    fleet, rng = _edge_fleet(P, seed)
    now = fleet.now
    pods = fleet.pods
    pods["used"] = pods["capacity"] - rng.integers(0, fleet.min_space_units, P)
    perm = [int(p) for p in rng.permutation(P)]
    Y = now - 440_000  # age / 10 and age / 4 below 45 000 and 120 000 from here on
    lru = [now - 3_000_007, now - 3_000_007 + 1_001, now - 3_000_007 + 2_002, Y, Y + 1_000, Y + 1_001]
    O0, O1, O2, Y5, Y6, Y7 = perm[:6]
    k = 6
    gaps = []
    if typed:  # instances exactly at, and one millisecond behind, the end of case (b)'s window of Y5 and of O1
        q = _tdiv(now - lru[1], 4)
        assert q > 120_000 and (now - lru[1]) % 4
        lru += [Y + 120_000, Y + 120_001, lru[1] + q, lru[1] + q + 1]
        gaps = perm[6:10]
        k = 10
    step = max(1, 100_000 // P)
    lru += [Y + 2_000 + i * step for i in range(P - k)]
    pods["lru_time"][perm] = lru
    if zero_oldest:
        pods["lru_time"][O0] = 0  # age(0) is 0 (:4162-4164)
    if future:  # the call's `now` lies before every lruTime: negative ages
        fleet.now = now = int(pods["lru_time"].min()) - 95
    open_pods = set(p for p in perm[k + 5::6] if p != perm[-1]) if mixed else set()
    pods["used"][sorted(open_pods)] = 500_000
    # counts that do not decrease along the order (full instances stand in lruTime order): the device keeps its per-type head
    # windows, and the shortlists it records from them at commit, only for such a table
    pods["count"][np.argsort(pods["lru_time"], kind="stable")] = 40 + np.arange(P) // 4
    pods["count"][sorted(open_pods)] = 1 + np.arange(len(open_pods))
    ids = string_ids(fleet, 400 + seed)
    order = cluster_order(fleet)
    assert set(order[:len(open_pods)]) == open_pods
    order = order[len(open_pods):]  # the full instances: all a type may use
    pos = {p: i for i, p in enumerate(order)}
    assert [pos[p] for p in (O0, O1, O2)] == [0, 1, 2] and pos[Y5] < pos[Y6] < pos[Y7] == pos[Y6] + 1
    far = order[-1]
    firsts = [O0, O1, O2, Y5, Y6, Y7] + ([order[pos[Y7] + 1]] if P > 8 else [])
    allowed, prefer = [None], [None]
    if typed:
        sub = sorted((set(firsts) | set(gaps) | {far} | set(int(p) for p in rng.choice(P, P // 2, replace=False))) - open_pods)
        if mixed:
            allowed, every = [list(order)], list(order)
        else:
            every = None
        # (the last two: types whose FIRST instance is Y6 / Y7 — what the device records per type at commit starts there)
        allowed += [sub, every, every, every, every, [order[-2], order[-3]], order[pos[Y6]:], order[pos[Y7]:]]
        prefer += [None, [gaps[0]], [gaps[1]], [gaps[2]], [gaps[3]], None, None, None]
        _set_types(fleet, allowed, prefer)
    specs, first_of, kind = [], [], []
    for t in range(2 if typed else 1):
        for b in firsts:
            specs.append((t, order[:pos[b]], []))
            first_of.append(b)
            kind.append("simple")
    if typed:
        for t, b in ((2, Y5), (3, Y5), (4, O1), (5, O1)):
            specs.append((t, order[:pos[b]], []))
            first_of.append(b)
            kind.append("b")
        specs.append((6, [order[-2]], [order[-3]]))  # every instance of its type holds or failed it: no candidate
        first_of.append(None)
        kind.append("none")
        for t, b in ((7, Y6), (8, Y7)):
            specs.append((t, [], []))
            first_of.append(b)
            kind.append("simple")
    _set_models(fleet, specs)
    rows = _PlaceRows(fleet, seed)
    T_of = {}
    for m, b in enumerate(first_of):
        if b is None:
            rows.add(m)
            rows.add(m, self_pod=far, favour=1)
            continue
        oldest = int(pods["lru_time"][b])
        T_of[m] = thr = max(45_000, _tdiv(_age(now, oldest), 10))
        elig = [p for p in order[pos[b] + 1:] if allowed[specs[m][0]] is None or p in allowed[specs[m][0]]]
        assert len(elig) >= 2 and elig[-1] == far
        if kind[m] == "b":
            rows.add(m, lru=oldest)
            rows.add(m, lru=oldest + thr + 1)
            rows.add(m, self_pod=gaps[specs[m][0] - 2], favour=1)
            rows.add(m, self_pod=gaps[specs[m][0] - 2], favour=0)
            continue
        for sp in (-1, far, elig[0]):
            for fav in (0, 1):
                i = [rows.add(m, self_pod=sp, favour=fav, lru=oldest + thr + d) for d in (-1, 0, 1)]
                if fav == 0:
                    rows.pair(i[1], i[2])
        rows.add(m, self_pod=b, favour=1)
        rows.add(m, self_pod=b, favour=0, lru=oldest + 50_000)
        rows.add(m, self_pod=b, favour=0, lru=oldest - 50_000, extra=[elig[0]])
    if typed:  # case (b): the preferred instance at the window's last millisecond / one behind it
        nb = len(firsts) * 2
        base = {m: None for m in range(nb, nb + 4)}
        for i, q in enumerate(rows.rows):
            m = int(q["model"][0])
            if m in base and base[m] is None:
                base[m] = i  # the model's first row: no caller, the fresh row at `oldest`
        rows.pair(base[nb], base[nb + 1])
        rows.pair(base[nb + 2], base[nb + 3])
    if caller:  # one caller: the fresh lruTime 45 001 ms behind Y6's and 45 000 behind Y7's
        for m in range(len(first_of)):
            if first_of[m] is not None:
                for _ in range(3):
                    rows.add(m)
        cur = pods[far]
        _one_caller(rows, far, lru=int(pods["lru_time"][Y6]) + 45_001, capacity=cur["capacity"], used=cur["used"], count=cur["count"], rpm=0)
        assert T_of[firsts.index(Y6)] == T_of[firsts.index(Y7)] == 45_000
        rows.pairs = []
        for t in range(2 if typed else 1):
            a, b = (t * len(firsts) + firsts.index(x) for x in (Y7, Y6))
            ia, ib = (next(i for i, q in enumerate(rows.rows) if q["model"][0] == m) for m in (a, b))
            rows.pair(ia, ib, -1)
        if typed:  # ... and as their types' first instances, nothing excluded
            ia, ib = (next(i for i, q in enumerate(rows.rows) if q["model"][0] == m) for m in (len(specs) - 1, len(specs) - 2))
            rows.pair(ia, ib, -1)
    return fleet, ids, rows


OPEN_COUNTS = (7, 8, 9, 10, 10, 11, 11, 11, 12, 12, 40, 50, 51, 52, 62, 63, 64, 65, 66)
FRESH_COUNTS = (7, 8, 9, 10, 40, 41, 50, 51, 52, 1_717_986_918, 1_717_986_919, INT_MAX)


def _breaks_open_case(P, seed, typed, caller=False):
    """Nothing full in front: the remaining-space break (:4922), the count break (:4926) inside and beyond the device's table of
    thresholds, case (a) with the caller behind the preferred instance (its row is judged by the FIRST entry's record, :4909)."""
    fleet, rng = _edge_fleet(P, seed)
    now, pods, msu = fleet.now, fleet.pods, fleet.min_space_units
    perm = [int(p) for p in rng.permutation(P)]
    role = {}

    def put(name, count, rem):
        p = perm[len(role)]
        role[name] = p
        pods["capacity"][p], pods["used"][p], pods["count"][p] = 1_000_000, 1_000_000 - rem, count
        return p
    put("S1", 1, 20_000)  # a quarter of their space lies below min_space: the full rule decides
    put("S2", 2, 20_001)
    for j in range(5):
        put(f"Q{j}", 3, 400_000 + j)  # remaining % 4 = 0 ... 3, and the next multiple
    for j, c in enumerate(OPEN_COUNTS):
        put(f"C{c}_{j}", c, 300_000 - j)
    put("Bp", 13, 80_004)
    for c in (14, 15, 16, 17):
        put(f"P{c}", c, 300_000)
    n_role = len(role)
    for p in perm[n_role:]:
        pods["capacity"][p], pods["count"][p] = 1_000_000, int(rng.integers(18, 40))
        pods["used"][p] = 1_000_000 - int(rng.integers(250_000, 350_000))
    # behind them: a full instance, and one whose `used` exceeds its capacity (getRemaining clamps to 0)
    pods["used"][perm[-1]] = pods["capacity"][perm[-1]] + 7
    pods["used"][perm[-2]] = pods["capacity"][perm[-2]] - msu + 1
    pods["count"][perm[-2:]] = 100  # (counts do not decrease along the order: the device keeps its head windows for such a table)
    ids = string_ids(fleet, 420 + seed)
    order = cluster_order(fleet)
    pos = {p: i for i, p in enumerate(order)}
    assert set(order[-2:]) == set(perm[-2:]) and [pos[role[x]] for x in ("S1", "S2")] == [0, 1]
    assert [order[2 + j] for j in range(5)] == [role[f"Q{4 - j}"] for j in range(5)]
    pref = [role[x] for x in ("Bp", "P14", "P15", "P16", "P17")]
    allowed, prefer = [None], [None]
    if typed:
        sub = sorted(set(role.values()) | set(int(p) for p in rng.choice(P, P // 2, replace=False)))
        # (the last two: types whose FIRST instance is Q4 / Q3 — what the device records per type at commit starts there)
        allowed += [sub, None, [perm[-3], perm[-4]], order[pos[role["Q4"]]:], order[pos[role["Q3"]]:]]
        prefer += [None, pref, None, None, None]
        _set_types(fleet, allowed, prefer)
    firsts = ["S1", "S2", "Q4", "Q3", "Q2", "Q1", "Q0"] + [f"C{c}_{j}" for j, c in enumerate(OPEN_COUNTS) if c not in OPEN_COUNTS[:j]][:10]
    specs, first_of = [], []
    for t in range(2 if typed else 1):
        for x in firsts:
            specs.append((t, order[:pos[role[x]]], []))
            first_of.append(x)
    if typed:
        specs += [(2, [], []), (2, [role["S1"]], []), (3, [perm[-3]], [perm[-4]]), (2, pref, [])]  # the last: no preferred instance left
        first_of += ["a:S1", "a:S2", None, "S1"]
        specs += [(4, [], []), (5, [], [])]
        first_of += ["Q4", "Q3"]
    _set_models(fleet, specs)
    rows = _PlaceRows(fleet, seed)
    far = order[-3]
    by_first = {}
    for m, x in enumerate(first_of):
        if x is None:
            rows.add(m)
            rows.add(m, self_pod=far, favour=1)
            continue
        if x.startswith("a:"):  # case (a): Bp becomes the best instance
            q = max(msu, (1_000_000 - int(pods["used"][role["Bp"]])) >> 2)
            i = [rows.add(m, self_pod=role["P15"], favour=0, used=1_000_000 - 300_000) for _ in range(2)]
            by_first[x] = i[0]
            j = [rows.add(m, used=1_000_000 - (q + d)) for d in (-1, 0, 1)]
            rows.pair(j[1], j[0])
            rows.add(m, self_pod=role["Bp"], favour=1)
            rows.add(m, self_pod=role["P16"], favour=1)
            continue
        b = role[x]
        b_rem = 1_000_000 - int(pods["used"][b])
        q = max(msu, b_rem >> 2)
        for sp in (-1, far):
            i = [rows.add(m, self_pod=sp, used=1_000_000 - (q + d)) for d in (-1, 0, 1)]
            rows.pair(i[1], i[0])
        i = [rows.add(m, used=1_000_000 - msu), rows.add(m, used=1_000_000 + 5), rows.add(m, used=LONG_MAX)]
        if q == msu:
            rows.pair(i[0], i[1])  # capacity - used <= 0: clamped to 0, full
        by_first.setdefault(x.split("_")[0], rows.add(m, used=500_000))
        rows.add(m, self_pod=b, favour=1)
        rows.add(m, self_pod=far, favour=1, used=500_000)
        if x.startswith("C"):  # the caller is the first candidate: firstCount is its FRESH count
            i = [rows.add(m, self_pod=b, count=c) for c in FRESH_COUNTS]
            if x == "C7_0":
                for a, o in zip(i[:-2], i[1:-1]):  # (the last two both wrap)
                    rows.pair(a, o)
    for a, o in ((7, 8), (8, 9), (9, 10), (50, 51), (51, 52)):  # ... and through the table's rows
        rows.pair(by_first[f"C{a}"], by_first[f"C{o}"], 1)  # (the next first instance stands one position behind)
    if typed:
        rows.pair(by_first["a:S2"], by_first["a:S1"])  # the caller behind Bp breaks on S1's remaining space, not on S2's
    if caller:  # one caller with 100 000 units left: a quarter of Q3's space, one short of a quarter of Q4's
        for m in range(len(first_of)):
            for _ in range(3):
                rows.add(m)
        cur = pods[far]
        _one_caller(rows, far, lru=cur["lru_time"], capacity=1_000_000, used=900_000, count=cur["count"], rpm=0)
        rows.pairs = []
        for t in range(2 if typed else 1):
            a, b = (t * len(firsts) + firsts.index(x) for x in ("Q3", "Q4"))
            ia, ib = (next(i for i, q in enumerate(rows.rows) if q["model"][0] == m) for m in (a, b))
            rows.pair(ia, ib, -1)
        if typed:  # ... and as their types' first instances, nothing excluded
            ia, ib = (next(i for i, q in enumerate(rows.rows) if q["model"][0] == m) for m in (len(specs) - 1, len(specs) - 2))
            rows.pair(ia, ib, -1)
    return fleet, ids, rows


AGO_EDGES = (-1_001, -1_000, 4_999, 5_000, 719_999, 720_000, 86_399_999, 86_400_000, 431_999_999, 432_000_000)
MIN_LOADS = (50, 101, 109, 110, 1_000)  # the table's rpm of the first candidate: min_load 100 (from below), 101, ...
WRAP_LOADS = (2**29 - 1, 2**29, 715_827_882, 715_827_883, 2**30 - 1, 2**30, INT_MAX)
B_RPMS = (100, 111, 151, 301, 401, 99, 100, 101)  # case (b)'s candidates carry their own (:4875)
CLASS_AGO = (-5_000, 0, 10_000, 1_000_000)  # one lastUsedAgo per clause: m11, m15, 3 * min, 4 * min is the strictest that applies


def _rpm_thresholds(min_load):
    m = max(100, min_load)
    return [min(m + m // 10, INT_MAX), min(m + m // 2, INT_MAX), _i32(m * 3), _i32(m * 4)]


def _rpm_case(P, seed, typed, caller=False):
    """Every instance full and as old as the first: the shortlist is everything eligible, and the rpm rule (:4951-4986) decides.  In
    the simple case the list is [the first candidate's rpm, the caller's fresh rpm, ...] (:4909, :4936)."""
    fleet, rng = _edge_fleet(P, seed)
    now, pods = fleet.now, fleet.pods
    pods["used"] = pods["capacity"] - rng.integers(0, fleet.min_space_units, P)
    perm = [int(p) for p in rng.permutation(P)]
    pods["lru_time"][perm] = now - 400_000 + 10 * np.arange(P)
    pods["count"][perm] = 5 + np.arange(P) // 4  # (not decreasing along the order: the device keeps its head windows for such a table)
    head = list(MIN_LOADS) + list(WRAP_LOADS)
    pods["rpm"][perm[:len(head)]] = head
    bp = perm[len(head)]
    Pb = perm[len(head) + 1: len(head) + 1 + len(B_RPMS)]
    pods["rpm"][Pb] = B_RPMS
    Pw = perm[len(head) + 9: len(head) + 13]
    pods["rpm"][Pw] = [2**30, 2**30, 2**30 + 5, 2**30]
    rest = perm[len(head) + 13:]
    ids = string_ids(fleet, 440 + seed)
    order = cluster_order(fleet)
    assert order == perm
    sizes = [n for n in (2, 3, 63, 64, 65) if n <= len(rest)] + ([len(rest)] if len(rest) < 63 else [])
    allowed, prefer = [None], [None]
    if typed:
        allowed += [None, None] + [rest[:n] for n in sizes] + [rest[:2]]
        prefer += [Pb, Pw] + [None] * len(sizes) + [None]
        _set_types(fleet, allowed, prefer)
    specs = [(0, perm[:k], []) for k in range(len(head))]
    if typed:
        specs += [(1, perm[:len(head)], []), (2, perm[:len(head)], [])]
        specs += [(3 + j, [], []) for j in range(len(sizes))]
        specs.append((3 + len(sizes), rest[:1], rest[1:2]))
    _set_models(fleet, specs)
    rows = _PlaceRows(fleet, seed)
    far = perm[-1]

    def lru_of(m):
        return int(pods["lru_time"][perm[m]])
    # lastUsedAgo on either side of every clause's limit; the fresh rpm such that this clause alone decides (min_load 100)
    for f in (111, 200, 350, 401, 100):
        i = [rows.add(0, ago=a, lru=lru_of(0), rpm=f) for a in AGO_EDGES]
        for a, o in ((1, 0), (3, 2), (5, 4), (7, 6)):
            if f == (111, 200, 350, 401)[a // 2]:
                rows.pair(i[a], i[o])
        z = rows.add(0, last_used=0, lru=lru_of(0), rpm=f)  # never used: age(0) == 0, within the 5 s clause
        if f == 200:
            rows.pair(i[3], z)
    # the fresh rpm below, at and above each clause's limit, per min_load
    for m in range(len(MIN_LOADS)):
        th = _rpm_thresholds(MIN_LOADS[m])
        for c in range(4):
            for sp in (-1, far):
                i = [rows.add(m, self_pod=sp, ago=CLASS_AGO[c], lru=lru_of(m), rpm=th[c] + d) for d in (-1, 0, 1)]
                rows.pair(i[1], i[2])
        for f in (99, 100, 101):
            rows.add(m, ago=0, lru=lru_of(m), rpm=f)
        rows.add(m, self_pod=perm[m], favour=1)
        for c in range(4):  # the first candidate alone is filtered
            rows.add(m, ago=CLASS_AGO[c], lru=lru_of(m), rpm=100)
    # min_load where 3 * min and 4 * min wrap and 1.1 * min, 1.5 * min saturate
    wi = {}
    for j, w in enumerate(WRAP_LOADS):
        m = len(MIN_LOADS) + j
        th = _rpm_thresholds(w)
        for c in range(4):
            for f in sorted({w, INT_MAX} | {min(max(t, w), INT_MAX) for t in (th[c] - 1, th[c], th[c] + 1)}):
                wi[(w, c, f)] = rows.add(m, ago=CLASS_AGO[c], lru=lru_of(m), rpm=f, pick=[0, 1, 2**31, 2**32 - 1][(j + c) % 4])
        rows.add(m, ago=90_000_000, lru=lru_of(m), rpm=INT_MAX)
    rows.pair(wi[(2**29 - 1, 3, 2**29 - 1)], wi[(2**29, 3, 2**29)])  # 4 * 2^29 wraps to MIN_VALUE: everything is filtered
    # (3 * min wraps from 715 827 883 on; 4 * min has wrapped by then and applies whenever 3 * min does: those rows are not a pair)
    if typed:
        mb = len(head)
        # case (b): the candidates' own rpm against every lastUsedAgo
        for sp, fav in ((-1, 0), (far, 0), (Pb[2], 0), (Pb[2], 1)):
            i = [rows.add(mb, self_pod=sp, favour=fav, ago=a) for a in AGO_EDGES]
            z = rows.add(mb, self_pod=sp, favour=fav, last_used=0)
            if sp == -1:
                for a, o in ((1, 0), (3, 2), (5, 4), (7, 6)):
                    rows.pair(i[a], i[o])
                rows.pair(i[3], z)
        for a in AGO_EDGES + (-5_000, 0, 10_000):
            for pk in (0, 1, 2**31, 2**32 - 1):
                rows.add(mb + 1, ago=a, pick=pk)  # min_load 2^30: 3 * min wraps, the filter stops at one survivor in mid-list
        for j in range(len(sizes)):  # pick against 2, 3, 63, 64, 65 survivors
            for pk in (0, 1, 2**31, 2**32 - 1):
                first = int(pods["lru_time"][rest[0]])
                rows.add(mb + 2 + j, pick=pk, lru=first, rpm=0)
                rows.add(mb + 2 + j, pick=pk, lru=first, rpm=500, ago=0)
                rows.add(mb + 2 + j, self_pod=rest[1], pick=pk, lru=first, rpm=0)
        rows.add(mb + 2 + len(sizes))
    if caller:  # one caller, fresh rpm 151: the 5 s clause's limit + 1 at min_load 100; lastUsedAgo varies by request
        rows.rows, rows.extra, rows.pairs = [], [], []
        for m in range(len(specs)):
            i = [rows.add(m, ago=a, pick=pk) for a in AGO_EDGES + (0,) for pk in (0, 2**31, 2**32 - 1)]
            z = rows.add(m, last_used=0)
            if m == 0 or (typed and m == len(head)):
                rows.pair(i[3 * 3], i[2 * 3])
                rows.pair(i[3 * 3], z)
        cur = pods[far]
        _one_caller(rows, far, lru=lru_of(0), capacity=cur["capacity"], used=cur["used"], count=cur["count"], rpm=151)
    return fleet, ids, rows


def _order_case(P, seed, after=False, caller=False):
    """PLACEMENT_ORDER's own thresholds (:4649-4701): instances that differ in one key, down to the id; two versions, every full
    instance of which is older than 2 * minChurnAge (the comparator's precondition).  after: the same table with a few rows moved
    across a threshold — what a delta commit re-ranks by insertion.  The counts are laid out per (version, full) band — version 8
    not full 0 ... 19, full 20; version 7 not full 30 ... 49, full 100 — so that they do not decrease along the order: the device
    records its per-type shortlists at commit only for such a table, and the delta commit must rebuild them.  caller: the
    requests are one instance's batch."""
    fleet, rng = _edge_fleet(P, seed)
    now, pods, msu, mc = fleet.now, fleet.pods, fleet.min_space_units, fleet.min_churn_age_ms
    perm = [int(p) for p in rng.permutation(P)]
    pods["version"] = np.where(rng.random(P) < 0.5, 8, 7)
    pods["count"] = 1 + pods["count"] % 19  # the band's offset is added below
    it = iter(perm)

    def put(**kw):
        p = next(it)
        pods["capacity"][p], pods["used"][p], pods["count"][p], pods["lru_time"][p] = 1_000_000, 600_000, 12, now - 2_000_000
        pods["loading_threads"][p], pods["loading_in_progress"][p], pods["rpm"][p], pods["version"][p] = 8, 1, 50, 7
        for k, v in kw.items():
            pods[k][p] = v
        return p
    eng = []
    for v in (7, 8):
        eng += [put(version=v, used=1_000_000 - msu), put(version=v, used=1_000_000 - msu + 1), put(version=v, used=1_000_000 - msu - 1)]
        eng += [put(version=v, used=1_000_000 - msu + 1, lru_time=2 * mc + 1), put(version=v, used=1_000_000 - msu, lru_time=2 * mc),
                put(version=v, used=1_000_000 - msu, lru_time=2 * mc + 1), put(version=v, used=1_000_007), put(version=v, used=1_000_000, count=0)]
        eng += [put(version=v) for _ in range(3)]  # equal in every key: the id decides
        eng += [put(version=v, loading_threads=INT_MAX, loading_in_progress=-1), put(version=v, loading_threads=INT_MIN, loading_in_progress=1),
                put(version=v, loading_threads=0, loading_in_progress=0), put(version=v, loading_threads=INT_MIN + 5, loading_in_progress=INT_MIN),
                put(version=v, loading_threads=INT_MIN + 4, loading_in_progress=INT_MAX)]
        eng += [put(version=v, loading_threads=7, loading_in_progress=0, rpm=r) for r in (INT_MIN, -1, 0, INT_MAX)]
        eng += [put(version=v, capacity=1_000_001, used=600_001), put(version=v, count=11), put(version=v, count=13),
                put(version=v, lru_time=now - 2_000_001)]
    assert len(eng) <= P
    if after:  # a few rows cross a threshold, take another's place, or swap the key that separated them
        a, b, c, d, e = eng[0], eng[1], eng[8], eng[11], eng[16]
        pods["used"][a] += 1
        pods["used"][b] -= 1
        pods["rpm"][c] = INT_MAX
        pods["loading_in_progress"][d] = INT_MAX
        pods["count"][e] = 0
        pods["lru_time"][eng[26]] = 2 * mc + 2
    rem = np.maximum(pods["capacity"] - pods["used"], 0)
    v7 = pods["version"] == 7
    pods["count"] = np.where(rem < msu, np.where(v7, 100, 20), pods["count"] + np.where(v7, 30, 0))
    ids = string_ids(fleet, 460 + seed)
    specs = []
    for _ in range(40):
        k, f = int(rng.integers(0, 4)), int(rng.integers(0, 3))
        ps = rng.choice(P, size=k + f, replace=False)
        specs.append((0, list(ps[:k]), list(ps[k:])))
    specs.append((0, perm[:P // 2], perm[P // 2:]))  # every instance holds or failed it
    _set_models(fleet, specs)
    rows = _PlaceRows(fleet, seed)
    for m in range(len(specs)):
        for sp in (-1, eng[m % len(eng)], perm[-1 - m % 5]):
            for fav in (0, 1):
                rows.add(m, self_pod=sp, favour=fav, ago=[0, 100_000_000][m % 2])
    if caller:  # one caller, not in any list's way; its fresh row has room before the rows move and min_space - 1 after: either recorded list
        _one_caller(rows, perm[-1], lru=now - 2_000_000, capacity=1_000_000, used=1_000_000 - msu + 1 if after else 600_000, count=12, rpm=50)
    return fleet, ids, rows


def _place_edge_cases():
    """(name, fleet, ids, _PlaceRows, caller, after)"""
    yield ("edge_breaks_full8",) + _breaks_full_case(8, 1, False, future=True) + (False, None)
    yield ("edge_breaks_full65",) + _breaks_full_case(65, 2, True, zero_oldest=True) + (False, None)
    yield ("edge_breaks_full200c",) + _breaks_full_case(200, 3, True, caller=True) + (True, None)
    yield ("edge_breaks_full700",) + _breaks_full_case(700, 4, True) + (False, None)
    yield ("edge_breaks_mixed200",) + _breaks_full_case(200, 11, True, mixed=True) + (False, None)
    yield ("edge_breaks_open64",) + _breaks_open_case(64, 5, False) + (False, None)
    yield ("edge_breaks_open200",) + _breaks_open_case(200, 6, True) + (False, None)
    yield ("edge_breaks_open65c",) + _breaks_open_case(65, 7, True, caller=True) + (True, None)
    yield ("edge_rpm_64",) + _rpm_case(64, 8, False) + (False, None)
    yield ("edge_rpm_200",) + _rpm_case(200, 9, True) + (False, None)
    yield ("edge_rpm_65c",) + _rpm_case(65, 10, True, caller=True) + (True, None)
    for P, seed, c in ((65, 12, True), (200, 14, False)):
        tag = f"{P}c" if c else f"{P}"
        yield (f"edge_order_{tag}",) + _order_case(P, seed, caller=c) + (c, f"edge_order_{tag}after")
        yield (f"edge_order_{tag}after",) + _order_case(P, seed, after=True, caller=c) + (c, None)


@functools.lru_cache(maxsize=None)
def _place_edge_all():
    """{name: (fleet, ids, reqs, extra, meta)}, built once; the consumers do not write into it."""
    out = {}
    for name, fleet, ids, rows, caller, after in _place_edge_cases():
        reqs, extra = rows.done()
        out[name] = (fleet, ids, reqs, extra, dict(pairs=list(rows.pairs), caller=caller, after=after))
    return out


def place_edge_cases():
    """(name, fleet, ids, reqs, extra) like place_cases, at the EDGES of getNext's value domain (MM.java:4777-5003); name =
    edge_<tier>_<case>.  breaks: the shortlist's break thresholds one unit inside, on and outside, best full and not full, through the
    caller's fresh row and through the table's rows.  rpm: the filter's age classes, its limits (wrapping and saturating ones
    included), the stop at one survivor, the pick.  order: PLACEMENT_ORDER's thresholds, each table once more after a few rows moved."""
    for name, (fleet, ids, reqs, extra, _) in _place_edge_all().items():
        yield name, fleet, ids, reqs, extra


def _rebalance_fleet(seed, pods, models, used):
    """Fleet where many models have 1-4 copies, often including self_pod = 0 (as tests/test_rebalance_gpu.py builds it)."""
    rng = np.random.default_rng(8000 + seed)
    fleet = wl.fuzz_fleet(seed + 70, pods=pods, models=models)
    now = fleet.now
    p = fleet.pods
    p["flags"] = np.where(rng.random(pods) < 0.05, 1, 2)
    p["flags"][0] = 2
    p["used"] = (p["capacity"] * np.clip(rng.normal(used, 0.02, pods), 0, 1.0)).astype(np.int64)
    p["rpm"] = rng.choice([0, 100, 3000, 9000, 50_000], pods)
    m = fleet.models
    k = rng.choice([0, 1, 1, 2, 2, 3, 4], models).clip(0, pods)
    f = rng.choice([0, 0, 0, 1], models).clip(0, max(pods - 4, 0))
    m["n_loaded"], m["n_failed"] = k, f
    off = np.zeros(models + 1, np.int64)
    np.cumsum(k + f, out=off[1:])
    m["ent_off"] = off[:-1]
    ent = np.zeros(int(off[-1]), np.int32)
    for i in range(models):
        c = rng.choice(pods, size=k[i] + f[i], replace=False)
        if k[i] and rng.random() < 0.7 and 0 not in c:
            c[0] = 0
        ent[off[i]: off[i + 1]] = c
    fleet.ent_pod = ent
    fleet.ent_time = (now - rng.choice([1_000, 25_000, 2_000_000, 90_000_000], len(ent))).astype(np.int64)
    return fleet, rng


def _local_entries(fleet, rng, n):
    e = np.zeros(n, dtype=_lib.CACHE_ENTRY)
    e["model"] = rng.integers(0, fleet.n_models, n)
    e["model"] = np.where(rng.random(n) < 0.03, -1, e["model"])
    e["weight"] = rng.choice([1, 2560, 6400, 60_000], n)
    e["last_used"] = np.where(rng.random(n) < 0.05, 0, fleet.now - rng.choice([500, 30_000, 4_000_000, 50_000_000], n))
    e["interval_count"] = rng.choice([0, 1, 50, 400, 5000], n)
    e["last_heavy_time"] = np.where(rng.random(n) < 0.4, 0, fleet.now - rng.choice([1_000, 700_000, 30_000_000], n))
    e["last_unload_time"] = np.where(rng.random(n) < 0.6, 0, fleet.now - rng.choice([10_000, 100_000], n))
    e["earlier_use_iteration"] = rng.integers(0, 120, n)
    e["last_used_iteration"] = e["earlier_use_iteration"] + rng.integers(0, 60, n)
    e["flags"] = (rng.random(n) < 0.05).astype(np.uint32)
    return e


def scaleup_cases():
    """(name, fleet, ids, entries, params): runs of the rate-tracking task (rateTrackingTask, MM.java:5636-5832) over the local
    cache entries of instance 0 — thresholds and clocks that reach the second-copy rule, the scale-up rule with and without
    overloaded instances, and the early returns."""
    for seed, pods, used in ((0, 12, 0.5), (1, 200, 0.97), (2, 200, 0.2), (3, 1, 0.5)):
        fleet, rng = _rebalance_fleet(seed, pods, 600, used)
        ids = string_ids(fleet, 80 + seed)
        now = fleet.now
        entries = _local_entries(fleet, rng, 800)
        for j, (thr, our_rpm, last_check) in enumerate(((2000, 100, now - 10_000), (100, 50_000, now - 9_000), (0, 0, now - 10_000),
                                                        (2000, 0, now - 1_000))):
            sp = np.zeros(1, dtype=_lib.SCALEUP_PARAMS)
            sp["self_pod"], sp["iteration_counter"] = 0, 130
            sp["second_copy_max_age_iters"], sp["second_copy_min_age_iters"] = 240, 42
            sp["scale_up_rpm_threshold"], sp["our_rpm"] = thr, our_rpm
            sp["now"], sp["last_check_time"], sp["rate_check_interval_ms"] = now, last_check, 10_000
            sp["second_copy_lru_threshold_ms"], sp["assume_completed_ms"] = 72_000_000, 30_000
            yield f"scaleup_{seed}_{j}", fleet, ids, entries, sp


def conc_rows(rng, n):
    """MaxConcCacheEntry state per cache entry (MM.java:2641-2797): countAndTimeSum with counts on both sides of the 64 / 8
    limits of getRpmScaleThreshold (:2769, :2780), with and without prior samples, zero time sums, a few queued requests."""
    c = np.zeros(n, dtype=_lib.CONC_ENTRY)
    count = rng.choice([0, 1, 7, 8, 30, 63, 64, 65, 500, 20_000], n)
    per_call = rng.choice([0, 1, 8, 50, 400, 30_000], n)  # mean duration in 1/10 ms
    c["count_and_time_sum"] = (count * per_call) * (1 << _lib.CONC_COUNT_BITS) + count
    c["prior_count"] = rng.choice([0, 0, 5, 64, 900, -1], n)
    c["prior_sum"] = np.where(c["prior_count"] > 0, c["prior_count"] * rng.choice([0, 2, 60, 500], n), rng.choice([0, 0, 7], n))
    c["max_conc"] = rng.choice([1, 1, 2, 4, 8, 16, 64], n)
    c["queued_requests"] = rng.choice([0, 0, 0, 1, 2, 9], n)
    return c


def scaleup_conc_cases():
    """(name, fleet, ids, entries, conc, params, conc_params): the rate task of a mesh that limits model concurrency (latencyBased,
    MM.java:5677): every entry's threshold is mcce.getRpmScaleThreshold(true) (:5704), averageModelParallelism feeds getExcludeSet
    (:5836) and is recomputed after the loop (:5815-5818)."""
    for seed, pods, used in ((0, 12, 0.5), (1, 200, 0.97), (2, 200, 0.2), (4, 64, 0.9)):
        fleet, rng = _rebalance_fleet(seed, pods, 600, used)
        ids = string_ids(fleet, 80 + seed)
        now = fleet.now
        entries = _local_entries(fleet, rng, 800)
        conc = conc_rows(rng, len(entries))
        for j, (thr, our_rpm, last_check, avg, pct) in enumerate(((2000, 100, now - 10_000, 1.0, 90), (300, 50_000, now - 9_000, 3.75, 90),
                                                                  (2000, 0, now - 1_000, 2.5, 90), (50, 9_000, now - 12_000, 11.3, 50))):
            sp = np.zeros(1, dtype=_lib.SCALEUP_PARAMS)
            sp["self_pod"], sp["iteration_counter"] = 0, 130
            sp["second_copy_max_age_iters"], sp["second_copy_min_age_iters"] = 240, 42
            sp["scale_up_rpm_threshold"], sp["our_rpm"] = thr, our_rpm
            sp["now"], sp["last_check_time"], sp["rate_check_interval_ms"] = now, last_check, 10_000
            sp["second_copy_lru_threshold_ms"], sp["assume_completed_ms"] = 72_000_000, 30_000
            cp = np.zeros(1, dtype=_lib.CONC_PARAMS)
            cp["dynamic_rpm_scale_constant"], cp["average_model_parallelism"] = 600_000 * pct // 100, avg
            yield f"scaleup_conc_{seed}_{j}", fleet, ids, entries, conc, sp, cp


def scaleup_edge_cases():
    """(name, fleet, ids, entries, params): rate-task runs that reach the lines the fleets above do not: no invocations since the
    last check (MM.java:5667-5669), a type confined to a single instance (:5697-5699), a scale-up with nothing overloaded (the
    exclude set stays the model's own instances, :5789)."""
    fleet, rng = _rebalance_fleet(5, 40, 300, 0.5)
    ids = string_ids(fleet, 91)
    now = fleet.now
    sp = np.zeros(1, dtype=_lib.SCALEUP_PARAMS)
    sp["self_pod"], sp["iteration_counter"] = 0, 130
    sp["second_copy_max_age_iters"], sp["second_copy_min_age_iters"] = 240, 42
    sp["scale_up_rpm_threshold"], sp["our_rpm"] = 100, 10**9
    sp["now"], sp["last_check_time"], sp["rate_check_interval_ms"] = now, now - 10_000, 10_000
    sp["second_copy_lru_threshold_ms"], sp["assume_completed_ms"] = 72_000_000, 1_000
    yield "scaleup_edge_empty", fleet, ids, _local_entries(fleet, rng, 0), sp
    # nothing overloaded (our own rpm is far above everyone's), loads old enough, plenty of candidates: scale-ups with an empty exclude set
    f2, rng2 = _rebalance_fleet(6, 60, 300, 0.3)
    f2.ent_time[:] = now - 90_000_000
    e2 = _local_entries(f2, rng2, 400)
    e2["interval_count"] = rng2.choice([400, 5000, 90_000], len(e2))
    yield "scaleup_edge_nothing_overloaded", f2, string_ids(f2, 92), e2, sp
    # type constraints under which one type may only run on instance 0 and another nowhere: typeSetStats(type).instanceCount < 2
    f3, rng3 = _rebalance_fleet(7, 30, 200, 0.4)
    T = 3
    al = np.ones((T, f3.n_pods), bool)
    al[1, 1:] = False
    al[2, :] = False
    f3.n_types = T
    f3.allowed, f3.prefer = wl.bitmap_from_bool(al), wl.bitmap_from_bool(np.zeros((T, f3.n_pods), bool))
    f3.has_allowed, f3.has_prefer = np.array([0, 1, 1], np.uint8), np.zeros(T, np.uint8)
    f3.models["type"] = rng3.integers(0, T, f3.n_models)
    yield "scaleup_edge_confined_types", f3, string_ids(f3, 93), _local_entries(f3, rng3, 300), sp


def scaledown_conc_cases():
    """(name, fleet, ids, entries, conc, params, dyn_const): janitor passes over MaxConcCacheEntry candidates (MM.java:6294-6305): the
    threshold of a model with three or more copies is mcce.getRpmScaleThreshold(false), a copy with queued requests stays."""
    for seed, pods, used in ((1, 200, 0.97), (4, 300, 0.99)):
        fleet, rng = _rebalance_fleet(seed, pods, 600, used)
        ids = string_ids(fleet, 80 + seed)
        now = fleet.now
        entries = _local_entries(fleet, rng, 800)
        entries["last_heavy_time"] = np.where(rng.random(len(entries)) < 0.5, 0, entries["last_heavy_time"])
        fleet.ent_time[:] = now - 90_000_000  # no copy loaded within the last 30 minutes (:6269)
        conc = conc_rows(rng, len(entries))
        for j, (thr, cap, pct) in enumerate(((2000, 10_000_000, 90), (10, 10_000_000, 10))):
            dp = np.zeros(1, dtype=_lib.SCALEDOWN_PARAMS)
            dp["self_pod"], dp["shutting_down"], dp["now"] = 0, 0, now
            dp["last_check_time"], dp["rate_check_interval_ms"] = now - 7_000, 10_000
            dp["adjusted_cache_capacity"], dp["scale_up_rpm_threshold"] = cap, thr
            yield f"scaledown_conc_{seed}_{j}", fleet, ids, entries, conc, dp, 600_000 * pct // 100


def scaledown_edge_cases():
    """(name, fleet, ids, entries, params): the sample period too small to judge a model's load (MM.java:6286-6289), and this
    instance shutting down / not in the table when a second copy is old enough to go (removeSecondModelCopy, :6322-6324)."""
    for k, (self_flags, last_check_ago) in enumerate(((2, 500), (1, 7_000), (4, 7_000))):
        fleet, rng = _rebalance_fleet(4, 300, 600, 0.99)
        fleet.pods["flags"][0] = self_flags
        if k:  # without type constraints instanceSetStats() stays the cluster's when this instance is not in clusterState (:1446-1448)
            fleet.n_types, fleet.allowed, fleet.prefer, fleet.has_allowed, fleet.has_prefer = 0, None, None, None, None
            fleet.models["type"] = 0
        fleet.ent_time[:] = fleet.now - 90_000_000
        entries = _local_entries(fleet, rng, 800)
        entries["last_heavy_time"] = 0
        dp = np.zeros(1, dtype=_lib.SCALEDOWN_PARAMS)
        dp["self_pod"], dp["shutting_down"], dp["now"] = 0, 0, fleet.now
        dp["last_check_time"], dp["rate_check_interval_ms"] = fleet.now - last_check_ago, 10_000
        dp["adjusted_cache_capacity"], dp["scale_up_rpm_threshold"] = 10_000_000, 2000
        yield f"scaledown_edge_{k}", fleet, string_ids(fleet, 95 + k), entries, dp


def scaledown_cases():
    """(name, fleet, ids, entries, params): janitor passes over scaleCopiesCandidates (MM.java:6110-6140 -> removeModelCopies
    :6197-6310 -> removeSecondModelCopy :6314-6335) for the local cache entries of instance 0."""
    for seed, pods, used in ((0, 12, 0.5), (1, 200, 0.97), (2, 200, 0.2), (3, 1, 0.5), (4, 300, 0.99)):
        fleet, rng = _rebalance_fleet(seed, pods, 600, used)
        ids = string_ids(fleet, 80 + seed)
        now = fleet.now
        entries = _local_entries(fleet, rng, 800)
        for j, (thr, cap, sd) in enumerate(((2000, 200_000, 0), (2000, 1_000, 0), (10, 10_000_000, 0), (2000, 200_000, 1))):
            dp = np.zeros(1, dtype=_lib.SCALEDOWN_PARAMS)
            dp["self_pod"], dp["shutting_down"], dp["now"] = 0, sd, now
            dp["last_check_time"], dp["rate_check_interval_ms"] = now - 7_000, 10_000
            dp["adjusted_cache_capacity"], dp["scale_up_rpm_threshold"] = cap, thr
            yield f"scaledown_{seed}_{j}", fleet, ids, entries, dp


def _plan_fleet(seed, pods, models, used_frac, dup_frac=0.3):
    """Mostly unloaded models, many sharing a lastUsed value (the reaper's TreeSet keeps the first of them); instances with
    and without loading capacity (as tests/test_rebalance_gpu.py builds it)."""
    rng = np.random.default_rng(7000 + seed)
    fleet = wl.fuzz_fleet(seed, pods=pods, models=models)
    now = fleet.now
    p = fleet.pods
    p["flags"] = np.where(rng.random(pods) < 0.05, 1, 2)  # a few shutting down
    p["capacity"] = rng.choice([131072, 1_000_000], pods)
    p["used"] = (p["capacity"] * np.clip(rng.normal(used_frac, 0.1, pods), 0, 1.02)).astype(np.int64)
    p["loading_threads"] = rng.choice([0, 1, 8], pods)
    p["loading_in_progress"] = rng.choice([0, 1, 60, 500], pods)
    p["count"] = rng.integers(0, 40, pods)
    p["lru_time"] = np.where(p["count"] == 0, 2**63 - 1, now - rng.integers(1_000, 50_000_000, pods))
    m = fleet.models
    unloaded = rng.random(models) < 0.8
    m["n_loaded"] = np.where(unloaded, 0, m["n_loaded"])
    m["n_failed"] = np.where(rng.random(models) < 0.1, 2, np.minimum(m["n_failed"], 1))
    lu = now - rng.integers(1_000, 60_000_000, models)
    dup = rng.random(models) < dup_frac
    lu = np.where(dup, now - rng.choice([5_000, 900_000, 30_000_000], models), lu)
    m["last_used"] = lu
    m["n_loaded"] = np.minimum(m["n_loaded"], max(pods - 2, 0))
    tot = m["n_loaded"] + m["n_failed"]
    off = np.zeros(models + 1, np.int64)
    np.cumsum(tot, out=off[1:])
    m["ent_off"] = off[:-1]
    # instanceIds / loadFailedInstanceIds are MAPS keyed by the instance id: a model's entries name distinct instances
    ent = np.zeros(int(off[-1]), np.int32)
    for i in np.flatnonzero(tot):
        ent[off[i]: off[i + 1]] = rng.choice(pods, size=int(tot[i]), replace=False)
    fleet.ent_pod = ent
    fleet.ent_time = (now - rng.integers(1_000, 1_000_000, int(off[-1]))).astype(np.int64)
    return fleet


def proactive_cases():
    """(name, fleet, ids, defaultModelSizeUnits, partitioned): one run of the leader's reaper as far as proactive loading goes
    (MM.java:6456-6490, :6574-6577, :6616-6747); partitioned: with type constraints, one pass per ProhibitedTypeSet partition."""
    from modelmesh_amd.solver import bitmap_from_bool
    for seed, pods, models, used in ((0, 8, 300, 0.5), (1, 64, 3000, 0.2), (2, 300, 12000, 0.9), (3, 300, 12000, 0.99), (5, 5, 50, 0.0)):
        fleet = _plan_fleet(seed, pods, models, used)
        ids = string_ids(fleet, 90 + seed)
        for units in (6400, 1):
            yield f"proactive_{seed}_{units}", fleet, ids, units, False
    for seed, total_copies in ((6, 2), (7, 8)):  # modelCopyCount < 3: defaultModelSizeUnits; <= 10: averaged with it (:6622-6629)
        fleet = _plan_fleet(seed, 6, 400, 0.3)
        fleet.pods["flags"] = 2
        fleet.pods["count"] = 0
        fleet.pods["count"][:2] = [total_copies // 2, total_copies - total_copies // 2]
        fleet.pods["lru_time"] = np.where(fleet.pods["count"] == 0, 2**63 - 1, fleet.pods["lru_time"])
        for units in (6400, 100):
            yield f"proactive_{seed}_{units}", fleet, string_ids(fleet, 90 + seed), units, False
    for seed in (0, 1, 2):
        fleet = _plan_fleet(seed + 20, 300, 6000, [0.5, 0.9, 0.2][seed])
        if not fleet.n_types:
            rng = np.random.default_rng(seed)
            fleet.n_types = 3
            al = rng.random((3, fleet.n_pods)) < np.array([[1.0], [0.4], [0.7]])
            fleet.allowed, fleet.prefer = bitmap_from_bool(al), bitmap_from_bool(np.zeros_like(al))
            fleet.has_allowed, fleet.has_prefer = np.array([0, 1, 1], np.uint8), np.zeros(3, np.uint8)
            fleet.models["type"] = rng.integers(0, 3, fleet.n_models)
        yield f"proactive_parts_{seed}", fleet, string_ids(fleet, 95 + seed), 6400, True


REBALANCE_EDGE_TIERS = ("rate", "janitor", "plan")
LOAD_AGO = 45_000_000  # a copy loaded long ago (older than every cutoff of the rebalancers)
ITER, MAX_AGE_ITERS, MIN_AGE_ITERS = 1000, 240, 42  # lower = 760, upper = 958: inside the entries' range
RATE_THR = 2001  # * 3 is no multiple of 4: heavy = 1500


class _RebRows:
    """The cache entries of one run with the registry behind them: a registry row per entry unless `model=` names an earlier one.
    loaded / failed: instances or (instance, time) pairs; the lists are stored in instance-id order, each time with its instance.
    pairs: [(row a, row b, the engineered field or None)]: the reference must answer the two rows differently."""

    def __init__(self, fleet):
        self.fleet, self.models, self.ent, self.rows, self.conc, self.pairs = fleet, [], [], [], [], []

    def model(self, loaded, failed=(), type=0, last_used=None):
        rank, old = self.fleet.pods["id_order"], self.fleet.now - LOAD_AGO
        norm = lambda xs: sorted(((int(x), old) if np.ndim(x) == 0 else (int(x[0]), int(x[1])) for x in xs), key=lambda x: rank[x[0]])  # noqa: E731
        lp, fp = norm(loaded), norm(failed)
        assert len({p for p, _ in lp}) == len(lp) and len({p for p, _ in fp}) == len(fp)
        self.models.append((type, len(self.ent), len(lp), len(fp), self.fleet.now - 5_000 if last_used is None else last_used))
        self.ent += lp + fp
        return len(self.models) - 1

    def add(self, loaded=(), failed=(), type=0, model=None, conc=None, **fields):
        e = np.zeros(1, dtype=_lib.CACHE_ENTRY)
        e["model"] = self.model(loaded, failed, type) if model is None else model
        e["weight"], e["last_used"] = 6400, self.fleet.now - 4_000_000
        for k, v in fields.items():
            e[k] = v
        c = np.zeros(1, dtype=_lib.CONC_ENTRY)
        c["max_conc"] = 1
        for k, v in (conc or {}).items():
            c[k] = v
        self.rows.append(e)
        self.conc.append(c)
        return len(self.rows) - 1

    def both(self, field, a, b, **kw):
        """Two rows that differ in `field` alone (a, then b), as a pair."""
        i = self.add(**{**kw, field: a})
        j = self.add(**{**kw, field: b})
        self.pairs.append((i, j, field))
        return i, j

    def both_conc(self, field, a, b, conc, **kw):
        i = self.add(conc={**conc, field: a}, **kw)
        j = self.add(conc={**conc, field: b}, **kw)
        self.pairs.append((i, j, "conc." + field))
        return i, j

    def pad(self, n, **kw):
        """Plain rows up to n entries on the first registry rows (the 256-thread blocks of the per-entry kernels)."""
        k = 0
        while len(self.rows) < n:
            self.add(model=k % len(self.models), interval_count=k % 7, **kw)
            k += 1
        assert len(self.rows) == n and len(self.models) <= 600

    def done(self):
        f = self.fleet
        f.models = np.array(self.models, dtype=_lib.MODEL_ROW) if self.models else np.zeros(0, _lib.MODEL_ROW)
        f.ent_pod = np.array([p for p, _ in self.ent], np.int32)
        f.ent_time = np.array([t for _, t in self.ent], np.int64)
        return np.concatenate(self.rows), np.concatenate(self.conc)


def _scaleup_params(fleet, thr=RATE_THR, our_rpm=0, delta=60_000, lru_thr=72_000_000, self_pod=0):
    """One run of the rate task: timeDelta 60 000 makes an entry's rpm its interval count."""
    sp = np.zeros(1, dtype=_lib.SCALEUP_PARAMS)
    sp["self_pod"], sp["iteration_counter"] = self_pod, ITER
    sp["second_copy_max_age_iters"], sp["second_copy_min_age_iters"] = MAX_AGE_ITERS, MIN_AGE_ITERS
    sp["scale_up_rpm_threshold"], sp["our_rpm"] = thr, our_rpm
    sp["now"], sp["last_check_time"], sp["rate_check_interval_ms"] = fleet.now, fleet.now - delta, 10_000
    sp["second_copy_lru_threshold_ms"], sp["assume_completed_ms"] = lru_thr, 30_000
    return sp


def _conc_params(dyn=540_000, avg=1.0):
    cp = np.zeros(1, dtype=_lib.CONC_PARAMS)
    cp["dynamic_rpm_scale_constant"], cp["average_model_parallelism"] = dyn, avg
    return cp


def _roomy(fleet):
    """Every instance half empty, old and quiet: the second-copy rule's fullness clause holds, nobody is overloaded."""
    p = fleet.pods
    p["capacity"], p["used"], p["rpm"] = 1_000_000, 500_000, 0
    p["lru_time"] = fleet.now - 3_000_000


def _window_rows(R, others, type=0, **kw):
    """The second-copy window (:5737-5744) on models with one copy, here: every edge of i1 / i2 against lower / upper."""
    lo, up = ITER - MAX_AGE_ITERS, ITER - MIN_AGE_ITERS
    one = dict(loaded=[0], type=type, **kw)
    R.both("last_used_iteration", lo - 1, lo, earlier_use_iteration=lo - 5, **one)
    R.both("earlier_use_iteration", up, up + 1, last_used_iteration=up + 3, **one)
    R.both("earlier_use_iteration", lo - 1, lo, last_used_iteration=up + 3, **one)
    R.both("last_used_iteration", up, up + 1, earlier_use_iteration=lo - 5, **one)
    combos = [R.add(earlier_use_iteration=a, last_used_iteration=b, **one) for a in (lo + 1, lo - 1) for b in (up - 1, up + 1)]
    R.pairs += [(combos[0], combos[3], None), (combos[1], combos[3], None), (combos[2], combos[3], None), (combos[0], combos[1], None)]
    # two copies: the rule is not applied, the markers stay
    two = R.add(loaded=[0, others[0]], type=type, earlier_use_iteration=lo + 1, last_used_iteration=up - 1, **kw)
    R.pairs.append((combos[0], two, None))
    return combos


def _rpm_rows(R, others, thr, type=0, **kw):
    """heavy, scaleUp and the copies asked for, on models with two old copies (the second-copy rule is not reached)."""
    heavy = _i32(thr * 3) // 4
    two = dict(loaded=[0, others[0]], type=type, **kw)
    R.both("interval_count", heavy, heavy + 1, **two)
    R.both("interval_count", thr - 1, thr, **two)
    R.both("interval_count", 2 * thr - 1, 2 * thr, **two)  # rpm / scaleUp 1 / 2 against many candidates
    # ... against exactly two candidates: one below, equal, one above (equal and above are decided alike: no pair)
    n = int(((R.fleet.pods["flags"] & 5) == 0).sum())
    few = dict(loaded=[0, others[0]], failed=others[1:n - 3], type=type, **kw)
    if n >= 6 and not type:
        R.both("interval_count", 2 * thr - 1, 2 * thr, **few)
        R.add(interval_count=3 * thr, **few)


def _loaded_since_rows(R, others, sp, thr):
    """loadedSince (:5860-5871) under the scale-up rule: the newest load on either side of recentLoadCutoff."""
    now = int(sp["now"][0])
    cut = now - (now - int(sp["last_check_time"][0]) + int(sp["rate_check_interval_ms"][0]) + 2 * int(sp["assume_completed_ms"][0]))
    hot = dict(interval_count=thr)
    a = R.add(loaded=[0, (others[0], cut)], **hot)
    b = R.add(loaded=[0, (others[0], cut + 1)], **hot)
    R.pairs.append((a, b, "ent_time"))
    own = R.add(loaded=[(0, cut + 1), others[0]], **hot)  # the caller's own load is ignored
    R.pairs.append((own, b, None))
    fl = R.add(loaded=[0, others[0]], failed=[(others[1], cut + 1)], **hot)  # the failed list is not looked at
    R.pairs.append((fl, b, None))
    if len(others) >= 6:  # a list position >= 4
        last = max(others[:5], key=lambda p: R.fleet.pods["id_order"][p])
        rest = [p for p in others[:5] if p != last]
        assert sum(R.fleet.pods["id_order"][p] < R.fleet.pods["id_order"][last] for p in [0] + rest) >= 4
        a = R.add(loaded=[0] + rest + [(last, cut)], **hot)
        b = R.add(loaded=[0] + rest + [(last, cut + 1)], **hot)
        R.pairs.append((a, b, "ent_time"))


def _rate_plain(P, seed, n_entries, latency=False):
    """No type constraints: window, candidate count, rpm and loadedSince rows on a roomy cluster."""
    fleet, rng = _edge_fleet(P, seed)
    ids = string_ids(fleet, 500 + seed)
    _roomy(fleet)
    others = [int(p) for p in np.argsort(fleet.pods["id_order"]) if p != 0]
    sp = _scaleup_params(fleet)
    R = _RebRows(fleet)
    _window_rows(R, others)
    lo, up = ITER - MAX_AGE_ITERS, ITER - MIN_AGE_ITERS
    # candidateInstCount 0 / 1: suitable - (loaded + failed)
    a = R.add(loaded=[0], failed=others[:P - 1], earlier_use_iteration=lo + 1, last_used_iteration=up - 1)
    b = R.add(loaded=[0], failed=others[:P - 2], earlier_use_iteration=lo + 1, last_used_iteration=up - 1)
    R.pairs.append((a, b, None))
    R.add(model=-1, interval_count=RATE_THR)  # no registry record: heavy only
    R.add(loaded=[], failed=[others[0]], interval_count=RATE_THR)  # no copy anywhere
    _rpm_rows(R, others, RATE_THR)
    _loaded_since_rows(R, others, sp, RATE_THR)
    R.pad(n_entries)
    entries, conc = R.done()
    return fleet, ids, entries, (conc if latency else None), sp, (_conc_params() if latency else None), dict(pairs=R.pairs)


# per-type stats of the fullness / lru case: (instances, what); type t + 1 <-> group t
def _fullness_groups(P):
    return [([1, 2], "10 * tf == tc"), ([3, 4], "10 * tf == tc - 1"), ([5], "one instance"), ([6, 7], "two instances"),
            (list(range(8, 20)), "roomy"), (list(range(20, P)), "full")]


def _rate_typed(P, seed, n_entries, lru_off, latency=False):
    """Type constraints: the fullness clause 10 * tf / tc >= 1 on either side per type, the lru clause on either side per RUN
    (lru_off: secondCopyLruThresholdMillis - (now - globalLru)), a type confined to one instance, a type row outside the table."""
    groups = _fullness_groups(P)
    fleet, rng = _edge_fleet(P, seed, [g for g, _ in groups])
    ids = string_ids(fleet, 510 + seed)
    pods, now = fleet.pods, fleet.now
    pods["capacity"], pods["used"], pods["rpm"] = 1_000_000, 1_000_000, 0  # full everywhere but where a group says otherwise
    pods["lru_time"] = now - rng.integers(400_000, 9_000_000, P)
    pods["lru_time"][9] = now - 10_000_000  # globalLru
    pods["used"][[1, 2]] = 900_000           # tc 2 000 000, tf 200 000
    pods["capacity"][4] = 1_000_001          # tc 2 000 001, tf 200 000
    pods["used"][3], pods["used"][4] = 900_000, 900_001
    pods["used"][5], pods["used"][[6, 7]] = 500_000, 500_000
    pods["used"][8:20] = 500_000
    pods["used"][0] = 500_000
    others = [int(p) for p in np.argsort(pods["id_order"]) if p != 0]
    sp = _scaleup_params(fleet, lru_thr=10_000_000 + lru_off)
    R = _RebRows(fleet)
    lo, up = ITER - MAX_AGE_ITERS, ITER - MIN_AGE_ITERS
    inside = dict(loaded=[0], earlier_use_iteration=lo + 1, last_used_iteration=up - 1)
    row = {what: R.add(type=t + 1, **inside) for t, (_, what) in enumerate(groups)}
    if lru_off >= 0:  # (past the lru threshold every type gets its second copy)
        R.pairs.append((row["10 * tf == tc"], row["10 * tf == tc - 1"], None))
    R.pairs.append((row["one instance"], row["two instances"], None))
    R.pairs.append((row["roomy"], row["full"], None) if lru_off >= 0 else (row["roomy"], row["one instance"], None))
    R.add(type=len(groups) + 5, **inside)  # no such type row: the stats of row 0
    R.add(type=-1, **inside)
    R.add(type=0, **inside)
    _window_rows(R, others, type=5)
    _rpm_rows(R, others, RATE_THR, type=5)
    R.pad(n_entries)
    entries, conc = R.done()
    return fleet, ids, entries, (conc if latency else None), sp, (_conc_params() if latency else None), \
        dict(pairs=R.pairs, lru_rows=[row["10 * tf == tc - 1"], row["full"]])


def _rate_suitable(P, seed, n_entries):
    """copiesToLoad 2 / 3 against suitable / 3 for suitable 6 ... 12 (types confined to groups of that many instances)."""
    sizes, groups, a = list(range(6, 13)), [], 1
    for k in sizes:
        groups.append(list(range(a, a + k)))
        a += k
    assert a <= P
    fleet, rng = _edge_fleet(P, seed, groups)
    ids = string_ids(fleet, 520 + seed)
    _roomy(fleet)
    sp = _scaleup_params(fleet)
    R = _RebRows(fleet)
    three = {}
    for t, g in enumerate(groups):
        R.add(loaded=[0, g[0]], type=t + 1, interval_count=2 * RATE_THR)
        three[len(g)] = R.add(loaded=[0, g[0]], type=t + 1, interval_count=3 * RATE_THR)
        R.add(loaded=[0, g[0]], type=t + 1, interval_count=5 * RATE_THR)
    R.pairs.append((three[8], three[9], None))  # at 8 three copies become two
    R.pad(n_entries)
    entries, conc = R.done()
    return fleet, ids, entries, None, sp, None, dict(pairs=R.pairs, suitable=sizes)


WRAP_DELTAS = (6_000, 10_000, 12_345)


def _rate_wrap(delta, seed=3):
    """count * 60000 / timeDelta on either side of 2^31 (the narrowing turns it negative) at three timeDeltas; 5 999 ms: the run
    returns before it looks at an entry (timeDelta * 5 < interval * 3)."""
    fleet, rng = _edge_fleet(8, seed)
    ids = string_ids(fleet, 530)
    _roomy(fleet)
    others = [int(p) for p in np.argsort(fleet.pods["id_order"]) if p != 0]
    sp = _scaleup_params(fleet, delta=delta)
    R = _RebRows(fleet)
    for d in WRAP_DELTAS:
        c = (2**31 * d - 1) // 60_000  # the largest count whose rpm stays below 2^31
        assert c * 60_000 // d < 2**31 <= (c + 1) * 60_000 // d
        R.both("interval_count", c, c + 1, loaded=[0, others[0]])
        if d != delta:
            R.pairs.pop()
    lo, up = ITER - MAX_AGE_ITERS, ITER - MIN_AGE_ITERS
    R.add(loaded=[0], earlier_use_iteration=lo + 1, last_used_iteration=up - 1)
    R.add(loaded=[0, others[0]], interval_count=RATE_THR * delta // 60_000 + 1)
    entries, conc = R.done()
    return fleet, ids, entries, None, sp, None, dict(pairs=R.pairs if delta != 5_999 else [])


def _rate_exclude(P, which, seed=4):
    """getExcludeSet (:5835-5856): instances at maxRpm and one above it, where 4 * thr is the larger term (a), where ourRpm - 2 * thr is
    (b), where they are equal (c); the caller and a shutting-down instance far above; models whose candidates it leaves 0 / 1 of."""
    thr, our = 100, dict(a=0, b=1_000, c=600)[which]
    max_rpm = max(4 * thr, our - 2 * thr)
    fleet, rng = _edge_fleet(P, seed)
    ids = string_ids(fleet, 540 + P)
    _roomy(fleet)
    pods = fleet.pods
    at, over = [1] + ([62] if P > 8 else []), [2] + ([63] if P > 8 else []) + ([64] if P > 64 else [])
    pods["rpm"][at], pods["rpm"][over] = max_rpm, max_rpm + 1
    pods["rpm"][0], pods["rpm"][3], pods["flags"][3] = 10**9, 10**9, 1
    S, k = P - 1, len(over)
    free = [p for p in range(4, P) if p not in at + over]
    sp = _scaleup_params(fleet, thr=thr, our_rpm=our)
    R = _RebRows(fleet)
    hot = dict(interval_count=thr)
    # the excluded instances in neither list: candidates - k - k
    a = R.add(loaded=[0, free[0]], failed=free[1:1 + S - 2 - 2 * k], **hot)
    b = R.add(loaded=[0, free[0]], failed=free[1:1 + S - 2 - 2 * k - 1], **hot)
    R.pairs.append((a, b, None))
    # in the loaded list, in the failed list: candidates - k
    for where in ("loaded", "failed"):
        n_fail = S - 1 - k - k  # candidates before: k
        lists = dict(loaded=[0] + over, failed=free[:n_fail]) if where == "loaded" else dict(loaded=[0], failed=over + free[:n_fail])
        a = R.add(**lists, last_used_iteration=1, **hot)
        lists["failed"] = lists["failed"][:-1]
        b = R.add(**lists, last_used_iteration=1, **hot)
        R.pairs.append((a, b, None))
    R.add(loaded=[0, free[0]], interval_count=3 * thr)
    entries, conc = R.done()
    return fleet, ids, entries, None, sp, None, dict(pairs=R.pairs, overloaded=over)


def _rate_count(n_live, seed=5):
    """clusterStats.instanceCount 1 / 2 (:5658): the run with one instance returns early."""
    fleet, rng = _edge_fleet(8, seed)
    ids = string_ids(fleet, 550)
    _roomy(fleet)
    fleet.pods["flags"][n_live:] = 1
    R = _RebRows(fleet)
    lo, up = ITER - MAX_AGE_ITERS, ITER - MIN_AGE_ITERS
    R.add(loaded=[0], earlier_use_iteration=lo + 1, last_used_iteration=up - 1)
    R.add(loaded=[0], interval_count=RATE_THR, last_used_iteration=1)
    entries, conc = R.done()
    return fleet, ids, entries, None, _scaleup_params(fleet), None, dict(pairs=[])


def _rate_nolru(with_lru, seed=9):
    """A full cluster (10 * tf < tc) in which no instance has an lru: globalLru is Long.MAX_VALUE and now - globalLru wraps negative, so the
    lru clause does not fire either; the same table with one instance 80 000 000 ms old: it does."""
    fleet, rng = _edge_fleet(8, seed)
    ids = string_ids(fleet, 555)
    p = fleet.pods
    p["capacity"], p["used"], p["rpm"], p["lru_time"] = 1_000_000, 1_000_000, 0, 0
    if with_lru:
        p["lru_time"][1] = fleet.now - 80_000_000
    R = _RebRows(fleet)
    lo, up = ITER - MAX_AGE_ITERS, ITER - MIN_AGE_ITERS
    R.add(loaded=[0], earlier_use_iteration=lo + 1, last_used_iteration=up - 1)
    R.add(loaded=[0, 1], interval_count=RATE_THR)
    entries, conc = R.done()
    return fleet, ids, entries, None, _scaleup_params(fleet), None, dict(pairs=[])


def _cts(count, per_call=100):
    return (count * per_call) * (1 << _lib.CONC_COUNT_BITS) + count


def _rate_conc(seed=6):
    """getRpmScaleThreshold(true) (:2766-2796): counts 63 / 64 and 7 / 8 with priorCount 0, 1, -1; timeSum 0 (Integer.MAX_VALUE, whose
    * 3 wraps to a heavy limit of 536 870 911); rpm on either side of a computed threshold."""
    fleet, rng = _edge_fleet(8, seed)
    ids = string_ids(fleet, 560)
    _roomy(fleet)
    others = [int(p) for p in np.argsort(fleet.pods["id_order"]) if p != 0]
    R = _RebRows(fleet)
    two = dict(loaded=[0, others[0]])
    for pc, ps in ((0, 0), (1, 7), (-1, 7)):
        for lo_c, hi_c in ((63, 64), (7, 8)):
            i = R.add(conc=dict(count_and_time_sum=_cts(lo_c), prior_count=pc, prior_sum=ps), interval_count=3_000, **two)
            j = R.add(conc=dict(count_and_time_sum=_cts(hi_c), prior_count=pc, prior_sum=ps), interval_count=3_000, **two)
            R.pairs.append((i, j, "conc.count_and_time_sum"))
    R.both("interval_count", 536_870_911, 536_870_912, conc=dict(count_and_time_sum=64), **two)
    R.both("interval_count", 536_870_911, 536_870_912, conc=dict(count_and_time_sum=3, prior_count=9), **two)
    # 64 calls of 10 ms, one at a time: 64 * 540 000 / 6 400 = 5 400
    R.both("interval_count", 5_399, 5_400, conc=dict(count_and_time_sum=_cts(64)), **two)
    R.both("interval_count", 4_050, 4_051, conc=dict(count_and_time_sum=_cts(64)), **two)  # its heavy limit
    R.both("interval_count", 21_599, 21_600, conc=dict(count_and_time_sum=_cts(64), max_conc=4), **two)
    entries, conc = R.done()
    return fleet, ids, entries, conc, _scaleup_params(fleet), _conc_params(), dict(pairs=R.pairs)


def _rate_conc_wrap(seed=7):
    """A threshold's quotient on either side of 2^31: 64 * 2^26 / timeSum at timeSum 2 (2^31: the narrowing gives Integer.MIN_VALUE) and 3."""
    fleet, rng = _edge_fleet(8, seed)
    ids = string_ids(fleet, 570)
    _roomy(fleet)
    others = [int(p) for p in np.argsort(fleet.pods["id_order"]) if p != 0]
    R = _RebRows(fleet)
    for cnt in (10, 3_000):
        i = R.add(loaded=[0, others[0]], interval_count=cnt, conc=dict(count_and_time_sum=(2 << _lib.CONC_COUNT_BITS) + 64))
        j = R.add(loaded=[0, others[0]], interval_count=cnt, conc=dict(count_and_time_sum=(3 << _lib.CONC_COUNT_BITS) + 64))
        R.pairs.append((i, j, "conc.count_and_time_sum"))
    entries, conc = R.done()
    return fleet, ids, entries, conc, _scaleup_params(fleet), _conc_params(dyn=2**26), dict(pairs=R.pairs)


AVG_BELOW, AVG_AT, AVG_BEYOND = 2147483646.5 / 900.0, 2147483647.5 / 900.0, 1.0e7


def _rate_conc_avg(avg, seed=8):
    """getExcludeSet's own threshold (int) (900.0 * averageModelParallelism) (:5836) at 2^31 - 2, saturated at 2^31 - 1, and far beyond:
    maxRpm is ourRpm + 4 / ourRpm + 2, an instance at ourRpm + 3 is excluded or not.  Every entry's maxConc is 0: the run's new
    averageModelParallelism is max(1.0, 0 / n) = 1.0."""
    assert int(900.0 * AVG_BELOW) == 2**31 - 2 and 900.0 * AVG_AT >= 2147483647.0
    our = 1_000
    fleet, rng = _edge_fleet(8, seed)
    ids = string_ids(fleet, 580)
    _roomy(fleet)
    fleet.pods["rpm"][[1, 2, 3]] = [our + 2, our + 3, our + 5]
    R = _RebRows(fleet)
    hot = dict(interval_count=100, conc=dict(max_conc=0))
    # 8 instances: candidates before 4 and 3; excluded {3} or {2, 3}, none of them held
    R.add(loaded=[0, 4], failed=[5, 6], **hot)
    R.add(loaded=[0, 4], failed=[5, 6, 7], **hot)
    R.add(loaded=[0, 4], **hot)
    entries, conc = R.done()
    return fleet, ids, entries, conc, _scaleup_params(fleet, thr=100, our_rpm=our), _conc_params(avg=avg), dict(pairs=[])


@functools.lru_cache(maxsize=None)
def _rate_edge_all():
    out = {}
    out["edge_rate_plain_8"] = _rate_plain(8, 0, 255)
    out["edge_rate_plain_64"] = _rate_plain(64, 1, 256)
    out["edge_rate_plainconc_65"] = _rate_plain(65, 2, 257, latency=True)
    out["edge_rate_typed_65_at"] = _rate_typed(65, 0, 257, 0)
    out["edge_rate_typed_65_over"] = _rate_typed(65, 0, 257, -1)
    out["edge_rate_typedconc_64_at"] = _rate_typed(64, 1, 120, 0, latency=True)
    out["edge_rate_suitable_64"] = _rate_suitable(64, 2, 256)
    for d in (5_999,) + WRAP_DELTAS:
        out[f"edge_rate_wrap_8_{d}"] = _rate_wrap(d)
    out["edge_rate_exclude_8_a"] = _rate_exclude(8, "a")
    out["edge_rate_exclude_64_b"] = _rate_exclude(64, "b")
    out["edge_rate_exclude_65_c"] = _rate_exclude(65, "c")
    out["edge_rate_count_8_1"], out["edge_rate_count_8_2"] = _rate_count(1), _rate_count(2)
    out["edge_rate_nolru_8_none"], out["edge_rate_nolru_8_old"] = _rate_nolru(False), _rate_nolru(True)
    out["edge_rate_conc_8"] = _rate_conc()
    out["edge_rate_concwrap_8"] = _rate_conc_wrap()
    for k, avg in (("below", AVG_BELOW), ("at", AVG_AT), ("beyond", AVG_BEYOND)):
        out[f"edge_rate_concavg_8_{k}"] = _rate_conc_avg(avg)
    return out


# pairs of RUNS: (case a, row a, case b, row b): the same row of two runs that differ in one parameter or one table value by one unit
# (row -1: the whole run — one of the two returns early)
def rate_run_pairs():
    c = _rate_edge_all()
    out = [("edge_rate_typed_65_at", r, "edge_rate_typed_65_over", r) for r in c["edge_rate_typed_65_at"][6]["lru_rows"]]
    out += [("edge_rate_wrap_8_5999", -1, "edge_rate_wrap_8_6000", -1), ("edge_rate_count_8_1", -1, "edge_rate_count_8_2", -1)]
    out += [("edge_rate_concavg_8_below", 0, "edge_rate_concavg_8_at", 0)]
    out += [("edge_rate_nolru_8_none", 0, "edge_rate_nolru_8_old", 0)]
    return out


def _scaledown_params(fleet, self_pod, thr=2000, cap=10**9, since=60_000, sd=0):
    """One janitor pass: timeSinceLastCheck 60 000 makes a candidate's rpm its interval count."""
    dp = np.zeros(1, dtype=_lib.SCALEDOWN_PARAMS)
    dp["self_pod"], dp["shutting_down"], dp["now"] = self_pod, sd, fleet.now
    dp["last_check_time"], dp["rate_check_interval_ms"] = fleet.now - since, 10_000
    dp["adjusted_cache_capacity"], dp["scale_up_rpm_threshold"] = cap, thr
    return dp


def _janitor_fleet(P, seed, glru, now=None):
    """A full cluster (tf == 0: the janitor goes on) whose oldest lru is glru; the caller in the middle of PLACEMENT_ORDER, a live
    instance before and one behind it, one shutting down and one gone.  -> (fleet, ids, caller, before, behind, down, gone)"""
    fleet, rng = _edge_fleet(P, seed)
    if now is not None:
        fleet.now = now
    ids = string_ids(fleet, 600 + seed)
    p = fleet.pods
    p["capacity"], p["used"], p["rpm"] = 1_000_000, 1_000_000, 0
    p["lru_time"] = glru + rng.permutation(P) * 1_000 + 1_000
    p["lru_time"][2] = glru
    down, gone = P - 1, P - 2
    p["flags"][down], p["flags"][gone] = 1, 4
    order = [int(x) for x in cluster_order(fleet)]
    assert len(order) == P - 2
    return fleet, ids, order[len(order) // 2], order[0], order[-1], down, gone


def _two_copy_rows(R, now, cache_age, S, before):
    """removeSecondModelCopy's age (:6240-6262): cacheAge / 10, capped at ten hours when the model was not heavy lately."""
    sda_u, fifth = cache_age // 10, cache_age // 5
    sda_c = min(36_000_000, sda_u)
    two = dict(loaded=[S, before])
    out = []
    for lh in (0, now - (fifth - 1)):  # the cap applies
        out.append(R.both("last_used", now - sda_c, now - (sda_c + 1), last_heavy_time=lh, **two))
    out.append(R.both("last_used", now - sda_u, now - (sda_u + 1), last_heavy_time=now - fifth, **two))  # ... and does not
    if sda_u > sda_c:
        R.both("last_heavy_time", now - fifth, now - (fifth - 1), last_used=now - (sda_c + 1), **two)
    return out


def _janitor_two(P, seed, cache_age, n_entries=0, self_flags=2):
    fleet, ids, S, before, behind, down, gone = _janitor_fleet(P, seed, wl.NOW_MS - cache_age)
    now = fleet.now
    R = _RebRows(fleet)
    _two_copy_rows(R, now, cache_age, S, before)
    old = dict(last_used=now - cache_age)
    a = R.add(loaded=[S, before], **old)   # the other copy before the caller in the order: ours goes
    b = R.add(loaded=[S, behind], **old)   # ... behind it: ours stays
    R.pairs.append((a, b, None))
    for other in (down, gone):             # no other live copy
        R.pairs.append((a, R.add(loaded=[S, other], **old), None))
    R.add(loaded=[S], **old)
    R.add(loaded=[S, before], last_used=0)
    R.add(model=-1, **old)
    R.add(loaded=[behind, before, S], **old)  # three copies: the other rule
    R.pad(n_entries or len(R.rows), last_used=now - 1_000)
    fleet.pods["flags"][S] = self_flags
    entries, conc = R.done()
    return fleet, ids, entries, None, _scaledown_params(fleet, S), 0, \
        dict(pairs=R.pairs if self_flags == 2 else [], cache_age=cache_age, order_row=a)


def min_age_of(glru):
    """minAgeMs as removeModelCopies computes it (:6277-6283: the ABSOLUTE lru, quirk B#13) -> (the quotient, the clamped value)"""
    q = _tdiv(_i64(_i64(3 * glru) + 10_400_000), 100)
    return q, min(max(q, 600_000), 18_000_000)


# globalLru values near the epoch, by the quotient (3 * globalLru + 10 400 000) / 100 they give
MIN_AGE_LRUS = {"599999": 16_533_333, "600000": 16_533_334, "600001": 16_533_367, "mid": 100_000_000, "17999999": 596_533_333,
                "18000000": 596_533_334, "18000001": 596_533_367}
JANITOR_COUNTS = (0, 1, 2, 3, 66, 67, 1333, 1334, 3600, 3601)


def _janitor_three(P, seed, glru, thr=2000, since=60_000, latency=False, n_entries=0):
    """Three copies (:6264-6306) under a clock near the epoch: lastUnloadTime, a recent load, minAgeMs in its three bands, the rpm rule."""
    fleet, ids, S, before, behind, down, gone = _janitor_fleet(P, seed, glru, now=glru + 50_000_000)
    now = fleet.now
    q, m = min_age_of(glru)
    R = _RebRows(fleet)
    three = dict(loaded=[S, before, behind])
    R.both("last_heavy_time", now - (m - 1), now - m, **three)
    R.add(last_heavy_time=0, **three)
    R.both("last_unload_time", now - 79_999, now - 80_000, **three)
    a = R.add(loaded=[S, (before, now - 1_800_000), behind])
    b = R.add(loaded=[S, (before, now - 1_800_000 + 1), behind])
    R.pairs.append((a, b, "ent_time"))
    R.pairs.append((a, R.add(loaded=[(S, now - 1_800_000 + 1), before, behind]), None))  # the caller's own load counts
    rows = {c: R.add(interval_count=c, **three) for c in JANITOR_COUNTS}
    lim = (thr * 2) // 3
    if since == 60_000 and not latency:
        R.pairs.append((rows[lim], rows[lim + 1], "interval_count"))
    if latency:  # 64 calls of 10 ms: 5 400, two thirds of it 3 600; no samples: scaleUpRpmThreshold
        busy = dict(count_and_time_sum=_cts(64))
        R.both("interval_count", 3_600, 3_601, conc=busy, **three)
        R.both("interval_count", lim, lim + 1, conc=dict(count_and_time_sum=7), **three)
        R.both_conc("queued_requests", 1, 2, {}, **three)
    R.pad(n_entries or len(R.rows), last_used=now - 1_000)
    entries, conc = R.done()
    return fleet, ids, entries, (conc if latency else None), _scaledown_params(fleet, S, thr=thr, since=since), 540_000, \
        dict(pairs=R.pairs if since >= 1_000 else [], min_age=(q, m), go_row=2)  # (a sample period too short refuses every row)


def _janitor_budget(entries_spec, cap, sd=0, pairs=()):
    """The serial allowance (:6117-6135) over two-copy candidates that removeModelCopies takes (True) or refuses (False)."""
    cache_age = 100_000_000
    fleet, ids, S, before, behind, down, gone = _janitor_fleet(8, 9, wl.NOW_MS - cache_age)
    R = _RebRows(fleet)
    for i, (w, takes) in enumerate(entries_spec):  # oldest first, no two alike: as scaleCopiesCandidates hands them over; refused: the other
        # copy stands behind the caller in the order
        R.add(loaded=[S, before if takes else behind], weight=w, last_used=fleet.now - cache_age - 1_000 * (len(entries_spec) - i))
    entries, conc = R.done()
    return fleet, ids, entries, None, _scaledown_params(fleet, S, cap=cap, sd=sd), 0, dict(pairs=list(pairs))


BUDGET_EXACT = ((60_000, True), (40_001, True), (30_000, False), (40_000, True), (1, True))  # allowance 100 000: rows 0 and 3 go
BUDGET_NEGATIVE = ((100_001, True), (1, True), (0, True))  # the first goes whatever it weighs; the allowance is then -1
BUDGET_SMALL = ((1, True), (0, True), (1, True))  # allowance 0 / 1 / 1 / 2 at capacities 19 / 20 / 39 / 40


def _janitor_full(extra, tf):
    """instanceSetStats() on either side of tf * 100 / tc > 5 (:6229): tc = 8 000 000 + extra over six live instances, all of tf on one."""
    fleet, ids, S, before, behind, down, gone = _janitor_fleet(8, 10, wl.NOW_MS - 100_000_000)
    p = fleet.pods
    live = [i for i in range(8) if i not in (down, gone)]
    p["capacity"][live] = [1_333_334, 1_333_334, 1_333_333, 1_333_333, 1_333_333, 1_333_333]
    p["used"][live] = p["capacity"][live]
    p["capacity"][live[0]] += extra
    p["used"][live[0]] = p["capacity"][live[0]] - tf
    assert int(p["capacity"][live].sum()) == 8_000_000 + extra
    order = [int(x) for x in cluster_order(fleet)]  # (the instance with room moves in the order)
    S, before, behind = order[len(order) // 2], order[0], order[-1]
    R = _RebRows(fleet)
    R.add(loaded=[S, before], last_used=fleet.now - 100_000_000)
    R.add(loaded=[S, before, behind])
    entries, conc = R.done()
    return fleet, ids, entries, None, _scaledown_params(fleet, S), 0, dict(pairs=[], totals=(8_000_000 + extra, tf))


@functools.lru_cache(maxsize=None)
def _janitor_edge_all():
    out = {}
    out["edge_janitor_two_8_low"] = _janitor_two(8, 0, 100_000_000, 255)
    out["edge_janitor_two_64_at"] = _janitor_two(64, 1, 360_000_000, 256)
    out["edge_janitor_two_65_at1"] = _janitor_two(65, 2, 360_000_010, 257)
    out["edge_janitor_two_8_far"] = _janitor_two(8, 3, 2_000_000_000)
    out["edge_janitor_two_8_selfdown"] = _janitor_two(8, 0, 100_000_000, 255, self_flags=1)
    out["edge_janitor_two_8_selfgone"] = _janitor_two(8, 0, 100_000_000, 255, self_flags=4)
    for k, g in MIN_AGE_LRUS.items():
        out[f"edge_janitor_three_8_{k}"] = _janitor_three(8, 4, g)
    out["edge_janitor_three_65_mid"] = _janitor_three(65, 5, MIN_AGE_LRUS["mid"], n_entries=257)
    for thr in (1, 2, 3, 100):
        out[f"edge_janitor_thr_8_{thr}"] = _janitor_three(8, 4, MIN_AGE_LRUS["mid"], thr=thr)
    for since in (999, 1_000):
        out[f"edge_janitor_since_8_{since}"] = _janitor_three(8, 4, MIN_AGE_LRUS["mid"], since=since)
    out["edge_janitor_conc_8"] = _janitor_three(8, 4, MIN_AGE_LRUS["mid"], latency=True)
    out["edge_janitor_budget_8_exact"] = _janitor_budget(BUDGET_EXACT, 2_000_000, pairs=[(1, 3, "weight")])
    out["edge_janitor_budget_8_down"] = _janitor_budget(BUDGET_EXACT, 2_000_000, sd=1)
    out["edge_janitor_budget_8_negative"] = _janitor_budget(BUDGET_NEGATIVE, 2_000_000, pairs=[(0, 1, None)])
    for cap in (19, 20, 39, 40):
        out[f"edge_janitor_budget_8_{cap}"] = _janitor_budget(BUDGET_SMALL, cap)
    # 6 * tc - 1 is odd and tf * 100 even: the nearest a table can come from below is 6 * tc - 2 (tc = 8 000 017)
    out["edge_janitor_full_8_below"] = _janitor_full(17, 480_001)   # tf * 100 == 6 * tc - 2: goes on
    out["edge_janitor_full_8_above"] = _janitor_full(17, 480_002)   # one unit more: refuses everything
    out["edge_janitor_full_8_under"] = _janitor_full(0, 479_999)    # tf * 100 == 6 * tc - 100: goes on
    out["edge_janitor_full_8_equal"] = _janitor_full(0, 480_000)    # tf * 100 == 6 * tc: refuses everything
    return out


def janitor_run_pairs():
    j = "edge_janitor_"
    r = _janitor_edge_all()[j + "two_8_low"][6]["order_row"]
    out = [(j + "two_8_low", r, j + "two_8_" + k, r) for k in ("selfdown", "selfgone")]  # the caller shutting down / not in the table
    out += [(j + "since_8_999", 2, j + "since_8_1000", 2), (j + "budget_8_exact", 0, j + "budget_8_down", 0)]
    out += [(j + "budget_8_19", 1, j + "budget_8_20", 1), (j + "budget_8_39", 2, j + "budget_8_40", 2)]
    out += [(j + "full_8_below", r, j + "full_8_above", r) for r in (0, 1)] + [(j + "full_8_under", r, j + "full_8_equal", r) for r in (0, 1)]
    return out


def plan_cutoff(now, lru_age):
    """proactiveLastUsedCutoff (:6657-6664) of a cluster whose globalLru is now - lru_age (None: no lru)"""
    return 0 if lru_age is None else now - lru_age + max(lru_age // 3, 1_200_000)


def _plan_case(seed, units, pods, copies, lru_age, models, groups=(), types=None, pairs=()):
    """pods: per instance (capacity, used, loadingThreads, loadingInProgress); copies: modelCopyCount, on the first instance (of every
    group); lru_age: now - globalLru (None: no instance has an lru); models: [(lastUsed, n_failed)], unloaded, in registry order.
    minSpaceUnits is 1, so that a single free unit counts into totalFree."""
    P = len(pods)
    fleet, rng = _edge_fleet(P, seed, groups)
    fleet.min_space_units = 1
    ids = string_ids(fleet, 700 + seed)
    p, now = fleet.pods, fleet.now
    for i, (c, u, t, ip) in enumerate(pods):
        p["capacity"][i], p["used"][i], p["loading_threads"][i], p["loading_in_progress"][i] = c, u, t, ip
    p["count"] = 0
    for g in (groups or [range(P)]):
        p["count"][list(g)[0]] = copies
    p["lru_time"] = 2**63 - 1 if lru_age is None else now - lru_age + 1_000 + np.arange(P) * 1_000
    if lru_age is not None:
        p["lru_time"][0] = now - lru_age
    rows = np.zeros(len(models), dtype=_lib.MODEL_ROW)
    ent = []
    for i, (lu, nf) in enumerate(models):
        rows[i] = (0 if types is None else types[i], len(ent), 0, nf, lu)
        ent += sorted(range(nf), key=lambda q: p["id_order"][q])
    fleet.models, fleet.ent_pod = rows, np.array(ent, np.int32)
    fleet.ent_time = np.full(len(ent), now - 3_000_000, np.int64)
    return fleet, ids, units, bool(groups), dict(pairs=list(pairs))


QUIET = (1_000_000, 500_000, 0, 0)  # room, but no loading thread: it adds nothing to spaceToFill
TINY = (8, 8, 0, 0)
NARROW_A = (2**30, 7 * 2**27 - 7, 8, 0)  # avail 7


def _narrow_pods(total_used):
    """Eight instances of 2^30 units whose `used` sums to total_used (nothing full but exactly-full ones: tc - tf == total_used); only the
    first can load."""
    rest, out = total_used - NARROW_A[1], [NARROW_A]
    for _ in range(7):
        u = min(rest, 2**30)
        out.append((2**30, u, 0, 0))
        rest -= u
    assert rest == 0
    return out


def _below(now, lru_age, n):
    """n distinct candidates older than the cutoff: loaded only as far as freeSpaceProactiveLoadCount reaches"""
    return [(plan_cutoff(now, lru_age) - 1_000_000 - 1_000 * i, 0) for i in range(n)]


@functools.lru_cache(maxsize=None)
def _plan_edge_all():
    now, age = wl.NOW_MS, 9_000_000
    cut = plan_cutoff(now, age)
    out = {}
    # sizeEstimate: modelCopyCount 2 / 3 and 10 / 11 (tc - tf = 4 000 000)
    a_pods = [(4_000_000, 2_000_000, 8, 0)] + [QUIET] * 4 + [(1_000_000, 0, 0, 0)] * 3
    for c in (2, 3, 10, 11):
        out[f"edge_plan_copies_8_{c}"] = _plan_case(0, 6400, a_pods, c, age, _below(now, age, 130))
    # (int) (tc - tf) binds before the division
    for name, used, c, units in (("2p31m1", 2**31 - 1, 11, 6400), ("2p31", 2**31, 11, 6400), ("2p32m1", 2**32 - 1, 5, 6401), ("2p32", 2**32, 5, 6401),
                                 ("2p32p4", 2**32 + 4, 5, 3), ("2p32p5", 2**32 + 5, 5, 3)):
        out[f"edge_plan_narrow_8_{name}"] = _plan_case(1, units, _narrow_pods(used), c, age, _below(now, age, 12))
    # spaceToFill at sizeEstimate 1: the first instance gives k, the second the engineered term
    sp = lambda k, v: [(1_000_000, 0, 1, 50 - k), v] + [QUIET] * 6  # noqa: E731
    odd = 1_000_003  # / 8 = 125 000
    for name, k, v, units in (("maxloads0", 1, (1_000_000, 0, 1, 50), 1), ("maxloads1", 1, (1_000_000, 0, 1, 49), 1),
                              ("avail0", 3, (odd, odd - 125_000, 8, 0), 1), ("avail1", 3, (odd, odd - 125_001, 8, 0), 1),
                              ("over", 3, (odd, odd + 5, 8, 0), 1),
                              ("by2", 3, (odd, odd - 125_002, 1, 47), 1), ("by3", 3, (odd, odd - 125_003, 1, 47), 1),
                              ("by4", 3, (odd, odd - 125_004, 1, 47), 1),
                              ("wrap1", 3, (1_000_000, 0, 1, 49), 2**30), ("wrap2", 3, (1_000_000, 0, 1, 48), 2**30)):
        out[f"edge_plan_space_8_{name}"] = _plan_case(2, units, sp(k, v), 2, age, _below(now, age, 12))
    # freeSpaceProactiveLoadCount below, at and above totalCapacity / (20 * sizeEstimate) = 10
    for avail in (19, 20, 21, 22):
        out[f"edge_plan_count_8_{avail}"] = _plan_case(3, 1, [(160, 140 - avail, 8, 0)] + [TINY] * 7, 2, age, _below(now, age, 14))
    # the gate: totalFree 0 / 1, totalCapacity 0 / 1
    full = (1_000_000, 1_000_000, 0, 0)
    gate_models = [(cut + 5, 0), (now - age, 1), (now - age + 1, 1), (now - age + 1, 2)]  # the registry rule lastUsed > globalLru
    out["edge_plan_gate_8_tf0"] = _plan_case(4, 100, [full] * 8, 2, age, gate_models)
    out["edge_plan_gate_8_tf1"] = _plan_case(4, 100, [(1_000_000, 999_999, 0, 0)] + [full] * 7, 2, age, gate_models)
    out["edge_plan_gate_8_tc0"] = _plan_case(4, 100, [(0, 0, 0, 0)] * 8, 2, age, gate_models)
    out["edge_plan_gate_8_tc1"] = _plan_case(4, 100, [(1, 0, 0, 0)] + [(0, 0, 0, 0)] * 7, 2, age, gate_models)
    # the cutoff: age / 3 on either side of 1 200 000, no lru at all; candidates at cutoff - 1, cutoff, cutoff + 1
    for name, a in (("1199999", 3_599_999), ("1200000", 3_600_000), ("1200001", 3_600_003), ("nolru", None)):
        c = plan_cutoff(now, a)
        ms = [(c - 1, 0), (c, 0), (c + 1, 0), (c + 5, 1), (c + 6, 2)]
        out[f"edge_plan_cutoff_8_{name}"] = _plan_case(5, 6400, [QUIET] * 8, 2, a, ms, pairs=[(1, 2, "last_used"), (3, 4, None)])  # (3, 4): one / two failures
    # ... with one free-space load: the first is taken whatever its age, the second must be >= cutoff
    out["edge_plan_cutoff_8_free1"] = _plan_case(5, 6400, [QUIET, (1_000_000, 0, 1, 48)] + [QUIET] * 6, 2, age,
                                                 [(cut - 1, 0), (cut + 1, 0), (cut, 0)], pairs=[(2, 0, "last_used")])
    # the TreeSet: exactly totalProactiveLoadCount (3) distinct candidates, and one more; ties are dropped, set full or not
    x = cut + 10
    set3 = [(x + 3, 0), (x + 2, 0), (x + 2, 0), (x + 1, 0)]
    small = [(600, 0, 0, 0)] + [TINY] * 7
    out["edge_plan_set_8_3"] = _plan_case(6, 10, small, 2, age, set3, pairs=[(1, 2, None)])
    out["edge_plan_set_8_4"] = _plan_case(6, 10, small, 2, age, set3 + [(x + 1, 0), (x, 0)], pairs=[(1, 2, None), (3, 4, None), (3, 5, "last_used")])
    # per partition: eight groups of eight instances, each one of the tables above; its models carry the group's type
    blocks = [a_pods, a_pods, sp(1, (1_000_000, 0, 1, 49)), sp(3, (odd, odd - 125_003, 1, 47)), [QUIET, (1_000_000, 0, 1, 48)] + [QUIET] * 6,
              small, [(160, 120, 8, 0)] + [TINY] * 7, [QUIET] * 8]
    pods = [r for b in blocks for r in b]
    models, types = [], []
    for k in range(8):
        models += [(cut - 5 + i, i % 3 == 2 and 2 or 0) for i in range(20)] + [(cut - 2_000_000 - 1_000 * i - k, 0) for i in range(20)]
        types += [k + 1] * 40
    models += [(cut + 100 + i, 0) for i in range(5)]
    types += [0, 99, -1, 0, 0]
    out["edge_plan_parts_64"] = _plan_case(7, 6400, pods, 3, age, models, groups=[list(range(8 * k, 8 * k + 8)) for k in range(8)], types=types)
    return out


def plan_run_pairs():
    p = "edge_plan_"
    names = [("copies_8_2", "copies_8_3"), ("copies_8_10", "copies_8_11"), ("narrow_8_2p31m1", "narrow_8_2p31"), ("narrow_8_2p32p4", "narrow_8_2p32p5"),
             ("space_8_maxloads0", "space_8_maxloads1"), ("space_8_avail0", "space_8_avail1"), ("space_8_by2", "space_8_by3"),
             ("count_8_19", "count_8_20"), ("count_8_21", "count_8_22"), ("gate_8_tf0", "gate_8_tf1"),
             ("cutoff_8_1199999", "cutoff_8_1200000")]
    return [(p + a, -1, p + b, -1) for a, b in names]


def rebalance_edge_tier(name):
    return name.split("_")[1]


def rebalance_edge_cases():
    """(name, tier, case): the rebalancers at the edges of their value domain, names edge_<tier>_<case>.
    rate: (fleet, ids, entries, conc | None, scaleup params, conc params | None, meta) — the rate-tracking task (:5636-5856);
    janitor: (fleet, ids, entries, conc | None, scaledown params, dynamicRpmScaleConstant, meta) — the scale-down (:6110-6335);
    plan: (fleet, ids, defaultModelSizeUnits, partitioned, meta) — the reaper's proactive loads (:6616-6747).
    meta["pairs"]: two rows (cache entries; registry rows for the plan) on either side of one threshold, (a, b, engineered field or None)."""
    for tier, cases in (("rate", _rate_edge_all()), ("janitor", _janitor_edge_all()), ("plan", _plan_edge_all())):
        for name, case in cases.items():
            yield name, tier, case


def rebalance_run_pairs():
    """(case a, row a, case b, row b): the same row of two RUNS that differ by one unit in one parameter or one table value (row -1: the
    run as a whole — an early return, or the plan's call list)."""
    return rate_run_pairs() + janitor_run_pairs() + plan_run_pairs()


def rebalance_blob(tier, case):
    """The harness' input for one case: the stats it is GIVEN are what oracle.bind computes from the fleet."""
    from oracle import bind as ob
    fleet, ids = case[0], case[1]
    if tier == "rate":
        _, _, entries, conc, sp, cp, _ = case
        cstats = np.zeros(1, dtype=ob.ORC_STATS)
        cstats[0] = ob.OracleFleet(fleet).stats()
        return input_blob(fleet, ids, scaleup=(entries, sp, cstats, np.ascontiguousarray(ob.type_set_stats(fleet))),
                          conc=None if conc is None else (conc, cp))
    if tier == "janitor":
        _, _, entries, conc, dp, dyn, _ = case
        cp = _conc_params(dyn=dyn)
        return input_blob(fleet, ids, scaledown=(entries, dp, ob.instance_set_stats(fleet, int(dp["self_pod"][0]))),
                          conc=None if conc is None else (conc, cp))
    from oracle.ref_harness.make_ref_vectors import proactive_inputs
    return input_blob(fleet, ids, proactive=proactive_inputs(fleet, case[2], case[3]))


TABLE_EVENT = np.dtype([("type", "<i4"), ("pod", "<i4"), ("row", _lib.POD_ROW)])  # type: 0 ENTRY_ADDED, 1 ENTRY_UPDATED, 2 ENTRY_DELETED


def table_event_cases():
    """(name, fleet, ids, events, checkpoint_every, tables): a stream of instance-table listener events (MM.java:1455-1568) from
    an empty table — every instance added, then records republished (load / used / count / lruTime change, an emptied cache,
    shutdown announcements), instances deleted and re-added.  tables[k] = the instance table (rows + flags) as it stands at
    checkpoint k, for the implementations that take a table rather than events."""
    for seed, pods, n_ev, ck in ((0, 6, 60, 1), (1, 40, 600, 7), (2, 300, 3000, 100), (3, 300, 3000, 250)):
        rng = np.random.default_rng(400 + seed)
        fleet = wl.fuzz_fleet(seed + 30, pods=pods, models=50, profile=[None, "full", "pref", None][seed])
        fleet.n_types, fleet.allowed, fleet.prefer = 0, None, None
        fleet.has_allowed = fleet.has_prefer = None
        ids = string_ids(fleet, 60 + seed)
        now = fleet.now
        rows = fleet.pods.copy()
        rows["flags"] = _lib_flag_live()
        cur = rows.copy()
        present = np.zeros(pods, bool)
        ev = np.zeros(pods + n_ev, dtype=TABLE_EVENT)
        tables = []

        def snapshot():
            t = cur.copy()
            t["flags"] = np.where(present, t["flags"], 4)  # absent: tombstone
            tables.append(t)
        k = 0
        for i in rng.permutation(pods):
            ev[k] = (0, i, cur[i])
            present[i] = True
            k += 1
            if k % ck == 0:
                snapshot()
        while k < len(ev):
            i = int(rng.integers(0, pods))
            u = rng.random()
            if not present[i]:
                r = rows[i].copy()
                r["flags"] = _lib_flag_live()
                cur[i] = r
                ev[k] = (0, i, r)
                present[i] = True
            elif u < 0.12:
                ev[k] = (2, i, cur[i])
                present[i] = False
            elif u < 0.18:  # announces its shutdown: the listener treats the update as a delete (:1462-1464)
                r = cur[i].copy()
                r["flags"] = r["flags"] | 1
                ev[k] = (1, i, r)
                present[i] = False
            elif u < 0.22:  # republished unchanged: "Identical instance record already exists" (:1505-1509)
                ev[k] = (1, i, cur[i])
            else:
                r = cur[i].copy()
                what = rng.integers(0, 6)
                if what == 0:
                    r["used"] = min(int(r["capacity"]), max(0, int(r["used"]) + int(rng.integers(-40_000, 40_000))))
                elif what == 1:
                    r["count"] = max(0, int(r["count"]) + int(rng.integers(-3, 4)))
                elif what == 2:
                    r["lru_time"] = now - int(rng.integers(1_000, 80_000_000))
                elif what == 3:
                    r["count"], r["used"], r["lru_time"] = 0, 0, 2**63 - 1  # emptied cache
                elif what == 4:
                    r["loading_in_progress"] = int(rng.integers(0, 9))
                    r["rpm"] = int(rng.choice([0, 50, 400, 9000]))
                else:
                    r["lru_time"] = 0  # a record that never reported one: not counted in the global LRU (InstanceSetStatsTracker:58)
                # (a FULL record without an lruTime does not occur — a full cache has an oldest entry — and it is the one shape
                # under which PLACEMENT_ORDER's version rule, :4654-4660, is not transitive: a skip-list set then keeps whatever
                # order its insertion history produced, and libmmplace refuses such a table with MMP_EORDER)
                if int(r["lru_time"]) == 0 and int(r["capacity"]) - int(r["used"]) < fleet.min_space_units:
                    r["lru_time"] = now - int(rng.integers(1_000, 80_000_000))
                cur[i] = r
                ev[k] = (1, i, r)
            k += 1
            if k % ck == 0 or k == len(ev):
                snapshot()
        yield f"table_events_{seed}", fleet, ids, ev, ck, tables


def migration_cases():
    """(name, fleet, ids, entries, self_pod, now): preShutdown of instance 0 (MM.java:6998-7046): its cache entries in
    descendingLruMap() order — held and not held by it according to the registry, failed, never used (lastUsed 0), older and
    younger than CUTOFF_AGE_MS."""
    for seed, pods, used in ((0, 12, 0.5), (1, 200, 0.97), (2, 200, 0.2), (3, 1, 0.5), (4, 300, 0.99)):
        fleet, rng = _rebalance_fleet(seed, pods, 600, used)
        entries = _local_entries(fleet, rng, 800)
        entries["last_used"] = np.where(rng.random(800) < 0.3, fleet.now - rng.choice([3_599_999, 3_600_000, 3_600_001, 7_000_000], 800),
                                        entries["last_used"])  # the cutoff's edges
        entries = entries[np.argsort(-entries["last_used"], kind="stable")]  # most recently used first
        yield f"migration_{seed}", fleet, string_ids(fleet, 50 + seed), entries, 0, fleet.now


def type_constraint_cases():
    """(name, fleet, ids, pod_bits, req_bits, pref_bits): a type-constraint configuration over an instance table (as
    tests/test_types_gpu.py draws them): bit i of an instance's word = it carries label i; per type the required and preferred labels."""
    for seed, P, T, n_labels, label_p in ((0, 5, 2, 2, 0.5), (1, 64, 4, 3, 0.4), (2, 200, 6, 5, 0.3), (3, 700, 8, 6, 0.15), (4, 65, 3, 2, 0.0),
                                           (5, 130, 5, 4, 0.9), (6, 300, 12, 8, 0.5), (7, 40, 1, 1, 0.5)):
        rng = np.random.default_rng(9000 + seed)
        fleet = wl.fuzz_fleet(seed, pods=P, models=50)
        fleet.n_types, fleet.allowed, fleet.prefer = 0, None, None
        fleet.has_allowed = fleet.has_prefer = None
        pod_bits = np.zeros(P, np.uint64)
        for p in range(P):
            pod_bits[p] = sum(1 << i for i in range(n_labels) if rng.random() < label_p)
        req_bits, pref_bits = np.zeros(T, np.uint64), np.zeros(T, np.uint64)
        for t in range(T):
            nr, nf = int(rng.choice([0, 0, 1, 2])), int(rng.choice([0, 1, 2]))
            req = rng.choice(n_labels, size=min(nr, n_labels), replace=False) if nr else []
            pref = [l for l in (rng.choice(n_labels, size=min(nf, n_labels), replace=False) if nf else []) if l not in req]  # kept disjoint (:96-99)
            req_bits[t] = sum(1 << int(l) for l in req)
            pref_bits[t] = sum(1 << int(l) for l in pref)
        yield f"type_constraints_{seed}", fleet, string_ids(fleet, 70 + seed), pod_bits, req_bits, pref_bits


UPGRADE_EVENT = np.dtype([("kind", "<i4"), ("replica_set", "<i4"), ("labels_key", "<i8"), ("start_time", "<i8"), ("now", "<i8")])


def upgrade_event_cases():
    """(name, events): rolling-update streams for UpgradeTracker (UpgradeTracker.java:85-200; as tests/test_upgrade_gpu.py draws
    them): instances of a few replica sets under two label sets come and go while the clock advances by 50 ms ... 7 min, with
    housekeeping passes in between.  kind 0 instanceAdded, 1 instanceRemoved, 2 doHousekeeping."""
    for seed in range(6):
        rng = np.random.default_rng(300 + seed)
        now = 1_760_000_000_000
        starts, members = {}, []
        ev = np.zeros(500, dtype=UPGRADE_EVENT)
        for step in range(500):
            now += int(rng.choice([50, 5_000, 60_000, 400_000]))
            r = rng.random()
            if r < 0.55 or not members:
                lk = int(rng.choice([0, 0, 0, 7]))
                rs = int(rng.choice([-1, 0, 1, 2, 3, 4]))
                if rs not in starts:
                    starts[rs] = now - int(rng.integers(0, 3_000_000)) * 7 - rs  # distinct per set: no ties in Stream.max
                st = starts[rs] + int(rng.integers(0, 100_000)) * 11
                ev[step] = (0, rs, lk, st, now)
                members.append((lk, rs))
            elif r < 0.9:
                lk, rs = members.pop(int(rng.integers(0, len(members))))
                if rng.random() < 0.1:
                    lk += 100  # a re-deserialised record: another labels array identity
                ev[step] = (1, rs, lk, 0, now)
            else:
                ev[step] = (2, -1, 0, 0, now)
        yield f"upgrade_events_{seed}", ev
    # rolling updates proper: a deployment's old replica set is replaced member by member by a new one (start times now),
    # a second deployment (other labels) follows with a lag, housekeeping runs every minute, then everything ages out
    for seed in range(6):
        rng = np.random.default_rng(900 + seed)
        now = 1_760_000_000_000
        rows = []
        n_old = int(rng.integers(3, 9))
        for lk, rs_old in ((0, 0), (7, 2)):
            for _ in range(n_old):
                rows.append((0, rs_old, lk, now - 86_400_000 - int(rng.integers(0, 3_600_000)), now))
                now += int(rng.integers(10, 2_000))
        live = {(0, 0): n_old, (7, 2): n_old}
        plan = [(0, 0, 1)] * n_old + [(7, 2, 3)] * n_old
        order = rng.permutation(len(plan)) if seed % 2 else np.arange(len(plan))
        for j in order:
            lk, rs_old, rs_new = plan[j]
            now += int(rng.choice([5_000, 20_000, 45_000, 200_000]))
            rows.append((0, rs_new, lk, now - int(rng.integers(1_000, 9_000)), now))
            now += int(rng.integers(500, 30_000))
            if live[(lk, rs_old)] > 0:
                rows.append((1, rs_old, lk, 0, now))
                live[(lk, rs_old)] -= 1
            if rng.random() < 0.4:
                now += 60_000
                rows.append((2, -1, 0, 0, now))
        for _ in range(6):  # ... and the aftermath: the map's entries expire 15 min after the last change
            now += int(rng.choice([240_000, 600_000]))
            rows.append((2, -1, 0, 0, now))
            rows.append((0, int(rng.choice([1, 3])), int(rng.choice([0, 7])), now - 2_000, now))
        yield f"upgrade_rolling_{seed}", np.array(rows, dtype=UPGRADE_EVENT)


def _lib_flag_live():
    return 2  # MMP_POD_LIVE


def input_blob(fleet, ids, reqs=None, extra=None, serve=None, gates=None, scaleup=None, scaledown=None, proactive=None, events=None,
               upgrade=None, types=None, migration=None, conc=None) -> bytes:
    """The harness' input file (layout: oracle/ref_harness/harness.cc main())."""
    P, M = fleet.n_pods, fleet.n_models
    T = int(fleet.n_types)
    W = (P + 63) // 64
    reqs = np.zeros(0, _lib.PLACE_REQ) if reqs is None else np.ascontiguousarray(reqs)
    extra = np.zeros(0, np.int32) if extra is None else np.ascontiguousarray(extra, dtype=np.int32)
    if serve is None:
        sreqs, in_use, last_used = np.zeros(0, _lib.SERVE_REQ), np.zeros(0, np.int32), np.zeros(0, np.int64)
        sx_pod, sx_time = np.zeros(0, np.int32), np.zeros(0, np.int64)
    else:
        sreqs, in_use, last_used, sx_pod, sx_time = serve
    repl = np.ascontiguousarray(fleet.replaced_rs, dtype=np.int32)
    if gates is None:
        greqs, gx_pod, gx_time, gexpl, g_expiry, tstats = np.zeros(0, _lib.GATE_REQ), np.zeros(0, np.int32), np.zeros(0, np.int64), \
            np.zeros(0, np.int32), 0, None
    else:
        greqs, gx_pod, gx_time, gexpl, g_expiry, tstats = gates  # tstats: typeSetStats(type) per type row (oracle.bind.ORC_STATS)
    hdr = [P, M, len(fleet.ent_pod), T, W, len(repl), len(reqs), len(extra), int(fleet.min_space_units), int(fleet.min_churn_age_ms),
           int(fleet.now), len(sreqs), len(sx_pod), len(greqs), len(gx_pod), len(gexpl)]
    idbuf = b"".join(s.encode("ascii").ljust(16, b"\0") for s in ids)
    parts = [b"MMREF1\0\0", struct.pack("<16q", *hdr), np.ascontiguousarray(fleet.pods).tobytes(), idbuf,
             np.ascontiguousarray(fleet.models).tobytes(), np.ascontiguousarray(fleet.ent_pod, dtype=np.int32).tobytes(),
             np.ascontiguousarray(fleet.ent_time, dtype=np.int64).tobytes()]
    if T:
        parts += [np.ascontiguousarray(fleet.has_allowed, dtype=np.uint8).tobytes(), np.ascontiguousarray(fleet.has_prefer, dtype=np.uint8).tobytes(),
                  np.ascontiguousarray(fleet.allowed, dtype=np.uint64).tobytes(), np.ascontiguousarray(fleet.prefer, dtype=np.uint64).tobytes()]
    parts += [repl.tobytes(), reqs.tobytes(), extra.tobytes(), np.ascontiguousarray(sreqs).tobytes()]
    if len(sreqs):
        parts += [np.ascontiguousarray(in_use, dtype=np.int32).tobytes(), np.ascontiguousarray(last_used, dtype=np.int64).tobytes()]
    parts += [np.ascontiguousarray(sx_pod, dtype=np.int32).tobytes(), np.ascontiguousarray(sx_time, dtype=np.int64).tobytes()]
    parts += [np.ascontiguousarray(greqs).tobytes(), np.ascontiguousarray(gx_pod, dtype=np.int32).tobytes(),
              np.ascontiguousarray(gx_time, dtype=np.int64).tobytes(), np.ascontiguousarray(gexpl, dtype=np.int32).tobytes()]
    if len(greqs):
        assert tstats.dtype.itemsize == 32 and len(tstats) == max(T, 1)
        parts += [struct.pack("<q", int(g_expiry)), np.ascontiguousarray(tstats).tobytes()]
    if scaleup is None:
        parts += [struct.pack("<q", -1)]
    else:
        entries, sp, cstats, ststats = scaleup  # cstats: the cluster's stats (1 ORC_STATS row); ststats: typeSetStats per type row
        assert cstats.dtype.itemsize == 32 and len(cstats) == 1 and len(ststats) == max(T, 1)
        parts += [struct.pack("<q", len(entries)), np.ascontiguousarray(sp).tobytes(), np.ascontiguousarray(entries).tobytes(),
                  np.ascontiguousarray(cstats).tobytes(), np.ascontiguousarray(ststats).tobytes()]
    if scaledown is None:
        parts += [struct.pack("<q", -1)]
    else:
        entries, dp, istats = scaledown  # istats: instanceSetStats() (1 ORC_STATS row)
        assert istats.dtype.itemsize == 32 and len(istats) == 1
        parts += [struct.pack("<q", len(entries)), np.ascontiguousarray(dp).tobytes(), np.ascontiguousarray(entries).tobytes(),
                  np.ascontiguousarray(istats).tobytes()]
    if proactive is None:
        parts += [struct.pack("<q", -1)]
    else:
        units, gstats, pstats, ptypes, pod_part = proactive  # cluster stats; per partition: its stats + prohibited type rows; pod -> partition
        assert gstats.dtype.itemsize == 32 and len(gstats) == 1 and len(pstats) == len(ptypes)
        parts += [struct.pack("<qq", len(ptypes), int(units)), np.ascontiguousarray(gstats).tobytes()]
        for k in range(len(ptypes)):
            t = np.ascontiguousarray(sorted(ptypes[k]), dtype=np.int32)
            parts += [np.ascontiguousarray(pstats[k: k + 1]).tobytes(), struct.pack("<q", len(t)), t.tobytes()]
        if len(ptypes):
            parts += [np.ascontiguousarray(pod_part, dtype=np.int32).tobytes()]
    if events is None:
        parts += [struct.pack("<q", -1)]
    else:
        ev, ck = events
        assert ev.dtype.itemsize == 72
        parts += [struct.pack("<qq", len(ev), int(ck)), np.ascontiguousarray(ev).tobytes()]
    if upgrade is None:
        parts += [struct.pack("<q", -1)]
    else:
        assert upgrade.dtype.itemsize == 32
        parts += [struct.pack("<q", len(upgrade)), np.ascontiguousarray(upgrade).tobytes()]
    if types is None:
        parts += [struct.pack("<q", -1)]
    else:
        pod_bits, req_bits, pref_bits = types
        assert len(pod_bits) == fleet.n_pods and len(req_bits) == len(pref_bits)
        parts += [struct.pack("<q", len(req_bits)), np.ascontiguousarray(pod_bits, dtype=np.uint64).tobytes(),
                  np.ascontiguousarray(req_bits, dtype=np.uint64).tobytes(), np.ascontiguousarray(pref_bits, dtype=np.uint64).tobytes()]
    if migration is None:
        parts += [struct.pack("<q", -1)]
    else:
        entries, self_pod, now = migration
        parts += [struct.pack("<qqq", len(entries), int(self_pod), int(now)), np.ascontiguousarray(entries).tobytes()]
    if conc is not None:  # optional trailer: limitModelConcurrency == true (the inputs without it keep their round-3/4 digests)
        rows, cparams = conc  # CONC_ENTRY per cache entry of the a15 / a16 section; 1 CONC_PARAMS row
        assert rows.dtype.itemsize == 32 and cparams.dtype.itemsize == 16 and len(cparams) == 1
        parts += [struct.pack("<q", len(rows)), np.ascontiguousarray(cparams).tobytes(), np.ascontiguousarray(rows).tobytes()]
    return b"".join(parts)


def digest(blob: bytes) -> str:
    return hashlib.sha256(blob).hexdigest()[:16]


def place_row_kinds(fleet, order, reqs, extra):
    """Per load-target request, from the inputs and the reference's instance order alone: (kind, full) with kind one of 'none',
    'simple', 'a found', 'a replay', 'b found', 'b replay' (MM.java:4822-4887) and full = isFull(best) as :4811 takes it."""
    P, T = fleet.n_pods, fleet.n_types
    al = [None] * max(T, 1)
    pf = [None] * max(T, 1)
    for t in range(T):
        bits = lambda bm: set(int(p) for p in range(P) if (int(bm[t][p >> 6]) >> (p & 63)) & 1)  # noqa: E731
        al[t] = bits(fleet.allowed) if fleet.has_allowed[t] else None
        pf[t] = bits(fleet.prefer) if fleet.has_prefer[t] else None
    live = (fleet.pods["flags"] & 2) != 0
    rem = np.maximum(fleet.pods["capacity"] - fleet.pods["used"], 0)
    out = []
    for q in reqs:
        m = fleet.models[q["model"]]
        t = int(m["type"]) if T else 0
        ex = set(int(p) for p in fleet.ent_pod[m["ent_off"]: m["ent_off"] + m["n_loaded"] + m["n_failed"]])
        ex |= set(int(p) for p in extra[q["extra_off"]: q["extra_off"] + q["n_extra"]])
        el = [int(p) for p in order if live[p] and p not in ex and (al[t] is None or p in al[t])]
        if not el:
            out.append(("none", False))
            continue
        b = el[0]
        us = b == q["self_pod"]
        b_rem = max(int(q["fresh_capacity"]) - int(q["fresh_used"]), 0) if us else int(rem[b])
        b_lru = int(q["fresh_lru"]) if us else int(fleet.pods["lru_time"][b])
        full = b_rem < fleet.min_space_units
        if pf[t] is None or b in pf[t]:
            out.append(("simple", full))
        elif not full:
            kind = "a replay"
            for p in el[1:]:
                if p in pf[t]:
                    kind = "a found"
                    break
                if rem[p] < fleet.min_space_units:
                    break
            out.append((kind, full))
        else:
            kind = "b replay"
            quarter = _tdiv(_age(fleet.now, b_lru), 4)
            for p in el[1:]:
                d = int(fleet.pods["lru_time"][p]) - b_lru
                if d > 120_000 and d > quarter:
                    break
                if p in pf[t]:
                    kind = "b found"
                    break
            out.append((kind, full))
    return out


# ---- the serve choice (ForwardingLB.getNext, MM.java:4316-4391) at the edges of its value domain: tests/golden/ref_serve_edges.npz
# A ROW is one request on a model of its own; a copy is (inUse, lastUsed, loadStarted, listed).  The harness takes inUse /
# lastUsed / LIVE per INSTANCE, so a case hands out instances on demand: a copy gets the first instance behind the previous
# copy's (the entries stand in id order, and ids here are in index order) that carries its three values, else a new one; a
# case that runs out of instances is closed and the next one begun.  A PAIR is two rows of one case whose VIEW (below) differs
# in one value by one unit; the generator refuses a pair the reference decides alike in chosen and chosenTimeStamp.
SERVE_EDGE_FLEETS = (8, 65)
SERVE_NOW = wl.NOW_MS
I32_MAX, I64_MAX, I64_MIN = 2**31 - 1, 2**63 - 1, -2**63
SERVE_PAIR = np.dtype([("a", "<i4"), ("b", "<i4"), ("name", "<i4")])
SERVE_CODA = 5  # rows every case ends with: remote, self, none, a still-loading pick, an unlisted copy


class _Full(Exception):
    pass


class _ServeCase:
    def __init__(self, P):
        self.P, self.pods, self.rows, self.pairs, self.tags = P, [], [], [], []

    def pod(self, attr, after):
        for i in range(after + 1, len(self.pods)):
            if self.pods[i] == attr:
                return i
        if len(self.pods) >= self.P - 2:  # (two instances stay free for the coda)
            raise _Full()
        self.pods.append(attr)
        return len(self.pods) - 1

    def row(self, tag, copies, self_at=None, flags=0, lif=0, lit=0, assume=3000, excl=(), model=None):
        """copies: [(inUse, lastUsed, loadStarted[, listed])] in id order; self_at: which of them is the caller (None: the caller
        holds no copy); excl: [(copy index or None for an instance without a copy, time or ANY_TIME)]"""
        at, ent = -1, []
        for c in copies:
            at = self.pod((int(c[0]), int(c[1]), bool(c[3]) if len(c) > 3 else True), at)
            ent.append((at, int(c[2])))
        ex = [((ent[k][0] if k is not None else self.P - 1), int(t)) for k, t in excl]
        self.rows.append(dict(ent=ent, self_pod=ent[self_at][0] if self_at is not None else -1, flags=flags, lif=lif, lit=lit,
                              assume=assume, excl=ex, model=model))
        self.tags.append(tag)
        return len(self.rows) - 1


def _serve_groups():
    """[(rows: [(tag, kwargs)], pairs: [(name, a, b)] by position in rows)]: the tier, fleet by fleet the same"""
    T = SERVE_NOW
    done = T - 100_000  # a load long complete
    G = []

    def group(rows, pairs=()):
        G.append((rows, list(pairs)))
    # the cutoff (:4350-4352): loadStarted at cutoff - 1 / cutoff; a competitor that is complete and busier stands beside it
    for assume in (0, 3000, 2**31):
        cut = T - assume
        for idx in (0, 3, 4, 8):
            rows = []
            for d in (-1, 0):
                cp = [(5, 50, cut - 10)] * 9
                cp[idx] = (0, 50, cut + d)
                rows.append((f"cutoff/{assume}/{idx}/{d:+d}", dict(copies=cp, assume=assume)))
            group(rows, [(f"loadStarted at cutoff - 1 / cutoff, assume {assume}, copy {idx}", 0, 1)])
    # inUse against the minimum (:4354, :4358): a second copy at min - 1 / min / min + 1, less and more recently used
    for m in (0, 1, I32_MAX - 1):
        for lu2, what in ((50, "older"), (200, "newer")):
            rows = [(f"inuse/{m}/{what}/{d:+d}", dict(copies=[(m, 100, done), (m + d, lu2, done)])) for d in (-1, 0, 1) if m + d <= I32_MAX]
            pairs = [(f"inUse at min - 1 / min, min {m}, {what}", 0, 1)] if what == "newer" else []
            if what == "older" and len(rows) == 3:
                pairs = [(f"inUse at min / min + 1, min {m}, {what}", 1, 2)]
            group(rows, pairs)
    # Integer.MAX_VALUE (:4358, :4372): a complete copy at MAX_VALUE is chosen and leaves min at MAX_VALUE, so a still-loading
    # copy BEHIND it takes its place; in front of it it does not
    for first in ("complete", "loading"):
        rows = []
        for u in (I32_MAX - 1, I32_MAX):
            q, s = (u, 50, done), (0, 50, T + 5)
            rows.append((f"quirk/{first}-first/{u}", dict(copies=[q, s] if first == "complete" else [s, q])))
        group(rows, [("inUse 2^31 - 2 / 2^31 - 1 on a complete copy, a loading copy behind", 0, 1)] if first == "complete" else [])
    group([("quirk/max-and-never-used", dict(copies=[(I32_MAX, I64_MAX, done), (I32_MAX, 7, done)])),
           ("quirk/max-alone", dict(copies=[(I32_MAX, I64_MAX, done)]))])
    # lastUsed ties (:4362): equal / one below at equal inUse; the first in id order keeps a tie
    for lu in (I64_MAX, I64_MAX - 1, 0, -1, I64_MIN + 1):
        rows = [(f"tie/{lu}/{d:+d}", dict(copies=[(1, lu, done), (1, lu + d, done)])) for d in (0, -1)]
        group(rows, [(f"lastUsed equal / one below, {lu}", 1, 0)])
    # the caller as a copy (:4334-4342, :4356, :4360, :4381)
    for xs in (0, 1):  # MMP_SERVE_EXCLUDE_SELF
        for pos in (0, 1):
            other = (1, 100, done)
            for lu2, what in ((50, "older"), (200, "newer")):
                rows = []
                for lif in (0, 1, 2):
                    cp = [(9, 9, done), other] if pos == 0 else [other, (9, 9, done)]
                    rows.append((f"self/x{xs}/at{pos}/lif{lif}/{what}", dict(copies=cp, self_at=pos, flags=xs, lif=lif, lit=lu2)))
                pairs = []
                if not xs and pos == 1:
                    pairs = [(f"local_in_flight at inUse - 1 / inUse, {what}", 0, 1)] if what == "newer" else \
                        [(f"local_in_flight at inUse / + 1, {what}", 1, 2)]
                group(rows, pairs)
            rows = [(f"self/x{xs}/at{pos}/lit{d:+d}", dict(copies=[(1, 100, done), (9, 9, done)][:: 1 if pos else -1], self_at=pos,
                                                          flags=xs, lif=1, lit=100 + d)) for d in (-1, 0, 1)]
            group(rows, [("last_invoke_time one below / at the other's lastUsed", 0, 1)] if not xs and pos == 1 else [])
            rows = [(f"self/x{xs}/at{pos}/prefer/{lu}", dict(copies=[(1, lu, done), (9, 9, done)][:: 1 if pos else -1], self_at=pos,
                                                            flags=xs | 2, lif=1, lit=T)) for lu in (-1, 0, 1)]
            group(rows, [("preferSelf against a lastUsed of 0 / 1", 1, 2)] if not xs and pos == 1 else [])
        group([(f"self/x{xs}/alone", dict(copies=[(9, 9, done)], self_at=0, flags=xs)),
               (f"self/x{xs}/alone-loading", dict(copies=[(9, 9, T + 1)], self_at=0, flags=xs))])
    # still loading (:4369-4376): the earliest start, ties to the first; a complete copy in front or behind wins
    for lead in ((), ((5, 5, done),)):
        for trail in ((), ((5, 5, done),)):
            rows = [(f"loading/{len(lead)}{len(trail)}/{d:+d}", dict(copies=list(lead) + [(0, 0, T + 10), (0, 0, T + 10 + d)] + list(trail)))
                    for d in (-1, 0, 1)]
            group(rows, [("loadStarted at firstStarted - 1 / firstStarted", 0, 1)] if not lead and not trail else [])
    # exclusions (MapFilteringSet.apply, :4279-4283): the copy's load, one millisecond off, any load; exclusion index below 4 and
    # from 4 on; copy index below 4 and from 4 on
    for pad_x in (0, 4):
        for pad_c in (0, 4):
            front = [(7, 7, done)] * pad_c
            rows = []
            for t, what in ((done, "hit"), (done + 1, "miss"), (_lib.ANY_TIME, "any")):
                rows.append((f"excl/x{pad_x}/c{pad_c}/{what}", dict(copies=front + [(0, 0, done), (5, 5, done)],
                                                                   excl=[(None, _lib.ANY_TIME)] * pad_x + [(pad_c, t)])))
            group(rows, [(f"exclusion at the copy's load / one millisecond off, exclusion {pad_x}, copy {pad_c}", 0, 1)])
    group([("excl/caller", dict(copies=[(9, 9, done), (5, 5, done)], self_at=0, lif=0, excl=[(0, _lib.ANY_TIME)])),
           ("excl/only-complete", dict(copies=[(0, 0, done), (5, 5, T + 3), (5, 5, T + 2)], excl=[(0, done)])),
           ("excl/all-but-one", dict(copies=[(0, 0, done), (1, 1, done), (2, 2, done)], excl=[(0, done), (1, _lib.ANY_TIME)])),
           ("excl/all", dict(copies=[(0, 0, done), (1, 1, done)], excl=[(0, done), (1, _lib.ANY_TIME)])),
           ("excl/all-of-nine", dict(copies=[(k, k, done) for k in range(9)], excl=[(k, _lib.ANY_TIME) for k in range(9)]))])
    # listing (:4343-4346): a copy on an instance litelinks does not list is passed over
    group([("unlisted/copy0", dict(copies=[(0, 0, done, False), (5, 5, done)])),
           ("unlisted/copy5", dict(copies=[(7, 7, done)] * 5 + [(0, 0, done, False), (6, 6, done)])),
           ("unlisted/all", dict(copies=[(0, 0, done, False), (0, 0, T + 1, False)])),
           ("unlisted/caller", dict(copies=[(0, 0, done, False), (5, 5, done)], self_at=0))])
    group([("empty", dict(copies=[])), ("model/-1", dict(copies=[], model=-1)), ("model/past-the-end", dict(copies=[], model=10**6))])
    return G


def _serve_coda(c):
    T, done = SERVE_NOW, SERVE_NOW - 100_000
    c.P += 2  # the two instances kept free
    c.row("coda/remote", [(0, 0, done)])
    c.row("coda/self", [(0, 0, done)], self_at=0)
    c.row("coda/none", [(0, 0, done)], excl=[(0, done)])
    c.row("coda/loading", [(0, 0, T + 1)])
    c.row("coda/unlisted", [(0, 0, done), (0, 0, done, False)])
    c.P -= 2


def _serve_case_arrays(name, c, seed):
    P = c.P
    fleet, _ = _edge_fleet(P, seed)
    pods = c.pods + [(0, 0, True)] * (P - len(c.pods))
    fleet.pods["id_order"] = np.arange(P)
    fleet.pods["replica_set"] = -1
    fleet.pods["flags"] = [_lib_flag_live() if p[2] else 0 for p in pods]
    ids = ["s" + _b36(p, 4) for p in range(P)]
    n = len(c.rows)
    models = np.zeros(n, dtype=_lib.MODEL_ROW)
    reqs = np.zeros(n, dtype=_lib.SERVE_REQ)
    ent_pod, ent_time, xp, xt = [], [], [], []
    for i, r in enumerate(c.rows):
        models[i] = (0, len(ent_pod), len(r["ent"]), 0, fleet.now - 5_000)
        ent_pod += [p for p, _ in r["ent"]]
        ent_time += [t for _, t in r["ent"]]
        reqs[i] = (i if r["model"] is None else r["model"], r["self_pod"], r["flags"], r["lif"], r["lit"], r["assume"], len(xp),
                   len(r["excl"]), 0, 0)
        xp += [p for p, _ in r["excl"]]
        xt += [t for _, t in r["excl"]]
    fleet.models, fleet.ent_pod, fleet.ent_time = models, np.array(ent_pod, np.int32), np.array(ent_time, np.int64)
    in_use = np.array([p[0] for p in pods], np.int32)
    last_used = np.array([p[1] for p in pods], np.int64)
    tag_names = sorted(set(c.tags))
    pair_names = sorted({p[0] for p in c.pairs})
    meta = {"tags": np.array([tag_names.index(t) for t in c.tags], np.int32), "tag_names": np.array(tag_names),
            "pairs": np.array([(a, b, pair_names.index(nm)) for nm, a, b in c.pairs], dtype=SERVE_PAIR),
            "pair_names": np.array(pair_names) if pair_names else np.zeros(0, "<U1")}
    return name, fleet, ids, reqs, in_use, last_used, np.array(xp, np.int32), np.array(xt, np.int64), meta


@functools.lru_cache(maxsize=1)
def _serve_edge_all():
    out = []
    for P in SERVE_EDGE_FLEETS:
        cases, cur = [], _ServeCase(P)
        for rows, pairs in _serve_groups():
            if P == 8 and any(len(kw["copies"]) > 6 for _, kw in rows):
                continue  # (a model of nine copies needs the larger fleet)
            for attempt in (0, 1):
                mark = (len(cur.pods), len(cur.rows), len(cur.pairs))
                try:
                    at = [cur.row(tag, **kw) for tag, kw in rows]
                    cur.pairs += [(nm, at[a], at[b]) for nm, a, b in pairs]
                    break
                except _Full:
                    assert attempt == 0, ("a group that no empty case holds", rows[0][0])
                    del cur.pods[mark[0]:], cur.rows[mark[1]:], cur.tags[mark[1]:], cur.pairs[mark[2]:]
                    cases.append(cur)
                    cur = _ServeCase(P)
        cases.append(cur)
        for k, c in enumerate(cases):
            _serve_coda(c)
            out.append(_serve_case_arrays(f"serve_edges_{P}_{k}", c, 70 + k))
    return out


def serve_edge_cases():
    """(name, fleet, ids, reqs, in_use, last_used, excl_pod, excl_time, meta): meta = tags, tag_names, pairs, pair_names"""
    return _serve_edge_all()


def serve_row_view(fleet, reqs, in_use, last_used, xp, xt, i):
    """everything request i hands ForwardingLB.getNext, as a flat tuple of integers: per copy in id order (is the caller,
    listed, inUse, lastUsed, loadStarted), then flags, local_in_flight, last_invoke_time, assume_completed_ms and per exclusion
    (the copy it names or -1, any-time, time)"""
    r = reqs[i]
    v = []
    pods = []
    if 0 <= r["model"] < len(fleet.models):
        m = fleet.models[r["model"]]
        for e in range(int(m["ent_off"]), int(m["ent_off"] + m["n_loaded"])):
            p = int(fleet.ent_pod[e])
            pods.append(p)
            v += [int(p == r["self_pod"]), int((fleet.pods["flags"][p] & 2) != 0), int(in_use[p]), int(last_used[p]), int(fleet.ent_time[e])]
    v += [int(r["flags"]), int(r["local_in_flight"]), int(r["last_invoke_time"]), int(r["assume_completed_ms"])]
    for k in range(int(r["excl_off"]), int(r["excl_off"] + r["n_excl"])):
        anyt = int(xt[k]) == _lib.ANY_TIME
        v += [pods.index(int(xp[k])) if int(xp[k]) in pods else -1, int(anyt), 0 if anyt else int(xt[k])]
    return tuple(v)


def serve_edge_occurrence(fleet, reqs, xp, xt, serve):
    """{an outcome or a branch of the loop: whether some row of the case takes it}, from the inputs and the reference's answers"""
    now = int(fleet.now)
    occ = {"remote": bool((serve[:, 0] >= 0).any()), "self": bool((serve[:, 0] == _lib.MMP_SELF).any()),
           "none": bool((serve[:, 0] == _lib.MMP_NONE).any()), "a complete copy chosen": False, "a still-loading copy chosen": False,
           "a copy excluded": False, "an unlisted copy": False, "the caller among the copies": False}
    for i, r in enumerate(reqs):
        if not 0 <= r["model"] < len(fleet.models):
            continue
        m = fleet.models[r["model"]]
        pods = fleet.ent_pod[m["ent_off"]: m["ent_off"] + m["n_loaded"]]
        times = fleet.ent_time[m["ent_off"]: m["ent_off"] + m["n_loaded"]]
        cutoff = now - int(r["assume_completed_ms"])
        if serve[i, 0] != _lib.MMP_NONE:
            occ["a complete copy chosen" if serve[i, 1] < cutoff else "a still-loading copy chosen"] = True
        occ["an unlisted copy"] |= bool(((fleet.pods["flags"][pods] & 2) == 0).any())
        occ["the caller among the copies"] |= bool((pods == r["self_pod"]).any())
        for k in range(int(r["excl_off"]), int(r["excl_off"] + r["n_excl"])):
            occ["a copy excluded"] |= bool(((pods == xp[k]) & ((xt[k] == _lib.ANY_TIME) | (times == xt[k]))).any())
    return occ


def type_edge_cases():
    """(name, fleet, ids, pod_bits, req_bits, pref_bits, meta): the type-constraint kernels at the edges of their value domain
    (tests/ref_type_edges.py, tests/golden/ref_type_edges.npz)"""
    from tests import ref_type_edges
    return ref_type_edges.type_edge_cases()
