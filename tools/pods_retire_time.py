"""Device span and call wall of mmp_pods_retire on C3 (10k pods x 100k models) with 1 %, 10 % and 50 % of the instances
tombstoned and pruned, beside the route a host has for the same result without it:

    mmp_pods_retire of the gone instances    beside    mmp_pod_ids_load + mmp_pods_ingest_json of the survivors
                                                        + (mmp_types_load) + mmp_models_ingest_json + mmp_model_ids_load
                                                        + mmp_snapshot_commit

    python tools/pods_retire_time.py [--repeats 5]

Before every timed retire the whole state is built again (not timed): ids, instances, registry, model ids, types, commit; the gone
instances are deleted by key and committed; one reaper pass marks them and one past gone_after_ms removes their registrations.
Both routes are timed at the C boundary, the reload with every value ALREADY packed — the host work of holding and packing the stored
values, which the retire takes away, is not in its wall.  It loses the `missings` marks, the label words and the replica-set
interning; the retire keeps them.

One JSON line per route and share: medians over `repeats` calls after 1 warm-up call, both routes alternating in one session.
device_us: mmp_profile / mmp_last_kernel_ms (the retire's includes its commit stage; the reload's is the sum of its calls' spans,
calls without a kernel add nothing); commit_us: the span of a from-scratch commit of the same table on its own; wall_us: the
call(s), both routes at the C boundary.  Then the P-dependent numbers before and after the 50 % retire: the from-scratch commit's span and the census's."""
import argparse
import ctypes as C
import json
import os
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modelmesh_amd import wire  # noqa: E402
from modelmesh_amd import workload as wl  # noqa: E402
from modelmesh_amd._lib import ptr  # noqa: E402
from modelmesh_amd.solver import Solver, bitmap_from_bool  # noqa: E402

GONE_AFTER = 600_000


def median_us(xs):
    return round(float(np.median(xs)), 1)


def scratch_commit_us(ctx):
    """a from-scratch commit of the staged table as it stands (the rows are loaded onto themselves)"""
    ctx.load_pods(ctx.get_pods())
    ctx.commit()
    return 1e3 * ctx.last_kernel_ms()


def census_us(ctx):
    ctx.registry_census()
    return 1e3 * ctx.last_kernel_ms()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    rng = np.random.default_rng(0xC3)
    fleet = wl.make_fleet("C3")
    M, P, now = fleet.n_models, fleet.n_pods, int(fleet.now)
    ids = wire.make_ids(rng, P)
    wire.adopt_ids(fleet, ids)
    type_names = ["NLCLASSIFIER"] + ["type-%d" % t for t in range(1, max(fleet.n_types, 1))]
    pv = [v.encode() for v in wire.pod_values(fleet, rng, np.zeros(P, np.int64))]
    mv = [v.encode() for v in wire.model_values(fleet, ids, type_names, rng, np.zeros(M, np.int64))]
    mids = [b"model-%07d-%05x" % (i, int(x)) for i, x in enumerate(rng.integers(0, 16**5, M))]
    T = fleet.n_types
    bits = None
    if T:
        unpack = lambda w: np.unpackbits(w.view(np.uint8), bitorder="little").reshape(T, -1)[:, :P].astype(bool)  # noqa: E731
        bits = (unpack(fleet.allowed), unpack(fleet.prefer))

    s, t = (Solver(fleet.min_space_units, fleet.min_churn_age_ms) for _ in range(2))
    for ctx in (s, t):
        ctx.profile(True)
        ctx.load_type_names(type_names, 0)
    L = s.lib

    def build():
        s.load_pod_ids(ids)
        assert not s.ingest_pods_json(pv, np.arange(P, dtype=np.int32))[0].any()
        assert not s.ingest_models_json(mv)[0].any()
        s.model_ids_load(mids)
        s.load_types(T, fleet.allowed, fleet.prefer, fleet.has_allowed, fleet.has_prefer)
        s.commit()

    def leave(gone):
        keys = [ids[p] for p in gone]
        assert not s.pods_events_json(keys, [""] * len(keys), deleted=np.ones(len(keys), np.uint8))[0].any()
        s.commit()
        s.prune_registry(0, now + 1000)
        s.prune_registry(0, now + 1000 + GONE_AFTER + 1)

    for share in (0.01, 0.10, 0.50):
        gone = np.sort(rng.choice(np.arange(1, P), int(P * share), replace=False)).astype(np.int32)  # (instance 0 is the reaper's own)
        keep = np.ones(P, bool)
        keep[gone] = False
        n_keep = int(keep.sum())
        # the survivors' stored values, packed: ids, instance records, the registry as the prune left it, the type rows
        build()
        p0_commit, p0_census = 1e3 * s.last_kernel_ms(), census_us(s)
        leave(gone)
        rows, ep, et = s.get_models()
        left = [ids[p] for p in np.nonzero(keep)[0]]
        new_of = np.cumsum(keep) - 1
        part = types.SimpleNamespace(models=rows, ent_pod=new_of[ep].astype(np.int32), ent_time=et)
        mv1 = [v.encode() for v in wire.model_values(part, left, type_names, rng, np.zeros(M, np.int64))]
        iblob, ioff = Solver._pack(left)
        pblob, poff = Solver._pack([pv[p] for p in np.nonzero(keep)[0]])
        mblob, moff = Solver._pack(mv1)
        kblob, koff = Solver._pack(mids)
        ioff32, koff32, pidx = ioff.astype(np.int32), koff.astype(np.int32), np.arange(n_keep, dtype=np.int32)
        pstatus, mstatus, lul = np.zeros(n_keep, np.int32), np.zeros(M, np.int32), np.zeros(M, np.int64)
        al = pf = None
        if T:
            al, pf = bitmap_from_bool(bits[0][:, keep]), bitmap_from_bool(bits[1][:, keep])
        span, wall, cspan, rspan, rcspan, rwall = [], [], [], [], [], []
        for k in range(1 + a.repeats):
            if k:
                build()
                leave(gone)
            remap, after, turned = np.zeros(P, np.int32), C.c_int32(0), C.c_int64(0)
            t0 = time.perf_counter()
            rc = L.mmp_pods_retire(s.h, ptr(gone), len(gone), 3, ptr(remap), P, C.byref(after), C.byref(turned))  # both guards
            t1 = time.perf_counter()
            ms = s.last_kernel_ms()
            assert rc == 0 and after.value == n_keep and turned.value == 0 and int((remap >= 0).sum()) == n_keep
            s.n_pods = n_keep  # (the wrapper was bypassed)
            p1_commit, p1_census = scratch_commit_us(s), census_us(s)
            spans = []
            t2 = time.perf_counter()
            rcs = [L.mmp_pod_ids_load(t.h, iblob, ptr(ioff32), n_keep, None, None)]
            spans.append(t.last_kernel_ms())
            rcs.append(L.mmp_pods_ingest_json(t.h, pblob, ptr(poff), n_keep, ptr(pidx), None, None, ptr(pstatus)))
            spans.append(t.last_kernel_ms())
            if T:
                rcs.append(L.mmp_types_load(t.h, T, ptr(al), ptr(pf), ptr(fleet.has_allowed), ptr(fleet.has_prefer)))
            rcs.append(L.mmp_models_ingest_json(t.h, mblob, ptr(moff), M, ptr(lul), ptr(mstatus)))
            spans.append(t.last_kernel_ms())
            rcs.append(L.mmp_model_ids_load(t.h, kblob, ptr(koff32), M))
            spans.append(t.last_kernel_ms())
            rcs.append(L.mmp_snapshot_commit(t.h))
            t3 = time.perf_counter()
            spans.append(t.last_kernel_ms())
            assert not any(rcs) and not pstatus.any() and not mstatus.any(), rcs
            t.n_pods = n_keep  # (the wrapper was bypassed)
            assert np.array_equal(s.order(), t.order())
            if k:
                span.append(1e3 * ms if ms >= 0 else -1.0)
                cspan.append(p1_commit)
                wall.append(1e6 * (t1 - t0))
                rspan.append(1e3 * sum(x for x in spans if x >= 0))
                rcspan.append(1e3 * spans[-1])
                rwall.append(1e6 * (t3 - t2))
        print(json.dumps({"route": "mmp_pods_retire", "fleet": "C3", "pods": P, "retired": len(gone), "device_us": median_us(span),
                          "commit_us": median_us(cspan), "wall_us": median_us(wall)}), flush=True)
        print(json.dumps({"route": "reload of the survivors", "fleet": "C3", "pods": P, "retired": len(gone), "device_us": median_us(rspan),
                          "commit_us": median_us(rcspan), "wall_us": median_us(rwall)}), flush=True)
        if share == 0.50:
            print(json.dumps({"fleet": "C3", "pods_before": P, "pods_after": n_keep, "scratch_commit_us": [round(p0_commit, 1), round(p1_commit, 1)],
                              "census_us": [round(p0_census, 1), round(p1_census, 1)]}), flush=True)
    s.close()
    t.close()


if __name__ == "__main__":
    main()
