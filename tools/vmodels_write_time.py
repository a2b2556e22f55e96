"""Device span and call wall of mmp_vmodels_write_json and mmp_models_refs_json over a registry of 100 000 models named by key, at
n = 1, 64, 4 096 and 20 000 requests, beside the host path they replace: json.loads of every stored value, the edit, json.dumps.

    python tools/vmodels_write_time.py [--sizes 1,64,4096,20000] [--repeats 7]

A write batch is one third forced SETs onto a vmodel in transition (the active model switches: two ids lose a referent), one third
COMPLETEs and one third DELETEs, every request on a stored VModelRecord of its own; a refs batch is an INC and a DEC in turn on the
stored ModelRecord of a model of its own.  Each call is timed as its write call (the buffer sized by one call before) and as its
sizes-only call.  One JSON line per size: medians over `repeats` calls after 2 warm-up calls, device span (mmp_profile /
mmp_last_kernel_ms) and wall time in microseconds."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modelmesh_amd import _lib  # noqa: E402
from modelmesh_amd import wire  # noqa: E402
from modelmesh_amd import workload as wl  # noqa: E402
from modelmesh_amd.solver import Solver  # noqa: E402

AGE = 3_600_000
M = 100_000


def timed(s, fn, repeats, warmup=2):
    wall, span = [], []
    for k in range(warmup + repeats):
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if k >= warmup:
            wall.append(1e6 * (t1 - t0))
            span.append(1e3 * s.last_kernel_ms() if s is not None else 0.0)
    return round(float(np.median(span)), 1), round(float(np.median(wall)), 1)


def host_write(olds, reqs, strs):
    """What the Java does per attempt, in Python: parse, edit the bean, serialise."""
    out = []
    for old, (op, _), (ida, _idb, _o) in zip(olds, reqs, strs):
        d = json.loads(old)
        if op == _lib.VW_DELETE:
            continue
        d["amid"] = d["tmid"] = ida.decode() if op == _lib.VW_SET else d["tmid"]
        d.pop("failed", None)
        out.append(json.dumps(d, separators=(",", ":")))
    return out


def host_refs(olds, reqs):
    out = []
    for old, (flags, _r, lu) in zip(olds, reqs):
        d = json.loads(old)
        if flags & _lib.MREF_INC:
            d["refs"], d["lu"] = d.get("refs", 0) + 1, int(lu)
        elif d.get("refs", 0) > 0:
            d["refs"] -= 1
        out.append(json.dumps(d, separators=(",", ":")))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,64,4096,20000")
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    rng = np.random.default_rng(0xC3)
    fleet = wl.make_fleet("C3")
    assert fleet.n_models >= M
    ids = wire.make_ids(rng, fleet.n_pods)
    wire.adopt_ids(fleet, ids)
    type_names = ["NLCLASSIFIER"] + ["type-%d" % t for t in range(1, max(fleet.n_types, 1))]
    values = [v.encode() for v in wire.model_values(fleet, ids, type_names, rng, np.zeros(fleet.n_models, np.int64))][:M]
    keys = [b"model-%06d" % k for k in range(M)]
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    s.load_pod_ids(ids)
    s.load_pods(fleet.pods)
    s.load_types(fleet.n_types, fleet.allowed, fleet.prefer, fleet.has_allowed, fleet.has_prefer)
    s.load_type_names(type_names, 0)
    s.commit()
    assert not len(s.ingest_models_json([])[0])
    s.model_ids_load([])
    status, _, _, n_app = s.models_events_json(keys, values, None, True)
    assert not status.any() and n_app == M
    now = int(fleet.now)
    s.profile(True)
    for n in (int(x) for x in a.sizes.split(",")):
        pick = rng.permutation(M)[:3 * n].reshape(n, 3)
        olds = [b'{"o":"owner-%d","amid":"%s","tmid":"%s","failed":true}' % (i % 7, keys[x], keys[y]) for i, (x, y, _) in enumerate(pick)]
        ops = np.arange(n) % 3
        reqs = np.zeros(n, _lib.VMODEL_WRITE_REQ)
        reqs["op"] = np.choose(ops, [_lib.VW_SET, _lib.VW_COMPLETE, _lib.VW_DELETE])
        reqs["flags"] = np.where(ops == 0, _lib.VWQ_FORCE, 0)
        strs = [(keys[z], b"", b"") if o == 0 else (keys[y], keys[x], b"") if o == 1 else (b"", b"", b"") for o, (x, y, z) in zip(ops, pick)]
        args = (reqs, strs, olds, now, AGE, b"")
        r = s.vmodels_write_json_raw(*args, 0)
        total = r[3]
        counts = np.bincount(r[2]["cls"], minlength=12)
        assert r[4] == 0 and counts[_lib.VWC_UPDATED] + counts[_lib.VWC_DELETE] == n, counts
        mvals = [values[x] for x, _, _ in pick]
        rreqs = np.zeros(n, _lib.REFS_REQ)
        rreqs["flags"] = np.where(np.arange(n) % 2 == 0, _lib.MREF_INC, 0)
        rreqs["last_used"] = now
        rr = s.models_refs_json_raw(rreqs, mvals, None, 0)
        rtotal = rr[4]
        assert rr[5] == 0 and (rr[2] == _lib.MREFC_SET).all()

        def write():
            assert s.vmodels_write_json_raw(*args, total)[4] == 0

        def sizes():
            assert s.vmodels_write_json_raw(*args, 0, null_out=True)[4] == 0

        def refs():
            assert s.models_refs_json_raw(rreqs, mvals, None, rtotal)[5] == 0

        def refs_sizes():
            assert s.models_refs_json_raw(rreqs, mvals, None, 0, null_out=True)[5] == 0
        w_span, w_wall = timed(s, write, a.repeats)
        z_span, z_wall = timed(s, sizes, a.repeats)
        f_span, f_wall = timed(s, refs, a.repeats)
        fz_span, fz_wall = timed(s, refs_sizes, a.repeats)
        _, hw_wall = timed(None, lambda: host_write(olds, list(zip(reqs["op"], reqs["flags"])), strs), a.repeats)
        _, hf_wall = timed(None, lambda: host_refs(mvals, rreqs.tolist()), a.repeats)
        print(json.dumps({"models": M, "requests": n, "updated": int(counts[_lib.VWC_UPDATED]), "deleted": int(counts[_lib.VWC_DELETE]),
                          "write_bytes_in": sum(map(len, olds)), "write_bytes_out": int(total), "write_device_us": w_span,
                          "write_wall_us": w_wall, "write_sizes_only_device_us": z_span, "write_sizes_only_wall_us": z_wall,
                          "host_json_write_wall_us": hw_wall, "refs_bytes_in": sum(map(len, mvals)), "refs_bytes_out": int(rtotal),
                          "refs_device_us": f_span, "refs_wall_us": f_wall, "refs_sizes_only_device_us": fz_span,
                          "refs_sizes_only_wall_us": fz_wall, "host_json_refs_wall_us": hf_wall}), flush=True)
    s.close()


if __name__ == "__main__":
    main()
