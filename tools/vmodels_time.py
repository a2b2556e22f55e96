"""Device span and call wall of the vmodel calls on C3-sized state (10k pods x 100k models, 20 000 vmodels, a tenth of them in
transition), each beside the route a host has without them, measured in the same run:

    mmp_vmodels_events_json of 1 / 256 / 4 096 / 20 000 events
    mmp_vmodels_resolve of 1 / 256 / 100 000 keys   beside  a Python dict from vmodel id to active id filled from json.loads,
                                                            then mmp_model_ids_resolve of the active ids
    mmp_vmodels_transitions                         beside  the numpy form (tests/vmodel_model.py: transitions_numpy) over
                                                            mmp_models_get and host arrays of the vmodels' registry rows

    python tools/vmodels_time.py [--repeats 7]

One JSON line per route: medians over `repeats` calls after 1 warm-up call, device span (mmp_profile / mmp_last_kernel_ms; -1
where the route brackets no kernel of its own) and wall time of the call as a Python host makes it — packing the keys included,
on both sides — in microseconds."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modelmesh_amd import wire  # noqa: E402
from modelmesh_amd import workload as wl  # noqa: E402
from modelmesh_amd.solver import Solver  # noqa: E402
from tests import vmodel_model as vm  # noqa: E402

NOW, AGE = 1_700_000_000_000, 600_000


def timed(s, fn, repeats, warmup=1):
    wall, span = [], []
    for k in range(warmup + repeats):
        t0 = time.perf_counter()
        fn(k)
        t1 = time.perf_counter()
        if k >= warmup:
            wall.append(1e6 * (t1 - t0))
            ms = s.last_kernel_ms()
            span.append(1e3 * ms if ms >= 0 else -1.0)
    return round(float(np.median(span)), 1), round(float(np.median(wall)), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--vmodels", type=int, default=20000)
    a = ap.parse_args()
    rng = np.random.default_rng(0xC3)
    fleet = wl.make_fleet("C3")
    M, P, V = fleet.n_models, fleet.n_pods, a.vmodels
    ids = wire.make_ids(rng, P)
    wire.adopt_ids(fleet, ids)
    type_names = ["NLCLASSIFIER"] + ["type-%d" % t for t in range(1, max(fleet.n_types, 1))]
    mv = [v.encode() for v in wire.model_values(fleet, ids, type_names, rng, np.zeros(M, np.int64))]
    mids = [b"model-%07d-%05x" % (i, int(x)) for i, x in enumerate(rng.integers(0, 16**5, M))]
    vids = [b"vmodel-%06d-%04x" % (i, int(x)) for i, x in enumerate(rng.integers(0, 16**4, V))]
    active = rng.integers(0, M, V)
    target = np.where(rng.random(V) < 0.1, rng.integers(0, M, V), active)  # a tenth in transition

    def value(v, gen=0):
        return vm.render(mids[active[v]].decode(), mids[target[v]].decode(), "owner-%d" % (v % 97 + gen), failed=bool(v % 31 == 0)).encode()

    def line(route, n, span, wall):
        print(json.dumps({"route": route, "fleet": "C3", "vmodels": V, "n": n, "device_us": span, "wall_us": wall}), flush=True)

    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    s.profile(True)
    s.load_pod_ids(ids)
    s.load_type_names(type_names, 0)
    assert not s.ingest_models_json(mv)[0].any()
    s.model_ids_load(mids)
    st, _, n_app = s.vmodels_events_json(vids, [value(v) for v in range(V)])  # start-up: one batch with APPEND
    assert not st.any() and n_app == V

    for n in (1, 256, 4096, V):
        which = rng.integers(0, V, n) if n < V else np.arange(V)
        keys = [vids[v] for v in which]
        vals = [[value(v, g) for v in which] for g in range(2)]
        line("mmp_vmodels_events_json", n, *timed(s, lambda k: s.vmodels_events_json(keys, vals[k % 2]), a.repeats))

    # the host route: the listener's json.loads fills a dict once (not timed); a request then costs a lookup and an id resolve
    active_of = {vids[v]: json.loads(value(v))["amid"].encode() for v in range(V)}
    for n in (1, 256, 100000):
        keys = [vids[v] for v in rng.integers(0, V, n)]
        line("mmp_vmodels_resolve", n, *timed(s, lambda k: s.vmodels_resolve(keys), a.repeats))
        line("dict + mmp_model_ids_resolve", n, *timed(s, lambda k: s.model_ids_resolve([active_of[x] for x in keys]), a.repeats))
        assert np.array_equal(s.vmodels_resolve(keys)["model"], s.model_ids_resolve([active_of[x] for x in keys]))

    line("mmp_vmodels_transitions", V, *timed(s, lambda k: s.vmodels_transitions(NOW, AGE), a.repeats))
    # the numpy form: the host keeps the vmodels' registry rows (refreshed by its listeners, not timed) and reads the registry back
    listed = active != target
    arow, trow, failed = active.astype(np.int32), target.astype(np.int32), np.arange(V) % 31 == 0
    out = []

    def numpy_form(k):
        rows = s.get_models()[0]
        empty = (rows["type"] == 0) & (rows["n_loaded"] == 0) & (rows["n_failed"] == 0) & (rows["last_used"] == 0)
        out[:] = [vm.transitions_numpy(listed, arow, trow, failed, rows["n_loaded"], rows["last_used"], empty, NOW, AGE)]

    span, wall = timed(s, numpy_form, a.repeats)
    line("numpy over mmp_models_get", V, -1.0, wall)
    assert out[0].tobytes() == s.vmodels_transitions(NOW, AGE)[0].tobytes()
    print(json.dumps({"vmodels_info": {k: int(s.vmodels_info()[k]) for k in ("n_rows", "n_live", "arena_bytes", "live_bytes", "capacity")}}))
    s.close()


if __name__ == "__main__":
    main()
