"""GPU: serve_eval (aux_kernels.hpp) at the edges of its value domain, through every caller, held to the REFERENCE'S OWN TEXT —
tests/golden/ref_serve_edges.npz, see tests/test_ref_serve_edges.py: mmp_serve_batch whole and in slot-sized pieces,
mmp_route_batch whole and one request per call (route_single_kernel for a request with at most four counters, route_batch_kernel
on a slot beyond), mmp_route_batch_c for the rows that share a caller.  The counters go in as the case lists them: one entry per
copy on a listed instance, in copy order.  Exact: chosen on every row, chosen_load_start wherever an instance is chosen."""
import os

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd.solver import Solver
from tests import ref_fleets as rf
from tests import seam_caller_model as scm

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_serve_edges.npz")
SLOT_BATCH = 128  # rows per call of the slot-sized pieces: within every latency slot
ROUTE_INLINE_COUNTERS = 4  # kRouteInlineCnt (gate_kernel.hpp): one route with at most this many counters rides route_single_kernel
CASES = {c[0]: c for c in rf.serve_edge_cases()}


@pytest.fixture(scope="module")
def ref():
    return np.load(GOLDEN)


def _check(what, got, want, rows=None):
    want = want if rows is None else want[rows]
    assert np.array_equal(got["chosen"], want[:, 0]), (what, np.nonzero(got["chosen"] != want[:, 0])[0][:5])
    picked = want[:, 0] != _lib.MMP_NONE  # (the reference reports the caller's own timestamp as well: tried.add comes first here)
    remote = want[:, 0] >= 0
    assert np.array_equal(got["chosen_load_start"][remote], want[remote, 1]), what
    assert (got["chosen_load_start"][~picked] == 0).all(), what


def _subset(sreqs, counters, xp, xt, rows):
    """the requests `rows` with pools of their own"""
    sr = np.ascontiguousarray(sreqs[rows]).copy()
    cnt, ep, et = [], [], []
    for k in range(len(sr)):
        a, n = int(sr["cnt_off"][k]), int(sr["n_cnt"][k])
        sr["cnt_off"][k] = sum(len(c) for c in cnt)
        cnt.append(counters[a:a + n])
        a, n = int(sr["excl_off"][k]), int(sr["n_excl"][k])
        sr["excl_off"][k] = sum(len(e) for e in ep)
        ep.append(xp[a:a + n]), et.append(xt[a:a + n])
    return (sr, np.concatenate(cnt) if cnt else np.zeros(0, _lib.SERVE_COUNTER), np.concatenate(ep).astype(np.int32),
            np.concatenate(et).astype(np.int64))


def _gates(sr):
    g = np.zeros(len(sr), dtype=_lib.GATE_REQ)  # guards of a request that asks for nothing but the route
    g["model"], g["self_pod"] = sr["model"], sr["self_pod"]
    g["excl_off"], g["n_excl"] = sr["excl_off"], sr["n_excl"]
    g["loaded_time"] = -1
    return g


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_caller_of_serve_eval_equals_the_reference_text_at_the_edges(ref, name):
    _, fleet, ids, reqs, in_use, last_used, xp, xt, meta = CASES[name]
    want = ref[f"{name}/serve"]
    none = np.zeros(0, np.int32)
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    try:
        s.load_fleet(fleet)
        sreqs, counters = s.serve_counters(reqs, in_use, last_used)
        # the counters are what the case says: one per copy on a listed instance, in copy order
        for i, r in enumerate(sreqs):
            if 0 <= r["model"] < len(fleet.models):
                m = fleet.models[r["model"]]
                pods = fleet.ent_pod[m["ent_off"]: m["ent_off"] + m["n_loaded"]]
                pods = pods[(fleet.pods["flags"][pods] & 2) != 0]
                c = counters[r["cnt_off"]: r["cnt_off"] + r["n_cnt"]]
                assert np.array_equal(c["pod"], pods) and np.array_equal(c["in_use"], in_use[pods]) and np.array_equal(c["last_used"], last_used[pods])
        _check((name, "mmp_serve_batch, whole"), s.serve_k(sreqs, counters, xp, xt, fleet.now), want)
        _, got = s.route(_gates(sreqs), sreqs, counters, xp, xt, none, fleet.now)
        _check((name, "mmp_route_batch, whole"), got, want)
        for a in range(0, len(sreqs), SLOT_BATCH):
            rows = np.arange(a, min(a + SLOT_BATCH, len(sreqs)))
            sr, cnt, ep, et = _subset(sreqs, counters, xp, xt, rows)
            _check((name, "mmp_serve_batch on a slot", a), s.serve_k(sr, cnt, ep, et, fleet.now), want, rows)
        # one request per call
        single = np.zeros(len(sreqs), bool)
        for i in range(len(sreqs)):
            sr, cnt, ep, et = _subset(sreqs, counters, xp, xt, np.array([i]))
            single[i] = len(cnt) <= ROUTE_INLINE_COUNTERS
            _, got = s.route(_gates(sr), sr, cnt, ep, et, none, fleet.now)
            _check((name, "mmp_route_batch, one request", i), got, want, np.array([i]))
            _check((name, "mmp_serve_batch, one request", i), s.serve_k(sr, cnt, ep, et, fleet.now), want, np.array([i]))
        # route_single_kernel takes the rows with at most four counters: every pair whose models have at most four copies
        small = fleet.models["n_loaded"][np.clip(reqs["model"], 0, len(fleet.models) - 1)] <= ROUTE_INLINE_COUNTERS
        assert single[small].all() and single.any()
        for p in meta["pairs"]:
            if small[p["a"]] and small[p["b"]]:
                assert single[p["a"]] and single[p["b"]]
        # the rows that share a caller, in the single-caller form
        key = np.stack([reqs["self_pod"], reqs["local_in_flight"], reqs["last_invoke_time"]], axis=1)
        n_c = 0
        for k in np.unique(key, axis=0):
            rows = np.nonzero((key == k).all(axis=1))[0]
            sr, cnt, ep, et = _subset(sreqs, counters, xp, xt, rows)
            caller = np.zeros(1, dtype=_lib.SEAM_CALLER)
            caller["self_pod"], caller["local_in_flight"], caller["last_invoke_time"] = int(k[0]), int(k[1]), int(k[2])
            g = np.zeros(len(rows), dtype=_lib.GATE_REQ_C)
            g["model"], g["excl_off"], g["n_excl"], g["loaded_time"] = sr["model"], sr["excl_off"], sr["n_excl"], -1
            _, got = s.route_c(caller, g, scm.serve_request_side(sr), cnt, ep, et, none, fleet.now)
            _check((name, "mmp_route_batch_c", tuple(int(x) for x in k)), got, want, rows)
            n_c += len(rows)
        assert n_c == len(reqs)
    finally:
        s.close()
