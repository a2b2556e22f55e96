"""The serve choice (ForwardingLB.getNext, MM.java:4316-4391) at the edges of its value domain, held to the REFERENCE'S OWN TEXT:
tests/golden/ref_serve_edges.npz is what the method body, compiled as it stands by oracle/ref_harness, decides on
tests/ref_fleets.serve_edge_cases() (regenerate with oracle/ref_harness/make_ref_vectors.py --serve-edges).  Here: the premises
of the cases, asserted from the inputs, and both restatements — oracle/mm_oracle.c (orc_serve) and oracle/py_oracle.py
(serve_get_next) — row by row.  The device is held to the same file in tests/test_ref_serve_edges_gpu.py.  Nothing here needs
the reference tree."""
import os

import numpy as np
import pytest

from modelmesh_amd import _lib
from oracle import bind as ob
from oracle import py_oracle as po
from tests import ref_fleets as rf

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_serve_edges.npz")


@pytest.fixture(scope="module")
def ref():
    return np.load(GOLDEN)


def _filtered(fleet, r, xp, xt):
    """the copies MapFilteringSet lets through (:4279-4283), in id order"""
    if not 0 <= r["model"] < len(fleet.models):
        return np.zeros(0, np.int32), np.zeros(0, np.int64)
    mm = fleet.models[r["model"]]
    pods = fleet.ent_pod[mm["ent_off"]: mm["ent_off"] + mm["n_loaded"]]
    times = fleet.ent_time[mm["ent_off"]: mm["ent_off"] + mm["n_loaded"]]
    keep = np.ones(len(pods), bool)
    for j in range(r["n_excl"]):
        p, t = xp[r["excl_off"] + j], xt[r["excl_off"] + j]
        keep &= ~((pods == p) & ((t == _lib.ANY_TIME) | (times == t)))
    return pods[keep], times[keep]


def test_the_file_holds_the_generators_cases(ref):
    cases = rf.serve_edge_cases()
    assert [c[0] for c in cases] == [str(n) for n in ref["names"]]
    assert {c[1].n_pods for c in cases} == set(rf.SERVE_EDGE_FLEETS)
    for name, fleet, ids, reqs, in_use, last_used, xp, xt, meta in cases:
        assert rf.digest(rf.input_blob(fleet, ids, serve=(reqs, in_use, last_used, xp, xt))) == bytes(ref[f"{name}/digest"]).decode(), name
        assert len(ref[f"{name}/serve"]) == len(reqs)
        n = fleet.models["n_loaded"]
        assert n.max() <= 9 and (np.diff(fleet.pods["id_order"]) == 1).all()
        for m in fleet.models:  # the entries stand in id order
            assert (np.diff(fleet.ent_pod[m["ent_off"]: m["ent_off"] + m["n_loaded"]]) > 0).all()
    assert {int(k) for c in cases if c[1].n_pods == 65 for k in c[1].models["n_loaded"]} >= {0, 1, 2, 3, 4, 6, 7, 9}  # 1 to 9 copies


def test_every_pair_differs_by_one_unit_in_one_value_and_is_decided(ref):
    n = 0
    for name, fleet, ids, reqs, in_use, last_used, xp, xt, meta in rf.serve_edge_cases():
        serve = ref[f"{name}/serve"]
        for p in meta["pairs"]:
            va = rf.serve_row_view(fleet, reqs, in_use, last_used, xp, xt, int(p["a"]))
            vb = rf.serve_row_view(fleet, reqs, in_use, last_used, xp, xt, int(p["b"]))
            what = (name, str(meta["pair_names"][p["name"]]))
            diff = [k for k in range(len(va)) if va[k] != vb[k]]
            assert len(va) == len(vb) and len(diff) == 1 and abs(va[diff[0]] - vb[diff[0]]) == 1, (what, diff)
            assert tuple(serve[p["a"]]) != tuple(serve[p["b"]]), what
            n += 1
    assert n == 54


def test_every_case_holds_every_outcome_and_branch(ref):
    tags = set()
    for name, fleet, ids, reqs, in_use, last_used, xp, xt, meta in rf.serve_edge_cases():
        occ = rf.serve_edge_occurrence(fleet, reqs, xp, xt, ref[f"{name}/serve"])
        assert all(occ.values()), (name, [k for k, ok in occ.items() if not ok])
        tags |= {str(meta["tag_names"][t]).split("/")[0] for t in meta["tags"]}
    assert tags == {"cutoff", "inuse", "quirk", "tie", "self", "loading", "excl", "unlisted", "empty", "model", "coda"}


def test_the_integer_max_value_quirk_is_in_the_vectors(ref):
    """A complete copy whose inUse is Integer.MAX_VALUE is chosen and leaves `min` at MAX_VALUE: a still-loading copy behind it
    takes its place (:4372); at MAX_VALUE - 1 it does not."""
    seen = 0
    for name, fleet, ids, reqs, in_use, last_used, xp, xt, meta in rf.serve_edge_cases():
        serve = ref[f"{name}/serve"]
        for i, t in enumerate(meta["tags"]):
            tag = str(meta["tag_names"][t])
            if tag.startswith("quirk/complete-first/"):
                pods = fleet.ent_pod[fleet.models[i]["ent_off"]:][:2]
                assert serve[i, 0] == (pods[1] if tag.endswith(str(2**31 - 1)) else pods[0]), (name, tag)
                seen += 1
    assert seen == 4


def test_both_restatements_equal_the_reference_text_at_the_edges(ref):
    n = 0
    for name, fleet, ids, reqs, in_use, last_used, xp, xt, meta in rf.serve_edge_cases():
        want = ref[f"{name}/serve"]
        live_mask = (fleet.pods["flags"] & 2) != 0
        live = np.ascontiguousarray(live_mask.astype(np.uint8))
        live_set = {int(p) for p in np.nonzero(live_mask)[0]}
        for i in range(len(reqs)):
            r = reqs[i]
            pods, times = _filtered(fleet, r, xp, xt)
            ch, ts = ob.serve(r["self_pod"], r["flags"] & 1, r["flags"] & 2, pods, times, fleet.now, r["assume_completed_ms"],
                              r["local_in_flight"], r["last_invoke_time"], live, in_use, last_used)
            pch, pts = po.serve_get_next([(int(p), int(t)) for p, t in zip(pods, times)], int(r["self_pod"]), bool(r["flags"] & 1),
                                         bool(r["flags"] & 2), live_set, int(fleet.now), int(r["assume_completed_ms"]),
                                         int(r["local_in_flight"]), int(r["last_invoke_time"]), in_use, last_used)
            assert ch == pch == want[i, 0], (name, i, ch, pch, want[i], r)
            if ch >= 0:
                assert ts == pts == want[i, 1], (name, i, ts, pts, want[i])
            n += 1
    assert n == 334
