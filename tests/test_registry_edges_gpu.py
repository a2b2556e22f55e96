"""GPU: mmp_janitor_plan (row a16') and mmp_registry_prune (row a17') against tests/golden/ref_registry_edges.npz — what the
reference's own text answered on the cases of tests/ref_registry_edges.py (see tests/test_registry_edges.py, which asserts the
premises and holds the restatements to the same vectors).  Every comparison is exact; this file reads the committed vectors alone.
Every case runs on a table loaded as it stands and a second time on a table reached by mmp_pods_upsert + a delta commit from a
neighbouring one."""
import copy

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd.solver import MmpError, Solver
from tests import janitor_model as jm
from tests import ref_registry_edges as rre
from tests import registry_prune_model as rp
from tests.test_registry_prune_gpu import same_registry

pytestmark = pytest.mark.gpu

REF = rre.load()
CASES = {str(n): rre.load_case(REF, str(n)) for n in REF["names"]}
JANITOR = [n for n, c in CASES.items() if c["meta"]["kind"] == "janitor"]
PRUNE = [n for n, c in CASES.items() if c["meta"]["kind"] == "prune" and c["meta"]["domain"]]
OUTSIDE = [n for n, c in CASES.items() if not c["meta"]["domain"]]
ROUTES = ("loaded", "delta")
JAN_INFO = ("n_edits", "n_candidates", "n_ties", "stopped_at", "truncated")
PRUNE_INFO = ("n_edits", "n_removed", "n_repaired", "n_missing_pods", "n_new_missing", "truncated")


def solver_for(c, route, flags=None):
    """a Solver holding the case's instance table and registry.  route "delta": a neighbouring table is committed first (three
    instances with other counters), then the case's rows arrive through mmp_pods_upsert and a delta commit"""
    fleet = rre.fleet_of(c, flags)
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    if route == "loaded":
        s.load_fleet(fleet)
        return s
    near = copy.copy(fleet)
    near.pods = fleet.pods.copy()
    idx = np.unique(np.array([0, fleet.n_pods // 2, fleet.n_pods - 1], np.int32))
    near.pods["used"][idx] += 1
    near.pods["count"][idx] += 1
    s.load_fleet(near)
    before = s.delta_commits()
    s.upsert_pods(idx, fleet.pods[idx])
    s.commit()
    assert s.delta_commits() == before + 1, "the second table was not reached by a delta commit"
    assert np.array_equal(s.get_pods(), fleet.pods)
    return s


def same_janitor(got, want, what):
    for g, w, part in zip(got[:4], want[:4], ("actions", "edits", "candidates", "candidate rows")):
        if part == "actions":
            g = rre.collapse(g)
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, part, g[:8], w[:8])
    for f in JAN_INFO:
        assert int(got[4][f]) == want[4][f], (what, f, got[4], want[4])
    assert [int(x) for x in rre.collapse(got[0])] == [int(x) for x in want[0]]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", JANITOR)
def test_the_janitor_plan_equals_the_text(name, route):
    c = CASES[name]
    reg, entries, prm = c["reg"], c["entries"], c["prm"]
    want = rre.expected_janitor(c["runs"][0], reg, entries, prm)
    s = solver_for(c, route)
    try:
        dry = s.janitor_plan(entries, prm, dry=True)          # once dry, which changes nothing
        same_janitor(dry, want, (name, route, "dry"))
        same_registry(s, reg)
        got = s.janitor_plan(entries, prm)                    # MMP_JANITOR_APPLY
        same_janitor(got, want, (name, route, "apply"))
        assert np.array_equal(got[0], dry[0])
        # the one byte the text cannot show (IN_ORDER leaves no call): the device's own bytes against the closed rule, which
        # tests/test_registry_edges.py holds to the sequential restatement on the same rows
        closed = jm.closed_rule(c["models"], c["ent_pod"], c["ent_time"], entries, prm, c["pods"]["id_order"])
        assert np.array_equal(got[0], closed[0]), (name, route, got[0], closed[0])
        same_registry(s, want[5])                             # the resident registry, record by record, against the text's records
    finally:
        s.close()


@pytest.mark.parametrize("name", JANITOR)
def test_the_janitor_plan_by_model_id_equals_the_text(name):
    """mmp_janitor_plan_k with the records' ids as keys; a row without a record names an id the table does not hold"""
    c = CASES[name]
    reg, entries, prm = c["reg"], c["entries"], c["prm"]
    want = rre.expected_janitor(c["runs"][0], reg, entries, prm)
    s = solver_for(c, "loaded")
    try:
        s.model_ids_load([f"m{i:05d}".encode() for i in range(len(reg))])
        keys = [rre.row_name(entries, r).encode() for r in range(len(entries))]
        blind = entries.copy()
        blind["model"] = -7                                   # by key: the row's model field is not read
        idx, actions, edits, cands, rows, removed, info = s.janitor_plan_k(blind, keys, prm)
        assert np.array_equal(idx, entries["model"]), name
        same_janitor((actions, edits, cands, rows, info), want, (name, "by id"))
        assert np.array_equal(actions, jm.closed_rule(c["models"], c["ent_pod"], c["ent_time"], entries, prm, c["pods"]["id_order"])[0]), name
        same_registry(s, want[5])
    finally:
        s.close()


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", PRUNE)
def test_the_registry_prune_equals_the_text_run_by_run(name, route):
    c = CASES[name]
    m = c["meta"]
    reg, miss = copy.deepcopy(c["reg"]), {}
    s = solver_for(c, route, np.array(m["runs"][0]["flags"], np.uint32))
    try:
        flags = np.array(m["runs"][0]["flags"], np.uint32)
        for k, (run, spec) in enumerate(zip(c["runs"], m["runs"])):
            new = np.array(spec["flags"], np.uint32)
            changed = np.nonzero(new != flags)[0].astype(np.int32)
            if len(changed):                                  # an instance returns, or leaves again
                rows = s.get_pods()[changed]
                rows["flags"] = new[changed]
                s.upsert_pods(changed, rows)
                s.commit()
                flags = new
            we, wr, winfo, wc, after, miss_after = rre.expected_prune(run, reg, miss)
            if k == len(c["runs"]) - 1:                       # the last run once dry first: nothing moves
                e, r, info = s.prune_registry(m["self_pod"], spec["now"], dry=True)
                assert np.array_equal(e, we) and np.array_equal(r, wr), (name, k, "dry")
                assert s.missing_instances() == miss
                same_registry(s, reg)
            e, r, info = s.prune_registry(m["self_pod"], spec["now"])
            assert np.array_equal(e, we), (name, route, k, e, we)
            assert np.array_equal(r, wr), (name, route, k, r, wr)
            for f in PRUNE_INFO:
                assert int(info[f]) == winfo[f], (name, route, k, f, info, winfo)
            assert int(info["n_unresolved"]) == 0
            assert s.missing_instances() == miss_after, (name, route, k, s.missing_instances(), miss_after)
            same_registry(s, after)
            # the candidate rule (:6574-6577) as mmp_proactive_plan applies it to the resident registry after the apply.  It takes
            # globalLru from the committed instance table: 0 while anything is free; where the run's globalLru is not 0 the case
            # carries a full table whose least recently used time is that value (tests/test_registry_edges.py asserts both)
            models, last_used, pinfo = s.proactive_plan(6400, spec["now"], len(reg))
            assert int(pinfo["n_candidates"]) == len(wc), (name, route, k, pinfo, wc)
            assert set(int(x) for x in models) <= set(wc), (name, route, k, models, wc)
            if spec["global_lru"]:                            # nothing is free: candidates are counted, none is selected
                assert int(pinfo["n_selected"]) == 0 and len(wc) > 0, (name, route, k, pinfo)
            reg, miss = after, miss_after
    finally:
        s.close()


def test_outside_the_documented_domain_the_device_does_what_the_header_says():
    """kept in the file, marked: a clock value of 0 is refused (the mark 0 stands for "no mark"); an entry whose id the instance table
    does not hold is never judged — where the text, which knows ids alone, prunes it"""
    assert len(OUTSIDE) == 2
    for name in OUTSIDE:
        c = CASES[name]
        m = c["meta"]
        s = solver_for(c, "loaded", np.array(m["runs"][0]["flags"], np.uint32))
        try:
            if m["which"] == "clock0":
                with pytest.raises(MmpError) as ei:
                    s.prune_registry(m["self_pod"], 0)
                assert ei.value.code == _lib.MMP_EINVAL
                assert s.missing_instances() == {}
            else:
                for spec in m["runs"]:
                    e, r, info = s.prune_registry(m["self_pod"], spec["now"])
                    assert len(e) == 0 and len(r) == 0 and int(info["n_unresolved"]) == 1 and s.missing_instances() == {}
            same_registry(s, c["reg"])
        finally:
            s.close()
