"""mmp_registry_unresolved: which records name an id the instance table does not know.  The list must equal a numpy pass over
mmp_models_get, its entry count the census's n_entries_unresolved; and the loop it exists for — an instance joins, the host
asks, the listener sends the stored values of those records again — must end in the registry and the decisions of a context that
knew every id from the start."""
import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd import workload as wl
from modelmesh_amd.solver import Solver
from oracle.bind import OracleFleet
from tests import wire
from tests.util import assert_same_decisions

pytestmark = pytest.mark.gpu

P = 50


def _numpy_list(s):
    rows, ep, _ = s.get_models()
    n_pods = len(s.get_pods())
    out, entries = [], 0
    for i, r in enumerate(rows):
        seg = ep[r["ent_off"]: r["ent_off"] + r["n_loaded"] + r["n_failed"]]
        u = int(((seg < 0) | (seg >= n_pods)).sum())
        if u:
            out.append(i)
            entries += u
    return np.array(out, np.int32), entries


def _registry(M, how, seed):
    """M records of 0 to 3 loaded and 0 to 2 failed entries; `how` says where the unresolved pods (-1, or beyond the table) go."""
    rng = np.random.default_rng(seed)
    k, f = rng.integers(0, 4, M), rng.integers(0, 3, M)
    if how in ("all", "failed_only"):
        f = np.maximum(f, 1)
    rows = np.zeros(M, _lib.MODEL_ROW)
    rows["n_loaded"], rows["n_failed"] = k, f
    rows["ent_off"] = np.r_[0, np.cumsum(k + f)][:M]
    n = int((k + f).sum())
    ent_pod = rng.integers(0, P, n).astype(np.int32)
    strange = np.where(rng.random(n) < 0.5, -1, P + rng.integers(0, 3, n)).astype(np.int32)
    is_failed = np.zeros(n, bool)
    for i in range(M):
        is_failed[rows["ent_off"][i] + k[i]: rows["ent_off"][i] + k[i] + f[i]] = True
    if how == "random":
        ent_pod = np.where(rng.random(n) < 0.15, strange, ent_pod)
    elif how == "failed_only":
        ent_pod = np.where(is_failed, strange, ent_pod)
    elif how == "all":  # every row: its first failed entry at least
        first_failed = np.zeros(n, bool)
        first_failed[rows["ent_off"] + k] = True
        ent_pod = np.where(first_failed | (rng.random(n) < 0.3), strange, ent_pod)
    return rows, ent_pod, np.arange(n, dtype=np.int64) + 1


def _check(s, expect_rows=None):
    want, want_entries = _numpy_list(s)
    got, n_models, n_entries = s.registry_unresolved()
    assert np.array_equal(got, want) and n_models == len(want) and n_entries == want_entries
    if expect_rows is not None:
        assert n_models == expect_rows
    stats = s.registry_census()[0]
    assert int(stats["n_entries_unresolved"]) == n_entries
    # sizes only, truncation (the lowest rows first, the counts always full), and a rerun: byte for byte
    nm, ne = _lib.C.c_int32(-1), _lib.C.c_int64(-1)
    assert s.lib.mmp_registry_unresolved(s.h, None, 0, _lib.C.byref(nm), _lib.C.byref(ne)) == 0
    assert (nm.value, ne.value) == (n_models, n_entries)
    for cap in {0, 1, max(n_models - 1, 0)}:
        part, nm2, ne2 = s.registry_unresolved(cap)
        assert np.array_equal(part, want[:cap]) and (nm2, ne2) == (n_models, n_entries)
    again = s.registry_unresolved()
    assert again[0].tobytes() == got.tobytes() and again[1:] == (n_models, n_entries)
    return got


@pytest.mark.parametrize("how", ["random", "none", "all", "failed_only"])
@pytest.mark.parametrize("M", [0, 1, 63, 64, 65, 257, 2000])
def test_the_list_against_numpy(M, how):
    rows, ent_pod, ent_time = _registry(M, how, 100 + M)
    s = Solver(100, 1000)
    try:
        s.load_pods(np.zeros(P, _lib.POD_ROW))
        s.load_models(rows, ent_pod, ent_time)
        got = _check(s, {"none": 0, "all": M}.get(how))
        if how == "failed_only" and M:
            assert len(got) == M  # (every row has a failed entry, and only those are unresolved)
            assert np.all((ent_pod[rows["ent_off"][0]: rows["ent_off"][0] + rows["n_loaded"][0]] >= 0))
    finally:
        s.close()


def test_a_long_record_with_the_unresolved_entry_last():
    rows, ent_pod, ent_time = _registry(300, "none", 5)
    long_row = 131
    rows["ent_off"][long_row], rows["n_loaded"][long_row], rows["n_failed"][long_row] = len(ent_pod), 40, 30
    ent_pod = np.r_[ent_pod, np.arange(70) % P].astype(np.int32)
    ent_time = np.r_[ent_time, np.arange(70)].astype(np.int64)
    s = Solver(100, 1000)
    try:
        s.load_pods(np.zeros(P, _lib.POD_ROW))
        s.load_models(rows, ent_pod, ent_time)
        assert len(_check(s)) == 0
        ent_pod[-1] = -1
        s.load_models(rows, ent_pod, ent_time)
        assert list(_check(s)) == [long_row] and s.registry_unresolved()[2] == 1
        ent_pod[-1] = P  # the first slot the table does not have
        s.load_models(rows, ent_pod, ent_time)
        assert list(_check(s)) == [long_row]
        s.upsert_pods(np.array([P], np.int32), np.zeros(1, _lib.POD_ROW))  # the table grows by a slot: resolved
        assert len(_check(s)) == 0
    finally:
        s.close()


def test_refusals_and_an_empty_registry():
    s = Solver(100, 1000)
    try:
        nm, ne = _lib.C.c_int32(-1), _lib.C.c_int64(-1)
        out = np.zeros(4, np.int32)
        assert s.lib.mmp_registry_unresolved(s.h, None, 0, _lib.C.byref(nm), _lib.C.byref(ne)) == 0 and (nm.value, ne.value) == (0, 0)
        assert s.lib.mmp_registry_unresolved(s.h, None, 4, _lib.C.byref(nm), _lib.C.byref(ne)) == _lib.MMP_EINVAL
        assert s.lib.mmp_registry_unresolved(s.h, _lib.ptr(out), -1, _lib.C.byref(nm), _lib.C.byref(ne)) == _lib.MMP_EINVAL
        assert s.lib.mmp_registry_unresolved(s.h, _lib.ptr(out), 4, None, _lib.C.byref(ne)) == _lib.MMP_EINVAL
        assert s.lib.mmp_registry_unresolved(s.h, _lib.ptr(out), 4, _lib.C.byref(nm), None) == _lib.MMP_EINVAL
    finally:
        s.close()


def _entries(s):
    """The registry as lists per row (the arena offsets differ between a reload and an upsert)."""
    rows, ep, et = s.get_models()
    return [(int(r["type"]), int(r["n_loaded"]), int(r["n_failed"]), int(r["last_used"]),
             ep[r["ent_off"]: r["ent_off"] + r["n_loaded"] + r["n_failed"]].tolist(),
             et[r["ent_off"]: r["ent_off"] + r["n_loaded"] + r["n_failed"]].tolist()) for r in rows]


def test_the_whole_loop_on_a_fleet():
    n_pods, n_models, held = 300, 2000, 5
    rng = np.random.default_rng(31)
    # (a fleet in which the five withheld instances are ones getNext picks: on many fuzz fleets the last five rows are full and
    # excluding them changes no decision of the oracle itself, which would leave step 6 with nothing to show)
    fleet = wl.fuzz_fleet(83, pods=n_pods, models=n_models)
    fleet.pods["flags"] &= ~np.uint32(4)
    ids = wire.make_ids(rng, n_pods)
    wire.adopt_ids(fleet, ids)
    type_names = ["NLCLASSIFIER"] + ["type-%d" % t for t in range(1, max(fleet.n_types, 1))]
    pv = wire.pod_values(fleet, rng, np.full(n_pods, 1000, np.int64))
    mv = wire.model_values(fleet, ids, type_names, rng, np.zeros(n_models, np.int64))
    live = ((fleet.pods["flags"] & 2) != 0).astype(np.uint8)
    known = n_pods - held
    m = fleet.models
    holds = np.array([bool((fleet.ent_pod[r["ent_off"]: r["ent_off"] + r["n_loaded"] + r["n_failed"]] >= known).any()) for r in m])
    affected = np.nonzero(holds)[0].astype(np.int32)
    assert 5 <= len(affected) < n_models
    s, twin = Solver(fleet.min_space_units, fleet.min_churn_age_ms), Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    try:
        # 1. the registry arrives before 5 of the instances are known
        s.load_pod_ids(ids[:known])
        s.load_type_names(type_names, unknown_type=0)
        assert not s.ingest_pods_json(pv[:known], np.arange(known), live[:known])[0].any()
        assert not s.ingest_models_json(mv)[0].any()
        # 2. the list names exactly the records that hold them
        assert np.array_equal(_check(s), affected)
        # 3. the instances join: the stored entries stay what they are
        status, idx, _, n_app = s.pods_events_json(ids[known:], pv[known:], live=live[known:])
        assert not status.any() and list(idx) == list(range(known, n_pods)) and n_app == held
        assert np.array_equal(s.get_pods(), fleet.pods)
        assert np.array_equal(_check(s), affected)
        s.load_types(fleet.n_types, fleet.allowed, fleet.prefer, fleet.has_allowed, fleet.has_prefer)
        s.load_replaced_rs(fleet.replaced_rs)
        s.commit()
        orc = OracleFleet(fleet)
        assert np.array_equal(s.order(), orc.order)
        reqs, extra = wl.fuzz_requests(fleet, 3, 3000)
        reqs["model"] = affected[np.arange(len(reqs)) % len(affected)]
        reqs["last_used"] = m["last_used"][reqs["model"]]
        want = orc.place(reqs, extra, fleet.now, threads=4)
        stale = s.place(reqs, extra, fleet.now)
        differ = (stale["chosen"] != want["chosen"]) | (stale["n_candidates"] != want["n_candidates"]) | (stale["hash"] != want["hash"])
        assert differ.any()  # an unresolved entry excludes nobody: the case is not vacuous
        # 4. the listener sends the stored values of those records again; no commit is needed
        assert not s.upsert_models_json([mv[j] for j in affected], affected)[0].any()
        assert len(_check(s)) == 0
        # 5. the registry of a context that knew every id from the start
        twin.load_pod_ids(ids)
        twin.load_type_names(type_names, unknown_type=0)
        assert not twin.ingest_models_json(mv)[0].any()
        assert _entries(s) == _entries(twin)
        # 6. and the oracle's decisions on the complete fleet
        assert_same_decisions(fleet, reqs, s.place(reqs, extra, fleet.now), want)
    finally:
        s.close()
        twin.close()
