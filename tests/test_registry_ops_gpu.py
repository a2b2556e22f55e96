"""mmp_registry_ops on the device against the sequential restatement (tests/registry_ops_model.py), exact: status bytes, edits
in op order, every info field and the resident registry after an apply; the wave and workgroup edges of the ballot scatter;
refused calls and the map they must leave clean; truncation, NULL buffers, dry runs; what follows an applied batch without a
commit; the place -> load -> evict -> deregister loop; a census beside applied batches; and the JNI veneer."""
import copy
import threading
from collections import OrderedDict

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd import workload as wl
from modelmesh_amd._lib import (ROP_DEREGISTER, ROP_EDIT_REM_LOADED, ROP_EDITED, ROP_LOAD_FAILED, ROP_REGISTER, ROP_SCALE_DOWN,
                                ROP_UNCHANGED, ROPF_MATCH_TIME, ROPS_BLOCK)
from modelmesh_amd.solver import MmpError, Solver
from oracle import bind as ob
from oracle.bind import OracleFleet
from tests import janitor_model as jm
from tests import registry_census_model as cm
from tests import registry_ops_model as ro
from tests import registry_prune_model as rp
from tests.registry_ops_model import Registry, op_row, ops_array
from tests.util import assert_same_decisions

pytestmark = pytest.mark.gpu

INFO_SCALARS = ("n_edits", "n_unchanged", "truncated", "n_entries_added", "n_entries_removed")


def ops_fleet(seed, pods, models, base=None):
    """A fuzz fleet whose registry holds the shapes every exit needs (ro.seed_shapes), as (fleet, Registry, rng)."""
    fleet = base if base is not None else wl.fuzz_fleet(seed + 1300, pods=pods, models=models)
    rng = np.random.default_rng(93_000 + seed)
    reg = Registry(ro.registry_from_arrays(fleet.models, fleet.ent_pod, fleet.ent_time), fleet.pods["id_order"].copy())
    ro.seed_shapes(reg.records, reg.id_order, int(fleet.now), rng)
    fleet.models, fleet.ent_pod, fleet.ent_time = ro.registry_to_arrays(reg.records)
    return fleet, reg, rng


def loaded(fleet):
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    s.load_fleet(fleet)
    return s


def same_outputs(got, want):
    (st, ed, info), (wst, wed, winfo) = got, want
    assert st.dtype == wst.dtype and np.array_equal(st, wst), (st[:8], wst[:8])
    assert ed.dtype == wed.dtype and np.array_equal(ed, wed), (ed[:4], wed[:4])
    for f in INFO_SCALARS:
        assert int(info[f]) == winfo[f], (f, info, winfo)
    assert list(info["n_edited_op"]) == winfo["n_edited_op"] and list(info["n_unchanged_op"]) == winfo["n_unchanged_op"], (info, winfo)


def same_registry(s, reg):
    got = rp.compact(*s.get_models())
    want = ro.registry_to_arrays(reg.records)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def janitor_rows(recs, self_pod, now, limit=150):
    """A cache for self_pod, MRU first: a row per model registered there (every third with another load time); the models
    beyond `limit` have no row, so the registry loop removes their entries."""
    rows = []
    for m, r in enumerate(recs):
        lt = dict(r.loaded).get(self_pod)
        if lt is None or len(rows) >= limit:
            continue
        k = len(rows) + 1
        rows.append((m, 10 + k, now - 2_000_000 - 7 * k, lt + (k % 3 == 0), 0, -1, 1, now - 7_000_000, 0, 0, 0,
                     _lib.JE_DONE | _lib.JE_STATE_LIVE, 0))
    return np.array(rows, dtype=_lib.JANITOR_ENTRY).reshape(-1)


def one_batch(s, reg, ops, now, apply=True, **kw):
    """The same batch on both sides (the restatement edits `reg` when the device applies); every output equal."""
    got = s.registry_ops(ops, now, apply=apply, **kw)
    want = reg.run(ops, now, dry=not apply)
    same_outputs(got, want)
    return want


# ---- sizes: the wave and workgroup edges of the ballot scatter ----------------------------------------------------------

@pytest.fixture(scope="module")
def small():
    """One 8 x 300 fleet for the tests that only read it or that restore what they change (each loads its own solver)."""
    return ops_fleet(0, 8, 300)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, ROPS_BLOCK - 1, ROPS_BLOCK, ROPS_BLOCK + 1])
def test_wave_and_workgroup_edges(small, n):
    fleet, reg0, _ = small
    reg, rng = copy.deepcopy(reg0), np.random.default_rng(n)
    s = loaded(fleet)
    try:
        ops = ro.draw_ops(reg.records, reg.id_order, int(fleet.now), rng, n)
        assert len(ops) == n
        st, ed, info = one_batch(s, reg, ops, int(fleet.now))
        assert info["n_edits"] + info["n_unchanged"] == n and (n < 63 or 0 < info["n_edits"] < n)
        same_registry(s, reg)
    finally:
        s.close()


def test_a_batch_of_unchanged_ops_and_a_batch_of_edits(small):
    fleet, reg0, _ = small
    reg, now = copy.deepcopy(reg0), int(fleet.now)
    s = loaded(fleet)
    try:
        n = ROPS_BLOCK + 9
        quiet = ops_array([op_row(i, 0, ROP_SCALE_DOWN, last_used=now, load_time=-77) for i in range(n)])  # no entry has this time
        st, ed, info = one_batch(s, reg, quiet, now)
        assert not st.any() and len(ed) == 0 and info["n_unchanged"] == n and info["n_unchanged_op"][ROP_SCALE_DOWN] == n
        same_registry(s, reg)
        loud = ops_array([op_row(i, i % 8, ROP_REGISTER, last_used=0, load_time=now + i) for i in range(n)])
        st, ed, info = one_batch(s, reg, loud, now)
        assert st.all() and len(ed) == n and list(ed["op_index"]) == list(range(n)) and info["n_edited_op"][ROP_REGISTER] == n
        same_registry(s, reg)
    finally:
        s.close()


# ---- records -------------------------------------------------------------------------------------------------------------

def test_records_with_no_entries_and_with_sixty_four_copies():
    fleet = wl.fuzz_fleet(1310, pods=80, models=300)
    now = int(fleet.now)
    reg = Registry(ro.registry_from_arrays(fleet.models, fleet.ent_pod, fleet.ent_time), fleet.pods["id_order"].copy())
    order = sorted(range(80), key=lambda p: reg.id_order[p])
    held, rest = order[:64:1], order[64:]
    for m in range(6):
        reg.records[m].instance_ids = OrderedDict((p, now - 100 - p) for p in held)
        reg.records[m].load_failed_instance_ids = OrderedDict()
    reg.records[5].load_failed_instance_ids = OrderedDict((p, now - 7) for p in rest[:3])
    for m in (6, 7, 8, 9):
        reg.records[m].instance_ids, reg.records[m].load_failed_instance_ids = OrderedDict(), OrderedDict()
    fleet.models, fleet.ent_pod, fleet.ent_time = ro.registry_to_arrays(reg.records)
    s = loaded(fleet)
    try:
        ops = ops_array([
            op_row(0, held[63], ROP_DEREGISTER, last_used=0),                                       # the last of 64
            op_row(1, rest[-1], ROP_REGISTER, last_used=now, load_time=now),                        # a 65th, at the end
            op_row(2, held[31], ROP_REGISTER, last_used=now, load_time=now),                        # replaced in the middle
            op_row(3, held[0], ROP_LOAD_FAILED, last_used=-1, load_time=now - 100 - held[0], load_complete_time=now),
            op_row(4, held[40], ROP_SCALE_DOWN, last_used=0, load_time=now - 100 - held[40]),
            op_row(5, rest[1], ROP_REGISTER, last_used=now, load_time=now),                         # 65 copies, a failure removed
            op_row(6, 3, ROP_REGISTER, last_used=0, load_time=now),                                 # onto an empty record
            op_row(7, 3, ROP_DEREGISTER, last_used=0),                                              # nothing there
            op_row(8, 3, ROP_LOAD_FAILED, last_used=0, load_time=0, load_complete_time=0),
            op_row(9, 3, ROP_SCALE_DOWN, last_used=0, load_time=0),
        ])
        st, ed, info = one_batch(s, reg, ops, now)
        assert list(st) == [1, 1, 1, 1, 1, 1, 1, 0, 0, 0]
        assert list(ed["n_loaded_after"]) == [63, 65, 64, 63, 63, 65, 1] and ed["inserted_pos"][1] == 64 and ed["inserted_pos"][5] == 64
        same_registry(s, reg)
    finally:
        s.close()


def test_preshutdown_deregisters_two_thousand_models_of_one_instance():
    fleet = wl.fuzz_fleet(1320, pods=8, models=2000)
    now, pod = int(fleet.now), 3
    reg = Registry(ro.registry_from_arrays(fleet.models, fleet.ent_pod, fleet.ent_time), fleet.pods["id_order"].copy())
    for m, r in enumerate(reg.records):  # every model stands on the instance: loaded, or failed, or (a few) both
        if m % 5 != 0 and pod not in r.instance_ids:
            ro.tree_put(r.instance_ids, pod, now - 1000 - m, reg.id_order)
        if m % 5 == 0 or m % 7 == 0:
            ro.tree_put(r.load_failed_instance_ids, pod, now - 500 - m, reg.id_order)
        if m % 5 == 0:
            r.instance_ids.pop(pod, None)
    fleet.models, fleet.ent_pod, fleet.ent_time = ro.registry_to_arrays(reg.records)
    s = loaded(fleet)
    try:
        before = s.registry_census()
        assert before[1][pod] == 1600 and before[2][pod] > 400
        ops = ops_array([op_row(m, pod, ROP_DEREGISTER, last_used=0) for m in range(2000)])
        st, ed, info = one_batch(s, reg, ops, now, max_edits=2000)
        assert st.all() and info["n_edits"] == 2000 and info["n_entries_removed"] == int(before[1][pod] + before[2][pod])
        after = s.registry_census()
        assert after[1][pod] == 0 and after[2][pod] == 0
        others = np.arange(8) != pod
        assert np.array_equal(after[1][others], before[1][others]) and np.array_equal(after[2][others], before[2][others])
        assert int(after[0]["n_models"]) == 2000
        same_registry(s, reg)
    finally:
        s.close()


# ---- fleets --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed,pods,models,n", [(0, 8, 300, 120), (1, 300, 2000, 700)])
def test_three_consecutive_batches_equal_the_restatement(seed, pods, models, n):
    fleet, reg, rng = ops_fleet(seed, pods, models)
    s = loaded(fleet)
    try:
        for batch in range(3):
            now = int(fleet.now) + 1000 * batch
            ops = ro.draw_ops(reg.records, reg.id_order, now, rng, n)
            before = copy.deepcopy(reg.records)
            st, ed, info = one_batch(s, reg, ops, now)
            by_op = {int(e["op_index"]): e for e in ed}
            seen = set()
            for i, o in enumerate(ops):
                seen.update(ro.classify(before[o["model"]], o, st[i], by_op.get(i)))
            assert seen == set(ro.EXITS), sorted(set(ro.EXITS) - seen)  # the batch took every exit of the four sites
            same_registry(s, reg)
            # (the registry is resident only: the shapes the next batch needs go in as registry events)
            mark = copy.deepcopy(reg.records)
            ro.seed_shapes(reg.records, reg.id_order, now + 1000, rng)
            changed = [m for m in range(models) if not reg.records[m] == mark[m]]
            sub = ro.registry_to_arrays([reg.records[m] for m in changed])
            s.upsert_models(np.array(changed, np.int32), *sub)
    finally:
        s.close()


def test_four_thousand_ops_on_c3():
    fleet, reg, rng = ops_fleet(2, 10_000, 100_000, wl.make_fleet("C3"))
    s = loaded(fleet)
    try:
        now = int(fleet.now)
        ops = ro.draw_ops(reg.records, reg.id_order, now, rng, 4096)
        assert len(ops) == 4096
        st, ed, info = one_batch(s, reg, ops, now, max_edits=4096)
        assert all(info["n_edited_op"]) and info["n_edits"] > 1000
        same_registry(s, reg)
    finally:
        s.close()


# ---- rejected calls ------------------------------------------------------------------------------------------------------

def test_refused_calls_change_nothing_and_leave_the_map_clean(small):
    fleet, reg0, rng = small
    reg, now = copy.deepcopy(reg0), int(fleet.now)
    s = loaded(fleet)
    try:
        resident = [a.copy() for a in s.get_models()]
        good = [op_row(m, m % 8, ROP_REGISTER, last_used=0, load_time=now) for m in range(10, 290)]
        dup_far = good + [op_row(10, 1, ROP_DEREGISTER)]          # the same model in two workgroups' worth of ops
        dup_near = good[:5] + [op_row(12, 1, ROP_DEREGISTER)]     # in one wave
        bad = [dup_far, dup_near, good + [op_row(300, 0, 0)], good + [op_row(-1, 0, 0)], good + [op_row(0, 8, 0)], good + [op_row(0, -1, 0)],
               good + [op_row(0, 0, 4)], good + [op_row(0, 0, -1)], good + [op_row(0, 0, 0, flags=4)]]
        for rows in bad:
            for flags in (_lib.ROPS_APPLY, 0):
                with pytest.raises(MmpError) as ei:
                    s.registry_ops_raw(ops_array(rows), now, flags, 1024)
                assert ei.value.code == _lib.MMP_EINVAL
        for now_bad in (0, -5):
            with pytest.raises(MmpError) as ei:
                s.registry_ops_raw(ops_array(good), now_bad, _lib.ROPS_APPLY, 1024)
            assert ei.value.code == _lib.MMP_EINVAL
        with pytest.raises(MmpError):
            s.registry_ops_raw(ops_array(good), now, _lib.ROPS_APPLY | _lib.ROPS_DRY, 1024)
        with pytest.raises(MmpError):
            s.registry_ops_raw(ops_array(good), now, 4, 1024)
        for a, b in zip(resident, s.get_models()):
            assert a.tobytes() == b.tobytes()  # bit-identical: rows, arena, nothing appended
        # a following valid call on the models the refused ones had marked is right: the map was left clean
        ops = ops_array(good + [op_row(0, 1, ROP_DEREGISTER), op_row(295, 1, ROP_DEREGISTER)])
        one_batch(s, reg, ops, now)
        one_batch(s, reg, ro.draw_ops(reg.records, reg.id_order, now, rng, 150), now)
        same_registry(s, reg)
        # and the janitor, which shares the map, finds it clean as well
        recs = ro.to_prune_records(reg.records)
        entries = janitor_rows(recs, 2, now)
        got = s.janitor_plan(entries, jm.params(2, now), dry=True)
        want = jm.Janitor().run(recs, entries, jm.params(2, now), fleet.pods["id_order"], dry=True)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    finally:
        s.close()


def test_ops_need_a_committed_snapshot():
    s = Solver(6553, 60_000)
    try:
        with pytest.raises(MmpError) as ei:
            s.registry_ops(ops_array([op_row(0, 0, 0)]), 1_700_000_000_000)
        assert ei.value.code == _lib.MMP_ESTATE
    finally:
        s.close()


# ---- buffers and modes ---------------------------------------------------------------------------------------------------

def test_truncation_null_buffers_and_dry_runs_change_nothing(small):
    fleet, reg0, _ = small
    reg, now = copy.deepcopy(reg0), int(fleet.now)
    s = loaded(fleet)
    try:
        ops = ro.draw_ops(reg.records, reg.id_order, now, np.random.default_rng(4), 200)
        wst, wed, winfo = reg.run(ops, now, dry=True)
        assert len(wed) > 20
        for flags in (_lib.ROPS_APPLY, 0):
            for cap in (3, len(wed) - 1, 0):
                st, ed, info = s.registry_ops_raw(ops, now, flags, cap)
                assert int(info["truncated"]) == 1 and np.array_equal(ed, wed[:cap]) and np.array_equal(st, wst)  # the prefix
                same_outputs((st, wed, info), (wst, wed, dict(winfo, truncated=1)))                               # the totals
                same_registry(s, reg)
        # NULL status: not returned; the rest as ever
        st, ed, info = s.registry_ops_raw(ops, now, 0, len(wed), want_status=False)
        assert not st.any()
        same_outputs((wst, ed, info), (wst, wed, winfo))
        # flags = 0 and DRY: computed, nothing changed
        same_outputs(s.registry_ops(ops, now, apply=False), (wst, wed, winfo))
        same_outputs(s.registry_ops(ops, now, dry=True), (wst, wed, winfo))
        same_registry(s, reg)
        # n = 0: a valid call with empty outputs, with and without buffers
        for cap in (0, 4):
            st, ed, info = s.registry_ops_raw(ops[:0], now, _lib.ROPS_APPLY, cap)
            assert len(st) == 0 and len(ed) == 0 and not any(int(info[f]) for f in INFO_SCALARS)
        # the repeat with room gives the full result (the Python veneer regrows from 2)
        one_batch(s, reg, ops, now, max_edits=2)
        same_registry(s, reg)
    finally:
        s.close()


# ---- after an applied batch, without a commit ----------------------------------------------------------------------------

def test_after_an_apply_everything_downstream_sees_the_edited_records():
    fleet, reg, rng = ops_fleet(5, 64, 1500, wl.make_fleet("C1", models=1500, pods=64))
    fleet.pods["used"] = fleet.pods["capacity"] // 4  # (the proactive plan has a budget)
    s = loaded(fleet)
    try:
        now, self_pod = int(fleet.now), 2
        ops = ro.draw_ops(reg.records, reg.id_order, now, rng, 600)
        st, ed, info = one_batch(s, reg, ops, now)
        touched = ed["model"]
        assert len(touched) > 200
        f2 = copy.copy(fleet)
        f2.pods = s.get_pods()
        f2.models, f2.ent_pod, f2.ent_time = ro.registry_to_arrays(reg.records)
        for n in (700, 6000):  # the latency slots and the batch path
            reqs, extra = wl.fuzz_requests(f2, 40 + n, n)
            reqs["model"][::2] = rng.choice(touched, len(reqs["model"][::2]))
            want = OracleFleet(f2).place(reqs, extra, f2.now, threads=4)
            assert_same_decisions(f2, reqs, s.place(reqs, extra, f2.now), want)
        from tests.test_registry_prune_gpu import _serve_check
        _serve_check(s, f2, rng, touched)
        recs = ro.to_prune_records(reg.records)
        # the janitor plan, the prune and the proactive plan read the same records
        entries = janitor_rows(recs, self_pod, now)
        assert len(entries) > 5
        prm = jm.params(self_pod, now)
        got = s.janitor_plan(entries, prm, dry=True)
        want = jm.Janitor().run(recs, entries, prm, fleet.pods["id_order"], dry=True)
        for g, w in zip(got[:4], want[:4]):
            assert np.array_equal(g, w)
        e, rm, pinfo = s.prune_registry(self_pod, now, dry=True)
        we, wrm, winfo, _ = rp.Reaper().run(f2.pods["flags"], recs, self_pod, now, dry=True)
        assert np.array_equal(e, we) and np.array_equal(rm, wrm) and int(pinfo["n_unresolved"]) == winfo["n_unresolved"]
        gm, gl, gi = s.proactive_plan(6400, now, fleet.n_models)
        wm, wl_, wi = ob.proactive_plan(f2, 6400, now, fleet.n_models)
        assert np.array_equal(gm, wm) and np.array_equal(gl, wl_) and int(gi["n_candidates"]) == int(wi["n_candidates"])
        assert len(gm) > 0
    finally:
        s.close()


# ---- the loop this closes ------------------------------------------------------------------------------------------------

def test_evicted_keys_go_straight_into_deregister_ops():
    fleet, reg, rng = ops_fleet(6, 8, 300)
    now, pod = int(fleet.now), 5
    mine = [m for m, r in enumerate(reg.records) if pod in r.instance_ids]
    assert len(mine) >= 12
    s = loaded(fleet)
    try:
        # the instance's cache holds exactly its registered models, oldest first, and is full
        lu = np.array([now - 10_000 + k for k in range(len(mine))], np.int64)
        s.load_caches_keyed(np.array([0, len(mine)], np.int32), lu, np.full(len(mine), 10, np.int32), np.array(mine, np.int32),
                            np.array([10 * len(mine)], np.int64))
        before = s.registry_census()
        fresh = [m for m in range(300) if m not in mine][:3]
        puts = np.array([(0, _lib.COP_PUT_IF_ABSENT, m, 30, now + k, 0, 0) for k, m in enumerate(fresh)], dtype=_lib.CACHE_OP)
        outs, ev = s.cache_replay(puts, now)
        evicted = [int(k) for o in outs for k in ev[o["evicted_off"]: o["evicted_off"] + o["n_evicted"]]]
        assert evicted and set(evicted) <= set(mine) and len(set(evicted)) == len(evicted)  # the puts pushed registered models out
        ops = ops_array([op_row(m, pod, ROP_DEREGISTER, flags=ROPF_MATCH_TIME, last_used=int(lu[mine.index(m)]), load_time=reg.records[m].instance_ids[pod],
                                load_complete_time=0) for k, m in enumerate(evicted)])
        st, ed, info = one_batch(s, reg, ops, now)
        assert st.all() and all(e["flags"] & ROP_EDIT_REM_LOADED for e in ed)
        after = s.registry_census()
        assert int(before[1][pod]) - int(after[1][pod]) == len(evicted)  # the instance's count fell by exactly the evicted
        others = np.arange(8) != pod
        assert np.array_equal(after[1][others], before[1][others])
        same_registry(s, reg)
    finally:
        s.close()


# ---- concurrency ---------------------------------------------------------------------------------------------------------

def test_a_census_beside_applied_batches_sees_one_of_the_prefix_states():
    fleet, reg, rng = ops_fleet(7, 16, 700)
    s = loaded(fleet)
    try:
        now = int(fleet.now)
        n_pods, n_types = s.registry_census_sizes()
        key = lambda c: (c[0].tobytes(), c[1].tobytes(), c[2].tobytes(), c[3].tobytes())  # noqa: E731
        batches, states = [], [key(cm.census_closed(*ro.registry_to_arrays(reg.records)[:2], n_pods, n_types))]
        twin = copy.deepcopy(reg)
        for k in range(24):
            ops = ro.draw_ops(twin.records, twin.id_order, now + k, rng, 12)
            twin.run(ops, now + k)
            batches.append(ops)
            states.append(key(cm.census_closed(*ro.registry_to_arrays(twin.records)[:2], n_pods, n_types)))
        assert len(set(states)) > 12
        results, errors, done = [], [], threading.Event()

        def count():
            try:
                while not done.is_set():
                    results.append(s.registry_census())
                results.append(s.registry_census())
            except Exception as ex:  # noqa: BLE001
                errors.append(ex)

        th = threading.Thread(target=count)
        th.start()
        try:
            for k, ops in enumerate(batches):
                one_batch(s, reg, ops, now + k)
        finally:
            done.set()
            th.join()
        assert not errors, errors
        at = []
        for got in results:
            g = key((got[0], got[1].astype(np.int32), got[2].astype(np.int32), got[3]))
            assert g in states, "a census saw a registry that is no prefix state"
            at.append(states.index(g))
        print(f"{len(results)} censuses beside {len(batches)} applied batches saw prefix states {sorted(set(at))}")
        assert at == sorted(at) and results and key(results[-1]) == states[-1]
        same_registry(s, reg)
    finally:
        s.close()


# ---- JNI -----------------------------------------------------------------------------------------------------------------

def test_the_veneer_entry_runs_under_the_mock_jvm(tmp_path, small):
    from tests import jni_mock as jmock
    from tests.test_jni_veneer import _java_natives
    veneer = jmock.Veneer(jmock.build(tmp_path), _java_natives())
    env = veneer.env
    fleet, reg0, _ = small
    reg, now = copy.deepcopy(reg0), int(fleet.now)
    direct = loaded(fleet)
    h = veneer.call("create", 0, fleet.min_space_units, fleet.min_churn_age_ms)
    assert h != 0 and env.pending() is None
    try:
        assert veneer.call("podsLoad", h, jmock.ByteBuffer(fleet.pods), fleet.n_pods) == 0
        assert veneer.call("modelsLoad", h, jmock.ByteBuffer(fleet.models), fleet.n_models, jmock.ByteBuffer(fleet.ent_pod),
                           jmock.ByteBuffer(fleet.ent_time), len(fleet.ent_pod)) == 0
        assert veneer.call("commit", h) == 0
        ops = ro.draw_ops(reg.records, reg.id_order, now, np.random.default_rng(8), 100)
        dst, ded, dinfo = direct.registry_ops(ops, now)
        n = len(ops)
        status = jmock.ByteBuffer(np.zeros(n, np.uint8))
        edits = jmock.ByteBuffer(np.zeros(n, dtype=_lib.REGISTRY_OP_EDIT))
        info = jmock.ByteBuffer(np.zeros(1, dtype=_lib.REGISTRY_OPS_INFO))
        rc = veneer.call("registryOps", h, jmock.ByteBuffer(ops), n, now, _lib.ROPS_APPLY, status, edits, n, info)
        assert rc == 0 and env.pending() is None
        assert np.array_equal(status.arr, dst) and np.array_equal(edits.arr[: len(ded)], ded) and info.arr[0].tobytes() == dinfo.tobytes()
        same_outputs((dst, ded, dinfo), reg.run(ops, now))
        # a short direct buffer is refused before the library is called
        short = jmock.ByteBuffer(np.zeros(n - 1, dtype=_lib.REGISTRY_OP_EDIT))
        assert veneer.call("registryOps", h, jmock.ByteBuffer(ops), n, now, 0, status, short, n, info) == -1
        assert env.pending()[0] == "java/lang/IllegalArgumentException" and "editsOut shorter" in env.pending()[1]
        env.clear()
        assert veneer.call("registryOps", h, jmock.ByteBuffer(ops[: n - 1]), n, now, 0, status, edits, n, info) == -1
        assert "ops shorter" in env.pending()[1]
        env.clear()
    finally:
        veneer.call("destroy", h)
        direct.close()
