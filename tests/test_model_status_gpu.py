"""mmp_models_status on the device against the sequential restatement of getStatus's answer (tests/model_status_model.py), exact
on every row and every copy: the wave and workgroup edges of the packed path, row lengths on both sides of the long-row path and
of its LDS tile, the CPU tests' boundary cases replayed, batches built to take every named case up to C3, buffer handling and
refused calls, after other writers of the registry and beside them, the JNI veneer, and run-to-run identity."""
import copy
import threading

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd import workload as wl
from modelmesh_amd._lib import (MST_ASK, MST_LOADING_FAILED, MST_NOT_FOUND, ROP_DEREGISTER, ROP_REGISTER, STATUS_BLOCK, STATUS_COPY,
                                STATUS_ROW, STATUS_TILE, STATUS_WAVE_ROW)
from modelmesh_amd.solver import Solver
from tests import model_status_model as sm
from tests import registry_ops_model as ro
from tests import test_model_status_model as cpu
from tests.model_status_model import LONG_MAX, LONG_MIN, assert_same_status, req_row, reqs_array
from tests.registry_prune_model import GONE_AFTER_MS as GONE

pytestmark = pytest.mark.gpu

# the packed path ranks rows of up to STATUS_WAVE_ROW copies (csrc/status_kernels.hpp: kStatusWaveRow), the workgroup path stages
# STATUS_TILE times in LDS at once (kStatusTile); requests and output entries go STATUS_BLOCK to a workgroup (kStatusBlock)
assert (STATUS_BLOCK, STATUS_WAVE_ROW, STATUS_TILE) == (256, 64, 1024)


def loaded(fleet, commit=True):
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    s.load_fleet(fleet, commit=commit)
    return s


def fleet_of(records, pods=8, id_order=None):
    """A fleet around hand-made records [(loaded, failed)], entries as (pod, time) in list order."""
    fleet = wl.fuzz_fleet(1511, pods=pods, models=1)
    fleet.n_types, fleet.allowed, fleet.prefer, fleet.has_allowed, fleet.has_prefer = 0, None, None, None, None
    if id_order is not None:
        fleet.pods["id_order"] = id_order
    reg = [ro.ModelRecord(0, l, f, 5) for l, f in records]
    fleet.models, fleet.ent_pod, fleet.ent_time = ro.registry_to_arrays(reg)
    return fleet, reg


def check(s, reg, id_order, reqs, now, what=""):
    """The device's answer equals the sequential form's; returns it."""
    reqs = reqs_array(reqs) if isinstance(reqs, list) else reqs
    got = s.models_status(reqs, now)
    assert_same_status(got, sm.status_sequential(reg, id_order, reqs, now), what)
    return got


@pytest.fixture(scope="module")
def small():
    """One 8 x 300 fleet with the planted records; nothing writes to it (each test loads its own solver)."""
    return cpu.status_fleet(0, 8, 300)


# ---- request counts ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_wave_and_workgroup_edges(small, n):
    fleet, reg, planted, _ = small
    s = loaded(fleet)
    try:
        reqs = sm.draw_reqs(reg, fleet.pods["id_order"], int(fleet.now), np.random.default_rng(n), n, planted)
        rows, copies = check(s, reg, fleet.pods["id_order"], reqs, int(fleet.now))
        assert len(rows) == n and (n < 63 or len(copies) > n // 2)
    finally:
        s.close()


def test_totals_across_a_wave_boundary_and_batches_of_empty_and_single_rows():
    T = 1_000
    recs = [([], []), ([(1, T)], []), ([(0, T + 1), (2, T + 3), (5, T + 2)], [(3, T + 2)]), ([], [(4, T)])]
    fleet, reg = fleet_of(recs)
    io, now = fleet.pods["id_order"], int(fleet.now)
    s = loaded(fleet)
    try:
        # 62 copies, then one request of 4: entries 62..65 of the output straddle the first wavefront's end
        rows, copies = check(s, reg, io, [req_row(1)] * 31 + [req_row(3)] * 31 + [req_row(2), req_row(1)], now)
        assert int(rows["copy_off"][62]) == 62 and copies["time"][62:66].tolist() == [T + 3, T + 2, T + 2, T + 1]
        assert copies["status"][63:65].tolist() == [0, 1]  # the tie: the loaded one first
        # the same at the workgroup's end: 254 copies, then 4
        rows, _ = check(s, reg, io, [req_row(1)] * 254 + [req_row(2, 6), req_row(2)], now)
        assert rows["copy_off"][254:].tolist() == [254, 259]
        # every request without entries (with the empty requests in front of, between and behind nothing at all)
        rows, copies = check(s, reg, io, [req_row(0), req_row(-1), req_row(0, -1, True)] * 100, now)
        assert len(copies) == 0 and not rows["copy_off"].any() and set(rows["cls"].tolist()) == {0, 1}
        # every request with exactly one entry: stored loaded, stored failed, the overlay's own
        rows, copies = check(s, reg, io, [req_row(1), req_row(3), req_row(0, 7), req_row(-1, 2)] * 80, now)
        assert rows["copy_off"].tolist() == list(range(320)) and len(copies) == 320
        # empty requests between the others: the bisection lands on the request that owns the entry
        check(s, reg, io, [req_row(0), req_row(2), req_row(0), req_row(0), req_row(1), req_row(0)] * 50, now)
    finally:
        s.close()


# ---- row lengths -------------------------------------------------------------------------------------------------------------

LENGTHS = [2, STATUS_WAVE_ROW - 1, STATUS_WAVE_ROW, STATUS_WAVE_ROW + 1, STATUS_TILE - 1, STATUS_TILE, STATUS_TILE + 1, 2 * STATUS_TILE + 3]


@pytest.fixture(scope="module")
def long_rows():
    """48 instances, 40 of them in use; per length a record of that many entries, two thirds loaded: the instances of the table first, ids the table
    does not know behind them.  Times from a handful of values (many ties) with the ends of the long range among them."""
    rng = np.random.default_rng(64)
    P, TABLE, now = 40, 48, 1_700_000_000_000
    pool = np.array([now, now - 1, now - 2, now - 3, 0, -1, LONG_MIN, LONG_MAX, now + 5], np.int64)
    recs = []
    for n in LENGTHS:
        nl = (2 * n + 2) // 3
        pods_l = list(range(min(nl, P))) + list(range(TABLE, TABLE + max(0, nl - P)))
        pods_f = list(range(5, 5 + min(n - nl, 20))) + list(range(TABLE + nl, TABLE + nl + max(0, n - nl - 20)))
        assert len(pods_l) == nl and len(pods_f) == n - nl
        recs.append((list(zip(pods_l, rng.choice(pool, nl).tolist())), list(zip(pods_f, rng.choice(pool, n - nl).tolist()))))
    fleet, reg = fleet_of(recs, pods=TABLE)
    fleet.now = now
    return fleet, reg


def test_rows_on_both_sides_of_the_long_row_path_and_of_its_tile(long_rows):
    fleet, reg = long_rows
    io, now = fleet.pods["id_order"], int(fleet.now)
    s = loaded(fleet)
    try:
        rows = []
        for i, n in enumerate(LENGTHS):
            # as stored; the overlay adds one (n + 1); it moves one from the loaded to the failed list (n); pod 5: in both lists of
            # the longer rows (nothing changes), loaded only in the shorter ones
            rows += [req_row(i), req_row(i, 45, True), req_row(i, 0), req_row(i, 5)]
        got_rows, copies = check(s, reg, io, rows, now)
        lens = (got_rows["n_not_checked"] + got_rows["n_failed"]).tolist()
        assert lens[0::4] == LENGTHS and lens[2::4] == LENGTHS
        assert lens[1::4] == [n + 1 for n in LENGTHS]  # 64 -> 65 and 1024 -> 1025 by the overlay
        for i in range(len(rows)):  # (what the comparison above implies, said directly: descending, a permutation of the row)
            t = copies["time"][got_rows["copy_off"][i]:got_rows["copy_off"][i] + lens[i]]
            assert (t[:-1] >= t[1:]).all()
        # each length alone (the long row first in the output), and the long rows alone
        for i in range(len(LENGTHS)):
            check(s, reg, io, [req_row(i, 7)], now, f"length {LENGTHS[i]} alone")
        check(s, reg, io, [req_row(i) for i in range(3, len(LENGTHS))] * 2, now, "long rows only")
    finally:
        s.close()


# ---- the CPU tests' boundary cases ------------------------------------------------------------------------------------------

def test_the_cpu_boundary_cases_replayed_on_the_device(monkeypatch):
    """Every batch the by-hand CPU tests send through both forms, collected and merged into one registry and one batch (plus each
    one alone on the merged registry)."""
    calls = []
    orig = cpu.both

    def recording(records, rows, now=cpu.NOW):
        calls.append((list(records), list(rows), now))
        return orig(records, rows, now)

    monkeypatch.setattr(cpu, "both", recording)
    for t in (cpu.test_no_record, cpu.test_overlay_onto_a_loaded_instance_and_onto_a_failed_one,
              cpu.test_where_the_overlay_goes_in_id_order_beside_an_unresolved_entry, cpu.test_ties_keep_the_concatenation_order,
              cpu.test_times_at_the_ends_of_the_long_range, cpu.test_a_model_requested_twice_and_the_offsets):
        t()
    for miss in (False, True):
        cpu.test_the_four_list_shapes_with_and_without_a_miss(miss)
    assert len(calls) >= 25 and all(now == cpu.NOW for _, _, now in calls), len(calls)
    records, batches = [], []
    for recs, rows, _ in calls:
        base = len(records)
        records += recs
        batches.append([(m + base if m >= 0 else -1, fp, fl, rs) for m, fp, fl, rs in rows])
    fleet, reg = fleet_of(records, pods=8, id_order=cpu.ID_ORDER)
    s = loaded(fleet)
    try:
        check(s, reg, cpu.ID_ORDER, [q for b in batches for q in b], cpu.NOW, "merged")
        for k, b in enumerate(batches):
            check(s, reg, cpu.ID_ORDER, b, cpu.NOW, f"call {k}")
    finally:
        s.close()


# ---- batches by construction ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pods,models,n", [(8, 300, 500), (300, 2000, 3000)])
def test_batches_by_construction_take_every_case(pods, models, n):
    fleet, reg, planted, rng = cpu.status_fleet(pods, pods, models)
    io, now = fleet.pods["id_order"], int(fleet.now)
    s = loaded(fleet)
    try:
        for batch in range(3):
            reqs = sm.draw_reqs(reg, io, now, rng, n, planted)
            missing = set(sm.CASES) - sm.cases_seen(reg, io, reqs, now)
            assert not missing, (batch, missing)
            check(s, reg, io, reqs, now, f"batch {batch}")
    finally:
        s.close()


def test_four_thousand_requests_on_c3():
    fleet = wl.make_fleet("C3")
    reg = ro.registry_from_arrays(fleet.models, fleet.ent_pod, fleet.ent_time)
    io, now = fleet.pods["id_order"], int(fleet.now)
    planted = sm.seed_shapes(reg, io, now)
    fleet.models, fleet.ent_pod, fleet.ent_time = ro.registry_to_arrays(reg)
    s = loaded(fleet)
    try:
        reqs = sm.draw_reqs(reg, io, now, np.random.default_rng(3), 4096, planted)
        missing = set(sm.CASES) - sm.cases_seen(reg, io, reqs, now)
        assert not missing, missing
        rows, copies = check(s, reg, io, reqs, now)
        assert len(rows) == 4096 and len(copies) > 2000
    finally:
        s.close()


# ---- requests and buffers ---------------------------------------------------------------------------------------------------

def test_one_model_twice_sizes_only_truncation_and_two_runs(small):
    fleet, reg, planted, _ = small
    io, now = fleet.pods["id_order"], int(fleet.now)
    by = [int(p) for p in np.argsort(io, kind="stable")]
    s = loaded(fleet)
    try:
        # record 3 (both lists, an unresolved entry) under four different overlays in one batch
        rows, copies = check(s, reg, io, [req_row(3, by[1]), req_row(3), req_row(3, by[7], True), req_row(3, by[4]), req_row(3, by[2])], now)
        assert rows["n_failed"].tolist() == [5, 4, 5, 5, 4] and rows["n_not_checked"].tolist() == [2, 2, 2, 1, 2]
        assert rows["cls"].tolist() == [MST_ASK, MST_ASK, MST_LOADING_FAILED, MST_ASK, MST_ASK]
        reqs = sm.draw_reqs(reg, io, now, np.random.default_rng(77), 300, planted)
        want = sm.status_sequential(reg, io, reqs, now)
        total = len(want[1])
        SENT = 0xA5
        # sizes only
        rows, copies, got_total, rc = s.models_status_raw(reqs, now, 0, fill=SENT)
        assert rc == 0 and got_total == total and len(copies) == 0
        assert_same_status((rows, want[1]), want, "sizes only")
        # a truncated list: the prefix exact (cutting a request's copies in two), the bytes behind it untouched, the total right
        mid = next(i for i in range(100, 300) if int(want[0]["n_not_checked"][i] + want[0]["n_failed"][i]) >= 2)
        cut = int(want[0]["copy_off"][mid]) + 1
        assert 0 < cut < total
        from modelmesh_amd.solver import ptr
        import ctypes as C
        buf = np.zeros(total, dtype=STATUS_COPY)
        buf.view(np.uint8)[:] = SENT
        out_rows, n_out = np.zeros(300, dtype=STATUS_ROW), C.c_int32(-1)
        assert s.lib.mmp_models_status(s.h, ptr(reqs), 300, now, ptr(out_rows), ptr(buf), cut, C.byref(n_out)) == 0
        assert n_out.value == total and np.array_equal(out_rows, want[0])
        assert np.array_equal(buf[:cut], want[1][:cut]) and (buf[cut:].view(np.uint8) == SENT).all()
        # more room than needed: the rest stays as it was
        rows, copies, got_total, rc = s.models_status_raw(reqs, now, total, fill=SENT)
        assert rc == 0
        assert_same_status((rows, copies), want, "exact room")
        # two runs of one batch: byte-identical
        a, b = s.models_status(reqs, now), s.models_status(reqs, now)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[1].tobytes() == want[1].tobytes()
    finally:
        s.close()


def test_refused_calls_write_nothing(small):
    fleet, reg, _, _ = small
    io, now, M, P = fleet.pods["id_order"], int(fleet.now), fleet.n_models, fleet.n_pods
    SENT = 0x5A
    s = loaded(fleet)
    try:
        good = [req_row(1), req_row(3, 2)]
        bad = {"model past the registry": ([req_row(M)], now), "model below -1": ([req_row(-2)], now),
               "pod past the table": ([req_row(1, P)], now), "pod below -1": ([req_row(1, -2)], now),
               "an unknown flag bit": ([(1, -1, 2, 0)], now), "reserved": ([(1, -1, 0, 1)], now),
               "now = 0 with a fail_pod": ([req_row(1, 2)], 0), "now < 0 with a fail_pod": ([req_row(-1, 2)], -5)}
        for what, (rows, t) in bad.items():
            reqs = reqs_array(good + rows)
            out_rows, copies, total, rc = s.models_status_raw(reqs, t, 16, fill=SENT)
            assert rc == _lib.MMP_EINVAL and total == -1, (what, rc, total)
            assert (out_rows.view(np.uint8) == SENT).all() and (copies.view(np.uint8) == SENT).all(), what
        # NULL buffers that are required
        reqs = reqs_array(good)
        assert s.models_status_raw(reqs, now, 0, null_out=True)[3] == _lib.MMP_EINVAL
        import ctypes as C
        from modelmesh_amd.solver import ptr
        out_rows, n_out = np.zeros(2, dtype=STATUS_ROW), C.c_int32(-1)
        assert s.lib.mmp_models_status(s.h, None, 2, now, ptr(out_rows), None, 0, C.byref(n_out)) == _lib.MMP_EINVAL
        assert s.lib.mmp_models_status(s.h, ptr(reqs), 2, now, ptr(out_rows), None, 4, C.byref(n_out)) == _lib.MMP_EINVAL
        assert s.lib.mmp_models_status(s.h, ptr(reqs), -1, now, ptr(out_rows), None, 0, C.byref(n_out)) == _lib.MMP_EINVAL
        assert n_out.value == -1 and not out_rows.view(np.uint8).any()
        # now <= 0 without a fail_pod is no error: no clock is read
        check(s, reg, io, [req_row(1), req_row(-1)], 0)
        check(s, reg, io, good, now)  # and the context answers as before
    finally:
        s.close()


def test_before_the_first_commit(small):
    fleet, reg, _, _ = small
    io, now = fleet.pods["id_order"], int(fleet.now)
    s = loaded(fleet, commit=False)
    try:
        check(s, reg, io, [req_row(i, -1, i % 2 == 1) for i in range(-1, 40)], now, "no fail_pod before the first commit")
        out_rows, copies, total, rc = s.models_status_raw(reqs_array([req_row(1), req_row(3, 2)]), now, 16, fill=0x33)
        assert rc == _lib.MMP_ESTATE and total == -1 and (out_rows.view(np.uint8) == 0x33).all() and (copies.view(np.uint8) == 0x33).all()
        s.commit()
        check(s, reg, io, [req_row(1), req_row(3, 2)], now, "after the commit")
    finally:
        s.close()


# ---- other writers ----------------------------------------------------------------------------------------------------------

def check_resident(s, id_order, reqs, now, what=""):
    """The answers equal the sequential form on the registry read back; returns (registry, answers)."""
    reg = ro.registry_from_arrays(*s.get_models())
    return reg, check(s, reg, id_order, reqs, now, what)


def test_after_applied_ops_and_an_applied_prune(small):
    fleet0, reg0, planted, _ = small
    fleet = copy.deepcopy(fleet0)
    fleet.pods["flags"] = np.where(fleet.pods["flags"] & _lib.POD_TOMBSTONE, _lib.POD_LIVE, fleet.pods["flags"])
    fleet.ent_time = np.where(fleet.ent_time > 0, np.minimum(fleet.ent_time, fleet.now - 2 * GONE), fleet.ent_time)  # old enough to prune
    io, now = fleet.pods["id_order"], int(fleet.now)
    s = loaded(fleet)
    try:
        reqs = sm.draw_reqs(reg0, io, now, np.random.default_rng(5), 400, planted)
        reg_a, before = check_resident(s, io, reqs, now, "as loaded")
        ops = ro.ops_array([ro.op_row(m, m % 8, ROP_REGISTER, load_time=now + m) for m in range(0, 120, 2)])
        _, edits, info = s.registry_ops(ops, now, apply=True)
        assert int(info["n_edits"]) == 60
        reg_b, after = check_resident(s, io, reqs, now, "after the ops")
        assert after[0].tobytes() != before[0].tobytes()
        s.remove_pods(np.array([3], np.int32))
        s.commit()
        s.prune_registry(0, now - GONE - 60_000, apply=False)  # first sighting
        _, removed, pinfo = s.prune_registry(0, now + 1_000, apply=True)
        assert int(pinfo["n_removed"]) == len(removed) > 0
        no3 = reqs.copy()
        no3["fail_pod"] = np.where(no3["fail_pod"] == 3, 4, no3["fail_pod"])
        check_resident(s, s.get_pods()["id_order"], no3, now, "after the prune")
    finally:
        s.close()


def test_after_json_events_without_a_commit():
    from tests.test_registry_upsert_json_gpu import fleet_pair, fleet_values, value_of
    pair, fleet, rng = fleet_pair(9, 8, 60)
    try:
        pair.start(fleet_values(fleet, np.arange(60), pair.ids, pair.type_names, rng))
        s, now = pair.j, int(fleet.now)
        io = s.get_pods()["id_order"]
        reqs = reqs_array([req_row(m, fp, miss) for m in range(-1, 60) for fp, miss in ((-1, False), (m % 8, True))])
        _, before = check_resident(s, io, reqs, now, "as ingested")
        recs = [(0, 9, ((1, now - 5), (4, now - 5)), ((2, now), (6, now - 9))), (0, 11, (), ((7, 3),)), (0, 4, ((0, now + 7),), ())]
        st, _ = s.upsert_models_json([value_of(r, pair.ids, pair.type_names) for r in recs] + ["{}"], [0, 5, 60, 7], deleted=[0, 0, 0, 1])
        assert not st.any()
        reqs2 = reqs_array([tuple(q) for q in reqs] + [req_row(60), req_row(60, 0), req_row(60, 2, True), req_row(7, 1)])
        reg, after = check_resident(s, io, reqs2, now, "after the events")
        assert list(reg[0].load_failed_instance_ids.items()) == [(2, now), (6, now - 9)] and not reg[7].instance_ids
        assert sm.copies_of(*after, len(reqs2) - 1) == [(1, 1, now)]  # the deleted record: an ordinary record without copies
    finally:
        pair.close()


def test_beside_registry_ops_every_answer_is_one_state_or_the_other(small):
    fleet, reg0, planted, _ = small
    io, now = fleet.pods["id_order"], int(fleet.now)
    by = [int(p) for p in np.argsort(io, kind="stable")]
    models = np.arange(20, 120)
    reg_a = copy.deepcopy(reg0)
    for m in models:  # state A: none of them holds by[6]; state B: all do, loaded at now + m
        reg_a[m].instance_ids.pop(by[6], None)
        reg_a[m].load_failed_instance_ids.pop(by[6], None)
    fleet_a = copy.deepcopy(fleet)
    fleet_a.models, fleet_a.ent_pod, fleet_a.ent_time = ro.registry_to_arrays(reg_a)
    reg_b = ro.Registry(copy.deepcopy(reg_a), io.copy())
    to_b = ro.ops_array([ro.op_row(int(m), by[6], ROP_REGISTER, last_used=1, load_time=now + int(m)) for m in models])
    to_a = ro.ops_array([ro.op_row(int(m), by[6], ROP_DEREGISTER, last_used=1) for m in models])
    reg_b.run(to_b, now)
    reqs = reqs_array([req_row(int(m), by[6] if m % 3 == 0 else (by[2] if m % 3 == 1 else -1), m % 2 == 0) for m in range(0, 140)])
    wa, wb = sm.status_sequential(reg_a, io, reqs, now), sm.status_sequential(reg_b.records, io, reqs, now)
    s = loaded(fleet_a)
    try:
        results, errors, done = [], [], threading.Event()

        def ask():
            try:
                for _ in range(200):
                    results.append(s.models_status(reqs, now))
            except Exception as ex:  # noqa: BLE001
                errors.append(ex)
            finally:
                done.set()

        th = threading.Thread(target=ask)
        th.start()
        flips, in_b, rng = 0, False, np.random.default_rng(31)
        try:
            while not done.is_set():
                # at random, whatever the state is (a strict alternation falls into step with the other thread: two batches per
                # answer); registering twice replaces the entry by itself, deregistering twice changes nothing
                in_b = bool(rng.random() < 0.5)
                s.registry_ops_raw(to_b if in_b else to_a, now, _lib.ROPS_APPLY, len(models), want_status=False)
                flips += 1
        finally:
            th.join()
        assert not errors, errors
        assert len(results) == 200
        saw_b = 0
        for rows, copies in results:
            for i in range(len(reqs)):
                got = (rows[i]["cls"], rows[i]["n_not_checked"], rows[i]["n_failed"], sm.copies_of(rows, copies, i))
                want = [(w[0][i]["cls"], w[0][i]["n_not_checked"], w[0][i]["n_failed"], sm.copies_of(*w, i)) for w in (wa, wb)]
                assert got in want, (i, got, want)
            saw_b += rows.tobytes() == wb[0].tobytes()
        print(f"200 calls beside {flips} applied batches: {saw_b} saw every record registered")
        assert 0 < saw_b < 200  # both states were seen
        last = wb if in_b else wa
        assert_same_status(s.models_status(reqs, now), last, "afterwards")
    finally:
        s.close()


# ---- the veneer -------------------------------------------------------------------------------------------------------------

def test_the_veneer_entry_runs_under_the_mock_jvm(tmp_path, small):
    from tests import jni_mock as jmock
    from tests.test_jni_veneer import _java_natives
    veneer = jmock.Veneer(jmock.build(tmp_path), _java_natives())
    env = veneer.env
    fleet, reg, planted, _ = small
    io, now = fleet.pods["id_order"], int(fleet.now)
    h = veneer.call("create", 0, fleet.min_space_units, fleet.min_churn_age_ms)
    assert h != 0 and env.pending() is None
    try:
        assert veneer.call("podsLoad", h, jmock.ByteBuffer(fleet.pods), fleet.n_pods) == 0
        assert veneer.call("modelsLoad", h, jmock.ByteBuffer(fleet.models), fleet.n_models, jmock.ByteBuffer(fleet.ent_pod),
                           jmock.ByteBuffer(fleet.ent_time), len(fleet.ent_pod)) == 0
        assert veneer.call("commit", h) == 0 and env.pending() is None
        reqs = sm.draw_reqs(reg, io, now, np.random.default_rng(8), 90, planted)
        want = sm.status_sequential(reg, io, reqs, now)
        rows, n_out = jmock.ByteBuffer(np.zeros(90, dtype=STATUS_ROW)), jmock.ByteBuffer(np.full(1, -1, np.int32))
        assert veneer.call("modelsStatus", h, jmock.ByteBuffer(reqs), 90, now, rows, None, 0, n_out) == 0 and env.pending() is None
        assert int(n_out.arr[0]) == len(want[1]) and np.array_equal(rows.arr, want[0])
        copies = jmock.ByteBuffer(np.zeros(len(want[1]), dtype=STATUS_COPY))
        assert veneer.call("modelsStatus", h, jmock.ByteBuffer(reqs), 90, now, rows, copies, len(want[1]), n_out) == 0 and env.pending() is None
        assert_same_status((rows.arr, copies.arr), want, "through the veneer")
        # a short buffer is refused before the library is called
        short = jmock.ByteBuffer(np.zeros(len(want[1]) - 1, dtype=STATUS_COPY))
        assert veneer.call("modelsStatus", h, jmock.ByteBuffer(reqs), 90, now, rows, short, len(want[1]), n_out) == -1
        assert env.pending()[0] == "java/lang/IllegalArgumentException" and "copiesOut shorter" in env.pending()[1]
        env.clear()
    finally:
        veneer.call("destroy", h)
