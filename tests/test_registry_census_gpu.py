"""mmp_registry_census on the device against the Python restatement of the registry listener's model counts
(tests/registry_census_model.py): every field and array, all integers, exact — at the wave and workgroup edges, with every atomic
on one address, on both sides of the per-pod and per-type LDS thresholds, up to C3; after an applied prune and janitor plan,
after an upsert without a commit; buffer handling; beside registry events on another thread; the JNI veneer."""
import threading

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd import workload as wl
from modelmesh_amd.solver import MmpError, Solver
from tests import janitor_model as jm
from tests import registry_census_model as cm
from tests import registry_prune_model as rp
from tests.registry_census_model import assert_same_census
from tests.registry_prune_model import GONE_AFTER_MS as GONE, LONG_MAX

pytestmark = pytest.mark.gpu

# the two pod-sized arrays are counted in LDS up to 80 KB together (csrc/census_kernels.hpp: kCensusPodLdsBytes), the per-type
# rows up to 512 types (kCensusTypeSlots)
POD_LDS_MAX_PODS = 80 * 1024 // 8
TYPE_LDS_MAX_TYPES = 512


def census_fleet(seed, pods, models, base=None):
    """A fuzz fleet with what the census distinguishes: ids the table does not know on both sides of it, Long.MAX / zero / negative
    lastUsed, types on both sides of the type table."""
    fleet = base if base is not None else wl.fuzz_fleet(seed + 1300, pods=pods, models=models)
    rng = np.random.default_rng(55_000 + seed)
    n_ent, M, T = len(fleet.ent_pod), fleet.n_models, fleet.n_types
    fleet.ent_pod = np.where(rng.random(n_ent) < 0.03, rng.choice([-1, pods, pods + 7], n_ent), fleet.ent_pod).astype(np.int32)
    fleet.models["last_used"] = np.where(rng.random(M) < 0.05, rng.choice([0, -1, LONG_MAX], M), fleet.models["last_used"])
    fleet.models["type"] = np.where(rng.random(M) < 0.05, rng.choice([-1, T, T + 3], M), fleet.models["type"])
    return fleet


def staged(fleet, commit=False):
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    s.load_fleet(fleet, commit=commit)
    return s


def want_of(fleet):
    return cm.census_closed(fleet.models, fleet.ent_pod, fleet.n_pods, fleet.n_types)


def check_resident(s, what=""):
    """The census equals the closed form over the registry read back; returns it."""
    models, ent_pod, _ = s.get_models()
    n_pods, n_types = s.registry_census_sizes()
    got = s.registry_census()
    assert_same_census(got, cm.census_closed(models, ent_pod, n_pods, n_types), what)
    return got


@pytest.mark.parametrize("models", [0, 1, 63, 64, 65, 255, 256, 257])
def test_wave_and_workgroup_edges(models):
    """P = 8, before the first commit: partial last waves, one workgroup and the first row of a second one."""
    fleet = census_fleet(models, 8, max(models, 1))
    if models == 0:
        fleet.models, fleet.ent_pod, fleet.ent_time = fleet.models[:0], fleet.ent_pod[:0], fleet.ent_time[:0]
    s = staged(fleet)
    try:
        got = s.registry_census()
        assert int(got[0]["n_models"]) == models and len(got[1]) == len(got[2]) == 8 and len(got[3]) == fleet.n_types
        assert_same_census(got, want_of(fleet), "closed")
        assert_same_census(got, cm.census_of_arrays(fleet.models, fleet.ent_pod, fleet.ent_time, 8, fleet.n_types), "sequential")
        if models == 0:
            assert not got[1].any() and not got[2].any() and all(int(got[0][f]) == 0 for f in cm.SCALARS)
    finally:
        s.close()


def _by_hand(pods, rows, ent_pod, n_types=0):
    """A fleet around hand-made registry rows: (type, n_loaded, n_failed, last_used) per model, entries in order."""
    fleet = wl.fuzz_fleet(1399, pods=pods, models=1)
    fleet.n_types, fleet.allowed, fleet.prefer, fleet.has_allowed, fleet.has_prefer = n_types, None, None, None, None
    m = np.zeros(len(rows), dtype=_lib.MODEL_ROW)
    off = 0
    for i, (ty, nl, nf, lu) in enumerate(rows):
        m[i] = (ty, off, nl, nf, lu)
        off += nl + nf
    fleet.models, fleet.ent_pod = m, np.asarray(ent_pod, np.int32)
    assert off == len(fleet.ent_pod)
    fleet.ent_time = np.full(off, fleet.now - 1000, np.int64)
    return fleet


def test_every_atomic_on_one_address():
    """P = 1 and 2 000 models all registered on it, every third with a failure record there too."""
    rows = [(0, 1, 1 if i % 3 == 0 else 0, 1_000 + i) for i in range(2000)]
    fleet = _by_hand(1, rows, np.zeros(sum(r[1] + r[2] for r in rows), np.int32))
    s = staged(fleet)
    try:
        got = s.registry_census()
        assert_same_census(got, want_of(fleet))
        assert got[1].tolist() == [2000] and got[2].tolist() == [667] and int(got[0]["n_loaded_and_failed"]) == 667
    finally:
        s.close()


def test_sixty_four_copies_and_ten_failures():
    P = 80
    rows = [(0, 64, 10, 5), (0, 3, 0, 5), (0, 4, 0, 5), (0, 0, 0, 5)]
    ent = list(range(64)) + list(range(64, 74)) + [0, 1, 2] + [0, 1, 2, 3]
    fleet = _by_hand(P, rows, ent)
    s = staged(fleet)
    try:
        st, pl, pf, _ = got = s.registry_census()
        assert_same_census(got, want_of(fleet))
        assert int(st["max_copies"]) == 64 and st["copies_hist"].tolist() == [1, 0, 0, 1, 2]
        assert int(st["n_entries_loaded"]) == 71 and int(st["n_entries_failed"]) == 10
        assert pl[:4].tolist() == [3, 3, 3, 2] and pl[4:64].tolist() == [1] * 60 and pf[64:74].tolist() == [1] * 10 and not pl[64:].any()
    finally:
        s.close()


def test_a_registry_in_which_every_entry_is_unresolved():
    fleet = census_fleet(7, 20, 500)
    fleet.ent_pod = np.where(np.arange(len(fleet.ent_pod)) % 2 == 0, -1, fleet.n_pods).astype(np.int32)
    s = staged(fleet)
    try:
        st, pl, pf, _ = got = s.registry_census()
        assert_same_census(got, want_of(fleet))
        assert not pl.any() and not pf.any()
        assert int(st["n_entries_unresolved"]) == len(fleet.ent_pod) == int(st["n_entries_loaded"] + st["n_entries_failed"]) > 0
        assert int(st["n_loaded"]) > 0  # the records still count as loaded
    finally:
        s.close()


def test_types_outside_the_table_and_no_type_table():
    rows = [(-1, 1, 0, 5), (2, 1, 1, 5), (1, 1, 0, 5), (0, 0, 1, 5), (7, 2, 0, 5)]
    ent = [0, 0, 1, 1, 1, 0, 1]
    for n_types in (2, 0):
        fleet = _by_hand(2, rows, ent, n_types=n_types)
        s = staged(fleet)
        try:
            st, _, _, ts = got = s.registry_census()
            assert_same_census(got, want_of(fleet))
            assert int(st["n_models"]) == 5 and int(st["n_loaded"]) == 4 and len(ts) == n_types
            if n_types:
                assert ts["n_models"].tolist() == [1, 1] and ts["n_loaded"].tolist() == [0, 1] and ts["n_failed"].tolist() == [1, 0]
        finally:
            s.close()


@pytest.mark.parametrize("pods", [POD_LDS_MAX_PODS, POD_LDS_MAX_PODS + 1])
def test_both_sides_of_the_per_pod_privatisation_threshold(pods):
    """300 models; the pod table's size picks the kernel.  The last slots of the table hold registrations on both sides."""
    fleet = census_fleet(pods % 7, pods, 300)
    fleet.ent_pod[:6] = [pods - 1, pods - 2, 0, pods - 1, pods, -1]
    s = staged(fleet)
    try:
        got = s.registry_census()
        assert_same_census(got, want_of(fleet))
        assert got[1][pods - 1] + got[2][pods - 1] >= 2
    finally:
        s.close()


@pytest.mark.parametrize("n_types", [TYPE_LDS_MAX_TYPES, TYPE_LDS_MAX_TYPES + 1])
def test_both_sides_of_the_per_type_table_threshold(n_types):
    rng = np.random.default_rng(n_types)
    rows = [(int(t), int(nl), int(nf), 5) for t, nl, nf in zip(rng.integers(-1, n_types + 2, 700), rng.integers(0, 4, 700), rng.integers(0, 2, 700))]
    rows[0], rows[1] = (n_types - 1, 2, 1, 5), (n_types, 1, 0, 5)
    fleet = _by_hand(8, rows, rng.integers(0, 8, sum(r[1] + r[2] for r in rows)), n_types=n_types)
    s = staged(fleet)
    try:
        got = s.registry_census()
        assert_same_census(got, want_of(fleet))
        assert len(got[3]) == n_types and int(got[3]["n_models"][n_types - 1]) >= 1
    finally:
        s.close()


def test_a_c3_sized_registry():
    fleet = census_fleet(3, 10_000, 100_000, wl.make_fleet("C3"))
    s = staged(fleet)
    try:
        got = s.registry_census()
        assert_same_census(got, want_of(fleet))
        assert int(got[0]["n_models"]) == 100_000 and len(got[1]) == 10_000 and len(got[3]) == 4
    finally:
        s.close()


def prune_inputs(seed, pods, models):
    """prune_fleet-style inputs: entry ages on both sides of gone-after, some ids not in the pod table, Long.MAX records, and 5 % of
    the instances gone."""
    rng = np.random.default_rng(78_000 + seed)
    fleet = wl.fuzz_fleet(seed + 1400, pods=pods, models=models)
    now, n_ent = fleet.now, len(fleet.ent_pod)
    fleet.pods["flags"] = np.where(fleet.pods["flags"] & _lib.POD_TOMBSTONE, _lib.POD_LIVE, fleet.pods["flags"])
    fleet.ent_time = (now - rng.choice([1_000, GONE - 1, GONE, GONE + 1, 2 * GONE, 86_400_000], n_ent)).astype(np.int64)
    fleet.ent_pod = np.where(rng.random(n_ent) < 0.01, -1, fleet.ent_pod).astype(np.int32)
    fleet.models["last_used"] = np.where(rng.random(models) < 0.01, LONG_MAX, fleet.models["last_used"])
    gone = np.sort(rng.choice(np.arange(1, pods), size=max(3, pods // 20), replace=False)).astype(np.int32)
    return fleet, gone


def test_after_an_applied_prune():
    fleet, gone = prune_inputs(1, 120, 3000)
    s = staged(fleet, commit=True)
    try:
        s.remove_pods(gone)
        s.commit()
        s.prune_registry(0, fleet.now - GONE - 60_000, apply=False)  # first sighting: the marks, older than gone-after at `now`
        before = check_resident(s, "before the prune")
        edits, removed, info = s.prune_registry(0, fleet.now, apply=True)
        assert int(info["n_removed"]) == len(removed) > 0 and int(info["n_repaired"]) > 0
        st, pl, pf, _ = check_resident(s, "after the prune")
        # the gone instances' counts drop by exactly the removed entries, nobody else's changes
        assert np.isin(removed["pod"], gone).all()
        assert np.array_equal(before[1] - pl, np.bincount(removed["pod"][removed["failed"] == 0], minlength=fleet.n_pods))
        assert np.array_equal(before[2] - pf, np.bincount(removed["pod"][removed["failed"] == 1], minlength=fleet.n_pods))
        assert int(before[0]["n_entries_loaded"] - st["n_entries_loaded"]) == int((removed["failed"] == 0).sum())
        assert int(st["n_last_used_max"]) == 0 < int(before[0]["n_last_used_max"])  # the repair
        assert int(st["n_loaded"]) < int(before[0]["n_loaded"])  # some model lost its only copies
    finally:
        s.close()


def test_after_an_applied_janitor_plan():
    fleet, self_pod, reg = jm.janitor_fleet(13, 64, 1500)
    s = staged(fleet, commit=True)
    try:
        before = check_resident(s, "before the plan")
        now = int(fleet.now)
        out = s.janitor_plan(jm.make_cache(fleet, reg, self_pod, 13_000, now), jm.params(self_pod, now), apply=True)
        assert int(out[4]["n_edits"]) > 0
        st, pl, pf, _ = check_resident(s, "after the plan")
        others = np.arange(fleet.n_pods) != self_pod
        assert np.array_equal(pl[others], before[1][others]) and np.array_equal(pf[others], before[2][others])  # the janitor edits its own registrations
        assert (pl[self_pod], pf[self_pod]) != (before[1][self_pod], before[2][self_pod])
    finally:
        s.close()


def _states(fleet, n=200):
    """Two replacements for the first n records: A — two copies each on pods 0 and 1; B — no copy, a failure on pod 2."""
    idx = np.arange(n, dtype=np.int32)
    a = np.zeros(n, dtype=_lib.MODEL_ROW)
    a["type"], a["ent_off"], a["n_loaded"], a["last_used"] = fleet.models["type"][:n], 2 * idx, 2, 77
    b = np.zeros(n, dtype=_lib.MODEL_ROW)
    b["type"], b["ent_off"], b["n_failed"], b["last_used"] = fleet.models["type"][:n], idx, 1, LONG_MAX
    A = (idx, a, np.tile(np.array([0, 1], np.int32), n), np.full(2 * n, fleet.now, np.int64))
    B = (idx, b, np.full(n, 2, np.int32), np.full(n, fleet.now, np.int64))
    return A, B


def _want_after(fleet, state):
    reg = rp.registry_from_arrays(fleet.models, fleet.ent_pod, fleet.ent_time)
    for i, row in zip(state[0], rp.registry_from_arrays(state[1], state[2], state[3])):
        reg[i] = row
    models, ent_pod, _ = rp.registry_to_arrays(reg)
    return cm.census_closed(models, ent_pod, fleet.n_pods, fleet.n_types)


def test_an_upsert_without_a_commit_is_seen():
    fleet = census_fleet(21, 16, 700)
    A, B = _states(fleet)
    s = staged(fleet)
    try:
        assert_same_census(s.registry_census(), want_of(fleet), "as loaded")
        s.upsert_models(*A)
        assert_same_census(s.registry_census(), _want_after(fleet, A), "after A")
        s.upsert_models(*B)
        assert_same_census(s.registry_census(), _want_after(fleet, B), "after B")
        new = np.zeros(1, dtype=_lib.MODEL_ROW)  # a record appended: the registry grows
        new["n_loaded"], new["last_used"] = 1, 5
        s.upsert_models(np.array([700], np.int32), new, np.array([15], np.int32), np.array([fleet.now], np.int64))
        got = check_resident(s, "after an append")
        assert int(got[0]["n_models"]) == 701
    finally:
        s.close()


def test_buffers_too_small_null_and_twice_in_a_row():
    fleet = census_fleet(22, 40, 600)
    fleet.n_types, fleet.allowed, fleet.prefer, fleet.has_allowed, fleet.has_prefer = 3, None, None, None, None
    fleet.models["type"] = np.arange(600) % 4
    s = staged(fleet)
    try:
        want = want_of(fleet)
        first = s.registry_census()
        assert_same_census(first, want)
        SENT = -123456
        # too small: MMP_EINVAL, the arrays untouched, the two counts set
        for mp, mt in ((39, 3), (40, 2), (1, 0), (0, 1)):
            st, pl, pf, ts, n_pods, n_types, rc = s.registry_census_raw(mp, mt, fill=SENT)
            assert rc == _lib.MMP_EINVAL and (n_pods, n_types) == (40, 3), (mp, mt, rc)
            assert (pl == SENT).all() and (pf == SENT).all() and (ts.view(np.int32) == SENT).all()
            assert all(int(st[f]) == 0 for f in cm.SCALARS)  # the totals were not written either
        # NULL buffers: the totals only
        st, pl, pf, ts, n_pods, n_types, rc = s.registry_census_raw(0, 0)
        assert rc == 0 and (n_pods, n_types) == (40, 3) and len(pl) == len(ts) == 0
        assert_same_census((st, want[1], want[2], want[3]), want, "totals only")
        # one kind of buffer without the other, and more room than needed (the rest stays as it was)
        st, pl, pf, ts, _, _, rc = s.registry_census_raw(0, 3)
        assert rc == 0
        assert_same_census((st, want[1], want[2], ts), want, "types only")
        st, pl, pf, ts, _, _, rc = s.registry_census_raw(50, 0, fill=SENT)
        assert rc == 0 and (pl[40:] == SENT).all() and (pf[40:] == SENT).all()
        assert_same_census((st, pl[:40], pf[:40], want[3]), want, "pods only")
        with pytest.raises(MmpError):
            s._ck(s.lib.mmp_registry_census(s.h, None, None, None, 0, None, None, 0, None))
        # twice in a row: nothing of the first call is left in the second
        second = s.registry_census()
        assert_same_census(second, first, "second call")
        assert_same_census(second, want, "second call")
    finally:
        s.close()


def test_beside_registry_events_every_census_is_one_state_or_the_other():
    fleet = census_fleet(23, 16, 700)
    A, B = _states(fleet)
    wa, wb = _want_after(fleet, A), _want_after(fleet, B)
    assert int(wa[0]["n_loaded"]) != int(wb[0]["n_loaded"]) and not np.array_equal(wa[1], wb[1])
    s = staged(fleet, commit=True)
    try:
        s.upsert_models(*A)
        results, errors, done = [], [], threading.Event()

        def count():
            try:
                for _ in range(200):
                    results.append(s.registry_census())
            except Exception as ex:  # noqa: BLE001
                errors.append(ex)
            finally:
                done.set()

        th = threading.Thread(target=count)
        th.start()
        flips, rng = 0, np.random.default_rng(23)
        try:
            while not done.is_set():
                s.upsert_models(*(B if rng.random() < 0.5 else A))  # (at random: a strict alternation falls into step with the other thread)
                flips += 1
        finally:
            th.join()
        assert not errors, errors
        sides = []
        for got in results:
            is_a = int(got[0]["n_loaded"]) == int(wa[0]["n_loaded"])
            assert_same_census(got, wa if is_a else wb, "a mixture of the two states")
            sides.append(is_a)
        print(f"{len(results)} censuses beside {flips} upserts: {sum(sides)} saw A, {len(sides) - sum(sides)} saw B")
        assert len(results) == 200 and 0 < sum(sides) < 200  # both states were seen
        check_resident(s, "afterwards")
    finally:
        s.close()


def test_the_veneer_entry_runs_under_the_mock_jvm(tmp_path):
    from tests import jni_mock as jmock
    from tests.test_jni_veneer import _java_natives
    veneer = jmock.Veneer(jmock.build(tmp_path), _java_natives())
    env = veneer.env
    fleet = census_fleet(24, 40, 900)
    P = fleet.n_pods
    h = veneer.call("create", 0, fleet.min_space_units, fleet.min_churn_age_ms)
    assert h != 0 and env.pending() is None
    try:
        assert veneer.call("podsLoad", h, jmock.ByteBuffer(fleet.pods), P) == 0
        assert veneer.call("modelsLoad", h, jmock.ByteBuffer(fleet.models), fleet.n_models, jmock.ByteBuffer(fleet.ent_pod),
                           jmock.ByteBuffer(fleet.ent_time), len(fleet.ent_pod)) == 0
        want = cm.census_closed(fleet.models, fleet.ent_pod, P, 0)  # (no type table was loaded)
        stats = jmock.ByteBuffer(np.zeros(1, dtype=_lib.REGISTRY_STATS))
        pl, pf = jmock.ByteBuffer(np.zeros(P, np.int32)), jmock.ByteBuffer(np.zeros(P, np.int32))
        n_pods, n_types = jmock.ByteBuffer(np.zeros(1, np.int32)), jmock.ByteBuffer(np.full(1, -1, np.int32))
        assert veneer.call("registryCensus", h, stats, pl, pf, P, n_pods, None, 0, n_types) == 0 and env.pending() is None
        assert int(n_pods.arr[0]) == P and int(n_types.arr[0]) == 0
        assert_same_census((stats.arr[0], pl.arr, pf.arr, want[3]), want, "through the veneer")
        # the totals alone
        stats2 = jmock.ByteBuffer(np.zeros(1, dtype=_lib.REGISTRY_STATS))
        assert veneer.call("registryCensus", h, stats2, None, None, 0, n_pods, None, 0, n_types) == 0 and env.pending() is None
        assert stats2.arr.tobytes() == stats.arr.tobytes()
        # a short buffer is refused before the library is called
        short = jmock.ByteBuffer(np.zeros(P - 1, np.int32))
        assert veneer.call("registryCensus", h, stats, pl, short, P, n_pods, None, 0, n_types) == -1
        assert env.pending()[0] == "java/lang/IllegalArgumentException" and "podFailedOut shorter" in env.pending()[1]
        env.clear()
    finally:
        veneer.call("destroy", h)
