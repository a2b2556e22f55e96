"""mmp_janitor_plan on the device against the sequential Python restatement of janitorTask's two loops
(tests/janitor_model.py), bit for bit: action bytes, edits, candidates and their order, every info field, over seeded sequences
of runs; the resident registry after an apply and what reads it next; the edge modes; concurrency with decisions; the veneer."""
import copy
import threading
import time

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd import workload as wl
from modelmesh_amd.solver import MmpError, Solver
from oracle import bind as ob
from oracle.bind import OracleFleet
from tests import janitor_model as jm
from tests import registry_prune_model as rp
from tests.registry_prune_model import LONG_MAX
from tests.test_registry_prune_gpu import _serve_check, same_registry
from tests.util import assert_same_decisions

pytestmark = pytest.mark.gpu

INFO_FIELDS = ("n_edits", "n_candidates", "n_ties", "stopped_at", "truncated")


def same_outputs(got, want):
    for g, w, what in zip(got[:4], want[:4], ("actions", "edits", "candidates", "candidate rows")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, g[:6], w[:6])
    for f in INFO_FIELDS:
        assert int(got[4][f]) == want[4][f], (f, got[4], want[4])
    assert list(got[4]["n_action"]) == want[4]["n_action"], (got[4], want[4])


def loaded(fleet):
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    s.load_fleet(fleet)
    return s


def setup(seed, pods, models, base=None):
    fleet, self_pod, reg = jm.janitor_fleet(seed, pods, models, base)
    return fleet, self_pod, reg, loaded(fleet)


def one_run(s, fleet, reg, self_pod, seed, now, **kw):
    """The same run on both sides (the restatement edits `reg`); asserts every output equal; returns them with the inputs."""
    entries = jm.make_cache(fleet, reg, self_pod, seed, now)
    prm = jm.params(self_pod, now)
    before = copy.deepcopy(reg)
    got = s.janitor_plan(entries, prm, **kw)
    want = jm.Janitor().run(reg, entries, prm, fleet.pods["id_order"])
    print(f"run at {now}: {len(entries)} rows, device {got[4]}")
    same_outputs(got, want)
    return entries, prm, before, want


@pytest.mark.parametrize("seed,pods,models", jm.GPU_FLEETS)
def test_three_runs_equal_the_restatement(seed, pods, models):
    fleet, self_pod, reg, s = setup(seed, pods, models, wl.make_fleet("C3") if models == 100_000 else None)
    assert (fleet.n_pods, fleet.n_models) == (pods, models)
    try:
        seen = {}
        for k in range(3):
            now = int(fleet.now) + k * jm.RUN_EVERY_MS
            entries, prm, before, (actions, edits, cands, rows, info) = one_run(s, fleet, reg, self_pod, 1000 * seed + k, now)
            v = jm.visibility(before, edits, actions, info, now)
            v["short_expiry"], v["full_expiry"], v["failure_stays"] = jm.expiry_kinds(before, reg, entries, self_pod, prm)
            for key, x in v.items():
                seen[key] = seen.get(key, 0) + x
            if models <= 2000 or k == 2:
                same_registry(s, reg)
        assert all(x > 0 for x in seen.values()), seen  # the visibility condition, on the restatement's output
    finally:
        s.close()


def test_after_an_apply_everything_downstream_sees_the_edited_records():
    fleet, self_pod, reg = jm.janitor_fleet(12, 64, 1500)
    now = int(fleet.now)
    # a cluster close to full (:6229) with a young cache (:6253-6258), or the scale-down removes nothing
    fleet.pods["used"] = fleet.pods["capacity"] - fleet.pods["capacity"] // 50
    fleet.pods["lru_time"] = now - 5_000_000
    s = loaded(fleet)
    try:
        entries, prm, before, (actions, edits, cands, rows, info) = one_run(s, fleet, reg, self_pod, 5, now)
        same_registry(s, reg)
        f2 = copy.copy(fleet)
        f2.pods = s.get_pods()
        f2.models, f2.ent_pod, f2.ent_time = rp.registry_to_arrays(reg)
        # the scale-down on the emitted candidates
        sp = np.zeros(1, dtype=_lib.SCALEDOWN_PARAMS)
        sp[0] = (self_pod, 0, now, now - 11_000, 10_000, 2_000_000, 2000, 0)
        assert len(cands) > 20
        rem = s.scaledown_plan(cands, sp)
        assert np.array_equal(rem, ob.scaledown_plan(f2, cands, sp))
        print(f"scale-down on {len(cands)} candidates: {int(rem.sum())} removed")
        assert rem.sum() > 0
        # load-target and serve decisions on the edited models, without a commit
        touched = edits["model"]
        rng = np.random.default_rng(3)
        for n in (700, 6000):
            reqs, extra = wl.fuzz_requests(f2, 40 + n, n)
            reqs["model"][::2] = rng.choice(touched, len(reqs["model"][::2]))
            want = OracleFleet(f2).place(reqs, extra, f2.now, threads=4)
            assert_same_decisions(f2, reqs, s.place(reqs, extra, f2.now), want)
        _serve_check(s, f2, rng, touched)
        # a following prune and proactive plan read the same records
        reaper = rp.Reaper()
        e, rm, pinfo = s.prune_registry(self_pod, now)
        we, wrm, winfo, _ = reaper.run(f2.pods["flags"], reg, self_pod, now)
        assert np.array_equal(e, we) and np.array_equal(rm, wrm)
        f2.models, f2.ent_pod, f2.ent_time = rp.registry_to_arrays(reg)
        gm, gl, gi = s.proactive_plan(6400, now, fleet.n_models)
        wm, wl_, wi = ob.proactive_plan(f2, 6400, now, fleet.n_models)
        assert np.array_equal(gm, wm) and np.array_equal(gl, wl_) and int(gi["n_candidates"]) == int(wi["n_candidates"])
        # and a second janitor run on the edited registry
        one_run(s, fleet, reg, self_pod, 6, now + jm.RUN_EVERY_MS)
        same_registry(s, reg)
    finally:
        s.close()


def test_the_stop_shutting_down_an_empty_cache_and_an_unnamed_pod():
    fleet, self_pod, reg, s = setup(13, 50, 1200)
    try:
        now = int(fleet.now)
        ident = fleet.pods["id_order"]
        base = jm.make_cache(fleet, reg, self_pod, 9, now)
        # the Long.MAX stop at the first, a middle and the last row: dry, so every variant sees the same registry
        for at in (0, len(base) // 2, len(base) - 1):
            entries = base.copy()
            entries["last_used"][at], entries["flags"][at] = LONG_MAX, _lib.JE_DONE | _lib.JE_STATE_LIVE
            prm = jm.params(self_pod, now)
            want = jm.Janitor().run(reg, entries, prm, ident, dry=True)
            assert want[4]["stopped_at"] == at and len(want[2]) == 0
            same_outputs(s.janitor_plan(entries, prm, dry=True), want)
        same_registry(s, reg)
        # shutting down: nothing
        prm = jm.params(self_pod, now, shutting_down=1)
        got = s.janitor_plan(base, prm)
        same_outputs(got, jm.Janitor().run(reg, base, prm, ident))
        assert not got[0].any() and int(got[4]["n_edits"]) == 0
        same_registry(s, reg)
        # a pod the registry does not name: its cache rows are registered or removed, nothing is deregistered
        other = next(p for p in range(fleet.n_pods) if p != self_pod and not (fleet.ent_pod == p).any()) if fleet.n_pods > 60 else None
        if other is None:
            other = self_pod + 1 if self_pod + 1 < fleet.n_pods else 0
            for r in reg:
                jm._remove(r.loaded, other)
                jm._remove(r.failed, other)
            s.load_models(*rp.registry_to_arrays(reg))
            s.commit()
        prm = jm.params(other, now)
        want = jm.Janitor().run(reg, base, prm, ident, dry=True)
        assert not (want[1]["flags"] & (_lib.JAN_EDIT_REM_LOADED | _lib.JAN_EDIT_REM_FAILED)).any() and len(want[1]) > 0
        same_outputs(s.janitor_plan(base, prm, dry=True), want)
        # an empty cache: every registration of self_pod goes
        prm = jm.params(self_pod, now)
        empty = np.zeros(0, dtype=_lib.JANITOR_ENTRY)
        got = s.janitor_plan(empty, prm)
        want = jm.Janitor().run(reg, empty, prm, ident)
        same_outputs(got, want)
        assert len(want[1]) > 10 and len(want[2]) == 0
        same_registry(s, reg)
        assert not any(p == self_pod for r in reg for p, _ in r.loaded)
    finally:
        s.close()


def test_truncation_dry_runs_and_refused_input_change_nothing():
    fleet, self_pod, reg, s = setup(14, 80, 2000)
    try:
        now = int(fleet.now)
        entries = jm.make_cache(fleet, reg, self_pod, 4, now)
        prm = jm.params(self_pod, now)
        want = jm.Janitor().run(reg, entries, prm, fleet.pods["id_order"], dry=True)
        ne, nc = len(want[1]), len(want[2])
        assert ne > 4 and nc > 4
        for flg in (_lib.JANITOR_APPLY, 0):
            for me, mc in ((3, nc), (ne, 2), (0, 0)):
                got = s.janitor_plan_raw(entries, prm, flg, me, mc)
                assert int(got[4]["truncated"]) == 1
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1][:me])  # the prefixes
                assert np.array_equal(got[2], want[2][:mc]) and np.array_equal(got[3], want[3][:mc])
                for f in INFO_FIELDS[:-1]:
                    assert int(got[4][f]) == want[4][f], f  # the totals
                same_registry(s, reg)
        same_outputs(s.janitor_plan(entries, prm, dry=True), want)
        same_registry(s, reg)
        same_outputs(s.janitor_plan(entries, prm, apply=False), want)  # flags = 0: the registry is the caller's to edit
        same_registry(s, reg)
        # refused: a model in two rows, a model index of M, both flags, no clock
        named = np.nonzero(entries["model"] >= 0)[0]
        for bad_row, bad_model in ((named[5], entries["model"][named[2]]), (named[1], fleet.n_models), (named[0], -2)):
            bad = entries.copy()
            bad["model"][bad_row] = bad_model
            with pytest.raises(MmpError) as ei:
                s.janitor_plan(bad, prm)
            assert ei.value.code == _lib.MMP_EINVAL
        with pytest.raises(MmpError):
            s.janitor_plan_raw(entries, prm, _lib.JANITOR_APPLY | _lib.JANITOR_DRY, ne, nc)
        with pytest.raises(MmpError):
            s.janitor_plan(entries, jm.params(self_pod, 0))
        with pytest.raises(MmpError):
            s.janitor_plan(entries, jm.params(fleet.n_pods, now))
        same_registry(s, reg)
        # the map was left clear by all of that: the real run still equals the restatement, with regrown buffers
        got = s.janitor_plan(entries, prm, max_edits=2, max_candidates=1)
        same_outputs(got, jm.Janitor().run(reg, entries, prm, fleet.pods["id_order"]))
        same_registry(s, reg)
    finally:
        s.close()


def test_the_plan_needs_a_committed_snapshot():
    s = Solver(6553, 60_000)
    try:
        with pytest.raises(MmpError) as ei:
            s.janitor_plan(np.zeros(0, dtype=_lib.JANITOR_ENTRY), jm.params(0, 1_700_000_000_000))
        assert ei.value.code == _lib.MMP_ESTATE
    finally:
        s.close()


def test_a_plan_during_place_batches_is_never_seen_half_applied():
    """Batches decided while the rows are rewritten equal the oracle on the registry before or after, per model."""
    fleet, self_pod, reg, s = setup(15, 200, 6000)
    try:
        now = int(fleet.now)
        entries = jm.make_cache(fleet, reg, self_pod, 8, now)
        prm = jm.params(self_pod, now)
        f0 = copy.copy(fleet)
        f0.pods = s.get_pods()
        reg1 = copy.deepcopy(reg)
        want = jm.Janitor().run(reg1, entries, prm, fleet.pods["id_order"])
        f1 = copy.copy(f0)
        f1.models, f1.ent_pod, f1.ent_time = rp.registry_to_arrays(reg1)
        changed = want[1]["model"][want[1]["n_loaded_after"] != f0.models["n_loaded"][want[1]["model"]]]
        assert len(changed) > 10
        rng = np.random.default_rng(5)
        batches = []
        for n in (300, 300, 3000, 9000):
            reqs, extra = wl.fuzz_requests(f0, 50 + n + len(batches), n)
            reqs["model"][::2] = rng.choice(changed, len(reqs["model"][::2]))
            batches.append((reqs, extra, OracleFleet(f0).place(reqs, extra, now, threads=4), OracleFleet(f1).place(reqs, extra, now, threads=4)))
        results, stop, errors = [], threading.Event(), []

        def decide():
            try:
                k = 0
                while not stop.is_set() or k < 8:
                    b = k % len(batches)
                    results.append((b, s.place(batches[b][0], batches[b][1], now)))
                    k += 1
            except Exception as ex:  # noqa: BLE001
                errors.append(ex)

        th = threading.Thread(target=decide)
        th.start()
        while len(results) < 3 and not errors:
            time.sleep(0.001)
        got = s.janitor_plan(entries, prm)
        n_at = len(results)
        while len(results) < n_at + 3 and not errors:
            time.sleep(0.001)
        stop.set()
        th.join()
        assert not errors, errors
        same_outputs(got, want)
        for b, out in results:
            reqs, _, w0, w1 = batches[b]
            eq0 = np.ones(len(reqs), bool)
            eq1 = np.ones(len(reqs), bool)
            for f in ("chosen", "best", "n_candidates", "hash"):
                eq0 &= out[f] == w0[f]
                eq1 &= out[f] == w1[f]
            assert (eq0 | eq1).all(), "a decision equals neither registry"
            for m in np.unique(reqs["model"][~(eq0 & eq1)]):
                rows = reqs["model"] == m
                assert eq0[rows].all() or eq1[rows].all(), f"model {m} was decided against a mixture"
        b, out = results[-1]
        assert_same_decisions(f1, batches[b][0], out, batches[b][3])  # the last batch started after the plan had returned
        same_registry(s, reg1)
    finally:
        s.close()


def test_the_veneer_entry_runs_under_the_mock_jvm(tmp_path):
    from tests import jni_mock as jmock
    from tests.test_jni_veneer import _java_natives
    veneer = jmock.Veneer(jmock.build(tmp_path), _java_natives())
    env = veneer.env
    fleet, self_pod, reg = jm.janitor_fleet(16, 40, 900)
    h = veneer.call("create", 0, fleet.min_space_units, fleet.min_churn_age_ms)
    assert h != 0 and env.pending() is None
    try:
        assert veneer.call("podsLoad", h, jmock.ByteBuffer(fleet.pods), fleet.n_pods) == 0
        assert veneer.call("modelsLoad", h, jmock.ByteBuffer(fleet.models), fleet.n_models, jmock.ByteBuffer(fleet.ent_pod),
                           jmock.ByteBuffer(fleet.ent_time), len(fleet.ent_pod)) == 0
        assert veneer.call("commit", h) == 0
        now = int(fleet.now)
        entries = jm.make_cache(fleet, reg, self_pod, 2, now)
        prm = jm.params(self_pod, now)
        want = jm.Janitor().run(reg, entries, prm, fleet.pods["id_order"])
        n, ne, nc = len(entries), len(want[1]), len(want[2])
        actions = jmock.ByteBuffer(np.zeros(n, np.uint8))
        edits = jmock.ByteBuffer(np.zeros(max(ne, 1), dtype=_lib.JANITOR_EDIT))
        cands = jmock.ByteBuffer(np.zeros(max(nc, 1), dtype=_lib.CACHE_ENTRY))
        rows = jmock.ByteBuffer(np.zeros(max(nc, 1), np.int32))
        info = jmock.ByteBuffer(np.zeros(1, dtype=_lib.JANITOR_INFO))
        rc = veneer.call("janitorPlan", h, jmock.ByteBuffer(entries), n, jmock.ByteBuffer(prm), _lib.JANITOR_APPLY, actions, edits, ne,
                         cands, rows, nc, info)
        assert rc == 0 and env.pending() is None
        same_outputs((actions.arr, edits.arr[:ne], cands.arr[:nc], rows.arr[:nc], info.arr[0]), want)
        # a short buffer is refused before the library is called
        env.clear()
        assert veneer.call("janitorPlan", h, jmock.ByteBuffer(entries), n, jmock.ByteBuffer(prm), 0, jmock.ByteBuffer(np.zeros(2, np.uint8)),
                           edits, ne, cands, rows, nc, info) == -1
        assert env.pending()[0] == "java/lang/IllegalArgumentException" and "actionsOut shorter" in env.pending()[1]
        env.clear()
    finally:
        veneer.call("destroy", h)
