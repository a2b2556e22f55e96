"""What the apply of a registry plan decides, the same for mmp_registry_ops, mmp_janitor_plan and mmp_registry_prune: when the
arena is squeezed, that the host's count of live entries survives the call, and the device span the call reports.

The fleet: M models, each loaded on the same c of P instances.  An applied call that takes one copy out of n of these records
appends the n records' remaining n*(c-1) entries to the arena and leaves their n*c old entries behind as garbage, beside
live = M*c - n entries; the arena is squeezed exactly when garbage > max(live, 65536)."""
import copy

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd import workload as wl
from modelmesh_amd._lib import ROP_DEREGISTER
from modelmesh_amd.solver import Solver
from oracle.bind import OracleFleet
from tests import janitor_model as jm
from tests import registry_ops_model as ro
from tests import registry_prune_model as rp
from tests.registry_ops_model import ModelRecord, Registry, op_row, ops_array
from tests.util import assert_same_decisions

pytestmark = pytest.mark.gpu

SQUEEZE_FLOOR = 1 << 16
GONE = rp.GONE_AFTER_MS
KINDS = ("registry_ops", "janitor_plan", "registry_prune")


class Fleet:
    """The fleet of the module docstring, resident on a solver, beside its sequential model.  held[0] is the instance whose
    copy a call takes out; for the prune it is gone from the table, marked missing by a first run, and due at self.now."""

    def __init__(self, M, c, P, kind, n):
        fleet = wl.fuzz_fleet(1400, pods=P, models=M)
        fleet.pods["flags"] = np.where(fleet.pods["flags"] & _lib.POD_TOMBSTONE, _lib.POD_LIVE, fleet.pods["flags"])
        self.id_order = fleet.pods["id_order"].copy()
        self.held = sorted(range(P), key=lambda p: self.id_order[p])[:c]  # (TreeMap order: the model inserts nothing out of place)
        self.M, self.c, self.now = M, c, int(fleet.now)
        out = self.held[0]
        if kind == "registry_prune":
            fleet.pods["flags"][out] = _lib.POD_TOMBSTONE
            self.now += GONE + 1  # the second run's clock; the first runs at fleet.now
        # the prune examines an entry older than gone-after: the first n records' copy on `out`, and no other entry
        recs = [ModelRecord(int(fleet.models["type"][m]),
                            [(p, self.now - 4 * GONE if p == out and m < n else self.now - 1000 - p) for p in self.held], [],
                            int(fleet.now) - 1_000_000) for m in range(M)]
        self.reg = Registry(recs, self.id_order)
        fleet.models, fleet.ent_pod, fleet.ent_time = ro.registry_to_arrays(recs)
        self.fleet = fleet
        self.s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
        self.s.load_fleet(fleet)
        self.reaper = rp.Reaper()
        if kind == "registry_prune":  # the first run: the mark, no edit
            e, _, info = self.s.prune_registry(self.held[1], int(fleet.now), gone_after_ms=GONE)
            we, _, winfo, _ = self.reaper.run(fleet.pods["flags"], ro.to_prune_records(recs), self.held[1], int(fleet.now), gone_after=GONE)
            assert len(e) == 0 and len(we) == 0 and int(info["n_new_missing"]) == winfo["n_new_missing"] == 1

    def entries(self):
        return sum(len(r.instance_ids) + len(r.load_failed_instance_ids) for r in self.reg.records)

    def cache_rows(self, self_pod, skip):
        """A cache for self_pod with a row in order for every model but those of `skip`: the registry loop removes self_pod's
        copy of exactly the skipped ones."""
        rows = []
        for m, r in enumerate(self.reg.records):
            if m in skip:
                continue
            k = len(rows) + 1
            rows.append((m, 10, self.now - 2_000_000 - 7 * k, r.instance_ids[self_pod], 0, -1, 1, self.now - 7_000_000, 0, 0, 0,
                         _lib.JE_DONE | _lib.JE_STATE_LIVE, 0))
        return np.array(rows, dtype=_lib.JANITOR_ENTRY).reshape(-1)

    def apply(self, kind, pod, models):
        """One applied call of `kind` on both sides that takes `pod`'s copy out of `models` (the prune: the due copies)."""
        s, M = self.s, self.M
        if kind == "registry_ops":
            ops = ops_array([op_row(m, pod, ROP_DEREGISTER, last_used=0) for m in models])
            st, ed, info = s.registry_ops(ops, self.now, max_edits=M)
            wst, wed, winfo = self.reg.run(ops, self.now)
            assert np.array_equal(st, wst) and np.array_equal(ed, wed)
        else:
            recs = ro.to_prune_records(self.reg.records)
            if kind == "janitor_plan":
                rows, prm = self.cache_rows(pod, set(models)), jm.params(pod, self.now)
                got = s.janitor_plan(rows, prm, max_edits=M, max_candidates=M)
                want = jm.Janitor().run(recs, rows, prm, self.id_order)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
                wed = want[1]
            else:
                e, rm, info = s.prune_registry(self.held[1], self.now, gone_after_ms=GONE, max_edits=M, max_removed=M * self.c)
                wed, wrm, winfo, _ = self.reaper.run(self.fleet.pods["flags"], recs, self.held[1], self.now, gone_after=GONE)
                assert np.array_equal(e, wed) and np.array_equal(rm, wrm) and s.missing_instances() == self.reaper.missings
            for m in wed["model"]:  # (the two restatements edit their own record type)
                old, r = self.reg.records[m], recs[m]
                self.reg.records[m] = ModelRecord(r.type, r.loaded, r.failed, r.last_used, old.last_unload_time)
        assert list(wed["model"]) == list(models)

    def same_registry(self):
        got = rp.compact(*self.s.get_models())
        for g, w in zip(got, ro.registry_to_arrays(self.reg.records)):
            assert np.array_equal(g, w)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,squeezed", [(1800, True), (1000, False)], ids=["over", "under"])
def test_the_arena_is_squeezed_exactly_over_the_threshold(kind, n, squeezed):
    M, c, P = 1800, 40, 48
    f = Fleet(M, c, P, kind, n)
    s = f.s
    try:
        assert f.entries() == M * c == len(s.get_models()[1])
        before = copy.deepcopy(f.reg.records[:n])
        f.apply(kind, f.held[0], range(n))
        # the arithmetic of the module docstring, from the model
        garbage = sum(len(r.instance_ids) for r in before)
        live, rebuilt = f.entries(), sum(len(r.instance_ids) for r in f.reg.records[:n])
        assert (garbage, live, rebuilt) == (n * c, M * c - n, n * (c - 1))
        assert (garbage > max(live, SQUEEZE_FLOOR)) == squeezed
        arena = len(s.get_models()[1])
        print(f"{kind} n={n}: garbage {garbage} live {live} arena {arena}")
        assert arena == (live if squeezed else M * c + rebuilt)
        f.same_registry()
        # a second applied call of another kind: the host's count of live entries survived the first
        second = KINDS[(KINDS.index(kind) + 1) % 2]  # ops -> janitor, janitor and prune -> ops
        f.apply(second, f.held[2], range(64))
        f.same_registry()
        # decisions on the committed registry
        s.commit()
        f2 = copy.copy(f.fleet)
        f2.pods = s.get_pods()
        f2.models, f2.ent_pod, f2.ent_time = ro.registry_to_arrays(f.reg.records)
        reqs, extra = wl.fuzz_requests(f2, 41, 1500)
        want = OracleFleet(f2).place(reqs, extra, f2.now, threads=4)
        assert_same_decisions(f2, reqs, s.place(reqs, extra, f2.now), want)
    finally:
        s.close()


def test_an_applied_plan_reports_its_device_span_only_when_profiled():
    for kind in KINDS:
        f = Fleet(96, 6, 8, kind, 70)
        s = f.s
        try:
            s.profile(True)
            assert s.last_kernel_ms() < 0
            f.apply(kind, f.held[0], range(70))
            ms = s.last_kernel_ms()
            print(f"{kind}: applied call, device span {ms * 1000:.1f} us")
            assert ms > 0
            f.same_registry()
        finally:
            s.close()
        f = Fleet(96, 6, 8, kind, 70)
        s = f.s
        try:
            s.profile(True)
            s.profile(False)
            f.apply(kind, f.held[0], range(70))
            assert s.last_kernel_ms() < 0
            f.same_registry()
        finally:
            s.close()
