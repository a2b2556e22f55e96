"""mmp_pods_retire: instance rows leave the index space; the staged table, the labels, the type rows and the id store are compacted
on the host, the registry's entries, the `missings` marks and the instance-id table on the device, and the call ends in a commit.
The oracle is tests/pod_retire_model.py over tests/pod_events_model.py, and a second context LOADED with exactly the survivors:
after a retire everything the first context answers equals what the second one answers.  A fresh load interns replica sets by
first appearance among the survivors, so the second context is given the rows of the model, whose replica_set numbers are the
pre-retire ones.  At the wavefront, workgroup, table-capacity and type-word edges, with events, registry plans and delta commits
behind the call, through the intended loop (deletion, prune, retire), every refusal with nothing changed, twice byte-identical,
beside a census reader and a placing thread.  All comparisons exact."""
import copy
import threading

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd import workload as wl
from modelmesh_amd.solver import MmpError, Solver, bitmap_from_bool
from tests import janitor_model as jm
from tests import registry_census_model as rcm
from tests import registry_prune_model as rp
from tests import wire
from tests.pod_events_model import PodEventsModel
from tests.pod_retire_model import PodRetireState, retire
from tests.registry_ops_model import op_row, ops_array
from tests.util import assert_same_decisions

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 2, 15, 16, 17, 63, 64, 65, 128, 129, 300)
MODELS = {0: 3, 1: 0, 2: 7, 15: 40, 16: 64, 17: 65, 63: 200, 64: 256, 65: 257, 128: 300, 129: 300, 300: 300}
NAMES = ["gpu", "l0", "l1", "l2", "l3", "spare"]
MALFORMED = "{"  # an event nobody applies: its pod_idx is the resolution of its key, the row stays
GONE_AFTER = 600_000


def bit_rows(words, n_types, p):
    """uint64 [T][W] -> T lists of p bits"""
    if not n_types:
        return []
    if p == 0:
        return [[] for _ in range(n_types)]
    by = np.unpackbits(np.ascontiguousarray(words, dtype=np.uint64).view(np.uint8), bitorder="little").reshape(n_types, -1)
    return [[int(b) for b in row[:p]] for row in by]


def word_rows(rows, p):
    """T lists of p bits -> uint64 [T][max(W, 1)]"""
    if p == 0:
        return np.zeros((len(rows), 1), np.uint64)
    return bitmap_from_bool(np.array(rows, bool).reshape(len(rows), p))


class Rig:
    """A fuzz fleet under instance ids, its state as the model holds it (PodRetireState), and contexts loaded from such a state."""

    def __init__(self, seed, pods, models, ids=True, from_labels=False):
        self.rng = rng = np.random.default_rng(7000 + seed)
        f = wl.fuzz_fleet(seed, pods=max(pods, 1), models=models)
        if pods == 0:
            f.pods = f.pods[:0]
            f.models["n_loaded"] = f.models["n_failed"] = f.models["ent_off"] = 0
            f.ent_pod, f.ent_time = f.ent_pod[:0], f.ent_time[:0]
            f.replaced_rs = f.replaced_rs[:0]
        self.fleet, self.now = f, int(f.now)
        self.from_labels = from_labels
        self.type_names = ["NLCLASSIFIER"] + ["type-%d" % t for t in range(1, max(f.n_types, 1) + 1)]
        st = self.state = PodRetireState()
        if ids:
            names = wire.make_ids(rng, pods)
            wire.adopt_ids(f, names)
            io, rs = st.pods.load(names)
            assert np.array_equal(io, f.pods["id_order"]) and np.array_equal(rs, f.pods["replica_set"])
        st.pods.rows = f.pods.copy()
        st.label_words = [int(w) for w in rng.integers(0, 64, pods)]
        st.label_counts = [bin(w).count("1") + int(rng.integers(0, 2)) for w in st.label_words]
        if from_labels:
            t = max(f.n_types, 2)
            self.required = rng.choice([0, 1, 2, 6, 8], t).astype(np.uint64)
            self.preferred = rng.choice([0, 0, 4, 16], t).astype(np.uint64)
            self.n_types = t + 1
        else:
            self.n_types = f.n_types
            self.has_allowed, self.has_prefer = f.has_allowed, f.has_prefer
            st.allowed, st.prefer = bit_rows(f.allowed, f.n_types, pods), bit_rows(f.prefer, f.n_types, pods)
        self.meta = [(int(m["type"]), int(m["last_used"])) for m in f.models]
        for m in f.models:
            o, k, n = int(m["ent_off"]), int(m["n_loaded"]), int(m["n_failed"])
            ent = [[int(p), int(t)] for p, t in zip(f.ent_pod[o:o + k + n], f.ent_time[o:o + k + n])]
            st.records.append((ent[:k], ent[k:]))

    def fresh(self):
        """a copy of the start state"""
        return copy.deepcopy(self.state)

    def solver(self):
        return Solver(self.fleet.min_space_units, self.fleet.min_churn_age_ms)

    def arrays(self, st):
        rows = np.zeros(len(st.records), dtype=_lib.MODEL_ROW)
        ep, et = [], []
        for i, (loaded, failed) in enumerate(st.records):
            rows[i] = (self.meta[i][0], len(ep), len(loaded), len(failed), self.meta[i][1])
            for p, t in loaded + failed:
                ep.append(p)
                et.append(t)
        return rows, np.array(ep, np.int32), np.array(et, np.int64)

    def load(self, s, st, commit=True):
        """The state into a context, as a host loads it."""
        m, p = st.pods, st.pods.n_pods
        if m.ids is not None:
            s.load_pod_ids(m.ids)
            s.load_type_names(self.type_names, 0)
        s.load_pods(m.rows)
        s.label_names_load(NAMES)
        if p:
            s.pod_labels_set(np.arange(p), np.array(st.label_words, np.uint64), np.array(st.label_counts, np.int32))
        types = self.load_types(s, st)
        s.load_replaced_rs(self.fleet.replaced_rs)
        s.load_models(*self.arrays(st))
        if commit:
            s.commit()
        return types

    def load_types(self, s, st):
        p = st.pods.n_pods
        if self.from_labels:
            return s.types_from_pod_labels(self.required, self.preferred)
        if self.n_types:
            s.load_types(self.n_types, word_rows(st.allowed, p), word_rows(st.prefer, p), self.has_allowed, self.has_prefer)
        else:
            s.load_types(0)
        return None

    def joined(self, ctxs, st, n):
        """n instances joined: the type rows cover them again (any instance may host, none is preferred), on every side"""
        for r in st.allowed:
            r.extend([1] * n)
        for r in st.prefer:
            r.extend([0] * n)
        for ctx in ctxs:
            self.load_types(ctx, st)

    def mark(self, s, st):
        """One reaper pass that changes no record: the instances it finds missing get their marks, the model copies them."""
        s.prune_registry(0, self.now, apply=False)
        since = s.missing_instances()
        st.missing = [since.get(p, 0) for p in range(s.missing_slots())]

    def fleet_of(self, st):
        f = copy.copy(self.fleet)
        f.pods = st.pods.rows
        f.models, f.ent_pod, f.ent_time = self.arrays(st)
        return f


def retire_sets(p0, rng):
    """(name, pods): none, all, first, last, every other, a run across 60-70, a random third out of order and with repeats"""
    third = [int(p) for p in rng.choice(p0, p0 // 3, replace=False)] if p0 else []
    third = third + third[:2]
    return [("none", []), ("all", list(range(p0))), ("first", [0][:p0]), ("last", [p0 - 1] if p0 else []),
            ("every other", list(range(0, p0, 2))), ("60-70", [p for p in range(60, 71) if p < p0]), ("a third", third)]


def dump(s, rig, st, keys=None, committed=True, decide=True):
    """Everything a context answers, as named lists of arrays.  st: the state the context is expected to hold (sizes the requests)."""
    f, p, m, now = rig.fleet_of(st), st.pods.n_pods, len(st.records), rig.now
    out = {"pods": [s.get_pods()], "labels": list(s.pod_labels_get()), "models": list(s.get_models()), "n": [np.array([s.n_pods, s.n_models])]}
    if keys is not None:
        status, idx, _, n_app = s.pods_events_json(keys, [MALFORMED] * len(keys), append=False)
        out["resolve"] = [status, idx, np.array([n_app])]
    stats, pl, pf, ts = s.registry_census()
    out["census"] = [np.array([int(stats[k]) for k in rcm.SCALARS]), stats["copies_hist"], pl, pf] + \
                    [ts[k] for k in ("n_models", "n_loaded", "n_failed", "n_entries_loaded")]
    rows, nm, ne = s.registry_unresolved()
    out["unresolved"] = [rows, np.array([nm, ne])]
    out["missing"] = [np.array(sorted(s.missing_instances().items()), np.int64).reshape(-1, 2), np.array([s.missing_slots()])]
    if not committed:
        return out
    if m:
        reqs = np.zeros(m, _lib.STATUS_REQ)
        reqs["model"], reqs["fail_pod"] = np.arange(m), -1
        out["status"] = list(s.models_status(reqs, now))
    parts, pstats = s.partitions()
    out["order"] = [s.order(), np.array([s.stats()]), parts] + [np.array([x[0]]) for x in pstats] + \
                   [np.array([x[1] & (2**63 - 1) for x in pstats], np.int64), np.array([s.type_stats(t) for t in range(rig.n_types)])]
    if decide and p and m:
        rng = np.random.default_rng(p * 1000 + m)
        reqs, extra = wl.fuzz_requests(f, 1, 300)
        place = s.place(reqs, extra, now)
        sr = np.zeros(200, dtype=_lib.SERVE_REQ)
        sr["model"], sr["self_pod"], sr["flags"] = rng.integers(0, m, 200), rng.integers(-1, p, 200), rng.integers(0, 4, 200)
        sr["assume_completed_ms"], sr["last_invoke_time"] = 3000, now - 10
        in_use, last_used = rng.integers(0, 3, p).astype(np.int32), (now - rng.choice([0, 5, 100, 10_000], p)).astype(np.int64)
        serve = s.serve(sr, in_use, last_used, np.zeros(0, np.int32), np.zeros(0, np.int64), now)
        g = np.zeros(100, dtype=_lib.GATE_REQ)
        pr = reqs[:100].copy()
        pr["self_pod"] = np.maximum(pr["self_pod"], 0)
        g["model"], g["self_pod"], g["last_used_time"] = pr["model"], pr["self_pod"], pr["last_used"]
        g["cache_capacity"], g["cache_weighted_size"], g["cache_oldest_time"] = 1_000_000, 400_000, now - 5_000_000
        g["size_hint"], g["loaded_time"], g["load_timeout_ms"], g["weight_predict_cutoff"] = 64, -1, 240_000, 20
        for k in ("fresh_lru", "fresh_capacity", "fresh_used", "fresh_count", "fresh_rpm"):
            g[k] = pr[k]
        g["fresh_loading_threads"] = 8
        none = np.zeros(0, np.int32)
        gate, miss = s.miss(g, pr, none, np.zeros(0, np.int64), none, extra, now)
        out["decisions"] = [place, serve, gate, miss, reqs]
    return out


def same(a, b, what, skip=()):
    assert a.keys() == b.keys(), what
    for k in a:
        if k in skip:
            continue
        if k == "decisions" and not np.array_equal(a[k][0], b[k][0]):
            assert_same_decisions(None, a[k][4], a[k][0], b[k][0])
        assert len(a[k]) == len(b[k]), (what, k)
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y), (what, k, i)


def resolve_keys(old_ids):
    return None if old_ids is None else list(old_ids) + [b"never-%d" % i for i in range(3)] + [i + b"x" for i in old_ids[:2]]


def assert_equals_a_load(rig, s, ref, st, old_ids, what, committed=True, decide=True):
    """Context s after a retire against the model's state st and against ref, a context loaded with st."""
    rig.load(ref, st, commit=committed)
    keys = resolve_keys(old_ids)
    got, want = dump(s, rig, st, keys, committed, decide), dump(ref, rig, st, keys, committed, decide)
    same(got, want, what, skip=("missing",))
    # ... and against the model itself: rows, labels, records (offsets and all: the arena is not squeezed), resolutions, marks
    m = st.pods
    assert np.array_equal(got["pods"][0], m.rows), what
    assert list(got["labels"][0]) == st.label_words and list(got["labels"][1]) == st.label_counts, what
    for g, w in zip(got["models"], rig.arrays(st)):
        assert np.array_equal(g, w), what
    if keys is not None:
        assert [int(i) for i in got["resolve"][1]] == [m.index.get(k, -1) for k in keys], what
        assert [int(x) for x in got["resolve"][0]] == [1 if k in m.index else 2 for k in keys], what
    if committed:
        assert {int(p): int(v) for p, v in got["missing"][0]} == {p: v for p, v in enumerate(st.missing) if v}, what
        assert int(got["missing"][1][0]) == len(st.missing), what
    assert np.array_equal(s._live, ref._live), what  # the wrapper's own mirror shrank with the table
    return got


def unresolved_of(s):
    return int(s.registry_census()[0]["n_entries_unresolved"])


def retire_both(rig, s, st, pods, what, **guards):
    """The same retire on the context and on the model: remap, count, and the census's unresolved entries rise by the count."""
    before = unresolved_of(s)
    want, count = retire(st, pods, **guards)
    got, n = s.pods_retire(pods, **guards)
    assert got.dtype == np.int32 and np.array_equal(got, want) and n == count, (what, n, count)
    assert s.n_pods == st.pods.n_pods and unresolved_of(s) == before + count == st.n_unresolved(), what
    return want, count


@pytest.mark.parametrize("p0", SIZES)
def test_retire_equals_a_load_of_the_survivors(p0):
    rig = Rig(p0, p0, MODELS[p0])
    s, ref = rig.solver(), rig.solver()
    try:
        for name, pods in retire_sets(p0, rig.rng):
            what, st = (p0, name), rig.fresh()
            rig.load(s, st)
            rig.mark(s, st)
            old_ids = list(st.pods.ids)
            remap, _ = retire_both(rig, s, st, pods, what)
            got = assert_equals_a_load(rig, s, ref, st, old_ids, what)
            assert [int(i) for i in got["resolve"][1][:p0]] == [int(r) for r in remap], what  # every old id: its new index, or unknown
    finally:
        s.close()
        ref.close()


@pytest.mark.parametrize("p0", (0, 17))
def test_without_a_published_snapshot_only_the_inputs_are_compacted(p0):
    rig = Rig(50 + p0, p0, MODELS[p0])
    for name, pods in [("none", []), ("all", list(range(p0))), ("every other", list(range(0, p0, 2)))]:
        s, ref = rig.solver(), rig.solver()
        try:
            st = rig.fresh()
            rig.load(s, st, commit=False)
            old_ids = list(st.pods.ids)
            retire_both(rig, s, st, pods, (p0, name))
            with pytest.raises(MmpError):
                s.order()  # no snapshot was made
            assert_equals_a_load(rig, s, ref, st, old_ids, (p0, name), committed=False)
            s.commit()  # and the inputs commit like the loaded ones
            ref.commit()
            same(dump(s, rig, st, resolve_keys(old_ids)), dump(ref, rig, st, resolve_keys(old_ids)), (p0, name, "committed"), skip=("missing",))
        finally:
            s.close()
            ref.close()


def test_table_capacity_edges():
    """33 ids (128 slots) retired down to 8 (16 slots); 9 more ids, one of them a retired one, across the edge of the shrunken table
    (17 ids: 64 slots); a second retire behind that."""
    rig = Rig(33, 33, 120)
    s, ref = rig.solver(), rig.solver()
    try:
        st = rig.fresh()
        rig.load(s, st)
        rig.mark(s, st)
        all_ids = list(st.pods.ids)
        gone = [p for p in range(33) if p % 4 != 1][:25]
        retire_both(rig, s, st, gone, "33 -> 8")
        assert st.pods.n_pods == 8
        assert_equals_a_load(rig, s, ref, st, all_ids, "33 -> 8")
        fresh = [all_ids[gone[3]]] + [b"rsjoin-%05d" % i for i in range(8)]
        values = wire.pod_values(rig.fleet, rig.rng, np.zeros(33, np.int64))[:9]
        want, got = st.pods.events(fresh, values), s.pods_events_json(fresh, values)
        for g, w in zip(got[:3], want[:3]):
            assert np.array_equal(g, w)
        assert got[3] == want[3] == 9 and list(got[1]) == list(range(8, 17))
        st.label_words, st.label_counts = [int(w) for w in s.pod_labels_get()[0]], [int(c) for c in s.pod_labels_get()[1]]
        assert np.array_equal(s.get_pods(), st.pods.rows)  # the retired id that came back keeps its replica-set number
        all_ids += fresh[1:]
        keys = resolve_keys(all_ids)
        assert [int(i) for i in s.pods_events_json(keys, [MALFORMED] * len(keys), append=False)[1]] == [st.pods.index.get(k, -1) for k in keys]
        rig.joined([s], st, 9)  # the type rows no longer cover the table, as after any join: loaded again
        s.commit()
        st.missing = [s.missing_instances().get(p, 0) for p in range(s.missing_slots())]
        retire_both(rig, s, st, [16, 0, 9, 9, 3], "17 -> 13")
        assert_equals_a_load(rig, s, ref, st, all_ids, "17 -> 13", decide=False)
    finally:
        s.close()
        ref.close()


@pytest.mark.parametrize("p0,gone", [(65, [64]), (65, [0]), (64, [63]), (64, [20])])
@pytest.mark.parametrize("from_labels", [False, True])
def test_type_word_edge(p0, gone, from_labels):
    """65 -> 64 and 64 -> 63 survivors: the type rows lose a word, or keep theirs with the bits moved down.  No reload in the first
    context, whichever call made its sets."""
    rig = Rig(80 + p0, p0, 200, from_labels=from_labels)
    assert rig.n_types > 0
    s, ref = rig.solver(), rig.solver()
    try:
        st = rig.fresh()
        rig.load(s, st)
        rig.mark(s, st)
        old_ids = list(st.pods.ids)
        retire_both(rig, s, st, gone, (p0, gone))
        got = assert_equals_a_load(rig, s, ref, st, old_ids, (p0, gone))
        if from_labels:  # the sets built anew over the compacted label words are the ones the retire left
            mine, theirs = s.types_from_pod_labels(rig.required, rig.preferred), ref.types_from_pod_labels(rig.required, rig.preferred)
            for a, b in zip(mine, theirs):
                assert np.array_equal(a, b)
            s.commit()
            ref.commit()
            same(dump(s, rig, st, resolve_keys(old_ids)), got, (p0, gone, "rebuilt"))
    finally:
        s.close()
        ref.close()


def test_records_naming_retired_instances():
    """A record of 64 copies, half of them on retired instances; a record with an entry that was unresolved already and one beyond
    the table; 2 000 models whose only copy is on one retired instance."""
    rig = Rig(91, 300, 2000)
    st0 = rig.state
    k = 7
    for i in range(2000):
        st0.records[i] = ([[k, 1000 + i]], [])
    st0.records[5] = ([[p, 500 + p] for p in range(0, 128, 2)], [])  # 64 copies on even instances
    st0.records[6] = ([[-1, 1], [k, 2], [300, 3], [9, 4]], [[k + 1, 5]])
    st0.records[8] = ([], [[k, 6]])
    s, ref = rig.solver(), rig.solver()
    try:
        st = rig.fresh()
        rig.load(s, st)
        rig.mark(s, st)
        old_ids = list(st.pods.ids)
        gone = [k] + [p for p in range(0, 128, 4)]
        _, count = retire_both(rig, s, st, gone, "records")
        assert count == (2000 - 3) + 32 + 2 + 1  # the single copies, half of the 64, record 6 (loaded on 7, failed on 8), record 8
        assert_equals_a_load(rig, s, ref, st, old_ids, "records")
    finally:
        s.close()
        ref.close()


def test_arena_garbage_neither_counts_nor_trips_the_guard():
    rig = Rig(92, 40, 100)
    s, ref = rig.solver(), rig.solver()
    try:
        st, k = rig.fresh(), 11
        st.records[0], st.records[1] = ([[k, 50], [3, 51]], []), ([], [[k, 52]])
        rig.load(s, st)
        rig.mark(s, st)
        named = [i for i, (a, b) in enumerate(st.records) if any(e[0] == k for e in a + b)]
        with pytest.raises(MmpError) as e:
            s.pods_retire([k], unreferenced=True)
        assert e.value.code == _lib.MMP_EINVAL and "instance %d " % k in str(e.value)
        # the records are rewritten without instance k: their old entries stay behind in the arena, referenced by no row
        for i in named:
            st.records[i] = ([e for e in st.records[i][0] if e[0] != k], [e for e in st.records[i][1] if e[0] != k])
        sub = copy.copy(st)
        sub.records = [st.records[i] for i in named]
        meta, rig.meta = rig.meta, [rig.meta[i] for i in named]
        rows, ep, et = rig.arrays(sub)
        rig.meta = meta
        s.upsert_models(np.array(named, np.int32), rows, ep, et)
        arena = s.get_models()[1]
        assert len(arena) > len(rig.arrays(st)[1]) and k in arena  # garbage, naming k
        _, count = retire_both(rig, s, st, [k], "garbage", unreferenced=True)
        assert count == 0
        rig.load(ref, st)
        keys = resolve_keys(list(rig.state.pods.ids))
        mine, theirs = dump(s, rig, st, keys), dump(ref, rig, st, keys)
        mine["models"], theirs["models"] = list(rp.compact(*mine["models"])), list(rp.compact(*theirs["models"]))
        same(mine, theirs, "garbage", skip=("missing",))
    finally:
        s.close()
        ref.close()


@pytest.mark.parametrize("pods,models", [(8, 300), (300, 2000)])
def test_the_intended_loop(pods, models):
    """Deleted events tombstone instances; a retire under both guards is refused while records name them; the prune past
    gone_after_ms removes their registrations; the same retire then succeeds with a count of 0; a prune afterwards finds what it
    finds in a context loaded with the survivors."""
    rig = Rig(93 + pods, pods, models)
    rig.fleet.pods["flags"] = _lib.POD_LIVE  # everybody is here, so only the deleted ones go missing
    rig.state.pods.rows["flags"] = _lib.POD_LIVE
    s, ref = rig.solver(), rig.solver()
    try:
        st, now = rig.fresh(), rig.now
        rig.load(s, st)
        named = sorted({e[0] for a, b in st.records for e in a + b} - {0})  # (instance 0 is the reaper's own)
        gone = sorted(int(p) for p in rig.rng.choice(named, max(len(named) // 4, 2), replace=False))
        gone_ids = [st.pods.ids[p] for p in gone]
        st.pods.events(gone_ids, [""] * len(gone), deleted=[1] * len(gone))
        status, idx, _, _ = s.pods_events_json(gone_ids, [""] * len(gone), deleted=[1] * len(gone))
        assert not status.any() and list(idx) == gone
        s.commit()
        t1 = now + 1000
        s.prune_registry(0, t1)  # first seen missing: marked, nothing removed yet
        assert sorted(s.missing_instances()) == gone
        before = dump(s, rig, st, resolve_keys(st.pods.ids))
        with pytest.raises(MmpError) as e:
            s.pods_retire(gone[::-1], gone_only=True, unreferenced=True)
        assert e.value.code == _lib.MMP_EINVAL and "instance %d " % gone[0] in str(e.value)
        same(dump(s, rig, st, resolve_keys(st.pods.ids)), before, "refused")
        edits, removed, info = s.prune_registry(0, t1 + GONE_AFTER + 1)
        assert info["n_removed"] > 0 and set(removed["pod"]) == set(gone)
        for a, b in st.records:
            a[:] = [x for x in a if x[0] not in gone]
            b[:] = [x for x in b if x[0] not in gone]
        rows, ep, et = s.get_models()
        rig.meta = [(int(r["type"]), int(r["last_used"])) for r in rows]  # (the prune repairs last_used of records it empties)
        st.missing = [s.missing_instances().get(p, 0) for p in range(s.missing_slots())]
        old_ids = list(st.pods.ids)
        _, count = retire_both(rig, s, st, gone[::-1], "loop", gone_only=True, unreferenced=True)
        assert count == 0 and not s.missing_instances()
        rig.load(ref, st)
        keys = resolve_keys(old_ids)
        mine, theirs = dump(s, rig, st, keys), dump(ref, rig, st, keys)
        mine["models"], theirs["models"] = list(rp.compact(*mine["models"])), list(rp.compact(*theirs["models"]))
        same(mine, theirs, "loop", skip=("missing",))  # (the second context has not run a reaper pass yet: no slots)
        # a survivor leaves next: both contexts mark it at the same pass and prune it at the same later one
        left = st.pods.ids[min(e[0] for a, b in st.records for e in a + b if e[0] > 0)]
        for ctx in (s, ref):
            ctx.pods_events_json([left], [""], deleted=[1])
            ctx.commit()
        for t in (t1 + 2 * GONE_AFTER, t1 + 4 * GONE_AFTER):
            for a, b in zip(s.prune_registry(0, t), ref.prune_registry(0, t)):
                assert np.array_equal(a, b), t
            assert s.missing_instances() == ref.missing_instances() and s.missing_slots() == ref.missing_slots()
    finally:
        s.close()
        ref.close()


def test_gone_only_refuses_an_instance_that_came_back():
    rig = Rig(94, 20, 60)
    s = rig.solver()
    try:
        st = rig.fresh()
        rig.load(s, st)
        ids = [st.pods.ids[p] for p in (3, 9, 12)]
        value = wire.pod_values(rig.fleet, rig.rng, np.zeros(20, np.int64))[0]
        s.pods_events_json(ids, [""] * 3, deleted=[1, 1, 1])
        s.pods_events_json([ids[1]], [value])  # 9 is back
        s.commit()
        before = dump(s, rig, st, resolve_keys(st.pods.ids), decide=False)
        with pytest.raises(MmpError) as e:
            s.pods_retire([12, 9, 3], gone_only=True)
        assert e.value.code == _lib.MMP_EINVAL and "instance 9 " in str(e.value)
        same(dump(s, rig, st, resolve_keys(st.pods.ids), decide=False), before, "refused")
        remap, _ = s.pods_retire([12, 3], gone_only=True)
        assert int(remap[9]) == 8 and s.n_pods == 18
    finally:
        s.close()


def test_life_goes_on_behind_the_call():
    """Events by key, registry events naming surviving and retired ids, registry_ops, a janitor plan and a delta commit give on the
    compacted context what they give on the loaded one."""
    rig = Rig(95, 40, 200)
    s, ref = rig.solver(), rig.solver()
    try:
        st, now = rig.fresh(), rig.now
        rig.load(s, st)
        rig.mark(s, st)
        old_ids = list(st.pods.ids)
        # every survivor's id prefix is first seen in the same order before and after: the second context interns alike
        gone = [p for p in range(10, 40, 3)]
        retire_both(rig, s, st, gone, "behind")
        probe = PodEventsModel()
        assert np.array_equal(probe.load(st.pods.ids)[1], st.pods.rows["replica_set"])
        assert_equals_a_load(rig, s, ref, st, old_ids, "behind")
        p1 = st.pods.n_pods
        # instance events by key: updates of survivors, a deletion, a retired id and a new one joining
        values = wire.pod_values(rig.fleet, rig.rng, np.arange(40))
        ev_keys = [st.pods.ids[2], st.pods.ids[p1 - 1], old_ids[gone[0]], b"rsnewx-00001", st.pods.ids[5]]
        dele = np.array([0, 0, 0, 0, 1], np.uint8)
        want = st.pods.events(ev_keys, values[:5], dele)
        for ctx in (s, ref):
            got = ctx.pods_events_json(ev_keys, values[:5], dele)
            for g, w in zip(got[:3], want[:3]):
                assert np.array_equal(g, w)
            assert got[3] == want[3] == 2
        assert np.array_equal(s.get_pods(), st.pods.rows)  # (the id that came back keeps its replica-set number)
        rig.joined([s, ref], st, 2)  # (a join outgrows the type rows, as ever)
        for ctx in (s, ref):
            ctx.commit()
        st.label_words, st.label_counts = [int(w) for w in s.pod_labels_get()[0]], [int(c) for c in s.pod_labels_get()[1]]
        # registry events by key: copies on a surviving, on a retired (unknown: -1) and on the rejoined id
        for ctx in (s, ref):
            ctx.model_ids_load([b"model-%d" % i for i in range(200)])
        def jrec(pairs):
            return '{"instanceIds":{%s},"lu":%d}' % (",".join('"%s":%d' % (k.decode(), t) for k, t in pairs), now - 5)
        mvals = [jrec([(st.pods.ids[1], now - 50), (old_ids[gone[1]], now - 40)]), jrec([(old_ids[gone[0]], now - 30)]), jrec([(b"rsnewx-00001", now - 20)])]
        outs = [ctx.models_events_json([b"model-3", b"model-4", b"model-new"], mvals) for ctx in (s, ref)]
        for a, b in zip(*outs):
            assert np.array_equal(a, b)
        for ctx in (s, ref):
            ctx.commit()
        rows, ep, et = s.get_models()
        o = int(rows[3]["ent_off"])
        assert sorted(ep[o:o + 2]) == [-1, 1] and int(ep[int(rows[4]["ent_off"])]) == st.pods.index[old_ids[gone[0]]] == p1
        for a, b in zip(rp.compact(*s.get_models()), rp.compact(*ref.get_models())):
            assert np.array_equal(a, b)
        m = s.n_models
        ops = ops_array([op_row(i, int(rig.rng.integers(0, s.n_pods)), i % 4, last_used=now - i, load_time=now - 10, load_complete_time=now)
                         for i in range(0, m, 3)])
        for a, b in zip(s.registry_ops(ops, now), ref.registry_ops(ops, now)):
            assert np.array_equal(a, b)
        ent = np.zeros(30, dtype=_lib.JANITOR_ENTRY)
        ent["model"], ent["weight"], ent["last_used"] = np.arange(0, 60, 2), 10, now - jm.OLD_MS - 7 * np.arange(30)
        ent["load_timestamp"], ent["last_unload_attempt_time"], ent["flags"] = now - 3_000_000, -1, _lib.JE_DONE | _lib.JE_STATE_LIVE
        for a, b in zip(s.janitor_plan(ent, jm.params(2, now)), ref.janitor_plan(ent, jm.params(2, now))):
            assert np.array_equal(a, b)
        for a, b in zip(rp.compact(*s.get_models()), rp.compact(*ref.get_models())):
            assert np.array_equal(a, b)
        # a delta commit: the from-scratch commit of the retire left a snapshot a few changed rows can be inserted into
        row = s.get_pods()[[4]].copy()
        row["lru_time"] -= 12_345
        deltas = []
        for ctx in (s, ref):
            n0 = ctx.delta_commits()
            ctx.upsert_pods(np.array([4], np.int32), row)
            ctx.commit()
            deltas.append(ctx.delta_commits() - n0)
            assert np.array_equal(ctx.order(), s.order())
        assert deltas[0] == deltas[1]
        reqs, extra = wl.fuzz_requests(rig.fleet_of(st), 5, 300)
        reqs["model"] %= 200
        assert_same_decisions(None, reqs, s.place(reqs, extra, now), ref.place(reqs, extra, now))
    finally:
        s.close()
        ref.close()


def test_a_delta_commit_follows_the_from_scratch_one():
    rig = Rig(96, 64, 50)
    rig.state.pods.rows["flags"] = _lib.POD_LIVE
    rig.state.pods.rows["version"] = 7  # one version: the order is total, so a few changed rows are inserted
    s = rig.solver()
    try:
        st = rig.fresh()
        rig.load(s, st)
        n0 = s.delta_commits()
        s.pods_retire([1, 2, 3])
        assert s.delta_commits() == n0  # the retire's commit ranks from scratch
        row = s.get_pods()[[10]].copy()
        row["lru_time"] -= 999
        s.upsert_pods(np.array([10], np.int32), row)
        s.commit()
        assert s.delta_commits() == n0 + 1
    finally:
        s.close()


def test_without_an_id_table():
    """load_pods hosts: rows, labels, types, marks, registry and decisions; the id_order column stays as the host supplied it."""
    rig = Rig(97, 70, 150, ids=False)
    for name, pods in [("every other", list(range(0, 70, 2))), ("60-70", list(range(60, 70))), ("a few", [69, 0, 33, 33])]:
        s, ref = rig.solver(), rig.solver()
        try:
            st = rig.fresh()
            rig.load(s, st)
            rig.mark(s, st)
            io = st.pods.rows["id_order"].copy()
            remap, _ = retire_both(rig, s, st, pods, name)
            assert np.array_equal(st.pods.rows["id_order"], io[remap >= 0])
            assert_equals_a_load(rig, s, ref, st, None, name)
        finally:
            s.close()
            ref.close()


def test_refusals_change_nothing():
    rig = Rig(98, 64, 100)
    pods = rig.state.pods.rows
    pods["flags"], pods["version"], pods["used"] = _lib.POD_LIVE, 1, 0
    s = rig.solver()
    try:
        st = rig.fresh()
        rig.load(s, st)
        rig.mark(s, st)
        keys = resolve_keys(st.pods.ids)
        before = dump(s, rig, st, keys)
        C = _lib.C
        remap = np.zeros(64, np.int32)

        def raw(pods, n, flags, remap_out, max_pods):
            return s.lib.mmp_pods_retire(s.h, pods, n, flags, remap_out, max_pods, None, None)

        two = np.array([1, 2], np.int32)
        assert raw(None, 2, 0, None, 0) == _lib.MMP_EINVAL  # NULL pods with n > 0
        assert raw(_lib.ptr(two), -1, 0, None, 0) == _lib.MMP_EINVAL
        assert raw(_lib.ptr(two), 2, 4, None, 0) == _lib.MMP_EINVAL  # an unknown flag bit
        assert raw(_lib.ptr(two), 2, 0, _lib.ptr(remap), 63) == _lib.MMP_EINVAL  # remap_out too short
        for bad in ([64], [-1], [3, 64, 5]):
            assert raw(_lib.ptr(np.array(bad, np.int32)), len(bad), 0, None, 0) == _lib.MMP_EINVAL
        for guards, needle in (({"gone_only": True}, "instance 1 "), ({"unreferenced": True}, "instance ")):
            with pytest.raises(MmpError) as e:
                s.pods_retire([2, 1] if "gone_only" in guards else sorted({x[0] for a, b in st.records for x in a + b if x[0] >= 0})[:2], **guards)
            assert e.value.code == _lib.MMP_EINVAL and needle in str(e.value)
        same(dump(s, rig, st, keys), before, "EINVAL")
        # n == 0: valid, the identity, no commit
        remap[:] = -7
        after, turned = C.c_int32(-1), C.c_int64(-1)
        assert s.lib.mmp_pods_retire(s.h, None, 0, 3, _lib.ptr(remap), 64, C.byref(after), C.byref(turned)) == 0
        assert list(remap) == list(range(64)) and after.value == 64 and turned.value == 0
        same(dump(s, rig, st, keys), before, "n == 0")
        # MMP_EORDER from the commit stage: the staged table carries an edit that makes the order cyclic (docs/PARITY.md: a full
        # row with a tiny lruTime beside differing versions); the retire names other rows
        rows = s.get_pods()[[0, 1]].copy()
        rows["version"], rows["used"] = [3, 2], rows["capacity"]
        rows["lru_time"] = [5, rig.now - 1000]
        s.upsert_pods(np.array([0, 1], np.int32), rows)
        staged = dump(s, rig, st, keys)
        assert not np.array_equal(staged["pods"][0], before["pods"][0])
        with pytest.raises(MmpError) as e:
            s.commit()
        assert e.value.code == _lib.MMP_EORDER
        with pytest.raises(MmpError) as e:
            s.pods_retire([10, 11])
        assert e.value.code == _lib.MMP_EORDER and s.n_pods == 64
        same(dump(s, rig, st, keys), staged, "EORDER")
        s.upsert_pods(np.array([0, 1], np.int32), before["pods"][0][[0, 1]])
        s.commit()
        same(dump(s, rig, st, keys), before, "edit undone")
        # MMP_ESTATE: the instance table outgrew the id table
        s.upsert_pods(np.array([64], np.int32), before["pods"][0][[0]])
        grown = dump(s, rig, st)  # (no resolutions: the by-key call refuses this context too)
        assert len(grown["pods"][0]) == 65
        with pytest.raises(MmpError) as e:
            s.pods_retire([1])
        assert e.value.code == _lib.MMP_ESTATE
        same(dump(s, rig, st), grown, "ESTATE, outgrown id table")
    finally:
        s.close()
    # ... and a pod-axis shard context
    s = rig.solver()
    try:
        st = rig.fresh()
        rig.load(s, st, commit=False)
        s.shard_configure(0, 2)
        before = dump(s, rig, st, committed=False)
        with pytest.raises(MmpError) as e:
            s.pods_retire([1])
        assert e.value.code == _lib.MMP_ESTATE and len(s.get_pods()) == 64
        same(dump(s, rig, st, committed=False), before, "ESTATE, shard context")
    finally:
        s.close()


@pytest.mark.parametrize("committed", [True, False])
def test_stale_type_rows_stay_refused(committed):
    """Types loaded for 64 instances, one id joins (65 rows: two words, a commit refuses the one-word rows), one instance is
    retired (64 rows again).  The stale rows must not pass the commit's check on the way back across the word edge: the retire is
    refused with nothing changed, and goes through once the host has loaded its types for the 65."""
    rig = Rig(103, 64, 100)
    assert rig.n_types > 0 and any(rig.has_allowed)
    s, ref = rig.solver(), rig.solver()
    try:
        st = rig.fresh()
        rig.load(s, st, commit=committed)
        st.pods.append([b"rsjoin-00001"])
        s.append_pod_ids([b"rsjoin-00001"])
        st.label_words.append(0)
        st.label_counts.append(0)
        assert np.array_equal(s.get_pods(), st.pods.rows)
        old_ids, keys = list(st.pods.ids), resolve_keys(st.pods.ids)
        with pytest.raises(MmpError) as e:
            s.commit()
        assert e.value.code == _lib.MMP_ESTATE
        before = dump(s, rig, st, keys, committed=committed, decide=False)
        for pods in ([3], [64], []):
            with pytest.raises(MmpError) as e:
                s.pods_retire(pods)
            assert e.value.code == _lib.MMP_ESTATE and "type" in str(e.value), pods
        same(dump(s, rig, st, keys, committed=committed, decide=False), before, "stale types")
        with pytest.raises(MmpError) as e:
            s.commit()  # 64 words would have fitted: still refused
        assert e.value.code == _lib.MMP_ESTATE
        rig.joined([s], st, 1)
        if committed:
            s.commit()
        st.missing = [s.missing_instances().get(p, 0) for p in range(s.missing_slots())]
        retire_both(rig, s, st, [3], "types reloaded")
        assert_equals_a_load(rig, s, ref, st, old_ids, "types reloaded", committed=committed)
    finally:
        s.close()
        ref.close()


def test_two_runs_are_byte_identical():
    rig = Rig(99, 129, 300)
    outs = []
    for _ in range(2):
        s = rig.solver()
        try:
            st = rig.fresh()
            rig.load(s, st)
            rig.mark(s, st)
            keys = resolve_keys(st.pods.ids)
            gone = [int(p) for p in np.random.default_rng(4).choice(129, 50, replace=False)]
            remap, count = s.pods_retire(gone)
            retire(st, gone)
            d = dump(s, rig, st, keys)
            d["remap"] = [remap, np.array([count])]
            d["raw"] = [np.frombuffer(x.tobytes(), np.uint8) for k in ("pods", "models", "census", "order") for x in d[k]]
            outs.append(d)
        finally:
            s.close()
    same(outs[0], outs[1], "two runs")


def test_beside_readers():
    """A census reader sees the state before or the state after.  A placing thread whose requests name only survivors, while the
    retire names only the HIGHEST indices (tombstones nobody is registered on, as the intended loop leaves them): the survivors'
    indices are the same on both sides, so every answer is the one expected answer."""
    rig = Rig(100, 120, 300)
    top = list(range(100, 120))
    rows = rig.state.pods.rows
    rows["flags"][100:] = (rows["flags"][100:] | _lib.POD_TOMBSTONE) & ~np.uint32(_lib.POD_LIVE)
    rig.state.records = [([e for e in a if e[0] < 100], [e for e in b if e[0] < 100]) for a, b in rig.state.records]
    s, ref = rig.solver(), rig.solver()
    try:
        st = rig.fresh()
        rig.load(s, st)

        def census(ctx):
            c = ctx.registry_census()
            return [np.array([int(c[0][k]) for k in rcm.SCALARS]), c[1], c[2]]

        states = [census(s)]
        reqs, extra = wl.fuzz_requests(rig.fleet_of(st), 3, 64)
        reqs["self_pod"] = np.where(reqs["self_pod"] >= 100, 7, reqs["self_pod"])
        extra = np.where(extra >= 100, extra - 50, extra).astype(np.int32)
        after = rig.fresh()
        retire(after, top)
        rig.load(ref, after)
        states.append(census(ref))
        assert len(states[0][1]) == 120 and len(states[1][1]) == 100
        expected = ref.place(reqs, extra, rig.now)
        assert_same_decisions(rig.fleet_of(st), reqs, s.place(reqs, extra, rig.now), expected)
        seen, placed, errors, started = [], [], [], threading.Event()

        def reader():
            try:
                for _ in range(200):
                    seen.append(census(s))
                    started.set()
            except Exception as e:  # noqa: BLE001
                errors.append(e)
                started.set()

        def placer():
            try:
                for _ in range(200):
                    placed.append(s.place(reqs, extra, rig.now))
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=reader), threading.Thread(target=placer)]
        for th in threads:
            th.start()
        started.wait()
        remap, count = s.pods_retire(top, gone_only=True, unreferenced=True)
        for th in threads:
            th.join()
        assert not errors, errors
        assert count == 0 and list(remap[:100]) == list(range(100))
        for c in seen + [census(s)]:
            assert any(len(c[1]) == len(w[1]) and all(np.array_equal(x, y) for x, y in zip(c, w)) for w in states)
        assert len(census(s)[1]) == 100
        for got in placed + [s.place(reqs, extra, rig.now)]:
            assert_same_decisions(rig.fleet_of(st), reqs, got, expected)
    finally:
        s.close()
        ref.close()
