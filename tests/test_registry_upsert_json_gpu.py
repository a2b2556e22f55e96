"""mmp_models_upsert_json: a batch of registry events (the registry's KV listener, MM.java:628, event() :2807-2854) passed as
stored — one whole ModelRecord JSON value per event, or a deletion — parsed on the device and applied in place.

Oracle = Python's json module.  A TWIN Solver receives the same events as mmp_model_row rows through upsert_models (parsed with
json.loads, ids resolved through the same id list); after every call the two registries must be equal record by record (type,
last_used, the loaded and the failed entries in order) and equal to the sequential model kept here, and the returned status /
lul must be what the test derived.  Everything is exact."""
import copy
import json
import threading
import types

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd import workload as wl
from modelmesh_amd._lib import MODEL_ROW, ROP_DEREGISTER, ROP_LOAD_FAILED, ROP_REGISTER, ptr
from modelmesh_amd.solver import MmpError, Solver
from oracle.bind import OracleFleet
from tests import registry_prune_model as rp
from tests import wire
from tests.registry_ops_model import op_row, ops_array
from tests.util import assert_same_decisions

pytestmark = pytest.mark.gpu

EMPTY = (0, 0, (), ())  # the empty row: all fields zero, no entries


def parse_value(v, pod_of, type_of, unknown_type, default_type):
    """One ModelRecord value as the bean takes it: None if malformed, else ((type, lu, loaded, failed), lul)."""
    try:
        d = json.loads(v)
    except ValueError:
        return None
    if not isinstance(d, dict):
        return None
    for k in ("lu", "lul"):
        if not (isinstance(d.get(k, 0), int) and not isinstance(d.get(k, 0), bool)):
            return None
    maps = []
    for k in ("instanceIds", "failedIn"):
        m = d.get(k)
        if m is None:
            m = {}
        if not isinstance(m, dict) or not all(isinstance(t, int) and not isinstance(t, bool) for t in m.values()):
            return None
        maps.append(tuple((pod_of.get(i, -1), t) for i, t in m.items()))
    t = d.get("type")
    ty = type_of.get(t, unknown_type) if isinstance(t, str) else default_type
    return (ty, d.get("lu", 0), maps[0], maps[1]), d.get("lul", 0)


def to_arrays(recs):
    """Records (type, lu, loaded, failed) -> compact (rows, ent_pod, ent_time)."""
    rows = np.zeros(len(recs), dtype=MODEL_ROW)
    ep, et = [], []
    for i, (ty, lu, loaded, failed) in enumerate(recs):
        rows[i] = (ty, len(ep), len(loaded), len(failed), lu)
        for p, t in tuple(loaded) + tuple(failed):
            ep.append(p)
            et.append(t)
    return rows, np.array(ep, np.int32), np.array(et, np.int64)


def value_of(rec, ids, type_names, lul=0, **more):
    ty, lu, loaded, failed = rec
    d = {"type": type_names[ty], "instanceIds": {ids[p]: t for p, t in loaded}, "failedIn": {ids[p]: t for p, t in failed},
         "lu": lu, "lul": lul}
    d.update(more)
    return json.dumps(d)


class Pair:
    """A Solver fed with JSON events (`j`), its twin fed with the parsed rows (`t`), and the sequential model (`recs`)."""

    def __init__(self, ids, type_names, unknown_type=0, fleet=None):
        self.ids, self.type_names, self.unknown = list(ids), list(type_names), unknown_type
        self.pod_of = {s: i for i, s in enumerate(self.ids)}
        self.type_of = {s: i for i, s in enumerate(self.type_names)}
        self.default = self.type_of.get("NLCLASSIFIER", unknown_type)
        self.recs = []
        ms, ca = (fleet.min_space_units, fleet.min_churn_age_ms) if fleet is not None else (100, 1000)
        self.j, self.t = Solver(ms, ca), Solver(ms, ca)
        for s in (self.j, self.t):
            s.load_pod_ids(self.ids)
            s.load_type_names(self.type_names, unknown_type)
            if fleet is not None:
                s.load_pods(fleet.pods)
                s.load_types(fleet.n_types, fleet.allowed, fleet.prefer, fleet.has_allowed, fleet.has_prefer)
                s.load_replaced_rs(fleet.replaced_rs)
                s.commit()

    def close(self):
        self.j.close()
        self.t.close()

    def parse(self, v):
        return parse_value(v, self.pod_of, self.type_of, self.unknown, self.default)

    def start(self, values):
        """The registry at start-up: a full reload from the stored values on one side, the parsed rows on the other."""
        parsed = [self.parse(v) for v in values]
        assert all(p is not None for p in parsed)
        self.recs = [p[0] for p in parsed]
        status, _ = self.j.ingest_models_json(values)
        assert not status.any()
        self.t.load_models(*to_arrays(self.recs))
        self.same()

    def events(self, values, idx, deleted=None):
        """One call on both sides; checks status, lul and the registries; returns the kinds of event the call held."""
        n, n_before = len(values), len(self.recs)
        st, lul = self.j.upsert_models_json(values, idx, deleted)
        want_st, want_lul, sent, kinds = [], [], [], set()
        state, goods, last_bad = {}, {}, {}
        for i in range(n):
            r = int(idx[i])
            if deleted is not None and deleted[i]:
                got = (EMPTY, 0)
                kinds.add("deletion")
            else:
                got = self.parse(values[i])
            want_st.append(0 if got else 1)
            want_lul.append(got[1] if got else 0)
            last_bad[r] = got is None
            if got:
                state[r] = got[0]
                goods[r] = goods.get(r, 0) + 1
                if r < n_before and not (deleted is not None and deleted[i]):
                    kinds.add("update")
                if any(p < 0 for p, _ in got[0][2] + got[0][3]):
                    kinds.add("unresolved id")
                if not (deleted is not None and deleted[i]) and not got[0][2] and not got[0][3]:
                    kinds.add("no entries")
                sent.append((r, got[0]))
            elif r >= n_before:  # the index has been handed out: the row exists from here on, as this call left it so far
                sent.append((r, state.get(r, EMPTY)))
        for r in last_bad:
            if goods.get(r, 0) >= 2:
                kinds.add("twice well-formed")
            if last_bad[r] and goods.get(r, 0):
                kinds.add("malformed behind well-formed")
            if not goods.get(r, 0):
                kinds.add("only malformed")
        appended = len({r for r in last_bad if r >= n_before})
        if appended >= 2:
            kinds.add("two appends")
        assert list(st) == want_st, [i for i in range(n) if st[i] != want_st[i]][:5]
        assert list(lul) == want_lul
        # the model: events in order, a malformed one changes nothing
        self.recs.extend([EMPTY] * appended)
        for r, rec in state.items():
            self.recs[r] = rec
        if sent:
            rows, ep, et = to_arrays([rec for _, rec in sent])
            self.t.upsert_models(np.array([r for r, _ in sent], np.int32), rows, ep, et)
        assert self.j.n_models == len(self.recs)
        self.same()
        return kinds

    def same(self):
        got, twin, want = rp.compact(*self.j.get_models()), rp.compact(*self.t.get_models()), to_arrays(self.recs)
        for g, t, w, what in zip(got, twin, want, ("rows", "ent_pod", "ent_time")):
            assert np.array_equal(t, w), "the twin left the model: " + what
            if not np.array_equal(g, w):
                bad = np.nonzero(g != w)[0][:5] if g.shape == w.shape else (g.shape, w.shape)
                raise AssertionError(f"{what} differ from the twin at {bad}")


def fleet_pair(seed, pods, models):
    rng = np.random.default_rng(7000 + seed)
    fleet = wl.fuzz_fleet(seed + 60, pods=pods, models=models)
    fleet.pods["flags"] &= ~np.uint32(4)  # tombstones do not exist on the wire
    ids = wire.make_ids(rng, pods)
    wire.adopt_ids(fleet, ids)
    type_names = ["NLCLASSIFIER"] + ["type-%d" % t for t in range(1, max(fleet.n_types, 1))]
    return Pair(ids, type_names, 0, fleet), fleet, rng


def fleet_values(fleet, models, ids, type_names, rng, lul=None):
    """wire.model_values (shuffled field order, defaults omitted, unknown fields) for these models of the fleet."""
    rows, ep, et = fleet.models[models].copy(), [], []
    for k, m in enumerate(fleet.models[models]):
        o, c = int(m["ent_off"]), int(m["n_loaded"] + m["n_failed"])
        rows["ent_off"][k] = len(ep)
        ep.extend(fleet.ent_pod[o:o + c])
        et.extend(fleet.ent_time[o:o + c])
    part = types.SimpleNamespace(models=rows, ent_pod=np.array(ep, np.int64), ent_time=np.array(et, np.int64))
    return wire.model_values(part, ids, type_names, rng, np.zeros(len(rows), np.int64) if lul is None else lul)


ALL_KINDS = {"update", "deletion", "two appends", "twice well-formed", "malformed behind well-formed", "only malformed",
             "unresolved id", "no entries"}


def test_sequences_on_a_fuzz_fleet():
    """8 calls of 1, 7, 63, 64, 65 and 257 events.  Every call of 63 or more holds by construction one of each kind of ALL_KINDS
    (the calls of 1 and 7 events are too short for all eight: an update; an update, a deletion, a doubled row and an append);
    the rest of a call are random updates and appends from the fleet's models.  Then types, commit, 1 500 decisions."""
    pair, fleet, rng = fleet_pair(1, 70, 400)
    ids, tn = pair.ids, pair.type_names
    try:
        pair.start(fleet_values(fleet, np.arange(300), ids, tn, rng))
        seen = set()
        for call, n in enumerate((63, 1, 64, 7, 65, 257, 64, 65)):
            M = len(pair.recs)
            src = rng.integers(0, 400, n)
            lul = np.where(rng.random(n) < 0.4, fleet.now - rng.integers(1, 10**8, n), 0).astype(np.int64)
            vals = fleet_values(fleet, src, ids, tn, rng, lul)
            idx = rng.integers(0, M, n).astype(np.int32)
            dele = np.zeros(n, np.uint8)
            if n >= 7:
                idx[:5] = rng.choice(M, 5, replace=False)
                idx[5] = idx[0]              # a row named twice, both events well-formed
                dele[1] = 1                  # a deletion (its value is a whole record: ignored)
                idx[n - 1] = M               # an append
            if n >= 63:
                rest = np.setdiff1d(np.arange(M), idx[:6])
                idx[6:n - 1] = rng.choice(rest, n - 7, replace=False)  # (the constructed rows have the constructed events only)
                idx[n - 2], idx[n - 1] = M, M + 1  # a second append
                idx[10] = idx[2]             # malformed behind a well-formed event of the same row
                vals[10] = vals[10][:len(vals[10]) // 2]
                vals[11] = '{"lu": 5,}'      # a row with a malformed event only
                vals[12] = json.dumps({"type": tn[-1], "lu": 77, "instanceIds": {ids[3]: 5, "gone-pod-1": 6, ids[1]: 7}})
                vals[13] = '{"type": null, "lu": 12, "instanceIds": {}}'  # a record with no entries
                if call % 2:
                    vals[n - 2] = "{"        # the first append is malformed: the empty row
            kinds = pair.events(vals, idx, dele)
            print(f"call {call}: n={n} models {M} -> {len(pair.recs)} kinds {sorted(kinds)}")
            if n >= 63:
                assert kinds == ALL_KINDS, ALL_KINDS - kinds
            seen |= kinds
        assert seen == ALL_KINDS
        # the records that name an instance nobody knows are registered anew (one more call), then: types, commit, decisions
        stale = [m for m, r in enumerate(pair.recs) if any(p < 0 for p, _ in r[2] + r[3])]
        assert stale
        pair.events(fleet_values(fleet, rng.integers(0, 400, len(stale)), ids, tn, rng), np.array(stale, np.int32))
        f2 = copy.copy(fleet)
        f2.models, f2.ent_pod, f2.ent_time = to_arrays(pair.recs)
        s = pair.j
        s.load_types(fleet.n_types, fleet.allowed, fleet.prefer, fleet.has_allowed, fleet.has_prefer)
        s.commit()
        reqs, extra = wl.fuzz_requests(f2, 1, 1500)
        orc = OracleFleet(f2)
        assert np.array_equal(s.order(), orc.order)
        assert_same_decisions(f2, reqs, s.place(reqs, extra, fleet.now), orc.place(reqs, extra, fleet.now, threads=4))
    finally:
        pair.close()


IDS3 = ["aaaaaa-00001", "aaaaaa-00002", "bbbbbb-00001"]
A = '{"type": "t1", "lu": 9, "lul": 4, "instanceIds": {"aaaaaa-00002": 5, "bbbbbb-00001": 7}}'
B = '{"lu": 11, "lul": 6, "failedIn": {"aaaaaa-00001": 3}, "instanceIds": {"bbbbbb-00001": 8}}'
REC_A, REC_B = (1, 9, ((1, 5), (2, 7)), ()), (0, 11, ((2, 8),), ((0, 3),))
BAD = '{"type": "t1", "instanceIds": {"aaaaaa-00001": }}'


def test_order_of_events_table():
    pair = Pair(IDS3, ["NLCLASSIFIER", "t1"])
    try:
        pair.start([B, B, B, B, B, B])
        #        row:  0  0    1  1      2  2     3   3    4      5 (untouched)   6 (appended)  7 (appended, deleted, empty value)
        vals = [A, B,  A, BAD,   A, "",  "", A,   BAD,                             BAD,          ""]
        idx = [0, 0,   1, 1,     2, 2,   3, 3,    4,                               6,            7]
        dele = [0, 0,  0, 0,     0, 1,   1, 0,    0,                               0,            1]
        pair.events(vals, np.array(idx, np.int32), np.array(dele, np.uint8))
        assert pair.recs == [REC_B, REC_A, EMPTY, REC_A, REC_B, REC_B, EMPTY, EMPTY]
        rows, ep, et = rp.compact(*pair.j.get_models())
        assert list(rows["type"]) == [0, 1, 0, 1, 0, 0, 0, 0] and list(rows["last_used"]) == [11, 9, 0, 9, 11, 11, 0, 0]
        assert list(rows["n_loaded"]) == [1, 2, 0, 2, 1, 1, 0, 0] and list(rows["n_failed"]) == [1, 0, 0, 0, 1, 1, 0, 0]
        assert list(ep) == [2, 0, 1, 2, 1, 2, 2, 0, 2, 0] and list(et) == [8, 3, 5, 7, 5, 7, 8, 3, 8, 3]
        # an empty value that is not deleted is malformed; deleted == NULL: no event is a deletion
        st, lul = pair.j.upsert_models_json(["", A, ""], np.array([5, 2, 2], np.int32), None)
        assert list(st) == [1, 0, 1] and list(lul) == [0, 4, 0]
        pair.t.upsert_models(np.array([2], np.int32), *to_arrays([REC_A]))
        pair.recs[2] = REC_A
        pair.same()
        st, lul = pair.j.upsert_models_json([A, B], np.array([0, 8], np.int32), np.array([0, 0], np.uint8))
        assert list(st) == [0, 0] and list(lul) == [4, 6] and pair.j.n_models == 9
    finally:
        pair.close()


def _ids_for(n):
    return ["p%d" % i for i in range(n)]


def _rec(rng, n_pods, n_loaded, n_failed, ty=1):
    pods = rng.choice(n_pods, n_loaded + n_failed, replace=False)
    ent = [(int(p), int(rng.integers(1, 10**12))) for p in pods]
    return (ty, int(rng.integers(1, 10**12)), tuple(ent[:n_loaded]), tuple(ent[n_loaded:]))


def test_parser_routes_through_the_indirection():
    """Values longer than the 2 048-byte LDS tile (one lane walks them) beside short ones: alone on their wavefront in a small
    call, and inside a wavefront's group of records in a call of 16 390 events (a wavefront takes two records from 16 384 events
    on); 64 copies on one record; 5 000 events (more than one round of workgroups); n = 0 and n = 1 of every kind."""
    rng = np.random.default_rng(31)
    ids, tn = _ids_for(400), ["NLCLASSIFIER", "t1"]
    pair = Pair(ids, tn)
    try:
        short = [value_of(_rec(rng, 400, int(rng.integers(0, 4)), int(rng.integers(0, 2))), ids, tn, lul=int(k)) for k in range(50)]
        pair.start(short[:40])
        long_map = value_of(_rec(rng, 400, 100, 20), ids, tn, lul=3)
        long_junk = value_of(_rec(rng, 400, 2, 1), ids, tn, lul=5, junk=["x" * 40, {"y": "a,b:{c}"}] * 60)
        copies64 = value_of(_rec(rng, 400, 64, 0), ids, tn)
        assert min(len(long_map), len(long_junk)) > 2048 > len(copies64) > max(map(len, short))
        pair.events([], np.zeros(0, np.int32))  # n = 0
        pair.events([short[41], long_map, short[42], long_junk, copies64, long_map[:-1], long_junk],
                    np.array([3, 5, 40, 7, 41, 5, 9], np.int32), np.array([0, 0, 0, 0, 0, 0, 1], np.uint8))
        one = [("update", short[43], 2, 0), ("deletion", short[44], 3, 1), ("deleted, empty value", "", 4, 1),
               ("append", short[45], len(pair.recs), 0), ("malformed", BAD, 6, 0), ("malformed append", "", len(pair.recs) + 1, 0),
               ("unresolved id", '{"instanceIds": {"nobody": 4}}', 8, 0), ("no entries", "{}", 10, 0), ("long", long_map, 11, 0),
               ("long malformed", long_junk[:-2], 11, 0), ("long deleted", long_junk, 11, 1)]
        for what, v, r, d in one:  # n = 1 of every kind
            pair.events([v], np.array([r], np.int32), np.array([d], np.uint8))
        M = len(pair.recs)
        for n in (5000, 16390):
            pool = short + [BAD, "", long_junk[:70]]
            pick = rng.integers(0, len(pool), n)
            vals = [pool[k] for k in pick]
            idx = rng.integers(0, M, n).astype(np.int32)
            dele = (rng.random(n) < 0.1).astype(np.uint8)
            for k, v in ((1, long_map), (2, long_junk), (7, long_map), (n - 1, long_junk), (n - 3, copies64)):
                vals[k], dele[k] = v, 0
            idx[n - 4:] = [M, 5, M + 1, M + 2]
            pair.events(vals, idx, dele)
            M = len(pair.recs)
    finally:
        pair.close()


def test_arena_growth_and_squeeze():
    """300 records, each call rewrites all of them with 64 entries: live = 19 200 entries, every call leaves as many behind, and
    the arena is squeezed when the garbage has passed max(live, 65 536): every 4th call.  Then an append beyond the row table."""
    rng = np.random.default_rng(32)
    ids, tn = _ids_for(200), ["NLCLASSIFIER", "t1"]
    M, K, floor = 300, 64, 1 << 16
    pair = Pair(ids, tn)
    try:
        def rewrite():
            return [value_of(_rec(rng, 200, K - 4, 4), ids, tn) for _ in range(M)]
        pair.start(rewrite())
        live = M * K
        per_squeeze = max(live, floor) // live + 1  # calls until garbage = calls * live > max(live, floor)
        squeezes, arena = 0, live
        for call in range(2 * per_squeeze):
            order = rng.permutation(M).astype(np.int32)
            pair.events(rewrite(), order)
            now = len(pair.j.get_models()[1])
            garbage = arena  # the call appends `live` entries behind the `arena` there were, and `live` of them all are live
            assert now == (live if garbage > max(live, floor) else arena + live), (call, now, arena)
            squeezes += now == live
            arena = now
        assert squeezes == 2 and per_squeeze == 4
        cap_rows = (M * MODEL_ROW.itemsize + 255) // 256 * 256 // MODEL_ROW.itemsize  # rows the table's allocation holds
        n_new = cap_rows - M + 40
        pair.events([value_of(_rec(rng, 200, 2, 1), ids, tn) for _ in range(n_new)], np.arange(M, M + n_new, dtype=np.int32))
        pair.events(rewrite()[:50], np.arange(M + n_new - 50, M + n_new, dtype=np.int32))
    finally:
        pair.close()


def _census_equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_host_bookkeeping_without_a_commit():
    """After a JSON upsert (no commit): census, an applied mmp_registry_ops on rows just written, an applied prune, load-target and
    serve decisions — the same on both sides."""
    pair, fleet, rng = fleet_pair(2, 60, 500)
    ids, tn = pair.ids, pair.type_names
    try:
        pair.start(fleet_values(fleet, np.arange(400), ids, tn, rng))
        n = 150
        src = rng.integers(0, 500, n)
        idx = np.concatenate([rng.choice(400, n - 30, replace=False), np.arange(400, 430)]).astype(np.int32)
        dele = (rng.random(n) < 0.1).astype(np.uint8)
        vals = fleet_values(fleet, src, ids, tn, rng)
        vals[3] = vals[3][:-2]
        pair.events(vals, idx, dele)
        j, t, now = pair.j, pair.t, int(fleet.now)
        for a, b in zip(j.registry_census(), t.registry_census()):
            assert np.array_equal(a, b)
        assert int(j.registry_census()[0]["n_models"]) == len(pair.recs) == 430
        # ops on rows the call has just written: a copy more, a copy less, a failed load
        written = [int(r) for r in idx[:60]]
        ops = []
        for k, m in enumerate(written[:45]):
            held = [p for p, _ in pair.recs[m][2]]
            if k % 3 == 0:
                ops.append(op_row(m, int(rng.integers(0, 60)), ROP_REGISTER, last_used=now - 5, load_time=now - 50))
            elif k % 3 == 1 and held:
                ops.append(op_row(m, held[0], ROP_DEREGISTER))
            else:
                ops.append(op_row(m, int(rng.integers(0, 60)), ROP_LOAD_FAILED, load_time=now - 7))
        ops = ops_array(list({o[0]: o for o in ops}.values()))
        got, want = j.registry_ops(ops, now), t.registry_ops(ops, now)
        assert int(got[2]["n_edits"]) > 10
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
        gone = 600_000
        got, want = j.prune_registry(0, now + gone, gone_after_ms=gone), t.prune_registry(0, now + gone, gone_after_ms=gone)
        got2, want2 = j.prune_registry(0, now + 3 * gone, gone_after_ms=gone), t.prune_registry(0, now + 3 * gone, gone_after_ms=gone)
        for a, b in zip(got + got2, want + want2):
            assert np.array_equal(a, b)
        assert j.missing_instances() == t.missing_instances()
        for a, b in zip(rp.compact(*j.get_models()), rp.compact(*t.get_models())):
            assert np.array_equal(a, b)
        for a, b in zip(j.registry_census(), t.registry_census()):
            assert np.array_equal(a, b)
        # decisions, still without a commit
        f2 = copy.copy(fleet)
        f2.models, f2.ent_pod, f2.ent_time = rp.compact(*t.get_models())
        reqs, extra = wl.fuzz_requests(f2, 2, 1500)
        assert_same_decisions(f2, reqs, j.place(reqs, extra, now), t.place(reqs, extra, now))
        sr = np.zeros(300, dtype=_lib.SERVE_REQ)
        sr["model"] = rng.choice(written, 300)
        sr["self_pod"] = rng.integers(-1, 60, 300)
        sr["flags"] = rng.integers(0, 4, 300)
        sr["assume_completed_ms"] = 3000
        sr["last_invoke_time"] = now - 10
        in_use = rng.integers(0, 3, 60).astype(np.int32)
        last_used = (now - rng.choice([0, 5, 100, 10_000], 60)).astype(np.int64)
        sr, counters = t.serve_counters(sr, in_use, last_used)
        # (the counter rows come from the twin's host mirror of the registry; both sides get the same ones)
        none32, none64 = np.zeros(0, np.int32), np.zeros(0, np.int64)
        assert np.array_equal(j.serve_k(sr, counters, none32, none64, now), t.serve_k(sr, counters, none32, none64, now))
    finally:
        pair.close()


def test_refusals_leave_the_registry_as_it_was():
    pair = Pair(IDS3, ["NLCLASSIFIER", "t1"])
    try:
        pair.start([A, B, A])
        j, L = pair.j, pair.j.lib
        before = [a.copy() for a in j.get_models()]
        blob = (A + B).encode()
        good_off = np.array([0, len(A), len(A) + len(B)], np.int64)
        lul, status = np.zeros(2, np.int64), np.zeros(2, np.int32)

        def call(off=good_off, idx=(0, 1), n=2, st=status, buf=blob):
            ix = np.array(idx, np.int32)
            return L.mmp_models_upsert_json(j.h, buf, ptr(off), n, ptr(ix), None, ptr(lul), ptr(st))

        assert call(idx=(0, 4)) == _lib.MMP_EINVAL         # an index gap (3 would append)
        assert call(idx=(3, 5)) == _lib.MMP_EINVAL         # ... behind an append of the same call
        assert call(idx=(-1, 1)) == _lib.MMP_EINVAL        # a negative index
        assert call(off=np.array([0, len(blob), len(A)], np.int64)) == _lib.MMP_EINVAL  # non-monotone offsets
        assert call(st=None) == _lib.MMP_EINVAL            # no status_out
        assert call(off=None) == _lib.MMP_EINVAL and call(buf=None) == _lib.MMP_EINVAL and call(n=-1) == _lib.MMP_EINVAL
        assert L.mmp_models_upsert_json(j.h, blob, ptr(good_off), 2, None, None, ptr(lul), ptr(status)) == _lib.MMP_EINVAL
        for a, b in zip(before, j.get_models()):
            assert np.array_equal(a, b)
        assert j.n_models == 3
        fresh = Solver(100, 1000)
        try:
            assert L.mmp_models_upsert_json(fresh.h, blob, ptr(good_off), 2, ptr(np.array([0, 1], np.int32)), None, ptr(lul),
                                            ptr(status)) == _lib.MMP_ESTATE  # before mmp_pod_ids_load
            with pytest.raises(MmpError):
                fresh.upsert_models_json([A], [0])
            assert fresh.get_models()[0].shape == (0,)
        finally:
            fresh.close()
        assert call() == _lib.MMP_OK and list(status) == [0, 0] and list(lul) == [4, 6]  # and the same call, well-formed, is taken
    finally:
        pair.close()


def test_beside_a_census_reader():
    """100 JSON upserts alternate 40 rows between two states while a second thread takes censuses: every census is one state's
    or the other's (a call is seen whole or not at all)."""
    pair, fleet, rng = fleet_pair(3, 40, 300)
    ids, tn = pair.ids, pair.type_names
    try:
        pair.start(fleet_values(fleet, np.arange(200), ids, tn, rng))
        rows = rng.choice(200, 40, replace=False).astype(np.int32)
        dele = np.zeros(40, np.uint8)
        dele[5] = 1
        states = [fleet_values(fleet, rng.integers(200, 300, 40), ids, tn, rng) for _ in range(2)]
        j, census = pair.j, []
        for v in states:
            pair.events(v, rows, dele if v is states[1] else None)
            census.append(j.registry_census())
        assert not _census_equal(census[0], census[1])
        turns = [0, 1] * 50  # alternating ...
        for k in rng.choice(98, 30, replace=False):
            turns[k] = turns[k + 1]  # ... with a state written twice in a row here and there, so that no reader keeps step with it
        seen, stop, errors = [], threading.Event(), []

        def reader():
            try:
                while not stop.is_set():
                    seen.append(j.registry_census())
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        th = threading.Thread(target=reader)
        th.start()
        try:
            for k in turns:
                st, _ = j.upsert_models_json(states[k], rows, dele if k else None)
                assert not st.any()
        finally:
            stop.set()
            th.join()
        assert not errors, errors
        which = [[_census_equal(c, w) for w in census] for c in seen]
        assert seen and all(a or b for a, b in which), sum(not (a or b) for a, b in which)
        print(f"{len(seen)} censuses beside 100 upserts: {sum(a for a, _ in which)} saw state 0, {sum(b for _, b in which)} state 1")
        assert _census_equal(j.registry_census(), census[1])
    finally:
        pair.close()
