"""mmp_pods_events_json: instance-table events by key.  Event streams built by construction go through the device path in
batches of 1, 5, 64, 65 and 300 events; after every batch the rows and every output equal tests/pod_events_model.py, at
checkpoints the rows equal a fresh context built from the current ids with mmp_pods_ingest_json / mmp_pods_remove, and after a
commit the order and the decisions equal the oracle's and that context's."""
import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd import workload as wl
from modelmesh_amd.solver import Fleet, MmpError, Solver
from oracle.bind import OracleFleet
from tests import wire
from tests.pod_events_model import APPLIED, MALFORMED, UNKNOWN, PodEventsModel
from tests.util import assert_same_decisions

pytestmark = pytest.mark.gpu

BATCHES = (1, 5, 64, 65, 300)
KINDS = {"update", "join", "join_malformed", "malformed_update", "deletion", "delete_unknown", "unknown_flag_off", "readd",
         "repeat_in_batch"}


def _stream(seed, n_base, n_pool):
    """-> (base ids, batches); a batch is (keys, values, deleted, live or None, append).  The head of the stream is fixed so
    that every outcome kind occurs; the rest is drawn."""
    rng = np.random.default_rng(7000 + seed)
    n_all = n_base + n_pool
    fleet = wl.fuzz_fleet(seed + 60, pods=n_all, models=10)
    fleet.pods["flags"] &= ~np.uint32(4)
    ids = wire.make_ids(rng, n_all + 4)
    pv = wire.pod_values(fleet, rng, (fleet.now - rng.integers(1, 10**9, n_all)).astype(np.int64))
    base, pool, never = ids[:n_base], list(ids[n_base:n_all]), ids[n_all:]
    known, good, bad = list(base), lambda: pv[int(rng.integers(n_all))], lambda: pv[int(rng.integers(n_all))][:-3]

    def join():
        known.append(pool.pop(0))
        return known[-1]

    k0 = base[0]
    u1, u2, u3 = pool[0], pool[1], pool[2]
    head = {
        0: [(k0, good(), 0)],
        1: [(pool[0], good(), 0), (never[0], "", 1), (k0, good(), 0), (base[-1], bad(), 0), (k0, "", 1)],  # append off
        2: [(u1, bad(), 0), (u1, good(), 0), (u2, good(), 0), (u2, "", 1), (k0, good(), 0), (u3, "", 1), (u3, good(), 0),
            (never[1], "", 1)],
    }
    for _ in range(3):
        join()
    batches = []
    for b, size in enumerate(BATCHES):
        ev = list(head.get(b, []))
        while len(ev) < size:
            r = rng.random()
            if r < 0.12 and pool:
                ev.append((join(), good() if rng.random() < 0.8 else bad(), 0))
            elif r < 0.22:
                ev.append((known[int(rng.integers(len(known)))], "", 1))
            elif r < 0.27:
                ev.append((never[int(rng.integers(len(never)))], "" if rng.random() < 0.5 else good(), int(rng.random() < 0.5)))
            elif r < 0.37:
                ev.append((known[int(rng.integers(len(known)))], bad(), 0))
            else:
                ev.append((known[int(rng.integers(len(known)))], good(), 0))
        keys, values, deleted = (list(x) for x in zip(*ev))
        live = None if b % 2 else (rng.random(size) < 0.8).astype(np.uint8)
        batches.append((keys, values, np.array(deleted, np.uint8), live, b != 1))
    return fleet, base, batches


def _kinds(model, batch, gone_before):
    """The outcome kinds of a batch, read off the model as it applies the events one by one."""
    keys, values, deleted, live, append = batch
    kinds, seen = set(), set()
    for i, key in enumerate(keys):
        k = key.encode()
        had = k in model.index
        was_gone = had and bool(model.rows["flags"][model.index[k]] & _lib.POD_TOMBSTONE) and k in gone_before
        st, _, _, n_app = model.events([key], [values[i]], deleted[i: i + 1], None if live is None else live[i: i + 1], append)
        if k in seen:
            kinds.add("repeat_in_batch")
        seen.add(k)
        if deleted[i]:
            kinds.add("deletion" if st[0] == APPLIED else "delete_unknown")
            if st[0] == APPLIED:
                gone_before.add(k)
        elif st[0] == UNKNOWN:
            kinds.add("unknown_flag_off")
        elif n_app:
            kinds.add("join" if st[0] == APPLIED else "join_malformed")
        elif st[0] == MALFORMED:
            kinds.add("malformed_update")
        else:
            kinds.add("readd" if was_gone else "update")
    return kinds


def _twin(model, last_good, fleet):
    """A fresh context with the model's ids, every pod's last applied value ingested, the deleted ones removed."""
    t = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    t.load_pod_ids(model.ids)
    items = sorted(last_good.items())
    if items:
        status, _ = t.ingest_pods_json([v for _, (v, _) in items], [p for p, _ in items], np.array([lv for _, (_, lv) in items], np.uint8))
        assert not status.any()
    gone = [p for p in range(model.n_pods) if model.rows["flags"][p] & _lib.POD_TOMBSTONE and p in last_good]
    t.remove_pods(np.array(gone, np.int32))
    return t


@pytest.mark.parametrize("seed,n_base,n_pool", [(0, 8, 40), (1, 300, 120)])
def test_event_streams_against_the_model(seed, n_base, n_pool):
    fleet, base, batches = _stream(seed, n_base, n_pool)
    # on the CPU first: every outcome kind occurs in this stream
    probe, kinds, gone = PodEventsModel(), set(), set()
    probe.load(base)
    for batch in batches:
        kinds |= _kinds(probe, batch, gone)
    assert kinds == KINDS, KINDS - kinds

    model, last_good = PodEventsModel(), {}
    model.load(base)
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    try:
        s.load_pod_ids(base)
        for b, (keys, values, deleted, live, append) in enumerate(batches):
            want = model.events(keys, values, deleted, live, append)
            got = s.pods_events_json(keys, values, deleted, live, append)
            for name, g, w in zip(("status", "pod_idx", "start_time"), got, want):
                assert np.array_equal(g, w), (b, name, np.nonzero(g != w)[0][:8])
            assert got[3] == want[3] and s.n_pods == model.n_pods
            assert np.array_equal(s.get_pods(), model.rows), b
            for i in range(len(keys)):
                if want[0][i] == APPLIED and not deleted[i]:
                    last_good[int(want[1][i])] = (values[i], 1 if live is None else int(live[i]))
            if b in (1, 3, 4):  # checkpoints
                t = _twin(model, last_good, fleet)
                try:
                    assert np.array_equal(t.get_pods(), model.rows), b
                    if b == 4:
                        _assert_same_commit(s, t, model, fleet, seed)
                finally:
                    t.close()
    finally:
        s.close()


def _assert_same_commit(s, twin, model, fleet, seed):
    """A registry over the final table, a commit on both contexts: the order and the decisions of the oracle."""
    rng = np.random.default_rng(seed)
    P, M = model.n_pods, 150
    k = rng.integers(0, 4, M)
    f = (rng.random(M) < 0.2).astype(np.int64)
    models = np.zeros(M, _lib.MODEL_ROW)
    models["n_loaded"], models["n_failed"] = k, f
    models["ent_off"] = np.r_[0, np.cumsum(k + f)[:-1]]
    models["last_used"] = fleet.now - rng.integers(0, 10**7, M)
    ent_pod = np.zeros(int((k + f).sum()), np.int32)
    for j in range(M):
        o = int(models["ent_off"][j])
        pods = rng.choice(P, int(k[j] + f[j]), replace=False)
        for a, b in ((o, o + int(k[j])), (o + int(k[j]), o + int(k[j] + f[j]))):  # each list in id order (a TreeMap)
            seg = pods[a - o: b - o]
            ent_pod[a:b] = seg[np.argsort(model.rows["id_order"][seg])]
    ent_time = (fleet.now - rng.integers(0, 10**7, len(ent_pod))).astype(np.int64)
    final = Fleet(model.rows.copy(), models, ent_pod, ent_time, fleet.min_space_units, fleet.min_churn_age_ms, fleet.now)
    orc = OracleFleet(final)
    reqs, extra = wl.fuzz_requests(final, seed, 1200)
    want = orc.place(reqs, extra, final.now, threads=4)
    for ctx in (s, twin):
        ctx.load_models(models, ent_pod, ent_time)
        ctx.commit()
        assert np.array_equal(ctx.order(), orc.order)
        assert_same_decisions(final, reqs, ctx.place(reqs, extra, final.now), want)


def test_refused_calls_change_nothing():
    good = '{"count": 3, "cap": 100, "startTime": 5}'
    s = Solver(100, 1000)
    try:
        L = s.lib
        koff, off = np.array([0, 3], np.int32), np.array([0, len(good)], np.int64)
        idx, st, status, n_app = np.full(4, -7, np.int32), np.zeros(4, np.int64), np.full(4, -7, np.int32), np.zeros(1, np.int32)

        def call(keys, koff, buf, off, n, flags=1, idx=idx, status=status):
            return L.mmp_pods_events_json(s.h, keys, _lib.ptr(koff), buf, _lib.ptr(off), n, None, None, flags, _lib.ptr(idx), _lib.ptr(st),
                                          _lib.ptr(status), n_app.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32)))

        assert call(b"new", koff, good.encode(), off, 1) == _lib.MMP_ESTATE  # before mmp_pod_ids_load
        s.load_pod_ids(["aaaaaa-1", "bbbbbb-1"])
        s.pods_events_json(["aaaaaa-1"], [good])
        before = s.get_pods().copy()
        assert call(b"", koff, None, off, 0) == 0  # n == 0 is valid
        two_k, two_v = np.array([0, 3, 6], np.int32), np.array([0, len(good), 2 * len(good)], np.int64)
        for rc in (call(None, koff, good.encode(), off, 1), call(b"new", None, good.encode(), off, 1),
                   call(b"new", koff, good.encode(), None, 1), call(b"new", koff, None, off, 1),
                   call(b"new", koff, good.encode(), off, 1, idx=None), call(b"new", koff, good.encode(), off, 1, status=None),
                   call(b"new", koff, good.encode(), off, 1, flags=2),
                   call(b"newold", np.array([0, 4, 3], np.int32), (good * 2).encode(), two_v, 2),   # key offsets not monotone
                   call(b"newold", two_k, (good * 2).encode(), np.array([0, 50, 40], np.int64), 2)):  # value offsets not monotone
            assert rc == _lib.MMP_EINVAL
            assert s.n_pods == 2 and np.array_equal(s.get_pods(), before) and np.all(idx == -7) and np.all(status == -7)
        # ... and the context still takes events: the refused joins handed no index out
        status2, idx2, _, n = s.pods_events_json(["new", "aaaaaa-1"], [good, ""], deleted=[0, 1])
        assert list(status2) == [0, 0] and list(idx2) == [2, 0] and n == 1 and len(s.get_pods()) == 3
    finally:
        s.close()


def test_a_resized_instance_table_is_refused():
    """mmp_pods_load / mmp_pods_upsert resize the staged table without the id store: a key would resolve to an index the table does
    not have (or the table would have rows no id names).  Every events call is refused then, with or without a join, and so is
    an append; a load of the ids puts the two in step again."""
    good = '{"count": 3, "cap": 100, "startTime": 5}'
    ids = ["aaaaaa-%04d" % k for k in range(10)]
    s = Solver(100, 1000)
    try:
        s.load_pod_ids(ids)
        s.pods_events_json(ids[:3], [good] * 3)
        for shrink in (True, False):
            if shrink:
                s.load_pods(s.get_pods()[:5].copy())  # 5 rows for 10 ids: id 7 has no row
            else:
                s.upsert_pods(np.array([10], np.int32), np.zeros(1, _lib.POD_ROW))  # 11 rows for 10 ids
            before = s.get_pods().copy()
            for keys, values, deleted, append in (([ids[7]], [good], None, True), ([ids[7]], [""], [1], True), ([ids[1]], [good], None, False),
                                                  (["brand-new-1"], [good], None, True)):
                with pytest.raises(MmpError) as e:
                    s.pods_events_json(keys, values, deleted=deleted, append=append)
                assert e.value.code == _lib.MMP_ESTATE and "resized" in str(e.value)
                assert np.array_equal(s.get_pods(), before)
            with pytest.raises(MmpError) as e:
                s.append_pod_ids(["brand-new-2"])
            assert e.value.code == _lib.MMP_ESTATE and np.array_equal(s.get_pods(), before)
            s.n_pods = len(before)
            s.load_pod_ids(ids)  # the ids again: rows and ids cover the same indices
            status, idx, _, n = s.pods_events_json([ids[7], "brand-new-1"], [good, good])
            assert list(status) == [0, 0] and list(idx) == [7, 10] and n == 1 and len(s.get_pods()) == 11
            s.load_pod_ids(ids)
    finally:
        s.close()
