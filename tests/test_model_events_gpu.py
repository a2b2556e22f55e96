"""mmp_models_events_json: registry events by key.  Streams built by construction go through the device path in batches of 1, 5,
64, 65, 300 and 4 096 events over an 8 x 300 fuzz fleet; after every batch every output equals tests/model_events_model.py and
the registry equals, record by record, a twin context fed the same events through a host dict and mmp_models_upsert_json
(tests/model_events_fixtures.py).  Then: one key 4 096 times and 4 096 new keys, twice each, byte-identical; the same streams with
the id hash masked so that ids collide; every refusal, with nothing changed; batches beside a census reader.  All exact."""
import threading

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd.solver import MmpError, Solver
from tests import registry_prune_model as rp
from tests.model_events_fixtures import BATCHES, World, make_model_ids, make_stream, run_stream, same_registry, start, to_arrays

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed,n_base", [(0, 8), (1, 300)])
def test_event_streams_against_the_model_and_the_twin(seed, n_base):
    world = World(seed)
    base, batches = make_stream(world, n_base)
    assert tuple(len(b[0]) for b in batches) == BATCHES
    run_stream(world, base, batches, checkpoints=(1, 3, 4, 5), decisions=True)


@pytest.mark.parametrize("bits", [0, 4])
def test_the_300_event_stream_when_ids_collide(monkeypatch, bits):
    """Probes are as long as the table is full here, so the stream stops at its 300-event batch."""
    monkeypatch.setenv("MMP_MODEL_ID_HASH_BITS", str(bits))
    world = World(2)
    base, batches = make_stream(world, 8, BATCHES[:5])
    run_stream(world, base, batches, checkpoints=(2, 4))


def _contended(world, keys, values, deleted):
    """One batch on a fresh context with 5 named rows -> everything the call and the table answer, as bytes."""
    base = [b"base-%d" % i for i in range(5)]
    s, twin, model = start(world, base)
    try:
        want = model.events(keys, values, deleted, True)
        got = s.models_events_json(keys, values, deleted, True)
        twin.events(keys, values, deleted, True)
        for name, g, w in zip(("status", "model_idx", "last_unload"), got, want):
            assert np.array_equal(g, w), (name, np.nonzero(g != w)[0][:8])
        assert got[3] == want[3]
        reg = rp.compact(*s.get_models())
        same_registry(reg, rp.compact(*twin.s.get_models()), "twin")
        same_registry(reg, to_arrays(model.recs), "model")
        ids = s.model_ids_get()
        assert ids == model.ids
        return [g.tobytes() for g in got[:3]] + [got[3], ids] + [a.tobytes() for a in reg]
    finally:
        s.close()
        twin.s.close()


def test_one_key_4096_times_and_4096_new_keys_twice_each():
    world = World(3)
    rng, n = np.random.default_rng(5), 4096
    values = [world.values[int(i)] if rng.random() < 0.85 else world.values[int(i)][:-3] for i in rng.integers(0, 300, n)]
    deleted = (rng.random(n) < 0.15).astype(np.uint8)
    deleted[:3] = 1  # the key is unknown until event 3
    deleted[3] = 0
    one = _contended(world, [b"the-one-key"] * n, values, deleted)
    assert one == _contended(world, [b"the-one-key"] * n, values, deleted)
    assert one[3] == 1
    keys = make_model_ids(np.random.default_rng(6), n)
    many = _contended(world, keys, values, np.zeros(n, np.uint8))
    assert many == _contended(world, keys, values, np.zeros(n, np.uint8))
    assert many[3] == n and many[4][5:] == keys


A = '{"type": "t1", "lu": 9, "lul": 4, "instanceIds": {"aaaaaa-00002": 5, "bbbbbb-00001": 7}}'
B = '{"lu": 11, "lul": 6, "failedIn": {"aaaaaa-00001": 3}, "instanceIds": {"bbbbbb-00001": 8}}'
IDS3 = ["aaaaaa-00001", "aaaaaa-00002", "bbbbbb-00001"]


def test_refusals_change_nothing():
    """Every MMP_EINVAL / MMP_ESTATE of the call but one: the entry-arena overflow is the shared pipeline's refusal (the line
    mmp_models_upsert_json has always had) and would need an arena of 2^31 entries to reach."""
    mids = [b"m-a", b"m-b", "m-é".encode()]
    s = Solver(100, 1000)
    try:
        L = s.lib
        koff, off = np.array([0, 3, 6], np.int32), np.array([0, len(A), len(A) + len(B)], np.int64)
        kblob, blob = b"newm-a", (A + B).encode()
        idx, lul, status, n_app = np.full(4, -7, np.int32), np.zeros(4, np.int64), np.full(4, -7, np.int32), np.zeros(1, np.int32)

        def call(keys=kblob, koff=koff, buf=blob, off=off, n=2, flags=1, idx=idx, status=status):
            return L.mmp_models_events_json(s.h, keys, _lib.ptr(koff), buf, _lib.ptr(off), n, None, flags, _lib.ptr(idx), _lib.ptr(lul),
                                            _lib.ptr(status), n_app.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32)))

        assert call() == _lib.MMP_ESTATE  # before mmp_pod_ids_load
        s.load_pod_ids(IDS3)
        s.load_type_names(["NLCLASSIFIER", "t1"], 0)
        st, _ = s.ingest_models_json([A, B, A])
        assert not st.any()
        assert call() == _lib.MMP_ESTATE  # before mmp_model_ids_load
        assert np.all(idx == -7) and np.all(status == -7)
        s.model_ids_load(mids)

        def state():
            return [a.copy() for a in s.get_models()], list(s.model_ids_resolve(mids + [b"new"])), s.model_ids_get()

        def unchanged(before):
            after = state()
            assert all(np.array_equal(x, y) for x, y in zip(before[0], after[0])) and before[1:] == after[1:]
            assert np.all(idx == -7) and np.all(status == -7)

        before = state()
        assert before[1] == [0, 1, 2, -1]
        assert call(n=0) == 0  # n == 0 is valid
        for rc in (call(keys=None), call(koff=None), call(off=None), call(buf=None), call(idx=None), call(status=None), call(flags=2),
                   call(n=-1),
                   call(koff=np.array([0, 4, 3], np.int32)),                   # key offsets not monotone
                   call(off=np.array([0, len(blob), len(A)], np.int64))):      # value offsets not monotone
            assert rc == _lib.MMP_EINVAL
            unchanged(before)
        # an append by index resizes the registry without the id table: still accepted, and the by-key calls then refuse
        st, _ = s.upsert_models_json([B], [1])
        assert not st.any()
        status2, idx2, lul2, n = s.models_events_json(["new", "m-a"], [A, B])  # an update by index left the spaces in step
        assert list(status2) == [0, 0] and list(idx2) == [3, 0] and list(lul2) == [4, 6] and n == 1
        mids.append(b"new")
        st, _ = s.upsert_models_json([A], [4])
        assert not st.any() and s.n_models == 5
        state_rows = [a.copy() for a in s.get_models()]
        for fn in (lambda: s.models_events_json(["m-a"], [A]), lambda: s.models_events_json(["m-a"], [""], deleted=[1]),
                   lambda: s.models_events_json(["m-a"], [A], append=False), lambda: s.models_events_json(["brand-new"], [A]),
                   lambda: s.model_ids_resolve(["m-a"]), lambda: s.model_ids_get(0, 1)):
            with pytest.raises(MmpError) as e:
                fn()
            assert e.value.code == _lib.MMP_ESTATE and "resized" in str(e.value)
            assert all(np.array_equal(x, y) for x, y in zip(state_rows, s.get_models()))
        # ... so do a reload of the registry (3 rows for 4 ids) and a load by rows; naming the rows again puts them in step
        s.ingest_models_json([A, B, A])
        with pytest.raises(MmpError) as e:
            s.models_events_json(["m-a"], [A])
        assert e.value.code == _lib.MMP_ESTATE
        s.model_ids_load(mids[:3])
        status2, idx2, _, n = s.models_events_json(["m-b", "new"], [A, A])
        assert list(status2) == [0, 0] and list(idx2) == [1, 3] and n == 1 and s.model_ids_get() == mids
    finally:
        s.close()


def _census_equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_beside_a_census_reader():
    """200 by-key batches alternate 40 rows between two states (one of them deletes a row and both name a key twice) while a second
    thread takes censuses: every census is one state's or the other's — a call is seen whole or not at all."""
    world = World(4)
    rng = np.random.default_rng(11)
    mids = make_model_ids(rng, 240)
    s, twin, _ = start(world, mids[:200])
    try:
        twin.s.close()
        keys = [mids[i] for i in rng.choice(200, 38, replace=False)] + [mids[200], mids[201]]
        keys.append(keys[0])
        dele = np.zeros(41, np.uint8)
        dele[5] = 1
        states = [[world.values[int(i)] for i in rng.integers(200, 300, 41)] for _ in range(2)]
        census = []
        for v in states:
            st, _, _, _ = s.models_events_json(keys, v, dele if v is states[1] else None)
            assert not st.any()
            census.append(s.registry_census())
        assert not _census_equal(census[0], census[1]) and s.n_models == 202
        turns = [0, 1] * 100  # alternating ...
        for k in rng.choice(198, 60, replace=False):
            turns[k] = turns[k + 1]  # ... with a state written twice in a row here and there, so that no reader keeps step with it
        seen, stop, errors = [], threading.Event(), []

        def reader():
            try:
                for _ in range(4000):  # bounded: the writer stops it long before
                    if stop.is_set():
                        break
                    seen.append(s.registry_census())
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        th = threading.Thread(target=reader)
        th.start()
        try:
            for k in turns:
                st, idx, _, n = s.models_events_json(keys, states[k], dele if k else None)
                assert not st.any() and n == 0 and idx[40] == idx[0]
        finally:
            stop.set()
            th.join()
        assert not errors, errors
        which = [[_census_equal(c, w) for w in census] for c in seen]
        assert seen and all(a or b for a, b in which), sum(not (a or b) for a, b in which)
        print(f"{len(seen)} censuses beside 200 batches: {sum(a for a, _ in which)} saw state 0, {sum(b for _, b in which)} state 1")
        assert _census_equal(s.registry_census(), census[turns[-1]])
    finally:
        s.close()
