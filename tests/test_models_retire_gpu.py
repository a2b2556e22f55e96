"""mmp_models_retire: registry rows leave the index space and the registry, its entry arena, the id arena and the model-id table
are compacted on the device.  The oracle is tests/model_retire_model.py over tests/model_events_model.py, and a second context
LOADED with exactly the survivors: after a retire everything the first context answers — records, ids, resolutions, census,
status, decisions — equals what the second one answers.  At the wavefront and workgroup edges of a lane-per-row kernel, with the
id hash masked so that ids collide, with events and further retires behind it, through a whole event stream, every refusal with
nothing changed, twice byte-identical, beside a census reader.  All comparisons exact."""
import copy
import threading

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd import workload as wl
from modelmesh_amd.solver import MmpError
from tests import registry_census_model as rcm
from tests import registry_prune_model as rp
from tests.ingest_model import model_bean
from tests.model_events_fixtures import World, make_model_ids, make_stream, same_registry, start, to_arrays
from tests.model_events_model import EMPTY
from tests.model_retire_model import retire
from tests.registry_ops_model import op_row, ops_array
from tests.util import assert_same_decisions

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 2, 8, 9, 63, 64, 65, 255, 256, 257, 300)
C = _lib.C


def records(world, n):
    """The first n stored values of the world as model records (type, lu, loaded, failed)."""
    m = world.model()
    out = []
    for v in world.values[:n]:
        b = model_bean(v, m.pod_of, m.type_names, 0)
        out.append((b.type, b.lu, tuple(b.loaded), tuple(b.failed)))
    return out


def load(s, recs, ids):
    """The registry and its names, as a host loads them."""
    s.load_models(*to_arrays(recs))
    s.model_ids_load(ids)


def retire_sets(m0, rng):
    """(name, rows): none, all, first, last, every other, a run across rows 60-70, one across 250-262, a random third — that one
    out of order and with rows named twice."""
    third = list(rng.choice(m0, m0 // 3, replace=False)) if m0 else []
    third = third + third[:2]
    return [("none", []), ("all", list(range(m0))), ("first", [0][:m0]), ("last", [m0 - 1] if m0 else []),
            ("every other", list(range(0, m0, 2))), ("60-70", [r for r in range(60, 71) if r < m0]),
            ("250-262", [r for r in range(250, 263) if r < m0]), ("a third", [int(r) for r in third])]


def plant(s, recs, keep):
    """Three surviving records get 0, 1 and 64 entries (on the context, through upsert_models, and in recs)."""
    a, b, c = keep[0], keep[len(keep) // 2], keep[-1]
    recs[a] = (recs[a][0], recs[a][1] or 5, (), ())
    recs[b] = (recs[b][0], recs[b][1], ((1, 11),), ())
    recs[c] = (recs[c][0], recs[c][1], tuple((k % 8, 1000 + k) for k in range(40)), tuple((k % 8, 2000 + k) for k in range(24)))
    rows, ep, et = to_arrays([recs[a], recs[b], recs[c]])
    s.upsert_models(np.array([a, b, c], np.int32), rows, ep, et)


def census_equal(a, b):
    try:
        rcm.assert_same_census(a, b)
    except AssertionError:
        return False
    return True


def assert_equals_a_load(s, ref, model, old_ids, remap, now, what, squeezed=True):
    """Context s after a retire against the model and against ref, a context loaded with the model's state.  squeezed: the call
    named a row, so it left the entry arena without garbage (n == 0 changes nothing, the arena included)."""
    m1 = model.n_models
    load(ref, model.recs, model.ids)
    assert s.n_models == m1 == ref.n_models == int((remap >= 0).sum()), what
    got, want = s.get_models(), to_arrays(model.recs)
    for g, w, name in zip(got if squeezed else rp.compact(*got), want, ("rows", "ent_pod", "ent_time")):  # offsets and all
        assert g.shape == w.shape and np.array_equal(g, w), (what, name)
    same_registry(rp.compact(*got), rp.compact(*ref.get_models()), what)
    assert s.model_ids_get() == model.ids == ref.model_ids_get(), what
    strangers = [b"never-%d" % i for i in range(3)] + [i + b"x" for i in old_ids[:2]]
    keys = list(old_ids) + strangers
    res = s.model_ids_resolve(keys)
    assert np.array_equal(res[:len(old_ids)], remap) and np.all(res[len(old_ids):] == -1), what
    assert np.array_equal(res, ref.model_ids_resolve(keys)) and np.array_equal(res, model.resolve(keys)), what
    rcm.assert_same_census(s.registry_census(), ref.registry_census(), what)
    if m1:
        reqs = np.zeros(m1, _lib.STATUS_REQ)
        reqs["model"], reqs["fail_pod"] = np.arange(m1), -1
        for x, y in zip(s.models_status(reqs, now), ref.models_status(reqs, now)):
            assert np.array_equal(x, y), what


def same_decisions(world, model, s, ref, what):
    f2 = copy.copy(world.fleet)
    f2.models, f2.ent_pod, f2.ent_time = to_arrays(model.recs)
    reqs, extra = wl.fuzz_requests(f2, 1, 600)
    assert_same_decisions(f2, reqs, s.place(reqs, extra, f2.now), ref.place(reqs, extra, f2.now))


def retire_equals_load(world, m0, sets=None, decide=False):
    rng = np.random.default_rng(100 + m0)
    ids, base = make_model_ids(rng, m0), records(world, m0)
    now = int(world.fleet.now)
    s, ref = world.solver(), world.solver()
    try:
        for name, rows in sets or retire_sets(m0, rng):
            what = (m0, name)
            model = world.model()
            model.recs = list(base)
            model.load(ids)
            load(s, model.recs, ids)
            keep = sorted(set(range(m0)) - set(rows))
            if len(keep) >= 3:
                plant(s, model.recs, keep)
                counts = {len(model.recs[r][2]) + len(model.recs[r][3]) for r in keep}
                assert 0 in counts and 1 in counts and max(counts) >= 64, what
            else:
                assert m0 < 8 or name == "all", what
            want = retire(model, rows)
            got = s.models_retire(rows)
            assert got.dtype == np.int32 and np.array_equal(got, want), what
            assert_equals_a_load(s, ref, model, ids, want, now, what, squeezed=len(rows) > 0)
            if decide and model.n_models:
                same_decisions(world, model, s, ref, what)  # right without a commit ...
                s.commit()
                ref.commit()
                same_decisions(world, model, s, ref, what)  # ... and after one
    finally:
        s.close()
        ref.close()


@pytest.mark.parametrize("m0", SIZES)
def test_retire_equals_a_load_of_the_survivors(m0):
    retire_equals_load(World(0), m0)


def test_decisions_after_a_retire_without_and_with_a_commit():
    rng = np.random.default_rng(7)
    retire_equals_load(World(1), 300, sets=[s for s in retire_sets(300, rng) if s[0] in ("every other", "a third")], decide=True)


@pytest.mark.parametrize("bits", [0, 4])
@pytest.mark.parametrize("m0", [9, 65, 300])
def test_retire_when_ids_collide(monkeypatch, bits, m0):
    monkeypatch.setenv("MMP_MODEL_ID_HASH_BITS", str(bits))
    retire_equals_load(World(2), m0)


def events_equal(s, model, keys, values, deleted, what):
    want = model.events(keys, values, deleted, True)
    got = s.models_events_json(keys, values, deleted, True)
    for name, g, w in zip(("status", "model_idx", "last_unload"), got, want):
        assert np.array_equal(g, w), (what, name)
    assert got[3] == want[3] and s.n_models == model.n_models, what
    same_registry(rp.compact(*s.get_models()), to_arrays(model.recs), what)
    assert s.model_ids_get() == model.ids, what
    assert list(s.model_ids_resolve(model.ids)) == list(range(model.n_models)), what
    return want


def test_life_goes_on_after_a_retire():
    """300 -> 7 survivors (a table of 16 slots), 2 joins (9 ids: 32 slots), 60 joins; new ids and RETIRED ids join alike.  Then a
    second retire, and a registry_ops apply and a prune apply give what they give on a fresh load."""
    world = World(3)
    rng = np.random.default_rng(31)
    ids = make_model_ids(rng, 340)
    base, fresh = ids[:300], ids[300:]
    s, twin, model = start(world, base)
    ref = twin.s
    now = int(world.fleet.now)
    try:
        keep = sorted(int(r) for r in rng.choice(300, 7, replace=False))
        rows = [r for r in range(300) if r not in keep]
        want = retire(model, rows)
        assert np.array_equal(s.models_retire(rows), want) and s.n_models == 7
        assert_equals_a_load(s, ref, model, base, want, now, "first retire")
        retired = [base[r] for r in rows]
        v = world.values
        keys = [retired[0], fresh[0], base[keep[0]], retired[0]]
        idx = events_equal(s, model, keys, [v[1], v[2], v[3], v[4]], np.zeros(4, np.uint8), "2 joins")[1]
        assert list(idx) == [7, 8, 0, 7] and s.n_models == 9
        keys = [k for pair in zip(retired[1:31], fresh[1:31]) for k in pair] + [base[keep[1]], retired[0]]
        dele = np.zeros(62, np.uint8)
        dele[61] = 1  # (the id that joined again is deleted again: its row stays, empty)
        events_equal(s, model, keys, [v[int(i)] for i in rng.integers(0, 300, 62)], dele, "60 joins")
        assert s.n_models == 69 and model.recs[7] == EMPTY
        old = list(model.ids)
        rows = [7, 68, 0, 33, 34, 35]
        want = retire(model, rows)
        assert np.array_equal(s.models_retire(rows), want)
        assert_equals_a_load(s, ref, model, old, want, now, "second retire")
        assert model.recs[7] != EMPTY  # the empty row 7 is gone: what sits there now is a record
        with pytest.raises(MmpError) as e:
            s.models_retire([7], empty_only=True)
        assert e.value.code == _lib.MMP_EINVAL and s.n_models == model.n_models
        # the registry plans on the compacted registry and on the fresh load
        pods = world.fleet.n_pods
        ops = ops_array([op_row(m, int(rng.integers(0, pods)), m % 4, last_used=now - m, load_time=now - 10, load_complete_time=now)
                         for m in range(0, model.n_models, 2)])
        for a, b in zip(s.registry_ops(ops, now), ref.registry_ops(ops, now)):
            assert np.array_equal(a, b)
        same_registry(rp.compact(*s.get_models()), rp.compact(*ref.get_models()), "after the ops")
        for t in (now, now + 700_000):
            for a, b in zip(s.prune_registry(0, t), ref.prune_registry(0, t)):
                assert np.array_equal(a, b)
        same_registry(rp.compact(*s.get_models()), rp.compact(*ref.get_models()), "after the prune")
        assert s.model_ids_get() == model.ids
    finally:
        s.close()
        ref.close()


def empty_rows_of(model, keys, deleted, status):
    """The rows the model holds as deleted by this batch and still empty."""
    gone = {k if isinstance(k, bytes) else k.encode() for k, d, st in zip(keys, deleted, status) if d and st == 0}
    return sorted(model.index[k] for k in gone if model.recs[model.index[k]] == EMPTY)


def test_a_stream_with_a_retire_after_every_batch():
    world = World(4)
    base, batches = make_stream(world, 300)
    # on the CPU first: the stream retires rows, and a retired id joins again later
    probe = world.model()
    probe.recs = records(world, len(base))
    probe.load(base)
    n_retired, left, rejoined = [], set(), 0
    for keys, values, deleted, append in batches:
        before = set(probe.ids)
        st = probe.events(keys, values, deleted, append)[0]
        rejoined += len((set(probe.ids) - before) & left)
        rows = empty_rows_of(probe, keys, deleted, st)
        left |= {probe.ids[r] for r in rows}
        retire(probe, rows, empty_only=True)
        n_retired.append(len(rows))
    assert max(n_retired) >= 1 and rejoined >= 1, (n_retired, rejoined)

    s, twin, model = start(world, base)
    ref = twin.s
    now = int(world.fleet.now)
    try:
        for b, (keys, values, deleted, append) in enumerate(batches):
            want = model.events(keys, values, deleted, append)
            got = s.models_events_json(keys, values, deleted, append)
            for name, g, w in zip(("status", "model_idx", "last_unload"), got, want):
                assert np.array_equal(g, w), (b, name)
            assert got[3] == want[3] and s.n_models == model.n_models, b
            rows = empty_rows_of(model, keys, deleted, want[0])
            assert len(rows) == n_retired[b]
            remap = retire(model, rows, empty_only=True)
            assert np.array_equal(s.models_retire(rows, empty_only=True), remap), b
            assert s.n_models == model.n_models, b
            same_registry(rp.compact(*s.get_models()), to_arrays(model.recs), b)
            assert s.model_ids_get() == model.ids, b
            assert list(s.model_ids_resolve(model.ids)) == list(range(model.n_models)), b
        ids = list(model.ids)
        assert_equals_a_load(s, ref, model, ids, np.arange(len(ids), dtype=np.int32), now, "the end", squeezed=n_retired[-1] > 0)
    finally:
        s.close()
        ref.close()


def test_half_of_2000_rows_over_300_instances():
    """More than one workgroup of every kernel does real work."""
    world = World(5, pods=300, models=2000)
    rng = np.random.default_rng(55)
    rows = [int(r) for r in rng.permutation(2000)[:1000]]
    retire_equals_load(world, 2000, sets=[("half", rows)])


A = '{"type": "type-1", "lu": 9, "lul": 4}'


def test_refusals_change_nothing():
    world = World(6)
    ids = make_model_ids(np.random.default_rng(61), 12)
    s, twin, model = start(world, ids)
    twin.s.close()
    try:
        L, m0 = s.lib, 12
        # row 1 has an entry, row 2 is deleted, row 3 was registered again without copies
        rows, ep, et = to_arrays([(0, 0, ((1, 11),), ()), (0, 77, (), ())])
        s.upsert_models(np.array([1, 3], np.int32), rows, ep, et)
        st, idx, _, _ = s.models_events_json([ids[2]], [""], np.array([1], np.uint8))
        assert list(st) == [0] and list(idx) == [2]
        remap = np.full(16, -7, np.int32)
        after = C.c_int32(-7)

        def call(rows=(2,), n=None, flags=0, remap=remap, max_models=16, null_rows=False):
            r = np.array(rows, np.int32)
            return L.mmp_models_retire(s.h, None if null_rows else _lib.ptr(r), len(r) if n is None else n, flags,
                                       None if remap is None else _lib.ptr(remap), max_models, C.byref(after))

        def state():
            return [a.copy() for a in s.get_models()], s.model_ids_get(), list(s.model_ids_resolve(ids + [b"stranger"]))

        def unchanged(before):
            now = state()
            assert all(np.array_equal(x, y) for x, y in zip(before[0], now[0])) and before[1:] == now[1:]
            assert np.all(remap == -7) and after.value == -7 and s.n_models == m0

        before = state()
        assert before[0][0]["last_used"][3] == 77 and before[0][0]["n_loaded"][3] == 0 and before[0][0]["n_loaded"][1] == 1
        assert not any(int(before[0][0][f][2]) for f in ("type", "n_loaded", "n_failed", "last_used"))  # a deletion leaves the empty row
        for rc in (call(rows=(-1,)), call(rows=(m0,)), call(rows=(2, m0)), call(null_rows=True, n=1), call(flags=2), call(flags=3),
                   call(max_models=m0 - 1), call(n=-1), call(max_models=-1)):
            assert rc == _lib.MMP_EINVAL
            unchanged(before)
        assert call(rows=(2, 1), flags=_lib.RETIRE_EMPTY_ONLY) == _lib.MMP_EINVAL  # a row with entries
        assert "row 1 " in L.mmp_last_error(s.h).decode()
        unchanged(before)
        assert call(rows=(3, 2), flags=_lib.RETIRE_EMPTY_ONLY) == _lib.MMP_EINVAL  # no entries, but a last_used
        assert "row 3 " in L.mmp_last_error(s.h).decode()
        unchanged(before)
        assert call(rows=(5, 3, 1, 2), flags=_lib.RETIRE_EMPTY_ONLY) == _lib.MMP_EINVAL  # the LOWEST such row is named
        assert "row 1 " in L.mmp_last_error(s.h).decode()
        unchanged(before)
        # n == 0 is valid and changes nothing: the identity, the count
        assert call(rows=(), null_rows=True) == 0
        assert list(remap[:m0]) == list(range(m0)) and np.all(remap[m0:] == -7) and after.value == m0
        remap[:] = -7
        after.value = -7
        unchanged(before)
        assert call(rows=(), remap=None, max_models=0) == 0 and after.value == m0
        after.value = -7
        unchanged(before)
        # an append by index puts the id count out of step: MMP_ESTATE, as for every by-key call
        st, _ = s.upsert_models_json([A], [m0])
        assert not st.any() and s.n_models == m0 + 1
        rows_before = [a.copy() for a in s.get_models()]
        for flags in (0, _lib.RETIRE_EMPTY_ONLY):
            assert call(flags=flags) == _lib.MMP_ESTATE and "resized" in L.mmp_last_error(s.h).decode()
            assert np.all(remap == -7) and after.value == -7
            assert all(np.array_equal(x, y) for x, y in zip(rows_before, s.get_models()))
        # naming the rows again puts them in step, and the guarded retire goes through
        s.model_ids_load(ids + [b"thirteenth"])
        got = s.models_retire([2], empty_only=True)
        assert list(got) == [0, 1, -1] + list(range(2, m0)) and s.n_models == m0
        assert s.model_ids_get() == ids[:2] + ids[3:] + [b"thirteenth"]
    finally:
        s.close()


@pytest.mark.parametrize("bits", [None, 0])
def test_two_runs_are_byte_identical(monkeypatch, bits):
    if bits is not None:
        monkeypatch.setenv("MMP_MODEL_ID_HASH_BITS", str(bits))
    world = World(7)
    rng = np.random.default_rng(71)
    ids, recs = make_model_ids(rng, 300), records(world, 300)
    rows = [int(r) for r in rng.choice(300, 120, replace=False)]
    out = []
    for _ in range(2):
        s = world.solver()
        try:
            load(s, recs, ids)
            remap = s.models_retire(rows)
            out.append([a.tobytes() for a in s.get_models()] + [b"\0".join(s.model_ids_get()), remap.tobytes(),
                                                                s.model_ids_resolve(ids).tobytes()])
        finally:
            s.close()
    assert out[0] == out[1]
    assert np.array_equal(np.frombuffer(out[0][4], np.int32), retire_remap(300, rows))


def retire_remap(m0, rows):
    keep = np.ones(m0, bool)
    keep[rows] = False
    return np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)


def test_beside_a_census_reader():
    """A second thread takes 50 censuses while this one retires three times: every census is that of one of the four states — a
    retire is seen whole or not at all."""
    world = World(8)
    rng = np.random.default_rng(81)
    ids = make_model_ids(rng, 300)
    s, twin, model = start(world, ids)
    twin.s.close()
    try:
        n_pods, n_types = s.registry_census_sizes()
        lists = [[int(r) for r in rng.choice(300 - 60 * k, 60, replace=False)] for k in range(3)]
        probe = copy.deepcopy(model)
        states = [rcm.census_closed(*to_arrays(probe.recs)[:2], n_pods, n_types)]
        for rows in lists:
            retire(probe, rows)
            states.append(rcm.census_closed(*to_arrays(probe.recs)[:2], n_pods, n_types))
        assert all(not census_equal(states[i], states[j]) for i in range(4) for j in range(i))
        assert census_equal(s.registry_census(), states[0])
        seen, errors, started = [], [], threading.Event()

        def reader():
            try:
                for _ in range(50):
                    seen.append(s.registry_census())
                    started.set()
            except Exception as e:  # noqa: BLE001
                errors.append(e)
                started.set()

        th = threading.Thread(target=reader)
        th.start()
        try:
            started.wait()
            for rows in lists:
                assert np.array_equal(s.models_retire(rows), retire(model, rows))
        finally:
            th.join()
        assert not errors, errors
        which = [[census_equal(c, w) for w in states] for c in seen]
        assert len(seen) == 50 and all(any(w) for w in which), sum(not any(w) for w in which)
        print("50 censuses beside 3 retires saw the states", [sum(w[k] for w in which) for k in range(4)])
        assert census_equal(s.registry_census(), states[3]) and s.model_ids_get() == model.ids
    finally:
        s.close()
