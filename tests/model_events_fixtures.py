"""What tests/test_model_ids_gpu.py and tests/test_model_events_gpu.py share: model ids of every awkward shape, event streams
whose head holds every outcome kind, and the TWIN — a second context fed the same events the parent's way, through a host dict
from id to row and mmp_models_upsert_json by index."""
import copy
import types

import numpy as np

from modelmesh_amd import _lib
from modelmesh_amd import workload as wl
from modelmesh_amd.solver import Solver
from tests import registry_prune_model as rp
from tests import wire
from tests.ingest_model import model_bean
from tests.model_events_model import APPLIED, MALFORMED, UNKNOWN, ModelEventsModel
from tests.util import assert_same_decisions

BATCHES = (1, 5, 64, 65, 300, 4096)
KINDS = {"update", "join", "join_malformed", "malformed_update", "deletion", "delete_unknown", "delete_before_join",
         "delete_after_join", "unknown_flag_off", "readd", "repeat_in_batch"}


def make_model_ids(rng, n):
    """n distinct ids as bytes: plain names, UTF-8, raw bytes >= 0x80, pairs where one id is a prefix of the other, the empty key."""
    ids, seen = [], set()

    def add(b):
        if b not in seen and len(ids) < n:
            seen.add(b)
            ids.append(b)

    k = 0
    while len(ids) < n:
        r, k = rng.random(), k + 1
        if k == 4:
            add(b"")
        elif r < 0.6:
            add(b"model-%d-%05x" % (k, int(rng.integers(0, 16**5))))
        elif r < 0.7:
            add(("modèle-%d-é" % k).encode())
        elif r < 0.8:
            add(bytes([0xff, 0x80 + k % 64]) + b"raw%d" % k)
        else:
            add(b"m%d" % k)
            add(b"m%d-x" % k)  # m<k> is its prefix
    order = rng.permutation(n)
    return [ids[i] for i in order]


def to_arrays(recs):
    """Records (type, lu, loaded, failed) -> compact (rows, ent_pod, ent_time)."""
    rows = np.zeros(len(recs), dtype=_lib.MODEL_ROW)
    ep, et = [], []
    for i, (ty, lu, loaded, failed) in enumerate(recs):
        rows[i] = (ty, len(ep), len(loaded), len(failed), lu)
        for p, t in tuple(loaded) + tuple(failed):
            ep.append(p)
            et.append(t)
    return rows, np.array(ep, np.int32), np.array(et, np.int64)


def same_registry(a, b, what=""):
    """Two registries record by record: fields and entries in order, not arena offsets."""
    for x, y, name in zip(a, b, ("rows", "ent_pod", "ent_time")):
        assert x.shape == y.shape and np.array_equal(x, y), (what, name)


class World:
    """An 8-instance fuzz fleet with 300 stored ModelRecord values, and the contexts built over it."""

    def __init__(self, seed, pods=8, models=300):
        self.rng = rng = np.random.default_rng(9000 + seed)
        self.fleet = fleet = wl.fuzz_fleet(seed + 60, pods=pods, models=models)
        fleet.pods["flags"] &= ~np.uint32(4)  # tombstones do not exist on the wire
        self.pod_ids = wire.make_ids(rng, pods)
        wire.adopt_ids(fleet, self.pod_ids)
        self.type_names = ["NLCLASSIFIER"] + ["type-%d" % t for t in range(1, max(fleet.n_types, 1))]
        lul = np.where(rng.random(models) < 0.4, fleet.now - rng.integers(1, 10**8, models), 0).astype(np.int64)
        part = types.SimpleNamespace(models=fleet.models, ent_pod=fleet.ent_pod, ent_time=fleet.ent_time)
        self.values = wire.model_values(part, self.pod_ids, self.type_names, rng, lul)

    def solver(self):
        f = self.fleet
        s = Solver(f.min_space_units, f.min_churn_age_ms)
        s.load_pod_ids(self.pod_ids)
        s.load_type_names(self.type_names, 0)
        s.load_pods(f.pods)
        s.load_types(f.n_types, f.allowed, f.prefer, f.has_allowed, f.has_prefer)
        s.load_replaced_rs(f.replaced_rs)
        s.commit()
        return s

    def model(self):
        return ModelEventsModel(self.pod_ids, self.type_names, 0)


class Twin:
    """The parent's route: the id -> row map is a host dict, the events go through mmp_models_upsert_json by index."""

    def __init__(self, solver, base_ids):
        self.s, self.row_of = solver, {k: i for i, k in enumerate(base_ids)}

    def events(self, keys, values, deleted, append):
        vals, idx, dele = [], [], []
        for i, key in enumerate(keys):
            gone = bool(deleted is not None and deleted[i])
            if key not in self.row_of:
                if gone or not append:
                    continue
                self.row_of[key] = len(self.row_of)
            vals.append(values[i])
            idx.append(self.row_of[key])
            dele.append(1 if gone else 0)
        if vals:
            self.s.upsert_models_json(vals, np.array(idx, np.int32), np.array(dele, np.uint8))


def start(world, base_ids):
    """(s, twin, model): the registry holds the first len(base_ids) stored values on every side, the rows named base_ids."""
    n = len(base_ids)
    s, t, model = world.solver(), world.solver(), world.model()
    status, _ = s.ingest_models_json(world.values[:n])
    assert not status.any()
    t.ingest_models_json(world.values[:n])
    model.recs = []
    for v in world.values[:n]:
        b = model_bean(v, model.pod_of, model.type_names, 0)
        model.recs.append((b.type, b.lu, tuple(b.loaded), tuple(b.failed)))
    model.load(base_ids)
    s.model_ids_load(base_ids)
    return s, Twin(t, base_ids), model


def make_stream(world, n_base, batches=BATCHES):
    """-> (base ids, batches); a batch is (keys, values, deleted, append).  The head of the stream is fixed so that every outcome
    kind occurs; the rest is drawn."""
    rng, pv = world.rng, world.values
    n_pool = sum(batches) // 5 + 16
    ids = make_model_ids(rng, n_base + n_pool + 4)
    base, pool, never = ids[:n_base], list(ids[n_base:n_base + n_pool]), ids[n_base + n_pool:]
    known = list(base)

    def good():
        return pv[int(rng.integers(len(pv)))]

    def bad():
        return good()[:-3]

    def join():
        known.append(pool.pop(0))
        return known[-1]

    k0 = base[0]
    u1, u2, u3 = pool[0], pool[1], pool[2]
    head = {
        0: [(k0, good(), 0)],
        1: [(pool[0], good(), 0), (never[0], "", 1), (k0, good(), 0), (base[-1], bad(), 0), (k0, "", 1)],  # append off
        2: [(u1, bad(), 0), (u1, good(), 0), (u2, good(), 0), (u2, "", 1), (k0, good(), 0), (u3, "", 1), (u3, good(), 0), (u3, "", 1),
            (u3, good(), 0), (never[1], "", 1), (u2, good(), 0)],
    }
    for _ in range(3):
        join()
    out = []
    for b, size in enumerate(batches):
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
        out.append((keys, values, np.array(deleted, np.uint8), b != 1))
    return base, out


def kinds_of(model, batch, gone):
    """The outcome kinds of a batch, read off the model as it applies the events one by one."""
    keys, values, deleted, append = batch
    kinds, seen, joined, refused_del = set(), set(), set(), set()
    for i, k in enumerate(keys):
        st, _, _, n_app = model.events([k], [values[i]], deleted[i:i + 1], append)
        if k in seen:
            kinds.add("repeat_in_batch")
        seen.add(k)
        if deleted[i]:
            if st[0] == APPLIED:
                kinds.add("deletion")
                gone.add(k)
                if k in joined:
                    kinds.add("delete_after_join")
            else:
                kinds.add("delete_unknown")
                refused_del.add(k)
        elif st[0] == UNKNOWN:
            kinds.add("unknown_flag_off")
        elif n_app:
            kinds.add("join" if st[0] == APPLIED else "join_malformed")
            joined.add(k)
            if k in refused_del:
                kinds.add("delete_before_join")
        elif st[0] == MALFORMED:
            kinds.add("malformed_update")
        else:
            kinds.add("readd" if k in gone else "update")
            gone.discard(k)
    return kinds


def run_stream(world, base, batches, checkpoints=(), decisions=False):
    """The stream through the by-key call; after every batch the outputs equal the model and the registry equals the twin's and
    the model's, at checkpoints the census and mmp_models_status of every touched row equal the twin's, and at the end (with
    `decisions`) both contexts commit and decide alike."""
    probe, kinds, gone = world.model(), set(), set()
    probe.recs = [(0, 0, (), ())] * len(base)
    probe.load(base)
    for batch in batches:
        kinds |= kinds_of(probe, batch, gone)
    assert kinds == KINDS, KINDS - kinds  # on the CPU first: every outcome kind occurs in this stream

    s, twin, model = start(world, base)
    t = twin.s
    try:
        touched = set()
        for b, (keys, values, deleted, append) in enumerate(batches):
            want = model.events(keys, values, deleted, append)
            got = s.models_events_json(keys, values, deleted, append)
            twin.events(keys, values, deleted, append)
            for name, g, w in zip(("status", "model_idx", "last_unload"), got, want):
                assert np.array_equal(g, w), (b, name, np.nonzero(g != w)[0][:8])
            assert got[3] == want[3] and s.n_models == model.n_models == t.n_models, b
            reg = rp.compact(*s.get_models())
            same_registry(reg, rp.compact(*t.get_models()), (b, "twin"))
            same_registry(reg, to_arrays(model.recs), (b, "model"))
            assert s.model_ids_get() == model.ids, b
            touched |= {int(r) for r in want[1] if r >= 0}
            if b in checkpoints:
                for x, y in zip(s.registry_census(), t.registry_census()):
                    assert np.array_equal(x, y), b
                reqs = np.zeros(len(touched), _lib.STATUS_REQ)
                reqs["model"], reqs["fail_pod"] = sorted(touched), -1
                for x, y in zip(s.models_status(reqs, int(world.fleet.now)), t.models_status(reqs, int(world.fleet.now))):
                    assert np.array_equal(x, y), b
        assert list(s.model_ids_resolve(model.ids)) == list(range(model.n_models))
        if decisions:
            f2 = copy.copy(world.fleet)
            f2.models, f2.ent_pod, f2.ent_time = to_arrays(model.recs)
            reqs, extra = wl.fuzz_requests(f2, 1, 1200)
            for ctx in (s, t):
                ctx.commit()
            assert_same_decisions(f2, reqs, s.place(reqs, extra, f2.now), t.place(reqs, extra, f2.now))
    finally:
        s.close()
        t.close()
