"""GPU: a context's whole life, over and over in one process — create, every call whose buffers mmp_destroy used to free from a
hand-written list (and the eight it did not name: the label tables and j_lab, k_evlu, ev_in / ev_out), a latency slot, a split
batch's words and their retirement, destroy.  Every buffer now frees itself inside mmp_destroy (modelmesh_amd/csrc/devbuf.hpp): a
double free, or a free of memory a kernel still reads, shows here as a fault or as a round that answers differently.

State: 4 instances, the second with one label; 3 models of one copy each (two on instance 0, one on instance 1); one cache of two
entries.  Every round's outputs are byte-equal to the first round's, and the first round's are the Python models' (tests/
pod_labels_model.py, tests/evictions_model.py, the oracle's cache and load-target walk).  Nothing here reads the device's free
memory: that figure belongs to the whole card."""
import ctypes as C

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd import workload as wl
from modelmesh_amd.solver import Fleet, Solver
from oracle import bind as ob
from tests import evictions_model as em
from tests import registry_ops_model as ro
from tests.pod_labels_model import PodLabelsModel
from tests.registry_ops_keyed_model import KeyedRegistry
from tests.registry_ops_model import ModelRecord
from tests.test_cache_keyed_gpu import cop
from tests.util import assert_same_decisions

pytestmark = pytest.mark.gpu
NOW = wl.NOW_MS
MIN_SPACE, CHURN = 6553, 30_000
POD_IDS = ["rs-one-a", "rs-one-b", "rs-two-a", "rs-two-b"]
MODEL_IDS = [b"model-a", b"model-b", b"model-c"]
LABELS = ["gpu"]
SELF_POD, TIMEOUT = 0, 1000
N_DEV = 3  # rows of the device-pointer batch; MMP_SPLIT_FROM is set to it: the smallest batch that splits
ROUNDS = 8


def _pod_values():
    out = []
    for i in range(4):
        labels = ',"labels":["gpu"]' if i == 1 else ""
        out.append('{"lruTime":%d,"count":%d,"cap":131072,"used":%d,"lThreads":1,"lInProg":0,"rpm":%d,"startTime":%d,"vers":7%s}'
                   % (NOW - 60_000 * (i + 1), 2 + i, 20_000 * (i + 1), 50 * i, NOW - 10_000_000 - i, labels))
    return out


def _records():
    t = NOW - 5_000_000
    return [ModelRecord(0, [(0, t)], [], NOW - 4_000), ModelRecord(0, [(0, t + 1)], [], NOW - 3_000), ModelRecord(0, [(1, t + 2)], [], NOW - 2_000)]


class _World:
    """The Python side of one round, computed once: the instance rows and labels, the cache's victim, the evictions' answer, the
    registry behind them, and the two request sets with the oracle's decisions on that registry."""

    def __init__(self):
        m = PodLabelsModel()
        m.names_load(LABELS)
        m.load(POD_IDS)
        self.pod_values = _pod_values()
        self.ingest = m.ingest(self.pod_values, np.arange(4))
        self.rows, self.labels = m.rows.copy(), m.labels_get()
        assert not self.ingest[0].any() and list(self.labels[0]) == [0, 1, 0, 0] and list(self.labels[1]) == [0, 1, 0, 0]
        recs = _records()
        self.models, self.ent_pod, self.ent_time = ro.registry_to_arrays(recs)
        fleet = Fleet(pods=self.rows, models=self.models, ent_pod=self.ent_pod, ent_time=self.ent_time, min_space_units=MIN_SPACE,
                      min_churn_age_ms=CHURN, now=NOW)
        self.order = ob.OracleFleet(fleet).order
        # the cache of instance 0: models a and b, 10 units each in 20; model c's 10 units push a out
        self.cache_lu = [NOW - 900, NOW - 800]
        h = ob.CCache(20, None, NOW)
        for r in (0, 1):
            assert h.apply(0, r, 10, self.cache_lu[r], 0, NOW) == (1, [])
        assert h.apply(0, 2, 10, NOW, 0, NOW) == (1, [0])
        self.victim, self.victim_lu = MODEL_IDS[0], self.cache_lu[0]
        k = KeyedRegistry(MODEL_IDS, recs, self.rows["id_order"].copy())
        self.entries = np.zeros(1, dtype=_lib.EVICTED_ENTRY)
        self.entries[0] = (self.victim_lu, recs[0].instance_ids[SELF_POD], 0, 10, 0)
        self.evictions = em.evictions_run(k, self.entries, [self.victim], SELF_POD, NOW, TIMEOUT, ob.type_set_stats(fleet))
        assert self.evictions[2][0] == _lib.ROP_EDITED  # the copy on instance 0 is deregistered
        self.registry_after = ro.registry_to_arrays(k.records_by_row())
        self.fleet = Fleet(pods=self.rows, models=self.registry_after[0], ent_pod=self.registry_after[1], ent_time=self.registry_after[2],
                           min_space_units=MIN_SPACE, min_churn_age_ms=CHURN, now=NOW)
        orc = ob.OracleFleet(self.fleet)
        self.host_reqs, self.host_extra = wl.fuzz_requests(self.fleet, 11, 1)
        self.dev_reqs, self.dev_extra = wl.fuzz_requests(self.fleet, 12, N_DEV)
        self.dev_reqs["model"] = np.arange(N_DEV)  # every model once, the deregistered one among them
        self.host_want = orc.place(self.host_reqs, self.host_extra, NOW)
        self.dev_want = orc.place(self.dev_reqs, self.dev_extra, NOW)


@pytest.fixture(scope="module")
def world():
    return _World()


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        a = np.zeros(1, np.int32)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(torch.device("cuda", 0))


def _round(w, retire):
    """one context from create to destroy; -> every output of the round, by name"""
    import torch
    from tests import registry_prune_model as rp
    out = {}
    s = Solver(MIN_SPACE, CHURN)
    try:
        s.label_names_load(LABELS)
        s.load_pod_ids(POD_IDS)
        out["ingest status"], out["ingest start"] = s.ingest_pods_json(w.pod_values, np.arange(4))   # lbtab_*, lb_arena, lb_off, j_lab
        out["pods"] = s.get_pods()
        out["label words"], out["label counts"] = s.pod_labels_get()
        s.load_models(w.models, w.ent_pod, w.ent_time)
        s.commit()
        out["order"] = s.order()
        s.model_ids_load(MODEL_IDS)
        out["cache rows"] = s.load_caches_keyed_k([0, 2], w.cache_lu, [10, 10], MODEL_IDS[:2], [20])
        put = np.array([cop(0, _lib.COP_PUT_IF_ABSENT, 10, NOW)], dtype=_lib.CACHE_OP)
        outs, ev, ev_ids, status, rows, ev_lu = s.cache_replay_kt(put, [MODEL_IDS[2]], NOW)           # k_evlu
        out["replay outs"], out["replay evicted"], out["replay status"], out["replay rows"], out["replay times"] = outs, ev, status, rows, ev_lu
        out["replay ids"] = np.frombuffer(b"|".join(ev_ids), np.uint8)
        m = int(outs[0]["n_evicted"])
        entries = np.zeros(m, dtype=_lib.EVICTED_ENTRY)
        for i in range(m):
            entries[i] = (int(ev_lu[i]), int(w.entries[0]["load_time"]), 0, 10, 0)
        idx, eouts, est, edits, info = s.evictions_k(entries, ev_ids[:m], SELF_POD, NOW, TIMEOUT)  # ev_in, ev_out
        out["evictions idx"], out["evictions outs"], out["evictions status"], out["evictions edits"] = idx, eouts, est, edits
        out["evictions info"] = np.frombuffer(info.tobytes(), np.uint8)
        for name, a in zip(("registry rows", "registry pods", "registry times"), rp.compact(*s.get_models())):
            out[name] = a
        out["host place"] = s.place(w.host_reqs, w.host_extra, NOW)                                # a latency slot
        st = torch.cuda.Stream()
        d_r, d_x = _dev(w.dev_reqs), _dev(w.dev_extra)
        d_o = torch.full((N_DEV * _lib.PLACE_OUT.itemsize,), 0xFF, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        s.place_dev(d_r.data_ptr(), N_DEV, d_x.data_ptr() if len(w.dev_extra) else 0, NOW, d_o.data_ptr(), st.cuda_stream)  # the miss words
        st.synchronize()
        out["dev place"] = np.frombuffer(d_o.cpu().numpy().tobytes(), dtype=_lib.PLACE_OUT).copy()
        out["split batches"] = np.array([s.split_batches()[0]])
        if retire:
            assert s.lib.mmp_stream_retire(s.h, C.c_void_p(st.cuda_stream)) == 0                  # ... freed here; else by the context
    finally:
        s.close()
    return out


def _against_the_models(w, got):
    assert np.array_equal(got["ingest status"], w.ingest[0]) and np.array_equal(got["ingest start"], w.ingest[1])
    assert got["pods"].tobytes() == w.rows.tobytes()
    assert np.array_equal(got["label words"], w.labels[0]) and np.array_equal(got["label counts"], w.labels[1])
    assert np.array_equal(got["order"], w.order)
    assert list(got["cache rows"]) == [0, 1]
    assert int(got["replay outs"][0]["n_evicted"]) == 1 and list(got["replay evicted"][:1]) == [0] and list(got["replay times"][:1]) == [w.victim_lu]
    assert got["replay ids"].tobytes().split(b"|")[0] == w.victim
    widx, wouts, wst, wed, _ = w.evictions
    assert np.array_equal(got["evictions idx"], widx) and got["evictions outs"].tobytes() == wouts.tobytes()
    assert np.array_equal(got["evictions status"], wst) and got["evictions edits"].tobytes() == wed.tobytes()
    for name, want in zip(("registry rows", "registry pods", "registry times"), w.registry_after):
        assert np.array_equal(got[name], want), name
    assert_same_decisions(w.fleet, w.host_reqs, got["host place"], w.host_want)
    assert_same_decisions(w.fleet, w.dev_reqs, got["dev place"], w.dev_want)
    assert list(got["split batches"]) == [1]  # the device-pointer batch did take the split route


@pytest.fixture
def _the_batch_splits(monkeypatch):
    monkeypatch.setenv("MMP_MEMO_FROM", "0")
    monkeypatch.setenv("MMP_SPLIT_FROM", str(N_DEV))


def test_eight_lives_in_one_process_answer_alike_and_as_the_models(world, _the_batch_splits):
    first = _round(world, retire=True)
    _against_the_models(world, first)
    for k in range(1, ROUNDS):
        again = _round(world, retire=True)
        assert again.keys() == first.keys()
        for name in first:
            assert again[name].tobytes() == first[name].tobytes(), (k, name)


def test_a_context_destroyed_without_the_stream_retire_frees_the_miss_words_itself(world, _the_batch_splits):
    _against_the_models(world, _round(world, retire=False))
    _against_the_models(world, _round(world, retire=True))  # the process goes on
