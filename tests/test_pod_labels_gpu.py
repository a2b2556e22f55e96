"""Instance labels from the wire format (mmp_label_names_load, ingest_pod_labels_kernel, mmp_pod_labels_set / _get): every case
exact against tests/pod_labels_model.py — status, pod index, start time, the rows and the resident words and counts."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd.solver import MmpError, Solver
from tests import pod_labels_corpus as pc
from tests.pod_labels_model import PodLabelsModel, pod_labels_bean

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = (0xABC, 5)


def _fresh(ids, names=pc.NAMES, sentinel=True):
    p = pc.Pair()
    if names is not None:
        p.names(names)
    p.load_ids(ids)
    if sentinel:
        p.set(np.arange(len(ids)), np.full(len(ids), SENTINEL[0], np.uint64), np.full(len(ids), SENTINEL[1], np.int32))
    return p


def test_hand_worked_values_each_alone_by_key_and_by_index():
    values = pc.hand_values()
    ids = ["%06x-%05d" % (k % 3, k) for k in range(len(values))]
    hand = {v: (w, c) for v, w, c in pc.ACCEPTED}
    p = _fresh(ids)
    try:
        for by_key in (True, False):
            for k, v in enumerate(values):  # n = 1: the word read back is the word of the event
                if by_key:
                    (status, idx, _, _), _ = p.events("alone, by key, value %d" % k, [ids[k]], [v])
                    assert idx[0] == k
                else:
                    (status, _), _ = p.ingest("alone, by index, value %d" % k, [v], [k])
                words, counts = p.s.pod_labels_get()
                want = hand.get(v)
                assert (int(status[0]), int(words[k]), int(counts[k])) == ((0,) + want if want else (1,) + SENTINEL), (by_key, v)
            assert not p.diffs, p.diffs[:5]
            p.load_ids(ids)  # a new index space: all words cleared
            p.state("after the ids load")
            p.set(np.arange(len(ids)), np.full(len(ids), SENTINEL[0], np.uint64), np.full(len(ids), SENTINEL[1], np.int32))
    finally:
        p.close()


def test_the_corpus_all_together():
    """hand-worked values, element rounds (63 / 64 / 65 / 130 elements, 8 x 9), chunk edges, tile edges on both routes, a batch"""
    diffs = pc.corpus_differences(4096 + 512)
    assert not diffs, diffs[:8]


def test_all_together_by_index():
    values = pc.hand_values() + pc.tile_fillers() + pc.chunk_edge_values()
    ids = ["%06x-%05d" % (k % 3, k) for k in range(len(values))]
    p = _fresh(ids)
    try:
        p.ingest("all together, by index", values, np.arange(len(values)))
        p.ingest("the same pod three times", [pc.rec('"labels":["gpu"]'), pc.rec('"labels":[1]'), pc.rec('"labels":["zone-a",""]'),
                                              pc.rec('"labels":7')], [3, 3, 3, 3])
        assert p.s.pod_labels_get()[0][3] == pc.ZONE | pc.EMPTY  # the last well-formed event
        assert not p.diffs, p.diffs[:5]
    finally:
        p.close()


@pytest.mark.parametrize("n", [1, 4, 5, 255, 256, 257])
def test_small_batches(n):
    keys, values, deleted = pc.big(n, n_keys=7, seed=n)
    p = _fresh(sorted(set(keys)) + ["spare-id-1"])
    try:
        p.events("n = %d" % n, keys, values, deleted)
        p.events("n = %d, joins" % n, ["new-%d" % (i % 3) for i in range(n)], values)  # unknown ids join with zero words first
        assert not p.diffs, p.diffs[:5]
    finally:
        p.close()


@pytest.mark.parametrize("n", [16384, 32768, 65536])
def test_records_per_wavefront_as_ingest_group_picks_them(n):
    """groups of 2, 4 and 8 short events per wavefront, rejected / over-long / empty values and deletions planted; the largest
    batch twice, on two contexts, with byte-identical outputs"""
    keys, values, deleted = pc.big(n)
    ids = sorted(set(keys))
    p = _fresh(ids)
    try:
        got, want = p.events("n = %d" % n, keys, values, deleted)
        assert not p.diffs, p.diffs[:5]
        assert want[0].any() and (want[0] == 0).sum() > n // 2 and p.m.labels_get()[0].any()
        if n == 65536:
            q = _fresh(ids)
            try:
                again = q.s.pods_events_json(keys, values, deleted)
                for a, b in zip(got[:3], again[:3]):
                    assert a.tobytes() == b.tobytes()
                assert q.s.get_pods().tobytes() == p.s.get_pods().tobytes()
                for a, b in zip(q.s.pod_labels_get(), p.s.pod_labels_get()):
                    assert a.tobytes() == b.tobytes()
            finally:
                q.close()
    finally:
        p.close()


@pytest.mark.parametrize("env", [{"MMP_JGROUP": "3"}, {"MMP_JGROUP": "7"}, {"MMP_LABEL_HASH_BITS": "0"}, {"MMP_LABEL_HASH_BITS": "4"}])
def test_the_corpus_in_a_fresh_process(env):
    """groups of 3 and 7 records per wavefront; the label hashes masked to 0 and 4 bits (every name collides / most do): the byte
    comparison decides, and the answers are those of the model all the same"""
    r = subprocess.run([sys.executable, "-m", "tests.pod_labels_child"], cwd=ROOT, env=dict(os.environ, **env), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "0 differences" in r.stdout


def test_no_table_loaded_is_a_context_that_never_heard_of_labels():
    values = []
    for v in pc.hand_values() + pc.tile_edge_values()[0]:
        try:  # (a value that is invalid only inside the skipped field is UNSPECIFIED while no table is loaded: not sent)
            pod_labels_bean(v, None)
            values.append(v)
        except ValueError:
            pass
    assert len(values) > 150
    ids = ["%06x-%05d" % (k % 3, k) for k in range(len(values))]
    never, unloaded, model = Solver(100, 1000), Solver(100, 1000), PodLabelsModel()
    try:
        unloaded.label_names_load(pc.NAMES)
        unloaded.label_names_load([])
        model.load(ids)
        want = model.events(ids, values)
        outs = []
        for s in (never, unloaded):
            s.load_pod_ids(ids)
            s.profile(True)
            outs.append(s.pods_events_json(ids, values))
            assert s.last_kernel_ms() > 0
            outs[-1] += s.ingest_pods_json(values[::-1], np.arange(len(values)))
            assert s.last_kernel_ms() > 0
            assert not s.pod_labels_get()[0].any() and not s.pod_labels_get()[1].any()
        for a, b in zip(*outs):
            assert np.array_equal(a, b)
        for g, w in zip(outs[0][:3], want[:3]):
            assert np.array_equal(g, w)
        assert np.array_equal(never.get_pods(), unloaded.get_pods())
        # a wrong-typed `labels` is a skipped field here: accepted
        wrong = [pc.rec('"labels":' + shape) for shape in pc.REJECTED if shape not in pc.JSON_REFUSES]
        for s in (never, unloaded):
            status, _, _, _ = s.pods_events_json(ids[:len(wrong)], wrong)
            assert not status.any()
        # ... and with names loaded the same call is a second launch inside the same device span, and rejects them
        unloaded.label_names_load(pc.NAMES)
        status, _, _, _ = unloaded.pods_events_json(ids[:len(wrong)], wrong)
        assert status.all() and unloaded.last_kernel_ms() > 0
    finally:
        never.close()
        unloaded.close()


def test_state_rules():
    ids = ["aaaaaa-1", "bbbbbb-1", "cccccc-1"]
    p = _fresh(ids, sentinel=False)
    try:
        p.events("start", ids, [pc.rec('"labels":["gpu"]'), pc.rec('"labels":["zone-a","q"]'), pc.rec('"labels":["label-63"]')])
        # a join inside the events call and an append: zero words
        p.events("join", ["dddddd-1", "dddddd-1", "eeeeee-1"], [pc.rec('"labels":[1]'), pc.rec('"labels":["gpu",""]'), pc.rec('"labels":"x"')])
        p.s.append_pod_ids(["ffffff-1"])
        p.m.append(["ffffff-1"])
        p.state("append")
        assert list(p.s.pod_labels_get()[0]) == [pc.GPU, pc.ZONE, 1 << 63, pc.GPU | pc.EMPTY, 0, 0]
        # set: all or nothing on a bad index
        before = [a.copy() for a in p.s.pod_labels_get()]
        for bad in ([1, 6], [-1, 1]):
            with pytest.raises(MmpError) as e:
                p.s.pod_labels_set(bad, [7, 7], [1, 1])
            assert e.value.code == _lib.MMP_EINVAL
        with pytest.raises(MmpError):
            p.s.pod_labels_set([1], [7], [-2])
        for a, b in zip(p.s.pod_labels_get(), before):
            assert np.array_equal(a, b)
        p.set([5, 1], [9, 10], [2, 3])
        p.state("set")
        # upsert and remove leave the words alone; a deleted event too
        rows = p.s.get_pods()
        p.s.upsert_pods(np.array([1], np.int32), rows[1:2])
        p.s.remove_pods(np.array([0], np.int32))
        p.m.rows["flags"][0] = (p.m.rows["flags"][0] | _lib.POD_TOMBSTONE) & ~np.uint32(_lib.POD_LIVE)
        p.events("deleted", ["bbbbbb-1"], [""], deleted=[1])
        assert list(p.s.pod_labels_get()[0]) == [pc.GPU, 10, 1 << 63, pc.GPU | pc.EMPTY, 0, 9]
        # a too-small and a NULL buffer on get
        n, words, counts = C.c_int32(0), np.full(2, 77, np.uint64), np.full(8, 77, np.int32)
        assert p.s.lib.mmp_pod_labels_get(p.s.h, _lib.ptr(words), None, 2, C.byref(n)) == 0
        assert n.value == 6 and list(words) == [pc.GPU, 10]
        assert p.s.lib.mmp_pod_labels_get(p.s.h, None, _lib.ptr(counts), 8, C.byref(n)) == 0
        assert n.value == 6 and list(counts) == [1, 3, 1, 2, 0, 2, 77, 77]
        assert p.s.lib.mmp_pod_labels_get(p.s.h, None, None, 0, C.byref(n)) == 0 and n.value == 6
        assert p.s.lib.mmp_pod_labels_get(p.s.h, None, None, 0, None) == _lib.MMP_EINVAL
        # refused name tables change nothing: the words stay and the old names still parse
        for bad in (["l%d" % i for i in range(65)], ["a", "b", "a"], ['a"b'], ["a\\b"], ["a\x01"]):
            with pytest.raises(MmpError) as e:
                p.s.label_names_load(bad)
            assert e.value.code == _lib.MMP_EINVAL
        p.state("refused names")
        p.events("old names", ["eeeeee-1"], [pc.rec('"labels":["label-4","größe-µ"]')])
        assert p.s.pod_labels_get()[0][4] == pc.L4 | pc.UTF
        # mmp_pods_load keeps the words of the indices that remain and zeroes new ones
        rows = p.s.get_pods()
        p.s.load_pods(rows[:4].copy())
        p.m.rows_load(rows[:4])
        p.state("rows load, shorter")
        p.s.load_pods(np.concatenate([rows[:4], rows[:3]]))
        p.m.rows_load(np.concatenate([rows[:4], rows[:3]]))
        p.state("rows load, longer")
        assert list(p.s.pod_labels_get()[0]) == [pc.GPU, 10, 1 << 63, pc.GPU | pc.EMPTY, 0, 0, 0]
        # a second names load clears every word (the bits change meaning) and the new order holds
        p.s.n_pods = 7
        p.names(["zone-a", "gpu"])
        p.state("second names load")
        assert not p.s.pod_labels_get()[0].any() and not p.s.pod_labels_get()[1].any()
        p.load_ids(ids)
        p.events("new order", ids[:1], [pc.rec('"labels":["gpu","label-4"]')])
        assert (p.s.pod_labels_get()[0][0], p.s.pod_labels_get()[1][0]) == (2, 2)
        # mmp_pod_ids_load clears all words
        p.load_ids(ids + ["gggggg-1"])
        p.state("ids load")
        assert not p.s.pod_labels_get()[0].any()
        # n_labels = 0 unloads: words cleared, labels a skipped field again
        p.set([2], [5], [1])
        p.names([])
        p.state("unloaded")
        assert not p.s.pod_labels_get()[0].any()
        (status, _, _, _), _ = p.events("no table", ids[:1], [pc.rec('"labels":7')])
        assert status[0] == 0 and not p.s.pod_labels_get()[1].any()
        assert not p.diffs, p.diffs[:8]
    finally:
        p.close()


def test_the_four_natives_through_the_veneer(tmp_path):
    """labelNamesLoad / podsEventsJson / podLabelsGet / podLabelsSet / typesFromPodLabels under the mock JVM give what the C ABI
    gives; a short direct buffer is refused before the library sees it."""
    from tests import jni_mock as jm
    from tests.test_jni_veneer import _java_natives
    v = jm.Veneer(jm.build(tmp_path), _java_natives())
    bb = lambda a, dtype=None: jm.ByteBuffer(np.ascontiguousarray(a, dtype=dtype))  # noqa: E731
    ids = ["aaaaaa-1", "bbbbbb-1", "cccccc-1"]
    values = [pc.rec('"labels":["gpu","zone-a"]'), pc.rec('"labels":[1]'), pc.rec('"labels":["x",""]')]
    s = Solver(100, 1000)
    h = v.call("create", 0, 100, 1000)
    try:
        assert h and v.env.pending() is None
        names, noff = Solver._pack(pc.NAMES)
        idb, ioff = Solver._pack(ids)
        vb, voff = Solver._pack(values)
        u8 = lambda b: np.frombuffer(b, np.uint8).copy()  # noqa: E731
        assert v.call("labelNamesLoad", h, bb(u8(names)), bb(noff, np.int32), len(pc.NAMES)) == 0
        assert v.call("podIdsLoad", h, bb(u8(idb)), bb(ioff, np.int32), 3, None, None) == 0
        idx, st, status, napp = bb(np.zeros(3, np.int32)), bb(np.zeros(3, np.int64)), bb(np.zeros(3, np.int32)), bb(np.zeros(1, np.int32))
        assert v.call("podsEventsJson", h, bb(u8(idb)), bb(ioff, np.int32), bb(u8(vb)), bb(voff, np.int64), 3, None, None, 1, idx, st,
                      status, napp) == 0 and v.env.pending() is None
        s.label_names_load(pc.NAMES)
        s.load_pod_ids(ids)
        want = s.pods_events_json(ids, values)
        assert np.array_equal(status.arr, want[0]) and list(status.arr) == [0, 1, 0]
        words, counts, n = bb(np.zeros(3, np.uint64)), bb(np.zeros(3, np.int32)), bb(np.zeros(1, np.int32))
        assert v.call("podLabelsGet", h, words, counts, 3, n) == 0 and int(n.arr[0]) == 3
        assert np.array_equal(words.arr, s.pod_labels_get()[0]) and list(words.arr) == [pc.GPU | pc.ZONE, 0, pc.EMPTY]
        assert np.array_equal(counts.arr, s.pod_labels_get()[1]) and list(counts.arr) == [2, 0, 2]
        assert v.call("podLabelsSet", h, bb([1], np.int32), bb([pc.GPU], np.uint64), bb([1], np.int32), 1) == 0
        s.pod_labels_set([1], [pc.GPU], [1])
        req, pref = np.array([pc.GPU, pc.ZONE], np.uint64), np.array([0, pc.EMPTY], np.uint64)
        al, pf, ha, hp = bb(np.zeros((3, 1), np.uint64)), bb(np.zeros((3, 1), np.uint64)), bb(np.zeros(3, np.uint8)), bb(np.zeros(3, np.uint8))
        assert v.call("typesFromPodLabels", h, 2, bb(req), bb(pref), al, pf, ha, hp) == 0 and v.env.pending() is None
        for got, w in zip((al, pf, ha, hp), s.types_from_pod_labels(req, pref)):
            assert np.array_equal(got.arr.reshape(w.shape), w)
        assert v.call("podLabelsGet", h, bb(np.zeros(1, np.uint64)), None, 3, n) != 0  # wordsOut shorter than maxPods
        assert v.env.pending() is not None
        v.env.clear()
    finally:
        v.call("destroy", h)
        s.close()
