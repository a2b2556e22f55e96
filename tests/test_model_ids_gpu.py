"""The model-id table on the device (mmp_model_ids_load / _resolve / _get): a load of A followed by events that make B join must
leave what a load of A + B leaves — every id resolves alike, ids in neither set give -1, mmp_model_ids_get gives the ids back —
across the table's capacity edges (16 slots for up to 8 ids, doubling whenever the ids outgrow half of it), with the full hash
and with the hash masked so that ids collide.  Everything is exact."""
import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd.solver import MmpError, Solver
from tests.model_events_fixtures import make_model_ids

pytestmark = pytest.mark.gpu

EDGES = [(0, 0), (0, 1), (1, 0), (1, 1), (7, 1), (7, 2), (8, 1), (0, 9), (63, 1), (63, 2), (64, 1), (0, 65), (65, 0), (255, 1), (255, 2),
         (256, 1), (1, 256), (0, 257)]


def _ctx(n_rows):
    s = Solver(100, 1000)
    s.load_pod_ids(["aaaaaa-1"])
    s.load_models(np.zeros(n_rows, _lib.MODEL_ROW), np.zeros(0, np.int32), np.zeros(0, np.int64))
    return s


def _equivalent(na, nb, seed):
    rng = np.random.default_rng(100 * na + nb + seed)
    ids = make_model_ids(rng, na + nb + 6)
    A, B, others = ids[:na], ids[na:na + nb], ids[na + nb:]
    s1, s2 = _ctx(na), _ctx(na + nb)
    try:
        s1.model_ids_load(A)
        assert list(s1.model_ids_resolve(A + B)) == list(range(na)) + [-1] * nb
        if nb:
            # B joins in two calls where it can, with a repeat and a deletion of a still unknown id in front
            cut = nb // 2
            for part in (B[:cut], B[cut:]):
                if not part:
                    continue
                keys = [part[-1]] + part + [part[0]]
                dele = [1] + [0] * len(part) + [0]
                st, idx, _, n_app = s1.models_events_json(keys, ["{}"] * len(keys), dele)
                assert n_app == len(part) and st[0] == 2 and not st[1:].any() and idx[0] == -1
        s2.model_ids_load(A + B)
        ask = A + B + others
        want = list(range(na + nb)) + [-1] * len(others)
        order = rng.permutation(len(ask))
        for s in (s1, s2):
            got = s.model_ids_resolve([ask[i] for i in order])
            assert list(got) == [want[i] for i in order]
            assert s.n_models == na + nb and s.model_ids_get() == A + B
            assert s.model_ids_get(na, nb) == B and s.model_ids_get(0, na) == A and s.model_ids_get(na + nb, 0) == []
    finally:
        s1.close()
        s2.close()


@pytest.mark.parametrize("na,nb", EDGES)
def test_load_then_join_equals_one_load(na, nb):
    _equivalent(na, nb, 0)


@pytest.mark.parametrize("bits", [0, 4])
@pytest.mark.parametrize("na,nb", [(0, 9), (7, 2), (200, 100)])
def test_the_same_when_ids_collide(monkeypatch, bits, na, nb):
    """MMP_MODEL_ID_HASH_BITS is read per context: every id of these contexts shares one hash (0 bits) or one of sixteen (4)."""
    monkeypatch.setenv("MMP_MODEL_ID_HASH_BITS", str(bits))
    _equivalent(na, nb, 1)


def test_load_refusals_change_nothing():
    ids = [b"a", b"bb", b"", "é".encode()]
    s = _ctx(4)
    try:
        L = s.lib
        out = np.full(4, -7, np.int32)
        off = np.array([0, 1, 3, 3, 5], np.int32)
        blob = b"".join(ids)
        assert L.mmp_model_ids_resolve(s.h, blob, _lib.ptr(off), 4, _lib.ptr(out)) == _lib.MMP_ESTATE  # before the load
        nb = _lib.C.c_int32(0)
        assert L.mmp_model_ids_get(s.h, 0, 0, None, 0, None, _lib.C.byref(nb)) == _lib.MMP_ESTATE
        with pytest.raises(MmpError) as e:
            s.model_ids_load(ids[:3])  # 3 ids for 4 rows
        assert e.value.code == _lib.MMP_ESTATE
        s.model_ids_load(ids)

        def same():
            assert list(s.model_ids_resolve(ids + [b"zz"])) == [0, 1, 2, 3, -1] and s.model_ids_get() == ids

        same()
        for bad in ([b"a", b"bb", b"a", b"c"], [b"", b"x", b"y", b""]):
            with pytest.raises(MmpError) as e:
                s.model_ids_load(bad)
            assert e.value.code == _lib.MMP_EINVAL and "equal" in str(e.value)
            same()
        assert L.mmp_model_ids_load(s.h, blob, None, 4) == _lib.MMP_EINVAL
        assert L.mmp_model_ids_load(s.h, blob, _lib.ptr(np.array([0, 2, 1, 3, 5], np.int32)), 4) == _lib.MMP_EINVAL  # not monotone
        assert L.mmp_model_ids_load(s.h, None, _lib.ptr(off), 4) == _lib.MMP_EINVAL
        assert L.mmp_model_ids_resolve(s.h, blob, None, 4, _lib.ptr(out)) == _lib.MMP_EINVAL
        assert L.mmp_model_ids_resolve(s.h, blob, _lib.ptr(off), 4, None) == _lib.MMP_EINVAL
        assert L.mmp_model_ids_resolve(s.h, blob, _lib.ptr(off), 0, None) == _lib.MMP_OK  # n == 0 is valid
        assert L.mmp_model_ids_get(s.h, 2, 3, None, 0, None, _lib.C.byref(nb)) == _lib.MMP_EINVAL  # rows 2 .. 4 of 4
        assert L.mmp_model_ids_get(s.h, -1, 1, None, 0, None, _lib.C.byref(nb)) == _lib.MMP_EINVAL
        assert L.mmp_model_ids_get(s.h, 0, 4, None, 0, None, None) == _lib.MMP_EINVAL
        assert np.all(out == -7)
        same()
        # the sizes-only form, and a buffer that is too small: the count, no bytes
        got_off, small = np.full(5, -7, np.int32), np.full(8, 0x55, np.uint8)
        assert L.mmp_model_ids_get(s.h, 0, 4, None, 0, _lib.ptr(got_off), _lib.C.byref(nb)) == 0 and nb.value == 5
        assert list(got_off) == [0, 1, 3, 3, 5]
        assert L.mmp_model_ids_get(s.h, 1, 3, _lib.ptr(small), 3, None, _lib.C.byref(nb)) == 0 and nb.value == 4 and np.all(small == 0x55)
        assert L.mmp_model_ids_get(s.h, 1, 3, _lib.ptr(small), 8, _lib.ptr(got_off), _lib.C.byref(nb)) == 0
        assert small[:4].tobytes() == b"bb" + "é".encode() and list(got_off[:4]) == [0, 2, 2, 4]
        # a second load replaces the table
        s.model_ids_load(ids[::-1])
        assert list(s.model_ids_resolve(ids)) == [3, 2, 1, 0] and s.model_ids_get() == ids[::-1]
    finally:
        s.close()
