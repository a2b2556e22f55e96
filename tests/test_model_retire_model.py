"""tests/model_retire_model.py on cases worked by hand — the model is the oracle of the retire kernels, so its own rules are pinned
here without a device — and the entry point of the C ABI, which must exist and refuse a NULL context."""
import ctypes as C

import numpy as np
import pytest

from modelmesh_amd import _lib
from tests.model_events_model import EMPTY, ModelEventsModel
from tests.model_retire_model import retire

IDS = [b"a", b"b", b"", b"d-\xff", b"e"]


def make(n=5):
    m = ModelEventsModel(["pod-0", "pod-1"], ["T0", "T1"], 0)
    m.recs = [(i % 2, 100 + i, ((0, 10 + i),) * (i % 3), ((1, 20 + i),) * (i % 2)) for i in range(n)]
    m.load(IDS[:n])
    return m


CASES = [
    ("nothing", [], [0, 1, 2, 3, 4]),
    ("everything", [0, 1, 2, 3, 4], [-1] * 5),
    ("first", [0], [-1, 0, 1, 2, 3]),
    ("last", [4], [0, 1, 2, 3, -1]),
    ("neighbours", [1, 2], [0, -1, -1, 1, 2]),
    ("twice", [3, 3], [0, 1, 2, -1, 3]),
    ("out of order", [4, 0, 2], [-1, 0, -1, 1, -1]),
]


@pytest.mark.parametrize("name,rows,want", CASES, ids=[c[0] for c in CASES])
def test_hand_worked(name, rows, want):
    m = make()
    recs0 = list(m.recs)
    remap = retire(m, rows)
    assert remap.dtype == np.int32 and list(remap) == want
    kept = [r for r in range(5) if want[r] >= 0]
    assert m.ids == [IDS[r] for r in kept] and m.get() == m.ids
    assert m.recs == [recs0[r] for r in kept] and m.n_models == len(kept)
    assert list(m.resolve(IDS)) == want  # a retired id is unknown, a survivor answers its new row


def test_without_ids_only_the_registry_is_compacted():
    m = ModelEventsModel()
    m.recs = [(0, i, (), ()) for i in range(4)]
    assert list(retire(m, [1])) == [0, -1, 1, 2] and [r[1] for r in m.recs] == [0, 2, 3] and m.ids is None


def test_refusals_change_nothing():
    m = make()
    ids0, recs0 = list(m.ids), list(m.recs)
    for rows in ([-1], [5], [0, 7]):
        with pytest.raises(ValueError):
            retire(m, rows)
    m.recs.append(EMPTY)  # an append by index: the id count is out of step
    with pytest.raises(RuntimeError):
        retire(m, [0])
    m.recs.pop()
    assert m.ids == ids0 and m.recs == recs0 and m.index == {s: i for i, s in enumerate(ids0)}


def test_empty_only():
    m = make()
    m.events([b"b", b"d-\xff"], ["", ""], np.array([1, 1], np.uint8))  # two deletions
    assert m.recs[1] == EMPTY and m.recs[3] == EMPTY
    snap = (list(m.ids), list(m.recs))
    with pytest.raises(ValueError, match="row 2 "):  # a row with entries (rows 2 and 4 have some: the lowest is named)
        retire(m, [4, 1, 2], empty_only=True)
    m.recs[3] = (0, 77, (), ())  # registered again without copies: no entries, a non-zero last_used
    snap = (list(m.ids), list(m.recs))
    with pytest.raises(ValueError, match="row 3 "):
        retire(m, [1, 3], empty_only=True)
    m.recs[3] = (1, 0, (), ())  # ... or only a type
    with pytest.raises(ValueError, match="row 3 "):
        retire(m, [3], empty_only=True)
    m.recs[3] = snap[1][3]
    assert (m.ids, m.recs) == snap
    assert list(retire(m, [1], empty_only=True)) == [0, -1, 1, 2, 3]
    assert list(retire(m, [2], empty_only=False)) == [0, 1, -1, 2]  # without the flag a full row goes as well


def test_a_retired_id_joins_again_at_the_end():
    m = make()
    retire(m, [1])
    value = '{"type":"T1","lastUsed":5}'
    st, idx, _, n_app = m.events([b"b", b"b", b"e"], [value, "", value], np.array([0, 1, 0], np.uint8), append=False)
    assert list(st) == [2, 2, 0] and list(idx) == [-1, -1, 3] and n_app == 0  # unknown like any other id
    st, idx, _, n_app = m.events([b"b"], [value], None, append=True)
    assert list(st) == [0] and list(idx) == [4] and n_app == 1
    assert m.ids == [b"a", b"", b"d-\xff", b"e", b"b"] and list(m.resolve([b"b"])) == [4]


def test_the_entry_point_exists_and_refuses_a_null_context():
    L = _lib.load()
    EINVAL = -1  # MMP_EINVAL
    n = C.c_int32(7)
    rows = np.zeros(1, np.int32)
    assert _lib.RETIRE_EMPTY_ONLY == 1
    assert L.mmp_models_retire(None, _lib.ptr(rows), 1, 0, None, 0, C.byref(n)) == EINVAL
    assert L.mmp_models_retire(None, None, 0, _lib.RETIRE_EMPTY_ONLY, None, 0, None) == EINVAL
    assert n.value == 7
