"""tests/vmodel_retire_model.py on cases worked by hand — the model is the oracle of the vmodel retire kernels, so its own rules
are pinned here without a device: the remap, ALL_ABSENT, ABSENT_ONLY, the refusals, and that events, resolve and transitions after
a retire are those of a table that was fed only the survivors (vmodel numbers compared through the remap)."""
import numpy as np
import pytest

from tests import vmodel_fixtures as fx
from tests import vmodel_model as vm
from tests.vmodel_retire_model import retire, through

IDS = [b"a", b"b", b"", b"d-\xff", b"e"]
VALUES = [vm.render("m1", "m1", "o"), vm.render("m1", "m2"), vm.render(None, "m3"), vm.render("", "", ""), vm.render("x\\y", "m1")]


def make(n=5):
    m = vm.VModels()
    m.events(IDS[:n], VALUES[:n])
    return m


CASES = [
    ("nothing", [], [0, 1, 2, 3, 4]),
    ("everything", [0, 1, 2, 3, 4], [-1] * 5),
    ("first", [0], [-1, 0, 1, 2, 3]),
    ("last", [4], [0, 1, 2, 3, -1]),
    ("neighbours", [1, 2], [0, -1, -1, 1, 2]),
    ("twice", [3, 3], [0, 1, 2, -1, 3]),
    ("out of order, twice", [4, 0, 2, 0, 4], [-1, 0, -1, 1, -1]),
]


@pytest.mark.parametrize("name,rows,want", CASES, ids=[c[0] for c in CASES])
def test_hand_worked(name, rows, want):
    m = make()
    ids0, rows0, same = m.ids, list(m.rows), (m.ids, m.rows, m.row_of)
    remap, n_after = retire(m, rows)
    assert remap.dtype == np.int32 and list(remap) == want
    kept = [r for r in range(5) if want[r] >= 0]
    assert n_after == len(kept) == len(m.rows)
    assert (m.ids, m.rows, m.row_of) == same and all(a is b for a, b in zip((m.ids, m.rows, m.row_of), same))  # rewritten in place
    assert ids0 == [IDS[r] for r in kept] and m.rows == [rows0[r] for r in kept]
    assert m.row_of == {IDS[r]: want[r] for r in kept}
    reg = vm.Registry([b"m1", b"m2", b"m3"], [(1, 0, 5, 0), (0, 0, 0, 0), (0, 1, 7, 0)])
    assert [a.vmodel for a in m.resolve_many(reg, IDS)] == want  # a retired id is unknown, a survivor answers its new row


def test_rows_none_is_the_empty_list():
    m = make()
    remap, n_after = retire(m)
    assert list(remap) == [0, 1, 2, 3, 4] and n_after == 5
    assert retire(vm.VModels())[1] == 0 and len(retire(vm.VModels(), [])[0]) == 0  # before the first vmodel call: V0 == 0
    assert retire(vm.VModels(), all_absent=True)[1] == 0


def test_all_absent_at_the_front_in_the_middle_and_at_the_end():
    ids = [b"v%d" % k for k in range(9)]
    m = vm.VModels()
    m.events(ids, [vm.render("m%d" % k, "m1") for k in range(9)])
    m.events([ids[k] for k in (0, 1, 4, 6, 8)], [""] * 5, np.ones(5, np.uint8))
    assert [r is None for r in m.rows] == [True, True, False, False, True, False, True, False, True]
    with pytest.raises(ValueError):
        retire(m, [0], all_absent=True)  # a list beside the flag
    with pytest.raises(ValueError):
        retire(m, [2], absent_only=True, all_absent=True)
    assert len(m.rows) == 9
    remap, n_after = retire(m, all_absent=True, absent_only=True)  # (ABSENT_ONLY beside it adds nothing)
    assert list(remap) == [-1, -1, 0, 1, -1, 2, -1, 3, -1] and n_after == 4
    assert m.ids == [ids[k] for k in (2, 3, 5, 7)] and all(r is not None for r in m.rows)
    remap, n_after = retire(m, all_absent=True)  # a second call is the identity
    assert list(remap) == [0, 1, 2, 3] and n_after == 4


def test_absent_only():
    m = make()
    m.events([b"b", b"d-\xff"], ["", ""], np.array([1, 1], np.uint8))
    snap = (list(m.ids), list(m.rows), dict(m.row_of))
    with pytest.raises(ValueError, match="row 2 "):  # rows 2 and 4 are set: the lowest is named
        retire(m, [4, 1, 2], absent_only=True)
    m.events([b"d-\xff"], [vm.render("again", "again")])  # set again in between
    with pytest.raises(ValueError, match="row 3 "):
        retire(m, [1, 3], absent_only=True)
    m.events([b"d-\xff"], [""], [1])
    assert (m.ids, m.rows, m.row_of) == snap
    assert list(retire(m, [1], absent_only=True)[0]) == [0, -1, 1, 2, 3]
    assert list(retire(m, [0])[0]) == [-1, 0, 1, 2]  # without the flag a set row goes as well


def test_refusals_change_nothing():
    m = make()
    snap = (list(m.ids), list(m.rows), dict(m.row_of))
    for kw in (dict(rows=[-1]), dict(rows=[5]), dict(rows=[0, 7]), dict(rows=[0], all_absent=True), dict(rows=[0], absent_only=True)):
        with pytest.raises(ValueError):
            retire(m, **kw)
        assert (m.ids, m.rows, m.row_of) == snap, kw


def test_a_retired_id_joins_again_at_the_end():
    m = make()
    retire(m, [1])
    st, idx, n_app = m.events([b"b", b"b", b"e"], [VALUES[1], "", VALUES[4]], np.array([0, 1, 0], np.uint8), append=False)
    assert list(st) == [2, 2, 0] and list(idx) == [-1, -1, 3] and n_app == 0  # unknown like any other id
    st, idx, n_app = m.events([b"b"], [VALUES[1]], None, append=True)
    assert list(st) == [0] and list(idx) == [4] and n_app == 1
    assert m.ids == [b"a", b"", b"d-\xff", b"e", b"b"]


@pytest.mark.parametrize("n_vm,pattern", [(65, "third"), (65, "first half"), (257, "third"), (17, "last")])
def test_after_a_retire_the_table_is_that_of_its_survivors(n_vm, pattern):
    mids = fx.model_ids(64)
    reg = vm.Registry(mids, fx.registry_values(["pod-%d" % i for i in range(8)], 64)[1])
    keys, values, deleted = fx.scenario(n_vm, mids)
    m = vm.VModels()
    m.events(keys, values, deleted)
    v0 = len(m.rows)
    rows = {"third": list(range(0, v0, 3)), "first half": list(range(v0 // 2)), "last": [v0 - 1]}[pattern]
    old_ids = list(m.ids)
    old_answers = m.resolve_many(reg, old_ids)
    old_trans = m.transitions(reg, fx.NOW, fx.AGE)[0]
    remap, n_after = retire(m, rows)
    # a table that only ever saw the survivors' events
    gone = {old_ids[r] for r in rows}
    keep = [i for i, k in enumerate(keys) if k not in gone]
    fresh = vm.VModels()
    fresh.events([keys[i] for i in keep], [values[i] for i in keep], deleted[keep])
    assert (m.ids, m.rows, m.row_of) == (fresh.ids, fresh.rows, fresh.row_of) and n_after == len(fresh.rows)
    # the questions, the retired ids among them
    qk, nf, ow, fl = fx.questions(fresh, extra_ids=tuple(sorted(gone)) + (b"never-seen",))
    assert m.resolve_many(reg, qk, nf, ow, fl) == fresh.resolve_many(reg, qk, nf, ow, fl)
    assert all(a.cls == vm.NOT_FOUND and a.vmodel == -1 for a in m.resolve_many(reg, sorted(gone)))
    # what the host held from before, renumbered
    new_answers = m.resolve_many(reg, old_ids)
    for old, new in zip(through(remap, old_answers), new_answers):
        assert old is None or old == new
    assert [t for t in through(remap, old_trans) if t is not None] == m.transitions(reg, fx.NOW, fx.AGE)[0]
    # and the same events afterwards
    more_k = old_ids[:10] + [b"brand-new"]
    more_v = [vm.render("m1", "m4-x", "late")] * 11
    for append in (False, True):
        got, want = m.events(more_k, more_v, None, append), fresh.events(more_k, more_v, None, append)
        assert all(np.array_equal(g, w) for g, w in zip(got[:2], want[:2])) and got[2] == want[2]
    assert (m.ids, m.rows) == (fresh.ids, fresh.rows)
