"""mmp_vmodels_retire on the device held to tests/vmodel_retire_model.py: after a retire the table is, in everything the calls
return, the table of a fresh context that got the survivors as one append batch — ids, flags, strings, capacity, a squeezed arena —
and the remap is the model's.  The fleet, the registry and the helpers are those of tests/test_vmodels_gpu.py; every table is
small (at most 300 rows over 64 or 300 models)."""
import threading

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd.solver import MmpError
from tests import vmodel_fixtures as fx
from tests import vmodel_model as vm
from tests import vmodel_retire_model as vrm
from tests.test_vmodels_gpu import (FILL, M, MIDS, REG_VALUES, WORLD, answers, check_questions, check_table, check_transitions, registry_of,
                                    send, start, tab_capacity)

pytestmark = pytest.mark.gpu

MIDS64 = MIDS[:64]
FILL_WORD = int(np.full(4, FILL, np.uint8).view(np.int32)[0])
LONG = "L" * 5000


def value_for(k):
    """Row k of the scenario, kind k % 10: each of amid, tmid and o null, each of them "", a backslash (HOST), `failed`, and in row 8
    one string of 5 000 bytes."""
    a, t = MIDS64[1 + k % 63].decode(), MIDS64[1 + (k + 7) % 63].decode()
    owner = "owner-%d" % k
    kind = k % 10
    if kind == 1:
        return vm.render(None, t, owner)
    if kind == 2:
        return vm.render(a, None, owner)
    if kind == 3:
        return vm.render(a, a, None)
    if kind == 4:
        return vm.render("", t, owner)
    if kind == 5:
        return vm.render(a, "", owner)
    if kind == 6:
        return vm.render(a, a, "")
    if kind == 7:
        return vm.render("esc\\aped-%d" % k, t, owner)
    if kind == 8:
        return vm.render(a, a, LONG if k == 8 else owner)
    if kind == 9:
        return vm.render(a, t, owner, failed=True)
    return vm.render(a, t, owner)


def build(s, m, v0, tag=b"rt"):
    """v0 rows, then a second batch that deletes the rows k % 7 == 3 and rewrites the rows k % 5 == 0 with longer values: ABSENT
    rows, and garbage in the arena that stays below the squeeze threshold."""
    ids = fx.vmodel_ids(v0, tag)
    send(s, m, ids, [value_for(k) for k in range(v0)])
    dele = [k for k in range(v0) if k % 7 == 3]
    upd = [k for k in range(v0) if k % 5 == 0 and k % 7 != 3]
    send(s, m, [ids[k] for k in dele + upd], [""] * len(dele) + [vm.render("upd-%d" % k, MIDS64[2].decode(), "owner-%d-updated" % k) for k in upd],
         np.array([1] * len(dele) + [0] * len(upd), np.uint8))
    info = s.vmodels_info()
    assert info["arena_bytes"] > info["live_bytes"] == m.info()[2], info  # garbage, not squeezed
    return ids


def raw_value(row):
    """The stored value of a model Row from its raw bytes; an ABSENT row as a value that is malformed (a joining id whose events
    are all malformed is ABSENT)."""
    if row is None:
        return b"{"
    parts = [b'"%s":"%s"' % (name, s) for name, s in ((b"amid", row.amid), (b"tmid", row.tmid), (b"o", row.owner)) if s is not None]
    if row.failed:
        parts.append(b'"failed":true')
    return b"{" + b",".join(parts) + b"}"


def table(s):
    ids, flags, strings = s.vmodels_get()
    return ids, flags.tobytes(), strings


def state(s, keys):
    """Everything the read calls return, as bytes."""
    rows, info = s.vmodels_transitions(fx.NOW, fx.AGE)
    return [table(s), s.vmodels_info().tobytes(), s.vmodels_resolve(keys).tobytes() if keys else b"", rows.tobytes(), info.tobytes()]


def retire_both(s, m, rows=None, what="", **kw):
    want, n_want = vrm.retire(m, rows, **kw)
    remap, n_after = s.vmodels_retire(rows, **kw)
    assert np.array_equal(remap, want) and n_after == n_want, (what, remap[:16], want[:16], n_after, n_want)
    return remap


def pattern_rows(pattern, v0):
    return {"third": list(range(0, v0, 3)), "first half": list(range((v0 + 1) // 2)), "last": [v0 - 1], "all": list(range(v0))[::-1],
            "none": []}[pattern]


def check_squeezed(s, what=""):
    info = s.vmodels_info()
    assert info["arena_bytes"] == info["live_bytes"], (what, info)


# ---- retire equals a fresh table of the survivors ------------------------------------------------------------------------------

def test_the_scenario_holds_what_it_must():
    m = vm.VModels()
    ids = fx.vmodel_ids(17, b"rt")
    m.events(ids, [value_for(k) for k in range(17)])
    rows = m.rows
    for f in ("amid", "tmid", "owner"):
        assert any(getattr(r, f) is None for r in rows) and any(getattr(r, f) == b"" for r in rows), f
    assert any(r.host for r in rows) and any(r.failed for r in rows) and len(rows[8].owner) == 5000
    assert (17 + 1) // 2 == 9 and tab_capacity(17) == 64 and tab_capacity(8) == 16  # 17 rows to 8: two capacities down


@pytest.mark.parametrize("pattern", ["third", "first half", "last", "all", "none"])
@pytest.mark.parametrize("v0", [1, 2, 17, 63, 64, 65, 257, 300])
def test_retire_equals_a_fresh_table_of_the_survivors(v0, pattern):
    s, fresh, m = WORLD.solver(), WORLD.solver(), vm.VModels()
    try:
        build(s, m, v0)
        rows = pattern_rows(pattern, v0)
        before = s.vmodels_info().tobytes()
        absent0 = [r is None for r in m.rows]
        remap = retire_both(s, m, rows + rows[:1])  # (the first one named twice)
        assert len(m.rows) == v0 - len(rows)
        if v0 >= 17 and pattern in ("third", "first half"):
            assert any(r is None for r in m.rows) and any(absent0[r] for r in rows)  # ABSENT rows stay, and leave
        check_table(s, m)
        if rows:
            check_squeezed(s)
        else:
            assert s.vmodels_info().tobytes() == before and list(remap) == list(range(v0))  # nothing changed: no squeeze
        if m.ids:
            st, idx, n_app = fresh.vmodels_events_json(m.ids, [raw_value(r) for r in m.rows])
            assert n_app == len(m.ids) and list(idx) == list(range(len(m.ids))) and [x != 0 for x in st] == [r is None for r in m.rows]
        assert table(s) == table(fresh)
        a, b = s.vmodels_info(), fresh.vmodels_info()
        assert (a["capacity"], a["n_rows"], a["n_live"], a["live_bytes"]) == (b["capacity"], b["n_rows"], b["n_live"], b["live_bytes"])
        assert a["capacity"] == (tab_capacity(len(m.ids)) if m.ids else 0)
    finally:
        s.close()
        fresh.close()


# ---- questions after a retire ---------------------------------------------------------------------------------------------------

def questions_about(s, m, extra, what=""):
    reg = registry_of(s)
    keys, nf, owners, flags = fx.questions(m, extra_ids=tuple(extra) + (b"never-seen", b""))
    got = s.vmodels_resolve(keys, nf, owners, flags)
    want = m.resolve_many(reg, keys, nf, owners, flags)
    bad = [i for i, (g, w) in enumerate(zip(answers(got), want)) if g != tuple(w)]
    assert not bad, (what, bad[:5], keys[bad[0]], answers(got)[bad[0]], want[bad[0]])


@pytest.mark.parametrize("pattern", ["third", "first half"])
def test_questions_after_a_retire(pattern):
    s, m = start(64), vm.VModels()
    try:
        send(s, m, *fx.scenario(65, MIDS64))
        old_ids = list(m.ids)
        old = [vm.Transition(*t) for t in answers(check_transitions(s, m, "before"))]
        rows = pattern_rows(pattern, len(old_ids))
        remap = retire_both(s, m, rows)
        gone = [old_ids[r] for r in rows]
        check_table(s, m)
        check_questions(s, m)
        questions_about(s, m, gone)
        a = s.vmodels_resolve(gone)
        assert (a["cls"] == vm.NOT_FOUND).all() and (a["vmodel"] == -1).all()
        assert list(s.vmodels_resolve(m.ids)["vmodel"]) == [-1 if r is None else i for i, r in enumerate(m.rows)]
        new = [vm.Transition(*t) for t in answers(check_transitions(s, m, "after"))]
        assert new == [t for t in vrm.through(remap, old) if t is not None] and 0 < len(new) < len(old)
    finally:
        s.close()


# ---- when ids collide -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("v0", [9, 65, 300])
@pytest.mark.parametrize("bits", [0, 4])
def test_when_ids_collide(monkeypatch, bits, v0):
    monkeypatch.setenv("MMP_VMODEL_ID_HASH_BITS", str(bits))
    s, m = start(64), vm.VModels()
    try:
        special = [b"pair-a", b"pair-b", b"pre", b"prefix-long"]
        ids = fx.vmodel_ids(v0 - 4, b"col")
        ids = ids[:2] + special[:2] + ids[2:] + special[2:]
        send(s, m, ids, [value_for(k) for k in range(v0)])
        rows = sorted({ids.index(b"pair-a"), ids.index(b"pre")} | set(range(4, v0 - 2, 5)))
        remap = retire_both(s, m, rows)
        check_table(s, m)
        check_squeezed(s)
        a = s.vmodels_resolve(ids)
        want = [int(remap[r]) for r in range(v0)]  # (every row is set: a survivor answers its new row, HOST rows included)
        got = [int(x) for x in a["vmodel"]]
        assert got == want, [(r, g, w) for r, (g, w) in enumerate(zip(got, want)) if g != w][:8]
        assert all(c == vm.NOT_FOUND for c, w in zip(a["cls"], want) if w < 0) and all(c != vm.NOT_FOUND for c, w in zip(a["cls"], want) if w >= 0)
        assert a["vmodel"][ids.index(b"pair-b")] == remap[ids.index(b"pair-b")] >= 0 and a["vmodel"][ids.index(b"prefix-long")] >= 0
        check_questions(s, m)
        questions_about(s, m, [ids[r] for r in rows])
        assert s.vmodels_info()["capacity"] == tab_capacity(len(m.ids))
    finally:
        s.close()


# ---- life goes on ---------------------------------------------------------------------------------------------------------------

def test_life_goes_on():
    s, m = start(64), vm.VModels()
    try:
        ids = build(s, m, 17)
        rows = pattern_rows("first half", 17)
        retire_both(s, m, rows)
        assert s.vmodels_info()["capacity"] == 16 and len(m.ids) == 8
        gone = [ids[r] for r in rows]
        # deletions and values of retired ids without APPEND: unknown ids, status 2; survivors are updated all the same
        st, idx, n_app = send(s, m, gone[:3] + [ids[16]] + gone[:2], ["", value_for(1), value_for(2), vm.render("m1", "m2", "upd"), "", ""],
                              [1, 0, 0, 0, 1, 1], append=False)
        assert list(st) == [2, 2, 2, 0, 2, 2] and n_app == 0 and idx[3] == 7
        # retired ids set again join at the end, behind them new ids across the capacity edge (8 + 9 + 20 rows: 16 -> 128 slots)
        new_ids = fx.vmodel_ids(20, b"fresh")
        st, idx, n_app = send(s, m, gone + new_ids + [ids[9], gone[0]], [value_for(k) for k in range(9 + 20)] + [value_for(3), ""],
                              [0] * 30 + [1])
        assert n_app == 29 and list(idx[:9]) == list(range(8, 17)) and not st.any()
        check_table(s, m)
        assert s.vmodels_info()["capacity"] == tab_capacity(37) == 128
        check_questions(s, m)
        # ... and again: the id deleted last (ABSENT_ONLY) and every fourth row
        retire_both(s, m, [8], absent_only=True)
        retire_both(s, m, list(range(0, len(m.ids), 4)))
        check_table(s, m)
        check_squeezed(s)
        check_questions(s, m)
        check_transitions(s, m)
        assert s.vmodels_info()["capacity"] == tab_capacity(len(m.ids)) == 64
    finally:
        s.close()


def test_retire_everything_then_one_append_batch():
    s, m = start(64), vm.VModels()
    try:
        ids = build(s, m, 65)
        remap = retire_both(s, m, list(range(65)))
        assert (remap == -1).all() and tuple(s.vmodels_info()) == (0, 0, 0, 0, 0, 0) and table(s) == ([], b"", [])
        assert answers(s.vmodels_resolve(ids[:3])) == [(0, 0, -1, -1, -1, 0, 0, 0)] * 3
        check_transitions(s, m, "empty")
        remap, n_after = s.vmodels_retire([])  # the empty table: valid, nothing to do
        assert len(remap) == 0 and n_after == 0 and s.vmodels_retire(all_absent=True)[1] == 0
        send(s, m, [ids[5]], [""], [1], append=True)  # a deletion of an id that has left: status 2
        assert s.vmodels_info()["n_rows"] == 0
        send(s, m, ids[::-1][:20], [value_for(k) for k in range(20)])
        assert m.ids == ids[::-1][:20] and s.vmodels_info()["capacity"] == tab_capacity(20)
        check_table(s, m)
        check_questions(s, m)
        retire_both(s, m, [0, 19])
        check_table(s, m)
    finally:
        s.close()


def test_before_the_first_vmodel_call():
    s = WORLD.solver()
    try:
        for kw in (dict(rows=[]), dict(rows=None), dict(all_absent=True), dict(rows=[], absent_only=True)):
            remap, n_after = s.vmodels_retire(**kw)
            assert len(remap) == 0 and n_after == 0 and tuple(s.vmodels_info()) == (0, 0, 0, 0, 0, 0)
        remap, after, rc = s.vmodels_retire_raw([0], fill=FILL)
        assert rc == _lib.MMP_EINVAL and after == FILL_WORD
    finally:
        s.close()


# ---- the two flags --------------------------------------------------------------------------------------------------------------

def test_all_absent():
    s, m = start(64), vm.VModels()
    try:
        ids = fx.vmodel_ids(65, b"aa")
        send(s, m, ids, [value_for(k) for k in range(65)])
        dele = [0, 1, 2, 13, 31, 32, 33, 50, 63, 64]
        send(s, m, [ids[k] for k in dele], [""] * len(dele), [1] * len(dele))
        send(s, m, [ids[13], ids[64]], [value_for(13), value_for(64)])  # two of them set again
        absent = [k for k in dele if k not in (13, 64)]
        remap, after, rc = s.vmodels_retire_raw([absent[0]], _lib.VMRETIRE_ALL_ABSENT, fill=FILL)  # a list beside the flag
        assert rc == _lib.MMP_EINVAL and (remap.view(np.uint8) == FILL).all() and after == FILL_WORD
        remap = retire_both(s, m, all_absent=True)
        assert [k for k in range(65) if remap[k] < 0] == absent
        check_table(s, m)
        check_squeezed(s)
        assert s.vmodels_info()["n_live"] == s.vmodels_info()["n_rows"] == 65 - len(absent)
        before = state(s, ids)
        remap = retire_both(s, m, all_absent=True, absent_only=True)  # right after: the identity
        assert list(remap) == list(range(65 - len(absent))) and state(s, ids) == before
        check_questions(s, m)
    finally:
        s.close()


def test_absent_only():
    s, m = start(64), vm.VModels()
    try:
        ids = build(s, m, 65)  # rows k % 7 == 3 are ABSENT
        absent = [k for k in range(65) if k % 7 == 3]
        send(s, m, [ids[31], ids[17]], [value_for(31), value_for(17)])  # two ids set again since their deletion
        before = state(s, ids)
        with pytest.raises(MmpError) as e:
            s.vmodels_retire(absent[::-1], absent_only=True)
        assert e.value.code == _lib.MMP_EINVAL and "row 17 " in str(e.value), str(e.value)  # the lowest revived row
        with pytest.raises(ValueError, match="row 17 "):
            vrm.retire(m, absent[::-1], absent_only=True)
        remap, after, rc = s.vmodels_retire_raw([31], _lib.VMRETIRE_ABSENT_ONLY, fill=FILL)
        assert rc == _lib.MMP_EINVAL and (remap.view(np.uint8) == FILL).all() and after == FILL_WORD
        assert "row 31 " in s.lib.mmp_last_error(s.h).decode()
        assert state(s, ids) == before
        rest = [k for k in absent if k not in (17, 31)]
        remap = retire_both(s, m, rest + rest[:2], absent_only=True)  # passes on the deleted rows
        assert [k for k in range(65) if remap[k] < 0] == rest
        check_table(s, m)
        check_squeezed(s)
    finally:
        s.close()


# ---- every refusal --------------------------------------------------------------------------------------------------------------

def test_refusals_change_nothing():
    s, m = start(64), vm.VModels()
    try:
        ids = build(s, m, 65)
        v0 = 65
        cases = [dict(rows=None, n=3), dict(rows=[v0]), dict(rows=[0, -1]), dict(rows=[1, 2, v0 + 7, 3]), dict(rows=[0], flags=4),
                 dict(rows=[3], flags=_lib.VMRETIRE_ABSENT_ONLY | 8), dict(rows=[3], max_vmodels=-1), dict(rows=[3], max_vmodels=v0 - 1),
                 dict(rows=[], max_vmodels=v0 - 1), dict(rows=[3, 4], flags=_lib.VMRETIRE_ABSENT_ONLY),
                 dict(rows=[3], flags=_lib.VMRETIRE_ALL_ABSENT), dict(rows=[3], flags=_lib.VMRETIRE_ALL_ABSENT | _lib.VMRETIRE_ABSENT_ONLY)]
        for kw in cases:
            before = state(s, ids)
            remap, after, rc = s.vmodels_retire_raw(fill=FILL, **kw)
            assert rc == _lib.MMP_EINVAL, kw
            assert (remap.view(np.uint8) == FILL).all() and after == FILL_WORD, kw
            assert state(s, ids) == before, kw
        # what is NOT refused: no remap_out at all whatever the room, room to spare, NULL rows with n == 0
        remap, after, rc = s.vmodels_retire_raw([], null_remap=True, max_vmodels=0, fill=FILL)
        assert rc == 0 and after == v0 and (remap.view(np.uint8) == FILL).all()
        remap, after, rc = s.vmodels_retire_raw(None, max_vmodels=v0 + 9, fill=FILL)
        assert rc == 0 and after == v0 and list(remap) == list(range(v0))
        assert s.lib.mmp_vmodels_retire(s.h, None, 0, 0, None, 0, None) == 0
        check_table(s, m)
        remap, after, rc = s.vmodels_retire_raw([3, 10], _lib.VMRETIRE_ABSENT_ONLY, null_remap=True, max_vmodels=0)
        assert rc == 0 and after == v0 - 2
        vrm.retire(m, [3, 10], absent_only=True)
        check_table(s, m)
    finally:
        s.close()


# ---- determinism ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [None, 0])
def test_two_runs_are_byte_identical(monkeypatch, bits):
    if bits is not None:
        monkeypatch.setenv("MMP_VMODEL_ID_HASH_BITS", str(bits))

    def run():
        s, m = start(64), vm.VModels()
        try:
            s.profile(True)
            ids = build(s, m, 257)
            out = []
            for kw in (dict(rows=list(range(1, 257, 3)) + [4, 4]), dict(all_absent=True), dict(rows=[0, 5, 6], absent_only=False)):
                remap, n_after = s.vmodels_retire(**kw)
                assert s.last_kernel_ms() > 0
                out += [remap.tobytes(), n_after] + state(s, ids)
            return out
        finally:
            s.close()

    assert run() == run()


# ---- beside readers -------------------------------------------------------------------------------------------------------------

def test_resolves_beside_event_batches_and_retires():
    """Two groups of ids take turns: the group at the front is deleted, retired (the other group's rows move down) and appended
    again at the end — six states.  200 resolves of both groups on a second thread: every answer array is one of the six."""
    s, m = start(64), vm.VModels()
    try:
        groups = [fx.vmodel_ids(12, b"ga"), fx.vmodel_ids(12, b"gb")]
        vals = [[vm.render(MIDS64[1 + (k + 5 * g) % 63].decode(), MIDS64[1 + (k + 9 * g) % 63].decode(), "o%d" % g) for k in range(12)] for g in (0, 1)]
        keys = groups[0] + groups[1]
        reg = registry_of(s)
        send(s, m, keys, vals[0] + vals[1])

        def steps(g, check):
            """-> the three calls of one turn for the group g at the front"""
            def delete():
                st, _, n = (send(s, m, groups[g], [""] * 12, [1] * 12) if check else s.vmodels_events_json(groups[g], [""] * 12, [1] * 12))
                assert not st.any() and n == 0

            def retire():
                if check:
                    retire_both(s, m, all_absent=True) if g else retire_both(s, m, list(range(12)), absent_only=True)
                else:
                    _, n_after = s.vmodels_retire(all_absent=True) if g else s.vmodels_retire(list(range(12)), absent_only=True)
                    assert n_after == 12

            def append():
                st, _, n = (send(s, m, groups[g], vals[g]) if check else s.vmodels_events_json(groups[g], vals[g]))
                assert not st.any() and n == 12

            return [delete, retire, append]

        want = []
        for g in (0, 1):  # one round in lock step with the model: the six states and their answers
            for call in steps(g, True):
                call()
                got = s.vmodels_resolve(keys)
                assert answers(got) == [tuple(a) for a in m.resolve_many(reg, keys)]
                want.append(got.tobytes())
        assert len(set(want)) >= 5  # (a delete and the retire behind it differ in the other group's row numbers)
        seen, errors, done = [], [], threading.Event()

        def reader():
            try:
                for _ in range(200):
                    seen.append(s.vmodels_resolve(keys).tobytes())
            except Exception as e:  # noqa: BLE001
                errors.append(e)
            finally:
                done.set()

        th = threading.Thread(target=reader)
        th.start()
        turn = 0
        try:
            while not done.is_set() and turn < 2000:  # bounded: the reader ends it
                for call in steps(turn % 2, False):
                    call()
                turn += 1
        finally:
            th.join()
        assert not errors, errors
        assert len(seen) == 200 and all(x in want for x in seen), sum(x not in want for x in seen)
        print(f"200 resolves beside {turn} turns of delete / retire / append: {[sum(x == w for x in seen) for w in want]} per state")
    finally:
        s.close()


# ---- the registry's retire in between -------------------------------------------------------------------------------------------

def test_a_registry_retire_between_two_vmodel_retires():
    s, m = start(), vm.VModels()
    try:
        send(s, m, [b"gone-0", b"v", b"gone-1", b"w", b"gone-2"],
             [vm.render("m1", "m1"), vm.render("not-yet-a-model", MIDS[9].decode()), "", vm.render(MIDS[200].decode(), MIDS[201].decode()),
              vm.render(MIDS[3].decode(), MIDS[4].decode())], [0, 0, 0, 0, 0])
        send(s, m, [b"gone-1"], [""], [1])
        retire_both(s, m, [0])
        a = s.vmodels_resolve([b"v", b"w"])
        assert list(a["vmodel"]) == [0, 2] and list(a["model"]) == [-1, 200] and list(a["target_model"]) == [9, 201]
        st, idx, _, n = s.models_events_json([b"not-yet-a-model"], [REG_VALUES[0]])
        assert not st.any() and list(idx) == [M] and n == 1
        before = (table(s), s.vmodels_info().tobytes())
        remap = s.models_retire([3, 4, 150, 201])  # rows below the answered ones, and an answered row itself
        assert remap[9] == 7 and remap[200] == 197 and remap[201] == -1 and remap[M] == M - 4
        assert (table(s), s.vmodels_info().tobytes()) == before  # no vmodel row changed
        a = s.vmodels_resolve([b"v", b"w", b"gone-2"])
        assert list(a["model"]) == [M - 4, 197, -1] and list(a["target_model"]) == [7, -1, -1]
        check_questions(s, m)
        retire_both(s, m, [1, 3], what="second")  # gone-1 (ABSENT) and gone-2
        a = s.vmodels_resolve([b"v", b"w", b"gone-2", b"gone-1"])
        assert list(a["vmodel"]) == [0, 1, -1, -1] and list(a["model"]) == [M - 4, 197, -1, -1] and list(a["target_model"]) == [7, -1, -1, -1]
        check_table(s, m)
        check_squeezed(s)
        check_questions(s, m)
        check_transitions(s, m)
    finally:
        s.close()
