"""tests/vmodel_write_model.py pinned without a device: on values worked out by hand from VModelManager.java (updateVModel
:174-189 / :216-300, deleteVModel :416-470, PendingTransition.run :725-766), against `json`, and through tests/vmodel_model.py (the
read side's oracle).  And, from the model alone, that every batch tests/test_vmodels_write_gpu.py sends holds every class, every
op and every flag, set and clear."""
import json

import pytest

from tests import vmodel_model as vm
from tests import vmodel_write_fixtures as fx
from tests import vmodel_write_model as wm

NOW, AGE = 1_000_000, 1_000
LONG_MAX = (1 << 63) - 1
# rows: one copy lu 50 / three copies lu 0 / no copy lu 70 / the empty row / one copy lu 0 / two copies
REG = vm.Registry([b"act", b"three", b"idle", b"gone", b"lu0", b"two", b"tgt", b"new"],
                  [(1, 0, 50, 0), (3, 0, 0, 0), (0, 1, 70, 0), (0, 0, 0, 0), (1, 0, 0, 0), (2, 0, 9, 0), (1, 0, 60, 0), (0, 0, 5, 0)])
ICT, ICT_NOW = NOW - 6 * AGE, NOW - AGE
NONE = ((-1, -1), (0, 0), (-1, -1))


def step(op, flags, strs, old, default_owner=b"", now=NOW, age=AGE):
    return wm.write_step(op, flags, strs, old, REG, now, age, default_owner)


def set_(old, target, expected=b"", owner=b"", flags=0, **kw):
    return step(wm.SET, flags, (target, expected, owner), old, **kw)


def row(cls, flags=0, model=-1, count=0, dec=NONE, last_used=0):
    return wm.Row(cls, flags, model, count, dec[0], dec[1], dec[2], last_used)


def test_every_class_op_and_flag_on_the_head():
    b = fx.to_batch(fx.head())
    _, rows = fx.run_model(b)
    assert [r.cls for r in rows[:12]] == list(wm.CLASSES)
    assert fx.holds_everything(b)


def test_no_stored_value():
    assert set_(b"", b"new") == (b'{"amid":"new","tmid":"new"}', row(wm.CREATED, model=7, last_used=ICT))
    assert set_(b"", b"new", flags=wm.LOAD_NOW)[1].last_used == ICT_NOW  # VMM:168-170
    assert set_(b"", b"new", owner=b"me", default_owner=b"dflt")[0] == b'{"o":"me","amid":"new","tmid":"new"}'
    assert set_(b"", b"nowhere", default_owner=b"dflt") == (b'{"o":"dflt","amid":"nowhere","tmid":"nowhere"}', row(wm.CREATED, last_used=ICT))
    assert set_(b"", b"new", flags=wm.UPDATE_ONLY) == (None, row(wm.NOT_FOUND))  # VMM:277
    assert set_(b"", b"new", expected=b"new")[1].cls == wm.CREATED  # VMM:180 expected == target: need not exist
    assert set_(b"", b"new", expected=b"old") == (None, row(wm.PRECONDITION))  # VMM:178
    assert set_(b"", b"new", expected=b"old", flags=wm.UPDATE_ONLY)[1].cls == wm.PRECONDITION  # :178 stands in front of :277
    assert set_(b"", b"new", expected=b"new", flags=wm.UPDATE_ONLY)[1].cls == wm.NOT_FOUND
    assert set_(b"", b'a"b\\c\n')[0] == b'{"amid":"a\\"b\\\\c\\u000a","tmid":"a\\"b\\\\c\\u000a"}'


def test_the_product_and_the_difference_wrap():
    assert set_(b"", b"new", now=5, age=LONG_MAX)[1].last_used == 11  # MAX * 6 wraps to -6
    assert set_(b"", b"new", now=5, age=LONG_MAX, flags=wm.LOAD_NOW)[1].last_used == 5 - LONG_MAX
    assert set_(b"", b"new", now=1, age=1_000)[1].last_used == -5_999  # negative, not wrapping


def test_the_owner():
    old = b'{"o":"owner-a","amid":"act","tmid":"act"}'
    assert set_(old, b"act", owner=b"owner-a")[1].cls == wm.UNCHANGED
    assert set_(old, b"act")[1].cls == wm.UNCHANGED  # no owner given: not compared
    assert set_(old, b"act", owner=b"owner-b") == (None, row(wm.OWNER_MISMATCH))  # differing in the last byte
    assert set_(b'{"amid":"act","tmid":"act"}', b"act", owner=b"owner-a")[1].cls == wm.OWNER_MISMATCH  # against a stored null
    assert set_(b'{"o":null,"amid":"act","tmid":"act"}', b"act", owner=b"x")[1].cls == wm.OWNER_MISMATCH
    assert set_(old, b"new", expected=b"zzz", owner=b"owner-b")[1].cls == wm.OWNER_MISMATCH  # VMM:181 in front of :184
    # o is final in the bean: an update keeps every occurrence as stored
    v, r = set_(b'{"o":"x","o":"owner-a","amid":"idle","tmid":"idle"}', b"new", owner=b"owner-a")
    assert v == b'{"o":"x","o":"owner-a","amid":"new","tmid":"new"}' and r.cls == wm.UPDATED


def test_the_expected_target():
    old = b'{"amid":"act","tmid":"tgt"}'
    assert set_(old, b"new", expected=b"tgt")[1].cls in (wm.UPDATED, wm.NEEDS_TARGET_STATUS)  # equal to the stored target
    assert set_(old, b"tgt", expected=b"zzz")[1].cls == wm.UNCHANGED  # the new one is the stored one: VMM:185
    assert set_(old, b"new", expected=b"new") == (None, row(wm.PRECONDITION))  # equal to the new one only
    assert set_(old, b"new", expected=b"zzz") == (None, row(wm.PRECONDITION))  # to neither
    assert set_(b'{"amid":"act"}', b"new", expected=b"tgt")[1].cls == wm.PRECONDITION  # a stored null equals nothing


def test_target_and_active_equal_different_and_null():
    both = b'{"amid":"act","tmid":"act"}'
    assert set_(both, b"act") == (None, row(wm.UNCHANGED, model=0))  # VMM:243
    assert set_(both, b"act", flags=wm.FORCE) == (None, row(wm.UNCHANGED, model=0))
    # the target matches, the active does not: VMM:245-250
    moving = b'{"amid":"act","tmid":"tgt"}'
    assert set_(moving, b"tgt") == (None, row(wm.UNCHANGED, wm.IN_TRANSITION, 6, 1))
    assert set_(b'{"amid":"three","tmid":"tgt"}', b"tgt")[1] == row(wm.UNCHANGED, wm.IN_TRANSITION, 6, 3)
    assert set_(b'{"amid":"gone","tmid":"tgt"}', b"tgt")[1] == row(wm.UNCHANGED, wm.IN_TRANSITION | wm.PREV_ACTIVE_UNKNOWN, 6, 0)
    assert set_(b'{"amid":"nowhere","tmid":"tgt"}', b"tgt")[1] == row(wm.UNCHANGED, wm.IN_TRANSITION | wm.PREV_ACTIVE_UNKNOWN, 6, 0)
    assert set_(b'{"tmid":"tgt"}', b"tgt")[1] == row(wm.UNCHANGED, wm.IN_TRANSITION, 6, 0)  # a null active id is not looked up
    # ... and forced: the active model switches, VMM:262
    assert set_(moving, b"tgt", flags=wm.FORCE) == (
        b'{"amid":"tgt","tmid":"tgt"}', row(wm.UPDATED, wm.ACTIVE_SWITCHED, 6, 1, ((-1, 0), (0, 9), (-1, 3)), 50))
    # the active matches, the target does not: the previous target goes, nothing is asked of the registry
    assert set_(moving, b"act") == (b'{"amid":"act","tmid":"act"}', row(wm.UPDATED, 0, 0, 0, ((6, -1), (22, 0), (3, -1)), ICT))
    # a null target, a null active
    assert set_(b'{"amid":"act"}', b"act") == (b'{"amid":"act","tmid":"act"}', row(wm.UPDATED, 0, 0, 0, NONE, ICT))
    assert set_(b'{"tmid":"tgt"}', b"new") == (b'{"amid":"new","tmid":"new"}', row(wm.UPDATED, 0, 7, 0, ((6, -1), (9, 0), (3, -1)), ICT))
    assert set_(b"{}", b"new") == (b'{"amid":"new","tmid":"new"}', row(wm.UPDATED, 0, 7, 0, NONE, ICT))


def test_the_previous_target_equal_to_the_previous_active_and_null():
    # equal: one model, and it is the ACTIVE one that may lose the referent (dec[1]), never dec[0]: VMM:237
    v, r = set_(b'{"amid":"idle","tmid":"idle"}', b"new")
    assert v == b'{"amid":"new","tmid":"new"}' and r == row(wm.UPDATED, wm.ACTIVE_SWITCHED, 7, 0, ((-1, 2), (0, 9), (-1, 4)), 70)
    # different: both go when the active switches
    v, r = set_(b'{"amid":"idle","tmid":"tgt"}', b"new")
    assert r == row(wm.UPDATED, wm.ACTIVE_SWITCHED, 7, 0, ((6, 2), (23, 9), (3, 4)), 70)


@pytest.mark.parametrize("active,count,lu", [(b"idle", 0, 70), (b"act", 1, 50), (b"two", 2, 9), (b"three", 3, 0), (b"lu0", 1, 0)])
@pytest.mark.parametrize("force", [0, wm.FORCE])
def test_copy_counts_and_the_status_flags(active, count, lu, force):
    old = b'{"amid":"%s","tmid":"%s","failed":true}' % (active, active)
    switched = b'{"amid":"new","tmid":"new"}'
    waiting = b'{"amid":"%s","tmid":"new"}' % active
    want_lu = lu if lu > 0 else ICT  # VMM:299 prevActive.getLastUsed() > 0
    for status in (0, wm.TARGET_LOADED, wm.TARGET_NOT_LOADED):
        for exists in (0, wm.TARGET_EXISTS):
            v, r = set_(old, b"new", flags=force | status | exists)
            switch = bool(force) or count == 0 or (bool(exists) and count == 1 and status == wm.TARGET_LOADED)  # VMM:262-265
            if not switch and exists and count == 1 and not status:
                assert (v, r) == (None, row(wm.NEEDS_TARGET_STATUS, 0, 7, 1))
                continue
            assert r.cls == wm.UPDATED and r.target_copy_count == count and r.last_used == want_lu and r.model == 7
            assert v == (switched if switch else waiting)  # failed := false either way, VMM:273
            assert r.flags == (wm.ACTIVE_SWITCHED if switch else wm.IN_TRANSITION)
            assert r.dec_len == ((-1, len(active)) if switch else (-1, -1)) and r.dec_model[1] == (REG.row(active) if switch else -1)


def test_an_unknown_and_an_empty_row_previous_active():
    for active in (b"nowhere", b"gone"):
        v, r = set_(b'{"amid":"%s","tmid":"tgt"}' % active, b"new", flags=wm.TARGET_EXISTS)
        assert v == b'{"amid":"new","tmid":"new"}'
        assert r.flags == wm.ACTIVE_SWITCHED | wm.PREV_ACTIVE_UNKNOWN and r.target_copy_count == 0 and r.last_used == ICT
        assert r.dec_model == (6, REG.row(active)) and r.dec_len == (3, len(active))


def test_delete():
    old = b'{"o":"owner-a","amid":"act","tmid":"tgt"}'
    d = lambda old, owner=b"": step(wm.DELETE, 0, (b"", b"", owner), old)  # noqa: E731
    assert d(b"") == (None, row(wm.NOOP)) and d(b"", b"owner-a") == (None, row(wm.NOOP))  # VMM:419
    assert d(old, b"owner-b") == (None, row(wm.NOOP))  # the owner2 delete without effect
    assert d(b'{"amid":"act","tmid":"tgt"}', b"owner-a") == (None, row(wm.NOOP))  # against a stored null
    both = row(wm.DELETED, dec=((0, 6), (23, 36), (3, 3)))
    assert d(old) == (None, both) and d(old, b"owner-a") == (None, both)  # models differing: both lose a referent
    assert d(b'{"amid":"act","tmid":"act"}')[1] == row(wm.DELETED, dec=((0, -1), (9, 0), (3, -1)))  # matching: one, VMM:441
    assert d(b'{"tmid":"tgt"}')[1] == row(wm.DELETED, dec=((-1, 6), (0, 9), (-1, 3)))  # a null active
    assert d(b'{"amid":"act"}')[1] == row(wm.DELETED, dec=((0, -1), (9, 0), (3, -1)))  # a null target
    assert d(b"{}")[1] == row(wm.DELETED)


def test_complete_on_both_sides_of_each_half_of_the_guard():
    c = lambda old, to, frm: step(wm.COMPLETE, 0, (to, frm, b""), old)  # noqa: E731
    old = b'{"o":"x","amid":"act","tmid":"tgt","failed":true,"keep":[1]}'
    assert c(old, b"tgt", b"act") == (b'{"o":"x","keep":[1],"amid":"tgt","tmid":"tgt"}', row(wm.UPDATED, dec=((0, -1), (17, 0), (3, -1))))
    assert c(old, b"tgt", b"acu") == (None, row(wm.CHANGED))  # VMM:762 the active moved
    assert c(old, b"tgu", b"act") == (None, row(wm.CHANGED))  # VMM:763 the target moved
    assert c(b"", b"tgt", b"act") == (None, row(wm.CHANGED))  # deleted meanwhile
    assert c(b'{"tmid":"tgt"}', b"tgt", b"") == (b'{"amid":"tgt","tmid":"tgt"}', row(wm.UPDATED))  # an empty fromId: a stored null
    assert c(b'{"tmid":"tgt"}', b"tgt", b"act")[1].cls == wm.CHANGED and c(old, b"tgt", b"")[1].cls == wm.CHANGED


def test_fail_flag_in_all_four_combinations():
    f = lambda old, want: step(wm.FAIL_FLAG, wm.FAILED if want else 0, (b"", b"", b""), old)  # noqa: E731
    plain, failed = b'{"amid":"act","tmid":"tgt"}', b'{"amid":"act","failed":true,"tmid":"tgt"}'
    assert f(plain, False) == (None, row(wm.UNCHANGED, wm.IN_TRANSITION)) and f(failed, True) == (None, row(wm.UNCHANGED, wm.IN_TRANSITION))
    assert f(plain, True) == (b'{"amid":"act","tmid":"tgt","failed":true}', row(wm.UPDATED, wm.IN_TRANSITION))
    assert f(failed, False) == (plain, row(wm.UPDATED, wm.IN_TRANSITION))
    assert f(b"", True) == (None, row(wm.NOOP))
    assert f(b'{"failed":true,"failed":false}', False)[1].cls == wm.UNCHANGED  # the last occurrence decides


def test_unknown_members_of_every_json_type_are_kept_and_stored_strings_stay_raw():
    kept = b'"a" : [1, {"amid":5}] , "b":{"tmid":"x","failed":true},"c":"x\\"amid\\"", "d":-1.5e3,"e":true,"f":null'
    old = b' { "amid":"act", ' + kept + b' , "tmid" : "t\xc3\xa9" ,"failed":true} '
    same = kept.replace(b" , ", b",").replace(b'"x\\"amid\\"", ', b'"x\\"amid\\"",')
    v, r = step(wm.FAIL_FLAG, 0, (b"", b"", b""), old)
    assert v == b"{" + same + b',"amid":"act","tmid":"t\xc3\xa9"}' and r.cls == wm.UPDATED


def test_malformed_and_the_host():
    for old in (b" ", b"{", b'{"amid":"a"', b'{"amid":7}', b'{"failed":"true"}', b'{"amid":7,"amid":"a"}'):
        for op in wm.OPS:
            assert step(op, 0, (b"a", b"a", b""), old) == (None, row(wm.MALFORMED)), (op, old)
    esc = b'{"o":"ow\\\\ner","amid":"act","tmid":"act"}'
    assert set_(esc, b"act")[1].cls == wm.UNCHANGED and set_(esc, b"act", owner=b"x") == (None, row(wm.HOST))
    for old in (b'{"amid":"a\\\\b","tmid":"act"}', b'{"amid":"act","tmid":"a\\u0041"}'):
        assert [step(op, 0, (b"act", b"act", b""), old)[1].cls for op in wm.OPS] == [wm.HOST, wm.HOST, wm.HOST, wm.UNCHANGED]
    assert set_(b'{"amid":"a\\\\b","amid":"act","tmid":"act"}', b"act")[1].cls == wm.UNCHANGED  # the escaped one lost
    with pytest.raises(ValueError):
        set_(b'{"\\u0061mid":"act"}', b"act")


def _rendered(b):
    vals, rows = fx.run_model(b)
    return [(i, v, r) for i, (v, r) in enumerate(zip(vals, rows)) if r.cls in wm.RENDERED]


@pytest.fixture(scope="module")
def batches():
    return fx.every_batch()


def _loads(v):
    return json.loads(v.decode("utf-8", "surrogateescape"), object_pairs_hook=list)


def test_against_json_and_through_the_read_sides_oracle(batches):
    """The new value means the old one with the owned keys replaced, and parses back to the intended record."""
    n = 0
    for b in batches:
        for i, v, r in _rendered(b):
            verdict, got = vm.classify(v)
            assert got is not None, (i, v)
            doc = _loads(v)
            ida, idb, owner = (x or b"" for x in b.strs[i])
            op, flags = b.reqs[i]
            if r.cls == wm.CREATED:
                own = owner or fx.DEFAULT_OWNER
                assert (got.amid, got.tmid, got.owner, got.failed) == (ida, ida, own, False) or b"\\" in v
                assert [k for k, _ in doc] == ["o", "amid", "tmid"]
                assert dict(doc)["amid"].encode("utf-8", "surrogateescape") == ida and dict(doc)["o"].encode("utf-8", "surrogateescape") == own
            else:
                old_doc, old = _loads(b.olds[i]), vm.classify(b.olds[i])[1]
                assert [(k, x) for k, x in doc if k not in ("amid", "tmid", "failed")] == [(k, x) for k, x in old_doc if k not in ("amid", "tmid", "failed")]
                assert [k for k, _ in doc if k in ("amid", "tmid", "failed")] == [k for k in ("amid", "tmid", "failed") if k in dict(doc)]
                assert got.owner == old.owner
                if op == wm.FAIL_FLAG:
                    assert (got.amid, got.tmid, got.failed) == (old.amid, old.tmid, bool(flags & wm.FAILED))
                elif op == wm.COMPLETE:
                    assert dict(doc)["amid"].encode("utf-8", "surrogateescape") == ida and got.tmid == old.tmid and not got.failed
                else:
                    assert dict(doc)["tmid"].encode("utf-8", "surrogateescape") == ida and not got.failed
                    switched = bool(r.flags & wm.ACTIVE_SWITCHED) or old.amid is None
                    assert dict(doc).get("amid", "").encode("utf-8", "surrogateescape") == (ida if switched or old.amid == ida else old.amid)
                assert bool(r.flags & wm.IN_TRANSITION) == vm.in_transition(got) or b"\\" in v
            n += 1
    assert n > 400  # (not vacuous)


def test_every_batch_the_gpu_test_sends_holds_every_class_op_and_flag(batches):
    for b in batches:
        assert len(b.reqs) >= len(fx.head()) and fx.holds_everything(b)
    singles = fx.single_batches()
    assert [fx.run_model(b)[1][0].cls for b in singles] == list(wm.CLASSES) and {b.reqs[0][0] for b in singles} == set(wm.OPS)
    drawn = fx.Batch(*zip(*[((o, f), t, v) for o, f, t, v in fx.drawn_items(240, 257)]))
    # the drawn requests bring every class on their own but the one that takes four flags at once (the head's)
    assert {r.cls for r in fx.run_model(drawn)[1]} >= set(wm.CLASSES) - {wm.NEEDS_TARGET_STATUS}
    lens = [len(o) for o in fx.tile_edge_batch().olds]
    assert all(lens.count(n) == 8 for n in range(fx.TILE - 2, fx.TILE + 3))
    assert sum(len(o) > fx.TILE for o in fx.member_batch(True).olds) == 3 * 5 * len(fx.MEMBER_COUNTS)
    assert fx.REG.recs[fx.MIDS.index(fx.A)][0] == 1 and fx.REG.recs[fx.MIDS.index(fx.C)][0] == 0


def test_a_generator_refuses_a_batch_that_lacks_a_class_an_op_or_a_flag():
    head = fx.head()
    for k in (0, 3, 4, 5, 6, 8, 9, 10, 11):  # (the classes the head holds once)
        with pytest.raises(ValueError):
            fx.to_batch(head[:k] + head[k + 1:] + [head[2]] * 2)
    with pytest.raises(ValueError):
        fx.to_batch([it if not it[1] & wm.LOAD_NOW else (it[0], it[1] & ~wm.LOAD_NOW) + it[2:] for it in head])
