"""CPU: tests/cache_keyed_model.py, the definition of the caches by model id, pinned on cases worked out by hand — every rule from
both sides: an id that resolves and one that does not, a live and a deleted record, an inserting and a non-inserting op under an
unknown id, a raw key and a keyless code, slots used and unused in the eviction record, a load that passes and one that is refused,
a retirement that passes and one that is refused."""
import numpy as np
import pytest

from modelmesh_amd import _lib
from oracle import bind as ob
from tests.cache_keyed_model import IdTable, Refused

NOW = 1_760_000_000_000
IDS = [b"a", b"bb", b"", "é".encode(), b"gone"]  # row 4 is the empty row of a deleted record


def table():
    return IdTable(IDS, empty_rows=[4])


def op(cache, code, arg=0, time=0, flag=0, key=0, reserved=0):
    return np.array([(cache, code, key, arg, time, flag, reserved)], dtype=_lib.CACHE_OP)[0]


def test_the_three_statuses():
    t = table()
    assert t.resolve(b"bb") == (_lib.CKEY_LIVE, 1)
    assert t.resolve(b"") == (_lib.CKEY_LIVE, 2)            # the empty id is an ordinary id
    assert t.resolve("é") == (_lib.CKEY_LIVE, 3)
    assert t.resolve(b"gone") == (_lib.CKEY_EMPTY_ROW, 4)   # the row as the table answers it
    assert t.resolve(b"nobody") == (_lib.CKEY_UNKNOWN, None)


def test_the_rule_by_key_and_its_two_exceptions():
    t = table()
    # the key the caller sent is never read
    assert t.op_key(op(0, _lib.COP_GET, key=77), b"bb") == (_lib.CKEY_LIVE, 1, True)
    assert t.op_key(op(0, _lib.COP_REMOVE, key=77), b"gone") == (_lib.CKEY_EMPTY_ROW, 4, True)
    # a raw key keeps the pseudo-entry's key, a keyless code has none: neither reads its id
    assert t.op_key(op(0, _lib.COP_GET, key=_lib.UNLOADBUF_KEY, reserved=_lib.COPK_RAW_KEY), b"nobody") == (_lib.CKEY_LIVE, _lib.UNLOADBUF_KEY, True)
    for code in _lib.COP_KEYLESS:
        assert t.op_key(op(0, code), b"nobody") == (_lib.CKEY_LIVE, -1, True)
    with pytest.raises(AssertionError):
        t.op_key(op(0, _lib.COP_GET, key=5, reserved=_lib.COPK_RAW_KEY), b"a")


def test_unknown_ids_inserting_and_not():
    t = table()
    for code in range(13):
        st, key, runs = t.op_key(op(0, code), b"nobody")
        if code in _lib.COP_KEYLESS:
            assert (st, key, runs) == (_lib.CKEY_LIVE, -1, True)
        else:
            assert (st, key) == (_lib.CKEY_UNKNOWN, _lib.CACHE_KEY_UNKNOWN) and runs == (code not in (0, 4, 12))
    assert _lib.CACHE_KEY_UNKNOWN == -2**31


def test_a_replay_by_hand_with_its_eviction_record():
    """capacity 10: a(4) b(4) at rows 0, 1; put é(4) evicts a; put nobody is not run; get gone is absent; a second, untouched cache
    gets no slots; the record has 2 entries + 2 inserting ops = 4 slots, one used."""
    t = table()
    h0, h1 = ob.CCache(10, None, NOW), ob.CCache(10, None, NOW)
    h0.put_if_absent(0, 4, NOW - 30, NOW)
    h0.put_if_absent(1, 4, NOW - 20, NOW)
    h1.put_if_absent(2, 1, NOW - 10, NOW)
    ops = [op(0, _lib.COP_PUT_IF_ABSENT, 4, NOW - 5), op(0, _lib.COP_PUT_IF_ABSENT, 1, NOW - 4), op(0, _lib.COP_GET), op(0, _lib.COP_GET)]
    out, (rows, ids) = t.replay([h0, h1], ops, ["é", b"nobody", b"gone", b"bb"], NOW)
    assert [(o["status"], o["key"], o["result"], o["evicted_rows"], o["evicted_ids"]) for o in out] == [
        (_lib.CKEY_LIVE, 3, 1, [0], [b"a"]),
        (_lib.CKEY_UNKNOWN, _lib.CACHE_KEY_UNKNOWN, 0, [], []),
        (_lib.CKEY_EMPTY_ROW, 4, 0, [], []),
        (_lib.CKEY_LIVE, 1, 1, [], [])]
    assert (rows, ids) == ([0, -1, -1, -1], [b"a", b"", b"", b""])
    assert list(h0.nodes()[2]) == [3, 1] and list(h1.nodes()[2]) == [2]  # (the read moved bb behind é)
    # no op at all: no slot
    assert t.replay([h0, h1], [], [], NOW) == ([], ([], []))


def test_a_non_inserting_op_under_an_unknown_id_is_the_absent_key():
    """adjustWeightAfterLoad on an absent key still moves the manager's sums: the same under the reserved key as under any key the
    cache does not hold."""
    t = table()
    a, b = ob.CCache(1000, 100, NOW), ob.CCache(1000, 100, NOW)
    o = op(0, _lib.COP_UBM_ADJUST_AFTER_LOAD, 7)
    out, _ = t.replay([a], [o], [b"nobody"], NOW)
    want = b.apply(_lib.COP_UBM_ADJUST_AFTER_LOAD, 12345, 7, 0, 0, NOW)
    assert (out[0]["result"], out[0]["evicted_rows"]) == want and out[0]["status"] == _lib.CKEY_UNKNOWN
    assert (a.u.total_occupancy, a.u.total_unloading, a.u.cache_deficit) == (b.u.total_occupancy, b.u.total_unloading, b.u.cache_deficit)
    assert [list(x) for x in a.nodes()] == [list(x) for x in b.nodes()]


def test_the_load_passes_and_is_refused():
    t = table()
    assert t.load_rows([b"bb", b"gone", b"", b"whatever"], [0, 0, 0, 1]) == [1, 4, 2, _lib.UNLOADBUF_KEY]
    with pytest.raises(Refused) as e:
        t.load_rows([b"bb", b"x", b"a", b"y"])
    assert (e.value.what, e.value.index) == ("entry", 1)  # the lowest one
    with pytest.raises(Refused):
        t.load_rows([b"whatever"], [0])                   # unmarked: read like any id


def test_the_retirement_guard_and_the_renumbering():
    t = table()
    live = [[3, 1], [_lib.UNLOADBUF_KEY, 4]]
    with pytest.raises(Refused) as e:
        t.retire([4, 2, 3], live)
    assert (e.value.what, e.value.index) == ("row", 3) and t.ids == IDS  # the lowest live key named; nothing changed
    remap = t.retire([0, 2, 2], live)                                      # below and between the keys; named twice, retired once
    assert remap == [-1, 0, -1, 1, 2]
    assert [t.renumber(k, remap) for k in live] == [[1, 0], [_lib.UNLOADBUF_KEY, 2]]
    assert t.ids == [b"bb", "é".encode(), b"gone"] and t.empty == {2}
    assert t.resolve(b"a") == (_lib.CKEY_UNKNOWN, None) and t.resolve(b"gone") == (_lib.CKEY_EMPTY_ROW, 2)
