"""GPU: cache_replay_kernel and evict_batch_kernel at the edges of their value domain, held to the REFERENCE'S OWN local-cache
text — tests/golden/ref_clhm_edges.npz, see tests/test_ref_clhm_edges.py.  Every case goes to the device three ways (one call;
prefix call + probe call; cut at every recorded boundary) and a fourth time with the recorded state before the probes loaded
through mmp_caches_load_keyed; every operation's result, evicted keys in listener order, buffer weight, weightedSize() and
oldestTime(), and after each call every cache's deque, capacity, weighted size and manager fields, bit for bit.  Which team
width a cache takes in a call follows from its recorded entry count and the call's inserts by mmp_cache_replay's rule
(ref_clhm_cases.team_width): asserted here on both sides of 48 and of 160 slots and at the 2047 slots of the full tile."""
import os

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd.solver import MmpError, Solver
from tests import ref_clhm_cases as rc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "ref_clhm_edges.npz")
NAMES = ("lengths_plain", "lengths_managed", "lengths_big", "mass_plain", "mass_managed", "clhm", "manager", "wide")


@pytest.fixture(scope="module")
def vec():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def solver():
    s = Solver(100, 1000)
    yield s
    s.close()


def _entries_at(v, j):
    """every cache's entry count at boundary j (0: the loaded state, the pinned entry of a managed cache)"""
    return (v["reserved"] >= 0).astype(np.int64) if j == 0 else v[f"b{j}/hdr"][:, 0]


def _call_widths(v, j0, j1):
    """{(team width, slots + 1)} of the caches with operations in the call [bounds[j0], bounds[j1]): the host's rule"""
    ops = v["ops"][v["bounds"][j0]: v["bounds"][j1]]
    n0 = _entries_at(v, j0)
    ins = np.bincount(ops["cache"][np.isin(ops["op"], (0, 4, 12))], minlength=len(n0))
    touched = np.bincount(ops["cache"], minlength=len(n0)) > 0
    return {(rc.team_width(int(n0[c] + ins[c])), int(n0[c] + ins[c]) + 1) for c in np.nonzero(touched)[0]}


def _check_outs(v, a, got, gev):
    outs, ev = v["outs"], v["evicted"]
    for i in range(len(got)):
        o, g = outs[a + i], got[i]
        want_ev = list(ev[o["evicted_off"]: o["evicted_off"] + o["n_evicted"]])
        have_ev = list(gev[g["evicted_off"]: g["evicted_off"] + g["n_evicted"]])
        assert (g["result"], have_ev, g["buffer_weight"], g["weighted_size"], g["oldest_time"]) == \
            (o["result"], want_ev, o["buffer_weight"], o["weighted_size"], o["oldest_time"]), (v["name"], a + i, v["ops"][a + i])


def _check_state(s, v, j):
    for c in range(len(v["caps"])):
        hdr, keys, wts, lus = rc.edge_state(v, j, c)
        st = s.cache_read(c)
        assert np.array_equal(st["key"], keys) and np.array_equal(st["weight"], wts) and np.array_equal(st["last_used"], lus), (v["name"], j, c)
        assert (st["capacity"], st["weighted_size"]) == (hdr[1], hdr[2]), (v["name"], j, c)
        if v["reserved"][c] >= 0:
            u = st["ubm"]
            assert (u["total_unloading"], u["total_occupancy"], u["cache_deficit"]) == (hdr[3], hdr[4], hdr[5]), (v["name"], j, c)


def _replay(s, v, cut_at):
    """from the empty caches, one call per [bounds[j0], bounds[j1]) of consecutive cut_at; -> the widths the calls took"""
    seg, lus, wts, keys = rc.initial_state(v["caps"], v["reserved"])
    ubm = np.zeros(len(v["caps"]), dtype=_lib.UBM_STATE)
    ubm["reserved"] = v["reserved"]
    s.load_caches_keyed(seg, lus, wts, keys, v["caps"], ubm)
    widths = set()
    for j0, j1 in zip(cut_at[:-1], cut_at[1:]):
        a, b = int(v["bounds"][j0]), int(v["bounds"][j1])
        widths |= _call_widths(v, j0, j1)
        got, gev = s.cache_replay(v["ops"][a:b].astype(_lib.CACHE_OP), rc.NOW)
        _check_outs(v, a, got, gev)
        _check_state(s, v, j1)
    return widths


def _load_boundary(s, v, j):
    """the recorded state at boundary j onto the device through mmp_caches_load_keyed"""
    hdr = v[f"b{j}/hdr"]
    seg = np.concatenate([[0], np.cumsum(hdr[:, 0])]).astype(np.int32)
    ubm = np.zeros(len(hdr), dtype=_lib.UBM_STATE)
    ubm["reserved"], ubm["total_unloading"], ubm["total_occupancy"], ubm["cache_deficit"] = v["reserved"], hdr[:, 3], hdr[:, 4], hdr[:, 5]
    s.load_caches_keyed(seg, v[f"b{j}/last_used"], v[f"b{j}/weight"], v[f"b{j}/key"], hdr[:, 1], ubm)


@pytest.mark.parametrize("name", NAMES)
def test_device_replay_equals_the_reference_text_at_the_edges(vec, solver, name):
    v = rc.load_edge_case(vec, name)
    last = len(v["bounds"]) - 1
    pre = last - 1
    w1 = _replay(solver, v, [0, last])
    w2 = _replay(solver, v, [0, pre, last])
    w3 = _replay(solver, v, list(range(last + 1)))
    _load_boundary(solver, v, pre)  # the state before the probes by another route onto the device
    got, gev = solver.cache_replay(v["ops"][v["n_prefix"]:].astype(_lib.CACHE_OP), rc.NOW)
    _check_outs(v, v["n_prefix"], got, gev)
    _check_state(solver, v, last)
    probe = _call_widths(v, pre, last)
    assert probe <= w2 and 0 not in {w for w, _ in w1 | w2 | w3}
    # mmp_cache_replay: 8 lanes while slots + 1 <= kTeam8Slots (48), 16 up to kTeam16Slots (160), else the wavefront
    if name in ("lengths_plain", "lengths_managed"):
        assert {(8, 48), (16, 49), (16, 160), (64, 161)} <= probe, sorted(probe)
        assert {8, 16, 64} == {w for w, _ in w1} == {w for w, _ in w3}
    if name == "lengths_big":
        assert probe == {(64, 2047), (64, 2048)} and (64, 2048) in w1
    if name.startswith("mass"):
        assert {8, 16, 64} == {w for w, _ in probe}


def test_a_cache_that_needs_2048_slots_is_refused_and_2047_slots_run(solver):
    """By hand: kCacheTile = 2048 columns hold slots + 1.  2047 entries and one insert is refused with MMP_EINVAL and leaves
    every cache as it was; 2046 entries and one insert run (the new key, older than all, becomes the head)."""
    n = np.array([2047, 2046, 3])
    seg = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    lus = np.concatenate([rc.T0 + 10 * np.arange(k) for k in n]).astype(np.int64)
    wts = np.full(int(seg[-1]), 3, np.int32)
    keys = np.concatenate([1 + np.arange(k) for k in n]).astype(np.int32)
    caps = np.full(3, 10**9, np.int64)
    solver.load_caches_keyed(seg, lus, wts, keys, caps, None)

    def unchanged(c):
        st = solver.cache_read(c)
        a, b = seg[c], seg[c + 1]
        return (np.array_equal(st["key"], keys[a:b]) and np.array_equal(st["weight"], wts[a:b]) and np.array_equal(st["last_used"], lus[a:b])
                and (st["capacity"], st["weighted_size"]) == (10**9, 3 * n[c]))
    ops = np.zeros(3, dtype=_lib.CACHE_OP)
    ops["cache"], ops["op"], ops["key"], ops["arg"], ops["time"] = [2, 0, 1], 0, rc.PROBE_KEY, 3, rc.T0 - 5
    with pytest.raises(MmpError) as e:
        solver.cache_replay(ops, rc.NOW)
    assert e.value.code == _lib.MMP_EINVAL
    assert all(unchanged(c) for c in range(3))
    got, gev = solver.cache_replay(ops[[0, 2]], rc.NOW)
    assert [tuple(g) for g in got[["result", "n_evicted", "buffer_weight", "weighted_size", "oldest_time"]]] == \
        [(1, 0, 0, 12, rc.T0 - 5), (1, 0, 0, 3 * 2047, rc.T0 - 5)]
    assert unchanged(0)
    st = solver.cache_read(1)
    assert np.array_equal(st["key"], np.concatenate([[rc.PROBE_KEY], keys[seg[1]: seg[2]]]))
    assert np.array_equal(st["last_used"], np.concatenate([[rc.T0 - 5], lus[seg[1]: seg[2]]])) and (st["weight"] == 3).all()


def _evict_rows(v):
    """the runs of a case whose probe is one putIfAbsent of an absent key on a plain cache"""
    rows = []
    for r in v["runs"]:
        c = int(r["cache"])
        _, q = rc.run_rows(v, c)
        op = v["ops"][q[0]]
        if v["reserved"][c] < 0 and op["op"] == 0 and v["outs"][q[0]]["result"] == 1:
            rows.append((c, int(q[0])))
    return rows


@pytest.mark.parametrize("name,team", [("clhm", 8), ("wide", 8), ("lengths_plain", 16), ("lengths_big", 16), ("mass_plain", 16)])
def test_stateless_eviction_equals_the_reference_text_at_the_edges(vec, solver, name, team):
    """Every such probe as one mmp_evict_batch evaluation on the recorded state before it (the first probe of a run: the state in
    front of a later probe is not recorded).  evict_launch takes 8 lanes per evaluation while the loaded deques average <= 24
    entries, 16 beyond: which one a case takes is asserted from the states loaded.  lengths_big: the two inserts on a deque of
    2 046 entries, 128 trips of the 16-lane loops."""
    v = rc.load_edge_case(vec, name)
    pre, last = len(v["bounds"]) - 2, len(v["bounds"]) - 1
    rows = _evict_rows(v)
    states = [rc.edge_state(v, pre, c) for c, _ in rows]
    seg = np.concatenate([[0], np.cumsum([len(k) for _, k, _, _ in states])]).astype(np.int32)
    assert rows and (8 if seg[-1] <= 24 * len(rows) else 16) == team  # (evict_launch's rule, mmplace.hip)
    solver.load_caches(seg, np.concatenate([lu for _, _, _, lu in states]), np.concatenate([w for _, _, w, _ in states]),
                       np.array([h[1] for h, _, _, _ in states], np.int64))
    reqs = np.zeros(len(rows), dtype=_lib.EVICT_REQ)
    reqs["cache"] = np.arange(len(rows))
    reqs["weight"] = [v["ops"][i]["arg"] for _, i in rows]
    reqs["last_used"] = [v["ops"][i]["time"] for _, i in rows]
    got = solver.evict(reqs, rc.NOW)
    for k, (c, i) in enumerate(rows):
        o, op = v["outs"][i], v["ops"][i]
        victims = [int(x) for x in v["evicted"][o["evicted_off"]: o["evicted_off"] + o["n_evicted"]]]
        nxt = [q for q in rc.run_rows(v, c)[1] if q > i]
        if op["key"] in victims:
            pos = victims.index(op["key"])
        elif not nxt:  # the key's place in the final deque + the victims polled in front of it
            pos = list(rc.edge_state(v, last, c)[1]).index(op["key"]) + len(victims)
        else:
            pos = None  # (a later probe moved it)
        g = got[k]
        assert (g["n_victims"], g["self_evicted"], g["weighted_size"], g["oldest_time"]) == \
            (len(victims), int(op["key"] in victims), o["weighted_size"], o["oldest_time"]), (name, c, op)
        if pos is not None:
            assert g["insert_pos"] == pos, (name, c, op)
    lengths = {int(v["runs"][c]["entries"]) for c, _ in rows}
    want = {"clhm": 9, "wide": 5, "lengths_big": 2, "mass_plain": 2 * len(rc.MASS)}  # the plain inserts each case holds
    if name == "lengths_plain":  # an insert at every length, head and tail and the team-width positions
        assert lengths == set(rc.LENGTHS) and len(rows) >= 4 * len(rc.LENGTHS)
    else:
        assert len(rows) == want[name] and (name != "lengths_big" or lengths == {2046})
