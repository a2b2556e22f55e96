"""The local cache at the edges of its value domain, held to the REFERENCE'S OWN TEXT: tests/golden/ref_clhm_edges.npz is what
clhm/ConcurrentLinkedHashMap.java, clhm/LinkedDeque.java and ModelCacheUnloadBufManager.java (compiled as they stand by
oracle/ref_harness; regenerate with oracle/ref_harness/make_clhm_vectors.py --edges) do on tests/ref_clhm_cases.edge_cases():
deque lengths around every chunk and team-width edge of cache_replay_kernel, one operation evicting 1 .. 257 entries, and
pairs of runs one unit either side of each comparison of the text.  Here: the premises of those cases, asserted from the
inputs, and the C oracle (oracle/mm_evict_oracle.c) operation by operation and at every recorded call boundary.  The device is
held to the same file in tests/test_ref_clhm_edges_gpu.py.  Nothing here needs the reference tree."""
import os

import numpy as np
import pytest

from oracle import bind as ob
from tests import ref_clhm_cases as rc

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "ref_clhm_edges.npz")


@pytest.fixture(scope="module")
def cases():
    vec = np.load(GOLDEN)
    return [rc.load_edge_case(vec, str(n)) for n in vec["names"]]


def test_the_file_holds_the_generators_cases(cases):
    """Inputs are reproducible from tests/ref_clhm_cases.py; nothing was cut (the domain rule refuses instead)."""
    want = rc.edge_cases()
    assert [v["name"] for v in cases] == [w["name"] for w in want]
    assert {v["tier"] for v in cases} == set(rc.EDGE_TIERS)
    for v, w in zip(cases, want):
        for k in ("caps", "reserved", "ops", "bounds", "runs", "pairs", "tag_names", "pair_names"):
            assert np.array_equal(v[k], w[k]), (v["name"], k)
        assert v["tier"] == w["tier"]
        assert len(v["outs"]) == len(v["ops"])
        ev = v["evicted"]
        assert rc.UNLOADBUF_KEY not in ev, v["name"]  # the pinned entry is never evicted
        reserved = v["reserved"]
        assert ((v["ops"]["op"] < 4) | (reserved[v["ops"]["cache"]] >= 0)).all()


def test_every_pair_differs_by_one_unit_in_the_stated_value_and_in_nothing_else(cases):
    n = alike = 0
    for v in cases:
        for p in v["pairs"]:
            a, b, field = int(p["a"]), int(p["b"]), rc.PAIR_FIELDS[p["field"]]
            name = (v["name"], str(v["pair_names"][p["name"]]))
            oa = v["ops"][np.concatenate(rc.run_rows(v, a))]
            ob_ = v["ops"][np.concatenate(rc.run_rows(v, b))]
            assert len(oa) == len(ob_) and v["reserved"][a] == v["reserved"][b], name
            diffs = [(i, f) for i in range(len(oa)) for f in ("op", "key", "arg", "time", "flag") if oa[i][f] != ob_[i][f]]
            if field == "cap":
                assert not diffs and abs(int(v["caps"][a]) - int(v["caps"][b])) == 1, name
            else:
                assert v["caps"][a] == v["caps"][b], name
                assert len(diffs) == 1 and diffs[0][1] == field, (name, diffs)
                i = diffs[0][0]
                assert abs(int(oa[i][field]) - int(ob_[i][field])) == 1, name
            # what the generator refused otherwise: the reference tells the two sides apart (or, marked alike, cannot)
            assert (rc.run_signature(v, v, a) == rc.run_signature(v, v, b)) == bool(p["alike"]), name
            n += 1
            alike += int(p["alike"])
    assert n >= 55 and alike == 3


def test_entry_counts_at_the_call_boundaries_are_the_listed_ones(cases):
    """Before the probe call a run holds the entries its tag promises (+ the pinned entry); the boundaries before cut every
    prefix; the widths that follow from the counts by mmp_cache_replay's rule are on both sides of 48 and of 160 slots."""
    for v in cases:
        pre = len(v["bounds"]) - 2  # the boundary in front of the probes
        assert v["bounds"][pre] == v["n_prefix"] and (v["ops"]["cache"][: v["n_prefix"]] >= 0).all()
        hdr = v[f"b{pre}/hdr"]
        for r in v["runs"]:
            pidx, qidx = rc.run_rows(v, int(r["cache"]))
            assert (len(pidx), len(qidx)) == (r["n_prefix"], r["n_probe"]) and r["n_probe"] >= 1
            if r["entries"] >= 0:
                assert hdr[r["cache"], 0] == r["entries"] + r["managed"], (v["name"], r)
        if v["name"] in ("lengths_plain", "lengths_managed"):
            mid = v["b1/hdr"][:, 0]
            assert ((mid > 0) & (mid < hdr[:, 0])).sum() > len(hdr) // 2  # the first cut lies inside most prefixes
    lens = {int(r["entries"]) for v in cases if v["name"] in ("lengths_plain", "lengths_managed") for r in v["runs"]}
    assert lens == set(rc.LENGTHS)
    big = next(v for v in cases if v["name"] == "lengths_big")
    assert {(int(r["entries"]), int(r["managed"])) for r in big["runs"]} == {(2046, 0), (2045, 1), (2046, 1)}


def test_every_tier_holds_what_it_is_there_for(cases):
    for v in cases:
        occ = rc.edge_occurrence(v, v["tier"], v["name"])
        assert occ and all(occ.values()), (v["name"], [k for k, ok in occ.items() if not ok])


def test_c_oracle_equals_the_reference_text_at_the_edges(cases):
    n_ops = n_ev = 0
    for v in cases:
        name, caps, reserved, ops, outs, ev = v["name"], v["caps"], v["reserved"], v["ops"], v["outs"], v["evicted"]
        caches = [ob.CCache(int(caps[c]), None if reserved[c] < 0 else int(reserved[c]), rc.NOW) for c in range(len(caps))]
        bounds = [int(b) for b in v["bounds"]]
        for i, op in enumerate(ops):
            h = caches[op["cache"]]
            if h.u is not None:
                h.u.n_evicted = 0  # (the oracle's eviction log is a fixed array)
            res, evk = h.apply(int(op["op"]), int(op["key"]), int(op["arg"]), int(op["time"]), int(op["flag"]), rc.NOW)
            o = outs[i]
            want_ev = [int(k) for k in ev[o["evicted_off"]: o["evicted_off"] + o["n_evicted"]]]
            bw = h.lib.orc_ubm_buffer_weight(ob.C.byref(h.u)) if h.u is not None else 0
            assert (res, [int(k) for k in evk], h.c.weighted_size, h.oldest_time(), bw) == \
                (o["result"], want_ev, o["weighted_size"], o["oldest_time"], o["buffer_weight"]), (name, i, op)
            n_ev += len(evk)
            if i + 1 in bounds:
                j = bounds.index(i + 1)
                for c, hc in enumerate(caches):
                    hdr, keys, wts, lus = rc.edge_state(v, j, c)
                    lu, wt, key = hc.nodes()
                    assert np.array_equal(key, keys) and np.array_equal(wt, wts) and np.array_equal(lu, lus), (name, j, c)
                    assert (hc.c.capacity, hc.c.weighted_size) == (hdr[1], hdr[2]), (name, j, c)
                    if hc.u is not None:
                        assert (hc.u.total_unloading, hc.u.total_occupancy, hc.u.cache_deficit) == (hdr[3], hdr[4], hdr[5]), (name, j, c)
        n_ops += len(ops)
    assert n_ops > 100_000 and n_ev > 5_000
