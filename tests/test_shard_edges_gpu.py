"""GPU: the pod-axis shard kernels (modelmesh_amd/csrc/shard_kernels.hpp) at the edges of the load target's value domain, against
what the reference's own text decided on the same rows (tests/golden/ref_place_edges.npz: the cases of tests/test_place_edges_gpu.py).
The shard code states the break thresholds, the rpm rule, the pick and the self exits a second time (derive3 … derive5 and the
phases around them), runs the lane kernels in an instantiation of their own (a view of the slice, head windows and count bitmaps
built per slice by the sharded commit, the packed exchange words), and ranks a slice of the table against the whole of it — so every
case goes through both pod-axis drivers, at shard counts that cut the table inside one word's reach, leave trailing slices empty and
make every word a slice.  tests/test_shard_edges_premise.py asserts on the CPU that the cases put their thresholds ACROSS slices.
Every comparison is exact, and made on every shard's output rows."""
import ctypes as C
import os
import re
import threading
import time

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd import dist as mdist
from modelmesh_amd.solver import MmpError, Solver
from oracle.bind import OracleFleet
from tests import ref_fleets as rf
from tests.place_edge_helpers import GOLDEN_PLACE_EDGES, NAMES, excluded_pods, n_words, shard_counts
from tests.test_place_edges_gpu import place_dev, subset
from tests.test_ref_vectors import check_place
from tests.test_shard_group_gpu import ThreadExchange, _async_run
from tests.test_shard_gpu import _load_shard

pytestmark = pytest.mark.gpu

CASES = {c[0]: c[1:] for c in rf.place_edge_cases()}
NAME_G = [(name, G) for name in NAMES for G in shard_counts(CASES[name][0])]
WITH_PAIRS = [name for name in NAMES if rf.place_edge_meta(name)["pairs"]]
STAT_FIELDS = ("total_capacity", "total_free", "global_lru", "instance_count", "model_copy_count")
JOIN_S = 120  # a shard thread that has not returned by then is reported, not waited for


def _kernel_constant(name):
    src = open(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc", "place_kernel.hpp")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


K_EARLY_EXTRA, K_INLINE_EXCL = _kernel_constant("kEarlyExtra"), _kernel_constant("kInlineExcl")
PAD_TOTALS = [K_EARLY_EXTRA, K_EARLY_EXTRA + 1, K_INLINE_EXCL, K_INLINE_EXCL + 1, 12]


@pytest.fixture(scope="module")
def ref():
    return np.load(GOLDEN_PLACE_EDGES)


@pytest.fixture(scope="module")
def oracle_stats():
    memo = {}

    def get(name):
        if name not in memo:
            memo[name] = OracleFleet(CASES[name][0]).stats()
        return memo[name]
    return get


def check_stats(name, st, want):
    for f in STAT_FIELDS:
        assert int(st[f]) == int(want[f]), (name, f)


def check_rank(name, fleet, rank, want):
    """The all-reduced rank vector: the present rows hold the positions 0 … n - 1, in the reference's order."""
    present = np.flatnonzero((fleet.pods["flags"] & 5) == 0)
    assert len(present) == len(want), name
    assert np.array_equal(np.sort(rank[present]), np.arange(len(want))), (name, "the present rows do not hold the first positions")
    assert np.array_equal(present[np.argsort(rank[present], kind="stable")], want), (name, "order")


def changed_rows(name, fleet, f2):
    ch = np.flatnonzero(f2.pods != fleet.pods).astype(np.int32)
    assert 0 < len(ch) <= 16, (name, len(ch))
    return ch


# ---- the phase API: G contexts advanced in lock step, the all-reduce done with tensor ops ---------------------------------------
class PhaseShards:
    def __init__(self, fleet, G, speculative):
        import torch
        self.dev, self.G = torch.device("cuda", 0), G
        self.solvers, self.placers = [], []
        for g in range(G):
            s, p = _load_shard(fleet, g, G, self.dev, speculative)
            self.solvers.append(s)
            self.placers.append(p)

    def commit(self):
        """-> the rank vector as every shard holds it after the all-reduce."""
        seen = []

        def tap(gen):
            for t, op in gen:
                assert op == "sum"
                yield t, op
                seen.append(t.cpu().numpy().copy())  # (run_lockstep wrote the reduced vector into every shard's tensor)
        mdist.run_lockstep([tap(p.commit_steps()) for p in self.placers])
        assert len(seen) == self.G
        for r in seen[1:]:
            assert np.array_equal(r, seen[0])
        return seen[0]

    def place(self, reqs, extra, now):
        """-> every shard's rows, n_rest"""
        import torch
        n = len(reqs)
        d_reqs = torch.from_numpy(np.ascontiguousarray(reqs).view(np.uint8).reshape(-1).copy()).to(self.dev)
        d_extra = torch.from_numpy(np.ascontiguousarray(extra if len(extra) else np.zeros(1, np.int32), dtype=np.int32)).to(self.dev)
        outs = [torch.zeros(max(n, 1) * _lib.PLACE_OUT.itemsize, dtype=torch.uint8, device=self.dev) for _ in range(self.G)]
        mdist.run_lockstep([p.place_steps(d_reqs, n, d_extra, now, o) for p, o in zip(self.placers, outs)])
        torch.cuda.synchronize()
        assert len({p.last_n_rest for p in self.placers}) == 1
        return [np.frombuffer(o.cpu().numpy().tobytes(), dtype=_lib.PLACE_OUT)[:n] for o in outs], self.placers[0].last_n_rest

    def close(self):
        for s in self.solvers:
            s.close()


def _phase_case(ref, oracle_stats, name, G, speculative, place=True):
    fleet, _, reqs, extra = CASES[name]
    meta = rf.place_edge_meta(name)
    sh = PhaseShards(fleet, G, speculative)
    try:
        check_rank(name, fleet, sh.commit(), ref[f"{name}/order"])
        for s in sh.solvers:
            check_stats(name, s.stats(), oracle_stats(name))
            with pytest.raises(MmpError):  # the order is not a shard's to give
                s.order()
        if place:
            rows, n_rest = sh.place(reqs, extra, fleet.now)
            assert n_rest == len(reqs) if not speculative else n_rest <= len(reqs)
            for g, got in enumerate(rows):
                check_place(f"{name} G={G} shard {g}", fleet, reqs, got, ref[f"{name}/place"])
        if meta["after"]:  # a few rows move: every shard takes them, the shards commit again together
            after = meta["after"]
            f2, _, r2, x2 = CASES[after]
            ch = changed_rows(name, fleet, f2)
            for s in sh.solvers:
                s.upsert_pods(ch, f2.pods[ch])
            check_rank(after + " (second sharded commit)", f2, sh.commit(), ref[f"{after}/order"])
            for s in sh.solvers:
                check_stats(after, s.stats(), oracle_stats(after))
            if place:
                rows, _ = sh.place(r2, x2, f2.now)
                for g, got in enumerate(rows):
                    check_place(f"{after} (second sharded commit) G={G} shard {g}", f2, r2, got, ref[f"{after}/place"])
    finally:
        sh.close()


@pytest.mark.parametrize("speculative", [True, False], ids=["speculative", "six-phases"])
@pytest.mark.parametrize("name,G", NAME_G)
def test_phase_api_equals_the_reference_text(ref, oracle_stats, name, G, speculative):
    """speculative=False sends every row through the six phases: derive3 … derive5 decide all of them."""
    _phase_case(ref, oracle_stats, name, G, speculative)


@pytest.mark.parametrize("mode", ["1", "3"])
@pytest.mark.parametrize("name", NAMES)
def test_sharded_rank_by_both_routes(ref, oracle_stats, name, mode, monkeypatch):
    """mmp_shard_rank_dev ranks a slice of the rows against the whole table — all pairs (1), or by sorting the table and keeping the
    slice's ranks (3).  Three shards where the table has more than one word (uneven row slices), two otherwise."""
    monkeypatch.setenv("MMP_RANK_MODE", mode)
    _phase_case(ref, oracle_stats, name, 2 if n_words(CASES[name][0]) == 1 else 3, True)


# ---- the in-library group: G contexts driven by G host threads through the library's transport callback -------------------------
def run_group(fleet, G, body):
    """body(solver, shard) on every shard of a committed group -> the bodies' results by shard.  No transport for a group of one."""
    xc = ThreadExchange(G) if G > 1 else None
    results, errors, keep = [None] * G, [], []

    def run(g):
        s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
        try:
            if xc is not None:
                cb = xc.fn_for(g)
                keep.append(cb)
                assert s.lib.mmp_shard_group_set_exchange(s.h, C.cast(cb, C.c_void_p), None) == 0
            s.shard_group_init(None, g, G)
            s.load_fleet(fleet, commit=False)
            s.shard_commit()
            results[g] = body(s, g)
            s.shard_group_destroy()
        except Exception as e:  # noqa: BLE001
            errors.append((g, repr(e)))
            if xc is not None:
                xc.bar.abort()
        finally:
            s.close()

    ths = [threading.Thread(target=run, args=(g,), daemon=True) for g in range(G)]
    for t in ths:
        t.start()
    deadline = time.monotonic() + JOIN_S
    for t in ths:
        t.join(max(0.0, deadline - time.monotonic()))
    alive = [g for g, t in enumerate(ths) if t.is_alive()]
    if alive:
        if xc is not None:
            xc.bar.abort()
        pytest.fail(f"shard threads {alive} of {G} have not returned after {JOIN_S} s")
    assert not errors, errors
    return results


def refuses_order(s):
    try:
        s.order()
    except MmpError:
        return True
    return False


def halves(reqs, extra):
    n = len(reqs)
    return [subset(reqs, np.arange(0, n // 2), extra), subset(reqs, np.arange(n // 2, n), extra)]


@pytest.mark.parametrize("name,G", NAME_G)
def test_group_equals_the_reference_text(ref, oracle_stats, name, G):
    """mmp_shard_commit / mmp_shard_place_batch, and the same rows as two mmp_shard_place_batch_async_dev batches closed by
    mmp_shard_wait.  A group of one runs place_shard_fast_direct_kernel."""
    fleet, _, reqs, extra = CASES[name]
    meta = rf.place_edge_meta(name)
    after = meta["after"]
    if after:
        f2, _, r2, x2 = CASES[after]
        ch = changed_rows(name, fleet, f2)

    def body(s, g):
        out = dict(stats=s.stats(), refused=refuses_order(s))
        out["rows"], out["n_rest"] = s.shard_place(reqs, extra, fleet.now)
        out["async"], _ = _async_run(s, fleet, halves(reqs, extra))
        if after:
            s.upsert_pods(ch, f2.pods[ch])
            s.shard_commit()
            out["stats2"] = s.stats()
            out["rows2"], _ = s.shard_place(r2, x2, f2.now)
        return out

    res = run_group(fleet, G, body)
    n = len(reqs)
    assert len({r["n_rest"] for r in res}) == 1
    for g, r in enumerate(res):
        tag = f"{name} group G={G} shard {g}"
        assert r["refused"], tag
        check_stats(tag, r["stats"], oracle_stats(name))
        check_place(tag, fleet, reqs, r["rows"], ref[f"{name}/place"])
        check_place(tag + " async, first batch", fleet, reqs[: n // 2], r["async"][0][: n // 2], ref[f"{name}/place"][: n // 2])
        check_place(tag + " async, second batch", fleet, reqs[n // 2:], r["async"][1][: n - n // 2], ref[f"{name}/place"][n // 2:])
        if after:
            check_stats(tag + " second commit", r["stats2"], oracle_stats(after))
            check_place(f"{after} (second sharded commit) group G={G} shard {g}", f2, r2, r["rows2"], ref[f"{after}/place"])


def test_every_tier_but_the_order_tier_has_pairs():
    assert sorted(WITH_PAIRS) == sorted(n for n in NAMES if not n.startswith("edge_order_")), WITH_PAIRS


@pytest.mark.parametrize("name", WITH_PAIRS)
def test_group_one_request_per_call(ref, name):
    """Both rows of every engineered pair through the group of two with n = 1."""
    fleet, _, reqs, extra = CASES[name]
    pairs = rf.place_edge_meta(name)["pairs"]
    rows = np.array(sorted({i for p in pairs for i in p[:2]}), np.int64)
    for a, b, _ in pairs:  # from the inputs: every engineered pair is sent
        assert a in rows and b in rows, (name, a, b)
    calls = [subset(reqs, [i], extra) for i in rows]

    def body(s, g):
        one = np.zeros(len(rows), dtype=_lib.PLACE_OUT)
        for k, (q, qx) in enumerate(calls):
            one[k] = s.shard_place(q, qx, fleet.now)[0][0]
        return one

    for g, one in enumerate(run_group(fleet, 2, body)):
        check_place(f"{name} one request per call, shard {g}", fleet, reqs[rows], one, ref[f"{name}/place"][rows])


# ---- more exclusions than the lane path holds inline: the group hands such a request to the six phases --------------------------
def padded_case(name):
    """The case with every row that already excludes an instance carrying copies of that instance up to a total (its model's entries
    + its own exclusions) of kEarlyExtra, kEarlyExtra + 1, kInlineExcl, kInlineExcl + 1 and 12 in rotation; a row that holds more
    already is left alone.  The reference's exclusion sets are sets: the expected rows do not change.
    -> (reqs, extra, padded rows, how many of them carry more than kInlineExcl)"""
    fleet, _, reqs, extra = CASES[name]
    out, pool, rows, beyond = reqs.copy(), [], [], 0
    for i, r in enumerate(reqs):
        own = [int(x) for x in extra[r["extra_off"]: r["extra_off"] + r["n_extra"]]]
        ex = excluded_pods(fleet, r, extra)
        if ex:
            m = fleet.models[r["model"]]
            n_ents = int(m["n_loaded"]) + int(m["n_failed"])
            own += [ex[0]] * max(0, PAD_TOTALS[len(rows) % len(PAD_TOTALS)] - n_ents - len(own))
            rows.append(i)
            beyond += n_ents + len(own) > K_INLINE_EXCL
        out["extra_off"][i], out["n_extra"][i] = len(pool), len(own)
        pool += own
    return out, np.array(pool, np.int32), np.array(rows, np.int64), beyond


def padded_routes():
    for name in NAMES:
        W = n_words(CASES[name][0])
        for G in sorted({2, W}):
            yield name, G
        yield name, 0  # the unsharded context: the same counts select its lane, late and wave routes


@pytest.mark.parametrize("name,G", list(padded_routes()), ids=lambda v: "unsharded" if v == 0 else str(v))
def test_padded_exclusions_take_the_six_phases(ref, name, G):
    fleet, _, reqs, _ = CASES[name]
    q, qx, rows, beyond = padded_case(name)
    # from the inputs: most rows can be padded, and most pair rows of a case that has pairs; two fifths of them go beyond the lane path
    pair_rows = sorted({i for p in rf.place_edge_meta(name)["pairs"] for i in p[:2]})
    assert 3 * len(rows) >= 2 * len(reqs), (name, len(rows), len(reqs))
    assert 2 * len(set(pair_rows) & set(rows.tolist())) >= len(pair_rows), name
    assert beyond >= 2 * (len(rows) // len(PAD_TOTALS)), (name, beyond)
    assert len(qx) == int(q["n_extra"].sum())
    want = ref[f"{name}/place"]
    if G == 0:
        s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
        try:
            s.load_fleet(fleet)
            check_place(name + " padded, place", fleet, q, s.place(q, qx, fleet.now), want)
            check_place(name + " padded, place_dev", fleet, q, place_dev(s, q, qx, fleet.now), want)
        finally:
            s.close()
        return
    res = run_group(fleet, G, lambda s, g: s.shard_place(q, qx, fleet.now))
    for g, (got, n_rest) in enumerate(res):
        print(name, "G", G, "shard", g, "padded rows", len(rows), "beyond kInlineExcl", beyond, "n_rest", n_rest)
        check_place(f"{name} padded, group G={G} shard {g}", fleet, q, got, want)
        check_place(f"{name} padded rows, group G={G} shard {g}", fleet, q[rows], got[rows], want[rows])
        assert n_rest >= beyond, (name, G, n_rest, beyond)
