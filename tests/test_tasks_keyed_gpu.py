"""mmp_scaleup_plan_k, mmp_scaledown_plan_k, mmp_migration_plan_k and mmp_janitor_plan_k on the device, every comparison exact:
against the calls each replaces (model_ids_resolve + the by-row call, and for the janitor with its scale-down a third call) on a
second context in the same state, against the restatement (tests/tasks_keyed_model.py), and on their own: unknown and deleted ids,
duplicates, the window a retirement opens between the calls, keys (empty, UTF-8, at the 16-byte chunk edge, beyond the LDS
staging region, offsets that do not start at 0), the chain, refusals, answers beside a writer, run-to-run identity.  Small fleets:
8 x 300 and one of 64 x 2000."""
import copy
import os
import re
import threading

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd._lib import CACHE_ENTRY, CONC_ENTRY, CONC_PARAMS, JAN_REMOVED, JANITOR_APPLY, JANITOR_DRY, JANITOR_ENTRY, SCALEUP_PARAMS
from modelmesh_amd.solver import MmpError, Solver
from tests import janitor_model as jm
from tests import registry_prune_model as rp
from tests import tasks_keyed_model as tk
from tests import test_rebalance_gpu as rb
from tests import test_status_by_id_gpu as sbg
from tests.registry_ops_model import ModelRecord
from tests.tasks_keyed_model import CHAIN_SELF, InvalidEntries, TaskWorld

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5
LONG_ID = b"L" * 17_000                         # one key longer than the 16 KB a workgroup stages
IDS = [b"", "modèle-é".encode(), LONG_ID, b"k" * 15, b"k" * 16, b"k" * 17] + [b"m%d" % i for i in range(6, 300)]
WIDE = lambda i: b"W" * 190 + b"%010d" % i      # noqa: E731  200 bytes: 256 of these in one workgroup are 51 200 key bytes
DYN = 60_000


def block_sizes():
    """kIdTabBlock, kKeyedLdsBytes and kJanTile as the source states them, and that the new kernel is built on the first two."""
    csrc = os.path.join(ROOT, "modelmesh_amd", "csrc")
    kernel = open(os.path.join(csrc, "tasks_keyed_kernels.hpp")).read()
    assert "__launch_bounds__(kIdTabBlock) void tasks_keyed_kernel" in kernel and "staged[kKeyedLdsBytes / 16]" in kernel
    assert "blockIdx.x * kIdTabBlock" in kernel and "vkeyed_stage(staged, kKeyedLdsBytes," in kernel
    text = "".join(open(os.path.join(csrc, f)).read() for f in ("pod_events_kernels.hpp", "model_ids_kernels.hpp", "keyed_kernels.hpp",
                                                                "janitor_kernels.hpp", "ingest_kernels.hpp"))
    val = lambda name: int(re.search(r"constexpr int " + name + r" = (\d+);", text).group(1))  # noqa: E731
    return val("kIdTabBlock"), val("kKeyedLdsBytes"), val("kJanTile")


IDTAB_BLOCK, LDS_BYTES, JAN_TILE = block_sizes()
SIZES = sorted({0, 1, 63, 64, 65, IDTAB_BLOCK - 1, IDTAB_BLOCK, IDTAB_BLOCK + 1})
CAND_COUNTS = sorted({0, 1, JAN_TILE - 1, JAN_TILE, JAN_TILE + 1})


def test_the_block_sizes_are_the_ones_the_sizes_were_chosen_for():
    assert (IDTAB_BLOCK, LDS_BYTES, JAN_TILE) == (256, 16384, 64)
    assert SIZES == [0, 1, 63, 64, 65, 255, 256, 257] and CAND_COUNTS == [0, 1, 63, 64, 65]
    assert len(LONG_ID) > LDS_BYTES and 256 * len(WIDE(0)) > LDS_BYTES


# ---- worlds -------------------------------------------------------------------------------------------------------------------

def jan_world(pods, models, ids=None, seed=0):
    """The janitor recipe's fleet, nearly full (so that the scale-down runs), three records deleted (the empty row) among the
    models the instance caches.  -> (fleet, self_pod, world, deleted rows)"""
    fleet, self_pod, reg = jm.janitor_fleet(seed, pods, models)
    fleet.pods["flags"] = 2
    fleet.pods["used"] = (fleet.pods["capacity"] * 0.97).astype(np.int64)
    dele = [int(m) for m in fleet.jan_chosen[20:23]]
    for i in dele:
        reg[i] = rp.Record(0, [], [], 0)
    fleet.models, fleet.ent_pod, fleet.ent_time = rp.registry_to_arrays(reg)
    ids = ids if ids is not None else [b"id-%d" % i for i in range(models)]
    return fleet, self_pod, TaskWorld(fleet, ids, reg), dele


def loaded(fleet, ids):
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    s.load_fleet(fleet)
    s.model_ids_load(ids)
    return s


def untouched(*xs):
    return all(set(np.asarray(x).tobytes()) <= {FILL} for x in xs)


def same_registry(s, w):
    for g, x in zip(rp.compact(*s.get_models()), rp.registry_to_arrays(w.records_by_row())):
        assert np.array_equal(g, x)


def same_contexts(s1, s2):
    for a, b in zip(rp.compact(*s1.get_models()), rp.compact(*s2.get_models())):
        assert a.tobytes() == b.tobytes()


def keys_of(w, models, tag=b"unknown"):
    """The id of each row, a distinct unknown id for -1; and the field itself poisoned: by key it is never read."""
    return [w.ids[int(m)] if m >= 0 else tag + b"-%d" % r for r, m in enumerate(models)]


def cache_rows(w, rng, n, self_pod, skip=()):
    """n mmp_cache_entry rows of a plausible local cache and their keys; `skip`: rows no entry may name (the composition's host
    skips what it knows to be deleted)."""
    e = rb._local_entries(w.fleet, self_pod, rng, n)
    for i in range(n):
        while int(e["model"][i]) in skip:
            e["model"][i] = (int(e["model"][i]) + 1) % len(w.ids)
    keys = keys_of(w, e["model"])
    rows = e["model"].copy()
    e["model"] = -12345
    return e, keys, rows


def jan_rows(w, fleet, self_pod, now, seed, n=None, skip=()):
    """The janitor recipe's cache rows over the registry as it stands, and their keys."""
    e = jm.make_cache(fleet, w.records_by_row(), self_pod, seed, now)
    e = e[~np.isin(e["model"], list(skip))] if len(skip) else e
    e = e[:n] if n is not None else e
    assert n is None or len(e) == n
    keys = keys_of(w, e["model"])
    rows = e["model"].copy()
    e = e.copy()
    e["model"] = -12345
    return e, keys, rows


def up_params(self_pod, now, thr=2000, our_rpm=100, last_check=None):
    sp = np.zeros(1, dtype=SCALEUP_PARAMS)
    sp["self_pod"], sp["iteration_counter"] = self_pod, 130
    sp["second_copy_max_age_iters"], sp["second_copy_min_age_iters"] = 240, 42
    sp["scale_up_rpm_threshold"], sp["our_rpm"] = thr, our_rpm
    sp["now"], sp["last_check_time"], sp["rate_check_interval_ms"] = now, now - 10_000 if last_check is None else last_check, 10_000
    sp["second_copy_lru_threshold_ms"], sp["assume_completed_ms"] = 72_000_000, 30_000
    return sp


def conc_random(rng, n):
    c = np.zeros(n, dtype=CONC_ENTRY)
    cnt, tsum = rng.integers(0, 400, n), rng.integers(0, 5_000_000, n)
    c["count_and_time_sum"] = (tsum << 21) | cnt             # MMP_CONC_COUNT_BITS
    c["prior_sum"], c["prior_count"] = rng.integers(0, 3_000_000, n), rng.integers(0, 300, n)
    c["max_conc"], c["queued_requests"] = rng.integers(1, 9, n), rng.integers(0, 4, n)
    return c


def conc_par(avg=1.5):
    cp = np.zeros(1, dtype=CONC_PARAMS)
    cp["dynamic_rpm_scale_constant"], cp["average_model_parallelism"] = DYN, avg
    return cp


def eq(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, a[:6], b[:6])


def up_vs_model(got, want, what):
    """The device's rate task against the oracle's: getExcludeSet() is built lazily in the Java (MM.java:5771-5774), so its content
    is compared only when some entry is scaled up, and rpm only in a run that was not skipped (tests/test_rebalance_gpu.py)."""
    idx, outs, ov, sk = got[0], got[1], got[-3] if len(got) == 6 else got[2], got[-2] if len(got) == 6 else got[3]
    widx, wouts, wov, wsk = want[0], want[1], want[-3] if len(want) == 6 else want[2], want[-2] if len(want) == 6 else want[3]
    eq(idx, widx, what)
    assert sk == wsk, what
    for f in ("action", "copies", "timestamp", "new_i1", "new_i2", "heavy") + (() if sk else ("rpm",)):
        assert np.array_equal(outs[f], wouts[f]), (what, f)
    if np.any(wouts["action"] == 2):
        assert np.array_equal(ov, wov), what
    if len(got) == 6:
        for f in ("threshold", "reset", "new_prior_sum", "new_prior_count"):
            assert np.array_equal(got[2][f], want[2][f]), (what, f)
        assert got[5].tobytes() == np.asarray(want[5]).tobytes(), what


@pytest.fixture(scope="module")
def big():
    """Two contexts in the same state on the 64 x 2000 fleet: `a` gets the one call, `b` the calls it replaces; both advance
    together, and so does the restatement."""
    fleet, self_pod, w, dele = jan_world(64, 2000)
    a, b = loaded(fleet, w.ids), loaded(fleet, w.ids)
    yield a, b, w, fleet, self_pod, dele
    a.close()
    b.close()


@pytest.fixture(scope="module")
def small():
    fleet, self_pod, w, dele = jan_world(8, 300, IDS)
    return fleet, self_pod, w, dele


# ---- equality with the calls each replaces, and with the restatement -------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_the_three_read_only_tasks_equal_resolve_plus_the_by_row_call(big, n):
    a, b, w, fleet, self_pod, dele = big
    now, rng = int(fleet.now), np.random.default_rng(4000 + n)
    e, keys, _ = cache_rows(w, rng, n, self_pod, skip=dele)
    by_row = e.copy()
    by_row["model"] = b.model_ids_resolve(keys) if n else 0
    conc = conc_random(rng, n)
    for thr, our_rpm, last_check in ((2000, 100, now - 10_000), (100, 50_000, now - 9_000), (2000, 0, now - 1_000)):
        sp = up_params(self_pod, now, thr, our_rpm, last_check)
        idx, outs, _, ov, sk, _, rc = a.scaleup_plan_k_raw(e, keys, sp, fill=FILL)
        assert rc == 0
        wouts, wov, wsk = b.scaleup_plan(by_row, sp)
        eq(idx, by_row["model"]), eq(outs, wouts), eq(ov, wov)
        assert sk == wsk
        up_vs_model((idx, outs, ov, sk), w.scaleup(e, keys, sp), (n, thr))
        idx, outs, couts, ov, sk, res, rc = a.scaleup_plan_k_raw(e, keys, sp, conc, conc_par(), fill=FILL)
        assert rc == 0
        wouts, wcouts, wov, wsk, wres = b.scaleup_plan_conc(by_row, conc, sp, conc_par())
        eq(idx, by_row["model"]), eq(outs, wouts), eq(couts, wcouts), eq(ov, wov), eq(res, wres)
        assert sk == wsk
        up_vs_model((idx, outs, couts, ov, sk, res), w.scaleup(e, keys, sp, conc, conc_par()), (n, thr, "conc"))
        # by row (both key pointers NULL) the new call IS the old one
        ridx, routs, _, rov, rsk, _, rc = a.scaleup_plan_k_raw(by_row, None, sp, fill=FILL)
        assert rc == 0 and rsk == b.scaleup_plan(by_row, sp)[2]
        eq(ridx, by_row["model"]), eq(routs, b.scaleup_plan(by_row, sp)[0])
    for cap, sd in ((200_000, 0), (1_000, 0), (10_000_000, 0), (200_000, 1)):
        dp = tk.chain_scaledown(now, cap, self_pod)
        dp["shutting_down"] = sd
        idx, rem, rc = a.scaledown_plan_k_raw(e, keys, dp, fill=FILL)
        assert rc == 0
        eq(idx, by_row["model"]), eq(rem, b.scaledown_plan(by_row, dp))
        eq(rem, w.scaledown(e, keys, dp)[1])
        idx, rem, rc = a.scaledown_plan_k_raw(e, keys, dp, conc, DYN, fill=FILL)
        assert rc == 0
        eq(idx, by_row["model"]), eq(rem, b.scaledown_plan_conc(by_row, conc, dp, DYN))
        eq(rem, w.scaledown(e, keys, dp, conc, DYN)[1])
        eq(a.scaledown_plan_k_raw(by_row, None, dp, fill=FILL)[1], b.scaledown_plan(by_row, dp))
    idx, act, wait, rc = a.migration_plan_k_raw(e, keys, self_pod, now, fill=FILL)
    assert rc == 0
    wact, wwait = b.migration_plan(by_row, self_pod, now)
    eq(idx, by_row["model"]), eq(act, wact), eq(wait, wwait)
    midx, mact, mwait = w.migration(e, keys, self_pod, now)
    eq(idx, midx), eq(act, mact), eq(wait, mwait)
    ridx, ract, rwait, rc = a.migration_plan_k_raw(by_row, None, self_pod, now, fill=FILL)
    assert rc == 0
    eq(ridx, by_row["model"]), eq(ract, wact), eq(rwait, wwait)
    same_contexts(a, b)


def three_calls(b, e, keys, prm, flags, cap, dp=None, conc=None):
    """model_ids_resolve, mmp_janitor_plan on the rows it answered, mmp_scaledown_plan / _conc on the candidates that returned."""
    e = e.copy()
    e["model"] = b.model_ids_resolve(keys) if len(e) else 0
    actions, edits, cands, rows, info = b.janitor_plan_raw(e, prm, flags, cap, cap)
    rem = None
    if dp is not None and not info["truncated"]:
        rem = b.scaledown_plan(cands, dp) if conc is None else b.scaledown_plan_conc(cands, conc[rows], dp, DYN)
    return e["model"].copy(), actions, edits, cands, rows, rem, info


def same_janitor(got, want, what=""):
    for g, x, f in zip(got[:5], want[:5], ("model_idx", "actions", "edits", "candidates", "candidate_rows")):
        eq(g, x, (what, f))
    if want[5] is not None:
        eq(got[5], want[5], (what, "removed"))
    for f in ("n_edits", "n_candidates", "n_ties", "stopped_at", "truncated"):
        assert int(got[6][f]) == int(want[6][f]), (what, f, got[6], want[6])
    assert list(got[6]["n_action"]) == list(want[6]["n_action"]), (what, got[6], want[6])


@pytest.mark.parametrize("n", SIZES)
def test_the_janitor_with_its_scale_down_equals_the_three_calls_it_replaces(big, n):
    a, b, w, fleet, self_pod, dele = big
    now = int(fleet.now) + n                     # (a clock value of its own per case: the state advances with every apply)
    prm, dp = jm.params(self_pod, now), tk.chain_scaledown(now, 10_000_000, self_pod)
    cap = max(n, 1) + 1200
    for step, flags in enumerate((0, JANITOR_DRY, JANITOR_APPLY, JANITOR_APPLY)):
        e, keys, _ = jan_rows(w, fleet, self_pod, now, 50 + step, n, skip=dele)
        conc = conc_random(np.random.default_rng(n + step), n) if step == 3 else None
        chain = dp if flags == JANITOR_APPLY else None
        got = a.janitor_plan_k_raw(e, keys, prm, flags, cap, cap, chain, conc, DYN, fill=FILL)
        assert got[-1] == 0
        want = three_calls(b, e, keys, prm, flags, cap, chain, conc)
        same_janitor(got, want, (n, flags))
        same_contexts(a, b)
        same_janitor(got, w.janitor(e, keys, prm, dry=flags != JANITOR_APPLY, scaledown=chain, conc=conc, dyn_const=DYN), (n, flags, "model"))
        same_registry(a, w)
    # by row (both key pointers NULL), without a chain, the new call IS the old one
    e, keys, rows = jan_rows(w, fleet, self_pod, now, 60, n, skip=dele)
    e["model"] = rows
    got = a.janitor_plan_k_raw(e, None, prm, 0, cap, cap, fill=FILL)
    assert got[-1] == 0
    act, ed, cands, crow, info = b.janitor_plan_raw(e, prm, 0, cap, cap)
    same_janitor(got, (rows, act, ed, cands, crow, None, info), (n, "by row"))


# ---- unknown and deleted ids ---------------------------------------------------------------------------------------------------

def test_unknown_and_deleted_ids_are_model_minus_one_in_all_four_calls(small):
    fleet, self_pod, w0, dele = small
    w, now = copy.deepcopy(w0), int(fleet.now)
    s = loaded(fleet, IDS)
    try:
        e, keys, rows = jan_rows(w, fleet, self_pod, now, 7)
        hit = [r for r, m in enumerate(rows) if m in dele]
        assert len(hit) == 3 and (rows == -1).sum() == 4
        got = s.janitor_plan_k(e, keys, jm.params(self_pod, now))
        same_janitor(got, w.janitor(e, keys, jm.params(self_pod, now)), "all")
        assert (got[0][hit] == rows[hit]).all() and (got[1][hit] == JAN_REMOVED).all()      # the row is answered, the entry goes (:5968)
        assert not np.isin(got[2]["model"], dele).any() and not np.isin(got[3]["model"], dele).any()
        same_registry(s, w)
        rng = np.random.default_rng(5)
        c, ckeys, crows = cache_rows(w, rng, 200, self_pod)
        for j, m in enumerate(dele):
            ckeys[j], crows[j] = w.ids[m], m
        c["last_used"][:6] = now - 5_000_000
        c["flags"][:6] = 0
        ckeys[3:6] = [b"nobody", b"nobody", b"k" * 14]
        sp, dp = up_params(self_pod, now), tk.chain_scaledown(now, 10_000_000, self_pod)
        up_vs_model(s.scaleup_plan_k(c, ckeys, sp), w.scaleup(c, ckeys, sp), "up")
        idx, rem = s.scaledown_plan_k(c, ckeys, dp)
        eq(idx, w.scaledown(c, ckeys, dp)[0]), eq(rem, w.scaledown(c, ckeys, dp)[1])
        idx, act, wait = s.migration_plan_k(c, ckeys, self_pod, now)
        midx, mact, mwait = w.migration(c, ckeys, self_pod, now)
        eq(idx, midx), eq(act, mact), eq(wait, mwait)
        assert idx[:6].tolist() == dele + [-1, -1, -1] and not act[:6].any() and not rem[:6].any()
        # a batch of unknown ids only: nothing resolves, nothing is edited, and the next call is correct (the map is clean)
        n = IDTAB_BLOCK + 3
        ghosts = e[np.arange(n) % len(e)].copy()
        gkeys = [b"ghost", b"ghost"] + [b"ghost-%d" % i for i in range(n - 2)]
        before = [x.copy() for x in s.get_models()]
        got = s.janitor_plan_k(ghosts, gkeys, jm.params(self_pod, now + 1))
        same_janitor(got, w.janitor(ghosts, gkeys, jm.params(self_pod, now + 1)), "ghosts")
        assert (got[0] == -1).all() and len(got[3]) == 0
        idx, act, wait = s.migration_plan_k(c[:n % len(c)], gkeys[:n % len(c)], self_pod, now)
        assert (idx == -1).all() and not act.any() and not wait.any()
        e2, k2, _ = jan_rows(w, fleet, self_pod, now + 2, 8)
        same_janitor(s.janitor_plan_k(e2, k2, jm.params(self_pod, now + 2)), w.janitor(e2, k2, jm.params(self_pod, now + 2)), "after")
        same_registry(s, w)
        assert len(before[0]) == len(s.get_models()[0])
    finally:
        s.close()


# ---- duplicates in the janitor -------------------------------------------------------------------------------------------------

def test_two_entries_of_one_record_are_refused_with_nothing_written_and_the_map_left_clean(big):
    a, b, w, fleet, self_pod, dele = big
    now = int(fleet.now) + 900
    prm = jm.params(self_pod, now)
    e, keys, rows = jan_rows(w, fleet, self_pod, now, 70, 300, skip=dele)
    live = [r for r in range(300) if rows[r] >= 0]
    assert live[-1] - live[2] >= IDTAB_BLOCK
    before = [x.copy() for x in a.get_models()]
    for dup in ([(live[1], live[0])], [(live[-1], live[2])], [(live[5], live[4]), (live[-2], live[4])]):   # adjacent; two workgroups; three times
        k2 = list(keys)
        for dst, src in dup:
            k2[dst] = keys[src]
        for flags, chain in ((JANITOR_APPLY, tk.chain_scaledown(now, 10_000_000, self_pod)), (JANITOR_APPLY, None), (0, None)):
            got = a.janitor_plan_k_raw(e, k2, prm, flags, 2000, 2000, chain, fill=FILL)
            assert got[-1] == _lib.MMP_EINVAL and untouched(*got[:7]), got[-1]
        with pytest.raises(InvalidEntries):
            copy.deepcopy(w).janitor(e, k2, prm)
        prm_down = jm.params(self_pod, now, shutting_down=1)
        got = a.janitor_plan_k_raw(e, k2, prm_down, 0, 2000, 2000, fill=FILL)                        # :5880 does not excuse it
        assert got[-1] == _lib.MMP_EINVAL and untouched(*got[:7])
    for x, y in zip(before, a.get_models()):
        assert x.tobytes() == y.tobytes()
    # the map is clean: a by-row dry run that follows equals the other context's
    e["model"] = rows
    ga, gb = a.janitor_plan_raw(e, prm, JANITOR_DRY, 2000, 2000), b.janitor_plan_raw(e, prm, JANITOR_DRY, 2000, 2000)
    for x, y in zip(ga, gb):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    # a run that is shutting down: every action NONE, the rows still answered
    e["model"] = -12345
    got = a.janitor_plan_k_raw(e, keys, jm.params(self_pod, now, shutting_down=1), JANITOR_APPLY, 2000, 2000,
                               tk.chain_scaledown(now, 10_000_000, self_pod), fill=FILL)
    assert got[-1] == 0 and not got[1].any() and np.array_equal(got[0], rows) and int(got[6]["n_action"][0]) == 300 and untouched(got[5])
    same_contexts(a, b)


# ---- keys ----------------------------------------------------------------------------------------------------------------------

def test_the_empty_key_utf8_keys_the_chunk_edge_one_long_key_and_offsets_that_do_not_start_at_zero(small):
    fleet, self_pod, w0, dele = small
    w, now = copy.deepcopy(w0), int(fleet.now)
    s = loaded(fleet, IDS)
    try:
        c = np.zeros(9, dtype=CACHE_ENTRY)
        c["last_used"], c["weight"] = now - 5_000_000, 10
        keys = [b"", "modèle-é".encode(), "modèle-e".encode(), b"k" * 14, b"k" * 15, b"k" * 16, b"k" * 17, b"k" * 18, LONG_ID]
        idx, act, wait = s.migration_plan_k(c, keys, self_pod, now)
        assert idx.tolist() == [0, 1, -1, -1, 3, 4, 5, -1, 2]
        midx, mact, mwait = w.migration(c, keys, self_pod, now)
        eq(idx, midx), eq(act, mact), eq(wait, mwait)
        # the long key leads a workgroup that reads in place; the next workgroup stages
        many = [LONG_ID] + [k for k in w.ids if k != LONG_ID][:IDTAB_BLOCK + 20]
        cm = np.zeros(len(many), dtype=CACHE_ENTRY)
        cm["last_used"], cm["weight"] = now - 5_000_000, 10
        for x, y in zip(s.migration_plan_k(cm, many, self_pod, now), w.migration(cm, many, self_pod, now)):
            eq(x, y)
        e, jkeys, rows = jan_rows(w, fleet, self_pod, now, 9)
        same_janitor(s.janitor_plan_k(e, jkeys, jm.params(self_pod, now), apply=False), w.janitor(e, jkeys, jm.params(self_pod, now), dry=True), "long")
        # key_off[0] != 0: the bytes in front belong to somebody else
        live = [k for k in w.ids if w.get(k) is not None and k != LONG_ID][:5]
        blob = b"junk-in-front" + b"".join(live)
        off = np.cumsum([13] + [len(x) for x in live]).astype(np.int32)
        got = s.migration_plan_k_raw(c[:5], live, self_pod, now, key_off=off, blob=blob)
        assert got[3] == 0
        eq(got[0], w.migration(c[:5], live, self_pod, now)[0]), eq(got[1], w.migration(c[:5], live, self_pod, now)[1])
        sp = up_params(self_pod, now)
        got = s.scaleup_plan_k_raw(c[:5], live, sp, key_off=off, blob=blob)
        assert got[-1] == 0
        up_vs_model((got[0], got[1], got[3], got[4]), w.scaleup(c[:5], live, sp), "offset")
        got = s.janitor_plan_k_raw(e[:5], live, jm.params(self_pod, now), 0, 400, 400, key_off=off, blob=blob)
        assert got[-1] == 0
        same_janitor(got, w.janitor(e[:5], live, jm.params(self_pod, now), dry=True), "offset")
    finally:
        s.close()


def test_staged_and_unstaged_keys_answer_alike():
    """256 keys of 200 bytes in one workgroup are past the staging region and are read where they lie; the same fleet under short
    ids is staged: the same rows, the same answers, in all four calls."""
    fleet, self_pod, w, dele = jan_world(64, 2000)
    wide = TaskWorld(fleet, [WIDE(i) for i in range(2000)], w.records_by_row())
    a, b = loaded(fleet, w.ids), loaded(fleet, wide.ids)
    try:
        now, rng = int(fleet.now), np.random.default_rng(12)
        c, ckeys, crows = cache_rows(w, rng, 2 * IDTAB_BLOCK + 9, self_pod)
        wkeys = keys_of(wide, crows)
        assert sum(len(k) for k in wkeys[:IDTAB_BLOCK]) > LDS_BYTES > sum(len(k) for k in ckeys[:IDTAB_BLOCK])
        sp, dp = up_params(self_pod, now), tk.chain_scaledown(now, 10_000_000, self_pod)
        for x, y in zip(a.scaleup_plan_k(c, ckeys, sp), b.scaleup_plan_k(c, wkeys, sp)):
            eq(x, y)
        for x, y in zip(a.scaledown_plan_k(c, ckeys, dp), b.scaledown_plan_k(c, wkeys, dp)):
            eq(x, y)
        for x, y in zip(a.migration_plan_k(c, ckeys, self_pod, now), b.migration_plan_k(c, wkeys, self_pod, now)):
            eq(x, y)
        e, jkeys, rows = jan_rows(w, fleet, self_pod, now, 31, 2 * IDTAB_BLOCK + 9)
        ga = a.janitor_plan_k(e, jkeys, jm.params(self_pod, now), scaledown=dp)
        gb = b.janitor_plan_k(e, keys_of(wide, rows), jm.params(self_pod, now), scaledown=dp)
        same_janitor(ga, gb, "wide")
        same_janitor(gb, wide.janitor(e, keys_of(wide, rows), jm.params(self_pod, now), scaledown=dp), "wide model")
        same_contexts(a, b)
    finally:
        a.close()
        b.close()


# ---- the window: worlds by key, where events and retirements can follow --------------------------------------------------------

def wire_world(n=40):
    """n records by key over the 8 instances of the status file's wire world; instance 1 holds a copy of every third."""
    fleet = sbg.W.fleet
    io = fleet.pods["id_order"]
    ids = [b"key-%d" % i for i in range(n)]
    recs = []
    for i in range(n):
        r = rp.Record(0, [], [], 1000 + i)
        for j, p in enumerate(range(8)):
            if (i + j) % 3 == 0:
                jm.put_in_id_order(r.loaded, p, 1000 * i + j + 1, io)
        recs.append(r)
    s = sbg.W.solver()
    status, _ = s.ingest_models_json([sbg.value_of(ModelRecord(0, r.loaded, r.failed, r.last_used)) for r in recs])
    assert not status.any()
    s.model_ids_load(ids)
    return s, TaskWorld(fleet, ids, recs)


def delete(s, w, key):
    s.models_events_json([key], [""], np.ones(1, np.uint8), True)
    w.delete(key)


def wire_rows(w, keys, now):
    """Old, live, done cache rows for `keys` (MRU first), in order with the registry where instance 1 holds a copy."""
    e = np.zeros(len(keys), dtype=JANITOR_ENTRY)
    for r, k in enumerate(keys):
        rec = w.get(k)
        lt = dict(rec.loaded).get(1, 777) if rec is not None else 777
        e[r] = (-12345, 10, now - 2_000_000 - r, lt, 0, -1, 0, 0, 0, 0, 0, _lib.JE_DONE | _lib.JE_STATE_LIVE, 0)
    c = np.zeros(len(keys), dtype=CACHE_ENTRY)
    c["model"], c["last_used"], c["weight"] = -12345, e["last_used"], 10
    return e, c


def test_a_retirement_between_resolve_and_the_by_row_call_answers_for_other_records_the_keyed_call_does_not():
    a, w = wire_world()
    b, _ = wire_world()
    try:
        now = 5_000_000
        gone = [b"key-2", b"key-3", b"key-11"]
        for s in (a, b):
            for key in gone:
                s.models_events_json([key], [""], np.ones(1, np.uint8), True)
        for key in gone:
            w.delete(key)
        keys = [b"key-%d" % i for i in (4, 6, 12, 15, 2, 30, 35)]  # (every stale row still in range)
        stale = b.model_ids_resolve(keys)                       # the host resolves ...
        rows = [w.row(k) for k in gone]
        for s in (a, b):
            s.models_retire(rows)                               # ... a retirement lands ...
        w.retire(rows)
        e, c = wire_rows(w, keys, now)
        want = w.migration(c, keys, 1, now)
        by_row = c.copy()
        by_row["model"] = stale                                 # ... and the by-row call answers for whoever has the rows now
        sact, _ = b.migration_plan(by_row, 1, now)
        assert not np.array_equal(sact, want[1])
        got = a.migration_plan_k(c, keys, 1, now)
        for x, y in zip(got, want):
            eq(x, y)
        assert got[0].tolist() == [2, 4, 9, 12, -1, 27, 32] and stale.tolist() == [4, 6, 12, 15, 2, 30, 35]
        dp = tk.chain_scaledown(now, 10_000_000, 1)
        eq(a.scaledown_plan_k(c, keys, dp)[1], w.scaledown(c, keys, dp)[1])
        up_vs_model(a.scaleup_plan_k(c, keys, up_params(1, now)), w.scaleup(c, keys, up_params(1, now)), "window")
        stale_e = e.copy()
        stale_e["model"] = stale
        sj = b.janitor_plan_raw(stale_e, jm.params(1, now), 0, 64, 64)
        wj = w.janitor(e, keys, jm.params(1, now), dry=True)
        assert not np.array_equal(sj[0], wj[1]) or sj[1]["model"].tolist() != wj[2]["model"].tolist()
        same_janitor(a.janitor_plan_k(e, keys, jm.params(1, now), scaledown=dp), w.janitor(e, keys, jm.params(1, now), scaledown=dp), "window")
        same_registry(a, w)
    finally:
        a.close()
        b.close()


def test_one_hundred_calls_beside_a_writer_each_answer_one_whole_state():
    """The writer deletes key-5, retires its row and registers it again (at the end of the table), over and over; key-9 sits
    behind it and moves between rows 9 and 8.  Every answer is that of ONE of the states the model passes through."""
    s, w = wire_world()
    try:
        now, stop, errors = 5_000_000, threading.Event(), []
        keys = [b"key-9", b"key-5", b"key-20", b"never"]
        e, c = wire_rows(w, keys, now)
        rec5 = copy.deepcopy(w.get(b"key-5"))
        states = []
        m = copy.deepcopy(w)
        for _ in range(2):                                      # the cycle's states repeat after the first pass
            for step in ("start", "deleted", "retired", "again"):
                if step == "deleted":
                    m.delete(b"key-5")
                elif step == "retired":
                    m.retire([m.row(b"key-5")])
                elif step == "again":
                    m.put(b"key-5", copy.deepcopy(rec5))
                states.append((tuple(x.tobytes() for x in m.migration(c, keys, 1, now)),
                               tuple(np.asarray(x).tobytes() for x in m.janitor(e, keys, jm.params(1, now), dry=True)[:5])))
        value = sbg.value_of(ModelRecord(0, rec5.loaded, rec5.failed, rec5.last_used))

        def writer():
            try:
                row = 5
                while not stop.is_set():
                    s.models_events_json([b"key-5"], [""], np.ones(1, np.uint8), True)
                    s.models_retire([row])
                    s.models_events_json([b"key-5"], [value], np.zeros(1, np.uint8), True)
                    row = 39
            except Exception as x:  # noqa: BLE001
                errors.append(x)
        t = threading.Thread(target=writer)
        t.start()
        seen = set()
        try:
            for call in range(100):
                got = tuple(x.tobytes() for x in s.migration_plan_k(c, keys, 1, now))
                jan = tuple(np.asarray(x).tobytes() for x in s.janitor_plan_k(e, keys, jm.params(1, now), apply=False)[:5])
                assert got in [st[0] for st in states], call
                assert jan in [st[1] for st in states], call
                seen.add(got)
        finally:
            stop.set()
            t.join()
        assert not errors, errors
        assert len(seen) >= 2                                   # the writer did get in between
    finally:
        s.close()


# ---- the chain -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def chain():
    w, now = tk.chain_world()
    return w, now


@pytest.mark.parametrize("k", CAND_COUNTS)
def test_the_chain_at_every_candidate_count_with_and_without_conc_and_under_a_permutation(chain, k):
    w0, now = chain
    prm = jm.params(CHAIN_SELF, now)
    e, keys = tk.chain_entries(w0, now, list(range(k)), recent=(1, 7))
    for cap, conc in ((10_000_000, None), (10_000_000, tk.conc_rows(k, queued=range(0, k, 5))), (600, None)):
        w = copy.deepcopy(w0)
        a, b = loaded(w0.fleet, w0.ids), loaded(w0.fleet, w0.ids)   # (every case from the start state)
        try:
            dp = tk.chain_scaledown(now, cap)
            got = a.janitor_plan_k_raw(e, keys, prm, JANITOR_APPLY, 128, 128, dp, conc, DYN, fill=FILL)
            assert got[-1] == 0 and int(got[6]["n_candidates"]) == k
            same_janitor(got, three_calls(b, e, keys, prm, JANITOR_APPLY, 128, dp, conc), (k, cap))
            want = w.janitor(e, keys, prm, scaledown=dp, conc=conc, dyn_const=DYN)
            same_janitor(got, want, (k, cap, "model"))
            same_contexts(a, b)
            same_registry(a, w)
            if k >= 63 and cap == 10_000_000:
                assert 0 < int(got[5].sum()) < k
                if conc is not None:                           # the rows with two queued requests stay: the candidates of THOSE rows
                    assert not got[5][np.isin(got[4], list(range(0, k, 5)))].any()
        finally:
            a.close()
            b.close()
    if k >= 2:                                                 # the input rows permuted, conc with them: the same copies go
        a = loaded(w0.fleet, w0.ids)
        try:
            perm = np.random.default_rng(k).permutation(k)
            conc = tk.conc_rows(k, queued=range(0, k, 5))
            e2 = e[perm].copy()
            e2["last_used"] = e["last_used"]
            k2 = [keys[i] for i in perm]
            got = a.janitor_plan_k_raw(e2, k2, prm, JANITOR_APPLY, 128, 128, tk.chain_scaledown(now), conc[perm], DYN, fill=FILL)
            assert got[-1] == 0
            same_janitor(got, copy.deepcopy(w0).janitor(e2, k2, prm, scaledown=tk.chain_scaledown(now), conc=conc[perm], dyn_const=DYN), (k, "perm"))
            kept = {k2[r] for r, x in zip(got[4], got[5]) if not x}
            assert {keys[r] for r in range(0, k, 5)} <= kept
        finally:
            a.close()


def test_the_chain_is_refused_without_apply_or_with_another_self_pod_and_a_truncated_or_stopped_run_decides_nothing(chain):
    w0, now = chain
    prm, dp = jm.params(CHAIN_SELF, now), tk.chain_scaledown(now)
    s = loaded(w0.fleet, w0.ids)
    try:
        e, keys = tk.chain_entries(w0, now, list(range(10)), recent=(1,))
        before = [x.copy() for x in s.get_models()]
        for flags, sd, conc in ((0, dp, None), (JANITOR_DRY, dp, None), (JANITOR_APPLY, tk.chain_scaledown(now, self_pod=CHAIN_SELF + 1), None),
                                (JANITOR_APPLY, None, tk.conc_rows(10))):
            got = s.janitor_plan_k_raw(e, keys, prm, flags, 128, 128, sd, conc, DYN, fill=FILL)
            assert got[-1] == _lib.MMP_EINVAL and untouched(*got[:7]), (flags, got[-1])
        got = s.janitor_plan_k_raw(e, keys, prm, JANITOR_APPLY, 128, 128, dp, null_removed=True, fill=FILL)
        assert got[-1] == _lib.MMP_EINVAL and untouched(*got[:7])
        # truncated: the prefix and the totals, nothing applied, removed_out untouched
        for me, mc in ((128, 4), (3, 128)):
            got = s.janitor_plan_k_raw(e, keys, prm, JANITOR_APPLY, me, mc, dp, fill=FILL)
            assert got[-1] == 0 and int(got[6]["truncated"]) == 1 and untouched(got[5])
            assert (int(got[6]["n_candidates"]), int(got[6]["n_edits"])) == (10, 61)
        for x, y in zip(before, s.get_models()):
            assert x.tobytes() == y.tobytes()
        # a run that stops at a repaired row has no candidates: nothing is decided
        stop = e.copy()
        stop["last_used"][0] = np.iinfo(np.int64).max
        got = s.janitor_plan_k_raw(stop, keys, prm, JANITOR_APPLY, 128, 128, dp, fill=FILL)
        w = copy.deepcopy(w0)
        want = w.janitor(stop, keys, prm, scaledown=dp)
        assert got[-1] == 0 and int(got[6]["stopped_at"]) == 0 and int(got[6]["n_candidates"]) == 0 and untouched(got[5])
        same_janitor(got, want, "stopped")
        same_registry(s, w)
    finally:
        s.close()


# ---- refusals, identity ----------------------------------------------------------------------------------------------------------

def test_nulls_one_key_pointer_offsets_that_fall_and_the_state_before_the_first_commit(small):
    fleet, self_pod, w, dele = small
    now = int(fleet.now)
    s = loaded(fleet, IDS)
    try:
        e, keys, rows = jan_rows(w, fleet, self_pod, now, 3, 20)
        c, ckeys, crows = cache_rows(w, np.random.default_rng(1), 20, self_pod)
        prm, sp, dp = jm.params(self_pod, now), up_params(self_pod, now), tk.chain_scaledown(now, 10_000_000, self_pod)
        bad_off = np.cumsum([0] + [len(k) for k in keys]).astype(np.int32)
        bad_off[7] = bad_off[6] - 1
        before = [x.copy() for x in s.get_models()]
        for kw in (dict(null_keys=True), dict(null_off=True), dict(key_off=bad_off)):
            got = s.janitor_plan_k_raw(e, keys, prm, JANITOR_APPLY, 64, 64, dp, fill=FILL, **kw)
            assert got[-1] == _lib.MMP_EINVAL and untouched(*got[:7]), kw
            got = s.scaleup_plan_k_raw(c, keys, sp, fill=FILL, **kw)
            assert got[-1] == _lib.MMP_EINVAL and untouched(got[0], got[1], got[3]) and got[4] == np.frombuffer(bytes([FILL] * 4), np.int32)[0], kw
            got = s.scaledown_plan_k_raw(c, keys, dp, fill=FILL, **kw)
            assert got[-1] == _lib.MMP_EINVAL and untouched(*got[:2]), kw
            got = s.migration_plan_k_raw(c, keys, self_pod, now, fill=FILL, **kw)
            assert got[-1] == _lib.MMP_EINVAL and untouched(*got[:3]), kw
        assert s.janitor_plan_k_raw(e, keys, prm, 0, 64, 64, null_info=True)[-1] == _lib.MMP_EINVAL
        assert s.scaleup_plan_k_raw(c, ckeys, sp, null_outs=True)[-1] == _lib.MMP_EINVAL
        assert s.scaleup_plan_k_raw(c, ckeys, sp, null_skipped=True)[-1] == _lib.MMP_EINVAL
        assert s.scaledown_plan_k_raw(c, ckeys, dp, null_removed=True)[-1] == _lib.MMP_EINVAL
        assert s.migration_plan_k_raw(c, ckeys, self_pod, now, null_action=True)[-1] == _lib.MMP_EINVAL
        # model_idx_out is optional
        assert s.janitor_plan_k_raw(e, keys, prm, 0, 64, 64, null_idx=True, fill=FILL)[-1] == 0
        got = s.migration_plan_k_raw(c, ckeys, self_pod, now, null_idx=True, fill=FILL)
        assert got[-1] == 0 and untouched(got[0])
        eq(got[1], s.migration_plan_k(c, ckeys, self_pod, now)[1])
        for x, y in zip(before, s.get_models()):
            assert x.tobytes() == y.tobytes()
    finally:
        s.close()
    fresh = Solver(fleet.min_space_units, fleet.min_churn_age_ms)        # before the first commit; and without a loaded id table
    try:
        assert fresh.migration_plan_k_raw(c, ckeys, self_pod, now)[-1] == _lib.MMP_ESTATE
        assert fresh.janitor_plan_k_raw(e, keys, prm, 0, 64, 64)[-1] == _lib.MMP_ESTATE
        fresh.load_fleet(fleet)
        for rc in (fresh.migration_plan_k_raw(c, ckeys, self_pod, now)[-1], fresh.janitor_plan_k_raw(e, keys, prm, 0, 64, 64)[-1],
                   fresh.scaleup_plan_k_raw(c, ckeys, sp)[-1], fresh.scaledown_plan_k_raw(c, ckeys, dp)[-1]):
            assert rc == _lib.MMP_ESTATE
        by_row = c.copy()
        by_row["model"] = crows
        assert fresh.migration_plan_k_raw(by_row, None, self_pod, now)[-1] == 0                                  # by row no id table is needed
        with pytest.raises(MmpError):
            fresh.migration_plan_k(c, ckeys, self_pod, now)
    finally:
        fresh.close()


def test_the_same_calls_on_the_same_state_twice_are_byte_identical(small):
    fleet, self_pod, w, dele = small
    now = int(fleet.now)
    s = loaded(fleet, IDS)
    try:
        e, keys, _ = jan_rows(w, fleet, self_pod, now, 5)
        c, ckeys, _ = cache_rows(w, np.random.default_rng(4), 257, self_pod)
        prm, sp, dp = jm.params(self_pod, now), up_params(self_pod, now), tk.chain_scaledown(now, 10_000_000, self_pod)
        runs = []
        for fill in (FILL, 0x3C):
            j = s.janitor_plan_k_raw(e, keys, prm, 0, 400, 400, fill=fill)
            u = s.scaleup_plan_k_raw(c, ckeys, sp, conc_random(np.random.default_rng(6), 257), conc_par(), fill=fill)
            d = s.scaledown_plan_k_raw(c, ckeys, dp, fill=fill)
            m = s.migration_plan_k_raw(c, ckeys, self_pod, now, fill=fill)
            assert j[-1] == u[-1] == d[-1] == m[-1] == 0 and int(j[6]["n_edits"]) > 20
            runs.append([np.asarray(x).tobytes() for x in j[:5] + u[:4] + (u[5],) + d[:2] + m[:3]] + [u[4]])
        assert runs[0] == runs[1]
        same_registry(s, w)
    finally:
        s.close()
