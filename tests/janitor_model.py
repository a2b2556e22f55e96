"""janitorTask's cache loop and registry loop (MM.java:5892-6008, :6014-6108), restated in Python.

Two forms.  `Janitor.run` is literal and sequential: the registry is a list of Records whose instanceIds and
loadFailedInstanceIds are ordered (pod, time) lists standing for the TreeMaps, the cache an ordered dict (MRU first) with
the snapshot of :5892 beside it; it cites the Java line at every step.  `closed_rule` is the vectorised numpy form of the
closed rule the device code uses (include/mmplace.h, mmp_janitor_plan): the cache is keyed by model id, so a model meets at
most one cache entry and its record is decided from that entry alone; what couples the models is the Long.MAX_VALUE stop
(:5929, a minimum over the entry index) and the TreeSet's tie drop (:6017, VALUE_COMP :6875-6881).
tests/test_janitor_model.py holds the two against each other.

The reference has no test that names this code (nothing under its src/test mentions janitorTask, scaleCopiesCandidates,
updateLastUsedTimeInRegistryIfStale or unloadAttemptedRecently).  The vectors are the text's own answers: the two loops are cut
out of the reference tree and compiled by oracle/ref_harness/registry_harness.cc, tests/golden/ref_registry_edges.npz holds what
they did at the value edges (tests/ref_registry_edges.py), and tests/test_registry_edges.py holds both forms below to every row.

One run uses ONE clock value (the library's convention); the Java reads currentTimeMillis() at :5899 and :6018.  Not restated:
verifyKvStoreConnection (:5886), the conditional-set retries (:5983-5996, :6074-6078; a record is what the registry holds),
registry.getStrong (:5944), an entry added to the cache while the run is under way (runtimeCache.getQuietly, :6036) and the
mid-run shuttingDown checks.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

from modelmesh_amd import _lib
from modelmesh_amd._lib import (CACHE_ENTRY, JAN_EDIT_REGISTERED, JAN_EDIT_REM_FAILED, JAN_EDIT_REM_LOADED, JAN_EDIT_REPAIRED,
                                JAN_EDIT_TIMESTAMP_MISMATCH, JAN_EDIT_TOUCHED, JAN_EDIT_UNLOAD_SET, JAN_EXPIRED, JAN_IN_ORDER,
                                JAN_NONE, JAN_REFRESHED, JAN_REGISTERED, JAN_REMOVED, JAN_REPAIRED, JANITOR_EDIT, JANITOR_PARAMS,
                                JE_DONE, JE_FAILED, JE_STATE_LIVE)
from tests.registry_prune_model import LONG_MAX, jsub

JANITOR_FREQ_SECS = 360                 # LOCAL_JANITOR_FREQ_SECS
LOAD_FAILURE_EXPIRY_MS = 900_000        # :219; IN_USE_LOAD_FAILURE_EXPIRY_MS is half of it (:221)
SHORT_EXPIRY_RECENT_USE_TIME_MS = 180_000
UNLOAD_ATTEMPT_RECENT_MS = 600_000      # :1865
LASTUSED_AGE_ON_ADD_MS = 3_600_000
CAND_FIELDS = ("weight", "interval_count", "last_heavy_time", "last_unload_time", "earlier_use_iteration", "last_used_iteration")


def params(self_pod, now, load_timeout_ms=240_000, min_stale_age_ms=6 * 3_600_000 + 1_234_567, shutting_down=0,
           janitor_freq_secs=JANITOR_FREQ_SECS, load_failure_expiry_ms=LOAD_FAILURE_EXPIRY_MS,
           short_expiry_recent_use_ms=SHORT_EXPIRY_RECENT_USE_TIME_MS, unload_attempt_recent_ms=UNLOAD_ATTEMPT_RECENT_MS,
           lastused_age_on_add_ms=LASTUSED_AGE_ON_ADD_MS):
    p = np.zeros(1, dtype=JANITOR_PARAMS)
    p[0] = (self_pod, shutting_down, now, janitor_freq_secs, load_timeout_ms, min_stale_age_ms, load_failure_expiry_ms,
            short_expiry_recent_use_ms, unload_attempt_recent_ms, lastused_age_on_add_ms)
    return p


def _get(lst, pod):
    for p, t in lst:
        if p == pod:
            return t
    return None


def _remove(lst, pod):
    lst[:] = [(p, t) for p, t in lst if p != pod]


def put_in_id_order(lst, pod, time, id_order):
    """TreeMap.put: the value is replaced where the key stands; a new key goes in front of the first RESOLVED entry whose id
    is greater.  Entries whose pod is not in the pod table (index < 0 or beyond it) keep their place and are never compared."""
    for k, (p, _) in enumerate(lst):
        if p == pod:
            lst[k] = (pod, time)
            return k
    for k, (p, _) in enumerate(lst):
        if 0 <= p < len(id_order) and id_order[p] > id_order[pod]:
            lst.insert(k, (pod, time))
            return k
    lst.append((pod, time))
    return len(lst) - 1


class _Edit:
    def __init__(self, entry):
        self.flags, self.last_unload, self.ins_time, self.entry = 0, 0, 0, entry


class Janitor:
    """One instance's janitor.  `run` edits `registry` (a list of registry_prune_model.Record) in place unless dry and returns
    (actions uint8[n], edits JANITOR_EDIT[], candidates CACHE_ENTRY[], candidate rows int32[], info dict)."""

    def run(self, registry, entries, prm, id_order, dry=False):
        prm = np.asarray(prm).reshape(-1)[0]
        self_pod, now = int(prm["self_pod"]), int(prm["now"])
        n = len(entries)
        actions = np.zeros(n, np.uint8)
        info = dict(n_edits=0, n_candidates=0, n_ties=0, stopped_at=-1, truncated=0)
        none = (actions, np.zeros(0, JANITOR_EDIT), np.zeros(0, CACHE_ENTRY), np.zeros(0, np.int32), info)
        if prm["shutting_down"]:                                        # :5880
            info["n_action"] = [n, 0, 0, 0, 0, 0, 0]
            return none
        if dry:
            import copy
            registry = copy.deepcopy(registry)
        min_stale, freq, load_timeout = int(prm["min_stale_age_ms"]), int(prm["janitor_freq_secs"]), int(prm["load_timeout_ms"])
        # cacheEntries: the snapshot of :5892 (row per model id); runtimeCache: what is in the cache NOW (ordered, MRU first)
        snapshot = {}
        cache = OrderedDict()
        for r in range(n):
            key = int(entries[r]["model"]) if entries[r]["model"] >= 0 else ("unregistered", r)
            snapshot[key] = r
            cache[key] = int(entries[r]["last_used"])
        edited = {}                                                     # model -> _Edit

        def ed(model, row):
            return edited.setdefault(model, _Edit(row))

        def get_last_used_time(key):                                    # runtimeCache.getLastUsedTime: -1 when absent
            return cache.get(key, -1)

        def update_last_used(model, last_used):                         # ModelRecord.java:239-246
            if last_used == 0:
                last_used = now
            if last_used > registry[model].last_used:
                registry[model].last_used = last_used
                ed(model, snapshot.get(model, -1)).flags |= JAN_EDIT_TOUCHED

        def update_if_stale(model, last_used):                          # :6165-6181
            if last_used == LONG_MAX:                                   # :6167
                return False
            if jsub(last_used, registry[model].last_used) < min_stale:  # :6174
                return False
            update_last_used(model, last_used)                          # :6177
            return True

        def unload_attempted_recently(t):                               # :1864-1866 with age() of :4162-4164
            age = 0 if t == 0 else jsub(now, t)
            return age < int(prm["unload_attempt_recent_ms"])

        stopped = False
        for key, r in list(snapshot.items()):                           # :5902 most to least recently used
            ce = entries[r]
            if not ce["flags"] & JE_DONE:                               # :5905
                continue
            last_used = get_last_used_time(key)                         # :5909
            if last_used <= 0:                                          # :5910
                continue
            model = int(ce["model"])
            mr = registry[model] if model >= 0 else None                # :5919
            if last_used == LONG_MAX:                                   # :5921
                cache[key] = jsub(now, 3 * int(prm["lastused_age_on_add_ms"]))  # :5924 forceSetLastUsedTime
                if mr is not None and mr.last_used == LONG_MAX:         # :6843
                    mr.last_used = jsub(now, 3 * int(prm["lastused_age_on_add_ms"]))  # :6844
                    ed(model, r).flags |= JAN_EDIT_REPAIRED
                actions[r] = JAN_REPAIRED
                info["stopped_at"] = r
                stopped = True
                break                                                   # :5929 return
            if jsub(now, last_used) < freq * 2000 + load_timeout:       # :5933 (strict)
                if mr is not None and update_if_stale(model, last_used):  # :5936-5937
                    actions[r] = JAN_REFRESHED
                continue
            failed = bool(ce["flags"] & JE_FAILED)                      # :5941
            reg_load_timestamp = None
            if mr is not None:                                          # :5949
                insts = mr.failed if failed else mr.loaded              # :5950
                local = int(ce["load_complete_timestamp"] if failed else ce["load_timestamp"])  # :5952
                reg_timestamp = _get(insts, self_pod)                   # :5953
                if reg_timestamp is not None and reg_timestamp == local:  # :5954
                    actions[r] = JAN_REFRESHED if update_if_stale(model, last_used) else JAN_IN_ORDER  # :5955
                    continue
                if not failed:
                    reg_load_timestamp = reg_timestamp                  # :5959
            live = bool(ce["flags"] & JE_STATE_LIVE)
            if mr is None or not live or unload_attempted_recently(int(ce["last_unload_attempt_time"])):  # :5968-5969
                del cache[key]                                          # :5970 ce.remove()
                actions[r] = JAN_REMOVED
                continue
            e = ed(model, r)
            put_in_id_order(mr.loaded, self_pod, int(ce["load_timestamp"]), id_order)  # :5980
            _remove(mr.failed, self_pod)                                # :5981
            update_last_used(model, last_used)                          # :5982
            e.flags |= JAN_EDIT_REGISTERED | (JAN_EDIT_TIMESTAMP_MISMATCH if reg_load_timestamp is not None else 0)  # :5985-5993
            e.ins_time = int(ce["load_timestamp"])
            actions[r] = JAN_REGISTERED

        candidates = []                                                 # scaleCopiesCandidates in insertion (registry) order
        if not stopped:
            for model, mr in enumerate(registry):                       # :6020
                loaded = _get(mr.loaded, self_pod) is not None          # :6028
                failed_time = _get(mr.failed, self_pod)                 # :6029
                if not loaded and failed_time is None:                  # :6030
                    continue
                r = snapshot.get(model)                                 # :6034 cacheEntries.get
                ce = entries[r] if r is not None else None
                ce_failed = ce is not None and bool(ce["flags"] & JE_FAILED)
                last_used = -2                                          # :6038
                rem_loaded = loaded and (ce is None or ce_failed)       # :6039
                rem_failed = False
                if failed_time is not None:                             # :6041
                    if ce is not None and not ce_failed:                # :6042
                        rem_failed = True
                    else:
                        last_used = get_last_used_time(model) if ce is not None else -1  # :6045
                        short = last_used > 0 and jsub(now, last_used) < int(prm["short_expiry_recent_use_ms"])  # :6047
                        expiry_age = int(prm["load_failure_expiry_ms"]) // 2 if short else int(prm["load_failure_expiry_ms"])
                        if jsub(now, failed_time) > expiry_age:         # :6049 (strict)
                            rem_failed = True
                if rem_loaded or rem_failed:                            # :6054
                    e = ed(model, r if r is not None else -1)
                    if rem_loaded:
                        _remove(mr.loaded, self_pod)                    # :6060
                        e.last_unload = 0 if len(mr.loaded) <= 2 else now  # :6061, ModelRecord.java:260-262
                        e.flags |= JAN_EDIT_REM_LOADED | JAN_EDIT_UNLOAD_SET
                    if rem_failed:
                        _remove(mr.failed, self_pod)                    # :6064
                        e.flags |= JAN_EDIT_REM_FAILED
                    if ce is not None:                                  # :6066
                        if last_used == -2:
                            last_used = get_last_used_time(model)       # :6068
                        if last_used > 0:
                            update_last_used(model, last_used)          # :6071
                if rem_failed and ce is not None and ce_failed:         # :6089
                    if model in cache:                                  # :6091 ce.remove()
                        del cache[model]
                        actions[r] = JAN_EXPIRED
                elif loaded and not rem_loaded:                         # :6092
                    if last_used <= 0:
                        last_used = get_last_used_time(model)           # :6094
                    if last_used > 0:
                        candidates.append((last_used, r))               # :6097
        # the TreeSet under VALUE_COMP (:6875-6881): add() of an element that compares equal to one present is dropped
        tree, n_ties = {}, 0
        for last_used, r in candidates:
            if last_used in tree:
                n_ties += 1
            else:
                tree[last_used] = r
        order = sorted(tree)                                            # :6121 oldest first
        cands = np.zeros(len(order), dtype=CACHE_ENTRY)
        rows = np.zeros(len(order), np.int32)
        for k, last_used in enumerate(order):
            r = tree[last_used]
            rows[k] = r
            cands[k]["model"], cands[k]["last_used"] = entries[r]["model"], last_used
            for f in CAND_FIELDS:
                cands[k][f] = entries[r][f]
        edits = np.zeros(len(edited), dtype=JANITOR_EDIT)
        for k, model in enumerate(sorted(edited)):
            e, mr = edited[model], registry[model]
            pos = -1
            if e.flags & JAN_EDIT_REGISTERED and not e.flags & JAN_EDIT_REM_LOADED:
                pos = [p for p, _ in mr.loaded].index(self_pod)
            edits[k] = (model, len(mr.loaded), len(mr.failed), e.flags, mr.last_used, e.last_unload,
                        e.ins_time if e.flags & JAN_EDIT_REGISTERED else 0, pos, e.entry)
        info.update(n_edits=len(edits), n_candidates=len(order), n_ties=n_ties,
                    n_action=[int((actions == a).sum()) for a in range(7)])
        return actions, edits, cands, rows, info


def apply_to_cache(entries, actions, prm):
    """The cache after the run, as rows: removed and expired entries leave, the repaired one gets its new time."""
    prm = np.asarray(prm).reshape(-1)[0]
    out = entries.copy()
    rep = actions == JAN_REPAIRED
    out["last_used"][rep] = jsub(int(prm["now"]), 3 * int(prm["lastused_age_on_add_ms"]))
    return out[(actions != JAN_REMOVED) & (actions != JAN_EXPIRED)]


def closed_rule(models, ent_pod, ent_time, entries, prm, id_order):
    """The same run as array arithmetic over the registry arrays (rows may lie anywhere in the arena).
    Returns (actions, edits, candidates, candidate rows, info)."""
    prm = np.asarray(prm).reshape(-1)[0]
    self_pod, now = int(prm["self_pod"]), np.int64(prm["now"])
    M, n, P = len(models), len(entries), len(id_order)
    info = dict(n_edits=0, n_candidates=0, n_ties=0, stopped_at=-1, truncated=0)
    actions = np.zeros(n, np.uint8)
    if prm["shutting_down"]:
        info["n_action"] = [n, 0, 0, 0, 0, 0, 0]
        return actions, np.zeros(0, JANITOR_EDIT), np.zeros(0, CACHE_ENTRY), np.zeros(0, np.int32), info
    repaired_lu = np.int64(jsub(int(now), 3 * int(prm["lastused_age_on_add_ms"])))
    # the record's entries for self_pod: position and time in each list
    nl, nf, off = models["n_loaded"].astype(np.int64), models["n_failed"].astype(np.int64), models["ent_off"].astype(np.int64)
    k = nl + nf
    seg = np.repeat(np.arange(M), k)
    start = np.zeros(M + 1, np.int64)
    np.cumsum(k, out=start[1:])
    pos = np.arange(int(start[-1])) - start[seg]
    idx = off[seg] + pos
    pod, time = ent_pod[idx].astype(np.int64), ent_time[idx].astype(np.int64)
    in_loaded = pos < nl[seg]
    is_self = pod == self_pod
    li = np.full(M, -1, np.int64)
    lt = np.zeros(M, np.int64)
    fi = np.full(M, -1, np.int64)
    ft = np.zeros(M, np.int64)
    s = is_self & in_loaded
    li[seg[s]], lt[seg[s]] = pos[s], time[s]
    s = is_self & ~in_loaded
    fi[seg[s]], ft[seg[s]] = pos[s] - nl[seg[s]], time[s]
    # where a new entry for self_pod would go: in front of the first resolved loaded entry with a greater id
    resolved = (pod >= 0) & (pod < P)
    order_of = np.asarray(id_order, np.int64)
    greater = in_loaded & resolved & (order_of[np.where(resolved, pod, 0)] > order_of[self_pod])
    ins = nl.copy()
    np.minimum.at(ins, seg[greater], pos[greater])
    # the join: model -> entry row
    row_of = np.full(M, -1, np.int64)
    em = entries["model"].astype(np.int64)
    has_model = em >= 0
    row_of[em[has_model]] = np.nonzero(has_model)[0]
    fl = entries["flags"]
    done, e_failed, live = (fl & JE_DONE) != 0, (fl & JE_FAILED) != 0, (fl & JE_STATE_LIVE) != 0
    lu = entries["last_used"].astype(np.int64)
    # the stop (:5929): a minimum over the entry index
    stops = done & (lu == LONG_MAX)
    stop = int(np.nonzero(stops)[0][0]) if stops.any() else n
    stopped = stop < n
    info["stopped_at"] = stop if stopped else -1
    with np.errstate(over="ignore"):
        walked = done & (lu > 0) & (np.arange(n) <= stop)
        safe_m = np.where(has_model, em, 0)
        rec_lu = np.where(has_model, models["last_used"][safe_m] if M else 0, 0).astype(np.int64)
        recent = (now - lu) < np.int64(int(prm["janitor_freq_secs"]) * 2000 + int(prm["load_timeout_ms"]))
        stale = (lu != LONG_MAX) & ~((lu - rec_lu) < np.int64(prm["min_stale_age_ms"])) & has_model
        has_l, has_f = (li[safe_m] >= 0) & has_model if M else np.zeros(n, bool), (fi[safe_m] >= 0) & has_model if M else np.zeros(n, bool)
        reg_has = np.where(e_failed, has_f, has_l)
        reg_ts = np.where(e_failed, ft[safe_m], lt[safe_m]) if M else np.zeros(n, np.int64)
        local = np.where(e_failed, entries["load_complete_timestamp"], entries["load_timestamp"]).astype(np.int64)
        equal = reg_has & (reg_ts == local)
        luat = entries["last_unload_attempt_time"].astype(np.int64)
        attempted = np.where(luat == 0, 0, now - luat) < np.int64(prm["unload_attempt_recent_ms"])
    is_stop = walked & (np.arange(n) == stop) & stops
    c_recent = walked & ~is_stop & recent
    c_equal = walked & ~is_stop & ~recent & equal
    c_remove = walked & ~is_stop & ~recent & ~equal & (~has_model | ~live | attempted)
    c_register = walked & ~is_stop & ~recent & ~equal & ~c_remove
    refreshed = (c_recent | c_equal) & stale
    actions[is_stop] = JAN_REPAIRED
    actions[c_equal] = JAN_IN_ORDER
    actions[refreshed] = JAN_REFRESHED
    actions[c_remove] = JAN_REMOVED
    actions[c_register] = JAN_REGISTERED
    # per model: the record after the cache loop
    r = row_of
    mr = np.where(r >= 0, r, 0)
    has_row = r >= 0

    def of_row(mask):
        return has_row & mask[mr] if n else np.zeros(M, bool)

    flags = np.zeros(M, np.uint32)
    m_lu = models["last_used"].astype(np.int64).copy()
    e_lu = lu[mr] if n else np.zeros(M, np.int64)
    rep = of_row(is_stop) & (m_lu == LONG_MAX)
    m_lu[rep] = repaired_lu
    flags[rep] |= JAN_EDIT_REPAIRED
    raise_ = (of_row(refreshed) | of_row(c_register)) & (e_lu > m_lu)
    m_lu[raise_] = e_lu[raise_]
    flags[raise_] |= JAN_EDIT_TOUCHED
    reg = of_row(c_register)
    flags[reg] |= JAN_EDIT_REGISTERED
    flags[reg & ~of_row(e_failed) & (li >= 0)] |= JAN_EDIT_TIMESTAMP_MISMATCH
    loaded = (li >= 0) | reg
    failed_has = (fi >= 0) & ~reg
    in_cache = has_row & ~of_row(c_remove)
    # the registry loop
    if not stopped:
        ce = has_row
        ce_failed = of_row(e_failed)
        glut = np.where(in_cache, e_lu, -1)
        rem_loaded = loaded & (~ce | ce_failed)
        with np.errstate(over="ignore"):
            short = (glut > 0) & ((now - glut) < np.int64(prm["short_expiry_recent_use_ms"]))
            expiry = np.where(short, np.int64(prm["load_failure_expiry_ms"]) // 2, np.int64(prm["load_failure_expiry_ms"]))
            rem_failed = failed_has & ((ce & ~ce_failed) | ((now - ft) > expiry))
        changed = rem_loaded | rem_failed
        flags[rem_loaded] |= JAN_EDIT_REM_LOADED | JAN_EDIT_UNLOAD_SET
        flags[rem_failed] |= JAN_EDIT_REM_FAILED
        touch = changed & ce & (glut > 0) & (glut > m_lu)
        m_lu[touch] = glut[touch]
        flags[touch] |= JAN_EDIT_TOUCHED
        expired = rem_failed & ce & ce_failed & in_cache
        actions[r[expired]] = JAN_EXPIRED
        cand = ~(rem_failed & ce & ce_failed) & loaded & ~rem_loaded & (glut > 0)
    else:
        rem_loaded = rem_failed = cand = np.zeros(M, bool)
        glut = np.zeros(M, np.int64)
    nl_after = nl + (reg & (li < 0)) - rem_loaded
    nf_after = nf - ((fi >= 0) & (reg | rem_failed))
    em_ = np.nonzero(flags)[0]
    edits = np.zeros(len(em_), dtype=JANITOR_EDIT)
    edits["model"], edits["n_loaded_after"], edits["n_failed_after"], edits["flags"] = em_, nl_after[em_], nf_after[em_], flags[em_]
    edits["last_used_after"] = m_lu[em_]
    edits["last_unload_after"] = np.where(rem_loaded[em_] & (nl_after[em_] > 2), now, 0)
    regs = reg[em_]
    edits["inserted_time"] = np.where(regs, entries["load_timestamp"][mr[em_]] if n else 0, 0)
    edits["inserted_pos"] = np.where(regs & ~rem_loaded[em_], np.where(li[em_] >= 0, li[em_], ins[em_]), -1)
    edits["entry"] = r[em_]
    # candidates: first in registry order per distinct time, oldest first
    cm = np.nonzero(cand)[0]
    vals, first = np.unique(glut[cm], return_index=True)
    rows = r[cm[first]].astype(np.int32)
    cands = np.zeros(len(vals), dtype=CACHE_ENTRY)
    if len(vals):
        cands["model"], cands["last_used"] = entries["model"][rows], vals
        for f in CAND_FIELDS:
            cands[f] = entries[f][rows]
    info.update(n_edits=len(edits), n_candidates=len(vals), n_ties=len(cm) - len(vals),
                n_action=[int((actions == a).sum()) for a in range(7)])
    return actions, edits, cands, rows, info


def check_entries(entries, n_models):
    """What mmp_janitor_plan refuses: a model index outside [-1, M) or a model in two rows."""
    m = entries["model"]
    if ((m < -1) | (m >= n_models)).any():
        return False
    named = m[m >= 0]
    return len(np.unique(named)) == len(named)


# ---- the test recipe (tests/test_janitor_model.py checks that it shows every outcome for every seed the GPU tests use) ----

GPU_FLEETS = [(0, 8, 300), (1, 40, 600), (2, 300, 2000), (3, 2000, 20000), (4, 10_000, 100_000)]
RUN_EVERY_MS = JANITOR_FREQ_SECS * 1000
OLD_MS = 1_000_000          # beyond janitor_freq_secs * 2000 + load_timeout_ms = 960 000


def janitor_fleet(seed, pods, models, base=None, cache_size=3000):
    """A fleet whose pod `self_pod` holds a cache of up to `cache_size` entries.  Returns (fleet, self_pod, registry): self_pod
    is registered as loaded on about 70 % of `cache_size` models and carries a failure record on about 15 % (times on both
    sides of both expiries for the runs at now, now + 6 min, now + 12 min); some records are stale by more than min_stale_age;
    a few models that will be registered hold an entry whose pod is not in the pod table."""
    from modelmesh_amd import workload as wl
    from tests import registry_prune_model as rp
    rng = np.random.default_rng(91_000 + seed)
    fleet = base if base is not None else wl.fuzz_fleet(seed + 500, pods=pods, models=models)
    now, M = int(fleet.now), fleet.n_models
    self_pod = int(rng.integers(0, fleet.n_pods))
    id_order = fleet.pods["id_order"]
    reg = rp.registry_from_arrays(fleet.models, fleet.ent_pod, fleet.ent_time)
    for r in reg:                                   # self_pod only where the recipe puts it
        _remove(r.loaded, self_pod)
        _remove(r.failed, self_pod)
        if r.last_used == LONG_MAX or r.last_used <= 0:
            r.last_used = now - 3_600_000
    k = min(cache_size, M // 2)
    chosen = rng.permutation(M)[:k]
    n_l, n_f = int(0.7 * k), int(0.15 * k)
    for m in chosen[:n_l]:
        put_in_id_order(reg[m].loaded, self_pod, now - int(rng.integers(2_000_000, 90_000_000)), id_order)
    for m in chosen[n_l:n_l + n_f]:
        put_in_id_order(reg[m].failed, self_pod, now - int(rng.choice([100_000, 400_000, 500_000, 800_000, 1_000_000, 2_000_000])), id_order)
    many = [int(m) for m in chosen[:4]]               # three other copies: lastUnloadTime = now when self_pod's goes
    for m in many:
        for other in [q for q in range(fleet.n_pods) if q != self_pod][:3]:
            put_in_id_order(reg[m].loaded, other, now - 3_000_000, id_order)
    for m in chosen[:k:9]:
        reg[m].last_used = now - 10 * 3_600_000     # stale beside a cache time of ~17 min ago
    unresolved = []
    for m in chosen[n_l + n_f:]:                    # models self_pod is not registered on: rows for them get registered
        if len(reg[m].loaded) >= 1 and len(unresolved) < 4:
            reg[m].loaded[int(rng.integers(0, len(reg[m].loaded)))] = (-1, now - 5_000_000)
            unresolved.append(int(m))
    fleet.models, fleet.ent_pod, fleet.ent_time = rp.registry_to_arrays(reg)
    fleet.jan_chosen, fleet.jan_unresolved, fleet.jan_many = chosen, unresolved, many
    return fleet, self_pod, reg


def make_cache(fleet, reg, self_pod, seed, now):
    """Cache rows (MRU first) built from the registry's own entries for self_pod at `now` and then perturbed: every kind of
    disagreement between cache and registry the two loops know."""
    from modelmesh_amd._lib import JANITOR_ENTRY
    rng = np.random.default_rng(seed)
    rows = []
    old = iter(now - OLD_MS - 7 * rng.permutation(len(fleet.jan_chosen) + 16) - 7)   # distinct old times
    full = JE_DONE | JE_STATE_LIVE

    def row(model, last_used, lt=0, lct=0, flags=full, luat=-1):
        rows.append((model, int(rng.integers(1, 400)), last_used, lt, lct, luat, int(rng.integers(0, 50)), now - 7_000_000,
                     int(rng.choice([0, now - 100_000, now - 5_000_000])), int(rng.integers(0, 9)), int(rng.integers(0, 9)), flags, 0))

    for m in fleet.jan_chosen:
        m = int(m)
        lt, ft = _get(reg[m].loaded, self_pod), _get(reg[m].failed, self_pod)
        u = rng.random()
        if m in fleet.jan_unresolved and lt is None and ft is None:
            row(m, next(old), lt=now - 3_000_000)                                     # registered beside an unresolved entry
        elif lt is not None and m in fleet.jan_many:
            pass                                                                      # no row: remLoaded with three copies left
        elif lt is not None:
            if u < 0.50: row(m, next(old), lt=lt)                                     # in order (refreshed where the record is stale)
            elif u < 0.56: pass                                                       # no row: remLoaded
            elif u < 0.64: row(m, next(old), lt=lt + 5)                               # registered, timestamp mismatch
            elif u < 0.68: row(m, next(old), lt=lt + 5, flags=JE_DONE)                # removed: not live
            elif u < 0.72: row(m, next(old), lt=lt + 5, luat=int(rng.choice([0, now - 1000, now - 599_999])))  # removed: unload attempt
            elif u < 0.74: row(m, next(old), lt=lt + 5, luat=now - 600_000)           # registered: the attempt is exactly 10 min old
            elif u < 0.84: row(m, now - int(rng.integers(1, 959_999)), lt=lt + int(rng.integers(0, 2)))  # recently used
            elif u < 0.88: row(m, next(old), lt=lt + 5, flags=JE_STATE_LIVE)          # not done
            elif u < 0.91: row(m, int(rng.choice([0, -1])), lt=lt)                    # no longer in the cache
            elif u < 0.95: row(m, next(old), lt=lt, lct=lt, flags=JE_DONE | JE_FAILED)  # a failed entry under a registration
            else: row(m, now - 960_000, lt=lt + 5)                                    # exactly at the recently-used boundary
        elif ft is not None:
            if u < 0.35: row(m, next(old), lct=ft, flags=JE_DONE | JE_FAILED)         # full expiry rule
            elif u < 0.60: row(m, now - int(rng.choice([1000, 179_999, 180_000])), lct=ft, flags=JE_DONE | JE_FAILED)  # short rule / its edge
            elif u < 0.72: pass                                                       # no row: lastUsed = -1
            elif u < 0.87: row(m, next(old), lct=ft + 1, flags=JE_DONE | JE_FAILED)   # removed, then met by the registry loop
            else: row(m, next(old), lt=now - 4_000_000)                               # a live copy under a failure record
        else:
            if u < 0.7: row(m, next(old), lt=now - 3_000_000)                         # registered, no timestamp there
            else: row(m, next(old), lt=now - 3_000_000, flags=JE_DONE)                # removed
    for _ in range(3):
        row(-1, next(old))                                                            # registry.get == null
    row(-1, now - 500)
    e = np.array(rows, dtype=JANITOR_ENTRY).reshape(-1)
    # ties: pairs of in-order rows share a time
    plain = np.nonzero((e["flags"] == full) & (e["last_used"] < now - OLD_MS) & (e["last_unload_attempt_time"] == -1))[0]
    for a, b in zip(plain[0:12:2], plain[1:12:2]):
        e["last_used"][b] = e["last_used"][a]
    return e[np.argsort(-e["last_used"], kind="stable")]


def visibility(reg_before, edits, actions, info, now):
    """What one run showed, for the visibility condition."""
    fl = edits["flags"]
    reg_ = (fl & JAN_EDIT_REGISTERED) != 0
    rl = (fl & JAN_EDIT_REM_LOADED) != 0
    rf = (fl & JAN_EDIT_REM_FAILED) != 0
    beside = sum(1 for ed in edits[reg_ & (edits["inserted_pos"] >= 0)] if any(p < 0 for p, _ in reg_before[ed["model"]].loaded))
    return dict(removed=int((actions == JAN_REMOVED).sum()), registered_mismatch=int((reg_ & ((fl & JAN_EDIT_TIMESTAMP_MISMATCH) != 0)).sum()),
                registered_new=int((reg_ & ((fl & JAN_EDIT_TIMESTAMP_MISMATCH) == 0)).sum()), refresh=int((actions == JAN_REFRESHED).sum()),
                rem_loaded_0=int((rl & (edits["last_unload_after"] == 0)).sum()), rem_loaded_now=int((rl & (edits["last_unload_after"] == now)).sum()),
                rem_failed=int(rf.sum()), expired=int((actions == JAN_EXPIRED).sum()), ties=int(info["n_ties"]), unresolved_beside_insert=beside)


def expiry_kinds(reg_before, reg_after, entries, self_pod, prm):
    """Failure records for self_pod by what became of them: (expired under the short rule only, expired under the full rule,
    stayed) — read off the records and the rows, not off the run's own reasoning."""
    prm = np.asarray(prm).reshape(-1)[0]
    now, full = int(prm["now"]), int(prm["load_failure_expiry_ms"])
    short = full // 2
    row_of = {int(m): r for r, m in enumerate(entries["model"]) if m >= 0}
    n_short = n_full = n_stay = 0
    for m, (b, a) in enumerate(zip(reg_before, reg_after)):
        ft = _get(b.failed, self_pod)
        if ft is None:
            continue
        r = row_of.get(m)
        if r is not None and not entries[r]["flags"] & JE_FAILED:
            continue
        if _get(a.failed, self_pod) is not None:
            n_stay += 1
        elif now - ft > full:
            n_full += 1
        elif now - ft > short:
            n_short += 1
    return n_short, n_full, n_stay
