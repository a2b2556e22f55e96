"""getStatus answered from a ModelRecord, restated in Python: the status class of invokeModel's "getStatus case"
(MM.java:3760-3768, with getStatus's own exits :3254-3259) and the copy list of makeStatusInfo (:3013-3058).

Two forms.  `status_sequential` is literal and sequential: a record keeps instanceIds and loadFailedInstanceIds as two ordered
dicts standing for the TreeMaps (tests/registry_ops_model.ModelRecord), requests are taken one at a time, the overlay is a
TreeMap.put / remove on copies of the maps, the list is sorted with Python's stable `sorted` under Long.compare(o.time, time), and
the Java line is cited at every step.  `status_closed` is the vectorised numpy form of the closed rule the device code uses
(include/mmplace.h, mmp_models_status): every stored entry and every overlay entry gets the key (request, ~time, list, position
in the list), and one lexicographic sort of the keys is the whole answer — ~time is -time - 1, so ascending ~time is descending
signed time without an overflow at Long.MIN_VALUE.  tests/test_model_status_model.py holds the two against each other.

The reference has no test that looks at copiesInfo or its order (nothing under its src/test mentions makeStatusInfo, CopyInfo or
getCopiesInfo), so there are no reference vectors: the restatement is read against the Java text.

One call uses ONE clock value (the library's convention) for currentTimeMillis() (:3020).  Not restated: the cache-hit loop
itself (:3640-3758 — a request says whether it was exhausted, MSTF_MISS), updateWithModelCopyInfo for LOADED / LOADING answers
(the host fills those in from the copy that answered, over the list returned with MST_ASK), and the messages (failInfos,
:3015, :3019, :3021, :3043-3045, :3049-3050: they are keyed by the same instance ids and stay with the caller; the
LOADING_FAILED rows in output order are their order, because :3044 sorts by the same times with the same stable sort over the
same TreeMap order).
"""
from __future__ import annotations

from collections import OrderedDict
from functools import cmp_to_key

import numpy as np

from modelmesh_amd._lib import (COPY_LOADING_FAILED, COPY_NOT_CHECKED, MST_ASK, MST_LOADING_FAILED, MST_NOT_FOUND, MST_NOT_LOADED,
                                MSTF_MISS, STATUS_COPY, STATUS_REQ, STATUS_ROW)
from tests.registry_ops_model import ModelRecord, tree_put

LONG_MIN, LONG_MAX = -2**63, 2**63 - 1


def req_row(model, fail_pod=-1, miss=False):
    return (model, fail_pod, MSTF_MISS if miss else 0, 0)


def reqs_array(rows):
    return np.array(rows, dtype=STATUS_REQ).reshape(-1)


def long_compare(a: int, b: int) -> int:                                   # Long.compare
    return -1 if a < b else (1 if a > b else 0)


def make_status_info(mr, fail_pod, now, id_order):
    """makeStatusInfo (:3013-3058) without the messages: (instTimes, failTimes after the overlay, copiesInfo as (pod, status,
    time) in the order of the reply)."""
    fail_times = OrderedDict(mr.load_failed_instance_ids) if mr is not None else OrderedDict()      # :3014 (always a copy here)
    inst_times = OrderedDict(mr.instance_ids) if mr is not None else OrderedDict()                  # :3016
    if fail_pod >= 0 and fail_pod not in fail_times:                       # :3017 mle != null && id != null && !containsKey
        tree_put(fail_times, fail_pod, now, id_order)                      # :3018, :3020 new TreeMap(failTimes).put(id, now)
        if fail_pod in inst_times:                                         # :3022
            del inst_times[fail_pod]                                       # :3023-3024
    copies = []
    for pod, t in inst_times.items():                                      # :3029-3035 in TreeMap order
        copies.append((pod, COPY_NOT_CHECKED, t))                          # :3034
    for pod, t in fail_times.items():                                      # :3037, :3046-3048 in TreeMap order
        copies.append((pod, COPY_LOADING_FAILED, t))                       # :3047
    # :3056 Collections.sort — a stable merge sort — under CopyInfo.compareTo = Long.compare(o.time, time)
    copies = sorted(copies, key=cmp_to_key(lambda me, o: long_compare(o[2], me[2])))
    return inst_times, fail_times, copies


def status_class(mr, fail_pod, miss, inst_times, fail_times):
    if mr is None:                                                         # :3256-3257 ModelNotFoundException -> SI_NOT_FOUND
        return MST_NOT_FOUND
    if inst_times and not miss:                                            # the cache-hit loop (:3640-3758) has copies to ask
        return MST_ASK
    if fail_pod >= 0 or fail_times:                                        # :3764 loadFailureSeen != null || mr.hasLoadFailure()
        return MST_LOADING_FAILED                                          # :3765
    return MST_NOT_LOADED                                                  # :3767


def status_sequential(registry, id_order, reqs, now):
    """(rows, copies) for a batch of STATUS_REQ rows over `registry` (ModelRecord per row); the registry is not changed."""
    rows = np.zeros(len(reqs), dtype=STATUS_ROW)
    out = []
    for i, q in enumerate(reqs):
        model, fail_pod, miss = int(q["model"]), int(q["fail_pod"]), bool(int(q["flags"]) & MSTF_MISS)
        mr = registry[model] if model >= 0 else None                       # mr == null
        inst_times, fail_times, copies = make_status_info(mr, fail_pod, now, id_order)
        rows[i] = (status_class(mr, fail_pod, miss, inst_times, fail_times), len(out), len(inst_times), len(fail_times))
        out.extend(copies)
    return rows, np.array(out, dtype=STATUS_COPY).reshape(-1)


def status_closed(models, ent_pod, ent_time, id_order, reqs, now):
    """The same answers on the array layout, without a loop over requests or entries."""
    n, P = len(reqs), len(id_order)
    model, fp = reqs["model"].astype(np.int64), reqs["fail_pod"].astype(np.int64)
    miss = (reqs["flags"] & MSTF_MISS) != 0
    has = model >= 0
    mi = np.where(has, model, 0)
    pick = (lambda f: np.where(has, models[f][mi], 0).astype(np.int64)) if len(models) else (lambda f: np.zeros(n, np.int64))
    off, nl0, nf0 = pick("ent_off"), pick("n_loaded"), pick("n_failed")
    cnt0 = nl0 + nf0
    seg = np.repeat(np.arange(n), cnt0)
    k = np.arange(int(cnt0.sum())) - np.repeat(np.cumsum(cnt0) - cnt0, cnt0)
    src = off[seg] + k
    pod, time = ent_pod[src].astype(np.int64), ent_time[src].astype(np.int64)
    failed = k >= nl0[seg]
    pos = np.where(failed, k - nl0[seg], k)                                # position in its own list
    hit = (fp[seg] >= 0) & (pod == fp[seg])
    overlay = (fp >= 0) & (np.bincount(seg[hit & failed], minlength=n) == 0)            # :3017
    drop = hit & ~failed & overlay[seg]                                                  # :3022-3024
    resolved = (pod >= 0) & (pod < P)
    order = np.asarray(id_order, np.int64)
    greater = failed & resolved & overlay[seg] & (order[np.where(resolved, pod, 0)] > order[np.where(fp >= 0, fp, 0)][seg])
    ins = nf0.copy()                                                       # TreeMap.put of a new key: in front of the first greater
    np.minimum.at(ins, seg[greater], pos[greater])
    ov = np.flatnonzero(overlay)
    keep = ~drop
    # all entries: the stored ones that stay, then the overlay's own (tie 0: in front of the stored entry at the same position)
    a_seg = np.concatenate([seg[keep], ov])
    a_pod = np.concatenate([pod[keep], fp[ov]])
    a_time = np.concatenate([time[keep], np.full(len(ov), now, np.int64)])
    a_list = np.concatenate([failed[keep].astype(np.int64), np.ones(len(ov), np.int64)])
    a_pos = np.concatenate([pos[keep], ins[ov]])
    a_tie = np.concatenate([np.ones(int(keep.sum()), np.int64), np.zeros(len(ov), np.int64)])
    o = np.lexsort((a_tie, a_pos, a_list, ~a_time, a_seg))                 # the last key is the primary one
    copies = np.zeros(len(o), dtype=STATUS_COPY)
    copies["pod"], copies["status"], copies["time"] = a_pod[o], np.where(a_list[o] == 1, COPY_LOADING_FAILED, COPY_NOT_CHECKED), a_time[o]
    nl = nl0 - np.bincount(seg[drop], minlength=n)
    nf = nf0 + overlay
    rows = np.zeros(n, dtype=STATUS_ROW)
    rows["cls"] = np.where(~has, MST_NOT_FOUND, np.where((nl > 0) & ~miss, MST_ASK, np.where((fp >= 0) | (nf > 0), MST_LOADING_FAILED, MST_NOT_LOADED)))
    rows["n_not_checked"], rows["n_failed"] = nl, nf
    rows["copy_off"] = np.cumsum(nl + nf) - (nl + nf)
    return rows, copies


def assert_same_status(got, want, what=""):
    (rows, copies), (wrows, wcopies) = got, want
    assert rows.dtype == wrows.dtype and len(rows) == len(wrows), (what, len(rows), len(wrows))
    bad = np.flatnonzero(rows != wrows)
    assert len(bad) == 0, (what, "row", int(bad[0]), rows[bad[0]], wrows[bad[0]])
    assert copies.dtype == wcopies.dtype and len(copies) == len(wcopies), (what, len(copies), len(wcopies))
    bad = np.flatnonzero(copies != wcopies)
    assert len(bad) == 0, (what, "copy", int(bad[0]), copies[max(0, bad[0] - 2):bad[0] + 3], wcopies[max(0, bad[0] - 2):bad[0] + 3])


def copies_of(rows, copies, i):
    r = rows[i]
    return [tuple(int(x) for x in c) for c in copies[int(r["copy_off"]):int(r["copy_off"]) + int(r["n_not_checked"]) + int(r["n_failed"])]]


# ---- batches by construction -----------------------------------------------------------------------------------------------

SHAPES = ("empty", "only_loaded", "only_failed", "both")
CASES = (("empty_record", "only_loaded", "only_failed", "both_kinds", "no_record", "no_record_with_fail_pod", "overlay_on_loaded",
          "overlay_on_failed_already_loaded_stays", "overlay_first", "overlay_middle", "overlay_last", "overlay_beside_unresolved",
          "tie_at_now_in_front_of_overlay", "tie_at_now_behind_overlay", "loaded_and_failed_equal_time", "equal_times_in_one_list",
          "time_zero", "time_minus_one", "time_long_min", "time_long_max")
         + tuple(f"miss_{s}" for s in SHAPES) + tuple(f"no_miss_{s}" for s in SHAPES))


def classify(registry, id_order, q, now):
    """The named cases one request takes (from the record and the sequential form's own intermediate state)."""
    model, fail_pod, miss = int(q["model"]), int(q["fail_pod"]), bool(int(q["flags"]) & MSTF_MISS)
    if model < 0:
        return {"no_record_with_fail_pod" if fail_pod >= 0 else "no_record"}
    mr, P, out = registry[model], len(id_order), set()
    L, F = mr.instance_ids, mr.load_failed_instance_ids
    shape = SHAPES[(1 if L else 0) + (2 if F else 0)]
    out.add({"empty": "empty_record", "only_loaded": "only_loaded", "only_failed": "only_failed", "both": "both_kinds"}[shape])
    out.add(("miss_" if miss else "no_miss_") + shape)
    if fail_pod >= 0 and fail_pod in F and fail_pod in L:
        out.add("overlay_on_failed_already_loaded_stays")
    if fail_pod >= 0 and fail_pod not in F:
        if fail_pod in L:
            out.add("overlay_on_loaded")
        _, fail_times, _ = make_status_info(mr, fail_pod, now, id_order)
        at, keys = list(fail_times).index(fail_pod), list(F)
        if F:
            out.add("overlay_first" if at == 0 else "overlay_last" if at == len(F) else "overlay_middle")
        if any(not 0 <= p < P for p in keys):
            out.add("overlay_beside_unresolved")
        if any(F[p] == now for p in keys[:at]):
            out.add("tie_at_now_in_front_of_overlay")
        if any(F[p] == now for p in keys[at:]):
            out.add("tie_at_now_behind_overlay")
    if set(L.values()) & set(F.values()):
        out.add("loaded_and_failed_equal_time")
    if len(set(L.values())) < len(L) or len(set(F.values())) < len(F):
        out.add("equal_times_in_one_list")
    for t, name in ((0, "time_zero"), (-1, "time_minus_one"), (LONG_MIN, "time_long_min"), (LONG_MAX, "time_long_max")):
        if t in L.values() or t in F.values():
            out.add(name)
    return out


N_PLANTED = 9


def seed_shapes(registry, id_order, now):
    """Rewrites the first N_PLANTED records so that every named case has a record to happen on (needs 8 instances); returns the
    requests that take them, as rows for reqs_array."""
    by = [int(p) for p in np.argsort(id_order, kind="stable")]  # instances in id order
    P, T = len(id_order), now - 1_000
    assert len(by) >= 8 and len(registry) > N_PLANTED

    def rec(i, loaded, failed):
        registry[i] = ModelRecord(registry[i].type, loaded, failed, registry[i].last_used)

    rec(0, [], [])
    rec(1, [(by[1], now - 5), (by[3], now - 9)], [])
    rec(2, [], [(by[2], now - 3), (by[5], now - 7)])
    rec(3, [(by[0], now - 10), (by[4], now - 20)], [(by[2], now - 15), (-1, now - 1), (by[5], now - 15), (P + 2, now - 30)])
    rec(4, [(by[2], now - 4)], [(by[2], now - 8)])
    rec(5, [], [(by[2], now), (by[6], now)])
    rec(6, [(by[1], T)], [(by[3], T)])
    rec(7, [(by[0], T), (by[1], T), (by[2], T)], [(by[5], T - 1), (by[6], T - 1)])
    rec(8, [(by[0], 0), (by[1], -1), (by[2], LONG_MIN), (by[3], LONG_MAX)], [(by[4], LONG_MIN), (by[5], LONG_MAX), (by[6], 0), (by[7], -1)])
    rows = [req_row(i, -1, miss) for i in range(N_PLANTED) for miss in (False, True)]
    rows += [req_row(-1), req_row(-1, by[3]), req_row(-1, by[3], True)]
    rows += [req_row(3, by[1]), req_row(3, by[3], True), req_row(3, by[7]), req_row(3, by[4]), req_row(3, by[4], True)]  # first, middle, last; onto a loaded one
    rows += [req_row(4, by[2]), req_row(4, by[2], True), req_row(5, by[4]), req_row(5, by[0]), req_row(5, by[7], True)]
    rows += [req_row(0, by[0]), req_row(1, by[3]), req_row(1, by[0], True), req_row(2, by[5]), req_row(6, by[1]), req_row(7, by[6]), req_row(8, by[3])]
    return rows


def draw_reqs(registry, id_order, now, rng, n, planted):
    """n requests: the planted ones first (as many as fit), then models, overlays and the MISS flag at random, models repeating."""
    rows = list(planted[:n])
    M, P = len(registry), len(id_order)
    while len(rows) < n:
        model = int(rng.integers(-1, M)) if rng.random() < 0.9 else int(rng.integers(0, min(M, N_PLANTED)))
        fail_pod = int(rng.integers(0, P)) if rng.random() < 0.4 else -1
        if fail_pod >= 0 and model >= 0 and rng.random() < 0.5:  # an instance the record names, where it names one
            mr = registry[model]
            named = [p for p in list(mr.instance_ids) + list(mr.load_failed_instance_ids) if 0 <= p < P]
            if named:
                fail_pod = int(named[int(rng.integers(0, len(named)))])
        rows.append(req_row(model, fail_pod, bool(rng.random() < 0.5)))
    return reqs_array(rows)


def cases_seen(registry, id_order, reqs, now):
    seen = set()
    for q in reqs:
        seen |= classify(registry, id_order, q, now)
    return seen
