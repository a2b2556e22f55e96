"""The edits an instance makes to ModelRecords itself, restated in Python: a load completes (loadLocal, MM.java:5204-5207), a
load fails (the CacheEntry failure path, :2484-2495), a copy is evicted or dropped (deregisterModel, :2948-2958) and a scale-down
removes the local copy (removeLocalModelCopyAsync, :6347-6365), with ModelRecord.addLoadFailure / removeLoadFailure /
updateLastUsed / updateLastUnloadTime (ModelRecord.java:156-179, :239-262).

Two forms.  `Registry.run` is literal and sequential: a record keeps instanceIds and loadFailedInstanceIds as two ordered dicts
standing for the TreeMaps, plus lastUsed and lastUnloadTime; ops are taken one at a time and the Java line is cited at every
step.  `closed_rule` is the per-op form on the array layout that the device code mirrors (include/mmplace.h, mmp_registry_ops):
a call names a record at most once, so an op is decided from its own row and entries alone, and the edited records are rebuilt
from the edit and the op.  tests/test_registry_ops_model.py holds the two against each other.

The reference has no test that names this code (nothing under its src/test mentions deregisterModel, removeLocalModelCopyAsync
or addLoadFailure), so there are no reference vectors: the restatement is read against the Java text.

One call uses ONE clock value (the library's convention) for every currentTimeMillis().  Not restated: the conditional-set
retries (:2496-2502, :2958-2960, :5208-5214, :6367; a record is what the registry holds), loadFailureInfos
(ModelRecord.java:158-165, :170, :175), isLoadedElsewhere (:6357: the host sends the op after it) and the CacheEntry state
machine around these sites.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

from modelmesh_amd._lib import (MODEL_ROW, REGISTRY_OP, REGISTRY_OP_EDIT, ROP_DEREGISTER, ROP_EDIT_PUT_FAILED, ROP_EDIT_PUT_LOADED,
                                ROP_EDIT_REM_FAILED, ROP_EDIT_REM_LOADED, ROP_EDIT_REPLACED, ROP_EDIT_TOUCHED, ROP_EDIT_UNLOAD_SET,
                                ROP_EDITED, ROP_LOAD_FAILED, ROP_REGISTER, ROP_SCALE_DOWN, ROP_UNCHANGED, ROPF_MATCH_TIME,
                                ROPF_SHUTTING_DOWN)
from tests.registry_prune_model import LONG_MAX, Record

KINDS = (ROP_REGISTER, ROP_LOAD_FAILED, ROP_DEREGISTER, ROP_SCALE_DOWN)


class InvalidOps(ValueError):
    """What the library answers with MMP_EINVAL."""


class ModelRecord:
    """One ModelRecord: the two TreeMaps as ordered dicts (instance -> time, in id order), lastUsed, lastUnloadTime."""

    def __init__(self, type, loaded, failed, last_used, last_unload=0):
        self.type = type
        self.instance_ids = OrderedDict(loaded)
        self.load_failed_instance_ids = OrderedDict(failed)
        self.last_used = last_used
        self.last_unload_time = last_unload

    def update_last_used(self, last_used, now):                       # ModelRecord.java:239-246
        if last_used == 0:                                            # :240
            last_used = now                                           # :241
        if last_used > self.last_used:                                # :243
            self.last_used = last_used
            return True
        return False

    def update_last_unload_time(self, now):                           # ModelRecord.java:260-262
        self.last_unload_time = 0 if len(self.instance_ids) <= 2 else now

    def __eq__(self, other):
        return (self.type, list(self.instance_ids.items()), list(self.load_failed_instance_ids.items()), self.last_used,
                self.last_unload_time) == (other.type, list(other.instance_ids.items()), list(other.load_failed_instance_ids.items()),
                                           other.last_used, other.last_unload_time)


def tree_put(d: OrderedDict, pod, time, id_order):
    """TreeMap.put: (position, replaced).  The value is replaced where the key stands; a new key goes in front of the first
    RESOLVED entry whose id is greater, at the end if there is none.  Entries whose instance is not in the instance table
    (index < 0 or beyond it) keep their place and are never compared."""
    keys = list(d)
    if pod in d:
        d[pod] = time
        return keys.index(pod), True
    at = len(keys)
    for k, p in enumerate(keys):
        if 0 <= p < len(id_order) and id_order[p] > id_order[pod]:
            at = k
            break
    items = list(d.items())
    items.insert(at, (pod, time))
    d.clear()
    d.update(items)
    return at, False


def tree_remove(d: OrderedDict, pod, time=None):
    """Map.remove(key) != null, or with a time Map.remove(key, value): the key is present AND its value equal."""
    if pod not in d or (time is not None and d[pod] != time):
        return False
    del d[pod]
    return True


def registry_from_arrays(models, ent_pod, ent_time):
    out = []
    for m in models:
        o, nl, nf = int(m["ent_off"]), int(m["n_loaded"]), int(m["n_failed"])
        ents = [(int(ent_pod[o + k]), int(ent_time[o + k])) for k in range(nl + nf)]
        out.append(ModelRecord(int(m["type"]), ents[:nl], ents[nl:], int(m["last_used"])))
    return out


def registry_to_arrays(registry):
    """Compact arrays (rows in order, a row's entries in order, no gaps)."""
    models = np.zeros(len(registry), dtype=MODEL_ROW)
    pods, times = [], []
    for i, r in enumerate(registry):
        models[i] = (r.type, len(pods), len(r.instance_ids), len(r.load_failed_instance_ids), r.last_used)
        for p, t in list(r.instance_ids.items()) + list(r.load_failed_instance_ids.items()):
            pods.append(p)
            times.append(t)
    return models, np.array(pods, np.int32).reshape(-1), np.array(times, np.int64).reshape(-1)


def to_prune_records(registry):
    """The same registry as tests/registry_prune_model.Record rows (what the prune, janitor and census restatements take)."""
    return [Record(r.type, list(r.instance_ids.items()), list(r.load_failed_instance_ids.items()), r.last_used) for r in registry]


def op_row(model, pod, op, flags=0, last_used=0, load_time=0, load_complete_time=0):
    return (model, pod, op, flags, last_used, load_time, load_complete_time)


def ops_array(rows):
    return np.array(rows, dtype=REGISTRY_OP).reshape(-1)


def check_ops(ops, n_models, n_pods, now):
    """The library's validation: anything here is MMP_EINVAL with nothing written or changed."""
    if now <= 0:
        raise InvalidOps("now")
    seen = set()
    for o in ops:
        if not 0 <= o["model"] < n_models:
            raise InvalidOps("model")
        if not 0 <= o["pod"] < n_pods:
            raise InvalidOps("pod")
        if int(o["op"]) not in KINDS:
            raise InvalidOps("op")
        if int(o["flags"]) & ~(ROPF_SHUTTING_DOWN | ROPF_MATCH_TIME):
            raise InvalidOps("flags")
        if int(o["model"]) in seen:
            raise InvalidOps("two ops name one model")
        seen.add(int(o["model"]))


def _info(ops, status, edits):
    info = dict(n_edits=len(edits), n_unchanged=len(ops) - len(edits), truncated=0, n_edited_op=[0] * 4, n_unchanged_op=[0] * 4,
                n_entries_added=0, n_entries_removed=0)
    for o, st in zip(ops, status):
        info["n_edited_op" if st == ROP_EDITED else "n_unchanged_op"][int(o["op"])] += 1
    for e in edits:
        f = int(e[4])
        info["n_entries_added"] += bool(f & (ROP_EDIT_PUT_LOADED | ROP_EDIT_PUT_FAILED)) and not f & ROP_EDIT_REPLACED
        info["n_entries_removed"] += bool(f & ROP_EDIT_REM_LOADED) + bool(f & ROP_EDIT_REM_FAILED)
    return info


class Registry:
    """The registry as the instances see it: a list of ModelRecord by model index, and the instance table's id order."""

    def __init__(self, records, id_order):
        self.records = records
        self.id_order = id_order

    def run(self, ops, now, dry=False):
        """The ops one at a time, in order.  Edits the records in place unless dry; returns (status uint8[], edits
        REGISTRY_OP_EDIT[] in op order, info dict)."""
        ops = np.ascontiguousarray(ops, dtype=REGISTRY_OP)
        check_ops(ops, len(self.records), len(self.id_order), now)
        status, edits = np.zeros(len(ops), np.uint8), []
        for i, o in enumerate(ops):
            model, pod, flags = int(o["model"]), int(o["pod"]), int(o["flags"])
            last_used, load_time, load_complete = int(o["last_used"]), int(o["load_time"]), int(o["load_complete_time"])
            live = self.records[model]
            mr = ModelRecord(live.type, live.instance_ids, live.load_failed_instance_ids, live.last_used, live.last_unload_time)
            ef, pos, edited = 0, -1, False
            if o["op"] == ROP_REGISTER:
                pos, replaced = tree_put(mr.instance_ids, pod, load_time, self.id_order)        # :5204
                ef |= ROP_EDIT_PUT_LOADED | (ROP_EDIT_REPLACED if replaced else 0)
                if tree_remove(mr.load_failed_instance_ids, pod):                               # :5206
                    ef |= ROP_EDIT_REM_FAILED
                if mr.update_last_used(now if last_used == 0 else last_used, now):              # :5207
                    ef |= ROP_EDIT_TOUCHED
                edited = True                                                                   # :5208 always submitted
            elif o["op"] == ROP_LOAD_FAILED:
                if last_used <= 0:                                                              # :2484
                    last_used = mr.last_used                                                    # :2485
                was_there = tree_remove(mr.instance_ids, pod, load_time)                        # :2487
                if was_there:                                                                   # :2488
                    ef |= ROP_EDIT_REM_LOADED
                    if not flags & ROPF_SHUTTING_DOWN:                                          # :2492
                        pos, replaced = tree_put(mr.load_failed_instance_ids, pod, load_complete, self.id_order)  # ModelRecord.java:157
                        ef |= ROP_EDIT_PUT_FAILED | (ROP_EDIT_REPLACED if replaced else 0)
                        assert not tree_remove(mr.instance_ids, pod)                            # ModelRecord.java:166 finds nothing
                    if mr.update_last_used(last_used, now):                                     # :2495
                        ef |= ROP_EDIT_TOUCHED
                    edited = True                                                               # :2496
            elif o["op"] == ROP_DEREGISTER:
                match = bool(flags & ROPF_MATCH_TIME)                                           # loadTime != null
                was_there = tree_remove(mr.instance_ids, pod, load_time if match else None)     # :2951-2952
                failed_was_there = tree_remove(mr.load_failed_instance_ids, pod, load_complete if match else None)  # :2953-2954
                if was_there or failed_was_there:                                               # :2955
                    ef |= (ROP_EDIT_REM_LOADED if was_there else 0) | (ROP_EDIT_REM_FAILED if failed_was_there else 0)
                    if mr.update_last_used(last_used, now):                                     # :2956
                        ef |= ROP_EDIT_TOUCHED
                    if was_there:                                                               # :2957
                        mr.update_last_unload_time(now)
                        ef |= ROP_EDIT_UNLOAD_SET
                    edited = True                                                               # :2958
            else:  # ROP_SCALE_DOWN
                reg_load_time = mr.instance_ids.get(pod)                                        # :6347
                if reg_load_time is not None and reg_load_time == load_time:                    # :6348
                    assert tree_remove(mr.instance_ids, pod)                                    # :6363
                    mr.update_last_unload_time(now)                                             # :6364
                    ef |= ROP_EDIT_REM_LOADED | ROP_EDIT_UNLOAD_SET
                    if mr.update_last_used(last_used, now):                                     # :6365
                        ef |= ROP_EDIT_TOUCHED
                    edited = True                                                               # :6367
            if not edited:
                continue
            status[i] = ROP_EDITED
            edits.append((model, i, len(mr.instance_ids), len(mr.load_failed_instance_ids), ef, pos, mr.last_used,
                          mr.last_unload_time if ef & ROP_EDIT_UNLOAD_SET else 0))
            if not dry:
                self.records[model] = mr                                                        # conditionalSetAndGet took it
        return status, np.array(edits, dtype=REGISTRY_OP_EDIT).reshape(-1), _info(ops, status, edits)


def _find(models_row, ent_pod, ent_time, pod):
    """(position in instanceIds, its time, position in loadFailedInstanceIds, its time); -1: absent."""
    o, nl, nf = int(models_row["ent_off"]), int(models_row["n_loaded"]), int(models_row["n_failed"])
    li = fi = -1
    lt = ft = 0
    for k in range(nl + nf):
        if int(ent_pod[o + k]) != pod:
            continue
        if k < nl:
            li, lt = k, int(ent_time[o + k])
        else:
            fi, ft = k - nl, int(ent_time[o + k])
    return li, lt, fi, ft


def insert_pos(ent_pod, off, cnt, pod, id_order):
    """Where a new key goes in the list arena[off, off + cnt): in front of the first resolved entry with a greater id."""
    for k in range(cnt):
        p = int(ent_pod[off + k])
        if 0 <= p < len(id_order) and id_order[p] > id_order[pod]:
            return k
    return cnt


def closed_rule(models, ent_pod, ent_time, ops, now, id_order):
    """Every op decided from its own row and entries, as the device does it: (status, edits, info).  Reads the arrays only."""
    ops = np.ascontiguousarray(ops, dtype=REGISTRY_OP)
    check_ops(ops, len(models), len(id_order), now)
    status, edits = np.zeros(len(ops), np.uint8), []
    for i, o in enumerate(ops):
        m = models[o["model"]]
        pod, flags, op_lu = int(o["pod"]), int(o["flags"]), int(o["last_used"])
        off, nl, nf, lu = int(m["ent_off"]), int(m["n_loaded"]), int(m["n_failed"]), int(m["last_used"])
        li, lt, fi, ft = _find(m, ent_pod, ent_time, pod)
        ef, pos, edited, unload, touch = 0, -1, False, False, None
        if o["op"] == ROP_REGISTER:
            edited, touch = True, op_lu
            ef |= ROP_EDIT_PUT_LOADED
            if li >= 0:
                ef, pos = ef | ROP_EDIT_REPLACED, li
            else:
                pos, nl = insert_pos(ent_pod, off, nl, pod, id_order), nl + 1
            if fi >= 0:
                ef, nf = ef | ROP_EDIT_REM_FAILED, nf - 1
        elif o["op"] == ROP_LOAD_FAILED:
            if li >= 0 and lt == int(o["load_time"]):
                edited, touch = True, (op_lu if op_lu > 0 else lu)
                ef, nl = ef | ROP_EDIT_REM_LOADED, nl - 1
                if not flags & ROPF_SHUTTING_DOWN:
                    ef |= ROP_EDIT_PUT_FAILED
                    if fi >= 0:
                        ef, pos = ef | ROP_EDIT_REPLACED, fi
                    else:
                        pos, nf = insert_pos(ent_pod, off + int(m["n_loaded"]), nf, pod, id_order), nf + 1
        elif o["op"] == ROP_DEREGISTER:
            match = bool(flags & ROPF_MATCH_TIME)
            was = li >= 0 and (not match or lt == int(o["load_time"]))
            fwas = fi >= 0 and (not match or ft == int(o["load_complete_time"]))
            if was or fwas:
                edited, touch, unload = True, op_lu, was
                ef |= (ROP_EDIT_REM_LOADED if was else 0) | (ROP_EDIT_REM_FAILED if fwas else 0)
                nl, nf = nl - was, nf - fwas
        else:
            if li >= 0 and lt == int(o["load_time"]):
                edited, touch, unload = True, op_lu, True
                ef, nl = ef | ROP_EDIT_REM_LOADED, nl - 1
        if not edited:
            continue
        t = now if touch == 0 else touch
        if t > lu:
            lu, ef = t, ef | ROP_EDIT_TOUCHED
        if unload:
            ef |= ROP_EDIT_UNLOAD_SET
        status[i] = ROP_EDITED
        edits.append((int(o["model"]), i, nl, nf, ef, pos, lu, now if unload and nl > 2 else 0))
    return status, np.array(edits, dtype=REGISTRY_OP_EDIT).reshape(-1), _info(ops, status, edits)


def apply_edits(models, ent_pod, ent_time, ops, edits):
    """What an apply leaves: the edited records rebuilt from (row, op, edit) alone and appended; returns new compact-able
    (models, ent_pod, ent_time) with the other rows untouched."""
    models, pods, times = models.copy(), list(ent_pod), list(ent_time)
    for e in edits:
        o, m = ops[e["op_index"]], models[e["model"]]
        f, pod = int(e["flags"]), int(o["pod"])
        start = len(pods)

        def one_list(off, cnt, rem, ins, t_ins):
            fresh = ins and not f & ROP_EDIT_REPLACED
            for k in range(cnt):
                p, t = int(ent_pod[off + k]), int(ent_time[off + k])
                if p == pod:
                    if ins:
                        pods.append(p), times.append(t_ins)
                    elif not rem:
                        pods.append(p), times.append(t)
                    continue
                if fresh and k == e["inserted_pos"]:
                    pods.append(pod), times.append(t_ins)
                pods.append(p), times.append(t)
            if fresh and e["inserted_pos"] == cnt:
                pods.append(pod), times.append(t_ins)

        one_list(int(m["ent_off"]), int(m["n_loaded"]), f & ROP_EDIT_REM_LOADED, f & ROP_EDIT_PUT_LOADED, int(o["load_time"]))
        one_list(int(m["ent_off"]) + int(m["n_loaded"]), int(m["n_failed"]), f & ROP_EDIT_REM_FAILED, f & ROP_EDIT_PUT_FAILED,
                 int(o["load_complete_time"]))
        assert len(pods) - start == e["n_loaded_after"] + e["n_failed_after"]
        models[e["model"]] = (m["type"], start, e["n_loaded_after"], e["n_failed_after"], e["last_used_after"])
    return models, np.array(pods, np.int32).reshape(-1), np.array(times, np.int64).reshape(-1)


# ---- batches drawn from the records, so that every exit of the four sites occurs ----------------------------------------

EXITS = ("register_new", "register_replace_same", "register_replace_other", "register_clears_failure", "register_beside_unresolved",
         "register_last_used_now", "register_not_lowered", "register_at_max",
         "failed_mismatch", "failed_absent", "failed_shutting_down", "failed_put_new", "failed_put_over", "failed_lu_from_record",
         "failed_lu_zero_is_now",
         "dereg_match_loaded_only", "dereg_match_failed_only", "dereg_match_both", "dereg_match_neither", "dereg_loaded", "dereg_failed",
         "dereg_both", "dereg_none", "dereg_unload_zero", "dereg_unload_now", "dereg_failed_only_no_unload",
         "scale_absent", "scale_mismatch", "scale_match", "scale_keeps_failure")


def classify(record: ModelRecord, o, st, e):
    """The exits (names of EXITS) that op `o` took on `record` (as it stood before the op); e = its edit row or None."""
    pod, flags, lu = int(o["pod"]), int(o["flags"]), int(o["last_used"])
    l, f = record.instance_ids, record.load_failed_instance_ids
    out = []
    if o["op"] == ROP_REGISTER:
        if pod not in l:
            out.append("register_new")
            if any(p < 0 for p in l):
                out.append("register_beside_unresolved")
        else:
            out.append("register_replace_same" if l[pod] == o["load_time"] else "register_replace_other")
        if pod in f:
            out.append("register_clears_failure")
        if lu == 0 and e["flags"] & ROP_EDIT_TOUCHED:
            out.append("register_last_used_now")
        if lu != 0 and lu < record.last_used < LONG_MAX:
            out.append("register_not_lowered")
        if record.last_used == LONG_MAX:
            out.append("register_at_max")
    elif o["op"] == ROP_LOAD_FAILED:
        if pod not in l:
            out.append("failed_absent")
        elif l[pod] != o["load_time"]:
            out.append("failed_mismatch")
        else:
            if flags & ROPF_SHUTTING_DOWN:
                out.append("failed_shutting_down")
            else:
                out.append("failed_put_over" if pod in f else "failed_put_new")
            if lu <= 0:
                out.append("failed_lu_zero_is_now" if record.last_used == 0 else "failed_lu_from_record")
    elif o["op"] == ROP_DEREGISTER:
        if flags & ROPF_MATCH_TIME:
            was, fwas = l.get(pod) == o["load_time"] and pod in l, f.get(pod) == o["load_complete_time"] and pod in f
            out.append("dereg_match_" + ("both" if was and fwas else "loaded_only" if was else "failed_only" if fwas else "neither"))
        else:
            was, fwas = pod in l, pod in f
            out.append("dereg_" + ("both" if was and fwas else "loaded" if was else "failed" if fwas else "none"))
        if was:
            out.append("dereg_unload_now" if len(l) - 1 > 2 else "dereg_unload_zero")
        elif fwas:
            out.append("dereg_failed_only_no_unload")
    else:
        if pod not in l:
            out.append("scale_absent")
        elif l[pod] != o["load_time"]:
            out.append("scale_mismatch")
        else:
            out.append("scale_match")
            if pod in f:
                out.append("scale_keeps_failure")
    assert (st == ROP_EDITED) == (e is not None)
    return out


def seed_shapes(registry, id_order, now, rng):
    """Rewrites a handful of records (in place) so that a batch drawn by draw_ops can take every exit whatever the fleet's
    generator produced: a record at Long.MAX_VALUE, one with lastUsed 0, ones that hold an instance in BOTH lists, ones with
    exactly 3 and 4 copies, and one with an unresolved entry.  Returns nothing; draw_ops looks the shapes up again."""
    n, P = len(registry), len(id_order)
    order = sorted(range(P), key=lambda p: id_order[p])
    pick = iter(rng.permutation(n)[: min(n, 13)].tolist())

    def rec(loaded, failed, last_used):
        r = registry[next(pick)]
        r.instance_ids = OrderedDict((p, now - 5000 - 7 * k) for k, p in enumerate(loaded))
        r.load_failed_instance_ids = OrderedDict((p, now - 900 - k) for k, p in enumerate(failed))
        r.last_used = last_used
        return r

    a, b, c, d, e = order[0], order[1], order[2], order[3], order[4]
    rec([a, b], [], LONG_MAX)                     # register_at_max
    rec([a], [], 0)                               # failed_lu_zero_is_now
    rec([a, c], [a], now - 10)                    # in both lists: dereg_both / dereg_match_both / scale_keeps_failure / failed_put_over
    rec([b, d], [b], now - 10)
    rec([a, e], [a], now - 10)
    rec([b, c], [b], now - 10)
    rec([c, d], [c], now - 10)
    rec([d, e], [d], now - 10)
    rec([a, b, c], [], now - 10)                  # dereg leaves 2: unload 0
    rec([a, b, c, d], [], now - 10)               # dereg leaves 3: unload now
    r = rec([b, d], [c], now - 10)                # an unresolved entry between resolved ones
    r.instance_ids = OrderedDict([(b, now - 1), (-1, now - 2), (d, now - 3)])
    rec([], [a], now - 10)                        # register_clears_failure on a record without copies
    rec([], [], now - 10)                         # an empty record


def draw_ops(registry, id_order, now, rng, n):
    """n ops on n distinct models, drawn BY CONSTRUCTION from the records so that every name of EXITS occurs when the registry
    offers the shapes (seed_shapes makes sure).  Each recipe looks for a record that fits and writes the op that takes the exit;
    the rest of the batch is drawn at random over kinds, instances and time matches."""
    P = len(id_order)
    used, rows = set(), []
    idx = rng.permutation(len(registry)).tolist()

    def find(pred):
        for i in idx:
            if i not in used and pred(registry[i]):
                used.add(i)
                return i, registry[i]
        return None, None

    def absent(r, also=()):
        for p in rng.permutation(P).tolist():
            if p not in r.instance_ids and p not in r.load_failed_instance_ids and p not in also:
                return p
        return None

    def both(r):
        return [p for p in r.instance_ids if p in r.load_failed_instance_ids]

    def add(i, pod, op, **kw):
        rows.append(op_row(i, pod, op, **kw))

    nl = lambda r: len(r.instance_ids)  # noqa: E731
    first = lambda d: next(iter(d))  # noqa: E731
    mid = lambda r: r.last_used if 0 < r.last_used < LONG_MAX else now - 10  # noqa: E731
    recipes = [
        # REGISTER
        (lambda r: nl(r) >= 1 and nl(r) < P - 1 and all(p >= 0 for p in r.instance_ids) and 0 < r.last_used < now,
         lambda i, r: add(i, absent(r), ROP_REGISTER, last_used=0, load_time=now - 3)),
        (lambda r: any(p < 0 for p in r.instance_ids) and nl(r) < P - 1,
         lambda i, r: add(i, absent(r), ROP_REGISTER, last_used=now, load_time=now - 3)),
        (lambda r: nl(r) >= 2, lambda i, r: add(i, list(r.instance_ids)[1], ROP_REGISTER, last_used=now, load_time=list(r.instance_ids.values())[1])),
        (lambda r: nl(r) >= 1, lambda i, r: add(i, first(r.instance_ids), ROP_REGISTER, last_used=now, load_time=now + 17)),
        (lambda r: len(r.load_failed_instance_ids) >= 1, lambda i, r: add(i, first(r.load_failed_instance_ids), ROP_REGISTER, last_used=now, load_time=now)),
        (lambda r: 1 < r.last_used < LONG_MAX, lambda i, r: add(i, 0, ROP_REGISTER, last_used=r.last_used - 1, load_time=now)),
        (lambda r: r.last_used == LONG_MAX, lambda i, r: add(i, 0, ROP_REGISTER, last_used=now, load_time=now)),
        # LOAD_FAILED
        (lambda r: nl(r) >= 1, lambda i, r: add(i, first(r.instance_ids), ROP_LOAD_FAILED, last_used=now, load_time=r.instance_ids[first(r.instance_ids)] + 1,
                                                load_complete_time=now)),
        (lambda r: absent(r) is not None, lambda i, r: add(i, absent(r), ROP_LOAD_FAILED, last_used=now, load_time=now, load_complete_time=now)),
        (lambda r: nl(r) >= 1, lambda i, r: add(i, first(r.instance_ids), ROP_LOAD_FAILED, flags=ROPF_SHUTTING_DOWN, last_used=now,
                                                load_time=r.instance_ids[first(r.instance_ids)], load_complete_time=now)),
        (lambda r: nl(r) >= 1 and not both(r) and r.last_used > 0,
         lambda i, r: add(i, list(r.instance_ids)[-1], ROP_LOAD_FAILED, last_used=-1, load_time=list(r.instance_ids.values())[-1], load_complete_time=now - 1)),
        (lambda r: both(r), lambda i, r: add(i, both(r)[0], ROP_LOAD_FAILED, last_used=now + 5, load_time=r.instance_ids[both(r)[0]], load_complete_time=now - 2)),
        (lambda r: nl(r) >= 1 and r.last_used == 0,
         lambda i, r: add(i, first(r.instance_ids), ROP_LOAD_FAILED, last_used=0, load_time=r.instance_ids[first(r.instance_ids)], load_complete_time=now)),
        # DEREGISTER with MATCH_TIME
        (lambda r: both(r), lambda i, r: add(i, both(r)[0], ROP_DEREGISTER, flags=ROPF_MATCH_TIME, last_used=0, load_time=r.instance_ids[both(r)[0]],
                                             load_complete_time=r.load_failed_instance_ids[both(r)[0]] + 1)),
        (lambda r: both(r), lambda i, r: add(i, both(r)[0], ROP_DEREGISTER, flags=ROPF_MATCH_TIME, last_used=mid(r), load_time=r.instance_ids[both(r)[0]] - 1,
                                             load_complete_time=r.load_failed_instance_ids[both(r)[0]])),
        (lambda r: both(r), lambda i, r: add(i, both(r)[0], ROP_DEREGISTER, flags=ROPF_MATCH_TIME, last_used=0, load_time=r.instance_ids[both(r)[0]],
                                             load_complete_time=r.load_failed_instance_ids[both(r)[0]])),
        (lambda r: nl(r) >= 1, lambda i, r: add(i, first(r.instance_ids), ROP_DEREGISTER, flags=ROPF_MATCH_TIME, last_used=0,
                                                load_time=r.instance_ids[first(r.instance_ids)] + 1, load_complete_time=1)),
        # DEREGISTER without it
        (lambda r: nl(r) == 3 and not both(r), lambda i, r: add(i, list(r.instance_ids)[1], ROP_DEREGISTER, last_used=0, load_time=-5)),
        (lambda r: nl(r) == 4 and not both(r), lambda i, r: add(i, list(r.instance_ids)[-1], ROP_DEREGISTER, last_used=mid(r))),
        (lambda r: any(p not in r.instance_ids for p in r.load_failed_instance_ids),
         lambda i, r: add(i, [p for p in r.load_failed_instance_ids if p not in r.instance_ids][0], ROP_DEREGISTER, last_used=0)),
        (lambda r: both(r), lambda i, r: add(i, both(r)[0], ROP_DEREGISTER, last_used=0)),
        (lambda r: absent(r) is not None, lambda i, r: add(i, absent(r), ROP_DEREGISTER, last_used=0)),
        # SCALE_DOWN
        (lambda r: absent(r) is not None, lambda i, r: add(i, absent(r), ROP_SCALE_DOWN, last_used=now, load_time=now)),
        (lambda r: nl(r) >= 1, lambda i, r: add(i, first(r.instance_ids), ROP_SCALE_DOWN, last_used=now, load_time=r.instance_ids[first(r.instance_ids)] - 1)),
        (lambda r: nl(r) >= 3 and not both(r), lambda i, r: add(i, list(r.instance_ids)[1], ROP_SCALE_DOWN, last_used=0, load_time=list(r.instance_ids.values())[1])),
        (lambda r: both(r), lambda i, r: add(i, both(r)[0], ROP_SCALE_DOWN, last_used=now, load_time=r.instance_ids[both(r)[0]])),
    ]
    # the recipes that need a rare shape choose first, so that no other recipe takes their record
    rare = (1, 6, 11, 12, 13, 14, 15, 17, 18, 19, 20, 25)
    for pred, write in [recipes[k] for k in rare] + [r for k, r in enumerate(recipes) if k not in rare]:
        if len(rows) >= n:
            break
        i, r = find(pred)
        if i is not None:
            write(i, r)
    # the rest at random: an instance of the record (either list) or a stranger, the right time or a wrong one
    for i in idx:
        if len(rows) >= n:
            break
        if i in used:
            continue
        used.add(i)
        r = registry[i]
        known = [p for p in list(r.instance_ids) + list(r.load_failed_instance_ids) if 0 <= p < P]
        pod = int(rng.choice(known)) if known and rng.random() < 0.7 else int(rng.integers(0, P))
        lt = r.instance_ids.get(pod, now) + int(rng.random() < 0.25)
        lct = r.load_failed_instance_ids.get(pod, now) + int(rng.random() < 0.25)
        add(i, pod, int(rng.integers(0, 4)), flags=int(rng.integers(0, 4)), last_used=int(rng.choice([-1, 0, now - 50, now, r.last_used])),
            load_time=lt, load_complete_time=lct)
    ops = ops_array(rows)
    return ops[rng.permutation(len(ops))] if len(ops) else ops
