"""The leader reaper's first half, restated in Python: pruneModelRegistry (MM.java:6524-6609) with
pruneMissingInstances (:6752-6784) and repairLastUsedTimeIfNeeded (:6837-6850).

Two forms.  `Reaper.run` is literal and sequential: it walks the registry in order, keeps `missings` in a dict as the Java
does and cites the Java line at every step.  `closed_rule` is the vectorised numpy form of the closed rule the device code
uses (include/mmplace.h, mmp_registry_prune): with one clock value per run, putIfAbsent(pod, now) can only matter for pods
without a mark, whose entries are then never removed in that run.  tests/test_registry_prune_model.py holds the two against
each other.

The reference has no test that names this code (nothing under its src/test mentions pruneModelRegistry,
pruneMissingInstances or missings).  The vectors are the text's own answers: the methods are cut out of the reference tree and
compiled by oracle/ref_harness/registry_harness.cc, tests/golden/ref_registry_edges.npz holds what they did over sequences of runs
at the value edges (tests/ref_registry_edges.py), and tests/test_registry_edges.py holds both forms below to every run.

One run uses ONE clock value (the library's convention); the Java reads currentTimeMillis() per record (:6758, :6603, :6844).
Not restated: readOnlyMode (:6543-6550), loadFailureInfos (:6779), the kv-error counter (:6583-6600) and the
conditional-set retry (:6555-6562): a record is what the registry holds.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from modelmesh_amd._lib import MODEL_ROW, POD_TOMBSTONE, PRUNE_EDIT, PRUNE_REMOVED

LONG_MAX = 2**63 - 1
GONE_AFTER_MS = 600_000            # ASSUME_INSTANCE_GONE_AFTER_MS
REAPER_FREQ_MS = 7 * 60_000        # REGISTRY_REAPER_FREQ_MINS
LASTUSED_AGE_ON_ADD_MS = 3_600_000


def jsub(a: int, b: int) -> int:
    """Java long subtraction (wraps)."""
    return ((int(a) - int(b) + 2**63) % 2**64) - 2**63


@dataclass
class Record:
    """One ModelRecord: instanceIds and loadFailedInstanceIds as (pod, time) lists in TreeMap order."""
    type: int
    loaded: list
    failed: list
    last_used: int


def registry_from_arrays(models, ent_pod, ent_time):
    out = []
    for m in models:
        o, nl, nf = int(m["ent_off"]), int(m["n_loaded"]), int(m["n_failed"])
        ents = [(int(ent_pod[o + k]), int(ent_time[o + k])) for k in range(nl + nf)]
        out.append(Record(int(m["type"]), ents[:nl], ents[nl:], int(m["last_used"])))
    return out


def registry_to_arrays(registry):
    """Compact arrays (rows in order, a row's entries in order, no gaps)."""
    models = np.zeros(len(registry), dtype=MODEL_ROW)
    pods, times = [], []
    for i, r in enumerate(registry):
        models[i] = (r.type, len(pods), len(r.loaded), len(r.failed), r.last_used)
        for p, t in r.loaded + r.failed:
            pods.append(p)
            times.append(t)
    return models, np.array(pods, np.int32).reshape(-1), np.array(times, np.int64).reshape(-1)


def compact(models, ent_pod, ent_time):
    """The registry a device arena holds (rows may point anywhere, with garbage between), in compact form."""
    return registry_to_arrays(registry_from_arrays(models, ent_pod, ent_time))


@dataclass
class Reaper:
    """The state the leader keeps across reaper runs: `missings` (instance -> first time seen missing)."""
    missings: dict = field(default_factory=dict)

    def run(self, pod_flags, registry, self_pod, now, gone_after=GONE_AFTER_MS, age_on_add=LASTUSED_AGE_ON_ADD_MS,
            candidates_enabled=True, global_lru=0, dry=False):
        """One pruneModelRegistry pass.  Edits `registry` (a list of Record) in place unless dry; returns
        (edits PRUNE_EDIT[], removed PRUNE_REMOVED[], info dict, candidates list of model indices)."""
        n_pods = len(pod_flags)
        missings = dict(self.missings) if dry else self.missings
        edits, removed, candidates = [], [], []
        n_unresolved = n_repaired = n_new = 0

        def prune_missing_instances(instances, is_failed, out):  # :6752-6784
            nonlocal n_unresolved, n_new
            keep = []
            for pod, time in instances:                             # :6759 entry (TreeMap) order
                if jsub(now, time) < gone_after:                    # :6761 ignore recently loaded
                    keep.append((pod, time))
                    continue
                if pod == self_pod:                                 # :6765 we think therefore we are
                    keep.append((pod, time))
                    continue
                if pod < 0 or pod >= n_pods:                        # an id the pod table does not hold: not ours to judge
                    n_unresolved += 1
                    keep.append((pod, time))
                    continue
                if not pod_flags[pod] & POD_TOMBSTONE:              # :6769-6771 present (a shutting-down row still is)
                    keep.append((pod, time))
                    continue
                missing_since = missings.get(pod)                   # :6776 putIfAbsent returns the previous value
                if missing_since is None:
                    missings[pod] = now
                    n_new += 1
                if missing_since is not None and jsub(now, missing_since) > gone_after:  # :6777
                    out.append((pod, 1 if is_failed else 0, time))  # :6778 it.remove()
                else:
                    keep.append((pod, time))
            return keep

        for i, mr in enumerate(registry):                           # :6536 registry order
            out = []
            loaded = prune_missing_instances(mr.loaded, False, out)  # :6552
            failed = prune_missing_instances(mr.failed, True, out)   # :6553
            last_used, repaired = mr.last_used, False
            if mr.last_used == LONG_MAX:                            # :6843
                last_used, repaired = jsub(now, 3 * age_on_add), True  # :6844
                n_repaired += 1
            if out or repaired:                                     # :6555 conditionalSetAndGet / :6845 conditionalSet
                edits.append((i, len(loaded), len(failed), 1 if repaired else 0, len(removed), len(out), last_used))
                removed.extend(out)
                if not dry:
                    mr.loaded, mr.failed, mr.last_used = loaded, failed, last_used
            # :6574-6577 (insts / failInsts are the pruned maps, lastUsed the repaired one)
            if candidates_enabled and not loaded and len(failed) < 2 and (global_lru == 0 or last_used > global_lru):
                candidates.append(i)

        # :6601-6606 clean out old entries from the missings map
        for pod in list(missings):
            present = pod < n_pods and not pod_flags[pod] & POD_TOMBSTONE
            if jsub(now, missings[pod]) > gone_after or present:
                del missings[pod]
        info = dict(n_edits=len(edits), n_removed=len(removed), n_repaired=n_repaired, n_unresolved=n_unresolved,
                    n_missing_pods=len(missings), n_new_missing=n_new, truncated=0)
        return (np.array(edits, dtype=PRUNE_EDIT).reshape(-1), np.array(removed, dtype=PRUNE_REMOVED).reshape(-1), info,
                candidates)

    def clear(self):
        """missings.clear() on a leader change (:6827)."""
        self.missings.clear()


def closed_rule(pod_flags, models, ent_pod, ent_time, since, self_pod, now, gone_after=GONE_AFTER_MS,
                age_on_add=LASTUSED_AGE_ON_ADD_MS):
    """The same run as array arithmetic.  `since`: int64 per pod slot, 0 = no mark (len(since) >= len(pod_flags)).
    Returns (edits, removed, info, since_after, keep mask over the entries)."""
    pod_flags = np.asarray(pod_flags)
    n_pods, n_ent = len(pod_flags), len(ent_pod)
    since = np.asarray(since, np.int64)
    k = models["n_loaded"].astype(np.int64) + models["n_failed"]
    # entry -> (model, position in its lists); rows may lie anywhere in the arena
    seg = np.repeat(np.arange(len(models)), k)
    start = np.zeros(len(models) + 1, np.int64)
    np.cumsum(k, out=start[1:])
    pos = np.arange(int(start[-1])) - start[seg]
    idx = models["ent_off"][seg].astype(np.int64) + pos
    pod, time = ent_pod[idx].astype(np.int64), ent_time[idx].astype(np.int64)
    with np.errstate(over="ignore"):
        age = np.int64(now) - time                                               # wraps as the Java does
        examined = ~(age < gone_after) & (pod != self_pod)
        resolved = (pod >= 0) & (pod < n_pods)
        spod = np.where(resolved, pod, 0)
        tomb = (pod_flags[spod] & POD_TOMBSTONE) != 0 if n_pods else np.zeros(len(pod), bool)
        missing = examined & resolved & tomb
        mark = since[spod] if n_pods else np.zeros(len(pod), np.int64)
        due = (mark != 0) & ((np.int64(now) - mark) > gone_after)
    gone = missing & due
    failed = pos >= models["n_loaded"][seg]
    rm_l = np.bincount(seg[gone & ~failed], minlength=len(models))
    rm_f = np.bincount(seg[gone & failed], minlength=len(models))
    repaired = models["last_used"] == LONG_MAX
    edit = (rm_l + rm_f > 0) | repaired
    em = np.nonzero(edit)[0]
    edits = np.zeros(len(em), dtype=PRUNE_EDIT)
    edits["model"] = em
    edits["n_loaded_after"] = models["n_loaded"][em] - rm_l[em]
    edits["n_failed_after"] = models["n_failed"][em] - rm_f[em]
    edits["flags"] = repaired[em]
    edits["n_removed"] = (rm_l + rm_f)[em]
    edits["removed_off"] = np.cumsum(edits["n_removed"]) - edits["n_removed"]
    edits["last_used_after"] = np.where(repaired[em], jsub(now, 3 * age_on_add), models["last_used"][em])
    removed = np.zeros(int(gone.sum()), dtype=PRUNE_REMOVED)
    removed["pod"], removed["failed"], removed["time"] = pod[gone], failed[gone], time[gone]
    # the map: new marks first, then the cleanup
    after = since.copy()
    seen = np.zeros(len(since), bool)
    seen[pod[missing]] = True
    fresh = seen & (after == 0)
    after[fresh] = now
    present = np.zeros(len(since), bool)
    present[:n_pods] = (pod_flags & POD_TOMBSTONE) == 0
    with np.errstate(over="ignore"):
        drop = (after != 0) & (((np.int64(now) - after) > gone_after) | present)
    after[drop] = 0
    info = dict(n_edits=len(edits), n_removed=len(removed), n_repaired=int(repaired.sum()),
                n_unresolved=int((examined & ~resolved).sum()), n_missing_pods=int((after != 0).sum()),
                n_new_missing=int(fresh.sum()), truncated=0)
    keep = np.ones(n_ent, bool)
    keep[idx[gone]] = False
    return edits, removed, info, after, keep
