"""The model counts every instance keeps beside its registry view, restated in Python: the registry listener event()
(MM.java:2807-2854) with its two id sets, logModelCountMetrics (:6852-6863) and hasRegistration (:2856-2858).

Two forms.  `Listener` is literal and sequential: it takes registry events one by one, keeps loadedModelIds and failedModelIds
as two Python sets exactly as :2828-2831 does, and cites the Java line at every step; `census_sequential` replays a registry
through it and asks hasRegistration record by record and instance by instance.  `census_closed` is the vectorised numpy form
of the closed rule (include/mmplace.h, mmp_registry_census): membership of a record in either set depends on the record alone,
so the sizes of the sets are counts over the registry as it stands and the per-instance numbers are np.bincount over the
entries.  The device code follows the second form.  tests/test_registry_census_model.py holds the two against each other.

The reference has no test that names loadedModelIds, failedModelCount or logModelCountMetrics, so there are no reference
vectors for them: the restatement is read against the Java text.

Not restated: the `initialized` gate and the leader / metrics switches (:2833-2853) decide WHEN the numbers are published, not
what they are; vModelManager.processModelChange (:2841) is another subsystem.
"""
from __future__ import annotations

import numpy as np

from modelmesh_amd._lib import REGISTRY_STATS, REGISTRY_TYPE_STATS
from tests.registry_prune_model import LONG_MAX, Record, registry_from_arrays

ENTRY_ADDED, ENTRY_UPDATED, ENTRY_DELETED = "ENTRY_ADDED", "ENTRY_UPDATED", "ENTRY_DELETED"

SCALARS = ("n_models", "n_loaded", "n_failed", "n_loaded_and_failed", "n_unloaded_used", "n_last_used_max", "n_entries_loaded",
           "n_entries_failed", "n_entries_unresolved", "max_copies")


def has_load_failure(record: Record) -> bool:
    return len(record.failed) != 0                                   # ModelRecord.java:181-183


def has_registration(record: Record, instance: int) -> bool:         # :2856-2858
    return any(p == instance for p, _ in record.loaded) or any(p == instance for p, _ in record.failed)


class Listener:
    """What event() maintains: the registry view (key -> record), loadedModelIds, failedModelIds and the two published counts."""

    def __init__(self):
        self.registry = {}
        self.loaded_model_ids, self.failed_model_ids = set(), set()
        self.loaded_model_count = self.failed_model_count = -1         # (until the first change)

    def event(self, type, key, record):
        if type == ENTRY_DELETED:                                     # (the kv-store's view: what registry.getCount() counts)
            self.registry.pop(key, None)
        else:
            self.registry[key] = record
        loaded = type != ENTRY_DELETED and len(record.loaded) != 0    # :2828 !record.getInstanceIds().isEmpty()
        failed = type != ENTRY_DELETED and has_load_failure(record)   # :2829 record.hasLoadFailure()
        loaded_changed = self._put(self.loaded_model_ids, key, loaded)  # :2830 loaded ? add(key) : remove(key)
        failed_changed = self._put(self.failed_model_ids, key, failed)  # :2831
        if loaded_changed:
            self.loaded_model_count = len(self.loaded_model_ids)      # :2844
        if failed_changed:
            self.failed_model_count = len(self.failed_model_ids)      # :2845

    @staticmethod
    def _put(ids, key, member):
        """Set.add / Set.remove: True iff the set changed."""
        if member:
            if key in ids:
                return False
            ids.add(key)
            return True
        if key in ids:
            ids.remove(key)
            return True
        return False

    def counts(self):
        """(MODELS_LOADED, MODELS_WITH_LOAD_FAIL, TOTAL_MODELS) as logModelCountMetrics reads them (:6860-6862)."""
        return len(self.loaded_model_ids), len(self.failed_model_ids), len(self.registry)

    def records(self):
        """The registry view in key order (keys are registry rows here)."""
        return [self.registry[k] for k in sorted(self.registry)]


def _empty(n_pods, n_types):
    return (np.zeros(1, dtype=REGISTRY_STATS)[0], np.zeros(n_pods, np.int32), np.zeros(n_pods, np.int32),
            np.zeros(n_types, dtype=REGISTRY_TYPE_STATS))


def census_sequential(registry, n_pods, n_types):
    """(stats, pod_loaded, pod_failed, type_stats) of a list of Record, one record at a time."""
    stats, pod_loaded, pod_failed, types = _empty(n_pods, n_types)
    lst = Listener()
    per_instance = {}                                                 # instance -> [in instanceIds, in loadFailedInstanceIds]
    for key, mr in enumerate(registry):
        lst.event(ENTRY_ADDED, key, mr)
        for inst in {p for p, _ in mr.loaded + mr.failed}:
            assert has_registration(mr, inst)                         # :2856-2858, split by list below
            c = per_instance.setdefault(inst, [0, 0])
            c[0] += sum(1 for p, _ in mr.loaded if p == inst)         # record.getInstanceIds().containsKey(instance)
            c[1] += sum(1 for p, _ in mr.failed if p == inst)         # record.loadFailedInInstance(instance)
        loaded, failed = key in lst.loaded_model_ids, key in lst.failed_model_ids
        stats["n_loaded_and_failed"] += loaded and failed
        stats["n_unloaded_used"] += (not loaded) and 0 < mr.last_used < LONG_MAX    # the population :6574 draws from
        stats["n_last_used_max"] += mr.last_used == LONG_MAX          # :6843
        stats["n_entries_loaded"] += len(mr.loaded)
        stats["n_entries_failed"] += len(mr.failed)
        stats["copies_hist"][min(len(mr.loaded), 4)] += 1
        stats["max_copies"] = max(int(stats["max_copies"]), len(mr.loaded))
        if 0 <= mr.type < n_types:
            t = types[mr.type]
            t["n_models"] += 1
            t["n_loaded"] += loaded
            t["n_failed"] += failed
            t["n_entries_loaded"] += len(mr.loaded)
    stats["n_loaded"], stats["n_failed"], stats["n_models"] = lst.counts()  # :6860-6862
    for inst, (nl, nf) in per_instance.items():
        if 0 <= inst < n_pods:
            pod_loaded[inst], pod_failed[inst] = nl, nf
        else:                                                         # an id the instance table does not know
            stats["n_entries_unresolved"] += nl + nf
    return stats, pod_loaded, pod_failed, types


def census_closed(models, ent_pod, n_pods, n_types):
    """The same numbers as array arithmetic over the arena (rows may lie anywhere in it, with garbage between)."""
    stats, _, _, types = _empty(n_pods, n_types)
    nl, nf = models["n_loaded"].astype(np.int64), models["n_failed"].astype(np.int64)
    lu = models["last_used"]
    loaded, failed = nl > 0, nf > 0
    stats["n_models"] = len(models)
    stats["n_loaded"], stats["n_failed"], stats["n_loaded_and_failed"] = loaded.sum(), failed.sum(), (loaded & failed).sum()
    stats["n_unloaded_used"] = (~loaded & (lu > 0) & (lu < LONG_MAX)).sum()
    stats["n_last_used_max"] = (lu == LONG_MAX).sum()
    stats["n_entries_loaded"], stats["n_entries_failed"] = nl.sum(), nf.sum()
    stats["copies_hist"] = np.bincount(np.minimum(nl, 4), minlength=5)
    stats["max_copies"] = nl.max() if len(models) else 0
    # the compacted arena: entry -> (model, position in its lists)
    k = nl + nf
    seg = np.repeat(np.arange(len(models)), k)
    start = np.zeros(len(models) + 1, np.int64)
    np.cumsum(k, out=start[1:])
    pos = np.arange(int(start[-1])) - start[seg]
    pod = np.asarray(ent_pod)[models["ent_off"][seg].astype(np.int64) + pos].astype(np.int64) if len(seg) else np.zeros(0, np.int64)
    in_failed = pos >= nl[seg]
    resolved = (pod >= 0) & (pod < n_pods)
    stats["n_entries_unresolved"] = (~resolved).sum()
    pod_loaded = np.bincount(pod[resolved & ~in_failed], minlength=n_pods).astype(np.int32)
    pod_failed = np.bincount(pod[resolved & in_failed], minlength=n_pods).astype(np.int32)
    typed = (models["type"] >= 0) & (models["type"] < n_types)
    ty = models["type"][typed]
    types["n_models"] = np.bincount(ty, minlength=n_types)
    types["n_loaded"] = np.bincount(ty[loaded[typed]], minlength=n_types)
    types["n_failed"] = np.bincount(ty[failed[typed]], minlength=n_types)
    types["n_entries_loaded"] = np.bincount(ty, weights=nl[typed], minlength=n_types).astype(np.int64)
    return stats, pod_loaded, pod_failed, types


def census_of_arrays(models, ent_pod, ent_time, n_pods, n_types):
    """census_sequential of a registry held as arrays."""
    return census_sequential(registry_from_arrays(models, ent_pod, ent_time), n_pods, n_types)


def assert_same_census(got, want, what=""):
    """Field for field and array for array; all integers, exact."""
    gs, gl, gf, gt = got
    ws, wl, wf, wt = want
    for f in SCALARS:
        assert int(gs[f]) == int(ws[f]), (what, f, int(gs[f]), int(ws[f]))
    assert np.array_equal(gs["copies_hist"], ws["copies_hist"]), (what, gs["copies_hist"], ws["copies_hist"])
    assert np.array_equal(gl, wl), (what, "pod_loaded", np.nonzero(gl != wl)[0][:8])
    assert np.array_equal(gf, wf), (what, "pod_failed", np.nonzero(gf != wf)[0][:8])
    assert len(gt) == len(wt), (what, len(gt), len(wt))
    for f in ("n_models", "n_loaded", "n_failed", "n_entries_loaded"):
        assert np.array_equal(gt[f], wt[f]), (what, "type " + f, gt[f][:8], wt[f][:8])
