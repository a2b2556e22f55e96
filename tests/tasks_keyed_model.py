"""The periodic tasks BY MODEL ID (mmp_scaleup_plan_k, mmp_scaledown_plan_k, mmp_migration_plan_k, mmp_janitor_plan_k) restated.

The Java loops iterate runtimeCache, whose keys are model ids, and begin each entry with `registry.get(modelId)` (MM.java:5672-5690
the rate task, :5896-5903 the janitor's cache loop, :6998-7010 preShutdown).  So the registry here is a dict from id bytes to record,
and resolution is a dict lookup: an unknown id, and an id whose record was deleted, give None — `model == -1` in the entry structs.
Beside the dict the world keeps `ids`, the device's model-id table (row -> id; a deletion does not take the row away until
mmp_models_retire renumbers), only to answer model_idx as the library does and to lay the records out by row for the restatements
the by-row calls are already held to:

  * the janitor: the sequential form `Janitor.run` of tests/janitor_model.py;
  * the rate task, the scale-down, the migration: oracle.bind (the C oracle) — `oracle/py_rebalance.py` restates the same text.

The janitor's scale-down in the same call is DEFINED as the janitor, applied, followed by the scale-down on the candidates it
returned, the MaxConcCacheEntry row of a candidate being the one of the INPUT row it came from.

One convention is the library's, not the Java's: a record that is all zero (type 0, no entries, lastUsed 0) IS the empty row a
deleted record leaves (retire_row_empty), so by key it is no record.  `get` says so.
"""
from __future__ import annotations

import copy

import numpy as np

from modelmesh_amd._lib import CACHE_ENTRY, JANITOR_ENTRY
from oracle import bind
from tests.janitor_model import Janitor
from tests.registry_prune_model import Record, registry_to_arrays


class InvalidEntries(Exception):
    """What the library answers MMP_EINVAL for, with nothing written or changed."""


def _bytes(k):
    return k if isinstance(k, bytes) else k.encode()


def is_empty(r):
    return r.type == 0 and not r.loaded and not r.failed and r.last_used == 0


def _up(params):
    return np.ascontiguousarray(params).reshape(1).view(bind.ORC_SCALEUP_PARAMS)


def _down(params):
    return np.ascontiguousarray(params).reshape(1).view(bind.ORC_SCALEDOWN_PARAMS)


class TaskWorld:
    """fleet: the instance table and everything else the tasks read (its registry arrays are ignored).  ids: row -> id.
    registry: dict id -> Record."""

    def __init__(self, fleet, ids, records):
        self.fleet = fleet
        self.ids = [_bytes(k) for k in ids]
        self.registry = {k: r for k, r in zip(self.ids, records) if r is not None and not is_empty(r)}

    # -- what the listeners do to the table (not part of the calls) --
    def delete(self, key):                       # ENTRY_DELETED: the record goes, the row stays, empty
        self.registry.pop(_bytes(key), None)

    def put(self, key, rec):                     # an event for the id: a known id keeps its row, a new one joins at the end
        key = _bytes(key)
        if key not in self.ids:
            self.ids.append(key)
        self.registry[key] = rec

    def retire(self, rows):                      # mmp_models_retire: the rows leave, the ones behind move up
        gone = {self.ids[r] for r in rows}
        assert not any(self.get(k) is not None for k in gone)
        self.ids = [k for k in self.ids if k not in gone]

    # -- the lookup --
    def row(self, key):                          # what mmp_model_ids_resolve answers
        key = _bytes(key)
        return self.ids.index(key) if key in self.ids else -1

    def get(self, key):                          # registry.get(modelId)
        r = self.registry.get(_bytes(key))
        return None if r is None or is_empty(r) else r

    def resolve(self, keys):
        """(model_idx, the `model` field the tasks see): the table's row, and that row only where registry.get is not null."""
        at = {k: i for i, k in enumerate(self.ids)}
        idx = np.array([at.get(_bytes(k), -1) for k in keys], np.int32).reshape(-1)
        live = np.array([i if self.get(k) is not None else -1 for i, k in zip(idx, keys)], np.int32).reshape(-1)
        return idx, live

    def records_by_row(self):
        return [self.registry.get(k) or Record(0, [], [], 0) for k in self.ids]

    def by_row(self, rows=None):
        """The fleet with the registry laid out by row, as the by-row restatements take it."""
        f = copy.copy(self.fleet)
        f.models, f.ent_pod, f.ent_time = registry_to_arrays(self.records_by_row() if rows is None else rows)
        return f

    def staged(self, entries, keys, dtype=CACHE_ENTRY):
        entries = np.ascontiguousarray(entries, dtype=dtype).copy()
        assert len(entries) == len(keys)
        idx, live = self.resolve(keys)
        entries["model"] = live                  # the field the caller sent is never read
        return idx, entries

    # -- the three read-only tasks --
    def scaleup(self, entries, keys, params, conc=None, conc_params=None):
        """rateTrackingTask: (model_idx, outs, overloaded, skipped) or, latency-based, (model_idx, outs, conc_outs, overloaded,
        skipped, result)."""
        idx, e = self.staged(entries, keys)
        if conc_params is None:
            return (idx,) + tuple(bind.scaleup_plan(self.by_row(), e, _up(params)))
        return (idx,) + tuple(bind.scaleup_plan_conc(self.by_row(), e, conc, _up(params), conc_params))

    def scaledown(self, entries, keys, params, conc=None, dyn_const=0):
        idx, e = self.staged(entries, keys)
        f = self.by_row()
        return idx, (bind.scaledown_plan(f, e, _down(params)) if conc is None else bind.scaledown_plan_conc(f, e, conc, _down(params), dyn_const))

    def migration(self, entries, keys, self_pod, now, cutoff_age_ms=3_600_000):
        idx, e = self.staged(entries, keys)
        return (idx,) + tuple(bind.migration_plan(self.by_row(), e, self_pod, now, cutoff_age_ms))

    # -- the janitor, and its scale-down --
    def janitor(self, entries, keys, prm, dry=False, scaledown=None, conc=None, dyn_const=0):
        """(model_idx, actions, edits, candidates, candidate rows, removed or None, info).  Edits the records unless dry.  The
        cache has one entry per model id: two entries that find the same record are refused (two that find none are two
        unknown ids, each removed on its own, :5968)."""
        if scaledown is not None:
            if dry:
                raise InvalidEntries("the scale-down reads the registry the two loops left: it needs the apply")
            if int(np.asarray(scaledown).reshape(-1)[0]["self_pod"]) != int(np.asarray(prm).reshape(-1)[0]["self_pod"]):
                raise InvalidEntries("self_pod")
        elif conc is not None:
            raise InvalidEntries("conc without scaledown")
        idx, e = self.staged(entries, keys, JANITOR_ENTRY)
        named = e["model"][e["model"] >= 0]
        if len(np.unique(named)) != len(named):
            raise InvalidEntries("two entries name one record")
        rows = self.records_by_row()
        actions, edits, cands, crow, info = Janitor().run(rows, e, prm, self.fleet.pods["id_order"], dry=dry)
        if not dry:
            for k, r in zip(self.ids, rows):
                if k in self.registry or not is_empty(r):
                    self.registry[k] = r
        removed = None
        if scaledown is not None:                                       # :6110-6145 on the registry as the loops left it
            f = self.by_row(rows)
            removed = (bind.scaledown_plan(f, cands, _down(scaledown)) if conc is None else
                       bind.scaledown_plan_conc(f, cands, np.ascontiguousarray(conc)[crow], _down(scaledown), dyn_const))
        return idx, actions, edits, cands, crow, removed, info


# ---- the recipe of the chain tests (tests/test_tasks_keyed_model.py checks that it shows what it is meant to show) ------------

CHAIN_SELF = 2


def chain_world(n_models=300, n_hot=70, seed=0):
    """An 8-instance fleet that is nearly full (removeModelCopies only runs below 5 % free, :6224) whose instance CHAIN_SELF holds a
    copy of the first n_hot models, two other old copies beside it: every one of them is a scale-down candidate, oldest first by
    its number.  Returns (world, now): ids b"hot-%d" / b"m%d"."""
    from modelmesh_amd import workload as wl
    from tests.janitor_model import put_in_id_order
    fleet = wl.fuzz_fleet(seed + 4100, pods=8, models=n_models)
    now = int(fleet.now)
    p = fleet.pods
    p["flags"] = 2
    p["used"] = (p["capacity"] * 0.97).astype(np.int64)
    io = p["id_order"]
    others = [q for q in range(8) if q != CHAIN_SELF]
    recs = []
    for m in range(n_models):
        r = Record(0, [], [], now - 3_600_000)
        if m < n_hot:
            for q, t in ((CHAIN_SELF, now - 40_000_000 - m), (others[m % 7], now - 50_000_000), (others[(m + 1) % 7], now - 60_000_000)):
                put_in_id_order(r.loaded, q, t, io)
        elif m % 3:
            put_in_id_order(r.loaded, others[m % 7], now - 50_000_000, io)
        recs.append(r)
    fleet.models, fleet.ent_pod, fleet.ent_time = registry_to_arrays(recs)
    ids = [b"hot-%d" % m if m < n_hot else b"m%d" % m for m in range(n_models)]
    return TaskWorld(fleet, ids, recs), now


def chain_entries(world, now, hot, recent=(), weight=100):
    """Cache rows for the hot models `hot` (MRU first, so the OLDEST candidate is the last row), in order with the registry —
    except those in `recent`, whose loadTimestamp is a second old: the cache loop re-registers the copy with that time (:5980),
    and a copy loaded within 30 minutes keeps every copy of its model (:6268)."""
    from modelmesh_amd._lib import JE_DONE, JE_STATE_LIVE
    e = np.zeros(len(hot), dtype=JANITOR_ENTRY)
    for r, m in enumerate(hot):
        lt = dict(world.get(b"hot-%d" % m).loaded)[CHAIN_SELF]
        e[r] = (-1, weight, now - 2_000_000 - 10 * r, now - 1000 if m in recent else lt, 0, -1, 0, now - 30_000_000, 0, 0, 0,
                JE_DONE | JE_STATE_LIVE, 0)
    return e, [b"hot-%d" % m for m in hot]


def chain_scaledown(now, cap=10_000_000, self_pod=CHAIN_SELF):
    from modelmesh_amd._lib import SCALEDOWN_PARAMS
    dp = np.zeros(1, dtype=SCALEDOWN_PARAMS)
    dp["self_pod"], dp["now"], dp["last_check_time"], dp["rate_check_interval_ms"] = self_pod, now, now - 7_000, 10_000
    dp["adjusted_cache_capacity"], dp["scale_up_rpm_threshold"] = cap, 2000
    return dp


def conc_rows(n, queued=()):
    """MaxConcCacheEntry rows without enough samples for a threshold of their own; `queued`: rows with two queued requests (:6303)."""
    from modelmesh_amd._lib import CONC_ENTRY
    c = np.zeros(n, dtype=CONC_ENTRY)
    c["max_conc"] = 4
    for r in queued:
        c["queued_requests"][r] = 2
    return c
