"""The definition the eviction loop by id is held to.

(a) THE VICTIMS' lastUsed — what the clhm hands its listener (ConcurrentLinkedHashMap.java:578-586: node.getLastUsed() at
notification; a dead node is touched by nobody, so it is the time the node had when evict() unlinked it, :329-352) — derived two ways:

  1. victim_times(): oracle.bind.CCache stepped one operation at a time, nodes() read in front of each.  An operation writes the
     time of its OWN node only (Node.touch, clhm :1357-1360, is called on the node the operation found or made: :383 afterRead,
     :646 UpdateTask, :825-834 put), so a victim that is not the operation's own key has the lastUsed it had in front of the
     operation.  A victim that IS the operation's own key has what the operation stamped on it before evict() ran:
       a put of an absent key        the new node, lastUsed 0, touched with the put's time: `now` for 0, else the time (:1357-1360)
       a weight update (UpdateTask)  touched only if newTime >= 0 and newTime != lastUsed (:646-647): `now` for 0, else
                                     max(lastUsed, newTime) (:1358); otherwise the time it had
       a read stamped <= 0           is a read "now" (:383) — a read never evicts, listed for completeness
       the manager's quiet updates   (adjustNewEntrySpaceRequest, adjustWeightAfterLoad: replaceQuietly) leave the time alone
  2. TimedClhm / timed_stream(): oracle/py_oracle.py's Clhm with an _evict that also records node[1], under py_oracle's
     UnloadBufManager.  Its domain is narrower than the streams' (py_oracle keeps a weights dict the Java does not have, and reads
     stamp max(lastUsed, t) for any t != 0): a cache is followed up to the first operation outside it — in_domain().

(b) mmp_evictions_k — evictions_run() further down.
"""
import numpy as np

from oracle import bind as ob
from oracle import py_oracle as po

UB = -1000000
INSERTING = (0, 4, 12)
KEYLESS = (6, 7, 9, 11)


# ---- (a) 1: the C oracle, stepped ---------------------------------------------------------------------------------------------------

def own_key_time(op, time, now, before):
    """what operation `op` leaves on its own node before evict() runs; before: the node's lastUsed in front of it, None if absent"""
    if op in INSERTING:
        if before is None:
            return now if time == 0 else time           # Node.touch on the fresh node (lastUsed 0), clhm :1357-1360
        return now if time == 0 else max(before, time)  # a put of a present key is a read (:832)
    if op == 2 and before is not None and time >= 0 and time != before:  # UpdateTask :646-647
        return now if time == 0 else max(before, time)
    if op == 1 and before is not None:                  # afterRead :383: a read stamped <= 0 is "now"
        return now if time <= 0 else max(before, time)
    return before


def victim_times(caps, reserved, ops, now):
    """per operation the list of (key, lastUsed) of its victims in listener order"""
    caches = [ob.CCache(int(caps[c]), None if reserved[c] < 0 else int(reserved[c]), now) for c in range(len(caps))]
    out = []
    for o in ops:
        h = caches[int(o["cache"])]
        lu, _, key = h.nodes()
        op, k = int(o["op"]), int(o["key"])
        _, evk = h.apply(op, k, int(o["arg"]), int(o["time"]), int(o["flag"]), now)
        before = {int(a): int(t) for a, t in zip(key, lu)} if evk else {}
        own = None if op in KEYLESS else k
        out.append([(int(v), own_key_time(op, int(o["time"]), now, before.get(v)) if v == own else before[v]) for v in evk])
        if h.u is not None and h.u.n_evicted > 900:
            h.u.n_evicted = 0
    return out


# ---- (a) 2: py_oracle with a recording _evict --------------------------------------------------------------------------------------

class TimedClhm(po.Clhm):
    """Clhm whose _evict() also records node[1] of every node it pops"""

    def __init__(self, capacity):
        super().__init__(capacity)
        self.victims = []  # (key, lastUsed) in the order evict() unlinks them

    def _evict(self):  # clhm :329-352
        out = []
        self.lastEvictedWeights = []
        while self.weightedSize > self.capacity:
            if not self.deque:
                break
            node = self.deque.pop(0)
            self.weightedSize -= abs(node[2])
            out.append(node[0])
            self.lastEvictedWeights.append(node[2])
            self.victims.append((node[0], node[1]))
        return out


class TimedManager(po.UnloadBufManager):
    """UnloadBufManager that keeps, beside `evicted`, the time of each victim in LISTENER order (the order entryRemoved sees them:
    depth first, MM.java:2876-2878)"""

    def __init__(self, cache, reserved, now):
        self.times = []
        super().__init__(cache, reserved, now)

    def _on_evicted(self, keys):
        n = len(keys or [])
        mine = self.cache.victims[len(self.cache.victims) - n:] if n else []  # this evict()'s run, before any nested one
        ws = list(self.cache.lastEvictedWeights) if keys else []
        for (k, t), w in zip(mine, ws):
            self.weights.pop(k, None)
            self.evicted.append((k, w))
            self.times.append((k, t))
            self.entryRemoved(w)


def in_domain(u, o):
    """is operation o inside what TimedClhm / TimedManager restate, on a cache whose manager is u (None: plain)"""
    op, t, k = int(o["op"]), int(o["time"]), int(o["key"])
    if t < 0 and not (op == 2 and t == -1):
        return False
    if op == 1 and t < 0:
        return False
    if u is None:
        return op in (0, 1, 2, 3)
    if op in (0, 2, 3):  # past the manager: its weights dict would not follow
        return False
    if op in (5, 8) and k in u.weights:
        if op == 8 and u.weights[k] + int(o["arg"]) <= 0:  # a sum at or below zero: the weigher's abs() is not restated there
            return False
        if op == 5 and int(o["flag"]):
            return False
    return True


def timed_stream(caps, reserved, ops, now):
    """per operation the victims' (key, lastUsed) in listener order, or None from the first operation of its cache outside the
    domain on"""
    cs = [TimedClhm(int(c)) for c in caps]
    us = [None if reserved[c] < 0 else TimedManager(cs[c], int(reserved[c]), now) for c in range(len(caps))]
    dead = [False] * len(caps)
    out = []
    for o in ops:
        c = int(o["cache"])
        if dead[c] or not in_domain(us[c], o):
            dead[c] = True
            out.append(None)
            continue
        h, u = cs[c], us[c]
        op, k, arg, t, flag = int(o["op"]), int(o["key"]), int(o["arg"]), int(o["time"]), int(o["flag"])
        n0 = len(h.victims) if u is None else len(u.times)
        if op == 0:
            h.putIfAbsent(k, arg, t, now)
        elif op == 1:
            h.get(k, t, now)
        elif op == 2:
            h.updateWeight(k, arg, t, now)
        elif op == 3:
            h.remove(k)
        elif op == 4:
            u.insertNewEntry(k, arg, t, now)
        elif op == 5:
            if k in u.weights:  # an entry that is gone: nothing to adjust (the caller's CacheEntry is no longer in the map)
                u.adjustNewEntrySpaceRequest(arg, k, now)
        elif op == 6:
            u.cacheSpaceIsReady(arg)
        elif op == 7:
            u.claimRequestedSpaceIfReady(arg, now)
        elif op == 8:
            gone = k not in u.weights  # the sums move all the same, replaceQuietly finds no entry (:224-246, MM.java:1784-1786)
            if gone:
                u.weights[k] = 0
            u.adjustWeightAfterLoad(arg, k, now)
            if gone:
                u.weights.pop(k, None)
        elif op == 9:
            u.unloadComplete(arg, bool(flag), now)
        elif op == 10:
            u.removeEntry(k, now)
        elif op == 11:
            u.discardFailedEntry(arg, now)
        elif op == 12:
            u.insertFailedPlaceholderEntry(k, arg, t, now)
        got = (h.victims if u is None else u.times)[n0:]
        out.append([(UB if kk == po.UnloadBufManager.KEY else int(kk), int(tt)) for kk, tt in got])
    return out


def flat_times(outs, per_op, n_slots):
    """per_op laid out by the eviction slots of a replay's outs: (keys, times) with -1 / 0 in unused slots"""
    keys, times = np.full(n_slots, -1, np.int64), np.zeros(n_slots, np.int64)
    for g, vs in zip(outs, per_op):
        assert int(g["n_evicted"]) == len(vs)
        for j, (k, t) in enumerate(vs):
            keys[int(g["evicted_off"]) + j] = k
            times[int(g["evicted_off"]) + j] = t
    return keys, times


# ---- (b) mmp_evictions_k: the task body of ModelMesh.onEviction, literal and sequential ---------------------------------------------
# On top of tests/registry_ops_keyed_model.py: the registry is a dict from model id to ModelRecord (KeyedRegistry), the victims are
# taken one at a time, every step cites its Java line (MM.java unless said).  One convention is the library's: a victim whose id is
# unknown or names the empty row a deleted record leaves answers MMP_ROP_NO_RECORD with NO flag set — the call reads and edits
# nothing for it (the Java of a missing record makes no edit either, :2945; its log line for a failed entry is the caller's).

I64 = 2**64


def jsub(a, b):
    """Java long subtraction"""
    return (a - b + 2**63) % I64 - 2**63


class InvalidEvictions(ValueError):
    """what the library answers with MMP_EINVAL, nothing written or changed"""


def evictions_run(kreg, entries, keys, self_pod, now, load_timeout_ms, type_stats, dry=False):
    """kreg: registry_ops_keyed_model.KeyedRegistry (edited in place unless dry).  entries: EVICTED_ENTRY rows.  type_stats:
    typeSetStats per type row (total_capacity, total_free, instance_count fields), the committed snapshot's.
    -> (model_idx, outs EVICTED_OUT[], status uint8[], edits REGISTRY_OP_EDIT[], info dict)"""
    from modelmesh_amd import _lib
    from tests import registry_ops_keyed_model as rk
    from tests.registry_ops_model import InvalidOps, op_row, ops_array
    keys = [k if isinstance(k, bytes) else k.encode() for k in keys]
    assert len(keys) == len(entries)
    if now <= 0 or not 0 <= self_pod < len(kreg.id_order) or any(int(e["flags"]) & ~_lib.EVF_FAILED for e in entries):
        raise InvalidEvictions("argument")
    named = [k for k in keys if kreg.get(k) is not None]
    if len(set(named)) != len(named):
        raise InvalidEvictions("two victims name one record")
    n = len(entries)
    idx = np.array([kreg.row(k) for k in keys], np.int32).reshape(-1)
    outs, status, edits = np.zeros(n, dtype=_lib.EVICTED_OUT), np.zeros(n, np.uint8), []
    for i, (e, key) in enumerate(zip(entries, keys)):
        last_used = int(e["last_used"])
        millis = jsub(now, last_used)                                              # :2899 millisSinceLastUsed = now - lastUsed
        mr = kreg.get(key)                                                         # :2888 registry.get(key)
        if mr is None:
            status[i] = _lib.ROP_NO_RECORD
            outs[i] = (0, _lib.ROP_NO_RECORD, -1, millis)
            continue
        attempt = in_registry = False                                              # :2886
        failed = bool(int(e["flags"]) & _lib.EVF_FAILED)                           #       failed = ce.isFailed()
        loaded_time = None
        if not failed:                                                             # :2887
            loaded_time = mr.instance_ids.get(self_pod)                            # :2890 mr.getInstanceIds().get(instanceId)
            if loaded_time is None:                                                # :2891
                loaded_time = mr.load_failed_instance_ids.get(self_pod)            # :2892
            in_registry = loaded_time is not None                                  # :2894
            attempt = in_registry and jsub(now, loaded_time) > 2 * load_timeout_ms  # :2895
        log = in_registry or failed                                                # :2900
        the_type = mr.type                                                         # (read before the edit; the edit leaves it alone)
        # :2913 deregisterModel(key, lastUsed, ce.loadTimestamp, ce.loadCompleteTimestamp) -> :2940-2958, the restatement of
        # registry_ops_keyed_model (loadTime is the boxed primitive: never null, so MATCH_TIME)
        op = ops_array([op_row(-1, self_pod, _lib.ROP_DEREGISTER, flags=_lib.ROPF_MATCH_TIME, last_used=last_used,
                               load_time=int(e["load_time"]), load_complete_time=int(e["load_complete_time"]))])
        try:
            _, st, ed, _ = kreg.run(op, [key], now, dry=dry)
        except InvalidOps as ex:  # (cannot happen: validated above)
            raise InvalidEvictions(str(ex))
        status[i] = st[0]
        for x in ed:
            edits.append((int(idx[i]), i) + tuple(int(x[f]) for f in _lib.REGISTRY_OP_EDIT.names[2:]))
        reload = False
        if attempt:                                                                # :2915
            stats = type_stats[the_type if 0 <= the_type < len(type_stats) else 0]  # :2918 typeSetStats(serviceType)
            tc, tf = int(stats["total_capacity"]), int(stats["total_free"])
            if tc > 0 and int(stats["instance_count"]) > 1 and (20 * tf) // tc >= 1:  # :2919-2920
                reload = True                                                      # :2922 ensureLoadedElsewhere: the caller's
        flags = (_lib.EVO_IN_REGISTRY if in_registry else 0) | (_lib.EVO_ATTEMPT_RELOAD if attempt else 0) | \
            (_lib.EVO_RELOAD if reload else 0) | (_lib.EVO_LOG if log else 0)
        outs[i] = (flags, int(st[0]), -1 if loaded_time is None else loaded_time, millis)
    edits = np.array(edits, dtype=_lib.REGISTRY_OP_EDIT).reshape(-1)
    dereg = ops_array([op_row(-1, self_pod, _lib.ROP_DEREGISTER, flags=_lib.ROPF_MATCH_TIME)] * n) if n else ops_array([])
    info = dict(n_in_registry=int((outs["flags"] & _lib.EVO_IN_REGISTRY != 0).sum()),
                n_attempt_reload=int((outs["flags"] & _lib.EVO_ATTEMPT_RELOAD != 0).sum()),
                n_reload=int((outs["flags"] & _lib.EVO_RELOAD != 0).sum()), n_log=int((outs["flags"] & _lib.EVO_LOG != 0).sum()),
                n_no_record=int((status == _lib.ROP_NO_RECORD).sum()), ops=rk.info_k(dereg, status, [tuple(x) for x in edits]))
    return idx, outs, status, edits, info
