"""mmp_pod_ids_load / mmp_pod_ids_append / mmp_pods_events_json as a plain sequential program: a dict from id to index, a
list of rows parsed with json.loads (tests/ingest_model.py states the bean), the events applied one after the other.  The
oracle of the device path (tests/test_pod_ids_append_gpu.py, tests/test_pods_events_json_gpu.py).

  index space   ids get indices in the order they arrive; an id never leaves (a gone instance is a tombstoned row)
  id_order      rank of the id among ALL ids under bytes comparison (String.compareTo on ASCII: shorter prefix first)
  replica_set   id[:6] interned in order of first appearance over the index order, -1 when |id| < 7
  a new row     all zero, flags = TOMBSTONE
  an event      deleted: the row gets TOMBSTONE and loses LIVE (status 0); unknown id: status 2, or — a non-deleted event with
                `append` — the id joins FIRST and the event goes on as for a known id; a malformed value: status 1, the row as it
                was; else the row is rewritten from the value (status 0)
"""
import numpy as np

from modelmesh_amd._lib import POD_LIVE, POD_ROW, POD_SHUTTING_DOWN, POD_TOMBSTONE
from tests.ingest_model import pod_bean

APPLIED, MALFORMED, UNKNOWN = 0, 1, 2


def _b(s):
    return s if isinstance(s, bytes) else s.encode()


class PodEventsModel:
    def __init__(self):
        self.ids = None  # index -> id bytes; None before the first load
        self.index = {}
        self.rows = np.zeros(0, POD_ROW)
        self._intern = {}

    @property
    def n_pods(self):
        return len(self.rows)

    def _attributes(self):
        order = sorted(range(len(self.ids)), key=lambda i: self.ids[i])  # bytes compare: bytewise, shorter prefix first
        for rank, i in enumerate(order):
            self.rows["id_order"][i] = rank
        for i, s in enumerate(self.ids):
            self.rows["replica_set"][i] = self._intern.setdefault(s[:6], len(self._intern)) if len(s) >= 7 else -1

    def _tombstones(self, n):
        rows = np.zeros(n, POD_ROW)
        rows["flags"] = POD_TOMBSTONE
        return rows

    def load(self, ids):
        ids = [_b(s) for s in ids]
        if len(set(ids)) != len(ids):
            raise ValueError("duplicate id")
        self.ids, self.index, self._intern = ids, {s: i for i, s in enumerate(ids)}, {}
        keep = min(len(self.rows), len(ids))  # rows the table already had stay (mmp_pod_ids_load resizes, it does not clear)
        self.rows = np.concatenate([self.rows[:keep], self._tombstones(len(ids) - keep)])
        self._attributes()
        return self.rows["id_order"].copy(), self.rows["replica_set"].copy()

    def append(self, ids):
        """-> (id_order, replica_set) of all pods; ValueError with nothing changed for a duplicate, RuntimeError before a load."""
        if self.ids is None:
            raise RuntimeError("no ids loaded")
        ids = [_b(s) for s in ids]
        if len(set(ids)) != len(ids) or any(s in self.index for s in ids):
            raise ValueError("duplicate id")
        for s in ids:
            self.index[s] = len(self.ids)
            self.ids.append(s)
        self.rows = np.concatenate([self.rows, self._tombstones(len(ids))])
        self._attributes()
        return self.rows["id_order"].copy(), self.rows["replica_set"].copy()

    def events(self, keys, values, deleted=None, live=None, append=True):
        """-> (status[n], pod_idx[n], start_time[n], n_appended), the events applied in order."""
        if self.ids is None:
            raise RuntimeError("no ids loaded")
        n = len(keys)
        status, idx, start = np.zeros(n, np.int32), np.full(n, -1, np.int32), np.zeros(n, np.int64)
        n_appended = 0
        for i in range(n):
            key, gone = _b(keys[i]), bool(deleted is not None and deleted[i])
            if key not in self.index:
                if gone or not append:
                    status[i] = UNKNOWN
                    continue
                self.append([key])  # whether or not the value turns out well-formed
                n_appended += 1
            k = idx[i] = self.index[key]
            if gone:
                self.rows["flags"][k] = (self.rows["flags"][k] | POD_TOMBSTONE) & ~np.uint32(POD_LIVE)
                continue
            bad, bean = pod_bean(values[i])
            if bad:
                status[i] = MALFORMED
                continue
            lru, count, cap, used, lthreads, linprog, rpm, shutdown, start_time, vers = bean
            flags = (POD_LIVE if live is None or live[i] else 0) | (POD_SHUTTING_DOWN if shutdown else 0)
            self.rows[k] = (lru, cap, used, vers, count, lthreads, linprog, rpm, self.rows["id_order"][k], self.rows["replica_set"][k],
                            flags, 0)
            start[i] = start_time
        return status, idx, start, n_appended
