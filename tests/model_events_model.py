"""mmp_model_ids_load / mmp_model_ids_resolve / mmp_model_ids_get / mmp_models_events_json as a plain sequential program: a dict
from id bytes to registry row, the rows parsed with json.loads (tests/ingest_model.py states the bean), the events applied one
after the other.  The oracle of the device path (tests/test_model_ids_gpu.py, tests/test_model_events_gpu.py).

  id space     ids are raw bytes — any UTF-8, the empty key included; nothing orders them.  An id gets its row when it first
               arrives and never leaves: a deleted record is the EMPTY row, still named, and a re-registered id gets it back
  an event     unknown id: status 2, or — a NON-DELETED event with `append` — the id joins first as the next row (EMPTY), whether
               or not its value turns out well-formed, and the event goes on as for a known id.  deleted: the row becomes EMPTY
               (status 0, lul 0).  A malformed value: status 1, the row as it was.  Else the row is the parsed value (status 0)
  a record     (type, last_used, loaded, failed): loaded / failed are tuples of (pod, time) in document order, pod -1 for an
               instance id the pod list does not hold
"""
import numpy as np

from tests.ingest_model import model_bean

APPLIED, MALFORMED, UNKNOWN = 0, 1, 2
EMPTY = (0, 0, (), ())


def _b(s):
    return s if isinstance(s, bytes) else s.encode()


class ModelEventsModel:
    def __init__(self, pod_ids=(), type_names=(), unknown_type=0):
        self.pod_of = {s: i for i, s in enumerate(pod_ids)}
        self.type_names, self.unknown_type = list(type_names), unknown_type
        self.ids = None  # row -> id bytes; None before the first load
        self.index = {}
        self.recs = []   # the registry, row by row

    @property
    def n_models(self):
        return len(self.recs)

    def load(self, ids):
        """Names the rows the registry has; ValueError with nothing changed for a repeated id, RuntimeError for a wrong count."""
        ids = [_b(s) for s in ids]
        if len(ids) != len(self.recs):
            raise RuntimeError("%d ids for %d rows" % (len(ids), len(self.recs)))
        if len(set(ids)) != len(ids):
            raise ValueError("duplicate id")
        self.ids, self.index = ids, {s: i for i, s in enumerate(ids)}

    def resolve(self, keys):
        if self.ids is None:
            raise RuntimeError("no ids loaded")
        return np.array([self.index.get(_b(k), -1) for k in keys], np.int32).reshape(len(keys))

    def get(self, first_row=0, n_rows=None):
        return list(self.ids[first_row:] if n_rows is None else self.ids[first_row:first_row + n_rows])

    def events(self, keys, values, deleted=None, append=True):
        """-> (status[n], model_idx[n], last_unload[n], n_appended), the events applied in order."""
        if self.ids is None:
            raise RuntimeError("no ids loaded")
        n = len(keys)
        status, idx, lul = np.zeros(n, np.int32), np.full(n, -1, np.int32), np.zeros(n, np.int64)
        n_appended = 0
        for i in range(n):
            key, gone = _b(keys[i]), bool(deleted is not None and deleted[i])
            if key not in self.index:
                if gone or not append:
                    status[i] = UNKNOWN
                    continue
                self.index[key] = len(self.ids)  # whether or not the value turns out well-formed
                self.ids.append(key)
                self.recs.append(EMPTY)
                n_appended += 1
            r = idx[i] = self.index[key]
            if gone:
                self.recs[r] = EMPTY
                continue
            v = values[i]
            bean = model_bean(v.decode() if isinstance(v, bytes) else v, self.pod_of, self.type_names, self.unknown_type)
            if bean.status:
                status[i] = MALFORMED
                continue
            self.recs[r] = (bean.type, bean.lu, tuple(bean.loaded), tuple(bean.failed))
            lul[i] = bean.lul
        return status, idx, lul, n_appended
