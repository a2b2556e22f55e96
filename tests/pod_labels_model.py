"""The `labels` of a stored InstanceRecord and the label state of the context as a plain sequential program: a list of names, a
dict from pod to (word, count), the events applied one after the other on top of tests/pod_events_model.PodEventsModel.  The
oracle of ingest_pod_labels_kernel and of mmp_label_names_load / mmp_pod_labels_set / mmp_pod_labels_get
(tests/test_pod_labels_gpu.py, tests/test_pod_labels_types_gpu.py).

  names         name i owns bit i of a label word; at most 64, no two equal, none holding '"', '\\' or a byte below 0x20.  A
                load clears every (word, count); no names = no table: `labels` is a skipped field again.
  labels        InstanceRecord.java:68-92: null, absent and [] are NO_LABELS.  EVERY occurrence must be null or an array of
                strings (else the value is rejected); the LAST one decides.  word = the bits of the elements that equal a name
                byte for byte as they stand between the quotes — an element holding a backslash equals none —, count = the
                number of elements, unknown and repeated ones included.
  an event      status, row, pod index, start time: PodEventsModel, with a value whose labels are rejected counting as
                malformed.  An applied non-deleted event sets (word, count) of its pod; a deleted one leaves them.
  state         ids load: all cleared (a new index space); append / join: new pods carry (0, 0); rows load: the pods that remain
                keep theirs; set: by index, all or nothing.

UNSPECIFIED (ValueError, no corpus may hold one): what tests/ingest_model.py names, a backslash escape in the field name
`labels`, and a raw control byte inside a label string.
"""
import functools

import numpy as np

from modelmesh_amd._lib import POD_LIVE, POD_ROW, POD_SHUTTING_DOWN, POD_TOMBSTONE
from tests.ingest_model import POD_FIELDS, REJECT, UNSPECIFIED, Pairs, _classify, _loads, _raw, _refused
from tests.pod_events_model import APPLIED, MALFORMED, UNKNOWN, PodEventsModel, _b

MAX_LABELS = 64
_ESC = "\ue000"  # what ingest_model._raw leaves where a backslash stood
_WITH_LABELS = dict(POD_FIELDS, labels="labels")  # (for _refused alone: `labels` is no skipped field)


def check_names(names):
    """-> the names as bytes; ValueError for a table mmp_label_names_load refuses."""
    names = [_b(s) for s in names]
    if len(names) > MAX_LABELS:
        raise ValueError("more than 64 names")
    if len(set(names)) != len(names):
        raise ValueError("duplicate name")
    for s in names:
        if any(c in (0x22, 0x5C) or c < 0x20 for c in s):
            raise ValueError("a byte that cannot stand raw inside a JSON string")
    return names


@functools.lru_cache(maxsize=None)
def _bean(value, names):
    text = value.decode("utf-8", "surrogateescape")
    try:
        doc = _loads(text)
    except ValueError:
        if _refused(text, _WITH_LABELS if names is not None else POD_FIELDS) == UNSPECIFIED:
            raise ValueError("unspecified: %r" % (value[:80],))
        return 1, None, 0, 0
    cls, d = _classify(value, POD_FIELDS)
    if cls == UNSPECIFIED:
        raise ValueError("unspecified: %r" % (value[:80],))
    bad, last = cls == REJECT, []
    if names is not None and isinstance(doc, Pairs):
        for (k, v), (rk, rv) in zip(doc, _loads(_raw(text))):
            if k != "labels":
                continue
            if rk != k:
                raise ValueError("unspecified: an escape in the field name")
            if v is None:
                last = []
            elif type(v) is list and all(isinstance(e, str) for e in v):
                last = rv  # the elements as they stand between the quotes
            else:
                bad = True
    if bad:
        return 1, None, 0, 0
    word = 0
    for e in last:
        raw = e.encode("utf-8", "surrogateescape")
        if _ESC not in e and raw in (names or ()):
            word |= 1 << names.index(raw)
    bean = tuple(d.get(f, False if kind == "bool" else 0) for f, kind in POD_FIELDS.items())
    return 0, bean, word, len(last)


def pod_labels_bean(value, names):
    """-> (status, bean, word, count) of one stored value: bean as tests/ingest_model.pod_bean gives it; names = the loaded label
    names in bit order, None for no table (labels are skipped: word and count 0).  A rejected value is (1, None, 0, 0)."""
    return _bean(_b(value), None if names is None else tuple(_b(s) for s in names))


class PodLabelsModel(PodEventsModel):
    def __init__(self):
        super().__init__()
        self.names = None  # no table
        self.labels = {}   # pod -> (word, count); a pod that is not there carries (0, 0)

    # ---- state ----------------------------------------------------------------------------------------------------------
    def names_load(self, names):
        names = check_names(names)  # a refused table changes nothing
        self.names = tuple(names) if names else None
        self.labels = {}

    def load(self, ids):
        out = super().load(ids)
        self.labels = {}
        return out

    def rows_load(self, rows):
        """mmp_pods_load"""
        self.rows = np.array(rows, POD_ROW)
        self.labels = {p: wc for p, wc in self.labels.items() if p < len(self.rows)}

    def labels_set(self, idx, words, counts):
        if any(not 0 <= int(k) < self.n_pods for k in idx) or any(int(c) < 0 for c in counts):
            raise ValueError("bad index or count")
        for k, w, c in zip(idx, words, counts):
            self.labels[int(k)] = (int(w), int(c))

    def labels_get(self):
        words, counts = np.zeros(self.n_pods, np.uint64), np.zeros(self.n_pods, np.int32)
        for p, (w, c) in self.labels.items():
            words[p], counts[p] = w, c
        return words, counts

    # ---- the two JSON calls -----------------------------------------------------------------------------------------------
    def _apply(self, k, bean, word, count, live):
        lru, n, cap, used, lthreads, linprog, rpm, shutdown, start_time, vers = bean
        flags = (POD_LIVE if live else 0) | (POD_SHUTTING_DOWN if shutdown else 0)
        self.rows[k] = (lru, cap, used, vers, n, lthreads, linprog, rpm, self.rows["id_order"][k], self.rows["replica_set"][k], flags, 0)
        if self.names is not None:
            self.labels[k] = (word, count)
        return start_time

    def ingest(self, values, pod_idx, live=None):
        """mmp_pods_ingest_json -> (status[n], start_time[n], word[n], count[n]); word / count of event i as parsed."""
        n = len(values)
        status, start = np.zeros(n, np.int32), np.zeros(n, np.int64)
        words, counts = np.zeros(n, np.uint64), np.zeros(n, np.int32)
        for i in range(n):
            bad, bean, words[i], counts[i] = _bean(_b(values[i]), self.names)
            status[i] = bad
            if not bad:
                start[i] = self._apply(int(pod_idx[i]), bean, int(words[i]), int(counts[i]), live is None or live[i])
        return status, start, words, counts

    def events(self, keys, values, deleted=None, live=None, append=True):
        """mmp_pods_events_json -> (status[n], pod_idx[n], start_time[n], n_appended, word[n], count[n])."""
        if self.ids is None:
            raise RuntimeError("no ids loaded")
        n = len(keys)
        status, idx, start = np.zeros(n, np.int32), np.full(n, -1, np.int32), np.zeros(n, np.int64)
        words, counts = np.zeros(n, np.uint64), np.zeros(n, np.int32)
        n_appended = 0
        for i in range(n):
            key, gone = _b(keys[i]), bool(deleted is not None and deleted[i])
            if key not in self.index:
                if gone or not append:
                    status[i] = UNKNOWN
                    continue
                self.append([key])  # whether or not the value turns out well-formed; the new pod carries no labels
                n_appended += 1
            k = idx[i] = self.index[key]
            if gone:
                self.rows["flags"][k] = (self.rows["flags"][k] | POD_TOMBSTONE) & ~np.uint32(POD_LIVE)
                continue  # (the labels stay: a tombstoned pod is in no set anyway)
            bad, bean, w, c = _bean(_b(values[i]), self.names)
            if bad:
                status[i] = MALFORMED
                continue
            status[i] = APPLIED
            words[i], counts[i] = w, c
            start[i] = self._apply(k, bean, w, c, live is None or live[i])
        return status, idx, start, n_appended, words, counts
