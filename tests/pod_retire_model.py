"""mmp_pods_retire as a plain sequential program over a PodEventsModel (tests/pod_events_model.py) and the state kept beside it
by instance index, all of it plain lists.  The oracle of the device path (tests/test_pods_retire_gpu.py).

  pods          instance indices in [0, P0) in any order; an index named twice is retired once
  remap         int32[P0]: the new index of every old index, -1 for a retired one; survivors keep their order and move down
  ids           the named ids are deleted from the dict and the list; id_order is recomputed — the rank among the SURVIVING ids
                under bytes comparison; the replica-set interning is kept: a survivor keeps its number, and so does a prefix that
                comes back.  Without ids (a table loaded by rows) the rows are squeezed and keep the id_order they carry
  labels, types one word / count per instance, one bit per instance and type: the retired instances' elements are squeezed out
  missing       the `missings` marks of the first len(missing) instances: squeezed the same way
  records       per registry record a list of loaded and a list of failed entries [pod, time]: an entry naming a survivor gets the
                new index, one naming a retired instance becomes -1 (unresolved) where it stands, anything outside [0, P0) stays
  count         the entries turned into -1
  gone_only     every named row must be a tombstone (TOMBSTONE set, LIVE clear)
  unreferenced  no record may name a retired instance, loaded or failed
  refusals      ValueError (MMP_EINVAL) with nothing changed: an index outside [0, P0), either guard — the message names the lowest
                offender.  RuntimeError (MMP_ESTATE): ids are loaded and their count is not the table's
"""
import numpy as np

from modelmesh_amd._lib import POD_LIVE, POD_TOMBSTONE
from tests.pod_events_model import PodEventsModel


class PodRetireState:
    def __init__(self, pods=None):
        self.pods = pods if pods is not None else PodEventsModel()
        self.label_words, self.label_counts = [], []  # per instance (shorter than P: the rest carry none)
        self.allowed, self.prefer = [], []  # per type: a list of P bits
        self.missing = []  # first-seen-missing time of the first len(missing) instances, 0 = no mark
        self.records = []  # per record: (loaded, failed), each a list of [pod, time]

    def entries(self):
        return [e for loaded, failed in self.records for e in loaded + failed]

    def n_unresolved(self):
        p = self.pods.n_pods
        return sum(1 for e in self.entries() if e[0] < 0 or e[0] >= p)


def retire(state, pods, gone_only=False, unreferenced=False):
    """-> (remap, n_entries_unresolved)"""
    m = state.pods
    p0 = m.n_pods
    if m.ids is not None and len(m.ids) != p0:
        raise RuntimeError("%d ids for %d rows" % (len(m.ids), p0))
    pods = [int(p) for p in pods]
    for p in pods:
        if p < 0 or p >= p0:
            raise ValueError("instance %d of %d" % (p, p0))
    gone = set(pods)
    if gone_only:
        alive = sorted(p for p in gone if (m.rows["flags"][p] & POD_LIVE) or not (m.rows["flags"][p] & POD_TOMBSTONE))
        if alive:
            raise ValueError("instance %d is not a tombstone" % alive[0])
    if unreferenced:
        named = sorted(e[0] for e in state.entries() if e[0] in gone)
        if named:
            raise ValueError("instance %d is still named" % named[0])
    remap = np.full(p0, -1, np.int32)
    keep = [p for p in range(p0) if p not in gone]
    remap[keep] = np.arange(len(keep), dtype=np.int32)
    if not gone:
        return remap, 0
    m.rows = m.rows[keep].copy()
    if m.ids is not None:
        m.ids = [m.ids[p] for p in keep]
        m.index = {s: i for i, s in enumerate(m.ids)}
        m._attributes()  # the ranks of the survivors; _intern is kept, so every replica_set stays
    squeeze = lambda xs: [xs[p] for p in keep if p < len(xs)]  # noqa: E731
    state.label_words, state.label_counts = squeeze(state.label_words), squeeze(state.label_counts)
    state.allowed, state.prefer = [squeeze(r) for r in state.allowed], [squeeze(r) for r in state.prefer]
    state.missing = squeeze(state.missing)
    count = 0
    for loaded, failed in state.records:
        for e in loaded + failed:
            if 0 <= e[0] < p0:
                e[0] = int(remap[e[0]])
                count += e[0] < 0
    return remap, int(count)
