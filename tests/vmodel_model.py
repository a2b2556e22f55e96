"""The vmodel table in plain, sequential Python: the oracle of mmp_vmodels_events_json / _resolve / _transitions
(modelmesh_amd/csrc/vmodel_kernels.hpp).  Every step cites the Java it stands for (VModelManager.java = VMM, VModelRecord.java).

State: a dict from id bytes to row number and, per row, a Row (None = ABSENT: never set, or deleted).  A Row holds the three
strings as their RAW bytes between the quotes (None = the member is absent or null) — Jackson would decode escapes; a row with a
backslash in one of them is flagged HOST and every question about it is answered "the host decides".

A stored value is read with json.loads under the type rules of VModelRecord.java:28-41 (o, amid, tmid: String; failed: boolean)
with a member walk of its own (object_pairs_hook), so that a duplicate member's last occurrence wins and an earlier occurrence is
still held to its type.  The classes ACCEPT / REJECT / UNSPECIFIED are those of tests/ingest_model.py; what is UNSPECIFIED there
(invalid only inside a skipped value, leading zeros, an escape in the NAME of a known member) stays unspecified here.

The registry is what the questions look models up in: ids in row order and per row (n_loaded, n_failed, last_used, type); the
empty row (what a deletion leaves) is all zero."""
import functools
import json
from collections import namedtuple

import numpy as np

from tests.ingest_model import ACCEPT, REJECT, UNSPECIFIED, Pairs, _loads, _raw, _refused

FIELDS = {"amid": "str", "tmid": "str", "o": "str", "failed": "bool"}
Row = namedtuple("Row", "amid tmid owner failed host")

# include/mmplace.h
F_FAILED, F_ABSENT, F_ACTIVE_NULL, F_TARGET_NULL, F_OWNER_NULL, F_HOST = 1, 2, 4, 8, 16, 32
NOT_FOUND, OK, STRONG_READ, TARGET_NOT_FOUND, HOST = range(5)
ACTIVE, TARGET = 0, 1
NULL_ID = 1
DEFINED, TRANSITIONING, TRANSITION_FAILED = range(3)
T_NONE, T_LOADING, T_LOADING_FAILED, T_NOT_FOUND = range(4)
PROMOTE, ENSURE_LOADED = 0, 1
XF_FAILED, XF_FROM_EMPTY, XF_TO_EMPTY = 1, 2, 4
Answer = namedtuple("Answer", "cls which vmodel model target_model vstatus target_status flags")
Transition = namedtuple("Transition", "vmodel from_model to_model target_count cls flags last_used")
I64_MASK = (1 << 64) - 1


def _unraw(s):
    """A string of the _raw document back to the bytes that stood between the quotes."""
    return s.replace("\ue000", "\\").replace("\ue001", '"').replace("\ue002", "\\").encode("utf-8", "surrogateescape")


@functools.lru_cache(maxsize=None)
def classify(value):
    """-> (class, Row or None).  (Cached: the large batches draw their values from a small corpus.)"""
    text = value.decode("utf-8", "surrogateescape") if isinstance(value, bytes) else value
    try:
        doc = _loads(text)
    except ValueError:
        return _refused(text, FIELDS), None
    if not isinstance(doc, Pairs):
        return REJECT, None
    raw = _loads(_raw(text))
    verdicts, last = set(), {"amid": None, "tmid": None, "o": None, "failed": False}
    for (k, v), (rk, rv) in zip(doc, raw):  # the member walk: every occurrence is held to its type, the last one wins
        kind = FIELDS.get(k)
        if kind is None:
            continue  # JsonExtensible: anything else is skipped
        if rk != k:
            verdicts.add(UNSPECIFIED)  # an escape in the name: the parsers hash raw bytes
        if kind == "bool":
            if not isinstance(v, bool):
                verdicts.add(REJECT)
            last[k] = v
        elif v is None:
            last[k] = None  # a later null wins over an earlier string
        elif isinstance(v, str):
            last[k] = _unraw(rv)
        else:
            verdicts.add(REJECT)
    if REJECT in verdicts:
        return REJECT, None
    if UNSPECIFIED in verdicts:
        return UNSPECIFIED, None
    host = any(b is not None and b"\\" in b for b in (last["amid"], last["tmid"], last["o"]))
    return ACCEPT, Row(last["amid"], last["tmid"], last["o"], last["failed"], host)


def parse(value):
    """-> (status, Row): 0 with the row, 1 (malformed) with None.  Raises ValueError for the UNSPECIFIED class."""
    cls, row = classify(value)
    if cls == UNSPECIFIED:
        raise ValueError("unspecified: %r" % (value[:80],))
    return (0, row) if cls == ACCEPT else (1, None)


def row_flags(r):
    if r is None:
        return F_ABSENT | F_ACTIVE_NULL | F_TARGET_NULL | F_OWNER_NULL
    return ((F_FAILED if r.failed else 0) | (F_ACTIVE_NULL if r.amid is None else 0) | (F_TARGET_NULL if r.tmid is None else 0) |
            (F_OWNER_NULL if r.owner is None else 0) | (F_HOST if r.host else 0))


def in_transition(r):
    """VModelRecord.inTransition(): !Objects.equals(activeModel, targetModel)."""
    return r.amid != r.tmid


class Registry:
    """ids[i] = the id of registry row i; recs[i] = (n_loaded, n_failed, last_used, type)."""

    def __init__(self, ids, recs):
        self.ids, self.recs = list(ids), [tuple(int(x) for x in r) for r in recs]
        self.row_of = {b: i for i, b in enumerate(self.ids)}

    def row(self, mid):
        return -1 if mid is None else self.row_of.get(mid, -1)

    def empty(self, i):
        return self.recs[i] == (0, 0, 0, 0)


class VModels:
    def __init__(self):
        self.ids, self.row_of, self.rows = [], {}, []

    def _key(self, k):
        return k if isinstance(k, bytes) else k.encode()

    def events(self, keys, values, deleted=None, append=True):
        """The listener's events one by one -> (status, vmodel_idx, n_appended)."""
        n = len(keys)
        status, idx, n_app = np.zeros(n, np.int32), np.full(n, -1, np.int32), 0
        for i in range(n):
            k, dele = self._key(keys[i]), bool(deleted is not None and deleted[i])
            if k not in self.row_of:
                if dele or not append:  # a deletion never appends
                    status[i] = 2
                    continue
                self.row_of[k] = len(self.ids)  # joins whether or not its value turns out well-formed
                self.ids.append(k)
                self.rows.append(None)
                n_app += 1
            v = idx[i] = self.row_of[k]
            if dele:
                self.rows[v] = None  # keeps its id and number
                continue
            status[i], row = parse(values[i])
            if status[i] == 0:
                self.rows[v] = row
        return status, idx, n_app

    def flags(self):
        return np.array([row_flags(r) for r in self.rows], np.uint32)

    def strings(self):
        return [(None, None, None) if r is None else (r.amid, r.tmid, r.owner) for r in self.rows]

    def info(self):
        live = [r for r in self.rows if r is not None]
        return len(self.rows), len(live), sum(len(s) for r in live for s in r[:3] if s is not None)

    # ---- resolveVModelId, VMM:569-597; absentOrOwnerMismatch :530-532; statusFromRecord :552-559;
    # ---- resolveTargetModelStatusInfo :537-549
    def resolve(self, reg, key, nf=None, owner=None, after_strong=False):
        nf, owner = nf or None, owner or None  # emptyToNull (:506)
        if nf is not None:
            nf = self._key(nf)
        if owner is not None:
            owner = self._key(owner)
        v = self.row_of.get(self._key(key), -1)
        r = self.rows[v] if v >= 0 else None
        none = Answer(NOT_FOUND, 0, -1, -1, -1, 0, 0, 0)
        if r is None:
            return none  # :570-573 vmr == null
        if r.host:
            return none._replace(cls=HOST, vmodel=v)
        if owner is not None and r.owner != owner:
            return none  # :531 owner != null && !Objects.equals(vmr.getOwner(), owner)
        which = None
        if nf is None or nf != r.amid:  # :575 (and :587 after the strong read: the same comparison on the fresh record)
            cls, which = OK, ACTIVE
        elif not after_strong:
            cls = STRONG_READ  # :582 vModels.getStrong
        elif nf != r.tmid:  # :590-592
            cls, which = OK, TARGET
        else:
            cls = TARGET_NOT_FOUND  # :594-596
        target_model = reg.row(r.tmid)
        model, flags = -1, 0
        if which is not None:
            mid = r.amid if which == ACTIVE else r.tmid
            model = reg.row(mid)
            flags = NULL_ID if mid is None else 0
        vstatus, tstatus = DEFINED, T_NONE
        if in_transition(r):  # :555-556
            vstatus = TRANSITION_FAILED if r.failed else TRANSITIONING
            if target_model < 0 or reg.empty(target_model):
                tstatus = T_NOT_FOUND  # :548 targetModel == null (the Java dereferences it first at :544 when `failed`)
            else:
                nl, nfail = reg.recs[target_model][:2]
                tstatus = T_LOADING_FAILED if r.failed and nfail > 0 and nl == 0 else T_LOADING  # :544-546
        return Answer(cls, which or 0, v, model, target_model, vstatus, tstatus, flags)

    def resolve_many(self, reg, keys, nf=None, owners=None, req_flags=None):
        n = len(keys)
        return [self.resolve(reg, keys[i], None if nf is None else nf[i], None if owners is None else owners[i],
                             bool(req_flags is not None and req_flags[i] & 1)) for i in range(n)]

    # ---- processVModels :617-634, processVModel :639-643, PendingTransition.run :701-708
    def transitions(self, reg, now_ms, age_ms):
        """-> (rows, info): info = (n_listed, n_promote, n_ensure_loaded, n_host_skipped)."""
        out, n_host = [], 0
        for v, r in enumerate(self.rows):  # :627 for (Entry<String, VModelRecord> ent : vModels)
            if r is None:
                continue  # :641 vmr == null
            if r.host:
                n_host += 1
                continue
            if not in_transition(r):
                continue  # :641
            frm, to = reg.row(r.amid), reg.row(r.tmid)
            flags = XF_FAILED if r.failed else 0
            target_count, cls, last_used = 0, PROMOTE, 0
            if frm >= 0:
                nl, _, lu, _ = reg.recs[frm]
                flags |= XF_FROM_EMPTY if reg.empty(frm) else 0
                target_count = nl  # :702 curActive.getInstanceIds().size()
                if nl > 0:  # :703
                    cls = ENSURE_LOADED
                    last_used = lu if lu != 0 else java_long(now_ms - age_ms)  # :705-708
            if to >= 0 and reg.empty(to):
                flags |= XF_TO_EMPTY
            out.append(Transition(v, frm, to, target_count, cls, flags, last_used))
        n_p = sum(t.cls == PROMOTE for t in out)
        return out, (len(out), n_p, len(out) - n_p, n_host)


def java_long(x):
    x &= I64_MASK
    return x - (1 << 64) if x >> 63 else x


def transitions_numpy(listed, amid_row, tmid_row, failed, n_loaded, last_used, empty, now_ms, age_ms):
    """The transition scan vectorised: per vmodel row — listed (not ABSENT, not HOST, in transition), the registry rows of amid /
    tmid (-1), failed; per registry row — n_loaded, last_used, empty.  -> a structured array in the layout of mmp_vmodel_transition."""
    from modelmesh_amd import _lib
    v = np.nonzero(listed)[0]
    frm, to = amid_row[v], tmid_row[v]
    out = np.zeros(len(v), _lib.VMODEL_TRANSITION)
    out["vmodel"], out["from_model"], out["to_model"] = v, frm, to
    has = frm >= 0
    f = np.where(has, frm, 0)
    tc = np.where(has, n_loaded[f], 0)
    out["target_count"] = tc
    out["cls"] = np.where(tc > 0, ENSURE_LOADED, PROMOTE)
    fallback = np.array(now_ms, np.int64) - np.array(age_ms, np.int64)  # int64 arithmetic wraps as Java's does
    lu = last_used[f]
    out["last_used"] = np.where(tc > 0, np.where(lu != 0, lu, fallback), 0)
    t = np.where(to >= 0, to, 0)
    out["flags"] = (np.where(failed[v], XF_FAILED, 0) | np.where(has & empty[f], XF_FROM_EMPTY, 0) |
                    np.where((to >= 0) & empty[t], XF_TO_EMPTY, 0))
    return out


def render(amid, tmid, owner=None, failed=False, extra=""):
    """A stored value as Jackson writes it (defaults omitted): strings given as str are JSON-escaped."""
    d = {}
    if owner is not None:
        d["o"] = owner
    if amid is not None:
        d["amid"] = amid
    if tmid is not None:
        d["tmid"] = tmid
    if failed:
        d["failed"] = True
    s = json.dumps(d, ensure_ascii=False, separators=(",", ":"))
    return s if not extra else (s[:-1] + ("," if d else "") + extra + "}")
