"""Thin Python veneer over the libmmplace C ABI (used by tests and bench.py).

Names follow the reference's domain: an *instance table* of pods
(InstanceRecord), a *registry* of models (ModelRecord), load-target decisions
(CacheMissForwardingLB.getNext, MM.java:4776), serve-target decisions
(ForwardingLB.getNext, MM.java:4315) and cache eviction (clhm).
Everything is computed by the HIP kernels behind the C ABI; nothing here
implements placement logic.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from . import _lib
from ._lib import (EVICT_OUT, EVICT_REQ, MODEL_ROW, PLACE_OUT, PLACE_REQ, POD_ROW, SERVE_COUNTER, SERVE_OUT,
                   SERVE_REQ, STATS, MmpConfig, ptr)


class MmpError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libmmplace error {code}: {msg}")
        self.code = code


@dataclass
class Fleet:
    """One consistent view of clusterState + registry + typeConstraints."""
    pods: np.ndarray                      # POD_ROW[P]
    models: np.ndarray                    # MODEL_ROW[M]
    ent_pod: np.ndarray                   # int32: loaded ids then failed ids per model
    ent_time: np.ndarray                  # int64: load start / failure time per entry
    min_space_units: int
    min_churn_age_ms: int
    now: int
    n_types: int = 0                      # 0 == typeConstraints is null
    allowed: Optional[np.ndarray] = None  # uint64 [T][W] bit p = pod p allowed
    prefer: Optional[np.ndarray] = None
    has_allowed: Optional[np.ndarray] = None  # uint8 [T]
    has_prefer: Optional[np.ndarray] = None
    replaced_rs: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))

    @property
    def n_pods(self) -> int:
        return int(self.pods.shape[0])

    @property
    def n_models(self) -> int:
        return int(self.models.shape[0])


def bitmap_from_bool(mask: np.ndarray) -> np.ndarray:
    """bool [T][P] -> uint64 [T][ceil(P/64)], bit p%64 of word p//64."""
    mask = np.atleast_2d(mask).astype(bool)
    t, p = mask.shape
    w = (p + 63) // 64
    padded = np.zeros((t, w * 64), dtype=np.uint8)
    padded[:, :p] = mask
    by = np.packbits(padded.reshape(t, w, 8, 8), axis=-1, bitorder="little").reshape(t, w, 8)
    return np.ascontiguousarray(by).view("<u8").reshape(t, w)


class Solver:
    def __init__(self, min_space_units: int, min_churn_age_ms: int, device: int = 0):
        self.lib = _lib.load()
        cfg = MmpConfig(device, 0, int(min_space_units), int(min_churn_age_ms))
        h = C.c_void_p()
        rc = self.lib.mmp_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise MmpError(rc, (self.lib.mmp_last_error(None) or b"").decode())
        self.h = h
        self.n_pods = 0

    def close(self):
        if getattr(self, "h", None):
            self.lib.mmp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc: int):
        if rc != 0:
            raise MmpError(rc, (self.lib.mmp_last_error(self.h) or b"").decode())

    # ---- snapshot ------------------------------------------------------
    def load_pods(self, pods: np.ndarray):
        pods = np.ascontiguousarray(pods, dtype=POD_ROW)
        self._ck(self.lib.mmp_pods_load(self.h, ptr(pods), len(pods)))
        self.n_pods = len(pods)
        self._live = (pods["flags"] & 2) != 0  # host mirror for serve_counters (what litelinks' instance list would hold)

    def upsert_pods(self, idx: np.ndarray, rows: np.ndarray):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        rows = np.ascontiguousarray(rows, dtype=POD_ROW)
        self._ck(self.lib.mmp_pods_upsert(self.h, ptr(idx), ptr(rows), len(idx)))
        self.n_pods = max(self.n_pods, int(idx.max()) + 1 if len(idx) else 0)
        if len(idx):
            live = getattr(self, "_live", np.zeros(0, bool))
            if self.n_pods > len(live):
                live = np.concatenate([live, np.zeros(self.n_pods - len(live), bool)])
            live[idx] = (rows["flags"] & 2) != 0
            self._live = live

    def remove_pods(self, idx: np.ndarray):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        self._ck(self.lib.mmp_pods_remove(self.h, ptr(idx), len(idx)))
        live = getattr(self, "_live", None)
        if live is not None and len(idx):
            live[idx[(idx >= 0) & (idx < len(live))]] = False  # a removed row leaves litelinks' list too

    def load_types(self, n_types, allowed=None, prefer=None, has_allowed=None, has_prefer=None):
        def u64(a):
            return None if a is None else np.ascontiguousarray(a, dtype=np.uint64)

        def u8(a):
            return None if a is None else np.ascontiguousarray(a, dtype=np.uint8)
        allowed, prefer, has_allowed, has_prefer = u64(allowed), u64(prefer), u8(has_allowed), u8(has_prefer)
        self._ck(self.lib.mmp_types_load(self.h, int(n_types), ptr(allowed), ptr(prefer),
                                         ptr(has_allowed), ptr(has_prefer)))

    def types_from_labels(self, required, preferred, pod_labels):
        """a18: returns (allowed[T+1][W], prefer[T+1][W], has_allowed[T+1], has_prefer[T+1]) and installs them."""
        required = np.ascontiguousarray(required, dtype=np.uint64)
        preferred = np.ascontiguousarray(preferred, dtype=np.uint64)
        pod_labels = np.ascontiguousarray(pod_labels, dtype=np.uint64)
        T, W = len(required), (self.n_pods + 63) // 64
        al = np.zeros((T + 1, max(W, 1)), np.uint64)
        pf = np.zeros((T + 1, max(W, 1)), np.uint64)
        ha = np.zeros(T + 1, np.uint8)
        hp = np.zeros(T + 1, np.uint8)
        self._ck(self.lib.mmp_types_from_labels(self.h, T, ptr(required) if T else None, ptr(preferred) if T else None,
                                                ptr(pod_labels) if len(pod_labels) else None, ptr(al), ptr(pf),
                                                ptr(ha), ptr(hp)))
        return al[:, :W], pf[:, :W], ha, hp

    def load_replaced_rs(self, rs):
        rs = np.ascontiguousarray(rs, dtype=np.int32)
        self._ck(self.lib.mmp_replaced_rs_load(self.h, ptr(rs) if len(rs) else None, len(rs)))

    # ---- KV wire format ------------------------------------------------------
    @staticmethod
    def _pack(strings):
        bs = [x if isinstance(x, bytes) else x.encode() for x in strings]
        off = np.zeros(len(bs) + 1, np.int64)
        np.cumsum([len(b) for b in bs], out=off[1:])
        return b"".join(bs), off

    def load_pod_ids(self, ids):
        """ids: instance id strings in pod-index order; returns (id_order, replica_set)."""
        blob, off = self._pack(ids)
        off32 = off.astype(np.int32)
        n = len(ids)
        io = np.zeros(max(n, 1), np.uint32)
        rs = np.zeros(max(n, 1), np.int32)
        self._ck(self.lib.mmp_pod_ids_load(self.h, blob, ptr(off32), n, ptr(io), ptr(rs)))
        self.n_pods = n
        return io[:n], rs[:n]

    def ingest_pods_json(self, values, pod_idx, live=None):
        """values: InstanceRecord JSON (bytes/str) per record; returns (status, start_time)."""
        blob, off = self._pack(values)
        n = len(values)
        pod_idx = np.ascontiguousarray(pod_idx, dtype=np.int32)
        live = None if live is None else np.ascontiguousarray(live, dtype=np.uint8)
        st = np.zeros(max(n, 1), np.int64)
        status = np.zeros(max(n, 1), np.int32)
        self._ck(self.lib.mmp_pods_ingest_json(self.h, blob, ptr(off), n, ptr(pod_idx), ptr(live), ptr(st), ptr(status)))
        # the host mirror serve_counters reads (what litelinks' instance list would hold): the ingested rows' live flags
        mirror = getattr(self, "_live", None)
        if mirror is not None and n:
            top = int(pod_idx.max()) + 1
            if top > len(mirror):
                mirror = np.concatenate([mirror, np.zeros(top - len(mirror), bool)])
            ok = status[:n] == 0
            mirror[pod_idx[ok]] = True if live is None else live[ok].astype(bool)
            self._live = mirror
        return status[:n], st[:n]

    def append_pod_ids(self, ids):
        """New instances join the index space (mmp_pod_ids_append): ids get the indices n_pods .. n_pods + len(ids) - 1; returns
        (id_order, replica_set) of ALL pods."""
        blob, off = self._pack(ids)
        off32 = off.astype(np.int32)
        total = self.n_pods + len(ids)
        io = np.zeros(max(total, 1), np.uint32)
        rs = np.zeros(max(total, 1), np.int32)
        self._ck(self.lib.mmp_pod_ids_append(self.h, blob, ptr(off32), len(ids), ptr(io), ptr(rs), total))
        self._grow_live(total)
        self.n_pods = total
        return io[:total], rs[:total]

    def _grow_live(self, n):
        """the host mirror serve_counters reads covers n pods (new slots: not live)"""
        mirror = getattr(self, "_live", None)
        if mirror is not None and n > len(mirror):
            self._live = np.concatenate([mirror, np.zeros(n - len(mirror), bool)])

    def pods_events_json(self, keys, values, deleted=None, live=None, append=True):
        """Instance-table events by key (mmp_pods_events_json): keys[i] is the instance id, values[i] its InstanceRecord JSON,
        deleted[i] marks a deletion.  Returns (status, pod_idx, start_time, n_appended)."""
        kblob, koff = self._pack(keys)
        koff32 = koff.astype(np.int32)
        blob, off = self._pack(values)
        n = len(keys)
        assert len(values) == n
        deleted = None if deleted is None else np.ascontiguousarray(deleted, dtype=np.uint8)
        live = None if live is None else np.ascontiguousarray(live, dtype=np.uint8)
        st = np.zeros(max(n, 1), np.int64)
        status = np.zeros(max(n, 1), np.int32)
        idx = np.full(max(n, 1), -1, np.int32)
        n_app = C.c_int32(0)
        self._ck(self.lib.mmp_pods_events_json(self.h, kblob, ptr(koff32), blob, ptr(off), n, ptr(deleted), ptr(live),
                                               _lib.PEV_APPEND if append else 0, ptr(idx), ptr(st), ptr(status), C.byref(n_app)))
        self.n_pods += n_app.value
        self._grow_live(self.n_pods)
        mirror = getattr(self, "_live", None)
        if mirror is not None:
            for i in range(n):  # in event order, as the library applies them
                if status[i] != 0:
                    continue
                if deleted is not None and deleted[i]:
                    mirror[idx[i]] = False
                else:
                    mirror[idx[i]] = True if live is None else bool(live[i])
        return status[:n], idx[:n], st[:n], n_app.value

    # ---- instance labels kept in the context ------------------------------------------------------
    def label_names_load(self, names):
        """Label name i owns bit i of a label word (mmp_label_names_load); at most 64 names, [] unloads the table.  While a
        table is loaded the two instance JSON calls read `labels` from the stored value.  Clears every resident word."""
        blob, off = self._pack(names)
        off32 = off.astype(np.int32)
        self._ck(self.lib.mmp_label_names_load(self.h, blob, ptr(off32), len(names)))

    def pod_labels_set(self, idx, words, counts):
        """Word and count of staged pods by index (mmp_pod_labels_set), for hosts that feed rows instead of JSON."""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        words = np.ascontiguousarray(words, dtype=np.uint64)
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        assert len(words) == len(idx) == len(counts)
        self._ck(self.lib.mmp_pod_labels_set(self.h, ptr(idx), ptr(words), ptr(counts), len(idx)))

    def pod_labels_get(self):
        """-> (words[P], counts[P]): the known-label bits and the `labels` element count of every staged pod."""
        n = C.c_int32(0)
        self._ck(self.lib.mmp_pod_labels_get(self.h, None, None, 0, C.byref(n)))
        words, counts = np.zeros(max(n.value, 1), np.uint64), np.zeros(max(n.value, 1), np.int32)
        self._ck(self.lib.mmp_pod_labels_get(self.h, ptr(words), ptr(counts), n.value, C.byref(n)))
        return words[:n.value], counts[:n.value]

    def types_from_pod_labels(self, required, preferred):
        """types_from_labels with the resident label words (mmp_types_from_pod_labels)."""
        required = np.ascontiguousarray(required, dtype=np.uint64)
        preferred = np.ascontiguousarray(preferred, dtype=np.uint64)
        T, W = len(required), (self.n_pods + 63) // 64
        al = np.zeros((T + 1, max(W, 1)), np.uint64)
        pf = np.zeros((T + 1, max(W, 1)), np.uint64)
        ha = np.zeros(T + 1, np.uint8)
        hp = np.zeros(T + 1, np.uint8)
        self._ck(self.lib.mmp_types_from_pod_labels(self.h, T, ptr(required) if T else None, ptr(preferred) if T else None,
                                                    ptr(al), ptr(pf), ptr(ha), ptr(hp)))
        return al[:, :W], pf[:, :W], ha, hp

    def registry_unresolved(self, max_models=None):
        """The registry rows holding an entry whose id the instance table does not know (mmp_registry_unresolved), ascending.
        Returns (rows, n_models, n_entries); max_models=None asks for all of them."""
        nm, ne = C.c_int32(0), C.c_int64(0)
        if max_models is None:
            self._ck(self.lib.mmp_registry_unresolved(self.h, None, 0, C.byref(nm), C.byref(ne)))
            max_models = nm.value
        out = np.full(max(max_models, 1), -1, np.int32)
        self._ck(self.lib.mmp_registry_unresolved(self.h, ptr(out) if max_models else None, int(max_models), C.byref(nm), C.byref(ne)))
        return out[: min(max_models, nm.value)], nm.value, ne.value

    def load_type_names(self, names, unknown_type):
        blob, off = self._pack(names)
        off32 = off.astype(np.int32)
        self._ck(self.lib.mmp_type_names_load(self.h, blob, ptr(off32), len(names), int(unknown_type)))

    def ingest_models_json(self, values):
        """values: ModelRecord JSON per model; returns (status, last_unload_time)."""
        blob, off = self._pack(values)
        n = len(values)
        lul = np.zeros(max(n, 1), np.int64)
        status = np.zeros(max(n, 1), np.int32)
        self._ck(self.lib.mmp_models_ingest_json(self.h, blob, ptr(off), n, ptr(lul), ptr(status)))
        self.n_models = n
        self._models = self._ent_pod = None  # (the registry now lives on the device only: serve_counters needs load_models / upsert_models)
        return status[:n], lul[:n]

    def upsert_models_json(self, values, idx, deleted=None):
        """Registry events as stored: values[i] (ModelRecord JSON, bytes/str) replaces model idx[i]; deleted[i] marks
        ENTRY_DELETED (the value is ignored).  Returns (status, last_unload_time)."""
        blob, off = self._pack(values)
        n = len(values)
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        deleted = None if deleted is None else np.ascontiguousarray(deleted, dtype=np.uint8)
        lul = np.zeros(max(n, 1), np.int64)
        status = np.zeros(max(n, 1), np.int32)
        self._ck(self.lib.mmp_models_upsert_json(self.h, blob, ptr(off), n, ptr(idx), ptr(deleted), ptr(lul), ptr(status)))
        if n:
            self.n_models = max(getattr(self, "n_models", 0), int(idx.max()) + 1)
            self._models = self._ent_pod = None  # (the registry now lives on the device only, as after ingest_models_json)
        return status[:n], lul[:n]

    def models_rewrite_json(self, rows, old_values, last_unload=None, fail=None):
        """The write side of the wire format (mmp_models_rewrite_json): old_values[i] (bytes/str) is the stored value of registry
        row rows[i]; the answer is the value to store next — what the device does not own copied byte for byte, instanceIds /
        failedIn / fails / lu (and lul from last_unload[i], when given) rendered from the resident row.  fail = (fail_pod,
        messages): addLoadFailure / removeLoadFailure of instance fail_pod[i] (-1: none) with messages[i] (bytes/str, empty:
        remove).  Returns (values, status): values[i] is bytes, or None where status[i] is MRW_MALFORMED / MRW_HOST.  Two calls:
        the sizes, then the bytes."""
        total = self.models_rewrite_json_raw(rows, old_values, last_unload, fail, 0)[3]
        out, off, status, total2, rc = self.models_rewrite_json_raw(rows, old_values, last_unload, fail, total)
        self._ck(rc)
        assert total2 == total  # (read-only over a registry nobody edited in between)
        vals = [bytes(out[off[i]:off[i + 1]]) if status[i] == 0 else None for i in range(len(status))]
        return vals, status

    def models_rewrite_json_raw(self, rows, old_values, last_unload, fail, out_cap, fill=0, null_out=False, flags=0, old_off=None,
                                msg_off=None, no_msgs=False):
        """One mmp_models_rewrite_json call with exactly this capacity (null_out: a NULL out_buf), the outputs filled with the
        byte `fill` first: (out bytes as uint8[out_cap], out_off[n + 1], status[n], total, rc).  Raises on rc only through the
        caller: rc is returned (total is -1 where the library did not set it).  old_off / msg_off: these offsets instead of the packed
        ones; no_msgs: fail_pod without the two message arrays."""
        blob, off = self._pack(old_values)
        n = len(old_values)
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        lul = None if last_unload is None else np.ascontiguousarray(last_unload, dtype=np.int64)
        fpod = fmsg = fmoff = None
        if fail is not None:
            fpod = np.ascontiguousarray(fail[0], dtype=np.int32)
            fmsg, fmoff64 = self._pack(fail[1])
            fmoff = fmoff64.astype(np.int32) if msg_off is None else np.ascontiguousarray(msg_off, dtype=np.int32)
            if no_msgs:
                fmsg = fmoff = None
        if old_off is not None:
            off = np.ascontiguousarray(old_off, dtype=np.int64)
        out = np.zeros(max(int(out_cap), 1), np.uint8)
        out_off = np.zeros(n + 1, np.int64)
        status = np.zeros(max(n, 1), np.int32)
        for a in (out, out_off, status):
            a.view(np.uint8)[:] = fill
        total = C.c_int64(-1)
        rc = self.lib.mmp_models_rewrite_json(self.h, ptr(rows), n, blob, ptr(off), ptr(lul), ptr(fpod), fmsg, ptr(fmoff), flags,
                                              None if null_out else ptr(out), int(out_cap), ptr(out_off), ptr(status),
                                              C.byref(total))
        return out[:int(out_cap)], out_off, status[:n], total.value, rc

    def models_register_json(self, reqs, infos, old_values, now_ms, lastused_age_on_add_ms, keys=None):
        """registerModel / deleteModel as a batch of questions (mmp_models_register_json): reqs is a REGISTER_REQ array, infos[i] =
        (type, encKey, mPath) as bytes/str with "" or None for null, old_values[i] the stored value (empty: registry.get() == null),
        keys the model ids (None: no rows are asked for).  Returns (values, classes, last_used, rows): values[i] is bytes where
        classes[i] is MREG_CREATED / MREG_TOUCHED and None elsewhere, rows is None without keys.  Two calls: the sizes, then the
        bytes."""
        args = (reqs, infos, old_values, now_ms, lastused_age_on_add_ms, keys)
        r = self.models_register_json_raw(*args, 0)
        self._ck(r[6])
        out, off, cls, lu, rows, total, rc = self.models_register_json_raw(*args, r[5])
        self._ck(rc)
        assert total == r[5]  # (a pure function of the arguments, and of the id table for the rows)
        rendered = (_lib.MREG_CREATED, _lib.MREG_TOUCHED)
        vals = [bytes(out[off[i]:off[i + 1]]) if cls[i] in rendered else None for i in range(len(cls))]
        return vals, cls, lu, rows

    def models_register_json_raw(self, reqs, infos, old_values, now_ms, lastused_age_on_add_ms, keys, out_cap, fill=0, null_out=False,
                                 flags=0, old_off=None, info_off=None, key_off=None):
        """One mmp_models_register_json call with exactly this capacity (null_out: a NULL out_buf), the outputs filled with the byte
        `fill` first: (out bytes as uint8[out_cap], out_off[n + 1], classes[n], last_used[n], rows[n] or None, total, rc); total is
        -1 where the library did not set it.  old_off / info_off / key_off: these offsets instead of the packed ones."""
        reqs = np.ascontiguousarray(reqs, dtype=_lib.REGISTER_REQ)
        n = len(reqs)
        assert len(infos) == n and len(old_values) == n and (keys is None or len(keys) == n)
        iblob, ioff = self._pack([x if x is not None else b"" for t in infos for x in t])
        ioff = ioff.astype(np.int32) if info_off is None else np.ascontiguousarray(info_off, dtype=np.int32)
        blob, off = self._pack(old_values)
        if old_off is not None:
            off = np.ascontiguousarray(old_off, dtype=np.int64)
        kblob = koff = rows = None
        if keys is not None:
            kblob, koff64 = self._pack(keys)
            koff = koff64.astype(np.int32) if key_off is None else np.ascontiguousarray(key_off, dtype=np.int32)
            rows = np.zeros(max(n, 1), np.int32)
        out = np.zeros(max(int(out_cap), 1), np.uint8)
        out_off = np.zeros(n + 1, np.int64)
        cls = np.zeros(max(n, 1), np.int32)
        lu = np.zeros(max(n, 1), np.int64)
        for a in (out, out_off, cls, lu) + (() if rows is None else (rows,)):
            a.view(np.uint8)[:] = fill
        total = C.c_int64(-1)
        rc = self.lib.mmp_models_register_json(self.h, ptr(reqs), n, kblob, ptr(koff), iblob, ptr(ioff), blob, ptr(off), int(now_ms),
                                               int(lastused_age_on_add_ms), flags, None if null_out else ptr(out), int(out_cap),
                                               ptr(out_off), ptr(cls), ptr(lu), ptr(rows), C.byref(total))
        return out[:int(out_cap)], out_off, cls[:n], lu[:n], None if rows is None else rows[:n], total.value, rc

    def models_refs_json(self, reqs, old_values, infos=None):
        """incRefCount / decRefCount on stored ModelRecord values (mmp_models_refs_json): reqs is a REFS_REQ array, old_values[i]
        the stored value (empty: mr == null), infos[i] = (type, encKey, mPath) as bytes/str with "" or None for null (None: no
        request brings one).  Returns (values, classes, refs): values[i] is bytes where classes[i] is MREFC_SET / MREFC_CREATED and
        None elsewhere, refs[i] the count the Java method returns.  Two calls: the sizes, then the bytes."""
        r = self.models_refs_json_raw(reqs, old_values, infos, 0)
        self._ck(r[5])
        out, off, cls, refs, total, rc = self.models_refs_json_raw(reqs, old_values, infos, r[4])
        self._ck(rc)
        assert total == r[4]  # (a pure function of the arguments)
        rendered = (_lib.MREFC_SET, _lib.MREFC_CREATED)
        vals = [bytes(out[off[i]:off[i + 1]]) if cls[i] in rendered else None for i in range(len(cls))]
        return vals, cls, refs

    def models_refs_json_raw(self, reqs, old_values, infos, out_cap, fill=0, null_out=False, flags=0, old_off=None, info_off=None):
        """One mmp_models_refs_json call with exactly this capacity (null_out: a NULL out_buf), the outputs filled with the byte
        `fill` first: (out bytes as uint8[out_cap], out_off[n + 1], classes[n], refs[n], total, rc); total is -1 where the library
        did not set it.  old_off / info_off: these offsets instead of the packed ones."""
        reqs = np.ascontiguousarray(reqs, dtype=_lib.REFS_REQ)
        n = len(reqs)
        assert len(old_values) == n and (infos is None or len(infos) == n)
        iblob = ioff = None
        if infos is not None:
            iblob, ioff = self._pack([x if x is not None else b"" for t in infos for x in t])
            ioff = ioff.astype(np.int32) if info_off is None else np.ascontiguousarray(info_off, dtype=np.int32)
        blob, off = self._pack(old_values)
        if old_off is not None:
            off = np.ascontiguousarray(old_off, dtype=np.int64)
        out = np.zeros(max(int(out_cap), 1), np.uint8)
        out_off = np.zeros(n + 1, np.int64)
        cls = np.zeros(max(n, 1), np.int32)
        refs = np.zeros(max(n, 1), np.int32)
        for a in (out, out_off, cls, refs):
            a.view(np.uint8)[:] = fill
        total = C.c_int64(-1)
        rc = self.lib.mmp_models_refs_json(self.h, ptr(reqs), n, iblob, ptr(ioff), blob, ptr(off), flags,
                                           None if null_out else ptr(out), int(out_cap), ptr(out_off), ptr(cls), ptr(refs),
                                           C.byref(total))
        return out[:int(out_cap)], out_off, cls[:n], refs[:n], total.value, rc

    def vmodels_write_json(self, reqs, strs, old_values, now_ms, lastused_age_on_add_ms, default_owner=b""):
        """The record step of the three vmodel writers (mmp_vmodels_write_json): reqs is a VMODEL_WRITE_REQ array, strs[i] =
        (id_a, id_b, owner) as bytes/str with "" or None for null, old_values[i] the stored VModelRecord value (empty: vmr == null).
        Returns (values, rows): values[i] is bytes where rows["cls"][i] is VWC_CREATED / VWC_UPDATED and None elsewhere, rows a
        VMODEL_WRITE_ROW array.  Two calls: the sizes, then the bytes."""
        args = (reqs, strs, old_values, now_ms, lastused_age_on_add_ms, default_owner)
        r = self.vmodels_write_json_raw(*args, 0)
        self._ck(r[4])
        out, off, rows, total, rc = self.vmodels_write_json_raw(*args, r[3])
        self._ck(rc)
        assert total == r[3]  # (read-only over a registry nobody edited in between)
        rendered = (_lib.VWC_CREATED, _lib.VWC_UPDATED)
        vals = [bytes(out[off[i]:off[i + 1]]) if rows["cls"][i] in rendered else None for i in range(len(rows))]
        return vals, rows

    def vmodels_write_json_raw(self, reqs, strs, old_values, now_ms, lastused_age_on_add_ms, default_owner, out_cap, fill=0,
                               null_out=False, flags=0, old_off=None, str_off=None):
        """One mmp_vmodels_write_json call with exactly this capacity (null_out: a NULL out_buf), the outputs filled with the byte
        `fill` first: (out bytes as uint8[out_cap], out_off[n + 1], rows[n], total, rc); total is -1 where the library did not set
        it.  old_off / str_off: these offsets instead of the packed ones."""
        reqs = np.ascontiguousarray(reqs, dtype=_lib.VMODEL_WRITE_REQ)
        n = len(reqs)
        assert len(strs) == n and len(old_values) == n
        sblob, soff = self._pack([x if x is not None else b"" for t in strs for x in t])
        soff = soff.astype(np.int32) if str_off is None else np.ascontiguousarray(str_off, dtype=np.int32)
        blob, off = self._pack(old_values)
        if old_off is not None:
            off = np.ascontiguousarray(old_off, dtype=np.int64)
        owner = default_owner.encode() if isinstance(default_owner, str) else bytes(default_owner or b"")
        out = np.zeros(max(int(out_cap), 1), np.uint8)
        out_off = np.zeros(n + 1, np.int64)
        rows = np.zeros(max(n, 1), _lib.VMODEL_WRITE_ROW)
        for a in (out, out_off, rows):
            a.view(np.uint8)[:] = fill
        total = C.c_int64(-1)
        rc = self.lib.mmp_vmodels_write_json(self.h, ptr(reqs), n, sblob, ptr(soff), owner or None, len(owner), blob, ptr(off),
                                             int(now_ms), int(lastused_age_on_add_ms), flags, None if null_out else ptr(out),
                                             int(out_cap), ptr(out_off), ptr(rows), C.byref(total))
        return out[:int(out_cap)], out_off, rows[:n], total.value, rc

    def model_ids_load(self, ids):
        """Name the registry's rows (mmp_model_ids_load): ids[i] (bytes/str) is the id of row i; len(ids) must equal the row count."""
        blob, off = self._pack(ids)
        off32 = off.astype(np.int32)
        self._ck(self.lib.mmp_model_ids_load(self.h, blob, ptr(off32), len(ids)))

    def model_ids_resolve(self, keys):
        """The registry row of every key, -1 for an unknown id (mmp_model_ids_resolve)."""
        blob, off = self._pack(keys)
        off32 = off.astype(np.int32)
        n = len(keys)
        out = np.full(max(n, 1), -1, np.int32)
        self._ck(self.lib.mmp_model_ids_resolve(self.h, blob, ptr(off32), n, ptr(out)))
        return out[:n]

    def model_ids_get(self, first_row=0, n_rows=None):
        """The ids (bytes) of rows [first_row, first_row + n_rows) (mmp_model_ids_get); n_rows=None: up to the last row."""
        if n_rows is None:
            n_rows = self.n_models - first_row
        nb = C.c_int32(0)
        self._ck(self.lib.mmp_model_ids_get(self.h, int(first_row), int(n_rows), None, 0, None, C.byref(nb)))
        buf = np.zeros(max(nb.value, 1), np.uint8)
        off = np.zeros(n_rows + 1, np.int32)
        self._ck(self.lib.mmp_model_ids_get(self.h, int(first_row), int(n_rows), ptr(buf), nb.value, ptr(off), C.byref(nb)))
        raw = buf.tobytes()
        return [raw[off[i]:off[i + 1]] for i in range(n_rows)]

    def models_events_json(self, keys, values, deleted=None, append=True):
        """Registry events by key (mmp_models_events_json): keys[i] is the model id (bytes/str), values[i] its ModelRecord JSON,
        deleted[i] marks ENTRY_DELETED.  Returns (status, model_idx, last_unload, n_appended)."""
        kblob, koff = self._pack(keys)
        koff32 = koff.astype(np.int32)
        blob, off = self._pack(values)
        n = len(keys)
        assert len(values) == n
        deleted = None if deleted is None else np.ascontiguousarray(deleted, dtype=np.uint8)
        lul = np.zeros(max(n, 1), np.int64)
        status = np.zeros(max(n, 1), np.int32)
        idx = np.full(max(n, 1), -1, np.int32)
        n_app = C.c_int32(0)
        self._ck(self.lib.mmp_models_events_json(self.h, kblob, ptr(koff32), blob, ptr(off), n, ptr(deleted),
                                                 _lib.MEV_APPEND if append else 0, ptr(idx), ptr(lul), ptr(status), C.byref(n_app)))
        if n:
            self.n_models = getattr(self, "n_models", 0) + n_app.value
            self._models = self._ent_pod = None  # (the registry now lives on the device only, as after ingest_models_json)
        return status[:n], idx[:n], lul[:n], n_app.value

    # ---- the vmodel table (VModelManager.java:101-110) ----

    def vmodels_events_json_raw(self, keys, values, deleted=None, flags=_lib.VMEV_APPEND, key_off=None, off=None, fill=0,
                                null_idx=False, null_status=False):
        """mmp_vmodels_events_json without the error check (tests: refusals): the outputs are pre-filled with `fill`, key_off /
        off replace the packed offsets.  Returns (status, vmodel_idx, n_appended, rc)."""
        kblob, koff = self._pack(keys)
        koff32 = koff.astype(np.int32) if key_off is None else np.ascontiguousarray(key_off, dtype=np.int32)
        blob, voff = self._pack(values)
        if off is not None:
            voff = np.ascontiguousarray(off, dtype=np.int64)
        n = len(keys)
        assert len(values) == n
        deleted = None if deleted is None else np.ascontiguousarray(deleted, dtype=np.uint8)
        status = np.zeros(max(n, 1), np.int32)
        idx = np.zeros(max(n, 1), np.int32)
        status.view(np.uint8)[:] = fill
        idx.view(np.uint8)[:] = fill
        n_app = C.c_int32(-1)
        rc = self.lib.mmp_vmodels_events_json(self.h, kblob, ptr(koff32), blob, ptr(voff), n, ptr(deleted), flags,
                                              None if null_idx else ptr(idx), None if null_status else ptr(status), C.byref(n_app))
        return status[:n], idx[:n], n_app.value, rc

    def vmodels_events_json(self, keys, values, deleted=None, append=True):
        """The vmodel listener's events by key (mmp_vmodels_events_json): keys[i] is the vmodel id (bytes/str), values[i] its
        VModelRecord JSON, deleted[i] marks ENTRY_DELETED.  Returns (status, vmodel_idx, n_appended)."""
        status, idx, n_app, rc = self.vmodels_events_json_raw(keys, values, deleted, _lib.VMEV_APPEND if append else 0)
        self._ck(rc)
        return status, idx, n_app

    def vmodels_resolve_raw(self, keys, nf=None, owners=None, req_flags=None, fill=0, key_off=None, null_out=False):
        """mmp_vmodels_resolve without the error check: nf / owners are lists of bytes/str/None (None and b"" are Java null), or
        None for a NULL buffer.  Returns (answers as VMODEL_ANSWER, rc)."""
        n = len(keys)
        kblob, koff = self._pack(keys)
        koff32 = koff.astype(np.int32) if key_off is None else np.ascontiguousarray(key_off, dtype=np.int32)
        nblob = noff = oblob = ooff = None
        if nf is not None:
            nblob, noff = self._pack([x if x is not None else b"" for x in nf])
            noff = noff.astype(np.int32)
        if owners is not None:
            oblob, ooff = self._pack([x if x is not None else b"" for x in owners])
            ooff = ooff.astype(np.int32)
        rf = None if req_flags is None else np.ascontiguousarray(req_flags, dtype=np.uint32)
        out = np.zeros(max(n, 1), _lib.VMODEL_ANSWER)
        out.view(np.uint8)[:] = fill
        rc = self.lib.mmp_vmodels_resolve(self.h, kblob, ptr(koff32), n, nblob, ptr(noff), oblob, ptr(ooff), ptr(rf),
                                          None if null_out else ptr(out))
        return out[:n], rc

    def vmodels_resolve(self, keys, nf=None, owners=None, req_flags=None):
        """resolveVModelId and the classes of getVModelStatus, one answer per key (mmp_vmodels_resolve)."""
        out, rc = self.vmodels_resolve_raw(keys, nf, owners, req_flags)
        self._ck(rc)
        return out

    def vmodels_transitions_raw(self, now_ms, lastused_age_on_add_ms, max_rows, fill=0, null_rows=False):
        """mmp_vmodels_transitions without the error check.  Returns (rows buffer of max_rows, n, info, rc)."""
        rows = np.zeros(max(int(max_rows), 1), _lib.VMODEL_TRANSITION)
        info = np.zeros(1, _lib.VMODEL_TRANSITIONS_INFO)
        rows.view(np.uint8)[:] = fill
        info.view(np.uint8)[:] = fill
        n = C.c_int32(-1)
        rc = self.lib.mmp_vmodels_transitions(self.h, int(now_ms), int(lastused_age_on_add_ms), None if null_rows else ptr(rows),
                                              int(max_rows), C.byref(n), ptr(info))
        return rows[:max(int(max_rows), 0)], n.value, info[0], rc

    def vmodels_transitions(self, now_ms, lastused_age_on_add_ms):
        """The leader's transition pass (mmp_vmodels_transitions): sizes first, then the rows.  Returns (rows, info)."""
        _, n, _, rc = self.vmodels_transitions_raw(now_ms, lastused_age_on_add_ms, 0, null_rows=True)
        self._ck(rc)
        rows, n2, info, rc = self.vmodels_transitions_raw(now_ms, lastused_age_on_add_ms, n)
        self._ck(rc)
        assert n2 == n
        return rows[:n], info

    def vmodels_info(self):
        """Rows, live rows, arena bytes, live arena bytes and table capacity of the vmodel table (mmp_vmodels_info)."""
        out = np.zeros(1, _lib.VMODELS_STATS)
        self._ck(self.lib.mmp_vmodels_info(self.h, ptr(out)))
        return out[0]

    def vmodels_get(self, first_row=0, n_rows=None):
        """Rows [first_row, first_row + n_rows) of the vmodel table (mmp_vmodels_get); n_rows=None: up to the last row.  Returns
        (ids, flags, strings): strings[r] = (amid, tmid, o) as bytes, None where the flags say null."""
        if n_rows is None:
            n_rows = int(self.vmodels_info()["n_rows"]) - first_row
        nid, nstr = C.c_int32(0), C.c_int32(0)
        self._ck(self.lib.mmp_vmodels_get(self.h, int(first_row), int(n_rows), None, 0, None, C.byref(nid), None, None, 0, None,
                                          C.byref(nstr)))
        ids = np.zeros(max(nid.value, 1), np.uint8)
        ioff = np.zeros(n_rows + 1, np.int32)
        flags = np.zeros(max(n_rows, 1), np.uint32)
        sb = np.zeros(max(nstr.value, 1), np.uint8)
        soff = np.zeros(3 * n_rows + 1, np.int32)
        self._ck(self.lib.mmp_vmodels_get(self.h, int(first_row), int(n_rows), ptr(ids), nid.value, ptr(ioff), C.byref(nid), ptr(flags),
                                          ptr(sb), nstr.value, ptr(soff), C.byref(nstr)))
        iraw, sraw = ids.tobytes(), sb.tobytes()
        null = (_lib.VMF_ACTIVE_NULL, _lib.VMF_TARGET_NULL, _lib.VMF_OWNER_NULL)
        strings = [tuple(None if flags[r] & null[k] else sraw[soff[3 * r + k]:soff[3 * r + k + 1]] for k in range(3))
                   for r in range(n_rows)]
        return [iraw[ioff[r]:ioff[r + 1]] for r in range(n_rows)], flags[:n_rows].copy(), strings

    def vmodels_retire_raw(self, rows=None, flags=0, fill=0, null_remap=False, max_vmodels=None, n=None):
        """mmp_vmodels_retire without the error check (tests: refusals): remap and n_after are pre-filled with `fill`; max_vmodels
        replaces the row count as remap's stated room, n the list's length, rows=None is a NULL list.  Returns (remap, n_after, rc)."""
        v0 = int(self.vmodels_info()["n_rows"])
        if rows is not None:
            rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
        room = v0 if max_vmodels is None else int(max_vmodels)
        remap = np.zeros(max(v0, room, 1), np.int32)
        after = np.zeros(1, np.int32)
        remap.view(np.uint8)[:] = fill
        after.view(np.uint8)[:] = fill
        rc = self.lib.mmp_vmodels_retire(self.h, ptr(rows) if rows is not None and len(rows) else None,
                                         (0 if rows is None else len(rows)) if n is None else int(n), int(flags),
                                         None if null_remap else ptr(remap), room, after.ctypes.data_as(C.POINTER(C.c_int32)))
        return remap[:v0], int(after[0]), rc

    def vmodels_retire(self, rows=None, absent_only=False, all_absent=False):
        """Retire vmodel rows (mmp_vmodels_retire): the rows leave the index space; rows, string arena and id table are compacted on
        the device.  all_absent: the device retires every ABSENT row (no list).  Returns (remap, n_after): remap is int32[V0], the
        new row of every old row, -1 for a retired one."""
        flags = (_lib.VMRETIRE_ABSENT_ONLY if absent_only else 0) | (_lib.VMRETIRE_ALL_ABSENT if all_absent else 0)
        remap, after, rc = self.vmodels_retire_raw(rows, flags)
        self._ck(rc)
        return remap, after

    def models_retire(self, rows, empty_only=False):
        """Retire registry rows (mmp_models_retire): the rows leave the index space, registry and id table are compacted on the
        device.  Returns remap, int32[M0]: the new row of every old row, -1 for a retired one."""
        rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
        m0 = getattr(self, "n_models", 0)
        remap = np.full(max(m0, 1), -1, np.int32)
        after = C.c_int32(0)
        self._ck(self.lib.mmp_models_retire(self.h, ptr(rows) if len(rows) else None, len(rows),
                                            _lib.RETIRE_EMPTY_ONLY if empty_only else 0, ptr(remap), m0, C.byref(after)))
        self.n_models = after.value
        if len(rows):
            self._models = self._ent_pod = None  # (the registry now lives on the device only, as after ingest_models_json)
        return remap[:m0]

    def pods_retire(self, pods, gone_only=False, unreferenced=False):
        """Retire instance rows (mmp_pods_retire): the instances leave the index space; the staged table, the id table, the type
        rows, the marks and the registry's entries are renumbered and, with a published snapshot, committed.  Returns
        (remap, n_entries_unresolved): remap is int32[P0], the new index of every old index, -1 for a retired one."""
        pods = np.ascontiguousarray(pods, dtype=np.int32).reshape(-1)
        p0 = self.n_pods
        remap = np.full(max(p0, 1), -1, np.int32)
        after, turned = C.c_int32(0), C.c_int64(0)
        flags = (_lib.PODS_RETIRE_GONE_ONLY if gone_only else 0) | (_lib.PODS_RETIRE_UNREFERENCED if unreferenced else 0)
        self._ck(self.lib.mmp_pods_retire(self.h, ptr(pods) if len(pods) else None, len(pods), flags, ptr(remap), p0,
                                          C.byref(after), C.byref(turned)))
        remap = remap[:p0]
        self.n_pods = after.value
        # the wrapper's own per-instance mirrors follow the renumbering: the live flags and the registry copy serve_counters reads
        mirror = getattr(self, "_live", None)
        if mirror is not None:
            self._grow_live(p0)
            self._live = self._live[:p0][remap >= 0]
        ent = getattr(self, "_ent_pod", None)
        if ent is not None and len(pods):
            ent = np.array(ent, dtype=np.int32)
            known = (ent >= 0) & (ent < p0)
            ent[known] = remap[ent[known]]
            self._ent_pod = ent
        return remap, turned.value

    def get_pods(self) -> np.ndarray:
        n = C.c_int32(0)
        self._ck(self.lib.mmp_pods_get(self.h, None, 0, C.byref(n)))
        rows = np.zeros(max(n.value, 1), dtype=POD_ROW)
        self._ck(self.lib.mmp_pods_get(self.h, ptr(rows), n.value, C.byref(n)))
        return rows[: n.value]

    def get_models(self):
        nm, ne = C.c_int32(0), C.c_int32(0)
        self._ck(self.lib.mmp_models_get(self.h, None, 0, None, None, 0, C.byref(nm), C.byref(ne)))
        rows = np.zeros(max(nm.value, 1), dtype=MODEL_ROW)
        ep = np.zeros(max(ne.value, 1), np.int32)
        et = np.zeros(max(ne.value, 1), np.int64)
        self._ck(self.lib.mmp_models_get(self.h, ptr(rows), nm.value, ptr(ep), ptr(et), ne.value, C.byref(nm), C.byref(ne)))
        return rows[: nm.value], ep[: ne.value], et[: ne.value]

    # UpgradeTracker (row a19)
    def upgrade_instance_added(self, labels_key, replica_set, start_time, now):
        self._ck(self.lib.mmp_upgrade_instance_added(self.h, int(labels_key), int(replica_set), int(start_time), int(now)))

    def upgrade_instance_removed(self, labels_key, replica_set, now):
        self._ck(self.lib.mmp_upgrade_instance_removed(self.h, int(labels_key), int(replica_set), int(now)))

    def upgrade_housekeeping(self, now):
        self._ck(self.lib.mmp_upgrade_housekeeping(self.h, int(now)))

    def upgrade_replaced(self) -> dict:
        rs = np.zeros(256, np.int32)
        ex = np.zeros(256, np.int64)
        n = C.c_int32(0)
        self._ck(self.lib.mmp_upgrade_replaced(self.h, ptr(rs), ptr(ex), 256, C.byref(n)))
        return {int(rs[i]): int(ex[i]) for i in range(min(n.value, 256))}

    def load_models(self, models, ent_pod, ent_time):
        models = np.ascontiguousarray(models, dtype=MODEL_ROW)
        ent_pod = np.ascontiguousarray(ent_pod, dtype=np.int32)
        ent_time = np.ascontiguousarray(ent_time, dtype=np.int64)
        self._ck(self.lib.mmp_models_load(self.h, ptr(models), len(models),
                                          ptr(ent_pod) if len(ent_pod) else None,
                                          ptr(ent_time) if len(ent_time) else None, len(ent_pod)))
        self.n_models = len(models)
        self._models, self._ent_pod = models.copy(), ent_pod.copy()  # host mirror for serve_counters

    def upsert_models(self, idx, rows, ent_pod, ent_time):
        """Registry events: rows[i] (its ent_off indexing ent_pod / ent_time of this call) replaces model idx[i]."""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        rows = np.ascontiguousarray(rows, dtype=MODEL_ROW)
        ent_pod = np.ascontiguousarray(ent_pod, dtype=np.int32)
        ent_time = np.ascontiguousarray(ent_time, dtype=np.int64)
        self._ck(self.lib.mmp_models_upsert(self.h, ptr(idx), ptr(rows), len(idx), ptr(ent_pod) if len(ent_pod) else None,
                                            ptr(ent_time) if len(ent_time) else None, len(ent_pod)))
        if len(idx):
            self.n_models = max(getattr(self, "n_models", 0), int(idx.max()) + 1)
            # the host mirror serve_counters reads: the changed records' entries are appended, their rows rewritten
            if getattr(self, "_models", None) is not None:
                if self.n_models > len(self._models):  # new records: the mirror grows with the registry
                    self._models = np.concatenate([self._models, np.zeros(self.n_models - len(self._models), MODEL_ROW)])
                shifted = rows.copy()
                shifted["ent_off"] += len(self._ent_pod)
                self._ent_pod = np.concatenate([self._ent_pod, ent_pod])
                self._models[idx] = shifted
                live_entries = int(self._models["n_loaded"].sum())
                if len(self._ent_pod) > 2 * live_entries + 1024:  # the replaced records' entries: compact, as the device pool does
                    k = self._models["n_loaded"].astype(np.int64)
                    off = np.zeros(len(k) + 1, np.int64)
                    np.cumsum(k, out=off[1:])
                    seg = np.repeat(np.arange(len(k)), k)
                    self._ent_pod = self._ent_pod[self._models["ent_off"][seg] + (np.arange(int(off[-1])) - off[seg])]
                    self._models["ent_off"] = off[:-1]

    def commit(self):
        self._ck(self.lib.mmp_snapshot_commit(self.h))

    def load_fleet(self, f: Fleet, commit: bool = True):
        """Stage a whole fleet; commit=False leaves the commit to the caller (pod-axis shard mode)."""
        self.load_pods(f.pods)
        self.load_types(f.n_types, f.allowed, f.prefer, f.has_allowed, f.has_prefer)
        self.load_replaced_rs(f.replaced_rs)
        self.load_models(f.models, f.ent_pod, f.ent_time)
        if commit:
            self.commit()

    def order(self) -> np.ndarray:
        out = np.zeros(max(self.n_pods, 1), dtype=np.int32)
        n = C.c_int32(0)
        self._ck(self.lib.mmp_get_order(self.h, ptr(out), C.byref(n)))
        return out[: n.value].copy()

    def delta_commits(self) -> int:
        """Commits of this context that re-ranked by insertion (a few changed rows) instead of sorting."""
        n = C.c_int64(0)
        self._ck(self.lib.mmp_delta_commits(self.h, C.byref(n)))
        return n.value

    def shortlists(self) -> np.ndarray:
        """The published snapshot's per-type shortlists (mmp_shortlists): rows [2 * type + bit] of (valid, lo, hi, n_candidates)."""
        out = np.zeros(24, dtype=np.dtype([("valid", "<i4"), ("lo", "<i4"), ("hi", "<i4"), ("n_candidates", "<i4")]))
        n = C.c_int32(0)
        self._ck(self.lib.mmp_shortlists(self.h, ptr(out), len(out), C.byref(n)))
        return out[: n.value].copy()

    def long_shortlists(self, cap_types: int = 256) -> np.ndarray:
        """The published snapshot's recorded walks of the long shortlists (mmp_long_shortlists): rows [2 * type + bit]."""
        out = np.zeros(2 * cap_types, dtype=np.dtype([("valid", "<i4"), ("lo", "<i4"), ("hi", "<i4"), ("n_candidates", "<i4")]))
        n = C.c_int32(0)
        self._ck(self.lib.mmp_long_shortlists(self.h, ptr(out), len(out), C.byref(n)))
        return out[: min(n.value, len(out))].copy()

    def split_batches(self):
        """(batches this context decided as two launches — shortlist check + tail —, whether that is switched off): mmp_split_batches."""
        n, off = C.c_int64(0), C.c_int32(0)
        self._ck(self.lib.mmp_split_batches(self.h, C.byref(n), C.byref(off)))
        return int(n.value), bool(off.value)

    def stats(self) -> np.ndarray:
        out = np.zeros(1, dtype=STATS)
        self._ck(self.lib.mmp_cluster_stats(self.h, ptr(out)))
        return out[0]

    def type_stats(self, type_row: int) -> np.ndarray:
        """typeSetStats(type): the stats of the instances a type may be placed on (cluster-wide if unconstrained)."""
        out = np.zeros(1, dtype=STATS)
        self._ck(self.lib.mmp_type_stats(self.h, int(type_row), ptr(out)))
        return out[0]

    def partitions(self):
        """-> (pod -> partition array, [(stats, prohibited type rows as a python int bitset)] per partition)"""
        n = np.zeros(1, np.int32)
        self._ck(self.lib.mmp_partition_count(self.h, ptr(n)))
        npods = np.zeros(1, np.int32)
        self._ck(self.lib.mmp_pod_partitions(self.h, None, 0, ptr(npods)))
        pts = np.zeros(max(int(npods[0]), 1), np.int32)
        self._ck(self.lib.mmp_pod_partitions(self.h, ptr(pts), int(npods[0]), ptr(npods)))
        out = []
        for k in range(int(n[0])):
            st = np.zeros(1, dtype=STATS)
            words = np.zeros(16, np.uint64)
            self._ck(self.lib.mmp_partition_stats(self.h, k, ptr(st), ptr(words), len(words)))
            out.append((st[0], sum(int(w) << (64 * i) for i, w in enumerate(words))))
        return pts[: int(npods[0])], out

    # ---- decisions -----------------------------------------------------
    def place(self, reqs: np.ndarray, extra_pool: Optional[np.ndarray], now: int) -> np.ndarray:
        reqs = np.ascontiguousarray(reqs, dtype=PLACE_REQ)
        extra = np.zeros(0, np.int32) if extra_pool is None else np.ascontiguousarray(extra_pool, dtype=np.int32)
        outs = np.zeros(len(reqs), dtype=PLACE_OUT)
        self._ck(self.lib.mmp_place_batch(self.h, ptr(reqs), len(reqs), ptr(extra) if len(extra) else None,
                                          len(extra), int(now), ptr(outs)))
        return outs

    def place_dev(self, d_reqs: int, n: int, d_extra: int, now: int, d_outs: int, stream: int = 0):
        """Launch on raw device pointers (torch ``data_ptr()``), no sync."""
        self._ck(self.lib.mmp_place_batch_dev(self.h, C.c_void_p(d_reqs), int(n), C.c_void_p(d_extra or None),
                                              int(now), C.c_void_p(d_outs), C.c_void_p(stream or None)))

    def place_dev2(self, d_reqs: int, n: int, d_extra: int, n_extra_pool: int, now: int, d_outs: int, stream: int = 0):
        """place_dev with the pool's length: requests whose exclusion range leaves it are answered MMP_BAD_REQUEST, not followed."""
        self._ck(self.lib.mmp_place_batch_dev2(self.h, C.c_void_p(d_reqs), int(n), C.c_void_p(d_extra or None), int(n_extra_pool),
                                               int(now), C.c_void_p(d_outs), C.c_void_p(stream or None)))

    def place_c(self, caller, reqs_c, extra_pool: Optional[np.ndarray], now: int) -> np.ndarray:
        """The single-caller form (mmp_place_batch_c): caller = 1 PLACE_CALLER row, reqs_c = PLACE_REQ_C rows."""
        return self._seam(self.lib.mmp_place_batch_c, [(caller, _lib.PLACE_CALLER)], [(reqs_c, _lib.PLACE_REQ_C)],
                          [[(extra_pool, np.int32)]], [now], [PLACE_OUT])[0]

    def place_c_dev(self, caller, d_reqs: int, n: int, d_extra: int, n_extra_pool: int, now: int, d_outs: int, stream: int = 0):
        """The single-caller form on raw device pointers (24-byte rows), no sync; `caller` is a host PLACE_CALLER row."""
        from ._lib import PLACE_CALLER
        caller = np.ascontiguousarray(caller, dtype=PLACE_CALLER).reshape(1)
        self._ck(self.lib.mmp_place_batch_c_dev(self.h, ptr(caller), C.c_void_p(d_reqs), int(n), C.c_void_p(d_extra or None),
                                                int(n_extra_pool), int(now), C.c_void_p(d_outs), C.c_void_p(stream or None)))

    def place_multi_dev(self, d_reqs, ns, d_extras, now: int, d_outs, stream: int = 0):
        """Several request arrays (raw device pointers), ONE launch, no sync: the same as place_dev per array."""
        k = len(d_reqs)
        arr = C.c_void_p * k
        r = arr(*[C.c_void_p(int(p)) for p in d_reqs])
        x = arr(*[C.c_void_p(int(p) or None) for p in d_extras])
        o = arr(*[C.c_void_p(int(p)) for p in d_outs])
        n = (C.c_int32 * k)(*[int(v) for v in ns])
        self._ck(self.lib.mmp_place_multi_dev(self.h, k, r, n, x, int(now), o, C.c_void_p(stream or None)))

    def serve_counters(self, reqs, in_use, last_used):
        """What a Java host assembles per request (MM.java:4343, :4356, :4360): for every copy of the request's model whose
        instance litelinks lists (here: the table's live flag), one (instance, inUse, lastUsed) entry.  -> (reqs with
        cnt_off / n_cnt filled, counters).  Needs the registry this Solver loaded (load_models)."""
        reqs = np.ascontiguousarray(reqs, dtype=SERVE_REQ).copy()
        in_use = np.ascontiguousarray(in_use, dtype=np.int32)
        last_used = np.ascontiguousarray(last_used, dtype=np.int64)
        models, ent_pod, live = getattr(self, "_models", None), getattr(self, "_ent_pod", None), getattr(self, "_live", None)
        if models is None or ent_pod is None or live is None:
            raise RuntimeError("serve_counters needs the host mirror of the registry and the instance list: load_models / load_pods "
                               "on this Solver (a registry ingested from JSON lives on the device only)")
        ok = (reqs["model"] >= 0) & (reqs["model"] < len(models))
        m = models[np.where(ok, reqs["model"], 0)]
        k = np.where(ok, m["n_loaded"], 0).astype(np.int64)
        off = np.zeros(len(reqs) + 1, np.int64)
        np.cumsum(k, out=off[1:])
        seg = np.repeat(np.arange(len(reqs)), k)
        j = np.arange(int(off[-1])) - off[seg]
        pod = ent_pod[m["ent_off"][seg] + j] if len(seg) else np.zeros(0, np.int32)
        listed = (pod >= 0) & (pod < len(live))
        listed[listed] &= live[pod[listed]]
        n_cnt = np.bincount(seg[listed], minlength=len(reqs)).astype(np.int32) if len(seg) else np.zeros(len(reqs), np.int32)
        c_off = np.zeros(len(reqs) + 1, np.int64)
        np.cumsum(n_cnt, out=c_off[1:])
        counters = np.zeros(int(c_off[-1]), dtype=SERVE_COUNTER)
        counters["pod"] = pod[listed]
        counters["in_use"] = in_use[pod[listed]]
        counters["last_used"] = last_used[pod[listed]]
        reqs["cnt_off"], reqs["n_cnt"] = c_off[:-1], n_cnt
        return reqs, counters

    def serve(self, reqs, in_use, last_used, excl_pod, excl_time, now) -> np.ndarray:
        """Convenience form for tests / benchmarks that hold per-INSTANCE counter arrays: builds the per-request counter
        entries (serve_counters) and calls serve_k."""
        reqs, counters = self.serve_counters(reqs, in_use, last_used)
        return self.serve_k(reqs, counters, excl_pod, excl_time, now)

    def serve_k(self, reqs, counters, excl_pod, excl_time, now) -> np.ndarray:
        """mmp_serve_batch: requests with their own (instance, inUse, lastUsed) entries — O(copies) per request."""
        reqs = np.ascontiguousarray(reqs, dtype=SERVE_REQ)
        counters = np.ascontiguousarray(counters, dtype=SERVE_COUNTER)
        excl_pod = np.ascontiguousarray(excl_pod, dtype=np.int32)
        excl_time = np.ascontiguousarray(excl_time, dtype=np.int64)
        outs = np.zeros(len(reqs), dtype=SERVE_OUT)
        self._ck(self.lib.mmp_serve_batch(self.h, ptr(reqs), len(reqs), ptr(counters) if len(counters) else None, len(counters),
                                          ptr(excl_pod) if len(excl_pod) else None,
                                          ptr(excl_time) if len(excl_time) else None, len(excl_pod),
                                          int(now), ptr(outs)))
        return outs

    def load_caches(self, seg_off, last_used, weight, capacity):
        seg_off = np.ascontiguousarray(seg_off, dtype=np.int32)
        last_used = np.ascontiguousarray(last_used, dtype=np.int64)
        weight = np.ascontiguousarray(weight, dtype=np.int32)
        capacity = np.ascontiguousarray(capacity, dtype=np.int64)
        self._ck(self.lib.mmp_caches_load(self.h, len(capacity), ptr(seg_off),
                                          ptr(last_used) if len(last_used) else None,
                                          ptr(weight) if len(weight) else None, ptr(capacity)))

    def evict(self, reqs, now) -> np.ndarray:
        reqs = np.ascontiguousarray(reqs, dtype=EVICT_REQ)
        outs = np.zeros(len(reqs), dtype=EVICT_OUT)
        self._ck(self.lib.mmp_evict_batch(self.h, ptr(reqs), len(reqs), int(now), ptr(outs)))
        return outs

    # ---- stateful keyed caches (rows a12 + a13) -------------------------------------------------
    def load_caches_keyed(self, seg_off, last_used, weight, key, capacity, ubm=None):
        from ._lib import UBM_STATE
        seg_off = np.ascontiguousarray(seg_off, dtype=np.int32)
        last_used = np.ascontiguousarray(last_used, dtype=np.int64)
        weight = np.ascontiguousarray(weight, dtype=np.int32)
        key = np.ascontiguousarray(key, dtype=np.int32)
        capacity = np.ascontiguousarray(capacity, dtype=np.int64)
        ubm = None if ubm is None else np.ascontiguousarray(ubm, dtype=UBM_STATE)
        self._kcache_slots = int(seg_off[-1])
        self._ck(self.lib.mmp_caches_load_keyed(self.h, len(capacity), ptr(seg_off),
                                                ptr(last_used) if len(last_used) else None,
                                                ptr(weight) if len(weight) else None, ptr(key) if len(key) else None,
                                                ptr(capacity), ptr(ubm)))

    def cache_replay(self, ops, now):
        """Apply clhm / ModelCacheUnloadBufManager operations in order; returns (outs, evicted_keys)."""
        from ._lib import CACHE_OP, CACHE_OP_OUT
        ops = np.ascontiguousarray(ops, dtype=CACHE_OP)
        outs = np.zeros(len(ops), dtype=CACHE_OP_OUT)
        self._kcache_slots = getattr(self, "_kcache_slots", 0) + len(ops)
        ev = np.zeros(max(self._kcache_slots, 1), np.int32)
        used = C.c_int32(0)
        self._ck(self.lib.mmp_cache_replay(self.h, ptr(ops) if len(ops) else None, len(ops), int(now),
                                           ptr(outs) if len(ops) else None, ptr(ev), len(ev), C.byref(used)))
        return outs, ev[: used.value]

    def cache_read(self, cache: int, max_entries: int = 4096):
        from ._lib import UBM_STATE
        lu = np.zeros(max_entries, np.int64)
        wt = np.zeros(max_entries, np.int32)
        key = np.zeros(max_entries, np.int32)
        n, cap, ws = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        ubm = np.zeros(1, dtype=UBM_STATE)
        self._ck(self.lib.mmp_cache_read(self.h, int(cache), max_entries, ptr(lu), ptr(wt), ptr(key), C.byref(n),
                                         C.byref(cap), C.byref(ws), ptr(ubm)))
        m = min(n.value, max_entries)
        return {"last_used": lu[:m], "weight": wt[:m], "key": key[:m], "capacity": cap.value,
                "weighted_size": ws.value, "ubm": ubm[0]}

    # ---- the stateful caches by model id: the key of an entry is the registry row its id names ----
    @staticmethod
    def _spans(raw, off, n):
        return [raw[off[i]:off[i + 1]] for i in range(n)]

    def load_caches_keyed_k(self, seg_off, last_used, weight, keys, capacity, ubm=None, is_unloadbuf=None, key_off=None, blob=None,
                            want_rows=True):
        """mmp_caches_load_keyed_k: keys[e] (bytes/str) is the model id of entry e; is_unloadbuf[e] marks the manager's
        pseudo-entry (its key is not read).  key_off / blob: raw offsets and bytes in place of `keys`.  Returns the entries' rows."""
        from ._lib import UBM_STATE
        seg_off = np.ascontiguousarray(seg_off, dtype=np.int32)
        last_used = np.ascontiguousarray(last_used, dtype=np.int64)
        weight = np.ascontiguousarray(weight, dtype=np.int32)
        capacity = np.ascontiguousarray(capacity, dtype=np.int64)
        ubm = None if ubm is None else np.ascontiguousarray(ubm, dtype=UBM_STATE)
        if blob is None:
            blob, off = self.pack_keys(keys)
        if key_off is not None:
            off = np.ascontiguousarray(key_off, dtype=np.int32)
        isu = None if is_unloadbuf is None else np.ascontiguousarray(is_unloadbuf, dtype=np.uint8)
        E = int(seg_off[-1])
        rows = np.full(max(E, 1), -1, np.int32)
        self._ck(self.lib.mmp_caches_load_keyed_k(self.h, len(capacity), ptr(seg_off), ptr(last_used) if len(last_used) else None,
                                                  ptr(weight) if len(weight) else None, blob, ptr(off), ptr(isu), ptr(capacity),
                                                  ptr(ubm), ptr(rows) if want_rows else None))
        self._kcache_slots = E
        return rows[:E]

    def cache_replay_k_raw(self, ops, keys, now, max_id_bytes, key_off=None, blob=None, fill=0, max_evicted=None, times=None):
        """mmp_cache_replay_k with a caller-sized id buffer.  Returns a dict: outs, evicted_rows, status, rows, id_off, id_bytes (the
        raw buffer, `fill` where nothing was written), need.  times: None = mmp_cache_replay_k; "out" = mmp_cache_replay_kt, the
        victims' lastUsed under "last_used"; "ctx" = mmp_cache_replay_kt with a NULL ev_last_used_out (the context keeps them)."""
        from ._lib import CACHE_OP, CACHE_OP_OUT
        ops = np.ascontiguousarray(ops, dtype=CACHE_OP)
        n = len(ops)
        if blob is None:
            blob, off = self.pack_keys(keys)
        if key_off is not None:
            off = np.ascontiguousarray(key_off, dtype=np.int32)
        outs = np.zeros(n, dtype=CACHE_OP_OUT)
        slots = getattr(self, "_kcache_slots", 0) + n if max_evicted is None else max_evicted
        ev = np.full(max(slots, 1), fill, np.int32)
        status = np.full(max(n, 1), fill, np.int32)
        rows = np.full(max(n, 1), fill, np.int32)
        id_off = np.full(max(slots, 0) + 1, fill, np.int32)
        buf = np.full(max(max_id_bytes, 1), fill, np.uint8)
        used, need = C.c_int32(0), C.c_int32(0)
        args = (self.h, ptr(ops) if n else None, n, blob, ptr(off), int(now), ptr(status), ptr(rows), ptr(outs) if n else None, ptr(ev),
                slots, C.byref(used), ptr(buf) if max_id_bytes else None, int(max_id_bytes), ptr(id_off), C.byref(need))
        lu = None
        if times is None:
            self._ck(self.lib.mmp_cache_replay_k(*args))
        else:
            lu = np.full(max(slots, 1), fill, np.int64) if times == "out" else None
            self._ck(self.lib.mmp_cache_replay_kt(*args, ptr(lu)))
        if max_evicted is None:
            self._kcache_slots = slots
        u = used.value
        r = {"outs": outs, "evicted_rows": ev[:u], "status": status[:n], "rows": rows[:n], "id_off": id_off[: u + 1],
             "id_bytes": buf[:max_id_bytes], "need": need.value}
        if lu is not None:
            r["last_used"] = lu[:u]
        return r

    def cache_replay_k(self, ops, keys, now, id_bytes_hint: int = 4096):
        """Apply cache operations by model id (mmp_cache_replay_k).  Returns (outs, evicted_rows, evicted_ids, status, rows):
        evicted_ids[s] is the id (bytes) of evicted_rows[s], b"" for a slot no op used.  The id buffer is sized by a hint; when
        it was short the ids come from the record the context keeps (mmp_cache_evicted_ids) — the replay itself ran once."""
        r = self.cache_replay_k_raw(ops, keys, now, id_bytes_hint)
        u = len(r["evicted_rows"])
        if r["need"] <= id_bytes_hint:
            ids = self._spans(r["id_bytes"][: r["need"]].tobytes(), r["id_off"], u)
        else:
            ids = self.cache_evicted_ids()
        return r["outs"], r["evicted_rows"], ids, r["status"], r["rows"]

    def cache_replay_kt(self, ops, keys, now, id_bytes_hint: int = 4096):
        """cache_replay_k with the victims' lastUsed (mmp_cache_replay_kt): returns (outs, evicted_rows, evicted_ids, status, rows,
        evicted_last_used); evicted_last_used[s] is the time entry evicted_rows[s] had when it was evicted, 0 for an unused slot."""
        r = self.cache_replay_k_raw(ops, keys, now, id_bytes_hint, times="out")
        u = len(r["evicted_rows"])
        if r["need"] <= id_bytes_hint:
            ids = self._spans(r["id_bytes"][: r["need"]].tobytes(), r["id_off"], u)
        else:
            ids = self.cache_evicted_ids()
        return r["outs"], r["evicted_rows"], ids, r["status"], r["rows"], r["last_used"]

    def cache_evicted_times(self):
        """The lastUsed of the victims of the last cache_replay_kt, one per eviction slot (mmp_cache_evicted_times, size then list).
        MmpError (MMP_ESTATE) when the last replay recorded none."""
        ns = C.c_int32(0)
        self._ck(self.lib.mmp_cache_evicted_times(self.h, None, 0, C.byref(ns)))
        out = np.zeros(max(ns.value, 1), np.int64)
        self._ck(self.lib.mmp_cache_evicted_times(self.h, ptr(out), ns.value, C.byref(ns)))
        return out[: ns.value]

    def cache_evicted_ids(self):
        """The ids the last cache_replay_k evicted, one per eviction slot (mmp_cache_evicted_ids, sizes then list)."""
        ns, nb = C.c_int32(0), C.c_int32(0)
        self._ck(self.lib.mmp_cache_evicted_ids(self.h, None, 0, None, C.byref(ns), C.byref(nb)))
        off = np.zeros(ns.value + 1, np.int32)
        buf = np.zeros(max(nb.value, 1), np.uint8)
        self._ck(self.lib.mmp_cache_evicted_ids(self.h, ptr(buf), nb.value, ptr(off), C.byref(ns), C.byref(nb)))
        return self._spans(buf.tobytes(), off, ns.value)

    def cache_read_k(self, cache: int, max_entries: int = 4096):
        """mmp_cache_read plus the entries' ids (mmp_cache_read_k): "row" are the keys, "ids" their model ids (b"" for the
        pseudo-entry, whose row is UNLOADBUF_KEY)."""
        from ._lib import UBM_STATE
        lu = np.zeros(max_entries, np.int64)
        wt = np.zeros(max_entries, np.int32)
        row = np.zeros(max_entries, np.int32)
        off = np.zeros(max_entries + 1, np.int32)
        n, nb, cap, ws = C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)
        ubm = np.zeros(1, dtype=UBM_STATE)
        self._ck(self.lib.mmp_cache_read_k(self.h, int(cache), max_entries, None, None, None, None, 0, None, C.byref(n), C.byref(nb),
                                           None, None, None))
        buf = np.zeros(max(nb.value, 1), np.uint8)
        self._ck(self.lib.mmp_cache_read_k(self.h, int(cache), max_entries, ptr(lu), ptr(wt), ptr(row), ptr(buf), nb.value, ptr(off),
                                           C.byref(n), C.byref(nb), C.byref(cap), C.byref(ws), ptr(ubm)))
        m = min(n.value, max_entries)
        return {"last_used": lu[:m], "weight": wt[:m], "row": row[:m], "ids": self._spans(buf.tobytes(), off, m),
                "capacity": cap.value, "weighted_size": ws.value, "ubm": ubm[0]}

    def gates(self, reqs, excl_pod, excl_time, explicit_pool, now, in_use_failure_expiry_ms=450_000) -> np.ndarray:
        from ._lib import GATE_OUT, GATE_REQ
        reqs = np.ascontiguousarray(reqs, dtype=GATE_REQ)
        excl_pod = np.ascontiguousarray(excl_pod, dtype=np.int32)
        excl_time = np.ascontiguousarray(excl_time, dtype=np.int64)
        explicit_pool = np.ascontiguousarray(explicit_pool, dtype=np.int32)
        outs = np.zeros(len(reqs), dtype=GATE_OUT)
        self._ck(self.lib.mmp_gate_batch(self.h, ptr(reqs), len(reqs), ptr(excl_pod) if len(excl_pod) else None,
                                         ptr(excl_time) if len(excl_time) else None, len(excl_pod),
                                         ptr(explicit_pool) if len(explicit_pool) else None, len(explicit_pool),
                                         int(now), int(in_use_failure_expiry_ms), ptr(outs)))
        return outs

    # ---- the per-request seams: route (cache hit), miss (cache miss), the load target; by row, single-caller, by id ----
    @staticmethod
    def _pool(a, dtype):
        """One array of a request call as the library takes it: (the contiguous array, its pointer or None when empty, its length)."""
        a = np.zeros(0, dtype) if a is None else np.ascontiguousarray(a, dtype=dtype)
        return a, (ptr(a) if len(a) else None), len(a)

    def _seam(self, fn, callers, rows, pools, times, out_dtypes, keyed=(), row_out=None):
        """One request-seam call, the arguments in the order every seam of include/mmplace.h has them:
        fn(ctx, *callers, *rows, n, *keyed, *(pool.., length).., *times, *outs, row_out) -> the outs.
        callers / rows: (array, dtype) each, n the length of the first rows; pools: groups of (array, dtype) that share one
        length (the exclusion pods and times); keyed / row_out: what a call by id adds (_keyed)."""
        callers = [self._pool(np.ascontiguousarray(a, dtype=dt).reshape(1), dt) for a, dt in callers]
        rows = [self._pool(a, dt) for a, dt in rows]
        n = rows[0][2]
        args = [self.h] + [p for _, p, _ in callers + rows] + [n] + [ptr(k) if isinstance(k, np.ndarray) else k for k in keyed]
        keep = [callers, rows]
        for group in pools:
            group = [self._pool(a, dt) for a, dt in group]
            keep.append(group)
            args += [p for _, p, _ in group] + [group[0][2]]
        args += [C.c_int64(int(t)) for t in times]
        outs = [np.zeros(n, dtype=dt) for dt in out_dtypes]
        args += [ptr(o) if n else None for o in outs]
        if keyed:
            args.append(ptr(row_out))
        self._ck(fn(*args))
        return outs

    @staticmethod
    def pack_keys(keys):
        """keys (a list of bytes / str, str as UTF-8) as the by-key calls take them, packed as model_ids_resolve packs them:
        (the bytes joined, n + 1 int32 offsets)."""
        blob, off = Solver._pack(keys)
        return blob, off.astype(np.int32)

    def _vkey_args(self, n, keys, nf, req_flags, want_vm):
        """What the _cv calls add: (key blob, key offsets, nf blob, nf offsets, flags, vm_out).  nf is a list of
        bytes/str/None (None and b"" are Java null) or None for NULL buffers; req_flags n words or None."""
        assert len(keys) == n
        blob, off = self.pack_keys(keys)
        nblob = noff = None
        if nf is not None:
            assert len(nf) == n
            nblob, noff = self.pack_keys([x if x is not None else b"" for x in nf])
        rf = None if req_flags is None else np.ascontiguousarray(req_flags, dtype=np.uint32)
        assert rf is None or len(rf) == n
        vm = np.zeros(max(n, 1), _lib.VSEAM_ROW)
        vm.view(np.uint8)[:] = 0xEE
        return blob, off, nblob, noff, rf, (vm if want_vm else None)

    def _keyed(self, rows, keys, want, vmodel=False, nf=None, req_flags=None):
        """What a call by id adds to the call it resolves in front of, as _seam's keywords: the arguments behind n (_ck: key blob
        and offsets; _cv: _vkey_args) and the rows it resolves (model_idx filled with -2, vm rows with 0xEE; None: a NULL output).
        rows: the request arrays, which are as long as keys."""
        n = len(rows[0])
        assert all(len(r) == n for r in rows)
        if vmodel:
            *keyed, out = self._vkey_args(n, keys, nf, req_flags, want)
        else:
            assert len(keys) == n
            keyed, out = self.pack_keys(keys), (np.full(max(n, 1), -2, np.int32) if want else None)
        return {"keyed": tuple(keyed), "row_out": out}, (out[:n] if want else None)

    def _route(self, fn, caller, gate_reqs, serve_reqs, counters, excl_pod, excl_time, explicit_pool, now, expiry, keyed=None):
        c = caller is not None
        return self._seam(fn, [(caller, _lib.SEAM_CALLER)] if c else [],
                          [(gate_reqs, _lib.GATE_REQ_C if c else _lib.GATE_REQ), (serve_reqs, _lib.SERVE_REQ_C if c else SERVE_REQ)],
                          [[(counters, SERVE_COUNTER)], [(excl_pod, np.int32), (excl_time, np.int64)], [(explicit_pool, np.int32)]],
                          [now, expiry], [_lib.GATE_OUT, SERVE_OUT], **(keyed or {}))

    def _miss(self, fn, callers, gate_reqs, place_reqs, excl_pod, excl_time, explicit_pool, extra_pool, now, expiry, keyed=None):
        c = callers is not None
        return self._seam(fn, [(callers[0], _lib.SEAM_CALLER), (callers[1], _lib.PLACE_CALLER)] if c else [],
                          [(gate_reqs, _lib.GATE_REQ_C if c else _lib.GATE_REQ), (place_reqs, _lib.PLACE_REQ_C if c else PLACE_REQ)],
                          [[(excl_pod, np.int32), (excl_time, np.int64)], [(explicit_pool, np.int32)], [(extra_pool, np.int32)]],
                          [now, expiry], [_lib.GATE_OUT, PLACE_OUT], **(keyed or {}))

    def route(self, gate_reqs, serve_reqs, counters, excl_pod, excl_time, explicit_pool, now, in_use_failure_expiry_ms=450_000):
        """The cache-hit route in one launch (mmp_route_batch): -> (gate outs, serve outs)."""
        return tuple(self._route(self.lib.mmp_route_batch, None, gate_reqs, serve_reqs, counters, excl_pod, excl_time, explicit_pool,
                                 now, in_use_failure_expiry_ms))

    def miss(self, gate_reqs, place_reqs, excl_pod, excl_time, explicit_pool, extra_pool, now, in_use_failure_expiry_ms=450_000):
        """The cache-miss route in one call (mmp_miss_batch): the request guards + the load target -> (gate outs, place outs)."""
        return tuple(self._miss(self.lib.mmp_miss_batch, None, gate_reqs, place_reqs, excl_pod, excl_time, explicit_pool, extra_pool,
                                now, in_use_failure_expiry_ms))

    def route_c(self, caller, gate_reqs_c, serve_reqs_c, counters, excl_pod, excl_time, explicit_pool, now,
                in_use_failure_expiry_ms=450_000):
        """The single-caller form of route (mmp_route_batch_c): caller = 1 SEAM_CALLER row, GATE_REQ_C / SERVE_REQ_C rows
        -> (gate outs, serve outs)."""
        return tuple(self._route(self.lib.mmp_route_batch_c, caller, gate_reqs_c, serve_reqs_c, counters, excl_pod, excl_time,
                                 explicit_pool, now, in_use_failure_expiry_ms))

    def miss_c(self, caller, place_caller, gate_reqs_c, place_reqs_c, excl_pod, excl_time, explicit_pool, extra_pool, now,
               in_use_failure_expiry_ms=450_000):
        """The single-caller form of miss (mmp_miss_batch_c): caller = 1 SEAM_CALLER row, place_caller = 1 PLACE_CALLER row,
        GATE_REQ_C / PLACE_REQ_C rows -> (gate outs, place outs)."""
        return tuple(self._miss(self.lib.mmp_miss_batch_c, (caller, place_caller), gate_reqs_c, place_reqs_c, excl_pod, excl_time,
                                explicit_pool, extra_pool, now, in_use_failure_expiry_ms))

    # ---- the single-caller forms by model id (mmp_place_batch_ck / _route_batch_ck / _miss_batch_ck) ----
    def place_batch_ck(self, caller, reqs_c, keys, extra_pool, now, want_idx=True):
        """mmp_place_batch_c with request i's model named by keys[i]: -> (outs, model_idx); the `model` field of reqs_c is
        ignored.  want_idx=False passes a NULL model_idx_out and returns None for it."""
        keyed, idx = self._keyed([reqs_c], keys, want_idx)
        outs, = self._seam(self.lib.mmp_place_batch_ck, [(caller, _lib.PLACE_CALLER)], [(reqs_c, _lib.PLACE_REQ_C)],
                           [[(extra_pool, np.int32)]], [now], [PLACE_OUT], **keyed)
        return outs, idx

    def route_batch_ck(self, caller, gate_reqs_c, serve_reqs_c, keys, counters, excl_pod, excl_time, explicit_pool, now,
                       in_use_failure_expiry_ms=450_000, want_idx=True):
        """mmp_route_batch_c with request i's model named by keys[i]: -> (gate outs, serve outs, model_idx)."""
        keyed, idx = self._keyed([gate_reqs_c, serve_reqs_c], keys, want_idx)
        return (*self._route(self.lib.mmp_route_batch_ck, caller, gate_reqs_c, serve_reqs_c, counters, excl_pod, excl_time,
                             explicit_pool, now, in_use_failure_expiry_ms, keyed), idx)

    def miss_batch_ck(self, caller, place_caller, gate_reqs_c, place_reqs_c, keys, excl_pod, excl_time, explicit_pool, extra_pool, now,
                      in_use_failure_expiry_ms=450_000, want_idx=True):
        """mmp_miss_batch_c with request i's model named by keys[i]: -> (gate outs, place outs, model_idx)."""
        keyed, idx = self._keyed([gate_reqs_c, place_reqs_c], keys, want_idx)
        return (*self._miss(self.lib.mmp_miss_batch_ck, (caller, place_caller), gate_reqs_c, place_reqs_c, excl_pod, excl_time,
                            explicit_pool, extra_pool, now, in_use_failure_expiry_ms, keyed), idx)

    # ---- the single-caller forms by vmodel id (mmp_place_batch_cv / _route_batch_cv / _miss_batch_cv) ----
    def place_batch_cv(self, caller, reqs_c, keys, extra_pool, now, nf=None, req_flags=None, want_vm=True):
        """mmp_place_batch_c with request i's model named by the VMODEL id keys[i], resolved (resolveVModelId with nf[i] and
        req_flags[i]) inside the call: -> (outs, vm rows as VSEAM_ROW); the `model` field of reqs_c is ignored.  want_vm=False
        passes a NULL vm_out and returns None for it."""
        keyed, vm = self._keyed([reqs_c], keys, want_vm, True, nf, req_flags)
        outs, = self._seam(self.lib.mmp_place_batch_cv, [(caller, _lib.PLACE_CALLER)], [(reqs_c, _lib.PLACE_REQ_C)],
                           [[(extra_pool, np.int32)]], [now], [PLACE_OUT], **keyed)
        return outs, vm

    def route_batch_cv(self, caller, gate_reqs_c, serve_reqs_c, keys, counters, excl_pod, excl_time, explicit_pool, now,
                       in_use_failure_expiry_ms=450_000, nf=None, req_flags=None, want_vm=True):
        """mmp_route_batch_c with request i's model named by the VMODEL id keys[i]: -> (gate outs, serve outs, vm rows)."""
        keyed, vm = self._keyed([gate_reqs_c, serve_reqs_c], keys, want_vm, True, nf, req_flags)
        return (*self._route(self.lib.mmp_route_batch_cv, caller, gate_reqs_c, serve_reqs_c, counters, excl_pod, excl_time,
                             explicit_pool, now, in_use_failure_expiry_ms, keyed), vm)

    def miss_batch_cv(self, caller, place_caller, gate_reqs_c, place_reqs_c, keys, excl_pod, excl_time, explicit_pool, extra_pool, now,
                      in_use_failure_expiry_ms=450_000, nf=None, req_flags=None, want_vm=True):
        """mmp_miss_batch_c with request i's model named by the VMODEL id keys[i]: -> (gate outs, place outs, vm rows)."""
        keyed, vm = self._keyed([gate_reqs_c, place_reqs_c], keys, want_vm, True, nf, req_flags)
        return (*self._miss(self.lib.mmp_miss_batch_cv, (caller, place_caller), gate_reqs_c, place_reqs_c, excl_pod, excl_time,
                            explicit_pool, extra_pool, now, in_use_failure_expiry_ms, keyed), vm)

    def proactive_plan(self, default_model_size_units: int, now: int, max_out: int, partition: int = -1, skip_models=None):
        """a17: (models, last_used, info) the leader would proactively load, MRU first; partition >= 0: for that
        ProhibitedTypeSet partition only (one reaper call per partition when type constraints exist)."""
        from ._lib import PROACTIVE_INFO
        om = np.zeros(max(max_out, 1), np.int32)
        ol = np.zeros(max(max_out, 1), np.int64)
        info = np.zeros(1, dtype=PROACTIVE_INFO)
        skip = np.ascontiguousarray(skip_models if skip_models is not None else np.zeros(0, np.int32), dtype=np.int32)
        self._ck(self.lib.mmp_proactive_plan_subset(self.h, int(partition), ptr(skip) if len(skip) else None, len(skip),
                                                    int(default_model_size_units), int(now), int(max_out),
                                                    ptr(om), ptr(ol), ptr(info)))
        n = min(int(info[0]["n_selected"]), max_out)
        return om[:n].copy(), ol[:n].copy(), info[0]

    def prune_registry(self, self_pod: int, now: int, gone_after_ms: int = 600_000, lastused_age_on_add_ms: int = 3_600_000,
                       apply: bool = True, dry: bool = False, max_edits: int = 1024, max_removed: int = 4096):
        """The reaper's first half (pruneModelRegistry, MM.java:6524-6609): (edits, removed, info).  The buffers start at
        max_edits / max_removed and are regrown to the run's totals when it reports `truncated` (a truncated run changes nothing)."""
        from ._lib import PRUNE_APPLY, PRUNE_DRY, PRUNE_EDIT, PRUNE_INFO, PRUNE_REMOVED
        flags = PRUNE_DRY if dry else (PRUNE_APPLY if apply else 0)
        info = np.zeros(1, dtype=PRUNE_INFO)
        while True:
            edits = np.zeros(max(max_edits, 1), dtype=PRUNE_EDIT)
            removed = np.zeros(max(max_removed, 1), dtype=PRUNE_REMOVED)
            self._ck(self.lib.mmp_registry_prune(self.h, int(self_pod), int(now), int(gone_after_ms), int(lastused_age_on_add_ms),
                                                 flags, ptr(edits), int(max_edits), ptr(removed), int(max_removed), ptr(info)))
            if not info[0]["truncated"]:
                break
            max_edits, max_removed = max(max_edits, int(info[0]["n_edits"])), max(max_removed, int(info[0]["n_removed"]))
        ne, nr = int(info[0]["n_edits"]), int(info[0]["n_removed"])
        if flags == PRUNE_APPLY and ne and getattr(self, "_models", None) is not None:
            self._models, self._ent_pod, _ = (a.copy() for a in self.get_models())  # the host mirror serve_counters reads
        return edits[:ne].copy(), removed[:nr].copy(), info[0].copy()

    def prune_registry_raw(self, self_pod, now, gone_after_ms, lastused_age_on_add_ms, flags, max_edits, max_removed):
        """One mmp_registry_prune call with exactly these capacities: (edits prefix, removed prefix, info)."""
        from ._lib import PRUNE_EDIT, PRUNE_INFO, PRUNE_REMOVED
        info = np.zeros(1, dtype=PRUNE_INFO)
        edits = np.zeros(max(max_edits, 1), dtype=PRUNE_EDIT)
        removed = np.zeros(max(max_removed, 1), dtype=PRUNE_REMOVED)
        self._ck(self.lib.mmp_registry_prune(self.h, int(self_pod), int(now), int(gone_after_ms), int(lastused_age_on_add_ms), int(flags),
                                             ptr(edits) if max_edits else None, int(max_edits), ptr(removed) if max_removed else None,
                                             int(max_removed), ptr(info)))
        return (edits[: min(max_edits, int(info[0]["n_edits"]))].copy(), removed[: min(max_removed, int(info[0]["n_removed"]))].copy(),
                info[0].copy())

    def missing_instances(self) -> dict:
        """`missings` (MM.java:6776) by pod index: {pod: first time seen missing}."""
        n = C.c_int32(0)
        self._ck(self.lib.mmp_registry_missing_get(self.h, None, 0, C.byref(n)))
        since = np.zeros(max(n.value, 1), np.int64)
        self._ck(self.lib.mmp_registry_missing_get(self.h, ptr(since), n.value, C.byref(n)))
        return {int(p): int(since[p]) for p in np.nonzero(since[: n.value])[0]}

    def missing_slots(self) -> int:
        """Pod slots the missing map covers."""
        n = C.c_int32(0)
        self._ck(self.lib.mmp_registry_missing_get(self.h, None, 0, C.byref(n)))
        return n.value

    def reset_missing_instances(self):
        """missings.clear() on a leader change (MM.java:6827)."""
        self._ck(self.lib.mmp_registry_missing_reset(self.h))

    def janitor_plan(self, entries, params, apply: bool = True, dry: bool = False, max_edits: int = 1024, max_candidates: int = 1024):
        """The janitor's cache and registry loops (MM.java:5892-6008, :6014-6108) for one instance: (actions, edits, candidates,
        candidate rows, info).  The candidates go to scaledown_plan unchanged.  The buffers are regrown to the run's totals when it
        reports `truncated` (a truncated run changes nothing)."""
        from ._lib import JANITOR_APPLY, JANITOR_DRY
        flags = JANITOR_DRY if dry else (JANITOR_APPLY if apply else 0)
        while True:
            out = self.janitor_plan_raw(entries, params, flags, max_edits, max_candidates)
            info = out[4]
            if not info["truncated"]:
                break
            max_edits, max_candidates = max(max_edits, int(info["n_edits"])), max(max_candidates, int(info["n_candidates"]))
        if flags == JANITOR_APPLY and int(info["n_edits"]) and getattr(self, "_models", None) is not None:
            self._models, self._ent_pod, _ = (a.copy() for a in self.get_models())  # the host mirror serve_counters reads
        return out

    def janitor_plan_raw(self, entries, params, flags, max_edits, max_candidates):
        """One mmp_janitor_plan call with exactly these capacities: (actions, edits prefix, candidates prefix, rows prefix, info)."""
        from ._lib import CACHE_ENTRY, JANITOR_EDIT, JANITOR_ENTRY, JANITOR_INFO, JANITOR_PARAMS
        entries = np.ascontiguousarray(entries, dtype=JANITOR_ENTRY)
        params = np.ascontiguousarray(params, dtype=JANITOR_PARAMS).reshape(1)
        n = len(entries)
        info = np.zeros(1, dtype=JANITOR_INFO)
        actions = np.zeros(max(n, 1), np.uint8)
        edits = np.zeros(max(max_edits, 1), dtype=JANITOR_EDIT)
        cands = np.zeros(max(max_candidates, 1), dtype=CACHE_ENTRY)
        rows = np.zeros(max(max_candidates, 1), np.int32)
        self._ck(self.lib.mmp_janitor_plan(self.h, ptr(entries) if n else None, n, ptr(params), int(flags), ptr(actions) if n else None,
                                           ptr(edits) if max_edits else None, int(max_edits), ptr(cands) if max_candidates else None,
                                           ptr(rows) if max_candidates else None, int(max_candidates), ptr(info)))
        ne, nc = min(max_edits, int(info[0]["n_edits"])), min(max_candidates, int(info[0]["n_candidates"]))
        return actions[:n].copy(), edits[:ne].copy(), cands[:nc].copy(), rows[:nc].copy(), info[0].copy()

    def registry_ops(self, ops, now: int, apply: bool = True, dry: bool = False, max_edits: int = 1024):
        """The edits an instance makes to ModelRecords itself (loadLocal MM.java:5204-5207, the load-failure path :2484-2495,
        deregisterModel :2948-2958, removeLocalModelCopyAsync :6347-6365), a batch of mmp_registry_op rows: (status, edits, info),
        the edits in op order.  The buffer is regrown to the call's total when it reports `truncated` (a truncated call changes
        nothing)."""
        from ._lib import ROPS_APPLY, ROPS_DRY
        flags = ROPS_DRY if dry else (ROPS_APPLY if apply else 0)
        while True:
            out = self.registry_ops_raw(ops, now, flags, max_edits)
            info = out[2]
            if not info["truncated"]:
                break
            max_edits = max(max_edits, int(info["n_edits"]))
        if flags == ROPS_APPLY and int(info["n_edits"]) and getattr(self, "_models", None) is not None:
            self._models, self._ent_pod, _ = (a.copy() for a in self.get_models())  # the host mirror serve_counters reads
        return out

    def registry_ops_raw(self, ops, now, flags, max_edits, want_status=True):
        """One mmp_registry_ops call with exactly this capacity (0: a NULL buffer): (status, edits prefix, info)."""
        from ._lib import REGISTRY_OP, REGISTRY_OP_EDIT, REGISTRY_OPS_INFO
        ops = np.ascontiguousarray(ops, dtype=REGISTRY_OP)
        n = len(ops)
        info = np.zeros(1, dtype=REGISTRY_OPS_INFO)
        status = np.zeros(max(n, 1), np.uint8)
        edits = np.zeros(max(max_edits, 1), dtype=REGISTRY_OP_EDIT)
        self._ck(self.lib.mmp_registry_ops(self.h, ptr(ops) if n else None, n, int(now), int(flags), ptr(status) if n and want_status else None,
                                           ptr(edits) if max_edits else None, int(max_edits), ptr(info)))
        ne = min(max_edits, int(info[0]["n_edits"]))
        return status[:n].copy(), edits[:ne].copy(), info[0].copy()

    def registry_ops_k(self, ops, keys, now: int, apply: bool = True, dry: bool = False, max_edits: int = 1024):
        """registry_ops BY MODEL ID, with the fifth kind ROP_DROP_LOCAL (the cache-hit loop's drop of its own copy, MM.java:3682-3687):
        (model_idx, status, edits, info) from one mmp_registry_ops_k call — the key resolved, the op evaluated and the edit applied
        under one hold of the batch lock; an unknown id and the empty row a deletion leaves answer ROP_NO_RECORD.  keys=None: by row
        (ops["model"]).  The buffer is regrown to the call's total when it reports `truncated` (a truncated call changes nothing)."""
        from ._lib import ROPS_APPLY, ROPS_DRY
        flags = ROPS_DRY if dry else (ROPS_APPLY if apply else 0)
        while True:
            idx, status, edits, info, rc = self.registry_ops_k_raw(ops, keys, now, flags, max_edits)
            self._ck(rc)
            if not info["truncated"]:
                break
            max_edits = max(max_edits, int(info["n_edits"]))
        if flags == ROPS_APPLY and int(info["n_edits"]) and getattr(self, "_models", None) is not None:
            self._models, self._ent_pod, _ = (a.copy() for a in self.get_models())  # the host mirror serve_counters reads
        return idx, status, edits, info

    def registry_ops_k_raw(self, ops, keys, now, flags, max_edits, fill=0, key_off=None, blob=None, null_keys=False, null_off=False,
                           null_status=False, null_idx=False, null_info=False, null_ops=False):
        """One mmp_registry_ops_k call with exactly this capacity (0: a NULL edits buffer), the outputs filled with the byte `fill`
        first: (model_idx, status, edits[:min(n_edits, max_edits)] — all max_edits rows when the call fails —, info, rc).  Does not
        raise.  keys: a list of bytes/str, or None for the by-row form (both key pointers NULL); key_off / blob replace the packed
        offsets / bytes; the null_* switches pass NULL for that one argument."""
        from ._lib import REGISTRY_OP, REGISTRY_OP_EDIT, REGISTRY_OPS_INFO_K
        ops = np.ascontiguousarray(ops, dtype=REGISTRY_OP)
        n = len(ops)
        kblob, off32 = None, None
        if keys is not None:
            kblob, off = self._pack(keys)
            off32 = off.astype(np.int32)
        if blob is not None:
            kblob = blob
        if key_off is not None:
            off32 = np.ascontiguousarray(key_off, dtype=np.int32)
        info = np.zeros(1, dtype=REGISTRY_OPS_INFO_K)
        idx = np.zeros(max(n, 1), np.int32)
        status = np.zeros(max(n, 1), np.uint8)
        edits = np.zeros(max(max_edits, 1), dtype=REGISTRY_OP_EDIT)
        for a in (info, idx, status, edits):
            a.view(np.uint8)[:] = fill
        rc = self.lib.mmp_registry_ops_k(self.h, None if null_ops or not n else ptr(ops), n, None if null_keys else kblob,
                                         None if null_off or off32 is None else ptr(off32), int(now), int(flags),
                                         None if null_idx else ptr(idx), None if null_status else ptr(status),
                                         ptr(edits) if max_edits else None, int(max_edits), None if null_info else ptr(info))
        ne = max_edits if rc != 0 else min(max_edits, int(info[0]["n_edits"]))
        return idx[:n].copy(), status[:n].copy(), edits[:ne].copy(), info[0].copy(), rc

    def evictions_k(self, entries, keys, self_pod: int, now: int, load_timeout_ms: int, apply: bool = True, dry: bool = False,
                    max_edits: int = 1024):
        """onEviction's task body by model id (mmp_evictions_k, MM.java:2886-2920) for a batch of victims — mmp_evicted_entry rows
        and their ids, e.g. the record of cache_replay_kt: (model_idx, outs, status, edits, info).  outs[i]: EVO_* flags, the
        deregistration's status, loaded_time, millis_since_last_used.  Regrown like registry_ops_k when truncated."""
        from ._lib import ROPS_APPLY, ROPS_DRY
        flags = ROPS_DRY if dry else (ROPS_APPLY if apply else 0)
        while True:
            idx, outs, status, edits, info, rc = self.evictions_k_raw(entries, keys, self_pod, now, load_timeout_ms, flags, max_edits)
            self._ck(rc)
            if not info["ops"]["truncated"]:
                break
            max_edits = max(max_edits, int(info["ops"]["n_edits"]))
        if flags == ROPS_APPLY and int(info["ops"]["n_edits"]) and getattr(self, "_models", None) is not None:
            self._models, self._ent_pod, _ = (a.copy() for a in self.get_models())  # the host mirror serve_counters reads
        return idx, outs, status, edits, info

    def evictions_k_raw(self, entries, keys, self_pod, now, load_timeout_ms, flags, max_edits, fill=0, key_off=None, blob=None):
        """One mmp_evictions_k call with exactly this edit capacity, the outputs filled with the byte `fill` first:
        (model_idx, outs, status, edits, info, rc).  Does not raise."""
        from ._lib import EVICT_PARAMS, EVICTED_ENTRY, EVICTED_OUT, EVICTIONS_INFO, REGISTRY_OP_EDIT
        entries = np.ascontiguousarray(entries, dtype=EVICTED_ENTRY)
        n = len(entries)
        kblob, off = self._pack(keys)
        off32 = off.astype(np.int32)
        if blob is not None:
            kblob = blob
        if key_off is not None:
            off32 = np.ascontiguousarray(key_off, dtype=np.int32)
        p = np.zeros(1, dtype=EVICT_PARAMS)
        p[0] = (int(self_pod), 0, int(now), int(load_timeout_ms))
        info = np.zeros(1, dtype=EVICTIONS_INFO)
        idx = np.zeros(max(n, 1), np.int32)
        outs = np.zeros(max(n, 1), dtype=EVICTED_OUT)
        status = np.zeros(max(n, 1), np.uint8)
        edits = np.zeros(max(max_edits, 1), dtype=REGISTRY_OP_EDIT)
        for a in (info, idx, outs, status, edits):
            a.view(np.uint8)[:] = fill
        rc = self.lib.mmp_evictions_k(self.h, ptr(entries) if n else None, n, kblob, ptr(off32), ptr(p), int(flags), ptr(idx), ptr(outs),
                                      ptr(status), ptr(edits) if max_edits else None, int(max_edits), ptr(info))
        ne = max_edits if rc != 0 else min(max_edits, int(info[0]["ops"]["n_edits"]))
        return idx[:n].copy(), outs[:n].copy(), status[:n].copy(), edits[:ne].copy(), info[0].copy(), rc

    def models_status(self, reqs, now: int):
        """getStatus answers (MM.java:3247; class :3760-3768, copy list makeStatusInfo :3013-3058) for a batch of mmp_status_req
        rows from the resident registry: (rows, copies) — one mmp_status_row per request, and the copies of request i, latest
        first, at copies[rows[i].copy_off : ... + n_not_checked + n_failed].  Two calls: the sizes, then the list; repeated if
        the registry changed in between."""
        max_copies = self.models_status_raw(reqs, now, 0)[2]
        while True:
            rows, copies, total, rc = self.models_status_raw(reqs, now, max_copies)
            self._ck(rc)
            if total <= max_copies:
                return rows, copies
            max_copies = total

    def models_status_raw(self, reqs, now, max_copies, fill=0, null_out=False):
        """One mmp_models_status call with exactly this capacity (0: a NULL copies buffer), the outputs filled with the byte
        `fill` first: (rows, copies[:min(total, max_copies)] — all max_copies rows when the call fails —, total, rc).  Does not
        raise: rc is the return code (total is -1 where the library did not set it).  null_out: NULL rows_out and n_copies_out."""
        from ._lib import STATUS_COPY, STATUS_REQ, STATUS_ROW
        reqs = np.ascontiguousarray(reqs, dtype=STATUS_REQ)
        n = len(reqs)
        rows = np.zeros(max(n, 1), dtype=STATUS_ROW)
        copies = np.zeros(max(max_copies, 1), dtype=STATUS_COPY)
        rows.view(np.uint8)[:] = fill
        copies.view(np.uint8)[:] = fill
        total = C.c_int32(-1)
        rc = self.lib.mmp_models_status(self.h, ptr(reqs) if n else None, n, int(now), None if null_out else ptr(rows),
                                        ptr(copies) if max_copies else None, int(max_copies), None if null_out else C.byref(total))
        got = max_copies if rc != 0 else min(max_copies, max(total.value, 0))
        return rows[:n].copy(), copies[:got].copy(), total.value, rc

    def models_status_k_raw(self, keys, now, max_copies, fail_pod=None, flags=None, fill=0, key_off=None, null_out=False,
                            null_idx=False):
        """One mmp_models_status_k call with exactly this capacity (0: a NULL copies buffer), the outputs filled with the byte `fill`
        first: (model_idx, rows, copies[:min(total, max_copies)] — all max_copies rows when the call fails —, total, rc).  Does not
        raise.  fail_pod / flags: n words or None (NULL); key_off replaces the packed offsets; null_out: NULL rows_out and
        n_copies_out; null_idx: NULL model_idx_out."""
        from ._lib import STATUS_COPY, STATUS_ROW
        n = len(keys)
        blob, off = self._pack(keys)
        off32 = off.astype(np.int32) if key_off is None else np.ascontiguousarray(key_off, dtype=np.int32)
        fp = None if fail_pod is None else np.ascontiguousarray(fail_pod, dtype=np.int32)
        fl = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint32)
        idx = np.zeros(max(n, 1), np.int32)
        rows = np.zeros(max(n, 1), dtype=STATUS_ROW)
        copies = np.zeros(max(max_copies, 1), dtype=STATUS_COPY)
        for a in (idx, rows, copies):
            a.view(np.uint8)[:] = fill
        total = C.c_int32(-1)
        rc = self.lib.mmp_models_status_k(self.h, blob, ptr(off32), n, ptr(fp), ptr(fl), int(now), None if null_idx else ptr(idx),
                                          None if null_out else ptr(rows), ptr(copies) if max_copies else None, int(max_copies),
                                          None if null_out else C.byref(total))
        got = max_copies if rc != 0 else min(max_copies, max(total.value, 0))
        return idx[:n].copy(), rows[:n].copy(), copies[:got].copy(), total.value, rc

    def models_status_k(self, keys, now: int, fail_pod=None, flags=None):
        """getStatus by model id (mmp_models_status_k): (model_idx, rows, copies) — what model_ids_resolve and models_status answer,
        from one call under one hold of the batch lock; an unknown id and the empty row a deletion leaves answer MST_NOT_FOUND.  Two
        calls: the sizes, then the list; repeated if the registry changed in between."""
        max_copies = self.models_status_k_raw(keys, now, 0, fail_pod, flags)[3]
        while True:
            idx, rows, copies, total, rc = self.models_status_k_raw(keys, now, max(max_copies, 0), fail_pod, flags)
            self._ck(rc)
            if total <= max_copies:
                return idx, rows, copies
            max_copies = total

    def vmodels_status_raw(self, keys, now, max_copies, max_str_bytes, owners=None, req_flags=None, fill=0, key_off=None,
                           owner_off=None, null_out=False, null_str_off=False):
        """One mmp_vmodels_status call with exactly these capacities (0: a NULL buffer), the outputs filled with the byte `fill`
        first.  owners: a list of bytes/str/None (None and b"" are Java null), or None for NULL buffers.  Returns a dict: vrows,
        rows (2n), copies (the part written; all of it when the call fails), n_copies, str_off (3n + 1), str_bytes (the whole
        buffer), n_str_bytes, rc.  Does not raise."""
        from ._lib import STATUS_COPY, STATUS_ROW, VSTATUS_ROW
        n = len(keys)
        kblob, koff = self._pack(keys)
        koff32 = koff.astype(np.int32) if key_off is None else np.ascontiguousarray(key_off, dtype=np.int32)
        oblob = ooff = None
        if owners is not None:
            oblob, ooff = self._pack([x if x is not None else b"" for x in owners])
            ooff = ooff.astype(np.int32) if owner_off is None else np.ascontiguousarray(owner_off, dtype=np.int32)
        rf = None if req_flags is None else np.ascontiguousarray(req_flags, dtype=np.uint32)
        vrows = np.zeros(max(n, 1), VSTATUS_ROW)
        rows = np.zeros(max(2 * n, 1), STATUS_ROW)
        copies = np.zeros(max(max_copies, 1), STATUS_COPY)
        soff = np.zeros(3 * n + 1, np.int32)
        sbytes = np.zeros(max(max_str_bytes, 1), np.uint8)
        for a in (vrows, rows, copies, soff, sbytes):
            a.view(np.uint8)[:] = fill
        nc, ns = C.c_int32(-1), C.c_int32(-1)
        rc = self.lib.mmp_vmodels_status(self.h, kblob, ptr(koff32), n, oblob, ptr(ooff), ptr(rf), int(now),
                                         None if null_out else ptr(vrows), None if null_out else ptr(rows),
                                         ptr(copies) if max_copies else None, int(max_copies), None if null_out else C.byref(nc),
                                         ptr(sbytes) if max_str_bytes else None, int(max_str_bytes), None if null_str_off else ptr(soff),
                                         C.byref(ns))
        got = max_copies if rc != 0 else min(max_copies, max(nc.value, 0))
        return dict(vrows=vrows[:n].copy(), rows=rows[:2 * n].copy(), copies=copies[:got].copy(), n_copies=nc.value, str_off=soff,
                    str_bytes=sbytes[:max_str_bytes].copy(), n_str_bytes=ns.value, rc=rc)

    def vmodels_status(self, keys, now: int, owners=None, req_flags=None):
        """getVModelStatus in full (mmp_vmodels_status): (vrows, rows, copies, strings) — one mmp_vstatus_row per key, the active
        model's status row at rows[2i] and the target's at rows[2i + 1] with their copies, and strings[i] = (amid, tmid, o) as bytes,
        None where the row's flags say null.  Every part of one answer is of one state.  Two calls: the sizes, then the lists;
        repeated if the state changed in between."""
        r = self.vmodels_status_raw(keys, now, 0, 0, owners, req_flags)
        self._ck(r["rc"])
        mc, ms = r["n_copies"], r["n_str_bytes"]
        while True:
            r = self.vmodels_status_raw(keys, now, mc, ms, owners, req_flags)
            self._ck(r["rc"])
            if r["n_copies"] <= mc and r["n_str_bytes"] <= ms:
                break
            mc, ms = max(mc, r["n_copies"]), max(ms, r["n_str_bytes"])
        raw, soff, vrows = r["str_bytes"].tobytes(), r["str_off"], r["vrows"]
        null = (_lib.VMF_ACTIVE_NULL, _lib.VMF_TARGET_NULL, _lib.VMF_OWNER_NULL)
        found = [int(v["cls"]) in (_lib.VMR_OK, _lib.VMR_STRONG_READ) for v in vrows]
        strings = [tuple(None if (not found[i] or vrows[i]["flags"] & null[k]) else raw[soff[3 * i + k]:soff[3 * i + k + 1]]
                         for k in range(3)) for i in range(len(keys))]
        return vrows, r["rows"], r["copies"], strings

    def registry_census(self):
        """The registry listener's model counts (MM.java:2807-2854, :6852-6863) over the resident registry: (stats, pod_loaded,
        pod_failed, type_stats) — one mmp_registry_stats row, per pod slot of the staged instance table the records that hold it in
        instanceIds / in loadFailedInstanceIds, and one mmp_registry_type_stats row per row of the type table."""
        while True:
            n_pods, n_types = self.registry_census_sizes()
            stats, pl, pf, ts, got_pods, got_types, rc = self.registry_census_raw(n_pods, n_types)
            if rc == _lib.MMP_EINVAL and (got_pods, got_types) != (n_pods, n_types):
                continue  # a table grew between the two calls
            self._ck(rc)
            return stats, pl, pf, ts

    def registry_census_sizes(self):
        """(pod slots, type rows) the census covers."""
        from ._lib import REGISTRY_STATS
        stats = np.zeros(1, dtype=REGISTRY_STATS)
        n_pods, n_types = C.c_int32(0), C.c_int32(0)
        self._ck(self.lib.mmp_registry_census(self.h, ptr(stats), None, None, 0, C.byref(n_pods), None, 0, C.byref(n_types)))
        return n_pods.value, n_types.value

    def registry_census_raw(self, max_pods, max_types, fill=0):
        """One mmp_registry_census call with exactly these capacities (0: a NULL buffer), the arrays filled with `fill` first:
        (stats, pod_loaded, pod_failed, type_stats, n_pods, n_types, rc).  Does not raise: rc is the return code."""
        from ._lib import REGISTRY_STATS, REGISTRY_TYPE_STATS
        stats = np.zeros(1, dtype=REGISTRY_STATS)
        pl = np.full(max(max_pods, 1), fill, np.int32)
        pf = np.full(max(max_pods, 1), fill, np.int32)
        ts = np.zeros(max(max_types, 1), dtype=REGISTRY_TYPE_STATS)
        ts.view(np.int32)[:] = fill
        n_pods, n_types = C.c_int32(-1), C.c_int32(-1)
        rc = self.lib.mmp_registry_census(self.h, ptr(stats), ptr(pl) if max_pods else None, ptr(pf) if max_pods else None, int(max_pods),
                                          C.byref(n_pods), ptr(ts) if max_types else None, int(max_types), C.byref(n_types))
        return stats[0].copy(), pl[:max_pods], pf[:max_pods], ts[:max_types], n_pods.value, n_types.value, rc

    def scaleup_plan(self, entries, params):
        """a15: (outs, overloaded[P], skipped)"""
        from ._lib import CACHE_ENTRY, SCALEUP_OUT, SCALEUP_PARAMS
        entries = np.ascontiguousarray(entries, dtype=CACHE_ENTRY)
        params = np.ascontiguousarray(params, dtype=SCALEUP_PARAMS).reshape(1)
        outs = np.zeros(len(entries), dtype=SCALEUP_OUT)
        ov = np.zeros(max(self.n_pods, 1), np.uint8)
        sk = C.c_int32(0)
        self._ck(self.lib.mmp_scaleup_plan(self.h, ptr(entries) if len(entries) else None, len(entries), ptr(params),
                                           ptr(outs) if len(entries) else None, ptr(ov), C.byref(sk)))
        return outs, ov[: self.n_pods], sk.value

    def scaleup_plan_conc(self, entries, conc, params, conc_params):
        """a15 with limitModelConcurrency == true (latency-based): (outs, conc_outs, overloaded[P], skipped, result)"""
        from ._lib import CACHE_ENTRY, CONC_ENTRY, CONC_OUT, CONC_PARAMS, CONC_RESULT, SCALEUP_OUT, SCALEUP_PARAMS
        entries = np.ascontiguousarray(entries, dtype=CACHE_ENTRY)
        conc = np.ascontiguousarray(conc, dtype=CONC_ENTRY)
        assert len(conc) == len(entries)
        params = np.ascontiguousarray(params, dtype=SCALEUP_PARAMS).reshape(1)
        cparams = np.ascontiguousarray(conc_params, dtype=CONC_PARAMS).reshape(1)
        outs = np.zeros(len(entries), dtype=SCALEUP_OUT)
        couts = np.zeros(len(entries), dtype=CONC_OUT)
        res = np.zeros(1, dtype=CONC_RESULT)
        ov = np.zeros(max(self.n_pods, 1), np.uint8)
        sk = C.c_int32(0)
        n = len(entries)
        self._ck(self.lib.mmp_scaleup_plan_conc(self.h, ptr(entries) if n else None, ptr(conc) if n else None, n, ptr(params),
                                                ptr(cparams), ptr(outs) if n else None, ptr(couts) if n else None, ptr(ov),
                                                C.byref(sk), ptr(res)))
        return outs, couts, ov[: self.n_pods], sk.value, res[0]

    def scaledown_plan_conc(self, entries, conc, params, dynamic_rpm_scale_constant):
        from ._lib import CACHE_ENTRY, CONC_ENTRY, SCALEDOWN_PARAMS
        entries = np.ascontiguousarray(entries, dtype=CACHE_ENTRY)
        conc = np.ascontiguousarray(conc, dtype=CONC_ENTRY)
        assert len(conc) == len(entries)
        params = np.ascontiguousarray(params, dtype=SCALEDOWN_PARAMS).reshape(1)
        rem = np.zeros(max(len(entries), 1), np.uint8)
        n = len(entries)
        self._ck(self.lib.mmp_scaledown_plan_conc(self.h, ptr(entries) if n else None, ptr(conc) if n else None, n, ptr(params),
                                                  int(dynamic_rpm_scale_constant), ptr(rem)))
        return rem[:n]

    def scaledown_plan(self, entries, params):
        from ._lib import CACHE_ENTRY, SCALEDOWN_PARAMS
        entries = np.ascontiguousarray(entries, dtype=CACHE_ENTRY)
        params = np.ascontiguousarray(params, dtype=SCALEDOWN_PARAMS).reshape(1)
        rem = np.zeros(max(len(entries), 1), np.uint8)
        self._ck(self.lib.mmp_scaledown_plan(self.h, ptr(entries) if len(entries) else None, len(entries), ptr(params),
                                             ptr(rem)))
        return rem[: len(entries)]

    def migration_plan(self, entries, self_pod, now, cutoff_age_ms=3_600_000):
        from ._lib import CACHE_ENTRY
        entries = np.ascontiguousarray(entries, dtype=CACHE_ENTRY)
        act = np.zeros(max(len(entries), 1), np.uint8)
        wait = np.zeros(max(len(entries), 1), np.uint8)
        self._ck(self.lib.mmp_migration_plan(self.h, ptr(entries) if len(entries) else None, len(entries), int(self_pod),
                                             int(now), int(cutoff_age_ms), ptr(act), ptr(wait)))
        return act[: len(entries)], wait[: len(entries)]

    # ---- the periodic tasks BY MODEL ID (include/mmplace.h "THE PERIODIC TASKS BY MODEL ID") ----
    def _task_keys(self, keys, key_off, blob, null_keys, null_off):
        """(key bytes, int32 offsets) as a _raw form passes them: keys a list of bytes/str or None (by row: both pointers NULL);
        key_off / blob replace the packed offsets / bytes; the null_* switches pass NULL for that one argument."""
        kblob, off32 = None, None
        if keys is not None:
            kblob, off = self._pack(keys)
            off32 = off.astype(np.int32)
        if blob is not None:
            kblob = blob
        if key_off is not None:
            off32 = np.ascontiguousarray(key_off, dtype=np.int32)
        return (None if null_keys else kblob), (None if null_off or off32 is None else off32)

    def scaleup_plan_k(self, entries, keys, params, conc=None, conc_params=None):
        """The rate task by model id: (model_idx, outs, overloaded[P], skipped) — with conc / conc_params (limitModelConcurrency ==
        true) (model_idx, outs, conc_outs, overloaded[P], skipped, result) — from one mmp_scaleup_plan_k call: the keys resolved
        and the entries evaluated under one hold of the batch lock; an unknown id and the empty row a deletion leaves are
        model == -1.  keys=None: by row (entries["model"])."""
        idx, outs, couts, ov, sk, res, rc = self.scaleup_plan_k_raw(entries, keys, params, conc, conc_params)
        self._ck(rc)
        return (idx, outs, ov, sk) if conc_params is None else (idx, outs, couts, ov, sk, res)

    def scaleup_plan_k_raw(self, entries, keys, params, conc=None, conc_params=None, fill=0, key_off=None, blob=None, null_keys=False,
                           null_off=False, null_idx=False, null_outs=False, null_skipped=False):
        """One mmp_scaleup_plan_k call, the outputs filled with the byte `fill` first: (model_idx, outs, conc_outs, overloaded,
        skipped, result, rc).  Does not raise."""
        from ._lib import CACHE_ENTRY, CONC_ENTRY, CONC_OUT, CONC_PARAMS, CONC_RESULT, SCALEUP_OUT, SCALEUP_PARAMS
        entries = np.ascontiguousarray(entries, dtype=CACHE_ENTRY)
        n = len(entries)
        params = np.ascontiguousarray(params, dtype=SCALEUP_PARAMS).reshape(1)
        kblob, off32 = self._task_keys(keys, key_off, blob, null_keys, null_off)
        latency = conc_params is not None
        if latency:
            conc = np.ascontiguousarray(conc, dtype=CONC_ENTRY)
            assert len(conc) == n
            cparams = np.ascontiguousarray(conc_params, dtype=CONC_PARAMS).reshape(1)
        idx = np.zeros(max(n, 1), np.int32)
        outs = np.zeros(max(n, 1), dtype=SCALEUP_OUT)
        couts = np.zeros(max(n, 1), dtype=CONC_OUT)
        res = np.zeros(1, dtype=CONC_RESULT)
        ov = np.zeros(max(self.n_pods, 1), np.uint8)
        sk = np.zeros(1, np.int32)
        for a in (idx, outs, couts, res, ov, sk):
            a.view(np.uint8)[:] = fill
        rc = self.lib.mmp_scaleup_plan_k(self.h, ptr(entries) if n else None, ptr(conc) if latency and n else None, n, kblob,
                                         None if off32 is None else ptr(off32), ptr(params), ptr(cparams) if latency else None,
                                         None if null_outs or not n else ptr(outs), ptr(couts) if latency and n else None, ptr(ov),
                                         None if null_skipped else sk.ctypes.data_as(C.POINTER(C.c_int32)),
                                         ptr(res) if latency else None, None if null_idx else ptr(idx))
        return idx[:n].copy(), outs[:n].copy(), couts[:n].copy(), ov[: self.n_pods].copy(), int(sk[0]), res[0].copy(), rc

    def scaledown_plan_k(self, entries, keys, params, conc=None, dynamic_rpm_scale_constant=0):
        """The janitor's scale-down by model id: (model_idx, removed) from one mmp_scaledown_plan_k call.  keys=None: by row."""
        idx, rem, rc = self.scaledown_plan_k_raw(entries, keys, params, conc, dynamic_rpm_scale_constant)
        self._ck(rc)
        return idx, rem

    def scaledown_plan_k_raw(self, entries, keys, params, conc=None, dynamic_rpm_scale_constant=0, fill=0, key_off=None, blob=None,
                             null_keys=False, null_off=False, null_idx=False, null_removed=False):
        """One mmp_scaledown_plan_k call, the outputs filled with the byte `fill` first: (model_idx, removed, rc).  Does not raise."""
        from ._lib import CACHE_ENTRY, CONC_ENTRY, SCALEDOWN_PARAMS
        entries = np.ascontiguousarray(entries, dtype=CACHE_ENTRY)
        n = len(entries)
        params = np.ascontiguousarray(params, dtype=SCALEDOWN_PARAMS).reshape(1)
        kblob, off32 = self._task_keys(keys, key_off, blob, null_keys, null_off)
        if conc is not None:
            conc = np.ascontiguousarray(conc, dtype=CONC_ENTRY)
            assert len(conc) == n
        idx = np.zeros(max(n, 1), np.int32)
        rem = np.zeros(max(n, 1), np.uint8)
        for a in (idx, rem):
            a.view(np.uint8)[:] = fill
        rc = self.lib.mmp_scaledown_plan_k(self.h, ptr(entries) if n else None, ptr(conc) if conc is not None and n else None, n, kblob,
                                           None if off32 is None else ptr(off32), ptr(params), int(dynamic_rpm_scale_constant),
                                           None if null_removed else ptr(rem), None if null_idx else ptr(idx))
        return idx[:n].copy(), rem[:n].copy(), rc

    def migration_plan_k(self, entries, keys, self_pod, now, cutoff_age_ms=3_600_000):
        """preShutdown's migration by model id: (model_idx, action, wait) from one mmp_migration_plan_k call.  keys=None: by row."""
        idx, act, wait, rc = self.migration_plan_k_raw(entries, keys, self_pod, now, cutoff_age_ms)
        self._ck(rc)
        return idx, act, wait

    def migration_plan_k_raw(self, entries, keys, self_pod, now, cutoff_age_ms=3_600_000, fill=0, key_off=None, blob=None, null_keys=False,
                             null_off=False, null_idx=False, null_action=False):
        """One mmp_migration_plan_k call, the outputs filled with the byte `fill` first: (model_idx, action, wait, rc).  Does not raise."""
        from ._lib import CACHE_ENTRY
        entries = np.ascontiguousarray(entries, dtype=CACHE_ENTRY)
        n = len(entries)
        kblob, off32 = self._task_keys(keys, key_off, blob, null_keys, null_off)
        idx = np.zeros(max(n, 1), np.int32)
        act = np.zeros(max(n, 1), np.uint8)
        wait = np.zeros(max(n, 1), np.uint8)
        for a in (idx, act, wait):
            a.view(np.uint8)[:] = fill
        rc = self.lib.mmp_migration_plan_k(self.h, ptr(entries) if n else None, n, kblob, None if off32 is None else ptr(off32), int(self_pod),
                                           int(now), int(cutoff_age_ms), None if null_action else ptr(act), ptr(wait),
                                           None if null_idx else ptr(idx))
        return idx[:n].copy(), act[:n].copy(), wait[:n].copy(), rc

    def janitor_plan_k(self, entries, keys, params, apply: bool = True, dry: bool = False, scaledown=None, conc=None,
                       dynamic_rpm_scale_constant=0, max_edits: int = 1024, max_candidates: int = 1024):
        """janitorTask by model id: (model_idx, actions, edits, candidates, candidate rows, removed, info) from one
        mmp_janitor_plan_k call — the keys resolved, the two loops evaluated and applied and, with `scaledown` (its params; conc:
        the MaxConcCacheEntry rows in INPUT-row order), the candidates' scale-down decided under one hold of the batch lock;
        removed is None without `scaledown`.  keys=None: by row.  The buffers are regrown to the run's totals when it reports
        `truncated` (a truncated run changes nothing)."""
        from ._lib import JANITOR_APPLY, JANITOR_DRY
        flags = JANITOR_DRY if dry else (JANITOR_APPLY if apply else 0)
        while True:
            out = self.janitor_plan_k_raw(entries, keys, params, flags, max_edits, max_candidates, scaledown, conc, dynamic_rpm_scale_constant)
            self._ck(out[-1])
            info = out[6]
            if not info["truncated"]:
                break
            max_edits, max_candidates = max(max_edits, int(info["n_edits"])), max(max_candidates, int(info["n_candidates"]))
        if flags == JANITOR_APPLY and int(info["n_edits"]) and getattr(self, "_models", None) is not None:
            self._models, self._ent_pod, _ = (a.copy() for a in self.get_models())  # the host mirror serve_counters reads
        return out[:5] + (out[5] if scaledown is not None else None,) + (info,)

    def janitor_plan_k_raw(self, entries, keys, params, flags, max_edits, max_candidates, scaledown=None, conc=None,
                           dynamic_rpm_scale_constant=0, fill=0, key_off=None, blob=None, null_keys=False, null_off=False, null_idx=False,
                           null_removed=False, null_info=False):
        """One mmp_janitor_plan_k call with exactly these capacities (0: NULL buffers), the outputs filled with the byte `fill`
        first: (model_idx, actions, edits, candidates, rows, removed, info, rc) — the prefixes the call reports, every row of each
        buffer when it fails.  Does not raise."""
        from ._lib import CACHE_ENTRY, CONC_ENTRY, JANITOR_EDIT, JANITOR_ENTRY, JANITOR_INFO, JANITOR_PARAMS, SCALEDOWN_PARAMS
        entries = np.ascontiguousarray(entries, dtype=JANITOR_ENTRY)
        params = np.ascontiguousarray(params, dtype=JANITOR_PARAMS).reshape(1)
        n = len(entries)
        kblob, off32 = self._task_keys(keys, key_off, blob, null_keys, null_off)
        if scaledown is not None:
            scaledown = np.ascontiguousarray(scaledown, dtype=SCALEDOWN_PARAMS).reshape(1)
        if conc is not None:
            conc = np.ascontiguousarray(conc, dtype=CONC_ENTRY)
            assert len(conc) == n
        info = np.zeros(1, dtype=JANITOR_INFO)
        idx = np.zeros(max(n, 1), np.int32)
        actions = np.zeros(max(n, 1), np.uint8)
        edits = np.zeros(max(max_edits, 1), dtype=JANITOR_EDIT)
        cands = np.zeros(max(max_candidates, 1), dtype=CACHE_ENTRY)
        rows = np.zeros(max(max_candidates, 1), np.int32)
        rem = np.zeros(max(max_candidates, 1), np.uint8)
        for a in (info, idx, actions, edits, cands, rows, rem):
            a.view(np.uint8)[:] = fill
        rc = self.lib.mmp_janitor_plan_k(self.h, ptr(entries) if n else None, n, kblob, None if off32 is None else ptr(off32), ptr(params),
                                         int(flags), None if scaledown is None else ptr(scaledown),
                                         ptr(conc) if conc is not None and n else None, int(dynamic_rpm_scale_constant),
                                         None if null_idx else ptr(idx), ptr(actions) if n else None, ptr(edits) if max_edits else None,
                                         int(max_edits), ptr(cands) if max_candidates else None, ptr(rows) if max_candidates else None,
                                         int(max_candidates), None if null_removed or not max_candidates else ptr(rem),
                                         None if null_info else ptr(info))
        ok = rc == 0
        ne = min(max_edits, int(info[0]["n_edits"])) if ok else max_edits
        nc = min(max_candidates, int(info[0]["n_candidates"])) if ok else max_candidates
        return (idx[:n].copy(), actions[:n].copy(), edits[:ne].copy(), cands[:nc].copy(), rows[:nc].copy(), rem[:nc].copy(), info[0].copy(), rc)

    # ---- pod-axis shard mode (include/mmplace.h "pod-axis sharding"; orchestrated by dist.py) ----
    def shard_configure(self, shard: int, n_shards: int):
        self._ck(self.lib.mmp_shard_configure(self.h, int(shard), int(n_shards)))
        self.shard, self.n_shards = int(shard), int(n_shards)

    def shard_xchg_slots(self, phase: int) -> int:
        return int(self.lib.mmp_shard_xchg_slots(int(phase), int(self.n_shards)))

    def shard_rank_dev(self, d_rank: int):
        self._ck(self.lib.mmp_shard_rank_dev(self.h, C.c_void_p(d_rank)))

    def shard_commit_dev(self, d_rank: int):
        self._ck(self.lib.mmp_shard_commit_dev(self.h, C.c_void_p(d_rank)))

    def shard_phase_dev(self, phase: int, d_reqs: int, n: int, d_extra: int, now: int, d_xchg, d_outs: int,
                        stream: int = 0):
        arr = (C.c_void_p * 6)(*[C.c_void_p(int(x)) for x in d_xchg])
        self._ck(self.lib.mmp_shard_place_phase_dev(self.h, int(phase), C.c_void_p(d_reqs), int(n),
                                                    C.c_void_p(d_extra or None), int(now), arr,
                                                    C.c_void_p(d_outs or None), C.c_void_p(stream or None)))

    def shard_fast_slots(self) -> int:
        return int(self.lib.mmp_shard_fast_slots())

    def shard_fast_dev(self, d_reqs: int, n: int, d_extra: int, now: int, d_xf: int, stream: int = 0):
        self._ck(self.lib.mmp_shard_place_fast_dev(self.h, C.c_void_p(d_reqs), int(n), C.c_void_p(d_extra or None), int(now),
                                                   C.c_void_p(d_xf), C.c_void_p(stream or None)))

    def shard_fast_finish_dev(self, d_reqs: int, n: int, d_xf: int, d_outs: int, stream: int = 0):
        """-> (n_rest, device pointer of the compacted requests, device pointer of their result rows)"""
        n_rest, rr, ro = C.c_int32(0), C.c_void_p(0), C.c_void_p(0)
        self._ck(self.lib.mmp_shard_place_fast_finish_dev(self.h, C.c_void_p(d_reqs), int(n), C.c_void_p(d_xf),
                                                          C.c_void_p(d_outs), C.c_void_p(stream or None), C.byref(n_rest),
                                                          C.byref(rr), C.byref(ro)))
        return n_rest.value, rr.value or 0, ro.value or 0

    def shard_fast_scatter_dev(self, n_rest: int, d_outs: int, stream: int = 0):
        self._ck(self.lib.mmp_shard_place_fast_scatter_dev(self.h, int(n_rest), C.c_void_p(d_outs), C.c_void_p(stream or None)))

    # ---- the pod-axis group with RCCL inside the library (include/mmplace.h) ----
    def shard_unique_id(self) -> bytes:
        buf = C.create_string_buffer(128)
        self._ck(self.lib.mmp_shard_unique_id(buf))
        return buf.raw

    def shard_group_init(self, unique_id: bytes | None, rank: int, world: int):
        buf = C.create_string_buffer(unique_id, 128) if unique_id is not None else None
        self._ck(self.lib.mmp_shard_group_init(self.h, buf, int(rank), int(world)))
        self.n_shards = int(world)

    def shard_group_destroy(self):
        self._ck(self.lib.mmp_shard_group_destroy(self.h))

    def shard_commit(self):
        self._ck(self.lib.mmp_shard_commit(self.h))

    def shard_place(self, reqs, extra, now: int):
        """Collective over the group, host pointers -> (outs, n_rest)."""
        reqs = np.ascontiguousarray(reqs, dtype=PLACE_REQ)
        extra = np.ascontiguousarray(extra if extra is not None else np.zeros(0, np.int32), dtype=np.int32)
        outs = np.zeros(len(reqs), dtype=PLACE_OUT)
        n_rest = C.c_int32(0)
        self._ck(self.lib.mmp_shard_place_batch(self.h, ptr(reqs), len(reqs), ptr(extra) if len(extra) else None, len(extra),
                                                int(now), ptr(outs), C.byref(n_rest)))
        return outs, n_rest.value

    def shard_place_dev(self, d_reqs: int, n: int, d_extra: int, now: int, d_outs: int) -> int:
        """Collective over the group, device pointers; returns when d_outs is complete -> n_rest."""
        n_rest = C.c_int32(0)
        self._ck(self.lib.mmp_shard_place_batch_dev(self.h, C.c_void_p(d_reqs), int(n), C.c_void_p(d_extra or None), int(now),
                                                    C.c_void_p(d_outs), C.byref(n_rest)))
        return n_rest.value

    def shard_place_async_dev(self, d_reqs: int, n: int, d_extra: int, now: int, d_outs: int):
        """The same without the synchronisation at the end: completed by the next group call or by shard_wait()."""
        self._ck(self.lib.mmp_shard_place_batch_async_dev(self.h, C.c_void_p(d_reqs), int(n), C.c_void_p(d_extra or None), int(now),
                                                          C.c_void_p(d_outs)))

    def shard_wait(self) -> int:
        n_rest = C.c_int32(0)
        self._ck(self.lib.mmp_shard_wait(self.h, C.byref(n_rest)))
        return n_rest.value

    def sync(self):
        self._ck(self.lib.mmp_sync(self.h))

    def profile(self, enable: bool = True):
        """HIP-event timing of the kernels inside each host-pointer call (read with last_kernel_ms())."""
        self._ck(self.lib.mmp_profile(self.h, 1 if enable else 0))

    def last_kernel_ms(self) -> float:
        return float(self.lib.mmp_last_kernel_ms(self.h))
