"""mmp_vmodels_write_json as a plain sequential program over bytes: the oracle of the device path
(tests/test_vmodels_write_gpu.py), pinned by tests/test_vmodel_write_model.py.  Every step cites the Java it restates
(VModelManager.java = VMM: updateVModel :137-385, deleteVModel :416-470, PendingTransition.run :716-767).

A request is (op, flags, (id_a, id_b, owner)) with b"" / None for Java null, on the stored value `old`, b"" for vmr == null.  The
verdict on a stored value is the read side's (tests/vmodel_model.py classify: status 1 = MALFORMED); the member walk below is the
model's own and trusts the value to be well-formed JSON.  The registry is tests/vmodel_model.py's Registry: ids in row order and per
row (n_loaded, n_failed, last_used, type), the empty row all zero.  No `json` renders or reads here.
"""
from collections import namedtuple

from tests import vmodel_model as vm
from tests.ingest_model import REJECT, UNSPECIFIED

SET, DELETE, COMPLETE, FAIL_FLAG = range(4)
OPS = (SET, DELETE, COMPLETE, FAIL_FLAG)
UPDATE_ONLY, FORCE, LOAD_NOW, TARGET_EXISTS, TARGET_LOADED, TARGET_NOT_LOADED, FAILED = 1, 2, 4, 8, 16, 32, 64
REQ_FLAGS = (UPDATE_ONLY, FORCE, LOAD_NOW, TARGET_EXISTS, TARGET_LOADED, TARGET_NOT_LOADED, FAILED)
(CREATED, UPDATED, UNCHANGED, NOT_FOUND, PRECONDITION, OWNER_MISMATCH, NEEDS_TARGET_STATUS, NOOP, DELETED, CHANGED, MALFORMED,
 HOST) = range(12)
CLASSES = tuple(range(12))
RENDERED = (CREATED, UPDATED)
IN_TRANSITION, ACTIVE_SWITCHED, PREV_ACTIVE_UNKNOWN = 1, 2, 4
ROW_FLAGS = (IN_TRANSITION, ACTIVE_SWITCHED, PREV_ACTIVE_UNKNOWN)
Row = namedtuple("Row", "cls flags model target_copy_count dec_model dec_off dec_len last_used")
_WS = b" \t\n\r"
_QUOTE, _BACKSLASH = 0x22, 0x5C
_OWNED = (b"amid", b"tmid", b"failed")


def jlong(x):
    """Java long arithmetic: the value wrapped into [-2^63, 2^63)."""
    return ((int(x) + (1 << 63)) & ((1 << 64) - 1)) - (1 << 63)


def _b(s):
    if s is None:
        return b""
    return s if isinstance(s, bytes) else s.encode()


def _blank(v, p):
    while p < len(v) and v[p] in _WS:
        p += 1
    return p


def _behind_string(v, p):
    p += 1
    while v[p] != _QUOTE:
        p += 2 if v[p] == _BACKSLASH else 1
    return p + 1


def _behind_value(v, p):
    if v[p] == _QUOTE:
        return _behind_string(v, p)
    if v[p] in b"{[":
        depth = 0
        while True:
            c = v[p]
            if c == _QUOTE:
                p = _behind_string(v, p)
                continue
            depth += (c in b"{[") - (c in b"}]")
            p += 1
            if depth == 0:
                return p
    while v[p] not in b",}] \t\n\r":
        p += 1
    return p


def members(v):
    """The top-level members of the object v in document order: [(raw name, index of the key's opening quote, index of the value's
    first byte, index behind the value)]."""
    out = []
    p = _blank(v, _blank(v, 0) + 1)
    while v[p] != 0x7D:
        if v[p] == 0x2C:
            p = _blank(v, p + 1)
        key_end = _behind_string(v, p)
        colon = _blank(v, key_end)
        assert v[colon] == 0x3A
        vs = _blank(v, colon + 1)
        ve = _behind_value(v, vs)
        out.append((bytes(v[p + 1:key_end - 1]), p, vs, ve))
        p = _blank(v, ve)
    return out


def escape(s):
    """The rule of mmp_models_rewrite_json: '"' and '\\' behind a backslash, below 0x20 as \\u00xx, the rest verbatim."""
    out = bytearray()
    for c in s:
        if c in (_QUOTE, _BACKSLASH):
            out += bytes((_BACKSLASH, c))
        elif c < 0x20:
            out += b"\\u00%02x" % c
        else:
            out.append(c)
    return bytes(out)


class _Str(namedtuple("_Str", "raw pos")):
    """A stored string: the raw bytes between its quotes and where they start in the value."""


def _stored(old, top, name):
    """The deciding (last) occurrence of a string member: a _Str, or None for absent / null."""
    for n, _ko, vs, ve in reversed(top):
        if n == name:
            return _Str(old[vs + 1:ve - 1], vs + 1) if old[vs] == _QUOTE else None
    return None


def _raw_of(s):
    return None if s is None else s.raw


def _prev_active(reg, mid):
    """registry.getOrStrongIfAbsent(prevActiveId) as the device holds it -> (copies, last_used, known)."""
    m = reg.row(mid)
    if m < 0 or reg.empty(m):
        return 0, 0, False
    n_loaded, _nf, lu, _t = reg.recs[m]
    return n_loaded, lu, True


def write_step(op, flags, strs, old, reg, now, age, default_owner=b"", strict=True):
    """-> (value or None, Row).  Raises ValueError for an old value of the class the parsers leave unspecified."""
    ida, idb, owner = (_b(x) for x in strs)
    old = _b(old)
    cls, flg, model, count, last_used = None, 0, -1, 0, 0
    dec = [None, None]

    def row(c):
        return Row(c, flg, model, count, tuple(reg.row(d.raw) if d else -1 for d in dec), tuple(d.pos if d else 0 for d in dec),
                   tuple(len(d.raw) if d else -1 for d in dec), last_used)

    am = tm = so = None
    failed = False
    top = []
    if old:
        verdict, _ = vm.classify(old)
        if verdict == UNSPECIFIED and strict:
            raise ValueError("unspecified: %r" % (old[:80],))
        if verdict == REJECT:
            return None, row(MALFORMED)
        top = members(old)
        am, tm, so = (_stored(old, top, n) for n in (b"amid", b"tmid", b"o"))
        for n, _ko, vs, ve in top:
            if n == b"failed":
                failed = old[vs:ve] == b"true"
        reads = [am, tm] + ([so] if op in (SET, DELETE) and owner else [])
        if op != FAIL_FLAG and any(s is not None and b"\\" in s.raw for s in reads):
            return None, row(HOST)  # the device compares raw bytes and Jackson would decode
    a, t, o = _raw_of(am), _raw_of(tm), _raw_of(so)
    new_a, new_t, new_failed = (a, False), (t, False), failed  # (bytes, from the request)

    if op == SET:
        ict = jlong(now - jlong(age * (1 if flags & LOAD_NOW else 6)))  # VMM:168-170
        force = bool(flags & FORCE)
        if not old:
            if idb and idb != ida:
                return None, row(PRECONDITION)  # VMM:178 (in front of the loop), :280
            if flags & UPDATE_ONLY:
                return None, row(NOT_FOUND)  # VMM:277
            own = owner or _b(default_owner)  # VMM:282 owner != null ? owner : DEFAULT_OWNER
            parts = ([b'"o":"%s"' % escape(own)] if own else []) + [b'"amid":"%s"' % escape(ida), b'"tmid":"%s"' % escape(ida)]
            model, last_used = reg.row(ida), ict
            return b"{" + b",".join(parts) + b"}", row(CREATED)
        if owner and o != owner:
            return None, row(OWNER_MISMATCH)  # VMM:181, :222
        tmatch, amatch = t == ida, a == ida  # VMM:229-230 (a stored null equals nothing)
        if not tmatch and idb and idb != t:
            return None, row(PRECONDITION)  # VMM:184, :232
        model = reg.row(ida)
        if tmatch and (amatch or not force):
            if not amatch and a is not None:  # VMM:246-249
                count, _lu, known = _prev_active(reg, a)
                flg |= 0 if known else PREV_ACTIVE_UNKNOWN
            flg |= IN_TRANSITION if a != t else 0  # VMM:344, as stored
            return None, row(UNCHANGED)  # VMM:243, :250
        prev_lu = 0
        if not tmatch:
            new_t = (ida, True)  # VMM:236
            if t is not None and t != a:
                dec[0] = tm  # VMM:237-239
        if not amatch:
            if a is None:
                new_a = (ida, True)  # VMM:258
            else:
                count, prev_lu, known = _prev_active(reg, a)  # VMM:260-261
                flg |= 0 if known else PREV_ACTIVE_UNKNOWN
                one = bool(flags & TARGET_EXISTS) and count == 1
                if force or count == 0 or (one and flags & TARGET_LOADED):  # VMM:262-265
                    new_a = (ida, True)  # VMM:268-269
                    dec[1] = am
                    flg |= ACTIVE_SWITCHED
                elif one and not flags & (TARGET_LOADED | TARGET_NOT_LOADED):
                    flg, dec[0] = 0, None
                    return None, row(NEEDS_TARGET_STATUS)  # getStatus(target) is the host's to ask
        new_failed = False  # VMM:273
        last_used = prev_lu if prev_lu > 0 else ict  # VMM:299-300
        cls = UPDATED
    elif op == DELETE:
        if not old or (owner and o != owner):
            return None, row(NOOP)  # VMM:419, :457 absentOrOwnerMismatch
        if a is not None:
            dec[0] = am  # VMM:438
        if t is not None and t != a:
            dec[1] = tm  # VMM:429, :441
        return None, row(DELETED)
    elif op == COMPLETE:
        # VMM:762-763; an empty fromId stands for a stored null amid, where the Java would throw
        if not old or (a != idb if idb else a is not None) or t != ida:
            return None, row(CHANGED)
        new_a, new_failed = (ida, True), False  # VMM:753-754
        if a is not None:
            dec[0] = am  # VMM:756
        cls = UPDATED
    else:  # FAIL_FLAG, VMM:736-738
        want = bool(flags & FAILED)
        if not old:
            return None, row(NOOP)  # VMM:726
        if want == failed:
            flg |= IN_TRANSITION if a != t else 0
            return None, row(UNCHANGED)
        new_failed = want
        cls = UPDATED
    flg |= IN_TRANSITION if new_a[0] != new_t[0] else 0  # VModelRecord.inTransition() after the step
    parts = [old[ko:ve] for n, ko, _vs, ve in top if n not in _OWNED]
    for name, (text, from_request) in ((b"amid", new_a), (b"tmid", new_t)):
        if text is not None:
            parts.append(b'"%s":"%s"' % (name, escape(text) if from_request else text))
    if new_failed:
        parts.append(b'"failed":true')
    return b"{" + b",".join(parts) + b"}", row(cls)


def write_batch(reqs, strs, olds, reg, now, age, default_owner=b""):
    """The call: reqs = [(op, flags)].  -> ([bytes or None], [Row])."""
    vals, rows = [], []
    for (op, flags), s, old in zip(reqs, strs, olds):
        v, r = write_step(int(op), int(flags), s, old, reg, now, age, default_owner)
        vals.append(v)
        rows.append(r)
    return vals, rows
