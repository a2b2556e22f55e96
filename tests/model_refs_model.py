"""mmp_models_refs_json as a plain sequential program over bytes: the oracle of the device path (tests/test_models_refs_gpu.py),
pinned by tests/test_model_refs_model.py.  Every step cites the Java it restates (VModelManager.java updateVModel :137-385,
decModelRefsInTxn :475-489; ModelRecord.java).

A request is (flags, last_used) with flags INC = 1 / AUTO_DELETE = 2, its info (type, encKey, mPath) as bytes with b"" for null,
and the stored value `old`, b"" for mr == null.  The member walk below is the model's own and trusts the value to be well-formed
JSON: the parser's verdict (tests/ingest_model.py) is settled first.  No `json` renders or reads here.
"""
import re

from tests.ingest_model import REJECT, UNSPECIFIED, model_class

INC, AUTO_DELETE = 1, 2
SET, CREATED, DELETE, ENSURE_ABSENT, NOT_FOUND, MALFORMED, HOST = range(7)
CLASSES = tuple(range(7))
RENDERED = (SET, CREATED)
_WS = b" \t\n\r"
_INT = re.compile(rb"-?[0-9]+")
_QUOTE, _BACKSLASH = 0x22, 0x5C


def jint(x):
    """Java int arithmetic: the value wrapped into [-2^31, 2^31)."""
    return ((int(x) + (1 << 31)) & ((1 << 32) - 1)) - (1 << 31)


def _b(s):
    return s if isinstance(s, bytes) else s.encode()


def _blank(v, p):
    while p < len(v) and v[p] in _WS:
        p += 1
    return p


def _behind_string(v, p):
    """v[p] opens a string -> the index behind its closing quote."""
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
    """The top-level members of the object v in document order: [(raw name, the member's bytes from the opening quote of its key
    to the last byte of its value, the value's bytes)]."""
    out = []
    p = _blank(v, _blank(v, 0) + 1)  # behind '{'
    while v[p] != 0x7D:
        if v[p] == 0x2C:
            p = _blank(v, p + 1)
        key_end = _behind_string(v, p)
        colon = _blank(v, key_end)
        assert v[colon] == 0x3A
        vs = _blank(v, colon + 1)
        ve = _behind_value(v, vs)
        out.append((bytes(v[p + 1:key_end - 1]), bytes(v[p:ve]), bytes(v[vs:ve])))
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


def _render(parts):
    return b"{" + b",".join(parts) + b"}"


def refs_step(flags, last_used, info, old, strict=True):
    """-> (value or None, class, the count the Java method returns).  Raises ValueError for an old value of the class the parsers
    leave unspecified (strict=False takes it as well-formed)."""
    typ, enc, path = (_b(x) if x is not None else b"" for x in (info or (b"", b"", b"")))
    old = _b(old)
    inc = bool(flags & INC)
    if not old:  # mr == null
        if not inc:
            return None, ENSURE_ABSENT, 0  # :485-487 else if (modelId != null) txn.ensureAbsent(registry, modelId)
        if not typ:
            return None, NOT_FOUND, 0  # :203-205 modelInfo == null && targetModel == null: "Target model ... not found"
        # :294 new ModelRecord(type, key, path, autoDelete); :301 setLastUsed; :302 incRefCount — as Jackson writes it: the
        # declaration order of ModelRecord.java:61-114, a member at its default omitted
        parts = [b'"type":"%s"' % escape(typ)]
        if enc:
            parts.append(b'"encKey":"%s"' % escape(enc))
        if path:
            parts.append(b'"mPath":"%s"' % escape(path))
        parts.append(b'"refs":1')
        if flags & AUTO_DELETE:
            parts.append(b'"autoDel":true')
        if last_used:
            parts.append(b'"lu":%d' % last_used)
        return _render(parts), CREATED, 1
    cls = model_class(old)
    if cls == UNSPECIFIED and strict:
        raise ValueError("unspecified: %r" % (old[:80],))
    if cls == REJECT:
        return None, MALFORMED, 0
    top = members(old)
    last = {}
    for name, _span, val in top:  # a later duplicate wins
        last[name] = val
    raw = last.get(b"refs")
    if raw is None:
        refs = 0  # the bean's default
    elif not _INT.fullmatch(raw) or not -(1 << 31) <= int(raw) < (1 << 31):
        return None, HOST, 0
    else:
        refs = int(raw)
    if inc:
        field = ret = jint(refs + 1)  # ModelRecord.java:221 return ++refCount
        owned = (b"refs", b"lu")      # :301 setLastUsed sets unconditionally
    else:
        auto = last.get(b"autoDel", b"false")
        if auto not in (b"true", b"false"):
            return None, HOST, 0
        field = refs - 1 if refs > 0 else refs  # ModelRecord.java:214 refCount > 0 ? --refCount : 0 — the field moves only above 0
        ret = refs - 1 if refs > 0 else 0
        if ret == 0 and auto == b"true":
            return None, DELETE, 0  # :478-480 txn.delete(registry, modelId, mr)
        owned = (b"refs",)
    parts = [span for name, span, _val in top if name not in owned]
    if field:
        parts.append(b'"refs":%d' % field)
    if inc and last_used:
        parts.append(b'"lu":%d' % last_used)
    return _render(parts), SET, ret  # :482 txn.set(registry, modelId, mr) / :304 .set(registry, targetModelId, targetModel)


def refs_batch(reqs, infos, olds):
    """The call: reqs = [(flags, last_used)], infos None or [(type, encKey, mPath)].  -> ([bytes or None], [class], [count])."""
    vals, classes, counts = [], [], []
    for k, ((flags, lu), old) in enumerate(zip(reqs, olds)):
        v, c, r = refs_step(int(flags), int(lu), None if infos is None else infos[k], old)
        vals.append(v)
        classes.append(c)
        counts.append(r)
    return vals, classes, counts
