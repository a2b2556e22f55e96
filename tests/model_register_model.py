"""mmp_models_register_json as a plain sequential program over bytes: the oracle of the device path
(tests/test_models_register_gpu.py), pinned by tests/test_model_register_model.py.  Every step cites the Java it restates
(ModelMesh.java registerModel :3088-3147, deleteModel :3181-3203; ModelRecord.java).

A request is (flags, initial_cache_timestamp) with flags LOAD_NOW = 1 / DELETE = 2, its info (type, encKey, mPath) as bytes with
b"" for null (the Java maps "" to null before it compares, :3094-3095), and the stored value `old`, b"" for registry.get() == null.
The member walk below is the model's own and trusts the value to be well-formed JSON: the parser's verdict (tests/ingest_model.py)
is settled first.  No `json` renders or reads here.
"""
import re

from tests.ingest_model import REJECT, UNSPECIFIED, model_class

LOAD_NOW, DELETE = 1, 2
CREATED, TOUCHED, EXISTS, CONFLICT, ABSENT, REFERENCED, DELETABLE, MALFORMED, HOST = range(9)
CLASSES = tuple(range(9))
DEFAULT_TYPE = b"NLCLASSIFIER"  # ModelRecord.java:130
WS = b" \t\n\r"
EQUAL, UNEQUAL, UNDECIDED = 0, 1, 2
_INT = re.compile(rb"-?[0-9]+")


def jlong(x):
    """Java long arithmetic: the value wrapped into [-2^63, 2^63)."""
    return ((int(x) + (1 << 63)) & ((1 << 64) - 1)) - (1 << 63)


def _b(s):
    return s if isinstance(s, bytes) else s.encode()


def _skip_ws(v, p):
    while p < len(v) and v[p] in WS:
        p += 1
    return p


def _string_end(v, p):
    """v[p] is an opening quote -> the index behind the closing one (a backslash takes the byte behind it along)."""
    p += 1
    while v[p] != 0x22:
        p += 2 if v[p] == 0x5C else 1
    return p + 1


def _value_end(v, p):
    if v[p] == 0x22:
        return _string_end(v, p)
    if v[p] in b"{[":
        depth = 0
        while True:
            if v[p] == 0x22:
                p = _string_end(v, p)
                continue
            if v[p] in b"{[":
                depth += 1
            elif v[p] in b"}]":
                depth -= 1
                if depth == 0:
                    return p + 1
            p += 1
    while v[p] not in b",}] \t\n\r":
        p += 1
    return p


def top_members(v):
    """The top-level members of the object v in document order: [(raw name, index of the key's opening quote, value bytes,
    index behind the value)]."""
    out = []
    p = _skip_ws(v, _skip_ws(v, 0) + 1)
    while v[p] != 0x7D:
        if v[p] == 0x2C:
            p = _skip_ws(v, p + 1)
        ko = p
        ke = _string_end(v, p)
        p = _skip_ws(v, ke)
        assert v[p] == 0x3A
        vs = _skip_ws(v, p + 1)
        ve = _value_end(v, vs)
        out.append((bytes(v[ko + 1:ke - 1]), ko, bytes(v[vs:ve]), ve))
        p = _skip_ws(v, ve)
    return out


def escape(s):
    """The rule of mmp_models_rewrite_json: '"' and '\\' behind a backslash, below 0x20 as \\u00xx, the rest verbatim."""
    out = bytearray()
    for c in s:
        if c in (0x22, 0x5C):
            out += bytes((0x5C, c))
        elif c < 0x20:
            out += b"\\u00%02x" % c
        else:
            out.append(c)
    return bytes(out)


def last_used_timestamp(flags, ict, now, age):
    """:3098-3101."""
    if ict >= now:
        return now
    if ict > 0:
        return ict
    return jlong(now - jlong(age * (1 if flags & LOAD_NOW else 6)))


def _attr(stored, asked, is_type):
    """One side of :3111-3113: the deciding occurrence's value bytes (None: no such member) against the request's bytes."""
    if stored is None or stored == b"null":
        if is_type:
            return EQUAL if asked == DEFAULT_TYPE else UNEQUAL  # ModelRecord.java:122: null reads as the default type
        return EQUAL if asked == b"" else UNEQUAL  # Objects.equals(null, null)
    if stored[:1] != b'"':
        return UNDECIDED  # neither a string nor null
    text = stored[1:-1]
    if b"\\" in text:
        return UNDECIDED  # the device compares raw bytes and Jackson would decode
    if not is_type and asked == b"":
        return UNEQUAL  # a stored "" is a string, the request's is null
    return EQUAL if text == asked else UNEQUAL


def register(flags, ict, info, old, now, age, strict=True):
    """-> (value or None, class, last_used).  Raises ValueError for an old value of the class the parsers leave unspecified
    (strict=False takes it as well-formed)."""
    typ, enc, path = (_b(x) if x is not None else b"" for x in info)
    old = _b(old)
    delete = bool(flags & DELETE)
    ts = 0 if delete else last_used_timestamp(flags, ict, now, age)
    if not old:  # registry.get(modelId) == null
        if delete:
            return None, ABSENT, 0  # :3187 while (mr != null): fine if not found
        # :3135-3137 new ModelRecord(type, encKey, mPath, false); setLastUsed(ts) — as Jackson writes it: the declaration order of
        # ModelRecord.java:61-114, a member at its default omitted
        parts = [b'"type":"%s"' % escape(typ)]
        if enc:
            parts.append(b'"encKey":"%s"' % escape(enc))
        if path:
            parts.append(b'"mPath":"%s"' % escape(path))
        if ts:
            parts.append(b'"lu":%d' % ts)
        return b"{" + b",".join(parts) + b"}", CREATED, ts
    cls = model_class(old)
    if cls == UNSPECIFIED and strict:
        raise ValueError("unspecified: %r" % (old[:80],))
    if cls == REJECT:
        return None, MALFORMED, ts
    top = top_members(old)
    last = {}
    for name, _ko, val, _ve in top:  # a later duplicate wins
        last[name] = val
    if delete:
        refs = last.get(b"refs")
        if refs is None:
            n = 0  # the bean's default
        elif not _INT.fullmatch(refs) or not -(1 << 31) <= int(refs) < (1 << 31):
            return None, HOST, 0
        else:
            n = int(refs)
        return None, (REFERENCED if n > 0 else DELETABLE), 0  # :3188-3191 getRefCount() > 0 / :3198 conditionalDelete
    verdicts = (_attr(last.get(b"type"), typ, True),      # :3111 !mr.getType().equals(type)
                _attr(last.get(b"encKey"), enc, False),   # :3112 !Objects.equals(mr.getEncryptionKey(), modelInfo.getEncKey())
                _attr(last.get(b"mPath"), path, False))   # :3113 !Objects.equals(mr.getModelPath(), modelInfo.getModelPath())
    if UNDECIDED in verdicts:
        return None, HOST, ts
    if UNEQUAL in verdicts:
        return None, CONFLICT, ts  # :3117 "Model already exists with different attribute values"
    lu = int(last.get(b"lu", b"0"))
    if flags & LOAD_NOW or not ts > jlong(lu + age):  # :3120 !loadNow && lastUsedTimestamp > mr.getLastUsed() + LASTUSED_AGE_ON_ADD_MS
        return None, EXISTS, ts  # :3129 weCreated = false, no compare-and-set
    t = now if ts == 0 else ts  # ModelRecord.java:240-242: 0 means "now"
    lu2 = t if t > lu else lu   # :243-245: only raised
    parts = [old[ko:ve] for name, ko, _val, ve in top if name != b"lu"]
    if lu2:
        parts.append(b'"lu":%d' % lu2)
    return b"{" + b",".join(parts) + b"}", TOUCHED, ts  # :3123 conditionalSetAndGet(modelId, mr), whether or not lu moved


def register_batch(reqs, infos, olds, now, age):
    """The call: reqs = [(flags, ict)].  -> ([bytes or None], [class], [last_used])."""
    vals, classes, lus = [], [], []
    for (flags, ict), info, old in zip(reqs, infos, olds):
        v, c, t = register(int(flags), int(ict), info, old, now, age)
        vals.append(v)
        classes.append(c)
        lus.append(t)
    return vals, classes, lus
