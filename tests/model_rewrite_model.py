"""mmp_models_rewrite_json as a plain sequential program over bytes: the oracle of the device path
(tests/test_models_rewrite_gpu.py), pinned by tests/test_model_rewrite_model.py.  The rule, as include/mmplace.h states it:

  new value    '{' kept members ',' owned members '}', joined by single commas, no other whitespace
  owned names  instanceIds, failedIn, fails, lu — and lul when a last_unload is given
  kept         every top-level member of the old value whose RAW name (the bytes between its quotes: an escaped spelling of an
               owned name is some other member) is not owned, in document order, duplicates included, from the opening quote of
               its key to the last byte of its value
  owned        in this order, each omitted at the bean's default:
                 "instanceIds":{"<id>":<time>,...}   the record's loaded entries in their order
                 "failedIn":{...}                    the failed entries likewise
                 "fails":{...}                       of the LAST top-level `fails` member that is an object: the members whose raw
                                                     key is the id of a failed entry, verbatim and in order; minus those keyed by
                                                     the id of fail_pod; plus "<id>":{"msg":"<escaped>"} when fail_pod is in the
                                                     failed list and its message is not empty
                 "lu":<last_used>   "lul":<last_unload>
  status       1: the old value is one the parser rejects (tests/ingest_model.py); 2: an entry names a pod outside the id list,
               or a rendered id holds '"', '\\', a byte below 0x20 or above 0x7e.  Both: no value.

A record is tests/model_events_model.py's: (type, last_used, loaded, failed), loaded / failed tuples of (pod, time).  The member
walk below is the model's own and trusts the value to be well-formed JSON — the status is settled first; no `json` renders here.
"""
from tests.ingest_model import REJECT, UNSPECIFIED, model_class

OK, MALFORMED, HOST = 0, 1, 2
WS = b" \t\n\r"


def _b(s):
    return s if isinstance(s, bytes) else s.encode()


def _skip_ws(v, p):
    while p < len(v) and v[p] in WS:
        p += 1
    return p


def _string_end(v, p):
    """v[p] is an opening quote -> the index behind the closing one."""
    p += 1
    while v[p] != 0x22:
        p += 2 if v[p] == 0x5C else 1
    return p + 1


def _value_end(v, p):
    """v[p] is the first byte of a value -> the index behind its last byte."""
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


def members(v, p):
    """v[p] is '{' -> [(raw key, key_open, value_start, value_end)] of the object's members in document order."""
    out = []
    p = _skip_ws(v, p + 1)
    while v[p] != 0x7D:
        if v[p] == 0x2C:
            p = _skip_ws(v, p + 1)
        ko = p
        ke = _string_end(v, p)
        p = _skip_ws(v, ke)
        assert v[p] == 0x3A
        vs = _skip_ws(v, p + 1)
        ve = _value_end(v, vs)
        out.append((bytes(v[ko + 1:ke - 1]), ko, vs, ve))
        p = _skip_ws(v, ve)
    return out


def needs_escape(ident):
    return any(c in (0x22, 0x5C) or c < 0x20 or c > 0x7E for c in ident)


def escape(msg):
    out = bytearray()
    for c in msg:
        if c in (0x22, 0x5C):
            out += bytes((0x5C, c))
        elif c < 0x20:
            out += b"\\u00%02x" % c
        else:
            out.append(c)
    return bytes(out)


def _id_map(name, entries, ids):
    return name + b":{" + b",".join(b'"%s":%d' % (ids[p], t) for p, t in entries) + b"}"


def rewrite(old, rec, pod_ids, last_unload=None, fail=None, strict=True):
    """-> (new value or None, status).  old: the stored value (bytes); rec: the record as the registry holds it now; pod_ids: the
    instance ids by pod index; last_unload: None or the lul to write; fail: None or (fail_pod, message) — fail_pod -1: none.
    Raises ValueError for an old value of the class the parsers leave unspecified; strict=False takes such a value as well-formed
    (for the one member of that class this rule does speak about: an escaped spelling of a name)."""
    old = _b(old)
    ids = [_b(s) for s in pod_ids]
    cls = model_class(old)
    if cls == UNSPECIFIED and strict:
        raise ValueError("unspecified: %r" % (old[:80],))
    if cls == REJECT:
        return None, MALFORMED
    _, lu, loaded, failed = rec
    for p, _t in tuple(loaded) + tuple(failed):
        if p < 0 or p >= len(ids) or needs_escape(ids[p]):
            return None, HOST
    owned = {b"instanceIds", b"failedIn", b"fails", b"lu"} | ({b"lul"} if last_unload is not None else set())
    v = old
    top = members(v, _skip_ws(v, 0))
    parts = [v[ko:ve] for key, ko, _vs, ve in top if key not in owned]
    if loaded:
        parts.append(_id_map(b'"instanceIds"', loaded, ids))
    if failed:
        parts.append(_id_map(b'"failedIn"', failed, ids))
    fail_pod, msg = (-1, b"") if fail is None else (int(fail[0]), _b(fail[1]))
    failed_ids = {ids[p] for p, _t in failed}
    fails = []
    objs = [vs for key, _ko, vs, _ve in top if key == b"fails" and v[vs] == 0x7B]
    if objs:
        for key, ko, _vs, ve in members(v, objs[-1]):
            if key in failed_ids and not (fail_pod >= 0 and key == ids[fail_pod]):
                fails.append(v[ko:ve])
    if fail_pod >= 0 and msg and ids[fail_pod] in failed_ids and any(p == fail_pod for p, _t in failed):
        fails.append(b'"%s":{"msg":"%s"}' % (ids[fail_pod], escape(msg)))
    if fails:
        parts.append(b'"fails":{' + b",".join(fails) + b"}")
    if lu:
        parts.append(b'"lu":%d' % lu)
    if last_unload:
        parts.append(b'"lul":%d' % last_unload)
    return b"{" + b",".join(parts) + b"}", OK


def rewrite_batch(olds, recs, rows, pod_ids, last_unload=None, fail=None):
    """The call: value i belongs to registry row rows[i].  -> ([bytes or None], [status])."""
    vals, status = [], []
    for i, old in enumerate(olds):
        f = None if fail is None else (fail[0][i], fail[1][i])
        val, st = rewrite(old, recs[int(rows[i])], pod_ids, None if last_unload is None else int(last_unload[i]), f)
        vals.append(val)
        status.append(st)
    return vals, status
