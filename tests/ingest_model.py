"""What a stored InstanceRecord / ModelRecord value means to the two beans, stated in plain Python: the single oracle of the
wire-format parsers (modelmesh_amd/csrc/ingest_kernels.hpp).  Built on json.loads with an object_pairs_hook, so that every
occurrence of a field is seen and a later duplicate wins, as with Jackson.

Every value belongs to one of three classes:

  ACCEPT       json.loads succeeds, the top level is an object, every occurrence of a known field holds its type (longs fit
               int64, the int fields int32; `type` is a string or null; instanceIds / failedIn are null or string -> long).
  REJECT       status 1, the row untouched: empty or blank, not an object, truncated, unbalanced nesting or strings, bytes other
               than blanks behind the closing brace, a known field or a map entry of the wrong type, missing / doubled /
               trailing separators.  For a value json.loads refuses this is decided on the value with its SKIPPED field values
               (unknown fields; loc, zone, labels, fails, ...) replaced by null: if it is still refused, it must be rejected.
  UNSPECIFIED  what the two device parsers need not agree on, and no corpus may contain: a value that is invalid only inside a
               skipped value ({"x": 1 2}); leading zeros; integers outside int64 / int32; a `type` that is neither a string nor
               null; a backslash escape in the name of a known field, in a key of an id map or in the type string (the parsers
               hash raw bytes, Jackson decodes).

An id map is an entry LIST here, as in the packed row: every entry in document order, a repeated key included (the TreeMap of
the bean would keep the last; the stores never write one).
"""
import json
import re
from collections import namedtuple

ACCEPT, REJECT, UNSPECIFIED = "must accept", "must reject", "unspecified"
WS = " \t\n\r"
I64 = (-(1 << 63), (1 << 63) - 1)
I32 = (-(1 << 31), (1 << 31) - 1)

MODEL_FIELDS = {"type": "type", "lu": "long", "lul": "long", "instanceIds": "map", "failedIn": "map"}
POD_FIELDS = {"lruTime": "long", "count": "int", "cap": "long", "used": "long", "lThreads": "int", "lInProg": "int", "rpm": "int",
              "shutdown": "bool", "startTime": "long", "vers": "long"}  # in the order pod_bean returns them

ModelBean = namedtuple("ModelBean", "status type lu lul loaded failed")


class Pairs(list):
    """A JSON object as its (key, value) pairs in document order, duplicates kept."""


def _no_constant(name):
    raise ValueError("not JSON: " + name)


def _loads(text):
    return json.loads(text, object_pairs_hook=Pairs, parse_constant=_no_constant)


def _raw(text):
    """The same document with every backslash escape made inert, so that its strings come out of json.loads as their raw bytes
    (private-use characters stand for the backslash and for an escaped quote or backslash)."""
    return re.sub(r"\\(.)", lambda m: "\ue000" + {'"': "\ue001", "\\": "\ue002"}.get(m.group(1), m.group(1)), text, flags=re.S)


_STRING = re.compile(r'"(?:[^"\\]|\\.)*"', re.S)
_LEADING_ZEROS = re.compile(r'(?<![0-9.eE+\-"\w])(-?)0+(?=\d)')


def _segments(text):
    """The members of the outer object as (text, position of the first ':' directly inside the object or None); None when the
    value is not one object closed exactly by its last non-blank byte with every string and container balanced."""
    s = text.strip(WS)
    if not s or s[0] != "{":
        return None
    depth, in_str, i, start, colon, segs = 0, False, 0, 1, None, []
    while i < len(s):
        ch = s[i]
        if in_str:
            if ch == "\\":
                i += 2
                continue
            in_str = ch != '"'
        elif ch == '"':
            in_str = True
        elif ch in "{[":
            depth += 1
        elif ch in "}]":
            depth -= 1
            if depth == 0:
                if i != len(s) - 1:
                    return None
                segs.append((s[start:i], colon))
        elif ch == "," and depth == 1:
            segs.append((s[start:i], colon))
            start, colon = i + 1, None
        elif ch == ":" and depth == 1 and colon is None:
            colon = i - start
        i += 1
    if in_str or depth != 0:
        return None
    if len(segs) == 1 and not segs[0][0].strip(WS):
        return []
    return segs


def _refused(text, fields):
    """The class of a value json.loads refuses."""
    segs = _segments(text)
    if segs is None:
        return REJECT
    kept = []
    for k, (seg, colon) in enumerate(segs):
        key = seg[:colon].strip(WS) if colon is not None else ""
        if not _STRING.fullmatch(key):
            kept.append(seg)  # no ':' or no string in front of it: nothing to skip here
            continue
        try:
            name = json.loads(key)
        except ValueError:
            name = None
        known = fields.get(key[1:-1]) or fields.get(name)
        if known == "type" and seg[colon + 1:].lstrip(WS)[:1] != '"':
            known = None  # a type that is not a string is skipped by both parsers
        kept.append(seg if known else '"skipped%d":null' % k)
    for strip_zeros in (False, True):
        doc = "{" + ",".join(_LEADING_ZEROS.sub(r"\1", seg) if strip_zeros else seg for seg in kept) + "}"
        try:
            _loads(doc)
            return UNSPECIFIED
        except ValueError:
            pass
    return REJECT


def _in(v, rng):
    return rng[0] <= v <= rng[1]


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _classify(value, fields):
    """-> (class, {field: value of its last occurrence}); map values come as Pairs."""
    # (bytes that are not UTF-8 — a value cut inside a character — stay what they are: the parsers do not decode)
    text = value.decode("utf-8", "surrogateescape") if isinstance(value, bytes) else value
    try:
        doc = _loads(text)
    except ValueError:
        return _refused(text, fields), None
    if not isinstance(doc, Pairs):
        return REJECT, None
    raw = _loads(_raw(text))
    verdicts, last = set(), {}
    for (k, v), (rk, rv) in zip(doc, raw):
        kind = fields.get(k)
        if kind is None:
            continue
        if rk != k:
            verdicts.add(UNSPECIFIED)
        last[k] = v
        if kind in ("long", "int"):
            if not _is_int(v):
                verdicts.add(REJECT)
            elif not _in(v, I64 if kind == "long" else I32):
                verdicts.add(UNSPECIFIED)
        elif kind == "bool":
            if not isinstance(v, bool):
                verdicts.add(REJECT)
        elif kind == "type":
            if not (v is None or (isinstance(v, str) and rv == v)):
                verdicts.add(UNSPECIFIED)
        elif v is not None:  # an id -> long map
            if not isinstance(v, Pairs):
                verdicts.add(REJECT)
                continue
            if [ek for ek, _ in v] != [ek for ek, _ in rv]:
                verdicts.add(UNSPECIFIED)
            for _, t in v:
                if not _is_int(t):
                    verdicts.add(REJECT)
                elif not _in(t, I64):
                    verdicts.add(UNSPECIFIED)
    if REJECT in verdicts:
        return REJECT, None
    if UNSPECIFIED in verdicts:
        return UNSPECIFIED, None
    return ACCEPT, last


def model_class(value):
    return _classify(value, MODEL_FIELDS)[0]


def pod_class(value):
    return _classify(value, POD_FIELDS)[0]


def model_bean(value, ids, type_names, unknown_type):
    """-> ModelBean(status, type, lu, lul, loaded, failed): loaded / failed are [(pod, time), ...] in document order, an id that
    is not in `ids` is pod -1; a missing or null type is "NLCLASSIFIER" (the unknown type if no such name is loaded), a type name
    that is not in `type_names` is `unknown_type`.  A rejected value is (1, None, 0, 0, [], []).  Raises ValueError for a value
    of the UNSPECIFIED class."""
    cls, d = _classify(value, MODEL_FIELDS)
    if cls == UNSPECIFIED:
        raise ValueError("unspecified: %r" % (value[:80],))
    if cls == REJECT:
        return ModelBean(1, None, 0, 0, [], [])
    pod_of = ids if isinstance(ids, dict) else {s: i for i, s in enumerate(ids)}
    names = list(type_names)
    default = names.index("NLCLASSIFIER") if "NLCLASSIFIER" in names else unknown_type
    t = d.get("type")
    ty = default if t is None else (names.index(t) if t in names else unknown_type)
    maps = [[(pod_of.get(k, -1), t) for k, t in (d.get(f) or ())] for f in ("instanceIds", "failedIn")]
    return ModelBean(0, ty, d.get("lu", 0), d.get("lul", 0), maps[0], maps[1])


def pod_bean(value):
    """-> (status, (lruTime, count, cap, used, lThreads, lInProg, rpm, shutdown, startTime, vers)); a field Jackson omits is
    0 / False.  A rejected value is (1, None).  Raises ValueError for a value of the UNSPECIFIED class."""
    cls, d = _classify(value, POD_FIELDS)
    if cls == UNSPECIFIED:
        raise ValueError("unspecified: %r" % (value[:80],))
    if cls == REJECT:
        return 1, None
    return 0, tuple(d.get(f, False if kind == "bool" else 0) for f, kind in POD_FIELDS.items())
