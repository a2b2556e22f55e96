"""The batches tests/test_models_register_gpu.py sends to mmp_models_register_json, built without a device so that
tests/test_model_register_model.py can assert what each of them holds.  An item is (flags, ict, (type, encKey, mPath), old, key);
every batch of nine requests or more starts with head(): one request of every class."""
from collections import namedtuple

import numpy as np

from tests import ingest_corpus as ic
from tests import model_register_model as mm
from tests.ingest_model import UNSPECIFIED, model_class

NOW = 1_700_000_000_000
AGE = 3_600_000  # lastused_age_on_add_ms of every batch
TILE = 2048
SIZES = (0, 1, 63, 64, 65, 257)
TYPES = (b"NLCLASSIFIER", b"type-1", b"type-2", b"no-such-type")
ESCAPES = b'q" b\\ nl\n tab\t \x01\x1f del\x7f e-acute \xc3\xa9'  # every kind: quote, backslash, below 0x20 — and bytes that stay
SEPS = ((b",", b":"), (b", ", b": "), (b" ,\n ", b" :\t"))

Batch = namedtuple("Batch", "reqs infos olds keys")


def obj(members, sep=0, lead=b"", trail=b""):
    """The object of (name, value bytes) members in this order, in one of the three separator styles."""
    c, k = SEPS[sep]
    return lead + b"{" + c.join(b'"%s"%s%s' % (n, k, v) for n, v in members) + b"}" + trail


def s(x):
    return b'"%s"' % x


def head():
    """One request of every class, in the order of model_register_model.CLASSES."""
    rec = obj([(b"type", s(b"type-1")), (b"mPath", s(b"p")), (b"lu", b"1000"), (b"instanceIds", b'{"i-0":5}')])
    return [
        (0, 0, (b"type-1", b"k", b"p"), b"", b"new-model"),
        (0, 0, (b"type-1", b"", b"p"), rec, b"m0"),
        (mm.LOAD_NOW, 0, (b"type-1", b"", b"p"), rec, b"m1"),
        (0, 0, (b"type-2", b"", b"p"), rec, b"m2"),
        (mm.DELETE, 0, (b"", b"", b""), b"", b"gone"),
        (mm.DELETE, 0, (b"", b"", b""), obj([(b"type", s(b"type-1")), (b"refs", b"2")]), b"m3"),
        (mm.DELETE | mm.LOAD_NOW, 7, (b"x", b"y", b"z"), rec, b"m4"),
        (0, 0, (b"type-1", b"", b"p"), b'{"type":"type-1"', b"m5"),
        (0, 0, (b"type-1", b"a\nb", b""), obj([(b"type", s(b"type-1")), (b"encKey", s(b"a\\nb"))]), b"m6"),
    ]


def to_batch(items):
    return Batch([(f, t) for f, t, _, _, _ in items], [i for _, _, i, _, _ in items], [o for _, _, _, o, _ in items],
                 [k for _, _, _, _, k in items])


def run_model(b, now=NOW, age=AGE):
    return mm.register_batch(b.reqs, b.infos, b.olds, now, age)


def has_every_class(b):
    return set(run_model(b)[1]) == set(mm.CLASSES)


def _pick(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


def drawn_items(n, seed):
    """n requests over stored values of every shape the rule speaks about, about two in three of them agreeing with the request."""
    rng = np.random.default_rng(4100 + seed)
    items = []
    for i in range(n):
        typ = _pick(rng, TYPES)
        enc = _pick(rng, (b"", b"", b"key-1", ESCAPES[:9], b"k" * 70))
        path = _pick(rng, (b"", b"/models/a", b"/models/" + b"d" * 190, "modèle".encode()))
        load_now = rng.random() < 0.3
        ict = int(_pick(rng, (0, 0, 1, NOW - 1, NOW, NOW + 1, NOW - 5 * AGE, int(rng.integers(1, NOW)))))
        flags = mm.LOAD_NOW if load_now else 0
        ts = mm.last_used_timestamp(flags, ict, NOW, AGE)
        r = rng.random()
        if r < 0.12:
            items.append((mm.DELETE if r < 0.04 else flags, ict, (typ, enc, path), b"", b"new-%d" % i))
            continue
        members = []
        st, se, sp = typ, enc, path
        if rng.random() < 0.12:
            st = _pick(rng, TYPES)
        if rng.random() < 0.1:
            se = _pick(rng, (b"", b"other", enc + b"x"))
        if rng.random() < 0.1:
            sp = _pick(rng, (b"", b"/other", path[:-1]))
        if st == b"NLCLASSIFIER" and rng.random() < 0.6:
            if rng.random() < 0.5:
                members.append((b"type", b"null"))
        else:
            members.append((b"type", s(st)))
        if se:
            members.append((b"encKey", s(mm.escape(se))))  # (a key that needs an escape is stored escaped: the host decides)
        elif rng.random() < 0.15:
            members.append((b"encKey", _pick(rng, (b"null", s(b"")))))
        if sp or rng.random() < 0.15:
            members.append((b"mPath", s(sp) if sp or rng.random() < 0.5 else b"null"))
        if rng.random() < 0.06:
            members.append((_pick(rng, (b"encKey", b"mPath")), _pick(rng, (b"5", b"true", b'{"a":"b"}', b'["x"]'))))
        if rng.random() < 0.5:
            members.append((b"refs", _pick(rng, (b"0", b"1", b"-1", b"2147483647", b"2147483648", b"-2147483648", b"-2147483649", b'"1"', b"1.5",
                                                 b"null", b"17"))))
        if rng.random() < 0.8:
            lu = _pick(rng, (ts - AGE - 1, ts - AGE, ts - AGE + 1, 0, ts, NOW, 5, (1 << 63) - 1, -(1 << 63), int(rng.integers(1, NOW))))
            members.append((b"lu", b"%d" % mm.jlong(lu)))
        if rng.random() < 0.5:
            members.append((b"instanceIds", b"{" + b",".join(b'"i-%d":%d' % (p, NOW - p) for p in range(int(rng.integers(0, 4)))) + b"}"))
        if rng.random() < 0.3:
            members.append((b"failedIn", b'{"i-7":%d}' % (NOW - 9)))
            members.append((b"fails", b'{"i-7":{"msg":"a \\"quoted\\" }{ failure"}}'))
        if rng.random() < 0.3:
            members.append((b"autoDel", b"true"))
        if rng.random() < 0.2:
            members.append((b"lul", b"%d" % (NOW - 77)))
        if rng.random() < 0.2:
            members.append((b"future", b'{"deep":[1,{"er":"}"}],"lu":3}'))
        order = rng.permutation(len(members))
        members = [members[j] for j in order]
        if members and rng.random() < 0.15:  # an earlier occurrence that loses
            name = _pick(rng, (b"type", b"encKey", b"mPath", b"refs", b"lu"))
            members.insert(0, (name, _pick(rng, (s(b"loser"), b"null", b"3"))) if name != b"lu" else (name, b"3"))
        old = obj(members, int(rng.integers(0, 3)), _pick(rng, (b"", b" ", b"\n\t")), _pick(rng, (b"", b"  ")))
        if r > 0.95:
            old = old[:-1 - int(rng.integers(0, max(len(old) - 2, 1)))]  # truncated
        if rng.random() < 0.3:
            flags, ict = mm.DELETE, 0
        if model_class(old) == UNSPECIFIED:
            old = obj([(b"type", s(typ))])
        items.append((flags, ict, (typ, enc, path), old, b"m%d" % int(rng.integers(0, 60))))
    return items


def sized_batch(n):
    if n < len(head()):
        return to_batch(head()[:n])
    return to_batch(head() + drawn_items(n - len(head()), n))


def single_batches():
    """n = 1, once per class."""
    return [to_batch([it]) for it in head()]


STRING_LENGTHS = (0, 1, 63, 64, 65, 200)


def string_batch():
    """Compared strings of 0, 1, 63, 64, 65 and 200 bytes against requests that are equal, and that differ only in the first, the
    last and the 64th byte — for each of the three attributes."""
    items = head()
    for L in STRING_LENGTHS:
        base = bytes(0x61 + (i * 7) % 26 for i in range(L))
        variants = [base]
        for at in (0, L - 1, 63):
            if 0 <= at < L:
                variants.append(base[:at] + b"#" + base[at + 1:])
        variants += [base + b"x", base[:-1]] if L else [b"x"]
        for which in range(3):
            for v in variants:
                stored = [b"type-1", b"ek", b"/p"]
                asked = list(stored)
                stored[which], asked[which] = base, v
                if which == 0 and not v:
                    continue  # (a register never asks for an empty type)
                old = obj([(b"type", s(stored[0])), (b"lu", b"5"), (b"encKey", s(stored[1])), (b"mPath", s(stored[2]))], L % 3)
                items.append((0, 0, tuple(asked), old, b"m%d" % L))
    return to_batch(items)


MEMBER_COUNTS = (63, 64, 65, 130)


def member_layouts():
    """[(n, k, members)]: values of 63, 64, 65 and 130 top-level members, the compared members (and lu) first, last, around the
    others, and as a losing first occurrence with the deciding one last, and the other way round."""
    want = [(b"type", s(b"type-2")), (b"encKey", s(b"ek")), (b"mPath", s(b"/p")), (b"refs", b"1"), (b"lu", b"9")]
    lose = [(b"type", s(b"type-1")), (b"encKey", b"null"), (b"mPath", s(b"/q")), (b"refs", b"0"), (b"lu", b"%d" % NOW)]
    out = []
    for n in MEMBER_COUNTS:
        fill = [(b"f%d" % i, b"%d" % i) for i in range(n - len(want))]
        short = [(b"f%d" % i, b"%d" % i) for i in range(n - 2 * len(want))]
        for k, members in enumerate((want + fill, fill + want, want[:2] + fill + want[2:], lose + short + want, want + short + lose)):
            assert len(members) == n
            out.append((n, k, members))
    return out


def _member_items(value_of):
    """head(), then each layout's value once as a touch and once as a delete."""
    items = head()
    for n, k, members in member_layouts():
        old = value_of(n, k, members)
        items.append((0, 0, (b"type-2", b"ek", b"/p"), old, b"m%d" % n))
        items.append((mm.DELETE, 0, (b"", b"", b""), old, b"m%d" % n))
    return to_batch(items)


def member_batch():
    """The member layouts on the tile, in the three separator styles."""
    def value_of(n, k, members):
        old = obj(members, k % 3)
        assert len(old) <= TILE
        return old
    return _member_items(value_of)


def padded_member_batch():
    """The same layouts padded past the tile (the pad in front, in the middle, at the end in turn): the serial walk sees a
    repeated compared name, and the compared members behind 64 and more others."""
    return _member_items(lambda n, k, members: padded(members, TILE + 1 + 13 * k, (0, n // 2, n)[k % 3]))


def padded(members, total, pad_at):
    """The object of `members` with a "pad" string member inserted at index pad_at so that the value has exactly `total` bytes."""
    probe = obj(members[:pad_at] + [(b"pad", s(b""))] + members[pad_at:])
    return obj(members[:pad_at] + [(b"pad", s(b"x" * (total - len(probe))))] + members[pad_at:])


def tile_edge_batch():
    """Stored values of 2 046 .. 2 050 bytes, each at every dword alignment of the value buffer: up to 2 048 bytes take the tile,
    longer ones the serial walk.  The compared members stand behind the padding, at the very end of the value."""
    items = head()
    at = sum(len(it[3]) for it in items)
    rec = [(b"autoDel", b"true"), (b"type", s(b"type-1")), (b"instanceIds", b'{"i-1":7}'), (b"lu", b"12"), (b"refs", b"3"),
           (b"encKey", s(b"ek")), (b"mPath", s(b"/models/edge"))]
    k = 0
    for total in range(TILE - 2, TILE + 3):
        for shift in range(4):
            fill = (shift - at) % 4 + 4
            items.append((0, 0, (b"NLCLASSIFIER", b"", b""), b"{}" + b" " * (fill - 2), b"fill"))
            at += fill
            assert at % 4 == shift
            old = padded(rec, total, (0, 1, 3)[k % 3])
            assert len(old) == total
            asked = [(b"type-1", b"ek", b"/models/edge"), (b"type-1", b"ek", b"/models/edgf"), (b"type-1", b"ek", b"/models/edge")][k % 3]
            flags = (0, 0, mm.DELETE, mm.LOAD_NOW)[k % 4]
            items.append((flags, 0, asked, old, b"m-edge"))
            at += total
            k += 1
    return to_batch(items)


def escape_batch():
    """Creations whose encKey and mPath need every kind of escape (the type stays plain: the read side leaves an escaped type
    unspecified)."""
    items = head()
    for k, (enc, path) in enumerate(((ESCAPES, b""), (b"", ESCAPES), (ESCAPES * 3, b'"' * 64 + b"\\" * 65), (b"\x00", b"\x1f" * 70))):
        items.append((0, k, (b"type-1", enc, path), b"", b"esc-%d" % k))
    return to_batch(items)


def corpus_values():
    """The malformed and edge lists of tests/ingest_corpus.py: every value that is not empty and that the parsers speak about."""
    values = list(ic.model_corpus()) + ic.chunk_edge_models() + ic.tile_edge_models()[0]
    values = [v if isinstance(v, bytes) else v.encode() for v in values]
    return [v for v in values if v and model_class(v) != UNSPECIFIED]


def corpus_batch(values):
    """Every non-empty value of a parser corpus as the stored value of a register and of a delete."""
    items = head()
    for v in values:
        items.append((0, 0, (b"t1", b"", b""), v, b"c"))
        items.append((mm.DELETE, 0, (b"", b"", b""), v, b"c"))
    return to_batch(items)


def every_batch(corpus_values=()):
    """Every batch of nine requests or more that the GPU test sends."""
    out = [sized_batch(n) for n in SIZES if n >= 9] + [string_batch(), member_batch(), padded_member_batch(), tile_edge_batch(), escape_batch()]
    if corpus_values:
        out.append(corpus_batch(corpus_values))
    return out
