"""The batches tests/test_models_refs_gpu.py sends to mmp_models_refs_json, built without a device so that
tests/test_model_refs_model.py can assert what each of them holds.  An item is (flags, last_used, (type, encKey, mPath), old);
every batch of seven requests or more starts with head(): one request of every class, both flags set and clear.  to_batch
refuses such a batch that lacks a class or a flag state."""
from collections import namedtuple

import numpy as np

from tests import ingest_corpus as ic
from tests import model_refs_model as mr
from tests.ingest_model import UNSPECIFIED, model_class
from tests.model_register_fixtures import ESCAPES, TILE, obj, padded, s

NOW = 1_700_000_000_000
SIZES = (0, 1, 63, 64, 65, 257)
NO_INFO = (b"", b"", b"")
LONG_MIN, LONG_MAX = -(1 << 63), (1 << 63) - 1
REFS_VALUES = (None, b"0", b"1", b"2", b"-1", b"2147483647", b"-2147483648", b"2147483648", b"-2147483649", b"1.0", b'"1"', b"null",
               b"17")
AUTO_VALUES = (None, b"true", b"false", b"null", b"1", b'"true"')
LAST_USED = (0, 1, NOW, LONG_MIN, LONG_MAX, -5)

Batch = namedtuple("Batch", "reqs infos olds")


def head():
    """One request of every class, in the order of model_refs_model.CLASSES."""
    rec = obj([(b"type", s(b"type-1")), (b"mPath", s(b"p")), (b"refs", b"2"), (b"lu", b"1000"), (b"instanceIds", b'{"i-0":5}')])
    return [
        (0, 0, NO_INFO, rec),
        (mr.INC | mr.AUTO_DELETE, NOW, (b"type-1", b"k", b"p"), b""),
        (0, 7, (b"x", b"y", b"z"), obj([(b"type", s(b"type-1")), (b"autoDel", b"true"), (b"refs", b"1")])),
        (mr.AUTO_DELETE, 0, NO_INFO, b""),
        (mr.INC, NOW, NO_INFO, b""),
        (mr.INC, NOW, NO_INFO, b'{"type":"type-1"'),
        (mr.INC, NOW, NO_INFO, obj([(b"type", s(b"type-1")), (b"refs", b"1.5")])),
    ]


def run_model(b):
    return mr.refs_batch(b.reqs, b.infos, b.olds)


def holds_everything(b):
    """Every class, and each of the two flags both set and clear."""
    flags = [f for f, _ in b.reqs]
    return (set(run_model(b)[1]) == set(mr.CLASSES) and all(any(f & bit for f in flags) and any(not f & bit for f in flags)
                                                            for bit in (mr.INC, mr.AUTO_DELETE)))


def to_batch(items):
    b = Batch([(f, t) for f, t, _, _ in items], [i for _, _, i, _ in items], [o for _, _, _, o in items])
    if len(items) >= len(head()) and not holds_everything(b):
        raise ValueError("a batch that lacks a class or a flag state")
    return b


def _pick(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


def drawn_items(n, seed):
    """n requests over stored values of every shape the rule speaks about."""
    rng = np.random.default_rng(7300 + seed)
    items = []
    for _ in range(n):
        flags = (mr.INC if rng.random() < 0.5 else 0) | (mr.AUTO_DELETE if rng.random() < 0.3 else 0)
        lu = int(_pick(rng, LAST_USED + (int(rng.integers(1, NOW)),)))
        info = (_pick(rng, (b"", b"type-1", b"type-2")), _pick(rng, (b"", b"key-1", ESCAPES[:9])), _pick(rng, (b"", b"/models/a")))
        if rng.random() < 0.15:
            items.append((flags, lu, info, b""))
            continue
        members = [(b"type", s(_pick(rng, (b"type-1", b"type-2"))))]
        refs = _pick(rng, REFS_VALUES)
        if refs is not None:
            members.append((b"refs", refs))
        auto = _pick(rng, AUTO_VALUES + (None, b"true", b"true"))
        if auto is not None:
            members.append((b"autoDel", auto))
        if rng.random() < 0.7:
            members.append((b"lu", b"%d" % _pick(rng, (0, 5, NOW - 9, LONG_MAX, LONG_MIN))))
        if rng.random() < 0.5:
            members.append((b"instanceIds", b"{" + b",".join(b'"i-%d":%d' % (p, NOW - p) for p in range(int(rng.integers(0, 4)))) + b"}"))
        if rng.random() < 0.3:
            members.append((b"failedIn", b'{"i-7":%d}' % (NOW - 9)))
            members.append((b"fails", b'{"i-7":{"msg":"a \\"quoted\\" }{ failure","refs":9}}'))
        if rng.random() < 0.3:
            members.append((b"mPath", s(b"/models/" + b"d" * int(rng.integers(0, 90)))))
        if rng.random() < 0.3:
            members.append((b"future", _pick(rng, (b'{"deep":[1,{"er":"}"}],"refs":3}', b"[1,2]", b"true", b"null", b"-1.5e3", s(b"x")))))
        members = [members[j] for j in rng.permutation(len(members))]
        if rng.random() < 0.2:  # an earlier occurrence that loses
            name = _pick(rng, (b"refs", b"autoDel", b"lu"))
            members.insert(0, (name, {b"refs": _pick(rng, (b"5", b'"x"')), b"autoDel": _pick(rng, (b"true", b"7")), b"lu": b"3"}[name]))
        old = obj(members, int(rng.integers(0, 3)), _pick(rng, (b"", b" ", b"\n\t")), _pick(rng, (b"", b"  ")))
        if rng.random() < 0.05:
            old = old[:-1 - int(rng.integers(0, max(len(old) - 2, 1)))]  # truncated
        if model_class(old) == UNSPECIFIED:
            old = obj([(b"type", s(b"type-1"))])
        items.append((flags, lu, info, old))
    return items


def sized_batch(n):
    if n < len(head()):
        return to_batch(head()[:n])
    return to_batch(head() + drawn_items(n - len(head()), n))


def single_batches():
    """n = 1, once per class."""
    return [to_batch([it]) for it in head()]


def boundary_batch():
    """Every refs value against every autoDel value, as an INC and as a DEC, with last_used at its edges."""
    items = head()
    k = 0
    for refs in REFS_VALUES:
        for auto in AUTO_VALUES:
            members = [(b"type", s(b"t"))] + ([(b"refs", refs)] if refs is not None else []) + \
                      ([(b"autoDel", auto)] if auto is not None else []) + [(b"lu", b"44")]
            for flags in (0, mr.INC):
                items.append((flags, LAST_USED[k % len(LAST_USED)], NO_INFO, obj(members, k % 3)))
                k += 1
    # a losing first occurrence of each noted name
    for first, then in ((b"7", b"1"), (b'"x"', b"0"), (b"1", b"null")):
        for flags in (0, mr.INC):
            items.append((flags, 3, NO_INFO, obj([(b"refs", first), (b"type", s(b"t")), (b"refs", then)])))
    for first, then in ((b"true", b"false"), (b"false", b"true"), (b"3", b"true"), (b"true", b"3")):
        for flags in (0, mr.INC):
            items.append((flags, 3, NO_INFO, obj([(b"autoDel", first), (b"refs", b"1"), (b"autoDel", then)])))
    return to_batch(items)


def created_batch():
    """Creations: each optional member present and omitted, strings that need every kind of escape, and rendered strings of
    1, 63, 64, 65 and 200 bytes."""
    items = head()
    for enc in (b"", b"k"):
        for path in (b"", b"/p"):
            for auto in (0, mr.AUTO_DELETE):
                for lu in (0, NOW, LONG_MIN):
                    items.append((mr.INC | auto, lu, (b"type-1", enc, path), b""))
    for k, (enc, path) in enumerate(((ESCAPES, b""), (b"", ESCAPES), (ESCAPES * 3, b'"' * 64 + b"\\" * 65), (b"\x00", b"\x1f" * 70))):
        items.append((mr.INC, k, (b"type-1", enc, path), b""))
    for n in (1, 63, 64, 65, 200):
        text = bytes(0x61 + (i * 7) % 26 for i in range(n))
        items.append((mr.INC, 1, (text, text, text), b""))
    return to_batch(items)


MEMBER_COUNTS = (63, 64, 65, 130)


def member_layouts():
    """[(n, k, members)]: values of 63, 64, 65 and 130 top-level members, the noted members (and lu) first, last, around the
    others, and as a losing first occurrence with the deciding one last, and the other way round."""
    want = [(b"refs", b"1"), (b"autoDel", b"true"), (b"lu", b"9")]
    lose = [(b"refs", b"5"), (b"autoDel", b"false"), (b"lu", b"%d" % NOW)]
    out = []
    for n in MEMBER_COUNTS:
        fill = [(b"f%d" % i, b"%d" % i) for i in range(n - len(want))]
        short = [(b"f%d" % i, b"%d" % i) for i in range(n - 2 * len(want))]
        for k, members in enumerate((want + fill, fill + want, want[:1] + fill + want[1:], lose + short + want, want + short + lose)):
            assert len(members) == n
            out.append((n, k, members))
    return out


def _member_items(value_of):
    items = head()
    for n, k, members in member_layouts():
        old = value_of(n, k, members)
        items.append((mr.INC, NOW + n, NO_INFO, old))
        items.append((0, 0, NO_INFO, old))
    return to_batch(items)


def member_batch():
    """The member layouts on the tile, in the three separator styles."""
    def value_of(n, k, members):
        old = obj(members, k % 3)
        assert len(old) <= TILE
        return old
    return _member_items(value_of)


def padded_member_batch():
    """The same layouts padded past the tile (the pad in front, in the middle, at the end in turn)."""
    return _member_items(lambda n, k, members: padded(members, TILE + 1 + 13 * k, (0, n // 2, n)[k % 3]))


def _padded_by_path(members, total):
    """The object of `members` with a kept "mPath" string in front, so long that the value has exactly `total` bytes."""
    probe = obj([(b"mPath", s(b"/"))] + members)
    return obj([(b"mPath", s(b"/" + b"m" * (total - len(probe))))] + members)


def tile_edge_batch():
    """Stored values of 2 046 .. 2 050 bytes, each at every dword alignment of the value buffer: up to 2 048 bytes take the tile,
    longer ones the serial walk.  Padded once by an unknown member and once by a long kept string; the noted members stand behind
    the padding, at the very end of the value."""
    items = head()
    at = sum(len(it[3]) for it in items)
    rec = [(b"type", s(b"type-1")), (b"instanceIds", b'{"i-1":7}'), (b"lu", b"12"), (b"autoDel", b"false"), (b"refs", b"3")]
    k = 0
    for total in range(TILE - 2, TILE + 3):
        for shift in range(4):
            for by_path in (False, True):
                fill = (shift - at) % 4 + 4
                items.append((0, 0, NO_INFO, b"{}" + b" " * (fill - 2)))
                at += fill
                assert at % 4 == shift
                old = _padded_by_path(rec, total) if by_path else padded(rec, total, (0, 1, 3)[k % 3])
                assert len(old) == total
                items.append(((mr.INC, 0)[k % 2], NOW + k, NO_INFO, old))
                at += total
                k += 1
    return to_batch(items)


def repeated_batch():
    """One stored value 64 times in a call, as an INC and as a DEC in turn."""
    old = obj([(b"type", s(b"type-1")), (b"refs", b"3"), (b"autoDel", b"true"), (b"lu", b"5"), (b"instanceIds", b'{"i-2":9}')], 1)
    return to_batch(head() + [((mr.INC, 0)[k % 2], k, NO_INFO, old) for k in range(64)])


def corpus_values():
    """The malformed and edge lists of tests/ingest_corpus.py: every value that is not empty and that the parsers speak about."""
    values = list(ic.model_corpus()) + ic.chunk_edge_models() + ic.tile_edge_models()[0]
    values = [v if isinstance(v, bytes) else v.encode() for v in values]
    return [v for v in values if v and model_class(v) != UNSPECIFIED]


def corpus_batch(values):
    """Every non-empty value of a parser corpus as the stored value of an INC and of a DEC."""
    items = head()
    for v in values:
        items.append((mr.INC, 5, NO_INFO, v))
        items.append((0, 0, NO_INFO, v))
    return to_batch(items)


def every_batch(corpus=()):
    """Every batch of seven requests or more that the GPU test sends."""
    out = [sized_batch(n) for n in SIZES if n >= 7] + [boundary_batch(), created_batch(), member_batch(), padded_member_batch(),
                                                       tile_edge_batch(), repeated_batch()]
    if corpus:
        out.append(corpus_batch(corpus))
    return out
