"""The batches tests/test_vmodels_write_gpu.py sends to mmp_vmodels_write_json, built without a device so that
tests/test_vmodel_write_model.py can assert what each of them holds.  The registry is tests/vmodel_fixtures.py's: kind k % 8 of
MODEL_KINDS at row k, so a batch names models by kind.  An item is (op, flags, (id_a, id_b, owner), old); every batch of seventeen
requests or more starts with head(): every class, every op, every request flag and every row flag, set and clear.  to_batch refuses
such a batch that lacks one."""
from collections import namedtuple

import numpy as np

from tests import vmodel_fixtures as vf
from tests import vmodel_model as vm
from tests import vmodel_write_model as wm
from tests.ingest_model import UNSPECIFIED
from tests.model_register_fixtures import ESCAPES, TILE, obj, s

NOW, AGE = vf.NOW, vf.AGE
M = 300
SIZES = (0, 1, 63, 64, 65, 257)
DEFAULT_OWNER = b"default-owner"
MIDS = vf.model_ids(M)
POD_IDS = ["pod-%d" % i for i in range(8)]  # (the CPU tests' stand-in: the records depend on the kinds only)
RECS = vf.registry_values(POD_IDS, M)[1]
REG = vm.Registry(MIDS, RECS)

Batch = namedtuple("Batch", "reqs strs olds")


def mid(kind, j=1):
    """The id of the j-th model of a kind (j >= 1: row 0 carries the empty id)."""
    return MIDS[vf.MODEL_KINDS.index(kind) + 8 * j]


def rec(amid=None, tmid=None, owner=None, failed=False, extra=(), sep=0, lead=b"", trail=b"", order=None):
    """A stored VModelRecord from RAW bytes (nothing is escaped); None: the member is omitted."""
    members = [(n, s(x)) for n, x in ((b"o", owner), (b"amid", amid), (b"tmid", tmid)) if x is not None]
    members += [(b"failed", b"true")] * bool(failed) + list(extra)
    if order is not None:  # (a numpy Generator: the members in a drawn order)
        members = [members[j] for j in order.permutation(len(members))]
    return obj(members, sep, lead, trail)


A, B, C = mid("loaded1"), mid("loaded1", 2), mid("not_loaded")
UNKNOWN = b"no-such-model"


def head():
    """Every class in the order of vmodel_write_model.CLASSES, then what the flags still lack."""
    X = wm
    return [
        (X.SET, X.LOAD_NOW, (A, b"", b"owner-a"), b""),
        (X.SET, X.FORCE, (B, b"", b""), rec(A, A, b"owner-a")),
        (X.SET, 0, (A, b"", b""), rec(A, A)),
        (X.SET, X.UPDATE_ONLY, (A, b"", b""), b""),
        (X.SET, 0, (B, C, b""), rec(A, A)),
        (X.SET, 0, (A, b"", b"owner-b"), rec(A, A, b"owner-a")),
        (X.SET, X.TARGET_EXISTS, (B, b"", b""), rec(A, A)),
        (X.DELETE, 0, (b"", b"", b""), b""),
        (X.DELETE, 0, (b"", b"", b"owner-a"), rec(A, B, b"owner-a")),
        (X.COMPLETE, 0, (B, A, b""), rec(A, C)),
        (X.FAIL_FLAG, X.FAILED, (b"", b"", b""), rec(A, B)[:-2]),
        (X.SET, 0, (A, b"", b""), rec(b"esc\\\\aped", A)),
        (X.SET, X.TARGET_EXISTS | X.TARGET_LOADED, (B, b"", b""), rec(A, A)),
        (X.SET, X.TARGET_EXISTS | X.TARGET_NOT_LOADED, (B, b"", b""), rec(A, A)),
        (X.FAIL_FLAG, X.FAILED, (b"", b"", b""), rec(A, B)),
        (X.SET, 0, (B, b"", b""), rec(UNKNOWN, UNKNOWN)),
        (X.COMPLETE, 0, (B, A, b""), rec(A, B, failed=True)),
    ]


def run_model(b, reg=REG, now=NOW, age=AGE, default_owner=DEFAULT_OWNER):
    return wm.write_batch(b.reqs, b.strs, b.olds, reg, now, age, default_owner)


def holds_everything(b, reg=REG):
    """Every class, every op, every request flag and every row flag, each flag both set and clear."""
    _, rows = run_model(b, reg)
    ops, qf, rf = [o for o, _ in b.reqs], [f for _, f in b.reqs], [r.flags for r in rows]
    both = lambda xs, bit: any(x & bit for x in xs) and any(not x & bit for x in xs)  # noqa: E731
    return ({r.cls for r in rows} == set(wm.CLASSES) and set(ops) == set(wm.OPS) and all(both(qf, bit) for bit in wm.REQ_FLAGS) and
            all(both(rf, bit) for bit in wm.ROW_FLAGS))


def to_batch(items, reg=REG):
    b = Batch([(o, f) for o, f, _, _ in items], [t for _, _, t, _ in items], [v for _, _, _, v in items])
    if len(items) >= len(head()) and not holds_everything(b, reg):
        raise ValueError("a batch that lacks a class, an op or a flag state")
    return b


def _pick(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


EXTRAS = ((b"future", b'{"a":[1,2,{"amid":null}],"tmid":"x"}'), (b"n", b"-1.5e3"), (b"str", s(b"x\\\"amid\\\"")), (b"t", b"true"), (b"z", b"null"),
          (b"arr", b'["amid",{"failed":true}]'))


def drawn_items(n, seed):
    """n requests over stored records of every shape the rule speaks about; ids and owners come from small pools, so that equal,
    different and null meet in every position."""
    rng = np.random.default_rng(8800 + seed)
    ids = (A, B, C, mid("loaded3_lu0"), mid("failed_only"), mid("empty"), mid("loaded_lu_max"), mid("loaded1_lu1"), UNKNOWN, b"")
    owners = (None, b"owner-a", b"owner-b", b"")
    items = []
    for _ in range(n):
        op = int(_pick(rng, (wm.SET,) * 5 + (wm.DELETE, wm.COMPLETE, wm.COMPLETE, wm.FAIL_FLAG)))
        flags = 0
        for bit in wm.REQ_FLAGS:
            if rng.random() < 0.3:
                flags |= bit
        if flags & wm.TARGET_LOADED and flags & wm.TARGET_NOT_LOADED:
            flags &= ~wm.TARGET_NOT_LOADED
        am, tm = _pick(rng, ids[:6] + (None,)), _pick(rng, ids[:6] + (None,))
        if rng.random() < 0.4:
            tm = am
        owner = _pick(rng, owners)
        ida = _pick(rng, ids[:9]) if rng.random() < 0.5 else (tm or A)
        idb = _pick(rng, (b"", b"", am or b"", tm or b"", ida, C))
        req_owner = _pick(rng, (b"", b"", owner or b"", b"owner-a", (owner[:-1] + b"?") if owner else b"x"))
        if op in (wm.SET, wm.COMPLETE) and not ida:
            ida = A
        if rng.random() < 0.12:
            items.append((op, flags, (ida, idb, req_owner), b""))
            continue
        extra = [EXTRAS[j] for j in range(len(EXTRAS)) if rng.random() < 0.25]
        old = rec(am, tm, owner, rng.random() < 0.4, extra, int(rng.integers(0, 3)), _pick(rng, (b"", b" ", b"\n\t")), _pick(rng, (b"", b"  ")),
                  rng)
        r = rng.random()
        if r < 0.1:  # an earlier occurrence that loses
            old = old.replace(b"{", b'{"%s":%s,' % (_pick(rng, (b"amid", b"tmid", b"o")), _pick(rng, (b"null", s(b"loser")))), 1)
        elif r < 0.15:
            old = old.replace(b"{", b'{"failed":%s,' % _pick(rng, (b"true", b"false")), 1)
        elif r < 0.2:
            old = old[:-1 - int(rng.integers(0, max(len(old) - 2, 1)))]  # truncated
        elif r < 0.25:
            old = rec(b"esc\\\\" + (am or b"x"), tm, owner)  # the host decides
        if vm.classify(old)[0] == UNSPECIFIED:
            old = rec(am, tm, owner)
        items.append((op, flags, (ida, idb, req_owner), old))
    return items


def sized_batch(n):
    if n < len(head()):
        return to_batch(head()[:n])
    return to_batch(head() + drawn_items(n - len(head()), n))


def single_batches():
    """n = 1, once per class (the first twelve of the head) — every op among them."""
    return [to_batch([it]) for it in head()[:len(wm.CLASSES)]]


def padded(total, by_owner, k):
    """A well-formed value of exactly `total` bytes, padded by a long kept `o` or by an unknown member; the owned members stand
    behind the padding (k odd) or in front of it."""
    fill = [(b"o", s(b""))] if by_owner else [(b"pad", s(b"")), (b"o", s(b"own"))]
    owned = [(b"amid", s(A)), (b"tmid", s(B)), (b"failed", b"true")]
    probe = obj(fill + owned if k % 2 else owned + fill)
    fill[0] = (fill[0][0], s(b"p" * (total - len(probe))))
    v = obj(fill + owned if k % 2 else owned + fill)
    assert len(v) == total
    return v


def tile_edge_batch():
    """Stored values of 2 046 .. 2 050 bytes, each at every dword alignment of the value buffer, padded once by a long kept string
    and once by an unknown member: up to 2 048 bytes take the tile, longer ones the serial walk."""
    items = head()
    at = sum(len(it[3]) for it in items)
    k = 0
    for total in range(TILE - 2, TILE + 3):
        for shift in range(4):
            for by_owner in (False, True):
                fill = (shift - at) % 4 + 4
                items.append((wm.FAIL_FLAG, 0, (b"", b"", b""), b"{}" + b" " * (fill - 2)))
                at += fill
                assert at % 4 == shift
                old = padded(total, by_owner, k)
                req = ((wm.SET, wm.FORCE, (C, b"", b"")), (wm.COMPLETE, 0, (B, A, b"")), (wm.FAIL_FLAG, 0, (b"", b"", b"")),
                       (wm.DELETE, 0, (b"", b"", b"")))[k % 4]
                items.append(req + (old,))
                at += total
                k += 1
    return to_batch(items)


MEMBER_COUNTS = (63, 64, 65, 130)


def member_batch(pad_past_tile=False):
    """Values of 63, 64, 65 and 130 members, the owned members (and o) first, last, around the others, and as a losing first
    occurrence with the deciding one last, and the other way round; each as a forced SET, a COMPLETE and a DELETE."""
    want = [(b"o", s(b"own")), (b"amid", s(A)), (b"tmid", s(B)), (b"failed", b"true")]
    lose = [(b"o", s(b"other")), (b"amid", s(C)), (b"tmid", b"null"), (b"failed", b"false")]
    items = head()
    for n in MEMBER_COUNTS:
        fill = [(b"f%d" % i, b"%d" % i) for i in range(n - len(want))]
        short = fill[:n - 2 * len(want)]
        for k, members in enumerate((want + fill, fill + want, want[:2] + fill + want[2:], lose + short + want, want + short + lose)):
            assert len(members) == n
            if pad_past_tile:
                members = members[:n // 2] + [(b"pad", s(b"x" * (TILE - 200 + 13 * k)))] + members[n // 2:]
            old = obj(members, k % 3)
            assert (len(old) > TILE) == pad_past_tile
            items.append((wm.SET, wm.FORCE, (C, b"", b"own"), old))
            items.append((wm.COMPLETE, 0, (B, A, b""), old))
            items.append((wm.DELETE, 0, (b"", b"", b"own"), old))
    return to_batch(items)


STRING_LENGTHS = (0, 1, 63, 64, 65, 200)


def string_batch():
    """Compared and rendered ids of 0, 1, 63, 64, 65 and 200 bytes against requests that are equal, and that differ only in the
    first, the last and the 64th byte — as the target of a SET, as fromId / toId of a COMPLETE and as the owner of a DELETE."""
    items = head()
    for L in STRING_LENGTHS:
        base = bytes(0x61 + (i * 7) % 26 for i in range(L))
        variants = [base]
        for at in (0, L - 1, 63):
            if 0 <= at < L:
                variants.append(base[:at] + b"#" + base[at + 1:])
        variants += [base + b"x", base[:-1]] if L else [b"x"]
        for v in variants:
            if v:
                items.append((wm.SET, 0, (v, b"", b""), rec(base, base, b"own")))         # UNCHANGED or UPDATED
                items.append((wm.SET, 0, (A, v, b""), rec(base, base, b"own")))           # the expected target
                items.append((wm.COMPLETE, 0, (v, A, b""), rec(A, base)))                # toId against tmid
            items.append((wm.COMPLETE, 0, (A, v, b""), rec(base, A)))                    # fromId against amid
            items.append((wm.DELETE, 0, (b"", b"", v), rec(A, B, base)))                 # the owner
            items.append((wm.SET, wm.FORCE, (C, b"", v), rec(base, A, base)))            # dec spans of that length
    return to_batch(items)


def escape_batch():
    """Request strings that need every kind of escape, rendered into created and updated records."""
    items = head()
    for e in (ESCAPES, ESCAPES * 3, b'"' * 64 + b"\\" * 65, b"\x01", b"\x1f" * 70):
        items.append((wm.SET, 0, (e, b"", e), b""))
        items.append((wm.SET, 0, (e, b"", b""), b""))
        items.append((wm.SET, wm.FORCE, (e, b"", b""), rec(A, B, b"own")))
        items.append((wm.SET, 0, (e, b"", b"own"), rec(None, None, b"own", True)))
        # (a COMPLETE renders no escape: its toId equals a stored string, and a stored string that holds one is the host's)
    return to_batch(items)


def corpus_values():
    """The malformed and edge lists of tests/vmodel_fixtures.py: every value that is not empty and that the parsers speak about."""
    values = [v.encode() for v in vf.MALFORMED + vf.EDGE] + [vf.template_across_chunks(k).encode() for k in range(64)]
    return [v for v in values if v and vm.classify(v)[0] != UNSPECIFIED]


def corpus_batch():
    """Every such value as the stored value of each of the four ops."""
    items = head()
    for v in corpus_values():
        items.append((wm.SET, wm.FORCE, (A, b"", b""), v))
        items.append((wm.DELETE, 0, (b"", b"", b""), v))
        items.append((wm.COMPLETE, 0, (b"a", b"a", b""), v))
        items.append((wm.FAIL_FLAG, wm.FAILED, (b"", b"", b""), v))
    return to_batch(items)


def repeated_batch():
    """One stored value 64 times in a call, under the four ops in turn."""
    old = rec(A, B, b"own", True, EXTRAS[:2], 1)
    reqs = ((wm.SET, wm.FORCE, (C, b"", b"")), (wm.DELETE, 0, (b"", b"", b"own")), (wm.COMPLETE, 0, (B, A, b"")), (wm.FAIL_FLAG, 0, (b"", b"", b"")))
    return to_batch(head() + [reqs[k % 4] + (old,) for k in range(64)])


def every_batch():
    """Every batch of seventeen requests or more that the GPU test sends."""
    return [sized_batch(n) for n in SIZES if n >= len(head())] + [tile_edge_batch(), member_batch(), member_batch(True), string_batch(),
                                                                 escape_batch(), corpus_batch(), repeated_batch()]
