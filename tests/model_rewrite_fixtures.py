"""What tests/test_model_rewrite_model.py and tests/test_models_rewrite_gpu.py share: an 8 x 300 world whose first rows are set
by construction, and the batches of the GPU tests — every one of them built here, so that the CPU test can assert from the model
alone that no GPU comparison hides behind skipped rows (check_conditions).

A batch is a Batch(rows, olds, last_unload, fail_pod, msgs).  Every batch of two or more rows starts with HEAD, eight items
that between them hold every status and every owned member both present and omitted."""
import json
from collections import namedtuple

import numpy as np

from tests import model_rewrite_model as mrm
from tests.ingest_model import model_bean
from tests.model_events_fixtures import World, make_model_ids

Batch = namedtuple("Batch", "rows olds last_unload fail_pod msgs")
OWNED = (b"instanceIds", b"failedIn", b"fails", b"lu", b"lul")
MESSAGES = (b"", b"load failed", b'quote " backslash \\ newline \n tab \t e-acute \xc3\xa9', b"\x01\x1f bell", b"x" * 150)
SEPS = ((",", ":"), (", ", ": "), (" ,\n ", " :\t"))  # the three separator styles of modelmesh_amd/wire.py
TILE = 2048


def rewrite_world(seed=0):
    """World + the ids of its 300 rows + the setup events (row, value, deleted) that fix rows 0 .. 4:
    0 deleted (no owned member at all)        1 failed only, with fails, lu 0        2 loaded only, lu set
    3 / 4 name an id no instance has: the device holds pod -1 for it (status 2)."""
    w = World(seed)
    w.base_ids = make_model_ids(w.rng, len(w.values))
    p = w.pod_ids
    w.setup = [
        (0, "", 1),
        (1, '{"type":"type-1","mPath":"s3://b/m1","failedIn":{"%s":5,"%s":6},"fails":{"%s":{"msg":"boom"},"%s":{"msg":"x","t":5}}}'
         % (p[0], p[2], p[0], p[2]), 0),
        (2, '{"instanceIds":{"%s":7},"lu":9,"refs":2}' % p[1], 0),
        (3, '{"instanceIds":{"ghost-1":7,"%s":8},"lu":3}' % p[1], 0),
        (4, '{"mPath":"m4","failedIn":{"ghost-2":1}}', 0),
    ]
    w.stored = [v.encode() for v in w.values]
    for row, v, gone in w.setup:
        w.stored[row] = b"{}" if gone else v.encode()
    return w


def recs_after_setup(w):
    """The registry, record by record, after the world's values and the setup events — from the model alone."""
    pod_of = {s: i for i, s in enumerate(w.pod_ids)}
    recs = []
    for v in w.stored:
        b = model_bean(v, pod_of, w.type_names, 0)
        assert b.status == 0
        recs.append((b.type, b.lu, tuple(b.loaded), tuple(b.failed)))
    recs[0] = (0, 0, (), ())
    return recs


def head(w):
    """Eight items: status 0 x 5 (rows 0, 1, 2, 1 with a new failure, a fleet row), status 2 x 2, status 1 x 1."""
    s = w.stored
    return [
        (0, s[0], 0, -1, b""),                      # the empty row, lul 0: '{}'
        (1, s[1], 12345, -1, b""),                  # failedIn + fails + lul, no instanceIds, no lu
        (2, s[2], 0, -1, b""),                      # instanceIds + lu, no failedIn / fails / lul
        (3, s[3], 5, -1, b""),                      # status 2
        (4, s[4], 0, -1, b""),                      # status 2
        (1, s[1], 7, 0, MESSAGES[2]),               # addLoadFailure on pod 0: its old entry replaced, escaped
        (2, s[2][:-3], 0, -1, b""),                 # status 1
        (7, s[7], -(1 << 63), -1, b""),
    ]


def to_batch(items):
    rows, olds, lul, fpod, msgs = (list(x) for x in zip(*items)) if items else ([], [], [], [], [])
    return Batch(np.array(rows, np.int32), olds, np.array(lul, np.int64), np.array(fpod, np.int32), msgs)


def drawn_items(w, recs, n, seed):
    """n items over the fleet rows (5 ..): the row's own stored value, one in twelve truncated; a fail_pod in a third of
    them, half of those on an instance of the failed list."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        r = int(rng.integers(5, len(w.stored)))
        old = w.stored[r] if rng.random() > 1 / 12 else w.stored[r][:-3]
        fp, msg = -1, b""
        if rng.random() < 1 / 3:
            failed = recs[r][3]
            fp = int(failed[int(rng.integers(len(failed)))][0]) if failed and rng.random() < 0.5 else int(rng.integers(len(w.pod_ids)))
            msg = MESSAGES[int(rng.integers(len(MESSAGES)))]
        lul = int(rng.integers(0, 3)) * int(rng.integers(1, 10**12))
        out.append((r, old, lul, fp, msg))
    return out


def sized_batch(w, recs, n):
    """The batch of n values: HEAD and drawn items; n = 0 and n = 1 are what they can be."""
    if n < 8:
        return to_batch(head(w)[:n])
    return to_batch(head(w) + drawn_items(w, recs, n - 8, 100 + n))


def single_batches(w):
    """n = 1 once per status."""
    h = head(w)
    return [to_batch([h[1]]), to_batch([h[6]]), to_batch([h[3]])]


def same_row_batch(w):
    """HEAD, then row 1 sixty-four times in one call under different fail_pod / messages."""
    items = head(w)
    for k in range(64):
        items.append((1, w.stored[1], k, k % (len(w.pod_ids) + 1) - 1, MESSAGES[k % len(MESSAGES)]))
    return to_batch(items)


def padded(fields, total, where):
    """A value of exactly `total` bytes: `fields` with the pad in the kept member mPath ('kept') or in a message inside fails."""
    def dump(pad):
        f = dict(fields)
        if where == "kept":
            f["mPath"] = "s3://" + "p" * pad
        else:
            f["fails"] = {k: ({"msg": "m" * pad} if i == 0 else v) for i, (k, v) in enumerate(f["fails"].items())}
        return json.dumps(f, separators=(",", ":")).encode()
    v = dump(total - len(dump(0)))
    assert len(v) == total
    return v


def tile_edge_batches(w):
    """Old values of 2046 .. 2050 bytes for row 1, the value starting at each of the four dword alignments of the buffer (a
    filler value of 8 + a bytes in front); the pad in a kept member, and once in fails.  2048 is the last size of the tile."""
    p = w.pod_ids
    fields = {"type": "type-1", "x": [1, {"y": "}"}], "failedIn": {p[0]: 5, p[2]: 6},
              "fails": {p[0]: {"msg": "boom"}, p[2]: {"msg": "x", "t": 5}, "gone": {"msg": "stale"}}, "lu": 4, "zz": None}
    out = []
    for a in range(4):
        filler = b'{"a":' + b"1" * (2 + a) + b"}"
        assert len(filler) == 8 + a
        items = head(w) + [(2, filler, 0, -1, b"")]
        for total in range(TILE - 2, TILE + 3):
            items.append((1, padded(fields, total, "kept"), total, 2, b"again"))
        if a == 1:
            for total in range(TILE - 2, TILE + 3):
                items.append((1, padded(fields, total, "fails"), 0, -1, b""))
        # (the filler sits right in front of the padded values: move HEAD behind them so that the alignment is the filler's)
        out.append(to_batch(items[8:] + items[:8]))
    return out


ENTRY_COUNTS = ((0, 0), (1, 0), (0, 1), (63, 0), (0, 64), (64, 1), (33, 30), (32, 32), (65, 65))  # 0, 1, 63, 64, 65, 130 entries
N_ENTRY_PODS = 140


def entry_world():
    """140 short instance ids and one registry row per entry count (loaded, failed); every row's stored value holds a fails
    member for each failed id and a stale one.  -> (pod ids, stored values, recs)."""
    ids = ["i%d" % k for k in range(N_ENTRY_PODS)]
    stored, recs = [], []
    for r, (nl, nf) in enumerate(ENTRY_COUNTS):
        loaded = [(k, 1000 + k) for k in range(nl)]
        failed = [(N_ENTRY_PODS - 1 - k, -k) for k in range(nf)]
        f = {"mPath": "m%d" % r, "instanceIds": {ids[p]: t for p, t in loaded}, "failedIn": {ids[p]: t for p, t in failed},
             "fails": dict([("stale", {"msg": "s"})] + [(ids[p], {"msg": "e%d" % p}) for p, _ in failed]), "lu": r}
        stored.append(json.dumps({k: v for k, v in f.items() if v not in (0, {})}, separators=SEPS[r % 3]).encode())
        recs.append((0, r, tuple(loaded), tuple(failed)))
    stored.append(b'{"instanceIds":{"ghost":5}}')  # an id no instance has: pod -1, status 2
    recs.append((0, 0, ((-1, 5),), ()))
    return ids, stored, recs


def entry_batch(ids, stored, recs):
    """Every row with its own (long) stored value and with a short old value that holds only the fails object — the tile
    route with up to 66 members of fails — plus a malformed value and a fail_pod on the last failed entry."""
    items = []
    for r, v in enumerate(stored):
        fails = json.loads(v).get("fails", {})
        short = json.dumps({"fails": fails, "k": r}, separators=(",", ":")).encode()
        assert len(short) <= TILE
        fp = recs[r][3][-1][0] if recs[r][3] else -1
        items += [(r, v, r, -1, b""), (r, short, 0, fp, b"late"), (r, short, 0, fp, b"")]
    items.append((0, b'{"a":1', 0, -1, b""))
    return to_batch(items)


MEMBER_COUNTS = (63, 64, 65, 130)
NON_OBJECTS = (b"3", b"null", b'"x"')
PAD = b',"pad":"' + b"p" * TILE + b'"'  # a kept string member behind the others: the value takes the serial route


def fails_object(w, tag):
    """A `fails` object for row 1 (failed: pods 0 and 2) whose kept members name their object: "<tag>-0", "<tag>-2"."""
    p0, p2 = w.pod_ids[0].encode(), w.pod_ids[2].encode()
    return b'{"%s":{"msg":"%s-0"},"stale":{"msg":"s"},"%s":{"msg":"%s-2"}}' % (p0, tag, p2, tag)


def member_layouts(w):
    """[(name, n, {member index: the value of a `fails` member there})]: one `fails` object at member 0, 63, 64 and last of
    values of 63 .. 130 members (the highest lane of a 64-member round and the lanes on both sides of it), and two `fails`
    members inside one round (10, 20) and across a round (10, 70): object then object, object then each kind of non-object, and
    non-objects only."""
    out = []
    for n in MEMBER_COUNTS:
        for at in sorted({0, 63, 64, n - 1}):
            if at < n:
                out.append(("one-%d-%d" % (n, at), n, {at: fails_object(w, b"only")}))
    for a, b in ((10, 20), (10, 70)):
        out.append(("obj-obj-%d" % b, 130, {a: fails_object(w, b"first"), b: fails_object(w, b"second")}))
        for v in NON_OBJECTS:
            out.append(("obj-%s-%d" % (v.decode(), b), 130, {a: fails_object(w, b"first"), b: v}))
        out.append(("non-%d" % b, 130, {a: NON_OBJECTS[0], b: NON_OBJECTS[2]}))
        out.append(("non-msg-%d" % b, 130, {a: NON_OBJECTS[1], b: NON_OBJECTS[0]}))
    return out


def member_value(n, fails_at, sep=0):
    comma, colon = (x.encode() for x in SEPS[sep])
    return b"{" + comma.join(b'"fails"%s%s' % (colon, fails_at[j]) if j in fails_at else b'"f%d"%s%d' % (j, colon, j)
                             for j in range(n)) + b"}"


def member_items(w, pad):
    """One item of row 1 per layout, in the order of member_layouts: the values of up to 65 members in the three separator
    styles in turn; a "-msg" layout brings a message for pod 0, every third one with an object replaces the entry of pod 2."""
    items = []
    for k, (name, n, at) in enumerate(member_layouts(w)):
        old = member_value(n, at, k % 3 if n < 130 else 0)
        assert len(old) <= TILE
        if pad:
            old = old[:-1] + PAD + b"}"
        fp, msg = (0, b"late") if "-msg" in name else (2, b"again") if k % 3 == 2 and name[:3] != "non" else (-1, b"")
        items.append((1, old, k, fp, msg))
    return items


def member_batches(w):
    """HEAD and the member layouts: [on the tile, padded past it]."""
    return [to_batch(head(w) + member_items(w, pad)) for pad in (False, True)]


def run_model(batch, recs, pod_ids, lul=True):
    return mrm.rewrite_batch(batch.olds, recs, batch.rows, pod_ids, batch.last_unload if lul else None, (batch.fail_pod, batch.msgs))


def check_conditions(vals, status):
    """From the model's answer alone: status 0 on at least half of the rows, status 1 and 2 both occur, and each of the five
    owned members is present in some status-0 value and omitted from another."""
    status = list(status)
    assert 2 * status.count(0) >= len(status), status
    assert 1 in status and 2 in status, status
    keys = [{k for k, _, _, _ in mrm.members(v, 0)} for v, st in zip(vals, status) if st == 0]
    for name in OWNED:
        assert any(name in k for k in keys), ("never present", name)
        assert any(name not in k for k in keys), ("never omitted", name)


SIZES = (0, 1, 63, 64, 65, 256, 257)
