"""The values the wire-format parser tests feed to the device (tests/test_ingest_paths_gpu.py, tests/ingest_group_child.py), and
what tests/ingest_model.py says about them.  Everything is built from fixed seeds: a child process builds the same batches.

No builder may emit a value of the UNSPECIFIED class; tests/test_ingest_model.py asserts it for every one of them."""
import functools
import json

import numpy as np

from tests import ingest_model as im
from tests.test_ingest_gpu import MALFORMED_MODELS, WELL_FORMED_MODELS, _rand_json

TILE = 2048  # kJTileBytes: a longer record is walked by one lane
N_IDS = 50
IDS = ["p%d" % i for i in range(N_IDS)]
POD_OF = {s: i for i, s in enumerate(IDS)}
TYPE_NAMES = ["NLCLASSIFIER", "t1", "t2"]
UNKNOWN_TYPE = 3

DUPLICATE_MODELS = [
    # an earlier, longer duplicate must leave nothing behind; failedIn's entries follow the winner's
    '{"failedIn":{"p1":4},"instanceIds":{"p2":1,"p3":2,"p4":3},"instanceIds":{"p5":9}}',
    '{"instanceIds":{"p1":4},"failedIn":{"p2":1,"p3":2,"p4":3},"failedIn":{"p5":9}}',
    '{"instanceIds":{"p2":1,"p3":2,"p4":3},"failedIn":{"p1":4,"p6":5},"instanceIds":{"p5":9,"p7":8},"failedIn":{"p8":6}}',
    '{"instanceIds":{"p1":1,"p2":2},"instanceIds":null,"failedIn":{"p3":3}}',
    '{"instanceIds":{"p1":1},"instanceIds":{},"failedIn":null,"failedIn":{"p3":3,"p4":4}}',
    '{"type":"t1","type":"t2","lul":3,"lul":4,"lu":1,"lu":2}',
    '{"type":"t1","type":null,"lu":1}',
    '{"lu":"5","lu":6}',                                        # the earlier duplicate has the wrong type: rejected
    '{"instanceIds":{"p1":"x"},"instanceIds":{"p1":1}}',
]


def straddle(first, second, n_before=63):
    """Two duplicates of a map behind `n_before` other fields: with 63, the duplicates are fields 63 and 64 of the record — the
    last lane of one 64-lane field round and the first of the next, when the record is the first of its wavefront."""
    return "{" + "".join('"f%d":0,' % k for k in range(n_before)) + '"instanceIds":%s,"instanceIds":%s}' % (first, second)


STRADDLE_MODELS = [
    straddle('{"p1":"x"}', '{"p1":1}'),                         # the earlier duplicate, of an earlier round, is malformed: rejected
    straddle('{"p1":1,"p2":2}', '{"p3":3}'),
    straddle('{"p1":1}', '{"p3":}'),
    straddle('{"p1":1,"p2":2}', 'null'),
    # a failedIn pair split over the rounds as well, the one of the earlier round malformed
    '{"failedIn":{"p4":"x"},' + straddle('{"p1":5,"p2":6}', '{"p3":3}', 62)[1:-1] + ',"failedIn":{"p4":4}}',
]
DUPLICATE_MODELS += STRADDLE_MODELS

# rejected for an earlier duplicate only: a parser built on a dict of the last occurrences cannot know
TWIN_BLIND = tuple(v.encode() for v in DUPLICATE_MODELS[7:9] + [STRADDLE_MODELS[0], STRADDLE_MODELS[4]])

EXTREME_MODELS = [
    '{"lu":-9223372036854775808,"lul":9223372036854775807}',
    '{"lu":9223372036854775807,"lul":-9223372036854775808}',
    '{"lu":2147483647,"lul":-2147483648}',
    '{"instanceIds":{"p1":-9223372036854775808,"p2":9223372036854775807},"failedIn":{"p3":2147483647,"p4":-2147483648}}',
    '{"lu":-0,"lul":0}',
]

# the InstanceRecord values of test_ingest_gpu.test_malformed_and_edge_case_values, and a value that closes twice
POD_VALUES = ['{"count":3,"cap":10}', '{"count":3,"cap":10', '{"count":"3"}', '{"shutdown":1}', '{"shutdown":true,"rpm":4}',
              '{"count":3 "cap":10}', '{}', '{"labels":["a","b"],"count":2}', '{"count":2,}', 'null', '{"cap":5}}']
EXTREME_PODS = [
    '{"lruTime":-9223372036854775808,"cap":9223372036854775807,"used":9223372036854775807,"vers":-9223372036854775808}',
    '{"count":2147483647,"lThreads":-2147483648,"lInProg":2147483647,"rpm":-2147483648,"startTime":9223372036854775807}',
    '{"cap":5} {"cap":6}', '{"cap":5,"cap":6,"shutdown":true,"shutdown":false}', '', '  ', '{"rpm":1.5}', '{"shutdown":"true"}',
]

_SEPS = [(",", ":"), (", ", ": "), (" ,\n ", " :\t")]


def _dump(rng, d):
    items = list(d.items())
    rng.shuffle(items)
    return json.dumps(dict(items), separators=_SEPS[int(rng.integers(0, 3))], ensure_ascii=bool(rng.integers(0, 2))).encode()


def random_models(seed, n):
    """Well-formed ModelRecord values: known fields of the right type in random positions between random junk fields whose values
    nest, escape and contain every structural character (the generator of test_random_documents_agree_with_a_json_library)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        d = {}
        for j in range(int(rng.integers(0, 5))):
            d["junk%d" % j] = _rand_json(rng)
        if rng.random() < 0.7:
            d["type"] = str(rng.choice(["t1", "t2", "NLCLASSIFIER", "unheard-of"]))
        if rng.random() < 0.7:
            d["lu"] = int(rng.integers(0, 10**13))
        if rng.random() < 0.5:
            d["lul"] = int(rng.integers(-5, 10**13))
        for fld in ("instanceIds", "failedIn"):
            if rng.random() < 0.7:
                pods = sorted(rng.choice(N_IDS, int(rng.integers(0, 5)), replace=False).tolist(), key=lambda p: IDS[p])
                d[fld] = {(IDS[p] if rng.random() < 0.9 else "gone-%d" % p): int(rng.integers(1, 10**13)) for p in pods}
        out.append(_dump(rng, d))
    return out


def random_pods(seed, n):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        d = {}
        for f, kind in im.POD_FIELDS.items():
            if rng.random() < 0.6:
                d[f] = bool(rng.integers(0, 2)) if kind == "bool" else int(rng.integers(-3, 2**31 if kind == "int" else 10**13))
        if rng.random() < 0.5:
            d["loc"] = "rack \"%d\"\\" % rng.integers(0, 9)
        if rng.random() < 0.5:
            d["labels"] = ["l%d,:{" % k for k in range(int(rng.integers(0, 4)))]
        for j in range(int(rng.integers(0, 3))):
            d["junk%d" % j] = _rand_json(rng)
        out.append(_dump(rng, d))
    return out


def _prefixes(seed, values):
    rng = np.random.default_rng(seed)
    return [v[:int(rng.integers(0, len(v)))] for v in values]


@functools.lru_cache(None)
def model_corpus():
    """The two lists of test_ingest_gpu, the duplicate-field cases, the integer extremes, 300 random documents and one random
    strict prefix of each of the first 100 of them.  A tuple of bytes."""
    docs = random_models(9200, 300)
    fixed = MALFORMED_MODELS + [v for v, _ in WELL_FORMED_MODELS] + DUPLICATE_MODELS + EXTREME_MODELS
    return tuple([v.encode() for v in fixed] + docs + _prefixes(9201, docs[:100]))


@functools.lru_cache(None)
def pod_corpus():
    docs = random_pods(9300, 100)
    return tuple([v.encode() for v in POD_VALUES + EXTREME_PODS] + docs + _prefixes(9301, docs[:40]))


# ---- the same value, longer ------------------------------------------------------------------------------------------------

def blanks_front(v, total=TILE + 1):
    return b" " * max(total - len(v), 0) + v


def blanks_behind(v, total=TILE + 1):
    return v + b" " * max(total - len(v), 0)


def pad_field(v, total=TILE + 1):
    """A first field "pad":"aaa..." that brings a value starting with '{' to `total` bytes (at least one 'a')."""
    assert v[:1] == b"{"
    body = v[1:]
    head, tail = b'{"pad":"', b'"' if body.lstrip(b" \t\n\r")[:1] == b"}" else b'",'
    return head + b"a" * max(total - len(head) - len(tail) - len(body), 1) + tail + body


def forms(v, cls):
    """The forms of B.1: as it stands, blanks in front / behind up to 2 049 bytes, and (well-formed values that start with '{')
    a first field of padding."""
    out = [v, blanks_front(v), blanks_behind(v)]
    if cls == im.ACCEPT and v[:1] == b"{":
        out.append(pad_field(v))
    return out


def sized(nbytes, lu, n_inst=0, n_fail=0, typ="t1"):
    """A well-formed ModelRecord value of exactly `nbytes` bytes."""
    d = {"type": typ, "lu": lu, "instanceIds": {IDS[(lu + k) % N_IDS]: lu * 100 + k for k in range(n_inst)},
         "failedIn": {IDS[(lu + 7 + k) % N_IDS]: lu * 100 + 50 + k for k in range(n_fail)}}
    v = pad_field(json.dumps(d, separators=(",", ":")).encode(), nbytes)
    assert len(v) == nbytes, (len(v), nbytes)
    return v


def sized_pod(nbytes, k):
    v = pad_field(json.dumps({"count": k, "cap": 10 * k, "lruTime": 10**12 + k, "shutdown": bool(k & 1)}, separators=(",", ":")).encode(),
                  nbytes)
    assert len(v) == nbytes
    return v


def five_byte_record(n):
    """n entries of five bytes: 17 + 5n bytes (the last entry has no comma, the braces make up for it)."""
    v = ('{"instanceIds":{' + ",".join('"":%d' % (k % 10) for k in range(n)) + "}}").encode()
    assert len(v) == 17 + 5 * n
    return v


def overclaiming_record(n):
    """n two-byte look-alikes of an entry and one real entry behind them: malformed."""
    return ('{"instanceIds":{' + ":," * n + '"":1}}').encode()


def planted_models(n, seed=5):
    """n records drawn from the corpus by index, with these shapes planted at fixed positions of their 8-record wavefronts
    (all below record 2 000): eight values of 256 bytes; eight of 257; a value longer than the tile at positions 0, 3 and 7; an
    empty value and a {} inside a group; a rejected value between accepted ones; a group with more than 64 fields; a group with
    more than 64 map entries; a record of 40 five-byte entries and one that announces 40 entries in 97 bytes, each with ten
    ordinary records of 120 bytes behind it; three groups in which the edge between two 64-lane field rounds falls between two
    duplicates of instanceIds (the earlier malformed; both well-formed; the later malformed)."""
    C = model_corpus()
    rng = np.random.default_rng(seed)
    vals = [C[k] for k in rng.integers(0, len(C), n)]
    plant = {}
    for k in range(8):
        plant[16 + k] = sized(256, 10 + k, 2, 1)
        plant[32 + k] = sized(257, 20 + k, 1, 2)
        plant[128 + k] = json.dumps(dict([("f%d" % j, j) for j in range(6)] + [("lu", 30 + k)] + [("g%d" % j, [j]) for j in range(5)]),
                                    separators=(",", ":")).encode()
        plant[144 + k] = sized(200, 40 + k, 7, 3, "t2")
    plant[48 + 0] = sized(2300, 50, 30, 10)
    plant[64 + 3] = sized(TILE + 1, 51, 3, 40)
    plant[80 + 7] = sized(3000, 52, 0, 2)
    plant[96 + 2], plant[96 + 5] = b"", b"{}"
    plant[112 + 2], plant[112 + 3], plant[112 + 4] = sized(100, 60, 2, 1), b'{"lu": 5,}', sized(101, 61, 1, 2)
    plant[160 + 1] = five_byte_record(40)
    plant[192 + 1] = overclaiming_record(40)
    for k in range(10):
        plant[160 + 2 + k] = sized(120, 70 + k, 2, 1)
        plant[192 + 2 + k] = sized(120, 80 + k, 1, 1)
    # a group whose round edge falls between two duplicates: 31 + 31 fields, then lu, instanceIds (field 63), instanceIds (64)
    for k in range(3):
        w = 208 + 8 * k
        plant[w], plant[w + 1] = (json.dumps({"f%d" % j: j for j in range(31)}, separators=(",", ":")).encode(),) * 2
        plant[w + 2] = ('{"lu":%d,"instanceIds":%s,"instanceIds":%s}'
                        % (w, ('{"p1":"x"}', '{"p1":1,"p2":2}', '{"p1":1}')[k], ('{"p1":1}', '{"p3":3}', '{"p3":}')[k])).encode()
        for j in range(3, 8):
            plant[w + j] = sized(100, 90 + j, 1, 1)
    for pos, v in plant.items():
        if pos < n:
            vals[pos] = v
    return vals


def planted_pods(n, seed=6):
    C = pod_corpus()
    rng = np.random.default_rng(seed)
    vals = [C[k] for k in rng.integers(0, len(C), n)]
    plant = {}
    for k in range(8):
        plant[16 + k] = sized_pod(256, 10 + k)
        plant[32 + k] = sized_pod(257, 20 + k)
        plant[128 + k] = json.dumps(dict([("f%d" % j, j) for j in range(6)] + [("rpm", 30 + k)] + [("g%d" % j, [j]) for j in range(5)]),
                                    separators=(",", ":")).encode()
    plant[48 + 0], plant[64 + 3], plant[80 + 7] = sized_pod(2300, 50), sized_pod(TILE + 1, 51), sized_pod(3000, 52)
    plant[96 + 2], plant[96 + 5] = b"", b"{}"
    plant[112 + 2], plant[112 + 3], plant[112 + 4] = sized_pod(100, 60), b'{"count":2,}', sized_pod(101, 61)
    for pos, v in plant.items():
        if pos < n:
            vals[pos] = v
    return vals


# ---- what the reference says, as arrays ------------------------------------------------------------------------------------

_model_cache, _pod_cache = {}, {}


def model_answer(v):
    a = _model_cache.get(v)
    if a is None:
        a = _model_cache[v] = im.model_bean(v, POD_OF, TYPE_NAMES, UNKNOWN_TYPE)
    return a


def pod_answer(v):
    a = _pod_cache.get(v)
    if a is None:
        a = _pod_cache[v] = im.pod_bean(v)
    return a


def check_models(values, status, lul, rows, ent_pod, ent_time, like=None):
    """Exact equality of one full reload with the reference: status, type, n_loaded, n_failed, last_used, lul, ent_off (the
    running sum of the counts) and the (pod, time) entries.  A rejected value has no entries and lul 0, and the row every
    rejected record gets (the default type, last_used 0).  `like[i]`: the value whose answer record i must give (default: itself).
    Returns a list of differences (empty: equal)."""
    ans = [model_answer(v) for v in (values if like is None else like)]
    n = len(values)
    default = TYPE_NAMES.index("NLCLASSIFIER")
    want = {"status": [a.status for a in ans], "type": [default if a.status else a.type for a in ans],
            "n_loaded": [len(a.loaded) for a in ans], "n_failed": [len(a.failed) for a in ans],
            "last_used": [a.lu for a in ans], "lul": [a.lul for a in ans]}
    cnt = np.array(want["n_loaded"], np.int64) + np.array(want["n_failed"], np.int64)
    want["ent_off"] = np.concatenate([[0], np.cumsum(cnt)[:-1]]) if n else np.zeros(0, np.int64)
    got = {"status": status, "lul": lul}
    got.update({f: rows[f] for f in ("type", "n_loaded", "n_failed", "last_used", "ent_off")})
    diffs = []
    if len(rows) != n:
        return ["%d rows for %d values" % (len(rows), n)]
    for f, w in want.items():
        w = np.array(w, dtype=np.int64)
        bad = np.nonzero(np.asarray(got[f]).astype(np.int64) != w)[0]
        for i in bad[:3]:
            diffs.append("record %d %s: got %d, want %d; value %r" % (i, f, got[f][i], w[i], bytes(values[i][:120])))
    ents = [e for a in ans for e in a.loaded + a.failed]
    wp, wt = np.array([p for p, _ in ents], np.int32), np.array([t for _, t in ents], np.int64)
    if len(ent_pod) != len(wp):
        diffs.append("%d entries, want %d" % (len(ent_pod), len(wp)))
    elif not (np.array_equal(ent_pod, wp) and np.array_equal(ent_time, wt)):
        e = int(np.nonzero((ent_pod != wp) | (ent_time != wt))[0][0])
        i = int(np.searchsorted(want["ent_off"], e, side="right")) - 1
        diffs.append("entry %d (record %d, entry %d of it): got (%d, %d), want (%d, %d); value %r"
                     % (e, i, e - want["ent_off"][i], ent_pod[e], ent_time[e], wp[e], wt[e], bytes(values[i][:120])))
    return diffs


POD_ROW_FIELDS = ("lru_time", "count", "capacity", "used", "loading_threads", "loading_in_progress", "rpm", None, None, "version")


def check_pods(values, status, start_time, rows, before, like=None):
    """Record i is pod i.  Exact equality with the reference: status, the ten fields; a rejected value leaves its row as it was
    (`before`).  Returns a list of differences."""
    ans = [pod_answer(v) for v in (values if like is None else like)]
    n = len(values)
    diffs = []
    st = np.array([a[0] for a in ans], np.int64)
    bad = np.nonzero(status.astype(np.int64) != st)[0]
    for i in bad[:3]:
        diffs.append("record %d status: got %d, want %d; value %r" % (i, status[i], st[i], bytes(values[i][:120])))
    ok = st == 0
    zero = (0,) * 10
    for k, f in enumerate(POD_ROW_FIELDS):
        w = np.array([(a[1] if a[0] == 0 else zero)[k] for a in ans], np.int64)
        if k == 7:
            g, name = (rows["flags"][:n] & 1).astype(np.int64), "shutdown"
        elif k == 8:
            g, name = np.where(ok, start_time, 0).astype(np.int64), "startTime"
        else:
            g, name = rows[f][:n].astype(np.int64), f
        bad = np.nonzero(ok & (g != w))[0]
        for i in bad[:3]:
            diffs.append("record %d %s: got %d, want %d; value %r" % (i, name, g[i], w[i], bytes(values[i][:120])))
    if not np.array_equal(rows[:n][~ok], before[:n][~ok]):
        diffs.append("a rejected value changed its row")
    if not np.array_equal(rows[:n]["flags"][ok] & 2, np.full(int(ok.sum()), 2, np.uint32)):
        diffs.append("an ingested row lost its LIVE flag")
    return diffs


# ---- positions relative to the 64-byte scan chunks and to the tile edge ------------------------------------------------------

CHUNK_MODELS = [
    rb'{"mPath":"ab\"","lu":7,"type":"t1"}',                                  # a junk string that ends in an escaped quote
    rb'{"mPath":"ab\\","lu":7,"type":"t1"}',                                  # ... in an escaped backslash
    rb'{"a":"x\"y","b":"x\\y","c":"x\\\"y","d":"x\\\\y","e":"\\\\","lu":7}',  # backslash runs of 1, 2, 3 and 4
    rb'{"mPath":"m","instanceIds":{"p1":11,"p2":12},"lu":7}',
    rb'{"type":"t2","lu":1234567890123}',
    rb'{"lu":7,"failedIn":null,"lul":8}',
]
CHUNK_PODS = [
    rb'{"loc":"ab\"","rpm":7,"count":1}',
    rb'{"loc":"ab\\","rpm":7,"count":1}',
    rb'{"a":"x\"y","b":"x\\y","c":"x\\\"y","d":"x\\\\y","e":"\\\\","rpm":7}',
    rb'{"zone":"z","labels":{"p1":11,"p2":12},"cap":7}',
    rb'{"count":2,"lruTime":1234567890123}',
    rb'{"rpm":7,"shutdown":true,"used":8}',
]


def _shifted(templates):
    """Every template behind 0..127 blanks: each of its bytes falls once on either side of the first two chunk edges."""
    return [b" " * k + t for t in templates for k in range(128)]


def chunk_edge_models():
    return _shifted(CHUNK_MODELS)


def chunk_edge_pods():
    return _shifted(CHUNK_PODS)


def tile_edge_models():
    """-> (values, like).  A well-formed and a malformed template brought to 2 046..2 050 bytes (by a first field of padding and
    by blanks behind), each at every alignment of its first byte modulo 4: a filler record `{}` + blanks in front of it sets the
    alignment (the fillers are 2..5 bytes long, so lengths 1, 2 and 3 modulo 4 all occur)."""
    good, bad = b'{"type":"t1","lu":77,"instanceIds":{"p3":5,"p4":6},"failedIn":{"p5":7},"lul":9}', b'{"lu": 5,"instanceIds":{"p3":5,}}'
    vals, like, off = [], [], 0
    for t in (good, bad):
        for pad in (pad_field, blanks_behind):
            for total in range(TILE - 2, TILE + 3):
                for align in range(4):
                    filler = b"{}" + b" " * ((align - off - 2) % 4)
                    off += len(filler)
                    assert off % 4 == align
                    v = pad(t, total)
                    assert len(v) == total
                    off += total
                    vals += [filler, v]
                    like += [b"{}", t]
    return vals, like
