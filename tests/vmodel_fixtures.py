"""What tests/test_vmodel_model.py (CPU) and tests/test_vmodels_gpu.py share: a registry drawn by construction so that every kind
of ModelRecord a vmodel question can meet is there, vmodel event batches that hold every outcome, and question batches that hold
every class of every output field.  The CPU test asserts that coverage from the model alone; the GPU test sends the same batches."""
import json

import numpy as np

from tests import vmodel_model as vm

LONG_MAX = (1 << 63) - 1
NOW = 1_700_000_000_000
AGE = 600_000


def model_ids(n):
    """n distinct model ids: the empty id, plain, UTF-8, and pairs where one id is a prefix of the other."""
    ids = [b""] + [(b"m%d" % k, b"m%d-x" % (k - 1), ("mod\u00e8le-%d" % k).encode(), b"model-%05d" % k)[k % 4] for k in range(1, n)]
    assert len(set(ids)) == n
    return ids


MODEL_KINDS = ("loaded1", "loaded3_lu0", "failed_only", "not_loaded", "loaded_lu_max", "empty", "loaded1_failed1", "loaded1_lu1")


def registry_values(pod_ids, n):
    """n stored ModelRecord values, kind k % 8 of MODEL_KINDS, and the (n_loaded, n_failed, last_used, type) each must give."""
    vals, recs = [], []
    for k in range(n):
        kind = MODEL_KINDS[k % len(MODEL_KINDS)]
        p = [pod_ids[(k + j) % len(pod_ids)] for j in range(4)]
        d = {"type": "NLCLASSIFIER"}
        if kind == "loaded1":
            d.update(lu=NOW - 1000 - k, instanceIds={p[0]: NOW - 5000})
        elif kind == "loaded3_lu0":
            d.update(instanceIds={p[0]: 1, p[1]: 2, p[2]: 3})
        elif kind == "failed_only":
            d.update(lu=NOW - 7, failedIn={p[0]: NOW - 9})
        elif kind == "not_loaded":
            d.update(lu=NOW - 11)
        elif kind == "loaded_lu_max":
            d.update(lu=LONG_MAX, instanceIds={p[1]: 4})
        elif kind == "empty":
            d = {}
        elif kind == "loaded1_failed1":
            d.update(lu=5, instanceIds={p[0]: 6}, failedIn={p[3]: 7})
        elif kind == "loaded1_lu1":
            d.update(lu=1, instanceIds={p[2]: 8})
        vals.append(json.dumps(d, separators=(",", ":")))
        recs.append((len(d.get("instanceIds", ())), len(d.get("failedIn", ())), d.get("lu", 0), 0))
    return vals, recs


def vmodel_ids(n, tag=b"vm"):
    ids = []
    for k in range(n):
        ids.append((tag + b"-%d" % k, tag + b"-%d-x" % k, tag + ("-é%d" % k).encode(), tag + b"%03d" % k)[k % 4])
    assert len(set(ids)) == n
    return ids


def record_for(k, mids):
    """The k-th stored VModelRecord of the scenario, by construction: (value, deleted).  mids: the registry's ids; kind j of
    MODEL_KINDS sits at rows j, j + 8, ..."""
    M = len(mids)

    def mid(kind, salt=0):
        j = MODEL_KINDS.index(kind) + 8 * ((k + salt) % (M // 8))
        return mids[j].decode()

    owner = (None, "owner-a", "owner-b", "")[k % 4]
    case = k % 20
    r = vm.render
    if case == 0:
        return r(mid("loaded1"), mid("loaded1"), owner), 0  # DEFINED
    if case == 1:
        return r(mid("loaded1"), mid("loaded1", 1), owner), 0  # TRANSITIONING, target LOADING, ENSURE_LOADED count 1
    if case == 2:
        return r(mid("loaded3_lu0"), mid("failed_only"), owner, failed=True), 0  # TRANSITION_FAILED, LOADING_FAILED, count 3, lu 0
    if case == 3:
        return r(mid("not_loaded"), mid("loaded1"), owner), 0  # PROMOTE (count 0)
    if case == 4:
        return r(mid("loaded_lu_max"), "no-such-model-%d" % k, owner, failed=True), 0  # target unknown: T_NOT_FOUND; lu Long.MAX
    if case == 5:
        return r(mid("loaded1_lu1"), mid("empty"), owner), 0  # target the empty row: T_NOT_FOUND, TO_EMPTY; lu 1
    if case == 6:
        return r(mid("empty"), mid("loaded1"), owner), 0  # FROM_EMPTY, PROMOTE
    if case == 7:
        return r(None, mid("loaded1"), owner), 0  # ACTIVE_NULL
    if case == 8:
        return r(mid("loaded1"), None, owner, failed=True), 0  # TARGET_NULL
    if case == 9:
        return r(None, None, owner), 0  # both null: not in transition
    if case == 10:
        return r("esc\\aped-%d" % k, mid("loaded1"), owner), 0  # HOST: the escape is in amid
    if case == 11:
        return "", 1  # deleted
    if case == 12:
        return r(mid("loaded1"), mid("loaded1"), owner)[:-2], 0  # malformed (truncated)
    if case == 13:
        return r("unknown-active-%d" % k, mid("loaded1_failed1"), owner, failed=True), 0  # from -1; failed but target loaded: LOADING
    if case == 14:
        return r(mid("loaded1"), mid("loaded1"), "own\\ner"), 0  # HOST: the escape is in o
    if case == 15:
        return r(mid("failed_only"), mid("not_loaded"), owner, failed=True,
                 extra='"future":{"a":[1,2,{"b":null}]},"n":-1.5e3,"s":"x","t":true,"z":null'), 0  # unknown members of every type
    if case == 16:
        return '{"amid":"%s","amid":null,"tmid":"%s","failed":true,"failed":false}' % (mid("loaded1"), mid("loaded1")), 0  # later null wins
    if case == 17:
        return '{"amid":7,"amid":"%s","tmid":"%s"}' % (mid("loaded1"), mid("loaded1")), 0  # earlier duplicate of the wrong type
    if case == 18:
        return r("", mid("loaded1"), owner), 0  # amid "" is a string, not null (and the empty model id is registry row 0)
    return " \n" + r(mid("loaded3_lu0"), mid("loaded3_lu0", 2), owner) + "\t ", 0  # blanks around the value


def scenario(n_vm, mids, tag=b"vm"):
    """-> (keys, values, deleted): one event per vmodel id, then a second round over every fifth id in which kinds move on by
    7 (a set row is deleted, a deleted one is set again, a malformed value follows a good one), a deletion of an id that never
    joined, and that id's first value behind it."""
    ids = vmodel_ids(n_vm, tag)
    ev = [(ids[k],) + record_for(k, mids) for k in range(n_vm)]
    ev += [(ids[k],) + record_for(k + 7, mids) for k in range(0, n_vm, 5)]
    late = tag + b"-late"
    ev = [(late, "", 1)] + ev + [(late, vm.render("a", "b"), 0), (late, "", 1), (late, vm.render("a", "a", "o"), 0)]
    keys, values, deleted = (list(x) for x in zip(*ev))
    return keys, values, np.array(deleted, np.uint8)


def questions(model, extra_ids=(b"never-seen", b"")):
    """Question batches over the model's CURRENT rows, by construction: every id of the table and ids in neither, with nf drawn
    from {null, "", active, target, other}, the owner from {null, equal, last byte differs, given}, both phases.
    -> (keys, nf, owners, req_flags)."""
    keys, nf, owners, flags = [], [], [], []
    rng = np.random.default_rng(len(model.ids))
    for v, key in enumerate(list(model.ids) + list(extra_ids)):
        r = model.rows[v] if v < len(model.rows) else None
        a, t, o = (r.amid, r.tmid, r.owner) if r else (None, None, None)
        for _ in range(3):
            keys.append(key)
            nf.append((None, b"", a, t, b"other-id", a)[int(rng.integers(6))])
            owners.append((None, o, (o[:-1] + b"?") if o else b"x", b"owner-given", None, o)[int(rng.integers(6))])
            flags.append(int(rng.integers(2)))
        for after in (0, 1):  # and the nf rule itself in both phases, whatever was drawn
            keys.append(key)
            nf.append(a)
            owners.append(None)
            flags.append(after)
    return keys, nf, owners, np.array(flags, np.uint32)


# ---- malformed and edge values: each is checked against json.loads by the tests before it is sent
MALFORMED = [
    "", " ", "[]", "null", "7", '"amid"', "{", '{"amid":"a"', '{"amid":"a"}}', '{"amid":"a"} x', '{"amid":"a",}', '{,"amid":"a"}',
    '{"amid":"a" "tmid":"b"}', '{"amid":"a",,"tmid":"b"}', '{"amid" "a"}', '{"amid"::"a"}', '{"amid":}', '{"amid":"a}',
    '{"amid":7}', '{"amid":true}', '{"amid":["a"]}', '{"amid":{"a":1}}', '{"tmid":1.5}', '{"o":false}', '{"failed":"true"}',
    '{"failed":1}', '{"failed":null}', '{"failed":tru}', '{"failed":truex}', '{"amid":nul}', '{"amid":nullx}', '{"amid":"a"x}',
    '{"amid":7,"amid":"a"}', '{"failed":0,"failed":true}', '{"o":{},"o":"x"}', '{"amid":"a\\"}',
    '{amid:"a"}', "{'amid':'a'}", '{"amid":"a"}{"tmid":"b"}',
]
EDGE = [
    "{}", " { } ", '{"amid":"a"}', '{"amid":"a","tmid":"a"}', '{"o":"","amid":"","tmid":""}', '{"amid":null,"tmid":null,"o":null}',
    '{"failed":true}', '{"failed":false}', '{"failed" : true , "amid" : "a" }', '{"amid":"a","amid":"b"}', '{"amid":"a","amid":null}',
    '{"amid":null,"amid":"a"}', '{"failed":true,"failed":false}', '{"x":1,"amid":"a","y":[{"amid":7}],"tmid":"b"}',
    '{"amid":"a","z":{"amid":5,"failed":"no"}}', '{"x":"}","amid":"a"}', '{"x":"a\\"b","amid":"c"}', '{"amid":"é","tmid":"日本"}',
    '{"amid":"a\\\\b"}', '{"o":"a\\u0041"}', '{"tmid":"q\\"q"}', '{"amids":"x","amid":"a","ami":"y"}', '{"O":"x","o":"y"}',
    '{"\\u0078":1,"amid":"a"}', '\n{"amid":"a"}\r\n', '{"x":null,"y":true,"z":false,"w":-0.5,"v":"s","u":[],"t":{}}',
]


def padded(total, by_owner):
    """A well-formed value of exactly `total` bytes, padded by a long `o` or by an unknown member."""
    head = '{"amid":"act-%d","tmid":"tgt","failed":true,' % total
    tail = '"o":"%s"}' if by_owner else '"pad":"%s","o":"own"}'
    fill = total - len(head) - len(tail) + 2
    v = head + tail % ("p" * fill)
    assert len(v) == total
    return v


def template_across_chunks(shift):
    """The template value behind `shift` blanks: with shift 0 .. 63 every byte of the template crosses every position of a 64-byte
    scan chunk."""
    return " " * shift + '{"o":"owner\\\\x","amid":"active-model","x":{"y":[1,"]"]},"tmid":null,"failed":true,"tmid":"target"}'
