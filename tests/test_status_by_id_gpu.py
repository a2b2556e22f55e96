"""mmp_models_status_k and mmp_vmodels_status on the device, every comparison exact: against the sequential Python restatement
(tests/status_by_id_model.py) AND against the composition of the existing calls on a quiescent context (model_ids_resolve +
models_status; vmodels_resolve + models_status + vmodels_get).  Sizes at the wavefront and workgroup edges, keys at the 16-byte
chunk edge and beyond the LDS region, colliding hashes, records on both sides of the packed and long emit kernels, the overlay,
every class, the strings and their buffers, refusals, state changes, one-state answers beside a writer, run-to-run identity."""
import json
import threading

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd import workload as wl
from modelmesh_amd._lib import (MST_NOT_FOUND, MSTF_MISS, STATUS_REQ, VMF_ACTIVE_NULL, VMF_OWNER_NULL, VMF_TARGET_NULL, VMR_HOST,
                                VMR_NOT_FOUND, VMR_OK, VMR_STRONG_READ, VSTATUS_ROW)
from modelmesh_amd.solver import Solver
from tests import registry_ops_model as ro
from tests import status_by_id_model as sb
from tests import test_status_by_id_model as cpu
from tests import vmodel_fixtures as fx
from tests import vmodel_model as vm
from tests.model_events_fixtures import World
from tests.registry_ops_model import ModelRecord

pytestmark = pytest.mark.gpu

NOW = 1_700_000_000_000
FILL = 0xA5
P = 8
LENGTHS = [0, 1, 2, 63, 64, 65, 1025]           # entries of the planted records: both sides of the packed / long emit kernels
LONG_ID = b"L" * 200                            # 256 of these in one workgroup are 51 200 key bytes: the byte-by-byte path
EDGE_IDS = [b"x", b"a" * 15, b"b" * 16, b"c" * 17, LONG_ID]
M = 300


# ---- the world by index: a registry of hand-made records, named by id ------------------------------------------------------------

def make_records():
    """M records.  Rows 1..7: the planted lengths, two thirds loaded, instances of the table first and ids the table does not know
    (distinct numbers >= P) behind them, times from a handful of values (ties).  Rows 10, 11: two long records (a vmodel's active and
    target); row 12: nothing but a failure.  Rows 20..24: deleted records (the empty row).  The rest: 0 to 3 entries."""
    rng = np.random.default_rng(505)
    pool = [NOW, NOW - 1, NOW - 2, 0, -1, sb.vm.I64_MASK >> 1, -(1 << 63), NOW + 5]

    def rec(n, lu=5):
        nl = (2 * n + 2) // 3
        pods = list(range(min(n, P))) + list(range(P + 10, P + 10 + max(0, n - P)))
        ent = [(p, int(rng.choice(pool))) for p in pods]
        return ModelRecord(0, ent[:nl], ent[nl:], lu)
    recs = []
    for i in range(M):
        if 1 <= i <= len(LENGTHS):
            recs.append(rec(LENGTHS[i - 1]))
        elif i in (10, 11):
            recs.append(rec(1025 if i == 10 else 200))
        elif i == 12:
            recs.append(ModelRecord(0, [], [(3, NOW - 9)], 5))
        elif 20 <= i <= 24:
            recs.append(ModelRecord(0, [], [], 0))
        else:
            recs.append(rec(int(rng.integers(0, 4)), int(rng.integers(1, 1000))))
    return recs


IDS = fx.model_ids(M - len(EDGE_IDS)) + EDGE_IDS
RECS = make_records()


def fleet_of(records):
    fleet = wl.fuzz_fleet(1511, pods=P, models=1)
    fleet.n_types, fleet.allowed, fleet.prefer, fleet.has_allowed, fleet.has_prefer = 0, None, None, None, None
    fleet.models, fleet.ent_pod, fleet.ent_time = ro.registry_to_arrays(records)
    return fleet


def vmodel_events():
    """A few dozen vmodels by construction over IDS: (keys, values).  Keys of 1, 15, 16 and 17 bytes, non-ASCII keys; strings of 0,
    1, 15, 16 and 17 bytes; null against ""; two vmodels sharing a model; active and target both long; every class."""
    d = lambda b: b.decode()
    r = vm.render
    ev = [(b"v", r(d(IDS[1]), d(IDS[1]), "o")),                                    # a 1-byte key, a record without entries
          (b"k" * 15, r("x", "a" * 15, "b" * 16)),                                 # strings of 1, 15, 16
          (b"k" * 16, r("c" * 17, "c" * 17, "")),                                  # 17; owner "" is not null
          (b"k" * 17, r("", d(IDS[3]), None)),                                     # amid "": the empty id is registry row 0
          ("vmodèle-é".encode(), r(d(IDS[2]), d(IDS[5]), "propriétaire")),
          (b"both-long", r(d(IDS[10]), d(IDS[11]), "o", failed=True)),
          (b"share-1", r(d(IDS[5]), d(IDS[6]))), (b"share-2", r(d(IDS[6]), d(IDS[5]), "o2", failed=True)),
          (b"target-failed", r(d(IDS[4]), d(IDS[12]), failed=True)),                # the target holds nothing but a failure
          (b"active-deleted", r(d(IDS[20]), d(IDS[21]))), (b"target-deleted", r(d(IDS[4]), d(IDS[22]), failed=True)),
          (b"active-unknown", r("no-such", d(IDS[4]))), (b"target-unknown", r(d(IDS[4]), "no-such", failed=True)),
          (b"amid-null", r(None, d(IDS[4]))), (b"tmid-null", r(d(IDS[4]), None)), (b"both-null", r(None, None, "o")),
          (b"host", r("es\\c", d(IDS[4]))), (b"long-id", r(d(LONG_ID), d(LONG_ID), "o"))]
    for k in range(30):                                                            # and the scenario's kinds over the random rows
        a, t = IDS[30 + 7 * k], IDS[30 + 7 * k + (k % 3)]
        ev.append((b"vm-%d" % k, r(d(a) if k % 11 else None, d(t), (None, "owner-a", "owner-b", "")[k % 4], failed=bool(k % 2))))
    return [k for k, _ in ev], [v for _, v in ev]


VKEYS, VVALUES = vmodel_events()


def start(vmodels=True, commit=True, records=RECS, ids=IDS):
    fleet = fleet_of(records)
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    s.load_fleet(fleet, commit=commit)
    s.model_ids_load(ids)
    st = sb.State(ids, list(records))
    if vmodels:
        s.vmodels_events_json(VKEYS + [b"gone"], VVALUES + [vm.render("a", "a")])
        s.vmodels_events_json([b"gone"], [""], np.ones(1, np.uint8))
        st.vmt.events(VKEYS + [b"gone"], VVALUES + [vm.render("a", "a")])
        st.vmt.events([b"gone"], [""], np.ones(1, np.uint8))
    return s, st, [int(x) for x in fleet.pods["id_order"]]


@pytest.fixture(scope="module")
def world():
    """One quiescent context; the tests that use it only ask."""
    s, st, io = start()
    yield s, st, io
    s.close()


# ---- the two references --------------------------------------------------------------------------------------------------------

def compose_models(s, keys, now, fail_pod=None, flags=None):
    """model_ids_resolve + models_status, the -1 a host has to send for deleted records included."""
    idx = s.model_ids_resolve(keys)
    rows = s.get_models()[0]
    empty = (rows["type"] == 0) & (rows["n_loaded"] == 0) & (rows["n_failed"] == 0) & (rows["last_used"] == 0)
    reqs = np.zeros(len(keys), STATUS_REQ)
    reqs["model"] = [(-1 if i < 0 or empty[i] else i) for i in idx]
    reqs["fail_pod"] = -1 if fail_pod is None else fail_pod
    reqs["flags"] = 0 if flags is None else flags
    return (idx,) + tuple(s.models_status(reqs, now))


def compose_vmodels(s, keys, now, owners=None, req_flags=None):
    """vmodels_resolve + models_status on two rows per vmodel + vmodels_get, stitched as a host stitches them."""
    n = len(keys)
    a = s.vmodels_resolve(keys, None, owners, req_flags)
    mrows = s.get_models()[0]
    live = lambda i: i >= 0 and not (mrows[i]["type"] == 0 and mrows[i]["n_loaded"] == 0 and mrows[i]["n_failed"] == 0 and mrows[i]["last_used"] == 0)
    _, vflags, vstr = s.vmodels_get() if int(s.vmodels_info()["n_rows"]) else ([], [], [])
    vrows, reqs, off, blob = np.zeros(n, VSTATUS_ROW), np.zeros(2 * n, STATUS_REQ), [0], b""
    reqs["model"], reqs["fail_pod"] = -1, -1
    for i in range(n):
        cls, v = int(a[i]["cls"]), int(a[i]["vmodel"])
        strings = (None, None, None)
        vrows[i] = (cls, v, -1, -1, 0, 0, 0, 0)
        if cls == VMR_OK:
            m, t = int(a[i]["model"]), int(a[i]["target_model"])
            reqs["model"][2 * i] = m if live(m) else -1
            if int(a[i]["vstatus"]) != _lib.VMS_DEFINED:
                reqs["model"][2 * i + 1] = t if live(t) else -1
            after = bool(req_flags is not None and req_flags[i] & 1)
            if reqs["model"][2 * i] < 0 and not after:
                cls = VMR_STRONG_READ
            vrows[i] = (cls, v, m, t, int(a[i]["vstatus"]), int(a[i]["target_status"]), int(vflags[v]) & _lib.VMF_REPLY, 0)
            strings = vstr[v]
        for x in strings:
            blob += x or b""
            off.append(len(blob))
    rows, copies = s.models_status(reqs, now)
    return dict(vrows=vrows, rows=rows, copies=copies, str_off=np.array(off, np.int32), str_bytes=blob)


def same_status(got, want, what):
    for name, g, w in zip(("model_idx", "rows", "copies"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, name, np.flatnonzero(g != w)[:5])


def ask_vmodels(s, keys, now=NOW, owners=None, req_flags=None):
    """One answer through the raw call, sizes first: a dict in the layout of the references."""
    r = s.vmodels_status_raw(keys, now, 0, 0, owners, req_flags)
    assert r["rc"] == 0, r["rc"]
    r = s.vmodels_status_raw(keys, now, r["n_copies"], r["n_str_bytes"], owners, req_flags)
    assert r["rc"] == 0 and len(r["copies"]) == r["n_copies"] and len(r["str_bytes"]) == r["n_str_bytes"] == r["str_off"][-1]
    return dict(vrows=r["vrows"], rows=r["rows"], copies=r["copies"], str_off=r["str_off"], str_bytes=r["str_bytes"].tobytes())


def same_vstatus(got, want, what):
    for name in ("vrows", "rows", "copies", "str_off"):
        g, w = got[name], want[name]
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, name, np.flatnonzero(g != w)[:5], g[:3], w[:3])
    assert got["str_bytes"] == want["str_bytes"], (what, "str_bytes")


def check_models(s, st, io, keys, fail_pod=None, flags=None, now=NOW, what=""):
    got = s.models_status_k(keys, now, fail_pod, flags)
    same_status(got, sb.models_status_k(st, keys, now, io, fail_pod, flags), (what, "model"))
    same_status(got, compose_models(s, keys, now, fail_pod, flags), (what, "composition"))
    return got


def check_vmodels(s, st, io, keys, owners=None, req_flags=None, now=NOW, what="", compose=True):
    got = ask_vmodels(s, keys, now, owners, req_flags)
    same_vstatus(got, sb.vmodels_status(st, keys, now, io, owners, req_flags), (what, "model"))
    if compose:
        same_vstatus(got, compose_vmodels(s, keys, now, owners, req_flags), (what, "composition"))
    return got


def draw_model_keys(rng, n):
    keys = [IDS[i] for i in range(1, 12)] + [IDS[20], b"no-such-model", IDS[0]] + EDGE_IDS[:4]
    while len(keys) < n:
        keys.append(IDS[int(rng.integers(0, M - 1))] if rng.random() < 0.85 else b"unknown-%d" % int(rng.integers(0, 50)))
    return keys[:n]


def draw_vmodel_questions(rng, n, st):
    keys, owners, flags = [], [], []
    pool = VKEYS + [b"gone", b"never-seen", b""]
    for i in range(n):
        k = pool[i % len(pool)] if i < 2 * len(pool) else pool[int(rng.integers(0, len(pool)))]
        v = st.vmt.row_of.get(k, -1)
        o = st.vmt.rows[v].owner if v >= 0 and st.vmt.rows[v] is not None else None
        keys.append(k)
        owners.append((None, o, (o[:-1] + b"?") if o else b"x", b"", None, o)[(i // len(pool) + i) % 6])
        flags.append(int(rng.integers(0, 2)))
    return keys, owners, np.array(flags, np.uint32)


# ---- sizes ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_wave_and_workgroup_edges(world, n):
    s, st, io = world
    rng = np.random.default_rng(n)
    keys = draw_model_keys(rng, n)
    fail_pod = np.where(rng.random(n) < 0.4, rng.integers(0, P, n), -1).astype(np.int32)
    flags = rng.integers(0, 2, n).astype(np.uint32)
    idx, rows, copies = check_models(s, st, io, keys, fail_pod, flags, what=n)
    assert len(rows) == n and (n < 63 or len(copies) > n)
    check_models(s, st, io, keys, what=(n, "no overlay, no flags"))
    vkeys, owners, vflags = draw_vmodel_questions(rng, n, st)
    got = check_vmodels(s, st, io, vkeys, owners, vflags, what=n)
    assert len(got["vrows"]) == n and len(got["rows"]) == 2 * n
    check_vmodels(s, st, io, vkeys, what=(n, "no owners, no flags"))


# ---- keys ----------------------------------------------------------------------------------------------------------------------

def test_keys_at_the_chunk_edge_and_beyond_the_lds_region(world):
    s, st, io = world
    idx, _, _ = check_models(s, st, io, EDGE_IDS[:4] + [b"y", b"a" * 14, b"b" * 17, b"c" * 16], what="1, 15, 16, 17 bytes")
    assert idx.tolist() == [M - 5, M - 4, M - 3, M - 2, -1, -1, -1, -1]
    # a workgroup whose keys exceed 16 KB next to one that fits, and the other way round; every key of the long one is checked
    for keys in ([LONG_ID] * 255 + [LONG_ID[:-1]] + [IDS[3], IDS[4]] * 20, [IDS[3]] * 256 + [LONG_ID, LONG_ID + b"L"] * 128):
        idx, rows, _ = check_models(s, st, io, keys, what="byte-by-byte path")
        assert (idx == M - 1).sum() in (255, 128)
    check_vmodels(s, st, io, [b"v", b"k" * 15, b"k" * 16, b"k" * 17, b"k" * 14, b"k" * 18, "vmodèle-é".encode(), "vmodèle-e".encode()],
                  what="vmodel keys at the chunk edge")
    big = [b"long-id"] * 3 + [b"V" * 120] * 250 + [b"both-long", b"v"] * 10      # 30 KB of keys, and 250 owners of 100 bytes
    check_vmodels(s, st, io, big, [b"o"] * 3 + [b"w" * 100] * 250 + [b"o", None] * 10, what="vmodel keys and owners beyond the LDS halves")
    check_vmodels(s, st, io, [b"share-1"] * 300 + [b"V" * 120] * 300, what="a staged workgroup next to one that is not")


def test_non_ascii_ids_an_id_asked_twice_and_every_key_unknown(world):
    s, st, io = world
    utf = [k for k in IDS if any(b > 127 for b in k)][:5]
    assert utf
    idx, rows, copies = check_models(s, st, io, utf + utf[:1] + [IDS[6], IDS[6]], what="utf-8, twice")
    assert idx[0] == idx[5] and idx[6] == idx[7] and rows[6]["n_not_checked"] == rows[7]["n_not_checked"] > 0
    idx, rows, copies = check_models(s, st, io, [b"nope-%d" % i for i in range(300)], what="every key unknown")
    assert (idx == -1).all() and (rows["cls"] == MST_NOT_FOUND).all() and len(copies) == 0
    got = check_vmodels(s, st, io, [b"nope-%d" % i for i in range(300)], what="every vmodel key unknown")
    assert (got["vrows"]["cls"] == VMR_NOT_FOUND).all() and got["str_off"][-1] == 0 and len(got["copies"]) == 0
    check_vmodels(s, st, io, ["vmodèle-é".encode()] * 2 + [b"share-1", b"share-2", b"share-1"], what="vmodels twice, sharing a model")


@pytest.mark.parametrize("bits", [0])
def test_the_whole_item_when_every_hash_collides(monkeypatch, bits):
    monkeypatch.setenv("MMP_MODEL_ID_HASH_BITS", str(bits))
    monkeypatch.setenv("MMP_VMODEL_ID_HASH_BITS", str(bits))
    s, st, io = start()
    try:
        test_keys_at_the_chunk_edge_and_beyond_the_lds_region((s, st, io))
        test_non_ascii_ids_an_id_asked_twice_and_every_key_unknown((s, st, io))
    finally:
        s.close()


# ---- records, overlay ----------------------------------------------------------------------------------------------------------

def test_records_on_both_sides_of_the_packed_and_long_kernels(world):
    s, st, io = world
    keys = [IDS[i] for i in range(1, 8)] + [IDS[10], IDS[11]]
    _, rows, copies = check_models(s, st, io, keys, what="planted lengths")
    assert (rows["n_not_checked"] + rows["n_failed"]).tolist() == LENGTHS + [1025, 200]
    got = check_vmodels(s, st, io, [b"both-long", b"share-1", b"share-2", b"both-long"], what="active and target both long; a shared model")
    assert (got["rows"]["n_not_checked"] + got["rows"]["n_failed"]).tolist() == [1025, 200, 64, 65, 65, 64, 1025, 200]


def test_the_overlay_and_the_miss_flag(world):
    s, st, io = world
    i3 = next(i for i in range(30, M) if len(RECS[i].load_failed_instance_ids) == 1)   # loaded on 0 and 1, failed on 2
    assert list(RECS[i3].instance_ids) == [0, 1] and list(RECS[i3].load_failed_instance_ids) == [2]
    for miss in (0, MSTF_MISS):
        keys = [IDS[i3]] * 4 + [IDS[2], IDS[1], IDS[20], b"no-such"] * 2
        fail = [2, 0, 5, -1] + [0, 3, 5, 6, -1, -1, -1, -1]                # among the failed, among the loaded, absent, none
        _, rows, _ = check_models(s, st, io, keys, np.array(fail, np.int32), np.full(len(keys), miss, np.uint32), what=("overlay", miss))
        assert rows[6]["cls"] == rows[7]["cls"] == MST_NOT_FOUND and rows[6]["n_failed"] == rows[7]["n_failed"] == 1
    rec = RECS[3]                                                         # two entries within the table
    among_failed, among_loaded = list(rec.load_failed_instance_ids), list(rec.instance_ids)
    assert among_loaded and all(p < P for p in among_loaded)
    _, rows, _ = check_models(s, st, io, [IDS[3]] * 3, np.array([among_loaded[0], -1, (among_loaded[0] + 3) % P], np.int32), what="loaded / absent")
    assert rows["n_failed"].tolist()[0] == len(among_failed) + 1 and rows["n_not_checked"].tolist()[0] == len(among_loaded) - 1


# ---- classes -------------------------------------------------------------------------------------------------------------------

def test_every_class_occurs_and_the_strong_read_is_answered_after_the_flag(world):
    s, st, io = world
    keys = VKEYS + [b"gone", b"never-seen"] + [b"share-2", b"active-unknown", b"active-deleted", b"amid-null"]
    owners = [None] * (len(VKEYS) + 2) + [b"wrong-owner", None, None, None]
    flags = np.array([0] * (len(VKEYS) + 2) + [0, 1, 1, 1], np.uint32)
    got = check_vmodels(s, st, io, keys, owners, flags, what="classes")
    v = got["vrows"]
    by = dict(zip(keys[:len(VKEYS) + 2], range(len(keys))))
    assert v["cls"][by[b"gone"]] == v["cls"][by[b"never-seen"]] == v["cls"][-4] == VMR_NOT_FOUND       # absent, unknown, owner mismatch
    assert got["vrows"][-4].tobytes() == got["vrows"][by[b"never-seen"]].tobytes()                    # nothing of the record leaks
    assert v["cls"][by[b"host"]] == VMR_HOST and v["cls"][by[b"v"]] == VMR_OK
    assert set(v["vstatus"].tolist()) == {0, 1, 2} and set(v["target_status"].tolist()) == {0, 1, 2, 3}
    for k, j in ((b"active-unknown", -3), (b"active-deleted", -2), (b"amid-null", -1)):
        first, again = v[by[k]], v[j]
        assert first["cls"] == VMR_STRONG_READ and again["cls"] == VMR_OK
        a, b = first.copy(), again.copy()
        a["cls"] = b["cls"] = 0
        assert a.tobytes() == b.tobytes()                                  # the row is filled in either way
        assert got["rows"]["cls"][2 * by[k]] == MST_NOT_FOUND
    assert v["model"][by[b"active-deleted"]] == 20 and v["flags"][by[b"amid-null"]] & VMF_ACTIVE_NULL
    assert set(got["rows"]["cls"].tolist()) == {0, 1, 2, 3}


def test_the_hand_worked_cases_on_the_device():
    recs = [r if r is not None else ModelRecord(0, [], [], 0) for r in cpu.hand_records()]
    s, st, io = start(vmodels=False, records=recs, ids=cpu.MODEL_IDS)
    try:
        for keys, values, deleted in cpu.hand_vmodel_events():
            s.vmodels_events_json(keys, values, deleted)
            st.vmt.events(keys, values, deleted)
        names = list(cpu.CASES)
        q = [cpu.CASES[n][0] for n in names]
        keys, owners, flags = [k for k, _, _ in q], [o for _, o, _ in q], np.array([int(a) for _, _, a in q], np.uint32)
        got = check_vmodels(s, st, io, keys, owners, flags, now=cpu.NOW, what="hand cases")
        want = [cpu.expected(st, n) for n in names]                        # the values written out by hand
        assert [tuple(int(x) for x in r) for r in got["vrows"]] == [w.vrow for w in want]
        for i, w in enumerate(want):
            for j, si in ((2 * i, w.active), (2 * i + 1, w.target)):
                r = got["rows"][j]
                assert (int(r["cls"]), int(r["n_not_checked"]), int(r["n_failed"])) == (si.cls, si.n_not_checked, si.n_failed), (names[i], j)
                o = int(r["copy_off"])
                assert [tuple(int(x) for x in c) for c in got["copies"][o:o + len(si.copies)]] == si.copies, (names[i], j)
            spans = [got["str_bytes"][got["str_off"][3 * i + k]:got["str_off"][3 * i + k + 1]] for k in range(3)]
            assert spans == [x or b"" for x in (w.strings or (None, None, None))], names[i]
        keys = [b"A", b"B", b"C", b"D", b"E", b"", b"nope", b"A", b"A", b"E", b"nope"]
        check_models(s, st, io, keys, np.array([-1, -1, -1, -1, -1, -1, -1, 1, 6, 2, 2], np.int32),
                     np.array([0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0], np.uint32), now=cpu.NOW, what="getStatus by hand")
    finally:
        s.close()


# ---- strings and buffers -------------------------------------------------------------------------------------------------------

def test_strings_null_against_empty_and_the_buffer_protocol(world):
    s, st, io = world
    keys = [b"k" * 15, b"k" * 16, b"k" * 17, b"both-null", b"amid-null", b"both-long", b"never-seen"]
    full = check_vmodels(s, st, io, keys, what="strings")
    off, raw = full["str_off"], full["str_bytes"]
    assert [int(off[i + 1] - off[i]) for i in range(9)] == [1, 15, 16, 17, 17, 0, 0, len(IDS[3]), 0]
    f = full["vrows"]["flags"]
    assert not f[1] & VMF_OWNER_NULL and f[2] & VMF_OWNER_NULL and not f[2] & VMF_ACTIVE_NULL          # "" against null
    assert f[3] & VMF_ACTIVE_NULL and f[3] & VMF_TARGET_NULL
    nc, ns = len(full["copies"]), len(raw)
    assert nc > 1025 and ns > 50
    # sizes only: everything but the two lists
    r = s.vmodels_status_raw(keys, NOW, 0, 0, fill=FILL)
    assert r["rc"] == 0 and (r["n_copies"], r["n_str_bytes"]) == (nc, ns)
    assert r["vrows"].tobytes() == full["vrows"].tobytes() and r["rows"].tobytes() == full["rows"].tobytes()
    assert r["str_off"].tobytes() == off.tobytes()
    # one byte short: the total and the offsets, no bytes; one copy short: the prefix
    r = s.vmodels_status_raw(keys, NOW, nc - 1, ns - 1, fill=FILL)
    assert r["rc"] == 0 and (r["n_copies"], r["n_str_bytes"]) == (nc, ns) and r["str_off"].tobytes() == off.tobytes()
    assert (r["str_bytes"] == FILL).all() and r["copies"].tobytes() == full["copies"][:nc - 1].tobytes()
    r = s.vmodels_status_raw(keys, NOW, nc + 3, ns + 5, fill=FILL, null_str_off=True)
    assert r["rc"] == 0 and r["str_bytes"][:ns].tobytes() == raw and (r["str_bytes"][ns:] == FILL).all()
    assert (r["str_off"].view(np.uint8) == FILL).all()
    # mmp_models_status_k: max_copies zero and one below the total
    mkeys = [IDS[i] for i in range(1, 8)]
    idx, rows, copies = s.models_status_k(mkeys, NOW)
    i0, r0, c0, total, rc = s.models_status_k_raw(mkeys, NOW, 0, fill=FILL)
    assert rc == 0 and total == len(copies) and r0.tobytes() == rows.tobytes() and i0.tobytes() == idx.tobytes() and len(c0) == 0
    i1, r1, c1, total, rc = s.models_status_k_raw(mkeys, NOW, len(copies) - 1, fill=FILL, null_idx=True)
    assert rc == 0 and total == len(copies) and c1.tobytes() == copies[:-1].tobytes() and r1.tobytes() == rows.tobytes()
    assert (i1.view(np.uint8) == FILL).all()


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def untouched(*arrays):
    return all((np.asarray(a).view(np.uint8) == FILL).all() for a in arrays)


def test_refusals_leave_every_output_untouched(world):
    s, st, io = world
    E = _lib.MMP_EINVAL
    keys = [IDS[3], IDS[4], IDS[5]]
    bad_models = [dict(key_off=[0, 5, 3, 9]), dict(fail_pod=[0, P, -1]), dict(fail_pod=[-2, 0, 0]), dict(flags=[0, 2, 0]),
                  dict(fail_pod=[0, -1, -1], now=0), dict(null_out=True)]
    for kw in bad_models:
        now = kw.pop("now", NOW)
        idx, rows, copies, total, rc = s.models_status_k_raw(keys, now, 16, fill=FILL, **kw)
        assert rc == E and total == -1 and untouched(idx, rows, copies), kw
    # more than INT32_MAX copies in all: 2^21 + 1 questions about the 1025-entry record
    n_big = (1 << 21) + 1
    idx, rows, copies, total, rc = s.models_status_k_raw([IDS[7]] * n_big, NOW, 4, fill=FILL)
    assert rc == E and total == -1 and untouched(idx, rows, copies) and b"copies in all" in s.lib.mmp_last_error(s.h)
    vkeys = [b"share-1", b"share-2", b"v"]
    bad_v = [dict(key_off=[0, 9, 7, 15]), dict(owners=[b"a", b"b", b"c"], owner_off=[0, 2, 1, 3]), dict(req_flags=[0, 2, 0]), dict(null_out=True)]
    for kw in bad_v:
        r = s.vmodels_status_raw(vkeys, NOW, 200, 200, fill=FILL, **kw)
        assert r["rc"] == E and r["n_str_bytes"] == -1 and r["n_copies"] == -1, kw
        assert untouched(r["vrows"], r["rows"], r["copies"], r["str_off"], r["str_bytes"]), kw
    r = s.vmodels_status_raw([b"both-long"] * n_big, NOW, 4, 4, fill=FILL)
    assert r["rc"] == E and untouched(r["vrows"], r["rows"], r["copies"], r["str_off"], r["str_bytes"]) and r["n_str_bytes"] == -1


# ---- state ---------------------------------------------------------------------------------------------------------------------

def test_before_the_first_commit_and_without_a_vmodel_call():
    s, st, io = start(vmodels=False, commit=False)
    try:
        check_models(s, st, io, [IDS[3], IDS[20], b"nope"], what="no commit, no fail_pod")
        idx, rows, copies, total, rc = s.models_status_k_raw([IDS[3]], NOW, 4, fail_pod=[0], fill=FILL)
        assert rc == _lib.MMP_ESTATE and untouched(idx, rows, copies)
        got = check_vmodels(s, st, io, [b"v", b"", b"share-1"], [None, b"o", None], what="no vmodel call")
        assert (got["vrows"]["cls"] == VMR_NOT_FOUND).all()
    finally:
        s.close()
    s = Solver(1, 1)
    try:                                                                   # no model-id table: MMP_ESTATE as mmp_model_ids_resolve
        assert s.models_status_k_raw([b"a"], NOW, 0, fill=FILL)[4] == _lib.MMP_ESTATE
        assert s.vmodels_status_raw([b"a"], NOW, 0, 0, fill=FILL)["rc"] == _lib.MMP_ESTATE
    finally:
        s.close()


# the world by key: stored values as the listeners bring them, so that event batches and retirements can follow
W = World(0)


def value_of(mr):
    d = {"type": "NLCLASSIFIER"}
    if mr.last_used:
        d["lu"] = mr.last_used
    if mr.instance_ids:
        d["instanceIds"] = {W.pod_ids[p]: t for p, t in mr.instance_ids.items()}
    if mr.load_failed_instance_ids:
        d["failedIn"] = {W.pod_ids[p]: t for p, t in mr.load_failed_instance_ids.items()}
    return json.dumps(d, separators=(",", ":"))


def keyed_world():
    """12 records by key over W's 8 instances, entries at distinct times (no ties: the stored order of a list does not matter)."""
    ids = [b"m%d" % i for i in range(12)]
    recs = [ModelRecord(0, [((i + j) % P, 1000 * i + j) for j in range(i % 4)], [((i + 5) % P, 1000 * i + 500)] if i % 3 == 0 else [], i + 1)
            for i in range(12)]
    s = W.solver()
    status, _ = s.ingest_models_json([value_of(r) for r in recs])
    assert not status.any()
    s.model_ids_load(ids)
    return s, sb.State(ids, recs)


class Keyed:
    """The device context and the Python state, changed together."""

    def __init__(self):
        self.s, self.st = keyed_world()

    def vmodel(self, key, value, deleted=False):
        d = np.array([deleted], np.uint8)
        self.s.vmodels_events_json([key], [value], d)
        self.st.vmt.events([key], [value], d)

    def model(self, key, mr):
        """mr None: ENTRY_DELETED."""
        self.s.models_events_json([key], [value_of(mr) if mr else ""], np.array([mr is None], np.uint8), True)
        if key not in self.st.models:
            self.st.ids.append(key)
        self.st.models[key] = mr

    def retire_model(self, key):
        row = self.st.ids.index(key)
        remap = self.s.models_retire([row])
        assert remap[row] == -1
        del self.st.ids[row]
        del self.st.models[key]

    def retire_vmodels(self):
        remap, after = self.s.vmodels_retire(all_absent=True)
        t, old = vm.VModels(), self.st.vmt
        for k, r in zip(old.ids, old.rows):
            if r is not None:
                t.row_of[k] = len(t.ids)
                t.ids.append(k)
                t.rows.append(r)
        self.st.vmt = t
        assert after == len(t.ids)


QKEYS = [b"X", b"Y", b"Z", b"X", b"never"]


def test_answers_follow_event_batches_and_retirements():
    k = Keyed()
    try:
        k.vmodel(b"Y", vm.render("m1", "m2", "oy"))
        k.vmodel(b"Z", vm.render("m9", "m9"))
        k.vmodel(b"X", vm.render("m3", "m6", "ox", failed=True))
        check_vmodels(k.s, k.st, None, QKEYS, what="start")
        check_models(k.s, k.st, None, k.st.ids + [b"nope"], what="start")
        k.model(b"m3", ModelRecord(0, [(1, 77)], [(2, 88)], 9))           # events without a commit
        k.model(b"m6", None)
        k.model(b"m12", ModelRecord(0, [(4, 5)], [], 3))
        k.vmodel(b"Z", vm.render("m12", "m3", "oz"))
        got = check_vmodels(k.s, k.st, None, QKEYS, what="after event batches")
        assert got["vrows"]["target_status"][0] == _lib.VMT_NOT_FOUND and got["vrows"]["model"][2] == 12
        check_models(k.s, k.st, None, k.st.ids + [b"nope"], what="after event batches")
        k.retire_model(b"m6")                                              # rows renumbered: the answers follow
        k.retire_model(b"m0")
        got = check_vmodels(k.s, k.st, None, QKEYS, what="after models_retire")
        assert got["vrows"]["model"][2] == 10 and got["vrows"]["target_model"][0] == -1
        idx, _, _ = check_models(k.s, k.st, None, [b"m12", b"m6", b"m0", b"m1"], what="after models_retire")
        assert idx.tolist() == [10, -1, -1, 0]
        k.vmodel(b"Y", "", deleted=True)
        k.retire_vmodels()                                                 # vmodel rows renumbered
        got = check_vmodels(k.s, k.st, None, QKEYS, what="after vmodels_retire")
        assert got["vrows"]["vmodel"].tolist() == [1, -1, 0, 1, -1]
    finally:
        k.s.close()


def test_every_answer_beside_a_writer_is_of_one_state():
    """A second thread takes the context round a cycle of five calls — the named model deleted, its row retired, the vmodel's record
    rewritten, the model joined again with another copy list, the record written back — while this one asks 200 times.  Each call is
    one hold of the batch lock, and so is each answer: it must be, whole, the Python model's answer for the state between two of
    those calls, never a mix.  The two principal states differ in every field that can differ for one vmodel id."""
    k = Keyed()
    try:
        rec_a, rec_b = vm.render("mP", "mP", "owner-a"), vm.render("ghost", "m3", "owner-bb", failed=True)
        copies_a = ModelRecord(0, [(1, 50), (2, 60)], [], 4)
        k.vmodel(b"Y", vm.render("m1", "m2", "oy"))
        k.model(b"mP", copies_a)
        k.vmodel(b"X", rec_a)
        steps = [lambda: k.model(b"mP", None), lambda: k.retire_model(b"mP"), lambda: k.vmodel(b"X", rec_b),
                 lambda: k.model(b"mP", copies_a), lambda: k.vmodel(b"X", rec_a)]
        keys = [b"X", b"Y", b"X"]

        def model_answer():
            w = sb.vmodels_status(k.st, keys, NOW, None)
            return b"".join(w[n].tobytes() for n in ("vrows", "rows", "copies", "str_off")) + w["str_bytes"]
        states = [model_answer()]                                          # the cycle once on a quiet context: every state's answer
        quiet = []
        for step in steps:
            quiet.append(check_vmodels(k.s, k.st, None, keys, what="quiet cycle"))
            step()
            states.append(model_answer())
        assert states[-1] == states[0] and states[3] == states[4] and len(set(states)) == 4
        a, b = quiet[0], quiet[3]                                          # the two principal states
        for f in ("cls", "model", "target_model", "vstatus", "target_status", "flags"):
            assert a["vrows"][f][0] != b["vrows"][f][0], f
        assert a["rows"][:2].tobytes() != b["rows"][:2].tobytes() and a["str_bytes"] != b["str_bytes"] and len(a["copies"]) != len(b["copies"])
        stop, errors = threading.Event(), []

        def writer():
            try:
                while not stop.is_set():
                    for step in steps:
                        step()
            except Exception as e:  # noqa: BLE001
                errors.append(e)
        t = threading.Thread(target=writer)
        t.start()
        seen = []
        try:
            for _ in range(200):
                vrows, rows, copies, strings = k.s.vmodels_status(keys, NOW)
                r = k.s.vmodels_status_raw(keys, NOW, len(copies) + 8, 256)
                assert r["rc"] == 0
                ns = r["n_str_bytes"]
                seen.append(b"".join(r[n].tobytes() for n in ("vrows", "rows")) + r["copies"][:r["n_copies"]].tobytes() + r["str_off"].tobytes() + r["str_bytes"][:ns].tobytes())
        finally:
            stop.set()
            t.join()
        assert not errors, errors
        valid = set(states)
        assert all(x in valid for x in seen), sum(x not in valid for x in seen)
        assert states[0] in seen and states[3] in seen, (seen.count(states[0]), seen.count(states[3]))
    finally:
        k.s.close()


# ---- determinism ---------------------------------------------------------------------------------------------------------------

def test_two_runs_are_byte_identical(world):
    s, st, io = world
    rng = np.random.default_rng(77)
    keys = draw_model_keys(rng, 700)
    fail_pod = np.where(rng.random(700) < 0.4, rng.integers(0, P, 700), -1).astype(np.int32)
    vkeys, owners, vflags = draw_vmodel_questions(rng, 700, st)
    runs = []
    for _ in range(3):
        a = s.models_status_k(keys, NOW, fail_pod)
        b = ask_vmodels(s, vkeys, NOW, owners, vflags)
        runs.append(b"".join(x.tobytes() for x in a) + b"".join(b[n].tobytes() for n in ("vrows", "rows", "copies", "str_off")) + b["str_bytes"])
    assert runs[0] == runs[1] == runs[2]
