"""The vmodel table on the device (mmp_vmodels_events_json / _resolve / _transitions / _get / _info) held to tests/vmodel_model.py
byte for byte, on an 8-instance fleet with 300 ModelRecords loaded by key (tests/vmodel_fixtures.py) unless stated otherwise.  The
registry the model looks ids up in is read back from the device (mmp_models_get / mmp_model_ids_get: pinned by their own tests).
tests/test_vmodel_model.py asserts, on the CPU, that the scenario batches hold every class of every output field."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd.solver import MmpError
from tests import vmodel_fixtures as fx
from tests import vmodel_model as vm
from tests.ingest_model import ACCEPT, REJECT
from tests.model_events_fixtures import World

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 300
WORLD = World(0)
MIDS = fx.model_ids(M)
REG_VALUES, REG_RECS = fx.registry_values(WORLD.pod_ids, M)
FILL = 0xA5


def start(n_models=M):
    s = WORLD.solver()
    st, _ = s.ingest_models_json(REG_VALUES[:n_models])
    assert not st.any()
    s.model_ids_load(MIDS[:n_models])
    return s


def registry_of(s):
    rows = s.get_models()[0]
    return vm.Registry(s.model_ids_get(), [(r["n_loaded"], r["n_failed"], r["last_used"], r["type"]) for r in rows])


def tab_capacity(n):
    cap = 16
    while cap < 2 * n:
        cap *= 2
    return cap


def check_table(s, m, what=""):
    ids, flags, strings = s.vmodels_get()
    assert ids == m.ids, what
    assert np.array_equal(flags, m.flags()), (what, np.nonzero(flags != m.flags())[0][:8])
    assert strings == m.strings(), what
    info = s.vmodels_info()
    n_rows, n_live, live_bytes = m.info()
    assert (info["n_rows"], info["n_live"], info["live_bytes"]) == (n_rows, n_live, live_bytes), (what, info)
    assert live_bytes <= info["arena_bytes"] <= 2 * live_bytes, (what, info)  # garbage never exceeds the live bytes after a call
    if n_rows:
        assert info["capacity"] >= tab_capacity(n_rows), what


def answers(a):
    return [tuple(int(x) for x in r) for r in a]


def check_questions(s, m, what="", reg=None):
    reg = reg or registry_of(s)
    keys, nf, owners, flags = fx.questions(m)
    got = s.vmodels_resolve(keys, nf, owners, flags)
    want = m.resolve_many(reg, keys, nf, owners, flags)
    bad = [i for i, (g, w) in enumerate(zip(answers(got), want)) if g != tuple(w)]
    assert not bad, (what, bad[:5], keys[bad[0]], nf[bad[0]], owners[bad[0]], flags[bad[0]], answers(got)[bad[0]], want[bad[0]])
    # the optional buffers left out: all null, phase one
    got = s.vmodels_resolve(keys)
    assert answers(got) == [tuple(a) for a in m.resolve_many(reg, keys)], what
    return got


def check_transitions(s, m, what="", reg=None, now=fx.NOW, age=fx.AGE):
    reg = reg or registry_of(s)
    rows, info = s.vmodels_transitions(now, age)
    want, winfo = m.transitions(reg, now, age)
    assert answers(rows) == [tuple(t) for t in want], what
    assert (info["n_listed"], info["n_promote"], info["n_ensure_loaded"], info["n_host_skipped"], info["truncated"]) == winfo + (0,), what
    return rows


def send(s, m, keys, values, deleted=None, append=True, what=""):
    want = m.events(keys, values, deleted, append)
    got = s.vmodels_events_json(keys, values, deleted, append)
    for name, g, w in zip(("status", "vmodel_idx"), got, want):
        assert np.array_equal(g, w), (what, name, np.nonzero(g != w)[0][:8])
    assert got[2] == want[2], what
    return got


# ---- events ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_vm", [0, 1, 63, 64, 65, 257])
def test_scenario_batches(n_vm):
    s, m = start(), vm.VModels()
    try:
        assert tuple(s.vmodels_info()) == (0, 0, 0, 0, 0, 0)  # no state before the first call
        check_transitions(s, m, "empty")
        if n_vm == 0:
            st, idx, n_app = s.vmodels_events_json([], [])
            assert len(st) == 0 and n_app == 0 and tuple(s.vmodels_info()) == (0, 0, 0, 0, 0, 0)
            assert answers(s.vmodels_resolve([b"x"])) == [(0, 0, -1, -1, -1, 0, 0, 0)]
            return
        keys, values, deleted = fx.scenario(n_vm, MIDS) if n_vm > 1 else ([b"only"], [vm.render("m1", "m4-x", "o")], np.zeros(1, np.uint8))
        send(s, m, keys, values, deleted, False, "append off")  # every id is unknown: status 2, nothing joins
        assert s.vmodels_info()["n_rows"] == 0
        send(s, m, keys, values, deleted, True, "append on")
        check_table(s, m)
        check_questions(s, m)
        check_transitions(s, m)
        send(s, m, keys, values, deleted, False, "again, append off")  # known ids apply, the others are still status 2
        check_table(s, m, "again")
    finally:
        s.close()


@pytest.mark.parametrize("a,b", [(7, 1), (8, 0), (8, 1), (15, 1), (16, 1), (16, 17), (31, 2)])
def test_two_batches_equal_one_across_capacity_edges(a, b):
    """V rows and n joining ids on either side of 2 (V + n) <= capacity."""
    ids = fx.vmodel_ids(a + b, b"cap")
    vals = [fx.record_for(k, MIDS)[0] if k % 20 not in (11, 12) else vm.render("m1", "m2") for k in range(a + b)]
    extra = [ids[0], ids[a - 1]]  # B also touches two rows of A
    kb, vb = ids[a:] + extra, vals[a:] + [vm.render(None, "m1"), vm.render("m5", "m5", "own")]
    one, two, m1, m2 = start(), start(), vm.VModels(), vm.VModels()
    try:
        send(one, m1, ids[:a], vals[:a])
        assert one.vmodels_info()["capacity"] == tab_capacity(a)
        send(one, m1, kb, vb)
        send(two, m2, ids[:a] + kb, vals[:a] + vb)
        assert one.vmodels_info()["capacity"] == two.vmodels_info()["capacity"] == tab_capacity(a + b)
        assert (2 * (a + b) <= tab_capacity(a)) == (tab_capacity(a + b) == tab_capacity(a))
        check_table(one, m1)
        check_table(two, m2)
        assert one.vmodels_get()[0] == two.vmodels_get()[0] and one.vmodels_get()[2] == two.vmodels_get()[2]
        q = ids + [b"cap-never", b"", ids[0] + b"x", ids[1][:-1]]
        assert np.array_equal(one.vmodels_resolve(q), two.vmodels_resolve(q))
        assert answers(one.vmodels_resolve(q)) == [tuple(x) for x in m1.resolve_many(registry_of(one), q)]
        assert list(one.vmodels_resolve(q)["vmodel"][:4]) == [0, 1, 2, 3] and (one.vmodels_resolve(q)["vmodel"][a + b:] == -1).all()
    finally:
        one.close()
        two.close()


def _contended(keys, values, deleted):
    s, m = start(8), vm.VModels()
    try:
        send(s, m, [b"base-%d" % i for i in range(5)], [vm.render("m1", "m2")] * 5)
        got = send(s, m, keys, values, deleted)
        check_table(s, m)
        ids, flags, strings = s.vmodels_get()
        q = s.vmodels_resolve(ids)
        return [got[0].tobytes(), got[1].tobytes(), got[2], ids, flags.tobytes(), strings, q.tobytes(), s.vmodels_info().tobytes()]
    finally:
        s.close()


def test_one_key_4096_times_and_4096_new_keys_twice_each():
    rng, n = np.random.default_rng(5), 4096
    pool = [fx.record_for(k, MIDS)[0] for k in range(40) if k % 20 != 11]
    values = [pool[int(i)] for i in rng.integers(0, len(pool), n)]
    deleted = (rng.random(n) < 0.15).astype(np.uint8)
    deleted[:3] = 1  # the key is unknown until event 3
    deleted[3] = 0
    one = _contended([b"the-one-key"] * n, values, deleted)
    assert one == _contended([b"the-one-key"] * n, values, deleted)
    assert one[2] == 1
    keys = fx.vmodel_ids(n, b"many")
    keys, values = keys + keys[::-1], values + values[::-1]  # 4 096 new keys, twice each
    many = _contended(keys, values, np.zeros(2 * n, np.uint8))
    assert many == _contended(keys, values, np.zeros(2 * n, np.uint8))
    assert many[2] == n and many[3][5:] == keys[:n]


def test_delete_set_again_and_deletions_of_unknown_ids():
    s, m = start(), vm.VModels()
    try:
        st, idx, n = send(s, m, [b"u", b"a", b"u", b"u", b"a"], ["", vm.render("m1", "m1"), vm.render("m1", "m2"), "", ""], [1, 0, 0, 1, 1])
        assert list(st) == [2, 0, 0, 0, 0] and list(idx) == [-1, 0, 1, 1, 0] and n == 2  # status 2 before the join, applied behind it
        check_table(s, m)
        assert list(s.vmodels_get()[1]) == [30, 30] and s.vmodels_info()["n_live"] == 0  # both ABSENT, ids and numbers kept
        assert answers(s.vmodels_resolve([b"a", b"u"])) == [(0, 0, -1, -1, -1, 0, 0, 0)] * 2
        st, idx, n = send(s, m, [b"a", b"nobody", b"u"], [vm.render("m2", "m2", "me"), "", "{}"], [0, 1, 0], append=False)
        assert list(st) == [0, 2, 0] and list(idx) == [0, -1, 1] and n == 0  # the old rows back
        check_table(s, m)
        check_questions(s, m)
    finally:
        s.close()


def test_malformed_and_edge_values():
    for v in fx.MALFORMED:
        ok = True
        try:
            ok = isinstance(json.loads(v), dict)
        except ValueError:
            ok = False
        assert vm.classify(v)[0] == REJECT and (not ok or "amid" in v or "tmid" in v or '"o"' in v or "failed" in v), v
    for v in fx.EDGE:
        assert isinstance(json.loads(v), dict) and vm.classify(v)[0] == ACCEPT, v
    s, m = start(), vm.VModels()
    try:
        n = len(fx.MALFORMED)
        keys = fx.vmodel_ids(n, b"bad")
        send(s, m, keys, [fx.record_for(k, MIDS)[0] if k % 20 not in (11, 12) else "{}" for k in range(n)])
        before = (s.vmodels_get(), s.vmodels_info().tobytes())
        st, idx, n_app = send(s, m, keys + [b"bad-new"], fx.MALFORMED + ["{"])
        assert st.all() and n_app == 1 and list(idx) == list(range(n + 1))
        after = s.vmodels_get(0, n)
        assert after[0] == before[0][0] and np.array_equal(after[1], before[0][1]) and after[2] == before[0][2]  # rows, strings untouched
        assert s.vmodels_info()["arena_bytes"] == np.frombuffer(before[1], _lib.VMODELS_STATS)[0]["arena_bytes"]
        assert s.vmodels_get(n, 1)[1][0] == 30  # a joined row whose events are all malformed is ABSENT
        st, _, _ = send(s, m, fx.vmodel_ids(len(fx.EDGE), b"edge"), fx.EDGE)
        assert not st.any()
        check_table(s, m)
        # both lists again longer than the tile, behind and in front of 2 100 blanks: the serial walk gives the tile's verdicts and rows
        for k, pad in enumerate((lambda v: " " * 2100 + v, lambda v: v + " " * 2100)):
            st, _, _ = send(s, m, fx.vmodel_ids(len(fx.MALFORMED + fx.EDGE), b"long%d" % k), [pad(v) for v in fx.MALFORMED + fx.EDGE])
            assert list(st) == [1] * len(fx.MALFORMED) + [0] * len(fx.EDGE)
        assert m.strings()[-len(fx.EDGE):] == m.strings()[-2 * len(fx.EDGE) - len(fx.MALFORMED):-len(fx.EDGE) - len(fx.MALFORMED)]
        check_table(s, m)
        check_questions(s, m)
    finally:
        s.close()


def test_tile_edge_at_every_alignment():
    """Values of 2 046 .. 2 050 bytes (2 048 is the last the tile takes) starting at every byte alignment of the staged dwords,
    padded by a long `o` and by an unknown member: the tile and the serial walk agree with the model."""
    keys, vals, starts, off = [], [], set(), 0
    for total in range(2046, 2051):
        for by_owner in (True, False):
            for align in range(4):
                filler = '{"amid":"f"}' + " " * ((align - off - 12) % 4)
                off += len(filler)
                starts.add((off % 4, total))
                v = fx.padded(total, by_owner)
                off += len(v)
                keys += [b"fill-%d" % len(keys), b"edge-%d" % len(keys)]
                vals += [filler, v]
    assert starts == {(a, t) for a in range(4) for t in range(2046, 2051)}
    s, m = start(), vm.VModels()
    try:
        st, _, _ = send(s, m, keys, vals)
        assert not st.any()
        check_table(s, m)
        bad = [v[:-1] for v in vals]  # ... and the same lengths less the closing brace: rejected on both routes
        st, _, _ = send(s, m, keys, bad)
        assert st[1::2].all()  # (a filler that ends in a blank only loses the blank)
        check_table(s, m, "after the truncated values")
    finally:
        s.close()


def test_every_template_byte_across_the_chunk_edges():
    vals = [fx.template_across_chunks(k) for k in range(128)]
    s, m = start(), vm.VModels()
    try:
        st, _, _ = send(s, m, [b"t%d" % k for k in range(128)], vals)
        assert not st.any() and m.rows[0] == m.rows[127] == vm.Row(b"active-model", b"target", b"owner\\\\x", True, True)
        check_table(s, m)
    finally:
        s.close()


GROUP_POOL = [fx.record_for(k, MIDS)[0] for k in range(60) if k % 20 != 11] + fx.MALFORMED[:12] + fx.EDGE


def grouped_batch(n, seed):
    """n events over n // 3 keys drawn from the corpus, a tenth deleted, one value longer than the tile in every 1 000."""
    rng = np.random.default_rng(seed)
    keys = [b"g%d" % int(i) for i in rng.integers(0, max(n // 3, 1), n)]
    values = [GROUP_POOL[int(i)] for i in rng.integers(0, len(GROUP_POOL), n)]
    for i in range(0, n, 1000):
        values[i] = fx.padded(2100 + i % 7, bool(i % 2))
    return keys, values, (rng.random(n) < 0.1).astype(np.uint8)


@pytest.mark.parametrize("n", [16383, 16384 + 3, 32768 + 1, 65536 + 5])
def test_grouped_path(n):
    """1, 2, 4 and 8 records per wavefront as the host picks them for these batch sizes, the last wavefront ragged."""
    s, m = start(), vm.VModels()
    try:
        send(s, m, *grouped_batch(n, n))
        check_table(s, m)
    finally:
        s.close()


@pytest.mark.parametrize("grp", [3, 7])
def test_odd_group_sizes(grp):
    """MMP_JGROUP is read once per process: a fresh child sends 4 096 events with 3 and 7 records per wavefront.  A child that ends
    by a signal or runs into its time limit fails the test; it is not started again."""
    r = subprocess.run([sys.executable, "-m", "tests.vmodel_group_child"], cwd=ROOT, env=dict(os.environ, MMP_JGROUP=str(grp)),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "MMP_JGROUP=%d: 4096 vmodel events, 0 differences" % grp in r.stdout


def test_ids_and_strings_that_differ_in_one_byte():
    """Ids and strings of 0, 1, 63, 64, 65 and 200 bytes that differ only in the first, the last and the 64th byte."""
    names = []
    for L in (0, 1, 63, 64, 65, 200):
        base = bytearray(b"k" * L)
        names.append(bytes(base))
        for pos in (0, L - 1, 63):
            if 0 <= pos < L:
                v = bytearray(base)
                v[pos] = ord("z")
                names.append(bytes(v))
    names = list(dict.fromkeys(names))
    s, m = start(), vm.VModels()
    try:
        st, _, _ = s.models_events_json(names, [REG_VALUES[0]] * len(names))[:3]  # the same names as model ids, rows M ..
        assert not st.any()
        vals = [vm.render(a.decode(), names[(i + 1) % len(names)].decode(), names[(i + 2) % len(names)].decode()) for i, a in enumerate(names)]
        send(s, m, names, vals)
        check_table(s, m)
        reg = registry_of(s)
        keys = [k for k in names for _ in names]
        other = [o for _ in names for o in names]
        got = s.vmodels_resolve(keys, other, other, np.ones(len(keys), np.uint32))
        assert answers(got) == [tuple(a) for a in m.resolve_many(reg, keys, other, other, np.ones(len(keys), np.uint32))]
        assert {int(c) for c in got["cls"]} == {vm.NOT_FOUND, vm.OK}
        got = s.vmodels_resolve(keys, other, None, np.ones(len(keys), np.uint32))
        assert answers(got) == [tuple(a) for a in m.resolve_many(reg, keys, other, None, np.ones(len(keys), np.uint32))]
        assert (got["model"][got["cls"] == vm.OK] >= 0).all() and {int(w) for w in got["which"]} == {vm.ACTIVE, vm.TARGET}
    finally:
        s.close()


@pytest.mark.parametrize("vbits,mbits", [(0, None), (4, None), (None, 0), (None, 4), (0, 0), (4, 4)])
def test_when_hashes_collide(monkeypatch, vbits, mbits):
    """Probes are as long as the tables are full here, so the fleet holds 64 models and the scenario 65 vmodels."""
    if vbits is not None:
        monkeypatch.setenv("MMP_VMODEL_ID_HASH_BITS", str(vbits))
    if mbits is not None:
        monkeypatch.setenv("MMP_MODEL_ID_HASH_BITS", str(mbits))
    s, m = start(64), vm.VModels()
    try:
        send(s, m, *fx.scenario(65, MIDS[:64]))
        check_table(s, m)
        check_questions(s, m)
        check_transitions(s, m)
    finally:
        s.close()


def test_arena_garbage_is_squeezed():
    keys = fx.vmodel_ids(64, b"ar")
    s, m = start(), vm.VModels()
    try:
        worst = 0
        for b in range(300):
            vals = [vm.render("active-%d-%d" % (b, k), "target-%d" % ((b * 7 + k) % 50), "owner" * (1 + (b + k) % 9)) for k in range(64)]
            send(s, m, keys, vals)
            info = s.vmodels_info()
            batch = sum(len(x) for r in m.strings() for x in r)
            assert info["live_bytes"] == m.info()[2] and info["arena_bytes"] <= 2 * info["live_bytes"] + batch, (b, info)
            worst = max(worst, int(info["arena_bytes"]))
        assert worst > m.info()[2]  # garbage did build up in between
        check_table(s, m)
    finally:
        s.close()


# ---- resolve --------------------------------------------------------------------------------------------------------------------

def test_a_model_that_joins_between_two_resolves_and_retired_rows():
    s, m = start(), vm.VModels()
    try:
        send(s, m, [b"v", b"w"], [vm.render("not-yet-a-model", MIDS[9].decode()), vm.render(MIDS[200].decode(), MIDS[201].decode())])
        a = s.vmodels_resolve([b"v", b"w"])
        assert list(a["model"]) == [-1, 200] and list(a["target_model"]) == [9, 201] and list(a["cls"]) == [vm.OK, vm.OK]
        st, idx, _, n = s.models_events_json([b"not-yet-a-model"], [REG_VALUES[0]])
        assert not st.any() and list(idx) == [M] and n == 1
        a = s.vmodels_resolve([b"v", b"w"])  # no vmodel call in between
        assert list(a["model"]) == [M, 200] and list(a["target_model"]) == [9, 201]
        check_questions(s, m)
        remap = s.models_retire([3, 4, 150, 201])  # rows below the answered ones, and an answered row itself
        assert remap[9] == 7 and remap[200] == 197 and remap[201] == -1 and remap[M] == M - 4
        a = s.vmodels_resolve([b"v", b"w"])
        assert list(a["model"]) == [M - 4, 197] and list(a["target_model"]) == [7, -1]
        assert list(a["target_status"]) == [vm.T_LOADING, vm.T_NOT_FOUND]
        check_questions(s, m)
        check_transitions(s, m)
    finally:
        s.close()


def test_the_strong_read_loop():
    s, m = start(), vm.VModels()
    try:
        old, new, tgt = MIDS[8].decode(), MIDS[16].decode(), MIDS[24].decode()
        send(s, m, [b"v"], [vm.render(old, old)])
        a = s.vmodels_resolve([b"v"])[0]
        assert (a["cls"], a["model"]) == (vm.OK, 8)
        # the host found model 8 gone and asks again with notFoundModelId
        assert s.vmodels_resolve([b"v"], [old])[0]["cls"] == vm.STRONG_READ
        send(s, m, [b"v"], [vm.render(new, new)])  # vModels.getStrong gave a newer value
        a = s.vmodels_resolve([b"v"], [old], None, [_lib.VMRQ_AFTER_STRONG])[0]
        assert (a["cls"], a["which"], a["model"]) == (vm.OK, vm.ACTIVE, 16)
        send(s, m, [b"v"], [vm.render(old, tgt)])  # ... or the same active id with a target
        a = s.vmodels_resolve([b"v"], [old], None, [_lib.VMRQ_AFTER_STRONG])[0]
        assert (a["cls"], a["which"], a["model"]) == (vm.OK, vm.TARGET, 24)
        send(s, m, [b"v"], [vm.render(old, old)])  # ... or nothing new at all
        assert s.vmodels_resolve([b"v"], [old], None, [_lib.VMRQ_AFTER_STRONG])[0]["cls"] == vm.TARGET_NOT_FOUND
        check_questions(s, m)
    finally:
        s.close()


def test_estate_without_a_model_id_table():
    s = WORLD.solver()
    try:
        st, _, n = s.vmodels_events_json([b"v"], [vm.render("a", "b")])  # the event call needs neither id load
        assert not st.any() and n == 1
        out, rc = s.vmodels_resolve_raw([b"v"], fill=FILL)
        assert rc == _lib.MMP_ESTATE and (out.view(np.uint8) == FILL).all()
        rows, n, info, rc = s.vmodels_transitions_raw(1, 1, 4, fill=FILL)
        assert rc == _lib.MMP_ESTATE and n == -1 and (rows.view(np.uint8) == FILL).all() and (np.array([info]).view(np.uint8) == FILL).all()
        s.ingest_models_json(REG_VALUES[:8])
        s.model_ids_load(MIDS[:8])
        assert s.vmodels_resolve([b"v"])[0]["cls"] == vm.OK
        s.upsert_models_json([REG_VALUES[0]], [8])  # an append by index: the two model spaces out of step
        with pytest.raises(MmpError) as e:
            s.vmodels_resolve([b"v"])
        assert e.value.code == _lib.MMP_ESTATE
    finally:
        s.close()


# ---- transitions ----------------------------------------------------------------------------------------------------------------

def test_transitions_follow_the_registry():
    s, m = start(), vm.VModels()
    try:
        send(s, m, *fx.scenario(257, MIDS))
        before = answers(check_transitions(s, m))
        # 1. an applied mmp_registry_ops: a not-loaded active model gets a copy (PROMOTE -> ENSURE_LOADED)
        k = next(t[0] for t in before if t[4] == vm.PROMOTE and t[1] >= 0 and not t[5] & vm.XF_FROM_EMPTY)
        frm = next(t[1] for t in before if t[0] == k)
        ops = np.zeros(1, _lib.REGISTRY_OP)
        ops[0] = (frm, 2, _lib.ROP_REGISTER, 0, fx.NOW, fx.NOW, fx.NOW)
        status, _, _ = s.registry_ops(ops, fx.NOW)
        assert status[0] == _lib.ROP_EDITED
        after = answers(check_transitions(s, m, "ops"))
        assert next(t for t in after if t[0] == k)[3:5] == (1, vm.ENSURE_LOADED)
        # 2. an applied prune: instance 1 is gone, its copies leave the records
        loaded = int(s.get_models()[0]["n_loaded"].sum())
        s.remove_pods(np.array([1], np.int32))
        s.commit()
        s.prune_registry(0, fx.NOW, gone_after_ms=1000)
        s.prune_registry(0, fx.NOW + 2000, gone_after_ms=1000)
        assert int(s.get_models()[0]["n_loaded"].sum()) < loaded
        pruned = answers(check_transitions(s, m, "prune"))
        assert pruned != after
        # 3. a deletion of the active model's record: FROM_EMPTY, PROMOTE
        t = next(t for t in pruned if t[4] == vm.ENSURE_LOADED)
        st, _, _, _ = s.models_events_json([MIDS[t[1]]], [""], deleted=[1])
        assert not st.any()
        gone = answers(check_transitions(s, m, "deleted"))
        assert next(x for x in gone if x[0] == t[0])[3:6] == (0, vm.PROMOTE, (t[5] | vm.XF_FROM_EMPTY))
        check_questions(s, m)
    finally:
        s.close()


def test_transitions_sizing_protocol():
    s, m = start(), vm.VModels()
    try:
        send(s, m, *fx.scenario(257, MIDS))
        want, winfo = m.transitions(registry_of(s), fx.NOW, fx.AGE)
        n = len(want)
        assert n > 8
        for cap, null in ((0, True), (0, False), (n - 1, False), (n, False), (n + 5, False)):
            rows, got_n, info, rc = s.vmodels_transitions_raw(fx.NOW, fx.AGE, cap, fill=FILL, null_rows=null)
            assert rc == 0 and got_n == n and info["truncated"] == (1 if cap < n else 0) and info["n_listed"] == n
            take = min(cap, n)
            assert answers(rows[:take]) == [tuple(t) for t in want[:take]]
            assert (rows[take:].view(np.uint8) == FILL).all()  # nothing beyond the prefix is written
        for rc in (s.vmodels_transitions_raw(fx.NOW, fx.AGE, 4, null_rows=True)[3], s.vmodels_transitions_raw(fx.NOW, fx.AGE, -1)[3]):
            assert rc == _lib.MMP_EINVAL
    finally:
        s.close()


def test_transition_scan_against_the_numpy_form():
    """2 000 vmodels over 300 instances x 2 000 models."""
    n = 2000
    world = World(2, pods=300, models=n)
    mids = fx.model_ids(n)
    vals, _ = fx.registry_values(world.pod_ids, n)
    s, m = world.solver(), vm.VModels()
    try:
        assert not s.ingest_models_json(vals)[0].any()
        s.model_ids_load(mids)
        keys, values, deleted = fx.scenario(n, mids)
        send(s, m, keys, values, deleted)
        reg = registry_of(s)
        rows, info = s.vmodels_transitions(fx.NOW, fx.AGE)
        ids, flags, strings = s.vmodels_get()
        mrows = s.get_models()[0]
        row_of = {b: i for i, b in enumerate(s.model_ids_get())}
        arow = np.array([row_of.get(a, -1) if a is not None else -1 for a, _, _ in strings], np.int32)
        trow = np.array([row_of.get(t, -1) if t is not None else -1 for _, t, _ in strings], np.int32)
        listed = ((flags & (vm.F_ABSENT | vm.F_HOST)) == 0) & np.array([a != t for a, t, _ in strings])
        empty = (mrows["type"] == 0) & (mrows["n_loaded"] == 0) & (mrows["n_failed"] == 0) & (mrows["last_used"] == 0)
        want = vm.transitions_numpy(listed, arow, trow, (flags & vm.F_FAILED) != 0, mrows["n_loaded"], mrows["last_used"], empty, fx.NOW, fx.AGE)
        assert rows.tobytes() == want.tobytes() and info["n_listed"] == len(want) > 500
        assert answers(rows) == [tuple(t) for t in m.transitions(reg, fx.NOW, fx.AGE)[0]]
    finally:
        s.close()


# ---- every call -----------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_untouched():
    s, m = start(), vm.VModels()
    try:
        send(s, m, *fx.scenario(65, MIDS))
        before = (s.vmodels_get(), s.vmodels_info().tobytes())
        keys, vals = [b"ka", b"kb"], [vm.render("a", "b"), vm.render("c", "d")]

        def ev(**kw):
            st, idx, n_app, rc = s.vmodels_events_json_raw(keys, vals, fill=FILL, **kw)
            assert (st.view(np.uint8) == FILL).all() and (idx.view(np.uint8) == FILL).all(), kw
            return rc

        L = len(vals[0])
        for rc in (ev(flags=2), ev(key_off=[0, 3, 2]), ev(off=[0, L + 5, L]), ev(null_idx=True), ev(null_status=True)):
            assert rc == _lib.MMP_EINVAL
        lib = s.lib
        koff, off = np.array([0, 2, 4], np.int32), np.array([0, L, L + len(vals[1])], np.int64)
        out = np.full(4, -7, np.int32)
        for args in ((None, _lib.ptr(koff), b"x" * 100, _lib.ptr(off), 2), (b"kakb", None, b"x" * 100, _lib.ptr(off), 2),
                     (b"kakb", _lib.ptr(koff), None, _lib.ptr(off), 2), (b"kakb", _lib.ptr(koff), b"x" * 100, None, 2),
                     (b"kakb", _lib.ptr(koff), b"x" * 100, _lib.ptr(off), -1)):
            assert lib.mmp_vmodels_events_json(s.h, *args, None, 1, _lib.ptr(out), _lib.ptr(out), None) == _lib.MMP_EINVAL
            assert (out == -7).all()
        # resolve: a NULL output, offsets that decrease, unknown request flags
        q = [b"vm-0", b"vm-1-x"]
        for kw in (dict(null_out=True), dict(key_off=[0, 5, 4]), dict(req_flags=[0, 2])):
            a, rc = s.vmodels_resolve_raw(q, fill=FILL, **kw)
            assert rc == _lib.MMP_EINVAL and (a.view(np.uint8) == FILL).all(), kw
        # get: a range outside the table, a NULL size word
        nid, nstr = _lib.C.c_int32(-3), _lib.C.c_int32(-3)
        n_rows = int(s.vmodels_info()["n_rows"])
        byref = _lib.C.byref
        assert lib.mmp_vmodels_get(s.h, 0, n_rows + 1, None, 0, None, byref(nid), None, None, 0, None, byref(nstr)) == _lib.MMP_EINVAL
        assert lib.mmp_vmodels_get(s.h, -1, 1, None, 0, None, byref(nid), None, None, 0, None, byref(nstr)) == _lib.MMP_EINVAL
        assert lib.mmp_vmodels_get(s.h, 0, 1, None, 0, None, None, None, None, 0, None, byref(nstr)) == _lib.MMP_EINVAL
        assert lib.mmp_vmodels_get(s.h, 0, 1, None, 4, None, byref(nid), None, None, 0, None, byref(nstr)) == _lib.MMP_EINVAL
        assert nid.value == -3 and nstr.value == -3
        # ... sizes first: undersized byte buffers get the sizes and no byte
        ids = np.full(4, FILL, np.uint8)
        strs = np.full(4, FILL, np.uint8)
        assert lib.mmp_vmodels_get(s.h, 0, n_rows, _lib.ptr(ids), 4, None, byref(nid), None, _lib.ptr(strs), 4, None, byref(nstr)) == 0
        assert nid.value == sum(map(len, m.ids)) and nstr.value == m.info()[2] and (ids == FILL).all() and (strs == FILL).all()
        assert lib.mmp_vmodels_info(s.h, None) == _lib.MMP_EINVAL
        after = (s.vmodels_get(), s.vmodels_info().tobytes())
        assert before[0][0] == after[0][0] and np.array_equal(before[0][1], after[0][1]) and before[0][2] == after[0][2] and before[1] == after[1]
    finally:
        s.close()


def test_two_runs_are_byte_identical():
    def run():
        s, m = start(), vm.VModels()
        try:
            s.profile(True)
            keys, values, deleted = fx.scenario(257, MIDS)
            got = s.vmodels_events_json(keys, values, deleted)
            assert s.last_kernel_ms() > 0
            qk, nf, ow, fl = fx.questions(vm_of(keys, values, deleted))
            a = s.vmodels_resolve(qk, nf, ow, fl)
            assert s.last_kernel_ms() > 0
            rows, info = s.vmodels_transitions(fx.NOW, fx.AGE)
            ids, flags, strings = s.vmodels_get()
            return [got[0].tobytes(), got[1].tobytes(), got[2], a.tobytes(), rows.tobytes(), info.tobytes(), ids, flags.tobytes(), strings,
                    s.vmodels_info().tobytes()]
        finally:
            s.close()

    assert run() == run()


def vm_of(keys, values, deleted):
    m = vm.VModels()
    m.events(keys, values, deleted)
    return m


def test_resolves_beside_event_batches():
    """200 resolves on a second thread beside event batches that alternate 40 rows between two states: every answer set equals the
    state before or the state after, never a mix."""
    s, m = start(), vm.VModels()
    try:
        keys = fx.vmodel_ids(40, b"alt")
        states = [[vm.render(MIDS[(k + 8 * j) % M].decode(), MIDS[(k + 16 * j + 1) % M].decode(), "o%d" % j, failed=bool(j)) for k in range(40)]
                  for j in range(2)]
        want = []
        for v in states:
            send(s, m, keys, v)
            want.append(s.vmodels_resolve(keys).tobytes())
        assert want[0] != want[1]
        seen, errors, done = [], [], threading.Event()

        def reader():
            try:
                for _ in range(200):
                    seen.append(s.vmodels_resolve(keys).tobytes())
            except Exception as e:  # noqa: BLE001
                errors.append(e)
            finally:
                done.set()

        th = threading.Thread(target=reader)
        th.start()
        turn = 0
        try:
            while not done.is_set() and turn < 2000:  # bounded: the reader ends it
                st, _, n = s.vmodels_events_json(keys, states[turn % 2])
                assert not st.any() and n == 0
                turn += 1
        finally:
            th.join()
        assert not errors, errors
        assert len(seen) == 200 and all(x in want for x in seen), sum(x not in want for x in seen)
        print(f"200 resolves beside {turn} batches: {sum(x == want[0] for x in seen)} saw state 0, {sum(x == want[1] for x in seen)} state 1")
    finally:
        s.close()
