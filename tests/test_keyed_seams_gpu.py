"""GPU: the request seams by model id (mmp_place_batch_ck / mmp_route_batch_ck / mmp_miss_batch_ck; keyed_resolve_kernel,
modelmesh_amd/csrc/keyed_kernels.hpp).

Their answers are DEFINED (include/mmplace.h, THE RULE BY KEY) as those of the existing _c calls on the same rows with model = the
row the key names, so every comparison here is of bytes, and WHICH row a key names comes from a Python dict kept in step with the
events the test sends (tests/keyed_seam_model.py), not from the library's lookup: (1) the rule across both slot thresholds, (2) with
colliding hashes, (3) while the id table grows, moves and is compacted, (4) the refusals, (5) beside writers of the id table and
holders of the batch lock, (6) twice."""
import threading

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd import wire
from modelmesh_amd import workload as wl
from modelmesh_amd._lib import MMP_EINVAL, MMP_ESTATE, MMP_OK, ptr
from modelmesh_amd.solver import Solver
from tests import keyed_seam_model as ksm
from tests import test_seam_caller_gpu as sc  # the fleets with long copy lists, one caller's batch, the byte comparison

pytestmark = pytest.mark.gpu

# 0 .. 256 ride a latency slot, 257 .. are staged (KeyedRouteSlot / KeyedMissSlot / KeyedPlaceSlot, mmplace.hip); 63 / 64 / 65: the
# last wavefront's fill; 2: more than the lone request
NS = (0, 1, 2, 63, 64, 65, 256, 257, 1000)
N_MAX = max(NS)
SLOT_N, SLOT_KEY_BYTES = 256, 16384
EXPIRY = sc.EXPIRY
GARBAGE_G, GARBAGE_P = 0x5A5A5A5A, 0x3C3C3C3C  # what the `model` fields hold on input: ignored, and two values in one request
N_MODELS = 300


def id_table_slots(n_ids):
    """model_ids_kernels.hpp: 16 slots for up to 8 ids, doubling whenever the ids outgrow half of it"""
    cap = 16
    while n_ids > cap // 2:
        cap *= 2
    return cap


class Mesh:
    """A typed 200-instance fuzz fleet with long copy lists, its registry rows named by ids of every awkward shape, one caller's
    batch of N_MAX requests built while the registry's host mirror stands, and the dict that knows which row a key names."""

    def __init__(self, seed=1, pods=200, load_ids=True, commit=True):
        fleet, self.long_models = sc.with_long_copy_lists(wl.fuzz_fleet(seed, pods=pods, models=N_MODELS, profile="typed"), seed)
        rng = self.rng = np.random.default_rng(7000 + seed)
        pod_ids = wire.make_ids(rng, pods)
        wire.adopt_ids(fleet, pod_ids)
        self.fleet = fleet
        self.s = s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
        s.load_pod_ids(pod_ids)
        s.load_fleet(fleet, commit=commit)
        self.ids = ksm.make_ids(rng, fleet.n_models)
        self.never = ksm.make_ids(rng, 64, tag=b"never")
        assert not set(self.ids) & set(self.never)
        self.km = ksm.KeyRows(self.ids)
        if load_ids:
            s.model_ids_load(self.ids)
        self.a = sc.make_batch(fleet, s, 900 + seed, N_MAX, 3, self.long_models)
        # the key of request i names the model the batch was built for (its counters are that model's copies) or misses
        self.keys = ksm.request_keys(rng, self.a["greqs"]["model"], self.ids, self.never, self.km.rows)

    def close(self):
        self.s.close()


@pytest.fixture(scope="module")
def mesh():
    m = Mesh()
    yield m
    m.close()


def staged(s, call):
    """(the call's result, whether it was staged: a staged call leaves its kernel time, a slot call does not)"""
    s.profile(True)
    out = call()
    was = s.last_kernel_ms() >= 0
    s.profile(False)
    return out, was


def with_model(rows_c, model):
    out = rows_c.copy()
    out["model"] = model
    return out


def keyed_calls(s, a, keys, want_idx=True):
    """The three keyed calls on one batch, the `model` fields filled with garbage -> {call: outputs + (model_idx,)}; the caller's
    arrays must come back as they went in."""
    g, p, sr = with_model(a["greqs"], GARBAGE_G), with_model(a["preqs"], GARBAGE_P), a["sreqs"]
    ins = {"g": g, "p": p, "s": sr, "counters": a["counters"], "xp": a["xp"], "xt": a["xt"], "expl": a["expl"], "extra": a["extra"],
           "caller": a["caller"], "pcaller": a["pcaller"]}
    before = {k: v.tobytes() for k, v in ins.items()}
    out = {
        "route": s.route_batch_ck(a["caller"], g, sr, keys, a["counters"], a["xp"], a["xt"], a["expl"], a["now"], EXPIRY, want_idx),
        "miss": s.miss_batch_ck(a["caller"], a["pcaller"], g, p, keys, a["xp"], a["xt"], a["expl"], a["extra"], a["now"], EXPIRY, want_idx),
        "place": s.place_batch_ck(a["pcaller"], p, keys, a["extra"], a["now"], want_idx),
    }
    assert {k: v.tobytes() for k, v in ins.items()} == before  # the caller's arrays are never written
    return out


def reference_calls(s, a, rows):
    """The existing _c calls on the same rows with model = rows"""
    g, p = with_model(a["greqs"], rows), with_model(a["preqs"], rows)
    return {
        "route": s.route_c(a["caller"], g, a["sreqs"], a["counters"], a["xp"], a["xt"], a["expl"], a["now"], EXPIRY),
        "miss": s.miss_c(a["caller"], a["pcaller"], g, p, a["xp"], a["xt"], a["expl"], a["extra"], a["now"], EXPIRY),
        "place": (s.place_c(a["pcaller"], p, a["extra"], a["now"]),),
    }


def assert_rule(s, a, keys, rows, what):
    """model_idx equals the dict's rows, every output array equals the _c call's on those rows — with and without model_idx_out"""
    n = len(keys)
    want = reference_calls(s, a, rows)
    for want_idx in (True, False):
        got = keyed_calls(s, a, keys, want_idx)
        for call in ("route", "miss", "place"):
            outs, idx = got[call][:-1], got[call][-1]
            if want_idx:
                assert idx.dtype == np.int32 and len(idx) == n and np.array_equal(idx, rows), (what, call, np.nonzero(idx != rows)[0][:8])
            else:
                assert idx is None
            assert all(len(o) == n for o in outs)
            sc.assert_bytes(outs, want[call], (what, call, n, want_idx))


# ---- 1. the rule ---------------------------------------------------------------------------------------------------------------
def test_the_batch_holds_what_part_1_is_about(mesh):
    a, rows = mesh.a, mesh.km.rows(mesh.keys)
    sc.check_contents(mesh.fleet, with_greq_rows(a, rows), mesh.long_models)
    assert len(a["counters"]) <= 4096 and len(a["xp"]) <= 2048 and len(a["expl"]) <= 2048 and len(a["extra"]) <= 2048  # the slots' pools
    ids = mesh.ids
    assert any(len(k.decode()) < len(k) for k in ids[:10])  # multi-byte UTF-8
    assert min(map(len, ids)) == 1 and max(map(len, ids)) == 200
    assert any(x != y and y.startswith(x) for x in ids[:10] for y in ids[:10])
    assert any(x != y and len(x) == len(y) and x[:-1] == y[:-1] for x in ids[:10] for y in ids[:10])
    assert any(x != y and len(x) == len(y) and x[1:] == y[1:] for x in ids[:10] for y in ids[:10])
    for n in NS:
        ksm.check_mix(rows[:n])
    assert sum(map(len, mesh.keys[:SLOT_N])) <= SLOT_KEY_BYTES  # at 256 requests the row count alone decides the path


def with_greq_rows(a, rows):
    b = dict(a)
    b["greqs"] = with_model(a["greqs"], rows)
    return b


@pytest.mark.parametrize("n", NS)
def test_keyed_calls_equal_the_c_calls_on_the_rows_the_keys_name(mesh, n):
    a, keys = sc.head(mesh.a, n), mesh.keys[:n]
    rows = mesh.km.rows(keys)
    assert_rule(mesh.s, a, keys, rows, "rule")
    if n:
        g, p = with_model(a["greqs"], GARBAGE_G), with_model(a["preqs"], GARBAGE_P)
        s = mesh.s
        paths = [staged(s, lambda: s.route_batch_ck(a["caller"], g, a["sreqs"], keys, a["counters"], a["xp"], a["xt"], a["expl"], a["now"]))[1],
                 staged(s, lambda: s.miss_batch_ck(a["caller"], a["pcaller"], g, p, keys, a["xp"], a["xt"], a["expl"], a["extra"], a["now"]))[1],
                 staged(s, lambda: s.place_batch_ck(a["pcaller"], p, keys, a["extra"], a["now"]))[1]]
        assert paths == [n > SLOT_N] * 3


def long_keys(mesh, total_bytes, n=200):
    """n keys of exactly total_bytes bytes: a fifth known ids, the rest never loaded, the last one cut to fit"""
    known = [k for k in mesh.ids if len(k) >= 30][: n // 5]
    assert len(known) == n // 5
    q, r = divmod(total_bytes - sum(map(len, known)), n - len(known))
    assert 16 <= q < 200
    unknown = [(b"never-long-%03d-" % i).ljust(q + (1 if i < r else 0), b"y") for i in range(n - len(known))]
    keys = [known[i // 5] if i % 5 == 0 else unknown[i - i // 5 - 1] for i in range(n)]
    assert len(keys) == n and sum(map(len, keys)) == total_bytes and len(set(keys)) == n
    return keys


@pytest.mark.parametrize("total_bytes,is_staged", [(SLOT_KEY_BYTES, False), (SLOT_KEY_BYTES + 1, True), (30_000, True)])
def test_the_key_bytes_decide_the_path_at_200_requests(mesh, total_bytes, is_staged):
    n, s = 200, mesh.s
    a, keys = sc.head(mesh.a, n), long_keys(mesh, total_bytes)
    rows = mesh.km.rows(keys)
    ksm.check_mix(rows)
    assert_rule(s, a, keys, rows, ("key bytes", total_bytes))
    g = with_model(a["greqs"], GARBAGE_G)
    _, was = staged(s, lambda: s.route_batch_ck(a["caller"], g, a["sreqs"], keys, a["counters"], a["xp"], a["xt"], a["expl"], a["now"]))
    assert was == is_staged


# ---- 2. colliding hashes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [0, 4])
def test_the_rule_when_ids_collide(monkeypatch, bits):
    """MMP_MODEL_ID_HASH_BITS is read per context: every id of this context shares one hash (0 bits) or one of sixteen (4), so a
    lookup is decided by the bytes."""
    monkeypatch.setenv("MMP_MODEL_ID_HASH_BITS", str(bits))
    m = Mesh(seed=2)
    try:
        for n in (1, 65, 257):
            keys = m.keys[:n]
            assert_rule(m.s, sc.head(m.a, n), keys, m.km.rows(keys), ("collide", bits))
    finally:
        m.close()


# ---- 3. a moving table ----------------------------------------------------------------------------------------------------------
def mixed_keys(m, rng, n, fresh):
    """n keys: ids of the table as it stands (the newest `fresh` among them), and misses"""
    ids = m.km.ids()
    pick = [ids[int(i)] for i in rng.integers(0, len(ids), n)]
    for j, k in enumerate(fresh[: n // 3]):
        pick[3 * j] = k
    for j in range(1, n, 4):
        pick[j] = m.never[j % len(m.never)] if j % 8 == 1 else pick[j] + b"+"
    return pick


def test_joins_resolve_in_the_next_call_and_a_retire_renumbers(mesh_moving):
    m = mesh_moving
    s, km, rng = m.s, m.km, np.random.default_rng(31)
    start_ids, start_bytes = km.n, sum(map(len, m.ids))
    joiners = ksm.make_ids(rng, 800, tag=b"joined", long_share=0.3)
    assert not set(joiners) & (set(m.ids) | set(m.never))
    for step in range(4):
        part = joiners[200 * step: 200 * step + 200]
        n_before = km.n
        st, idx, _, n_app = s.models_events_json(part, ["{}"] * len(part))
        km.join(part)
        assert n_app == 200 and not st.any() and np.array_equal(idx, km.rows(part)) and idx.min() == n_before
        for n in (1, 65, 257):
            keys = mixed_keys(m, rng, n, part)
            rows = km.rows(keys)
            if n > 1:
                assert (rows >= n_before).sum() >= n // 5 and (rows < 0).sum() >= n // 8  # rows at and above the old count; misses
            assert_rule(s, sc.head(m.a, n), keys, rows, ("joined", step))
    # the growth, through what the test can see: the ids outgrew the starting table twice over, and the arena its starting bytes
    assert id_table_slots(km.n) >= 4 * id_table_slots(start_ids)
    assert sum(map(len, joiners)) > 2 * (start_bytes + 16)
    # deletions, then the rows retired: old ids and joined ones
    gone = [m.ids[i] for i in (0, 5, 17, 150, 299)] + joiners[3:700:50]
    st, idx, _, _ = s.models_events_json(gone, [""] * len(gone), np.ones(len(gone), np.uint8))
    assert not st.any() and np.array_equal(idx, km.rows(gone))
    remap = s.models_retire(idx, empty_only=True)
    km.retire(remap)
    assert np.all(km.rows(gone) == -1) and km.n == start_ids + 800 - len(gone)
    for n in (1, 65, 257):
        keys = mixed_keys(m, rng, n, joiners[700:]) + gone[: min(n, 4)]
        keys = keys[-n:]
        rows = km.rows(keys)
        assert rows[-1] == -1  # a retired id
        assert_rule(s, sc.head(m.a, n), keys, rows, "retired")
    assert s.model_ids_get() == km.ids()


@pytest.fixture()
def mesh_moving():
    m = Mesh(seed=3)
    yield m
    m.close()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------
SENTINEL = 0xA5


def raw_args(m, n):
    a = sc.head(m.a, n)
    a = dict(a, g=with_model(a["greqs"], GARBAGE_G), p=with_model(a["preqs"], GARBAGE_P))
    blob, off = Solver.pack_keys(m.keys[:n])
    a["blob"], a["off"] = np.frombuffer(blob, np.uint8).copy(), off
    for k, dt in (("gouts", _lib.GATE_OUT), ("souts", _lib.SERVE_OUT), ("pouts", _lib.PLACE_OUT), ("idx", np.dtype(np.int32))):
        a[k] = np.frombuffer(bytes([SENTINEL]) * (dt.itemsize * n), dtype=dt).copy()
    return a


CALLS = ("route", "miss", "place")


def raw_calls(s, a, n, which=CALLS):
    """the calls named in `which` on raw pointers (None: NULL) -> their return codes"""
    p = lambda k: ptr(a[k]) if a[k] is not None and len(a[k]) else None  # noqa: E731
    L, now = s.lib, int(a["now"])
    run = {
        "route": lambda: L.mmp_route_batch_ck(s.h, p("caller"), p("g"), p("sreqs"), n, p("blob"), p("off"), p("counters"),
                                              len(a["counters"]), p("xp"), p("xt"), len(a["xp"]), p("expl"), len(a["expl"]), now, EXPIRY,
                                              p("gouts"), p("souts"), p("idx")),
        "miss": lambda: L.mmp_miss_batch_ck(s.h, p("caller"), p("pcaller"), p("g"), p("p"), n, p("blob"), p("off"), p("xp"), p("xt"),
                                            len(a["xp"]), p("expl"), len(a["expl"]), p("extra"), len(a["extra"]), now, EXPIRY,
                                            p("gouts"), p("pouts"), p("idx")),
        "place": lambda: L.mmp_place_batch_ck(s.h, p("pcaller"), p("p"), n, p("blob"), p("off"), p("extra"), len(a["extra"]), now,
                                              p("pouts"), p("idx")),
    }
    return tuple(run[c]() for c in which)


def outputs(a):
    return {k: a[k].tobytes() for k in ("gouts", "souts", "pouts", "idx")}


@pytest.mark.parametrize("n", [2, 300])
def test_einval_leaves_every_output_as_it_was(mesh, n):
    s, a = mesh.s, raw_args(mesh, n)
    before = outputs(a)
    INT_MAX = 2**31 - 1
    falling = a["off"].copy()
    falling[n - 1] = falling[n] + 1
    cases = [("null key_off", dict(a, off=None), n, CALLS), ("offsets that fall", dict(a, off=falling), n, CALLS),
             ("null keys with bytes present", dict(a, blob=None), n, CALLS), ("n < 0", a, -1, CALLS)]
    # a range outside a pool, in the last row, for the calls that read that array
    for arr, off_f, cnt_f, pool, which in (("g", "excl_off", "n_excl", "xp", ("route", "miss")), ("g", "explicit_off", "n_explicit", "expl", ("route", "miss")),
                                           ("p", "extra_off", "n_extra", "extra", ("miss", "place")), ("sreqs", "cnt_off", "n_cnt", "counters", ("route",))):
        for off, cnt in [(-1, 1), (0, -1), (INT_MAX, 1), (len(a[pool]), 1)]:
            b = dict(a)
            b[arr] = a[arr].copy()
            b[arr][off_f][n - 1], b[arr][cnt_f][n - 1] = off, cnt
            cases.append((f"{arr}.{off_f} = {off}, {cnt_f} = {cnt}", b, n, which))
    for what, b, nn, which in cases:
        assert raw_calls(s, b, nn, which) == (MMP_EINVAL,) * len(which), what
        assert outputs(a) == before, what
    assert raw_calls(s, a, n) == (MMP_OK, MMP_OK, MMP_OK)  # (what was refused above was the one argument alone)
    after = outputs(a)
    assert all(after[k] != before[k] for k in before)
    assert np.array_equal(a["idx"], mesh.km.rows(mesh.keys[:n]))


@pytest.mark.parametrize("n", [2, 300])
def test_estate_without_ids_without_a_commit_and_after_an_append_by_index(n):
    m = Mesh(seed=4, load_ids=False)
    try:
        s, a = m.s, raw_args(m, n)
        before = outputs(a)
        assert raw_calls(s, a, n) == (MMP_ESTATE,) * 3  # before mmp_model_ids_load
        assert "mmp_model_ids_load" in (s.lib.mmp_last_error(s.h) or b"").decode()
        assert raw_calls(s, a, 0) == (MMP_ESTATE,) * 3  # (n = 0 is a valid call: it is answered from the state alone)
        s.model_ids_load(m.ids)
        assert raw_calls(s, a, n) == (MMP_OK,) * 3 and raw_calls(s, a, 0) == (MMP_OK,) * 3
        a = raw_args(m, n)
        row = np.zeros(1, _lib.MODEL_ROW)
        s.upsert_models(np.array([N_MODELS], np.int32), row, np.zeros(0, np.int32), np.zeros(0, np.int64))  # an append by index
        assert raw_calls(s, a, n) == (MMP_ESTATE,) * 3
        assert outputs(a) == before
        s.model_ids_load(m.ids + [b"the three hundred and first"])
        assert raw_calls(s, a, n) == (MMP_OK,) * 3
        assert np.array_equal(a["idx"], m.km.rows(m.keys[:n]))
    finally:
        m.close()
    m = Mesh(seed=4, commit=False)
    try:
        a = raw_args(m, n)
        before = outputs(a)
        assert raw_calls(m.s, a, n) == (MMP_ESTATE,) * 3  # ids loaded, nothing committed
        assert outputs(a) == before
        falling = a["off"].copy()
        falling[n - 1] = falling[n] + 1
        assert raw_calls(m.s, dict(a, off=falling), n) == (MMP_EINVAL,) * 3  # the arguments are looked at first
    finally:
        m.close()


# ---- 5. beside writers ----------------------------------------------------------------------------------------------------------
def test_keyed_calls_beside_joins_and_holders_of_the_batch_lock():
    m = Mesh(seed=5)
    s, a, rng = m.s, m.a, np.random.default_rng(55)
    try:
        joiners = ksm.make_ids(rng, 800, tag=b"later")
        final_row = {k: N_MODELS + i for i, k in enumerate(joiners)}
        assert id_table_slots(N_MODELS + 800) >= 4 * id_table_slots(N_MODELS)
        # 64 small calls: windows of 1 to 8 requests of the batch, each with (at most) one key that joins during the run
        variants = []
        for v in range(64):
            n, lo = 1 + v % 8, int(rng.integers(0, N_MAX - 8))
            b = {k: (np.ascontiguousarray(a[k][lo:lo + n]) if k in ("greqs", "sreqs", "preqs") else a[k]) for k in a}
            keys = list(m.keys[lo:lo + n])
            joins = v % 3 == 0
            if joins:
                keys[v % n] = joiners[(37 * v) % 800]
            stable = np.array([k not in final_row for k in keys])
            rows = m.km.rows(keys)
            want = reference_calls(s, b, rows)  # on the starting state: no event touches the stable ids or their rows
            variants.append((b, keys, stable, rows, want))
        assert sum(int(v[2].sum()) for v in variants) >= 200 and sum(int((~v[2]).sum()) for v in variants) >= 20
        big_n = 20_000  # a host-pointer batch past every slot: staged, the batch lock held for the whole call
        big = wl.make_requests(m.fleet, 9, n=big_n, extra_frac=0.0)[0]
        big_c = np.zeros(big_n, dtype=_lib.PLACE_REQ_C)
        for f in _lib.PLACE_REQ_C.names:
            big_c[f] = big[f]
        big_want = s.place_c(a["pcaller"], big_c, None, a["now"])
        errors, cond, state = [], threading.Condition(), {"calls": 0, "done": False, "joined": 0, "big": 0}

        def keyed_thread():
            try:
                for rep in range(2000):
                    b, keys, stable, rows, want = variants[rep % len(variants)]
                    call = ("route", "miss", "place")[rep % 3]
                    got = keyed_calls_one(s, b, keys, call)
                    outs, idx = got[:-1], got[-1]
                    assert np.array_equal(idx[stable], rows[stable]), (rep, call)
                    for k in np.nonzero(~stable)[0]:
                        assert idx[k] in (-1, final_row[keys[k]]), (rep, call, int(idx[k]))
                    for o, w in zip(outs, want[call]):
                        assert o[stable].tobytes() == w[stable].tobytes(), (rep, call)
                    with cond:
                        state["calls"] += 1
                        cond.notify_all()
            except BaseException as e:  # noqa: BLE001
                errors.append(e)
            finally:
                with cond:
                    state["done"] = True
                    cond.notify_all()

        def paced(every, total, body):
            """`total` runs of body, run k once the keyed thread has answered k * every calls (or has ended)"""
            def run():
                try:
                    for k in range(total):
                        with cond:
                            cond.wait_for(lambda: state["calls"] >= k * every or state["done"])
                        body(k)
                except BaseException as e:  # noqa: BLE001
                    errors.append(e)
            return threading.Thread(target=run)

        def join_batch(k):
            part = joiners[100 * k: 100 * k + 100]
            st, idx, _, n_app = s.models_events_json(part, ["{}"] * 100)
            assert n_app == 100 and not st.any() and list(idx) == [final_row[x] for x in part]
            state["joined"] += 100

        def big_batch(k):
            sc.assert_bytes((s.place_c(a["pcaller"], big_c, None, a["now"]),), (big_want,), ("big", k))
            state["big"] += 1

        threads = [threading.Thread(target=keyed_thread), paced(200, 8, join_batch), paced(50, 30, big_batch)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors[:2]
        assert state["calls"] == 2000 and state["joined"] == 800 and state["big"] == 30
        # afterwards every key answers its final row
        for b, keys, stable, rows, want in variants[:8]:
            idx = keyed_calls_one(s, b, keys, "route")[-1]
            assert list(idx) == [final_row.get(k, int(r)) for k, r in zip(keys, rows)]
    finally:
        m.close()


def keyed_calls_one(s, a, keys, call):
    g, p = with_model(a["greqs"], GARBAGE_G), with_model(a["preqs"], GARBAGE_P)
    if call == "route":
        return s.route_batch_ck(a["caller"], g, a["sreqs"], keys, a["counters"], a["xp"], a["xt"], a["expl"], a["now"], EXPIRY)
    if call == "miss":
        return s.miss_batch_ck(a["caller"], a["pcaller"], g, p, keys, a["xp"], a["xt"], a["expl"], a["extra"], a["now"], EXPIRY)
    return s.place_batch_ck(a["pcaller"], p, keys, a["extra"], a["now"])


# ---- 6. twice -------------------------------------------------------------------------------------------------------------------
def test_two_runs_over_the_same_state_are_byte_identical(mesh):
    runs = [keyed_calls(mesh.s, mesh.a, mesh.keys) for _ in range(2)]
    for call in ("route", "miss", "place"):
        sc.assert_bytes(runs[0][call], runs[1][call], (call, "twice"))
