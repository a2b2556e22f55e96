"""GPU: the request seams by vmodel id (mmp_place_batch_cv / mmp_route_batch_cv / mmp_miss_batch_cv; vkeyed_resolve_kernel,
modelmesh_amd/csrc/vkeyed_kernels.hpp).

Their answers are DEFINED (include/mmplace.h, THE RULE BY VMODEL KEY) as those of the existing _c calls on the same rows with model =
the registry row resolveVModelId's answer names, and vm_out as mmp_vmodels_resolve's answer on the shared fields.  So every
comparison here is of bytes against the _c calls, and WHICH row a (vmodel key, nf, flags) names comes from Python dicts kept in
step with the events the test sends (tests/vkeyed_seam_model.py), never from the library's lookup: (1) the rule across the slot
threshold, (2) the byte limits of a slot, (3) colliding hashes in both id tables, (4) while both tables move, (5) equality with the
two-call sequence, (6) the refusals, (7) beside writers of the vmodel table and holders of the batch lock, (8) twice."""
import threading

import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd._lib import MMP_EINVAL, MMP_ESTATE, MMP_OK, ptr
from modelmesh_amd.solver import Solver
from tests import keyed_seam_model as ksm
from tests import test_keyed_seams_gpu as tk  # the 200-instance / 300-model Mesh, the _c reference calls, the staged() probe
from tests import test_seam_caller_gpu as sc
from tests import vkeyed_seam_model as vksm
from tests import vmodel_model as vm
from modelmesh_amd import workload as wl

pytestmark = pytest.mark.gpu

NS = (0, 1, 2, 63, 64, 65, 256, 257, 1000)  # 0 .. 256 ride a latency slot, 257 .. are staged; 63 / 64 / 65: the wavefront's fill
N_MAX = tk.N_MAX
SLOT_N, SLOT_KEY_BYTES, SLOT_NF_BYTES = 256, 8192, 8192  # VKeyed*Slot, mmplace.hip
LDS_BYTES = 8192  # vkeyed_kernels.hpp: what a workgroup stages of each kind
EXPIRY = tk.EXPIRY
N_VM = 120
KINDS = ("defined", "transition", "transition failed", "active null", "target null", "owner", "amid unknown", "absent", "host")
with_model = tk.with_model


def value(amid=None, tmid=None, owner=None, failed=False):
    """a stored VModelRecord with the ids as their raw bytes between the quotes"""
    parts = []
    if owner is not None:
        parts.append(b'"o":"' + owner + b'"')
    if amid is not None:
        parts.append(b'"amid":"' + amid + b'"')
    if tmid is not None:
        parts.append(b'"tmid":"' + tmid + b'"')
    if failed:
        parts.append(b'"failed":true')
    return b"{" + b",".join(parts) + b"}"


class VMesh:
    """tk.Mesh plus N_VM vmodels of every kind in KINDS, one request key / nf / flag word per request of the batch, and the dicts
    that know what each names."""

    def __init__(self, seed=1, send=True, **kw):
        self.m = m = tk.Mesh(seed=seed, **kw)
        self.s, self.a, self.km, self.ids = m.s, m.a, m.km, m.ids
        self.rng = rng = np.random.default_rng(8100 + seed)
        self.vk = vksm.VKeyRows(m.km)
        # (few long ids: 256 keys have to fit a slot's 8192 key bytes; the engineered first ten hold a 200-byte one)
        self.vids = ksm.make_ids(rng, N_VM, tag=b"v", long_share=0.0)
        self.vnever = ksm.make_ids(rng, 32, tag=b"Xnever", long_share=0.0)
        assert not set(self.vids) & set(self.vnever)
        self.short_ids = [k for k in self.ids if len(k) < 60]  # (256 nf spans have to fit a slot's 8192 nf bytes)
        # the models the batch asks for, in order of appearance: vmodel j's active model is one of them
        self.uniq = uniq = list(dict.fromkeys(int(r) for r in self.a["greqs"]["model"] if 0 <= r < tk.N_MODELS))
        assert len(uniq) >= N_VM
        self.values = [self.value_of(j, j % len(KINDS)) for j in range(N_VM)]
        self.absent = [self.vids[j] for j in range(N_VM) if KINDS[j % len(KINDS)] == "absent"]
        # the requests are drawn against the table as it stands after these two batches, whether or not they are sent now
        plan = vksm.VKeyRows(m.km)
        plan.events(self.vids, self.values)
        plan.events(self.absent, [b""] * len(self.absent), np.ones(len(self.absent), np.uint8))
        if send:
            self.send(self.vids, self.values)
            self.send(self.absent, [b""] * len(self.absent), np.ones(len(self.absent), np.uint8))
        self.keys, self.nf, self.flags = self.requests(self.a["greqs"]["model"], vt=plan.vt)

    def amid_of(self, j):
        return self.ids[self.uniq[j % len(self.uniq)]]

    def value_of(self, j, kind):
        A, B = self.amid_of(j), self.amid_of(j + 1)
        k = KINDS[kind]
        if k in ("defined", "absent"):
            return value(A, A)
        if k == "transition":
            return value(A, B)
        if k == "transition failed":
            return value(A, B, failed=True)
        if k == "active null":
            return value(None, B)
        if k == "target null":
            return value(A, None)
        if k == "owner":
            return value(A, A, owner=b"owner-%d" % j)
        if k == "amid unknown":
            return value(self.m.never[j % len(self.m.never)], B)
        return value(b"back\\\\slash-%d" % j, B)  # host: a backslash between the quotes

    def send(self, keys, values, deleted=None):
        """one event batch to the device and to the dict; the two must agree on status, rows and joins"""
        st, idx, n_app = self.s.vmodels_events_json(keys, values, deleted)
        st2, idx2, n_app2 = self.vk.events(keys, values, deleted)
        assert np.array_equal(st, st2) and np.array_equal(idx, idx2) and n_app == n_app2
        return n_app

    def requests(self, want_models, fresh=(), vt=None):
        """One (key, nf, flags) per request.  Keys: a vmodel whose active model is the one the request was built for, any vmodel
        (the newest `fresh` among them), a never-seen id, the empty key, a known id plus a byte.  nf: empty, the stored active id,
        the stored target id (both at once for a defined vmodel), another model's id.  Flags: AFTER_STRONG or not."""
        rng, vt = self.rng, vt or self.vk.vt
        by_amid = {}
        for v, r in enumerate(vt.rows):
            if r is not None and not r.host and r.amid is not None:
                by_amid.setdefault(self.km.row.get(r.amid, -1), []).append(v)
        keys, nf, flags = [], [], np.zeros(len(want_models), np.uint32)
        fresh = list(fresh)
        for i, want in enumerate(want_models):
            u = rng.random()
            mine = by_amid.get(int(want))
            if fresh and i % 3 == 0:
                k = fresh[(i // 3) % len(fresh)]
            elif u < 0.55 and mine and want >= 0:
                k = vt.ids[mine[int(rng.integers(len(mine)))]]
            elif u < 0.78:
                k = vt.ids[int(rng.integers(len(vt.ids)))]
            elif u < 0.86:
                k = self.vnever[int(rng.integers(len(self.vnever)))]
            elif u < 0.90:
                k = b""
            else:
                k = vt.ids[int(rng.integers(len(vt.ids)))] + b"+"
            keys.append(k)
            rec = vt.rows[vt.row_of[k]] if k in vt.row_of else None
            t = int(rng.integers(0, 6))
            if t <= 1 or rec is None:
                nf.append(None if t == 0 else b"")
            elif t in (2, 3):
                nf.append(rec.amid if rec.amid is not None else b"no-such-active")
            elif t == 4:
                nf.append(rec.tmid if rec.tmid is not None else b"no-such-target")
            else:
                nf.append(self.short_ids[int(rng.integers(len(self.short_ids)))])
            flags[i] = int(rng.integers(0, 2))
        return keys, nf, flags

    def close(self):
        self.m.close()


@pytest.fixture(scope="module")
def vmesh():
    m = VMesh()
    yield m
    m.close()


def head3(keys, nf, flags, n):
    return keys[:n], nf[:n], flags[:n]


def v_calls(s, a, keys, nf, flags, want_vm=True):
    """The three calls on one batch, the `model` fields filled with garbage -> {call: outputs + (vm rows,)}; the caller's arrays
    must come back as they went in."""
    g, p, sr = with_model(a["greqs"], tk.GARBAGE_G), with_model(a["preqs"], tk.GARBAGE_P), a["sreqs"]
    ins = {"g": g, "p": p, "s": sr, "counters": a["counters"], "xp": a["xp"], "xt": a["xt"], "expl": a["expl"], "extra": a["extra"],
           "caller": a["caller"], "pcaller": a["pcaller"]}
    if flags is not None:
        ins["flags"] = flags
    before = {k: v.tobytes() for k, v in ins.items()}
    out = {
        "route": s.route_batch_cv(a["caller"], g, sr, keys, a["counters"], a["xp"], a["xt"], a["expl"], a["now"], EXPIRY, nf, flags, want_vm),
        "miss": s.miss_batch_cv(a["caller"], a["pcaller"], g, p, keys, a["xp"], a["xt"], a["expl"], a["extra"], a["now"], EXPIRY, nf, flags,
                                want_vm),
        "place": s.place_batch_cv(a["pcaller"], p, keys, a["extra"], a["now"], nf, flags, want_vm),
    }
    assert {k: v.tobytes() for k, v in ins.items()} == before  # the caller's arrays are never written
    return out


def v_call_one(s, a, keys, nf, flags, call):
    g, p = with_model(a["greqs"], tk.GARBAGE_G), with_model(a["preqs"], tk.GARBAGE_P)
    if call == "route":
        return s.route_batch_cv(a["caller"], g, a["sreqs"], keys, a["counters"], a["xp"], a["xt"], a["expl"], a["now"], EXPIRY, nf, flags)
    if call == "miss":
        return s.miss_batch_cv(a["caller"], a["pcaller"], g, p, keys, a["xp"], a["xt"], a["expl"], a["extra"], a["now"], EXPIRY, nf, flags)
    return s.place_batch_cv(a["pcaller"], p, keys, a["extra"], a["now"], nf, flags)


def assert_rule(s, a, keys, nf, flags, vk, what):
    """vm_out equals the dicts' answer byte for byte (`reserved` 0 included), every output array equals the _c call's on the rows
    that answer decides — with and without vm_out.  -> the answers"""
    n = len(keys)
    ans = vk.answers(keys, nf, flags)
    rows = vk.decided_rows(ans)
    want = tk.reference_calls(s, a, rows)
    for want_vm in (True, False):
        got = v_calls(s, a, keys, nf, flags, want_vm)
        for call in ("route", "miss", "place"):
            outs, vmo = got[call][:-1], got[call][-1]
            if want_vm:
                assert vmo.dtype == _lib.VSEAM_ROW and len(vmo) == n
                bad = [i for i in range(n) if vmo[i] != ans[i]][:6]
                assert vmo.tobytes() == ans.tobytes(), (what, call, bad, [(vmo[i], ans[i]) for i in bad[:2]])
            else:
                assert vmo is None
            assert all(len(o) == n for o in outs)
            sc.assert_bytes(outs, want[call], (what, call, n, want_vm))
    return ans


def was_staged(s, a, keys, nf, flags):
    g, p = with_model(a["greqs"], tk.GARBAGE_G), with_model(a["preqs"], tk.GARBAGE_P)
    return [tk.staged(s, lambda: s.route_batch_cv(a["caller"], g, a["sreqs"], keys, a["counters"], a["xp"], a["xt"], a["expl"], a["now"],
                                                  EXPIRY, nf, flags))[1],
            tk.staged(s, lambda: s.miss_batch_cv(a["caller"], a["pcaller"], g, p, keys, a["xp"], a["xt"], a["expl"], a["extra"], a["now"],
                                                 EXPIRY, nf, flags))[1],
            tk.staged(s, lambda: s.place_batch_cv(a["pcaller"], p, keys, a["extra"], a["now"], nf, flags))[1]]


# ---- 1. the rule ---------------------------------------------------------------------------------------------------------------
def test_the_vmodels_and_requests_hold_what_part_1_is_about(vmesh):
    m, vt = vmesh, vmesh.vk.vt
    f = vt.flags()
    live = [r for r in vt.rows if r is not None and not r.host]
    assert len(vt.rows) == N_VM and all(N_VM // len(KINDS) <= sum(j % len(KINDS) == k for j in range(N_VM)) for k in range(len(KINDS)))
    assert any(r.amid == r.tmid for r in live) and any(vm.in_transition(r) and not r.failed for r in live)  # defined; in transition
    assert any(vm.in_transition(r) and r.failed for r in live)
    assert (f & vm.F_ACTIVE_NULL).any() and (f & vm.F_TARGET_NULL).any() and any(r.owner is not None for r in live)
    assert any(r.amid is not None and r.amid not in m.km.row for r in live)  # amid naming an id the registry does not have
    assert ((f & vm.F_ABSENT) != 0).sum() == len(m.absent) >= 10 and ((f & vm.F_HOST) != 0).sum() >= 10
    got_ids, got_flags, got_strs = m.s.vmodels_get()
    assert got_ids == vt.ids and np.array_equal(got_flags, f) and got_strs == vt.strings()  # the device holds the same table
    for n in (256, N_MAX):  # the slot's fill and the staged batch each see every class and both choices
        keys, nf, flags = head3(m.keys, m.nf, m.flags, n)
        ans = m.vk.answers(keys, nf, flags)
        assert set(ans["cls"]) == {vm.NOT_FOUND, vm.OK, vm.STRONG_READ, vm.TARGET_NOT_FOUND, vm.HOST}, n
        ok = ans["cls"] == vm.OK
        assert set(ans["which"][ok]) == {vm.ACTIVE, vm.TARGET} and (ans["flags"][ok] & vm.NULL_ID).any()
        assert ((ans["flags"][ok] & vm.NULL_ID == 0) & (ans["model"][ok] < 0)).any()  # OK, an id, unknown to the registry
        assert any(k not in vt.row_of and k for k in keys) and any(k == b"" for k in keys)  # never seen; empty
        in_table = [i for i, k in enumerate(keys) if k in vt.row_of and vt.rows[vt.row_of[k]] is not None and not vt.rows[vt.row_of[k]].host]
        rec = lambda i: vt.rows[vt.row_of[keys[i]]]  # noqa: E731
        for after in (0, 1):  # nf empty / = active only / = target only / = both, each with and without AFTER_STRONG
            sel = [i for i in in_table if flags[i] == after]
            assert any(not nf[i] for i in sel)
            assert any(nf[i] and nf[i] == rec(i).amid and nf[i] != rec(i).tmid for i in sel)
            assert any(nf[i] and nf[i] == rec(i).tmid and nf[i] != rec(i).amid for i in sel)
            assert any(nf[i] and nf[i] == rec(i).amid == rec(i).tmid for i in sel)
    for n in NS:
        ksm.check_mix(m.vk.rows(*head3(m.keys, m.nf, m.flags, n)))
    assert sum(map(len, m.keys[:SLOT_N])) <= SLOT_KEY_BYTES and sum(len(x or b"") for x in m.nf[:SLOT_N]) <= SLOT_NF_BYTES
    a = m.a
    assert len(a["counters"]) <= 4096 and len(a["xp"]) <= 2048 and len(a["expl"]) <= 2048 and len(a["extra"]) <= 2048  # the slots' pools


@pytest.mark.parametrize("n", NS)
def test_vkeyed_calls_equal_the_c_calls_on_the_rows_the_answers_decide(vmesh, n):
    m = vmesh
    a = sc.head(m.a, n)
    keys, nf, flags = head3(m.keys, m.nf, m.flags, n)
    assert_rule(m.s, a, keys, nf, flags, m.vk, "rule")
    if n:
        assert was_staged(m.s, a, keys, nf, flags) == [n > SLOT_N] * 3
        if n in (2, 65, 257):  # NULL nf_keys / nf_off and NULL req_flags: every nf is Java null, no flag is set
            ans = assert_rule(m.s, a, keys, None, None, m.vk, "no nf, no flags")
            assert not set(ans["cls"]) & {vm.STRONG_READ, vm.TARGET_NOT_FOUND}


# ---- 2. the byte limits of a slot -----------------------------------------------------------------------------------------------
def sized(fixed, total, tag):
    """the spans of `fixed` with every None replaced by a distinct filler so that the bytes add up to `total`"""
    holes = [i for i, x in enumerate(fixed) if x is None]
    q, r = divmod(total - sum(len(x) for x in fixed if x is not None), len(holes))
    assert 16 <= q < 200
    out = list(fixed)
    for j, i in enumerate(holes):
        out[i] = (tag + b"-%03d-" % j).ljust(q + (1 if j < r else 0), b"y")
    assert sum(map(len, out)) == total
    return out


@pytest.mark.parametrize("key_bytes,nf_bytes,is_staged", [(SLOT_KEY_BYTES, SLOT_NF_BYTES, False), (SLOT_KEY_BYTES - 1, SLOT_NF_BYTES - 1, False),
                                                         (SLOT_KEY_BYTES + 1, None, True), (None, SLOT_NF_BYTES + 1, True),
                                                         (30_000, 30_000, True)])
def test_the_key_bytes_and_the_nf_bytes_decide_the_path_at_200_requests(vmesh, key_bytes, nf_bytes, is_staged):
    m, n = vmesh, 200
    a = sc.head(m.a, n)
    keys, nf, flags = head3(m.keys, m.nf, m.flags, n)
    vt = m.vk.vt
    if key_bytes is not None:  # a fifth of the keys stay vmodel ids, the rest become never-seen ids of the size that fills the total
        keys = sized([k if i % 5 == 0 and k in vt.row_of else None for i, k in enumerate(keys)], key_bytes, b"vnever-long")
        assert len(set(keys) - set(vt.row_of)) >= 150
    if nf_bytes is not None:  # the nf of the known keys stay (they decide classes), the others are filled up
        nf = sized([(x or b"") if keys[i] in vt.row_of else None for i, x in enumerate(nf)], nf_bytes, b"nf-long")
    if key_bytes == 30_000:
        assert key_bytes > 2 * LDS_BYTES and nf_bytes > 2 * LDS_BYTES  # both workgroups of the call read in place
    ans = assert_rule(m.s, a, keys, nf, flags, m.vk, ("bytes", key_bytes, nf_bytes))
    if key_bytes is not None:
        assert (ans["cls"] == vm.OK).sum() >= 5 and (ans["cls"] == vm.NOT_FOUND).sum() >= 100
    else:
        assert len(set(ans["cls"])) >= 4
    assert was_staged(m.s, a, keys, nf, flags) == [is_staged] * 3


# ---- 3. colliding hashes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [0, 4])
def test_the_rule_when_ids_collide_in_both_tables(monkeypatch, bits):
    """MMP_VMODEL_ID_HASH_BITS and MMP_MODEL_ID_HASH_BITS are read per context: every id of either table shares one hash (0 bits) or
    one of sixteen (4), so both lookups — the second with the hash the row stores — are decided by the bytes."""
    monkeypatch.setenv("MMP_VMODEL_ID_HASH_BITS", str(bits))
    monkeypatch.setenv("MMP_MODEL_ID_HASH_BITS", str(bits))
    m = VMesh(seed=2)
    try:
        for n in (1, 65, 257):
            keys, nf, flags = head3(m.keys, m.nf, m.flags, n)
            ans = assert_rule(m.s, sc.head(m.a, n), keys, nf, flags, m.vk, ("collide", bits))
            if n > 1:
                assert ((ans["cls"] == vm.OK) & (ans["model"] >= 0)).sum() >= n // 8
    finally:
        m.close()


# ---- 4. moving tables ------------------------------------------------------------------------------------------------------------
def check_moving(m, what, fresh=()):
    for n in (1, 65, 257):
        keys, nf, flags = m.requests(m.a["greqs"]["model"][:n], fresh)
        ans = assert_rule(m.s, sc.head(m.a, n), keys, nf, flags, m.vk, (what, n))
        if n > 1:
            assert ((ans["cls"] == vm.OK) & (ans["model"] >= 0)).sum() >= n // 10 and (ans["model"] < 0).sum() >= n // 10, what
    return ans


def test_the_rule_while_the_vmodel_table_and_the_registry_move():
    m = VMesh(seed=3)
    try:
        s, vk, vt, rng = m.s, m.vk, m.vk.vt, np.random.default_rng(41)
        defined = [j for j in range(N_VM) if KINDS[j % len(KINDS)] == "defined"]
        # a transition starts on existing rows (rewritten beside the published ones), then ends
        m.send([m.vids[j] for j in defined], [value(m.amid_of(j), m.amid_of(j + 7)) for j in defined])
        assert all(vm.in_transition(vt.rows[vt.row_of[m.vids[j]]]) for j in defined)
        check_moving(m, "transition started", [m.vids[j] for j in defined])
        m.send([m.vids[j] for j in defined], [value(m.amid_of(j + 7), m.amid_of(j + 7)) for j in defined])
        check_moving(m, "transition ended", [m.vids[j] for j in defined])
        # vmodels join: two growths of the id table, and the string arena outgrows its first allocation several times over
        info0 = s.vmodels_info()
        joiners = ksm.make_ids(rng, 800, tag=b"jv", long_share=0.3)
        long_ids = [k for k in m.ids if len(k) >= 150]
        for step in range(4):
            part = joiners[200 * step: 200 * step + 200]
            vals = [value(long_ids[(step + i) % len(long_ids)] if i % 2 else m.amid_of(i), m.amid_of(i + step)) for i in range(200)]
            assert m.send(part, vals) == 200
            check_moving(m, ("joined", step), part)
        info1 = s.vmodels_info()
        assert info1["capacity"] >= 4 * info0["capacity"] and info1["live_bytes"] > 4 * (info0["arena_bytes"] + 16)
        # rewrites until the arena's garbage outweighs its live bytes: the squeeze swaps rows and arena
        squeezed = 0
        for rep in range(3):
            before = int(s.vmodels_info()["arena_bytes"])
            part = joiners[:600]
            m.send(part, [value(m.amid_of(i + rep), long_ids[(i + rep) % len(long_ids)]) for i in range(600)])
            squeezed += int(s.vmodels_info()["arena_bytes"]) < before  # (an append alone only grows it)
            check_moving(m, ("rewritten", rep), part[rep::50])
        assert squeezed >= 1
        # mmp_vmodels_retire renumbers the vmodel rows
        gone = [m.vids[j] for j in (0, 9, 18)] + joiners[5:700:40]
        m.send(gone, [b""] * len(gone), np.ones(len(gone), np.uint8))
        n_before = len(vt.rows)
        remap, n_after = s.vmodels_retire(all_absent=True)
        vk.retire(remap)
        assert n_after == len(vt.rows) == n_before - len(gone) - len(m.absent) and all(k not in vt.row_of for k in gone)
        keys, nf, flags = m.requests(m.a["greqs"]["model"][:257], gone[:8])
        ans = assert_rule(s, sc.head(m.a, 257), keys, nf, flags, vk, "vmodels retired")
        assert all(ans["cls"][i] == vm.NOT_FOUND and ans["vmodel"][i] == -1 for i in range(0, 24, 3))  # the retired ids
        assert (ans["vmodel"] >= 0).sum() >= 100 and s.vmodels_get()[0] == vt.ids
        check_moving(m, "vmodels retired")
        # mmp_models_retire renumbers the registry rows: a vmodel that names a retired model decides as -1, the others move with it
        named = [r.amid for r in vt.rows if r is not None and not r.host and r.amid in m.km.row]
        gone_models = list(dict.fromkeys(named))[:12]
        st, idx, _, _ = s.models_events_json(gone_models, [""] * len(gone_models), np.ones(len(gone_models), np.uint8))
        assert not st.any() and np.array_equal(idx, m.km.rows(gone_models))
        m.km.retire(s.models_retire(idx, empty_only=True))
        assert np.all(m.km.rows(gone_models) == -1)
        orphans = [k for k in vt.ids if vt.rows[vt.row_of[k]] is not None and vt.rows[vt.row_of[k]].amid in gone_models]
        assert len(orphans) >= 12
        ans = check_moving(m, "models retired", orphans)
        assert any(ans["cls"][i] == vm.OK and ans["model"][i] == -1 and not ans["flags"][i] for i in range(0, 257, 3))
    finally:
        m.close()


# ---- 5. equality with the two-call sequence --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [200, 257])
def test_vm_out_equals_what_mmp_vmodels_resolve_answers_for_the_same_questions(vmesh, n):
    m, s = vmesh, vmesh.s
    keys, nf, flags = head3(m.keys, m.nf, m.flags, n)
    two = s.vmodels_resolve(keys, nf, None, flags)
    a = sc.head(m.a, n)
    for call in ("route", "miss", "place"):
        vmo = v_call_one(s, a, keys, nf, flags, call)[-1]
        for f in ("cls", "which", "vmodel", "model", "flags"):
            assert np.array_equal(vmo[f], two[f]), (call, f)
        assert not vmo["reserved"].any()
    # ... and the decision is the _c call's on the row the two-call host would pass on
    rows = np.where((two["cls"] == vm.OK) & (two["flags"] & vm.NULL_ID == 0), two["model"], -1).astype(np.int32)
    want = tk.reference_calls(s, a, rows)
    got = v_calls(s, a, keys, nf, flags)
    for call in ("route", "miss", "place"):
        sc.assert_bytes(got[call][:-1], want[call], ("two calls", call))


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
SENTINEL = 0xA5
CALLS = ("route", "miss", "place")


def raw_args(m, n):
    a = sc.head(m.a, n)
    a = dict(a, g=with_model(a["greqs"], tk.GARBAGE_G), p=with_model(a["preqs"], tk.GARBAGE_P))
    keys, nf, flags = head3(m.keys, m.nf, m.flags, n)
    blob, off = Solver.pack_keys(keys)
    nblob, noff = Solver.pack_keys([x or b"" for x in nf])
    assert len(nblob) > 0
    a["blob"], a["off"] = np.frombuffer(blob, np.uint8).copy(), off
    a["nblob"], a["noff"], a["flags"] = np.frombuffer(nblob, np.uint8).copy(), noff, flags.copy()
    for k, dt in (("gouts", _lib.GATE_OUT), ("souts", _lib.SERVE_OUT), ("pouts", _lib.PLACE_OUT), ("vm", _lib.VSEAM_ROW)):
        a[k] = np.frombuffer(bytes([SENTINEL]) * (dt.itemsize * n), dtype=dt).copy()
    return a


def raw_calls(s, a, n, which=CALLS):
    """the calls named in `which` on raw pointers (None: NULL) -> their return codes"""
    p = lambda k: ptr(a[k]) if a[k] is not None and len(a[k]) else None  # noqa: E731
    L, now = s.lib, int(a["now"])
    run = {
        "route": lambda: L.mmp_route_batch_cv(s.h, p("caller"), p("g"), p("sreqs"), n, p("blob"), p("off"), p("nblob"), p("noff"), p("flags"),
                                              p("counters"), len(a["counters"]), p("xp"), p("xt"), len(a["xp"]), p("expl"), len(a["expl"]),
                                              now, EXPIRY, p("gouts"), p("souts"), p("vm")),
        "miss": lambda: L.mmp_miss_batch_cv(s.h, p("caller"), p("pcaller"), p("g"), p("p"), n, p("blob"), p("off"), p("nblob"), p("noff"),
                                            p("flags"), p("xp"), p("xt"), len(a["xp"]), p("expl"), len(a["expl"]), p("extra"),
                                            len(a["extra"]), now, EXPIRY, p("gouts"), p("pouts"), p("vm")),
        "place": lambda: L.mmp_place_batch_cv(s.h, p("pcaller"), p("p"), n, p("blob"), p("off"), p("nblob"), p("noff"), p("flags"), p("extra"),
                                              len(a["extra"]), now, p("pouts"), p("vm")),
    }
    return tuple(run[c]() for c in which)


def outputs(a):
    return {k: a[k].tobytes() for k in ("gouts", "souts", "pouts", "vm")}


@pytest.mark.parametrize("n", [2, 300])
def test_einval_leaves_every_output_as_it_was(vmesh, n):
    s, a = vmesh.s, raw_args(vmesh, n)
    before = outputs(a)
    INT_MAX = 2**31 - 1

    def falling(off):
        f = off.copy()
        f[n - 1] = f[n] + 1
        return f

    bad_flags = a["flags"].copy()
    bad_flags[n - 1] |= 2
    cases = [("null key_off", dict(a, off=None), n, CALLS), ("key offsets that fall", dict(a, off=falling(a["off"])), n, CALLS),
             ("null keys with bytes present", dict(a, blob=None), n, CALLS), ("n < 0", a, -1, CALLS),
             ("nf offsets that fall", dict(a, noff=falling(a["noff"])), n, CALLS),
             ("null nf_keys with nf bytes present", dict(a, nblob=None), n, CALLS),
             ("unknown flag bits", dict(a, flags=bad_flags), n, CALLS),
             ("every flag bit", dict(a, flags=np.full(n, 0xFFFFFFFF, np.uint32)), n, CALLS)]
    # what the _ck forms refuse of the rows: a range outside a pool, in the last row, for the calls that read that array
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
    assert a["vm"].tobytes() == vmesh.vk.answers(*head3(vmesh.keys, vmesh.nf, vmesh.flags, n)).tobytes()
    # NULL nf_off with nf_keys given, and NULL vm_out, are valid calls
    assert raw_calls(s, dict(a, noff=None), n) == (MMP_OK,) * 3 and raw_calls(s, dict(a, vm=None), n) == (MMP_OK,) * 3


@pytest.mark.parametrize("n", [2, 300])
def test_estate_as_the_ck_forms_and_a_context_without_a_vmodel_call_answers_not_found(n):
    m = VMesh(seed=4, send=False, load_ids=False)
    try:
        s, a = m.s, raw_args(m, n)
        before = outputs(a)
        assert raw_calls(s, a, n) == (MMP_ESTATE,) * 3  # before mmp_model_ids_load
        assert "mmp_model_ids_load" in (s.lib.mmp_last_error(s.h) or b"").decode()
        assert raw_calls(s, a, 0) == (MMP_ESTATE,) * 3  # (n = 0 is a valid call: it is answered from the state alone)
        assert outputs(a) == before
        assert raw_calls(s, dict(a, noff=np.flip(a["noff"]).copy()), n) == (MMP_EINVAL,) * 3  # the arguments are looked at first
        s.model_ids_load(m.ids)
        assert raw_calls(s, a, 0) == (MMP_OK,) * 3
        # no vmodel call yet: the vmodel table is empty, a valid call, every request NOT_FOUND and decided as model -1
        assert int(s.vmodels_info()["n_rows"]) == 0 and m.vk.vt.rows == []
        b = sc.head(m.a, n)
        ans = assert_rule(s, b, *head3(m.keys, m.nf, m.flags, n), m.vk, "no vmodel call yet")
        assert np.all(ans["cls"] == vm.NOT_FOUND) and np.all(ans["vmodel"] == -1)
        # ... and the first vmodel call is seen by the next request
        m.send(m.vids, m.values)
        ans = assert_rule(s, b, *head3(m.keys, m.nf, m.flags, n), m.vk, "first vmodel call")
        if n > 2:
            assert (ans["cls"] == vm.OK).sum() >= n // 10
    finally:
        m.close()


# ---- 7. beside writers -----------------------------------------------------------------------------------------------------------
def test_vkeyed_calls_beside_vmodel_writers_and_holders_of_the_batch_lock():
    """One thread issues _cv calls (n = 1 and n = 200), the main thread sends 200 event batches that flip vmodels between two known
    targets, join new vmodels, squeeze (the rewrites' garbage) and retire once, a third thread holds batch_mu with 20 000-row
    host-pointer batches.  Nobody waits for anybody.  Afterwards every recorded answer must be one the dicts gave in SOME state the
    writer went through for that request — for a flipping vmodel the two targets, for a joining one NOT_FOUND or its record, around
    the retire the old or the new numbering — and its result rows those of the _c call on the row it names."""
    m = VMesh(seed=5)
    s, a, vk, rng = m.s, m.a, m.vk, np.random.default_rng(77)
    try:
        flip = [j for j in range(N_VM) if KINDS[j % len(KINDS)] in ("defined", "owner", "transition")]
        doomed = [m.vids[j] for j in range(N_VM) if KINDS[j % len(KINDS)] == "target null"][:6]
        joiners = ksm.make_ids(rng, 200, tag=b"lv")
        state_values = [[value(m.amid_of(j + 3 * k), m.amid_of(j + 3 * k)) for j in flip] for k in (0, 1)]
        flip_ids = [m.vids[j] for j in flip]
        m.send(flip_ids, state_values[0])
        # the calls: the first 200 requests, and 16 lone requests; keys of flipping, doomed and joining vmodels among them
        keys, nf, flags = m.requests(a["greqs"]["model"][:200])
        for i in range(0, 200, 5):
            q = (i // 5) % len(flip)  # (every other one with nf = its first target: STRONG_READ / TARGET_NOT_FOUND in that state)
            keys[i], nf[i] = flip_ids[q], (None if i % 2 == 0 else m.amid_of(flip[q]))
        for i in range(1, 200, 20):
            keys[i] = joiners[(7 * i) % 200]
        for i in range(2, 200, 40):
            keys[i] = doomed[(i // 40) % len(doomed)]
        variants = [(sc.head(a, 200), keys, nf, flags)]
        for w in range(16):
            lo = 12 * w
            b = {k: (np.ascontiguousarray(a[k][lo:lo + 1]) if k in ("greqs", "sreqs", "preqs") else a[k]) for k in a}
            variants.append((b, keys[lo:lo + 1], nf[lo:lo + 1], flags[lo:lo + 1]))
        allowed = [[set() for _ in v[1]] for v in variants]

        def note_state():
            for v, (_, vkeys, vnf, vflags) in enumerate(variants):
                for i, row in enumerate(vk.answers(vkeys, vnf, vflags)):
                    allowed[v][i].add(tuple(int(x) for x in row))

        note_state()
        big_n = 20_000  # a host-pointer batch past every slot: staged, the batch lock held for the whole call
        big = wl.make_requests(m.m.fleet, 9, n=big_n, extra_frac=0.0)[0]
        big_c = np.zeros(big_n, dtype=_lib.PLACE_REQ_C)
        for f in _lib.PLACE_REQ_C.names:
            big_c[f] = big[f]
        big_want = s.place_c(a["pcaller"], big_c, None, a["now"])
        errors, record = [], []

        def caller_thread():
            try:
                for rep in range(600):
                    v = 0 if rep % 2 else 1 + (rep // 2) % 16
                    b, vkeys, vnf, vflags = variants[v]
                    call = CALLS[rep % 3]
                    record.append((v, call, v_call_one(s, b, vkeys, vnf, vflags, call)))  # (an error code raises)
            except BaseException as e:  # noqa: BLE001
                errors.append(e)

        def big_thread():
            try:
                for k in range(12):
                    sc.assert_bytes((s.place_c(a["pcaller"], big_c, None, a["now"]),), (big_want,), ("big", k))
            except BaseException as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=caller_thread), threading.Thread(target=big_thread)]
        for th in threads:
            th.start()
        squeezed = retired = 0
        for k in range(200):  # the writer: bounded, unpaced
            before = int(s.vmodels_info()["arena_bytes"])
            ev_keys, ev_vals = list(flip_ids), list(state_values[(k + 1) % 2])
            if k % 20 == 0:
                part = joiners[k: k + 20]
                ev_keys += part
                ev_vals += [value(m.amid_of(k + i), m.amid_of(k + i + 1)) for i in range(20)]
            m.send(ev_keys, ev_vals)
            note_state()
            squeezed += int(s.vmodels_info()["arena_bytes"]) < before
            if k == 100:
                m.send(doomed, [b""] * len(doomed), np.ones(len(doomed), np.uint8))
                note_state()
                remap, _ = s.vmodels_retire(all_absent=True)
                vk.retire(remap)
                note_state()
                retired += int((remap < 0).sum())
        for th in threads:
            th.join()
        assert not errors, errors[:2]
        assert len(record) == 600 and squeezed >= 1 and retired >= len(doomed) and len(vk.vt.rows) == N_VM + 200 - retired
        # the flipping keys have two states each (four around the retire), the joining ones NOT_FOUND and their record
        assert all(len(allowed[0][i]) >= 2 for i in range(0, 200, 5)) and all(len(allowed[0][i]) >= 2 for i in range(1, 200, 20))
        # the registry never moved: the _c calls on every row a request could be decided on, per variant
        refs = []
        for v, (b, vkeys, _, _) in enumerate(variants):
            poss = [sorted({(t[3] if t[0] == vm.OK and not t[4] & vm.NULL_ID else -1) for t in allowed[v][i]}) for i in range(len(vkeys))]
            depth = max(map(len, poss))
            by_depth = []
            for d in range(depth):
                rows = np.array([p[min(d, len(p) - 1)] for p in poss], np.int32)
                by_depth.append((rows, tk.reference_calls(s, b, rows)))
            refs.append(by_depth)
        for v, call, got in record:
            outs, vmo = got[:-1], got[-1]
            n = len(vmo)
            for i in range(n):
                t = tuple(int(x) for x in vmo[i])
                assert t in allowed[v][i], (v, call, i, t, sorted(allowed[v][i]))
            decided = vksm.VKeyRows.decided_rows(vmo)
            covered = np.zeros(n, bool)
            for rows, want in refs[v]:
                hit = (decided == rows) & ~covered
                for o, w in zip(outs, want[call]):
                    assert o[hit].tobytes() == w[hit].tobytes(), (v, call)
                covered |= hit
            assert covered.all()
        # afterwards every key answers the final state
        for b, vkeys, vnf, vflags in variants[:4]:
            assert v_call_one(s, b, vkeys, vnf, vflags, "route")[-1].tobytes() == vk.answers(vkeys, vnf, vflags).tobytes()
    finally:
        m.close()


# ---- 8. twice ---------------------------------------------------------------------------------------------------------------------
def test_two_runs_over_the_same_state_are_byte_identical(vmesh):
    runs = [v_calls(vmesh.s, vmesh.a, vmesh.keys, vmesh.nf, vmesh.flags) for _ in range(2)]
    for call in CALLS:
        sc.assert_bytes(runs[0][call], runs[1][call], (call, "twice"))
