"""The boundaries of getVModelStatus (VModelManager.java:505-559) and of getStatus by model id (MM.java:3247-3263) worked by hand
through tests/status_by_id_model.py: every expected value below is written out, not computed.  tests/test_status_by_id_gpu.py
replays the same world and the same cases on the device."""
import numpy as np

from modelmesh_amd import _lib
from modelmesh_amd._lib import (MST_ASK, MST_LOADING_FAILED, MST_NOT_FOUND, MST_NOT_LOADED, VMF_ACTIVE_NULL, VMF_FAILED, VMF_OWNER_NULL,
                                VMF_TARGET_NULL, VMR_HOST, VMR_NOT_FOUND, VMR_OK, VMR_STRONG_READ, VMS_DEFINED, VMS_TRANSITION_FAILED,
                                VMS_TRANSITIONING, VMT_LOADING, VMT_LOADING_FAILED, VMT_NONE, VMT_NOT_FOUND)
from tests import status_by_id_model as sb
from tests import vmodel_model as vm
from tests.registry_ops_model import ModelRecord

NOW = 1_700_000_000_000
ID_ORDER = list(range(8))
NC, LF = _lib.COPY_NOT_CHECKED, _lib.COPY_LOADING_FAILED

# the registry, in row order; E is a deleted record (its row is the empty row), "" is an id like any other
MODEL_IDS = [b"A", b"B", b"C", b"D", b"E", b""]


def hand_records():
    return [ModelRecord(0, [(0, 100), (1, 300)], [], 5),           # A: two copies
            ModelRecord(0, [], [(2, 200)], 5),                     # B: only a failure
            ModelRecord(0, [(3, 50)], [(4, 60)], 5),               # C: a failure and a copy
            ModelRecord(0, [], [], 7),                             # D: registered, nothing loaded
            None,                                                  # E: deleted
            ModelRecord(0, [(5, 10)], [], 5)]                      # "": one copy


# the vmodels: (id, stored value or None for a deleted one)
VMODELS = [
    (b"v_def", vm.render("A", "A", "own")),
    (b"v_tr", vm.render("A", "D")),
    (b"v_failB", vm.render("A", "B", "own", failed=True)),
    (b"v_failC", vm.render("A", "C", failed=True)),
    (b"v_failX", vm.render("A", "nope", failed=True)),
    (b"v_failE", vm.render("A", "E", failed=True)),
    (b"v_anull", vm.render(None, "A")),
    (b"v_tnull", vm.render("A", None)),
    (b"v_bothnull", vm.render(None, None, "own")),
    (b"v_ghost", vm.render("ghost", "ghost")),
    (b"v_del", vm.render("E", "E")),
    (b"v_host", vm.render("es\\c", "A")),
    (b"v_gone", None),
    (b"v_empty", vm.render("", "", "")),
    (b"v_same", vm.render("C", "C", "own")),
]
VROW_OF = {k: i for i, (k, _) in enumerate(VMODELS)}
A_COPIES = [(1, NC, 300), (0, NC, 100)]      # latest first
B_COPIES = [(2, LF, 200)]
C_COPIES = [(4, LF, 60), (3, NC, 50)]
E_COPIES = [(5, NC, 10)]
NONE = (MST_NOT_FOUND, [])
ASK_A, ASK_C = (MST_ASK, A_COPIES), (MST_ASK, C_COPIES)

# (vmodel id, owner, after_strong) -> (cls, model, target_model, vstatus, target_status, flags, active, target, strings)
# model / target_model are registry rows (A 0, B 1, C 2, D 3, E 4, "" 5)
CASES = {
    "no owner given":            ((b"v_def", None, False), (VMR_OK, 0, 0, VMS_DEFINED, VMT_NONE, 0, ASK_A, NONE, (b"A", b"A", b"own"))),
    "owner equal":               ((b"v_def", b"own", False), (VMR_OK, 0, 0, VMS_DEFINED, VMT_NONE, 0, ASK_A, NONE, (b"A", b"A", b"own"))),
    "owner differs":             ((b"v_def", b"owm", False), None),
    "owner a prefix":            ((b"v_def", b"ow", False), None),
    "owner against OWNER_NULL":  ((b"v_tr", b"own", False), None),
    "owner '' is null":          ((b"v_tr", b"", False), (VMR_OK, 0, 3, VMS_TRANSITIONING, VMT_LOADING, VMF_OWNER_NULL, ASK_A, (MST_NOT_LOADED, []), (b"A", b"D", None))),
    "stored owner '' asked null": ((b"v_empty", None, False), (VMR_OK, 5, 5, VMS_DEFINED, VMT_NONE, 0, (MST_ASK, E_COPIES), NONE, (b"", b"", b""))),
    "stored owner '' asked x":   ((b"v_empty", b"x", False), None),
    "failed, target only failures": ((b"v_failB", b"own", False), (VMR_OK, 0, 1, VMS_TRANSITION_FAILED, VMT_LOADING_FAILED, VMF_FAILED, ASK_A, (MST_LOADING_FAILED, B_COPIES), (b"A", b"B", b"own"))),
    "failed, target failures and a copy": ((b"v_failC", None, False), (VMR_OK, 0, 2, VMS_TRANSITION_FAILED, VMT_LOADING, VMF_FAILED | VMF_OWNER_NULL, ASK_A, ASK_C, (b"A", b"C", None))),
    "failed, target without a record": ((b"v_failX", None, False), (VMR_OK, 0, -1, VMS_TRANSITION_FAILED, VMT_NOT_FOUND, VMF_FAILED | VMF_OWNER_NULL, ASK_A, NONE, (b"A", b"nope", None))),
    "failed, target deleted":    ((b"v_failE", None, False), (VMR_OK, 0, 4, VMS_TRANSITION_FAILED, VMT_NOT_FOUND, VMF_FAILED | VMF_OWNER_NULL, ASK_A, NONE, (b"A", b"E", None))),
    "amid null":                 ((b"v_anull", None, False), (VMR_STRONG_READ, -1, 0, VMS_TRANSITIONING, VMT_LOADING, VMF_ACTIVE_NULL | VMF_OWNER_NULL, NONE, ASK_A, (None, b"A", None))),
    "amid null, after":          ((b"v_anull", None, True), (VMR_OK, -1, 0, VMS_TRANSITIONING, VMT_LOADING, VMF_ACTIVE_NULL | VMF_OWNER_NULL, NONE, ASK_A, (None, b"A", None))),
    "tmid null":                 ((b"v_tnull", None, False), (VMR_OK, 0, -1, VMS_TRANSITIONING, VMT_NOT_FOUND, VMF_TARGET_NULL | VMF_OWNER_NULL, ASK_A, NONE, (b"A", None, None))),
    "both null":                 ((b"v_bothnull", b"own", False), (VMR_STRONG_READ, -1, -1, VMS_DEFINED, VMT_NONE, VMF_ACTIVE_NULL | VMF_TARGET_NULL, NONE, NONE, (None, None, b"own"))),
    "amid == tmid":              ((b"v_same", None, False), (VMR_OK, 2, 2, VMS_DEFINED, VMT_NONE, 0, ASK_C, NONE, (b"C", b"C", b"own"))),
    "active unknown":            ((b"v_ghost", None, False), (VMR_STRONG_READ, -1, -1, VMS_DEFINED, VMT_NONE, VMF_OWNER_NULL, NONE, NONE, (b"ghost", b"ghost", None))),
    "active unknown, after":     ((b"v_ghost", None, True), (VMR_OK, -1, -1, VMS_DEFINED, VMT_NONE, VMF_OWNER_NULL, NONE, NONE, (b"ghost", b"ghost", None))),
    "active deleted":            ((b"v_del", None, False), (VMR_STRONG_READ, 4, 4, VMS_DEFINED, VMT_NONE, VMF_OWNER_NULL, NONE, NONE, (b"E", b"E", None))),
    "active deleted, after":     ((b"v_del", None, True), (VMR_OK, 4, 4, VMS_DEFINED, VMT_NONE, VMF_OWNER_NULL, NONE, NONE, (b"E", b"E", None))),
    "host row":                  ((b"v_host", None, False), "host"),
    "host row, any owner":       ((b"v_host", b"zzz", True), "host"),
    "deleted vmodel":            ((b"v_gone", None, False), None),
    "unknown vmodel":            ((b"v_never", b"own", True), None),
}


def hand_state():
    st = sb.State(MODEL_IDS, hand_records())
    keys = [k for k, _ in VMODELS]
    status, _, n_app = st.vmt.events(keys, [v or "" for _, v in VMODELS], np.array([v is None for _, v in VMODELS], np.uint8))
    # (a deletion never appends: v_gone joins with a value first, then goes)
    st.vmt.events([b"v_gone"], [vm.render("A", "A")], None)
    st.vmt.events([b"v_gone"], [""], np.ones(1, np.uint8))
    return st


def hand_vmodel_events():
    """The same three batches for a device context: [(keys, values, deleted)]."""
    keys = [k for k, _ in VMODELS]
    return [(keys, [v or "" for _, v in VMODELS], np.array([v is None for _, v in VMODELS], np.uint8)),
            ([b"v_gone"], [vm.render("A", "A")], None), ([b"v_gone"], [""], np.ones(1, np.uint8))]


def expected(st, name):
    """The hand-written answer of a case as a sb.VStatus."""
    (vmid, owner, after), want = CASES[name]
    none = sb.StatusInfo(MST_NOT_FOUND, 0, 0, [])
    if want is None:
        return sb.VStatus(sb.DEFAULT_VROW, none, none, None)
    v = st.vmt.row_of[vmid]
    if want == "host":
        return sb.VStatus((VMR_HOST, v, -1, -1, 0, 0, 0, 0), none, none, None)
    cls, model, target, vstatus, tstatus, flags, active, tgt, strings = want

    def info(a):
        return sb.StatusInfo(a[0], sum(c[1] == NC for c in a[1]), sum(c[1] == LF for c in a[1]), list(a[1]))
    return sb.VStatus((cls, v, model, target, vstatus, tstatus, flags, 0), info(active), info(tgt), strings)


def test_the_vmodel_ids_keep_their_numbers():
    st = hand_state()
    # v_gone was refused by the first batch (a deletion never appends) and joined behind the others
    assert st.vmt.row_of[b"v_gone"] == len(VMODELS) - 1 and st.vmt.rows[st.vmt.row_of[b"v_gone"]] is None
    assert st.vmt.rows[st.vmt.row_of[b"v_host"]].host


def test_every_boundary_by_hand():
    st = hand_state()
    for name, ((vmid, owner, after), _) in CASES.items():
        got = sb.get_vmodel_status(st, vmid, owner, after, NOW, ID_ORDER)
        assert got == expected(st, name), (name, got, expected(st, name))


def test_every_class_occurs_among_the_hand_cases():
    st = hand_state()
    got = [sb.get_vmodel_status(st, *CASES[n][0], NOW, ID_ORDER) for n in CASES]
    assert {g.vrow[0] for g in got} == {VMR_NOT_FOUND, VMR_OK, VMR_STRONG_READ, VMR_HOST}
    assert {g.vrow[4] for g in got} == {VMS_DEFINED, VMS_TRANSITIONING, VMS_TRANSITION_FAILED}
    assert {g.vrow[5] for g in got} == {VMT_NONE, VMT_LOADING, VMT_LOADING_FAILED, VMT_NOT_FOUND}
    assert {g.active.cls for g in got} | {g.target.cls for g in got} == {MST_NOT_FOUND, MST_NOT_LOADED, MST_LOADING_FAILED, MST_ASK}


def test_the_strong_read_round_trip():
    """:514-525: the first answer asks for the strong read; the fresh record names another active model; the second stands."""
    st = hand_state()
    first = sb.get_vmodel_status(st, b"v_ghost", None, False, NOW, ID_ORDER)
    assert first.vrow[0] == VMR_STRONG_READ and first.strings == (b"ghost", b"ghost", None)
    st.vmt.events([b"v_ghost"], [vm.render("B", "ghost")], None)           # :516 getStrong found a newer record
    second = sb.get_vmodel_status(st, b"v_ghost", None, True, NOW, ID_ORDER)
    assert second.vrow[0] == VMR_OK and second.active == sb.StatusInfo(MST_LOADING_FAILED, 0, 1, B_COPIES)      # :520
    assert second.vrow[4:6] == (VMS_TRANSITIONING, VMT_NOT_FOUND) and second.target.cls == MST_NOT_FOUND
    st.vmt.events([b"v_ghost"], [""], np.ones(1, np.uint8))                # or the strong read finds it gone
    assert sb.get_vmodel_status(st, b"v_ghost", None, True, NOW, ID_ORDER).vrow == sb.DEFAULT_VROW              # :517-518


def test_an_owner_mismatch_says_nothing_of_the_record():
    st = hand_state()
    a = sb.get_vmodel_status(st, b"v_failB", b"other", False, NOW, ID_ORDER)
    b = sb.get_vmodel_status(st, b"v_never", b"other", False, NOW, ID_ORDER)
    assert a == b


def test_get_status_by_id_by_hand():
    st = hand_state()
    keys = [b"A", b"B", b"C", b"D", b"E", b"", b"nope", b"A", b"A", b"E", b"nope"]
    fail_pod = [-1, -1, -1, -1, -1, -1, -1, 1, 6, 2, 2]
    flags = [0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0]
    idx, rows, copies = sb.models_status_k(st, keys, NOW, ID_ORDER, fail_pod, flags)
    assert idx.tolist() == [0, 1, 2, 3, 4, 5, -1, 0, 0, 4, -1]
    assert rows["cls"].tolist() == [MST_ASK, MST_LOADING_FAILED, MST_LOADING_FAILED, MST_NOT_LOADED, MST_NOT_FOUND, MST_NOT_LOADED,
                                    MST_NOT_FOUND, MST_ASK, MST_LOADING_FAILED, MST_NOT_FOUND, MST_NOT_FOUND]
    assert rows["n_not_checked"].tolist() == [2, 0, 1, 0, 0, 1, 0, 1, 2, 0, 0]
    assert rows["n_failed"].tolist() == [0, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1]
    assert rows["copy_off"].tolist() == [0, 2, 3, 5, 5, 5, 6, 6, 8, 11, 12]
    # A with instance 1's load failed now: its loaded entry leaves, the failure is the latest
    assert [tuple(int(x) for x in c) for c in copies[6:8]] == [(1, LF, NOW), (0, NC, 100)]
    # the deleted record and the unknown id with a failure reported: no record, the overlay's entry alone (makeStatusInfo(…, mle, null))
    assert [tuple(int(x) for x in c) for c in copies[11:13]] == [(2, LF, NOW), (2, LF, NOW)]


def test_a_live_record_equal_to_the_empty_row_is_taken_for_deleted():
    st = sb.State([b"Z"], [ModelRecord(0, [], [], 0)])
    assert sb.get_status(st, b"Z", NOW, ID_ORDER).cls == MST_NOT_FOUND
    st = sb.State([b"Z"], [ModelRecord(0, [], [], 1)])
    assert sb.get_status(st, b"Z", NOW, ID_ORDER).cls == MST_NOT_LOADED
