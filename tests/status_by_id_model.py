"""getStatus by model id and getVModelStatus, restated in plain sequential Python: the oracle of mmp_models_status_k and
mmp_vmodels_status (modelmesh_amd/csrc/status_keyed_kernels.hpp).  Every step cites the Java it stands for (VModelManager.java =
VMM :505-559, ModelMesh.java = MM :3247-3263).

State (class State): the records as Python objects, not the library's lookups —
  models   a dict from model id (bytes) to its ModelRecord (tests/registry_ops_model.py), None for a DELETED record: the id keeps
           its registry row, which is the empty row.  A live record that is indistinguishable from that row (type 0, no copies,
           lastUsed 0) is taken for deleted as well: the library's rule (retire_row_empty), stated here and nowhere hidden
  ids      the registry's ids in row order — the numbering the answers carry (model_idx, model, target_model)
  vmt      a tests/vmodel_model.VModels: the vmodel records (Row or None) by vmodel id, and their numbering

What is already stated elsewhere is called, not restated: makeStatusInfo and the status class (tests/model_status_model.py:
make_status_info, status_class), absentOrOwnerMismatch, inTransition and the classes of statusFromRecord /
resolveTargetModelStatusInfo (tests/vmodel_model.py: VModels.resolve, in_transition).

One call uses one clock value.  The strong read (VMM:514-525) is a round trip of the host's: the device answers
MMP_VMR_STRONG_READ with everything filled in, the host performs getStrong, sends the value as an event and asks again with
AFTER_STRONG; `after_strong` is that second question, answered from the (fresh) state as it stands (:519-524)."""
from collections import namedtuple

import numpy as np

from modelmesh_amd import _lib
from modelmesh_amd._lib import MST_NOT_FOUND, MSTF_MISS, STATUS_COPY, STATUS_ROW, VSTATUS_ROW
from tests import vmodel_model as vm
from tests.model_status_model import make_status_info, status_class

StatusInfo = namedtuple("StatusInfo", "cls n_not_checked n_failed copies")
VStatus = namedtuple("VStatus", "vrow active target strings")  # vrow: the 8 words of mmp_vstatus_row; strings: (amid, tmid, o) or None


def is_empty_record(mr):
    return mr is None or (mr.type == 0 and not mr.instance_ids and not mr.load_failed_instance_ids and mr.last_used == 0)


class State:
    def __init__(self, ids, records, vmt=None):
        self.ids = [k if isinstance(k, bytes) else k.encode() for k in ids]
        self.models = dict(zip(self.ids, records))
        assert len(self.models) == len(self.ids)
        self.vmt = vmt if vmt is not None else vm.VModels()

    def row(self, mid):
        return self.ids.index(mid) if mid in self.models else -1

    def registry(self):
        """The vm.Registry the vmodel model's questions look models up in: (n_loaded, n_failed, last_used, type) per row."""
        recs = []
        for k in self.ids:
            mr = self.models[k]
            recs.append((0, 0, 0, 0) if mr is None else (len(mr.instance_ids), len(mr.load_failed_instance_ids), mr.last_used, mr.type))
        return vm.Registry(self.ids, recs)


def get_status(state, model_id, now, id_order, fail_pod=-1, miss=False):
    """MM:3247-3263 getStatus(modelId) -> StatusInfo.  fail_pod / miss: the overlay and the exhausted cache-hit loop of the class
    (tests/model_status_model.py), -1 / False for getVModelStatus's two questions."""
    mr = None if model_id is None else state.models.get(model_id)          # :3256 internalOperation -> the registry's record
    if is_empty_record(mr):                                                # :3257 ModelNotFoundException -> SI_NOT_FOUND
        mr = None
    inst, fails, copies = make_status_info(mr, fail_pod, now, id_order)    # :3013-3058
    return StatusInfo(status_class(mr, fail_pod, miss, inst, fails), len(inst), len(fails), copies)


DEFAULT_VROW = (vm.NOT_FOUND, -1, -1, -1, 0, 0, 0, 0)


def get_vmodel_status(state, vmid, owner, after_strong, now, id_order):
    """VMM:505-559 getVModelStatus(vmid, owner) -> VStatus."""
    owner = owner or None                                                  # :506 emptyToNull
    if owner is not None and not isinstance(owner, bytes):
        owner = owner.encode()
    key = vmid if isinstance(vmid, bytes) else vmid.encode()
    v = state.vmt.row_of.get(key, -1)
    vmr = state.vmt.rows[v] if v >= 0 else None                            # :507 vModels.getOrStrongIfAbsent(vmid)
    none = get_status(state, None, now, id_order)
    if vmr is None or (not vmr.host and owner is not None and vmr.owner != owner):  # :508, :530-532 absentOrOwnerMismatch
        return VStatus(DEFAULT_VROW, none, none, None)                     # :509 getDefaultInstance(): nothing of the record
    if vmr.host:                                                           # an escape in a string: the host decodes the record
        return VStatus((vm.HOST, v, -1, -1, 0, 0, 0, 0), none, none, None)
    reg = state.registry()
    a = state.vmt.resolve(reg, key, None, owner, after_strong)             # the classes vmodel_model.py states (:555-556, :537-549)
    assert a.cls == vm.OK and a.vmodel == v
    model_id = vmr.amid                                                    # :511
    si = get_status(state, model_id, now, id_order)                        # :513 modelMesh.getStatus(modelId)
    cls = vm.OK
    if si.cls == MST_NOT_FOUND and not after_strong:                       # :514-515: vModels.getStrong is the host's; it asks again
        cls = vm.STRONG_READ
    # (after the strong read :516-524 is this function again over the fresh record: absentOrOwnerMismatch, getStatus of ITS
    # active model, and a NOT_FOUND that stands with a warning, :521-523)
    tmsi = none                                                            # :538-540 not in transition: null (no target status)
    if vm.in_transition(vmr):                                              # :538
        tmsi = get_status(state, vmr.tmid, now, id_order)                  # :541, :547-548 (targetModel == null -> NOT_FOUND)
    flags = vm.row_flags(vmr) & _lib.VMF_REPLY
    vrow = (cls, v, reg.row(vmr.amid), a.target_model, a.vstatus, a.target_status, flags, 0)
    return VStatus(vrow, si, tmsi, (vmr.amid, vmr.tmid, vmr.owner))        # :553-558 statusFromRecord: the three ids and both answers


# ---- a batch in the library's layout ------------------------------------------------------------------------------------------

def _rows_and_copies(infos):
    rows, out = np.zeros(len(infos), STATUS_ROW), []
    for i, si in enumerate(infos):
        rows[i] = (si.cls, len(out), si.n_not_checked, si.n_failed)
        out.extend(si.copies)
    return rows, np.array(out, dtype=STATUS_COPY).reshape(-1)


def models_status_k(state, keys, now, id_order, fail_pod=None, flags=None):
    """-> (model_idx, rows, copies) as mmp_models_status_k answers."""
    keys = [k if isinstance(k, bytes) else k.encode() for k in keys]
    idx = np.array([state.row(k) for k in keys], np.int32).reshape(-1)
    infos = [get_status(state, k, now, id_order, -1 if fail_pod is None else int(fail_pod[i]),
                        bool(flags is not None and int(flags[i]) & MSTF_MISS)) for i, k in enumerate(keys)]
    return (idx,) + _rows_and_copies(infos)


def vmodels_status(state, keys, now, id_order, owners=None, req_flags=None):
    """-> dict(vrows, rows, copies, str_off, str_bytes) as mmp_vmodels_status answers."""
    n = len(keys)
    ans = [get_vmodel_status(state, keys[i], None if owners is None else owners[i],
                             bool(req_flags is not None and int(req_flags[i]) & 1), now, id_order) for i in range(n)]
    vrows = np.array([a.vrow for a in ans], dtype=VSTATUS_ROW).reshape(-1)
    rows, copies = _rows_and_copies([si for a in ans for si in (a.active, a.target)])
    off, blob = [0], b""
    for a in ans:
        for s in (a.strings or (None, None, None)):
            blob += s or b""
            off.append(len(blob))
    return dict(vrows=vrows, rows=rows, copies=copies, str_off=np.array(off, np.int32), str_bytes=blob)
