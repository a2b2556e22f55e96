"""The oracle of tests/test_vkeyed_seams_gpu.py for WHICH REGISTRY ROW a (vmodel key, notFoundModelId, flags) names, and for the
mmp_vseam_row the call answers beside it: the composition of two sequential models, both kept in step with the events the test
sends and neither touching the library's lookup —

    tests/vmodel_model.py      VModels: the vmodel table, and resolveVModelId (VModelManager.java:569-597) restated in Python
    tests/keyed_seam_model.py  KeyRows: model id -> registry row

resolveVModelId on the request path takes no owner, and its answer reaches a decision only when the class is OK and the id it
names is one the registry knows: every other class, a null id and an unknown id decide as model -1."""
import numpy as np

from tests import vmodel_model as vm
from tests.keyed_seam_model import KeyRows

VSEAM_FIELDS = ("cls", "which", "vmodel", "model", "flags", "reserved")
AFTER_STRONG = 1


class _RowsOnly:
    """The registry as VModels.resolve asks for it, answered from the KeyRows dict.  Every row is `empty`: the request path does
    not read the registry rows, and the target's status is not part of a mmp_vseam_row."""

    def __init__(self, km):
        self.km = km

    def row(self, mid):
        return -1 if mid is None else self.km.row.get(mid, -1)

    def empty(self, i):
        return True


class VKeyRows:
    """vmodel id (bytes) -> vmodel row -> VModelRecord -> chosen model id -> registry row"""

    def __init__(self, km: KeyRows):
        self.km, self.vt = km, vm.VModels()

    def events(self, keys, values, deleted=None, append=True):
        return self.vt.events(keys, values, deleted, append)

    def retire(self, remap):
        """mmp_vmodels_retire returned remap[old row] = new row, -1 for a retired one"""
        vt = self.vt
        assert len(remap) == len(vt.rows)
        keep = [(int(remap[r]), k, vt.rows[r]) for r, k in enumerate(vt.ids) if remap[r] >= 0]
        keep.sort()
        assert [r for r, _, _ in keep] == list(range(len(keep)))
        vt.ids = [k for _, k, _ in keep]
        vt.rows = [row for _, _, row in keep]
        vt.row_of = {k: r for r, k in enumerate(vt.ids)}

    def answer(self, key, nf=None, flags=0):
        """-> (cls, which, vmodel, model, flags, reserved) of request (key, nf, flags)"""
        a = self.vt.resolve(_RowsOnly(self.km), key, nf, None, bool(flags & AFTER_STRONG))
        return (a.cls, a.which, a.vmodel, a.model, a.flags, 0)

    def answers(self, keys, nf=None, flags=None):
        """-> the mmp_vseam_row array the call must answer (dtype _lib.VSEAM_ROW's layout, built here from its field names)"""
        out = np.zeros(len(keys), np.dtype([("cls", "<i4"), ("which", "<i4"), ("vmodel", "<i4"), ("model", "<i4"), ("flags", "<u4"),
                                            ("reserved", "<i4")]))
        for i, k in enumerate(keys):
            out[i] = self.answer(k, None if nf is None else nf[i], 0 if flags is None else int(flags[i]))
        return out

    @staticmethod
    def decided_rows(ans):
        """The rule: the registry row request i is decided on — vm_out[i].model when the class is OK and the id is not null, else -1"""
        ok = (ans["cls"] == vm.OK) & ((ans["flags"] & vm.NULL_ID) == 0)
        rows = np.where(ok, ans["model"], -1).astype(np.int32)
        assert np.all(ans["model"][~ok] == -1)  # (and the answer itself names no model then)
        return rows

    def rows(self, keys, nf=None, flags=None):
        return self.decided_rows(self.answers(keys, nf, flags))
