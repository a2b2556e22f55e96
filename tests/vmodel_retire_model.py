"""mmp_vmodels_retire as a plain sequential program over a VModels (tests/vmodel_model.py): the named rows are deleted from the
lists, the dict is rebuilt, the remap is returned.  The oracle of the device path (tests/test_vmodels_retire_gpu.py).

  rows         vmodel rows in [0, V0) in any order; a row named twice is retired once
  remap        int32[V0]: the new row of every old row, -1 for a retired one; survivors keep their order and move down
  absent_only  every named row must be ABSENT (None: never set, or deleted)
  all_absent   no list: every ABSENT row leaves; absent_only beside it adds nothing
  refusals     ValueError (MMP_EINVAL) with nothing changed: a row outside [0, V0), a row that is set under absent_only — the
               message names the lowest one —, a list beside all_absent
"""
import numpy as np


def retire(m, rows=None, absent_only=False, all_absent=False):
    v0 = len(m.rows)
    rows = [] if rows is None else [int(r) for r in rows]
    if all_absent and rows:
        raise ValueError("a list of %d rows beside all_absent" % len(rows))
    for r in rows:
        if r < 0 or r >= v0:
            raise ValueError("row %d of %d" % (r, v0))
    gone = {r for r in range(v0) if m.rows[r] is None} if all_absent else set(rows)
    if absent_only:
        live = sorted(r for r in gone if m.rows[r] is not None)
        if live:
            raise ValueError("row %d is not ABSENT" % live[0])
    keep = [r for r in range(v0) if r not in gone]
    remap = np.full(v0, -1, np.int32)
    remap[keep] = np.arange(len(keep), dtype=np.int32)
    m.ids[:] = [m.ids[r] for r in keep]
    m.rows[:] = [m.rows[r] for r in keep]
    m.row_of.clear()
    m.row_of.update((b, i) for i, b in enumerate(m.ids))
    return remap, len(keep)


def through(remap, answers):
    """Answers or transitions (namedtuples with a `vmodel` field) asked BEFORE a retire as the host renumbers them: the vmodel
    number through remap; a transition of a retired row leaves the list, an answer about one is NOT_FOUND afterwards and is not
    the host's to renumber (returned as None)."""
    out = []
    for a in answers:
        if a.vmodel < 0:
            out.append(a)
        elif remap[a.vmodel] >= 0:
            out.append(a._replace(vmodel=int(remap[a.vmodel])))
        else:
            out.append(None)
    return out
