"""mmp_models_retire as a plain sequential program over a ModelEventsModel (tests/model_events_model.py): the named rows are
deleted from the lists, the dict is rebuilt, the remap is returned.  The oracle of the device path (tests/test_models_retire_gpu.py).

  rows         registry rows in [0, M0) in any order; a row named twice is retired once
  remap        int32[M0]: the new row of every old row, -1 for a retired one; survivors keep their order and move down
  empty_only   every named row must be EMPTY — (0, 0, (), ()), what a deletion leaves; a record without copies but with a type or a
               last_used is not
  refusals     ValueError (MMP_EINVAL) with nothing changed: a row outside [0, M0), a non-empty row under empty_only — the message
               names the lowest one.  RuntimeError (MMP_ESTATE): ids are loaded and their count is not the registry's
"""
import numpy as np

from tests.model_events_model import EMPTY


def retire(model, rows, empty_only=False):
    m0 = len(model.recs)
    if model.ids is not None and len(model.ids) != m0:
        raise RuntimeError("%d ids for %d rows" % (len(model.ids), m0))
    rows = [int(r) for r in rows]
    for r in rows:
        if r < 0 or r >= m0:
            raise ValueError("row %d of %d" % (r, m0))
    gone = set(rows)
    if empty_only:
        full = sorted(r for r in gone if tuple(model.recs[r]) != EMPTY)
        if full:
            raise ValueError("row %d is not empty" % full[0])
    remap = np.full(m0, -1, np.int32)
    keep = [r for r in range(m0) if r not in gone]
    remap[keep] = np.arange(len(keep), dtype=np.int32)
    model.recs = [model.recs[r] for r in keep]
    if model.ids is not None:
        model.ids = [model.ids[r] for r in keep]
        model.index = {s: i for i, s in enumerate(model.ids)}
    return remap
