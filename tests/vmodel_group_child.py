"""Child of tests/test_vmodels_gpu.py::test_odd_group_sizes: MMP_JGROUP is read once per process, so a fresh process sends one
batch of 4 096 vmodel events with the group size of its environment and compares every output and the table with the model."""
import os
import sys

import numpy as np

from tests import test_vmodels_gpu as t
from tests import vmodel_model as vm


def main():
    grp = int(os.environ["MMP_JGROUP"])
    s, m = t.start(8), vm.VModels()
    try:
        keys, values, deleted = t.grouped_batch(4096, grp)
        want = m.events(keys, values, deleted)
        got = s.vmodels_events_json(keys, values, deleted)
        diffs = int((got[0] != want[0]).sum() + (got[1] != want[1]).sum()) + (got[2] != want[2])
        ids, flags, strings = s.vmodels_get()
        diffs += (ids != m.ids) + int((flags != m.flags()).sum()) + sum(a != b for a, b in zip(strings, m.strings()))
    finally:
        s.close()
    print("MMP_JGROUP=%d: 4096 vmodel events, %d differences" % (grp, diffs))
    return 1 if diffs else 0


if __name__ == "__main__":
    sys.exit(main())
