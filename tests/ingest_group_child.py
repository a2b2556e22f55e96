"""Run by tests/test_ingest_paths_gpu.py as a fresh process with MMP_JGROUP set (the library reads it once per process): ingests
the first 4 096 records of the planted ModelRecord and InstanceRecord batches of tests/ingest_corpus.py with that many records
per wavefront, compares every record with tests/ingest_model.py and exits non-zero on a difference.  The same ModelRecord values
then go as registry events (upsert_models_json, event i appends row i) onto a second, empty context and must leave the status,
lul and registry of the reload: NLCLASSIFIER is type 0, so a rejected append and a rejected reload row are the same empty row.

usage: MMP_JGROUP=3 python -m tests.ingest_group_child"""
import os
import sys

import numpy as np

from modelmesh_amd.solver import Solver
from tests import ingest_corpus as ic
from tests import registry_prune_model as rp

N = 4096


def events_like_reload(vals, status, lul, registry):
    """The differences between the reload's answers and those of the same values sent as events onto an empty registry."""
    e = Solver(100, 1000)
    try:
        e.load_pod_ids(ic.IDS)
        e.load_type_names(ic.TYPE_NAMES, ic.UNKNOWN_TYPE)
        ev_status, ev_lul = e.upsert_models_json(vals, np.arange(len(vals), dtype=np.int32))
        ev_registry = rp.compact(*e.get_models())
    finally:
        e.close()
    diffs = ["event %d: status %d, the reload's %d" % (i, ev_status[i], status[i]) for i in np.flatnonzero(ev_status != status)]
    diffs += ["event %d: lul %d, the reload's %d" % (i, ev_lul[i], lul[i]) for i in np.flatnonzero(ev_lul != lul)]
    for name, a, b in zip(("rows", "ent_pod", "ent_time"), ev_registry, registry):
        if not np.array_equal(a, b):
            diffs.append("events: the compacted %s differ from the reload's" % name)
    return diffs


def main():
    grp = os.environ.get("MMP_JGROUP")
    if grp is None:
        print("MMP_JGROUP is not set")
        return 2
    s = Solver(100, 1000)
    try:
        s.load_pod_ids(ic.IDS)
        s.load_type_names(ic.TYPE_NAMES, ic.UNKNOWN_TYPE)
        vals = ic.planted_models(N)
        status, lul = s.ingest_models_json(vals)
        diffs = ic.check_models(vals, status, lul, *s.get_models())
        diffs += events_like_reload(vals, status, lul, rp.compact(*s.get_models()))
        s.load_pod_ids(["p%d" % i for i in range(N)])
        before = s.get_pods()
        vals = ic.planted_pods(N)
        status, start = s.ingest_pods_json(vals, range(N))
        diffs += ic.check_pods(vals, status, start, s.get_pods(), before)
    finally:
        s.close()
    print("MMP_JGROUP=%s: %d records of each kind, %d differences" % (grp, N, len(diffs)))
    for d in diffs:
        print(d)
    return 1 if diffs else 0


if __name__ == "__main__":
    sys.exit(main())
