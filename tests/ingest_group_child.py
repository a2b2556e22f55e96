"""Run by tests/test_ingest_paths_gpu.py as a fresh process with MMP_JGROUP set (the library reads it once per process): ingests
the first 4 096 records of the planted ModelRecord and InstanceRecord batches of tests/ingest_corpus.py with that many records
per wavefront, compares every record with tests/ingest_model.py and exits non-zero on a difference.

usage: MMP_JGROUP=3 python -m tests.ingest_group_child"""
import os
import sys

from modelmesh_amd.solver import Solver
from tests import ingest_corpus as ic

N = 4096


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
