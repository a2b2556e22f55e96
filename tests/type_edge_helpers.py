"""Shared by tests/test_type_edges.py and tests/test_type_edges_gpu.py: the cases of tests/ref_type_edges.py beside the committed
vectors (tests/golden/ref_type_edges.npz), and the restatements' tables of a case in the form check_type_tables takes."""
import copy
import os

import numpy as np

from modelmesh_amd.solver import bitmap_from_bool
from oracle import bind as ob
from oracle import py_types
from tests import ref_fleets as rf
from tests import ref_type_edges as te
from tests.test_ref_vectors import STAT_FIELDS

GOLDEN_TYPE_EDGES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_type_edges.npz")
CASES = {c[0]: c for c in rf.type_edge_cases()}
NAMES = list(CASES)


def tier_names(tier):
    return [n for n in NAMES if CASES[n][6]["tier"] == tier]


def load():
    return np.load(GOLDEN_TYPE_EDGES)


def labels_of(bits):
    return [i for i in range(64) if (int(bits) >> i) & 1]


def py_tables(fleet, pod_bits, req_bits, pref_bits):
    """oracle/py_types.py on a case -> tables(t) for t in 0..T as check_type_tables takes them"""
    P, T = fleet.n_pods, len(req_bits)
    present = {p: set(labels_of(pod_bits[p])) for p in range(P) if not (fleet.pods["flags"][p] & 5)}
    cfg = {t: (labels_of(req_bits[t]), labels_of(pref_bits[t])) for t in range(T)}
    want, want_default = py_types.type_tables(present, cfg)

    def tables(t):
        if t == T:
            return None, None if want_default is None else set(want_default)
        return None if want[t][0] is None else set(want[t][0]), None if want[t][1] is None else set(want[t][1])
    return tables


def with_tables(fleet, T, tables):
    """a copy of the fleet with the T + 1 rows of tables(t) installed -> (fleet, allowed, prefer, has_allowed, has_prefer)"""
    P = fleet.n_pods
    al, pf = np.zeros((T + 1, P), bool), np.zeros((T + 1, P), bool)
    ha, hp = np.zeros(T + 1, np.uint8), np.zeros(T + 1, np.uint8)
    for t in range(T + 1):
        a, b = tables(t)
        ha[t], hp[t] = a is not None, b is not None
        al[t, sorted(a or [])] = True
        pf[t, sorted(b or [])] = True
    f = copy.copy(fleet)
    f.n_types, f.allowed, f.prefer, f.has_allowed, f.has_prefer = T + 1, bitmap_from_bool(al), bitmap_from_bool(pf), ha, hp
    return f


def ref_tables(ref, name, P):
    """the reference's own rows of a case as tables(t)"""
    rows = ref[f"{name}/rows"]
    W = (P + 63) // 64
    return lambda t: (te.set_of(rows[t], W, 0), te.set_of(rows[t], W, 1))


def oracle_partitions(f):
    """oracle.bind's partitions and stats of a fleet with tables -> (partitions, type_stats) as check_type_tables takes them"""
    pts, sets, pst = ob.partition_stats(f)
    parts = [(tuple(int(pst[k][x]) for x in STAT_FIELDS), frozenset(int(t) for t in sets[k])) for k in range(len(sets))]
    tss = ob.type_set_stats(f)
    g = ob.OracleFleet(f).stats()
    return (pts, parts), lambda t: tuple(int((g if t is None else tss[t])[x]) for x in STAT_FIELDS)
