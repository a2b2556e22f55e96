"""CPU: mmp_vmodels_retire is declared in include/mmplace.h with seven arguments, exported by libmmplace and bound with as many,
and its two flags have the header's values in modelmesh_amd/_lib.py.  (The two defines stand in a value column of their own:
tests/test_vmodel_abi.py counts the vmodel constants that are written with a single blank, the 28 of the table's first commit,
and stays as it is; this file reads the two new ones.)"""
import ctypes as C
import os
import re

import numpy as np

from modelmesh_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "mmplace.h")).read()


def test_the_flags_equal_the_headers():
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+MMP_(VMRETIRE_\w+)\s+(\d+)u?\b", header(), flags=re.M)}
    assert defs == {"VMRETIRE_ABSENT_ONLY": 1, "VMRETIRE_ALL_ABSENT": 2}
    for name, v in defs.items():
        assert getattr(_lib, name) == v, name


def test_the_declaration_has_seven_arguments_and_follows_mmp_vmodels_info():
    hdr = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"\bint\s+mmp_vmodels_retire\s*\(([^)]*)\)\s*;", hdr)
    assert m, "mmp_vmodels_retire is not declared"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["mmp_ctx *ctx", "const int32_t *rows", "int32_t n", "uint32_t flags", "int32_t *remap_out", "int32_t max_vmodels",
                      "int32_t *n_vmodels_after_out"]
    assert hdr.index("mmp_vmodels_info(") < m.start() < hdr.index("mmp_pods_get(")


def test_the_call_is_exported_bound_and_refuses_a_null_context():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = _lib.load()
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "mmp_vmodels_retire")
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    assert len(bound["mmp_vmodels_retire"]) == 7
    n = C.c_int32(7)
    rows = np.zeros(1, np.int32)
    assert L.mmp_vmodels_retire(None, _lib.ptr(rows), 1, 0, None, 0, C.byref(n)) == _lib.MMP_EINVAL
    assert L.mmp_vmodels_retire(None, None, 0, _lib.VMRETIRE_ALL_ABSENT, None, 0, None) == _lib.MMP_EINVAL
    assert n.value == 7


def test_the_veneer_and_the_java_declaration_exist():
    assert "Java_com_ibm_watson_modelmesh_MmPlace_vmodelsRetire" in open(os.path.join(ROOT, "integration", "mmplace_jni.cc")).read()
    assert "static native int vmodelsRetire(" in open(os.path.join(ROOT, "integration", "GpuPlacementLB.java")).read()
