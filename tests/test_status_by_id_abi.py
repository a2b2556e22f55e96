"""CPU: the two status calls by id at the boundary — include/mmplace.h declares mmp_models_status_k and mmp_vmodels_status in the
stated order, modelmesh_amd/_lib.py binds them with the header's argument kinds and struct sizes, libmmplace exports them and
refuses a NULL context, the ABI version stays 3, and the JNI veneer defines the natives integration/GpuPlacementLB.java declares."""
import ctypes as C
import os
import re

from modelmesh_amd import _lib
from modelmesh_amd.solver import Solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmplace.h")

ORDER = {
    "mmp_models_status_k": ["ctx", "keys", "key_off", "n", "fail_pod", "flags", "now_ms", "model_idx_out", "rows_out", "copies_out",
                            "max_copies", "n_copies_out"],
    "mmp_vmodels_status": ["ctx", "keys", "key_off", "n", "owners", "owner_off", "req_flags", "now_ms", "vrows_out", "rows_out",
                           "copies_out", "max_copies", "n_copies_out", "str_bytes_out", "max_str_bytes", "str_off_out", "n_str_bytes_out"],
}
TYPES = {"keys": "const char *", "key_off": "const int32_t *", "owners": "const char *", "owner_off": "const int32_t *",
         "fail_pod": "const int32_t *", "flags": "const uint32_t *", "req_flags": "const uint32_t *", "n": "int32_t", "now_ms": "int64_t",
         "model_idx_out": "int32_t *", "vrows_out": "mmp_vstatus_row *", "rows_out": "mmp_status_row *", "copies_out": "mmp_status_copy *",
         "max_copies": "int32_t", "n_copies_out": "int32_t *", "str_bytes_out": "char *", "max_str_bytes": "int32_t",
         "str_off_out": "int32_t *", "n_str_bytes_out": "int32_t *", "ctx": "mmp_ctx *"}
NATIVES = {"modelsStatusKeyed": "mmp_models_status_k", "vmodelsStatus": "mmp_vmodels_status"}


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def header_params(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header_text())
    assert m, name + " is not declared in include/mmplace.h"
    out = []
    for p in m.group(1).split(","):
        pm = re.match(r"^(.*?)(\w+)$", " ".join(p.split()))
        out.append((pm.group(1).strip(), pm.group(2)))
    return out


def ctype_of(type_text, name):
    if "*" in type_text:
        return C.POINTER(C.c_int32) if name in ("n_copies_out", "n_str_bytes_out") else C.c_void_p
    return {"int32_t": C.c_int32, "int64_t": C.c_int64}[type_text]


def test_the_header_declares_both_calls_in_the_stated_order():
    for name, order in ORDER.items():
        params = header_params(name)
        assert [a for _, a in params] == order, name
        for t, a in params:
            assert t == TYPES[a], (name, a, t)
    text = open(HEADER).read()
    assert "THE RULE BY KEY: model_idx_out[i] is what mmp_model_ids_resolve answers" in text and "MMP_VMR_STRONG_READ when a.cls" in text
    assert re.search(r"#define\s+MMP_ABI_VERSION\s+3\b", text)


def test_sizeof_mmp_vstatus_row_is_32_and_lib_agrees_field_by_field():
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*mmp_vstatus_row\s*;", header_text())
    assert m, "mmp_vstatus_row is not declared"
    fields = []
    for decl in m.group(1).split(";"):
        decl = " ".join(decl.split())
        if decl:
            t, names = decl.split(" ", 1)
            fields += [(x.strip(), {"int32_t": "<i4", "uint32_t": "<u4"}[t]) for x in names.split(",")]
    assert fields == [(n, _lib.VSTATUS_ROW.fields[n][0].str) for n in _lib.VSTATUS_ROW.names]
    assert _lib.VSTATUS_ROW.itemsize == 32 and _lib.STATUS_ROW.itemsize == 16 and _lib.STATUS_COPY.itemsize == 16
    assert _lib.VMF_REPLY == 1 | 4 | 8 | 16


def test_lib_binds_them_with_the_headers_argument_kinds():
    bound = {name: (ret, args) for name, ret, args in _lib.SYMBOLS}
    for name in ORDER:
        assert name in bound, name + " is not bound in modelmesh_amd/_lib.py"
        ret, args = bound[name]
        assert ret is C.c_int
        assert list(args) == [ctype_of(t, a) for t, a in header_params(name)], name
    for method in ("models_status_k", "models_status_k_raw", "vmodels_status", "vmodels_status_raw"):
        assert callable(getattr(Solver, method))


def test_libmmplace_exports_them_and_refuses_a_null_context():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    assert lib.mmp_abi_version() == 3
    total, nstr = C.c_int32(-7), C.c_int32(-7)
    assert lib.mmp_models_status_k(None, None, None, 0, None, None, 1, None, None, None, 0, C.byref(total)) == _lib.MMP_EINVAL
    assert lib.mmp_vmodels_status(None, None, None, 0, None, None, None, 1, None, None, None, 0, C.byref(total), None, 0, None,
                                  C.byref(nstr)) == _lib.MMP_EINVAL
    assert (total.value, nstr.value) == (-7, -7)


def test_the_jni_veneer_names_the_natives_java_declares():
    java = open(os.path.join(ROOT, "integration", "GpuPlacementLB.java")).read()
    veneer = open(os.path.join(ROOT, "integration", "mmplace_jni.cc")).read()
    for native, call in NATIVES.items():
        m = re.search(r"static\s+native\s+int\s+" + native + r"\s*\(([^)]*)\)\s*;", java)
        assert m, native + " is not declared in GpuPlacementLB.java"
        n_java = len(m.group(1).split(","))
        v = re.search(r"JNIEXPORT\s+jint\s+JNICALL\s+Java_com_ibm_watson_modelmesh_MmPlace_" + native + r"\s*\(([^)]*)\)\s*\{(.*?)\n\}", veneer,
                      flags=re.S)
        assert v, native + " is not defined in mmplace_jni.cc"
        assert len(v.group(1).split(",")) == n_java + 2  # JNIEnv *, jclass in front
        assert call + "(" in v.group(2)
        assert n_java == len(ORDER[call])  # one Java argument per C argument (long h: the context)
    assert "MmPlace.modelsStatusKeyed(" in java and "MmPlace.vmodelsStatus(" in java
