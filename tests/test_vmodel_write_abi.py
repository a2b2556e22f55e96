"""CPU: the boundary of the write side of the vmodel transactions — the declarations of mmp_models_refs_json and
mmp_vmodels_write_json in include/mmplace.h (argument lists, position behind mmp_vmodels_retire), every new constant against
modelmesh_amd/_lib.py and the models, the sizes (16 / 8 / 48 bytes) and field offsets of the three structs from a C99 program
compiled against the header, the exported and bound symbols, the refusal of a NULL context, the veneer and the Java declarations."""
import ctypes as C
import os
import re
import subprocess

from modelmesh_amd import _lib
from tests import model_refs_model as mr
from tests import vmodel_write_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"mmp_refs_req": _lib.REFS_REQ, "mmp_vmodel_write_req": _lib.VMODEL_WRITE_REQ, "mmp_vmodel_write_row": _lib.VMODEL_WRITE_ROW}
REFS_ARGS = ["mmp_ctx *ctx", "const mmp_refs_req *reqs", "int32_t n", "const char *info", "const int32_t *info_off", "const char *old_buf",
             "const int64_t *old_off", "uint32_t flags", "char *out_buf", "int64_t out_cap", "int64_t *out_off", "int32_t *class_out",
             "int32_t *refs_out", "int64_t *n_bytes_out"]
WRITE_ARGS = ["mmp_ctx *ctx", "const mmp_vmodel_write_req *reqs", "int32_t n", "const char *strs", "const int32_t *str_off",
              "const char *default_owner", "int32_t default_owner_len", "const char *old_buf", "const int64_t *old_off", "int64_t now_ms",
              "int64_t lastused_age_on_add_ms", "uint32_t flags", "char *out_buf", "int64_t out_cap", "int64_t *out_off",
              "mmp_vmodel_write_row *rows_out", "int64_t *n_bytes_out"]


def header():
    return open(os.path.join(ROOT, "include", "mmplace.h")).read()


def declaration(name):
    m = re.search(r"^int " + name + r"\(([^;]*)\);", header(), flags=re.M)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")], m.start()


def test_the_declarations():
    bound = {name: a for name, _, a in _lib.SYMBOLS}
    for name, want in (("mmp_models_refs_json", REFS_ARGS), ("mmp_vmodels_write_json", WRITE_ARGS)):
        args, at = declaration(name)
        assert args == want, name
        assert at > declaration("mmp_vmodels_retire")[1], name
        assert len(bound[name]) == len(want), name


def test_constants_agree_with_the_header_the_binding_and_the_model():
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+MMP_(MREFC?_\w+)\s+(\d+)u?\b", header(), flags=re.M)}
    assert len(defs) == 9
    for name, v in defs.items():
        assert getattr(_lib, name) == v, name
    pairs = {"MREF_INC": "INC", "MREF_AUTO_DELETE": "AUTO_DELETE", "MREFC_SET": "SET", "MREFC_CREATED": "CREATED", "MREFC_DELETE": "DELETE",
             "MREFC_ENSURE_ABSENT": "ENSURE_ABSENT", "MREFC_NOT_FOUND": "NOT_FOUND", "MREFC_MALFORMED": "MALFORMED", "MREFC_HOST": "HOST"}
    assert set(pairs) == set(defs)
    for lib_name, model_name in pairs.items():
        assert defs[lib_name] == getattr(mr, model_name), lib_name
    assert sorted(defs[k] for k in defs if k.startswith("MREFC_")) == list(mr.CLASSES)


def test_the_vmodel_write_constants_agree_with_the_header_the_binding_and_the_model():
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+MMP_(VW[QCF]?_\w+)\s+(\d+)u?\b", header(), flags=re.M)}
    assert len(defs) == 4 + 7 + 12 + 3
    for name, v in defs.items():
        assert getattr(_lib, name) == v, name
    pairs = {"VW_SET": "SET", "VW_DELETE": "DELETE", "VW_COMPLETE": "COMPLETE", "VW_FAIL_FLAG": "FAIL_FLAG", "VWQ_UPDATE_ONLY": "UPDATE_ONLY",
             "VWQ_FORCE": "FORCE", "VWQ_LOAD_NOW": "LOAD_NOW", "VWQ_TARGET_EXISTS": "TARGET_EXISTS", "VWQ_TARGET_LOADED": "TARGET_LOADED",
             "VWQ_TARGET_NOT_LOADED": "TARGET_NOT_LOADED", "VWQ_FAILED": "FAILED", "VWC_CREATED": "CREATED", "VWC_UPDATED": "UPDATED",
             "VWC_UNCHANGED": "UNCHANGED", "VWC_NOT_FOUND": "NOT_FOUND", "VWC_PRECONDITION": "PRECONDITION",
             "VWC_OWNER_MISMATCH": "OWNER_MISMATCH", "VWC_NEEDS_TARGET_STATUS": "NEEDS_TARGET_STATUS", "VWC_NOOP": "NOOP",
             "VWC_DELETE": "DELETED", "VWC_CHANGED": "CHANGED", "VWC_MALFORMED": "MALFORMED", "VWC_HOST": "HOST",
             "VWF_IN_TRANSITION": "IN_TRANSITION", "VWF_ACTIVE_SWITCHED": "ACTIVE_SWITCHED", "VWF_PREV_ACTIVE_UNKNOWN": "PREV_ACTIVE_UNKNOWN"}
    assert set(pairs) == set(defs)
    for lib_name, model_name in pairs.items():
        assert defs[lib_name] == getattr(wm, model_name), lib_name
    assert sorted(v for k, v in defs.items() if k.startswith("VWC_")) == list(wm.CLASSES)
    assert wm.Row._fields == _lib.VMODEL_WRITE_ROW.names
    # none of the new constants stands in the MMP_VM namespace, whose defines an existing test counts
    assert not re.search(r"^#define\s+MMP_VM\w*(WRITE|VW)", header(), flags=re.M)


def test_the_struct_has_the_headers_layout(tmp_path):
    assert [dt.itemsize for dt in STRUCTS.values()] == [16, 8, 48]
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "mmplace.h"', "int main(void) {"]
    for struct, dt in STRUCTS.items():
        lines.append(f'    printf("{struct} sizeof %lu\\n", (unsigned long)sizeof({struct}));')
        for f in dt.names:
            lines.append(f'    printf("{struct} {f} %lu\\n", (unsigned long)offsetof({struct}, {f}));')
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "offsets.c", tmp_path / "offsets"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {(s, f): int(v) for s, f, v in (ln.split() for ln in out.splitlines())}
    for struct, dt in STRUCTS.items():
        assert got[(struct, "sizeof")] == dt.itemsize, struct
        assert sum(dt.fields[f][0].itemsize for f in dt.names) == dt.itemsize, struct  # the fields tile the struct without gaps
        for f in dt.names:
            assert got[(struct, f)] == dt.fields[f][1], (struct, f)


def _lib_loaded():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_the_calls_are_exported_and_bound():
    _lib_loaded()
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "mmp_models_refs_json") and hasattr(lib, "mmp_vmodels_write_json")


def test_a_null_context_is_refused():
    lib = _lib_loaded()
    total, off = C.c_int64(-1), (C.c_int64 * 1)(-1)
    assert lib.mmp_models_refs_json(None, None, 0, None, None, None, None, 0, None, 0, off, None, None, C.byref(total)) == _lib.MMP_EINVAL
    assert total.value == -1 and off[0] == -1
    assert lib.mmp_vmodels_write_json(None, None, 0, None, None, None, 0, None, None, 1, 0, 0, None, 0, off, None,
                                      C.byref(total)) == _lib.MMP_EINVAL
    assert total.value == -1 and off[0] == -1


def test_the_veneer_and_the_java_declarations_exist():
    veneer = open(os.path.join(ROOT, "integration", "mmplace_jni.cc")).read()
    java = open(os.path.join(ROOT, "integration", "GpuPlacementLB.java")).read()
    for name in ("modelsRefsJson", "vmodelsWriteJson"):
        assert "Java_com_ibm_watson_modelmesh_MmPlace_" + name in veneer, name
        assert "static native int %s(" % name in java, name
