"""CPU: mmp_registry_ops_k at the boundary — include/mmplace.h declares it in the stated order and states its rule by key, the size
and every field offset of mmp_registry_ops_info_k come from a C99 program compiled against the header, libmmplace exports the
symbol and refuses a NULL context, modelmesh_amd/_lib.py carries the two new constants and binds the call with the header's
argument kinds, and mmp_registry_ops keeps its 56-byte info."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from modelmesh_amd import _lib
from modelmesh_amd.solver import Solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmplace.h")

ORDER = ["ctx", "ops", "n", "keys", "key_off", "now_ms", "flags", "model_idx_out", "status_out", "edits_out", "max_edits", "info_out"]
TYPES = {"ctx": "mmp_ctx *", "ops": "const mmp_registry_op *", "n": "int32_t", "keys": "const char *", "key_off": "const int32_t *",
         "now_ms": "int64_t", "flags": "uint32_t", "model_idx_out": "int32_t *", "status_out": "uint8_t *",
         "edits_out": "mmp_registry_op_edit *", "max_edits": "int32_t", "info_out": "mmp_registry_ops_info_k *"}
FIELDS = ["n_edits", "n_unchanged", "n_no_record", "truncated", "n_edited_op", "n_unchanged_op", "n_entries_added", "n_entries_removed"]


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


def test_the_header_declares_the_call_in_the_stated_order_and_states_the_rule():
    params = header_params("mmp_registry_ops_k")
    assert [a for _, a in params] == ORDER
    for t, a in params:
        assert t == TYPES[a], (a, t)
    text = open(HEADER).read()
    assert "THE RULE BY KEY: model_idx_out[i] is what mmp_model_ids_resolve answers for key i.  Op i is evaluated exactly as" in text
    assert "it refuses MMP_ROP_DROP_LOCAL (kind 4)" in text          # the old call says that it did not change
    assert re.search(r"#define\s+MMP_ABI_VERSION\s+3\b", text)
    assert [a for _, a in header_params("mmp_registry_ops")][-1] == "info_out"


def test_the_two_constants_agree_with_lib():
    text = header_text()
    for name, want in (("MMP_ROP_DROP_LOCAL", _lib.ROP_DROP_LOCAL), ("MMP_ROP_NO_RECORD", _lib.ROP_NO_RECORD)):
        m = re.search(r"#define\s+" + name + r"\s+(\d+)\b", text)
        assert m and int(m.group(1)) == want, name
    assert (_lib.ROP_DROP_LOCAL, _lib.ROP_NO_RECORD) == (4, 2)
    assert _lib.ROP_NO_RECORD not in (_lib.ROP_UNCHANGED, _lib.ROP_EDITED)
    assert _lib.ROP_DROP_LOCAL not in (_lib.ROP_REGISTER, _lib.ROP_LOAD_FAILED, _lib.ROP_DEREGISTER, _lib.ROP_SCALE_DOWN)


def test_sizeof_and_every_offset_of_the_info_struct_from_a_c99_program(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no C compiler for the layout program")
    src = tmp_path / "layout.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "mmplace.h"', "int main(void) {",
             '    printf("sizeof %zu\\n", sizeof(mmp_registry_ops_info_k));', '    printf("old %zu\\n", sizeof(mmp_registry_ops_info));']
    lines += ['    printf("%s %%zu %%zu\\n", offsetof(mmp_registry_ops_info_k, %s), sizeof(((mmp_registry_ops_info_k *)0)->%s));' % (f, f, f)
              for f in FIELDS]
    lines += ["    return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(ln.split(" ", 1) for ln in subprocess.check_output([str(exe)], text=True).strip().split("\n"))
    assert out["sizeof"] == "88" and out["old"] == "56"
    dt = _lib.REGISTRY_OPS_INFO_K
    assert dt.itemsize == 88 and list(dt.names) == FIELDS
    for f in FIELDS:
        off, size = (int(x) for x in out[f].split())
        assert (off, size) == (dt.fields[f][1], dt.fields[f][0].itemsize), f
    assert out["n_edited_op"] == "16 32" and out["n_unchanged_op"] == "48 32" and out["n_entries_removed"] == "84 4"
    assert _lib.REGISTRY_OPS_INFO.itemsize == 56


def test_lib_binds_it_with_the_headers_argument_kinds():
    bound = {name: (ret, args) for name, ret, args in _lib.SYMBOLS}
    assert "mmp_registry_ops_k" in bound
    ret, args = bound["mmp_registry_ops_k"]
    assert ret is C.c_int
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32}
    assert list(args) == [C.c_void_p if "*" in t else kinds[t] for t, _ in header_params("mmp_registry_ops_k")]
    for method in ("registry_ops_k", "registry_ops_k_raw"):
        assert callable(getattr(Solver, method))


def test_libmmplace_exports_it_and_refuses_a_null_context():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    assert lib.mmp_abi_version() == 3
    info = (C.c_int32 * 22)(*([-7] * 22))
    assert lib.mmp_registry_ops_k(None, None, 0, None, None, 1, 0, None, None, None, 0, info) == _lib.MMP_EINVAL
    assert list(info) == [-7] * 22


def test_the_jni_veneer_defines_the_native_java_declares_and_the_five_sites_use_it():
    java = open(os.path.join(ROOT, "integration", "GpuPlacementLB.java")).read()
    veneer = open(os.path.join(ROOT, "integration", "mmplace_jni.cc")).read()
    m = re.search(r"static\s+native\s+int\s+registryOpsKeyed\s*\(([^)]*)\)\s*;", java)
    assert m, "registryOpsKeyed is not declared in GpuPlacementLB.java"
    n_java = len(m.group(1).split(","))
    v = re.search(r"JNIEXPORT\s+jint\s+JNICALL\s+Java_com_ibm_watson_modelmesh_MmPlace_registryOpsKeyed\s*\(([^)]*)\)\s*\{(.*?)\n\}", veneer, flags=re.S)
    assert v, "registryOpsKeyed is not defined in mmplace_jni.cc"
    assert len(v.group(1).split(",")) == n_java + 2 and n_java == len(ORDER)  # JNIEnv *, jclass in front; one argument per C argument
    assert "mmp_registry_ops_k(" in v.group(2) and "mmp_registry_ops_info_k" in v.group(2)
    assert java.count("MmPlace.registryOpsKeyed(") == 1                         # one statement of the call, five sites through it
    for site in ("registered", "loadFailed", "deregistered", "scaledDown", "droppedLocal"):
        assert re.search(r"static\s+Edit\s+" + site + r"\s*\(", java), site
    assert re.search(r"DROP_LOCAL\s*=\s*4\b", java) and re.search(r"NO_RECORD\s*=\s*2\b", java)
