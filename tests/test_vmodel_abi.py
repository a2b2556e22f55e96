"""CPU: the numpy mirrors of the vmodel structs have the header's layout — sizes and every field offset, from a C99 program
compiled against include/mmplace.h — the constants agree with tests/vmodel_model.py, and libmmplace exports the five calls."""
import ctypes as C
import os
import re
import subprocess

from modelmesh_amd import _lib
from tests import vmodel_model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"mmp_vmodel_answer": _lib.VMODEL_ANSWER, "mmp_vmodel_transition": _lib.VMODEL_TRANSITION,
           "mmp_vmodel_transitions_info": _lib.VMODEL_TRANSITIONS_INFO, "mmp_vmodels_stats": _lib.VMODELS_STATS}


def test_sizes():
    assert [dt.itemsize for dt in STRUCTS.values()] == [32, 32, 24, 32]


def test_every_field_offset_equals_offsetof_in_c99(tmp_path):
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
    n = 0
    for struct, dt in STRUCTS.items():
        assert got[(struct, "sizeof")] == dt.itemsize, struct
        assert sum(dt.fields[f][0].itemsize for f in dt.names) == dt.itemsize, struct  # the fields tile the struct without gaps
        for f in dt.names:
            assert got[(struct, f)] == dt.fields[f][1], (struct, f)
            n += 1
    assert n == 8 + 7 + 6 + 6


def test_constants_agree_with_the_header_and_the_model():
    hdr = open(os.path.join(ROOT, "include", "mmplace.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define MMP_(VM\w+) (\d+)u?\b", hdr, flags=re.M)}
    assert len(defs) == 28
    for name, v in defs.items():
        assert getattr(_lib, name) == v, name
    pairs = {"VMF_FAILED": "F_FAILED", "VMF_ABSENT": "F_ABSENT", "VMF_ACTIVE_NULL": "F_ACTIVE_NULL", "VMF_TARGET_NULL": "F_TARGET_NULL",
             "VMF_OWNER_NULL": "F_OWNER_NULL", "VMF_HOST": "F_HOST", "VMR_NOT_FOUND": "NOT_FOUND", "VMR_OK": "OK",
             "VMR_STRONG_READ": "STRONG_READ", "VMR_TARGET_NOT_FOUND": "TARGET_NOT_FOUND", "VMR_HOST": "HOST", "VMW_ACTIVE": "ACTIVE",
             "VMW_TARGET": "TARGET", "VMRF_NULL_ID": "NULL_ID", "VMS_DEFINED": "DEFINED", "VMS_TRANSITIONING": "TRANSITIONING",
             "VMS_TRANSITION_FAILED": "TRANSITION_FAILED", "VMT_NONE": "T_NONE", "VMT_LOADING": "T_LOADING",
             "VMT_LOADING_FAILED": "T_LOADING_FAILED", "VMT_NOT_FOUND": "T_NOT_FOUND", "VMX_PROMOTE": "PROMOTE",
             "VMX_ENSURE_LOADED": "ENSURE_LOADED", "VMXF_FAILED": "XF_FAILED", "VMXF_FROM_EMPTY": "XF_FROM_EMPTY",
             "VMXF_TO_EMPTY": "XF_TO_EMPTY"}
    for lib_name, model_name in pairs.items():
        assert defs[lib_name] == getattr(vm, model_name), lib_name
    assert vm.Answer._fields == _lib.VMODEL_ANSWER.names and vm.Transition._fields == _lib.VMODEL_TRANSITION.names


def test_the_calls_are_exported_and_bound():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    _lib.load()
    lib = C.CDLL(_lib.LIB_PATH)
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    for name, n_args in (("mmp_vmodels_events_json", 11), ("mmp_vmodels_resolve", 10), ("mmp_vmodels_transitions", 7),
                         ("mmp_vmodels_get", 12), ("mmp_vmodels_info", 2)):
        assert hasattr(lib, name), name
        assert len(bound[name]) == n_args, name
