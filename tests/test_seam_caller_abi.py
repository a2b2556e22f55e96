"""CPU: the numpy mirrors of mmp_seam_caller / mmp_gate_req_c / mmp_serve_req_c have the header's layout — sizes and every
field offset, the latter from a C99 program compiled against include/mmplace.h — and libmmplace exports both calls."""
import ctypes as C
import os
import subprocess

from modelmesh_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"mmp_seam_caller": _lib.SEAM_CALLER, "mmp_gate_req_c": _lib.GATE_REQ_C, "mmp_serve_req_c": _lib.SERVE_REQ_C}


def test_sizes():
    assert _lib.SEAM_CALLER.itemsize == 112 and _lib.GATE_REQ_C.itemsize == 48 and _lib.SERVE_REQ_C.itemsize == 24


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
        # (a field the mirror lacks would leave a hole: the fields tile the struct without gaps)
        assert sum(dt.fields[f][0].itemsize for f in dt.names) == dt.itemsize, struct
        for f in dt.names:
            assert got[(struct, f)] == dt.fields[f][1], (struct, f, got[(struct, f)], dt.fields[f][1])
            n += 1
    assert n == 19 + 10 + 5


def test_both_calls_are_exported_and_bound():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    _lib.load()
    lib = C.CDLL(_lib.LIB_PATH)
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    for name, n_args in (("mmp_route_batch_c", 16), ("mmp_miss_batch_c", 17)):
        assert hasattr(lib, name), name
        assert len(bound[name]) == n_args, name
