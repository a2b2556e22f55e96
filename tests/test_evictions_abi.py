"""CPU: the eviction loop by id at the boundary — include/mmplace.h declares mmp_cache_replay_kt (the arguments of mmp_cache_replay_k
and one more), mmp_cache_evicted_times and mmp_evictions_k; mmp_cache_replay_k, mmp_cache_replay and mmp_cache_evicted_ids keep
their argument lists; the size and every field offset of the four new structs from a C99 program compiled against the header equal
modelmesh_amd/_lib.py's dtypes; the constants agree; libmmplace exports the calls and each refuses a NULL context."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from modelmesh_amd import _lib
from modelmesh_amd.solver import Solver
from tests.test_cache_keyed_abi import NEW as KEYED, OLD, header_params, header_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"mmp_evicted_entry": (_lib.EVICTED_ENTRY, 32), "mmp_evict_params": (_lib.EVICT_PARAMS, 24), "mmp_evicted_out": (_lib.EVICTED_OUT, 24),
           "mmp_evictions_info": (_lib.EVICTIONS_INFO, 112)}
EVICTIONS_K = ["ctx", "entries", "n", "keys", "key_off", "params", "flags", "model_idx_out", "outs", "status_out", "edits_out", "max_edits",
               "info_out"]


def test_replay_kt_is_replay_k_and_one_more_argument_and_the_three_calls_it_leaves_alone_are_what_they_were():
    k, kt = header_params("mmp_cache_replay_k"), header_params("mmp_cache_replay_kt")
    assert kt[:-1] == k and kt[-1] == ("int64_t *", "ev_last_used_out")
    assert [a for _, a in k] == KEYED["mmp_cache_replay_k"]
    assert [a for _, a in header_params("mmp_cache_evicted_ids")] == KEYED["mmp_cache_evicted_ids"]
    assert header_params("mmp_cache_replay") == OLD["mmp_cache_replay"]
    assert header_params("mmp_cache_evicted_times") == [("mmp_ctx *", "ctx"), ("int64_t *", "out"), ("int32_t", "max_slots"),
                                                         ("int32_t *", "n_slots_out")]
    p = header_params("mmp_evictions_k")
    assert [a for _, a in p] == EVICTIONS_K
    t = dict((a, t) for t, a in p)
    assert (t["entries"], t["params"], t["outs"], t["info_out"], t["flags"]) == \
        ("const mmp_evicted_entry *", "const mmp_evict_params *", "mmp_evicted_out *", "mmp_evictions_info *", "uint32_t")
    # behind mmp_registry_ops_k, whose path it ends in
    text = header_text()
    assert text.index("int mmp_registry_ops_k") < text.index("int mmp_evictions_k")
    assert text.index("int mmp_cache_evicted_ids") < text.index("int mmp_cache_replay_kt") < text.index("int mmp_cache_evicted_times")


def test_the_constants_agree_and_the_abi_is_still_3():
    text = header_text()
    assert re.search(r"#define\s+MMP_ABI_VERSION\s+3\b", text)
    for name, want in (("MMP_EVF_FAILED", _lib.EVF_FAILED), ("MMP_EVO_IN_REGISTRY", _lib.EVO_IN_REGISTRY),
                       ("MMP_EVO_ATTEMPT_RELOAD", _lib.EVO_ATTEMPT_RELOAD), ("MMP_EVO_RELOAD", _lib.EVO_RELOAD), ("MMP_EVO_LOG", _lib.EVO_LOG)):
        m = re.search(r"#define\s+" + name + r"\s+(\d+)u\b", text)
        assert m and int(m.group(1)) == want, name
    assert (_lib.EVO_IN_REGISTRY, _lib.EVO_ATTEMPT_RELOAD, _lib.EVO_RELOAD, _lib.EVO_LOG) == (1, 2, 4, 8)


def test_sizeof_and_every_offset_of_the_four_structs_from_a_c99_program(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no C compiler for the layout program")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "mmplace.h"', "int main(void) {"]
    for name, (dt, _) in STRUCTS.items():
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        lines += ['    printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (name, f, name, f, name, f) for f in dt.names]
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(ln.split(" ", 1) for ln in subprocess.check_output([str(exe)], text=True).strip().split("\n"))
    for name, (dt, size) in STRUCTS.items():
        assert int(out[name]) == size == dt.itemsize, name
        for f in dt.names:
            off, sz = (int(x) for x in out[f"{name}.{f}"].split())
            assert (off, sz) == (dt.fields[f][1], dt.fields[f][0].itemsize), (name, f)
    assert out["mmp_evictions_info.ops"] == "24 88" and _lib.EVICTIONS_INFO.fields["ops"][0] == _lib.REGISTRY_OPS_INFO_K


def test_lib_binds_the_three_calls_with_the_headers_argument_kinds():
    bound = {name: (ret, args) for name, ret, args in _lib.SYMBOLS}
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32}
    for name in ("mmp_cache_replay_kt", "mmp_cache_evicted_times", "mmp_evictions_k"):
        ret, args = bound[name]
        params = header_params(name)
        assert ret is C.c_int and len(args) == len(params), name
        for got, (t, a) in zip(args, params):
            assert got in ((kinds[t],) if "*" not in t else (C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64))), (name, a)
    assert bound["mmp_cache_replay_kt"][1][:-1] == bound["mmp_cache_replay_k"][1]
    for method in ("cache_replay_kt", "cache_evicted_times", "evictions_k", "evictions_k_raw"):
        assert callable(getattr(Solver, method))


def test_libmmplace_exports_them_and_each_refuses_a_null_context():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    assert lib.mmp_abi_version() == 3
    n = (C.c_int32 * 32)(*([-7] * 32))
    p = lambda i: C.cast(C.byref(n, 4 * i), C.POINTER(C.c_int32))  # noqa: E731
    assert lib.mmp_cache_replay_kt(None, None, 0, None, None, 1, None, None, None, None, 0, p(0), None, 0, None, p(1), None) == _lib.MMP_EINVAL
    assert lib.mmp_cache_evicted_times(None, None, 0, p(2)) == _lib.MMP_EINVAL
    params = (C.c_int64 * 3)(0, 1, 1)
    assert lib.mmp_evictions_k(None, None, 0, None, None, params, 0, None, None, None, None, 0, C.cast(n, C.c_void_p)) == _lib.MMP_EINVAL
    assert list(n) == [-7] * 32


def test_the_jni_veneer_and_the_java_side_carry_the_three_calls():
    java = open(os.path.join(ROOT, "integration", "GpuPlacementLB.java")).read()
    veneer = open(os.path.join(ROOT, "integration", "mmplace_jni.cc")).read()
    for native, call in (("cacheReplayKT", "mmp_cache_replay_kt"), ("cacheEvictedTimes", "mmp_cache_evicted_times"),
                         ("evictionsKeyed", "mmp_evictions_k")):
        assert re.search(r"static\s+native\s+int\s+" + native + r"\s*\(", java), native
        v = re.search(r"JNIEXPORT\s+jint\s+JNICALL\s+Java_com_ibm_watson_modelmesh_MmPlace_" + native + r"\s*\(([^)]*)\)\s*\{(.*?)\n\}", veneer,
                      flags=re.S)
        assert v and call + "(" in v.group(2), native
    assert "class EvictionsById" in java and "MmPlace.cacheReplayKT(" in java and "MmPlace.evictionsKeyed(" in java
