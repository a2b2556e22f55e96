"""CPU: the request seams by model id at the boundary — include/mmplace.h declares the three calls (keys / key_off behind n,
model_idx_out last, everything else in the _c forms' order), modelmesh_amd/_lib.py binds them with the header's argument kinds in
the header's order, Solver packs keys as model_ids_resolve packs them, and the JNI veneer defines the three natives
integration/GpuPlacementLB.java declares."""
import ctypes as C
import os
import re

import numpy as np

from modelmesh_amd import _lib
from modelmesh_amd.solver import Solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmplace.h")

# the argument names of the header, in order
ORDER = {
    "mmp_place_batch_ck": ["ctx", "caller", "reqs", "n", "keys", "key_off", "extra_pool", "n_extra", "now_ms", "outs", "model_idx_out"],
    "mmp_route_batch_ck": ["ctx", "caller", "gate_reqs", "serve_reqs", "n", "keys", "key_off", "counters", "n_counters", "excl_pod",
                           "excl_time", "n_excl", "explicit_pool", "n_explicit", "now_ms", "in_use_expiry_ms", "gate_outs", "serve_outs",
                           "model_idx_out"],
    "mmp_miss_batch_ck": ["ctx", "caller", "place_caller", "gate_reqs", "place_reqs", "n", "keys", "key_off", "excl_pod", "excl_time",
                          "n_excl", "explicit_pool", "n_explicit", "extra_pool", "n_extra", "now_ms", "in_use_expiry_ms", "gate_outs",
                          "place_outs", "model_idx_out"],
}
# ... and the struct each row array is declared with
ROWS = {
    "mmp_place_batch_ck": {"caller": "mmp_place_caller", "reqs": "mmp_place_req_c", "outs": "mmp_place_out"},
    "mmp_route_batch_ck": {"caller": "mmp_seam_caller", "gate_reqs": "mmp_gate_req_c", "serve_reqs": "mmp_serve_req_c",
                           "gate_outs": "mmp_gate_out", "serve_outs": "mmp_serve_out"},
    "mmp_miss_batch_ck": {"caller": "mmp_seam_caller", "place_caller": "mmp_place_caller", "gate_reqs": "mmp_gate_req_c",
                          "place_reqs": "mmp_place_req_c", "gate_outs": "mmp_gate_out", "place_outs": "mmp_place_out"},
}


def header_params(name):
    """[(type text, argument name)] of the header's declaration"""
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, name + " is not declared in include/mmplace.h"
    out = []
    for p in m.group(1).split(","):
        p = " ".join(p.split())
        pm = re.match(r"^(.*?)(\w+)$", p)
        out.append((pm.group(1).strip(), pm.group(2)))
    return out


def ctype_of(type_text):
    if "*" in type_text:
        return C.c_void_p
    return {"int32_t": C.c_int32, "int64_t": C.c_int64}[type_text]


def test_the_header_declares_the_three_calls_in_the_stated_order():
    for name, order in ORDER.items():
        params = header_params(name)
        assert [p[1] for p in params] == order, name
        for arg, struct in ROWS[name].items():
            t = dict((a, t) for t, a in params)[arg]
            assert struct in t and "*" in t, (name, arg, t)
            assert ("const" in t) == (not arg.endswith("outs")), (name, arg, t)
        types = dict((a, t) for t, a in params)
        assert types["keys"] == "const char *" and types["key_off"] == "const int32_t *" and types["model_idx_out"] == "int32_t *"
        assert types["n"] == "int32_t" and types["now_ms"] == "int64_t"
    assert "THE RULE BY KEY" in open(HEADER).read()


def test_lib_binds_them_with_the_headers_argument_kinds():
    bound = {name: (ret, args) for name, ret, args in _lib.SYMBOLS}
    for name in ORDER:
        assert name in bound, name + " is not bound in modelmesh_amd/_lib.py"
        ret, args = bound[name]
        assert ret is C.c_int
        assert list(args) == [ctype_of(t) for t, _ in header_params(name)], name


def test_libmmplace_exports_them():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ORDER:
        assert hasattr(lib, name), name


def test_solver_packs_keys_as_model_ids_resolve_does():
    blob, off = Solver.pack_keys([])
    assert blob == b"" and off.dtype == np.int32 and list(off) == [0]
    keys = ["modèle-é", b"modele", "", b"\xff\x80raw", "日本"]
    blob, off = Solver.pack_keys(keys)
    as_bytes = [k.encode() if isinstance(k, str) else k for k in keys]
    assert blob == b"".join(as_bytes) and off.dtype == np.int32
    assert list(off) == [0, 10, 16, 16, 21, 27] and [blob[off[i]:off[i + 1]] for i in range(len(keys))] == as_bytes
    assert Solver.pack_keys(["abc", "é"])[0] == Solver.pack_keys([b"abc", "é".encode()])[0]  # str is its UTF-8 bytes
    # ... which is what model_ids_resolve hands over
    ref_blob, ref_off = Solver._pack(keys)
    assert ref_blob == blob and np.array_equal(ref_off.astype(np.int32), off)
    for method in ("place_batch_ck", "route_batch_ck", "miss_batch_ck"):
        assert callable(getattr(Solver, method))


def test_the_jni_veneer_names_the_three_natives_java_declares():
    java = open(os.path.join(ROOT, "integration", "GpuPlacementLB.java")).read()
    veneer = open(os.path.join(ROOT, "integration", "mmplace_jni.cc")).read()
    for native, call in (("placeBatchKeyed", "mmp_place_batch_ck"), ("routeBatchKeyed", "mmp_route_batch_ck"),
                         ("missBatchKeyed", "mmp_miss_batch_ck")):
        m = re.search(r"static\s+native\s+int\s+" + native + r"\s*\(([^)]*)\)\s*;", java)
        assert m, native + " is not declared in GpuPlacementLB.java"
        n_java = len(m.group(1).split(","))
        v = re.search(r"JNIEXPORT\s+jint\s+JNICALL\s+Java_com_ibm_watson_modelmesh_MmPlace_" + native + r"\s*\(([^)]*)\)\s*\{(.*?)\n\}", veneer, flags=re.S)
        assert v, native + " is not defined in mmplace_jni.cc"
        assert len(v.group(1).split(",")) == n_java + 2  # JNIEnv *, jclass in front
        assert call + "(" in v.group(2)
        assert n_java == len(ORDER[call])  # one Java argument per C argument (long h: the context)
    # the request path of the load balancers hands over the id's bytes where the ids are resident
    assert "MmPlace.placeBatchKeyed(" in java and "MmPlace.routeBatchKeyed(" in java
