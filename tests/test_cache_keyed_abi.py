"""CPU: the caches by model id at the boundary — include/mmplace.h declares mmp_caches_load_keyed_k, mmp_cache_replay_k,
mmp_cache_evicted_ids and mmp_cache_read_k in the stated order with the new constants, the ABI is still 3, the argument lists of the
three plain cache calls and of mmp_models_retire are what they were, modelmesh_amd/_lib.py binds the four calls with the header's
argument kinds, and libmmplace exports them and refuses a NULL context."""
import ctypes as C
import os
import re

from modelmesh_amd import _lib
from modelmesh_amd.solver import Solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmplace.h")

NEW = {
    "mmp_caches_load_keyed_k": ["ctx", "n_caches", "seg_off", "last_used", "weight", "keys", "key_off", "is_unloadbuf", "capacity", "ubm",
                                "key_row_out"],
    "mmp_cache_replay_k": ["ctx", "ops", "n_ops", "keys", "key_off", "now_ms", "key_status_out", "key_row_out", "outs", "evicted_rows",
                           "max_evicted", "n_evicted_slots", "ev_id_bytes_out", "max_id_bytes", "ev_id_off_out", "n_id_bytes_out"],
    "mmp_cache_evicted_ids": ["ctx", "bytes_out", "max_bytes", "off_out", "n_slots_out", "n_bytes_out"],
    "mmp_cache_read_k": ["ctx", "cache", "max_entries", "last_used", "weight", "row_out", "id_bytes_out", "max_id_bytes", "id_off_out",
                         "n_out", "n_id_bytes_out", "capacity", "weighted_size", "ubm"],
}
# the plain calls and the retirement, as they were before the caches could be bound
OLD = {
    "mmp_caches_load_keyed": [("mmp_ctx *", "ctx"), ("int32_t", "n_caches"), ("const int32_t *", "seg_off"), ("const int64_t *", "last_used"),
                              ("const int32_t *", "weight"), ("const int32_t *", "key"), ("const int64_t *", "capacity"),
                              ("const mmp_ubm_state *", "ubm")],
    "mmp_cache_replay": [("mmp_ctx *", "ctx"), ("const mmp_cache_op *", "ops"), ("int32_t", "n_ops"), ("int64_t", "now_ms"),
                         ("mmp_cache_op_out *", "outs"), ("int32_t *", "evicted_keys"), ("int32_t", "max_evicted"),
                         ("int32_t *", "n_evicted_slots")],
    "mmp_cache_read": [("mmp_ctx *", "ctx"), ("int32_t", "cache"), ("int32_t", "max_entries"), ("int64_t *", "last_used"),
                       ("int32_t *", "weight"), ("int32_t *", "key"), ("int32_t *", "n_out"), ("int64_t *", "capacity"),
                       ("int64_t *", "weighted_size"), ("mmp_ubm_state *", "ubm")],
    "mmp_models_retire": [("mmp_ctx *", "ctx"), ("const int32_t *", "rows"), ("int32_t", "n"), ("uint32_t", "flags"), ("int32_t *", "remap_out"),
                          ("int32_t", "max_models"), ("int32_t *", "n_models_after_out")],
}


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


def test_the_header_declares_the_four_calls_in_the_stated_order():
    for name, order in NEW.items():
        params = header_params(name)
        assert [a for _, a in params] == order, name
        assert params[0][0] == "mmp_ctx *"
    p = dict((a, t) for t, a in header_params("mmp_cache_replay_k"))
    assert (p["ops"], p["keys"], p["key_off"], p["ev_id_bytes_out"]) == ("const mmp_cache_op *", "const char *", "const int32_t *", "char *")
    assert dict((a, t) for t, a in header_params("mmp_caches_load_keyed_k"))["is_unloadbuf"] == "const uint8_t *"


def test_the_constants_agree_with_lib_and_the_abi_is_still_3():
    text = header_text()
    assert re.search(r"#define\s+MMP_ABI_VERSION\s+3\b", text)
    for name, want in (("MMP_COPK_RAW_KEY", _lib.COPK_RAW_KEY), ("MMP_CKEY_LIVE", _lib.CKEY_LIVE), ("MMP_CKEY_EMPTY_ROW", _lib.CKEY_EMPTY_ROW),
                       ("MMP_CKEY_UNKNOWN", _lib.CKEY_UNKNOWN)):
        m = re.search(r"#define\s+" + name + r"\s+(\d+)\b", text)
        assert m and int(m.group(1)) == want, name
    assert (_lib.COPK_RAW_KEY, _lib.CKEY_LIVE, _lib.CKEY_EMPTY_ROW, _lib.CKEY_UNKNOWN) == (1, 0, 1, 2)
    m = re.search(r"#define\s+MMP_CACHE_KEY_UNKNOWN\s+\((-2147483647 - 1)\)", text)
    assert m and _lib.CACHE_KEY_UNKNOWN == -2147483648 == eval(m.group(1))  # INT32_MIN, spelled as C spells it
    assert _lib.CACHE_KEY_UNKNOWN != _lib.UNLOADBUF_KEY
    assert set(_lib.COP_KEYLESS) == {6, 7, 9, 11} and set(_lib.COP_INSERTING) == {0, 4, 12}


def test_the_plain_cache_calls_and_the_retirement_keep_their_argument_lists():
    for name, want in OLD.items():
        assert header_params(name) == want, name


def test_lib_binds_the_four_calls_with_the_headers_argument_kinds():
    bound = {name: (ret, args) for name, ret, args in _lib.SYMBOLS}
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32}
    for name in NEW:
        assert name in bound, name
        ret, args = bound[name]
        assert ret is C.c_int

        def kind(t, a):
            if "*" not in t:
                return (kinds[t],)
            return (C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64))  # a pointer is bound untyped or by its scalar type

        params = header_params(name)
        assert len(args) == len(params), name
        for got, (t, a) in zip(args, params):
            assert got in kind(t, a), (name, a)
    for method in ("load_caches_keyed_k", "cache_replay_k", "cache_replay_k_raw", "cache_evicted_ids", "cache_read_k"):
        assert callable(getattr(Solver, method))


def test_libmmplace_exports_them_and_each_refuses_a_null_context():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    assert lib.mmp_abi_version() == 3
    n = (C.c_int32 * 4)(*([-7] * 4))
    p = lambda i: C.cast(C.byref(n, 4 * i), C.POINTER(C.c_int32))  # noqa: E731
    seg = (C.c_int32 * 1)(0)
    assert lib.mmp_caches_load_keyed_k(None, 0, seg, None, None, None, None, None, None, None, None) == _lib.MMP_EINVAL
    assert lib.mmp_cache_replay_k(None, None, 0, None, None, 1, None, None, None, None, 0, p(0), None, 0, None, p(1)) == _lib.MMP_EINVAL
    assert lib.mmp_cache_evicted_ids(None, None, 0, None, p(0), p(1)) == _lib.MMP_EINVAL
    assert lib.mmp_cache_read_k(None, 0, 0, None, None, None, None, 0, None, p(2), p(3), None, None, None) == _lib.MMP_EINVAL
    assert list(n) == [-7] * 4
