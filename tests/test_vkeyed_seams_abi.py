"""CPU: the request seams by vmodel id at the boundary — include/mmplace.h declares the three calls (the _ck signatures with
nf_keys / nf_off / req_flags behind key_off and vm_out in the place of model_idx_out) and the 24-byte mmp_vseam_row,
modelmesh_amd/_lib.py binds them with the header's argument kinds in the header's order, the library exports them, and the JNI
veneer defines the natives integration/GpuPlacementLB.java declares.  Also the oracle of the GPU test
(tests/vkeyed_seam_model.py) held to the reference's own vmodel scenarios (tests/golden/vmodel_kats.json) where they speak of a
resolution."""
import ctypes as C
import json
import os
import re

import numpy as np

from modelmesh_amd import _lib
from modelmesh_amd.solver import Solver
from tests import vkeyed_seam_model as vksm
from tests import vmodel_model as vm
from tests.keyed_seam_model import KeyRows
from tests.test_keyed_seams_abi import ORDER as CK_ORDER, ROWS as CK_ROWS, ctype_of, header_params
from tests.vmodel_minimesh import MiniVMesh, run_scenario

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmplace.h")


def cv_order(ck_order):
    """the _ck argument list with the three arrays behind key_off and vm_out last"""
    at = ck_order.index("key_off") + 1
    assert ck_order[-1] == "model_idx_out"
    return ck_order[:at] + ["nf_keys", "nf_off", "req_flags"] + ck_order[at:-1] + ["vm_out"]


ORDER = {name[:-1] + "v": cv_order(order) for name, order in CK_ORDER.items()}
ROWS = {name[:-1] + "v": rows for name, rows in CK_ROWS.items()}


def test_the_header_declares_the_three_calls_as_the_ck_forms_with_the_stated_differences():
    assert sorted(ORDER) == ["mmp_miss_batch_cv", "mmp_place_batch_cv", "mmp_route_batch_cv"]
    for name, order in ORDER.items():
        params = header_params(name)
        assert [p[1] for p in params] == order, name
        types = dict((a, t) for t, a in params)
        for arg, struct in ROWS[name].items():
            assert struct in types[arg] and "*" in types[arg], (name, arg)
            assert ("const" in types[arg]) == (not arg.endswith("outs")), (name, arg)
        assert types["keys"] == "const char *" and types["key_off"] == "const int32_t *"
        assert types["nf_keys"] == "const char *" and types["nf_off"] == "const int32_t *" and types["req_flags"] == "const uint32_t *"
        assert types["vm_out"] == "mmp_vseam_row *"
        assert types["n"] == "int32_t" and types["now_ms"] == "int64_t"
    text = open(HEADER).read()
    assert "THE RULE BY VMODEL KEY" in text
    m = re.search(r"typedef struct \{([^}]*)\} mmp_vseam_row;", text)
    assert m, "mmp_vseam_row is not declared"
    fields = [(t, f.strip()) for t, names in re.findall(r"(u?int32_t)\s+([^;]+);", m.group(1)) for f in names.split(",")]
    assert fields == [("int32_t", "cls"), ("int32_t", "which"), ("int32_t", "vmodel"), ("int32_t", "model"), ("uint32_t", "flags"),
                      ("int32_t", "reserved")]


def test_sizeof_mmp_vseam_row_is_24_and_its_fields_are_the_shared_ones_of_the_answer():
    assert _lib.VSEAM_ROW.itemsize == 24 and _lib.VSEAM_ROW.names == vksm.VSEAM_FIELDS
    assert [_lib.VSEAM_ROW.fields[f][1] for f in _lib.VSEAM_ROW.names] == [0, 4, 8, 12, 16, 20]
    for f in ("cls", "which", "vmodel", "model", "flags"):
        assert _lib.VSEAM_ROW.fields[f][0] == _lib.VMODEL_ANSWER.fields[f][0]
    assert vksm.VKeyRows(KeyRows([])).answers([]).dtype == _lib.VSEAM_ROW


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
    for method in ("place_batch_cv", "route_batch_cv", "miss_batch_cv"):
        assert callable(getattr(Solver, method))


def test_the_jni_veneer_names_the_three_natives_java_declares():
    java = open(os.path.join(ROOT, "integration", "GpuPlacementLB.java")).read()
    veneer = open(os.path.join(ROOT, "integration", "mmplace_jni.cc")).read()
    for native, call in (("placeBatchVKeyed", "mmp_place_batch_cv"), ("routeBatchVKeyed", "mmp_route_batch_cv"),
                         ("missBatchVKeyed", "mmp_miss_batch_cv")):
        m = re.search(r"static\s+native\s+int\s+" + native + r"\s*\(([^)]*)\)\s*;", java)
        assert m, native + " is not declared in GpuPlacementLB.java"
        n_java = len(m.group(1).split(","))
        v = re.search(r"JNIEXPORT\s+jint\s+JNICALL\s+Java_com_ibm_watson_modelmesh_MmPlace_" + native + r"\s*\(([^)]*)\)\s*\{(.*?)\n\}", veneer, flags=re.S)
        assert v, native + " is not defined in mmplace_jni.cc"
        assert len(v.group(1).split(",")) == n_java + 2  # JNIEnv *, jclass in front
        assert call + "(" in v.group(2)
        assert n_java == len(ORDER[call])  # one Java argument per C argument (long h: the context)
    assert "MmPlace.routeBatchVKeyed(" in java  # the callModel loop of a vmodel request


# ---- the oracle of the GPU test against the reference's own scenarios ---------------------------------------------------------------
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "vmodel_kats.json")))
NOW, AGE = 1_700_000_000_000, 600_000


def composed(mesh):
    """The two dicts of the composition rebuilt from the mesh's two KV tables as a listener would see them"""
    km = KeyRows(list(mesh.registry))
    vk = vksm.VKeyRows(km)
    keys = list(mesh.vmodels)
    st, _, n_app = vk.events(keys, [mesh.vmodels[k] for k in keys])
    assert not st.any() and n_app == len(keys)
    return km, vk


def test_the_composition_answers_what_the_reference_scenarios_expect():
    checked = {"model": 0, "active": 0, "not_found": 0}
    for name in ("vModelsTest", "vModelOwnerTest"):
        mesh = MiniVMesh(NOW, AGE)

        def after(m, st):
            km, vk = composed(m)
            expect, key = st.get("expect", {}), st.get("vmodel", "").encode()
            # every stored vmodel: with no notFoundModelId the request resolves to its active model's registry row
            for k, stored in m.vmodels.items():
                rec = vm.classify(stored)[1]
                cls, which, v, model, flags, _ = vk.answer(k)
                assert (cls, which, v) == (vm.OK, vm.ACTIVE, vk.vt.row_of[k]) and model == km.row.get(rec.amid, -1) and flags == 0
                assert vk.rows([k])[0] == model
            if "error" in expect or not key or st.get("owner"):  # (owners are not on the request path)
                return
            ans = vk.answers([key])
            if st["call"] == "resolve":  # resolveVModelId's own assertion
                assert ans["cls"][0] == vm.OK and km.ids()[ans["model"][0]] == expect["model"].encode()
                checked["model"] += 1
            elif "active" in expect and expect["active"]:
                assert ans["cls"][0] == vm.OK and ans["which"][0] == vm.ACTIVE
                assert km.ids()[vk.rows([key])[0]] == expect["active"].encode()
                checked["active"] += 1
                # the second attempt of callModel: the active model was not found
                target = expect["target"].encode()
                again = vk.answers([key], [expect["active"].encode()], [0])
                assert again["cls"][0] == vm.STRONG_READ and vk.rows([key], [expect["active"].encode()], [0])[0] == -1
                after_strong = vk.answers([key], [expect["active"].encode()], [vksm.AFTER_STRONG])
                if target != expect["active"].encode():
                    assert (after_strong["cls"][0], after_strong["which"][0]) == (vm.OK, vm.TARGET)
                    assert km.ids()[after_strong["model"][0]] == target
                else:
                    assert after_strong["cls"][0] == vm.TARGET_NOT_FOUND and after_strong["model"][0] == -1
            elif expect.get("status") == "NOT_FOUND":
                assert ans["cls"][0] == vm.NOT_FOUND and ans["vmodel"][0] == -1 and vk.rows([key])[0] == -1
                checked["not_found"] += 1

        run_scenario(mesh, KATS[name]["steps"], after)
    assert checked["model"] == 1 and checked["active"] >= 2 and checked["not_found"] >= 2, checked


def test_a_retire_renumbers_the_vmodel_rows_of_the_composition():
    vk = vksm.VKeyRows(KeyRows([b"m0", b"m1"]))
    vk.events([b"a", b"b", b"c"], [vm.render("m0", "m0"), vm.render("m1", "m0"), vm.render("m1", "m1")])
    vk.events([b"a"], [""], [1])
    assert vk.answer(b"a")[0] == vm.NOT_FOUND and vk.answer(b"c")[2:4] == (2, 1)
    vk.retire(np.array([-1, 0, 1], np.int32))
    assert vk.answer(b"a") == (vm.NOT_FOUND, 0, -1, -1, 0, 0) and vk.answer(b"b")[2:4] == (0, 1) and vk.answer(b"c")[2:4] == (1, 1)
    assert vk.answer(b"b", b"m1", vksm.AFTER_STRONG) == (vm.OK, vm.TARGET, 0, 0, 0, 0)
    vk.km.retire(np.array([-1, 0], np.int32))  # m0 leaves the registry: the vmodel still names it, the registry no longer does
    assert vk.answer(b"b", b"m1", vksm.AFTER_STRONG) == (vm.OK, vm.TARGET, 0, -1, 0, 0) and vk.rows([b"b"])[0] == 0
