"""CPU: the reference's own vmodel tests as a closed loop.  tests/golden/vmodel_kats.json holds the steps and assertions of
VModelsTest.vModelsTest and VModelsTest.vModelOwnerTest; tests/vmodel_minimesh.py runs them with its three writers written against
the answers of the two calls, here given by tests/vmodel_write_model.py and tests/model_refs_model.py.  Every assertion of the two
tests is reproduced, and the refs arithmetic behind them is followed step by step."""
import json
import os

import pytest

from tests import model_refs_model as mr
from tests.vmodel_minimesh import MeshError, MiniVMesh, run_scenario

KATS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vmodel_kats.json")))
NOW, AGE = 1_700_000_000_000, 600_000


def refs_of(mesh, model):
    last = dict((n, v) for n, _s, v in mr.members(mesh.registry[model]))
    return int(last.get(b"refs", b"0"))


def test_the_fixture_names_its_source_lines():
    for name in ("vModelsTest", "vModelOwnerTest"):
        kat = KATS[name]
        assert "VModelsTest.java:" in kat["source"] and all(st["at"].startswith(":") for st in kat["steps"])
    assert sum("expect" in st for st in KATS["vModelsTest"]["steps"]) == 11
    assert sum("expect" in st for st in KATS["vModelOwnerTest"]["steps"]) == 10


def test_vmodels_test():
    """unregisterModel refused while referenced, then allowed; both FAILED_PRECONDITIONs; active = myNextModel3 while the target is
    myNextModel4; myNextModel3 auto-deleted by the transition; myNextModel4 kept by the vmodel's deletion."""
    mesh = MiniVMesh(NOW, AGE)
    trail = []

    def after(m, st):
        trail.append((st["at"], {k.decode(): refs_of(m, k) for k in sorted(m.registry)}, sorted(k.decode() for k in m.vmodels)))

    run_scenario(mesh, KATS["vModelsTest"]["steps"], after)
    by_line = {at: (refs, vms) for at, refs, vms in trail}
    assert by_line[":93-94"] == ({"myModel": 1}, ["test-vmodel-a"])
    assert by_line[":114-125"][0] == {"myModel": 0, "myNextModel3": 1}      # the transition gave myModel's referent back
    assert by_line[":132-133"][0] == {"myNextModel3": 1}                    # ... so it could be unregistered
    assert by_line[":136-139"][0] == {"myNextModel3": 1}                    # the same target: no second referent
    assert by_line[":170-179"][0] == {"another-model": 0, "myNextModel3": 1, "myNextModel4": 1}
    assert by_line[":189-191"][0] == {"another-model": 0, "myNextModel4": 1}  # myNextModel3 was created with autoDelete
    assert by_line[":200-201"] == ({"another-model": 0, "myNextModel4": 0}, [])  # myNextModel4 was not
    assert b'"autoDel"' not in mesh.registry[b"another-model"] and sorted(mesh.registry) == [b"another-model"]


def test_vmodel_owner_test():
    """ALREADY_EXISTS with the stored owner; the owner2 delete without effect, the owner1 delete with effect."""
    mesh = MiniVMesh(NOW, AGE)
    seen = []
    run_scenario(mesh, KATS["vModelOwnerTest"]["steps"], lambda m, st: seen.append((st["at"], refs_of(m, b"myModel") if m.registry else None,
                                                                                   sorted(m.vmodels))))
    by_line = {at: rest for at, *rest in seen}
    assert by_line[":247-249"] == [2, [b"test-vmodel-a", b"test-vmodel-owner1"]]
    assert by_line[":262-269"] == [2, [b"test-vmodel-a", b"test-vmodel-owner1"]]  # a refused set changes nothing
    assert by_line[":288-289"] == [2, [b"test-vmodel-a", b"test-vmodel-owner1"]]
    assert by_line[":297-298"] == [1, [b"test-vmodel-a"]]
    assert by_line[":305"] == [0, []] and by_line[":306"] == [None, []]
    assert mesh.vmodels == {} and mesh.registry == {}


def test_a_transaction_is_all_or_nothing():
    mesh = MiniVMesh(NOW, AGE)
    with pytest.raises(MeshError) as e:
        mesh.set_vmodel(b"v", b"no-such-model")  # no modelInfo and no stored target: VMM:203-205
    assert e.value.code == "NOT_FOUND" and mesh.vmodels == {} and mesh.registry == {}
    mesh.set_vmodel(b"v", b"made", type_=b"t", auto_delete=True)
    assert mesh.registry[b"made"] == b'{"type":"t","refs":1,"autoDel":true,"lu":%d}' % (NOW - 6 * AGE)
    assert mesh.vmodels[b"v"] == b'{"amid":"made","tmid":"made"}'
    mesh.delete_vmodel(b"v")
    assert mesh.vmodels == {} and mesh.registry == {}  # created for the vmodel, deleted with it
