"""From raw instance events to committed type sets without decoding a record: streams of tests/ref_tcm_cases.py driven as
tests/test_ref_tcm_gpu.py drives them (walk, tests/golden/ref_tcm.npz: the reference's own listener + TypeConstraintManager text),
except that the instance events go in as KV events BY KEY through mmp_pods_events_json, with values rendered here — shuffled
field order, `labels` from the instance's label bits as "label-<i>" strings mixed with labels no type names — and that
mmp_types_from_pod_labels, over the label words the parser left in the context, stands in for mmp_types_from_labels.  One stream
also goes through mmp_pod_labels_set + mmp_pods_upsert.  The same checks under the same documented exceptions as that test.

Every stream must show that the labels matter: a pod's resident word changes between two checkpoints, and with the table as
it stands the type sets computed from the words before and after differ — the allowed sets wherever a type requires a label
(tcm_events_1, tcm_events_8, tcm_events_exact_0); in tcm_events_0 no type requires one (allowed is null throughout, req_bits
== [0, 0]), there it is type 0's preferred set."""
import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd.solver import Solver
from tests import ref_fleets as rf
from tests import ref_tcm_cases as tc
from tests.test_ref_tcm import GOLDEN, walk

pytestmark = pytest.mark.gpu
STREAMS = ("tcm_events_0", "tcm_events_1", "tcm_events_8", "tcm_events_exact_0")
NAMES = ["label-%d" % i for i in range(8)]
FIELDS = (("lruTime", "lru_time"), ("count", "count"), ("cap", "capacity"), ("used", "used"), ("lThreads", "loading_threads"),
          ("lInProg", "loading_in_progress"), ("rpm", "rpm"), ("vers", "version"))


@pytest.fixture(scope="module")
def cases():
    return dict(tc.cases())


def render(row, bits, rng):
    """the stored value of an instance: its row and its labels, fields in any order"""
    known = ["label-%d" % i for i in range(64) if (int(bits) >> i) & 1]
    els = known + ["other-%d" % int(rng.integers(100)) for _ in range(int(rng.integers(0, 3)))] + known[:int(rng.integers(0, 2))]
    rng.shuffle(els)
    members = ['"%s":%d' % (j, int(row[f])) for j, f in FIELDS] + ['"loc":"rack-%d"' % int(rng.integers(9)), '"shutdown":false']
    if els or rng.random() < 0.5:
        members.append('"labels":[%s]' % ",".join('"%s"' % e for e in els))
    elif rng.random() < 0.5:
        members.append('"labels":null')
    rng.shuffle(members)
    return "{%s}" % ",".join(members)


def drive(name, case, ref, by_json):
    fleet = case["fleet"]
    ids = rf.string_ids(fleet, 200)
    case["name"] = name
    P, T = fleet.n_pods, len(case["req_bits"])
    cks, _ = tc.parse(ref[f"{name}/words"], P, T)
    rng = np.random.default_rng(len(name))
    seen = {"word": False, "allowed": False, "prefer": False}
    s = Solver(fleet.min_space_units, fleet.min_churn_age_ms)
    try:
        s.label_names_load(NAMES)
        if by_json:
            io, _ = s.load_pod_ids(ids)
            assert np.array_equal(io, fleet.pods["id_order"])
        else:
            rows = fleet.pods.copy()
            rows["flags"] = _lib.POD_TOMBSTONE
            s.load_pods(rows)
        dev_table = {}

        def device_eval(f, table, cfg):
            # bring the device's table to `table`: the events since the last checkpoint, net
            words0 = s.pod_labels_get()[0].copy()
            gone = [p for p in dev_table if p not in table]
            if gone:
                if by_json:
                    status, idx, _, n = s.pods_events_json([ids[p] for p in gone], [""] * len(gone), deleted=np.ones(len(gone), np.uint8))
                    assert not status.any() and list(idx) == gone and n == 0
                else:
                    s.remove_pods(np.array(gone, np.int32))
                for p in gone:
                    del dev_table[p]
            changed = [p for p in table if p not in dev_table or dev_table[p].tobytes() != f.pods[p].tobytes()]
            if changed:
                if by_json:
                    status, idx, _, n = s.pods_events_json([ids[p] for p in changed], [render(f.pods[p], case["pod_bits"][p], rng) for p in changed])
                    assert not status.any() and list(idx) == changed and n == 0
                else:
                    s.pod_labels_set(changed, case["pod_bits"][changed], [bin(int(b)).count("1") for b in case["pod_bits"][changed]])
                    s.upsert_pods(np.array(changed, np.int32), f.pods[changed])
                for p in changed:
                    dev_table[p] = f.pods[p].copy()
            words1 = s.pod_labels_get()[0]
            for p in dev_table:
                assert words1[p] == case["pod_bits"][p], (name, p)
            req = np.array([cfg[t][0] for t in range(T)], np.uint64)
            pref = np.array([cfg[t][1] & ~cfg[t][0] for t in range(T)], np.uint64)
            if not np.array_equal(words0, words1):  # the same table under the words as they were: what the labels alone change
                seen["word"] = True
                al0, pf0, _, _ = s.types_from_labels(req, pref, words0)
            al, pf, ha, hp = s.types_from_pod_labels(req, pref)
            if not np.array_equal(words0, words1):
                seen["allowed"] |= not np.array_equal(al0, al)
                seen["prefer"] |= not np.array_equal(pf0, pf)
            W = (P + 63) // 64
            assert np.array_equal(ha, f.has_allowed) and np.array_equal(hp, f.has_prefer), name
            assert np.array_equal(al[:, :W], f.allowed[:, :W]) and np.array_equal(pf[:, :W], f.prefer[:, :W]), name
            s.commit()
            pts, parts = s.partitions()
            sets = [{t for t in range(T + 1) if (m >> t) & 1} for _, m in parts]
            pst = [st for st, _ in parts]
            return s.order()[: len(table)], s.stats(), pts, sets, pst, [s.type_stats(t) for t in range(T)]

        walk(case, cks, device_eval)
    finally:
        s.close()
    assert seen["word"], name
    if case["req_bits"].any():
        assert seen["allowed"], name
    else:
        assert name == "tcm_events_0" and seen["prefer"], name
    return len(cks)


@pytest.mark.parametrize("name", STREAMS)
def test_type_sets_from_kv_events_equal_the_reference_text(name, cases):
    assert drive(name, cases[name], np.load(GOLDEN), by_json=True) >= 8


def test_the_same_through_pod_labels_set_and_upsert(cases):
    assert drive("tcm_events_8", cases["tcm_events_8"], np.load(GOLDEN), by_json=False) >= 8
