"""CPU: the expansion rule of the single-caller route and miss calls (tests/seam_caller_model.py) on rows worked out by hand,
and as the inverse of splitting a full row, on every row of tests/golden/ref_gate_edges.npz's cases."""
import numpy as np
import pytest

from modelmesh_amd import _lib
from tests import seam_caller_model as scm
from tests.gate_helpers import GOLDEN_GATE_EDGES, gate_edge_inputs

FAVOUR, HAVE_ENTRY, DONE, CREATED, HINT, FORCE = 1, 2, 4, 8, 32, 64


def hand_caller():
    c = np.zeros(1, dtype=_lib.SEAM_CALLER)
    c["self_pod"], c["gate_flags"] = 7, FAVOUR | FORCE  # FAVOUR only here, FORCE here and on row 1
    c["loading_count"], c["weight_predict_cutoff"] = 11, 10
    c["cache_capacity"], c["cache_weighted_size"], c["cache_oldest_time"] = 8_388_608, 8_000_000, 1_700_000_000_123
    c["load_timeout_ms"] = 240_000
    c["fresh_lru"], c["fresh_capacity"], c["fresh_used"] = -1, 8_388_608, 7_999_999
    c["fresh_count"], c["fresh_loading_threads"], c["fresh_in_progress"], c["fresh_rpm"] = 40, 8, 2, 150
    c["last_published"] = 1_700_000_000_000
    c["local_in_flight"], c["reserved"], c["last_invoke_time"] = 3, 0x5A5A, 1_700_000_000_456  # reserved reaches no row
    return c


def hand_rows():
    g = np.zeros(3, dtype=_lib.GATE_REQ_C)
    g["model"] = [5, -1, 299]
    g["flags"] = [0, FORCE | HINT, HAVE_ENTRY | DONE]  # HINT and HAVE_ENTRY | DONE only on a row
    g["excl_off"], g["n_excl"] = [0, 2, 2], [2, 0, 6]
    g["explicit_off"], g["n_explicit"] = [3, 0, 0], [5, 0, 1]
    g["size_hint"], g["loader_predicted"] = [0, 6400, -1], [100, 200, 2**31 - 1]
    g["last_used_time"], g["loaded_time"] = [0, 12, -(2**63)], [-1, 2**63 - 1, 34]
    s = np.zeros(3, dtype=_lib.SERVE_REQ_C)
    s["flags"], s["cnt_off"], s["n_cnt"] = [0, 1, 3], [0, 2, 2], [2, 0, 5]
    s["reserved"] = [9, 9, 9]  # reaches no row
    s["assume_completed_ms"] = [3000, 30_000, 0]
    return g, s


def test_the_gate_row_worked_out_by_hand():
    c, (g, s) = hand_caller(), hand_rows()
    full = scm.expand_gate(c, g)
    assert full.dtype == _lib.GATE_REQ and len(full) == 3
    # flags: the caller's bits are ORed into every row's
    assert full["flags"].tolist() == [FAVOUR | FORCE, FAVOUR | FORCE | HINT, FAVOUR | FORCE | HAVE_ENTRY | DONE]
    want0 = (5, 7, FAVOUR | FORCE, 0, 2, 3, 5, 0, 0, 8_388_608, 8_000_000, 1_700_000_000_123, 100, 11, 10, 0, -1, 240_000,
             -1, 8_388_608, 7_999_999, 40, 8, 2, 150, 1_700_000_000_000)
    assert full[0].tolist() == want0  # field by field in the order of mmp_gate_req
    assert full["model"].tolist() == [5, -1, 299] and full["self_pod"].tolist() == [7, 7, 7]
    assert full["size_hint"].tolist() == [0, 6400, -1] and full["loader_predicted"].tolist() == [100, 200, 2**31 - 1]
    assert full["last_used_time"].tolist() == [0, 12, -(2**63)] and full["loaded_time"].tolist() == [-1, 2**63 - 1, 34]
    assert full["excl_off"].tolist() == [0, 2, 2] and full["n_excl"].tolist() == [2, 0, 6]
    assert full["explicit_off"].tolist() == [3, 0, 0] and full["n_explicit"].tolist() == [5, 0, 1]
    assert full["reserved"].tolist() == [0, 0, 0]
    for f in scm.GATE_CALLER_FIELDS:  # the caller's side is the same in every row
        assert (full[f] == c[f][0]).all(), f


def test_the_serve_row_takes_the_gate_rows_model_and_exclusion_range():
    c, (g, s) = hand_caller(), hand_rows()
    gate, serve = scm.expand_route(c, g, s)
    assert np.array_equal(gate, scm.expand_gate(c, g))
    assert serve.dtype == _lib.SERVE_REQ
    assert serve[2].tolist() == (299, 7, 3, 3, 1_700_000_000_456, 0, 2, 6, 2, 5)  # mmp_serve_req's field order
    assert serve["excl_off"].tolist() == g["excl_off"].tolist() and serve["n_excl"].tolist() == g["n_excl"].tolist()
    assert serve["model"].tolist() == [5, -1, 299]
    assert serve["flags"].tolist() == [0, 1, 3]  # MMP_SERVE_*: the caller's MMP_GATE_* bits do not reach them
    assert serve["cnt_off"].tolist() == [0, 2, 2] and serve["n_cnt"].tolist() == [2, 0, 5]
    assert serve["assume_completed_ms"].tolist() == [3000, 30_000, 0]
    assert (serve["local_in_flight"] == 3).all() and (serve["last_invoke_time"] == 1_700_000_000_456).all()


def test_the_miss_rows_are_the_gate_rows_and_place_batch_cs_rows():
    c, (g, _) = hand_caller(), hand_rows()
    pc = np.zeros(1, dtype=_lib.PLACE_CALLER)
    pc["self_pod"], pc["flags"], pc["fresh_lru"], pc["fresh_capacity"], pc["fresh_used"] = 7, 1, 55, 66, 77
    pc["fresh_count"], pc["fresh_rpm"] = 8, 9
    pq = np.zeros(3, dtype=_lib.PLACE_REQ_C)
    pq["model"], pq["pick"], pq["last_used"] = g["model"], [1, 2**32 - 1, 3], [10, 20, 30]
    pq["extra_off"], pq["n_extra"] = [0, 0, 4], [0, 4, 1]
    gate, place = scm.expand_miss(c, pc, g, pq)
    assert np.array_equal(gate, scm.expand_gate(c, g))
    assert place.dtype == _lib.PLACE_REQ
    assert place[1].tolist() == (-1, 7, 1, 2**32 - 1, 20, 0, 4, 55, 66, 77, 8, 9)
    assert np.array_equal(place, _lib.join_caller(pc, pq))


def test_empty_batches_expand_to_empty_rows():
    c = hand_caller()
    gate, serve = scm.expand_route(c, np.zeros(0, _lib.GATE_REQ_C), np.zeros(0, _lib.SERVE_REQ_C))
    assert len(gate) == 0 and len(serve) == 0 and gate.dtype == _lib.GATE_REQ and serve.dtype == _lib.SERVE_REQ


@pytest.fixture(scope="module")
def edge_cases():
    return gate_edge_inputs(np.load(GOLDEN_GATE_EDGES))


def test_split_then_expand_is_the_identity_on_every_row_of_the_gate_edge_cases(edge_cases):
    total = 0
    for name, _, _, r, *_ in edge_cases:
        assert (r["reserved"] == 0).all(), name
        sides = scm.request_side(r)
        for i in range(len(r)):
            caller, row = scm.split_gate(r[i])
            assert caller["gate_flags"][0] == 0 and row[0] == sides[i]
            back = scm.expand_gate(caller, row)
            assert back.tobytes() == r[i:i + 1].tobytes(), (name, i)
        # ... and wherever the shared flag bits sit: on the caller, on the row, or on both
        common = int(np.bitwise_and.reduce(r["flags"]))
        for i in (0, len(r) // 2, len(r) - 1):
            caller, row = scm.split_gate(r[i])
            fl = int(r["flags"][i])
            for on_caller, on_row in ((fl, 0), (fl & 0x0F, fl & ~0x0F), (fl, fl), (common, fl)):
                caller["gate_flags"], row["flags"] = on_caller, on_row
                assert scm.expand_gate(caller, row).tobytes() == r[i:i + 1].tobytes(), (name, i, on_caller, on_row)
        total += len(r)
    ref = np.load(GOLDEN_GATE_EDGES)
    assert total == sum(len(ref[f"{n}/gate"]) for n in ref["names"]) == 16_751  # every row of the twelve cases
