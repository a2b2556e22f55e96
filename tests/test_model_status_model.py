"""The two Python forms of getStatus's answer (tests/model_status_model.py) against hand-worked cases and against each other:
the literal restatement of makeStatusInfo (MM.java:3013-3058) with the class of :3760-3768, and the vectorised closed rule the
device code uses.  No GPU."""
import numpy as np
import pytest

from modelmesh_amd import workload as wl
from modelmesh_amd._lib import (COPY_LOADING_FAILED as F, COPY_NOT_CHECKED as N, MST_ASK, MST_LOADING_FAILED, MST_NOT_FOUND,
                                MST_NOT_LOADED)
from tests import model_status_model as sm
from tests import registry_ops_model as ro
from tests.model_status_model import LONG_MAX, LONG_MIN, req_row, reqs_array

NOW = 1_700_000_000_000
# eight instances whose index order is NOT their id order: id_order[p] = rank of p's id
ID_ORDER = np.array([3, 0, 6, 1, 7, 2, 5, 4], np.uint32)
BY = [int(p) for p in np.argsort(ID_ORDER)]  # instances in id order: BY[0] has the smallest id


def both(records, rows, now=NOW):
    """One batch through both forms; they agree; returns (rows, copies)."""
    reg = [ro.ModelRecord(0, loaded, failed, 5) for loaded, failed in records]
    reqs = reqs_array(rows)
    want = sm.status_sequential(reg, ID_ORDER, reqs, now)
    got = sm.status_closed(*ro.registry_to_arrays(reg), ID_ORDER, reqs, now)
    sm.assert_same_status(got, want, "closed against sequential")
    for r, (loaded, failed) in zip(reg, records):  # nothing was written
        assert list(r.instance_ids.items()) == list(loaded) and list(r.load_failed_instance_ids.items()) == list(failed)
    return want


def one(loaded, failed, fail_pod=-1, miss=False, now=NOW):
    rows, copies = both([(loaded, failed)], [req_row(0, fail_pod, miss)], now)
    r = rows[0]
    assert int(r["copy_off"]) == 0 and int(r["n_not_checked"]) + int(r["n_failed"]) == len(copies)
    return int(r["cls"]), int(r["n_not_checked"]), int(r["n_failed"]), [tuple(int(x) for x in c) for c in copies]


@pytest.mark.parametrize("miss", [False, True])
def test_the_four_list_shapes_with_and_without_a_miss(miss):
    assert one([], [], miss=miss) == (MST_NOT_LOADED, 0, 0, [])                                        # :3767
    L, Fl = [(BY[1], NOW - 5), (BY[3], NOW - 9)], [(BY[2], NOW - 3), (BY[5], NOW - 7)]
    assert one(L, [], miss=miss) == (MST_NOT_LOADED if miss else MST_ASK, 2, 0, [(BY[1], N, NOW - 5), (BY[3], N, NOW - 9)])
    assert one([], Fl, miss=miss) == (MST_LOADING_FAILED, 0, 2, [(BY[2], F, NOW - 3), (BY[5], F, NOW - 7)])  # :3764 hasLoadFailure
    assert one(L, Fl, miss=miss) == (MST_LOADING_FAILED if miss else MST_ASK, 2, 2,
                                     [(BY[2], F, NOW - 3), (BY[1], N, NOW - 5), (BY[5], F, NOW - 7), (BY[3], N, NOW - 9)])
    # a load failure seen on the way with nothing recorded: LOADING_FAILED with the one copy
    assert one([], [], fail_pod=BY[4], miss=miss) == (MST_LOADING_FAILED, 0, 1, [(BY[4], F, NOW)])


def test_no_record():
    rows, copies = both([([], [])], [req_row(-1), req_row(-1, BY[3]), req_row(-1, -1, True), req_row(-1, BY[0], True)])
    assert rows["cls"].tolist() == [MST_NOT_FOUND] * 4                                                  # :3257
    assert rows["n_failed"].tolist() == [0, 1, 0, 1] and rows["n_not_checked"].tolist() == [0] * 4 and rows["copy_off"].tolist() == [0, 0, 1, 1]
    assert [tuple(int(x) for x in c) for c in copies] == [(BY[3], F, NOW), (BY[0], F, NOW)]             # the :3259 shape


def test_overlay_onto_a_loaded_instance_and_onto_a_failed_one():
    L, Fl = [(BY[1], NOW - 5), (BY[2], NOW - 4)], [(BY[2], NOW - 8)]
    # BY[1] is loaded and not failed: its loaded entry goes (:3022-3024), the failure is put at now
    assert one(L, Fl, fail_pod=BY[1]) == (MST_ASK, 1, 2, [(BY[1], F, NOW), (BY[2], N, NOW - 4), (BY[2], F, NOW - 8)])
    # the only loaded entry goes: nothing left to ask
    assert one([(BY[1], NOW - 5)], [], fail_pod=BY[1]) == (MST_LOADING_FAILED, 0, 1, [(BY[1], F, NOW)])
    # BY[2] is among the failed entries already: nothing changes, and its loaded entry stays (:3017)
    assert one(L, Fl, fail_pod=BY[2]) == (MST_ASK, 2, 1, [(BY[2], N, NOW - 4), (BY[1], N, NOW - 5), (BY[2], F, NOW - 8)])
    assert one(L, Fl, fail_pod=BY[2], miss=True)[0] == MST_LOADING_FAILED


def test_where_the_overlay_goes_in_id_order_beside_an_unresolved_entry():
    """All failed entries at time NOW: the output order of the ties IS the list order."""
    Fl = [(BY[2], NOW), (-1, NOW), (BY[5], NOW), (8, NOW)]  # -1 and 8 are not in the table of 8: never compared
    pods = lambda c: [p for p, _, _ in c]
    assert pods(one([], Fl, fail_pod=BY[0])[3]) == [BY[0], BY[2], -1, BY[5], 8]   # first
    assert pods(one([], Fl, fail_pod=BY[3])[3]) == [BY[2], -1, BY[3], BY[5], 8]   # middle: in front of the first RESOLVED greater one
    assert pods(one([], Fl, fail_pod=BY[7])[3]) == [BY[2], -1, BY[5], 8, BY[7]]   # last: behind the unresolved tail too
    # a failed entry at exactly `now` on each side of the overlay in id order
    got = one([], [(BY[2], NOW), (BY[6], NOW)], fail_pod=BY[4])
    assert got == (MST_LOADING_FAILED, 0, 3, [(BY[2], F, NOW), (BY[4], F, NOW), (BY[6], F, NOW)])
    # only unresolved entries: at the end
    assert pods(one([], [(-1, NOW), (9, NOW)], fail_pod=BY[0])[3]) == [-1, 9, BY[0]]


def test_ties_keep_the_concatenation_order():
    T = NOW - 1000
    assert one([(BY[1], T)], [(BY[0], T)])[3] == [(BY[1], N, T), (BY[0], F, T)]                      # the loaded one first
    assert one([(BY[0], T), (BY[1], T), (BY[2], T)], [(BY[5], T), (BY[6], T)])[3] == \
        [(BY[0], N, T), (BY[1], N, T), (BY[2], N, T), (BY[5], F, T), (BY[6], F, T)]                  # equal times within a list
    assert one([(BY[0], T), (BY[1], T + 1), (BY[2], T)], [])[3] == [(BY[1], N, T + 1), (BY[0], N, T), (BY[2], N, T)]


def test_times_at_the_ends_of_the_long_range():
    L = [(BY[0], 0), (BY[1], -1), (BY[2], LONG_MIN), (BY[3], LONG_MAX)]
    Fl = [(BY[4], LONG_MIN), (BY[5], LONG_MAX), (BY[6], 0), (BY[7], -1)]
    assert one(L, Fl)[3] == [(BY[3], N, LONG_MAX), (BY[5], F, LONG_MAX), (BY[0], N, 0), (BY[6], F, 0), (BY[1], N, -1), (BY[7], F, -1),
                             (BY[2], N, LONG_MIN), (BY[4], F, LONG_MIN)]
    # Long.compare, not a subtraction: MAX against MIN and -1 does not wrap
    assert one([(BY[0], LONG_MIN), (BY[1], LONG_MAX), (BY[2], -1)], [])[3] == [(BY[1], N, LONG_MAX), (BY[2], N, -1), (BY[0], N, LONG_MIN)]


def test_a_model_requested_twice_and_the_offsets():
    recs = [([(BY[1], NOW - 5)], [(BY[2], NOW - 3)]), ([], [])]
    rows, copies = both(recs, [req_row(0), req_row(1), req_row(0, BY[1], True), req_row(-1), req_row(0, BY[4])])
    assert rows["copy_off"].tolist() == [0, 2, 2, 4, 4] and len(copies) == 7
    assert rows["cls"].tolist() == [MST_ASK, MST_NOT_LOADED, MST_LOADING_FAILED, MST_NOT_FOUND, MST_ASK]
    assert sm.copies_of(rows, copies, 2) == [(BY[1], F, NOW), (BY[2], F, NOW - 3)]
    assert sm.copies_of(rows, copies, 4) == [(BY[4], F, NOW), (BY[2], F, NOW - 3), (BY[1], N, NOW - 5)]


def test_an_empty_batch_and_an_empty_registry():
    rows, copies = both([([], [])], [])
    assert len(rows) == 0 and len(copies) == 0
    empty = np.zeros(0, dtype=ro.MODEL_ROW)
    got = sm.status_closed(empty, np.zeros(0, np.int32), np.zeros(0, np.int64), ID_ORDER, reqs_array([req_row(-1, 2)]), NOW)
    sm.assert_same_status(got, sm.status_sequential([], ID_ORDER, reqs_array([req_row(-1, 2)]), NOW))


def status_fleet(seed, pods, models):
    """A fuzz fleet with the planted records: (fleet, registry, planted request rows, rng)."""
    fleet = wl.fuzz_fleet(seed + 1500, pods=pods, models=models)
    rng = np.random.default_rng(97_000 + seed)
    n_ent = len(fleet.ent_pod)
    fleet.ent_pod = np.where(rng.random(n_ent) < 0.03, rng.choice([-1, pods, pods + 7], n_ent), fleet.ent_pod).astype(np.int32)
    reg = ro.registry_from_arrays(fleet.models, fleet.ent_pod, fleet.ent_time)
    for r in reg:  # (a TreeMap holds a key once: an unresolved id drawn twice for one list collapses)
        r.instance_ids, r.load_failed_instance_ids = type(r.instance_ids)(r.instance_ids), type(r.load_failed_instance_ids)(r.load_failed_instance_ids)
    planted = sm.seed_shapes(reg, fleet.pods["id_order"], int(fleet.now))
    fleet.models, fleet.ent_pod, fleet.ent_time = ro.registry_to_arrays(reg)
    return fleet, reg, planted, rng


@pytest.mark.parametrize("pods,models,n", [(8, 300, 500), (300, 2000, 3000)])
def test_batches_by_construction_take_every_case_and_the_forms_agree(pods, models, n):
    fleet, reg, planted, rng = status_fleet(pods, pods, models)
    now, id_order = int(fleet.now), fleet.pods["id_order"]
    for batch in range(3):
        reqs = sm.draw_reqs(reg, id_order, now, rng, n, planted)
        missing = set(sm.CASES) - sm.cases_seen(reg, id_order, reqs, now)
        assert not missing, (batch, missing)
        want = sm.status_sequential(reg, id_order, reqs, now)
        sm.assert_same_status(sm.status_closed(fleet.models, fleet.ent_pod, fleet.ent_time, id_order, reqs, now), want, f"batch {batch}")
        assert len(want[1]) == int((want[0]["n_not_checked"] + want[0]["n_failed"]).sum())
        assert len(set(reqs["model"].tolist())) < len(reqs)  # models repeat
