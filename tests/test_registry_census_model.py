"""The two restatements of the registry census (tests/registry_census_model.py) against each other and against hand-worked
cases: the listener's two id sets over an event stream, and every boundary of the closed rule."""
import numpy as np
import pytest

from modelmesh_amd import workload as wl
from modelmesh_amd._lib import MODEL_ROW
from tests import registry_census_model as cm
from tests.registry_census_model import ENTRY_ADDED, ENTRY_DELETED, ENTRY_UPDATED, Listener, assert_same_census
from tests.registry_prune_model import LONG_MAX, Record, registry_from_arrays, registry_to_arrays

T0 = 1_760_000_000_000


def both(registry, n_pods, n_types):
    """The census of a list of Record in both forms; asserts them equal; returns it."""
    seq = cm.census_sequential(registry, n_pods, n_types)
    models, ent_pod, _ = registry_to_arrays(registry)
    assert_same_census(cm.census_closed(models, ent_pod, n_pods, n_types), seq, "closed against sequential")
    return seq


@pytest.mark.parametrize("seed,pods,models", [(0, 8, 300), (1, 40, 600), (2, 300, 2000), (3, 1, 50), (4, 70, 1)])
def test_the_two_forms_agree_on_fuzz_fleets(seed, pods, models):
    fleet = wl.fuzz_fleet(seed + 1200, pods=pods, models=models)
    rng = np.random.default_rng(seed)
    n_ent = len(fleet.ent_pod)
    # ids the table does not know on both sides of it, Long.MAX and never-used records, types beyond the table
    fleet.ent_pod = np.where(rng.random(n_ent) < 0.05, rng.choice([-1, pods, pods + 7], n_ent), fleet.ent_pod).astype(np.int32)
    fleet.models["last_used"] = np.where(rng.random(models) < 0.1, rng.choice([0, -1, LONG_MAX], models), fleet.models["last_used"])
    fleet.models["type"] = np.where(rng.random(models) < 0.1, rng.choice([-1, fleet.n_types, fleet.n_types + 3], models), fleet.models["type"])
    reg = registry_from_arrays(fleet.models, fleet.ent_pod, fleet.ent_time)
    stats, pl, pf, ts = both(reg, pods, fleet.n_types)
    # the arena in another layout (rows reversed, garbage between them): the closed form reads through ent_off
    order = np.arange(models)[::-1]
    m2 = fleet.models.copy()
    pods2 = []
    for i in order:
        r = fleet.models[i]
        pods2 += [-7, -7]  # garbage no row refers to
        m2[i]["ent_off"] = len(pods2)
        pods2 += list(fleet.ent_pod[r["ent_off"]: r["ent_off"] + r["n_loaded"] + r["n_failed"]])
    assert_same_census(cm.census_closed(m2, np.array(pods2, np.int32), pods, fleet.n_types), (stats, pl, pf, ts), "scattered arena")
    assert int(stats["n_models"]) == models and int(stats["copies_hist"].sum()) == models
    assert int(pl.sum() + pf.sum() + stats["n_entries_unresolved"]) == int(stats["n_entries_loaded"] + stats["n_entries_failed"])


def test_an_event_stream_by_hand():
    """add, update that empties instanceIds, update that adds a failure, delete: after each event the listener's counts equal a
    census of the registry at that point."""
    lst = Listener()

    def check(want_loaded, want_failed, want_total):
        assert lst.counts() == (want_loaded, want_failed, want_total)
        s, _, _, _ = both(lst.records(), 4, 0)
        assert (int(s["n_loaded"]), int(s["n_failed"]), int(s["n_models"])) == lst.counts()

    check(0, 0, 0)
    lst.event(ENTRY_ADDED, 0, Record(0, [(1, T0)], [], T0))
    check(1, 0, 1)
    assert lst.loaded_model_count == 1 and lst.failed_model_count == -1  # (failedChanged was false: :2845 did not run)
    lst.event(ENTRY_ADDED, 1, Record(0, [(1, T0), (2, T0)], [], T0))
    check(2, 0, 2)
    lst.event(ENTRY_ADDED, 2, Record(0, [], [], T0))                    # registered, loaded nowhere
    check(2, 0, 3)
    lst.event(ENTRY_UPDATED, 0, Record(0, [], [], T0))                  # the update empties instanceIds
    check(1, 0, 3)
    lst.event(ENTRY_UPDATED, 0, Record(0, [], [], T0 + 1))              # an update that changes neither set
    check(1, 0, 3)
    assert lst.loaded_model_count == 1
    lst.event(ENTRY_UPDATED, 1, Record(0, [(1, T0), (2, T0)], [(3, T0)], T0))  # a failure beside two copies
    check(1, 1, 3)
    assert lst.failed_model_count == 1
    lst.event(ENTRY_UPDATED, 2, Record(0, [], [(3, T0)], T0))           # a failure and no copy
    check(1, 2, 3)
    lst.event(ENTRY_DELETED, 1, Record(0, [(1, T0), (2, T0)], [(3, T0)], T0))  # (the deleted record still lists its instances: :2828 type != ENTRY_DELETED)
    check(0, 1, 2)
    lst.event(ENTRY_DELETED, 2, Record(0, [], [(3, T0)], T0))
    check(0, 0, 1)
    lst.event(ENTRY_DELETED, 0, Record(0, [], [], T0))
    check(0, 0, 0)


def test_only_failed_entries_and_both_lists():
    reg = [Record(0, [], [(2, T0), (0, T0)], T0),          # only failed entries: in failedModelIds, not in loadedModelIds
           Record(1, [(0, T0), (1, T0)], [(2, T0)], T0),   # both lists
           Record(1, [(1, T0)], [], T0)]
    s, pl, pf, ts = both(reg, 3, 2)
    assert (int(s["n_models"]), int(s["n_loaded"]), int(s["n_failed"]), int(s["n_loaded_and_failed"])) == (3, 2, 2, 1)
    assert (int(s["n_entries_loaded"]), int(s["n_entries_failed"]), int(s["n_entries_unresolved"])) == (3, 3, 0)
    assert pl.tolist() == [1, 2, 0] and pf.tolist() == [1, 0, 2]
    assert s["copies_hist"].tolist() == [1, 1, 1, 0, 0] and int(s["max_copies"]) == 2
    assert ts["n_models"].tolist() == [1, 2] and ts["n_loaded"].tolist() == [0, 2] and ts["n_failed"].tolist() == [1, 1]
    assert ts["n_entries_loaded"].tolist() == [0, 3]
    assert int(s["n_unloaded_used"]) == 1  # the first record: no copy, a real lastUsed


def test_last_used_boundaries():
    """n_unloaded_used needs 0 < last_used < Long.MAX and no copy; n_last_used_max counts Long.MAX whatever the copies."""
    lus = [0, -1, 1, LONG_MAX - 1, LONG_MAX, T0]
    reg = [Record(0, [], [], lu) for lu in lus] + [Record(0, [(0, T0)], [], lu) for lu in lus]
    s, _, _, _ = both(reg, 1, 0)
    assert int(s["n_unloaded_used"]) == 3      # 1, Long.MAX - 1, T0 among the unloaded
    assert int(s["n_last_used_max"]) == 2      # one unloaded, one loaded
    assert int(s["n_loaded"]) == 6 and s["copies_hist"].tolist() == [6, 6, 0, 0, 0]


def test_ids_the_table_does_not_know():
    P = 5
    reg = [Record(0, [(-1, T0), (0, T0)], [(P, T0)], T0),     # pod -1 and pod == P: both outside [0, P)
           Record(0, [(P - 1, T0)], [(-1, T0), (-1, T0)], T0)]  # the last slot is inside; two unknown ids in one list both count
    s, pl, pf, _ = both(reg, P, 0)
    assert int(s["n_entries_unresolved"]) == 4
    assert pl.tolist() == [1, 0, 0, 0, 1] and pf.tolist() == [0] * P
    assert int(s["n_loaded"]) == 2 and int(s["n_failed"]) == 2  # an unknown id still makes its record loaded / failed
    assert int(s["n_entries_loaded"]) == 3 and int(s["n_entries_failed"]) == 3


def test_three_and_four_copies():
    reg = [Record(0, [(p, T0) for p in range(3)], [], T0), Record(0, [(p, T0) for p in range(4)], [], T0),
           Record(0, [(p, T0) for p in range(9)], [], T0)]
    s, pl, _, _ = both(reg, 9, 0)
    assert s["copies_hist"].tolist() == [0, 0, 0, 1, 2] and int(s["max_copies"]) == 9
    assert pl.tolist() == [3, 3, 3, 2, 1, 1, 1, 1, 1]


def test_types_outside_the_table_count_in_the_totals_only():
    reg = [Record(-1, [(0, T0)], [], T0), Record(2, [(0, T0)], [(1, T0)], T0), Record(1, [(1, T0)], [], T0)]
    s, _, _, ts = both(reg, 2, 2)
    assert int(s["n_models"]) == 3 and int(s["n_loaded"]) == 3
    assert ts["n_models"].tolist() == [0, 1] and ts["n_loaded"].tolist() == [0, 1] and ts["n_failed"].tolist() == [0, 0]
    s0, _, _, ts0 = both(reg, 2, 0)  # no type table
    assert len(ts0) == 0 and int(s0["n_models"]) == 3


def test_the_empty_registry():
    s, pl, pf, ts = both([], 3, 2)
    assert all(int(s[f]) == 0 for f in cm.SCALARS) and not s["copies_hist"].any()
    assert pl.tolist() == [0, 0, 0] and pf.tolist() == [0, 0, 0] and not ts["n_models"].any()
    models = np.zeros(0, dtype=MODEL_ROW)
    assert_same_census(cm.census_closed(models, np.zeros(0, np.int32), 0, 0), cm.census_sequential([], 0, 0))
