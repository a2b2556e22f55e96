"""CPU: the periodic tasks by model id as tests/tasks_keyed_model.py restates them, the boundaries worked by hand — an unknown id
and a deleted record are `model == -1` and the cache loop REMOVES their entries (:5968); the janitor's scale-down reads the registry
the two loops left; the budget of :6117-6130; a MaxConcCacheEntry row follows its candidate, not its position.  And the recipe of
the chain tests shows what the GPU file relies on."""
import copy

import numpy as np
import pytest

from modelmesh_amd._lib import (CACHE_ENTRY, JAN_IN_ORDER, JAN_REGISTERED, JAN_REMOVED, JANITOR_ENTRY, JE_DONE, JE_STATE_LIVE)
from tests import janitor_model as jm
from tests import tasks_keyed_model as tk
from tests.tasks_keyed_model import CHAIN_SELF, InvalidEntries


@pytest.fixture(scope="module")
def chain():
    return tk.chain_world()


def old_row(now, r=0):
    e = np.zeros(1, dtype=JANITOR_ENTRY)
    e[0] = (-1, 100, now - 2_000_000 - r, now - 3_000_000, 0, -1, 0, 0, 0, 0, 0, JE_DONE | JE_STATE_LIVE, 0)
    return e


def test_an_entry_whose_id_is_unknown_is_removed_by_the_cache_loop_and_a_deleted_record_behaves_the_same(chain):
    w0, now = chain
    w = copy.deepcopy(w0)
    prm = jm.params(CHAIN_SELF, now)
    e = np.concatenate([old_row(now, 0), old_row(now, 1), old_row(now, 2)])
    w.delete(b"hot-1")
    before = copy.deepcopy(w.registry)
    idx, actions, edits, cands, crow, removed, info = w.janitor(e, [b"never-seen", b"hot-1", b"m100"], prm)
    assert idx.tolist() == [-1, 1, 100]                                   # the deleted id keeps its row in the table
    assert actions.tolist() == [JAN_REMOVED, JAN_REMOVED, JAN_REGISTERED]  # :5968 mr == null, twice; a live record is registered
    assert b"hot-1" not in w.registry and w.get(b"hot-1") is None
    assert 100 in edits["model"].tolist() and 1 not in edits["model"].tolist()
    # the same two ids in the three read-only tasks: model -1
    c = np.zeros(3, dtype=CACHE_ENTRY)
    c["last_used"], c["weight"] = now - 5_000_000, 10
    w = copy.deepcopy(w0)
    w.delete(b"hot-1")
    idx, act, wait = w.migration(c, [b"never-seen", b"hot-1", b"hot-2"], CHAIN_SELF, now)
    assert idx.tolist() == [-1, 1, 2] and act.tolist() == [0, 0, 1]
    idx, rem = w.scaledown(c, [b"never-seen", b"hot-1", b"hot-2"], tk.chain_scaledown(now))
    assert idx.tolist() == [-1, 1, 2] and rem.tolist()[:2] == [0, 0]
    assert before.keys() == w.registry.keys()
    # an all-zero record IS the empty row
    w.put(b"hot-3", tk.Record(0, [], [], 0))
    assert w.get(b"hot-3") is None and w.resolve([b"hot-3"])[1].tolist() == [-1]


def test_two_entries_of_one_record_are_refused_and_two_unknown_ids_are_not(chain):
    w0, now = chain
    w = copy.deepcopy(w0)
    prm = jm.params(CHAIN_SELF, now)
    e = np.concatenate([old_row(now, r) for r in range(3)])
    with pytest.raises(InvalidEntries):
        w.janitor(e, [b"hot-4", b"m120", b"hot-4"], prm)
    assert w.registry == w0.registry
    out = w.janitor(e, [b"ghost", b"ghost", b"hot-4"], prm, dry=True)
    assert out[0].tolist() == [-1, -1, 4] and out[1].tolist()[:2] == [JAN_REMOVED, JAN_REMOVED]


def test_the_scale_down_reads_the_record_the_cache_loop_just_edited(chain):
    w0, now = chain
    prm, dp = jm.params(CHAIN_SELF, now), tk.chain_scaledown(now)
    hot = list(range(6))
    e, keys = tk.chain_entries(w0, now, hot, recent=(2,))
    w = copy.deepcopy(w0)
    idx, actions, edits, cands, crow, removed, info = w.janitor(e, keys, prm, scaledown=dp)
    assert crow.tolist() == [5, 4, 3, 2, 1, 0] and info["n_candidates"] == 6          # oldest first: the last row leads
    assert actions.tolist() == [JAN_IN_ORDER, JAN_IN_ORDER, JAN_REGISTERED, JAN_IN_ORDER, JAN_IN_ORDER, JAN_IN_ORDER]
    assert removed.tolist() == [1, 1, 1, 0, 1, 1]                                      # hot-2: its copy was just registered anew
    assert dict(w.get(b"hot-2").loaded)[CHAIN_SELF] == now - 1000
    # on the registry as it was BEFORE the run the same candidate would go: the chain is not the scale-down in front of the apply
    stale = copy.deepcopy(w0)
    _, early = stale.scaledown(cands, [b"hot-%d" % hot[r] for r in crow], dp)
    assert early.tolist() == [1, 1, 1, 1, 1, 1]
    with pytest.raises(InvalidEntries):
        copy.deepcopy(w0).janitor(e, keys, prm, dry=True, scaledown=dp)
    with pytest.raises(InvalidEntries):
        copy.deepcopy(w0).janitor(e, keys, prm, scaledown=tk.chain_scaledown(now, self_pod=CHAIN_SELF + 1))


def test_a_budget_takes_the_first_candidate_and_refuses_the_second(chain):
    w0, now = chain
    prm = jm.params(CHAIN_SELF, now)
    e, keys = tk.chain_entries(w0, now, [0, 1, 2], weight=100)
    e["weight"] = [100, 40, 10]                                                        # candidates, oldest first: 10, 40, 100
    out = copy.deepcopy(w0).janitor(e, keys, prm, scaledown=tk.chain_scaledown(now, cap=1000))   # maxWeight 50
    assert out[5].tolist() == [1, 1, 0]       # the first always (removedCount == 0), 40 <= 50 - 10, then 100 > 0
    out = copy.deepcopy(w0).janitor(e, keys, prm, scaledown=tk.chain_scaledown(now, cap=600))    # maxWeight 30
    assert out[5].tolist() == [1, 0, 0]       # the first is taken, the second refused: 40 > 30 - 10
    out = copy.deepcopy(w0).janitor(e, keys, prm, scaledown=tk.chain_scaledown(now, cap=10_000_000))
    assert out[5].tolist() == [1, 1, 1]


def test_a_conc_row_follows_its_candidate_not_its_position(chain):
    w0, now = chain
    prm, dp = jm.params(CHAIN_SELF, now), tk.chain_scaledown(now)
    e, keys = tk.chain_entries(w0, now, [0, 1, 2, 3])
    conc = tk.conc_rows(4, queued=(0,))                                                # INPUT row 0 has two queued requests
    out = copy.deepcopy(w0).janitor(e, keys, prm, scaledown=dp, conc=conc, dyn_const=60_000)
    assert out[4].tolist() == [3, 2, 1, 0] and out[5].tolist() == [1, 1, 1, 0]        # ... which is the LAST candidate
    perm = [2, 0, 3, 1]                                                                # the rows in another order: conc moves with them
    e2, k2, c2 = e[perm].copy(), [keys[i] for i in perm], conc[perm]
    e2["last_used"] = e["last_used"]                                                   # (MRU first again: the times stay in place)
    out2 = copy.deepcopy(w0).janitor(e2, k2, prm, scaledown=dp, conc=c2, dyn_const=60_000)
    kept = [k2[r] for r, x in zip(out2[4], out2[5]) if not x]
    assert kept == [b"hot-0"]
    with pytest.raises(InvalidEntries):
        copy.deepcopy(w0).janitor(e, keys, prm, conc=conc)


def test_the_chain_recipe_gives_the_candidate_counts_the_gpu_file_asks_for(chain):
    w0, now = chain
    prm, dp = jm.params(CHAIN_SELF, now), tk.chain_scaledown(now)
    for k in (0, 1, 63, 64, 65):
        e, keys = tk.chain_entries(w0, now, list(range(k)), recent=(1, 7))
        out = copy.deepcopy(w0).janitor(e, keys, prm, scaledown=dp)
        assert out[6]["n_candidates"] == k == len(out[5]) and (k < 2 or 0 < int(out[5].sum()) < k)
