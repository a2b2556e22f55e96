"""CPU: what tests/test_shard_edges_gpu.py rests on.  A test of the pod-axis shard kernels (modelmesh_amd/csrc/shard_kernels.hpp) is
worth little if every decision of its cases sits inside slice 0, so this file asserts — from the committed load-target edge cases
(tests/ref_fleets.py:place_edge_cases, tests/golden/ref_place_edges.npz) and oracle/py_oracle.py alone — that the cases put their
thresholds ACROSS slices.  The walk is the loop of tests/place_edge_helpers.py:py_place with each row's shortlist kept as rank
positions; the slice rule is the sharded commit's: with W = ceil(P / 64) words and G shards, Wl = ceil(W / G) and the owner of
position p is (p >> 6) // Wl.  The floors are the counts measured with exactly this loop on the committed cases."""
import numpy as np
import pytest

from oracle import bind as ob
from oracle import py_oracle as po
from tests import ref_fleets as rf
from tests.place_edge_helpers import GOLDEN_PLACE_EDGES, NAMES, audit_hash, excluded_pods, n_words
from tests.place_edge_helpers import slice_owner as owner_fn
from tests.test_ref_vectors import expected_audit


def walk(fleet, reqs, extra):
    """Per request row what oracle/py_oracle.py decides, in rank positions: sl (the shortlist, in list order), remaining, chosen,
    best0 (the first eligible instance), bestpos (the final best instance), selfpos, case ('simple' / 'a' / 'b': how the final best
    instance was found)."""
    P, T = fleet.n_pods, fleet.n_types
    mesh = po.Mesh(fleet.min_space_units, fleet.min_churn_age_ms, fleet.now)
    pods = rf.py_pods(fleet)
    order = mesh.sorted_cluster_state(pods)
    pos = {p: i for i, p in enumerate(order)}
    live = {i for i in range(P) if fleet.pods["flags"][i] & 2}
    rs = set(int(x) for x in fleet.replaced_rs)
    al = ob.unpack_bitmap(fleet.allowed, P) if T else None
    pf = ob.unpack_bitmap(fleet.prefer, P) if T else None
    sets, rows = {}, []
    for r in reqs:
        m = fleet.models[r["model"]]
        t = int(m["type"])
        if t not in sets:
            sets[t] = (set(int(p) for p in np.nonzero(al[t])[0]) if T and fleet.has_allowed[t] else None,
                       set(int(p) for p in np.nonzero(pf[t])[0]) if T and fleet.has_prefer[t] else None)
        ents = fleet.ent_pod[m["ent_off"]: m["ent_off"] + m["n_loaded"] + m["n_failed"]]
        loaded, failed = set(int(x) for x in ents[: m["n_loaded"]]), set(int(x) for x in ents[m["n_loaded"]:])
        tried = set(int(x) for x in extra[r["extra_off"]: r["extra_off"] + r["n_extra"]])
        fresh = dict(lru_time=int(r["fresh_lru"]), capacity=int(r["fresh_capacity"]), used=int(r["fresh_used"]), count=int(r["fresh_count"]),
                     rpm=int(r["fresh_rpm"]))
        chosen, best, shortlist, remaining = po.get_next(mesh, pods, order, live, rs, sets[t][0], sets[t][1], [tried, loaded, failed],
                                                         int(r["self_pod"]), bool(r["flags"] & 1), fresh, int(r["last_used"]), int(r["pick"]))
        excl = tried | loaded | failed
        first = next((p for p in order if p in live and p not in excl and (sets[t][0] is None or p in sets[t][0])
                      and not (rs and pods[p]["replica_set"] >= 0 and pods[p]["replica_set"] in rs)), None)
        sl = [pos[c] for c in shortlist]
        prefer = sets[t][1]
        case = "simple"
        if shortlist and prefer is not None and first is not None and first not in prefer:
            if pos[best] != pos[first]:
                case = "a"  # the best instance was re-designated (:4836-4841)
            elif sl and sl[0] != pos[first]:
                case = "b"  # the first instance is not in its own list (:4867-4877)
        rows.append(dict(chosen=chosen, sl=sl, remaining=remaining, best0=pos[first] if first is not None else -1,
                         bestpos=pos.get(best, -1), selfpos=pos.get(int(r["self_pod"]), -1), case=case))
    return order, rows


@pytest.fixture(scope="module")
def walks():
    cases = {c[0]: c[1:] for c in rf.place_edge_cases()}
    return cases, {name: walk(cases[name][0], cases[name][2], cases[name][3]) for name in NAMES}


def pair_rows(name):
    return sorted({i for p in rf.place_edge_meta(name)["pairs"] for i in p[:2]})


# (case, G) -> engineered pairs whose two rows' lists END in different slices: the threshold decides whether the walk enters the next one
PAIRS_END_APART = {("edge_breaks_full65", 2): 48, ("edge_breaks_full700", 2): 48, ("edge_breaks_mixed200", 2): 48,
                   ("edge_breaks_full200c", 2): 3, ("edge_breaks_open200", 2): 4, ("edge_breaks_open200", 8): 14}
# (case, G) -> (pair rows whose list spans two or more slices, pair rows): survivors, pick and the owner prefix cross shards
PAIR_ROWS_SPANNING = {("edge_rpm_200", 2): (91, 100), ("edge_rpm_65c", 2): (3, 6)}


@pytest.mark.parametrize("name,G", sorted(PAIRS_END_APART))
def test_pairs_end_in_different_slices(walks, name, G):
    cases, w = walks
    own = owner_fn(cases[name][0], G)
    rows = w[name][1]
    n = sum(1 for a, b, _ in rf.place_edge_meta(name)["pairs"]
            if rows[a]["sl"] and rows[b]["sl"] and own(max(rows[a]["sl"])) != own(max(rows[b]["sl"])))
    print(name, "G", G, "pairs whose lists end in different slices:", n)
    assert n >= PAIRS_END_APART[(name, G)], (name, G, n)


@pytest.mark.parametrize("name,G", sorted(PAIR_ROWS_SPANNING))
def test_pair_rows_span_slices(walks, name, G):
    cases, w = walks
    own = owner_fn(cases[name][0], G)
    rows, pr = w[name][1], pair_rows(name)
    n = sum(1 for i in pr if rows[i]["sl"] and own(min(rows[i]["sl"])) != own(max(rows[i]["sl"])))
    print(name, "G", G, "pair rows whose list spans two or more slices:", n, "of", len(pr))
    want, of = PAIR_ROWS_SPANNING[(name, G)]
    assert len(pr) == of and n >= want, (name, G, n, len(pr))


def test_lists_start_behind_slice_0(walks):
    cases, w = walks
    name = "edge_breaks_open200"
    own = owner_fn(cases[name][0], 2)
    rows, pr = w[name][1], set(pair_rows(name))
    behind = [i for i, r in enumerate(rows) if r["sl"] and own(r["sl"][0]) != 0]
    print(name, "rows whose list starts in a slice other than 0:", len(behind), "pair rows among them:", len(pr & set(behind)))
    assert len(behind) >= 184 and len(pr & set(behind)) >= 35, (len(behind), len(pr & set(behind)))


def test_eight_shards_leave_slices_empty(walks):
    cases, _ = walks
    small = [name for name in NAMES if n_words(cases[name][0]) < 8]
    assert len(small) >= 14, small  # every case but the 700-instance one
    for name in small:
        W = n_words(cases[name][0])
        wl = -(-W // 8)
        empty = [g for g in range(8) if min(W, g * wl + wl) - min(W, g * wl) == 0]
        assert empty, name


def test_rpm_64_has_rows_on_which_the_rule_filters_every_entry(walks):
    """The row class of the one difference the load-target tier found: the reference stops its filter at one survivor (:4975-4977), the
    entry it never reached, so the row has a target and a hash built with remaining = 1; a filter that is applied to EVERY entry —
    which is how the device states the rule (RpmRule in place_kernel.hpp) — leaves nothing."""
    cases, w = walks
    name = "edge_rpm_64"
    fleet, _, reqs, extra = cases[name]
    ref = np.load(GOLDEN_PLACE_EDGES)[f"{name}/place"]
    chosen, n_cand, want_hash = expected_audit(reqs, ref)
    order, rows = w[name]
    mesh = po.Mesh(fleet.min_space_units, fleet.min_churn_age_ms, fleet.now)
    pods = rf.py_pods(fleet)
    found = []
    for i, (r, row) in enumerate(zip(reqs, rows)):
        if len(row["sl"]) < 2 or row["case"] == "b":
            continue
        ago = mesh.age(int(r["last_used"]))
        if not ago < 5 * 86_400_000:
            continue
        # the loads the list carries (py_oracle.get_next): the best entry's own (the fresh row if it is the caller), the first
        # entry's record for the caller's entry, the caller's fresh row for every other
        bestpod, selfpod = order[row["bestpos"]], int(r["self_pod"])
        loads = []
        for k, p in enumerate(row["sl"]):
            pod = order[p]
            if k == 0:
                loads.append(int(r["fresh_rpm"]) if pod == selfpod and row["bestpos"] == row["best0"] and row["case"] == "simple"
                             else pods[bestpod]["rpm"])
            elif pod == selfpod:
                loads.append(pods[order[row["best0"]]]["rpm"])
            else:
                loads.append(int(r["fresh_rpm"]))
        lo = max(100, min(loads))
        m11, m15, m3, m4 = po._d2i(1.1 * lo), po._d2i(1.5 * lo), po._i(lo * 3), po._i(lo * 4)

        def nulls(rpm):
            return rpm >= 100 and ((ago < -1000 and rpm > m11) or (ago < 5000 and rpm > m15) or (ago < 720_000 and rpm > m3)
                                   or (ago < 86_400_000 and rpm > m4))
        if all(nulls(x) for x in loads):
            found.append(i)
            assert row["remaining"] == 1 and row["chosen"] == order[row["sl"][-1]], (i, row)  # the oracle's loop stopped at the last entry
            assert chosen[i] >= 0 and n_cand[i] == len(row["sl"]), (i, ref[i])
            assert want_hash[i] == audit_hash(order, [order[p] for p in row["sl"]], 1), (i, ref[i])
    print(name, "rows on which the rpm rule filters every entry:", len(found), "first:", found[:3])
    assert len(found) >= 1


@pytest.mark.parametrize("name", ["edge_rpm_200", "edge_rpm_65c"])
def test_case_b_lists_whose_every_candidate_is_filtered(walks, name):
    """The same row class in case (b), where the candidates carry their own rpm (:4875) and the shards count the survivors per slice."""
    cases, w = walks
    fleet, _, reqs, extra = cases[name]
    ref = np.load(GOLDEN_PLACE_EDGES)[f"{name}/place"]
    chosen, n_cand, want_hash = expected_audit(reqs, ref)
    order, rows = w[name]
    mesh = po.Mesh(fleet.min_space_units, fleet.min_churn_age_ms, fleet.now)
    pods = rf.py_pods(fleet)
    found = []
    for i, (r, row) in enumerate(zip(reqs, rows)):
        ago = mesh.age(int(r["last_used"]))
        if row["case"] != "b" or len(row["sl"]) < 2 or not ago < 5 * 86_400_000:
            continue
        loads = [pods[order[p]]["rpm"] for p in row["sl"]]
        lo = max(100, min(loads))
        m11, m15, m3, m4 = po._d2i(1.1 * lo), po._d2i(1.5 * lo), po._i(lo * 3), po._i(lo * 4)
        if all(x >= 100 and ((ago < -1000 and x > m11) or (ago < 5000 and x > m15) or (ago < 720_000 and x > m3)
                             or (ago < 86_400_000 and x > m4)) for x in loads):
            found.append(i)
            assert row["remaining"] == 1 and row["chosen"] == order[row["sl"][-1]], (i, row)
            assert chosen[i] >= 0 and n_cand[i] == len(row["sl"]), (i, ref[i])
            assert want_hash[i] == audit_hash(order, [order[p] for p in row["sl"]], 1), (i, ref[i])
    print(name, "case (b) rows on which the rpm rule filters every candidate:", len(found), "first:", found[:3])
    assert len(found) >= 1


def test_report_what_crosses_slices_beyond_the_floors(walks):
    """No floor: the counts docs/PARITY.md quotes for the combinations the cases may or may not pin on the pod axis."""
    cases, w = walks
    total = {}
    for name in NAMES:
        fleet = cases[name][0]
        W = n_words(fleet)
        if W < 2:
            continue
        own = owner_fn(fleet, 2)
        tier = name.split("_")[1]
        rows = w[name][1]
        a = sum(1 for r in rows if r["case"] == "a" and own(r["bestpos"]) != own(r["best0"]))
        b = sum(1 for r in rows if r["case"] == "b" and r["sl"] and own(r["sl"][0]) != own(r["best0"]))
        s = sum(1 for r in rows if r["selfpos"] >= 0 and r["bestpos"] >= 0 and own(r["selfpos"]) != own(r["bestpos"]))
        print(f"{name}: G = 2: case (a) with the preferred instance in another slice than the first: {a}; case (b): {b}; "
              f"caller in another slice than the best instance: {s}")
        t = total.setdefault(tier, [0, 0, 0])
        t[0], t[1], t[2] = t[0] + a, t[1] + b, t[2] + s
    for tier, (a, b, s) in sorted(total.items()):
        print(f"tier {tier}: case (a) across slices {a}, case (b) across slices {b}, caller and best instance in different slices {s}")


def test_rows_with_an_excluded_instance(walks):
    """The floors tests/test_shard_edges_gpu.py pads from: at least two thirds of every case's rows carry an instance that is already
    excluded, and at least half of the pair rows of every case that has pairs."""
    cases, _ = walks
    for name in NAMES:
        fleet, _, reqs, extra = cases[name]
        has = np.array([bool(excluded_pods(fleet, r, extra)) for r in reqs])
        pr = pair_rows(name)
        print(name, "rows with an excluded instance:", int(has.sum()), "of", len(reqs), "pair rows:", int(has[pr].sum()) if pr else 0, "of", len(pr))
        assert 3 * int(has.sum()) >= 2 * len(reqs), name
        if pr:
            assert 2 * int(has[pr].sum()) >= len(pr), name
