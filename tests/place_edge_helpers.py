"""Shared by tests/test_place_edges.py (CPU), tests/test_place_edges_gpu.py and the pod-axis pair tests/test_shard_edges_premise.py
(CPU) / tests/test_shard_edges_gpu.py: the committed vectors of the load-target edge cases (tests/golden/ref_place_edges.npz), the
Python restatement's decisions in the device's output format, and the sharded commit's slice rule."""
import os

import numpy as np

from modelmesh_amd import _lib
from oracle import bind as ob
from oracle import py_oracle as po
from tests import ref_fleets as rf

GOLDEN_PLACE_EDGES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_place_edges.npz")
NAMES = [str(n) for n in np.load(GOLDEN_PLACE_EDGES)["names"]]
M64 = (1 << 64) - 1


def audit_hash(order, shortlist, remaining):
    """The audit hash of a shortlist (csrc/wave.hpp: audit_mul / audit_term) and its survivor count."""
    pos = {p: i for i, p in enumerate(order)}
    words = {}
    for c in shortlist:
        words[pos[c] >> 6] = words.get(pos[c] >> 6, 0) | (1 << (pos[c] & 63))

    def mul(w):
        x = ((w + 1) * 0x9E3779B97F4A7C15) & M64
        x ^= x >> 29
        x = (x * 0xBF58476D1CE4E5B9) & M64
        x ^= x >> 32
        return x | 1
    h = 0
    for w, b in words.items():
        h = (h + b * mul(w)) & M64
    return ((h ^ (h >> 32)) & 0xFFFFFFFF) ^ ((remaining * 0x9E3779B1) & 0xFFFFFFFF)


def n_words(fleet):
    """W: the 64-bit words of a rank-ordered bitmap of the fleet's table."""
    return max(-(-fleet.n_pods // 64), 1)


def slice_owner(fleet, G):
    """The sharded commit's slice rule (mmp_shard_commit_dev): Wl = ceil(W / G) words per shard, position p belongs to (p >> 6) // Wl."""
    wl = -(-n_words(fleet) // G)
    return lambda p: (p >> 6) // wl


def shard_counts(fleet):
    """The shard counts the pod-axis edge tests run a case at: one word has nothing to cut (1 and 2 — more shards only add empty
    slices); otherwise 1, 2, 3, 8 (which leaves trailing slices empty up to 7 words) and one shard per word."""
    W = n_words(fleet)
    return [1, 2] if W == 1 else sorted({1, 2, 3, 8, W})


def excluded_pods(fleet, r, extra):
    """The instances of the table that request row r already excludes: its own exclusions first, then its model's entries."""
    m = fleet.models[r["model"]]
    own = [int(x) for x in extra[r["extra_off"]: r["extra_off"] + r["n_extra"]]]
    ents = [int(x) for x in fleet.ent_pod[m["ent_off"]: m["ent_off"] + m["n_loaded"] + m["n_failed"]]]
    return [p for p in own + ents if 0 <= p < fleet.n_pods]


def py_place(fleet, reqs, extra):
    """(order, mmp_place_out rows) as oracle/py_oracle.py decides them."""
    P, T = fleet.n_pods, fleet.n_types
    mesh = po.Mesh(fleet.min_space_units, fleet.min_churn_age_ms, fleet.now)
    pods = rf.py_pods(fleet)
    order = mesh.sorted_cluster_state(pods)
    live = {i for i in range(P) if fleet.pods["flags"][i] & 2}
    rs = set(int(x) for x in fleet.replaced_rs)
    al = ob.unpack_bitmap(fleet.allowed, P) if T else None
    pf = ob.unpack_bitmap(fleet.prefer, P) if T else None
    sets = {}
    out = np.zeros(len(reqs), dtype=_lib.PLACE_OUT)
    for i, r in enumerate(reqs):
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
        out[i] = (chosen, best, len(shortlist), audit_hash(order, shortlist, remaining) if shortlist else 0)
    return np.array(order, np.int32), out
