"""Helpers shared by the parity tests."""
import numpy as np


def describe_mismatch(fleet, reqs, got, want, limit=8):
    """Human-readable dump of the first differing decisions (shows up in the GPU log)."""
    bad = np.nonzero((got["chosen"] != want["chosen"]) | (got["best"] != want["best"]) |
                     (got["n_candidates"] != want["n_candidates"]) | (got["hash"] != want["hash"]))[0]
    lines = [f"{len(bad)} of {len(reqs)} decisions differ"]
    for i in bad[:limit]:
        r = reqs[i]
        m = fleet.models[r["model"]]
        lines.append(
            f"  req {i}: model={r['model']} type={m['type']} k={m['n_loaded']} f={m['n_failed']} self={r['self_pod']} "
            f"flags={r['flags']} n_extra={r['n_extra']} last_used={r['last_used']} pick={r['pick']}\n"
            f"     got  chosen={got[i]['chosen']} best={got[i]['best']} n={got[i]['n_candidates']} hash={got[i]['hash']:#x}\n"
            f"     want chosen={want[i]['chosen']} best={want[i]['best']} n={want[i]['n_candidates']} hash={want[i]['hash']:#x}")
    return "\n".join(lines)


def assert_same_decisions(fleet, reqs, got, want):
    same = (np.array_equal(got["chosen"], want["chosen"]) and np.array_equal(got["best"], want["best"]) and
            np.array_equal(got["n_candidates"], want["n_candidates"]) and np.array_equal(got["hash"], want["hash"]))
    assert same, describe_mismatch(fleet, reqs, got, want)


def covered_share(s, fleet, orc, reqs, extra):
    """Share of the requests the recorded shortlists answer: no position of the request's own inside [lo, hi) of its type's
    valid rows (either bit: an upper bound on the misses is enough for the assertion below)."""
    rows = s.shortlists()
    pos_of = np.empty(fleet.n_pods, np.int64)
    pos_of[orc.order] = np.arange(len(orc.order))
    m = fleet.models[reqs["model"]]
    t = np.clip(m["type"], 0, max(fleet.n_types - 1, 0))
    lo = np.minimum(rows["lo"][2 * t], rows["lo"][2 * t + 1])
    hi = np.maximum(rows["hi"][2 * t], rows["hi"][2 * t + 1])
    ok = (rows["valid"][2 * t] & rows["valid"][2 * t + 1]).astype(bool) & (t < 12)
    sp = np.where(reqs["self_pod"] >= 0, pos_of[np.maximum(reqs["self_pod"], 0)], -1)
    ok &= ~((sp >= lo) & (sp < hi))
    tot = m["n_loaded"] + m["n_failed"]
    ok &= tot <= 6
    for j in range(6):
        p = pos_of[fleet.ent_pod[np.minimum(m["ent_off"] + j, len(fleet.ent_pod) - 1)]]
        ok &= ~((tot > j) & (p >= lo) & (p < hi))
    for j in range(4):
        has = reqs["n_extra"] > j
        p = pos_of[extra[np.minimum(reqs["extra_off"] + j, max(len(extra) - 1, 0))]] if len(extra) else np.zeros(len(reqs), np.int64)
        ok &= ~(has & (p >= lo) & (p < hi))
    ok &= reqs["n_extra"] <= 4
    return float(ok.mean())
