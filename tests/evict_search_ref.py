"""What mmp_evict_batch must answer on a deque too long to walk in Python, and the cases tests/test_evict_search_edges_gpu.py
sends to the device.  `walk` (tests/test_evict_search_gpu.py) is the definition.  `linear_rows` states the same two rules on whole
arrays — the insert position from ONE compare of every stamp, the victim count from ONE compare of every merged suffix sum — with
no search, no prefix table kept between requests and no assumption that the deque is in time order: it is right on unordered
deques and on negative weights, where evict_search_kernel must not search.  tests/test_evict_search_ref.py holds it to `walk` on
the CPU on every case below that is short enough to walk.

A case is (caches, reqs): caches = [(last_used, weight, capacity)], reqs = [(cache, weight, last_used)] — what `check` of
tests/test_evict_search_gpu.py takes.  The capacity belongs to the cache, so a deque asked under several capacities is loaded
once per capacity (`fan`)."""
import numpy as np

from tests.test_evict_search_gpu import CHUNK, NOW, T0, TEAM, walk  # noqa: F401  (walk: imported, not copied)

W31 = 2**31 - 1
MIXED_LENGTHS = [0, 1025, 0, 0, 1, 1024, 2049, 16, 4914, 0]
DEPTH_LENGTHS = [17**3 - 1, 17**3, 17**3 + 1, 65536, 17**4 - 1, 17**4, 17**4 + 1]
EXHAUSTIVE = 290
WIDE_LENGTHS = [256 * CHUNK, 256 * CHUNK + 1, 257 * CHUNK + 1]  # 256, 257 and 258 chunks: the carry loop's second trip needs 258
NAMED_CAPS = (0, -1, 2**62, -2**62, -2**63, 2**63 - 1)
WALKABLE = 5000  # entries up to which the CPU test walks a deque in Python


def linear_rows(lu, wt, w, ts, caps):
    """one insert (weight w, stamp ts) on the deque under each capacity of `caps`: [(insert_pos, n_victims, self_evicted,
    weighted_size, oldest_time)]"""
    lu, wt = np.asarray(lu, np.int64), np.asarray(wt, np.int64)
    ts, E = int(ts) or NOW, len(lu)
    le = np.nonzero(lu <= ts)[0]  # every stamp compared: the walk from the tail stops behind the LAST of these
    pos = int(le[-1]) + 1 if len(le) else 0
    merged = np.concatenate([wt[:pos], [int(w)], wt[pos:]]).astype(np.int64)
    stamps = np.concatenate([lu[:pos], [ts], lu[pos:]]).astype(np.int64)
    left = int(merged.sum()) - np.concatenate([[0], np.cumsum(merged)])  # left[v]: weightedSize after v polls, v = 0 .. E + 1
    rows = []
    for cap in caps:
        hit = left <= int(cap)
        v = int(hit.argmax())  # the first index at which the size fits; none: the deque is polled empty
        if not hit[v]:
            v = E + 1
        rows.append((pos, v, int(v > pos), int(left[v]), int(stamps[v]) if v <= E else -1))
    return rows


def linear(lu, wt, cap, w, ts):
    """`walk`'s signature"""
    return linear_rows(lu, wt, w, ts, [cap])[0]


def suffix_caps(wt, pos, w):
    """cap[v] = the weight `v` polls leave of the deque with `w` merged in at pos, v = 0 .. E + 1: with positive weights the
    capacity under which exactly v entries are victims"""
    merged = [int(x) for x in wt[:pos]] + [int(w)] + [int(x) for x in wt[pos:]]
    return [int(x) for x in sum(merged) - np.concatenate([[0], np.cumsum(np.array(merged, dtype=np.int64))])]


def searchable(lu, wt):
    """what the scan must find: in time order and no negative weight"""
    return bool((np.diff(np.asarray(lu, np.int64)) >= 0).all() and (np.asarray(wt) >= 0).all())


def expected_info(caches, reqs, search_from):
    """(n_above, n_searchable, rows_searched) of a load and one batch on it, from the inputs alone"""
    above = [len(c[0]) > search_from for c in caches]
    ok = [a and searchable(c[0], c[1]) for a, c in zip(above, caches)]
    return sum(above), sum(ok), sum(1 for k, w, _ in reqs if 0 <= k < len(caches) and ok[k] and w >= 0)


def stamps(E, base=T0):
    return base + 10 * np.arange(E, dtype=np.int64)


def stamp_at(lu_base, pos):
    """a stamp that `stamps` puts in front of entry pos (0: older than the head, E: younger than the tail)"""
    return int(lu_base) + 10 * pos - 5


def weights(E, k=0):
    """E positive weights, a pattern of period 5 + k that starts somewhere else for every k"""
    return (1 + ((3 + k) * np.arange(E) + 2 * k) % (5 + k)).astype(np.int32)


def fan(lu, wt, asks):
    """asks = [(weight, stamp, capacity)] on ONE deque -> (caches, reqs), a cache per distinct capacity in order of appearance"""
    at = {}
    reqs = [(at.setdefault(int(cap), len(at)), int(w), int(ts)) for w, ts, cap in asks]
    return [(lu, wt, cap) for cap in at], reqs


# ---- a. caches of different lengths in one load -------------------------------------------------------------------------------
def mixed_store():
    """[(lu, wt)] of MIXED_LENGTHS; every stamp of cache k + 1 is older than every stamp of cache k"""
    n = len(MIXED_LENGTHS)
    return [(stamps(E, T0 + (n - k) * 1_000_000), weights(E, k)) for k, E in enumerate(MIXED_LENGTHS)]


def mixed_cases():
    """15 loads of mixed_store: (which position, which victim count) picks every cache's capacity; every load asks every cache
    at the head, the middle and the tail, and two requests name no cache.  -> [(label, caches, reqs, [(request, victims)])]"""
    store, w, out = mixed_store(), 3, []
    places = {"head": lambda E: 0, "middle": lambda E: E // 2, "tail": lambda E: E}
    targets = {"0": lambda p, E: 0, "1": lambda p, E: 1, "pos": lambda p, E: p, "pos+1": lambda p, E: p + 1, "E+1": lambda p, E: E + 1}
    for pn, place in places.items():
        for tn, target in targets.items():
            caches, reqs, named = [], [], []
            for k, (lu, wt) in enumerate(store):
                E = len(lu)
                v = target(place(E), E)
                caches.append((lu, wt, suffix_caps(wt, place(E), w)[v]))
                for qn, q in places.items():
                    if qn == pn:
                        named.append((len(reqs), v))
                    reqs.append((k, w, stamp_at(lu[0] if E else T0, q(E))))
                if k == 4:
                    reqs.append((-1, w, T0))
            reqs.append((len(store), w, T0))
            out.append((f"{pn}/{tn}", caches, reqs, named))
    return out


# ---- b. search depth ------------------------------------------------------------------------------------------------------------
def probe_indices(E, seed):
    """the first step's probes lo + (t + 1) * s - 1, s = E // 17 + 1, one to either side of each, the ends, 64 random: as insert
    positions 0 .. E; the victim search over [1, E + 1] probes (t + 1) * s, the right-hand neighbours"""
    s = E // (TEAM + 1) + 1
    named = {(t + 1) * s - 1 + d for t in range(TEAM) for d in (-1, 0, 1)} | {0, 1, E - 1, E}
    rnd = np.random.default_rng(seed).integers(0, E + 1, 64)
    return sorted({int(j) for j in named | set(rnd.tolist()) if 0 <= j <= E})


def depth_case(E):
    """one deque of E entries: inserts at probe_indices, and for each the capacities that put the victim count on those same
    indices (and on E + 1).  -> (caches, reqs, victims per request).  The capacity that leaves v victims is P-dependent only
    through which side of the insert v lies: T + w - P[v] up to pos, T - P[v - 1] beyond, so two caches per index serve all."""
    lu, wt, w = stamps(E), weights(E), 3
    idx = probe_indices(E, E)
    P = np.concatenate([[0], np.cumsum(wt.astype(np.int64))])
    T = int(P[E])
    asks, victims = [], []
    for p in idx:
        for v in idx + [E + 1]:
            asks.append((w, stamp_at(T0, p), T + w - int(P[v]) if v <= p else T - int(P[v - 1])))
            victims.append(v)
    return fan(lu, wt, asks) + (victims,)


def exhaustive_case(E=EXHAUSTIVE):
    """every insert position 0 .. E; for each the victim counts 0, 1, pos, pos + 1, E + 1 and the capacity one to either side"""
    lu, wt, w = stamps(E), weights(E), 3
    asks = []
    for p in range(E + 1):
        caps = suffix_caps(wt, p, w)
        asks += [(w, stamp_at(T0, p), caps[v] + d) for v in sorted({0, 1, p, p + 1, E + 1}) for d in (0, -1, 1)]
    return fan(lu, wt, asks)


# ---- c. more than 256 chunks --------------------------------------------------------------------------------------------------
def wide_cases():
    """WIDE_LENGTHS in one load, every weight 2^31 - 1; one load per k, the capacity k entries' weight: the victim counts land in
    each cache's last chunk (k = 600: in the middle of it).  -> [(k, caches, reqs)]"""
    out = []
    for k in (0, 1, 2, 3, 600):
        caches = [(stamps(E), np.full(E, W31, np.int32), k * W31) for E in WIDE_LENGTHS]
        reqs = [(c, W31, stamp_at(T0, p)) for c, E in enumerate(WIDE_LENGTHS)
                for p in sorted({0, CHUNK - 1, CHUNK, 256 * CHUNK - 1, 256 * CHUNK, E // 2, E}) if p <= E]
        out.append((k, caches, reqs))
    return out


# ---- d. caches the search must leave to the walk ----------------------------------------------------------------------------
def defect_cases():
    """{name: (defective deque (lu, wt), whether it stays searchable)}: one defect each, at a chunk edge"""
    def deque(E, edit):
        lu, wt = stamps(E), weights(E)
        edit(lu, wt)
        return lu, wt

    def older(j):  # entry j one tick older than entry j - 1, younger than entry j - 2
        def edit(lu, wt):
            lu[j] = lu[j - 1] - 1
        return edit

    def negative(j):
        def edit(lu, wt):
            wt[j] = -1
        return edit

    def equal(j):
        def edit(lu, wt):
            lu[j] = lu[j - 1]
        return edit
    E = 2 * CHUNK + 1
    return {"order at 1023/1024": (deque(E, older(CHUNK)), False), "order at 2047/2048": (deque(E, older(2 * CHUNK)), False),
            "negative first in the third chunk": (deque(E + 11, negative(2 * CHUNK)), False),
            "negative last": (deque(E, negative(E - 1)), False),
            "equal stamps at 1023/1024": (deque(E, equal(CHUNK)), True), "equal stamps at 2047/2048": (deque(E, equal(2 * CHUNK)), True)}


def defect_load(name):
    """the defective cache first, a clean one beside it, requests around the defect on both -> (caches, reqs)"""
    (lu, wt), _ = defect_cases()[name]
    E = len(lu)
    clean = (stamps(E), weights(E, 1))
    at = [j for j in (CHUNK, 2 * CHUNK, E - 1) if lu[j] != stamps(E)[j] or wt[j] < 0][0]
    ts = [T0 - 5, int(lu[at - 1]) - 1, int(lu[at - 1]), int(lu[at]), int(lu[at]) + 5, stamp_at(T0, E // 2), stamp_at(T0, E), 0]
    caches, reqs = [], []
    for cap_of in (lambda x: int(x.sum()) // 2, lambda x: int(x[at:].sum()) + 1, lambda x: 0):
        k = len(caches)
        caches += [(lu, wt, cap_of(wt.astype(np.int64))), (clean[0], clean[1], cap_of(clean[1].astype(np.int64)))]
        reqs += [(k + c, w, t) for t in ts for c in (0, 1) for w in (3, 0)]
    return caches, reqs


# ---- e. values ----------------------------------------------------------------------------------------------------------------
def value_case(E):
    """runs of zero weights at the head, in the middle and at the tail; request weights 0 and 3 at the head, the middle and the
    tail; capacities that put the victim boundary in front of, inside and behind each run, the total and one to either side of
    it, and NAMED_CAPS"""
    lu, wt = stamps(E), weights(E)
    m = E // 2
    for a, b in ((0, 4), (m - 2, m + 2), (E - 4, E)):
        wt[a:b] = 0
    asks = []
    for w in (0, 3):
        for p in (0, m, E):
            caps = suffix_caps(wt, p, w)
            near = {v for a in (0, m - 2, E - 4) for v in range(a - 1, a + 7) if 0 <= v <= E + 1} | {E + 1}
            for cap in [caps[v] for v in sorted(near)] + [caps[0] - 1, caps[0] + 1] + list(NAMED_CAPS):
                asks.append((w, stamp_at(T0, p), cap))
    return fan(lu, wt, asks)


# ---- g. default threshold -----------------------------------------------------------------------------------------------------
def threshold_case(lengths, unordered=()):
    """caches of `lengths`, those in `unordered` with two entries swapped in mid-deque; capacity half the weight; every cache asked
    at the head, the middle, the tail and "now" -> (caches, reqs)"""
    caches, reqs = [], []
    for k, E in enumerate(lengths):
        lu, wt = stamps(E, T0 + 1000 * k), weights(E, k)
        if k in unordered:
            lu[[E // 2, E // 2 + 1]] = lu[[E // 2 + 1, E // 2]]
        caches.append((lu, wt, int(wt.sum()) // 2))
        reqs += [(k, 3, ts) for ts in (stamp_at(lu[0], 0), stamp_at(T0 + 1000 * k, E // 2), stamp_at(T0 + 1000 * k, E), 0)]
    return caches, reqs


# ---- f. call paths ----------------------------------------------------------------------------------------------------------------
def small_store():
    """eight searchable caches of 100 entries under different capacities and one out of time order"""
    caches, _ = threshold_case([100] * 9, unordered=(8,))
    return [(lu, wt, cap * (k + 1) // 5) for k, (lu, wt, cap) in enumerate(caches)]


def small_reqs(caches, n, start=0):
    """n requests on the searchable caches, a different (cache, position) each until the 808 are used up"""
    out = []
    for i in range(start, start + n):
        k, p = i % 8, (i // 8) % 101
        out.append((k, 1 + i % 4, stamp_at(caches[k][0][0], p)))
    return out


def reference(caches, reqs):
    """linear_rows on every request of a case (requests of one insert on one deque, as `fan` lays them out, share the call); a
    request that names no cache gets the zero row with oldest_time -1"""
    rows, groups = [(0, 0, 0, 0, -1)] * len(reqs), {}
    for i, (k, w, ts) in enumerate(reqs):
        if 0 <= k < len(caches):
            groups.setdefault((id(caches[k][0]), id(caches[k][1]), w, ts), []).append(i)
    for (_, _, w, ts), at in groups.items():
        lu, wt, _ = caches[reqs[at[0]][0]]
        for i, row in zip(at, linear_rows(lu, wt, w, ts, [caches[reqs[i][0]][2] for i in at])):
            rows[i] = row
    return rows
