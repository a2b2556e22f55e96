"""Operation streams for the local cache (SURVEY.md §8 rows a12 + a13) that the reference-text harness
(oracle/ref_harness/clhm_harness.cc), the C oracle (oracle/mm_evict_oracle.c) and the device (cache_replay_kernel) all replay.
Seeded; the committed vectors (tests/golden/ref_clhm.npz) carry the streams themselves, so the tests do not regenerate them.

Domain of a stream = what ModelMesh guarantees about its own cache (MM.java:748-753, :1766): an unload reserve in
(0, capacity / 10], entry weights >= 1 at all times, and the pinned unload-buffer entry is never evicted.  make_clhm_vectors.py
cuts a cache's stream where the reference itself would evict that entry (a failed unload that shrinks the capacity below the
buffer).  The edge cases further down (edge_cases(), tests/golden/ref_clhm_edges.npz) keep the same domain but are refused, not
cut, where the reference would evict that entry."""
import numpy as np

NOW = 1_760_000_000_000
CACHE_OP = np.dtype([("cache", "<i4"), ("op", "<i4"), ("key", "<i4"), ("arg", "<i4"), ("time", "<i8"), ("flag", "<i4"),
                     ("reserved", "<i4")])
UNLOADBUF_KEY = -1000000


def random_stream(seed, n_caches, n_ops, keys_per_cache=40, fail_unload=0.15):
    """Few distinct timestamps (ties are the rule: LinkedDeque.java:267), reads with older timestamps (touch = max, clhm :1358),
    weight growth after load, claims, failed unloads."""
    rng = np.random.default_rng(seed)
    caps = rng.choice([5_000, 25_600, 131_072, 400_000], n_caches).astype(np.int64)
    managed = rng.random(n_caches) < 0.6
    reserved = np.where(managed, np.minimum(rng.choice([64, 256, 2_560, 9_600], n_caches), caps // 10), -1).astype(np.int32)
    ops = np.zeros(n_ops, dtype=CACHE_OP)
    lb = {}  # a lower bound of every key's weight (negative deltas must leave it >= 1)
    for i in range(n_ops):
        c = int(rng.integers(0, n_caches))
        key = int(rng.integers(0, keys_per_cache)) + 1000 * c
        t = int(rng.choice([0, NOW - 500, NOW - 2_000, NOW - 2_000, NOW - 7_200_000, NOW + 5, NOW - int(rng.integers(0, 5000))]))
        w = int(rng.choice([1, 640, 2_560, 6_400, 30_000]))
        flag = 0
        if managed[c]:
            op = int(rng.choice([4, 4, 4, 5, 5, 6, 7, 8, 8, 9, 10, 11, 12, 1, 1]))
        else:
            op = int(rng.choice([0, 0, 0, 0, 1, 1, 2, 2, 3]))
        arg = w
        if op in (4, 12):
            arg = 1 if rng.random() < 0.7 else w
        elif op == 2:
            t = int(rng.choice([-1, -1, 0, NOW - 100]))
        elif op == 5:
            arg, flag = int(rng.choice([639, 2_559, 6_399])), int(rng.random() < 0.3)
        elif op in (6, 7):
            arg = int(rng.choice([1, 640, 6_400, 100_000]))
        elif op == 8:
            arg = int(rng.choice([-600, -1, 0, 1, 700, 20_000]))
            if arg < 0 and lb.get(key, 1) + arg < 1:
                arg = 0
        elif op == 9:
            arg, flag = int(rng.choice([640, 2_560])), int(rng.random() >= fail_unload)
        elif op == 11:
            arg = int(rng.choice([1, 640]))
        if op in (0, 4, 12, 2):
            lb[key] = min(lb.get(key, arg), arg)
        elif op in (5, 8):
            lb[key] = lb.get(key, 1) + arg
        ops[i] = (c, op, key, arg, t, flag, 0)
    return caps, reserved, ops


def kat_basic_eviction():
    """EvictionsModelMeshTest.basicEvictionTest (:36-125): capacity 131072 units, reserve 9600; models of
    6400 units registered 10 ms apart (lastUsed = now - 1 h + 10 ms * m); the 19th insert evicts myModel0, then 1, 2; re-adding
    myModel0 evicts 3; a model sized 160 MiB after its load evicts 4, 5, 6."""
    rows = []
    t0 = NOW - 3_600_000

    def load(m, t):  # ensureLoaded: placeholder (INSERTION_WEIGHT 1), predicted size, claim before the load starts, unloads complete
        rows.append((0, 4, m, 1, t, 0, 0))
        rows.append((0, 5, m, 6399, 0, 0, 0))
        rows.append((0, 7, 0, 6400, 0, 0, 0))
    for m in range(21):
        load(m, t0 + 10 * m)
        if m >= 18:
            rows.append((0, 9, 0, 6400, 0, 1, 0))  # the evicted model's unload completes
    load(0, NOW)                                  # myModel0 again: evicts 3
    rows.append((0, 9, 0, 6400, 0, 1, 0))
    load(21, NOW)                                 # predicted 50 MiB ...
    rows.append((0, 9, 0, 6400, 0, 1, 0))
    rows.append((0, 8, 21, 20480 - 6400, 0, 0, 0))  # ... sized 160 MiB after the load
    ops = np.array(rows, dtype=CACHE_OP)
    return np.array([131072], np.int64), np.array([9600], np.int32), ops


def kat_concurrent_eviction():
    """EvictionsModelMeshTest.concurrentEvictionTest (:136-200): 18 loaded, ten placeholders inserted together, then grown."""
    rows = []
    t0 = NOW - 3_600_000
    for m in range(18):
        rows += [(0, 4, m, 1, t0 + 10 * m, 0, 0), (0, 5, m, 6399, 0, 0, 0), (0, 7, 0, 6400, 0, 0, 0)]
    for m in range(18, 28):
        rows.append((0, 4, m, 1, t0 + 1000 + m, 0, 0))
    for m in range(18, 28):
        rows.append((0, 5, m, 6399, 0, 0, 0))
    return np.array([131072], np.int64), np.array([9600], np.int32), np.array(rows, dtype=CACHE_OP)


def kat_standalone_lru():
    """ModelMeshEvictionsTest (:156-280, Appendix C.2): capacity 25600, size 2560, reserve 2560; 12 sequential loads leave the
    last 9; then reads of three re-order the LRU before three more loads."""
    rows = []
    t0 = NOW - 60_000
    for m in range(12):
        rows += [(0, 4, m, 1, t0 + 10 * m, 0, 0), (0, 5, m, 2559, 0, 0, 0), (0, 9, 0, 2560, 0, 1, 0)]
    for m in (3, 4, 5):
        rows.append((0, 1, m, 0, 0, 0, 0))  # invoke: get(key) stamps now
    for m in range(12, 15):
        rows += [(0, 4, m, 1, NOW, 0, 0), (0, 5, m, 2559, 0, 0, 0), (0, 9, 0, 2560, 0, 1, 0)]
    return np.array([25600], np.int64), np.array([2560], np.int32), np.array(rows, dtype=CACHE_OP)


def head_reads():
    """A cache in use: every read is of the least recently used entry (a round-robin client), which moves the deque's head to
    its tail each time (LinkedDeque.reposition :243-255) — 30 entries, 900 reads, no insert in between; one managed, one not."""
    rows = []
    for c, op in ((0, 4), (1, 0)):
        for m in range(30):
            rows.append((c, op, 1000 * c + m, 100, NOW - 10_000 + m, 0, 0))
    for r in range(30):
        for c in (0, 1):
            for m in range(30):
                rows.append((c, 1, 1000 * c + m, 0, 0 if r % 2 else NOW + 1 + 30 * r + m, 0, 0))
    return np.array([100_000, 100_000], np.int64), np.array([2_560, -1], np.int32), np.array(rows, dtype=CACHE_OP)


def cases():
    """(name, capacities, reserves, ops)"""
    out = [("kat_basic_eviction",) + kat_basic_eviction(), ("kat_concurrent_eviction",) + kat_concurrent_eviction(),
           ("kat_standalone_lru",) + kat_standalone_lru(), ("head_reads",) + head_reads()]
    rng = np.random.default_rng(0xC1A)
    for k in range(36):
        n_caches = int(rng.choice([1, 3, 8, 24]))
        n_ops = int(rng.choice([60, 300, 1000, 1500]))
        out.append((f"stream{k:02d}",) + random_stream(9000 + k, n_caches, n_ops, keys_per_cache=int(rng.choice([12, 40, 90])),
                                                       fail_unload=float(rng.choice([0.0, 0.15, 0.4]))))
    return out


def initial_state(caps, reserved):
    """The device / oracle state the streams start from: empty caches; a managed one holds the manager's pinned entry
    (newInternalCacheEntry, MM.java:1617-1622: lastUsed = Long.MAX_VALUE, weight = the reserve)."""
    seg = [0]
    lus, wts, keys = [], [], []
    for r in reserved:
        if r >= 0:
            lus.append(np.iinfo(np.int64).max), wts.append(int(r)), keys.append(UNLOADBUF_KEY)
        seg.append(len(lus))
    return (np.array(seg, np.int32), np.array(lus, np.int64), np.array(wts, np.int32), np.array(keys, np.int32))


# ================================================ edges of the value domain ================================================
# tests/golden/ref_clhm_edges.npz (make_clhm_vectors.py --edges).  A CASE is a set of independent caches; each cache is one RUN:
# a build prefix, then one or a few probe operations.  The prefixes of a case are interleaved step by step, the probes follow,
# so the case replays in a few calls and every call boundary cuts every cache's prefix.  A PAIR is two runs that differ in
# one value by one unit, on either side of one threshold of the reference text.
EDGE_TIERS = ("lengths", "clhm", "manager", "wide")
T0 = NOW - 10_000_000
PROBE_KEY = 900_001
I32_MAX, I64_MAX, I64_MIN = 2**31 - 1, 2**63 - 1, -2**63
LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 46, 47, 48, 63, 64, 65, 127, 128, 129, 158, 159, 160, 191, 192, 193)
BIG_LENGTHS = (2045, 2046)
MASS = (1, 2, 63, 64, 65, 127, 128, 129, 130, 131, 257)
CACHE_TILE, TEAM8_SLOTS, TEAM16_SLOTS = 2048, 48, 160  # cache_kernels.hpp: kCacheTile, kTeam8Slots, kTeam16Slots
PAIR_FIELDS = ("arg", "time", "cap")
EDGE_RUN = np.dtype([("cache", "<i4"), ("tag", "<i4"), ("n_prefix", "<i4"), ("n_probe", "<i4"), ("managed", "<i4"), ("entries", "<i4")])
EDGE_PAIR = np.dtype([("a", "<i4"), ("b", "<i4"), ("field", "<i4"), ("name", "<i4"), ("alike", "<i4")])


def team_width(slots):
    """mmp_cache_replay's rule (mmplace.hip): the deque slots a cache's replay needs = its entries + the call's inserts; 8 lanes
    while slots + 1 <= 48, 16 up to 160, the wavefront up to the 2048-slot tile, beyond which the call is refused."""
    if slots + 1 > CACHE_TILE:
        return 0
    return 8 if slots + 1 <= TEAM8_SLOTS else 16 if slots + 1 <= TEAM16_SLOTS else 64


def is_insert(op):
    return op in (0, 4, 12)


class _Case:
    def __init__(self, name, tier):
        self.name, self.tier = name, tier
        self.caps, self.res, self.prefix, self.probe, self.tags, self.pairs, self.entries = [], [], [], [], [], [], []

    def run(self, tag, cap, reserved, prefix, probe, entries=-1):
        """rows are (op, key, arg, time, flag); -> the cache index of the run"""
        self.caps.append(cap), self.res.append(reserved), self.prefix.append(list(prefix)), self.probe.append(list(probe))
        self.tags.append(tag), self.entries.append(entries)
        return len(self.caps) - 1

    def pair(self, name, field, a, b, alike=False):
        """alike: the two sides cannot differ in anything the reference shows — no pair decides that comparison (the generator
        checks that too, and docs/PARITY.md lists them)"""
        self.pairs.append((a, b, PAIR_FIELDS.index(field), name, int(alike)))

    def build(self):
        rows = []
        for part in (self.prefix, self.probe):
            keyed = [(step, c, r) for c, rs in enumerate(part) for step, r in enumerate(rs)]
            rows += [(c,) + tuple(r) + (0,) for _, c, r in sorted(keyed, key=lambda t: (t[0], t[1]))]
        ops = np.array(rows, dtype=CACHE_OP) if rows else np.zeros(0, CACHE_OP)
        n_pre = sum(len(p) for p in self.prefix)
        bounds = np.unique(np.array([0, n_pre // 3, 2 * n_pre // 3, n_pre, len(ops)], np.int32))
        tag_names = sorted(set(self.tags))
        pair_names = sorted({p[3] for p in self.pairs})
        assert len(pair_names) == len(self.pairs), "pair names are unique"
        runs = np.array([(c, tag_names.index(self.tags[c]), len(self.prefix[c]), len(self.probe[c]), self.res[c] >= 0, self.entries[c])
                         for c in range(len(self.caps))], dtype=EDGE_RUN)
        pairs = np.array([(a, b, f, pair_names.index(n), k) for a, b, f, n, k in self.pairs], dtype=EDGE_PAIR)
        return {"name": self.name, "tier": self.tier, "caps": np.array(self.caps, np.int64), "reserved": np.array(self.res, np.int32),
                "ops": ops, "bounds": bounds, "n_prefix": n_pre, "runs": runs, "pairs": pairs, "tag_names": np.array(tag_names),
                "pair_names": np.array(pair_names if pair_names else [""])[: len(pair_names)]}


def _len_prefix(L, managed, order=None, tie=None):
    """L entries (keys 1..L, weight 3, lastUsed T0 + 10 i: the deque's index of key i + 1 is i) inserted in `order`; tie = (a, b):
    the entries a..b-1 share entry a's lastUsed (FIFO among equals, LinkedDeque.java:267: inserted in ascending order)"""
    lu = [T0 + 10 * i for i in range(L)]
    if tie:
        for i in range(tie[0], tie[1]):
            lu[i] = lu[tie[0]]
    return [(4 if managed else 0, i + 1, 3, lu[i], 0) for i in (range(L) if order is None else order)]


def _chunk_edges(n, tw):
    """the deque indices at which a second and a last tw-lane chunk of the cooperative loops begin"""
    return sorted({e for e in (tw, tw * ((n - 1) // tw)) if 0 < e < n})


def _length_runs(case, L, managed, inserts=True, full=True):
    P = int(managed)
    res = 64 if managed else -1
    cap = 10**9
    n = L + P  # the deque's length before the probe (the pinned entry is its tail)
    put, rem = (4, 10) if managed else (0, 3)
    k = [0]

    def order():  # in turn: ascending (every insert at the tail), descending (every insert at the head: the whole deque shifts,
        k[0] += 1  # chunk by chunk), evens up then odds down (inserts in the middle)
        return (None, list(range(L - 1, -1, -1)), list(range(0, L, 2)) + list(range(L - 1 - L % 2, 0, -2)))[k[0] % 3]
    if inserts:
        tw = team_width(n + 1)
        assert tw, (L, managed)
        at = {0: "head", L: "tail"}
        if full:
            for d in (tw - 1, tw, tw + 1):
                if 0 < d < L:
                    at.setdefault(d, f"head+{d - tw:+d}")
                if 0 < n - d < L:
                    at.setdefault(n - d, f"end-{d - tw:+d}")
        for q, what in sorted(at.items()):
            case.run(f"insert/{what}", cap, res, _len_prefix(L, managed, order()), [(put, PROBE_KEY, 3, T0 + 10 * q - 5, 0)], L)
        for e in _chunk_edges(n + 1, tw) if full else ():
            if e - 2 >= 0 and e + 2 <= L:
                case.run("insert/behind-ties", cap, res, _len_prefix(L, managed, None, (e - 2, e + 2)),
                         [(put, PROBE_KEY, 3, T0 + 10 * (e - 2), 0)], L)
    tw = team_width(n)
    where = {0: "head", L - 1: "tail"}
    for e in _chunk_edges(n, tw) if full else ():
        where.setdefault(e - 1, "edge-1"), where.setdefault(e, "edge")
    for i, what in sorted(where.items()):
        if 0 <= i < L:
            case.run(f"get/{what}", cap, res, _len_prefix(L, managed, order()), [(1, i + 1, 0, 0, 0)], L)
            case.run(f"remove/{what}", cap, res, _len_prefix(L, managed, order()), [(rem, i + 1, 0, 0, 0)], L)
    if L == 0:
        case.run("get/absent", cap, res, [], [(1, 1, 0, 0, 0)], 0)
        case.run("remove/absent", cap, res, [], [(rem, 1, 0, 0, 0)], 0)


def _lengths_cases():
    out = []
    for managed in (False, True):
        c = _Case("lengths_managed" if managed else "lengths_plain", "lengths")
        for L in LENGTHS:
            _length_runs(c, L, managed)
        out.append(c)
    c = _Case("lengths_big", "lengths")
    # 2047 slots is the most a replay takes: 2046 entries and one insert, or 2045, the pinned entry and one insert; 2046 entries
    # beside the pinned entry leave no room for an insert (reads and removals only)
    _length_runs(c, 2046, False, full=False)
    for q, what in ((0, "head"), (2045, "tail")):
        c.run(f"insert/{what}", 10**9, 64, _len_prefix(2045, True), [(4, PROBE_KEY, 3, T0 + 10 * q - 5, 0)], 2045)
    _length_runs(c, 2046, True, inserts=False, full=False)
    out.append(c)
    # one operation that evicts N entries.  Plain: N + 3 entries of weight 10 leave 5 units; a put of 10 N - 4 evicts N, of
    # 10 N - 5 evicts N - 1 (weightedSize > capacity, clhm :321).
    c = _Case("mass_plain", "lengths")
    for N in MASS:
        M = N + 3
        pre = [(0, i + 1, 10, T0 + 10 * i, 0) for i in range(M)]
        a = c.run(f"evict/{N}", 10 * M + 5, -1, pre, [(0, PROBE_KEY, 10 * N - 4, 0, 0)], M)
        b = c.run(f"evict/{N}-1", 10 * M + 5, -1, pre, [(0, PROBE_KEY, 10 * N - 5, 0, 0)], M)
        c.pair(f"weightedSize > capacity, {N} victims", "arg", b, a)
    out.append(c)
    # Managed, all victims of one evict() pending at once (insertNewEntry takes its weight off the buffer first, :134, so the
    # listener's growth never passes the reserve): the reversal of the pending run.  And the cascade: a plain put on a full
    # managed cache with a reserve of 1 — from the second victim on every entryRemoved grows the buffer by what was just
    # evicted, which evicts again inside the drain, until only the pinned entry is left, clamped to the capacity (:384-388).
    c = _Case("mass_managed", "lengths")
    for N in MASS:
        M = N + 3
        R = 10 * M  # (0, capacity / 10]
        pre = [(4, i + 1, 10, T0 + 10 * i, 0) for i in range(M)] + [(4, M + 1, 90 * M, T0 + 10 * M, 0)]
        a = c.run(f"pending/{N}", 110 * M + 5, R, pre, [(4, PROBE_KEY, 10 * N - 4, 0, 0)], M + 1)
        b = c.run(f"pending/{N}-1", 110 * M + 5, R, pre, [(4, PROBE_KEY, 10 * N - 5, 0, 0)], M + 1)
        c.pair(f"weightedSize > capacity, {N} pending", "arg", b, a)
        if N >= 2:
            pre = [(4, i + 1, 10, T0 + 10 * i, 0) for i in range(N - 1)] + [(7, 0, 10 * (N - 1), 0, 0)]
            c.run(f"cascade/{N}", 10 * (N - 1) + 1, 1, pre, [(0, PROBE_KEY, 2, 0, 0)], N - 1)
    out.append(c)
    return out


def _clhm_case():
    """Plain caches: the comparisons of put / AddTask, LinkedDeque.insert and .reposition, Node.touch, UpdateTask, RemovalTask."""
    c = _Case("clhm", "clhm")
    five = [(0, i + 1, 10, T0 + i, 0) for i in range(5)]  # lastUsed T0 .. T0 + 4: neighbours one unit apart
    # weightedSize == capacity / + 1 after a put and after a weight update (quiet and stamped)
    a = c.run("put/fits", 60, -1, five, [(0, PROBE_KEY, 10, 0, 0)])
    b = c.run("put/over", 60, -1, five, [(0, PROBE_KEY, 11, 0, 0)])
    c.pair("put: weightedSize at capacity / + 1", "arg", a, b)
    for t, how in ((-1, "quiet"), (T0 + 100, "stamped")):
        a = c.run(f"update/{how}/fits", 60, -1, five, [(2, 3, 20, t, 0)])
        b = c.run(f"update/{how}/over", 60, -1, five, [(2, 3, 21, t, 0)])
        c.pair(f"weight update ({how}): weightedSize at capacity / + 1", "arg", a, b)
    a = c.run("put/fits-by-capacity", 60, -1, five, [(0, PROBE_KEY, 10, 0, 0)])
    b = c.run("put/over-by-capacity", 59, -1, five, [(0, PROBE_KEY, 10, 0, 0)])
    c.pair("put: capacity at weightedSize / - 1", "cap", b, a)
    # an insert one below, at and one above a neighbour's lastUsed (insert walks from the tail to the first lastUsed <= time)
    runs = [c.run(f"insert/time{d:+d}", 1000, -1, five, [(0, PROBE_KEY, 10, T0 + 2 + d, 0)]) for d in (-1, 0, 1)]
    c.pair("insert: time one below / at a neighbour", "time", runs[0], runs[1])
    c.pair("insert: time at / one above a neighbour", "time", runs[1], runs[2])
    # reposition after a read.  Right neighbour at lu / lu - 1: a read of the entry at T0 + 1 stamped T0 + 2 stays, T0 + 3 moves
    runs = [c.run(f"get/stamp{d:+d}", 1000, -1, five, [(1, 2, 0, T0 + 2 + d, 0)]) for d in (-2, -1, 0, 1)]
    c.pair("touch: older / equal time", "time", runs[0], runs[1], alike=True)  # max(lastUsed, time), :1358
    c.pair("touch: equal / newer time", "time", runs[1], runs[2])
    c.pair("reposition: right neighbour at lu / lu - 1", "time", runs[2], runs[3])
    # left neighbour at lu / lu + 1: only a read "now" (time 0) of an entry stamped in the future lowers a lastUsed
    for d in (0, 1):
        pre = [(0, 1, 10, NOW - 5, 0), (0, 2, 10, NOW + d, 0), (0, 3, 10, NOW + 7, 0), (0, 4, 10, NOW + 9, 0)]
        runs.append(c.run(f"get/now/left{d:+d}", 1000, -1, pre, [(1, 3, 0, 0, 0)]))
    c.pair("reposition: left neighbour at lu / lu + 1", "time", runs[-2], runs[-1])
    # between two neighbours of its own lastUsed a read leaves the entry where it is (both comparisons admit equality, :246-249)
    ties = [(0, i + 1, 10, T0, 0) for i in range(5)]
    c.run("get/among-ties", 1000, -1, ties, [(1, 3, 0, T0, 0)])
    c.run("get/among-ties-older", 1000, -1, ties, [(1, 3, 0, T0 - 1, 0)])
    c.run("get/now", 1000, -1, five, [(1, 2, 0, 0, 0)])
    c.run("get/absent", 1000, -1, five, [(1, 77, 0, 0, 0)])
    c.run("put/present", 1000, -1, five, [(0, 2, 10, T0 + 3, 0)])  # putIfAbsent of a present key: a read (:832)
    # a weight update stamped with the entry's own lastUsed / + 1 (UpdateTask :647), quiet, and with no difference
    runs = [c.run(f"update/stamp{d:+d}", 1000, -1, five, [(2, 2, 15, T0 + 1 + d, 0)]) for d in (-1, 0, 1, 2)]
    # `newTime != lastUsed` (:647) guards a touch that would change nothing: touch keeps the larger time
    c.pair("weight update: time one below / at lastUsed", "time", runs[0], runs[1], alike=True)
    c.pair("weight update: time at lastUsed / + 1", "time", runs[1], runs[2])
    c.pair("weight update: time at the right neighbour / + 1", "time", runs[2], runs[3])
    c.run("update/quiet", 1000, -1, five, [(2, 2, 15, -1, 0)])
    c.run("update/now", 1000, -1, five, [(2, 2, 15, 0, 0)])
    a = c.run("update/same-weight/quiet", 1000, -1, five, [(2, 2, 10, -1, 0)])
    c.run("update/same-weight/stamped", 1000, -1, five, [(2, 2, 10, T0 + 3, 0)])
    b = c.run("update/one-more/quiet", 1000, -1, five, [(2, 2, 11, -1, 0)])
    c.pair("weight update: difference 0 / 1", "arg", a, b)
    c.run("update/absent", 1000, -1, five, [(2, 77, 11, -1, 0)])
    # removing the only entry: oldestTime is -1 again (clhm :1117)
    c.run("remove/only", 1000, -1, five[:1], [(3, 1, 0, 0, 0), (1, 1, 0, 0, 0)])
    c.run("remove/absent", 1000, -1, five, [(3, 77, 0, 0, 0)])
    c.run("remove/head-then-put", 1000, -1, five, [(3, 1, 0, 0, 0), (0, 1, 10, T0 - 1, 0)])
    # an entry heavier than the whole cache is evicted by its own insert, after everything older
    a = c.run("put/self-evicted", 60, -1, five, [(0, PROBE_KEY, 61, 0, 0)])
    b = c.run("put/whole-cache", 60, -1, five, [(0, PROBE_KEY, 60, 0, 0)])
    c.pair("put: an entry of the capacity / + 1", "arg", b, a)
    return c


def _managed_prefix(weights, cap, claim_back=True):
    """entries of the given weights as ModelMesh loads them: insertNewEntry, then the space claimed back (totalUnloadingWeight 0)"""
    rows = []
    for i, w in enumerate(weights):
        rows.append((4, i + 1, w, T0 + i, 0))
        if claim_back:
            rows.append((7, 0, w, 0, 0))
    return rows


def _manager_case():
    """ModelCacheUnloadBufManager's comparisons; capacity 10 000, reserve 100 unless said."""
    c = _Case("manager", "manager")
    C, R = 10_000, 100
    full = _managed_prefix([4_000, 3_000, 2_900], C)  # occupancy 9 900 + the reserve: exactly full
    half = _managed_prefix([3_000, 2_000], C)         # occupancy 5 000
    for op, how in ((6, "ready"), (7, "claim")):
        # totalUnloadingWeight + required at the reserve / + 1 (:397)
        a = c.run(f"{how}/tuw-at-reserve", C, R, full, [(op, 0, R, 0, 0), (6, 0, 1, 0, 0)])
        b = c.run(f"{how}/tuw-over-reserve", C, R, full, [(op, 0, R + 1, 0, 0), (6, 0, 1, 0, 0)])
        c.pair(f"{how}: totalUnloadingWeight + required at reserved / + 1", "arg", a, b)
        # newTuw + occupancy at the capacity / + 1 (:400)
        a = c.run(f"{how}/occupancy-at-capacity", C, R, half, [(op, 0, 5_000, 0, 0), (6, 0, 1, 0, 0)])
        b = c.run(f"{how}/occupancy-over-capacity", C, R, half, [(op, 0, 5_001, 0, 0), (6, 0, 1, 0, 0)])
        c.pair(f"{how}: newTuw + occupancy at capacity / + 1", "arg", a, b)
    # ... at the reserve with an occupancy that no longer fits beside it (a load reported for an entry that is gone, 4 901 past
    # 5 000: occupancy 9 901, a deficit of 1, totalUnloadingWeight -1): the first comparison alone says "ready"
    gone = half + [(8, 77, 4_901, 0, 0)]
    for op, how in ((6, "ready"), (7, "claim")):
        a = c.run(f"{how}/tuw-at-reserve/no-room", C, R, gone, [(op, 0, R + 1, 0, 0), (6, 0, 1, 0, 0)])
        b = c.run(f"{how}/tuw-over-reserve/no-room", C, R, gone, [(op, 0, R + 2, 0, 0), (6, 0, 1, 0, 0)])
        c.pair(f"{how}: totalUnloadingWeight + required at reserved / + 1, no room", "arg", a, b)
    # the buffer's new weight at the reserve / + 1 (:379)
    a = c.run("claim/weight-at-reserve", C, R, half, [(7, 0, R, 0, 0)])
    b = c.run("claim/weight-over-reserve", C, R, half, [(7, 0, R + 1, 0, 0)])
    c.pair("adjustAggregateUnloadingWeight: newWeight at reserved / + 1", "arg", a, b)
    u = c.run("claim/one-under-reserve", C, R, half, [(7, 0, R - 1, 0, 0)])
    c.pair("adjustAggregateUnloadingWeight: newWeight at reserved - 1 / reserved", "arg", u, a)
    # ... and at the capacity / + 1 (the pathological clamp, :384): a claimed buffer of capacity - 50, then an entry of 50 / 51
    # put past the manager and removed through it — totalUnloadingWeight reaches capacity / capacity + 1
    pre = [(7, 0, C - 50, 0, 0)]
    a = c.run("clamp/at-capacity", C, R, pre, [(0, 1, 50, T0, 0), (10, 1, 0, 0, 0), (6, 0, 1, 0, 0)])
    b = c.run("clamp/over-capacity", C, R, pre, [(0, 1, 51, T0, 0), (10, 1, 0, 0, 0), (6, 0, 1, 0, 0)])
    c.pair("adjustAggregateUnloadingWeight: newWeight at capacity / + 1", "arg", a, b)
    # delta - cacheRemaining() at 0 / 1 (:229, :253): 5 100 of 10 000 used, 4 900 remain
    for key, who in ((2, "present"), (77, "absent")):
        a = c.run(f"after-load/{who}/fits", C, R, half, [(8, key, 4_900, 0, 0), (6, 0, 1, 0, 0)])
        b = c.run(f"after-load/{who}/deficit", C, R, half, [(8, key, 4_901, 0, 0), (6, 0, 1, 0, 0)])
        c.pair(f"adjustWeightAfterLoad ({who}): delta - cacheRemaining at 0 / 1", "arg", a, b)
        a = c.run(f"failed-placeholder/{who}/fits", C, R, half, [(12, key, 4_900, T0 + 9, 0), (6, 0, 1, 0, 0)])
        b = c.run(f"failed-placeholder/{who}/deficit", C, R, half, [(12, key, 4_901, T0 + 9, 0), (6, 0, 1, 0, 0)])
        # (over a present key the deficit is taken off the buffer and paid straight back, :256-266: nothing shows)
        c.pair(f"insertFailedPlaceholderEntry ({who}): weight - cacheRemaining at 0 / 1", "arg", a, b, alike=who == "present")
    c.run("after-load/zero", C, R, half, [(8, 2, 0, 0, 0), (8, 77, 0, 0, 0)])
    # min(weight, cacheDeficit) (:354) in its three callers: a deficit of 40 (an entry grown 40 past what remains), then
    # unloadComplete(39 / 40 / 41), discardFailedEntry(..), adjustWeightAfterLoad(- ..)
    owe = half + [(8, 2, 4_940, 0, 0)]
    for op, flag, sign, who in ((9, 1, 1, "unloadComplete"), (11, 0, 1, "discardFailedEntry"), (8, 0, -1, "adjustWeightAfterLoad")):
        runs = [c.run(f"pay-down/{who}/{w}", C, R, owe, [(op, 2, sign * w, 0, flag), (6, 0, 1, 0, 0)]) for w in (39, 40, 41)]
        c.pair(f"{who}: weight at cacheDeficit - 1 / cacheDeficit", "arg", runs[0], runs[1])
        c.pair(f"{who}: weight at cacheDeficit / + 1", "arg", runs[1], runs[2])
    # a failed unload (:323-329): capacity - weight at 2 / 1 / 0 / -1 on a cache whose reserve is 1, holding one entry of
    # weight 1 that the capacity of 1 evicts; oldestTime keeps the evicted entry's time until the next write (clhm :305-316)
    tiny = [(4, 1, 1, T0, 0), (7, 0, 1, 0, 0)]
    runs = [c.run(f"failed-unload/capacity-less-{w}", 10, 1, tiny, [(9, 0, w, 0, 0), (6, 0, 1, 0, 0), (1, 77, 0, 0, 0), (4, 2, 1, T0 + 5, 0)])
            for w in (7, 8, 9, 10, 11)]
    for i, what in enumerate(("3 / 2", "2 / 1", "1 / 0", "0 / -1")):
        c.pair(f"failed unload: capacity - weight at {what}", "arg", runs[i], runs[i + 1])
    # weightedSize at the capacity / + 1 after setCapacity
    pre = _managed_prefix([4_000, 3_000, 2_000], C)  # 9 100 of 10 000
    a = c.run("failed-unload/to-weightedSize", C, R, pre, [(9, 0, 900, 0, 0), (6, 0, 1, 0, 0), (1, 2, 0, 0, 0)])
    b = c.run("failed-unload/under-weightedSize", C, R, pre, [(9, 0, 901, 0, 0), (6, 0, 1, 0, 0), (1, 2, 0, 0, 0)])
    c.pair("setCapacity: capacity at weightedSize / - 1", "arg", a, b)
    # insertNewEntry over an existing key pays the weight back at once (:139)
    c.run("insert/existing", C, R, half, [(4, 2, 700, T0 + 50, 0), (6, 0, 1, 0, 0)])
    c.run("insert/existing-now", C, R, half, [(4, 1, 700, 0, 0)])
    # a weak prediction (adjustNewEntrySpaceRequest(.., weakPrediction): the entry's weight is stored negated, MM.java:1755-1760)
    # removed through the manager, and evicted
    weak = half + [(5, 2, 500, 0, 1)]
    c.run("weak/removed", C, R, weak, [(10, 2, 0, 0, 0), (6, 0, 1, 0, 0)])
    c.run("weak/evicted", C, R, weak, [(9, 0, 9_000, 0, 0), (6, 0, 1, 0, 0)])
    c.run("space-request/absent", C, R, half, [(5, 77, 500, 0, 0)])
    c.run("space-request/strong", C, R, half, [(5, 2, 500, 0, 0), (7, 0, 500, 0, 0)])
    c.run("remove/absent", C, R, half, [(10, 77, 0, 0, 0)])
    c.run("read", C, R, half, [(1, 1, 0, 0, 0), (1, 77, 0, 0, 0)])
    c.run("unload-complete", C, R, half, [(9, 0, 300, 0, 1)])
    return c


def _wide_case():
    """Values no mesh produces but the types allow: capacities at the int clamps (:348, :384), a totalUnloadingWeight within one
    unit of wrapping, a weight of 2^31 - 1, lastUsed at the ends of long beside the pinned entry's Long.MAX_VALUE."""
    c = _Case("wide", "wide")
    for cap in (2**31 - 2, 2**31 - 1, 2**31, 2**40):
        one = _managed_prefix([1_000], cap)
        # cacheRemaining()'s clamp: what remains is capacity - 1 100
        for delta in sorted({d for d in (cap - 1_101, cap - 1_100, cap - 1_099, I32_MAX - 1, I32_MAX) if d <= I32_MAX}):
            c.run(f"remaining/{cap}", cap, 100, one, [(8, 1, delta, 0, 0), (6, 0, 1, 0, 0)])
        # the buffer's weight against (int) capacity: claims up to what the capacity admits
        for want in (I32_MAX - 1_001, I32_MAX - 1_000):
            c.run(f"claim/{cap}", cap, 100, one, [(7, 0, want, 0, 0), (7, 0, 1, 0, 0), (6, 0, 1, 0, 0)])
    # totalUnloadingWeight one unit from wrapping: 2^31 - 2, + 1, + 1 (wraps negative: "ready" again, :397)
    c.run("tuw/wraps", 2**40, 100, [], [(7, 0, I32_MAX - 1, 0, 0), (7, 0, 1, 0, 0), (6, 0, 1, 0, 0), (7, 0, 1, 0, 0), (6, 0, 1, 0, 0)])
    c.run("tuw/wraps-down", 2**40, 100, [], [(4, 1, I32_MAX, T0, 0), (4, 2, 2, T0 + 1, 0), (7, 0, 1, 0, 0)])
    # a load reported 600 units smaller for an entry of 1 / 599 / 601: the sum -599 / -1 / 1 is stored as it is, and the weigher
    # answers its magnitude (CacheEntry.getWeight, MM.java:1759): 599, 1 and 1.  (A sum of 0 is outside the domain: a dead node.)
    for w in (1, 599, 601):
        c.run(f"after-load/below-zero/{w}", 10_000, 100, _managed_prefix([w, 50], 10_000),
              [(8, 1, -600, 0, 0), (6, 0, 1, 0, 0), (1, 1, 0, 0, 0), (10, 1, 0, 0, 0), (6, 0, 1, 0, 0)])
    c.run("weight/int-max", 2**40, -1, [(0, 1, 5, T0, 0)], [(0, 2, I32_MAX, T0 + 1, 0), (0, 3, I32_MAX, T0 + 2, 0), (2, 1, I32_MAX, -1, 0), (3, 2, 0, 0, 0)])
    c.run("weight/int-max-evicts", 2**31, -1, [(0, 1, 5, T0, 0)], [(0, 2, I32_MAX, T0 + 1, 0), (0, 3, I32_MAX, T0 + 2, 0)])
    # lastUsed 1 and Long.MAX_VALUE - 1 (a put throws on a negative time, clhm :825: -1 and Long.MIN_VALUE come as read stamps)
    for managed in (False, True):
        put, res = (4, 100) if managed else (0, -1)
        pre = [(put, 1, 10, T0, 0), (put, 2, 10, T0 + 1, 0)]
        for t in (1, I64_MAX - 1, I64_MAX):
            c.run(f"put/time{t}", 10_000, res, pre, [(put, PROBE_KEY, 10, t, 0), (1, 1, 0, t, 0)])
        for t in (-1, I64_MIN, 1, I64_MAX - 1, I64_MAX):
            c.run(f"get/time{t}", 10_000, res, pre, [(1, 1, 0, t, 0), (1, 2, 0, 0, 0)])
    return c


def _edge_builders():
    return _lengths_cases() + [_clhm_case(), _manager_case(), _wide_case()]


def edge_cases():
    """[{name, tier, caps, reserved, ops, bounds, n_prefix, runs, pairs, tag_names, pair_names}]"""
    return [c.build() for c in _edge_builders()]


def run_rows(case, c):
    """the operation indices of cache c: (prefix, probe)"""
    idx = np.nonzero(case["ops"]["cache"] == c)[0]
    return idx[idx < case["n_prefix"]], idx[idx >= case["n_prefix"]]


EDGE_OP_OUT = np.dtype([("result", "<i4"), ("n_evicted", "<i4"), ("evicted_off", "<i4"), ("buffer_weight", "<i4"),
                        ("weighted_size", "<i8"), ("oldest_time", "<i8")])


def load_edge_case(vec, name):
    """one case of tests/golden/ref_clhm_edges.npz as edge_cases() lays it out, with the reference's answers beside it (the
    file keeps `ops` and `outs` a column per entry)"""
    pre = f"{name}/"
    v = {k[len(pre):]: vec[k] for k in vec.files if k.startswith(pre) and "." not in k[len(pre):]}
    for what, dt in (("ops", CACHE_OP), ("outs", EDGE_OP_OUT)):
        a = np.zeros(len(vec[f"{pre}{what}.{dt.names[0]}"]), dtype=dt)
        for f in dt.names:
            a[f] = vec[f"{pre}{what}.{f}"]
        v[what] = a
    v["name"], v["tier"], v["n_prefix"] = name, str(v["tier"]), int(v["bounds"][-2])
    return v


def edge_state(v, j, c):
    """cache c after the operations before boundary j: (hdr, key, weight, last_used); hdr = entries, capacity, weightedSize,
    totalUnloadingWeight, totalModelCacheOccupancy, cacheDeficit, data.size()"""
    hdr = v[f"b{j}/hdr"]
    a = int(hdr[:c, 0].sum())
    b = a + int(hdr[c, 0])
    return hdr[c], v[f"b{j}/key"][a:b], v[f"b{j}/weight"][a:b], v[f"b{j}/last_used"][a:b]


def run_signature(v, case, c):
    """everything the reference shows of run c from its probe on: per probe operation the result, the evicted keys in listener
    order, the buffer weight, weightedSize and oldestTime; then the final deque, the capacity and the manager's three fields"""
    _, probe = run_rows(case, c)
    outs, ev = v["outs"], v["evicted"]
    sig = [(int(o["result"]), tuple(int(k) for k in ev[o["evicted_off"]: o["evicted_off"] + o["n_evicted"]]), int(o["buffer_weight"]),
            int(o["weighted_size"]), int(o["oldest_time"])) for o in outs[probe]]
    hdr, key, wt, lu = edge_state(v, len(case["bounds"]) - 1, c)
    return sig, tuple(int(x) for x in hdr[1:6]), key.tobytes(), wt.tobytes(), lu.tobytes()


def edge_occurrence(v, tier, name):
    """{what the case is there for: whether it occurs}; v: the case's arrays (inputs and the reference's answers)"""
    ops, outs, runs, tags = v["ops"], v["outs"], v["runs"], [str(t) for t in v["tag_names"]]
    last = len(v["bounds"]) - 1
    hdr = v[f"b{last}/hdr"]
    occ = {}
    want_ops = {"lengths_plain": (0, 1, 3), "lengths_managed": (4, 1, 10), "lengths_big": (0, 1, 3, 4, 10), "mass_plain": (0,),
                "mass_managed": (0, 4, 7), "clhm": (0, 1, 2, 3), "manager": (0, 1, 4, 5, 6, 7, 8, 9, 10, 11, 12), "wide": (0, 1, 2, 3, 4, 7, 8)}[name]
    for op in want_ops:
        occ[f"op {op}"] = bool((ops["op"] == op).any())
        res = outs["result"][ops["op"] == op]
        if op in {"clhm": (0, 1, 2, 3), "manager": (1, 4, 5, 6, 7, 8, 9, 12)}.get(name, ()):
            occ[f"op {op} answers 0 and 1"] = bool((res == 0).any() and (res == 1).any())
    probe_n_ev = {}
    for r in runs:
        idx = np.nonzero(ops["cache"] == r["cache"])[0]
        probe_n_ev[int(r["cache"])] = int(outs["n_evicted"][idx[idx >= int(v["bounds"][-2])]].max(initial=0))
    if name.startswith("lengths"):
        widths = set()
        for r in runs:
            n = int(r["entries"]) + int(r["managed"])
            ins = int(sum(is_insert(int(o)) for o in ops["op"][(ops["cache"] == r["cache"]) & (np.arange(len(ops)) >= int(v["bounds"][-2]))]))
            widths.add((team_width(n + ins), n + ins + 1))
        if name == "lengths_big":
            occ["2047 slots"] = (64, 2048) in widths
        else:
            for tw, s in ((8, 48), (16, 49), (16, 160), (64, 161)):  # slots + 1 on both sides of kTeam8Slots and kTeam16Slots
                occ[f"{tw} lanes at {s} slots"] = (tw, s) in widths
        for what in ("insert/head", "insert/tail", "get/head", "get/tail", "remove/head", "remove/tail"):
            occ[what] = what in tags
        if name != "lengths_big":
            for what in ("insert/behind-ties", "get/edge", "get/edge-1", "remove/edge", "remove/edge-1", "insert/head+-1", "insert/head++0",
                         "insert/head++1", "insert/end--1", "insert/end-+0", "insert/end-+1"):
                occ[what] = what in tags
    if name.startswith("mass"):
        kinds = ("evict",) if name == "mass_plain" else ("pending", "cascade")
        for kind in kinds:
            for N in MASS:
                if kind == "cascade" and N < 2:
                    continue
                c = [int(r["cache"]) for r in runs if tags[r["tag"]] == f"{kind}/{N}"]
                occ[f"{kind}: {N} evicted by one operation"] = len(c) == 1 and probe_n_ev[c[0]] == N
        if name == "mass_managed":
            occ["the buffer clamped to the capacity"] = bool(((hdr[:, 3] > hdr[:, 1]) & (hdr[:, 2] == hdr[:, 1])).any())
    if name == "clhm":
        occ["oldestTime -1 after a removal"] = bool(((ops["op"] == 3) & (outs["oldest_time"] == -1)).any())
        occ["a put that evicts itself"] = any(PROBE_KEY in v["evicted"][o["evicted_off"]: o["evicted_off"] + o["n_evicted"]] for o in outs)
    if name == "manager":
        occ["a deficit"] = bool((hdr[:, 5] > 0).any())
        occ["removeEntry answers -1 and a weight"] = bool(((ops["op"] == 10) & (outs["result"] == -1)).any() and ((ops["op"] == 10) & (outs["result"] > 0)).any())
        occ["a deficit paid down to 0"] = any(tags[r["tag"]].startswith("pay-down") and hdr[r["cache"], 5] == 0 for r in runs)
        occ["capacity 1"] = bool((hdr[:, 1] == 1).any())
        occ["a negative totalUnloadingWeight"] = bool((hdr[:, 3] < 0).any())
        stale = False
        for i in np.nonzero((ops["op"] == 9) & (ops["flag"] == 0) & (outs["n_evicted"] > 0))[0]:
            nxt = [k for k in range(i + 1, len(ops)) if ops["cache"][k] == ops["cache"][i]]
            stale |= bool(nxt) and outs["oldest_time"][nxt[0]] == outs["oldest_time"][i] and ops["op"][nxt[0]] == 6
        occ["a stale oldestTime after a failed unload"] = bool(stale)
        occ["the buffer above its reserve"] = bool((outs["buffer_weight"] > 100).any())
    if name == "wide":
        occ["capacity above int"] = bool((hdr[:, 1] > I32_MAX).any())
        occ["totalUnloadingWeight wrapped"] = bool((hdr[:, 3] < -2**30).any())
        occ["a weight of 2^31 - 1"] = bool((v[f"b{last}/weight"] == I32_MAX).any())
        occ["weightedSize above int"] = bool((hdr[:, 2] > I32_MAX).any())
        lus = v[f"b{last}/last_used"]
        occ["lastUsed 1 and Long.MAX_VALUE - 1"] = bool((lus == 1).any() and (lus == I64_MAX - 1).any())
    return occ
