"""The values the label parser is held to (tests/test_pod_labels_model.py pins the hand-worked ones on the CPU,
tests/test_pod_labels_gpu.py and tests/pod_labels_child.py send all of them through the device): the hand-worked shapes, the
records that fill an element round, the chunk and tile edges, the planted batches — and Pair, a context and the model side by
side, which collects every difference instead of stopping at the first (the child process prints them)."""
import numpy as np

from modelmesh_amd.solver import MmpError, Solver
from tests.pod_labels_model import PodLabelsModel

# bits 0..4 as the hand-worked values use them: plain, plain, the empty string, UTF-8, plain; then label-5 .. label-63
NAMES = ["gpu", "zone-a", "", "größe-µ", "label-4"] + ["label-%d" % i for i in range(5, 64)]
GPU, ZONE, EMPTY, UTF, L4 = 1, 2, 4, 8, 16
TILE = 2048  # kJTileBytes: a longer value takes the serial route


def rec(labels_member):
    """a well-formed record with the given text as one of its members"""
    return '{"count":3,%s,"cap":100,"startTime":7}' % labels_member


# (value, word, count): the accepted shapes, worked by hand
ACCEPTED = [
    ('{"count":3,"cap":100}', 0, 0),                                   # absent
    (rec('"labels":null'), 0, 0),
    (rec('"labels":[]'), 0, 0),
    (rec('"labels": [ \t\n ] '), 0, 0),
    (rec('"labels":["gpu"]'), GPU, 1),                                 # one known
    (rec('"labels":["tpu"]'), 0, 1),                                   # one unknown: counted, no bit
    (rec('"labels":["gpu","gpu"]'), GPU, 2),                           # repeated: one bit, counted twice
    (rec('"labels":["zone-a" , "gpu" ,"other"]'), GPU | ZONE, 3),
    (rec('"labels":["gp\\u0075"]'), 0, 1),                             # an escape that would decode to "gpu": the raw bytes differ
    (rec('"labels":["a\\"b","gpu"]'), GPU, 2),                         # an escaped quote inside an element
    (rec('"labels":["zone-a\\\\"]'), 0, 1),
    (rec('"labels":[""]'), EMPTY, 1),                                  # the empty-string name
    (rec('"labels":["größe-µ","x"]'), UTF, 2),                         # a UTF-8 name, matched by bytes
    (rec('"labels":["gpu"],"labels":null'), 0, 0),                     # array then null: the last decides
    (rec('"labels":null,"labels":["label-4"]'), L4, 1),                # null then array
    (rec('"labels":["gpu","zone-a"],"x":1,"labels":["label-4"]'), L4, 1),
    (rec('"labels":["],[","gpu"]'), GPU, 2),                           # structure inside a string is text
    ('{"labels":["gpu"]}', GPU, 1),                                    # the only member
    ('{"count":1,"labels":["zone-a"]}', ZONE, 1),                      # the last member
]

# the rejected shapes of a `labels` value; JSON_REFUSES: those json.loads itself refuses (rejected with or without a table)
REJECTED = ['1', '-0.5', '"gpu"', '{}', '{"gpu":1}', 'true', 'false',
            '[1]', '["gpu",1]', '[null]', '["gpu",null]', '[["gpu"]]', '["gpu",["zone-a"]]', '[{"a":"b"}]', '[true]',
            '[,"gpu"]', '["gpu",,"zone-a"]', '["gpu",]', '[,]', '["gpu" "zone-a"]', '["gpu""zone-a"]']
JSON_REFUSES = ('[,"gpu"]', '["gpu",,"zone-a"]', '["gpu",]', '[,]', '["gpu" "zone-a"]', '["gpu""zone-a"]')
UNTERMINATED = ['{"count":3,"labels":["gpu"', '{"count":3,"labels":["gpu","cap":100}', '{"count":3,"labels":["gpu}', '{"labels":[']
MALFORMED_RECORDS = ['{"count":"x","labels":["gpu"]}', '{"labels":["gpu"]} x', '']


def rejected_variants(shape):
    """the shape as the last occurrence, alone, and as an earlier or later duplicate of a well-formed one"""
    return [rec('"labels":' + shape), '{"labels":%s}' % shape, rec('"labels":%s,"labels":["gpu"]' % shape),
            rec('"labels":%s,"labels":null' % shape), rec('"labels":["gpu"],"labels":' + shape)]


def hand_values():
    out = [v for v, _, _ in ACCEPTED]
    for shape in REJECTED:
        out += rejected_variants(shape)
    return out + UNTERMINATED + MALFORMED_RECORDS


def _element(i):
    return '"%s"' % (NAMES[i % 70] if i % 70 < 64 else "unk-%d" % i)


def filler(n_elements, first=0):
    """a record whose labels array holds n_elements elements: the 64 names in turn, six unknown ones between the rounds"""
    return rec('"labels":[%s]' % ",".join(_element(first + i) for i in range(n_elements)))


def tile_fillers():
    """63, 64, 65 and 130 elements: an element round not full, full, one over, and three rounds"""
    return [filler(63), filler(64), filler(65), filler(130)]


def nine_block():
    """eight records of 9 elements each: 72 elements in one group of 8"""
    return [filler(9, first=7 * r) for r in range(8)]


CHUNK_TEMPLATE = '{"count":3,%s"labels":["gpu", "x","zone-a" ,"label-63"],"cap":100,"startTime":7}'


def chunk_edge_values():
    """One template shifted by 0 .. 63 padding blanks in front of `"labels"`: every byte of the member — the name, the '[', each
    comma, each quote, the ']' — falls on the last byte of a 64-byte chunk in one value and on the first in the next."""
    return [CHUNK_TEMPLATE % (" " * (40 + pad)) for pad in range(64)]


def _padded(member_fmt, length):
    v = rec(member_fmt % "")
    return rec(member_fmt % (" " * (length - len(v))))


def tile_edge_values():
    """-> (values, groups): values of 2 046 .. 2 050 bytes — both sides of the serial route — at the four dword alignments (a
    `{}` record of 2 .. 5 bytes in front shifts what follows); groups = lists of indices whose label content is the same, so
    that both routes must give them equal answers."""
    values, groups = [], []
    for fmt in ('"labels":["gpu",%s"zone-a","x","label-63"]', '"labels":["gpu","zone-a",%s]', '"labels":["gpu" %s"zone-a"]',
                '"labels":[1%s]', '"labels":["gpu"],%s"labels":null'):
        group = []
        for shim in range(4):
            values.append("{}" + " " * shim)
            for length in range(TILE - 2, TILE + 3):
                group.append(len(values))
                values.append(_padded(fmt, length))
        groups.append(group)
    return values, groups


def big(n, n_keys=64, seed=5):
    """-> (keys, values, deleted): n short events over n_keys ids, drawn from a pool of distinct values, with rejected, over-long
    (serial route, one well-formed and one rejected) and empty values and deletions planted, and nine_block() at event 4 096
    (a multiple of every group size ingest_group picks) when n reaches that far."""
    rng = np.random.default_rng(seed)
    ids = ["%06x-%04d" % (k % 5, k) for k in range(n_keys)]
    pool = []
    for k in range(32):
        els = [_element(int(rng.integers(0, 70))) for _ in range(int(rng.integers(0, 6)))]
        member = '"labels":%s' % ("null" if k % 8 == 7 else "[%s]" % ",".join(els))
        pool.append('{"count":%d,"used":%d,%s,"cap":%d,"startTime":%d}' % (k, 10 * k, member, 1000 + k, 50 + k) if k % 4 else
                    '{"count":%d,"cap":%d,"startTime":%d}' % (k, 1000 + k, 50 + k))
    bad = [v for shape in REJECTED for v in rejected_variants(shape)[::2]] + UNTERMINATED
    long_good, long_bad = _padded('"labels":["label-9",%s"q","label-63"]', TILE + 60), _padded('"labels":["label-9",%s]', TILE + 60)
    pick = rng.integers(0, len(pool), n)
    key = rng.integers(0, n_keys, n)
    keys, values, deleted = [], [], np.zeros(n, np.uint8)
    for i in range(n):
        if i % 97 == 3:
            v = bad[(i // 97) % len(bad)]
        elif i % 1531 == 7:
            v = long_bad if (i // 1531) % 3 == 2 else long_good
        elif i % 211 == 5:
            v = ""
        else:
            v = pool[pick[i]]
        if i % 53 == 0:
            deleted[i] = 1
        keys.append(ids[key[i]])
        values.append(v)
    if n >= 4096 + 8:
        values[4096:4104] = nine_block()
        deleted[4096:4104] = 0
    return keys, values, deleted


class Pair:
    """A context and the model, given the same calls; every difference is noted in self.diffs."""

    def __init__(self):
        self.s, self.m, self.diffs = Solver(100, 1000), PodLabelsModel(), []

    def close(self):
        self.s.close()

    def load_ids(self, ids):
        self.s.load_pod_ids(ids)
        self.m.load(ids)

    def names(self, names):
        self.s.label_names_load(names)
        self.m.names_load(names)

    def set(self, idx, words, counts):
        self.s.pod_labels_set(idx, words, counts)
        self.m.labels_set(idx, words, counts)

    def _same(self, tag, name, got, want):
        got, want = np.asarray(got), np.asarray(want)
        if got.shape != want.shape or not np.array_equal(got, want):
            where = np.flatnonzero(got != want)[:6] if got.shape == want.shape else "shapes"
            self.diffs.append("%s: %s differs at %s: %s, the model's %s" % (tag, name, where, got[where] if got.shape == want.shape else got.shape,
                                                                            want[where] if got.shape == want.shape else want.shape))

    def state(self, tag):
        """the rows and the resident labels"""
        self._same(tag, "rows", self.s.get_pods(), self.m.rows)
        for name, g, w in zip(("label words", "label counts"), self.s.pod_labels_get(), self.m.labels_get()):
            self._same(tag, name, g, w)

    def events(self, tag, keys, values, deleted=None, live=None, append=True):
        want = self.m.events(keys, values, deleted, live, append)
        got = self.s.pods_events_json(keys, values, deleted, live, append)
        for name, g, w in zip(("status", "pod_idx", "start_time"), got, want):
            self._same(tag, name, g, w)
        if got[3] != want[3]:
            self.diffs.append("%s: %d ids joined, the model's %d" % (tag, got[3], want[3]))
        self.state(tag)
        return got, want

    def ingest(self, tag, values, pod_idx, live=None):
        want = self.m.ingest(values, pod_idx, live)
        got = self.s.ingest_pods_json(values, pod_idx, live)
        for name, g, w in zip(("status", "start_time"), got, want):
            self._same(tag, name, g, w)
        self.state(tag)
        return got, want


def corpus_differences(n_big):
    """The whole corpus against the model in the process' environment (MMP_JGROUP, MMP_LABEL_HASH_BITS): the hand-worked values
    and the edges by key with a pod of its own per value — so that the words read back are the words per event —, the element
    rounds, then big(n_big).  Every pod starts from a sentinel word, so an event that must change nothing shows."""
    p = Pair()
    try:
        tile_values, groups = tile_edge_values()
        sets = [("hand", hand_values()), ("fillers", tile_fillers() + nine_block()), ("chunk edges", chunk_edge_values()),
                ("tile edges", tile_values)]
        p.names(NAMES)
        for tag, values in sets:
            ids = ["%06x-%05d" % (k % 3, k) for k in range(len(values))]
            p.load_ids(ids)
            p.set(np.arange(len(ids)), np.full(len(ids), 0xABC, np.uint64), np.full(len(ids), 5, np.int32))
            (status, _, _, _), _ = p.events(tag, ids, values)
            if tag == "chunk edges" and status.any():
                p.diffs.append("chunk edges: a shifted copy of a well-formed value was rejected")
            if tag == "tile edges":
                words, counts = p.s.pod_labels_get()
                for g in groups:
                    if len({(int(status[i]), int(words[i]), int(counts[i])) for i in g}) != 1:
                        p.diffs.append("tile edges: the two routes differ on the same label content (values %s)" % g[:3])
        keys, values, deleted = big(n_big)
        p.load_ids(sorted(set(keys)))
        p.events("big(%d)" % n_big, keys, values, deleted)
        return p.diffs
    except MmpError as e:
        return p.diffs + ["MmpError: %s" % e]
    finally:
        p.close()
