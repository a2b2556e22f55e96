"""The oracle of tests/test_keyed_seams_gpu.py for WHICH ROW a key names: a Python dict over the loaded ids, kept in step with the
events the test sends (an id that joins gets the next row; a retire applies the remap the call returned).  Nothing here hashes,
probes or compares bytes the way the library's lookup does, so the two cannot share a mistake.  Also the generators of ids with
every awkward relation between two of them, and of request keys that hit and miss."""
import numpy as np


class KeyRows:
    """id (bytes) -> registry row"""

    def __init__(self, ids):
        self.row = {}
        for k in ids:
            assert k not in self.row
            self.row[k] = len(self.row)
        self.n = len(ids)

    def join(self, keys):
        """an appending event batch: every key not yet known gets the next row, in order of first appearance"""
        for k in keys:
            if k not in self.row:
                self.row[k] = self.n
                self.n += 1

    def retire(self, remap):
        """mmp_models_retire returned remap[old row] = new row, -1 for a retired one"""
        assert len(remap) == self.n
        self.row = {k: int(remap[r]) for k, r in self.row.items() if remap[r] >= 0}
        self.n = len(self.row)
        assert sorted(self.row.values()) == list(range(self.n))

    def rows(self, keys):
        return np.array([self.row.get(k, -1) for k in keys], np.int32).reshape(len(keys))

    def ids(self):
        out = [None] * self.n
        for k, r in self.row.items():
            out[r] = k
        return out


def make_ids(rng, n, tag=b"m", long_share=0.15):
    """n distinct ids of 1 to 200 bytes.  The first ten are engineered: multi-byte UTF-8, an id that is a proper prefix of another,
    two that differ in their last byte only, two of equal length that differ in the first byte only, one byte, 200 bytes."""
    utf = "modèle-日本語-Ω-".encode() + tag
    fixed = [utf, tag + b"-prefix", tag + b"-prefix-and-more", tag + b"-last-a", tag + b"-last-b", b"A" + tag + b"-first", b"B" + tag + b"-first",
             tag[:1], (tag + b"-two-hundred-") .ljust(200, b"x"), utf + "é".encode()]
    assert len(fixed[8]) == 200 and len(fixed[7]) == 1 and fixed[2].startswith(fixed[1])
    assert fixed[3][:-1] == fixed[4][:-1] and fixed[5][1:] == fixed[6][1:] and len(fixed[5]) == len(fixed[6])
    ids, seen = [], set()
    for k in fixed[:n]:
        assert k not in seen
        seen.add(k)
        ids.append(k)
    i = 0
    while len(ids) < n:
        i += 1
        head = tag + b"-%d-" % i
        size = int(rng.integers(150, 201)) if rng.random() < long_share else int(rng.integers(len(head) + 1, 48))
        body = bytes(rng.integers(0x61, 0x7b, size - len(head), dtype=np.uint8))
        k = head + body
        if k not in seen:
            seen.add(k)
            ids.append(k)
    assert all(1 <= len(k) <= 200 for k in ids)
    return ids


def request_keys(rng, want_rows, ids, never, rows_of):
    """One key per request.  want_rows[i] >= 0: usually the id of that row (a hit); otherwise, and for the rest, a miss of one of three
    kinds — an id never loaded, a known id plus one byte, a known id minus its last byte.  rows_of (KeyRows.rows) says what each key
    names in the end: a shortened id may be another id.  REFUSES a batch of 20 or more requests in which fewer than a tenth of the
    keys are known or fewer than a tenth unknown."""
    keys = []
    for i, r in enumerate(want_rows):
        if 0 <= r < len(ids) and rng.random() < 0.65:
            keys.append(ids[r])
            continue
        kind = int(rng.integers(0, 3))
        base = ids[int(rng.integers(len(ids)))]
        if kind == 0:
            keys.append(never[int(rng.integers(len(never)))])
        elif kind == 1:
            keys.append(base + bytes([int(rng.integers(1, 256))]))
        else:
            keys.append(base[:-1] if len(base) > 1 else base + b"\x00")
    check_mix(rows_of(keys))
    return keys


def check_mix(rows):
    n = len(rows)
    if n >= 20:
        known = int((rows >= 0).sum())
        assert known * 10 >= n and (n - known) * 10 >= n, (n, known)
