"""The definition of the caches by model id (mmp_caches_load_keyed_k, mmp_cache_replay_k, mmp_cache_read_k, and what
mmp_models_retire does to bound caches), in Python: a dict from id to row on top of the cache oracle tests/test_cache_replay_gpu.py
uses (oracle.bind.CCache, whose integer keys are the registry rows here).

The rule by key.  Op i is what the plain replay makes of it with key = the row the id table answers for id i — the row AS THE
TABLE ANSWERS IT: a deleted record keeps its row (the empty row), and its entry is still found, read and removed.  Two kinds of op
read no id: reserved == COPK_RAW_KEY (the op keeps UNLOADBUF_KEY) and the four keyless codes (their key is reported as -1).

The statuses.  CKEY_LIVE: the id names a live record (and the two kinds above); CKEY_EMPTY_ROW: the row exists, its record is
deleted, the op ran as usual; CKEY_UNKNOWN: the table does not know the id.

Unknown ids.  A non-inserting op runs with CACHE_KEY_UNKNOWN, a key no cache holds: the answer for an absent key, with what
adjustWeightAfterLoad does to the manager's sums.  An inserting op is NOT RUN: result 0, nothing evicted, the cache as the preceding
op left it.

The eviction record.  The slots are mmp_cache_replay's: caches with ops, in index order, get (entries before the call + inserting
ops of the call, unknown ids included) slots each; a cache's victims fill its slots from the front in listener order; the other
slots hold row -1 and the empty span.  A victim's id is the id of its row.

The load.  Every entry's id must be known (the empty row counts as known); the lowest unknown entry is named and nothing changes.
A marked pseudo-entry gets UNLOADBUF_KEY and its id is not read.

The retirement.  A named row that is the key of a live entry refuses the call, the lowest such row is named; otherwise every live
key >= 0 becomes remap[key] (the survivors move down in order) and UNLOADBUF_KEY stays."""
from modelmesh_amd import _lib


class Refused(Exception):
    def __init__(self, what, index):
        super().__init__(f"{what} {index}")
        self.what, self.index = what, index


class IdTable:
    """id (bytes) -> row, and which rows are the empty row of a deleted record"""

    def __init__(self, ids, empty_rows=()):
        self.ids = [x if isinstance(x, bytes) else x.encode() for x in ids]
        self.empty = set(empty_rows)
        assert len(set(self.ids)) == len(self.ids)

    def resolve(self, key):
        """(status, row or None)"""
        key = key if isinstance(key, bytes) else key.encode()
        if key not in self.ids:
            return _lib.CKEY_UNKNOWN, None
        r = self.ids.index(key)
        return (_lib.CKEY_EMPTY_ROW if r in self.empty else _lib.CKEY_LIVE), r

    def load_rows(self, entry_ids, is_unloadbuf=None):
        """the keys of a load's entries; Refused("entry", lowest unknown entry)"""
        rows = []
        for e, k in enumerate(entry_ids):
            if is_unloadbuf is not None and is_unloadbuf[e]:
                rows.append(_lib.UNLOADBUF_KEY)
                continue
            st, r = self.resolve(k)
            if st == _lib.CKEY_UNKNOWN:
                raise Refused("entry", e)
            rows.append(r)
        return rows

    def op_key(self, op, key):
        """(status, key the op runs with, runs at all)"""
        if op["reserved"] == _lib.COPK_RAW_KEY:
            assert op["key"] == _lib.UNLOADBUF_KEY
            return _lib.CKEY_LIVE, _lib.UNLOADBUF_KEY, True
        if op["op"] in _lib.COP_KEYLESS:
            return _lib.CKEY_LIVE, -1, True
        st, r = self.resolve(key)
        if st == _lib.CKEY_UNKNOWN:
            return st, _lib.CACHE_KEY_UNKNOWN, op["op"] not in _lib.COP_INSERTING
        return st, r, True

    def replay(self, caches, ops, keys, now):
        """Apply the ops to the oracle caches (keys = rows).  -> (per op dicts, eviction record as (rows, ids) per slot)"""
        n_before = [len(h.nodes()[2]) for h in caches]
        out, victims = [], {}
        for op, key in zip(ops, keys):
            c = int(op["cache"])
            st, k, runs = self.op_key(op, key)
            res, ev = (0, [])
            if runs:
                res, ev = caches[c].apply(int(op["op"]), int(k), int(op["arg"]), int(op["time"]), int(op["flag"]), now)
            victims.setdefault(c, []).extend(ev)
            out.append({"status": st, "key": k, "result": res, "evicted_rows": list(ev), "evicted_ids": [self.ids[r] for r in ev]})
        rec_rows, rec_ids = [], []
        for c in sorted(victims):
            slots = n_before[c] + sum(1 for op in ops if op["cache"] == c and op["op"] in _lib.COP_INSERTING)
            v = victims[c]
            assert len(v) <= slots
            rec_rows += v + [-1] * (slots - len(v))
            rec_ids += [self.ids[r] for r in v] + [b""] * (slots - len(v))
        return out, (rec_rows, rec_ids)

    def retire(self, rows, live_keys):
        """live_keys: the live keys of every cache.  -> remap (list, -1 for a retired row); Refused("row", lowest live key named).
        The table itself is renumbered too."""
        named = set(int(r) for r in rows)
        hit = sorted(k for keys in live_keys for k in keys if k in named)
        if hit:
            raise Refused("row", hit[0])
        remap, nxt = [], 0
        for r in range(len(self.ids)):
            remap.append(-1 if r in named else nxt)
            nxt += r not in named
        self.ids = [x for r, x in enumerate(self.ids) if r not in named]
        self.empty = {remap[r] for r in self.empty if remap[r] >= 0}
        return remap

    @staticmethod
    def renumber(keys, remap):
        return [remap[k] if k >= 0 else k for k in keys]
