"""The wire-format parsers (modelmesh_amd/csrc/ingest_kernels.hpp) hold two parsers for one grammar — the wave path, which takes
up to eight records per wavefront inside one 2 048-byte LDS tile, and the serial walk of one lane for a longer record.  Here one
value is sent down every route and must give the same answer: exactly what tests/ingest_model.py says (status, type, n_loaded,
n_failed, last_used, lul, ent_off and the (pod, time) entries; for InstanceRecords the ten fields).  Nothing is measured.

The corpus (tests/ingest_corpus.py, built once): the MALFORMED / WELL_FORMED lists of test_ingest_gpu, duplicate fields, the
int64 / int32 extremes, 300 random documents and a strict prefix of each of the first 100."""
import os
import subprocess
import sys

import numpy as np
import pytest

from modelmesh_amd.solver import Solver
from tests import ingest_corpus as ic
from tests import ingest_model as im
from tests import registry_prune_model as rp
from tests.test_registry_upsert_json_gpu import Pair

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORPUS = ic.model_corpus()
CLASS = [im.model_class(v) for v in CORPUS]
PODS = ic.pod_corpus()
POD_CLASS = [im.pod_class(v) for v in PODS]
BIG = 65536 + 5  # eight records per wavefront, a ragged last wavefront


def _forms(corpus, classes, skip=()):
    vals, like = [], []
    for v, c in zip(corpus, classes):
        if v not in skip:
            for w in ic.forms(v, c):
                vals.append(w)
                like.append(v)
    return vals, like


@pytest.fixture(scope="module")
def solver():
    s = Solver(100, 1000)
    s.load_pod_ids(ic.IDS)
    s.load_type_names(ic.TYPE_NAMES, ic.UNKNOWN_TYPE)
    yield s
    s.close()


def reload(s, vals, like=None):
    status, lul = s.ingest_models_json(vals)
    diffs = ic.check_models(vals, status, lul, *s.get_models(), like=like)
    assert not diffs, "\n".join(diffs)


def ingest_pods(vals, like=None):
    """Record i into pod i of a fresh context."""
    s = Solver(100, 1000)
    try:
        s.load_pod_ids(["p%d" % i for i in range(len(vals))])
        before = s.get_pods()
        status, start = s.ingest_pods_json(vals, np.arange(len(vals), dtype=np.int32))
        diffs = ic.check_pods(vals, status, start, s.get_pods(), before, like=like)
    finally:
        s.close()
    assert not diffs, "\n".join(diffs)


# ---- 1. the serial walk is held to what the wave path is held to ---------------------------------------------------------------

def test_forced_serial_walk_models(solver):
    """Every corpus value as it stands, behind blanks up to 2 049 bytes, in front of as many, and (well-formed ones) behind a
    first field of padding: the long forms are walked by one lane and must give the short form's answer."""
    vals, like = _forms(CORPUS, CLASS)
    assert sum(len(v) > ic.TILE for v in vals) > 2 * len(CORPUS)
    reload(solver, vals, like)


def test_forced_serial_walk_pods():
    vals, like = _forms(PODS, POD_CLASS)
    ingest_pods(vals, like)


def test_forced_serial_walk_events():
    """The same forms as registry events on an existing registry (mmp_models_upsert_json), against the twin context that
    receives the parsed rows; then rejected values alone, one per row: the registry stays as it was.  Among them, in every form,
    the values that are rejected for an EARLIER duplicate only, which the twin's parser (it reads a dict) cannot judge."""
    pair = Pair(ic.IDS, ic.TYPE_NAMES, ic.UNKNOWN_TYPE)
    try:
        rows = 64
        pair.start([ic.sized(100 + k, k + 1, 2, 1) for k in range(rows)])
        vals, like = _forms(CORPUS, CLASS, skip=ic.TWIN_BLIND)
        pair.events(vals, (np.arange(len(vals)) % rows).astype(np.int32))
        blind = [w for v in ic.TWIN_BLIND for w in ic.forms(v, im.REJECT)]
        bad = (blind + [w for w, v in zip(vals, like) if ic.model_answer(v).status])[:rows]
        assert len(bad) == rows and len(blind) == 12 and sum(len(w) > ic.TILE for w in bad) > rows // 2
        assert all(ic.model_answer(v).status == 1 for v in ic.TWIN_BLIND)
        before = [a.copy() for a in rp.compact(*pair.j.get_models())]
        st, lul = pair.j.upsert_models_json(bad, np.arange(rows, dtype=np.int32))
        assert st.all() and not lul.any()
        for a, b in zip(before, rp.compact(*pair.j.get_models())):
            assert np.array_equal(a, b)
        pair.same()
    finally:
        pair.close()


# ---- 2. / 3. the tile edge and the chunk edges -----------------------------------------------------------------------------

def test_tile_edge_and_alignment(solver):
    """Values of 2 046..2 050 bytes (2 048 is the last the wave path takes), starting at each byte alignment of the staged dwords."""
    vals, like = ic.tile_edge_models()
    off = np.concatenate([[0], np.cumsum([len(v) for v in vals])])
    starts = {(int(off[i]) % 4, len(vals[i])) for i in range(1, len(vals), 2)}
    assert starts == {(a, n) for a in range(4) for n in range(ic.TILE - 2, ic.TILE + 3)}
    reload(solver, vals, like)


def test_chunk_edges_models(solver):
    """Six templates behind 0..127 blanks each: the escape carry, a quote, a key, a digit run and a literal across bytes 63 | 64
    and 127 | 128 of the 64-byte scan."""
    vals = ic.chunk_edge_models()
    assert len(vals) == 768 and all(ic.model_answer(t).status == 0 for t in ic.CHUNK_MODELS)
    reload(solver, vals, [t for t in ic.CHUNK_MODELS for _ in range(128)])


def test_chunk_edges_pods():
    vals = ic.chunk_edge_pods()
    assert len(vals) == 768 and all(ic.pod_answer(t)[0] == 0 for t in ic.CHUNK_PODS)
    ingest_pods(vals, [t for t in ic.CHUNK_PODS for _ in range(128)])


# ---- 4. the grouped wave path at the host's own group sizes -------------------------------------------------------------------

@pytest.mark.parametrize("n", [16383, 16384 + 3, 32768 + 1, BIG])
def test_grouped_path_random_batches(solver, n):
    """1, 2, 4 and 8 records per wavefront (the host's choice for these batch sizes), the last wavefront ragged; the records are
    drawn from the corpus by index, well-formed and malformed mixed."""
    rng = np.random.default_rng(n)
    reload(solver, [CORPUS[k] for k in rng.integers(0, len(CORPUS), n)])


def test_grouped_path_planted_models(solver):
    """Eight records per wavefront, with the shapes ic.planted_models names at fixed positions of their wavefronts."""
    vals = ic.planted_models(BIG)
    assert [len(v) for v in vals[16:24]] == [256] * 8 and [len(v) for v in vals[32:40]] == [257] * 8
    assert min(len(vals[48]), len(vals[67]), len(vals[87])) > ic.TILE and vals[98] == b"" and vals[101] == b"{}"
    assert [ic.model_answer(v).status for v in vals[114:117]] == [0, 1, 0]
    assert sum(v.count(b":") for v in vals[128:136]) > 64 and sum(len(v) for v in vals[128:136]) <= ic.TILE
    assert sum(len(a.loaded) + len(a.failed) for a in map(ic.model_answer, vals[144:152])) > 64
    assert sum(len(v) for v in vals[144:152]) <= ic.TILE
    for w in (208, 216, 224):  # fields 63 and 64 of the group are the two duplicates
        assert sum(v.count(b":") for v in vals[w:w + 2]) == 62 and vals[w + 2].count(b'"instanceIds"') == 2
        assert sum(len(v) for v in vals[w:w + 8]) <= ic.TILE
    assert [ic.model_answer(vals[w + 2]).status for w in (208, 216, 224)] == [1, 0, 1]
    reload(solver, vals)


def test_grouped_path_planted_pods():
    ingest_pods(ic.planted_pods(BIG))


# ---- 5. group sizes the host never picks by itself -----------------------------------------------------------------------------

@pytest.mark.parametrize("grp", [3, 7, 8])
def test_odd_group_sizes(grp):
    """MMP_JGROUP is read once per process: a fresh child ingests the first 4 096 records of the planted batches with 3, 7 and 8
    records per wavefront (4 096 records never reach 8 by the host's own choice), then sends the ModelRecords as registry events, which
    must give what the reload gave.  A child that ends by a signal or runs into its time limit fails the test; it is not started again."""
    r = subprocess.run([sys.executable, "-m", "tests.ingest_group_child"], cwd=ROOT, env=dict(os.environ, MMP_JGROUP=str(grp)),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "MMP_JGROUP=%d: 4096 records of each kind, 0 differences" % grp in r.stdout


# ---- 6. five-byte entries ------------------------------------------------------------------------------------------------------

def test_five_byte_entries_and_overclaiming_maps(solver):
    """`"":1,` is an entry of five bytes.  A record of 40 of them parks its entries where a rule of six bytes per entry keeps the
    next records' slots; and a malformed map that announces 40 entries in 97 bytes may park nothing beyond its own slots.  One
    record per wavefront here; ic.planted_models holds the same two records inside the batch of 65 541.  Ten ordinary records
    follow each, and 16 more (over 1 KB) end the batch."""
    five, over = ic.five_byte_record(40), ic.overclaiming_record(40)
    follow = [ic.sized(120, 70 + k, 2, 1) for k in range(26)]
    vals = follow[:3] + [five] + follow[:10] + [over] + follow[10:]
    a = ic.model_answer(five)
    assert a.status == 0 and a.loaded == [(-1, k % 10) for k in range(40)] and ic.model_answer(over).status == 1
    assert sum(len(v) for v in vals[-16:]) > 1024 and min(map(len, follow)) >= 100
    reload(solver, vals)
