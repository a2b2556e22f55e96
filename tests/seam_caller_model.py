"""The expansion rule of the single-caller route and miss calls (include/mmplace.h: mmp_route_batch_c, mmp_miss_batch_c) as a
program: request i of a call is decided exactly as mmp_route_batch / mmp_miss_batch decide the rows these functions return.
Plain numpy, no library call: the GPU tests feed the existing calls with what comes out of here."""
import numpy as np

from modelmesh_amd import _lib

# which side of a mmp_gate_req each field is
GATE_CALLER_FIELDS = ("self_pod", "cache_capacity", "cache_weighted_size", "cache_oldest_time", "loading_count",
                      "weight_predict_cutoff", "load_timeout_ms", "fresh_lru", "fresh_capacity", "fresh_used", "fresh_count",
                      "fresh_loading_threads", "fresh_in_progress", "fresh_rpm", "last_published")
GATE_ROW_FIELDS = ("model", "excl_off", "n_excl", "explicit_off", "n_explicit", "size_hint", "last_used_time", "loader_predicted",
                   "loaded_time")
assert set(GATE_CALLER_FIELDS) | set(GATE_ROW_FIELDS) | {"flags", "reserved"} == set(_lib.GATE_REQ.names)
assert set(GATE_ROW_FIELDS) | {"flags"} == set(_lib.GATE_REQ_C.names)


def _one(caller, dtype):
    return np.ascontiguousarray(caller, dtype=dtype).reshape(-1)[0]


def expand_gate(caller, gate_reqs_c):
    """SEAM_CALLER row + GATE_REQ_C rows -> GATE_REQ rows."""
    c = _one(caller, _lib.SEAM_CALLER)
    g = np.ascontiguousarray(gate_reqs_c, dtype=_lib.GATE_REQ_C)
    out = np.zeros(len(g), dtype=_lib.GATE_REQ)
    for f in GATE_ROW_FIELDS:
        out[f] = g[f]
    for f in GATE_CALLER_FIELDS:
        out[f] = c[f]
    out["flags"] = np.uint32(c["gate_flags"]) | g["flags"]
    out["reserved"] = 0
    return out


def expand_serve(caller, gate_reqs_c, serve_reqs_c):
    """The serve rows: model and exclusion range are the GATE row's (one MapFilteringSet for both selections)."""
    c = _one(caller, _lib.SEAM_CALLER)
    g = np.ascontiguousarray(gate_reqs_c, dtype=_lib.GATE_REQ_C)
    s = np.ascontiguousarray(serve_reqs_c, dtype=_lib.SERVE_REQ_C)
    assert len(g) == len(s)
    out = np.zeros(len(g), dtype=_lib.SERVE_REQ)
    out["model"], out["self_pod"], out["flags"] = g["model"], c["self_pod"], s["flags"]
    out["local_in_flight"], out["last_invoke_time"] = c["local_in_flight"], c["last_invoke_time"]
    out["assume_completed_ms"] = s["assume_completed_ms"]
    out["excl_off"], out["n_excl"] = g["excl_off"], g["n_excl"]
    out["cnt_off"], out["n_cnt"] = s["cnt_off"], s["n_cnt"]
    return out


def expand_route(caller, gate_reqs_c, serve_reqs_c):
    """-> (GATE_REQ rows, SERVE_REQ rows): the arguments of mmp_route_batch that mmp_route_batch_c answers for."""
    return expand_gate(caller, gate_reqs_c), expand_serve(caller, gate_reqs_c, serve_reqs_c)


def expand_miss(caller, place_caller, gate_reqs_c, place_reqs_c):
    """-> (GATE_REQ rows, PLACE_REQ rows): the arguments of mmp_miss_batch that mmp_miss_batch_c answers for."""
    assert len(gate_reqs_c) == len(place_reqs_c)
    return expand_gate(caller, gate_reqs_c), _lib.join_caller(place_caller, np.ascontiguousarray(place_reqs_c, dtype=_lib.PLACE_REQ_C))


def split_gate(gate_req_row, local_in_flight=0, last_invoke_time=0):
    """One GATE_REQ row -> (SEAM_CALLER[1] holding its caller side, with every flag left on the row; GATE_REQ_C[1])."""
    r = np.ascontiguousarray(gate_req_row, dtype=_lib.GATE_REQ).reshape(-1)[:1]
    c = np.zeros(1, dtype=_lib.SEAM_CALLER)
    for f in GATE_CALLER_FIELDS:
        c[f] = r[f]
    c["local_in_flight"], c["last_invoke_time"] = local_in_flight, last_invoke_time
    return c, request_side(r)


def request_side(gate_reqs):
    """GATE_REQ rows -> their GATE_REQ_C side (all flags stay with the row)."""
    r = np.ascontiguousarray(gate_reqs, dtype=_lib.GATE_REQ)
    g = np.zeros(len(r), dtype=_lib.GATE_REQ_C)
    for f in GATE_ROW_FIELDS + ("flags",):
        g[f] = r[f]
    return g


def serve_request_side(serve_reqs):
    """SERVE_REQ rows -> their SERVE_REQ_C side."""
    r = np.ascontiguousarray(serve_reqs, dtype=_lib.SERVE_REQ)
    s = np.zeros(len(r), dtype=_lib.SERVE_REQ_C)
    for f in ("flags", "cnt_off", "n_cnt", "assume_completed_ms"):
        s[f] = r[f]
    return s
