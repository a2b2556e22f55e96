"""Every host-pointer request call refuses in its own name.

The place / route / miss seams exist in four forms each (rows, single caller, by model id, by vmodel id) that share their argument
test, their range loop and — the forms by id — their state check.  What those shared pieces are handed is the name of the call
the host made: a refusal must begin with it, on the argument test, on the range loop (which names the request too) and on both
paths of the forms by id.
"""
import numpy as np
import pytest

from modelmesh_amd import _lib
from modelmesh_amd._lib import MMP_EINVAL, MMP_ESTATE, ptr
from modelmesh_amd.solver import Solver
from tests import test_keyed_seams_gpu as ks
from tests import test_seam_caller_gpu as sc

pytestmark = pytest.mark.gpu

EXPIRY = sc.EXPIRY
FORMS = ("", "_c", "_ck", "_cv")
SEAMS = ("place", "route", "miss")


def zero_batch(n, pool=1):
    """n all-zero requests of every row type (each range is [0, +0)) and pools of `pool` entries"""
    a = {"now": 0, "caller": np.zeros(1, _lib.SEAM_CALLER), "pcaller": np.zeros(1, _lib.PLACE_CALLER),
         "counters": np.zeros(pool, _lib.SERVE_COUNTER), "xp": np.zeros(pool, np.int32), "xt": np.zeros(pool, np.int64),
         "expl": np.zeros(pool, np.int32), "extra": np.zeros(pool, np.int32), "keys": [b"k"] * max(n, 0)}
    for k, dt in (("greqs", _lib.GATE_REQ), ("sreqs", _lib.SERVE_REQ), ("preqs", _lib.PLACE_REQ), ("greqs_c", _lib.GATE_REQ_C),
                  ("sreqs_c", _lib.SERVE_REQ_C), ("preqs_c", _lib.PLACE_REQ_C), ("ereqs", _lib.EVICT_REQ)):
        a[k] = np.zeros(max(n, 1), dt)
    return a


def compact_batch(b):
    """a batch of test_seam_caller_gpu.make_batch (compact rows) under zero_batch's names"""
    return dict(b, greqs_c=b["greqs"], sreqs_c=b["sreqs"], preqs_c=b["preqs"])


def call(s, seam, form, n, a):
    """mmp_<seam>_batch<form> on the arrays of `a` -> (the call's name, its return code, mmp_last_error)"""
    L, h, now = s.lib, s.h, int(a["now"])
    p = lambda k: ptr(a[k]) if len(a[k]) else None  # noqa: E731
    name, c = f"mmp_{seam}_batch{form}", "_c" if form else ""
    blob, off = Solver.pack_keys(a["keys"][:max(n, 0)])
    keep = [np.zeros(max(n, 1), dt) for dt in (_lib.GATE_OUT, _lib.SERVE_OUT, _lib.PLACE_OUT, _lib.VSEAM_ROW, _lib.EVICT_OUT)]
    gouts, souts, pouts, rows, eouts = (ptr(o) for o in keep)
    keyed = {"": (), "_c": (), "_ck": (blob, ptr(off)), "_cv": (blob, ptr(off), None, None, None)}[form]
    row_out = (rows,) if keyed else ()
    excl = (p("xp"), p("xt"), len(a["xp"]), p("expl"), len(a["expl"]))
    if seam == "place":
        args = (p("pcaller"),) * bool(form) + (p("preqs" + c), n, *keyed, p("extra"), len(a["extra"]), now, pouts, *row_out)
    elif seam == "route":
        args = (p("caller"),) * bool(form) + (p("greqs" + c), p("sreqs" + c), n, *keyed, p("counters"), len(a["counters"]), *excl, now,
                                               EXPIRY, gouts, souts, *row_out)
    elif seam == "miss":
        args = (p("caller"), p("pcaller")) * bool(form) + (p("greqs" + c), p("preqs" + c), n, *keyed, *excl, p("extra"), len(a["extra"]),
                                                            now, EXPIRY, gouts, pouts, *row_out)
    elif seam == "serve":
        args = (p("sreqs"), n, p("counters"), len(a["counters"]), p("xp"), p("xt"), len(a["xp"]), now, souts)
    elif seam == "gate":
        args = (p("greqs"), n, *excl, now, EXPIRY, gouts)
    else:
        assert seam == "evict"
        args = (p("ereqs"), n, now, eouts)
    rc = getattr(L, name)(h, *args)
    return name, rc, (L.mmp_last_error(h) or b"").decode()


@pytest.fixture(scope="module")
def bare():
    s = Solver(1, 1)
    yield s
    s.close()


def test_a_negative_count_is_refused_in_the_name_of_the_call(bare):
    calls = [(seam, form) for seam in SEAMS for form in FORMS] + [("serve", ""), ("gate", ""), ("evict", "")]
    assert len(calls) == 15
    for seam, form in calls:
        name, rc, msg = call(bare, seam, form, -1, zero_batch(2))
        assert rc == MMP_EINVAL and msg.startswith(name + ":"), (name, rc, msg)


# the range that leaves its pool, in the gate row or in the other half's: (rows, count field)
RANGES = {"place": [("preqs", "n_extra")], "route": [("greqs", "n_excl"), ("greqs", "n_explicit"), ("sreqs", "n_cnt")],
          "miss": [("greqs", "n_excl"), ("greqs", "n_explicit"), ("preqs", "n_extra")]}


def test_a_range_past_its_pool_is_refused_in_the_name_of_the_call_and_names_the_request(bare):
    for seam in SEAMS:
        for form in FORMS:
            for rows, field in RANGES[seam]:
                a = zero_batch(2)
                a[rows + ("_c" if form else "")][field][1] = 2  # [0, +2) of a pool of one entry, in the second request
                name, rc, msg = call(bare, seam, form, 2, a)
                assert rc == MMP_EINVAL and msg.startswith(name + ":") and "request 1 " in msg, (name, field, rc, msg)


def test_the_calls_by_id_refuse_a_state_without_ids_in_their_own_name_on_both_paths():
    m = ks.Mesh(seed=4, load_ids=False)
    try:
        for n in (2, 300):  # a slot; staged
            a = compact_batch(dict(sc.head(m.a, n), keys=m.keys))
            for seam in SEAMS:
                for form in ("_ck", "_cv"):
                    name, rc, msg = call(m.s, seam, form, n, a)
                    assert rc == MMP_ESTATE and msg.startswith(name + ":"), (name, n, rc, msg)
    finally:
        m.close()
