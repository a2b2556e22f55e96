"""ctypes binding of libmmplace (include/mmplace.h).

The library is built in-tree by ``__graft_entry__.build()`` (hipcc, gfx950).
There is no Python or CPU implementation behind this module: if the shared
object is missing, import of the solver fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MMP_LIB_PATH") or os.path.join(HERE, "lib", "libmmplace.so")

MMP_OK = 0
MMP_EINVAL, MMP_ENODEVICE, MMP_EHIP, MMP_EORDER, MMP_ESTATE, MMP_ENOMEM = -1, -2, -3, -4, -5, -6
MMP_NONE, MMP_SELF = -1, -2
POD_SHUTTING_DOWN, POD_LIVE, POD_TOMBSTONE = 1, 2, 4
REQ_FAVOUR_SELF = 1
SERVE_EXCLUDE_SELF, SERVE_PREFER_SELF = 1, 2
ANY_TIME = -(2**63)
JAVA_LONG_MAX = 2**63 - 1

# numpy mirrors of the C structs (all naturally aligned, no padding surprises)
POD_ROW = np.dtype(
    [("lru_time", "<i8"), ("capacity", "<i8"), ("used", "<i8"), ("version", "<i8"),
     ("count", "<i4"), ("loading_threads", "<i4"), ("loading_in_progress", "<i4"), ("rpm", "<i4"),
     ("id_order", "<u4"), ("replica_set", "<i4"), ("flags", "<u4"), ("reserved", "<u4")])
MODEL_ROW = np.dtype(
    [("type", "<i4"), ("ent_off", "<i4"), ("n_loaded", "<i4"), ("n_failed", "<i4"), ("last_used", "<i8")])
PLACE_REQ = np.dtype(
    [("model", "<i4"), ("self_pod", "<i4"), ("flags", "<u4"), ("pick", "<u4"), ("last_used", "<i8"),
     ("extra_off", "<i4"), ("n_extra", "<i4"), ("fresh_lru", "<i8"), ("fresh_capacity", "<i8"),
     ("fresh_used", "<i8"), ("fresh_count", "<i4"), ("fresh_rpm", "<i4")])
PLACE_OUT = np.dtype([("chosen", "<i4"), ("best", "<i4"), ("n_candidates", "<i4"), ("hash", "<u4")])
# the single-caller form: the caller's side once per call, 24 bytes per decision
PLACE_CALLER = np.dtype([("self_pod", "<i4"), ("flags", "<u4"), ("fresh_lru", "<i8"), ("fresh_capacity", "<i8"), ("fresh_used", "<i8"),
                         ("fresh_count", "<i4"), ("fresh_rpm", "<i4")])
PLACE_REQ_C = np.dtype([("model", "<i4"), ("pick", "<u4"), ("last_used", "<i8"), ("extra_off", "<i4"), ("n_extra", "<i4")])
assert PLACE_CALLER.itemsize == 40 and PLACE_REQ_C.itemsize == 24
MMP_BAD_REQUEST = -3


def split_caller(reqs):
    """mmp_place_req rows that share one caller -> (PLACE_CALLER[1], PLACE_REQ_C[n]); asserts that they do."""
    reqs = np.ascontiguousarray(reqs, dtype=PLACE_REQ)
    caller = np.zeros(1, dtype=PLACE_CALLER)
    for f in PLACE_CALLER.names:
        assert len(reqs) == 0 or np.all(reqs[f] == reqs[f][0]), f
        if len(reqs):
            caller[f] = reqs[f][0]
    rc = np.zeros(len(reqs), dtype=PLACE_REQ_C)
    for f in PLACE_REQ_C.names:
        rc[f] = reqs[f]
    return caller, rc


def join_caller(caller, reqs_c):
    """The same decisions as mmp_place_req rows."""
    caller = np.asarray(caller).reshape(-1)[0]
    out = np.zeros(len(reqs_c), dtype=PLACE_REQ)
    for f in PLACE_REQ_C.names:
        out[f] = reqs_c[f]
    for f in PLACE_CALLER.names:
        out[f] = caller[f]
    return out
SERVE_REQ = np.dtype(
    [("model", "<i4"), ("self_pod", "<i4"), ("flags", "<u4"), ("local_in_flight", "<i4"),
     ("last_invoke_time", "<i8"), ("assume_completed_ms", "<i8"), ("excl_off", "<i4"), ("n_excl", "<i4"),
     ("cnt_off", "<i4"), ("n_cnt", "<i4")])
SERVE_COUNTER = np.dtype([("pod", "<i4"), ("in_use", "<i4"), ("last_used", "<i8")])
SERVE_OUT = np.dtype([("chosen", "<i4"), ("pad", "<i4"), ("chosen_load_start", "<i8")])
STATS = np.dtype(
    [("total_capacity", "<i8"), ("total_free", "<i8"), ("global_lru", "<i8"),
     ("instance_count", "<i4"), ("model_copy_count", "<i4")])
EVICT_REQ = np.dtype([("cache", "<i4"), ("weight", "<i4"), ("last_used", "<i8")])
EVICT_OUT = np.dtype(
    [("insert_pos", "<i4"), ("n_victims", "<i4"), ("self_evicted", "<i4"), ("pad", "<i4"),
     ("weighted_size", "<i8"), ("oldest_time", "<i8")])

GATE_REQ = np.dtype(
    [("model", "<i4"), ("self_pod", "<i4"), ("flags", "<u4"), ("excl_off", "<i4"), ("n_excl", "<i4"),
     ("explicit_off", "<i4"), ("n_explicit", "<i4"), ("size_hint", "<i4"), ("last_used_time", "<i8"),
     ("cache_capacity", "<i8"), ("cache_weighted_size", "<i8"), ("cache_oldest_time", "<i8"),
     ("loader_predicted", "<i4"), ("loading_count", "<i4"), ("weight_predict_cutoff", "<i4"), ("reserved", "<i4"),
     ("loaded_time", "<i8"), ("load_timeout_ms", "<i8"), ("fresh_lru", "<i8"), ("fresh_capacity", "<i8"),
     ("fresh_used", "<i8"), ("fresh_count", "<i4"), ("fresh_loading_threads", "<i4"), ("fresh_in_progress", "<i4"),
     ("fresh_rpm", "<i4"), ("last_published", "<i8")])
GATE_OUT = np.dtype([("bits", "<u4"), ("initial_size", "<i4")])
assert GATE_REQ.itemsize == 144 and GATE_OUT.itemsize == 8
# the single-caller forms of the route and miss seams (mmp_route_batch_c / mmp_miss_batch_c): the calling instance's side once per
# call, 48 + 24 bytes per route request instead of 144 + 48
SEAM_CALLER = np.dtype(
    [("self_pod", "<i4"), ("gate_flags", "<u4"), ("loading_count", "<i4"), ("weight_predict_cutoff", "<i4"),
     ("cache_capacity", "<i8"), ("cache_weighted_size", "<i8"), ("cache_oldest_time", "<i8"), ("load_timeout_ms", "<i8"),
     ("fresh_lru", "<i8"), ("fresh_capacity", "<i8"), ("fresh_used", "<i8"), ("fresh_count", "<i4"),
     ("fresh_loading_threads", "<i4"), ("fresh_in_progress", "<i4"), ("fresh_rpm", "<i4"), ("last_published", "<i8"),
     ("local_in_flight", "<i4"), ("reserved", "<i4"), ("last_invoke_time", "<i8")])
GATE_REQ_C = np.dtype(
    [("model", "<i4"), ("flags", "<u4"), ("excl_off", "<i4"), ("n_excl", "<i4"), ("explicit_off", "<i4"), ("n_explicit", "<i4"),
     ("size_hint", "<i4"), ("loader_predicted", "<i4"), ("last_used_time", "<i8"), ("loaded_time", "<i8")])
SERVE_REQ_C = np.dtype([("flags", "<u4"), ("cnt_off", "<i4"), ("n_cnt", "<i4"), ("reserved", "<i4"), ("assume_completed_ms", "<i8")])
assert SEAM_CALLER.itemsize == 112 and GATE_REQ_C.itemsize == 48 and SERVE_REQ_C.itemsize == 24
GATE_GO_LOCAL, GATE_FAILURES_BREACHED, GATE_LOCATIONS_BREACHED, GATE_LOCAL_NOT_ALLOWED = 1, 2, 4, 8
GATE_CHURN_REJECT, GATE_EARLY_REJECT, GATE_RELOAD_ELSEWHERE, GATE_SHOULD_PUBLISH = 16, 32, 64, 128

PROACTIVE_INFO = np.dtype(
    [("size_estimate", "<i4"), ("free_count", "<i4"), ("total_count", "<i4"), ("n_candidates", "<i4"),
     ("n_selected", "<i4"), ("error", "<i4"), ("space_to_fill", "<i8"), ("cutoff", "<i8")])
assert PROACTIVE_INFO.itemsize == 40

# mmp_registry_prune (pruneModelRegistry, MM.java:6524-6609)
PRUNE_APPLY, PRUNE_DRY, PRUNE_EDIT_REPAIRED = 1, 2, 1
PRUNE_EDIT = np.dtype([("model", "<i4"), ("n_loaded_after", "<i4"), ("n_failed_after", "<i4"), ("flags", "<u4"),
                       ("removed_off", "<i4"), ("n_removed", "<i4"), ("last_used_after", "<i8")])
PRUNE_REMOVED = np.dtype([("pod", "<i4"), ("failed", "<i4"), ("time", "<i8")])
PRUNE_INFO = np.dtype([("n_edits", "<i4"), ("n_removed", "<i4"), ("n_repaired", "<i4"), ("n_unresolved", "<i4"),
                       ("n_missing_pods", "<i4"), ("n_new_missing", "<i4"), ("truncated", "<i4"), ("reserved", "<i4")])
assert PRUNE_EDIT.itemsize == 32 and PRUNE_REMOVED.itemsize == 16 and PRUNE_INFO.itemsize == 32

# mmp_janitor_plan (janitorTask's cache and registry loops, MM.java:5892-6008, :6014-6108)
JANITOR_APPLY, JANITOR_DRY = 1, 2
JE_DONE, JE_FAILED, JE_STATE_LIVE = 1, 2, 4
(JAN_NONE, JAN_REPAIRED, JAN_REFRESHED, JAN_IN_ORDER, JAN_REMOVED, JAN_REGISTERED, JAN_EXPIRED) = range(7)
(JAN_EDIT_REGISTERED, JAN_EDIT_TIMESTAMP_MISMATCH, JAN_EDIT_REM_LOADED, JAN_EDIT_REM_FAILED, JAN_EDIT_TOUCHED, JAN_EDIT_REPAIRED,
 JAN_EDIT_UNLOAD_SET) = (1, 2, 4, 8, 16, 32, 64)
JANITOR_ENTRY = np.dtype(
    [("model", "<i4"), ("weight", "<i4"), ("last_used", "<i8"), ("load_timestamp", "<i8"), ("load_complete_timestamp", "<i8"),
     ("last_unload_attempt_time", "<i8"), ("interval_count", "<i8"), ("last_heavy_time", "<i8"), ("last_unload_time", "<i8"),
     ("earlier_use_iteration", "<i4"), ("last_used_iteration", "<i4"), ("flags", "<u4"), ("reserved", "<i4")])
JANITOR_PARAMS = np.dtype(
    [("self_pod", "<i4"), ("shutting_down", "<i4"), ("now", "<i8"), ("janitor_freq_secs", "<i8"), ("load_timeout_ms", "<i8"),
     ("min_stale_age_ms", "<i8"), ("load_failure_expiry_ms", "<i8"), ("short_expiry_recent_use_ms", "<i8"),
     ("unload_attempt_recent_ms", "<i8"), ("lastused_age_on_add_ms", "<i8")])
JANITOR_EDIT = np.dtype(
    [("model", "<i4"), ("n_loaded_after", "<i4"), ("n_failed_after", "<i4"), ("flags", "<u4"), ("last_used_after", "<i8"),
     ("last_unload_after", "<i8"), ("inserted_time", "<i8"), ("inserted_pos", "<i4"), ("entry", "<i4")])
JANITOR_INFO = np.dtype([("n_edits", "<i4"), ("n_candidates", "<i4"), ("n_ties", "<i4"), ("stopped_at", "<i4"), ("truncated", "<i4"),
                         ("n_action", "<i4", (7,))])
assert JANITOR_ENTRY.itemsize == 80 and JANITOR_PARAMS.itemsize == 72 and JANITOR_EDIT.itemsize == 48 and JANITOR_INFO.itemsize == 48

# mmp_registry_ops (loadLocal MM.java:5204-5207, the load-failure path :2484-2495, deregisterModel :2948-2958,
# removeLocalModelCopyAsync :6347-6365)
ROPS_APPLY, ROPS_DRY = 1, 2
ROPS_BLOCK = 256  # ops per workgroup of the device pass (csrc/registry_ops_kernels.hpp: kRopsBlock)
(ROP_REGISTER, ROP_LOAD_FAILED, ROP_DEREGISTER, ROP_SCALE_DOWN) = range(4)
ROPF_SHUTTING_DOWN, ROPF_MATCH_TIME = 1, 2
ROP_UNCHANGED, ROP_EDITED = 0, 1
(ROP_EDIT_REM_LOADED, ROP_EDIT_REM_FAILED, ROP_EDIT_PUT_LOADED, ROP_EDIT_PUT_FAILED, ROP_EDIT_REPLACED, ROP_EDIT_TOUCHED,
 ROP_EDIT_UNLOAD_SET) = (1, 2, 4, 8, 16, 32, 64)
REGISTRY_OP = np.dtype([("model", "<i4"), ("pod", "<i4"), ("op", "<i4"), ("flags", "<u4"), ("last_used", "<i8"), ("load_time", "<i8"),
                        ("load_complete_time", "<i8")])
REGISTRY_OP_EDIT = np.dtype([("model", "<i4"), ("op_index", "<i4"), ("n_loaded_after", "<i4"), ("n_failed_after", "<i4"), ("flags", "<u4"),
                             ("inserted_pos", "<i4"), ("last_used_after", "<i8"), ("last_unload_after", "<i8")])
REGISTRY_OPS_INFO = np.dtype([("n_edits", "<i4"), ("n_unchanged", "<i4"), ("truncated", "<i4"), ("reserved", "<i4"),
                              ("n_edited_op", "<i4", (4,)), ("n_unchanged_op", "<i4", (4,)), ("n_entries_added", "<i4"),
                              ("n_entries_removed", "<i4")])
assert REGISTRY_OP.itemsize == 40 and REGISTRY_OP_EDIT.itemsize == 40 and REGISTRY_OPS_INFO.itemsize == 56
# mmp_registry_ops_k: the same by model id, and the fifth kind (the cache-hit loop's drop of its own copy, MM.java:3682-3687)
ROP_DROP_LOCAL = 4
ROP_NO_RECORD = 2  # status byte: the key is unknown or names the empty row (registry.get == null, :2481 / :2945)
REGISTRY_OPS_INFO_K = np.dtype([("n_edits", "<i4"), ("n_unchanged", "<i4"), ("n_no_record", "<i4"), ("truncated", "<i4"),
                                ("n_edited_op", "<i4", (8,)), ("n_unchanged_op", "<i4", (8,)), ("n_entries_added", "<i4"),
                                ("n_entries_removed", "<i4")])
assert REGISTRY_OPS_INFO_K.itemsize == 88
# mmp_evictions_k: onEviction's task body by model id (MM.java:2886-2920)
EVF_FAILED = 1
EVO_IN_REGISTRY, EVO_ATTEMPT_RELOAD, EVO_RELOAD, EVO_LOG = 1, 2, 4, 8
EVICTED_ENTRY = np.dtype([("last_used", "<i8"), ("load_time", "<i8"), ("load_complete_time", "<i8"), ("weight", "<i4"), ("flags", "<u4")])
EVICT_PARAMS = np.dtype([("self_pod", "<i4"), ("reserved", "<i4"), ("now", "<i8"), ("load_timeout_ms", "<i8")])
EVICTED_OUT = np.dtype([("flags", "<u4"), ("status", "<i4"), ("loaded_time", "<i8"), ("millis_since_last_used", "<i8")])
EVICTIONS_INFO = np.dtype([("n_in_registry", "<i4"), ("n_attempt_reload", "<i4"), ("n_reload", "<i4"), ("n_log", "<i4"),
                           ("n_no_record", "<i4"), ("reserved", "<i4"), ("ops", REGISTRY_OPS_INFO_K)])
assert EVICTED_ENTRY.itemsize == 32 and EVICT_PARAMS.itemsize == 24 and EVICTED_OUT.itemsize == 24 and EVICTIONS_INFO.itemsize == 112

# mmp_models_status (getStatus MM.java:3247: the class of :3760-3768, the copy list of makeStatusInfo :3013-3058)
(MST_NOT_FOUND, MST_NOT_LOADED, MST_LOADING_FAILED, MST_ASK) = range(4)
MSTF_MISS = 1
COPY_NOT_CHECKED, COPY_LOADING_FAILED = 0, 1
STATUS_BLOCK = 256       # requests / output entries per workgroup (csrc/status_kernels.hpp: kStatusBlock)
STATUS_WAVE_ROW = 64     # copies a packed lane still ranks on its own (kStatusWaveRow); longer rows take the workgroup path
STATUS_TILE = 1024       # times of one long row staged in LDS at once (kStatusTile)
STATUS_REQ = np.dtype([("model", "<i4"), ("fail_pod", "<i4"), ("flags", "<u4"), ("reserved", "<u4")])
STATUS_ROW = np.dtype([("cls", "<i4"), ("copy_off", "<i4"), ("n_not_checked", "<i4"), ("n_failed", "<i4")])
STATUS_COPY = np.dtype([("pod", "<i4"), ("status", "<i4"), ("time", "<i8")])
assert STATUS_REQ.itemsize == 16 and STATUS_ROW.itemsize == 16 and STATUS_COPY.itemsize == 16

# mmp_registry_census (the registry listener's model counts, MM.java:2807-2854, :6852-6863)
REGISTRY_STATS = np.dtype(
    [("n_models", "<i4"), ("n_loaded", "<i4"), ("n_failed", "<i4"), ("n_loaded_and_failed", "<i4"), ("n_unloaded_used", "<i4"),
     ("n_last_used_max", "<i4"), ("n_entries_loaded", "<i8"), ("n_entries_failed", "<i8"), ("n_entries_unresolved", "<i8"),
     ("copies_hist", "<i4", (5,)), ("max_copies", "<i4")])
REGISTRY_TYPE_STATS = np.dtype([("n_models", "<i4"), ("n_loaded", "<i4"), ("n_failed", "<i4"), ("reserved", "<i4"),
                                ("n_entries_loaded", "<i8")])
assert REGISTRY_STATS.itemsize == 72 and REGISTRY_TYPE_STATS.itemsize == 24

# mmp_pods_events_json (instance-table events by key, handleInstanceTableChange MM.java:1455)
PEV_APPEND = 1
PEV_APPLIED, PEV_MALFORMED, PEV_UNKNOWN = 0, 1, 2  # status_out

# mmp_models_events_json (registry events by key, the registry listener MM.java:628): the status values are those above
MEV_APPEND = 1
# mmp_models_rewrite_json (the write side of the wire format): status_out
MRW_OK, MRW_MALFORMED, MRW_HOST = 0, 1, 2
# mmp_models_register_json (registerModel / deleteModel): request flags, class_out
REGISTER_REQ = np.dtype([("flags", "<u4"), ("reserved", "<i4"), ("initial_cache_timestamp", "<i8")])
assert REGISTER_REQ.itemsize == 16
MREG_LOAD_NOW, MREG_DELETE = 1, 2
(MREG_CREATED, MREG_TOUCHED, MREG_EXISTS, MREG_CONFLICT, MREG_ABSENT, MREG_REFERENCED, MREG_DELETABLE, MREG_MALFORMED,
 MREG_HOST) = range(9)
# mmp_models_refs_json (incRefCount / decRefCount on stored ModelRecord values): request flags, class_out
REFS_REQ = np.dtype([("flags", "<u4"), ("reserved", "<i4"), ("last_used", "<i8")])
assert REFS_REQ.itemsize == 16
MREF_INC, MREF_AUTO_DELETE = 1, 2
(MREFC_SET, MREFC_CREATED, MREFC_DELETE, MREFC_ENSURE_ABSENT, MREFC_NOT_FOUND, MREFC_MALFORMED, MREFC_HOST) = range(7)
# mmp_vmodels_write_json (the record step of updateVModel / deleteVModel / PendingTransition.run): ops, request flags, classes, row flags
VMODEL_WRITE_REQ = np.dtype([("op", "<u4"), ("flags", "<u4")])
VMODEL_WRITE_ROW = np.dtype([("cls", "<i4"), ("flags", "<u4"), ("model", "<i4"), ("target_copy_count", "<i4"), ("dec_model", "<i4", (2,)),
                             ("dec_off", "<i4", (2,)), ("dec_len", "<i4", (2,)), ("last_used", "<i8")])
assert VMODEL_WRITE_REQ.itemsize == 8 and VMODEL_WRITE_ROW.itemsize == 48
VW_SET, VW_DELETE, VW_COMPLETE, VW_FAIL_FLAG = range(4)
(VWQ_UPDATE_ONLY, VWQ_FORCE, VWQ_LOAD_NOW, VWQ_TARGET_EXISTS, VWQ_TARGET_LOADED, VWQ_TARGET_NOT_LOADED, VWQ_FAILED) = (1, 2, 4, 8, 16, 32, 64)
(VWC_CREATED, VWC_UPDATED, VWC_UNCHANGED, VWC_NOT_FOUND, VWC_PRECONDITION, VWC_OWNER_MISMATCH, VWC_NEEDS_TARGET_STATUS, VWC_NOOP,
 VWC_DELETE, VWC_CHANGED, VWC_MALFORMED, VWC_HOST) = range(12)
VWF_IN_TRANSITION, VWF_ACTIVE_SWITCHED, VWF_PREV_ACTIVE_UNKNOWN = 1, 2, 4
# the vmodel table (VModelManager.java:101-110): mmp_vmodels_events_json / _resolve / _transitions / _get / _info
VMEV_APPEND = 1
(VMF_FAILED, VMF_ABSENT, VMF_ACTIVE_NULL, VMF_TARGET_NULL, VMF_OWNER_NULL, VMF_HOST) = (1, 2, 4, 8, 16, 32)
VMRQ_AFTER_STRONG = 1
(VMR_NOT_FOUND, VMR_OK, VMR_STRONG_READ, VMR_TARGET_NOT_FOUND, VMR_HOST) = range(5)
VMW_ACTIVE, VMW_TARGET = 0, 1
VMRF_NULL_ID = 1
VMS_DEFINED, VMS_TRANSITIONING, VMS_TRANSITION_FAILED = range(3)
VMT_NONE, VMT_LOADING, VMT_LOADING_FAILED, VMT_NOT_FOUND = range(4)
VMX_PROMOTE, VMX_ENSURE_LOADED = 0, 1
VMXF_FAILED, VMXF_FROM_EMPTY, VMXF_TO_EMPTY = 1, 2, 4
VMODEL_ANSWER = np.dtype([("cls", "<i4"), ("which", "<i4"), ("vmodel", "<i4"), ("model", "<i4"), ("target_model", "<i4"),
                          ("vstatus", "<i4"), ("target_status", "<i4"), ("flags", "<u4")])
VMODEL_TRANSITION = np.dtype([("vmodel", "<i4"), ("from_model", "<i4"), ("to_model", "<i4"), ("target_count", "<i4"), ("cls", "<i4"),
                              ("flags", "<u4"), ("last_used", "<i8")])
VMODEL_TRANSITIONS_INFO = np.dtype([("n_listed", "<i4"), ("n_promote", "<i4"), ("n_ensure_loaded", "<i4"), ("n_host_skipped", "<i4"),
                                    ("truncated", "<i4"), ("reserved", "<i4")])
VMODELS_STATS = np.dtype([("n_rows", "<i4"), ("n_live", "<i4"), ("arena_bytes", "<i8"), ("live_bytes", "<i8"), ("capacity", "<i4"),
                          ("reserved", "<i4")])
assert VMODEL_ANSWER.itemsize == 32 and VMODEL_TRANSITION.itemsize == 32 and VMODEL_TRANSITIONS_INFO.itemsize == 24
# mmp_vstatus_row: what mmp_vmodels_status answers per vmodel (getVModelStatus, VModelManager.java:505-559); flags = VMF_REPLY bits
VSTATUS_ROW = np.dtype([("cls", "<i4"), ("vmodel", "<i4"), ("model", "<i4"), ("target_model", "<i4"), ("vstatus", "<i4"),
                        ("target_status", "<i4"), ("flags", "<u4"), ("reserved", "<i4")])
assert VSTATUS_ROW.itemsize == 32
VMF_REPLY = VMF_FAILED | VMF_ACTIVE_NULL | VMF_TARGET_NULL | VMF_OWNER_NULL
# mmp_vseam_row: what the request calls by vmodel id answer per request (the shared fields of VMODEL_ANSWER)
VSEAM_ROW = np.dtype([("cls", "<i4"), ("which", "<i4"), ("vmodel", "<i4"), ("model", "<i4"), ("flags", "<u4"), ("reserved", "<i4")])
assert VSEAM_ROW.itemsize == 24
assert VMODELS_STATS.itemsize == 32
# mmp_vmodels_retire: every named row must be ABSENT / the device retires every ABSENT row (no list)
VMRETIRE_ABSENT_ONLY = 1
VMRETIRE_ALL_ABSENT = 2
# mmp_models_retire: every named row must be the empty row a deletion leaves
RETIRE_EMPTY_ONLY = 1
# mmp_pods_retire: every named row must be a tombstone / no referenced registry entry may name a retired instance
PODS_RETIRE_GONE_ONLY = 1
PODS_RETIRE_UNREFERENCED = 2

CACHE_ENTRY = np.dtype(
    [("model", "<i4"), ("weight", "<i4"), ("last_used", "<i8"), ("interval_count", "<i8"), ("last_heavy_time", "<i8"),
     ("last_unload_time", "<i8"), ("earlier_use_iteration", "<i4"), ("last_used_iteration", "<i4"), ("flags", "<u4"),
     ("reserved", "<i4")])
SCALEUP_PARAMS = np.dtype(
    [("self_pod", "<i4"), ("iteration_counter", "<i4"), ("second_copy_max_age_iters", "<i4"),
     ("second_copy_min_age_iters", "<i4"), ("scale_up_rpm_threshold", "<i4"), ("our_rpm", "<i4"), ("now", "<i8"),
     ("last_check_time", "<i8"), ("rate_check_interval_ms", "<i8"), ("second_copy_lru_threshold_ms", "<i8"),
     ("assume_completed_ms", "<i8")])
CONC_ENTRY = np.dtype([("count_and_time_sum", "<i8"), ("prior_sum", "<i8"), ("prior_count", "<i4"), ("max_conc", "<i4"),
                       ("queued_requests", "<i4"), ("reserved", "<i4")])
CONC_OUT = np.dtype([("threshold", "<i4"), ("reset", "<i4"), ("new_prior_sum", "<i8"), ("new_prior_count", "<i4"), ("reserved", "<i4")])
CONC_PARAMS = np.dtype([("dynamic_rpm_scale_constant", "<i8"), ("average_model_parallelism", "<f8")])
CONC_RESULT = np.dtype([("average_model_parallelism", "<f8"), ("exclude_set_rpms", "<i4"), ("model_parallelism_sum", "<i4")])
assert CONC_ENTRY.itemsize == 32 and CONC_OUT.itemsize == 24 and CONC_PARAMS.itemsize == 16 and CONC_RESULT.itemsize == 16
CONC_COUNT_BITS = 21
SCALEUP_OUT = np.dtype([("action", "<i4"), ("copies", "<i4"), ("timestamp", "<i8"), ("new_i1", "<i4"),
                        ("new_i2", "<i4"), ("heavy", "<i4"), ("rpm", "<i4")])
SCALEDOWN_PARAMS = np.dtype(
    [("self_pod", "<i4"), ("shutting_down", "<i4"), ("now", "<i8"), ("last_check_time", "<i8"),
     ("rate_check_interval_ms", "<i8"), ("adjusted_cache_capacity", "<i8"), ("scale_up_rpm_threshold", "<i4"),
     ("reserved", "<i4")])
assert CACHE_ENTRY.itemsize == 56 and SCALEUP_PARAMS.itemsize == 64 and SCALEUP_OUT.itemsize == 32
assert SCALEDOWN_PARAMS.itemsize == 48

CACHE_OP = np.dtype([("cache", "<i4"), ("op", "<i4"), ("key", "<i4"), ("arg", "<i4"), ("time", "<i8"), ("flag", "<i4"),
                     ("reserved", "<i4")])
CACHE_OP_OUT = np.dtype([("result", "<i4"), ("n_evicted", "<i4"), ("evicted_off", "<i4"), ("buffer_weight", "<i4"),
                         ("weighted_size", "<i8"), ("oldest_time", "<i8")])
UBM_STATE = np.dtype([("reserved", "<i4"), ("total_unloading", "<i4"), ("total_occupancy", "<i8"),
                      ("cache_deficit", "<i4"), ("pad", "<i4")])
assert CACHE_OP.itemsize == 32 and CACHE_OP_OUT.itemsize == 32 and UBM_STATE.itemsize == 24
UNLOADBUF_KEY = -1000000
(COP_PUT_IF_ABSENT, COP_GET, COP_UPDATE_WEIGHT, COP_REMOVE, COP_UBM_INSERT_NEW_ENTRY, COP_UBM_ADJUST_SPACE_REQUEST,
 COP_UBM_SPACE_IS_READY, COP_UBM_CLAIM_SPACE, COP_UBM_ADJUST_AFTER_LOAD, COP_UBM_UNLOAD_COMPLETE, COP_UBM_REMOVE_ENTRY,
 COP_UBM_DISCARD_FAILED, COP_UBM_INSERT_FAILED_PLACEHOLDER) = range(13)
# the caches by model id (mmp_caches_load_keyed_k, mmp_cache_replay_k, mmp_cache_read_k)
COPK_RAW_KEY = 1  # mmp_cache_op.reserved: the op keeps its key, which must be UNLOADBUF_KEY
CKEY_LIVE, CKEY_EMPTY_ROW, CKEY_UNKNOWN = range(3)
CACHE_KEY_UNKNOWN = -(2 ** 31)
COP_KEYLESS = (COP_UBM_SPACE_IS_READY, COP_UBM_CLAIM_SPACE, COP_UBM_UNLOAD_COMPLETE, COP_UBM_DISCARD_FAILED)
COP_INSERTING = (COP_PUT_IF_ABSENT, COP_UBM_INSERT_NEW_ENTRY, COP_UBM_INSERT_FAILED_PLACEHOLDER)

assert POD_ROW.itemsize == 64 and MODEL_ROW.itemsize == 24 and PLACE_REQ.itemsize == 64
assert PLACE_OUT.itemsize == 16 and SERVE_REQ.itemsize == 48 and SERVE_COUNTER.itemsize == 16 and SERVE_OUT.itemsize == 16
assert STATS.itemsize == 32 and EVICT_REQ.itemsize == 16 and EVICT_OUT.itemsize == 32


class MmpConfig(C.Structure):
    _fields_ = [("device", C.c_int32), ("reserved0", C.c_int32),
                ("min_space_units", C.c_int64), ("min_churn_age_ms", C.c_int64)]


# every symbol include/mmplace.h declares: (name, restype, argtypes)
_P = C.c_void_p
SYMBOLS = [
    ("mmp_abi_version", C.c_int, []),
    ("mmp_create", C.c_int, [C.POINTER(MmpConfig), C.POINTER(_P)]),
    ("mmp_destroy", None, [_P]),
    ("mmp_last_error", C.c_char_p, [_P]),
    ("mmp_backend", C.c_int, [_P]),
    ("mmp_min_space_units", C.c_int64, [C.c_int32, C.c_int32, C.c_int64, C.c_int]),
    ("mmp_pods_load", C.c_int, [_P, _P, C.c_int32]),
    ("mmp_pods_upsert", C.c_int, [_P, _P, _P, C.c_int32]),
    ("mmp_pods_remove", C.c_int, [_P, _P, C.c_int32]),
    ("mmp_types_load", C.c_int, [_P, C.c_int32, _P, _P, _P, _P]),
    ("mmp_types_from_labels", C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P, _P]),
    ("mmp_replaced_rs_load", C.c_int, [_P, _P, C.c_int32]),
    ("mmp_upgrade_instance_added", C.c_int, [_P, C.c_int64, C.c_int32, C.c_int64, C.c_int64]),
    ("mmp_upgrade_instance_removed", C.c_int, [_P, C.c_int64, C.c_int32, C.c_int64]),
    ("mmp_upgrade_housekeeping", C.c_int, [_P, C.c_int64]),
    ("mmp_upgrade_replaced", C.c_int, [_P, _P, _P, C.c_int32, C.POINTER(C.c_int32)]),
    ("mmp_models_load", C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int32]),
    ("mmp_models_upsert", C.c_int, [_P, _P, _P, C.c_int32, _P, _P, C.c_int32]),
    ("mmp_snapshot_commit", C.c_int, [_P]),
    ("mmp_get_order", C.c_int, [_P, _P, C.POINTER(C.c_int32)]),
    ("mmp_delta_commits", C.c_int, [_P, C.POINTER(C.c_int64)]),
    ("mmp_shortlists", C.c_int, [_P, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    ("mmp_long_shortlists", C.c_int, [_P, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    ("mmp_split_batches", C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    ("mmp_place_batch_dev2", C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, C.c_int64, _P, _P]),
    ("mmp_place_batch_c", C.c_int, [_P, _P, _P, C.c_int32, _P, C.c_int32, C.c_int64, _P]),
    ("mmp_place_batch_c_dev", C.c_int, [_P, _P, _P, C.c_int32, _P, C.c_int32, C.c_int64, _P, _P]),
    ("mmp_cluster_stats", C.c_int, [_P, _P]),
    ("mmp_type_stats", C.c_int, [_P, C.c_int32, _P]),
    ("mmp_partition_count", C.c_int, [_P, _P]),
    ("mmp_partition_stats", C.c_int, [_P, C.c_int32, _P, _P, C.c_int32]),
    ("mmp_pod_partitions", C.c_int, [_P, _P, C.c_int32, _P]),
    ("mmp_place_batch", C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, C.c_int64, _P]),
    ("mmp_place_batch_dev", C.c_int, [_P, _P, C.c_int32, _P, C.c_int64, _P, _P]),
    ("mmp_place_multi_dev", C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_int64, _P, _P]),
    ("mmp_stream_retire", C.c_int, [_P, _P]),
    ("mmp_resident", C.c_int, [_P, C.c_int]),
    ("mmp_resident_stats", C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("mmp_issue_threads", C.c_int, [_P, C.c_int32]),
    ("mmp_issue_flush", C.c_int, [_P]),
    ("mmp_serve_batch", C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, _P, _P, C.c_int32, C.c_int64, _P]),
    ("mmp_caches_load", C.c_int, [_P, C.c_int32, _P, _P, _P, _P]),
    ("mmp_evict_batch", C.c_int, [_P, _P, C.c_int32, C.c_int64, _P]),
    ("mmp_caches_load_keyed", C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P]),
    ("mmp_cache_replay", C.c_int, [_P, _P, C.c_int32, C.c_int64, _P, _P, C.c_int32, C.POINTER(C.c_int32)]),
    ("mmp_cache_read", C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P, C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                                 C.POINTER(C.c_int64), _P]),
    ("mmp_caches_load_keyed_k", C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    ("mmp_cache_replay_k", C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int64, _P, _P, _P, _P, C.c_int32, C.POINTER(C.c_int32), _P, C.c_int32,
                                     _P, C.POINTER(C.c_int32)]),
    ("mmp_cache_evicted_ids", C.c_int, [_P, _P, C.c_int32, _P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("mmp_cache_replay_kt", C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int64, _P, _P, _P, _P, C.c_int32, C.POINTER(C.c_int32), _P, C.c_int32,
                                      _P, C.POINTER(C.c_int32), _P]),
    ("mmp_cache_evicted_times", C.c_int, [_P, _P, C.c_int32, C.POINTER(C.c_int32)]),
    ("mmp_cache_read_k", C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int32, _P, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                   C.POINTER(C.c_int64), C.POINTER(C.c_int64), _P]),
    ("mmp_gate_batch", C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int32, _P, C.c_int32, C.c_int64, C.c_int64, _P]),
    ("mmp_miss_batch", C.c_int, [_P, _P, _P, C.c_int32, _P, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32, C.c_int64, C.c_int64, _P, _P]),
    ("mmp_route_batch", C.c_int, [_P, _P, _P, C.c_int32, _P, C.c_int32, _P, _P, C.c_int32, _P, C.c_int32, C.c_int64, C.c_int64, _P, _P]),
    ("mmp_route_batch_c", C.c_int, [_P, _P, _P, _P, C.c_int32, _P, C.c_int32, _P, _P, C.c_int32, _P, C.c_int32, C.c_int64, C.c_int64,
                                    _P, _P]),
    ("mmp_miss_batch_c", C.c_int, [_P, _P, _P, _P, _P, C.c_int32, _P, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32, C.c_int64,
                                   C.c_int64, _P, _P]),
    # the same three by model id: keys / key_off behind n, model_idx_out last
    ("mmp_place_batch_ck", C.c_int, [_P, _P, _P, C.c_int32, _P, _P, _P, C.c_int32, C.c_int64, _P, _P]),
    ("mmp_route_batch_ck", C.c_int, [_P, _P, _P, _P, C.c_int32, _P, _P, _P, C.c_int32, _P, _P, C.c_int32, _P, C.c_int32, C.c_int64,
                                     C.c_int64, _P, _P, _P]),
    ("mmp_miss_batch_ck", C.c_int, [_P, _P, _P, _P, _P, C.c_int32, _P, _P, _P, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32,
                                    C.c_int64, C.c_int64, _P, _P, _P]),
    ("mmp_proactive_plan",C.c_int, [_P, C.c_int32, C.c_int64, C.c_int32, _P, _P, _P]),
    ("mmp_proactive_plan_subset", C.c_int, [_P, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int64, C.c_int32, _P, _P, _P]),
    ("mmp_registry_prune", C.c_int, [_P, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_uint32, _P, C.c_int32, _P, C.c_int32, _P]),
    ("mmp_registry_missing_get", C.c_int, [_P, _P, C.c_int32, C.POINTER(C.c_int32)]),
    ("mmp_registry_missing_reset", C.c_int, [_P]),
    ("mmp_janitor_plan", C.c_int, [_P, _P, C.c_int32, _P, C.c_uint32, _P, _P, C.c_int32, _P, _P, C.c_int32, _P]),
    ("mmp_registry_ops", C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_uint32, _P, _P, C.c_int32, _P]),
    # the same by model id: ops / n, keys / key_off, now, flags, model_idx_out, status_out, edits_out, max_edits, info_out
    ("mmp_registry_ops_k", C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int64, C.c_uint32, _P, _P, _P, C.c_int32, _P]),
    ("mmp_evictions_k", C.c_int, [_P, _P, C.c_int32, _P, _P, _P, C.c_uint32, _P, _P, _P, _P, C.c_int32, _P]),
    ("mmp_models_status", C.c_int, [_P, _P, C.c_int32, C.c_int64, _P, _P, C.c_int32, C.POINTER(C.c_int32)]),
    # the same by model id: keys / key_off / n, fail_pod[n], flags[n], now, model_idx_out, then the outputs of mmp_models_status
    ("mmp_models_status_k", C.c_int, [_P, _P, _P, C.c_int32, _P, _P, C.c_int64, _P, _P, _P, C.c_int32, C.POINTER(C.c_int32)]),
    # getVModelStatus: keys / key_off / n, owners / owner_off, req_flags, now, vrows, rows[2n], copies, strings
    ("mmp_vmodels_status", C.c_int, [_P, _P, _P, C.c_int32, _P, _P, _P, C.c_int64, _P, _P, _P, C.c_int32, C.POINTER(C.c_int32), _P,
                                     C.c_int32, _P, C.POINTER(C.c_int32)]),
    ("mmp_registry_census", C.c_int, [_P, _P, _P, _P, C.c_int32, C.POINTER(C.c_int32), _P, C.c_int32, C.POINTER(C.c_int32)]),
    ("mmp_scaleup_plan", C.c_int, [_P, _P, C.c_int32, _P, _P, _P, C.POINTER(C.c_int32)]),
    ("mmp_scaledown_plan", C.c_int, [_P, _P, C.c_int32, _P, _P]),
    ("mmp_scaleup_plan_conc", C.c_int, [_P, _P, _P, C.c_int32, _P, _P, _P, _P, _P, C.POINTER(C.c_int32), _P]),
    ("mmp_scaledown_plan_conc", C.c_int, [_P, _P, _P, C.c_int32, _P, C.c_int64, _P]),
    ("mmp_migration_plan", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int64, C.c_int64, _P, _P]),
    # the periodic tasks by model id: the by-row argument lists with keys / key_off behind n and model_idx_out at the end
    # entries, conc, n, keys, key_off, params, conc_params, outs, conc_outs, overloaded_out, skipped, result, model_idx_out
    ("mmp_scaleup_plan_k", C.c_int, [_P, _P, _P, C.c_int32, _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_int32), _P, _P]),
    # entries, conc, n, keys, key_off, params, dynamic_rpm_scale_constant, removed_out, model_idx_out
    ("mmp_scaledown_plan_k", C.c_int, [_P, _P, _P, C.c_int32, _P, _P, _P, C.c_int64, _P, _P]),
    # entries, n, keys, key_off, self_pod, now, cutoff_age_ms, action_out, wait_out, model_idx_out
    ("mmp_migration_plan_k", C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int32, C.c_int64, C.c_int64, _P, _P, _P]),
    # entries, n, keys, key_off, params, flags, scaledown, conc, dynamic_rpm_scale_constant, model_idx_out, actions_out, edits_out,
    # max_edits, candidates_out, candidate_rows_out, max_candidates, removed_out, info_out
    ("mmp_janitor_plan_k", C.c_int, [_P, _P, C.c_int32, _P, _P, _P, C.c_uint32, _P, _P, C.c_int64, _P, _P, _P, C.c_int32, _P, _P,
                                     C.c_int32, _P, _P]),
    ("mmp_pod_ids_load", C.c_int, [_P, _P, _P, C.c_int32, _P, _P]),
    ("mmp_pods_ingest_json", C.c_int, [_P, _P, _P, C.c_int32, _P, _P, _P, _P]),
    ("mmp_type_names_load", C.c_int, [_P, _P, _P, C.c_int32, C.c_int32]),
    ("mmp_models_ingest_json", C.c_int, [_P, _P, _P, C.c_int32, _P, _P]),
    ("mmp_models_upsert_json", C.c_int, [_P, _P, _P, C.c_int32, _P, _P, _P, _P]),
    ("mmp_pod_ids_append", C.c_int, [_P, _P, _P, C.c_int32, _P, _P, C.c_int32]),
    ("mmp_pods_events_json", C.c_int, [_P, _P, _P, _P, _P, C.c_int32, _P, _P, C.c_uint32, _P, _P, _P, C.POINTER(C.c_int32)]),
    ("mmp_registry_unresolved", C.c_int, [_P, _P, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    ("mmp_label_names_load", C.c_int, [_P, _P, _P, C.c_int32]),
    ("mmp_pod_labels_set", C.c_int, [_P, _P, _P, _P, C.c_int32]),
    ("mmp_pod_labels_get", C.c_int, [_P, _P, _P, C.c_int32, C.POINTER(C.c_int32)]),
    ("mmp_types_from_pod_labels", C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P]),
    ("mmp_model_ids_load", C.c_int, [_P, _P, _P, C.c_int32]),
    ("mmp_model_ids_resolve", C.c_int, [_P, _P, _P, C.c_int32, _P]),
    ("mmp_model_ids_get", C.c_int, [_P, C.c_int32, C.c_int32, _P, C.c_int32, _P, C.POINTER(C.c_int32)]),
    ("mmp_models_events_json", C.c_int, [_P, _P, _P, _P, _P, C.c_int32, _P, C.c_uint32, _P, _P, _P, C.POINTER(C.c_int32)]),
    ("mmp_models_retire", C.c_int, [_P, _P, C.c_int32, C.c_uint32, _P, C.c_int32, C.POINTER(C.c_int32)]),
    ("mmp_pods_retire", C.c_int, [_P, _P, C.c_int32, C.c_uint32, _P, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    ("mmp_models_rewrite_json", C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P, _P, _P, C.c_uint32, _P, C.c_int64, _P, _P,
                                          C.POINTER(C.c_int64)]),
    ("mmp_models_register_json", C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P, _P, _P, C.c_int64, C.c_int64, C.c_uint32, _P, C.c_int64,
                                           _P, _P, _P, _P, C.POINTER(C.c_int64)]),
    ("mmp_vmodels_events_json", C.c_int, [_P, _P, _P, _P, _P, C.c_int32, _P, C.c_uint32, _P, _P, C.POINTER(C.c_int32)]),
    ("mmp_vmodels_resolve", C.c_int, [_P, _P, _P, C.c_int32, _P, _P, _P, _P, _P, _P]),
    # the request calls by vmodel id: the _ck signatures with nf_keys / nf_off / req_flags behind key_off, vm_out last
    ("mmp_place_batch_cv", C.c_int, [_P, _P, _P, C.c_int32, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int64, _P, _P]),
    ("mmp_route_batch_cv", C.c_int, [_P, _P, _P, _P, C.c_int32, _P, _P, _P, _P, _P, _P, C.c_int32, _P, _P, C.c_int32, _P, C.c_int32,
                                     C.c_int64, C.c_int64, _P, _P, _P]),
    ("mmp_miss_batch_cv", C.c_int, [_P, _P, _P, _P, _P, C.c_int32, _P, _P, _P, _P, _P, _P, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32,
                                    C.c_int64, C.c_int64, _P, _P, _P]),
    ("mmp_vmodels_transitions", C.c_int, [_P, C.c_int64, C.c_int64, _P, C.c_int32, C.POINTER(C.c_int32), _P]),
    ("mmp_vmodels_get", C.c_int, [_P, C.c_int32, C.c_int32, _P, C.c_int32, _P, C.POINTER(C.c_int32), _P, _P, C.c_int32, _P,
                                  C.POINTER(C.c_int32)]),
    ("mmp_vmodels_info", C.c_int, [_P, _P]),
    ("mmp_vmodels_retire", C.c_int, [_P, _P, C.c_int32, C.c_uint32, _P, C.c_int32, C.POINTER(C.c_int32)]),
    ("mmp_models_refs_json", C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P, C.c_uint32, _P, C.c_int64, _P, _P, _P,
                                       C.POINTER(C.c_int64)]),
    ("mmp_vmodels_write_json", C.c_int, [_P, _P, C.c_int32, _P, _P, _P, C.c_int32, _P, _P, C.c_int64, C.c_int64, C.c_uint32, _P, C.c_int64,
                                         _P, _P, C.POINTER(C.c_int64)]),
    ("mmp_pods_get", C.c_int, [_P, _P, C.c_int32, C.POINTER(C.c_int32)]),
    ("mmp_models_get", C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("mmp_shard_configure", C.c_int, [_P, C.c_int32, C.c_int32]),
    ("mmp_shard_xchg_slots", C.c_int32, [C.c_int32, C.c_int32]),
    ("mmp_shard_xchg_is_sum", C.c_int32, [C.c_int32]),
    ("mmp_shard_rank_dev", C.c_int, [_P, _P]),
    ("mmp_shard_commit_dev", C.c_int, [_P, _P]),
    ("mmp_shard_place_phase_dev", C.c_int, [_P, C.c_int32, _P, C.c_int32, _P, C.c_int64, _P, _P, _P]),
    ("mmp_shard_fast_slots", C.c_int32, []),
    ("mmp_shard_place_fast_dev", C.c_int, [_P, _P, C.c_int32, _P, C.c_int64, _P, _P]),
    ("mmp_shard_place_fast_finish_dev", C.c_int, [_P, _P, C.c_int32, _P, _P, _P, C.POINTER(C.c_int32), C.POINTER(C.c_void_p),
                                                  C.POINTER(C.c_void_p)]),
    ("mmp_shard_place_fast_scatter_dev", C.c_int, [_P, C.c_int32, _P, _P]),
    ("mmp_shard_unique_id", C.c_int, [_P]),
    ("mmp_shard_group_set_exchange", C.c_int, [_P, _P, _P]),
    ("mmp_shard_group_init", C.c_int, [_P, _P, C.c_int32, C.c_int32]),
    ("mmp_shard_group_destroy", C.c_int, [_P]),
    ("mmp_shard_commit", C.c_int, [_P]),
    ("mmp_shard_place_batch", C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, C.c_int64, _P, C.POINTER(C.c_int32)]),
    ("mmp_shard_place_batch_dev", C.c_int, [_P, _P, C.c_int32, _P, C.c_int64, _P, C.POINTER(C.c_int32)]),
    ("mmp_shard_place_batch_async_dev", C.c_int, [_P, _P, C.c_int32, _P, C.c_int64, _P]),
    ("mmp_shard_wait", C.c_int, [_P, C.POINTER(C.c_int32)]),
    ("mmp_sync", C.c_int, [_P]),
    ("mmp_profile", C.c_int, [_P, C.c_int]),
    ("mmp_last_kernel_ms", C.c_double, [_P]),
]

_lib = None


def load() -> C.CDLL:
    """dlopen libmmplace.so and type every exported entry point."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build the HIP library first "
            "(python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback.")
    # One HIP runtime per process.  PyTorch wheels bundle their own libamdhip64 / libhsa-runtime64; if
    # /opt/rocm's copy (libmmplace's DT_NEEDED) initialises first, torch later reports "No HIP GPUs are
    # available".  Python hosts of this library use torch for device buffers and collectives, so let
    # torch's runtime load first; libmmplace then binds to the same, already loaded, runtime.
    if os.environ.get("MMP_NO_TORCH_PRELOAD") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    lib = C.CDLL(LIB_PATH)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)  # AttributeError here == a header symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def ptr(a):
    """void* of a numpy array (None -> NULL)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)
