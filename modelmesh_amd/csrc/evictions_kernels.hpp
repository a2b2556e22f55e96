// evictions_kernels.hpp — the task body of ModelMesh.onEviction (MM.java:2886-2920) BY MODEL ID (mmp_evictions_k): per victim the
// registry read (loadedTime of this instance: instanceIds first, else loadFailedInstanceIds, :2888-2895), the reload decision
// (:2895, :2918-2920: the clause gate_eval applies, gate_kernel.hpp) and the deregistration (:2913 -> deregisterModel :2940-2958),
// the read and the edit of ONE registry state under one hold of the batch lock.
//
//   evict_stage_kernel   one lane per victim, behind rops_keyed_kernel (which wrote the row its id names, or -1 for an unknown id or
//                        the empty row, into the staged op's `model`): one scan of the row's entries for self_pod
//                        (janitor_find_self, the walk of rops_eval), the output flags, and the op row {MMP_ROP_DEREGISTER, self_pod,
//                        MMP_ROPF_MATCH_TIME, last_used, load_time, load_complete_time} for the unchanged evaluation behind it
//                        (registry_ops_kernels.hpp), which reads its rows from device memory.  The row is read BEFORE the edit:
//                        the apply runs after the evaluation.
//
// No sort, no atomics, no host read between the launches: two runs over the same state are byte-identical.
#pragma once
#include "gate_kernel.hpp"
#include "registry_ops_keyed_kernels.hpp"

namespace mmp {

constexpr int kEvictBlock = 256;

struct EvictStageArgs {
    const mmp_evicted_entry *entries;
    int32_t n;
    int32_t self_pod;
    int64_t now, load_timeout_ms;
    const mmp_model_row *models;
    const int32_t *ent_pod;
    const int64_t *ent_time;
    const StatsAcc *tstats;  // typeSetStats(type) of the committed snapshot, as gate_eval reads them
    int32_t T_rows;
    mmp_registry_op *ops;    // n staged ops: `model` is read, everything else is written
    mmp_evicted_out *outs;   // (status is filled in when the evaluation has run)
};

__global__ __launch_bounds__(kEvictBlock) void evict_stage_kernel(EvictStageArgs A)
{
    const int i = blockIdx.x * kEvictBlock + threadIdx.x;
    if (i >= A.n) return;
    const mmp_evicted_entry e = A.entries[i];
    const int32_t row = A.ops[i].model;
    mmp_evicted_out o{};
    o.loaded_time = -1;
    o.millis_since_last_used = jsub64(A.now, e.last_used);  // :2899
    if (row >= 0) {  // (registry.get(key) != null; the Java of a missing record makes no edit either, :2945)
        const bool failed = e.flags & MMP_EVF_FAILED;  // ce.isFailed(), :2886
        bool in_registry = false;
        if (!failed) {  // :2887
            const mmp_model_row m = A.models[row];
            const JanSelf s = janitor_find_self(m, A.ent_pod, A.ent_time, A.self_pod);
            int64_t loaded_time = 0;
            if (s.li >= 0) {  // :2890
                in_registry = true;
                loaded_time = s.lt;
            } else if (s.fi >= 0) {  // :2891-2893
                in_registry = true;
                loaded_time = s.ft;
            }
            if (in_registry) {  // :2894
                o.flags |= MMP_EVO_IN_REGISTRY;
                o.loaded_time = loaded_time;
                if (reload_overdue(A.now, loaded_time, A.load_timeout_ms)) {  // :2895
                    o.flags |= MMP_EVO_ATTEMPT_RELOAD;
                    const StatsAcc *st = type_stats_row(A.tstats, A.T_rows, m.type);  // :2918
                    if (reload_room_elsewhere((int64_t)st->total_capacity, st->instance_count, (int64_t)st->total_free))  // :2919-2920
                        o.flags |= MMP_EVO_RELOAD;
                }
            }
        }
        if (in_registry || failed) o.flags |= MMP_EVO_LOG;  // :2900
    }
    A.outs[i] = o;
    mmp_registry_op op;  // :2913
    op.model = row;
    op.pod = A.self_pod;
    op.op = MMP_ROP_DEREGISTER;
    op.flags = MMP_ROPF_MATCH_TIME;  // loadTime is the primitive ce.loadTimestamp boxed: never null
    op.last_used = e.last_used;
    op.load_time = e.load_time;
    op.load_complete_time = e.load_complete_time;
    A.ops[i] = op;
}

}  // namespace mmp
