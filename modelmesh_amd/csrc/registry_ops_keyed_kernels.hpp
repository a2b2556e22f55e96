// registry_ops_keyed_kernels.hpp — the edits an instance makes to ModelRecords itself BY MODEL ID (mmp_registry_ops_k): the Java
// sites begin with registry.get(modelId) / getOrStrongIfAbsent(modelId) and return when that is null (MM.java:2481, :2945), so the
// key is resolved on the device, one launch in front of the unchanged evaluation (registry_ops_kernels.hpp), which reads its
// mmp_registry_op rows from device memory and does not care who wrote their `model` field.
//
//   rops_keyed_kernel   one lane per op: (masked) FNV-1a over the model id, mid_find against the model-id table, the row (or -1)
//                       into model_idx[i], and stkey_live_row of it — the row unless it is unknown or the EMPTY row a deleted
//                       record leaves (retire_row_empty) — into the `model` field of the staged op; the field the caller sent is
//                       never read
//
// The keys are staged as status_keyed_kernel stages them: a workgroup's keys are contiguous, its lanes copy them into LDS in
// 16-byte chunks and hash and compare from there, under keyed_resolve_kernel's contract on the staged copy (16-byte aligned,
// kKeyedPad readable bytes behind the last span).  A region that does not fit is read where it is; which of the two happens is
// uniform over the workgroup and the answers are the same.  No scratch, no atomics: two runs over the same state are byte-identical.
#pragma once
#include "registry_ops_kernels.hpp"
#include "status_keyed_kernels.hpp"

namespace mmp {

struct RopsKeyArgs {
    const char *keys;      // key i = keys[off[i] - off[0], off[i + 1] - off[0])
    const int32_t *off;    // n + 1 offsets (monotone: checked on the host)
    int32_t n;
    uint64_t hmask;        // MMP_MODEL_ID_HASH_BITS
    VmModels M;            // the model-id table and the resident rows
    int32_t *model_idx;    // n words: what mmp_model_ids_resolve answers
    mmp_registry_op *ops;  // n staged ops: `model` is written, nothing else is touched
};

__global__ __launch_bounds__(kIdTabBlock) void rops_keyed_kernel(RopsKeyArgs A)
{
    __shared__ uint4 staged[kKeyedLdsBytes / 16];
    const int first = blockIdx.x * kIdTabBlock;
    const int last = min(first + kIdTabBlock, A.n);  // (first < n: the grid is div_up(n, kIdTabBlock))
    const int32_t o0 = A.off[0];
    const int32_t lo = (A.off[first] - o0) & ~15, hi = A.off[last] - o0;
    const bool in_lds = vkeyed_stage(staged, kKeyedLdsBytes, A.keys, lo, hi);
    __syncthreads();
    const int i = first + threadIdx.x;
    if (i >= A.n) return;
    const int32_t o = A.off[i] - o0, len = A.off[i + 1] - A.off[i];
    const char *key = in_lds ? reinterpret_cast<const char *>(staged) + (o - lo) : A.keys + o;
    const int32_t row = mid_find(A.M.ids, fnv1a(key, len) & A.hmask, key, len);
    A.model_idx[i] = row;
    A.ops[i].model = stkey_live_row(A.M, row);
}

}  // namespace mmp
