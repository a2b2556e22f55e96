// tasks_keyed_kernels.hpp — an instance's periodic tasks BY MODEL ID (mmp_scaleup_plan_k, mmp_scaledown_plan_k,
// mmp_migration_plan_k, mmp_janitor_plan_k): the Java loops iterate runtimeCache, which holds ids, and begin each entry with
// registry.get(modelId) (MM.java:5672-5690 the rate task, :5896-5903 the janitor, :6998-7010 preShutdown), so the key is resolved
// on the device, one launch in front of the unchanged plan kernels (rebalance_kernels.hpp, janitor_kernels.hpp), which read their
// mmp_cache_entry / mmp_janitor_entry rows from device memory and do not care who wrote their `model` field.
//
//   tasks_keyed_kernel<Entry, Claim>   one lane per entry: (masked) FNV-1a over the model id, mid_find against the model-id table,
//                                      the row (or -1) into model_idx[i], and stkey_live_row of it — the row unless it is unknown
//                                      or the EMPTY row a deleted record leaves (retire_row_empty) — into the `model` field of the
//                                      staged entry; the field the caller sent is never read.  Entry: mmp_cache_entry (56 bytes)
//                                      or mmp_janitor_entry (80 bytes); `model` stands at offset 0 in both.
//   TasksNoClaim                       the rate task, the scale-down, the migration: nothing more (entries may repeat a model)
//   TasksJanitorClaim                  the janitor: what the host loop of the by-row call settles before any kernel runs — no
//                                      model has two rows — cannot be left to a host that holds no rows, so the lane CLAIMS its
//                                      resolved row in the model map with atomicCAS(&map[row], -1, i) (rops_count_kernel's
//                                      protocol) and a lost claim counts into JanitorScalars::n_dup; the host refuses the call
//                                      when that is not 0.  The same lane does janitor_entry_kernel's work (the stop index), so
//                                      the keyed janitor has no more launches in front of janitor_count_kernel than the by-row
//                                      one.  Which of two equal keys wins the word is not defined and does not matter: nothing of
//                                      a refused call is returned or applied, and janitor_finish_kernel puts every word this call
//                                      took back to -1 (each entry of a model stores the same -1).  Two equal keys that resolve to
//                                      NO record both become -1 and are not detected: the by-row call accepts several -1 rows too.
//   tasks_unclaim_kernel               the map words back to -1 where no janitor_finish_kernel follows (a run that is shutting
//                                      down evaluates nothing)
//   tasks_conc_gather_kernel           the janitor's scale-down in the same call: candidate j came from input row orow[j], and its
//                                      MaxConcCacheEntry row is conc[orow[j]] — gathered so that scaledown_decide_kernel reads
//                                      conc[j] beside candidate j, as it does for mmp_scaledown_plan_conc
//
// The keys are staged as rops_keyed_kernel stages them: a workgroup's keys are contiguous, its lanes copy them into LDS in
// 16-byte chunks and hash and compare from there, under keyed_resolve_kernel's contract on the staged copy (16-byte aligned,
// kKeyedPad readable bytes behind the last span).  A region that does not fit is read where it is; which of the two happens is
// uniform over the workgroup and the answers are the same.  No scratch, no atomics on positions: two runs over the same state are
// byte-identical.
#pragma once
#include "janitor_kernels.hpp"
#include "status_keyed_kernels.hpp"

namespace mmp {

static_assert(sizeof(mmp_cache_entry) == 56 && sizeof(mmp_janitor_entry) == 80, "the two entry types of the periodic tasks");
static_assert(offsetof(mmp_cache_entry, model) == 0 && offsetof(mmp_janitor_entry, model) == 0, "`model` leads both");

template <class Entry>
struct TasksKeyArgs {
    const char *keys;    // key i = keys[off[i] - off[0], off[i + 1] - off[0])
    const int32_t *off;  // n + 1 offsets (monotone: checked on the host)
    int32_t n;
    uint64_t hmask;      // MMP_MODEL_ID_HASH_BITS
    VmModels M;          // the model-id table and the resident rows
    int32_t *model_idx;  // n words: what mmp_model_ids_resolve answers
    Entry *entries;      // n staged entries: `model` is written, nothing else is touched
};

struct TasksNoClaim {
    __device__ __forceinline__ bool operator()(int, int32_t, const mmp_cache_entry *) const { return false; }
    __device__ __forceinline__ void lost(int) const {}
};

struct TasksJanitorClaim {
    int32_t *map;  // M words, all -1 between runs (model_map_cover)
    JanitorScalars *js;
    mmp_janitor_params p;
    int32_t n;
    // entry i resolved to `row` (-1: no record): true when another entry of the call holds that row
    __device__ __forceinline__ bool operator()(int i, int32_t row, const mmp_janitor_entry *entries) const
    {
        const bool dup = row >= 0 && atomicCAS(&map[row], -1, i) != -1;
        if (janitor_row_class(entries[i], p) == 1) atomicMax(&js->stop_inv, n - i);  // (janitor_entry_kernel's statement)
        return dup;
    }
    __device__ __forceinline__ void lost(int nd) const { atomicAdd(&js->n_dup, nd); }
};

template <class Entry, class Claim>
__global__ __launch_bounds__(kIdTabBlock) void tasks_keyed_kernel(TasksKeyArgs<Entry> A, Claim claim)
{
    __shared__ uint4 staged[kKeyedLdsBytes / 16];
    const int first = blockIdx.x * kIdTabBlock;
    const int last = min(first + kIdTabBlock, A.n);  // (first < n: the grid is div_up(n, kIdTabBlock))
    const int32_t o0 = A.off[0];
    const int32_t lo = (A.off[first] - o0) & ~15, hi = A.off[last] - o0;
    const bool in_lds = vkeyed_stage(staged, kKeyedLdsBytes, A.keys, lo, hi);
    __syncthreads();
    const int i = first + threadIdx.x;
    bool dup = false;
    if (i < A.n) {
        const int32_t o = A.off[i] - o0, len = A.off[i + 1] - A.off[i];
        const char *key = in_lds ? reinterpret_cast<const char *>(staged) + (o - lo) : A.keys + o;
        const int32_t row = mid_find(A.M.ids, fnv1a(key, len) & A.hmask, key, len);
        A.model_idx[i] = row;
        const int32_t live = stkey_live_row(A.M, row);
        A.entries[i].model = live;
        dup = claim(i, live, A.entries);
    }
    const int nd = __popcll(__ballot(dup));
    if (lane_id() == 0 && nd) claim.lost(nd);
}

// every map word the claims of a call took, back to -1 (the entries carry the rows tasks_keyed_kernel wrote)
__global__ void tasks_unclaim_kernel(const mmp_janitor_entry *__restrict__ entries, int32_t n, int32_t *__restrict__ map)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int32_t m = entries[r].model;
    if (m >= 0) map[m] = -1;
}

// out[j] = conc[orow[j]] for the nc candidates the rank kernel placed (orow[j] in [0, n): it is an input row index)
__global__ void tasks_conc_gather_kernel(const mmp_conc_entry *__restrict__ conc, const int32_t *__restrict__ orow, int32_t nc,
                                         mmp_conc_entry *__restrict__ out)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < nc) out[j] = conc[orow[j]];
}

}  // namespace mmp
