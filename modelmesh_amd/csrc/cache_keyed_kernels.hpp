// cache_keyed_kernels.hpp — the stateful per-instance caches BY MODEL ID (mmp_caches_load_keyed_k, mmp_cache_replay_k,
// mmp_cache_read_k, and what mmp_models_retire does to bound caches): runtimeCache is a map from model id to CacheEntry
// (MM.java:2863-2913), so the key of an entry is the registry row its id names, resolved on the device, and what a replay evicts
// comes back as ids — the deregistration that follows each eviction (onEviction -> deregisterModel) goes through
// mmp_registry_ops_k by id.  cache_replay_kernel (cache_kernels.hpp) is unchanged: it reads its mmp_cache_op rows from device
// memory and does not care who wrote their `key` field.
//
//   ckey_ops_kernel       one lane per CALLER op: (masked) FNV-1a over its id, mid_find against the model-id table, then
//                         status and row into the caller-ordered outputs and the key into the staged op at inv[i], its place
//                         in the grouped order the replay kernel reads.  The row is taken AS THE TABLE ANSWERS IT, not through
//                         stkey_live_row: the entry of a deleted record must still be found, read and removed (the janitor's
//                         MMP_COP_REMOVE).  An unknown id gives MMP_CACHE_KEY_UNKNOWN, a key no cache can hold; an INSERTING
//                         op under an unknown id becomes a MMP_COP_GET of that key, which writes exactly the out row the
//                         contract asks for (result 0, no eviction, the state as the preceding op left it).
//   ckey_entries_kernel   one lane per entry of a load: the row into key[e]; the lowest entry whose id is unknown through ONE
//                         atomicMin word (a minimum: whichever lanes race, the word is the same)
//   ckey_len_kernel       one lane per row word (eviction slot / deque entry): the byte length of its id from mid_off, 0 for a
//                         word that names no row (an unused slot's -1, the pseudo-entry's MMP_UNLOADBUF_KEY)
//   rocprim::exclusive_scan over those lengths: n + 1 offsets, the last one the total
//   ckey_gather_kernel    a team of kGatherTeam lanes per id: the bytes of row[i] to out[off[i] ...), lane t the bytes t,
//                         t + kGatherTeam, ... (consecutive lanes, consecutive bytes)
//   ckey_retire_check_kernel / ckey_retire_remap_kernel   one lane per deque slot of the store: the slot's cache by a binary
//                         search of the region offsets, LIVE when its position is below n[c] (the slots behind that are garbage
//                         and are not read); the check atomicMin's the lowest retired row that is a live key, the remap writes
//                         remap[key] over every live key >= 0
//
// Why the op resolver runs in caller order and scatters through the inverse of `order`: the keys go up as the caller gave them,
// in ONE copy, and status / row come out by caller op with no second permutation; grouping the key bytes on the host instead
// would copy every id once more there and still need the permutation for the two outputs.
//
// The keys are staged as rops_keyed_kernel stages them (16-byte chunks into LDS when a workgroup's keys fit kKeyedLdsBytes, read
// where they are otherwise; uniform over the workgroup, same answers).  No scratch; no atomic decides a position: two runs over
// the same state are byte-identical.
#pragma once
#include "cache_kernels.hpp"
#include "registry_ops_keyed_kernels.hpp"

namespace mmp {

constexpr int kGatherTeam = 16;  // lanes that copy one id (ids are tens of bytes)

__device__ __forceinline__ bool ckey_op_keyless(int32_t op)
{
    return op == MMP_COP_UBM_SPACE_IS_READY || op == MMP_COP_UBM_CLAIM_SPACE || op == MMP_COP_UBM_UNLOAD_COMPLETE ||
           op == MMP_COP_UBM_DISCARD_FAILED;
}
__device__ __forceinline__ bool ckey_op_inserts(int32_t op)
{
    return op == MMP_COP_PUT_IF_ABSENT || op == MMP_COP_UBM_INSERT_NEW_ENTRY || op == MMP_COP_UBM_INSERT_FAILED_PLACEHOLDER;
}

struct CkeyOpsArgs {
    const char *keys;    // key i = keys[off[i] - off[0], off[i + 1] - off[0])
    const int32_t *off;  // n + 1 offsets (monotone: checked on the host)
    int32_t n;
    uint64_t hmask;      // MMP_MODEL_ID_HASH_BITS
    VmModels M;          // the model-id table and the resident rows
    const int32_t *inv;  // caller op i is staged op inv[i]
    mmp_cache_op *ops;   // n staged ops in grouped order: `key` is written (and `op` of an insert under an unknown id)
    int32_t *status;     // n words by caller op: MMP_CKEY_*
    int32_t *row;        // n words by caller op: the key the op ran under
};

__global__ __launch_bounds__(kIdTabBlock) void ckey_ops_kernel(CkeyOpsArgs A)
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
    const int32_t q = A.inv[i];
    const int32_t code = A.ops[q].op;
    int32_t st = MMP_CKEY_LIVE, key;
    if (A.ops[q].reserved == MMP_COPK_RAW_KEY)
        key = MMP_UNLOADBUF_KEY;  // (the host has seen that the op carries it)
    else if (ckey_op_keyless(code))
        key = -1;
    else {
        const int32_t o = A.off[i] - o0, len = A.off[i + 1] - A.off[i];
        const char *k = in_lds ? reinterpret_cast<const char *>(staged) + (o - lo) : A.keys + o;
        const int32_t r = mid_find(A.M.ids, fnv1a(k, len) & A.hmask, k, len);
        if (r >= 0 && r < A.M.n_models) {
            key = r;
            if (retire_row_empty(A.M.rows[r])) st = MMP_CKEY_EMPTY_ROW;
        } else {
            key = MMP_CACHE_KEY_UNKNOWN;
            st = MMP_CKEY_UNKNOWN;
            if (ckey_op_inserts(code)) A.ops[q].op = MMP_COP_GET;  // not run: the mesh never loads a model without a record
        }
    }
    A.ops[q].key = key;
    A.status[i] = st;
    A.row[i] = key;
}

struct CkeyEntriesArgs {
    const char *keys;            // as CkeyOpsArgs
    const int32_t *off;
    int32_t n;
    uint64_t hmask;
    VmModels M;
    const uint8_t *is_unloadbuf;  // n bytes or nullptr: entry e is the manager's pseudo-entry, its span is not read
    int32_t *key;                 // n words: the row, MMP_UNLOADBUF_KEY, or -1 for an unknown id
    int32_t *lowest_unknown;      // one word, INT32_MAX before the launch
};

__global__ __launch_bounds__(kIdTabBlock) void ckey_entries_kernel(CkeyEntriesArgs A)
{
    __shared__ uint4 staged[kKeyedLdsBytes / 16];
    const int first = blockIdx.x * kIdTabBlock;
    const int last = min(first + kIdTabBlock, A.n);
    const int32_t o0 = A.off[0];
    const int32_t lo = (A.off[first] - o0) & ~15, hi = A.off[last] - o0;
    const bool in_lds = vkeyed_stage(staged, kKeyedLdsBytes, A.keys, lo, hi);
    __syncthreads();
    const int e = first + threadIdx.x;
    if (e >= A.n) return;
    if (A.is_unloadbuf && A.is_unloadbuf[e]) {
        A.key[e] = MMP_UNLOADBUF_KEY;
        return;
    }
    const int32_t o = A.off[e] - o0, len = A.off[e + 1] - A.off[e];
    const char *k = in_lds ? reinterpret_cast<const char *>(staged) + (o - lo) : A.keys + o;
    int32_t r = mid_find(A.M.ids, fnv1a(k, len) & A.hmask, k, len);
    if (r >= A.M.n_models) r = -1;
    A.key[e] = r;  // (the empty row of a deleted record is a row like any other: the janitor removes such entries)
    if (r < 0) atomicMin(A.lowest_unknown, e);
}

// len[i] = the id bytes of row[i], 0 for a word that names no row; len[n] = 0, so that the scan's last element is the total
__global__ __launch_bounds__(kIdTabBlock) void ckey_len_kernel(const int32_t *__restrict__ row, int32_t n, int32_t n_rows,
                                                               const int32_t *__restrict__ mid_off, int32_t *__restrict__ len)
{
    const int i = blockIdx.x * kIdTabBlock + threadIdx.x;
    if (i > n) return;
    int32_t l = 0;
    if (i < n) {
        const int32_t r = row[i];
        if (r >= 0 && r < n_rows) l = mid_off[r + 1] - mid_off[r];
    }
    len[i] = l;
}

// off = the exclusive scan of len; out has room for off[n] bytes
__global__ __launch_bounds__(kIdTabBlock) void ckey_gather_kernel(const int32_t *__restrict__ row, int32_t n, int32_t n_rows,
                                                                  const int32_t *__restrict__ mid_off, const char *__restrict__ mid_bytes,
                                                                  const int32_t *__restrict__ off, char *__restrict__ out)
{
    const int i = (blockIdx.x * kIdTabBlock + threadIdx.x) / kGatherTeam, t = threadIdx.x & (kGatherTeam - 1);
    if (i >= n) return;
    const int32_t r = row[i];
    if (r < 0 || r >= n_rows) return;
    const int32_t src = mid_off[r], len = mid_off[r + 1] - src, dst = off[i];
    for (int32_t j = t; j < len; j += kGatherTeam) out[dst + j] = mid_bytes[src + j];
}

// the cache of deque slot e: the last c with off[c] <= e (regions may be empty); e < off[n_caches]
__device__ __forceinline__ int ckey_slot_cache(const int32_t *__restrict__ off, int32_t n_caches, int32_t e)
{
    int lo = 0, hi = n_caches;  // off[lo] <= e < off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= e)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// keep[r] == 0: row r is named by the retirement.  *live_key = the lowest such row that is the key of a live entry.
__global__ __launch_bounds__(kRetireBlock) void ckey_retire_check_kernel(CacheStore S, int32_t n_caches, int32_t n_slots, int32_t M,
                                                                         const int32_t *__restrict__ keep, int32_t *__restrict__ live_key)
{
    const int e = blockIdx.x * kRetireBlock + threadIdx.x;
    if (e >= n_slots) return;
    const int c = ckey_slot_cache(S.off, n_caches, e);
    if (e - S.off[c] >= S.n[c]) return;
    const int32_t k = S.key[e];
    if (k >= 0 && k < M && !keep[k]) atomicMin(live_key, k);
}

__global__ __launch_bounds__(kRetireBlock) void ckey_retire_remap_kernel(CacheStore S, int32_t n_caches, int32_t n_slots, int32_t M,
                                                                         const int32_t *__restrict__ remap)
{
    const int e = blockIdx.x * kRetireBlock + threadIdx.x;
    if (e >= n_slots) return;
    const int c = ckey_slot_cache(S.off, n_caches, e);
    if (e - S.off[c] >= S.n[c]) return;
    const int32_t k = S.key[e];
    if (k >= 0 && k < M) S.key[e] = remap[k];  // (MMP_UNLOADBUF_KEY stays as it is)
}

}  // namespace mmp
