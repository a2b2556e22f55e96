// status_keyed_kernels.hpp — the management path's two status questions BY ID (mmp_models_status_k, mmp_vmodels_status): getStatus by
// model id (MM.java:3247-3263) and getVModelStatus in full (VModelManager.java:505-559), each one launch in front of the unchanged
// status pipeline (status_kernels.hpp), which reads its mmp_status_req rows from device memory and does not care who wrote them.
//
//   status_keyed_kernel     one lane per key: (masked) FNV-1a over the model id, mid_find against the model-id table, the row (or
//                           -1) into model_idx[i], and the request {r, fail_pod, flags, 0} where r is that row unless it is unknown
//                           or the EMPTY row (retire_row_empty: what a deleted record leaves, :3257 mr == null)
//   vstatus_keyed_kernel    one lane per vmodel key: the key looked up in the vmodel-id table, absentOrOwnerMismatch (:530-532) by
//                           vm_choose, the rows of amid / tmid by vm_model_of, the classes of :555-556 and :537-549 by vm_status_of
//                           — the statements of vmodel_kernels.hpp, not restated —, then the mmp_vstatus_row, the two requests of
//                           the reply (active: row 2i, :513; target: row 2i + 1, :537-549, asked only in transition) and the
//                           lengths of the reply's three strings; the strong read of :514-525 is a class (MMP_VMR_STRONG_READ)
//   rocprim::exclusive_scan over the 3n + 1 lengths: where each string goes, and the total
//   vstatus_strings_kernel  one lane per string, behind the one read-back of the sizes: the bytes from the vmodel string arena
//
// The keys.  A workgroup's keys are contiguous: its lanes copy them into LDS in 16-byte chunks and hash and compare from there, under
// keyed_resolve_kernel's contract on the staged copy (16-byte aligned, kKeyedPad readable bytes behind the last span).  The vmodel
// form stages the owners the same way, half the LDS each (vkeyed_stage).  A region that does not fit is read where it is, byte by
// byte; which of the two happens is uniform over the workgroup and the answers are the same.  No scratch, no atomic decides a
// position (the one atomic is an integer sum, the same in any order): two runs over the same state are byte-identical.
#pragma once
#include "status_kernels.hpp"
#include "vkeyed_kernels.hpp"

namespace mmp {

// the row a status request names for the table's row `row`: -1 for an unknown id and for the empty row (a deleted record's
// getStatus is SI_NOT_FOUND, :3257; what mmp_vmodels_resolve treats as "not found" for a target)
__device__ __forceinline__ int32_t stkey_live_row(const VmModels &M, int32_t row)
{
    return row >= 0 && row < M.n_models && !retire_row_empty(M.rows[row]) ? row : -1;
}

struct StKeyArgs {
    const char *keys;         // key i = keys[off[i] - off[0], off[i + 1] - off[0])
    const int32_t *off;       // n + 1 offsets (monotone: checked on the host)
    int32_t n;
    uint64_t hmask;           // MMP_MODEL_ID_HASH_BITS
    VmModels M;               // the model-id table and the resident rows
    const int32_t *fail_pod;  // n words, or nullptr: all -1 (ranges checked on the host)
    const uint32_t *flags;    // n words, or nullptr: all 0
    int32_t *model_idx;       // n words: what mmp_model_ids_resolve answers
    mmp_status_req *reqs;     // n rows: what status_count_kernel reads
};

__global__ __launch_bounds__(kIdTabBlock) void status_keyed_kernel(StKeyArgs A)
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
    A.reqs[i] = mmp_status_req{stkey_live_row(A.M, row), A.fail_pod ? A.fail_pod[i] : -1, A.flags ? A.flags[i] : 0u, 0u};
}

struct VStKeyScalars {
    unsigned long long n_str_bytes;  // the 64-bit total: the int32 offsets are only used when it fits
};

struct VStKeyArgs {
    const char *keys;          // key i = keys[off[i] - off[0], off[i + 1] - off[0]): the vmodel id
    const int32_t *off;        // n + 1 offsets (monotone: checked on the host)
    const char *owners;        // owner i likewise; an empty span is Java null (emptyToNull, :506)
    const int32_t *owner_off;  // n + 1 offsets, or nullptr: no owner is given
    const uint32_t *flags;     // n words (MMP_VMRQ_AFTER_STRONG), or nullptr: all 0
    int32_t n;
    uint64_t hmask;            // MMP_VMODEL_ID_HASH_BITS
    VmTab V;                   // the vmodel table (no vmodel call yet: all zero)
    VmModels M;
    mmp_vstatus_row *vrows;    // n rows
    mmp_status_req *reqs;      // 2n rows: 2i the active model's, 2i + 1 the target's
    int32_t *str_len;          // 3n + 1 words: amid, tmid, o of key i at 3i ..; the last one 0 (the scan's total)
    VStKeyScalars *sc;         // zero before the launch
};

constexpr uint32_t kVmfReply = kVmfFailed | kVmfActiveNull | kVmfTargetNull | kVmfOwnerNull;  // what mmp_vstatus_row::flags carries

__global__ __launch_bounds__(kIdTabBlock) void vstatus_keyed_kernel(VStKeyArgs A)
{
    __shared__ uint4 skeys[kVKeyedLdsBytes / 16], sown[kVKeyedLdsBytes / 16];
    const int first = blockIdx.x * kIdTabBlock;
    const int last = min(first + kIdTabBlock, A.n);  // (first < n: the grid is div_up(n, kIdTabBlock))
    const int32_t o0 = A.off[0], q0 = A.owner_off ? A.owner_off[0] : 0;
    const int32_t klo = (A.off[first] - o0) & ~15, khi = A.off[last] - o0;
    const int32_t wlo = A.owner_off ? (A.owner_off[first] - q0) & ~15 : 0, whi = A.owner_off ? A.owner_off[last] - q0 : 0;
    const bool k_lds = vkeyed_stage(skeys, kVKeyedLdsBytes, A.keys, klo, khi);
    const bool w_lds = vkeyed_stage(sown, kVKeyedLdsBytes, A.owners, wlo, whi);  // (no owners: no chunk, nothing is read)
    __syncthreads();
    const int i = first + threadIdx.x;
    int64_t bytes = 0;
    if (i < A.n) {
        const int32_t o = A.off[i] - o0, klen = A.off[i + 1] - A.off[i];
        const int32_t q = A.owner_off ? A.owner_off[i] - q0 : 0, olen = A.owner_off ? A.owner_off[i + 1] - A.owner_off[i] : 0;
        const char *key = k_lds ? reinterpret_cast<const char *>(skeys) + (o - klo) : A.keys + o;
        const char *owner = w_lds ? reinterpret_cast<const char *>(sown) + (q - wlo) : A.owners + q;
        const bool after = A.flags && (A.flags[i] & MMP_VMRQ_AFTER_STRONG);
        const int32_t v = mid_find(A.V.ids, fnv1a(key, klen) & A.hmask, key, klen);
        const VmRow r = v >= 0 && v < A.V.n_rows ? A.V.rows[v] : vm_absent_row();
        // no notFoundModelId on this path: vm_choose answers NOT_FOUND (absent, :508; owner mismatch, :530-532), HOST or OK
        const VmChoice ch = vm_choose(A.V, r, owner, olen, nullptr, 0, after);
        mmp_vstatus_row w{};
        w.cls = ch.cls;
        w.vmodel = w.model = w.target_model = -1;
        int32_t m = -1, t = -1, l0 = 0, l1 = 0, l2 = 0;  // the two requests' rows; the three lengths
        if (ch.cls == MMP_VMR_HOST)
            w.vmodel = v;
        else if (ch.cls == MMP_VMR_OK) {
            w.vmodel = v;
            w.model = vm_model_of(A.V, A.M, r, 0);
            w.target_model = vm_model_of(A.V, A.M, r, 1);
            const VmStatus vs = vm_status_of(A.V, A.M, r, w.target_model);
            w.vstatus = vs.vstatus;
            w.target_status = vs.target_status;
            w.flags = r.flags & kVmfReply;
            m = stkey_live_row(A.M, w.model);                                          // :513 getStatus(amid)
            if (vs.vstatus != MMP_VMS_DEFINED) t = stkey_live_row(A.M, w.target_model);  // :537-549, only in transition
            if (m < 0 && !after) w.cls = MMP_VMR_STRONG_READ;                          // :514-525
            l0 = r.len[0];
            l1 = r.len[1];
            l2 = r.len[2];
        }
        A.vrows[i] = w;
        A.reqs[2 * (size_t)i] = mmp_status_req{m, -1, 0u, 0u};
        A.reqs[2 * (size_t)i + 1] = mmp_status_req{t, -1, 0u, 0u};
        A.str_len[3 * (size_t)i] = l0;
        A.str_len[3 * (size_t)i + 1] = l1;
        A.str_len[3 * (size_t)i + 2] = l2;
        if (i == 0) A.str_len[3 * (size_t)A.n] = 0;
        bytes = (int64_t)l0 + l1 + l2;
    }
    const int64_t wsum = wave_sum_i64(bytes);
    if (lane_id() == 0 && wsum) atomicAdd(&A.sc->n_str_bytes, (unsigned long long)wsum);  // (an integer sum: the same in any order)
}

// pos = the exclusive scan of str_len: string j (= 3i + s) to out[pos[j], pos[j + 1]).  A string with bytes belongs to a row whose
// class is OK or STRONG_READ, so vrows[i].vmodel is a row of the table.
__global__ __launch_bounds__(256) void vstatus_strings_kernel(const mmp_vstatus_row *__restrict__ vrows, int32_t n_strings,
                                                              const int32_t *__restrict__ pos, VmTab V, char *__restrict__ out)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_strings) return;
    const int32_t o = pos[j], len = pos[j + 1] - o;
    if (len == 0) return;
    const int i = j / 3, s = j - 3 * i;
    const VmRow r = V.rows[vrows[i].vmodel];
    const int32_t src = s == 0 ? r.off[0] : s == 1 ? r.off[1] : r.off[2];  // (selects: the row stays in registers)
    for (int32_t q = 0; q < len; q++) out[o + q] = V.arena[src + q];
}

}  // namespace mmp
