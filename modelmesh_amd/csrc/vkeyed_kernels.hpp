// vkeyed_kernels.hpp — the request seams by VMODEL id (mmp_place_batch_cv, mmp_route_batch_cv, mmp_miss_batch_cv): a request names a
// vmodel by KEY, and resolveVModelId (ModelMeshApi.callModel :452-476 -> VModelManager.java:569-597) runs on the device inside the
// call, in front of the unchanged decision kernels on the same stream.
//
//   vkeyed_resolve_kernel  one lane per request: (masked) FNV-1a over its vmodel key, mid_find against the vmodel-id table the call
//                          captured, the VmRow, the choice of resolveVModelId (vm_choose, vmodel_kernels.hpp: the one statement of
//                          the Java), ONE mid_find of the chosen string against the captured MODEL-id table with the hash the row
//                          stores (VmRow::hash[which]: no second hash), the bound m < n_models, the row (or -1) into the `model`
//                          field of up to two request-row arrays (KeyedPatch, keyed_kernels.hpp) and the mmp_vseam_row
//
// What the host did in two calls (mmp_vmodels_resolve under the batch lock, then a _c call on the row it answered) is one launch in
// front of the decision.  The kernel reads the vmodel rows, the string arena and the two id tables — never the registry rows: the
// target's status is the management path's (getVModelStatus is not on the request path: mmp_vmodels_status, status_keyed_kernels.hpp).  There are no owners here either:
// resolveVModelId on the request path takes none.
//
// The bytes.  On a slot the vmodel keys and the notFoundModelId spans lie in pinned host memory; a workgroup's keys are contiguous
// and so are its nf spans, so its lanes first copy both into LDS in 16-byte chunks (one coalesced pass each) and hash and compare
// from there.  The padding contract is keyed_resolve_kernel's: each region is 16-byte aligned and has kKeyedPad readable bytes
// behind its last span.  A region of a workgroup that does not fit its half of the LDS (large staged calls with long ids) is read
// where it is; which of the two happens is uniform over the workgroup, and the answers are the same.  No scratch, no atomics; two
// runs are byte-identical.
#pragma once
#include "keyed_kernels.hpp"
#include "vmodel_kernels.hpp"

namespace mmp {

constexpr int kVKeyedLdsBytes = 8192;  // a workgroup's vmodel keys, and its nf spans, staged in LDS up to this size EACH

struct VKeyedArgs {
    const char *keys;        // key i = keys[off[i] - off[0], off[i + 1] - off[0])
    const int32_t *off;      // n + 1 offsets as the caller gave them (monotone: checked on the host)
    const char *nf;          // nf i likewise; an empty span is Java null
    const int32_t *nf_off;   // n + 1 offsets (all equal when the caller gave none)
    const uint32_t *flags;   // n words: MMP_VMRQ_AFTER_STRONG
    int32_t n;
    uint64_t hmask;          // MMP_VMODEL_ID_HASH_BITS
    VmTab V;                 // the vmodel table as published when the call captured it (no vmodel call yet: all zero)
    ModelIdTab models;       // the model-id table, captured in the same hold
    int32_t n_models;        // ... and the registry's row count
    mmp_vseam_row *out;      // n rows
    KeyedPatch a, b;
};

// [lo, hi) of `src` (lo a multiple of 16) into `dst` in 16-byte chunks when it fits `cap` bytes; the caller puts the barrier
__device__ __forceinline__ bool vkeyed_stage(uint4 *dst, int cap, const char *src, int32_t lo, int32_t hi)
{
    const int32_t chunks = (hi - lo + 15) >> 4;
    if (chunks > cap / 16) return false;  // uniform over the workgroup: lo and hi are
    const uint4 *s = reinterpret_cast<const uint4 *>(src + lo);
    for (int32_t k = threadIdx.x; k < chunks; k += kIdTabBlock) dst[k] = s[k];
    return true;
}

__global__ __launch_bounds__(kIdTabBlock) void vkeyed_resolve_kernel(VKeyedArgs A)
{
    __shared__ uint4 skeys[kVKeyedLdsBytes / 16], snf[kVKeyedLdsBytes / 16];
    const int first = blockIdx.x * kIdTabBlock;
    const int last = min(first + kIdTabBlock, A.n);  // (first < n: the grid is div_up(n, kIdTabBlock))
    const int32_t o0 = A.off[0], q0 = A.nf_off[0];
    const int32_t klo = (A.off[first] - o0) & ~15, khi = A.off[last] - o0;
    const int32_t nlo = (A.nf_off[first] - q0) & ~15, nhi = A.nf_off[last] - q0;
    const bool k_lds = vkeyed_stage(skeys, kVKeyedLdsBytes, A.keys, klo, khi);
    const bool n_lds = vkeyed_stage(snf, kVKeyedLdsBytes, A.nf, nlo, nhi);
    __syncthreads();
    const int i = first + threadIdx.x;
    if (i >= A.n) return;
    const int32_t o = A.off[i] - o0, klen = A.off[i + 1] - A.off[i];
    const int32_t q = A.nf_off[i] - q0, nlen = A.nf_off[i + 1] - A.nf_off[i];
    const char *key = k_lds ? reinterpret_cast<const char *>(skeys) + (o - klo) : A.keys + o;
    const char *np = n_lds ? reinterpret_cast<const char *>(snf) + (q - nlo) : A.nf + q;
    const int32_t v = mid_find(A.V.ids, fnv1a(key, klen) & A.hmask, key, klen);
    const VmRow r = v >= 0 && v < A.V.n_rows ? A.V.rows[v] : vm_absent_row();
    const VmChoice ch = vm_choose(A.V, r, nullptr, 0, np, nlen, A.flags[i] & MMP_VMRQ_AFTER_STRONG);
    mmp_vseam_row w{};
    w.cls = ch.cls;
    w.vmodel = w.model = -1;
    if (ch.cls != MMP_VMR_NOT_FOUND) w.vmodel = v;
    if (ch.which >= 0) {  // MMP_VMR_OK
        w.which = ch.which;
        // (the row lives in registers: its string is picked by selects, not by an index the compiler would take to scratch)
        const bool target = ch.which == MMP_VMW_TARGET;
        const uint64_t h = target ? r.hash[1] : r.hash[0];
        const int32_t so = target ? r.off[1] : r.off[0], slen = target ? r.len[1] : r.len[0];
        if (r.flags & (target ? kVmfTargetNull : kVmfActiveNull))
            w.flags = MMP_VMRF_NULL_ID;
        else {
            const int32_t m = mid_find(A.models, h, A.V.arena + so, slen);
            w.model = m < A.n_models ? m : -1;
        }
    }
    A.out[i] = w;
    keyed_patch(A.a, i, w.model);  // (-1 unless the class is OK and the id is one the model-id table knows)
    keyed_patch(A.b, i, w.model);
}

}  // namespace mmp
