// keyed_kernels.hpp — the request seams by model id (mmp_place_batch_ck, mmp_route_batch_ck, mmp_miss_batch_ck): a request names its
// model by KEY, and the key is resolved on the device inside the call, in front of the unchanged decision kernels on the same stream.
//
//   keyed_resolve_kernel   one lane per request: (masked) FNV-1a over its key, mid_find against the id table the call captured, the
//                          row (or -1) into model_idx[i] and into the `model` field of up to two request-row arrays
//
// What mmp_model_ids_resolve does in two launches with a hash array between them is one launch here: nothing else reads the hashes.
// The row arrays are the call's own copies — its region of a latency slot, or the scratch a large call is staged through — never the
// caller's memory: a patch is given by base pointer, row stride and field offset, so one kernel serves full rows and compact rows,
// gate + place, gate + serve, or place alone.
//
// The keys.  On a slot the key bytes lie in pinned host memory, which a lane would read over the bus one byte at a time (the hash,
// then the comparison against the arena): a workgroup's keys are contiguous, so its lanes first copy them into LDS in 16-byte
// chunks (one coalesced pass), and hash and compare from there.  `keys` is 16-byte aligned and has 16 readable bytes behind the
// last key (the host side's contract: the slot regions and the staged copy are laid out so), which is what lets the copy run in
// whole chunks.  A workgroup whose keys do not fit the 16 KB (large staged calls with long ids) reads them where they are, byte by
// byte, from device memory.  No scratch, no atomics; two runs are byte-identical.
#pragma once
#include "model_ids_kernels.hpp"

namespace mmp {

constexpr int kKeyedLdsBytes = 16384;  // a workgroup's keys staged in LDS up to this size (the slot layouts' key region)
constexpr int kKeyedPad = 16;          // readable bytes behind the last key

// the `model` field of row i is *(int32_t *)(base + i * stride + field); base == nullptr: no such array
struct KeyedPatch {
    char *base;
    int32_t stride, field;
};

struct KeyedArgs {
    const char *keys;    // key i = keys[off[i] - off[0], off[i + 1] - off[0])
    const int32_t *off;  // n + 1 offsets as the caller gave them (monotone: checked on the host)
    int32_t n;
    uint64_t hmask;      // MMP_MODEL_ID_HASH_BITS
    ModelIdTab tab;      // the table as published when the call captured it
    int32_t *model_idx;  // n words
    KeyedPatch a, b;
};

__device__ __forceinline__ void keyed_patch(const KeyedPatch &p, int i, int32_t row)
{
    if (p.base) *reinterpret_cast<int32_t *>(p.base + (size_t)i * (size_t)p.stride + p.field) = row;
}

__global__ __launch_bounds__(kIdTabBlock) void keyed_resolve_kernel(KeyedArgs A)
{
    __shared__ uint4 staged[kKeyedLdsBytes / 16];
    const int first = blockIdx.x * kIdTabBlock;
    const int last = min(first + kIdTabBlock, A.n);  // (first < n: the grid is div_up(n, kIdTabBlock))
    const int32_t o0 = A.off[0];
    const int32_t lo = (A.off[first] - o0) & ~15, hi = A.off[last] - o0;
    const int32_t chunks = (hi - lo + 15) >> 4;
    const bool in_lds = chunks <= kKeyedLdsBytes / 16;  // uniform over the workgroup
    if (in_lds) {
        const uint4 *src = reinterpret_cast<const uint4 *>(A.keys + lo);
        for (int32_t k = threadIdx.x; k < chunks; k += kIdTabBlock) staged[k] = src[k];
        __syncthreads();
    }
    const int i = first + threadIdx.x;
    if (i >= A.n) return;
    const int32_t o = A.off[i] - o0, len = A.off[i + 1] - A.off[i];
    const char *key = in_lds ? reinterpret_cast<const char *>(staged) + (o - lo) : A.keys + o;
    const int32_t row = mid_find(A.tab, fnv1a(key, len) & A.hmask, key, len);
    A.model_idx[i] = row;
    keyed_patch(A.a, i, row);
    keyed_patch(A.b, i, row);
}

}  // namespace mmp
