// pods_retire_kernels.hpp — instance rows leave the index space (mmp_pods_retire): what the device holds by instance index — the
// registry's entry arena, the `missings` marks and the instance-id table — is rewritten on the device, beside the published state;
// the host swaps it in, together with its own compacted vectors, and commits.
//
// remap[old] = the new index of a survivor (old minus the retired indices below it), -1 for a retired instance: P0 words the host
// derives from the caller's list and uploads once.  Every kernel here is a gather through it.
//
//   pods_retire_entries_kernel  one lane per used word of the entry arena, referenced by a row or not: an entry in [0, P0) becomes
//                               remap[entry], anything else (-1, an index the table never had) is copied.  Coalesced, no divergence
//   pods_retire_count_kernel    one lane per registry row, over the entries the row REFERENCES in the OLD arena: how many name a
//                               retired instance (they become -1: unresolved), and the lowest retired instance named.  The arena's
//                               garbage is not walked, so it is neither counted nor trips MMP_PODS_RETIRE_UNREFERENCED.  A wavefront
//                               sums its lanes and adds once
//   pods_retire_marks_kernel    one lane per slot of the old `missings` map: a survivor's mark moves to its new slot
//   retire_table_kernel         (retire_kernels.hpp) the stored hashes of the survivors into the emptied next table
//   pods_retire_verify_kernel   a launch of its own, one lane per slot of the old table: tab_find of a survivor's stored hash in the
//                               next table must answer its new index; the lowest new index that does not is atomicMin'ed into a word
//
// No output position comes from an atomic: positions are remap's, the count is an integer sum and the two words are minima.  Two
// runs are byte-identical.  A word written non-atomically in one launch is read only in later launches.
#pragma once
#include "retire_kernels.hpp"

namespace mmp {

// what the count launch leaves: entries turned into -1, the lowest retired instance a record names, the lowest new index the
// verify lost (the host fills the words with 0 / INT32_MAX / INT32_MAX)
struct PodsRetireWords {
    unsigned long long n_turned;
    int32_t lowest_named, lost;
};

__global__ __launch_bounds__(kRetireBlock) void pods_retire_entries_kernel(const int32_t *__restrict__ old_pod, int32_t n_used,
                                                                           const int32_t *__restrict__ remap, int32_t P0,
                                                                           int32_t *__restrict__ new_pod)
{
    const int i = blockIdx.x * kRetireBlock + threadIdx.x;
    if (i >= n_used) return;
    const int32_t p = old_pod[i];
    new_pod[i] = (uint32_t)p < (uint32_t)P0 ? remap[p] : p;
}

__global__ __launch_bounds__(kRetireBlock) void pods_retire_count_kernel(const mmp_model_row *__restrict__ models, int32_t M,
                                                                         const int32_t *__restrict__ old_pod,
                                                                         const int32_t *__restrict__ remap, int32_t P0,
                                                                         PodsRetireWords *__restrict__ words)
{
    const int r = blockIdx.x * kRetireBlock + threadIdx.x;
    int32_t turned = 0, lowest = INT32_MAX;
    if (r < M) {
        const mmp_model_row m = models[r];
        const int32_t k = m.n_loaded + m.n_failed;
        for (int32_t e = 0; e < k; e++) {
            const int32_t p = old_pod[m.ent_off + e];
            if ((uint32_t)p < (uint32_t)P0 && remap[p] < 0) {
                turned++;
                lowest = min(lowest, p);
            }
        }
    }
    turned = wave_sum_i32(turned);
    lowest = wave_min_i32(lowest);
    if (lane_id() == 0 && turned > 0) {
        atomicAdd(&words->n_turned, (unsigned long long)turned);
        atomicMin(&words->lowest_named, lowest);
    }
}

// n_map <= P0; new_since has a slot for every survivor among the first n_map
__global__ __launch_bounds__(kRetireBlock) void pods_retire_marks_kernel(const int64_t *__restrict__ old_since, int32_t n_map,
                                                                         const int32_t *__restrict__ remap,
                                                                         int64_t *__restrict__ new_since)
{
    const int i = blockIdx.x * kRetireBlock + threadIdx.x;
    if (i >= n_map) return;
    const int32_t r = remap[i];
    if (r >= 0) new_since[r] = old_since[i];
}

__global__ __launch_bounds__(kRetireBlock) void pods_retire_verify_kernel(const uint64_t *__restrict__ old_hash,
                                                                          const int32_t *__restrict__ old_val, uint32_t old_cap,
                                                                          const int32_t *__restrict__ remap, int32_t P0, HashTab t,
                                                                          PodsRetireWords *__restrict__ words)
{
    const uint32_t s = blockIdx.x * kRetireBlock + threadIdx.x;
    if (s >= old_cap) return;
    const int32_t v = old_val[s];
    if ((uint32_t)v >= (uint32_t)P0) return;  // (an empty slot is INT32_MIN)
    const int32_t r = remap[v];
    if (r >= 0 && tab_find(t, old_hash[s], -1) != r) atomicMin(&words->lost, r);
}

}  // namespace mmp
