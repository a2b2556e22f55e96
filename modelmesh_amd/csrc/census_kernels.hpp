// census_kernels.hpp — the model-count side of the registry listener (MM.java:2807-2854) and of logModelCountMetrics
// (:6852-6863) as one read-only pass over the resident registry: loadedModelIds.size(), failedModelIds.size(),
// registry.getCount(), and hasRegistration (:2856-2858) summed per instance and per list.
//
// The Java keeps two sets up to date event by event; a record is in loadedModelIds iff !instanceIds.isEmpty() (:2828) and in
// failedModelIds iff hasLoadFailure() (:2829).  Both are properties of the record alone, so the sizes of the sets are counts
// over the registry as it stands, whatever events led there.
//
//   census_walk_kernel   one lane per model row (grid-stride over tiles of kCensusBlock rows): the scalars and the copies
//                        histogram by ballot / lane reduction -> LDS -> one global atomic per workgroup and counter; the per-type
//                        rows through an LDS table (one atomic per non-zero slot) or global atomics; the per-pod counts through
//                        a private LDS table (POD_LDS) or global atomics.
//
// The caller zeroes the outputs (one fill) before the launch.  Every sum is an integer sum: the result does not depend on the
// order of the atomics.
#pragma once
#include "registry_kernels.hpp"

namespace mmp {

constexpr int kCensusBlock = kPruneBlock;
constexpr size_t kLdsPerCU = 160 * 1024;  // gfx950
// The two pod-sized count arrays are kept private to a workgroup when they take no more than half of a compute unit's LDS
// (a 10k-instance table: 2 x 40 KB); beyond that (50k instances: 2 x 200 KB) the lanes add to the global arrays directly.
constexpr size_t kCensusPodLdsBytes = kLdsPerCU / 2;
constexpr int kCensusTypeSlots = 512;  // type tables up to this many rows are counted in LDS (20 bytes a row)
constexpr size_t kCensusStaticLds = 12 * 1024;  // (an upper bound of the kernel's static LDS: the type table and the counters)
constexpr int kCensusGridMax = 2048;   // workgroups of the walk when nothing but registers and the small tables limit them

// per-workgroup counters: the predicates of mmp_registry_stats in its field order, then the three entry sums
enum { kCnModels, kCnLoaded, kCnFailed, kCnBoth, kCnUnloadedUsed, kCnLuMax, kCnHist0, kCnPreds = kCnHist0 + 5 };
static_assert(offsetof(mmp_registry_stats, n_last_used_max) == 4 * kCnLuMax && offsetof(mmp_registry_stats, n_entries_loaded) == 24 &&
                  offsetof(mmp_registry_stats, n_entries_unresolved) == 40 && offsetof(mmp_registry_stats, copies_hist) == 48 &&
                  sizeof(mmp_registry_stats) == 72 && sizeof(mmp_registry_type_stats) == 24,
              "census_walk_kernel flushes its counters by field position");

__device__ __forceinline__ int32_t wave_max_i32(int32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int32_t t = __shfl_xor(v, o, 64);
        v = t > v ? t : v;
    }
    return v;
}

// pod_counts = pod_loaded[P] | pod_failed[P].  POD_LDS: launched with 2 * P * 4 bytes of dynamic LDS.
template <bool POD_LDS>
__global__ __launch_bounds__(kCensusBlock) void census_walk_kernel(const mmp_model_row *__restrict__ models, int32_t M,
                                                                   const int32_t *__restrict__ ent_pod, int32_t P, int32_t T,
                                                                   mmp_registry_stats *__restrict__ stats,
                                                                   mmp_registry_type_stats *__restrict__ types,
                                                                   int32_t *__restrict__ pod_counts)
{
    extern __shared__ int32_t s_pod[];
    __shared__ int32_t s_type[kCensusTypeSlots * 3];  // n_models, n_loaded, n_failed
    __shared__ unsigned long long s_tent[kCensusTypeSlots];  // entries loaded
    __shared__ int32_t s_pred[kCnPreds], s_max;
    __shared__ unsigned long long s_sum[3];
    const bool type_lds = T <= kCensusTypeSlots;
    if (POD_LDS)
        for (int s = threadIdx.x; s < 2 * P; s += kCensusBlock) s_pod[s] = 0;
    if (type_lds)
        for (int s = threadIdx.x; s < 3 * T; s += kCensusBlock) {
            s_type[s] = 0;
            if (s < T) s_tent[s] = 0;
        }
    if (threadIdx.x < kCnPreds) s_pred[threadIdx.x] = 0;
    if (threadIdx.x < 3) s_sum[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_max = 0;
    __syncthreads();

    int32_t *const pod_tbl = POD_LDS ? s_pod : pod_counts;
    int32_t pred[kCnPreds] = {};  // wave-uniform: popcounts of ballots
    int64_t e_loaded = 0, e_failed = 0, e_unres = 0;
    int32_t mx = 0;
    // every wave runs the same number of rounds (the ballots need whole waves); a lane beyond M sits a round out
    for (int64_t base = (int64_t)blockIdx.x * kCensusBlock; base < M; base += (int64_t)gridDim.x * kCensusBlock) {
        const int64_t i = base + threadIdx.x;
        const bool live = i < M;
        mmp_model_row m{};
        if (live) m = models[i];
        const bool loaded = live && m.n_loaded > 0;  // :2828
        const bool failed = live && m.n_failed > 0;  // :2829, ModelRecord.java:181-183
        pred[kCnModels] += __popcll(__ballot(live));
        pred[kCnLoaded] += __popcll(__ballot(loaded));
        pred[kCnFailed] += __popcll(__ballot(failed));
        pred[kCnBoth] += __popcll(__ballot(loaded && failed));
        pred[kCnUnloadedUsed] += __popcll(__ballot(live && !loaded && m.last_used > 0 && m.last_used < INT64_MAX));
        pred[kCnLuMax] += __popcll(__ballot(live && m.last_used == INT64_MAX));  // :6843
        const int bin = m.n_loaded < 4 ? m.n_loaded : 4;
#pragma unroll
        for (int b = 0; b < 5; b++) pred[kCnHist0 + b] += __popcll(__ballot(live && bin == b));
        if (live) {
            e_loaded += m.n_loaded;
            e_failed += m.n_failed;
            mx = m.n_loaded > mx ? m.n_loaded : mx;
            if (m.type >= 0 && m.type < T) {
                if (type_lds) {
                    atomicAdd(&s_type[3 * m.type + 0], 1);
                    if (loaded) atomicAdd(&s_type[3 * m.type + 1], 1);
                    if (failed) atomicAdd(&s_type[3 * m.type + 2], 1);
                    if (loaded) atomicAdd(&s_tent[m.type], (unsigned long long)m.n_loaded);
                } else {
                    mmp_registry_type_stats *t = types + m.type;
                    atomicAdd(&t->n_models, 1);
                    if (loaded) atomicAdd(&t->n_loaded, 1);
                    if (failed) atomicAdd(&t->n_failed, 1);
                    if (loaded) atomicAdd((unsigned long long *)&t->n_entries_loaded, (unsigned long long)m.n_loaded);
                }
            }
            // hasRegistration (:2856-2858) per instance: instanceIds first, then loadFailedInstanceIds
            const int32_t n = m.n_loaded + m.n_failed;
            for (int32_t k = 0; k < n; k++) {
                const int32_t pod = ent_pod[m.ent_off + k];
                if (pod < 0 || pod >= P)  // an id the instance table does not know
                    e_unres++;
                else
                    atomicAdd(&pod_tbl[(k < m.n_loaded ? 0 : P) + pod], 1);
            }
        }
    }
    const unsigned long long wl = wave_sum_u64((uint64_t)e_loaded), wf = wave_sum_u64((uint64_t)e_failed),
                             wu = wave_sum_u64((uint64_t)e_unres);
    const int32_t wm = wave_max_i32(mx);
    if (lane_id() == 0) {
#pragma unroll
        for (int q = 0; q < kCnPreds; q++)
            if (pred[q]) atomicAdd(&s_pred[q], pred[q]);
        if (wl) atomicAdd(&s_sum[0], wl);
        if (wf) atomicAdd(&s_sum[1], wf);
        if (wu) atomicAdd(&s_sum[2], wu);
        if (wm) atomicMax(&s_max, wm);
    }
    __syncthreads();
    // one global atomic per workgroup and counter (mmp_registry_stats: six int32, three int64, five bins, the maximum)
    if (threadIdx.x < kCnHist0) {
        const int32_t v = s_pred[threadIdx.x];
        if (v) atomicAdd(&stats->n_models + threadIdx.x, v);
    } else if (threadIdx.x < kCnPreds) {
        const int32_t v = s_pred[threadIdx.x];
        if (v) atomicAdd(&stats->copies_hist[threadIdx.x - kCnHist0], v);
    } else if (threadIdx.x < kCnPreds + 3) {
        const unsigned long long v = s_sum[threadIdx.x - kCnPreds];
        if (v) atomicAdd((unsigned long long *)&stats->n_entries_loaded + (threadIdx.x - kCnPreds), v);
    } else if (threadIdx.x == kCnPreds + 3) {
        if (s_max) atomicMax(&stats->max_copies, s_max);
    }
    if (type_lds)
        for (int t = threadIdx.x; t < T; t += kCensusBlock) {
            const int32_t nm = s_type[3 * t + 0];
            if (nm == 0) continue;  // (no record of the type: the other three are zero too)
            atomicAdd(&types[t].n_models, nm);
            if (s_type[3 * t + 1]) atomicAdd(&types[t].n_loaded, s_type[3 * t + 1]);
            if (s_type[3 * t + 2]) atomicAdd(&types[t].n_failed, s_type[3 * t + 2]);
            if (s_tent[t]) atomicAdd((unsigned long long *)&types[t].n_entries_loaded, s_tent[t]);
        }
    if (POD_LDS)
        for (int s = threadIdx.x; s < 2 * P; s += kCensusBlock) {
            const int32_t v = s_pod[s];
            if (v) atomicAdd(&pod_counts[s], v);
        }
}

}  // namespace mmp
