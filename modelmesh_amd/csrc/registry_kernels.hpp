// registry_kernels.hpp — the leader reaper's FIRST half: pruneModelRegistry (MM.java:6524-6609) with
// pruneMissingInstances (:6752-6784) and repairLastUsedTimeIfNeeded (:6837-6850), as one pass over the
// resident registry.  (The second half, triggerProactiveLoadsForInstanceSubset, is rebalance_kernels.hpp.)
//
// The Java walks the registry sequentially and keeps `missings` (instance id -> first time it was seen missing)
// across runs.  One run uses one clock value here, so the only sequential piece — missings.putIfAbsent (:6776) —
// closes: an instance first seen missing in THIS run gets since = now and nothing of it is removed; an entry is
// removed iff it is examined (:6761, :6765), its instance is missing (:6769-6770) and the instance had a mark
// BEFORE the run with now - since > gone_after (:6777).  Whether a run sees an instance missing at all is an OR
// over the examined entries, which a flag per pod collects.
//
//   prune_pods_kernel     pod-sized: one state byte per pod (present / missing / missing and due), flags cleared
//   prune_count_kernel    one lane per model: walks its entries, per-workgroup counts of (edits, removed, kept)
//   prune_scan_kernel     one workgroup: exclusive scan of the three counts, the totals
//   prune_scatter_kernel  the same walk: edits and removed lists scattered in registry / list order
//                         (count -> scan -> ballot scatter, as proactive_count_kernel / proactive_scatter_kernel)
//   prune_marks_kernel    pod-sized: new marks first, then the cleanup of :6601-6606
//   prune_build_kernel    (apply) one lane per edit: the surviving entries appended to the arena, the edited row
//                         staged for upsert_models_kernel
// The count and scatter kernels here, in janitor_kernels.hpp and in registry_ops_kernels.hpp hand prune_scan_kernel one triple
// per workgroup and take their offsets back from it by one protocol: triple_count / triple_offsets below.
#pragma once
#include "rebalance_kernels.hpp"

namespace mmp {

struct PruneScalars {  // mirrors mmp_prune_info + work counters
    int32_t n_edits, n_removed, n_repaired, n_unresolved, n_missing_pods, n_new_missing, truncated;
    int32_t n_kept;  // entries the edited models keep (what an apply appends to the arena)
};

struct PruneArgs {
    int32_t self_pod, P;
    int64_t now, gone_after, repaired_last_used;  // repaired_last_used = now - 3 * lastused_age_on_add_ms
};

constexpr uint8_t kPodPresent = 0, kPodMissing = 1, kPodDue = 2;
constexpr int kPruneBlock = kCompactBlock;
constexpr int32_t kMarksKeep = 0, kMarksAdvance = 1, kMarksIfNoEdits = 2;  // prune_marks_kernel: whether the map is written

// ---- the per-workgroup triple (edits, column 1, entries the edited records keep) ----
// A count kernel leaves block_counts[3 * b + 0..2] for its workgroup b, prune_scan_kernel turns them into exclusive offsets in place
// (and the totals), and the scatter kernel of the same grid, its lanes contributing the same three, places its output there in lane
// order.  Column 1 is what the call lists beside its edits: removed entries (the prune: a sum), candidates (the janitor: a count
// of lanes), nothing (the ops: constant 0, no LDS).  Each helper holds one __syncthreads(): the whole workgroup calls it, or none.
enum TripleCol1 { kCol1None, kCol1Count, kCol1Sum };
struct TripleOff { int32_t e, r, k; };  // the lane's exclusive offset in each column
// count side: thread 0 stores the workgroup's three totals
template <TripleCol1 C1>
__device__ __forceinline__ void triple_count(bool edit, int32_t v1, int32_t kept, int32_t *__restrict__ block_counts)
{
    constexpr int W = kCompactBlock / 64, K = C1 == kCol1None ? 1 : 2;
    __shared__ int32_t s[K + 1][W];  // per wave: edits, column 1 if there is one, kept
    const int ne = __popcll(__ballot(edit));
    const int32_t n1 = C1 == kCol1Count ? __popcll(__ballot(v1 != 0)) : C1 == kCol1Sum ? wave_sum_i32(v1) : 0, nk = wave_sum_i32(kept);
    const int w = threadIdx.x >> 6;
    if (lane_id() == 0) {
        s[0][w] = ne;
        if (C1 != kCol1None) s[1][w] = n1;
        s[K][w] = nk;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t e = 0, r = 0, k = 0;
        for (int x = 0; x < W; x++) {
            e += s[0][x];
            if (C1 != kCol1None) r += s[1][x];
            k += s[K][x];
        }
        block_counts[3 * blockIdx.x + 0] = e;
        block_counts[3 * blockIdx.x + 1] = r;
        block_counts[3 * blockIdx.x + 2] = k;
    }
}

// scatter side: the workgroup's offsets from the scan, plus the preceding waves, plus the preceding lanes
template <TripleCol1 C1>
__device__ __forceinline__ TripleOff triple_offsets(bool edit, int32_t v1, int32_t kept, const int32_t *__restrict__ block_off)
{
    constexpr int W = kCompactBlock / 64, K = C1 == kCol1None ? 1 : 2;
    __shared__ int32_t s[K + 1][W];
    const uint64_t be = __ballot(edit), b1 = C1 == kCol1Count ? __ballot(v1 != 0) : 0;
    const int32_t i1 = C1 == kCol1Sum ? wave_incl_scan_i32(v1) : 0, ik = wave_incl_scan_i32(kept);
    const int lane = lane_id(), w = threadIdx.x >> 6;
    if (lane == 63) {
        s[0][w] = __popcll(be);
        if (C1 != kCol1None) s[1][w] = C1 == kCol1Count ? __popcll(b1) : i1;
        s[K][w] = ik;
    }
    __syncthreads();
    TripleOff o{block_off[3 * blockIdx.x + 0], C1 != kCol1None ? block_off[3 * blockIdx.x + 1] : 0, block_off[3 * blockIdx.x + 2]};
    for (int x = 0; x < w; x++) {
        o.e += s[0][x];
        if (C1 != kCol1None) o.r += s[1][x];
        o.k += s[K][x];
    }
    const uint64_t below = (1ull << lane) - 1ull;
    o.e += __popcll(be & below);
    o.r += C1 == kCol1Count ? __popcll(b1 & below) : i1 - v1;
    o.k += ik - kept;
    return o;
}

// One state byte per pod slot of the instance table; `seen` is cleared for the walk.  since[] covers n_map >= P slots.
__global__ void prune_pods_kernel(const mmp_pod_row *__restrict__ pods, PruneArgs A, const int64_t *__restrict__ since,
                                  uint8_t *__restrict__ state, uint8_t *__restrict__ seen, PruneScalars *ps)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p == 0) *ps = PruneScalars{};
    if (p >= A.P) return;
    uint8_t s = kPodPresent;
    if (pods[p].flags & MMP_POD_TOMBSTONE) {  // a shutting-down row is still in instanceInfo: present
        const int64_t t = since[p];
        s = (t != 0 && jsub64(A.now, t) > A.gone_after) ? kPodDue : kPodMissing;  // :6777 (strict)
    }
    state[p] = s;
    seen[p] = 0;
}

// What one model's walk yields.
struct PruneWalk {
    int32_t rm_loaded, rm_failed, unresolved;
};

// pruneMissingInstances over instanceIds, then over loadFailedInstanceIds (:6552-6553).  EMIT: removed entries go to
// `out` (list order), bounded by `cap` (indices in the call's removed list).
template <bool EMIT>
__device__ __forceinline__ PruneWalk prune_walk(const mmp_model_row &m, const int32_t *__restrict__ ent_pod,
                                                const int64_t *__restrict__ ent_time, const PruneArgs &A,
                                                const uint8_t *__restrict__ state, uint8_t *__restrict__ seen,
                                                mmp_prune_removed *__restrict__ out, int32_t dst, int32_t cap)
{
    PruneWalk w{0, 0, 0};
    const int32_t n = m.n_loaded + m.n_failed;
    for (int32_t k = 0; k < n; k++) {
        const int64_t t = ent_time[m.ent_off + k];
        if (jsub64(A.now, t) < A.gone_after) continue;  // :6761 ignore recently loaded (strict)
        const int32_t pod = ent_pod[m.ent_off + k];
        if (pod == A.self_pod) continue;  // :6765
        if (pod < 0 || pod >= A.P) {      // an id that is not in the pod table: never pruned, never marked
            w.unresolved++;
            continue;
        }
        const uint8_t s = state[pod];
        if (s == kPodPresent) continue;  // :6769-6771
        if (!EMIT) seen[pod] = 1;        // the instance is missing (:6776; every writer stores the same byte)
        if (s != kPodDue) continue;
        const bool failed = k >= m.n_loaded;
        if (EMIT) {
            const int32_t d = dst + w.rm_loaded + w.rm_failed;
            if (d < cap) out[d] = mmp_prune_removed{pod, failed ? 1 : 0, t};
        }
        if (failed)
            w.rm_failed++;
        else
            w.rm_loaded++;
    }
    return w;
}

// pass 1: per-workgroup counts of (edits, removed entries, entries the edited models keep)
__global__ __launch_bounds__(kPruneBlock) void prune_count_kernel(const mmp_model_row *__restrict__ models, int32_t M,
                                                                  const int32_t *__restrict__ ent_pod,
                                                                  const int64_t *__restrict__ ent_time, PruneArgs A,
                                                                  const uint8_t *__restrict__ state, uint8_t *__restrict__ seen,
                                                                  int32_t *__restrict__ block_counts, PruneScalars *ps)
{
    __shared__ int32_t s_u[kPruneBlock / 64], s_p[kPruneBlock / 64];
    const int i = blockIdx.x * kPruneBlock + threadIdx.x;
    bool edit = false, repair = false;
    int32_t rm = 0, kept = 0, unres = 0;
    if (i < M) {
        const mmp_model_row m = models[i];
        const PruneWalk w = prune_walk<false>(m, ent_pod, ent_time, A, state, seen, nullptr, 0, 0);
        rm = w.rm_loaded + w.rm_failed;
        unres = w.unresolved;
        repair = m.last_used == INT64_MAX;  // :6843
        edit = rm > 0 || repair;
        if (edit) kept = m.n_loaded + m.n_failed - rm;
    }
    const int np = __popcll(__ballot(repair));
    const int32_t nu = wave_sum_i32(unres);
    const int w = threadIdx.x >> 6;
    if (lane_id() == 0) {
        s_u[w] = nu;
        s_p[w] = np;
    }
    triple_count<kCol1Sum>(edit, rm, kept, block_counts);  // (its barrier covers s_u / s_p too)
    if (threadIdx.x == 0) {
        int32_t u = 0, p = 0;
        for (int x = 0; x < kPruneBlock / 64; x++) {
            u += s_u[x];
            p += s_p[x];
        }
        if (u) atomicAdd(&ps->n_unresolved, u);
        if (p) atomicAdd(&ps->n_repaired, p);
    }
}

// exclusive scan of the nb (edits, removed, kept) triples by ONE workgroup; the totals and the truncation verdict
__global__ __launch_bounds__(256) void prune_scan_kernel(int32_t *__restrict__ counts, int32_t nb, int32_t max_edits,
                                                         int32_t max_removed, PruneScalars *ps)
{
    __shared__ int32_t carry[3], wtot[3][4];
    if (threadIdx.x < 3) carry[threadIdx.x] = 0;
    __syncthreads();
    for (int base = 0; base < nb; base += 256) {
        const int i = base + threadIdx.x;
        int32_t v[3], incl[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            v[c] = i < nb ? counts[3 * i + c] : 0;
            incl[c] = wave_incl_scan_i32(v[c]);
            if (lane_id() == 63) wtot[c][threadIdx.x >> 6] = incl[c];
        }
        __syncthreads();
        int32_t before[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            before[c] = carry[c];
            for (int w = 0; w < (int)(threadIdx.x >> 6); w++) before[c] += wtot[c][w];
            if (i < nb) counts[3 * i + c] = before[c] + incl[c] - v[c];
        }
        __syncthreads();
        if (threadIdx.x == 255) {
#pragma unroll
            for (int c = 0; c < 3; c++) carry[c] = before[c] + incl[c];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        ps->n_edits = carry[0];
        ps->n_removed = carry[1];
        ps->n_kept = carry[2];
        ps->truncated = (carry[0] > max_edits || carry[1] > max_removed) ? 1 : 0;
    }
}

// pass 2: edits in registry order, their removed entries in list order; keep_off[e] = where edit e's surviving
// entries start among the kept ones.  Writes are bounded by the caller's capacities (a truncated prefix).
__global__ __launch_bounds__(kPruneBlock) void prune_scatter_kernel(const mmp_model_row *__restrict__ models, int32_t M,
                                                                    const int32_t *__restrict__ ent_pod,
                                                                    const int64_t *__restrict__ ent_time, PruneArgs A,
                                                                    const uint8_t *__restrict__ state,
                                                                    const int32_t *__restrict__ block_off, const PruneScalars *ps,
                                                                    mmp_prune_edit *__restrict__ edits, int32_t max_edits,
                                                                    mmp_prune_removed *__restrict__ removed, int32_t max_removed,
                                                                    int32_t *__restrict__ keep_off)
{
    if (ps->n_edits == 0) return;  // (uniform: the whole grid leaves)
    const int i = blockIdx.x * kPruneBlock + threadIdx.x;
    mmp_model_row m{};
    bool edit = false, repair = false;
    int32_t rm = 0, rm_l = 0, rm_f = 0, kept = 0;
    if (i < M) {
        m = models[i];
        // the count pass, without output: the offsets have to be known before the entries can be placed
        const PruneWalk w = prune_walk<true>(m, ent_pod, ent_time, A, state, nullptr, nullptr, 0, 0);
        rm_l = w.rm_loaded;
        rm_f = w.rm_failed;
        rm = rm_l + rm_f;
        repair = m.last_used == INT64_MAX;
        edit = rm > 0 || repair;
        if (edit) kept = m.n_loaded + m.n_failed - rm;
    }
    const TripleOff o = triple_offsets<kCol1Sum>(edit, rm, kept, block_off);
    if (!edit) return;
    const int32_t e = o.e, roff = o.r;
    if (e < max_edits) {
        mmp_prune_edit ed;
        ed.model = i;
        ed.n_loaded_after = m.n_loaded - rm_l;
        ed.n_failed_after = m.n_failed - rm_f;
        ed.flags = repair ? 1u : 0u;
        ed.removed_off = roff;
        ed.n_removed = rm;
        ed.last_used_after = repair ? A.repaired_last_used : m.last_used;  // :6844
        edits[e] = ed;
        keep_off[e] = o.k;
    }
    if (rm > 0) (void)prune_walk<true>(m, ent_pod, ent_time, A, state, nullptr, removed, roff, max_removed);
}

// missings after the run: putIfAbsent(pod, now) for the pods seen missing (:6776), then the cleanup of :6601-6606 — a mark
// older than gone_after or whose instance is present again is dropped.  Slots >= P belong to no row of the table: absent.
// Stores happen only when `advance` says so (kMarksIfNoEdits: a run that found no edit) and the outputs were not truncated; the
// counts are always what the run would leave.
__global__ void prune_marks_kernel(PruneArgs A, int32_t n_map, const uint8_t *__restrict__ state, const uint8_t *__restrict__ seen,
                                   int64_t *__restrict__ since, int32_t advance, PruneScalars *ps)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    bool held = false, fresh = false;
    if (p < n_map) {
        const int64_t old = since[p];
        int64_t s = old;
        if (p < A.P && s == 0 && seen[p]) {
            s = A.now;
            fresh = true;
        }
        if (s != 0) {
            const bool present = p < A.P && state[p] == kPodPresent;
            if (jsub64(A.now, s) > A.gone_after || present) s = 0;
        }
        held = s != 0;
        const bool store = advance == kMarksAdvance || (advance == kMarksIfNoEdits && ps->n_edits == 0);
        if (store && !ps->truncated && s != old) since[p] = s;
    }
    const int nh = __popcll(__ballot(held)), nf = __popcll(__ballot(fresh));
    if (lane_id() == 0) {
        if (nh) atomicAdd(&ps->n_missing_pods, nh);
        if (nf) atomicAdd(&ps->n_new_missing, nf);
    }
}

// apply: edit e's surviving entries, in their order, to arena[base + keep_off[e] ...); its row for upsert_models_kernel.
// `base + n_kept` lies inside the arena (the host grew it), and nothing refers to that part yet.
__global__ void prune_build_kernel(const mmp_prune_edit *__restrict__ edits, const int32_t *__restrict__ keep_off, int32_t n_edits,
                                   const mmp_model_row *__restrict__ models, int32_t *__restrict__ ent_pod,
                                   int64_t *__restrict__ ent_time, int32_t base, int32_t arena_end, PruneArgs A,
                                   const uint8_t *__restrict__ state, int32_t *__restrict__ u_idx, mmp_model_row *__restrict__ u_rows)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_edits) return;
    const mmp_prune_edit ed = edits[e];
    const mmp_model_row m = models[ed.model];
    int32_t dst = base + keep_off[e];
    const int32_t n = m.n_loaded + m.n_failed;
    for (int32_t k = 0; k < n; k++) {
        const int64_t t = ent_time[m.ent_off + k];
        const int32_t pod = ent_pod[m.ent_off + k];
        const bool gone = !(jsub64(A.now, t) < A.gone_after) && pod != A.self_pod && pod >= 0 && pod < A.P && state[pod] == kPodDue;
        if (gone) continue;
        if (dst < arena_end) {
            ent_pod[dst] = pod;
            ent_time[dst] = t;
        }
        dst++;
    }
    u_idx[e] = ed.model;
    u_rows[e] = mmp_model_row{m.type, base + keep_off[e], ed.n_loaded_after, ed.n_failed_after, ed.last_used_after};
}

}  // namespace mmp
