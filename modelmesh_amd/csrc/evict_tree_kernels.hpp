// evict_tree_kernels.hpp — eviction evaluations on long deques: prefix-weight tables and a TEAM-ary search over them.
//
// evict_batch_kernel (aux_kernels.hpp) walks a deque twice, TEAM entries a trip: right for the ~20 entries of a C3 pod, 2 x 4 096
// dependent trips on a cache of 65 536.  Nothing in an evaluation needs the walk.  On a deque in time order with weights >= 0,
//   pos        = #{ j : lu[j] <= ts }                              (LinkedDeque.insert's walk from the tail stops there)
//   n_victims  = min{ j in 1 .. E+1 : total - M(j) <= cap }        (evict() polls the head while weightedSize > capacity)
// are both the first index at which a monotone predicate turns true, where P[j] = wt[0] + .. + wt[j-1] and M is P with the new
// entry merged in at pos: M(j) = P[j] for j <= pos, P[j-1] + weight beyond.  So the context keeps, for the flat store that
// mmp_evict_batch reads (seg_off / last_used / weight of mmp_caches_load), a table EvictTables:
//   P     int64, E + 1 values per cache; cache k's start at seg_off[k] + k.  Weights reach 2^31 - 1: the sums pass 32 bits.
//   ok    one word per cache: 1 iff lu is non-decreasing along the deque and every weight is >= 0 ("searchable")
// and evict_search_kernel decides a request on a searchable cache of more than `from` entries (request weight >= 0) by two
// searches of ceil(log_{TEAM+1}) steps — 4 steps of 16 lanes for 65 536 entries — and every other request by the linear walk of
// evict_batch_kernel (evict_team_walk), inside the same launch.  Every field of mmp_evict_out is the walk's.
//
// The table is built by a segmented scan in two launches over fixed chunks of kScanChunk entries, one workgroup per chunk, a cache
// spanning as many chunks as it needs (chunk_off[k] .. chunk_off[k+1], at least one: an empty cache still owns P[0]):
//   evict_chunk_reduce_kernel   chunk -> its weight total and its "in order, no negative weight" bit.  The order compare of a
//                               chunk's first entry reads the entry before it, in the chunk to the left: it crosses the edge.
//   evict_chunk_scan_kernel     chunk -> carry = the totals of the cache's chunks to its left (<= 256 of them: one pass of the
//                               workgroup), then the exclusive scan of its own weights on top: shuffles inside a wavefront, the
//                               four wavefront totals through LDS.  The cache's last chunk also writes P[E] and the ok word.
// Carry by a second pass, not by look-back: a cache has at most 256 chunks, so the "small pass" is one strided read and one
// reduction inside the workgroup that needs it; no workgroup waits for another (nothing spins, no order of dispatch is assumed),
// P is written once, and the launch boundary is the only barrier.  Look-back would save the second read of the weights (4 of the
// 20 bytes an entry costs) and pay for it with flags polled across workgroups.
#pragma once
#include "aux_kernels.hpp"

namespace mmp {

constexpr int kScanBlock = 256;
constexpr int kScanPer = 4;                          // consecutive entries per lane
constexpr int kScanChunk = kScanBlock * kScanPer;    // 1 024 entries per workgroup
// rows_searched: a call counts in slot seq % kSearchRing of a ring and clears the slot 8 calls ahead.  A slot is kSearchWays words,
// one cache line apart, and a wavefront adds to the word of its index: 4 096 wavefronts adding to ONE word took 45 us of a 16 384-row
// call's 53 (profiles/evict_search), the atomic unit serving an address one add at a time.
constexpr int kSearchRing = 16, kSearchWays = 16, kSearchWayStride = 32;
constexpr int kSearchSlotWords = kSearchWays * kSearchWayStride;

struct EvictTables {
    int64_t *P;              // [entries + n_caches]
    int32_t *ok;             // [n_caches]
    const int32_t *chunk_off;  // [n_caches + 1]
    int64_t *chunk_total;    // [chunks]
    int32_t *chunk_ok;       // [chunks]
    uint32_t *ring;          // [kSearchRing * kSearchSlotWords]
};

// the cache of chunk q: the last k with chunk_off[k] <= q (every cache has a chunk, so there is exactly one)
__device__ __forceinline__ int scan_chunk_cache(const int32_t *__restrict__ chunk_off, int32_t n_caches, int32_t q)
{
    int lo = 0, hi = n_caches;  // chunk_off[lo] <= q < chunk_off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunk_off[mid] <= q) lo = mid; else hi = mid;
    }
    return lo;
}

// the workgroup's sum of one 64-bit value per lane, in every lane (kScanBlock lanes; `red` holds one word per wavefront)
__device__ __forceinline__ int64_t block_sum_i64(int64_t v, int64_t *red)
{
    constexpr int kWaves = kScanBlock / kWave;
    v = wave_sum_i64(v);
    __syncthreads();  // (red may still be read from the call before)
    if (lane_id() == 0) red[threadIdx.x / kWave] = v;
    __syncthreads();
    int64_t s = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) s += red[w];
    return s;
}

__global__ __launch_bounds__(kScanBlock) void evict_chunk_reduce_kernel(EvictArgs A, EvictTables T)
{
    __shared__ int64_t red[kScanBlock / kWave];
    __shared__ int32_t bad[kScanBlock / kWave];
    const int q = blockIdx.x;
    const int k = scan_chunk_cache(T.chunk_off, A.n_caches, q);
    const int s0 = A.seg_off[k], E = A.seg_off[k + 1] - s0;
    const int64_t *lu = A.last_used + s0;
    const int32_t *wt = A.weight + s0;
    const int j0 = (q - T.chunk_off[k]) * kScanChunk + (int)threadIdx.x * kScanPer;
    int64_t sum = 0;
    bool ok = true;
    int64_t prev = j0 > 0 && j0 <= E ? lu[j0 - 1] : INT64_MIN;  // (lane 0 of a later chunk: the last entry of the chunk before)
#pragma unroll
    for (int i = 0; i < kScanPer; i++) {
        const int j = j0 + i;
        if (j < E) {
            const int64_t t = lu[j];
            const int32_t w = wt[j];
            ok = ok && prev <= t && w >= 0;
            prev = t;
            sum += (int64_t)w;
        }
    }
    const int64_t total = block_sum_i64(sum, red);
    const bool wave_bad = __ballot(!ok) != 0;
    if (lane_id() == 0) bad[threadIdx.x / kWave] = wave_bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        int b = 0;
#pragma unroll
        for (int w = 0; w < kScanBlock / kWave; w++) b |= bad[w];
        T.chunk_total[q] = total;
        T.chunk_ok[q] = !b;
    }
}

__global__ __launch_bounds__(kScanBlock) void evict_chunk_scan_kernel(EvictArgs A, EvictTables T)
{
    __shared__ int64_t red[kScanBlock / kWave];
    __shared__ int64_t wtot[kScanBlock / kWave];
    const int q = blockIdx.x, lane = lane_id(), wave = threadIdx.x / kWave;
    const int k = scan_chunk_cache(T.chunk_off, A.n_caches, q);
    const int q0 = T.chunk_off[k], q1 = T.chunk_off[k + 1];
    const int s0 = A.seg_off[k], E = A.seg_off[k + 1] - s0;
    const int32_t *wt = A.weight + s0;
    int64_t *P = T.P + s0 + k;
    // the chunks to the left
    int64_t c = 0;
    for (int p = q0 + (int)threadIdx.x; p < q; p += kScanBlock) c += T.chunk_total[p];
    const int64_t carry = block_sum_i64(c, red);
    // this chunk: the lane's entries, the lanes of a wavefront by shuffles, the wavefronts through LDS
    const int j0 = (q - q0) * kScanChunk + (int)threadIdx.x * kScanPer;
    int64_t w[kScanPer], mine = 0;
#pragma unroll
    for (int i = 0; i < kScanPer; i++) {
        w[i] = j0 + i < E ? (int64_t)wt[j0 + i] : 0;
        mine += w[i];
    }
    int64_t incl = mine;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const int64_t t = (int64_t)shfl_u64((uint64_t)incl, lane >= o ? lane - o : lane);
        if (lane >= o) incl += t;
    }
    if (lane == kWave - 1) wtot[wave] = incl;
    __syncthreads();
    int64_t run = carry + incl - mine;
#pragma unroll
    for (int v = 0; v < kScanBlock / kWave; v++)
        if (v < wave) run += wtot[v];
#pragma unroll
    for (int i = 0; i < kScanPer; i++) {
        if (j0 + i < E) P[j0 + i] = run;
        run += w[i];
    }
    if (q == q1 - 1) {  // the cache's last chunk: the sum of everything, and whether every chunk was in order
        int32_t b = 0;
        for (int p = q0 + (int)threadIdx.x; p < q1; p += kScanBlock) b |= !T.chunk_ok[p];
        const int64_t any_bad = block_sum_i64((int64_t)b, red);
        if (threadIdx.x == 0) {
            int64_t tot = carry;
#pragma unroll
            for (int v = 0; v < kScanBlock / kWave; v++) tot += wtot[v];
            P[E] = tot;
            T.ok[k] = any_bad == 0;
        }
    }
}

// The first index in [lo, hi] at which `pred` is true, for the TEAM lanes of every searching team of the wavefront at once; pred is
// monotone over [lo, hi) and taken as true at hi.  A step probes TEAM indices s apart, s = n / (TEAM + 1) + 1 for a range of n: the
// first lane whose probe is true closes the range above, the lane before it opens it below, and at most s - 1 < n / (TEAM + 1) + 1
// indices are left.  The whole wavefront calls it (ballots); a team that does not search passes lo == hi.
template <int TEAM, class Pred>
__device__ __forceinline__ int team_search(int lo, int hi, int tl, int tbase, Pred pred)
{
    constexpr uint32_t kTeamMask = (1u << TEAM) - 1u;
    while (__ballot(hi > lo) != 0) {
        const int n = hi - lo, s = n / (TEAM + 1) + 1;
        const int idx = lo + (tl + 1) * s - 1;
        const bool t = hi > lo && (idx >= hi || pred(idx));
        const uint32_t tb = (uint32_t)(__ballot(t) >> tbase) & kTeamMask;
        if (hi > lo) {
            const int f = tb ? __ffs(tb) - 1 : TEAM;
            const int nlo = lo + f * s;
            if (f < TEAM) hi = min(nlo + s - 1, hi);
            lo = nlo;
        }
    }
    return lo;
}

template <int TEAM>
__global__ __launch_bounds__(kEvBlock) void evict_search_kernel(EvictArgs A, EvictTables T, int32_t from, uint32_t seq)
{
    const int lane = lane_id();
    const int team = lane / TEAM, tl = lane & (TEAM - 1), tbase = team * TEAM;
    const int i = (blockIdx.x * blockDim.x + threadIdx.x) / TEAM;
    if (blockIdx.x == 0 && threadIdx.x < kSearchWays)  // a later call's slot (see mmp_ctx::ev_ring)
        T.ring[(seq + kSearchRing / 2) % kSearchRing * kSearchSlotWords + threadIdx.x * kSearchWayStride] = 0;
    const bool in_range = i < A.n;
    mmp_evict_req r;
    r.cache = -1;
    r.weight = 0;
    r.last_used = 0;
    if (in_range) r = A.reqs[i];
    const bool valid = in_range && r.cache >= 0 && r.cache < A.n_caches;
    int s0 = 0, E = 0;
    int64_t cap = 0;
    bool srch = false;
    if (valid) {
        s0 = A.seg_off[r.cache];
        E = A.seg_off[r.cache + 1] - s0;
        cap = A.capacity[r.cache];
        srch = E > from && r.weight >= 0 && T.ok[r.cache] != 0;
    }
    const int64_t *lu = A.last_used + s0;
    const int32_t *wt = A.weight + s0;
    const int64_t ts = r.last_used == 0 ? A.now : r.last_used;
    int pos = 0, n_victims = 0;
    int64_t after = 0;
    const uint64_t searching = __ballot(srch);
    if (__ballot(in_range && !srch) != 0)  // wave-uniform.  The searching teams walk an empty deque beside the others.
        evict_team_walk<TEAM>(lu, wt, srch ? 0 : E, r.weight, ts, valid && !srch, cap, pos, n_victims, after);
    if (searching != 0) {
        const int64_t *P = T.P + s0 + (valid ? r.cache : 0);
        const int64_t w = (int64_t)r.weight;
        const int p = team_search<TEAM>(0, srch ? E : 0, tl, tbase, [&](int j) { return lu[j] > ts; });
        int64_t total = 0;
        bool over = false;
        if (srch) {
            total = P[E] + w;
            over = total > cap;
        }
        const auto M = [&](int j) { return j <= p ? P[j] : P[j - 1] + w; };  // merged prefix, j in 0 .. E+1
        // the walk's own compare, what is left against the capacity: 0 <= total - M(j) <= total on a searchable cache, where
        // "M(j) >= total - cap" wraps for a capacity below total - 2^63 and stopped at one victim where the walk polls them all
        const int v = team_search<TEAM>(over ? 1 : 0, over ? E + 1 : 0, tl, tbase, [&](int j) { return total - M(j) <= cap; });
        if (srch) {
            pos = p;
            n_victims = over ? v : 0;
            after = over ? total - M(v) : total;
        }
        const uint32_t way = (blockIdx.x * (kEvBlock / kWave) + threadIdx.x / kWave) % kSearchWays;
        if (lane == 0) atomicAdd(&T.ring[seq % kSearchRing * kSearchSlotWords + way * kSearchWayStride], (uint32_t)__popcll(searching) / TEAM);
    }
    if (in_range && tl == 0) A.outs[i] = evict_out_row(valid, lu, E, ts, pos, n_victims, after);
    announce_done(A.done);
}

}  // namespace mmp
