// evict_resident_kernels.hpp — eviction evaluations on the RESIDENT caches by model id (mmp_evict_batch_k): what a
// mmp_cache_replay_k of one MMP_COP_PUT_IF_ABSENT or MMP_COP_UBM_INSERT_NEW_ENTRY would answer on the store of
// mmp_caches_load_keyed_k / mmp_cache_replay_k as it stands, nothing applied.
//
// The store is CacheStore (cache_kernels.hpp): regions [off[c], off[c+1]) of which the first n[c] slots are live, with
// weighted_size / capacity / oldest / ubm beside it.  Per cache of more than `from` live entries that a batch names, the context
// keeps three tables (ResDesc), built lazily behind a change of the store and never for a short cache:
//   P     int64, n[c] + 1 values: P[j] = wt[0] + .. + wt[j-1] over the LIVE entries
//   ok    one word: 1 iff lastUsed is non-decreasing along the deque and no weight is negative ("searchable")
//   tab   open addressing, key -> deque position: cells {key, position} of 64 bits, a power of two of at least twice the entries,
//         home cell wide_hash(key) & mask, linear probing, empty = all ones.  Nothing is ever deleted from a table (a change of the
//         store drops it whole), so a key sits in front of the first empty cell of its run.
// Two launches over chunks of kScanChunk entries, as evict_tree_kernels.hpp builds its tables — siblings of its two kernels, which
// read seg_off differences where this store has n[c] and know no keys:
//   resident_chunk_reduce_kernel   chunk -> weight total and order/sign bit
//   resident_chunk_scan_kernel     chunk -> carry by a second pass over the chunk totals, the exclusive scan on top, and every
//                                  entry's key into the index by atomicCAS on the first empty cell of its run.  No workgroup waits
//                                  for another: a lost CAS moves on to the next cell.
//
// evict_resident_kernel: a team of 16 lanes per row, four rows a wavefront, behind ckey_ops_kernel (the id resolution of the keyed
// replay, with the identity as its permutation).  Three steps:
//   1. presence, and on a managed cache the pinned entry: one index probe each on a cache with tables — 16 cells a team, 64 cells a
//      wavefront load — or the team's scan of the key column on a short one (dq_find's loop)
//   2. the insert position: team_search on lu[j] > ts on a searchable cache, the walk from the tail's rule (the last lu[j] <= ts)
//      by one pass otherwise
//   3. the victim count v: the first j >= 1 at which what is left after j victims fits the capacity,
//        left(j) = total - M(j)                                          unmanaged
//        left(j) = total - M(j) + bw(j) - bw(0),  bw(j) = clamp(t + M(j), reserved, min(cap, INT_MAX))   managed
//      M the prefix weights with the new entry merged in at the insert position, t = totalUnloadingWeight (less the new entry's
//      weight for insertNewEntry, which takes it off first, :134, and leaves it off), total = weightedSize + weight (+ bw(0) - the
//      pinned entry's weight, where insertNewEntry's first adjustment moved it).
//
// WHY THE SEARCH APPLIES TO A MANAGED CACHE.  The replay evicts a run, hands each victim to entryRemoved, which grows the pinned
// entry to clamp(totalUnloadingWeight), which may evict again, depth first.  Every victim is processed before the operation ends,
// all victims are the head run of the merged deque, and with weights >= 0 the buffer only grows on the way; so the final count is
// the least j whose FINAL state fits: at every j' < j the loop went on under a buffer no heavier than bw(j'), hence left(j') > cap.
// And left does not increase: left(j+1) - left(j) = -m_j + bw(j+1) - bw(j) with m_j >= 0 the weight of merged entry j, and
// x -> clamp(x, lo, hi) is non-decreasing with slope at most one, so bw(j+1) - bw(j) <= m_j.  The first j with left(j) <= cap is
// therefore the first index at which a monotone predicate turns true, which team_search finds.  The argument needs t + M(j) not to
// wrap an int: a row where t + P[n] + weight leaves the int range is walked.  The order the listener sees the victims in (the
// reversed pending runs) is the one thing that depends on the recursion, and it is not reported.
//
// Rows the search does not take — a short cache, a cache out of time order or with a negative weight, a negative request weight, a
// managed sum that would wrap — are WALKED in the same launch: step 2 by one pass over the stamps, step 3 from the head, 16 merged
// entries a trip with both sums in registers, O(victims).  The walk evaluates the same left(j) (|weight| for the size, as makeDead
// subtracts it, the signed weight for the manager's sum).  The pinned entry is never a victim: the count stops in front of it.
#pragma once
#include "cache_keyed_kernels.hpp"
#include "cache_wide_kernels.hpp"
#include "evict_tree_kernels.hpp"

namespace mmp {

constexpr unsigned long long kResCellEmpty = ~0ull;

struct ResDesc {  // per cache of the store; P == nullptr: no tables (a short cache, or one no batch has named since the change)
    int64_t *P;
    unsigned long long *tab;
    uint32_t mask;
    int32_t pad;
};

struct ResBuildArgs {
    CacheStore S;
    const ResDesc *desc;        // [n_caches]
    int32_t *ok;                // [n_caches]
    const int32_t *bcache;      // [nb] the caches this build covers
    const int32_t *bchunk_off;  // [nb + 1] their chunks (at least one each: an empty cache still owns P[0])
    int32_t nb;
    int64_t *chunk_total;       // [chunks]
    int32_t *chunk_ok;          // [chunks]
};

__global__ __launch_bounds__(kScanBlock) void resident_chunk_reduce_kernel(ResBuildArgs A)
{
    __shared__ int64_t red[kScanBlock / kWave];
    __shared__ int32_t bad[kScanBlock / kWave];
    const int q = blockIdx.x;
    const int b = scan_chunk_cache(A.bchunk_off, A.nb, q);
    const int c = A.bcache[b];
    const int s0 = A.S.off[c], E = A.S.n[c];
    const int64_t *lu = A.S.lu + s0;
    const int32_t *wt = A.S.wt + s0;
    const int j0 = (q - A.bchunk_off[b]) * kScanChunk + (int)threadIdx.x * kScanPer;
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
        int any = 0;
#pragma unroll
        for (int w = 0; w < kScanBlock / kWave; w++) any |= bad[w];
        A.chunk_total[q] = total;
        A.chunk_ok[q] = !any;
    }
}

__global__ __launch_bounds__(kScanBlock) void resident_chunk_scan_kernel(ResBuildArgs A)
{
    __shared__ int64_t red[kScanBlock / kWave];
    __shared__ int64_t wtot[kScanBlock / kWave];
    const int q = blockIdx.x, lane = lane_id(), wave = threadIdx.x / kWave;
    const int b = scan_chunk_cache(A.bchunk_off, A.nb, q);
    const int c = A.bcache[b];
    const int q0 = A.bchunk_off[b], q1 = A.bchunk_off[b + 1];
    const int s0 = A.S.off[c], E = A.S.n[c];
    const int32_t *wt = A.S.wt + s0;
    const int32_t *key = A.S.key + s0;
    const ResDesc d = A.desc[c];
    // the chunks to the left
    int64_t cs = 0;
    for (int p = q0 + (int)threadIdx.x; p < q; p += kScanBlock) cs += A.chunk_total[p];
    const int64_t carry = block_sum_i64(cs, red);
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
        const int j = j0 + i;
        if (j < E) {
            d.P[j] = run;
            // the key into the first empty cell of its run (the table has at least E empty cells: the loop ends)
            const unsigned long long cell = (unsigned long long)(uint32_t)key[j] | ((unsigned long long)(uint32_t)j << 32);
            uint32_t at = wide_hash(key[j]) & d.mask;
            for (uint32_t t = 0; t <= d.mask; t++, at = (at + 1) & d.mask)
                if (atomicCAS(&d.tab[at], kResCellEmpty, cell) == kResCellEmpty) break;
        }
        run += w[i];
    }
    if (q == q1 - 1) {  // the cache's last chunk: the sum of everything, and whether every chunk was in order
        int32_t bd = 0;
        for (int p = q0 + (int)threadIdx.x; p < q1; p += kScanBlock) bd |= !A.chunk_ok[p];
        const int64_t any_bad = block_sum_i64((int64_t)bd, red);
        if (threadIdx.x == 0) {
            int64_t tot = carry;
#pragma unroll
            for (int v = 0; v < kScanBlock / kWave; v++) tot += wtot[v];
            d.P[E] = tot;
            A.ok[c] = any_bad == 0;
        }
    }
}

struct ResidentArgs {
    CacheStore S;
    const int64_t *capacity, *weighted_size, *oldest;  // [n_caches]
    const mmp_ubm_state *ubm;
    const ResDesc *desc;
    const int32_t *ok;
    const mmp_cache_op *ops;  // caller order, `key` (and `op` under an unknown id) as ckey_ops_kernel left them
    const int32_t *status;    // MMP_CKEY_* by row
    mmp_evict_k_out *outs;
    int32_t n, n_caches, from;
    int64_t now;
};

// The deque position of key k by the index, -1 if absent, for every probing team of the wavefront at once (`active`: this team
// probes).  A step reads TEAM consecutive cells of the run; a hit ends it, so does an empty cell.
template <int TEAM>
__device__ __forceinline__ int res_probe(const unsigned long long *tab, uint32_t mask, int32_t k, bool active, int tl, int tbase)
{
    constexpr uint32_t kTeamMask = (1u << TEAM) - 1u;
    const uint32_t h = wide_hash(k);
    int found = -1;
    bool done = !active;
    for (uint32_t p = 0; __ballot(!done) != 0; p += TEAM) {
        const unsigned long long cell = done ? kResCellEmpty : tab[(h + p + (uint32_t)tl) & mask];
        const bool hit = !done && cell != kResCellEmpty && (int32_t)(uint32_t)cell == k;
        const uint32_t hb = (uint32_t)(__ballot(hit) >> tbase) & kTeamMask;
        const uint32_t eb = (uint32_t)(__ballot(!done && cell == kResCellEmpty) >> tbase) & kTeamMask;
        const int l = hb ? __ffs(hb) - 1 : 0;
        const int at = __shfl((int)(cell >> 32), tbase + l, 64);
        if (!done) {
            if (hb) found = at;
            if (hb || eb || p + TEAM > mask) done = true;
        }
    }
    return found;
}

__device__ __forceinline__ int32_t res_clamp(int64_t sum, int32_t reserved, int64_t cap)
{
    const int32_t t = (int32_t)(uint32_t)(uint64_t)sum;  // totalUnloadingWeight is an int
    if (t <= reserved) return reserved;
    const int32_t c32 = cap > INT32_MAX ? INT32_MAX : (int32_t)cap;
    return c32 < t ? c32 : t;
}

template <int TEAM>
__global__ __launch_bounds__(kEvBlock) void evict_resident_kernel(ResidentArgs A)
{
    constexpr uint32_t kTeamMask = (1u << TEAM) - 1u;
    const int lane = lane_id();
    const int team = lane / TEAM, tl = lane & (TEAM - 1), tbase = team * TEAM;
    const int i = (blockIdx.x * blockDim.x + threadIdx.x) / TEAM;
    const bool in_range = i < A.n;
    mmp_cache_op o;
    o.cache = -1; o.op = 0; o.key = 0; o.arg = 0; o.time = 0; o.flag = 0; o.reserved = 0;
    int32_t st = MMP_CKEY_LIVE;
    if (in_range) {
        o = A.ops[i];
        st = A.status[i];
    }
    const bool cache_ok = in_range && o.cache >= 0 && o.cache < A.n_caches;
    const bool known = cache_ok && st != MMP_CKEY_UNKNOWN;
    int s0 = 0, E = 0;
    int64_t cap = 0, ws = 0, old_field = -1;
    mmp_ubm_state u;
    u.reserved = -1; u.total_unloading = 0; u.total_occupancy = 0; u.cache_deficit = 0; u.pad = 0;
    ResDesc d;
    d.P = nullptr; d.tab = nullptr; d.mask = 0; d.pad = 0;
    bool ordered = false;
    if (cache_ok) {
        s0 = A.S.off[o.cache];
        E = A.S.n[o.cache];
        cap = A.capacity[o.cache];
        ws = A.weighted_size[o.cache];
        old_field = A.oldest[o.cache];
        u = A.ubm[o.cache];
        if (E > A.from) {
            d = A.desc[o.cache];
            ordered = d.P != nullptr && A.ok[o.cache] != 0;
        }
    }
    const int64_t *lu = A.S.lu + s0;
    const int32_t *wt = A.S.wt + s0;
    const int32_t *key = A.S.key + s0;
    const bool tabled = d.P != nullptr;
    const bool managed = u.reserved >= 0;
    int emax = tabled ? 0 : E;  // the teams of a wavefront loop together; a team with tables scans nothing
#pragma unroll
    for (int s = 32; s >= TEAM; s >>= 1) {
        const int t = __shfl_xor(emax, s, 64);
        emax = t > emax ? t : emax;
    }

    // 1. where the key is, and where the pinned entry is
    int at = -1, ub = -1;
    if (__ballot(tabled) != 0) {
        at = res_probe<TEAM>(d.tab, d.mask, o.key, tabled && known, tl, tbase);
        if (__ballot(tabled && managed) != 0) ub = res_probe<TEAM>(d.tab, d.mask, MMP_UNLOADBUF_KEY_C, tabled && managed, tl, tbase);
    }
    for (int base = 0; base < emax; base += TEAM) {
        const int j = base + tl;
        const int32_t k = !tabled && j < E ? key[j] : MMP_CACHE_KEY_UNKNOWN;
        const uint32_t kb = (uint32_t)(__ballot(known && !tabled && j < E && k == o.key) >> tbase) & kTeamMask;
        const uint32_t pb = (uint32_t)(__ballot(managed && !tabled && j < E && k == MMP_UNLOADBUF_KEY_C) >> tbase) & kTeamMask;
        if (kb && at < 0) at = base + __ffs(kb) - 1;
        if (pb && ub < 0) ub = base + __ffs(pb) - 1;
    }
    const bool present = known && at >= 0, absent = known && at < 0;
    const bool mg = managed && ub >= 0;
    const int32_t bw0 = mg ? wt[ub] : 0;

    // 2. the position.  An absent key: where LinkedDeque.insert links the new node.  A present one: whether the touched node
    // would still have a node at or below its stamp (reposition then cannot make it the head).
    int64_t ts = o.time == 0 ? A.now : o.time;  // Node ctor / touch, clhm :1357-1360
    if (present) {
        const int64_t was = lu[at];
        ts = o.time == 0 ? A.now : (was > o.time ? was : o.time);
    }
    int pos = team_search<TEAM>(0, absent && ordered ? E : 0, tl, tbase, [&](int j) { return lu[j] > ts; });
    if (__ballot(known && !ordered) != 0) {
        int emx = known && !ordered ? E : 0;
#pragma unroll
        for (int s = 32; s >= TEAM; s >>= 1) {
            const int t = __shfl_xor(emx, s, 64);
            emx = t > emx ? t : emx;
        }
        for (int base = 0; base < emx; base += TEAM) {
            const int j = base + tl;
            const bool le = known && !ordered && j < E && j != at && lu[j] <= ts;
            const uint32_t tb = (uint32_t)(__ballot(le) >> tbase) & kTeamMask;
            if (tb) pos = base + (31 - __clz(tb)) + 1;
        }
    }

    // 3. the victims of an insert
    const int64_t w = (int64_t)o.arg, wabs = w < 0 ? -w : w;
    const bool op4 = o.op == MMP_COP_UBM_INSERT_NEW_ENTRY;
    const int64_t t0 = mg ? (int64_t)(int32_t)((uint32_t)u.total_unloading - (op4 ? (uint32_t)o.arg : 0u)) : 0;
    const int32_t bws = mg && op4 && o.arg != 0 ? res_clamp(t0, u.reserved, cap) : bw0;  // insertNewEntry's first adjustment, :134
    const int64_t total = ws + (int64_t)bws - (int64_t)bw0 + w;
    const int ubm = ub < pos ? ub : ub + 1;         // the pinned entry's merged index
    const int hi_v = mg ? ubm : E + 1;              // the most victims: the pinned entry stays
    const bool over = absent && total > cap && hi_v >= 1;
    // (vs: the manager's sum of the victims' weights; 0: adjustAggregateUnloadingWeight returns at once, :376)
    const auto bw_at = [&](int64_t vs) { return mg ? (vs == 0 ? bws : res_clamp(t0 + vs, u.reserved, cap)) : 0; };
    bool srch = over && ordered && w >= 0;
    if (srch && mg) srch = t0 + d.P[E] + w <= INT32_MAX;  // (t0 is an int and the weights are >= 0: no sum on the way wraps)
    int v = 0;
    int64_t after = total;
    int32_t bw_out = bws;
    if (__ballot(srch) != 0) {
        const int64_t *P = tabled ? d.P : nullptr;
        const auto M = [&](int j) { return j <= pos ? P[j] : P[j - 1] + w; };  // merged prefix, j in 0 .. E+1
        const auto left = [&](int j) {
            const int64_t m = M(j);
            return total - m + (int64_t)bw_at(m) - (int64_t)bws;
        };
        const int sv = team_search<TEAM>(srch ? 1 : 0, srch ? hi_v : 0, tl, tbase, [&](int j) { return left(j) <= cap; });
        if (srch) {
            v = sv;
            after = left(sv);
            bw_out = bw_at(M(sv));
        }
    }
    const bool walk = over && !srch;
    if (__ballot(walk) != 0) {
        int64_t size_carry = 0, sum_carry = 0;  // |weight| and signed weight of the merged entries in front of this trip
        bool done = !walk;
        for (int base = 0; __ballot(!done) != 0; base += TEAM) {
            const int j = base + tl + 1, e = j - 1;  // j victims: merged entries 0 .. e
            int64_t m = 0;
            if (!done && j <= hi_v) m = e < pos ? (int64_t)wt[e] : (e == pos ? w : (int64_t)wt[e - 1]);
            int64_t size_in = e == pos ? wabs : (m < 0 ? -m : m), sum_in = m;
            if (done || j > hi_v) size_in = 0;
#pragma unroll
            for (int s = 1; s < TEAM; s <<= 1) {
                const int64_t a = (int64_t)shfl_u64((uint64_t)size_in, tl >= s ? lane - s : lane);
                const int64_t b = (int64_t)shfl_u64((uint64_t)sum_in, tl >= s ? lane - s : lane);
                if (tl >= s) {
                    size_in += a;
                    sum_in += b;
                }
            }
            const int32_t bwj = bw_at(sum_carry + sum_in);
            const int64_t left = total - (size_carry + size_in) + (int64_t)bwj - (int64_t)bws;
            const uint32_t tb = (uint32_t)(__ballot(!done && j <= hi_v && (left <= cap || j == hi_v)) >> tbase) & kTeamMask;
            const int l = tb ? __ffs(tb) - 1 : 0;
            const int64_t left_at = (int64_t)shfl_u64((uint64_t)left, tbase + l);
            const int32_t bw_at_l = __shfl(bwj, tbase + l, 64);
            const int64_t size_last = (int64_t)shfl_u64((uint64_t)size_in, tbase + TEAM - 1);
            const int64_t sum_last = (int64_t)shfl_u64((uint64_t)sum_in, tbase + TEAM - 1);
            if (!done && tb) {
                v = base + l + 1;
                after = left_at;
                bw_out = bw_at_l;
                done = true;
            }
            size_carry += size_last;
            sum_carry += sum_last;
        }
    }

    if (in_range && tl == 0) {
        mmp_evict_k_out r;
        r.key_status = st;
        r.row = o.key;
        r.result = -1;
        r.n_evicted = 0; r.self_evicted = 0; r.insert_pos = 0; r.buffer_weight = 0; r.pad = 0;
        r.weighted_size = 0;
        r.oldest_time = -1;
        if (cache_ok) {  // (an unknown id: the state as it is, the `oldestTime` field as the last write left it)
            r.buffer_weight = bw0;
            r.weighted_size = ws;
            r.oldest_time = old_field;
        }
        if (present) {
            // touch and reposition (LinkedDeque.java:243-256), then the reader's updateOldestTime: the head's stamp
            r.result = 0;
            r.insert_pos = at;
            const bool stays = (at == 0 || lu[at - 1] <= ts) && (at == E - 1 || lu[at + 1] >= ts);
            int64_t head;
            if (stays)
                head = at == 0 ? ts : lu[0];
            else if (ordered)  // (only the head can have to move on a deque in time order, and then behind its neighbour)
                head = at == 0 ? lu[1] : lu[0];
            else
                head = pos == 0 ? ts : (at == 0 ? lu[1] : lu[0]);
            r.oldest_time = head;
        }
        if (absent) {
            r.result = 1;
            r.insert_pos = pos;
            r.n_evicted = v;
            r.self_evicted = v > pos ? 1 : 0;
            r.buffer_weight = mg ? bw_out : 0;
            r.weighted_size = after;
            // oldestTime(): the head of what is left, as evict_out_row reads it
            r.oldest_time = v <= E ? (v < pos ? lu[v] : (v == pos ? ts : lu[v - 1])) : -1;
        }
        A.outs[i] = r;
    }
}

}  // namespace mmp
