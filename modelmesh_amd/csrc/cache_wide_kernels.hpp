// cache_wide_kernels.hpp — the replay of a cache whose evictionDeque does not fit the LDS tile of cache_replay_kernel
// (cache_kernels.hpp): up to kCacheSlotsMax deque slots, the deque BLOCKED in global memory.  The rules are the ones of
// cache_kernels.hpp (apply_op, ubm_*, dq_evict: generic over the deque type); this file gives the blocked deque its primitives.
//
// A flat deque in global memory would move O(E) entries whenever an entry leaves the middle (every cache hit repositions one to
// the tail) and read O(E) keys per lookup, on a chain of dependent operations that one wavefront walks.  Instead:
//
//   blocks     kWideBlock = 128 slots each (columns lastUsed / weight / key), the live entries of block b in slots
//              [first, first + count).  Built with kWideFill = 64 entries per block; NB = ceil(slots / 64) + 1 blocks, so the block
//              behind the last used one is always there and empty.  Deque order = block order, then slot order.  A position is
//              b * 128 + slot.  Two copies: a re-spread writes the other one.
//   directory  per block {first, count} and the MINIMUM lastUsed of its entries, in the wavefront's LDS (12 bytes a block).  A pop
//              from the head advances `first`; LinkedDeque.insert's walk from the tail runs over the minima, 64 blocks a ballot,
//              and stops at the first block that holds an entry with lastUsed <= ts — which is where the flat walk stops, since
//              every block behind it holds none.
//   key index  open addressing in global memory, cells {key, block}, a power of two >= 2 x slots: 64 lanes probe 64 consecutive
//              cells (one coalesced load), then the <= 128 keys of that block.  A removed key leaves a tombstone; an insert takes
//              the first free cell; live cells + tombstones <= entries + inserts <= half the table, so a probe always ends.
//   full block the LAST block spills its upper half into the next, empty one; any other full block (and a last block with no
//              block behind it) re-spreads the cache to 64 per block, O(E) by the wavefront.
//
// Three launches: cache_wide_spread_kernel (grid over blocks: flat src -> blocks, keys into the index by atomicCAS),
// cache_wide_replay_kernel (one 64-lane workgroup per cache, wave_sync only), cache_wide_compact_kernel (grid over blocks:
// blocks -> flat dst at the offsets the replay left).  No workgroup barrier anywhere: every workgroup is one wavefront.
#pragma once
#include "cache_kernels.hpp"

namespace mmp {

constexpr int kWideBlock = 128, kWideFill = 64;
constexpr int kCacheSlotsMax = MMP_CACHE_SLOTS_MAX;
constexpr int kWideMaxBlocks = kCacheSlotsMax / kWideFill + 1;
constexpr int32_t kCellEmpty = -1, kCellDead = -2;  // a cell's block field; a table is cleared to 0xff bytes
static_assert(kWideMaxBlocks * 12 <= 65536, "the block directory exceeds the LDS of a launch");

struct WideDesc {  // one per cache on this route
    int32_t cache, nb;
    int32_t blk0;  // its first block among all blocks of the call
    int32_t tab0, tab_mask;  // its cells of the index
    int32_t stk0;  // its slots of the pending LIFO
};

struct WideArgs {
    const WideDesc *desc;
    int32_t n_wide, n_blocks;
    int64_t *lu0, *lu1;  // [n_blocks * 128] the two copies
    int32_t *wt0, *wt1, *key0, *key1;
    int64_t *bmin;   // [n_blocks] the directory as the spread builds it and the replay leaves it
    uint32_t *bfc;   // first | count << 16
    int32_t *bflat;  // a block's offset in the flat deque (replay -> compact)
    int32_t *cur;    // [n_wide] the copy that holds the result
    unsigned long long *tab;
    int32_t *stk_key, *stk_wt;
    int64_t *stk_lu;
};

__device__ __forceinline__ uint32_t wide_hash(int32_t k) { return (uint32_t)splitmix64((uint32_t)k); }

// the cache of block g: the last w with blk0 <= g
__device__ __forceinline__ int wide_of(const WideArgs &W, int g)
{
    int lo = 0, hi = W.n_wide;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (W.desc[mid].blk0 <= g)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(64) void cache_wide_spread_kernel(ReplayArgs A, WideArgs W)
{
    const int g = blockIdx.x, lane = lane_id();
    const WideDesc d = W.desc[wide_of(W, g)];
    const int b = g - d.blk0;
    const int rest = A.src.n[d.cache] - b * kWideFill;
    const int cnt = rest < 0 ? 0 : rest > kWideFill ? kWideFill : rest;
    int64_t m = INT64_MAX;
    if (lane < cnt) {
        const int e = A.src.off[d.cache] + b * kWideFill + lane;
        const size_t s = (size_t)g * kWideBlock + lane;
        const int32_t k = A.src.key[e];
        m = A.src.lu[e];
        W.lu0[s] = m;
        W.wt0[s] = A.src.wt[e];
        W.key0[s] = k;
        unsigned long long *tab = W.tab + d.tab0;
        const unsigned long long v = (unsigned long long)(uint32_t)k | ((unsigned long long)(uint32_t)b << 32);
        uint32_t q = wide_hash(k) & (uint32_t)d.tab_mask;
        for (int t = 0; t <= d.tab_mask; t++, q = (q + 1) & (uint32_t)d.tab_mask)
            if (atomicCAS(&tab[q], ~0ull, v) == ~0ull) break;
    }
    m = wave_min_i64(m);
    if (lane == 0) {
        W.bmin[g] = m;
        W.bfc[g] = (uint32_t)cnt << 16;
    }
}

__global__ __launch_bounds__(64) void cache_wide_compact_kernel(ReplayArgs A, WideArgs W)
{
    const int g = blockIdx.x, lane = lane_id();
    const int w = wide_of(W, g);
    const WideDesc d = W.desc[w];
    const bool one = W.cur[w] != 0;
    const int64_t *lu = one ? W.lu1 : W.lu0;
    const int32_t *wt = one ? W.wt1 : W.wt0, *key = one ? W.key1 : W.key0;
    const uint32_t fc = W.bfc[g];
    const int first = fc & 0xffff, count = fc >> 16;
    const int dn = A.dst.off[d.cache] + W.bflat[g];
    for (int j = lane; j < count; j += 64) {
        const size_t s = (size_t)g * kWideBlock + first + j;
        A.dst.lu[dn + j] = lu[s];
        A.dst.wt[dn + j] = wt[s];
        A.dst.key[dn + j] = key[s];
    }
}

struct BDeque : CacheRegs {
    int64_t *lu, *lu2;  // the copy in use and the other one (pointers to this cache's block 0)
    int32_t *wt, *wt2, *key, *key2;
    int64_t *dmin;  // LDS: the directory
    uint32_t *dfc;
    int2 *tab;  // {key, block}
    uint32_t mask;
    int nb, firstb, last;  // the first and last block with entries (equal, and empty, when n == 0)
    int cur;
    int32_t fkey;  // the key ix_find answered last and its cell (-1: none)
    int fcell;
};

__device__ __forceinline__ int bd_first(const BDeque &D, int b) { return D.dfc[b] & 0xffff; }
__device__ __forceinline__ int bd_count(const BDeque &D, int b) { return D.dfc[b] >> 16; }
__device__ __forceinline__ void bd_set(BDeque &D, int b, int first, int count, int64_t mn)
{
    wave_sync();
    if (lane_id() == 0) {
        D.dfc[b] = (uint32_t)first | ((uint32_t)count << 16);
        D.dmin[b] = mn;
    }
    wave_sync();
}

// the directory row of block b from its slots: an unlink or a touch may have taken the minimum away
__device__ __forceinline__ void bd_refresh(BDeque &D, int b, int first, int count)
{
    const int lane = lane_id();
    int64_t m = INT64_MAX;
    for (int j = lane; j < count; j += 64) {
        const int64_t v = D.lu[b * kWideBlock + first + j];
        m = v < m ? v : m;
    }
    m = wave_min_i64(m);
    bd_set(D, b, count ? first : 0, count, m);
}

// the live entry before / behind position p, -1 at the ends
__device__ __forceinline__ int bd_prev(const BDeque &D, int p)
{
    int b = p / kWideBlock;
    if ((p & (kWideBlock - 1)) > bd_first(D, b)) return p - 1;
    for (b--; b >= D.firstb; b--)
        if (bd_count(D, b)) return b * kWideBlock + bd_first(D, b) + bd_count(D, b) - 1;
    return -1;
}
__device__ __forceinline__ int bd_next(const BDeque &D, int p)
{
    int b = p / kWideBlock;
    if ((p & (kWideBlock - 1)) < bd_first(D, b) + bd_count(D, b) - 1) return p + 1;
    for (b++; b <= D.last; b++)
        if (bd_count(D, b)) return b * kWideBlock + bd_first(D, b);
    return -1;
}

// ---- the key index ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int ix_find(BDeque &D, int32_t k)
{
    if (D.fcell >= 0 && D.fkey == k) return D.fcell;
    const uint32_t h = wide_hash(k);
    for (uint32_t p = 0; p <= D.mask; p += 64) {
        const int2 c = D.tab[(h + p + lane_id()) & D.mask];
        const uint64_t hit = __ballot(c.y >= 0 && c.x == k);
        if (hit) {
            D.fkey = k;
            D.fcell = (int)((h + p + (uint32_t)(__ffsll((unsigned long long)hit) - 1)) & D.mask);
            return D.fcell;
        }
        if (__ballot(c.y == kCellEmpty)) return -1;
    }
    return -1;
}

__device__ __forceinline__ void ix_set(BDeque &D, int cell, int32_t blk)
{
    wave_sync();
    if (lane_id() == 0) D.tab[cell].y = blk;
    wave_sync();
}

// an absent key into the first free cell of its probe sequence
__device__ __forceinline__ void ix_add(BDeque &D, int32_t k, int32_t blk)
{
    const uint32_t h = wide_hash(k);
    for (uint32_t p = 0; p <= D.mask; p += 64) {
        const uint64_t free = __ballot(D.tab[(h + p + lane_id()) & D.mask].y < 0);
        if (!free) continue;
        const int cell = (int)((h + p + (uint32_t)(__ffsll((unsigned long long)free) - 1)) & D.mask);
        wave_sync();
        if (lane_id() == 0) D.tab[cell] = make_int2(k, blk);
        wave_sync();
        D.fkey = k;
        D.fcell = cell;
        return;
    }
}

// ONE LANE's key moved to block blk (lanes run this side by side on different keys: no ballot, no wave_sync in here)
__device__ __forceinline__ void ix_move_lane(BDeque &D, int32_t k, int32_t blk)
{
    uint32_t q = wide_hash(k) & D.mask;
    for (uint32_t t = 0; t <= D.mask; t++, q = (q + 1) & D.mask) {
        const int2 c = D.tab[q];
        if (c.y >= 0 && c.x == k) {
            D.tab[q].y = blk;
            return;
        }
        if (c.y == kCellEmpty) return;
    }
}

// ---- blocks ---------------------------------------------------------------------------------------------------------
// slots [lo, hi) one slot towards the tail (d = 1, tail chunk first) or the head (d = -1, head chunk first)
__device__ __forceinline__ void bd_shift(BDeque &D, int lo, int hi, int d)
{
    const int lane = lane_id();
    for (int done = 0; done < hi - lo; done += 64) {
        int a = d > 0 ? hi - done - 64 : lo + done, z = a + 64;
        a = a < lo ? lo : a;
        z = z > hi ? hi : z;
        const int i = a + lane;
        const bool v = i < z;
        int64_t t = 0;
        int32_t w = 0, k = 0;
        if (v) {
            t = D.lu[i];
            w = D.wt[i];
            k = D.key[i];
        }
        wave_sync();
        if (v) {
            D.lu[i + d] = t;
            D.wt[i + d] = w;
            D.key[i + d] = k;
        }
        wave_sync();
    }
}

// the entry at p leaves its block (the index is the caller's)
__device__ __forceinline__ void bd_remove_at(BDeque &D, int p)
{
    const int b = p / kWideBlock;
    int first = bd_first(D, b), count = bd_count(D, b);
    const int j = (p & (kWideBlock - 1)) - first;
    if (j == 0)
        first++;
    else if (j < count - 1)
        bd_shift(D, p + 1, b * kWideBlock + first + count, -1);
    count--;
    D.n--;
    bd_refresh(D, b, first, count);
    if (count == 0) {
        if (D.n == 0)
            D.firstb = D.last = b;
        else {
            while (D.firstb < D.last && bd_count(D, D.firstb) == 0) D.firstb++;
            while (D.last > D.firstb && bd_count(D, D.last) == 0) D.last--;
        }
    }
}

// LinkedDeque.insert's walk (LinkedDeque.java:259-288) over the directory, then inside the block it stops in: the block b and
// the index idx among b's live entries at which a node stamped ts is linked
__device__ __forceinline__ void bd_locate(const BDeque &D, int64_t ts, int &b, int &idx)
{
    const int lane = lane_id();
    b = -1;
    for (int base = D.last & ~63; base >= 0; base -= 64) {
        const int i = base + lane;
        const uint64_t hit = __ballot(i <= D.last && D.dmin[i] <= ts);
        if (hit) {
            b = base + 63 - __clzll((unsigned long long)hit);
            break;
        }
    }
    if (b < 0) {  // older than everything: the new head
        b = D.firstb;
        idx = 0;
        return;
    }
    const int first = bd_first(D, b), count = bd_count(D, b), at = b * kWideBlock + first;
    const uint64_t hi = __ballot(lane + 64 < count && D.lu[at + 64 + lane] <= ts);
    if (hi) {
        idx = 64 + 64 - __clzll((unsigned long long)hi);
        return;
    }
    const uint64_t lo = __ballot(lane < count && D.lu[at + lane] <= ts);
    idx = lo ? 64 - __clzll((unsigned long long)lo) : 0;
}

// the full last block b hands its upper half to the empty block behind it
__device__ __forceinline__ void bd_spill(BDeque &D, int b)
{
    const int lane = lane_id(), from = b * kWideBlock + kWideFill + lane, to = (b + 1) * kWideBlock + lane;
    const int32_t k = D.key[from];
    D.lu[to] = D.lu[from];
    D.wt[to] = D.wt[from];
    D.key[to] = k;
    ix_move_lane(D, k, b + 1);
    wave_sync();
    bd_refresh(D, b, 0, kWideFill);
    bd_refresh(D, b + 1, 0, kWideFill);
    D.last = b + 1;
}

// every entry into the other copy, kWideFill per block from block 0
__device__ __forceinline__ void bd_respread(BDeque &D)
{
    const int lane = lane_id();
    int f = 0;
    for (int b = D.firstb; b <= D.last; b++) {
        const int first = bd_first(D, b), count = bd_count(D, b);
        for (int j = lane; j < count; j += 64) {
            const int from = b * kWideBlock + first + j, g = f + j, to = (g / kWideFill) * kWideBlock + (g % kWideFill);
            const int32_t k = D.key[from];
            D.lu2[to] = D.lu[from];
            D.wt2[to] = D.wt[from];
            D.key2[to] = k;
            ix_move_lane(D, k, g / kWideFill);
        }
        f += count;
    }
    wave_sync();
    int64_t *const l = D.lu;
    int32_t *const w = D.wt, *const k = D.key;
    D.lu = D.lu2, D.wt = D.wt2, D.key = D.key2;
    D.lu2 = l, D.wt2 = w, D.key2 = k;
    D.cur ^= 1;
    const int used = (f + kWideFill - 1) / kWideFill;
    for (int b = 0; b < used; b++) bd_refresh(D, b, 0, f - b * kWideFill < kWideFill ? f - b * kWideFill : kWideFill);
    wave_sync();
    for (int b = used + lane; b < D.nb; b += 64) {
        D.dfc[b] = 0;
        D.dmin[b] = INT64_MAX;
    }
    wave_sync();
    D.firstb = 0;
    D.last = used ? used - 1 : 0;
}

// a node stamped ts into the blocks (the index is the caller's); returns its position
__device__ __forceinline__ int bd_place(BDeque &D, int64_t ts, int32_t w, int32_t k)
{
    int b, idx;
    bd_locate(D, ts, b, idx);
    if (bd_count(D, b) == kWideBlock) {
        if (b == D.last && b + 1 < D.nb) {
            bd_spill(D, b);
            if (idx > kWideFill) {
                b++;
                idx -= kWideFill;
            }
        } else {
            bd_respread(D);
            bd_locate(D, ts, b, idx);
        }
    }
    int first = bd_first(D, b);
    const int count = bd_count(D, b), at = b * kWideBlock;
    if (first + count < kWideBlock)
        bd_shift(D, at + first + idx, at + first + count, 1);
    else {
        bd_shift(D, at + first, at + first + idx, -1);
        first--;
    }
    const int p = at + first + idx;
    if (lane_id() == 0) {
        D.lu[p] = ts;
        D.wt[p] = w;
        D.key[p] = k;
    }
    const int64_t m = D.dmin[b];
    bd_set(D, b, first, count + 1, ts < m ? ts : m);
    if (D.n == 0) D.firstb = D.last = b;
    if (b > D.last) D.last = b;
    D.n++;
    return p;
}

// ---- the primitives the rules of cache_kernels.hpp are written in -----------------------------------------------------
__device__ __forceinline__ int dq_head(const BDeque &D) { return D.firstb * kWideBlock + bd_first(D, D.firstb); }
__device__ __forceinline__ int64_t dq_lu(const BDeque &D, int p) { return D.lu[p]; }
__device__ __forceinline__ int32_t dq_wt(const BDeque &D, int p) { return D.wt[p]; }

template <int TW>
__device__ __forceinline__ int dq_find(BDeque &D, int32_t k)
{
    const int cell = ix_find(D, k);
    if (cell < 0) return -1;
    const int b = D.tab[cell].y, lane = lane_id();
    const int count = bd_count(D, b), at = b * kWideBlock + bd_first(D, b);
    const uint64_t lo = __ballot(lane < count && D.key[at + lane] == k);
    if (lo) return at + __ffsll((unsigned long long)lo) - 1;
    const uint64_t hi = __ballot(lane + 64 < count && D.key[at + 64 + lane] == k);
    return hi ? at + 64 + __ffsll((unsigned long long)hi) - 1 : -1;
}

template <int TW>
__device__ __forceinline__ int dq_insert(BDeque &D, int64_t ts, int32_t w, int32_t k)
{
    const int p = bd_place(D, ts, w, k);
    ix_add(D, k, p / kWideBlock);
    return p;
}

template <int TW>
__device__ __forceinline__ void dq_unlink(BDeque &D, int p, int64_t &ts, int32_t &w, int32_t &k)
{
    ts = D.lu[p];
    w = D.wt[p];
    k = D.key[p];
    wave_sync();
    const int cell = ix_find(D, k);
    bd_remove_at(D, p);
    if (cell >= 0) ix_set(D, cell, kCellDead);
    D.fcell = -1;
}

template <int TW>
__device__ __forceinline__ void dq_touch(BDeque &D, int p, int64_t time, int64_t now)
{
    const int64_t old = D.lu[p];
    const int64_t nv = time == 0 ? now : (old > time ? old : time);
    wave_sync();
    if (lane_id() == 0) D.lu[p] = nv;
    wave_sync();
    const int b = p / kWideBlock;
    bd_refresh(D, b, bd_first(D, b), bd_count(D, b));
}

// LinkedDeque.reposition: the neighbours are the live entries before and behind, in whichever block
template <int TW>
__device__ __forceinline__ void dq_reposition(BDeque &D, int p)
{
    const int64_t lu = D.lu[p];
    const int prev = bd_prev(D, p), next = bd_next(D, p);
    if (prev < 0 || D.lu[prev] <= lu) {
        if (next < 0 || D.lu[next] >= lu) return;
    }
    const int32_t w = D.wt[p], k = D.key[p];
    wave_sync();
    const int cell = ix_find(D, k);
    bd_remove_at(D, p);
    const int q = bd_place(D, lu, w, k);
    if (cell >= 0) ix_set(D, cell, q / kWideBlock);
}

template <int TW>
__device__ __forceinline__ void dq_set_wt(BDeque &D, int p, int32_t w)
{
    wave_sync();
    if (lane_id() == 0) D.wt[p] = w;
    wave_sync();
}

__device__ __forceinline__ void dq_refresh_oldest(BDeque &D) { D.oldest = D.n ? D.lu[dq_head(D)] : -1; }

// One 64-lane workgroup per cache of W.desc.  Dynamic LDS: 12 bytes per block of the largest cache.
template <bool TIMES>
__global__ __launch_bounds__(64) void cache_wide_replay_kernel(ReplayArgs A, WideArgs W, int32_t max_nb)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int wi = blockIdx.x, lane = lane_id();
    const WideDesc d = W.desc[wi];
    const int c = d.cache;
    BDeque D;
    D.dmin = reinterpret_cast<int64_t *>(smem);
    D.dfc = reinterpret_cast<uint32_t *>(D.dmin + max_nb);
    const size_t at = (size_t)d.blk0 * kWideBlock;
    D.lu = W.lu0 + at, D.wt = W.wt0 + at, D.key = W.key0 + at;
    D.lu2 = W.lu1 + at, D.wt2 = W.wt1 + at, D.key2 = W.key1 + at;
    D.tab = reinterpret_cast<int2 *>(W.tab + d.tab0);
    D.mask = (uint32_t)d.tab_mask;
    D.stk_key = W.stk_key + d.stk0;
    D.stk_wt = W.stk_wt + d.stk0;
    D.stk_lu = W.stk_lu + d.stk0;
    D.nb = d.nb;
    D.cur = 0;
    D.fcell = -1;
    D.fkey = 0;
    D.sp = 0;
    D.n = A.src.n[c];
    D.firstb = 0;
    D.last = D.n ? (D.n - 1) / kWideFill : 0;
    for (int b = lane; b < d.nb; b += 64) {
        D.dmin[b] = W.bmin[d.blk0 + b];
        D.dfc[b] = W.bfc[d.blk0 + b];
    }
    wave_sync();
    D.wsize = A.weighted_size[c];
    D.oldest = A.oldest[c];
    D.cap = A.capacity[c];
    const mmp_ubm_state u = A.ubm[c];
    D.reserved = u.reserved;
    D.tu = u.total_unloading;
    D.occ = u.total_occupancy;
    D.deficit = u.cache_deficit;
    D.ev = A.evicted + A.ev_off[c];
    if constexpr (TIMES) D.ev_lu = A.evicted_lu + A.ev_off[c];
    D.nev = 0;
    const int o0 = A.op_off[c], o1 = A.op_off[c + 1];
    for (int q = o0; q < o1; q++) {
        const mmp_cache_op o = A.ops[q];
        const int ev0 = D.nev;
        const int32_t res = apply_op<64, TIMES>(D, o, A.now);
        const int ubi = u.reserved >= 0 ? dq_find<64>(D, MMP_UNLOADBUF_KEY_C) : -1;
        if (lane == 0) {
            mmp_cache_op_out r;
            r.result = res;
            r.n_evicted = D.nev - ev0;
            r.evicted_off = A.ev_off[c] + ev0;
            r.buffer_weight = ubi >= 0 ? D.wt[ubi] : 0;
            r.weighted_size = D.wsize;
            r.oldest_time = D.oldest;
            A.outs[A.op_order[q]] = r;
        }
        wave_sync();
    }
    // where each block goes in the flat deque
    int run = 0;
    for (int base = 0; base < d.nb; base += 64) {
        const int b = base + lane;
        const uint32_t fc = b < d.nb ? D.dfc[b] : 0;
        const int32_t incl = wave_incl_scan_i32((int32_t)(fc >> 16));
        if (b < d.nb) {
            W.bfc[d.blk0 + b] = fc;
            W.bflat[d.blk0 + b] = run + incl - (int32_t)(fc >> 16);
        }
        run += shfl_i32(incl, 63);
    }
    if (lane == 0) {
        W.cur[wi] = D.cur;
        A.dst.n[c] = D.n;
        A.weighted_size[c] = D.wsize;
        A.oldest[c] = D.oldest;
        A.capacity[c] = D.cap;
        mmp_ubm_state v = u;
        v.total_unloading = D.tu;
        v.total_occupancy = D.occ;
        v.cache_deficit = D.deficit;
        A.ubm[c] = v;
    }
}

}  // namespace mmp
