// janitor_kernels.hpp — what every instance's janitorTask does BEFORE the scale-down of copies: the cache loop
// (MM.java:5892-6008) and the registry loop (:6014-6108), joined against the resident registry at one clock value.
// (The scale-down itself, :6110-6145 with removeModelCopies, is rebalance_kernels.hpp.)
//
// The cache is keyed by model id, so a model meets at most one cache row and its record is decided from that row alone
// (janitor_eval: the cache loop's step, then the registry loop's step on the record as the first left it).  Two things couple
// the models.  The Long.MAX_VALUE stop (:5929) ends the run at the FIRST such row: a minimum over the row index, taken by the
// entry kernel before anything is evaluated, so that no lane evaluates a row it should not have reached.  The TreeSet of
// candidates under VALUE_COMP (:6875-6881) keeps the first of equal times and hands them out oldest first: a rank.
//
//   janitor_entry_kernel    one lane per cache row: model -> row into the map (M int32 words of context scratch, all -1
//                           between runs), the stop index
//   janitor_count_kernel    one lane per model: row, map word, entry walk for self_pod; a model with neither an entry for
//                           self_pod nor a cache row ends there.  Per-workgroup counts of (edits, candidates, entries kept)
//   prune_scan_kernel       (registry_kernels.hpp) the one-workgroup scan of those triples (protocol: triple_count there)
//   janitor_scatter_kernel  the same walk: edits in registry order, candidates (time, row) in registry order
//   janitor_tie_kernel      a candidate is dropped when an EARLIER one (registry order) has its time       } all pairs over the
//   janitor_rank_kernel     rank = kept candidates with a smaller time; the candidate row scattered there  } candidates, for
//                           every size: the count is bounded by the cache rows (16k rows: 2.7e8 compares), a workgroup per 64
//                           candidates whose waves hand the other candidates round from registers (measured figures:
//                           profiles/janitor/).  rank_sample.hpp ranks mmp_pod_row under the placement comparator and does
//                           not fit a bare int64 key.  Deterministic: counts, no atomics on positions.
//   janitor_finish_kernel   one lane per cache row: the row's action byte (the same janitor_eval on its model), the per-action
//                           totals, and the map word cleared again — no M-sized memset per run
//   janitor_build_kernel    (apply) one lane per edit: the record's entries appended to the arena without / with self_pod's,
//                           the row staged for upsert_models_kernel
#pragma once
#include "registry_kernels.hpp"

namespace mmp {

struct JanitorScalars {
    int32_t stop_inv;  // max over stopping rows of (n - row); 0 = no stop
    int32_t n_cands, n_ties;
    int32_t n_action[7];
    int32_t n_dup;  // by key (tasks_keyed_kernels.hpp): entries whose resolved row another entry of the call had claimed
};

constexpr int kJanBlock = kCompactBlock;

// one model's outcome
struct JanEval {
    uint32_t flags;  // MMP_JANITOR_EDIT_*; != 0 <=> the record changes
    int32_t nl, nf;  // counts after
    int64_t last_used, last_unload, ins_time;
    int32_t ins_pos;
    uint8_t action;  // of the model's cache row
    bool cand;
    int64_t cand_time;
};

// where self_pod stands in a record
struct JanSelf {
    int32_t li, fi, ins;  // position in instanceIds / loadFailedInstanceIds (-1: absent); where a new instanceIds entry goes
    int64_t lt, ft;
};

__device__ __forceinline__ JanSelf janitor_find_self(const mmp_model_row &m, const int32_t *__restrict__ ent_pod,
                                                     const int64_t *__restrict__ ent_time, int32_t self_pod)
{
    JanSelf s{-1, -1, -1, 0, 0};
    const int32_t n = m.n_loaded + m.n_failed;
    for (int32_t k = 0; k < n; k++) {
        if (ent_pod[m.ent_off + k] != self_pod) continue;
        if (k < m.n_loaded) {
            s.li = k;
            s.lt = ent_time[m.ent_off + k];
        } else {
            s.fi = k - m.n_loaded;
            s.ft = ent_time[m.ent_off + k];
        }
    }
    return s;
}

// TreeMap.put of a new key: in front of the first RESOLVED entry whose id is greater; unresolved entries are never compared
__device__ __forceinline__ int32_t janitor_insert_pos(const mmp_model_row &m, const int32_t *__restrict__ ent_pod,
                                                      const mmp_pod_row *__restrict__ pods, int32_t P, int32_t self_pod)
{
    const uint32_t mine = pods[self_pod].id_order;
    for (int32_t k = 0; k < m.n_loaded; k++) {
        const int32_t pod = ent_pod[m.ent_off + k];
        if (pod >= 0 && pod < P && pods[pod].id_order > mine) return k;
    }
    return m.n_loaded;
}

// updateLastUsedTimeInRegistryIfStale (:6165-6181): whether it gets as far as updateLastUsed
__device__ __forceinline__ bool janitor_stale(int64_t last_used, int64_t rec_last_used, const mmp_janitor_params &p)
{
    if (last_used == INT64_MAX) return false;                                   // :6167
    return !(jsub64(last_used, rec_last_used) < p.min_stale_age_ms);            // :6174
}

// The cache loop's verdict on one row, the record aside: 0 skipped, 1 the stop, 2 recently used, 3 goes on to the timestamps
__device__ __forceinline__ int janitor_row_class(const mmp_janitor_entry &e, const mmp_janitor_params &p)
{
    if (!(e.flags & MMP_JE_DONE)) return 0;                                                             // :5905
    if (e.last_used <= 0) return 0;                                                                     // :5910
    if (e.last_used == INT64_MAX) return 1;                                                             // :5921
    if (jsub64(p.now, e.last_used) < p.janitor_freq_secs * 2000 + p.load_timeout_ms) return 2;          // :5933 (strict)
    return 3;
}

// A cache row whose model the registry does not hold (registry.get == null, :5919).
__device__ __forceinline__ uint8_t janitor_eval_unregistered(const mmp_janitor_entry &e, int32_t row, int32_t stop, const mmp_janitor_params &p)
{
    if (row > stop) return MMP_JANITOR_NONE;
    const int c = janitor_row_class(e, p);
    return c == 1 ? MMP_JANITOR_REPAIRED : c == 3 ? MMP_JANITOR_REMOVED : MMP_JANITOR_NONE;             // :5968 mr == null
}

// One model: the cache loop's step for its row (if it has one and the run got that far), then the registry loop's step.
__device__ __forceinline__ JanEval janitor_eval(const mmp_model_row &m, const JanSelf &s, const mmp_janitor_entry *__restrict__ entries,
                                                int32_t row, int32_t stop, bool stopped, const mmp_janitor_params &p)
{
    JanEval r{};
    r.action = MMP_JANITOR_NONE;
    r.ins_pos = -1;
    int64_t rec_lu = m.last_used;
    bool loaded = s.li >= 0, failed_has = s.fi >= 0, registered = false;
    const bool ce = row >= 0;
    mmp_janitor_entry e{};
    if (ce) e = entries[row];
    bool in_cache = ce;
    const bool ce_failed = ce && (e.flags & MMP_JE_FAILED);
    auto update_last_used = [&](int64_t t) {  // ModelRecord.java:239-246 (t != 0 wherever this is reached)
        if (t > rec_lu) {
            rec_lu = t;
            r.flags |= MMP_JANITOR_EDIT_TOUCHED;
        }
    };
    if (ce && row <= stop) {
        const int c = janitor_row_class(e, p);
        if (c == 1) {
            r.action = MMP_JANITOR_REPAIRED;
            if (rec_lu == INT64_MAX) {  // repairLastUsedTimeIfNeeded, :6843-6844
                rec_lu = (int64_t)((uint64_t)p.now - 3ull * (uint64_t)p.lastused_age_on_add_ms);
                r.flags |= MMP_JANITOR_EDIT_REPAIRED;
            }
        } else if (c == 2) {
            if (janitor_stale(e.last_used, rec_lu, p)) {  // :5937
                update_last_used(e.last_used);
                r.action = MMP_JANITOR_REFRESHED;
            }
        } else if (c == 3) {
            const bool has = ce_failed ? failed_has : loaded;                                 // :5950
            const int64_t reg_ts = ce_failed ? s.ft : s.lt;                                   // :5953
            const int64_t local = ce_failed ? e.load_complete_timestamp : e.load_timestamp;   // :5952
            if (has && reg_ts == local) {                                                     // :5954
                if (janitor_stale(e.last_used, rec_lu, p)) {
                    update_last_used(e.last_used);
                    r.action = MMP_JANITOR_REFRESHED;
                } else
                    r.action = MMP_JANITOR_IN_ORDER;
            } else if (!(e.flags & MMP_JE_STATE_LIVE) || age_of(e.last_unload_attempt_time, p.now) < p.unload_attempt_recent_ms) {  // :5968-5969
                r.action = MMP_JANITOR_REMOVED;
                in_cache = false;
            } else {                                                                          // :5980-5982
                r.flags |= MMP_JANITOR_EDIT_REGISTERED;
                if (!ce_failed && loaded) r.flags |= MMP_JANITOR_EDIT_TIMESTAMP_MISMATCH;     // :5959, :5985
                registered = loaded = true;
                failed_has = false;
                update_last_used(e.last_used);
                r.ins_time = e.load_timestamp;
                r.action = MMP_JANITOR_REGISTERED;
            }
        }
    }
    bool rem_loaded = false, rem_failed = false;
    if (!stopped && (loaded || failed_has)) {                                                 // :6030
        const int64_t glut = in_cache ? e.last_used : -1;                                     // runtimeCache.getLastUsedTime
        rem_loaded = loaded && (!ce || ce_failed);                                            // :6039
        if (failed_has) {
            if (ce && !ce_failed)                                                             // :6042
                rem_failed = true;
            else {
                const bool shorter = glut > 0 && jsub64(p.now, glut) < p.short_expiry_recent_use_ms;  // :6047
                const int64_t expiry = shorter ? p.load_failure_expiry_ms / 2 : p.load_failure_expiry_ms;
                rem_failed = jsub64(p.now, s.ft) > expiry;                                    // :6049 (strict)
            }
        }
        if (rem_loaded) r.flags |= MMP_JANITOR_EDIT_REM_LOADED | MMP_JANITOR_EDIT_UNLOAD_SET;
        if (rem_failed) r.flags |= MMP_JANITOR_EDIT_REM_FAILED;
        if ((rem_loaded || rem_failed) && ce && glut > 0) update_last_used(glut);             // :6066-6073
        if (rem_failed && ce_failed) {                                                        // :6089-6091
            if (in_cache) r.action = MMP_JANITOR_EXPIRED;
        } else if (loaded && !rem_loaded && glut > 0) {                                       // :6092-6099
            r.cand = true;
            r.cand_time = glut;
        }
    }
    r.nl = m.n_loaded + ((registered && s.li < 0) ? 1 : 0) - (rem_loaded ? 1 : 0);
    r.nf = m.n_failed - ((s.fi >= 0 && (registered || rem_failed)) ? 1 : 0);
    r.last_used = rec_lu;
    r.last_unload = (rem_loaded && r.nl > 2) ? p.now : 0;                                     // ModelRecord.java:260-262
    if (registered && !rem_loaded) r.ins_pos = s.li >= 0 ? s.li : s.ins;
    return r;
}

__global__ void janitor_entry_kernel(const mmp_janitor_entry *__restrict__ entries, int32_t n, int32_t *__restrict__ map,
                                     mmp_janitor_params p, JanitorScalars *js)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const mmp_janitor_entry e = entries[r];
    if (e.model >= 0) map[e.model] = r;  // (the host checked the range and that no model has two rows)
    if (janitor_row_class(e, p) == 1) atomicMax(&js->stop_inv, n - r);
}

// the model's evaluation for the count and scatter passes; `live` = there is anything to evaluate
__device__ __forceinline__ bool janitor_model(const mmp_model_row *__restrict__ models, int32_t i, const int32_t *__restrict__ ent_pod,
                                              const int64_t *__restrict__ ent_time, const mmp_pod_row *__restrict__ pods, int32_t P,
                                              const int32_t *__restrict__ map, const mmp_janitor_entry *__restrict__ entries, int32_t n,
                                              const mmp_janitor_params &p, const JanitorScalars *js, JanEval &ev, int32_t &row)
{
    const mmp_model_row m = models[i];
    JanSelf s = janitor_find_self(m, ent_pod, ent_time, p.self_pod);
    row = map[i];
    if (row < 0 && s.li < 0 && s.fi < 0) return false;
    const int32_t inv = js->stop_inv;
    const bool stopped = inv > 0;
    const int32_t stop = stopped ? n - inv : INT32_MAX;
    if (row >= 0 && s.li < 0) s.ins = janitor_insert_pos(m, ent_pod, pods, P, p.self_pod);
    ev = janitor_eval(m, s, entries, row, stop, stopped, p);
    return true;
}

// (its own copy of triple_count: with the helper this kernel took two more VGPRs and two more SGPRs)
__global__ __launch_bounds__(kJanBlock) void janitor_count_kernel(const mmp_model_row *__restrict__ models, int32_t M,
                                                                  const int32_t *__restrict__ ent_pod, const int64_t *__restrict__ ent_time,
                                                                  const mmp_pod_row *__restrict__ pods, int32_t P,
                                                                  const int32_t *__restrict__ map,
                                                                  const mmp_janitor_entry *__restrict__ entries, int32_t n,
                                                                  mmp_janitor_params p, const JanitorScalars *js,
                                                                  int32_t *__restrict__ block_counts)
{
    __shared__ int32_t s_e[kJanBlock / 64], s_c[kJanBlock / 64], s_k[kJanBlock / 64];
    const int i = blockIdx.x * kJanBlock + threadIdx.x;
    bool edit = false, cand = false;
    int32_t kept = 0;
    if (i < M) {
        JanEval ev;
        int32_t row;
        if (janitor_model(models, i, ent_pod, ent_time, pods, P, map, entries, n, p, js, ev, row)) {
            edit = ev.flags != 0;
            cand = ev.cand;
            if (edit) kept = ev.nl + ev.nf;
        }
    }
    const int ne = __popcll(__ballot(edit)), nc = __popcll(__ballot(cand));
    const int32_t nk = wave_sum_i32(kept);
    const int w = threadIdx.x >> 6;
    if (lane_id() == 0) {
        s_e[w] = ne;
        s_c[w] = nc;
        s_k[w] = nk;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t a = 0, b = 0, c = 0;
        for (int x = 0; x < kJanBlock / 64; x++) {
            a += s_e[x];
            b += s_c[x];
            c += s_k[x];
        }
        block_counts[3 * blockIdx.x + 0] = a;
        block_counts[3 * blockIdx.x + 1] = b;
        block_counts[3 * blockIdx.x + 2] = c;
    }
}

// edits in registry order (bounded by max_edits: a truncated prefix), candidates in registry order (never more than n)
__global__ __launch_bounds__(kJanBlock) void janitor_scatter_kernel(const mmp_model_row *__restrict__ models, int32_t M,
                                                                    const int32_t *__restrict__ ent_pod, const int64_t *__restrict__ ent_time,
                                                                    const mmp_pod_row *__restrict__ pods, int32_t P,
                                                                    const int32_t *__restrict__ map,
                                                                    const mmp_janitor_entry *__restrict__ entries, int32_t n,
                                                                    mmp_janitor_params p, const JanitorScalars *js,
                                                                    const int32_t *__restrict__ block_off, const PruneScalars *ps,
                                                                    mmp_janitor_edit *__restrict__ edits, int32_t max_edits,
                                                                    int32_t *__restrict__ keep_off, int64_t *__restrict__ cand_time,
                                                                    int32_t *__restrict__ cand_row)
{
    if (ps->n_edits == 0 && ps->n_removed == 0) return;  // (uniform: the whole grid leaves)
    const int i = blockIdx.x * kJanBlock + threadIdx.x;
    JanEval ev{};
    int32_t row = -1, kept = 0;
    bool edit = false, cand = false;
    if (i < M && janitor_model(models, i, ent_pod, ent_time, pods, P, map, entries, n, p, js, ev, row)) {
        edit = ev.flags != 0;
        cand = ev.cand;
        if (edit) kept = ev.nl + ev.nf;
    }
    const TripleOff o = triple_offsets<kCol1Count>(edit, cand, kept, block_off);
    if (edit) {
        const int32_t x = o.e;
        if (x < max_edits) {
            mmp_janitor_edit ed;
            ed.model = i;
            ed.n_loaded_after = ev.nl;
            ed.n_failed_after = ev.nf;
            ed.flags = ev.flags;
            ed.last_used_after = ev.last_used;
            ed.last_unload_after = ev.last_unload;
            ed.inserted_time = ev.ins_time;
            ed.inserted_pos = ev.ins_pos;
            ed.entry = row;
            edits[x] = ed;
            keep_off[x] = o.k;
        }
    }
    if (cand) {
        const int32_t x = o.r;
        if (x < n) {  // (a candidate has a cache row of its own: there are never more than n)
            cand_time[x] = ev.cand_time;
            cand_row[x] = row;
        }
    }
}

// lane k's 64-bit value to every lane (k is uniform: two v_readlane, no memory)
__device__ __forceinline__ int64_t wave_bcast_i64(int64_t v, int k)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)v, k);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), k);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

constexpr int kJanTile = 64;  // candidates per workgroup of the two all-pairs kernels: one per lane; its four waves share the tiles

// dropped[i] = an earlier candidate (registry order) has the same time: TreeSet.add under VALUE_COMP returns false.
// One workgroup per 64 candidates i (a lane each, in every wave); the tiles of 64 candidates j in front of them are dealt to the
// four waves, a lane loads one j and the wave hands the 64 values round from registers.
__global__ __launch_bounds__(256) void janitor_tie_kernel(const int64_t *__restrict__ cand_time, const PruneScalars *ps,
                                                          uint8_t *__restrict__ dropped, JanitorScalars *js)
{
    __shared__ int32_t s_hit[kJanTile];
    const int32_t nc = ps->n_removed;  // (the scan's second total: the candidates)
    const int i0 = blockIdx.x * kJanTile;
    if (i0 >= nc) return;  // (uniform)
    const int lane = lane_id(), w = threadIdx.x >> 6;
    if (w == 0) s_hit[lane] = 0;
    __syncthreads();
    const int i = i0 + lane;
    const int64_t mine = i < nc ? cand_time[i] : 0;
    bool hit = false;
    int t = w;
    int64_t v = (t <= (int)blockIdx.x && t * kJanTile + lane < nc) ? cand_time[t * kJanTile + lane] : 0;
    for (; t <= (int)blockIdx.x; t += 4) {  // only candidates in front of this workgroup's last: tiles 0 .. its own
        const int tn = t + 4;
        const int64_t vn = (tn <= (int)blockIdx.x && tn * kJanTile + lane < nc) ? cand_time[tn * kJanTile + lane] : 0;  // the next tile, ahead
#pragma unroll
        for (int k = 0; k < kJanTile; k++) hit |= (wave_bcast_i64(v, k) == mine) && (t * kJanTile + k < i);  // j < i < nc
        v = vn;
    }
    if (hit && i < nc) s_hit[lane] = 1;  // (every writer stores the same word)
    __syncthreads();
    if (w != 0) return;
    const bool drop = i < nc && s_hit[lane];
    if (i < nc) dropped[i] = drop ? 1 : 0;
    const int nd = __popcll(__ballot(drop)), nk = __popcll(__ballot(i < nc && !drop));
    if (lane == 0) {
        if (nd) atomicAdd(&js->n_ties, nd);
        if (nk) atomicAdd(&js->n_cands, nk);
    }
}

// a kept candidate's place = kept candidates with a smaller time; it goes there as a complete mmp_cache_entry.  The same shape
// as the tie kernel, over all tiles; the four waves' partial counts meet in LDS.
__global__ __launch_bounds__(256) void janitor_rank_kernel(const int64_t *__restrict__ cand_time, const int32_t *__restrict__ cand_row,
                                                           const uint8_t *__restrict__ dropped, const PruneScalars *ps,
                                                           const mmp_janitor_entry *__restrict__ entries,
                                                           mmp_cache_entry *__restrict__ out, int32_t *__restrict__ out_row, int32_t max_out)
{
    __shared__ int32_t s_rank[kJanTile];
    const int32_t nc = ps->n_removed;
    const int i0 = blockIdx.x * kJanTile;
    if (i0 >= nc) return;  // (uniform)
    const int lane = lane_id(), w = threadIdx.x >> 6;
    if (w == 0) s_rank[lane] = 0;
    __syncthreads();
    const int i = i0 + lane;
    const int64_t mine = i < nc ? cand_time[i] : 0;
    const int nt = (nc + kJanTile - 1) / kJanTile;
    int32_t rank = 0;
    int t = w;
    int j = t * kJanTile + lane;
    int64_t v = (t < nt && j < nc) ? cand_time[j] : 0;
    bool ok = t < nt && j < nc && !dropped[j];
    for (; t < nt; t += 4) {
        const int tn = t + 4, jn = tn * kJanTile + lane;
        const int64_t vn = (tn < nt && jn < nc) ? cand_time[jn] : 0;  // the next tile, ahead
        const bool okn = tn < nt && jn < nc && !dropped[jn];
        const uint64_t kept = __ballot(ok);
#pragma unroll
        for (int k = 0; k < kJanTile; k++) rank += (((kept >> k) & 1ull) && wave_bcast_i64(v, k) < mine) ? 1 : 0;
        v = vn;
        ok = okn;
    }
    if (rank) atomicAdd(&s_rank[lane], rank);
    __syncthreads();
    if (w != 0) return;
    rank = s_rank[lane];
    if (i >= nc || dropped[i] || rank >= max_out) return;
    const int32_t row = cand_row[i];
    const mmp_janitor_entry e = entries[row];
    mmp_cache_entry c;
    c.model = e.model;
    c.weight = e.weight;
    c.last_used = mine;
    c.interval_count = e.interval_count;
    c.last_heavy_time = e.last_heavy_time;
    c.last_unload_time = e.last_unload_time;
    c.earlier_use_iteration = e.earlier_use_iteration;
    c.last_used_iteration = e.last_used_iteration;
    c.flags = 0;  // (a candidate's entry is not failed, :6039)
    c.reserved = 0;
    out[rank] = c;
    out_row[rank] = row;
}

// the row's action byte, the totals per action, and the map word back to -1
__global__ void janitor_finish_kernel(const mmp_janitor_entry *__restrict__ entries, int32_t n, const mmp_model_row *__restrict__ models,
                                      const int32_t *__restrict__ ent_pod, const int64_t *__restrict__ ent_time, int32_t *__restrict__ map,
                                      mmp_janitor_params p, uint8_t *__restrict__ actions, JanitorScalars *js)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    uint8_t a = 0xff;
    if (r < n) {
        const int32_t inv = js->stop_inv;
        const bool stopped = inv > 0;
        const int32_t stop = stopped ? n - inv : INT32_MAX;
        const mmp_janitor_entry e = entries[r];
        if (e.model < 0)
            a = janitor_eval_unregistered(e, r, stop, p);
        else {
            const mmp_model_row m = models[e.model];
            const JanSelf s = janitor_find_self(m, ent_pod, ent_time, p.self_pod);  // (.ins is not needed for the action)
            a = janitor_eval(m, s, entries, r, stop, stopped, p).action;
            map[e.model] = -1;
        }
        actions[r] = a;
    }
#pragma unroll
    for (int k = 0; k < 7; k++) {
        const int c = __popcll(__ballot(a == k));
        if (c && lane_id() == 0) atomicAdd(&js->n_action[k], c);
    }
}

// apply: edit x's record, rebuilt at arena[base + keep_off[x] ...): instanceIds without / with self_pod's entry (replaced where
// it stood, or inserted at inserted_pos), then loadFailedInstanceIds; its row for upsert_models_kernel.  `base + n_kept` lies
// inside the arena (the host grew it), and nothing refers to that part yet.
__global__ void janitor_build_kernel(const mmp_janitor_edit *__restrict__ edits, const int32_t *__restrict__ keep_off, int32_t n_edits,
                                     const mmp_model_row *__restrict__ models, int32_t *__restrict__ ent_pod, int64_t *__restrict__ ent_time,
                                     int32_t base, int32_t arena_end, int32_t self_pod, int32_t *__restrict__ u_idx,
                                     mmp_model_row *__restrict__ u_rows)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_edits) return;
    const mmp_janitor_edit ed = edits[x];
    const mmp_model_row m = models[ed.model];
    int32_t dst = base + keep_off[x];
    auto put = [&](int32_t pod, int64_t t) {
        if (dst < arena_end) {
            ent_pod[dst] = pod;
            ent_time[dst] = t;
        }
        dst++;
    };
    const bool drop_loaded = ed.flags & MMP_JANITOR_EDIT_REM_LOADED;
    const bool drop_failed = ed.flags & (MMP_JANITOR_EDIT_REM_FAILED | MMP_JANITOR_EDIT_REGISTERED);
    for (int32_t k = 0; k < m.n_loaded; k++) {
        const int32_t pod = ent_pod[m.ent_off + k];
        const int64_t t = ent_time[m.ent_off + k];
        if (pod == self_pod) {
            if (!drop_loaded) put(pod, k == ed.inserted_pos ? ed.inserted_time : t);
            continue;
        }
        if (k == ed.inserted_pos) put(self_pod, ed.inserted_time);
        put(pod, t);
    }
    if (ed.inserted_pos == m.n_loaded) put(self_pod, ed.inserted_time);
    for (int32_t k = m.n_loaded; k < m.n_loaded + m.n_failed; k++) {
        const int32_t pod = ent_pod[m.ent_off + k];
        if (pod == self_pod && drop_failed) continue;
        put(pod, ent_time[m.ent_off + k]);
    }
    u_idx[x] = ed.model;
    u_rows[x] = mmp_model_row{m.type, base + keep_off[x], ed.n_loaded_after, ed.n_failed_after, ed.last_used_after};
}

}  // namespace mmp
