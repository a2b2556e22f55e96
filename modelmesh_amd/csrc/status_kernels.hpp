// status_kernels.hpp — getStatus answered from the resident registry, a batch of questions at a time (mmp_models_status): the
// status class of invokeModel's "getStatus case" (MM.java:3760-3768) and the copy list of makeStatusInfo (:3013-3058) — the
// failure overlay of :3017-3026, instanceIds as NOT_CHECKED then loadFailedInstanceIds as LOADING_FAILED (:3029-3041), sorted
// by Long.compare(o.time, time) (:3057): stable, signed time descending.
//
// Almost every record holds 0 to 3 entries, so nothing here gives a request a wavefront of its own:
//
//   status_count_kernel  one lane per request: the overlay decided from the record's own entries (where the put entry goes in
//                        loadFailedInstanceIds, which loaded entry leaves), the class, the two counts; per-workgroup (rows
//                        longer than a wavefront, -, copies) for the scan, and the 64-bit total of the copies
//   prune_scan_kernel    (registry_kernels.hpp) the one-workgroup scan of those triples (protocol: triple_count there)
//   status_rows_kernel   one lane per request: copy_off = the exclusive prefix sum in request order; the requests with more than
//                        kStatusWaveRow copies listed in request order
//   status_emit_kernel   the requests PACKED: one lane per output entry.  A lane finds its request by bisecting the scanned
//                        offsets, gathers its own entry (the overlay applied while gathering) and walks its segment: its place
//                        is the number of entries that are later in time, or equal in time and earlier in the concatenation.
//                        Lanes of a listed long row leave.
//   status_long_kernel   one workgroup per listed row: the times staged in LDS, kStatusTile at a time, every thread ranking one
//                        entry against the tile.  A row beyond the tile is ranked the same way, tile after tile (slow, exact).
//
// Nothing is written to the registry, and no atomic decides a position: every output word has one writer and a place that
// depends on the inputs alone.
#pragma once
#include "registry_ops_kernels.hpp"

namespace mmp {

constexpr int kStatusBlock = kCompactBlock;
constexpr int32_t kStatusWaveRow = 64;  // copies a packed lane still walks on its own; longer rows go to status_long_kernel
constexpr int32_t kStatusTile = 1024;   // times of one row in LDS at once (8 KB)
constexpr int kStatusLongBlock = 256;

// what the emit kernels need of a request beside its row: which loaded entry the overlay took out and where in
// loadFailedInstanceIds it put its own (-1: neither)
struct StatusAux {
    int32_t rm_loaded, ins_failed;
};

struct StatusScalars {
    unsigned long long n_copies;  // the 64-bit total: the int32 offsets are only used when it fits
};

__device__ __forceinline__ mmp_model_row status_record(const mmp_status_req &q, const mmp_model_row *__restrict__ models)
{
    return q.model >= 0 ? models[q.model] : mmp_model_row{0, 0, 0, 0, 0};  // mr == null: both lists empty (:3259)
}

// (the host checked model, fail_pod, flags and reserved of every request before anything was launched)
__device__ __forceinline__ mmp_status_row status_eval(const mmp_status_req &q, const mmp_model_row &m, const int32_t *__restrict__ ent_pod,
                                                      const mmp_pod_row *__restrict__ pods, int32_t P, StatusAux &a)
{
    a = StatusAux{-1, -1};
    int32_t nl = m.n_loaded, nf = m.n_failed;
    if (q.fail_pod >= 0) {
        int32_t li = -1, fi = -1;
        for (int32_t k = 0; k < nl + nf; k++) {
            if (ent_pod[m.ent_off + k] != q.fail_pod) continue;
            if (k < nl)
                li = k;
            else
                fi = k - nl;
        }
        if (fi < 0) {  // :3018 !failedInstances.containsKey(instanceId)
            const mmp_model_row f{m.type, m.ent_off + m.n_loaded, m.n_failed, 0, 0};
            a.ins_failed = janitor_insert_pos(f, ent_pod, pods, P, q.fail_pod);  // :3020 TreeMap.put of a new key
            nf++;
            if (li >= 0) {  // :3023 loadedInstances.remove(instanceId)
                a.rm_loaded = li;
                nl--;
            }
        }
    }
    int32_t cls;
    if (q.model < 0)
        cls = MMP_MST_NOT_FOUND;
    else if (nl > 0 && !(q.flags & MMP_MSTF_MISS))
        cls = MMP_MST_ASK;
    else if (q.fail_pod >= 0 || nf > 0)
        cls = MMP_MST_LOADING_FAILED;
    else
        cls = MMP_MST_NOT_LOADED;
    return mmp_status_row{cls, 0, nl, nf};
}

// entry k of the concatenation (instanceIds, then loadFailedInstanceIds) after the overlay: its time, and where it is stored
// (-1: the overlay's own entry, which is stored nowhere)
__device__ __forceinline__ int32_t status_src(const mmp_model_row &m, const mmp_status_row &r, const StatusAux &a, int32_t k)
{
    if (k < r.n_not_checked) return m.ent_off + k + (a.rm_loaded >= 0 && k >= a.rm_loaded ? 1 : 0);
    const int32_t f = k - r.n_not_checked;
    if (a.ins_failed >= 0) {
        if (f == a.ins_failed) return -1;
        return m.ent_off + m.n_loaded + f - (f > a.ins_failed ? 1 : 0);
    }
    return m.ent_off + m.n_loaded + f;
}

__global__ __launch_bounds__(kStatusBlock) void status_count_kernel(const mmp_status_req *__restrict__ reqs, int32_t n,
                                                                    const mmp_model_row *__restrict__ models,
                                                                    const int32_t *__restrict__ ent_pod, const mmp_pod_row *__restrict__ pods,
                                                                    int32_t P, mmp_status_row *__restrict__ rows, StatusAux *__restrict__ aux,
                                                                    int32_t *__restrict__ block_counts, StatusScalars *ss)
{
    const int i = blockIdx.x * kStatusBlock + threadIdx.x;
    int64_t cnt = 0;
    if (i < n) {
        const mmp_status_req q = reqs[i];
        StatusAux a;
        const mmp_status_row r = status_eval(q, status_record(q, models), ent_pod, pods, P, a);
        rows[i] = r;
        aux[i] = a;
        cnt = (int64_t)r.n_not_checked + r.n_failed;
    }
    const int64_t wsum = wave_sum_i64(cnt);
    if (lane_id() == 0 && wsum) atomicAdd(&ss->n_copies, (unsigned long long)wsum);  // (an integer sum: the same in any order)
    triple_count<kCol1None>(cnt > kStatusWaveRow, 0, (int32_t)cnt, block_counts);
}

__global__ __launch_bounds__(kStatusBlock) void status_rows_kernel(int32_t n, mmp_status_row *__restrict__ rows,
                                                                   const int32_t *__restrict__ block_off, int32_t *__restrict__ long_list)
{
    const int i = blockIdx.x * kStatusBlock + threadIdx.x;
    int32_t cnt = 0;
    if (i < n) cnt = rows[i].n_not_checked + rows[i].n_failed;
    const bool is_long = cnt > kStatusWaveRow;
    const TripleOff o = triple_offsets<kCol1None>(is_long, 0, cnt, block_off);
    if (i < n) {
        rows[i].copy_off = o.k;
        if (is_long) long_list[o.e] = i;
    }
}

// the copy at concatenation index k of request i
__device__ __forceinline__ mmp_status_copy status_copy_of(const mmp_status_req &q, const mmp_status_row &r, int32_t src, int32_t k,
                                                          const int32_t *__restrict__ ent_pod, const int64_t *__restrict__ ent_time,
                                                          int64_t now)
{
    const int32_t st = k < r.n_not_checked ? MMP_COPY_NOT_CHECKED : MMP_COPY_LOADING_FAILED;
    return src < 0 ? mmp_status_copy{q.fail_pod, st, now} : mmp_status_copy{ent_pod[src], st, ent_time[src]};
}

__global__ __launch_bounds__(kStatusBlock) void status_emit_kernel(const mmp_status_req *__restrict__ reqs, int32_t n, int32_t total,
                                                                   const mmp_model_row *__restrict__ models,
                                                                   const int32_t *__restrict__ ent_pod, const int64_t *__restrict__ ent_time,
                                                                   int64_t now, const mmp_status_row *__restrict__ rows,
                                                                   const StatusAux *__restrict__ aux, mmp_status_copy *__restrict__ copies,
                                                                   int32_t max_copies)
{
    const int g = blockIdx.x * kStatusBlock + threadIdx.x;
    if (g >= total) return;
    // the last request whose offset is <= g: the requests behind it with the same offset are empty
    int32_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo + 1) / 2;
        if (rows[mid].copy_off <= g)
            lo = mid;
        else
            hi = mid - 1;
    }
    const mmp_status_row r = rows[lo];
    const int32_t L = r.n_not_checked + r.n_failed;
    if (L > kStatusWaveRow) return;  // status_long_kernel's
    const mmp_status_req q = reqs[lo];
    const StatusAux a = aux[lo];
    const mmp_model_row m = status_record(q, models);
    const int32_t k = g - r.copy_off;
    const mmp_status_copy mine = status_copy_of(q, r, status_src(m, r, a, k), k, ent_pod, ent_time, now);
    int32_t rank = 0;
    for (int32_t j = 0; j < L; j++) {
        const int32_t s = status_src(m, r, a, j);
        const int64_t t = s < 0 ? now : ent_time[s];
        rank += (t > mine.time || (t == mine.time && j < k)) ? 1 : 0;
    }
    const int32_t dst = r.copy_off + rank;  // rank < L: inside the segment
    if (dst < max_copies) copies[dst] = mine;
}

__global__ __launch_bounds__(kStatusLongBlock) void status_long_kernel(const mmp_status_req *__restrict__ reqs,
                                                                       const int32_t *__restrict__ long_list,
                                                                       const mmp_model_row *__restrict__ models,
                                                                       const int32_t *__restrict__ ent_pod, const int64_t *__restrict__ ent_time,
                                                                       int64_t now, const mmp_status_row *__restrict__ rows,
                                                                       const StatusAux *__restrict__ aux, mmp_status_copy *__restrict__ copies,
                                                                       int32_t max_copies)
{
    __shared__ int64_t s_time[kStatusTile];
    const int32_t i = long_list[blockIdx.x];
    const mmp_status_req q = reqs[i];
    const mmp_status_row r = rows[i];
    const StatusAux a = aux[i];
    const mmp_model_row m = status_record(q, models);
    const int32_t L = r.n_not_checked + r.n_failed;
    const bool one_tile = L <= kStatusTile;  // (uniform over the workgroup, as L is: the barriers below are reached by all or none)
    for (int32_t kb = 0; kb < L; kb += kStatusLongBlock) {
        const int32_t k = kb + (int32_t)threadIdx.x;
        mmp_status_copy mine{};
        if (k < L) mine = status_copy_of(q, r, status_src(m, r, a, k), k, ent_pod, ent_time, now);
        int32_t rank = 0;
        for (int32_t jb = 0; jb < L; jb += kStatusTile) {
            const int32_t nt = min(kStatusTile, L - jb);
            if (!one_tile || kb == 0) {  // a row inside the tile is staged once
                __syncthreads();
                for (int32_t x = threadIdx.x; x < nt; x += kStatusLongBlock) {
                    const int32_t s = status_src(m, r, a, jb + x);
                    s_time[x] = s < 0 ? now : ent_time[s];
                }
                __syncthreads();
            }
            if (k < L)
                for (int32_t x = 0; x < nt; x++) {
                    const int64_t t = s_time[x];
                    rank += (t > mine.time || (t == mine.time && jb + x < k)) ? 1 : 0;
                }
        }
        if (k < L) {
            const int32_t dst = r.copy_off + rank;
            if (dst < max_copies) copies[dst] = mine;
        }
    }
}

}  // namespace mmp
