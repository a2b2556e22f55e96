// seam_caller_kernels.hpp — the single-caller forms of the route and miss seams (include/mmplace.h: mmp_route_batch_c,
// mmp_miss_batch_c) on their compact rows: 48-byte mmp_gate_req_c and 24-byte mmp_serve_req_c, the calling instance's side
// (mmp_seam_caller) once per call.
//
// No rule is stated here.  A lane assembles the mmp_gate_req / mmp_serve_req the header's rule defines in registers and calls
// gate_eval / serve_eval (gate_kernel.hpp, aux_kernels.hpp): the answers are those of route_batch_kernel / gate_batch_kernel on the
// expanded rows by construction.
//
// What differs is how the rows reach the lanes.  The full-row kernels read 144-byte and 48-byte AoS rows lane-per-row: every
// load instruction of a wavefront touches 64 different rows, and the kernels are bandwidth-bound on the traffic that wastes.  Here
// the caller rides in the kernel arguments — wave-uniform, so the churn guard and most of the publish rule are scalar work — and
// each wavefront stages ITS OWN 64 rows into LDS by contiguous loads, 16 bytes per lane (3 072 bytes of gate rows = 3 loads per
// lane, 1 536 bytes of serve rows = 1 load per lane and a second by lanes 0-31), then every lane reads its own row back.  No
// workgroup barrier: a wavefront reads only what it wrote itself (the per-wavefront pattern place_memo_body uses for its records),
// so wave_sync() is all that is needed.  LDS banking (ds_read_b128 / ds_read_b64 are served in groups of 16 / 32 lanes over 64
// banks): a 48-byte stride puts lane L's quad at dword 12·L, and 12·L mod 64 takes 16 different multiples of 4 over any 16 lanes
// with different L mod 16 — every hardware lane group is such a set; a 24-byte stride puts lane L's pair at dword 6·L, 32
// different even banks over 32 consecutive lanes.  Both reads are conflict-free.
#pragma once
#include "gate_kernel.hpp"

namespace mmp {

struct SeamCArgs {
    const mmp_gate_req_c *greqs;   // [n], 16-byte aligned (a staging buffer's start)
    const mmp_serve_req_c *sreqs;  // [n], 16-byte aligned; unused by gate_batch_c_kernel
    int32_t n;
    mmp_seam_caller caller;
};

constexpr int kSeamCBlock = 256;  // four wavefronts, each with a tile of its own
constexpr int kSeamCWaves = kSeamCBlock / 64;
constexpr int kSeamCGateTile = 64 * (int)sizeof(mmp_gate_req_c);    // 3 072
constexpr int kSeamCServeTile = 64 * (int)sizeof(mmp_serve_req_c);  // 1 536
static_assert(sizeof(mmp_seam_caller) == 112 && sizeof(mmp_gate_req_c) == 48 && sizeof(mmp_serve_req_c) == 24, "compact row layout");
static_assert(kSeamCGateTile % 1024 == 0 && kSeamCServeTile == 1024 + 512, "one 16-byte load per lane moves 1 024 bytes");

// Rows [w0, w0 + cnt) of `src` (ROW bytes each; cnt <= 64) into the wavefront's tile.  A wavefront's rows start at a multiple of
// 64 rows, so at a multiple of 16 bytes.  The LAST wavefront must not read past the end of the array: a 16-byte piece is loaded
// only if it ends inside the cnt rows; where cnt · ROW is not a multiple of 16 (24-byte rows, cnt odd) the last 8 bytes are loaded
// as 8 — the staging allocation needs no rounding.  Tile bytes beyond the rows are left as they are: no lane reads them.
template <int ROW>
__device__ __forceinline__ void stage_rows(const void *src, int w0, int cnt, unsigned char *tile)
{
    static_assert(ROW % 8 == 0, "rows are multiples of 8 bytes");
    const int lane = lane_id();
    const int bytes = cnt * ROW;
    const unsigned char *g = static_cast<const unsigned char *>(src) + (size_t)w0 * ROW;
    constexpr int kPieces = (64 * ROW + 1023) / 1024;
    uint4 v[kPieces];
#pragma unroll
    for (int k = 0; k < kPieces; k++) {  // every load of the wavefront in flight before the first LDS write
        const int off = (k * 64 + lane) * 16;
        v[k] = uint4{0u, 0u, 0u, 0u};
        if (off + 16 <= bytes) {
            v[k] = *reinterpret_cast<const uint4 *>(g + off);
        } else if (off + 8 <= bytes) {
            const uint2 h = *reinterpret_cast<const uint2 *>(g + off);
            v[k].x = h.x;
            v[k].y = h.y;
        }
    }
#pragma unroll
    for (int k = 0; k < kPieces; k++) {
        const int off = (k * 64 + lane) * 16;
        if (off < 64 * ROW && off < bytes) *reinterpret_cast<uint4 *>(tile + off) = v[k];
    }
}

// the header's rule, gate row (host: the calls within the slot sizes write their rows out with it)
__host__ __device__ __forceinline__ mmp_gate_req expand_gate(const mmp_seam_caller &c, const mmp_gate_req_c &g)
{
    mmp_gate_req r;
    r.model = g.model;
    r.self_pod = c.self_pod;
    r.flags = c.gate_flags | g.flags;
    r.excl_off = g.excl_off;
    r.n_excl = g.n_excl;
    r.explicit_off = g.explicit_off;
    r.n_explicit = g.n_explicit;
    r.size_hint = g.size_hint;
    r.last_used_time = g.last_used_time;
    r.cache_capacity = c.cache_capacity;
    r.cache_weighted_size = c.cache_weighted_size;
    r.cache_oldest_time = c.cache_oldest_time;
    r.loader_predicted = g.loader_predicted;
    r.loading_count = c.loading_count;
    r.weight_predict_cutoff = c.weight_predict_cutoff;
    r.reserved = 0;
    r.loaded_time = g.loaded_time;
    r.load_timeout_ms = c.load_timeout_ms;
    r.fresh_lru = c.fresh_lru;
    r.fresh_capacity = c.fresh_capacity;
    r.fresh_used = c.fresh_used;
    r.fresh_count = c.fresh_count;
    r.fresh_loading_threads = c.fresh_loading_threads;
    r.fresh_in_progress = c.fresh_in_progress;
    r.fresh_rpm = c.fresh_rpm;
    r.last_published = c.last_published;
    return r;
}
// the header's rule, serve row: the exclusion range is the GATE row's
__host__ __device__ __forceinline__ mmp_serve_req expand_serve(const mmp_seam_caller &c, const mmp_gate_req_c &g, const mmp_serve_req_c &s)
{
    mmp_serve_req r;
    r.model = g.model;
    r.self_pod = c.self_pod;
    r.flags = s.flags;
    r.local_in_flight = c.local_in_flight;
    r.last_invoke_time = c.last_invoke_time;
    r.assume_completed_ms = s.assume_completed_ms;
    r.excl_off = g.excl_off;
    r.n_excl = g.n_excl;
    r.cnt_off = s.cnt_off;
    r.n_cnt = s.n_cnt;
    return r;
}

// a lane's own row out of its wavefront's tile: three 16-byte reads / three 8-byte reads
__device__ __forceinline__ mmp_gate_req_c tile_gate_row(const unsigned char *tile, int lane)
{
    const uint4 *p = reinterpret_cast<const uint4 *>(tile + lane * (int)sizeof(mmp_gate_req_c));
    const uint4 q[3] = {p[0], p[1], p[2]};
    mmp_gate_req_c g;
    __builtin_memcpy(&g, q, sizeof(g));
    return g;
}
__device__ __forceinline__ mmp_serve_req_c tile_serve_row(const unsigned char *tile, int lane)
{
    const uint2 *p = reinterpret_cast<const uint2 *>(tile + lane * (int)sizeof(mmp_serve_req_c));
    const uint2 q[3] = {p[0], p[1], p[2]};
    mmp_serve_req_c s;
    __builtin_memcpy(&s, q, sizeof(s));
    return s;
}

// the guards of a large mmp_miss_batch_c: gate_batch_kernel's answers on the expanded rows
__global__ __launch_bounds__(kSeamCBlock) void gate_batch_c_kernel(GateArgs A, SeamCArgs R)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_gate[kSeamCWaves][kSeamCGateTile];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int w0 = blockIdx.x * kSeamCBlock + wave * 64;  // (wave-uniform)
    const int cnt = R.n - w0 < 64 ? R.n - w0 : 64;        // <= 0: a wavefront past the end
    if (cnt > 0) {
        stage_rows<(int)sizeof(mmp_gate_req_c)>(R.greqs, w0, cnt, s_gate[wave]);
        wave_sync();
        if (lane < cnt) {
            const mmp_gate_req r = expand_gate(R.caller, tile_gate_row(s_gate[wave], lane));
            A.outs[w0 + lane] = gate_eval(A, r);
        }
    }
    announce_done(A.done);
}

// mmp_route_batch_c: route_batch_kernel's answers on the expanded rows
__global__ __launch_bounds__(kSeamCBlock) void route_batch_c_kernel(GateArgs G, ServeArgs S, SeamCArgs R)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_gate[kSeamCWaves][kSeamCGateTile];
    __shared__ __attribute__((aligned(16))) unsigned char s_serve[kSeamCWaves][kSeamCServeTile];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int w0 = blockIdx.x * kSeamCBlock + wave * 64;
    const int cnt = R.n - w0 < 64 ? R.n - w0 : 64;
    if (cnt > 0) {
        stage_rows<(int)sizeof(mmp_gate_req_c)>(R.greqs, w0, cnt, s_gate[wave]);
        stage_rows<(int)sizeof(mmp_serve_req_c)>(R.sreqs, w0, cnt, s_serve[wave]);
        wave_sync();
        if (lane < cnt) {
            const mmp_gate_req_c g = tile_gate_row(s_gate[wave], lane);
            const mmp_serve_req_c s = tile_serve_row(s_serve[wave], lane);
            const mmp_serve_req sr = expand_serve(R.caller, g, s);
            const mmp_gate_req gr = expand_gate(R.caller, g);
            const mmp_serve_out so = serve_eval(S, sr);
            const mmp_gate_out go = gate_eval(G, gr);
            S.outs[w0 + lane] = so;
            G.outs[w0 + lane] = go;
        }
    }
    announce_done(G.done);
}

}  // namespace mmp
