// retire_kernels.hpp — registry rows leave the index space (mmp_models_retire): the registry, its entry arena, the id arena and the
// model-id table are compacted on the device, beside the published ones; the host swaps them in once the new table has verified.
//
// The survivors keep their relative order: a survivor's new row is its old row minus the retired rows below it, its entries and
// its id bytes stand where the survivors in front of it end.  All three positions are ONE exclusive scan over per-row triples.
//
//   retire_mark_kernel     one lane per element of the caller's list: keep[row] = 0 (keep[] was filled with 1; a row named twice
//                          is cleared twice).  With `empty_only` the lane also reads the row and atomicMin's it into one word when
//                          it is not the empty row — the lowest such row, whichever lanes raced
//   retire_flags_kernel    one lane per row: (kept, id bytes if kept, entries if kept); counts[M] = the zero triple, so that the
//                          scan's last element is the three totals
//   rocprim::exclusive_scan over those triples: new row, new id-arena offset, new ent_off
//   retire_move_kernel     one lane per row: a survivor's row with its new ent_off, its entries, its id bytes and its end offset
//                          into the new arrays, remap[old] = new; a retired row writes remap[old] = -1 and nothing else
//   retire_table_kernel    one lane per slot of the OLD table: a slot whose row survives claims the first empty slot of its probe
//                          sequence in the (emptied) next table with its STORED hash and its new row (tab_claim) — no id string is
//                          hashed again, so a masked hash (MMP_MODEL_ID_HASH_BITS) stays masked
//   retire_verify_kernel   a launch of its own, one lane per slot of the old table: the lookup of a surviving id in the next table,
//                          byte-verified against the NEW arena, must answer its new row; the lowest new row that does not is
//                          atomicMin'ed into one word
//
// A word written non-atomically in one launch is read only in later launches (model_ids_kernels.hpp).  Which slot a colliding id
// gets in the next table depends on the race of the claims; no output does: rows, arenas and remap are functions of the scan, and
// the two atomicMin words are minima.  Two runs are byte-identical.
//
// Almost every record holds 0 to 3 entries and an id tens of bytes: a long record is a loop of its lane.
#pragma once
#include "model_ids_kernels.hpp"

namespace mmp {

constexpr int kRetireBlock = kIdTabBlock;

// per row, and after the exclusive scan per row position: surviving rows, id bytes and entries in front of it
struct RetireCount {
    int32_t row, bytes, ents;
};
struct RetirePlus {
    __host__ __device__ RetireCount operator()(const RetireCount &a, const RetireCount &b) const
    {
        return RetireCount{a.row + b.row, a.bytes + b.bytes, a.ents + b.ents};
    }
};

// what a deletion leaves (ingest_kernels.hpp: ENTRY_DELETED): every field zero, no entry.  ent_off is a position, not a value.
__device__ __forceinline__ bool retire_row_empty(const mmp_model_row &m)
{
    return m.type == 0 && m.n_loaded == 0 && m.n_failed == 0 && m.last_used == 0;
}

// rows[i] in [0, M): the host has checked the range
__global__ __launch_bounds__(kRetireBlock) void retire_mark_kernel(const int32_t *__restrict__ rows, int32_t n,
                                                                   const mmp_model_row *__restrict__ models, int32_t empty_only,
                                                                   int32_t *__restrict__ keep, int32_t *__restrict__ not_empty)
{
    const int i = blockIdx.x * kRetireBlock + threadIdx.x;
    if (i >= n) return;
    const int32_t r = rows[i];
    keep[r] = 0;
    if (empty_only && !retire_row_empty(models[r])) atomicMin(not_empty, r);
}

// mid_off == nullptr: no id table, the bytes column stays zero
__global__ __launch_bounds__(kRetireBlock) void retire_flags_kernel(int32_t M, const int32_t *__restrict__ keep,
                                                                    const mmp_model_row *__restrict__ models,
                                                                    const int32_t *__restrict__ mid_off, RetireCount *__restrict__ counts)
{
    const int i = blockIdx.x * kRetireBlock + threadIdx.x;
    if (i > M) return;
    RetireCount f{0, 0, 0};
    if (i < M && keep[i]) {
        f.row = 1;
        f.bytes = mid_off ? mid_off[i + 1] - mid_off[i] : 0;
        f.ents = models[i].n_loaded + models[i].n_failed;
    }
    counts[i] = f;
}

// the old registry and id arena, and the new ones beside them (new_off[0] = 0 is the host's to write)
struct RetireMove {
    const mmp_model_row *models;
    const int32_t *ent_pod;
    const int64_t *ent_time;
    const char *mid_bytes;  // nullptr with mid_off: no id table
    const int32_t *mid_off;
    mmp_model_row *new_models;
    int32_t *new_pod;
    int64_t *new_time;
    char *new_bytes;
    int32_t *new_off;
};

__global__ __launch_bounds__(kRetireBlock) void retire_move_kernel(int32_t M, const int32_t *__restrict__ keep,
                                                                   const RetireCount *__restrict__ pos, RetireMove A,
                                                                   int32_t *__restrict__ remap)
{
    const int i = blockIdx.x * kRetireBlock + threadIdx.x;
    if (i >= M) return;
    if (!keep[i]) {
        remap[i] = -1;
        return;
    }
    const RetireCount p = pos[i];
    mmp_model_row m = A.models[i];
    const int32_t k = m.n_loaded + m.n_failed;
    for (int32_t e = 0; e < k; e++) {
        A.new_pod[p.ents + e] = A.ent_pod[m.ent_off + e];
        A.new_time[p.ents + e] = A.ent_time[m.ent_off + e];
    }
    m.ent_off = p.ents;
    A.new_models[p.row] = m;
    if (A.mid_off) {
        const int32_t o = A.mid_off[i], len = A.mid_off[i + 1] - o;
        for (int32_t j = 0; j < len; j++) A.new_bytes[p.bytes + j] = A.mid_bytes[o + j];
        A.new_off[p.row + 1] = p.bytes + len;
    }
    remap[i] = p.row;
}

// nt has at least twice as many slots as rows survive (tab_capacity), so every claim ends at an empty slot
__global__ __launch_bounds__(kRetireBlock) void retire_table_kernel(const uint64_t *__restrict__ old_hash, const int32_t *__restrict__ old_val,
                                                                    uint32_t old_cap, const int32_t *__restrict__ remap, HashTabW nt)
{
    const uint32_t s = blockIdx.x * kRetireBlock + threadIdx.x;
    if (s >= old_cap) return;
    const int32_t v = old_val[s];
    if (v == INT32_MIN) return;
    const int32_t r = remap[v];
    if (r >= 0) tab_claim(nt, old_hash[s], r);
}

// t: the next table over the NEW arena
__global__ __launch_bounds__(kRetireBlock) void retire_verify_kernel(const uint64_t *__restrict__ old_hash, const int32_t *__restrict__ old_val,
                                                                     uint32_t old_cap, const int32_t *__restrict__ remap, ModelIdTab t,
                                                                     int32_t *__restrict__ lost)
{
    const uint32_t s = blockIdx.x * kRetireBlock + threadIdx.x;
    if (s >= old_cap) return;
    const int32_t v = old_val[s];
    if (v == INT32_MIN) return;
    const int32_t r = remap[v];
    if (r < 0) return;
    const int32_t o = t.off[r];
    if (mid_find(t, old_hash[s], t.bytes + o, t.off[r + 1] - o) != r) atomicMin(lost, r);
}

}  // namespace mmp
