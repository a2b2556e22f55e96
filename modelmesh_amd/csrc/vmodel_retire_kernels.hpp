// vmodel_retire_kernels.hpp — vmodel rows leave the index space (mmp_vmodels_retire): the rows, the string arena, the vmodel-id arena
// and the vmodel-id table are compacted on the device, beside the published ones; the host swaps them in once the new table has
// verified.  The launch sequence is that of retire_kernels.hpp, the fields are VmRow's.
//
// The survivors keep their relative order: a survivor's new row is its old row minus the retired rows below it, its strings and
// its id bytes stand where the survivors in front of it end.  All three positions are ONE exclusive scan over per-row counts.
//
//   vm_retire_mark_kernel    one lane per element of the caller's list: keep[row] = 0 (keep[] was filled with 1; a row named twice
//                            is cleared twice).  With `absent_only` the lane also reads the row's flags and atomicMin's the row into
//                            one word when it is not ABSENT — the lowest such row, whichever lanes raced
//   vm_retire_absent_kernel  instead of the list (MMP_VMRETIRE_ALL_ABSENT): one lane per row, keep[row] = the row is not ABSENT
//   vm_retire_count_kernel   one lane per row: (kept, id bytes if kept, string bytes if kept — the three len[], a null holds 0 —,
//                            kept and not ABSENT); counts[V] = the zero element, so that the scan's last element is the totals
//   rocprim::exclusive_scan over those: new row, new id-arena offset, new string-arena offset; the fourth column positions
//                            nothing, its total is the survivors that are not ABSENT (a list may name rows that are set)
//   vm_retire_move_kernel    one lane per row: a survivor's strings in the order amid, tmid, o into the new arena, its VmRow with
//                            the new off[] (hash[], len[] and flags as stored: no string is hashed again), its id bytes and its end
//                            offset into the new id arena, remap[old] = new; a retired row writes remap[old] = -1 and nothing else
//   retire_table_kernel / retire_verify_kernel (retire_kernels.hpp), as they are, on the vid_* table
//
// A word written non-atomically in one launch is read only in later launches (model_ids_kernels.hpp).  Which slot a colliding id
// gets in the next table depends on the race of the claims; no output does: rows, arenas and remap are functions of the scan, and
// the two atomicMin words are minima.  Two runs are byte-identical.
//
// Ids and strings are tens of bytes: a long one is a loop of its lane, as in retire_move_kernel.
#pragma once
#include "vmodel_kernels.hpp"

namespace mmp {

// per row, and after the exclusive scan per row position: surviving rows, id bytes, string bytes and surviving rows that are not
// ABSENT in front of it
struct VmRetireCount {
    int32_t row, bytes, strs, live;
};
struct VmRetirePlus {
    __host__ __device__ VmRetireCount operator()(const VmRetireCount &a, const VmRetireCount &b) const
    {
        return VmRetireCount{a.row + b.row, a.bytes + b.bytes, a.strs + b.strs, a.live + b.live};
    }
};

// rows[i] in [0, V): the host has checked the range
__global__ __launch_bounds__(kRetireBlock) void vm_retire_mark_kernel(const int32_t *__restrict__ rows, int32_t n,
                                                                      const VmRow *__restrict__ vrows, int32_t absent_only,
                                                                      int32_t *__restrict__ keep, int32_t *__restrict__ not_absent)
{
    const int i = blockIdx.x * kRetireBlock + threadIdx.x;
    if (i >= n) return;
    const int32_t r = rows[i];
    keep[r] = 0;
    if (absent_only && !(vrows[r].flags & kVmfAbsent)) atomicMin(not_absent, r);
}

__global__ __launch_bounds__(kRetireBlock) void vm_retire_absent_kernel(int32_t V, const VmRow *__restrict__ vrows,
                                                                        int32_t *__restrict__ keep)
{
    const int i = blockIdx.x * kRetireBlock + threadIdx.x;
    if (i >= V) return;
    keep[i] = (vrows[i].flags & kVmfAbsent) ? 0 : 1;
}

__global__ __launch_bounds__(kRetireBlock) void vm_retire_count_kernel(int32_t V, const int32_t *__restrict__ keep,
                                                                       const VmRow *__restrict__ vrows,
                                                                       const int32_t *__restrict__ vid_off,
                                                                       VmRetireCount *__restrict__ counts)
{
    const int i = blockIdx.x * kRetireBlock + threadIdx.x;
    if (i > V) return;
    VmRetireCount f{0, 0, 0, 0};
    if (i < V && keep[i]) {
        const VmRow r = vrows[i];
        f.row = 1;
        f.bytes = vid_off[i + 1] - vid_off[i];
        f.strs = r.len[0] + r.len[1] + r.len[2];
        f.live = (r.flags & kVmfAbsent) ? 0 : 1;
    }
    counts[i] = f;
}

// the old rows, string arena and id arena, and the new ones beside them (new_off[0] = 0 is the host's to write)
struct VmRetireMove {
    const VmRow *rows;
    const char *arena;
    const char *vid_bytes;
    const int32_t *vid_off;
    VmRow *new_rows;
    char *new_arena;
    char *new_bytes;
    int32_t *new_off;
};

__global__ __launch_bounds__(kRetireBlock) void vm_retire_move_kernel(int32_t V, const int32_t *__restrict__ keep,
                                                                      const VmRetireCount *__restrict__ pos, VmRetireMove A,
                                                                      int32_t *__restrict__ remap)
{
    const int i = blockIdx.x * kRetireBlock + threadIdx.x;
    if (i >= V) return;
    if (!keep[i]) {
        remap[i] = -1;
        return;
    }
    const int32_t row = pos[i].row, bytes = pos[i].bytes;
    int32_t o = pos[i].strs;
    // hash[], len[] and flags go as they are; the three offsets are written behind the copy
    const VmRow *src = A.rows + i;
    VmRow *dst = A.new_rows + row;
    const int32_t off[3] = {src->off[0], src->off[1], src->off[2]}, len[3] = {src->len[0], src->len[1], src->len[2]};
    *dst = *src;
#pragma unroll
    for (int s = 0; s < 3; s++) {  // (the offsets of vm_squeeze_copy_kernel: a string without bytes stands at 0)
        for (int32_t q = 0; q < len[s]; q++) A.new_arena[o + q] = A.arena[off[s] + q];
        dst->off[s] = len[s] ? o : 0;
        o += len[s];
    }
    const int32_t b = A.vid_off[i], blen = A.vid_off[i + 1] - b;
    for (int32_t j = 0; j < blen; j++) A.new_bytes[bytes + j] = A.vid_bytes[b + j];
    A.new_off[row + 1] = bytes + blen;
    remap[i] = row;
}

}  // namespace mmp
