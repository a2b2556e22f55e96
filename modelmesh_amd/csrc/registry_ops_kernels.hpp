// registry_ops_kernels.hpp — the edits an instance makes to ModelRecords itself, a batch of them against the resident registry:
// a load completes (loadLocal, MM.java:5204-5207), a load fails (the CacheEntry failure path, :2484-2495), a copy is evicted or
// dropped (deregisterModel, :2948-2958), a scale-down removes the local copy (removeLocalModelCopyAsync, :6347-6365) and the
// cache-hit loop drops its own copy when getFromCache finds nothing (invokeModel, :3682-3687; mmp_registry_ops_k only), with
// ModelRecord.addLoadFailure / removeLoadFailure / updateLastUsed / updateLastUnloadTime (ModelRecord.java:156-179, :239-262).
//
// An op names one record and one instance, and a call names a record at most once, so every op is decided from its own row and
// entries (rops_eval).  The work is O(ops + entries of the records they name): nothing here walks the M rows.  An op whose
// `model` is negative names NO record (registry.get == null, :2481 / :2945 — written by rops_keyed_kernel,
// registry_ops_keyed_kernels.hpp, for an unknown id or the empty row; a host-checked call never carries one): it takes no map
// word, is no edit, gets the status MMP_ROP_NO_RECORD and is counted in n_no_record; nothing is indexed with it.
//
//   rops_count_kernel    one lane per op: its model marked in the janitor's map (M int32 words, all -1 between runs) with a
//                        compare-and-swap — a word already taken is a second op on that model, counted; the op evaluated;
//                        per-workgroup counts of (edits, -, entries the edited records hold afterwards)
//   prune_scan_kernel    (registry_kernels.hpp) the one-workgroup scan of those triples (protocol: triple_count there)
//   rops_scatter_kernel  the same evaluation: edits in OP order by ballot and popcount (no atomics on positions), status bytes,
//                        the totals per op kind, and the map words back to -1 — no M-sized memset per call.  With a duplicate
//                        it only clears the map.
//   rops_build_kernel    (apply) one lane per edit: the record's entries appended to the arena without the removed ones and
//                        with the put one, the row staged for upsert_models_kernel
#pragma once
#include "janitor_kernels.hpp"

namespace mmp {

struct RopsScalars {
    int32_t n_dup;  // ops whose model an earlier-arriving op of the call had taken
    int32_t n_edited[8], n_unchanged[8];  // per MMP_ROP_* kind, kRopKinds used
    int32_t n_added, n_removed;
    int32_t n_no_record;  // ops with model < 0
};

constexpr int kRopKinds = 5;

constexpr int kRopsBlock = kCompactBlock;

// one op's outcome
struct RopEval {
    uint32_t flags;  // MMP_ROP_EDIT_*
    bool edited;     // the Java reaches its compare-and-set
    int32_t nl, nf;  // counts after
    int32_t ins_pos;
    int64_t last_used, last_unload;
};

__device__ __forceinline__ RopEval rops_eval(const mmp_model_row &m, const int32_t *__restrict__ ent_pod, const int64_t *__restrict__ ent_time,
                                             const mmp_pod_row *__restrict__ pods, int32_t P, const mmp_registry_op &op, int64_t now)
{
    RopEval r{};
    r.ins_pos = -1;
    r.nl = m.n_loaded;
    r.nf = m.n_failed;
    r.last_used = m.last_used;
    const JanSelf s = janitor_find_self(m, ent_pod, ent_time, op.pod);
    auto update_last_used = [&](int64_t t) {  // ModelRecord.java:239-246: 0 means now; only raises
        if (t == 0) t = now;
        if (t > r.last_used) {
            r.last_used = t;
            r.flags |= MMP_ROP_EDIT_TOUCHED;
        }
    };
    auto update_last_unload = [&] {  // ModelRecord.java:260-262, after the removal
        r.last_unload = r.nl <= 2 ? 0 : now;
        r.flags |= MMP_ROP_EDIT_UNLOAD_SET;
    };
    if (op.op == MMP_ROP_REGISTER) {
        r.edited = true;  // (the record is always submitted, :5208)
        r.flags |= MMP_ROP_EDIT_PUT_LOADED;  // :5204
        if (s.li >= 0) {
            r.flags |= MMP_ROP_EDIT_REPLACED;
            r.ins_pos = s.li;
        } else {
            r.ins_pos = janitor_insert_pos(m, ent_pod, pods, P, op.pod);
            r.nl++;
        }
        if (s.fi >= 0) {  // :5206
            r.flags |= MMP_ROP_EDIT_REM_FAILED;
            r.nf--;
        }
        update_last_used(op.last_used == 0 ? now : op.last_used);  // :5207
    } else if (op.op == MMP_ROP_LOAD_FAILED) {
        int64_t lu = op.last_used;
        if (lu <= 0) lu = m.last_used;                          // :2484-2486
        if (s.li >= 0 && s.lt == op.load_time) {                // :2487-2488
            r.edited = true;
            r.flags |= MMP_ROP_EDIT_REM_LOADED;
            r.nl--;
            if (!(op.flags & MMP_ROPF_SHUTTING_DOWN)) {         // :2492-2493, ModelRecord.java:157
                r.flags |= MMP_ROP_EDIT_PUT_FAILED;
                if (s.fi >= 0) {
                    r.flags |= MMP_ROP_EDIT_REPLACED;
                    r.ins_pos = s.fi;
                } else {
                    // TreeMap.put into loadFailedInstanceIds: the same rule over the failed list
                    const mmp_model_row f{m.type, m.ent_off + m.n_loaded, m.n_failed, 0, 0};
                    r.ins_pos = janitor_insert_pos(f, ent_pod, pods, P, op.pod);
                    r.nf++;
                }
            }
            update_last_used(lu);                               // :2495
        }
    } else if (op.op == MMP_ROP_DEREGISTER) {
        const bool match = op.flags & MMP_ROPF_MATCH_TIME;      // loadTime != null
        const bool was = s.li >= 0 && (!match || s.lt == op.load_time);                // :2951-2952
        const bool fwas = s.fi >= 0 && (!match || s.ft == op.load_complete_time);      // :2953-2954
        if (was || fwas) {                                      // :2955
            r.edited = true;
            if (was) {
                r.flags |= MMP_ROP_EDIT_REM_LOADED;
                r.nl--;
            }
            if (fwas) {
                r.flags |= MMP_ROP_EDIT_REM_FAILED;
                r.nf--;
            }
            update_last_used(op.last_used);                     // :2956
            if (was) update_last_unload();                      // :2957
        }
    } else if (op.op == MMP_ROP_SCALE_DOWN) {
        if (s.li >= 0 && s.lt == op.load_time) {                // :6347-6348
            r.edited = true;
            r.flags |= MMP_ROP_EDIT_REM_LOADED;                 // :6363
            r.nl--;
            update_last_unload();                               // :6364
            update_last_used(op.last_used);                     // :6365
        }
    } else {  // MMP_ROP_DROP_LOCAL
        r.edited = true;  // (the record is always submitted, :3687)
        if (s.li >= 0) {                                        // :3685 instanceIds.remove(pod), whatever its time
            r.flags |= MMP_ROP_EDIT_REM_LOADED;
            r.nl--;
        }
        update_last_used(op.last_used);                         // :3686; no updateLastUnloadTime on this path
    }
    return r;
}

// (the host checked pod, op and flags of every op before anything was launched, and model < M; model < 0: no record)
__global__ __launch_bounds__(kRopsBlock) void rops_count_kernel(const mmp_registry_op *__restrict__ ops, int32_t n,
                                                                const mmp_model_row *__restrict__ models, const int32_t *__restrict__ ent_pod,
                                                                const int64_t *__restrict__ ent_time, const mmp_pod_row *__restrict__ pods,
                                                                int32_t P, int64_t now, int32_t *__restrict__ map, RopsScalars *rs,
                                                                int32_t *__restrict__ block_counts)
{
    const int i = blockIdx.x * kRopsBlock + threadIdx.x;
    bool edit = false, dup = false;
    int32_t kept = 0;
    if (i < n) {
        const mmp_registry_op op = ops[i];
        if (op.model >= 0) {
            dup = atomicCAS(&map[op.model], -1, i) != -1;
            const RopEval ev = rops_eval(models[op.model], ent_pod, ent_time, pods, P, op, now);
            edit = ev.edited;
            if (edit) kept = ev.nl + ev.nf;
        }
    }
    const int nd = __popcll(__ballot(dup));
    if (lane_id() == 0 && nd) atomicAdd(&rs->n_dup, nd);
    triple_count<kCol1None>(edit, 0, kept, block_counts);
}

// edits in op order (bounded by max_edits: a truncated prefix), one status byte per op, the totals; every map word this call
// took is -1 again when this kernel has run
__global__ __launch_bounds__(kRopsBlock) void rops_scatter_kernel(const mmp_registry_op *__restrict__ ops, int32_t n,
                                                                  const mmp_model_row *__restrict__ models, const int32_t *__restrict__ ent_pod,
                                                                  const int64_t *__restrict__ ent_time, const mmp_pod_row *__restrict__ pods,
                                                                  int32_t P, int64_t now, int32_t *__restrict__ map, RopsScalars *rs,
                                                                  const int32_t *__restrict__ block_off, mmp_registry_op_edit *__restrict__ edits,
                                                                  int32_t max_edits, int32_t *__restrict__ keep_off, uint8_t *__restrict__ status)
{
    const int i = blockIdx.x * kRopsBlock + threadIdx.x;
    mmp_registry_op op{};
    bool rec = false;  // the op names a record
    if (i < n) {
        op = ops[i];
        rec = op.model >= 0;
        if (rec) map[op.model] = -1;  // (every op of a model stores the same word)
    }
    if (rs->n_dup != 0) return;  // (uniform: the whole grid leaves; the call is refused)
    RopEval ev{};
    if (rec) ev = rops_eval(models[op.model], ent_pod, ent_time, pods, P, op, now);
    const bool edit = ev.edited;
    const int32_t kept = edit ? ev.nl + ev.nf : 0;
    const TripleOff o = triple_offsets<kCol1None>(edit, 0, kept, block_off);
    const int lane = lane_id();
    if (i < n) status[i] = !rec ? MMP_ROP_NO_RECORD : edit ? MMP_ROP_EDITED : MMP_ROP_UNCHANGED;
    if (edit) {
        const int32_t x = o.e;
        if (x < max_edits) {
            mmp_registry_op_edit ed;
            ed.model = op.model;
            ed.op_index = i;
            ed.n_loaded_after = ev.nl;
            ed.n_failed_after = ev.nf;
            ed.flags = ev.flags;
            ed.inserted_pos = ev.ins_pos;
            ed.last_used_after = ev.last_used;
            ed.last_unload_after = ev.last_unload;
            edits[x] = ed;
            keep_off[x] = o.k;
        }
    }
#pragma unroll
    for (int k = 0; k < kRopKinds; k++) {
        const int ce = __popcll(__ballot(rec && op.op == k && edit)), cu = __popcll(__ballot(rec && op.op == k && !edit));
        if (lane == 0) {
            if (ce) atomicAdd(&rs->n_edited[k], ce);
            if (cu) atomicAdd(&rs->n_unchanged[k], cu);
        }
    }
    const bool put_new = (ev.flags & (MMP_ROP_EDIT_PUT_LOADED | MMP_ROP_EDIT_PUT_FAILED)) && !(ev.flags & MMP_ROP_EDIT_REPLACED);
    const int na = __popcll(__ballot(put_new));
    const int nr = __popcll(__ballot(ev.flags & MMP_ROP_EDIT_REM_LOADED)) + __popcll(__ballot(ev.flags & MMP_ROP_EDIT_REM_FAILED));
    const int nn = __popcll(__ballot(i < n && !rec));
    if (lane == 0) {
        if (na) atomicAdd(&rs->n_added, na);
        if (nr) atomicAdd(&rs->n_removed, nr);
        if (nn) atomicAdd(&rs->n_no_record, nn);
    }
}

// apply: edit x's record, rebuilt at arena[base + keep_off[x] ...): instanceIds, then loadFailedInstanceIds, each without the
// op's instance where it was removed and with it — replaced where it stood, or inserted at inserted_pos — where it was put; its
// row for upsert_models_kernel.  `base + n_kept` lies inside the arena (the host grew it), and nothing refers to that part yet.
__global__ void rops_build_kernel(const mmp_registry_op_edit *__restrict__ edits, const int32_t *__restrict__ keep_off, int32_t n_edits,
                                  const mmp_registry_op *__restrict__ ops, const mmp_model_row *__restrict__ models,
                                  int32_t *__restrict__ ent_pod, int64_t *__restrict__ ent_time, int32_t base, int32_t arena_end,
                                  int32_t *__restrict__ u_idx, mmp_model_row *__restrict__ u_rows)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_edits) return;
    const mmp_registry_op_edit ed = edits[x];
    const mmp_registry_op op = ops[ed.op_index];
    const mmp_model_row m = models[ed.model];
    int32_t dst = base + keep_off[x];
    auto put = [&](int32_t pod, int64_t t) {
        if (dst < arena_end) {
            ent_pod[dst] = pod;
            ent_time[dst] = t;
        }
        dst++;
    };
    // one list: `rem` drops the op's instance, `ins` puts (op.pod, t_ins) — over its old entry, or as a new one at inserted_pos
    auto list = [&](int32_t off, int32_t cnt, bool rem, bool ins, int64_t t_ins) {
        const bool fresh = ins && !(ed.flags & MMP_ROP_EDIT_REPLACED);
        for (int32_t k = 0; k < cnt; k++) {
            const int32_t pod = ent_pod[off + k];
            const int64_t t = ent_time[off + k];
            if (pod == op.pod) {
                if (ins)
                    put(pod, t_ins);
                else if (!rem)
                    put(pod, t);
                continue;
            }
            if (fresh && k == ed.inserted_pos) put(op.pod, t_ins);
            put(pod, t);
        }
        if (fresh && ed.inserted_pos == cnt) put(op.pod, t_ins);
    };
    list(m.ent_off, m.n_loaded, ed.flags & MMP_ROP_EDIT_REM_LOADED, ed.flags & MMP_ROP_EDIT_PUT_LOADED, op.load_time);
    list(m.ent_off + m.n_loaded, m.n_failed, ed.flags & MMP_ROP_EDIT_REM_FAILED, ed.flags & MMP_ROP_EDIT_PUT_FAILED, op.load_complete_time);
    u_idx[x] = ed.model;
    u_rows[x] = mmp_model_row{m.type, base + keep_off[x], ed.n_loaded_after, ed.n_failed_after, ed.last_used_after};
}

}  // namespace mmp
