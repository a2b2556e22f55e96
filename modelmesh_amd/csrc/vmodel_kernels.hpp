// vmodel_kernels.hpp — the vmodel table resident on the device (VModelManager.java:101-110, VModelRecord.java:26-41): its
// listener's events are taken by key (mmp_vmodels_events_json), and resolveVModelId, the classes of getVModelStatus and the
// leader's transition scan are answered from the rows (mmp_vmodels_resolve, mmp_vmodels_transitions).
//
// A vmodel id is an arbitrary user string like a model id: the id -> row map is a second ModelIdTab (model_ids_kernels.hpp), driven
// by the same kernels and the same host sequence.  A row holds no registry row: `amid` and `tmid` are kept as bytes in a string
// arena with their model-id hashes (masked as the model-id table's are), and every question resolves them through the model-id
// table with mid_find — a model that joins later, or one mmp_models_retire renumbered, is found without any vmodel call.
//
//   vm_parse_kernel        VModelRecord values on the frame of ingest_kernels.hpp (j_ingest_wave): the third record type, its own
//                          slots (VmSlot).  A string slot is (position, length, has-backslash): no byte is copied here.  A
//                          well-formed or deleted event atomicMax'es its index into its row's slot of `win` (the winner rule)
//   vm_counts_kernel       one lane per distinct row of the call: the bytes its winner appends, the bytes the row it replaces
//                          held, the change in rows that are not ABSENT
//   rocprim::exclusive_scan over those triples: where each winner's strings go, and the three totals
//   vm_build_kernel        one lane per distinct row: the winner's three strings into the arena, the hashes of amid / tmid, the row
//   vm_resolve_kernel      one lane per question
//   vm_trans_count_kernel / prune_scan_kernel / vm_trans_list_kernel   the transition scan, in row order (triple_count protocol)
//   vm_squeeze_len_kernel / rocprim scan / vm_squeeze_copy_kernel      the live strings into a fresh arena, rows beside the old ones
//
// No position comes from an atomic: which lane wins a race in `win` does not matter (the maximum does not depend on it), and every
// output is a function of the maxima and the scans, so two runs are byte-identical.  Strings are tens of bytes: a string is a loop
// of its lane, as in model_ids_kernels.hpp.
#pragma once
#include "retire_kernels.hpp"

namespace mmp {

constexpr int kVmBlock = kCompactBlock;  // (triple_count / triple_offsets are written for workgroups of this size)

// ---- VModelRecord: its slots and the name of each -------------------------------------------------------------------------------
enum VmSlot { kVmAmid, kVmTmid, kVmOwner, kVmFailed, kVmSlots };
static_assert(kVmSlots <= kJSlots, "JWaveLds::val / win hold every slot");

// the slot of a member name (VModelRecord.java:28-41), -1 for anything else (JsonExtensible: skipped)
template <class B>
__device__ __forceinline__ int vm_slot_of(uint64_t h, int klen, const B *kp)
{
    if (KEY_IS(h, klen, kp, "amid")) return kVmAmid;
    if (KEY_IS(h, klen, kp, "tmid")) return kVmTmid;
    if (KEY_IS(h, klen, kp, "o")) return kVmOwner;
    if (KEY_IS(h, klen, kp, "failed")) return kVmFailed;
    return -1;
}

// A string slot: 0 = absent or null; else bit 62, the has-backslash bit, the length, and the position of the first byte behind the
// opening quote, relative to the value's first byte.  The host refuses values of kVmMaxValue bytes and more.
constexpr int64_t kVmStrSet = 1ll << 62, kVmStrBs = 1ll << 61;
constexpr int kVmLenShift = 31;
constexpr int64_t kVmMaxValue = 1ll << 30;
__device__ __forceinline__ int64_t vm_str(int pos, int len, bool bs)
{
    return kVmStrSet | (bs ? kVmStrBs : 0) | ((int64_t)len << kVmLenShift) | (int64_t)pos;
}
__device__ __forceinline__ int32_t vm_str_pos(int64_t s) { return (int32_t)(s & 0x7fffffffll); }
__device__ __forceinline__ int32_t vm_str_len(int64_t s) { return (int32_t)((s >> kVmLenShift) & 0x3fffffffll); }

template <class B>
__device__ __forceinline__ bool vm_has_backslash(const B *p, int n)
{
    for (int i = 0; i < n; i++)
        if ((unsigned char)p[i] == '\\') return true;
    return false;
}

// one parsed event: the three string slots and `failed`; deleted: the event is ENTRY_DELETED
struct VmEvent {
    int64_t s[3];
    int32_t failed, deleted;
};

// row flags (include/mmplace.h: MMP_VMF_*)
constexpr uint32_t kVmfFailed = 1u, kVmfAbsent = 2u, kVmfActiveNull = 4u, kVmfTargetNull = 8u, kVmfOwnerNull = 16u, kVmfHost = 32u;

struct VmRow {  // 48 bytes
    uint64_t hash[2];            // the model-id hashes of amid and tmid (masked as the model-id table's)
    int32_t off[3], len[3];      // amid, tmid, o in the string arena
    uint32_t flags;
    int32_t reserved;
};
__host__ __device__ inline VmRow vm_absent_row()
{
    VmRow r{};
    r.flags = kVmfAbsent | kVmfActiveNull | kVmfTargetNull | kVmfOwnerNull;
    return r;
}

struct VmParseArgs {
    const char *buf;
    const int64_t *off;
    int32_t n, grp;
    const uint8_t *deleted;  // or nullptr
    const int32_t *slot;     // event -> its row's position among the call's distinct rows (k for an event without a row)
    int32_t *win;            // [k + 1] -1 before the launch
    VmEvent *ev;
    int32_t *status;
};

// One VModelRecord value walked by ONE lane (longer than the LDS tile) into the cleared slots fv[]: a later duplicate wins by
// program order, an earlier one is held to its type all the same.
__device__ __forceinline__ bool vm_record_serial(const char *b, const char *e, int64_t *fv)
{
    JCur c{b, e, false};
    j_members(c, true, [&](uint64_t h, int klen, const char *kp) {
        const int s = vm_slot_of(h, klen, kp);
        if (s < 0)
            j_skip_value(c);
        else if (s == kVmFailed)
            fv[s] = (int64_t)j_bool(c);
        else {
            j_ws(c);
            if (c.p < c.e && *c.p == '"') {
                const char *sp = c.p + 1;
                (void)j_string_hash(c);
                if (!c.bad) {
                    const int len = (int)(c.p - sp) - 1;
                    fv[s] = vm_str((int)(sp - b), len, vm_has_backslash(sp, len));
                }
            } else if (j_lit(c, "null", 4))
                fv[s] = 0;  // (what follows the literal is the member loop's to check)
            else
                c.bad = true;
        }
    });
    return c.bad;
}

// VModelRecord values, A.grp per WAVEFRONT.
__global__ __launch_bounds__(kJBlock) void vm_parse_kernel(VmParseArgs A)
{
    __shared__ JWaveLds lds[kJWaves];
    const int lane = lane_id();
    j_ingest_wave(
        lds, A.buf, A.off, A.n, A.grp,
        [&](JWaveLds &S, int i, const char *b, const char *e) {
            if (A.deleted && A.deleted[i]) return true;  // (a deleted event's value is not walked)
            return vm_record_serial(b, e, S.val[0]);
        },
        [&](JWaveLds &S, int, int cnt) {  // every member of every record of the group on its own lane
            const int total = j_prefix_fields(S, cnt);
            for (int base = 0; base < total; base += 64) {
                JField F{};
                int fid = -1;
                int64_t val = 0;
                bool lbad = false;
                if (base + lane < total) {
                    JView R;
                    lbad = !j_field_at(S, cnt, base + lane, R, F);
                    if (!lbad && (fid = vm_slot_of(F.m.h, F.m.klen, F.m.kp)) >= 0) {
                        int v = F.m.v;
                        if (fid == kVmFailed) {
                            if (j_lit_at(R, v, "true", 4)) {
                                val = 1;
                                v += 4;
                            } else if (j_lit_at(R, v, "false", 5))
                                v += 5;
                            else
                                lbad = true;
                        } else if (v < R.L && j_bit(R.rq, v)) {
                            const int ve = j_nth_after(R.rq, R.nch, v, 0);  // closing quote (strings are balanced)
                            val = vm_str(v + 1, ve - v - 1, vm_has_backslash(R.by + v + 1, ve - v - 1));
                            v = ve + 1;
                        } else if (j_lit_at(R, v, "null", 4))
                            v += 4;  // claimed, so that it also wins over an earlier duplicate that held a string
                        else
                            lbad = true;
                        if (!lbad && !j_term(R, v, R.m1, R.g, F.last)) lbad = true;
                    }
                }
                if (j_claim(S, F, fid, lbad) && S.win[F.r][fid] == F.j) S.val[F.r][fid] = val;
                wave_sync();
            }
        },
        // Events apply in order and a malformed one changes nothing: the row ends as its highest-numbered good event left it.
        [&](int i, bool bad, const int64_t *fv) {
            VmEvent e{};
            if (A.deleted && A.deleted[i]) {
                bad = false;
                e.deleted = 1;
            } else if (!bad) {
                e.s[0] = fv[kVmAmid];
                e.s[1] = fv[kVmTmid];
                e.s[2] = fv[kVmOwner];
                e.failed = (int32_t)fv[kVmFailed];
            }
            A.status[i] = bad ? 1 : 0;
            A.ev[i] = e;
            if (!bad) atomicMax(&A.win[A.slot[i]], i);
        });
}

// per distinct row, and after the exclusive scan per position: bytes appended in front of it, bytes of replaced rows in front of
// it, and the change in rows that are not ABSENT
struct VmBytes {
    int32_t add, sub, live;
};
struct VmBytesPlus {
    __host__ __device__ VmBytes operator()(const VmBytes &a, const VmBytes &b) const
    {
        return VmBytes{a.add + b.add, a.sub + b.sub, a.live + b.live};
    }
};

__device__ __forceinline__ int32_t vm_event_bytes(const VmEvent &e)
{
    return e.deleted ? 0 : vm_str_len(e.s[0]) + vm_str_len(e.s[1]) + vm_str_len(e.s[2]);
}

// cnt[k] = the zero triple, so that the scan's last element is the totals.  n_before: the rows before the call.
__global__ __launch_bounds__(256) void vm_counts_kernel(const int32_t *__restrict__ win, const VmEvent *__restrict__ ev, int32_t k,
                                                        const int32_t *__restrict__ slot_row, int32_t n_before,
                                                        const VmRow *__restrict__ rows, VmBytes *__restrict__ cnt)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j > k) return;
    VmBytes b{0, 0, 0};
    const int32_t w = j < k ? win[j] : -1;
    if (w >= 0) {
        b.add = vm_event_bytes(ev[w]);
        b.live = ev[w].deleted ? 0 : 1;
        const int32_t r = slot_row[j];
        if (r < n_before) {
            b.sub = rows[r].len[0] + rows[r].len[1] + rows[r].len[2];
            b.live -= (rows[r].flags & kVmfAbsent) ? 0 : 1;
        }
    }
    cnt[j] = b;
}

// One lane per distinct row.  The winner's strings go to arena[base + pos[j].add ...), which lies inside the arena (the host grew
// it by the scan's total) and beyond anything a published row refers to.  A row without a winner saw malformed events only: an
// existing one stays as it is, an appended one is ABSENT, because its number has been handed out.
__global__ __launch_bounds__(256) void vm_build_kernel(const int32_t *__restrict__ win, const int32_t *__restrict__ slot_row, int32_t k,
                                                       int32_t n_before, int32_t base, const VmBytes *__restrict__ pos,
                                                       const VmEvent *__restrict__ ev, const char *__restrict__ buf,
                                                       const int64_t *__restrict__ off, uint64_t model_hmask, VmRow *__restrict__ rows,
                                                       char *__restrict__ arena)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= k) return;
    const int32_t w = win[j], row = slot_row[j];
    if (w < 0) {
        if (row >= n_before) rows[row] = vm_absent_row();
        return;
    }
    const VmEvent e = ev[w];
    VmRow r = vm_absent_row();
    if (!e.deleted) {
        r.flags = e.failed ? kVmfFailed : 0u;
        int32_t o = base + pos[j].add;
        const char *val = buf + off[w];
#pragma unroll
        for (int s = 0; s < 3; s++) {
            if (!(e.s[s] & kVmStrSet)) {
                r.flags |= kVmfActiveNull << s;
                continue;
            }
            const int32_t len = vm_str_len(e.s[s]);
            const char *src = val + vm_str_pos(e.s[s]);
            for (int32_t q = 0; q < len; q++) arena[o + q] = src[q];
            if (e.s[s] & kVmStrBs) r.flags |= kVmfHost;
            if (s < 2) r.hash[s] = fnv1a(src, len) & model_hmask;
            r.off[s] = o;
            r.len[s] = len;
            o += len;
        }
    }
    rows[row] = r;
}
static_assert(kVmfTargetNull == kVmfActiveNull << 1 && kVmfOwnerNull == kVmfActiveNull << 2, "the null flags follow the slots");

// ---- the questions ---------------------------------------------------------------------------------------------------------------

struct VmTab {  // the published vmodel state
    ModelIdTab ids;
    const VmRow *rows;
    const char *arena;
    int32_t n_rows;
};
struct VmModels {  // the registry side: the model-id table and the resident rows
    ModelIdTab ids;
    const mmp_model_row *rows;
    int32_t n_models;
};

// the registry row of string s of the vmodel row, -1 for null or an id the model-id table does not know
__device__ __forceinline__ int32_t vm_model_of(const VmTab &V, const VmModels &M, const VmRow &r, int s)
{
    if (r.flags & (kVmfActiveNull << s)) return -1;
    const int32_t m = mid_find(M.ids, r.hash[s], V.arena + r.off[s], r.len[s]);
    return m < M.n_models ? m : -1;
}

// String.equals of the stored string s against the bytes [p, p + n): a stored null equals nothing
__device__ __forceinline__ bool vm_str_is(const VmTab &V, const VmRow &r, int s, const char *p, int32_t n)
{
    return !(r.flags & (kVmfActiveNull << s)) && r.len[s] == n && mid_same(V.arena + r.off[s], p, n);
}

// VModelRecord.inTransition(): !Objects.equals(amid, tmid), on bytes
__device__ __forceinline__ bool vm_in_transition(const VmTab &V, const VmRow &r)
{
    const bool an = r.flags & kVmfActiveNull, tn = r.flags & kVmfTargetNull;
    if (an || tn) return an != tn;
    return !(r.len[0] == r.len[1] && mid_same(V.arena + r.off[0], V.arena + r.off[1], r.len[0]));
}

__device__ __forceinline__ bool vm_model_empty(const mmp_model_row &m) { return retire_row_empty(m); }

// THE CHOICE of resolveVModelId (VModelManager.java:569-597) in both phases, behind absentOrOwnerMismatch (:530-532), stated once for
// vm_resolve_kernel and vkeyed_resolve_kernel (vkeyed_kernels.hpp).  [owner, owner + olen) and [np, np + nlen) are the owner and the
// notFoundModelId, an empty span Java null; after: the question is asked again behind the strong read.  which = -1 unless cls is
// MMP_VMR_OK.  For MMP_VMR_NOT_FOUND and MMP_VMR_HOST nothing else of the row is answered.
struct VmChoice {
    int32_t cls, which;
};
__device__ __forceinline__ VmChoice vm_choose(const VmTab &V, const VmRow &r, const char *owner, int32_t olen, const char *np, int32_t nlen,
                                              bool after)
{
    if (r.flags & kVmfAbsent) return VmChoice{MMP_VMR_NOT_FOUND, -1};  // :570-573
    if (r.flags & kVmfHost) return VmChoice{MMP_VMR_HOST, -1};
    if (olen > 0 && !vm_str_is(V, r, 2, owner, olen)) return VmChoice{MMP_VMR_NOT_FOUND, -1};  // :530-532, an owner is given and differs
    if (nlen == 0 || !vm_str_is(V, r, 0, np, nlen)) return VmChoice{MMP_VMR_OK, MMP_VMW_ACTIVE};  // :575, and :587 after the strong read
    if (!after) return VmChoice{MMP_VMR_STRONG_READ, -1};  // :582
    if (!vm_str_is(V, r, 1, np, nlen)) return VmChoice{MMP_VMR_OK, MMP_VMW_TARGET};  // :591
    return VmChoice{MMP_VMR_TARGET_NOT_FOUND, -1};  // :594
}

// The class of statusFromRecord (:555-556) and of resolveTargetModelStatusInfo (:537-549) for a row whose tmid resolved to the
// registry row target_model (-1: null or unknown), stated once for vm_resolve_kernel and vstatus_keyed_kernel
// (status_keyed_kernels.hpp).  Not in transition: DEFINED / NONE.
struct VmStatus {
    int32_t vstatus, target_status;
};
__device__ __forceinline__ VmStatus vm_status_of(const VmTab &V, const VmModels &M, const VmRow &r, int32_t target_model)
{
    if (!vm_in_transition(V, r)) return VmStatus{MMP_VMS_DEFINED, MMP_VMT_NONE};
    const bool failed = r.flags & kVmfFailed;
    VmStatus s{failed ? MMP_VMS_TRANSITION_FAILED : MMP_VMS_TRANSITIONING, MMP_VMT_NOT_FOUND};
    if (target_model >= 0) {
        const mmp_model_row t = M.rows[target_model];
        if (!vm_model_empty(t)) s.target_status = failed && t.n_failed > 0 && t.n_loaded == 0 ? MMP_VMT_LOADING_FAILED : MMP_VMT_LOADING;
    }
    return s;
}

// resolveVModelId and absentOrOwnerMismatch (vm_choose), the class of statusFromRecord
// (:555-556) and of resolveTargetModelStatusInfo (:537-549).  Spans: key i, and where given nf i and owner i; an empty span is
// Java null.
__global__ __launch_bounds__(kIdTabBlock) void vm_resolve_kernel(const char *__restrict__ keys, const int32_t *__restrict__ key_off,
                                                                 int32_t n, uint64_t vm_hmask, const char *__restrict__ nf,
                                                                 const int32_t *__restrict__ nf_off, const char *__restrict__ owners,
                                                                 const int32_t *__restrict__ owner_off,
                                                                 const uint32_t *__restrict__ req_flags, VmTab V, VmModels M,
                                                                 mmp_vmodel_answer *__restrict__ out)
{
    const int i = blockIdx.x * kIdTabBlock + threadIdx.x;
    if (i >= n) return;
    mmp_vmodel_answer a{};
    a.cls = MMP_VMR_NOT_FOUND;
    a.vmodel = a.model = a.target_model = -1;
    const char *key = keys + key_off[i];
    const int32_t klen = key_off[i + 1] - key_off[i];
    const int32_t v = mid_find(V.ids, fnv1a(key, klen) & vm_hmask, key, klen);
    const VmRow r = v >= 0 && v < V.n_rows ? V.rows[v] : vm_absent_row();
    const int32_t olen = owner_off ? owner_off[i + 1] - owner_off[i] : 0, nlen = nf_off ? nf_off[i + 1] - nf_off[i] : 0;
    const VmChoice ch = vm_choose(V, r, olen > 0 ? owners + owner_off[i] : nullptr, olen, nlen > 0 ? nf + nf_off[i] : nullptr, nlen,
                                  req_flags && (req_flags[i] & MMP_VMRQ_AFTER_STRONG));
    a.cls = ch.cls;
    if (ch.cls == MMP_VMR_HOST)
        a.vmodel = v;
    else if (ch.cls != MMP_VMR_NOT_FOUND) {
        const int which = ch.which;
        a.vmodel = v;
        a.target_model = vm_model_of(V, M, r, 1);
        if (which >= 0) {
            a.which = which;
            a.model = which ? a.target_model : vm_model_of(V, M, r, 0);
            if (r.flags & (kVmfActiveNull << which)) a.flags |= MMP_VMRF_NULL_ID;
        }
        const VmStatus vs = vm_status_of(V, M, r, a.target_model);
        a.vstatus = vs.vstatus;
        a.target_status = vs.target_status;
    }
    out[i] = a;
}

// ---- processVModels (:617-634), the filter of processVModel (:639-643), the prologue of PendingTransition.run (:701-708) ----------

struct VmTransArgs {
    VmTab V;
    VmModels M;
    int64_t now, age;
};

// listed: the row is neither ABSENT nor HOST and in transition; the rest of `t` is written for a listed row
__device__ __forceinline__ bool vm_transition(const VmTransArgs &A, int32_t v, mmp_vmodel_transition &t, bool &host)
{
    host = false;
    if (v >= A.V.n_rows) return false;
    const VmRow r = A.V.rows[v];
    if (r.flags & kVmfAbsent) return false;
    if (r.flags & kVmfHost) {
        host = true;
        return false;
    }
    if (!vm_in_transition(A.V, r)) return false;
    t = mmp_vmodel_transition{};
    t.vmodel = v;
    t.from_model = vm_model_of(A.V, A.M, r, 0);
    t.to_model = vm_model_of(A.V, A.M, r, 1);
    t.flags = (r.flags & kVmfFailed) ? MMP_VMXF_FAILED : 0u;
    t.cls = MMP_VMX_PROMOTE;
    if (t.from_model >= 0) {
        const mmp_model_row m = A.M.rows[t.from_model];
        if (vm_model_empty(m)) t.flags |= MMP_VMXF_FROM_EMPTY;
        t.target_count = m.n_loaded;  // :702
        if (m.n_loaded > 0) {
            t.cls = MMP_VMX_ENSURE_LOADED;  // :705-708, Java long arithmetic
            t.last_used = m.last_used != 0 ? m.last_used : (int64_t)((uint64_t)A.now - (uint64_t)A.age);
        }
    }
    if (t.to_model >= 0 && vm_model_empty(A.M.rows[t.to_model])) t.flags |= MMP_VMXF_TO_EMPTY;
    return true;
}

// the triple of a row: listed, of those PROMOTE, HOST rows skipped
__global__ __launch_bounds__(kVmBlock) void vm_trans_count_kernel(VmTransArgs A, int32_t *__restrict__ block_counts)
{
    const int v = blockIdx.x * kVmBlock + threadIdx.x;
    mmp_vmodel_transition t{};
    bool host;
    const bool listed = vm_transition(A, v, t, host);
    triple_count<kCol1Count>(listed, listed && t.cls == MMP_VMX_PROMOTE, host ? 1 : 0, block_counts);
}

__global__ __launch_bounds__(kVmBlock) void vm_trans_list_kernel(VmTransArgs A, const int32_t *__restrict__ block_off,
                                                                 mmp_vmodel_transition *__restrict__ out, int32_t max_rows)
{
    const int v = blockIdx.x * kVmBlock + threadIdx.x;
    mmp_vmodel_transition t{};
    bool host;
    const bool listed = vm_transition(A, v, t, host);
    const TripleOff o = triple_offsets<kCol1Count>(listed, listed && t.cls == MMP_VMX_PROMOTE, host ? 1 : 0, block_off);
    if (listed && o.e < max_rows) out[o.e] = t;
}

// ---- the string arena's garbage ------------------------------------------------------------------------------------------------

// len[v] = the bytes row v holds, len[n] = 0 (so that the scan's last element is the live bytes)
__global__ __launch_bounds__(256) void vm_squeeze_len_kernel(const VmRow *__restrict__ rows, int32_t n, int32_t *__restrict__ len)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v > n) return;
    len[v] = v < n ? rows[v].len[0] + rows[v].len[1] + rows[v].len[2] : 0;
}

// pos = the exclusive scan of len: row v's strings to next_arena[pos[v] ...), amid, tmid, o in that order; next_rows beside rows
__global__ __launch_bounds__(256) void vm_squeeze_copy_kernel(const VmRow *__restrict__ rows, int32_t n, const int32_t *__restrict__ pos,
                                                              const char *__restrict__ arena, VmRow *__restrict__ next_rows,
                                                              char *__restrict__ next_arena)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    VmRow r = rows[v];
    int32_t o = pos[v];
#pragma unroll
    for (int s = 0; s < 3; s++) {
        const int32_t len = r.len[s];
        for (int32_t q = 0; q < len; q++) next_arena[o + q] = arena[r.off[s] + q];
        r.off[s] = len ? o : 0;
        o += len;
    }
    next_rows[v] = r;
}

}  // namespace mmp
