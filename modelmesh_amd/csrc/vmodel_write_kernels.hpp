// vmodel_write_kernels.hpp — the record step of the three vmodel writers (mmp_vmodels_write_json): updateVModel
// (VModelManager.java:137-385), deleteVModel (:416-470) and the tail of PendingTransition.run (:716-767).
//
// What one attempt of such a transaction computes — the class of the request, the next VModelRecord bytes and the ids whose refs
// move — is a pure function of the request, the stored vmodel value and two facts of the resident registry: the number of loaded
// copies of the previous active model (:248 / :261) and its lastUsed (:299).  include/mmplace.h states the rule for callers,
// tests/vmodel_write_model.py as a program.  The transaction itself, its retry loop and the waiters stay in Java.
//
//   next value   every top-level member of the old value not named amid / tmid / failed, verbatim and in document order (o among
//                them: it is final in the bean), then "amid":"..", "tmid":"..", "failed":true, each omitted at null / false.  A
//                string that stays is copied raw from the stored value, one the request brings is escaped by the rewrite's rule
//   dec          an id whose ModelRecord loses a referent (mmp_models_refs_json renders that step), named as a span of the old value
//
// ONE GRAMMAR: the verdict and the three string slots are vm_parse_kernel's, which has run over the same staged values; the kept
// members come from rewrite_kernels.hpp's rw_walk with a classifier of three names; request strings go through rw_put_escaped.
// String comparisons are spread over the lanes as reg_attr spreads them; ids are resolved with mid_find on hashes computed from
// the bytes, as vm_build_kernel computes them.
//
// One kernel body, two instantiations: the size pass settles the row and the bytes a value takes, the write pass runs the same
// code with the stores switched on.  A wavefront takes one request.  Pure byte work: no MFMA.
#pragma once
#include "register_kernels.hpp"
#include "vmodel_kernels.hpp"

namespace mmp {

struct VmWriteArgs : StoredArgs {  // (an empty span of buf: vmr == null; pev[i]: the parser's slots of value i)
    const mmp_vmodel_write_req *reqs;
    const char *strs;  // id_a, id_b, owner of request i = spans 3i, 3i + 1, 3i + 2; span 3n: the default owner
    const int32_t *str_off;
    VmModels M;
    uint64_t model_hmask;
    int64_t now, age;
    mmp_vmodel_write_row *rows;
};

// A Java String of the step: null, or len bytes at p.  pos: where a stored one starts in its value.
struct VwStr {
    const char *p;
    int32_t len, pos;
    bool set;
};

__device__ __forceinline__ VwStr vw_request(const VmWriteArgs &A, int span)  // (an empty span is null)
{
    const int32_t o = A.str_off[span], n = A.str_off[span + 1] - o;
    return VwStr{A.strs + o, n, 0, n > 0};
}

__device__ __forceinline__ VwStr vw_stored(const char *val, int64_t slot)
{
    if (!(slot & kVmStrSet)) return VwStr{val, 0, 0, false};
    return VwStr{val + vm_str_pos(slot), vm_str_len(slot), vm_str_pos(slot), true};
}

// String.equals on bytes, the bytes spread over the lanes; null equals nothing
__device__ __forceinline__ bool vw_eq(const VwStr &a, const VwStr &b)
{
    if (!a.set || !b.set || a.len != b.len) return false;
    bool diff = false;
    for (int32_t k = lane_id(); k < a.len; k += 64) diff |= a.p[k] != b.p[k];
    return __ballot(diff) == 0;
}

// Objects.equals: null equals null
__device__ __forceinline__ bool vw_objects_eq(const VwStr &a, const VwStr &b) { return a.set || b.set ? vw_eq(a, b) : true; }

// the registry row of an id, -1 for null or an id the model-id table does not know
__device__ __forceinline__ int32_t vw_model(const VmWriteArgs &A, const VwStr &s)
{
    if (!s.set) return -1;
    const int32_t m = mid_find(A.M.ids, fnv1a(s.p, s.len) & A.model_hmask, s.p, s.len);
    return m >= 0 && m < A.M.n_models ? m : -1;
}

// prevActive = registry.getOrStrongIfAbsent(prevActiveId) as the device holds it: its loaded copies (unresolved entries included)
// and its lastUsed; an unknown id and the empty row read as null
__device__ __forceinline__ void vw_prev_active(const VmWriteArgs &A, const VwStr &id, mmp_vmodel_write_row &r, int64_t &last_used)
{
    const int32_t m = vw_model(A, id);
    last_used = 0;
    r.target_copy_count = 0;
    if (m >= 0) {
        const mmp_model_row row = A.M.rows[m];
        if (!vm_model_empty(row)) {
            r.target_copy_count = row.n_loaded;
            last_used = row.last_used;
            return;
        }
    }
    r.flags |= MMP_VWF_PREV_ACTIVE_UNKNOWN;
}

__device__ __forceinline__ void vw_dec(const VmWriteArgs &A, mmp_vmodel_write_row &r, int k, const VwStr &id)
{
    r.dec_model[k] = vw_model(A, id);
    r.dec_off[k] = id.pos;
    r.dec_len[k] = id.len;
}

// ,"name":"<bytes>" as a unit of the record object: raw from the stored value, escaped from the request
template <bool WRITE>
__device__ __forceinline__ void vw_string(RwOut &E, const char *head, int hlen, const VwStr &s, bool from_request)
{
    if (from_request) {
        reg_string<WRITE>(E, head, hlen, s.p, s.len);
        return;
    }
    rw_head<WRITE>(E, E.units, head, hlen);
    for (int32_t k = lane_id(); k < s.len; k += 64) rw_putc<WRITE>(E, E.pos + k, (unsigned char)s.p[k]);
    E.pos += s.len;
    rw_close<WRITE>(E, '"');
}

// One request per wavefront.  WRITE false: rows[i], len[i]; WRITE true: the bytes of every CREATED / UPDATED value at out_off[i].
template <bool WRITE>
__global__ __launch_bounds__(kJBlock) void vmodels_write_kernel(VmWriteArgs A)
{
    __shared__ JWaveLds lds[kJWaves];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = lane_id();
    JWaveLds &S = lds[wave];
    const int i = blockIdx.x * kJWaves + wave;
    if (i >= A.n) return;
    if (WRITE) {
        const int32_t k = A.rows[i].cls;
        if (k != MMP_VWC_CREATED && k != MMP_VWC_UPDATED) return;
    }
    const mmp_vmodel_write_req q = A.reqs[i];
    const VwStr ida = vw_request(A, 3 * i), idb = vw_request(A, 3 * i + 1), own = vw_request(A, 3 * i + 2);
    const bool absent = A.off[i + 1] == A.off[i], bad = !absent && A.pstatus[i] != 0;
    const char *val = A.buf + A.off[i];
    VmEvent ev{};
    if (!absent && !bad) ev = A.pev[i];
    const VwStr am = vw_stored(val, ev.s[kVmAmid]), tm = vw_stored(val, ev.s[kVmTmid]), so = vw_stored(val, ev.s[kVmOwner]);
    const bool failed = ev.failed != 0;

    mmp_vmodel_write_row r{};
    r.model = r.dec_model[0] = r.dec_model[1] = -1;
    r.dec_len[0] = r.dec_len[1] = -1;
    // the record after the step; *_req: the string is the request's
    VwStr nam = am, ntm = tm;
    bool am_req = false, tm_req = false, nfailed = failed;
    int32_t cls;
    const bool reads_owner = (q.op == MMP_VW_SET || q.op == MMP_VW_DELETE) && own.set;
    if (bad)
        cls = MMP_VWC_MALFORMED;
    else if (q.op != MMP_VW_FAIL_FLAG && (((ev.s[kVmAmid] | ev.s[kVmTmid]) & kVmStrBs) || (reads_owner && (ev.s[kVmOwner] & kVmStrBs))))
        cls = MMP_VWC_HOST;  // (an absent value has no slots)
    else if (q.op == MMP_VW_SET) {
        // initialCacheTimestamp, :168-170 (Java long arithmetic: the product and the difference wrap)
        const int64_t ict = (int64_t)((uint64_t)A.now - (uint64_t)A.age * ((q.flags & MMP_VWQ_LOAD_NOW) ? 1ull : 6ull));
        const bool force = (q.flags & MMP_VWQ_FORCE) != 0;
        if (absent) {
            if (idb.set && !vw_eq(idb, ida))
                cls = MMP_VWC_PRECONDITION;  // :178 (the strong read stands in front of the loop), :280
            else if (q.flags & MMP_VWQ_UPDATE_ONLY)
                cls = MMP_VWC_NOT_FOUND;  // :277
            else {
                cls = MMP_VWC_CREATED;  // :282
                r.last_used = ict;
            }
        } else if (own.set && !vw_eq(so, own))
            cls = MMP_VWC_OWNER_MISMATCH;  // :181, :222
        else {
            const bool tmatch = vw_eq(tm, ida), amatch = vw_eq(am, ida);  // :229-230
            int64_t prev_lu = 0;
            if (!tmatch && idb.set && !vw_eq(idb, tm))
                cls = MMP_VWC_PRECONDITION;  // :184, :232
            else if (tmatch && (amatch || !force)) {
                cls = MMP_VWC_UNCHANGED;  // :243, :250
                if (!amatch && am.set) vw_prev_active(A, am, r, prev_lu);  // :246-249
            } else {
                mmp_vmodel_write_row d = r;  // (the dec fields and flags of an UPDATED answer)
                bool needs = false;
                if (!tmatch) {
                    ntm = ida;  // :236
                    tm_req = true;
                    if (tm.set && !vw_eq(tm, am)) vw_dec(A, d, 0, tm);  // :237-239
                }
                if (!amatch) {
                    if (!am.set) {
                        nam = ida;  // :258
                        am_req = true;
                    } else {
                        vw_prev_active(A, am, d, prev_lu);  // :260-261
                        const bool exists = (q.flags & MMP_VWQ_TARGET_EXISTS) != 0, one = exists && d.target_copy_count == 1;
                        if (force || d.target_copy_count == 0 || (one && (q.flags & MMP_VWQ_TARGET_LOADED))) {  // :262-265
                            nam = ida;  // :268-269
                            am_req = true;
                            vw_dec(A, d, 1, am);
                            d.flags |= MMP_VWF_ACTIVE_SWITCHED;
                        } else if (one && !(q.flags & (MMP_VWQ_TARGET_LOADED | MMP_VWQ_TARGET_NOT_LOADED)))
                            needs = true;  // getStatus(target) is the host's to ask
                    }
                }
                if (needs) {
                    cls = MMP_VWC_NEEDS_TARGET_STATUS;
                    r.target_copy_count = 1;
                    nam = am;
                    ntm = tm;
                } else {
                    cls = MMP_VWC_UPDATED;
                    r = d;
                    nfailed = false;                             // :273
                    r.last_used = prev_lu > 0 ? prev_lu : ict;  // :299-300
                }
            }
        }
        if (cls == MMP_VWC_CREATED || cls == MMP_VWC_UPDATED || cls == MMP_VWC_UNCHANGED || cls == MMP_VWC_NEEDS_TARGET_STATUS)
            r.model = vw_model(A, ida);
    } else if (q.op == MMP_VW_DELETE) {
        if (absent || (own.set && !vw_eq(so, own)))
            cls = MMP_VWC_NOOP;  // :419, :457 absentOrOwnerMismatch
        else {
            cls = MMP_VWC_DELETE;
            if (am.set) vw_dec(A, r, 0, am);                         // :438
            if (tm.set && !vw_objects_eq(tm, am)) vw_dec(A, r, 1, tm);  // :429, :441
        }
    } else if (q.op == MMP_VW_COMPLETE) {
        // :762-763 (an empty id_b stands for a stored null amid, where the Java would throw)
        if (absent || !(idb.set ? vw_eq(am, idb) : !am.set) || !vw_eq(tm, ida))
            cls = MMP_VWC_CHANGED;
        else {
            cls = MMP_VWC_UPDATED;
            nam = ida;  // :753
            am_req = true;
            nfailed = false;  // :754
            if (am.set) vw_dec(A, r, 0, am);  // :756
        }
    } else {  // MMP_VW_FAIL_FLAG, :736-738
        const bool want = (q.flags & MMP_VWQ_FAILED) != 0;
        if (absent)
            cls = MMP_VWC_NOOP;  // :726
        else if (want == failed)
            cls = MMP_VWC_UNCHANGED;
        else {
            cls = MMP_VWC_UPDATED;
            nfailed = want;
        }
    }
    // VModelRecord.inTransition() of the record as it stands after the step (UNCHANGED: as stored)
    if ((cls == MMP_VWC_UPDATED || cls == MMP_VWC_UNCHANGED) && !vw_objects_eq(nam, ntm)) r.flags |= MMP_VWF_IN_TRANSITION;

    RwOut E = rw_open<WRITE>(A, i);
    if (cls == MMP_VWC_CREATED) {  // new VModelRecord(targetModelId, owner != null ? owner : DEFAULT_OWNER), :282
        const VwStr o = own.set ? own : vw_request(A, 3 * A.n);
        if (o.set) vw_string<WRITE>(E, "\"o\":\"", 5, o, true);
        vw_string<WRITE>(E, "\"amid\":\"", 8, ida, true);
        vw_string<WRITE>(E, "\"tmid\":\"", 8, ida, true);
        rw_close_record<WRITE>(E);
    } else if (cls == MMP_VWC_UPDATED) {
        int vs[1], ve[1];
        (void)rw_walk<WRITE>(A, i, S, E, [](uint64_t h, int klen, const auto *kp, uint32_t) {
            const int slot = vm_slot_of(h, klen, kp);
            return RwMember{slot < 0 || slot == kVmOwner, -1};
        }, vs, ve);
        if (nam.set) vw_string<WRITE>(E, "\"amid\":\"", 8, nam, am_req);
        if (ntm.set) vw_string<WRITE>(E, "\"tmid\":\"", 8, ntm, tm_req);
        if (nfailed) rw_head<WRITE>(E, E.units, "\"failed\":true", 13);
        rw_close_record<WRITE>(E);
    }
    if (!WRITE && lane == 0) {
        r.cls = cls;
        A.rows[i] = r;
        A.len[i] = cls == MMP_VWC_CREATED || cls == MMP_VWC_UPDATED ? E.pos : 0;
    }
}

}  // namespace mmp
