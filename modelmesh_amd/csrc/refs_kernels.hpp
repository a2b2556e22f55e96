// refs_kernels.hpp — incRefCount / decRefCount on a stored ModelRecord value (mmp_models_refs_json).
//
// The three vmodel writers (VModelManager.java updateVModel :137-385, deleteVModel :416-470, PendingTransition.run :716-767) move
// `refs` on up to three ModelRecords per transaction: the new target gains a referent and the previous active model's lu
// (:299-302), the models a vmodel lets go lose one and are deleted with it when they were created for it (decModelRefsInTxn
// :475-489).  The next bytes of such a record are a pure function of the request and its stored value (include/mmplace.h states
// the rule for callers, tests/model_refs_model.py as a program):
//
//   DEC  field = refs > 0 ? refs - 1 : refs,  return = refs > 0 ? refs - 1 : 0                   (ModelRecord.java:213-215)
//        ENSURE_ABSENT  no stored value: txn.ensureAbsent                                         (:485-487)
//        DELETE         return == 0 && autoDel: txn.delete with the old value                      (:478-480)
//        SET            every member not named refs, verbatim, then "refs":<field>, omitted at 0   (:482)
//   INC  field = return = refs + 1 as a Java int (2^31 - 1 wraps), lu = last_used                 (ModelRecord.java:220-222, :232-234)
//        CREATED        no stored value, a type given: {"type":..,"encKey":..,"mPath":..,"refs":1,"autoDel":true,"lu":<last_used>},
//                       encKey / mPath / autoDel / lu omitted at null / false / 0                   (:294, :301-302)
//        NOT_FOUND      no stored value, no type: "Target model not found"                         (:203-205)
//        SET            every member not named refs or lu, verbatim, then "refs":<field>, "lu":<last_used>, each omitted at 0
//   MALFORMED the parser's own verdict on the stored value;  HOST  a refs that is no int32, an autoDel (read by a DEC only) that
//        is neither true nor false
//
// ONE GRAMMAR and ONE WALK, rewrite_kernels.hpp's rw_walk, as in register_kernels.hpp: the walk keeps every member the request does
// not own and notes the value span of the last refs and the last autoDel, on the tile or, for a longer value, by lane 0.  The
// verdict is ingest_models_kernel's, which has run over the same staged values.
//
// One kernel body, two instantiations: the size pass settles class, count and the bytes a value takes, the write pass runs the
// same code with the stores switched on.  A wavefront takes one request.  Pure byte work: no MFMA.
#pragma once
#include "register_kernels.hpp"

namespace mmp {

struct RefsArgs : StoredArgs {  // (an empty span of buf: mr == null)
    const mmp_refs_req *reqs;
    const char *info;  // type, encKey, mPath of request i = spans 3i, 3i + 1, 3i + 2 (read by a CREATED only)
    const int32_t *info_off;
    int32_t *cls;
    int32_t *refs;
};

enum RefSlot { kRefRefs, kRefAutoDel, kRefNoted, kRefLu = kRefNoted };

// the noted names and lu (raw bytes, as the parser matches names); -1 for every other member
template <class B>
__device__ __forceinline__ int ref_slot_of(uint64_t h, int klen, const B *kp)
{
    if (KEY_IS(h, klen, kp, "refs")) return kRefRefs;
    if (KEY_IS(h, klen, kp, "autoDel")) return kRefAutoDel;
    if (KEY_IS(h, klen, kp, "lu")) return kRefLu;
    return -1;
}

// autoDel of the stored value: false where it is neither of the two literals (absent: false)
template <class B>
__device__ __forceinline__ bool ref_auto_del(const B *by, int vs, int ve, bool &auto_del)
{
    auto_del = false;
    if (vs < 0) return true;
    if (ve - vs == 4 && bytes_equal(by + vs, "true", 4)) {
        auto_del = true;
        return true;
    }
    return ve - vs == 5 && bytes_equal(by + vs, "false", 5);
}

// Class and count of a request whose stored value is there and well-formed; vs / ve: the value spans of the last refs and the
// last autoDel in `by`.  E holds the members that stay; a SET appends the owned ones and closes.
template <bool WRITE, class B>
__device__ __forceinline__ int32_t ref_decide(RwOut &E, const B *by, const int (&vs)[kRefNoted], const int (&ve)[kRefNoted], bool inc,
                                              int64_t last_used, int32_t &ret)
{
    int32_t refs, field;
    bool auto_del = false;
    ret = 0;
    if (!reg_refs(by, vs[kRefRefs], ve[kRefRefs], refs)) return MMP_MREFC_HOST;
    if (inc)
        field = ret = (int32_t)((uint32_t)refs + 1u);  // ++refCount, ModelRecord.java:221
    else {
        if (!ref_auto_del(by, vs[kRefAutoDel], ve[kRefAutoDel], auto_del)) return MMP_MREFC_HOST;
        field = refs > 0 ? refs - 1 : refs;  // refCount > 0 ? --refCount : 0, ModelRecord.java:214: the field stays where it is
        ret = refs > 0 ? refs - 1 : 0;
        if (ret == 0 && auto_del) return MMP_MREFC_DELETE;  // VModelManager.java:478-480
    }
    rw_long<WRITE>(E, "\"refs\":", 7, field);
    if (inc) rw_long<WRITE>(E, "\"lu\":", 5, last_used);  // setLastUsed, :301
    rw_close_record<WRITE>(E);
    return MMP_MREFC_SET;
}

// One request per wavefront.  WRITE false: cls[i], refs[i], len[i]; WRITE true: the bytes of every SET / CREATED value at
// out_off[i].
template <bool WRITE>
__global__ __launch_bounds__(kJBlock) void models_refs_kernel(RefsArgs A)
{
    __shared__ JWaveLds lds[kJWaves];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = lane_id();
    JWaveLds &S = lds[wave];
    const int i = blockIdx.x * kJWaves + wave;
    if (i >= A.n) return;
    if (WRITE) {
        const int32_t k = A.cls[i];
        if (k != MMP_MREFC_SET && k != MMP_MREFC_CREATED) return;
    }
    const mmp_refs_req q = A.reqs[i];
    const bool inc = (q.flags & MMP_MREF_INC) != 0;
    const int32_t o0 = A.info_off[3 * i], o1 = A.info_off[3 * i + 1], o2 = A.info_off[3 * i + 2], o3 = A.info_off[3 * i + 3];

    RwOut E = rw_open<WRITE>(A, i);
    int32_t cls, ret = 0;
    if (A.off[i + 1] == A.off[i]) {  // mr == null
        if (!inc)
            cls = MMP_MREFC_ENSURE_ABSENT;  // :485-487
        else if (o1 == o0)
            cls = MMP_MREFC_NOT_FOUND;  // :203-205: no modelInfo to create it from
        else {  // new ModelRecord(type, key, path, autoDelete) + setLastUsed + incRefCount, :294 / :301-302, defaults omitted
            reg_string<WRITE>(E, "\"type\":\"", 8, A.info + o0, o1 - o0);
            if (o2 > o1) reg_string<WRITE>(E, "\"encKey\":\"", 10, A.info + o1, o2 - o1);
            if (o3 > o2) reg_string<WRITE>(E, "\"mPath\":\"", 9, A.info + o2, o3 - o2);
            rw_head<WRITE>(E, E.units, "\"refs\":1", 8);
            if (q.flags & MMP_MREF_AUTO_DELETE) rw_head<WRITE>(E, E.units, "\"autoDel\":true", 14);
            rw_long<WRITE>(E, "\"lu\":", 5, q.last_used);
            rw_close_record<WRITE>(E);
            cls = MMP_MREFC_CREATED;
            ret = 1;
        }
    } else if (A.pstatus[i] != 0)
        cls = MMP_MREFC_MALFORMED;
    else {
        // ---- every member not named refs (an INC: nor lu) is a unit of a SET value; noted: the last refs and the last autoDel
        int vs[kRefNoted], ve[kRefNoted];
        const bool tile = rw_walk<WRITE>(A, i, S, E, [inc](uint64_t h, int klen, const auto *kp, uint32_t) {
            const int slot = ref_slot_of(h, klen, kp);
            return RwMember{slot != kRefRefs && !(inc && slot == kRefLu), slot < kRefNoted ? slot : -1};
        }, vs, ve);
        const auto decide = [&](const auto *by) {  // (the spans are offsets into what the walk ran over)
            return ref_decide<WRITE>(E, by, vs, ve, inc, q.last_used, ret);
        };
        cls = tile ? decide(j_view(S, 0).by) : decide(A.buf + S.off[0]);
    }
    if (!WRITE && lane == 0) {
        A.cls[i] = cls;
        A.refs[i] = ret;
        A.len[i] = cls == MMP_MREFC_SET || cls == MMP_MREFC_CREATED ? E.pos : 0;
    }
}

}  // namespace mmp
