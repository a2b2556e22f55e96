// register_kernels.hpp — registerModel / deleteModel as questions about a stored ModelRecord value (mmp_models_register_json).
//
// The management API's two registry writers (ModelMesh.java:3088-3147 registerModel, :3181-3203 deleteModel) read four members of
// the stored value the device does not hold — type, encKey, mPath for the "already exists with different attributes" check, refs for
// the delete guard — plus lu for the touch rule, and write either a whole new record or the old one with a raised lu.  The answer is a
// pure function of the request, the stored value, now and LASTUSED_AGE_ON_ADD_MS (include/mmplace.h states the rule for callers,
// tests/model_register_model.py as a program):
//
//   ts       ict >= now ? now : ict > 0 ? ict : now - age * (loadNow ? 1 : 6)                     (:3098-3101, Java long arithmetic)
//   CREATED  no stored value: {"type":"<t>","encKey":"<k>","mPath":"<p>","lu":<ts>}, the last three omitted at null / 0  (:3135-3137)
//   CONFLICT one of the three attributes differs from the deciding (last) occurrence in the stored value            (:3111-3118)
//   TOUCHED  !loadNow && ts > lu + age: every member not named lu, verbatim, then "lu":<max(lu, ts or now)>          (:3120-3122)
//   EXISTS   otherwise                                                                                             (:3129)
//   ABSENT / REFERENCED / DELETABLE  a delete: no stored value / refs > 0 / the host may conditionalDelete        (:3187-3198)
//   MALFORMED the parser's own verdict on the stored value;  HOST  a compared member the device will not decide (an escape in a
//            compared string, an encKey / mPath / type of another kind, a refs that is no int32)
//
// ONE GRAMMAR and ONE WALK, rewrite_kernels.hpp's rw_walk: it keeps every member not named lu and notes the value span of the last
// occurrence of each compared name, on the tile or, for a longer value, by lane 0; the string comparison is spread over the
// lanes.  The verdict is ingest_models_kernel's, which has run over the same staged values and also leaves lu.
//
// One kernel body, two instantiations: the size pass settles class, last_used and the bytes a value takes, the write pass runs
// the same code with the stores switched on.  A wavefront takes one request (measured beside the rewrite).
#pragma once
#include "rewrite_kernels.hpp"

namespace mmp {

struct RegisterArgs : StoredArgs {  // (an empty span of buf: registry.get() == null; prow[i].last_used = lu)
    const mmp_register_req *reqs;
    const char *info;  // type, encKey, mPath of request i = spans 3i, 3i + 1, 3i + 2
    const int32_t *info_off;
    int64_t now, age;
    int32_t *cls;
    int64_t *last_used;
};

enum RegSlot { kRegType, kRegEncKey, kRegMPath, kRegRefs, kRegCompared, kRegLu = kRegCompared };

// the compared names and lu (raw bytes, as the parser matches names); -1 for every other member
template <class B>
__device__ __forceinline__ int reg_slot_of(uint64_t h, int klen, const B *kp)
{
    if (KEY_IS(h, klen, kp, "type")) return kRegType;
    if (KEY_IS(h, klen, kp, "encKey")) return kRegEncKey;
    if (KEY_IS(h, klen, kp, "mPath")) return kRegMPath;
    if (KEY_IS(h, klen, kp, "refs")) return kRegRefs;
    if (KEY_IS(h, klen, kp, "lu")) return kRegLu;
    return -1;
}

enum RegCmp { kRegEqual, kRegUnequal, kRegHost };

// One attribute of the stored value, by[vs, ve) being the deciding occurrence's value (vs < 0: no such member), against the
// request's bytes (rlen 0: null, except for the type, which is never empty).  Whole wavefront, the bytes spread over the lanes.
template <class B>
__device__ __forceinline__ int reg_attr(const B *by, int vs, int ve, const char *req, int rlen, bool is_type)
{
    const int lane = lane_id();
    if (vs < 0 || (ve - vs == 4 && bytes_equal(by + vs, "null", 4))) {
        if (!is_type) return rlen == 0 ? kRegEqual : kRegUnequal;                       // null against null
        return rlen == 12 && bytes_equal(req, "NLCLASSIFIER", 12) ? kRegEqual : kRegUnequal;  // ModelRecord.java:122
    }
    if (ve - vs < 2 || by[vs] != '"') return kRegHost;  // neither a string nor null
    const int s = vs + 1, n = ve - vs - 2;
    bool esc = false, diff = false;
    for (int b = lane; b < n; b += 64) {
        const uint32_t ch = (unsigned char)by[s + b];
        esc |= ch == '\\';
        if (n == rlen) diff |= ch != (uint32_t)(unsigned char)req[b];
    }
    if (__ballot(esc)) return kRegHost;
    if (n != rlen || (!is_type && rlen == 0)) return kRegUnequal;  // (a stored "" is not the request's null)
    return __ballot(diff) ? kRegUnequal : kRegEqual;
}

// refs of the stored value: false where it is not an integer in int32 (absent: 0).  Every lane reads the same few bytes.
template <class B>
__device__ __forceinline__ bool reg_refs(const B *by, int vs, int ve, int32_t &refs)
{
    refs = 0;
    if (vs < 0) return true;
    int p = vs;
    const bool neg = by[p] == '-';
    if (neg) p++;
    if (p >= ve) return false;
    uint64_t v = 0;
    for (; p < ve; p++) {
        const uint32_t ch = (unsigned char)by[p];
        if (ch < '0' || ch > '9') return false;
        v = v * 10u + (ch - '0');
        if (v > 0x80000000ull) return false;
    }
    if (!neg && v > 0x7fffffffull) return false;
    refs = neg ? (int32_t)(0 - (uint32_t)v) : (int32_t)v;
    return true;
}

// ,"name":"<escaped bytes>" as a unit of the record object
template <bool WRITE>
__device__ __forceinline__ void reg_string(RwOut &E, const char *head, int hlen, const char *s, int n)
{
    rw_head<WRITE>(E, E.units, head, hlen);
    rw_put_escaped<WRITE>(E, s, n);
    rw_close<WRITE>(E, '"');
}

// Class, and with it the length, of a request whose stored value is there and well-formed; vs / ve: the value spans of the last
// occurrence of each compared name in `by`.  E holds the members that are not lu; a touch appends the raised lu and closes.
template <bool WRITE, class B>
__device__ __forceinline__ int32_t reg_decide(RwOut &E, const RegisterArgs &A, const B *by, const int (&vs)[kRegCompared],
                                              const int (&ve)[kRegCompared], bool del, bool load_now, int64_t ts, int64_t lu,
                                              const char *info, int32_t o0, int32_t o1, int32_t o2, int32_t o3)
{
    if (del) {
        int32_t refs;
        if (!reg_refs(by, vs[kRegRefs], ve[kRegRefs], refs)) return MMP_MREG_HOST;
        return refs > 0 ? MMP_MREG_REFERENCED : MMP_MREG_DELETABLE;  // ModelMesh.java:3188-3191 / :3198
    }
    const int a = reg_attr(by, vs[kRegType], ve[kRegType], info + o0, o1 - o0, true);      // :3111
    const int b = reg_attr(by, vs[kRegEncKey], ve[kRegEncKey], info + o1, o2 - o1, false);  // :3112
    const int c = reg_attr(by, vs[kRegMPath], ve[kRegMPath], info + o2, o3 - o2, false);    // :3113
    if (a == kRegHost || b == kRegHost || c == kRegHost) return MMP_MREG_HOST;
    if (a != kRegEqual || b != kRegEqual || c != kRegEqual) return MMP_MREG_CONFLICT;  // :3117
    if (load_now || !(ts > (int64_t)((uint64_t)lu + (uint64_t)A.age))) return MMP_MREG_EXISTS;  // :3120, :3129
    const int64_t t = ts == 0 ? A.now : ts;  // updateLastUsed, ModelRecord.java:239-246: 0 means now, and only upwards
    rw_long<WRITE>(E, "\"lu\":", 5, t > lu ? t : lu);
    rw_close_record<WRITE>(E);
    return MMP_MREG_TOUCHED;
}

// One request per wavefront.  WRITE false: cls[i], last_used[i], len[i]; WRITE true: the bytes of every CREATED / TOUCHED value
// at out_off[i].
template <bool WRITE>
__global__ __launch_bounds__(kJBlock) void models_register_kernel(RegisterArgs A)
{
    __shared__ JWaveLds lds[kJWaves];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = lane_id();
    JWaveLds &S = lds[wave];
    const int i = blockIdx.x * kJWaves + wave;
    if (i >= A.n) return;
    if (WRITE) {
        const int32_t k = A.cls[i];
        if (k != MMP_MREG_CREATED && k != MMP_MREG_TOUCHED) return;
    }
    const mmp_register_req q = A.reqs[i];
    const bool del = (q.flags & MMP_MREG_DELETE) != 0, load_now = (q.flags & MMP_MREG_LOAD_NOW) != 0;
    const int64_t ict = q.initial_cache_timestamp;
    // lastUsedTimestamp, ModelMesh.java:3098-3101 (Java long arithmetic: the product and the difference wrap)
    const int64_t ts = del ? 0
                           : ict >= A.now ? A.now
                                          : ict > 0 ? ict : (int64_t)((uint64_t)A.now - (uint64_t)A.age * (load_now ? 1ull : 6ull));
    const int32_t o0 = A.info_off[3 * i], o1 = A.info_off[3 * i + 1], o2 = A.info_off[3 * i + 2], o3 = A.info_off[3 * i + 3];

    RwOut E = rw_open<WRITE>(A, i);
    int32_t cls;
    if (A.off[i + 1] == A.off[i]) {  // registry.get() == null
        if (del)
            cls = MMP_MREG_ABSENT;  // :3187: fine if not found
        else {  // new ModelRecord(type, encKey, mPath, false) + setLastUsed, :3135-3137, as Jackson writes it (defaults omitted)
            reg_string<WRITE>(E, "\"type\":\"", 8, A.info + o0, o1 - o0);
            if (o2 > o1) reg_string<WRITE>(E, "\"encKey\":\"", 10, A.info + o1, o2 - o1);
            if (o3 > o2) reg_string<WRITE>(E, "\"mPath\":\"", 9, A.info + o2, o3 - o2);
            rw_long<WRITE>(E, "\"lu\":", 5, ts);
            rw_close_record<WRITE>(E);
            cls = MMP_MREG_CREATED;
        }
    } else if (A.pstatus[i] != 0)
        cls = MMP_MREG_MALFORMED;
    else {
        // ---- every member not named lu is a unit of a touched value; noted: the last occurrence of each compared name
        int vs[kRegCompared], ve[kRegCompared];
        const bool tile = rw_walk<WRITE>(A, i, S, E, [](uint64_t h, int klen, const auto *kp, uint32_t) {
            const int slot = reg_slot_of(h, klen, kp);
            return RwMember{slot != kRegLu, slot < kRegCompared ? slot : -1};
        }, vs, ve);
        const auto decide = [&](const auto *by) {  // (the spans are offsets into what the walk ran over)
            return reg_decide<WRITE>(E, A, by, vs, ve, del, load_now, ts, A.prow[i].last_used, A.info, o0, o1, o2, o3);
        };
        cls = tile ? decide(j_view(S, 0).by) : decide(A.buf + S.off[0]);
    }
    if (!WRITE && lane == 0) {
        A.cls[i] = cls;
        A.last_used[i] = ts;
        A.len[i] = cls == MMP_MREG_CREATED || cls == MMP_MREG_TOUCHED ? E.pos : 0;
    }
}

}  // namespace mmp

