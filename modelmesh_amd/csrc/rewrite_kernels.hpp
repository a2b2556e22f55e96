// rewrite_kernels.hpp — the write side of the wire format: the next stored value of a ModelRecord (mmp_models_rewrite_json).
//
// Every edit of the registry ends, in the reference, in a compare-and-set that writes a whole serialised ModelRecord back
// (ModelMesh.java: 13 conditionalSet / conditionalSetAndGet sites, 12 of them on the registry, every one of the 12 with a device
// edit call: the last, :3687, is MMP_ROP_DROP_LOCAL of mmp_registry_ops_k).  The device holds what the mesh
// owns of a record — the two id maps and lu — and nothing of the rest (type, mPath, encKey, refs, autoDel, the failure texts,
// any future field), so the new value is made of two halves: the members of the OLD value the device does not own, copied byte
// for byte, and the owned members rendered from the resident row.  The rule (include/mmplace.h states it for callers, tests/model_rewrite_model.py as a program):
//
//   new = '{' kept members ',' owned members '}', joined by single commas, no other blanks
//   kept   every top-level member whose raw name is not instanceIds / failedIn / fails / lu (/ lul when last_unload is given), in
//          document order, duplicates included, from the opening quote of its key to the last byte of its value
//   owned  "instanceIds":{"<id>":<time>,...}  "failedIn":{...}  "fails":{...}  "lu":<n>  "lul":<n>, each omitted at its default;
//          fails = the members of the last old `fails` object whose key is the id of a failed entry, minus those of fail_pod,
//          plus "<id>":{"msg":"<escaped>"} for a fail_pod that is in the failed list and brings a message
//
// ONE GRAMMAR: nothing here restates what an object is.  A value that fits the LDS tile is staged and classified by j_scan; the
// level-1 ':' / ',' masks give the spans of its members, the level-2 masks the members of `fails`, and lanes are spread over
// members, entries and copy bytes.  A longer value is walked by lane 0 through j_members.  Both routes over the top-level members
// are ONE WALK, rw_walk, which register_kernels.hpp calls too: a kernel brings a classifier.  The verdict (status 1) is the parser's
// own: ingest_models_kernel runs over the same staged values first, so the write side accepts exactly what the read side accepts.
// What ingest_kernels.hpp leaves UNSPECIFIED (a value invalid only inside a skipped value) stays unspecified here.
//
// One kernel body, two instantiations: the size pass counts the bytes a record takes (and settles status 2: an entry the device
// cannot name), the write pass runs the same code again with the stores switched on, every record at the offset the scan of the
// sizes gave it.  A wavefront takes one record.  Pure byte work: no MFMA, bound by the bytes read and written once.
#pragma once
#include "ingest_kernels.hpp"

namespace mmp {

struct VmEvent;  // (vmodel_kernels.hpp)

// What every "next stored value" kernel is given alike, and what the host's two-pass frame fills in (mmplace.hip, render_stored_values).
struct StoredArgs {
    const char *buf;  // the staged stored values (the buffers the parser has just read)
    const int64_t *off;
    int32_t n;
    const int32_t *pstatus;     // the parser's verdict on value i
    const mmp_model_row *prow;  // ... and the row it read (ModelRecord values: ingest_models_kernel)
    const VmEvent *pev;         // ... or the slots it read (VModelRecord values: vm_parse_kernel)
    int64_t *len;               // size pass: bytes of value i
    const int64_t *out_off;     // write pass: exclusive scan of len, out_off[n] = the total
    char *out;
};

struct RewriteArgs : StoredArgs {
    const int32_t *rows;  // registry row of value i
    const mmp_model_row *models;
    const int32_t *ent_pod;
    const int64_t *ent_time;
    const char *id_bytes;  // instance id p = id_bytes[id_off[p], id_off[p + 1]), p in [0, n_pods)
    const int32_t *id_off;
    int32_t n_pods;
    const int64_t *last_unload;  // nullptr: lul is an ordinary kept member
    const int32_t *fail_pod;     // nullptr: no row has one
    const char *fail_msg;
    const int32_t *fail_msg_off;
    int32_t *status;
};

// Where a record's bytes go.  Everything is laid out as UNITS: a separator byte and what follows it, the separator being the
// container's opener for its first unit and ',' for the others — so the opener costs nothing extra and no lane has to know
// whether something will follow.  pos and units are wave-uniform.
struct RwOut {
    char *out;
    int64_t pos, end;
    int32_t units;  // units of the record object so far
};

// The record of value i: nowhere in the size pass (pos counts its bytes from 0), at the offset the scan gave it in the write pass.
template <bool WRITE>
__device__ __forceinline__ RwOut rw_open(const StoredArgs &A, int i)
{
    RwOut E{A.out, 0, 0, 0};
    if (WRITE) {
        E.pos = A.out_off[i];
        E.end = A.out_off[i + 1];
    }
    return E;
}

template <bool WRITE>
__device__ __forceinline__ void rw_putc(const RwOut &E, int64_t p, uint32_t ch)
{
    if (WRITE && p < E.end) E.out[p] = (char)ch;  // (end: a record never writes into its neighbour)
}

// a Java long in plain decimal, Long.MIN_VALUE included
__device__ __forceinline__ int rw_dec_len(int64_t v)
{
    uint64_t m = v < 0 ? 0 - (uint64_t)v : (uint64_t)v;
    int n = v < 0 ? 1 : 0;
    do {
        n++;
        m /= 10u;
    } while (m);
    return n;
}

template <bool WRITE>
__device__ __forceinline__ void rw_dec_put(const RwOut &E, int64_t p, int64_t v, int len)
{
    uint64_t m = v < 0 ? 0 - (uint64_t)v : (uint64_t)v;
    const int first = v < 0 ? 1 : 0;
    for (int k = len - 1; k >= first; k--) {
        rw_putc<WRITE>(E, p + k, '0' + (uint32_t)(m % 10u));
        m /= 10u;
    }
    if (first) rw_putc<WRITE>(E, p, '-');
}

// a byte that cannot stand raw in a rendered key: the host renders such a record (status 2)
__device__ __forceinline__ bool rw_needs_escape(uint32_t c) { return c == '"' || c == '\\' || c < 0x20 || c > 0x7e; }

// The head of a unit of the record object, by the whole wavefront: its separator and the literal behind it (at most 63 bytes).
template <bool WRITE>
__device__ __forceinline__ void rw_head(RwOut &E, int32_t &units, const char *lit, int n)
{
    const int lane = lane_id();
    if (lane == 0) rw_putc<WRITE>(E, E.pos, units == 0 ? '{' : ',');
    if (lane < n) rw_putc<WRITE>(E, E.pos + 1 + lane, (unsigned char)lit[lane]);
    E.pos += 1 + n;
    units++;
}

template <bool WRITE>
__device__ __forceinline__ void rw_close(RwOut &E, uint32_t ch)
{
    if (lane_id() == 0) rw_putc<WRITE>(E, E.pos, ch);
    E.pos++;
}

// the close of the record object; one without units is '{}'
template <bool WRITE>
__device__ __forceinline__ void rw_close_record(RwOut &E)
{
    if (E.units == 0) rw_close<WRITE>(E, '{');
    rw_close<WRITE>(E, '}');
}

// Every lane may bring one span of `by` (len < 0: none): the spans become units behind E.pos in lane order, and every span is
// copied by all lanes together.
template <bool WRITE, class B>
__device__ __forceinline__ void rw_put_spans(RwOut &E, int32_t &units, const B *by, int soff, int len)
{
    const int lane = lane_id();
    const bool has = len >= 0;
    const int32_t unit = has ? len + 1 : 0;
    const int32_t incl = wave_incl_scan_i32(unit), cincl = wave_incl_scan_i32(has ? 1 : 0);
    const int32_t excl = incl - unit;
    if (WRITE) {
        if (has) rw_putc<WRITE>(E, E.pos + excl, units + cincl - 1 == 0 ? '{' : ',');
        uint64_t todo = __ballot(has && len > 0);
        while (todo) {
            const int l = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            const int s = readlane_i32(soff, l), n = readlane_i32(len, l);
            const int64_t d = E.pos + readlane_i32(excl, l) + 1;
            for (int b = lane; b < n; b += 64) rw_putc<WRITE>(E, d + b, (unsigned char)by[s + b]);
        }
    }
    E.pos += readlane_i32(incl, 63);
    units += readlane_i32(cincl, 63);
}

// The same by ONE lane, for a value longer than the tile: the separator, then the bytes [s, e) verbatim.
template <bool WRITE>
__device__ __forceinline__ void rw_put_serial(RwOut &E, int32_t &units, const char *s, const char *e)
{
    rw_putc<WRITE>(E, E.pos++, units++ == 0 ? '{' : ',');
    for (; s < e; s++) rw_putc<WRITE>(E, E.pos++, (unsigned char)*s);
}

// The unit of member M, the j-th of the n members of the container by[open .. close] (`commas`: the mask of its level): by[soff, end),
// from the opening quote of its key to the byte before its ',' (the closer behind the last member), blanks trimmed.
__device__ __forceinline__ bool rw_member_span(const JView &R, const uint64_t *commas, int open, int close, int n, int j, const JMember &M,
                                               int &soff, int &end)
{
    end = j == n - 1 ? close : j_nth_after(commas, R.nch, open, j);
    if (end < 0) return false;
    while (end > M.v && j_is_ws(R.by[end - 1])) end--;
    soff = (int)(M.kp - R.by) - 1;
    return true;
}

// What a caller of rw_walk says of a member: whether it stays, and the note slot it belongs to (-1: none).
struct RwMember {
    bool keep;
    int note;
};

// THE MEMBER WALK of both "next stored value" kernels, by the whole wavefront over value i: every top-level member that
// classify(hash, key length, key bytes, first byte of the value) keeps becomes a unit of the record object behind E.pos, in
// document order, and [vs[s], ve[s]) is the value of the LAST member classified into note slot s (-1: none).  True: the value
// fits the tile, which is staged and scanned (j_view(S, 0)) — one lane per member, 64 a round, the spans offsets into R.by.
// False: lane 0 has walked it through j_members, the spans are offsets into the value at A.buf + S.off[0], and a member whose
// value j_skip_value could not skip is neither kept nor noted.  E.pos, E.units and the spans are wave-uniform either way.
template <bool WRITE, int NOTES, class Off, class C>
__device__ __forceinline__ bool rw_walk(const StoredArgs &A, int i, JWaveLds &S, RwOut &E, const C &classify, Off (&vs)[NOTES],
                                        Off (&ve)[NOTES])
{
    const int lane = lane_id();
#pragma unroll
    for (int s = 0; s < NOTES; s++) vs[s] = ve[s] = -1;
    j_load_offsets(A.off, i, i + 1, S);
    if (j_group_len(S, 0, 1) == 1) {
        j_stage_and_scan(A.buf, 0, 1, S);
        const JView R = j_view(S, 0);
        for (int base = 0; base < R.n1; base += 64) {
            const int j = base + lane;
            int len = -1, soff = 0, end = -1, v = -1, note = -1;
            JMember M;
            if (j < R.n1 && j_member_at(R, R.c1, R.m1, R.f, j, M)) {
                const RwMember k = classify(M.h, M.klen, M.kp, M.v < R.L ? (uint32_t)R.by[M.v] : 0u);
                if ((k.keep || k.note >= 0) && rw_member_span(R, R.m1, R.f, R.g, R.n1, j, M, soff, end)) {
                    v = M.v;
                    note = k.note;
                    if (k.keep) len = end - soff;
                }
            }
#pragma unroll
            for (int s = 0; s < NOTES; s++) {  // the last member of the round in slot s: the highest lane that holds one
                const uint64_t m = __ballot(note == s);
                if (m) {
                    const int l = 63 - __clzll((unsigned long long)m);
                    vs[s] = readlane_i32(v, l);
                    ve[s] = readlane_i32(end, l);
                }
            }
            rw_put_spans<WRITE>(E, E.units, R.by, soff, len);
        }
        return true;
    }
    if (lane == 0) {
        const char *b = A.buf + S.off[0];
        JCur c{b, A.buf + S.off[1], false};
        j_members(c, true, [&](uint64_t h, int klen, const char *kp) {
            j_ws(c);
            const char *v = c.p;
            j_skip_value(c);
            if (c.bad) return;
            const RwMember k = classify(h, klen, kp, v < c.e ? (uint32_t)(unsigned char)*v : 0u);
#pragma unroll
            for (int s = 0; s < NOTES; s++)
                if (k.note == s) {
                    vs[s] = (Off)(v - b);
                    ve[s] = (Off)(c.p - b);
                }
            if (k.keep) rw_put_serial<WRITE>(E, E.units, kp - 1, c.p);
        });
    }
    E.pos = (int64_t)shfl_u64((uint64_t)E.pos, 0);
    E.units = shfl_i32(E.units, 0);
#pragma unroll
    for (int s = 0; s < NOTES; s++) {
        vs[s] = __shfl(vs[s], 0, 64);
        ve[s] = __shfl(ve[s], 0, 64);
    }
    return false;
}

// the owned names (matched as the parser matches names: raw bytes)
template <class B>
__device__ __forceinline__ bool rw_is_fails(uint64_t h, int klen, const B *kp) { return KEY_IS(h, klen, kp, "fails"); }
template <class B>
__device__ __forceinline__ bool rw_owned(uint64_t h, int klen, const B *kp, bool lul)
{
    const int s = model_slot_of(h, klen, kp);
    return s == kModLu || s == kModLoaded || s == kModFailed || (s == kModLul && lul) || rw_is_fails(h, klen, kp);
}

// The entries [eo, eo + cnt) of a row can all be named: the pod is a slot of the id store and its id stands raw between quotes.
__device__ __forceinline__ bool rw_renderable(const RewriteArgs &A, int32_t eo, int32_t cnt)
{
    const int lane = lane_id();
    bool bad = false;
    for (int32_t e = lane; e < cnt; e += 64) {
        const int32_t pod = A.ent_pod[eo + e];
        if (pod < 0 || pod >= A.n_pods)
            bad = true;
        else
            for (int32_t q = A.id_off[pod]; q < A.id_off[pod + 1]; q++) bad |= rw_needs_escape((unsigned char)A.id_bytes[q]);
    }
    return __ballot(bad) == 0;
}

// "instanceIds":{"<id>":<time>,...} / "failedIn":{...}: one lane per entry, placed by a wave prefix sum; omitted when empty
template <bool WRITE>
__device__ __forceinline__ void rw_id_map(RwOut &E, const RewriteArgs &A, const char *name, int nlen, int32_t eo, int32_t cnt)
{
    if (cnt == 0) return;
    const int lane = lane_id();
    rw_head<WRITE>(E, E.units, name, nlen);
    for (int32_t base = 0; base < cnt; base += 64) {
        const int32_t e = base + lane;
        const bool has = e < cnt;
        int32_t o = 0, idlen = 0, dlen = 0;
        int64_t t = 0;
        if (has) {
            const int32_t pod = A.ent_pod[eo + e];  // (in range: the size pass has settled status 2)
            o = A.id_off[pod];
            idlen = A.id_off[pod + 1] - o;
            t = A.ent_time[eo + e];
            dlen = rw_dec_len(t);
        }
        const int32_t unit = has ? idlen + 4 + dlen : 0;  // sep " id " : digits
        const int32_t incl = wave_incl_scan_i32(unit);
        if (WRITE && has) {
            int64_t p = E.pos + incl - unit;
            rw_putc<WRITE>(E, p++, e == 0 ? '{' : ',');
            rw_putc<WRITE>(E, p++, '"');
            for (int32_t q = 0; q < idlen; q++) rw_putc<WRITE>(E, p++, (unsigned char)A.id_bytes[o + q]);
            rw_putc<WRITE>(E, p++, '"');
            rw_putc<WRITE>(E, p++, ':');
            rw_dec_put<WRITE>(E, p, t, dlen);
        }
        E.pos += readlane_i32(incl, 63);
    }
    rw_close<WRITE>(E, '}');
}

// "lu":<n> / "lul":<n>, omitted at 0
template <bool WRITE>
__device__ __forceinline__ void rw_long(RwOut &E, const char *name, int nlen, int64_t v)
{
    if (v == 0) return;
    rw_head<WRITE>(E, E.units, name, nlen);
    const int dlen = rw_dec_len(v);
    if (lane_id() == 0) rw_dec_put<WRITE>(E, E.pos, v, dlen);
    E.pos += dlen;
}

// the message of addLoadFailure between quotes: '"' and '\' behind a backslash, a byte below 0x20 as \u00xx, the rest verbatim
template <bool WRITE>
__device__ __forceinline__ void rw_put_escaped(RwOut &E, const char *m, int n)
{
    const int lane = lane_id();
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const bool has = i < n;
        const uint32_t ch = has ? (unsigned char)m[i] : 0u;
        const int32_t w = !has ? 0 : (ch == '"' || ch == '\\') ? 2 : ch < 0x20 ? 6 : 1;
        const int32_t incl = wave_incl_scan_i32(w);
        if (WRITE && has) {
            int64_t p = E.pos + incl - w;
            if (w == 1)
                rw_putc<WRITE>(E, p, ch);
            else {
                rw_putc<WRITE>(E, p++, '\\');
                if (w == 2)
                    rw_putc<WRITE>(E, p, ch);
                else {
                    const uint32_t hi = ch >> 4, lo = ch & 15u;
                    rw_putc<WRITE>(E, p++, 'u');
                    rw_putc<WRITE>(E, p++, '0');
                    rw_putc<WRITE>(E, p++, '0');
                    rw_putc<WRITE>(E, p++, '0' + hi);
                    rw_putc<WRITE>(E, p, lo < 10 ? '0' + lo : 'a' + lo - 10);
                }
            }
        }
        E.pos += readlane_i32(incl, 63);
    }
}

// What the fails rule needs of a row: its failed entries and the instance of fail_pod (fp < 0: none).
struct RwFails {
    int32_t fo, nf;  // the failed entries of the row
    int32_t fp;
    int32_t fid_off, fid_len;  // the id of fp
};

// A member of the old `fails` object stays when its raw key is the id of a failed entry and not the id of fail_pod.
template <class B>
__device__ __forceinline__ bool rw_fails_keep(const RewriteArgs &A, const RwFails &F, const B *kp, int klen)
{
    if (F.fp >= 0 && F.fid_len == klen && bytes_equal(kp, A.id_bytes + F.fid_off, klen)) return false;
    for (int32_t e = 0; e < F.nf; e++) {
        const int32_t pod = A.ent_pod[F.fo + e];
        if (pod < 0 || pod >= A.n_pods) continue;
        const int32_t o = A.id_off[pod];
        if (A.id_off[pod + 1] - o == klen && bytes_equal(kp, A.id_bytes + o, klen)) return true;
    }
    return false;
}

// The members that stay of the `fails` object the walk noted at byte `at`, by the route the walk took — the tile: one lane per
// member, spans from the level-2 masks; else lane 0 through j_members: counted (EMIT false) or put as the units of the new
// object.  Returns how many.
template <bool WRITE, bool EMIT>
__device__ __forceinline__ int32_t rw_fails_members(RwOut &E, int32_t &funits, const RewriteArgs &A, const RwFails &F, const JWaveLds &S,
                                                    bool tile, int64_t at)
{
    const int lane = lane_id();
    int32_t kept = 0;
    if (tile) {
        const JView R = j_view(S, 0);
        const int open = (int)at, close = j_nth_after(R.e2, R.nch, open, 0);
        if (close < 0) return 0;
        const int nm = j_count(R.c2, open, close);
        for (int base = 0; base < nm; base += 64) {
            const int k = base + lane;
            int len = -1, soff = 0, end;
            JMember M;
            if (k < nm && j_member_at(R, R.c2, R.m2, open, k, M) && rw_fails_keep(A, F, M.kp, M.klen) &&
                rw_member_span(R, R.m2, open, close, nm, k, M, soff, end))
                len = end - soff;
            if (EMIT)
                rw_put_spans<WRITE>(E, funits, R.by, soff, len);
            else
                kept += __popcll((unsigned long long)__ballot(len >= 0));
        }
        return kept;
    }
    if (lane == 0) {
        JCur c{A.buf + S.off[0] + at, A.buf + S.off[1], false};
        j_members(c, false, [&](uint64_t, int klen, const char *kp) {
            j_skip_value(c);
            if (c.bad || !rw_fails_keep(A, F, kp, klen)) return;
            kept++;
            if (EMIT) rw_put_serial<WRITE>(E, funits, kp - 1, c.p);
        });
    }
    E.pos = (int64_t)shfl_u64((uint64_t)E.pos, 0);
    funits = shfl_i32(funits, 0);
    return shfl_i32(kept, 0);
}

// One record per wavefront.  WRITE false: len[i] and status[i]; WRITE true: the bytes of every status-0 record at out_off[i].
template <bool WRITE>
__global__ __launch_bounds__(kJBlock) void models_rewrite_kernel(RewriteArgs A)
{
    __shared__ JWaveLds lds[kJWaves];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = lane_id();
    JWaveLds &S = lds[wave];
    const int i = blockIdx.x * kJWaves + wave;
    if (i >= A.n) return;
    if (WRITE) {
        if (A.status[i] != 0) return;
    } else if (A.pstatus[i] != 0) {
        if (lane == 0) {
            A.status[i] = 1;
            A.len[i] = 0;
        }
        return;
    }
    const mmp_model_row row = A.models[A.rows[i]];
    const int32_t eo = row.ent_off, nl = row.n_loaded, nf = row.n_failed;
    if (!WRITE && !rw_renderable(A, eo, nl + nf)) {
        if (lane == 0) {
            A.status[i] = 2;
            A.len[i] = 0;
        }
        return;
    }
    RwFails F{eo + nl, nf, A.fail_pod ? A.fail_pod[i] : -1, 0, 0};
    const char *msg = nullptr;
    int32_t msg_len = 0;
    bool fp_failed = false;
    if (F.fp >= 0) {  // (inside [0, n_pods): the host has checked)
        F.fid_off = A.id_off[F.fp];
        F.fid_len = A.id_off[F.fp + 1] - F.fid_off;
        msg = A.fail_msg + A.fail_msg_off[i];
        msg_len = A.fail_msg_off[i + 1] - A.fail_msg_off[i];
        bool mine = false;
        for (int32_t e = lane; e < nf; e += 64) mine |= A.ent_pod[F.fo + e] == F.fp;
        fp_failed = __ballot(mine) != 0;
    }
    const bool append = F.fp >= 0 && msg_len > 0 && fp_failed;
    const bool lul = A.last_unload != nullptr;

    // ---- the kept members; noted: the '{' of the last `fails` member that is an object (one that is not is neither)
    RwOut E = rw_open<WRITE>(A, i);
    int64_t fails_at[1], fails_end[1];
    const bool tile = rw_walk<WRITE>(A, i, S, E, [lul](uint64_t h, int klen, const auto *kp, uint32_t v0) {
        return RwMember{!rw_owned(h, klen, kp, lul), rw_is_fails(h, klen, kp) && v0 == '{' ? 0 : -1};
    }, fails_at, fails_end);

    // ---- the owned members, from the resident row
    rw_id_map<WRITE>(E, A, "\"instanceIds\":", 14, eo, nl);
    rw_id_map<WRITE>(E, A, "\"failedIn\":", 11, eo + nl, nf);
    {
        int32_t funits = 0;
        const int32_t kept = fails_at[0] >= 0 && nf > 0 ? rw_fails_members<WRITE, false>(E, funits, A, F, S, tile, fails_at[0]) : 0;
        if (kept > 0 || append) {
            rw_head<WRITE>(E, E.units, "\"fails\":", 8);
            if (kept > 0) (void)rw_fails_members<WRITE, true>(E, funits, A, F, S, tile, fails_at[0]);
            if (append) {  // "<id>":{"msg":"<escaped message>"}
                if (lane == 0) {
                    int64_t p = E.pos;
                    rw_putc<WRITE>(E, p++, funits == 0 ? '{' : ',');
                    rw_putc<WRITE>(E, p++, '"');
                    for (int32_t q = 0; q < F.fid_len; q++) rw_putc<WRITE>(E, p++, (unsigned char)A.id_bytes[F.fid_off + q]);
                }
                E.pos += 2 + F.fid_len;
                const char *mid = "\":{\"msg\":\"";
                if (lane < 10) rw_putc<WRITE>(E, E.pos + lane, (unsigned char)mid[lane]);
                E.pos += 10;
                rw_put_escaped<WRITE>(E, msg, msg_len);
                if (lane == 0) {
                    rw_putc<WRITE>(E, E.pos, '"');
                    rw_putc<WRITE>(E, E.pos + 1, '}');
                }
                E.pos += 2;
            }
            rw_close<WRITE>(E, '}');
        }
    }
    rw_long<WRITE>(E, "\"lu\":", 5, row.last_used);
    if (lul) rw_long<WRITE>(E, "\"lul\":", 6, A.last_unload[i]);
    rw_close_record<WRITE>(E);
    if (!WRITE && lane == 0) {
        A.status[i] = 0;
        A.len[i] = E.pos;
    }
}

}  // namespace mmp

