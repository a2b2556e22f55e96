// rewrite_kernels.hpp — the write side of the wire format: the next stored value of a ModelRecord (mmp_models_rewrite_json).
//
// Every edit of the registry ends, in the reference, in a compare-and-set that writes a whole serialised ModelRecord back
// (ModelMesh.java: 13 conditionalSet / conditionalSetAndGet sites, 12 of them on the registry).  The device holds what the mesh
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
// members, entries and copy bytes.  A longer value is walked by lane 0 through j_members.  The verdict (status 1) is the parser's
// own: ingest_models_kernel runs over the same staged values first, so the write side accepts exactly what the read side accepts.
// What ingest_kernels.hpp leaves UNSPECIFIED (a value invalid only inside a skipped value) stays unspecified here.
//
// One kernel body, two instantiations: the size pass counts the bytes a record takes (and settles status 2: an entry the device
// cannot name), the write pass runs the same code again with the stores switched on, every record at the offset the scan of the
// sizes gave it.  A wavefront takes one record.  Pure byte work: no MFMA, bound by the bytes read and written once.
#pragma once
#include "ingest_kernels.hpp"

namespace mmp {

struct RewriteArgs {
    const char *buf;      // the staged old values (the buffers the parser has just read)
    const int64_t *off;
    int32_t n;
    const int32_t *rows;     // registry row of value i
    const int32_t *pstatus;  // the parser's verdict on value i
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
    int64_t *len;            // size pass: bytes of record i
    const int64_t *out_off;  // write pass: exclusive scan of len, out_off[n] = the total
    int32_t *status;
    char *out;
};

// Where a record's bytes go.  Everything is laid out as UNITS: a separator byte and what follows it, the separator being the
// container's opener for its first unit and ',' for the others — so the opener costs nothing extra and no lane has to know
// whether something will follow.  pos and units are wave-uniform.
struct RwOut {
    char *out;
    int64_t pos, end;
    int32_t units;  // units of the record object so far
};

template <bool WRITE>
__device__ __forceinline__ void rw_putc(const RwOut &E, int64_t p, uint32_t ch)
{
    if (WRITE && p < E.end) E.out[p] = (char)ch;  // (end: a record never writes into its neighbour)
}

__device__ __forceinline__ int32_t rw_wave_max(int32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int32_t t = __shfl_xor(v, o, 64);
        v = t > v ? t : v;
    }
    return v;
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

// The members of the `fails` object at tile byte `open` that stay, by the whole wavefront, one lane per member: counted
// (EMIT false; returns how many) or put as the units of the new object.
template <bool WRITE, bool EMIT>
__device__ __forceinline__ int32_t rw_fails_tile(RwOut &E, int32_t &funits, const RewriteArgs &A, const RwFails &F, const JView &R,
                                                 int open)
{
    const int lane = lane_id();
    const int close = j_nth_after(R.e2, R.nch, open, 0);
    if (close < 0) return 0;
    const int nm = j_count(R.c2, open, close);
    int32_t kept = 0;
    for (int base = 0; base < nm; base += 64) {
        const int k = base + lane;
        int len = -1, soff = 0;
        JMember M;
        if (k < nm && j_member_at(R, R.c2, R.m2, open, k, M) && M.p < close && rw_fails_keep(A, F, M.kp, M.klen)) {
            int e = j_nth_after(R.m2, R.nch, M.p, 0);  // the ',' behind the value, or the closer behind the last one
            if (e < 0 || e > close) e = close;
            while (e > M.v && j_is_ws(R.by[e - 1])) e--;
            soff = (int)(M.kp - R.by) - 1;
            len = e - soff;
        }
        if (EMIT)
            rw_put_spans<WRITE>(E, funits, R.by, soff, len);
        else
            kept += __popcll((unsigned long long)__ballot(len >= 0));
    }
    return kept;
}

// The same by ONE lane, for a value longer than the tile: the object at b[at], walked through j_members.
template <bool WRITE, bool EMIT>
__device__ __forceinline__ int32_t rw_fails_serial(RwOut &E, int32_t &funits, const RewriteArgs &A, const RwFails &F, const char *b,
                                                   const char *e, int64_t at)
{
    JCur c{b + at, e, false};
    int32_t kept = 0;
    j_members(c, false, [&](uint64_t, int klen, const char *kp) {
        j_skip_value(c);
        if (c.bad || !rw_fails_keep(A, F, kp, klen)) return;
        kept++;
        if (EMIT) {
            rw_putc<WRITE>(E, E.pos++, funits++ == 0 ? '{' : ',');
            for (const char *q = kp - 1; q < c.p; q++) rw_putc<WRITE>(E, E.pos++, (unsigned char)*q);
        }
    });
    return kept;
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

    RwOut E{A.out, 0, 0, 0};
    if (WRITE) {
        E.pos = A.out_off[i];
        E.end = A.out_off[i + 1];
    }
    const int64_t start = E.pos;

    j_load_offsets(A.off, i, i + 1, S);
    const char *b = A.buf + S.off[0], *e = A.buf + S.off[1];
    const bool tile = j_group_len(S, 0, 1) == 1;
    int64_t fails_at = -1;  // the '{' of the last `fails` member that is an object: tile byte / value byte
    if (tile) {
        // ---- the kept members: one lane per member of the record object, spans from the level-1 masks
        j_stage_and_scan(A.buf, 0, 1, S);
        const JView R = j_view(S, 0);
        int32_t fails_j = -1;
        for (int base = 0; base < R.n1; base += 64) {
            const int j = base + lane;
            int len = -1, soff = 0, cand = -1;
            JMember M;
            if (j < R.n1 && j_member_at(R, R.c1, R.m1, R.f, j, M)) {
                if (rw_owned(M.h, M.klen, M.kp, lul)) {
                    if (rw_is_fails(M.h, M.klen, M.kp) && M.v < R.L && R.by[M.v] == '{') cand = j;
                } else {
                    int ce = j == R.n1 - 1 ? R.g : j_nth_after(R.m1, R.nch, R.f, j);
                    if (ce >= 0) {
                        while (ce > M.v && j_is_ws(R.by[ce - 1])) ce--;
                        soff = (int)(M.kp - R.by) - 1;
                        len = ce - soff;
                    }
                }
            }
            fails_j = max(fails_j, rw_wave_max(cand));
            rw_put_spans<WRITE>(E, E.units, R.by, soff, len);
        }
        if (fails_j >= 0) {
            JMember M;
            if (j_member_at(R, R.c1, R.m1, R.f, fails_j, M)) fails_at = M.v;
        }
    } else {
        // ---- the same by lane 0 through j_members
        if (lane == 0) {
            JCur c{b, e, false};
            j_members(c, true, [&](uint64_t h, int klen, const char *kp) {
                j_ws(c);
                const char *v = c.p;
                j_skip_value(c);
                if (c.bad) return;
                if (rw_owned(h, klen, kp, lul)) {
                    if (rw_is_fails(h, klen, kp) && v < e && *v == '{') fails_at = v - b;
                    return;
                }
                rw_putc<WRITE>(E, E.pos++, E.units++ == 0 ? '{' : ',');
                for (const char *q = kp - 1; q < c.p; q++) rw_putc<WRITE>(E, E.pos++, (unsigned char)*q);
            });
        }
        E.pos = (int64_t)shfl_u64((uint64_t)E.pos, 0);
        E.units = shfl_i32(E.units, 0);
        fails_at = (int64_t)shfl_u64((uint64_t)fails_at, 0);
    }

    // ---- the owned members, from the resident row
    rw_id_map<WRITE>(E, A, "\"instanceIds\":", 14, eo, nl);
    rw_id_map<WRITE>(E, A, "\"failedIn\":", 11, eo + nl, nf);
    {
        int32_t kept = 0, funits = 0;
        if (fails_at >= 0 && nf > 0) {
            if (tile)
                kept = rw_fails_tile<WRITE, false>(E, funits, A, F, j_view(S, 0), (int)fails_at);
            else {
                if (lane == 0) kept = rw_fails_serial<WRITE, false>(E, funits, A, F, b, e, fails_at);
                kept = shfl_i32(kept, 0);
            }
        }
        if (kept > 0 || append) {
            rw_head<WRITE>(E, E.units, "\"fails\":", 8);
            if (kept > 0) {
                if (tile)
                    (void)rw_fails_tile<WRITE, true>(E, funits, A, F, j_view(S, 0), (int)fails_at);
                else {
                    if (lane == 0) (void)rw_fails_serial<WRITE, true>(E, funits, A, F, b, e, fails_at);
                    E.pos = (int64_t)shfl_u64((uint64_t)E.pos, 0);
                    funits = shfl_i32(funits, 0);
                }
            }
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
    if (E.units == 0) rw_close<WRITE>(E, '{');
    rw_close<WRITE>(E, '}');
    if (!WRITE && lane == 0) {
        A.status[i] = 0;
        A.len[i] = E.pos - start;
    }
}

}  // namespace mmp
