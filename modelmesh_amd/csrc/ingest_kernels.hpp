// ingest_kernels.hpp — the KV-store wire format straight into the packed tables.
//
// ModelMesh keeps InstanceRecord and ModelRecord values as Jackson JSON in etcd / ZooKeeper
// (MM.java:346 INST_REC_SERIALIZER, :628 registry view).  These kernels parse the raw values on the
// device.  A WAVEFRONT takes a group of up to kJGroup consecutive records (j_ingest_wave, the frame of both
// kernels).  The records of the group that fit the LDS tile together are staged into it with coalesced
// dword loads and classified 64 bytes at a time with ballots (j_scan: unescaped quotes, string interiors by
// prefix-xor, nesting depth by popcounts), after which every field / map entry of every such record is
// parsed by its own lane; a record longer than the tile is walked by one lane.  Both routes leave the
// values of the known fields in the wavefront's slots (JWaveLds::val), and one publish turns the slots into
// the packed row.
//
// ONE GRAMMAR, stated once.  What an object is — braces, members, separators — is j_members for the lane
// that walks and j_scan + j_member_at for the lanes of the tile.  What a record holds is stated per record
// type, for both routes: the slots (PodSlot, ModelSlot), the @JsonProperty name of each slot, matched by
// length + FNV-1a hash and then byte for byte (pod_slot_of, model_slot_of — InstanceRecord.java:37-69,
// ModelRecord.java:61-114; `instanceIds` has no @JsonProperty and serialises under its bean name), and the
// row made of the slots (pod_row_from_slots, the publish of ingest_models_kernel).  Fields Jackson omits
// because they hold the default value come out as 0 / false, exactly like the bean's defaults.  Instance
// ids inside a ModelRecord (the keys of instanceIds / failedIn) are resolved to pod indices through an
// open-addressing table of id hashes built when the ids are loaded.  The `labels` of an InstanceRecord are no slot of the
// pod parser: once label names are loaded (mmp_label_names_load) a second kernel over the same staged values,
// ingest_pod_labels_kernel, turns the array into a 64-bit word of known-label bits and an element count.
//
// Pure byte / integer work: no MFMA, bound by the bytes of JSON read once.
//
// Malformed values (status 1, row untouched): empty or blank values, truncated or unbalanced nesting / strings, a value
// that does not start with '{', bytes other than blanks behind its closing brace, a known field or a map entry whose
// value has the wrong type, missing, doubled or trailing ',' or ':' separators.  Both routes give the same verdict and
// the same row for such a value and for every well-formed one, whatever its length; a later duplicate of a field wins,
// the maps included (the row holds the entries of the last instanceIds / failedIn only), also a `"type":null` or a
// `"shutdown":false` behind an earlier one; an EARLIER duplicate is held to its type all the same (the entries of a
// map that lost are walked, not written).  A rejected ModelRecord of a full reload leaves the empty row of the default
// type.  A map key may be empty: `"":1,`
// is the shortest entry, five bytes, which is what the parking rule of the entries rests on (kJEntryBytes below).
// UNSPECIFIED — the two routes may differ, tests/ingest_model.py names the class and no test relies on it: a value that
// is invalid only INSIDE a value that is skipped (unknown fields, loc / zone, fails, and labels while no label names are loaded:
// the wave path checks balanced nesting there and nothing else, the serial walk a little more), a raw control byte inside
// a label string, leading zeros, integers outside int64 / int32,
// a `type` that is neither a string nor null, and backslash escapes in the names and keys the parsers hash.
#pragma once
#include "snapshot.hpp"

namespace mmp {

constexpr uint64_t kFnvBasis = 0xcbf29ce484222325ull;
__host__ __device__ constexpr uint64_t fnv1a_step(uint64_t h, uint64_t byte) { return (h ^ byte) * 0x100000001b3ull; }

template <class B>
__host__ __device__ constexpr uint64_t fnv1a(const B *s, int n)
{
    uint64_t h = kFnvBasis;
    for (int i = 0; i < n; i++) h = fnv1a_step(h, (unsigned char)s[i]);
    return h;
}
#define MMP_KEY(lit) fnv1a(lit, (int)sizeof(lit) - 1)
template <class B>
__device__ __forceinline__ bool bytes_equal(const B *p, const char *lit, int n)
{
    for (int i = 0; i < n; i++)
        if ((unsigned char)p[i] != (unsigned char)lit[i]) return false;
    return true;
}
// A field name is recognised by hash + length and then CONFIRMED byte for byte (kp = its first byte): an unknown
// field whose name collides on both (FNV-1a is not collision resistant against a chosen name) is skipped like any
// other unknown field instead of being parsed as the known one.
#define KEY_IS(h, klen, kp, lit) \
    ((h) == MMP_KEY(lit) && (klen) == (int)sizeof(lit) - 1 && bytes_equal((kp), lit, (int)sizeof(lit) - 1))

__device__ __forceinline__ bool j_is_ws(uint32_t c) { return c == ' ' || c == '\n' || c == '\t' || c == '\r'; }

struct JCur {
    const char *p, *e;
    bool bad;
};

__device__ __forceinline__ void j_ws(JCur &c)
{
    while (c.p < c.e && j_is_ws(*c.p)) c.p++;
}

__device__ __forceinline__ bool j_eat(JCur &c, char ch)
{
    j_ws(c);
    if (c.p < c.e && *c.p == ch) {
        c.p++;
        return true;
    }
    return false;
}

// the literal at the cursor, taken if it is there
__device__ __forceinline__ bool j_lit(JCur &c, const char *lit, int n)
{
    if (c.e - c.p < n || !bytes_equal(c.p, lit, n)) return false;
    c.p += n;
    return true;
}

// at the opening quote: hash the raw bytes up to the closing quote (escapes are hashed verbatim)
__device__ __forceinline__ uint64_t j_string_hash(JCur &c)
{
    uint64_t h = kFnvBasis;
    if (c.p >= c.e || *c.p != '"') {
        c.bad = true;
        return 0;
    }
    c.p++;
    while (c.p < c.e && *c.p != '"') {
        if (*c.p == '\\') {
            h = fnv1a_step(h, (unsigned char)*c.p);
            c.p++;
            if (c.p >= c.e) break;
        }
        h = fnv1a_step(h, (unsigned char)*c.p);
        c.p++;
    }
    if (c.p >= c.e) {
        c.bad = true;
        return 0;
    }
    c.p++;  // closing quote
    return h;
}

__device__ __forceinline__ void j_skip_value(JCur &c)
{
    j_ws(c);
    if (c.p >= c.e) {
        c.bad = true;
        return;
    }
    if (*c.p == '"') {
        (void)j_string_hash(c);
        return;
    }
    if (*c.p == '{' || *c.p == '[') {
        int depth = 0;
        while (c.p < c.e) {
            const char ch = *c.p;
            if (ch == '"') {
                (void)j_string_hash(c);
                if (c.bad) return;
                continue;
            }
            if (ch == '{' || ch == '[') depth++;
            if (ch == '}' || ch == ']') {
                depth--;
                if (depth == 0) {
                    c.p++;
                    return;
                }
            }
            c.p++;
        }
        c.bad = true;
        return;
    }
    // number / true / false / null
    while (c.p < c.e && *c.p != ',' && *c.p != '}' && *c.p != ']' && !j_is_ws(*c.p)) c.p++;
}

// a Java long / int written by Jackson: optional '-', digits (wraps like Long.parseLong would not — a
// value that does not fit is malformed for these beans)
__device__ __forceinline__ int64_t j_int(JCur &c)
{
    j_ws(c);
    bool neg = false;
    if (c.p < c.e && *c.p == '-') {
        neg = true;
        c.p++;
    }
    if (c.p >= c.e || *c.p < '0' || *c.p > '9') {
        c.bad = true;
        return 0;
    }
    uint64_t v = 0;
    while (c.p < c.e && *c.p >= '0' && *c.p <= '9') {
        v = v * 10u + (uint64_t)(*c.p - '0');
        c.p++;
    }
    if (c.p < c.e && (*c.p == '.' || *c.p == 'e' || *c.p == 'E')) c.bad = true;  // not an integer
    return neg ? (int64_t)(0 - v) : (int64_t)v;
}

__device__ __forceinline__ bool j_bool(JCur &c)
{
    j_ws(c);
    if (j_lit(c, "true", 4)) return true;
    if (!j_lit(c, "false", 5)) c.bad = true;
    return false;
}

// The members of the object at the cursor, the serial statement of what j_scan + j_member_at check on the tile: '{', members
// `"key" : value` separated by exactly one ',', '}'.  member(h, klen, kp) gets the key's hash, length and first byte with the
// cursor behind the ':' and consumes the value.  whole_value: the object is the record, and nothing but blanks may follow
// its closing brace (the wave path: zero_pos == R.g).
template <class F>
__device__ __forceinline__ void j_members(JCur &c, bool whole_value, F &&member)
{
    if (!j_eat(c, '{')) c.bad = true;
    bool first = true;
    while (!c.bad) {
        j_ws(c);
        if (c.p < c.e && *c.p == '}') {
            c.p++;
            if (whole_value) {
                j_ws(c);
                if (c.p < c.e) c.bad = true;
            }
            break;
        }
        if (!first && !j_eat(c, ',')) {
            c.bad = true;
            break;
        }
        first = false;
        j_ws(c);
        const char *kp = c.p + 1;
        const uint64_t h = j_string_hash(c);
        const int klen = (int)(c.p - kp) - 1;
        if (c.bad || !j_eat(c, ':')) {
            c.bad = true;
            break;
        }
        member(h, klen, kp);
    }
}

// ---- InstanceRecord: its slots, the name of each, the row they make -------------------------------------------------------------

enum PodSlot { kPodLruTime, kPodCount, kPodCap, kPodUsed, kPodLThreads, kPodLInProg, kPodRpm, kPodShutdown, kPodStartTime, kPodVers, kPodSlots };

// the slot of a field name, -1 for loc, zone (interned on the host), labels (ingest_pod_labels_kernel) and anything newer
template <class B>
__device__ __forceinline__ int pod_slot_of(uint64_t h, int klen, const B *kp)
{
    if (KEY_IS(h, klen, kp, "lruTime")) return kPodLruTime;
    if (KEY_IS(h, klen, kp, "count")) return kPodCount;
    if (KEY_IS(h, klen, kp, "cap")) return kPodCap;
    if (KEY_IS(h, klen, kp, "used")) return kPodUsed;
    if (KEY_IS(h, klen, kp, "lThreads")) return kPodLThreads;
    if (KEY_IS(h, klen, kp, "lInProg")) return kPodLInProg;
    if (KEY_IS(h, klen, kp, "rpm")) return kPodRpm;
    if (KEY_IS(h, klen, kp, "shutdown")) return kPodShutdown;
    if (KEY_IS(h, klen, kp, "startTime")) return kPodStartTime;
    if (KEY_IS(h, klen, kp, "vers")) return kPodVers;
    return -1;
}

// `r` arrives with id_order / replica_set / flags(LIVE) set by the host; every numeric field is (re)written from the slots
__device__ __forceinline__ void pod_row_from_slots(mmp_pod_row &r, const int64_t *fv, int64_t &start_time)
{
    r.lru_time = fv[kPodLruTime];
    r.count = (int32_t)fv[kPodCount];
    r.capacity = fv[kPodCap];
    r.used = fv[kPodUsed];
    r.loading_threads = (int32_t)fv[kPodLThreads];
    r.loading_in_progress = (int32_t)fv[kPodLInProg];
    r.rpm = (int32_t)fv[kPodRpm];
    r.flags = fv[kPodShutdown] ? (r.flags | MMP_POD_SHUTTING_DOWN) : (r.flags & ~MMP_POD_SHUTTING_DOWN);
    r.version = fv[kPodVers];
    start_time = fv[kPodStartTime];
}

// One InstanceRecord value walked by ONE lane (longer than the LDS tile of the wave path) into the cleared slots fv[]: a later
// duplicate wins by program order.  Returns true when the value is malformed.
__device__ __forceinline__ bool pod_record_serial(const char *b, const char *e, int64_t *fv)
{
    JCur c{b, e, false};
    j_members(c, true, [&](uint64_t h, int klen, const char *kp) {
        const int s = pod_slot_of(h, klen, kp);
        if (s < 0)
            j_skip_value(c);
        else
            fv[s] = s == kPodShutdown ? (int64_t)j_bool(c) : j_int(c);
    });
    return c.bad;
}

// open-addressing table of 64-bit string hashes -> small int (instance id -> pod, type name -> type)
struct HashTab {
    const uint64_t *hash;
    const int32_t *val;
    uint32_t mask;  // capacity - 1 (power of two); 0 with hash == nullptr means "empty table"
};

// where the probe sequence of hash h starts (the host's build_hash_table and the device's inserts start there too)
__host__ __device__ constexpr uint32_t tab_home(uint64_t h, uint32_t mask) { return (uint32_t)(h ^ (h >> 32)) & mask; }

__device__ __forceinline__ int32_t tab_find(const HashTab &t, uint64_t h, int32_t missing)
{
    if (!t.hash) return missing;
    uint32_t s = tab_home(h, t.mask);
    for (uint32_t probe = 0; probe <= t.mask; probe++) {
        const int32_t v = t.val[s];
        if (v == INT32_MIN) return missing;  // empty slot
        if (t.hash[s] == h) return v;
        s = (s + 1) & t.mask;
    }
    return missing;
}

// The label names of mmp_label_names_load: name i owns bit i of a label word.  `tab` maps the masked hash of a name to i and,
// unlike the id tables, may hold EQUAL hashes (MMP_LABEL_HASH_BITS masks them down to provoke that): a probe goes on past an
// entry whose bytes differ.  At most 64 names in a table of >= 128 slots, so every probe sequence meets an empty slot.
struct LabelTab {
    HashTab tab;
    const int32_t *name_off;  // name i = arena[name_off[i], name_off[i + 1])
    const char *arena;
    uint64_t hmask;  // the hash bits that count
};

// the bit of the label whose raw bytes are p[0, len) with FNV-1a hash h; -1 for a label no type can name
template <class B>
__device__ __forceinline__ int32_t label_find(const LabelTab &T, uint64_t h, int len, const B *p)
{
    h &= T.hmask;
    uint32_t s = tab_home(h, T.tab.mask);
    for (uint32_t probe = 0; probe <= T.tab.mask; probe++) {
        const int32_t v = T.tab.val[s];
        if (v == INT32_MIN) return -1;  // empty slot
        if (T.tab.hash[s] == h) {       // hash first, then the length, then the bytes
            const int32_t o = T.name_off[v];
            if (T.name_off[v + 1] - o == len && bytes_equal(p, T.arena + o, len)) return v;
        }
        s = (s + 1) & T.tab.mask;
    }
    return -1;
}

// At the value of a `labels` member (InstanceRecord.java:68-92: a String[], null and [] alike NO_LABELS), the serial statement
// of what the element round of ingest_pod_labels_kernel checks on the tile: `null`, or '[', strings separated by exactly one
// ',', ']'.  word = the bits of the known labels (T == nullptr: the grammar alone), count = the elements, unknown and repeated
// ones included.  A string is matched by its raw bytes, so one that holds a backslash escape matches no name.
__device__ __forceinline__ void j_labels(JCur &c, const LabelTab *T, uint64_t &word, int32_t &count)
{
    word = 0;
    count = 0;
    j_ws(c);
    if (j_lit(c, "null", 4)) return;
    if (!j_eat(c, '[')) {
        c.bad = true;
        return;
    }
    if (j_eat(c, ']')) return;
    for (;;) {
        j_ws(c);
        const char *kp = c.p + 1;
        const uint64_t h = j_string_hash(c);
        if (c.bad) return;
        const int32_t b = T ? label_find(*T, h, (int)(c.p - kp) - 1, kp) : -1;
        if (b >= 0) word |= 1ull << b;
        count++;
        if (j_eat(c, ',')) continue;
        if (!j_eat(c, ']')) c.bad = true;
        return;
    }
}

// at an id -> long map (instanceIds / failedIn; Jackson writes a null map as `null`): count the entries, and when
// out_pod != nullptr write them in document order (a TreeMap serialises in key order, which is what the paths expect)
__device__ __forceinline__ int32_t j_id_map(JCur &c, const HashTab &ids, int32_t *out_pod, int64_t *out_time)
{
    int32_t n = 0;
    j_ws(c);
    if (j_lit(c, "null", 4)) return 0;
    j_members(c, false, [&](uint64_t h, int, const char *) {
        const int64_t t = j_int(c);
        if (out_pod) {
            out_pod[n] = tab_find(ids, h, -1);
            out_time[n] = t;
        }
        n++;
    });
    return n;
}

// The parking rule.  The shortest map entry is `"":1,` — an empty key is a key — so n entries of one record take at least
// 5n + 1 bytes of its JSON (5n - 1 for the entries, the map's braces), and record i may park its entries at slot
// off[i] / kJEntryBytes + e: off[i + 1] >= off[i] + 5n + 1 puts the next record's first slot behind them, and the last
// record's behind bytes / kJEntryBytes.  The host sizes the parking arrays as bytes / kJEntryBytes + 2 (mmplace.hip).  The
// wave path refuses a map whose separators announce more entries than its bytes can hold BEFORE any entry is parked: the
// entry lanes write independently, and a lane with a well-formed entry behind malformed two-byte ones would otherwise park
// it beyond the record's slots.
constexpr int kJEntryBytes = 5;

struct IngestModelsArgs {
    const char *buf;
    const int64_t *off;
    int32_t n;
    HashTab ids, types;
    int32_t unknown_type;  // index for a type name that is not in the table
    int32_t default_type;  // index of ModelRecord.DEFAULT_TYPE ("NLCLASSIFIER", ModelRecord.java:133)
    mmp_model_row *rows;   // type / n_loaded / n_failed / last_used (ent_off: compact_entries_kernel)
    int64_t *last_unload;
    int32_t *status;
    int32_t *cnt;          // n_loaded + n_failed per record (scanned into the CSR offsets)
    int32_t *ent_pod;      // entries of record i are parked at slot off[i] / kJEntryBytes (so the slots of consecutive
    int64_t *ent_time;     // records never overlap) until the offsets are known
    int32_t grp;           // records per wavefront (1..kJGroup)
    // mmp_models_upsert_json (all three NULL for the full reload, where record i IS row i): the records are EVENTS, rows / cnt /
    // last_unload / status are per-event scratch, and event i belongs to the registry row in slot[i] of the call's distinct rows.
    const uint8_t *deleted;  // event i is ENTRY_DELETED: its value is not read, it leaves the empty row and counts as well-formed
    const int32_t *slot;
    int32_t *win;            // per slot: the last event that is well-formed or deleted (-1 before the launch; atomicMax)
};

// ---- ModelRecord: its slots and the name of each ---------------------------------------------------------------------------------
//
// The two maps take three slots each: the entry count, and on the tile the positions of the map's opener and closer (0 = no
// map yet, -1 = null).
enum ModelSlot { kModType, kModLu, kModLul, kModLoaded, kModFailed, kModLoadedOpen, kModLoadedClose, kModFailedOpen, kModFailedClose, kModSlots };
// map m (0 instanceIds, 1 failedIn): its count in slot kModLoaded + m, its opener in slot j_map_open(m), its closer in the next
__device__ __forceinline__ int j_map_open(int m) { return kModLoadedOpen + 2 * m; }
static_assert(kModFailed == kModLoaded + 1 && kModLoadedClose == kModLoadedOpen + 1 && kModFailedOpen == kModLoadedOpen + 2 &&
                  kModFailedClose == kModFailedOpen + 1, "the slots of the two maps are laid out alike");

// the slot of a field name (kModType .. kModFailed), -1 for every other field
template <class B>
__device__ __forceinline__ int model_slot_of(uint64_t h, int klen, const B *kp)
{
    if (KEY_IS(h, klen, kp, "type")) return kModType;
    if (KEY_IS(h, klen, kp, "lu")) return kModLu;
    if (KEY_IS(h, klen, kp, "lul")) return kModLul;
    if (KEY_IS(h, klen, kp, "instanceIds")) return kModLoaded;
    if (KEY_IS(h, klen, kp, "failedIn")) return kModFailed;
    return -1;
}

// One ModelRecord value walked by ONE lane into the slots fv[] / win[] (cleared, fv[kModType] = the default type).  PASS 0: type,
// lu, lul, the maps' counts, and in win[] the index of the field that set each map's count (the last duplicate: the one that
// wins); PASS 1: the entries, of those two fields only, parked from slot `park` on — an earlier duplicate is walked but not
// written, so the row holds exactly the winner's entries, as on the wave path.
template <int PASS>
__device__ __forceinline__ bool model_record_serial(const IngestModelsArgs &A, const char *b, const char *e, int64_t *fv,
                                                    int32_t *win, int64_t park)
{
    JCur c{b, e, false};
    int32_t f = -1;  // index of the field being read
    j_members(c, true, [&](uint64_t h, int klen, const char *kp) {
        f++;
        const int s = model_slot_of(h, klen, kp);
        if (s >= kModLoaded) {
            const bool wr = PASS && f == win[s];
            const int64_t at = park + (s == kModFailed ? fv[kModLoaded] : 0);
            const int32_t k = j_id_map(c, A.ids, wr ? A.ent_pod + at : nullptr, wr ? A.ent_time + at : nullptr);
            if (PASS == 0) {
                fv[s] = k;
                win[s] = f;
            }
        } else if (PASS == 0 && s == kModType) {
            j_ws(c);
            if (c.p < c.e && *c.p == '"')
                fv[s] = tab_find(A.types, j_string_hash(c), A.unknown_type);
            else {  // null -> DEFAULT_TYPE (ModelRecord.java:121), also behind an earlier duplicate that named a type
                // (exactly `null`, as on the wave path; anything else that is not a string is skipped)
                JCur v = c;
                if (j_lit(v, "null", 4) && (v.p == v.e || *v.p == ',' || *v.p == '}' || j_is_ws(*v.p))) fv[s] = A.default_type;
                j_skip_value(c);
            }
        } else if (PASS == 0 && s >= 0)
            fv[s] = j_int(c);  // lu, lul
        else
            j_skip_value(c);
    });
    return c.bad;
}

// ---- the wave path ----------------------------------------------------------------------------------------
//
// A wavefront takes up to kJGroup consecutive records.  Their bytes are contiguous in the value buffer, so the
// whole group is staged into an LDS tile with coalesced dword loads.  Then, per record, j_scan classifies
// the bytes 64 at a time, one byte per lane, with ballots (the masks are wave-uniform 64-bit scalars):
//   unescaped quotes   = '"' & ~escaped, `escaped` from the odd-length-backslash-run carry arithmetic
//   string interiors   = prefix-xor of the unescaped quotes (carried across chunks)
//   nesting depth      = running popcount(open) - popcount(close) over the structural characters
// and keeps, per chunk, the ':' and ',' masks of the two levels the beans use (fields of the record;
// entries of the id -> time maps) plus the closers of level-2 containers.  After that the FIELDS of all
// records of the group are spread over the lanes — the k-th set bit of a record's ':' mask is its k-th
// field, the key is the string that ends before it, the value starts after it — and, for ModelRecords,
// the map ENTRIES of all records are spread over the lanes the same way.  (One lane per field of ONE record
// was measured first: 0.29 ms per pass over 100k ModelRecords, VALU-issue bound with ~6 of 64 lanes busy.)
constexpr int kJWaves = 4;           // wavefronts per workgroup
constexpr int kJGroup = 8;           // records per wavefront
constexpr int kJTileBytes = 2048;    // LDS tile of one wavefront; a record longer than this: serial path
constexpr int kJTileChunks = kJTileBytes / 64 + kJGroup;
constexpr int kJBlock = kJWaves * 64;
constexpr int kJSlots = 10;          // slots per record
static_assert(kPodSlots <= kJSlots && kModSlots <= kJSlots, "JWaveLds::val / win hold every slot of either record type");

struct JRecInfo {  // one record of the tile
    int32_t base;  // first byte inside the tile
    int32_t L, nch;
    int32_t mb;    // first mask word
    int32_t f, g;  // first / last non-whitespace byte: the record's '{' and '}'
    int32_t n1;    // level-1 ':' = fields
    int32_t bad;
};

struct __attribute__((aligned(16))) JWaveLds {
    uint32_t dw[kJTileBytes / 4 + 4];  // the group's bytes, dword-staged from the aligned address below them
    uint64_t rq[kJTileChunks];         // unescaped '"'
    uint64_t c1[kJTileChunks];         // ':' outside strings, directly inside the record object
    uint64_t c2[kJTileChunks];         // ':' one level down (entries of instanceIds / failedIn / fails)
    uint64_t m1[kJTileChunks];         // ',' at those two levels
    uint64_t m2[kJTileChunks];
    uint64_t e2[kJTileChunks];         // closers of containers opened directly inside the record object
    JRecInfo rec[kJGroup];
    int32_t pf[kJGroup + 1];           // prefix sums of the per-record item counts (fields, then entries)
    int64_t val[kJGroup][kJSlots];     // value of each known field ...
    int32_t win[kJGroup][kJSlots];     // ... and the index of the field it came from (a later duplicate wins)
    int64_t off[kJGroup + 1];          // byte offsets of the wavefront's records
};

struct JView {  // what a lane needs to work on one record
    const uint8_t *by;
    const uint64_t *rq, *c1, *c2, *m1, *m2, *e2;
    int L, nch, f, g, n1;
};

__device__ __forceinline__ JView j_view(const JWaveLds &S, int r)
{
    const JRecInfo I = S.rec[r];
    JView V;
    V.by = reinterpret_cast<const uint8_t *>(S.dw) + I.base;
    V.rq = S.rq + I.mb;
    V.c1 = S.c1 + I.mb;
    V.c2 = S.c2 + I.mb;
    V.m1 = S.m1 + I.mb;
    V.m2 = S.m2 + I.mb;
    V.e2 = S.e2 + I.mb;
    V.L = I.L;
    V.nch = I.nch;
    V.f = I.f;
    V.g = I.g;
    V.n1 = I.n1;
    return V;
}

__device__ __forceinline__ uint64_t j_prefix_xor(uint64_t x)
{
    x ^= x << 1;
    x ^= x << 2;
    x ^= x << 4;
    x ^= x << 8;
    x ^= x << 16;
    x ^= x << 32;
    return x;
}

// Characters escaped by a backslash.  Runs of backslashes: a run that starts on an odd bit is told apart
// from one that starts on an even bit by letting an addition carry through the run (the usual
// bit-parallel formulation); `carry` = the first byte of the next chunk is escaped.
__device__ __forceinline__ uint64_t j_escaped(uint64_t backslash, uint64_t &carry)
{
    backslash &= ~carry;
    const uint64_t follows = (backslash << 1) | carry;
    const uint64_t even = 0x5555555555555555ull;
    const uint64_t odd_starts = backslash & ~even & ~follows;
    const uint64_t sum = odd_starts + backslash;
    carry = sum < odd_starts ? 1ull : 0ull;
    return (even ^ (sum << 1)) & follows;
}

// Classify the record at tile bytes [base, base + L): whole wavefront, one byte per lane per step.
__device__ __forceinline__ JRecInfo j_scan(JWaveLds &S, int base, int L, int mb)
{
    const int lane = lane_id();
    const uint8_t *by = reinterpret_cast<const uint8_t *>(S.dw) + base;
    JRecInfo R;
    R.base = base;
    R.L = L;
    R.nch = (L + 63) >> 6;
    R.mb = mb;
    uint64_t esc_carry = 0, in_str = 0;
    int depth = 0, zero_pos = kNoPos, nm1 = 0, n_nonws = 0;
    R.f = kNoPos;
    R.g = -1;
    R.n1 = 0;
    const uint64_t lt = (1ull << lane) - 1ull;
    for (int c = 0; c < R.nch; c++) {
        const int idx = c * 64 + lane;
        const uint32_t B = idx < L ? by[idx] : (uint32_t)' ';
        const uint64_t bs = __ballot(B == '\\');
        const uint64_t esc = (bs | esc_carry) ? j_escaped(bs, esc_carry) : 0ull;
        const uint64_t rq = __ballot(B == '"') & ~esc;
        const uint64_t ins = j_prefix_xor(rq) ^ in_str;  // opening quote .. byte before the closing quote
        in_str = (uint64_t)((int64_t)ins >> 63);
        const uint64_t op = __ballot(B == '{' || B == '[') & ~ins;
        const uint64_t cl = __ballot(B == '}' || B == ']') & ~ins;
        const uint64_t co = __ballot(B == ':') & ~ins;
        const uint64_t cm = __ballot(B == ',') & ~ins;
        const uint64_t nonws = ~__ballot(j_is_ws(B));
        const int d_before = depth + __popcll((unsigned long long)(op & lt)) - __popcll((unsigned long long)(cl & lt));
        const uint64_t at1 = __ballot(d_before == 1), at2 = __ballot(d_before == 2);
        const uint64_t z = cl & __ballot(d_before <= 1);  // closers that bring the depth to <= 0
        if (z && zero_pos == kNoPos) zero_pos = c * 64 + (__ffsll((unsigned long long)z) - 1);
        if (nonws) {
            if (R.f == kNoPos) R.f = c * 64 + (__ffsll((unsigned long long)nonws) - 1);
            R.g = c * 64 + 63 - __clzll((unsigned long long)nonws);
            n_nonws += __popcll((unsigned long long)nonws);
        }
        if (lane == 0) {
            S.rq[mb + c] = rq;
            S.c1[mb + c] = co & at1;
            S.c2[mb + c] = co & at2;
            S.m1[mb + c] = cm & at1;
            S.m2[mb + c] = cm & at2;
            S.e2[mb + c] = cl & at2;
        }
        R.n1 += __popcll((unsigned long long)(co & at1));
        nm1 += __popcll((unsigned long long)(cm & at1));
        depth += __popcll((unsigned long long)op) - __popcll((unsigned long long)cl);
    }
    // one object, closed exactly by the last non-blank byte, nothing open at the end, fields separated by
    // exactly one ',' each, and "{}" holds nothing but blanks
    const bool bad = R.f == kNoPos || by[R.f] != '{' || zero_pos != R.g || by[R.g] != '}' || depth != 0 || in_str != 0 ||
                     nm1 != (R.n1 > 0 ? R.n1 - 1 : 0) || (R.n1 == 0 && n_nonws != 2);
    R.bad = bad ? 1 : 0;
    return R;
}

__device__ __forceinline__ bool j_bit(const uint64_t *m, int pos) { return (m[pos >> 6] >> (pos & 63)) & 1ull; }

// position of the k-th (0-based) set bit at a position > after; -1 if there is none
__device__ __forceinline__ int j_nth_after(const uint64_t *m, int nch, int after, int k)
{
    int w = (after + 1) >> 6;
    if (w >= nch) return -1;
    uint64_t v = m[w] & (~0ull << ((after + 1) & 63));
    for (;;) {
        const int c = __popcll((unsigned long long)v);
        if (k < c) return w * 64 + select_kth_bit(v, k);
        k -= c;
        if (++w >= nch) return -1;
        v = m[w];
    }
}

// highest set bit at a position < before; -1 if there is none
__device__ __forceinline__ int j_prev(const uint64_t *m, int before)
{
    if (before <= 0) return -1;
    int w = (before - 1) >> 6;
    const int hb = (before - 1) & 63;
    uint64_t v = m[w];
    if (hb != 63) v &= (1ull << (hb + 1)) - 1ull;
    for (;;) {
        if (v) return w * 64 + 63 - __clzll((unsigned long long)v);
        if (--w < 0) return -1;
        v = m[w];
    }
}

// set bits at positions in (lo, hi)
__device__ __forceinline__ int j_count(const uint64_t *m, int lo, int hi)
{
    if (hi - lo < 2) return 0;
    const int a = lo + 1, b = hi - 1, wa = a >> 6, wb = b >> 6;
    int n = 0;
    for (int w = wa; w <= wb; w++) {
        uint64_t v = m[w];
        if (w == wa) v &= ~0ull << (a & 63);
        if (w == wb && (b & 63) != 63) v &= (1ull << ((b & 63) + 1)) - 1ull;
        n += __popcll((unsigned long long)v);
    }
    return n;
}

// The key of the ':' at p — FNV-1a of the raw bytes between its quotes — and the separator before it:
// the container's opener for the first member, a ',' of this level (`commas`) otherwise.
__device__ __forceinline__ bool j_key(const JView &R, int p, const uint64_t *commas, int open_pos, bool first,
                                      uint64_t &h, int &klen, const uint8_t *&kp)
{
    int q = p - 1;
    while (q >= 0 && j_is_ws(R.by[q])) q--;
    if (q < 0 || !j_bit(R.rq, q)) return false;  // not a string
    const int ks = j_prev(R.rq, q);
    if (ks < 0) return false;
    int sp = ks - 1;
    while (sp >= 0 && j_is_ws(R.by[sp])) sp--;
    if (sp < 0 || (first ? sp != open_pos : !j_bit(commas, sp))) return false;
    klen = q - ks - 1;
    kp = R.by + ks + 1;
    h = fnv1a(kp, klen);
    return true;
}

// after a value that ended before byte p: a ',' of this level, or the container's closer after the last member
__device__ __forceinline__ bool j_term(const JView &R, int p, const uint64_t *commas, int close_pos, bool last)
{
    while (p < R.L && j_is_ws(R.by[p])) p++;
    if (p >= R.L) return false;
    return last ? p == close_pos : j_bit(commas, p);
}

__device__ __forceinline__ bool j_int_at(const JView &R, int &p, int64_t &out)
{
    bool neg = false;
    if (p < R.L && R.by[p] == '-') {
        neg = true;
        p++;
    }
    if (p >= R.L || R.by[p] < '0' || R.by[p] > '9') return false;
    uint64_t v = 0;
    while (p < R.L && R.by[p] >= '0' && R.by[p] <= '9') {
        v = v * 10u + (uint64_t)(R.by[p] - '0');
        p++;
    }
    out = neg ? (int64_t)(0 - v) : (int64_t)v;
    return true;  // j_term rejects a fraction / exponent / junk behind the digits
}

__device__ __forceinline__ bool j_lit_at(const JView &R, int p, const char *lit, int n)
{
    return p + n <= R.L && bytes_equal(R.by + p, lit, n);
}

// The byte offsets of the wavefront's records, fetched with one load (S.off[k] = off[i0 + k]).
__device__ __forceinline__ void j_load_offsets(const int64_t *off, int i0, int i1, JWaveLds &S)
{
    const int lane = lane_id();
    if (lane <= i1 - i0) S.off[lane] = off[i0 + lane];
    wave_sync();
}

// How many of the records [k, k1) of the wavefront fit one tile together (0: the first alone is too long).
__device__ __forceinline__ int j_group_len(const JWaveLds &S, int k, int k1)
{
    const int64_t b0 = S.off[k];
    int c = 0;
    while (k + c < k1 && S.off[k + c + 1] - b0 <= kJTileBytes) c++;
    return c;
}

// the slots of records [0, cnt) of the tile: no value, no field that set one
__device__ __forceinline__ void j_clear_slots(JWaveLds &S, int cnt)
{
    for (int q = lane_id(); q < cnt * kJSlots; q += 64) {
        (&S.val[0][0])[q] = 0;
        (&S.win[0][0])[q] = -1;
    }
    wave_sync();
}

// Stage records [k, k+cnt) of the wavefront into the tile and scan them; fills S.rec[0..cnt).
__device__ __forceinline__ void j_stage_and_scan(const char *buf, int k, int cnt, JWaveLds &S)
{
    const int lane = lane_id();
    const int64_t *off = S.off + k;
    const int64_t b0 = off[0], a0 = b0 & ~3ll;  // the buffer is device-allocated (256-byte aligned)
    const int shift = (int)(b0 - a0);
    const int ndw = (shift + (int)(off[cnt] - b0) + 3) >> 2;
    const uint32_t *g32 = reinterpret_cast<const uint32_t *>(buf + a0);
    for (int q = lane; q < ndw; q += 64) S.dw[q] = g32[q];
    wave_sync();
    int mb = 0;
    for (int r = 0; r < cnt; r++) {
        const JRecInfo R = j_scan(S, shift + (int)(off[r] - b0), (int)(off[r + 1] - off[r]), mb);
        if (lane == 0) S.rec[r] = R;
        mb += R.nch;
    }
    j_clear_slots(S, cnt);
}

// pf[0..cnt] = exclusive prefix sums of the per-record item counts held by lanes 0..cnt-1; returns the total
__device__ __forceinline__ int j_prefix_items(JWaveLds &S, int cnt, int mine)
{
    const int lane = lane_id();
    const int incl = wave_incl_scan_i32(lane < cnt ? mine : 0);
    if (lane < cnt) S.pf[lane + 1] = incl;
    if (lane == 0) S.pf[0] = 0;
    wave_sync();
    return S.pf[cnt];
}

// item t -> (record, index inside the record)
__device__ __forceinline__ int j_item_record(const JWaveLds &S, int cnt, int t, int &k)
{
    int r = 0;
#pragma unroll
    for (int q = 1; q < kJGroup; q++)
        if (q < cnt && t >= S.pf[q]) r = q;
    k = t - S.pf[r];
    return r;
}

// the group's fields as items: records the scan rejected have none
__device__ __forceinline__ int j_prefix_fields(JWaveLds &S, int cnt)
{
    const int lane = lane_id();
    return j_prefix_items(S, cnt, lane < cnt && !S.rec[lane].bad ? S.rec[lane].n1 : 0);
}

// Member k of the container opened at byte `open` of the record, `colons` / `commas` being the masks of its level.
struct JMember {
    uint64_t h;  // the key: FNV-1a, length, first byte
    int klen;
    const uint8_t *kp;
    int p, v;    // the ':' and the first byte of the value
};

__device__ __forceinline__ bool j_member_at(const JView &R, const uint64_t *colons, const uint64_t *commas, int open, int k, JMember &M)
{
    M.p = j_nth_after(colons, R.nch, open, k);
    if (M.p < 0 || !j_key(R, M.p, commas, open, k == 0, M.h, M.klen, M.kp)) return false;
    M.v = M.p + 1;
    while (M.v < R.L && j_is_ws(R.by[M.v])) M.v++;
    return true;
}

// The head of a field round: item t of the group's fields is field j of record r (the j-th ':' directly inside the record object).
struct JField {
    int r, j;
    bool last;  // the record's last field: its value ends at the closing brace, not at a ','
    JMember m;
};

__device__ __forceinline__ bool j_field_at(const JWaveLds &S, int cnt, int t, JView &R, JField &F)
{
    F.r = j_item_record(S, cnt, t, F.j);
    R = j_view(S, F.r);
    F.last = F.j == R.n1 - 1;
    return j_member_at(R, R.c1, R.m1, R.f, F.j, F.m);
}

// The claims of a field round, by every lane of the wavefront: a malformed field rejects its record; the value of a known field
// (fid >= 0) claims the slot, where the field with the highest index wins (Jackson keeps the last duplicate).  True for a lane
// that claimed: once this returns S.win[r][fid] == j tells it whether it won.  The caller stores what the winners hold and ends
// the round with a wave_sync.
__device__ __forceinline__ bool j_claim(JWaveLds &S, const JField &F, int fid, bool lbad)
{
    if (lbad) S.rec[F.r].bad = 1;
    const bool claims = fid >= 0 && !lbad;
    if (claims) atomicMax(&S.win[F.r][fid], F.j);
    wave_sync();
    return claims;
}

// The frame of both kernels, by every wavefront: grp consecutive records, taken in groups that fit the LDS tile together.
// tile(S, k, cnt) parses the staged and scanned records [k, k + cnt) of the wavefront, every lane at work; a record longer than
// the tile is a group of one that lane 0 walks: walk(S, i, b, e) -> malformed.  Both leave the values in S.val and the verdict
// in S.rec[].bad, and publish(i, bad, fv) writes record i from its slots.
template <class Walk, class Tile, class Publish>
__device__ __forceinline__ void j_ingest_wave(JWaveLds *lds, const char *buf, const int64_t *off, int32_t n, int32_t grp, Walk &&walk,
                                              Tile &&tile, Publish &&publish)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = lane_id();
    JWaveLds &S = lds[wave];
    const int i0 = (blockIdx.x * kJWaves + wave) * grp;
    if (i0 >= n) return;
    const int i1 = i0 + grp < n ? i0 + grp : n;
    j_load_offsets(off, i0, i1, S);
    int i = i0;
    while (i < i1) {
        const int k = i - i0;
        int cnt = j_group_len(S, k, i1 - i0);
        if (cnt == 0) {
            j_clear_slots(S, cnt = 1);
            if (lane == 0) S.rec[0].bad = walk(S, i, buf + S.off[k], buf + S.off[k + 1]) ? 1 : 0;
            wave_sync();
        } else {
            j_stage_and_scan(buf, k, cnt, S);
            tile(S, k, cnt);
        }
        if (lane < cnt) publish(i + lane, S.rec[lane].bad != 0, S.val[lane]);
        wave_sync();
        i += cnt;
    }
}

// InstanceRecord values, grp per WAVEFRONT.
__global__ __launch_bounds__(kJBlock) void ingest_pods_kernel(const char *__restrict__ buf, const int64_t *__restrict__ off,
                                                              int32_t n, int32_t grp, mmp_pod_row *__restrict__ rows,
                                                              int64_t *__restrict__ start_time, int32_t *__restrict__ status)
{
    __shared__ JWaveLds lds[kJWaves];
    const int lane = lane_id();
    j_ingest_wave(
        lds, buf, off, n, grp, [&](JWaveLds &S, int, const char *b, const char *e) { return pod_record_serial(b, e, S.val[0]); },
        [&](JWaveLds &S, int, int cnt) {  // every field of every record of the group on its own lane
            const int total = j_prefix_fields(S, cnt);
            for (int base = 0; base < total; base += 64) {
                JField F{};
                int fid = -1;
                int64_t val = 0;
                bool lbad = false;
                if (base + lane < total) {
                    JView R;
                    lbad = !j_field_at(S, cnt, base + lane, R, F);
                    if (!lbad && (fid = pod_slot_of(F.m.h, F.m.klen, F.m.kp)) >= 0) {
                        int v = F.m.v;
                        if (fid == kPodShutdown) {
                            if (j_lit_at(R, v, "true", 4)) {
                                val = 1;
                                v += 4;
                            } else if (j_lit_at(R, v, "false", 5))
                                v += 5;
                            else
                                lbad = true;
                        } else if (!j_int_at(R, v, val))
                            lbad = true;
                        if (!lbad && !j_term(R, v, R.m1, R.g, F.last)) lbad = true;
                    }
                }
                if (j_claim(S, F, fid, lbad) && S.win[F.r][fid] == F.j) S.val[F.r][fid] = val;
                wave_sync();
            }
        },
        [&](int i, bool bad, const int64_t *fv) {
            status[i] = bad ? 1 : 0;
            if (!bad) {
                mmp_pod_row r = rows[i];
                pod_row_from_slots(r, fv, start_time[i]);
                rows[i] = r;
            }
        });
}

// The `labels` of InstanceRecord values, grp per WAVEFRONT: a second launch over the values ingest_pods_kernel has parsed, made
// only while label names are loaded (ingest_pods_kernel has no slot left, and one more would change the LDS layout of both record
// types).  word[i] / count[i] = the known-label bits and the element count of the LAST `labels` member of value i (absent, null
// and [] alike 0 / 0); status[i] = 1 when the value is malformed as a whole or ANY of its `labels` members is not null or an
// array of strings, which the host ORs into the parser's status.
enum LabelSlot { kLabWord, kLabCount, kLabOpen, kLabClose, kLabSlots };  // kLabOpen / kLabClose: the winning array's brackets on the tile
static_assert(kLabSlots <= kJSlots, "JWaveLds::val / win hold every slot");

__global__ __launch_bounds__(kJBlock) void ingest_pod_labels_kernel(const char *__restrict__ buf, const int64_t *__restrict__ off,
                                                                    int32_t n, int32_t grp, LabelTab T, uint64_t *__restrict__ word,
                                                                    int32_t *__restrict__ count, int32_t *__restrict__ status)
{
    __shared__ JWaveLds lds[kJWaves];
    const int lane = lane_id();
    j_ingest_wave(
        lds, buf, off, n, grp,
        [&](JWaveLds &S, int, const char *b, const char *e) {  // a later duplicate wins by program order
            JCur c{b, e, false};
            j_members(c, true, [&](uint64_t h, int klen, const char *kp) {
                if (KEY_IS(h, klen, kp, "labels")) {
                    uint64_t w;
                    int32_t k;
                    j_labels(c, &T, w, k);
                    S.val[0][kLabWord] = (int64_t)w;
                    S.val[0][kLabCount] = k;
                } else
                    j_skip_value(c);
            });
            return c.bad;
        },
        [&](JWaveLds &S, int, int cnt) {
            // the `labels` members of every record of the group: the last one claims kLabCount and leaves its brackets
            int total = j_prefix_fields(S, cnt);
            for (int base = 0; base < total; base += 64) {
                JField F{};
                int fid = -1;
                int64_t val = 0;
                int vopen = -1, vclose = -1;
                bool lbad = false;
                if (base + lane < total) {
                    JView R;
                    if (!j_field_at(S, cnt, base + lane, R, F))
                        lbad = true;
                    else if (KEY_IS(F.m.h, F.m.klen, F.m.kp, "labels")) {
                        fid = kLabCount;
                        const int v = F.m.v;
                        if (j_lit_at(R, v, "null", 4)) {
                            if (!j_term(R, v + 4, R.m1, R.g, F.last)) lbad = true;
                        } else if (v < R.L && R.by[v] == '[') {
                            const int ce = j_nth_after(R.e2, R.nch, v, 0);
                            if (ce < 0 || R.by[ce] != ']')
                                lbad = true;
                            else {
                                vopen = v;
                                vclose = ce;
                                val = j_count(R.m2, v, ce) + 1;  // the elements are the m2 commas between the brackets, plus one
                                if (val == 1) {                  // ... unless nothing but blanks stands there
                                    int q = v + 1;
                                    while (q < ce && j_is_ws(R.by[q])) q++;
                                    if (q == ce) val = 0;
                                }
                                if (!j_term(R, ce + 1, R.m1, R.g, F.last)) lbad = true;
                            }
                        } else
                            lbad = true;
                    }
                }
                const int r = F.r;
                const bool claims = j_claim(S, F, fid, lbad);
                // An array that loses to a later duplicate is read by no element lane, so it is walked here, as the lost maps of
                // ingest_models_kernel are: one of THIS round that lost its claim walks itself, the winner of an EARLIER round
                // (its opener is > 0; -1 = null) is walked by the lane that replaces it.
                int lost_open = -1, lost_close = -1;
                if (claims) {
                    if (S.win[r][fid] == F.j) {
                        int64_t *fv = S.val[r];
                        if (fv[kLabOpen] > 0) {
                            lost_open = (int)fv[kLabOpen];
                            lost_close = (int)fv[kLabClose];
                        }
                        fv[kLabCount] = val;
                        fv[kLabOpen] = vopen;
                        fv[kLabClose] = vclose;
                    } else {
                        lost_open = vopen;
                        lost_close = vclose;
                    }
                }
                if (lost_open >= 0) {
                    const JView R = j_view(S, r);
                    JCur c{reinterpret_cast<const char *>(R.by) + lost_open, reinterpret_cast<const char *>(R.by) + lost_close + 1, false};
                    uint64_t w;
                    int32_t k;
                    j_labels(c, nullptr, w, k);
                    if (c.bad) S.rec[r].bad = 1;
                }
                wave_sync();
            }
            // the elements of the winning arrays of all records, one lane each: element e stands between separator e - 1 (the
            // opener for the first) and separator e (the closer for the last)
            total = j_prefix_items(S, cnt, lane < cnt && !S.rec[lane].bad ? (int)S.val[lane][kLabCount] : 0);
            for (int base = 0; base < total; base += 64) {
                const int t = base + lane;
                if (t < total) {
                    int e;
                    const int r = j_item_record(S, cnt, t, e);
                    const JView R = j_view(S, r);
                    const int64_t *fv = S.val[r];
                    const int open = (int)fv[kLabOpen], close = (int)fv[kLabClose], kcnt = (int)fv[kLabCount];
                    const int lo = e == 0 ? open : j_nth_after(R.m2, R.nch, open, e - 1);
                    const int hi = e == kcnt - 1 ? close : j_nth_after(R.m2, R.nch, open, e);
                    int p = lo + 1, q = -1;
                    while (p < hi && j_is_ws(R.by[p])) p++;
                    bool ok = lo >= 0 && p < hi && R.by[p] == '"';  // one string ...
                    if (ok) {
                        q = j_nth_after(R.rq, R.nch, p, 0);  // its closing quote
                        ok = q > p && q < hi;
                    }
                    if (ok) {  // ... with nothing but blanks behind it
                        int z = q + 1;
                        while (z < hi && j_is_ws(R.by[z])) z++;
                        ok = z == hi;
                    }
                    if (!ok)
                        S.rec[r].bad = 1;
                    else {
                        const int len = q - p - 1;
                        const int32_t b = label_find(T, fnv1a(R.by + p + 1, len), len, R.by + p + 1);
                        if (b >= 0) atomicOr(reinterpret_cast<unsigned long long *>(&S.val[r][kLabWord]), 1ull << b);
                    }
                }
            }
            wave_sync();
        },
        [&](int i, bool bad, const int64_t *fv) {
            status[i] = bad ? 1 : 0;
            word[i] = bad ? 0ull : (uint64_t)fv[kLabWord];
            count[i] = bad ? 0 : (int32_t)fv[kLabCount];
        });
}

// ModelRecord values, A.grp per WAVEFRONT, one pass: type / n_loaded / n_failed / last_used, the status
// (the whole value is validated, entries included) and the entries themselves, parked at slot
// off[i] / kJEntryBytes + e of ent_pod / ent_time until compact_entries_kernel moves them to their CSR position.
__global__ __launch_bounds__(kJBlock) void ingest_models_kernel(IngestModelsArgs A)
{
    __shared__ JWaveLds lds[kJWaves];
    const int lane = lane_id();
    j_ingest_wave(
        lds, A.buf, A.off, A.n, A.grp,
        [&](JWaveLds &S, int i, const char *b, const char *e) {  // a second walk writes the entries
            if (A.deleted && A.deleted[i]) return true;           // (a deleted event's value is not walked)
            S.val[0][kModType] = A.default_type;
            const int64_t park = (b - A.buf) / kJEntryBytes;
            if (model_record_serial<0>(A, b, e, S.val[0], S.win[0], park)) return true;
            (void)model_record_serial<1>(A, b, e, S.val[0], S.win[0], park);
            return false;
        },
        [&](JWaveLds &S, int k0, int cnt) {
            if (lane < cnt) S.val[lane][kModType] = A.default_type;
            wave_sync();
            int total = j_prefix_fields(S, cnt);
            for (int base = 0; base < total; base += 64) {
                JField F{};
                int fid = -1;
                int64_t val = 0;
                int vopen = -1, vclose = -1;
                bool lbad = false;
                if (base + lane < total) {
                    JView R;
                    if (!j_field_at(S, cnt, base + lane, R, F))
                        lbad = true;
                    else {
                        fid = model_slot_of(F.m.h, F.m.klen, F.m.kp);
                        int v = F.m.v;
                        const bool last = F.last;
                        if (fid == kModType) {
                            if (v < R.L && j_bit(R.rq, v)) {
                                const int ve = j_nth_after(R.rq, R.nch, v, 0);  // closing quote (strings are balanced)
                                val = tab_find(A.types, fnv1a(R.by + v + 1, ve - v - 1), A.unknown_type);
                                if (!j_term(R, ve + 1, R.m1, R.g, last)) lbad = true;
                            } else if (j_lit_at(R, v, "null", 4) && j_term(R, v + 4, R.m1, R.g, last)) {
                                val = A.default_type;  // null -> DEFAULT_TYPE (ModelRecord.java:121); claimed, so that it also
                                                       // wins over an earlier duplicate that named a type
                            } else {
                                fid = -1;  // not a string: the field is skipped
                            }
                        } else if (fid == kModLu || fid == kModLul) {
                            if (!j_int_at(R, v, val) || !j_term(R, v, R.m1, R.g, last)) lbad = true;
                        } else if (fid >= kModLoaded) {
                            if (j_lit_at(R, v, "null", 4)) {
                                if (!j_term(R, v + 4, R.m1, R.g, last)) lbad = true;
                            } else if (v < R.L && R.by[v] == '{') {
                                const int ce = j_nth_after(R.e2, R.nch, v, 0);
                                if (ce < 0 || R.by[ce] != '}')
                                    lbad = true;
                                else {
                                    vopen = v;
                                    vclose = ce;
                                    val = j_count(R.c2, v, ce);
                                    if (j_count(R.m2, v, ce) != (val > 0 ? val - 1 : 0)) lbad = true;
                                    if (val * kJEntryBytes > ce - v) lbad = true;  // more entries than bytes: see kJEntryBytes
                                    if (val == 0) {
                                        int q = v + 1;
                                        while (q < ce && j_is_ws(R.by[q])) q++;
                                        if (q != ce) lbad = true;
                                    }
                                    if (!j_term(R, ce + 1, R.m1, R.g, last)) lbad = true;
                                }
                            } else
                                lbad = true;
                        }
                    }
                }
                const int r = F.r;
                const bool claims = j_claim(S, F, fid, lbad);
                // A map that loses to a later duplicate is read by no entry lane, so it is walked here (the serial walk's map
                // grammar, nothing written): a malformed entry rejects the record wherever it stands.  S.win is final only for
                // the fields of the rounds run so far, so there are two kinds of loser: a map of THIS round that lost its claim
                // walks itself; a map that won an EARLIER round is still in S.val (its opener is > 0; 0 = none yet, -1 = null)
                // and is walked by the lane that now replaces it.
                int lost_open = -1, lost_close = -1;
                if (claims) {
                    if (S.win[r][fid] == F.j) {
                        S.val[r][fid] = val;
                        if (fid >= kModLoaded) {
                            int64_t *span = &S.val[r][j_map_open(fid - kModLoaded)];  // opener, closer
                            if (span[0] > 0) {
                                lost_open = (int)span[0];
                                lost_close = (int)span[1];
                            }
                            span[0] = vopen;
                            span[1] = vclose;
                        }
                    } else if (fid >= kModLoaded) {
                        lost_open = vopen;
                        lost_close = vclose;
                    }
                }
                if (lost_open >= 0) {
                    const JView R = j_view(S, r);
                    JCur c{reinterpret_cast<const char *>(R.by) + lost_open, reinterpret_cast<const char *>(R.by) + lost_close + 1, false};
                    (void)j_id_map(c, A.ids, nullptr, nullptr);
                    if (c.bad) S.rec[r].bad = 1;
                }
                wave_sync();
            }
            // the entries of both maps of every record, one lane each: instanceIds first, then failedIn (CSR layout)
            total = j_prefix_items(S, cnt, lane < cnt && !S.rec[lane].bad ? (int)(S.val[lane][kModLoaded] + S.val[lane][kModFailed]) : 0);
            for (int base = 0; base < total; base += 64) {
                const int t = base + lane;
                if (t < total) {
                    int e;
                    const int r = j_item_record(S, cnt, t, e);
                    const JView R = j_view(S, r);
                    const int64_t *fv = S.val[r];
                    const int nl = (int)fv[kModLoaded];
                    const int m = e < nl ? 0 : 1;  // which map
                    const int k = m ? e - nl : e, kcnt = (int)fv[kModLoaded + m];
                    const int open = (int)fv[j_map_open(m)], close = (int)fv[j_map_open(m) + 1];
                    JMember M;
                    int64_t tm = 0;
                    bool ok = j_member_at(R, R.c2, R.m2, open, k, M) && M.p <= close;
                    if (ok) {
                        int v = M.v;
                        ok = j_int_at(R, v, tm) && j_term(R, v, R.m2, close, k == kcnt - 1);
                    }
                    if (!ok)
                        S.rec[r].bad = 1;
                    else {
                        const int64_t slot = S.off[k0 + r] / kJEntryBytes + e;
                        A.ent_pod[slot] = tab_find(A.ids, M.h, -1);
                        A.ent_time[slot] = tm;
                    }
                }
            }
            wave_sync();
        },
        // What every route leaves for record i.  With the row indirection the event also stands for its row: events apply in
        // order and a malformed one changes nothing, so the row ends as its highest-numbered good event left it.
        [&](int i, bool bad, const int64_t *fv) {
            mmp_model_row r{};
            int64_t lul = 0;
            if (A.deleted && A.deleted[i])
                bad = false;  // ENTRY_DELETED: whatever the value, the empty row, and it counts as well-formed
            else if (bad)
                r.type = A.default_type;
            else {
                r.type = (int32_t)fv[kModType];
                r.n_loaded = (int32_t)fv[kModLoaded];
                r.n_failed = (int32_t)fv[kModFailed];
                r.last_used = fv[kModLu];
                lul = fv[kModLul];
            }
            A.status[i] = bad ? 1 : 0;
            A.rows[i] = r;
            A.cnt[i] = r.n_loaded + r.n_failed;
            A.last_unload[i] = lul;
            if (A.slot && !bad) atomicMax(&A.win[A.slot[i]], i);
        });
}

// offs = exclusive scan of cnt (rocPRIM): move every record's entries from their parking slots to
// [offs[i], offs[i] + cnt[i]) of the registry's entry arrays and publish ent_off.  One lane per record
// (a model has 1-3 copies).
__global__ void compact_entries_kernel(const int64_t *__restrict__ off, int32_t n, const int32_t *__restrict__ cnt,
                                       const int32_t *__restrict__ offs, const int32_t *__restrict__ tmp_pod,
                                       const int64_t *__restrict__ tmp_time, mmp_model_row *__restrict__ rows,
                                       int32_t *__restrict__ ent_pod, int64_t *__restrict__ ent_time)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t k = cnt[i], o = offs[i];
    const int64_t slot = off[i] / kJEntryBytes;
    rows[i].ent_off = o;
    for (int32_t e = 0; e < k; e++) {
        ent_pod[o + e] = tmp_pod[slot + e];
        ent_time[o + e] = tmp_time[slot + e];
    }
}

// ---- mmp_models_upsert_json: from the parsed events to the rows registry_rewrite takes -----------------------------------------
//
// Slot j is the j-th distinct registry row the call names (slot_model[j]); win[j] is the event that decides it (see
// the publish of ingest_models_kernel).  Everything here is sized by the call's events and distinct rows, never by the registry.

// s_cnt[j] = entries slot j appends to the arena (scanned into s_offs); s_cnt[k] = 0 so that the scan's last element is the total
__global__ void upsert_json_counts_kernel(const int32_t *__restrict__ win, const int32_t *__restrict__ ev_cnt, int32_t k,
                                          int32_t *__restrict__ s_cnt)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > k) return;
    const int32_t w = j < k ? win[j] : -1;
    s_cnt[j] = w >= 0 ? ev_cnt[w] : 0;
}

// One lane per slot (a model has 1-3 copies): the winner's parked entries to arena[base + s_offs[j] ...), which lies inside the
// arena (the host grew it by the scan's total) and beyond anything a published row refers to; u_idx / u_rows for
// upsert_models_kernel.  A slot without a winner saw malformed events only: an existing row (model < n_before) is staged as it
// stands, so the rewrite leaves it as it was; an appended one becomes the empty row, because its index has been handed out.
__global__ void upsert_json_build_kernel(const int32_t *__restrict__ win, const int32_t *__restrict__ slot_model, int32_t k,
                                         int32_t n_before, int32_t base, const int32_t *__restrict__ s_offs,
                                         const mmp_model_row *__restrict__ ev_rows, const int64_t *__restrict__ off,
                                         const int32_t *__restrict__ tmp_pod, const int64_t *__restrict__ tmp_time,
                                         const mmp_model_row *__restrict__ models, int32_t *__restrict__ ent_pod,
                                         int64_t *__restrict__ ent_time, int32_t *__restrict__ u_idx, mmp_model_row *__restrict__ u_rows)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k) return;
    const int32_t w = win[j], model = slot_model[j];
    mmp_model_row r{};
    if (w >= 0) {
        r = ev_rows[w];
        const int32_t cnt = r.n_loaded + r.n_failed, o = base + s_offs[j];
        const int64_t slot = off[w] / kJEntryBytes;
        for (int32_t e = 0; e < cnt; e++) {
            ent_pod[o + e] = tmp_pod[slot + e];
            ent_time[o + e] = tmp_time[slot + e];
        }
        r.ent_off = cnt ? o : 0;
    } else if (model < n_before)
        r = models[model];
    u_idx[j] = model;
    u_rows[j] = r;
}

}  // namespace mmp
