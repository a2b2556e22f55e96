// model_ids_kernels.hpp — the model-id table resident on the device: registry events arrive by key, and their keys are resolved,
// deduplicated and numbered here (mmp_model_ids_load, mmp_model_ids_resolve, mmp_model_ids_get, mmp_models_events_json).
//
// The table is the open addressing of the pod table (ingest_kernels.hpp: HashTab; linear probing, no deletion, tab_home), with one
// difference: a model id is an arbitrary user string, so a slot is identified by its hash AND its bytes.  The context keeps the id
// bytes on the device (a byte arena and int32 offsets per row, both growing by append); a lookup that meets a slot whose hash is
// equal but whose bytes differ probes on, and colliding ids coexist.  The hash may be masked to a few bits
// (MMP_MODEL_ID_HASH_BITS) so that this path is exercised: every kernel reads hashes from the array mid_hash_kernel wrote.
//
//   mid_hash_kernel      one lane per staged key: (masked) FNV-1a into hashes[]; nothing later hashes again
//   mid_resolve_kernel   one lane per key: its registry row or -1, byte-verified against the arena
//   mid_dedupe_kernel    one lane per event, a table sized by the CALL's events: the event finds or claims the slot of its key
//                        (identity = the bytes of the claiming event's key in the staged buffer) and atomicMin's its index into the
//                        slot's two words, first event and first non-deleted event
//   mid_flags_kernel     one lane per event: (joins, opens a slot, id bytes appended) as a function of the two minima
//   rocprim::exclusive_scan over those triples: append rank, slot number, arena position
//   mid_number_kernel    one lane per event: model_idx, slot, slot_model; a joining key's bytes and offset into the arena
//   idtab_rehash_kernel  (pod_events_kernels.hpp) the stored hashes into a larger table when it outgrows twice the keys
//   mid_insert_kernel    one lane per joining key: tab_claim of the first empty slot of its probe sequence
//   mid_verify_kernel    one lane per joining key, a launch of its own: the lookup must answer the row it was given
//
// A word written non-atomically in one launch is compared only in later launches (the discipline of tab_claim): hashes[] and the
// staged keys are complete before mid_dedupe_kernel starts, and within it a slot's owner is read only through the atomic that
// claimed it.  Which lane claims a slot, and under equal hashes which slot a key gets, depends on the race; no output does — all
// are functions of the two minima, so two runs are byte-identical.
//
// Ownership of the MODEL-id table (the vmodel-id table, driven by the same kernels, has the same rule for the request calls by
// vmodel id: mmp_ctx::vid_hash in mmplace.hip, vkeyed_kernels.hpp).
// Writers hold batch_mu for the call and build beside the published table: the next table in mid_next_*, the arena where it has to
// move, and an append in place only beyond the rows the published table lists — a captured ModelIdTab cannot reach rows it does
// not list.  The swap happens under the state lock held exclusive, in the hold that publishes the registry's new row count.  Readers
// hold batch_mu (mmp_model_ids_resolve / _get, the registry calls that resolve), or the state lock SHARED: the request calls by
// model id (keyed_kernels.hpp) capture the published ModelIdTab there and enqueue on a latency slot's stream, without batch_mu.  So
// whatever a swap retires — the old table, which the NEXT joining call rewrites as mid_next_*; an arena or offset array that moved
// — is neither rewritten nor released until quiesce_decisions has run behind the swap (mmplace.hip: model_ids_retired_drain;
// mmp_models_retire drains in front of its swap, inside the exclusive hold).
//
// Model ids are tens of bytes (as resolve_keys_kernel assumes for instance ids): a key is a loop of its lane.  With the hash masked
// probes run as long as the table is full and lanes of a wavefront diverge for that long; that mode is a diagnostic.
#pragma once
#include "pod_events_kernels.hpp"

namespace mmp {

// the published table and the arena it verifies against: row v's id = bytes[off[v], off[v + 1])
struct ModelIdTab {
    const uint64_t *hash;  // nullptr: no table (every key is unknown)
    const int32_t *val;
    uint32_t mask;
    const char *bytes;
    const int32_t *off;
};

// the call-local table: owner = the event that claimed the slot (-1 empty), first / first_nd = the lowest event index (lowest
// non-deleted one) of the slot's key, INT32_MAX for none
struct MidBatch {
    int32_t *owner, *first, *first_nd;
    uint32_t mask;
};

// per event, and after the exclusive scan per event position: joining keys, opened slots, arena bytes in front of it
struct MidCount {
    int32_t join, slot, bytes;
};
struct MidPlus {
    __host__ __device__ MidCount operator()(const MidCount &a, const MidCount &b) const
    {
        return MidCount{a.join + b.join, a.slot + b.slot, a.bytes + b.bytes};
    }
};

__device__ __forceinline__ bool mid_same(const char *__restrict__ a, const char *__restrict__ b, int32_t n)
{
    for (int32_t j = 0; j < n; j++)
        if (a[j] != b[j]) return false;
    return true;
}

__device__ __forceinline__ int32_t mid_find(const ModelIdTab &t, uint64_t h, const char *key, int32_t len)
{
    if (!t.hash) return -1;
    uint32_t s = tab_home(h, t.mask);
    for (uint32_t probe = 0; probe <= t.mask; probe++) {
        const int32_t v = t.val[s];
        if (v == INT32_MIN) return -1;  // empty slot
        if (t.hash[s] == h) {
            const int32_t o = t.off[v];
            if (t.off[v + 1] - o == len && mid_same(t.bytes + o, key, len)) return v;
        }
        s = (s + 1) & t.mask;
    }
    return -1;
}

// key i = keys[off[i], off[i + 1]): the raw bytes of the KV key (any UTF-8: nothing orders model ids)
__global__ __launch_bounds__(kIdTabBlock) void mid_hash_kernel(const char *__restrict__ keys, const int32_t *__restrict__ off, int32_t n,
                                                               uint64_t hmask, uint64_t *__restrict__ hashes)
{
    const int i = blockIdx.x * kIdTabBlock + threadIdx.x;
    if (i < n) hashes[i] = fnv1a(keys + off[i], off[i + 1] - off[i]) & hmask;
}

__global__ __launch_bounds__(kIdTabBlock) void mid_resolve_kernel(const char *__restrict__ keys, const int32_t *__restrict__ off, int32_t n,
                                                                  const uint64_t *__restrict__ hashes, ModelIdTab t,
                                                                  int32_t *__restrict__ row)
{
    const int i = blockIdx.x * kIdTabBlock + threadIdx.x;
    if (i < n) row[i] = mid_find(t, hashes[i], keys + off[i], off[i + 1] - off[i]);
}

// B has at least twice as many slots as the call has events, so every probe ends at the key's slot or an empty one.
//
// Contention.  The worst batch is one key repeated throughout: every lane of every wavefront ends on ONE slot.  (1) The claim looks
// before it swaps, so only the lanes that see the slot empty issue a compare-and-swap.  (2) Lanes are in event order, so when a
// whole wavefront sits on one slot its lowest live lane holds the wavefront's minimum and its lowest non-deleted lane the other:
// two atomics per wavefront instead of 128 serialised on one word.  (3) A minimum only falls, so a lane that reads a value at or
// below its own index has nothing to add and skips the atomic; a stale read costs one redundant atomicMin, never a wrong one.
__global__ __launch_bounds__(kIdTabBlock) void mid_dedupe_kernel(const char *__restrict__ keys, const int32_t *__restrict__ off, int32_t n,
                                                                 const uint64_t *__restrict__ hashes,
                                                                 const uint8_t *__restrict__ deleted, MidBatch B,
                                                                 int32_t *__restrict__ ev_slot)
{
    const int i = blockIdx.x * kIdTabBlock + threadIdx.x;
    const bool live = i < n;
    uint32_t s = 0;
    if (live) {
        const uint64_t h = hashes[i];
        const char *key = keys + off[i];
        const int32_t len = off[i + 1] - off[i];
        s = tab_home(h, B.mask);
        for (uint32_t probe = 0; probe <= B.mask; probe++) {
            int32_t o = __atomic_load_n(&B.owner[s], __ATOMIC_RELAXED);
            if (o < 0) {
                o = atomicCAS(&B.owner[s], -1, i);
                if (o < 0) break;  // claimed: this event's key names the slot
            }
            // someone's slot (o is an event index the claim published atomically; its hash and bytes are from earlier launches)
            if (o == i || (hashes[o] == h && off[o + 1] - off[o] == len && mid_same(keys + off[o], key, len))) break;
            s = (s + 1) & B.mask;
        }
    }
    const bool nd = live && !(deleted && deleted[i]);
    const int lane = threadIdx.x & 63;
    const unsigned long long act = __ballot(live), ndm = __ballot(nd);
    const int lead = act ? __ffsll((long long)act) - 1 : 0;
    const uint32_t s_lead = (uint32_t)__shfl((int)s, lead);
    const bool uniform = __ballot(live && s != s_lead) == 0;
    const bool do_first = live && (!uniform || lane == lead);
    const bool do_nd = nd && (!uniform || lane == __ffsll((long long)ndm) - 1);
    if (do_first && __atomic_load_n(&B.first[s], __ATOMIC_RELAXED) > i) atomicMin(&B.first[s], i);
    if (do_nd && __atomic_load_n(&B.first_nd[s], __ATOMIC_RELAXED) > i) atomicMin(&B.first_nd[s], i);
    if (live) ev_slot[i] = (int32_t)s;
}

// The flags of the two scans.  An event JOINS when it is its key's first non-deleted event, the key is unknown and append is on; it
// OPENS A SLOT when it is its key's first applicable event: the first event of a known key, the joining event of an unknown one
// (deletions in front of that are status 2).  counts[n] = the zero triple, so that the scan's last element is the totals.
__global__ __launch_bounds__(kIdTabBlock) void mid_flags_kernel(int32_t n, const int32_t *__restrict__ row, const int32_t *__restrict__ ev_slot,
                                                                MidBatch B, const int32_t *__restrict__ off, int32_t append,
                                                                MidCount *__restrict__ counts)
{
    const int i = blockIdx.x * kIdTabBlock + threadIdx.x;
    if (i > n) return;
    MidCount f{0, 0, 0};
    if (i < n) {
        const int32_t s = ev_slot[i];
        const bool join = append && row[i] < 0 && B.first_nd[s] == i;
        f.join = join ? 1 : 0;
        f.slot = (row[i] >= 0 ? B.first[s] == i : join) ? 1 : 0;
        f.bytes = join ? off[i + 1] - off[i] : 0;
    }
    counts[i] = f;
}

// pos = the exclusive scan of the flags; k = the slots of the call (pos[n].slot), n_before = the registry's rows before the call.
// model_idx[i] = the row of event i, -1 for an unknown id; slot[i] = its row's position among the call's distinct rows in order of
// first appearance (k, a spare word of `win`, for an event without a row); slot_model[j] = the row of slot j.  A joining key gets
// row n_before + its rank: join_ev[rank] = its event, its bytes go to arena_bytes[arena_base + pos.bytes ...) and its end offset to
// arena_off[row + 1] — beyond what the published table refers to.
__global__ __launch_bounds__(kIdTabBlock) void mid_number_kernel(int32_t n, int32_t n_before, int32_t k, const int32_t *__restrict__ row,
                                                                 const int32_t *__restrict__ ev_slot, MidBatch B, int32_t append,
                                                                 const MidCount *__restrict__ pos, const char *__restrict__ keys,
                                                                 const int32_t *__restrict__ off, int32_t arena_base,
                                                                 int32_t *__restrict__ model_idx, int32_t *__restrict__ slot,
                                                                 int32_t *__restrict__ slot_model, int32_t *__restrict__ join_ev,
                                                                 char *__restrict__ arena_bytes, int32_t *__restrict__ arena_off)
{
    const int i = blockIdx.x * kIdTabBlock + threadIdx.x;
    if (i >= n) return;
    const int32_t s = ev_slot[i];
    int32_t idx = row[i], head = B.first[s];  // head: the key's first applicable event
    if (idx < 0) {
        head = B.first_nd[s];
        // a non-deleted event has head <= i; a deletion applies only behind the event that made the id join
        idx = (append && head <= i) ? n_before + pos[head].join : -1;
    }
    model_idx[i] = idx;
    slot[i] = idx >= 0 ? pos[head].slot : k;
    if (idx >= 0 && head == i) slot_model[pos[i].slot] = idx;
    if (row[i] < 0 && append && head == i) {
        const int32_t rank = pos[i].join, len = off[i + 1] - off[i], o = arena_base + pos[i].bytes;
        join_ev[rank] = i;
        arena_off[n_before + rank + 1] = o + len;
        for (int32_t j = 0; j < len; j++) arena_bytes[o + j] = keys[off[i] + j];
    }
}

// The joining keys are distinct (deduplicated) and unknown to the table (unresolved): the first empty slot of the probe sequence is
// theirs whichever lanes race, and no byte is compared here.
__global__ __launch_bounds__(kIdTabBlock) void mid_insert_kernel(int32_t n_join, const int32_t *__restrict__ join_ev,
                                                                 const uint64_t *__restrict__ hashes, int32_t n_before, HashTabW nt)
{
    const int r = blockIdx.x * kIdTabBlock + threadIdx.x;
    if (r < n_join) tab_claim(nt, hashes[join_ev[r]], n_before + r);
}

__global__ __launch_bounds__(kIdTabBlock) void mid_verify_kernel(int32_t n_join, const int32_t *__restrict__ join_ev,
                                                                 const uint64_t *__restrict__ hashes, const char *__restrict__ keys,
                                                                 const int32_t *__restrict__ off, ModelIdTab t, int32_t *__restrict__ found)
{
    const int r = blockIdx.x * kIdTabBlock + threadIdx.x;
    if (r >= n_join) return;
    const int32_t i = join_ev[r];
    found[r] = mid_find(t, hashes[i], keys + off[i], off[i + 1] - off[i]);
}

}  // namespace mmp
