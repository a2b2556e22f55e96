// pod_events_kernels.hpp — instances join the index space after mmp_pod_ids_load, instance-table events arrive by id, and the
// registry rows that name an id the table does not know are listed (mmp_pod_ids_append, mmp_pods_events_json,
// mmp_registry_unresolved).
//
// The id -> pod table (ingest_kernels.hpp: HashTab, tab_find) is open addressing with linear probing and no deletion, so a key
// sits in the first slot of its probe sequence that was empty when it arrived, and every slot in front of it stays taken.  That
// invariant is all tab_find needs, and an atomic claim of the first empty slot keeps it whichever lanes race.
//
//   idtab_rehash_kernel       one lane per slot of the old table: its (hash, pod) claimed in the larger one — the stored 64-bit
//                             hashes are enough, no id string is read
//   idtab_insert_kernel       one lane per new id: fnv1a over its bytes, the probe sequence of tab_find, an atomic claim
//   idtab_verify_kernel       one lane per new id, a launch of its own: what tab_find answers for its hash.  An id that is equal
//                             to (or collides with) an older id or another new one finds that one's pod in front of its own —
//                             the same verdict whichever lane claimed first
//   resolve_keys_kernel       one lane per event: fnv1a over the key bytes, tab_find
//   unresolved_count_kernel   one lane per registry row: the entries whose pod lies outside [0, P); per-workgroup (rows, -, entries)
//   prune_scan_kernel         (registry_kernels.hpp) the one-workgroup scan of those triples (protocol: triple_count there)
//   unresolved_list_kernel    the same walk: the rows listed in ascending order at their scanned positions
//
// Almost every record holds 0 to 3 entries: a long record is a loop of its lane and takes no wavefront of its
// own.  No atomic decides a position in the list: two runs are byte-identical.
#pragma once
#include "ingest_kernels.hpp"
#include "registry_kernels.hpp"

namespace mmp {

constexpr int kIdTabBlock = 256;
constexpr int kUnresolvedBlock = kCompactBlock;  // (triple_count / triple_offsets are written for workgroups of this size)

// the table being built beside the published one
struct HashTabW {
    uint64_t *hash;
    int32_t *val;
    uint32_t mask;
};

// the first empty slot of h's probe sequence becomes (h, v).  The table has more slots than keys (the host sizes it at twice
// the keys), so the loop ends at an empty slot; the bound keeps a full table from spinning.
__device__ __forceinline__ void tab_claim(const HashTabW &t, uint64_t h, int32_t v)
{
    uint32_t s = tab_home(h, t.mask);
    for (uint32_t probe = 0; probe <= t.mask; probe++) {
        if (atomicCAS(&t.val[s], INT32_MIN, v) == INT32_MIN) {
            t.hash[s] = h;  // read by later launches only: nothing in this one compares hashes
            return;
        }
        s = (s + 1) & t.mask;
    }
}

__global__ __launch_bounds__(kIdTabBlock) void idtab_rehash_kernel(const uint64_t *__restrict__ old_hash,
                                                                   const int32_t *__restrict__ old_val, uint32_t old_cap, HashTabW nt)
{
    const uint32_t s = blockIdx.x * kIdTabBlock + threadIdx.x;
    if (s >= old_cap) return;
    const int32_t v = old_val[s];
    if (v != INT32_MIN) tab_claim(nt, old_hash[s], v);
}

// id i = ids[off[i], off[i + 1]) becomes pod base + i; hashes[i] is kept for the verify launch
__global__ __launch_bounds__(kIdTabBlock) void idtab_insert_kernel(const char *__restrict__ ids, const int32_t *__restrict__ off,
                                                                   int32_t n, int32_t base, HashTabW nt, uint64_t *__restrict__ hashes)
{
    const int i = blockIdx.x * kIdTabBlock + threadIdx.x;
    if (i >= n) return;
    const uint64_t h = fnv1a(ids + off[i], off[i + 1] - off[i]);
    hashes[i] = h;
    tab_claim(nt, h, base + i);
}

__global__ __launch_bounds__(kIdTabBlock) void idtab_verify_kernel(const uint64_t *__restrict__ hashes, int32_t n, HashTab t,
                                                                   int32_t *__restrict__ found)
{
    const int i = blockIdx.x * kIdTabBlock + threadIdx.x;
    if (i < n) found[i] = tab_find(t, hashes[i], -1);
}

// event i's key = keys[off[i], off[i + 1]): the raw bytes of the KV key, not JSON-escaped
__global__ __launch_bounds__(kIdTabBlock) void resolve_keys_kernel(const char *__restrict__ keys, const int32_t *__restrict__ off,
                                                                   int32_t n, HashTab t, int32_t *__restrict__ pod)
{
    const int i = blockIdx.x * kIdTabBlock + threadIdx.x;
    if (i < n) pod[i] = tab_find(t, fnv1a(keys + off[i], off[i + 1] - off[i]), -1);
}

// entries of record m (loaded or failed) whose pod is outside [0, P): the census's n_entries_unresolved, per record
__device__ __forceinline__ int32_t unresolved_entries(const mmp_model_row &m, const int32_t *__restrict__ ent_pod, int32_t P)
{
    int32_t u = 0;
    const int32_t n = m.n_loaded + m.n_failed;
    for (int32_t k = 0; k < n; k++) {
        const int32_t pod = ent_pod[m.ent_off + k];
        u += (pod < 0 || pod >= P) ? 1 : 0;
    }
    return u;
}

__global__ __launch_bounds__(kUnresolvedBlock) void unresolved_count_kernel(const mmp_model_row *__restrict__ models, int32_t M,
                                                                            const int32_t *__restrict__ ent_pod, int32_t P,
                                                                            int32_t *__restrict__ block_counts)
{
    const int i = blockIdx.x * kUnresolvedBlock + threadIdx.x;
    const int32_t u = i < M ? unresolved_entries(models[i], ent_pod, P) : 0;
    triple_count<kCol1None>(u > 0, 0, u, block_counts);
}

__global__ __launch_bounds__(kUnresolvedBlock) void unresolved_list_kernel(const mmp_model_row *__restrict__ models, int32_t M,
                                                                           const int32_t *__restrict__ ent_pod, int32_t P,
                                                                           const int32_t *__restrict__ block_off,
                                                                           int32_t *__restrict__ model_out, int32_t max_models)
{
    const int i = blockIdx.x * kUnresolvedBlock + threadIdx.x;
    const int32_t u = i < M ? unresolved_entries(models[i], ent_pod, P) : 0;
    const TripleOff o = triple_offsets<kCol1None>(u > 0, 0, u, block_off);
    if (u > 0 && o.e < max_models) model_out[o.e] = i;
}

}  // namespace mmp
