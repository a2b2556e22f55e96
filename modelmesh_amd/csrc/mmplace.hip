// mmplace.hip — libmmplace: C-ABI (include/mmplace.h) over the gfx950 kernels.
//
// Host side only marshals: it keeps a staging copy of the instance table so
// single-row events (MM.java:1455 handleInstanceTableChange) can be applied,
// uploads, launches, and hands results back.  All ranking, filtering,
// shortlisting and victim selection runs in the kernels; there is no CPU
// implementation of the path in this library.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>  // types and enums only: the library is bound at run time (dlopen), not at link time
#include <rocprim/device/device_radix_sort.hpp>
#include <chrono>
#include <rocprim/device/device_merge_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <array>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <thread>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/mmplace.h"
#include "aux_kernels.hpp"
#include "cache_kernels.hpp"
#include "gate_kernel.hpp"
#include "seam_caller_kernels.hpp"
#include "ingest_kernels.hpp"
#include "place_kernel.hpp"
#include "rebalance_kernels.hpp"
#include "registry_kernels.hpp"
#include "janitor_kernels.hpp"
#include "registry_ops_kernels.hpp"
#include "status_kernels.hpp"
#include "status_keyed_kernels.hpp"
#include "registry_ops_keyed_kernels.hpp"
#include "evictions_kernels.hpp"
#include "cache_keyed_kernels.hpp"
#include "tasks_keyed_kernels.hpp"
#include "census_kernels.hpp"
#include "pod_events_kernels.hpp"
#include "model_ids_kernels.hpp"
#include "keyed_kernels.hpp"
#include "pods_retire_kernels.hpp"
#include "rewrite_kernels.hpp"
#include "register_kernels.hpp"
#include "refs_kernels.hpp"
#include "vmodel_kernels.hpp"
#include "vkeyed_kernels.hpp"
#include "vmodel_retire_kernels.hpp"
#include "vmodel_write_kernels.hpp"
#include "shard_kernels.hpp"
#include "multi_kernel.hpp"
#include "rank_sample.hpp"
#include "snapshot.hpp"
#include "types_kernel.hpp"
#include "upgrade_tracker.hpp"

using namespace mmp;

namespace {

// mmp_last_error() returns the calling thread's own last message: the library is entered concurrently (latency
// slots) and the JNI veneer hands this pointer to ThrowNew, so it must not be a string another thread can rewrite.
thread_local std::string g_thread_err;

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = std::max<size_t>(bytes, 256);
        want = (want + 255) & ~size_t(255);
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T *as() const { return reinterpret_cast<T *>(p); }
};

// A DevBuf built beside a published one: the carrier of the library's ownership rule (written out at mmp_ctx::mid_hash).  Its
// owner holds batch_mu and declares it ahead of the work; move_into, under the state lock held EXCLUSIVE, publishes it and takes
// what it replaced, which stays allocated and unwritten until this object ends or is released explicitly.  Between the swap and
// that end the owner runs the drain (quiesce_decisions: inside the hold, or behind it), so no kernel that captured the replaced
// buffer is still running when it goes.  Never published: released on every way out, a thrown one included.
struct ScopedDevBuf {
    DevBuf b;
    ScopedDevBuf() = default;
    ScopedDevBuf(const ScopedDevBuf &) = delete;
    ScopedDevBuf &operator=(const ScopedDevBuf &) = delete;
    ~ScopedDevBuf() { b.release(); }
    bool move_into(DevBuf &dst)  // whether there was anything to publish
    {
        if (!b.p) return false;
        std::swap(dst, b);
        return true;
    }
    void release() { b.release(); }
};

// device storage of one committed snapshot
struct SnapBufs {
    DevBuf pods, lru, rem, cnt, rpm, orig, pos_of, elig, elig_nors, pref, has_pref, fullw, ge, pc, ph, nz, heads, bslots, bpm, bwin, bsurv, bpcs;
    DevBuf sel, rk;  // Snap::sel / ::rk
    DevBuf amul;     // Snap::amul
    int32_t amul_w = 0;  // words it holds
    DevBuf memo, memo_cand, memo_rk;  // Snap::memo / ::memo_cand / ::memo_rk (place_kernel.hpp: TypeMemo)
    DevBuf lmemo;                     // Snap::lmemo (place_kernel.hpp: LongMemo)
    DevBuf ctpos;  // Snap::ctpos
    uint64_t types_gen = 0;  // has_pref holds the type table of this generation
    int32_t n_bslots = 0;  // case (b) slots this snapshot has (place_kernel.hpp: BSlot), read back at commit
    void release()
    {
        for (DevBuf *b : {&pods, &lru, &rem, &cnt, &rpm, &orig, &pos_of, &elig, &elig_nors, &pref, &has_pref, &fullw, &ge, &pc, &ph, &nz, &heads, &bslots, &bpm, &bwin, &bsurv, &bpcs, &ctpos, &sel, &rk, &amul, &memo, &memo_cand, &memo_rk, &lmemo})
            b->release();
    }
};

// What Snap and ShardSnap share: the sizes, and B's rank-ordered columns and bitmaps (a template: in front of the extern "C" part).
template <class SnapT>
SnapT snap_columns(const SnapBufs &B, int32_t P, int32_t W, int32_t T, bool any_rs, int64_t min_space)
{
    SnapT S{};
    S.P = P;
    S.W = W;
    S.T = T;
    S.any_rs = any_rs;
    S.min_space = min_space;
    S.lru = B.lru.as<int64_t>();
    S.rem = B.rem.as<int64_t>();
    S.cnt = B.cnt.as<int32_t>();
    S.rpm = B.rpm.as<int32_t>();
    S.orig = B.orig.as<int32_t>();
    S.pos_of = B.pos_of.as<int32_t>();
    S.elig = B.elig.as<uint64_t>();
    S.elig_nors = B.elig_nors.as<uint64_t>();
    S.pref = B.pref.as<uint64_t>();
    S.has_pref = B.has_pref.as<uint8_t>();
    S.fullw = B.fullw.as<uint64_t>();
    return S;
}

// What decisions read besides the Snap columns, one set per committed snapshot (double-buffered with SnapBufs, so
// that a commit builds the next set while decisions keep reading the published one): the type table's allowed
// rows, the cluster / partition / type-set stats (device + host mirrors), the instance partitions, and the
// registry view resolved against THIS snapshot's rank positions.
struct SnapSide {
    DevBuf d_allowed, d_has_allowed, stats_acc, d_pts, d_prohib, pstats, tstats, rmodels;
    DevBuf mtw;  // PlaceArgs::mtw: rmodels[i].type, an int per model (valid whenever rmodels is)
    uint64_t types_gen = 0;  // d_allowed / d_has_allowed hold the type table of this generation
    bool rmodels_ok = false;
    std::vector<int32_t> pts_of;        // pod -> partition (-1: not in the table)
    std::vector<uint64_t> pts_prohib;   // [n_pts][tw] prohibited type rows
    int32_t n_pts = 0, pts_tw = 1;
    std::vector<StatsAcc> pstats_h, tstats_h;  // host mirrors (pstats_h has n_pts + 1 entries: the last is EMPTY_STATS)
    void release()
    {
        for (DevBuf *b : {&d_allowed, &d_has_allowed, &stats_acc, &d_pts, &d_prohib, &pstats, &tstats, &rmodels, &mtw}) b->release();
    }
};

}  // namespace

// Low-latency slot for small host-pointer batches (the single ensureLoaded / invokeModel request):
// pinned, device-mapped request / result buffers and a stream of its own, so that one decision never
// queues behind a 100k-decision batch or a commit (SURVEY.md §8b "Threading").
// Every pinned buffer the device and the host hand data through WHILE A KERNEL RUNS (completion flags, result rows of
// the latency slots, the resident kernel's request slots) is allocated fine-grained and device-mapped explicitly:
// hipHostMallocDefault would leave the choice to the process environment (HIP_HOST_COHERENT).
constexpr unsigned int kPinnedFlags = hipHostMallocCoherent | hipHostMallocMapped;
constexpr size_t kSelMaxBytes = (size_t)32 << 20;  // Snap::sel / ::rk are built up to this size each (per snapshot side)
constexpr int kTailStaticLds = 512;  // what place_tail_body keeps in static LDS beside place_block's own
constexpr int kTailBlocks = 64;    // one-wavefront workgroups of a split batch's tail launch (measured: profiles/tail_slot)
constexpr int kMaxMissBufs = 64;   // streams with split batches in flight that get a buffer of their own (more: those batches go unsplit)
constexpr int kFastSlots = 4;
constexpr int kFastN = 4096;       // decisions per fast call
constexpr int kFastExtra = 16384;  // extra-exclusion pool entries per fast call
struct FastSlot {
    std::mutex mu;
    hipStream_t stream = nullptr;
    mmp_place_req *reqs = nullptr;  // hipHostMalloc'ed: same pointer is valid on the device
    int32_t *extra = nullptr;
    mmp_place_out *outs = nullptr;
    uint32_t *done = nullptr;  // pinned: the kernel stores the call's sequence number here when its results are visible
    uint32_t *blocks = nullptr;  // device: finished-workgroup counter of the call in flight
    // sequence number of the slot's last launch: bumped by the owner (under f.mu and the shared state lock), read by
    // quiesce_decisions without either — hence atomic
    std::atomic<uint32_t> seq{0};
};

// ---- the slot layout table: what each request call puts where in a slot's three buffers -----------------------------------------
// A call rides a slot while every count it brings is within its row here (k*: the crossover thresholds — they decide latency);
// beyond them it is staged through device scratch on the context's batch stream (seam_run).  A region is a byte range of `reqs`
// (kSlotReq), `extra` (kSlotPool) or `outs` (kSlotOut); slot_after puts one behind another, 16-byte aligned, so regions of one row
// cannot overlap; slot_fits says of EVERY region of a row that it is aligned and ends inside its buffer.
enum SlotBuf { kSlotReq, kSlotPool, kSlotOut };
constexpr size_t kSlotBufBytes[3] = {kFastN * sizeof(mmp_place_req), kFastExtra * sizeof(int32_t), kFastN * sizeof(mmp_place_out)};
struct SlotRegion {
    SlotBuf buf;
    size_t off, bytes;
};
constexpr SlotRegion kStagedOnly{kSlotReq, 0, 0};  // an array of a call that never rides a slot
constexpr SlotRegion slot_first(SlotBuf buf, size_t count, size_t elem) { return {buf, 0, count * elem}; }
constexpr SlotRegion slot_after(SlotRegion prev, size_t count, size_t elem)
{
    return {prev.buf, (prev.off + prev.bytes + 15) & ~size_t(15), count * elem};
}
constexpr bool slot_fits(std::initializer_list<SlotRegion> regions)
{
    for (const SlotRegion &r : regions)
        if (r.off % 16 != 0 || r.off + r.bytes > kSlotBufBytes[r.buf]) return false;
    return true;
}
struct PlaceSlot {  // mmp_place_batch; mmp_place_batch_c writes calls of this size out as mmp_place_req rows
    static constexpr int kN = kFastN, kExtra = kFastExtra;
    static constexpr SlotRegion reqs = slot_first(kSlotReq, kN, sizeof(mmp_place_req)), extra = slot_first(kSlotPool, kExtra, 4),
                                outs = slot_first(kSlotOut, kN, sizeof(mmp_place_out));
    static_assert(slot_fits({reqs, extra, outs}), "place slot layout");
};
struct ServeSlot {  // mmp_serve_batch: everything a call brings is O(copies), 48 B + 16 B per listed copy
    static constexpr int kN = 1024, kCounters = 8192, kExcl = 4096;
    static constexpr SlotRegion reqs = slot_first(kSlotReq, kN, sizeof(mmp_serve_req)),
                                counters = slot_after(reqs, kCounters, sizeof(mmp_serve_counter)),
                                excl_pod = slot_first(kSlotPool, kExcl, 4), excl_time = slot_after(excl_pod, kExcl, 8),
                                outs = slot_first(kSlotOut, kN, sizeof(mmp_serve_out));
    static_assert(slot_fits({reqs, counters, excl_pod, excl_time, outs}), "serve slot layout");
};
struct GateSlot {  // mmp_gate_batch: as many 144-byte requests as the request buffer holds (1820; their 8-byte results fit with room)
    static constexpr int kN = (int)(kSlotBufBytes[kSlotReq] / sizeof(mmp_gate_req)), kExcl = 4096, kExplicit = 4096;
    static constexpr SlotRegion reqs = slot_first(kSlotReq, kN, sizeof(mmp_gate_req)), excl_pod = slot_first(kSlotPool, kExcl, 4),
                                explicit_pool = slot_after(excl_pod, kExplicit, 4), excl_time = slot_after(explicit_pool, kExcl, 8),
                                gouts = slot_first(kSlotOut, kN, sizeof(mmp_gate_out));
    static_assert(slot_fits({reqs, excl_pod, explicit_pool, excl_time, gouts}), "gate slot layout");
};
struct MissSlot {  // mmp_miss_batch: the load-target half where mmp_place_batch has it, the guards' half behind
    static constexpr int kN = 256, kPool = 2048;  // kPool: each of extras, exclusion pairs, explicit
    static constexpr SlotRegion preqs = slot_first(kSlotReq, kN, sizeof(mmp_place_req)), greqs = slot_after(preqs, kN, sizeof(mmp_gate_req)),
                                extra = slot_first(kSlotPool, kPool, 4), excl_pod = slot_after(extra, kPool, 4),
                                explicit_pool = slot_after(excl_pod, kPool, 4), excl_time = slot_after(explicit_pool, kPool, 8),
                                pouts = slot_first(kSlotOut, kN, sizeof(mmp_place_out)), gouts = slot_after(pouts, kN, sizeof(mmp_gate_out));
    static_assert(slot_fits({preqs, greqs, extra, excl_pod, explicit_pool, excl_time, pouts, gouts}), "miss slot layout");
};
struct RouteSlot {  // mmp_route_batch: the serve half shares the guards' exclusion pairs
    static constexpr int kN = 256, kCounters = 4096, kExcl = 4096, kExplicit = 4096;
    static constexpr SlotRegion greqs = slot_first(kSlotReq, kN, sizeof(mmp_gate_req)), sreqs = slot_after(greqs, kN, sizeof(mmp_serve_req)),
                                counters = slot_after(sreqs, kCounters, sizeof(mmp_serve_counter)),
                                excl_pod = slot_first(kSlotPool, kExcl, 4), explicit_pool = slot_after(excl_pod, kExplicit, 4),
                                excl_time = slot_after(explicit_pool, kExcl, 8),
                                gouts = slot_first(kSlotOut, kN, sizeof(mmp_gate_out)), souts = slot_after(gouts, kN, sizeof(mmp_serve_out));
    static_assert(slot_fits({greqs, sreqs, counters, excl_pod, explicit_pool, excl_time, gouts, souts}), "route slot layout");
};
// The request calls by id: the layout of the call they resolve in front of, with what the resolver reads behind its requests and the
// rows it resolves behind its results.  A tail is that addition, stated once per resolver and put behind any base: `req_end` is
// the base's last region of the request buffer, `out_end` its last region of the result buffer.  kKeyBytes / kNfBytes: the bytes
// of each a call may bring onto a slot — what the resolving kernel stages in LDS of each.
constexpr int kKeyedN = 256;
// By model id (mmp_place_batch_ck / _route_batch_ck / _miss_batch_ck; keyed_kernels.hpp): the key bytes (kKeyedPad readable bytes
// behind them) and the n + 1 key offsets; the n resolved rows.
template <const SlotRegion &req_end, const SlotRegion &out_end>
struct KeyTail {
    static constexpr int kKeyBytes = kKeyedLdsBytes, kNfBytes = 0;
    static constexpr SlotRegion keys = slot_after(req_end, kKeyBytes + kKeyedPad, 1), key_off = slot_after(keys, kKeyedN + 1, 4),
                                idx = slot_after(out_end, kKeyedN, 4);
    static constexpr bool fits = slot_fits({keys, key_off, idx});
};
// By VMODEL id (mmp_place_batch_cv / _route_batch_cv / _miss_batch_cv; vkeyed_kernels.hpp): the vmodel key bytes, the n + 1 key
// offsets, the notFoundModelId bytes (each byte region with kKeyedPad readable bytes behind it), their n + 1 offsets and the n flag
// words; the n mmp_vseam_row.
static_assert(sizeof(mmp_vseam_row) == 24, "mmp_vseam_row is 24 bytes");
template <const SlotRegion &req_end, const SlotRegion &out_end>
struct VKeyTail {
    static constexpr int kKeyBytes = kVKeyedLdsBytes, kNfBytes = kVKeyedLdsBytes;
    static constexpr SlotRegion keys = slot_after(req_end, kKeyBytes + kKeyedPad, 1), key_off = slot_after(keys, kKeyedN + 1, 4),
                                nf = slot_after(key_off, kNfBytes + kKeyedPad, 1), nf_off = slot_after(nf, kKeyedN + 1, 4),
                                flags = slot_after(nf_off, kKeyedN, 4), vm = slot_after(out_end, kKeyedN, sizeof(mmp_vseam_row));
    static constexpr bool fits = slot_fits({keys, key_off, nf, nf_off, flags, vm});
};
template <template <const SlotRegion &, const SlotRegion &> class Tail>
struct KeyedPlaceSlot {  // a 256-request layout of its own: PlaceSlot fills its buffers
    static constexpr int kN = kKeyedN, kExtra = MissSlot::kPool;
    static constexpr SlotRegion reqs = slot_first(kSlotReq, kN, sizeof(mmp_place_req)), extra = slot_first(kSlotPool, kExtra, 4),
                                outs = slot_first(kSlotOut, kN, sizeof(mmp_place_out));
    using T = Tail<reqs, outs>;
    static_assert(slot_fits({reqs, extra, outs}) && T::fits, "keyed place slot layout");
};
template <template <const SlotRegion &, const SlotRegion &> class Tail>
struct KeyedMissSlot {
    using L = MissSlot;
    static constexpr int kN = kKeyedN;
    using T = Tail<L::greqs, L::gouts>;
    static_assert(kN <= L::kN && T::fits, "keyed miss slot layout");
};
template <template <const SlotRegion &, const SlotRegion &> class Tail>
struct KeyedRouteSlot {
    using L = RouteSlot;
    static constexpr int kN = kKeyedN;
    using T = Tail<L::counters, L::souts>;
    static_assert(kN <= L::kN && T::fits, "keyed route slot layout");
};
// every region where it has always been: the byte offsets of keys, key_off, (nf, nf_off, flags,) idx / vm
template <class T>
constexpr bool key_tail_at(size_t keys, size_t key_off, size_t idx)
{
    return T::keys.off == keys && T::key_off.off == key_off && T::idx.off == idx;
}
template <class T>
constexpr bool vkey_tail_at(size_t keys, size_t key_off, size_t nf, size_t nf_off, size_t flags, size_t vm)
{
    return T::keys.off == keys && T::key_off.off == key_off && T::nf.off == nf && T::nf_off.off == nf_off && T::flags.off == flags && T::vm.off == vm;
}
static_assert(key_tail_at<KeyedPlaceSlot<KeyTail>::T>(16384, 32784, 4096), "keyed place slot offsets");
static_assert(key_tail_at<KeyedMissSlot<KeyTail>::T>(53248, 69648, 6144), "keyed miss slot offsets");
static_assert(key_tail_at<KeyedRouteSlot<KeyTail>::T>(114688, 131088, 6144), "keyed route slot offsets");
static_assert(vkey_tail_at<KeyedPlaceSlot<VKeyTail>::T>(16384, 24592, 25632, 33840, 34880, 4096), "vmodel-keyed place slot offsets");
static_assert(vkey_tail_at<KeyedMissSlot<VKeyTail>::T>(53248, 61456, 62496, 70704, 71744, 6144), "vmodel-keyed miss slot offsets");
static_assert(vkey_tail_at<KeyedRouteSlot<VKeyTail>::T>(114688, 122896, 123936, 132144, 133184, 6144), "vmodel-keyed route slot offsets");
struct EvictSlot {  // mmp_evict_batch: as many 32-byte result rows as the result buffer holds (2048); their 16-byte requests fit
    static constexpr int kN = (int)(kSlotBufBytes[kSlotOut] / sizeof(mmp_evict_out));
    static constexpr SlotRegion reqs = slot_first(kSlotReq, kN, sizeof(mmp_evict_req)), outs = slot_first(kSlotOut, kN, sizeof(mmp_evict_out));
    static_assert(slot_fits({reqs, outs}), "evict slot layout");
};

// The environment switches (all MMP_*), read once per context at mmp_create (read_tuning).  The defaults are the product's routes;
// the switches force routes for the tests and for comparison runs.
struct Tuning {
    int32_t force_wave = 0;      // MMP_FORCE_WAVE=1: every decision takes the wave-per-decision kernel (tests)
    int32_t no_memo = 0;         // MMP_NO_MEMO=1: batches do not use the per-type shortlists (place_kernel.hpp: TypeMemo)
    int32_t memo_from = -1;      // MMP_MEMO_FROM=n: decisions from which a batch takes the kernel with the shortlists in front (default kMemoFrom / kMemoFromC)
    int32_t no_long_memo = 0;    // MMP_NO_LONG_MEMO=1: commit records no walks of the long shortlists (place_kernel.hpp: LongMemo)
    int32_t no_split = 0;        // MMP_NO_SPLIT=1: batches are never split (place_memo_kernel + place_tail_kernel); the one-launch kernels instead
    int32_t split_from = -1;     // MMP_SPLIT_FROM=n: decisions from which a batch is split (default kSplitFrom / kSplitFromC)
    int32_t tail_blocks = kTailBlocks;  // MMP_TAIL_BLOCKS=n: one-wavefront workgroups of a split batch's tail launch (1 .. kRestLists)
    int32_t split_notail = 0;    // MMP_SPLIT_NOTAIL=1: the tail launch is left out — the batch's results are INCOMPLETE (bench.py times the first launch alone)
    int32_t no_long_lds = 0;     // MMP_NO_LONG_LDS=1: the long path reads its per-type tables from global memory (tests, comparison)
    int32_t no_caseb = 0;        // MMP_NO_CASEB=1: case (b) decisions never use the whole-window tables (tests: the wave path decides them)
    int32_t long_dense_from = kLongDenseFrom;  // MMP_LONG_DENSE_FROM=n: decisions from which a full-cluster batch takes the 4-wavefront instantiation with its tables staged in LDS
    bool long_dense_env = false;                // (... and whether it was given: see dense_from)
    int32_t long_mode = -1;      // MMP_LONG_MODE: -1 auto (the long-shortlist kernel for snapshots whose instances are nearly all full), 0 never, 1 always (tests)
    int32_t rank_mode = 0;       // MMP_RANK_MODE: 0 auto (rank by sampling from kRankSortMinPods pods), 1 all-pairs, 2 by sampling whenever legal, 3 merge sort whenever legal (tests)
    int32_t no_delta = 0;        // MMP_NO_DELTA=1: every commit ranks from scratch (tests)
    int32_t plan_sorted = 0;     // MMP_PLAN_SORTED=1: mmp_proactive_plan takes its sorted (fallback) path on every input; 2: never (tests)
    int32_t plan_fused = 1;      // MMP_PLAN_FUSED=0: the plan as its eight dependent launches (comparison; the one-launch form is the default)
    int32_t resident = 0;        // MMP_RESIDENT=1: mmp_create turns the resident decision kernel on (mmp_resident)
    int32_t label_hash_bits = 64;     // MMP_LABEL_HASH_BITS=b: the same for the label-name hashes (tests: the byte comparison of label_find)
    int32_t model_id_hash_bits = 64;  // MMP_MODEL_ID_HASH_BITS=b: every model-id hash is masked to its low b bits, 0: all equal (tests: ids that collide)
    int32_t vmodel_id_hash_bits = 64;  // MMP_VMODEL_ID_HASH_BITS=b: the same for the vmodel-id hashes
};

struct mmp_ctx {
    mmp_config cfg{};
    hipStream_t stream = nullptr;
    // lock order: batch_mu (owner of `stream`, the s_* / r_* scratch and the commit's INPUTS — the staged instance
    // table, type table, replica-set list, registry — for a whole call) -> mu (the published snapshot pointers +
    // host staging as readers see it; decision paths hold it only while they capture the pointers and enqueue,
    // loaders hold it for the whole call, a commit only for its final pointer swap)
    std::mutex batch_mu, err_mu, cs_mu;
    // the state lock: decision paths that only capture the published pointers and enqueue take it SHARED (so that the
    // submission threads of mmp_issue_threads launch concurrently), whoever changes what they capture takes it exclusive
    std::shared_mutex mu;
    // submission threads (mmp_issue_threads); null: launches are issued by the caller.  Read and swapped under pool_mu
    // (a leaf lock): a submitter keeps its own reference for the duration of its call, so mmp_issue_threads(ctx, 0 / n)
    // on another thread cannot free the rings underneath it
    std::shared_ptr<struct IssuePool> pool;
    std::mutex pool_mu;
    // the resident decision kernel for single requests (place_kernel.hpp: place_resident_kernel; mmp_resident)
    struct Resident {
        // written under launch_mu (running, generation) / the state lock (enabled) and READ without either by every single request on its
        // way in (the optimistic checks of mmp_place_batch / resident_place; resident_ensure looks again under the locks): atomics
        // (tools/asan_lib.sh, ThreadSanitizer: plain bools here were its first two reports)
        std::atomic<bool> enabled{false}, running{false};
        std::atomic<uint32_t> generation{0};  // of the kernel launched last (1, 2, ...)
        hipStream_t stream = nullptr;
        ResidentSlot *slots = nullptr;  // pinned, device-mapped: host -> device
        ResidentAnswer *answers = nullptr;  // pinned, device-mapped: device -> host
        ResidentCtl *ctl = nullptr;     // pinned
        std::mutex launch_mu;           // taken AFTER the state lock
        std::mutex slot_mu[kResidentSlots];
        uint32_t seq[kResidentSlots] = {};
        std::atomic<uint32_t> rr{0};
        long long idle_ticks = 5'000'000;  // 50 ms at the 100 MHz wall clock
        std::atomic<uint64_t> launches{0}, served{0}, punted{0};
        std::atomic<int> slow{0};  // answers in a row that took longer than 20 ms (self-check in resident_place)
        std::atomic<int> punt_streak{0}, skip{0};  // hand-backs in a row; single requests still to be sent to the launch path directly
    } res;
    // caller-owned streams that *_dev calls were enqueued on (leaf lock cs_mu): whoever rewrites state a decision
    // kernel reads waits for them as well as for the library's own streams (quiesce_decisions)
    std::vector<hipStream_t> caller_streams;
    std::string err;
    FastSlot fast[kFastSlots];
    std::atomic<uint32_t> fast_rr{0};
    // mmp_profile(): HIP events around the kernels (not the staging copies) of each host-pointer call
    bool prof = false, prof_armed = false;
    hipEvent_t pe0 = nullptr, pe1 = nullptr;
    double last_kernel_ms = -1.0;
    size_t lds_limit = 64 * 1024;    // LDS a workgroup may use on this device (hipDeviceAttributeMaxSharedMemoryPerBlock)
    // a registry event's in-place rewrite is enqueued under the state lock and finishes after it: kernels that read the registry
    // from other streams are ordered behind reg_event while reg_pending (order_after_registry)
    DevBuf rt_sreqs, rt_souts, rt_cnt;  // mmp_route_batch: the serve half's staging (the gate half uses s_reqs / s_outs / s_a / s_c / s_d)
    hipEvent_t reg_event = nullptr;
    std::atomic<bool> reg_pending{false};
    std::atomic<size_t> lds_granted{48 * 1024};  // dynamic LDS the place kernels may be launched with so far
    Tuning tune;                  // the environment switches (read_tuning)
    int32_t plan_grid_max = 0;    // workgroups the one-launch plan may have: all of them resident at once
    // the split form of a large batch (place_kernel.hpp: place_memo_kernel + place_tail_kernel):
    // per stream that has issued a split batch: the words its first launches leave for its tails (launches of one stream are ordered,
    // so one buffer per stream will do) and a pinned pair the tail reports to: {undecided, of how many}.  A tail decides whatever
    // the lists hold and zeroes them, so the two launches of a batch must follow each other on the stream: `mu` is held from the
    // buffer's lookup until the tail is enqueued (two host threads on one stream).  Slots have fixed addresses; mmp_stream_retire
    // returns a stream's slot.
    struct MissBuf {
        std::mutex mu;             // taken after the state lock, before miss_mu; guards words / cap
        bool used = false;         // (used, st, report: under miss_mu; a slot in use is returned only with mu held as well)
        hipStream_t st = nullptr;
        int32_t *words = nullptr;  // place_kernel.hpp: rest_buffer_ints — counters, gate line + kRestLists lists
        size_t cap = 0;            // ints
        uint32_t calls = 0;        // split batches enqueued on `words`: its parity names the call's gate word (place_kernel.hpp, above kRestLists); under mu
        int32_t *report = nullptr;
    };
    MissBuf miss_bufs[kMaxMissBufs];
    std::vector<void *> miss_retired; // outgrown word buffers: a launch in flight may still read them; freed with the context (miss_mu)
    int32_t *miss_reports = nullptr;  // pinned, kMaxMissBufs pairs (slot i: pair i)
    std::mutex miss_mu;               // a leaf lock: slot lookup / allocation, miss_retired, miss_reports
    std::atomic<bool> split_off{false};  // a tail reported more than 1/32 of its batch: batches go unsplit until the next commit / registry event
    std::atomic<int64_t> n_split{0};     // split batches issued (mmp_split_batches)

    // host staging (inputs of the next commit)
    std::vector<mmp_pod_row> pods;
    int32_t n_types = 0, types_w = 0;
    std::vector<uint64_t> allowed, prefer;
    std::vector<uint8_t> has_allowed, has_prefer;
    std::vector<int32_t> replaced_rs;
    UpgradeTracker upgrades;

    // committed snapshot (double-buffered; `cur` is what decisions read): the rank-ordered columns and bitmaps,
    // and the instance partitions / subset stats / resolved registry view that belong to them (snapshot.hpp)
    SnapBufs sb[2];
    SnapSide side[2];
    int cur = 0;
    bool committed = false;
    Snap snap{};
    mmp_stats stats{};

    // pod-axis shard mode (mmp_shard_configure): this context owns the rank positions of
    // `ssnap` only; n_shards == 0 means the ordinary single-device snapshot
    int32_t shard = 0, n_shards = 0;
    ShardSnap ssnap{};
    DevBuf rk_rows, rk_idx, rk_tmp;  // ranking by sorting (snapshot.hpp)
    bool snap_long = false;  // the committed snapshot takes place_batch_long_kernel
    bool snap_full = false;  // ... because (nearly) all of its instances are full (not only because a type is sparse)
    // the rows written since the last commit (a commit of a few changed rows re-ranks by insertion: delta_scatter_kernel)
    uint64_t types_gen = 1;       // bumped by every load of the type table; device copies remember the one they hold
    uint64_t d_prefer_gen = 0;
    std::vector<int32_t> sig_of;    // per instance: id of its ProhibitedTypeSet among the distinct ones (valid while the type table stands)
    std::vector<uint64_t> sig_rows;
    bool sig_valid = false;
    std::vector<int32_t> dirty;
    bool dirty_all = true;          // the table was replaced / grew: the next commit ranks from scratch
    bool order_total = false;       // the published order came from a total order (sort-legal rows): unchanged rows keep their order
    std::vector<int32_t> h_order, h_pos;  // host mirror of the published order (position -> row, row -> position), fetched lazily
    bool h_order_valid = false;
    int64_t n_delta_commits = 0;
    Snap sview{};  // the lane path's view of this shard's slice (place_shard_fast_kernel)
    DevBuf f_offs, f_idx, f_reqs, f_outs, f_scan_tmp;  // speculative form: the compacted rest of a batch
    // ... and what ONE batch in flight owns until its rest count has been read, twice (slot = batch parity): an asynchronous
    // batch is completed after the NEXT one has been enqueued, so the two must not share flags, counter, word or exchange words
    DevBuf f_flags[2];             // per decision: undecided by the single exchange
    DevBuf f_cnt[2];               // finished workgroups << 32 | flagged decisions of the finish launch in flight (zero between launches)
    uint64_t *f_done = nullptr;    // pinned, words [0] and [8]: seq << 32 | flagged decisions, stored by the finish kernel's last workgroup
    uint32_t f_slot = 0;
    uint32_t f_seq = 0;
    // mmp_shard_place_batch_async_dev: the batch whose finish kernel is enqueued and whose rest count has not been read yet
    struct ShardPending {
        bool active = false;
        const void *d_reqs = nullptr, *d_extra = nullptr;
        void *d_outs = nullptr;
        int32_t n = 0;
        int64_t now = 0;
        uint32_t seq = 0, slot = 0;
    } pend;
    int32_t last_n_rest = 0;
    bool rank_pending = false;

    // RCCL group of the pod-axis shards (mmp_shard_group_init): collectives run on c->stream, inside the boundary
    std::mutex group_mu;  // one group-level call at a time (taken before batch_mu / mu by the group entry points)
    ncclComm_t comm = nullptr;
    mmp_exchange_fn xfn = nullptr;  // a host-supplied transport instead of RCCL (mmp_shard_group_set_exchange)
    void *xuser = nullptr;
    bool group = false;
    int32_t g_rank = 0, g_world = 1;
    DevBuf g_rankbuf, g_xf[2], g_x[6];

    // commit scratch
    DevBuf rank, occupancy, flag, rs_list, rs_bad, d_prefer;

    // model registry view
    DevBuf models, ent_pod, ent_time;
    int32_t n_models = 0, n_entries = 0;  // n_entries = used part of the entry arena (mmp_models_upsert appends)
    std::vector<int32_t> m_cnt;           // host shadow: entries per model (for the arena's garbage accounting)
    int64_t ent_live = 0;                 // entries still referenced by a row
    DevBuf u_idx, u_rows, u_cnt, u_offs, u_tmp;
    // mmp_registry_prune: `missings` (MM.java:6776) by pod index — first time seen missing, 0 = no mark — for miss_n pod slots, and
    // the scratch only the prune uses (registry_kernels.hpp).  Owned by batch_mu; only the prune kernels, on c->stream, touch them.
    DevBuf miss_since, p_state, p_seen, p_removed;
    int32_t miss_n = 0;
    // The scratch the registry plans share (mmp_registry_prune, mmp_janitor_plan, mmp_registry_ops).  The sharing is safe by one
    // rule: every user holds batch_mu from its first use of a buffer to its last, and uses it on c->stream only.
    struct PlanScratch {
        DevBuf totals, block_counts;   // PruneScalars from prune_scan_kernel; the per-workgroup triples, then offsets
        DevBuf edits, keep_off;        // the call's edit structs in output order; where each one's kept entries start
        DevBuf rows_in, call_scalars;  // the caller's rows (cache rows / ops); the call's own counters (JanitorScalars / RopsScalars)
        DevBuf row_tmp;                // row-sized scratch (janitor: carved; ops: the status bytes)
        DevBuf model_map;              // model -> row, all -1 between runs over its first model_map_n words (0: not known to be clear)
        int32_t model_map_n = 0;
    } plan;
    std::vector<uint64_t> u_stamp;        // per model: (call generation, row index) of the last row naming it
    uint32_t u_gen = 0;
    // (the registry view resolved against a snapshot, place_kernel.hpp: ResolvedModel, lives in SnapSide)

    // eviction caches
    DevBuf c_seg, c_lu, c_wt, c_cap;
    int32_t n_caches = 0;
    int64_t cache_entries = 0;  // entries of all deques loaded by mmp_caches_load (picks the eviction kernel's team size)

    // stateful keyed caches (mmp_caches_load_keyed / mmp_cache_replay): two layouts, ping-pong
    struct KeyedStore {
        DevBuf off, lu, wt, key, n;
    } ks[2];
    int ks_cur = 0;
    int32_t k_caches = 0;
    std::vector<int32_t> k_n;  // host mirror of the live entry counts
    DevBuf r_part;  // per-workgroup partials of the proactive plan's first pass
    DevBuf rs_split, rs_int;  // rank_sample.hpp: the sorted samples; range_of[P] | idx[P] | hist | cur | off
    DevBuf k_cap, k_wsize, k_oldest, k_ubm, k_ops, k_order, k_opoff, k_outs, k_ev, k_evlu, k_evoff, k_ids;  // k_ids: cache ids grouped by replay team width
    // the caches by model id (cache_keyed_kernels.hpp).  k_bound: the keys of the current store are registry rows (set by
    // mmp_caches_load_keyed_k; dropped by mmp_caches_load_keyed and mmp_model_ids_load).  k_slots: the deque slots of the current
    // store, off[k_caches].  evid_*: the eviction record of the last mmp_cache_replay_k, as bytes — a retirement cannot change it.
    bool k_bound = false;
    int32_t k_slots = 0;
    std::vector<char> evid_bytes;
    std::vector<int32_t> evid_off{0};
    std::vector<int64_t> evid_lu;  // the victims' lastUsed by slot, kept with the id record; evid_timed: the last replay recorded them
    bool evid_timed = false;       // (mmp_cache_replay_kt; a plain mmp_cache_replay_k or a cache load clears it)
    DevBuf ev_in, ev_out;  // mmp_evictions_k: the victims' entries, their mmp_evicted_out rows
    DevBuf k_inv, k_kstat, k_krow, k_len, k_goff, k_gbytes;  // inverse of k_order; status / row by caller op; the id gather's lengths, offsets, bytes

    // wire-format ingestion: per-pod id attributes and the hash tables the parsers probe
    std::vector<uint32_t> id_order_v;
    std::vector<int32_t> replica_set_v;
    DevBuf idtab_hash, idtab_val, tytab_hash, tytab_val, j_buf, j_off, j_rows, j_aux, j_status, j_cnt, j_offs, j_tmp_pod, j_tmp_time,
        j_scan_tmp, j_ev;  // j_ev: the per-event / per-distinct-row words of the registry event calls (UpsertJsonEvents, carve)
    uint32_t idtab_mask = 0, tytab_mask = 0;
    bool have_ids = false, have_types = false;
    int32_t unknown_type = 0, default_type = 0;
    // what mmp_pod_ids_append continues from the load: the id bytes (id i = id_bytes[id_offs[i], id_offs[i + 1])), the pods in id
    // order, and the replica-set interning.  idtab_next_*: the table built beside the published one (swapped in when the call
    // succeeds); ida_*: the new ids / event keys of one call on the device — bytes, offsets, hashes, what tab_find answered.
    std::string id_bytes;
    std::vector<int32_t> id_offs{0}, id_sorted;
    std::unordered_map<std::string, int32_t> rs_intern;
    DevBuf idtab_next_hash, idtab_next_val, ida_bytes, ida_off, ida_hash, ida_found;
    // The instance labels.  pod_label_word / pod_label_count sit beside c->pods under the same locks and are as long as it
    // (labels_cover): the known-label bits of each staged instance and the element count of its `labels` array (0 = NO_LABELS).
    // lbtab_* / lb_arena / lb_off: the label names on the device (ingest_kernels.hpp: LabelTab), read under batch_mu by
    // ingest_pod_labels_kernel alone; j_lab: one call's words | counts | statuses.
    std::vector<uint64_t> pod_label_word;
    std::vector<int32_t> pod_label_count;
    DevBuf lbtab_hash, lbtab_val, lb_arena, lb_off, j_lab;
    uint32_t lbtab_mask = 0;
    uint64_t lb_hmask = ~0ull;
    bool have_labels = false;
    DevBuf unres_list;  // mmp_registry_unresolved: the listed rows (its other scratch is the registry plans')
    // The model-id table (model_ids_kernels.hpp): mid_hash / mid_val / mid_mask the published table, mid_bytes / mid_off the id arena
    // (row r = mid_bytes[mid_off[r], mid_off[r + 1]); mid_n rows, mid_nbytes bytes); mid_next_*: the table built beside the published
    // one.  OWNERSHIP: every writer holds batch_mu for its whole call, and builds beside the published table (the arena's append
    // lands beyond the rows the published table lists).  The published fields (the six above without mid_next_*, and
    // have_model_ids) change under the state lock held EXCLUSIVE, in the same hold that publishes the registry's row count
    // (n_models); readers hold batch_mu, or — the request calls by model id on a latency slot — the state lock SHARED while they
    // capture the fields and enqueue.  A buffer a swap retires (the old table, which becomes mid_next_*; an arena or offset array
    // that moved) is neither rewritten nor released before quiesce_decisions has run behind the swap (model_ids_retired_drain).
    // ScopedDevBuf carries the rule for every buffer that is not one of a ping-pong pair: built in it, published by move_into, the
    // retired allocation released when it ends.
    // me_*: one call's keys on the device — hashes, resolved rows, dedupe
    // slots, the call-local table (owner | first | first_nd), the flags and their scan, model_idx, the joining events, what the
    // verify found.  (slot / slot_model and the deleted bytes are written where the pipeline reads them: j_ev.)
    DevBuf mid_hash, mid_val, mid_next_hash, mid_next_val, mid_bytes, mid_off;
    DevBuf me_hash, me_row, me_slot, me_tab, me_cnt, me_pos, me_idx, me_join, me_found;
    // the staged path of the request calls by model id: the key bytes, their offsets, the resolved rows, and the load-target half of
    // mmp_miss_batch_ck (its guards' half takes the scratch of mmp_gate_batch).  Owned by batch_mu, used on c->stream.
    DevBuf kq_keys, kq_off, kq_idx, kq_preqs, kq_pouts;
    uint32_t mid_mask = 0;
    int32_t mid_n = 0, mid_nbytes = 0;
    bool have_model_ids = false;
    // mmp_models_retire (retire_kernels.hpp): the caller's list, keep[row], remap[row] and the two atomicMin words (the lowest
    // non-empty row | the lowest row the verify lost).  Owned by batch_mu, used on c->stream; the triples and their scan are me_cnt /
    // me_pos / j_scan_tmp.  mmp_pods_retire (pods_retire_kernels.hpp) keeps its remap[instance] in ret_remap and its PodsRetireWords
    // in ret_word, under the same rule.
    DevBuf ret_rows, ret_keep, ret_remap, ret_word;

    // per-call scratch for the host-pointer entry points
    DevBuf s_reqs, s_outs, s_extra, s_a, s_b, s_c, s_d;
    // rebalancer scratch
    DevBuf r_ps, r_counts, r_keys, r_vals, r_keys2, r_vals2, r_tmp, r_out_model, r_out_lu;
    // mmp_registry_census (census_kernels.hpp): the call's outputs on the device — stats | type rows | pod_loaded | pod_failed — zeroed
    // by every call, and their host copy.  Owned by batch_mu, used on c->stream.  census_pod_lds: the dynamic LDS the walk may be
    // launched with (beyond it the per-pod counts go to global memory; 32 KB need no grant, the first call asks for
    // kCensusPodLdsBytes); census_cus: compute units of the device (0: not asked yet).
    DevBuf cn_out;
    std::vector<unsigned char> cn_host;
    size_t census_pod_lds = 32 * 1024;
    int32_t census_cus = 0;
    // mmp_models_status (status_kernels.hpp): the call's copy list on the device.  Owned by batch_mu, used on c->stream; its other
    // scratch is the registry plans' (plan).
    DevBuf st_copies;
    // mmp_models_status_k / mmp_vmodels_status (status_keyed_kernels.hpp): one call's fail_pod and flags words, the 64-bit total of
    // the reply's string bytes, and the strings on the device.  The keys are ida_*, the owners vm_ow_*, the request flags vm_rflags,
    // the resolved rows me_row, the vrows vm_ans, the lengths and their scan j_cnt / j_offs / j_scan_tmp.  Owned by batch_mu, used on
    // c->stream.
    DevBuf sk_fpod, sk_flags, sk_sc, sk_str;
    // mmp_models_rewrite_json (rewrite_kernels.hpp).  idd_bytes / idd_off: the device copy of the instance id store (id_bytes /
    // id_offs), uploaded lazily: every writer of the host store bumps id_gen, the call uploads when idd_gen differs.  rw_*: one
    // call's rows, last_unload, fail_pod, messages and their offsets, sizes, offsets, statuses and rendered bytes.  Owned by
    // batch_mu, used on c->stream; the parser's scratch is the j_* of the registry event calls.
    DevBuf idd_bytes, idd_off, rw_rows, rw_lul, rw_fpod, rw_fmsg, rw_fmoff, rw_len, rw_off, rw_status, rw_out;
    // mmp_models_register_json (register_kernels.hpp): one call's requests, their three strings and offsets, classes and
    // last_used; sizes, offsets and rendered bytes are rw_len / rw_off / rw_out.  Owned by batch_mu, used on c->stream.
    DevBuf rg_reqs, rg_info, rg_ioff, rg_cls, rg_lu;
    // mmp_models_refs_json (refs_kernels.hpp): one call's requests, strings, offsets and classes are the rg_* above (both request
    // structs take 16 bytes); rf_refs: its counts.  Owned by batch_mu, used on c->stream.
    DevBuf rf_refs;
    // mmp_vmodels_write_json (vmodel_write_kernels.hpp): one call's requests, their strings (the default owner behind them) and
    // offsets, and the answers; the parser's scratch is vm_ev / j_ev / j_status.  Owned by batch_mu, used on c->stream.
    DevBuf vw_reqs, vw_strs, vw_soff, vw_rows;
    uint64_t id_gen = 1, idd_gen = 0;
    // The vmodel table (vmodel_kernels.hpp), nothing of it allocated before the first vmodel call.  vid_*: its id table, the fields
    // of the model-id table over again (both are driven through IdTabRef).  vm_rows: one VmRow per vmodel; vm_arena: the strings,
    // vm_arena_bytes of them used, vm_live_bytes referred to by a row; vm_live_rows: rows that are not ABSENT.  vm_ev / vm_cnt /
    // vm_pos: one event call's parsed events, byte counts and their scan; vm_nf_* / vm_ow_* / vm_rflags / vm_ans: one resolve's
    // staged strings, flags and answers; vm_list: the transition scan's rows.  The scratch is owned by batch_mu, used on c->stream.
    // mmp_vmodels_retire (vmodel_retire_kernels.hpp) takes its scratch from mmp_models_retire: ret_*, me_cnt / me_pos / j_scan_tmp.
    // OWNERSHIP of the table itself — vid_hash / vid_val / vid_mask / vid_bytes / vid_off / vid_n / vid_nbytes, vm_rows, vm_arena,
    // vm_arena_bytes and have_vmodels — is the rule written at mid_hash: every writer (mmp_vmodels_events_json, its squeeze,
    // mmp_vmodels_retire) holds batch_mu for its whole call and builds beside what is published: the next id table in vid_next_*,
    // the row array in vm_rows_next whenever a row of a known id is rewritten or the array has to grow (a ping-pong pair, as
    // mid_next_* is), the arenas where they have to move; in place it only appends — id bytes and rows beyond vid_n, strings beyond
    // vm_arena_bytes, which nothing a captured table lists refers to.  The published fields change under the state lock held
    // EXCLUSIVE, all in one hold.  Readers hold batch_mu (mmp_vmodels_resolve, _transitions, _get, _info, _write_json), or — the
    // request calls by vmodel id on a latency slot — the state lock SHARED while they capture the fields and enqueue.  What a swap
    // retires (the old id table, now vid_next_*; the old rows, now vm_rows_next; an arena that moved, in its ScopedDevBuf) is neither
    // rewritten nor released before quiesce_decisions has run behind the swap (vmodels_retired_drain).
    // vq_*: the staged path of the request calls by vmodel id — the nf bytes, their offsets, the flags, the mmp_vseam_row (the keys
    // and the load-target half take kq_*).  Owned by batch_mu, used on c->stream.
    DevBuf vid_hash, vid_val, vid_next_hash, vid_next_val, vid_bytes, vid_off;
    DevBuf vm_rows, vm_rows_next, vm_arena, vm_ev, vm_cnt, vm_pos, vm_nf_bytes, vm_nf_off, vm_ow_bytes, vm_ow_off, vm_rflags, vm_ans, vm_list;
    DevBuf vq_nf, vq_nf_off, vq_flags, vq_out;
    uint32_t vid_mask = 0;
    int32_t vid_n = 0, vid_nbytes = 0, vm_arena_bytes = 0, vm_live_rows = 0;
    int64_t vm_live_bytes = 0;
    bool have_vmodels = false;
};

namespace {

int fail(mmp_ctx *c, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_thread_err = buf;
    if (c) {
        std::lock_guard<std::mutex> g(c->err_mu);
        c->err = buf;  // kept for debuggers; readers go through the thread-local copy
    }
    return code;
}

#define HIP_TRY(c, expr)                                                                       \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail((c), MMP_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                   \
    } while (0)

// The end of every entry point's function-try-block: no C++ exception crosses the C boundary.
#define MMP_CATCH(c, name)                                                                  \
    catch (const std::bad_alloc &) { return fail((c), MMP_ENOMEM, "%s: out of host memory", name); } \
    catch (const std::exception &e_) { return fail((c), MMP_EHIP, "%s: %s", name, e_.what()); }

inline int div_up(int a, int b) { return (a + b - 1) / b; }

// the side state of the published snapshot (read with c->mu held, or by the owner of c->batch_mu: only a commit,
// which holds batch_mu, flips c->cur)
inline SnapSide &cur_side(mmp_ctx *c) { return c->side[c->cur]; }

// Blocking copy on the context's own (non-blocking) stream.  The library never touches the legacy null
// stream: one synchronous hipMemset there at context creation was measured to serialise, for the rest of the
// process, kernels that the host issues on separate streams (8-stream step time 4.0 -> 9.8 us).
// tests/test_abi.py::test_library_never_uses_the_null_stream keeps it that way.
hipError_t copy_sync(mmp_ctx *c, void *dst, const void *src, size_t bytes, hipMemcpyKind kind);
constexpr int kRankSortMinPods = 8192;
constexpr int kSampleMinPods = 1024;  // (the sample path needs P >= its 512 samples; MMP_RANK_MODE=3: the merge sort instead)

// Kernel-time bracket of a host-pointer entry point (owner of c->batch_mu): KT_BEGIN after the H2D
// copies are enqueued, KT_END after the last kernel, kt_collect() once the stream has been synchronised.
#define KT_BEGIN(c, st)                                             \
    do {                                                            \
        (c)->prof_armed = false;                                    \
        if ((c)->prof && hipEventRecord((c)->pe0, (st)) == hipSuccess) (c)->prof_armed = true; \
    } while (0)
#define KT_END(c, st)                                               \
    do {                                                            \
        if ((c)->prof_armed && hipEventRecord((c)->pe1, (st)) != hipSuccess) (c)->prof_armed = false; \
    } while (0)
inline void kt_collect(mmp_ctx *c)
{
    if (!c->prof) return;
    float ms = -1.f;
    if (c->prof_armed && hipEventElapsedTime(&ms, c->pe0, c->pe1) != hipSuccess) ms = -1.f;
    c->last_kernel_ms = ms;
    c->prof_armed = false;
}
// The device span of a call is the sum of its brackets: kt_add behind the last kt_collect adds what an earlier bracket collected.
// Where either span is unknown (negative), or profiling is off, the later one stands.  kt_sum: the rule as a value (a_ms stands).
inline void kt_add(mmp_ctx *c, double earlier_ms)
{
    if (c->prof && earlier_ms >= 0 && c->last_kernel_ms >= 0) c->last_kernel_ms += earlier_ms;
}
inline double kt_sum(const mmp_ctx *c, double a_ms, double b_ms) { return c->prof && a_ms >= 0 && b_ms >= 0 ? a_ms + b_ms : a_ms; }

// Called with c->mu held, before device state that decisions read is overwritten: every decision
// kernel was enqueued under c->mu, so once the streams are idle nothing reads the old state.
hipError_t copy_sync(mmp_ctx *c, void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
{
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, c->stream);
    return e != hipSuccess ? e : hipStreamSynchronize(c->stream);
}

// The resident kernel holds the snapshot it was launched with: whoever publishes another one or rewrites what it reads
// stops it (called with the state lock held, or from mmp_destroy); the next single request launches a new one.
void resident_stop(mmp_ctx *c)
{
    auto &R = c->res;
    if (!R.slots) return;
    std::lock_guard<std::mutex> g(R.launch_mu);
    if (!R.running) return;
    __atomic_store_n(&R.ctl->stop, R.generation.load(std::memory_order_relaxed), __ATOMIC_RELEASE);
    (void)hipStreamSynchronize(R.stream);
    R.running = false;
}

hipError_t slot_wait(FastSlot *f, uint32_t seq);
hipError_t quiesce_decisions(mmp_ctx *c)
{
    resident_stop(c);
    // A latency slot has a kernel in flight only while its completion word lags its sequence number (the kernel stores the word
    // last; the owner bumps the number under the state lock, which the caller of this function holds or which no launch can pass
    // any more): an idle slot costs a load here, not a hipStreamSynchronize (the slots' synchronisations were 50-100 us under the
    // exclusive lock).  The number is read ONCE per slot: the quiescer waits for the launches that existed when it came, not for
    // the ones a busy owner keeps adding behind them (sequence numbers wrap: compare by difference).
    for (FastSlot &f : c->fast) {
        if (!f.done) continue;
        const uint32_t snap = f.seq.load(std::memory_order_acquire);
        if ((int32_t)(__atomic_load_n(f.done, __ATOMIC_ACQUIRE) - snap) >= 0) continue;
        hipError_t e = slot_wait(&f, snap);
        if (e != hipSuccess) return e;
    }
    std::vector<hipStream_t> cs;
    {
        std::lock_guard<std::mutex> g(c->cs_mu);
        cs = c->caller_streams;
    }
    for (hipStream_t st : cs) {
        hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) return e;
    }
    return hipStreamSynchronize(c->stream);
}

// hipStreamPerThread is a different stream in every thread that names it: the library could neither wait for what another thread
// enqueued on it (quiesce_decisions) nor keep one split buffer per stream (miss_buffer).  Every entry point that takes a stream
// refuses it (include/mmplace.h).
int refuse_per_thread_stream(mmp_ctx *c, const void *stream, const char *who)
{
    if (stream != static_cast<const void *>(hipStreamPerThread)) return MMP_OK;
    return fail(c, MMP_EINVAL, "%s: hipStreamPerThread (stream handle %p) names a different stream in every thread; pass a stream "
                "created with hipStreamCreate", who, stream);
}

// a *_dev call was enqueued on `st` (called with c->mu held)
void note_caller_stream(mmp_ctx *c, hipStream_t st)
{
    if (st == c->stream) return;
    std::lock_guard<std::mutex> g(c->cs_mu);
    for (hipStream_t k : c->caller_streams)
        if (k == st) return;
    c->caller_streams.push_back(st);
}

// Re-resolve every model's entry list against a snapshot's rank positions, into that snapshot's side state.
// For the PUBLISHED snapshot (after the model table changed): call with c->mu held and the decision streams idle.
// For the snapshot a commit is building: the side is not visible to decisions yet; the caller owns c->batch_mu,
// which keeps the model table still.
int rebuild_resolved(mmp_ctx *c, SnapSide &sd, const Snap &snap, bool committed, bool sync = true)
{
    sd.rmodels_ok = false;
    if (!committed || c->n_models <= 0) return MMP_OK;  // (shard contexts: `snap` carries the whole table's pos_of — resolved positions are GLOBAL)
    HIP_TRY(c, sd.rmodels.ensure((size_t)c->n_models * sizeof(ResolvedModel)));
    HIP_TRY(c, sd.mtw.ensure((size_t)c->n_models * 4));
    hipLaunchKernelGGL(resolve_models_kernel, dim3(div_up(c->n_models, 256)), dim3(256), 0, c->stream, snap,
                       c->models.as<mmp_model_row>(), c->ent_pod.as<int32_t>(), c->n_models,
                       sd.rmodels.as<ResolvedModel>(), sd.mtw.as<int32_t>());
    HIP_TRY(c, hipGetLastError());
    if (sync) HIP_TRY(c, hipStreamSynchronize(c->stream));
    sd.rmodels_ok = true;
    return MMP_OK;
}
int rebuild_resolved(mmp_ctx *c) { return rebuild_resolved(c, cur_side(c), c->snap, c->committed); }

// ---- latency slots (FastSlot): pinned, device-mapped buffers + a completion flag ---------------------
// Small host-pointer calls do not stage through hipMemcpy and do not hold the context's batch stream: the
// kernel reads its requests from and writes its results to pinned host memory on the slot's own
// high-priority stream and announces completion through the slot's pinned flag (wave.hpp: announce_done).
FastSlot *slot_acquire(mmp_ctx *c, std::unique_lock<std::mutex> &lock)
{
    const uint32_t first = c->fast_rr.fetch_add(1, std::memory_order_relaxed);
    for (int k = 0; k < kFastSlots; k++) {
        FastSlot &cand = c->fast[(first + k) % kFastSlots];
        std::unique_lock<std::mutex> t(cand.mu, std::try_to_lock);
        if (t.owns_lock()) {
            lock = std::move(t);
            return &cand;
        }
    }
    FastSlot *f = &c->fast[first % kFastSlots];
    lock = std::unique_lock<std::mutex>(f->mu);
    return f;
}

// Spin on the slot's flag until launch number `seq` has completed (the owner passes its own launch's number, a quiescer the
// number it read when it came); the ordinary stream synchronisation is the fallback when it is late.
hipError_t slot_wait(FastSlot *f, uint32_t seq)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spins = 0;; spins++) {
        if ((int32_t)(__atomic_load_n(f->done, __ATOMIC_ACQUIRE) - seq) >= 0) return hipSuccess;
        if ((spins & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(500)) break;
        __builtin_ia32_pause();
    }
    return hipStreamSynchronize(f->stream);
}

hipError_t order_after_registry(mmp_ctx *c, hipStream_t st);
// The buffer of a split batch on `st` (`ints`: rest_buffer_ints of its first launch) and the stream's report pair, returned with the
// stream's slot locked in `hold` (the caller enqueues both launches before it lets go); false: none to be had (too many streams, no
// memory) — the batch goes unsplit, nothing is held.  Also reads what the stream's last tail reported.  `calls`: the slot's count of
// split batches, which the caller advances once BOTH launches are enqueued (a count advanced for a batch that then went unsplit would
// hand the next one the gate word its predecessor's tail has not zeroed).
bool miss_buffer(mmp_ctx *c, hipStream_t st, size_t ints, int32_t **words, int32_t **report, uint32_t **calls, std::unique_lock<std::mutex> &hold)
{
    mmp_ctx::MissBuf *mb = nullptr;
    while (!mb) {
        {
            std::lock_guard<std::mutex> g(c->miss_mu);
            mmp_ctx::MissBuf *fresh = nullptr;
            for (auto &b : c->miss_bufs) {
                if (b.used && b.st == st) mb = &b;
                if (!b.used && !fresh) fresh = &b;
            }
            if (!mb) {
                if (!fresh) return false;
                if (!c->miss_reports) {
                    if (hipHostMalloc(reinterpret_cast<void **>(&c->miss_reports), (size_t)kMaxMissBufs * 2 * sizeof(int32_t), kPinnedFlags) != hipSuccess) {
                        c->miss_reports = nullptr;
                        return false;
                    }
                    memset(c->miss_reports, 0, (size_t)kMaxMissBufs * 2 * sizeof(int32_t));
                }
                fresh->used = true;
                fresh->st = st;
                fresh->report = c->miss_reports + 2 * (fresh - c->miss_bufs);
                fresh->report[0] = fresh->report[1] = 0;  // (a reused slot: what the retired stream's tails reported is not this one's)
                mb = fresh;
            }
        }
        // the slot's lock with miss_mu let go: a thread enqueueing on the same stream holds it for two launches, the other streams go on
        hold = std::unique_lock<std::mutex>(mb->mu);
        std::lock_guard<std::mutex> g(c->miss_mu);
        if (!mb->used || mb->st != st) {  // retired (and maybe handed to another stream) meanwhile: look again
            hold.unlock();
            mb = nullptr;
        }
    }
    if (mb->cap < ints) {
        size_t want = std::max<size_t>(ints, 65536);
        want = std::max(want, mb->cap + mb->cap / 2);
        void *p = nullptr;
        if (hipMalloc(&p, want * sizeof(int32_t)) != hipSuccess) {
            hold.unlock();
            return false;
        }
        // the counters and both gate words start at zero (every tail leaves its lists' counters and the other call's gate word so);
        // ordered before the stream's first launch on this buffer
        if (hipMemsetAsync(p, 0, (size_t)kRestHeadInts * sizeof(int32_t), st) != hipSuccess) {
            (void)hipFree(p);
            hold.unlock();
            return false;
        }
        if (mb->words) {  // (a launch in flight may still read it)
            std::lock_guard<std::mutex> g(c->miss_mu);
            c->miss_retired.push_back(mb->words);
        }
        mb->words = static_cast<int32_t *>(p);
        mb->cap = want;
    }
    // the last tail of this stream that has finished: more than 1/32 of its batch undecided -> the records do not fit these batches
    const int32_t undecided = __atomic_load_n(&mb->report[0], __ATOMIC_RELAXED), of = __atomic_load_n(&mb->report[1], __ATOMIC_RELAXED);
    if (of > 0 && (int64_t)undecided * 32 > (int64_t)of) c->split_off.store(true, std::memory_order_relaxed);
    *words = mb->words;
    *report = mb->report;
    *calls = &mb->calls;
    return true;
}
// a new snapshot / registry: split batches get another chance (the reports of the old one's tails are void)
void split_reset(mmp_ctx *c)
{
    std::lock_guard<std::mutex> g(c->miss_mu);
    if (c->miss_reports) memset(c->miss_reports, 0, (size_t)kMaxMissBufs * 2 * sizeof(int32_t));
    c->split_off.store(false, std::memory_order_relaxed);
}

Tuning read_tuning()
{
    Tuning t;
    const auto flag = [](const char *name, int32_t &v) { if (const char *e = getenv(name)) v = e[0] == '1'; };
    const auto num = [](const char *name, int32_t &v) { if (const char *e = getenv(name)) v = atoi(e); };
    flag("MMP_FORCE_WAVE", t.force_wave);
    flag("MMP_NO_MEMO", t.no_memo), num("MMP_MEMO_FROM", t.memo_from), flag("MMP_NO_LONG_MEMO", t.no_long_memo);
    flag("MMP_NO_SPLIT", t.no_split), num("MMP_SPLIT_FROM", t.split_from);
    num("MMP_TAIL_BLOCKS", t.tail_blocks);
    t.tail_blocks = std::max(1, std::min(t.tail_blocks, kRestLists));
    flag("MMP_SPLIT_NOTAIL", t.split_notail), flag("MMP_NO_LONG_LDS", t.no_long_lds), flag("MMP_NO_CASEB", t.no_caseb);
    t.long_dense_env = getenv("MMP_LONG_DENSE_FROM") != nullptr;
    num("MMP_LONG_DENSE_FROM", t.long_dense_from), num("MMP_LONG_MODE", t.long_mode);
    num("MMP_RANK_MODE", t.rank_mode), flag("MMP_NO_DELTA", t.no_delta);
    num("MMP_PLAN_SORTED", t.plan_sorted), num("MMP_PLAN_FUSED", t.plan_fused);
    flag("MMP_RESIDENT", t.resident);
    num("MMP_MODEL_ID_HASH_BITS", t.model_id_hash_bits);
    t.model_id_hash_bits = std::max(0, std::min(t.model_id_hash_bits, 64));
    num("MMP_VMODEL_ID_HASH_BITS", t.vmodel_id_hash_bits);
    t.vmodel_id_hash_bits = std::max(0, std::min(t.vmodel_id_hash_bits, 64));
    num("MMP_LABEL_HASH_BITS", t.label_hash_bits);
    t.label_hash_bits = std::max(0, std::min(t.label_hash_bits, 64));
    return t;
}

// The argument block of the place kernels, as far as every caller fills it alike: `rmodels` is the registry view resolved against the
// published snapshot (null where the caller does not use it, or it is not built); the caller sets what is its own (wins, mtw, n_dev,
// force_wave, the latency fields) afterwards.
PlaceArgs place_args(mmp_ctx *c, const void *d_reqs, int32_t n, const void *d_extra, int64_t now, void *d_outs, bool resolved, int32_t n_pods_all)
{
    PlaceArgs A{};
    A.reqs = static_cast<const mmp_place_req *>(d_reqs);
    A.models = c->models.as<mmp_model_row>();
    A.rmodels = (resolved && cur_side(c).rmodels_ok) ? cur_side(c).rmodels.as<ResolvedModel>() : nullptr;
    A.ent_pod = c->ent_pod.as<int32_t>();
    A.extra = static_cast<const int32_t *>(d_extra);
    A.outs = static_cast<mmp_place_out *>(d_outs);
    A.n = n;
    A.n_models = c->n_models;
    A.now = now;
    A.n_pods_all = n_pods_all;
    return A;
}

// What only some callers of place_launch bring; all unset: a batch of mmp_place_req rows on one stream.
struct PlaceCall {
    const mmp_place_caller *caller = nullptr;  // the single-caller form: the requests are mmp_place_req_c rows (batch kernels only)
    int32_t extra_bound = 0;                   // bounded calls: 1 + the entries of the exclusion pool the caller declared; 0: not declared
    // the latency path (FastSlot): the pinned completion flag, this launch's sequence number, the slot's workgroup counter
    uint32_t *done_flag = nullptr;
    uint32_t done_seq = 0;
    uint32_t *done_blocks = nullptr;
    const mmp_place_req *inline_req = nullptr;  // one request without exclusions, passed in the kernel arguments
    const PlaceSegs *segs = nullptr;            // several request arrays in one launch of seg_blocks workgroups (multi_kernel.hpp)
    int32_t seg_blocks = 0;
    const GateArgs *fused_gate = nullptr;       // with inline_req: the cache-miss route, the guards beside the load target
    const mmp_gate_req *fused_greq = nullptr;
};

// a place launch that announces completion through `done` (seam_run: a slot's flag and this launch's sequence number, or none)
PlaceCall slot_call(const DoneFlag &done, const mmp_place_req *inline_req)
{
    PlaceCall o;
    o.done_flag = done.flag;
    o.done_seq = done.seq;
    o.done_blocks = done.blocks;
    o.inline_req = inline_req;
    return o;
}

// The kernel (or, for a split batch, the pair of kernels) a place launch takes.
enum class PlaceRoute {
    memo_split, memo_split_c,  // place_memo_kernel + place_tail_kernel (_c: the single-caller form)
    multi, multi_m, multi_long, multi_long4,
    miss_single, single_lean, flag,
    batch, batch_m, batch_c, batch_c_m, batch_long, batch_long4, batch_long_c, batch_long4_c,
};
bool is_split(PlaceRoute r) { return r == PlaceRoute::memo_split || r == PlaceRoute::memo_split_c; }

// What the route depends on besides the tuning, the call and its size: plain values, captured under the state lock.
struct RouteState {
    bool snap_long = false, snap_full = false;  // mmp_ctx::snap_long / snap_full
    bool memo = false, lmemo = false;           // the snapshot has TypeMemo / LongMemo records
    bool wins = false, rmodels = false;         // PlaceArgs::wins / rmodels are set
    bool split_ok = false;                      // a split buffer is to be had for the stream and split_off is not set
    bool memo_tail_lds = false;                 // the tail of a memo split fits the device's LDS
};

// the long kernel on a full cluster: the case (b) tables and the first lane phase on the prefix tables (PlaceArgs::long_first)
bool long_first(const RouteState &s) { return s.snap_long && s.snap_full && s.rmodels; }

// decisions from which a full-cluster batch takes the 4-wavefront instantiation with its tables in LDS.  With the recorded long walks
// (place_kernel.hpp: LongMemo) hardly a request searches those tables, and the barrier-free instantiation is the faster one at every
// size (C3 full cluster, 200k / 400k / 800k requests per launch: 16.0 / 25.6 / 40.3 us against 18.5 / 28.9 / 43.5 us;
// profiles/r6/long_records.txt) — unless MMP_LONG_DENSE_FROM is given.
int32_t dense_from(const Tuning &t, const RouteState &s)
{
    return (long_first(s) && s.lmemo && !t.long_dense_env) ? INT32_MAX : t.long_dense_from;
}

PlaceRoute place_route(const Tuning &t, const RouteState &s, int32_t n, const PlaceCall &o)
{
    const bool caller = o.caller != nullptr, latency = o.inline_req || o.done_flag;
    // batches with the per-type shortlists in front: head windows and the resolved registry view in place, not the full-cluster
    // regime (its shortlists span the table), none of the diagnostic routes, a launch that fills the chip
    const bool use_memo = !latency && !s.snap_long && !t.no_memo && !t.force_wave && s.wins && s.rmodels && s.memo &&
                          n >= (t.memo_from >= 0 ? t.memo_from : (caller ? kMemoFromC : kMemoFrom));
    // the split form: the check alone in a launch of its own, the rest in a dense tail behind it (place_kernel.hpp: place_memo_kernel);
    // one launch instead when there is no buffer, split_off is set or the tail's LDS does not fit
    const bool split = !o.segs && !t.no_split && s.split_ok;
    if (use_memo && split && s.memo_tail_lds && n >= (t.split_from >= 0 ? t.split_from : (caller ? kSplitFromC : kSplitFrom)))
        return caller ? PlaceRoute::memo_split_c : PlaceRoute::memo_split;
    if (o.segs) {
        // (the multi path compares with MMP_LONG_DENSE_FROM's value as it is, the batch path with dense_from())
        if (s.snap_long) return n >= t.long_dense_from ? PlaceRoute::multi_long4 : PlaceRoute::multi_long;
        return use_memo ? PlaceRoute::multi_m : PlaceRoute::multi;
    }
    if (o.inline_req) return o.fused_gate ? PlaceRoute::miss_single : PlaceRoute::single_lean;
    if (o.done_flag && n > kPlaceBlock) return PlaceRoute::flag;
    if (caller && s.snap_long) return n >= dense_from(t, s) ? PlaceRoute::batch_long4_c : PlaceRoute::batch_long_c;
    if (use_memo) return caller ? PlaceRoute::batch_c_m : PlaceRoute::batch_m;
    if (caller) return PlaceRoute::batch_c;
    if (s.snap_long) return n >= dense_from(t, s) ? PlaceRoute::batch_long4 : PlaceRoute::batch_long;
    return PlaceRoute::batch;
}

template <class K>
const void *kfn(K *k) { return reinterpret_cast<const void *>(k); }
// Dynamic LDS beyond the default grant (48 KB): asked once for every place kernel, up to the device's limit less the static part.
int grant_place_lds(mmp_ctx *c)
{
    static std::mutex grant_mu;  // (decision paths hold the state lock shared)
    std::lock_guard<std::mutex> g(grant_mu);
    const int want = (int)(c->lds_limit - kPlaceStaticLds);
    const int tail = want - kTailStaticLds;  // the tails keep kTailStaticLds of static LDS beside place_block's own
    const struct {
        const void *fn;
        int max_lds;
    } kernels[] = {
        {kfn(place_batch_kernel), want}, {kfn(place_batch_m_kernel), want}, {kfn(place_batch_c_kernel), want},
        {kfn(place_batch_c_m_kernel), want}, {kfn(place_batch_long_kernel), want}, {kfn(place_batch_long4_kernel), want},
        {kfn(place_batch_long_c_kernel), want}, {kfn(place_batch_long4_c_kernel), want}, {kfn(place_batch_flag_kernel), want},
        {kfn(place_single_lean_kernel), want}, {kfn(miss_single_kernel), want}, {kfn(place_multi_kernel), want},
        {kfn(place_multi_m_kernel), want}, {kfn(place_multi_long_kernel), want}, {kfn(place_multi_long4_kernel), want},
        {kfn(place_tail_kernel), tail}, {kfn(place_tail_c_kernel), tail},
    };
    for (const auto &k : kernels) HIP_TRY(c, hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, k.max_lds));
    c->lds_granted.store((size_t)want, std::memory_order_release);
    return MMP_OK;
}

int place_launch(mmp_ctx *c, const void *d_reqs, int32_t n, const void *d_extra, int64_t now, void *d_outs, hipStream_t st,
                 const PlaceCall &o = PlaceCall{})
{
    if (n == 0) return MMP_OK;
    if (o.caller && (o.segs || o.inline_req || o.done_flag)) return fail(c, MMP_EINVAL, "the single-caller form takes the batch kernels only");
    const Tuning &t = c->tune;
    const Snap &S = c->snap;
    const SnapBufs &B = c->sb[c->cur];
    // 1. the argument block and the dynamic LDS
    PlaceArgs A = place_args(c, d_reqs, n, d_extra, now, d_outs, true, S.P);
    A.mtw = cur_side(c).rmodels_ok ? cur_side(c).mtw.as<int32_t>() : nullptr;
    A.wins = c->n_shards > 0 ? nullptr : B.heads.as<TypeWin>();
    A.force_wave = t.force_wave;
    A.done_flag = o.done_flag;
    A.done_seq = o.done_seq;
    A.extra_bound = o.extra_bound;
    RouteState rs;
    rs.snap_long = c->snap_long, rs.snap_full = c->snap_full, rs.memo = S.memo != nullptr, rs.lmemo = S.lmemo != nullptr;
    rs.wins = A.wins != nullptr, rs.rmodels = A.rmodels != nullptr;
    const bool latency = o.inline_req || o.done_flag;
    const int wpad = (S.W + 1) & ~1;
    // one dynamic region: the lane phase's windows + scratch, re-used by the wave path's tiles (place_block)
    size_t lds = std::max<size_t>((size_t)kPlaceWaves * 2 * wpad * sizeof(uint64_t), (size_t)place_lane_lds(S.T));
    A.long_first = long_first(rs) ? 1 : 0;
    // the long path's per-type tables in LDS when they are small (C3: 20 KB) and the launch fills the chip: measured on the full
    // cluster, 800k decisions per launch 70.8 -> 67.1 us; at 100k (1.5 wavefronts per SIMD) 20.4 -> 21.0 us, hence the size condition
    if (A.long_first && !latency && !t.no_long_lds && n >= dense_from(t, rs)) {
        const size_t tb = long_tables_bytes(S.T, S.W);
        // (only where they fit beside the wave tile and the static part: a device with 64 KB of LDS per workgroup keeps reading
        // them from global memory instead of failing the launch)
        if (tb <= 24 * 1024 && ((lds + 15) & ~(size_t)15) + tb + kPlaceStaticLds <= c->lds_limit) {
            const size_t off = (lds + 15) & ~(size_t)15;
            A.long_first = 1 + (int32_t)off;
            lds = off + tb;
        }
    }
    if (c->snap_long && !latency && A.wins && !t.no_caseb && B.n_bslots > 0) {
        A.bslots = B.bslots.as<BSlot>();
        A.n_bslots = std::min(B.n_bslots, kBSlots);
        A.bwin = B.bwin.as<BLaunch>();
        A.bsurv = B.bsurv.as<uint64_t>();
        A.bpcs = B.bpcs.as<int32_t>();
    }
    // the wave path's tile (two bitmaps of the whole table per wavefront) next to the static LDS of place_block;
    // gfx950 gives a workgroup up to 160 KB (c->lds_limit is the device's answer), which admits ~120k instances
    if (lds + kPlaceStaticLds > c->lds_limit)
        return fail(c, MMP_EINVAL, "instance table too large for the LDS staging tile (%d pods: %zu + %d bytes of LDS, the device "
                    "gives a workgroup %zu)", S.P, lds, kPlaceStaticLds, c->lds_limit);
    if (lds > c->lds_granted.load(std::memory_order_acquire))
        if (const int rc = grant_place_lds(c)) return rc;
    // NOBAR kernels: a region per wavefront (place_wave_lds) instead of the shared one
    const size_t lds_nobar = (size_t)kPlaceWaves * place_wave_lds(wpad);
    // the tail of a split batch: workgroups of ONE wavefront, that wavefront's region alone
    const size_t lds_tail = (size_t)place_wave_lds(wpad);
    rs.memo_tail_lds = lds_tail + kPlaceStaticLds + kTailStaticLds <= c->lds_limit && (size_t)kPlaceWaves * memo_region_bytes(S.T) <= c->lds_limit;
    HIP_TRY(c, order_after_registry(c, st));
    // 2. the route; a split route holds the stream's buffer from here until its tail is enqueued (miss_buffer)
    const int grid = div_up(n, kPlaceBlock);
    const int cap = rest_list_cap(grid * kPlaceWaves);  // the first launch's wavefronts share kRestLists lists
    int32_t *words = nullptr, *report = nullptr;
    uint32_t *calls = nullptr;
    std::unique_lock<std::mutex> pair;
    rs.split_ok = !c->split_off.load(std::memory_order_relaxed);
    PlaceRoute r = place_route(t, rs, n, o);
    if (is_split(r) && (!miss_buffer(c, st, rest_buffer_ints(grid * kPlaceWaves), &words, &report, &calls, pair) ||
                        c->split_off.load(std::memory_order_relaxed))) {
        if (pair) pair.unlock();
        rs.split_ok = false;
        r = place_route(t, rs, n, o);
    }
    if (t.split_notail) words = nullptr;  // (diagnostics: the undecided requests are not even recorded)
    // 3. the launch
    const size_t lds_memo = (size_t)kPlaceWaves * memo_region_bytes(S.T);  // per wavefront: a copy of the types' records / its lane scratch
    const dim3 block(kPlaceBlock), tails(t.tail_blocks), tail_block(kTailBlock);
    const bool tail = !t.split_notail;
    const int32_t par = calls ? (int32_t)(*calls & 1u) : 0;  // the call's gate word (held: `pair`)
    const mmp_place_caller C = o.caller ? *o.caller : mmp_place_caller{};
    switch (r) {
    case PlaceRoute::memo_split:
        hipLaunchKernelGGL(place_memo_kernel, dim3(grid), block, lds_memo, st, S, A, words, cap, par);
        if (tail) hipLaunchKernelGGL(place_tail_kernel, tails, tail_block, lds_tail, st, S, A, wpad, words, cap, par, report);
        break;
    case PlaceRoute::memo_split_c:
        hipLaunchKernelGGL(place_memo_c_kernel, dim3(grid), block, lds_memo, st, S, A, words, cap, par, C);
        if (tail) hipLaunchKernelGGL(place_tail_c_kernel, tails, tail_block, lds_tail, st, S, A, wpad, words, cap, par, report, C);
        break;
    case PlaceRoute::multi: hipLaunchKernelGGL(place_multi_kernel, dim3(o.seg_blocks), block, lds, st, S, A, wpad, *o.segs); break;
    case PlaceRoute::multi_m: hipLaunchKernelGGL(place_multi_m_kernel, dim3(o.seg_blocks), block, lds_nobar, st, S, A, wpad, *o.segs); break;
    case PlaceRoute::multi_long: hipLaunchKernelGGL(place_multi_long_kernel, dim3(o.seg_blocks), block, lds, st, S, A, wpad, *o.segs); break;
    case PlaceRoute::multi_long4: hipLaunchKernelGGL(place_multi_long4_kernel, dim3(o.seg_blocks), block, lds, st, S, A, wpad, *o.segs); break;
    case PlaceRoute::miss_single:
        hipLaunchKernelGGL(miss_single_kernel, dim3(1), dim3(128), lds, st, S, A, wpad, *o.inline_req, *o.fused_gate, *o.fused_greq);
        break;
    case PlaceRoute::single_lean: hipLaunchKernelGGL(place_single_lean_kernel, dim3(1), dim3(64), lds, st, S, A, wpad, *o.inline_req); break;
    case PlaceRoute::flag: hipLaunchKernelGGL(place_batch_flag_kernel, dim3(grid), block, lds, st, S, A, wpad, o.done_blocks); break;
    case PlaceRoute::batch: hipLaunchKernelGGL(place_batch_kernel, dim3(grid), block, lds, st, S, A, wpad); break;
    case PlaceRoute::batch_m: hipLaunchKernelGGL(place_batch_m_kernel, dim3(grid), block, lds_nobar, st, S, A, wpad); break;
    case PlaceRoute::batch_c: hipLaunchKernelGGL(place_batch_c_kernel, dim3(grid), block, lds, st, S, A, wpad, C); break;
    case PlaceRoute::batch_c_m: hipLaunchKernelGGL(place_batch_c_m_kernel, dim3(grid), block, lds_nobar, st, S, A, wpad, C); break;
    case PlaceRoute::batch_long: hipLaunchKernelGGL(place_batch_long_kernel, dim3(grid), block, lds_nobar, st, S, A, wpad); break;
    case PlaceRoute::batch_long4: hipLaunchKernelGGL(place_batch_long4_kernel, dim3(grid), block, lds, st, S, A, wpad); break;
    case PlaceRoute::batch_long_c: hipLaunchKernelGGL(place_batch_long_c_kernel, dim3(grid), block, lds_nobar, st, S, A, wpad, C); break;
    case PlaceRoute::batch_long4_c: hipLaunchKernelGGL(place_batch_long4_c_kernel, dim3(grid), block, lds, st, S, A, wpad, C); break;
    }
    HIP_TRY(c, hipGetLastError());
    if (is_split(r) && tail && calls) ++*calls;  // both launches are on the stream: the next split batch takes the other gate word
    if (is_split(r)) c->n_split.fetch_add(1, std::memory_order_relaxed);
    return MMP_OK;
}

// ---- the request seam: what the fifteen host-pointer request calls share (mmp_place_batch, _place_batch_c, _place_batch_ck, _place_batch_cv,
// _serve_batch, _gate_batch, _miss_batch, _miss_batch_c, _miss_batch_ck, _miss_batch_cv, _route_batch, _route_batch_c, _route_batch_ck,
// _route_batch_cv, _evict_batch) — the range checks, the kernels' argument blocks, and the driver of their two paths ----------

// [off, off + n) lies inside a pool of `len` entries (int64: off + n may pass INT32_MAX)
inline bool in_pool(int32_t off, int32_t n, int32_t len) { return off >= 0 && n >= 0 && (int64_t)off + n <= len; }
int bad_range(mmp_ctx *c, const char *call, int32_t i, const char *pool, int32_t off, int32_t n, int32_t len)
{
    return fail(c, MMP_EINVAL, "%s: request %d %s range [%d, +%d) outside the pool of %d", call, i, pool, off, n, len);
}
// The pool ranges of one request of each request struct, refused before any state is looked at.  Each entry point walks its requests
// once and asks these of request i (inline: a request in range costs the comparisons alone).
template <class Req>  // mmp_place_req, mmp_place_req_c
inline int check_place_req(mmp_ctx *c, const char *call, int32_t i, const Req &r, int32_t n_extra)
{
    return in_pool(r.extra_off, r.n_extra, n_extra) ? MMP_OK : bad_range(c, call, i, "extra", r.extra_off, r.n_extra, n_extra);
}
template <class Req>  // mmp_gate_req, mmp_gate_req_c
inline int check_gate_req(mmp_ctx *c, const char *call, int32_t i, const Req &r, int32_t n_excl, int32_t n_explicit)
{
    if (!in_pool(r.excl_off, r.n_excl, n_excl)) return bad_range(c, call, i, "exclude", r.excl_off, r.n_excl, n_excl);
    if (!in_pool(r.explicit_off, r.n_explicit, n_explicit)) return bad_range(c, call, i, "explicit", r.explicit_off, r.n_explicit, n_explicit);
    return MMP_OK;
}
inline int check_serve_req(mmp_ctx *c, const char *call, int32_t i, const mmp_serve_req &r, int32_t n_excl, int32_t n_counters)
{
    if (!in_pool(r.excl_off, r.n_excl, n_excl)) return bad_range(c, call, i, "exclude", r.excl_off, r.n_excl, n_excl);
    if (!in_pool(r.cnt_off, r.n_cnt, n_counters)) return bad_range(c, call, i, "counter", r.cnt_off, r.n_cnt, n_counters);
    return MMP_OK;
}
// (the compact serve row: its exclusion range IS the gate row's)
inline int check_serve_req(mmp_ctx *c, const char *call, int32_t i, const mmp_serve_req_c &r, int32_t, int32_t n_counters)
{
    return in_pool(r.cnt_off, r.n_cnt, n_counters) ? MMP_OK : bad_range(c, call, i, "counter", r.cnt_off, r.n_cnt, n_counters);
}
// the two halves of one request (mmp_miss_batch, mmp_route_batch) name one model
inline int check_same_model(mmp_ctx *c, const char *call, int32_t i, int32_t gate_model, int32_t other_model)
{
    return gate_model == other_model ? MMP_OK : fail(c, MMP_EINVAL, "%s: request %d names two models", call, i);
}

// The state a decision call reads, looked at under the lock it launches under (seam_run).  whole_table: not on a pod-axis shard
// context, whose snapshot holds a slice of the instances only (the load targets go through mmp_shard_place_phase_dev there).
int need_snapshot(mmp_ctx *c, bool whole_table)
{
    if (!c->committed) return fail(c, MMP_ESTATE, "no committed snapshot");
    if (whole_table && c->n_shards > 0) return fail(c, MMP_ESTATE, "context is a pod-axis shard (the mmp_shard_* calls decide there)");
    return MMP_OK;
}

// The kernels' argument blocks as far as the context fills them; the caller binds its own arrays and the completion flag.
GateArgs gate_args(mmp_ctx *c, int32_t n, int64_t now, int64_t in_use_expiry)
{
    GateArgs A{};
    A.models = c->models.as<mmp_model_row>();
    A.ent_pod = c->ent_pod.as<int32_t>();
    A.ent_time = c->ent_time.as<int64_t>();
    A.pods = c->sb[c->cur].pods.as<mmp_pod_row>();
    A.allowed = cur_side(c).d_allowed.as<uint64_t>();
    A.has_allowed = cur_side(c).d_has_allowed.as<uint8_t>();
    A.stats = cur_side(c).stats_acc.as<StatsAcc>();
    A.tstats = cur_side(c).tstats.as<StatsAcc>();
    A.T_rows = std::max(c->n_types, 1);
    A.n = n;
    A.n_models = c->n_models;
    A.P = c->snap.P;
    A.W = c->snap.W;
    A.T = c->n_types;
    A.now = now;
    A.in_use_expiry = in_use_expiry;
    A.min_space = c->cfg.min_space_units;
    A.min_churn = c->cfg.min_churn_age_ms;
    A.done = DoneFlag{nullptr, nullptr, 0};
    return A;
}
ServeArgs serve_args(mmp_ctx *c, int32_t n, int64_t now)
{
    ServeArgs A{};
    A.models = c->models.as<mmp_model_row>();
    A.ent_pod = c->ent_pod.as<int32_t>();
    A.ent_time = c->ent_time.as<int64_t>();
    A.n = n;
    A.n_models = c->n_models;
    A.P = c->snap.P;
    A.now = now;
    A.done = DoneFlag{nullptr, nullptr, 0};
    return A;
}
EvictArgs evict_args(mmp_ctx *c, int32_t n, int64_t now)
{
    EvictArgs A;  // (every field is set: the arrays and the flag by the caller)
    A.seg_off = c->c_seg.as<int32_t>();
    A.last_used = c->c_lu.as<int64_t>();
    A.weight = c->c_wt.as<int32_t>();
    A.capacity = c->c_cap.as<int64_t>();
    A.n = n;
    A.n_caches = c->n_caches;
    A.now = now;
    A.done = DoneFlag{nullptr, nullptr, 0};
    return A;
}
// eight lanes per evaluation while the deques are short, sixteen otherwise (aux_kernels.hpp)
void evict_launch(mmp_ctx *c, const EvictArgs &A, int32_t n, hipStream_t st)
{
    if (c->cache_entries <= (int64_t)24 * std::max(c->n_caches, 1))
        hipLaunchKernelGGL(evict_batch_kernel<8>, dim3(div_up(n, kEvBlock / 8)), dim3(kEvBlock), 0, st, A);
    else
        hipLaunchKernelGGL(evict_batch_kernel<16>, dim3(div_up(n, kEvBlock / 16)), dim3(kEvBlock), 0, st, A);
}

// One input or output array of a request call: the caller's array, its region of a slot (the layout table beside FastSlot), and the
// scratch buffer that stages it when the call does not ride a slot.
struct SeamIo {
    void *host;  // (an input is only read)
    size_t bytes;
    SlotRegion at;
    DevBuf *stage;
    void *dev = nullptr;  // where the kernels find it: seam_run sets it before the launch body runs
    template <class T>
    T *as() const { return static_cast<T *>(dev); }
};
template <class T>
SeamIo seam_io(const T *host, int32_t count, const SlotRegion &at, DevBuf &stage)
{
    return SeamIo{const_cast<T *>(host), (size_t)count * sizeof(T), at, &stage};
}
template <class T>  // an array of a call that always rides a slot
SeamIo seam_io(const T *host, int32_t count, const SlotRegion &at)
{
    return SeamIo{const_cast<T *>(host), (size_t)count * sizeof(T), at, nullptr};
}
// The input or the output arrays of a call, as seam_run takes them: a braced list, or a fixed-size array a caller put together
// (seam_list: a seam's own arrays with a resolver's behind them).  It is a view: the list lives as long as the call's expression.
struct SeamSpan {
    SeamIo *const *first;
    size_t count;
    SeamSpan(std::initializer_list<SeamIo *> l) : first(l.begin()), count(l.size()) {}
    template <size_t N>
    SeamSpan(const std::array<SeamIo *, N> &a) : first(a.data()), count(N) {}
    SeamIo *const *begin() const { return first; }
    SeamIo *const *end() const { return first + count; }
};
template <size_t N, class... Io>
std::array<SeamIo *, sizeof...(Io) + N> seam_list(const std::array<SeamIo *, N> &behind, Io *...own)
{
    std::array<SeamIo *, sizeof...(Io) + N> a{own...};
    for (size_t i = 0; i < N; i++) a[sizeof...(Io) + i] = behind[i];
    return a;
}
inline void *slot_ptr(FastSlot *f, const SlotRegion &r)
{
    char *base = r.buf == kSlotReq ? reinterpret_cast<char *>(f->reqs) : r.buf == kSlotPool ? reinterpret_cast<char *>(f->extra) : reinterpret_cast<char *>(f->outs);
    return base + r.off;
}

// The two paths of a request call.  `check()` refuses the call when the state it needs is not there; `launch(stream, done, on_slot)`
// binds the arrays' device addresses (SeamIo::dev) and enqueues the kernels, the last of them announcing `done`; on_slot is
// std::true_type on the latency path, so what a body does there only costs nothing elsewhere.

// The latency path (slot_acquire): the arrays are copied into the slot's pinned, device-mapped buffers, the kernels run on the slot's
// own stream and the host spins on the slot's completion flag: no staging copies, no batch lock, no kernel timing.  The state lock is
// held SHARED over check, the sequence number's bump and the enqueue — quiesce_decisions relies on that.  The number is bumped before
// the body runs: a body that fails leaves it ahead of every kernel, which costs the next quiescer a stream synchronisation (slot_wait's
// fallback) and never hides a kernel in flight.  Inlined into each entry point: the array lists are unrolled and the regions' addresses
// folded there.
template <class Check, class Launch>
__attribute__((always_inline)) inline int seam_slot(mmp_ctx *c, SeamSpan ins, SeamSpan outs, Check &check, Launch &launch)
{
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    std::unique_lock<std::mutex> fl;
    FastSlot *f = slot_acquire(c, fl);
    for (SeamIo *io : ins) {
        io->dev = slot_ptr(f, io->at);
        if (io->bytes) memcpy(io->dev, io->host, io->bytes);
    }
    for (SeamIo *io : outs) io->dev = slot_ptr(f, io->at);
    {
        std::shared_lock<std::shared_mutex> g(c->mu);  // capture the published state + enqueue
        if (const int rc = check()) return rc;
        if (const int rc = launch(f->stream, DoneFlag{f->done, f->blocks, ++f->seq}, std::true_type{})) return rc;
    }
    HIP_TRY(c, slot_wait(f, f->seq.load(std::memory_order_relaxed)));
    for (SeamIo *io : outs) memcpy(io->host, io->dev, io->bytes);
    return MMP_OK;
}

// The staged path, n == 0 included: batch_mu owns c->stream and the scratch for the whole call, and every writer of the state the
// call reads (commit, the loaders, registry events) takes it too: the published snapshot cannot change underneath, so the state is
// checked first.  The state lock c->mu is NOT held, so that latency-path calls keep flowing — except by the place calls
// (kLaunchExcl; they answer n == 0 themselves), which hold it exclusive over their check and place_launch.  Kernel time (KT_*)
// brackets the launches alone, not the copies.
template <bool kLaunchExcl, class Check, class Launch>
__attribute__((noinline)) int seam_staged(mmp_ctx *c, int32_t n, SeamSpan ins, SeamSpan outs, Check &check, Launch &launch)
{
    std::lock_guard<std::mutex> gb(c->batch_mu);
    if constexpr (!kLaunchExcl)
        if (const int rc = check()) return rc;
    if (n == 0) return MMP_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    for (const auto &side : {ins, outs})
        for (SeamIo *io : side) {
            HIP_TRY(c, io->stage->ensure(std::max<size_t>(io->bytes, 1)));  // (an empty pool still gets an address)
            io->dev = io->stage->p;
        }
    for (SeamIo *io : ins)
        if (io->bytes) HIP_TRY(c, hipMemcpyAsync(io->dev, io->host, io->bytes, hipMemcpyHostToDevice, st));
    {
        std::unique_lock<std::shared_mutex> g(c->mu, std::defer_lock);
        if constexpr (kLaunchExcl) {
            g.lock();
            if (const int rc = check()) return rc;
        }
        KT_BEGIN(c, st);
        if (const int rc = launch(st, DoneFlag{nullptr, nullptr, 0}, std::false_type{})) return rc;
        KT_END(c, st);
    }
    for (SeamIo *io : outs) HIP_TRY(c, hipMemcpyAsync(io->host, io->dev, io->bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    kt_collect(c);
    return MMP_OK;
}

template <bool kLaunchExcl, class Check, class Launch>
__attribute__((always_inline)) inline int seam_run(mmp_ctx *c, int32_t n, bool rides_slot, SeamSpan ins, SeamSpan outs, Check &&check,
                                                   Launch &&launch)
{
    return rides_slot ? seam_slot(c, ins, outs, check, launch) : seam_staged<kLaunchExcl>(c, n, ins, outs, check, launch);
}

}  // namespace

extern "C" {

int mmp_abi_version(void) { return MMP_ABI_VERSION; }

int64_t mmp_min_space_units(int32_t dflt, int32_t threads, int64_t cap_units, int have_unload)
{
    // MM.java:765-771, Java int arithmetic
    const int32_t mn = (int32_t)((uint32_t)dflt * ((have_unload || threads <= 1) ? 1u : 2u));
    const int32_t a = (int32_t)((uint32_t)dflt * (uint32_t)threads);
    const int32_t b = (int32_t)(cap_units / 20);
    const int32_t target = a < b ? a : b;
    return mn > target ? mn : target;
}

int mmp_create(const mmp_config *cfg, mmp_ctx **out)
{
    if (!cfg || !out) return fail(nullptr, MMP_EINVAL, "mmp_create: null argument");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, MMP_ENODEVICE, "no HIP device available (%s); libmmplace has no CPU path",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(nullptr, MMP_EINVAL, "device %d out of range (have %d)", cfg->device, ndev);
    if ((e = hipSetDevice(cfg->device)) != hipSuccess)
        return fail(nullptr, MMP_EHIP, "hipSetDevice: %s", hipGetErrorString(e));
    mmp_ctx *c = new (std::nothrow) mmp_ctx();
    if (!c) return fail(nullptr, MMP_ENOMEM, "out of memory");
    c->cfg = *cfg;
    {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, cfg->device) == hipSuccess && v > 0) c->lds_limit = (size_t)v;
    }
    c->tune = read_tuning();  // per context: tests change the environment between contexts
    {
        // the one-launch plan waits at grid-wide barriers: every workgroup has to be on the chip (one per compute unit at most);
        // it keeps the bucket offsets in 64 KB of dynamic LDS beside its 23 KB of static
        int cus = 0, per_cu = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg->device) == hipSuccess && cus > 0 &&
            hipFuncSetAttribute(reinterpret_cast<const void *>(proactive_plan_fused_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)kPlanFusedLds) == hipSuccess &&
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, proactive_plan_fused_kernel, kPlanFusedBlock, kPlanFusedLds) == hipSuccess &&
            per_cu > 0)
            c->plan_grid_max = std::min(cus, kPlanFusedGrid);
        (void)hipGetLastError();
    }
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) {
        delete c;
        return fail(nullptr, MMP_EHIP, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    if ((e = hipEventCreateWithFlags(&c->reg_event, hipEventDisableTiming)) != hipSuccess) {
        (void)hipStreamDestroy(c->stream);
        delete c;
        return fail(nullptr, MMP_EHIP, "hipEventCreate: %s", hipGetErrorString(e));
    }
    for (FastSlot &f : c->fast) {
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);  // hi is the numerically lowest = highest priority
        hipError_t e1 = hipStreamCreateWithPriority(&f.stream, hipStreamNonBlocking, hi);
        hipError_t e2 = hipHostMalloc(reinterpret_cast<void **>(&f.reqs), kFastN * sizeof(mmp_place_req), kPinnedFlags);
        hipError_t e3 = hipHostMalloc(reinterpret_cast<void **>(&f.extra), kFastExtra * sizeof(int32_t), kPinnedFlags);
        hipError_t e4 = hipHostMalloc(reinterpret_cast<void **>(&f.outs), kFastN * sizeof(mmp_place_out), kPinnedFlags);
        if (e4 == hipSuccess) e4 = hipHostMalloc(reinterpret_cast<void **>(&f.done), 64, kPinnedFlags);
        if (e4 == hipSuccess) *f.done = 0;
        if (e4 == hipSuccess) e4 = hipMalloc(reinterpret_cast<void **>(&f.blocks), 64);
        if (e4 == hipSuccess) e4 = hipMemsetAsync(f.blocks, 0, 64, c->stream);
        if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess || e4 != hipSuccess) {
            mmp_destroy(c);
            return fail(nullptr, MMP_EHIP, "fast-slot allocation failed");
        }
    }
    (void)hipStreamSynchronize(c->stream);
    *out = c;
    if (c->tune.resident && mmp_resident(c, 1) != MMP_OK) {
        *out = nullptr;
        mmp_destroy(c);
        return fail(nullptr, MMP_EHIP, "the resident decision kernel could not be set up");
    }
    return MMP_OK;
}

namespace {
void group_comm_destroy(ncclComm_t comm);  // defined with the RCCL binding below
}
extern "C" int mmp_issue_threads(mmp_ctx *c, int32_t n);
extern "C" int mmp_resident(mmp_ctx *c, int enable);
namespace {
void resident_stop(mmp_ctx *c);
}

void mmp_destroy(mmp_ctx *c)
{
    if (!c) return;
    (void)mmp_issue_threads(c, 0);  // launches still in the rings are issued, the helpers join
    (void)hipSetDevice(c->cfg.device);
    resident_stop(c);
    if (c->res.stream) (void)hipStreamDestroy(c->res.stream);
    if (c->res.slots) (void)hipHostFree(c->res.slots);
    if (c->res.ctl) (void)hipHostFree(c->res.ctl);
    if (c->res.answers) (void)hipHostFree(c->res.answers);
    c->res.slots = nullptr;
    for (FastSlot &f : c->fast) {
        if (f.stream) {
            (void)hipStreamSynchronize(f.stream);
            (void)hipStreamDestroy(f.stream);
        }
        if (f.reqs) (void)hipHostFree(f.reqs);
        if (f.done) (void)hipHostFree(f.done);
        if (f.blocks) (void)hipFree(f.blocks);
        if (f.extra) (void)hipHostFree(f.extra);
        if (f.outs) (void)hipHostFree(f.outs);
    }

    if (c->stream) (void)hipStreamSynchronize(c->stream);  // (an asynchronous pod-axis batch may still be writing its count)
    if (c->f_done) (void)hipHostFree(c->f_done);
    if (c->comm) {
        group_comm_destroy(c->comm);
        c->comm = nullptr;
    }
    for (DevBuf *b : {&c->g_rankbuf, &c->g_xf[0], &c->g_xf[1], &c->g_x[0], &c->g_x[1], &c->g_x[2], &c->g_x[3], &c->g_x[4], &c->g_x[5]}) b->release();
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->reg_event) (void)hipEventDestroy(c->reg_event);
    if (c->pe0) (void)hipEventDestroy(c->pe0);
    if (c->pe1) (void)hipEventDestroy(c->pe1);
    c->sb[0].release();
    c->sb[1].release();
    c->side[0].release();
    c->side[1].release();
    // (caller-owned streams a split batch ran on are the caller's to drain before it destroys the context, as for every *_dev call)
    for (auto &mb : c->miss_bufs)
        if (mb.words) (void)hipFree(mb.words);
    for (void *p : c->miss_retired) (void)hipFree(p);
    if (c->miss_reports) (void)hipHostFree(c->miss_reports);
    for (DevBuf *b : {&c->rank, &c->occupancy, &c->flag, &c->rs_list, &c->rs_bad, &c->d_prefer,
                      &c->models, &c->ent_pod, &c->ent_time, &c->c_seg,
                      &c->c_lu, &c->c_wt, &c->c_cap, &c->s_reqs, &c->s_outs, &c->s_extra, &c->s_a, &c->s_b,
                      &c->s_c, &c->s_d, &c->r_ps, &c->r_counts, &c->r_keys, &c->r_vals, &c->r_keys2, &c->r_vals2,
                      &c->r_tmp, &c->r_part, &c->rs_split, &c->rs_int, &c->r_out_model, &c->r_out_lu, &c->rt_sreqs, &c->rt_souts, &c->rt_cnt, &c->k_ids, &c->k_cap, &c->k_wsize, &c->k_oldest, &c->k_ubm, &c->k_ops, &c->k_order,
                      &c->k_opoff, &c->k_outs, &c->k_ev, &c->k_evoff, &c->k_inv, &c->k_kstat, &c->k_krow, &c->k_len, &c->k_goff, &c->k_gbytes, &c->idtab_hash, &c->idtab_val, &c->tytab_hash,
                      &c->tytab_val, &c->j_buf, &c->j_off, &c->j_rows, &c->j_aux, &c->j_status, &c->j_cnt, &c->j_offs, &c->j_tmp_pod, &c->idd_bytes, &c->idd_off, &c->rw_rows, &c->rw_lul, &c->rw_fpod, &c->rw_fmsg, &c->rw_fmoff, &c->rw_len,
                      &c->rw_off, &c->rw_status, &c->rw_out, &c->rg_reqs, &c->rg_info, &c->rg_ioff, &c->rg_cls, &c->rg_lu, &c->rf_refs, &c->vw_reqs, &c->vw_strs, &c->vw_soff, &c->vw_rows,
                      &c->vid_hash, &c->vid_val, &c->vid_next_hash, &c->vid_next_val, &c->vid_bytes, &c->vid_off, &c->vm_rows, &c->vm_rows_next, &c->vm_arena,
                      &c->vq_nf, &c->vq_nf_off, &c->vq_flags, &c->vq_out,
                      &c->vm_ev, &c->vm_cnt, &c->vm_pos, &c->vm_nf_bytes, &c->vm_nf_off, &c->vm_ow_bytes, &c->vm_ow_off, &c->vm_rflags,
                      &c->vm_ans, &c->vm_list,
                      &c->j_tmp_time, &c->j_scan_tmp, &c->j_ev, &c->rk_rows, &c->rk_idx, &c->rk_tmp, &c->u_idx, &c->u_rows, &c->u_cnt, &c->u_offs, &c->u_tmp, &c->miss_since, &c->p_state, &c->p_seen, &c->plan.totals, &c->plan.block_counts, &c->plan.edits, &c->p_removed, &c->plan.keep_off, &c->plan.model_map, &c->plan.rows_in, &c->plan.call_scalars, &c->plan.row_tmp, &c->cn_out, &c->st_copies, &c->sk_fpod, &c->sk_flags, &c->sk_sc, &c->sk_str, &c->idtab_next_hash, &c->idtab_next_val, &c->ida_bytes, &c->ida_off, &c->ida_hash, &c->ida_found, &c->unres_list, &c->kq_keys, &c->kq_off, &c->kq_idx, &c->kq_preqs, &c->kq_pouts, &c->mid_hash, &c->mid_val, &c->mid_next_hash, &c->mid_next_val, &c->mid_bytes, &c->mid_off, &c->me_hash, &c->me_row, &c->me_slot, &c->me_tab, &c->me_cnt, &c->me_pos, &c->me_idx, &c->me_join, &c->me_found, &c->ret_rows, &c->ret_keep, &c->ret_remap, &c->ret_word, &c->f_flags[0], &c->f_flags[1], &c->f_offs, &c->f_idx, &c->f_reqs, &c->f_outs, &c->f_scan_tmp, &c->f_cnt[0], &c->f_cnt[1],
                      &c->ks[0].off, &c->ks[0].lu, &c->ks[0].wt,
                      &c->ks[0].key, &c->ks[0].n, &c->ks[1].off, &c->ks[1].lu, &c->ks[1].wt, &c->ks[1].key, &c->ks[1].n})
        b->release();
    delete c;
}

const char *mmp_last_error(mmp_ctx *) { return g_thread_err.c_str(); }

int mmp_backend(mmp_ctx *c) { return c ? 1 : 0; }

int mmp_profile(mmp_ctx *c, int enable)
try {
    if (!c) return MMP_EINVAL;
    std::lock_guard<std::mutex> gb(c->batch_mu);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    if (enable && !c->pe0) {
        HIP_TRY(c, hipEventCreate(&c->pe0));
        HIP_TRY(c, hipEventCreate(&c->pe1));
    }
    c->prof = enable != 0;
    c->last_kernel_ms = -1.0;
    return MMP_OK;
} MMP_CATCH(c, "mmp_backend")

double mmp_last_kernel_ms(mmp_ctx *c) { return c ? c->last_kernel_ms : -1.0; }

int mmp_sync(mmp_ctx *c)
try {
    if (!c) return MMP_EINVAL;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MMP_OK;
} MMP_CATCH(c, "mmp_sync")

/* ---- staging of the instance table -------------------------------------- */

namespace {
// a row written since the last commit; a long list is as good as "everything" (a context that never commits must not grow it)
inline void note_dirty(mmp_ctx *c, int32_t k)
{
    if (c->dirty_all) return;
    if (c->dirty.size() >= (size_t)8 * kDeltaRows) {
        c->dirty_all = true;
        c->dirty.clear();
        return;
    }
    c->dirty.push_back(k);
}

// the label state is as long as the staged instance table: indices that remain keep their word, new ones carry none
inline void labels_cover(mmp_ctx *c)
{
    c->pod_label_word.resize(c->pods.size(), 0);
    c->pod_label_count.resize(c->pods.size(), 0);
}
}  // namespace

int mmp_pods_load(mmp_ctx *c, const mmp_pod_row *rows, int32_t n)
try {
    if (!c || n < 0 || (n > 0 && !rows)) return fail(c, MMP_EINVAL, "mmp_pods_load: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    c->pods.assign(rows, rows + n);
    labels_cover(c);
    c->dirty_all = true;
    return MMP_OK;
} MMP_CATCH(c, "mmp_pods_load")

int mmp_pods_upsert(mmp_ctx *c, const int32_t *idx, const mmp_pod_row *rows, int32_t n)
try {
    if (!c || n < 0 || (n > 0 && (!rows || !idx))) return fail(c, MMP_EINVAL, "mmp_pods_upsert: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    {  // all of the call or none of it: a bad index must not leave the rows before it applied
        int32_t count = (int32_t)c->pods.size();
        for (int32_t i = 0; i < n; i++) {
            if (idx[i] < 0 || idx[i] > count) return fail(c, MMP_EINVAL, "mmp_pods_upsert: index %d out of range", idx[i]);
            if (idx[i] == count) count++;
        }
    }
    for (int32_t i = 0; i < n; i++) {
        const int32_t k = idx[i];
        if (k == (int32_t)c->pods.size()) {
            c->pods.push_back(rows[i]);
            labels_cover(c);
            c->dirty_all = true;
        } else {
            c->pods[k] = rows[i];
            note_dirty(c, k);
        }
    }
    return MMP_OK;
} MMP_CATCH(c, "mmp_pods_upsert")

int mmp_pods_remove(mmp_ctx *c, const int32_t *idx, int32_t n)
try {
    if (!c || n < 0 || (n > 0 && !idx)) return fail(c, MMP_EINVAL, "mmp_pods_remove: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    for (int32_t i = 0; i < n; i++)  // (all of the call or none of it)
        if (idx[i] < 0 || idx[i] >= (int32_t)c->pods.size()) return fail(c, MMP_EINVAL, "mmp_pods_remove: index %d out of range", idx[i]);
    for (int32_t i = 0; i < n; i++) {
        const int32_t k = idx[i];
        c->pods[k].flags |= MMP_POD_TOMBSTONE;
        c->pods[k].flags &= ~MMP_POD_LIVE;
        note_dirty(c, k);
    }
    return MMP_OK;
} MMP_CATCH(c, "mmp_pods_remove")

int mmp_types_load(mmp_ctx *c, int32_t n_types, const uint64_t *allowed, const uint64_t *prefer,
                   const uint8_t *has_allowed, const uint8_t *has_prefer)
try {
    if (!c || n_types < 0) return fail(c, MMP_EINVAL, "mmp_types_load: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    const int32_t W = div_up((int)c->pods.size(), 64);
    c->n_types = n_types;
    c->types_w = W;
    c->sig_valid = false;
    c->types_gen++;
    const size_t words = (size_t)n_types * W;
    c->allowed.assign(words, 0);
    c->prefer.assign(words, 0);
    c->has_allowed.assign(std::max(n_types, 1), 0);
    c->has_prefer.assign(std::max(n_types, 1), 0);
    for (int32_t t = 0; t < n_types; t++) {
        if (has_allowed && has_allowed[t]) {
            if (!allowed) return fail(c, MMP_EINVAL, "mmp_types_load: allowed bitmap missing");
            c->has_allowed[t] = 1;
            std::copy(allowed + (size_t)t * W, allowed + (size_t)(t + 1) * W, c->allowed.begin() + (size_t)t * W);
        }
        if (has_prefer && has_prefer[t]) {
            if (!prefer) return fail(c, MMP_EINVAL, "mmp_types_load: prefer bitmap missing");
            c->has_prefer[t] = 1;
            std::copy(prefer + (size_t)t * W, prefer + (size_t)(t + 1) * W, c->prefer.begin() + (size_t)t * W);
        }
    }
    return MMP_OK;
} MMP_CATCH(c, "mmp_types_load")

namespace {
// The body of mmp_types_from_labels and mmp_types_from_pod_labels (batch_mu and the state lock held): pod_labels[P] is the
// caller's array or the resident words.
int types_from_labels_locked(mmp_ctx *c, int32_t n_types, const uint64_t *required, const uint64_t *preferred,
                             const uint64_t *pod_labels, uint64_t *allowed_out, uint64_t *prefer_out, uint8_t *has_allowed_out,
                             uint8_t *has_prefer_out)
{
    const int32_t P = (int32_t)c->pods.size();
    const int32_t W = div_up(P, 64), T = n_types, R = T + 1;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    const size_t words = (size_t)std::max(R * W, 1);
    // scratch: pods, labels, required, preferred, allowed, cpref, prefer, score, has_*
    HIP_TRY(c, c->s_reqs.ensure((size_t)std::max(P, 1) * sizeof(mmp_pod_row)));
    HIP_TRY(c, c->s_a.ensure((size_t)std::max(P, 1) * 8));
    HIP_TRY(c, c->s_b.ensure((size_t)std::max(T, 1) * 16));
    HIP_TRY(c, c->s_c.ensure(words * 8 * 3));
    HIP_TRY(c, c->s_d.ensure((size_t)std::max(P, 1) * 4 + (size_t)R * 2));
    uint64_t *d_req = c->s_b.as<uint64_t>(), *d_prf = d_req + std::max(T, 1);
    uint64_t *d_al = c->s_c.as<uint64_t>(), *d_cp = d_al + words, *d_pf = d_cp + words;
    int32_t *d_score = c->s_d.as<int32_t>();
    uint8_t *d_ha = reinterpret_cast<uint8_t *>(d_score + std::max(P, 1)), *d_hp = d_ha + R;
    if (P) {
        HIP_TRY(c, hipMemcpyAsync(c->s_reqs.p, c->pods.data(), (size_t)P * sizeof(mmp_pod_row), hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipMemcpyAsync(c->s_a.p, pod_labels, (size_t)P * 8, hipMemcpyHostToDevice, st));
    }
    if (T) {
        HIP_TRY(c, hipMemcpyAsync(d_req, required, (size_t)T * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipMemcpyAsync(d_prf, preferred, (size_t)T * 8, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(c, hipMemsetAsync(d_al, 0, words * 8 * 3, st));
    if (W > 0) {
        hipLaunchKernelGGL(type_sets_kernel, dim3(div_up(W, 4)), dim3(256), 0, st, c->s_reqs.as<mmp_pod_row>(),
                           c->s_a.as<uint64_t>(), P, W, T, d_req, d_prf, d_al, d_cp, d_score);
    }
    hipLaunchKernelGGL(type_prefer_kernel, dim3(R), dim3(256), 0, st, P, W, T, d_req, d_al, d_cp, d_score, d_pf, d_ha, d_hp);
    HIP_TRY(c, hipGetLastError());
    // install as the type table of the next commit (same staging the host-bitmap entry point fills)
    c->n_types = R;
    c->types_w = W;
    c->sig_valid = false;
    c->types_gen++;
    c->allowed.assign((size_t)R * W, 0);
    c->prefer.assign((size_t)R * W, 0);
    c->has_allowed.assign(R, 0);
    c->has_prefer.assign(R, 0);
    if (W > 0) {
        HIP_TRY(c, hipMemcpyAsync(c->allowed.data(), d_al, (size_t)R * W * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(c->prefer.data(), d_pf, (size_t)R * W * 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(c, hipMemcpyAsync(c->has_allowed.data(), d_ha, R, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(c->has_prefer.data(), d_hp, R, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (allowed_out && W > 0) memcpy(allowed_out, c->allowed.data(), (size_t)R * W * 8);
    if (prefer_out && W > 0) memcpy(prefer_out, c->prefer.data(), (size_t)R * W * 8);
    if (has_allowed_out) memcpy(has_allowed_out, c->has_allowed.data(), R);
    if (has_prefer_out) memcpy(has_prefer_out, c->has_prefer.data(), R);
    return MMP_OK;
}
}  // namespace

int mmp_types_from_labels(mmp_ctx *c, int32_t n_types, const uint64_t *required, const uint64_t *preferred,
                          const uint64_t *pod_labels, uint64_t *allowed_out, uint64_t *prefer_out,
                          uint8_t *has_allowed_out, uint8_t *has_prefer_out)
try {
    if (!c || n_types < 0 || (n_types > 0 && (!required || !preferred)))
        return fail(c, MMP_EINVAL, "mmp_types_from_labels: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    if (!c->pods.empty() && !pod_labels) return fail(c, MMP_EINVAL, "mmp_types_from_labels: pod_labels is null");
    return types_from_labels_locked(c, n_types, required, preferred, pod_labels, allowed_out, prefer_out, has_allowed_out, has_prefer_out);
} MMP_CATCH(c, "mmp_types_from_labels")

int mmp_types_from_pod_labels(mmp_ctx *c, int32_t n_types, const uint64_t *required, const uint64_t *preferred, uint64_t *allowed_out,
                              uint64_t *prefer_out, uint8_t *has_allowed_out, uint8_t *has_prefer_out)
try {
    if (!c || n_types < 0 || (n_types > 0 && (!required || !preferred)))
        return fail(c, MMP_EINVAL, "mmp_types_from_pod_labels: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    labels_cover(c);
    return types_from_labels_locked(c, n_types, required, preferred, c->pod_label_word.data(), allowed_out, prefer_out, has_allowed_out,
                                    has_prefer_out);
} MMP_CATCH(c, "mmp_types_from_pod_labels")

int mmp_pod_labels_set(mmp_ctx *c, const int32_t *idx, const uint64_t *words, const int32_t *counts, int32_t n)
try {
    if (!c || n < 0 || (n > 0 && (!idx || !words || !counts))) return fail(c, MMP_EINVAL, "mmp_pod_labels_set: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    labels_cover(c);
    for (int32_t i = 0; i < n; i++) {  // (all of the call or none of it)
        if (idx[i] < 0 || idx[i] >= (int32_t)c->pods.size()) return fail(c, MMP_EINVAL, "mmp_pod_labels_set: index %d out of range", idx[i]);
        if (counts[i] < 0) return fail(c, MMP_EINVAL, "mmp_pod_labels_set: count %d of entry %d", counts[i], i);
    }
    for (int32_t i = 0; i < n; i++) {
        c->pod_label_word[idx[i]] = words[i];
        c->pod_label_count[idx[i]] = counts[i];
    }
    return MMP_OK;
} MMP_CATCH(c, "mmp_pod_labels_set")

int mmp_pod_labels_get(mmp_ctx *c, uint64_t *words_out, int32_t *counts_out, int32_t max_pods, int32_t *n_out)
try {
    if (!c || !n_out || max_pods < 0) return fail(c, MMP_EINVAL, "mmp_pod_labels_get: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    labels_cover(c);
    *n_out = (int32_t)c->pods.size();
    const int32_t m = std::min(*n_out, max_pods);
    if (words_out && m > 0) memcpy(words_out, c->pod_label_word.data(), (size_t)m * 8);
    if (counts_out && m > 0) memcpy(counts_out, c->pod_label_count.data(), (size_t)m * 4);
    return MMP_OK;
} MMP_CATCH(c, "mmp_pod_labels_get")

int mmp_replaced_rs_load(mmp_ctx *c, const int32_t *rs, int32_t n)
try {
    if (!c || n < 0 || (n > 0 && !rs)) return fail(c, MMP_EINVAL, "mmp_replaced_rs_load: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    c->replaced_rs.assign(rs, rs + n);
    return MMP_OK;
} MMP_CATCH(c, "mmp_replaced_rs_load")

static void publish_upgrades(mmp_ctx *c)
{
    c->replaced_rs.clear();
    for (auto &e : c->upgrades.replaced) c->replaced_rs.push_back(e.first);
}

int mmp_upgrade_instance_added(mmp_ctx *c, int64_t labels_key, int32_t rs, int64_t start_time, int64_t now)
try {
    if (!c) return MMP_EINVAL;
    std::lock_guard<std::mutex> gb(c->batch_mu);  // replaced_rs is an input of the commit
    std::lock_guard<std::shared_mutex> g(c->mu);
    c->upgrades.instance_added(labels_key, rs, start_time, now);
    publish_upgrades(c);
    return MMP_OK;
} MMP_CATCH(c, "mmp_upgrade_instance_added")

int mmp_upgrade_instance_removed(mmp_ctx *c, int64_t labels_key, int32_t rs, int64_t now)
try {
    if (!c) return MMP_EINVAL;
    std::lock_guard<std::mutex> gb(c->batch_mu);  // replaced_rs is an input of the commit
    std::lock_guard<std::shared_mutex> g(c->mu);
    c->upgrades.instance_removed(labels_key, rs, now);
    publish_upgrades(c);
    return MMP_OK;
} MMP_CATCH(c, "mmp_upgrade_instance_removed")

int mmp_upgrade_housekeeping(mmp_ctx *c, int64_t now)
try {
    if (!c) return MMP_EINVAL;
    std::lock_guard<std::mutex> gb(c->batch_mu);  // replaced_rs is an input of the commit
    std::lock_guard<std::shared_mutex> g(c->mu);
    c->upgrades.housekeeping(now);
    publish_upgrades(c);
    return MMP_OK;
} MMP_CATCH(c, "mmp_upgrade_housekeeping")

int mmp_upgrade_replaced(mmp_ctx *c, int32_t *rs_out, int64_t *expiry_out, int32_t max, int32_t *n_out)
try {
    if (!c || !n_out || max < 0 || (max > 0 && (!rs_out || !expiry_out))) return fail(c, MMP_EINVAL, "mmp_upgrade_replaced: bad argument");
    std::lock_guard<std::shared_mutex> g(c->mu);
    int32_t i = 0;
    for (auto &e : c->upgrades.replaced) {
        if (i < max) {
            rs_out[i] = e.first;
            expiry_out[i] = e.second;
        }
        i++;
    }
    *n_out = i;
    return MMP_OK;
} MMP_CATCH(c, "mmp_upgrade_replaced")

int mmp_models_load(mmp_ctx *c, const mmp_model_row *rows, int32_t n_models, const int32_t *ent_pod,
                    const int64_t *ent_time, int32_t n_entries)
try {
    if (!c || n_models < 0 || n_entries < 0 || (n_models > 0 && !rows) || (n_entries > 0 && (!ent_pod || !ent_time)))
        return fail(c, MMP_EINVAL, "mmp_models_load: bad argument");
    for (int32_t i = 0; i < n_models; i++) {
        const mmp_model_row &m = rows[i];
        if (m.n_loaded < 0 || m.n_failed < 0 || m.ent_off < 0 ||
            (int64_t)m.ent_off + m.n_loaded + m.n_failed > (int64_t)n_entries)
            return fail(c, MMP_EINVAL, "mmp_models_load: model %d entry range out of bounds", i);
    }
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, quiesce_decisions(c));  // the table is overwritten in place
    c->side[0].rmodels_ok = c->side[1].rmodels_ok = false;
    HIP_TRY(c, c->models.ensure((size_t)std::max(n_models, 1) * sizeof(mmp_model_row)));
    HIP_TRY(c, c->ent_pod.ensure((size_t)std::max(n_entries, 1) * sizeof(int32_t)));
    HIP_TRY(c, c->ent_time.ensure((size_t)std::max(n_entries, 1) * sizeof(int64_t)));
    if (n_models) HIP_TRY(c, copy_sync(c, c->models.p, rows, (size_t)n_models * sizeof(mmp_model_row), hipMemcpyHostToDevice));
    if (n_entries) {
        HIP_TRY(c, copy_sync(c, c->ent_pod.p, ent_pod, (size_t)n_entries * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(c, copy_sync(c, c->ent_time.p, ent_time, (size_t)n_entries * sizeof(int64_t), hipMemcpyHostToDevice));
    }
    c->n_models = n_models;
    c->n_entries = n_entries;
    c->m_cnt.resize(n_models);
    c->ent_live = 0;
    for (int32_t i = 0; i < n_models; i++) {
        c->m_cnt[i] = rows[i].n_loaded + rows[i].n_failed;
        c->ent_live += c->m_cnt[i];
    }
    split_reset(c);
    return rebuild_resolved(c);
} MMP_CATCH(c, "mmp_models_load")

namespace {
// grow a device buffer, keeping its first `used` bytes
// Called with c->mu held (shared) right before a kernel that reads the registry (models / resolved rows / entry arena) is
// enqueued on `st`: a registry event whose rewrite kernel is still running on the context's stream is waited for ON THE DEVICE.
hipError_t order_after_registry(mmp_ctx *c, hipStream_t st)
{
    if (!c->reg_pending.load(std::memory_order_acquire) || st == c->stream) return hipSuccess;
    return hipStreamWaitEvent(st, c->reg_event, 0);
}

// Growing a table decisions read, without holding them off for the copy: the new allocation is filled beside the old one
// (batch_mu keeps other writers away), the pointer is swapped under the state lock, and the old allocation is freed once the
// kernels that captured it have drained.  grow_cow fills `fresh` (enqueued on c->stream) where b has to grow, and leaves it
// empty where it has not; the caller publishes it with move_into and drains before `fresh`, then holding the old allocation, ends.
int grow_cow(mmp_ctx *c, const DevBuf &b, size_t used, size_t want, ScopedDevBuf &fresh)
{
    if (want <= b.cap) return MMP_OK;
    HIP_TRY(c, fresh.b.ensure(std::max(want, b.cap * 2)));
    if (used && b.p) HIP_TRY(c, hipMemcpyAsync(fresh.b.p, b.p, used, hipMemcpyDeviceToDevice, c->stream));
    return MMP_OK;
}

int grow_keep(mmp_ctx *c, DevBuf &b, size_t used, size_t want)
{
    if (want <= b.cap) return MMP_OK;
    ScopedDevBuf nb;
    HIP_TRY(c, nb.b.ensure(std::max(want, b.cap * 2)));
    if (used && b.p) HIP_TRY(c, copy_sync(c, nb.b.p, b.p, used, hipMemcpyDeviceToDevice));
    nb.move_into(b);  // (no kernel in flight reads b: the old allocation goes when nb ends)
    return MMP_OK;
}

// squeeze the garbage out of the entry arena (rows keep their order, entries their order inside a row).  Copy-on-write: the rows
// with their new offsets and the squeezed arena are built BESIDE the published ones (called with batch_mu, without the state
// lock: decisions keep reading the old tables), swapped in under the state lock, and the old ones freed when the kernels that
// captured them have drained.  (In place under the lock this held every decision off for the whole rebuild: the 0.4-0.6 ms
// maximum of a single decision under churn in round 3.)
int compact_registry(mmp_ctx *c)
{
    const int32_t n = c->n_models;
    hipStream_t st = c->stream;
    HIP_TRY(c, c->u_cnt.ensure((size_t)(n + 1) * 4));
    HIP_TRY(c, c->u_offs.ensure((size_t)(n + 1) * 4));
    size_t tmp = 0;
    HIP_TRY(c, rocprim::exclusive_scan(nullptr, tmp, c->u_cnt.as<int32_t>(), c->u_offs.as<int32_t>(), (int32_t)0, (size_t)n + 1,
                                       rocprim::plus<int32_t>(), st));
    HIP_TRY(c, c->u_tmp.ensure(std::max<size_t>(tmp, 16)));
    ScopedDevBuf nm, np, nt;
    const size_t cap = (size_t)std::max<int64_t>(c->ent_live + c->ent_live / 2, 1024);
    if (nm.b.ensure(std::max<size_t>(c->models.cap, 16)) != hipSuccess || np.b.ensure(cap * 4) != hipSuccess || nt.b.ensure(cap * 8) != hipSuccess)
        return fail(c, MMP_ENOMEM, "compact_registry: out of device memory");
    hipError_t e = hipMemcpyAsync(nm.b.p, c->models.p, (size_t)n * sizeof(mmp_model_row), hipMemcpyDeviceToDevice, st);
    hipLaunchKernelGGL(model_counts_kernel, dim3(div_up(n + 1, 256)), dim3(256), 0, st, c->models.as<mmp_model_row>(), n,
                       c->u_cnt.as<int32_t>());
    (void)rocprim::exclusive_scan(c->u_tmp.p, tmp, c->u_cnt.as<int32_t>(), c->u_offs.as<int32_t>(), (int32_t)0, (size_t)n + 1,
                                  rocprim::plus<int32_t>(), st);
    hipLaunchKernelGGL(move_entries_kernel, dim3(div_up(std::max(n, 1), 256)), dim3(256), 0, st, nm.b.as<mmp_model_row>(), n,
                       c->u_offs.as<int32_t>(), c->ent_pod.as<int32_t>(), c->ent_time.as<int64_t>(), np.b.as<int32_t>(),
                       nt.b.as<int64_t>());
    const hipError_t se = hipStreamSynchronize(st);  // (whatever was enqueued has finished before the new buffers may go)
    HIP_TRY(c, e != hipSuccess ? e : se);
    {
        std::lock_guard<std::shared_mutex> g(c->mu);  // the swap: three pointers
        nm.move_into(c->models);
        np.move_into(c->ent_pod);
        nt.move_into(c->ent_time);
        c->n_entries = (int32_t)c->ent_live;
    }
    HIP_TRY(c, quiesce_decisions(c));  // kernels that captured the old tables, which go when nm / np / nt end
    return MMP_OK;
}

// Make room for `count` registry rows and `base + n_entries` arena entries (called with batch_mu, by mmp_models_upsert and by an
// applied registry plan, registry_apply_edits, before they append entries at `base`).
int registry_grow(mmp_ctx *c, int32_t count, int32_t base, int32_t n_entries)
{
    hipStream_t st = c->stream;
    // A table that has to grow moves (the old allocation is freed): only then is the state lock needed this early.
    const bool grows = (size_t)count * sizeof(mmp_model_row) > c->models.cap || (size_t)(base + n_entries) * 4 > c->ent_pod.cap ||
                       (size_t)(base + n_entries) * 8 > c->ent_time.cap ||
                       (cur_side(c).rmodels_ok && ((size_t)count * sizeof(ResolvedModel) > cur_side(c).rmodels.cap || (size_t)count * 4 > cur_side(c).mtw.cap));
    if (grows) {  // copy-on-write (grow_cow): decisions are held off for the pointer swap only
        ScopedDevBuf fm, fp, ft, fr, fw;
        int rc = grow_cow(c, c->models, (size_t)c->n_models * sizeof(mmp_model_row), (size_t)count * sizeof(mmp_model_row), fm);
        if (rc == MMP_OK) rc = grow_cow(c, c->ent_pod, (size_t)base * 4, (size_t)(base + n_entries) * 4, fp);
        if (rc == MMP_OK) rc = grow_cow(c, c->ent_time, (size_t)base * 8, (size_t)(base + n_entries) * 8, ft);
        // (the unpublished side's view is rebuilt from the model table by the next commit)
        if (rc == MMP_OK && cur_side(c).rmodels_ok)
            rc = grow_cow(c, cur_side(c).rmodels, (size_t)c->n_models * sizeof(ResolvedModel), (size_t)count * sizeof(ResolvedModel), fr);
        if (rc == MMP_OK && cur_side(c).rmodels_ok) rc = grow_cow(c, cur_side(c).mtw, (size_t)c->n_models * 4, (size_t)count * 4, fw);
        if (rc == MMP_OK && hipStreamSynchronize(st) != hipSuccess) rc = fail(c, MMP_EHIP, "growing the registry tables failed");
        if (rc != MMP_OK) return rc;
        {
            std::lock_guard<std::shared_mutex> g(c->mu);
            fm.move_into(c->models);
            fp.move_into(c->ent_pod);
            ft.move_into(c->ent_time);
            fr.move_into(cur_side(c).rmodels);
            fw.move_into(cur_side(c).mtw);
        }
        HIP_TRY(c, quiesce_decisions(c));  // kernels that captured the old allocations, which go when fm ... fw end
    }
    return MMP_OK;
}

// The in-place rewrite of k registry rows staged in u_idx / u_rows, whose entries already stand in the arena (called with batch_mu):
// afterwards the registry has `count` rows and `n_entries_after` arena entries.  with_count: what else the call publishes in the hold
// of the state lock that publishes the new row count (a by-key event batch: the model-id table that names the new rows).
int registry_rewrite(mmp_ctx *c, int32_t k, int32_t count, int32_t n_entries_after, bool bracket_open = false,
                     const std::function<void()> &with_count = {})
{
    hipStream_t st = c->stream;
    {
        // Rows (and their resolved positions) are rewritten in place.  Under the state lock: the decisions in flight drain, the
        // rewrite kernel is ENQUEUED and an event recorded behind it; decisions launched from now on order themselves behind that
        // event on the device (order_after_registry).  The lock is not held while the kernel runs.
        std::lock_guard<std::shared_mutex> g(c->mu);
        HIP_TRY(c, quiesce_decisions(c));
        const bool resolved = cur_side(c).rmodels_ok && c->committed;
        if (!bracket_open) KT_BEGIN(c, st);  // (registry_apply_edits opened the bracket in front of the plan's build kernel)
        hipLaunchKernelGGL(upsert_models_kernel, dim3(div_up(k, 256)), dim3(256), 0, st, c->snap, c->u_idx.as<int32_t>(),
                           c->u_rows.as<mmp_model_row>(), k, c->ent_pod.as<int32_t>(), c->models.as<mmp_model_row>(),
                           resolved ? cur_side(c).rmodels.as<ResolvedModel>() : nullptr, resolved ? cur_side(c).mtw.as<int32_t>() : nullptr);
        KT_END(c, st);
        // From here on the rewrite may be running.  Nothing may leave this block with the lock released, the rewrite enqueued
        // and no way for later decisions to order themselves behind it: a launch or event error drains the stream first, and
        // the new counts are published only once the event stands.
        hipError_t le = hipGetLastError();
        if (le == hipSuccess) le = hipEventRecord(c->reg_event, st);
        if (le != hipSuccess) {
            (void)hipStreamSynchronize(st);
            HIP_TRY(c, le);
        }
        c->reg_pending.store(true, std::memory_order_release);
        c->n_models = count;
        c->n_entries = n_entries_after;
        if (with_count) with_count();
    }
    const hipError_t se = hipStreamSynchronize(st);
    if (se == hipSuccess) c->reg_pending.store(false, std::memory_order_release);  // (a failed wait leaves later launches ordered behind the event)
    HIP_TRY(c, se);
    kt_collect(c);
    return MMP_OK;
}

// More garbage in the arena than live entries (and enough to matter): squeeze it (called with batch_mu, after a rewrite).
int squeeze_if_garbage(mmp_ctx *c)
{
    return (int64_t)c->n_entries - c->ent_live > std::max<int64_t>(c->ent_live, 1 << 16) ? compact_registry(c) : (int)MMP_OK;
}

// The apply of a registry plan (mmp_registry_prune, mmp_janitor_plan, mmp_registry_ops; called with batch_mu, the evaluation
// collected): the E edited records, n_kept entries in all, are rebuilt at the end of the arena ON THE DEVICE, beyond anything a
// published row refers to; then the rows are rewritten in place exactly as a registry event's are (registry_rewrite).
// launch_build(base, arena_end) only enqueues the call's build kernel on c->stream, inside the bracket opened here; after_rewrite
// runs once the registry holds the edited records, before the arena may be squeezed.  `edits`: the E edit structs, on the host.
extern "C++" template <class Edit, class LaunchBuild>  // (a template inside the file's extern "C" block)
int registry_apply_edits(mmp_ctx *c, int32_t E, int32_t n_kept, const Edit *edits, LaunchBuild &&launch_build,
                         const std::function<int()> &after_rewrite = {})
{
    const double eval_ms = c->last_kernel_ms;
    const int32_t M = c->n_models, base = c->n_entries;
    if (const int rc = registry_grow(c, M, base, n_kept)) return rc;
    HIP_TRY(c, c->u_idx.ensure((size_t)E * 4));
    HIP_TRY(c, c->u_rows.ensure((size_t)E * sizeof(mmp_model_row)));
    KT_BEGIN(c, c->stream);
    launch_build(base, base + n_kept);
    HIP_TRY(c, hipGetLastError());
    if (const int rc = registry_rewrite(c, E, M, base + n_kept, true)) return rc;
    kt_add(c, eval_ms);  // the call's device span: evaluation + apply
    // the host shadow, from the counts the edits leave.  (The prune's edits carry n_removed as well: m_cnt[model] == n_loaded +
    // n_failed holds before the call, so this is m_cnt[model] -= n_removed, and ent_live falls by the removed entries.)
    for (int32_t e = 0; e < E; e++) {
        const int32_t cnt = edits[e].n_loaded_after + edits[e].n_failed_after;
        c->ent_live += (int64_t)cnt - c->m_cnt[edits[e].model];
        c->m_cnt[edits[e].model] = cnt;
    }
    if (after_rewrite)
        if (const int rc = after_rewrite()) return rc;
    return squeeze_if_garbage(c);
}
// What the registry plans refuse before they touch the device, in the three places where each call checks it: the flag word among
// the arguments (before batch_mu is taken), the context's state, and, behind the call's own row checks, the arena's room: an apply
// appends at most the live entries and `extra` more (one per row of the call that can put an entry).
constexpr uint32_t kPlanFlags = MMP_PRUNE_APPLY | MMP_PRUNE_DRY;
static_assert(MMP_JANITOR_APPLY == MMP_PRUNE_APPLY && MMP_ROPS_APPLY == MMP_PRUNE_APPLY && MMP_JANITOR_DRY == MMP_PRUNE_DRY && MMP_ROPS_DRY == MMP_PRUNE_DRY, "");
inline bool plan_flags_bad(uint32_t flags) { return (flags & ~kPlanFlags) || flags == kPlanFlags; }
int plan_state_guard(mmp_ctx *c, const char *fn)
{
    if (!c->committed) return fail(c, MMP_ESTATE, "no committed snapshot");
    if (c->n_shards > 0) return fail(c, MMP_ESTATE, "%s: not available on a pod-axis shard context", fn);
    return MMP_OK;
}
int plan_arena_guard(mmp_ctx *c, const char *fn, bool apply, int32_t extra)
{
    if (apply && (int64_t)c->n_entries + c->ent_live + extra > INT32_MAX) return fail(c, MMP_EINVAL, "%s: entry arena overflow; reload the registry", fn);
    return MMP_OK;
}
}  // namespace

int mmp_models_upsert(mmp_ctx *c, const int32_t *idx, const mmp_model_row *rows, int32_t n, const int32_t *ent_pod,
                      const int64_t *ent_time, int32_t n_entries)
try {
    if (!c || n < 0 || n_entries < 0 || (n > 0 && (!idx || !rows)) || (n_entries > 0 && (!ent_pod || !ent_time)))
        return fail(c, MMP_EINVAL, "mmp_models_upsert: bad argument");
    if (n == 0) return MMP_OK;
    // batch_mu keeps the registry's host bookkeeping and device tables to this call (every other writer of them
    // takes it); decisions are held off (c->mu + idle decision streams) only while the rows are rewritten in place —
    // the entries of the changed records are appended to the arena beyond anything a published row refers to, and
    // the new rows wait in scratch, before that.
    std::lock_guard<std::mutex> gb(c->batch_mu);
    int32_t count = c->n_models;
    for (int32_t i = 0; i < n; i++) {
        const mmp_model_row &m = rows[i];
        if (idx[i] < 0 || idx[i] > count) return fail(c, MMP_EINVAL, "mmp_models_upsert: row %d names model %d of %d", i, idx[i], count);
        if (idx[i] == count) count++;
        if (m.n_loaded < 0 || m.n_failed < 0 || m.ent_off < 0 || (int64_t)m.ent_off + m.n_loaded + m.n_failed > (int64_t)n_entries)
            return fail(c, MMP_EINVAL, "mmp_models_upsert: row %d entry range out of bounds", i);
    }
    if ((int64_t)c->n_entries + n_entries > INT32_MAX) return fail(c, MMP_EINVAL, "mmp_models_upsert: entry arena overflow; reload the registry");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    // the last row wins when a model appears twice in one call (events are applied in order)
    std::vector<int32_t> last(n);
    {
        const uint64_t gen = (uint64_t)(++c->u_gen) << 32;
        if (c->u_stamp.size() < (size_t)count) c->u_stamp.resize(count, 0);
        for (int32_t i = 0; i < n; i++) c->u_stamp[idx[i]] = gen | (uint32_t)i;
        int32_t k = 0;
        for (int32_t i = 0; i < n; i++)
            if (c->u_stamp[idx[i]] == (gen | (uint32_t)i)) last[k++] = i;
        last.resize(k);
    }
    const int32_t k = (int32_t)last.size();
    const int32_t base = c->n_entries;
    std::vector<int32_t> h_idx(k);
    std::vector<mmp_model_row> h_rows(k);
    c->m_cnt.resize(count, 0);
    for (int32_t j = 0; j < k; j++) {
        const int32_t i = last[j];
        h_idx[j] = idx[i];
        h_rows[j] = rows[i];
        h_rows[j].ent_off += base;
        c->ent_live += (int64_t)(rows[i].n_loaded + rows[i].n_failed) - c->m_cnt[idx[i]];
        c->m_cnt[idx[i]] = rows[i].n_loaded + rows[i].n_failed;
    }
    if (const int rc = registry_grow(c, count, base, n_entries)) return rc;
    HIP_TRY(c, c->u_idx.ensure((size_t)k * 4));
    HIP_TRY(c, c->u_rows.ensure((size_t)k * sizeof(mmp_model_row)));
    if (n_entries) {
        HIP_TRY(c, hipMemcpyAsync(c->ent_pod.as<int32_t>() + base, ent_pod, (size_t)n_entries * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipMemcpyAsync(c->ent_time.as<int64_t>() + base, ent_time, (size_t)n_entries * 8, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(c, hipMemcpyAsync(c->u_idx.p, h_idx.data(), (size_t)k * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->u_rows.p, h_rows.data(), (size_t)k * sizeof(mmp_model_row), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipStreamSynchronize(st));  // the pageable sources above are this call's stack / the caller's arrays
    if (const int rc = registry_rewrite(c, k, count, base + n_entries)) return rc;
    return squeeze_if_garbage(c);
} MMP_CATCH(c, "mmp_models_upsert")

/* ---- commit: rank + permute + bitmaps + stats, all on the device --------- */

namespace {
// Rank the table from scratch by sampling (rank_sample.hpp): ranks of the rows [p_lo, p_hi) into `rank` (the others untouched).
// Only for a table on which the comparator is a strict total order (the caller's O(P) check).
int rank_by_sampling(mmp_ctx *c, const mmp_pod_row *d_pods, int32_t P, int64_t min_space, int64_t churn2, int32_t p_lo, int32_t p_hi,
                     int32_t *d_rank, hipStream_t st)
{
    const int32_t S = P >= 32768 ? 512 : 256;
    HIP_TRY(c, c->rs_split.ensure((size_t)2 * S * sizeof(RankRow)));
    HIP_TRY(c, c->rs_int.ensure(((size_t)2 * P + (2 * kCtrStride + 1) * (size_t)(S + 2)) * 4));
    RankRow *split = c->rs_split.as<RankRow>();
    int32_t *range_of = c->rs_int.as<int32_t>(), *idx = range_of + P, *hist = idx + P, *cur = hist + (S + 2) * kCtrStride,
            *off = cur + (S + 2) * kCtrStride;
    RankRow *srows = split + S;
    hipLaunchKernelGGL(sample_gather_kernel, dim3(div_up(S + 1, 256)), dim3(256), 0, st, d_pods, P, S, min_space, srows, hist, cur);
    hipLaunchKernelGGL(sample_sort_kernel, dim3(S), dim3(256), 0, st, srows, S, churn2, split);
    hipLaunchKernelGGL(sample_range_kernel, dim3(div_up(P, 256)), dim3(256), 0, st, d_pods, P, S, min_space, churn2, split, range_of, hist);
    hipLaunchKernelGGL(sample_scatter_kernel, dim3(div_up(P, 256)), dim3(256), 0, st, P, S, range_of, hist, cur, off, idx);
    hipLaunchKernelGGL(sample_rank_kernel, dim3(div_up(P, 16)), dim3(1024), 0, st, d_pods, P, min_space, churn2, range_of, off, idx, p_lo, p_hi,
                       d_rank);
    HIP_TRY(c, hipGetLastError());
    return MMP_OK;
}

struct ZeroBatch {  // collects buffers, clears them with one zero_regions_kernel launch
    ZeroList Z{};
    size_t most = 0;
    hipStream_t stream = nullptr;
    explicit ZeroBatch(hipStream_t st) : stream(st) {}
    void add(void *p, size_t bytes)
    {
        if (!p || bytes == 0) return;
        if (Z.n == kZeroRegions) launch(stream);  // (a full table goes out; the rest follows in another launch)
        Z.p[Z.n] = p;
        Z.bytes[Z.n] = (bytes + 3) & ~(size_t)3;  // (DevBuf allocations are rounded up: the tail bytes exist)
        most = std::max(most, bytes);
        Z.n++;
    }
    void launch(hipStream_t st)
    {
        if (Z.n == 0) return;
        const int blocks = (int)std::min<size_t>(std::max<size_t>(most / (256 * 4 * 4), 1), 256);
        hipLaunchKernelGGL(zero_regions_kernel, dim3(blocks), dim3(256), 0, st, Z);
        Z.n = 0;
        most = 0;
    }
};

/* The stages of a commit.  mmp_snapshot_commit and the pod-axis pair mmp_shard_rank_dev / mmp_shard_commit_dev are lists of these;
   every stage enqueues on the stream it is given and none synchronises it, except where its comment says so. */

inline int64_t churn2_of(const mmp_ctx *c) { return (int64_t)((uint64_t)c->cfg.min_churn_age_ms * 2u); }

// The sizes of an unsharded commit, and which optional tables it builds.
struct CommitDims {
    int32_t P, W, T;  // rows, 64-position words (>= 1), bitmap rows (>= 1)
    int32_t n_rs;     // replaced replica sets
    size_t padded;    // W * 64
    int64_t min_space, churn2;
    // the long path's inverse tables (Snap::sel / ::rk): 512 bytes per type row and 64-position word, each, rebuilt at every commit —
    // 320 KB on C3, but a table of 100 type rows x 100 000 instances would be 80 MB a piece: beyond kSelMaxBytes they are not built
    // and a shortlist that spans the table takes the wave path
    size_t sel_bytes;
    bool have_sel;
    bool have_lmemo;    // the recorded walks of the long shortlists (place_kernel.hpp: LongMemo)
    size_t wins_bytes;  // rounded up to the 1 KB chunks place_block stages (rows beyond T are never read as windows)
};
CommitDims commit_dims(const mmp_ctx *c)
{
    CommitDims D{};
    D.P = (int32_t)c->pods.size();
    D.W = std::max(div_up(D.P, 64), 1);
    D.T = std::max(c->n_types, 1);
    D.n_rs = (int32_t)c->replaced_rs.size();
    D.padded = (size_t)D.W * 64;
    D.min_space = c->cfg.min_space_units;
    D.churn2 = churn2_of(c);
    D.sel_bytes = (size_t)2 * D.T * D.W * 64 * 4;
    D.have_sel = D.sel_bytes <= kSelMaxBytes;
    D.have_lmemo = D.P > 0 && D.have_sel && !c->tune.no_long_memo;
    D.wins_bytes = (((size_t)std::max(D.T, kWinLds) * sizeof(TypeWin) + 1023) / 1024) * 1024;
    return D;
}

// The rank-ordered columns and bitmaps, Wc words a row (a pod-axis shard: its slice); pos_of spans the whole table's W words.
int ensure_columns(mmp_ctx *c, SnapBufs &B, int32_t T, int32_t Wc, int32_t W)
{
    const size_t padded = (size_t)Wc * 64;
    // A column that was (re)allocated starts as zeros.  A commit whose order is not total leaves one rank's slot of every column,
    // and the loser's pos_of word, without a writer (scatter_pods_kernel returns on the second row of a rank), and the table
    // kernels run on the columns before the host reads the flag and refuses with MMP_EORDER: what they find there must be an
    // index inside the table — zero, or what an earlier commit of this context wrote — never what the allocator left behind.
    bool fresh = false;
    auto column = [&](DevBuf &b, size_t bytes) {
        const size_t was = b.cap;
        hipError_t e = b.ensure(bytes);
        if (e == hipSuccess && b.cap != was) {
            fresh = true;
            e = hipMemsetAsync(b.p, 0, b.cap, c->stream);
        }
        return e;
    };
    HIP_TRY(c, column(B.lru, padded * 8));
    HIP_TRY(c, column(B.rem, padded * 8));
    HIP_TRY(c, column(B.cnt, padded * 4));
    HIP_TRY(c, column(B.rpm, padded * 4));
    HIP_TRY(c, column(B.orig, padded * 4));
    HIP_TRY(c, column(B.pos_of, (size_t)W * 64 * 4));
    if (fresh) HIP_TRY(c, hipStreamSynchronize(c->stream));  // (rare: the columns only grow; whichever stream the commit builds on)
    HIP_TRY(c, B.elig.ensure((size_t)T * Wc * 8));
    HIP_TRY(c, B.elig_nors.ensure((size_t)T * Wc * 8));
    HIP_TRY(c, B.pref.ensure((size_t)T * Wc * 8));
    HIP_TRY(c, B.has_pref.ensure(T));
    HIP_TRY(c, B.fullw.ensure((size_t)Wc * 8));
    HIP_TRY(c, B.ge.ensure((size_t)kGeRows * Wc * 8));
    return MMP_OK;
}
// What a commit reads or scribbles on besides the table: the scatter's scratch, the staged type table, the replica-set list.
int ensure_commit_scratch(mmp_ctx *c, SnapSide &N, int32_t T, int32_t W)
{
    HIP_TRY(c, c->occupancy.ensure((size_t)W * 64 * 4));
    HIP_TRY(c, c->flag.ensure(sizeof(int32_t)));
    HIP_TRY(c, N.stats_acc.ensure(sizeof(StatsAcc)));
    HIP_TRY(c, c->rs_bad.ensure((size_t)W * 64));
    HIP_TRY(c, c->rs_list.ensure(std::max<size_t>(c->replaced_rs.size(), 1) * 4));
    HIP_TRY(c, N.d_allowed.ensure(std::max<size_t>((size_t)T * W, 1) * 8));
    HIP_TRY(c, c->d_prefer.ensure(std::max<size_t>((size_t)T * W, 1) * 8));
    HIP_TRY(c, N.d_has_allowed.ensure(T));
    return MMP_OK;
}
// Everything an unsharded snapshot is made of.
int ensure_snapshot_buffers(mmp_ctx *c, SnapBufs &B, SnapSide &N, const CommitDims &D)
{
    const int32_t T = D.T, W = D.W;
    HIP_TRY(c, B.pods.ensure(std::max<size_t>(D.P, 1) * sizeof(mmp_pod_row)));
    if (const int rc = ensure_columns(c, B, T, W, W)) return rc;
    HIP_TRY(c, B.ctpos.ensure((size_t)(kGeRows + 1) * 4));
    HIP_TRY(c, B.pc.ensure((size_t)2 * T * (W + 1) * 4));
    HIP_TRY(c, B.nz.ensure((size_t)2 * T * (W + 1) * 4));
    HIP_TRY(c, B.ph.ensure((size_t)2 * T * (W + 1) * 8));
    if (D.have_sel) {
        HIP_TRY(c, B.sel.ensure(D.sel_bytes));
        HIP_TRY(c, B.rk.ensure(D.sel_bytes));
    }
    if (D.have_lmemo) HIP_TRY(c, B.lmemo.ensure((size_t)T * kLongLevels * sizeof(LongMemo)));
    HIP_TRY(c, B.memo.ensure((size_t)kWinLds * sizeof(TypeMemo)));
    HIP_TRY(c, B.memo_cand.ensure((size_t)kWinLds * kMemoCand * 4));
    HIP_TRY(c, B.memo_rk.ensure((size_t)kWinLds * kMemoCand * 2));
    HIP_TRY(c, B.heads.ensure(D.wins_bytes));
    HIP_TRY(c, B.bslots.ensure(kBSlots * sizeof(BSlot) + 16));
    HIP_TRY(c, B.bpm.ensure((size_t)kBSlots * W * 64 * 4));
    HIP_TRY(c, B.bwin.ensure(kBSlots * sizeof(BLaunch)));
    HIP_TRY(c, B.bsurv.ensure((size_t)kBSlots * kBClasses * W * 8));
    HIP_TRY(c, B.bpcs.ensure((size_t)kBSlots * kBClasses * (W + 1) * 4));
    HIP_TRY(c, c->rank.ensure(D.padded * 4));
    return ensure_commit_scratch(c, N, T, W);
}

// The unsharded commit's scratch cleared, and the tails of its columns beyond P.
void clear_commit_scratch(mmp_ctx *c, SnapBufs &B, const CommitDims &D, hipStream_t st)
{
    ZeroBatch zb(st);
    zb.add(c->rank.p, D.padded * 4);
    zb.add(c->occupancy.p, D.padded * 4);
    zb.add(c->flag.p, sizeof(int32_t));
    zb.add(B.bslots.p, kBSlots * sizeof(BSlot) + 16);
    zb.launch(st);
    hipLaunchKernelGGL(zero_tails_kernel, dim3(1), dim3(64), 0, st, B.lru.as<int64_t>(), B.rem.as<int64_t>(), B.cnt.as<int32_t>(),
                       B.rpm.as<int32_t>(), B.orig.as<int32_t>(), B.pos_of.as<int32_t>(), D.P, (int32_t)D.padded);
}

// Is the literal comparator a strict total order on these rows?  (see snapshot.hpp "ranking by sorting")
struct OrderCheck {
    bool sort_legal;
    int32_t n_present, n_nonfull;
};
OrderCheck check_placement_order(const std::vector<mmp_pod_row> &pods, int64_t min_space, int64_t churn2)
{
    bool versions_differ = false, full_low_lru = false, wide_count = false;
    OrderCheck oc{};
    for (const mmp_pod_row &r : pods) {
        if (r.version != pods[0].version) versions_differ = true;
        if (r.count > (1 << 30) || r.count < -(1 << 30)) wide_count = true;  // :4676 is an int subtraction
        const uint64_t d = (uint64_t)r.capacity - (uint64_t)r.used;
        const int64_t rem = (int64_t)d > 0 ? (int64_t)d : 0;
        if (rem < min_space && r.lru_time <= churn2) full_low_lru = true;
        if (!(r.flags & (MMP_POD_SHUTTING_DOWN | MMP_POD_TOMBSTONE))) {
            oc.n_present++;
            if (!(rem < min_space)) oc.n_nonfull++;
        }
    }
    oc.sort_legal = !(versions_differ && full_low_lru) && !wide_count;
    return oc;
}

// A few rows changed since the published snapshot, and both orders are total: re-rank by insertion (snapshot.hpp "a commit
// whose table differs ... in a few rows"); the unpublished set is then rebuilt from the PUBLISHED one.  Sets `delta` when this
// commit can go that way, and then fills `dl` and the host mirror of the new order.  The only stage that may wait for the
// device: the first delta after a commit from scratch fetches the published order.
int plan_delta(mmp_ctx *c, const CommitDims &D, bool sort_legal, DeltaRows &dl, std::vector<int32_t> &new_order, bool &delta)
{
    const int32_t P = D.P;
    delta = false;
    if (!(c->committed && !c->dirty_all && !c->tune.no_delta && sort_legal && c->order_total && P >= 2 && P == c->snap.P)) return MMP_OK;
    std::vector<int32_t> chg(c->dirty);
    std::sort(chg.begin(), chg.end());
    chg.erase(std::unique(chg.begin(), chg.end()), chg.end());
    if ((int32_t)chg.size() > kDeltaRows) return MMP_OK;
    if (!c->h_order_valid) {  // the host's mirror of the published order, fetched when a delta first needs it
        c->h_order.resize(P);
        c->h_pos.resize(P);
        HIP_TRY(c, copy_sync(c, c->h_order.data(), c->sb[c->cur].orig.p, (size_t)P * 4, hipMemcpyDeviceToHost));
        for (int32_t q = 0; q < P; q++) c->h_pos[c->h_order[q]] = q;
        c->h_order_valid = true;
    }
    const int32_t K = (int32_t)chg.size();
    dl.K = K;
    std::vector<int32_t> rem_sorted(K);
    for (int32_t k = 0; k < K; k++) rem_sorted[k] = c->h_pos[chg[k]];
    std::sort(rem_sorted.begin(), rem_sorted.end());
    auto unchanged_at = [&](int32_t j) {  // the j-th row of the old order with the changed rows taken out
        int32_t pos = j;
        for (int32_t k = 0; k < K; k++)
            if (rem_sorted[k] <= pos) pos++;
        return c->h_order[pos];
    };
    RankRow rr[kDeltaRows];
    for (int32_t k = 0; k < K; k++) rr[k] = make_rank_row(c->pods[chg[k]], D.min_space);
    // The order this path publishes must be STRICT, as the one from scratch is (scatter_pods_kernel reports two rows
    // of one rank as MMP_EORDER): a changed row that now ties with its neighbour or with another changed row — a
    // duplicate or unset id_order, every other field equal — sends the commit down the full path, which reports it.
    bool strict = true;
    for (int32_t k = 0; k < K; k++) {
        int32_t lo = 0, hi = P - K;
        while (lo < hi) {
            const int32_t mid = (lo + hi) >> 1;
            if (placement_less(make_rank_row(c->pods[unchanged_at(mid)], D.min_space), rr[k], D.churn2))
                lo = mid + 1;
            else
                hi = mid;
        }
        // (every unchanged row before lo is less than the row by the search; the one at lo must be greater, not equal)
        if (lo < P - K && !placement_less(rr[k], make_rank_row(c->pods[unchanged_at(lo)], D.min_space), D.churn2)) strict = false;
        int32_t before = 0;
        for (int32_t k2 = 0; k2 < K; k2++) {
            if (k2 == k) continue;
            const bool lt = placement_less(rr[k2], rr[k], D.churn2);
            if (lt) before++;
            else if (!placement_less(rr[k], rr[k2], D.churn2)) strict = false;  // neither before the other: a tie
        }
        dl.pod[k] = chg[k];
        dl.removed[k] = rem_sorted[k];
        dl.ins[k] = lo;
        dl.newrank[k] = lo + before;
        dl.rows[k] = c->pods[chg[k]];
    }
    // the host mirror of the NEW order (published with the snapshot)
    if (strict) {
        new_order.assign(P, -1);
        std::vector<uint8_t> is_chg(P, 0);
        for (int32_t k = 0; k < K; k++) {
            new_order[dl.newrank[k]] = chg[k];
            is_chg[chg[k]] = 1;
        }
        int32_t w = 0;
        for (int32_t q = 0; q < P; q++) {
            const int32_t pod = c->h_order[q];
            if (is_chg[pod]) continue;
            while (new_order[w] >= 0) w++;
            new_order[w++] = pod;
        }
    }
    delta = strict;
    return MMP_OK;
}

// The host sources of upload_commit_inputs' copies: pageable, so they stay with the caller until it has synchronised the stream.
struct InputStage {
    std::vector<uint8_t> hp, ha;
    StatsAcc init{};
};
// The inputs besides the instance table: the type table's flags and allowed / prefer rows, the replica-set list and the
// cluster stats' initial value.  A type table goes up only when it was reloaded since the buffer set / the side / the staging
// copy last took it (their types_gen), or always when `force`; the caller marks the generations once the copies have landed.
int upload_commit_inputs(mmp_ctx *c, SnapBufs &B, SnapSide &N, int32_t T, bool force, InputStage &in, hipStream_t st)
{
    in.hp.assign(T, 0);
    in.ha.assign(T, 0);
    for (int32_t t = 0; t < c->n_types; t++) {
        in.hp[t] = c->has_prefer[t];
        in.ha[t] = c->has_allowed[t];
    }
    const bool side_stale = force || N.types_gen != c->types_gen;
    if (force || B.types_gen != c->types_gen) HIP_TRY(c, hipMemcpyAsync(B.has_pref.p, in.hp.data(), T, hipMemcpyHostToDevice, st));
    if (side_stale) HIP_TRY(c, hipMemcpyAsync(N.d_has_allowed.p, in.ha.data(), T, hipMemcpyHostToDevice, st));
    if (c->n_types > 0 && !c->allowed.empty()) {
        if (side_stale) HIP_TRY(c, hipMemcpyAsync(N.d_allowed.p, c->allowed.data(), c->allowed.size() * 8, hipMemcpyHostToDevice, st));
        if (force || c->d_prefer_gen != c->types_gen)
            HIP_TRY(c, hipMemcpyAsync(c->d_prefer.p, c->prefer.data(), c->prefer.size() * 8, hipMemcpyHostToDevice, st));
    }
    const size_t n_rs = c->replaced_rs.size();
    if (n_rs) HIP_TRY(c, hipMemcpyAsync(c->rs_list.p, c->replaced_rs.data(), n_rs * 4, hipMemcpyHostToDevice, st));
    in.init = StatsAcc{};
    in.init.global_lru = INT64_MAX;
    HIP_TRY(c, hipMemcpyAsync(N.stats_acc.p, &in.init, sizeof in.init, hipMemcpyHostToDevice, st));
    return MMP_OK;
}

// The audit hash's word multipliers (Snap::amul): a function of the word index alone, so uploaded, and waited for, once per table size.
int ensure_audit_multipliers(mmp_ctx *c, SnapBufs &B, int32_t W, hipStream_t st)
{
    if (B.amul_w == W) return MMP_OK;
    HIP_TRY(c, B.amul.ensure((size_t)W * 8));
    std::vector<uint64_t> am((size_t)W);
    for (int32_t w = 0; w < W; w++) am[(size_t)w] = audit_mul((uint64_t)w);
    HIP_TRY(c, hipMemcpyAsync(B.amul.p, am.data(), (size_t)W * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipStreamSynchronize(st));  // (`am` leaves scope)
    B.amul_w = W;
    return MMP_OK;
}

// The unsharded snapshot over B (B.amul is in place: ensure_audit_multipliers).
Snap snap_of(const SnapBufs &B, const CommitDims &D)
{
    Snap S = snap_columns<Snap>(B, D.P, D.W, D.T, D.n_rs > 0, D.min_space);
    S.ge = B.ge.as<uint64_t>();
    S.pc = B.pc.as<int32_t>();
    S.nz = B.nz.as<int32_t>();
    S.ph = B.ph.as<uint64_t>();
    S.ctpos = D.P > 0 ? B.ctpos.as<int32_t>() : nullptr;
    S.amul = B.amul.as<uint64_t>();
    S.sel = D.P > 0 && D.have_sel ? B.sel.as<int32_t>() : nullptr;
    S.rk = D.P > 0 && D.have_sel ? B.rk.as<int32_t>() : nullptr;
    S.memo = B.memo.as<TypeMemo>();
    S.memo_cand = B.memo_cand.as<int32_t>();
    S.memo_rk = B.memo_rk.as<int16_t>();
    S.lmemo = D.have_lmemo ? B.lmemo.as<LongMemo>() : nullptr;
    return S;
}

// Ranks of the rows [p_lo, p_hi) of the P-row table at d_pods into d_rank, from scratch: by sampling, by a merge sort of the
// whole table, or all pairs.  all-pairs is embarrassingly parallel and wins below ~8k pods (measured: 10k pods 172 us all-pairs
// vs 120 us sort; 50k pods 4.3 ms vs 0.25 ms); a merge sort of a few thousand 64-byte keys is latency bound.  `want_sort` is
// the caller's threshold (the whole table against a shard's slice of the pairs); sorting also needs the comparator to be a
// total order (`sort_legal`).  `slice`: the caller is a pod-axis shard, whose d_rank holds only its range's ranks.
int launch_rank(mmp_ctx *c, const mmp_pod_row *d_pods, int32_t P, int32_t p_lo, int32_t p_hi, bool slice, bool want_sort, bool sort_legal,
                int32_t *d_rank, hipStream_t st)
{
    const int64_t min_space = c->cfg.min_space_units, churn2 = churn2_of(c);
    if (want_sort && sort_legal && P >= kSampleMinPods && c->tune.rank_mode != 3)
        return rank_by_sampling(c, d_pods, P, min_space, churn2, p_lo, p_hi, d_rank, st);
    if (want_sort && sort_legal && P >= 2) {
        HIP_TRY(c, c->rk_rows.ensure((size_t)P * sizeof(RankRow)));
        HIP_TRY(c, c->rk_idx.ensure((size_t)P * sizeof(RankRow)));
        const PlacementRowLess less{churn2};
        size_t tmp_bytes = 0;
        HIP_TRY(c, rocprim::merge_sort(nullptr, tmp_bytes, c->rk_rows.as<RankRow>(), c->rk_idx.as<RankRow>(), (size_t)P, less, st));
        HIP_TRY(c, c->rk_tmp.ensure(std::max<size_t>(tmp_bytes, 16)));
        hipLaunchKernelGGL(rank_rows_kernel, dim3(div_up(P, 256)), dim3(256), 0, st, d_pods, P, min_space, c->rk_rows.as<RankRow>());
        HIP_TRY(c, rocprim::merge_sort(c->rk_tmp.p, tmp_bytes, c->rk_rows.as<RankRow>(), c->rk_idx.as<RankRow>(), (size_t)P, less, st));
        if (slice)
            hipLaunchKernelGGL(rank_from_order_range_kernel, dim3(div_up(P, 256)), dim3(256), 0, st, c->rk_idx.as<RankRow>(), P, p_lo, p_hi, d_rank);
        else
            hipLaunchKernelGGL(rank_from_order_kernel, dim3(div_up(P, 256)), dim3(256), 0, st, c->rk_idx.as<RankRow>(), P, d_rank);
        return MMP_OK;
    }
    const int pb = div_up(p_hi - p_lo, kRankBlock);
    const int slices = std::max(1, std::min(64, 2048 / pb));
    hipLaunchKernelGGL(rank_pods_kernel, dim3(pb, slices), dim3(kRankBlock), 0, st, d_pods, P, min_space, churn2, slices, p_lo, p_hi, d_rank);
    return MMP_OK;
}

void launch_mark_replaced(mmp_ctx *c, const SnapBufs &B, int32_t P, hipStream_t st)
{
    const int32_t n_rs = (int32_t)c->replaced_rs.size();
    if (n_rs)
        hipLaunchKernelGGL(mark_replaced_kernel, dim3(div_up(P, 256)), dim3(256), 0, st, B.pods.as<mmp_pod_row>(), P, c->rs_list.as<int32_t>(),
                           n_rs, c->rs_bad.as<uint8_t>());
}

// level 1: everything that needs only the table and the rank-ordered columns, in ONE launch (place_kernel.hpp CommitL1)
CommitL1 make_commit_l1(const mmp_ctx *c, const SnapBufs &B, const SnapSide &N, const CommitDims &D)
{
    const int32_t P = D.P, W = D.W, T = D.T;
    CommitL1 L1{};
    L1.pods = B.pods.as<mmp_pod_row>();
    L1.P = P;
    L1.W = W;
    L1.T = T;
    L1.min_space = D.min_space;
    L1.orig = B.orig.as<int32_t>();
    L1.cnt = B.cnt.as<int32_t>();
    L1.allowed = N.d_allowed.as<uint64_t>();
    L1.prefer = c->d_prefer.as<uint64_t>();
    L1.has_allowed = N.d_has_allowed.as<uint8_t>();
    L1.has_prefer = B.has_pref.as<uint8_t>();
    L1.rs_bad = D.n_rs ? c->rs_bad.as<uint8_t>() : nullptr;
    L1.elig = B.elig.as<uint64_t>();
    L1.elig_nors = B.elig_nors.as<uint64_t>();
    L1.pref = B.pref.as<uint64_t>();
    L1.fullw = B.fullw.as<uint64_t>();
    L1.ge = B.ge.as<uint64_t>();
    L1.ctpos = B.ctpos.as<int32_t>();
    L1.acc = N.stats_acc.as<StatsAcc>();
    L1.pod_pts = N.d_pts.as<int32_t>();
    L1.NP = N.n_pts;
    L1.pstats = N.pstats.as<StatsAcc>();
    L1.nb_masks = div_up(T * W, 4);
    L1.nb_ge = div_up(kGeRows * W, 4);
    L1.nb_stats = std::min(div_up(P, 256), 512);
    L1.nb_pstats = N.n_pts > 0 ? std::min(div_up(P, 256), 64) : 0;
    return L1;
}
inline int32_t *n_bslots_dev(const SnapBufs &B) { return reinterpret_cast<int32_t *>(static_cast<char *>(B.bslots.p) + kBSlots * sizeof(BSlot)); }
// level 2: what needs the bitmaps / the stats: prefix tables, head windows (place_kernel.hpp: TypeWin), case (b) slots
// (where case (b) starts per preferring type), partition / type subset stats
CommitL2 make_commit_l2(const mmp_ctx *c, const SnapBufs &B, const SnapSide &N, const Snap &S)
{
    CommitL2 L2{};
    L2.S = S;
    L2.pods = B.pods.as<mmp_pod_row>();
    L2.wins = B.heads.as<TypeWin>();
    L2.slots = B.bslots.as<BSlot>();
    L2.n_slots = n_bslots_dev(B);
    L2.acc = N.stats_acc.as<StatsAcc>();
    L2.pstats = N.pstats.as<StatsAcc>();
    L2.NP = N.n_pts;
    L2.Tw = N.pts_tw;
    L2.prohib = N.d_prohib.as<uint64_t>();
    L2.has_allowed = c->n_types > 0 ? N.d_has_allowed.as<uint8_t>() : nullptr;
    L2.tstats = N.tstats.as<StatsAcc>();
    L2.nb_finish = div_up(std::max(N.n_pts, S.T), 64);
    return L2;
}
// The tables of a non-empty unsharded snapshot, from its rank-ordered columns: level 1, level 2, the inverse tables and
// shortlists, the case (b) tables.
void launch_snapshot_tables(mmp_ctx *c, SnapBufs &B, SnapSide &N, const Snap &S, const CommitDims &D, hipStream_t st)
{
    const int32_t T = D.T, W = D.W;
    const CommitL1 L1 = make_commit_l1(c, B, N, D);
    hipLaunchKernelGGL(commit_level1_kernel, dim3(L1.nb_stats + L1.nb_pstats + 1 + L1.nb_masks + L1.nb_ge), dim3(256), 0, st, L1);
    const CommitL2 L2 = make_commit_l2(c, B, N, S);
    hipLaunchKernelGGL(commit_level2_kernel, dim3(4 * T + L2.nb_finish), dim3(64), 0, st, L2);
    // sel / rk from the prefix tables, and the per-type shortlists (TypeMemo) from the finished head windows (every row a decision
    // can name is written, valid or not): one launch; the registry view is resolved against the shortlists' ranges afterwards
    hipLaunchKernelGGL(build_sel_memo_kernel, dim3((D.have_sel ? 2 * T * W : 0) + std::min(T, kWinLds) + (S.lmemo ? T : 0)), dim3(64), 0, st, S,
                       D.have_sel ? B.sel.as<int32_t>() : nullptr, D.have_sel ? B.rk.as<int32_t>() : nullptr, B.heads.as<TypeWin>(),
                       B.memo.as<TypeMemo>(), B.memo_cand.as<int32_t>(), B.memo_rk.as<int16_t>(), B.lmemo.as<LongMemo>());
    // the running minimum of the case (b) candidates' rpm, then the survivor bitmaps of the rpm rule's four limits
    hipLaunchKernelGGL(prefix_min_rpm_kernel, dim3(kBSlots), dim3(64), 0, st, S, B.bslots.as<BSlot>(), n_bslots_dev(B), B.bpm.as<int32_t>(),
                       (int32_t)(W * 64));
    hipLaunchKernelGGL(build_bsurv_kernel, dim3(kBSlots), dim3(256), 0, st, S, B.bslots.as<BSlot>(), n_bslots_dev(B), B.bpm.as<int32_t>(),
                       (int32_t)(W * 64), B.bwin.as<BLaunch>(), B.bsurv.as<uint64_t>(), B.bpcs.as<int32_t>());
}
// The same tables of an empty one.
int clear_snapshot_tables(mmp_ctx *c, SnapBufs &B, const CommitDims &D, hipStream_t st)
{
    const size_t T = D.T, W = D.W;
    HIP_TRY(c, hipMemsetAsync(B.heads.p, 0, D.wins_bytes, st));
    HIP_TRY(c, hipMemsetAsync(B.memo.p, 0, (size_t)kWinLds * sizeof(TypeMemo), st));
    HIP_TRY(c, hipMemsetAsync(B.pc.p, 0, 2 * T * (W + 1) * 4, st));
    HIP_TRY(c, hipMemsetAsync(B.nz.p, 0, 2 * T * (W + 1) * 4, st));
    HIP_TRY(c, hipMemsetAsync(B.ph.p, 0, 2 * T * (W + 1) * 8, st));
    HIP_TRY(c, hipMemsetAsync(B.elig.p, 0, T * W * 8, st));
    HIP_TRY(c, hipMemsetAsync(B.elig_nors.p, 0, T * W * 8, st));
    HIP_TRY(c, hipMemsetAsync(B.pref.p, 0, T * W * 8, st));
    HIP_TRY(c, hipMemsetAsync(B.fullw.p, 0, W * 8, st));
    HIP_TRY(c, hipMemsetAsync(B.ge.p, 0, kGeRows * W * 8, st));
    return MMP_OK;
}

/* Partition the present instances by their ProhibitedTypeSet and build the per-partition / per-type ClusterStats of the
   snapshot being committed (snapshot.hpp "instance partitions"), in three stages.  N = the side state of the snapshot being built. */

// The host's interning of the partitions and their uploads: inputs, like the table itself.
int stage_partitions(mmp_ctx *c, SnapSide &N, int32_t P, hipStream_t st)
{
    const int32_t T = std::max(c->n_types, 1), Tw = div_up(T, 64);
    N.pts_of.assign(P, -1);
    N.pts_prohib.clear();
    N.n_pts = 0;
    N.pts_tw = Tw;
    if (c->n_types > 0) {
        // every instance's ProhibitedTypeSet as an id of the distinct sets: a function of the type table alone, kept until
        // that table is reloaded (interning P signatures of T bits through a map was most of a small commit's host time)
        if (!c->sig_valid || (int32_t)c->sig_of.size() != P) {
            std::map<std::vector<uint64_t>, int32_t> intern;
            std::vector<uint64_t> sig(Tw);
            const int32_t Wf = c->types_w;
            c->sig_of.assign(P, 0);
            c->sig_rows.clear();
            for (int32_t p = 0; p < P; p++) {
                std::fill(sig.begin(), sig.end(), 0);
                for (int32_t t = 0; t < c->n_types; t++)
                    if (c->has_allowed[t] && !((c->allowed[(size_t)t * Wf + (p >> 6)] >> (p & 63)) & 1ull))
                        sig[t >> 6] |= 1ull << (t & 63);
                auto it = intern.find(sig);
                if (it == intern.end()) {
                    it = intern.emplace(sig, (int32_t)intern.size()).first;
                    c->sig_rows.insert(c->sig_rows.end(), sig.begin(), sig.end());
                }
                c->sig_of[p] = it->second;
            }
            c->sig_valid = true;
        }
        // partitions are numbered by first appearance among the instances PRESENT in this table
        std::vector<int32_t> number(c->sig_rows.size() / std::max(Tw, 1), -1);
        for (int32_t p = 0; p < P; p++) {
            if (c->pods[p].flags & (MMP_POD_SHUTTING_DOWN | MMP_POD_TOMBSTONE)) continue;
            const int32_t sid = c->sig_of[p];
            if (number[sid] < 0) {
                number[sid] = N.n_pts++;
                N.pts_prohib.insert(N.pts_prohib.end(), c->sig_rows.begin() + (size_t)sid * Tw, c->sig_rows.begin() + (size_t)(sid + 1) * Tw);
            }
            N.pts_of[p] = number[sid];
        }
    }
    const int32_t NP = N.n_pts;
    N.pstats_h.assign(NP + 1, StatsAcc{});
    N.pstats_h[NP].global_lru = INT64_MAX;  // InstanceSetStatsTracker.EMPTY_STATS
    N.tstats_h.assign(T, StatsAcc{});
    HIP_TRY(c, N.d_pts.ensure(std::max<size_t>(P, 1) * 4));
    HIP_TRY(c, N.d_prohib.ensure(std::max<size_t>((size_t)NP * Tw, 1) * 8));
    HIP_TRY(c, N.pstats.ensure((size_t)(NP + 1) * sizeof(StatsAcc)));
    HIP_TRY(c, N.tstats.ensure((size_t)T * sizeof(StatsAcc)));
    if (P) HIP_TRY(c, hipMemcpyAsync(N.d_pts.p, N.pts_of.data(), (size_t)P * 4, hipMemcpyHostToDevice, st));
    if (NP) HIP_TRY(c, hipMemcpyAsync(N.d_prohib.p, N.pts_prohib.data(), (size_t)NP * Tw * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(N.pstats.p, N.pstats_h.data(), (size_t)(NP + 1) * sizeof(StatsAcc), hipMemcpyHostToDevice, st));
    return MMP_OK;
}
// The kernels, for a commit whose level launches do not hold them (an empty table, a pod-axis shard).  After the cluster
// stats: N.stats_acc and N.d_has_allowed are filled.
int launch_subset_stats(mmp_ctx *c, SnapSide &N, const mmp_pod_row *d_pods, int32_t P, int64_t min_space, hipStream_t st)
{
    const int32_t T = std::max(c->n_types, 1), NP = N.n_pts;
    if (NP > 0 && P > 0)
        hipLaunchKernelGGL(partition_stats_kernel, dim3(std::min(div_up(P, 256), 64)), dim3(256), 0, st, d_pods, P, min_space,
                           N.d_pts.as<int32_t>(), NP, N.pstats.as<StatsAcc>());
    hipLaunchKernelGGL(subset_stats_finish_kernel, dim3(div_up(std::max(NP, T), 256)), dim3(256), 0, st, N.stats_acc.as<StatsAcc>(),
                       N.pstats.as<StatsAcc>(), NP, N.d_prohib.as<uint64_t>(), N.pts_tw, T,
                       c->n_types > 0 ? N.d_has_allowed.as<uint8_t>() : nullptr, N.tstats.as<StatsAcc>());
    HIP_TRY(c, hipGetLastError());
    return MMP_OK;
}
// The results into the host mirrors, valid once the caller has synchronised st.
int fetch_subset_stats(mmp_ctx *c, SnapSide &N, hipStream_t st)
{
    const int32_t T = std::max(c->n_types, 1), NP = N.n_pts;
    HIP_TRY(c, hipMemcpyAsync(N.pstats_h.data(), N.pstats.p, (size_t)(NP + 1) * sizeof(StatsAcc), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(N.tstats_h.data(), N.tstats.p, (size_t)T * sizeof(StatsAcc), hipMemcpyDeviceToHost, st));
    return MMP_OK;
}

// The scatter's "two rows of one rank" flag and the cluster stats, into the caller's words: valid once it has synchronised st.
int fetch_commit_result(mmp_ctx *c, SnapSide &N, int32_t *bad, StatsAcc *acc, hipStream_t st)
{
    HIP_TRY(c, hipMemcpyAsync(bad, c->flag.p, sizeof *bad, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(acc, N.stats_acc.p, sizeof *acc, hipMemcpyDeviceToHost, st));
    return MMP_OK;
}
void publish_cluster_stats(mmp_ctx *c, const StatsAcc &acc)
{
    c->stats.total_capacity = (int64_t)acc.total_capacity;
    c->stats.total_free = (int64_t)acc.total_free;
    c->stats.global_lru = (int64_t)acc.global_lru;
    c->stats.instance_count = acc.instance_count;
    c->stats.model_copy_count = acc.model_copy_count;
}

// The commit itself (mmp_snapshot_commit below; the caller holds batch_mu).  state_locked: the caller holds the state lock as well
// and keeps it — mmp_pods_retire, whose swapped inputs and the snapshot built from them must become visible together.
int commit_staged(mmp_ctx *c, bool state_locked)
{
    // Wait-free for decisions (SURVEY.md §8b "Threading"): the whole build runs with batch_mu only.  batch_mu keeps
    // the inputs still — every loader of the instance table, the type table, the registry and the replica-set list
    // takes it, and so does any other commit — and it owns c->stream and the commit scratch.  Everything a decision
    // reads is double-buffered (SnapBufs + SnapSide): the build fills the set that is NOT published, decisions keep
    // capturing the published one under c->mu, and c->mu is taken only for the pointer swap at the end.
    if (c->n_shards > 0)
        return fail(c, MMP_ESTATE, "context is a pod-axis shard: commit with mmp_shard_rank_dev + mmp_shard_commit_dev");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    // The set about to be rewritten was published until the previous commit's swap; a kernel that still reads it
    // was enqueued before that swap.  Waiting for the decision streams (without c->mu: new decisions only ever
    // capture the published set) retires those.
    HIP_TRY(c, quiesce_decisions(c));

    // sizes
    const CommitDims D = commit_dims(c);
    const int32_t P = D.P;
    if (c->n_types > 0 && c->types_w != div_up(P, 64))
        return fail(c, MMP_ESTATE, "type bitmaps were loaded for a different pod count; reload them before commit");
    SnapBufs &B = c->sb[1 - c->cur];
    SnapSide &N = c->side[1 - c->cur];
    hipStream_t st = c->stream;
    if (const int rc = ensure_snapshot_buffers(c, B, N, D)) return rc;

    // order check, delta plan
    const OrderCheck oc = check_placement_order(c->pods, D.min_space, D.churn2);
    DeltaRows dl{};
    std::vector<int32_t> new_order;
    bool delta = false;
    if (const int rc = plan_delta(c, D, oc.sort_legal, dl, new_order, delta)) return rc;

    // uploads (a delta takes its rows inside `dl`), with the scratch and the column tails cleared
    if (P && !delta) HIP_TRY(c, hipMemcpyAsync(B.pods.p, c->pods.data(), (size_t)P * sizeof(mmp_pod_row), hipMemcpyHostToDevice, st));
    clear_commit_scratch(c, B, D, st);
    InputStage in;
    if (const int rc = upload_commit_inputs(c, B, N, D.T, false, in, st)) return rc;
    const uint64_t types_gen_uploaded = c->types_gen;  // (marked current once the copies have landed: behind the synchronisation)
    if (const int rc = ensure_audit_multipliers(c, B, D.W, st)) return rc;
    const Snap S = snap_of(B, D);
    if (const int rc = stage_partitions(c, N, P, st)) return rc;

    bool next_long = c->tune.long_mode == 1, next_full = false;
    KT_BEGIN(c, st);
    if (P > 0) {
        // (nearly) every instance full: getNext is in its LRU-window mode and whole-table shortlists are common
        next_full = oc.n_present > 0 && oc.n_nonfull * 16 <= oc.n_present;
        next_long = c->tune.long_mode == 1 || (c->tune.long_mode != 0 && next_full);
        // rank + scatter into the rank-ordered columns
        if (delta) {
            const SnapBufs &A = c->sb[c->cur];
            hipLaunchKernelGGL(delta_scatter_kernel, dim3(div_up(P, 256)), dim3(256), 0, st, A.pods.as<mmp_pod_row>(), A.pos_of.as<int32_t>(),
                               P, dl, B.pods.as<mmp_pod_row>(), c->rank.as<int32_t>(), B.lru.as<int64_t>(), B.rem.as<int64_t>(),
                               B.cnt.as<int32_t>(), B.rpm.as<int32_t>(), B.orig.as<int32_t>(), B.pos_of.as<int32_t>());
        } else {
            const bool want_sort = c->tune.rank_mode == 2 || c->tune.rank_mode == 3 || (c->tune.rank_mode == 0 && P >= kRankSortMinPods);
            if (const int rc = launch_rank(c, B.pods.as<mmp_pod_row>(), P, 0, P, false, want_sort, oc.sort_legal, c->rank.as<int32_t>(), st))
                return rc;
            hipLaunchKernelGGL(scatter_pods_kernel, dim3(div_up(P, 256)), dim3(256), 0, st, B.pods.as<mmp_pod_row>(), P,
                               D.min_space, c->rank.as<int32_t>(), c->occupancy.as<int32_t>(), B.lru.as<int64_t>(),
                               B.rem.as<int64_t>(), B.cnt.as<int32_t>(), B.rpm.as<int32_t>(), B.orig.as<int32_t>(),
                               B.pos_of.as<int32_t>(), c->flag.as<int32_t>());
        }
        launch_mark_replaced(c, B, P, st);
        // level 1, level 2 (the subset stats ride in them), sel / memo, case (b) tables
        launch_snapshot_tables(c, B, N, S, D, st);
        HIP_TRY(c, hipGetLastError());
    } else {
        if (const int rc = clear_snapshot_tables(c, B, D, st)) return rc;
        if (const int rc = launch_subset_stats(c, N, B.pods.as<mmp_pod_row>(), P, D.min_space, st)) return rc;
    }
    if (const int rc = fetch_subset_stats(c, N, st)) return rc;
    KT_END(c, st);
    // the registry view resolved against the new order (still invisible to decisions), queued before the one synchronisation
    if (const int rc = rebuild_resolved(c, N, S, true, false)) return rc;
    int32_t bad = 0, n_bslots = 0;
    StatsAcc acc{};
    if (const int rc = fetch_commit_result(c, N, &bad, &acc, st)) return rc;
    HIP_TRY(c, hipMemcpyAsync(&n_bslots, n_bslots_dev(B), sizeof n_bslots, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    B.types_gen = N.types_gen = c->d_prefer_gen = types_gen_uploaded;
    B.n_bslots = std::min(n_bslots, kBSlots);
    kt_collect(c);
    if (bad)
        return fail(c, MMP_EORDER,
                    "PLACEMENT_ORDER is not a total order on these rows (a full instance with lruTime <= "
                    "2*minChurnAgeMs next to differing instanceVersions); snapshot not published");

    // a type only a few instances may host: its first candidate is usually beyond a lane scan's reach, and only the
    // long variant carries the prefix-table jump that finds it without the wave path
    if (c->tune.long_mode < 0 && acc.sparse_types) next_long = true;
    // publish: the only part of a commit a decision can ever wait for
    std::unique_lock<std::shared_mutex> g(c->mu, std::defer_lock);
    if (!state_locked) g.lock();
    resident_stop(c);  // it answers for the snapshot it was launched with; the next single request starts one on the new
    c->order_total = oc.sort_legal;
    if (delta) {
        c->h_order.swap(new_order);
        for (int32_t q = 0; q < P; q++) c->h_pos[c->h_order[q]] = q;
        c->n_delta_commits++;
    } else
        c->h_order_valid = false;
    c->dirty.clear();
    c->dirty_all = false;
    c->snap_long = next_long;
    c->snap_full = next_full;
    c->snap = S;
    c->cur = 1 - c->cur;
    c->committed = true;
    split_reset(c);
    publish_cluster_stats(c, acc);
    return MMP_OK;
}
}  // namespace

int mmp_snapshot_commit(mmp_ctx *c)
try {
    if (!c) return MMP_EINVAL;
    std::lock_guard<std::mutex> gb(c->batch_mu);
    return commit_staged(c, false);
} MMP_CATCH(c, "mmp_snapshot_commit")

int mmp_delta_commits(mmp_ctx *c, int64_t *n_out)
{
    if (!c || !n_out) return fail(c, MMP_EINVAL, "mmp_delta_commits: null argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    *n_out = c->n_delta_commits;
    return MMP_OK;
}

int mmp_get_order(mmp_ctx *c, int32_t *order_out, int32_t *n_out)
try {
    if (!c || !order_out || !n_out) return fail(c, MMP_EINVAL, "mmp_get_order: null argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    if (!c->committed) return fail(c, MMP_ESTATE, "no committed snapshot");
    if (c->n_shards > 0) return fail(c, MMP_ESTATE, "mmp_get_order: a pod-axis shard holds only its own slice of the order");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const int32_t n = c->stats.instance_count;  // absent rows sort last
    if (n) HIP_TRY(c, copy_sync(c, order_out, c->snap.orig, (size_t)n * 4, hipMemcpyDeviceToHost));
    *n_out = n;
    return MMP_OK;
} MMP_CATCH(c, "mmp_get_order")

int mmp_shortlists(mmp_ctx *c, mmp_shortlist_row *rows, int32_t cap_rows, int32_t *n_rows_out)
try {
    if (!c || !n_rows_out || (!rows && cap_rows > 0) || cap_rows < 0) return fail(c, MMP_EINVAL, "mmp_shortlists: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    if (!c->committed) return fail(c, MMP_ESTATE, "no committed snapshot");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const int32_t nt = c->snap.memo ? std::min(c->snap.T, kWinLds) : 0;
    std::vector<TypeMemo> h((size_t)std::max(nt, 1));  // (whole rows: the records' heads are read below)
    if (nt) HIP_TRY(c, copy_sync(c, h.data(), c->snap.memo, (size_t)nt * sizeof(TypeMemo), hipMemcpyDeviceToHost));
    for (int32_t i = 0; i < 2 * nt && i < cap_rows; i++) {
        const MemoVar &v = h[i >> 1].v[i & 1];
        rows[i] = mmp_shortlist_row{v.valid, v.lo, v.hi, v.ccount};
    }
    *n_rows_out = 2 * nt;
    return MMP_OK;
} MMP_CATCH(c, "mmp_shortlists")

int mmp_long_shortlists(mmp_ctx *c, mmp_shortlist_row *rows, int32_t cap_rows, int32_t *n_rows_out)
try {
    if (!c || !n_rows_out || (!rows && cap_rows > 0) || cap_rows < 0) return fail(c, MMP_EINVAL, "mmp_long_shortlists: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    if (!c->committed) return fail(c, MMP_ESTATE, "no committed snapshot");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const int32_t nt = c->snap.lmemo ? c->snap.T : 0;
    std::vector<LongMemo> h((size_t)std::max(nt, 1) * kLongLevels);
    if (nt) HIP_TRY(c, copy_sync(c, h.data(), c->snap.lmemo, (size_t)nt * kLongLevels * sizeof(LongMemo), hipMemcpyDeviceToHost));
    for (int32_t i = 0; i < 2 * nt && i < cap_rows; i++) {
        const LongMemo &m = h[(size_t)(i >> 1) * kLongLevels];  // (the record of a request that excludes none of the first instances)
        const LongVar &v = m.v[i & 1];
        rows[i] = mmp_shortlist_row{v.valid, m.best0, v.end, v.ccount};
    }
    *n_rows_out = 2 * nt;
    return MMP_OK;
} MMP_CATCH(c, "mmp_long_shortlists")

int mmp_split_batches(mmp_ctx *c, int64_t *n_split_out, int32_t *off_out)
{
    if (!c) return fail(c, MMP_EINVAL, "mmp_split_batches: null context");
    if (n_split_out) *n_split_out = c->n_split.load(std::memory_order_relaxed);
    if (off_out) *off_out = c->split_off.load(std::memory_order_relaxed) ? 1 : 0;
    return MMP_OK;
}

int mmp_cluster_stats(mmp_ctx *c, mmp_stats *out)
try {
    if (!c || !out) return fail(c, MMP_EINVAL, "mmp_cluster_stats: null argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    if (!c->committed) return fail(c, MMP_ESTATE, "no committed snapshot");
    *out = c->stats;
    return MMP_OK;
} MMP_CATCH(c, "mmp_cluster_stats")

namespace {
mmp_stats stats_of(const StatsAcc &a)
{
    mmp_stats s{};
    s.total_capacity = (int64_t)a.total_capacity;
    s.total_free = (int64_t)a.total_free;
    s.global_lru = (int64_t)a.global_lru;
    s.instance_count = a.instance_count;
    s.model_copy_count = a.model_copy_count;
    return s;
}
}  // namespace

int mmp_type_stats(mmp_ctx *c, int32_t type, mmp_stats *out)
try {
    if (!c || !out) return fail(c, MMP_EINVAL, "mmp_type_stats: null argument");
    std::lock_guard<std::shared_mutex> g(c->mu);
    if (!c->committed) return fail(c, MMP_ESTATE, "no committed snapshot");
    const int32_t T = (int32_t)cur_side(c).tstats_h.size();
    *out = stats_of(cur_side(c).tstats_h[(type < 0 || type >= T) ? 0 : type]);
    return MMP_OK;
} MMP_CATCH(c, "mmp_type_stats")

int mmp_partition_count(mmp_ctx *c, int32_t *n_out)
try {
    if (!c || !n_out) return fail(c, MMP_EINVAL, "mmp_partition_count: null argument");
    std::lock_guard<std::shared_mutex> g(c->mu);
    if (!c->committed) return fail(c, MMP_ESTATE, "no committed snapshot");
    *n_out = cur_side(c).n_pts;
    return MMP_OK;
} MMP_CATCH(c, "mmp_partition_count")

int mmp_partition_stats(mmp_ctx *c, int32_t partition, mmp_stats *out, uint64_t *prohibited_out, int32_t max_words)
try {
    if (!c || !out || max_words < 0 || (max_words > 0 && !prohibited_out))
        return fail(c, MMP_EINVAL, "mmp_partition_stats: bad argument");
    std::lock_guard<std::shared_mutex> g(c->mu);
    if (!c->committed) return fail(c, MMP_ESTATE, "no committed snapshot");
    if (partition < 0 || partition >= cur_side(c).n_pts) return fail(c, MMP_EINVAL, "mmp_partition_stats: no partition %d", partition);
    *out = stats_of(cur_side(c).pstats_h[partition]);
    for (int32_t w = 0; w < max_words; w++)
        prohibited_out[w] = w < cur_side(c).pts_tw ? cur_side(c).pts_prohib[(size_t)partition * cur_side(c).pts_tw + w] : 0;
    return MMP_OK;
} MMP_CATCH(c, "mmp_partition_stats")

int mmp_pod_partitions(mmp_ctx *c, int32_t *partition_out, int32_t max_pods, int32_t *n_out)
try {
    if (!c || !n_out || max_pods < 0 || (max_pods > 0 && !partition_out))
        return fail(c, MMP_EINVAL, "mmp_pod_partitions: bad argument");
    std::lock_guard<std::shared_mutex> g(c->mu);
    if (!c->committed) return fail(c, MMP_ESTATE, "no committed snapshot");
    *n_out = (int32_t)cur_side(c).pts_of.size();
    const int32_t m = std::min(*n_out, max_pods);
    if (m > 0) memcpy(partition_out, cur_side(c).pts_of.data(), (size_t)m * 4);
    return MMP_OK;
} MMP_CATCH(c, "mmp_pod_partitions")

/* ---- wire-format ingestion (§8f-1) ------------------------------------------ */

namespace {
// Records per wavefront of the wave-path parsers: a group shares the lanes in the per-field phase (more
// lanes busy), but fewer wavefronts are in flight; keep >= ~8 wavefronts per SIMD before growing the group.
int ingest_group(int32_t n)
{
    static const int forced = [] {
        const char *e = getenv("MMP_JGROUP");
        return e ? atoi(e) : 0;
    }();
    if (forced >= 1 && forced <= kJGroup) return forced;
    int g = 1;
    while (g < kJGroup && n / (g * 2) >= 8192) g *= 2;
    return g;
}

// What every table of this section takes for n keys: a power of two, at least 16 and at least twice the keys
uint32_t tab_capacity(int32_t n)
{
    uint32_t cap = 16;
    while (cap < (uint32_t)n * 2u) cap <<= 1;
    return cap;
}

// MMP_LABEL_HASH_BITS / MMP_MODEL_ID_HASH_BITS: the hashes of a table masked to their low `bits` bits, so that they collide
uint64_t hash_mask(int bits) { return bits >= 64 ? ~0ull : (1ull << bits) - 1ull; }

// off[0 .. n] must not decrease (nor off2[0 .. n], where a call brings two kinds: the first index at which either does is named).
// On its own where a call must refuse before anything is staged; `what`: "", "key " or "id ".
extern "C++" template <class Off, class Off2 = Off>  // (a template inside the file's extern "C" block)
int check_offsets(mmp_ctx *c, const char *fn, const char *what, const Off *off, int32_t n, const Off2 *off2 = nullptr)
{
    for (int32_t i = 0; i < n; i++)
        if (off[i + 1] < off[i] || (off2 && off2[i + 1] < off2[i]))
            return fail(c, MMP_EINVAL, "%s: %soffsets not monotone at %d", fn, what, i);
    return MMP_OK;
}

// n strings of a call onto the device (the device is set, batch_mu held) — the values into j_buf / j_off, ids and event keys
// into ida_bytes / ida_off: off[0 .. n] must not decrease; d_bytes gets the bytes [off[0], off[n]) — none needs no buf —, d_off
// the offsets rebased to off[0].  Both uploads are enqueued on c->stream; `rel` is what d_off is uploaded from (rel[n]: the
// bytes) and stays with the caller until it has synchronised.
extern "C++" template <class Off>
int stage_strings(mmp_ctx *c, const char *fn, const char *what, const char *buf, const Off *off, int32_t n, DevBuf &d_bytes,
                  DevBuf &d_off, std::vector<Off> &rel)
{
    if (const int rc = check_offsets(c, fn, what, off, n)) return rc;
    rel.assign((size_t)n + 1, 0);
    for (int32_t i = 0; i < n; i++) rel[i + 1] = off[i + 1] - off[0];
    const size_t bytes = (size_t)rel[n];
    if (bytes > 0 && !buf) return fail(c, MMP_EINVAL, "%s: bad argument", fn);
    HIP_TRY(c, d_bytes.ensure(bytes + 16));  // the wave path stages whole dwords
    HIP_TRY(c, d_off.ensure((size_t)(n + 1) * sizeof(Off)));
    if (bytes) HIP_TRY(c, hipMemcpyAsync(d_bytes.p, buf + off[0], bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_off.p, rel.data(), (size_t)(n + 1) * sizeof(Off), hipMemcpyHostToDevice, c->stream));
    return MMP_OK;
}

// host side of the open-addressing table the device probes (ingest_kernels.hpp: tab_find)
// (hmask / equal_ok: the label names, whose hashes may be masked down until they are equal — the device then tells them apart by
// their bytes, ingest_kernels.hpp: label_find; the caller has refused equal names)
int build_hash_table(mmp_ctx *c, const char *strs, const int32_t *off, int32_t n, DevBuf &d_hash, DevBuf &d_val,
                     uint32_t &mask_out, const char *what, uint64_t hmask = ~0ull, bool equal_ok = false)
{
    if (const int rc = check_offsets(c, what, "", off, n)) return rc;
    const uint32_t cap = tab_capacity(n);
    std::vector<uint64_t> hs(cap, 0);
    std::vector<int32_t> vs(cap, INT32_MIN);
    for (int32_t i = 0; i < n; i++) {
        const uint64_t h = fnv1a(strs + off[i], off[i + 1] - off[i]) & hmask;
        uint32_t s = tab_home(h, cap - 1);
        while (vs[s] != INT32_MIN) {
            if (hs[s] == h && !equal_ok) return fail(c, MMP_EINVAL, "%s: entries %d and %d are equal or collide under FNV-1a", what, vs[s], i);
            s = (s + 1) & (cap - 1);
        }
        hs[s] = h;
        vs[s] = i;
    }
    HIP_TRY(c, d_hash.ensure((size_t)cap * 8));
    HIP_TRY(c, d_val.ensure((size_t)cap * 4));
    HIP_TRY(c, copy_sync(c, d_hash.p, hs.data(), (size_t)cap * 8, hipMemcpyHostToDevice));
    HIP_TRY(c, copy_sync(c, d_val.p, vs.data(), (size_t)cap * 4, hipMemcpyHostToDevice));
    mask_out = cap - 1;
    return MMP_OK;
}

// An open-addressing table with no key in it (enqueued on c->stream)
int empty_table(mmp_ctx *c, const HashTabW &nt)
{
    HIP_TRY(c, hipMemsetAsync(nt.hash, 0, ((size_t)nt.mask + 1) * 8, c->stream));
    HIP_TRY(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(nt.val), INT32_MIN, (size_t)nt.mask + 1, c->stream));
    return MMP_OK;
}

// The table a call builds beside the published one (cap0 slots; cap0 == 0: there is none), in two steps.  next_table_room: the
// capacity for n_keys keys in all, never below the published one, and next_hash / next_val that large: `nt`.  next_table, inside
// the caller's bracket, enqueued on c->stream: room for the new keys — the slots of hash / val as they are; else the stored
// hashes go into the larger, emptied table (idtab_rehash_kernel reads no key).  `nt` is then ready for the claims of the
// joining keys; the caller swaps the buffers in once they have verified.
int next_table_room(mmp_ctx *c, uint32_t cap0, int32_t n_keys, DevBuf &next_hash, DevBuf &next_val, HashTabW &nt)
{
    const uint32_t cap = std::max(tab_capacity(n_keys), cap0);
    HIP_TRY(c, next_hash.ensure((size_t)cap * 8));
    HIP_TRY(c, next_val.ensure((size_t)cap * 4));
    nt = HashTabW{next_hash.as<uint64_t>(), next_val.as<int32_t>(), cap - 1};
    return MMP_OK;
}
int next_table(mmp_ctx *c, const DevBuf &hash, const DevBuf &val, uint32_t cap0, const HashTabW &nt)
{
    hipStream_t st = c->stream;
    const size_t cap = (size_t)nt.mask + 1;
    if (cap == cap0) {
        HIP_TRY(c, hipMemcpyAsync(nt.hash, hash.p, cap * 8, hipMemcpyDeviceToDevice, st));
        HIP_TRY(c, hipMemcpyAsync(nt.val, val.p, cap * 4, hipMemcpyDeviceToDevice, st));
        return MMP_OK;
    }
    if (const int rc = empty_table(c, nt)) return rc;
    if (cap0)
        hipLaunchKernelGGL(idtab_rehash_kernel, dim3(div_up((int)cap0, kIdTabBlock)), dim3(kIdTabBlock), 0, st, hash.as<uint64_t>(),
                           val.as<int32_t>(), cap0, nt);
    return MMP_OK;
}

// An id table of the context as one host sequence sees it: the model-id table (mid_*) or the vmodel-id table (vid_*).  Both are
// one ModelIdTab on the device, so one sequence drives the kernels of model_ids_kernels.hpp and retire_kernels.hpp for either.
struct IdTabRef {
    DevBuf &hash, &val, &next_hash, &next_val, &bytes, &off;
    uint32_t &mask;
    int32_t &n, &nbytes;
    int32_t hash_bits;
    ModelIdTab published() const { return ModelIdTab{hash.as<uint64_t>(), val.as<int32_t>(), mask, bytes.as<char>(), off.as<int32_t>()}; }
};
extern "C++" IdTabRef model_id_tab(mmp_ctx *c)  // (references: no C linkage inside the file's extern "C" block)
{
    return IdTabRef{c->mid_hash, c->mid_val, c->mid_next_hash, c->mid_next_val, c->mid_bytes, c->mid_off, c->mid_mask, c->mid_n, c->mid_nbytes,
                    c->tune.model_id_hash_bits};
}
extern "C++" IdTabRef vmodel_id_tab(mmp_ctx *c)
{
    return IdTabRef{c->vid_hash, c->vid_val, c->vid_next_hash, c->vid_next_val, c->vid_bytes, c->vid_off, c->vid_mask, c->vid_n, c->vid_nbytes,
                    c->tune.vmodel_id_hash_bits};
}

// ---- The retire frame: what mmp_models_retire, mmp_vmodels_retire and mmp_pods_retire do alike -------------------------------
// A retire call squeezes named indices out of an index space of N0 and answers remap[old] = new or -1.  With batch_mu held:
//   guard     retire_list_guard refuses a list out of range or a remap_out too small; a call that retires nothing answers the
//             identity (retire_nothing) without touching the device;
//   mark      (registry side) retire_mark_scan: keep[index] from the list, the caller's count kernel, the scan that numbers the
//             survivors; ONE host round trip brings back the totals and the guard word (an *_ONLY flag refuses here);
//   build     everything compacted BESIDE what is published, in ScopedDevBufs and the table's next_* pair — for an id table
//             retire_id_table_room ahead of the bracket, retire_id_table inside it: the survivors' stored hashes claimed under
//             their new numbers (retire_table_claim, no key is read), then a verifying lookup in a launch of its own;
//   read      (registry side) retire_build: the SECOND round trip, remap and the lost word; whatever was enqueued has finished
//             before a new buffer may go;
//   publish   the caller's swap under the state lock held EXCLUSIVE (an id table: retire_id_table_publish), and its drain.
// mmp_pods_retire numbers the survivors on the host and reads back one PodsRetireWords: it takes the guard, the table's room, the
// emptying and the claim from here, and has one round trip in all.
struct RetireNoun {
    const char *list, *item, *holder;  // "rows", "row", "the registry"
};
int retire_list_guard(mmp_ctx *c, const char *fn, const RetireNoun &w, const int32_t *list, int32_t n, int32_t N0, const int32_t *remap_out,
                      int32_t max_out)
{
    if (remap_out && max_out < N0) return fail(c, MMP_EINVAL, "%s: room for %d %s in remap_out, %s has %d", fn, max_out, w.list, w.holder, N0);
    for (int32_t i = 0; i < n; i++)
        if (list[i] < 0 || list[i] >= N0) return fail(c, MMP_EINVAL, "%s: %s[%d] names %s %d of %d", fn, w.list, i, w.item, list[i], N0);
    return MMP_OK;
}
int retire_nothing(mmp_ctx *c, int32_t N0, int32_t *remap_out, int32_t *n_after_out)  // nothing leaves: no launch
{
    if (remap_out)
        for (int32_t r = 0; r < N0; r++) remap_out[r] = r;
    if (n_after_out) *n_after_out = N0;
    if (c->prof) c->last_kernel_ms = -1;
    return MMP_OK;
}

// What the mark step brings back: the scan's totals, the guard word (INT32_MAX: nothing refused), the caller's own word read in
// the same round trip, and the bracket's span.  On the device it leaves keep in ret_keep and the scan in me_pos.
extern "C++" template <class Count>
struct RetireMarked {
    Count tot{};
    int32_t refused = INT32_MAX, extra = INT32_MAX;
    double ms = 0;
};
// list == nullptr: no list is staged and keep is not preset (the caller's mark writes every word of it).  enqueue(d_list, d_keep,
// d_word, d_cnt) launches the caller's mark and count kernels inside the bracket; d_extra: a device word of the caller's, or nullptr.
extern "C++" template <class Count, class Plus, class Enqueue>
int retire_mark_scan(mmp_ctx *c, const int32_t *list, int32_t n, int32_t N0, Enqueue &&enqueue, RetireMarked<Count> &R,
                     const int32_t *d_extra = nullptr)
{
    hipStream_t st = c->stream;
    HIP_TRY(c, c->ret_rows.ensure((size_t)std::max(n, 1) * 4));
    HIP_TRY(c, c->ret_keep.ensure((size_t)N0 * 4));
    HIP_TRY(c, c->ret_remap.ensure((size_t)N0 * 4));
    HIP_TRY(c, c->ret_word.ensure(8));
    HIP_TRY(c, c->me_cnt.ensure(((size_t)N0 + 1) * sizeof(Count)));
    HIP_TRY(c, c->me_pos.ensure(((size_t)N0 + 1) * sizeof(Count)));
    Count *d_cnt = c->me_cnt.as<Count>(), *d_pos = c->me_pos.as<Count>();
    int32_t *d_keep = c->ret_keep.as<int32_t>(), *d_word = c->ret_word.as<int32_t>();
    size_t scan_bytes = 0;
    HIP_TRY(c, rocprim::exclusive_scan(nullptr, scan_bytes, d_cnt, d_pos, Count{}, (size_t)N0 + 1, Plus(), st));
    HIP_TRY(c, c->j_scan_tmp.ensure(std::max<size_t>(scan_bytes, 16)));
    if (list) {
        HIP_TRY(c, hipMemcpyAsync(c->ret_rows.p, list, (size_t)n * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_keep), 1, (size_t)N0, st));
    }
    HIP_TRY(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_word), INT32_MAX, 2, st));
    KT_BEGIN(c, st);
    enqueue(c->ret_rows.as<int32_t>(), d_keep, d_word, d_cnt);
    HIP_TRY(c, rocprim::exclusive_scan(c->j_scan_tmp.p, scan_bytes, d_cnt, d_pos, Count{}, (size_t)N0 + 1, Plus(), st));
    KT_END(c, st);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(&R.refused, d_word, 4, hipMemcpyDeviceToHost, st));
    if (d_extra) HIP_TRY(c, hipMemcpyAsync(&R.extra, d_extra, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, copy_sync(c, &R.tot, d_pos + N0, sizeof R.tot, hipMemcpyDeviceToHost));
    kt_collect(c);
    R.ms = c->last_kernel_ms;
    return MMP_OK;
}

// The survivors' stored hashes of the published table hash / val claimed in the emptied `next` under their new numbers (enqueued)
void retire_table_claim(mmp_ctx *c, const DevBuf &hash, const DevBuf &val, uint32_t cap0, const int32_t *d_remap, const HashTabW &next)
{
    hipLaunchKernelGGL(retire_table_kernel, dim3(div_up((int)cap0, kRetireBlock)), dim3(kRetireBlock), 0, c->stream, hash.as<uint64_t>(),
                       val.as<int32_t>(), cap0, d_remap, next);
}

// The compacted id table of T, for `survivors` ids of `bytes` bytes.  _room, ahead of the bracket: the id arena in nb / no, the
// table (it may shrink: tab_capacity(survivors)) in T.next_*, emptied, and new_off[0] = 0.  A failure behind the first enqueue
// waits for the stream before it returns: nb / no go with the caller.
int retire_id_table_room(mmp_ctx *c, const char *fn, const IdTabRef &T, int32_t survivors, int32_t bytes, ScopedDevBuf &nb, ScopedDevBuf &no,
                         HashTabW &next)
{
    if (nb.b.ensure((size_t)bytes + 16) != hipSuccess || no.b.ensure(((size_t)survivors + 1) * 4) != hipSuccess ||
        next_table_room(c, 0, survivors, T.next_hash, T.next_val, next) != MMP_OK)
        return fail(c, MMP_ENOMEM, "%s: out of device memory", fn);
    int rc = empty_table(c, next);
    if (rc == MMP_OK && hipMemsetAsync(no.b.p, 0, 4, c->stream) != hipSuccess) rc = fail(c, MMP_EHIP, "%s: hipMemsetAsync failed", fn);
    if (rc != MMP_OK) (void)hipStreamSynchronize(c->stream);
    return rc;
}
// inside the bracket, behind the caller's move kernel (which wrote d_remap and the arena): the claims, then the verifying lookup of
// every survivor's id in a launch of its own; *d_lost: the lowest new row it did not find
void retire_id_table(mmp_ctx *c, const IdTabRef &T, const int32_t *d_remap, const HashTabW &next, const ScopedDevBuf &nb, const ScopedDevBuf &no,
                     int32_t *d_lost)
{
    const uint32_t cap0 = T.mask + 1;
    retire_table_claim(c, T.hash, T.val, cap0, d_remap, next);
    hipLaunchKernelGGL(retire_verify_kernel, dim3(div_up((int)cap0, kRetireBlock)), dim3(kRetireBlock), 0, c->stream, T.hash.as<uint64_t>(),
                       T.val.as<int32_t>(), cap0, d_remap, ModelIdTab{next.hash, next.val, next.mask, nb.b.as<char>(), no.b.as<int32_t>()}, d_lost);
}
// under the state lock held EXCLUSIVE: the table, the arena and the counts change together; nb / no hold the old arena afterwards
void retire_id_table_publish(const IdTabRef &T, const HashTabW &next, ScopedDevBuf &nb, ScopedDevBuf &no, int32_t survivors, int32_t bytes)
{
    std::swap(T.hash, T.next_hash);
    std::swap(T.val, T.next_val);
    nb.move_into(T.bytes);
    no.move_into(T.off);
    T.mask = next.mask;
    T.n = survivors;
    T.nbytes = bytes;
}

// The second round trip of a registry-side retire.  enqueue() launches the caller's move kernel and, for an id table,
// retire_id_table, inside the bracket; remap (N0 words) and the lost word come back behind them.  The stream is waited for on
// every way out: whatever was enqueued has finished before the caller's new buffers may go.  mark_ms: the first bracket's span.
extern "C++" template <class Enqueue>
int retire_build(mmp_ctx *c, const char *fn, int32_t N0, double mark_ms, Enqueue &&enqueue, std::vector<int32_t> &remap)
{
    hipStream_t st = c->stream;
    const int32_t *d_remap = c->ret_remap.as<int32_t>(), *d_lost = c->ret_word.as<int32_t>() + 1;
    int32_t lost = INT32_MAX;
    KT_BEGIN(c, st);
    enqueue();
    KT_END(c, st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(remap.data(), d_remap, (size_t)N0 * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&lost, d_lost, 4, hipMemcpyDeviceToHost, st);
    const hipError_t se = hipStreamSynchronize(st);
    if (e == hipSuccess) e = se;
    if (e != hipSuccess) return fail(c, MMP_EHIP, "%s: %s", fn, hipGetErrorString(e));
    if (lost != INT32_MAX) return fail(c, MMP_EHIP, "%s: the id of new row %d was not found in the compacted table", fn, lost);
    kt_collect(c);
    kt_add(c, mark_ms);  // the call's device span: mark + scan + move + table + verify
    return MMP_OK;
}

// What ingest_models_kernel is given by either caller, for n staged values of `bytes` bytes: the tables, the per-record status /
// lul / count words, and the parking arrays: ent_cap slots (ingest_kernels.hpp, the parking rule: n entries take >= 5n + 1 bytes
// of JSON).  The rows and the event members are the caller's to set.
int ingest_models_args(mmp_ctx *c, int32_t n, int64_t bytes, IngestModelsArgs &A, size_t &ent_cap)
{
    ent_cap = (size_t)(bytes / kJEntryBytes + 2);
    HIP_TRY(c, c->j_aux.ensure((size_t)(n + 1) * 8));
    HIP_TRY(c, c->j_status.ensure((size_t)n * 4));
    HIP_TRY(c, c->j_cnt.ensure((size_t)(n + 1) * 4));
    HIP_TRY(c, c->j_tmp_pod.ensure(ent_cap * 4));
    HIP_TRY(c, c->j_tmp_time.ensure(ent_cap * 8));
    A = IngestModelsArgs{};
    A.buf = c->j_buf.as<char>();
    A.off = c->j_off.as<int64_t>();
    A.n = n;
    A.ids = HashTab{c->idtab_hash.as<uint64_t>(), c->idtab_val.as<int32_t>(), c->idtab_mask};
    if (c->have_types) {
        A.types = HashTab{c->tytab_hash.as<uint64_t>(), c->tytab_val.as<int32_t>(), c->tytab_mask};
        A.unknown_type = c->unknown_type;
        A.default_type = c->default_type;
    }
    A.last_unload = c->j_aux.as<int64_t>();
    A.status = c->j_status.as<int32_t>();
    A.cnt = c->j_cnt.as<int32_t>();
    A.ent_pod = c->j_tmp_pod.as<int32_t>();
    A.ent_time = c->j_tmp_time.as<int64_t>();
    A.grp = ingest_group(n);
    return MMP_OK;
}
// String.compareTo on ASCII ids == bytewise comparison, shorter prefix first (ids a and b of the context's id store)
bool id_less(const mmp_ctx *c, int32_t a, int32_t b)
{
    const int la = c->id_offs[a + 1] - c->id_offs[a], lb = c->id_offs[b + 1] - c->id_offs[b];
    const int m = memcmp(c->id_bytes.data() + c->id_offs[a], c->id_bytes.data() + c->id_offs[b], (size_t)std::min(la, lb));
    return m != 0 ? m < 0 : la < lb;
}

// interned id.substring(0, 6) of stored id i: a prefix seen before keeps its number, a new one gets the next
int32_t intern_replica_set(mmp_ctx *c, int32_t i)
{
    if (c->id_offs[i + 1] - c->id_offs[i] < 7) return -1;  // MM.java:4769: iid.length() > 6
    return c->rs_intern.emplace(std::string(c->id_bytes.data() + c->id_offs[i], 6), (int32_t)c->rs_intern.size()).first->second;
}
}  // namespace

int mmp_pod_ids_load(mmp_ctx *c, const char *ids, const int32_t *id_off, int32_t n_pods, uint32_t *id_order_out,
                     int32_t *replica_set_out)
try {
    if (!c || n_pods < 0 || !id_off || (n_pods > 0 && !ids)) return fail(c, MMP_EINVAL, "mmp_pod_ids_load: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, quiesce_decisions(c));
    int rc = build_hash_table(c, ids, id_off, n_pods, c->idtab_hash, c->idtab_val, c->idtab_mask, "mmp_pod_ids_load");
    if (rc != MMP_OK) return rc;
    // the ids, their order and the interning stay with the context: mmp_pod_ids_append continues all three
    c->id_bytes.assign(n_pods ? ids + id_off[0] : "", n_pods ? (size_t)(id_off[n_pods] - id_off[0]) : 0);
    c->id_gen++;
    c->id_offs.resize((size_t)n_pods + 1);
    for (int32_t i = 0; i <= n_pods; i++) c->id_offs[i] = id_off[i] - id_off[0];
    c->id_sorted.resize(n_pods);
    for (int32_t i = 0; i < n_pods; i++) c->id_sorted[i] = i;
    std::sort(c->id_sorted.begin(), c->id_sorted.end(), [c](int32_t a, int32_t b) { return id_less(c, a, b); });
    c->id_order_v.assign(n_pods, 0);
    for (int32_t r = 0; r < n_pods; r++) c->id_order_v[c->id_sorted[r]] = (uint32_t)r;
    c->rs_intern.clear();
    c->replica_set_v.assign(n_pods, -1);
    for (int32_t i = 0; i < n_pods; i++) c->replica_set_v[i] = intern_replica_set(c, i);
    const size_t old = c->pods.size();
    c->pods.resize(n_pods);
    c->pod_label_word.assign(n_pods, 0);  // a new index space: the labels of the old one mean nothing in it (as the marks below)
    c->pod_label_count.assign(n_pods, 0);
    c->dirty_all = true;
    for (size_t i = 0; i < (size_t)n_pods; i++) {
        if (i >= old) {
            c->pods[i] = mmp_pod_row{};
            c->pods[i].flags = MMP_POD_TOMBSTONE;
        }
        c->pods[i].id_order = c->id_order_v[i];
        c->pods[i].replica_set = c->replica_set_v[i];
    }
    c->have_ids = true;
    c->miss_n = 0;  // the index space is redefined: marks kept by pod index mean nothing any more (mmp_registry_missing_get)
    if (id_order_out && n_pods) memcpy(id_order_out, c->id_order_v.data(), (size_t)n_pods * 4);
    if (replica_set_out && n_pods) memcpy(replica_set_out, c->replica_set_v.data(), (size_t)n_pods * 4);
    return MMP_OK;
} MMP_CATCH(c, "mmp_pod_ids_load")

namespace {
// The parse stage of the two instance JSON calls (batch_mu and the state lock held, the device set, n > 0): event i's row starts
// from the id attributes of pod src[i] — a negative src[i] leaves them zero: an event nobody applies — and `live`, the values
// are staged and go through ingest_pods_kernel, every event into a row of its own.  Left on the host: the parsed rows, the start
// times, and in status_out the parser's verdict ORed with the labels'.  The caller applies the events; the two differ on purpose.
// The label side is a no-op from end to end while no label names are loaded: the second launch over the staged values (inside
// the same kernel-time bracket), its words / counts / statuses back on the host, and the word and count of an applied event.
struct PodParse {
    std::vector<mmp_pod_row> rows;
    std::vector<int64_t> start;
    int run(mmp_ctx *c, const char *fn, const char *buf, const int64_t *off, int32_t n, const int32_t *src, const uint8_t *live,
            int32_t *status_out)
    {
        hipStream_t st = c->stream;
        rows.assign(n, mmp_pod_row{});
        for (int32_t i = 0; i < n; i++) {
            if (src[i] >= 0) {
                rows[i].id_order = c->id_order_v[src[i]];
                rows[i].replica_set = c->replica_set_v[src[i]];
            }
            rows[i].flags = (!live || live[i]) ? MMP_POD_LIVE : 0u;
        }
        std::vector<int64_t> rel;
        if (const int rc = stage_strings(c, fn, "", buf, off, n, c->j_buf, c->j_off, rel)) return rc;
        HIP_TRY(c, c->j_rows.ensure((size_t)n * sizeof(mmp_pod_row)));
        HIP_TRY(c, c->j_aux.ensure((size_t)n * 8));
        HIP_TRY(c, c->j_status.ensure((size_t)n * 4));
        HIP_TRY(c, hipMemcpyAsync(c->j_rows.p, rows.data(), (size_t)n * sizeof(mmp_pod_row), hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipMemsetAsync(c->j_aux.p, 0, (size_t)n * 8, st));
        labels = c->have_labels;
        labels_cover(c);
        if (labels) HIP_TRY(c, c->j_lab.ensure((size_t)n * 16));
        KT_BEGIN(c, st);
        const int grp = ingest_group(n);
        hipLaunchKernelGGL(ingest_pods_kernel, dim3(div_up(n, kJWaves * grp)), dim3(kJBlock), 0, st, c->j_buf.as<char>(),
                           c->j_off.as<int64_t>(), n, grp, c->j_rows.as<mmp_pod_row>(), c->j_aux.as<int64_t>(), c->j_status.as<int32_t>());
        uint64_t *d_word = labels ? c->j_lab.as<uint64_t>() : nullptr;  // j_lab: words | counts | statuses
        int32_t *d_count = labels ? reinterpret_cast<int32_t *>(d_word + n) : nullptr;
        if (labels) {
            const LabelTab T{HashTab{c->lbtab_hash.as<uint64_t>(), c->lbtab_val.as<int32_t>(), c->lbtab_mask}, c->lb_off.as<int32_t>(),
                             c->lb_arena.as<char>(), c->lb_hmask};
            hipLaunchKernelGGL(ingest_pod_labels_kernel, dim3(div_up(n, kJWaves * grp)), dim3(kJBlock), 0, st, c->j_buf.as<char>(),
                               c->j_off.as<int64_t>(), n, grp, T, d_word, d_count, d_count + n);
        }
        KT_END(c, st);
        HIP_TRY(c, hipGetLastError());
        if (labels) {
            word.resize(n), count.resize(n), status.resize(n);
            HIP_TRY(c, hipMemcpyAsync(word.data(), d_word, (size_t)n * 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(c, hipMemcpyAsync(count.data(), d_count, (size_t)n * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(c, hipMemcpyAsync(status.data(), d_count + n, (size_t)n * 4, hipMemcpyDeviceToHost, st));
        }
        start.resize(n);
        HIP_TRY(c, hipMemcpyAsync(rows.data(), c->j_rows.p, (size_t)n * sizeof(mmp_pod_row), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(start.data(), c->j_aux.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(status_out, c->j_status.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        kt_collect(c);
        if (labels)
            for (int32_t i = 0; i < n; i++) status_out[i] |= status[i];
        return MMP_OK;
    }
    void apply_labels(mmp_ctx *c, int32_t i, int32_t pod) const  // of an applied event i
    {
        if (!labels) return;
        c->pod_label_word[pod] = word[i];
        c->pod_label_count[pod] = count[i];
    }

private:
    bool labels = false;
    std::vector<uint64_t> word;
    std::vector<int32_t> count, status;
};
}  // namespace

int mmp_label_names_load(mmp_ctx *c, const char *names, const int32_t *name_off, int32_t n_labels)
try {
    if (!c || n_labels < 0 || n_labels > 64 || (n_labels > 0 && !name_off))
        return fail(c, MMP_EINVAL, "mmp_label_names_load: bad argument (0 to 64 names)");
    if (const int rc = check_offsets(c, "mmp_label_names_load", "", name_off, n_labels)) return rc;
    const int32_t nbytes = n_labels ? name_off[n_labels] - name_off[0] : 0;
    if (nbytes > 0 && !names) return fail(c, MMP_EINVAL, "mmp_label_names_load: bad argument");
    for (int32_t i = 0; i < n_labels; i++) {
        const char *a = names + name_off[i];
        const int32_t la = name_off[i + 1] - name_off[i];
        for (int32_t q = 0; q < la; q++)  // what cannot stand raw inside a JSON string
            if (a[q] == '"' || a[q] == '\\' || (unsigned char)a[q] < 0x20)
                return fail(c, MMP_EINVAL, "mmp_label_names_load: name %d holds a byte that JSON escapes (0x%02x)", i, (unsigned char)a[q]);
        for (int32_t j = 0; j < i; j++)
            if (name_off[j + 1] - name_off[j] == la && memcmp(names + name_off[j], a, (size_t)la) == 0)
                return fail(c, MMP_EINVAL, "mmp_label_names_load: names %d and %d are equal", j, i);
    }
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (n_labels > 0) {
        const uint64_t hmask = hash_mask(c->tune.label_hash_bits);
        std::vector<int32_t> rel((size_t)n_labels + 1);
        for (int32_t i = 0; i <= n_labels; i++) rel[i] = name_off[i] - name_off[0];
        HIP_TRY(c, c->lb_arena.ensure((size_t)nbytes + 16));
        HIP_TRY(c, c->lb_off.ensure((size_t)(n_labels + 1) * 4));
        c->have_labels = false;  // (a HIP failure below leaves no half-built table in use)
        if (const int rc = build_hash_table(c, names, name_off, n_labels, c->lbtab_hash, c->lbtab_val, c->lbtab_mask, "mmp_label_names_load",
                                            hmask, true))
            return rc;
        if (nbytes) HIP_TRY(c, copy_sync(c, c->lb_arena.p, names + name_off[0], (size_t)nbytes, hipMemcpyHostToDevice));
        HIP_TRY(c, copy_sync(c, c->lb_off.p, rel.data(), (size_t)(n_labels + 1) * 4, hipMemcpyHostToDevice));
        c->lb_hmask = hmask;
    }
    c->have_labels = n_labels > 0;
    c->pod_label_word.assign(c->pods.size(), 0);  // the bits change meaning
    c->pod_label_count.assign(c->pods.size(), 0);
    return MMP_OK;
} MMP_CATCH(c, "mmp_label_names_load")

int mmp_pods_ingest_json(mmp_ctx *c, const char *buf, const int64_t *off, int32_t n, const int32_t *pod_idx,
                         const uint8_t *live, int64_t *start_time_out, int32_t *status_out)
try {
    if (!c || n < 0 || (n > 0 && (!buf || !off || !pod_idx || !status_out)))
        return fail(c, MMP_EINVAL, "mmp_pods_ingest_json: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    if (!c->have_ids) return fail(c, MMP_ESTATE, "mmp_pods_ingest_json: load the instance ids first (mmp_pod_ids_load)");
    if (n == 0) return MMP_OK;
    const int32_t P = (int32_t)c->pods.size();
    for (int32_t i = 0; i < n; i++)
        if (pod_idx[i] < 0 || pod_idx[i] >= P) return fail(c, MMP_EINVAL, "mmp_pods_ingest_json: record %d names pod %d", i, pod_idx[i]);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    PodParse parse;
    if (const int rc = parse.run(c, "mmp_pods_ingest_json", buf, off, n, pod_idx, live, status_out)) return rc;
    for (int32_t i = 0; i < n; i++) {
        if (status_out[i] == 0) {
            c->pods[pod_idx[i]] = parse.rows[i];
            note_dirty(c, pod_idx[i]);
            parse.apply_labels(c, i, pod_idx[i]);
        }
        if (start_time_out) start_time_out[i] = status_out[i] == 0 ? parse.start[i] : 0;  // (the parser leaves 0 for a value IT rejects)
    }
    return MMP_OK;
} MMP_CATCH(c, "mmp_pods_ingest_json")

namespace {
int missing_cover(mmp_ctx *c, int32_t n);  // (defined with the prune below)

// The staged instance table and the id store cover the same indices: mmp_pods_load / mmp_pods_upsert resize the table without
// telling the id store, and an index of one space must not be used in the other.
int id_space_guard(mmp_ctx *c, const char *fn)
{
    if (c->pods.size() + 1 == c->id_offs.size()) return MMP_OK;
    return fail(c, MMP_ESTATE, "%s: the instance table has %d rows for %d loaded ids (mmp_pods_load / mmp_pods_upsert resized it)", fn,
                (int32_t)c->pods.size(), (int32_t)c->id_offs.size() - 1);
}

// The body of mmp_pod_ids_append (batch_mu and the state lock held, the device set, c->have_ids, n_new > 0, the offsets checked):
// the next table is built beside the published one and everything is swapped in only once the new ids have verified.
int pod_ids_append_locked(mmp_ctx *c, const char *fn, const char *ids, const int32_t *id_off, int32_t n_new)
{
    const int32_t P = (int32_t)c->pods.size();
    if (const int rc = id_space_guard(c, fn)) return rc;
    if ((int64_t)P + n_new > INT32_MAX / 4) return fail(c, MMP_EINVAL, "%s: %d + %d ids", fn, P, n_new);
    hipStream_t st = c->stream;
    std::vector<int32_t> rel;
    if (const int rc = stage_strings(c, fn, "id ", ids, id_off, n_new, c->ida_bytes, c->ida_off, rel)) return rc;
    const uint32_t cap0 = c->idtab_mask + 1;
    HashTabW nt;
    if (const int rc = next_table_room(c, cap0, P + n_new, c->idtab_next_hash, c->idtab_next_val, nt)) return rc;
    HIP_TRY(c, c->ida_hash.ensure((size_t)n_new * 8));
    HIP_TRY(c, c->ida_found.ensure((size_t)n_new * 4));
    KT_BEGIN(c, st);
    if (const int rc = next_table(c, c->idtab_hash, c->idtab_val, cap0, nt)) return rc;
    hipLaunchKernelGGL(idtab_insert_kernel, dim3(div_up(n_new, kIdTabBlock)), dim3(kIdTabBlock), 0, st, c->ida_bytes.as<char>(),
                       c->ida_off.as<int32_t>(), n_new, P, nt, c->ida_hash.as<uint64_t>());
    hipLaunchKernelGGL(idtab_verify_kernel, dim3(div_up(n_new, kIdTabBlock)), dim3(kIdTabBlock), 0, st, c->ida_hash.as<uint64_t>(), n_new,
                       HashTab{nt.hash, nt.val, nt.mask}, c->ida_found.as<int32_t>());
    KT_END(c, st);
    HIP_TRY(c, hipGetLastError());
    std::vector<int32_t> found(n_new);
    HIP_TRY(c, copy_sync(c, found.data(), c->ida_found.p, (size_t)n_new * 4, hipMemcpyDeviceToHost));
    kt_collect(c);
    for (int32_t i = 0; i < n_new; i++) {
        if (found[i] == P + i) continue;
        if (found[i] < 0) return fail(c, MMP_EHIP, "%s: id %d was not inserted", fn, P + i);
        // (whichever of two new ids claimed its slot first: the pair is reported lower index first, as the load does)
        return fail(c, MMP_EINVAL, "%s: entries %d and %d are equal or collide under FNV-1a", fn, std::min(found[i], P + i),
                    std::max(found[i], P + i));
    }
    HIP_TRY(c, hipStreamSynchronize(st));
    if (const int rc = missing_cover(c, P + n_new)) return rc;  // the marks stay, the new slots carry none (the last step that can fail)
    // nothing fails from here on: the table, the id store, the order, the interning and the rows change together
    std::swap(c->idtab_hash, c->idtab_next_hash);
    std::swap(c->idtab_val, c->idtab_next_val);
    c->idtab_mask = nt.mask;
    const int32_t base = c->id_offs[P];
    c->id_bytes.append(ids + id_off[0], (size_t)rel[n_new]);
    c->id_gen++;
    for (int32_t i = 1; i <= n_new; i++) c->id_offs.push_back(base + rel[i]);
    std::vector<int32_t> fresh(n_new), merged((size_t)P + n_new);
    for (int32_t i = 0; i < n_new; i++) fresh[i] = P + i;
    const auto less = [c](int32_t a, int32_t b) { return id_less(c, a, b); };
    std::sort(fresh.begin(), fresh.end(), less);
    std::merge(c->id_sorted.begin(), c->id_sorted.end(), fresh.begin(), fresh.end(), merged.begin(), less);
    c->id_sorted.swap(merged);
    c->id_order_v.resize((size_t)P + n_new);
    for (int32_t r = 0; r < P + n_new; r++) c->id_order_v[c->id_sorted[r]] = (uint32_t)r;
    c->replica_set_v.resize((size_t)P + n_new, -1);
    for (int32_t i = P; i < P + n_new; i++) c->replica_set_v[i] = intern_replica_set(c, i);
    c->pods.resize((size_t)P + n_new);
    labels_cover(c);
    for (int32_t i = 0; i < P + n_new; i++) {
        if (i >= P) {
            c->pods[i] = mmp_pod_row{};
            c->pods[i].flags = MMP_POD_TOMBSTONE;
            c->pods[i].replica_set = c->replica_set_v[i];
        }
        c->pods[i].id_order = c->id_order_v[i];
    }
    c->dirty_all = true;  // every row's id_order may have moved: the next commit ranks from scratch
    c->dirty.clear();
    return MMP_OK;
}
}  // namespace

int mmp_pod_ids_append(mmp_ctx *c, const char *ids, const int32_t *id_off, int32_t n_new, uint32_t *id_order_out,
                       int32_t *replica_set_out, int32_t max_pods)
try {
    if (!c || n_new < 0 || !id_off || (n_new > 0 && !ids) || max_pods < 0) return fail(c, MMP_EINVAL, "mmp_pod_ids_append: bad argument");
    // the locks of the load.  The id table is read by the ingest kernels alone, which run under batch_mu: no quiesce_decisions (a
    // decision still waits for the state lock while this call holds it)
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    if (!c->have_ids) return fail(c, MMP_ESTATE, "mmp_pod_ids_append: load the instance ids first (mmp_pod_ids_load)");
    if (const int rc = check_offsets(c, "mmp_pod_ids_append", "id ", id_off, n_new)) return rc;
    const int64_t total = (int64_t)c->pods.size() + n_new;
    if ((id_order_out || replica_set_out) && max_pods < total)
        return fail(c, MMP_EINVAL, "mmp_pod_ids_append: room for %d pods, the table will have %lld", max_pods, (long long)total);
    if (n_new > 0) {
        HIP_TRY(c, hipSetDevice(c->cfg.device));
        if (const int rc = pod_ids_append_locked(c, "mmp_pod_ids_append", ids, id_off, n_new)) return rc;
    }
    const size_t n = std::min(c->id_order_v.size(), c->pods.size());
    if (id_order_out && n) memcpy(id_order_out, c->id_order_v.data(), n * 4);
    if (replica_set_out && n) memcpy(replica_set_out, c->replica_set_v.data(), n * 4);
    return MMP_OK;
} MMP_CATCH(c, "mmp_pod_ids_append")

int mmp_pods_events_json(mmp_ctx *c, const char *keys, const int32_t *key_off, const char *buf, const int64_t *off, int32_t n,
                         const uint8_t *deleted, const uint8_t *live, uint32_t flags, int32_t *pod_idx_out, int64_t *start_time_out,
                         int32_t *status_out, int32_t *n_appended_out)
try {
    if (!c || n < 0 || (flags & ~MMP_PEV_APPEND) || (n > 0 && (!keys || !key_off || !off || !pod_idx_out || !status_out)))
        return fail(c, MMP_EINVAL, "mmp_pods_events_json: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    if (!c->have_ids) return fail(c, MMP_ESTATE, "mmp_pods_events_json: load the instance ids first (mmp_pod_ids_load)");
    // a key resolves to an index of the id space, and step 4 writes the staged row of that index: the two must be one space
    if (const int rc = id_space_guard(c, "mmp_pods_events_json")) return rc;
    if (n_appended_out) *n_appended_out = 0;
    if (n == 0) return MMP_OK;
    // (both kinds, before anything is staged: a refused call changes nothing)
    if (const int rc = check_offsets(c, "mmp_pods_events_json", "", off, n)) return rc;
    if (off[n] > off[0] && !buf) return fail(c, MMP_EINVAL, "mmp_pods_events_json: bad argument");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    // 1. the keys against the id table, a lane per event
    std::vector<int32_t> krel, idx(n);
    if (const int rc = stage_strings(c, "mmp_pods_events_json", "key ", keys, key_off, n, c->ida_bytes, c->ida_off, krel)) return rc;
    HIP_TRY(c, c->ida_found.ensure((size_t)n * 4));
    KT_BEGIN(c, st);
    hipLaunchKernelGGL(resolve_keys_kernel, dim3(div_up(n, kIdTabBlock)), dim3(kIdTabBlock), 0, st, c->ida_bytes.as<char>(),
                       c->ida_off.as<int32_t>(), n, HashTab{c->idtab_hash.as<uint64_t>(), c->idtab_val.as<int32_t>(), c->idtab_mask},
                       c->ida_found.as<int32_t>());
    KT_END(c, st);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, copy_sync(c, idx.data(), c->ida_found.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    kt_collect(c);
    double span_ms = c->last_kernel_ms;
    // 2. the ids nobody knows: with MMP_PEV_APPEND the distinct ones of non-deleted events join, in order of first appearance (a
    // map sized by the unknown keys of the call).  A deletion resolves to such an id only behind the event that made it join.
    const int32_t P0 = (int32_t)c->pods.size();
    const bool append = flags & MMP_PEV_APPEND;
    std::string join_bytes;
    std::vector<int32_t> join_off{0};
    {
        std::unordered_map<std::string, int32_t> joined;
        for (int32_t i = 0; i < n; i++) {
            if (idx[i] >= 0) continue;
            const bool del = deleted && deleted[i];
            if (!append && !del) continue;
            std::string key(keys + key_off[i], (size_t)(key_off[i + 1] - key_off[i]));
            if (del) {
                const auto it = joined.find(key);
                if (it != joined.end()) idx[i] = it->second;
                continue;
            }
            const auto it = joined.emplace(std::move(key), P0 + (int32_t)join_off.size() - 1);
            if (it.second) {
                join_bytes.append(it.first->first);
                join_off.push_back((int32_t)join_bytes.size());
            }
            idx[i] = it.first->second;
        }
    }
    const int32_t n_join = (int32_t)join_off.size() - 1;
    if (n_join > 0) {
        if (const int rc = pod_ids_append_locked(c, "mmp_pods_events_json", join_bytes.data(), join_off.data(), n_join)) return rc;
        span_ms = kt_sum(c, span_ms, c->last_kernel_ms);
    }
    // 3. the values through the parser of mmp_pods_ingest_json, every event into a row of its own
    PodParse parse;
    if (const int rc = parse.run(c, "mmp_pods_events_json", buf, off, n, idx.data(), live, status_out)) return rc;
    kt_add(c, span_ms);  // the call's device span: resolve + join + parse
    // 4. the events in order: a pod ends as its last well-formed or deleted event left it, labels included
    for (int32_t i = 0; i < n; i++) {
        const int32_t k = idx[i];
        pod_idx_out[i] = k;
        int64_t started = 0;
        if (k < 0) {
            status_out[i] = 2;
        } else if (deleted && deleted[i]) {  // mmp_pods_remove
            status_out[i] = 0;
            c->pods[k].flags |= MMP_POD_TOMBSTONE;
            c->pods[k].flags &= ~MMP_POD_LIVE;
            note_dirty(c, k);
        } else if (status_out[i] == 0) {
            c->pods[k] = parse.rows[i];
            note_dirty(c, k);
            parse.apply_labels(c, i, k);
            started = parse.start[i];
        }
        if (start_time_out) start_time_out[i] = started;
    }
    if (n_appended_out) *n_appended_out = n_join;
    return MMP_OK;
} MMP_CATCH(c, "mmp_pods_events_json")

int mmp_type_names_load(mmp_ctx *c, const char *names, const int32_t *name_off, int32_t n_types, int32_t unknown_type)
try {
    if (!c || n_types < 0 || !name_off || (n_types > 0 && !names)) return fail(c, MMP_EINVAL, "mmp_type_names_load: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    int rc = build_hash_table(c, names, name_off, n_types, c->tytab_hash, c->tytab_val, c->tytab_mask, "mmp_type_names_load");
    if (rc != MMP_OK) return rc;
    c->unknown_type = unknown_type;
    c->default_type = unknown_type;
    static const char kDefault[] = "NLCLASSIFIER";
    for (int32_t i = 0; i < n_types; i++)
        if (name_off[i + 1] - name_off[i] == (int)sizeof(kDefault) - 1 && memcmp(names + name_off[i], kDefault, sizeof(kDefault) - 1) == 0)
            c->default_type = i;
    c->have_types = true;
    return MMP_OK;
} MMP_CATCH(c, "mmp_type_names_load")

int mmp_models_ingest_json(mmp_ctx *c, const char *buf, const int64_t *off, int32_t n_models, int64_t *last_unload_out,
                           int32_t *status_out)
try {
    if (!c || n_models < 0 || (n_models > 0 && (!buf || !off || !status_out)))
        return fail(c, MMP_EINVAL, "mmp_models_ingest_json: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    if (!c->have_ids) return fail(c, MMP_ESTATE, "mmp_models_ingest_json: load the instance ids first (mmp_pod_ids_load)");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, quiesce_decisions(c));  // the registry view is replaced in place
    hipStream_t st = c->stream;
    const int32_t n = n_models;
    c->side[0].rmodels_ok = c->side[1].rmodels_ok = false;
    if (n == 0) {
        c->n_models = 0;
        c->n_entries = 0;
        c->ent_live = 0;
        c->m_cnt.clear();
        return MMP_OK;
    }
    std::vector<int64_t> rel;
    if (const int rc = stage_strings(c, "mmp_models_ingest_json", "", buf, off, n, c->j_buf, c->j_off, rel)) return rc;
    // one pass: every record's entries are parked, the counts are scanned, and the entries move to their CSR position — no host
    // round trip in between
    IngestModelsArgs A;
    size_t ent_cap;
    if (const int rc = ingest_models_args(c, n, rel[n], A, ent_cap)) return rc;
    HIP_TRY(c, c->models.ensure((size_t)n * sizeof(mmp_model_row)));
    HIP_TRY(c, hipMemsetAsync(c->models.p, 0, (size_t)n * sizeof(mmp_model_row), st));
    A.rows = c->models.as<mmp_model_row>();
    HIP_TRY(c, c->ent_pod.ensure(ent_cap * 4));
    HIP_TRY(c, c->ent_time.ensure(ent_cap * 8));
    HIP_TRY(c, c->j_offs.ensure((size_t)(n + 1) * 4));
    size_t scan_bytes = 0;
    HIP_TRY(c, rocprim::exclusive_scan(nullptr, scan_bytes, c->j_cnt.as<int32_t>(), c->j_offs.as<int32_t>(), (int32_t)0,
                                       (size_t)n + 1, rocprim::plus<int32_t>(), st));
    HIP_TRY(c, c->j_scan_tmp.ensure(std::max<size_t>(scan_bytes, 16)));
    HIP_TRY(c, hipMemsetAsync(c->j_cnt.as<int32_t>() + n, 0, 4, st));
    KT_BEGIN(c, st);
    hipLaunchKernelGGL(ingest_models_kernel, dim3(div_up(n, kJWaves * A.grp)), dim3(kJBlock), 0, st, A);
    HIP_TRY(c, rocprim::exclusive_scan(c->j_scan_tmp.p, scan_bytes, c->j_cnt.as<int32_t>(), c->j_offs.as<int32_t>(), (int32_t)0,
                                       (size_t)n + 1, rocprim::plus<int32_t>(), st));
    hipLaunchKernelGGL(compact_entries_kernel, dim3(div_up(n, 256)), dim3(256), 0, st, A.off, n, A.cnt, c->j_offs.as<int32_t>(),
                       A.ent_pod, A.ent_time, A.rows, c->ent_pod.as<int32_t>(), c->ent_time.as<int64_t>());
    KT_END(c, st);
    HIP_TRY(c, hipGetLastError());
    int32_t total = 0;
    HIP_TRY(c, hipMemcpyAsync(&total, c->j_offs.as<int32_t>() + n, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(status_out, c->j_status.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (last_unload_out) HIP_TRY(c, hipMemcpyAsync(last_unload_out, c->j_aux.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    c->m_cnt.resize(n);
    HIP_TRY(c, hipMemcpyAsync(c->m_cnt.data(), c->j_cnt.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    kt_collect(c);
    c->n_models = n;
    c->n_entries = total;
    c->ent_live = total;
    return rebuild_resolved(c);
} MMP_CATCH(c, "mmp_models_ingest_json")

namespace {
// What mmp_models_upsert_json and mmp_models_events_json hand to the pipeline they share, all of it on the device: the one resolves
// the events' rows on the host from indices, the other on the device from keys (model_ids_kernels.hpp).
struct UpsertJsonEvents {
    int32_t *slot;            // [n] event -> its row's position among the call's distinct rows in order of first appearance; k for an
                              // event without a row (an unknown id of mmp_models_events_json)
    int32_t *slot_model;      // [k] the registry row of each slot
    int32_t *win;             // [k + 1] -1; win[k] takes the events without a row and is never read
    uint8_t *deleted;         // [n], or nullptr: no event is a deletion
    int32_t *s_cnt, *s_offs;  // [k + 1] each
    int32_t k, count;         // distinct rows (> 0); the registry's rows after the call
};

// j_ev, in words, for n events and room for kcap distinct rows (by index the k of the call, by key n: k is known on the device
// first): slot[n] | slot_model[kcap] | win[kcap + 1] | deleted[n bytes, padded to a word] | s_cnt[kcap + 1] | s_offs[kcap + 1].
// slot .. deleted are what the by-index call uploads in one copy: ev_upload_words of ev_words.  deleted, k and count are the
// caller's to set (deleted to nullptr where no event is a deletion).
size_t ev_upload_words(int32_t n, int32_t kcap) { return (size_t)n + 2 * (size_t)kcap + 1 + ((size_t)n + 3) / 4; }
size_t ev_words(int32_t n, int32_t kcap) { return ev_upload_words(n, kcap) + 2 * ((size_t)kcap + 1); }
UpsertJsonEvents carve(int32_t *base, int32_t n, int32_t kcap, bool scan_words = true)  // (false: base holds the uploaded part only)
{
    UpsertJsonEvents E{};
    E.slot = base;
    E.slot_model = E.slot + n;
    E.win = E.slot_model + kcap;
    E.deleted = reinterpret_cast<uint8_t *>(E.win + kcap + 1);
    if (scan_words) {
        E.s_cnt = base + ev_upload_words(n, kcap);
        E.s_offs = E.s_cnt + kcap + 1;
    }
    return E;
}

// From the events' slots on the device to the rewritten registry (batch_mu held, the device set, n > 0, E.k > 0): the values are
// staged and parsed, each slot's winner picked, the winners' entries appended to the arena and the rows rewritten in place.
// h_model: the rows of the slots on the host, for the m_cnt shadow; given empty it is read back from E.slot_model.  Nothing but
// scratch is written before the last refusal (entry arena overflow).  The caller squeezes the arena afterwards.  with_count: see
// registry_rewrite (it has run, once, exactly when the registry's counts were published).
int models_upsert_json_run(mmp_ctx *c, const char *fn, const char *buf, const int64_t *off, int32_t n, const UpsertJsonEvents &E,
                           std::vector<int32_t> &h_model, int64_t *last_unload_out, int32_t *status_out,
                           const std::function<void()> &with_count = {})
{
    const int32_t k = E.k, count = E.count, M0 = c->n_models;
    hipStream_t st = c->stream;
    std::vector<int64_t> rel;
    if (const int rc = stage_strings(c, fn, "", buf, off, n, c->j_buf, c->j_off, rel)) return rc;
    IngestModelsArgs A;
    size_t ent_cap;
    if (const int rc = ingest_models_args(c, n, rel[n], A, ent_cap)) return rc;
    if ((int64_t)ent_cap > INT32_MAX) return fail(c, MMP_EINVAL, "%s: more than 2^31 entries in one call", fn);
    HIP_TRY(c, c->j_rows.ensure((size_t)n * sizeof(mmp_model_row)));
    int32_t *d_win = E.win, *d_model = E.slot_model, *s_cnt = E.s_cnt, *s_offs = E.s_offs;
    size_t scan_bytes = 0;
    HIP_TRY(c, rocprim::exclusive_scan(nullptr, scan_bytes, s_cnt, s_offs, (int32_t)0, (size_t)k + 1, rocprim::plus<int32_t>(), st));
    HIP_TRY(c, c->j_scan_tmp.ensure(std::max<size_t>(scan_bytes, 16)));
    A.rows = c->j_rows.as<mmp_model_row>();
    A.deleted = E.deleted;
    A.slot = E.slot;
    A.win = d_win;
    // parse the events (entries parked in scratch), pick each row's winner, and size what the winners append
    KT_BEGIN(c, st);
    hipLaunchKernelGGL(ingest_models_kernel, dim3(div_up(n, kJWaves * A.grp)), dim3(kJBlock), 0, st, A);
    hipLaunchKernelGGL(upsert_json_counts_kernel, dim3(div_up(k + 1, 256)), dim3(256), 0, st, d_win, A.cnt, k, s_cnt);
    HIP_TRY(c, rocprim::exclusive_scan(c->j_scan_tmp.p, scan_bytes, s_cnt, s_offs, (int32_t)0, (size_t)k + 1, rocprim::plus<int32_t>(), st));
    KT_END(c, st);
    HIP_TRY(c, hipGetLastError());
    // back to the host: the winners and the per-event counts (for the host shadow) and the arena room needed; no entry, no row
    std::vector<int32_t> h_win(k), h_cnt(n);
    int32_t total = 0;
    HIP_TRY(c, hipMemcpyAsync(h_win.data(), d_win, (size_t)k * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(h_cnt.data(), A.cnt, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&total, s_offs + k, 4, hipMemcpyDeviceToHost, st));
    if (h_model.empty()) {
        h_model.resize(k);
        HIP_TRY(c, hipMemcpyAsync(h_model.data(), d_model, (size_t)k * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(c, hipStreamSynchronize(st));
    kt_collect(c);
    const double parse_ms = c->last_kernel_ms;
    const int32_t base = c->n_entries;
    if ((int64_t)base + total > INT32_MAX)  // (nothing but scratch has been written so far)
        return fail(c, MMP_EINVAL, "%s: entry arena overflow; reload the registry", fn);
    if (const int rc = registry_grow(c, count, base, total)) return rc;
    HIP_TRY(c, c->u_idx.ensure((size_t)k * 4));
    HIP_TRY(c, c->u_rows.ensure((size_t)k * sizeof(mmp_model_row)));
    HIP_TRY(c, hipMemcpyAsync(status_out, c->j_status.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (last_unload_out) HIP_TRY(c, hipMemcpyAsync(last_unload_out, c->j_aux.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    KT_BEGIN(c, st);
    hipLaunchKernelGGL(upsert_json_build_kernel, dim3(div_up(k, 256)), dim3(256), 0, st, d_win, d_model, k, M0, base, s_offs, A.rows, A.off,
                       A.ent_pod, A.ent_time, c->models.as<mmp_model_row>(), c->ent_pod.as<int32_t>(), c->ent_time.as<int64_t>(),
                       c->u_idx.as<int32_t>(), c->u_rows.as<mmp_model_row>());
    HIP_TRY(c, hipGetLastError());
    if (const int rc = registry_rewrite(c, k, count, base + total, true, with_count)) return rc;
    kt_add(c, parse_ms);  // the call's device span: parse + apply
    // the host shadow: a slot without a winner keeps its count (an existing row) or has none (an appended one)
    c->m_cnt.resize(count, 0);
    for (int32_t j = 0; j < k; j++) {
        if (h_win[j] < 0) continue;
        const int32_t cnt = h_cnt[h_win[j]];
        c->ent_live += (int64_t)cnt - c->m_cnt[h_model[j]];
        c->m_cnt[h_model[j]] = cnt;
    }
    return MMP_OK;
}
}  // namespace

int mmp_models_upsert_json(mmp_ctx *c, const char *buf, const int64_t *off, int32_t n, const int32_t *model_idx,
                           const uint8_t *deleted, int64_t *last_unload_out, int32_t *status_out)
try {
    if (!c || n < 0 || (n > 0 && (!off || !model_idx || !status_out)))
        return fail(c, MMP_EINVAL, "mmp_models_upsert_json: bad argument");
    // the locking of mmp_models_upsert: batch_mu for the call; decisions are held off only while the rows are rewritten
    std::lock_guard<std::mutex> gb(c->batch_mu);
    if (!c->have_ids) return fail(c, MMP_ESTATE, "mmp_models_upsert_json: load the instance ids first (mmp_pod_ids_load)");
    if (n == 0) return MMP_OK;
    const int32_t M0 = c->n_models;
    int32_t count = M0;
    // slot = the distinct registry rows of the call in order of first appearance (found through a map sized by the events:
    // nothing here is sized by the registry)
    std::vector<int32_t> h_slot(n), h_model;
    {
        std::unordered_map<int32_t, int32_t> slot_of;
        slot_of.reserve((size_t)n * 2);
        for (int32_t i = 0; i < n; i++) {
            if (model_idx[i] < 0 || model_idx[i] > count)
                return fail(c, MMP_EINVAL, "mmp_models_upsert_json: event %d names model %d of %d", i, model_idx[i], count);
            if (model_idx[i] == count) count++;
            const auto it = slot_of.emplace(model_idx[i], (int32_t)h_model.size());
            if (it.second) h_model.push_back(model_idx[i]);
            h_slot[i] = it.first->second;
        }
    }
    const int32_t k = (int32_t)h_model.size();
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    // what the call uploads of j_ev, carved on the host as it is on the device
    std::vector<int32_t> up(ev_upload_words(n, k), 0);
    const UpsertJsonEvents H = carve(up.data(), n, k, false);
    memcpy(H.slot, h_slot.data(), (size_t)n * 4);
    memcpy(H.slot_model, h_model.data(), (size_t)k * 4);
    std::fill(H.win, H.win + k + 1, -1);
    if (deleted)
        for (int32_t i = 0; i < n; i++) H.deleted[i] = deleted[i] ? 1 : 0;
    HIP_TRY(c, c->j_ev.ensure(ev_words(n, k) * 4));
    UpsertJsonEvents E = carve(c->j_ev.as<int32_t>(), n, k);
    if (!deleted) E.deleted = nullptr;
    E.k = k;
    E.count = count;
    HIP_TRY(c, hipMemcpyAsync(c->j_ev.p, up.data(), up.size() * 4, hipMemcpyHostToDevice, st));
    if (const int rc = models_upsert_json_run(c, "mmp_models_upsert_json", buf, off, n, E, h_model, last_unload_out, status_out)) return rc;
    return squeeze_if_garbage(c);
} MMP_CATCH(c, "mmp_models_upsert_json")

namespace {
// One call's keys resolved, deduplicated and numbered on the device, and the table / arena that would hold the joining ids built
// beside the published ones.  Nothing of the context's published state has changed until model_ids_publish.
struct ModelIdsPlan {
    int32_t k = 0, n_join = 0, join_bytes = 0;  // distinct applicable rows; ids that join; their bytes
    int32_t n_before = 0, bytes_before = 0;
    uint32_t cap = 0;                // capacity of the table built in mid_next_* (0: none was needed)
    ScopedDevBuf fresh_bytes, fresh_off;  // the arena, where it had to move (or is replaced); after model_ids_publish: what it replaced
    bool swapped = false;            // whether the publish retired anything a captured ModelIdTab may name
    std::vector<int32_t> idx;        // model_idx per event
    double ms = 0;                   // device span (profiling)
};

// The staged keys (ida_*) hashed once into me_hash and looked up in `tab` into me_row (enqueued inside the caller's bracket)
void mid_resolve_launch(mmp_ctx *c, int32_t n, const ModelIdTab &tab, int32_t hash_bits)
{
    const dim3 grid(div_up(n, kIdTabBlock)), block(kIdTabBlock);
    hipLaunchKernelGGL(mid_hash_kernel, grid, block, 0, c->stream, c->ida_bytes.as<char>(), c->ida_off.as<int32_t>(), n,
                       hash_mask(hash_bits), c->me_hash.as<uint64_t>());
    hipLaunchKernelGGL(mid_resolve_kernel, grid, block, 0, c->stream, c->ida_bytes.as<char>(), c->ida_off.as<int32_t>(), n,
                       c->me_hash.as<uint64_t>(), tab, c->me_row.as<int32_t>());
}

// batch_mu held, the device set, n > 0, the key offsets monotone.  T: the table the keys belong to.  replace: the keys are a whole
// id space (mmp_model_ids_load) or the table's first (the vmodel table's first call) — resolved against no table, numbered from
// row 0, table and arena built fresh.  deleted: host bytes or nullptr.
int model_ids_plan(mmp_ctx *c, const IdTabRef &T, const char *fn, const char *keys, const int32_t *key_off, int32_t n,
                   const uint8_t *deleted, bool append, bool replace, ModelIdsPlan &P)
{
    if (n > INT32_MAX / 8) return fail(c, MMP_EINVAL, "%s: %d keys in one call", fn, n);
    hipStream_t st = c->stream;
    const int32_t M0 = P.n_before = replace ? 0 : T.n, B0 = P.bytes_before = replace ? 0 : T.nbytes;
    std::vector<int32_t> krel;
    if (const int rc = stage_strings(c, fn, "key ", keys, key_off, n, c->ida_bytes, c->ida_off, krel)) return rc;
    const uint32_t bcap = tab_capacity(n);  // the call-local table: twice the events
    HIP_TRY(c, c->me_hash.ensure((size_t)n * 8));
    HIP_TRY(c, c->me_row.ensure((size_t)n * 4));
    HIP_TRY(c, c->me_slot.ensure((size_t)n * 4));
    HIP_TRY(c, c->me_tab.ensure((size_t)bcap * 3 * 4));
    HIP_TRY(c, c->me_cnt.ensure(((size_t)n + 1) * sizeof(MidCount)));
    HIP_TRY(c, c->me_pos.ensure(((size_t)n + 1) * sizeof(MidCount)));
    HIP_TRY(c, c->me_idx.ensure((size_t)n * 4));
    HIP_TRY(c, c->me_join.ensure((size_t)n * 4));
    HIP_TRY(c, c->me_found.ensure((size_t)n * 4));
    HIP_TRY(c, c->j_ev.ensure(ev_words(n, n) * 4));
    const UpsertJsonEvents E = carve(c->j_ev.as<int32_t>(), n, n);  // (k is known on the device first)
    const MidBatch B{c->me_tab.as<int32_t>(), c->me_tab.as<int32_t>() + bcap, c->me_tab.as<int32_t>() + 2 * (size_t)bcap, bcap - 1};
    const char *d_keys = c->ida_bytes.as<char>();
    const int32_t *d_off = c->ida_off.as<int32_t>();
    const uint64_t *d_hash = c->me_hash.as<uint64_t>();
    const uint8_t *d_del = deleted ? E.deleted : nullptr;
    MidCount *d_cnt = c->me_cnt.as<MidCount>(), *d_pos = c->me_pos.as<MidCount>();
    ModelIdTab cur = T.published();
    if (replace) cur.hash = nullptr;
    if (deleted) HIP_TRY(c, hipMemcpyAsync(E.deleted, deleted, (size_t)n, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemsetAsync(B.owner, 0xff, (size_t)bcap * 4, st));
    HIP_TRY(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(B.first), INT32_MAX, (size_t)bcap * 2, st));
    size_t scan_bytes = 0;
    HIP_TRY(c, rocprim::exclusive_scan(nullptr, scan_bytes, d_cnt, d_pos, MidCount{0, 0, 0}, (size_t)n + 1, MidPlus(), st));
    HIP_TRY(c, c->j_scan_tmp.ensure(std::max<size_t>(scan_bytes, 16)));
    const dim3 grid(div_up(n, kIdTabBlock)), block(kIdTabBlock);
    // 1. hash once; the rows the table knows; the call's own duplicates; the flags and their scan
    KT_BEGIN(c, st);
    mid_resolve_launch(c, n, cur, T.hash_bits);
    hipLaunchKernelGGL(mid_dedupe_kernel, grid, block, 0, st, d_keys, d_off, n, d_hash, d_del, B, c->me_slot.as<int32_t>());
    hipLaunchKernelGGL(mid_flags_kernel, dim3(div_up(n + 1, kIdTabBlock)), block, 0, st, n, c->me_row.as<int32_t>(), c->me_slot.as<int32_t>(), B,
                       d_off, append ? 1 : 0, d_cnt);
    HIP_TRY(c, rocprim::exclusive_scan(c->j_scan_tmp.p, scan_bytes, d_cnt, d_pos, MidCount{0, 0, 0}, (size_t)n + 1, MidPlus(), st));
    KT_END(c, st);
    HIP_TRY(c, hipGetLastError());
    MidCount tot{};
    HIP_TRY(c, copy_sync(c, &tot, d_pos + n, sizeof tot, hipMemcpyDeviceToHost));
    kt_collect(c);
    P.ms = c->last_kernel_ms;
    P.k = tot.slot;
    P.n_join = tot.join;
    P.join_bytes = tot.bytes;
    if ((int64_t)M0 + P.n_join > INT32_MAX / 4) return fail(c, MMP_EINVAL, "%s: %d + %d ids", fn, M0, P.n_join);
    if ((int64_t)B0 + P.join_bytes > INT32_MAX) return fail(c, MMP_EINVAL, "%s: more than 2^31 id bytes", fn);
    // 2. the arena the joining ids are appended to: in place beyond the published rows, or moved when it has to grow
    if (replace) {
        HIP_TRY(c, P.fresh_bytes.b.ensure((size_t)P.join_bytes + 16));
        HIP_TRY(c, P.fresh_off.b.ensure(((size_t)P.n_join + 1) * 4));
        HIP_TRY(c, hipMemsetAsync(P.fresh_off.b.p, 0, 4, st));
    } else {
        if (const int rc = grow_cow(c, T.bytes, (size_t)B0, (size_t)B0 + P.join_bytes, P.fresh_bytes)) return rc;
        if (const int rc = grow_cow(c, T.off, ((size_t)M0 + 1) * 4, ((size_t)M0 + P.n_join + 1) * 4, P.fresh_off)) return rc;
    }
    char *a_bytes = P.fresh_bytes.b.p ? P.fresh_bytes.b.as<char>() : T.bytes.as<char>();
    int32_t *a_off = P.fresh_off.b.p ? P.fresh_off.b.as<int32_t>() : T.off.as<int32_t>();
    // 3. number the events; 4. the next table, copy-on-write, and a verifying lookup in a launch of its own
    KT_BEGIN(c, st);
    hipLaunchKernelGGL(mid_number_kernel, grid, block, 0, st, n, M0, P.k, c->me_row.as<int32_t>(), c->me_slot.as<int32_t>(), B, append ? 1 : 0,
                       d_pos, d_keys, d_off, B0, c->me_idx.as<int32_t>(), E.slot, E.slot_model, c->me_join.as<int32_t>(), a_bytes, a_off);
    if (P.n_join > 0 || replace) {
        const uint32_t cap0 = replace ? 0u : T.mask + 1;
        HashTabW nt;
        if (const int rc = next_table_room(c, cap0, M0 + P.n_join, T.next_hash, T.next_val, nt)) return rc;
        if (const int rc = next_table(c, T.hash, T.val, cap0, nt)) return rc;
        if (P.n_join > 0) {
            const dim3 jgrid(div_up(P.n_join, kIdTabBlock));
            hipLaunchKernelGGL(mid_insert_kernel, jgrid, block, 0, st, P.n_join, c->me_join.as<int32_t>(), d_hash, M0, nt);
            hipLaunchKernelGGL(mid_verify_kernel, jgrid, block, 0, st, P.n_join, c->me_join.as<int32_t>(), d_hash, d_keys, d_off,
                               ModelIdTab{nt.hash, nt.val, nt.mask, a_bytes, a_off}, c->me_found.as<int32_t>());
        }
        P.cap = nt.mask + 1;
    }
    KT_END(c, st);
    HIP_TRY(c, hipGetLastError());
    P.idx.resize(n);
    std::vector<int32_t> found(P.n_join);
    HIP_TRY(c, hipMemcpyAsync(P.idx.data(), c->me_idx.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (P.n_join > 0) HIP_TRY(c, hipMemcpyAsync(found.data(), c->me_found.p, (size_t)P.n_join * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    kt_collect(c);
    P.ms = kt_sum(c, P.ms, c->last_kernel_ms);
    for (int32_t r = 0; r < P.n_join; r++)
        if (found[r] != M0 + r) return fail(c, MMP_EHIP, "%s: id %d was not inserted (the lookup answered %d)", fn, M0 + r, found[r]);
    return MMP_OK;
}

// nothing fails from here on: the table, the arena and the counts change together (batch_mu held, the stream idle; for the
// model-id table the state lock held exclusive as well: the ownership rule at mmp_ctx::mid_hash).  What the swap retires stays
// allocated and unwritten: the old table is mid_next_* now, the old arena stands in the plan's ScopedDevBufs, which release it
// when the plan ends — for the model-id table only behind model_ids_retired_drain.
void model_ids_publish(const IdTabRef &T, ModelIdsPlan &P)
{
    if (P.cap) {
        std::swap(T.hash, T.next_hash);
        std::swap(T.val, T.next_val);
        T.mask = P.cap - 1;
    }
    const bool moved_bytes = P.fresh_bytes.move_into(T.bytes), moved_off = P.fresh_off.move_into(T.off);
    P.swapped = P.cap || moved_bytes || moved_off;
    T.n = P.n_before + P.n_join;
    T.nbytes = P.bytes_before + P.join_bytes;
}

// Behind a publish of the MODEL-id table, with batch_mu and without the state lock: a request call by model id that captured the
// table before the swap may still be running on a latency slot.  It was enqueued under the state lock, so quiesce_decisions sees
// it; once it has drained the retired table may be rewritten (by the next joining call, which finds it as mid_next_*) and the
// retired arena released (by the plan).  Nothing to wait for when the publish swapped nothing (no id joined).
hipError_t model_ids_retired_drain(mmp_ctx *c, const ModelIdsPlan &P) { return P.swapped ? quiesce_decisions(c) : hipSuccess; }

// The registry and the id table cover the same rows: mmp_models_load, mmp_models_ingest_json and an append by index
// (mmp_models_upsert / mmp_models_upsert_json) resize the registry without telling the id table (the rule of id_space_guard).
int model_id_space_guard(mmp_ctx *c, const char *fn)
{
    if (!c->have_model_ids) return fail(c, MMP_ESTATE, "%s: load the model ids first (mmp_model_ids_load)", fn);
    if (c->mid_n == c->n_models) return MMP_OK;
    return fail(c, MMP_ESTATE, "%s: the registry has %d rows for %d loaded model ids (resized by index since mmp_model_ids_load)", fn,
                c->n_models, c->mid_n);
}
}  // namespace

int mmp_model_ids_load(mmp_ctx *c, const char *ids, const int32_t *id_off, int32_t n_models)
try {
    if (!c || n_models < 0 || (n_models > 0 && !id_off)) return fail(c, MMP_EINVAL, "mmp_model_ids_load: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    if (n_models != c->n_models)
        return fail(c, MMP_ESTATE, "mmp_model_ids_load: %d ids for a registry of %d rows", n_models, c->n_models);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    ModelIdsPlan P;
    if (n_models == 0) {  // a valid start: the empty table, every id joins through mmp_models_events_json
        HashTabW nt;
        if (const int rc = next_table_room(c, 0, 0, c->mid_next_hash, c->mid_next_val, nt)) return rc;
        P.cap = nt.mask + 1;
        HIP_TRY(c, P.fresh_bytes.b.ensure(16));
        HIP_TRY(c, P.fresh_off.b.ensure(4));
        if (const int rc = next_table(c, c->mid_hash, c->mid_val, 0, nt)) return rc;
        HIP_TRY(c, hipMemsetAsync(P.fresh_off.b.p, 0, 4, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    } else {
        if (const int rc = model_ids_plan(c, model_id_tab(c), "mmp_model_ids_load", ids, id_off, n_models, nullptr, true, true, P)) return rc;
        if (P.n_join != n_models) {  // up to the first repeat an id's row is its index
            int32_t i = 0;
            while (i < n_models && P.idx[i] == i) i++;
            return fail(c, MMP_EINVAL, "mmp_model_ids_load: ids %d and %d are equal", i < n_models ? P.idx[i] : -1, i);
        }
    }
    {
        std::lock_guard<std::shared_mutex> g(c->mu);  // the swap (the ownership rule at mmp_ctx::mid_hash)
        model_ids_publish(model_id_tab(c), P);
        c->have_model_ids = true;
        c->k_bound = false;  // the keys of bound caches named rows of the replaced table: the contents stay, the binding goes
    }
    HIP_TRY(c, model_ids_retired_drain(c, P));  // request calls by model id that captured the replaced table
    return MMP_OK;
} MMP_CATCH(c, "mmp_model_ids_load")

int mmp_model_ids_resolve(mmp_ctx *c, const char *keys, const int32_t *key_off, int32_t n, int32_t *model_idx_out)
try {
    if (!c || n < 0 || (n > 0 && (!key_off || !model_idx_out))) return fail(c, MMP_EINVAL, "mmp_model_ids_resolve: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    if (const int rc = model_id_space_guard(c, "mmp_model_ids_resolve")) return rc;
    if (n == 0) return MMP_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    std::vector<int32_t> krel;
    if (const int rc = stage_strings(c, "mmp_model_ids_resolve", "key ", keys, key_off, n, c->ida_bytes, c->ida_off, krel)) return rc;
    HIP_TRY(c, c->me_hash.ensure((size_t)n * 8));
    HIP_TRY(c, c->me_row.ensure((size_t)n * 4));
    KT_BEGIN(c, st);
    mid_resolve_launch(c, n, model_id_tab(c).published(), c->tune.model_id_hash_bits);
    KT_END(c, st);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, copy_sync(c, model_idx_out, c->me_row.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    kt_collect(c);
    return MMP_OK;
} MMP_CATCH(c, "mmp_model_ids_resolve")

int mmp_model_ids_get(mmp_ctx *c, int32_t first_row, int32_t n_rows, char *bytes_out, int32_t max_bytes, int32_t *off_out,
                      int32_t *n_bytes_out)
try {
    if (!c || first_row < 0 || n_rows < 0 || !n_bytes_out || max_bytes < 0 || (max_bytes > 0 && !bytes_out))
        return fail(c, MMP_EINVAL, "mmp_model_ids_get: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    if (const int rc = model_id_space_guard(c, "mmp_model_ids_get")) return rc;
    if ((int64_t)first_row + n_rows > c->mid_n)
        return fail(c, MMP_EINVAL, "mmp_model_ids_get: rows [%d, %d + %d) of %d", first_row, first_row, n_rows, c->mid_n);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    std::vector<int32_t> offs((size_t)n_rows + 1);
    HIP_TRY(c, copy_sync(c, offs.data(), c->mid_off.as<int32_t>() + first_row, ((size_t)n_rows + 1) * 4, hipMemcpyDeviceToHost));
    const int32_t nb = offs[n_rows] - offs[0];
    *n_bytes_out = nb;
    if (off_out)
        for (int32_t r = 0; r <= n_rows; r++) off_out[r] = offs[r] - offs[0];
    if (nb > 0 && max_bytes >= nb) HIP_TRY(c, copy_sync(c, bytes_out, c->mid_bytes.as<char>() + offs[0], (size_t)nb, hipMemcpyDeviceToHost));
    if (c->prof) c->last_kernel_ms = -1;  // two copies, no kernel
    return MMP_OK;
} MMP_CATCH(c, "mmp_model_ids_get")

int mmp_models_events_json(mmp_ctx *c, const char *keys, const int32_t *key_off, const char *buf, const int64_t *off, int32_t n,
                           const uint8_t *deleted, uint32_t flags, int32_t *model_idx_out, int64_t *last_unload_out, int32_t *status_out,
                           int32_t *n_appended_out)
try {
    if (!c || n < 0 || (flags & ~MMP_MEV_APPEND) || (n > 0 && (!key_off || !off || !model_idx_out || !status_out)))
        return fail(c, MMP_EINVAL, "mmp_models_events_json: bad argument");
    // the locking of mmp_models_upsert_json.  The id table: built beside the published one under batch_mu, published under the state
    // lock in the hold that publishes the registry's row count, what the swap retired drained before it is reused (the ownership
    // rule at mmp_ctx::mid_hash) — a request call by model id sees this batch before or after, never an id without its row
    std::lock_guard<std::mutex> gb(c->batch_mu);
    if (!c->have_ids) return fail(c, MMP_ESTATE, "mmp_models_events_json: load the instance ids first (mmp_pod_ids_load)");
    // a key resolves to a row of the id space and the pipeline rewrites the registry row of that number: the two must be one space
    if (const int rc = model_id_space_guard(c, "mmp_models_events_json")) return rc;
    if (n_appended_out) *n_appended_out = 0;
    if (n == 0) return MMP_OK;
    // (both kinds, before anything is staged: a refused call changes nothing)
    if (const int rc = check_offsets(c, "mmp_models_events_json", "", off, n, key_off)) return rc;
    if ((off[n] > off[0] && !buf) || (key_off[n] > key_off[0] && !keys)) return fail(c, MMP_EINVAL, "mmp_models_events_json: bad argument");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    ModelIdsPlan P;
    if (const int rc = model_ids_plan(c, model_id_tab(c), "mmp_models_events_json", keys, key_off, n, deleted, flags & MMP_MEV_APPEND, false, P))
        return rc;
    if (P.k > 0) {
        // everything behind the resolution is mmp_models_upsert_json: slot / slot_model are on the device already
        UpsertJsonEvents E = carve(c->j_ev.as<int32_t>(), n, n);  // as model_ids_plan carved it
        if (!deleted) E.deleted = nullptr;
        E.k = P.k;
        E.count = P.n_before + P.n_join;
        HIP_TRY(c, hipMemsetAsync(E.win, 0xff, ((size_t)P.k + 1) * 4, st));
        std::vector<int32_t> h_model;
        const int rc = models_upsert_json_run(c, "mmp_models_events_json", buf, off, n, E, h_model, last_unload_out, status_out,
                                              [&] { model_ids_publish(model_id_tab(c), P); });
        // (whether or not the rest of the run succeeded: a table that was swapped out is drained before this call lets go of it)
        const hipError_t q = model_ids_retired_drain(c, P);
        if (rc != MMP_OK) return rc;
        HIP_TRY(c, q);
        kt_add(c, P.ms);  // the call's device span: resolve + parse + apply
    } else if (c->prof)
        c->last_kernel_ms = P.ms;
    for (int32_t i = 0; i < n; i++) {
        model_idx_out[i] = P.idx[i];
        if (P.idx[i] >= 0) continue;
        status_out[i] = 2;  // an unknown id: nothing was read, nothing changes
        if (last_unload_out) last_unload_out[i] = 0;
    }
    if (n_appended_out) *n_appended_out = P.n_join;
    return P.k > 0 ? squeeze_if_garbage(c) : (int)MMP_OK;
} MMP_CATCH(c, "mmp_models_events_json")

namespace {
// Behind a swap of the vmodel table, with batch_mu and without the state lock (model_ids_retired_drain for the vmodel side): a
// request call by vmodel id that captured the table before the swap may still be running on a latency slot; it was enqueued under
// the state lock, so quiesce_decisions sees it.  Only then may what the swap retired be rewritten (vid_next_*, vm_rows_next: by the
// next event call) or released (the ScopedDevBufs and the plan, when their owner returns).
hipError_t vmodels_retired_drain(mmp_ctx *c, bool swapped) { return swapped ? quiesce_decisions(c) : hipSuccess; }

VmTab vmodel_tab(mmp_ctx *c)
{
    VmTab V{};
    if (c->have_vmodels) V = VmTab{vmodel_id_tab(c).published(), c->vm_rows.as<VmRow>(), c->vm_arena.as<char>(), c->vid_n};
    return V;
}
VmModels vmodel_models(mmp_ctx *c) { return VmModels{model_id_tab(c).published(), c->models.as<mmp_model_row>(), c->n_models}; }

// The vmodel string arena's garbage (batch_mu held, the device set): as squeeze_if_garbage for the entry arena — when the bytes no
// row refers to exceed the live ones, the rows with their new offsets and the squeezed arena are built beside the published ones
// and swapped in under the state lock.
int vmodels_squeeze_if_garbage(mmp_ctx *c)
{
    const int32_t V = c->vid_n;
    if ((int64_t)c->vm_arena_bytes - c->vm_live_bytes <= c->vm_live_bytes) return MMP_OK;
    hipStream_t st = c->stream;
    ScopedDevBuf rows, arena;
    HIP_TRY(c, rows.b.ensure(std::max<size_t>(c->vm_rows.cap, 16)));
    HIP_TRY(c, arena.b.ensure(std::max<size_t>((size_t)c->vm_live_bytes * 2, 16)));
    HIP_TRY(c, c->j_cnt.ensure(((size_t)V + 1) * 4));
    HIP_TRY(c, c->j_offs.ensure(((size_t)V + 1) * 4));
    size_t scan_bytes = 0;
    HIP_TRY(c, rocprim::exclusive_scan(nullptr, scan_bytes, c->j_cnt.as<int32_t>(), c->j_offs.as<int32_t>(), (int32_t)0, (size_t)V + 1,
                                       rocprim::plus<int32_t>(), st));
    HIP_TRY(c, c->j_scan_tmp.ensure(std::max<size_t>(scan_bytes, 16)));
    const double events_ms = c->last_kernel_ms;
    KT_BEGIN(c, st);
    hipLaunchKernelGGL(vm_squeeze_len_kernel, dim3(div_up(V + 1, 256)), dim3(256), 0, st, c->vm_rows.as<VmRow>(), V, c->j_cnt.as<int32_t>());
    HIP_TRY(c, rocprim::exclusive_scan(c->j_scan_tmp.p, scan_bytes, c->j_cnt.as<int32_t>(), c->j_offs.as<int32_t>(), (int32_t)0,
                                       (size_t)V + 1, rocprim::plus<int32_t>(), st));
    if (V > 0)
        hipLaunchKernelGGL(vm_squeeze_copy_kernel, dim3(div_up(V, 256)), dim3(256), 0, st, c->vm_rows.as<VmRow>(), V, c->j_offs.as<int32_t>(),
                           c->vm_arena.as<char>(), rows.b.as<VmRow>(), arena.b.as<char>());
    KT_END(c, st);
    HIP_TRY(c, hipGetLastError());
    int32_t live = 0;
    HIP_TRY(c, copy_sync(c, &live, c->j_offs.as<int32_t>() + V, 4, hipMemcpyDeviceToHost));
    kt_collect(c);
    kt_add(c, events_ms);
    if (live != c->vm_live_bytes) return fail(c, MMP_EHIP, "vmodel arena: %d live bytes on the device, %lld accounted", live, (long long)c->vm_live_bytes);
    {
        std::lock_guard<std::shared_mutex> g(c->mu);
        rows.move_into(c->vm_rows);
        arena.move_into(c->vm_arena);
        c->vm_arena_bytes = live;
    }
    HIP_TRY(c, vmodels_retired_drain(c, true));  // the replaced rows and arena are released behind it, when `rows` / `arena` end
    return MMP_OK;
}
}  // namespace

int mmp_vmodels_events_json(mmp_ctx *c, const char *keys, const int32_t *key_off, const char *buf, const int64_t *off, int32_t n,
                            const uint8_t *deleted, uint32_t flags, int32_t *vmodel_idx_out, int32_t *status_out, int32_t *n_appended_out)
try {
    if (!c || n < 0 || (flags & ~MMP_VMEV_APPEND) || (n > 0 && (!key_off || !off || !vmodel_idx_out || !status_out)))
        return fail(c, MMP_EINVAL, "mmp_vmodels_events_json: bad argument");
    // batch_mu for the call; the table is built beside the published one and swapped under the state lock, and what the swap retired
    // is drained before this call lets go of it (the ownership rule at mmp_ctx::vid_hash)
    std::lock_guard<std::mutex> gb(c->batch_mu);
    if (n_appended_out) *n_appended_out = 0;
    if (n == 0) return MMP_OK;
    // (both kinds, before anything is staged: a refused call changes nothing)
    if (const int rc = check_offsets(c, "mmp_vmodels_events_json", "", off, n, key_off)) return rc;
    if ((off[n] > off[0] && !buf) || (key_off[n] > key_off[0] && !keys)) return fail(c, MMP_EINVAL, "mmp_vmodels_events_json: bad argument");
    for (int32_t i = 0; i < n; i++)
        if (off[i + 1] - off[i] >= kVmMaxValue) return fail(c, MMP_EINVAL, "mmp_vmodels_events_json: value %d has 2^30 bytes or more", i);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    const IdTabRef T = vmodel_id_tab(c);
    ModelIdsPlan P;
    if (const int rc = model_ids_plan(c, T, "mmp_vmodels_events_json", keys, key_off, n, deleted, flags & MMP_VMEV_APPEND, !c->have_vmodels, P))
        return rc;
    const int32_t V0 = P.n_before, V1 = V0 + P.n_join, k = P.k;
    ScopedDevBuf fresh_arena;
    bool rows_beside = false;
    VmBytes tot{0, 0, 0};
    double ms = P.ms;
    if (k > 0) {
        // slot / slot_model are on the device already, as model_ids_plan carved them: the winner rule of mmp_models_upsert_json
        UpsertJsonEvents E = carve(c->j_ev.as<int32_t>(), n, n);
        HIP_TRY(c, hipMemsetAsync(E.win, 0xff, ((size_t)k + 1) * 4, st));
        std::vector<int64_t> rel;
        if (const int rc = stage_strings(c, "mmp_vmodels_events_json", "", buf, off, n, c->j_buf, c->j_off, rel)) return rc;
        HIP_TRY(c, c->vm_ev.ensure((size_t)n * sizeof(VmEvent)));
        HIP_TRY(c, c->j_status.ensure((size_t)n * 4));
        HIP_TRY(c, c->vm_cnt.ensure(((size_t)k + 1) * sizeof(VmBytes)));
        HIP_TRY(c, c->vm_pos.ensure(((size_t)k + 1) * sizeof(VmBytes)));
        // The rows.  A call whose distinct rows all join only appends: in place, beyond the vid_n rows a captured table lists.  One
        // that rewrites a row of a known id, or outgrows the array, builds in vm_rows_next — the published rows copied there first —
        // and the publish swaps the two: a ping-pong pair as mid_next_* is (not a forced grow_cow: no allocation per call), which
        // the drain behind the swap makes free for the next call.
        const size_t rows_want = (size_t)V1 * sizeof(VmRow);
        rows_beside = k > P.n_join || rows_want > c->vm_rows.cap;
        if (rows_beside) {  // (an array that has to grow doubles, as grow_cow's do)
            HIP_TRY(c, c->vm_rows_next.ensure(rows_want > c->vm_rows.cap ? std::max(rows_want, c->vm_rows.cap * 2) : rows_want));
            if (V0 > 0) HIP_TRY(c, hipMemcpyAsync(c->vm_rows_next.p, c->vm_rows.p, (size_t)V0 * sizeof(VmRow), hipMemcpyDeviceToDevice, st));
        }
        VmBytes *d_cnt = c->vm_cnt.as<VmBytes>(), *d_pos = c->vm_pos.as<VmBytes>();
        size_t scan_bytes = 0;
        HIP_TRY(c, rocprim::exclusive_scan(nullptr, scan_bytes, d_cnt, d_pos, VmBytes{0, 0, 0}, (size_t)k + 1, VmBytesPlus(), st));
        HIP_TRY(c, c->j_scan_tmp.ensure(std::max<size_t>(scan_bytes, 16)));
        VmParseArgs A{c->j_buf.as<char>(), c->j_off.as<int64_t>(), n, ingest_group(n), deleted ? E.deleted : nullptr, E.slot, E.win,
                      c->vm_ev.as<VmEvent>(), c->j_status.as<int32_t>()};
        // parse the events, pick each row's winner, and size what the winners append
        KT_BEGIN(c, st);
        hipLaunchKernelGGL(vm_parse_kernel, dim3(div_up(n, kJWaves * A.grp)), dim3(kJBlock), 0, st, A);
        hipLaunchKernelGGL(vm_counts_kernel, dim3(div_up(k + 1, 256)), dim3(256), 0, st, E.win, A.ev, k, E.slot_model, V0, c->vm_rows.as<VmRow>(),
                           d_cnt);
        HIP_TRY(c, rocprim::exclusive_scan(c->j_scan_tmp.p, scan_bytes, d_cnt, d_pos, VmBytes{0, 0, 0}, (size_t)k + 1, VmBytesPlus(), st));
        KT_END(c, st);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, copy_sync(c, &tot, d_pos + k, sizeof tot, hipMemcpyDeviceToHost));
        kt_collect(c);
        ms = kt_sum(c, ms, c->last_kernel_ms);
        const int32_t base = c->vm_arena_bytes;
        if ((int64_t)base + tot.add > INT32_MAX)  // (nothing but scratch has been written so far)
            return fail(c, MMP_EINVAL, "mmp_vmodels_events_json: more than 2^31 bytes in the string arena");
        if (const int rc = grow_cow(c, c->vm_arena, (size_t)base, (size_t)base + tot.add + 16, fresh_arena)) return rc;
        VmRow *rows = rows_beside ? c->vm_rows_next.as<VmRow>() : c->vm_rows.as<VmRow>();
        char *arena = fresh_arena.b.p ? fresh_arena.b.as<char>() : c->vm_arena.as<char>();
        // nothing is refused from here on: the winners' strings behind the published bytes, the rows beside the published ones
        KT_BEGIN(c, st);
        hipLaunchKernelGGL(vm_build_kernel, dim3(div_up(k, 256)), dim3(256), 0, st, E.win, E.slot_model, k, V0, base, d_pos, A.ev, A.buf, A.off,
                           hash_mask(c->tune.model_id_hash_bits), rows, arena);
        KT_END(c, st);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(status_out, c->j_status.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        kt_collect(c);
        ms = kt_sum(c, ms, c->last_kernel_ms);
    }
    if (c->prof) c->last_kernel_ms = ms;
    {
        std::lock_guard<std::shared_mutex> g(c->mu);  // table, arenas and counts change together
        model_ids_publish(T, P);
        if (rows_beside) std::swap(c->vm_rows, c->vm_rows_next);
        fresh_arena.move_into(c->vm_arena);
        c->vm_arena_bytes += tot.add;
        c->vm_live_bytes += (int64_t)tot.add - tot.sub;
        c->vm_live_rows += tot.live;
        c->have_vmodels = true;
    }
    // request calls by vmodel id that captured what the swap retired: the id table (rewritten by the next joining call), the rows
    // (by the next call that rewrites one), the arenas (released when this call returns)
    HIP_TRY(c, vmodels_retired_drain(c, P.swapped || rows_beside || fresh_arena.b.p != nullptr));
    for (int32_t i = 0; i < n; i++) {
        vmodel_idx_out[i] = P.idx[i];
        if (P.idx[i] < 0) status_out[i] = 2;  // an unknown id: nothing was read, nothing changes
    }
    if (n_appended_out) *n_appended_out = P.n_join;
    return vmodels_squeeze_if_garbage(c);
} MMP_CATCH(c, "mmp_vmodels_events_json")

int mmp_vmodels_resolve(mmp_ctx *c, const char *keys, const int32_t *key_off, int32_t n, const char *nf_keys, const int32_t *nf_off,
                        const char *owners, const int32_t *owner_off, const uint32_t *req_flags, mmp_vmodel_answer *rows_out)
try {
    if (!c || n < 0 || (n > 0 && (!key_off || !rows_out))) return fail(c, MMP_EINVAL, "mmp_vmodels_resolve: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    if (const int rc = model_id_space_guard(c, "mmp_vmodels_resolve")) return rc;
    if (n == 0) return MMP_OK;
    // (all three kinds and the flags, before anything is staged)
    if (const int rc = check_offsets(c, "mmp_vmodels_resolve", "key ", key_off, n)) return rc;
    if (nf_off)
        if (const int rc = check_offsets(c, "mmp_vmodels_resolve", "nf ", nf_off, n)) return rc;
    if (owner_off)
        if (const int rc = check_offsets(c, "mmp_vmodels_resolve", "owner ", owner_off, n)) return rc;
    if ((key_off[n] > key_off[0] && !keys) || (nf_off && nf_off[n] > nf_off[0] && !nf_keys) || (owner_off && owner_off[n] > owner_off[0] && !owners))
        return fail(c, MMP_EINVAL, "mmp_vmodels_resolve: bad argument");
    if (req_flags)
        for (int32_t i = 0; i < n; i++)
            if (req_flags[i] & ~MMP_VMRQ_AFTER_STRONG) return fail(c, MMP_EINVAL, "mmp_vmodels_resolve: request %d has unknown flag bits", i);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    std::vector<int32_t> krel, nrel, orel;
    if (const int rc = stage_strings(c, "mmp_vmodels_resolve", "key ", keys, key_off, n, c->ida_bytes, c->ida_off, krel)) return rc;
    if (nf_off)
        if (const int rc = stage_strings(c, "mmp_vmodels_resolve", "nf ", nf_keys, nf_off, n, c->vm_nf_bytes, c->vm_nf_off, nrel)) return rc;
    if (owner_off)
        if (const int rc = stage_strings(c, "mmp_vmodels_resolve", "owner ", owners, owner_off, n, c->vm_ow_bytes, c->vm_ow_off, orel)) return rc;
    if (req_flags) {
        HIP_TRY(c, c->vm_rflags.ensure((size_t)n * 4));
        HIP_TRY(c, hipMemcpyAsync(c->vm_rflags.p, req_flags, (size_t)n * 4, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(c, c->vm_ans.ensure((size_t)n * sizeof(mmp_vmodel_answer)));
    KT_BEGIN(c, st);
    hipLaunchKernelGGL(vm_resolve_kernel, dim3(div_up(n, kIdTabBlock)), dim3(kIdTabBlock), 0, st, c->ida_bytes.as<char>(), c->ida_off.as<int32_t>(),
                       n, hash_mask(c->tune.vmodel_id_hash_bits), nf_off ? c->vm_nf_bytes.as<char>() : nullptr,
                       nf_off ? c->vm_nf_off.as<int32_t>() : nullptr, owner_off ? c->vm_ow_bytes.as<char>() : nullptr,
                       owner_off ? c->vm_ow_off.as<int32_t>() : nullptr, req_flags ? c->vm_rflags.as<uint32_t>() : nullptr, vmodel_tab(c),
                       vmodel_models(c), c->vm_ans.as<mmp_vmodel_answer>());
    KT_END(c, st);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, copy_sync(c, rows_out, c->vm_ans.p, (size_t)n * sizeof(mmp_vmodel_answer), hipMemcpyDeviceToHost));
    kt_collect(c);
    return MMP_OK;
} MMP_CATCH(c, "mmp_vmodels_resolve")

int mmp_vmodels_transitions(mmp_ctx *c, int64_t now_ms, int64_t lastused_age_on_add_ms, mmp_vmodel_transition *rows_out, int32_t max_rows,
                            int32_t *n_out, mmp_vmodel_transitions_info *info_out)
try {
    if (!c || !n_out || max_rows < 0 || (max_rows > 0 && !rows_out)) return fail(c, MMP_EINVAL, "mmp_vmodels_transitions: bad argument");
    // read-only, the locking of mmp_registry_unresolved: batch_mu owns c->stream and the plans' scratch
    std::lock_guard<std::mutex> gb(c->batch_mu);
    if (const int rc = model_id_space_guard(c, "mmp_vmodels_transitions")) return rc;
    *n_out = 0;
    if (info_out) *info_out = mmp_vmodel_transitions_info{};
    const int32_t V = c->have_vmodels ? c->vid_n : 0;
    if (V == 0) return MMP_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    const int nb = div_up(V, kVmBlock);
    const int32_t cap = std::min(max_rows, V);
    HIP_TRY(c, c->plan.totals.ensure(sizeof(PruneScalars)));
    HIP_TRY(c, c->plan.block_counts.ensure((size_t)nb * 3 * 4));
    HIP_TRY(c, c->vm_list.ensure((size_t)std::max(cap, 1) * sizeof(mmp_vmodel_transition)));
    int32_t *counts = c->plan.block_counts.as<int32_t>();
    PruneScalars *ps = c->plan.totals.as<PruneScalars>();
    const VmTransArgs A{vmodel_tab(c), vmodel_models(c), now_ms, lastused_age_on_add_ms};
    KT_BEGIN(c, st);
    hipLaunchKernelGGL(vm_trans_count_kernel, dim3(nb), dim3(kVmBlock), 0, st, A, counts);
    hipLaunchKernelGGL(prune_scan_kernel, dim3(1), dim3(256), 0, st, counts, nb, INT32_MAX, INT32_MAX, ps);
    if (cap > 0) hipLaunchKernelGGL(vm_trans_list_kernel, dim3(nb), dim3(kVmBlock), 0, st, A, counts, c->vm_list.as<mmp_vmodel_transition>(), cap);
    KT_END(c, st);
    HIP_TRY(c, hipGetLastError());
    PruneScalars h{};
    HIP_TRY(c, copy_sync(c, &h, ps, sizeof h, hipMemcpyDeviceToHost));
    kt_collect(c);
    const int32_t take = std::min(h.n_edits, cap);
    if (take > 0) HIP_TRY(c, copy_sync(c, rows_out, c->vm_list.p, (size_t)take * sizeof(mmp_vmodel_transition), hipMemcpyDeviceToHost));
    *n_out = h.n_edits;
    if (info_out) {
        info_out->n_listed = h.n_edits;
        info_out->n_promote = h.n_removed;
        info_out->n_ensure_loaded = h.n_edits - h.n_removed;
        info_out->n_host_skipped = h.n_kept;
        info_out->truncated = h.n_edits > max_rows ? 1 : 0;
    }
    return MMP_OK;
} MMP_CATCH(c, "mmp_vmodels_transitions")

int mmp_vmodels_get(mmp_ctx *c, int32_t first_row, int32_t n_rows, char *id_bytes_out, int32_t max_id_bytes, int32_t *id_off_out,
                    int32_t *n_id_bytes_out, uint32_t *flags_out, char *str_bytes_out, int32_t max_str_bytes, int32_t *str_off_out,
                    int32_t *n_str_bytes_out)
try {
    if (!c || first_row < 0 || n_rows < 0 || !n_id_bytes_out || !n_str_bytes_out || max_id_bytes < 0 || max_str_bytes < 0 ||
        (max_id_bytes > 0 && !id_bytes_out) || (max_str_bytes > 0 && !str_bytes_out))
        return fail(c, MMP_EINVAL, "mmp_vmodels_get: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    const int32_t V = c->have_vmodels ? c->vid_n : 0;
    if ((int64_t)first_row + n_rows > V)
        return fail(c, MMP_EINVAL, "mmp_vmodels_get: rows [%d, %d + %d) of %d", first_row, first_row, n_rows, V);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    std::vector<int32_t> offs((size_t)n_rows + 1, 0);
    std::vector<VmRow> rows((size_t)n_rows);
    std::vector<char> arena;
    if (n_rows > 0) {
        HIP_TRY(c, copy_sync(c, offs.data(), c->vid_off.as<int32_t>() + first_row, ((size_t)n_rows + 1) * 4, hipMemcpyDeviceToHost));
        HIP_TRY(c, copy_sync(c, rows.data(), c->vm_rows.as<VmRow>() + first_row, (size_t)n_rows * sizeof(VmRow), hipMemcpyDeviceToHost));
    }
    int64_t sb = 0;
    for (const VmRow &r : rows) sb += (int64_t)r.len[0] + r.len[1] + r.len[2];
    if (sb > INT32_MAX) return fail(c, MMP_EINVAL, "mmp_vmodels_get: more than 2^31 string bytes; ask for fewer rows");
    const int32_t nb = offs[n_rows] - offs[0];
    const bool want_str = sb > 0 && max_str_bytes >= sb;
    if (want_str) {  // the rows' strings lie anywhere in the arena: one copy of it, sliced here
        arena.resize((size_t)c->vm_arena_bytes);
        HIP_TRY(c, copy_sync(c, arena.data(), c->vm_arena.p, arena.size(), hipMemcpyDeviceToHost));
    }
    if (nb > 0 && max_id_bytes >= nb)
        HIP_TRY(c, copy_sync(c, id_bytes_out, c->vid_bytes.as<char>() + offs[0], (size_t)nb, hipMemcpyDeviceToHost));
    *n_id_bytes_out = nb;
    *n_str_bytes_out = (int32_t)sb;
    if (id_off_out)
        for (int32_t r = 0; r <= n_rows; r++) id_off_out[r] = offs[r] - offs[0];
    int32_t o = 0;
    for (int32_t r = 0; r < n_rows; r++) {
        if (flags_out) flags_out[r] = rows[r].flags;
        for (int s = 0; s < 3; s++) {
            if (str_off_out) str_off_out[3 * r + s] = o;
            if (want_str && rows[r].len[s]) memcpy(str_bytes_out + o, arena.data() + rows[r].off[s], (size_t)rows[r].len[s]);
            o += rows[r].len[s];
        }
    }
    if (str_off_out) str_off_out[3 * (size_t)n_rows] = o;
    if (c->prof) c->last_kernel_ms = -1;  // copies, no kernel
    return MMP_OK;
} MMP_CATCH(c, "mmp_vmodels_get")

int mmp_vmodels_info(mmp_ctx *c, mmp_vmodels_stats *out)
try {
    if (!c || !out) return fail(c, MMP_EINVAL, "mmp_vmodels_info: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    *out = mmp_vmodels_stats{};
    if (!c->have_vmodels) return MMP_OK;
    out->n_rows = c->vid_n;
    out->n_live = c->vm_live_rows;
    out->arena_bytes = c->vm_arena_bytes;
    out->live_bytes = c->vm_live_bytes;
    out->capacity = (int32_t)(c->vid_mask + 1);
    return MMP_OK;
} MMP_CATCH(c, "mmp_vmodels_info")

int mmp_vmodels_retire(mmp_ctx *c, const int32_t *rows, int32_t n, uint32_t flags, int32_t *remap_out, int32_t max_vmodels,
                       int32_t *n_vmodels_after_out)
try {
    const bool all = flags & MMP_VMRETIRE_ALL_ABSENT;
    if (!c || n < 0 || (n > 0 && !rows) || (flags & ~(MMP_VMRETIRE_ABSENT_ONLY | MMP_VMRETIRE_ALL_ABSENT)) || max_vmodels < 0)
        return fail(c, MMP_EINVAL, "mmp_vmodels_retire: bad argument");
    if (all && n > 0) return fail(c, MMP_EINVAL, "mmp_vmodels_retire: MMP_VMRETIRE_ALL_ABSENT takes no list (n = %d)", n);
    // The retire frame (at retire_list_guard).  Its own: the state lock for the swap only, the drain BEHIND the hold (the request calls
    // by vmodel id go on reading the old table from the latency slots); no decision kernel reads a vmodel row: no rebuild_resolved.
    std::lock_guard<std::mutex> gb(c->batch_mu);
    const char *fn = "mmp_vmodels_retire";
    const int32_t V0 = c->have_vmodels ? c->vid_n : 0;
    if (const int rc = retire_list_guard(c, fn, RetireNoun{"rows", "row", "the table"}, rows, n, V0, remap_out, max_vmodels)) return rc;
    if (all ? c->vm_live_rows == V0 : n == 0) return retire_nothing(c, V0, remap_out, n_vmodels_after_out);  // (no squeeze either)
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    const IdTabRef T = vmodel_id_tab(c);
    const dim3 block(kRetireBlock), vgrid(div_up(V0, kRetireBlock));
    const VmRow *old_rows = c->vm_rows.as<VmRow>();
    // mark — the list, and with ABSENT_ONLY the lowest named row that is not ABSENT, or every ABSENT row
    RetireMarked<VmRetireCount> K;
    if (const int rc = retire_mark_scan<VmRetireCount, VmRetirePlus>(
            c, all ? nullptr : rows, n, V0,
            [&](const int32_t *d_list, int32_t *d_keep, int32_t *d_word, VmRetireCount *d_cnt) {
                if (all)
                    hipLaunchKernelGGL(vm_retire_absent_kernel, vgrid, block, 0, st, V0, old_rows, d_keep);
                else
                    hipLaunchKernelGGL(vm_retire_mark_kernel, dim3(div_up(n, kRetireBlock)), block, 0, st, d_list, n, old_rows,
                                       (flags & MMP_VMRETIRE_ABSENT_ONLY) ? 1 : 0, d_keep, d_word);
                hipLaunchKernelGGL(vm_retire_count_kernel, dim3(div_up(V0 + 1, kRetireBlock)), block, 0, st, V0, d_keep, old_rows, T.off.as<int32_t>(),
                                   d_cnt);
            },
            K))
        return rc;
    if (K.refused != INT32_MAX)
        return fail(c, MMP_EINVAL, "%s: row %d is not ABSENT (set again since its deletion?); nothing was retired", fn, K.refused);
    const int32_t V1 = K.tot.row, B1 = K.tot.bytes, S1 = K.tot.strs;
    // build: the compacted rows, string arena, id arena and table
    std::vector<int32_t> remap((size_t)V0);
    ScopedDevBuf nr, na, nb, no;
    HashTabW next{};
    if (nr.b.ensure((size_t)std::max(V1, 1) * sizeof(VmRow)) != hipSuccess || na.b.ensure((size_t)S1 + 16) != hipSuccess)
        return fail(c, MMP_ENOMEM, "%s: out of device memory", fn);
    if (const int rc = retire_id_table_room(c, fn, T, V1, B1, nb, no, next)) return rc;
    const VmRetireMove A{old_rows, c->vm_arena.as<char>(), T.bytes.as<char>(), T.off.as<int32_t>(), nr.b.as<VmRow>(), na.b.as<char>(),
                         nb.b.as<char>(), no.b.as<int32_t>()};
    int32_t *d_remap = c->ret_remap.as<int32_t>();
    const int rc = retire_build(c, fn, V0, K.ms, [&] {
        hipLaunchKernelGGL(vm_retire_move_kernel, vgrid, block, 0, st, V0, c->ret_keep.as<int32_t>(), c->me_pos.as<VmRetireCount>(), A, d_remap);
        retire_id_table(c, T, d_remap, next, nb, no, c->ret_word.as<int32_t>() + 1);
    }, remap);
    if (rc != MMP_OK) return rc;
    {
        std::lock_guard<std::shared_mutex> g(c->mu);  // nothing fails from here on: rows, arenas, table and counts change together
        nr.move_into(c->vm_rows);
        na.move_into(c->vm_arena);
        retire_id_table_publish(T, next, nb, no, V1, B1);
        c->vm_arena_bytes = S1;
        c->vm_live_bytes = S1;
        c->vm_live_rows = K.tot.live;
        c->have_vmodels = V1 > 0;  // (no row: the state before the first vmodel call, which the next event batch starts from)
    }
    // a request call by vmodel id saw the numbering before the swap or sees the one after it; the ones that captured the old rows,
    // arenas and table are drained before nr / na / nb / no release those and the next event call rewrites vid_next_*
    HIP_TRY(c, vmodels_retired_drain(c, true));
    if (remap_out) memcpy(remap_out, remap.data(), (size_t)V0 * 4);
    if (n_vmodels_after_out) *n_vmodels_after_out = V1;
    return MMP_OK;
} MMP_CATCH(c, "mmp_vmodels_retire")

int mmp_models_retire(mmp_ctx *c, const int32_t *rows, int32_t n, uint32_t flags, int32_t *remap_out, int32_t max_models,
                      int32_t *n_models_after_out)
try {
    if (!c || n < 0 || (n > 0 && !rows) || (flags & ~MMP_RETIRE_EMPTY_ONLY) || max_models < 0)
        return fail(c, MMP_EINVAL, "mmp_models_retire: bad argument");
    // The retire frame (at retire_list_guard).  Its own: the drain INSIDE the hold, which also covers the re-resolution.
    std::lock_guard<std::mutex> gb(c->batch_mu);
    const char *fn = "mmp_models_retire";
    const int32_t M0 = c->n_models;
    const bool ids = c->have_model_ids;
    if (ids && c->mid_n != M0)
        return fail(c, MMP_ESTATE, "%s: the registry has %d rows for %d loaded model ids (resized by index since mmp_model_ids_load)", fn, M0, c->mid_n);
    if (const int rc = retire_list_guard(c, fn, RetireNoun{"rows", "row", "the registry"}, rows, n, M0, remap_out, max_models)) return rc;
    if (n == 0) return retire_nothing(c, M0, remap_out, n_models_after_out);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    const IdTabRef T = model_id_tab(c);
    const dim3 block(kRetireBlock);
    const int32_t *old_off = ids ? T.off.as<int32_t>() : nullptr;
    // bound caches are carried along (cache_keyed_kernels.hpp); the cache calls hold batch_mu too, so the store stands still
    const bool carry = c->k_bound && c->k_caches > 0 && c->k_slots > 0;
    mmp_ctx::KeyedStore &KS = c->ks[c->ks_cur];
    const CacheStore kstore{KS.off.as<int32_t>(), KS.lu.as<int64_t>(), KS.wt.as<int32_t>(), KS.key.as<int32_t>(), KS.n.as<int32_t>()};
    int32_t *d_live_key = nullptr;
    if (carry) {
        HIP_TRY(c, c->k_len.ensure(4));
        d_live_key = c->k_len.as<int32_t>();
        HIP_TRY(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_live_key), INT32_MAX, 1, st));
    }
    // mark, and with the flag the lowest named row that is not empty; with bound caches the lowest that is the key of a live entry
    RetireMarked<RetireCount> K;
    if (const int rc = retire_mark_scan<RetireCount, RetirePlus>(
            c, rows, n, M0,
            [&](const int32_t *d_list, int32_t *d_keep, int32_t *d_word, RetireCount *d_cnt) {
                hipLaunchKernelGGL(retire_mark_kernel, dim3(div_up(n, kRetireBlock)), block, 0, st, d_list, n, c->models.as<mmp_model_row>(),
                                   (flags & MMP_RETIRE_EMPTY_ONLY) ? 1 : 0, d_keep, d_word);
                if (carry)
                    hipLaunchKernelGGL(ckey_retire_check_kernel, dim3(div_up(c->k_slots, kRetireBlock)), block, 0, st, kstore, c->k_caches, c->k_slots,
                                       M0, d_keep, d_live_key);
                hipLaunchKernelGGL(retire_flags_kernel, dim3(div_up(M0 + 1, kRetireBlock)), block, 0, st, M0, d_keep, c->models.as<mmp_model_row>(),
                                   old_off, d_cnt);
            },
            K, d_live_key))
        return rc;
    if (K.refused != INT32_MAX)
        return fail(c, MMP_EINVAL, "%s: row %d is not empty (registered again since its deletion?); nothing was retired", fn, K.refused);
    if (K.extra != INT32_MAX)
        return fail(c, MMP_EINVAL, "%s: row %d is the key of a live cache entry (remove the entry first); nothing was retired", fn, K.extra);
    const int32_t M1 = K.tot.row, B1 = K.tot.bytes, E1 = K.tot.ents;
    // build: the compacted registry, and with loaded ids their arena and table
    std::vector<int32_t> remap((size_t)M0);
    ScopedDevBuf nm, np, nt, nb, no;
    HashTabW next{};
    const size_t ecap = (size_t)std::max<int64_t>((int64_t)E1 + E1 / 2, 1024);
    if (nm.b.ensure((size_t)std::max(M1, 1) * sizeof(mmp_model_row)) != hipSuccess || np.b.ensure(ecap * 4) != hipSuccess ||
        nt.b.ensure(ecap * 8) != hipSuccess)
        return fail(c, MMP_ENOMEM, "%s: out of device memory", fn);
    if (ids)
        if (const int rc = retire_id_table_room(c, fn, T, M1, B1, nb, no, next)) return rc;
    const RetireMove A{c->models.as<mmp_model_row>(), c->ent_pod.as<int32_t>(), c->ent_time.as<int64_t>(), ids ? T.bytes.as<char>() : nullptr,
                       old_off, nm.b.as<mmp_model_row>(), np.b.as<int32_t>(), nt.b.as<int64_t>(), nb.b.as<char>(), no.b.as<int32_t>()};
    int32_t *d_remap = c->ret_remap.as<int32_t>();
    const int rc = retire_build(c, fn, M0, K.ms, [&] {
        hipLaunchKernelGGL(retire_move_kernel, dim3(div_up(M0, kRetireBlock)), block, 0, st, M0, c->ret_keep.as<int32_t>(), c->me_pos.as<RetireCount>(), A,
                           d_remap);
        if (ids) retire_id_table(c, T, d_remap, next, nb, no, c->ret_word.as<int32_t>() + 1);
    }, remap);
    if (rc != MMP_OK) return rc;
    // nothing fails from here on but the drain and the re-resolution: registry, arena, table and counts change together
    {
        std::lock_guard<std::shared_mutex> g(c->mu);
        HIP_TRY(c, quiesce_decisions(c));  // kernels that captured the old tables; the resolved view is rewritten in place
        nm.move_into(c->models);
        np.move_into(c->ent_pod);
        nt.move_into(c->ent_time);
        c->n_models = M1;
        c->n_entries = E1;
        c->ent_live = E1;
        c->m_cnt.resize(M0, 0);
        for (int32_t r = 0; r < M0; r++)  // (remap[r] <= r: in place)
            if (remap[r] >= 0) c->m_cnt[remap[r]] = c->m_cnt[r];
        c->m_cnt.resize(M1);
        c->u_stamp.assign(std::min<size_t>(c->u_stamp.size(), (size_t)M1), 0);  // (stamps name a call generation: zero = none)
        c->plan.model_map_n = std::min(c->plan.model_map_n, M1);
        if (ids) retire_id_table_publish(T, next, nb, no, M1, B1);
        // (the drain above ran inside this exclusive hold, so no decision and no request call by model id holds what the swap
        // retired: it goes here, before rebuild_resolved allocates)
        for (ScopedDevBuf *b : {&nm, &np, &nt, &nb, &no}) b->release();
        c->side[0].rmodels_ok = c->side[1].rmodels_ok = false;
        split_reset(c);
        if (carry) {  // the keys of the bound caches follow their rows, in place (d_remap: the M0 words retire_move_kernel wrote)
            hipLaunchKernelGGL(ckey_retire_remap_kernel, dim3(div_up(c->k_slots, kRetireBlock)), block, 0, st, kstore, c->k_caches, c->k_slots, M0,
                               d_remap);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipStreamSynchronize(st));
        }
        if (const int rr = rebuild_resolved(c)) return rr;
    }
    if (remap_out) memcpy(remap_out, remap.data(), (size_t)M0 * 4);
    if (n_models_after_out) *n_models_after_out = M1;
    return MMP_OK;
} MMP_CATCH(c, "mmp_models_retire")

int mmp_pods_retire(mmp_ctx *c, const int32_t *pods, int32_t n, uint32_t flags, int32_t *remap_out, int32_t max_pods,
                    int32_t *n_pods_after_out, int64_t *n_entries_unresolved_out)
try {
    if (!c || n < 0 || (n > 0 && !pods) || (flags & ~(MMP_PODS_RETIRE_GONE_ONLY | MMP_PODS_RETIRE_UNREFERENCED)) || max_pods < 0)
        return fail(c, MMP_EINVAL, "mmp_pods_retire: bad argument");
    // The retire frame (at retire_list_guard).  Its own: the remap made on the host, one round trip, the hold kept across the commit.
    std::lock_guard<std::mutex> gb(c->batch_mu);
    if (c->n_shards > 0) return fail(c, MMP_ESTATE, "mmp_pods_retire: not available on a pod-axis shard context");
    const int32_t P0 = (int32_t)c->pods.size();
    const bool ids = c->have_ids;
    if (ids)
        if (const int rc = id_space_guard(c, "mmp_pods_retire")) return rc;
    // Type rows loaded for another word count are stale, and a commit refuses them.  They must stay refused: squeezing is impossible
    // (their bits belong to no numbering of these rows) and leaving them would let the check pass once P crosses the word edge back.
    if (c->n_types > 0 && c->types_w != div_up(P0, 64))
        return fail(c, MMP_ESTATE, "mmp_pods_retire: the type bitmaps were loaded for a different pod count (%d words for %d pods); reload them first",
                    c->types_w, P0);
    if (const int rc = retire_list_guard(c, "mmp_pods_retire", RetireNoun{"pods", "instance", "the table"}, pods, n, P0, remap_out, max_pods))
        return rc;
    if (n == 0) {
        if (n_entries_unresolved_out) *n_entries_unresolved_out = 0;
        return retire_nothing(c, P0, remap_out, n_pods_after_out);
    }
    // 1. the remap, on the host: P0 words from the caller's list
    std::vector<int32_t> remap((size_t)P0, 0);
    for (int32_t i = 0; i < n; i++) remap[pods[i]] = -1;
    int32_t P1 = 0;
    for (int32_t p = 0; p < P0; p++) {
        if (remap[p] == 0) {
            remap[p] = P1++;
            continue;
        }
        if ((flags & MMP_PODS_RETIRE_GONE_ONLY) && ((c->pods[p].flags & MMP_POD_LIVE) || !(c->pods[p].flags & MMP_POD_TOMBSTONE)))
            return fail(c, MMP_EINVAL, "mmp_pods_retire: instance %d is not a tombstone (its id came back since the deletion?); nothing was retired", p);
    }
    // 2. what the device holds by instance index, beside the published state: the entry arena's pods, the marks, the id table
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    const int32_t M = c->n_models, E = c->n_entries, miss0 = std::min(c->miss_n, P0);
    int32_t miss1 = 0;
    for (int32_t p = 0; p < miss0; p++) miss1 += remap[p] >= 0;
    HIP_TRY(c, c->ret_remap.ensure((size_t)P0 * 4));
    HIP_TRY(c, c->ret_word.ensure(sizeof(PodsRetireWords)));
    const int32_t *d_remap = c->ret_remap.as<int32_t>();
    PodsRetireWords *d_words = c->ret_word.as<PodsRetireWords>();
    PodsRetireWords words{0ull, INT32_MAX, INT32_MAX};
    ScopedDevBuf np, nmiss;  // the new arena and marks, after the swap the old ones (marks with no survivor stay: miss_n says so)
    const uint32_t cap0 = ids ? c->idtab_mask + 1 : 0u;
    HashTabW next{};
    bool room = (!c->ent_pod.p || np.b.ensure(c->ent_pod.cap) == hipSuccess) && (miss1 == 0 || nmiss.b.ensure((size_t)miss1 * 8) == hipSuccess);
    if (room && ids) room = next_table_room(c, 0, P1, c->idtab_next_hash, c->idtab_next_val, next) == MMP_OK;  // tab_capacity(P1): the table shrinks
    if (!room) return fail(c, MMP_ENOMEM, "mmp_pods_retire: out of device memory");
    const dim3 block(kRetireBlock);
    hipError_t e = hipMemcpyAsync(c->ret_remap.p, remap.data(), (size_t)P0 * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_words, &words, sizeof words, hipMemcpyHostToDevice, st);
    int rc = MMP_OK;
    KT_BEGIN(c, st);
    if (e == hipSuccess) {
        if (E > 0)
            hipLaunchKernelGGL(pods_retire_entries_kernel, dim3(div_up(E, kRetireBlock)), block, 0, st, c->ent_pod.as<int32_t>(), E, d_remap, P0,
                               np.b.as<int32_t>());
        if (M > 0)
            hipLaunchKernelGGL(pods_retire_count_kernel, dim3(div_up(M, kRetireBlock)), block, 0, st, c->models.as<mmp_model_row>(), M,
                               c->ent_pod.as<int32_t>(), d_remap, P0, d_words);
        if (miss0 > 0 && miss1 > 0)
            hipLaunchKernelGGL(pods_retire_marks_kernel, dim3(div_up(miss0, kRetireBlock)), block, 0, st, c->miss_since.as<int64_t>(), miss0,
                               d_remap, nmiss.b.as<int64_t>());
        if (ids && (rc = empty_table(c, next)) == MMP_OK) {  // the frame's claims; the verify is this call's own (the ids are on the host)
            retire_table_claim(c, c->idtab_hash, c->idtab_val, cap0, d_remap, next);
            hipLaunchKernelGGL(pods_retire_verify_kernel, dim3(div_up((int)cap0, kRetireBlock)), block, 0, st, c->idtab_hash.as<uint64_t>(),
                               c->idtab_val.as<int32_t>(), cap0, d_remap, P0, HashTab{next.hash, next.val, next.mask}, d_words);
        }
    }
    KT_END(c, st);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&words, d_words, sizeof words, hipMemcpyDeviceToHost, st);
    const hipError_t se = hipStreamSynchronize(st);  // (whatever was enqueued has finished before the new buffers may go)
    if (e == hipSuccess) e = se;
    if (rc == MMP_OK && e != hipSuccess) rc = fail(c, MMP_EHIP, "mmp_pods_retire: %s", hipGetErrorString(e));
    if (rc == MMP_OK && (flags & MMP_PODS_RETIRE_UNREFERENCED) && words.n_turned > 0)
        rc = fail(c, MMP_EINVAL, "mmp_pods_retire: instance %d is still named by a registry entry (prune the registry first); nothing was retired",
                  words.lowest_named);
    if (rc == MMP_OK && words.lost != INT32_MAX)
        rc = fail(c, MMP_EHIP, "mmp_pods_retire: the id of new instance %d was not found in the compacted table", words.lost);
    if (rc != MMP_OK) return rc;
    kt_collect(c);
    const double build_ms = c->last_kernel_ms;
    // 3. what the host holds by instance index: rows, labels, type bit rows, the id store
    struct HostSide {
        std::vector<mmp_pod_row> pods;
        std::vector<uint64_t> label_word, allowed, prefer;
        std::vector<int32_t> label_count, id_offs, id_sorted, replica_set_v, dirty;
        std::vector<uint32_t> id_order_v;
        std::string id_bytes;
        int32_t types_w = 0;
    } H;
    H.pods.resize((size_t)P1);
    H.label_word.assign((size_t)P1, 0);
    H.label_count.assign((size_t)P1, 0);
    const bool labels = c->pod_label_word.size() == (size_t)P0 && c->pod_label_count.size() == (size_t)P0;
    for (int32_t p = 0; p < P0; p++) {
        const int32_t q = remap[p];
        if (q < 0) continue;
        H.pods[q] = c->pods[p];
        if (labels) H.label_word[q] = c->pod_label_word[p], H.label_count[q] = c->pod_label_count[p];
    }
    if (ids) {
        // the ranks of the survivors among the surviving ids: id_sorted filtered, not sorted again
        H.id_offs.assign(1, 0);
        H.id_order_v.assign((size_t)P1, 0);
        H.replica_set_v.assign((size_t)P1, -1);
        for (int32_t p = 0; p < P0; p++) {
            if (remap[p] < 0) continue;
            H.id_bytes.append(c->id_bytes, (size_t)c->id_offs[p], (size_t)(c->id_offs[p + 1] - c->id_offs[p]));
            H.id_offs.push_back((int32_t)H.id_bytes.size());
            H.replica_set_v[remap[p]] = c->replica_set_v[p];
        }
        H.id_sorted.reserve((size_t)P1);
        for (const int32_t p : c->id_sorted)
            if (remap[p] >= 0) {
                H.id_order_v[remap[p]] = (uint32_t)H.id_sorted.size();
                H.id_sorted.push_back(remap[p]);
            }
        for (int32_t q = 0; q < P1; q++) H.pods[q].id_order = H.id_order_v[q];
    }
    const bool types = c->n_types > 0;  // (they cover P0: checked on the way in)
    if (types) {
        const int32_t W0 = c->types_w, W1 = div_up(P1, 64);
        H.types_w = W1;
        H.allowed.assign((size_t)c->n_types * W1, 0);
        H.prefer.assign((size_t)c->n_types * W1, 0);
        for (int32_t t = 0; t < c->n_types; t++) {
            const uint64_t *a0 = c->allowed.data() + (size_t)t * W0, *f0 = c->prefer.data() + (size_t)t * W0;
            uint64_t *a1 = H.allowed.data() + (size_t)t * W1, *f1 = H.prefer.data() + (size_t)t * W1;
            for (int32_t p = 0; p < P0; p++) {
                const int32_t q = remap[p];
                if (q < 0) continue;
                a1[q >> 6] |= ((a0[p >> 6] >> (p & 63)) & 1ull) << (q & 63);
                f1[q >> 6] |= ((f0[p >> 6] >> (p & 63)) & 1ull) << (q & 63);
            }
        }
    }
    // 4. the swap and the commit, under the state lock: a decision sees the whole old index space or the whole new one
    {
        std::lock_guard<std::shared_mutex> g(c->mu);
        HIP_TRY(c, quiesce_decisions(c));
        const bool dirty_all0 = c->dirty_all;
        const int32_t miss_n0 = c->miss_n;
        const uint32_t mask0 = c->idtab_mask;
        const auto swap_inputs = [&] {  // (its own inverse)
            c->pods.swap(H.pods);
            c->pod_label_word.swap(H.label_word);
            c->pod_label_count.swap(H.label_count);
            c->dirty.swap(H.dirty);
            if (types) {
                c->allowed.swap(H.allowed);
                c->prefer.swap(H.prefer);
                std::swap(c->types_w, H.types_w);
                c->types_gen++;  // (never back to a generation a device copy may carry)
                c->sig_valid = false;
            }
            if (ids) {
                c->id_bytes.swap(H.id_bytes);
                c->id_gen++;
                c->id_offs.swap(H.id_offs);
                c->id_sorted.swap(H.id_sorted);
                c->id_order_v.swap(H.id_order_v);
                c->replica_set_v.swap(H.replica_set_v);
                std::swap(c->idtab_hash, c->idtab_next_hash);
                std::swap(c->idtab_val, c->idtab_next_val);
            }
            np.move_into(c->ent_pod);
            nmiss.move_into(c->miss_since);
        };
        swap_inputs();
        c->idtab_mask = ids ? next.mask : mask0;
        c->miss_n = miss1;
        c->dirty_all = true;
        const bool commit = c->committed;
        try {
            if (commit) rc = commit_staged(c, true);
        } catch (const std::exception &ex) {
            rc = fail(c, MMP_ENOMEM, "mmp_pods_retire: %s in the commit stage", ex.what());
        }
        if (rc != MMP_OK) {  // nothing was published: the old inputs go back
            (void)hipStreamSynchronize(st);
            swap_inputs();
            c->idtab_mask = mask0;
            c->miss_n = miss_n0;
            c->dirty_all = dirty_all0;
            return rc;
        }
        if (commit) kt_add(c, build_ms);  // the call's device span: remap + count + marks + table + verify, and the commit's
    }
    // (the old arena and marks go with np / nmiss, after the hold: the drain ran inside it)
    if (remap_out) memcpy(remap_out, remap.data(), (size_t)P0 * 4);
    if (n_pods_after_out) *n_pods_after_out = P1;
    if (n_entries_unresolved_out) *n_entries_unresolved_out = (int64_t)words.n_turned;
    return MMP_OK;
} MMP_CATCH(c, "mmp_pods_retire")

int mmp_pods_get(mmp_ctx *c, mmp_pod_row *rows_out, int32_t max_rows, int32_t *n_out)
try {
    if (!c || !n_out || max_rows < 0 || (max_rows > 0 && !rows_out)) return fail(c, MMP_EINVAL, "mmp_pods_get: bad argument");
    std::lock_guard<std::shared_mutex> g(c->mu);
    *n_out = (int32_t)c->pods.size();
    const int32_t m = std::min(*n_out, max_rows);
    if (m > 0) memcpy(rows_out, c->pods.data(), (size_t)m * sizeof(mmp_pod_row));
    return MMP_OK;
} MMP_CATCH(c, "mmp_pods_get")

int mmp_models_get(mmp_ctx *c, mmp_model_row *rows_out, int32_t max_models, int32_t *ent_pod_out, int64_t *ent_time_out,
                   int32_t max_entries, int32_t *n_models_out, int32_t *n_entries_out)
try {
    if (!c || !n_models_out || !n_entries_out || max_models < 0 || max_entries < 0)
        return fail(c, MMP_EINVAL, "mmp_models_get: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *n_models_out = c->n_models;
    *n_entries_out = c->n_entries;
    const int32_t m = std::min(c->n_models, max_models), e = std::min(c->n_entries, max_entries);
    if (m > 0 && rows_out) HIP_TRY(c, copy_sync(c, rows_out, c->models.p, (size_t)m * sizeof(mmp_model_row), hipMemcpyDeviceToHost));
    if (e > 0 && ent_pod_out) HIP_TRY(c, copy_sync(c, ent_pod_out, c->ent_pod.p, (size_t)e * 4, hipMemcpyDeviceToHost));
    if (e > 0 && ent_time_out) HIP_TRY(c, copy_sync(c, ent_time_out, c->ent_time.p, (size_t)e * 8, hipMemcpyDeviceToHost));
    return MMP_OK;
} MMP_CATCH(c, "mmp_models_get")

/* ---- pod-axis sharding --------------------------------- */

int mmp_shard_configure(mmp_ctx *c, int32_t shard, int32_t n_shards)
try {
    if (!c || n_shards < 1 || n_shards > kMaxShards || shard < 0 || shard >= n_shards)
        return fail(c, MMP_EINVAL, "mmp_shard_configure: need 0 <= shard < n_shards <= %d", kMaxShards);
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    c->shard = shard;
    c->n_shards = n_shards;
    c->committed = false;
    c->rank_pending = false;
    return MMP_OK;
} MMP_CATCH(c, "mmp_shard_configure")

int32_t mmp_shard_xchg_slots(int32_t phase, int32_t n_shards)
{
    switch (phase) {
    case 1: return kX1;
    case 2: return kX2;
    case 3: return kX3;
    case 4: return kX4;
    case 5: return x5_slots(n_shards);
    case 6: return kX6;
    default: return 0;
    }
}

int32_t mmp_shard_xchg_is_sum(int32_t phase) { return phase == 5 ? 1 : 0; }

int mmp_shard_rank_dev(mmp_ctx *c, void *d_rank)
try {
    if (!c || !d_rank) return fail(c, MMP_EINVAL, "mmp_shard_rank_dev: null argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    if (c->n_shards < 1) return fail(c, MMP_ESTATE, "mmp_shard_configure has not been called");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const int32_t P = (int32_t)c->pods.size();
    if (P >= kShardMaxPods)
        return fail(c, MMP_EINVAL, "pod-axis mode: %d instances exceed the %d the exchange words can carry", P, kShardMaxPods - 1);
    SnapBufs &B = c->sb[1 - c->cur];
    hipStream_t st = c->stream;
    HIP_TRY(c, B.pods.ensure(std::max<size_t>(P, 1) * sizeof(mmp_pod_row)));
    if (P) {
        HIP_TRY(c, hipMemcpyAsync(B.pods.p, c->pods.data(), (size_t)P * sizeof(mmp_pod_row), hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipMemsetAsync(d_rank, 0, (size_t)P * 4, st));
        const int per = div_up(P, c->n_shards);
        const int p_lo = std::min(P, c->shard * per), p_hi = std::min(P, p_lo + per);
        if (p_hi > p_lo) {
            // the slice against all rows is (P / shards) x P comparator calls; from where an unsharded commit sorts (8192^2 pairs)
            // sorting the whole table is cheaper — when the comparator is a total order on it (snapshot.hpp "ranking by sorting")
            const bool want_sort = c->tune.rank_mode == 2 || c->tune.rank_mode == 3 || (c->tune.rank_mode == 0 && (int64_t)(p_hi - p_lo) * P >= (int64_t)kRankSortMinPods * kRankSortMinPods);
            const bool sort_legal = check_placement_order(c->pods, c->cfg.min_space_units, churn2_of(c)).sort_legal;
            if (const int rc = launch_rank(c, B.pods.as<mmp_pod_row>(), P, p_lo, p_hi, true, want_sort, sort_legal, static_cast<int32_t *>(d_rank), st))
                return rc;
            HIP_TRY(c, hipGetLastError());
        }
    }
    HIP_TRY(c, hipStreamSynchronize(st));
    c->rank_pending = true;
    return MMP_OK;
} MMP_CATCH(c, "mmp_shard_rank_dev")

int mmp_shard_commit_dev(mmp_ctx *c, const void *d_rank)
try {
    if (!c || !d_rank) return fail(c, MMP_EINVAL, "mmp_shard_commit_dev: null argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    if (c->n_shards < 1 || !c->rank_pending) return fail(c, MMP_ESTATE, "mmp_shard_commit_dev: call mmp_shard_rank_dev first");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, quiesce_decisions(c));

    // sizes: the table's, and the slice of its words this shard owns
    const int32_t P = (int32_t)c->pods.size();
    const int32_t W = std::max(div_up(P, 64), 1);
    const int32_t Wfull = div_up(P, 64);
    const int32_t T = std::max(c->n_types, 1);
    if (c->n_types > 0 && c->types_w != Wfull)
        return fail(c, MMP_ESTATE, "type bitmaps were loaded for a different pod count; reload them before commit");
    const int32_t Wl = div_up(W, c->n_shards);
    const int32_t w_lo = std::min(W, c->shard * Wl);
    const int32_t Wn = std::min(W, w_lo + Wl) - w_lo;
    const int32_t Wn1 = std::max(Wn, 1);
    const int32_t P_local = std::max(0, std::min(P - w_lo * 64, Wn * 64));
    const size_t padded = (size_t)Wn1 * 64, padded_full = (size_t)W * 64;
    const int64_t min_space = c->cfg.min_space_units;
    const int32_t n_rs = (int32_t)c->replaced_rs.size();
    SnapBufs &B = c->sb[1 - c->cur];  // B.pods was filled by mmp_shard_rank_dev
    SnapSide &N = c->side[1 - c->cur];
    hipStream_t st = c->stream;
    if (const int rc = ensure_columns(c, B, T, Wn1, W)) return rc;
    if (const int rc = ensure_commit_scratch(c, N, T, W)) return rc;

    // uploads, with the scratch and the slice's columns cleared
    {
        ZeroBatch zb(st);
        zb.add(c->occupancy.p, padded_full * 4);
        zb.add(c->flag.p, sizeof(int32_t));
        zb.add(B.lru.p, padded * 8);
        zb.add(B.rem.p, padded * 8);
        zb.add(B.cnt.p, padded * 4);
        zb.add(B.rpm.p, padded * 4);
        zb.add(B.orig.p, padded * 4);
        zb.add(B.pos_of.p, padded_full * 4);
        zb.add(B.elig.p, (size_t)T * Wn1 * 8);
        zb.add(B.elig_nors.p, (size_t)T * Wn1 * 8);
        zb.add(B.pref.p, (size_t)T * Wn1 * 8);
        zb.add(B.fullw.p, (size_t)Wn1 * 8);
        zb.add(B.ge.p, (size_t)kGeRows * Wn1 * 8);
        zb.launch(st);
        HIP_TRY(c, hipGetLastError());
    }
    InputStage in;
    if (const int rc = upload_commit_inputs(c, B, N, T, true, in, st)) return rc;
    B.types_gen = N.types_gen = c->d_prefer_gen = 0;  // (uploaded unconditionally here; "unknown" makes an ordinary commit upload again)

    if (P > 0) {
        // scatter by the all-reduced ranks, then the slice's bitmaps and the cluster stats, a launch each
        hipLaunchKernelGGL(scatter_shard_kernel, dim3(div_up(P, 256)), dim3(256), 0, st, B.pods.as<mmp_pod_row>(), P,
                           static_cast<const int32_t *>(d_rank), c->occupancy.as<int32_t>(), w_lo * 64, (w_lo + Wn) * 64,
                           B.lru.as<int64_t>(), B.rem.as<int64_t>(), B.cnt.as<int32_t>(), B.rpm.as<int32_t>(),
                           B.orig.as<int32_t>(), B.pos_of.as<int32_t>(), c->flag.as<int32_t>());
        launch_mark_replaced(c, B, P, st);
        if (Wn > 0)
            hipLaunchKernelGGL(build_masks_shard_kernel, dim3(div_up(T * Wn, 4)), dim3(256), 0, st, B.pods.as<mmp_pod_row>(),
                               P, Wfull, w_lo, Wn, T, min_space, B.orig.as<int32_t>(), N.d_allowed.as<uint64_t>(),
                               N.d_has_allowed.as<uint8_t>(), c->d_prefer.as<uint64_t>(), B.has_pref.as<uint8_t>(),
                               n_rs ? c->rs_bad.as<uint8_t>() : nullptr, B.elig.as<uint64_t>(),
                               B.elig_nors.as<uint64_t>(), B.pref.as<uint64_t>(), B.fullw.as<uint64_t>());
        if (Wn > 0)  // the count-threshold bitmaps of the slice (the lane path's count break)
            hipLaunchKernelGGL(build_ge_kernel, dim3(div_up(kGeRows * Wn, 4)), dim3(256), 0, st, B.cnt.as<int32_t>(), P_local, Wn,
                               B.ge.as<uint64_t>());
        hipLaunchKernelGGL(cluster_stats_kernel, dim3(std::min(div_up(P, 256), 512)), dim3(256), 0, st,
                           B.pods.as<mmp_pod_row>(), P, min_space, N.stats_acc.as<StatsAcc>());
        HIP_TRY(c, hipGetLastError());
    }
    // subset stats, in one go
    if (const int rc = stage_partitions(c, N, P, st)) return rc;
    if (const int rc = launch_subset_stats(c, N, B.pods.as<mmp_pod_row>(), P, min_space, st)) return rc;
    if (const int rc = fetch_subset_stats(c, N, st)) return rc;
    int32_t bad = 0;
    StatsAcc acc{};
    if (const int rc = fetch_commit_result(c, N, &bad, &acc, st)) return rc;
    HIP_TRY(c, hipStreamSynchronize(st));
    c->rank_pending = false;
    if (bad)
        return fail(c, MMP_EORDER, "PLACEMENT_ORDER is not a total order on these rows; snapshot not published");

    ShardSnap S = snap_columns<ShardSnap>(B, P, W, T, n_rs > 0, min_space);
    S.shard = c->shard;
    S.n_shards = c->n_shards;
    S.Wl = Wl;
    S.w_lo = w_lo;
    S.Wn = Wn;
    c->ssnap = S;
    Snap V = snap_columns<Snap>(B, P_local, Wn, T, n_rs > 0, min_space);  // the slice as the lane-per-decision path sees it: local positions, global pos_of
    V.ge = B.ge.as<uint64_t>();
    V.pos_base = w_lo * 64;
    V.w_base = w_lo;
    V.more_after = (w_lo + Wn) * 64 < P ? 1 : 0;
    Snap M{};  // what the non-placement entry points read in shard mode: the sizes and pos_of alone
    M.P = P;
    M.W = W;
    M.T = T;
    M.any_rs = S.any_rs;
    M.min_space = min_space;
    M.pos_of = S.pos_of;
    {
        // the slice's per-type head windows (place_kernel.hpp: TypeWin, built over the VIEW) and the registry's resolved rows
        // (global rank positions; resolve_req<true> translates them): what place_shard_fast_kernel decides from
        const size_t wins_bytes = (size_t)std::max(T, kWinLds) * sizeof(TypeWin);
        HIP_TRY(c, B.heads.ensure(wins_bytes));
        HIP_TRY(c, hipMemsetAsync(B.heads.p, 0, wins_bytes, st));
        if (V.P > 0 && V.W > 0) hipLaunchKernelGGL(build_wins_kernel, dim3(T), dim3(64), 0, st, V, B.heads.as<TypeWin>());
        HIP_TRY(c, hipGetLastError());
        if (const int rc = rebuild_resolved(c, N, M, true)) return rc;  // (synchronizes the stream)
    }
    // publish (c->mu has been held throughout)
    c->sview = V;
    c->snap = M;
    c->cur = 1 - c->cur;
    c->committed = true;
    publish_cluster_stats(c, acc);
    return MMP_OK;
} MMP_CATCH(c, "mmp_shard_commit_dev")

namespace {
// one phase of the general protocol on `st` (called with c->mu held); n_dev: see PlaceArgs::n_dev
int shard_phase_launch(mmp_ctx *c, int32_t phase, const void *d_reqs, int32_t n, const int32_t *n_dev, const void *d_extra,
                       int64_t now, void *const *d_xchg, void *d_outs, hipStream_t st)
{
    HIP_TRY(c, order_after_registry(c, st));
    PlaceArgs A = place_args(c, d_reqs, n, d_extra, now, d_outs, false, c->ssnap.P);
    A.n_dev = n_dev;
    XchgPtrs X{static_cast<int64_t *>(d_xchg[0]), static_cast<int64_t *>(d_xchg[1]), static_cast<int64_t *>(d_xchg[2]),
               static_cast<int64_t *>(d_xchg[3]), static_cast<int64_t *>(d_xchg[4]), static_cast<int64_t *>(d_xchg[5])};
    const ShardSnap &S = c->ssnap;
    const int wpad = (std::max(S.Wn, 1) + 1) & ~1;
    const size_t lds = (size_t)kPlaceWaves * 2 * wpad * sizeof(uint64_t);
    if (lds > 64 * 1024) return fail(c, MMP_EINVAL, "shard slice too large for the LDS staging tile (%d words)", S.Wn);
    const int blocks = std::min(div_up(n, kPlaceWaves), 256 * 8);
    const dim3 grid(blocks), block(kPlaceWaves * 64);
    switch (phase) {
    case 1: hipLaunchKernelGGL(place_shard_kernel<1>, grid, block, lds, st, S, A, X, wpad); break;
    case 2: hipLaunchKernelGGL(place_shard_kernel<2>, grid, block, lds, st, S, A, X, wpad); break;
    case 3: hipLaunchKernelGGL(place_shard_kernel<3>, grid, block, lds, st, S, A, X, wpad); break;
    case 4: hipLaunchKernelGGL(place_shard_kernel<4>, grid, block, lds, st, S, A, X, wpad); break;
    case 5: hipLaunchKernelGGL(place_shard_kernel<5>, grid, block, lds, st, S, A, X, wpad); break;
    case 6: hipLaunchKernelGGL(place_shard_kernel<6>, grid, block, lds, st, S, A, X, wpad); break;
    default: hipLaunchKernelGGL(place_shard_finish_kernel, dim3(div_up(n, 256)), dim3(256), 0, st, S, A, X); break;
    }
    HIP_TRY(c, hipGetLastError());
    return MMP_OK;
}
}  // namespace

int mmp_shard_place_phase_dev(mmp_ctx *c, int32_t phase, const void *d_reqs, int32_t n, const void *d_extra, int64_t now,
                              void *const *d_xchg, void *d_outs, void *stream)
try {
    if (!c || phase < 1 || phase > 7 || n < 0 || !d_xchg || (n > 0 && (!d_reqs || (phase == 7 && !d_outs))))
        return fail(c, MMP_EINVAL, "mmp_shard_place_phase_dev: bad argument");
    if (const int rc = refuse_per_thread_stream(c, stream, "mmp_shard_place_phase_dev")) return rc;
    for (int i = 0; i < 6; i++)
        if (n > 0 && !d_xchg[i]) return fail(c, MMP_EINVAL, "mmp_shard_place_phase_dev: exchange buffer %d is null", i + 1);
    std::shared_lock<std::shared_mutex> g(c->mu);  // capture the published shard snapshot + enqueue; no wait
    if (c->n_shards < 1 || !c->committed) return fail(c, MMP_ESTATE, "no committed shard snapshot");
    if (n == 0) return MMP_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    note_caller_stream(c, st);
    return shard_phase_launch(c, phase, d_reqs, n, nullptr, d_extra, now, d_xchg, d_outs, st);
} MMP_CATCH(c, "mmp_shard_place_phase_dev")

int32_t mmp_shard_fast_slots(void) { return kXF; }

namespace {
PlaceArgs shard_args(mmp_ctx *c, const void *d_reqs, int32_t n, const void *d_extra, int64_t now, void *d_outs)
{
    PlaceArgs A = place_args(c, d_reqs, n, d_extra, now, d_outs, true, c->ssnap.P);
    A.wins = c->sview.P <= 0 ? nullptr : c->sb[c->cur].heads.as<TypeWin>();
    return A;
}
}  // namespace

int mmp_shard_place_fast_dev(mmp_ctx *c, const void *d_reqs, int32_t n, const void *d_extra, int64_t now, void *d_xf,
                             void *stream)
try {
    if (!c || n < 0 || (n > 0 && (!d_reqs || !d_xf))) return fail(c, MMP_EINVAL, "mmp_shard_place_fast_dev: bad argument");
    if (const int rc = refuse_per_thread_stream(c, stream, "mmp_shard_place_fast_dev")) return rc;
    std::lock_guard<std::shared_mutex> g(c->mu);
    if (c->n_shards < 1 || !c->committed) return fail(c, MMP_ESTATE, "no committed shard snapshot");
    if (n == 0) return MMP_OK;
    const PlaceArgs A = shard_args(c, d_reqs, n, d_extra, now, nullptr);
    note_caller_stream(c, static_cast<hipStream_t>(stream));
    HIP_TRY(c, order_after_registry(c, static_cast<hipStream_t>(stream)));
    hipLaunchKernelGGL(place_shard_fast_kernel, dim3(div_up(n, kPlaceBlock)), dim3(kPlaceBlock), (size_t)place_lane_lds(c->sview.T),
                       static_cast<hipStream_t>(stream), c->sview, A, c->shard, static_cast<int64_t *>(d_xf));
    HIP_TRY(c, hipGetLastError());
    return MMP_OK;
} MMP_CATCH(c, "mmp_shard_place_fast_dev")

namespace {
// After the all-reduce: the decided rows are written, the rest flagged and COUNTED; the count reaches the host through a
// pinned word (place_shard_fast_finish_kernel).  Three steps so that a caller may leave between the first and the second
// (mmp_shard_place_batch_async_dev): enqueue the kernel; synchronise and read the count; only when it is not zero, flags ->
// exclusive scan -> gather of the undecided requests (decision order, identical on every shard).  Called with c->mu held.
int shard_finish_prepare(mmp_ctx *c, uint32_t slot, int32_t n, hipStream_t st, uint32_t *seq_out)
{
    HIP_TRY(c, c->f_flags[slot].ensure((size_t)(n + 1) * 4));
    if (!c->f_cnt[slot].p) {
        HIP_TRY(c, c->f_cnt[slot].ensure(16));
        HIP_TRY(c, hipMemsetAsync(c->f_cnt[slot].p, 0, 16, st));
    }
    if (!c->f_done) {
        HIP_TRY(c, hipHostMalloc(reinterpret_cast<void **>(&c->f_done), 128, kPinnedFlags));
        c->f_done[0] = c->f_done[8] = 0;
    }
    *seq_out = ++c->f_seq;
    return MMP_OK;
}
int shard_finish_enqueue(mmp_ctx *c, uint32_t slot, int32_t n, const void *d_xf, void *d_outs, hipStream_t st, uint32_t *seq_out)
{
    uint32_t seq = 0;
    const int prc = shard_finish_prepare(c, slot, n, st, &seq);
    if (prc != MMP_OK) return prc;
    hipLaunchKernelGGL(place_shard_fast_finish_kernel, dim3(div_up(n + 1, 256)), dim3(256), 0, st, static_cast<const int64_t *>(d_xf),
                       n, c->ssnap.any_rs, static_cast<mmp_place_out *>(d_outs), c->f_flags[slot].as<int32_t>(),
                       c->f_cnt[slot].as<unsigned long long>(), c->f_done + 8 * slot, seq);
    HIP_TRY(c, hipGetLastError());
    *seq_out = seq;
    return MMP_OK;
}
// The count arrives in pinned memory with the finish kernel's last workgroup: the host polls the word (no copy, and no wait for
// whatever a later batch has enqueued behind that kernel); a word that stays away for 2 ms is waited for with the stream.
// Everything the host does with the count afterwards is enqueued on the same stream, i.e. ordered behind the kernel.
int shard_finish_collect(mmp_ctx *c, uint32_t slot, hipStream_t st, uint32_t seq, int32_t *n_rest_out)
{
    const uint64_t *w = c->f_done + 8 * slot;
    uint64_t word = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spins = 0;; spins++) {
        word = __atomic_load_n(w, __ATOMIC_ACQUIRE);
        if ((uint32_t)(word >> 32) == seq) break;
        if ((spins & 255) == 255 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) {
            HIP_TRY(c, hipStreamSynchronize(st));
            word = __atomic_load_n(w, __ATOMIC_ACQUIRE);
            if ((uint32_t)(word >> 32) != seq) return fail(c, MMP_EHIP, "shard finish kernel did not report its count");
            break;
        }
        __builtin_ia32_pause();
    }
    *n_rest_out = (int32_t)(uint32_t)word;
    return MMP_OK;
}
int shard_rest_gather(mmp_ctx *c, uint32_t slot, const void *d_reqs, int32_t n, int32_t n_rest, hipStream_t st)
{
    HIP_TRY(c, c->f_offs.ensure((size_t)(n + 1) * 4));
    HIP_TRY(c, c->f_idx.ensure((size_t)n_rest * 4));
    HIP_TRY(c, c->f_reqs.ensure((size_t)n_rest * sizeof(mmp_place_req)));
    HIP_TRY(c, c->f_outs.ensure((size_t)n_rest * sizeof(mmp_place_out)));
    const int32_t *flags = c->f_flags[slot].as<int32_t>();
    size_t scan_bytes = 0;
    HIP_TRY(c, rocprim::exclusive_scan(nullptr, scan_bytes, flags, c->f_offs.as<int32_t>(), (int32_t)0, (size_t)n + 1, rocprim::plus<int32_t>(), st));
    HIP_TRY(c, c->f_scan_tmp.ensure(std::max<size_t>(scan_bytes, 16)));
    HIP_TRY(c, rocprim::exclusive_scan(c->f_scan_tmp.p, scan_bytes, flags, c->f_offs.as<int32_t>(), (int32_t)0, (size_t)n + 1,
                                       rocprim::plus<int32_t>(), st));
    hipLaunchKernelGGL(place_shard_gather_kernel, dim3(div_up(n, 256)), dim3(256), 0, st, static_cast<const mmp_place_req *>(d_reqs),
                       n, flags, c->f_offs.as<int32_t>(), c->f_reqs.as<mmp_place_req>(), c->f_idx.as<int32_t>());
    HIP_TRY(c, hipGetLastError());
    return MMP_OK;
}
int shard_finish_launch(mmp_ctx *c, const void *d_reqs, int32_t n, const void *d_xf, void *d_outs, hipStream_t st, int32_t *n_rest_out)
{
    uint32_t seq = 0;  // (the step-wise calls: one batch at a time, slot 0; the caller reads d_outs next: synchronise)
    int rc = shard_finish_enqueue(c, 0, n, d_xf, d_outs, st, &seq);
    if (rc == MMP_OK) rc = shard_finish_collect(c, 0, st, seq, n_rest_out);
    if (rc == MMP_OK && *n_rest_out > 0) rc = shard_rest_gather(c, 0, d_reqs, n, *n_rest_out, st);
    if (rc == MMP_OK) HIP_TRY(c, hipStreamSynchronize(st));
    return rc;
}
}  // namespace

int mmp_shard_place_fast_finish_dev(mmp_ctx *c, const void *d_reqs, int32_t n, const void *d_xf, void *d_outs, void *stream,
                                    int32_t *n_rest_out, void **d_rest_reqs_out, void **d_rest_outs_out)
try {
    if (!c || n < 0 || !n_rest_out || !d_rest_reqs_out || !d_rest_outs_out || (n > 0 && (!d_reqs || !d_xf || !d_outs)))
        return fail(c, MMP_EINVAL, "mmp_shard_place_fast_finish_dev: bad argument");
    if (const int rc = refuse_per_thread_stream(c, stream, "mmp_shard_place_fast_finish_dev")) return rc;
    *n_rest_out = 0;
    *d_rest_reqs_out = *d_rest_outs_out = nullptr;
    std::lock_guard<std::shared_mutex> g(c->mu);
    if (c->n_shards < 1 || !c->committed) return fail(c, MMP_ESTATE, "no committed shard snapshot");
    // the step-wise calls use count slot 0 and the context's rest buffers, which an asynchronous batch still in flight may own
    if (c->pend.active) return fail(c, MMP_ESTATE, "mmp_shard_place_fast_finish_dev: an asynchronous batch is pending (mmp_shard_wait first)");
    if (n == 0) return MMP_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    note_caller_stream(c, st);
    int32_t n_rest = 0;
    {
        const int rc = shard_finish_launch(c, d_reqs, n, d_xf, d_outs, st, &n_rest);
        if (rc != MMP_OK) return rc;
    }
    *n_rest_out = n_rest;
    if (n_rest) {
        *d_rest_reqs_out = c->f_reqs.p;
        *d_rest_outs_out = c->f_outs.p;
    }
    return MMP_OK;
} MMP_CATCH(c, "mmp_shard_place_fast_finish_dev")

int mmp_shard_place_fast_scatter_dev(mmp_ctx *c, int32_t n_rest, void *d_outs, void *stream)
try {
    if (!c || n_rest < 0 || (n_rest > 0 && !d_outs)) return fail(c, MMP_EINVAL, "mmp_shard_place_fast_scatter_dev: bad argument");
    if (const int rc = refuse_per_thread_stream(c, stream, "mmp_shard_place_fast_scatter_dev")) return rc;
    std::lock_guard<std::shared_mutex> g(c->mu);
    if (c->n_shards < 1 || !c->committed) return fail(c, MMP_ESTATE, "no committed shard snapshot");
    if (n_rest == 0) return MMP_OK;
    hipLaunchKernelGGL(place_shard_scatter_kernel, dim3(div_up(n_rest, 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       c->f_outs.as<mmp_place_out>(), c->f_idx.as<int32_t>(), n_rest, static_cast<mmp_place_out *>(d_outs));
    HIP_TRY(c, hipGetLastError());
    return MMP_OK;
} MMP_CATCH(c, "mmp_shard_place_fast_scatter_dev")

/* ---- RCCL inside the boundary: the pod-axis group ------------------------- */
namespace {
// librccl is bound at run time: a host without RCCL (or a CPU-only test box) still loads libmmplace, and a process
// that already carries a copy (PyTorch bundles one) reuses it instead of mapping a second one.
struct RcclApi {
    void *h = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    std::string why;
};
// why_out: receives the reason when the call returns null (copied out under the binding's lock).
// MMP_RCCL_PATH=<file> names the one library to bind (a host with its own RCCL build; also how the tests reach the
// "no RCCL on this host" answer on a box that has one).
RcclApi *rccl_api(std::string *why_out = nullptr)
{
    static std::mutex mu;
    static RcclApi api;
    std::lock_guard<std::mutex> g(mu);
    if (api.h) return &api;
    struct Why {  // the reason leaves with every null return, whichever one it is
        RcclApi &a;
        std::string *out;
        ~Why() { if (out && !a.h) *out = a.why; }
    } why_guard{api, why_out};
    const char *only = getenv("MMP_RCCL_PATH");
    if (only && *only) {
        api.h = dlopen(only, RTLD_NOW | RTLD_LOCAL);
    } else {
        const char *names[] = {"librccl.so.1", "librccl.so"};
        for (int pass = 0; pass < 2 && !api.h; pass++)
            for (const char *nm : names) {
                api.h = dlopen(nm, RTLD_NOW | RTLD_LOCAL | (pass == 0 ? RTLD_NOLOAD : 0));
                if (api.h) break;
            }
        if (!api.h) api.h = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_LOCAL);
    }
    if (!api.h) {
        const char *e = dlerror();  // ONE call: dlerror() clears the message it returns
        api.why = e ? e : "librccl.so not found";
        return nullptr;
    }
    api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(dlsym(api.h, "ncclGetUniqueId"));
    api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(dlsym(api.h, "ncclCommInitRank"));
    api.AllReduce = reinterpret_cast<decltype(api.AllReduce)>(dlsym(api.h, "ncclAllReduce"));
    api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(dlsym(api.h, "ncclCommDestroy"));
    api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(dlsym(api.h, "ncclGetErrorString"));
    if (!api.GetUniqueId || !api.CommInitRank || !api.AllReduce || !api.CommDestroy) {
        api.why = "librccl.so lacks ncclGetUniqueId / ncclCommInitRank / ncclAllReduce / ncclCommDestroy";
        dlclose(api.h);
        api.h = nullptr;
        return nullptr;
    }
    return &api;
}

void group_comm_destroy(ncclComm_t comm)
{
    if (RcclApi *R = rccl_api()) (void)R->CommDestroy(comm);
}

#define RCCL_TRY(c, expr)                                                                                  \
    do {                                                                                                   \
        ncclResult_t r_ = (expr);                                                                          \
        if (r_ != ncclSuccess)                                                                             \
            return fail((c), MMP_EHIP, "%s failed: %s (%s:%d)", #expr,                                     \
                        rccl_api()->GetErrorString ? rccl_api()->GetErrorString(r_) : "rccl error", __FILE__, __LINE__); \
    } while (0)

// all-reduce in place on the context's stream; a group of one without a communicator has nothing to exchange
int group_allreduce(mmp_ctx *c, void *buf, size_t count, ncclDataType_t dt, ncclRedOp_t op)
{
    if (count == 0) return MMP_OK;
    if (c->xfn) {
        const int rc = c->xfn(c->xuser, buf, (int64_t)count, dt == ncclInt64 ? 1 : 0, op == ncclMin ? 1 : 0, c->stream);
        return rc == 0 ? MMP_OK : fail(c, MMP_EHIP, "the host's exchange callback failed (%d)", rc);
    }
    if (!c->comm) return MMP_OK;
    RCCL_TRY(c, rccl_api()->AllReduce(buf, buf, count, dt, op, c->comm, c->stream));
    return MMP_OK;
}

// the six exchange phases + the result rows for `n` request rows (n_dev: the real row count on the device, or null)
int group_general(mmp_ctx *c, const void *d_reqs, int32_t n, const int32_t *n_dev, const void *d_extra, int64_t now, void *d_outs)
{
    void *xs[6];
    for (int ph = 1; ph <= 6; ph++) {
        HIP_TRY(c, c->g_x[ph - 1].ensure((size_t)std::max(n, 1) * mmp_shard_xchg_slots(ph, c->n_shards) * 8));
        xs[ph - 1] = c->g_x[ph - 1].p;
    }
    for (int ph = 1; ph <= 7; ph++) {
        {
            std::lock_guard<std::shared_mutex> g(c->mu);
            const int rc = shard_phase_launch(c, ph, d_reqs, n, n_dev, d_extra, now, xs, d_outs, c->stream);
            if (rc != MMP_OK) return rc;
        }
        if (ph <= 6) {
            const int rc = group_allreduce(c, xs[ph - 1], (size_t)n * mmp_shard_xchg_slots(ph, c->n_shards), ncclInt64,
                                           mmp_shard_xchg_is_sum(ph) ? ncclSum : ncclMin);
            if (rc != MMP_OK) return rc;
        }
    }
    return MMP_OK;
}
}  // namespace

int mmp_shard_unique_id(void *id_out)
{
    if (!id_out) return fail(nullptr, MMP_EINVAL, "mmp_shard_unique_id: null argument");
    std::string why;
    RcclApi *R = rccl_api(&why);
    if (!R) return fail(nullptr, MMP_ENODEVICE, "RCCL is not available: %s", why.c_str());
    ncclUniqueId id;
    RCCL_TRY(nullptr, R->GetUniqueId(&id));
    memcpy(id_out, &id, sizeof id);
    return MMP_OK;
}

int mmp_shard_group_init(mmp_ctx *c, const void *unique_id, int32_t rank, int32_t world)
try {
    if (!c || world < 1 || rank < 0 || rank >= world || (world > 1 && !unique_id && !c->xfn))
        return fail(c, MMP_EINVAL, "mmp_shard_group_init: bad argument (a group of more than one shard needs a unique id or an exchange callback)");
    std::lock_guard<std::mutex> gg(c->group_mu);
    if (c->group) return fail(c, MMP_ESTATE, "mmp_shard_group_init: the context already belongs to a group");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    if (unique_id) {
        std::string why;
        RcclApi *R = rccl_api(&why);
        if (!R) return fail(c, MMP_ENODEVICE, "RCCL is not available on this host: %s", why.c_str());
        ncclUniqueId id;
        memcpy(&id, unique_id, sizeof id);
        RCCL_TRY(c, R->CommInitRank(&c->comm, world, id, rank));
    }
    const int rc = mmp_shard_configure(c, rank, world);
    if (rc != MMP_OK) {
        if (c->comm) (void)rccl_api()->CommDestroy(c->comm);
        c->comm = nullptr;
        return rc;
    }
    c->g_rank = rank;
    c->g_world = world;
    c->group = true;
    return MMP_OK;
} MMP_CATCH(c, "mmp_shard_group_init")

int mmp_shard_group_set_exchange(mmp_ctx *c, mmp_exchange_fn fn, void *user)
{
    if (!c) return MMP_EINVAL;
    std::lock_guard<std::mutex> gg(c->group_mu);
    if (c->group) return fail(c, MMP_ESTATE, "mmp_shard_group_set_exchange: set the callback before mmp_shard_group_init");
    c->xfn = fn;
    c->xuser = user;
    return MMP_OK;
}

namespace {
int shard_resolve_pending(mmp_ctx *c);
}
int mmp_shard_group_destroy(mmp_ctx *c)
{
    if (!c) return MMP_EINVAL;
    std::lock_guard<std::mutex> gg(c->group_mu);
    if (!c->group) return MMP_OK;
    (void)hipSetDevice(c->cfg.device);
    (void)shard_resolve_pending(c);
    (void)hipStreamSynchronize(c->stream);
    if (c->comm) (void)rccl_api()->CommDestroy(c->comm);
    c->comm = nullptr;
    c->group = false;
    return MMP_OK;
}

/* Sharded commit, collective over the group: every shard ranks its slice of the instances against all of them,
 * ncclAllReduce(SUM) of int32 rank[P] on the library's stream, every shard scatters the positions it owns. */
int mmp_shard_commit(mmp_ctx *c)
try {
    if (!c) return MMP_EINVAL;
    std::lock_guard<std::mutex> gg(c->group_mu);
    if (!c->group) return fail(c, MMP_ESTATE, "mmp_shard_commit: call mmp_shard_group_init first");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    {
        const int rc0 = shard_resolve_pending(c);  // an open asynchronous batch is decided against the snapshot it was issued on
        if (rc0 != MMP_OK) return rc0;
    }
    size_t P;
    {
        std::lock_guard<std::shared_mutex> g(c->mu);
        P = c->pods.size();
    }
    HIP_TRY(c, c->g_rankbuf.ensure(std::max<size_t>(P, 1) * 4));
    int rc = mmp_shard_rank_dev(c, c->g_rankbuf.p);  // synchronises c->stream
    if (rc != MMP_OK) return rc;
    rc = group_allreduce(c, c->g_rankbuf.p, P, ncclInt32, ncclSum);
    if (rc != MMP_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return mmp_shard_commit_dev(c, c->g_rankbuf.p);
} MMP_CATCH(c, "mmp_shard_commit")

/* One batch on the pod-axis group, device pointers, collective: returns when d_outs is complete on every shard.
 * fast kernel -> ncclAllReduce(MIN, 2 int64 per decision) -> decided rows + compaction of the rest -> the six
 * exchange phases over a sub-batch of fixed CAPACITY (max(1024, n / 16) rows; the real count stays on the device, so
 * no host round trip sits between the kernels and every collective has a size the host knows) -> scatter.  Only
 * when more decisions than that capacity need the six phases — the host learns it with the results — are they run
 * again at their exact size. */
namespace {
int shard_place_batch_locked(mmp_ctx *c, const void *d_reqs, int32_t n, const void *d_extra, int64_t now, void *d_outs, int32_t *n_rest_out,
                             bool wait);
int shard_resolve_pending(mmp_ctx *c);
}
int mmp_shard_place_batch_dev(mmp_ctx *c, const void *d_reqs, int32_t n, const void *d_extra, int64_t now, void *d_outs,
                              int32_t *n_rest_out)
try {
    if (!c || n < 0 || (n > 0 && (!d_reqs || !d_outs))) return fail(c, MMP_EINVAL, "mmp_shard_place_batch_dev: bad argument");
    std::lock_guard<std::mutex> gg(c->group_mu);
    return shard_place_batch_locked(c, d_reqs, n, d_extra, now, d_outs, n_rest_out, true);
} MMP_CATCH(c, "mmp_shard_place_batch_dev")

namespace {
// the batch of mmp_shard_place_batch_async_dev that is still open: wait for its finish kernel, read the rest count, run the six
// phases over the rest if there is one.  The caller holds c->group_mu.  n_rest identical on every shard (the same reduced
// words): the group stays in step.
int shard_resolve_pending(mmp_ctx *c)
{
    if (!c->pend.active) return MMP_OK;
    const mmp_ctx::ShardPending P = c->pend;
    c->pend.active = false;
    hipStream_t st = c->stream;
    int32_t n_rest = 0;
    // the count is polled WITHOUT the state lock (every decision path holds it shared: a spin under the exclusive lock stalled them
    // for the whole wait); only the gather's buffers need it
    int rc = shard_finish_collect(c, P.slot, st, P.seq, &n_rest);
    if (rc == MMP_OK && n_rest > 0) {
        std::lock_guard<std::shared_mutex> g(c->mu);
        rc = shard_rest_gather(c, P.slot, P.d_reqs, P.n, n_rest, st);
    }
    if (rc != MMP_OK) return rc;
    c->last_n_rest = n_rest;
    if (n_rest > 0) {
        rc = group_general(c, c->f_reqs.p, n_rest, nullptr, P.d_extra, P.now, c->f_outs.p);
        if (rc != MMP_OK) return rc;
        hipLaunchKernelGGL(place_shard_scatter_kernel, dim3(div_up(n_rest, 256)), dim3(256), 0, st, c->f_outs.as<mmp_place_out>(),
                           c->f_idx.as<int32_t>(), n_rest, static_cast<mmp_place_out *>(P.d_outs), nullptr);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(st));
    }
    return MMP_OK;
}

// the body of the group's batch calls; the caller holds c->group_mu (and nothing that is ordered behind it).  wait = false:
// returns with the fast kernel, the all-reduce and the finish kernel enqueued (mmp_shard_place_batch_async_dev)
int shard_place_batch_locked(mmp_ctx *c, const void *d_reqs, int32_t n, const void *d_extra, int64_t now, void *d_outs, int32_t *n_rest_out,
                             bool wait = true)
{
    if (!c->group) return fail(c, MMP_ESTATE, "mmp_shard_place_batch_dev: call mmp_shard_group_init first");
    if (n_rest_out) *n_rest_out = 0;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int rc;
    if (n == 0) {
        rc = shard_resolve_pending(c);
        c->last_n_rest = rc == MMP_OK ? 0 : c->last_n_rest;
        return rc;
    }
    // This batch is enqueued FIRST, on the buffers of the other slot; the batch before it — whose finish kernel has had the time
    // of these three launches to end — is completed afterwards, and whatever its rest needs is enqueued behind this batch.
    hipStream_t st = c->stream;
    const uint32_t slot = c->f_slot ^= 1u;
    uint32_t seq = 0;
    if (c->n_shards == 1) {
        // a group of one shard: the slice's answer IS the answer — one launch writes rows, rest flags and count (no exchange words,
        // no all-reduce, no finish kernel)
        std::lock_guard<std::shared_mutex> g(c->mu);
        if (!c->committed) return fail(c, MMP_ESTATE, "no committed shard snapshot");
        rc = shard_finish_prepare(c, slot, n, st, &seq);
        if (rc != MMP_OK) return rc;
        const PlaceArgs A = shard_args(c, d_reqs, n, d_extra, now, d_outs);
        hipLaunchKernelGGL(place_shard_fast_direct_kernel, dim3(div_up(n + 1, kPlaceBlock)), dim3(kPlaceBlock), (size_t)place_lane_lds(c->sview.T),
                           st, c->sview, A, c->shard, c->ssnap.any_rs, c->f_flags[slot].as<int32_t>(), c->f_cnt[slot].as<unsigned long long>(),
                           c->f_done + 8 * slot, seq);
        HIP_TRY(c, hipGetLastError());
    } else {
        HIP_TRY(c, c->g_xf[slot].ensure((size_t)n * kXF * 8));
        rc = mmp_shard_place_fast_dev(c, d_reqs, n, d_extra, now, c->g_xf[slot].p, st);
        if (rc != MMP_OK) return rc;
        rc = group_allreduce(c, c->g_xf[slot].p, (size_t)n * kXF, ncclInt64, ncclMin);
        if (rc != MMP_OK) return rc;
        std::lock_guard<std::shared_mutex> g(c->mu);
        rc = shard_finish_enqueue(c, slot, n, c->g_xf[slot].p, d_outs, st, &seq);
        if (rc != MMP_OK) return rc;
    }
    rc = shard_resolve_pending(c);
    if (rc != MMP_OK) return rc;
    c->pend.slot = slot;
    c->pend.active = true;
    c->pend.d_reqs = d_reqs;
    c->pend.d_extra = d_extra;
    c->pend.d_outs = d_outs;
    c->pend.n = n;
    c->pend.now = now;
    c->pend.seq = seq;
    if (!wait) return MMP_OK;
    // Round 2 kept the rest count on the device and ALWAYS ran the six-exchange protocol over a fixed-capacity sub-batch (seven
    // launches and six collectives that mostly found no rows): 99 us per 100k decisions at one shard against 50 us for the form
    // that asks.
    rc = shard_resolve_pending(c);
    if (rc != MMP_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(st));  // the caller reads d_outs next
    if (n_rest_out) *n_rest_out = c->last_n_rest;
    return MMP_OK;
}
}  // namespace

int mmp_shard_place_batch_async_dev(mmp_ctx *c, const void *d_reqs, int32_t n, const void *d_extra, int64_t now, void *d_outs)
try {
    if (!c || n < 0 || (n > 0 && (!d_reqs || !d_outs))) return fail(c, MMP_EINVAL, "mmp_shard_place_batch_async_dev: bad argument");
    std::lock_guard<std::mutex> gg(c->group_mu);
    return shard_place_batch_locked(c, d_reqs, n, d_extra, now, d_outs, nullptr, false);
} MMP_CATCH(c, "mmp_shard_place_batch_async_dev")

int mmp_shard_wait(mmp_ctx *c, int32_t *n_rest_out)
try {
    if (!c) return MMP_EINVAL;
    std::lock_guard<std::mutex> gg(c->group_mu);
    if (!c->group) return fail(c, MMP_ESTATE, "mmp_shard_wait: call mmp_shard_group_init first");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const int rc = shard_resolve_pending(c);
    if (rc != MMP_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (n_rest_out) *n_rest_out = c->last_n_rest;
    return MMP_OK;
} MMP_CATCH(c, "mmp_shard_wait")

/* The same with host pointers (what a JVM holds): staged through the context's scratch. */
int mmp_shard_place_batch(mmp_ctx *c, const mmp_place_req *reqs, int32_t n, const int32_t *extra_pool, int32_t n_extra,
                          int64_t now, mmp_place_out *outs, int32_t *n_rest_out)
try {
    if (!c || n < 0 || n_extra < 0 || (n > 0 && (!reqs || !outs)) || (n_extra > 0 && !extra_pool))
        return fail(c, MMP_EINVAL, "mmp_shard_place_batch: bad argument");
    for (int32_t i = 0; i < n; i++)
        if (reqs[i].n_extra < 0 || reqs[i].extra_off < 0 || (int64_t)reqs[i].extra_off + reqs[i].n_extra > n_extra)
            return fail(c, MMP_EINVAL, "mmp_shard_place_batch: request %d extra range out of bounds", i);
    if (n_rest_out) *n_rest_out = 0;
    if (n == 0) return MMP_OK;
    // lock order of the group entry points: group_mu, then batch_mu (mmp_shard_commit and mmp_shard_group_init take
    // batch_mu through the calls they make while holding group_mu)
    std::lock_guard<std::mutex> gg(c->group_mu);
    std::lock_guard<std::mutex> gb(c->batch_mu);  // the staging scratch
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, c->s_reqs.ensure((size_t)n * sizeof(mmp_place_req)));
    HIP_TRY(c, c->s_outs.ensure((size_t)n * sizeof(mmp_place_out)));
    HIP_TRY(c, c->s_extra.ensure((size_t)std::max(n_extra, 1) * 4));
    HIP_TRY(c, hipMemcpyAsync(c->s_reqs.p, reqs, (size_t)n * sizeof(mmp_place_req), hipMemcpyHostToDevice, c->stream));
    if (n_extra) HIP_TRY(c, hipMemcpyAsync(c->s_extra.p, extra_pool, (size_t)n_extra * 4, hipMemcpyHostToDevice, c->stream));
    const int rc = shard_place_batch_locked(c, c->s_reqs.p, n, c->s_extra.p, now, c->s_outs.p, n_rest_out, true);
    if (rc != MMP_OK) return rc;
    HIP_TRY(c, copy_sync(c, outs, c->s_outs.p, (size_t)n * sizeof(mmp_place_out), hipMemcpyDeviceToHost));
    return MMP_OK;
} MMP_CATCH(c, "mmp_shard_place_batch")

/* ---- submission threads ---------------------------------------------------
 * One host thread needs ~3 us per kernel launch (HIP's launch path), which is more than a 100k-decision batch takes the
 * GPU when several are in flight.  mmp_issue_threads(ctx, n) starts n helper threads that spin on per-helper rings;
 * while they run, mmp_place_batch_dev only validates, appends a descriptor (tens of ns) and returns, and the helpers
 * launch in parallel — every caller stream is pinned to one helper, so launches on one stream keep their order.
 * mmp_issue_flush waits until everything submitted so far has been launched (and reports the first launch error);
 * mmp_stream_retire, mmp_issue_threads and mmp_destroy flush first.  A commit or a registry event does NOT (it holds
 * the state lock the helpers launch under, and it need not): a helper captures the published snapshot when it launches,
 * so a descriptor that is still in a ring when another snapshot is published is decided against that one, and the
 * stream it is bound for was noted at submission, so whoever rewrites state afterwards waits for it. */
struct IssueItem {
    const void *d_reqs, *d_extra;
    void *d_outs;
    hipStream_t st;
    int64_t now;
    int32_t n;
};
struct IssueRing {
    static constexpr uint32_t kCap = 4096;
    IssueItem items[kCap];
    alignas(64) std::atomic<uint32_t> tail{0};  // producers (under push_mu)
    alignas(64) std::atomic<uint32_t> head{0};  // the helper
    std::mutex push_mu;
};
struct IssuePool {
    std::vector<std::thread> th;
    std::vector<IssueRing *> rings;
    std::atomic<bool> stop{false};
    std::atomic<bool> closed{false};  // set (then every push_mu taken once) before the helpers are told to stop: a submitter
                                      // that still holds a reference launches by itself instead of appending
    ~IssuePool()
    {
        for (IssueRing *R : rings) delete R;
    }
    std::atomic<int> first_rc{MMP_OK};
    std::mutex map_mu;
    std::vector<std::pair<hipStream_t, int>> stream_ring;  // caller stream -> helper, assigned round-robin at first sight
    int next_ring = 0;
};

namespace {
void issue_helper(mmp_ctx *c, IssuePool *P, IssueRing *R)
{
    (void)hipSetDevice(c->cfg.device);
    uint32_t idle = 0;
    for (;;) {
        const uint32_t h = R->head.load(std::memory_order_relaxed);
        if (h == R->tail.load(std::memory_order_acquire)) {
            if (P->stop.load(std::memory_order_acquire)) return;
            if (++idle > 64) __builtin_ia32_pause();
            continue;
        }
        idle = 0;
        const IssueItem it = R->items[h % IssueRing::kCap];
        int rc;
        {
            std::shared_lock<std::shared_mutex> g(c->mu);  // capture the published snapshot + enqueue
            rc = !c->committed ? fail(c, MMP_ESTATE, "no committed snapshot")
                               : place_launch(c, it.d_reqs, it.n, it.d_extra, it.now, it.d_outs, it.st);
        }
        if (rc != MMP_OK) {
            int expect = MMP_OK;
            (void)P->first_rc.compare_exchange_strong(expect, rc);
        }
        R->head.store(h + 1, std::memory_order_release);
    }
}

int issue_ring_of(IssuePool *P, hipStream_t st)
{
    std::lock_guard<std::mutex> g(P->map_mu);
    for (auto &kv : P->stream_ring)
        if (kv.first == st) return kv.second;
    const int r = P->next_ring++ % (int)P->rings.size();
    P->stream_ring.emplace_back(st, r);
    return r;
}

void pool_get(mmp_ctx *c, std::shared_ptr<IssuePool> &out)
{
    std::lock_guard<std::mutex> g(c->pool_mu);
    out = c->pool;
}

// everything submitted so far has been handed to HIP (called without the state lock)
int issue_flush_pool(IssuePool *P)
{
    if (!P) return MMP_OK;
    for (IssueRing *R : P->rings)
        while (R->head.load(std::memory_order_acquire) != R->tail.load(std::memory_order_acquire)) __builtin_ia32_pause();
    return P->first_rc.exchange(MMP_OK);
}
int issue_flush(mmp_ctx *c)
{
    std::shared_ptr<IssuePool> P;
    pool_get(c, P);
    return issue_flush_pool(P.get());
}
}  // namespace

int mmp_issue_threads(mmp_ctx *c, int32_t n)
try {
    if (!c || n < 0 || n > 64) return fail(c, MMP_EINVAL, "mmp_issue_threads: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::shared_ptr<IssuePool> old;
    {
        std::lock_guard<std::mutex> g(c->pool_mu);
        old.swap(c->pool);  // new submitters launch by themselves from here on
    }
    if (old) {
        old->closed.store(true, std::memory_order_release);
        for (IssueRing *R : old->rings) std::lock_guard<std::mutex> barrier(R->push_mu);  // appends in flight have landed
        const int rc = issue_flush_pool(old.get());
        old->stop.store(true, std::memory_order_release);
        for (std::thread &t : old->th) t.join();
        old.reset();  // the rings go with the last reference (a submitter may still hold one; it sees `closed`)
        if (rc != MMP_OK) return rc;
    }
    if (n == 0) return MMP_OK;
    auto P = std::make_shared<IssuePool>();
    for (int i = 0; i < n; i++) P->rings.push_back(new IssueRing());
    for (int i = 0; i < n; i++) P->th.emplace_back(issue_helper, c, P.get(), P->rings[i]);
    {
        std::lock_guard<std::mutex> g(c->pool_mu);
        c->pool = P;
    }
    return MMP_OK;
} MMP_CATCH(c, "mmp_issue_threads")

int mmp_issue_flush(mmp_ctx *c)
{
    if (!c) return MMP_EINVAL;
    const int rc = issue_flush(c);
    return rc == MMP_OK ? MMP_OK : fail(c, rc, "a launch submitted through the issue threads failed (%d)", rc);
}

/* ---- the resident decision kernel: single requests without a launch --------- */
namespace {
constexpr int kResidentFallback = 1;  // "take the launch path" (never an MMP_* code)

// make sure a resident kernel is running on the published snapshot (lock order: state lock, then launch_mu)
int resident_ensure(mmp_ctx *c)
{
    auto &R = c->res;
    std::shared_lock<std::shared_mutex> gs(c->mu);
    if (!c->committed) return fail(c, MMP_ESTATE, "no committed snapshot");
    if (c->n_shards > 0) return kResidentFallback;
    std::lock_guard<std::mutex> g(R.launch_mu);
    if (R.running && __atomic_load_n(&R.ctl->exited, __ATOMIC_ACQUIRE) != R.generation) return MMP_OK;
    if (R.running) {
        HIP_TRY(c, hipStreamSynchronize(R.stream));  // it left by itself (idle): returns at once
        R.running = false;
    }
    {
        uint32_t g2 = R.generation.load(std::memory_order_relaxed) + 1;
        if (g2 == 0) g2 = 1;
        R.generation.store(g2, std::memory_order_release);
    }
    PlaceArgs A = place_args(c, nullptr, 1, nullptr, 0, nullptr, true, c->snap.P);
    A.wins = c->sb[c->cur].heads.as<TypeWin>();
    HIP_TRY(c, order_after_registry(c, R.stream));
    hipLaunchKernelGGL(place_resident_kernel, dim3(1), dim3(64), (size_t)kPlaceLaneLds, R.stream, c->snap, A, R.slots, R.answers, R.ctl,
                       R.idle_ticks, R.generation.load(std::memory_order_relaxed));
    HIP_TRY(c, hipGetLastError());
    R.running = true;
    R.launches.fetch_add(1, std::memory_order_relaxed);
    return MMP_OK;
}

int resident_place(mmp_ctx *c, const mmp_place_req &rq, int64_t now, mmp_place_out *out)
{
    auto &R = c->res;
    if (R.skip.load(std::memory_order_relaxed) > 0) {
        R.skip.fetch_sub(1, std::memory_order_relaxed);
        return kResidentFallback;
    }
    // a slot of our own for the duration of the call
    const uint32_t first = R.rr.fetch_add(1, std::memory_order_relaxed);
    int si = -1;
    std::unique_lock<std::mutex> sl;
    for (int k = 0; k < kResidentSlots && si < 0; k++) {
        const int cand = (int)((first + k) % kResidentSlots);
        std::unique_lock<std::mutex> t(R.slot_mu[cand], std::try_to_lock);
        if (t.owns_lock()) {
            sl = std::move(t);
            si = cand;
        }
    }
    if (si < 0) {
        si = (int)(first % kResidentSlots);
        sl = std::unique_lock<std::mutex>(R.slot_mu[si]);
    }
    ResidentSlot *S = &R.slots[si];
    ResidentAnswer *Ans = &R.answers[si];
    uint32_t seq = (R.seq[si] + 1) & 0xfffffu;  // 20 bits ride in the bell next to now_ms
    if (seq == 0) seq = 1;
    R.seq[si] = seq;
    S->req = rq;
    __atomic_store_n(&S->bell, ((uint64_t)seq << kResidentNowBits) | ((uint64_t)now & ((1ull << kResidentNowBits) - 1ull)),
                     __ATOMIC_RELEASE);  // the bell: written last
    bool restarted = false;  // this call (re)started the kernel, or waited for a commit to do so: not a sample for the self-check
    if (!R.running || __atomic_load_n(&R.ctl->exited, __ATOMIC_ACQUIRE) == R.generation) {
        const int rc = resident_ensure(c);
        if (rc != MMP_OK) return rc;
        restarted = true;
    }
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spins = 0;; spins++) {
        const uint32_t d = __atomic_load_n(&Ans->done, __ATOMIC_ACQUIRE);
        if ((d & ~kResidentPunt) == seq) {
            if (d & kResidentPunt) {
                R.punted.fetch_add(1, std::memory_order_relaxed);
                // a table on which most decisions need the wave path (every instance a candidate ...) makes the resident
                // attempt pure overhead: after 8 hand-backs in a row the next 4096 single requests go to the launch path directly
                if (R.punt_streak.fetch_add(1, std::memory_order_relaxed) + 1 >= 8) {
                    R.punt_streak.store(0, std::memory_order_relaxed);
                    R.skip.store(4096, std::memory_order_relaxed);
                }
                return kResidentFallback;  // a shape the resident wavefront leaves to the launch path
            }
            R.punt_streak.store(0, std::memory_order_relaxed);
            *out = Ans->out;
            R.served.fetch_add(1, std::memory_order_relaxed);
            // Self-check: an answer takes ~10 us.  Three answers IN A ROW slower than 20 ms — from a kernel that was running
            // when the request was posted and was not restarted while it waited (a commit stops it) — switch the resident path
            // off for this context and the launch path takes over (what that looked like before the resident stream got a
            // priority level of its own: 50 ms per call, the time the resident kernel needs to idle out of the way of a launch
            // queued behind it).  A request thread that lost its core for a few milliseconds is not such a sample.
            const bool slow_answer = !restarted && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20);
            if (!slow_answer && !restarted) R.slow.store(0, std::memory_order_relaxed);
            if (slow_answer && R.slow.fetch_add(1) + 1 >= 3) {
                R.enabled = false;
                (void)fail(c, MMP_OK, "resident decision kernel disabled: three answers in a row took longer than 20 ms on this host");
            }
            return MMP_OK;
        }
        if ((spins & 255) == 255) {
            if (__atomic_load_n(&R.ctl->exited, __ATOMIC_ACQUIRE) == R.generation) {  // it left (idle, or stopped for a commit) before it saw the bell
                const int rc = resident_ensure(c);
                if (rc != MMP_OK) return rc;
                restarted = true;
            }
            if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200))
                return fail(c, MMP_EHIP, "the resident decision kernel did not answer within 200 ms");
        }
        __builtin_ia32_pause();
    }
}
}  // namespace

int mmp_resident(mmp_ctx *c, int enable)
try {
    if (!c) return MMP_EINVAL;
    std::lock_guard<std::mutex> gb(c->batch_mu);
    auto &R = c->res;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    if (enable && !R.slots) {
        // A stream of the LOWEST priority: HIP multiplexes the streams of one priority level onto a small pool of hardware
        // queues, and a kernel that never ends blocks whatever else lands on its queue.  On the latency slots' level (highest)
        // it held their launches back until it idled out — 50 ms per request that it had handed back to the launch path
        // (tools/micro/single_calls.cc, SINGLE_CALLS_FLAT=1).  Nothing else in the library uses the lowest level.
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        HIP_TRY(c, hipStreamCreateWithPriority(&R.stream, hipStreamNonBlocking, lo));
        HIP_TRY(c, hipHostMalloc(reinterpret_cast<void **>(&R.slots), sizeof(ResidentSlot) * kResidentSlots, kPinnedFlags));
        HIP_TRY(c, hipHostMalloc(reinterpret_cast<void **>(&R.ctl), sizeof(ResidentCtl), kPinnedFlags));
        HIP_TRY(c, hipHostMalloc(reinterpret_cast<void **>(&R.answers), sizeof(ResidentAnswer) * kResidentSlots, kPinnedFlags));
        memset(R.answers, 0, sizeof(ResidentAnswer) * kResidentSlots);
        memset(R.slots, 0, sizeof(ResidentSlot) * kResidentSlots);
        memset(R.ctl, 0, sizeof(ResidentCtl));
        int khz = 100000;
        (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->cfg.device);
        long long ms = 50;
        if (const char *e = getenv("MMP_RESIDENT_IDLE_MS")) ms = std::max(1, atoi(e));
        R.idle_ticks = (long long)khz * ms;
    }
    if (!enable) {
        std::lock_guard<std::shared_mutex> g(c->mu);
        R.enabled = false;
        resident_stop(c);
        return MMP_OK;
    }
    R.enabled = true;
    return MMP_OK;
} MMP_CATCH(c, "mmp_resident")

int mmp_resident_stats(mmp_ctx *c, uint64_t *launches, uint64_t *served, uint64_t *punted)
{
    if (!c) return MMP_EINVAL;
    if (launches) *launches = c->res.launches.load();
    if (served) *served = c->res.served.load();
    if (punted) *punted = c->res.punted.load();
    return MMP_OK;
}

/* ---- decisions ---------------------------------------------------------- */

int mmp_place_multi_dev(mmp_ctx *c, int32_t k, const void *const *d_reqs, const int32_t *n, const void *const *d_extra, int64_t now,
                        void *const *d_outs, void *stream)
try {
    if (!c || k < 0 || (k > 0 && (!d_reqs || !n || !d_outs))) return fail(c, MMP_EINVAL, "mmp_place_multi_dev: bad argument");
    for (int32_t i = 0; i < k; i++)
        if (n[i] < 0 || (n[i] > 0 && (!d_reqs[i] || !d_outs[i]))) return fail(c, MMP_EINVAL, "mmp_place_multi_dev: bad argument (array %d)", i);
    if (const int rc = refuse_per_thread_stream(c, stream, "mmp_place_multi_dev")) return rc;
    {  // launches handed to submission threads earlier are issued first: this call launches from the calling thread, in stream order
        std::shared_ptr<IssuePool> P;
        pool_get(c, P);
        if (P) {
            const int rc = issue_flush(c);
            if (rc != MMP_OK) return fail(c, rc, "a launch submitted through the issue threads failed (%d)", rc);
        }
    }
    std::shared_lock<std::shared_mutex> g(c->mu);  // capture the published snapshot + enqueue; no wait
    if (!c->committed) return fail(c, MMP_ESTATE, "no committed snapshot");
    if (c->n_shards > 0) return fail(c, MMP_ESTATE, "context is a pod-axis shard: use mmp_shard_place_phase_dev");
    hipStream_t st = static_cast<hipStream_t>(stream);
    note_caller_stream(c, st);
    for (int32_t i0 = 0; i0 < k;) {  // kMaxSegs arrays per launch
        PlaceSegs G{};
        int32_t blocks = 0;
        int64_t total = 0;
        int32_t i = i0;
        for (; i < k && G.n_segs < kMaxSegs; i++) {
            if (n[i] == 0) continue;
            PlaceSeg &sg = G.seg[G.n_segs++];
            sg.reqs = static_cast<const mmp_place_req *>(d_reqs[i]);
            sg.outs = static_cast<mmp_place_out *>(d_outs[i]);
            sg.extra = d_extra ? static_cast<const int32_t *>(d_extra[i]) : nullptr;
            sg.first_block = blocks;
            sg.n = n[i];
            blocks += div_up(n[i], kPlaceBlock);
            total += n[i];
        }
        i0 = i;
        if (G.n_segs == 0) continue;
        if (total > INT32_MAX - kPlaceBlock * (int64_t)kMaxSegs) return fail(c, MMP_EINVAL, "mmp_place_multi_dev: more than 2^31 decisions in one launch");
        PlaceCall o;
        o.segs = &G;
        o.seg_blocks = blocks;
        const int rc = place_launch(c, G.seg[0].reqs, (int32_t)total, G.seg[0].extra, now, G.seg[0].outs, st, o);
        if (rc != MMP_OK) return rc;
    }
    return MMP_OK;
} MMP_CATCH(c, "mmp_place_multi_dev")

int mmp_place_batch_dev(mmp_ctx *c, const void *d_reqs, int32_t n, const void *d_extra, int64_t now, void *d_outs,
                        void *stream)
try {
    if (!c || n < 0 || (n > 0 && (!d_reqs || !d_outs))) return fail(c, MMP_EINVAL, "mmp_place_batch_dev: bad argument");
    if (const int rc = refuse_per_thread_stream(c, stream, "mmp_place_batch_dev")) return rc;
    std::shared_ptr<IssuePool> P;
    pool_get(c, P);
    if (P) {  // submission threads: append and return
        if (n == 0) return MMP_OK;
        hipStream_t st = static_cast<hipStream_t>(stream);
        IssueRing *R = P->rings[issue_ring_of(P.get(), st)];
        {
            std::shared_lock<std::shared_mutex> g(c->mu);
            if (!c->committed) return fail(c, MMP_ESTATE, "no committed snapshot");
            if (c->n_shards > 0) return fail(c, MMP_ESTATE, "context is a pod-axis shard: use mmp_shard_place_phase_dev");
            note_caller_stream(c, st);
        }
        std::lock_guard<std::mutex> gp(R->push_mu);
        if (!P->closed.load(std::memory_order_acquire)) {
            const uint32_t t = R->tail.load(std::memory_order_relaxed);
            while (t - R->head.load(std::memory_order_acquire) >= IssueRing::kCap) __builtin_ia32_pause();
            R->items[t % IssueRing::kCap] = IssueItem{d_reqs, d_extra, d_outs, st, now, n};
            R->tail.store(t + 1, std::memory_order_release);
            return MMP_OK;
        }
        // the pool was retired while this call held its reference: launch here, like a context without helpers
    }
    std::shared_lock<std::shared_mutex> g(c->mu);  // capture the published snapshot + enqueue; no wait
    if (!c->committed) return fail(c, MMP_ESTATE, "no committed snapshot");
    if (c->n_shards > 0) return fail(c, MMP_ESTATE, "context is a pod-axis shard: use mmp_shard_place_phase_dev");
    note_caller_stream(c, static_cast<hipStream_t>(stream));
    return place_launch(c, d_reqs, n, d_extra, now, d_outs, static_cast<hipStream_t>(stream));
} MMP_CATCH(c, "mmp_place_batch_dev")

int mmp_stream_retire(mmp_ctx *c, void *stream)
try {
    if (!c) return MMP_EINVAL;
    if (const int rc = refuse_per_thread_stream(c, stream, "mmp_stream_retire")) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    (void)issue_flush(c);  // launches submitted for this stream have reached it
    {
        std::lock_guard<std::mutex> g(c->cs_mu);
        auto it = std::find(c->caller_streams.begin(), c->caller_streams.end(), st);
        if (it == c->caller_streams.end()) return MMP_OK;
        c->caller_streams.erase(it);
    }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamSynchronize(st));  // what was enqueued on it has finished reading the library's tables
    // ... and its split batches with their buffer: the slot goes back (a stream created later may get the same handle)
    mmp_ctx::MissBuf *mb = nullptr;
    {
        std::lock_guard<std::mutex> g(c->miss_mu);
        for (auto &b : c->miss_bufs)
            if (b.used && b.st == st) mb = &b;
    }
    if (mb) {
        std::lock_guard<std::mutex> gs(mb->mu);
        void *words = nullptr;
        {
            std::lock_guard<std::mutex> g(c->miss_mu);
            if (mb->used && mb->st == st) {
                words = mb->words;
                mb->words = nullptr;
                mb->cap = 0;
                mb->used = false;
                mb->st = nullptr;
            }
        }
        if (words) HIP_TRY(c, hipFree(words));
    }
    return MMP_OK;
} MMP_CATCH(c, "mmp_stream_retire")

int mmp_place_batch_dev2(mmp_ctx *c, const void *d_reqs, int32_t n, const void *d_extra, int32_t n_extra_pool, int64_t now,
                         void *d_outs, void *stream)
try {
    if (!c || n < 0 || n_extra_pool < 0 || (n > 0 && (!d_reqs || !d_outs)) || (n_extra_pool > 0 && !d_extra))
        return fail(c, MMP_EINVAL, "mmp_place_batch_dev2: bad argument");
    if (const int rc = refuse_per_thread_stream(c, stream, "mmp_place_batch_dev2")) return rc;
    std::shared_lock<std::shared_mutex> g(c->mu);  // capture the published snapshot + enqueue; no wait
    if (!c->committed) return fail(c, MMP_ESTATE, "no committed snapshot");
    if (c->n_shards > 0) return fail(c, MMP_ESTATE, "context is a pod-axis shard: use mmp_shard_place_phase_dev");
    note_caller_stream(c, static_cast<hipStream_t>(stream));
    PlaceCall o;
    o.extra_bound = n_extra_pool + 1;
    return place_launch(c, d_reqs, n, d_extra, now, d_outs, static_cast<hipStream_t>(stream), o);
} MMP_CATCH(c, "mmp_place_batch_dev2")

int mmp_place_batch_c_dev(mmp_ctx *c, const mmp_place_caller *caller, const void *d_reqs, int32_t n, const void *d_extra,
                          int32_t n_extra_pool, int64_t now, void *d_outs, void *stream)
try {
    if (!c || !caller || n < 0 || n_extra_pool < 0 || (n > 0 && (!d_reqs || !d_outs)) || (n_extra_pool > 0 && !d_extra))
        return fail(c, MMP_EINVAL, "mmp_place_batch_c_dev: bad argument");
    if (const int rc = refuse_per_thread_stream(c, stream, "mmp_place_batch_c_dev")) return rc;
    std::shared_lock<std::shared_mutex> g(c->mu);
    if (!c->committed) return fail(c, MMP_ESTATE, "no committed snapshot");
    if (c->n_shards > 0) return fail(c, MMP_ESTATE, "context is a pod-axis shard: use mmp_shard_place_phase_dev");
    note_caller_stream(c, static_cast<hipStream_t>(stream));
    PlaceCall o;
    o.caller = caller;
    o.extra_bound = n_extra_pool + 1;
    return place_launch(c, d_reqs, n, d_extra, now, d_outs, static_cast<hipStream_t>(stream), o);
} MMP_CATCH(c, "mmp_place_batch_c_dev")

int mmp_place_batch(mmp_ctx *c, const mmp_place_req *reqs, int32_t n, const int32_t *extra_pool, int32_t n_extra,
                    int64_t now, mmp_place_out *outs);
int mmp_miss_batch(mmp_ctx *c, const mmp_gate_req *greqs, const mmp_place_req *preqs, int32_t n, const int32_t *excl_pod,
                   const int64_t *excl_time, int32_t n_excl, const int32_t *explicit_pool, int32_t n_explicit, const int32_t *extra_pool,
                   int32_t n_extra, int64_t now, int64_t in_use_expiry, mmp_gate_out *gouts, mmp_place_out *pouts);
int mmp_route_batch(mmp_ctx *c, const mmp_gate_req *greqs, const mmp_serve_req *sreqs, int32_t n, const mmp_serve_counter *counters,
                    int32_t n_counters, const int32_t *excl_pod, const int64_t *excl_time, int32_t n_excl,
                    const int32_t *explicit_pool, int32_t n_explicit, int64_t now, int64_t in_use_expiry, mmp_gate_out *gouts,
                    mmp_serve_out *souts);

// ---- the per-request seams: load target (place), cache hit (route), cache miss (miss) -----------------------------------------
// Each seam has a form on full rows (mmp_place_batch / _route_batch / _miss_batch), a single-caller form on compact rows (_c:
// include/mmplace.h: THE RULE; kernels: seam_caller_kernels.hpp) and the single-caller form with the model named by model id (_ck:
// THE RULE BY KEY; keyed_kernels.hpp) or by vmodel id (_cv: THE RULE BY VMODEL KEY; vkeyed_kernels.hpp).  What all of them share is
// stated here once: the argument test, the binding of the kernels' argument blocks, the rows written out, the staged launch bodies.
// How a call's model gets named is a RESOLVER (NoResolver, ByModelId, ByVModelId below): the keyed seams are one body each
// (keyed_place / keyed_route / keyed_miss) with the resolver as a parameter.
extern "C++" {
namespace {
// the guards' pools as every route and miss call brings them
struct GatePools {
    const int32_t *excl_pod;
    const int64_t *excl_time;
    int32_t n_excl;
    const int32_t *explicit_pool;
    int32_t n_explicit;
    bool bad() const { return n_excl < 0 || n_explicit < 0 || (n_excl > 0 && (!excl_pod || !excl_time)) || (n_explicit > 0 && !explicit_pool); }
};

// The argument test of each seam, `fn` the call the host made: NULL / negative arguments, then the pool ranges in request order, the
// gate row's before the other half's.  has_callers: the caller rows the form takes are there.  same_model: the two halves carry a
// model each and must agree (not by id: there both take the resolved row).
template <class Req>
__attribute__((always_inline)) inline int check_place_call(mmp_ctx *c, const char *fn, bool has_callers, const Req *reqs, int32_t n,
                                                           const int32_t *extra_pool, int32_t n_extra, const mmp_place_out *outs)
{
    if (!c || !has_callers || n < 0 || n_extra < 0 || (n > 0 && (!reqs || !outs)) || (n_extra > 0 && !extra_pool))
        return fail(c, MMP_EINVAL, "%s: bad argument", fn);
    for (int32_t i = 0; i < n; i++)
        if (const int rc = check_place_req(c, fn, i, reqs[i], n_extra)) return rc;
    return MMP_OK;
}
template <class GReq, class SReq>
__attribute__((always_inline)) inline int check_route_call(mmp_ctx *c, const char *fn, bool has_callers, const GReq *greqs, const SReq *sreqs,
                                                           int32_t n, const mmp_serve_counter *counters, int32_t n_counters,
                                                           const GatePools &P, const mmp_gate_out *gouts, const mmp_serve_out *souts)
{
    if (!c || !has_callers || n < 0 || n_counters < 0 || P.bad() || (n > 0 && (!greqs || !sreqs || !gouts || !souts)) ||
        (n_counters > 0 && !counters))
        return fail(c, MMP_EINVAL, "%s: bad argument", fn);
    for (int32_t i = 0; i < n; i++) {
        if (const int rc = check_gate_req(c, fn, i, greqs[i], P.n_excl, P.n_explicit)) return rc;
        if (const int rc = check_serve_req(c, fn, i, sreqs[i], P.n_excl, n_counters)) return rc;
        if constexpr (std::is_same_v<SReq, mmp_serve_req>)  // (the compact serve row has no model of its own)
            if (const int rc = check_same_model(c, fn, i, greqs[i].model, sreqs[i].model)) return rc;
    }
    return MMP_OK;
}
template <class GReq, class PReq>
__attribute__((always_inline)) inline int check_miss_call(mmp_ctx *c, const char *fn, bool has_callers, bool same_model, const GReq *greqs,
                                                          const PReq *preqs, int32_t n, const GatePools &P, const int32_t *extra_pool,
                                                          int32_t n_extra, const mmp_gate_out *gouts, const mmp_place_out *pouts)
{
    if (!c || !has_callers || n < 0 || n_extra < 0 || P.bad() || (n > 0 && (!greqs || !preqs || !gouts || !pouts)) ||
        (n_extra > 0 && !extra_pool))
        return fail(c, MMP_EINVAL, "%s: bad argument", fn);
    for (int32_t i = 0; i < n; i++) {
        if (const int rc = check_gate_req(c, fn, i, greqs[i], P.n_excl, P.n_explicit)) return rc;
        if (const int rc = check_place_req(c, fn, i, preqs[i], n_extra)) return rc;
        if (same_model)
            if (const int rc = check_same_model(c, fn, i, greqs[i].model, preqs[i].model)) return rc;
    }
    return MMP_OK;
}
// the counts within which the route and the miss ride a slot
inline bool route_slot_sized(int32_t n, int32_t n_counters, const GatePools &P)
{
    using L = RouteSlot;
    return n <= L::kN && n_counters <= L::kCounters && P.n_excl <= L::kExcl && P.n_explicit <= L::kExplicit;
}
inline bool miss_slot_sized(int32_t n, int32_t n_extra, const GatePools &P)
{
    using L = MissSlot;
    return n <= L::kN && n_extra <= L::kPool && P.n_excl <= L::kPool && P.n_explicit <= L::kPool;
}

// The guards' arrays of a call (all but the request rows): the pools and the results, on the regions of layout L when the call
// rides a slot, staged through the scratch mmp_gate_batch stages them through.
struct GateIo {
    SeamIo xp, xt, ex, go;
};
struct StagedRows {  // the layout of a call that never rides a slot
    static constexpr SlotRegion excl_pod = kStagedOnly, excl_time = kStagedOnly, explicit_pool = kStagedOnly, gouts = kStagedOnly;
};
template <class L>
GateIo gate_io(mmp_ctx *c, const GatePools &P, mmp_gate_out *gouts, int32_t n)
{
    return GateIo{seam_io(P.excl_pod, P.n_excl, L::excl_pod, c->s_c), seam_io(P.excl_time, P.n_excl, L::excl_time, c->s_d),
                  seam_io(P.explicit_pool, P.n_explicit, L::explicit_pool, c->s_a), seam_io(gouts, n, L::gouts, c->s_outs)};
}
// The guards' argument block bound to them (inside a launch body: SeamIo::dev is set).  full_rows: the mmp_gate_req rows, or null
// where the kernel reads compact rows (SeamCArgs).  `done` is the completion flag where the guards' kernel is the call's last.
constexpr DoneFlag kNoDone{nullptr, nullptr, 0};
GateArgs gate_args(mmp_ctx *c, int32_t n, int64_t now, int64_t in_use_expiry, const GateIo &g, const SeamIo *full_rows, const DoneFlag &done)
{
    GateArgs G = gate_args(c, n, now, in_use_expiry);
    G.reqs = full_rows ? full_rows->as<mmp_gate_req>() : nullptr;
    G.excl_pod = g.xp.as<int32_t>();
    G.excl_time = g.xt.as<int64_t>();
    G.explicit_pool = g.ex.as<int32_t>();
    G.outs = g.go.as<mmp_gate_out>();
    G.done = done;
    return G;
}
// the serve half beside them: it shares the guards' exclusion pairs
ServeArgs serve_args(mmp_ctx *c, int32_t n, int64_t now, const GateArgs &G, const SeamIo *full_rows, const SeamIo &cnt, const SeamIo &so)
{
    ServeArgs S = serve_args(c, n, now);
    S.reqs = full_rows ? full_rows->as<mmp_serve_req>() : nullptr;
    S.counters = cnt.as<mmp_serve_counter>();
    S.excl_pod = G.excl_pod;
    S.excl_time = G.excl_time;
    S.outs = so.as<mmp_serve_out>();
    return S;
}

// Compact rows written out in full (the header's rule; gate and serve rows: expand_gate / expand_serve, seam_caller_kernels.hpp —
// one statement for host and device).  unnamed: with model = -1, for a resolver to name on the device.
mmp_place_req full_place_row(const mmp_place_caller &c, const mmp_place_req_c &q)
{
    mmp_place_req r;
    r.model = q.model;
    r.self_pod = c.self_pod;
    r.flags = c.flags;
    r.pick = q.pick;
    r.last_used = q.last_used;
    r.extra_off = q.extra_off;
    r.n_extra = q.n_extra;
    r.fresh_lru = c.fresh_lru;
    r.fresh_capacity = c.fresh_capacity;
    r.fresh_used = c.fresh_used;
    r.fresh_count = c.fresh_count;
    r.fresh_rpm = c.fresh_rpm;
    return r;
}
std::vector<mmp_place_req> full_place_rows(const mmp_place_caller &caller, const mmp_place_req_c *reqs, int32_t n, bool unnamed)
{
    std::vector<mmp_place_req> full((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        full[(size_t)i] = full_place_row(caller, reqs[i]);
        if (unnamed) full[(size_t)i].model = -1;
    }
    return full;
}
std::vector<mmp_gate_req> full_gate_rows(const mmp_seam_caller &caller, const mmp_gate_req_c *greqs, int32_t n, bool unnamed)
{
    std::vector<mmp_gate_req> full((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        full[(size_t)i] = expand_gate(caller, greqs[i]);
        if (unnamed) full[(size_t)i].model = -1;
    }
    return full;
}
std::vector<mmp_serve_req> full_serve_rows(const mmp_seam_caller &caller, const mmp_gate_req_c *greqs, const mmp_serve_req_c *sreqs, int32_t n,
                                           bool unnamed)
{
    std::vector<mmp_serve_req> full((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        full[(size_t)i] = expand_serve(caller, greqs[i], sreqs[i]);
        if (unnamed) full[(size_t)i].model = -1;
    }
    return full;
}

// The launches behind the registry's writes that more than one seam makes.
int launch_gate(mmp_ctx *c, hipStream_t st, const GateArgs &G, int32_t n)
{
    HIP_TRY(c, order_after_registry(c, st));
    hipLaunchKernelGGL(gate_batch_kernel, dim3(div_up(n, 256)), dim3(256), 0, st, G);
    HIP_TRY(c, hipGetLastError());
    return MMP_OK;
}
int launch_route(mmp_ctx *c, hipStream_t st, const GateArgs &G, const ServeArgs &S, int32_t n)
{
    HIP_TRY(c, order_after_registry(c, st));
    hipLaunchKernelGGL(route_batch_kernel, dim3(div_up(n, 256)), dim3(256), 0, st, G, S);
    HIP_TRY(c, hipGetLastError());
    return MMP_OK;
}
// on the compact rows: gq the mmp_gate_req_c, sq the mmp_serve_req_c
SeamCArgs seam_c_args(const mmp_seam_caller &caller, const SeamIo &gq, const SeamIo *sq, int32_t n)
{
    SeamCArgs R;
    R.greqs = gq.as<mmp_gate_req_c>();
    R.sreqs = sq ? sq->as<mmp_serve_req_c>() : nullptr;
    R.n = n;
    R.caller = caller;
    return R;
}
int launch_gate_c(mmp_ctx *c, hipStream_t st, const GateArgs &G, const mmp_seam_caller &caller, const SeamIo &gq, int32_t n)
{
    HIP_TRY(c, order_after_registry(c, st));
    hipLaunchKernelGGL(gate_batch_c_kernel, dim3(div_up(n, kSeamCBlock)), dim3(kSeamCBlock), 0, st, G, seam_c_args(caller, gq, nullptr, n));
    HIP_TRY(c, hipGetLastError());
    return MMP_OK;
}
int launch_route_c(mmp_ctx *c, hipStream_t st, const GateArgs &G, const ServeArgs &S, const mmp_seam_caller &caller, const SeamIo &gq,
                   const SeamIo &sq, int32_t n)
{
    HIP_TRY(c, order_after_registry(c, st));
    hipLaunchKernelGGL(route_batch_c_kernel, dim3(div_up(n, kSeamCBlock)), dim3(kSeamCBlock), 0, st, G, S, seam_c_args(caller, gq, &sq, n));
    HIP_TRY(c, hipGetLastError());
    return MMP_OK;
}
int place_launch_c(mmp_ctx *c, const mmp_place_caller *caller, const SeamIo &q, const SeamIo &x, const SeamIo &o, int32_t n, int64_t now,
                   hipStream_t st)
{
    PlaceCall call;
    call.caller = caller;
    return place_launch(c, q.dev, n, x.dev, now, o.dev, st, call);
}

// ---- the resolvers ---------------------------------------------------------------------------------------------------------------
// What a call by id has beyond the call it resolves in front of.  The id is resolved on the device inside the call: the resolver's
// kernel is enqueued in front of the unchanged decision kernels on the same stream and writes each request's row into the call's
// OWN copy of the request rows (its slot region, or its staged scratch: a KeyedPatch each), so the call waits once.  On a slot the
// state lock is held shared over the guard, the capture of the published tables and every enqueue (seam_slot), and batch_mu is
// never taken: the ownership rules at mmp_ctx::mid_hash and ::vid_hash are what make that capture safe.  Beyond the slot sizes the
// call is staged under batch_mu like every large call, on the compact rows.
//   check(c, fn, n)       what the call refuses in its own arguments, after the ranges: keys, then nf, then flag bits
//   fits<T>()             its byte counts are within tail T's kKeyBytes / kNfBytes
//   bind<At>(c, n, slot)  its arrays as SeamIos, on the regions of At (a tail of the layout table, or StagedTail)
//   ins() / outs()        those arrays, for seam_list
//   state(c, fn)          the state the call needs, looked at under the lock it launches under
//   launch(c, st, n, a, b) its one kernel, naming the model in up to two arrays of rows
constexpr KeyedPatch kNoPatch{nullptr, 0, 0};
template <class Row>  // the `model` field of an array of Row as the call holds it
KeyedPatch keyed_patch_of(const SeamIo &rows)
{
    return KeyedPatch{rows.as<char>(), (int32_t)sizeof(Row), (int32_t)offsetof(Row, model)};
}
struct StagedTail {
    static constexpr SlotRegion keys = kStagedOnly, key_off = kStagedOnly, nf = kStagedOnly, nf_off = kStagedOnly, flags = kStagedOnly,
                                idx = kStagedOnly, vm = kStagedOnly;
};
// The rows name their model themselves (the _c forms): nothing in front.
struct NoResolver {
    template <class At>
    void bind(mmp_ctx *, int32_t, bool) {}
    std::array<SeamIo *, 0> ins() { return {}; }
    std::array<SeamIo *, 0> outs() { return {}; }
    int state(mmp_ctx *c, const char *) const { return need_snapshot(c, true); }
    int launch(mmp_ctx *, hipStream_t, int32_t, const KeyedPatch &, const KeyedPatch &) const { return MMP_OK; }
};
int keyed_state(mmp_ctx *c, const char *fn)
{
    if (const int rc = need_snapshot(c, true)) return rc;
    return model_id_space_guard(c, fn);
}
int keyed_empty(mmp_ctx *c, const char *fn)  // n == 0: answered from the state
{
    std::shared_lock<std::shared_mutex> g(c->mu);
    return keyed_state(c, fn);
}
// n byte spans (`what`: "key " / "nf ") as n + 1 offsets into `bytes`: the offsets, the 2^31 bound, the bytes being there
int check_spans(mmp_ctx *c, const char *fn, const char *what, const char *bytes, const int32_t *off, int32_t n, int32_t &n_bytes)
{
    if (const int rc = check_offsets(c, fn, what, off, n)) return rc;
    const int64_t b = (int64_t)off[n] - off[0];
    if (b > INT32_MAX - kKeyedPad) return fail(c, MMP_EINVAL, "%s: more than 2^31 %sbytes", fn, what);
    if (b > 0 && !bytes) return fail(c, MMP_EINVAL, "%s: bad argument", fn);
    n_bytes = (int32_t)b;
    return MMP_OK;
}
// n byte spans of a call as the resolving kernels take them: the bytes and their n + 1 offsets as the caller gave them.  On a slot
// the bytes are copied as they are (the layouts leave kKeyedPad bytes behind them); staged, from a copy that carries the padding.
struct KeyedSpans {
    std::vector<char> padded;
    SeamIo kb, ko;
    void bind(const char *keys, const int32_t *key_off, int32_t n, int32_t key_bytes, bool on_slot, const SlotRegion &keys_at,
              const SlotRegion &off_at, DevBuf &bytes_stage, DevBuf &off_stage)
    {
        const char *first = key_bytes > 0 ? keys + key_off[0] : nullptr;
        if (!on_slot) {
            padded.assign((size_t)key_bytes + kKeyedPad, 0);
            if (key_bytes > 0) memcpy(padded.data(), first, (size_t)key_bytes);
            kb = seam_io(padded.data(), key_bytes + kKeyedPad, keys_at, bytes_stage);
        } else
            kb = seam_io(first, key_bytes, keys_at, bytes_stage);
        ko = seam_io(key_off, n + 1, off_at, off_stage);
    }
};
// The keys of a call by id (model ids and vmodel ids alike) as the call brings them: checked, and carried through kq_keys / kq_off.
struct KeyArg {
    const char *keys;
    const int32_t *key_off;
    int32_t bytes = 0;
    KeyedSpans io;
    int check(mmp_ctx *c, const char *fn, int32_t n)
    {
        if (n == 0) return MMP_OK;
        if (!key_off) return fail(c, MMP_EINVAL, "%s: bad argument", fn);
        return check_spans(c, fn, "key ", keys, key_off, n, bytes);
    }
    template <class At>
    void bind(mmp_ctx *c, int32_t n, bool on_slot)
    {
        io.bind(keys, key_off, n, bytes, on_slot, At::keys, At::key_off, c->kq_keys, c->kq_off);
    }
};
// By model id: the key bytes and their offsets in, the resolved rows out.  A NULL model_idx_out gets a sink: the kernel writes the
// rows either way.
struct ByModelId {
    template <const SlotRegion &req_end, const SlotRegion &out_end>
    using Tail = KeyTail<req_end, out_end>;
    KeyArg key;  // (the call's arguments)
    int32_t *model_idx_out;
    std::vector<int32_t> sink;
    SeamIo ix;
    int check(mmp_ctx *c, const char *fn, int32_t n) { return key.check(c, fn, n); }
    template <class T>
    bool fits() const { return key.bytes <= T::kKeyBytes; }
    template <class At>
    void bind(mmp_ctx *c, int32_t n, bool on_slot)
    {
        key.template bind<At>(c, n, on_slot);
        if (!model_idx_out) {
            sink.resize((size_t)n);
            model_idx_out = sink.data();
        }
        ix = seam_io(model_idx_out, n, At::idx, c->kq_idx);
    }
    std::array<SeamIo *, 2> ins() { return {&key.io.kb, &key.io.ko}; }
    std::array<SeamIo *, 1> outs() { return {&ix}; }
    int state(mmp_ctx *c, const char *fn) const { return keyed_state(c, fn); }
    // (called with the state lock held, or by the owner of batch_mu under which no writer of the id table runs)
    int launch(mmp_ctx *c, hipStream_t st, int32_t n, const KeyedPatch &a, const KeyedPatch &b) const
    {
        KeyedArgs A;
        A.keys = key.io.kb.as<char>();
        A.off = key.io.ko.as<int32_t>();
        A.n = n;
        A.hmask = hash_mask(c->tune.model_id_hash_bits);
        A.tab = model_id_tab(c).published();
        A.model_idx = ix.as<int32_t>();
        A.a = a;
        A.b = b;
        hipLaunchKernelGGL(keyed_resolve_kernel, dim3(div_up(n, kIdTabBlock)), dim3(kIdTabBlock), 0, st, A);
        HIP_TRY(c, hipGetLastError());
        return MMP_OK;
    }
};
// By vmodel id: resolveVModelId and the lookup of the id it returns.  Beyond the model-id form it takes the notFoundModelId spans and
// the flags in and gives an mmp_vseam_row per request.  The kernel takes all of them, so what the caller left out is supplied here: no
// nf is n + 1 equal offsets, no flags n zero words, a NULL vm_out a sink.
struct ByVModelId {
    template <const SlotRegion &req_end, const SlotRegion &out_end>
    using Tail = VKeyTail<req_end, out_end>;
    KeyArg key;  // (the call's arguments)
    const char *nf_keys;
    const int32_t *nf_off;
    const uint32_t *req_flags;
    mmp_vseam_row *vm_out;
    int32_t nf_bytes = 0;
    std::vector<int32_t> no_nf;
    std::vector<uint32_t> no_flags;
    std::vector<mmp_vseam_row> sink;
    KeyedSpans nf;
    SeamIo fl, vo;
    int check(mmp_ctx *c, const char *fn, int32_t n)
    {
        if (const int rc = key.check(c, fn, n)) return rc;
        if (n > 0 && nf_off)
            if (const int rc = check_spans(c, fn, "nf ", nf_keys, nf_off, n, nf_bytes)) return rc;
        if (req_flags)
            for (int32_t i = 0; i < n; i++)
                if (req_flags[i] & ~MMP_VMRQ_AFTER_STRONG) return fail(c, MMP_EINVAL, "%s: request %d has unknown flag bits", fn, i);
        return MMP_OK;
    }
    template <class T>
    bool fits() const { return key.bytes <= T::kKeyBytes && nf_bytes <= T::kNfBytes; }
    template <class At>
    void bind(mmp_ctx *c, int32_t n, bool on_slot)
    {
        key.template bind<At>(c, n, on_slot);
        if (!nf_off) {
            no_nf.assign((size_t)n + 1, 0);
            nf_off = no_nf.data();
        }
        nf.bind(nf_keys, nf_off, n, nf_bytes, on_slot, At::nf, At::nf_off, c->vq_nf, c->vq_nf_off);
        if (!req_flags) {
            no_flags.assign((size_t)n, 0u);
            req_flags = no_flags.data();
        }
        fl = seam_io(req_flags, n, At::flags, c->vq_flags);
        if (!vm_out) {
            sink.resize((size_t)n);
            vm_out = sink.data();
        }
        vo = seam_io(vm_out, n, At::vm, c->vq_out);
    }
    std::array<SeamIo *, 5> ins() { return {&key.io.kb, &key.io.ko, &nf.kb, &nf.ko, &fl}; }
    std::array<SeamIo *, 1> outs() { return {&vo}; }
    int state(mmp_ctx *c, const char *fn) const { return keyed_state(c, fn); }
    // (called with the state lock held, or by the owner of batch_mu under which no writer of either table runs)
    int launch(mmp_ctx *c, hipStream_t st, int32_t n, const KeyedPatch &a, const KeyedPatch &b) const
    {
        VKeyedArgs A;
        A.keys = key.io.kb.as<char>();
        A.off = key.io.ko.as<int32_t>();
        A.nf = nf.kb.as<char>();
        A.nf_off = nf.ko.as<int32_t>();
        A.flags = fl.as<uint32_t>();
        A.n = n;
        A.hmask = hash_mask(c->tune.vmodel_id_hash_bits);
        A.V = vmodel_tab(c);
        A.models = model_id_tab(c).published();
        A.n_models = c->n_models;
        A.out = vo.as<mmp_vseam_row>();
        A.a = a;
        A.b = b;
        hipLaunchKernelGGL(vkeyed_resolve_kernel, dim3(div_up(n, kIdTabBlock)), dim3(kIdTabBlock), 0, st, A);
        HIP_TRY(c, hipGetLastError());
        return MMP_OK;
    }
};

// ---- the seams on the compact rows, resolver K in front ----------------------------------------------------------------------------
// The staged load target and the staged route: what mmp_place_batch_c / mmp_route_batch_c do beyond the slot sizes (NoResolver) and
// what the forms by id do there.  The arrays stage through the scratch of the row forms: the calls never overlap, batch_mu owns it
// for a call.
template <class R>
int place_c_staged(mmp_ctx *c, const char *fn, R &K, const mmp_place_caller *caller, const mmp_place_req_c *reqs, int32_t n,
                   const int32_t *extra_pool, int32_t n_extra, int64_t now, mmp_place_out *outs)
{
    K.template bind<StagedTail>(c, n, false);
    SeamIo q = seam_io(reqs, n, kStagedOnly, c->s_reqs), x = seam_io(extra_pool, n_extra, kStagedOnly, c->s_extra),
           o = seam_io(outs, n, kStagedOnly, c->s_outs);
    return seam_run<true>(c, n, false, seam_list(K.ins(), &q, &x), seam_list(K.outs(), &o), [&] { return K.state(c, fn); },
                    [&](hipStream_t st, const DoneFlag &, auto) {
                        if (const int rc = K.launch(c, st, n, keyed_patch_of<mmp_place_req_c>(q), kNoPatch)) return rc;
                        return place_launch_c(c, caller, q, x, o, n, now, st);
                    });
}
template <class R>
int route_c_staged(mmp_ctx *c, const char *fn, R &K, const mmp_seam_caller *caller, const mmp_gate_req_c *greqs, const mmp_serve_req_c *sreqs,
                   int32_t n, const mmp_serve_counter *counters, int32_t n_counters, const GatePools &P, int64_t now, int64_t in_use_expiry,
                   mmp_gate_out *gouts, mmp_serve_out *souts)
{
    K.template bind<StagedTail>(c, n, false);
    GateIo g = gate_io<StagedRows>(c, P, gouts, n);
    SeamIo gq = seam_io(greqs, n, kStagedOnly, c->s_reqs), sq = seam_io(sreqs, n, kStagedOnly, c->rt_sreqs),
           cnt = seam_io(counters, n_counters, kStagedOnly, c->rt_cnt), so = seam_io(souts, n, kStagedOnly, c->rt_souts);
    return seam_run<false>(c, n, false, seam_list(K.ins(), &gq, &sq, &cnt, &g.xp, &g.xt, &g.ex), seam_list(K.outs(), &g.go, &so),
                    [&] { return K.state(c, fn); },
                    [&](hipStream_t st, const DoneFlag &done, auto) {
                        const GateArgs G = gate_args(c, n, now, in_use_expiry, g, nullptr, done);
                        const ServeArgs S = serve_args(c, n, now, G, nullptr, cnt, so);
                        // (the compact serve row has no model of its own: the serve half reads the gate row's)
                        if (const int rc = K.launch(c, st, n, keyed_patch_of<mmp_gate_req_c>(gq), kNoPatch)) return rc;
                        return launch_route_c(c, st, G, S, *caller, gq, sq, n);
                    });
}

// The three seams by id.  Within the slot sizes: the rows written out in full with model = -1, as the _c forms write them out, the
// resolver's launch, then the ROW kernels — a lone request takes them too, its model is not known at launch.  Beyond: staged on the
// compact rows.  Inlined into their entry points, one instance each.
template <class R>
__attribute__((always_inline)) inline int keyed_place(mmp_ctx *c, const char *fn, R &K, const mmp_place_caller *caller,
                                                      const mmp_place_req_c *reqs, int32_t n, const int32_t *extra_pool, int32_t n_extra,
                                                      int64_t now, mmp_place_out *outs)
{
    if (const int rc = check_place_call(c, fn, caller != nullptr, reqs, n, extra_pool, n_extra, outs)) return rc;
    if (const int rc = K.check(c, fn, n)) return rc;
    if (n == 0) return keyed_empty(c, fn);
    using L = KeyedPlaceSlot<R::template Tail>;
    if (!(n <= L::kN && n_extra <= L::kExtra && K.template fits<typename L::T>()))
        return place_c_staged(c, fn, K, caller, reqs, n, extra_pool, n_extra, now, outs);
    K.template bind<typename L::T>(c, n, true);
    const std::vector<mmp_place_req> full = full_place_rows(*caller, reqs, n, true);
    SeamIo q = seam_io(full.data(), n, L::reqs), x = seam_io(extra_pool, n_extra, L::extra), o = seam_io(outs, n, L::outs);
    return seam_run<true>(c, n, true, seam_list(K.ins(), &q, &x), seam_list(K.outs(), &o), [&] { return K.state(c, fn); },
                    [&](hipStream_t st, const DoneFlag &done, auto) {
                        if (const int rc = K.launch(c, st, n, keyed_patch_of<mmp_place_req>(q), kNoPatch)) return rc;
                        return place_launch(c, q.dev, n, x.dev, now, o.dev, st, slot_call(done, nullptr));
                    });
}
template <class R>
__attribute__((always_inline)) inline int keyed_route(mmp_ctx *c, const char *fn, R &K, const mmp_seam_caller *caller,
                                                      const mmp_gate_req_c *greqs, const mmp_serve_req_c *sreqs, int32_t n,
                                                      const mmp_serve_counter *counters, int32_t n_counters, const GatePools &P, int64_t now,
                                                      int64_t in_use_expiry, mmp_gate_out *gouts, mmp_serve_out *souts)
{
    if (const int rc = check_route_call(c, fn, caller != nullptr, greqs, sreqs, n, counters, n_counters, P, gouts, souts)) return rc;
    if (const int rc = K.check(c, fn, n)) return rc;
    if (n == 0) return keyed_empty(c, fn);
    using KL = KeyedRouteSlot<R::template Tail>;
    using L = RouteSlot;
    if (!(n <= KL::kN && route_slot_sized(n, n_counters, P) && K.template fits<typename KL::T>()))
        return route_c_staged(c, fn, K, caller, greqs, sreqs, n, counters, n_counters, P, now, in_use_expiry, gouts, souts);
    K.template bind<typename KL::T>(c, n, true);
    const std::vector<mmp_gate_req> fg = full_gate_rows(*caller, greqs, n, true);
    const std::vector<mmp_serve_req> fs = full_serve_rows(*caller, greqs, sreqs, n, true);
    GateIo g = gate_io<L>(c, P, gouts, n);
    SeamIo gq = seam_io(fg.data(), n, L::greqs), sq = seam_io(fs.data(), n, L::sreqs), cnt = seam_io(counters, n_counters, L::counters),
           so = seam_io(souts, n, L::souts);
    return seam_run<false>(c, n, true, seam_list(K.ins(), &gq, &sq, &cnt, &g.xp, &g.xt, &g.ex), seam_list(K.outs(), &g.go, &so),
                    [&] { return K.state(c, fn); },
                    [&](hipStream_t st, const DoneFlag &done, auto) {
                        const GateArgs G = gate_args(c, n, now, in_use_expiry, g, &gq, done);
                        const ServeArgs S = serve_args(c, n, now, G, &sq, cnt, so);
                        if (const int rc = K.launch(c, st, n, keyed_patch_of<mmp_gate_req>(gq), keyed_patch_of<mmp_serve_req>(sq))) return rc;
                        return launch_route(c, st, G, S, n);
                    });
}
// The miss: on a slot THREE launches on its stream (the resolver, the guards, the load targets: the last one's completion flag covers
// all), one wait; beyond, both halves staged in ONE hold of batch_mu (one resolution names both halves' rows), the load-target half
// through buffers of its own (kq_preqs, kq_pouts).
template <class R>
__attribute__((always_inline)) inline int keyed_miss(mmp_ctx *c, const char *fn, R &K, const mmp_seam_caller *caller,
                                                     const mmp_place_caller *pcaller, const mmp_gate_req_c *greqs, const mmp_place_req_c *preqs,
                                                     int32_t n, const GatePools &P, const int32_t *extra_pool, int32_t n_extra, int64_t now,
                                                     int64_t in_use_expiry, mmp_gate_out *gouts, mmp_place_out *pouts)
{
    if (const int rc = check_miss_call(c, fn, caller && pcaller, false, greqs, preqs, n, P, extra_pool, n_extra, gouts, pouts)) return rc;
    if (const int rc = K.check(c, fn, n)) return rc;
    if (n == 0) return keyed_empty(c, fn);
    using KL = KeyedMissSlot<R::template Tail>;
    using L = MissSlot;
    GateIo g = gate_io<L>(c, P, gouts, n);
    SeamIo x = seam_io(extra_pool, n_extra, L::extra, c->s_extra), po = seam_io(pouts, n, L::pouts, c->kq_pouts);
    if (n <= KL::kN && miss_slot_sized(n, n_extra, P) && K.template fits<typename KL::T>()) {
        K.template bind<typename KL::T>(c, n, true);
        const std::vector<mmp_gate_req> fg = full_gate_rows(*caller, greqs, n, true);
        const std::vector<mmp_place_req> fp = full_place_rows(*pcaller, preqs, n, true);
        SeamIo pq = seam_io(fp.data(), n, L::preqs), gq = seam_io(fg.data(), n, L::greqs);
        return seam_run<true>(c, n, true, seam_list(K.ins(), &pq, &gq, &x, &g.xp, &g.xt, &g.ex), seam_list(K.outs(), &po, &g.go),
                        [&] { return K.state(c, fn); },
                        [&](hipStream_t st, const DoneFlag &done, auto) {
                            const GateArgs G = gate_args(c, n, now, in_use_expiry, g, &gq, kNoDone);
                            if (const int rc = K.launch(c, st, n, keyed_patch_of<mmp_gate_req>(gq), keyed_patch_of<mmp_place_req>(pq))) return rc;
                            if (const int rc = launch_gate(c, st, G, n)) return rc;
                            return place_launch(c, pq.dev, n, x.dev, now, po.dev, st, slot_call(done, nullptr));
                        });
    }
    K.template bind<StagedTail>(c, n, false);
    SeamIo gq = seam_io(greqs, n, kStagedOnly, c->s_reqs), pq = seam_io(preqs, n, kStagedOnly, c->kq_preqs);
    return seam_run<true>(c, n, false, seam_list(K.ins(), &pq, &gq, &x, &g.xp, &g.xt, &g.ex), seam_list(K.outs(), &po, &g.go),
                    [&] { return K.state(c, fn); },
                    [&](hipStream_t st, const DoneFlag &done, auto) {
                        const GateArgs G = gate_args(c, n, now, in_use_expiry, g, nullptr, done);
                        if (const int rc = K.launch(c, st, n, keyed_patch_of<mmp_gate_req_c>(gq), keyed_patch_of<mmp_place_req_c>(pq))) return rc;
                        if (const int rc = launch_gate_c(c, st, G, *caller, gq, n)) return rc;
                        return place_launch_c(c, pcaller, pq, x, po, n, now, st);
                    });
}
}  // namespace
}  // extern "C++"

int mmp_place_batch_c(mmp_ctx *c, const mmp_place_caller *caller, const mmp_place_req_c *reqs, int32_t n, const int32_t *extra_pool,
                      int32_t n_extra, int64_t now, mmp_place_out *outs)
try {
    const char *fn = "mmp_place_batch_c";
    if (const int rc = check_place_call(c, fn, caller != nullptr, reqs, n, extra_pool, n_extra, outs)) return rc;
    // a handful of requests: the latency path of mmp_place_batch (slots, the single-decision kernels, the resident kernel) on the same
    // decisions written out as mmp_place_req rows
    if (n <= PlaceSlot::kN && n_extra <= PlaceSlot::kExtra)
        return mmp_place_batch(c, full_place_rows(*caller, reqs, n, false).data(), n, extra_pool, n_extra, now, outs);
    NoResolver K;
    return place_c_staged(c, fn, K, caller, reqs, n, extra_pool, n_extra, now, outs);
} MMP_CATCH(c, "mmp_place_batch_c")

int mmp_place_batch(mmp_ctx *c, const mmp_place_req *reqs, int32_t n, const int32_t *extra_pool, int32_t n_extra,
                    int64_t now, mmp_place_out *outs)
try {
    if (const int rc = check_place_call(c, "mmp_place_batch", true, reqs, n, extra_pool, n_extra, outs)) return rc;
    if (n == 0) {
        std::lock_guard<std::shared_mutex> g(c->mu);
        return need_snapshot(c, true);
    }
    const bool lone = n == 1 && reqs[0].n_extra == 0;  // a single request without exclusions of its own
    if (lone && c->res.enabled && now >= 0 && (now >> kResidentNowBits) == 0) {
        // the resident kernel, no launch at all
        HIP_TRY(c, hipSetDevice(c->cfg.device));
        const int rc = resident_place(c, reqs[0], now, outs);
        if (rc != kResidentFallback) return rc;
    }
    SeamIo q = seam_io(reqs, n, PlaceSlot::reqs, c->s_reqs), x = seam_io(extra_pool, n_extra, PlaceSlot::extra, c->s_extra),
           o = seam_io(outs, n, PlaceSlot::outs, c->s_outs);
    return seam_run<true>(c, n, n <= PlaceSlot::kN && n_extra <= PlaceSlot::kExtra, {&q, &x}, {&o}, [&] { return need_snapshot(c, true); },
                    [&](hipStream_t st, const DoneFlag &done, auto on_slot) {
                        // (on a slot a lone request rides in the kernel arguments)
                        return place_launch(c, q.dev, n, x.dev, now, o.dev, st, slot_call(done, on_slot && lone ? &reqs[0] : nullptr));
                    });
} MMP_CATCH(c, "mmp_place_batch")

// What the LB's one call per request (MM.java:4315) needs: on a slot, one launch and the completion flag.
int mmp_serve_batch(mmp_ctx *c, const mmp_serve_req *reqs, int32_t n, const mmp_serve_counter *counters, int32_t n_counters,
                    const int32_t *excl_pod, const int64_t *excl_time, int32_t n_excl, int64_t now, mmp_serve_out *outs)
try {
    if (!c || n < 0 || n_excl < 0 || n_counters < 0 || (n > 0 && (!reqs || !outs)) || (n_counters > 0 && !counters) ||
        (n_excl > 0 && (!excl_pod || !excl_time)))
        return fail(c, MMP_EINVAL, "mmp_serve_batch: bad argument");
    for (int32_t i = 0; i < n; i++)
        if (const int rc = check_serve_req(c, "mmp_serve_batch", i, reqs[i], n_excl, n_counters)) return rc;
    using L = ServeSlot;
    SeamIo q = seam_io(reqs, n, L::reqs, c->s_reqs), cnt = seam_io(counters, n_counters, L::counters, c->s_a),
           xp = seam_io(excl_pod, n_excl, L::excl_pod, c->s_c), xt = seam_io(excl_time, n_excl, L::excl_time, c->s_d),
           o = seam_io(outs, n, L::outs, c->s_outs);
    return seam_run<false>(c, n, n > 0 && n <= L::kN && n_counters <= L::kCounters && n_excl <= L::kExcl, {&q, &cnt, &xp, &xt}, {&o},
                    [&] { return need_snapshot(c, false); },
                    [&](hipStream_t st, const DoneFlag &done, auto on_slot) {
                        ServeArgs A = serve_args(c, n, now);
                        A.reqs = q.as<mmp_serve_req>();
                        A.counters = cnt.as<mmp_serve_counter>();
                        A.excl_pod = xp.as<int32_t>();
                        A.excl_time = xt.as<int64_t>();
                        A.outs = o.as<mmp_serve_out>();
                        A.done = done;
                        HIP_TRY(c, order_after_registry(c, st));
                        hipLaunchKernelGGL(serve_batch_kernel, dim3(div_up(n, 256)), dim3(256), 0, st, A);
                        HIP_TRY(c, hipGetLastError());
                        return MMP_OK;
                    });
} MMP_CATCH(c, "mmp_serve_batch")

int mmp_gate_batch(mmp_ctx *c, const mmp_gate_req *reqs, int32_t n, const int32_t *excl_pod, const int64_t *excl_time,
                   int32_t n_excl, const int32_t *explicit_pool, int32_t n_explicit, int64_t now, int64_t in_use_expiry,
                   mmp_gate_out *outs)
try {
    const GatePools P{excl_pod, excl_time, n_excl, explicit_pool, n_explicit};
    if (!c || n < 0 || P.bad() || (n > 0 && (!reqs || !outs))) return fail(c, MMP_EINVAL, "mmp_gate_batch: bad argument");
    for (int32_t i = 0; i < n; i++)
        if (const int rc = check_gate_req(c, "mmp_gate_batch", i, reqs[i], n_excl, n_explicit)) return rc;
    using L = GateSlot;
    GateIo g = gate_io<L>(c, P, outs, n);
    SeamIo q = seam_io(reqs, n, L::reqs, c->s_reqs);
    return seam_run<false>(c, n, n > 0 && n <= L::kN && n_excl <= L::kExcl && n_explicit <= L::kExplicit, {&q, &g.xp, &g.xt, &g.ex}, {&g.go},
                    [&] { return need_snapshot(c, false); },
                    [&](hipStream_t st, const DoneFlag &done, auto) {
                        return launch_gate(c, st, gate_args(c, n, now, in_use_expiry, g, &q, done), n);
                    });
} MMP_CATCH(c, "mmp_gate_batch")

int mmp_miss_batch(mmp_ctx *c, const mmp_gate_req *greqs, const mmp_place_req *preqs, int32_t n, const int32_t *excl_pod,
                   const int64_t *excl_time, int32_t n_excl, const int32_t *explicit_pool, int32_t n_explicit, const int32_t *extra_pool,
                   int32_t n_extra, int64_t now, int64_t in_use_expiry, mmp_gate_out *gouts, mmp_place_out *pouts)
try {
    const GatePools P{excl_pod, excl_time, n_excl, explicit_pool, n_explicit};
    if (const int rc = check_miss_call(c, "mmp_miss_batch", true, true, greqs, preqs, n, P, extra_pool, n_extra, gouts, pouts)) return rc;
    if (n == 0) return MMP_OK;
    using L = MissSlot;
    if (!miss_slot_sized(n, n_extra, P)) {  // large batches: the two calls
        const int rc = mmp_gate_batch(c, greqs, n, excl_pod, excl_time, n_excl, explicit_pool, n_explicit, now, in_use_expiry, gouts);
        return rc != MMP_OK ? rc : mmp_place_batch(c, preqs, n, extra_pool, n_extra, now, pouts);
    }
    // One latency slot, TWO launches on its stream (the guards, then the load targets: in stream order, so the second kernel's
    // completion flag covers both), ONE wait: what two calls did in two launch-wait-return round trips.  Always on a slot: the staged
    // path is the two calls above.
    GateIo g = gate_io<L>(c, P, gouts, n);
    SeamIo pq = seam_io(preqs, n, L::preqs), gq = seam_io(greqs, n, L::greqs), x = seam_io(extra_pool, n_extra, L::extra),
           po = seam_io(pouts, n, L::pouts);
    return seam_run<false>(c, n, true, {&pq, &gq, &x, &g.xp, &g.xt, &g.ex}, {&po, &g.go}, [&] { return need_snapshot(c, true); },
                    [&](hipStream_t st, const DoneFlag &done, auto) {
                        const GateArgs G = gate_args(c, n, now, in_use_expiry, g, &gq, kNoDone);
                        if (n == 1 && preqs[0].n_extra == 0) {  // ONE launch: both requests in the kernel arguments, guards and load target on two wavefronts
                            PlaceCall call = slot_call(done, &preqs[0]);
                            call.fused_gate = &G;
                            call.fused_greq = &greqs[0];
                            return place_launch(c, pq.dev, n, x.dev, now, po.dev, st, call);
                        }
                        if (const int rc = launch_gate(c, st, G, n)) return rc;
                        return place_launch(c, pq.dev, n, x.dev, now, po.dev, st, slot_call(done, nullptr));
                    });
} MMP_CATCH(c, "mmp_miss_batch")

// The per-request seam (invokeModel asks for ONE route at a time): the guards and the serve target of every request in one launch.
int mmp_route_batch(mmp_ctx *c, const mmp_gate_req *greqs, const mmp_serve_req *sreqs, int32_t n, const mmp_serve_counter *counters,
                    int32_t n_counters, const int32_t *excl_pod, const int64_t *excl_time, int32_t n_excl,
                    const int32_t *explicit_pool, int32_t n_explicit, int64_t now, int64_t in_use_expiry, mmp_gate_out *gouts,
                    mmp_serve_out *souts)
try {
    const GatePools P{excl_pod, excl_time, n_excl, explicit_pool, n_explicit};
    if (const int rc = check_route_call(c, "mmp_route_batch", true, greqs, sreqs, n, counters, n_counters, P, gouts, souts)) return rc;
    using L = RouteSlot;
    // (staged, the gate half takes the scratch mmp_gate_batch takes, the serve half buffers of its own)
    GateIo g = gate_io<L>(c, P, gouts, n);
    SeamIo gq = seam_io(greqs, n, L::greqs, c->s_reqs), sq = seam_io(sreqs, n, L::sreqs, c->rt_sreqs),
           cnt = seam_io(counters, n_counters, L::counters, c->rt_cnt), so = seam_io(souts, n, L::souts, c->rt_souts);
    return seam_run<false>(c, n, n > 0 && route_slot_sized(n, n_counters, P), {&gq, &sq, &cnt, &g.xp, &g.xt, &g.ex}, {&g.go, &so},
                    [&] { return need_snapshot(c, true); },
                    [&](hipStream_t st, const DoneFlag &done, auto on_slot) {
                        const GateArgs G = gate_args(c, n, now, in_use_expiry, g, &gq, done);
                        const ServeArgs S = serve_args(c, n, now, G, &sq, cnt, so);
                        if (!(on_slot && n == 1 && n_counters <= kRouteInlineCnt && sreqs[0].n_cnt <= kRouteInlineCnt))
                            return launch_route(c, st, G, S, n);
                        // ONE route on a slot: the requests ride in the kernel arguments
                        RouteInline R{};
                        R.g = greqs[0];
                        R.s = sreqs[0];
                        for (int32_t j = 0; j < sreqs[0].n_cnt; j++) R.cnt[j] = counters[sreqs[0].cnt_off + j];
                        HIP_TRY(c, order_after_registry(c, st));
                        hipLaunchKernelGGL(route_single_kernel, dim3(1), dim3(128), 0, st, G, S, R);
                        HIP_TRY(c, hipGetLastError());
                        return MMP_OK;
                    });
} MMP_CATCH(c, "mmp_route_batch")

// ---- the single-caller forms of the two routes: within the slot sizes the row forms on the rows written out ---------------------
int mmp_route_batch_c(mmp_ctx *c, const mmp_seam_caller *caller, const mmp_gate_req_c *greqs, const mmp_serve_req_c *sreqs, int32_t n,
                      const mmp_serve_counter *counters, int32_t n_counters, const int32_t *excl_pod, const int64_t *excl_time,
                      int32_t n_excl, const int32_t *explicit_pool, int32_t n_explicit, int64_t now, int64_t in_use_expiry,
                      mmp_gate_out *gouts, mmp_serve_out *souts)
try {
    const char *fn = "mmp_route_batch_c";
    const GatePools P{excl_pod, excl_time, n_excl, explicit_pool, n_explicit};
    if (const int rc = check_route_call(c, fn, caller != nullptr, greqs, sreqs, n, counters, n_counters, P, gouts, souts)) return rc;
    // within the latency slots' sizes (and n = 0): mmp_route_batch — its slots, its n = 1 kernel — on the rows written out
    if (route_slot_sized(n, n_counters, P))
        return mmp_route_batch(c, full_gate_rows(*caller, greqs, n, false).data(), full_serve_rows(*caller, greqs, sreqs, n, false).data(), n,
                               counters, n_counters, excl_pod, excl_time, n_excl, explicit_pool, n_explicit, now, in_use_expiry, gouts, souts);
    NoResolver K;
    return route_c_staged(c, fn, K, caller, greqs, sreqs, n, counters, n_counters, P, now, in_use_expiry, gouts, souts);
} MMP_CATCH(c, "mmp_route_batch_c")

int mmp_miss_batch_c(mmp_ctx *c, const mmp_seam_caller *caller, const mmp_place_caller *pcaller, const mmp_gate_req_c *greqs,
                     const mmp_place_req_c *preqs, int32_t n, const int32_t *excl_pod, const int64_t *excl_time, int32_t n_excl,
                     const int32_t *explicit_pool, int32_t n_explicit, const int32_t *extra_pool, int32_t n_extra, int64_t now,
                     int64_t in_use_expiry, mmp_gate_out *gouts, mmp_place_out *pouts)
try {
    const char *fn = "mmp_miss_batch_c";
    const GatePools P{excl_pod, excl_time, n_excl, explicit_pool, n_explicit};
    if (const int rc = check_miss_call(c, fn, caller && pcaller, true, greqs, preqs, n, P, extra_pool, n_extra, gouts, pouts)) return rc;
    // within the latency slot's sizes (and n = 0): mmp_miss_batch on the rows written out
    if (miss_slot_sized(n, n_extra, P))
        return mmp_miss_batch(c, full_gate_rows(*caller, greqs, n, false).data(), full_place_rows(*pcaller, preqs, n, false).data(), n,
                              excl_pod, excl_time, n_excl, explicit_pool, n_explicit, extra_pool, n_extra, now, in_use_expiry, gouts, pouts);
    // a large batch is two calls, as mmp_miss_batch's is: the guards on the compact rows, then the load targets where
    // mmp_place_batch_c has them
    GateIo g = gate_io<StagedRows>(c, P, gouts, n);
    SeamIo gq = seam_io(greqs, n, kStagedOnly, c->s_reqs);
    const int rc = seam_run<false>(c, n, false, {&gq, &g.xp, &g.xt, &g.ex}, {&g.go}, [&] { return need_snapshot(c, true); },
                    [&](hipStream_t st, const DoneFlag &done, auto) {
                        return launch_gate_c(c, st, gate_args(c, n, now, in_use_expiry, g, nullptr, done), *caller, gq, n);
                    });
    if (rc != MMP_OK) return rc;
    // (profiling: the call's device span is the sum of its two brackets; a load-target half that rides a slot leaves none.
    // last_kernel_ms belongs to batch_mu)
    double gate_ms = -1.0;
    {
        std::lock_guard<std::mutex> gb(c->batch_mu);
        if (c->prof) std::swap(gate_ms, c->last_kernel_ms);
    }
    const int rc2 = mmp_place_batch_c(c, pcaller, preqs, n, extra_pool, n_extra, now, pouts);
    if (gate_ms >= 0) {
        std::lock_guard<std::mutex> gb(c->batch_mu);
        if (c->prof) c->last_kernel_ms = c->last_kernel_ms >= 0 ? c->last_kernel_ms + gate_ms : gate_ms;
    }
    return rc2;
} MMP_CATCH(c, "mmp_miss_batch_c")

// ---- the request calls by model id and by vmodel id: an argument pack and the seam (keyed_place / keyed_route / keyed_miss) -----
int mmp_place_batch_ck(mmp_ctx *c, const mmp_place_caller *caller, const mmp_place_req_c *reqs, int32_t n, const char *keys,
                       const int32_t *key_off, const int32_t *extra_pool, int32_t n_extra, int64_t now, mmp_place_out *outs,
                       int32_t *model_idx_out)
try {
    ByModelId K{{keys, key_off}, model_idx_out};
    return keyed_place(c, "mmp_place_batch_ck", K, caller, reqs, n, extra_pool, n_extra, now, outs);
} MMP_CATCH(c, "mmp_place_batch_ck")

int mmp_route_batch_ck(mmp_ctx *c, const mmp_seam_caller *caller, const mmp_gate_req_c *greqs, const mmp_serve_req_c *sreqs, int32_t n,
                       const char *keys, const int32_t *key_off, const mmp_serve_counter *counters, int32_t n_counters,
                       const int32_t *excl_pod, const int64_t *excl_time, int32_t n_excl, const int32_t *explicit_pool, int32_t n_explicit,
                       int64_t now, int64_t in_use_expiry, mmp_gate_out *gouts, mmp_serve_out *souts, int32_t *model_idx_out)
try {
    ByModelId K{{keys, key_off}, model_idx_out};
    return keyed_route(c, "mmp_route_batch_ck", K, caller, greqs, sreqs, n, counters, n_counters,
                       GatePools{excl_pod, excl_time, n_excl, explicit_pool, n_explicit}, now, in_use_expiry, gouts, souts);
} MMP_CATCH(c, "mmp_route_batch_ck")

int mmp_miss_batch_ck(mmp_ctx *c, const mmp_seam_caller *caller, const mmp_place_caller *pcaller, const mmp_gate_req_c *greqs,
                      const mmp_place_req_c *preqs, int32_t n, const char *keys, const int32_t *key_off, const int32_t *excl_pod,
                      const int64_t *excl_time, int32_t n_excl, const int32_t *explicit_pool, int32_t n_explicit, const int32_t *extra_pool,
                      int32_t n_extra, int64_t now, int64_t in_use_expiry, mmp_gate_out *gouts, mmp_place_out *pouts, int32_t *model_idx_out)
try {
    ByModelId K{{keys, key_off}, model_idx_out};
    return keyed_miss(c, "mmp_miss_batch_ck", K, caller, pcaller, greqs, preqs, n, GatePools{excl_pod, excl_time, n_excl, explicit_pool, n_explicit},
                      extra_pool, n_extra, now, in_use_expiry, gouts, pouts);
} MMP_CATCH(c, "mmp_miss_batch_ck")

int mmp_place_batch_cv(mmp_ctx *c, const mmp_place_caller *caller, const mmp_place_req_c *reqs, int32_t n, const char *keys,
                       const int32_t *key_off, const char *nf_keys, const int32_t *nf_off, const uint32_t *req_flags,
                       const int32_t *extra_pool, int32_t n_extra, int64_t now, mmp_place_out *outs, mmp_vseam_row *vm_out)
try {
    ByVModelId K{{keys, key_off}, nf_keys, nf_off, req_flags, vm_out};
    return keyed_place(c, "mmp_place_batch_cv", K, caller, reqs, n, extra_pool, n_extra, now, outs);
} MMP_CATCH(c, "mmp_place_batch_cv")

int mmp_route_batch_cv(mmp_ctx *c, const mmp_seam_caller *caller, const mmp_gate_req_c *greqs, const mmp_serve_req_c *sreqs, int32_t n,
                       const char *keys, const int32_t *key_off, const char *nf_keys, const int32_t *nf_off, const uint32_t *req_flags,
                       const mmp_serve_counter *counters, int32_t n_counters, const int32_t *excl_pod, const int64_t *excl_time,
                       int32_t n_excl, const int32_t *explicit_pool, int32_t n_explicit, int64_t now, int64_t in_use_expiry,
                       mmp_gate_out *gouts, mmp_serve_out *souts, mmp_vseam_row *vm_out)
try {
    ByVModelId K{{keys, key_off}, nf_keys, nf_off, req_flags, vm_out};
    return keyed_route(c, "mmp_route_batch_cv", K, caller, greqs, sreqs, n, counters, n_counters,
                       GatePools{excl_pod, excl_time, n_excl, explicit_pool, n_explicit}, now, in_use_expiry, gouts, souts);
} MMP_CATCH(c, "mmp_route_batch_cv")

int mmp_miss_batch_cv(mmp_ctx *c, const mmp_seam_caller *caller, const mmp_place_caller *pcaller, const mmp_gate_req_c *greqs,
                      const mmp_place_req_c *preqs, int32_t n, const char *keys, const int32_t *key_off, const char *nf_keys,
                      const int32_t *nf_off, const uint32_t *req_flags, const int32_t *excl_pod, const int64_t *excl_time, int32_t n_excl,
                      const int32_t *explicit_pool, int32_t n_explicit, const int32_t *extra_pool, int32_t n_extra, int64_t now,
                      int64_t in_use_expiry, mmp_gate_out *gouts, mmp_place_out *pouts, mmp_vseam_row *vm_out)
try {
    ByVModelId K{{keys, key_off}, nf_keys, nf_off, req_flags, vm_out};
    return keyed_miss(c, "mmp_miss_batch_cv", K, caller, pcaller, greqs, preqs, n, GatePools{excl_pod, excl_time, n_excl, explicit_pool, n_explicit},
                      extra_pool, n_extra, now, in_use_expiry, gouts, pouts);
} MMP_CATCH(c, "mmp_miss_batch_cv")


int mmp_evict_batch(mmp_ctx *c, const mmp_evict_req *reqs, int32_t n, int64_t now, mmp_evict_out *outs)
try {
    if (!c || n < 0 || (n > 0 && (!reqs || !outs))) return fail(c, MMP_EINVAL, "mmp_evict_batch: bad argument");
    SeamIo q = seam_io(reqs, n, EvictSlot::reqs, c->s_reqs), o = seam_io(outs, n, EvictSlot::outs, c->s_outs);
    return seam_run<false>(c, n, n > 0 && n <= EvictSlot::kN, {&q}, {&o},
                    [&] { return n > 0 && c->n_caches <= 0 ? fail(c, MMP_ESTATE, "no caches loaded") : MMP_OK; },
                    [&](hipStream_t st, const DoneFlag &done, auto on_slot) {
                        EvictArgs A = evict_args(c, n, now);
                        A.reqs = q.as<mmp_evict_req>();
                        A.outs = o.as<mmp_evict_out>();
                        A.done = done;
                        evict_launch(c, A, n, st);
                        HIP_TRY(c, hipGetLastError());
                        return MMP_OK;
                    });
} MMP_CATCH(c, "mmp_evict_batch")

int mmp_proactive_plan(mmp_ctx *c, int32_t default_units, int64_t now, int32_t max_out, int32_t *out_model,
                       int64_t *out_last_used, mmp_proactive_info *info)
try {
    return mmp_proactive_plan_subset(c, -1, nullptr, 0, default_units, now, max_out, out_model, out_last_used, info);
} MMP_CATCH(c, "mmp_proactive_plan")

int mmp_proactive_plan_subset(mmp_ctx *c, int32_t partition, const int32_t *skip_models, int32_t n_skip, int32_t default_units,
                              int64_t now, int32_t max_out, int32_t *out_model, int64_t *out_last_used,
                              mmp_proactive_info *info)
try {
    if (!c || !info || max_out < 0 || n_skip < 0 || (n_skip > 0 && !skip_models) || (max_out > 0 && (!out_model || !out_last_used)))
        return fail(c, MMP_EINVAL, "mmp_proactive_plan: bad argument");
    // batch_mu owns c->stream and the scratch for the whole call, and every writer of the state this call reads
    // (commit, the loaders, registry events) takes it too: the published snapshot cannot change underneath.  The
    // state lock c->mu is NOT held: latency-path calls (mmp_place_batch / _gate / _evict on the slots) keep flowing.
    std::lock_guard<std::mutex> gb(c->batch_mu);
    if (!c->committed) return fail(c, MMP_ESTATE, "no committed snapshot");
    if (partition >= cur_side(c).n_pts || partition < -1) return fail(c, MMP_EINVAL, "mmp_proactive_plan: no partition %d", partition);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    const int32_t M = c->n_models, P = c->snap.P;
    const int nb = std::max(div_up(std::max(M, 1), kCompactBlock), 1);
    HIP_TRY(c, c->r_ps.ensure(sizeof(PlanScalars)));
    HIP_TRY(c, c->r_counts.ensure((size_t)(nb + 1) * 4));
    HIP_TRY(c, c->r_keys.ensure((size_t)std::max(M, 1) * 8));
    HIP_TRY(c, c->r_keys2.ensure((size_t)std::max(M, 1) * 8));
    HIP_TRY(c, c->r_vals.ensure((size_t)std::max(M, 1) * 4));
    HIP_TRY(c, c->r_vals2.ensure((size_t)std::max(M, 1) * 4));
    HIP_TRY(c, c->r_out_model.ensure((size_t)std::max(max_out, 1) * 4));
    HIP_TRY(c, c->r_out_lu.ensure((size_t)std::max(max_out, 1) * 8));
    PlanScalars *ps = c->r_ps.as<PlanScalars>();
    const StatsAcc *stats = cur_side(c).stats_acc.as<StatsAcc>();
    const mmp_pod_row *pods = c->sb[c->cur].pods.as<mmp_pod_row>();
    const mmp_model_row *models = c->models.as<mmp_model_row>();
    int32_t *counts = nullptr;
    HIP_TRY(c, hipMemsetAsync(ps, 0, sizeof(PlanScalars), st));
    PlanSubset U{};
    U.global = stats;
    U.stats = partition >= 0 ? cur_side(c).pstats.as<StatsAcc>() + partition : stats;
    U.pod_pts = cur_side(c).d_pts.as<int32_t>();
    U.prohib = partition >= 0 ? cur_side(c).d_prohib.as<uint64_t>() + (size_t)partition * cur_side(c).pts_tw : nullptr;
    U.skip = nullptr;
    U.pts = partition;
    U.n_types = c->n_types;
    if (n_skip > 0) {  // models already triggered for an earlier partition of this run
        std::vector<uint8_t> mask((size_t)std::max(M, 1), 0);
        for (int32_t i = 0; i < n_skip; i++)
            if (skip_models[i] >= 0 && skip_models[i] < M) mask[skip_models[i]] = 1;
        HIP_TRY(c, c->s_d.ensure(mask.size()));
        HIP_TRY(c, hipMemcpyAsync(c->s_d.p, mask.data(), mask.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipStreamSynchronize(st));  // `mask` leaves scope
        U.skip = c->s_d.as<uint8_t>();
    }
    // The bucketed plan: six dependent launches, every size read on the device, ONE read of the result at the end.
    const int32_t n_cnt_words = 3 * (kPlanBuckets + 1) + 3 * kPlanBuckets + 1;  // (even: the one-launch plan's chunk totals follow, 8 bytes each)
    static_assert((3 * (kPlanBuckets + 1) + 3 * kPlanBuckets + 1) % 2 == 0, "chunk totals are 8-byte aligned");
    HIP_TRY(c, c->r_counts.ensure((size_t)std::max(n_cnt_words + 2 * div_up(std::max(M, 1), kPlanFusedBlock), nb + 1) * 4));
    HIP_TRY(c, c->r_part.ensure((size_t)nb * std::max(sizeof(PlanPartial), (size_t)kPlanPartWords * 8)));
    counts = c->r_counts.as<int32_t>();
    int32_t *hist = counts, *dcnt = hist + kPlanBuckets, *dge = dcnt + kPlanBuckets, *off = dge + kPlanBuckets,
            *cur = off + kPlanBuckets + 1, *doff = cur + kPlanBuckets + 1;
    PlanPartial *part = c->r_part.as<PlanPartial>();
    KT_BEGIN(c, st);  // device span of the whole plan
    // The one-launch form prefetches registry / instance rows unconditionally and waits at grid-wide barriers: it needs a registry
    // and a table to read (an empty or never-loaded one takes the eight launches, which guard every access: ADVICE r5), and every
    // workgroup on the chip at once — plan_grid_max is what the occupancy query granted at mmp_create; a launch never asks for more
    const bool fused_ok = c->tune.plan_fused && c->plan_grid_max > 0 && M > 0 && P > 0 && models != nullptr && pods != nullptr;
    if (fused_ok) {
        // ONE launch, the steps separated by grid-wide barriers (rebalance_kernels.hpp: proactive_plan_fused_kernel)
        const int G = std::max(std::min(div_up(std::max(M, 1), kPlanFusedBlock), (int)c->plan_grid_max), 1);
        hipLaunchKernelGGL(proactive_plan_fused_kernel, dim3(G), dim3(kPlanFusedBlock), kPlanFusedLds, st, pods, P, models, M, U, default_units, now,
                           ps, c->r_part.as<uint64_t>(), hist, c->r_keys2.as<int32_t>(), c->r_keys.as<int64_t>(), c->r_vals.as<int32_t>(),
                           c->r_vals2.as<int32_t>(), reinterpret_cast<uint64_t *>(counts + n_cnt_words), max_out,
                           c->r_out_model.as<int32_t>(), c->r_out_lu.as<int64_t>());
    } else {
        hipLaunchKernelGGL(proactive_space_scalars_kernel, dim3(std::min(std::max(div_up(P, 256), 1), 512)), dim3(256), 0, st, pods, P,
                           U, default_units, now, ps);
        hipLaunchKernelGGL(proactive_qualify_kernel, dim3(nb), dim3(kCompactBlock), 0, st, models, M, U, ps, part, hist);
        hipLaunchKernelGGL(proactive_hist_kernel, dim3(nb), dim3(kCompactBlock), 0, st, models, M, U, ps, part, nb, hist);
        hipLaunchKernelGGL(proactive_scan_kernel, dim3(1), dim3(kPlanScanBlock), 0, st, ps, hist, off, cur);
        hipLaunchKernelGGL(proactive_bin_kernel, dim3(nb), dim3(kCompactBlock), 0, st, models, M, U, ps, cur, c->r_keys.as<int64_t>(),
                           c->r_vals.as<int32_t>());
        hipLaunchKernelGGL(proactive_bucket_rank_kernel, dim3(kPlanBuckets / 4), dim3(256), 0, st, c->r_keys.as<int64_t>(),
                           c->r_vals.as<int32_t>(), off, ps, c->r_vals2.as<int32_t>(), dcnt, dge);
        hipLaunchKernelGGL(proactive_scan2_kernel, dim3(1), dim3(kPlanScanBlock), 0, st, ps, dcnt, dge, doff);
        hipLaunchKernelGGL(proactive_emit_kernel, dim3(nb), dim3(kCompactBlock), 0, st, c->r_keys.as<int64_t>(), c->r_vals.as<int32_t>(),
                           c->r_vals2.as<int32_t>(), doff, ps, max_out, c->r_out_model.as<int32_t>(), c->r_out_lu.as<int64_t>());
    }
    KT_END(c, st);
    HIP_TRY(c, hipGetLastError());
    PlanScalars h{};
    HIP_TRY(c, hipMemcpyAsync(&h, ps, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    kt_collect(c);
    // (overflow == 2: the one-launch plan gave up at a grid barrier — its workgroups were not all on the chip; the general path below)
    if (h.overflow && c->tune.plan_sorted == 2) return fail(c, MMP_ESTATE, "mmp_proactive_plan: a key bucket overflowed and MMP_PLAN_SORTED=2 forbids the sorted path");
    if (!h.overflow && c->tune.plan_sorted != 1) {
        const int32_t n_copy = std::min(h.n_selected, max_out);
        if (n_copy > 0) {
            HIP_TRY(c, copy_sync(c, out_model, c->r_out_model.p, (size_t)n_copy * 4, hipMemcpyDeviceToHost));
            HIP_TRY(c, copy_sync(c, out_last_used, c->r_out_lu.p, (size_t)n_copy * 8, hipMemcpyDeviceToHost));
        }
    } else {
        // lastUsed values piled on a few milliseconds (a bucket above kPlanBucketMax): the general path — order-preserving
        // compaction, a stable descending radix sort sized by the qualified count the host has just read, run starts
        HIP_TRY(c, hipMemsetAsync(ps, 0, sizeof(PlanScalars), st));
        KT_BEGIN(c, st);
        hipLaunchKernelGGL(proactive_space_kernel, dim3(std::min(std::max(div_up(P, 256), 1), 512)), dim3(256), 0, st, pods, P,
                           U, default_units, ps);
        hipLaunchKernelGGL(proactive_scalars_kernel, dim3(1), dim3(64), 0, st, U, default_units, now, ps);
        hipLaunchKernelGGL(proactive_count_kernel, dim3(nb), dim3(kCompactBlock), 0, st, models, M, U, ps, counts,
                           &ps->n_candidates);
        hipLaunchKernelGGL(block_scan_kernel, dim3(1), dim3(256), 0, st, counts, nb, &ps->n_qualified);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(&h, ps, sizeof h, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        const int32_t nq = h.n_qualified;
        if (nq <= 0) {
            KT_END(c, st);
            HIP_TRY(c, hipStreamSynchronize(st));
            kt_collect(c);
        } else {
            hipLaunchKernelGGL(proactive_scatter_kernel, dim3(nb), dim3(kCompactBlock), 0, st, models, M, U, ps, counts,
                               c->r_keys.as<int64_t>(), c->r_vals.as<int32_t>());
            // stable descending radix sort: equal lastUsed keep registry order, so the first one seen wins
            size_t tmp_bytes = 0;
            HIP_TRY(c, rocprim::radix_sort_pairs_desc(nullptr, tmp_bytes, c->r_keys.as<int64_t>(), c->r_keys2.as<int64_t>(),
                                                      c->r_vals.as<int32_t>(), c->r_vals2.as<int32_t>(), (size_t)nq, 0, 64, st));
            HIP_TRY(c, c->r_tmp.ensure(std::max<size_t>(tmp_bytes, 16)));
            HIP_TRY(c, rocprim::radix_sort_pairs_desc(c->r_tmp.p, tmp_bytes, c->r_keys.as<int64_t>(), c->r_keys2.as<int64_t>(),
                                                      c->r_vals.as<int32_t>(), c->r_vals2.as<int32_t>(), (size_t)nq, 0, 64, st));
            const int nb2 = div_up(nq, kCompactBlock);
            hipLaunchKernelGGL(distinct_count_kernel, dim3(nb2), dim3(kCompactBlock), 0, st, c->r_keys2.as<int64_t>(), nq, counts);
            hipLaunchKernelGGL(block_scan_kernel, dim3(1), dim3(256), 0, st, counts, nb2, &ps->n_distinct);
            hipLaunchKernelGGL(distinct_scatter_kernel, dim3(nb2), dim3(kCompactBlock), 0, st, c->r_keys2.as<int64_t>(),
                               c->r_vals2.as<int32_t>(), nq, counts, ps, max_out, c->r_out_model.as<int32_t>(),
                               c->r_out_lu.as<int64_t>());
            hipLaunchKernelGGL(proactive_final_kernel, dim3(1), dim3(64), 0, st, ps);
            KT_END(c, st);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipMemcpyAsync(&h, ps, sizeof h, hipMemcpyDeviceToHost, st));
            HIP_TRY(c, hipStreamSynchronize(st));
            kt_collect(c);
            const int32_t n_copy = std::min(h.n_selected, max_out);
            if (n_copy > 0) {
                HIP_TRY(c, copy_sync(c, out_model, c->r_out_model.p, (size_t)n_copy * 4, hipMemcpyDeviceToHost));
                HIP_TRY(c, copy_sync(c, out_last_used, c->r_out_lu.p, (size_t)n_copy * 8, hipMemcpyDeviceToHost));
            }
        }
    }
    info->size_estimate = h.size_estimate;
    info->free_count = h.free_count;
    info->total_count = h.total_count;
    info->n_candidates = h.n_candidates;
    info->n_selected = h.n_selected;
    info->error = h.error;
    info->space_to_fill = h.space_to_fill;
    info->cutoff = h.cutoff;
    return MMP_OK;
} MMP_CATCH(c, "mmp_proactive_plan_subset")

namespace {
// the missing map covers at least n slots; new slots carry no mark (called with batch_mu)
int missing_cover(mmp_ctx *c, int32_t n)
{
    if (n <= c->miss_n) return MMP_OK;
    if (const int rc = grow_keep(c, c->miss_since, (size_t)c->miss_n * 8, (size_t)n * 8)) return rc;
    HIP_TRY(c, hipMemsetAsync(c->miss_since.as<int64_t>() + c->miss_n, 0, (size_t)(n - c->miss_n) * 8, c->stream));
    c->miss_n = n;
    return MMP_OK;
}
}  // namespace

int mmp_registry_prune(mmp_ctx *c, int32_t self_pod, int64_t now, int64_t gone_after, int64_t age_on_add, uint32_t flags,
                       mmp_prune_edit *edits_out, int32_t max_edits, mmp_prune_removed *removed_out, int32_t max_removed,
                       mmp_prune_info *info)
try {
    if (!c || !info || max_edits < 0 || max_removed < 0 || (max_edits > 0 && !edits_out) || (max_removed > 0 && !removed_out) || now <= 0 ||
        gone_after < 0 || age_on_add < 0 || plan_flags_bad(flags))
        return fail(c, MMP_EINVAL, "mmp_registry_prune: bad argument");
    // batch_mu owns c->stream, the scratch and the missing map for the whole call, and every writer of the state this call reads
    // (commit, the loaders, registry events) takes it too.  The state lock is taken only by an apply, for its in-place rewrite.
    std::lock_guard<std::mutex> gb(c->batch_mu);
    if (const int rc = plan_state_guard(c, "mmp_registry_prune")) return rc;
    const bool apply = flags & MMP_PRUNE_APPLY, dry = flags & MMP_PRUNE_DRY;
    if (const int rc = plan_arena_guard(c, "mmp_registry_prune", apply, 0)) return rc;  // (refused before anything advances)
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    const int32_t M = c->n_models, P = c->snap.P;
    const int nb = div_up(M, kPruneBlock);
    const int32_t cap_e = std::min(max_edits, M), cap_r = std::min(max_removed, c->n_entries);  // (a run has no more than these)
    if (const int rc = missing_cover(c, P)) return rc;
    const int32_t n_map = c->miss_n;
    HIP_TRY(c, c->p_state.ensure((size_t)std::max(P, 1)));
    HIP_TRY(c, c->p_seen.ensure((size_t)std::max(P, 1)));
    HIP_TRY(c, c->plan.totals.ensure(sizeof(PruneScalars)));
    HIP_TRY(c, c->plan.block_counts.ensure((size_t)std::max(nb, 1) * 3 * 4));
    HIP_TRY(c, c->plan.edits.ensure((size_t)std::max(cap_e, 1) * sizeof(mmp_prune_edit)));
    HIP_TRY(c, c->p_removed.ensure((size_t)std::max(cap_r, 1) * sizeof(mmp_prune_removed)));
    HIP_TRY(c, c->plan.keep_off.ensure((size_t)std::max(cap_e, 1) * 4));
    PruneArgs A{};
    A.self_pod = self_pod;
    A.P = P;
    A.now = now;
    A.gone_after = gone_after;
    A.repaired_last_used = (int64_t)((uint64_t)now - 3ull * (uint64_t)age_on_add);  // :6844
    const mmp_pod_row *pods = c->sb[c->cur].pods.as<mmp_pod_row>();  // the committed rows: what mmp_proactive_plan reads
    const mmp_model_row *models = c->models.as<mmp_model_row>();
    PruneScalars *ps = c->plan.totals.as<PruneScalars>();
    uint8_t *state = c->p_state.as<uint8_t>(), *seen = c->p_seen.as<uint8_t>();
    int64_t *since = c->miss_since.as<int64_t>();
    // the marks advance with the scan only when nothing can fail afterwards: always without an apply, and with an apply that
    // finds no edit (an apply with edits advances them once the registry has been rewritten)
    const int32_t advance = dry ? kMarksKeep : apply ? kMarksIfNoEdits : kMarksAdvance;
    KT_BEGIN(c, st);  // device span of the scan
    hipLaunchKernelGGL(prune_pods_kernel, dim3(std::max(div_up(P, 256), 1)), dim3(256), 0, st, pods, A, since, state, seen, ps);
    if (nb > 0) {
        hipLaunchKernelGGL(prune_count_kernel, dim3(nb), dim3(kPruneBlock), 0, st, models, M, c->ent_pod.as<int32_t>(),
                           c->ent_time.as<int64_t>(), A, state, seen, c->plan.block_counts.as<int32_t>(), ps);
        hipLaunchKernelGGL(prune_scan_kernel, dim3(1), dim3(256), 0, st, c->plan.block_counts.as<int32_t>(), nb, max_edits, max_removed, ps);
        hipLaunchKernelGGL(prune_scatter_kernel, dim3(nb), dim3(kPruneBlock), 0, st, models, M, c->ent_pod.as<int32_t>(),
                           c->ent_time.as<int64_t>(), A, state, c->plan.block_counts.as<int32_t>(), ps, c->plan.edits.as<mmp_prune_edit>(), cap_e,
                           c->p_removed.as<mmp_prune_removed>(), cap_r, c->plan.keep_off.as<int32_t>());
    }
    hipLaunchKernelGGL(prune_marks_kernel, dim3(std::max(div_up(n_map, 256), 1)), dim3(256), 0, st, A, n_map, state, seen, since, advance, ps);
    KT_END(c, st);
    HIP_TRY(c, hipGetLastError());
    PruneScalars h{};
    HIP_TRY(c, hipMemcpyAsync(&h, ps, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    kt_collect(c);
    const int32_t ne = std::min(h.n_edits, max_edits), nr = std::min(h.n_removed, max_removed);
    if (ne > 0) HIP_TRY(c, copy_sync(c, edits_out, c->plan.edits.p, (size_t)ne * sizeof(mmp_prune_edit), hipMemcpyDeviceToHost));
    if (nr > 0) HIP_TRY(c, copy_sync(c, removed_out, c->p_removed.p, (size_t)nr * sizeof(mmp_prune_removed), hipMemcpyDeviceToHost));
    info->n_edits = h.n_edits;
    info->n_removed = h.n_removed;
    info->n_repaired = h.n_repaired;
    info->n_unresolved = h.n_unresolved;
    info->n_missing_pods = h.n_missing_pods;
    info->n_new_missing = h.n_new_missing;
    info->truncated = h.truncated;
    info->reserved = 0;
    if (!apply || h.truncated || h.n_edits == 0) return MMP_OK;

    return registry_apply_edits(
        c, h.n_edits, h.n_kept, edits_out, [&](int32_t base, int32_t arena_end) {  // the surviving entries of the edited records
            hipLaunchKernelGGL(prune_build_kernel, dim3(div_up(h.n_edits, 256)), dim3(256), 0, st, c->plan.edits.as<mmp_prune_edit>(),
                               c->plan.keep_off.as<int32_t>(), h.n_edits, c->models.as<mmp_model_row>(), c->ent_pod.as<int32_t>(),
                               c->ent_time.as<int64_t>(), base, arena_end, A, state, c->u_idx.as<int32_t>(), c->u_rows.as<mmp_model_row>());
        },
        [&] {  // the registry holds the edited records: now the marks advance
            hipLaunchKernelGGL(prune_marks_kernel, dim3(std::max(div_up(n_map, 256), 1)), dim3(256), 0, st, A, n_map, state, seen, since, kMarksAdvance, ps);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipStreamSynchronize(st));
            return (int)MMP_OK;
        });
} MMP_CATCH(c, "mmp_registry_prune")

int mmp_registry_census(mmp_ctx *c, mmp_registry_stats *out, int32_t *pod_loaded_out, int32_t *pod_failed_out, int32_t max_pods,
                        int32_t *n_pods_out, mmp_registry_type_stats *types_out, int32_t max_types, int32_t *n_types_out)
try {
    if (!c || !out || !n_pods_out || !n_types_out || max_pods < 0 || max_types < 0 || (max_pods > 0 && (!pod_loaded_out || !pod_failed_out)) ||
        (max_types > 0 && !types_out))
        return fail(c, MMP_EINVAL, "mmp_registry_census: bad argument");
    // batch_mu owns c->stream and the scratch for the whole call, and every writer of what this call reads — registry events, an
    // applied prune or janitor plan, the loaders of the registry, the instance table and the type table — takes it too and leaves
    // with its work on c->stream finished.  The state lock is not taken: nothing decisions read is written.
    std::lock_guard<std::mutex> gb(c->batch_mu);
    const int32_t M = c->n_models, P = (int32_t)c->pods.size(), T = c->n_types;
    *n_pods_out = P;
    *n_types_out = T;
    if ((max_pods > 0 && max_pods < P) || (max_types > 0 && max_types < T))
        return fail(c, MMP_EINVAL, "mmp_registry_census: room for %d pods and %d types, the tables have %d and %d", max_pods, max_types, P, T);
    const bool want_pods = max_pods > 0, want_types = max_types > 0;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    if (c->census_cus == 0) {  // the first call: the device's size, and the dynamic LDS the walk keeps its per-pod counts in
        int cus = 0;
        c->census_cus = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->cfg.device) == hipSuccess && cus > 0 ? cus : 256;
        if (kCensusPodLdsBytes + kCensusStaticLds <= c->lds_limit &&
            hipFuncSetAttribute(reinterpret_cast<const void *>(census_walk_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)kCensusPodLdsBytes) == hipSuccess)
            c->census_pod_lds = kCensusPodLdsBytes;
        (void)hipGetLastError();
    }
    hipStream_t st = c->stream;
    const size_t o_types = 128, o_pods = o_types + (size_t)T * sizeof(mmp_registry_type_stats), total = o_pods + (size_t)P * 8;
    static_assert(sizeof(mmp_registry_stats) <= 128, "the scalars come first");
    HIP_TRY(c, c->cn_out.ensure(total));
    char *d = c->cn_out.as<char>();
    // private per-pod counts when the two arrays fit the LDS the kernel was granted; as many workgroups as stay resident with it
    const size_t pod_lds = (size_t)P * 8;
    const bool priv = pod_lds <= c->census_pod_lds;
    const int nb = div_up(M, kCensusBlock);
    const int per_cu = priv ? (int)std::min<size_t>(8, std::max<size_t>(1, kLdsPerCU / (pod_lds + kCensusStaticLds))) : 8;
    const int grid = std::min(nb, std::min(kCensusGridMax, c->census_cus * per_cu));
    KT_BEGIN(c, st);
    HIP_TRY(c, hipMemsetAsync(d, 0, total, st));
    if (nb > 0) {
        if (priv)
            hipLaunchKernelGGL(census_walk_kernel<true>, dim3(grid), dim3(kCensusBlock), pod_lds, st, c->models.as<mmp_model_row>(), M,
                               c->ent_pod.as<int32_t>(), P, T, (mmp_registry_stats *)d, (mmp_registry_type_stats *)(d + o_types),
                               (int32_t *)(d + o_pods));
        else
            hipLaunchKernelGGL(census_walk_kernel<false>, dim3(grid), dim3(kCensusBlock), 0, st, c->models.as<mmp_model_row>(), M,
                               c->ent_pod.as<int32_t>(), P, T, (mmp_registry_stats *)d, (mmp_registry_type_stats *)(d + o_types),
                               (int32_t *)(d + o_pods));
    }
    KT_END(c, st);
    HIP_TRY(c, hipGetLastError());
    const size_t take = want_pods ? total : o_pods;  // (the pod arrays come last)
    c->cn_host.resize(total);
    HIP_TRY(c, copy_sync(c, c->cn_host.data(), d, take, hipMemcpyDeviceToHost));
    kt_collect(c);
    memcpy(out, c->cn_host.data(), sizeof *out);
    if (want_types && T > 0) memcpy(types_out, c->cn_host.data() + o_types, (size_t)T * sizeof(mmp_registry_type_stats));
    if (want_pods && P > 0) {
        memcpy(pod_loaded_out, c->cn_host.data() + o_pods, (size_t)P * 4);
        memcpy(pod_failed_out, c->cn_host.data() + o_pods + (size_t)P * 4, (size_t)P * 4);
    }
    return MMP_OK;
} MMP_CATCH(c, "mmp_registry_census")

int mmp_registry_unresolved(mmp_ctx *c, int32_t *model_out, int32_t max_models, int32_t *n_models_out, int64_t *n_entries_out)
try {
    if (!c || !n_models_out || !n_entries_out || max_models < 0 || (max_models > 0 && !model_out))
        return fail(c, MMP_EINVAL, "mmp_registry_unresolved: bad argument");
    // read-only, the locking of the census: batch_mu owns c->stream and the plans' scratch, every writer of the registry and of the
    // instance table takes it too; nothing decisions read is written
    std::lock_guard<std::mutex> gb(c->batch_mu);
    const int32_t M = c->n_models, P = (int32_t)c->pods.size();
    *n_models_out = 0;
    *n_entries_out = 0;
    if (M == 0) return MMP_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    const int nb = div_up(M, kUnresolvedBlock);
    const int32_t cap = std::min(max_models, M);
    HIP_TRY(c, c->plan.totals.ensure(sizeof(PruneScalars)));
    HIP_TRY(c, c->plan.block_counts.ensure((size_t)nb * 3 * 4));
    HIP_TRY(c, c->unres_list.ensure((size_t)std::max(cap, 1) * 4));
    const mmp_model_row *models = c->models.as<mmp_model_row>();
    int32_t *counts = c->plan.block_counts.as<int32_t>();
    PruneScalars *ps = c->plan.totals.as<PruneScalars>();
    KT_BEGIN(c, st);
    hipLaunchKernelGGL(unresolved_count_kernel, dim3(nb), dim3(kUnresolvedBlock), 0, st, models, M, c->ent_pod.as<int32_t>(), P, counts);
    hipLaunchKernelGGL(prune_scan_kernel, dim3(1), dim3(256), 0, st, counts, nb, INT32_MAX, INT32_MAX, ps);
    if (cap > 0)
        hipLaunchKernelGGL(unresolved_list_kernel, dim3(nb), dim3(kUnresolvedBlock), 0, st, models, M, c->ent_pod.as<int32_t>(), P, counts,
                           c->unres_list.as<int32_t>(), cap);
    KT_END(c, st);
    HIP_TRY(c, hipGetLastError());
    PruneScalars h{};
    HIP_TRY(c, copy_sync(c, &h, ps, sizeof h, hipMemcpyDeviceToHost));
    kt_collect(c);
    const int32_t take = std::min(h.n_edits, cap);
    if (take > 0) HIP_TRY(c, copy_sync(c, model_out, c->unres_list.p, (size_t)take * 4, hipMemcpyDeviceToHost));
    *n_models_out = h.n_edits;
    *n_entries_out = h.n_kept;
    return MMP_OK;
} MMP_CATCH(c, "mmp_registry_unresolved")

int mmp_registry_missing_get(mmp_ctx *c, int64_t *since_out, int32_t max_pods, int32_t *n_out)
try {
    if (!c || !n_out || max_pods < 0 || (max_pods > 0 && !since_out)) return fail(c, MMP_EINVAL, "mmp_registry_missing_get: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    *n_out = c->miss_n;
    const int32_t n = std::min(c->miss_n, max_pods);
    if (n > 0) HIP_TRY(c, copy_sync(c, since_out, c->miss_since.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    return MMP_OK;
} MMP_CATCH(c, "mmp_registry_missing_get")

int mmp_registry_missing_reset(mmp_ctx *c)
try {
    if (!c) return fail(c, MMP_EINVAL, "mmp_registry_missing_reset: null context");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    if (c->miss_n > 0) {
        HIP_TRY(c, hipMemsetAsync(c->miss_since.p, 0, (size_t)c->miss_n * 8, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return MMP_OK;
} MMP_CATCH(c, "mmp_registry_missing_reset")

namespace {
// The model-indexed map of mmp_janitor_plan and mmp_registry_ops covers M words, all -1 (called with batch_mu).  The one M-sized
// fill: when the map is new, grew or was left in doubt.  It is in doubt from here on (model_map_n = 0) until the caller has seen the
// kernel that clears its words again complete, and says so with model_map_n = M.
int model_map_cover(mmp_ctx *c, int32_t M, hipStream_t st)
{
    if (c->plan.model_map_n < M || (size_t)M * 4 > c->plan.model_map.cap) {
        HIP_TRY(c, c->plan.model_map.ensure((size_t)std::max(M, 1) * 4));
        HIP_TRY(c, hipMemsetAsync(c->plan.model_map.p, 0xff, (size_t)std::max(M, 1) * 4, st));
    }
    c->plan.model_map_n = 0;
    return MMP_OK;
}
// the scale-down's two kernels on candidates that stand on the device (defined with the rebalance calls below)
int scaledown_enqueue(mmp_ctx *c, hipStream_t st, const mmp_cache_entry *d_entries, const mmp_conc_entry *d_conc, int32_t n,
                      const mmp_scaledown_params *p, int64_t dyn_const);

// the keys of a periodic task (tasks_keyed_kernels.hpp), in two steps around the caller's KT_BEGIN: the staged copy — it keeps
// keyed_resolve_kernel's contract: the buffer is an allocation of its own with 16 bytes behind the keys — and the launch that
// writes `model` of the n staged entries and c->me_row.  `rel` stays with the caller until it has synchronised.
int tasks_keys_stage(mmp_ctx *c, const char *fn, const char *keys, const int32_t *key_off, int32_t n, std::vector<int32_t> &rel)
{
    if (const int rc = stage_strings(c, fn, "key ", keys, key_off, n, c->ida_bytes, c->ida_off, rel)) return rc;
    HIP_TRY(c, c->me_row.ensure((size_t)n * 4));
    return MMP_OK;
}
extern "C++" template <class Entry, class Claim>  // (a template inside the file's extern "C" block)
void tasks_keys_launch(mmp_ctx *c, int32_t n, Entry *d_entries, const Claim &claim)
{
    const TasksKeyArgs<Entry> A{c->ida_bytes.as<char>(), c->ida_off.as<int32_t>(), n, hash_mask(c->tune.model_id_hash_bits), vmodel_models(c),
                                c->me_row.as<int32_t>(), d_entries};
    hipLaunchKernelGGL((tasks_keyed_kernel<Entry, Claim>), dim3(div_up(n, kIdTabBlock)), dim3(kIdTabBlock), 0, c->stream, A, claim);
}
// model_idx_out of a _k call: the table's rows by key, the caller's own rows by row
extern "C++" template <class Entry>
int tasks_model_idx(mmp_ctx *c, bool keyed, const Entry *entries, int32_t n, int32_t *model_idx_out)
{
    if (!model_idx_out || n == 0) return MMP_OK;
    if (keyed) {
        HIP_TRY(c, copy_sync(c, model_idx_out, c->me_row.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    } else
        for (int32_t i = 0; i < n; i++) model_idx_out[i] = entries[i].model;
    return MMP_OK;
}

// what both janitor entry points refuse before the lock is taken
bool janitor_args_bad(const mmp_ctx *c, const mmp_janitor_entry *entries, int32_t n, const mmp_janitor_params *p, uint32_t flags,
                      const uint8_t *actions_out, const mmp_janitor_edit *edits_out, int32_t max_edits, const mmp_cache_entry *cands_out,
                      const int32_t *cand_rows_out, int32_t max_cands, const mmp_janitor_info *info)
{
    return !c || !p || !info || n < 0 || max_edits < 0 || max_cands < 0 || (n > 0 && (!entries || !actions_out)) || (max_edits > 0 && !edits_out) ||
           (max_cands > 0 && (!cands_out || !cand_rows_out)) || p->now <= 0 || p->janitor_freq_secs < 0 || p->load_timeout_ms < 0 ||
           p->min_stale_age_ms < 0 || p->load_failure_expiry_ms < 0 || p->short_expiry_recent_use_ms < 0 || p->unload_attempt_recent_ms < 0 ||
           p->lastused_age_on_add_ms < 0 || plan_flags_bad(flags);
}

// What mmp_janitor_plan_k adds to the plan: the scale-down of the candidates in the same hold (sd == nullptr: no chain)
struct JanitorChain {
    const mmp_scaledown_params *sd;
    const mmp_conc_entry *conc;  // n rows in INPUT-row order; nullptr: not latency-based
    int64_t dyn_const;
    uint8_t *removed_out;        // one byte per candidate
};

// THE JANITOR PIPELINE (janitor_kernels.hpp), stated once for mmp_janitor_plan and mmp_janitor_plan_k: the caller has refused its
// NULL and negative arguments; this takes batch_mu, refuses everything else BEFORE anything is staged or written, stages the
// entries, resolves and claims by key when there are keys (tasks_keyed_kernel in the place of janitor_entry_kernel: `model` of the
// staged entry is then the device's, the caller's is never read), evaluates, reads back, applies, and — with a chain — decides
// the scale-down of the candidates where they lie, behind the apply.  keys / key_off both NULL: by row, range and
// one-row-per-model checked here.
int janitor_drive(mmp_ctx *c, const char *fn, const mmp_janitor_entry *entries, int32_t n, const char *keys, const int32_t *key_off,
                  const mmp_janitor_params *p, uint32_t flags, const JanitorChain &ch, int32_t *model_idx_out, uint8_t *actions_out,
                  mmp_janitor_edit *edits_out, int32_t max_edits, mmp_cache_entry *cands_out, int32_t *cand_rows_out, int32_t max_cands,
                  mmp_janitor_info *info)
{
    const bool keyed = keys || key_off;
    // batch_mu owns c->stream, the scratch, the map and the model-id table for the whole call, and every writer of the state this
    // call reads takes it too: the row a key resolves to, the edit of that row and the scale-down that reads the edited record see
    // ONE sequence of states no other writer enters.  The state lock is taken only by an apply, for its in-place rewrite.
    std::lock_guard<std::mutex> gb(c->batch_mu);
    if (const int rc = plan_state_guard(c, fn)) return rc;
    if (keyed)
        if (const int rc = model_id_space_guard(c, fn)) return rc;
    const int32_t M = c->n_models, P = c->snap.P;
    if (p->self_pod < 0 || p->self_pod >= P) return fail(c, MMP_EINVAL, "%s: self_pod %d of %d", fn, p->self_pod, P);
    if (ch.sd && ch.sd->self_pod != p->self_pod)
        return fail(c, MMP_EINVAL, "%s: the scale-down is self_pod %d's, the run self_pod %d's", fn, ch.sd->self_pod, p->self_pod);
    if (keyed) {
        // (by key the row is the device's own and lies in [-1, M); that no model has two rows is settled by the first kernel, on the map)
        if (const int rc = check_offsets(c, fn, "key ", key_off, n)) return rc;
    } else {
        // the rows index the map: range and one-row-per-model are settled here, before any kernel reads them
        if (++c->u_gen == 0) ++c->u_gen;  // (generation 0 is what an untouched stamp carries)
        const uint64_t gen = (uint64_t)c->u_gen << 32;
        if (c->u_stamp.size() < (size_t)M) c->u_stamp.resize(M, 0);
        for (int32_t r = 0; r < n; r++) {
            const int32_t m = entries[r].model;
            if (m < -1 || m >= M) return fail(c, MMP_EINVAL, "%s: row %d names model %d of %d", fn, r, m, M);
            if (m < 0) continue;
            if ((c->u_stamp[m] & ~0xffffffffull) == gen) return fail(c, MMP_EINVAL, "%s: model %d has two rows", fn, m);
            c->u_stamp[m] = gen | (uint32_t)r;
        }
    }
    // (by row *info is reset here, as mmp_janitor_plan always did; by key a refused call writes nothing, and the duplicates are
    // only known behind the first kernel: there it is reset behind that check)
    if (!keyed) {
        *info = mmp_janitor_info{};
        info->stopped_at = -1;
    }
    const bool apply = flags & MMP_JANITOR_APPLY;
    hipStream_t st = c->stream;
    std::vector<int32_t> krel;  // (what the staged offsets are uploaded from: lives until the first synchronisation below)
    if (p->shutting_down) {  // :5880
        if (keyed && n > 0) {  // nothing is evaluated; the keys are still resolved, and two entries of one record still refused
            HIP_TRY(c, hipSetDevice(c->cfg.device));
            if (const int rc = tasks_keys_stage(c, fn, keys, key_off, n, krel)) return rc;
            HIP_TRY(c, c->plan.rows_in.ensure((size_t)n * sizeof(mmp_janitor_entry)));
            HIP_TRY(c, c->plan.call_scalars.ensure(sizeof(JanitorScalars)));
            if (const int rc = model_map_cover(c, M, st)) return rc;
            mmp_janitor_entry *d_in = c->plan.rows_in.as<mmp_janitor_entry>();
            JanitorScalars *js = c->plan.call_scalars.as<JanitorScalars>();
            HIP_TRY(c, hipMemcpyAsync(d_in, entries, (size_t)n * sizeof(mmp_janitor_entry), hipMemcpyHostToDevice, st));
            HIP_TRY(c, hipMemsetAsync(js, 0, sizeof(JanitorScalars), st));
            KT_BEGIN(c, st);
            tasks_keys_launch(c, n, d_in, TasksJanitorClaim{c->plan.model_map.as<int32_t>(), js, *p, n});
            hipLaunchKernelGGL(tasks_unclaim_kernel, dim3(div_up(n, 256)), dim3(256), 0, st, d_in, n, c->plan.model_map.as<int32_t>());
            KT_END(c, st);
            HIP_TRY(c, hipGetLastError());
            JanitorScalars hj{};
            HIP_TRY(c, copy_sync(c, &hj, js, sizeof hj, hipMemcpyDeviceToHost));
            c->plan.model_map_n = M;
            kt_collect(c);
            if (hj.n_dup != 0) return fail(c, MMP_EINVAL, "%s: %d entries name a model another entry of the call names", fn, hj.n_dup);
        }
        if (const int rc = tasks_model_idx(c, keyed, entries, n, model_idx_out)) return rc;
        *info = mmp_janitor_info{};
        info->stopped_at = -1;
        if (n > 0) memset(actions_out, MMP_JANITOR_NONE, (size_t)n);
        info->n_action[MMP_JANITOR_NONE] = n;
        return MMP_OK;
    }
    if (const int rc = plan_arena_guard(c, fn, apply, n)) return rc;  // (refused before anything is done)
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const int nb = div_up(M, kJanBlock), n1 = std::max(n, 1);
    const int32_t cap_e = std::min(max_edits, M);
    // the row-sized scratch, carved from one buffer
    size_t off = 0;
    auto carve = [&off](size_t bytes) {
        const size_t at = off;
        off = (off + bytes + 255) & ~size_t(255);
        return at;
    };
    const size_t o_ctime = carve((size_t)n1 * 8), o_crow = carve((size_t)n1 * 4), o_drop = carve((size_t)n1), o_act = carve((size_t)n1),
                 o_cands = carve((size_t)n1 * sizeof(mmp_cache_entry)), o_orow = carve((size_t)n1 * 4);
    HIP_TRY(c, c->plan.row_tmp.ensure(off));
    char *tmp = c->plan.row_tmp.as<char>();
    HIP_TRY(c, c->plan.rows_in.ensure((size_t)n1 * sizeof(mmp_janitor_entry)));
    HIP_TRY(c, c->plan.call_scalars.ensure(sizeof(JanitorScalars)));
    HIP_TRY(c, c->plan.totals.ensure(sizeof(PruneScalars)));
    HIP_TRY(c, c->plan.block_counts.ensure((size_t)std::max(nb, 1) * 3 * 4));
    HIP_TRY(c, c->plan.edits.ensure((size_t)std::max(cap_e, 1) * sizeof(mmp_janitor_edit)));
    HIP_TRY(c, c->plan.keep_off.ensure((size_t)std::max(cap_e, 1) * 4));
    if (const int rc = model_map_cover(c, M, st)) return rc;  // (in doubt until the finish kernel has been seen to complete)
    const mmp_pod_row *pods = c->sb[c->cur].pods.as<mmp_pod_row>();  // the committed rows
    const mmp_model_row *models = c->models.as<mmp_model_row>();
    const int32_t *ent_pod = c->ent_pod.as<int32_t>();
    const int64_t *ent_time = c->ent_time.as<int64_t>();
    mmp_janitor_entry *d_in = c->plan.rows_in.as<mmp_janitor_entry>();
    int32_t *map = c->plan.model_map.as<int32_t>();
    JanitorScalars *js = c->plan.call_scalars.as<JanitorScalars>();
    PruneScalars *ps = c->plan.totals.as<PruneScalars>();
    int64_t *ctime = (int64_t *)(tmp + o_ctime);
    int32_t *crow = (int32_t *)(tmp + o_crow), *orow = (int32_t *)(tmp + o_orow);
    uint8_t *drop = (uint8_t *)(tmp + o_drop), *act = (uint8_t *)(tmp + o_act);
    mmp_cache_entry *d_cands = (mmp_cache_entry *)(tmp + o_cands);
    if (keyed && n > 0)
        if (const int rc = tasks_keys_stage(c, fn, keys, key_off, n, krel)) return rc;
    if (ch.sd && ch.conc && n > 0) {  // the MaxConcCacheEntry rows in input-row order, and room for the candidates' beside them
        HIP_TRY(c, c->s_c.ensure((size_t)n * sizeof(mmp_conc_entry)));
        HIP_TRY(c, c->s_d.ensure((size_t)n * sizeof(mmp_conc_entry)));
        HIP_TRY(c, hipMemcpyAsync(c->s_c.p, ch.conc, (size_t)n * sizeof(mmp_conc_entry), hipMemcpyHostToDevice, st));
    }
    if (n > 0) HIP_TRY(c, hipMemcpyAsync(c->plan.rows_in.p, entries, (size_t)n * sizeof(mmp_janitor_entry), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemsetAsync(js, 0, sizeof(JanitorScalars), st));
    HIP_TRY(c, hipMemsetAsync(ps, 0, sizeof(PruneScalars), st));
    KT_BEGIN(c, st);  // device span of the plan
    const int gn = div_up(n, 256);
    if (n > 0) {
        if (keyed)  // the row from the key, the claim of it on the map, the stop index: one launch in the entry kernel's place
            tasks_keys_launch(c, n, d_in, TasksJanitorClaim{map, js, *p, n});
        else
            hipLaunchKernelGGL(janitor_entry_kernel, dim3(gn), dim3(256), 0, st, d_in, n, map, *p, js);
    }
    if (nb > 0) {
        hipLaunchKernelGGL(janitor_count_kernel, dim3(nb), dim3(kJanBlock), 0, st, models, M, ent_pod, ent_time, pods, P, map, d_in, n, *p, js,
                           c->plan.block_counts.as<int32_t>());
        hipLaunchKernelGGL(prune_scan_kernel, dim3(1), dim3(256), 0, st, c->plan.block_counts.as<int32_t>(), nb, INT32_MAX, INT32_MAX, ps);
        hipLaunchKernelGGL(janitor_scatter_kernel, dim3(nb), dim3(kJanBlock), 0, st, models, M, ent_pod, ent_time, pods, P, map, d_in, n, *p, js,
                           c->plan.block_counts.as<int32_t>(), ps, c->plan.edits.as<mmp_janitor_edit>(), cap_e, c->plan.keep_off.as<int32_t>(), ctime, crow);
    }
    if (n > 0) {
        const int gt = div_up(n, kJanTile);
        hipLaunchKernelGGL(janitor_tie_kernel, dim3(gt), dim3(256), 0, st, ctime, ps, drop, js);
        hipLaunchKernelGGL(janitor_rank_kernel, dim3(gt), dim3(256), 0, st, ctime, crow, drop, ps, d_in, d_cands, orow, n);
        hipLaunchKernelGGL(janitor_finish_kernel, dim3(gn), dim3(256), 0, st, d_in, n, models, ent_pod, ent_time, map, *p, act, js);
    }
    KT_END(c, st);
    HIP_TRY(c, hipGetLastError());
    JanitorScalars hj{};
    PruneScalars h{};
    HIP_TRY(c, hipMemcpyAsync(&hj, js, sizeof hj, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&h, ps, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    c->plan.model_map_n = M;
    kt_collect(c);
    // two entries of one record: refused with nothing written (the finish kernel has put every claimed map word back to -1)
    if (hj.n_dup != 0) return fail(c, MMP_EINVAL, "%s: %d entries name a model another entry of the call names", fn, hj.n_dup);
    if (const int rc = tasks_model_idx(c, keyed, entries, n, model_idx_out)) return rc;
    *info = mmp_janitor_info{};
    const int32_t ne = std::min(h.n_edits, max_edits), nc = std::min(hj.n_cands, max_cands);
    if (n > 0) HIP_TRY(c, copy_sync(c, actions_out, act, (size_t)n, hipMemcpyDeviceToHost));
    if (ne > 0) HIP_TRY(c, copy_sync(c, edits_out, c->plan.edits.p, (size_t)ne * sizeof(mmp_janitor_edit), hipMemcpyDeviceToHost));
    if (nc > 0) {
        HIP_TRY(c, copy_sync(c, cands_out, d_cands, (size_t)nc * sizeof(mmp_cache_entry), hipMemcpyDeviceToHost));
        HIP_TRY(c, copy_sync(c, cand_rows_out, orow, (size_t)nc * 4, hipMemcpyDeviceToHost));
    }
    info->n_edits = h.n_edits;
    info->n_candidates = hj.n_cands;
    info->n_ties = hj.n_ties;
    info->stopped_at = hj.stop_inv > 0 ? n - hj.stop_inv : -1;
    info->truncated = (h.n_edits > max_edits || hj.n_cands > max_cands) ? 1 : 0;
    for (int k = 0; k < 7; k++) info->n_action[k] = hj.n_action[k];
    if (!apply || info->truncated) return MMP_OK;
    if (h.n_edits > 0)
        if (const int rc = registry_apply_edits(c, h.n_edits, h.n_kept, edits_out, [&](int32_t base, int32_t arena_end) {  // the records without / with self_pod's entry
                hipLaunchKernelGGL(janitor_build_kernel, dim3(div_up(h.n_edits, 256)), dim3(256), 0, st, c->plan.edits.as<mmp_janitor_edit>(),
                                   c->plan.keep_off.as<int32_t>(), h.n_edits, c->models.as<mmp_model_row>(), c->ent_pod.as<int32_t>(),
                                   c->ent_time.as<int64_t>(), base, arena_end, p->self_pod, c->u_idx.as<int32_t>(), c->u_rows.as<mmp_model_row>());
            }))
            return rc;
    // THE SCALE-DOWN IN THE SAME CALL (MM.java:6110-6145 is the tail of the one janitorTask): the candidates stand where the rank
    // kernel put them, the registry holds what the two loops left, and nobody else has had the batch lock in between.  (A run that
    // stopped at a repaired row has no candidates: the registry loop was never reached.)
    if (!ch.sd || hj.n_cands == 0) return MMP_OK;
    const int32_t nk = hj.n_cands;
    const double before_ms = c->last_kernel_ms;
    HIP_TRY(c, c->s_a.ensure((size_t)nk));
    HIP_TRY(c, c->s_b.ensure((size_t)nk));
    KT_BEGIN(c, st);
    if (ch.conc)
        hipLaunchKernelGGL(tasks_conc_gather_kernel, dim3(div_up(nk, 256)), dim3(256), 0, st, c->s_c.as<mmp_conc_entry>(), orow, nk,
                           c->s_d.as<mmp_conc_entry>());
    if (const int rc = scaledown_enqueue(c, st, d_cands, ch.conc ? c->s_d.as<mmp_conc_entry>() : nullptr, nk, ch.sd, ch.dyn_const)) return rc;
    KT_END(c, st);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, copy_sync(c, ch.removed_out, c->s_b.p, (size_t)nk, hipMemcpyDeviceToHost));
    kt_collect(c);
    kt_add(c, before_ms);  // the call's device span: plan + apply + scale-down
    return MMP_OK;
}
}  // namespace

int mmp_janitor_plan(mmp_ctx *c, const mmp_janitor_entry *entries, int32_t n, const mmp_janitor_params *p, uint32_t flags,
                     uint8_t *actions_out, mmp_janitor_edit *edits_out, int32_t max_edits, mmp_cache_entry *cands_out,
                     int32_t *cand_rows_out, int32_t max_cands, mmp_janitor_info *info)
try {
    if (janitor_args_bad(c, entries, n, p, flags, actions_out, edits_out, max_edits, cands_out, cand_rows_out, max_cands, info))
        return fail(c, MMP_EINVAL, "mmp_janitor_plan: bad argument");
    return janitor_drive(c, "mmp_janitor_plan", entries, n, nullptr, nullptr, p, flags, JanitorChain{}, nullptr, actions_out, edits_out, max_edits,
                         cands_out, cand_rows_out, max_cands, info);
} MMP_CATCH(c, "mmp_janitor_plan")

namespace {
// THE REGISTRY-OPS PIPELINE (registry_ops_kernels.hpp), stated once for mmp_registry_ops and mmp_registry_ops_k: the caller has
// refused its NULL arguments; this takes batch_mu, refuses everything else BEFORE anything is staged, stages the ops, resolves
// the keys in front of the evaluation when there are any (rops_keyed_kernel: `model` of the staged op is then the device's, the
// caller's is never read), evaluates, reads back and applies.  max_kind: the last MMP_ROP_* kind the entry point admits.
// keys / key_off both NULL: by row, `model` range-checked here.  *info is written only by a call that answers MMP_OK.
// ev (mmp_evictions_k; keyed, ops == nullptr): the op rows are not the caller's — evict_stage_kernel (evictions_kernels.hpp) builds them
// on the device from the victims' entries, behind the resolve stage and in front of the evaluation, and reads the row for
// onEviction's decision there; ev->outs is written where status_out is.
struct RopsEvict {
    const mmp_evicted_entry *entries;
    const mmp_evict_params *p;
    mmp_evicted_out *outs;
};
int rops_drive(mmp_ctx *c, const char *fn, int32_t max_kind, const mmp_registry_op *ops, int32_t n, const char *keys, const int32_t *key_off,
               int64_t now, uint32_t flags, int32_t *model_idx_out, uint8_t *status_out, mmp_registry_op_edit *edits_out, int32_t max_edits,
               mmp_registry_ops_info_k *info, const RopsEvict *ev = nullptr)
{
    const bool keyed = keys || key_off;
    // batch_mu owns c->stream, the scratch, the map and the model-id table for the whole call, and every writer of the state this
    // call reads takes it too: the row a key resolves to and the edit of that row see ONE state.  The state lock is taken only by
    // an apply, for its in-place rewrite.
    std::lock_guard<std::mutex> gb(c->batch_mu);
    if (const int rc = plan_state_guard(c, fn)) return rc;
    if (keyed)
        if (const int rc = model_id_space_guard(c, fn)) return rc;
    const int32_t M = c->n_models, P = c->snap.P;
    // the ops index the map, the rows and the instance table: their ranges are settled here, before any kernel reads them (that
    // no model is named twice is settled by the first kernel, on the map; by key the row is the device's own and lies in [-1, M))
    if (ev) {
        if (ev->p->self_pod < 0 || ev->p->self_pod >= P) return fail(c, MMP_EINVAL, "%s: self_pod %d of %d", fn, ev->p->self_pod, P);
        for (int32_t i = 0; i < n; i++)
            if (ev->entries[i].flags & ~MMP_EVF_FAILED) return fail(c, MMP_EINVAL, "%s: entry %d has flags %u", fn, i, ev->entries[i].flags);
    }
    for (int32_t i = 0; i < n && !ev; i++) {
        const mmp_registry_op &o = ops[i];
        if (!keyed && (o.model < 0 || o.model >= M)) return fail(c, MMP_EINVAL, "%s: op %d names model %d of %d", fn, i, o.model, M);
        if (o.pod < 0 || o.pod >= P) return fail(c, MMP_EINVAL, "%s: op %d names pod %d of %d", fn, i, o.pod, P);
        if (o.op < MMP_ROP_REGISTER || o.op > max_kind) return fail(c, MMP_EINVAL, "%s: op %d has kind %d", fn, i, o.op);
        if ((o.flags & ~(MMP_ROPF_SHUTTING_DOWN | MMP_ROPF_MATCH_TIME)) || (o.op == MMP_ROP_DROP_LOCAL && o.flags))
            return fail(c, MMP_EINVAL, "%s: op %d has flags %u", fn, i, o.flags);
    }
    if (keyed)
        if (const int rc = check_offsets(c, fn, "key ", key_off, n)) return rc;
    if (n == 0) {
        *info = mmp_registry_ops_info_k{};
        return MMP_OK;
    }
    const bool apply = flags & MMP_ROPS_APPLY;
    if (const int rc = plan_arena_guard(c, fn, apply, n)) return rc;  // (refused before anything is done)
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    const int nb = div_up(n, kRopsBlock);
    const int32_t cap_e = std::min(max_edits, n);
    HIP_TRY(c, c->plan.rows_in.ensure((size_t)n * sizeof(mmp_registry_op)));
    HIP_TRY(c, c->plan.call_scalars.ensure(std::max(sizeof(RopsScalars), sizeof(JanitorScalars))));
    HIP_TRY(c, c->plan.row_tmp.ensure((size_t)n));
    HIP_TRY(c, c->plan.totals.ensure(sizeof(PruneScalars)));
    HIP_TRY(c, c->plan.block_counts.ensure((size_t)nb * 3 * 4));
    HIP_TRY(c, c->plan.edits.ensure((size_t)std::max(cap_e, 1) * sizeof(mmp_registry_op_edit)));
    HIP_TRY(c, c->plan.keep_off.ensure((size_t)std::max(cap_e, 1) * 4));
    std::vector<int32_t> krel;  // (what the staged offsets are uploaded from: lives until the synchronisation below)
    if (keyed) {
        if (const int rc = stage_strings(c, fn, "key ", keys, key_off, n, c->ida_bytes, c->ida_off, krel)) return rc;
        HIP_TRY(c, c->me_row.ensure((size_t)n * 4));
    }
    if (ev) {
        HIP_TRY(c, c->ev_in.ensure((size_t)n * sizeof(mmp_evicted_entry)));
        HIP_TRY(c, c->ev_out.ensure((size_t)n * sizeof(mmp_evicted_out)));
    }
    if (const int rc = model_map_cover(c, M, st)) return rc;  // (in doubt until the scatter kernel has been seen to complete)
    const mmp_pod_row *pods = c->sb[c->cur].pods.as<mmp_pod_row>();  // the committed rows: what the janitor's insert reads
    const mmp_model_row *models = c->models.as<mmp_model_row>();
    const int32_t *ent_pod = c->ent_pod.as<int32_t>();
    const int64_t *ent_time = c->ent_time.as<int64_t>();
    mmp_registry_op *d_ops = c->plan.rows_in.as<mmp_registry_op>();
    int32_t *map = c->plan.model_map.as<int32_t>();
    RopsScalars *rs = c->plan.call_scalars.as<RopsScalars>();
    PruneScalars *ps = c->plan.totals.as<PruneScalars>();
    uint8_t *d_status = c->plan.row_tmp.as<uint8_t>();
    if (ev)
        HIP_TRY(c, hipMemcpyAsync(c->ev_in.p, ev->entries, (size_t)n * sizeof(mmp_evicted_entry), hipMemcpyHostToDevice, st));
    else
        HIP_TRY(c, hipMemcpyAsync(c->plan.rows_in.p, ops, (size_t)n * sizeof(mmp_registry_op), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemsetAsync(rs, 0, sizeof(RopsScalars), st));
    HIP_TRY(c, hipMemsetAsync(ps, 0, sizeof(PruneScalars), st));
    KT_BEGIN(c, st);  // device span of the evaluation
    if (keyed) {
        // (the staged copy keeps keyed_resolve_kernel's contract: the buffer is an allocation of its own with 16 bytes behind the keys)
        const RopsKeyArgs A{c->ida_bytes.as<char>(), c->ida_off.as<int32_t>(), n, hash_mask(c->tune.model_id_hash_bits), vmodel_models(c),
                            c->me_row.as<int32_t>(), d_ops};
        hipLaunchKernelGGL(rops_keyed_kernel, dim3(div_up(n, kIdTabBlock)), dim3(kIdTabBlock), 0, st, A);
    }
    if (ev) {  // the registry read and the op rows: of the state the evaluation behind it reads, before any edit
        const EvictStageArgs E{c->ev_in.as<mmp_evicted_entry>(), n, ev->p->self_pod, ev->p->now, ev->p->load_timeout_ms, models, ent_pod, ent_time,
                               cur_side(c).tstats.as<StatsAcc>(), std::max(c->n_types, 1), d_ops, c->ev_out.as<mmp_evicted_out>()};
        hipLaunchKernelGGL(evict_stage_kernel, dim3(div_up(n, kEvictBlock)), dim3(kEvictBlock), 0, st, E);
    }
    hipLaunchKernelGGL(rops_count_kernel, dim3(nb), dim3(kRopsBlock), 0, st, d_ops, n, models, ent_pod, ent_time, pods, P, now, map, rs,
                       c->plan.block_counts.as<int32_t>());
    hipLaunchKernelGGL(prune_scan_kernel, dim3(1), dim3(256), 0, st, c->plan.block_counts.as<int32_t>(), nb, max_edits, INT32_MAX, ps);
    hipLaunchKernelGGL(rops_scatter_kernel, dim3(nb), dim3(kRopsBlock), 0, st, d_ops, n, models, ent_pod, ent_time, pods, P, now, map, rs,
                       c->plan.block_counts.as<int32_t>(), c->plan.edits.as<mmp_registry_op_edit>(), cap_e, c->plan.keep_off.as<int32_t>(), d_status);
    KT_END(c, st);
    HIP_TRY(c, hipGetLastError());
    RopsScalars hr{};
    PruneScalars h{};
    HIP_TRY(c, hipMemcpyAsync(&hr, rs, sizeof hr, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&h, ps, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    c->plan.model_map_n = M;
    kt_collect(c);
    if (hr.n_dup != 0) return fail(c, MMP_EINVAL, "%s: %d ops name a model another op of the call names", fn, hr.n_dup);
    const int32_t ne = std::min(h.n_edits, max_edits);
    if (model_idx_out) {
        if (keyed)
            HIP_TRY(c, copy_sync(c, model_idx_out, c->me_row.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        else
            for (int32_t i = 0; i < n; i++) model_idx_out[i] = ops[i].model;
    }
    if (status_out) HIP_TRY(c, copy_sync(c, status_out, d_status, (size_t)n, hipMemcpyDeviceToHost));
    if (ev) {
        std::vector<uint8_t> stv((size_t)n);
        HIP_TRY(c, copy_sync(c, stv.data(), d_status, (size_t)n, hipMemcpyDeviceToHost));
        HIP_TRY(c, copy_sync(c, ev->outs, c->ev_out.p, (size_t)n * sizeof(mmp_evicted_out), hipMemcpyDeviceToHost));
        for (int32_t i = 0; i < n; i++) ev->outs[i].status = stv[i];
    }
    if (ne > 0) HIP_TRY(c, copy_sync(c, edits_out, c->plan.edits.p, (size_t)ne * sizeof(mmp_registry_op_edit), hipMemcpyDeviceToHost));
    *info = mmp_registry_ops_info_k{};
    info->n_edits = h.n_edits;
    info->n_unchanged = n - h.n_edits - hr.n_no_record;
    info->n_no_record = hr.n_no_record;
    info->truncated = h.truncated;
    for (int k = 0; k < kRopKinds; k++) {
        info->n_edited_op[k] = hr.n_edited[k];
        info->n_unchanged_op[k] = hr.n_unchanged[k];
    }
    info->n_entries_added = hr.n_added;
    info->n_entries_removed = hr.n_removed;
    if (!apply || h.truncated || h.n_edits == 0) return MMP_OK;

    return registry_apply_edits(c, h.n_edits, h.n_kept, edits_out, [&](int32_t base, int32_t arena_end) {  // the records without / with the op's entry
        hipLaunchKernelGGL(rops_build_kernel, dim3(div_up(h.n_edits, 256)), dim3(256), 0, st, c->plan.edits.as<mmp_registry_op_edit>(),
                           c->plan.keep_off.as<int32_t>(), h.n_edits, d_ops, c->models.as<mmp_model_row>(), c->ent_pod.as<int32_t>(),
                           c->ent_time.as<int64_t>(), base, arena_end, c->u_idx.as<int32_t>(), c->u_rows.as<mmp_model_row>());
    });
}
}  // namespace

// by row, kinds 0..3, its own 56-byte info: unchanged since ABI 3 (MMP_ROP_DROP_LOCAL is refused here: mmp_registry_ops_k)
int mmp_registry_ops(mmp_ctx *c, const mmp_registry_op *ops, int32_t n, int64_t now, uint32_t flags, uint8_t *status_out,
                     mmp_registry_op_edit *edits_out, int32_t max_edits, mmp_registry_ops_info *info)
try {
    if (!c || !info || n < 0 || max_edits < 0 || (n > 0 && !ops) || (max_edits > 0 && !edits_out) || now <= 0 ||
        plan_flags_bad(flags))
        return fail(c, MMP_EINVAL, "mmp_registry_ops: bad argument");
    mmp_registry_ops_info_k k{};
    if (const int rc = rops_drive(c, "mmp_registry_ops", MMP_ROP_SCALE_DOWN, ops, n, nullptr, nullptr, now, flags, nullptr, status_out,
                                  edits_out, max_edits, &k))
        return rc;
    *info = mmp_registry_ops_info{};
    info->n_edits = k.n_edits;
    info->n_unchanged = k.n_unchanged;
    info->truncated = k.truncated;
    for (int q = 0; q < 4; q++) {
        info->n_edited_op[q] = k.n_edited_op[q];
        info->n_unchanged_op[q] = k.n_unchanged_op[q];
    }
    info->n_entries_added = k.n_entries_added;
    info->n_entries_removed = k.n_entries_removed;
    return MMP_OK;
} MMP_CATCH(c, "mmp_registry_ops")

// by model id (or by row with keys == key_off == NULL), kinds 0..4
int mmp_registry_ops_k(mmp_ctx *c, const mmp_registry_op *ops, int32_t n, const char *keys, const int32_t *key_off, int64_t now,
                       uint32_t flags, int32_t *model_idx_out, uint8_t *status_out, mmp_registry_op_edit *edits_out, int32_t max_edits,
                       mmp_registry_ops_info_k *info)
try {
    if (!c || !info || n < 0 || max_edits < 0 || (n > 0 && !ops) || (max_edits > 0 && !edits_out) || now <= 0 ||
        plan_flags_bad(flags) || (keys == nullptr) != (key_off == nullptr))
        return fail(c, MMP_EINVAL, "mmp_registry_ops_k: bad argument");
    return rops_drive(c, "mmp_registry_ops_k", MMP_ROP_DROP_LOCAL, ops, n, keys, key_off, now, flags, model_idx_out, status_out, edits_out,
                      max_edits, info);
} MMP_CATCH(c, "mmp_registry_ops_k")

// onEviction's task body by model id: the registry read, the reload decision and the deregistration of one registry state
int mmp_evictions_k(mmp_ctx *c, const mmp_evicted_entry *entries, int32_t n, const char *keys, const int32_t *key_off, const mmp_evict_params *p,
                    uint32_t flags, int32_t *model_idx_out, mmp_evicted_out *outs, uint8_t *status_out, mmp_registry_op_edit *edits_out,
                    int32_t max_edits, mmp_evictions_info *info)
try {
    if (!c || !info || !p || n < 0 || max_edits < 0 || (n > 0 && (!entries || !outs || !key_off)) || (max_edits > 0 && !edits_out) || p->now <= 0 ||
        plan_flags_bad(flags) || (keys == nullptr) != (key_off == nullptr))
        return fail(c, MMP_EINVAL, "mmp_evictions_k: bad argument");
    const RopsEvict ev{entries, p, outs};
    mmp_registry_ops_info_k k{};
    if (const int rc = rops_drive(c, "mmp_evictions_k", MMP_ROP_DROP_LOCAL, nullptr, n, keys, key_off, p->now, flags, model_idx_out, status_out,
                                  edits_out, max_edits, &k, &ev))
        return rc;
    *info = mmp_evictions_info{};
    for (int32_t i = 0; i < n; i++) {
        const uint32_t f = outs[i].flags;
        info->n_in_registry += (f & MMP_EVO_IN_REGISTRY) != 0;
        info->n_attempt_reload += (f & MMP_EVO_ATTEMPT_RELOAD) != 0;
        info->n_reload += (f & MMP_EVO_RELOAD) != 0;
        info->n_log += (f & MMP_EVO_LOG) != 0;
    }
    info->n_no_record = k.n_no_record;
    info->ops = k;
    return MMP_OK;
} MMP_CATCH(c, "mmp_evictions_k")

namespace {
// What a caller of status_drive adds around the pipeline; each defaults to nothing.
struct StatusNoHook {
    int operator()() const { return MMP_OK; }
};

// THE STATUS PIPELINE over device-resident requests (status_kernels.hpp): mmp_models_status behind its host-side validation, shared
// with the calls that write the requests on the device (status_keyed_kernels.hpp).  The caller owns batch_mu, has set the device,
// has refused what it refuses of the requests, and has n > 0 mmp_status_req rows in (or on their way into) c->plan.rows_in — staged
// by a copy it enqueued on c->stream, or written by the kernels `front` launches.  pods / P: the committed rows for the overlay,
// nullptr / 0 when no request carries a fail_pod.  The hooks, all on c->stream:
//   front   launches in front of the count kernel, inside the device span
//   back    further read-backs enqueued beside the pipeline's own, in front of the ONE synchronisation on the sizes
//   sized   the sizes are on the host: what the caller refuses of its own, and the room for what `tail` writes
//   tail    launches behind the emit kernels, inside the device span
// Nothing reaches rows_out / copies_out / n_copies_out before the last step that refuses.
extern "C++" template <class Front = StatusNoHook, class Back = StatusNoHook, class Sized = StatusNoHook, class Tail = StatusNoHook>
int status_drive(mmp_ctx *c, const char *fn, int32_t n, int64_t now, const mmp_pod_row *pods, int32_t P, mmp_status_row *rows_out,
                 mmp_status_copy *copies_out, int32_t max_copies, int32_t *n_copies_out, Front front = Front(), Back back = Back(),
                 Sized sized = Sized(), Tail tail = Tail())
{
    hipStream_t st = c->stream;
    const int nb = div_up(n, kStatusBlock);
    HIP_TRY(c, c->plan.edits.ensure((size_t)n * sizeof(mmp_status_row)));
    HIP_TRY(c, c->plan.keep_off.ensure((size_t)n * sizeof(StatusAux)));
    HIP_TRY(c, c->plan.row_tmp.ensure((size_t)n * 4));
    HIP_TRY(c, c->plan.call_scalars.ensure(std::max(sizeof(StatusScalars), std::max(sizeof(RopsScalars), sizeof(JanitorScalars)))));
    HIP_TRY(c, c->plan.totals.ensure(sizeof(PruneScalars)));
    HIP_TRY(c, c->plan.block_counts.ensure((size_t)nb * 3 * 4));
    const mmp_model_row *models = c->models.as<mmp_model_row>();
    const int32_t *ent_pod = c->ent_pod.as<int32_t>();
    const int64_t *ent_time = c->ent_time.as<int64_t>();
    const mmp_status_req *d_reqs = c->plan.rows_in.as<mmp_status_req>();
    mmp_status_row *d_rows = c->plan.edits.as<mmp_status_row>();
    StatusAux *d_aux = c->plan.keep_off.as<StatusAux>();
    int32_t *d_long = c->plan.row_tmp.as<int32_t>();
    StatusScalars *ss = c->plan.call_scalars.as<StatusScalars>();
    PruneScalars *ps = c->plan.totals.as<PruneScalars>();
    HIP_TRY(c, hipMemsetAsync(ss, 0, sizeof(StatusScalars), st));
    HIP_TRY(c, hipMemsetAsync(ps, 0, sizeof(PruneScalars), st));
    KT_BEGIN(c, st);  // device span: count, scan, offsets — and, behind the one read-back of the sizes, the two emit kernels
    if (const int rc = front()) return rc;
    hipLaunchKernelGGL(status_count_kernel, dim3(nb), dim3(kStatusBlock), 0, st, d_reqs, n, models, ent_pod, pods, P, d_rows, d_aux,
                       c->plan.block_counts.as<int32_t>(), ss);
    hipLaunchKernelGGL(prune_scan_kernel, dim3(1), dim3(256), 0, st, c->plan.block_counts.as<int32_t>(), nb, INT32_MAX, INT32_MAX, ps);
    hipLaunchKernelGGL(status_rows_kernel, dim3(nb), dim3(kStatusBlock), 0, st, n, d_rows, c->plan.block_counts.as<int32_t>(), d_long);
    HIP_TRY(c, hipGetLastError());
    StatusScalars hs{};
    PruneScalars h{};
    HIP_TRY(c, hipMemcpyAsync(&hs, ss, sizeof hs, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&h, ps, sizeof h, hipMemcpyDeviceToHost, st));
    if (const int rc = back()) return rc;
    HIP_TRY(c, hipStreamSynchronize(st));
    if (hs.n_copies > (unsigned long long)INT32_MAX) {
        c->prof_armed = false;
        return fail(c, MMP_EINVAL, "%s: %llu copies in all; split the batch", fn, hs.n_copies);
    }
    if (const int rc = sized()) {
        c->prof_armed = false;
        return rc;
    }
    const int32_t total = h.n_kept, n_long = h.n_edits, take = std::min(total, max_copies);
    if (take > 0) {
        HIP_TRY(c, c->st_copies.ensure((size_t)take * sizeof(mmp_status_copy)));
        mmp_status_copy *d_copies = c->st_copies.as<mmp_status_copy>();
        hipLaunchKernelGGL(status_emit_kernel, dim3(div_up(total, kStatusBlock)), dim3(kStatusBlock), 0, st, d_reqs, n, total, models, ent_pod,
                           ent_time, now, d_rows, d_aux, d_copies, take);
        if (n_long > 0)
            hipLaunchKernelGGL(status_long_kernel, dim3(n_long), dim3(kStatusLongBlock), 0, st, d_reqs, d_long, models, ent_pod, ent_time, now,
                               d_rows, d_aux, d_copies, take);
    }
    if (const int rc = tail()) return rc;
    KT_END(c, st);
    HIP_TRY(c, hipGetLastError());
    // every word of copies[0, take) has exactly one writer above: the ranks of a segment are a permutation of its indices
    if (take > 0) HIP_TRY(c, copy_sync(c, copies_out, c->st_copies.p, (size_t)take * sizeof(mmp_status_copy), hipMemcpyDeviceToHost));
    HIP_TRY(c, copy_sync(c, rows_out, d_rows, (size_t)n * sizeof(mmp_status_row), hipMemcpyDeviceToHost));
    kt_collect(c);
    *n_copies_out = total;
    return MMP_OK;
}
}  // namespace

int mmp_models_status(mmp_ctx *c, const mmp_status_req *reqs, int32_t n, int64_t now, mmp_status_row *rows_out,
                      mmp_status_copy *copies_out, int32_t max_copies, int32_t *n_copies_out)
try {
    if (!c || !n_copies_out || n < 0 || max_copies < 0 || (n > 0 && (!reqs || !rows_out)) || (max_copies > 0 && !copies_out))
        return fail(c, MMP_EINVAL, "mmp_models_status: bad argument");
    // batch_mu owns c->stream and the scratch for the whole call, and every writer of what this call reads — registry events, an
    // applied prune, janitor plan or batch of ops, the loaders of the registry, a commit — takes it too and leaves with its work
    // on c->stream finished.  The state lock is not taken: nothing decisions read is written.
    std::lock_guard<std::mutex> gb(c->batch_mu);
    const int32_t M = c->n_models;
    // the requests index the rows and the instance table: their ranges are settled here, before any kernel reads them
    bool overlay = false;
    for (int32_t i = 0; i < n; i++) {
        const mmp_status_req &q = reqs[i];
        if (q.model < -1 || q.model >= M) return fail(c, MMP_EINVAL, "mmp_models_status: request %d names model %d of %d", i, q.model, M);
        if (q.fail_pod < -1) return fail(c, MMP_EINVAL, "mmp_models_status: request %d names pod %d", i, q.fail_pod);
        if ((q.flags & ~MMP_MSTF_MISS) || q.reserved) return fail(c, MMP_EINVAL, "mmp_models_status: request %d has flags %u, reserved %u", i, q.flags, q.reserved);
        overlay |= q.fail_pod >= 0;
    }
    int32_t P = 0;
    const mmp_pod_row *pods = nullptr;  // the committed rows, read for id_order by the overlay alone
    if (overlay) {
        if (now <= 0) return fail(c, MMP_EINVAL, "mmp_models_status: now_ms = %lld with a fail_pod", (long long)now);
        if (const int rc = plan_state_guard(c, "mmp_models_status")) return rc;
        P = c->snap.P;
        pods = c->sb[c->cur].pods.as<mmp_pod_row>();
        for (int32_t i = 0; i < n; i++)
            if (reqs[i].fail_pod >= P) return fail(c, MMP_EINVAL, "mmp_models_status: request %d names pod %d of %d", i, reqs[i].fail_pod, P);
    }
    if (n == 0) {
        *n_copies_out = 0;
        return MMP_OK;
    }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, c->plan.rows_in.ensure((size_t)n * sizeof(mmp_status_req)));
    HIP_TRY(c, hipMemcpyAsync(c->plan.rows_in.p, reqs, (size_t)n * sizeof(mmp_status_req), hipMemcpyHostToDevice, c->stream));
    return status_drive(c, "mmp_models_status", n, now, pods, P, rows_out, copies_out, max_copies, n_copies_out);
} MMP_CATCH(c, "mmp_models_status")

// getStatus by model id: the keys resolved and the requests written on the device, in front of the pipeline (status_keyed_kernel).
int mmp_models_status_k(mmp_ctx *c, const char *keys, const int32_t *key_off, int32_t n, const int32_t *fail_pod, const uint32_t *flags,
                        int64_t now, int32_t *model_idx_out, mmp_status_row *rows_out, mmp_status_copy *copies_out, int32_t max_copies,
                        int32_t *n_copies_out)
try {
    if (!c || !n_copies_out || n < 0 || max_copies < 0 || (n > 0 && (!key_off || !rows_out)) || (max_copies > 0 && !copies_out))
        return fail(c, MMP_EINVAL, "mmp_models_status_k: bad argument");
    // the locking of mmp_models_status; the model-id table is batch_mu's as well (mmp_model_ids_resolve)
    std::lock_guard<std::mutex> gb(c->batch_mu);
    if (const int rc = model_id_space_guard(c, "mmp_models_status_k")) return rc;
    // (everything that is refused, before anything is staged)
    if (const int rc = check_offsets(c, "mmp_models_status_k", "key ", key_off, n)) return rc;
    if (n > 0 && key_off[n] > key_off[0] && !keys) return fail(c, MMP_EINVAL, "mmp_models_status_k: bad argument");
    bool overlay = false;
    for (int32_t i = 0; i < n; i++) {
        if (fail_pod && fail_pod[i] < -1) return fail(c, MMP_EINVAL, "mmp_models_status_k: request %d names pod %d", i, fail_pod[i]);
        if (flags && (flags[i] & ~MMP_MSTF_MISS)) return fail(c, MMP_EINVAL, "mmp_models_status_k: request %d has flags %u", i, flags[i]);
        overlay |= fail_pod && fail_pod[i] >= 0;
    }
    int32_t P = 0;
    const mmp_pod_row *pods = nullptr;  // the committed rows, read for id_order by the overlay alone
    if (overlay) {
        if (now <= 0) return fail(c, MMP_EINVAL, "mmp_models_status_k: now_ms = %lld with a fail_pod", (long long)now);
        if (const int rc = plan_state_guard(c, "mmp_models_status_k")) return rc;
        P = c->snap.P;
        pods = c->sb[c->cur].pods.as<mmp_pod_row>();
        for (int32_t i = 0; i < n; i++)
            if (fail_pod[i] >= P) return fail(c, MMP_EINVAL, "mmp_models_status_k: request %d names pod %d of %d", i, fail_pod[i], P);
    }
    if (n == 0) {
        *n_copies_out = 0;
        return MMP_OK;
    }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    std::vector<int32_t> krel;
    if (const int rc = stage_strings(c, "mmp_models_status_k", "key ", keys, key_off, n, c->ida_bytes, c->ida_off, krel)) return rc;
    HIP_TRY(c, c->me_row.ensure((size_t)n * 4));
    HIP_TRY(c, c->plan.rows_in.ensure((size_t)n * sizeof(mmp_status_req)));
    if (fail_pod) {
        HIP_TRY(c, c->sk_fpod.ensure((size_t)n * 4));
        HIP_TRY(c, hipMemcpyAsync(c->sk_fpod.p, fail_pod, (size_t)n * 4, hipMemcpyHostToDevice, st));
    }
    if (flags) {
        HIP_TRY(c, c->sk_flags.ensure((size_t)n * 4));
        HIP_TRY(c, hipMemcpyAsync(c->sk_flags.p, flags, (size_t)n * 4, hipMemcpyHostToDevice, st));
    }
    // (the staged copy keeps keyed_resolve_kernel's contract: the buffer is an allocation of its own with 16 bytes behind the keys)
    const StKeyArgs A{c->ida_bytes.as<char>(), c->ida_off.as<int32_t>(), n, hash_mask(c->tune.model_id_hash_bits), vmodel_models(c),
                      fail_pod ? c->sk_fpod.as<int32_t>() : nullptr, flags ? c->sk_flags.as<uint32_t>() : nullptr, c->me_row.as<int32_t>(),
                      c->plan.rows_in.as<mmp_status_req>()};
    const int rc = status_drive(c, "mmp_models_status_k", n, now, pods, P, rows_out, copies_out, max_copies, n_copies_out, [&]() -> int {
        hipLaunchKernelGGL(status_keyed_kernel, dim3(div_up(n, kIdTabBlock)), dim3(kIdTabBlock), 0, st, A);
        return MMP_OK;
    });
    if (rc) return rc;
    if (model_idx_out) HIP_TRY(c, copy_sync(c, model_idx_out, c->me_row.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return MMP_OK;
} MMP_CATCH(c, "mmp_models_status_k")

// getVModelStatus in full: the vmodel keys resolved, the vrows, both requests per vmodel and the string lengths written on the
// device in front of the pipeline (vstatus_keyed_kernel); the strings copied behind its one read-back of the sizes.
int mmp_vmodels_status(mmp_ctx *c, const char *keys, const int32_t *key_off, int32_t n, const char *owners, const int32_t *owner_off,
                       const uint32_t *req_flags, int64_t now, mmp_vstatus_row *vrows_out, mmp_status_row *rows_out,
                       mmp_status_copy *copies_out, int32_t max_copies, int32_t *n_copies_out, char *str_bytes_out, int32_t max_str_bytes,
                       int32_t *str_off_out, int32_t *n_str_bytes_out)
try {
    if (!c || !n_copies_out || !n_str_bytes_out || n < 0 || max_copies < 0 || max_str_bytes < 0 ||
        (n > 0 && (!key_off || !vrows_out || !rows_out)) || (max_copies > 0 && !copies_out) || (max_str_bytes > 0 && !str_bytes_out))
        return fail(c, MMP_EINVAL, "mmp_vmodels_status: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);  // the locking of mmp_vmodels_resolve and mmp_models_status: one hold for the whole answer
    if (const int rc = model_id_space_guard(c, "mmp_vmodels_status")) return rc;
    if (n > INT32_MAX / 8) return fail(c, MMP_EINVAL, "mmp_vmodels_status: %d keys in one call", n);
    // (both kinds and the flags, before anything is staged)
    if (const int rc = check_offsets(c, "mmp_vmodels_status", "key ", key_off, n)) return rc;
    if (owner_off)
        if (const int rc = check_offsets(c, "mmp_vmodels_status", "owner ", owner_off, n)) return rc;
    if (n > 0 && ((key_off[n] > key_off[0] && !keys) || (owner_off && owner_off[n] > owner_off[0] && !owners)))
        return fail(c, MMP_EINVAL, "mmp_vmodels_status: bad argument");
    if (req_flags)
        for (int32_t i = 0; i < n; i++)
            if (req_flags[i] & ~MMP_VMRQ_AFTER_STRONG) return fail(c, MMP_EINVAL, "mmp_vmodels_status: request %d has unknown flag bits", i);
    if (n == 0) {
        *n_copies_out = 0;
        *n_str_bytes_out = 0;
        if (str_off_out) str_off_out[0] = 0;
        return MMP_OK;
    }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    std::vector<int32_t> krel, orel;
    if (const int rc = stage_strings(c, "mmp_vmodels_status", "key ", keys, key_off, n, c->ida_bytes, c->ida_off, krel)) return rc;
    if (owner_off)
        if (const int rc = stage_strings(c, "mmp_vmodels_status", "owner ", owners, owner_off, n, c->vm_ow_bytes, c->vm_ow_off, orel)) return rc;
    if (req_flags) {
        HIP_TRY(c, c->vm_rflags.ensure((size_t)n * 4));
        HIP_TRY(c, hipMemcpyAsync(c->vm_rflags.p, req_flags, (size_t)n * 4, hipMemcpyHostToDevice, st));
    }
    const size_t n_str = 3 * (size_t)n;
    HIP_TRY(c, c->vm_ans.ensure((size_t)n * sizeof(mmp_vstatus_row)));
    HIP_TRY(c, c->plan.rows_in.ensure(2 * (size_t)n * sizeof(mmp_status_req)));
    HIP_TRY(c, c->j_cnt.ensure((n_str + 1) * 4));
    HIP_TRY(c, c->j_offs.ensure((n_str + 1) * 4));
    HIP_TRY(c, c->sk_sc.ensure(sizeof(VStKeyScalars)));
    int32_t *d_len = c->j_cnt.as<int32_t>(), *d_pos = c->j_offs.as<int32_t>();
    size_t scan_bytes = 0;
    HIP_TRY(c, rocprim::exclusive_scan(nullptr, scan_bytes, d_len, d_pos, (int32_t)0, n_str + 1, rocprim::plus<int32_t>(), st));
    HIP_TRY(c, c->j_scan_tmp.ensure(std::max<size_t>(scan_bytes, 16)));
    HIP_TRY(c, hipMemsetAsync(c->sk_sc.p, 0, sizeof(VStKeyScalars), st));
    const VmTab V = vmodel_tab(c);
    const VStKeyArgs A{c->ida_bytes.as<char>(), c->ida_off.as<int32_t>(), owner_off ? c->vm_ow_bytes.as<char>() : nullptr,
                       owner_off ? c->vm_ow_off.as<int32_t>() : nullptr, req_flags ? c->vm_rflags.as<uint32_t>() : nullptr, n,
                       hash_mask(c->tune.vmodel_id_hash_bits), V, vmodel_models(c), c->vm_ans.as<mmp_vstatus_row>(),
                       c->plan.rows_in.as<mmp_status_req>(), d_len, c->sk_sc.as<VStKeyScalars>()};
    VStKeyScalars hv{};
    bool want_str = false;
    const int rc = status_drive(
        c, "mmp_vmodels_status", 2 * n, now, nullptr, 0, rows_out, copies_out, max_copies, n_copies_out,
        [&]() -> int {  // the requests, and the strings' lengths scanned
            hipLaunchKernelGGL(vstatus_keyed_kernel, dim3(div_up(n, kIdTabBlock)), dim3(kIdTabBlock), 0, st, A);
            HIP_TRY(c, rocprim::exclusive_scan(c->j_scan_tmp.p, scan_bytes, d_len, d_pos, (int32_t)0, n_str + 1, rocprim::plus<int32_t>(), st));
            return MMP_OK;
        },
        [&]() -> int {  // the strings' total, read back with the copy total
            HIP_TRY(c, hipMemcpyAsync(&hv, c->sk_sc.p, sizeof hv, hipMemcpyDeviceToHost, st));
            return MMP_OK;
        },
        [&]() -> int {
            if (hv.n_str_bytes > (unsigned long long)INT32_MAX)
                return fail(c, MMP_EINVAL, "mmp_vmodels_status: %llu string bytes in all; split the batch", hv.n_str_bytes);
            want_str = hv.n_str_bytes > 0 && (unsigned long long)max_str_bytes >= hv.n_str_bytes;
            if (want_str) HIP_TRY(c, c->sk_str.ensure((size_t)hv.n_str_bytes));
            return MMP_OK;
        },
        [&]() -> int {
            if (want_str)
                hipLaunchKernelGGL(vstatus_strings_kernel, dim3(div_up((int)n_str, 256)), dim3(256), 0, st, A.vrows, (int32_t)n_str, d_pos, V,
                                   c->sk_str.as<char>());
            return MMP_OK;
        });
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(vrows_out, c->vm_ans.p, (size_t)n * sizeof(mmp_vstatus_row), hipMemcpyDeviceToHost, st));
    if (str_off_out) HIP_TRY(c, hipMemcpyAsync(str_off_out, d_pos, (n_str + 1) * 4, hipMemcpyDeviceToHost, st));
    if (want_str) HIP_TRY(c, hipMemcpyAsync(str_bytes_out, c->sk_str.p, (size_t)hv.n_str_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    *n_str_bytes_out = (int32_t)hv.n_str_bytes;
    return MMP_OK;
} MMP_CATCH(c, "mmp_vmodels_status")

// THE TWO-PASS FRAME of the "next stored value" calls (rewrite_kernels.hpp, register_kernels.hpp): stored values in, rendered
// values out.  The caller (owner of batch_mu, the device set, every refusal behind it) has staged its own inputs and filled its
// own members of A; the frame stages the stored values where the parser reads them and fills StoredArgs.  Size bracket: `front`
// (launches in front of the parser), the parser stage the caller names (ModelValueParser / VModelValueParser below), the size
// pass, the scan of the sizes; then the ONE read-back — the offsets and every array of `back` — that decides whether anything is
// written; write bracket: the write pass and the copy of the bytes, where out_buf holds them.  Nothing reaches the caller's
// arrays before the last step that can fail, and the call's device span is the sum of the two brackets.
struct RenderBack {
    void *host;  // the caller's array (nullptr with 0 bytes: not asked for)
    const DevBuf *dev;
    size_t bytes;
};
// The parser stage over ModelRecord values: ingest_models_kernel as over non-deleted events (rows and entries into scratch).
struct ModelValueParser {
    IngestModelsArgs J;
    int prepare(mmp_ctx *c, int32_t n, int64_t bytes, StoredArgs &A)
    {
        size_t ent_cap;
        if (const int rc = ingest_models_args(c, n, bytes, J, ent_cap)) return rc;
        HIP_TRY(c, c->j_rows.ensure((size_t)n * sizeof(mmp_model_row)));
        J.rows = c->j_rows.as<mmp_model_row>();
        A.buf = J.buf;
        A.off = J.off;
        A.pstatus = J.status;
        A.prow = J.rows;
        return MMP_OK;
    }
    void launch(int32_t n, hipStream_t st) const
    {
        hipLaunchKernelGGL(ingest_models_kernel, dim3(div_up(n, kJWaves * J.grp)), dim3(kJBlock), 0, st, J);
    }
};
// The parser stage over VModelRecord values: vm_parse_kernel as over non-deleted events, every event on the one slot of a table
// nobody reads (the winner rule has nothing to decide here).
struct VModelValueParser {
    VmParseArgs J;
    int prepare(mmp_ctx *c, int32_t n, int64_t, StoredArgs &A)
    {
        HIP_TRY(c, c->j_ev.ensure(((size_t)n + 1) * 4));
        HIP_TRY(c, c->vm_ev.ensure((size_t)n * sizeof(VmEvent)));
        HIP_TRY(c, c->j_status.ensure((size_t)n * 4));
        int32_t *slot = c->j_ev.as<int32_t>();
        HIP_TRY(c, hipMemsetAsync(slot, 0, (size_t)n * 4, c->stream));
        HIP_TRY(c, hipMemsetAsync(slot + n, 0xff, 4, c->stream));
        J = VmParseArgs{c->j_buf.as<char>(), c->j_off.as<int64_t>(), n, ingest_group(n), nullptr, slot, slot + n, c->vm_ev.as<VmEvent>(),
                        c->j_status.as<int32_t>()};
        A.buf = J.buf;
        A.off = J.off;
        A.pstatus = J.status;
        A.pev = J.ev;
        return MMP_OK;
    }
    void launch(int32_t n, hipStream_t st) const { hipLaunchKernelGGL(vm_parse_kernel, dim3(div_up(n, kJWaves * J.grp)), dim3(kJBlock), 0, st, J); }
};
extern "C++" template <class Args, class Parser, class Front>
int render_stored_values(mmp_ctx *c, const char *fn, const char *old_buf, const int64_t *old_off, int32_t n, Args &A, Parser &&parser,
                         void (*size_pass)(Args), void (*write_pass)(Args), Front &&front, std::initializer_list<RenderBack> back, char *out_buf, int64_t out_cap,
                         int64_t *out_off, int64_t *n_bytes_out)
{
    hipStream_t st = c->stream;
    std::vector<int64_t> rel;
    if (const int rc = stage_strings(c, fn, "", old_buf, old_off, n, c->j_buf, c->j_off, rel)) return rc;
    if (const int rc = parser.prepare(c, n, rel[n], A)) return rc;
    HIP_TRY(c, c->rw_len.ensure((size_t)(n + 1) * 8));
    HIP_TRY(c, c->rw_off.ensure((size_t)(n + 1) * 8));
    int64_t *d_len = c->rw_len.as<int64_t>(), *d_off = c->rw_off.as<int64_t>();
    size_t scan_bytes = 0;
    HIP_TRY(c, rocprim::exclusive_scan(nullptr, scan_bytes, d_len, d_off, (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>(), st));
    HIP_TRY(c, c->j_scan_tmp.ensure(std::max<size_t>(scan_bytes, 16)));
    HIP_TRY(c, hipMemsetAsync(d_len + n, 0, 8, st));
    A.n = n;
    A.len = d_len;
    A.out_off = d_off;
    const dim3 grid(div_up(n, kJWaves)), block(kJBlock);
    KT_BEGIN(c, st);
    front();
    parser.launch(n, st);
    hipLaunchKernelGGL(size_pass, grid, block, 0, st, A);
    HIP_TRY(c, rocprim::exclusive_scan(c->j_scan_tmp.p, scan_bytes, d_len, d_off, (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>(), st));
    KT_END(c, st);
    HIP_TRY(c, hipGetLastError());
    std::vector<int64_t> h_off((size_t)n + 1);
    std::vector<std::vector<char>> h_back;
    HIP_TRY(c, hipMemcpyAsync(h_off.data(), d_off, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, st));
    for (const RenderBack &b : back) {
        h_back.emplace_back(b.bytes);
        if (b.bytes) HIP_TRY(c, hipMemcpyAsync(h_back.back().data(), b.dev->p, b.bytes, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(c, hipStreamSynchronize(st));
    kt_collect(c);
    const double size_ms = c->last_kernel_ms;
    const int64_t total = h_off[n];
    if (out_buf && out_cap >= total && total > 0) {
        HIP_TRY(c, c->rw_out.ensure((size_t)total));
        A.out = c->rw_out.as<char>();
        KT_BEGIN(c, st);
        hipLaunchKernelGGL(write_pass, grid, block, 0, st, A);
        KT_END(c, st);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, copy_sync(c, out_buf, c->rw_out.p, (size_t)total, hipMemcpyDeviceToHost));
        kt_collect(c);
        kt_add(c, size_ms);  // the call's device span: size + write
    }
    memcpy(out_off, h_off.data(), (size_t)(n + 1) * 8);
    for (size_t k = 0; k < back.size(); k++)
        if (back.begin()[k].bytes) memcpy(back.begin()[k].host, h_back[k].data(), back.begin()[k].bytes);
    *n_bytes_out = total;
    return MMP_OK;
}

int mmp_models_rewrite_json(mmp_ctx *c, const int32_t *rows, int32_t n, const char *old_buf, const int64_t *old_off,
                            const int64_t *last_unload, const int32_t *fail_pod, const char *fail_msg, const int32_t *fail_msg_off,
                            uint32_t flags, char *out_buf, int64_t out_cap, int64_t *out_off, int32_t *status_out, int64_t *n_bytes_out)
try {
    if (!c || n < 0 || flags || out_cap < 0 || !out_off || !n_bytes_out || (n > 0 && (!rows || !old_off || !status_out)) ||
        (fail_pod && (!fail_msg || !fail_msg_off)))
        return fail(c, MMP_EINVAL, "mmp_models_rewrite_json: bad argument");
    // read-only: the locking of mmp_models_status without a fail_pod (batch_mu owns the stream, the scratch, the registry's
    // writers and the id store's)
    std::lock_guard<std::mutex> gb(c->batch_mu);
    if (!c->have_ids) return fail(c, MMP_ESTATE, "mmp_models_rewrite_json: load the instance ids first (mmp_pod_ids_load)");
    if (const int rc = id_space_guard(c, "mmp_models_rewrite_json")) return rc;
    const int32_t M = c->n_models, P = (int32_t)c->pods.size();
    if (const int rc = check_offsets(c, "mmp_models_rewrite_json", "", old_off, n)) return rc;
    if (fail_pod)
        if (const int rc = check_offsets(c, "mmp_models_rewrite_json", "message ", fail_msg_off, n)) return rc;
    for (int32_t i = 0; i < n; i++) {
        if (rows[i] < 0 || rows[i] >= M) return fail(c, MMP_EINVAL, "mmp_models_rewrite_json: value %d names model %d of %d", i, rows[i], M);
        if (fail_pod && (fail_pod[i] < -1 || fail_pod[i] >= P))
            return fail(c, MMP_EINVAL, "mmp_models_rewrite_json: value %d names pod %d of %d", i, fail_pod[i], P);
    }
    if (n > 0 && old_off[n] > old_off[0] && !old_buf) return fail(c, MMP_EINVAL, "mmp_models_rewrite_json: bad argument");
    if (n == 0) {
        out_off[0] = 0;
        *n_bytes_out = 0;
        return MMP_OK;
    }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    // the call's own inputs
    std::vector<int32_t> mrel;
    HIP_TRY(c, c->rw_rows.ensure((size_t)n * 4));
    HIP_TRY(c, hipMemcpyAsync(c->rw_rows.p, rows, (size_t)n * 4, hipMemcpyHostToDevice, st));
    if (last_unload) {
        HIP_TRY(c, c->rw_lul.ensure((size_t)n * 8));
        HIP_TRY(c, hipMemcpyAsync(c->rw_lul.p, last_unload, (size_t)n * 8, hipMemcpyHostToDevice, st));
    }
    if (fail_pod) {
        HIP_TRY(c, c->rw_fpod.ensure((size_t)n * 4));
        HIP_TRY(c, hipMemcpyAsync(c->rw_fpod.p, fail_pod, (size_t)n * 4, hipMemcpyHostToDevice, st));
        if (const int rc = stage_strings(c, "mmp_models_rewrite_json", "message ", fail_msg, fail_msg_off, n, c->rw_fmsg, c->rw_fmoff, mrel))
            return rc;
    }
    if (c->idd_gen != c->id_gen) {  // the id store moved since the last call: its device copy follows
        HIP_TRY(c, c->idd_bytes.ensure(c->id_bytes.size() + 16));
        HIP_TRY(c, c->idd_off.ensure(c->id_offs.size() * 4));
        if (!c->id_bytes.empty())
            HIP_TRY(c, hipMemcpyAsync(c->idd_bytes.p, c->id_bytes.data(), c->id_bytes.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipMemcpyAsync(c->idd_off.p, c->id_offs.data(), c->id_offs.size() * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipStreamSynchronize(st));  // (the host store may change once batch_mu is released)
        c->idd_gen = c->id_gen;
    }
    HIP_TRY(c, c->rw_status.ensure((size_t)n * 4));
    RewriteArgs A{};
    A.rows = c->rw_rows.as<int32_t>();
    A.models = c->models.as<mmp_model_row>();
    A.ent_pod = c->ent_pod.as<int32_t>();
    A.ent_time = c->ent_time.as<int64_t>();
    A.id_bytes = c->idd_bytes.as<char>();
    A.id_off = c->idd_off.as<int32_t>();
    A.n_pods = P;
    A.last_unload = last_unload ? c->rw_lul.as<int64_t>() : nullptr;
    A.fail_pod = fail_pod ? c->rw_fpod.as<int32_t>() : nullptr;
    A.fail_msg = fail_pod ? c->rw_fmsg.as<char>() : nullptr;
    A.fail_msg_off = fail_pod ? c->rw_fmoff.as<int32_t>() : nullptr;
    A.status = c->rw_status.as<int32_t>();
    return render_stored_values(c, "mmp_models_rewrite_json", old_buf, old_off, n, A, ModelValueParser(), models_rewrite_kernel<false>,
                                models_rewrite_kernel<true>,
                                [] {}, {{status_out, &c->rw_status, (size_t)n * 4}}, out_buf, out_cap, out_off, n_bytes_out);
} MMP_CATCH(c, "mmp_models_rewrite_json")

int mmp_models_register_json(mmp_ctx *c, const mmp_register_req *reqs, int32_t n, const char *keys, const int32_t *key_off,
                             const char *info, const int32_t *info_off, const char *old_buf, const int64_t *old_off, int64_t now_ms,
                             int64_t lastused_age_on_add_ms, uint32_t flags, char *out_buf, int64_t out_cap, int64_t *out_off,
                             int32_t *class_out, int64_t *last_used_out, int32_t *model_idx_out, int64_t *n_bytes_out)
try {
    const char *fn = "mmp_models_register_json";
    if (!c || n < 0 || n > INT32_MAX / 3 - 1 || flags || out_cap < 0 || !out_off || !n_bytes_out ||
        (n > 0 && (!reqs || !info_off || !old_off || !class_out || !last_used_out || (model_idx_out && !key_off))))
        return fail(c, MMP_EINVAL, "%s: bad argument", fn);
    if (now_ms <= 0 || lastused_age_on_add_ms < 0)
        return fail(c, MMP_EINVAL, "%s: now_ms = %lld, lastused_age_on_add_ms = %lld", fn, (long long)now_ms, (long long)lastused_age_on_add_ms);
    // read-only: the locking of mmp_models_status without a fail_pod (batch_mu owns the stream, the scratch, and the writers of the
    // id tables the two by-key stages read)
    std::lock_guard<std::mutex> gb(c->batch_mu);
    if (!c->have_ids) return fail(c, MMP_ESTATE, "%s: load the instance ids first (mmp_pod_ids_load)", fn);
    if (model_idx_out)
        if (const int rc = model_id_space_guard(c, fn)) return rc;
    // every refusal stands before anything is staged or written: the three kinds of offsets, then the requests
    if (const int rc = check_offsets(c, fn, "", old_off, n)) return rc;
    if (const int rc = check_offsets(c, fn, "info ", info_off, 3 * n)) return rc;
    if (model_idx_out)
        if (const int rc = check_offsets(c, fn, "key ", key_off, n)) return rc;
    for (int32_t i = 0; i < n; i++) {
        const mmp_register_req &q = reqs[i];
        if ((q.flags & ~(MMP_MREG_LOAD_NOW | MMP_MREG_DELETE)) || q.reserved)
            return fail(c, MMP_EINVAL, "%s: request %d has flags %u, reserved %d", fn, i, q.flags, q.reserved);
        if (!(q.flags & MMP_MREG_DELETE) && info_off[3 * i + 1] == info_off[3 * i])
            return fail(c, MMP_EINVAL, "%s: request %d registers an empty type", fn, i);
        if (old_off[i + 1] - old_off[i] >= INT32_MAX) return fail(c, MMP_EINVAL, "%s: value %d holds 2^31 bytes or more", fn, i);
    }
    if (n > 0 && ((old_off[n] > old_off[0] && !old_buf) || (info_off[3 * n] > info_off[0] && !info) ||
                  (model_idx_out && key_off[n] > key_off[0] && !keys)))
        return fail(c, MMP_EINVAL, "%s: bad argument", fn);
    if (n == 0) {
        out_off[0] = 0;
        *n_bytes_out = 0;
        return MMP_OK;
    }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    // the requests, their strings, and the keys where the by-key stage reads them
    std::vector<int32_t> irel, krel;
    if (const int rc = stage_strings(c, fn, "info ", info, info_off, 3 * n, c->rg_info, c->rg_ioff, irel)) return rc;
    if (model_idx_out) {
        if (const int rc = stage_strings(c, fn, "key ", keys, key_off, n, c->ida_bytes, c->ida_off, krel)) return rc;
        HIP_TRY(c, c->me_hash.ensure((size_t)n * 8));
        HIP_TRY(c, c->me_row.ensure((size_t)n * 4));
    }
    HIP_TRY(c, c->rg_reqs.ensure((size_t)n * sizeof(mmp_register_req)));
    HIP_TRY(c, hipMemcpyAsync(c->rg_reqs.p, reqs, (size_t)n * sizeof(mmp_register_req), hipMemcpyHostToDevice, st));
    HIP_TRY(c, c->rg_cls.ensure((size_t)n * 4));
    HIP_TRY(c, c->rg_lu.ensure((size_t)n * 8));
    RegisterArgs A{};
    A.reqs = c->rg_reqs.as<mmp_register_req>();
    A.info = c->rg_info.as<char>();
    A.info_off = c->rg_ioff.as<int32_t>();
    A.now = now_ms;
    A.age = lastused_age_on_add_ms;
    A.cls = c->rg_cls.as<int32_t>();
    A.last_used = c->rg_lu.as<int64_t>();
    const auto by_key = [&] {  // the rows of the keys, in front of the parser
        if (model_idx_out) mid_resolve_launch(c, n, model_id_tab(c).published(), c->tune.model_id_hash_bits);
    };
    return render_stored_values(c, fn, old_buf, old_off, n, A, ModelValueParser(), models_register_kernel<false>,
                                models_register_kernel<true>, by_key,
                                {{class_out, &c->rg_cls, (size_t)n * 4},
                                 {last_used_out, &c->rg_lu, (size_t)n * 8},
                                 {model_idx_out, &c->me_row, model_idx_out ? (size_t)n * 4 : 0}},
                                out_buf, out_cap, out_off, n_bytes_out);
} MMP_CATCH(c, "mmp_models_register_json")

int mmp_models_refs_json(mmp_ctx *c, const mmp_refs_req *reqs, int32_t n, const char *info, const int32_t *info_off, const char *old_buf,
                         const int64_t *old_off, uint32_t flags, char *out_buf, int64_t out_cap, int64_t *out_off, int32_t *class_out,
                         int32_t *refs_out, int64_t *n_bytes_out)
try {
    const char *fn = "mmp_models_refs_json";
    if (!c || n < 0 || n > INT32_MAX / 3 - 1 || flags || out_cap < 0 || !out_off || !n_bytes_out ||
        (n > 0 && (!reqs || !old_off || !class_out || !refs_out)))
        return fail(c, MMP_EINVAL, "%s: bad argument", fn);
    // read-only: the locking of mmp_models_register_json
    std::lock_guard<std::mutex> gb(c->batch_mu);
    if (!c->have_ids) return fail(c, MMP_ESTATE, "%s: load the instance ids first (mmp_pod_ids_load)", fn);
    // every refusal stands before anything is staged or written: the two kinds of offsets, then the requests
    if (const int rc = check_offsets(c, fn, "", old_off, n)) return rc;
    if (info_off)
        if (const int rc = check_offsets(c, fn, "info ", info_off, 3 * n)) return rc;
    for (int32_t i = 0; i < n; i++) {
        const mmp_refs_req &q = reqs[i];
        if ((q.flags & ~(MMP_MREF_INC | MMP_MREF_AUTO_DELETE)) || q.reserved)
            return fail(c, MMP_EINVAL, "%s: request %d has flags %u, reserved %d", fn, i, q.flags, q.reserved);
        if (old_off[i + 1] - old_off[i] >= INT32_MAX) return fail(c, MMP_EINVAL, "%s: value %d holds 2^31 bytes or more", fn, i);
    }
    if (n > 0 && ((old_off[n] > old_off[0] && !old_buf) || (info_off && info_off[3 * n] > info_off[0] && !info)))
        return fail(c, MMP_EINVAL, "%s: bad argument", fn);
    if (n == 0) {
        out_off[0] = 0;
        *n_bytes_out = 0;
        return MMP_OK;
    }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    // the requests and their strings (no info: 3n empty spans)
    std::vector<int32_t> irel, none;
    if (!info_off) none.assign((size_t)3 * n + 1, 0);
    if (const int rc = stage_strings(c, fn, "info ", info, info_off ? info_off : none.data(), 3 * n, c->rg_info, c->rg_ioff, irel)) return rc;
    HIP_TRY(c, c->rg_reqs.ensure((size_t)n * sizeof(mmp_refs_req)));
    HIP_TRY(c, hipMemcpyAsync(c->rg_reqs.p, reqs, (size_t)n * sizeof(mmp_refs_req), hipMemcpyHostToDevice, st));
    HIP_TRY(c, c->rg_cls.ensure((size_t)n * 4));
    HIP_TRY(c, c->rf_refs.ensure((size_t)n * 4));
    RefsArgs A{};
    A.reqs = c->rg_reqs.as<mmp_refs_req>();
    A.info = c->rg_info.as<char>();
    A.info_off = c->rg_ioff.as<int32_t>();
    A.cls = c->rg_cls.as<int32_t>();
    A.refs = c->rf_refs.as<int32_t>();
    return render_stored_values(c, fn, old_buf, old_off, n, A, ModelValueParser(), models_refs_kernel<false>,
                                models_refs_kernel<true>, [] {},
                                {{class_out, &c->rg_cls, (size_t)n * 4}, {refs_out, &c->rf_refs, (size_t)n * 4}}, out_buf, out_cap,
                                out_off, n_bytes_out);
} MMP_CATCH(c, "mmp_models_refs_json")

int mmp_vmodels_write_json(mmp_ctx *c, const mmp_vmodel_write_req *reqs, int32_t n, const char *strs, const int32_t *str_off,
                           const char *default_owner, int32_t default_owner_len, const char *old_buf, const int64_t *old_off, int64_t now_ms,
                           int64_t lastused_age_on_add_ms, uint32_t flags, char *out_buf, int64_t out_cap, int64_t *out_off,
                           mmp_vmodel_write_row *rows_out, int64_t *n_bytes_out)
try {
    const char *fn = "mmp_vmodels_write_json";
    if (!c || n < 0 || n > INT32_MAX / 3 - 1 || flags || out_cap < 0 || !out_off || !n_bytes_out || default_owner_len < 0 ||
        (default_owner_len > 0 && !default_owner) || (n > 0 && (!reqs || !str_off || !old_off || !rows_out)))
        return fail(c, MMP_EINVAL, "%s: bad argument", fn);
    if (now_ms <= 0 || lastused_age_on_add_ms < 0)
        return fail(c, MMP_EINVAL, "%s: now_ms = %lld, lastused_age_on_add_ms = %lld", fn, (long long)now_ms, (long long)lastused_age_on_add_ms);
    // read-only: the locking of mmp_vmodels_resolve (batch_mu owns the stream, the scratch, and the writers of the model-id table
    // and the registry this call reads)
    std::lock_guard<std::mutex> gb(c->batch_mu);
    if (const int rc = model_id_space_guard(c, fn)) return rc;
    // every refusal stands before anything is staged or written: the two kinds of offsets, then the requests
    if (const int rc = check_offsets(c, fn, "", old_off, n)) return rc;
    if (const int rc = check_offsets(c, fn, "string ", str_off, 3 * n)) return rc;
    constexpr uint32_t kSetFlags = MMP_VWQ_UPDATE_ONLY | MMP_VWQ_FORCE | MMP_VWQ_LOAD_NOW | MMP_VWQ_TARGET_EXISTS | MMP_VWQ_TARGET_LOADED |
                                   MMP_VWQ_TARGET_NOT_LOADED | MMP_VWQ_FAILED;
    for (int32_t i = 0; i < n; i++) {
        const mmp_vmodel_write_req &q = reqs[i];
        if (q.op > MMP_VW_FAIL_FLAG || (q.flags & ~kSetFlags))
            return fail(c, MMP_EINVAL, "%s: request %d has op %u, flags %u", fn, i, q.op, q.flags);
        if ((q.flags & MMP_VWQ_TARGET_LOADED) && (q.flags & MMP_VWQ_TARGET_NOT_LOADED))
            return fail(c, MMP_EINVAL, "%s: request %d says the target is loaded and not loaded", fn, i);
        if ((q.op == MMP_VW_SET || q.op == MMP_VW_COMPLETE) && str_off[3 * i + 1] == str_off[3 * i])
            return fail(c, MMP_EINVAL, "%s: request %d brings no id_a", fn, i);
        if (old_off[i + 1] - old_off[i] >= kVmMaxValue) return fail(c, MMP_EINVAL, "%s: value %d has 2^30 bytes or more", fn, i);
    }
    if (n > 0 && ((old_off[n] > old_off[0] && !old_buf) || (str_off[3 * n] > str_off[0] && !strs))) return fail(c, MMP_EINVAL, "%s: bad argument", fn);
    if (n == 0) {
        out_off[0] = 0;
        *n_bytes_out = 0;
        return MMP_OK;
    }
    if ((int64_t)str_off[3 * n] - str_off[0] + default_owner_len > INT32_MAX) return fail(c, MMP_EINVAL, "%s: 2^31 string bytes or more", fn);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    // the requests and their strings; the default owner rides behind them as span 3n
    const int32_t s0 = str_off[0], sbytes = str_off[3 * n] - s0;
    std::vector<char> blob((size_t)sbytes + default_owner_len);
    if (sbytes) memcpy(blob.data(), strs + s0, (size_t)sbytes);
    if (default_owner_len) memcpy(blob.data() + sbytes, default_owner, (size_t)default_owner_len);
    std::vector<int32_t> soff((size_t)3 * n + 2), srel;
    for (int32_t k = 0; k <= 3 * n; k++) soff[k] = str_off[k] - s0;
    soff[(size_t)3 * n + 1] = sbytes + default_owner_len;
    if (const int rc = stage_strings(c, fn, "string ", blob.data(), soff.data(), 3 * n + 1, c->vw_strs, c->vw_soff, srel)) return rc;
    HIP_TRY(c, c->vw_reqs.ensure((size_t)n * sizeof(mmp_vmodel_write_req)));
    HIP_TRY(c, hipMemcpyAsync(c->vw_reqs.p, reqs, (size_t)n * sizeof(mmp_vmodel_write_req), hipMemcpyHostToDevice, st));
    HIP_TRY(c, c->vw_rows.ensure((size_t)n * sizeof(mmp_vmodel_write_row)));
    VmWriteArgs A{};
    A.reqs = c->vw_reqs.as<mmp_vmodel_write_req>();
    A.strs = c->vw_strs.as<char>();
    A.str_off = c->vw_soff.as<int32_t>();
    A.M = vmodel_models(c);
    A.model_hmask = hash_mask(c->tune.model_id_hash_bits);
    A.now = now_ms;
    A.age = lastused_age_on_add_ms;
    A.rows = c->vw_rows.as<mmp_vmodel_write_row>();
    return render_stored_values(c, fn, old_buf, old_off, n, A, VModelValueParser(), vmodels_write_kernel<false>, vmodels_write_kernel<true>,
                                [] {}, {{rows_out, &c->vw_rows, (size_t)n * sizeof(mmp_vmodel_write_row)}}, out_buf, out_cap, out_off,
                                n_bytes_out);
} MMP_CATCH(c, "mmp_vmodels_write_json")

namespace {
// What the three read-only periodic tasks refuse about their keys, behind the committed check and before anything is written or
// staged (the order of mmp_registry_ops_k); called with batch_mu.  By row: nothing.
int tasks_keys_guard(mmp_ctx *c, const char *fn, bool keyed, const int32_t *key_off, int32_t n)
{
    if (!keyed) return MMP_OK;
    if (const int rc = model_id_space_guard(c, fn)) return rc;
    return check_offsets(c, fn, "key ", key_off, n);
}

// rateTrackingTask, the one body of mmp_scaleup_plan (conc == null), mmp_scaleup_plan_conc and mmp_scaleup_plan_k, for a caller
// who HOLDS batch_mu (it owns c->stream and the scratch for the whole call, and every writer of the state the call reads —
// commit, the loaders, registry events, a retirement — takes it too: the published snapshot, the registry and the model-id table
// cannot change underneath).  keys / key_off both NULL: by row.  By key the entries' `model` is written on the device, one launch
// in front of the plan (tasks_keyed_kernel), and the caller's is never read.
int scaleup_locked(mmp_ctx *c, const char *fn, const mmp_cache_entry *entries, const char *keys, const int32_t *key_off,
                   const mmp_conc_entry *conc, int32_t n, const mmp_scaleup_params *p, const mmp_conc_params *cp, mmp_scaleup_out *outs,
                   mmp_conc_out *conc_outs, uint8_t *overloaded_out, int32_t *skipped, mmp_conc_result *result, int32_t *model_idx_out)
{
    const bool latency = cp != nullptr, keyed = keys || key_off;
    if (!c->committed) return fail(c, MMP_ESTATE, "no committed snapshot");
    const int32_t P = c->snap.P;
    if (P > 0 && !overloaded_out) return fail(c, MMP_EINVAL, "%s: overloaded_out is null", fn);
    if (const int rc = tasks_keys_guard(c, fn, keyed, key_off, n)) return rc;
    if (P > 0) memset(overloaded_out, 0, (size_t)P);
    for (int32_t i = 0; i < n; i++) {
        outs[i] = mmp_scaleup_out{};
        outs[i].new_i1 = entries[i].earlier_use_iteration;
        outs[i].new_i2 = entries[i].last_used_iteration;
        if (latency) {
            conc_outs[i] = mmp_conc_out{};
            conc_outs[i].new_prior_sum = conc[i].prior_sum;
            conc_outs[i].new_prior_count = conc[i].prior_count;
        }
    }
    if (latency) {  // (a run that returns early leaves the task's field as it was)
        *result = mmp_conc_result{};
        result->average_model_parallelism = cp->average_model_parallelism;
    }
    // the three early returns of the task, MM.java:5646-5648, :5658-5660, :5667-5669
    const int64_t time_delta = (int64_t)((uint64_t)p->now - (uint64_t)p->last_check_time);
    *skipped = (time_delta * 5 < p->rate_check_interval_ms * 3 || c->stats.instance_count < 2 || n == 0) ? 1 : 0;
    hipStream_t st = c->stream;
    std::vector<int32_t> krel;  // (what the staged offsets are uploaded from: lives until the synchronisation below)
    if (*skipped) {  // the task returned before it looked at an entry: the rows of the keys are all there is to answer
        if (keyed && n > 0 && model_idx_out) {  // the same launch as below, with no plan behind it (one resolution path)
            HIP_TRY(c, hipSetDevice(c->cfg.device));
            if (const int rc = tasks_keys_stage(c, fn, keys, key_off, n, krel)) return rc;
            HIP_TRY(c, c->s_reqs.ensure((size_t)n * sizeof(mmp_cache_entry)));
            HIP_TRY(c, hipMemcpyAsync(c->s_reqs.p, entries, (size_t)n * sizeof(mmp_cache_entry), hipMemcpyHostToDevice, st));
            KT_BEGIN(c, st);
            tasks_keys_launch(c, n, c->s_reqs.as<mmp_cache_entry>(), TasksNoClaim{});
            KT_END(c, st);
            HIP_TRY(c, hipGetLastError());
            const int rc = tasks_model_idx(c, true, entries, n, model_idx_out);
            kt_collect(c);
            return rc;
        }
        return tasks_model_idx(c, keyed, entries, n, model_idx_out);  // (by row: the caller's own rows; nothing else to answer)
    }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    if (keyed)
        if (const int rc = tasks_keys_stage(c, fn, keys, key_off, n, krel)) return rc;
    HIP_TRY(c, c->s_reqs.ensure((size_t)n * sizeof(mmp_cache_entry)));
    HIP_TRY(c, c->s_outs.ensure((size_t)n * sizeof(mmp_scaleup_out)));
    HIP_TRY(c, c->s_a.ensure((size_t)std::max(P, 1)));
    HIP_TRY(c, c->s_b.ensure(2 * sizeof(int32_t)));  // [0] overloaded instances, [1] latency-based: getExcludeSet's maxRpm
    HIP_TRY(c, hipMemcpyAsync(c->s_reqs.p, entries, (size_t)n * sizeof(mmp_cache_entry), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemsetAsync(c->s_b.p, 0, 2 * sizeof(int32_t), st));
    if (latency) {
        HIP_TRY(c, c->s_c.ensure((size_t)n * sizeof(mmp_conc_entry)));
        HIP_TRY(c, c->s_d.ensure((size_t)n * sizeof(mmp_conc_out) + sizeof(mmp_conc_result)));
        HIP_TRY(c, hipMemcpyAsync(c->s_c.p, conc, (size_t)n * sizeof(mmp_conc_entry), hipMemcpyHostToDevice, st));
    }
    mmp_conc_result *d_res = latency ? reinterpret_cast<mmp_conc_result *>(static_cast<char *>(c->s_d.p) + (size_t)n * sizeof(mmp_conc_out)) : nullptr;
    const int32_t a = (int32_t)((uint32_t)p->scale_up_rpm_threshold * 4u);
    const int32_t b = (int32_t)((uint32_t)p->our_rpm - 2u * (uint32_t)p->scale_up_rpm_threshold);
    const mmp_pod_row *pods = c->sb[c->cur].pods.as<mmp_pod_row>();
    KT_BEGIN(c, st);
    if (keyed) tasks_keys_launch(c, n, c->s_reqs.as<mmp_cache_entry>(), TasksNoClaim{});
    if (latency)  // getExcludeSet's threshold comes from the task's averageModelParallelism (:5836)
        hipLaunchKernelGGL(conc_exclude_rpms_kernel, dim3(1), dim3(64), 0, st, cp->average_model_parallelism, p->our_rpm,
                           c->s_b.as<int32_t>() + 1, d_res);
    if (P > 0)
        hipLaunchKernelGGL(overloaded_pods_kernel, dim3(div_up(P, 256)), dim3(256), 0, st, pods, P, p->self_pod,
                           a > b ? a : b, latency ? c->s_b.as<int32_t>() + 1 : nullptr, c->s_a.as<uint8_t>(), c->s_b.as<int32_t>());
    ScaleupArgs A;
    A.entries = c->s_reqs.as<mmp_cache_entry>();
    A.models = c->models.as<mmp_model_row>();
    A.ent_pod = c->ent_pod.as<int32_t>();
    A.ent_time = c->ent_time.as<int64_t>();
    A.stats = cur_side(c).stats_acc.as<StatsAcc>();
    A.tstats = cur_side(c).tstats.as<StatsAcc>();
    A.T_rows = std::max(c->n_types, 1);
    A.has_tc = c->n_types > 0 ? 1 : 0;
    A.overloaded = c->s_a.as<uint8_t>();
    A.excluded_count = c->s_b.as<int32_t>();
    A.outs = c->s_outs.as<mmp_scaleup_out>();
    A.p = *p;
    A.n = n;
    A.n_models = c->n_models;
    A.P = P;
    A.conc = latency ? c->s_c.as<mmp_conc_entry>() : nullptr;
    A.conc_outs = latency ? c->s_d.as<mmp_conc_out>() : nullptr;
    A.conc_res = d_res;
    A.dyn_const = latency ? cp->dynamic_rpm_scale_constant : 0;
    hipLaunchKernelGGL(scaleup_plan_kernel, dim3(div_up(n, 256)), dim3(256), 0, st, A);
    if (latency) hipLaunchKernelGGL(conc_average_kernel, dim3(1), dim3(64), 0, st, n, d_res);
    KT_END(c, st);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(outs, c->s_outs.p, (size_t)n * sizeof(mmp_scaleup_out), hipMemcpyDeviceToHost, st));
    if (P > 0) HIP_TRY(c, hipMemcpyAsync(overloaded_out, c->s_a.p, (size_t)P, hipMemcpyDeviceToHost, st));
    if (latency) {
        HIP_TRY(c, hipMemcpyAsync(conc_outs, c->s_d.p, (size_t)n * sizeof(mmp_conc_out), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(result, d_res, sizeof(mmp_conc_result), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(c, hipStreamSynchronize(st));
    kt_collect(c);
    return tasks_model_idx(c, keyed, entries, n, model_idx_out);
}

// the argument check and the hold of batch_mu around scaleup_locked.  The state lock c->mu is NOT held: latency-path calls
// (mmp_place_batch / _gate / _evict on the slots) keep flowing.
int scaleup_plan_impl(mmp_ctx *c, const char *fn, const mmp_cache_entry *entries, const char *keys, const int32_t *key_off,
                      const mmp_conc_entry *conc, int32_t n, const mmp_scaleup_params *p, const mmp_conc_params *cp, mmp_scaleup_out *outs,
                      mmp_conc_out *conc_outs, uint8_t *overloaded_out, int32_t *skipped, mmp_conc_result *result, int32_t *model_idx_out)
{
    const bool latency = cp != nullptr;
    if (!c || !p || !skipped || n < 0 || (n > 0 && (!entries || !outs)) || (latency && (!result || (n > 0 && (!conc || !conc_outs)))) ||
        (keys == nullptr) != (key_off == nullptr))
        return fail(c, MMP_EINVAL, "%s: bad argument", fn);
    std::lock_guard<std::mutex> gb(c->batch_mu);
    return scaleup_locked(c, fn, entries, keys, key_off, conc, n, p, cp, outs, conc_outs, overloaded_out, skipped, result, model_idx_out);
}
}  // namespace

int mmp_scaleup_plan(mmp_ctx *c, const mmp_cache_entry *entries, int32_t n, const mmp_scaleup_params *p,
                     mmp_scaleup_out *outs, uint8_t *overloaded_out, int32_t *skipped)
try {
    return scaleup_plan_impl(c, "mmp_scaleup_plan", entries, nullptr, nullptr, nullptr, n, p, nullptr, outs, nullptr, overloaded_out, skipped,
                             nullptr, nullptr);
} MMP_CATCH(c, "mmp_scaleup_plan")

// by model id (or by row with keys == key_off == NULL); conc_params NULL: limitModelConcurrency == false
int mmp_scaleup_plan_k(mmp_ctx *c, const mmp_cache_entry *entries, const mmp_conc_entry *conc, int32_t n, const char *keys,
                       const int32_t *key_off, const mmp_scaleup_params *p, const mmp_conc_params *cp, mmp_scaleup_out *outs,
                       mmp_conc_out *conc_outs, uint8_t *overloaded_out, int32_t *skipped, mmp_conc_result *result, int32_t *model_idx_out)
try {
    if (!cp && (conc || conc_outs || result))
        return fail(c, MMP_EINVAL, "mmp_scaleup_plan_k: conc, conc_outs and result come with conc_params or not at all");
    return scaleup_plan_impl(c, "mmp_scaleup_plan_k", entries, keys, key_off, conc, n, p, cp, outs, conc_outs, overloaded_out, skipped, result,
                             model_idx_out);
} MMP_CATCH(c, "mmp_scaleup_plan_k")

int mmp_scaleup_plan_conc(mmp_ctx *c, const mmp_cache_entry *entries, const mmp_conc_entry *conc, int32_t n,
                          const mmp_scaleup_params *p, const mmp_conc_params *cp, mmp_scaleup_out *outs, mmp_conc_out *conc_outs,
                          uint8_t *overloaded_out, int32_t *skipped, mmp_conc_result *result)
try {
    if (!cp) return fail(c, MMP_EINVAL, "mmp_scaleup_plan_conc: conc_params is null");
    return scaleup_plan_impl(c, "mmp_scaleup_plan_conc", entries, nullptr, nullptr, conc, n, p, cp, outs, conc_outs, overloaded_out, skipped,
                             result, nullptr);
} MMP_CATCH(c, "mmp_scaleup_plan_conc")

namespace {
// the janitor's scale-down ON THE DEVICE: the decision and the budget walk over n candidates that stand in device memory
// (d_conc: their MaxConcCacheEntry rows beside them, or nullptr), into c->s_a (decide) and c->s_b (removed), which the caller has
// sized.  Only enqueues, inside the caller's bracket; called with batch_mu, so that a caller who owns the lock can chain it behind
// its own work — mmp_janitor_plan_k does, behind the apply.  The registry pointers are read HERE: an apply may have moved them.
int scaledown_enqueue(mmp_ctx *c, hipStream_t st, const mmp_cache_entry *d_entries, const mmp_conc_entry *d_conc, int32_t n,
                      const mmp_scaledown_params *p, int64_t dyn_const)
{
    ScaledownArgs A;
    A.entries = d_entries;
    A.models = c->models.as<mmp_model_row>();
    A.ent_pod = c->ent_pod.as<int32_t>();
    A.ent_time = c->ent_time.as<int64_t>();
    A.pods = c->sb[c->cur].pods.as<mmp_pod_row>();
    A.pos_of = c->snap.pos_of;
    // instanceSetStats(): with type constraints, the stats of the partition this instance belongs to
    // (EMPTY_STATS when it is not in the table), cluster-wide otherwise
    {
        const int32_t sp = p->self_pod;
        const int32_t k = (sp >= 0 && sp < (int32_t)cur_side(c).pts_of.size()) ? cur_side(c).pts_of[sp] : -1;
        A.stats = c->n_types > 0 ? cur_side(c).pstats.as<StatsAcc>() + (k >= 0 ? k : cur_side(c).n_pts) : cur_side(c).stats_acc.as<StatsAcc>();
    }
    A.decide = c->s_a.as<uint8_t>();
    A.removed = c->s_b.as<uint8_t>();
    A.p = *p;
    A.n = n;
    A.n_models = c->n_models;
    A.P = c->snap.P;
    A.conc = d_conc;
    A.dyn_const = dyn_const;
    hipLaunchKernelGGL(scaledown_decide_kernel, dim3(div_up(n, 256)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(scaledown_budget_kernel, dim3(1), dim3(64), 0, st, A);
    return MMP_OK;
}

// the one body of mmp_scaledown_plan (conc == null), mmp_scaledown_plan_conc and mmp_scaledown_plan_k, for a caller who HOLDS
// batch_mu (the ownership scaleup_locked states): the candidates staged, their keys resolved when there are any, then
// scaledown_enqueue.  keys / key_off both NULL: by row.
int scaledown_locked(mmp_ctx *c, const char *fn, const mmp_cache_entry *entries, const char *keys, const int32_t *key_off,
                     const mmp_conc_entry *conc, int32_t n, const mmp_scaledown_params *p, int64_t dyn_const, uint8_t *removed_out,
                     int32_t *model_idx_out)
{
    const bool keyed = keys || key_off;
    if (!c->committed) return fail(c, MMP_ESTATE, "no committed snapshot");
    if (const int rc = tasks_keys_guard(c, fn, keyed, key_off, n)) return rc;
    if (n == 0) return MMP_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    std::vector<int32_t> krel;  // (what the staged offsets are uploaded from: lives until the synchronisation below)
    if (keyed)
        if (const int rc = tasks_keys_stage(c, fn, keys, key_off, n, krel)) return rc;
    HIP_TRY(c, c->s_reqs.ensure((size_t)n * sizeof(mmp_cache_entry)));
    HIP_TRY(c, c->s_a.ensure((size_t)n));
    HIP_TRY(c, c->s_b.ensure((size_t)n));
    HIP_TRY(c, hipMemcpyAsync(c->s_reqs.p, entries, (size_t)n * sizeof(mmp_cache_entry), hipMemcpyHostToDevice, st));
    if (conc) {
        HIP_TRY(c, c->s_c.ensure((size_t)n * sizeof(mmp_conc_entry)));
        HIP_TRY(c, hipMemcpyAsync(c->s_c.p, conc, (size_t)n * sizeof(mmp_conc_entry), hipMemcpyHostToDevice, st));
    }
    KT_BEGIN(c, st);
    if (keyed) tasks_keys_launch(c, n, c->s_reqs.as<mmp_cache_entry>(), TasksNoClaim{});
    if (const int rc = scaledown_enqueue(c, st, c->s_reqs.as<mmp_cache_entry>(), conc ? c->s_c.as<mmp_conc_entry>() : nullptr, n, p, dyn_const))
        return rc;
    KT_END(c, st);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(removed_out, c->s_b.p, (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    kt_collect(c);
    return tasks_model_idx(c, keyed, entries, n, model_idx_out);
}

// the argument check and the hold of batch_mu around scaledown_locked.  The state lock c->mu is NOT held: latency-path calls
// (mmp_place_batch / _gate / _evict on the slots) keep flowing.
int scaledown_plan_impl(mmp_ctx *c, const char *fn, const mmp_cache_entry *entries, const char *keys, const int32_t *key_off,
                        const mmp_conc_entry *conc, int32_t n, const mmp_scaledown_params *p, int64_t dyn_const, uint8_t *removed_out,
                        int32_t *model_idx_out)
{
    if (!c || !p || n < 0 || (n > 0 && (!entries || !removed_out)) || (keys == nullptr) != (key_off == nullptr))
        return fail(c, MMP_EINVAL, "%s: bad argument", fn);
    std::lock_guard<std::mutex> gb(c->batch_mu);
    return scaledown_locked(c, fn, entries, keys, key_off, conc, n, p, dyn_const, removed_out, model_idx_out);
}

// preShutdown's migration, the one body of mmp_migration_plan and mmp_migration_plan_k (the ownership scaleup_locked states)
int migration_plan_impl(mmp_ctx *c, const char *fn, const mmp_cache_entry *entries, int32_t n, const char *keys, const int32_t *key_off,
                        int32_t self_pod, int64_t now, int64_t cutoff_age_ms, uint8_t *action_out, uint8_t *wait_out, int32_t *model_idx_out)
{
    const bool keyed = keys || key_off;
    if (!c || n < 0 || (n > 0 && (!entries || !action_out || !wait_out)) || (keys == nullptr) != (key_off == nullptr))
        return fail(c, MMP_EINVAL, "%s: bad argument", fn);
    std::lock_guard<std::mutex> gb(c->batch_mu);
    if (!c->committed) return fail(c, MMP_ESTATE, "no committed snapshot");
    if (const int rc = tasks_keys_guard(c, fn, keyed, key_off, n)) return rc;
    if (n == 0) return MMP_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    std::vector<int32_t> krel;  // (what the staged offsets are uploaded from: lives until the synchronisation below)
    if (keyed)
        if (const int rc = tasks_keys_stage(c, fn, keys, key_off, n, krel)) return rc;
    HIP_TRY(c, c->s_reqs.ensure((size_t)n * sizeof(mmp_cache_entry)));
    HIP_TRY(c, c->s_a.ensure((size_t)n));
    HIP_TRY(c, c->s_b.ensure((size_t)n));
    HIP_TRY(c, hipMemcpyAsync(c->s_reqs.p, entries, (size_t)n * sizeof(mmp_cache_entry), hipMemcpyHostToDevice, st));
    KT_BEGIN(c, st);
    if (keyed) tasks_keys_launch(c, n, c->s_reqs.as<mmp_cache_entry>(), TasksNoClaim{});
    hipLaunchKernelGGL(migration_plan_kernel, dim3(div_up(n, 256)), dim3(256), 0, st, c->s_reqs.as<mmp_cache_entry>(), n,
                       c->models.as<mmp_model_row>(), c->n_models, c->ent_pod.as<int32_t>(), self_pod,
                       (int64_t)((uint64_t)now - (uint64_t)cutoff_age_ms), c->s_a.as<uint8_t>(), c->s_b.as<uint8_t>());
    KT_END(c, st);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(action_out, c->s_a.p, (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(wait_out, c->s_b.p, (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    kt_collect(c);
    return tasks_model_idx(c, keyed, entries, n, model_idx_out);
}
}  // namespace

int mmp_scaledown_plan(mmp_ctx *c, const mmp_cache_entry *entries, int32_t n, const mmp_scaledown_params *p,
                       uint8_t *removed_out)
try {
    return scaledown_plan_impl(c, "mmp_scaledown_plan", entries, nullptr, nullptr, nullptr, n, p, 0, removed_out, nullptr);
} MMP_CATCH(c, "mmp_scaledown_plan")

int mmp_scaledown_plan_conc(mmp_ctx *c, const mmp_cache_entry *entries, const mmp_conc_entry *conc, int32_t n,
                            const mmp_scaledown_params *p, int64_t dynamic_rpm_scale_constant, uint8_t *removed_out)
try {
    if (n > 0 && !conc) return fail(c, MMP_EINVAL, "mmp_scaledown_plan_conc: conc is null");
    return scaledown_plan_impl(c, "mmp_scaledown_plan_conc", entries, nullptr, nullptr, conc, n, p, dynamic_rpm_scale_constant, removed_out, nullptr);
} MMP_CATCH(c, "mmp_scaledown_plan_conc")

// by model id (or by row with keys == key_off == NULL); conc NULL: not latency-based
int mmp_scaledown_plan_k(mmp_ctx *c, const mmp_cache_entry *entries, const mmp_conc_entry *conc, int32_t n, const char *keys,
                         const int32_t *key_off, const mmp_scaledown_params *p, int64_t dynamic_rpm_scale_constant, uint8_t *removed_out,
                         int32_t *model_idx_out)
try {
    return scaledown_plan_impl(c, "mmp_scaledown_plan_k", entries, keys, key_off, conc, n, p, conc ? dynamic_rpm_scale_constant : 0, removed_out,
                               model_idx_out);
} MMP_CATCH(c, "mmp_scaledown_plan_k")

int mmp_migration_plan(mmp_ctx *c, const mmp_cache_entry *entries, int32_t n, int32_t self_pod, int64_t now,
                       int64_t cutoff_age_ms, uint8_t *action_out, uint8_t *wait_out)
try {
    return migration_plan_impl(c, "mmp_migration_plan", entries, n, nullptr, nullptr, self_pod, now, cutoff_age_ms, action_out, wait_out, nullptr);
} MMP_CATCH(c, "mmp_migration_plan")

int mmp_migration_plan_k(mmp_ctx *c, const mmp_cache_entry *entries, int32_t n, const char *keys, const int32_t *key_off, int32_t self_pod,
                         int64_t now, int64_t cutoff_age_ms, uint8_t *action_out, uint8_t *wait_out, int32_t *model_idx_out)
try {
    return migration_plan_impl(c, "mmp_migration_plan_k", entries, n, keys, key_off, self_pod, now, cutoff_age_ms, action_out, wait_out,
                               model_idx_out);
} MMP_CATCH(c, "mmp_migration_plan_k")

// the janitor by model id (or by row with keys == key_off == NULL), with its scale-down in the same call (scaledown != NULL)
int mmp_janitor_plan_k(mmp_ctx *c, const mmp_janitor_entry *entries, int32_t n, const char *keys, const int32_t *key_off,
                       const mmp_janitor_params *p, uint32_t flags, const mmp_scaledown_params *scaledown, const mmp_conc_entry *conc,
                       int64_t dynamic_rpm_scale_constant, int32_t *model_idx_out, uint8_t *actions_out, mmp_janitor_edit *edits_out,
                       int32_t max_edits, mmp_cache_entry *cands_out, int32_t *cand_rows_out, int32_t max_cands, uint8_t *removed_out,
                       mmp_janitor_info *info)
try {
    if (janitor_args_bad(c, entries, n, p, flags, actions_out, edits_out, max_edits, cands_out, cand_rows_out, max_cands, info) ||
        (keys == nullptr) != (key_off == nullptr) || (!scaledown && conc) || (scaledown && max_cands > 0 && !removed_out))
        return fail(c, MMP_EINVAL, "mmp_janitor_plan_k: bad argument");
    // the scale-down reads the registry as the two loops LEFT it: only an applied run has such a registry
    if (scaledown && !(flags & MMP_JANITOR_APPLY)) return fail(c, MMP_EINVAL, "mmp_janitor_plan_k: the scale-down needs MMP_JANITOR_APPLY");
    return janitor_drive(c, "mmp_janitor_plan_k", entries, n, keys, key_off, p, flags,
                         JanitorChain{scaledown, scaledown ? conc : nullptr, conc ? dynamic_rpm_scale_constant : 0, removed_out}, model_idx_out,
                         actions_out, edits_out, max_edits, cands_out, cand_rows_out, max_cands, info);
} MMP_CATCH(c, "mmp_janitor_plan_k")

/* ---- stateful keyed caches (a12 + a13) ------------------------------------- */

namespace {
// what both loads refuse of the segments; E = seg_off[n_caches]
int caches_keyed_segs_bad(mmp_ctx *c, const char *fn, int32_t n_caches, const int32_t *seg_off, const int64_t *capacity)
{
    if (!c || n_caches < 0 || !seg_off || (n_caches > 0 && !capacity)) return fail(c, MMP_EINVAL, "%s: bad argument", fn);
    if (seg_off[0] != 0) return fail(c, MMP_EINVAL, "%s: seg_off[0] must be 0", fn);
    for (int32_t i = 0; i < n_caches; i++)
        if (seg_off[i + 1] < seg_off[i]) return fail(c, MMP_EINVAL, "%s: seg_off not monotone at %d", fn, i);
    return MMP_OK;
}

// The load itself, shared by mmp_caches_load_keyed and mmp_caches_load_keyed_k (bound: the keys are registry rows the device
// resolved).  The caller holds batch_mu and the state lock, has set the device and has refused what it refuses.
int caches_keyed_store(mmp_ctx *c, int32_t n_caches, const int32_t *seg_off, const int64_t *last_used, const int32_t *weight,
                       const int32_t *key, const int64_t *capacity, const mmp_ubm_state *ubm, bool bound)
{
    const int32_t E = seg_off[n_caches];
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    mmp_ctx::KeyedStore &K = c->ks[c->ks_cur];
    HIP_TRY(c, K.off.ensure((size_t)(n_caches + 1) * 4));
    HIP_TRY(c, K.lu.ensure((size_t)std::max(E, 1) * 8));
    HIP_TRY(c, K.wt.ensure((size_t)std::max(E, 1) * 4));
    HIP_TRY(c, K.key.ensure((size_t)std::max(E, 1) * 4));
    HIP_TRY(c, K.n.ensure((size_t)std::max(n_caches, 1) * 4));
    HIP_TRY(c, c->k_cap.ensure((size_t)std::max(n_caches, 1) * 8));
    HIP_TRY(c, c->k_wsize.ensure((size_t)std::max(n_caches, 1) * 8));
    HIP_TRY(c, c->k_oldest.ensure((size_t)std::max(n_caches, 1) * 8));
    HIP_TRY(c, c->k_ubm.ensure((size_t)std::max(n_caches, 1) * sizeof(mmp_ubm_state)));
    c->k_n.assign(n_caches, 0);
    std::vector<int64_t> ws(std::max(n_caches, 1), 0), old(std::max(n_caches, 1), -1);
    std::vector<mmp_ubm_state> us(std::max(n_caches, 1));
    for (int32_t i = 0; i < n_caches; i++) {
        c->k_n[i] = seg_off[i + 1] - seg_off[i];
        if (c->k_n[i] > 0) old[i] = last_used[seg_off[i]];  // oldestTime as the last write left it (clhm :1129-1133)
        for (int32_t e = seg_off[i]; e < seg_off[i + 1]; e++) ws[i] += weight[e] < 0 ? -(int64_t)weight[e] : weight[e];
        if (ubm)
            us[i] = ubm[i];
        else {
            us[i] = mmp_ubm_state{};
            us[i].reserved = -1;
        }
    }
    HIP_TRY(c, copy_sync(c, K.off.p, seg_off, (size_t)(n_caches + 1) * 4, hipMemcpyHostToDevice));
    if (E) {
        HIP_TRY(c, copy_sync(c, K.lu.p, last_used, (size_t)E * 8, hipMemcpyHostToDevice));
        HIP_TRY(c, copy_sync(c, K.wt.p, weight, (size_t)E * 4, hipMemcpyHostToDevice));
        HIP_TRY(c, copy_sync(c, K.key.p, key, (size_t)E * 4, hipMemcpyHostToDevice));
    }
    if (n_caches) {
        HIP_TRY(c, copy_sync(c, K.n.p, c->k_n.data(), (size_t)n_caches * 4, hipMemcpyHostToDevice));
        HIP_TRY(c, copy_sync(c, c->k_cap.p, capacity, (size_t)n_caches * 8, hipMemcpyHostToDevice));
        HIP_TRY(c, copy_sync(c, c->k_wsize.p, ws.data(), (size_t)n_caches * 8, hipMemcpyHostToDevice));
        HIP_TRY(c, copy_sync(c, c->k_oldest.p, old.data(), (size_t)n_caches * 8, hipMemcpyHostToDevice));
        HIP_TRY(c, copy_sync(c, c->k_ubm.p, us.data(), (size_t)n_caches * sizeof(mmp_ubm_state), hipMemcpyHostToDevice));
    }
    c->k_caches = n_caches;
    c->k_slots = E;
    c->k_bound = bound;
    c->evid_bytes.clear();  // the eviction record of a keyed replay ends with the store it was made on
    c->evid_off.assign(1, 0);
    c->evid_lu.clear();
    c->evid_timed = false;
    return MMP_OK;
}

// THE ID GATHER, shared by the eviction record and mmp_cache_read_k (cache_keyed_kernels.hpp), in two steps around the one
// read-back of the sizes.  ckey_gather_sizes, inside the caller's bracket: the id lengths of the n row words at d_rows and their
// exclusive scan, n + 1 offsets into c->k_goff.  ckey_gather_bytes, once the caller has the total on the host: the bytes into
// c->k_gbytes and on into `out`, in a bracket of its own.  The caller owns batch_mu and has seen the id space guard pass.
int ckey_gather_sizes(mmp_ctx *c, const int32_t *d_rows, int32_t n)
{
    hipStream_t st = c->stream;
    size_t scan_bytes = 0;
    HIP_TRY(c, rocprim::exclusive_scan(nullptr, scan_bytes, c->k_len.as<int32_t>(), c->k_goff.as<int32_t>(), 0, (size_t)n + 1, rocprim::plus<int32_t>(), st));
    HIP_TRY(c, c->j_scan_tmp.ensure(std::max<size_t>(scan_bytes, 16)));
    hipLaunchKernelGGL(ckey_len_kernel, dim3(div_up(n + 1, kIdTabBlock)), dim3(kIdTabBlock), 0, st, d_rows, n, c->mid_n, c->mid_off.as<int32_t>(),
                       c->k_len.as<int32_t>());
    HIP_TRY(c, rocprim::exclusive_scan(c->j_scan_tmp.p, scan_bytes, c->k_len.as<int32_t>(), c->k_goff.as<int32_t>(), 0, (size_t)n + 1,
                                       rocprim::plus<int32_t>(), st));
    return MMP_OK;
}
int ckey_gather_room(mmp_ctx *c, int32_t n)
{
    HIP_TRY(c, c->k_len.ensure(((size_t)n + 1) * 4));
    HIP_TRY(c, c->k_goff.ensure(((size_t)n + 1) * 4));
    return MMP_OK;
}
int ckey_gather_bytes(mmp_ctx *c, const int32_t *d_rows, int32_t n, int32_t total, char *out)
{
    if (total <= 0) return MMP_OK;
    hipStream_t st = c->stream;
    HIP_TRY(c, c->k_gbytes.ensure((size_t)total));
    const double earlier = c->last_kernel_ms;
    KT_BEGIN(c, st);
    hipLaunchKernelGGL(ckey_gather_kernel, dim3(div_up(n, kIdTabBlock / kGatherTeam)), dim3(kIdTabBlock), 0, st, d_rows, n, c->mid_n,
                       c->mid_off.as<int32_t>(), c->mid_bytes.as<char>(), c->k_goff.as<int32_t>(), c->k_gbytes.as<char>());
    KT_END(c, st);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, copy_sync(c, out, c->k_gbytes.p, (size_t)total, hipMemcpyDeviceToHost));
    kt_collect(c);
    kt_add(c, earlier);
    return MMP_OK;
}

// the caches are bound and the id table covers the registry (what every _k cache call answers MMP_ESTATE to)
int caches_bound_guard(mmp_ctx *c, const char *fn)
{
    if (const int rc = model_id_space_guard(c, fn)) return rc;
    if (!c->k_bound) return fail(c, MMP_ESTATE, "%s: the caches are not bound to model ids (mmp_caches_load_keyed_k)", fn);
    return MMP_OK;
}

// what mmp_cache_replay_k adds to the replay
struct ReplayKeyed {
    const char *keys;
    const int32_t *key_off;
    int32_t *status_out, *row_out;
    char *id_bytes_out;
    int32_t max_id_bytes;
    int32_t *id_off_out, *n_id_bytes_out;
    bool times;           // mmp_cache_replay_kt: the TIMES instantiations, the record carries the victims' lastUsed
    int64_t *ev_lu_out;   // (may be NULL: the times stay in the context)
};
}  // namespace

int mmp_caches_load_keyed(mmp_ctx *c, int32_t n_caches, const int32_t *seg_off, const int64_t *last_used,
                          const int32_t *weight, const int32_t *key, const int64_t *capacity, const mmp_ubm_state *ubm)
try {
    if (const int rc = caches_keyed_segs_bad(c, "mmp_caches_load_keyed", n_caches, seg_off, capacity)) return rc;
    const int32_t E = seg_off[n_caches];
    if (E > 0 && (!last_used || !weight || !key)) return fail(c, MMP_EINVAL, "mmp_caches_load_keyed: null entry arrays");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    return caches_keyed_store(c, n_caches, seg_off, last_used, weight, key, capacity, ubm, false);
} MMP_CATCH(c, "mmp_caches_load_keyed")

int mmp_caches_load_keyed_k(mmp_ctx *c, int32_t n_caches, const int32_t *seg_off, const int64_t *last_used, const int32_t *weight,
                            const char *keys, const int32_t *key_off, const uint8_t *is_unloadbuf, const int64_t *capacity,
                            const mmp_ubm_state *ubm, int32_t *key_row_out)
try {
    const char *fn = "mmp_caches_load_keyed_k";
    if (const int rc = caches_keyed_segs_bad(c, fn, n_caches, seg_off, capacity)) return rc;
    const int32_t E = seg_off[n_caches];
    if ((keys == nullptr) != (key_off == nullptr) || (E > 0 && (!last_used || !weight || !key_off)))
        return fail(c, MMP_EINVAL, "%s: null entry arrays", fn);
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    if (const int rc = model_id_space_guard(c, fn)) return rc;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    std::vector<int32_t> rows((size_t)std::max(E, 1), 0), krel;
    if (E > 0) {
        if (const int rc = stage_strings(c, fn, "key ", keys, key_off, E, c->ida_bytes, c->ida_off, krel)) return rc;
        HIP_TRY(c, c->k_krow.ensure((size_t)E * 4));
        HIP_TRY(c, c->k_len.ensure(4));
        if (is_unloadbuf) {
            HIP_TRY(c, c->k_kstat.ensure((size_t)E));
            HIP_TRY(c, hipMemcpyAsync(c->k_kstat.p, is_unloadbuf, (size_t)E, hipMemcpyHostToDevice, st));
        }
        int32_t *d_word = c->k_len.as<int32_t>();
        HIP_TRY(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_word), INT32_MAX, 1, st));
        const CkeyEntriesArgs A{c->ida_bytes.as<char>(), c->ida_off.as<int32_t>(), E, hash_mask(c->tune.model_id_hash_bits), vmodel_models(c),
                                is_unloadbuf ? c->k_kstat.as<uint8_t>() : nullptr, c->k_krow.as<int32_t>(), d_word};
        KT_BEGIN(c, st);
        hipLaunchKernelGGL(ckey_entries_kernel, dim3(div_up(E, kIdTabBlock)), dim3(kIdTabBlock), 0, st, A);
        KT_END(c, st);
        HIP_TRY(c, hipGetLastError());
        int32_t lowest = INT32_MAX;
        HIP_TRY(c, hipMemcpyAsync(&lowest, d_word, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, copy_sync(c, rows.data(), c->k_krow.p, (size_t)E * 4, hipMemcpyDeviceToHost));
        kt_collect(c);
        if (lowest != INT32_MAX) return fail(c, MMP_EINVAL, "%s: entry %d names an id the table does not know; nothing was loaded", fn, lowest);
    }
    const double resolve_ms = c->last_kernel_ms;
    if (const int rc = caches_keyed_store(c, n_caches, seg_off, last_used, weight, rows.data(), capacity, ubm, true)) return rc;
    if (c->prof) c->last_kernel_ms = E > 0 ? resolve_ms : -1;
    if (key_row_out && E > 0) memcpy(key_row_out, rows.data(), (size_t)E * 4);
    return MMP_OK;
} MMP_CATCH(c, "mmp_caches_load_keyed_k")

namespace {
// THE REPLAY, by key (mmp_cache_replay: kx == nullptr) or by model id.  The caller holds batch_mu and the state lock and has
// refused NULL buffers.  Nothing of the store changes before the last step that refuses.
int cache_replay_drive(mmp_ctx *c, const char *fn, const mmp_cache_op *ops, int32_t n_ops, int64_t now, mmp_cache_op_out *outs,
                       int32_t *evicted_keys, int32_t max_evicted, int32_t *n_evicted_slots, const ReplayKeyed *kx)
{
    const int32_t NC = c->k_caches;
    if (NC <= 0 && n_ops > 0) return fail(c, MMP_ESTATE, "no keyed caches loaded");
    *n_evicted_slots = 0;
    if (n_ops == 0) {
        if (kx) {  // a valid call: its record is the empty one
            c->evid_bytes.clear();
            c->evid_off.assign(1, 0);
            c->evid_lu.clear();
            c->evid_timed = kx->times;
            *kx->n_id_bytes_out = 0;
            if (kx->id_off_out) kx->id_off_out[0] = 0;
            if (c->prof) c->last_kernel_ms = -1;
        }
        return MMP_OK;
    }
    // group the operations by cache (stable) and size the new layout: every insert may add a slot
    std::vector<int32_t> cnt(NC + 1, 0), ins(NC, 0);
    for (int32_t i = 0; i < n_ops; i++) {
        const mmp_cache_op &o = ops[i];
        if (o.cache < 0 || o.cache >= NC) return fail(c, MMP_EINVAL, "%s: op %d names cache %d", fn, i, o.cache);
        if (o.op < 0 || o.op > MMP_COP_UBM_INSERT_FAILED_PLACEHOLDER) return fail(c, MMP_EINVAL, "%s: op %d has code %d", fn, i, o.op);
        if (kx && (o.reserved < 0 || o.reserved > MMP_COPK_RAW_KEY || (o.reserved == MMP_COPK_RAW_KEY && o.key != MMP_UNLOADBUF_KEY)))
            return fail(c, MMP_EINVAL, "%s: op %d has reserved %d with key %d", fn, i, o.reserved, o.key);
        cnt[o.cache + 1]++;
        if (o.op == MMP_COP_PUT_IF_ABSENT || o.op == MMP_COP_UBM_INSERT_NEW_ENTRY || o.op == MMP_COP_UBM_INSERT_FAILED_PLACEHOLDER)
            ins[o.cache]++;
    }
    std::vector<int32_t> op_off(NC + 1, 0), new_off(NC + 1, 0), ev_off(NC + 1, 0);
    // team width per cache by the deque slots its replay needs: [0] 8 lanes, [1] 16 lanes, [2] the whole wavefront
    int32_t tile = 1, tiles[3] = {1, 1, 1};
    std::vector<int32_t> ids[3];
    for (int32_t k = 0; k < NC; k++) {
        op_off[k + 1] = op_off[k] + cnt[k + 1];
        const int32_t slots = c->k_n[k] + ins[k];
        new_off[k + 1] = new_off[k] + slots;
        ev_off[k + 1] = ev_off[k] + (cnt[k + 1] ? slots : 0);  // a cache cannot evict more than it ever held
        const int w = slots + 1 <= kTeam8Slots ? 0 : slots + 1 <= kTeam16Slots ? 1 : 2;
        ids[w].push_back(k);
        if (cnt[k + 1]) {
            tile = std::max(tile, slots + 1);
            tiles[w] = std::max(tiles[w], slots + 1);
        }
    }
    if (tile > kCacheTile) return fail(c, MMP_EINVAL, "%s: a cache needs %d deque slots, the tile holds %d", fn, tile, kCacheTile);
    if (ev_off[NC] > max_evicted) return fail(c, MMP_EINVAL, "%s: evicted_keys needs room for %d keys", fn, ev_off[NC]);
    if (kx)
        if (const int rc = check_offsets(c, fn, "key ", kx->key_off, n_ops)) return rc;
    std::vector<int32_t> order(n_ops), fill(op_off.begin(), op_off.end() - 1);
    for (int32_t i = 0; i < n_ops; i++) order[fill[ops[i].cache]++] = i;
    std::vector<mmp_cache_op> grouped((size_t)n_ops);  // the kernel reads an operation with ONE load (no index in between)
    for (int32_t q = 0; q < n_ops; q++) grouped[q] = ops[order[q]];

    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    const int32_t n_slots = ev_off[NC];
    std::vector<int32_t> inv, krel;  // (what the uploads below are from: they live to the end)
    if (kx) {
        // the keys go up as the caller gave them, in one copy; the resolver scatters through the inverse of `order`
        inv.resize((size_t)n_ops);
        for (int32_t q = 0; q < n_ops; q++) inv[order[q]] = q;
        if (const int rc = stage_strings(c, fn, "key ", kx->keys, kx->key_off, n_ops, c->ida_bytes, c->ida_off, krel)) return rc;
        HIP_TRY(c, c->k_inv.ensure((size_t)n_ops * 4));
        HIP_TRY(c, c->k_kstat.ensure((size_t)n_ops * 4));
        HIP_TRY(c, c->k_krow.ensure((size_t)n_ops * 4));
        if (const int rc = ckey_gather_room(c, n_slots)) return rc;
        HIP_TRY(c, hipMemcpyAsync(c->k_inv.p, inv.data(), (size_t)n_ops * 4, hipMemcpyHostToDevice, st));
    }
    mmp_ctx::KeyedStore &S = c->ks[c->ks_cur], &D = c->ks[1 - c->ks_cur];
    const int32_t Enew = new_off[NC];
    HIP_TRY(c, D.off.ensure((size_t)(NC + 1) * 4));
    HIP_TRY(c, D.lu.ensure((size_t)std::max(Enew, 1) * 8));
    HIP_TRY(c, D.wt.ensure((size_t)std::max(Enew, 1) * 4));
    HIP_TRY(c, D.key.ensure((size_t)std::max(Enew, 1) * 4));
    HIP_TRY(c, D.n.ensure((size_t)NC * 4));
    HIP_TRY(c, c->k_ops.ensure((size_t)n_ops * sizeof(mmp_cache_op)));
    HIP_TRY(c, c->k_order.ensure((size_t)n_ops * 4));
    HIP_TRY(c, c->k_opoff.ensure((size_t)(NC + 1) * 4));
    HIP_TRY(c, c->k_outs.ensure((size_t)n_ops * sizeof(mmp_cache_op_out)));
    HIP_TRY(c, c->k_ev.ensure((size_t)std::max(ev_off[NC], 1) * 4));
    HIP_TRY(c, c->k_evoff.ensure((size_t)(NC + 1) * 4));
    const bool times = kx && kx->times;
    if (times) HIP_TRY(c, c->k_evlu.ensure((size_t)std::max(ev_off[NC], 1) * 8));
    HIP_TRY(c, hipMemcpyAsync(D.off.p, new_off.data(), (size_t)(NC + 1) * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->k_ops.p, grouped.data(), (size_t)n_ops * sizeof(mmp_cache_op), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->k_order.p, order.data(), (size_t)n_ops * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->k_opoff.p, op_off.data(), (size_t)(NC + 1) * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->k_evoff.p, ev_off.data(), (size_t)(NC + 1) * 4, hipMemcpyHostToDevice, st));
    ReplayArgs A;
    A.src = CacheStore{S.off.as<int32_t>(), S.lu.as<int64_t>(), S.wt.as<int32_t>(), S.key.as<int32_t>(), S.n.as<int32_t>()};
    A.dst = CacheStore{D.off.as<int32_t>(), D.lu.as<int64_t>(), D.wt.as<int32_t>(), D.key.as<int32_t>(), D.n.as<int32_t>()};
    A.capacity = c->k_cap.as<int64_t>();
    A.weighted_size = c->k_wsize.as<int64_t>();
    A.oldest = c->k_oldest.as<int64_t>();
    A.ubm = c->k_ubm.as<mmp_ubm_state>();
    A.ops = c->k_ops.as<mmp_cache_op>();
    A.op_order = c->k_order.as<int32_t>();
    A.op_off = c->k_opoff.as<int32_t>();
    A.outs = c->k_outs.as<mmp_cache_op_out>();
    A.evicted = c->k_ev.as<int32_t>();
    A.evicted_lu = times ? c->k_evlu.as<int64_t>() : nullptr;
    A.ev_off = c->k_evoff.as<int32_t>();
    A.n_caches = NC;
    A.tile = tile;
    A.now = now;
    HIP_TRY(c, c->k_ids.ensure((size_t)NC * 4));
    {
        std::vector<int32_t> all;
        all.reserve(NC);
        for (auto &v : ids) all.insert(all.end(), v.begin(), v.end());
        HIP_TRY(c, hipMemcpyAsync(c->k_ids.p, all.data(), (size_t)NC * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipStreamSynchronize(st));  // `all` leaves scope (the other uploads above are from vectors that live to the end)
    }
    if (kx && n_slots)  // a slot no op used holds -1
        HIP_TRY(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c->k_ev.as<int32_t>()), -1, (size_t)n_slots, st));
    if (times && n_slots)  // and its time is 0
        HIP_TRY(c, hipMemsetAsync(c->k_evlu.p, 0, (size_t)n_slots * 8, st));
    KT_BEGIN(c, st);
    if (kx) {
        // (the staged copy keeps keyed_resolve_kernel's contract: the buffer is an allocation of its own with 16 bytes behind the keys)
        const CkeyOpsArgs K{c->ida_bytes.as<char>(), c->ida_off.as<int32_t>(), n_ops, hash_mask(c->tune.model_id_hash_bits), vmodel_models(c),
                            c->k_inv.as<int32_t>(), c->k_ops.as<mmp_cache_op>(), c->k_kstat.as<int32_t>(), c->k_krow.as<int32_t>()};
        hipLaunchKernelGGL(ckey_ops_kernel, dim3(div_up(n_ops, kIdTabBlock)), dim3(kIdTabBlock), 0, st, K);
    }
    const int32_t *d_ids = c->k_ids.as<int32_t>();
    for (int w = 0; w < 3; w++)
        if ((int32_t)ids[w].size() == NC) d_ids = nullptr;  // one width for every cache: the list is the identity
    // bytes of LDS per deque slot: lu 8, weight 4, key 4, the pending LIFO 4 + 4 — and 8 for its lastUsed column with TIMES, where
    // the full tile of a wavefront (2 048 slots) takes 65 536 bytes: the most a launch gets without a function attribute
    const size_t slot_lds = times ? 32 : 24;
    static_assert(kCacheTile * 32 <= 65536 && kTeam8Slots * 32 * 8 <= 65536 && kTeam16Slots * 32 * 4 <= 65536, "replay tile exceeds the LDS of a launch");
    const auto launch = [&](auto k8, auto k16, auto k64) {
        if (!ids[0].empty()) {
            A.tile = tiles[0];
            hipLaunchKernelGGL(k8, dim3(div_up((int)ids[0].size(), 8)), dim3(64), (size_t)tiles[0] * slot_lds * 8, st, A, d_ids,
                               (int32_t)ids[0].size());
        }
        if (!ids[1].empty()) {
            A.tile = tiles[1];
            hipLaunchKernelGGL(k16, dim3(div_up((int)ids[1].size(), 4)), dim3(64), (size_t)tiles[1] * slot_lds * 4, st, A,
                               d_ids ? d_ids + ids[0].size() : nullptr, (int32_t)ids[1].size());
        }
        if (!ids[2].empty()) {
            A.tile = tiles[2];
            hipLaunchKernelGGL(k64, dim3((int)ids[2].size()), dim3(64), (size_t)tiles[2] * slot_lds, st, A,
                               d_ids ? d_ids + ids[0].size() + ids[1].size() : nullptr, (int32_t)ids[2].size());
        }
    };
    if (times)
        launch(cache_replay_kernel<8, true>, cache_replay_kernel<16, true>, cache_replay_kernel<64, true>);
    else
        launch(cache_replay_kernel<8, false>, cache_replay_kernel<16, false>, cache_replay_kernel<64, false>);
    if (kx && n_slots)  // the lengths of the victims' ids and their scan, in the same span
        if (const int rc = ckey_gather_sizes(c, c->k_ev.as<int32_t>(), n_slots)) return rc;
    KT_END(c, st);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(outs, c->k_outs.p, (size_t)n_ops * sizeof(mmp_cache_op_out), hipMemcpyDeviceToHost, st));
    if (ev_off[NC]) HIP_TRY(c, hipMemcpyAsync(evicted_keys, c->k_ev.p, (size_t)ev_off[NC] * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(c->k_n.data(), D.n.p, (size_t)NC * 4, hipMemcpyDeviceToHost, st));
    std::vector<int32_t> id_off((size_t)n_slots + 1, 0);
    if (kx) {
        if (kx->status_out) HIP_TRY(c, hipMemcpyAsync(kx->status_out, c->k_kstat.p, (size_t)n_ops * 4, hipMemcpyDeviceToHost, st));
        if (kx->row_out) HIP_TRY(c, hipMemcpyAsync(kx->row_out, c->k_krow.p, (size_t)n_ops * 4, hipMemcpyDeviceToHost, st));
        if (n_slots) HIP_TRY(c, hipMemcpyAsync(id_off.data(), c->k_goff.p, ((size_t)n_slots + 1) * 4, hipMemcpyDeviceToHost, st));
    }
    std::vector<int64_t> ev_lu(times ? (size_t)n_slots : 0);
    if (times && n_slots) HIP_TRY(c, hipMemcpyAsync(ev_lu.data(), c->k_evlu.p, (size_t)n_slots * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    kt_collect(c);
    // the replay is applied from here on, whatever becomes of the record: it is stateful and cannot be asked twice
    c->ks_cur = 1 - c->ks_cur;
    c->k_slots = Enew;
    *n_evicted_slots = ev_off[NC];
    if (!kx) return MMP_OK;
    // the eviction record: the context keeps the bytes (a retirement between this call and mmp_cache_evicted_ids cannot change
    // them), the caller gets them when they fit
    const int32_t need = id_off[n_slots];
    c->evid_off.assign(1, 0);
    c->evid_lu.clear();
    c->evid_timed = false;
    c->evid_bytes.assign((size_t)need, 0);
    if (const int rc = ckey_gather_bytes(c, c->k_ev.as<int32_t>(), n_slots, need, c->evid_bytes.data())) {
        c->evid_bytes.clear();
        return rc;
    }
    c->evid_off = id_off;
    if (times) {
        if (kx->ev_lu_out && n_slots) memcpy(kx->ev_lu_out, ev_lu.data(), (size_t)n_slots * 8);
        c->evid_lu = std::move(ev_lu);
        c->evid_timed = true;
    }
    *kx->n_id_bytes_out = need;
    if (kx->id_off_out) memcpy(kx->id_off_out, id_off.data(), ((size_t)n_slots + 1) * 4);
    if (need > 0 && kx->max_id_bytes >= need) memcpy(kx->id_bytes_out, c->evid_bytes.data(), (size_t)need);
    return MMP_OK;
}
}  // namespace

int mmp_cache_replay(mmp_ctx *c, const mmp_cache_op *ops, int32_t n_ops, int64_t now, mmp_cache_op_out *outs,
                     int32_t *evicted_keys, int32_t max_evicted, int32_t *n_evicted_slots)
try {
    if (!c || n_ops < 0 || max_evicted < 0 || (n_ops > 0 && (!ops || !outs)) || (max_evicted > 0 && !evicted_keys) ||
        !n_evicted_slots)
        return fail(c, MMP_EINVAL, "mmp_cache_replay: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    return cache_replay_drive(c, "mmp_cache_replay", ops, n_ops, now, outs, evicted_keys, max_evicted, n_evicted_slots, nullptr);
} MMP_CATCH(c, "mmp_cache_replay")

int mmp_cache_replay_k(mmp_ctx *c, const mmp_cache_op *ops, int32_t n_ops, const char *keys, const int32_t *key_off, int64_t now,
                       int32_t *key_status_out, int32_t *key_row_out, mmp_cache_op_out *outs, int32_t *evicted_rows, int32_t max_evicted,
                       int32_t *n_evicted_slots, char *ev_id_bytes_out, int32_t max_id_bytes, int32_t *ev_id_off_out, int32_t *n_id_bytes_out)
try {
    if (!c || n_ops < 0 || max_evicted < 0 || (n_ops > 0 && (!ops || !outs)) || (max_evicted > 0 && !evicted_rows) || !n_evicted_slots ||
        !n_id_bytes_out || max_id_bytes < 0 || (max_id_bytes > 0 && !ev_id_bytes_out) || (keys == nullptr) != (key_off == nullptr) ||
        (n_ops > 0 && !key_off))
        return fail(c, MMP_EINVAL, "mmp_cache_replay_k: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    if (const int rc = caches_bound_guard(c, "mmp_cache_replay_k")) return rc;
    const ReplayKeyed kx{keys, key_off, key_status_out, key_row_out, ev_id_bytes_out, max_id_bytes, ev_id_off_out, n_id_bytes_out, false, nullptr};
    return cache_replay_drive(c, "mmp_cache_replay_k", ops, n_ops, now, outs, evicted_rows, max_evicted, n_evicted_slots, &kx);
} MMP_CATCH(c, "mmp_cache_replay_k")

int mmp_cache_replay_kt(mmp_ctx *c, const mmp_cache_op *ops, int32_t n_ops, const char *keys, const int32_t *key_off, int64_t now,
                        int32_t *key_status_out, int32_t *key_row_out, mmp_cache_op_out *outs, int32_t *evicted_rows, int32_t max_evicted,
                        int32_t *n_evicted_slots, char *ev_id_bytes_out, int32_t max_id_bytes, int32_t *ev_id_off_out, int32_t *n_id_bytes_out,
                        int64_t *ev_last_used_out)
try {
    if (!c || n_ops < 0 || max_evicted < 0 || (n_ops > 0 && (!ops || !outs)) || (max_evicted > 0 && !evicted_rows) || !n_evicted_slots ||
        !n_id_bytes_out || max_id_bytes < 0 || (max_id_bytes > 0 && !ev_id_bytes_out) || (keys == nullptr) != (key_off == nullptr) ||
        (n_ops > 0 && !key_off))
        return fail(c, MMP_EINVAL, "mmp_cache_replay_kt: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    if (const int rc = caches_bound_guard(c, "mmp_cache_replay_kt")) return rc;
    const ReplayKeyed kx{keys, key_off, key_status_out, key_row_out, ev_id_bytes_out, max_id_bytes, ev_id_off_out, n_id_bytes_out, true,
                         ev_last_used_out};
    return cache_replay_drive(c, "mmp_cache_replay_kt", ops, n_ops, now, outs, evicted_rows, max_evicted, n_evicted_slots, &kx);
} MMP_CATCH(c, "mmp_cache_replay_kt")

int mmp_cache_evicted_times(mmp_ctx *c, int64_t *out, int32_t max_slots, int32_t *n_slots_out)
try {
    if (!c || !n_slots_out || max_slots < 0 || (max_slots > 0 && !out)) return fail(c, MMP_EINVAL, "mmp_cache_evicted_times: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    if (const int rc = caches_bound_guard(c, "mmp_cache_evicted_times")) return rc;
    if (!c->evid_timed)
        return fail(c, MMP_ESTATE, "mmp_cache_evicted_times: the last replay recorded no times (mmp_cache_replay_kt records them)");
    const int32_t ns = (int32_t)c->evid_lu.size();
    *n_slots_out = ns;
    if (ns > 0 && max_slots >= ns) memcpy(out, c->evid_lu.data(), (size_t)ns * 8);
    if (c->prof) c->last_kernel_ms = -1;  // no kernel: the record is words the context holds
    return MMP_OK;
} MMP_CATCH(c, "mmp_cache_evicted_times")

int mmp_cache_evicted_ids(mmp_ctx *c, char *bytes_out, int32_t max_bytes, int32_t *off_out, int32_t *n_slots_out, int32_t *n_bytes_out)
try {
    if (!c || !n_slots_out || !n_bytes_out || max_bytes < 0 || (max_bytes > 0 && !bytes_out))
        return fail(c, MMP_EINVAL, "mmp_cache_evicted_ids: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    if (const int rc = caches_bound_guard(c, "mmp_cache_evicted_ids")) return rc;
    const int32_t ns = (int32_t)c->evid_off.size() - 1, nb = c->evid_off[ns];
    *n_slots_out = ns;
    *n_bytes_out = nb;
    if (off_out) memcpy(off_out, c->evid_off.data(), ((size_t)ns + 1) * 4);
    if (nb > 0 && max_bytes >= nb) memcpy(bytes_out, c->evid_bytes.data(), (size_t)nb);
    if (c->prof) c->last_kernel_ms = -1;  // no kernel: the record is bytes the context holds
    return MMP_OK;
} MMP_CATCH(c, "mmp_cache_evicted_ids")

int mmp_cache_read_k(mmp_ctx *c, int32_t cache, int32_t max_entries, int64_t *last_used, int32_t *weight, int32_t *row_out,
                     char *id_bytes_out, int32_t max_id_bytes, int32_t *id_off_out, int32_t *n_out, int32_t *n_id_bytes_out,
                     int64_t *capacity, int64_t *weighted_size, mmp_ubm_state *ubm)
try {
    if (!c || !n_out || !n_id_bytes_out || max_entries < 0 || max_id_bytes < 0 || (max_id_bytes > 0 && !id_bytes_out))
        return fail(c, MMP_EINVAL, "mmp_cache_read_k: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    if (const int rc = caches_bound_guard(c, "mmp_cache_read_k")) return rc;
    if (cache < 0 || cache >= c->k_caches) return fail(c, MMP_EINVAL, "mmp_cache_read_k: cache %d out of range", cache);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    HIP_TRY(c, hipStreamSynchronize(st));
    mmp_ctx::KeyedStore &K = c->ks[c->ks_cur];
    int32_t off = 0;
    HIP_TRY(c, copy_sync(c, &off, K.off.as<int32_t>() + cache, 4, hipMemcpyDeviceToHost));
    const int32_t n = c->k_n[cache];
    *n_out = n;
    const int32_t m = std::min(n, max_entries);
    std::vector<int32_t> id_off((size_t)m + 1, 0);
    const int32_t *d_rows = K.key.as<int32_t>() + off;
    if (c->prof) c->last_kernel_ms = -1;
    if (m > 0) {
        if (const int rc = ckey_gather_room(c, m)) return rc;
        KT_BEGIN(c, st);
        if (const int rc = ckey_gather_sizes(c, d_rows, m)) return rc;
        KT_END(c, st);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, copy_sync(c, id_off.data(), c->k_goff.p, ((size_t)m + 1) * 4, hipMemcpyDeviceToHost));
        kt_collect(c);
        if (last_used) HIP_TRY(c, copy_sync(c, last_used, K.lu.as<int64_t>() + off, (size_t)m * 8, hipMemcpyDeviceToHost));
        if (weight) HIP_TRY(c, copy_sync(c, weight, K.wt.as<int32_t>() + off, (size_t)m * 4, hipMemcpyDeviceToHost));
        if (row_out) HIP_TRY(c, copy_sync(c, row_out, d_rows, (size_t)m * 4, hipMemcpyDeviceToHost));
    }
    const int32_t need = id_off[m];
    *n_id_bytes_out = need;
    if (id_off_out) memcpy(id_off_out, id_off.data(), ((size_t)m + 1) * 4);
    if (need > 0 && max_id_bytes >= need)
        if (const int rc = ckey_gather_bytes(c, d_rows, m, need, id_bytes_out)) return rc;
    if (capacity) HIP_TRY(c, copy_sync(c, capacity, c->k_cap.as<int64_t>() + cache, 8, hipMemcpyDeviceToHost));
    if (weighted_size) HIP_TRY(c, copy_sync(c, weighted_size, c->k_wsize.as<int64_t>() + cache, 8, hipMemcpyDeviceToHost));
    if (ubm) HIP_TRY(c, copy_sync(c, ubm, c->k_ubm.as<mmp_ubm_state>() + cache, sizeof(mmp_ubm_state), hipMemcpyDeviceToHost));
    return MMP_OK;
} MMP_CATCH(c, "mmp_cache_read_k")

int mmp_cache_read(mmp_ctx *c, int32_t cache, int32_t max_entries, int64_t *last_used, int32_t *weight, int32_t *key,
                   int32_t *n_out, int64_t *capacity, int64_t *weighted_size, mmp_ubm_state *ubm)
try {
    if (!c || !n_out || max_entries < 0) return fail(c, MMP_EINVAL, "mmp_cache_read: bad argument");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    if (cache < 0 || cache >= c->k_caches) return fail(c, MMP_EINVAL, "mmp_cache_read: cache %d out of range", cache);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    mmp_ctx::KeyedStore &K = c->ks[c->ks_cur];
    int32_t off = 0;
    HIP_TRY(c, copy_sync(c, &off, K.off.as<int32_t>() + cache, 4, hipMemcpyDeviceToHost));
    const int32_t n = c->k_n[cache];
    *n_out = n;
    const int32_t m = std::min(n, max_entries);
    if (m > 0) {
        if (last_used) HIP_TRY(c, copy_sync(c, last_used, K.lu.as<int64_t>() + off, (size_t)m * 8, hipMemcpyDeviceToHost));
        if (weight) HIP_TRY(c, copy_sync(c, weight, K.wt.as<int32_t>() + off, (size_t)m * 4, hipMemcpyDeviceToHost));
        if (key) HIP_TRY(c, copy_sync(c, key, K.key.as<int32_t>() + off, (size_t)m * 4, hipMemcpyDeviceToHost));
    }
    if (capacity) HIP_TRY(c, copy_sync(c, capacity, c->k_cap.as<int64_t>() + cache, 8, hipMemcpyDeviceToHost));
    if (weighted_size) HIP_TRY(c, copy_sync(c, weighted_size, c->k_wsize.as<int64_t>() + cache, 8, hipMemcpyDeviceToHost));
    if (ubm) HIP_TRY(c, copy_sync(c, ubm, c->k_ubm.as<mmp_ubm_state>() + cache, sizeof(mmp_ubm_state), hipMemcpyDeviceToHost));
    return MMP_OK;
} MMP_CATCH(c, "mmp_cache_read")

int mmp_caches_load(mmp_ctx *c, int32_t n_caches, const int32_t *seg_off, const int64_t *last_used,
                    const int32_t *weight, const int64_t *capacity)
try {
    if (!c || n_caches < 0 || !seg_off || (n_caches > 0 && !capacity)) return fail(c, MMP_EINVAL, "mmp_caches_load: bad argument");
    if (seg_off[0] != 0) return fail(c, MMP_EINVAL, "mmp_caches_load: seg_off[0] must be 0");
    for (int32_t i = 0; i < n_caches; i++)
        if (seg_off[i + 1] < seg_off[i]) return fail(c, MMP_EINVAL, "mmp_caches_load: seg_off not monotone at %d", i);
    const int32_t E = seg_off[n_caches];
    if (E > 0 && (!last_used || !weight)) return fail(c, MMP_EINVAL, "mmp_caches_load: null entry arrays");
    std::lock_guard<std::mutex> gb(c->batch_mu);
    std::lock_guard<std::shared_mutex> g(c->mu);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, quiesce_decisions(c));  // small eviction batches read these tables from the latency slots' streams
    HIP_TRY(c, c->c_seg.ensure((size_t)(n_caches + 1) * 4));
    HIP_TRY(c, c->c_lu.ensure((size_t)std::max(E, 1) * 8));
    HIP_TRY(c, c->c_wt.ensure((size_t)std::max(E, 1) * 4));
    HIP_TRY(c, c->c_cap.ensure((size_t)std::max(n_caches, 1) * 8));
    HIP_TRY(c, copy_sync(c, c->c_seg.p, seg_off, (size_t)(n_caches + 1) * 4, hipMemcpyHostToDevice));
    if (E) {
        HIP_TRY(c, copy_sync(c, c->c_lu.p, last_used, (size_t)E * 8, hipMemcpyHostToDevice));
        HIP_TRY(c, copy_sync(c, c->c_wt.p, weight, (size_t)E * 4, hipMemcpyHostToDevice));
    }
    if (n_caches) HIP_TRY(c, copy_sync(c, c->c_cap.p, capacity, (size_t)n_caches * 8, hipMemcpyHostToDevice));
    c->n_caches = n_caches;
    c->cache_entries = E;
    return MMP_OK;
} MMP_CATCH(c, "mmp_caches_load")

}  // extern "C"
