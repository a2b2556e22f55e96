/*
 * mmplace.h — C ABI of libmmplace: the MI355X (gfx950) placement / eviction
 * solver that replaces the bodies of ModelMesh's instance-selection hot path.
 *
 * Every entry point is `extern "C"`, takes plain pointers and sizes, never
 * throws and never aborts the process.  Return value: 0 (MMP_OK) or a negative
 * MMP_E* code; text via mmp_last_error().  There is NO CPU fallback: if no HIP
 * device is usable mmp_create() fails with MMP_ENODEVICE.
 *
 * Each function cites the reference interface it replaces.  "MM.java" =
 * src/main/java/com/ibm/watson/modelmesh/ModelMesh.java of kserve/modelmesh.
 * The JNI / Java binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Pod and model indices are dense ints chosen by the caller (the Java side
 * interns instance ids; `id_order` carries String.compareTo order).
 */
#ifndef MMPLACE_H
#define MMPLACE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMP_ABI_VERSION 3 /* 3: latency-based rebalancers (mmp_*_plan_conc), the single-caller request form, bounded device-pointer calls */

/* return codes */
#define MMP_OK 0
#define MMP_EINVAL (-1)     /* bad argument                                    */
#define MMP_ENODEVICE (-2)  /* no usable HIP device (never falls back to CPU)  */
#define MMP_EHIP (-3)       /* a HIP runtime call failed                       */
#define MMP_EORDER (-4)     /* PLACEMENT_ORDER is not a total order on rows    */
#define MMP_ESTATE (-5)     /* call sequence error (e.g. place before commit)  */
#define MMP_ENOMEM (-6)

/* `chosen` conventions — LoadBalancer.getNext return values:
 *   null                         -> MMP_NONE   (MM.java:4796,4803,4872,4942)
 *   LoadBalancer.ABORT_REQUEST   -> MMP_SELF   (MM.java:4384,4894,4932,4990)
 *   a ServiceInstanceInfo        -> its pod index */
#define MMP_NONE (-1)
#define MMP_SELF (-2)

typedef struct mmp_ctx mmp_ctx;

/* Solver parameters that are inputs, not constants. */
typedef struct {
    int32_t device;           /* HIP device ordinal                             */
    int32_t reserved0;
    int64_t min_space_units;  /* MM.java:765-771 (see mmp_min_space_units)      */
    int64_t min_churn_age_ms; /* MM.java:697                                    */
} mmp_config;

/* One InstanceRecord (InstanceRecord.java:37-69) — 64 bytes.
 * flags: bit0 shuttingDown (row is treated as deleted, MM.java:1462-1464),
 *        bit1 live = present in the litelinks instance map (MM.java:4765),
 *        bit2 tombstone (slot unused; keeps indices stable across removals). */
#define MMP_POD_SHUTTING_DOWN 1u
#define MMP_POD_LIVE 2u
#define MMP_POD_TOMBSTONE 4u
typedef struct {
    int64_t lru_time; /* Long.MAX_VALUE when empty */
    int64_t capacity; /* 8 KiB units, ModelLoader.java:37 */
    int64_t used;
    int64_t version;  /* instanceVersion */
    int32_t count;
    int32_t loading_threads;
    int32_t loading_in_progress;
    int32_t rpm;
    uint32_t id_order;   /* dense rank of the id under String.compareTo  */
    int32_t replica_set; /* interned id.substring(0,6); -1 if |id| < 7   */
    uint32_t flags;
    uint32_t reserved;
} mmp_pod_row;

/* One ModelRecord (ModelRecord.java:61-114) — 24 bytes + 12 bytes per entry.
 * Entries [ent_off, ent_off+n_loaded) are instanceIds in TreeMap (id) order,
 * followed by n_failed loadFailedInstanceIds. */
typedef struct {
    int32_t type;     /* interned model type; ignored when no type table */
    int32_t ent_off;
    int32_t n_loaded;
    int32_t n_failed;
    int64_t last_used;
} mmp_model_row;

/* One CacheMissForwardingLB.getNext call (MM.java:4776) — 64 bytes.
 * flags bit0 = exclude.favourSelf (MM.java:4781).  The fresh_* fields are the
 * caller's getFreshInstanceRecord() (MM.java:5369-5386; its rpm is 0 there). */
#define MMP_REQ_FAVOUR_SELF 1u
typedef struct {
    int32_t model;      /* row in the model table                            */
    int32_t self_pod;   /* caller's pod index, -1 if not in the table        */
    uint32_t flags;
    uint32_t pick;      /* replaces ThreadLocalRandom: index=(pick*n)>>32    */
    int64_t last_used;  /* exclude.lastUsedTime (MM.java:4736,4951)          */
    int32_t extra_off;  /* tried-this-request ∪ explicit excludes (pool idx) */
    int32_t n_extra;
    int64_t fresh_lru;
    int64_t fresh_capacity;
    int64_t fresh_used;
    int32_t fresh_count;
    int32_t fresh_rpm;
} mmp_place_req;

/* The single-caller form of a batch of load-target decisions.  `self` and getFreshInstanceRecord() (MM.java:5369-5386) belong
 * to the CALLING INSTANCE, not to the request, and every batch the reference itself produces is issued by one instance: the rate
 * task (:5636), the janitor (:6110), the reaper (:6616), preShutdown (:6959), an instance's own request threads.  The caller's
 * side travels once per call (mmp_place_caller, 40 bytes), a decision is 24 bytes instead of 64: mmp_place_batch_c.  The
 * decision is the one of mmp_place_req {model, caller.self_pod, caller.flags, pick, last_used, extra_off, n_extra, caller.fresh_*}. */
typedef struct {
    int32_t self_pod; /* the calling instance, -1 if not in the table */
    uint32_t flags;   /* MMP_REQ_FAVOUR_SELF                          */
    int64_t fresh_lru;
    int64_t fresh_capacity;
    int64_t fresh_used;
    int32_t fresh_count;
    int32_t fresh_rpm;
} mmp_place_caller;
typedef struct {
    int32_t model;
    uint32_t pick;
    int64_t last_used;
    int32_t extra_off;
    int32_t n_extra;
} mmp_place_req_c;

/* mmp_place_out::best of a decision whose request the library refused to follow (bounded device-pointer calls: an exclusion
 * range outside the pool the caller declared); its chosen is MMP_NONE, n_candidates and hash are 0. */
#define MMP_BAD_REQUEST (-3)

/* 16 bytes per decision. On early returns (no eligible pod, or the immediate
 * "choose self" returns at MM.java:4872,4894,4932) n_candidates = hash = 0. */
typedef struct {
    int32_t chosen;       /* pod index | MMP_NONE | MMP_SELF                 */
    int32_t best;         /* final bestIid's pod index, -1 if none           */
    int32_t n_candidates; /* candidates.size() before the rpm filter         */
    uint32_t hash;        /* shortlist bitmap hash (audit)      */
} mmp_place_out;

/* One ForwardingLB.getNext call (MM.java:4315) — cache-hit routing, 48 bytes.
 * The reference reads litelinks' per-instance counters only for the instances that hold a copy of the model
 * (si.getInUseCount() / si.getLastUsedTime(), MM.java:4356,4360, inside the loop over filteredInstances): the
 * request brings exactly those — [cnt_off, cnt_off + n_cnt) of the call's mmp_serve_counter pool, one entry per
 * copy whose instance litelinks lists (siMap.get(iid) != null, :4343).  A copy WITHOUT an entry is a copy litelinks
 * does not list: it is skipped as at :4344-4347.  Nothing the size of the instance table crosses the boundary. */
#define MMP_SERVE_EXCLUDE_SELF 1u
#define MMP_SERVE_PREFER_SELF 2u
typedef struct {
    int32_t pod;       /* the instance (pod index)                         */
    int32_t in_use;    /* ServiceInstance.getInUseCount(), MM.java:4356    */
    int64_t last_used; /* ServiceInstance.getLastUsedTime(), MM.java:4360  */
} mmp_serve_counter;
typedef struct {
    int32_t model;
    int32_t self_pod;
    uint32_t flags;
    int32_t local_in_flight;     /* localInvokesInFlight (MM.java:4303)         */
    int64_t last_invoke_time;    /* lastInvokeTime (MM.java:4304)               */
    int64_t assume_completed_ms; /* TimeStats.assumeCompletedAfterMillis        */
    int32_t excl_off;            /* (pod,loadStart) pairs already tried + keyExcludes */
    int32_t n_excl;
    int32_t cnt_off;             /* this request's counters in the pool               */
    int32_t n_cnt;
} mmp_serve_req;

typedef struct {
    int32_t chosen; /* pod index | MMP_NONE | MMP_SELF */
    int32_t pad;
    int64_t chosen_load_start;
} mmp_serve_out;

/* ClusterStats (MM.java:1570-1591, InstanceSetStatsTracker.java:53-92). */
typedef struct {
    int64_t total_capacity;
    int64_t total_free;
    int64_t global_lru; /* Long.MAX_VALUE if none */
    int32_t instance_count;
    int32_t model_copy_count;
} mmp_stats;

/* One eviction evaluation on one pod's cache (clhm/ConcurrentLinkedHashMap.java
 * :329-352,590-652; clhm/LinkedDeque.java:243-288): insert an entry of `weight`
 * stamped `last_used` (0 = now) into the time-ordered deque, then evict from
 * the head while weightedSize > capacity. */
typedef struct {
    int32_t cache;      /* which per-pod cache segment                        */
    int32_t weight;     /* weight of the incoming entry (or weight delta)     */
    int64_t last_used;  /* 0 means now (clhm :1357-1360)                      */
} mmp_evict_req;

typedef struct {
    int32_t insert_pos;    /* deque position the new node is linked at         */
    int32_t n_victims;     /* nodes polled from the head                       */
    int32_t self_evicted;  /* 1 if the new node itself was among the victims   */
    int32_t pad;
    int64_t weighted_size; /* after eviction                                   */
    int64_t oldest_time;   /* oldestTime() after eviction, -1 if empty         */
} mmp_evict_out;

/* Stateful per-pod caches (rows a12 + a13): the clhm operations and the ModelCacheUnloadBufManager
 * methods, replayed in caller order per cache by mmp_cache_replay.  Keys are interned model ids;
 * MMP_UNLOADBUF_KEY is the manager's pinned "___UNLOADBUF" pseudo-entry
 * (ModelCacheUnloadBufManager.java:42,88), which a managed cache must contain when it is loaded.
 * The eviction listener belongs to the cache (MM.java:2863-2879): what MMP_COP_PUT_IF_ABSENT or MMP_COP_UPDATE_WEIGHT evicts
 * from a managed cache reaches entryRemoved like every other victim.  A read stamped <= 0 is a read "now" (clhm :383).
 * Domain: the weight `arg` of MMP_COP_PUT_IF_ABSENT, _UPDATE_WEIGHT, _UBM_INSERT_NEW_ENTRY and _UBM_INSERT_FAILED_PLACEHOLDER is
 * >= 1 (the weigher is CacheEntry.getWeight = Math.abs(weight), MM.java:1759: no caller can hand the cache a negative weight, and
 * a weight of 0 is a node that is never linked, clhm :604); a negative or zero `arg` there is outside the domain and its
 * outcome unspecified.  The manager's SUMS (weight + delta / + increase) may go negative or wrap: they are stored by magnitude
 * as the weigher answers them (Integer.MIN_VALUE stays as it is, as Math.abs leaves it).
 * MMP_COP_UBM_ADJUST_SPACE_REQUEST's `flag` (weakPrediction) is deliberately unused on the device: it negates CacheEntry.weight,
 * a field only the weigher reads, by magnitude — nothing the cache or the manager shows depends on it. */
#define MMP_UNLOADBUF_KEY (-1000000)
#define MMP_COP_PUT_IF_ABSENT 0           /* clhm putIfAbsent(key, w=arg, time)  :804-834; result 1 = inserted      */
#define MMP_COP_GET 1                     /* clhm get(key, time)                 :726-733; result = found           */
#define MMP_COP_UPDATE_WEIGHT 2           /* replace / replaceQuietly, new weight = arg, time -1 = quiet  :902-985   */
#define MMP_COP_REMOVE 3                  /* clhm remove(key)                    :861-870                           */
#define MMP_COP_UBM_INSERT_NEW_ENTRY 4    /* insertNewEntry(key, w=arg, time)    ModelCacheUnloadBufManager :130-145 */
#define MMP_COP_UBM_ADJUST_SPACE_REQUEST 5 /* adjustNewEntrySpaceRequest(increase=arg, key)              :152-166   */
#define MMP_COP_UBM_SPACE_IS_READY 6      /* cacheSpaceIsReady(required=arg)     :395-402 (read only)               */
#define MMP_COP_UBM_CLAIM_SPACE 7         /* claimRequestedSpaceIfReady(required=arg)                    :190-202   */
#define MMP_COP_UBM_ADJUST_AFTER_LOAD 8   /* adjustWeightAfterLoad(delta=arg, key)                       :224-246   */
#define MMP_COP_UBM_UNLOAD_COMPLETE 9     /* unloadComplete(weight=arg, success=flag)                    :318-338   */
#define MMP_COP_UBM_REMOVE_ENTRY 10       /* removeEntry(key) + entryRemoved; result = weight or -1      :281-316   */
#define MMP_COP_UBM_DISCARD_FAILED 11     /* discardFailedEntry(weight=arg)                              :343-349   */
#define MMP_COP_UBM_INSERT_FAILED_PLACEHOLDER 12 /* insertFailedPlaceholderEntry(key, w=arg, time)       :250-274   */
typedef struct {
    int32_t cache;
    int32_t op;
    int32_t key;
    int32_t arg;
    int64_t time; /* lastUsed: 0 = now (clhm :1357-1360) */
    int32_t flag;
    int32_t reserved;
} mmp_cache_op;

typedef struct {
    int32_t result;
    int32_t n_evicted;     /* entries this operation evicted (listener order)            */
    int32_t evicted_off;   /* their keys start here in the call's evicted_keys array      */
    int32_t buffer_weight; /* getUnloadBufferWeight() after the operation (0: unmanaged)  */
    int64_t weighted_size; /* runtimeCache.weightedSize() after the operation             */
    int64_t oldest_time;   /* runtimeCache.oldestTime(), -1 if empty                      */
} mmp_cache_op_out;

/* ModelCacheUnloadBufManager fields (:57-79); reserved < 0 = this cache has no manager. */
typedef struct {
    int32_t reserved;        /* unloadsReservedSizeUnits   */
    int32_t total_unloading; /* totalUnloadingWeight       */
    int64_t total_occupancy; /* totalModelCacheOccupancy   */
    int32_t cache_deficit;   /* cacheDeficit               */
    int32_t pad;
} mmp_ubm_state;

/* The request-level guards invokeModel evaluates around the two selections
 * (SURVEY.md §8 rows a10, a11, a14, a20), batched.  One struct carries the
 * scalar inputs of all of them; unused groups may be left zero. */
#define MMP_GATE_FAVOUR_SELF_FOR_HITS 1u /* favourSelfForHits, MM.java:3606             */
#define MMP_GATE_HAVE_CACHE_ENTRY 2u     /* getFromCache(...) != null, MM.java:3607-3612  */
#define MMP_GATE_ENTRY_DONE 4u           /* cacheEntry.isDone(), MM.java:3613             */
#define MMP_GATE_WE_CREATED_ENTRY 8u     /* weCreatedCacheEntry, MM.java:5186             */
#define MMP_GATE_ENTRY_FAILED 16u        /* ce.isFailed(), MM.java:2886                   */
#define MMP_GATE_HAVE_SIZE_HINT 32u      /* tas.known_size present, MM.java:5160          */
#define MMP_GATE_PUBLISH_FORCE 64u       /* publishInstanceRecord(force, ...), MM.java:5388 */
#define MMP_GATE_PRE_SHUTDOWN 128u
#define MMP_GATE_FRESH_SHUTTING_DOWN 256u
typedef struct {
    int32_t model;
    int32_t self_pod;
    uint32_t flags;
    int32_t excl_off, n_excl;         /* cache-hit (pod,loadStart) excludes filtering the copies */
    int32_t explicit_off, n_explicit; /* explicitExcludes / load-target filter members (pod idx)  */
    int32_t size_hint;                /* tas.known_size                                          */
    int64_t last_used_time;
    int64_t cache_capacity;           /* runtimeCache.capacity()                                 */
    int64_t cache_weighted_size;      /* runtimeCache.weightedSize()                             */
    int64_t cache_oldest_time;        /* runtimeCache.oldestTime(), -1 if empty                  */
    int32_t loader_predicted;         /* ce.loaderPredictedWeight()                              */
    int32_t loading_count;            /* loadingCount.get()                                      */
    int32_t weight_predict_cutoff;    /* loadingThreads + loadingThreads/3, MM.java:5013         */
    int32_t reserved;
    int64_t loaded_time;              /* registry load time of the evicted copy, <0 if absent    */
    int64_t load_timeout_ms;
    int64_t fresh_lru, fresh_capacity, fresh_used; /* getFreshInstanceRecord(), MM.java:5369; fresh_lru may be
                                                      runtimeCache.oldestTime() as it is: -1 (empty cache) is read as
                                                      Long.MAX_VALUE by the publish rule (:5423-5425)         */
    int32_t fresh_count, fresh_loading_threads, fresh_in_progress, fresh_rpm;
    int64_t last_published;           /* lastPublished, MM.java:5387                             */
} mmp_gate_req;

#define MMP_GATE_GO_LOCAL 1u            /* serve the hit locally, MM.java:3603-3626               */
#define MMP_GATE_FAILURES_BREACHED 2u   /* checkLoadFailureCount would throw, MM.java:4607-4627   */
#define MMP_GATE_LOCATIONS_BREACHED 4u  /* checkLoadLocationCount would throw, MM.java:4590-4604  */
#define MMP_GATE_LOCAL_NOT_ALLOWED 8u   /* throwIfLocalLoadNotAllowed would throw, MM.java:4003    */
#define MMP_GATE_CHURN_REJECT 16u       /* "Cache churn threshold exceeded", MM.java:3870-3884     */
#define MMP_GATE_EARLY_REJECT 32u       /* loadLocal aborts before inserting, MM.java:5185-5197    */
#define MMP_GATE_RELOAD_ELSEWHERE 64u   /* onEviction re-places the model, MM.java:2895,2919-2920  */
#define MMP_GATE_SHOULD_PUBLISH 128u    /* publishInstanceRecord writes an update, MM.java:5397-5468 */
typedef struct {
    uint32_t bits;
    int32_t initial_size; /* signed initialSize of loadLocal (negative = average-based), MM.java:5158-5179 */
} mmp_gate_out;

/* Leader "reaper" proactive-load plan. */
typedef struct {
    int32_t size_estimate; /* sizeEstimate, MM.java:6622-6629                           */
    int32_t free_count;    /* freeSpaceProactiveLoadCount, MM.java:6651                  */
    int32_t total_count;   /* totalProactiveLoadCount, MM.java:6655                      */
    int32_t n_candidates;  /* models passing the registry rule MM.java:6574-6577         */
    int32_t n_selected;    /* ensureLoadedInternal calls the Java would make             */
    int32_t error;         /* 1: sizeEstimate == 0 (the Java throws ArithmeticException) */
    int64_t space_to_fill; /* MM.java:6633-6650                                          */
    int64_t cutoff;        /* proactiveLastUsedCutoff, MM.java:6662-6664                 */
} mmp_proactive_info;

/* One local CacheEntry as the rebalancers see it (rows a15, a16, a21) — 56 bytes. */
#define MMP_CE_FAILED 1u /* ce == null || ce.isFailed() */
typedef struct {
    int32_t model;                 /* registry row, -1 if registry.get(modelId) == null */
    int32_t weight;                /* ce.getWeight()                                    */
    int64_t last_used;             /* cache last-used time                              */
    int64_t interval_count;        /* getAndResetIntervalCount() / getIntervalCount()   */
    int64_t last_heavy_time;       /* ce.getLastHeavyTime()                             */
    int64_t last_unload_time;      /* mr.getLastUnloadTime()                            */
    int32_t earlier_use_iteration; /* ce.earlierUseIteration                            */
    int32_t last_used_iteration;   /* ce.lastUsedIteration                              */
    uint32_t flags;
    int32_t reserved;
} mmp_cache_entry;

/* MaxConcCacheEntry (MM.java:2641-2797): what a mesh that runs with limitModelConcurrency == true keeps per loaded model — one
 * row per cache entry, in the order of the entries.  The rate task evaluates getRpmScaleThreshold(true) on it (the row's own
 * threshold replaces scale_up_rpm_threshold: "latency-based" scaling, MM.java:5677, :5702-5707), the janitor
 * getRpmScaleThreshold(false) and queuedRequestCount() (:6294-6305). */
#define MMP_CONC_COUNT_BITS 21 /* MM.java:2653: completed invocations in the low bits of countAndTimeSum, the sum of their
                                  durations in 1/10 ms above */
typedef struct {
    int64_t count_and_time_sum; /* countAndTimeSum.sum()                      */
    int64_t prior_sum;          /* priorSum                                   */
    int32_t prior_count;        /* priorCount                                 */
    int32_t max_conc;           /* maxConc                                    */
    int32_t queued_requests;    /* queuedRequestCount() (the janitor, :6303)  */
    int32_t reserved;
} mmp_conc_entry;
typedef struct {
    int32_t threshold;       /* getRpmScaleThreshold(true) as the task got it; 0 for an entry it skipped before the call (:5697) */
    int32_t reset;           /* 1: the call took countAndTimeSum.sumThenReset() (:2771): the caller resets its adder and stores: */
    int64_t new_prior_sum;   /*    priorSum   (unchanged when reset == 0)                                                        */
    int32_t new_prior_count; /*    priorCount                                                                                    */
    int32_t reserved;
} mmp_conc_out;
typedef struct {
    int64_t dynamic_rpm_scale_constant; /* 600 000 * percentage / 100, MM.java:370, :732                           */
    double average_model_parallelism;   /* the task's field going into this run (:5634; 1.0 before the first run)   */
} mmp_conc_params;
typedef struct {
    double average_model_parallelism; /* after this run: max(1.0, (double) modelParallelismSum / entries), :5815-5818 — the
                                         input value when the run returned early.  The path's only floating-point value: a sum
                                         of ints, one IEEE division, one comparison — compared EXACTLY with the reference's    */
    int32_t exclude_set_rpms;         /* (int) (900.0 * averageModelParallelism) of the INPUT value: getExcludeSet's threshold, :5836 */
    int32_t model_parallelism_sum;    /* modelParallelismSum, :5706                                                          */
} mmp_conc_result;

/* rateTrackingTask (MM.java:5636-5832).  mmp_scaleup_plan: limitModelConcurrency == false; mmp_scaleup_plan_conc: true. */
typedef struct {
    int32_t self_pod;
    int32_t iteration_counter;
    int32_t second_copy_max_age_iters; /* MM.java:5621 */
    int32_t second_copy_min_age_iters; /* MM.java:5622 */
    int32_t scale_up_rpm_threshold;    /* MM.java:240  */
    int32_t our_rpm;                   /* invokeCounter.getBusyness(), MM.java:5837 */
    int64_t now;
    int64_t last_check_time;
    int64_t rate_check_interval_ms;        /* MM.java:238  */
    int64_t second_copy_lru_threshold_ms;  /* MM.java:5628 */
    int64_t assume_completed_ms;           /* loadingTimeStats(type).assumeCompletedAfterMillis() */
} mmp_scaleup_params;
#define MMP_SCALE_NONE 0
#define MMP_SCALE_SECOND_COPY 1 /* ensureLoadedInternalAsync(id, lastTime, w, excludeThisInstance, 0), MM.java:5755 */
#define MMP_SCALE_UP 2          /* ensureLoadedInternalAsync(id, now+20s, w, exclude, copies-1), MM.java:5805     */
typedef struct {
    int32_t action;
    int32_t copies;    /* copiesToLoad */
    int64_t timestamp; /* lastUsedTime to pass to the load-target decision */
    int32_t new_i1, new_i2; /* updated earlierUseIteration / lastUsedIteration */
    int32_t heavy;     /* ce.setLastHeavyTime(now) */
    int32_t rpm;
} mmp_scaleup_out;

/* janitor scale-down (MM.java:6110-6145, removeModelCopies :6197-6310). */
typedef struct {
    int32_t self_pod;
    int32_t shutting_down;
    int64_t now;
    int64_t last_check_time;
    int64_t rate_check_interval_ms;
    int64_t adjusted_cache_capacity; /* getAdjustedCacheCapacity(), MM.java:6117 */
    int32_t scale_up_rpm_threshold;
    int32_t reserved;
} mmp_scaledown_params;

/* ---- lifecycle --------------------------------------------------------- */
int mmp_abi_version(void);
int mmp_create(const mmp_config *cfg, mmp_ctx **out);
void mmp_destroy(mmp_ctx *ctx);
/* Text of the CALLING THREAD's last failure in this library (any context; ctx may be NULL).  The pointer stays
 * valid until the same thread fails again: concurrent callers never see each other's message. */
const char *mmp_last_error(mmp_ctx *ctx);
/* 1 = hip (single device). There is no host backend. */
int mmp_backend(mmp_ctx *ctx);

/* MM.java:765-771 */
int64_t mmp_min_space_units(int32_t default_model_size_units, int32_t loading_threads,
                            int64_t capacity_units, int have_unload_manager);

/* ---- snapshot: what clusterState/registry/typeConstraints hold --------- */
/* Replace the whole instance table (MM.java:332 clusterState, fed by
 * handleInstanceTableChange MM.java:1455). Host pointer, copied. */
int mmp_pods_load(mmp_ctx *ctx, const mmp_pod_row *rows, int32_t n_pods);
/* Upsert / delete single rows by index (ENTRY_ADDED/UPDATED/DELETED,
 * MM.java:1476-1542). idx[i] may equal the current pod count to append. */
int mmp_pods_upsert(mmp_ctx *ctx, const int32_t *idx, const mmp_pod_row *rows, int32_t n);
int mmp_pods_remove(mmp_ctx *ctx, const int32_t *idx, int32_t n);
/* TypeConstraintManager.getCandidateInstances / getPreferredInstances
 * (TypeConstraintManager.java:242-251) as bitmaps over pod index, row-major
 * [n_types][ceil(n_pods/64)] uint64 words, bit p%64 of word p/64.
 * has_allowed[t]==0 / has_prefer[t]==0 mean the Java returned null.
 * n_types==0 means typeConstraints==null. */
int mmp_types_load(mmp_ctx *ctx, int32_t n_types, const uint64_t *allowed, const uint64_t *prefer,
                   const uint8_t *has_allowed, const uint8_t *has_prefer);
/* Rebuild the per-type instance sets from labels ON THE DEVICE (row a18): labels are interned to
 * bits; pod_labels[p] = the instance's label set, required[t]/preferred[t] = the type's
 * requiredLabels / preferredLabels (TypeConstraintManager.java:337-447, :478-486, :680-747).
 * Installs n_types+1 type rows for the next commit: row n_types is the row for model types that
 * are not in the config (no constraint, defaultPreferredInstances). Optional outputs (may be
 * NULL) return the computed tables in the mmp_types_load format with n_types+1 rows. */
int mmp_types_from_labels(mmp_ctx *ctx, int32_t n_types, const uint64_t *required, const uint64_t *preferred,
                          const uint64_t *pod_labels, uint64_t *allowed_out, uint64_t *prefer_out,
                          uint8_t *has_allowed_out, uint8_t *has_prefer_out);
/* UpgradeTracker.getLikelyReplacedReplicaSets (UpgradeTracker.java:78). */
int mmp_replaced_rs_load(mmp_ctx *ctx, const int32_t *replica_sets, int32_t n);
/* UpgradeTracker as a stateful part of the context (row a19; UpgradeTracker.java:85-200): the Java
 * instance-table listener forwards its three calls (MM.java:1532,1553,1563).  labels_key = identity of
 * the record's labels array as the reference's HashMap<String[],..> sees it (0 for NO_LABELS),
 * replica_set = interned id.substring(0,6) or -1 if |id| < 7.  The resulting replica-set list replaces
 * the one given to mmp_replaced_rs_load and takes effect at the next commit. */
int mmp_upgrade_instance_added(mmp_ctx *ctx, int64_t labels_key, int32_t replica_set, int64_t start_time, int64_t now_ms);
int mmp_upgrade_instance_removed(mmp_ctx *ctx, int64_t labels_key, int32_t replica_set, int64_t now_ms);
int mmp_upgrade_housekeeping(mmp_ctx *ctx, int64_t now_ms);
/* getLikelyReplacedReplicaSets(): up to max entries (replica set, expiry); *n_out = entries in the map. */
int mmp_upgrade_replaced(mmp_ctx *ctx, int32_t *rs_out, int64_t *expiry_out, int32_t max, int32_t *n_out);
/* The model registry view (MM.java:308). ent_pod / ent_time have n_entries items. */
int mmp_models_load(mmp_ctx *ctx, const mmp_model_row *rows, int32_t n_models,
                    const int32_t *ent_pod, const int64_t *ent_time, int32_t n_entries);
/* Registry events (the registry's KV listener, MM.java:628; ModelRecord is replaced as a whole on every
 * change): rows[i] replaces model idx[i] (idx[i] == current model count appends); rows[i].ent_off indexes
 * the ent_pod / ent_time arrays of THIS call.  A deleted record is upserted as an empty row.  When a model
 * appears twice the last row wins.  O(rows + entries) per call: the new entries are appended to an
 * arena, the rows (and their resolved exclusion positions) are rewritten in place; the arena is squeezed
 * when it holds more garbage than live entries.  Takes effect immediately (no commit needed: the
 * registry is not part of the snapshot). */
int mmp_models_upsert(mmp_ctx *ctx, const int32_t *idx, const mmp_model_row *rows, int32_t n, const int32_t *ent_pod,
                      const int64_t *ent_time, int32_t n_entries);
/* Rank pods by PLACEMENT_ORDER (MM.java:4646-4703) on the device and publish
 * the new immutable snapshot. MMP_EORDER if the comparator is inconsistent.
 * Wait-free for the latency path: the snapshot is built beside the published one and published with a
 * pointer swap; concurrent calls that ride the latency slots — mmp_place_batch up to 4096 decisions,
 * mmp_gate_batch up to 1820 requests, mmp_evict_batch up to 2048 evaluations — and mmp_place_batch_dev
 * launches keep answering for the published snapshot until then.  Calls that stage through the context's
 * batch stream (larger host-pointer batches, mmp_serve_batch, the plan calls, mmp_cache_replay) share that
 * stream and its scratch with the commit and therefore queue behind a running one; so do loaders of the
 * commit's inputs and other commits. */
int mmp_snapshot_commit(mmp_ctx *ctx);
/* handleInstanceTableChange delivers ONE InstanceRecord per event (MM.java:1455-1568): when at most 16 rows were written
 * (mmp_pods_upsert / _remove / _ingest_json) since the published snapshot and PLACEMENT_ORDER is a total order on the table
 * before and after, the commit re-ranks by insertion — the unchanged rows keep their relative order, the changed ones are
 * placed by binary search with the literal comparator — instead of sorting; the result is the same snapshot.
 * *n_commits_out = commits that took that path on this context (diagnostics; MMP_NO_DELTA=1 in the environment disables it). */
int mmp_delta_commits(mmp_ctx *ctx, int64_t *n_commits_out);
/* The per-type SHORTLISTS of the published snapshot (diagnostics).  What getNext's walk (MM.java:4806-4947: first eligible instance,
 * preference step, the three breaks, count) yields depends on the request only through positions of its own — its exclusions, the
 * calling instance — that lie INSIDE the shortlist, and through one bit, the fresh-row test of :4913-4922.  commit records, per type row
 * (the first 12) and per value of that bit, the shortlist of a request that has no position of its own in reach; large single-caller
 * batches (mmp_place_batch_c / _c_dev) decide a request from it after checking exactly that, and every other request by the ordinary
 * path in the same launch (results identical either way; MMP_NO_MEMO=1 in the environment keeps every request on the ordinary path).
 * rows[2 * t + bit] = {valid, lo, hi, n_candidates}: the list holds for requests without a position in [lo, hi).
 * *n_rows_out = 2 * min(type rows, 12); rows beyond cap_rows are not written. */
typedef struct {
    int32_t valid;
    int32_t lo, hi;
    int32_t n_candidates;
} mmp_shortlist_row;
int mmp_shortlists(mmp_ctx *ctx, mmp_shortlist_row *rows, int32_t cap_rows, int32_t *n_rows_out);
/* The same for the LONG shortlists of a cluster whose instances are (nearly) all full (diagnostics; ModelMesh.java:4880-4991 through the
 * prefix tables): there a shortlist spans the table and a request always has positions of its own inside it, which the prefix-table
 * path treats as corrections (count, audit hash, the pick's rank) of a list it never builds.  The walk itself — first eligible
 * instance, preference step, break scans — depends on the request only when an exclusion or the calling instance sits on a position
 * that steers it; commit records it per type row (every row) and per value of the fresh-row bit, and a request none of whose own
 * positions is one of those is decided from the record (results identical; MMP_NO_LONG_MEMO=1 in the environment: no records).
 * rows[2 * t + bit] = {valid, lo = the type's first eligible position, hi = where the list ends, n_candidates}; *n_rows_out = 2 * type
 * rows (0: no records for this snapshot). */
int mmp_long_shortlists(mmp_ctx *ctx, mmp_shortlist_row *rows, int32_t cap_rows, int32_t *n_rows_out);
/* Large batches (request rows from 393 216 decisions, the single-caller form from 524 288; host-pointer and device-pointer calls alike)
 * are decided by TWO launches on the call's stream: the first checks every request against the shortlists above and decides what they
 * cover — on the bench configuration 99.97 % — the second, a few workgroups, decides the rest by the ordinary path (results identical
 * either way; MMP_NO_SPLIT=1 in the environment keeps such batches in one launch).  The second launch is hidden behind the first launch of
 * the next batch only if that one runs on ANOTHER hardware queue: a host that issues batches from several streams should give each a queue
 * of its own (GPU_MAX_HW_QUEUES >= its streams + the library's: 8 for four).  A second launch that finds more than 1/32 of its batch left
 * switches the split off until the next commit.  Diagnostics: *n_split_out = batches issued that way on this
 * context, *off_out = 1 while the split is switched off (either may be null). */
int mmp_split_batches(mmp_ctx *ctx, int64_t *n_split_out, int32_t *off_out);
/* clusterState iteration order (the `getCacheState` dump, MM.java:5552-5608).
 * order_out has room for n_pods ints; *n_out = rows actually in the set. */
int mmp_get_order(mmp_ctx *ctx, int32_t *order_out, int32_t *n_out);
/* ClusterStats of the committed snapshot (MM.java:1570-1591). */
int mmp_cluster_stats(mmp_ctx *ctx, mmp_stats *out);
/* With type constraints the mesh does not use the cluster-wide stats everywhere (TypeConstraintManager): the
 * instances are partitioned by their ProhibitedTypeSet — the constrained types they cannot host — each
 * partition has its own stats (InstanceSetStatsTracker), typeSetStats(type) is the sum over the partitions
 * that can host the type (MM.java:1432-1439: loadLocal sizing :5169, the onEviction reload rule :2918, the
 * scale-up task :5691) and instanceSetStats() is the partition of this instance (:1446-1448: scale-down
 * :6228).  The library rebuilds all of them at commit and uses them in mmp_gate_batch, mmp_scaleup_plan,
 * mmp_scaledown_plan; these calls read them back.  A partition's lru is the cluster-wide minimum (the Java
 * re-accumulates it over ALL instances on every event, MM.java:1515-1542).  Without type constraints there are
 * no partitions and every type's stats are the cluster's. */
int mmp_type_stats(mmp_ctx *ctx, int32_t type, mmp_stats *out);
int mmp_partition_count(mmp_ctx *ctx, int32_t *n_out);
/* prohibited_out (may be NULL with max_words 0): the partition's prohibited types as a bitset over type rows */
int mmp_partition_stats(mmp_ctx *ctx, int32_t partition, mmp_stats *out, uint64_t *prohibited_out, int32_t max_words);
/* partition of every pod slot (-1: not in the table); *n_out = pod slots */
int mmp_pod_partitions(mmp_ctx *ctx, int32_t *partition_out, int32_t max_pods, int32_t *n_out);

/* ---- decisions --------------------------------------------------------- */
/* n load-target decisions = n × CacheMissForwardingLB.getNext (MM.java:4776-5005).
 * extra_pool: pod indices referenced by reqs[i].extra_off/n_extra. Host pointers. */
int mmp_place_batch(mmp_ctx *ctx, const mmp_place_req *reqs, int32_t n, const int32_t *extra_pool,
                    int32_t n_extra_pool, int64_t now_ms, mmp_place_out *outs);
/* Same, with every buffer already in device memory and launched on `stream`
 * (a hipStream_t, NULL = default) without synchronising.  The library remembers every stream it was handed:
 * before it rewrites state such a launch may still be reading (the second commit after it, registry loads
 * and events, cache-table loads) it waits for those streams as it waits for its own.  A stream must
 * therefore stay valid until mmp_stream_retire() or mmp_destroy().  Several host threads may call the *_dev entry points
 * concurrently, on one stream (NULL included) or on several: the two launches of a split batch (mmp_split_batches) share a buffer per
 * stream and are enqueued back to back under that buffer's lock.  hipStreamPerThread (handle 2) is refused with MMP_EINVAL by every
 * entry point that takes a stream: it names a different stream in every thread that uses it, so the library could neither wait for
 * what another thread enqueued on it before rewriting state nor keep one split buffer per stream.  Pass a stream of your own. */
int mmp_place_batch_dev(mmp_ctx *ctx, const void *d_reqs, int32_t n, const void *d_extra_pool,
                        int64_t now_ms, void *d_outs, void *stream);
/* mmp_place_batch_dev with the pool's length (entries): a request whose exclusion range [extra_off, extra_off + n_extra) does not
 * lie inside the pool is not followed — its result row is {MMP_NONE, MMP_BAD_REQUEST, 0, 0} — instead of being read wherever it
 * points (mmp_place_batch_dev cannot check: it is not told the length).  d_extra_pool may be NULL when n_extra_pool == 0. */
int mmp_place_batch_dev2(mmp_ctx *ctx, const void *d_reqs, int32_t n, const void *d_extra_pool, int32_t n_extra_pool,
                         int64_t now_ms, void *d_outs, void *stream);
/* The single-caller form (mmp_place_caller + mmp_place_req_c, above): host pointers / device pointers.  `caller` is host memory
 * in both (it rides in the kernel's arguments).  The device-pointer call is bounded like mmp_place_batch_dev2.  Results are
 * bit-identical to the same decisions as mmp_place_req rows. */
int mmp_place_batch_c(mmp_ctx *ctx, const mmp_place_caller *caller, const mmp_place_req_c *reqs, int32_t n,
                      const int32_t *extra_pool, int32_t n_extra_pool, int64_t now_ms, mmp_place_out *outs);
int mmp_place_batch_c_dev(mmp_ctx *ctx, const mmp_place_caller *caller, const void *d_reqs, int32_t n, const void *d_extra_pool,
                          int32_t n_extra_pool, int64_t now_ms, void *d_outs, void *stream);
/* k request arrays decided by ONE launch: the same as k calls of mmp_place_batch_dev on `stream` (array i: n[i] requests at
 * d_reqs[i], its own exclusion pool d_extra_pool[i] — the array may be NULL when no request carries extras —, results to
 * d_outs[i]), for a host that holds many batches the size of one request set: a 100k-decision launch lasts an empty launch + one
 * dependent chain (7.8 us, 0.18 of the HBM peak), eight of them in one launch run at the rate of an 800k batch (25 us instead of
 * 62).  The pointer ARRAYS are host memory and are read before the call returns; at most 16 arrays share a launch (more are
 * split).  Results are bit-identical to the separate calls. */
int mmp_place_multi_dev(mmp_ctx *ctx, int32_t k, const void *const *d_reqs, const int32_t *n, const void *const *d_extra_pool,
                        int64_t now_ms, void *const *d_outs, void *stream);
/* The resident decision kernel.  A single request through mmp_place_batch(n = 1) normally costs a kernel launch
 * (6.5 us before the decision's first instruction, tools/micro/doorbell.hip).  mmp_resident(ctx, 1) — or MMP_RESIDENT=1
 * in the environment of mmp_create — keeps ONE wavefront resident instead: its 64 lanes poll 64 request slots in pinned
 * host memory, so up to 64 request threads are decided concurrently and none of them launches anything; a request is
 * a 64-byte store plus a tag, the answer a 16-byte row plus the tag.  It serves requests WITHOUT exclusions of their
 * own (n_extra = 0; the others, and the rare shapes that need the wave path, take the launch path transparently), holds
 * the published snapshot (a commit, registry event or cache-table load stops it and the next request starts a new one)
 * and leaves the GPU by itself after MMP_RESIDENT_IDLE_MS (default 50) without a request.  Results are bit-identical.
 * Two guards: eight hand-backs to the launch path in a row send the next 4096 single requests there directly (a table on
 * which most decisions need the wave path), and three answers in a row slower than 20 ms from a kernel that was not
 * restarted meanwhile switch the resident path off for the context (mmp_last_error says so). */
int mmp_resident(mmp_ctx *ctx, int enable);
int mmp_resident_stats(mmp_ctx *ctx, uint64_t *launches, uint64_t *served, uint64_t *punted);
/* Submission threads.  One host thread spends ~3 us in HIP's launch path per kernel — more than a 100k-decision batch
 * takes the GPU when several are in flight.  mmp_issue_threads(ctx, n) starts n helper threads (they spin: use them for
 * bursts) and mmp_place_batch_dev then only validates, appends a descriptor to the ring of the helper that owns the
 * stream (launches on one stream keep their order) and returns; the helper captures the published snapshot and launches.
 * mmp_issue_flush returns once everything submitted so far has been handed to the HIP stream (first launch error, if
 * any); call it before synchronising the streams.  n = 0 stops the helpers. */
int mmp_issue_threads(mmp_ctx *ctx, int32_t n);
int mmp_issue_flush(mmp_ctx *ctx);
/* Forget a caller-owned stream (waits for what was enqueued on it first, then frees the stream's split-batch buffer); call before
 * destroying a stream that was passed to a *_dev entry point.  A context keeps split-batch buffers for 64 streams at a time: batches
 * on a stream beyond those go unsplit (same results) until a retire frees a buffer. */
int mmp_stream_retire(mmp_ctx *ctx, void *stream);

/* n serve-target decisions = n × ForwardingLB.getNext (MM.java:4315-4392).
 * counters: the requests' mmp_serve_counter entries (see mmp_serve_req); excl_pod / excl_time: pairs referenced by
 * excl_off.  O(copies) per request on both sides of the boundary; calls of up to 1024 requests (8192 counters, 4096
 * exclusion pairs) ride the latency slots like mmp_place_batch's. */
int mmp_serve_batch(mmp_ctx *ctx, const mmp_serve_req *reqs, int32_t n, const mmp_serve_counter *counters,
                    int32_t n_counters, const int32_t *excl_pod, const int64_t *excl_time, int32_t n_excl_pool,
                    int64_t now_ms, mmp_serve_out *outs);

/* Per-pod cache segments for eviction: seg_off has n_caches+1 entries; entry i
 * of a segment is the i-th node of that cache's evictionDeque (oldest first). */
int mmp_caches_load(mmp_ctx *ctx, int32_t n_caches, const int32_t *seg_off, const int64_t *last_used,
                    const int32_t *weight, const int64_t *capacity);
int mmp_evict_batch(mmp_ctx *ctx, const mmp_evict_req *reqs, int32_t n, int64_t now_ms,
                    mmp_evict_out *outs);

/* Stateful caches: entry i of cache c's segment is the i-th node of its evictionDeque (oldest first)
 * with its key; ubm may be NULL (no cache is managed). */
int mmp_caches_load_keyed(mmp_ctx *ctx, int32_t n_caches, const int32_t *seg_off, const int64_t *last_used,
                          const int32_t *weight, const int32_t *key, const int64_t *capacity, const mmp_ubm_state *ubm);
/* Apply n_ops operations (each cache's operations in the order given) to the stateful caches.
 * evicted_keys has room for max_evicted keys; *n_evicted_slots = slots the call used (outs index into
 * it).  MMP_EINVAL if one cache's entries + inserts exceed the 2048-slot tile or max_evicted is too small. */
int mmp_cache_replay(mmp_ctx *ctx, const mmp_cache_op *ops, int32_t n_ops, int64_t now_ms, mmp_cache_op_out *outs,
                     int32_t *evicted_keys, int32_t max_evicted, int32_t *n_evicted_slots);
/* Read one cache back (deque order). */
int mmp_cache_read(mmp_ctx *ctx, int32_t cache, int32_t max_entries, int64_t *last_used, int32_t *weight, int32_t *key,
                   int32_t *n_out, int64_t *capacity, int64_t *weighted_size, mmp_ubm_state *ubm);

/* ---- the stateful caches by model id (cache_keyed_kernels.hpp) -----------------------------------------------------------------
 * runtimeCache maps a model id to its CacheEntry (MM.java:2863-2913).  Caches loaded through mmp_caches_load_keyed_k are BOUND:
 * the key of an entry is the registry row its model id names, the device resolves every id, and what a replay evicts comes back
 * as ids — ready for the MMP_ROP_DEREGISTER ops of mmp_registry_ops_k that follow each eviction (onEviction -> deregisterModel).
 * The host invents no key and keeps no map.  Caches loaded through mmp_caches_load_keyed are unbound; the plain calls above behave
 * on both kinds exactly as they always did.  mmp_model_ids_load drops the binding (the contents stay): the _k calls then answer
 * MMP_ESTATE until the next mmp_caches_load_keyed_k.  mmp_models_retire carries bound caches along (see there).
 * Every _k call takes the locks of the plain cache calls, answers MMP_ESTATE as mmp_model_ids_resolve does (no id table, or the
 * registry resized by index since) and when the caches are not bound, and takes keys as mmp_model_ids_resolve does: raw bytes,
 * n + 1 monotone offsets that need not start at 0, the empty id an ordinary id. */
#define MMP_COPK_RAW_KEY 1                  /* mmp_cache_op.reserved: the op keeps its `key`, which must be MMP_UNLOADBUF_KEY        */
#define MMP_CKEY_LIVE 0                     /* key_status_out: the id names a live record                                           */
#define MMP_CKEY_EMPTY_ROW 1                /* the row exists and its record is deleted; the op ran as usual                        */
#define MMP_CKEY_UNKNOWN 2                  /* the table does not know the id                                                       */
#define MMP_CACHE_KEY_UNKNOWN (-2147483647 - 1) /* the key a non-inserting op under an unknown id runs with: no cache can hold it  */
/* mmp_caches_load_keyed with one id per entry, resolved on the device: entry e has the id keys[key_off[e], key_off[e+1]), E =
 * seg_off[n_caches] ids in all.  is_unloadbuf (E bytes, may be NULL): a marked entry is the manager's pseudo-entry, gets
 * MMP_UNLOADBUF_KEY and its span is not read.  An id whose row is the empty row of a deleted record is accepted (the janitor
 * exists to remove such entries).  key_row_out (may be NULL) receives the E keys.  MMP_EINVAL with nothing changed — the caches
 * loaded before, bound or not, stay as they were: what mmp_caches_load_keyed refuses, non-monotone key offsets, an id the table
 * does not know (mmp_last_error names the lowest such entry). */
int mmp_caches_load_keyed_k(mmp_ctx *ctx, int32_t n_caches, const int32_t *seg_off, const int64_t *last_used,
                            const int32_t *weight, const char *keys, const int32_t *key_off, const uint8_t *is_unloadbuf,
                            const int64_t *capacity, const mmp_ubm_state *ubm, int32_t *key_row_out);
/* mmp_cache_replay by model id.  Op i is evaluated exactly as mmp_cache_replay evaluates it with `key` = the row
 * mmp_model_ids_resolve answers for key i (the row as the table answers it: the entry of a deleted record is still found, read and
 * removed); the `key` the caller sent is never read.  Exceptions: an op with reserved == MMP_COPK_RAW_KEY must carry key ==
 * MMP_UNLOADBUF_KEY and keeps it; the keyless codes (MMP_COP_UBM_SPACE_IS_READY, _CLAIM_SPACE, _UNLOAD_COMPLETE, _DISCARD_FAILED)
 * have none; neither reads its span.  key_status_out[i] = MMP_CKEY_* (MMP_CKEY_LIVE for those two kinds); key_row_out[i] = the key
 * the op ran with (-1 for a keyless code).  Under an UNKNOWN id a non-inserting op runs with MMP_CACHE_KEY_UNKNOWN, i.e. is
 * answered as the reference answers an absent key (with what adjustWeightAfterLoad does to the manager's sums); an inserting op
 * (MMP_COP_PUT_IF_ABSENT, _UBM_INSERT_NEW_ENTRY, _UBM_INSERT_FAILED_PLACEHOLDER) is NOT RUN — the mesh never loads a model without
 * a record — and its out row carries result 0, n_evicted 0 and the cache's state as the preceding op left it; the slot sizing
 * still counts it as a possible insert (an upper bound).
 * outs, evicted_rows, max_evicted, n_evicted_slots: as in mmp_cache_replay, the evicted keys being rows; a slot no op used holds
 * -1.  The ids of the evicted rows are gathered on the device in the same hold of the locks: ev_id_off_out (*n_evicted_slots + 1
 * words; room for max_evicted + 1) are offsets into ev_id_bytes_out, an unused slot has an empty span; *n_id_bytes_out = the bytes
 * needed, always.  With max_id_bytes below that the offsets are returned and the bytes are not — the replay is applied all the
 * same (it is stateful and cannot be asked twice) and the context keeps the record: mmp_cache_evicted_ids returns the same offsets
 * and bytes until the next mmp_cache_replay_k or cache load.  The record holds bytes, not rows: a mmp_models_retire in between
 * cannot change it.  key_status_out, key_row_out, ev_id_bytes_out (with max_id_bytes 0) and ev_id_off_out may be NULL.
 * MMP_EINVAL with nothing changed: what mmp_cache_replay refuses, keys without key_off or the reverse, neither with n_ops > 0,
 * non-monotone offsets, reserved outside {0, MMP_COPK_RAW_KEY}, MMP_COPK_RAW_KEY with another key.  n_ops == 0 is valid (and
 * leaves an empty record). */
int mmp_cache_replay_k(mmp_ctx *ctx, const mmp_cache_op *ops, int32_t n_ops, const char *keys, const int32_t *key_off, int64_t now_ms,
                       int32_t *key_status_out, int32_t *key_row_out, mmp_cache_op_out *outs, int32_t *evicted_rows, int32_t max_evicted,
                       int32_t *n_evicted_slots, char *ev_id_bytes_out, int32_t max_id_bytes, int32_t *ev_id_off_out,
                       int32_t *n_id_bytes_out);
/* The eviction record of the last mmp_cache_replay_k, by the sizes-then-list protocol of mmp_model_ids_get: *n_slots_out and
 * *n_bytes_out always; off_out (n_slots + 1 words) when it is not NULL; the bytes when max_bytes >= *n_bytes_out.  No record
 * (none yet, or a cache load since): 0 slots. */
int mmp_cache_evicted_ids(mmp_ctx *ctx, char *bytes_out, int32_t max_bytes, int32_t *off_out, int32_t *n_slots_out,
                          int32_t *n_bytes_out);
/* mmp_cache_replay_k with the eviction record carrying every victim's lastUsed — the value the clhm hands its listener
 * (ConcurrentLinkedHashMap.java:578-586, node.getLastUsed() at notification), which onEviction passes to deregisterModel ->
 * mr.updateLastUsed (MM.java:2913, :2956) and to ensureLoadedElsewhere (:2922).  It is the time the entry had when evict()
 * unlinked it; a host cannot know it, the deque lives on the device.  Every argument and every output of mmp_cache_replay_k is as
 * there, byte for byte; ev_last_used_out[s] is the time of slot s (room for max_evicted words), 0 for a slot no op used (row -1).
 * ev_last_used_out may be NULL: the times are then kept in the context only.  The context keeps them with the id record, under the
 * same lifetime: mmp_cache_evicted_times.  (The replay kernels of this call are instantiations of their own with a third column on
 * the pending-victim stack — 32 bytes of LDS per deque slot instead of 24; mmp_cache_replay and mmp_cache_replay_k launch the
 * kernels they always did.) */
int mmp_cache_replay_kt(mmp_ctx *ctx, const mmp_cache_op *ops, int32_t n_ops, const char *keys, const int32_t *key_off, int64_t now_ms,
                        int32_t *key_status_out, int32_t *key_row_out, mmp_cache_op_out *outs, int32_t *evicted_rows, int32_t max_evicted,
                        int32_t *n_evicted_slots, char *ev_id_bytes_out, int32_t max_id_bytes, int32_t *ev_id_off_out,
                        int32_t *n_id_bytes_out, int64_t *ev_last_used_out);
/* The times of the last mmp_cache_replay_kt's eviction record, sizes then list: *n_slots_out always (the slots of
 * mmp_cache_evicted_ids), the words when max_slots >= *n_slots_out.  MMP_ESTATE when the last replay recorded none: a plain
 * mmp_cache_replay_k since, a cache load since, or no replay yet. */
int mmp_cache_evicted_times(mmp_ctx *ctx, int64_t *out, int32_t max_slots, int32_t *n_slots_out);
/* mmp_cache_read plus the ids of the deque's entries, gathered on the device: row_out = the keys (rows), id_off_out (min(n,
 * max_entries) + 1 words) offsets into id_bytes_out, *n_id_bytes_out = the bytes of those entries' ids, always; the bytes are
 * written when max_id_bytes is at least that.  The pseudo-entry has row_out == MMP_UNLOADBUF_KEY and an empty span, which tells
 * it apart from the empty id. */
int mmp_cache_read_k(mmp_ctx *ctx, int32_t cache, int32_t max_entries, int64_t *last_used, int32_t *weight, int32_t *row_out,
                     char *id_bytes_out, int32_t max_id_bytes, int32_t *id_off_out, int32_t *n_out, int32_t *n_id_bytes_out,
                     int64_t *capacity, int64_t *weighted_size, mmp_ubm_state *ubm);

/* n guard evaluations (rows a10/a11/a14/a20). in_use_failure_expiry_ms = IN_USE_LOAD_FAILURE_EXPIRY_MS
 * (MM.java:221). excl_pod/excl_time and explicit_pool are the pools the requests index. */
int mmp_gate_batch(mmp_ctx *ctx, const mmp_gate_req *reqs, int32_t n, const int32_t *excl_pod,
                   const int64_t *excl_time, int32_t n_excl_pool, const int32_t *explicit_pool,
                   int32_t n_explicit_pool, int64_t now_ms, int64_t in_use_failure_expiry_ms,
                   mmp_gate_out *outs);
/* The cache-MISS route of one request: the request guards (as mmp_gate_batch) AND the load target (as mmp_place_batch) of the
 * same model in ONE call — invokeModel evaluates the guards and then asks CacheMissForwardingLB.getNext (MM.java:3603-3626,
 * :4590-4627, :4776).  greqs[i] and preqs[i] name the same model; the gate pools (excl_pod / excl_time / explicit_pool) and the
 * load target's extra_pool are separate, as in the two calls.  Up to 256 requests ride one latency slot: the two kernels are
 * enqueued behind one another on the slot's stream and the call waits ONCE (one request: p50 ~14 us against 23 us for the two
 * calls); larger batches are the two calls.  Rows are bit-identical to the two calls'. */
int mmp_miss_batch(mmp_ctx *ctx, const mmp_gate_req *gate_reqs, const mmp_place_req *place_reqs, int32_t n, const int32_t *excl_pod,
                   const int64_t *excl_time, int32_t n_excl, const int32_t *explicit_pool, int32_t n_explicit,
                   const int32_t *extra_pool, int32_t n_extra_pool, int64_t now_ms, int64_t in_use_expiry_ms, mmp_gate_out *gate_outs,
                   mmp_place_out *place_outs);
/* The cache-hit route of invokeModel in one call and ONE launch: request i's guards (gate_reqs[i], as mmp_gate_batch) and its
 * serve target among the model's copies (serve_reqs[i], as mmp_serve_batch; serve_reqs[i].model == gate_reqs[i].model).  The two
 * request arrays index the SAME (excl_pod, excl_time) pool — cacheHitExcludeTl's MapFilteringSet is one object for goLocal and
 * for ForwardingLB.getNext (MM.java:3634, :4316) — and the serve requests their counters as in mmp_serve_batch.  Results equal
 * those of the two separate calls. */
int mmp_route_batch(mmp_ctx *ctx, const mmp_gate_req *gate_reqs, const mmp_serve_req *serve_reqs, int32_t n,
                    const mmp_serve_counter *counters, int32_t n_counters, const int32_t *excl_pod, const int64_t *excl_time,
                    int32_t n_excl, const int32_t *explicit_pool, int32_t n_explicit, int64_t now_ms,
                    int64_t in_use_failure_expiry_ms, mmp_gate_out *gate_outs, mmp_serve_out *serve_outs);

/* The single-caller forms of the two routes.  About two thirds of a mmp_gate_req + mmp_serve_req (or + mmp_place_req) describe the
 * CALLING INSTANCE, not the request — self, the local cache's capacity / weighted size / oldest time, loadingCount and its cutoff,
 * loadTimeoutMs, getFreshInstanceRecord(), lastPublished, localInvokesInFlight, lastInvokeTime — and a batch is what ONE instance's
 * request threads hand over together.  That side travels once per call (mmp_seam_caller, 112 bytes); a route request is 48 + 24
 * bytes instead of 144 + 48, a miss request 48 + 24 instead of 144 + 64.
 *
 * THE RULE: request i of a call is decided exactly as the existing call decides these rows —
 *   gate row   {model = g.model, caller.self_pod, flags = caller.gate_flags | g.flags, g.excl_off, g.n_excl, g.explicit_off,
 *               g.n_explicit, g.size_hint, g.last_used_time, caller.cache_capacity, caller.cache_weighted_size,
 *               caller.cache_oldest_time, g.loader_predicted, caller.loading_count, caller.weight_predict_cutoff, reserved = 0,
 *               g.loaded_time, caller.load_timeout_ms, caller.fresh_*, caller.last_published}
 *   serve row  {g.model, caller.self_pod, s.flags, caller.local_in_flight, caller.last_invoke_time, s.assume_completed_ms,
 *               g.excl_off, g.n_excl, s.cnt_off, s.n_cnt}     (the serve half reads the GATE row's exclusion range: the two
 *               selections share one MapFilteringSet, MM.java:3634, :4316)
 *   place row  as mmp_place_batch_c defines it from place_caller and place_reqs[i]
 * (g = gate_reqs[i], s = serve_reqs[i]), and the results are those rows' results, byte for byte.  Validation is that of the
 * expanded rows: the MMP_EINVAL cases of mmp_route_batch / mmp_miss_batch (null arguments, negative counts, ranges outside the
 * pools, gate_reqs[i].model != place_reqs[i].model), a NULL caller or place_caller as well, all with the outputs untouched;
 * MMP_ESTATE as for the existing calls; n = 0 is a valid call.  `caller` / `place_caller` are host memory (they ride in the
 * kernels' arguments).  Calls within the existing calls' latency-slot sizes (256 requests, their pool limits) are written out as
 * full rows and take that path; larger ones stage the compact rows as they are and run kernels of their own on them
 * (csrc/seam_caller_kernels.hpp). */
typedef struct {                 /* the calling instance's side of a batch of route / miss requests — 112 bytes */
    int32_t  self_pod;
    uint32_t gate_flags;         /* MMP_GATE_* bits ORed into every request's flags */
    int32_t  loading_count;
    int32_t  weight_predict_cutoff;
    int64_t  cache_capacity, cache_weighted_size, cache_oldest_time;
    int64_t  load_timeout_ms;
    int64_t  fresh_lru, fresh_capacity, fresh_used;
    int32_t  fresh_count, fresh_loading_threads, fresh_in_progress, fresh_rpm;
    int64_t  last_published;
    int32_t  local_in_flight;    /* serve half: localInvokesInFlight (MM.java:4303) */
    int32_t  reserved;
    int64_t  last_invoke_time;   /* serve half: lastInvokeTime (MM.java:4304) */
} mmp_seam_caller;

typedef struct {                 /* the request's own side of mmp_gate_req — 48 bytes */
    int32_t  model;
    uint32_t flags;              /* MMP_GATE_*; the request's flags are caller.gate_flags | flags */
    int32_t  excl_off, n_excl;
    int32_t  explicit_off, n_explicit;
    int32_t  size_hint;
    int32_t  loader_predicted;
    int64_t  last_used_time;
    int64_t  loaded_time;
} mmp_gate_req_c;

typedef struct {                 /* the request's own side of mmp_serve_req — 24 bytes */
    uint32_t flags;              /* MMP_SERVE_* */
    int32_t  cnt_off, n_cnt;
    int32_t  reserved;
    int64_t  assume_completed_ms;
} mmp_serve_req_c;

int mmp_route_batch_c(mmp_ctx *ctx, const mmp_seam_caller *caller, const mmp_gate_req_c *gate_reqs,
                      const mmp_serve_req_c *serve_reqs, int32_t n, const mmp_serve_counter *counters, int32_t n_counters,
                      const int32_t *excl_pod, const int64_t *excl_time, int32_t n_excl, const int32_t *explicit_pool,
                      int32_t n_explicit, int64_t now_ms, int64_t in_use_expiry_ms, mmp_gate_out *gate_outs,
                      mmp_serve_out *serve_outs);

int mmp_miss_batch_c(mmp_ctx *ctx, const mmp_seam_caller *caller, const mmp_place_caller *place_caller,
                     const mmp_gate_req_c *gate_reqs, const mmp_place_req_c *place_reqs, int32_t n,
                     const int32_t *excl_pod, const int64_t *excl_time, int32_t n_excl, const int32_t *explicit_pool,
                     int32_t n_explicit, const int32_t *extra_pool, int32_t n_extra, int64_t now_ms,
                     int64_t in_use_expiry_ms, mmp_gate_out *gate_outs, mmp_place_out *place_outs);

/* The single-caller forms BY MODEL ID.  The three calls above name a request's model by registry row, and a caller that keeps no id
 * map (the id table lives on the device: mmp_model_ids_load, below) would first ask mmp_model_ids_resolve — a call that takes the
 * batch lock and queues behind every large batch.  These forms take the model's KEY instead (the raw bytes of the model id, as the
 * registry listener hands them to mmp_models_events_json) and resolve it on the device inside the same call: one latency slot, one
 * stream, one wait, no batch lock (csrc/keyed_kernels.hpp).
 *
 * Key i is keys[key_off[i], key_off[i + 1]): n + 1 monotone offsets, under the conventions of mmp_model_ids_resolve.  The `model`
 * field of the request rows is IGNORED on input, and the caller's arrays are never written (mmp_miss_batch_c's "names two models"
 * check has no counterpart: both halves take the key's row).  model_idx_out (n words, may be NULL) receives the row each key
 * resolved to, or -1.
 *
 * THE RULE BY KEY: request i is decided exactly as the existing _c call decides the same rows with model = r, where r is the row
 * mmp_model_ids_resolve answers for key i against the id table as published at the moment the call captured it; an unknown id is
 * r = -1, which every decision treats as "no such model", as it treats any model outside [0, n_models).  The result rows are those
 * rows' results byte for byte, and model_idx_out[i] = r.  A registry event batch (mmp_models_events_json) publishes the ids that
 * join together with their registry rows: a call sees a batch before or after, never an id whose row the registry does not have.
 *
 * MMP_EINVAL, every output untouched: everything the _c forms refuse; a NULL key_off with n > 0; offsets that are not monotone; NULL
 * keys with key bytes present.  MMP_ESTATE: as the _c forms (no commit yet, a pod-axis shard context), and under the conditions of
 * the id table's guard — no mmp_model_ids_load yet, or the registry was resized by index since.  n = 0 is a valid call.  Up to 256
 * requests with up to 16384 key bytes (and the pools of the _c forms' latency path; the load targets' extra pool up to 2048) ride a
 * latency slot; larger calls are staged under the batch lock like every large call. */
int mmp_place_batch_ck(mmp_ctx *ctx, const mmp_place_caller *caller, const mmp_place_req_c *reqs, int32_t n, const char *keys,
                       const int32_t *key_off, const int32_t *extra_pool, int32_t n_extra, int64_t now_ms, mmp_place_out *outs,
                       int32_t *model_idx_out);
int mmp_route_batch_ck(mmp_ctx *ctx, const mmp_seam_caller *caller, const mmp_gate_req_c *gate_reqs,
                       const mmp_serve_req_c *serve_reqs, int32_t n, const char *keys, const int32_t *key_off,
                       const mmp_serve_counter *counters, int32_t n_counters, const int32_t *excl_pod, const int64_t *excl_time,
                       int32_t n_excl, const int32_t *explicit_pool, int32_t n_explicit, int64_t now_ms, int64_t in_use_expiry_ms,
                       mmp_gate_out *gate_outs, mmp_serve_out *serve_outs, int32_t *model_idx_out);
int mmp_miss_batch_ck(mmp_ctx *ctx, const mmp_seam_caller *caller, const mmp_place_caller *place_caller,
                      const mmp_gate_req_c *gate_reqs, const mmp_place_req_c *place_reqs, int32_t n, const char *keys,
                      const int32_t *key_off, const int32_t *excl_pod, const int64_t *excl_time, int32_t n_excl,
                      const int32_t *explicit_pool, int32_t n_explicit, const int32_t *extra_pool, int32_t n_extra, int64_t now_ms,
                      int64_t in_use_expiry_ms, mmp_gate_out *gate_outs, mmp_place_out *place_outs, int32_t *model_idx_out);

/* triggerProactiveLoadsForInstanceSubset (MM.java:6616-6747, excludeTypes == null) over the
 * committed snapshot and the loaded model table (models in registry iteration order): which
 * unloaded models the leader would proactively load, most recently used first. The caller then
 * feeds them to mmp_place_batch with last_used = out_last_used[i] (MM.java:6727). */
int mmp_proactive_plan(mmp_ctx *ctx, int32_t default_model_size_units, int64_t now_ms, int32_t max_out,
                       int32_t *out_model, int64_t *out_last_used, mmp_proactive_info *info);
/* The same plan for ONE instance partition: with type constraints the reaper calls
 * triggerProactiveLoadsForInstanceSubset once per ProhibitedTypeSet partition (MM.java:6473-6488) with that
 * partition's stats, its instances for the free-space budget, and its prohibited types excluded from the
 * candidates; skip_models = the models already triggered for an earlier partition of the same run
 * (allCandidates.set(index, null), :6724).  partition = -1: the whole cluster (typeConstraints == null),
 * which is what mmp_proactive_plan does.  The candidate rule (pruneModelRegistry, :6459-6462, :6574-6577)
 * always uses the cluster-wide stats. */
int mmp_proactive_plan_subset(mmp_ctx *ctx, int32_t partition, const int32_t *skip_models, int32_t n_skip,
                              int32_t default_model_size_units, int64_t now_ms, int32_t max_out, int32_t *out_model,
                              int64_t *out_last_used, mmp_proactive_info *info);

/* The reaper's FIRST half: pruneModelRegistry (MM.java:6524-6609) with pruneMissingInstances (:6752-6784) and
 * repairLastUsedTimeIfNeeded (:6837-6850) — one full pass over the resident registry at one clock value now_ms (> 0).  The
 * reference runs it before triggerProactiveLoadsForInstanceSubset in every reaper run (:6459-6488): a model whose only copies
 * sat on instances that are gone becomes a proactive-load candidate (`insts.isEmpty() && failInsts.size() < 2`, :6574) only once
 * this pass has taken those registrations out.  So: mmp_registry_prune(MMP_PRUNE_APPLY), then mmp_proactive_plan.
 *
 * For every model in registry order, its loaded entries first and then its failed entries, each list in entry (TreeMap) order:
 *   - an entry is EXAMINED unless now - time < gone_after_ms (:6761, strict) or its pod is self_pod (:6765);
 *   - an examined entry whose pod index is < 0 or >= the pod count is UNRESOLVED (the JSON ingest's "id not in the pod table"):
 *     never pruned, never marked, counted in n_unresolved;
 *   - an examined entry's pod is MISSING when its slot of the instance table is a tombstone (MMP_POD_TOMBSTONE; a shutting-down
 *     row is still in instanceInfo and therefore present, :6769-6770);
 *   - missings.putIfAbsent(pod, now) (:6776): a pod first seen missing in this run gets since = now and nothing of it is removed;
 *     an entry is REMOVED iff it is examined, its pod is missing, the pod had a mark before the run and now - since >
 *     gone_after_ms (:6777, strict);
 *   - after the pass (:6601-6606) every mark with now - since > gone_after_ms is dropped, and every mark whose pod is present;
 *   - a record with last_used == INT64_MAX gets now - 3 * lastused_age_on_add_ms (:6843-6844), before the candidate rule reads it.
 * The reference's constants: gone_after_ms = ASSUME_INSTANCE_GONE_AFTER_MS = 600 000, lastused_age_on_add_ms =
 * LASTUSED_AGE_ON_ADD_MS, a run every REGISTRY_REAPER_FREQ_MINS = 7 minutes.
 *
 * The INSTANCE TABLE the pass reads is the one mmp_proactive_plan reads: the rows of the committed snapshot (the last
 * mmp_snapshot_commit), not rows staged since.  A prune followed by a plan sees one table.  MMP_ESTATE before the first commit.
 *
 * An EDIT is what the Java hands to registry.conditionalSetAndGet (:6555) / conditionalSet (:6845): the record without the
 * removed entries and with the repaired last_used.  Edits come in registry order, the removed entries of an edit in list order
 * at removed_out[removed_off, removed_off + n_removed).  The compare-and-set retry against the KV store stays in Java.
 *
 * Not restated here: readOnlyMode (:6543-6550), loadFailureInfos (`secondary.remove`, :6779), the kv-error counter
 * (:6583-6600) and cleanLeaselessEtcdInstanceRecords (:6787).  (The janitor's per-instance registry loop, :6014-6108, which
 * needs the local cache joined in, is mmp_janitor_plan.) */
#define MMP_PRUNE_APPLY 1u /* rewrite the resident registry: rows in place (as mmp_models_upsert does), no commit needed */
#define MMP_PRUNE_DRY 2u   /* compute everything, advance nothing: registry and missing map stay as they are (sizing, diagnostics) */
#define MMP_PRUNE_EDIT_REPAIRED 1u
typedef struct {
    int32_t model;
    int32_t n_loaded_after;
    int32_t n_failed_after;
    uint32_t flags;        /* bit0 (MMP_PRUNE_EDIT_REPAIRED): last_used was Long.MAX_VALUE */
    int32_t removed_off;   /* this edit's entries in removed_out */
    int32_t n_removed;
    int64_t last_used_after;
} mmp_prune_edit;
typedef struct {
    int32_t pod;
    int32_t failed; /* 0: from instanceIds, 1: from loadFailedInstanceIds */
    int64_t time;
} mmp_prune_removed;
typedef struct {
    int32_t n_edits;        /* totals of the run, also when the buffers held only a prefix */
    int32_t n_removed;
    int32_t n_repaired;
    int32_t n_unresolved;
    int32_t n_missing_pods; /* marks held after the run (for a dry or truncated run: that it would hold) */
    int32_t n_new_missing;  /* pods first seen missing in this run */
    int32_t truncated;      /* 1: n_edits > max_edits or n_removed > max_removed */
    int32_t reserved;
} mmp_prune_info;
/* flags = 0: the edits are computed and the missing map advances, the resident registry is left to the caller (who applies the
 * records the KV store accepted through mmp_models_upsert); MMP_PRUNE_APPLY: the library also rewrites the resident registry —
 * the surviving entries are appended to the entry arena on the device and the rows rewritten in place under the protocol of
 * mmp_models_upsert, so decisions and plans see the edited records at once; MMP_PRUNE_DRY (alone).  When an output buffer is
 * too small the prefix that fits and the totals are returned with truncated = 1 and NOTHING is applied or advanced, whatever
 * the flags: the caller repeats the call with larger buffers.  Buffers may be NULL with a capacity of 0. */
int mmp_registry_prune(mmp_ctx *ctx, int32_t self_pod, int64_t now_ms, int64_t gone_after_ms, int64_t lastused_age_on_add_ms,
                       uint32_t flags, mmp_prune_edit *edits_out, int32_t max_edits, mmp_prune_removed *removed_out,
                       int32_t max_removed, mmp_prune_info *info_out);
/* The missing map (`missings`, MM.java:6776): since_out[p] = the time pod p was first seen missing, 0 = no mark; *n_out = pod
 * slots the map covers.  Lifetime: the map is kept BY POD INDEX inside the context; it grows (unmarked) when pods are appended;
 * it survives mmp_pods_load / _upsert / _remove, which keep the index space; mmp_pod_ids_load, which redefines the index space,
 * clears it; mmp_registry_missing_reset is missings.clear() on a leader change (:6427, :6827).
 * LIMIT: a mark of 0 cannot be told from no mark, which is why mmp_registry_prune refuses now_ms <= 0.  The reference run at a
 * clock value of 0 writes the mark 0 and prunes on it one run later; that case, and an entry whose id the instance table does not
 * hold (UNRESOLVED above: the reference prunes it like any missing instance), are kept in tests/golden/ref_registry_edges.npz
 * marked as outside this domain (docs/PARITY.md). */
int mmp_registry_missing_get(mmp_ctx *ctx, int64_t *since_out, int32_t max_pods, int32_t *n_out);
int mmp_registry_missing_reset(mmp_ctx *ctx);

/* a16': what every instance's janitorTask does BEFORE the scale-down of copies — the CACHE LOOP (MM.java:5892-6008) and the
 * REGISTRY LOOP (:6014-6108) — joined against the resident registry at one clock value params->now (> 0).  The output feeds
 * mmp_scaledown_plan / _conc: the candidates are scaleCopiesCandidates (:6017) as complete mmp_cache_entry rows, oldest first.
 *
 * INPUT: one mmp_janitor_entry per local cache entry in runtimeCache.descendingMap() order (most recently used first), without
 * the unload-buffer entry (:5893-5895).  A model appears in at most one row (the cache is keyed by model id); a duplicate, or a
 * model index outside [-1, n_models), is MMP_EINVAL with nothing changed.  params->self_pod is a row of the committed instance
 * table (its id_order places an inserted entry).  MMP_ESTATE before the first commit.
 *
 * CACHE LOOP, per row in order:
 *   - skipped unless MMP_JE_DONE (:5905) and last_used > 0 (:5910);
 *   - last_used == INT64_MAX: the entry is repaired to now - 3 * lastused_age_on_add_ms, the record too if its last_used is
 *     INT64_MAX (:5924-5927), and THE RUN RETURNS (:5929): no later row is looked at, the registry loop does not run, there
 *     are no candidates.  info.stopped_at is that row;
 *   - now - last_used < janitor_freq_secs * 2000 + load_timeout_ms (strict, :5933): only the stale-lastUsed refresh
 *     (:6165-6181: when last_used - record.last_used >= min_stale_age_ms, never for INT64_MAX; updateLastUsed only raises);
 *   - otherwise the registry's timestamp for self_pod is compared with the entry's — loadFailedInstanceIds and
 *     load_complete_timestamp for a MMP_JE_FAILED entry, instanceIds and load_timestamp otherwise (:5950-5953).  Equal: the
 *     refresh, done.  Else, when model == -1, or not MMP_JE_STATE_LIVE, or age(last_unload_attempt_time) <
 *     unload_attempt_recent_ms with age(0) == 0 (:5968-5969, :4162): the entry is REMOVED from the cache.  Else it is
 *     REGISTERED (:5980-5982): instanceIds.put(self_pod, load_timestamp), removeLoadFailure(self_pod),
 *     updateLastUsed(last_used); MMP_JANITOR_EDIT_TIMESTAMP_MISMATCH says a different load timestamp stood there (:5990).
 * REGISTRY LOOP, per model in registry order, on the records AS THE CACHE LOOP LEFT THEM.  The entry it finds is the snapshot's
 * (:5892, :6034): a row the cache loop removed is still found and its FAILED bit read, but getLastUsedTime gives -1 for it.
 *   - remLoaded = loaded && (no row || FAILED) (:6039); updateLastUnloadTime gives 0 when at most two copies are left after
 *     the removal, else now (ModelRecord.java:260-262) — the model row has no such field, the edit reports it;
 *   - remFailed (:6041-6053): the entry is not FAILED, or now - failedTime > expiry (strict), expiry being
 *     load_failure_expiry_ms / 2 when lastUsed > 0 && now - lastUsed < short_expiry_recent_use_ms, else load_failure_expiry_ms;
 *   - updateLastUsed(lastUsed) when either holds, a row exists and lastUsed > 0 (:6066-6073);
 *   - an expired failure record's FAILED entry also leaves the cache (:6089-6091);
 *   - loaded && !remLoaded with lastUsed > 0 is a CANDIDATE (:6092-6099).  The TreeSet compares the time alone (VALUE_COMP,
 *     :6875-6881): a second candidate with an equal time is dropped, the first in registry order stays (info.n_ties).
 *
 * WHERE A REGISTERED ENTRY GOES: instanceIds is in id order.  Where self_pod already stands its time is replaced in place;
 * otherwise it goes in front of the first RESOLVED entry (0 <= pod < pod count) whose id_order is greater, at the end if there
 * is none.  Entries with an unresolved pod keep their place and are never compared.
 *
 * OUTPUT: per input row one action byte — the LAST thing the run did to it; one EDIT per record that changes, in registry
 * order, as registry.conditionalSetAndGet would receive it last (the compare-and-set retry against the KV store stays in
 * Java); the candidates with the index of their input row beside them. */
#define MMP_JE_DONE 1u       /* ce.isDone()                               */
#define MMP_JE_FAILED 2u     /* ce.isFailed()                             */
#define MMP_JE_STATE_LIVE 4u /* CacheEntry.LOADING <= ce.state <= ACTIVE  */
typedef struct {
    int32_t model;                   /* registry row, -1 if registry.get(modelId) == null */
    int32_t weight;                  /* ce.getWeight()                                    */
    int64_t last_used;               /* runtimeCache.getLastUsedTime(modelId); may be INT64_MAX */
    int64_t load_timestamp;          /* ce.loadTimestamp                                  */
    int64_t load_complete_timestamp; /* ce.loadCompleteTimestamp                          */
    int64_t last_unload_attempt_time; /* ce.lastUnloadAttemptTime (-1: never, 0 reads as "now") */
    int64_t interval_count;          /* these five pass through into the candidate row    */
    int64_t last_heavy_time;
    int64_t last_unload_time;
    int32_t earlier_use_iteration;
    int32_t last_used_iteration;
    uint32_t flags;                  /* MMP_JE_*                                          */
    int32_t reserved;
} mmp_janitor_entry; /* 80 bytes */
typedef struct {
    int32_t self_pod;
    int32_t shutting_down;              /* != 0: the run does nothing (:5880)                              */
    int64_t now;
    int64_t janitor_freq_secs;          /* LOCAL_JANITOR_FREQ_SECS = 360                                   */
    int64_t load_timeout_ms;
    int64_t min_stale_age_ms;           /* drawn once per mesh: 6 h + up to 1 h (:6162)                    */
    int64_t load_failure_expiry_ms;     /* LOAD_FAILURE_EXPIRY_MS = 900 000; in use: half of it (:221)     */
    int64_t short_expiry_recent_use_ms; /* SHORT_EXPIRY_RECENT_USE_TIME_MS = 180 000                       */
    int64_t unload_attempt_recent_ms;   /* 600 000 (:1865)                                                 */
    int64_t lastused_age_on_add_ms;     /* LASTUSED_AGE_ON_ADD_MS                                          */
} mmp_janitor_params; /* 72 bytes */
#define MMP_JANITOR_NONE 0       /* skipped, recently used, or not reached                     */
#define MMP_JANITOR_REPAIRED 1   /* INT64_MAX repaired; the run stopped here                   */
#define MMP_JANITOR_REFRESHED 2  /* the record's stale lastUsed was refreshed                  */
#define MMP_JANITOR_IN_ORDER 3   /* timestamps equal, nothing to do                            */
#define MMP_JANITOR_REMOVED 4    /* removed from the cache by the cache loop (:5970)           */
#define MMP_JANITOR_REGISTERED 5 /* left in the cache, the record updated (:5980)              */
#define MMP_JANITOR_EXPIRED 6    /* its failure record expired, removed from the cache (:6091) */
#define MMP_JANITOR_EDIT_REGISTERED 1u
#define MMP_JANITOR_EDIT_TIMESTAMP_MISMATCH 2u
#define MMP_JANITOR_EDIT_REM_LOADED 4u
#define MMP_JANITOR_EDIT_REM_FAILED 8u
#define MMP_JANITOR_EDIT_TOUCHED 16u    /* updateLastUsed raised last_used                 */
#define MMP_JANITOR_EDIT_REPAIRED 32u   /* the record's last_used was INT64_MAX            */
#define MMP_JANITOR_EDIT_UNLOAD_SET 64u /* last_unload_after is to be stored               */
typedef struct {
    int32_t model;
    int32_t n_loaded_after;
    int32_t n_failed_after;
    uint32_t flags;            /* MMP_JANITOR_EDIT_*                                                              */
    int64_t last_used_after;
    int64_t last_unload_after; /* with MMP_JANITOR_EDIT_UNLOAD_SET: 0 or now                                      */
    int64_t inserted_time;     /* with MMP_JANITOR_EDIT_REGISTERED: (self_pod, load_timestamp) was put, and stands */
    int32_t inserted_pos;      /*   at this place of instanceIds after the edit; -1: none, or taken out again     */
    int32_t entry;             /* the model's input row, -1 if it has none                                        */
} mmp_janitor_edit; /* 48 bytes */
typedef struct {
    int32_t n_edits;      /* totals of the run, also when the buffers held only a prefix */
    int32_t n_candidates; /* after the tie drop                                          */
    int32_t n_ties;       /* candidates dropped because an earlier one had their time    */
    int32_t stopped_at;   /* the repaired row, -1 if the run did not stop                */
    int32_t truncated;    /* 1: n_edits > max_edits or n_candidates > max_candidates     */
    int32_t n_action[7];  /* input rows per action byte                                  */
} mmp_janitor_info;
#define MMP_JANITOR_APPLY 1u /* rewrite the resident registry: rows in place (as mmp_models_upsert does), no commit needed */
#define MMP_JANITOR_DRY 2u   /* compute everything, change nothing: the same as flags = 0 here (the plan keeps no state of its
                                own between runs); kept so that callers write the prune and the plan alike */
/* actions_out holds n bytes.  flags = 0: the plan is computed, the resident registry is left to the caller (who applies the
 * records the KV store accepted through mmp_models_upsert); MMP_JANITOR_APPLY: the library also rewrites the resident registry —
 * the edited records' entries, the inserted one among them, are appended to the entry arena on the device and the rows
 * rewritten in place under the protocol of mmp_models_upsert; MMP_JANITOR_DRY (alone).  When edits_out or the candidate
 * buffers are too small the prefix that fits and the totals are returned with truncated = 1 and NOTHING is applied.  Buffers
 * may be NULL with a capacity of 0. */
int mmp_janitor_plan(mmp_ctx *ctx, const mmp_janitor_entry *entries, int32_t n, const mmp_janitor_params *params, uint32_t flags,
                     uint8_t *actions_out, mmp_janitor_edit *edits_out, int32_t max_edits, mmp_cache_entry *candidates_out,
                     int32_t *candidate_rows_out, int32_t max_candidates, mmp_janitor_info *info_out);

/* A census of the resident registry: what the registry listener keeps on every instance (event(), MM.java:2807-2854) and
 * logModelCountMetrics publishes (:6852-6863).  A record is in loadedModelIds iff !instanceIds.isEmpty() (:2828) and in
 * failedModelIds iff hasLoadFailure() (:2829, ModelRecord.java:181-183); both depend on the record alone, so the sizes of the two
 * sets are counts over the registry as it stands.  After mmp_registry_prune / mmp_janitor_plan have rewritten rows on the device
 * this is how a host learns them without reading the registry back.
 *
 * Read-only; needs no committed snapshot (the registry does not depend on one).  Pod indices are those of the STAGED instance
 * table, as in mmp_models_upsert.  The call sees the registry between two writers, never inside one: it takes the registry the
 * way mmp_models_upsert and the applied prune / janitor plan do, and like them it does not hold decisions off. */
typedef struct {
    int32_t n_models;          /* registry.getCount(), :2851, :6862                                            */
    int32_t n_loaded;          /* records with n_loaded > 0 = loadedModelIds.size(), :2828, :2844               */
    int32_t n_failed;          /* records with n_failed > 0 = failedModelIds.size(), :2829, :2845               */
    int32_t n_loaded_and_failed;
    int32_t n_unloaded_used;   /* n_loaded == 0, 0 < last_used < INT64_MAX: the population :6574 draws from     */
    int32_t n_last_used_max;   /* last_used == INT64_MAX: what repairLastUsedTimeIfNeeded (:6837) looks for     */
    int64_t n_entries_loaded;  /* sum of n_loaded                                                               */
    int64_t n_entries_failed;  /* sum of n_failed                                                               */
    int64_t n_entries_unresolved; /* entries whose pod is outside [0, pod slots): ids the table does not know   */
    int32_t copies_hist[5];    /* records with 0, 1, 2, 3, >= 4 instanceIds (a15's second copy, a16's >= 3 rule) */
    int32_t max_copies;        /* the largest n_loaded                                                          */
} mmp_registry_stats;
typedef struct {
    int32_t n_models, n_loaded, n_failed, reserved;
    int64_t n_entries_loaded;
} mmp_registry_type_stats;
/* pod_loaded_out[p] / pod_failed_out[p] = records whose instanceIds / loadFailedInstanceIds hold pod p — hasRegistration
 * (:2856-2858) summed over the registry, per list — for every slot of the pod table, tombstoned ones included.  types_out[t] covers
 * the loaded type table (*n_types_out = 0 without one); a record whose type lies outside it counts in the totals only.
 * *n_pods_out / *n_types_out are always set.  The pod buffers (both or neither) and the type buffer may be NULL with a capacity
 * of 0: that part is not returned.  A capacity that is positive and smaller than the count: MMP_EINVAL, nothing else written. */
int mmp_registry_census(mmp_ctx *ctx, mmp_registry_stats *out, int32_t *pod_loaded_out, int32_t *pod_failed_out, int32_t max_pods,
                        int32_t *n_pods_out, mmp_registry_type_stats *types_out, int32_t max_types, int32_t *n_types_out);

/* The edits an instance makes to ModelRecords itself, as a batch against the resident registry.  Each op names one record
 * (`model`) and one instance (`pod` = the reference's instanceId: a slot of the instance table, present, shutting down or
 * tombstoned); now_ms (> 0) stands for every currentTimeMillis() below.  With r the record of `model`:
 *
 *   MMP_ROP_REGISTER (loadLocal, MM.java:5204-5207) — always an edit (the record is always submitted):
 *     instanceIds.put(pod, load_time): over the entry that is there, else in front of the first RESOLVED entry with a greater
 *     id_order (at the end if there is none; unresolved entries are never compared); removeLoadFailure(pod);
 *     updateLastUsed(last_used == 0 ? now : last_used).
 *   MMP_ROP_LOAD_FAILED (the CacheEntry failure path, :2484-2495):
 *     lu = last_used, or r.last_used when last_used <= 0; instanceIds.remove(pod, load_time) — key present AND time equal — or
 *     else nothing changes; unless MMP_ROPF_SHUTTING_DOWN, loadFailedInstanceIds.put(pod, load_complete_time) (addLoadFailure,
 *     ModelRecord.java:156-167: over the entry that is there, else in id order within that list); updateLastUsed(lu), where an
 *     lu that is still 0 means now (ModelRecord.java:239-246).
 *   MMP_ROP_DEREGISTER (deregisterModel, :2948-2958):
 *     with MMP_ROPF_MATCH_TIME (loadTime != null) the loaded entry goes only if its time == load_time and the failed entry only
 *     if its time == load_complete_time (ModelRecord.java:173-179); without it either goes if present.  Neither: nothing
 *     changes (:2955).  Else updateLastUsed(last_used) (0 = now) and, if the loaded entry went, updateLastUnloadTime(): 0 when
 *     instanceIds.size() <= 2 after the removal, else now (ModelRecord.java:260-262).
 *   MMP_ROP_SCALE_DOWN (removeLocalModelCopyAsync, :6347-6365):
 *     no loaded entry for pod, or its time != load_time: nothing changes (:6348).  Else it is removed, updateLastUnloadTime(),
 *     updateLastUsed(last_used).  loadFailedInstanceIds is not touched.  (isLoadedElsewhere, :6357, is a remote check: the host
 *     sends the op after it.)
 *
 * updateLastUsed only raises (a record at INT64_MAX stays there).  The model row has no lastUnloadTime: the edit reports it.
 * The instance table read for id_order is the committed one, as for mmp_janitor_plan.  The compare-and-set retry against the
 * KV store, loadFailureInfos and the CacheEntry state machine around these sites stay with the caller.
 *
 * MMP_EINVAL, with nothing written or changed: a model outside [0, n_models), a pod outside the instance table, an unknown op
 * or flag bit, now_ms <= 0, two ops naming the same model (an instance has one cache entry per model; a host that needs both
 * flushes between them).  MMP_ESTATE before the first commit.  n = 0 is a valid call with empty outputs. */
#define MMP_ROP_REGISTER 0
#define MMP_ROP_LOAD_FAILED 1
#define MMP_ROP_DEREGISTER 2
#define MMP_ROP_SCALE_DOWN 3
#define MMP_ROPF_SHUTTING_DOWN 1u /* MMP_ROP_LOAD_FAILED: no failure record is written (:2492) */
#define MMP_ROPF_MATCH_TIME 2u    /* MMP_ROP_DEREGISTER: loadTime != null (:2951)              */
typedef struct {
    int32_t model;
    int32_t pod;
    int32_t op;                 /* MMP_ROP_*                                                   */
    uint32_t flags;             /* MMP_ROPF_*                                                  */
    int64_t last_used;
    int64_t load_time;          /* ce.loadTimestamp / loadTime                                 */
    int64_t load_complete_time; /* loadCompleteTimestamp / loadCompletedTime                   */
} mmp_registry_op; /* 40 bytes */
#define MMP_ROP_UNCHANGED 0 /* the Java returned without a compare-and-set */
#define MMP_ROP_EDITED 1
#define MMP_ROP_EDIT_REM_LOADED 1u
#define MMP_ROP_EDIT_REM_FAILED 2u
#define MMP_ROP_EDIT_PUT_LOADED 4u
#define MMP_ROP_EDIT_PUT_FAILED 8u
#define MMP_ROP_EDIT_REPLACED 16u   /* the put found the key: its time was replaced in place */
#define MMP_ROP_EDIT_TOUCHED 32u    /* updateLastUsed raised last_used                       */
#define MMP_ROP_EDIT_UNLOAD_SET 64u /* last_unload_after is to be stored                     */
typedef struct {
    int32_t model;
    int32_t op_index;          /* the op that made this edit                                                     */
    int32_t n_loaded_after;
    int32_t n_failed_after;
    uint32_t flags;            /* MMP_ROP_EDIT_*                                                                 */
    int32_t inserted_pos;      /* where the put entry stands in its list (instanceIds for PUT_LOADED,            */
                               /*   loadFailedInstanceIds for PUT_FAILED) after the edit; -1: nothing was put    */
    int64_t last_used_after;
    int64_t last_unload_after; /* with MMP_ROP_EDIT_UNLOAD_SET: 0 or now                                         */
} mmp_registry_op_edit; /* 40 bytes */
typedef struct {
    int32_t n_edits;           /* totals of the call, also when edits_out held only a prefix */
    int32_t n_unchanged;
    int32_t truncated;         /* 1: n_edits > max_edits                                     */
    int32_t reserved;
    int32_t n_edited_op[4];    /* per MMP_ROP_* kind                                         */
    int32_t n_unchanged_op[4];
    int32_t n_entries_added;   /* puts that found no key                                     */
    int32_t n_entries_removed;
} mmp_registry_ops_info; /* 56 bytes */
#define MMP_ROPS_APPLY 1u /* rewrite the resident registry: rows in place (as mmp_models_upsert does), no commit needed */
#define MMP_ROPS_DRY 2u   /* compute everything, change nothing: the same as flags = 0 here; kept so that callers write the
                             prune, the janitor plan and this alike */
/* status_out holds n bytes (MMP_ROP_UNCHANGED / MMP_ROP_EDITED); edits_out one row per edited record IN OP ORDER — the order
 * the Java would issue its conditionalSetAndGet calls in.  flags = 0: computed only, the resident registry is left to the
 * caller (who applies what the KV store accepted through mmp_models_upsert); MMP_ROPS_APPLY: the edited records' entries are
 * appended to the entry arena on the device and the rows rewritten in place under the protocol of mmp_models_upsert;
 * MMP_ROPS_DRY (alone).  When edits_out is too small the prefix that fits and the totals are returned with truncated = 1 and
 * NOTHING is applied.  edits_out may be NULL with a capacity of 0; a NULL status_out is not
 * returned.
 *
 * This call is by registry row and keeps its 56-byte info and its four kinds: it refuses MMP_ROP_DROP_LOCAL (kind 4) and never
 * answers MMP_ROP_NO_RECORD.  The fifth kind, and all five by model id, are mmp_registry_ops_k below. */
int mmp_registry_ops(mmp_ctx *ctx, const mmp_registry_op *ops, int32_t n, int64_t now_ms, uint32_t flags, uint8_t *status_out,
                     mmp_registry_op_edit *edits_out, int32_t max_edits, mmp_registry_ops_info *info_out);
/* The same edits BY MODEL ID, and the fifth kind: mmp_model_ids_resolve and mmp_registry_ops as ONE staged call under one hold of
 * the batch lock, so that no registry event batch and no mmp_models_retire can land between the row a key names and the edit of
 * that row (csrc/registry_ops_keyed_kernels.hpp: one launch in front of the unchanged evaluation).
 *   ops                n ops; with keys the `model` field is ignored
 *   keys / key_off     n keys, raw id bytes, under the conventions of mmp_model_ids_resolve; BOTH NULL: the by-row form
 *   model_idx_out      n words, may be NULL (by row: ops[i].model again)
 *   status_out, edits_out, max_edits, flags: exactly as mmp_registry_ops (truncation, MMP_ROPS_APPLY / MMP_ROPS_DRY / 0, NULLs)
 *
 *   MMP_ROP_DROP_LOCAL (invokeModel's cache-hit loop: goLocal and getFromCache == null, MM.java:3682-3687) — always an edit (the
 *     record is always submitted, as for MMP_ROP_REGISTER): instanceIds.remove(pod), whether or not the key is there and whatever
 *     its time; updateLastUsed(last_used) (0 = now).  There is NO updateLastUnloadTime — MMP_ROP_EDIT_UNLOAD_SET is never set,
 *     the difference from MMP_ROP_DEREGISTER and MMP_ROP_SCALE_DOWN — and loadFailedInstanceIds is not touched.  No MMP_ROPF_*
 *     bit is valid; load_time / load_complete_time are not read.  The edit's flags: MMP_ROP_EDIT_REM_LOADED if the entry went,
 *     MMP_ROP_EDIT_TOUCHED if last_used rose; inserted_pos is -1.  refreshAfterUpdatedModelRecord and the KV-error branch
 *     (:3693-3709, whose failed placeholder entry is an op of mmp_cache_replay) stay with the caller.
 *
 * THE RULE BY KEY: model_idx_out[i] is what mmp_model_ids_resolve answers for key i.  Op i is evaluated exactly as
 * mmp_registry_ops evaluates it with `model` set to the row model_idx_out[i] names.  When the id is unknown OR that row is the
 * empty row — the all-zero row a deleted record leaves, the definition of MMP_RETIRE_EMPTY_ONLY and the rule of
 * mmp_models_status_k — the op is MMP_ROP_NO_RECORD (registry.get / getOrStrongIfAbsent == null, the Java returns, :2481,
 * :2945): it makes no edit, counts in n_no_record and in no per-kind total, and touches nothing.  Resolution, evaluation and
 * apply run under one hold of the batch lock.  By row an empty row is an ordinary record, as in mmp_registry_ops.
 *
 * MMP_EINVAL, with nothing written or changed: everything mmp_registry_ops refuses, with the kinds 0..4 valid (by key there is no
 * model range to refuse); a flag bit on a MMP_ROP_DROP_LOCAL op; key offsets that are not monotone; keys without key_off or
 * key_off without keys; two ops whose keys resolve to the same live row (two MMP_ROP_NO_RECORD ops under one unknown key are
 * not duplicates).  MMP_ESTATE before the first commit and, with keys, under the conditions of mmp_model_ids_resolve.  n == 0 is
 * valid; two runs over the same state with flags 0 are byte-identical. */
#define MMP_ROP_DROP_LOCAL 4 /* invokeModel's cache-hit loop: goLocal, getFromCache == null (MM.java:3682-3687) */
#define MMP_ROP_NO_RECORD 2  /* status byte: the key is unknown or names the empty row a deleted record leaves —
                                registry.get / getOrStrongIfAbsent == null, the Java returns (:2481, :2945) */
typedef struct {
    int32_t n_edits, n_unchanged, n_no_record, truncated; /* n_edits + n_unchanged + n_no_record == n */
    int32_t n_edited_op[8], n_unchanged_op[8];            /* per MMP_ROP_* kind, 5 used */
    int32_t n_entries_added, n_entries_removed;
} mmp_registry_ops_info_k; /* 88 bytes */
int mmp_registry_ops_k(mmp_ctx *ctx, const mmp_registry_op *ops, int32_t n, const char *keys, const int32_t *key_off,
                       int64_t now_ms, uint32_t flags, int32_t *model_idx_out, uint8_t *status_out,
                       mmp_registry_op_edit *edits_out, int32_t max_edits, mmp_registry_ops_info_k *info_out);

/* ---- the eviction loop by model id: onEviction's task body in one call (csrc/evictions_kernels.hpp) ---------------------------
 * What the task of ModelMesh.onEviction does per victim (MM.java:2886-2920): read this instance's loadedTime from the record
 * (instanceIds, else loadFailedInstanceIds), decide whether a reload elsewhere is to be attempted, and deregister — the read and
 * the edit under ONE hold of the batch lock, so that they are of one registry state, and without a ModelRecord on the host: a
 * host that parses no stored value has none to read loadedTime from.  With mmp_cache_replay_kt in front, the eviction loop is two
 * calls: the record's ids are `keys`, its times are `last_used`.
 *   entries            n victims: last_used (the record's time), load_time = ce.loadTimestamp, load_complete_time =
 *                      ce.loadCompleteTimestamp (primitives in the Java: MMP_ROPF_MATCH_TIME always holds), weight (carried for
 *                      the host's reload request; not read), flags = MMP_EVF_FAILED for ce.isFailed()
 *   keys / key_off     the victims' ids, under the conventions of mmp_model_ids_resolve
 *   params             self_pod (this instance), now, load_timeout_ms
 *   flags              MMP_ROPS_APPLY / MMP_ROPS_DRY / 0, as in mmp_registry_ops_k
 * Per victim, in this order:
 *   1. the id is resolved as mmp_registry_ops_k resolves it.  Unknown, or the empty row of a deleted record: status
 *      MMP_ROP_NO_RECORD, nothing read, nothing edited, no flag set, loaded_time -1.
 *   2. unless MMP_EVF_FAILED (:2887): loaded_time = the time self_pod has among the row's instanceIds; if it is not there, among
 *      its loadFailedInstanceIds (:2890-2893).  MMP_EVO_IN_REGISTRY if either list holds it (:2894); MMP_EVO_ATTEMPT_RELOAD if so
 *      and now - loaded_time > 2 * load_timeout_ms (:2895: strict, Java long arithmetic).
 *   3. MMP_EVO_RELOAD if MMP_EVO_ATTEMPT_RELOAD and, on the committed stats of the RECORD's type (typeSetStats, as mmp_gate_batch
 *      reads them): totalCapacity > 0, instanceCount > 1, (20 * totalFree) / totalCapacity >= 1 (:2918-2920) — the clause that
 *      sets MMP_GATE_RELOAD_ELSEWHERE, shared with it.
 *   4. MMP_EVO_LOG if in the registry or failed (:2900); millis_since_last_used = now - last_used (:2899, wrapping).
 *   5. the op {MMP_ROP_DEREGISTER, pod = self_pod, MMP_ROPF_MATCH_TIME, last_used, load_time, load_complete_time} (:2913), built on
 *      the device, evaluated and — with MMP_ROPS_APPLY — applied by the path of mmp_registry_ops_k.  Steps 2-3 read the row BEFORE
 *      this edit.
 * model_idx_out, status_out, edits_out, max_edits, truncation (nothing applied), NULLs: exactly as mmp_registry_ops_k; outs[i].status
 * repeats status_out[i].  info_out: the counts per flag and `ops`, what mmp_registry_ops_k reports of the n deregistrations.
 * MMP_EINVAL with nothing written or changed: what mmp_registry_ops_k refuses (self_pod outside the instance table, non-monotone
 * offsets, keys without key_off or the reverse, two victims whose ids name the same live row — the host splits the call), an entry
 * flag other than MMP_EVF_FAILED, now <= 0.  MMP_ESTATE as mmp_registry_ops_k, which is also what mmp_gate_batch answers without
 * a committed snapshot.  n == 0 is valid.
 * NOT here: ensureLoadedElsewhere itself (:2922) — a victim with MMP_EVO_RELOAD goes to the _ck seams with the caller excluded
 * and the record's last_used / weight; ce.doRemove (:2910); the metrics and log texts (:2902-2906: MMP_EVO_LOG and
 * millis_since_last_used are their inputs); the compare-and-set retry (:2958-2960: the edits go to mmp_models_rewrite_json as
 * ever). */
#define MMP_EVF_FAILED 1u          /* mmp_evicted_entry.flags: ce.isFailed() */
#define MMP_EVO_IN_REGISTRY 1u     /* mmp_evicted_out.flags */
#define MMP_EVO_ATTEMPT_RELOAD 2u
#define MMP_EVO_RELOAD 4u
#define MMP_EVO_LOG 8u
typedef struct {
    int64_t last_used;
    int64_t load_time;
    int64_t load_complete_time;
    int32_t weight;
    uint32_t flags;
} mmp_evicted_entry; /* 32 bytes */
typedef struct {
    int32_t self_pod;
    int32_t reserved;
    int64_t now;
    int64_t load_timeout_ms;
} mmp_evict_params; /* 24 bytes */
typedef struct {
    uint32_t flags;  /* MMP_EVO_* */
    int32_t status;  /* MMP_ROP_UNCHANGED / MMP_ROP_EDITED / MMP_ROP_NO_RECORD of the deregistration */
    int64_t loaded_time;             /* -1: none was read */
    int64_t millis_since_last_used;
} mmp_evicted_out; /* 24 bytes */
typedef struct {
    int32_t n_in_registry, n_attempt_reload, n_reload, n_log;
    int32_t n_no_record, reserved;
    mmp_registry_ops_info_k ops;
} mmp_evictions_info; /* 112 bytes */
int mmp_evictions_k(mmp_ctx *ctx, const mmp_evicted_entry *entries, int32_t n, const char *keys, const int32_t *key_off,
                    const mmp_evict_params *params, uint32_t flags, int32_t *model_idx_out, mmp_evicted_out *outs,
                    uint8_t *status_out, mmp_registry_op_edit *edits_out, int32_t max_edits, mmp_evictions_info *info_out);

/* getStatus (MM.java:3247) answered from the resident registry, a batch of questions at a time: the status class of
 * invokeModel's "getStatus case" (:3760-3768) and the copy list makeStatusInfo builds for the reply (:3013-3058).  Each answer
 * is a pure function of the record, so after an applied prune, janitor plan or mmp_registry_ops a host asks here instead of
 * reading the registry back.
 *
 * A request names a registry row (`model`; -1: no record, mr == null, :3257 — both lists empty) and optionally the instance
 * whose local load failed (`fail_pod` = the pod of mle.getInstanceId(); -1: no mle).  An all-zero row — what a deleted record
 * leaves behind — is an ordinary record without copies: the library cannot tell it from a live one, and a host that deletes
 * records sends -1 for them.
 *
 *   The failure overlay (:3017-3026).  fail_pod >= 0 and NOT among the record's loadFailedInstanceIds: it is put there with time
 *   now_ms, where mmp_registry_ops puts a new key — in front of the first RESOLVED entry (0 <= pod < pod count) with a greater
 *   id_order in the committed instance table, at the end if there is none; unresolved entries are never compared — and its
 *   entry in instanceIds, if any, is removed.  fail_pod already among the failed entries: nothing changes, and its loaded entry
 *   stays too (that is what the Java does).  The registry is not written.
 *
 *   The class, from the lists after the overlay: model -1: MMP_MST_NOT_FOUND; else loaded entries and no MMP_MSTF_MISS:
 *   MMP_MST_ASK; else fail_pod >= 0 or any failed entry: MMP_MST_LOADING_FAILED (:3764); else MMP_MST_NOT_LOADED.
 *
 *   The copies (:3029-3057): the loaded entries in list order as MMP_COPY_NOT_CHECKED, then the failed entries in list order as
 *   MMP_COPY_LOADING_FAILED, then Collections.sort with Long.compare(o.time, time): a STABLE sort by signed time, descending —
 *   equal times keep the concatenation order; times are arbitrary int64 values.  `pod` is reported as stored (an unresolved
 *   entry keeps its -1 or out-of-table value).  The MMP_COPY_LOADING_FAILED rows, read in output order, are also the order of
 *   the reply's message list (:3043-3045); the messages themselves (loadFailureInfos) stay with the caller, as in
 *   mmp_registry_ops.
 *
 * rows_out[i].copy_off is the exclusive prefix sum of the counts in request order; the copies of request i are
 * copies_out[copy_off, copy_off + n_not_checked + n_failed).  *n_copies_out is always the total.  copies_out == NULL with
 * max_copies == 0 returns the rows and the total only.  A positive max_copies below the total returns every copy whose global
 * index is below max_copies, the complete rows and the total, and still 0.  The answers are identical from run to run.
 *
 * Requests may repeat a model; n == 0 is valid.  Read-only: the call sees the registry between two writers, never inside one
 * (it takes it the way mmp_registry_census does) and does not hold decisions off.  MMP_EINVAL, with nothing written: a model
 * outside [-1, n_models), a fail_pod outside [-1, pod slots of the committed instance table), an unknown flag bit or a non-zero
 * `reserved`, now_ms <= 0 while a request carries a fail_pod, a NULL required buffer, more than INT32_MAX copies in all.
 * MMP_ESTATE when a request carries a fail_pod >= 0 before the first commit (the overlay needs id_order); without a fail_pod no
 * commit is needed. */
#define MMP_MST_NOT_FOUND 0      /* mr == null (:3257)                                             */
#define MMP_MST_NOT_LOADED 1     /* SI_NOT_LOADED (:3767)                                          */
#define MMP_MST_LOADING_FAILED 2 /* :3765 / :3981                                                  */
#define MMP_MST_ASK 3            /* the record has copies and the cache-hit loop has not been run: */
                                 /* the host asks a copy (mmp_serve_batch / mmp_route_batch); on   */
                                 /* LOADED / LOADING the list below is updateWithModelCopyInfo's   */
#define MMP_MSTF_MISS 1u         /* the cache-hit loop is exhausted: global cache miss, :3760      */
#define MMP_COPY_NOT_CHECKED 0
#define MMP_COPY_LOADING_FAILED 1
typedef struct { int32_t model; int32_t fail_pod; uint32_t flags; uint32_t reserved; } mmp_status_req;   /* 16 bytes */
typedef struct { int32_t cls; int32_t copy_off; int32_t n_not_checked; int32_t n_failed; } mmp_status_row; /* 16 bytes */
typedef struct { int32_t pod; int32_t status; int64_t time; } mmp_status_copy;                            /* 16 bytes */
int mmp_models_status(mmp_ctx *ctx, const mmp_status_req *reqs, int32_t n, int64_t now_ms, mmp_status_row *rows_out,
                      mmp_status_copy *copies_out, int32_t max_copies, int32_t *n_copies_out);
/* getStatus BY MODEL ID (MM.java:3247-3263): mmp_model_ids_resolve and mmp_models_status as ONE staged call under one hold of the
 * batch lock, so that no registry event batch and no mmp_models_retire can land between the row and its copy list
 * (csrc/status_keyed_kernels.hpp: one launch in front of the unchanged status kernels).
 *   keys / key_off     n keys, raw id bytes, under the conventions of mmp_model_ids_resolve
 *   fail_pod           int32[n], may be NULL (all -1)
 *   flags              uint32[n], may be NULL (all 0); the only bit is MMP_MSTF_MISS
 *   model_idx_out      n words, may be NULL
 *   rows_out, copies_out, max_copies, n_copies_out: exactly as mmp_models_status (sizes only with max_copies == 0, truncation)
 *
 * THE RULE BY KEY: model_idx_out[i] is what mmp_model_ids_resolve answers for key i.  Request i is answered exactly as
 * mmp_models_status answers {model = r, fail_pod[i], flags[i], 0}, where r is the row model_idx_out[i] names, and r = -1 when the
 * id is unknown OR that row is the empty row — the all-zero row a deleted record leaves, the definition of MMP_RETIRE_EMPTY_ONLY
 * and what mmp_vmodels_resolve treats as "not found" for a target: a deleted record's getStatus is SI_NOT_FOUND (:3257).  So a
 * host that keeps no id map does not have to "send -1" for deleted records; model_idx_out still carries the table's row, which
 * tells the two cases apart.
 *
 * MMP_EINVAL, with nothing written: key offsets that are not monotone, a NULL required buffer (NULL keys with key bytes present
 * included), a fail_pod outside [-1, pod slots of the committed instance table), an unknown flag bit, now_ms <= 0 while a
 * fail_pod is present, more than INT32_MAX copies in all.  MMP_ESTATE under the conditions of mmp_model_ids_resolve, and before
 * the first commit when a fail_pod >= 0 is present.  Read-only, locking as mmp_models_status; n == 0 is valid; two runs over the
 * same state are byte-identical. */
int mmp_models_status_k(mmp_ctx *ctx, const char *keys, const int32_t *key_off, int32_t n, const int32_t *fail_pod,
                        const uint32_t *flags, int64_t now_ms, int32_t *model_idx_out, mmp_status_row *rows_out,
                        mmp_status_copy *copies_out, int32_t max_copies, int32_t *n_copies_out);

/* a15: entries = usedSinceLastRun (runtimeCache.descendingMapWithCutoff(lastTime)) in iteration order.
 * overloaded_out has one byte per pod = membership in getExcludeSet() (MM.java:5835-5856); for
 * MMP_SCALE_UP rows the caller passes those pods as extra excludes of the load-target decisions
 * (the Java builds the set lazily, so it is only meaningful when some row is MMP_SCALE_UP).
 * *skipped = 1 when the task returns before looking at the entries (MM.java:5646, :5658). */
int mmp_scaleup_plan(mmp_ctx *ctx, const mmp_cache_entry *entries, int32_t n, const mmp_scaleup_params *params,
                     mmp_scaleup_out *outs, uint8_t *overloaded_out, int32_t *skipped);
/* a15 with limitModelConcurrency == true (MM.java:5677: latencyBased): conc[i] = the MaxConcCacheEntry state of entries[i].  Per
 * entry the threshold is mcce.getRpmScaleThreshold(true) (:5704, :2766-2796; params->scale_up_rpm_threshold is what that
 * returns for an entry without enough samples, :2781), heavyRpms three quarters of it, and maxConc adds to modelParallelismSum;
 * getExcludeSet() uses (int) (900.0 * averageModelParallelism) of the PREVIOUS run (:5836).  conc_outs[i] = the threshold and the
 * counter reset the call made; *result = the task's averageModelParallelism afterwards. */
int mmp_scaleup_plan_conc(mmp_ctx *ctx, const mmp_cache_entry *entries, const mmp_conc_entry *conc, int32_t n,
                          const mmp_scaleup_params *params, const mmp_conc_params *conc_params, mmp_scaleup_out *outs,
                          mmp_conc_out *conc_outs, uint8_t *overloaded_out, int32_t *skipped, mmp_conc_result *result);
/* a16: entries = scaleCopiesCandidates, oldest first; removed_out[i] = this copy is removed. */
int mmp_scaledown_plan(mmp_ctx *ctx, const mmp_cache_entry *entries, int32_t n,
                       const mmp_scaledown_params *params, uint8_t *removed_out);
/* a16 with MaxConcCacheEntry entries (MM.java:6294-6305): the threshold of a model with three or more copies is
 * mcce.getRpmScaleThreshold(false), and a copy with more than one queued request stays. */
int mmp_scaledown_plan_conc(mmp_ctx *ctx, const mmp_cache_entry *entries, const mmp_conc_entry *conc, int32_t n,
                            const mmp_scaledown_params *params, int64_t dynamic_rpm_scale_constant, uint8_t *removed_out);
/* a21: entries = runtimeCache.descendingLruMap() (MRU first). action_out[i] = 1:
 * triggerNewModelCopyElsewhere (MM.java:6913-6928) is issued with lastUsedTime = entry.last_used
 * and excludes = current holders ∪ self; wait_out[i] = 1: shutdown waits for it (CUTOFF_AGE_MS). */
int mmp_migration_plan(mmp_ctx *ctx, const mmp_cache_entry *entries, int32_t n, int32_t self_pod, int64_t now_ms,
                       int64_t cutoff_age_ms, uint8_t *action_out, uint8_t *wait_out);

/* THE PERIODIC TASKS BY MODEL ID.  The rate task (MM.java:5672-5690), the janitor's cache loop (:5896-5903) and preShutdown's
 * migration (:6998-7010) iterate runtimeCache, whose keys are model ids, and begin each entry with registry.get(modelId): an
 * instance holds ids, never registry rows.  Each call below keeps the argument list of its by-row call and adds
 *   keys / key_off     n keys, raw id bytes, n + 1 offsets that need not start at 0 (the conventions of mmp_model_ids_resolve)
 *   model_idx_out      n words, may be NULL: what mmp_model_ids_resolve answers for key i
 * and resolves the keys on the device under THE SAME hold of the batch lock that evaluates (and, for the janitor, applies): no
 * registry event batch that deletes and re-registers an id, and no mmp_models_retire, can move a row between its resolution and
 * its use (csrc/tasks_keyed_kernels.hpp: one launch in front of the unchanged plan kernels).
 *
 * THE RULE BY KEY: entry i is evaluated exactly as the by-row call evaluates it with `model` set to the row model_idx_out[i]
 * names, and to -1 — "registry.get(modelId) == null", what every one of these structs already says -1 means — when the id is
 * unknown OR that row is the empty row a deleted record leaves (the definition of MMP_RETIRE_EMPTY_ONLY, the rule of
 * mmp_models_status_k and mmp_registry_ops_k).  The `model` field the caller sent is never read.  With keys == key_off == NULL
 * each call IS its by-row call (model_idx_out then repeats the entries' `model`); one of the two NULL is MMP_EINVAL.  Key offsets
 * that are not monotone are MMP_EINVAL; MMP_ESTATE before the first commit and, with keys, under the conditions of
 * mmp_model_ids_resolve; a refused call writes nothing.  n == 0 is valid; two runs over one state are byte-identical.
 *
 * mmp_scaleup_plan_k: mmp_scaleup_plan when conc_params is NULL (conc, conc_outs and result are then NULL too:
 * limitModelConcurrency == false), mmp_scaleup_plan_conc otherwise.  A run that is skipped (*skipped = 1) still answers
 * model_idx_out.  mmp_scaledown_plan_k: mmp_scaledown_plan when conc is NULL, mmp_scaledown_plan_conc otherwise. */
int mmp_scaleup_plan_k(mmp_ctx *ctx, const mmp_cache_entry *entries, const mmp_conc_entry *conc, int32_t n, const char *keys,
                       const int32_t *key_off, const mmp_scaleup_params *params, const mmp_conc_params *conc_params,
                       mmp_scaleup_out *outs, mmp_conc_out *conc_outs, uint8_t *overloaded_out, int32_t *skipped,
                       mmp_conc_result *result, int32_t *model_idx_out);
int mmp_scaledown_plan_k(mmp_ctx *ctx, const mmp_cache_entry *entries, const mmp_conc_entry *conc, int32_t n, const char *keys,
                         const int32_t *key_off, const mmp_scaledown_params *params, int64_t dynamic_rpm_scale_constant,
                         uint8_t *removed_out, int32_t *model_idx_out);
int mmp_migration_plan_k(mmp_ctx *ctx, const mmp_cache_entry *entries, int32_t n, const char *keys, const int32_t *key_off,
                         int32_t self_pod, int64_t now_ms, int64_t cutoff_age_ms, uint8_t *action_out, uint8_t *wait_out,
                         int32_t *model_idx_out);
/* janitorTask (MM.java:5876-6145) as ONE call: mmp_janitor_plan by model id, and — with `scaledown` — the scale-down of the
 * candidates it found (:6110-6145, removeModelCopies :6197-6310) in the same hold, where today the candidates travel to the host
 * as rows and come back into mmp_scaledown_plan in another call.
 *
 * NO MODEL HAS TWO ROWS is settled on the device by key: two entries whose keys resolve to the same live row are MMP_EINVAL, with
 * nothing written, nothing applied and the library's scratch as it was (a by-row call that follows is not disturbed).  Two equal
 * keys that resolve to NO record both become -1 and are NOT detected — the by-row call accepts several -1 rows as well, and each
 * is removed by the cache loop on its own (:5968).  A run that is shutting down (:5880) still resolves and still refuses.
 *
 * THE SCALE-DOWN IN THE SAME CALL (scaledown != NULL; also by row).  The answer is DEFINED as that of mmp_janitor_plan with
 * MMP_JANITOR_APPLY followed by mmp_scaledown_plan (conc == NULL) / mmp_scaledown_plan_conc on the candidates it returned:
 *   scaledown                    the scale-down's parameters; scaledown->self_pod must equal params->self_pod
 *   conc                         n MaxConcCacheEntry rows in INPUT-row order (conc[r] belongs to entries[r]; the candidate that came
 *                                from input row candidate_rows_out[j] is decided on conc[candidate_rows_out[j]]); NULL: not
 *                                latency-based, dynamic_rpm_scale_constant is then not read
 *   removed_out                  one byte per candidate, aligned with candidates_out: n_candidates bytes are written
 * The scale-down reads the registry as the two loops left it, so it needs MMP_JANITOR_APPLY (MMP_EINVAL otherwise).  On a
 * truncated plan nothing is applied, as in mmp_janitor_plan, and removed_out is not written.  A run that stopped at a repaired row
 * (stopped_at >= 0) or that is shutting down has no candidates: nothing is decided.  conc without scaledown is MMP_EINVAL. */
int mmp_janitor_plan_k(mmp_ctx *ctx, const mmp_janitor_entry *entries, int32_t n, const char *keys, const int32_t *key_off,
                       const mmp_janitor_params *params, uint32_t flags, const mmp_scaledown_params *scaledown,
                       const mmp_conc_entry *conc, int64_t dynamic_rpm_scale_constant, int32_t *model_idx_out, uint8_t *actions_out,
                       mmp_janitor_edit *edits_out, int32_t max_edits, mmp_cache_entry *candidates_out,
                       int32_t *candidate_rows_out, int32_t max_candidates, uint8_t *removed_out, mmp_janitor_info *info_out);

/* ---- ingestion of the KV-store wire format ---------------------------------------
 * The instance table and the registry live in etcd / ZooKeeper as Jackson JSON values
 * (MM.java:346 INST_REC_SERIALIZER, :628 registry view; InstanceRecord.java:37-69,
 * ModelRecord.java:61-114).  These entry points take the raw values and parse them on the device. */
/* Define the pod index space from the instance ids (the KV keys): computes id_order (rank under
 * String.compareTo; ids must be ASCII) and replica_set (interned id.substring(0,6), -1 if |id| < 7,
 * MM.java:4769) for every pod, and the id -> pod table used to resolve ModelRecord.instanceIds keys.
 * Rows not yet ingested are absent (tombstones).  Optional outputs may be NULL. */
int mmp_pod_ids_load(mmp_ctx *ctx, const char *ids, const int32_t *id_off, int32_t n_pods, uint32_t *id_order_out,
                     int32_t *replica_set_out);
/* n InstanceRecord JSON values, value i = buf[off[i], off[i+1]) for pod pod_idx[i]; live[i] != 0 marks
 * the instance as present in the litelinks registry (MM.java:4765).  Equivalent to mmp_pods_upsert with
 * rows parsed from the JSON.  status_out[i] = 1 for a malformed value (that row is left unchanged);
 * start_time_out[i] = InstanceRecord.startTime (input of mmp_upgrade_instance_added). */
int mmp_pods_ingest_json(mmp_ctx *ctx, const char *buf, const int64_t *off, int32_t n, const int32_t *pod_idx,
                         const uint8_t *live, int64_t *start_time_out, int32_t *status_out);
/* Names of the model types in type-table order (ModelRecord "type"); a name not listed maps to
 * unknown_type (the extra row mmp_types_from_labels installs), an absent / null type to the index of
 * "NLCLASSIFIER" (ModelRecord.DEFAULT_TYPE, ModelRecord.java:121-133) if listed, else unknown_type. */
int mmp_type_names_load(mmp_ctx *ctx, const char *names, const int32_t *name_off, int32_t n_types, int32_t unknown_type);
/* Replace the registry view (like mmp_models_load) from n_models ModelRecord JSON values; model i =
 * value i.  Ids that are not in the pod table become entries with pod -1 (they still count as copies).
 * last_unload_out[i] = "lul" (ModelRecord.lastUnloadTime, an input of the scale-down plan). */
int mmp_models_ingest_json(mmp_ctx *ctx, const char *buf, const int64_t *off, int32_t n_models, int64_t *last_unload_out,
                           int32_t *status_out);
/* Registry events as stored (the registry's KV listener, MM.java:628, event() :2807-2854, delivers one whole ModelRecord value per
 * change): mmp_models_upsert with the rows parsed on the device.  Event i is the value buf[off[i], off[i+1]) for registry row
 * model_idx[i]; indices follow mmp_models_upsert (model_idx[i] == the running model count appends, in event order).
 * deleted[i] != 0 is ENTRY_DELETED: the value is ignored (it may be empty) and the row becomes the empty row — all fields zero, no
 * entries — which is what mmp_models_upsert documents for a deleted record; deleted may be NULL (no event is a deletion).
 * Grammar, field set, type-name resolution, default type and id resolution are those of mmp_models_ingest_json: an id that is not
 * in the pod table gives an entry with pod -1, entries stay in document order, mmp_pod_ids_load is required first (MMP_ESTATE
 * without it), the type table is optional.  status_out[i] = 1 for a malformed value.  Events apply in order and a malformed event
 * changes nothing, so a row ends as its LAST WELL-FORMED OR DELETED event left it: an existing row whose events in this call are
 * all malformed is untouched; an appended row whose events are all malformed becomes the empty row (its index has been handed
 * out).  last_unload_out[i] = the event's "lul", 0 for a deleted or malformed event; it may be NULL.  Takes effect at once, no
 * commit; locking as in mmp_models_upsert (decisions are held off only while the rows are rewritten in place).  n == 0 is valid.
 * MMP_EINVAL, with nothing changed: a NULL required buffer, non-monotone offsets, an index < 0 or beyond the running count, entry
 * arena overflow.  O(events + their bytes + their entries), whatever the size of the registry: the values are parsed and the
 * winning events' entries appended to the arena on the device; only the per-event status, lul and entry counts come back. */
int mmp_models_upsert_json(mmp_ctx *ctx, const char *buf, const int64_t *off, int32_t n, const int32_t *model_idx,
                           const uint8_t *deleted, int64_t *last_unload_out, int32_t *status_out);
/* New instances join the index space: the n_new ids get the pod indices P .. P + n_new - 1 (P = the pod count at the call), their
 * rows are appended as tombstones — what mmp_pod_ids_load leaves for a row it has not seen ingested — and the id -> pod table
 * learns them.  id_order is recomputed for all P + n_new ids (rank under String.compareTo, as the load); replica_set of the new
 * ids continues the load's interning: a six-character prefix seen before keeps its number, a new one gets the next, |id| < 7
 * gives -1.  Both outputs are optional and cover ALL P + n_new pods; with either, max_pods >= P + n_new is required.
 * Unlike a second mmp_pod_ids_load the call keeps the `missings` marks of mmp_registry_prune (the map grows by zero marks for
 * the new slots), re-sorts only the new ids, extends the device table on the device (copy-on-write: a copy, or a rehash of the
 * stored hashes when it outgrows its capacity, then an atomic insert per new id and a verifying lookup; swapped in on success)
 * and does not quiesce decisions: nothing a decision kernel reads is rewritten.  (The call holds the state lock like the load, so
 * a decision issued meanwhile waits for it to return.)  The next mmp_snapshot_commit RANKS FROM SCRATCH, as after mmp_pod_ids_load: a join moves
 * the id_order of other rows, so it is not eligible for the insertion commit.  To the type tables the appended pods are what
 * pods appended through mmp_pods_upsert are.  Records that named one of the ids before it joined: mmp_registry_unresolved.
 * MMP_EINVAL with NOTHING changed (table, rows, marks, ids): a NULL required buffer, non-monotone offsets, an id equal to an
 * existing id or to another new one or colliding with one under FNV-1a (the rule of the load), an output with max_pods too
 * small.  MMP_ESTATE before the first mmp_pod_ids_load (a load of 0 ids is a valid start) and when mmp_pods_load /
 * mmp_pods_upsert have resized the table since.  n_new == 0 is valid and changes nothing. */
int mmp_pod_ids_append(mmp_ctx *ctx, const char *ids, const int32_t *id_off, int32_t n_new, uint32_t *id_order_out,
                       int32_t *replica_set_out, int32_t max_pods);
/* Instance-table events as stored (handleInstanceTableChange, MM.java:1455): event i is the instance id
 * keys[key_off[i], key_off[i+1]) — the raw ASCII bytes of the KV key, not JSON-escaped — with the InstanceRecord value
 * buf[off[i], off[i+1]).  The keys are resolved against the id table on the device.  deleted[i] != 0: the effect of
 * mmp_pods_remove on that pod; the value is ignored and may be empty.  Otherwise the value goes through the parser of
 * mmp_pods_ingest_json (live as there).  status_out[i]: 0 applied, 1 malformed value (the row is left as it was), 2 unknown id
 * (nothing changes; pod_idx_out[i] = -1).  An id the table does not know: with MMP_PEV_APPEND in flags the distinct unknown ids
 * of NON-DELETED events join through mmp_pod_ids_append, in order of first appearance, whether or not their values turn out
 * well-formed (the index has been handed out, the row stays a tombstone: the rule of mmp_models_upsert_json for appended rows);
 * without the flag such an event is status 2.  A deletion never appends: of an id that is unknown when the event is reached —
 * the table and the events before it — it is status 2.  Events apply in order: a pod ends as its LAST WELL-FORMED OR DELETED event
 * left it.  pod_idx_out[i] = the resolved index (mmp_upgrade_instance_added and the serve counters need it);
 * start_time_out[i] = InstanceRecord.startTime of an applied value, else 0; *n_appended_out = ids that joined.  deleted, live,
 * start_time_out, n_appended_out may be NULL.  After a join the next commit ranks from scratch (mmp_pod_ids_append).
 * MMP_EINVAL with nothing changed: a NULL required buffer, non-monotone offsets of either kind, unknown flags, two new ids that
 * collide under FNV-1a.  MMP_ESTATE, with nothing changed: before mmp_pod_ids_load, and when mmp_pods_load / mmp_pods_upsert
 * have resized the instance table since (its rows and the ids no longer cover the same indices; checked for every call, with or
 * without a join).  Locking as mmp_pod_ids_append.  n == 0 is valid. */
#define MMP_PEV_APPEND 1u
int mmp_pods_events_json(mmp_ctx *ctx, const char *keys, const int32_t *key_off, const char *buf, const int64_t *off, int32_t n,
                         const uint8_t *deleted, const uint8_t *live, uint32_t flags, int32_t *pod_idx_out, int64_t *start_time_out,
                         int32_t *status_out, int32_t *n_appended_out);
/* ---- instance labels from the stored value ---------------------------------------------------------------------------------
 * InstanceRecord.labels (InstanceRecord.java:68-92: a String[]; null, absent and an empty array are all NO_LABELS) kept inside the
 * context, one label word and one element count per staged instance, as long as the staged instance table.  Only the labels some
 * type names can matter (TypeConstraintManager.java:478-486, instanceMatches), so the host loads those names once and hands every
 * instance event over as stored.
 *
 * mmp_label_names_load: label name i = names[name_off[i], name_off[i+1]) owns bit i of a label word; 0 <= n_labels <= 64 (one
 * uint64 per instance, the width mmp_types_from_labels fixes).  Names match by bytes against the RAW bytes between the quotes of an
 * element; an empty name and non-ASCII UTF-8 names are allowed.  A successful load clears every resident label word and count (the
 * bits change meaning); n_labels == 0 unloads the table (names / name_off may then be NULL).  MMP_EINVAL with nothing changed:
 * more than 64 names, two equal names, non-monotone offsets, a name holding '"', '\' or a byte below 0x20 (none can stand raw
 * inside a JSON string, and Jackson writes no escapes for any other character).
 *
 * While a table is loaded, mmp_pods_ingest_json and mmp_pods_events_json read `labels` as a known field of type "null or array
 * of strings" with a second kernel over the staged values (mmp_last_kernel_ms covers it); without one they behave and launch
 * exactly as before.  Every occurrence is held to its type — a number, a string, an object, true, an element that is not a
 * string, a leading / doubled / trailing comma, two strings without a comma, an unterminated array: status 1, neither the row nor
 * the labels change — and the LAST occurrence decides the set.  Every applied non-deleted event sets word and count of its pod
 * (0 / 0 when the field is absent, null or []); a deleted event leaves them.  An element whose raw bytes hold a backslash matches
 * no name and counts as an unknown label; a repeated label sets its bit once and counts twice.  Unspecified: a raw control byte
 * inside a label string.
 *
 * State: mmp_pod_ids_append and a join inside mmp_pods_events_json add zero words; mmp_pods_load keeps the words of the indices
 * that remain and zeroes new ones; mmp_pod_ids_load clears all (a new index space, as for the `missings` marks); mmp_pods_upsert
 * and mmp_pods_remove leave them alone (an appended row starts with none). */
int mmp_label_names_load(mmp_ctx *ctx, const char *names, const int32_t *name_off, int32_t n_labels);
/* For hosts that feed rows (mmp_pods_upsert) instead of JSON: word and count of the staged pods idx[0..n), all of the call or
 * none of it on an index outside the staged table (MMP_EINVAL; also a negative count, a NULL buffer).  Needs no name table. */
int mmp_pod_labels_set(mmp_ctx *ctx, const int32_t *idx, const uint64_t *words, const int32_t *counts, int32_t n);
/* words_out[p] = the known-label bits of pod p, counts_out[p] = the number of elements of its `labels` array, unknown and
 * repeated ones included: 0 means NO_LABELS, which is what a host passes as labels_key == 0 (mmp_upgrade_instance_added).
 * *n_out = the staged pod count, always; at most max_pods entries are written.  Either output may be NULL. */
int mmp_pod_labels_get(mmp_ctx *ctx, uint64_t *words_out, int32_t *counts_out, int32_t max_pods, int32_t *n_out);
/* mmp_types_from_labels with the resident label words in place of pod_labels: from raw instance events to the type sets of the
 * next commit without the host decoding a record.  required[t] / preferred[t] are bitsets over the loaded name order. */
int mmp_types_from_pod_labels(mmp_ctx *ctx, int32_t n_types, const uint64_t *required, const uint64_t *preferred,
                              uint64_t *allowed_out, uint64_t *prefer_out, uint8_t *has_allowed_out, uint8_t *has_prefer_out);
/* Which records name an id the table does not know: the registry rows that hold at least one entry (loaded or failed) whose pod
 * is outside [0, pod slots of the staged table), in ascending row order.  *n_models_out / *n_entries_out are always the full
 * counts (*n_entries_out = mmp_registry_stats.n_entries_unresolved); at most max_models rows are written, lowest rows first;
 * model_out == NULL with max_models == 0 asks for the sizes only.  Read-only, locking as mmp_registry_census, no commit needed;
 * two runs over the same registry are byte-identical.
 * The intended loop: (1) an instance joins (mmp_pod_ids_append / mmp_pods_events_json); (2) the host asks here; (3) it sends
 * the stored values of those records through mmp_models_upsert_json again — the registry listener has them.  The library cannot
 * do step 3 by itself: the registry keeps neither the bytes nor the hash of an id it could not resolve, only pod -1.  Until
 * then such an entry still counts as a copy but excludes nobody in a decision. */
int mmp_registry_unresolved(mmp_ctx *ctx, int32_t *model_out, int32_t max_models, int32_t *n_models_out, int64_t *n_entries_out);
/* ---- registry events by key: the model-id table (model_ids_kernels.hpp) --------------------------------------------------------
 * The registry's rows are numbered; its listener (MM.java:628, event() :2807-2854) gets a key and a value.  The context keeps the
 * id -> row map on the device — open addressing like the instance table's, but a model id is an arbitrary user string (raw key
 * bytes, any UTF-8, no ASCII rule: nothing orders them), so a slot is matched on its 64-bit FNV-1a hash AND its bytes, which the
 * context keeps in a device arena.  Ids that collide coexist; nothing is refused for colliding.  A slot is never deleted in
 * place: ids leave only through mmp_models_retire, which builds the next table without them.
 * MMP_MODEL_ID_HASH_BITS=b (read with the other MMP_* switches, per context at mmp_create) masks every model-id hash to its low b
 * bits, 0: all equal — a diagnostic that makes the collision path testable. */
/* Name the registry's rows 0 .. n_models-1: id i = ids[id_off[i], id_off[i+1]).  The table is built on the device and replaces
 * the loaded one.  MMP_ESTATE unless n_models equals the registry's row count (load the registry first; 0 ids over an empty
 * registry is a valid start, every id then joins through mmp_models_events_json).  MMP_EINVAL with nothing changed: a NULL
 * required buffer, non-monotone offsets, two equal ids. */
int mmp_model_ids_load(mmp_ctx *ctx, const char *ids, const int32_t *id_off, int32_t n_models);
/* model_idx_out[i] = the registry row of key i = keys[key_off[i], key_off[i+1]), -1 for an id the table does not know.
 * Read-only: this is how a host that keeps the row map itself (and renumbers it after mmp_models_retire) learns a row.  A host
 * without a map does not resolve and then call — a retirement could land between the two: it asks by id in one call
 * (mmp_models_status_k, mmp_registry_ops_k, the _ck / _cv request seams).  MMP_ESTATE before
 * mmp_model_ids_load and when the registry has been resized by index since (see mmp_models_events_json).  n == 0 is valid. */
int mmp_model_ids_resolve(mmp_ctx *ctx, const char *keys, const int32_t *key_off, int32_t n, int32_t *model_idx_out);
/* The way back: the ids of rows [first_row, first_row + n_rows) — the prune, janitor, unresolved and status calls answer in rows.
 * *n_bytes_out = their bytes, always; off_out (n_rows + 1 words, rebased to 0) is written when it is not NULL; the bytes are
 * written when max_bytes >= *n_bytes_out.  bytes_out == NULL with max_bytes == 0 asks for the sizes only.  MMP_EINVAL for a range
 * outside the table; MMP_ESTATE as mmp_model_ids_resolve. */
int mmp_model_ids_get(mmp_ctx *ctx, int32_t first_row, int32_t n_rows, char *bytes_out, int32_t max_bytes, int32_t *off_out,
                      int32_t *n_bytes_out);
/* Registry events as the listener gets them: event i is the model id keys[key_off[i], key_off[i+1]) — the raw bytes of the KV
 * key — with the ModelRecord value buf[off[i], off[i+1]).  The keys are resolved, deduplicated and numbered on the device;
 * everything behind the resolution is mmp_models_upsert_json (same parser, same winner rule, same arena append — both calls run
 * one pipeline).  deleted[i] != 0 is ENTRY_DELETED: the value is ignored and the row becomes the empty row; it KEEPS its id and
 * its number, and an id that is registered again gets its old row back — until the host hands the row back through
 * mmp_models_retire, after which the id is unknown again.
 * status_out[i]: 0 applied, 1 malformed value, 2 unknown id (nothing changes; model_idx_out[i] = -1).  An id the table does not
 * know: with MMP_MEV_APPEND in flags the distinct unknown ids of NON-DELETED events join as rows M0, M0+1, ... (M0 = the row count
 * at the call) in order of first appearance, whether or not their values turn out well-formed (the appended-row rule of
 * mmp_models_upsert_json: a joined row whose events are all malformed is the empty row); without the flag such an event is
 * status 2.  A deletion never appends: of an id that is unknown when the event is reached — the table and the events before
 * it — it is status 2; behind the event that made the id join, it applies.  Events apply in order: a row ends as its LAST
 * WELL-FORMED OR DELETED event left it.  model_idx_out[i] = the resolved row; last_unload_out[i] = "lul" of an applied value,
 * else 0; *n_appended_out = ids that joined.  deleted, last_unload_out, n_appended_out may be NULL.
 * Only O(events) words come back to the host; two runs over the same state and events are byte-identical, whichever lanes raced.
 * MMP_EINVAL with nothing changed (table, id arena, registry): a NULL required buffer, non-monotone offsets of either kind,
 * unknown flags, entry arena overflow.  MMP_ESTATE with nothing changed: before mmp_model_ids_load or mmp_pod_ids_load, and when
 * the registry's row count no longer equals the id count — mmp_models_load, mmp_models_ingest_json or an append by index
 * (mmp_models_upsert / mmp_models_upsert_json) resized one space without the other; load the ids again.  Locking as
 * mmp_models_upsert_json.  n == 0 is valid. */
#define MMP_MEV_APPEND 1u
int mmp_models_events_json(mmp_ctx *ctx, const char *keys, const int32_t *key_off, const char *buf, const int64_t *off, int32_t n,
                           const uint8_t *deleted, uint32_t flags, int32_t *model_idx_out, int64_t *last_unload_out,
                           int32_t *status_out, int32_t *n_appended_out);
/* Retire registry rows: the named rows leave the index space, and the registry, its entry arena, the id arena and the model-id
 * table are compacted on the device (retire_kernels.hpp).  rows[0 .. n) are registry rows in [0, M0), M0 = the row count at the
 * call, in any order; a row named twice is retired once.  The survivors keep their relative order and move down: a survivor's
 * new row is its old row minus the number of retired rows below it.  remap_out (may be NULL; else max_models >= M0 words):
 * remap_out[old] = the new row, -1 for a retired one, for all M0 old rows.  *n_models_after_out (may be NULL) = the new count.
 * Registry: the survivors' records are unchanged — type, last_used, the loaded and failed entries in their order; the retired
 * rows' entries are dropped, and the call leaves the entry arena squeezed (ent_off = the exclusive prefix of the survivors'
 * counts, no garbage).  Model-id table, when one is loaded: the retired ids leave the table and the arena,
 * mmp_model_ids_resolve of a retired id gives -1, mmp_model_ids_get returns the survivors' ids under their new rows, the table
 * has the capacity of a fresh load of the survivors (no id is hashed again: MMP_MODEL_ID_HASH_BITS still holds), and a retired
 * id that arrives again through mmp_models_events_json with MMP_MEV_APPEND joins as a new row at the end, like any unknown id.
 * Both spaces shrink together, so the by-key calls go on without a reload.  Without an id table only the registry is compacted.
 * MMP_RETIRE_EMPTY_ONLY guards the intended loop — (1) deletion events arrive, (2) the host collects their model_idx, (3) it
 * retires them later: every named row must then be the empty row (all fields zero, no entries: what a deletion leaves), checked
 * on the device rows; if one is not — its id was registered again in between, with or without copies — the call is MMP_EINVAL
 * with nothing changed and mmp_last_error names the lowest such row.
 * Decisions: the compacted tables are built beside the published ones; the pointers and counts are swapped under the state lock
 * once the decisions in flight have drained, and the resolved view is rebuilt as in mmp_models_load — a decision sees the whole
 * old registry or the whole new one, and decisions after the call are right without a commit.  Row numbers the HOST holds —
 * request rows in flight, the keys of UNBOUND keyed caches (mmp_caches_load_keyed), its own maps — are the host's to renumber from
 * remap_out.  BOUND caches (mmp_caches_load_keyed_k) are carried along: a named row that is the key of a LIVE entry of any cache
 * (a position below the cache's entry count; the slots behind it are not looked at) makes the call MMP_EINVAL with nothing
 * changed — registry, id table and caches — and mmp_last_error names the lowest such row, checked on the device in front of the
 * swap like MMP_RETIRE_EMPTY_ONLY (the cache's counterpart of MMP_PODS_RETIRE_UNREFERENCED; the intended loop: deletion event,
 * the janitor's MMP_COP_REMOVE, then retire); once nothing can fail any more every live key >= 0 becomes remap[key] on the
 * device, and MMP_UNLOADBUF_KEY stays as it is.  Without bound caches the call is what it always was.
 * MMP_EINVAL with nothing changed: NULL rows with n > 0, a row outside [0, M0), an unknown flag bit, remap_out with
 * max_models < M0, a non-empty row under MMP_RETIRE_EMPTY_ONLY, a row that is a live key of a bound cache.  MMP_ESTATE with nothing changed: an id table is loaded and its
 * row count no longer equals the registry's (as mmp_model_ids_resolve).  n == 0 is valid and changes nothing: remap_out is the
 * identity, *n_models_after_out = M0.  No commit is needed before or after.  The work is O(registry), as a reload is — the host
 * decides how often to call; two runs over the same state and list are byte-identical.  Locking: batch_mu throughout. */
#define MMP_RETIRE_EMPTY_ONLY 1u
int mmp_models_retire(mmp_ctx *ctx, const int32_t *rows, int32_t n, uint32_t flags, int32_t *remap_out, int32_t max_models,
                      int32_t *n_models_after_out);
/* Retire instance rows: the named instances leave the index space, the other index space of the wire-format path and the one
 * that churns (every rolling update replaces every instance by one with a new id, and a tombstone keeps its index).  pods[0 .. n)
 * are staged instance indices in [0, P0), P0 = the staged count at the call, in any order; an index named twice is retired once.
 * The survivors keep their relative order and move down: a survivor's new index is its old index minus the number of retired
 * indices below it.  remap_out (may be NULL; else max_pods >= P0 words): remap_out[old] = the new index, -1 for a retired one,
 * for all P0 old indices.  *n_pods_after_out (may be NULL) = the new count P1.  *n_entries_unresolved_out (may be NULL) = the
 * registry entries the call turned into pod -1.
 * Staged table, label words and counts: compacted.  With an id table loaded the survivors' id_order becomes their rank among the
 * surviving ids — what a fresh mmp_pod_ids_load of the survivors gives; replica_set numbers and the interning are NOT renumbered
 * (mmp_replaced_rs_load and the upgrade tracker hold them, and an id prefix seen before keeps its number when it comes back).
 * Without an id table the rows keep the id_order the host supplied.  Instance-id table and id store: the retired ids leave both;
 * the table gets the capacity of a fresh load of the survivors, built from the stored hashes (no id is hashed again) and verified
 * in a launch of its own.  A retired id is unknown afterwards: mmp_pods_events_json answers status 2 for it, and with
 * MMP_PEV_APPEND it joins as a new index at the end.  Type table: the retired instances' bits are squeezed out of the allowed /
 * prefer rows, whichever call loaded them — no reload is needed.  `missings` marks: the survivors' marks move with them;
 * mmp_registry_missing_get returns the old map read through remap.  Registry: rows, times and offsets are untouched and the entry
 * arena is NOT squeezed; an entry naming a survivor gets its new index, an entry naming a retired instance becomes -1 (it still
 * counts as a copy and excludes nobody: mmp_registry_unresolved), an entry outside [0, P0) is copied as it is.
 * MMP_PODS_RETIRE_GONE_ONLY: every named row must be a tombstone in the staged table (MMP_POD_TOMBSTONE set, MMP_POD_LIVE clear) —
 * the guard against an id that came back between its deletion and the retire; otherwise MMP_EINVAL, mmp_last_error names the
 * lowest such index.  MMP_PODS_RETIRE_UNREFERENCED: no entry a registry row references, loaded or failed, may name a retired
 * instance (checked on the device registry; the arena's garbage is not looked at); otherwise MMP_EINVAL naming the lowest such
 * instance.  The intended loop: a deletion event tombstones the row, mmp_registry_prune removes its registrations after
 * gone_after_ms, then both guards hold and the index is handed back.
 * Decisions: this call changes what the published snapshot is indexed by, so it ENDS IN A COMMIT.  Everything above is built
 * beside the published state; then the state lock is taken exclusively, the decisions in flight drain, the inputs are swapped and
 * the stages of mmp_snapshot_commit run from scratch and publish — with the state lock held, which is accepted for this call:
 * decisions issued meanwhile wait, a decision sees the whole old index space or the whole new one, and every answer after the
 * call is in the new numbering.  If the commit stage fails (MMP_EORDER when the staged table carries other edits) the old inputs
 * are put back and nothing has changed.  A context without a published snapshot only has its inputs compacted.
 * Everything numbered by instance that the HOST holds — request rows, exclusion lists, serve counters, self_pod, fail_pod — is
 * the host's to renumber from remap_out.  Cache numbers (mmp_caches_load*) are the host's own index space and are not touched.
 * MMP_EINVAL with nothing changed (rows, ids, table, labels, types, marks, registry, snapshot): NULL pods with n > 0, an index
 * outside [0, P0), an unknown flag bit, remap_out with max_pods < P0, either guard.  MMP_ESTATE with nothing changed: an id table
 * is loaded and no longer covers the staged rows (the rule of mmp_pod_ids_append); a type table is loaded whose word count is not
 * that of the P0 staged rows (the table a commit refuses: it could not be squeezed, and must not pass the commit's check once the
 * count crosses the word edge back — reload the types first); the context is a pod-axis shard (out of scope: reload the shards).  n == 0 is valid and changes nothing: remap_out is the identity and no commit is run.  The work is
 * O(P0 + table slots + entry arena + registry rows) plus the commit; two runs over the same state and list are byte-identical.
 * Locking: batch_mu throughout, the state lock from the swap to the publication. */
#define MMP_PODS_RETIRE_GONE_ONLY 1u
#define MMP_PODS_RETIRE_UNREFERENCED 2u
int mmp_pods_retire(mmp_ctx *ctx, const int32_t *pods, int32_t n, uint32_t flags, int32_t *remap_out, int32_t max_pods,
                    int32_t *n_pods_after_out, int64_t *n_entries_unresolved_out);
/* ---- the write side of the wire format (rewrite_kernels.hpp) ---------------------------------------------------------------------
 * Every edit of the registry ends, in the reference, in a compare-and-set that writes a WHOLE serialised ModelRecord back to the
 * KV store (ModelMesh.java: 13 conditionalSet / conditionalSetAndGet sites, 12 of them on the registry).  The library answers an edit with edit rows
 * (mmp_registry_op_edit, mmp_prune_edit, mmp_janitor_edit); this call turns the stored value of a record, plus the record as the
 * device now holds it, into the value to store next — so that the host decodes no ModelRecord on the way out either.  The device
 * does not hold type, mPath, encKey, refs, autoDel, the failure texts or any future field: those pass through BYTE FOR BYTE from
 * the old value.  It renders what the mesh owns, from the resident row: instanceIds, failedIn, lu, optionally lul, and the key set
 * of fails.
 *
 * Value i: the old value old_buf[old_off[i], old_off[i+1]) of registry row rows[i]; a row may appear more than once.  With the
 * OWNED names instanceIds, failedIn, fails, lu — and lul when last_unload != NULL — the new value is
 *     { kept members , owned members }
 * joined by single commas with no other whitespace.
 * Kept members: every top-level member of the old value whose name is not an owned name, in document order, every occurrence of
 * a duplicate included, each copied verbatim from the opening quote of its key to the last byte of its value (whitespace inside
 * that span stays, whitespace around it goes).  Names match as the parser matches them: raw bytes, so an escaped spelling of an
 * owned name is an unknown member and is kept.  The owned members come last, so under any reader for which a later duplicate wins
 * the owned ones win.  With last_unload == NULL, lul is an ordinary kept member.
 * Owned members, in this order, each omitted when it holds the bean's default, as Jackson omits it:
 *   1. "instanceIds":{"<id>":<time>,...}   the row's loaded entries in resident order; omitted when there are none
 *   2. "failedIn":{...}                    the failed entries likewise
 *   3. "fails":{...}                       start from the LAST top-level fails member of the old value that is an object (null or
 *        absent: none); keep, verbatim and in order, the members whose raw key bytes equal the id of an instance in the row's
 *        failed list; if fail_pod[i] >= 0, drop those keyed by that instance's id and, if its message
 *        fail_msg[fail_msg_off[i], fail_msg_off[i+1]) is not empty and the instance is in the failed list, append
 *        "<id>":{"msg":"<escaped message>"} — addLoadFailure / removeLoadFailure (ModelRecord.java:156-179) and the
 *        secondary.remove of the prune.  Escaping: '"' becomes \", '\' becomes \\, a byte below 0x20 becomes \u00xx in
 *        lower-case hex, everything else is verbatim.  Omitted when it ends up empty
 *   4. "lu":<last_used>                    omitted when 0
 *   5. "lul":<last_unload[i]>              only when last_unload is given; omitted when 0
 * Times are int64 in plain decimal, Long.MIN_VALUE included.  A row the registry holds as empty (a deleted record) renders like
 * any other: its kept members and no owned ones.
 *
 * status_out[i]: MMP_MRW_OK; MMP_MRW_MALFORMED exactly when mmp_models_upsert_json gives status 1 for the old value as a
 * non-deleted event (the parser itself runs over the old values: the write side accepts what the read side accepts, and what is
 * unspecified there stays unspecified here); MMP_MRW_HOST when the value is well-formed but the device cannot name what it must
 * render — an entry whose pod is outside [0, pod slots) (an unresolved id: its bytes are gone), or an id among the rendered entries
 * that holds a byte needing JSON escaping ('"', '\', below 0x20, above 0x7e).  Both give length 0; the host renders the latter.
 *
 * Output: new value i = out_buf[out_off[i], out_off[i+1]), out_off has n + 1 words; *n_bytes_out = the bytes of all rendered
 * values.  out_off, status_out and *n_bytes_out are always complete; NO byte of out_buf is written when out_buf is NULL or out_cap
 * is smaller than the total, and the call still returns MMP_OK: the caller repeats it with a larger buffer.  The device makes a
 * size pass, scans the sizes, the host reads the total back once, and a write pass follows if there is room.
 * Read-only: no commit, locking as mmp_models_status without a fail_pod.  flags must be 0.  last_unload may be NULL; fail_pod,
 * fail_msg, fail_msg_off may be NULL all three.  n == 0 is valid.  MMP_EINVAL with nothing written: a NULL required buffer,
 * non-monotone offsets of either kind, a row outside [0, models), a fail_pod outside [-1, pod slots), fail_pod without the two
 * message arrays, flags != 0.  MMP_ESTATE before mmp_pod_ids_load and when the id store and the instance table no longer cover
 * the same indices (the check of mmp_pods_events_json).  Two runs over the same state are byte-identical. */
#define MMP_MRW_OK 0        /* rendered */
#define MMP_MRW_MALFORMED 1 /* the old value is malformed: length 0 in the output */
#define MMP_MRW_HOST 2      /* well-formed, but the device cannot render it: length 0, the host renders this one */
int mmp_models_rewrite_json(mmp_ctx *ctx, const int32_t *rows, int32_t n, const char *old_buf, const int64_t *old_off,
                            const int64_t *last_unload, const int32_t *fail_pod, const char *fail_msg, const int32_t *fail_msg_off,
                            uint32_t flags, char *out_buf, int64_t out_cap, int64_t *out_off, int32_t *status_out,
                            int64_t *n_bytes_out);
/* ---- registerModel / deleteModel (register_kernels.hpp) ------------------------------------------------------------------------------
 * The management API's own registry writers: registerModel's touch of an existing record (ModelMesh.java:3120-3127), its creation of
 * a new one (:3135-3142) and deleteModel's conditionalDelete (:3181-3203).  A batch of such questions; each answer is a pure function
 * of the request, the stored value the host's listener holds for that key, now_ms and lastused_age_on_add_ms
 * (LASTUSED_AGE_ON_ADD_MS).  The host parses no stored value and serialises no ModelRecord; the compare-and-set itself, its retry
 * loop (call again with the value the store answered) and readOnlyMode stay in Java.
 *
 * Request i: reqs[i]; its type, encKey and mPath are the spans 3i, 3i + 1, 3i + 2 of info / info_off (3n + 1 offsets).  An EMPTY
 * encKey or mPath span is null — the Java maps "" to null before it compares (:3094-3095); an empty type span on a request that is
 * not a delete is MMP_EINVAL.  The stored value is old_buf[old_off[i], old_off[i+1]); an EMPTY span is registry.get() == null.  A
 * delete reads nothing of its three strings and its timestamp.
 *
 * last_used_out[i] = lastUsedTimestamp of :3098-3101,
 *     ts = ict >= now ? now : (ict > 0 ? ict : now - age * (loadNow ? 1 : 6))
 * in Java long arithmetic (the product and the difference wrap); 0 for a delete.  The host passes it on to ensureLoaded (:3158).
 *
 * The stored value is read as the parser reads it: the top-level member walk, names matched as raw bytes, a later duplicate wins.
 *     type            a string; absent or null reads as "NLCLASSIFIER" (ModelRecord.java:122)
 *     encKey, mPath   a string, or null / absent
 *     lu              long, absent = 0 (the parser's own reading)        refs   int, absent = 0
 *
 * class_out[i], in this order of precedence:
 *   register or delete, old span empty    MMP_MREG_CREATED with the value below / MMP_MREG_ABSENT (:3187, fine if not found)
 *   MMP_MREG_MALFORMED   exactly where mmp_models_upsert_json gives status 1 for the old value as a non-deleted event (the parser
 *                        itself runs over the old values first, as in mmp_models_rewrite_json)
 *   MMP_MREG_HOST        the value is well-formed but the device will not decide it, the host decides this one: the deciding
 *                        (last) occurrence of a member the request compares — type, encKey, mPath for a register, refs for a
 *                        delete — is a type / encKey / mPath string that holds a backslash, a type / encKey / mPath that is
 *                        neither a string nor null, or a refs that is not an integer in int32
 *   delete               refs > 0: MMP_MREG_REFERENCED (:3188-3191); otherwise MMP_MREG_DELETABLE: the host issues
 *                        conditionalDelete with the old value (:3198)
 *   MMP_MREG_CONFLICT    register, any of the three attributes unequal (:3111-3118): raw bytes of the escape-free stored string
 *                        against the request's bytes, null against null; a stored "" does not equal the request's null
 *   MMP_MREG_TOUCHED     register, attributes equal, !loadNow && ts > lu + age (the sum wraps as in Java), :3120.  The value is
 *                        every top-level member of the old value whose name is not lu, verbatim and in document order as
 *                        mmp_models_rewrite_json keeps members, then "lu":<lu'>, omitted at 0, with lu' = updateLastUsed(ts)
 *                        (ModelRecord.java:239-246): a ts of 0 means now_ms, and the value is only raised.  The class is TOUCHED
 *                        and a value is rendered even when lu' == lu: the Java submits the record all the same
 *   MMP_MREG_EXISTS      register otherwise: no compare-and-set, weCreated = false (:3129)
 * The CREATED value is {"type":"<t>","encKey":"<k>","mPath":"<p>","lu":<ts>}, each of the last three omitted at null / 0, the
 * strings escaped by the rule of mmp_models_rewrite_json ('"' and '\' behind a backslash, a byte below 0x20 as \u00xx, everything
 * else verbatim).  Every class but CREATED and TOUCHED has length 0.
 *
 * model_idx_out (may be NULL): the row of key i = keys[key_off[i], key_off[i+1]) in the resident model-id table, -1 for an unknown
 * id, from the stage mmp_model_ids_resolve uses — the host goes straight on to mmp_models_status / mmp_place_batch_c.  MMP_ESTATE
 * under that call's conditions.  With model_idx_out == NULL, keys / key_off may be NULL and no id table is needed.
 *
 * Output and sizing as mmp_models_rewrite_json: value i = out_buf[out_off[i], out_off[i+1]); out_off (n + 1 words), class_out,
 * last_used_out, model_idx_out and *n_bytes_out are always complete; NO byte of out_buf is written when out_buf is NULL or out_cap
 * is smaller than the total, and the call still returns MMP_OK.  Read-only: no commit, locking as mmp_models_status without a
 * fail_pod.  n == 0 is valid.  MMP_EINVAL with nothing written: a NULL required buffer, non-monotone offsets of any of the three
 * kinds, unknown request flag bits or a non-zero reserved word, flags != 0, now_ms <= 0, lastused_age_on_add_ms < 0, an empty type
 * on a register.  MMP_ESTATE before mmp_pod_ids_load (the parser's condition).  Two runs over the same state are byte-identical. */
typedef struct {
    uint32_t flags;
    int32_t reserved;
    int64_t initial_cache_timestamp; /* 0: not specified */
} mmp_register_req;             /* 16 bytes */
#define MMP_MREG_LOAD_NOW 1u    /* registerModel(loadNow = true) */
#define MMP_MREG_DELETE 2u      /* deleteModel: the three strings and the timestamp are ignored */
/* class_out */
#define MMP_MREG_CREATED 0      /* no stored value: the new record is rendered */
#define MMP_MREG_TOUCHED 1      /* the same model, lu raised: the next value is rendered */
#define MMP_MREG_EXISTS 2       /* the same model, nothing to write */
#define MMP_MREG_CONFLICT 3     /* "Model already exists with different attribute values" */
#define MMP_MREG_ABSENT 4       /* delete of a model that is not there */
#define MMP_MREG_REFERENCED 5   /* delete refused: the model has referents */
#define MMP_MREG_DELETABLE 6    /* delete: conditionalDelete with the old value */
#define MMP_MREG_MALFORMED 7    /* the old value is malformed */
#define MMP_MREG_HOST 8         /* well-formed, but the host decides this one */
int mmp_models_register_json(mmp_ctx *ctx, const mmp_register_req *reqs, int32_t n, const char *keys, const int32_t *key_off,
                             const char *info, const int32_t *info_off, const char *old_buf, const int64_t *old_off, int64_t now_ms,
                             int64_t lastused_age_on_add_ms, uint32_t flags, char *out_buf, int64_t out_cap, int64_t *out_off,
                             int32_t *class_out, int64_t *last_used_out, int32_t *model_idx_out, int64_t *n_bytes_out);
/* ---- the vmodel table on the device (vmodel_kernels.hpp) ------------------------------------------------------------------------
 * VModelManager.java:101-110 watches a second table: vmodel id -> VModelRecord {o, amid, tmid, failed} (VModelRecord.java:26-41).
 * The context keeps it on the device like the registry: an id -> row map with the open addressing of the model-id table (a slot is
 * matched on the 64-bit FNV-1a hash AND the bytes, ids that collide coexist, a slot is never deleted in place) and one row per
 * vmodel holding the raw bytes of amid, tmid and o in a string arena, the model-id hashes of amid and tmid, and the MMP_VMF_* flags.
 * NO registry row is stored in a vmodel row: amid and tmid are looked up in the model-id table when a question is asked, so a model
 * that joins later, or one mmp_models_retire renumbered, is found without any vmodel call in between.  The state exists only once
 * the first vmodel call has been made; the table starts empty at mmp_create, and start-up is one mmp_vmodels_events_json batch
 * with MMP_VMEV_APPEND — there is no separate load call.  The string arena grows by append: an applied event leaves its
 * predecessor's strings as garbage, which is squeezed out when it exceeds the live bytes.
 * MMP_VMODEL_ID_HASH_BITS=b (read with the other MMP_* switches, per context at mmp_create) masks every vmodel-id hash to its low b
 * bits, 0: all equal — the diagnostic of MMP_MODEL_ID_HASH_BITS for this table.
 * Writes stay with the host: updateVModel / deleteVModel are multi-key KV transactions. */
#define MMP_VMF_FAILED 1u      /* `failed` as stored                                                 */
#define MMP_VMF_ABSENT 2u      /* never set, or deleted                                              */
#define MMP_VMF_ACTIVE_NULL 4u /* amid absent or null                                                */
#define MMP_VMF_TARGET_NULL 8u /* tmid absent or null                                                */
#define MMP_VMF_OWNER_NULL 16u /* o absent or null                                                   */
#define MMP_VMF_HOST 32u       /* one of the three strings holds a backslash escape: the host decodes this one record */
/* The listener's events as it gets them: event i is the vmodel id keys[key_off[i], key_off[i+1]) — the raw bytes of the KV key —
 * with the VModelRecord value buf[off[i], off[i+1]).  The contract is that of mmp_models_events_json, clause for clause: the keys
 * are resolved, deduplicated and numbered on the device by the same kernels; deleted[i] != 0 is ENTRY_DELETED: the value is
 * ignored and the row becomes ABSENT; it KEEPS its id and its number, and an id that is set again gets its old row back.
 * status_out[i]: 0 applied, 1 malformed value, 2 unknown id (nothing changes; vmodel_idx_out[i] = -1).  An id the table does not
 * know: with MMP_VMEV_APPEND in flags the distinct unknown ids of NON-DELETED events join as rows V0, V0+1, ... (V0 = the row count
 * at the call) in order of first appearance, whether or not their values turn out well-formed (a joined row whose events are all
 * malformed is ABSENT); without the flag such an event is status 2.  A deletion never appends: of an id that is unknown when the
 * event is reached — the table and the events before it — it is status 2; behind the event that made the id join, it applies.
 * Events apply in order: a row ends as its LAST WELL-FORMED OR DELETED event left it.
 * The value: amid, tmid and o are each a string or null, failed is true / false; every occurrence of one of the four is held to
 * its type, a later duplicate wins (a later null included), any other member is skipped whatever its type (JsonExtensible), and
 * nothing but blanks may follow the closing brace — the grammar and the verdicts of mmp_models_upsert_json.  A value of 2^30
 * bytes or more is refused.  The strings are kept as their raw bytes between the quotes; one that holds a backslash flags the row
 * MMP_VMF_HOST.
 * vmodel_idx_out[i] = the resolved row; *n_appended_out = ids that joined.  deleted, n_appended_out may be NULL.
 * Only O(events) words come back to the host; two runs over the same state and events are byte-identical, whichever lanes raced.
 * MMP_EINVAL with nothing changed (table, id arena, rows, string arena): a NULL required buffer, non-monotone offsets of either
 * kind, unknown flags, a value of 2^30 bytes or more, more than 2^31 arena bytes.  The call needs neither mmp_model_ids_load nor
 * mmp_pod_ids_load: the hashes of amid / tmid are computed from the bytes.  Locking: batch_mu for the call, which every
 * reader of the vmodel state holds too except the request calls by vmodel id on a latency slot (mmp_*_batch_cv), which capture
 * the published table under the state lock.  So the id table, the id arena and string arena where they have to grow, and the row
 * array whenever a row of a known id is rewritten or it has to grow, are built beside the published ones and swapped together
 * with the counts under the state lock, and what the swap retired is neither reused nor released before the latency slots have
 * drained behind it.  n == 0 is valid. */
#define MMP_VMEV_APPEND 1u
int mmp_vmodels_events_json(mmp_ctx *ctx, const char *keys, const int32_t *key_off, const char *buf, const int64_t *off, int32_t n,
                            const uint8_t *deleted, uint32_t flags, int32_t *vmodel_idx_out, int32_t *status_out,
                            int32_t *n_appended_out);
/* resolveVModelId (VModelManager.java:569-597, from ModelMeshApi.callModel :457-476) and the classes getVModelStatus needs
 * (:505-528, :537-559), one question per request, one lane per question: key i = keys[key_off[i], key_off[i+1]) is the vmodel id,
 * nf i = nf_keys[nf_off[i], nf_off[i+1]) the notFoundModelId and owner i = owners[owner_off[i], owner_off[i+1]) the owner; an empty
 * span is Java null, and nf_keys / nf_off, owners / owner_off and req_flags may each be NULL (all null / 0).  Strings compare on
 * bytes; a stored null equals nothing (String.equals(null)).
 * rows_out[i].cls:
 *   MMP_VMR_NOT_FOUND         the id is unknown or the row is ABSENT (:570-573); also when an owner is given and differs from the
 *                             stored one byte for byte (absentOrOwnerMismatch, :530-532; a row with OWNER_NULL mismatches any owner)
 *   MMP_VMR_HOST              the row is flagged MMP_VMF_HOST: the host decodes the record (mmp_vmodels_get) and decides
 *   MMP_VMR_OK                `which` (MMP_VMW_ACTIVE / MMP_VMW_TARGET) names the id resolveVModelId returns; MMP_VMRF_NULL_ID in
 *                             flags when that id is null (the Java returns null), model = -1 then
 *   MMP_VMR_STRONG_READ       nf equals the active id as held (:575 fails): the host performs vModels.getStrong (:582), sends that
 *                             value through mmp_vmodels_events_json and asks again with MMP_VMRQ_AFTER_STRONG in req_flags[i]
 *   MMP_VMR_TARGET_NOT_FOUND  with MMP_VMRQ_AFTER_STRONG (:587-596): active if it differs from nf, else target if it differs, else
 *                             this — the Java throws INTERNAL "Target model ... not found".  An empty nf answers active in
 *                             either phase
 * vmodel = the row (-1 for NOT_FOUND); model = the registry row of the answered id in the model-id table, -1 when the table does
 * not know it (or the class answers none); target_model likewise for tmid; vstatus = MMP_VMS_DEFINED / _TRANSITIONING /
 * _TRANSITION_FAILED (:555-556; inTransition() is !Objects.equals(amid, tmid) on bytes, null-aware); target_status = 0 when not in
 * transition, otherwise (:537-549) MMP_VMT_LOADING_FAILED when `failed` is set and the target's resident row has n_failed > 0 and
 * n_loaded == 0, MMP_VMT_NOT_FOUND when the target's row is unknown or is the empty row, MMP_VMT_LOADING otherwise;
 * mmp_models_status fills in the rest.  (The Java would throw a NullPointerException at :544 for `failed` with a missing target
 * record; the device answers MMP_VMT_NOT_FOUND there.)  For NOT_FOUND and HOST every other field is -1 / 0.
 * Read-only, no commit.  MMP_ESTATE under the conditions of mmp_model_ids_resolve (no model-id table, or the registry resized by
 * index since).  MMP_EINVAL with nothing written: a NULL required buffer, non-monotone offsets of any of the three kinds, unknown
 * request flag bits.  Locking as mmp_model_ids_resolve: the model-id table is owned by batch_mu, so the call holds it and is
 * serialised with the event calls (it sees the state before or after one, never a mix); it does not take the state lock
 * exclusive, so the request calls go on beside it.  n == 0 is valid.  Two runs over the same state are byte-identical. */
#define MMP_VMRQ_AFTER_STRONG 1u
#define MMP_VMR_NOT_FOUND 0
#define MMP_VMR_OK 1
#define MMP_VMR_STRONG_READ 2
#define MMP_VMR_TARGET_NOT_FOUND 3
#define MMP_VMR_HOST 4
#define MMP_VMW_ACTIVE 0
#define MMP_VMW_TARGET 1
#define MMP_VMRF_NULL_ID 1u
#define MMP_VMS_DEFINED 0
#define MMP_VMS_TRANSITIONING 1
#define MMP_VMS_TRANSITION_FAILED 2
#define MMP_VMT_NONE 0
#define MMP_VMT_LOADING 1
#define MMP_VMT_LOADING_FAILED 2
#define MMP_VMT_NOT_FOUND 3
typedef struct {
    int32_t cls, which;
    int32_t vmodel, model, target_model;
    int32_t vstatus, target_status;
    uint32_t flags;
} mmp_vmodel_answer; /* 32 bytes */
int mmp_vmodels_resolve(mmp_ctx *ctx, const char *keys, const int32_t *key_off, int32_t n, const char *nf_keys, const int32_t *nf_off,
                        const char *owners, const int32_t *owner_off, const uint32_t *req_flags, mmp_vmodel_answer *rows_out);
/* getVModelStatus IN FULL (VModelManager.java:505-559) as ONE staged call under one hold of the batch lock: what a host otherwise
 * stitches from mmp_vmodels_resolve, mmp_models_status on two rows per vmodel and mmp_vmodels_get per row — with an event batch or
 * a retirement free to land between any two of them (csrc/status_keyed_kernels.hpp).
 *   keys / key_off       n vmodel ids
 *   owners / owner_off   may be NULL; an empty span is Java null (emptyToNull, :506)
 *   req_flags            n words, may be NULL; the only bit is MMP_VMRQ_AFTER_STRONG
 *   vrows_out            n rows (below)
 *   rows_out             2n mmp_status_row: row 2i is the active model's answer, row 2i + 1 the target's; copy_off is the
 *                        exclusive prefix sum over the 2n rows in that order
 *   copies_out / max_copies / n_copies_out   as mmp_models_status
 *   str_off_out          3n + 1 words, rebased to 0, may be NULL: span 3i is amid, 3i + 1 tmid, 3i + 2 o
 *   str_bytes_out / max_str_bytes / n_str_bytes_out   under the conventions of mmp_vmodels_get: the total always, the offsets
 *                        always, the bytes only when max_str_bytes >= the total; raw bytes as stored, a null string is an empty
 *                        span and vrows_out[i].flags tells it from ""
 *
 * THE RULE.  Let a be what mmp_vmodels_resolve answers for (key i, no nf, owner i, req_flags i) against the state the call
 * captured.  cls, vmodel, target_model, vstatus and target_status are a's; `model` is the row of amid as the model-id table knows
 * it, else -1; flags = the row's MMP_VMF_FAILED / _ACTIVE_NULL / _TARGET_NULL / _OWNER_NULL as stored.  The active request (row 2i)
 * is {m, -1, 0, 0}: m = model, or -1 when amid is null, unknown or names the empty row (:513).  The target request (row 2i + 1) is
 * {t, -1, 0, 0}: t = target_model when the vmodel is in transition and that row is known and not empty, else -1 (:538, :548; the
 * device keeps answering MMP_VMT_NOT_FOUND where the Java would throw at :544).  Rows 2i, 2i + 1 and their copies are byte for
 * byte what mmp_models_status answers for those two requests.
 *   The strong read (:514-525): cls becomes MMP_VMR_STRONG_READ when a.cls is MMP_VMR_OK, the active answer's class is
 *   MMP_MST_NOT_FOUND and MMP_VMRQ_AFTER_STRONG is clear.  Every other field is still filled in.  The host performs getStrong,
 *   sends the value through mmp_vmodels_events_json and asks again with the flag; with the flag the answer stands as it is.
 *   MMP_VMR_NOT_FOUND (absent row, unknown id, owner mismatch) and MMP_VMR_HOST: both status rows are the -1 request's answer,
 *   all three spans are empty, flags is 0, the ids are -1 (except vmodel for HOST).  An owner mismatch says nothing of the record:
 *   the Java returns the default instance.
 *
 * MMP_EINVAL, every output untouched: what mmp_vmodels_resolve refuses (a NULL required buffer, offsets of either kind that are
 * not monotone, unknown request flag bits), what mmp_models_status refuses of its buffers, more than INT32_MAX copies or string
 * bytes in all.  MMP_ESTATE as mmp_vmodels_resolve.  Read-only, no commit; a context that never had a vmodel call answers
 * MMP_VMR_NOT_FOUND for everything.  n == 0 is valid.  Two runs over the same state are byte-identical. */
typedef struct {
    int32_t cls;                  /* MMP_VMR_NOT_FOUND / _OK / _STRONG_READ / _HOST */
    int32_t vmodel, model, target_model;
    int32_t vstatus, target_status; /* MMP_VMS_*, MMP_VMT_* */
    uint32_t flags;               /* MMP_VMF_FAILED | _ACTIVE_NULL | _TARGET_NULL | _OWNER_NULL */
    int32_t reserved;             /* 0 */
} mmp_vstatus_row; /* 32 bytes */
int mmp_vmodels_status(mmp_ctx *ctx, const char *keys, const int32_t *key_off, int32_t n, const char *owners,
                       const int32_t *owner_off, const uint32_t *req_flags, int64_t now_ms, mmp_vstatus_row *vrows_out,
                       mmp_status_row *rows_out, mmp_status_copy *copies_out, int32_t max_copies, int32_t *n_copies_out,
                       char *str_bytes_out, int32_t max_str_bytes, int32_t *str_off_out, int32_t *n_str_bytes_out);
/* The single-caller request forms BY VMODEL ID: ModelMeshApi.callModel (:452-476) for a request that names a vmodel — first
 * resolveVModelId(vModelId, notFoundModelId), then invokeModel's seams on the model id it returned.  With mmp_vmodels_resolve (a
 * staged call under the batch lock, which answers a registry ROW) in front of a _c call that is two calls and one batch lock on the
 * request path.  These are the _ck forms (mmp_place_batch_ck ...) with the resolution of the VMODEL id inside the call: one latency
 * slot, one stream, one wait, no batch lock (csrc/vkeyed_kernels.hpp).  Against the _ck signatures:
 *   keys / key_off     key i is the VMODEL id of request i
 *   nf_keys / nf_off   behind them: the notFoundModelId spans under the conventions of mmp_vmodels_resolve — both may be NULL, an
 *                      empty span is Java null
 *   req_flags          n words, may be NULL; the only bit is MMP_VMRQ_AFTER_STRONG.  There are no owners: resolveVModelId on the
 *                      request path takes none
 *   vm_out             n rows in place of model_idx_out, may be NULL; `reserved` is written 0.  cls is MMP_VMR_*, which MMP_VMW_*,
 *                      flags MMP_VMRF_NULL_ID
 *
 * THE RULE BY VMODEL KEY: vm_out[i] equals, field by field, what mmp_vmodels_resolve answers for (key i, nf i, no owner, flags i)
 * against the vmodel table, the model-id table and the registry row count as published at the moment the call captured them.
 * Request i is decided exactly as the _c call decides the same rows with model = r, where r = vm_out[i].model when cls ==
 * MMP_VMR_OK and MMP_VMRF_NULL_ID is clear, and r = -1 otherwise: NOT_FOUND, HOST, STRONG_READ, TARGET_NOT_FOUND, a null id, or an
 * id the model-id table does not know.  The result rows are those rows' results byte for byte.  The caller's arrays are never
 * written, and the `model` fields of the request rows are ignored on input.  The host reads cls before it believes a decision; on
 * MMP_VMR_STRONG_READ it does what mmp_vmodels_resolve asks for (getStrong, the value through mmp_vmodels_events_json, the call
 * again with MMP_VMRQ_AFTER_STRONG).  A vmodel event batch, mmp_vmodels_retire (which renumbers vmodel rows) and the registry's
 * event batches and retirements are each seen before or after, never as a mix.
 *
 * MMP_EINVAL, every output untouched: everything the _ck forms refuse; nf_off that is not monotone; NULL nf_keys with nf bytes
 * present; unknown request flag bits.  MMP_ESTATE as the _ck forms.  A context that never had a vmodel call has an empty vmodel
 * table: a valid call, every request answers MMP_VMR_NOT_FOUND.  n = 0 is a valid call.  Up to 256 requests with up to 8192 key
 * bytes and up to 8192 nf bytes (and the pools of the _ck forms' latency path) ride a latency slot; larger calls are staged under
 * the batch lock on the compact rows, as the _ck forms are. */
typedef struct {
    int32_t cls, which;
    int32_t vmodel, model;
    uint32_t flags;
    int32_t reserved;
} mmp_vseam_row; /* 24 bytes */
int mmp_place_batch_cv(mmp_ctx *ctx, const mmp_place_caller *caller, const mmp_place_req_c *reqs, int32_t n, const char *keys,
                       const int32_t *key_off, const char *nf_keys, const int32_t *nf_off, const uint32_t *req_flags,
                       const int32_t *extra_pool, int32_t n_extra, int64_t now_ms, mmp_place_out *outs, mmp_vseam_row *vm_out);
int mmp_route_batch_cv(mmp_ctx *ctx, const mmp_seam_caller *caller, const mmp_gate_req_c *gate_reqs,
                       const mmp_serve_req_c *serve_reqs, int32_t n, const char *keys, const int32_t *key_off, const char *nf_keys,
                       const int32_t *nf_off, const uint32_t *req_flags, const mmp_serve_counter *counters, int32_t n_counters,
                       const int32_t *excl_pod, const int64_t *excl_time, int32_t n_excl, const int32_t *explicit_pool,
                       int32_t n_explicit, int64_t now_ms, int64_t in_use_expiry_ms, mmp_gate_out *gate_outs,
                       mmp_serve_out *serve_outs, mmp_vseam_row *vm_out);
int mmp_miss_batch_cv(mmp_ctx *ctx, const mmp_seam_caller *caller, const mmp_place_caller *place_caller,
                      const mmp_gate_req_c *gate_reqs, const mmp_place_req_c *place_reqs, int32_t n, const char *keys,
                      const int32_t *key_off, const char *nf_keys, const int32_t *nf_off, const uint32_t *req_flags,
                      const int32_t *excl_pod, const int64_t *excl_time, int32_t n_excl, const int32_t *explicit_pool,
                      int32_t n_explicit, const int32_t *extra_pool, int32_t n_extra, int64_t now_ms, int64_t in_use_expiry_ms,
                      mmp_gate_out *gate_outs, mmp_place_out *place_outs, mmp_vseam_row *vm_out);
/* The leader's transition pass: processVModels (:617-634), the filter of processVModel (:639-643) and the prologue of
 * PendingTransition.run (:701-708) as one scan over all rows in row order.  Listed: every row that is not ABSENT, not HOST and
 * in transition.  Per listed row: vmodel; from_model / to_model = the registry rows of amid / tmid, -1 for null or unknown;
 * target_count = curActive.getInstanceIds().size() — the resident row's n_loaded, unresolved entries included, 0 when from_model
 * is -1; cls = MMP_VMX_PROMOTE when target_count == 0 (:703 is skipped, the host goes straight to the record update at :749), else
 * MMP_VMX_ENSURE_LOADED with last_used = the row's last_used, or now_ms - lastused_age_on_add_ms in Java long arithmetic when that
 * is 0 (:705-708); last_used is 0 for PROMOTE.  flags: MMP_VMXF_FAILED as stored, MMP_VMXF_FROM_EMPTY / _TO_EMPTY when that registry
 * row is the empty row (what a deletion leaves: the definition of MMP_RETIRE_EMPTY_ONLY).
 * Sizing and truncation as mmp_registry_unresolved: *n_out = the listed rows, always; rows_out receives the first
 * min(*n_out, max_rows) of them in row order, rows_out may be NULL with max_rows == 0.  info_out (may be NULL): counts per class,
 * the HOST rows skipped, truncated = *n_out > max_rows.  No atomic decides a position: two runs are byte-identical.
 * What stays with the host: the pendingTransitions de-duplication (:644-652), the status switch after ensureLoadedInternal
 * (:716-747, which asks mmp_models_status), stuckTransitions / processModelChange, and the transaction.
 * Read-only, locking and MMP_ESTATE as mmp_vmodels_resolve.  MMP_EINVAL with nothing written: a NULL n_out, max_rows < 0, max_rows
 * > 0 without rows_out.  An empty vmodel table lists nothing. */
#define MMP_VMX_PROMOTE 0
#define MMP_VMX_ENSURE_LOADED 1
#define MMP_VMXF_FAILED 1u
#define MMP_VMXF_FROM_EMPTY 2u
#define MMP_VMXF_TO_EMPTY 4u
typedef struct {
    int32_t vmodel, from_model, to_model, target_count;
    int32_t cls;
    uint32_t flags;
    int64_t last_used;
} mmp_vmodel_transition; /* 32 bytes */
typedef struct {
    int32_t n_listed, n_promote, n_ensure_loaded, n_host_skipped, truncated, reserved;
} mmp_vmodel_transitions_info; /* 24 bytes */
int mmp_vmodels_transitions(mmp_ctx *ctx, int64_t now_ms, int64_t lastused_age_on_add_ms, mmp_vmodel_transition *rows_out,
                            int32_t max_rows, int32_t *n_out, mmp_vmodel_transitions_info *info_out);
/* The way back: rows [first_row, first_row + n_rows).  Their ids as mmp_model_ids_get gives model ids: *n_id_bytes_out always,
 * id_off_out (n_rows + 1 words, rebased to 0) when not NULL, the bytes when max_id_bytes >= *n_id_bytes_out.  flags_out (n_rows
 * words, may be NULL) = MMP_VMF_*.  The three strings of row r are spans 3r (amid), 3r + 1 (tmid), 3r + 2 (o) of str_bytes_out /
 * str_off_out (3 * n_rows + 1 words, rebased to 0, may be NULL), raw bytes as stored, a null string an empty span (the flags tell
 * it from ""): *n_str_bytes_out always, the bytes when max_str_bytes >= *n_str_bytes_out.  Copies only, no kernel.  MMP_EINVAL
 * with nothing written for a range outside the table or a NULL required buffer.  Locking: batch_mu. */
int mmp_vmodels_get(mmp_ctx *ctx, int32_t first_row, int32_t n_rows, char *id_bytes_out, int32_t max_id_bytes, int32_t *id_off_out,
                    int32_t *n_id_bytes_out, uint32_t *flags_out, char *str_bytes_out, int32_t max_str_bytes, int32_t *str_off_out,
                    int32_t *n_str_bytes_out);
/* For tests and operators: rows, rows that are not ABSENT, the string arena's bytes and those a row refers to, the id table's
 * capacity (0 before the first vmodel call).  No kernel.  Locking: batch_mu. */
typedef struct {
    int32_t n_rows, n_live;
    int64_t arena_bytes, live_bytes;
    int32_t capacity, reserved;
} mmp_vmodels_stats; /* 32 bytes */
int mmp_vmodels_info(mmp_ctx *ctx, mmp_vmodels_stats *out);
/* Retire vmodel rows: the named rows leave the index space, and the vmodel rows, the string arena, the vmodel-id arena and the
 * vmodel-id table are compacted on the device (vmodel_retire_kernels.hpp) — the counterpart of mmp_models_retire for the third
 * resident table.  rows[0 .. n) are vmodel rows in [0, V0), V0 = the row count at the call, in any order; a row named twice is
 * retired once.  The survivors keep their relative order and move down: a survivor's new row is its old row minus the number of
 * retired rows below it.  remap_out (may be NULL; else max_vmodels >= V0 words): remap_out[old] = the new row, -1 for a retired
 * one, for all V0 old rows.  *n_vmodels_after_out (may be NULL) = the new count V1.
 * Rows: a survivor keeps its flags (MMP_VMF_*, HOST included), the raw bytes of amid, tmid and o (a null stays null and "" stays
 * "": the flags tell them apart) and its two model-id hashes as stored; the retired rows' strings are dropped, and the call leaves
 * the string arena squeezed (arena_bytes == live_bytes in mmp_vmodels_info; n_live and live_bytes follow).  Vmodel-id table: the
 * retired ids leave the table and the id arena, mmp_vmodels_resolve of a retired id answers MMP_VMR_NOT_FOUND with vmodel == -1,
 * mmp_vmodels_get returns the survivors' ids under their new rows, the table has the capacity a fresh context reports after one
 * MMP_VMEV_APPEND batch of V1 ids — 0 when no row is left: the state before the first vmodel call — (no string is hashed again:
 * MMP_MODEL_ID_HASH_BITS and MMP_VMODEL_ID_HASH_BITS still hold), and a retired id that arrives again through
 * mmp_vmodels_events_json with MMP_VMEV_APPEND joins as a new row at the end, like any unknown id; without the flag, and for a
 * deletion, it is status 2.  A vmodel row stores ids and never registry rows: nothing on the model side is touched.
 * MMP_VMRETIRE_ABSENT_ONLY guards the intended loop — (1) deletion events arrive, (2) the host collects their vmodel_idx, (3) it
 * retires them later: every named row must then carry MMP_VMF_ABSENT, checked on the device rows; if one does not — its id was
 * set again in between — the call is MMP_EINVAL with nothing changed and mmp_last_error names the lowest such row.
 * MMP_VMRETIRE_ALL_ABSENT: the device chooses — every row flagged MMP_VMF_ABSENT at the call is retired; n must be 0 (a list
 * beside the flag is MMP_EINVAL).  The form for a host that keeps no id map.  MMP_VMRETIRE_ABSENT_ONLY beside it is accepted and
 * adds nothing.
 * Readers: no decision kernel reads vmodel state; mmp_vmodels_resolve, _transitions, _get and _info hold batch_mu, which this
 * call holds throughout, and the request calls by vmodel id (mmp_*_batch_cv) capture the table under the state lock — either kind
 * sees the numbering before the retire or after it, never a mix; no resolved view is rebuilt.  The new rows, arenas and table are
 * built beside the published ones and swapped together with the counts under the state lock, as mmp_vmodels_events_json swaps
 * what it built, and the latency slots are drained behind the swap before what it retired is released; everything that can fail — allocation, a HIP error,
 * an id the verifying lookup does not find (MMP_EHIP) — fails before the swap, with nothing published.  Row numbers the HOST holds
 * — answers of mmp_vmodels_resolve and _transitions — are the host's to renumber from remap_out.
 * MMP_EINVAL with nothing changed and every output untouched: NULL rows with n > 0, a row outside [0, V0), an unknown flag bit,
 * max_vmodels < 0, remap_out with max_vmodels < V0, a row that is not ABSENT under MMP_VMRETIRE_ABSENT_ONLY,
 * MMP_VMRETIRE_ALL_ABSENT with n > 0.  No MMP_ESTATE: the call needs neither mmp_model_ids_load nor mmp_pod_ids_load.  n == 0
 * without MMP_VMRETIRE_ALL_ABSENT — and that flag where no row is ABSENT — is valid and changes nothing (no squeeze, no launch):
 * remap_out is the identity, *n_vmodels_after_out = V0; also before the first vmodel call, where V0 == 0.  No commit is needed
 * before or after.  The work is O(table), as a rebuild from the survivors is — the host decides how often to call; two runs over
 * the same state and list are byte-identical.  Locking: batch_mu throughout. */
#define MMP_VMRETIRE_ABSENT_ONLY  1u
#define MMP_VMRETIRE_ALL_ABSENT   2u
int mmp_vmodels_retire(mmp_ctx *ctx, const int32_t *rows, int32_t n, uint32_t flags, int32_t *remap_out, int32_t max_vmodels,
                       int32_t *n_vmodels_after_out);
/* ---- incRefCount / decRefCount on stored ModelRecord values (refs_kernels.hpp) -----------------------------------------------------
 * The write side of the vmodel transactions, the ModelRecord half: updateVModel (VModelManager.java:137-385), deleteVModel
 * (:416-470) and the tail of PendingTransition.run (:716-767) each change `refs` on up to three ModelRecords — the new target gains
 * a referent and a lastUsed (:299-302), a model the vmodel lets go loses one and is deleted with it when it was created for it
 * (decModelRefsInTxn :475-489).  A batch of such steps; the next bytes of a record are a pure function of the request and of the
 * stored value the host holds for that id.  The host parses no stored value and serialises no ModelRecord; the transaction, its
 * retry loop (call again with the values the store answered) and readOnlyMode stay in Java.
 *
 * Request i: reqs[i], on the stored value old_buf[old_off[i], old_off[i+1]); an EMPTY span is mr == null.  With MMP_MREF_INC the
 * request is setLastUsed(last_used) + incRefCount() (:301-302), without it decModelRefsInTxn, which reads nothing else of the
 * request.  info / info_off (3n + 1 offsets; both may be NULL: every span empty) bring type, encKey and mPath as the spans 3i,
 * 3i + 1, 3i + 2, as in mmp_models_register_json; they are read only by an INC onto no stored value, as is MMP_MREF_AUTO_DELETE
 * (the autoDelete of the record :294 creates).
 *
 * The stored value is read as mmp_models_register_json reads it: the top-level member walk, names matched as raw bytes, a later
 * duplicate wins.
 *     refs      int, absent = 0; what that call's delete guard refuses (not an integer in int32) is MMP_MREFC_HOST
 *     autoDel   the literal true or false, absent = false; anything else is MMP_MREFC_HOST.  Read only by a DEC
 * A DEC (ModelRecord.java:213-215, refCount > 0 ? --refCount : 0): the FIELD becomes refs > 0 ? refs - 1 : refs — a stored -1
 * stays -1 — and the RETURN value is refs > 0 ? refs - 1 : 0.  An INC (:220-222): both are refs + 1 as a Java int, 2^31 - 1 wraps
 * to -2^31; setLastUsed sets unconditionally.
 *
 * class_out[i], in this order of precedence:
 *   DEC, old span empty                   MMP_MREFC_ENSURE_ABSENT (:485-487, txn.ensureAbsent).  Length 0
 *   INC, old span empty, type not empty   MMP_MREFC_CREATED with the value
 *                                         {"type":"<t>","encKey":"<k>","mPath":"<p>","refs":1,"autoDel":true,"lu":<last_used>},
 *                                         encKey / mPath omitted at an empty span, autoDel without MMP_MREF_AUTO_DELETE, lu at 0; the
 *                                         strings escaped by the rule of mmp_models_rewrite_json (:294, :301-302)
 *   INC, old span empty, type empty       MMP_MREFC_NOT_FOUND (:203-205, "Target model not found"); also with info_off == NULL
 *   MMP_MREFC_MALFORMED   exactly where mmp_models_upsert_json gives status 1 for the old value as a non-deleted event (the parser
 *                         itself runs over the old values first, as in the other two calls)
 *   MMP_MREFC_HOST        the value is well-formed but the device will not decide it, by the refs / autoDel rules above
 *   DEC, return == 0 && autoDel           MMP_MREFC_DELETE (:478-480).  Length 0: the host deletes with the old value.  A stored
 *                                         refs of 0 or -1 with autoDel is a DELETE too: the return value decides
 *   DEC otherwise                         MMP_MREFC_SET: every top-level member of the old value not named refs, verbatim and in
 *                                         document order as mmp_models_rewrite_json keeps members, then "refs":<field>, omitted at 0
 *   INC, stored value present             MMP_MREFC_SET: every member not named refs or lu, then "refs":<refs + 1>, omitted at 0,
 *                                         then "lu":<last_used>, omitted at 0
 * refs_out[i] = the count the Java method returns (1 for CREATED); 0 for the classes that compute none.  Numbers are plain decimal,
 * Long.MIN_VALUE included.  Every class but SET and CREATED has length 0.
 *
 * Output and sizing as mmp_models_rewrite_json: value i = out_buf[out_off[i], out_off[i+1]); out_off (n + 1 words), class_out,
 * refs_out and *n_bytes_out are always complete; NO byte of out_buf is written when out_buf is NULL or out_cap is smaller than the
 * total, and the call still returns MMP_OK.  Read-only: no commit, locking as mmp_models_register_json.  n == 0 is valid.
 * MMP_EINVAL with every output untouched: a NULL required buffer (info and info_off may be NULL), non-monotone offsets of either
 * kind, unknown request flag bits or a non-zero reserved word, flags != 0, out_cap < 0, a value of 2^31 bytes or more.  MMP_ESTATE
 * before mmp_pod_ids_load (the parser's condition).  Two runs are byte-identical. */
typedef struct {
    uint32_t flags;
    int32_t reserved;
    int64_t last_used; /* an INC: the record's next lu (newLastUsedTime, :299-300) */
} mmp_refs_req;                      /* 16 bytes */
#define MMP_MREF_INC 1u              /* setLastUsed(last_used) + incRefCount(); without it: decModelRefsInTxn */
#define MMP_MREF_AUTO_DELETE 2u      /* read only by an INC onto no stored value: autoDelete of the created record */
/* class_out */
#define MMP_MREFC_SET 0              /* txn.set: the next value is rendered */
#define MMP_MREFC_CREATED 1          /* no stored value, an INC with a type: the new record is rendered */
#define MMP_MREFC_DELETE 2           /* a DEC to 0 of an autoDel record: txn.delete with the old value */
#define MMP_MREFC_ENSURE_ABSENT 3    /* a DEC of no stored value: txn.ensureAbsent */
#define MMP_MREFC_NOT_FOUND 4        /* an INC of no stored value and no type */
#define MMP_MREFC_MALFORMED 5        /* the old value is malformed */
#define MMP_MREFC_HOST 6             /* well-formed, but the host decides this one */
int mmp_models_refs_json(mmp_ctx *ctx, const mmp_refs_req *reqs, int32_t n, const char *info, const int32_t *info_off,
                         const char *old_buf, const int64_t *old_off, uint32_t flags, char *out_buf, int64_t out_cap, int64_t *out_off,
                         int32_t *class_out, int32_t *refs_out, int64_t *n_bytes_out);
/* ---- the record step of the three vmodel writers (vmodel_write_kernels.hpp) ----------------------------------------------------------
 * updateVModel (VModelManager.java:137-385), deleteVModel (:416-470) and the tail of PendingTransition.run (:716-767) each read the
 * stored VModelRecord, decide, render the next one and name up to two models that lose a referent.  A batch of such steps; each
 * answer is a pure function of the request, the stored value, now_ms, lastused_age_on_add_ms (LASTUSED_AGE_ON_ADD_MS) and two facts
 * of the resident registry — the loaded copies of the previous active model (:248, :261) and its lastUsed (:299).  The transaction,
 * its retry loop (call again with the values the store answered), the waiters and readOnlyMode stay in Java; the ModelRecord half
 * of a transaction is mmp_models_refs_json.  The resident vmodel table is not read and need not exist.
 *
 * Request i: reqs[i]; its strings are the spans 3i (id_a), 3i + 1 (id_b), 3i + 2 (owner) of strs / str_off (3n + 1 offsets); an EMPTY
 * span is Java null.  The stored value is old_buf[old_off[i], old_off[i+1]); an EMPTY span is vmr == null.  It is read by the grammar
 * and the verdicts of mmp_vmodels_events_json (the parser itself runs over the old values first): a malformed value is
 * MMP_VWC_MALFORMED; amid, tmid and o are strings or null (absent = null), failed a boolean (absent = false), a later duplicate
 * wins; strings compare on raw bytes, a stored null equals nothing.  MMP_VWC_HOST: the value is well-formed but the stored amid or
 * tmid (every op but FAIL_FLAG) or, where a SET or DELETE brings an owner, the stored o holds a backslash.  default_owner
 * (default_owner_len bytes, 0: none) is DEFAULT_OWNER of :282.
 *
 * Rendering.  The next value is every top-level member of the old value not named amid / tmid / failed, verbatim and in document
 * order as mmp_models_rewrite_json keeps members, duplicates included, o among them (it is final in the bean); then "amid":"..",
 * "tmid":"..", "failed":true, each omitted at null / false.  A string that stays is copied raw from the stored value; one the
 * request brings is escaped by the rule of mmp_models_rewrite_json.  A CREATED value is {"o":"<owner>","amid":"<id_a>",
 * "tmid":"<id_a>"}, the owner the request's, else default_owner, else omitted.  Only CREATED and UPDATED have a length.
 *
 * MMP_VW_SET (updateVModel :174-189, :216-284): id_a = targetModelId (empty: MMP_EINVAL), id_b = expectedTargetModelId.
 *   no stored value, in this order (the strong read of :174-179 stands in front of the loop):
 *     id_b given and != id_a            MMP_VWC_PRECONDITION (:178, :280)
 *     MMP_VWQ_UPDATE_ONLY               MMP_VWC_NOT_FOUND (:277)
 *     otherwise                         MMP_VWC_CREATED
 *   stored value present, in this order:
 *     1. owner given and != stored o    MMP_VWC_OWNER_MISMATCH (:181, :222)
 *     2. id_b given, != stored tmid, and id_a != stored tmid       MMP_VWC_PRECONDITION (:184, :232)
 *     3. id_a == stored tmid and == stored amid                     MMP_VWC_UNCHANGED (:243)
 *     4. id_a == stored tmid and no MMP_VWQ_FORCE                   MMP_VWC_UNCHANGED, target_copy_count from the previous active
 *                                       model when that id is not null (:246-250), looked up as in 5
 *     5. otherwise tmid := id_a where it differed, and dec[0] = the previous target when it is not null and differs from the
 *        previous active id (:237-239).  When id_a != stored amid: a null previous active gives amid := id_a (:258); else the
 *        previous active id is looked up in the model-id table and target_copy_count = the resident row's n_loaded (unresolved
 *        entries included, as in mmp_vmodels_transitions), 0 for an unknown id or the empty row, which sets
 *        MMP_VWF_PREV_ACTIVE_UNKNOWN.  The active model switches — amid := id_a, dec[1] = the previous active id,
 *        MMP_VWF_ACTIVE_SWITCHED — under MMP_VWQ_FORCE, or at a count of 0, or at a count of 1 with MMP_VWQ_TARGET_EXISTS and
 *        MMP_VWQ_TARGET_LOADED (:262-270).  At a count of 1 with TARGET_EXISTS, without FORCE and with neither status flag the class
 *        is MMP_VWC_NEEDS_TARGET_STATUS: nothing is rendered, target_copy_count is 1; the host asks getStatus(target) and calls
 *        again with the answer, as MMP_VMR_STRONG_READ works.  Then failed := false (:273), class MMP_VWC_UPDATED
 *   request flags: MMP_VWQ_TARGET_EXISTS = the host holds a stored value for the target (targetModel != null, :264);
 *   MMP_VWQ_TARGET_LOADED / _NOT_LOADED = the answer to getStatus(target) == LOADED (both: MMP_EINVAL).
 *   last_used (CREATED / UPDATED, :299-300; the host passes it to the INC of mmp_models_refs_json) = the previous active row's
 *   last_used where step 5 looked that row up, it is known and > 0; otherwise now_ms - age * (LOAD_NOW ? 1 : 6) in Java long
 *   arithmetic (:168-170).  model (CREATED / UPDATED / UNCHANGED / NEEDS_TARGET_STATUS) = the registry row of id_a, -1 unknown.
 * MMP_VW_DELETE (:416-470): owner = span 2.  No stored value, or an owner given that != stored o: MMP_VWC_NOOP (:419, :457).
 *   Otherwise MMP_VWC_DELETE: dec[0] = the active id when not null (:438), dec[1] = the target id when it is not null and not equal
 *   to the active one (:441).  Nothing is rendered: the host deletes with the old value.
 * MMP_VW_COMPLETE (:750-766): id_a = toId (empty: MMP_EINVAL), id_b = fromId.  No stored value, stored amid != id_b or stored tmid !=
 *   id_a: MMP_VWC_CHANGED (:762-764; the first attempt, with origVmr, satisfies the guard by construction).  Otherwise amid := id_a,
 *   failed := false, dec[0] = the stored amid, class MMP_VWC_UPDATED.  An empty id_b matches only a stored null amid — where the
 *   Java would throw at :762 — and then names no dec.
 * MMP_VW_FAIL_FLAG (:725-742): MMP_VWQ_FAILED is the new value.  No stored value: MMP_VWC_NOOP; equal to the stored flag:
 *   MMP_VWC_UNCHANGED; otherwise MMP_VWC_UPDATED with failed set.
 * MMP_VWF_IN_TRANSITION (UPDATED / UNCHANGED): !Objects.equals(amid, tmid) of the record as it stands after the step, for
 *   UNCHANGED as stored (:344).
 * dec: dec_off[k] / dec_len[k] name the id as a span of raw bytes INSIDE old value i (dec_len -1: none, dec_off then 0), so the
 * host needs no parse to key the transaction; dec_model[k] = its registry row, -1 unknown.  Every field a class does not define is
 * 0, the three row numbers -1, dec_len -1.
 *
 * Output and sizing as mmp_models_rewrite_json: value i = out_buf[out_off[i], out_off[i+1]); out_off (n + 1 words), rows_out and
 * *n_bytes_out are always complete; NO byte of out_buf is written when out_buf is NULL or out_cap is smaller than the total, and the
 * call still returns MMP_OK.  Read-only: no commit; locking as mmp_vmodels_resolve.  n == 0 is valid.  MMP_EINVAL with every output
 * untouched: an unknown op or flag bits, a NULL required buffer, non-monotone offsets of either kind, now_ms <= 0,
 * lastused_age_on_add_ms < 0, flags != 0, out_cap < 0, default_owner_len < 0, a value of 2^30 bytes or more, an empty id_a on SET /
 * COMPLETE, both status flags.  MMP_ESTATE under the conditions of mmp_model_ids_resolve.  Two runs over the same state are
 * byte-identical. */
typedef struct {
    uint32_t op;    /* MMP_VW_* */
    uint32_t flags; /* MMP_VWQ_* */
} mmp_vmodel_write_req;              /* 8 bytes */
typedef struct {
    int32_t cls;               /* MMP_VWC_* */
    uint32_t flags;            /* MMP_VWF_* */
    int32_t model;             /* SET: the registry row of id_a, -1 unknown */
    int32_t target_copy_count; /* SET: loaded copies of the previous active model (:248, :261) */
    int32_t dec_model[2];      /* the registry rows of the ids that lose a referent, -1 unknown or none */
    int32_t dec_off[2];        /* ... and the ids as spans of old value i */
    int32_t dec_len[2];        /* -1: none */
    int64_t last_used;         /* SET, CREATED / UPDATED: newLastUsedTime (:299-300) */
} mmp_vmodel_write_row;              /* 48 bytes */
#define MMP_VW_SET 0                 /* updateVModel */
#define MMP_VW_DELETE 1              /* deleteVModel */
#define MMP_VW_COMPLETE 2            /* the tail of PendingTransition.run */
#define MMP_VW_FAIL_FLAG 3           /* setTargetLoadFailed (:736-738) */
/* request flags */
#define MMP_VWQ_UPDATE_ONLY 1u
#define MMP_VWQ_FORCE 2u
#define MMP_VWQ_LOAD_NOW 4u
#define MMP_VWQ_TARGET_EXISTS 8u
#define MMP_VWQ_TARGET_LOADED 16u
#define MMP_VWQ_TARGET_NOT_LOADED 32u
#define MMP_VWQ_FAILED 64u           /* FAIL_FLAG: the new value */
/* cls */
#define MMP_VWC_CREATED 0            /* the new record is rendered */
#define MMP_VWC_UPDATED 1            /* the next record is rendered */
#define MMP_VWC_UNCHANGED 2          /* no record updates needed */
#define MMP_VWC_NOT_FOUND 3          /* updateOnly and no vmodel */
#define MMP_VWC_PRECONDITION 4       /* FAILED_PRECONDITION */
#define MMP_VWC_OWNER_MISMATCH 5     /* ALREADY_EXISTS with a different owner */
#define MMP_VWC_NEEDS_TARGET_STATUS 6 /* call again with MMP_VWQ_TARGET_LOADED or _NOT_LOADED */
#define MMP_VWC_NOOP 7               /* nothing to do: absent, or another owner's */
#define MMP_VWC_DELETE 8             /* delete with the old value */
#define MMP_VWC_CHANGED 9            /* COMPLETE: things changed, give up */
#define MMP_VWC_MALFORMED 10         /* the old value is malformed */
#define MMP_VWC_HOST 11              /* well-formed, but the host decides this one */
/* row flags */
#define MMP_VWF_IN_TRANSITION 1u
#define MMP_VWF_ACTIVE_SWITCHED 2u
#define MMP_VWF_PREV_ACTIVE_UNKNOWN 4u
int mmp_vmodels_write_json(mmp_ctx *ctx, const mmp_vmodel_write_req *reqs, int32_t n, const char *strs, const int32_t *str_off,
                           const char *default_owner, int32_t default_owner_len, const char *old_buf, const int64_t *old_off,
                           int64_t now_ms, int64_t lastused_age_on_add_ms, uint32_t flags, char *out_buf, int64_t out_cap,
                           int64_t *out_off, mmp_vmodel_write_row *rows_out, int64_t *n_bytes_out);
/* Read the staged instance table / the loaded registry view back (tests, diagnostics). */
int mmp_pods_get(mmp_ctx *ctx, mmp_pod_row *rows_out, int32_t max_rows, int32_t *n_out);
int mmp_models_get(mmp_ctx *ctx, mmp_model_row *rows_out, int32_t max_models, int32_t *ent_pod_out, int64_t *ent_time_out,
                   int32_t max_entries, int32_t *n_models_out, int32_t *n_entries_out);

/* ---- pod-axis sharding across the GPUs of one node ---------------------------
 * There is no reference counterpart: the reference walks clusterState (MM.java:4763) on one JVM
 * thread.  Here shard g of G owns a contiguous range of PLACEMENT_ORDER positions (the words
 * [g*ceil(W/G), ...) of every rank-ordered bitmap and column); every shard sees the whole request
 * batch, and one CacheMissForwardingLB.getNext (MM.java:4776-5005) is evaluated as six local scans
 * with an all-reduce of a small per-decision int64 vector after each (MIN, except phase 5 = SUM).
 * The library launches the kernels; the HOST performs the collectives between phases (RCCL
 * all-reduce over xGMI: modelmesh_amd/dist.py does it with torch.distributed; a Java host would
 * call ncclAllReduce on the same device buffers).  Results are bit-identical to mmp_place_batch.
 *
 *   mmp_shard_configure(ctx, g, G)        once, before the first commit (G = 1 is allowed)
 *   commit:  mmp_shard_rank_dev(ctx, d_rank)   -> all-reduce SUM of int32 d_rank[n_pods]
 *            mmp_shard_commit_dev(ctx, d_rank)     (both synchronise the context's stream)
 *   batch:   for phase in 1..6: mmp_shard_place_phase_dev(...); all-reduce d_xchg[phase-1]
 *            mmp_shard_place_phase_dev(phase 7) writes d_outs on every shard
 * d_xchg[k] (k = 0..5) are device int64 buffers of n * mmp_shard_xchg_slots(k+1, G) elements. */
int mmp_shard_configure(mmp_ctx *ctx, int32_t shard, int32_t n_shards);
int32_t mmp_shard_xchg_slots(int32_t phase, int32_t n_shards);
int32_t mmp_shard_xchg_is_sum(int32_t phase); /* 1: SUM, 0: MIN */
/* PLACEMENT_ORDER ranks (MM.java:4646-4703) of this shard's slice of the pod table against all
 * pods; other entries of d_rank (device int32[n_pods]) are zeroed. */
int mmp_shard_rank_dev(mmp_ctx *ctx, void *d_rank);
int mmp_shard_commit_dev(mmp_ctx *ctx, const void *d_rank);
int mmp_shard_place_phase_dev(mmp_ctx *ctx, int32_t phase, const void *d_reqs, int32_t n, const void *d_extra_pool,
                              int64_t now_ms, void *const *d_xchg, void *d_outs, void *stream);

/* The speculative single-exchange form in front of the phases above (csrc/shard_kernels.hpp).  The head of
 * PLACEMENT_ORDER decides almost every request, so each shard first runs the complete lane-per-decision
 * getNext on its own slice and publishes, per decision, mmp_shard_fast_slots() int64 words: INT64_MAX = "no
 * eligible pod in my slice", otherwise its result keyed by the shard number, with an "incomplete" bit when
 * the shortlist runs off the end of the slice or the decision needs the general path.  After ONE
 * all-reduce(MIN) of d_xf[n * slots] the lowest shard holding an eligible pod has won every slot:
 *
 *   mmp_shard_place_fast_dev(ctx, d_reqs, n, d_extra, now, d_xf, stream)        -> all-reduce MIN d_xf
 *   mmp_shard_place_fast_finish_dev(..., &n_rest, &d_rest_reqs, &d_rest_outs)      writes the decided rows of
 *        d_outs, counts the undecided requests (the count reaches the host in pinned memory; `stream` is
 *        synchronised) and, only when there are any, compacts them (same order on every shard) into
 *        library-owned device buffers
 *   if n_rest: phases 1..7 of mmp_shard_place_phase_dev on (d_rest_reqs, n_rest, d_rest_outs), then
 *        mmp_shard_place_fast_scatter_dev(ctx, n_rest, d_outs, stream)             rows back into d_outs
 *
 * One batch in flight per shard context (the rest buffers belong to the context).  Results are
 * bit-identical to mmp_place_batch. */
int32_t mmp_shard_fast_slots(void);
int mmp_shard_place_fast_dev(mmp_ctx *ctx, const void *d_reqs, int32_t n, const void *d_extra_pool, int64_t now_ms,
                             void *d_xf, void *stream);
int mmp_shard_place_fast_finish_dev(mmp_ctx *ctx, const void *d_reqs, int32_t n, const void *d_xf, void *d_outs,
                                    void *stream, int32_t *n_rest_out, void **d_rest_reqs_out, void **d_rest_outs_out);
int mmp_shard_place_fast_scatter_dev(mmp_ctx *ctx, int32_t n_rest, void *d_outs, void *stream);

/* ---- the pod-axis group with RCCL inside the boundary (north star: "the pod axis shards naturally across the 8
 * GPUs of one node with an RCCL allreduce over xGMI of per-shard best-candidate scores") -------------------------
 * One context per GPU (one process per GPU, or one thread per context).  The calls above leave the collectives to
 * the host (a torch.distributed process group in modelmesh_amd/dist.py); the calls below run them themselves, on
 * the context's own stream, through librccl (bound at run time), so that a host that holds no RCCL handles — the
 * Java mesh — reaches the multi-GPU layout through host pointers alone:
 *   rank 0:      mmp_shard_unique_id(id)                     128 bytes, handed to the other ranks out of band
 *                                                            (the mesh's KV store, litelinks, a file ...)
 *   every rank:  mmp_shard_group_init(ctx, id, rank, world)  ncclCommInitRank + mmp_shard_configure(rank, world)
 *                load the instance table / types / registry as for an unsharded context
 *                mmp_shard_commit(ctx)                       collective: rank slice -> ncclAllReduce(SUM) -> scatter
 *                mmp_shard_place_batch(ctx, reqs, n, ...)    collective: every rank passes the SAME batch and gets
 *                                                            the same result rows (bit-identical to mmp_place_batch)
 * A batch is: place_shard_fast_kernel (the slice's head windows + resolved registry rows, as the unsharded kernel) ->
 * ncclAllReduce(MIN, 2 int64 per decision) -> decided rows + the COUNT of the undecided rest, which the host reads
 * (identical on every shard: the words are the reduced ones) -> only when it is not zero: compaction, the six exchange
 * phases (5 x MIN, 1 x SUM) over exactly those rows, scatter (*n_rest_out = how many took the six phases).  (Round 2
 * kept the count on the device and always ran the six phases over a fixed-capacity sub-batch: seven launches and six
 * collectives per batch that mostly found no rows.)  unique_id may be NULL for world == 1: a group of one shard
 * without a communicator (no RCCL needed). */
#define MMP_SHARD_UNIQUE_ID_BYTES 128
/* mmp_shard_place_batch_async_dev: the same batch WITHOUT the host synchronisation at its end — the fast kernel, the
 * all-reduce and the finish kernel are enqueued on the context's stream and the call returns.  The batch is completed (its
 * rest count read, the six phases run if there is a rest) by the NEXT group call on the context — another batch, a commit —
 * or by mmp_shard_wait, which also returns the rest count.  Until then d_reqs / d_extra_pool / d_outs must stay valid and
 * d_outs must not be read: its rows are defined only once mmp_shard_wait (or a synchronous group call) has returned — those
 * synchronise the context's stream; the rest count the library polls in between carries no ordering for the rows.  Every shard of the group must issue the same sequence of calls.  (One shard, 100k decisions:
 * 26 us per batch with the synchronisation, 14 us without: the device's own time.  The exchange words, flags and count of a
 * batch live in one of two slots, so the batch before is completed AFTER this one has been enqueued.) */
int mmp_shard_unique_id(void *id_out);
/* A host that moves the exchange words itself (another transport than RCCL; several shards driven from one process)
 * installs a callback BEFORE mmp_shard_group_init and passes unique_id = NULL there.  The callback must all-reduce
 * `count` elements at device pointer `dev_buf` in place across the group — elem64: 0 = int32, 1 = int64; op_min:
 * 0 = SUM, 1 = MIN — ordered after everything already queued on `stream` (the context's hipStream_t), and return 0. */
typedef int (*mmp_exchange_fn)(void *user, void *dev_buf, int64_t count, int32_t elem64, int32_t op_min, void *stream);
int mmp_shard_group_set_exchange(mmp_ctx *ctx, mmp_exchange_fn fn, void *user);
int mmp_shard_group_init(mmp_ctx *ctx, const void *unique_id, int32_t rank, int32_t world);
int mmp_shard_group_destroy(mmp_ctx *ctx);
int mmp_shard_commit(mmp_ctx *ctx);
int mmp_shard_place_batch(mmp_ctx *ctx, const mmp_place_req *reqs, int32_t n, const int32_t *extra_pool,
                          int32_t n_extra_pool, int64_t now_ms, mmp_place_out *outs, int32_t *n_rest_out);
int mmp_shard_place_batch_dev(mmp_ctx *ctx, const void *d_reqs, int32_t n, const void *d_extra_pool, int64_t now_ms,
                              void *d_outs, int32_t *n_rest_out);
int mmp_shard_place_batch_async_dev(mmp_ctx *ctx, const void *d_reqs, int32_t n, const void *d_extra_pool, int64_t now_ms,
                                    void *d_outs);
int mmp_shard_wait(mmp_ctx *ctx, int32_t *n_rest_out);

/* Wait for everything queued on the context's own stream. */
int mmp_sync(mmp_ctx *ctx);

/* Operator metrics (the role of ModelMesh's Metrics timers around these decisions, Metrics.java):
 * with profiling enabled every host-pointer entry point brackets its kernels (not its staging copies)
 * with HIP events on the context's stream; mmp_last_kernel_ms returns the device time of the most
 * recent such call, or a negative value if none was recorded. */
int mmp_profile(mmp_ctx *ctx, int enable);
double mmp_last_kernel_ms(mmp_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* MMPLACE_H */
