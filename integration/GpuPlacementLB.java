/*
 * GpuPlacementLB.java — the reference-side binding a ModelMesh maintainer adds.
 * Lives in package com.ibm.watson.modelmesh next to ModelMesh.java.  The two litelinks clients are built at
 * ModelMesh.java:1103-1110; the patch replaces the two LoadBalancer factories there:
 *
 *     runtimeClient   = ... .withLoadBalancer(gpu ? () -> new GpuForwardingLB(binding)  : ForwardingLB::new) ...
 *     cacheMissClient = ... .withLoadBalancer(gpu ? () -> new GpuCacheMissLB(binding)   : CacheMissForwardingLB::new) ...
 *
 * or, to PIN the solver against the reference on live traffic before switching (INTEGRATION.md §4):
 *
 *     ... .withLoadBalancer(() -> new ShadowCacheMissLB(new CacheMissForwardingLB(), new GpuCacheMissLB(binding), binding))
 *     ... .withLoadBalancer(() -> new ShadowForwardingLB(new ForwardingLB(), new GpuForwardingLB(binding), binding))
 *
 * This repository's image has no JDK, so nothing here is compiled in CI; tests/test_jni_veneer.py checks the
 * `native` declarations against integration/mmplace_jni.cc (names, arity, types) and against include/mmplace.h.
 * Everything the classes need from the enclosing ModelMesh instance goes through GpuMeshBinding, which the
 * patch implements as an inner class of ModelMesh (it reads instanceId, clusterState, registry, the two
 * ThreadLocals and the litelinks ServiceInstance counters).
 */
package com.ibm.watson.modelmesh;

import java.nio.ByteBuffer;
import java.nio.ByteOrder;
import java.util.Collection;
import java.util.HashSet;
import java.util.Map;
import java.util.Set;
import java.util.concurrent.ThreadLocalRandom;
import java.util.concurrent.atomic.AtomicLong;

import com.ibm.watson.litelinks.ThreadContext;
import com.ibm.watson.litelinks.client.LoadBalancer;
import com.ibm.watson.litelinks.client.ServiceInstance;
import com.ibm.watson.litelinks.client.ServiceInstanceInfo;

/** static natives implemented by integration/mmplace_jni.cc */
final class MmPlace {
    static { System.loadLibrary("mmplace_jni"); }
    static native long create(int device, long minSpaceUnits, long minChurnAgeMs);
    static native void destroy(long h);
    static native int podsLoad(long h, ByteBuffer rows, int n);
    static native int podsUpsert(long h, ByteBuffer idx, ByteBuffer rows, int n);
    static native int podsRemove(long h, ByteBuffer idx, int n);
    static native int typesLoad(long h, int nTypes, ByteBuffer allowed, ByteBuffer prefer,
                                ByteBuffer hasAllowed, ByteBuffer hasPrefer);
    static native int replacedReplicaSetsLoad(long h, ByteBuffer rs, int n);
    static native int modelsLoad(long h, ByteBuffer rows, int nModels, ByteBuffer entPod, ByteBuffer entTime, int nEntries);
    static native int modelsUpsert(long h, ByteBuffer idx, ByteBuffer rows, int n, ByteBuffer entPod, ByteBuffer entTime, int nEntries);
    static native int commit(long h);
    static native int placeBatch(long h, ByteBuffer reqs, int n, ByteBuffer extraPool, int nExtra, long nowMs, ByteBuffer outs);
    /** the single-caller form: caller = one mmp_place_caller (this instance's index, favourSelf, getFreshInstanceRecord()),
     *  reqs = n mmp_place_req_c rows of 24 bytes {model, pick, lastUsedTime, extraOff, nExtra} — what the rate task, the janitor,
     *  the reaper and preShutdown issue: every decision of such a batch has the same self */
    static native int placeBatchCaller(long h, ByteBuffer caller, ByteBuffer reqs, int n, ByteBuffer extraPool, int nExtra,
                                       long nowMs, ByteBuffer outs);
    static native int serveBatch(long h, ByteBuffer reqs, int n, ByteBuffer counters, int nCounters,
                                 ByteBuffer exclPod, ByteBuffer exclTime, int nExcl, long nowMs, ByteBuffer outs);
    /** keep one wavefront resident that serves placeBatch(n = 1) from 64 pinned request slots: no launch per request */
    static native int resident(long h, boolean enable);
    // the pod-axis group: several GPUs of one node, RCCL runs inside libmmplace (include/mmplace.h)
    static native int shardUniqueId(ByteBuffer idOut);
    static native int shardGroupInit(long h, ByteBuffer id, int rank, int world);
    static native int shardGroupDestroy(long h);
    static native int shardCommit(long h);
    static native int shardPlaceBatch(long h, ByteBuffer reqs, int n, ByteBuffer extraPool, int nExtra, long nowMs,
                                      ByteBuffer outs, ByteBuffer nRestOut);
    static native int clusterStats(long h, ByteBuffer out);
    static native int typeStats(long h, int type, ByteBuffer out);
    static native int partitionCount(long h, ByteBuffer nOut);
    static native int partitionStats(long h, int partition, ByteBuffer out, ByteBuffer prohibitedOut, int maxWords);
    static native int podPartitions(long h, ByteBuffer partitionOut, int maxPods, ByteBuffer nOut);
    // eviction (clhm) and the unload-buffer manager
    static native int cachesLoad(long h, int nCaches, ByteBuffer segOff, ByteBuffer lastUsed, ByteBuffer weight,
                                 ByteBuffer capacity);
    static native int evictBatch(long h, ByteBuffer reqs, int n, long nowMs, ByteBuffer outs);
    static native int cachesLoadKeyed(long h, int nCaches, ByteBuffer segOff, ByteBuffer lastUsed, ByteBuffer weight,
                                      ByteBuffer key, ByteBuffer capacity, ByteBuffer ubm);
    static native int cacheReplay(long h, ByteBuffer ops, int nOps, long nowMs, ByteBuffer outs, ByteBuffer evictedKeys,
                                  int maxEvicted, ByteBuffer nEvictedSlots);
    static native int cacheRead(long h, int cache, int maxEntries, ByteBuffer lastUsed, ByteBuffer weight, ByteBuffer key,
                                ByteBuffer scalars, ByteBuffer ubm);
    // the caches by model id (mmp_caches_load_keyed_k ...): the key of an entry is the registry row its id names, resolved on the
    // device; what a replay evicts comes back as ids.  A thin pass-through: no Java site is moved onto these calls yet.
    // cacheReplayK sizes = {nEvictedSlots, nIdBytes}; cacheEvictedIds sizes = {nSlots, nBytes}; cacheReadK scalars = {int n, int
    // nIdBytes, long capacity, long weightedSize}.
    static native int cachesLoadKeyedK(long h, int nCaches, ByteBuffer segOff, ByteBuffer lastUsed, ByteBuffer weight, ByteBuffer keys,
                                       ByteBuffer keyOff, ByteBuffer isUnloadbuf, ByteBuffer capacity, ByteBuffer ubm,
                                       ByteBuffer keyRowOut);
    static native int cacheReplayK(long h, ByteBuffer ops, int nOps, ByteBuffer keys, ByteBuffer keyOff, long nowMs,
                                   ByteBuffer keyStatusOut, ByteBuffer keyRowOut, ByteBuffer outs, ByteBuffer evictedRows,
                                   int maxEvicted, ByteBuffer evIdBytesOut, int maxIdBytes, ByteBuffer evIdOffOut, ByteBuffer sizes);
    static native int cacheEvictedIds(long h, ByteBuffer bytesOut, int maxBytes, ByteBuffer offOut, ByteBuffer sizes);
    // cacheReplayK with each victim's lastUsed beside its id (the value the clhm hands onEviction): evLastUsedOut = maxEvicted longs, or
    // null — cacheEvictedTimes(out, maxSlots, nSlotsOut) reads them from the context (sizes then list; an error when the last replay
    // recorded none)
    static native int cacheReplayKT(long h, ByteBuffer ops, int nOps, ByteBuffer keys, ByteBuffer keyOff, long nowMs,
                                    ByteBuffer keyStatusOut, ByteBuffer keyRowOut, ByteBuffer outs, ByteBuffer evictedRows,
                                    int maxEvicted, ByteBuffer evIdBytesOut, int maxIdBytes, ByteBuffer evIdOffOut, ByteBuffer sizes,
                                    ByteBuffer evLastUsedOut);
    static native int cacheEvictedTimes(long h, ByteBuffer out, int maxSlots, ByteBuffer nSlotsOut);
    static native int cacheReadK(long h, int cache, int maxEntries, ByteBuffer lastUsed, ByteBuffer weight, ByteBuffer rowOut,
                                 ByteBuffer idBytesOut, int maxIdBytes, ByteBuffer idOffOut, ByteBuffer scalars, ByteBuffer ubm);
    // request guards and rebalancer plans
    static native int gateBatch(long h, ByteBuffer reqs, int n, ByteBuffer exclPod, ByteBuffer exclTime, int nExcl,
                                ByteBuffer explicitPool, int nExplicit, long nowMs, long inUseFailureExpiryMs,
                                ByteBuffer outs);
    static native int missBatch(long h, ByteBuffer gateReqs, ByteBuffer placeReqs, int n, ByteBuffer exclPod, ByteBuffer exclTime, int nExcl,
                                ByteBuffer explicitPool, int nExplicit, ByteBuffer extraPool, int nExtra, long nowMs,
                                long inUseFailureExpiryMs, ByteBuffer gateOuts, ByteBuffer placeOuts);
    static native int routeBatch(long h, ByteBuffer gateReqs, ByteBuffer serveReqs, int n, ByteBuffer counters, int nCounters,
                                 ByteBuffer exclPod, ByteBuffer exclTime, int nExcl, ByteBuffer explicitPool, int nExplicit,
                                 long nowMs, long inUseFailureExpiryMs, ByteBuffer gateOuts, ByteBuffer serveOuts);
    /** the single-caller forms of the two routes: caller = one mmp_seam_caller (112 bytes: this instance's index, the flags every
     *  request of the batch shares, loadingCount and its cutoff, runtimeCache capacity / weightedSize / oldestTime, loadTimeoutMs,
     *  getFreshInstanceRecord(), lastPublished, localInvokesInFlight, lastInvokeTime), filled ONCE per batch; gateReqs = n
     *  mmp_gate_req_c rows of 48 bytes, serveReqs = n mmp_serve_req_c rows of 24 bytes, placeReqs = n mmp_place_req_c rows.  A batch
     *  is what one instance's request threads hand over together. */
    static native int routeBatchCaller(long h, ByteBuffer caller, ByteBuffer gateReqs, ByteBuffer serveReqs, int n, ByteBuffer counters,
                                       int nCounters, ByteBuffer exclPod, ByteBuffer exclTime, int nExcl, ByteBuffer explicitPool,
                                       int nExplicit, long nowMs, long inUseFailureExpiryMs, ByteBuffer gateOuts, ByteBuffer serveOuts);
    static native int missBatchCaller(long h, ByteBuffer caller, ByteBuffer placeCaller, ByteBuffer gateReqs, ByteBuffer placeReqs, int n,
                                      ByteBuffer exclPod, ByteBuffer exclTime, int nExcl, ByteBuffer explicitPool, int nExplicit,
                                      ByteBuffer extraPool, int nExtra, long nowMs, long inUseFailureExpiryMs, ByteBuffer gateOuts,
                                      ByteBuffer placeOuts);
    /** the single-caller forms BY MODEL ID (mmp_place_batch_ck / _route_batch_ck / _miss_batch_ck): request i names its model by
     *  keys[keyOff[i], keyOff[i + 1]) — the model id's UTF-8 bytes, keyOff = n + 1 ints — and the library resolves it on the device
     *  inside the call (one latency slot, one wait, no batch lock: no modelIdsResolve in front).  The rows' model field is ignored;
     *  modelIdxOut (n ints, may be null) receives the row of each key, -1 for an unknown id. */
    static native int placeBatchKeyed(long h, ByteBuffer caller, ByteBuffer reqs, int n, ByteBuffer keys, ByteBuffer keyOff,
                                      ByteBuffer extraPool, int nExtra, long nowMs, ByteBuffer outs, ByteBuffer modelIdxOut);
    static native int routeBatchKeyed(long h, ByteBuffer caller, ByteBuffer gateReqs, ByteBuffer serveReqs, int n, ByteBuffer keys,
                                      ByteBuffer keyOff, ByteBuffer counters, int nCounters, ByteBuffer exclPod, ByteBuffer exclTime,
                                      int nExcl, ByteBuffer explicitPool, int nExplicit, long nowMs, long inUseFailureExpiryMs,
                                      ByteBuffer gateOuts, ByteBuffer serveOuts, ByteBuffer modelIdxOut);
    static native int missBatchKeyed(long h, ByteBuffer caller, ByteBuffer placeCaller, ByteBuffer gateReqs, ByteBuffer placeReqs, int n,
                                     ByteBuffer keys, ByteBuffer keyOff, ByteBuffer exclPod, ByteBuffer exclTime, int nExcl,
                                     ByteBuffer explicitPool, int nExplicit, ByteBuffer extraPool, int nExtra, long nowMs,
                                     long inUseFailureExpiryMs, ByteBuffer gateOuts, ByteBuffer placeOuts, ByteBuffer modelIdxOut);
    /** the single-caller forms BY VMODEL ID (mmp_place_batch_cv / _route_batch_cv / _miss_batch_cv): keys name VMODELS, and
     *  resolveVModelId (VModelManager.java:569-597) runs on the device inside the call — no vmodelsResolve (a staged call under the
     *  batch lock) in front.  nfKeys / nfOff (both may be null): the notFoundModelId spans, an empty span is null; reqFlags (n ints,
     *  may be null): 1 = the question is asked again after vModels.getStrong.  vmOut (n rows of 24 bytes, may be null): int cls (0 not
     *  found / 1 ok / 2 strong read wanted / 3 target not found / 4 the host decides), int which (0 active / 1 target), int vmodel,
     *  int model, int flags (1 = the answered id is null), int reserved.  The decision is the one for vmOut.model when cls is 1 and
     *  flags is 0, and the one for "no such model" otherwise: READ cls BEFORE BELIEVING THE DECISION (VModelCall below). */
    static native int placeBatchVKeyed(long h, ByteBuffer caller, ByteBuffer reqs, int n, ByteBuffer keys, ByteBuffer keyOff,
                                       ByteBuffer nfKeys, ByteBuffer nfOff, ByteBuffer reqFlags, ByteBuffer extraPool, int nExtra,
                                       long nowMs, ByteBuffer outs, ByteBuffer vmOut);
    static native int routeBatchVKeyed(long h, ByteBuffer caller, ByteBuffer gateReqs, ByteBuffer serveReqs, int n, ByteBuffer keys,
                                       ByteBuffer keyOff, ByteBuffer nfKeys, ByteBuffer nfOff, ByteBuffer reqFlags, ByteBuffer counters,
                                       int nCounters, ByteBuffer exclPod, ByteBuffer exclTime, int nExcl, ByteBuffer explicitPool,
                                       int nExplicit, long nowMs, long inUseFailureExpiryMs, ByteBuffer gateOuts, ByteBuffer serveOuts,
                                       ByteBuffer vmOut);
    static native int missBatchVKeyed(long h, ByteBuffer caller, ByteBuffer placeCaller, ByteBuffer gateReqs, ByteBuffer placeReqs, int n,
                                      ByteBuffer keys, ByteBuffer keyOff, ByteBuffer nfKeys, ByteBuffer nfOff, ByteBuffer reqFlags,
                                      ByteBuffer exclPod, ByteBuffer exclTime, int nExcl, ByteBuffer explicitPool, int nExplicit,
                                      ByteBuffer extraPool, int nExtra, long nowMs, long inUseFailureExpiryMs, ByteBuffer gateOuts,
                                      ByteBuffer placeOuts, ByteBuffer vmOut);
    static native int proactivePlan(long h, int defaultModelSizeUnits, long nowMs, int maxOut, ByteBuffer outModel,
                                    ByteBuffer outLastUsed, ByteBuffer info);
    static native int proactivePlanSubset(long h, int partition, ByteBuffer skipModels, int nSkip, int defaultModelSizeUnits,
                                          long nowMs, int maxOut, ByteBuffer outModel, ByteBuffer outLastUsed, ByteBuffer info);
    // pruneModelRegistry (MM.java:6524-6609) before the plan above: flags 1 = apply to the resident registry, 2 = dry run; editsOut =
    // mmp_prune_edit rows (32 bytes: what goes to registry.conditionalSetAndGet), removedOut = mmp_prune_removed rows (16 bytes),
    // info = one mmp_prune_info; info.truncated: nothing was applied, repeat with larger buffers.  registryMissingReset is
    // missings.clear() on a leader change (MM.java:6827).
    static native int registryPrune(long h, int selfPod, long nowMs, long goneAfterMs, long lastUsedAgeOnAddMs, int flags,
                                    ByteBuffer editsOut, int maxEdits, ByteBuffer removedOut, int maxRemoved, ByteBuffer info);
    static native int registryMissingGet(long h, ByteBuffer sinceOut, int maxPods, ByteBuffer nOut);
    static native int registryMissingReset(long h);
    // loadedModelCount / failedModelCount / registry.getCount() (event(), MM.java:2828-2852; logModelCountMetrics, :6852-6863) over the
    // resident registry, after registryPrune / janitorPlan have rewritten it: statsOut = one mmp_registry_stats (72 bytes: n_models,
    // n_loaded, n_failed at offsets 0, 4, 8); podLoadedOut / podFailedOut = one int per pod slot (hasRegistration, :2856-2858, summed
    // over the records), typesOut = mmp_registry_type_stats rows (24 bytes); nPodsOut / nTypesOut = the table sizes, always set.
    // Buffers may be null with a capacity of 0.
    static native int registryCensus(long h, ByteBuffer statsOut, ByteBuffer podLoadedOut, ByteBuffer podFailedOut, int maxPods,
                                     ByteBuffer nPodsOut, ByteBuffer typesOut, int maxTypes, ByteBuffer nTypesOut);
    // janitorTask's cache loop and registry loop (MM.java:5892-6008, :6014-6108) for this instance: entries = mmp_janitor_entry rows
    // (80 bytes, runtimeCache.descendingMap() order without the unload-buffer entry), params = one mmp_janitor_params; flags 1 =
    // apply to the resident registry, 2 = dry run.  actionsOut = one byte per row (4 / 6: ce.remove()), editsOut = mmp_janitor_edit
    // rows (48 bytes: what goes to registry.conditionalSetAndGet), candidatesOut = scaleCopiesCandidates oldest first as
    // mmp_cache_entry rows for scaledownPlan, candidateRowsOut their input rows; info.truncated: nothing was applied.
    static native int janitorPlan(long h, ByteBuffer entries, int n, ByteBuffer params, int flags, ByteBuffer actionsOut,
                                  ByteBuffer editsOut, int maxEdits, ByteBuffer candidatesOut, ByteBuffer candidateRowsOut,
                                  int maxCandidates, ByteBuffer info);
    // the edits this instance makes to ModelRecords itself: ops = mmp_registry_op rows (40 bytes: model, pod, op, flags, lastUsed,
    // loadTime, loadCompleteTime); op 0 = loadLocal's put (MM.java:5204-5207), 1 = the load-failure path (:2484-2495; flag 1 =
    // shuttingDown), 2 = deregisterModel (:2948-2958; flag 2 = loadTime != null), 3 = removeLocalModelCopyAsync (:6347-6365, sent
    // after isLoadedElsewhere).  flags 1 = apply to the resident registry, 2 = dry run.  statusOut = one byte per op (1: the record
    // changed and goes to registry.conditionalSetAndGet), editsOut = mmp_registry_op_edit rows (40 bytes) in op order, info = one
    // mmp_registry_ops_info (56 bytes); info.truncated: nothing was applied.
    static native int registryOps(long h, ByteBuffer ops, int n, long nowMs, int flags, ByteBuffer statusOut, ByteBuffer editsOut,
                                  int maxEdits, ByteBuffer info);
    // the same BY MODEL ID (mmp_registry_ops_k): keys / keyOff name the record of op i (the op's model field is ignored; both null:
    // by row), resolved, evaluated and applied under ONE hold of the batch lock — no event batch or modelsRetire can land between
    // the row and its edit.  op 4 = the cache-hit loop dropping its own copy (:3682-3687; always an edit, no lastUnloadTime, no
    // flag bit).  statusOut 2 = no record (unknown id, or deleted: registry.get == null, the Java returns); modelIdxOut = n ints (may
    // be null); info = one mmp_registry_ops_info_k (88 bytes: nEdits, nUnchanged, nNoRecord, truncated, int[8] edited per kind,
    // int[8] unchanged per kind, entries added, entries removed).
    static native int registryOpsKeyed(long h, ByteBuffer ops, int n, ByteBuffer keys, ByteBuffer keyOff, long nowMs, int flags,
                                       ByteBuffer modelIdxOut, ByteBuffer statusOut, ByteBuffer editsOut, int maxEdits, ByteBuffer info);
    // onEviction's task body (MM.java:2886-2920) by model id: entries = mmp_evicted_entry rows (32 bytes: lastUsed, loadTimestamp,
    // loadCompleteTimestamp, int weight, int flags 1 = ce.isFailed()), params = {int selfPod, int 0, long now, long loadTimeoutMs},
    // outs = mmp_evicted_out rows (24 bytes: int flags 1 in registry / 2 attempt reload / 4 reload / 8 log, int status, long
    // loadedTime or -1, long millisSinceLastUsed), info = mmp_evictions_info (112 bytes)
    static native int evictionsKeyed(long h, ByteBuffer entries, int n, ByteBuffer keys, ByteBuffer keyOff, ByteBuffer params, int flags,
                                     ByteBuffer modelIdxOut, ByteBuffer outs, ByteBuffer statusOut, ByteBuffer editsOut, int maxEdits,
                                     ByteBuffer info);
    // getStatus (MM.java:3247) from the resident registry: reqs = mmp_status_req rows (16 bytes: model or -1 for mr == null, failPod =
    // the pod of mle.getInstanceId() or -1, flags 1 = the cache-hit loop is exhausted, 0).  rowsOut = mmp_status_row rows (16 bytes:
    // class 0 NOT_FOUND / 1 NOT_LOADED / 2 LOADING_FAILED / 3 ask a copy, copyOff, nNotChecked, nFailed), copiesOut = mmp_status_copy
    // rows (16 bytes: pod, 0 NOT_CHECKED / 1 LOADING_FAILED, time) in makeStatusInfo's sorted order (:3013-3058), request i's at
    // copyOff; nCopiesOut = the total, also when copiesOut (null with maxCopies 0: sizes only) held a prefix.
    static native int modelsStatus(long h, ByteBuffer reqs, int n, long nowMs, ByteBuffer rowsOut, ByteBuffer copiesOut, int maxCopies,
                                   ByteBuffer nCopiesOut);
    static native int scaleupPlan(long h, ByteBuffer entries, int n, ByteBuffer params, ByteBuffer outs,
                                  ByteBuffer overloadedOut, ByteBuffer skipped);
    static native int scaledownPlan(long h, ByteBuffer entries, int n, ByteBuffer params, ByteBuffer removedOut);
    // limitModelConcurrency == true: mmp_conc_entry rows (MaxConcCacheEntry: countAndTimeSum.sum(), priorSum, priorCount, maxConc,
    // queuedRequestCount()) beside the entries; concOuts tell the caller which entries to sumThenReset() and what to store in
    // priorSum / priorCount, result carries the task's averageModelParallelism after the run (a double at offset 0)
    static native int scaleupPlanConc(long h, ByteBuffer entries, ByteBuffer conc, int n, ByteBuffer params, ByteBuffer concParams,
                                      ByteBuffer outs, ByteBuffer concOuts, ByteBuffer overloadedOut, ByteBuffer skipped,
                                      ByteBuffer result);
    static native int scaledownPlanConc(long h, ByteBuffer entries, ByteBuffer conc, int n, ByteBuffer params,
                                        long dynamicRpmScaleConstant, ByteBuffer removedOut);
    static native int migrationPlan(long h, ByteBuffer entries, int n, int selfPod, long nowMs, long cutoffAgeMs,
                                    ByteBuffer actionOut, ByteBuffer waitOut);
    // THE PERIODIC TASKS BY MODEL ID (mmp_scaleup_plan_k, mmp_scaledown_plan_k, mmp_migration_plan_k, mmp_janitor_plan_k): the
    // loops iterate runtimeCache, whose keys are ids (MM.java:5672-5690, :5896-5903, :6998-7010), so keys / keyOff (TaskKeys.of)
    // name the record of entry i — the entry's model field is ignored; both null: by row — and are resolved under the hold of the
    // batch lock that evaluates: no event batch or modelsRetire can land between the row and its use.  An unknown id and a deleted
    // record are model -1 (registry.get == null).  modelIdxOut = n ints (may be null).  conc / concParams / concOuts / result null:
    // limitModelConcurrency == false.
    static native int scaleupPlanKeyed(long h, ByteBuffer entries, ByteBuffer conc, int n, ByteBuffer keys, ByteBuffer keyOff,
                                       ByteBuffer params, ByteBuffer concParams, ByteBuffer outs, ByteBuffer concOuts,
                                       ByteBuffer overloadedOut, ByteBuffer skipped, ByteBuffer result, ByteBuffer modelIdxOut);
    static native int scaledownPlanKeyed(long h, ByteBuffer entries, ByteBuffer conc, int n, ByteBuffer keys, ByteBuffer keyOff,
                                         ByteBuffer params, long dynamicRpmScaleConstant, ByteBuffer removedOut, ByteBuffer modelIdxOut);
    static native int migrationPlanKeyed(long h, ByteBuffer entries, int n, ByteBuffer keys, ByteBuffer keyOff, int selfPod, long nowMs,
                                         long cutoffAgeMs, ByteBuffer actionOut, ByteBuffer waitOut, ByteBuffer modelIdxOut);
    // janitorTask as ONE call (:5876-6145): janitorPlan by id — two entries of one record are refused — and, with scaledown (one
    // mmp_scaledown_params of the same selfPod; flags must be 1 = apply), the scale-down of its candidates in the same hold:
    // conc = n mmp_conc_entry rows in INPUT-row order (null: not latency-based), removedOut = one byte per candidate, aligned with
    // candidatesOut.  info.truncated: nothing was applied and removedOut was not written.
    static native int janitorPlanKeyed(long h, ByteBuffer entries, int n, ByteBuffer keys, ByteBuffer keyOff, ByteBuffer params, int flags,
                                       ByteBuffer scaledown, ByteBuffer conc, long dynamicRpmScaleConstant, ByteBuffer modelIdxOut,
                                       ByteBuffer actionsOut, ByteBuffer editsOut, int maxEdits, ByteBuffer candidatesOut,
                                       ByteBuffer candidateRowsOut, int maxCandidates, ByteBuffer removedOut, ByteBuffer info);
    // type constraints, upgrade tracker
    static native int typesFromLabels(long h, int nTypes, ByteBuffer required, ByteBuffer preferred, ByteBuffer podLabels,
                                      ByteBuffer allowedOut, ByteBuffer preferOut, ByteBuffer hasAllowedOut,
                                      ByteBuffer hasPreferOut);
    static native int upgradeInstanceAdded(long h, long labelsKey, int replicaSet, long startTime, long nowMs);
    static native int upgradeInstanceRemoved(long h, long labelsKey, int replicaSet, long nowMs);
    static native int upgradeHousekeeping(long h, long nowMs);
    static native int upgradeReplaced(long h, ByteBuffer rsOut, ByteBuffer expiryOut, int max, ByteBuffer nOut);
    // KV wire format (the raw values of the KV events)
    static native int podIdsLoad(long h, ByteBuffer ids, ByteBuffer idOff, int nPods, ByteBuffer idOrderOut,
                                 ByteBuffer replicaSetOut);
    static native int podsIngestJson(long h, ByteBuffer json, ByteBuffer off, int n, ByteBuffer podIdx, ByteBuffer live,
                                     ByteBuffer startTimeOut, ByteBuffer statusOut);
    static native int typeNamesLoad(long h, ByteBuffer names, ByteBuffer nameOff, int nTypes, int unknownType);
    static native int modelsIngestJson(long h, ByteBuffer json, ByteBuffer off, int nModels, ByteBuffer lastUnloadOut,
                                       ByteBuffer statusOut);
    /** a batch of registry events as stored: value i for model modelIdx[i]; deleted (may be null) marks ENTRY_DELETED */
    static native int modelsUpsertJson(long h, ByteBuffer json, ByteBuffer off, int n, ByteBuffer modelIdx, ByteBuffer deleted,
                                       ByteBuffer lastUnloadOut, ByteBuffer statusOut);
    // instances join after podIdsLoad: the nNew ids get the indices P .. P + nNew - 1; idOrderOut / replicaSetOut (may be null)
    // cover ALL P + nNew pods and need maxPods >= P + nNew.  The missings marks of registryPrune are kept (a second podIdsLoad
    // clears them); the next commit ranks from scratch.
    static native int podIdsAppend(long h, ByteBuffer ids, ByteBuffer idOff, int nNew, ByteBuffer idOrderOut,
                                   ByteBuffer replicaSetOut, int maxPods);
    /** handleInstanceTableChange (MM.java:1455) as stored: event i = the raw key bytes keys[keyOff[i], keyOff[i+1]) (the instance
     *  id) with the raw value json[off[i], off[i+1]); deleted (may be null) marks a deletion; flags 1 = unknown ids join.
     *  podIdxOut = the pod of each event (-1 with status 2), statusOut 0 applied / 1 malformed / 2 unknown id; nAppendedOut =
     *  ids that joined (one int, may be null). */
    static native int podsEventsJson(long h, ByteBuffer keys, ByteBuffer keyOff, ByteBuffer json, ByteBuffer off, int n,
                                     ByteBuffer deleted, ByteBuffer live, int flags, ByteBuffer podIdxOut,
                                     ByteBuffer startTimeOut, ByteBuffer statusOut, ByteBuffer nAppendedOut);
    // Instance labels kept in the context.  labelNamesLoad: the label names some type constraint mentions, name i = bit i of a
    // label word (at most 64; nLabels 0 unloads; clears every resident word).  While names are loaded podsIngestJson and
    // podsEventsJson read `labels` from the stored value, so the listener decodes no InstanceRecord: podLabelsGet gives words
    // and element counts back (count 0 = NO_LABELS = labelsKey 0 of upgradeInstanceAdded; either buffer may be null, nOut = the
    // pod count), typesFromPodLabels is typesFromLabels over the resident words, podLabelsSet is for hosts that upsert rows.
    static native int labelNamesLoad(long h, ByteBuffer names, ByteBuffer nameOff, int nLabels);
    static native int podLabelsSet(long h, ByteBuffer idx, ByteBuffer words, ByteBuffer counts, int n);
    static native int podLabelsGet(long h, ByteBuffer wordsOut, ByteBuffer countsOut, int maxPods, ByteBuffer nOut);
    static native int typesFromPodLabels(long h, int nTypes, ByteBuffer required, ByteBuffer preferred, ByteBuffer allowedOut,
                                         ByteBuffer preferOut, ByteBuffer hasAllowedOut, ByteBuffer hasPreferOut);
    // the registry rows holding an entry whose instance id the table does not know, ascending; after a join the listener sends
    // their stored values through modelsUpsertJson again.  nModelsOut (int) / nEntriesOut (long) are the full counts.
    static native int registryUnresolved(long h, ByteBuffer modelOut, int maxModels, ByteBuffer nModelsOut, ByteBuffer nEntriesOut);
    // registry events by key: the model-id table lives on the device.  modelIdsLoad names rows 0 .. nModels-1 (nModels must be
    // the registry's row count; 0 ids over an empty registry is a valid start); modelIdsResolve gives the row of each key, -1 for
    // an unknown id (modelsStatus / registryOps / a request row by id); modelIdsGet gives the ids of a row range back (a null
    // bytesOut with maxBytes 0: nBytesOut only; offOut, may be null, holds nRows + 1 ints).
    static native int modelIdsLoad(long h, ByteBuffer ids, ByteBuffer idOff, int nModels);
    static native int modelIdsResolve(long h, ByteBuffer keys, ByteBuffer keyOff, int n, ByteBuffer modelIdxOut);
    static native int modelIdsGet(long h, int firstRow, int nRows, ByteBuffer bytesOut, int maxBytes, ByteBuffer offOut,
                                  ByteBuffer nBytesOut);
    /** the registry listener (MM.java:628, event() :2807-2854) as it is called: event i = the raw key bytes keys[keyOff[i],
     *  keyOff[i+1]) (the model id, any UTF-8) with the raw value json[off[i], off[i+1]); deleted (may be null) marks
     *  ENTRY_DELETED; flags 1 = unknown ids join as new rows.  modelIdxOut = the row of each event (-1 with status 2), statusOut
     *  0 applied / 1 malformed / 2 unknown id; lastUnloadOut (may be null); nAppendedOut = ids that joined (one int, may be null). */
    static native int modelsEventsJson(long h, ByteBuffer keys, ByteBuffer keyOff, ByteBuffer json, ByteBuffer off, int n,
                                       ByteBuffer deleted, int flags, ByteBuffer modelIdxOut, ByteBuffer lastUnloadOut,
                                       ByteBuffer statusOut, ByteBuffer nAppendedOut);
    /** the vmodel table (VModelManager.java:101-110) on the device.  vmodelsEventsJson takes the vmodel listener's events as
     *  modelsEventsJson takes the registry's: raw key bytes, raw VModelRecord value, deleted (may be null), flags 1 = unknown ids
     *  join as new rows; there is no load call, start-up is one batch with flags 1.  statusOut 0 applied / 1 malformed / 2 unknown. */
    static native int vmodelsEventsJson(long h, ByteBuffer keys, ByteBuffer keyOff, ByteBuffer json, ByteBuffer off, int n,
                                        ByteBuffer deleted, int flags, ByteBuffer vmodelIdxOut, ByteBuffer statusOut,
                                        ByteBuffer nAppendedOut);
    /** resolveVModelId (:569-597) and the classes of getVModelStatus (:505-559), one 32-byte answer per key: cls (0 not found / 1 ok /
     *  2 strong read wanted / 3 target not found / 4 the host decodes), which (0 active / 1 target), vmodel, model, target_model,
     *  vstatus, target_status, flags.  nfKeys / nfOff (notFoundModelId), owners / ownerOff and reqFlags (1 = after the strong read)
     *  may each be null; an empty span is null.  model goes straight into a request row. */
    static native int vmodelsResolve(long h, ByteBuffer keys, ByteBuffer keyOff, int n, ByteBuffer nfKeys, ByteBuffer nfOff,
                                     ByteBuffer owners, ByteBuffer ownerOff, ByteBuffer reqFlags, ByteBuffer rowsOut);
    /** processVModels (:617-634) with the prologue of PendingTransition.run (:701-708): the rows in transition, 32 bytes each —
     *  vmodel, from_model, to_model, target_count, cls (0 promote / 1 ensureLoaded), flags, last_used.  nOut = the full count;
     *  a null rowsOut with maxRows 0 sizes.  infoOut (24 bytes, may be null). */
    static native int vmodelsTransitions(long h, long nowMs, long lastUsedAgeOnAddMs, ByteBuffer rowsOut, int maxRows, ByteBuffer nOut,
                                         ByteBuffer infoOut);
    /** the way back: ids, flags and the three raw strings (amid, tmid, o: spans 3r .. 3r + 2) of a row range; sizes first. */
    static native int vmodelsGet(long h, int firstRow, int nRows, ByteBuffer idBytesOut, int maxIdBytes, ByteBuffer idOffOut,
                                 ByteBuffer nIdBytesOut, ByteBuffer flagsOut, ByteBuffer strBytesOut, int maxStrBytes,
                                 ByteBuffer strOffOut, ByteBuffer nStrBytesOut);
    /** getStatus BY MODEL ID (MM.java:3247-3263) in one call under one hold of the library's batch lock — modelIdsResolve and
     *  modelsStatus with nothing able to land between them.  failPod / flags (n ints each) and modelIdxOut (n ints) may be null; an
     *  unknown id AND the empty row a deleted record leaves answer class 0 (NOT_FOUND), modelIdxOut tells them apart.  Sizes and
     *  truncation as modelsStatus. */
    static native int modelsStatusKeyed(long h, ByteBuffer keys, ByteBuffer keyOff, int n, ByteBuffer failPod, ByteBuffer flags, long nowMs,
                                        ByteBuffer modelIdxOut, ByteBuffer rowsOut, ByteBuffer copiesOut, int maxCopies,
                                        ByteBuffer nCopiesOut);
    /** getVModelStatus IN FULL (VModelManager.java:505-559) in one call: vrowsOut = n rows of 32 bytes (cls 0 not found / 1 ok /
     *  2 strong read wanted / 4 the host decodes, vmodel, model, target_model, vstatus, target_status, flags 1 failed | 4 amid null |
     *  8 tmid null | 16 o null, 0); rowsOut = 2 n mmp_status_row (2 i the active model's, 2 i + 1 the target's) with their copies in
     *  copiesOut; the reply's three strings of key i are spans 3 i (amid), 3 i + 1 (tmid), 3 i + 2 (o) of strBytesOut / strOffOut.
     *  owners / ownerOff, reqFlags (1 = after the strong read) and strOffOut may be null; null copiesOut / strBytesOut with
     *  capacities 0 give nCopiesOut / nStrBytesOut only. */
    static native int vmodelsStatus(long h, ByteBuffer keys, ByteBuffer keyOff, int n, ByteBuffer owners, ByteBuffer ownerOff,
                                    ByteBuffer reqFlags, long nowMs, ByteBuffer vrowsOut, ByteBuffer rowsOut, ByteBuffer copiesOut,
                                    int maxCopies, ByteBuffer nCopiesOut, ByteBuffer strBytesOut, int maxStrBytes, ByteBuffer strOffOut,
                                    ByteBuffer nStrBytesOut);
    /** rows, live rows, arena bytes, live bytes, table capacity (32 bytes). */
    static native int vmodelsInfo(long h, ByteBuffer out);
    /** hand vmodel rows back (mmp_vmodels_retire): rows = n ints, the rows whose deletion the vmodel listener has seen; flags 1 =
     *  every named row must still be ABSENT (else MMP_EINVAL, nothing changed: the id was set again), 2 = no list (n 0), the device
     *  retires every ABSENT row.  The survivors move down in order; remapOut (maxVmodels >= the row count at the call, may be null)
     *  gives old row -> new row, -1 for a retired one — row numbers the Java side holds from vmodelsResolve / vmodelsTransitions are
     *  renumbered from it; nVmodelsAfterOut (one int, may be null). */
    static native int vmodelsRetire(long h, ByteBuffer rows, int n, int flags, ByteBuffer remapOut, int maxVmodels,
                                    ByteBuffer nVmodelsAfterOut);
    /** the write side of the wire format (mmp_models_rewrite_json), for the 13 conditionalSet / conditionalSetAndGet sites of
     *  ModelMesh.java: value i = the stored bytes oldJson[oldOff[i], oldOff[i+1]) of registry row rows[i]; the answer is the value to
     *  store next — what the device does not own copied byte for byte, instanceIds / failedIn / fails / lu (and lul from lastUnload,
     *  may be null) rendered from the resident row; failPod / failMsg / failMsgOff (all three may be null) are addLoadFailure /
     *  removeLoadFailure of one instance per value.  New value i = outBuf[outOff[i], outOff[i+1]); statusOut 0 rendered / 1 the
     *  old value is malformed / 2 the host renders this one (an unresolved or unprintable id); nBytesOut (one long) = the bytes of
     *  all values.  Nothing is written to outBuf when it is null or outCap is smaller than that: call again with room.  flags 0. */
    static native int modelsRewriteJson(long h, ByteBuffer rows, int n, ByteBuffer oldJson, ByteBuffer oldOff, ByteBuffer lastUnload,
                                        ByteBuffer failPod, ByteBuffer failMsg, ByteBuffer failMsgOff, int flags, ByteBuffer outBuf,
                                        long outCap, ByteBuffer outOff, ByteBuffer statusOut, ByteBuffer nBytesOut);
    /** registerModel / deleteModel (ModelMesh.java:3088-3147, :3181-3203) as a batch of questions (mmp_models_register_json):
     *  request i = reqs[i] (16 bytes: int flags 1 = loadNow / 2 = delete, int reserved, long initialCacheTimestamp), its type, encKey
     *  and mPath the spans 3i .. 3i + 2 of info / infoOff (an empty encKey / mPath span is null), and the stored value
     *  oldJson[oldOff[i], oldOff[i+1]) the registry listener holds for that id (empty: registry.get() == null).  classOut 0 created /
     *  1 touched (both: the value to conditionalSet is outBuf[outOff[i], outOff[i+1])) / 2 exists / 3 different attributes / 4 absent /
     *  5 has referents / 6 conditionalDelete the old value / 7 malformed / 8 the host decides; lastUsedOut = lastUsedTimestamp of
     *  :3098-3101.  modelIdxOut (may be null, then keys / keyOff too) = the row of each id, -1 unknown.  Sizing as modelsRewriteJson:
     *  nothing is written to outBuf when it is null or outCap is smaller than nBytesOut.  flags 0. */
    static native int modelsRegisterJson(long h, ByteBuffer reqs, int n, ByteBuffer keys, ByteBuffer keyOff, ByteBuffer info,
                                         ByteBuffer infoOff, ByteBuffer oldJson, ByteBuffer oldOff, long nowMs, long lastUsedAgeOnAddMs,
                                         int flags, ByteBuffer outBuf, long outCap, ByteBuffer outOff, ByteBuffer classOut,
                                         ByteBuffer lastUsedOut, ByteBuffer modelIdxOut, ByteBuffer nBytesOut);
    /** the ModelRecord half of the vmodel transactions (VModelManager.java:299-302, decModelRefsInTxn :475-489) as a batch of steps
     *  (mmp_models_refs_json): request i = reqs[i] (16 bytes: int flags 1 = setLastUsed + incRefCount, else decModelRefsInTxn / 2 =
     *  autoDelete of a created record, int reserved, long lastUsed) on the stored value oldJson[oldOff[i], oldOff[i+1]) (empty: mr ==
     *  null); info / infoOff (may be null both) bring type, encKey, mPath for a record the INC creates.  classOut 0 txn.set / 1
     *  created (both: the value is outBuf[outOff[i], outOff[i+1])) / 2 txn.delete with the old value / 3 txn.ensureAbsent / 4 target
     *  model not found / 5 malformed / 6 the host decides; refsOut = what incRefCount / decRefCount return.  Sizing as
     *  modelsRewriteJson: nothing is written to outBuf when it is null or outCap is smaller than nBytesOut.  flags 0. */
    static native int modelsRefsJson(long h, ByteBuffer reqs, int n, ByteBuffer info, ByteBuffer infoOff, ByteBuffer oldJson,
                                     ByteBuffer oldOff, int flags, ByteBuffer outBuf, long outCap, ByteBuffer outOff,
                                     ByteBuffer classOut, ByteBuffer refsOut, ByteBuffer nBytesOut);
    /** the record step of updateVModel (VModelManager.java:174-189, :216-284), deleteVModel (:416-470) and the tail of
     *  PendingTransition.run (:725-766) as a batch (mmp_vmodels_write_json): request i = reqs[i] (8 bytes: int op 0 set / 1 delete /
     *  2 complete / 3 fail flag, int flags 1 updateOnly / 2 force / 4 loadNow / 8 the target has a stored value / 16, 32 getStatus(target)
     *  is / is not LOADED / 64 the new failed flag), its id_a, id_b and owner the spans 3i .. 3i + 2 of strs / strOff (empty: null),
     *  on the stored VModelRecord oldJson[oldOff[i], oldOff[i+1]) (empty: vmr == null).  rowsOut[i] (48 bytes: int cls, int flags,
     *  int model, int targetCopyCount, int[2] decModel, int[2] decOff, int[2] decLen, long lastUsed): cls 0 created / 1 updated (both:
     *  the value to set is outBuf[outOff[i], outOff[i+1])) / 2 unchanged / 3 not found / 4 failed precondition / 5 another owner /
     *  6 call again with 16 or 32 / 7 nothing to do / 8 delete with the old value / 9 things changed / 10 malformed / 11 the host
     *  decides; decOff / decLen name the ids whose refs go down (modelsRefsJson) inside the old value.  Sizing as modelsRewriteJson.
     *  flags 0. */
    static native int vmodelsWriteJson(long h, ByteBuffer reqs, int n, ByteBuffer strs, ByteBuffer strOff, ByteBuffer defaultOwner,
                                       int defaultOwnerLen, ByteBuffer oldJson, ByteBuffer oldOff, long nowMs, long lastUsedAgeOnAddMs,
                                       int flags, ByteBuffer outBuf, long outCap, ByteBuffer outOff, ByteBuffer rowsOut,
                                       ByteBuffer nBytesOut);
    /** hand registry rows back (mmp_models_retire): rows = n ints, the rows whose deletion the listener has seen; flags 1 = every
     *  named row must still be the empty row a deletion leaves (else MMP_EINVAL, nothing changed: the id was registered again).
     *  The survivors move down in order; remapOut (maxModels >= the row count at the call, may be null) gives old row -> new row,
     *  -1 for a retired one — every row number the Java side holds is renumbered from it; nModelsAfterOut (one int, may be null). */
    static native int modelsRetire(long h, ByteBuffer rows, int n, int flags, ByteBuffer remapOut, int maxModels,
                                   ByteBuffer nModelsAfterOut);
    /** hand instance indices back (mmp_pods_retire): pods = n ints, the instances whose deletion the instance listener has seen
     *  and whose registrations the reaper has pruned; flags 1 = every named row must still be a tombstone (else MMP_EINVAL,
     *  nothing changed: the id came back), 2 = no registry record may still name one.  The survivors move down in order and the
     *  call commits; remapOut (maxPods >= the instance count at the call, may be null) gives old index -> new index, -1 for a
     *  retired one — every instance number the Java side holds (request rows, exclusions, serve counters, selfPod) is renumbered
     *  from it; nPodsAfterOut (one int) and nEntriesUnresolvedOut (one long, the entries that now name nobody) may be null. */
    static native int podsRetire(long h, ByteBuffer pods, int n, int flags, ByteBuffer remapOut, int maxPods,
                                 ByteBuffer nPodsAfterOut, ByteBuffer nEntriesUnresolvedOut);
    // misc
    static native long minSpaceUnits(int defaultModelSizeUnits, int loadingThreads, long capacityUnits,
                                     boolean haveUnloadManager);
    static native int getOrder(long h, ByteBuffer orderOut, ByteBuffer nOut);
    static native int deltaCommits(long h, ByteBuffer nOut);
    static native int profile(long h, boolean enable);
    static native double lastKernelMs(long h);
    static native int abiVersion();
    static final int NONE = -1, SELF = -2;

    static ByteBuffer direct(int bytes) { return ByteBuffer.allocateDirect(bytes).order(ByteOrder.LITTLE_ENDIAN); }
    /** bytes [off, off + len) of a direct buffer as a direct buffer of its own (the natives read a buffer from its address) */
    static ByteBuffer slice(ByteBuffer b, int off, int len) {
        ByteBuffer d = b.duplicate();
        d.position(off).limit(off + len);
        return d.slice().order(ByteOrder.LITTLE_ENDIAN);
    }
}

/** One model id as the keyed natives take it: { the id's UTF-8 bytes, keyOff = {0, length} }, in per-thread direct buffers. */
final class ModelKey {
    private static final ThreadLocal<ByteBuffer[]> BUF = ThreadLocal.withInitial(() -> new ByteBuffer[] { MmPlace.direct(256), MmPlace.direct(8) });

    static ByteBuffer[] of(String modelId) {
        final byte[] utf8 = modelId.getBytes(java.nio.charset.StandardCharsets.UTF_8);
        ByteBuffer[] b = BUF.get();
        if (b[0].capacity() < utf8.length) b[0] = MmPlace.direct(Math.max(utf8.length, 2 * b[0].capacity()));
        b[0].clear();
        b[0].put(utf8);
        b[1].putInt(0, 0);
        b[1].putInt(4, utf8.length);
        return b;
    }
}

/**
 * The ids of a periodic task's entries as the keyed natives take them: { the ids' UTF-8 bytes back to back, keyOff = n + 1 ints },
 * in iteration order.  The rate task, the janitor and preShutdown iterate runtimeCache (descendingMapWithCutoff, descendingMap,
 * descendingLruMap: MM.java:5672, :5892, :6998), whose keys are model ids: a binding without an id map (modelIdsResident() == true)
 * fills the entry rows' model field with -1 and hands the keys over here, ONE scaleupPlanKeyed / janitorPlanKeyed /
 * migrationPlanKeyed call per run instead of modelIdsResolve + the by-row call.
 */
final class TaskKeys {
    static ByteBuffer[] of(java.util.Collection<String> modelIds) {
        final byte[][] utf8 = new byte[modelIds.size()][];
        int total = 0, i = 0;
        for (String id : modelIds) {
            utf8[i] = id.getBytes(java.nio.charset.StandardCharsets.UTF_8);
            total = Math.addExact(total, utf8[i++].length);
        }
        final ByteBuffer keys = MmPlace.direct(Math.max(total, 1)), off = MmPlace.direct(4 * (utf8.length + 1));
        off.putInt(0, 0);
        for (i = 0; i < utf8.length; i++) {
            keys.put(utf8[i]);
            off.putInt(4 * (i + 1), keys.position());
        }
        return new ByteBuffer[] { keys, off };
    }
}

/**
 * ModelMeshApi.callModel (:452-476) for a request that names a VMODEL, on a binding whose vmodel table is resident on the device
 * (vmodelsEventsJson): resolveVModelId and the route seam of invokeModel are ONE call on a latency slot (routeBatchVKeyed) instead of
 * vmodelsResolve — which takes the library's batch lock — followed by routeBatchCaller on the row it answered.
 *
 *   first attempt      nf = null: the active model is answered (cls 1, which 0)
 *   MODEL_NOT_FOUND    the invocation came back with "model not found" for that id: the second attempt passes it as nf (:466-470).
 *                      cls 2 (the stored active id IS nf): vModels.getStrong(vModelId) (:582), its value through vmodelsEventsJson
 *                      — so that the device holds what the strong read saw — and the call again with reqFlags = 1; then cls 1 with
 *                      which = 1 (the target) or cls 3 (:594, INTERNAL "Target model ... not found")
 *   cls 0 / 4          NOT_FOUND to the client (:570-573) / a record with an escaped string: the host resolves it from the KV value
 * The gate and serve rows are the caller's to fill, as for routeBatchKeyed; only the answer's class is interpreted here.
 */
final class VModelCall {
    static final int NOT_FOUND = 0, OK = 1, STRONG_READ = 2, TARGET_NOT_FOUND = 3, HOST = 4;
    static final int AFTER_STRONG = 1, NULL_ID = 1;

    /** what the strong read needs from the enclosing instance: vModels.getStrong(id) as the raw stored bytes, null for absent */
    interface StrongReader { byte[] getStrong(String vModelId) throws Exception; }

    private static final ThreadLocal<ByteBuffer> VM_OUT = ThreadLocal.withInitial(() -> MmPlace.direct(24));
    private static final ThreadLocal<ByteBuffer> FLAGS = ThreadLocal.withInitial(() -> MmPlace.direct(4));
    private static final ThreadLocal<ByteBuffer[]> NF = ThreadLocal.withInitial(() -> new ByteBuffer[] { MmPlace.direct(256), MmPlace.direct(8) });
    private static final ThreadLocal<ByteBuffer> ONE_OFF = ThreadLocal.withInitial(() -> MmPlace.direct(32));

    private static ByteBuffer[] span(ThreadLocal<ByteBuffer[]> tl, byte[] utf8) {
        ByteBuffer[] b = tl.get();
        if (b[0].capacity() < utf8.length) b[0] = MmPlace.direct(Math.max(utf8.length, 2 * b[0].capacity()));
        b[0].clear();
        b[0].put(utf8);
        b[1].putInt(0, 0);
        b[1].putInt(4, utf8.length);
        return b;
    }

    /**
     * One route of a vmodel request: { cls, which, vmodel row, model row, flags } of the answer the decision in gateOut / serveOut
     * belongs to.  notFoundModelId == null: the first attempt.  The caller invokes on serveOut only when cls is OK and flags is 0.
     */
    static int[] route(GpuMeshBinding mesh, StrongReader kv, String vModelId, String notFoundModelId, ByteBuffer caller, ByteBuffer gate,
                       ByteBuffer serve, ByteBuffer counters, int nCounters, ByteBuffer exclPod, ByteBuffer exclTime, int nExcl, long nowMs,
                       ByteBuffer gateOut, ByteBuffer serveOut) throws Exception {
        final ByteBuffer[] key = ModelKey.of(vModelId);
        final ByteBuffer[] nf = notFoundModelId == null ? null
                : span(NF, notFoundModelId.getBytes(java.nio.charset.StandardCharsets.UTF_8));
        final ByteBuffer vm = VM_OUT.get(), flags = FLAGS.get();
        flags.putInt(0, 0);
        for (int attempt = 0; ; attempt++) {
            MmPlace.routeBatchVKeyed(mesh.handle(), caller, gate, serve, 1, key[0], key[1], nf != null ? nf[0] : null,
                                     nf != null ? nf[1] : null, flags, counters, nCounters, exclPod, exclTime, nExcl, null, 0, nowMs,
                                     ModelMesh.IN_USE_LOAD_FAILURE_EXPIRY_MS, gateOut, serveOut, vm);
            final int cls = vm.getInt(0);
            if (cls != STRONG_READ || attempt > 0) break;       // (after the strong read the device never answers STRONG_READ)
            // :582 — the strong read, and its value to the device before the question is asked again
            final byte[] fresh = kv.getStrong(vModelId);
            final byte[] value = fresh != null ? fresh : new byte[0];
            final ByteBuffer json = MmPlace.direct(Math.max(value.length, 1));
            json.put(value);
            final ByteBuffer off = ONE_OFF.get();
            off.putLong(0, 0L); off.putLong(8, value.length);
            final ByteBuffer deleted = MmPlace.slice(off, 16, 1), idx = MmPlace.slice(off, 20, 4), status = MmPlace.slice(off, 24, 4);
            deleted.put(0, (byte) (fresh == null ? 1 : 0));
            MmPlace.vmodelsEventsJson(mesh.handle(), key[0], key[1], json, MmPlace.slice(off, 0, 16), 1, deleted, 1, idx, status, null);
            flags.putInt(0, AFTER_STRONG);
        }
        return new int[] { vm.getInt(0), vm.getInt(4), vm.getInt(8), vm.getInt(12), vm.getInt(16) };
    }
}

/**
 * The five sites at which an instance edits a ModelRecord itself, for a binding without an id map (modelIdsResident() == true): ONE
 * registryOpsKeyed call per site instead of modelIdsResolve + registryOps, so that the row and its edit are of one state of the
 * registry.  Each method answers the edit (null: the Java returns without a compare-and-set — nothing changed, or there is no
 * record); the caller submits the record through registry.conditionalSetAndGet as before and keeps the retry loop, loadFailureInfos
 * and refreshAfterUpdatedModelRecord.
 */
final class RegistryOpsById {
    static final int REGISTER = 0, LOAD_FAILED = 1, DEREGISTER = 2, SCALE_DOWN = 3, DROP_LOCAL = 4;
    static final int SHUTTING_DOWN = 1, MATCH_TIME = 2;         // op flags
    static final int UNCHANGED = 0, EDITED = 1, NO_RECORD = 2;  // status bytes
    static final int APPLY = 1;

    /** one edit: the mmp_registry_op_edit row */
    static final class Edit {
        int row, nLoadedAfter, nFailedAfter, flags, insertedPos;   // flags: 1 rem loaded, 2 rem failed, 4 put loaded, 8 put failed,
        long lastUsedAfter, lastUnloadAfter;                       //   16 replaced, 32 lastUsed raised, 64 lastUnloadAfter is to be stored
    }

    private static Edit one(GpuMeshBinding mesh, String modelId, int pod, int op, int flags, long lastUsed, long loadTime,
                            long loadCompleteTime, long nowMs) {
        if (!mesh.modelIdsResident()) throw new IllegalStateException("a binding with an id map sends rows: MmPlace.registryOps");
        final ByteBuffer[] key = ModelKey.of(modelId);
        final ByteBuffer row = MmPlace.direct(40), status = MmPlace.direct(1), edit = MmPlace.direct(40), info = MmPlace.direct(88);
        row.putInt(0, -1); row.putInt(4, pod); row.putInt(8, op); row.putInt(12, flags);
        row.putLong(16, lastUsed); row.putLong(24, loadTime); row.putLong(32, loadCompleteTime);
        MmPlace.registryOpsKeyed(mesh.handle(), row, 1, key[0], key[1], nowMs, APPLY, null, status, edit, 1, info);
        if (status.get(0) != EDITED) return null;               // UNCHANGED, or NO_RECORD: mr == null (:2481, :2945)
        final Edit e = new Edit();
        e.row = edit.getInt(0); e.nLoadedAfter = edit.getInt(8); e.nFailedAfter = edit.getInt(12);
        e.flags = edit.getInt(16); e.insertedPos = edit.getInt(20);
        e.lastUsedAfter = edit.getLong(24); e.lastUnloadAfter = edit.getLong(32);
        return e;
    }

    /** loadLocal's put, MM.java:5204-5207 */
    static Edit registered(GpuMeshBinding mesh, String modelId, int self, long lastUsed, long loadTime, long nowMs) {
        return one(mesh, modelId, self, REGISTER, 0, lastUsed, loadTime, 0L, nowMs);
    }
    /** the CacheEntry failure path, :2484-2495 */
    static Edit loadFailed(GpuMeshBinding mesh, String modelId, int self, boolean shuttingDown, long lastUsed, long loadTime,
                           long loadCompleteTime, long nowMs) {
        return one(mesh, modelId, self, LOAD_FAILED, shuttingDown ? SHUTTING_DOWN : 0, lastUsed, loadTime, loadCompleteTime, nowMs);
    }
    /** deregisterModel, :2948-2958; loadTime null: either entry goes if present */
    static Edit deregistered(GpuMeshBinding mesh, String modelId, int self, long lastUsed, Long loadTime, long loadCompletedTime,
                             long nowMs) {
        return one(mesh, modelId, self, DEREGISTER, loadTime != null ? MATCH_TIME : 0, lastUsed, loadTime != null ? loadTime : 0L,
                   loadCompletedTime, nowMs);
    }
    /** removeLocalModelCopyAsync, :6347-6365, sent after isLoadedElsewhere */
    static Edit scaledDown(GpuMeshBinding mesh, String modelId, int self, long lastUsed, long loadTime, long nowMs) {
        return one(mesh, modelId, self, SCALE_DOWN, 0, lastUsed, loadTime, 0L, nowMs);
    }
    /** invokeModel's cache-hit loop: goLocal and getFromCache == null, :3682-3687 — always an edit when the record exists; the
     *  KV-error branch (:3693-3709) stays with the caller */
    static Edit droppedLocal(GpuMeshBinding mesh, String modelId, int self, long lastUsed, long nowMs) {
        return one(mesh, modelId, self, DROP_LOCAL, 0, lastUsed, 0L, 0L, nowMs);
    }
}

/**
 * The eviction loop for a binding without an id map (modelIdsResident() == true), written as ModelMesh.onEviction's task body
 * (MM.java:2886-2920) against TWO calls and nothing in between: MmPlace.cacheReplayKT — the replay that evicts; its record carries each
 * victim's id and the lastUsed the clhm hands the listener — and MmPlace.evictionsKeyed here.  No row, no invented time and no
 * ModelRecord on the host: loadedTime is read from the resident record, in the same hold of the library's batch lock that
 * deregisters, so the read and the edit are of one registry state.
 */
final class EvictionsById {
    static final int IN_REGISTRY = 1, ATTEMPT_RELOAD = 2, RELOAD = 4, LOG = 8;

    /** one victim: the record's id and lastUsed, and what the CacheEntry holds */
    static final class Victim {
        String modelId;
        long lastUsed, loadTimestamp, loadCompleteTimestamp;   // lastUsed: cacheReplayKT's evLastUsedOut
        int weight;                                            // ce.getWeight(), for ensureLoadedElsewhere
        boolean failed;                                        // ce.isFailed()
    }
    /** what the task body decided for it */
    static final class Settled {
        boolean inRegistry, attemptReload, reloadElsewhere, log;   // :2894, :2895, :2918-2920, :2900
        long loadedTime, millisSinceLastUsed;                      // loadedTime -1: none was read
        RegistryOpsById.Edit edit;                                 // null: deregisterModel returned without a compare-and-set
    }

    /** the first call: the replay that evicts.  ops / keys / outs as cacheReplayK takes them; answers one Victim per eviction slot
     *  with its id and lastUsed filled in (null for a slot no op used).  The caller adds what its CacheEntry holds. */
    static Victim[] replay(GpuMeshBinding mesh, ByteBuffer ops, int nOps, ByteBuffer keys, ByteBuffer keyOff, long nowMs, ByteBuffer outs,
                           int maxEvicted, int idBytesHint) {
        final ByteBuffer rows = MmPlace.direct(Math.max(4 * maxEvicted, 1)), off = MmPlace.direct(4 * (maxEvicted + 1)), sizes = MmPlace.direct(8),
                         times = MmPlace.direct(Math.max(8 * maxEvicted, 1));
        ByteBuffer bytes = MmPlace.direct(Math.max(idBytesHint, 1));
        MmPlace.cacheReplayKT(mesh.handle(), ops, nOps, keys, keyOff, nowMs, null, null, outs, rows, maxEvicted, bytes, idBytesHint, off, sizes,
                              times);
        final int slots = sizes.getInt(0), need = sizes.getInt(4);
        if (need > idBytesHint) {                                  // the replay ran once; the context kept the record
            bytes = MmPlace.direct(need);
            MmPlace.cacheEvictedIds(mesh.handle(), bytes, need, off, sizes);
        }
        final Victim[] out = new Victim[slots];
        for (int s = 0; s < slots; s++) {
            if (rows.getInt(4 * s) < 0) continue;
            final byte[] id = new byte[off.getInt(4 * (s + 1)) - off.getInt(4 * s)];
            for (int k = 0; k < id.length; k++) id[k] = bytes.get(off.getInt(4 * s) + k);
            out[s] = new Victim();
            out[s].modelId = new String(id, java.nio.charset.StandardCharsets.UTF_8);
            out[s].lastUsed = times.getLong(8 * s);
        }
        return out;
    }

    /** the second call: victims of one replay.  Two victims that name one record (an id evicted, put back and evicted again inside
     *  one replay) are refused with nothing changed: the caller splits the list in front of the second one. */
    static Settled[] settle(GpuMeshBinding mesh, java.util.List<Victim> victims, int self, long nowMs, long loadTimeoutMs) {
        if (!mesh.modelIdsResident()) throw new IllegalStateException("a binding with an id map runs onEviction on its records");
        final int n = victims.size();
        final java.util.List<String> ids = new java.util.ArrayList<>(n);
        final ByteBuffer entries = MmPlace.direct(Math.max(32 * n, 1)), params = MmPlace.direct(24), outs = MmPlace.direct(Math.max(24 * n, 1)),
                         status = MmPlace.direct(Math.max(n, 1)), edits = MmPlace.direct(Math.max(40 * n, 1)), info = MmPlace.direct(112);
        for (int i = 0; i < n; i++) {
            final Victim v = victims.get(i);
            ids.add(v.modelId);
            entries.putLong(32 * i, v.lastUsed); entries.putLong(32 * i + 8, v.loadTimestamp);
            entries.putLong(32 * i + 16, v.loadCompleteTimestamp);
            entries.putInt(32 * i + 24, v.weight); entries.putInt(32 * i + 28, v.failed ? 1 : 0);
        }
        params.putInt(0, self); params.putInt(4, 0); params.putLong(8, nowMs); params.putLong(16, loadTimeoutMs);
        final ByteBuffer[] keys = TaskKeys.of(ids);
        MmPlace.evictionsKeyed(mesh.handle(), entries, n, keys[0], keys[1], params, RegistryOpsById.APPLY, null, outs, status, edits, n, info);
        final Settled[] out = new Settled[n];
        int x = 0;                                                 // edits come in victim order
        for (int i = 0; i < n; i++) {
            final Settled s = out[i] = new Settled();
            final int flags = outs.getInt(24 * i);
            s.inRegistry = (flags & IN_REGISTRY) != 0; s.attemptReload = (flags & ATTEMPT_RELOAD) != 0;
            s.reloadElsewhere = (flags & RELOAD) != 0; s.log = (flags & LOG) != 0;
            s.loadedTime = outs.getLong(24 * i + 8); s.millisSinceLastUsed = outs.getLong(24 * i + 16);
            if (status.get(i) != RegistryOpsById.EDITED) continue;
            final RegistryOpsById.Edit e = s.edit = new RegistryOpsById.Edit();
            e.row = edits.getInt(40 * x); e.nLoadedAfter = edits.getInt(40 * x + 8); e.nFailedAfter = edits.getInt(40 * x + 12);
            e.flags = edits.getInt(40 * x + 16); e.insertedPos = edits.getInt(40 * x + 20);
            e.lastUsedAfter = edits.getLong(40 * x + 24); e.lastUnloadAfter = edits.getLong(40 * x + 32);
            x++;
        }
        // the caller: logs and metrics where s.log (:2902-2906), ce.doRemove (:2910), the record through conditionalSetAndGet where
        // s.edit != null (:2958), and for s.reloadElsewhere ensureLoadedElsewhere (:2922) through the _ck seams with itself excluded
        return out;
    }
}

/**
 * The management path's two status RPCs answered by id, one library call each instead of the sequence modelIdsResolve + modelsStatus
 * (getModelStatus) and vmodelsResolve + modelsStatus + vmodelsGet per row (getVModelStatus): every part of an answer comes from ONE
 * state of the registry and the vmodel table, whatever event batch or retirement the listeners send meanwhile.
 */
final class StatusById {
    /** one answered status: class (0 NOT_FOUND / 1 NOT_LOADED / 2 LOADING_FAILED / 3 ask a copy) and the copies, latest first */
    static final class Status {
        int cls, row;             // row: the registry row the id table names (-1 unknown; a deleted record keeps its row)
        int[] pod, copyStatus;    // 0 NOT_CHECKED / 1 LOADING_FAILED
        long[] time;
    }
    /** getVModelStatus's reply: cls as VModelCall (0 NOT_FOUND: the default instance; 4 HOST: decode the KV value instead) */
    static final class VStatus {
        int cls, vstatus, targetStatus;
        String activeModelId, targetModelId, owner;   // null where the record holds null
        Status active, target;                        // target: class 0 and no copies when not in transition
    }

    private static Status status(ByteBuffer rows, int i, ByteBuffer copies, int row) {
        final Status s = new Status();
        s.cls = rows.getInt(16 * i);
        s.row = row;
        final int off = rows.getInt(16 * i + 4), n = rows.getInt(16 * i + 8) + rows.getInt(16 * i + 12);
        s.pod = new int[n]; s.copyStatus = new int[n]; s.time = new long[n];
        for (int k = 0; k < n; k++) {
            s.pod[k] = copies.getInt(16 * (off + k));
            s.copyStatus[k] = copies.getInt(16 * (off + k) + 4);
            s.time[k] = copies.getLong(16 * (off + k) + 8);
        }
        return s;
    }

    /** getStatus(modelId), MM.java:3247-3263: sizes first, then the list (again if the record grew in between) */
    static Status getModelStatus(GpuMeshBinding mesh, String modelId, long nowMs) {
        final ByteBuffer[] key = ModelKey.of(modelId);
        final ByteBuffer rows = MmPlace.direct(16), idx = MmPlace.direct(4), total = MmPlace.direct(4);
        MmPlace.modelsStatusKeyed(mesh.handle(), key[0], key[1], 1, null, null, nowMs, idx, rows, null, 0, total);
        for (;;) {
            final int cap = total.getInt(0);
            final ByteBuffer copies = MmPlace.direct(Math.max(16 * cap, 16));
            MmPlace.modelsStatusKeyed(mesh.handle(), key[0], key[1], 1, null, null, nowMs, idx, rows, cap > 0 ? copies : null, cap, total);
            if (total.getInt(0) <= cap) return status(rows, 0, copies, idx.getInt(0));
        }
    }

    private static String str(ByteBuffer bytes, ByteBuffer off, int span, boolean isNull) {
        if (isNull) return null;
        final byte[] b = new byte[off.getInt(4 * (span + 1)) - off.getInt(4 * span)];
        for (int k = 0; k < b.length; k++) b[k] = bytes.get(off.getInt(4 * span) + k);
        return new String(b, java.nio.charset.StandardCharsets.UTF_8);
    }

    /** getVModelStatus(vmid, owner), VModelManager.java:505-559, the strong read of :514-525 included */
    static VStatus getVModelStatus(GpuMeshBinding mesh, VModelCall.StrongReader kv, String vModelId, String owner, long nowMs)
            throws Exception {
        final ByteBuffer[] key = ModelKey.of(vModelId);
        final ByteBuffer[] own = owner == null || owner.isEmpty() ? null : ModelKey.of(owner);   // :506 emptyToNull
        final ByteBuffer vrow = MmPlace.direct(32), rows = MmPlace.direct(32), flags = MmPlace.direct(4), strOff = MmPlace.direct(16);
        final ByteBuffer nCopies = MmPlace.direct(4), nStr = MmPlace.direct(4);
        flags.putInt(0, 0);
        int capCopies = 0, capStr = 0;
        ByteBuffer copies = MmPlace.direct(16), strs = MmPlace.direct(16);
        for (boolean strong = false; ; ) {
            MmPlace.vmodelsStatus(mesh.handle(), key[0], key[1], 1, own != null ? own[0] : null, own != null ? own[1] : null, flags, nowMs,
                                  vrow, rows, capCopies > 0 ? copies : null, capCopies, nCopies, capStr > 0 ? strs : null, capStr, strOff, nStr);
            if (vrow.getInt(0) == VModelCall.STRONG_READ && !strong) {   // :515 vModels.getStrong, its value to the device, again
                final byte[] fresh = kv.getStrong(vModelId);
                final byte[] value = fresh != null ? fresh : new byte[0];
                final ByteBuffer json = MmPlace.direct(Math.max(value.length, 1)), off = MmPlace.direct(32);
                json.put(value);
                off.putLong(0, 0L); off.putLong(8, value.length);
                final ByteBuffer deleted = MmPlace.slice(off, 16, 1), idx = MmPlace.slice(off, 20, 4), status = MmPlace.slice(off, 24, 4);
                deleted.put(0, (byte) (fresh == null ? 1 : 0));
                MmPlace.vmodelsEventsJson(mesh.handle(), key[0], key[1], json, MmPlace.slice(off, 0, 16), 1, deleted, 1, idx, status, null);
                flags.putInt(0, VModelCall.AFTER_STRONG);
                strong = true;
                continue;
            }
            if (nCopies.getInt(0) <= capCopies && nStr.getInt(0) <= capStr) break;
            capCopies = Math.max(capCopies, nCopies.getInt(0));   // the sizes are known: the same question with room for the lists
            capStr = Math.max(capStr, nStr.getInt(0));
            copies = MmPlace.direct(Math.max(16 * capCopies, 16));
            strs = MmPlace.direct(Math.max(capStr, 16));
        }
        final VStatus v = new VStatus();
        v.cls = vrow.getInt(0);
        v.vstatus = vrow.getInt(16);
        v.targetStatus = vrow.getInt(20);
        final int f = vrow.getInt(24);
        final boolean found = v.cls == VModelCall.OK || v.cls == VModelCall.STRONG_READ;
        v.activeModelId = str(strs, strOff, 0, !found || (f & 4) != 0);
        v.targetModelId = str(strs, strOff, 1, !found || (f & 8) != 0);
        v.owner = str(strs, strOff, 2, !found || (f & 16) != 0);
        v.active = status(rows, 0, copies, vrow.getInt(8));
        v.target = status(rows, 1, copies, vrow.getInt(12));
        return v;
    }
}

/**
 * What the GPU load balancers need from the enclosing ModelMesh instance.  The patch implements it as an inner
 * class of ModelMesh: the interner maps instance id <-> dense pod index (id_order == rank under String.compareTo,
 * replica_set == interned id.substring(0,6)) and model id -> dense model index; the snapshot handle is refreshed by
 * the instance-table listener (handleInstanceTableChange, ModelMesh.java:1455: podsEventsJson with the raw key and value
 * of each event + commit, registryUnresolved + modelsUpsertJson after a join; or podsUpsert / podsRemove with parsed rows) and
 * by the registry listener (modelsIngestJson of the stored values and modelIdsLoad of their keys once, then modelsEventsJson
 * per batch of events with the raw key and the raw byte[] of each event, ENTRY_DELETED as a deleted flag: the listener keeps no
 * id map, modelIndexOf is modelIdsResolve; a listener that numbers its rows itself uses modelsUpsertJson by index, one that holds
 * parsed ModelRecords modelsLoad / modelsUpsert).
 *
 * The REQUEST PATH of a binding without an id map (modelIdsResident() == true) never calls modelIndexOf: modelIdsResolve takes the
 * library's batch lock and would queue every getNext behind the large batches.  The load balancers below hand the model id's UTF-8
 * bytes to placeBatchKeyed / routeBatchKeyed instead, which resolve the id on the device inside the one call on a latency slot.
 */
interface GpuMeshBinding {
    long handle();
    int podCount();
    int podIndexOf(String instanceId);      // -1 if unknown
    String instanceIdOf(int podIndex);
    int modelIndexOf(String modelId);       // -1 if unknown
    boolean modelIdsResident();             // the id -> row map lives in the library alone (modelIdsLoad + modelsEventsJson)
    String selfInstanceId();
    boolean sendDestinationId();            // ModelMesh.sendDestinationId
    InstanceRecord freshSelf();             // getFreshInstanceRecord(), ModelMesh.java:5369
    String currentModelId();                // the model id of the request in flight on this thread
    ModelMesh.CacheMissExcludeSet cacheMissExcludes();            // cacheMissExcludeTl.get(), ModelMesh.java:4755
    ModelMesh.MapFilteringSet<String, Long> cacheHitExcludes();   // cacheHitExcludeTl.get(), ModelMesh.java:4307
    Collection<String> cacheHitKeyExcludes();                     // its private keyExcludes field (:4269), may be null
    int localInvokesInFlight();             // ModelMesh.java:4303
    long lastInvokeTime();                  // ModelMesh.java:4304
    long assumeCompletedAfterMillis(String modelType);            // loadingTimeStats(type), ModelMesh.java:4350
}

/**
 * Replaces the BODY of CacheMissForwardingLB.getNext (ModelMesh.java:4776-5005): one mmp_place_batch(n = 1) per
 * request; everything around it (thread-locals, ThreadContext side effects, the returned ServiceInstanceInfo) is
 * as in the reference.
 */
class GpuCacheMissLB extends ModelMesh.IdBasedLoadBalancer {
    static final int MAX_LIVE_RETRIES = 8;
    final GpuMeshBinding mesh;
    /**
     * The result row (chosen, best, n_candidates, hash) of the last decision OF THE CALLING THREAD, for the shadow harness.
     * litelinks shares one LB instance across all request threads (which is why the reference keeps its request state in
     * ThreadLocals, ModelMesh.java:4755), so nothing a decision produces may live in a field of the LB.
     */
    private static final ThreadLocal<int[]> LAST_OUT = ThreadLocal.withInitial(() -> new int[4]);
    int[] lastOut() { return LAST_OUT.get(); }

    GpuCacheMissLB(GpuMeshBinding mesh) { this.mesh = mesh; }

    private static final ThreadLocal<ByteBuffer> REQ = ThreadLocal.withInitial(() -> MmPlace.direct(64));
    private static final ThreadLocal<ByteBuffer> OUT = ThreadLocal.withInitial(() -> MmPlace.direct(16));
    private static final ThreadLocal<ByteBuffer[]> EXTRA = ThreadLocal.withInitial(() -> new ByteBuffer[] { MmPlace.direct(4 * 64) });

    /** the per-thread exclusion pool, grown (never truncated) to hold n pod indices */
    static ByteBuffer extraPool(int n) {
        ByteBuffer[] box = EXTRA.get();
        if (box[0].capacity() < 4 * n) box[0] = MmPlace.direct(4 * Math.max(n, 2 * (box[0].capacity() / 4)));
        box[0].clear();
        return box[0];
    }

    /** One decision for the request state on this thread; pick replaces ThreadLocalRandom.nextInt(remaining) (:4981). */
    int decide(Map<String, ServiceInstanceInfo> siMap, ModelMesh.CacheMissExcludeSet exclude, Set<String> notLive, int pick,
               long nowMs) {
        final InstanceRecord fresh = mesh.freshSelf();
        // the HashSet itself ∪ explicit (:4740-4743); loaded / failed come from the library's registry view.
        // notLive: instances the snapshot holds as live but siMap no longer contains (!siMap.containsKey(iid), :4766)
        final int bound = exclude.size() + (exclude.explicit != null ? exclude.explicit.size() : 0) + notLive.size();
        ByteBuffer x = extraPool(Math.max(bound, 1));
        int nExtra = 0;
        for (String iid : exclude) { int p = mesh.podIndexOf(iid); if (p >= 0) { x.putInt(p); nExtra++; } }
        if (exclude.explicit != null)
            for (String iid : exclude.explicit) { int p = mesh.podIndexOf(iid); if (p >= 0) { x.putInt(p); nExtra++; } }
        for (String iid : notLive) { int p = mesh.podIndexOf(iid); if (p >= 0) { x.putInt(p); nExtra++; } }

        if (mesh.modelIdsResident()) return decideKeyed(exclude, fresh, x, nExtra, pick, nowMs);
        ByteBuffer q = REQ.get(); q.clear();               // mmp_place_req, 64 bytes (include/mmplace.h)
        q.putInt(mesh.modelIndexOf(mesh.currentModelId())); // model
        q.putInt(mesh.podIndexOf(mesh.selfInstanceId()));   // self_pod
        q.putInt(exclude.favourSelf ? 1 : 0);               // flags (MMP_REQ_FAVOUR_SELF)
        q.putInt(pick);                                     // pick
        q.putLong(exclude.lastUsedTime);                    // last_used (:4951)
        q.putInt(0); q.putInt(nExtra);                      // extra_off, n_extra
        q.putLong(fresh.getLruTime()); q.putLong(fresh.getCapacity()); q.putLong(fresh.getUsed());
        q.putInt(fresh.getCount()); q.putInt(fresh.getReqsPerMinute()); // 0, InstanceRecord.java:97-109

        ByteBuffer o = OUT.get();
        MmPlace.placeBatch(mesh.handle(), q, 1, x, nExtra, nowMs, o); // throws IllegalStateException on error
        final int[] last = LAST_OUT.get();
        for (int i = 0; i < 4; i++) last[i] = o.getInt(4 * i);        // chosen, best, n_candidates, hash
        return o.getInt(0);  // read from this thread's own OUT buffer, never from shared state
    }

    private static final ThreadLocal<ByteBuffer> CALLER = ThreadLocal.withInitial(() -> MmPlace.direct(40));
    private static final ThreadLocal<ByteBuffer> REQ_C = ThreadLocal.withInitial(() -> MmPlace.direct(24));

    /** The same decision with the model named by its id: mmp_place_caller (40 bytes) + one mmp_place_req_c (24 bytes) + the id's
     *  UTF-8 bytes; the library resolves the id on the device inside the call (no modelIndexOf, no batch lock). */
    private int decideKeyed(ModelMesh.CacheMissExcludeSet exclude, InstanceRecord fresh, ByteBuffer x, int nExtra, int pick, long nowMs) {
        ByteBuffer c = CALLER.get(); c.clear();
        c.putInt(mesh.podIndexOf(mesh.selfInstanceId()));   // self_pod
        c.putInt(exclude.favourSelf ? 1 : 0);               // flags (MMP_REQ_FAVOUR_SELF)
        c.putLong(fresh.getLruTime()); c.putLong(fresh.getCapacity()); c.putLong(fresh.getUsed());
        c.putInt(fresh.getCount()); c.putInt(fresh.getReqsPerMinute());
        ByteBuffer q = REQ_C.get(); q.clear();
        q.putInt(-1);                                       // model: ignored, the key names it
        q.putInt(pick);
        q.putLong(exclude.lastUsedTime);
        q.putInt(0); q.putInt(nExtra);                      // extra_off, n_extra
        final ByteBuffer[] key = ModelKey.of(mesh.currentModelId());
        ByteBuffer o = OUT.get();
        MmPlace.placeBatchKeyed(mesh.handle(), c, q, 1, key[0], key[1], x, nExtra, nowMs, o, null);
        final int[] last = LAST_OUT.get();
        for (int i = 0; i < 4; i++) last[i] = o.getInt(4 * i);
        return o.getInt(0);
    }

    @SuppressWarnings("unchecked")
    @Override
    public <T> T getNext(Object[] sis, String method, Object[] args) {
        final ModelMesh.CacheMissExcludeSet exclude = mesh.cacheMissExcludes();
        final Map<String, ServiceInstanceInfo> siMap = getMap(sis);
        final long now = System.currentTimeMillis();
        // The reference filters on siMap membership per call (:4765-4766); the snapshot freezes liveness at commit
        // (MMP_POD_LIVE).  An instance chosen from the snapshot that siMap does not contain is excluded and the
        // decision repeated — the same walk the reference's filter would have taken.
        Set<String> notLive = java.util.Collections.emptySet();
        String chosenInstId = null;
        for (int attempt = 0;; attempt++) {
            final int chosen = decide(siMap, exclude, notLive, ThreadLocalRandom.current().nextInt(), now);
            if (chosen == MmPlace.NONE) return null;                           // :4796, :4803, :4872, :4942
            if (chosen == MmPlace.SELF) return (T) LoadBalancer.ABORT_REQUEST;  // :4894, :4932, :4990
            chosenInstId = mesh.instanceIdOf(chosen);
            if (siMap.containsKey(chosenInstId)) break;
            if (attempt == MAX_LIVE_RETRIES) return null;  // the table is far behind litelinks: let the caller retry
            if (notLive.isEmpty()) notLive = new HashSet<>();
            notLive.add(chosenInstId);
        }
        // side effects exactly as at ModelMesh.java:4992-5003
        final boolean exclusions = !exclude.isEmpty();
        if (exclusions || mesh.sendDestinationId()) {
            Map<String, String> contextMap = ModelMesh.ensureContextMapIsMutable(ThreadContext.getCurrentContext());
            if (exclusions) contextMap.put(ModelMesh.CACHE_MISS_EXCLUDES_KEY, ModelMesh.COMMA_JOIN.join(exclude));
            if (mesh.sendDestinationId()) contextMap.put(ModelMesh.DEST_INST_ID_KEY, chosenInstId);
        }
        exclude.add(chosenInstId);
        return (T) siMap.get(chosenInstId);
    }
}

/**
 * Replaces the BODY of ForwardingLB.getNext (ModelMesh.java:4315-4392), the cache-hit routing: one
 * mmp_serve_batch(n = 1) per request.  The copies of the model come from the library's registry view; the litelinks
 * counters (getInUseCount / getLastUsedTime, :4356, :4360) of THOSE copies ride in the request — O(copies) per call.
 */
class GpuForwardingLB extends ModelMesh.IdBasedLoadBalancer {
    final GpuMeshBinding mesh;
    /** chosen, chosen_load_start of the calling thread's last decision (one LB instance serves every request thread) */
    private static final ThreadLocal<long[]> LAST_OUT = ThreadLocal.withInitial(() -> new long[2]);
    long[] lastOut() { return LAST_OUT.get(); }

    GpuForwardingLB(GpuMeshBinding mesh) { this.mesh = mesh; }

    private static final ThreadLocal<ByteBuffer> REQ = ThreadLocal.withInitial(() -> MmPlace.direct(48));
    private static final ThreadLocal<ByteBuffer> OUT = ThreadLocal.withInitial(() -> MmPlace.direct(16));
    private static final ThreadLocal<ByteBuffer[]> POOLS = ThreadLocal.withInitial(() -> new ByteBuffer[4]);

    private static ByteBuffer pool(int slot, int bytes) {
        ByteBuffer[] p = POOLS.get();
        if (p[slot] == null || p[slot].capacity() < bytes) p[slot] = MmPlace.direct(Math.max(bytes, 256));
        p[slot].clear();
        return p[slot];
    }

    int decide(Map<String, ServiceInstanceInfo> siMap, ModelMesh.MapFilteringSet<String, Long> filtered, long nowMs) {
        // The reference touches litelinks' counters only for the model's copies (si.getInUseCount() / getLastUsedTime(),
        // :4356, :4360, inside the loop over filteredInstances): one mmp_serve_counter per copy that siMap lists.  A copy
        // without an entry is one litelinks does not list (sii == null -> continue, :4343-4347).  O(copies), nothing P-sized.
        final Map<String, Long> copies = filtered.map();
        ByteBuffer cnt = pool(0, 16 * Math.max(copies.size(), 1));
        int nCnt = 0;
        for (String iid : copies.keySet()) {
            final ServiceInstanceInfo sii = siMap.get(iid);
            if (sii == null) continue;
            final int p = mesh.podIndexOf(iid);
            if (p < 0) continue;
            final ServiceInstance<?> si = (ServiceInstance<?>) sii;
            cnt.putInt(16 * nCnt, p);
            cnt.putInt(16 * nCnt + 4, si.getInUseCount());
            cnt.putLong(16 * nCnt + 8, si.getLastUsedTime());
            nCnt++;
        }
        // already-tried (instance, loadStart) pairs — the MapFilteringSet's own keys — plus keyExcludes (:4278-4280);
        // an exclusion with load start Long.MIN_VALUE excludes the instance whatever its time stamp
        final Collection<String> keyExcludes = mesh.cacheHitKeyExcludes();
        final int bound = filtered.size() + (keyExcludes != null ? keyExcludes.size() : 0) + 1;
        ByteBuffer ep = pool(2, 4 * bound), et = pool(3, 8 * bound);
        int nExcl = 0;
        if (keyExcludes != null) for (String iid : keyExcludes) {
            int p = mesh.podIndexOf(iid);
            if (p >= 0) { ep.putInt(4 * nExcl, p); et.putLong(8 * nExcl, Long.MIN_VALUE); nExcl++; }
        }
        for (Map.Entry<String, Long> tried : filtered.keySet()) {
            int p = mesh.podIndexOf(tried.getKey());
            if (p >= 0) { ep.putInt(4 * nExcl, p); et.putLong(8 * nExcl, tried.getValue()); nExcl++; }
        }
        if (mesh.modelIdsResident()) return decideKeyed(filtered, cnt, nCnt, ep, et, nExcl, nowMs);
        ByteBuffer q = REQ.get(); q.clear();            // mmp_serve_req, 48 bytes
        q.putInt(mesh.modelIndexOf(mesh.currentModelId()));
        q.putInt(mesh.podIndexOf(mesh.selfInstanceId()));
        q.putInt((filtered.excludeSelf ? 1 : 0) | (filtered.preferSelf ? 2 : 0)); // MMP_SERVE_EXCLUDE_SELF | _PREFER_SELF
        q.putInt(mesh.localInvokesInFlight());
        q.putLong(mesh.lastInvokeTime());
        q.putLong(mesh.assumeCompletedAfterMillis(filtered.modelType));
        q.putInt(0); q.putInt(nExcl);                   // excl_off, n_excl
        q.putInt(0); q.putInt(nCnt);                    // cnt_off, n_cnt
        ByteBuffer o = OUT.get();
        MmPlace.serveBatch(mesh.handle(), q, 1, cnt, nCnt, ep, et, nExcl, nowMs, o);
        final long[] last = LAST_OUT.get();
        last[0] = o.getInt(0);
        last[1] = o.getLong(8);
        return o.getInt(0);
    }

    private static final ThreadLocal<ByteBuffer> CALLER = ThreadLocal.withInitial(() -> MmPlace.direct(112));
    private static final ThreadLocal<ByteBuffer> ROWS_C = ThreadLocal.withInitial(() -> MmPlace.direct(48 + 24 + 8));

    /** The same selection with the model named by its id, through the keyed route seam (there is no keyed serve-only call: the
     *  per-request seam of invokeModel is guards + serve target).  The serve row is the one decide() fills — the library builds it
     *  from mmp_seam_caller {self_pod, local_in_flight, last_invoke_time}, the gate row's exclusion range and the mmp_serve_req_c
     *  row (include/mmplace.h, THE RULE) — and the guards' half, evaluated on a row that carries that range alone, is not read. */
    private int decideKeyed(ModelMesh.MapFilteringSet<String, Long> filtered, ByteBuffer cnt, int nCnt, ByteBuffer ep, ByteBuffer et,
                            int nExcl, long nowMs) {
        ByteBuffer c = CALLER.get();
        for (int i = 0; i < 112; i += 8) c.putLong(i, 0L);
        c.putInt(0, mesh.podIndexOf(mesh.selfInstanceId()));   // self_pod
        c.putInt(96, mesh.localInvokesInFlight());             // local_in_flight
        c.putLong(104, mesh.lastInvokeTime());                 // last_invoke_time
        ByteBuffer r = ROWS_C.get();
        for (int i = 0; i < 80; i += 8) r.putLong(i, 0L);
        r.putInt(0, -1);                                       // gate row: model (ignored, the key names it)
        r.putInt(8, 0); r.putInt(12, nExcl);                   // gate row: excl_off, n_excl — the range the serve half reads
        r.putInt(48, (filtered.excludeSelf ? 1 : 0) | (filtered.preferSelf ? 2 : 0)); // serve row: flags
        r.putInt(52, 0); r.putInt(56, nCnt);                   // cnt_off, n_cnt
        r.putLong(64, mesh.assumeCompletedAfterMillis(filtered.modelType));
        final ByteBuffer gate = MmPlace.slice(r, 0, 48), serve = MmPlace.slice(r, 48, 24), gateOut = MmPlace.slice(r, 72, 8);
        final ByteBuffer[] key = ModelKey.of(mesh.currentModelId());
        ByteBuffer o = OUT.get();
        MmPlace.routeBatchKeyed(mesh.handle(), c, gate, serve, 1, key[0], key[1], cnt, nCnt, ep, et, nExcl, null, 0, nowMs,
                                ModelMesh.IN_USE_LOAD_FAILURE_EXPIRY_MS, gateOut, o, null);
        final long[] last = LAST_OUT.get();
        last[0] = o.getInt(0);
        last[1] = o.getLong(8);
        return o.getInt(0);
    }

    @SuppressWarnings("unchecked")
    @Override
    public <T> T getNext(Object[] sis, String method, Object[] args) {
        final ModelMesh.MapFilteringSet<String, Long> filtered = mesh.cacheHitExcludes();
        final Map<String, Long> filteredInstances = filtered.map();
        if (filteredInstances == null || filteredInstances.isEmpty()) return null;   // :4318-4321
        final Map<String, ServiceInstanceInfo> siMap = getMap(sis);
        final int chosen = decide(siMap, filtered, System.currentTimeMillis());
        if (chosen == MmPlace.NONE) return null;
        if (chosen == MmPlace.SELF) return (T) LoadBalancer.ABORT_REQUEST;            // :4381-4385
        final String chosenId = mesh.instanceIdOf(chosen);
        if (mesh.sendDestinationId()) {                                               // :4386-4388
            ModelMesh.ensureContextMapIsMutable(ThreadContext.getCurrentContext()).put(ModelMesh.DEST_INST_ID_KEY, chosenId);
        }
        filtered.add(chosenId, LAST_OUT.get()[1]);                                    // :4389 (this thread's own decision)
        return (T) siMap.get(chosenId);
    }
}

/** Counters of a shadow run; exported by the patch through the mesh's metrics. */
final class ShadowStats {
    final AtomicLong calls = new AtomicLong(), compared = new AtomicLong(), agree = new AtomicLong(),
            disagree = new AtomicLong(), gpuErrors = new AtomicLong();
    volatile String lastDisagreement;

    @Override
    public String toString() {
        return "shadow[calls=" + calls + " compared=" + compared + " agree=" + agree + " disagree=" + disagree
                + " gpuErrors=" + gpuErrors + (lastDisagreement != null ? " last=" + lastDisagreement : "") + "]";
    }
}

/**
 * Shadow mode for the load-target decision: the reference LB answers the request; on a sample of the calls the GPU
 * solver decides the SAME request state and the two are compared.  The reference draws its candidate with
 * ThreadLocalRandom.nextInt(remaining) (:4981), which cannot be replayed — so the solver is asked for EVERY index
 * (4 x n_candidates evenly spaced picks cover every index of any remaining <= n_candidates) and the reference's
 * choice must be one of the solver's possible choices; null / ABORT_REQUEST must match exactly, and a shortlist of
 * one must name the same instance.  This pins PLACEMENT_ORDER, the filter, the breaks and the rpm filter — the rows
 * SURVEY.md §8(c) lists as parity-unpinned — on live traffic, one JVM-equipped box, one system property.
 */
class ShadowCacheMissLB extends ModelMesh.IdBasedLoadBalancer {
    static final ShadowStats STATS = new ShadowStats();
    static final int SAMPLE_ONE_IN = Integer.getInteger("mmesh.gpu.shadow.sample", 64);
    final LoadBalancer reference;
    final GpuCacheMissLB gpu;
    final GpuMeshBinding mesh;

    ShadowCacheMissLB(LoadBalancer reference, GpuCacheMissLB gpu, GpuMeshBinding mesh) {
        this.reference = reference; this.gpu = gpu; this.mesh = mesh;
    }

    @Override
    public <T> T getNext(Object[] sis, String method, Object[] args) {
        STATS.calls.incrementAndGet();
        final boolean sample = ThreadLocalRandom.current().nextInt(SAMPLE_ONE_IN) == 0;
        final ModelMesh.CacheMissExcludeSet exclude = mesh.cacheMissExcludes();
        Set<Integer> possible = null;
        boolean sawNone = false, sawSelf = false;
        if (sample) {
            try {  // BEFORE the reference call: it adds its choice to the exclude set (:5002)
                final Map<String, ServiceInstanceInfo> siMap = getMap(sis);
                final long now = System.currentTimeMillis();
                final Set<String> none = java.util.Collections.emptySet();
                int first = gpu.decide(siMap, exclude, none, 0, now);
                final int nCand = Math.max(gpu.lastOut()[2], 1);
                possible = new HashSet<>();
                for (int j = 0, picks = 4 * nCand; j < picks; j++) {
                    int c = j == 0 ? first : gpu.decide(siMap, exclude, none, (int) ((((long) j) << 32) / picks), now);
                    if (c == MmPlace.NONE) sawNone = true; else if (c == MmPlace.SELF) sawSelf = true; else possible.add(c);
                }
            } catch (RuntimeException e) {
                STATS.gpuErrors.incrementAndGet();
                possible = null;
            }
        }
        final T ref = reference.getNext(sis, method, args);
        if (possible != null) {
            STATS.compared.incrementAndGet();
            final boolean ok;
            if (ref == null) ok = sawNone && possible.isEmpty() && !sawSelf;
            else if (ref == LoadBalancer.ABORT_REQUEST) ok = sawSelf;
            else ok = possible.contains(mesh.podIndexOf(((ServiceInstanceInfo) ref).getInstanceId()));
            if (ok) STATS.agree.incrementAndGet();
            else {
                STATS.disagree.incrementAndGet();
                STATS.lastDisagreement = "model=" + mesh.currentModelId() + " ref=" + ref + " gpu=" + possible
                        + (sawNone ? "+null" : "") + (sawSelf ? "+self" : "") + " excl=" + exclude;
            }
        }
        return ref;
    }
}

/** Shadow mode for the serve-target decision (deterministic: the two answers must be the same instance). */
class ShadowForwardingLB extends ModelMesh.IdBasedLoadBalancer {
    static final ShadowStats STATS = new ShadowStats();
    final LoadBalancer reference;
    final GpuForwardingLB gpu;
    final GpuMeshBinding mesh;

    ShadowForwardingLB(LoadBalancer reference, GpuForwardingLB gpu, GpuMeshBinding mesh) {
        this.reference = reference; this.gpu = gpu; this.mesh = mesh;
    }

    @Override
    public <T> T getNext(Object[] sis, String method, Object[] args) {
        STATS.calls.incrementAndGet();
        final ModelMesh.MapFilteringSet<String, Long> filtered = mesh.cacheHitExcludes();
        int chosen = Integer.MIN_VALUE;
        if (ThreadLocalRandom.current().nextInt(ShadowCacheMissLB.SAMPLE_ONE_IN) == 0
                && filtered.map() != null && !filtered.map().isEmpty()) {
            try {  // before the reference adds its choice to the filtering set (:4389)
                chosen = gpu.decide(getMap(sis), filtered, System.currentTimeMillis());
            } catch (RuntimeException e) {
                STATS.gpuErrors.incrementAndGet();
            }
        }
        final T ref = reference.getNext(sis, method, args);
        if (chosen != Integer.MIN_VALUE) {
            STATS.compared.incrementAndGet();
            final int refIdx = ref == null ? MmPlace.NONE : ref == LoadBalancer.ABORT_REQUEST ? MmPlace.SELF
                    : mesh.podIndexOf(((ServiceInstanceInfo) ref).getInstanceId());
            if (refIdx == chosen) STATS.agree.incrementAndGet();
            else {
                STATS.disagree.incrementAndGet();
                STATS.lastDisagreement = "model=" + mesh.currentModelId() + " ref=" + refIdx + " gpu=" + chosen;
            }
        }
        return ref;
    }
}
