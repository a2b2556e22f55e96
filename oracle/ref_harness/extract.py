#!/usr/bin/env python3
"""Reference-text extractor of the `oracle/_ref` harness (test infrastructure, never shipped).

The reference is Java and neither box has a JDK (profiles/r3/jdk_probe_*.txt), so its load-target / serve-target
selection cannot be RUN as Java.  What can be done: take the reference's own method bodies, verbatim by line range, from
where they lie under /root/reference, and compile THAT TEXT with g++ against a small header of stand-ins for the Java /
Guava / eclipse-collections / litelinks types it names (javastub.hpp).  The decision logic that executes is then the
reference's own statements, in its own order, with its own constants — not a restatement.

Nothing of the reference is copied into the repository: this script writes the extracted text into oracle/_ref/gen/
(git-ignored, rebuilt from /root/reference by build.sh each time).

What the rewrite does to the text is TOKEN-LEVEL ONLY, listed exhaustively in RULES below; every rule is a syntax
difference between Java and C++, none knows anything about placement.  After rewriting, the script checks that every
non-blank source line of every range survives in the output up to those rules (same count of lines).
"""
import os
import re
import sys

REF = os.environ.get("MMP_REFERENCE", "/root/reference")
MM = "src/main/java/com/ibm/watson/modelmesh/ModelMesh.java"
IR = "src/main/java/com/ibm/watson/modelmesh/InstanceRecord.java"
UT = "src/main/java/com/ibm/watson/modelmesh/Utils.java"

# (output name, file, first line, last line, first line must contain, last line must contain): bodies only —
# the enclosing Java declaration (generics on methods, annotations, anonymous classes) is supplied by harness.cc
RANGES = [
    ("isFull_body", MM, 4641, 4641, "return availableUnits < minSpaceUnits;", "minSpaceUnits"),
    ("placement_order_compare_body", MM, 4649, 4701, "InstanceRecord ir1 = e1.getValue()", ".result();"),
    ("isExcluded_body", MM, 4741, 4742, "return contains(instanceId)", "explicit.contains(instanceId)"),
    ("filter_body", MM, 4763, 4771, "return Iterators.filter(clusterState.iterator()", "});"),
    ("cachemiss_getNext_body", MM, 4777, 5003, "final CacheMissExcludeSet exclude = cacheMissExcludeTl.get();",
     "return (T) siMap.get(chosenInstId);"),
    ("forwarding_getNext_body", MM, 4316, 4391, "final MapFilteringSet<String, Long> filtered", "return (T) chosen;"),
    ("mapfilteringset_apply_body", MM, 4282, 4282, "return !containsKey(input)", "keyExcludes.contains"),
    ("age_body", MM, 4163, 4163, "return timeMillis == 0 ? 0L", "currentTimeMillis() - timeMillis"),
    ("getRemaining_body", IR, 204, 204, "return Math.max(0L, capacity - used);", "capacity - used"),
    ("string_array_comp_body", UT, 26, 35, "int diff = l1.length - l2.length;", "return 0;"),
    ("lb_constants", MM, 4751, 4753, "TWELVE_MIN_MS = MILLISECONDS.convert(12, MINUTES);", "FIVE_DAYS_MS = MILLISECONDS.convert(5, DAYS);"),
    # ---- the request-level guards around the two selections
    ("publish_constants", MM, 231, 232, "INSTANCE_REC_PUBLISH_FREQ_MS = 40_000L;", "INSTANCE_REC_PUBLISH_MIN_PERIOD_MS = 2_000L;"),
    ("failure_constants", MM, 222, 224, "MAX_LOAD_FAILURES = 3;", "MAX_LOAD_LOCATIONS = 5;"),
    ("goLocal_fragment", MM, 3599, 3626, "int filteredCount = filteredInstances.size();", "}"),
    ("oldest_body", MM, 4167, 4167, "return Collections.min(instances.values());", "instances.values()"),
    ("getMostRecent_body", MM, 4630, 4636, "Entry<String, Long> mostRecent = null;", "return mostRecent != null ? mostRecent.getKey() : null;"),
    ("checkLoadLocationCount_body", MM, 4593, 4603, "int count = 0;", "}"),
    ("checkLoadFailureCount_body", MM, 4609, 4626, "Map<String, Long> failedInInstances = mr.getLoadFailedInstanceIds();", "}"),
    ("throwIfLocalLoadNotAllowed_body", MM, 4011, 4041, "boolean localFiltered = loadTargetFilter != null", "}"),
    ("churn_fragment", MM, 3872, 3884, "if (minChurnAgeMs > 0) {", "}"),
    ("weightPredictCutoff_body", MM, 5014, 5014, "return (loadingThreads + (loadingThreads / 3));", "loadingThreads / 3"),
    ("loadLocal_sizing_fragment", MM, 5159, 5197, "int initialSize = 0;", "}"),
    ("onEviction_attempt_fragment", MM, 2886, 2897, "boolean attemptReload = false, inRegistry = false, failed = ce.isFailed();", "}"),
    ("onEviction_cluster_fragment", MM, 2918, 2920, "ClusterStats stats = typeSetStats(ce.modelInfo.getServiceType());",
     "&& ((20L * stats.totalFree) / stats.totalCapacity) >= 1) {"),
    # publishInstanceRecord's decision, without lines 5409-5422: `if (unloadManager != null) { lock; try {...} finally {...}; cap -= ...}`
    # (C++ has no `finally`; the request's fresh_* fields ARE the values after that adjustment, include/mmplace.h mmp_gate_req)
    ("publish_fragment_a", MM, 5395, 5408, "long now = currentTimeMillis(), lastDone = now - lastPublished;", "long totalCacheOccupancy = -1;"),
    ("publish_fragment_b", MM, 5423, 5468, "if (oldest == -1L) {", "}"),
    ("loadingChange_body", MM, 5537, 5542, "int curInProg = curRec.getLoadingInProgress();", "return Math.abs(loadInProg - curInProg) >= 3;"),
    ("loadChange_body", MM, 5547, 5549, "int diff = Math.abs(curRecRpms - rpms);", "(100 * diff) / curRecRpms > 10);"),
    # ---- a15: rateTrackingTask (the scale-up planner), getExcludeSet, loadedSince.  The `try {` / `} catch ... finally {`
    # lines around the loop body (5656, 5686-5687, 5807-5813) are Java plumbing with no C++ counterpart: the body is taken
    # from inside them
    # MaxConcCacheEntry.getRpmScaleThreshold (limitModelConcurrency == true: the per-model threshold of the latency-based rate task, :5704,
    # and of the janitor, :6295) and the constants it reads
    ("mcce_count_bits", MM, 2653, 2653, "private static final int COUNT_BITS = 21;", "COUNT_BITS = 21;", "member_consts"),
    ("mcce_count_mask", MM, 2760, 2760, "static final long COUNT_MASK = (1 << COUNT_BITS) - 1;", "COUNT_MASK", "member_consts"),
    ("mcce_getRpmScaleThreshold_body", MM, 2767, 2795, "long curVal = countAndTimeSum.sum(), timeSum;",
     "return (int) ((maxConc * (count * dynamicRpmScaleConstant)) / timeSum);", "ushr"),
    ("ratetask_prologue_a", MM, 5641, 5654, "final long lastTime = lastCheckTime, now = currentTimeMillis();", "final int upper = iterationCounter - secondCopyMinAgeIters;"),
    ("ratetask_prologue_b", MM, 5657, 5685, "int instCount = clusterStats.instanceCount;", "int modelParallelismSum = 0;"),
    ("ratetask_loop_body", MM, 5688, 5806, "modelId = ent.getKey();", "copiesToLoad - 1);"),
    ("ratetask_epilogue", MM, 5815, 5818, "if (latencyBased) {", "}"),
    ("getExcludeSet_body", MM, 5836, 5855, "int scaleUpRpms = limitModelConcurrency", "return excludeSet != null ? excludeSet : Collections.emptySet();"),
    ("loadedSince_body", MM, 5861, 5870, "for (Entry<String, Long> entry : mr.getInstanceIds().entrySet()) {", "return false;"),
    # ---- a16: the janitor's scale-down of model copies
    ("janitor_scaledown_fragment", MM, 6111, 6140, "if (shuttingDown) {", "}"),
    ("removeModelCopies_body", MM, 6199, 6309, "if (lastUsed == 0L) {", "return false;"),
    ("removeSecondModelCopy_body", MM, 6318, 6334, "if (otherValidInstance == null) {", "return removeLocalModelCopyAsync(modelId, mr, ce, lastUsed);"),
    ("getRpm_body", MM, 1739, 1740, "long countSinceLastTime = getIntervalCount();", "(60_000L * countSinceLastTime) / timeSinceLastCheck;"),
    ("second_copy_remove_constant", MM, 257, 257, "SECOND_COPY_REMOVE_MAX_AGE_MS = 10 * 3600_000L;", "10hours"),
    # ---- a5: the instance-table listener and the cluster's aggregate stats
    ("ist_resetLru_body", "src/main/java/com/ibm/watson/modelmesh/InstanceSetStatsTracker.java", 54, 54, "lru = Long.MAX_VALUE;", "MAX_VALUE;"),
    ("ist_addLru_body", "src/main/java/com/ibm/watson/modelmesh/InstanceSetStatsTracker.java", 58, 60, "if (lru > 0L && lru < this.lru) {", "}"),
    ("ist_add_body", "src/main/java/com/ibm/watson/modelmesh/InstanceSetStatsTracker.java", 64, 71, "count++;", "}"),
    ("ist_remove_body", "src/main/java/com/ibm/watson/modelmesh/InstanceSetStatsTracker.java", 75, 83, "count--;", "return count <= 0;"),
    ("ist_update_body", "src/main/java/com/ibm/watson/modelmesh/InstanceSetStatsTracker.java", 87, 91, "ClusterStats newStats = new ClusterStats(totalCapacity, totalFree, lru, count, modelCount);", "return newStats;"),
    ("handleInstanceTableChange_body", MM, 1456, 1567, "if (logger.isDebugEnabled()) {", "}", "LISTENER_SWITCH"),
    # ---- a21: preShutdown — which local copies get a new copy elsewhere, and which of those the shutdown waits for
    ("preshutdown_cutoff_constant", MM, 276, 276, "CUTOFF_AGE_MS = 60 * 60_000L;", "1 hour"),
    ("preshutdown_migration_fragment", MM, 6998, 7046, "List<Future<Entry<String, Long>>> waitFor = new ArrayList<>(cacheEntries.size());", "}", "SHUTDOWN"),
    # ---- a18: TypeConstraintManager — the per-type instance sets, the instance partitions and their stats (the static computation:
    # typeMappingsUpdated's building blocks; the incremental updateInstance path is not extracted)
    ("tcm_partition_stats_comp_body", "src/main/java/com/ibm/watson/modelmesh/TypeConstraintManager.java", 265, 270, "ClusterStats cs1 = isst1.currentStats, cs2 = isst2.currentStats;", "return Long.compare(cs2.totalCapacity, cs1.totalCapacity);", "TCM"),
    ("tcm_candidateSubsetStats_body", "src/main/java/com/ibm/watson/modelmesh/TypeConstraintManager.java", 357, 375, "if (instanceSetStats == null) {", "return new ClusterStats(capacity, free, lru, count, modelCopyCount);", "TCM"),
    ("tcm_fromInstanceSet_body", "src/main/java/com/ibm/watson/modelmesh/TypeConstraintManager.java", 419, 447, "// assumption is that requiredLabels and preferredLabels are already sorted", "requiredInstances, preferredSet, instanceSetStats, preferredSet);", "TCM"),
    ("tcm_allowedOnInstance_body", "src/main/java/com/ibm/watson/modelmesh/TypeConstraintManager.java", 451, 451, "return allowedInstances == null || allowedInstances.contains(iid);", "contains(iid);", "TCM"),
    ("tcm_instanceMatches_body", "src/main/java/com/ibm/watson/modelmesh/TypeConstraintManager.java", 480, 485, "if (instanceLabels.length == 0 || typeLabels.length == 0) {", "labelStream.anyMatch(hasLabel);", "TCM"),
    ("tcm_prohibited_types_fragment", "src/main/java/com/ibm/watson/modelmesh/TypeConstraintManager.java", 561, 567, "ArrayList<String> newPts = new ArrayList<>(tcMap.size());", "ProhibitedTypeSet pts = new ProhibitedTypeSet(newPts);", "TCM"),
    ("tcm_scores_fragment", "src/main/java/com/ibm/watson/modelmesh/TypeConstraintManager.java", 684, 699, "MutableObjectIntMap<String> instanceScores", "Set<String> defaultPreferred = inferPreferredInstances(instanceScores, null);", "TCM"),
    ("tcm_per_type_fragment", "src/main/java/com/ibm/watson/modelmesh/TypeConstraintManager.java", 707, 723, "for (Map.Entry<String, ModelTypeConstraints> ent : mtcMap.entrySet()) {", "}", "TCM"),
    ("tcm_inferPreferredInstances_body", "src/main/java/com/ibm/watson/modelmesh/TypeConstraintManager.java", 728, 746, "Set<String> instanceIds = new HashSet<>(include != null ? include.size() : 8);", "return min < max ? ImmutableSet.copyOf(instanceIds) : null;", "TCM"),
    # ---- a19: UpgradeTracker (replica sets that a rolling update is replacing)
    ("upgrade_constants", "src/main/java/com/ibm/watson/modelmesh/UpgradeTracker.java", 48, 50, "TEN_MINS = 600_000L;", "TWENTY_MINS = 1200_000L;"),
    ("upgrade_instanceRemoved_body", "src/main/java/com/ibm/watson/modelmesh/UpgradeTracker.java", 86, 114, "if (iid.length() < 7) {", "}", "STREAMS"),
    ("upgrade_instanceAdded_body", "src/main/java/com/ibm/watson/modelmesh/UpgradeTracker.java", 121, 186, "if (iid.length() < 7) {", "}", "STREAMS"),
    ("upgrade_doHousekeeping_body", "src/main/java/com/ibm/watson/modelmesh/UpgradeTracker.java", 193, 200, "// Check for and remove expired entries", "}", "STREAMS"),
    # ---- a17: the leader's reaper — proactive loading of unloaded models
    ("modeltoload_compareTo_body", MM, 6407, 6407, "return Long.compare(m.lastUsed, lastUsed);", "lastUsed);"),
    ("reaper_candidates_prologue", MM, 6456, 6463, "ClusterStats globalStats = clusterStats;", "}"),
    ("reaper_candidate_rule", MM, 6574, 6577, "if (proactiveLoadCandidates != null && insts.isEmpty() && failInsts.size() < 2", "}"),
    ("reaper_dispatch_fragment", MM, 6473, 6489, "if (typeConstraints == null) {", "}"),
    ("triggerProactiveLoads_body", MM, 6619, 6746, "// get free units", "}"),
]

# ---- a12 / a13: the local cache — clhm (the timestamp-ordered weighted LRU) and ModelCacheUnloadBufManager, plus the three
# ModelMesh fragments that tie them together (CacheEntry's weight, the internal entry, the eviction callback's accounting).
# Compiled by clhm_harness.cc (a second binary: the cache is self-contained).  Single-threaded: the read buffers are drained
# by the reading thread itself (tryLock succeeds), which is the reference's own code path, not an assumption of the harness
CL = "src/main/java/com/ibm/watson/modelmesh/clhm/ConcurrentLinkedHashMap.java"
LD = "src/main/java/com/ibm/watson/modelmesh/clhm/LinkedDeque.java"
UB = "src/main/java/com/ibm/watson/modelmesh/ModelCacheUnloadBufManager.java"
CLHM_RANGES = [
    ("clhm_constants", CL, 164, 182, "MAXIMUM_CAPACITY = Long.MAX_VALUE - Integer.MAX_VALUE;", "READ_BUFFER_INDEX_MASK = READ_BUFFER_SIZE - 1;", "CLHM"),
    ("clhm_capacity_body", CL, 295, 295, "return capacity.get();", "capacity.get();", "CLHM"),
    ("clhm_setCapacity_body", CL, 306, 315, "checkArgument(capacity >= 0);", "}", "CLHM"),
    ("clhm_hasOverflowed_body", CL, 321, 321, "return weightedSize.get() > capacity.get();", "capacity.get();", "CLHM"),
    ("clhm_evict_body", CL, 336, 351, "while (hasOverflowed()) {", "}", "CLHM"),
    ("clhm_afterRead_body", CL, 383, 386, "final Object record = lastUsed > 0L ? new ReadRecord(node, lastUsed) : node;", "drainOnReadIfNeeded(bufferIndex, writeCount);", "CLHM"),
    ("clhm_readBufferIndex_body", CL, 394, 394, "return ((int) Thread.currentThread().getId()) & READ_BUFFERS_MASK;", "READ_BUFFERS_MASK;", "CLHM"),
    ("clhm_recordRead_body", CL, 408, 415, "final AtomicLong counter = readBufferWriteCount[bufferIndex];", "return writeCount;", "CLHM"),
    ("clhm_drainOnReadIfNeeded_body", CL, 426, 430, "final long pending = (writeCount - readBufferDrainAtWriteCount[bufferIndex].get());", "}", "CLHM"),
    ("clhm_afterWrite_body", CL, 439, 451, "evictionLock.lock();", "}", "CLHM"),
    ("clhm_tryToDrainBuffers_body", CL, 459, 468, "if (evictionLock.tryLock()) {", "}", "CLHM"),
    ("clhm_drainBuffers_body", CL, 474, 478, "final int start = (int) Thread.currentThread().getId();", "}", "CLHM"),
    ("clhm_drainReadBuffer_body", CL, 484, 508, "final long writeCount = readBufferWriteCount[bufferIndex].get();", "readBufferDrainAtWriteCount[bufferIndex].lazySet(writeCount);", "CLHM"),
    ("clhm_applyRead_body", CL, 514, 521, "// An entry may be scheduled for reordering despite having been removed.", "}", "CLHM"),
    ("clhm_tryToRetire_body", CL, 533, 537, "if (expect.isAlive()) {", "return false;", "CLHM"),
    ("clhm_makeRetired_body", CL, 547, 556, "for (;;) {", "}", "CLHM"),
    ("clhm_makeDead_body", CL, 567, 574, "for (;;) {", "}", "CLHM"),
    ("clhm_notifyListener_body", CL, 579, 586, "Node<K, V> node;", "}", "CLHM"),
    ("clhm_AddTask_run_body", CL, 602, 609, "weightedSize.lazySet(weightedSize.get() + weight);", "}", "CLHM"),
    ("clhm_RemovalTask_run_body", CL, 624, 626, "// add may not have been processed yet", "makeDead(node);", "CLHM"),
    ("clhm_UpdateTask_run_body", CL, 645, 650, "weightedSize.lazySet(weightedSize.get() + weightDifference);", "evict();", "CLHM"),
    ("clhm_weightedSize_body", CL, 672, 672, "return Math.max(0, weightedSize.get());", "weightedSize.get());", "CLHM"),
    ("clhm_get_body", CL, 729, 734, "final Node<K, V> node = data.get(key);", "return node.getValue();", "CLHM"),
    ("clhm_getQuietly_body", CL, 785, 786, "final Node<K, V> node = data.get(key);", "return (node == null) ? null : node.getValue();", "CLHM"),
    ("clhm_putIfAbsent3_body", CL, 807, 807, "return put(key, value, lastUsed, true);", "true);", "CLHM"),
    ("clhm_put_body", CL, 822, 857, "checkNotNull(key);", "}", "CLHM"),
    ("clhm_remove_body", CL, 862, 869, "final Node<K, V> node = data.remove(key);", "return node.getValue();", "CLHM"),
    ("clhm_remove2_body", CL, 874, 897, "final Node<K, V> node = data.get(key);", "}", "CLHM"),
    ("clhm_replaceQuietly_body", CL, 961, 984, "checkNotNull(key);", "}", "CLHM"),
    ("clhm_oldestTime_body", CL, 1126, 1126, "return oldestTime;", "oldestTime;", "CLHM"),
    ("clhm_updateOldestTime_body", CL, 1131, 1132, "final Node<K, V> first = evictionDeque.peekFirst();", "EMPTY_OLDEST_TIME;", "CLHM"),
    ("clhm_wv_contains_body", CL, 1307, 1307, "return (o == value) || value.equals(o);", "value.equals(o);", "CLHM"),
    ("clhm_wv_isAlive_body", CL, 1314, 1314, "return weight > 0;", "weight > 0;", "CLHM"),
    ("clhm_node_touch_body", CL, 1358, 1359, "lastUsed = time == 0L ? System.currentTimeMillis()", ": Math.max(lastUsed, time);", "CLHM"),
    ("clhm_node_getLastUsed_body", CL, 1364, 1364, "return lastUsed;", "lastUsed;", "CLHM"),
    ("clhm_node_getValue_body", CL, 1393, 1393, "return get().value;", "get().value;", "CLHM"),
    ("deque_linkFirst_body", LD, 89, 97, "final E f = first;", "}", "CLHM"),
    ("deque_unlinkFirst_body", LD, 120, 130, "final E f = first;", "return f;", "CLHM"),
    ("deque_unlink_body", LD, 149, 164, "final E prev = e.getPrevious();", "}", "CLHM"),
    ("deque_isEmpty_body", LD, 169, 169, "return (first == null);", "null);", "CLHM"),
    ("deque_contains_body", LD, 211, 213, "return (e.getPrevious() != null)", "|| (e == first);", "CLHM"),
    ("deque_reposition_body", LD, 244, 254, "final long lu = e.getLastUsed();", "insert(e);", "CLHM"),
    ("deque_insert_body", LD, 259, 287, "if(contains(e)) return false;", "}", "CLHM"),
    ("deque_peekFirst_body", LD, 299, 299, "return first;", "first;", "CLHM"),
    ("deque_poll_body", LD, 369, 369, "return pollFirst();", "pollFirst();", "CLHM"),
    ("deque_pollFirst_body", LD, 374, 374, "return isEmpty() ? null : unlinkFirst();", "unlinkFirst();", "CLHM"),
    ("deque_remove_body", LD, 395, 399, "if (contains(e)) {", "return false;", "CLHM"),
    ("ubm_key_constant", UB, 41, 41, 'UNLOAD_BUFFER_CACHE_KEY = "___UNLOADBUF";', "___UNLOADBUF", "CLHM"),
    ("ubm_ctor_body", UB, 83, 87, "this.runtimeCache = cache;", "this.cacheLockCondition = cacheLock.newCondition();", "CLHM"),
    ("ubm_getAdjustedCacheCapacity_body", UB, 91, 91, "return runtimeCache.capacity() - UNLOAD_BUFF.getWeight();", "getWeight();", "CLHM"),
    ("ubm_getUnloadBufferWeight_body", UB, 95, 95, "return UNLOAD_BUFF.getWeight();", "getWeight();", "CLHM"),
    ("ubm_insertNewEntry_body", UB, 131, 144, "final int weight = ce.getWeight();", "}", "CLHM"),
    ("ubm_adjustNewEntrySpaceRequest_body", UB, 153, 165, "final int newWeight = entry.getWeight() + increase;", "}", "CLHM"),
    ("ubm_claimRequestedSpaceIfReady_body", UB, 204, 213, "cacheLock.lock();", "return false;", "CLHM"),
    ("ubm_adjustWeightAfterLoad_body", UB, 225, 245, "if (delta == 0) return;", "}", "CLHM"),
    ("ubm_insertFailedPlaceholderEntry_body", UB, 250, 273, "final int weight = ce.getWeight();", "}", "CLHM"),
    ("ubm_removeEntry_body", UB, 282, 296, "String modelId = entry.modelId;", "}", "CLHM"),
    ("ubm_entryRemoved_body", UB, 307, 309, "assert weight > 0;", "adjustAggregateUnloadingWeight(weight);", "CLHM"),
    ("ubm_unloadComplete_body", UB, 313, 331, "assert weight > 0;", "+ newCapacity);", "CLHM"),
    ("ubm_discardFailedEntry_body", UB, 335, 341, "cacheLock.lock();", "}", "CLHM"),
    ("ubm_cacheRemaining_body", UB, 348, 348, "return (int) Math.min(runtimeCache.capacity() - runtimeCache.weightedSize(), Integer.MAX_VALUE);", "MAX_VALUE);", "CLHM"),
    ("ubm_payDownDeficit_body", UB, 353, 366, "assert weight > 0;", "}", "CLHM"),
    ("ubm_adjustTotalModelCacheOccupancy_body", UB, 371, 371, "totalModelCacheOccupancy += delta;", "delta;", "CLHM"),
    ("ubm_adjustAggregateUnloadingWeight_body", UB, 376, 391, "if (delta == 0) return;", "UNLOAD_BUFF.updateWeightLocked(newWeight);", "CLHM"),
    ("ubm_cacheSpaceIsReady_body", UB, 396, 401, "int newTuw = totalUnloadingWeight + required;", "return totalRequired <= runtimeCache.capacity();", "CLHM"),
    ("mm_ce_getWeight_body", MM, 1759, 1759, "return Math.abs(weight);", "abs(weight);", "CLHM"),
    ("mm_ce_updateWeightLocked_body", MM, 1779, 1786, "int oldWeight = this.weight;", "}", "CLHM"),
    ("mm_newInternalCacheEntry_body", MM, 1618, 1621, "CacheEntry<?> ce = new CacheEntry(id, weight);", "return ce;", "CLHM"),
    ("mm_onEviction_weight_fragment", MM, 2871, 2871, "int removalWeight = ce.getWeight();", "getWeight();", "CLHM"),
    ("mm_onEviction_manager_fragment", MM, 2876, 2878, "if (unloadManager != null) {", "}", "CLHM"),
]


# ---- a18 (incremental) + a5 with type constraints: TypeConstraintManager as the instance-table listener drives it — instanceAdded /
# instanceRemoved / instanceUpdated / updateInstance / updateInstanceSet / getInstanceSetStats / refreshPerTypeInstanceSets /
# updateInstanceSetStats / typeMappingsUpdated and the accessors the mesh reads — compiled by tcm_harness.cc (a third binary)
TC = "src/main/java/com/ibm/watson/modelmesh/TypeConstraintManager.java"
IS = "src/main/java/com/ibm/watson/modelmesh/InstanceSetStatsTracker.java"
TCMI_RANGES = [
    ("tcmi_default_type_constant", TC, 67, 67, 'DEFAULT_TYPE_MAPPING = "_default";', "_default", "TCMI"),
    ("tcmi_cfg_isEmpty_body", TC, 85, 85, "return empty(required) && empty(preferred);", "empty(preferred);", "TCMI"),
    ("tcmi_getTypeSetStats_body", TC, 231, 232, "ModelTypeConstraints mtc = typeConstraintsMap.get(type);", "return mtc != null ? mtc.candidateSubsetStats() : null;", "TCMI"),
    ("tcmi_getLocalInstanceSetStats_body", TC, 237, 238, "InstanceSetStatsTracker liss = localInstanceSetStats;", "EMPTY_STATS;", "TCMI"),
    ("tcmi_getCandidateInstances_body", TC, 243, 244, "ModelTypeConstraints mtc = getTypeConstraints(type);", "return mtc != null ? mtc.allowedInstances : null;", "TCMI"),
    ("tcmi_getPreferredInstances_body", TC, 249, 250, "ModelTypeConstraints mtc = getTypeConstraints(type);", "defaultPreferredInstances;", "TCMI"),
    ("tcmi_getTypeConstraints_body", TC, 259, 261, "final Map<String, ModelTypeConstraints> tcm = typeConstraintsMap;", "tcm.get(DEFAULT_TYPE_MAPPING);", "TCMI"),
    ("tcmi_mtc_ctor_body", TC, 382, 387, "this.requiredLabels = requiredLabels;", "this.instanceSetStats = instanceSetStats;", "TCMI"),
    ("tcmi_updateInstanceSetStats_body", TC, 397, 413, "boolean inferredMatch = Objects.equal(preferredInstances, newInferredPreferred);", "allowedInstances, configuredPreferredInstances, newStatArray, newInferredPreferred);", "TCMI"),
    ("tcmi_labelsMatch_body", TC, 458, 459, "return Arrays.equals(requiredLabels, required)", "&& Arrays.equals(preferredLabels, preferred);", "TCMI"),
    ("tcmi_updateInstance_body", TC, 464, 474, "Set<String> newReqInstances = allowedInstances;", "newReqInstances, newPrefInstances, instanceSetStats, newPrefInstances);", "TCMI"),
    ("tcmi_updateInstanceSet_body", TC, 491, 504, "boolean curMatch = instanceSet != null && instanceSet.contains(iid);", "return instanceSet;", "TCMI"),
    ("tcmi_getStatsForLabels_body", TC, 509, 509, "return labelsToInstanceSetStats.get(labels);", "get(labels);", "TCMI"),
    ("tcmi_instanceAdded_body", TC, 514, 524, "assert labels != null;", "return instanceSetStats;", "TCMI"),
    ("tcmi_instanceRemoved_body", TC, 528, 548, "final Map<String, ModelTypeConstraints> mtcMap = typeConstraintsMap;", "}", "TCMI"),
    ("tcmi_getInstanceSetStats_body", TC, 559, 578, "InstanceSetStatsTracker instanceSetStats = labelsToInstanceSetStats.get(labels);", "return instanceSetStats;", "TCMI"),
    ("tcmi_instanceUpdated_body", TC, 583, 599, "HashMap<String, ModelTypeConstraints> newMap = null;", "return newMap != null ? newMap : mtcMap;", "TCMI"),
    ("tcmi_typeMappingsUpdated_body", TC, 608, 667, "Map<String, ModelTypeConstraints> mtcMap = typeConstraintsMap, newMap = null;", "}", "TCMI"),
    ("tcmi_refreshPerTypeInstanceSets_body", TC, 684, 724, "MutableObjectIntMap<String> instanceScores", "return mtcMap;", "TCMI"),
    ("tcmi_ist_getInstanceCount_body", IS, 50, 50, "return count;", "count;", "TCMI"),
    ("tcmi_ist_ctor_body", IS, 45, 46, "this.prohibitedTypesSet = prohibitedTypesSet;", "this.isFull = isFull;", "TCMI"),
    ("tcmi_typeSetStats_body", MM, 1433, 1437, "if (typeConstraints == null) {", "return stats != null ? stats : clusterStats;", "TCMI"),
    ("tcmi_instanceSetStats_body", MM, 1447, 1447, "return typeConstraints != null ? typeConstraints.getLocalInstanceSetStats() : clusterStats;", "clusterStats;", "TCMI"),
]


# ---- a16' / a17': the janitor's cache loop and registry loop, pruneModelRegistry with pruneMissingInstances, and the ModelRecord
# methods they call — compiled by registry_harness.cc (a fourth binary).  The registry loop is cut in two: :6014-6107 and its last
# line (:6108, the `}` that closes the `for`), so that the harness can put the target of `continue registryLoop` between them
MR = "src/main/java/com/ibm/watson/modelmesh/ModelRecord.java"
REG_RANGES = [
    ("reg_failure_expiry_constants", MM, 219, 221, "LOAD_FAILURE_EXPIRY_MS = getLongParameter(LOAD_FAILURE_EXPIRY_ENV_VAR, 900_000L);",
     "IN_USE_LOAD_FAILURE_EXPIRY_MS = LOAD_FAILURE_EXPIRY_MS / 2;", "REG"),
    ("reg_janitor_freq_constant", MM, 235, 235, 'LOCAL_JANITOR_FREQ_SECS = Long.getLong("tas.janitor_freq_secs", 6 * 60);', "6mins", "REG"),
    ("reg_lastused_age_constant", MM, 266, 266, "LASTUSED_AGE_ON_ADD_MS = 3600_000;", "1hour", "REG"),
    ("reg_gone_after_constant", MM, 270, 270, "ASSUME_INSTANCE_GONE_AFTER_MS = 10 * 60_000L;", "10min", "REG"),
    ("reg_short_expiry_constant", MM, 280, 280, "SHORT_EXPIRY_RECENT_USE_TIME_MS = 3 * 60_000L;", "3mins", "REG"),
    ("reg_ce_states", MM, 1841, 1848, "NEW = 0,", "REMOVED = 7;", "REG"),
    ("reg_unloadAttemptedRecently_body", MM, 1865, 1865, "return age(lastUnloadAttemptTime) < 600_000L;", "10 mins", "REG"),
    ("reg_janitor_cache_loop", MM, 5892, 6008, "Map<String, CacheEntry<?>> cacheEntries = runtimeCache.descendingMap();", "}", "REG"),
    ("reg_janitor_between_loops", MM, 6010, 6013, "if (shuttingDown) {", "before = nanoTime();", "REG"),
    ("reg_janitor_registry_loop", MM, 6014, 6107, "// find references to this instance in the registry and prune where necessary", "}", "REG"),
    ("reg_janitor_registry_loop_close", MM, 6108, 6108, "}", "}", "REG"),  # the brace that closes the `for`
    ("reg_updateIfStale_body", MM, 6167, 6184, "if (lastUsed == Long.MAX_VALUE) {", "}", "REG"),
    ("reg_repairLastUsed_body", MM, 6843, 6849, "if (mr != null && mr.getLastUsed() == Long.MAX_VALUE) {", "}", "REG"),
    ("reg_value_comp_body", MM, 6876, 6880, "Long l1 = e1.getValue(), l2 = e2.getValue();", "return l1.compareTo(l2);", "REG"),
    ("reg_prune_body", MM, 6529, 6608, "int kvConnectionErrorCount = 0;", "return true;", "REG"),
    ("reg_pruneMissing_body", MM, 6754, 6783, "if (instances.isEmpty()) {", "return modCount;", "REG"),
    ("reg_mr_removeLoadFailure_body", MR, 170, 170, "return loadFailedInstanceIds.remove(instanceId) != null | failures.remove(instanceId) != null;",
     "!= null;", "REG"),
    ("reg_mr_getLastUsed_body", MR, 229, 229, "return lastUsed;", "lastUsed;", "REG"),
    ("reg_mr_setLastUsed_body", MR, 233, 233, "this.lastUsed = lastUsed;", "lastUsed;", "REG"),
    ("reg_mr_updateLastUsed_body", MR, 240, 245, "if (lastUsed == 0L) {", "}", "REG"),
    ("reg_mr_updateLastUnloadTime_body", MR, 261, 261, "this.lastUnloadTime = instanceIds.size() <= 2 ? 0L : System.currentTimeMillis();",
     "currentTimeMillis();", "REG"),
]

# The one control-flow rewrite: the listener's `switch (type)` (MM.java:1474-1563) declares locals in `case ENTRY_UPDATED` and
# falls through into `case ENTRY_DELETED`; C++ forbids the jump past those initialisations that a direct entry at the second
# label would be.  Its four label lines become the equivalent if-chain (ADDED/UPDATED run both blocks, DELETED the second,
# anything else nothing); every statement between them stays the reference's text.
EXTRA_RULES = {
    # constant declarations of a nested class: the member modifiers in front of them
    "member_consts": [
        (re.compile(r"^\s*(?:private\s+)?static\s+final\s+"), "static const "),
    ],
    # the unsigned right shift of a long does not exist in C++: `x >>> n` -> JUSHR(x, n)  (only in the body that uses it: elsewhere
    # `>>>` closes three generic brackets)
    "ushr": [
        (re.compile(r"\b(\w+)\s*>>>\s*(\w+)\b"), r"JUSHR(\1, \2)"),
    ],
    "LISTENER_SWITCH": [
        (re.compile(r"^(\s*)switch \(type\) \{\s*$"), r"\1const EventType sw_type = type;  // switch (type) {"),
        (re.compile(r"^(\s*)case ENTRY_ADDED:\s*$"), r"\1if (sw_type == ENTRY_ADDED || sw_type == ENTRY_UPDATED) {  // case ENTRY_ADDED:"),
        (re.compile(r"^(\s*)case ENTRY_UPDATED:\s*$"), r"\1// case ENTRY_UPDATED:"),
        (re.compile(r"^(\s*)case ENTRY_DELETED:\s*$"), r"\1} if (sw_type == ENTRY_ADDED || sw_type == ENTRY_UPDATED || sw_type == ENTRY_DELETED) {  // case ENTRY_DELETED: (also by fall-through)"),
        (re.compile(r"^(\s*)default:\s*$"), r"\1} if (false) {  // default:"),
        (re.compile(r"^(\s*)break;\s*$"), r"\1;  // break;"),
    ],
}

# Java streams and expression lambdas of UpgradeTracker (:141-154, :196-197): lambda SYNTAX only — `(a, b)` / `x ->` become C++
# lambda heads, an expression body gets its `return` and braces (where the expression spans lines, on the line it ends on),
# `Entry::getKey` / `Collectors.toSet()` become methods of the stand-in stream
EXTRA_RULES["STREAMS"] = [
    (re.compile(r"\.max\(\(rs1, rs2\)\s*$"), ".max([=](auto rs1, auto rs2)"),
    (re.compile(r"^(\s*)->\s*(Long\.compare\(rs1\.earliestStartTime, rs2\.earliestStartTime\))\)\.get\(\);"), r"\1{ return \2; }).get();"),
    (re.compile(r"\.filter\(e -> "), ".filter([=](auto e) { return "),
    (re.compile(r"(\|\| e\.getValue\(\)\.lastChangeTime > now - FIFTEEN_MINS\))\)\s*$"), r"\1; })"),
    (re.compile(r"\.map\(Entry::getKey\)\.collect\(Collectors\.toSet\(\)\)"), ".map_getKey().collect_toSet()"),
    (re.compile(r"anySatisfy\(expires -> now >= expires\)"), "anySatisfy([=](auto expires) { return now >= expires; })"),
    (re.compile(r"reject\(\(r, expires\) -> now >= expires\)"), "reject([=](auto r, auto expires) { return now >= expires; })"),
    (re.compile(r"\bnew ObjectLongHashMap<>\("), "ObjectLongHashMap_new("),
    (re.compile(r"\bnew PerTypeLabelStats\(\)"), "PerTypeLabelStats::make()"),
    (re.compile(r"\bnew ReplicaSetStats\(\)"), "ReplicaSetStats::make()"),
    (re.compile(r"\bMap\.Entry\b"), "Entry"),
    (re.compile(r"\bSystem\.currentTimeMillis\(\)"), "currentTimeMillis()"),
]

# TypeConstraintManager: library type names with dots / generics / arrays, its one expression lambda, field reads through a
# tracker reference (the stand-in is a handle: `->`)
EXTRA_RULES["TCM"] = [
    (re.compile(r"\bImmutableSet\.Builder<String>"), "ImmutableSetBuilder"),
    (re.compile(r"\bMap\.Entry\b"), "Entry"),
    (re.compile(r"l -> Arrays\.binarySearch\(instanceLabels, l\) >= 0;"), "[=](const String &l) { return Arrays.binarySearch(instanceLabels, l) >= 0; };"),
    (re.compile(r"\bnew ObjectIntHashMap<String>\("), "ObjectIntHashMap_new("),
    (re.compile(r"\bnew HashSet<>\("), "HashSet_new("),
    (re.compile(r"\.currentStats\b"), "->currentStats"),
    (re.compile(r"\bString\[\]"), "StringArray"),
]

# preShutdown (:7015): the task's lambda returns an entry or null — C++ wants the return type named; Java enum constants
EXTRA_RULES["SHUTDOWN"] = [
    (re.compile(r"taskPool\.submit\(\(\) -> \{"), "taskPool.submit([=]() -> Entry<String, Long> {"),
    (re.compile(r"\bStatus\.(LOADING_FAILED|LOADING)\b"), r"Status::\1"),
    (re.compile(r"\bConcurrentHashMap\.newKeySet\(\)"), "ConcurrentHashMap_newKeySet()"),
]

# clhm / ModelCacheUnloadBufManager: generic object creation (`new WeightedValue<V>(..)`), `try { .. } finally { .. }` without a
# catch clause (every try of these ranges: the finally blocks release the lock / reset the drain status and no `return` inside a
# try skips anything but an unlock, which is a no-op here) becomes two plain blocks, Java's `assert`, member modifiers
EXTRA_RULES["CLHM"] = [
    (re.compile(r"\bnew\s+(\w+)<([\w, ]*)>\("), r"\1<\2>("),
    (re.compile(r"^(\s*)try \{\s*$"), r"\1{  // try {"),
    (re.compile(r"^(\s*)assert ([^;]*);"), r"\1JAVA_ASSERT(\2);"),
    (re.compile(r"^\s*(?:/\*\*.*\*/\s*)?(?:private\s+)?static\s+"), "static "),
    (re.compile(r"\bDrainStatus\.IDLE\b"), "IDLE"),
    (re.compile(r"\bSystem\.currentTimeMillis\(\)"), "currentTimeMillis()"),
    (re.compile(r"\bThread\.currentThread\(\)\.getId\(\)"), "Thread_currentThread_getId()"),
]

# TypeConstraintManager's incremental path: the TCM rules plus method references, the generic-method call syntax of Guava's
# builders, `new X[0]`-style array creation and the array constructor reference
EXTRA_RULES["TCMI"] = EXTRA_RULES["TCM"] + [
    (re.compile(r"\bnewStats::contains\b"), "[=](auto x) { return newStats.contains(x); }"),
    (re.compile(r"\.toArray\(InstanceSetStatsTracker\[\]::new\)"), ".toArray_()"),
    (re.compile(r"ImmutableSet\.<String>builder"), "ImmutableSet.builder"),
    (re.compile(r"e -> !e\.equals\(iid\)"), "[=](auto e) { return !e.equals(iid); }"),
    (re.compile(r"\.forEach\(InstanceSetStatsTracker::update\)"), ".forEach_update()"),
    (re.compile(r"\bnew HashMap<>\("), "HashMap_new("),
    (re.compile(r"\bnew ArrayList<>\("), "ArrayList_new("),
    (re.compile(r"^(\s*)assert ([^;]*);"), r"\1JAVA_ASSERT(\2);"),
    (re.compile(r"^\s*private\s+static\s+"), "static "),
    (re.compile(r'\.map\(e -> e\.getKey\(\) \+ ": " \+ e\.getValue\(\)\.getInstanceCount\(\)\)'), ".map_log()"),
    (re.compile(r'\.collect\(Collectors\.joining\(", ", "\{", "\}"\)\)'), ".collect_joining()"),
    (re.compile(r'\(defaultPreferred != null \? defaultPreferred : "<none>"\)'), "LOGSTR(defaultPreferred)"),
    (re.compile(r"\bInstanceSetStatsTracker\[\]"), "TrackerArray"),
    (re.compile(r"\bModelTypeConstraints\.fromInstanceSet\("), "ModelTypeConstraints::fromInstanceSet("),
    (re.compile(r"\bInstanceSetStatsTracker\.EMPTY_STATS\b"), "EMPTY_STATS"),
]

# The janitor's loops and the prune (registry_harness.cc).  Syntax only:
#  - `registryLoop:` labels the `for` (:6019) and `continue registryLoop;` (:6031) leaves the inner `while (true)` for the next
#    record: C++ has no labelled continue, the statement becomes a `goto` to a label that the harness puts in front of the brace
#    closing that `for` (:6108), and the Java label line becomes a comment
#  - `new Object[] { a, b, c }` (:6098) is an aggregate of the stand-in for Object[]; `new TreeSet<>(VALUE_COMP)` / `new HashSet<>()`
#    become factory calls; `CacheEntry.LOADING` names a constant of a class (`::`); `instanceInfo::contains` (:6549, a method
#    reference in the readOnlyMode branch) names a function object
#  - the `removeIf` lambda (:6604-6605) is an expression lambda that spans two lines: head, `return` and the closing brace
#  - member modifiers of the instance constants (`public final long`)
EXTRA_RULES["REG"] = [
    (re.compile(r"^(\s*)registryLoop:\s*$"), r"\1// registryLoop:"),
    (re.compile(r"\bcontinue registryLoop;"), "goto registryLoop_continue;"),
    (re.compile(r"\bnew Object\[\] \{"), "ObjectArr3{"),
    (re.compile(r"\bnew TreeSet<>\(VALUE_COMP\)"), "SortedSet_new(VALUE_COMP)"),
    (re.compile(r"\bnew HashSet<>\("), "HashSet_new("),
    (re.compile(r"\bCacheEntry\.(LOADING|ACTIVE)\b"), r"CacheEntry::\1"),
    (re.compile(r"\binstanceInfo::contains\b"), "instanceInfo_contains"),
    (re.compile(r"\.removeIf\(ent -> "), ".removeIf([=](auto ent) { return "),
    (re.compile(r"(\|\| instanceInfo\.contains\(ent\.getKey\(\)\))\);"), r"\1; });"),
    (re.compile(r"^\s*public\s+final\s+long\s+"), "static const long "),
    (re.compile(r"\bSystem\.currentTimeMillis\(\)"), "currentTimeMillis()"),
]

# token-level rewrites, applied in order to every extracted line
RULES = [
    # Java numeric literals may carry underscores: 120_000L -> 120000L
    (re.compile(r"\b\d+(?:_\d+)+L?\b"), lambda m: m.group(0).replace("_", "")),
    # `final` on locals has no C++ counterpart that matters here
    (re.compile(r"\bfinal\s+"), ""),
    # object creation: `new ArrayList<>(n)` / `new IntArrayList(n)` -> factory calls of the stand-ins (the diamond's type
    # argument is inferred from the declaration on the left, as in Java); any other `new X(...)` -> a value of the handle class X
    (re.compile(r"\bnew\s+ArrayList<>\("), "ArrayList_new("),
    (re.compile(r"\bnew\s+TreeSet<>\("), "TreeSet_new("),
    (re.compile(r"\bnew\s+IntArrayList\("), "IntArrayList_new("),
    (re.compile(r"\bnew\s+(\w+)\("), r"\1("),
    # string literals are java.lang.String objects (they are concatenated with + into log / exception messages)
    (re.compile(r'"(?:[^"\\]|\\.)*"'), lambda m: "String(" + m.group(0) + ")"),
    # Java keeps methods and variables in separate name spaces (`long oldest = oldest(filteredInstances);`, :3617): the call
    # gets the stand-in's name
    (re.compile(r"\boldest\("), "oldest_of("),
    # lambdas: `ent -> {` (a Java lambda captures effectively-final locals by value; here: copies of handles)
    # `() -> {` (a Runnable): a lambda without parameters
    (re.compile(r"\(\)\s*->\s*\{"), "[=]() {"),
    (re.compile(r"\b(\w+)\s*->\s*\{"), r"[=](auto \1) {"),
    # wildcard generics do not exist in C++: ServiceInstance<?> -> ServiceInstance
    (re.compile(r"<\?>"), ""),
    # the narrowing primitive conversion (int) of a parenthesised double expression saturates in Java (JLS 5.1.3) and is
    # undefined on overflow in C++: route it through a function with the Java semantics
    (re.compile(r"\(int\)\s*\("), "J2I("),
    # a Java array's length is a field, a C++ stand-in needs a call
    (re.compile(r"\.length\b(?!\()"), ".length()"),
    # `explicit` (a field of CacheMissExcludeSet) is a C++ keyword
    (re.compile(r"\bexplicit\b"), "explicit_"),
    # static members of the boxed types: Long.compare / Long.MAX_VALUE / Integer.MAX_VALUE (Long is also a type argument,
    # Map<String, Long>, so it has to be a class on the C++ side)
    (re.compile(r"\b(Long|Integer|Collections)\.(?=[A-Za-z])"), r"\1::"),
    # the Java array type Object[] as a type argument (Entry<Object[], Long>) -> the stand-in's name
    (re.compile(r"\bObject\[\]"), "ObjectArr3"),
    # `x instanceof T` -> a function of the stand-ins (C++ has no runtime type test on these handles)
    (re.compile(r"\b(\w+)\s+instanceof\s+(\w+)"), r"instanceof_\2(\1)"),
    # `union` (Guava's Sets.union) is a C++ keyword
    (re.compile(r"\.union\("), ".union_("),
    # `register` is a C++ keyword (Phaser.register()); try/catch/finally: the finally block becomes a plain block behind the
    # try statement (equivalent whenever no exception leaves the catch clauses, which is the case for the stubs' calls)
    (re.compile(r"\bthis\."), "this->"),
    (re.compile(r"\.register\("), ".register_("),
    (re.compile(r"\}\s*finally\s*\{"), "} {"),
    # member modifiers in front of the constant declarations
    (re.compile(r"^\s*(?:protected|public)\s+static\s+"), ""),
]


def extract():
    out_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "_ref", "gen")
    os.makedirs(out_dir, exist_ok=True)
    manifest = []
    for name, rel, a, b, must_first, must_last, *extra in RANGES + CLHM_RANGES + TCMI_RANGES + REG_RANGES:
        path = os.path.join(REF, rel)
        lines = open(path, encoding="utf-8").read().split("\n")
        body = lines[a - 1:b]
        if must_first not in body[0] or must_last not in body[-1]:
            sys.exit(f"extract.py: {rel}:{a}-{b} is not the text this harness was written against "
                     f"(expected {must_first!r} ... {must_last!r}); the reference moved — fix RANGES")
        out = []
        for ln in body:
            for rx, rep in (EXTRA_RULES[extra[0]] if extra else []) + RULES:
                ln = rx.sub(rep, ln)
            out.append(ln)
        assert len(out) == len(body)
        with open(os.path.join(out_dir, name + ".inc"), "w", encoding="utf-8") as f:
            f.write(f"// GENERATED by oracle/ref_harness/extract.py from {rel}:{a}-{b} — reference text, do not commit\n")
            f.write("\n".join(out) + "\n")
        manifest.append(f"{name}: {rel}:{a}-{b} ({len(body)} lines)")
    with open(os.path.join(out_dir, "MANIFEST.txt"), "w") as f:
        f.write("\n".join(manifest) + "\n")
    return manifest


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit(f"extract.py: no reference tree at {REF}")
    for m in extract():
        print(m)
