// mmplace_jni.cc — thin JNI veneer over include/mmplace.h for the Java mesh.
//
// This repository's image has no JDK / jni.h, so the shipped build does not include it; it is the
// file a ModelMesh maintainer compiles next to libmmplace.so (tests/test_jni_veneer.py compiles and
// links it against a stub jni.h and checks the exported names against the Java `native` declarations):
//   g++ -shared -fPIC -I$JAVA_HOME/include -I$JAVA_HOME/include/linux -I../include mmplace_jni.cc
//       -L../modelmesh_amd/lib -lmmplace -o libmmplace_jni.so
//
// Java side: integration/GpuPlacementLB.java (class com.ibm.watson.modelmesh.MmPlace).
// All buffers are direct ByteBuffers laid out exactly as the C structs (little
// endian), so nothing is copied or translated here.
#include <jni.h>

#include "mmplace.h"

namespace {
inline mmp_ctx *ctx_of(jlong h) { return reinterpret_cast<mmp_ctx *>(static_cast<intptr_t>(h)); }

// Never let a solver error take the JVM down: surface it as IllegalStateException.
jint check(JNIEnv *env, mmp_ctx *c, int rc)
{
    if (rc != MMP_OK) {
        jclass ex = env->FindClass("java/lang/IllegalStateException");
        if (ex) env->ThrowNew(ex, mmp_last_error(c));
    }
    return rc;
}
template <class T>
T *buf(JNIEnv *env, jobject bb) { return bb ? static_cast<T *>(env->GetDirectBufferAddress(bb)) : nullptr; }

// A direct buffer that must hold `count` elements of T: the C ABI trusts its sizes, the JVM must not (a short buffer
// would be read or written past its end by the library).  Throws IllegalArgumentException and returns false.
template <class T>
bool holds(JNIEnv *env, jobject bb, jlong count, const char *what)
{
    if (count <= 0) return true;
    const jlong cap = bb ? env->GetDirectBufferCapacity(bb) : -1;
    if (cap >= 0 && cap >= count * static_cast<jlong>(sizeof(T))) return true;
    jclass ex = env->FindClass("java/lang/IllegalArgumentException");
    if (ex) env->ThrowNew(ex, what);
    return false;
}
}  // namespace

extern "C" {

JNIEXPORT jlong JNICALL Java_com_ibm_watson_modelmesh_MmPlace_create(JNIEnv *env, jclass, jint device,
                                                                     jlong minSpaceUnits, jlong minChurnAgeMs)
{
    mmp_config cfg{};
    cfg.device = device;
    cfg.min_space_units = minSpaceUnits;  // MM.java:765-771
    cfg.min_churn_age_ms = minChurnAgeMs; // MM.java:697
    mmp_ctx *c = nullptr;
    if (check(env, nullptr, mmp_create(&cfg, &c)) != MMP_OK) return 0;
    return static_cast<jlong>(reinterpret_cast<intptr_t>(c));
}

JNIEXPORT void JNICALL Java_com_ibm_watson_modelmesh_MmPlace_destroy(JNIEnv *, jclass, jlong h) { mmp_destroy(ctx_of(h)); }

// handleInstanceTableChange (MM.java:1455): whole-table load or single-row upserts, then commit.
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_podsLoad(JNIEnv *env, jclass, jlong h, jobject rows, jint n)
{
    return check(env, ctx_of(h), mmp_pods_load(ctx_of(h), buf<mmp_pod_row>(env, rows), n));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_podsUpsert(JNIEnv *env, jclass, jlong h, jobject idx,
                                                                        jobject rows, jint n)
{
    return check(env, ctx_of(h), mmp_pods_upsert(ctx_of(h), buf<int32_t>(env, idx), buf<mmp_pod_row>(env, rows), n));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_podsRemove(JNIEnv *env, jclass, jlong h, jobject idx, jint n)
{
    return check(env, ctx_of(h), mmp_pods_remove(ctx_of(h), buf<int32_t>(env, idx), n));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_typesLoad(JNIEnv *env, jclass, jlong h, jint nTypes,
                                                                       jobject allowed, jobject prefer,
                                                                       jobject hasAllowed, jobject hasPrefer)
{
    return check(env, ctx_of(h),
                 mmp_types_load(ctx_of(h), nTypes, buf<uint64_t>(env, allowed), buf<uint64_t>(env, prefer),
                                buf<uint8_t>(env, hasAllowed), buf<uint8_t>(env, hasPrefer)));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_replacedReplicaSetsLoad(JNIEnv *env, jclass, jlong h,
                                                                                     jobject rs, jint n)
{
    return check(env, ctx_of(h), mmp_replaced_rs_load(ctx_of(h), buf<int32_t>(env, rs), n));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_modelsLoad(JNIEnv *env, jclass, jlong h, jobject rows,
                                                                        jint nModels, jobject entPod, jobject entTime,
                                                                        jint nEntries)
{
    return check(env, ctx_of(h),
                 mmp_models_load(ctx_of(h), buf<mmp_model_row>(env, rows), nModels, buf<int32_t>(env, entPod),
                                 buf<int64_t>(env, entTime), nEntries));
}
// registry listener events: whole ModelRecords replaced by index (see mmp_models_upsert)
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_modelsUpsert(JNIEnv *env, jclass, jlong h, jobject idx,
                                                                          jobject rows, jint n, jobject entPod,
                                                                          jobject entTime, jint nEntries)
{
    return check(env, ctx_of(h),
                 mmp_models_upsert(ctx_of(h), buf<int32_t>(env, idx), buf<mmp_model_row>(env, rows), n,
                                   buf<int32_t>(env, entPod), buf<int64_t>(env, entTime), nEntries));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_commit(JNIEnv *env, jclass, jlong h)
{
    return check(env, ctx_of(h), mmp_snapshot_commit(ctx_of(h)));
}

// CacheMissForwardingLB.getNext (MM.java:4776): n requests in, n 16-byte results out.
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_placeBatch(JNIEnv *env, jclass, jlong h, jobject reqs,
                                                                        jint n, jobject extraPool, jint nExtra,
                                                                        jlong nowMs, jobject outs)
{
    if (!holds<mmp_place_req>(env, reqs, n, "placeBatch: reqs shorter than n requests") ||
        !holds<int32_t>(env, extraPool, nExtra, "placeBatch: extraPool shorter than nExtra entries") ||
        !holds<mmp_place_out>(env, outs, n, "placeBatch: outs shorter than n results"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_place_batch(ctx_of(h), buf<mmp_place_req>(env, reqs), n, buf<int32_t>(env, extraPool), nExtra,
                                 nowMs, buf<mmp_place_out>(env, outs)));
}
// the single-caller form: the caller's side (mmp_place_caller, 40 bytes) once per call, 24-byte requests — the batches of the rate
// task, the janitor, the reaper and preShutdown, which all run on ONE instance
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_placeBatchCaller(JNIEnv *env, jclass, jlong h, jobject caller,
                                                                              jobject reqs, jint n, jobject extraPool,
                                                                              jint nExtra, jlong nowMs, jobject outs)
{
    if (!holds<mmp_place_caller>(env, caller, 1, "placeBatchCaller: caller shorter than one mmp_place_caller") ||
        !holds<mmp_place_req_c>(env, reqs, n, "placeBatchCaller: reqs shorter than n requests") ||
        !holds<int32_t>(env, extraPool, nExtra, "placeBatchCaller: extraPool shorter than nExtra entries") ||
        !holds<mmp_place_out>(env, outs, n, "placeBatchCaller: outs shorter than n results"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_place_batch_c(ctx_of(h), buf<mmp_place_caller>(env, caller), buf<mmp_place_req_c>(env, reqs), n,
                                   buf<int32_t>(env, extraPool), nExtra, nowMs, buf<mmp_place_out>(env, outs)));
}

// The resident decision kernel: placeBatch(n = 1) without a kernel launch (include/mmplace.h: mmp_resident).
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_resident(JNIEnv *env, jclass, jlong h, jboolean enable)
{
    return check(env, ctx_of(h), mmp_resident(ctx_of(h), enable ? 1 : 0));
}

// ---- the pod-axis group (several GPUs of one node; RCCL runs inside libmmplace) ----
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_shardUniqueId(JNIEnv *env, jclass, jobject idOut)
{
    if (!holds<char>(env, idOut, MMP_SHARD_UNIQUE_ID_BYTES, "shardUniqueId: idOut shorter than 128 bytes")) return MMP_EINVAL;
    return check(env, nullptr, mmp_shard_unique_id(buf<char>(env, idOut)));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_shardGroupInit(JNIEnv *env, jclass, jlong h, jobject id,
                                                                            jint rank, jint world)
{
    if (id && !holds<char>(env, id, MMP_SHARD_UNIQUE_ID_BYTES, "shardGroupInit: id shorter than 128 bytes")) return MMP_EINVAL;
    return check(env, ctx_of(h), mmp_shard_group_init(ctx_of(h), buf<char>(env, id), rank, world));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_shardGroupDestroy(JNIEnv *env, jclass, jlong h)
{
    return check(env, ctx_of(h), mmp_shard_group_destroy(ctx_of(h)));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_shardCommit(JNIEnv *env, jclass, jlong h)
{
    return check(env, ctx_of(h), mmp_shard_commit(ctx_of(h)));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_shardPlaceBatch(JNIEnv *env, jclass, jlong h, jobject reqs,
                                                                             jint n, jobject extraPool, jint nExtra,
                                                                             jlong nowMs, jobject outs, jobject nRestOut)
{
    if (!holds<mmp_place_req>(env, reqs, n, "shardPlaceBatch: reqs shorter than n requests") ||
        !holds<int32_t>(env, extraPool, nExtra, "shardPlaceBatch: extraPool shorter than nExtra entries") ||
        !holds<mmp_place_out>(env, outs, n, "shardPlaceBatch: outs shorter than n results") ||
        (nRestOut && !holds<int32_t>(env, nRestOut, 1, "shardPlaceBatch: nRestOut shorter than one int")))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_shard_place_batch(ctx_of(h), buf<mmp_place_req>(env, reqs), n, buf<int32_t>(env, extraPool), nExtra,
                                       nowMs, buf<mmp_place_out>(env, outs), buf<int32_t>(env, nRestOut)));
}

// ForwardingLB.getNext (MM.java:4315): the request brings the counters of its own copies (O(copies), no table-sized buffer)
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_serveBatch(JNIEnv *env, jclass, jlong h, jobject reqs,
                                                                        jint n, jobject counters, jint nCounters,
                                                                        jobject exclPod, jobject exclTime, jint nExcl,
                                                                        jlong nowMs, jobject outs)
{
    if (!holds<mmp_serve_req>(env, reqs, n, "serveBatch: reqs shorter than n requests") ||
        !holds<mmp_serve_counter>(env, counters, nCounters, "serveBatch: counters shorter than nCounters entries") ||
        !holds<int32_t>(env, exclPod, nExcl, "serveBatch: exclPod shorter than nExcl entries") ||
        !holds<int64_t>(env, exclTime, nExcl, "serveBatch: exclTime shorter than nExcl entries") ||
        !holds<mmp_serve_out>(env, outs, n, "serveBatch: outs shorter than n results"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_serve_batch(ctx_of(h), buf<mmp_serve_req>(env, reqs), n, buf<mmp_serve_counter>(env, counters), nCounters,
                                 buf<int32_t>(env, exclPod), buf<int64_t>(env, exclTime), nExcl, nowMs, buf<mmp_serve_out>(env, outs)));
}

JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_clusterStats(JNIEnv *env, jclass, jlong h, jobject out)
{
    return check(env, ctx_of(h), mmp_cluster_stats(ctx_of(h), buf<mmp_stats>(env, out)));
}

// typeSetStats / instanceSetStats and the ProhibitedTypeSet partitions (MM.java:1432-1448, TypeConstraintManager)
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_typeStats(JNIEnv *env, jclass, jlong h, jint type, jobject out)
{
    return check(env, ctx_of(h), mmp_type_stats(ctx_of(h), type, buf<mmp_stats>(env, out)));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_partitionCount(JNIEnv *env, jclass, jlong h, jobject nOut)
{
    return check(env, ctx_of(h), mmp_partition_count(ctx_of(h), buf<int32_t>(env, nOut)));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_partitionStats(JNIEnv *env, jclass, jlong h, jint partition,
                                                                            jobject out, jobject prohibitedOut, jint maxWords)
{
    return check(env, ctx_of(h),
                 mmp_partition_stats(ctx_of(h), partition, buf<mmp_stats>(env, out), buf<uint64_t>(env, prohibitedOut), maxWords));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_podPartitions(JNIEnv *env, jclass, jlong h, jobject partitionOut,
                                                                           jint maxPods, jobject nOut)
{
    return check(env, ctx_of(h), mmp_pod_partitions(ctx_of(h), buf<int32_t>(env, partitionOut), maxPods, buf<int32_t>(env, nOut)));
}

// ---- eviction: clhm put/evict (ConcurrentLinkedHashMap.java:590-611,329-352) -----------------------
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_cachesLoad(JNIEnv *env, jclass, jlong h, jint nCaches,
                                                                        jobject segOff, jobject lastUsed,
                                                                        jobject weight, jobject capacity)
{
    return check(env, ctx_of(h),
                 mmp_caches_load(ctx_of(h), nCaches, buf<int32_t>(env, segOff), buf<int64_t>(env, lastUsed),
                                 buf<int32_t>(env, weight), buf<int64_t>(env, capacity)));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_evictBatch(JNIEnv *env, jclass, jlong h, jobject reqs,
                                                                        jint n, jlong nowMs, jobject outs)
{
    return check(env, ctx_of(h),
                 mmp_evict_batch(ctx_of(h), buf<mmp_evict_req>(env, reqs), n, nowMs, buf<mmp_evict_out>(env, outs)));
}

// ---- stateful caches + ModelCacheUnloadBufManager (ModelCacheUnloadBufManager.java:130-402) --------
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_cachesLoadKeyed(JNIEnv *env, jclass, jlong h,
                                                                             jint nCaches, jobject segOff,
                                                                             jobject lastUsed, jobject weight,
                                                                             jobject key, jobject capacity,
                                                                             jobject ubm)
{
    return check(env, ctx_of(h),
                 mmp_caches_load_keyed(ctx_of(h), nCaches, buf<int32_t>(env, segOff), buf<int64_t>(env, lastUsed),
                                       buf<int32_t>(env, weight), buf<int32_t>(env, key),
                                       buf<int64_t>(env, capacity), buf<mmp_ubm_state>(env, ubm)));
}
// nEvictedSlots: direct IntBuffer of one element
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_cacheReplay(JNIEnv *env, jclass, jlong h, jobject ops,
                                                                         jint nOps, jlong nowMs, jobject outs,
                                                                         jobject evictedKeys, jint maxEvicted,
                                                                         jobject nEvictedSlots)
{
    return check(env, ctx_of(h),
                 mmp_cache_replay(ctx_of(h), buf<mmp_cache_op>(env, ops), nOps, nowMs,
                                  buf<mmp_cache_op_out>(env, outs), buf<int32_t>(env, evictedKeys), maxEvicted,
                                  buf<int32_t>(env, nEvictedSlots)));
}
// scalars: direct buffer {int32 n; int32 pad; int64 capacity; int64 weightedSize}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_cacheRead(JNIEnv *env, jclass, jlong h, jint cache,
                                                                       jint maxEntries, jobject lastUsed,
                                                                       jobject weight, jobject key, jobject scalars,
                                                                       jobject ubm)
{
    struct Scalars {
        int32_t n, pad;
        int64_t capacity, weighted_size;
    } *sc = buf<Scalars>(env, scalars);
    if (!sc) return check(env, ctx_of(h), MMP_EINVAL);
    return check(env, ctx_of(h),
                 mmp_cache_read(ctx_of(h), cache, maxEntries, buf<int64_t>(env, lastUsed), buf<int32_t>(env, weight),
                                buf<int32_t>(env, key), &sc->n, &sc->capacity, &sc->weighted_size,
                                buf<mmp_ubm_state>(env, ubm)));
}
// the caches by model id (see mmp_caches_load_keyed_k): a thin pass-through, the buffers are the caller's to size as the header says
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_cachesLoadKeyedK(JNIEnv *env, jclass, jlong h, jint nCaches, jobject segOff,
                                                                              jobject lastUsed, jobject weight, jobject keys,
                                                                              jobject keyOff, jobject isUnloadbuf, jobject capacity,
                                                                              jobject ubm, jobject keyRowOut)
{
    return check(env, ctx_of(h),
                 mmp_caches_load_keyed_k(ctx_of(h), nCaches, buf<int32_t>(env, segOff), buf<int64_t>(env, lastUsed), buf<int32_t>(env, weight),
                                         buf<char>(env, keys), buf<int32_t>(env, keyOff), buf<uint8_t>(env, isUnloadbuf),
                                         buf<int64_t>(env, capacity), buf<mmp_ubm_state>(env, ubm), buf<int32_t>(env, keyRowOut)));
}
// sizes: direct IntBuffer of two elements {nEvictedSlots, nIdBytes}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_cacheReplayK(JNIEnv *env, jclass, jlong h, jobject ops, jint nOps, jobject keys,
                                                                          jobject keyOff, jlong nowMs, jobject keyStatusOut,
                                                                          jobject keyRowOut, jobject outs, jobject evictedRows,
                                                                          jint maxEvicted, jobject evIdBytesOut, jint maxIdBytes,
                                                                          jobject evIdOffOut, jobject sizes)
{
    int32_t *sz = buf<int32_t>(env, sizes);
    if (!sz || !holds<int32_t>(env, sizes, 2, "cacheReplayK: sizes shorter than two ints")) return check(env, ctx_of(h), MMP_EINVAL);
    return check(env, ctx_of(h),
                 mmp_cache_replay_k(ctx_of(h), buf<mmp_cache_op>(env, ops), nOps, buf<char>(env, keys), buf<int32_t>(env, keyOff), nowMs,
                                    buf<int32_t>(env, keyStatusOut), buf<int32_t>(env, keyRowOut), buf<mmp_cache_op_out>(env, outs),
                                    buf<int32_t>(env, evictedRows), maxEvicted, sz, buf<char>(env, evIdBytesOut), maxIdBytes,
                                    buf<int32_t>(env, evIdOffOut), sz + 1));
}
// sizes: direct IntBuffer of two elements {nSlots, nBytes}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_cacheEvictedIds(JNIEnv *env, jclass, jlong h, jobject bytesOut, jint maxBytes,
                                                                             jobject offOut, jobject sizes)
{
    int32_t *sz = buf<int32_t>(env, sizes);
    if (!sz || !holds<int32_t>(env, sizes, 2, "cacheEvictedIds: sizes shorter than two ints")) return check(env, ctx_of(h), MMP_EINVAL);
    return check(env, ctx_of(h), mmp_cache_evicted_ids(ctx_of(h), buf<char>(env, bytesOut), maxBytes, buf<int32_t>(env, offOut), sz, sz + 1));
}
// cacheReplayK with the victims' lastUsed beside their ids (mmp_cache_replay_kt): evLastUsedOut holds maxEvicted longs, or is null
// (the context keeps the times: cacheEvictedTimes)
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_cacheReplayKT(JNIEnv *env, jclass, jlong h, jobject ops, jint nOps, jobject keys,
                                                                           jobject keyOff, jlong nowMs, jobject keyStatusOut,
                                                                           jobject keyRowOut, jobject outs, jobject evictedRows,
                                                                           jint maxEvicted, jobject evIdBytesOut, jint maxIdBytes,
                                                                           jobject evIdOffOut, jobject sizes, jobject evLastUsedOut)
{
    int32_t *sz = buf<int32_t>(env, sizes);
    if (!sz || !holds<int32_t>(env, sizes, 2, "cacheReplayKT: sizes shorter than two ints") ||
        (evLastUsedOut && !holds<int64_t>(env, evLastUsedOut, maxEvicted, "cacheReplayKT: evLastUsedOut shorter than maxEvicted")))
        return check(env, ctx_of(h), MMP_EINVAL);
    return check(env, ctx_of(h),
                 mmp_cache_replay_kt(ctx_of(h), buf<mmp_cache_op>(env, ops), nOps, buf<char>(env, keys), buf<int32_t>(env, keyOff), nowMs,
                                     buf<int32_t>(env, keyStatusOut), buf<int32_t>(env, keyRowOut), buf<mmp_cache_op_out>(env, outs),
                                     buf<int32_t>(env, evictedRows), maxEvicted, sz, buf<char>(env, evIdBytesOut), maxIdBytes,
                                     buf<int32_t>(env, evIdOffOut), sz + 1, buf<int64_t>(env, evLastUsedOut)));
}
// nSlotsOut: direct IntBuffer of one element; out holds maxSlots longs (null with maxSlots 0: the size only)
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_cacheEvictedTimes(JNIEnv *env, jclass, jlong h, jobject out, jint maxSlots,
                                                                               jobject nSlotsOut)
{
    if (maxSlots < 0 || !holds<int32_t>(env, nSlotsOut, 1, "cacheEvictedTimes: nSlotsOut shorter than one int") ||
        !holds<int64_t>(env, out, maxSlots, "cacheEvictedTimes: out shorter than maxSlots"))
        return check(env, ctx_of(h), MMP_EINVAL);
    return check(env, ctx_of(h), mmp_cache_evicted_times(ctx_of(h), buf<int64_t>(env, out), maxSlots, buf<int32_t>(env, nSlotsOut)));
}
// scalars: direct buffer {int32 n; int32 nIdBytes; int64 capacity; int64 weightedSize}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_cacheReadK(JNIEnv *env, jclass, jlong h, jint cache, jint maxEntries,
                                                                        jobject lastUsed, jobject weight, jobject rowOut, jobject idBytesOut,
                                                                        jint maxIdBytes, jobject idOffOut, jobject scalars, jobject ubm)
{
    struct Scalars {
        int32_t n, n_id_bytes;
        int64_t capacity, weighted_size;
    } *sc = buf<Scalars>(env, scalars);
    if (!sc) return check(env, ctx_of(h), MMP_EINVAL);
    return check(env, ctx_of(h),
                 mmp_cache_read_k(ctx_of(h), cache, maxEntries, buf<int64_t>(env, lastUsed), buf<int32_t>(env, weight),
                                  buf<int32_t>(env, rowOut), buf<char>(env, idBytesOut), maxIdBytes, buf<int32_t>(env, idOffOut), &sc->n,
                                  &sc->n_id_bytes, &sc->capacity, &sc->weighted_size, buf<mmp_ubm_state>(env, ubm)));
}

// ---- request guards (MM.java:3603-3626, 3870-3884, 4003-4042, 4590-4627, 5158-5197, 2867-2933, 5440-5468)
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_gateBatch(JNIEnv *env, jclass, jlong h, jobject reqs,
                                                                       jint n, jobject exclPod, jobject exclTime,
                                                                       jint nExcl, jobject explicitPool,
                                                                       jint nExplicit, jlong nowMs,
                                                                       jlong inUseFailureExpiryMs, jobject outs)
{
    return check(env, ctx_of(h),
                 mmp_gate_batch(ctx_of(h), buf<mmp_gate_req>(env, reqs), n, buf<int32_t>(env, exclPod),
                                buf<int64_t>(env, exclTime), nExcl, buf<int32_t>(env, explicitPool), nExplicit, nowMs,
                                inUseFailureExpiryMs, buf<mmp_gate_out>(env, outs)));
}

// ---- the cache-MISS route in one launch: the guards + the load target of every request (include/mmplace.h: mmp_miss_batch)
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_missBatch(JNIEnv *env, jclass, jlong h, jobject gateReqs,
                                                                       jobject placeReqs, jint n, jobject exclPod, jobject exclTime,
                                                                       jint nExcl, jobject explicitPool, jint nExplicit,
                                                                       jobject extraPool, jint nExtra, jlong nowMs,
                                                                       jlong inUseFailureExpiryMs, jobject gateOuts, jobject placeOuts)
{
    return check(env, ctx_of(h),
                 mmp_miss_batch(ctx_of(h), buf<mmp_gate_req>(env, gateReqs), buf<mmp_place_req>(env, placeReqs), n,
                                buf<int32_t>(env, exclPod), buf<int64_t>(env, exclTime), nExcl, buf<int32_t>(env, explicitPool), nExplicit,
                                buf<int32_t>(env, extraPool), nExtra, nowMs, inUseFailureExpiryMs, buf<mmp_gate_out>(env, gateOuts),
                                buf<mmp_place_out>(env, placeOuts)));
}
// ---- the cache-HIT route in one launch: the guards + the serve target of every request (include/mmplace.h: mmp_route_batch)
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_routeBatch(JNIEnv *env, jclass, jlong h, jobject gateReqs,
                                                                        jobject serveReqs, jint n, jobject counters,
                                                                        jint nCounters, jobject exclPod, jobject exclTime,
                                                                        jint nExcl, jobject explicitPool, jint nExplicit,
                                                                        jlong nowMs, jlong inUseFailureExpiryMs,
                                                                        jobject gateOuts, jobject serveOuts)
{
    return check(env, ctx_of(h),
                 mmp_route_batch(ctx_of(h), buf<mmp_gate_req>(env, gateReqs), buf<mmp_serve_req>(env, serveReqs), n,
                                 buf<mmp_serve_counter>(env, counters), nCounters, buf<int32_t>(env, exclPod),
                                 buf<int64_t>(env, exclTime), nExcl, buf<int32_t>(env, explicitPool), nExplicit, nowMs,
                                 inUseFailureExpiryMs, buf<mmp_gate_out>(env, gateOuts), buf<mmp_serve_out>(env, serveOuts)));
}
// ---- the single-caller forms of the two routes: the calling instance's side (mmp_seam_caller, 112 bytes) once per batch, 48-byte
// gate rows and 24-byte serve / load-target rows (include/mmplace.h: mmp_route_batch_c, mmp_miss_batch_c)
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_routeBatchCaller(JNIEnv *env, jclass, jlong h, jobject caller,
                                                                              jobject gateReqs, jobject serveReqs, jint n,
                                                                              jobject counters, jint nCounters, jobject exclPod,
                                                                              jobject exclTime, jint nExcl, jobject explicitPool,
                                                                              jint nExplicit, jlong nowMs, jlong inUseFailureExpiryMs,
                                                                              jobject gateOuts, jobject serveOuts)
{
    if (!holds<mmp_seam_caller>(env, caller, 1, "routeBatchCaller: caller shorter than one mmp_seam_caller") ||
        !holds<mmp_gate_req_c>(env, gateReqs, n, "routeBatchCaller: gateReqs shorter than n requests") ||
        !holds<mmp_serve_req_c>(env, serveReqs, n, "routeBatchCaller: serveReqs shorter than n requests") ||
        !holds<mmp_gate_out>(env, gateOuts, n, "routeBatchCaller: gateOuts shorter than n results") ||
        !holds<mmp_serve_out>(env, serveOuts, n, "routeBatchCaller: serveOuts shorter than n results"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_route_batch_c(ctx_of(h), buf<mmp_seam_caller>(env, caller), buf<mmp_gate_req_c>(env, gateReqs),
                                   buf<mmp_serve_req_c>(env, serveReqs), n, buf<mmp_serve_counter>(env, counters), nCounters,
                                   buf<int32_t>(env, exclPod), buf<int64_t>(env, exclTime), nExcl, buf<int32_t>(env, explicitPool),
                                   nExplicit, nowMs, inUseFailureExpiryMs, buf<mmp_gate_out>(env, gateOuts),
                                   buf<mmp_serve_out>(env, serveOuts)));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_missBatchCaller(JNIEnv *env, jclass, jlong h, jobject caller,
                                                                             jobject placeCaller, jobject gateReqs, jobject placeReqs,
                                                                             jint n, jobject exclPod, jobject exclTime, jint nExcl,
                                                                             jobject explicitPool, jint nExplicit, jobject extraPool,
                                                                             jint nExtra, jlong nowMs, jlong inUseFailureExpiryMs,
                                                                             jobject gateOuts, jobject placeOuts)
{
    if (!holds<mmp_seam_caller>(env, caller, 1, "missBatchCaller: caller shorter than one mmp_seam_caller") ||
        !holds<mmp_place_caller>(env, placeCaller, 1, "missBatchCaller: placeCaller shorter than one mmp_place_caller") ||
        !holds<mmp_gate_req_c>(env, gateReqs, n, "missBatchCaller: gateReqs shorter than n requests") ||
        !holds<mmp_place_req_c>(env, placeReqs, n, "missBatchCaller: placeReqs shorter than n requests") ||
        !holds<mmp_gate_out>(env, gateOuts, n, "missBatchCaller: gateOuts shorter than n results") ||
        !holds<mmp_place_out>(env, placeOuts, n, "missBatchCaller: placeOuts shorter than n results"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_miss_batch_c(ctx_of(h), buf<mmp_seam_caller>(env, caller), buf<mmp_place_caller>(env, placeCaller),
                                  buf<mmp_gate_req_c>(env, gateReqs), buf<mmp_place_req_c>(env, placeReqs), n,
                                  buf<int32_t>(env, exclPod), buf<int64_t>(env, exclTime), nExcl, buf<int32_t>(env, explicitPool),
                                  nExplicit, buf<int32_t>(env, extraPool), nExtra, nowMs, inUseFailureExpiryMs,
                                  buf<mmp_gate_out>(env, gateOuts), buf<mmp_place_out>(env, placeOuts)));
}
// ---- the single-caller forms BY MODEL ID: request i names its model by keys[keyOff[i], keyOff[i + 1]) (the model id's UTF-8 bytes),
// resolved on the device inside the call; modelIdxOut (n ints, may be null) receives the rows (include/mmplace.h: THE RULE BY KEY)
static bool holds_keys(JNIEnv *env, const char *who, jobject keys, jobject keyOff, jint n, jobject modelIdxOut)
{
    if (n < 0) return false;
    if (n == 0) return true;  // (a valid call without keys)
    if (!holds<int32_t>(env, keyOff, (jlong)n + 1, who)) return false;
    if (!holds<char>(env, keys, (jlong)buf<int32_t>(env, keyOff)[n], who)) return false;
    return !modelIdxOut || holds<int32_t>(env, modelIdxOut, n, who);
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_placeBatchKeyed(JNIEnv *env, jclass, jlong h, jobject caller, jobject reqs,
                                                                             jint n, jobject keys, jobject keyOff, jobject extraPool,
                                                                             jint nExtra, jlong nowMs, jobject outs, jobject modelIdxOut)
{
    if (!holds_keys(env, "placeBatchKeyed: keyOff / keys / modelIdxOut shorter than the call's n", keys, keyOff, n, modelIdxOut) ||
        !holds<mmp_place_caller>(env, caller, 1, "placeBatchKeyed: caller shorter than one mmp_place_caller") ||
        !holds<mmp_place_req_c>(env, reqs, n, "placeBatchKeyed: reqs shorter than n requests") ||
        !holds<int32_t>(env, extraPool, nExtra, "placeBatchKeyed: extraPool shorter than nExtra entries") ||
        !holds<mmp_place_out>(env, outs, n, "placeBatchKeyed: outs shorter than n results"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_place_batch_ck(ctx_of(h), buf<mmp_place_caller>(env, caller), buf<mmp_place_req_c>(env, reqs), n, buf<char>(env, keys),
                                    buf<int32_t>(env, keyOff), buf<int32_t>(env, extraPool), nExtra, nowMs, buf<mmp_place_out>(env, outs),
                                    buf<int32_t>(env, modelIdxOut)));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_routeBatchKeyed(JNIEnv *env, jclass, jlong h, jobject caller,
                                                                             jobject gateReqs, jobject serveReqs, jint n, jobject keys,
                                                                             jobject keyOff, jobject counters, jint nCounters,
                                                                             jobject exclPod, jobject exclTime, jint nExcl,
                                                                             jobject explicitPool, jint nExplicit, jlong nowMs,
                                                                             jlong inUseFailureExpiryMs, jobject gateOuts, jobject serveOuts,
                                                                             jobject modelIdxOut)
{
    if (!holds_keys(env, "routeBatchKeyed: keyOff / keys / modelIdxOut shorter than the call's n", keys, keyOff, n, modelIdxOut) ||
        !holds<mmp_seam_caller>(env, caller, 1, "routeBatchKeyed: caller shorter than one mmp_seam_caller") ||
        !holds<mmp_gate_req_c>(env, gateReqs, n, "routeBatchKeyed: gateReqs shorter than n requests") ||
        !holds<mmp_serve_req_c>(env, serveReqs, n, "routeBatchKeyed: serveReqs shorter than n requests") ||
        !holds<mmp_gate_out>(env, gateOuts, n, "routeBatchKeyed: gateOuts shorter than n results") ||
        !holds<mmp_serve_out>(env, serveOuts, n, "routeBatchKeyed: serveOuts shorter than n results"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_route_batch_ck(ctx_of(h), buf<mmp_seam_caller>(env, caller), buf<mmp_gate_req_c>(env, gateReqs),
                                    buf<mmp_serve_req_c>(env, serveReqs), n, buf<char>(env, keys), buf<int32_t>(env, keyOff),
                                    buf<mmp_serve_counter>(env, counters), nCounters, buf<int32_t>(env, exclPod),
                                    buf<int64_t>(env, exclTime), nExcl, buf<int32_t>(env, explicitPool), nExplicit, nowMs,
                                    inUseFailureExpiryMs, buf<mmp_gate_out>(env, gateOuts), buf<mmp_serve_out>(env, serveOuts),
                                    buf<int32_t>(env, modelIdxOut)));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_missBatchKeyed(JNIEnv *env, jclass, jlong h, jobject caller,
                                                                            jobject placeCaller, jobject gateReqs, jobject placeReqs,
                                                                            jint n, jobject keys, jobject keyOff, jobject exclPod,
                                                                            jobject exclTime, jint nExcl, jobject explicitPool,
                                                                            jint nExplicit, jobject extraPool, jint nExtra, jlong nowMs,
                                                                            jlong inUseFailureExpiryMs, jobject gateOuts, jobject placeOuts,
                                                                            jobject modelIdxOut)
{
    if (!holds_keys(env, "missBatchKeyed: keyOff / keys / modelIdxOut shorter than the call's n", keys, keyOff, n, modelIdxOut) ||
        !holds<mmp_seam_caller>(env, caller, 1, "missBatchKeyed: caller shorter than one mmp_seam_caller") ||
        !holds<mmp_place_caller>(env, placeCaller, 1, "missBatchKeyed: placeCaller shorter than one mmp_place_caller") ||
        !holds<mmp_gate_req_c>(env, gateReqs, n, "missBatchKeyed: gateReqs shorter than n requests") ||
        !holds<mmp_place_req_c>(env, placeReqs, n, "missBatchKeyed: placeReqs shorter than n requests") ||
        !holds<mmp_gate_out>(env, gateOuts, n, "missBatchKeyed: gateOuts shorter than n results") ||
        !holds<mmp_place_out>(env, placeOuts, n, "missBatchKeyed: placeOuts shorter than n results"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_miss_batch_ck(ctx_of(h), buf<mmp_seam_caller>(env, caller), buf<mmp_place_caller>(env, placeCaller),
                                   buf<mmp_gate_req_c>(env, gateReqs), buf<mmp_place_req_c>(env, placeReqs), n, buf<char>(env, keys),
                                   buf<int32_t>(env, keyOff), buf<int32_t>(env, exclPod), buf<int64_t>(env, exclTime), nExcl,
                                   buf<int32_t>(env, explicitPool), nExplicit, buf<int32_t>(env, extraPool), nExtra, nowMs,
                                   inUseFailureExpiryMs, buf<mmp_gate_out>(env, gateOuts), buf<mmp_place_out>(env, placeOuts),
                                   buf<int32_t>(env, modelIdxOut)));
}
// ---- the single-caller forms BY VMODEL ID: keys name VMODELS, nfKeys / nfOff (both may be null) the notFoundModelId spans, reqFlags
// (n ints, may be null) MMP_VMRQ_AFTER_STRONG; resolveVModelId runs on the device inside the call and vmOut (n mmp_vseam_row, may be
// null) says what it answered (include/mmplace.h: THE RULE BY VMODEL KEY)
static bool holds_vkeys(JNIEnv *env, const char *who, jobject keys, jobject keyOff, jobject nfKeys, jobject nfOff, jobject reqFlags, jint n,
                        jobject vmOut)
{
    if (!holds_keys(env, who, keys, keyOff, n, nullptr)) return false;
    if (n == 0) return true;
    if (nfOff && (!holds<int32_t>(env, nfOff, (jlong)n + 1, who) || !holds<char>(env, nfKeys, (jlong)buf<int32_t>(env, nfOff)[n], who)))
        return false;
    if (reqFlags && !holds<uint32_t>(env, reqFlags, n, who)) return false;
    return !vmOut || holds<mmp_vseam_row>(env, vmOut, n, who);
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_placeBatchVKeyed(JNIEnv *env, jclass, jlong h, jobject caller, jobject reqs,
                                                                              jint n, jobject keys, jobject keyOff, jobject nfKeys,
                                                                              jobject nfOff, jobject reqFlags, jobject extraPool,
                                                                              jint nExtra, jlong nowMs, jobject outs, jobject vmOut)
{
    if (!holds_vkeys(env, "placeBatchVKeyed: keyOff / keys / nfOff / nfKeys / reqFlags / vmOut shorter than the call's n", keys, keyOff, nfKeys,
                     nfOff, reqFlags, n, vmOut) ||
        !holds<mmp_place_caller>(env, caller, 1, "placeBatchVKeyed: caller shorter than one mmp_place_caller") ||
        !holds<mmp_place_req_c>(env, reqs, n, "placeBatchVKeyed: reqs shorter than n requests") ||
        !holds<int32_t>(env, extraPool, nExtra, "placeBatchVKeyed: extraPool shorter than nExtra entries") ||
        !holds<mmp_place_out>(env, outs, n, "placeBatchVKeyed: outs shorter than n results"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_place_batch_cv(ctx_of(h), buf<mmp_place_caller>(env, caller), buf<mmp_place_req_c>(env, reqs), n, buf<char>(env, keys),
                                    buf<int32_t>(env, keyOff), buf<char>(env, nfKeys), buf<int32_t>(env, nfOff), buf<uint32_t>(env, reqFlags),
                                    buf<int32_t>(env, extraPool), nExtra, nowMs, buf<mmp_place_out>(env, outs),
                                    buf<mmp_vseam_row>(env, vmOut)));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_routeBatchVKeyed(JNIEnv *env, jclass, jlong h, jobject caller,
                                                                              jobject gateReqs, jobject serveReqs, jint n, jobject keys,
                                                                              jobject keyOff, jobject nfKeys, jobject nfOff,
                                                                              jobject reqFlags, jobject counters, jint nCounters,
                                                                              jobject exclPod, jobject exclTime, jint nExcl,
                                                                              jobject explicitPool, jint nExplicit, jlong nowMs,
                                                                              jlong inUseFailureExpiryMs, jobject gateOuts,
                                                                              jobject serveOuts, jobject vmOut)
{
    if (!holds_vkeys(env, "routeBatchVKeyed: keyOff / keys / nfOff / nfKeys / reqFlags / vmOut shorter than the call's n", keys, keyOff, nfKeys,
                     nfOff, reqFlags, n, vmOut) ||
        !holds<mmp_seam_caller>(env, caller, 1, "routeBatchVKeyed: caller shorter than one mmp_seam_caller") ||
        !holds<mmp_gate_req_c>(env, gateReqs, n, "routeBatchVKeyed: gateReqs shorter than n requests") ||
        !holds<mmp_serve_req_c>(env, serveReqs, n, "routeBatchVKeyed: serveReqs shorter than n requests") ||
        !holds<mmp_gate_out>(env, gateOuts, n, "routeBatchVKeyed: gateOuts shorter than n results") ||
        !holds<mmp_serve_out>(env, serveOuts, n, "routeBatchVKeyed: serveOuts shorter than n results"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_route_batch_cv(ctx_of(h), buf<mmp_seam_caller>(env, caller), buf<mmp_gate_req_c>(env, gateReqs),
                                    buf<mmp_serve_req_c>(env, serveReqs), n, buf<char>(env, keys), buf<int32_t>(env, keyOff),
                                    buf<char>(env, nfKeys), buf<int32_t>(env, nfOff), buf<uint32_t>(env, reqFlags),
                                    buf<mmp_serve_counter>(env, counters), nCounters, buf<int32_t>(env, exclPod),
                                    buf<int64_t>(env, exclTime), nExcl, buf<int32_t>(env, explicitPool), nExplicit, nowMs,
                                    inUseFailureExpiryMs, buf<mmp_gate_out>(env, gateOuts), buf<mmp_serve_out>(env, serveOuts),
                                    buf<mmp_vseam_row>(env, vmOut)));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_missBatchVKeyed(JNIEnv *env, jclass, jlong h, jobject caller,
                                                                             jobject placeCaller, jobject gateReqs, jobject placeReqs,
                                                                             jint n, jobject keys, jobject keyOff, jobject nfKeys,
                                                                             jobject nfOff, jobject reqFlags, jobject exclPod,
                                                                             jobject exclTime, jint nExcl, jobject explicitPool,
                                                                             jint nExplicit, jobject extraPool, jint nExtra, jlong nowMs,
                                                                             jlong inUseFailureExpiryMs, jobject gateOuts, jobject placeOuts,
                                                                             jobject vmOut)
{
    if (!holds_vkeys(env, "missBatchVKeyed: keyOff / keys / nfOff / nfKeys / reqFlags / vmOut shorter than the call's n", keys, keyOff, nfKeys,
                     nfOff, reqFlags, n, vmOut) ||
        !holds<mmp_seam_caller>(env, caller, 1, "missBatchVKeyed: caller shorter than one mmp_seam_caller") ||
        !holds<mmp_place_caller>(env, placeCaller, 1, "missBatchVKeyed: placeCaller shorter than one mmp_place_caller") ||
        !holds<mmp_gate_req_c>(env, gateReqs, n, "missBatchVKeyed: gateReqs shorter than n requests") ||
        !holds<mmp_place_req_c>(env, placeReqs, n, "missBatchVKeyed: placeReqs shorter than n requests") ||
        !holds<mmp_gate_out>(env, gateOuts, n, "missBatchVKeyed: gateOuts shorter than n results") ||
        !holds<mmp_place_out>(env, placeOuts, n, "missBatchVKeyed: placeOuts shorter than n results"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_miss_batch_cv(ctx_of(h), buf<mmp_seam_caller>(env, caller), buf<mmp_place_caller>(env, placeCaller),
                                   buf<mmp_gate_req_c>(env, gateReqs), buf<mmp_place_req_c>(env, placeReqs), n, buf<char>(env, keys),
                                   buf<int32_t>(env, keyOff), buf<char>(env, nfKeys), buf<int32_t>(env, nfOff),
                                   buf<uint32_t>(env, reqFlags), buf<int32_t>(env, exclPod), buf<int64_t>(env, exclTime), nExcl,
                                   buf<int32_t>(env, explicitPool), nExplicit, buf<int32_t>(env, extraPool), nExtra, nowMs,
                                   inUseFailureExpiryMs, buf<mmp_gate_out>(env, gateOuts), buf<mmp_place_out>(env, placeOuts),
                                   buf<mmp_vseam_row>(env, vmOut)));
}

// ---- rebalancers (MM.java:5636-5871, 6110-6335, 6616-6747, 6959-7147) ---------------------------------
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_proactivePlan(JNIEnv *env, jclass, jlong h,
                                                                           jint defaultModelSizeUnits, jlong nowMs,
                                                                           jint maxOut, jobject outModel,
                                                                           jobject outLastUsed, jobject info)
{
    return check(env, ctx_of(h),
                 mmp_proactive_plan(ctx_of(h), defaultModelSizeUnits, nowMs, maxOut, buf<int32_t>(env, outModel),
                                    buf<int64_t>(env, outLastUsed), buf<mmp_proactive_info>(env, info)));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_proactivePlanSubset(JNIEnv *env, jclass, jlong h, jint partition,
                                                                                 jobject skipModels, jint nSkip,
                                                                                 jint defaultModelSizeUnits, jlong nowMs,
                                                                                 jint maxOut, jobject outModel,
                                                                                 jobject outLastUsed, jobject info)
{
    return check(env, ctx_of(h),
                 mmp_proactive_plan_subset(ctx_of(h), partition, buf<int32_t>(env, skipModels), nSkip, defaultModelSizeUnits,
                                           nowMs, maxOut, buf<int32_t>(env, outModel), buf<int64_t>(env, outLastUsed),
                                           buf<mmp_proactive_info>(env, info)));
}
// The reaper's first half (pruneModelRegistry, MM.java:6524-6609): the output buffers' capacities are checked here, the
// library only knows maxEdits / maxRemoved.
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_registryPrune(JNIEnv *env, jclass, jlong h, jint selfPod, jlong nowMs,
                                                                           jlong goneAfterMs, jlong lastUsedAgeOnAddMs, jint flags,
                                                                           jobject editsOut, jint maxEdits, jobject removedOut,
                                                                           jint maxRemoved, jobject info)
{
    if (!holds<mmp_prune_edit>(env, editsOut, maxEdits, "registryPrune: editsOut shorter than maxEdits") ||
        !holds<mmp_prune_removed>(env, removedOut, maxRemoved, "registryPrune: removedOut shorter than maxRemoved") ||
        !holds<mmp_prune_info>(env, info, 1, "registryPrune: info shorter than one mmp_prune_info"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_registry_prune(ctx_of(h), selfPod, nowMs, goneAfterMs, lastUsedAgeOnAddMs, static_cast<uint32_t>(flags),
                                    buf<mmp_prune_edit>(env, editsOut), maxEdits, buf<mmp_prune_removed>(env, removedOut), maxRemoved,
                                    buf<mmp_prune_info>(env, info)));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_registryMissingGet(JNIEnv *env, jclass, jlong h, jobject sinceOut,
                                                                                jint maxPods, jobject nOut)
{
    if (!holds<int64_t>(env, sinceOut, maxPods, "registryMissingGet: sinceOut shorter than maxPods") ||
        !holds<int32_t>(env, nOut, 1, "registryMissingGet: nOut shorter than one int"))
        return MMP_EINVAL;
    return check(env, ctx_of(h), mmp_registry_missing_get(ctx_of(h), buf<int64_t>(env, sinceOut), maxPods, buf<int32_t>(env, nOut)));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_registryMissingReset(JNIEnv *env, jclass, jlong h)
{
    return check(env, ctx_of(h), mmp_registry_missing_reset(ctx_of(h)));
}
// The registry listener's model counts (MM.java:2807-2854, :6852-6863): the buffers' capacities are checked here, the library only
// knows maxPods / maxTypes.  A null buffer with a capacity of 0: that part is not returned.
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_registryCensus(JNIEnv *env, jclass, jlong h, jobject statsOut,
                                                                            jobject podLoadedOut, jobject podFailedOut, jint maxPods,
                                                                            jobject nPodsOut, jobject typesOut, jint maxTypes,
                                                                            jobject nTypesOut)
{
    if (!holds<mmp_registry_stats>(env, statsOut, 1, "registryCensus: statsOut shorter than one mmp_registry_stats") ||
        !holds<int32_t>(env, podLoadedOut, maxPods, "registryCensus: podLoadedOut shorter than maxPods") ||
        !holds<int32_t>(env, podFailedOut, maxPods, "registryCensus: podFailedOut shorter than maxPods") ||
        !holds<int32_t>(env, nPodsOut, 1, "registryCensus: nPodsOut shorter than one int") ||
        !holds<mmp_registry_type_stats>(env, typesOut, maxTypes, "registryCensus: typesOut shorter than maxTypes") ||
        !holds<int32_t>(env, nTypesOut, 1, "registryCensus: nTypesOut shorter than one int"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_registry_census(ctx_of(h), buf<mmp_registry_stats>(env, statsOut), buf<int32_t>(env, podLoadedOut),
                                     buf<int32_t>(env, podFailedOut), maxPods, buf<int32_t>(env, nPodsOut),
                                     buf<mmp_registry_type_stats>(env, typesOut), maxTypes, buf<int32_t>(env, nTypesOut)));
}
// The janitor's cache and registry loops (MM.java:5892-6008, :6014-6108): every buffer's capacity is checked here, the library
// only knows n / maxEdits / maxCandidates.
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_janitorPlan(JNIEnv *env, jclass, jlong h, jobject entries, jint n,
                                                                         jobject params, jint flags, jobject actionsOut,
                                                                         jobject editsOut, jint maxEdits, jobject candidatesOut,
                                                                         jobject candidateRowsOut, jint maxCandidates, jobject info)
{
    if (!holds<mmp_janitor_entry>(env, entries, n, "janitorPlan: entries shorter than n") ||
        !holds<mmp_janitor_params>(env, params, 1, "janitorPlan: params shorter than one mmp_janitor_params") ||
        !holds<uint8_t>(env, actionsOut, n, "janitorPlan: actionsOut shorter than n") ||
        !holds<mmp_janitor_edit>(env, editsOut, maxEdits, "janitorPlan: editsOut shorter than maxEdits") ||
        !holds<mmp_cache_entry>(env, candidatesOut, maxCandidates, "janitorPlan: candidatesOut shorter than maxCandidates") ||
        !holds<int32_t>(env, candidateRowsOut, maxCandidates, "janitorPlan: candidateRowsOut shorter than maxCandidates") ||
        !holds<mmp_janitor_info>(env, info, 1, "janitorPlan: info shorter than one mmp_janitor_info"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_janitor_plan(ctx_of(h), buf<mmp_janitor_entry>(env, entries), n, buf<mmp_janitor_params>(env, params),
                                  static_cast<uint32_t>(flags), buf<uint8_t>(env, actionsOut), buf<mmp_janitor_edit>(env, editsOut), maxEdits,
                                  buf<mmp_cache_entry>(env, candidatesOut), buf<int32_t>(env, candidateRowsOut), maxCandidates,
                                  buf<mmp_janitor_info>(env, info)));
}
// loadLocal / the load-failure path / deregisterModel / removeLocalModelCopyAsync (MM.java:5204-5207, :2484-2495, :2948-2958,
// :6347-6365) as a batch of ops: every buffer's capacity is checked here, the library only knows n / maxEdits
// (a null statusOut is not returned).
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_registryOps(JNIEnv *env, jclass, jlong h, jobject ops, jint n, jlong nowMs,
                                                                         jint flags, jobject statusOut, jobject editsOut, jint maxEdits,
                                                                         jobject info)
{
    if (!holds<mmp_registry_op>(env, ops, n, "registryOps: ops shorter than n") ||
        (statusOut && !holds<uint8_t>(env, statusOut, n, "registryOps: statusOut shorter than n")) ||
        !holds<mmp_registry_op_edit>(env, editsOut, maxEdits, "registryOps: editsOut shorter than maxEdits") ||
        !holds<mmp_registry_ops_info>(env, info, 1, "registryOps: info shorter than one mmp_registry_ops_info"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_registry_ops(ctx_of(h), buf<mmp_registry_op>(env, ops), n, nowMs, static_cast<uint32_t>(flags), buf<uint8_t>(env, statusOut),
                                  buf<mmp_registry_op_edit>(env, editsOut), maxEdits, buf<mmp_registry_ops_info>(env, info)));
}
// the same BY MODEL ID, with the fifth kind (the cache-hit loop's drop of its own copy, MM.java:3682-3687): the keys resolved, the
// ops evaluated and the edits applied under one hold of the batch lock (mmp_registry_ops_k).  keys and keyOff both null: by row.
// modelIdxOut and statusOut may be null; info holds one mmp_registry_ops_info_k (88 bytes).
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_registryOpsKeyed(JNIEnv *env, jclass, jlong h, jobject ops, jint n, jobject keys,
                                                                              jobject keyOff, jlong nowMs, jint flags, jobject modelIdxOut,
                                                                              jobject statusOut, jobject editsOut, jint maxEdits, jobject info)
{
    if (n < 0 || maxEdits < 0 || !holds<mmp_registry_op>(env, ops, n, "registryOpsKeyed: ops shorter than n") ||
        (keyOff && !holds<int32_t>(env, keyOff, (jlong)n + 1, "registryOpsKeyed: keyOff shorter than n + 1")) ||
        (keyOff && keys && n > 0 && !holds<char>(env, keys, buf<int32_t>(env, keyOff)[n], "registryOpsKeyed: keys shorter than keyOff[n]")) ||
        (modelIdxOut && !holds<int32_t>(env, modelIdxOut, n, "registryOpsKeyed: modelIdxOut shorter than n")) ||
        (statusOut && !holds<uint8_t>(env, statusOut, n, "registryOpsKeyed: statusOut shorter than n")) ||
        !holds<mmp_registry_op_edit>(env, editsOut, maxEdits, "registryOpsKeyed: editsOut shorter than maxEdits") ||
        !holds<mmp_registry_ops_info_k>(env, info, 1, "registryOpsKeyed: info shorter than one mmp_registry_ops_info_k"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_registry_ops_k(ctx_of(h), buf<mmp_registry_op>(env, ops), n, buf<char>(env, keys), buf<int32_t>(env, keyOff), nowMs,
                                    static_cast<uint32_t>(flags), buf<int32_t>(env, modelIdxOut), buf<uint8_t>(env, statusOut),
                                    buf<mmp_registry_op_edit>(env, editsOut), maxEdits, buf<mmp_registry_ops_info_k>(env, info)));
}
// onEviction's task body by model id (mmp_evictions_k, MM.java:2886-2920): entries n x 32 bytes, params 24 bytes, outs n x 24 bytes,
// info one mmp_evictions_info (112 bytes); modelIdxOut and statusOut may be null
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_evictionsKeyed(JNIEnv *env, jclass, jlong h, jobject entries, jint n, jobject keys,
                                                                            jobject keyOff, jobject params, jint flags, jobject modelIdxOut,
                                                                            jobject outs, jobject statusOut, jobject editsOut, jint maxEdits,
                                                                            jobject info)
{
    if (n < 0 || maxEdits < 0 || !holds<mmp_evicted_entry>(env, entries, n, "evictionsKeyed: entries shorter than n") ||
        (keyOff && !holds<int32_t>(env, keyOff, (jlong)n + 1, "evictionsKeyed: keyOff shorter than n + 1")) ||
        (keyOff && keys && n > 0 && !holds<char>(env, keys, buf<int32_t>(env, keyOff)[n], "evictionsKeyed: keys shorter than keyOff[n]")) ||
        !holds<mmp_evict_params>(env, params, 1, "evictionsKeyed: params shorter than one mmp_evict_params") ||
        (modelIdxOut && !holds<int32_t>(env, modelIdxOut, n, "evictionsKeyed: modelIdxOut shorter than n")) ||
        !holds<mmp_evicted_out>(env, outs, n, "evictionsKeyed: outs shorter than n") ||
        (statusOut && !holds<uint8_t>(env, statusOut, n, "evictionsKeyed: statusOut shorter than n")) ||
        !holds<mmp_registry_op_edit>(env, editsOut, maxEdits, "evictionsKeyed: editsOut shorter than maxEdits") ||
        !holds<mmp_evictions_info>(env, info, 1, "evictionsKeyed: info shorter than one mmp_evictions_info"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_evictions_k(ctx_of(h), buf<mmp_evicted_entry>(env, entries), n, buf<char>(env, keys), buf<int32_t>(env, keyOff),
                                 buf<mmp_evict_params>(env, params), static_cast<uint32_t>(flags), buf<int32_t>(env, modelIdxOut),
                                 buf<mmp_evicted_out>(env, outs), buf<uint8_t>(env, statusOut), buf<mmp_registry_op_edit>(env, editsOut), maxEdits,
                                 buf<mmp_evictions_info>(env, info)));
}
// getStatus answers from the resident registry (MM.java:3247; class :3760-3768, copy list makeStatusInfo :3013-3058): every
// buffer's capacity is checked here, the library only knows n / maxCopies.  A null copiesOut with maxCopies = 0: the sizes only.
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_modelsStatus(JNIEnv *env, jclass, jlong h, jobject reqs, jint n, jlong nowMs,
                                                                          jobject rowsOut, jobject copiesOut, jint maxCopies,
                                                                          jobject nCopiesOut)
{
    if (!holds<mmp_status_req>(env, reqs, n, "modelsStatus: reqs shorter than n") ||
        !holds<mmp_status_row>(env, rowsOut, n, "modelsStatus: rowsOut shorter than n") ||
        !holds<mmp_status_copy>(env, copiesOut, maxCopies, "modelsStatus: copiesOut shorter than maxCopies") ||
        !holds<int32_t>(env, nCopiesOut, 1, "modelsStatus: nCopiesOut shorter than one int"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_models_status(ctx_of(h), buf<mmp_status_req>(env, reqs), n, nowMs, buf<mmp_status_row>(env, rowsOut),
                                   buf<mmp_status_copy>(env, copiesOut), maxCopies, buf<int32_t>(env, nCopiesOut)));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_scaleupPlan(JNIEnv *env, jclass, jlong h, jobject entries,
                                                                         jint n, jobject params, jobject outs,
                                                                         jobject overloadedOut, jobject skipped)
{
    return check(env, ctx_of(h),
                 mmp_scaleup_plan(ctx_of(h), buf<mmp_cache_entry>(env, entries), n,
                                  buf<mmp_scaleup_params>(env, params), buf<mmp_scaleup_out>(env, outs),
                                  buf<uint8_t>(env, overloadedOut), buf<int32_t>(env, skipped)));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_scaledownPlan(JNIEnv *env, jclass, jlong h,
                                                                           jobject entries, jint n, jobject params,
                                                                           jobject removedOut)
{
    return check(env, ctx_of(h),
                 mmp_scaledown_plan(ctx_of(h), buf<mmp_cache_entry>(env, entries), n,
                                    buf<mmp_scaledown_params>(env, params), buf<uint8_t>(env, removedOut)));
}
// the rate task / the janitor of a mesh that runs with limitModelConcurrency == true (MaxConcCacheEntry rows beside the entries)
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_scaleupPlanConc(JNIEnv *env, jclass, jlong h, jobject entries,
                                                                             jobject conc, jint n, jobject params,
                                                                             jobject concParams, jobject outs, jobject concOuts,
                                                                             jobject overloadedOut, jobject skipped, jobject result)
{
    if (!holds<mmp_cache_entry>(env, entries, n, "scaleupPlanConc: entries shorter than n rows") ||
        !holds<mmp_conc_entry>(env, conc, n, "scaleupPlanConc: conc shorter than n rows") ||
        !holds<mmp_scaleup_params>(env, params, 1, "scaleupPlanConc: params shorter than one mmp_scaleup_params") ||
        !holds<mmp_conc_params>(env, concParams, 1, "scaleupPlanConc: concParams shorter than one mmp_conc_params") ||
        !holds<mmp_scaleup_out>(env, outs, n, "scaleupPlanConc: outs shorter than n rows") ||
        !holds<mmp_conc_out>(env, concOuts, n, "scaleupPlanConc: concOuts shorter than n rows") ||
        !holds<uint8_t>(env, overloadedOut, 1, "scaleupPlanConc: overloadedOut shorter than one byte") ||
        !holds<int32_t>(env, skipped, 1, "scaleupPlanConc: skipped shorter than one int") ||
        !holds<mmp_conc_result>(env, result, 1, "scaleupPlanConc: result shorter than one mmp_conc_result"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_scaleup_plan_conc(ctx_of(h), buf<mmp_cache_entry>(env, entries), buf<mmp_conc_entry>(env, conc), n,
                                       buf<mmp_scaleup_params>(env, params), buf<mmp_conc_params>(env, concParams),
                                       buf<mmp_scaleup_out>(env, outs), buf<mmp_conc_out>(env, concOuts),
                                       buf<uint8_t>(env, overloadedOut), buf<int32_t>(env, skipped),
                                       buf<mmp_conc_result>(env, result)));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_scaledownPlanConc(JNIEnv *env, jclass, jlong h, jobject entries,
                                                                               jobject conc, jint n, jobject params,
                                                                               jlong dynamicRpmScaleConstant, jobject removedOut)
{
    if (!holds<mmp_cache_entry>(env, entries, n, "scaledownPlanConc: entries shorter than n rows") ||
        !holds<mmp_conc_entry>(env, conc, n, "scaledownPlanConc: conc shorter than n rows") ||
        !holds<mmp_scaledown_params>(env, params, 1, "scaledownPlanConc: params shorter than one mmp_scaledown_params") ||
        !holds<uint8_t>(env, removedOut, n, "scaledownPlanConc: removedOut shorter than n bytes"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_scaledown_plan_conc(ctx_of(h), buf<mmp_cache_entry>(env, entries), buf<mmp_conc_entry>(env, conc), n,
                                         buf<mmp_scaledown_params>(env, params), dynamicRpmScaleConstant,
                                         buf<uint8_t>(env, removedOut)));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_migrationPlan(JNIEnv *env, jclass, jlong h,
                                                                           jobject entries, jint n, jint selfPod,
                                                                           jlong nowMs, jlong cutoffAgeMs,
                                                                           jobject actionOut, jobject waitOut)
{
    return check(env, ctx_of(h),
                 mmp_migration_plan(ctx_of(h), buf<mmp_cache_entry>(env, entries), n, selfPod, nowMs, cutoffAgeMs,
                                    buf<uint8_t>(env, actionOut), buf<uint8_t>(env, waitOut)));
}
// THE PERIODIC TASKS BY MODEL ID (MM.java:5672-5690, :5896-5903, :6998-7010: the loops iterate runtimeCache's ids): the keys
// resolved and the entries evaluated under one hold of the batch lock.  keys and keyOff both null: by row.  Every buffer's
// capacity is checked here; the optional ones (conc, concParams, concOuts, result, modelIdxOut, scaledown, removedOut) may be null.
static bool task_keys_held(JNIEnv *env, jobject keys, jobject keyOff, jint n, const char *what_off, const char *what_keys)
{
    return (!keyOff || holds<int32_t>(env, keyOff, (jlong)n + 1, what_off)) &&
           (!keyOff || !keys || n <= 0 || holds<char>(env, keys, buf<int32_t>(env, keyOff)[n], what_keys));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_scaleupPlanKeyed(JNIEnv *env, jclass, jlong h, jobject entries, jobject conc,
                                                                              jint n, jobject keys, jobject keyOff, jobject params,
                                                                              jobject concParams, jobject outs, jobject concOuts,
                                                                              jobject overloadedOut, jobject skipped, jobject result,
                                                                              jobject modelIdxOut)
{
    if (n < 0 || !holds<mmp_cache_entry>(env, entries, n, "scaleupPlanKeyed: entries shorter than n rows") ||
        (conc && !holds<mmp_conc_entry>(env, conc, n, "scaleupPlanKeyed: conc shorter than n rows")) ||
        !task_keys_held(env, keys, keyOff, n, "scaleupPlanKeyed: keyOff shorter than n + 1", "scaleupPlanKeyed: keys shorter than keyOff[n]") ||
        !holds<mmp_scaleup_params>(env, params, 1, "scaleupPlanKeyed: params shorter than one mmp_scaleup_params") ||
        (concParams && !holds<mmp_conc_params>(env, concParams, 1, "scaleupPlanKeyed: concParams shorter than one mmp_conc_params")) ||
        !holds<mmp_scaleup_out>(env, outs, n, "scaleupPlanKeyed: outs shorter than n rows") ||
        (concOuts && !holds<mmp_conc_out>(env, concOuts, n, "scaleupPlanKeyed: concOuts shorter than n rows")) ||
        !holds<uint8_t>(env, overloadedOut, 1, "scaleupPlanKeyed: overloadedOut shorter than one byte") ||
        !holds<int32_t>(env, skipped, 1, "scaleupPlanKeyed: skipped shorter than one int") ||
        (result && !holds<mmp_conc_result>(env, result, 1, "scaleupPlanKeyed: result shorter than one mmp_conc_result")) ||
        (modelIdxOut && !holds<int32_t>(env, modelIdxOut, n, "scaleupPlanKeyed: modelIdxOut shorter than n")))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_scaleup_plan_k(ctx_of(h), buf<mmp_cache_entry>(env, entries), buf<mmp_conc_entry>(env, conc), n, buf<char>(env, keys),
                                    buf<int32_t>(env, keyOff), buf<mmp_scaleup_params>(env, params), buf<mmp_conc_params>(env, concParams),
                                    buf<mmp_scaleup_out>(env, outs), buf<mmp_conc_out>(env, concOuts), buf<uint8_t>(env, overloadedOut),
                                    buf<int32_t>(env, skipped), buf<mmp_conc_result>(env, result), buf<int32_t>(env, modelIdxOut)));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_scaledownPlanKeyed(JNIEnv *env, jclass, jlong h, jobject entries, jobject conc,
                                                                                jint n, jobject keys, jobject keyOff, jobject params,
                                                                                jlong dynamicRpmScaleConstant, jobject removedOut,
                                                                                jobject modelIdxOut)
{
    if (n < 0 || !holds<mmp_cache_entry>(env, entries, n, "scaledownPlanKeyed: entries shorter than n rows") ||
        (conc && !holds<mmp_conc_entry>(env, conc, n, "scaledownPlanKeyed: conc shorter than n rows")) ||
        !task_keys_held(env, keys, keyOff, n, "scaledownPlanKeyed: keyOff shorter than n + 1", "scaledownPlanKeyed: keys shorter than keyOff[n]") ||
        !holds<mmp_scaledown_params>(env, params, 1, "scaledownPlanKeyed: params shorter than one mmp_scaledown_params") ||
        !holds<uint8_t>(env, removedOut, n, "scaledownPlanKeyed: removedOut shorter than n bytes") ||
        (modelIdxOut && !holds<int32_t>(env, modelIdxOut, n, "scaledownPlanKeyed: modelIdxOut shorter than n")))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_scaledown_plan_k(ctx_of(h), buf<mmp_cache_entry>(env, entries), buf<mmp_conc_entry>(env, conc), n, buf<char>(env, keys),
                                      buf<int32_t>(env, keyOff), buf<mmp_scaledown_params>(env, params), dynamicRpmScaleConstant,
                                      buf<uint8_t>(env, removedOut), buf<int32_t>(env, modelIdxOut)));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_migrationPlanKeyed(JNIEnv *env, jclass, jlong h, jobject entries, jint n,
                                                                                jobject keys, jobject keyOff, jint selfPod, jlong nowMs,
                                                                                jlong cutoffAgeMs, jobject actionOut, jobject waitOut,
                                                                                jobject modelIdxOut)
{
    if (n < 0 || !holds<mmp_cache_entry>(env, entries, n, "migrationPlanKeyed: entries shorter than n rows") ||
        !task_keys_held(env, keys, keyOff, n, "migrationPlanKeyed: keyOff shorter than n + 1", "migrationPlanKeyed: keys shorter than keyOff[n]") ||
        !holds<uint8_t>(env, actionOut, n, "migrationPlanKeyed: actionOut shorter than n bytes") ||
        !holds<uint8_t>(env, waitOut, n, "migrationPlanKeyed: waitOut shorter than n bytes") ||
        (modelIdxOut && !holds<int32_t>(env, modelIdxOut, n, "migrationPlanKeyed: modelIdxOut shorter than n")))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_migration_plan_k(ctx_of(h), buf<mmp_cache_entry>(env, entries), n, buf<char>(env, keys), buf<int32_t>(env, keyOff), selfPod,
                                      nowMs, cutoffAgeMs, buf<uint8_t>(env, actionOut), buf<uint8_t>(env, waitOut),
                                      buf<int32_t>(env, modelIdxOut)));
}
// janitorTask as one call (MM.java:5876-6145): by model id, with the scale-down of its candidates in the same hold when
// `scaledown` is not null (removedOut: maxCandidates bytes, aligned with candidatesOut).
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_janitorPlanKeyed(JNIEnv *env, jclass, jlong h, jobject entries, jint n, jobject keys,
                                                                              jobject keyOff, jobject params, jint flags, jobject scaledown,
                                                                              jobject conc, jlong dynamicRpmScaleConstant, jobject modelIdxOut,
                                                                              jobject actionsOut, jobject editsOut, jint maxEdits,
                                                                              jobject candidatesOut, jobject candidateRowsOut, jint maxCandidates,
                                                                              jobject removedOut, jobject info)
{
    if (n < 0 || maxEdits < 0 || maxCandidates < 0 || !holds<mmp_janitor_entry>(env, entries, n, "janitorPlanKeyed: entries shorter than n") ||
        !task_keys_held(env, keys, keyOff, n, "janitorPlanKeyed: keyOff shorter than n + 1", "janitorPlanKeyed: keys shorter than keyOff[n]") ||
        !holds<mmp_janitor_params>(env, params, 1, "janitorPlanKeyed: params shorter than one mmp_janitor_params") ||
        (scaledown && !holds<mmp_scaledown_params>(env, scaledown, 1, "janitorPlanKeyed: scaledown shorter than one mmp_scaledown_params")) ||
        (conc && !holds<mmp_conc_entry>(env, conc, n, "janitorPlanKeyed: conc shorter than n rows")) ||
        (modelIdxOut && !holds<int32_t>(env, modelIdxOut, n, "janitorPlanKeyed: modelIdxOut shorter than n")) ||
        !holds<uint8_t>(env, actionsOut, n, "janitorPlanKeyed: actionsOut shorter than n") ||
        !holds<mmp_janitor_edit>(env, editsOut, maxEdits, "janitorPlanKeyed: editsOut shorter than maxEdits") ||
        !holds<mmp_cache_entry>(env, candidatesOut, maxCandidates, "janitorPlanKeyed: candidatesOut shorter than maxCandidates") ||
        !holds<int32_t>(env, candidateRowsOut, maxCandidates, "janitorPlanKeyed: candidateRowsOut shorter than maxCandidates") ||
        (removedOut && !holds<uint8_t>(env, removedOut, maxCandidates, "janitorPlanKeyed: removedOut shorter than maxCandidates")) ||
        !holds<mmp_janitor_info>(env, info, 1, "janitorPlanKeyed: info shorter than one mmp_janitor_info"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_janitor_plan_k(ctx_of(h), buf<mmp_janitor_entry>(env, entries), n, buf<char>(env, keys), buf<int32_t>(env, keyOff),
                                    buf<mmp_janitor_params>(env, params), static_cast<uint32_t>(flags), buf<mmp_scaledown_params>(env, scaledown),
                                    buf<mmp_conc_entry>(env, conc), dynamicRpmScaleConstant, buf<int32_t>(env, modelIdxOut),
                                    buf<uint8_t>(env, actionsOut), buf<mmp_janitor_edit>(env, editsOut), maxEdits,
                                    buf<mmp_cache_entry>(env, candidatesOut), buf<int32_t>(env, candidateRowsOut), maxCandidates,
                                    buf<uint8_t>(env, removedOut), buf<mmp_janitor_info>(env, info)));
}

// ---- type constraints from labels (TypeConstraintManager.java:337-506, 680-747) ----------------------
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_typesFromLabels(JNIEnv *env, jclass, jlong h,
                                                                             jint nTypes, jobject required,
                                                                             jobject preferred, jobject podLabels,
                                                                             jobject allowedOut, jobject preferOut,
                                                                             jobject hasAllowedOut,
                                                                             jobject hasPreferOut)
{
    return check(env, ctx_of(h),
                 mmp_types_from_labels(ctx_of(h), nTypes, buf<uint64_t>(env, required), buf<uint64_t>(env, preferred),
                                       buf<uint64_t>(env, podLabels), buf<uint64_t>(env, allowedOut),
                                       buf<uint64_t>(env, preferOut), buf<uint8_t>(env, hasAllowedOut),
                                       buf<uint8_t>(env, hasPreferOut)));
}

// ---- UpgradeTracker (UpgradeTracker.java:85-200; called at MM.java:1532,1553,1563) -------------------
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_upgradeInstanceAdded(JNIEnv *env, jclass, jlong h,
                                                                                  jlong labelsKey, jint replicaSet,
                                                                                  jlong startTime, jlong nowMs)
{
    return check(env, ctx_of(h), mmp_upgrade_instance_added(ctx_of(h), labelsKey, replicaSet, startTime, nowMs));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_upgradeInstanceRemoved(JNIEnv *env, jclass, jlong h,
                                                                                    jlong labelsKey, jint replicaSet,
                                                                                    jlong nowMs)
{
    return check(env, ctx_of(h), mmp_upgrade_instance_removed(ctx_of(h), labelsKey, replicaSet, nowMs));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_upgradeHousekeeping(JNIEnv *env, jclass, jlong h,
                                                                                 jlong nowMs)
{
    return check(env, ctx_of(h), mmp_upgrade_housekeeping(ctx_of(h), nowMs));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_upgradeReplaced(JNIEnv *env, jclass, jlong h,
                                                                             jobject rsOut, jobject expiryOut,
                                                                             jint max, jobject nOut)
{
    return check(env, ctx_of(h),
                 mmp_upgrade_replaced(ctx_of(h), buf<int32_t>(env, rsOut), buf<int64_t>(env, expiryOut), max,
                                      buf<int32_t>(env, nOut)));
}

// ---- KV wire format: the raw byte[] of the KV events, packed back to back in a direct buffer ----------
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_podIdsLoad(JNIEnv *env, jclass, jlong h, jobject ids,
                                                                        jobject idOff, jint nPods,
                                                                        jobject idOrderOut, jobject replicaSetOut)
{
    return check(env, ctx_of(h),
                 mmp_pod_ids_load(ctx_of(h), buf<char>(env, ids), buf<int32_t>(env, idOff), nPods,
                                  buf<uint32_t>(env, idOrderOut), buf<int32_t>(env, replicaSetOut)));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_podsIngestJson(JNIEnv *env, jclass, jlong h, jobject json,
                                                                            jobject off, jint n, jobject podIdx,
                                                                            jobject live, jobject startTimeOut,
                                                                            jobject statusOut)
{
    return check(env, ctx_of(h),
                 mmp_pods_ingest_json(ctx_of(h), buf<char>(env, json), buf<int64_t>(env, off), n,
                                      buf<int32_t>(env, podIdx), buf<uint8_t>(env, live),
                                      buf<int64_t>(env, startTimeOut), buf<int32_t>(env, statusOut)));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_typeNamesLoad(JNIEnv *env, jclass, jlong h, jobject names,
                                                                           jobject nameOff, jint nTypes,
                                                                           jint unknownType)
{
    return check(env, ctx_of(h),
                 mmp_type_names_load(ctx_of(h), buf<char>(env, names), buf<int32_t>(env, nameOff), nTypes, unknownType));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_modelsIngestJson(JNIEnv *env, jclass, jlong h,
                                                                              jobject json, jobject off,
                                                                              jint nModels, jobject lastUnloadOut,
                                                                              jobject statusOut)
{
    return check(env, ctx_of(h),
                 mmp_models_ingest_json(ctx_of(h), buf<char>(env, json), buf<int64_t>(env, off), nModels,
                                        buf<int64_t>(env, lastUnloadOut), buf<int32_t>(env, statusOut)));
}
// registry listener events as stored: the raw byte[] of each event, parsed on the device (see mmp_models_upsert_json)
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_modelsUpsertJson(JNIEnv *env, jclass, jlong h,
                                                                              jobject json, jobject off, jint n,
                                                                              jobject modelIdx, jobject deleted,
                                                                              jobject lastUnloadOut, jobject statusOut)
{
    return check(env, ctx_of(h),
                 mmp_models_upsert_json(ctx_of(h), buf<char>(env, json), buf<int64_t>(env, off), n,
                                        buf<int32_t>(env, modelIdx), buf<uint8_t>(env, deleted),
                                        buf<int64_t>(env, lastUnloadOut), buf<int32_t>(env, statusOut)));
}

// Instances join after podIdsLoad (see mmp_pod_ids_append).  The capacities are checked here — the offsets, the id bytes up to the
// last offset, the outputs — the library only knows nNew / maxPods.
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_podIdsAppend(JNIEnv *env, jclass, jlong h, jobject ids,
                                                                          jobject idOff, jint nNew, jobject idOrderOut,
                                                                          jobject replicaSetOut, jint maxPods)
{
    if (!holds<int32_t>(env, idOff, (jlong)nNew + 1, "podIdsAppend: idOff shorter than nNew + 1") ||
        (nNew > 0 && !holds<char>(env, ids, buf<int32_t>(env, idOff)[nNew], "podIdsAppend: ids shorter than idOff[nNew]")) ||
        (idOrderOut && !holds<uint32_t>(env, idOrderOut, maxPods, "podIdsAppend: idOrderOut shorter than maxPods")) ||
        (replicaSetOut && !holds<int32_t>(env, replicaSetOut, maxPods, "podIdsAppend: replicaSetOut shorter than maxPods")))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_pod_ids_append(ctx_of(h), buf<char>(env, ids), buf<int32_t>(env, idOff), nNew,
                                    buf<uint32_t>(env, idOrderOut), buf<int32_t>(env, replicaSetOut), maxPods));
}
// instance labels kept in the context: the names some type constraint mentions (name i = bit i), then `labels` is read from the
// stored values by podsIngestJson / podsEventsJson (see mmp_label_names_load)
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_labelNamesLoad(JNIEnv *env, jclass, jlong h, jobject names, jobject nameOff, jint nLabels)
{
    if (nLabels > 0 && (!holds<int32_t>(env, nameOff, (jlong)nLabels + 1, "labelNamesLoad: nameOff shorter than nLabels + 1") ||
                        !holds<char>(env, names, buf<int32_t>(env, nameOff)[nLabels], "labelNamesLoad: names shorter than nameOff[nLabels]")))
        return MMP_EINVAL;
    return check(env, ctx_of(h), mmp_label_names_load(ctx_of(h), buf<char>(env, names), buf<int32_t>(env, nameOff), nLabels));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_podLabelsSet(JNIEnv *env, jclass, jlong h, jobject idx, jobject words, jobject counts, jint n)
{
    if (!holds<int32_t>(env, idx, n, "podLabelsSet: idx shorter than n") || !holds<uint64_t>(env, words, n, "podLabelsSet: words shorter than n") ||
        !holds<int32_t>(env, counts, n, "podLabelsSet: counts shorter than n"))
        return MMP_EINVAL;
    return check(env, ctx_of(h), mmp_pod_labels_set(ctx_of(h), buf<int32_t>(env, idx), buf<uint64_t>(env, words), buf<int32_t>(env, counts), n));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_podLabelsGet(JNIEnv *env, jclass, jlong h, jobject wordsOut, jobject countsOut, jint maxPods, jobject nOut)
{
    if ((wordsOut && !holds<uint64_t>(env, wordsOut, maxPods, "podLabelsGet: wordsOut shorter than maxPods")) ||
        (countsOut && !holds<int32_t>(env, countsOut, maxPods, "podLabelsGet: countsOut shorter than maxPods")) ||
        !holds<int32_t>(env, nOut, 1, "podLabelsGet: nOut shorter than one int"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_pod_labels_get(ctx_of(h), buf<uint64_t>(env, wordsOut), buf<int32_t>(env, countsOut), maxPods, buf<int32_t>(env, nOut)));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_typesFromPodLabels(JNIEnv *env, jclass, jlong h, jint nTypes, jobject required, jobject preferred,
                                              jobject allowedOut, jobject preferOut, jobject hasAllowedOut, jobject hasPreferOut)
{
    return check(env, ctx_of(h),
                 mmp_types_from_pod_labels(ctx_of(h), nTypes, buf<uint64_t>(env, required), buf<uint64_t>(env, preferred),
                                           buf<uint64_t>(env, allowedOut), buf<uint64_t>(env, preferOut), buf<uint8_t>(env, hasAllowedOut),
                                           buf<uint8_t>(env, hasPreferOut)));
}
// instance-table events as stored: the raw key and value bytes of each event (see mmp_pods_events_json)
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_podsEventsJson(JNIEnv *env, jclass, jlong h, jobject keys,
                                                                            jobject keyOff, jobject json, jobject off, jint n,
                                                                            jobject deleted, jobject live, jint flags,
                                                                            jobject podIdxOut, jobject startTimeOut,
                                                                            jobject statusOut, jobject nAppendedOut)
{
    if (!holds<int32_t>(env, keyOff, (jlong)n + 1, "podsEventsJson: keyOff shorter than n + 1") ||
        !holds<int64_t>(env, off, (jlong)n + 1, "podsEventsJson: off shorter than n + 1") ||
        (n > 0 && !holds<char>(env, keys, buf<int32_t>(env, keyOff)[n], "podsEventsJson: keys shorter than keyOff[n]")) ||
        (n > 0 && !holds<char>(env, json, buf<int64_t>(env, off)[n], "podsEventsJson: json shorter than off[n]")) ||
        (deleted && !holds<uint8_t>(env, deleted, n, "podsEventsJson: deleted shorter than n")) ||
        (live && !holds<uint8_t>(env, live, n, "podsEventsJson: live shorter than n")) ||
        !holds<int32_t>(env, podIdxOut, n, "podsEventsJson: podIdxOut shorter than n") ||
        (startTimeOut && !holds<int64_t>(env, startTimeOut, n, "podsEventsJson: startTimeOut shorter than n")) ||
        !holds<int32_t>(env, statusOut, n, "podsEventsJson: statusOut shorter than n") ||
        (nAppendedOut && !holds<int32_t>(env, nAppendedOut, 1, "podsEventsJson: nAppendedOut shorter than one int")))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_pods_events_json(ctx_of(h), buf<char>(env, keys), buf<int32_t>(env, keyOff), buf<char>(env, json),
                                      buf<int64_t>(env, off), n, buf<uint8_t>(env, deleted), buf<uint8_t>(env, live),
                                      static_cast<uint32_t>(flags), buf<int32_t>(env, podIdxOut), buf<int64_t>(env, startTimeOut),
                                      buf<int32_t>(env, statusOut), buf<int32_t>(env, nAppendedOut)));
}
// which records name an id the table does not know (see mmp_registry_unresolved); a null modelOut with maxModels 0: sizes only
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_registryUnresolved(JNIEnv *env, jclass, jlong h, jobject modelOut,
                                                                                jint maxModels, jobject nModelsOut,
                                                                                jobject nEntriesOut)
{
    if (!holds<int32_t>(env, modelOut, maxModels, "registryUnresolved: modelOut shorter than maxModels") ||
        !holds<int32_t>(env, nModelsOut, 1, "registryUnresolved: nModelsOut shorter than one int") ||
        !holds<int64_t>(env, nEntriesOut, 1, "registryUnresolved: nEntriesOut shorter than one long"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_registry_unresolved(ctx_of(h), buf<int32_t>(env, modelOut), maxModels, buf<int32_t>(env, nModelsOut),
                                         buf<int64_t>(env, nEntriesOut)));
}

// ---- registry events by key: the model-id table on the device (see mmp_model_ids_load ... mmp_models_events_json) -----------
// The capacities are checked here, as for the instance calls: the library only knows n.
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_modelIdsLoad(JNIEnv *env, jclass, jlong h, jobject ids, jobject idOff,
                                                                          jint nModels)
{
    if (nModels < 0 || !holds<int32_t>(env, idOff, (jlong)nModels + 1, "modelIdsLoad: idOff shorter than nModels + 1") ||
        (nModels > 0 && !holds<char>(env, ids, buf<int32_t>(env, idOff)[nModels], "modelIdsLoad: ids shorter than idOff[nModels]")))
        return MMP_EINVAL;
    return check(env, ctx_of(h), mmp_model_ids_load(ctx_of(h), buf<char>(env, ids), buf<int32_t>(env, idOff), nModels));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_modelIdsResolve(JNIEnv *env, jclass, jlong h, jobject keys,
                                                                             jobject keyOff, jint n, jobject modelIdxOut)
{
    if (n < 0 || !holds<int32_t>(env, keyOff, (jlong)n + 1, "modelIdsResolve: keyOff shorter than n + 1") ||
        (n > 0 && !holds<char>(env, keys, buf<int32_t>(env, keyOff)[n], "modelIdsResolve: keys shorter than keyOff[n]")) ||
        !holds<int32_t>(env, modelIdxOut, n, "modelIdsResolve: modelIdxOut shorter than n"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_model_ids_resolve(ctx_of(h), buf<char>(env, keys), buf<int32_t>(env, keyOff), n, buf<int32_t>(env, modelIdxOut)));
}
// a null bytesOut with maxBytes 0: sizes only; offOut (may be null) holds nRows + 1 ints
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_modelIdsGet(JNIEnv *env, jclass, jlong h, jint firstRow, jint nRows,
                                                                         jobject bytesOut, jint maxBytes, jobject offOut,
                                                                         jobject nBytesOut)
{
    if (nRows < 0 || maxBytes < 0 || !holds<char>(env, bytesOut, maxBytes, "modelIdsGet: bytesOut shorter than maxBytes") ||
        (offOut && !holds<int32_t>(env, offOut, (jlong)nRows + 1, "modelIdsGet: offOut shorter than nRows + 1")) ||
        !holds<int32_t>(env, nBytesOut, 1, "modelIdsGet: nBytesOut shorter than one int"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_model_ids_get(ctx_of(h), firstRow, nRows, buf<char>(env, bytesOut), maxBytes, buf<int32_t>(env, offOut),
                                   buf<int32_t>(env, nBytesOut)));
}
// registry listener events as the listener gets them: the raw key and value bytes of each event (see mmp_models_events_json)
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_modelsEventsJson(JNIEnv *env, jclass, jlong h, jobject keys,
                                                                              jobject keyOff, jobject json, jobject off, jint n,
                                                                              jobject deleted, jint flags, jobject modelIdxOut,
                                                                              jobject lastUnloadOut, jobject statusOut,
                                                                              jobject nAppendedOut)
{
    if (n < 0 || !holds<int32_t>(env, keyOff, (jlong)n + 1, "modelsEventsJson: keyOff shorter than n + 1") ||
        !holds<int64_t>(env, off, (jlong)n + 1, "modelsEventsJson: off shorter than n + 1") ||
        (n > 0 && !holds<char>(env, keys, buf<int32_t>(env, keyOff)[n], "modelsEventsJson: keys shorter than keyOff[n]")) ||
        (n > 0 && !holds<char>(env, json, buf<int64_t>(env, off)[n], "modelsEventsJson: json shorter than off[n]")) ||
        (deleted && !holds<uint8_t>(env, deleted, n, "modelsEventsJson: deleted shorter than n")) ||
        !holds<int32_t>(env, modelIdxOut, n, "modelsEventsJson: modelIdxOut shorter than n") ||
        (lastUnloadOut && !holds<int64_t>(env, lastUnloadOut, n, "modelsEventsJson: lastUnloadOut shorter than n")) ||
        !holds<int32_t>(env, statusOut, n, "modelsEventsJson: statusOut shorter than n") ||
        (nAppendedOut && !holds<int32_t>(env, nAppendedOut, 1, "modelsEventsJson: nAppendedOut shorter than one int")))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_models_events_json(ctx_of(h), buf<char>(env, keys), buf<int32_t>(env, keyOff), buf<char>(env, json),
                                        buf<int64_t>(env, off), n, buf<uint8_t>(env, deleted), static_cast<uint32_t>(flags),
                                        buf<int32_t>(env, modelIdxOut), buf<int64_t>(env, lastUnloadOut), buf<int32_t>(env, statusOut),
                                        buf<int32_t>(env, nAppendedOut)));
}

// ---- the vmodel table on the device (see mmp_vmodels_events_json ... mmp_vmodels_info) -------------------------------------
// The capacities are checked here, as for the registry calls: the library only knows n.
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_vmodelsEventsJson(JNIEnv *env, jclass, jlong h, jobject keys,
                                                                               jobject keyOff, jobject json, jobject off, jint n,
                                                                               jobject deleted, jint flags, jobject vmodelIdxOut,
                                                                               jobject statusOut, jobject nAppendedOut)
{
    if (n < 0 || !holds<int32_t>(env, keyOff, (jlong)n + 1, "vmodelsEventsJson: keyOff shorter than n + 1") ||
        !holds<int64_t>(env, off, (jlong)n + 1, "vmodelsEventsJson: off shorter than n + 1") ||
        (n > 0 && !holds<char>(env, keys, buf<int32_t>(env, keyOff)[n], "vmodelsEventsJson: keys shorter than keyOff[n]")) ||
        (n > 0 && !holds<char>(env, json, buf<int64_t>(env, off)[n], "vmodelsEventsJson: json shorter than off[n]")) ||
        (deleted && !holds<uint8_t>(env, deleted, n, "vmodelsEventsJson: deleted shorter than n")) ||
        !holds<int32_t>(env, vmodelIdxOut, n, "vmodelsEventsJson: vmodelIdxOut shorter than n") ||
        !holds<int32_t>(env, statusOut, n, "vmodelsEventsJson: statusOut shorter than n") ||
        (nAppendedOut && !holds<int32_t>(env, nAppendedOut, 1, "vmodelsEventsJson: nAppendedOut shorter than one int")))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_vmodels_events_json(ctx_of(h), buf<char>(env, keys), buf<int32_t>(env, keyOff), buf<char>(env, json),
                                         buf<int64_t>(env, off), n, buf<uint8_t>(env, deleted), static_cast<uint32_t>(flags),
                                         buf<int32_t>(env, vmodelIdxOut), buf<int32_t>(env, statusOut), buf<int32_t>(env, nAppendedOut)));
}
// nfKeys / nfOff, owners / ownerOff and reqFlags may each be null; rowsOut holds n mmp_vmodel_answer structs
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_vmodelsResolve(JNIEnv *env, jclass, jlong h, jobject keys, jobject keyOff,
                                                                            jint n, jobject nfKeys, jobject nfOff, jobject owners,
                                                                            jobject ownerOff, jobject reqFlags, jobject rowsOut)
{
    if (n < 0 || !holds<int32_t>(env, keyOff, (jlong)n + 1, "vmodelsResolve: keyOff shorter than n + 1") ||
        (n > 0 && !holds<char>(env, keys, buf<int32_t>(env, keyOff)[n], "vmodelsResolve: keys shorter than keyOff[n]")) ||
        (nfOff && !holds<int32_t>(env, nfOff, (jlong)n + 1, "vmodelsResolve: nfOff shorter than n + 1")) ||
        (nfOff && n > 0 && !holds<char>(env, nfKeys, buf<int32_t>(env, nfOff)[n], "vmodelsResolve: nfKeys shorter than nfOff[n]")) ||
        (ownerOff && !holds<int32_t>(env, ownerOff, (jlong)n + 1, "vmodelsResolve: ownerOff shorter than n + 1")) ||
        (ownerOff && n > 0 && !holds<char>(env, owners, buf<int32_t>(env, ownerOff)[n], "vmodelsResolve: owners shorter than ownerOff[n]")) ||
        (reqFlags && !holds<uint32_t>(env, reqFlags, n, "vmodelsResolve: reqFlags shorter than n")) ||
        !holds<mmp_vmodel_answer>(env, rowsOut, n, "vmodelsResolve: rowsOut shorter than n answers"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_vmodels_resolve(ctx_of(h), buf<char>(env, keys), buf<int32_t>(env, keyOff), n, buf<char>(env, nfKeys),
                                     buf<int32_t>(env, nfOff), buf<char>(env, owners), buf<int32_t>(env, ownerOff),
                                     buf<uint32_t>(env, reqFlags), buf<mmp_vmodel_answer>(env, rowsOut)));
}
// a null rowsOut with maxRows 0: nOut and infoOut only; infoOut (may be null) holds one mmp_vmodel_transitions_info
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_vmodelsTransitions(JNIEnv *env, jclass, jlong h, jlong nowMs,
                                                                                jlong lastUsedAgeOnAddMs, jobject rowsOut, jint maxRows,
                                                                                jobject nOut, jobject infoOut)
{
    if (maxRows < 0 || !holds<mmp_vmodel_transition>(env, rowsOut, maxRows, "vmodelsTransitions: rowsOut shorter than maxRows") ||
        !holds<int32_t>(env, nOut, 1, "vmodelsTransitions: nOut shorter than one int") ||
        (infoOut && !holds<mmp_vmodel_transitions_info>(env, infoOut, 1, "vmodelsTransitions: infoOut shorter than one info")))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_vmodels_transitions(ctx_of(h), nowMs, lastUsedAgeOnAddMs, buf<mmp_vmodel_transition>(env, rowsOut), maxRows,
                                         buf<int32_t>(env, nOut), buf<mmp_vmodel_transitions_info>(env, infoOut)));
}
// sizes first: null byte buffers with capacities 0 give nIdBytesOut / nStrBytesOut; idOffOut (nRows + 1 ints), flagsOut (nRows ints)
// and strOffOut (3 nRows + 1 ints) may be null
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_vmodelsGet(JNIEnv *env, jclass, jlong h, jint firstRow, jint nRows,
                                                                        jobject idBytesOut, jint maxIdBytes, jobject idOffOut,
                                                                        jobject nIdBytesOut, jobject flagsOut, jobject strBytesOut,
                                                                        jint maxStrBytes, jobject strOffOut, jobject nStrBytesOut)
{
    if (nRows < 0 || maxIdBytes < 0 || maxStrBytes < 0 ||
        !holds<char>(env, idBytesOut, maxIdBytes, "vmodelsGet: idBytesOut shorter than maxIdBytes") ||
        (idOffOut && !holds<int32_t>(env, idOffOut, (jlong)nRows + 1, "vmodelsGet: idOffOut shorter than nRows + 1")) ||
        !holds<int32_t>(env, nIdBytesOut, 1, "vmodelsGet: nIdBytesOut shorter than one int") ||
        (flagsOut && !holds<uint32_t>(env, flagsOut, nRows, "vmodelsGet: flagsOut shorter than nRows")) ||
        !holds<char>(env, strBytesOut, maxStrBytes, "vmodelsGet: strBytesOut shorter than maxStrBytes") ||
        (strOffOut && !holds<int32_t>(env, strOffOut, 3 * (jlong)nRows + 1, "vmodelsGet: strOffOut shorter than 3 nRows + 1")) ||
        !holds<int32_t>(env, nStrBytesOut, 1, "vmodelsGet: nStrBytesOut shorter than one int"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_vmodels_get(ctx_of(h), firstRow, nRows, buf<char>(env, idBytesOut), maxIdBytes, buf<int32_t>(env, idOffOut),
                                 buf<int32_t>(env, nIdBytesOut), buf<uint32_t>(env, flagsOut), buf<char>(env, strBytesOut), maxStrBytes,
                                 buf<int32_t>(env, strOffOut), buf<int32_t>(env, nStrBytesOut)));
}
// getStatus by model id (mmp_models_status_k): failPod / flags (n ints each) and modelIdxOut (n ints) may be null; a null copiesOut
// with maxCopies 0 gives the sizes only
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_modelsStatusKeyed(JNIEnv *env, jclass, jlong h, jobject keys, jobject keyOff,
                                                                               jint n, jobject failPod, jobject flags, jlong nowMs,
                                                                               jobject modelIdxOut, jobject rowsOut, jobject copiesOut,
                                                                               jint maxCopies, jobject nCopiesOut)
{
    if (n < 0 || maxCopies < 0 || !holds<int32_t>(env, keyOff, (jlong)n + 1, "modelsStatusKeyed: keyOff shorter than n + 1") ||
        (n > 0 && !holds<char>(env, keys, buf<int32_t>(env, keyOff)[n], "modelsStatusKeyed: keys shorter than keyOff[n]")) ||
        (failPod && !holds<int32_t>(env, failPod, n, "modelsStatusKeyed: failPod shorter than n")) ||
        (flags && !holds<uint32_t>(env, flags, n, "modelsStatusKeyed: flags shorter than n")) ||
        (modelIdxOut && !holds<int32_t>(env, modelIdxOut, n, "modelsStatusKeyed: modelIdxOut shorter than n")) ||
        !holds<mmp_status_row>(env, rowsOut, n, "modelsStatusKeyed: rowsOut shorter than n") ||
        !holds<mmp_status_copy>(env, copiesOut, maxCopies, "modelsStatusKeyed: copiesOut shorter than maxCopies") ||
        !holds<int32_t>(env, nCopiesOut, 1, "modelsStatusKeyed: nCopiesOut shorter than one int"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_models_status_k(ctx_of(h), buf<char>(env, keys), buf<int32_t>(env, keyOff), n, buf<int32_t>(env, failPod),
                                     buf<uint32_t>(env, flags), nowMs, buf<int32_t>(env, modelIdxOut), buf<mmp_status_row>(env, rowsOut),
                                     buf<mmp_status_copy>(env, copiesOut), maxCopies, buf<int32_t>(env, nCopiesOut)));
}
// getVModelStatus in full (mmp_vmodels_status): owners / ownerOff, reqFlags and strOffOut (3 n + 1 ints) may be null; vrowsOut holds n
// mmp_vstatus_row structs, rowsOut 2 n mmp_status_row structs; null copiesOut / strBytesOut with capacities 0 give the sizes only
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_vmodelsStatus(JNIEnv *env, jclass, jlong h, jobject keys, jobject keyOff, jint n,
                                                                           jobject owners, jobject ownerOff, jobject reqFlags, jlong nowMs,
                                                                           jobject vrowsOut, jobject rowsOut, jobject copiesOut,
                                                                           jint maxCopies, jobject nCopiesOut, jobject strBytesOut,
                                                                           jint maxStrBytes, jobject strOffOut, jobject nStrBytesOut)
{
    if (n < 0 || maxCopies < 0 || maxStrBytes < 0 || !holds<int32_t>(env, keyOff, (jlong)n + 1, "vmodelsStatus: keyOff shorter than n + 1") ||
        (n > 0 && !holds<char>(env, keys, buf<int32_t>(env, keyOff)[n], "vmodelsStatus: keys shorter than keyOff[n]")) ||
        (ownerOff && !holds<int32_t>(env, ownerOff, (jlong)n + 1, "vmodelsStatus: ownerOff shorter than n + 1")) ||
        (ownerOff && n > 0 && !holds<char>(env, owners, buf<int32_t>(env, ownerOff)[n], "vmodelsStatus: owners shorter than ownerOff[n]")) ||
        (reqFlags && !holds<uint32_t>(env, reqFlags, n, "vmodelsStatus: reqFlags shorter than n")) ||
        !holds<mmp_vstatus_row>(env, vrowsOut, n, "vmodelsStatus: vrowsOut shorter than n rows") ||
        !holds<mmp_status_row>(env, rowsOut, 2 * (jlong)n, "vmodelsStatus: rowsOut shorter than 2 n rows") ||
        !holds<mmp_status_copy>(env, copiesOut, maxCopies, "vmodelsStatus: copiesOut shorter than maxCopies") ||
        !holds<int32_t>(env, nCopiesOut, 1, "vmodelsStatus: nCopiesOut shorter than one int") ||
        !holds<char>(env, strBytesOut, maxStrBytes, "vmodelsStatus: strBytesOut shorter than maxStrBytes") ||
        (strOffOut && !holds<int32_t>(env, strOffOut, 3 * (jlong)n + 1, "vmodelsStatus: strOffOut shorter than 3 n + 1")) ||
        !holds<int32_t>(env, nStrBytesOut, 1, "vmodelsStatus: nStrBytesOut shorter than one int"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_vmodels_status(ctx_of(h), buf<char>(env, keys), buf<int32_t>(env, keyOff), n, buf<char>(env, owners),
                                    buf<int32_t>(env, ownerOff), buf<uint32_t>(env, reqFlags), nowMs, buf<mmp_vstatus_row>(env, vrowsOut),
                                    buf<mmp_status_row>(env, rowsOut), buf<mmp_status_copy>(env, copiesOut), maxCopies,
                                    buf<int32_t>(env, nCopiesOut), buf<char>(env, strBytesOut), maxStrBytes, buf<int32_t>(env, strOffOut),
                                    buf<int32_t>(env, nStrBytesOut)));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_vmodelsInfo(JNIEnv *env, jclass, jlong h, jobject out)
{
    if (!holds<mmp_vmodels_stats>(env, out, 1, "vmodelsInfo: out shorter than one mmp_vmodels_stats")) return MMP_EINVAL;
    return check(env, ctx_of(h), mmp_vmodels_info(ctx_of(h), buf<mmp_vmodels_stats>(env, out)));
}
// rows: n ints (may be null with n == 0); remapOut (may be null) holds maxVmodels ints, nVmodelsAfterOut (may be null) one (see
// mmp_vmodels_retire)
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_vmodelsRetire(JNIEnv *env, jclass, jlong h, jobject rows, jint n, jint flags,
                                                                           jobject remapOut, jint maxVmodels, jobject nVmodelsAfterOut)
{
    if (n < 0 || maxVmodels < 0 || !holds<int32_t>(env, rows, n, "vmodelsRetire: rows shorter than n") ||
        (remapOut && !holds<int32_t>(env, remapOut, maxVmodels, "vmodelsRetire: remapOut shorter than maxVmodels")) ||
        (nVmodelsAfterOut && !holds<int32_t>(env, nVmodelsAfterOut, 1, "vmodelsRetire: nVmodelsAfterOut shorter than one int")))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_vmodels_retire(ctx_of(h), buf<int32_t>(env, rows), n, static_cast<uint32_t>(flags), buf<int32_t>(env, remapOut),
                                    maxVmodels, buf<int32_t>(env, nVmodelsAfterOut)));
}

// the write side of the wire format: the stored value of each edited record and the record as the device holds it give the value
// to store next (see mmp_models_rewrite_json).  The capacities are checked here; outCap is what outBuf holds (0 with null: sizes).
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_modelsRewriteJson(JNIEnv *env, jclass, jlong h, jobject rows, jint n,
                                                                               jobject oldJson, jobject oldOff, jobject lastUnload,
                                                                               jobject failPod, jobject failMsg, jobject failMsgOff,
                                                                               jint flags, jobject outBuf, jlong outCap, jobject outOff,
                                                                               jobject statusOut, jobject nBytesOut)
{
    if (n < 0 || outCap < 0 || !holds<int32_t>(env, rows, n, "modelsRewriteJson: rows shorter than n") ||
        !holds<int64_t>(env, oldOff, (jlong)n + 1, "modelsRewriteJson: oldOff shorter than n + 1") ||
        (n > 0 && !holds<char>(env, oldJson, buf<int64_t>(env, oldOff)[n], "modelsRewriteJson: oldJson shorter than oldOff[n]")) ||
        (lastUnload && !holds<int64_t>(env, lastUnload, n, "modelsRewriteJson: lastUnload shorter than n")) ||
        (failPod && !holds<int32_t>(env, failPod, n, "modelsRewriteJson: failPod shorter than n")) ||
        (failMsgOff && !holds<int32_t>(env, failMsgOff, (jlong)n + 1, "modelsRewriteJson: failMsgOff shorter than n + 1")) ||
        (failMsg && failMsgOff && n > 0 &&
         !holds<char>(env, failMsg, buf<int32_t>(env, failMsgOff)[n], "modelsRewriteJson: failMsg shorter than failMsgOff[n]")) ||
        (outBuf && !holds<char>(env, outBuf, outCap, "modelsRewriteJson: outBuf shorter than outCap")) ||
        !holds<int64_t>(env, outOff, (jlong)n + 1, "modelsRewriteJson: outOff shorter than n + 1") ||
        !holds<int32_t>(env, statusOut, n, "modelsRewriteJson: statusOut shorter than n") ||
        !holds<int64_t>(env, nBytesOut, 1, "modelsRewriteJson: nBytesOut shorter than one long"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_models_rewrite_json(ctx_of(h), buf<int32_t>(env, rows), n, buf<char>(env, oldJson), buf<int64_t>(env, oldOff),
                                         buf<int64_t>(env, lastUnload), buf<int32_t>(env, failPod), buf<char>(env, failMsg),
                                         buf<int32_t>(env, failMsgOff), static_cast<uint32_t>(flags), buf<char>(env, outBuf), outCap,
                                         buf<int64_t>(env, outOff), buf<int32_t>(env, statusOut), buf<int64_t>(env, nBytesOut)));
}

// registerModel / deleteModel as a batch of questions about the stored values (see mmp_models_register_json): reqs = n
// mmp_register_req, infoOff 3n + 1 ints, keys / keyOff / modelIdxOut may be null all three.  The capacities are checked here.
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_modelsRegisterJson(JNIEnv *env, jclass, jlong h, jobject reqs, jint n,
                                                                                jobject keys, jobject keyOff, jobject info,
                                                                                jobject infoOff, jobject oldJson, jobject oldOff,
                                                                                jlong nowMs, jlong lastUsedAgeOnAddMs, jint flags,
                                                                                jobject outBuf, jlong outCap, jobject outOff,
                                                                                jobject classOut, jobject lastUsedOut,
                                                                                jobject modelIdxOut, jobject nBytesOut)
{
    if (n < 0 || n > INT32_MAX / 3 - 1 || outCap < 0 ||
        !holds<mmp_register_req>(env, reqs, n, "modelsRegisterJson: reqs shorter than n") ||
        !holds<int32_t>(env, infoOff, 3 * (jlong)n + 1, "modelsRegisterJson: infoOff shorter than 3n + 1") ||
        !holds<int64_t>(env, oldOff, (jlong)n + 1, "modelsRegisterJson: oldOff shorter than n + 1") ||
        (n > 0 && !holds<char>(env, info, buf<int32_t>(env, infoOff)[3 * n], "modelsRegisterJson: info shorter than infoOff[3n]")) ||
        (n > 0 && !holds<char>(env, oldJson, buf<int64_t>(env, oldOff)[n], "modelsRegisterJson: oldJson shorter than oldOff[n]")) ||
        (modelIdxOut && !holds<int32_t>(env, modelIdxOut, n, "modelsRegisterJson: modelIdxOut shorter than n")) ||
        (modelIdxOut && !holds<int32_t>(env, keyOff, (jlong)n + 1, "modelsRegisterJson: keyOff shorter than n + 1")) ||
        (modelIdxOut && n > 0 && !holds<char>(env, keys, buf<int32_t>(env, keyOff)[n], "modelsRegisterJson: keys shorter than keyOff[n]")) ||
        (outBuf && !holds<char>(env, outBuf, outCap, "modelsRegisterJson: outBuf shorter than outCap")) ||
        !holds<int64_t>(env, outOff, (jlong)n + 1, "modelsRegisterJson: outOff shorter than n + 1") ||
        !holds<int32_t>(env, classOut, n, "modelsRegisterJson: classOut shorter than n") ||
        !holds<int64_t>(env, lastUsedOut, n, "modelsRegisterJson: lastUsedOut shorter than n") ||
        !holds<int64_t>(env, nBytesOut, 1, "modelsRegisterJson: nBytesOut shorter than one long"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_models_register_json(ctx_of(h), buf<mmp_register_req>(env, reqs), n, buf<char>(env, keys), buf<int32_t>(env, keyOff),
                                          buf<char>(env, info), buf<int32_t>(env, infoOff), buf<char>(env, oldJson),
                                          buf<int64_t>(env, oldOff), nowMs, lastUsedAgeOnAddMs, static_cast<uint32_t>(flags),
                                          buf<char>(env, outBuf), outCap, buf<int64_t>(env, outOff), buf<int32_t>(env, classOut),
                                          buf<int64_t>(env, lastUsedOut), buf<int32_t>(env, modelIdxOut), buf<int64_t>(env, nBytesOut)));
}

// incRefCount / decRefCount of the vmodel transactions as a batch of steps on stored values (see mmp_models_refs_json): reqs = n
// mmp_refs_req, info / infoOff (3n + 1 ints) may be null both.  The capacities are checked here.
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_modelsRefsJson(JNIEnv *env, jclass, jlong h, jobject reqs, jint n, jobject info,
                                                                            jobject infoOff, jobject oldJson, jobject oldOff, jint flags,
                                                                            jobject outBuf, jlong outCap, jobject outOff, jobject classOut,
                                                                            jobject refsOut, jobject nBytesOut)
{
    if (n < 0 || n > INT32_MAX / 3 - 1 || outCap < 0 || !holds<mmp_refs_req>(env, reqs, n, "modelsRefsJson: reqs shorter than n") ||
        (infoOff && !holds<int32_t>(env, infoOff, 3 * (jlong)n + 1, "modelsRefsJson: infoOff shorter than 3n + 1")) ||
        !holds<int64_t>(env, oldOff, (jlong)n + 1, "modelsRefsJson: oldOff shorter than n + 1") ||
        (infoOff && n > 0 && !holds<char>(env, info, buf<int32_t>(env, infoOff)[3 * n], "modelsRefsJson: info shorter than infoOff[3n]")) ||
        (n > 0 && !holds<char>(env, oldJson, buf<int64_t>(env, oldOff)[n], "modelsRefsJson: oldJson shorter than oldOff[n]")) ||
        (outBuf && !holds<char>(env, outBuf, outCap, "modelsRefsJson: outBuf shorter than outCap")) ||
        !holds<int64_t>(env, outOff, (jlong)n + 1, "modelsRefsJson: outOff shorter than n + 1") ||
        !holds<int32_t>(env, classOut, n, "modelsRefsJson: classOut shorter than n") ||
        !holds<int32_t>(env, refsOut, n, "modelsRefsJson: refsOut shorter than n") ||
        !holds<int64_t>(env, nBytesOut, 1, "modelsRefsJson: nBytesOut shorter than one long"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_models_refs_json(ctx_of(h), buf<mmp_refs_req>(env, reqs), n, buf<char>(env, info), buf<int32_t>(env, infoOff),
                                      buf<char>(env, oldJson), buf<int64_t>(env, oldOff), static_cast<uint32_t>(flags),
                                      buf<char>(env, outBuf), outCap, buf<int64_t>(env, outOff), buf<int32_t>(env, classOut),
                                      buf<int32_t>(env, refsOut), buf<int64_t>(env, nBytesOut)));
}

// the record step of updateVModel / deleteVModel / PendingTransition.run as a batch (see mmp_vmodels_write_json): reqs = n
// mmp_vmodel_write_req, strOff 3n + 1 ints, rowsOut n mmp_vmodel_write_row; defaultOwner may be null with length 0.  The capacities
// are checked here.
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_vmodelsWriteJson(JNIEnv *env, jclass, jlong h, jobject reqs, jint n, jobject strs,
                                                                              jobject strOff, jobject defaultOwner, jint defaultOwnerLen,
                                                                              jobject oldJson, jobject oldOff, jlong nowMs,
                                                                              jlong lastUsedAgeOnAddMs, jint flags, jobject outBuf,
                                                                              jlong outCap, jobject outOff, jobject rowsOut,
                                                                              jobject nBytesOut)
{
    if (n < 0 || n > INT32_MAX / 3 - 1 || outCap < 0 || defaultOwnerLen < 0 ||
        !holds<mmp_vmodel_write_req>(env, reqs, n, "vmodelsWriteJson: reqs shorter than n") ||
        !holds<int32_t>(env, strOff, 3 * (jlong)n + 1, "vmodelsWriteJson: strOff shorter than 3n + 1") ||
        !holds<int64_t>(env, oldOff, (jlong)n + 1, "vmodelsWriteJson: oldOff shorter than n + 1") ||
        (n > 0 && !holds<char>(env, strs, buf<int32_t>(env, strOff)[3 * n], "vmodelsWriteJson: strs shorter than strOff[3n]")) ||
        (n > 0 && !holds<char>(env, oldJson, buf<int64_t>(env, oldOff)[n], "vmodelsWriteJson: oldJson shorter than oldOff[n]")) ||
        (defaultOwnerLen > 0 && !holds<char>(env, defaultOwner, defaultOwnerLen, "vmodelsWriteJson: defaultOwner shorter than its length")) ||
        (outBuf && !holds<char>(env, outBuf, outCap, "vmodelsWriteJson: outBuf shorter than outCap")) ||
        !holds<int64_t>(env, outOff, (jlong)n + 1, "vmodelsWriteJson: outOff shorter than n + 1") ||
        !holds<mmp_vmodel_write_row>(env, rowsOut, n, "vmodelsWriteJson: rowsOut shorter than n") ||
        !holds<int64_t>(env, nBytesOut, 1, "vmodelsWriteJson: nBytesOut shorter than one long"))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_vmodels_write_json(ctx_of(h), buf<mmp_vmodel_write_req>(env, reqs), n, buf<char>(env, strs), buf<int32_t>(env, strOff),
                                        buf<char>(env, defaultOwner), defaultOwnerLen, buf<char>(env, oldJson), buf<int64_t>(env, oldOff),
                                        nowMs, lastUsedAgeOnAddMs, static_cast<uint32_t>(flags), buf<char>(env, outBuf), outCap,
                                        buf<int64_t>(env, outOff), buf<mmp_vmodel_write_row>(env, rowsOut), buf<int64_t>(env, nBytesOut)));
}

// rows: n ints; remapOut (may be null) holds maxModels ints, nModelsAfterOut (may be null) one (see mmp_models_retire)
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_modelsRetire(JNIEnv *env, jclass, jlong h, jobject rows, jint n, jint flags,
                                                                          jobject remapOut, jint maxModels, jobject nModelsAfterOut)
{
    if (n < 0 || maxModels < 0 || !holds<int32_t>(env, rows, n, "modelsRetire: rows shorter than n") ||
        (remapOut && !holds<int32_t>(env, remapOut, maxModels, "modelsRetire: remapOut shorter than maxModels")) ||
        (nModelsAfterOut && !holds<int32_t>(env, nModelsAfterOut, 1, "modelsRetire: nModelsAfterOut shorter than one int")))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_models_retire(ctx_of(h), buf<int32_t>(env, rows), n, static_cast<uint32_t>(flags), buf<int32_t>(env, remapOut),
                                   maxModels, buf<int32_t>(env, nModelsAfterOut)));
}

// pods: n ints; remapOut (may be null) holds maxPods ints, nPodsAfterOut (may be null) one int, nEntriesUnresolvedOut (may be null)
// one long (see mmp_pods_retire)
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_podsRetire(JNIEnv *env, jclass, jlong h, jobject pods, jint n, jint flags,
                                                                        jobject remapOut, jint maxPods, jobject nPodsAfterOut,
                                                                        jobject nEntriesUnresolvedOut)
{
    if (n < 0 || maxPods < 0 || !holds<int32_t>(env, pods, n, "podsRetire: pods shorter than n") ||
        (remapOut && !holds<int32_t>(env, remapOut, maxPods, "podsRetire: remapOut shorter than maxPods")) ||
        (nPodsAfterOut && !holds<int32_t>(env, nPodsAfterOut, 1, "podsRetire: nPodsAfterOut shorter than one int")) ||
        (nEntriesUnresolvedOut && !holds<int64_t>(env, nEntriesUnresolvedOut, 1, "podsRetire: nEntriesUnresolvedOut shorter than one long")))
        return MMP_EINVAL;
    return check(env, ctx_of(h),
                 mmp_pods_retire(ctx_of(h), buf<int32_t>(env, pods), n, static_cast<uint32_t>(flags), buf<int32_t>(env, remapOut), maxPods,
                                 buf<int32_t>(env, nPodsAfterOut), buf<int64_t>(env, nEntriesUnresolvedOut)));
}

// ---- misc -----------------------------------------------------------------------------------------
JNIEXPORT jlong JNICALL Java_com_ibm_watson_modelmesh_MmPlace_minSpaceUnits(JNIEnv *, jclass,
                                                                            jint defaultModelSizeUnits,
                                                                            jint loadingThreads, jlong capacityUnits,
                                                                            jboolean haveUnloadManager)
{
    return mmp_min_space_units(defaultModelSizeUnits, loadingThreads, capacityUnits, haveUnloadManager ? 1 : 0);
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_getOrder(JNIEnv *env, jclass, jlong h, jobject orderOut,
                                                                      jobject nOut)
{
    return check(env, ctx_of(h), mmp_get_order(ctx_of(h), buf<int32_t>(env, orderOut), buf<int32_t>(env, nOut)));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_deltaCommits(JNIEnv *env, jclass, jlong h, jobject nOut)
{
    return check(env, ctx_of(h), mmp_delta_commits(ctx_of(h), buf<int64_t>(env, nOut)));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_profile(JNIEnv *env, jclass, jlong h, jboolean enable)
{
    return check(env, ctx_of(h), mmp_profile(ctx_of(h), enable ? 1 : 0));
}
JNIEXPORT jdouble JNICALL Java_com_ibm_watson_modelmesh_MmPlace_lastKernelMs(JNIEnv *, jclass, jlong h)
{
    return mmp_last_kernel_ms(ctx_of(h));
}
JNIEXPORT jint JNICALL Java_com_ibm_watson_modelmesh_MmPlace_abiVersion(JNIEnv *, jclass) { return mmp_abi_version(); }

}  // extern "C"
