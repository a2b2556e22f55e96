// registry_harness.cc — `oracle/_ref/registry_harness`: the reference's OWN janitor loops and registry prune, run as C++
// (test infrastructure; fourth binary of oracle/ref_harness, see harness.cc / clhm_harness.cc / tcm_harness.cc).
//
// What executes: janitorTask's cache loop (MM.java:5892-6008) and registry loop (:6014-6108) in ONE function body, so that a
// `return` of the first cancels the second as in the Java; updateLastUsedTimeInRegistryIfStale (:6165-6185),
// repairLastUsedTimeIfNeeded (:6837-6850), CacheEntry.unloadAttemptedRecently (:1864-1866) with age (:4162-4164), VALUE_COMP
// (:6875-6881), pruneModelRegistry (:6524-6609) with pruneMissingInstances (:6752-6784), ModelRecord.removeLoadFailure /
// getLastUsed / setLastUsed / updateLastUsed / updateLastUnloadTime and the constants all of these read — cut out of the
// reference tree by line range at build time (extract.py: REG_RANGES) and #included below.
// What this file adds: class shells, the stand-ins (registry, runtimeCache, CacheEntry, instanceInfo, missings, logger, the clock)
// and a driver that reads cases from stdin and prints WHAT THE STAND-INS SAW AND HOLD — never a re-derivation.
//
// One run has one clock value (currentTimeMillis() and System.currentTimeMillis() both return it): the library's convention.
// unloadManager is null, readOnlyMode false, every conditional set succeeds (conditionalSetAndGet returns its argument).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <list>

#include "javastub.hpp"

std::vector<std::shared_ptr<void>> g_lists_created;

// ---- the clock, the logger, what the text names and no decision reads
static long g_now;
static long currentTimeMillis() { return g_now; }
static long nanoTime() { return 0; }
static long msSince(long) { return 0; }
static String readableTime(long) { return String(""); }
static void publishInstanceRecordAsync() {}
struct Exception {};
static const struct {
    template <class... A> void info(const A &...) const {}
    template <class... A> void warn(const A &...) const {}
    template <class... A> void error(const A &...) const {}
} logger;
static const struct {
    struct { struct { struct R { int getCode() const { return 0; } }; R fromThrowable(const Exception &) const { return R(); } } Status; } grpc;
} io;
static const struct { int UNAVAILABLE = 14; } Code;
static const String LOAD_FAILURE_ENV("MM_LOAD_FAILURE_EXPIRY_TIME_MS");
#define LOAD_FAILURE_EXPIRY_ENV_VAR LOAD_FAILURE_ENV
static long getLongParameter(const String &, long def) { return def; }

#include "../_ref/gen/reg_failure_expiry_constants.inc"
#include "../_ref/gen/reg_janitor_freq_constant.inc"
#include "../_ref/gen/reg_lastused_age_constant.inc"
#include "../_ref/gen/reg_gone_after_constant.inc"
#include "../_ref/gen/reg_short_expiry_constant.inc"

static long age(long timeMillis)
{
#include "../_ref/gen/age_body.inc"
}

// ---- what the stand-ins saw, in call order
static std::vector<std::string> g_log;
static std::string fmt_long(long v) { return std::to_string(v); }

// ---- ModelRecord: the fields the text reads, its own method bodies
struct FailureInfo {
    bool isnull = true;
    FailureInfo() {}
    FailureInfo(std::nullptr_t) {}
    bool operator!=(std::nullptr_t) const { return !isnull; }
    bool operator==(std::nullptr_t) const { return isnull; }
};
struct ModelRecordObj {
    Map<String, Long> instanceIds = Map<String, Long>::make(), loadFailedInstanceIds = Map<String, Long>::make();
    Map<String, FailureInfo> failures = Map<String, FailureInfo>::make();
    long lastUsed = 0, lastUnloadTime = 0;
    boolean removeLoadFailure(const String &instanceId)
    {
#include "../_ref/gen/reg_mr_removeLoadFailure_body.inc"
    }
    long getLastUsed()
    {
#include "../_ref/gen/reg_mr_getLastUsed_body.inc"
    }
    void setLastUsed(long lastUsed)
    {
#include "../_ref/gen/reg_mr_setLastUsed_body.inc"
    }
    void updateLastUsed(long lastUsed)
    {
#include "../_ref/gen/reg_mr_updateLastUsed_body.inc"
    }
    void updateLastUnloadTime()
    {
#include "../_ref/gen/reg_mr_updateLastUnloadTime_body.inc"
    }
};
class ModelRecord {
public:
    std::shared_ptr<ModelRecordObj> p;
    ModelRecord() {}
    ModelRecord(std::nullptr_t) {}
    static ModelRecord make() { ModelRecord m; m.p = std::make_shared<ModelRecordObj>(); return m; }
    bool operator==(std::nullptr_t) const { return !p; }
    bool operator!=(std::nullptr_t) const { return (bool)p; }
    bool operator==(const ModelRecord &o) const { return p == o.p; }  // Java `==`: identity
    bool operator!=(const ModelRecord &o) const { return p != o.p; }
    Map<String, Long> getInstanceIds() const { return p->instanceIds; }
    Map<String, Long> getLoadFailedInstanceIds() const { return p->loadFailedInstanceIds; }
    Map<String, FailureInfo> getLoadFailureInfos() const { return p->failures; }
    boolean removeLoadFailure(const String &i) const { return p->removeLoadFailure(i); }
    long getLastUsed() const { return p->getLastUsed(); }
    void setLastUsed(long v) const { p->setLastUsed(v); }
    void updateLastUsed(long v) const { p->updateLastUsed(v); }
    void updateLastUnloadTime() const { p->updateLastUnloadTime(); }
};
static std::string record_text(const ModelRecord &mr)
{
    std::string s = fmt_long(mr.p->lastUsed) + " " + fmt_long(mr.p->lastUnloadTime) + " " + std::to_string(mr.p->instanceIds.size()) + " " +
                    std::to_string(mr.p->loadFailedInstanceIds.size());
    for (auto &e : mr.p->instanceIds.entrySet()) s += " " + e.getKey().str() + " " + fmt_long(e.getValue());
    for (auto &e : mr.p->loadFailedInstanceIds.entrySet()) s += " " + e.getKey().str() + " " + fmt_long(e.getValue());
    return s;
}

// ---- registry: an ordered map; every conditional set succeeds and is recorded with the record's content at the call
static struct Registry {
    std::map<std::string, ModelRecord> m;
    ModelRecord get(const String &k) const { auto it = m.find(k.str()); return it == m.end() ? ModelRecord(null) : it->second; }
    ModelRecord getStrong(const String &k) const { return get(k); }
    boolean conditionalSet(const String &k, const ModelRecord &mr)
    {
        g_log.push_back("SET " + k.str() + " cs " + record_text(mr));
        m[k.str()] = mr;
        return true;
    }
    ModelRecord conditionalSetAndGet(const String &k, const ModelRecord &mr)
    {
        g_log.push_back("SET " + k.str() + " csg " + record_text(mr));
        m[k.str()] = mr;
        return mr;
    }
    std::vector<Entry<String, ModelRecord>> noThrowIterable() const
    {
        std::vector<Entry<String, ModelRecord>> v;
        for (auto &kv : m) v.emplace_back(String(kv.first), kv.second);
        return v;
    }
} registry;

// ---- the local cache
struct RuntimeCache;
extern RuntimeCache runtimeCache;
class CacheEntry {
public:
    struct Rep { std::string modelId; };
    std::shared_ptr<Rep> p;
    static const int
#include "../_ref/gen/reg_ce_states.inc"
    int state = 0;
    long loadTimestamp = 0, loadCompleteTimestamp = 0, lastUnloadAttemptTime = -1;
    bool done = false, failed_ = false;
    CacheEntry() {}
    CacheEntry(std::nullptr_t) {}
    bool operator==(std::nullptr_t) const { return !p; }
    bool operator!=(std::nullptr_t) const { return (bool)p; }
    boolean isDone() const { return done; }
    boolean isFailed() const { return failed_; }
    boolean unloadAttemptedRecently() const
    {
#include "../_ref/gen/reg_unloadAttemptedRecently_body.inc"
    }
    boolean remove() const;
    int getWeight() const { return 1; }
};
// Map<String, CacheEntry>: runtimeCache.descendingMap() is ordered most recently used first, not by key
template <> class Map<String, CacheEntry> {
public:
    std::shared_ptr<std::vector<std::pair<std::string, CacheEntry>>> p = std::make_shared<std::vector<std::pair<std::string, CacheEntry>>>();
    int size() const { return (int)p->size(); }
    CacheEntry get(const String &k) const
    {
        for (auto &kv : *p)
            if (kv.first == k.str()) return kv.second;
        return CacheEntry(null);
    }
    std::vector<Entry<String, CacheEntry>> entrySet() const
    {
        std::vector<Entry<String, CacheEntry>> es;
        for (auto &kv : *p) es.emplace_back(String(kv.first), kv.second);
        return es;
    }
};
struct RuntimeCache {
    std::vector<std::pair<std::string, CacheEntry>> order;  // MRU first
    std::map<std::string, long> lastUsed;                   // what is in the cache now
    Map<String, CacheEntry> descendingMap() const
    {
        Map<String, CacheEntry> m;
        *m.p = order;
        return m;
    }
    long getLastUsedTime(const String &k) const { auto it = lastUsed.find(k.str()); return it == lastUsed.end() ? -1L : it->second; }
    boolean forceSetLastUsedTime(const String &k, long t)
    {
        g_log.push_back("FORCE " + k.str() + " " + fmt_long(t));
        auto it = lastUsed.find(k.str());
        if (it == lastUsed.end()) return false;
        it->second = t;
        return true;
    }
    CacheEntry getQuietly(const String &k) const
    {
        if (!lastUsed.count(k.str())) return CacheEntry(null);
        for (auto &kv : order)
            if (kv.first == k.str()) return kv.second;
        return CacheEntry(null);
    }
} runtimeCache;
boolean CacheEntry::remove() const
{
    const bool was = runtimeCache.lastUsed.erase(p->modelId) != 0;
    g_log.push_back("REMOVE " + p->modelId + " " + (was ? "1" : "0"));
    return was;
}
static const struct UnloadManager {
    bool operator!=(std::nullptr_t) const { return false; }
    void removeUnloadBufferEntry(const Map<String, CacheEntry> &) const {}
} unloadManager;
static long getAdjustedCacheCapacity() { return 0; }

// ---- the instance table, the missing map
struct InstanceRecordH {
    bool present = false;
    bool operator!=(std::nullptr_t) const { return present; }
};
static struct InstanceInfo {
    std::set<std::string> present;
    boolean contains(const String &k) const { return present.count(k.str()) != 0; }
    InstanceRecordH getStrong(const String &k) const { return InstanceRecordH{contains(k)}; }
} instanceInfo;
static const struct { boolean operator()(const String &k) const { return instanceInfo.contains(k); } } instanceInfo_contains;
static const struct {
    template <class M, class P> M filterKeys(const M &m, const P &) const { return m; }
    template <class K, class V> struct Imm {  // the declared entry type decides how the value is boxed
        K k; V v;
        template <class V2> operator Entry<K, V2>() const { return Entry<K, V2>(k, V2(v)); }
    };
    template <class K, class V> Imm<K, V> immutableEntry(const K &k, const V &v) const { return Imm<K, V>{k, v}; }
} Maps;
static Map<String, Long> missings = Map<String, Long>::make();

// ---- Object[] { modelId, mr, ce } and the TreeSet under VALUE_COMP
struct ObjectArr3 { String modelId; ModelRecord mr; CacheEntry ce; };
struct ValueComp {
    template <class E> int operator()(const E &e1, const E &e2) const
    {
#include "../_ref/gen/reg_value_comp_body.inc"
    }
};
static const ValueComp VALUE_COMP;
template <class E> class SortedSet {
public:
    std::shared_ptr<std::vector<E>> p = std::make_shared<std::vector<E>>();  // kept sorted under the comparator
    boolean add(const E &e) const  // TreeSet.add: an element that compares equal to one present is not added
    {
        size_t i = 0;
        for (; i < p->size(); i++) {
            const int c = VALUE_COMP(e, (*p)[i]);
            if (c == 0) {
                g_log.push_back("TIE " + e.getKey().modelId.str() + " " + fmt_long(e.getValue()));
                return false;
            }
            if (c < 0) break;
        }
        p->insert(p->begin() + i, e);
        return true;
    }
    boolean isEmpty() const { return p->empty(); }
    typename std::vector<E>::const_iterator begin() const { return p->begin(); }
    typename std::vector<E>::const_iterator end() const { return p->end(); }
};
struct SortedSet_new {
    SortedSet_new(const ValueComp &) {}
    template <class E> operator SortedSet<E>() const { return SortedSet<E>(); }
};

// ---- the mesh's fields the text reads
static String instanceId;
static boolean shuttingDown, readOnlyMode = false;
static long loadTimeoutMs, minStaleAge;

static void updateLastUsedTimeInRegistryIfStale(String modelId, ModelRecord mr, long lastUsed)
{
#include "../_ref/gen/reg_updateIfStale_body.inc"
}
static void repairLastUsedTimeIfNeeded(String modelId, ModelRecord mr)
{
#include "../_ref/gen/reg_repairLastUsed_body.inc"
}

// janitorTask.run from :5891 to :6108: the cache loop, the lines between the loops and the registry loop are the text; this file adds
// the declaration of `before` (:5891), a marker where the second loop starts and the label `continue registryLoop` jumps to
static void janitor_run()
{
    long before = nanoTime();
#include "../_ref/gen/reg_janitor_cache_loop.inc"
#include "../_ref/gen/reg_janitor_between_loops.inc"
    g_log.push_back("LOOP2");
#include "../_ref/gen/reg_janitor_registry_loop.inc"
    registryLoop_continue:;
#include "../_ref/gen/reg_janitor_registry_loop_close.inc"
    for (auto &ent : scaleCopiesCandidates)  // at :6108, in the set's order
        g_log.push_back("CAND " + ent.getKey().modelId.str() + " " + fmt_long(ent.getValue()));
    g_log.push_back("REGLOOP " + std::to_string(i) + " " + std::to_string(j));
}

template <class S> static int pruneMissingInstances(Map<String, Long> instances, S secondary, Set<String> notFound)
{
    Map<String, Long> before = Map<String, Long>::make();
    *before.p = *instances.p;
    int rc = [&]() -> int {
#include "../_ref/gen/reg_pruneMissing_body.inc"
    }();
    for (auto &e : before.entrySet())  // what `it.remove()` took out of the map, in entry order
        if (!instances.containsKey(e.getKey())) g_log.push_back(std::string(std::is_same<S, EmptyMapT>::value ? "GONE 0 " : "GONE 1 ") + e.getKey().str() + " " + fmt_long(e.getValue()));
    return rc;
}
static boolean pruneModelRegistry(List<Entry<String, ModelRecord>> proactiveLoadCandidates, long globalLru)
{
#include "../_ref/gen/reg_prune_body.inc"
}

// ---- the driver.  Input (whitespace-separated tokens):
//   R n { modelId lastUsed lastUnloadTime nl nf (id time)*nl (id time)*nf }*n     the registry (replaces it)
//   C n { modelId done failed state loadTimestamp loadCompleteTimestamp lastUnloadAttemptTime lastUsed }*n   the cache, MRU first
//   I n { id }*n                                                                  instanceInfo: the ids it contains
//   M clear                                                                       missings.clear()
//   J self now loadTimeoutMs minStaleAge shuttingDown                             one janitor run
//   P self now wantCandidates globalLru                                           one pruneModelRegistry run
// Output per run: the stand-ins' log in call order, then every record and the missing map as they stand.
static void dump_state(const char *what)
{
    for (auto &l : g_log) printf("%s\n", l.c_str());
    g_log.clear();
    for (auto &kv : registry.m) printf("REC %s %s\n", kv.first.c_str(), record_text(kv.second).c_str());
    for (auto &kv : runtimeCache.lastUsed) printf("CACHE %s %ld\n", kv.first.c_str(), kv.second);
    for (auto &e : missings.entrySet()) printf("MISS %s %ld\n", e.getKey().str().c_str(), (long)e.getValue());
    printf("END %s\n", what);
}

int main()
{
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "R") {
            int n;
            std::cin >> n;
            registry.m.clear();
            for (int k = 0; k < n; k++) {
                std::string id, pod;
                int nl, nf;
                long t;
                ModelRecord mr = ModelRecord::make();
                std::cin >> id >> mr.p->lastUsed >> mr.p->lastUnloadTime >> nl >> nf;
                for (int e = 0; e < nl; e++) { std::cin >> pod >> t; mr.p->instanceIds.put(String(pod), Long(t)); }
                for (int e = 0; e < nf; e++) { std::cin >> pod >> t; mr.p->loadFailedInstanceIds.put(String(pod), Long(t)); }
                registry.m[id] = mr;
            }
        } else if (cmd == "C") {
            int n;
            std::cin >> n;
            runtimeCache.order.clear();
            runtimeCache.lastUsed.clear();
            for (int k = 0; k < n; k++) {
                CacheEntry ce;
                std::string id;
                int done, failed;
                long lu;
                std::cin >> id >> done >> failed >> ce.state >> ce.loadTimestamp >> ce.loadCompleteTimestamp >> ce.lastUnloadAttemptTime >> lu;
                ce.p = std::make_shared<CacheEntry::Rep>(CacheEntry::Rep{id});
                ce.done = done != 0;
                ce.failed_ = failed != 0;
                runtimeCache.order.emplace_back(id, ce);
                runtimeCache.lastUsed[id] = lu;
            }
        } else if (cmd == "I") {
            int n;
            std::cin >> n;
            instanceInfo.present.clear();
            for (int k = 0; k < n; k++) { std::string id; std::cin >> id; instanceInfo.present.insert(id); }
        } else if (cmd == "M") {
            std::string what;
            std::cin >> what;
            missings.p->clear();
        } else if (cmd == "J") {
            std::string self;
            int sd;
            std::cin >> self >> g_now >> loadTimeoutMs >> minStaleAge >> sd;
            instanceId = String(self);
            shuttingDown = sd != 0;
            if (!shuttingDown) janitor_run();  // :5880
            dump_state("J");
        } else if (cmd == "P") {
            std::string self;
            int want;
            long globalLru;
            std::cin >> self >> g_now >> want >> globalLru;
            instanceId = String(self);
            List<Entry<String, ModelRecord>> cands = null;
            if (want) cands = ArrayList_new(0);
            const boolean ok = pruneModelRegistry(cands, globalLru);
            if (want)
                for (int k = 0; k < cands.size(); k++) g_log.push_back("PCAND " + cands.get(k).getKey().str());
            g_log.push_back(std::string("PRUNED ") + (ok ? "1" : "0"));
            dump_state("P");
        } else {
            fprintf(stderr, "registry_harness: unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
