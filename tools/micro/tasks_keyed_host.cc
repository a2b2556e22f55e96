// Host side of the four periodic tasks by model id (mmp_scaleup_plan_k, mmp_scaledown_plan_k, mmp_migration_plan_k,
// mmp_janitor_plan_k) for the AddressSanitizer / UndefinedBehaviorSanitizer build of the library: a stand-alone program, itself
// instrumented, so no runtime has to be preloaded.  It walks what the entry points decide on the host before they touch the
// device — the NULL and negative arguments, one key pointer without the other, the chain's arguments — with every output buffer
// guarded by a canary, and checks that a refused call wrote nothing.  Without a device mmp_create fails and the walk is the
// whole run (the library has no CPU path); with one the same refusals are repeated on a live context before the first commit,
// where every call must answer MMP_ESTATE or MMP_EINVAL.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -shared -fPIC -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer \
//         -Wno-unused-function modelmesh_amd/csrc/mmplace.hip -o /tmp/libmmplace_asan.so -ldl -lpthread
//   hipcc -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude tools/micro/tasks_keyed_host.cc \
//         -L/tmp -lmmplace_asan -Wl,-rpath,/tmp -lpthread -o /tmp/tasks_keyed_host
#include <cstdio>
#include <cstring>
#include <vector>

#include "mmplace.h"

static int g_fail = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            g_fail++;                                                  \
            fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #cond);    \
        }                                                              \
    } while (0)

template <class T>
static bool canary(const std::vector<T> &v)
{
    const unsigned char *p = reinterpret_cast<const unsigned char *>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(T); i++)
        if (p[i] != 0xA5) return false;
    return true;
}
template <class T>
static std::vector<T> filled(size_t n)
{
    std::vector<T> v(n);
    memset(v.data(), 0xA5, n * sizeof(T));
    return v;
}

static void walk(mmp_ctx *c, int refused_a, int refused_b)
{
    const int n = 3;
    const char keys[] = "abcdefghi";
    const int32_t off[4] = {0, 3, 6, 9};
    std::vector<mmp_cache_entry> e(n);
    std::vector<mmp_janitor_entry> j(n);
    std::vector<mmp_conc_entry> conc(n);
    memset(e.data(), 0, n * sizeof(mmp_cache_entry));
    memset(j.data(), 0, n * sizeof(mmp_janitor_entry));
    memset(conc.data(), 0, n * sizeof(mmp_conc_entry));
    mmp_scaleup_params sp;
    mmp_scaledown_params dp;
    mmp_janitor_params jp;
    mmp_conc_params cp;
    memset(&sp, 0, sizeof sp);
    memset(&dp, 0, sizeof dp);
    memset(&jp, 0, sizeof jp);
    memset(&cp, 0, sizeof cp);
    jp.now = sp.now = dp.now = 1760000000000LL;
    auto idx = filled<int32_t>(n), rows = filled<int32_t>(n), skipped = filled<int32_t>(1);
    auto outs = filled<mmp_scaleup_out>(n);
    auto couts = filled<mmp_conc_out>(n);
    auto res = filled<mmp_conc_result>(1);
    auto ov = filled<uint8_t>(64), rem = filled<uint8_t>(n), act = filled<uint8_t>(n), wait = filled<uint8_t>(n);
    auto edits = filled<mmp_janitor_edit>(n);
    auto cands = filled<mmp_cache_entry>(n);
    auto info = filled<mmp_janitor_info>(1);
    auto ok = [&](int rc) { return rc == refused_a || rc == refused_b; };
    // one key pointer without the other
    EXPECT(mmp_scaleup_plan_k(c, e.data(), nullptr, n, keys, nullptr, &sp, nullptr, outs.data(), nullptr, ov.data(), skipped.data(), nullptr, idx.data()) == MMP_EINVAL);
    EXPECT(mmp_scaledown_plan_k(c, e.data(), nullptr, n, nullptr, off, &dp, 0, rem.data(), idx.data()) == MMP_EINVAL);
    EXPECT(mmp_migration_plan_k(c, e.data(), n, keys, nullptr, 0, jp.now, 3600000, act.data(), wait.data(), idx.data()) == MMP_EINVAL);
    EXPECT(mmp_janitor_plan_k(c, j.data(), n, nullptr, off, &jp, 0, nullptr, nullptr, 0, idx.data(), act.data(), edits.data(), n, cands.data(), rows.data(), n,
                              nullptr, info.data()) == MMP_EINVAL);
    // NULL required buffers, negative counts, the chain's arguments
    EXPECT(mmp_scaleup_plan_k(c, e.data(), nullptr, n, keys, off, &sp, nullptr, nullptr, nullptr, ov.data(), skipped.data(), nullptr, idx.data()) == MMP_EINVAL);
    EXPECT(mmp_scaleup_plan_k(c, e.data(), conc.data(), n, keys, off, &sp, nullptr, outs.data(), nullptr, ov.data(), skipped.data(), nullptr, idx.data()) == MMP_EINVAL);
    EXPECT(mmp_scaleup_plan_k(c, e.data(), conc.data(), n, keys, off, &sp, &cp, outs.data(), couts.data(), ov.data(), skipped.data(), nullptr, idx.data()) == MMP_EINVAL);
    EXPECT(mmp_scaledown_plan_k(c, e.data(), nullptr, -1, keys, off, &dp, 0, rem.data(), idx.data()) == MMP_EINVAL);
    EXPECT(mmp_scaledown_plan_k(c, e.data(), nullptr, n, keys, off, &dp, 0, nullptr, idx.data()) == MMP_EINVAL);
    EXPECT(mmp_migration_plan_k(c, nullptr, n, keys, off, 0, jp.now, 3600000, act.data(), wait.data(), idx.data()) == MMP_EINVAL);
    EXPECT(mmp_janitor_plan_k(c, j.data(), n, keys, off, &jp, 3u, nullptr, nullptr, 0, idx.data(), act.data(), edits.data(), n, cands.data(), rows.data(), n, nullptr,
                              info.data()) == MMP_EINVAL);
    EXPECT(mmp_janitor_plan_k(c, j.data(), n, keys, off, &jp, 0, &dp, nullptr, 0, idx.data(), act.data(), edits.data(), n, cands.data(), rows.data(), n, rem.data(),
                              info.data()) == MMP_EINVAL);  // the chain without MMP_JANITOR_APPLY
    EXPECT(mmp_janitor_plan_k(c, j.data(), n, keys, off, &jp, MMP_JANITOR_APPLY, nullptr, conc.data(), 0, idx.data(), act.data(), edits.data(), n, cands.data(),
                              rows.data(), n, nullptr, info.data()) == MMP_EINVAL);  // conc without scaledown
    EXPECT(mmp_janitor_plan_k(c, j.data(), n, keys, off, &jp, MMP_JANITOR_APPLY, &dp, nullptr, 0, idx.data(), act.data(), edits.data(), n, cands.data(), rows.data(),
                              n, nullptr, info.data()) == MMP_EINVAL);  // the chain without removed_out
    // well-formed calls: refused for the context's state (or for the NULL context), still nothing written
    EXPECT(ok(mmp_scaleup_plan_k(c, e.data(), nullptr, n, keys, off, &sp, nullptr, outs.data(), nullptr, ov.data(), skipped.data(), nullptr, idx.data())));
    EXPECT(ok(mmp_scaledown_plan_k(c, e.data(), conc.data(), n, keys, off, &dp, 60000, rem.data(), idx.data())));
    EXPECT(ok(mmp_migration_plan_k(c, e.data(), n, keys, off, 0, jp.now, 3600000, act.data(), wait.data(), idx.data())));
    EXPECT(ok(mmp_janitor_plan_k(c, j.data(), n, keys, off, &jp, MMP_JANITOR_APPLY, &dp, conc.data(), 60000, idx.data(), act.data(), edits.data(), n, cands.data(),
                                 rows.data(), n, rem.data(), info.data())));
    EXPECT(ok(mmp_janitor_plan_k(c, j.data(), n, nullptr, nullptr, &jp, 0, nullptr, nullptr, 0, nullptr, act.data(), edits.data(), n, cands.data(), rows.data(), n,
                                 nullptr, info.data())));
    EXPECT(canary(idx) && canary(rows) && canary(skipped) && canary(outs) && canary(couts) && canary(res) && canary(ov) && canary(rem) && canary(act) &&
           canary(wait) && canary(edits) && canary(cands) && canary(info));
}

int main()
{
    walk(nullptr, MMP_EINVAL, MMP_EINVAL);
    mmp_config cfg;
    memset(&cfg, 0, sizeof cfg);
    mmp_ctx *c = nullptr;
    if (mmp_create(&cfg, &c) != MMP_OK) c = nullptr;
    if (c) {  // a device: the same walk on a live context before the first commit
        walk(c, MMP_ESTATE, MMP_EINVAL);
        mmp_destroy(c);
    }
    printf("tasks_keyed_host: %s context, %d failures\n", c ? "NULL and live" : "NULL (no device)", g_fail);
    return g_fail ? 1 : 0;
}
