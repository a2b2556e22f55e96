/* The C ABI from plain C (C99, no C++/Python): build a 4-instance table and one model, commit, ask for one
 * load target — what a JNI / cgo / FFI host does through its binding.  Needs a GPU to run (mmp_create fails
 * with MMP_ENODEVICE otherwise; there is no CPU path).
 *   gcc -std=c99 -Iinclude examples/place_one.c -Lmodelmesh_amd/lib -lmmplace -Wl,-rpath,$PWD/modelmesh_amd/lib -o /tmp/place_one
 */
#include <stdio.h>
#include <string.h>

#include "mmplace.h"

int main(void)
{
    mmp_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.device = 0;
    cfg.min_space_units = mmp_min_space_units(6400, 8, 8388608, 1); /* MM.java:765-771 */
    cfg.min_churn_age_ms = 600000;
    mmp_ctx *ctx = NULL;
    int rc = mmp_create(&cfg, &ctx);
    if (rc != MMP_OK) {
        fprintf(stderr, "mmp_create: %d (%s)\n", rc, mmp_last_error(NULL));
        return rc == MMP_ENODEVICE ? 77 : 1;
    }
    const int64_t now = 1760000000000LL;
    mmp_pod_row pods[4];
    memset(pods, 0, sizeof pods);
    for (int p = 0; p < 4; p++) {
        pods[p].lru_time = now - 3600000 - p;
        pods[p].capacity = 8388608;
        pods[p].used = 1000000 * (p + 1); /* pod 0 has the most free space */
        pods[p].version = 1;
        pods[p].count = 5;
        pods[p].loading_threads = 8;
        pods[p].id_order = (uint32_t)p;
        pods[p].replica_set = 0;
        pods[p].flags = MMP_POD_LIVE;
    }
    mmp_model_row model;
    memset(&model, 0, sizeof model);
    model.n_loaded = 1; /* already loaded on pod 0: excluded from the load targets */
    int32_t ent_pod[1] = {0};
    int64_t ent_time[1] = {now - 60000};
    mmp_place_req rq;
    memset(&rq, 0, sizeof rq);
    rq.self_pod = 3;
    rq.fresh_lru = pods[3].lru_time;
    rq.fresh_capacity = pods[3].capacity;
    rq.fresh_used = pods[3].used;
    rq.fresh_count = pods[3].count;
    mmp_place_out out;
    if ((rc = mmp_pods_load(ctx, pods, 4)) || (rc = mmp_models_load(ctx, &model, 1, ent_pod, ent_time, 1)) ||
        (rc = mmp_snapshot_commit(ctx)) || (rc = mmp_place_batch(ctx, &rq, 1, NULL, 0, now, &out))) {
        fprintf(stderr, "libmmplace: %d (%s)\n", rc, mmp_last_error(ctx));
        mmp_destroy(ctx);
        return 1;
    }
    printf("chosen=%d best=%d candidates=%d\n", out.chosen, out.best, out.n_candidates);
    /* The same request with the model named by its id: the registry's rows are named once (mmp_model_ids_load), then a request
     * brings the id's bytes and the library resolves them on the device inside the call (mmp_place_batch_ck). */
    const char ids[] = "my-model";
    const int32_t id_off[2] = {0, (int32_t)sizeof ids - 1};
    mmp_place_caller caller;
    memset(&caller, 0, sizeof caller);
    caller.self_pod = rq.self_pod;
    caller.fresh_lru = rq.fresh_lru;
    caller.fresh_capacity = rq.fresh_capacity;
    caller.fresh_used = rq.fresh_used;
    caller.fresh_count = rq.fresh_count;
    mmp_place_req_c rc_row;
    memset(&rc_row, 0, sizeof rc_row);
    rc_row.model = -1; /* ignored: the key names the model */
    mmp_place_out keyed;
    int32_t row = -2;
    if ((rc = mmp_model_ids_load(ctx, ids, id_off, 1)) ||
        (rc = mmp_place_batch_ck(ctx, &caller, &rc_row, 1, ids, id_off, NULL, 0, now, &keyed, &row))) {
        fprintf(stderr, "libmmplace: %d (%s)\n", rc, mmp_last_error(ctx));
        mmp_destroy(ctx);
        return 1;
    }
    printf("by id: row=%d chosen=%d best=%d candidates=%d\n", row, keyed.chosen, keyed.best, keyed.n_candidates);
    /* And with the request naming a VMODEL: the vmodel listener's one event makes "my-vmodel" point at "my-model"; a request brings
     * the vmodel id's bytes, resolveVModelId runs on the device inside the call (mmp_place_batch_cv), and the host reads the class
     * of the answer before it believes the decision. */
    const char vids[] = "my-vmodel";
    const int32_t vid_off[2] = {0, (int32_t)sizeof vids - 1};
    const char record[] = "{\"amid\":\"my-model\",\"tmid\":\"my-model\"}";
    const int64_t rec_off[2] = {0, (int64_t)sizeof record - 1};
    int32_t vrow = -2, vstatus = -2;
    mmp_place_out by_vmodel;
    mmp_vseam_row vm;
    if ((rc = mmp_vmodels_events_json(ctx, vids, vid_off, record, rec_off, 1, NULL, MMP_VMEV_APPEND, &vrow, &vstatus, NULL)) ||
        (rc = mmp_place_batch_cv(ctx, &caller, &rc_row, 1, vids, vid_off, NULL, NULL, NULL, NULL, 0, now, &by_vmodel, &vm))) {
        fprintf(stderr, "libmmplace: %d (%s)\n", rc, mmp_last_error(ctx));
        mmp_destroy(ctx);
        return 1;
    }
    printf("by vmodel id: class=%d vmodel=%d model=%d chosen=%d best=%d candidates=%d\n", vm.cls, vm.vmodel, vm.model, by_vmodel.chosen,
           by_vmodel.best, by_vmodel.n_candidates);
    /* The management path by id: getVModelStatus of "my-vmodel" in one call (mmp_vmodels_status) — the vmodel's row, the status of
     * its active and target model with their copies, and the three strings of the reply, all of one state. */
    mmp_vstatus_row vs;
    mmp_status_row st_rows[2];
    mmp_status_copy st_copies[4];
    char strs[64];
    int32_t str_off[4], n_copies = -1, n_str = -1;
    if ((rc = mmp_vmodels_status(ctx, vids, vid_off, 1, NULL, NULL, NULL, now, &vs, st_rows, st_copies, 4, &n_copies, strs, (int32_t)sizeof strs,
                                 str_off, &n_str))) {
        fprintf(stderr, "libmmplace: %d (%s)\n", rc, mmp_last_error(ctx));
        mmp_destroy(ctx);
        return 1;
    }
    printf("status by vmodel id: class=%d vstatus=%d active: class=%d copies=%d, active id \"%.*s\"\n", vs.cls, vs.vstatus, st_rows[0].cls,
           st_rows[0].n_not_checked + st_rows[0].n_failed, (int)(str_off[1] - str_off[0]), strs + str_off[0]);
    /* A periodic task by id: preShutdown asks, for the one entry of this instance's cache, whether a copy is to be triggered
     * elsewhere (mmp_migration_plan_k) — the cache holds ids, so the entry's model field stays -1 and the id's bytes name it. */
    mmp_cache_entry ce;
    memset(&ce, 0, sizeof ce);
    ce.model = -1; /* ignored: the key names the model */
    ce.weight = 100;
    ce.last_used = now - 1000;
    uint8_t mig_action = 9, mig_wait = 9;
    int32_t mig_row = -2;
    if ((rc = mmp_migration_plan_k(ctx, &ce, 1, ids, id_off, 0, now, 3600000, &mig_action, &mig_wait, &mig_row))) {
        fprintf(stderr, "libmmplace: %d (%s)\n", rc, mmp_last_error(ctx));
        mmp_destroy(ctx);
        return 1;
    }
    printf("migration by id: row=%d action=%d wait=%d\n", mig_row, mig_action, mig_wait);
    mmp_destroy(ctx);
    if (mig_row != 0 || mig_action > 1 || mig_wait > 1) return 6;
    if (vs.cls != MMP_VMR_OK || vs.model != 0 || vs.vstatus != MMP_VMS_DEFINED || st_rows[0].cls != MMP_MST_ASK || n_copies != 1 ||
        st_rows[1].cls != MMP_MST_NOT_FOUND || n_str != 16 || memcmp(strs, "my-modelmy-model", 16) != 0)
        return 5;
    /* pod 0 holds the model, so the most desirable eligible pod is pod 1; the id names row 0 and decides the same, and so does the
     * vmodel whose active model it is */
    if (row != 0 || memcmp(&keyed, &out, sizeof out) != 0) return 3;
    if (vm.cls != MMP_VMR_OK || vm.which != MMP_VMW_ACTIVE || vm.vmodel != 0 || vm.model != 0 || vm.flags != 0 ||
        memcmp(&by_vmodel, &out, sizeof out) != 0)
        return 4;
    return out.best == 1 ? 0 : 2;
}
