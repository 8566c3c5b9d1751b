// ssm_objects.hip -- the device path of object extraction behind the C ABI.  DESIGN.md s.21 is the contract.  Stage 1 is the launches of kernels_objects.hip on the
// main stream with TWO waits: one for the number of components, from which the record buffers are sized (as vocabulary training reads its flag between launches),
// one for the info.  Stage 2 is one upload of the cloud table (cloud_table.h; the grid poses are grid_core.h's grid_pose under the grid build's remembered
// parameters), two launches, one download of the info and one wait.  The labelling's arrays and the records belong to the target, the info, the per-point ids and
// the staging of hand-made cells to the context.  The host functions, the defaults and the argument checks are ssm_objects_host.cpp.
#include "ssm_ctx.h"
#include "ssm_host.h"
using namespace ssm_objc;

static int objects_work(ssm_ctx* c)
{
    ObjectsWork& W = c->objects;
    if (!W.info) { DALLOC(c, W.h_info, 8); DALLOC(c, W.h_count, 1); DALLOC(c, W.info, 8); }
    return SSM_OK;
}
static int objects_target_ok(ssm_ctx* c, const ssm_objects_target* t)
{
    if (!t) FAIL(c, SSM_E_INVAL, "null argument");
    if (t->owner != c) FAIL(c, SSM_E_INVAL, "objects: target of another context");
    return SSM_OK;
}
static int objects_grid_ok(ssm_ctx* c, const ssm_grid_target* g)
{
    if (!g) FAIL(c, SSM_E_INVAL, "null argument");
    if (g->owner != c) FAIL(c, SSM_E_INVAL, "objects: grid target of another context");
    if (!g->built) FAIL(c, SSM_E_INVAL, "objects: nothing has been built into the grid target");
    return SSM_OK;
}
// stage 1 on cell arrays in device memory, from the first launch to the call's last wait
static int objects_stage1(ssm_ctx* c, ssm_objects_target* t, const ObjectsCells& G, const Setup& S, ssm_objects_info* info)
{
    { const int r = objects_work(c); if (r) return r; }
    ObjectsWork& W = c->objects; hipStream_t s = c->main.stream;
    const int64_t nc = (int64_t)G.nx * G.ny;
    const ObjectsBufs B{t->labels, t->isroot, t->rank, t->object_id, t->loc, t->tmp, t->tmp_bytes};
    t->staged = false;
    prof_begin(c, s, "objects_cells");
    HIPCHK(c, k_objects_label(G, S, B, W.info, s));
    HIPCHK(c, hipMemcpyAsync(W.h_count, t->rank + nc, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));                                           // the number of components sizes the records
    const int32_t C = *W.h_count;
    if (C > t->comp_cap) {
        t->comp_cap = 0;
        DALLOC(c, t->comp, C); DALLOC(c, t->objs, C); DALLOC(c, t->keep, (size_t)C + 1); DALLOC(c, t->kid, (size_t)C + 1);
        t->comp_cap = C;
    }
    HIPCHK(c, k_objects_records(G, S, B, C, t->comp, t->keep, t->kid, t->objs, W.info, s));
    prof_end(c, s);
    static_assert(sizeof(ssm_objects_info) == 64, "info is eight 64-bit counts");
    HIPCHK(c, hipMemcpyAsync(W.h_info, W.info, 64, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    t->staged = true; t->nx = G.nx; t->ny = G.ny; t->K = (int)W.h_info[2];
    if (info) memcpy(info, W.h_info, 64);
    return SSM_OK;
}

extern "C" int ssm_objects_target_create(ssm_ctx* c, int nx, int ny, ssm_objects_target** out)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (!out) FAIL(c, SSM_E_INVAL, "null argument");
    *out = nullptr;
    if (nx < 1 || ny < 1 || (int64_t)nx * ny > ssm_gridc::MAX_CELLS) FAIL(c, SSM_E_INVAL, "objects: at least 1 x 1 and at most 2^24 cells");
    std::unique_ptr<ssm_objects_target> t(new ssm_objects_target());
    const size_t nc = (size_t)nx * ny;
    t->cap = (int64_t)nc; t->device = c->device; t->owner = c;
    DALLOC(c, t->labels, nc); DALLOC(c, t->isroot, nc + 1); DALLOC(c, t->rank, nc + 1); DALLOC(c, t->object_id, nc); DALLOC(c, t->loc, nc);
    t->tmp_bytes = k_objects_tmp_bytes((int64_t)nc);
    DALLOC(c, t->tmp, t->tmp_bytes);
    *out = t.release();
    return SSM_OK;
}
extern "C" void ssm_objects_target_free(ssm_ctx* c, ssm_objects_target* t)
{ free_after_wait(c, t); }

extern "C" int ssm_objects_grid(ssm_ctx* c, const ssm_grid_target* g, const ssm_objects_params* params, ssm_objects_target* t, ssm_objects_info* info)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    { const int r = objects_target_ok(c, t); if (r) return r; }
    { const int r = objects_grid_ok(c, g); if (r) return r; }
    ssm_objects_params P; ssm_objects_params_default(&P); if (params) P = *params;
    Setup S;
    { const int r = objects_check(c, P, &S); if (r) return r; }
    if ((int64_t)g->nx * g->ny > t->cap) FAIL(c, SSM_E_INVAL, "objects: the grid has more cells than the target");
    { const int r = objects_extent_check(c, g->params.x0, g->params.y0, g->params.cell, g->nx, g->ny); if (r) return r; }
    const ObjectsCells G{g->cls, g->obstacle_label, g->ground_q, g->top_q, g->n_high, g->nx, g->ny};
    { const int r = objects_stage1(c, t, G, S, info); if (r) return r; }
    t->grid = g; t->grid_build = g->builds;
    return SSM_OK;
}
extern "C" int ssm_debug_objects_cells(ssm_ctx* c, ssm_objects_target* t, const uint8_t* cls, const uint8_t* obstacle_label, const int32_t* ground_q, const int32_t* top_q,
                                       const uint32_t* n_high, int nx, int ny, const ssm_objects_params* params, ssm_objects_info* info)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    { const int r = objects_target_ok(c, t); if (r) return r; }
    if (!cls || !obstacle_label || !ground_q || !top_q || !n_high) FAIL(c, SSM_E_INVAL, "null argument");
    ssm_objects_params P; ssm_objects_params_default(&P); if (params) P = *params;
    Setup S;
    { const int r = objects_check(c, P, &S); if (r) return r; }
    if (nx < 1 || ny < 1 || (int64_t)nx * ny > t->cap) FAIL(c, SSM_E_INVAL, "objects: at least 1 x 1 cells and at most the target's");
    ObjectsWork& W = c->objects; hipStream_t s = c->main.stream;
    const size_t nc = (size_t)nx * ny;
    {   // a built grid holds fewer than 2^31 points, which is what lets the device add a tile's n_high in 32 bits: hand-made cells must keep to it
        uint64_t sum = 0;
        for (size_t i = 0; i < nc; i++) sum += n_high[i];
        if (sum >= (uint64_t)ssm_gridc::MAX_POINTS) FAIL(c, SSM_E_INVAL, "objects: the cells' n_high must sum to fewer than 2^31 points");
    }
    if ((int64_t)nc > W.in_cap) {
        HIPCHK(c, hipStreamSynchronize(s)); W.in_cap = 0;
        DALLOC(c, W.in_cls, nc); DALLOC(c, W.in_label, nc); DALLOC(c, W.in_ground, nc); DALLOC(c, W.in_top, nc); DALLOC(c, W.in_high, nc);
        W.in_cap = (int64_t)nc;
    }
    HIPCHK(c, hipMemcpyAsync(W.in_cls, cls, nc, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(W.in_label, obstacle_label, nc, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(W.in_ground, ground_q, nc * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(W.in_top, top_q, nc * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(W.in_high, n_high, nc * 4, hipMemcpyHostToDevice, s));
    const ObjectsCells G{W.in_cls, W.in_label, W.in_ground, W.in_top, W.in_high, nx, ny};
    { const int r = objects_stage1(c, t, G, S, info); if (r) return r; }
    t->grid = nullptr; t->grid_build = 0;
    return SSM_OK;
}

// what every stage-2 call checks first
static int objects_points_begin(ssm_ctx* c, const ssm_grid_target* g, const ssm_objects_target* t, ssm_gridc::Setup* GS)
{
    { const int r = objects_target_ok(c, t); if (r) return r; }
    { const int r = objects_grid_ok(c, g); if (r) return r; }
    if (!t->staged || !t->grid || t->grid != g) FAIL(c, SSM_E_INVAL, "objects: the cells of this grid target have not been labelled (ssm_objects_grid comes first)");
    if (t->grid_build != g->builds) FAIL(c, SSM_E_INVAL, "objects: the grid target has been built again since its cells were labelled");
    return grid_check(c, g->params, GS);
}
static int objects_count_check(ssm_ctx* c, const ssm_grid_target* g, int64_t total)
{
    if (total != g->n_in) FAIL(c, SSM_E_INVAL, "objects: the clouds hold " + std::to_string(total) + " points, the grid was built from " + std::to_string(g->n_in));
    return SSM_OK;
}
// segs: pts and n filled by cloud_call; everything from the grid poses and the table's upload to the call's wait
static int objects_points_run(ssm_ctx* c, const ssm_grid_target* g, ssm_objects_target* t, const ssm_gridc::Setup& GS, std::vector<CloudSeg>& segs, int64_t total,
                              const double* T_clouds, int32_t* ids_out, ssm_objects_info* info)
{
    { const int r = objects_count_check(c, g, total); if (r) return r; }
    { const int r = objects_work(c); if (r) return r; }
    ObjectsWork& W = c->objects; hipStream_t s = c->main.stream;
    if (std::max<int64_t>(total, 1) > W.ids_cap) { HIPCHK(c, hipStreamSynchronize(s)); W.ids_cap = 0; DALLOC(c, W.ids, std::max<int64_t>(total, 1)); W.ids_cap = std::max<int64_t>(total, 1); }
    W.n_ids = -1;
    for (size_t k = 0; k < segs.size(); k++) ssm_gridc::grid_pose(g->params.G, T_clouds + 16 * k, segs[k].M);
    CloudTable tab;
    { const int r = cloud_table_upload(c, segs, k_objects_block(), &tab); if (r) return r; }
    prof_begin(c, s, "objects_points");
    HIPCHK(c, k_objects_points(GS, tab.seg, tab.blk, tab.total, g->cells, t->object_id, t->objs, t->K, W.ids, W.info, W.form, s));
    prof_end(c, s);
    HIPCHK(c, hipMemcpyAsync(W.h_info, W.info, 64, hipMemcpyDeviceToHost, s));
    if (ids_out && total) HIPCHK(c, hipMemcpyAsync(ids_out, W.ids, (size_t)total * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    tab.in_flight = nullptr;
    W.n_ids = total;
    if (info) memcpy(info, W.h_info, 64);
    return SSM_OK;
}
extern "C" int ssm_objects_clouds(ssm_ctx* c, const ssm_grid_target* g, ssm_objects_target* t, ssm_cloud* const* clouds, const double* T_clouds, int m, ssm_objects_info* info)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    ssm_gridc::Setup GS;
    { const int r = objects_points_begin(c, g, t, &GS); if (r) return r; }
    std::vector<CloudSeg> segs; int64_t total = 0;
    { const int r = cloud_call(c, cloud_handles(clouds, T_clouds, m), objects_cloud_rule(), CLOUD_EYE, segs, &total); if (r) return r; }
    return objects_points_run(c, g, t, GS, segs, total, T_clouds, nullptr, info);
}
extern "C" int ssm_objects_points(ssm_ctx* c, const ssm_grid_target* g, ssm_objects_target* t, const ssm_point* const* pts, const int32_t* n, const double* T_clouds, int m,
                                  int32_t* ids_out, ssm_objects_info* info)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    ssm_gridc::Setup GS;
    { const int r = objects_points_begin(c, g, t, &GS); if (r) return r; }
    std::vector<CloudSeg> segs; int64_t total = 0;
    // the counts alone say whether these can be the grid's clouds: refused before an array is read or staged (a count is the caller's word for its array's size)
    if (m < 0 || (m && (!pts || !n || !T_clouds))) FAIL(c, SSM_E_INVAL, "null argument");
    { const int r = cloud_total_check(c, objects_cloud_rule(), n, m, &total); if (r) return r; }
    { const int r = objects_count_check(c, g, total); if (r) return r; }
    { const int r = cloud_call(c, cloud_arrays(pts, n, T_clouds, m), objects_cloud_rule(), CLOUD_EYE, segs, &total); if (r) return r; }
    return objects_points_run(c, g, t, GS, segs, total, T_clouds, ids_out, info);
}
extern "C" int ssm_objects_viewer_map(ssm_ctx* c, const ssm_grid_target* g, ssm_objects_target* t, ssm_objects_info* info)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    ssm_gridc::Setup GS;
    { const int r = objects_points_begin(c, g, t, &GS); if (r) return r; }
    std::vector<CloudSeg> segs; int64_t total = 0;
    { const int r = cloud_call(c, cloud_viewer_map("objects: the context holds no viewer map"), objects_cloud_rule(), CLOUD_EYE, segs, &total); if (r) return r; }
    return objects_points_run(c, g, t, GS, segs, total, CLOUD_EYE, nullptr, info);
}
extern "C" int ssm_objects_fetch(ssm_ctx* c, const ssm_objects_target* t, ssm_object* out, int cap, int* n_out, int32_t* object_id)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    { const int r = objects_target_ok(c, t); if (r) return r; }
    if (!t->staged) FAIL(c, SSM_E_INVAL, "objects: no cells have been labelled into the target");
    if (cap < 0 || (out && !n_out)) FAIL(c, SSM_E_INVAL, "null argument");
    if (n_out) *n_out = t->K;
    if (out && t->K > cap) FAIL(c, SSM_E_CAPACITY, "record buffer too small (need " + std::to_string(t->K) + ")");
    hipStream_t s = c->main.stream;
    if (out && t->K) HIPCHK(c, hipMemcpyAsync(out, t->objs, (size_t)t->K * sizeof(ssm_object), hipMemcpyDeviceToHost, s));
    if (object_id) HIPCHK(c, hipMemcpyAsync(object_id, t->object_id, (size_t)t->nx * t->ny * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return SSM_OK;
}
extern "C" int ssm_debug_objects_form(ssm_ctx* c, int form)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (form < -1 || form > OBJECTS_FORM_RUNS) FAIL(c, SSM_E_INVAL, "objects: the accumulate form is 0 (per point), 1 (per run) or -1 (the default)");
    c->objects.form = form < 0 ? (int)OBJECTS_FORM_DEFAULT : form;
    return SSM_OK;
}
extern "C" int ssm_debug_objects_point_ids(ssm_ctx* c, int32_t* out, int64_t n)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    ObjectsWork& W = c->objects;
    if (W.n_ids < 0) FAIL(c, SSM_E_INVAL, "objects: no points have been assigned on this context");
    if (n != W.n_ids || (n && !out)) FAIL(c, SSM_E_INVAL, "objects: the last call assigned " + std::to_string(W.n_ids) + " points");
    if (n) HIPCHK(c, hipMemcpyAsync(out, W.ids, (size_t)n * 4, hipMemcpyDeviceToHost, c->main.stream));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    return SSM_OK;
}
extern "C" int ssm_debug_objects_tile_w(void) { return k_objects_tile_w(); }
extern "C" int ssm_debug_objects_tile_h(void) { return k_objects_tile_h(); }
