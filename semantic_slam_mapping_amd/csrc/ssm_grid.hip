// ssm_grid.hip -- the device path of the ground grid behind the C ABI.  DESIGN.md s.19 is the contract.  A build is one upload of the cloud table (cloud_table.h;
// the grid poses M_k = G . T_cloud_k are worked out on the host by grid_core.h's grid_pose, the same 12 doubles the host function uses), the launches of
// kernels_grid.hip on the main stream, one download of the info and ONE wait.  The cells and the output arrays belong to the target, the table and the staging of
// the host-array call to the context (CloudTableWork).  The host function, the defaults and the argument checks are ssm_grid_host.cpp.
#include "ssm_ctx.h"
#include "ssm_host.h"
using namespace ssm_gridc;

static std::atomic<int64_t> g_grid_builds{0};          // every build of every target has a number of its own: what ssm_objects.hip remembers of the build it labelled
// what every build checks first
static int grid_begin(ssm_ctx* c, ssm_grid_target* t, const ssm_grid_params* params, ssm_grid_params* P, Setup* S)
{
    if (!t) FAIL(c, SSM_E_INVAL, "null argument");
    if (t->device != c->device) FAIL(c, SSM_E_INVAL, "target of another device");
    ssm_grid_params_default(P); if (params) *P = *params;
    { const int r = grid_check(c, *P, S); if (r) return r; }
    if ((int64_t)P->nx * P->ny > t->cap) FAIL(c, SSM_E_INVAL, "grid: more cells than the target has");
    return SSM_OK;
}
// segs: pts and n filled by cloud_list; everything from the grid poses and the table's upload to the call's wait
static int grid_run(ssm_ctx* c, ssm_grid_target* t, const ssm_grid_params& P, const Setup& S, std::vector<CloudSeg>& segs, const double* T_clouds, ssm_grid_info* info)
{
    GridWork& W = c->grid; hipStream_t s = c->main.stream;
    if (!W.info) { DALLOC(c, W.h_info, 10); DALLOC(c, W.info, 10); }
    for (size_t k = 0; k < segs.size(); k++) grid_pose(P.G, T_clouds + 16 * k, segs[k].M);
    CloudTable tab;
    { const int r = cloud_table_upload(c, segs, k_grid_block(), &tab); if (r) return r; }
    const GridBufs B{t->cells, t->cls, t->ground_label, t->obstacle_label, t->ground_q, t->top_q, t->n, t->n_high};
    t->built = false;
    prof_begin(c, s, "grid");
    HIPCHK(c, k_grid(S, tab.seg, tab.blk, tab.total, B, W.info, W.form, s));
    prof_end(c, s);
    static_assert(sizeof(ssm_grid_info) == 80, "info is ten 64-bit counts");
    HIPCHK(c, hipMemcpyAsync(W.h_info, W.info, 80, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    tab.in_flight = nullptr;
    t->built = true; t->nx = S.nx; t->ny = S.ny; t->params = P; t->builds = ++g_grid_builds; t->n_in = tab.total;
    unsigned long long* hi = W.h_info;
    hi[1] = hi[0] - hi[1];                       // the kernels count the rejected points: n_finite = n_in - rejected
    if (info) memcpy(info, hi, 80);
    return SSM_OK;
}

extern "C" int ssm_grid_target_create(ssm_ctx* c, int nx, int ny, ssm_grid_target** out)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (!out) FAIL(c, SSM_E_INVAL, "null argument");
    *out = nullptr;
    if (nx < 1 || ny < 1 || (int64_t)nx * ny > MAX_CELLS) FAIL(c, SSM_E_INVAL, "grid: at least 1 x 1 and at most 2^24 cells");
    std::unique_ptr<ssm_grid_target> t(new ssm_grid_target());
    const size_t nc = (size_t)nx * ny;
    t->cap = (int64_t)nc; t->device = c->device; t->owner = c;
    DALLOC(c, t->cells, nc); DALLOC(c, t->cls, nc); DALLOC(c, t->ground_label, nc); DALLOC(c, t->obstacle_label, nc); DALLOC(c, t->ground_q, nc); DALLOC(c, t->top_q, nc);
    DALLOC(c, t->n, nc); DALLOC(c, t->n_high, nc);
    *out = t.release();
    return SSM_OK;
}
extern "C" void ssm_grid_target_free(ssm_ctx* c, ssm_grid_target* t)
{ free_after_wait(c, t); }
extern "C" int ssm_grid_points(ssm_ctx* c, ssm_grid_target* t, const ssm_point* const* pts, const int32_t* n, const double* T_clouds, int m, const ssm_grid_params* params,
                               ssm_grid_info* info)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    ssm_grid_params P; Setup S;
    { const int r = grid_begin(c, t, params, &P, &S); if (r) return r; }
    std::vector<CloudSeg> segs; int64_t total = 0;
    { const int r = cloud_call(c, cloud_arrays(pts, n, T_clouds, m), grid_cloud_rule(), CLOUD_EYE, segs, &total); if (r) return r; }
    return grid_run(c, t, P, S, segs, T_clouds, info);
}
extern "C" int ssm_grid_clouds(ssm_ctx* c, ssm_grid_target* t, ssm_cloud* const* clouds, const double* T_clouds, int m, const ssm_grid_params* params, ssm_grid_info* info)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    ssm_grid_params P; Setup S;
    { const int r = grid_begin(c, t, params, &P, &S); if (r) return r; }
    std::vector<CloudSeg> segs; int64_t total = 0;
    { const int r = cloud_call(c, cloud_handles(clouds, T_clouds, m), grid_cloud_rule(), CLOUD_EYE, segs, &total); if (r) return r; }
    return grid_run(c, t, P, S, segs, T_clouds, info);
}
extern "C" int ssm_grid_viewer_map(ssm_ctx* c, ssm_grid_target* t, const ssm_grid_params* params, ssm_grid_info* info)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    ssm_grid_params P; Setup S;
    { const int r = grid_begin(c, t, params, &P, &S); if (r) return r; }
    std::vector<CloudSeg> segs; int64_t total = 0;
    { const int r = cloud_call(c, cloud_viewer_map("grid: the context holds no viewer map"), grid_cloud_rule(), CLOUD_EYE, segs, &total); if (r) return r; }
    return grid_run(c, t, P, S, segs, CLOUD_EYE, info);
}
static int grid_target_ready(ssm_ctx* c, const ssm_grid_target* t)
{
    if (!t) FAIL(c, SSM_E_INVAL, "null argument");
    if (t->device != c->device) FAIL(c, SSM_E_INVAL, "target of another device");
    if (!t->built) FAIL(c, SSM_E_INVAL, "grid: nothing has been built into the target");
    return SSM_OK;
}
extern "C" int ssm_grid_fetch(ssm_ctx* c, const ssm_grid_target* t, uint8_t* cls, uint8_t* ground_label, uint8_t* obstacle_label, int32_t* ground_q, int32_t* top_q,
                              uint32_t* n, uint32_t* n_high)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    { const int r = grid_target_ready(c, t); if (r) return r; }
    hipStream_t s = c->main.stream; const size_t nc = (size_t)t->nx * t->ny;
    if (cls) HIPCHK(c, hipMemcpyAsync(cls, t->cls, nc, hipMemcpyDeviceToHost, s));
    if (ground_label) HIPCHK(c, hipMemcpyAsync(ground_label, t->ground_label, nc, hipMemcpyDeviceToHost, s));
    if (obstacle_label) HIPCHK(c, hipMemcpyAsync(obstacle_label, t->obstacle_label, nc, hipMemcpyDeviceToHost, s));
    if (ground_q) HIPCHK(c, hipMemcpyAsync(ground_q, t->ground_q, nc * 4, hipMemcpyDeviceToHost, s));
    if (top_q) HIPCHK(c, hipMemcpyAsync(top_q, t->top_q, nc * 4, hipMemcpyDeviceToHost, s));
    if (n) HIPCHK(c, hipMemcpyAsync(n, t->n, nc * 4, hipMemcpyDeviceToHost, s));
    if (n_high) HIPCHK(c, hipMemcpyAsync(n_high, t->n_high, nc * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return SSM_OK;
}
extern "C" int ssm_debug_grid_form(ssm_ctx* c, int form)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (form < -1 || form > GRID_FORM_RUNS) FAIL(c, SSM_E_INVAL, "grid: the accumulate form is 0 (per point), 1 (per run) or -1 (the default)");
    c->grid.form = form < 0 ? (int)GRID_FORM_DEFAULT : form;
    return SSM_OK;
}
extern "C" int ssm_debug_grid_cells(ssm_ctx* c, const ssm_grid_target* t, ssm_grid_cell* cells)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    { const int r = grid_target_ready(c, t); if (r) return r; }
    if (!cells) FAIL(c, SSM_E_INVAL, "null argument");
    HIPCHK(c, hipMemcpyAsync(cells, t->cells, (size_t)t->nx * t->ny * sizeof(ssm_grid_cell), hipMemcpyDeviceToHost, c->main.stream));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    return SSM_OK;
}
