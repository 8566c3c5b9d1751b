// ssm_render.hip -- the device path of map rendering behind the C ABI.  DESIGN.md s.17 is the contract.  A rendering is one upload of the cloud table
// (cloud_table.h; the relative poses are worked out on the host by carve_core.h's rel_pose, the same 12 doubles the host function uses), the launches of
// kernels_render.hip on the main stream, one download of the info and ONE wait.  The z-buffer and the images belong to the target, the table and the staging
// of the host-array call to the context (CloudTableWork) and grow with the largest call.  The host functions, the defaults and the argument
// checks are ssm_render_host.cpp.
#include "ssm_ctx.h"
#include "ssm_host.h"
using namespace ssm_renderc;

// the info and the counts, made by the first call that needs them
static int render_work(ssm_ctx* c)
{
    RenderWork& W = c->render;
    if (!W.info) { DALLOC(c, W.h_info, 4); DALLOC(c, W.counts, 9); DALLOC(c, W.h_counts, 9); DALLOC(c, W.info, 4); }
    return SSM_OK;
}
// segs: pts, n and M filled by cloud_call; everything from the table's upload to the call's wait
static int render_run(ssm_ctx* c, ssm_render_target* t, const Setup& S, std::vector<CloudSeg>& segs, ssm_render_info* info)
{
    RenderWork& W = c->render; hipStream_t s = c->main.stream;
    { const int r = render_work(c); if (r) return r; }
    CloudTable tab;
    { const int r = cloud_table_upload(c, segs, k_render_block(), &tab); if (r) return r; }
    const RenderImgs I{t->keys, t->depth, t->bgr, t->label, t->index};
    t->rendered = false;
    prof_begin(c, s, "render");
    HIPCHK(c, k_render(S, tab.seg, tab.blk, (int)segs.size(), tab.total, I, W.info, s));
    prof_end(c, s);
    HIPCHK(c, hipMemcpyAsync(W.h_info, W.info, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    tab.in_flight = nullptr;
    t->rendered = true;
    static_assert(sizeof(ssm_render_info) == 16, "info is four ints");
    if (info) memcpy(info, (const int32_t*)W.h_info, 16);
    return SSM_OK;
}
// what every rendering call checks first
static int render_begin(ssm_ctx* c, ssm_render_target* t, const ssm_camera* cam, const double* T_view, const ssm_render_params* params, Setup* S)
{
    if (!t) FAIL(c, SSM_E_INVAL, "null argument");
    if (t->device != c->device) FAIL(c, SSM_E_INVAL, "target of another device");
    ssm_render_params P; ssm_render_params_default(&P); if (params) P = *params;
    int r = render_check(c, t->w, t->h, cam, P, S); if (!r) r = carve_pose_check(c, T_view);
    return r;
}

extern "C" int ssm_render_target_create(ssm_ctx* c, int w, int h, ssm_render_target** out)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (!out) FAIL(c, SSM_E_INVAL, "null argument");
    *out = nullptr;
    { const int r = render_size_check(c, w, h); if (r) return r; }
    std::unique_ptr<ssm_render_target> t(new ssm_render_target());
    t->w = w; t->h = h; t->device = c->device;
    const size_t np = (size_t)w * h;
    DALLOC(c, t->keys, np); DALLOC(c, t->depth, np); DALLOC(c, t->bgr, np * 3); DALLOC(c, t->label, np); DALLOC(c, t->index, np);
    DALLOC(c, t->f_depth, np); DALLOC(c, t->f_sem, np * 3); DALLOC(c, t->cls, np);
    *out = t.release();
    return SSM_OK;
}
extern "C" void ssm_render_target_free(ssm_ctx* c, ssm_render_target* t)
{ free_after_wait(c, t); }
extern "C" int ssm_render_points(ssm_ctx* c, ssm_render_target* t, const ssm_camera* cam, const double* T_view, const ssm_point* const* pts, const int32_t* n,
                                 const double* T_clouds, int m, const ssm_render_params* params, ssm_render_info* info)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    Setup S;
    { const int r = render_begin(c, t, cam, T_view, params, &S); if (r) return r; }
    std::vector<CloudSeg> segs; int64_t total = 0;
    { const int r = cloud_call(c, cloud_arrays(pts, n, T_clouds, m), render_cloud_rule(), T_view, segs, &total); if (r) return r; }
    return render_run(c, t, S, segs, info);
}
extern "C" int ssm_render_clouds(ssm_ctx* c, ssm_render_target* t, const ssm_camera* cam, const double* T_view, ssm_cloud* const* clouds, const double* T_clouds, int m,
                                 const ssm_render_params* params, ssm_render_info* info)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    Setup S;
    { const int r = render_begin(c, t, cam, T_view, params, &S); if (r) return r; }
    std::vector<CloudSeg> segs; int64_t total = 0;
    { const int r = cloud_call(c, cloud_handles(clouds, T_clouds, m), render_cloud_rule(), T_view, segs, &total); if (r) return r; }
    return render_run(c, t, S, segs, info);
}
extern "C" int ssm_render_viewer_map(ssm_ctx* c, ssm_render_target* t, const ssm_camera* cam, const double* T_view, const ssm_render_params* params, ssm_render_info* info)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    Setup S;
    { const int r = render_begin(c, t, cam, T_view, params, &S); if (r) return r; }
    std::vector<CloudSeg> segs; int64_t total = 0;
    { const int r = cloud_call(c, cloud_viewer_map("render: the context holds no viewer map"), render_cloud_rule(), T_view, segs, &total); if (r) return r; }
    return render_run(c, t, S, segs, info);
}
static int render_target_ready(ssm_ctx* c, const ssm_render_target* t)
{
    if (!t) FAIL(c, SSM_E_INVAL, "null argument");
    if (t->device != c->device) FAIL(c, SSM_E_INVAL, "target of another device");
    if (!t->rendered) FAIL(c, SSM_E_INVAL, "render: nothing has been rendered into the target");
    return SSM_OK;
}
extern "C" int ssm_render_fetch(ssm_ctx* c, const ssm_render_target* t, uint16_t* depth, uint8_t* bgr, uint8_t* label, int32_t* index)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    { const int r = render_target_ready(c, t); if (r) return r; }
    hipStream_t s = c->main.stream; const size_t np = (size_t)t->w * t->h;
    if (depth) HIPCHK(c, hipMemcpyAsync(depth, t->depth, np * 2, hipMemcpyDeviceToHost, s));
    if (bgr) HIPCHK(c, hipMemcpyAsync(bgr, t->bgr, np * 3, hipMemcpyDeviceToHost, s));
    if (label) HIPCHK(c, hipMemcpyAsync(label, t->label, np, hipMemcpyDeviceToHost, s));
    if (index) HIPCHK(c, hipMemcpyAsync(index, t->index, np * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return SSM_OK;
}
extern "C" int ssm_debug_render_keys(ssm_ctx* c, const ssm_render_target* t, uint64_t* keys)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    { const int r = render_target_ready(c, t); if (r) return r; }
    if (!keys) FAIL(c, SSM_E_INVAL, "null argument");
    HIPCHK(c, hipMemcpyAsync(keys, t->keys, (size_t)t->w * t->h * 8, hipMemcpyDeviceToHost, c->main.stream));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    return SSM_OK;
}
extern "C" int ssm_render_compare(ssm_ctx* c, ssm_render_target* t, const uint16_t* depth, const uint8_t* sem_bgr, double cam_scale, const ssm_render_params* params,
                                  ssm_render_compare_info* info, uint8_t* class_img)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    { const int r = render_target_ready(c, t); if (r) return r; }
    ssm_render_params P; ssm_render_params_default(&P); if (params) P = *params;
    int64_t tol_abs = 0;
    { const int r = render_compare_check(c, P, cam_scale, &tol_abs); if (r) return r; }
    if (!depth || !sem_bgr) FAIL(c, SSM_E_INVAL, "null argument");
    { const int r = render_work(c); if (r) return r; }
    RenderWork& W = c->render; hipStream_t s = c->main.stream;
    const size_t np = (size_t)t->w * t->h;
    HIPCHK(c, hipMemcpyAsync(t->f_depth, depth, np * 2, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(t->f_sem, sem_bgr, np * 3, hipMemcpyHostToDevice, s));
    prof_begin(c, s, "render_compare");
    HIPCHK(c, k_render_compare(t->depth, t->label, t->f_depth, t->f_sem, (int64_t)np, tol_abs, P.tol_rel_ppm, t->cls, W.counts, s));
    prof_end(c, s);
    HIPCHK(c, hipMemcpyAsync(W.h_counts, W.counts, 72, hipMemcpyDeviceToHost, s));
    if (class_img) HIPCHK(c, hipMemcpyAsync(class_img, t->cls, np, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    static_assert(sizeof(ssm_render_compare_info) == 72, "info is nine 64-bit counts");
    if (info) memcpy(info, (const unsigned long long*)W.h_counts, 72);
    return SSM_OK;
}
