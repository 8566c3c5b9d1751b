// ssm_render.hip -- the device path of map rendering behind the C ABI.  DESIGN.md s.17 is the contract.  A rendering is one upload of a small table (the clouds'
// pointers, sizes and relative poses -- worked out on the host by carve_core.h's rel_pose, the same 12 doubles the host function uses -- and each block's first
// cloud), the launches of kernels_render.hip on the main stream, one download of the info and ONE wait.  The z-buffer and the images belong to the target, the
// table and the staging of the host-array call to the context (RenderWork) and grow with the largest call.  The host functions, the defaults and the argument
// checks are ssm_render_host.cpp.
#include "ssm_ctx.h"
#include "ssm_host.h"
using namespace ssm_renderc;

static int render_reserve(ssm_ctx* c, size_t m, size_t nb)
{
    RenderWork& W = c->render;
    if (m <= W.cap_m && nb <= W.cap_b && W.info) return SSM_OK;
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    const size_t mm = std::max(std::max(m, W.cap_m), (size_t)8), bb = std::max(std::max(nb, W.cap_b), (size_t)1024);
    W.cap_m = 0; W.cap_b = 0;
    const size_t bytes = mm * sizeof(RenderSeg) + bb * 4;
    DALLOC(c, W.table, bytes); DALLOC(c, W.h_table, bytes);
    DALLOC(c, W.info, 4); DALLOC(c, W.h_info, 4); DALLOC(c, W.counts, 9); DALLOC(c, W.h_counts, 9);
    W.cap_m = mm; W.cap_b = bb;
    return SSM_OK;
}
// segs: pts, n and M filled by the caller; everything from the table's upload to the call's wait
static int render_run(ssm_ctx* c, ssm_render_target* t, const Setup& S, std::vector<RenderSeg>& segs, int64_t total, ssm_render_info* info)
{
    RenderWork& W = c->render; hipStream_t s = c->main.stream;
    const int m = (int)segs.size();
    const int64_t T = k_render_block(), nb = (total + T - 1) / T;
    { const int r = render_reserve(c, (size_t)m, (size_t)nb); if (r) return r; }
    RenderSeg* hs = reinterpret_cast<RenderSeg*>((uint8_t*)W.h_table);
    int32_t* hb = reinterpret_cast<int32_t*>((uint8_t*)W.h_table + (size_t)m * sizeof(RenderSeg));
    int64_t at = 0;
    for (int k = 0; k < m; k++) { segs[k].off = at; segs[k].pad = 0; hs[k] = segs[k]; at += segs[k].n; }
    for (int64_t b = 0, k = 0; b < nb; b++) { while (b * T >= segs[k].off + segs[k].n) k++; hb[b] = (int32_t)k; }
    const size_t bytes = (size_t)m * sizeof(RenderSeg) + (size_t)nb * 4;
    if (bytes) HIPCHK(c, hipMemcpyAsync(W.table, W.h_table, bytes, hipMemcpyHostToDevice, s));
    const RenderImgs I{t->keys, t->depth, t->bgr, t->label, t->index};
    t->rendered = false;
    prof_begin(c, s, "render");
    HIPCHK(c, k_render(S, W.table.as<RenderSeg>(), reinterpret_cast<const int32_t*>((uint8_t*)W.table + (size_t)m * sizeof(RenderSeg)), m, total, I, W.info, s));
    prof_end(c, s);
    HIPCHK(c, hipMemcpyAsync(W.h_info, W.info, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
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
{
    if (!t) return;
    if (c) { std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device); hipStreamSynchronize(c->main.stream); }
    delete t;
}
extern "C" int ssm_render_points(ssm_ctx* c, ssm_render_target* t, const ssm_camera* cam, const double* T_view, const ssm_point* const* pts, const int32_t* n,
                                 const double* T_clouds, int m, const ssm_render_params* params, ssm_render_info* info)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    Setup S;
    { const int r = render_begin(c, t, cam, T_view, params, &S); if (r) return r; }
    if (m < 0 || (m && (!pts || !n || !T_clouds))) FAIL(c, SSM_E_INVAL, "null argument");
    int64_t total = 0;
    { const int r = render_total_check(c, n, m, &total); if (r) return r; }
    std::vector<RenderSeg> segs((size_t)m);
    for (int k = 0; k < m; k++) {
        if (n[k] && !pts[k]) FAIL(c, SSM_E_INVAL, "null argument");
        { const int r = carve_pose_check(c, T_clouds + 16 * k); if (r) return r; }
        ssm_carvec::rel_pose(T_view, T_clouds + 16 * k, segs[k].M);
    }
    RenderWork& W = c->render; hipStream_t s = c->main.stream;
    const size_t nn = (size_t)std::max<int64_t>(total, 1);
    if (nn > W.in_cap) { HIPCHK(c, hipStreamSynchronize(s)); W.in_cap = 0; DALLOC(c, W.in, nn); W.in_cap = nn; }
    size_t at = 0;
    for (int k = 0; k < m; k++) {
        if (n[k]) HIPCHK(c, hipMemcpyAsync(W.in + at, pts[k], (size_t)n[k] * sizeof(ssm_point), hipMemcpyHostToDevice, s));
        segs[k].pts = W.in + at; segs[k].n = n[k]; at += (size_t)n[k];
    }
    return render_run(c, t, S, segs, total, info);
}
extern "C" int ssm_render_clouds(ssm_ctx* c, ssm_render_target* t, const ssm_camera* cam, const double* T_view, ssm_cloud* const* clouds, const double* T_clouds, int m,
                                 const ssm_render_params* params, ssm_render_info* info)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    Setup S;
    { const int r = render_begin(c, t, cam, T_view, params, &S); if (r) return r; }
    if (m < 0 || (m && (!clouds || !T_clouds))) FAIL(c, SSM_E_INVAL, "null argument");
    std::vector<RenderSeg> segs((size_t)m);
    int64_t total = 0;
    for (int k = 0; k < m; k++) {
        const ssm_cloud* cl = clouds[k];
        if (!cl) FAIL(c, SSM_E_INVAL, "null argument");
        if (cl->device != c->device) FAIL(c, SSM_E_INVAL, "cloud of another device");
        { const int r = carve_pose_check(c, T_clouds + 16 * k); if (r) return r; }
        ssm_carvec::rel_pose(T_view, T_clouds + 16 * k, segs[k].M);
        segs[k].pts = cl->d; segs[k].n = cl->n; total += cl->n;
    }
    if (total >= ((int64_t)1 << 32)) FAIL(c, SSM_E_INVAL, "render: 2^32 points or more in one call");
    return render_run(c, t, S, segs, total, info);
}
extern "C" int ssm_render_viewer_map(ssm_ctx* c, ssm_render_target* t, const ssm_camera* cam, const double* T_view, const ssm_render_params* params, ssm_render_info* info)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    Setup S;
    { const int r = render_begin(c, t, cam, T_view, params, &S); if (r) return r; }
    if (!c->d_vmap || c->vmap_n <= 0) FAIL(c, SSM_E_INVAL, "render: the context holds no viewer map");
    static const double EYE[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::vector<RenderSeg> segs(1);
    ssm_carvec::rel_pose(T_view, EYE, segs[0].M);
    segs[0].pts = c->d_vmap; segs[0].n = c->vmap_n;
    return render_run(c, t, S, segs, c->vmap_n, info);
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
    { const int r = render_reserve(c, 0, 0); if (r) return r; }
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
