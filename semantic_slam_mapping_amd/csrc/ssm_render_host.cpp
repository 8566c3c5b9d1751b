// ssm_render_host.cpp -- map rendering on the CPU: ssm_render_host, ssm_render_compare_host, the palette image, the parameter defaults and the
// argument checks the device entry points share.  Plain C++ over include/ssm/render_core.h with one thread: a loop over the points and a minimum per pixel where
// the device path has one thread per point and an integer atomic minimum.
#include "ssm_host.h"
using namespace ssm_renderc;

extern "C" void ssm_render_params_default(ssm_render_params* p)
{
    if (!p) return;
    p->point_size = 0.0; p->max_radius = 3; p->pad = 0; p->z_min = 0.1; p->z_max = 1.0e9; p->tol_abs = 0.05; p->tol_rel_ppm = 20000; p->pad2 = 0;
}
static int render_tol_check(ssm_ctx* c, const ssm_render_params& P, double scale)
{
    using namespace ssm_carvec;
    if (!(P.tol_abs >= 0.0 && P.tol_abs <= TOL_ABS_MAX)) return host_fail(c, SSM_E_INVAL, "render: tol_abs must be finite, 0..1e6 m");
    if (P.tol_rel_ppm < 0 || P.tol_rel_ppm > PPM_MAX) return host_fail(c, SSM_E_INVAL, "render: tol_rel_ppm must be 0..1000000");
    if (!(scale > 0.0 && scale <= SCALE_MAX)) return host_fail(c, SSM_E_INVAL, "render: the camera's scale must be in (0, 1e6]");
    return SSM_OK;
}
int render_size_check(ssm_ctx* c, int w, int h)
{
    if (w < 1 || h < 1 || (int64_t)w * h > MAX_PIXELS) return host_fail(c, SSM_E_INVAL, "render: the view must be at least 1 x 1 and at most 2^26 pixels");
    return SSM_OK;
}
int render_check(ssm_ctx* c, int w, int h, const ssm_camera* cam, const ssm_render_params& P, Setup* S)
{
    using ssm_carvec::finite_d;
    if (!cam) return host_fail(c, SSM_E_INVAL, "null argument");
    { const int r = render_size_check(c, w, h); if (r) return r; }
    if (P.max_radius < 0 || P.max_radius > MAX_RADIUS) return host_fail(c, SSM_E_INVAL, "render: max_radius must be 0..8");
    if (!(P.point_size >= 0.0 && finite_d(P.point_size))) return host_fail(c, SSM_E_INVAL, "render: point_size must be finite and not negative");
    if (!(P.z_min >= 0.0 && finite_d(P.z_min))) return host_fail(c, SSM_E_INVAL, "render: z_min must be finite and not negative");
    if (!(P.z_max >= 0.0 && finite_d(P.z_max))) return host_fail(c, SSM_E_INVAL, "render: z_max must be finite and not negative (1e9: no limit)");
    if (!(finite_d(cam->fx) && finite_d(cam->fy) && finite_d(cam->cx) && finite_d(cam->cy))) return host_fail(c, SSM_E_INVAL, "render: the camera must be finite");
    { const int r = render_tol_check(c, P, cam->scale); if (r) return r; }
    S->fx = cam->fx; S->fy = cam->fy; S->cx = cam->cx; S->cy = cam->cy; S->scale = cam->scale; S->z_min = P.z_min; S->z_max = P.z_max;
    S->point_size = P.point_size; S->half = (0.5 * cam->fx) * P.point_size;
    S->w = w; S->h = h; S->max_radius = P.max_radius; S->pad = 0;
    return SSM_OK;
}
int render_compare_check(ssm_ctx* c, const ssm_render_params& P, double scale, int64_t* tol_abs)
{
    const int r = render_tol_check(c, P, scale); if (r) return r;
    *tol_abs = ssm_carvec::tol_abs_units(P.tol_abs, scale);
    return SSM_OK;
}
CloudRule render_cloud_rule() { return {nullptr, 1, (int64_t)1 << 32, nullptr, "render: a negative point count", "render: 2^32 points or more in one call"}; }

extern "C" int ssm_render_host(int w, int h, const ssm_camera* cam, const double* T_view, const ssm_point* const* pts, const int32_t* n, const double* T_clouds, int m,
                               const ssm_render_params* params, uint16_t* depth, uint8_t* bgr, uint8_t* label, int32_t* index, uint64_t* keys, ssm_render_info* info)
{
    ssm_render_params P; ssm_render_params_default(&P); if (params) P = *params;
    Setup S;
    { int r = render_check(nullptr, w, h, cam, P, &S); if (!r) r = carve_pose_check(nullptr, T_view); if (r) return r; }
    if (m < 0 || (m && (!pts || !n || !T_clouds))) return host_fail(nullptr, SSM_E_INVAL, "null argument");
    int64_t total = 0;
    const CloudRule R = render_cloud_rule();
    { int r = cloud_total_check(nullptr, R, n, m, &total); if (!r) r = cloud_arrays_check(nullptr, R.twice_msg, pts, n, T_clouds, m); if (r) return r; }
    const size_t np = (size_t)w * h;
    std::vector<uint64_t> zb(np, KEY_EMPTY);
    std::vector<int64_t> first((size_t)m + 1, 0);
    ssm_render_info I{}; I.n_in = (int32_t)(uint32_t)total;
    for (int k = 0; k < m; k++) {
        double M[12]; ssm_carvec::rel_pose(T_view, T_clouds + 16 * k, M);
        first[k + 1] = first[k] + n[k];
        for (int i = 0; i < n[k]; i++) {
            Splat sp;
            if (!splat_of(pts[k][i].x, pts[k][i].y, pts[k][i].z, M, S, &sp)) continue;
            I.n_visible++;
            const uint64_t key = key_of(sp.zq, (uint32_t)(first[k] + i));
            for (int y = sp.y0; y <= sp.y1; y++) for (int x = sp.x0; x <= sp.x1; x++) { uint64_t& a = zb[(size_t)y * w + x]; if (key < a) a = key; }
        }
    }
    for (size_t p = 0; p < np; p++) {
        const uint64_t key = zb[p];
        uint16_t d = 0; uint8_t c3[3] = {0, 0, 0}, l = 255; int32_t ix = -1;
        if (key != KEY_EMPTY) {
            const uint32_t idx = (uint32_t)key;
            int k = 0; while ((int64_t)idx >= first[k + 1]) k++;
            const ssm_point& q = pts[k][(int64_t)idx - first[k]];
            d = (uint16_t)(key >> 32); c3[0] = q.b; c3[1] = q.g; c3[2] = q.r; l = (uint8_t)(q.label & 255u); ix = (int32_t)idx;
            I.n_covered++;
        }
        if (depth) depth[p] = d;
        if (bgr) { bgr[p * 3] = c3[0]; bgr[p * 3 + 1] = c3[1]; bgr[p * 3 + 2] = c3[2]; }
        if (label) label[p] = l;
        if (index) index[p] = ix;
    }
    if (keys) memcpy(keys, zb.data(), np * 8);
    if (info) *info = I;
    return SSM_OK;
}

extern "C" int ssm_render_compare_host(const uint16_t* rdepth, const uint8_t* rlabel, int w, int h, const uint16_t* depth, const uint8_t* sem_bgr, double cam_scale,
                                       const ssm_render_params* params, ssm_render_compare_info* info, uint8_t* class_img)
{
    ssm_render_params P; ssm_render_params_default(&P); if (params) P = *params;
    int64_t tol_abs = 0;
    { int r = render_size_check(nullptr, w, h); if (!r) r = render_compare_check(nullptr, P, cam_scale, &tol_abs); if (r) return r; }
    if (!rdepth || !rlabel || !depth || !sem_bgr) return host_fail(nullptr, SSM_E_INVAL, "null argument");
    ssm_render_compare_info I{};
    const size_t np = (size_t)w * h;
    I.n_pixels = (int64_t)np;
    for (size_t p = 0; p < np; p++) {
        const uint8_t lf = label_of_bgr24((uint32_t)sem_bgr[p * 3] | ((uint32_t)sem_bgr[p * 3 + 1] << 8) | ((uint32_t)sem_bgr[p * 3 + 2] << 16));
        int lab;
        const int cls = class_of(rdepth[p], depth[p], rlabel[p], lf, tol_abs, P.tol_rel_ppm, &lab);
        (cls == UNRENDERED ? I.unrendered : cls == NO_DEPTH ? I.no_depth : cls == IN_FRONT ? I.in_front : cls == BEHIND ? I.behind : I.agree)++;
        if (lab == LABEL_AGREE) I.label_agree++; else if (lab == LABEL_DISAGREE) I.label_disagree++; else if (lab == LABEL_UNKNOWN) I.label_unknown++;
        if (class_img) class_img[p] = (uint8_t)cls;
    }
    if (info) *info = I;
    return SSM_OK;
}

extern "C" void ssm_render_label_colours(const uint8_t* label, int64_t n, uint8_t* out)
{
    if (!label || !out) return;
    for (int64_t i = 0; i < n; i++) { const uint32_t c = bgr24_of_label(label[i]); out[i * 3] = (uint8_t)c; out[i * 3 + 1] = (uint8_t)(c >> 8); out[i * 3 + 2] = (uint8_t)(c >> 16); }
}
