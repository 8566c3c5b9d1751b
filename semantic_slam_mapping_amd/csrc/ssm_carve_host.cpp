// ssm_carve_host.cpp -- free-space carving on the CPU: ssm_carve_host, the parameter defaults and the argument check the device entry points
// share.  Plain C++ over include/ssm/carve_core.h with one thread: a loop over the points where the device path has one thread per point and a block scan.
#include "ssm_host.h"
using namespace ssm_carvec;

extern "C" void ssm_carve_params_default(ssm_carve_params* p)
{
    if (!p) return;
    p->min_votes = 2; p->radius = 1; p->tol_abs = 0.05; p->tol_rel_ppm = 20000; p->pad = 0; p->z_min = 0.1;
}
int carve_check(ssm_ctx* c, int w, int h, const ssm_camera* cam, const ssm_carve_params& P, Setup* S)
{
    if (!cam || w < 1 || h < 1 || (int64_t)w * h > ((int64_t)1 << 28)) return host_fail(c, SSM_E_INVAL, "carve: bad view size or null camera");
    if (P.min_votes < 1 || P.min_votes > MAX_RUN) return host_fail(c, SSM_E_INVAL, "carve: min_votes must be 1..255");
    if (P.radius < 0 || P.radius > MAX_RADIUS) return host_fail(c, SSM_E_INVAL, "carve: radius must be 0..3");
    if (!(P.tol_abs >= 0.0 && P.tol_abs <= TOL_ABS_MAX)) return host_fail(c, SSM_E_INVAL, "carve: tol_abs must be finite, 0..1e6 m");
    if (P.tol_rel_ppm < 0 || P.tol_rel_ppm > PPM_MAX) return host_fail(c, SSM_E_INVAL, "carve: tol_rel_ppm must be 0..1000000");
    if (!(P.z_min >= 0.0 && finite_d(P.z_min))) return host_fail(c, SSM_E_INVAL, "carve: z_min must be finite and not negative");
    if (!(finite_d(cam->fx) && finite_d(cam->fy) && finite_d(cam->cx) && finite_d(cam->cy) && cam->scale > 0.0 && cam->scale <= SCALE_MAX))
        return host_fail(c, SSM_E_INVAL, "carve: the camera must be finite, its scale in (0, 1e6]");
    S->fx = cam->fx; S->fy = cam->fy; S->cx = cam->cx; S->cy = cam->cy; S->scale = cam->scale; S->z_min = P.z_min;
    S->w = w; S->h = h; S->r = P.radius; S->tol_abs = tol_abs_units(P.tol_abs, cam->scale); S->ppm = P.tol_rel_ppm;
    return SSM_OK;
}
int carve_pose_check(ssm_ctx* c, const double* T)
{
    if (!T) return host_fail(c, SSM_E_INVAL, "null argument");
    for (int i = 0; i < 16; i++) if (!finite_d(T[i])) return host_fail(c, SSM_E_INVAL, "carve: a pose is not finite");
    return SSM_OK;
}
int cloud_arrays_check(ssm_ctx* c, const char* twice_msg, const ssm_point* const* pts, const int32_t* n, const double* T_clouds, int m)
{
    for (int k = 0; k < m; k++) {
        if (n[k] && !pts[k]) return host_fail(c, SSM_E_INVAL, "null argument");
        if (twice_msg) for (int j = 0; j < k; j++) if (n[k] && n[j] && pts[j] == pts[k]) return host_fail(c, SSM_E_INVAL, twice_msg);
        const int r = carve_pose_check(c, T_clouds + 16 * k); if (r) return r;
    }
    return SSM_OK;
}

extern "C" int ssm_carve_host(const uint16_t* depth, int w, int h, const ssm_camera* cam, const double* T_view, const ssm_point* pts, int n, const double* T_cloud,
                              uint8_t* run_inout, const ssm_carve_params* params, ssm_point* out, int cap, int* n_out, ssm_carve_info* info, uint8_t* verdict, uint8_t* run)
{
    ssm_carve_params P; ssm_carve_params_default(&P); if (params) P = *params;
    Setup S;
    { const int r = carve_check(nullptr, w, h, cam, P, &S); if (r) return r; }
    if (!depth || !n_out || n < 0 || (n && !pts) || cap < 0) return host_fail(nullptr, SSM_E_INVAL, "null argument");
    { int r = carve_pose_check(nullptr, T_view); if (!r) r = carve_pose_check(nullptr, T_cloud); if (r) return r; }
    double M[12]; rel_pose(T_view, T_cloud, M);
    ssm_carve_info I{}; I.n_in = n;
    std::vector<uint8_t> vd((size_t)n, 0), rn((size_t)n, 0);
    for (int i = 0; i < n; i++) {
        const int v = verdict_of(pts[i].x, pts[i].y, pts[i].z, M, depth, S);
        vd[i] = (uint8_t)v; rn[i] = run_after(run_inout ? run_inout[i] : (uint8_t)0, v);
        (v == UNKNOWN ? I.unknown : v == OCCLUDED ? I.occluded : v == SUPPORTED ? I.supported : I.seen_through)++;
        if (!leaves(rn[i], P.min_votes)) I.n_kept++;
    }
    I.removed = n - I.n_kept;
    *n_out = I.n_kept;
    if (info) *info = I;
    if (verdict && n) memcpy(verdict, vd.data(), (size_t)n);
    if (run && n) memcpy(run, rn.data(), (size_t)n);
    if (I.n_kept > cap) return host_fail(nullptr, SSM_E_CAPACITY, "point buffer too small (need " + std::to_string(I.n_kept) + ")");
    if (I.n_kept && !out) return host_fail(nullptr, SSM_E_INVAL, "null argument");
    for (int i = 0, o = 0; i < n; i++) if (!leaves(rn[i], P.min_votes)) { out[o] = pts[i]; if (run_inout) run_inout[o] = rn[i]; o++; }
    return SSM_OK;
}
