// ssm_align_host.cpp -- dense alignment on the CPU: ssm_align_host, the parameter defaults, the argument checks and the iteration loop
// (align_drive) that the device entry points share: they differ only in who adds up one iteration's sums.  Plain C++ over include/ssm/align_core.h with one
// thread: a loop over the points where the device path has one thread per point and an integer reduction.
#include "ssm_host.h"
using namespace ssm_alignc;

extern "C" void ssm_align_params_default(ssm_align_params* p)
{
    if (!p) return;
    p->max_iterations = 10; p->stride = 1; p->z_min = 0.1; p->z_max = 80.0; p->dist_max = 0.25; p->delta = 0.05; p->damping = 1.0e-6; p->eps_rot = 1.0e-4;
    p->eps_trans = 1.0e-4; p->min_inliers = 1000; p->pad = 0; p->max_shift = 1.0; p->max_angle = 0.2; p->tol_abs = 0.05; p->tol_rel_ppm = 20000; p->pad2 = 0;
}
static bool nonneg(double v) { return v >= 0.0 && finite_d(v); }
int align_check(ssm_ctx* c, int w, int h, const ssm_camera* cam, const ssm_align_params& P, Setup* S)
{
    using namespace ssm_carvec;
    if (!cam) return host_fail(c, SSM_E_INVAL, "null argument");
    if (w < 3 || h < 3 || (int64_t)w * h > ssm_alignc::MAX_PIXELS) return host_fail(c, SSM_E_INVAL, "align: the view must be at least 3 x 3 and at most 2^26 pixels");
    if (P.max_iterations < 1 || P.max_iterations > MAX_ITERATIONS) return host_fail(c, SSM_E_INVAL, "align: max_iterations must be 1..64");
    if (P.stride < 1 || P.stride > MAX_STRIDE) return host_fail(c, SSM_E_INVAL, "align: stride must be 1..2^20");
    if (P.min_inliers < 0) return host_fail(c, SSM_E_INVAL, "align: min_inliers must not be negative");
    if (!(nonneg(P.z_min) && nonneg(P.z_max) && nonneg(P.dist_max) && nonneg(P.delta) && nonneg(P.damping) && nonneg(P.eps_rot) && nonneg(P.eps_trans) &&
          nonneg(P.max_shift) && nonneg(P.max_angle)))
        return host_fail(c, SSM_E_INVAL, "align: every parameter must be finite and not negative");
    if (P.z_max < P.z_min) return host_fail(c, SSM_E_INVAL, "align: z_max is below z_min");
    if (P.max_angle > 3.141592653589793) return host_fail(c, SSM_E_INVAL, "align: max_angle must be at most pi");
    if (!(P.tol_abs >= 0.0 && P.tol_abs <= TOL_ABS_MAX)) return host_fail(c, SSM_E_INVAL, "align: tol_abs must be finite, 0..1e6 m");
    if (P.tol_rel_ppm < 0 || P.tol_rel_ppm > PPM_MAX) return host_fail(c, SSM_E_INVAL, "align: tol_rel_ppm must be 0..1000000");
    if (!(finite_d(cam->fx) && finite_d(cam->fy) && finite_d(cam->cx) && finite_d(cam->cy) && cam->scale > 0.0 && cam->scale <= SCALE_MAX))
        return host_fail(c, SSM_E_INVAL, "align: the camera must be finite, its scale in (0, 1e6]");
    S->fx = cam->fx; S->fy = cam->fy; S->cx = cam->cx; S->cy = cam->cy; S->scale = cam->scale; S->z_min = P.z_min; S->z_max = P.z_max; S->dist_max = P.dist_max;
    S->delta = P.delta; S->w = w; S->h = h; S->tol_abs = tol_abs_units(P.tol_abs, cam->scale); S->ppm = P.tol_rel_ppm;
    return SSM_OK;
}
CloudRule align_cloud_rule(const Setup& S, int stride)
{
    return {"align: the same cloud twice", stride, 0, &S, "align: a negative point count",
            "align: the sums of this many points at this z_max, dist_max and field of view could reach 2^62"};
}

int align_drive(const ssm_align_params& P, int64_t n_in, const double* T_view, const std::function<int(const double*, int64_t*)>& accumulate, double* T_view_out,
                ssm_align_info* info, std::vector<ssm_align_iter>* record)
{
    using namespace ssm_pnp;
    ssm_align_info I{}; I.n_in = n_in; I.status = MAX_ITER;
    Pose E; for (int k = 0; k < 9; k++) E.R[k] = (k % 4 == 0) ? 1.0 : 0.0;
    E.t[0] = E.t[1] = E.t[2] = 0.0;
    double sn, cos_max; sincos64(P.max_angle, sn, cos_max);
    const double hb = 1.0 / (double)((int64_t)1 << S_HB), ch = 1.0 / (double)((int64_t)1 << S_CHI);
    if (record) record->clear();
    for (int it = 0; it < P.max_iterations; it++) {
        ssm_align_iter R{};
        for (int r = 0; r < 3; r++) { for (int k = 0; k < 3; k++) R.E[4 * r + k] = E.R[3 * r + k]; R.E[4 * r + 3] = E.t[r]; }
        { const int r = accumulate(R.E, R.sums); if (r) return r; }
        if (record) record->push_back(R);
        const int64_t tested = R.sums[I_TESTED], inl = R.sums[I_INLIER];
        const double chi2 = (double)R.sums[I_CHI] * ch;
        if (it == 0) { I.tested_first = tested; I.inliers_first = inl; I.chi2_first = chi2; }
        I.tested_last = tested; I.inliers_last = inl; I.chi2_last = chi2; I.iterations = it + 1;
        if (inl < (int64_t)P.min_inliers) { I.status = TOO_FEW; break; }
        double H[NH], b[NB], x[6] = {0, 0, 0, 0, 0, 0};
        for (int q = 0; q < NH; q++) H[q] = (double)R.sums[q] * hb;
        for (int q = 0; q < NB; q++) b[q] = (double)R.sums[I_B + q] * hb;
        if (!solve_ldlt(H, P.damping * (double)inl, b, x)) { I.status = DEGENERATE; break; }
        pose_oplus(E, x);
        bool fin = true; for (int k = 0; k < 9; k++) fin = fin && finite_d(E.R[k]);
        for (int k = 0; k < 3; k++) fin = fin && finite_d(E.t[k]);
        const double shift = sqrt((E.t[0] * E.t[0] + E.t[1] * E.t[1]) + E.t[2] * E.t[2]), cs = (((E.R[0] + E.R[4]) + E.R[8]) - 1.0) * 0.5;
        if (!fin || shift > P.max_shift || cs < cos_max) { I.status = DIVERGED; break; }
        const double rot = sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]), tr = sqrt((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]);
        if (rot < P.eps_rot && tr < P.eps_trans) { I.status = CONVERGED; break; }
    }
    if (I.status != MAX_ITER && I.status != CONVERGED) { for (int k = 0; k < 9; k++) E.R[k] = (k % 4 == 0) ? 1.0 : 0.0; E.t[0] = E.t[1] = E.t[2] = 0.0; }
    pose_to_iso(E, I.E);
    if (T_view_out) {
        if (I.status != MAX_ITER && I.status != CONVERGED) memcpy(T_view_out, T_view, 16 * sizeof(double));
        else { double Ei[16]; iso_inverse(I.E, Ei); iso_mul(T_view, Ei, T_view_out); }
    }
    if (info) *info = I;
    return SSM_OK;
}

extern "C" int ssm_align_host(const uint16_t* depth, int w, int h, const ssm_camera* cam, const double* T_view, const ssm_point* const* pts, const int32_t* n,
                              const double* T_clouds, int m, const ssm_align_params* params, double* T_view_out, ssm_align_info* info, uint8_t* valid, float* normals,
                              ssm_align_iter* record, int record_cap, int* n_record)
{
    ssm_align_params P; ssm_align_params_default(&P); if (params) P = *params;
    Setup S;
    { int r = align_check(nullptr, w, h, cam, P, &S); if (!r) r = carve_pose_check(nullptr, T_view); if (r) return r; }
    if (!depth || m < 0 || (m && (!pts || !n || !T_clouds)) || record_cap < 0) return host_fail(nullptr, SSM_E_INVAL, "null argument");
    int64_t total = 0;
    const CloudRule R = align_cloud_rule(S, P.stride);
    { int r = cloud_total_check(nullptr, R, n, m, &total); if (!r) r = cloud_arrays_check(nullptr, R.twice_msg, pts, n, T_clouds, m); if (r) return r; }
    std::vector<double> M((size_t)m * 12);
    for (int k = 0; k < m; k++) ssm_carvec::rel_pose(T_view, T_clouds + 16 * k, M.data() + 12 * (size_t)k);
    std::vector<Normal> nm((size_t)w * h);
    for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) {
        const size_t at = (size_t)y * w + x;
        const bool ok = normal_of(depth, x, y, S, &nm[at]);
        if (valid) valid[at] = ok ? 1 : 0;
    }
    if (normals) memcpy(normals, nm.data(), nm.size() * sizeof(Normal));
    std::vector<ssm_align_iter> rec;
    const int r = align_drive(P, total, T_view, [&](const double* E, int64_t* sums) {
        for (int q = 0; q < NSUM; q++) sums[q] = 0;
        for (int k = 0; k < m; k++)
            for (int64_t i = 0; i < n[k]; i += P.stride) point_terms(pts[k][i].x, pts[k][i].y, pts[k][i].z, M.data() + 12 * (size_t)k, E, depth, nm.data(), S, sums);
        return (int)SSM_OK;
    }, T_view_out, info, &rec);
    if (r) return r;
    if (n_record) *n_record = (int)rec.size();
    if (record) {
        if ((int)rec.size() > record_cap) return host_fail(nullptr, SSM_E_CAPACITY, "record buffer too small (need " + std::to_string(rec.size()) + ")");
        if (!rec.empty()) memcpy(record, rec.data(), rec.size() * sizeof(ssm_align_iter));
    }
    return SSM_OK;
}
