// ssm_relabel_host.cpp -- label fusion on the CPU: ssm_relabel_host, ssm_relabel_labels_host, the parameter defaults and the argument checks the
// device entry points share.  Plain C++ over include/ssm/relabel_core.h with one thread: a loop over the points where the device path has one thread per point.
#include "ssm_host.h"
using namespace ssm_relabelc;

extern "C" void ssm_relabel_params_default(ssm_relabel_params* p)
{
    if (!p) return;
    p->radius = 1; p->edge_guard = 1; p->own_weight = 1; p->min_votes = 2; p->tol_abs = 0.05; p->tol_rel_ppm = 20000; p->pad = 0; p->z_min = 0.1;
}
int relabel_check(ssm_ctx* c, int v, const ssm_relabel_params& P)
{
    if (v < 0 || v > MAX_VIEWS) return host_fail(c, SSM_E_INVAL, "relabel: 0..16 views per call");
    if (P.radius < 0 || P.radius > ssm_carvec::MAX_RADIUS) return host_fail(c, SSM_E_INVAL, "relabel: radius must be 0..3");
    if (P.edge_guard < 0 || P.edge_guard > 1) return host_fail(c, SSM_E_INVAL, "relabel: edge_guard must be 0 or 1");
    if (P.own_weight < 0 || P.own_weight > MAX_OWN_WEIGHT) return host_fail(c, SSM_E_INVAL, "relabel: own_weight must be 0..15");
    if (P.min_votes < 1 || P.min_votes > MAX_MIN_VOTES) return host_fail(c, SSM_E_INVAL, "relabel: min_votes must be 1..31");
    if (!(P.tol_abs >= 0.0 && P.tol_abs <= ssm_carvec::TOL_ABS_MAX)) return host_fail(c, SSM_E_INVAL, "relabel: tol_abs must be finite, 0..1e6 m");
    if (P.tol_rel_ppm < 0 || P.tol_rel_ppm > ssm_carvec::PPM_MAX) return host_fail(c, SSM_E_INVAL, "relabel: tol_rel_ppm must be 0..1000000");
    if (!(P.z_min >= 0.0 && ssm_carvec::finite_d(P.z_min))) return host_fail(c, SSM_E_INVAL, "relabel: z_min must be finite and not negative");
    return SSM_OK;
}
int relabel_view_fill(ssm_ctx* c, int w, int h, const ssm_camera* cam, const double* T_view, const double* T_cloud, const ssm_relabel_params& P, View* V)
{
    ssm_carve_params CP; CP.min_votes = 1; CP.radius = P.radius; CP.tol_abs = P.tol_abs; CP.tol_rel_ppm = P.tol_rel_ppm; CP.pad = 0; CP.z_min = P.z_min;
    { int r = carve_check(c, w, h, cam, CP, &V->S); if (!r) r = carve_pose_check(c, T_view); if (r) return r; }
    ssm_carvec::rel_pose(T_view, T_cloud, V->M);
    return SSM_OK;
}
static void relabel_point(const View* views, int v, const ssm_relabel_params& P, const ssm_point& p, uint64_t* votes, uint32_t* label, ssm_relabel_info* I)
{
    const uint32_t L0 = p.label;
    uint64_t c = own_vote(L0, P.own_weight);
    int ns = 0, nv = 0;
    for (int k = 0; k < v; k++) { int s, t; c = view_vote(c, p.x, p.y, p.z, views[k], P.edge_guard, &s, &t); ns += s; nv += t; }
    const uint32_t L1 = decide(L0, c, P.min_votes);
    *votes = c; *label = L1;
    I->n_supported += ns > 0; I->n_voted += nv > 0; I->pairs_supported += ns; I->pairs_voted += nv;
    if (L1 != L0) { I->n_changed++; I->n_filled += L0 >= (uint32_t)N_LABELS; }
}

extern "C" int ssm_relabel_host(const ssm_relabel_host_view* views, const double* T_views, int v, const ssm_point* pts, int n, const double* T_cloud,
                                const ssm_relabel_params* params, uint32_t* label_out, uint64_t* votes_out, ssm_relabel_info* info)
{
    ssm_relabel_params P; ssm_relabel_params_default(&P); if (params) P = *params;
    { const int r = relabel_check(nullptr, v, P); if (r) return r; }
    if (n < 0 || (n && (!pts || !label_out)) || (v && (!views || !T_views))) return host_fail(nullptr, SSM_E_INVAL, "null argument");
    { const int r = carve_pose_check(nullptr, T_cloud); if (r) return r; }
    std::vector<View> V((size_t)v);
    for (int k = 0; k < v; k++) {
        if (!views[k].depth || !views[k].label) return host_fail(nullptr, SSM_E_INVAL, "relabel: a null view");
        const int r = relabel_view_fill(nullptr, views[k].w, views[k].h, &views[k].cam, T_views + 16 * k, T_cloud, P, &V[k]); if (r) return r;
        V[k].depth = views[k].depth; V[k].label = views[k].label;
    }
    ssm_relabel_info I{}; I.n_in = n;
    for (int i = 0; i < n; i++) { uint64_t c; relabel_point(V.data(), v, P, pts[i], &c, &label_out[i], &I); if (votes_out) votes_out[i] = c; }
    if (info) *info = I;
    return SSM_OK;
}
extern "C" int ssm_relabel_labels_host(const uint8_t* sem_bgr, int64_t n, uint8_t* label_out)
{
    if (n < 0 || (n && (!sem_bgr || !label_out))) return host_fail(nullptr, SSM_E_INVAL, "null argument");
    for (int64_t i = 0; i < n; i++) label_out[i] = ssm_renderc::label_of_bgr24((uint32_t)sem_bgr[3 * i] | (uint32_t)sem_bgr[3 * i + 1] << 8 | (uint32_t)sem_bgr[3 * i + 2] << 16);
    return SSM_OK;
}
