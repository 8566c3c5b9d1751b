// ssm_grid_host.cpp -- the ground grid on the CPU: ssm_grid_host, the colour and height images, the frame helper, the parameter defaults and the
// argument checks the device entry points share.  Plain C++ over include/ssm/grid_core.h with one thread: loops over the points and the cells where the device path
// has one thread per point with integer atomics and one thread per cell.
#include "ssm_host.h"
using namespace ssm_gridc;

extern "C" void ssm_grid_params_default(ssm_grid_params* p)
{
    if (!p) return;
    static const double G[12] = {1, 0, 0, 0, 0, 0, 1, 0, 0, -1, 0, 0};
    memcpy(p->G, G, sizeof(G));
    p->cell = 0.2; p->nx = 512; p->ny = 512; p->x0 = -51.2; p->y0 = -10.0; p->h_min = -3.0; p->h_max = 3.0; p->step = 0.3; p->ground_radius = 1; p->min_obstacle_points = 3;
}
extern "C" int ssm_grid_frame_from_up(const double up[3], const double forward[3], double G[12])
{
    if (!up || !forward || !G) return host_fail(nullptr, SSM_E_INVAL, "null argument");
    if (!frame_from_up(up, forward, G)) return host_fail(nullptr, SSM_E_INVAL, "grid: up and forward must be finite, up not of length 0, forward not along up");
    return SSM_OK;
}
int grid_check(ssm_ctx* c, const ssm_grid_params& P, Setup* S)
{
    using ssm_carvec::finite_d;
    for (int i = 0; i < 12; i++) if (!finite_d(P.G[i])) return host_fail(c, SSM_E_INVAL, "grid: G must be finite");
    if (!(finite_d(P.x0) && finite_d(P.y0))) return host_fail(c, SSM_E_INVAL, "grid: x0 and y0 must be finite");
    if (!(P.cell > 0.0 && finite_d(P.cell))) return host_fail(c, SSM_E_INVAL, "grid: cell must be finite and positive");
    if (P.nx < 1 || P.ny < 1 || (int64_t)P.nx * P.ny > MAX_CELLS) return host_fail(c, SSM_E_INVAL, "grid: at least 1 x 1 and at most 2^24 cells");
    if (!(finite_d(P.h_min) && finite_d(P.h_max) && P.h_min <= P.h_max && fabs(P.h_min) <= H_LIMIT && fabs(P.h_max) <= H_LIMIT))
        return host_fail(c, SSM_E_INVAL, "grid: h_min <= h_max, both finite and within 2^20 m");
    if (!(P.step >= 0.0 && finite_d(P.step))) return host_fail(c, SSM_E_INVAL, "grid: step must be finite and not negative");
    if (P.ground_radius < 0 || P.ground_radius > MAX_GROUND_RADIUS) return host_fail(c, SSM_E_INVAL, "grid: ground_radius must be 0..4");
    if (P.min_obstacle_points < 1) return host_fail(c, SSM_E_INVAL, "grid: min_obstacle_points must be at least 1");
    S->x0 = P.x0; S->y0 = P.y0; S->cell = P.cell; S->h_min = P.h_min; S->h_max = P.h_max; S->step_q = step_units(P.step);
    S->nx = P.nx; S->ny = P.ny; S->ground_radius = P.ground_radius; S->min_obstacle_points = P.min_obstacle_points;
    return SSM_OK;
}
CloudRule grid_cloud_rule() { return {"grid: the same cloud twice", 1, MAX_POINTS, nullptr, "grid: a negative point count", "grid: 2^31 points or more in one call"}; }

// the base of cell (cx, cy) with n > 0: the smallest hmin over the non-empty cells of its window, clipped at the grid's edge
static int32_t base_of(const ssm_grid_cell* cells, const Setup& S, int cx, int cy)
{
    int32_t b = BASE_EMPTY;
    for (int y = std::max(cy - S.ground_radius, 0); y <= std::min(cy + S.ground_radius, S.ny - 1); y++)
        for (int x = std::max(cx - S.ground_radius, 0); x <= std::min(cx + S.ground_radius, S.nx - 1); x++) {
            const ssm_grid_cell& o = cells[(size_t)y * S.nx + x];
            if (o.n && o.hmin < b) b = o.hmin;
        }
    return b;
}

extern "C" int ssm_grid_host(const ssm_point* const* pts, const int32_t* n, const double* T_clouds, int m, const ssm_grid_params* params, uint8_t* cls, uint8_t* ground_label,
                             uint8_t* obstacle_label, int32_t* ground_q, int32_t* top_q, uint32_t* n_out, uint32_t* n_high, ssm_grid_cell* cells_out, ssm_grid_info* info)
{
    ssm_grid_params P; ssm_grid_params_default(&P); if (params) P = *params;
    Setup S;
    { const int r = grid_check(nullptr, P, &S); if (r) return r; }
    if (m < 0 || (m && (!pts || !n || !T_clouds))) return host_fail(nullptr, SSM_E_INVAL, "null argument");
    int64_t total = 0;
    const CloudRule R = grid_cloud_rule();
    { int r = cloud_total_check(nullptr, R, n, m, &total); if (!r) r = cloud_arrays_check(nullptr, R.twice_msg, pts, n, T_clouds, m); if (r) return r; }
    const size_t nc = (size_t)S.nx * S.ny;
    ssm_grid_cell empty; memset(&empty, 0, sizeof(empty)); empty.hmin = HMIN_EMPTY; empty.hmax = HMAX_EMPTY; empty.base = BASE_EMPTY;
    std::vector<ssm_grid_cell> cells(nc, empty);
    ssm_grid_info I{}; I.n_in = total;
    std::vector<double> M((size_t)m * 12 + 1);
    for (int k = 0; k < m; k++) grid_pose(P.G, T_clouds + 16 * k, M.data() + 12 * k);
    for (int k = 0; k < m; k++) for (int i = 0; i < n[k]; i++) {                 // pass A
        Hit h;
        const int st = point_of(pts[k][i].x, pts[k][i].y, pts[k][i].z, M.data() + 12 * k, S, &h);
        if (st == P_REJECTED) continue;
        I.n_finite++;
        if (st == P_OUT_OF_BAND) { I.out_of_band++; continue; }
        if (st == P_OUTSIDE) { I.outside++; continue; }
        I.n_used++;
        ssm_grid_cell& c = cells[(size_t)h.cy * S.nx + h.cx];
        c.n++; if (h.hq < c.hmin) c.hmin = h.hq; if (h.hq > c.hmax) c.hmax = h.hq;
    }
    for (int cy = 0; cy < S.ny; cy++) for (int cx = 0; cx < S.nx; cx++) {       // ground
        ssm_grid_cell& c = cells[(size_t)cy * S.nx + cx];
        if (c.n) c.base = base_of(cells.data(), S, cx, cy);
    }
    for (int k = 0; k < m; k++) for (int i = 0; i < n[k]; i++) {                 // pass B
        Hit h;
        if (point_of(pts[k][i].x, pts[k][i].y, pts[k][i].z, M.data() + 12 * k, S, &h) != P_USED) continue;
        ssm_grid_cell& c = cells[(size_t)h.cy * S.nx + h.cx];
        const uint32_t l = pts[k][i].label;
        if (is_low(h.hq, c.base, S.step_q)) { c.n_low++; c.sum_low += h.hq; if (l < (uint32_t)NLABEL) c.hist_low[l]++; }
        else { c.n_high++; if (l < (uint32_t)NLABEL) c.hist_high[l]++; }
    }
    int64_t* by_class = &I.unobserved;
    for (size_t i = 0; i < nc; i++) {                                             // resolve
        const Resolved r = resolve_of(cells[i], S.min_obstacle_points);
        by_class[r.cls]++;
        if (cls) cls[i] = r.cls;
        if (ground_label) ground_label[i] = r.ground_label;
        if (obstacle_label) obstacle_label[i] = r.obstacle_label;
        if (ground_q) ground_q[i] = r.ground_q;
        if (top_q) top_q[i] = r.top_q;
        if (n_out) n_out[i] = cells[i].n;
        if (n_high) n_high[i] = cells[i].n_high;
    }
    if (cells_out) memcpy(cells_out, cells.data(), nc * sizeof(ssm_grid_cell));
    if (info) *info = I;
    return SSM_OK;
}

extern "C" void ssm_grid_colours(const uint8_t* cls, const uint8_t* ground_label, const uint8_t* obstacle_label, const int32_t* ground_q, int nx, int ny, double h_min,
                                 uint8_t* bgr, uint16_t* height)
{
    if (!cls || nx < 1 || ny < 1) return;
    const int64_t h0 = fabs(h_min) <= H_LIMIT ? (int64_t)llrint(h_min * H_UNIT) : 0;
    for (int r = 0; r < ny; r++) for (int x = 0; x < nx; x++) {
        const size_t i = (size_t)(ny - 1 - r) * nx + x, o = (size_t)r * nx + x;
        if (bgr) {
            uint32_t c = 0;
            if (cls[i] == OBSTACLE) { const uint8_t l = obstacle_label ? obstacle_label[i] : (uint8_t)LABEL_NONE; c = l < NLABEL ? ssm_renderc::bgr24_of_label(l) : 0xFFFFFFu; }
            else if (cls[i] != UNOBSERVED) { const uint8_t l = ground_label ? ground_label[i] : (uint8_t)LABEL_NONE; c = l < NLABEL ? ssm_renderc::bgr24_of_label(l) : 0x404040u; }
            bgr[o * 3] = (uint8_t)c; bgr[o * 3 + 1] = (uint8_t)(c >> 8); bgr[o * 3 + 2] = (uint8_t)(c >> 16);
        }
        if (height) {
            uint16_t v = 0;
            if (cls[i] != UNOBSERVED && ground_q) { const int64_t d = (int64_t)ground_q[i] - h0; v = (uint16_t)((d < 0 ? 0 : d > 65534 ? 65534 : d) + 1); }
            height[o] = v;
        }
    }
}
