// ssm_objects_host.cpp -- object extraction on the CPU: ssm_objects_cells_host (stage 1 from cell arrays), ssm_objects_host (the grid, then both
// stages), the parameter defaults and the argument checks the device entry points share.  Plain C++ over include/ssm/objects_core.h with one thread: a flood fill
// from every member cell not yet reached, in ascending cell order, where the device path has a union-find per tile; loops over the points where it has one thread
// per point with integer atomics.
#include "ssm_host.h"
using namespace ssm_objc;

static_assert(sizeof(ssm_object) == 104, "a record is 104 bytes");
static_assert(sizeof(ssm_objects_info) == 64, "info is eight 64-bit counts");

extern "C" void ssm_objects_params_default(ssm_objects_params* p)
{
    if (!p) return;
    p->label_mask = (1u << 9) | (1u << 10) | (1u << 11); p->connectivity = 8; p->min_cells = 2; p->min_points = 20; p->min_height = 0.3;
}
int objects_check(ssm_ctx* c, const ssm_objects_params& P, Setup* S)
{
    if (P.connectivity != 4 && P.connectivity != 8) return host_fail(c, SSM_E_INVAL, "objects: connectivity must be 4 or 8");
    if (P.min_cells < 0 || P.min_points < 0) return host_fail(c, SSM_E_INVAL, "objects: min_cells and min_points must not be negative");
    if (!(P.min_height >= 0.0 && ssm_carvec::finite_d(P.min_height))) return host_fail(c, SSM_E_INVAL, "objects: min_height must be finite and not negative");
    S->label_mask = P.label_mask; S->connectivity = P.connectivity; S->min_cells = P.min_cells; S->min_points = P.min_points; S->min_height_q = height_units(P.min_height);
    return SSM_OK;
}
int objects_extent_check(ssm_ctx* c, double x0, double y0, double cell, int nx, int ny)
{
    if (!extent_fits(x0, y0, cell, nx, ny)) return host_fail(c, SSM_E_INVAL, "objects: the grid's extent must stay within 2^20 m of the origin");
    return SSM_OK;
}
CloudRule objects_cloud_rule()
{ return {"objects: the same cloud twice", 1, ssm_gridc::MAX_POINTS, nullptr, "objects: a negative point count", "objects: 2^31 points or more in one call"}; }

// stage 1 -> every component's record in ascending root order, the component of every cell (-1: not a member)
static void components_of(const uint8_t* cls, const uint8_t* ol, const int32_t* gq, const int32_t* tq, const uint32_t* nh, int nx, int ny, const Setup& S,
                          std::vector<ssm_object>& comp, std::vector<int32_t>& comp_of, int64_t* member_cells)
{
    const size_t nc = (size_t)nx * ny;
    comp_of.assign(nc, -1); comp.clear(); *member_cells = 0;
    std::vector<int32_t> stack;
    static const int DX[8] = {-1, 1, 0, 0, -1, 1, -1, 1}, DY[8] = {0, 0, -1, 1, -1, -1, 1, 1};          // the first four: the 4-neighbourhood
    for (size_t i = 0; i < nc; i++) {
        if (!member(cls[i], ol[i], S.label_mask)) continue;
        ++*member_cells;
        if (comp_of[i] >= 0) continue;
        ssm_object o; memset(&o, 0, sizeof(o)); clear_cells(&o); clear_points(&o);
        o.root = (int32_t)i; o.label = ol[i];
        const int32_t k = (int32_t)comp.size();
        comp_of[i] = k; stack.assign(1, (int32_t)i);
        while (!stack.empty()) {
            const int32_t a = stack.back(); stack.pop_back();
            const int cx = a % nx, cy = a / nx;
            o.cells++; o.cell_points += nh[a];
            o.cx_min = std::min(o.cx_min, cx); o.cx_max = std::max(o.cx_max, cx); o.cy_min = std::min(o.cy_min, cy); o.cy_max = std::max(o.cy_max, cy);
            o.ground_q = std::min(o.ground_q, gq[a]); o.top_q = std::max(o.top_q, tq[a]);
            for (int d = 0; d < S.connectivity; d++) {
                const int x = cx + DX[d], y = cy + DY[d];
                if (x < 0 || y < 0 || x >= nx || y >= ny) continue;
                const size_t b = (size_t)y * nx + x;
                if (comp_of[b] >= 0 || !member(cls[b], ol[b], S.label_mask) || ol[b] != ol[i]) continue;
                comp_of[b] = k; stack.push_back((int32_t)b);
            }
        }
        comp.push_back(o);
    }
}
// the keep decision -> the kept records in ascending root order, the object of every component (-1: rejected), the info's stage-1 counts
static void keep_of(const std::vector<ssm_object>& comp, const Setup& S, int64_t member_cells, std::vector<ssm_object>& objs, std::vector<int32_t>& id_of, ssm_objects_info* I)
{
    memset(I, 0, sizeof(*I));
    I->member_cells = member_cells; I->components = (int64_t)comp.size();
    id_of.assign(comp.size(), -1); objs.clear();
    for (size_t k = 0; k < comp.size(); k++) {
        const int v = verdict_of(comp[k].cells, comp[k].cell_points, comp[k].ground_q, comp[k].top_q, S);
        if (v == REJECT_CELLS) I->rejected_cells++; else if (v == REJECT_POINTS) I->rejected_points++; else if (v == REJECT_HEIGHT) I->rejected_height++;
        else { id_of[k] = (int32_t)objs.size(); objs.push_back(comp[k]); }
    }
    I->kept = (int64_t)objs.size();
}
static int cells_run(const uint8_t* cls, const uint8_t* ol, const int32_t* gq, const int32_t* tq, const uint32_t* nh, int nx, int ny, const Setup& S,
                     std::vector<ssm_object>& objs, std::vector<int32_t>& object_id, ssm_objects_info* I)
{
    std::vector<ssm_object> comp; std::vector<int32_t> comp_of, id_of; int64_t members = 0;
    components_of(cls, ol, gq, tq, nh, nx, ny, S, comp, comp_of, &members);
    keep_of(comp, S, members, objs, id_of, I);
    object_id.resize(comp_of.size());
    for (size_t i = 0; i < comp_of.size(); i++) object_id[i] = comp_of[i] >= 0 ? id_of[(size_t)comp_of[i]] : -1;
    return SSM_OK;
}
static int cells_args(const ssm_objects_params* params, int nx, int ny, Setup* S)
{
    ssm_objects_params P; ssm_objects_params_default(&P); if (params) P = *params;
    { const int r = objects_check(nullptr, P, S); if (r) return r; }
    if (nx < 1 || ny < 1 || (int64_t)nx * ny > ssm_gridc::MAX_CELLS) return host_fail(nullptr, SSM_E_INVAL, "objects: at least 1 x 1 and at most 2^24 cells");
    return SSM_OK;
}

extern "C" int ssm_objects_cells_host(const uint8_t* cls, const uint8_t* obstacle_label, const int32_t* ground_q, const int32_t* top_q, const uint32_t* n_high, int nx, int ny,
                                      const ssm_objects_params* params, ssm_object* out, int cap, int* n_out, int32_t* object_id, ssm_objects_info* info)
{
    Setup S;
    { const int r = cells_args(params, nx, ny, &S); if (r) return r; }
    if (!cls || !obstacle_label || !ground_q || !top_q || !n_high || !n_out || cap < 0 || (cap && !out)) return host_fail(nullptr, SSM_E_INVAL, "null argument");
    std::vector<ssm_object> objs; std::vector<int32_t> ids; ssm_objects_info I;
    cells_run(cls, obstacle_label, ground_q, top_q, n_high, nx, ny, S, objs, ids, &I);
    *n_out = (int)objs.size();
    if ((int)objs.size() > cap) return host_fail(nullptr, SSM_E_CAPACITY, "record buffer too small (need " + std::to_string(objs.size()) + ")");
    if (!objs.empty()) memcpy(out, objs.data(), objs.size() * sizeof(ssm_object));
    if (object_id) memcpy(object_id, ids.data(), ids.size() * 4);
    if (info) *info = I;
    return SSM_OK;
}

extern "C" int ssm_objects_host(const ssm_point* const* pts, const int32_t* n, const double* T_clouds, int m, const ssm_grid_params* grid_params, const ssm_objects_params* params,
                                ssm_object* out, int cap, int* n_out, int32_t* object_id, int32_t* ids_out, ssm_objects_info* info)
{
    ssm_grid_params G; ssm_grid_params_default(&G); if (grid_params) G = *grid_params;
    ssm_gridc::Setup GS; Setup S;
    { const int r = grid_check(nullptr, G, &GS); if (r) return r; }
    { const int r = cells_args(params, G.nx, G.ny, &S); if (r) return r; }
    { const int r = objects_extent_check(nullptr, G.x0, G.y0, G.cell, G.nx, G.ny); if (r) return r; }
    if (!n_out || cap < 0 || (cap && !out)) return host_fail(nullptr, SSM_E_INVAL, "null argument");
    const size_t nc = (size_t)G.nx * G.ny;
    std::vector<uint8_t> cls(nc), ol(nc); std::vector<int32_t> gq(nc), tq(nc); std::vector<uint32_t> nh(nc); std::vector<ssm_grid_cell> cells(nc);
    ssm_grid_info GI;
    { const int r = ssm_grid_host(pts, n, T_clouds, m, &G, cls.data(), nullptr, ol.data(), gq.data(), tq.data(), nullptr, nh.data(), cells.data(), &GI); if (r) return r; }
    std::vector<ssm_object> objs; std::vector<int32_t> ids; ssm_objects_info I;
    cells_run(cls.data(), ol.data(), gq.data(), tq.data(), nh.data(), G.nx, G.ny, S, objs, ids, &I);
    *n_out = (int)objs.size();
    if ((int)objs.size() > cap) return host_fail(nullptr, SSM_E_CAPACITY, "record buffer too small (need " + std::to_string(objs.size()) + ")");
    I.n_in = GI.n_in;
    size_t at = 0;
    for (int k = 0; k < m; k++) {                                                  // stage 2
        double M[12]; ssm_gridc::grid_pose(G.G, T_clouds + 16 * k, M);
        for (int i = 0; i < n[k]; i++, at++) {
            const ssm_point& p = pts[k][i];
            Hit h; int32_t id = -1;
            if (point_of(p.x, p.y, p.z, M, GS, &h) == ssm_gridc::P_USED && !ssm_gridc::is_low(h.hq, cells[(size_t)h.cell].base, GS.step_q)) id = ids[(size_t)h.cell];
            if (ids_out) ids_out[at] = id;
            if (id < 0) continue;
            ssm_object& o = objs[(size_t)id];
            I.object_points++;
            o.n_points++; if (p.label == (uint32_t)o.label) o.n_label++;
            o.x_min_q = std::min(o.x_min_q, h.xq); o.x_max_q = std::max(o.x_max_q, h.xq); o.y_min_q = std::min(o.y_min_q, h.yq); o.y_max_q = std::max(o.y_max_q, h.yq);
            o.z_min_q = std::min(o.z_min_q, h.zq); o.z_max_q = std::max(o.z_max_q, h.zq);
            o.sum_x += h.xq; o.sum_y += h.yq; o.sum_z += h.zq;
        }
    }
    if (!objs.empty()) memcpy(out, objs.data(), objs.size() * sizeof(ssm_object));
    if (object_id) memcpy(object_id, ids.data(), nc * 4);
    if (info) *info = I;
    return SSM_OK;
}
