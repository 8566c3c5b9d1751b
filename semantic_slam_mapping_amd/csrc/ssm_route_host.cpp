// ssm_route_host.cpp -- the route field on the CPU: ssm_route_cells_host, ssm_route_path_host, the parameter defaults and the argument checks the
// device entry points share.  Plain C++ over include/ssm/route_core.h with one thread and an algorithm of its own: Dijkstra with a circular bucket queue (an edge
// costs 10 .. 126, so the open costs never span more than 127 values), then every parent by the contract's key, then the info -- where the device path relaxes
// to a fixed point.
#include "ssm_host.h"
using namespace ssm_rtc;

static_assert(sizeof(ssm_route_info) == 64, "info is eight 64-bit counts");
static_assert(sizeof(ssm_route_path_info) == 56, "path info is seven 64-bit counts");
static_assert(sizeof(ssm_route_params) == 24, "the parameters are 24 bytes");

extern "C" void ssm_route_params_default(ssm_route_params* p)
{
    if (!p) return;
    p->moves = 8; p->near_weight = 2; p->comfort = 2.0; p->cell = 1.0;
}
int route_check(ssm_ctx* c, const ssm_route_params& P, int nx, int ny, double cell, Setup* S)
{
    using ssm_carvec::finite_d;
    if (nx < 1 || ny < 1 || (int64_t)nx * ny > ssm_gridc::MAX_CELLS) return host_fail(c, SSM_E_INVAL, "route: at least 1 x 1 and at most 2^24 cells");
    if (nx > ssm_clrc::MAX_SIDE || ny > ssm_clrc::MAX_SIDE) return host_fail(c, SSM_E_INVAL, "route: a side of the grid may have at most 32768 cells");
    if (P.moves != 4 && P.moves != 8) return host_fail(c, SSM_E_INVAL, "route: moves must be 4 or 8");
    if (P.near_weight < 0 || P.near_weight > MAX_NEAR_WEIGHT) return host_fail(c, SSM_E_INVAL, "route: near_weight must be 0 .. 8");
    if (!(P.comfort >= 0.0 && finite_d(P.comfort))) return host_fail(c, SSM_E_INVAL, "route: comfort must be finite and not negative");
    if (!(cell > 0.0 && finite_d(cell))) return host_fail(c, SSM_E_INVAL, "route: the cell size must be finite and positive");
    S->moves = P.moves; S->near_weight = P.near_weight; S->comfort2 = comfort2_of(P.comfort, cell);
    return SSM_OK;
}
int route_goal_check(ssm_ctx* c, int nx, int ny, int goal_cx, int goal_cy, int goal_snap)
{
    if (goal_snap < 0 || goal_snap > ssm_clrc::MAX_SNAP) return host_fail(c, SSM_E_INVAL, "route: goal_snap must be 0 .. 1024 cells");
    if (goal_cx < 0 || goal_cy < 0 || goal_cx >= nx || goal_cy >= ny) return host_fail(c, SSM_E_INVAL, "route: the goal must be a cell of the grid");
    return SSM_OK;
}
int route_source_check(ssm_ctx* c, const uint8_t* reach, int nx, int ny, int source_cell)
{
    if (source_cell == -1) return SSM_OK;
    if (source_cell < 0 || (int64_t)source_cell >= (int64_t)nx * ny || reach[source_cell] != ssm_clrc::REACHABLE)
        return host_fail(c, SSM_E_INVAL, "route: the source is -1 or a cell of the grid with reach == 2");
    return SSM_OK;
}
void route_path_none(ssm_route_path_info* I) { memset(I, 0, sizeof *I); I->goal_cell = -1; I->cost = -1; I->min_d2 = -1; }

namespace {
// the moves that exist at the cell (cx, cy): f(neighbour index, step)
template <class F> inline void for_moves(const uint8_t* in, int nx, int ny, int cx, int cy, int moves, F f)
{
    for (int m = 0; m < moves; m++) {
        const int dx = move_dx(m), dy = move_dy(m), x = cx + dx, y = cy + dy;
        if (x < 0 || y < 0 || x >= nx || y >= ny) continue;
        const size_t b = (size_t)y * nx + x;
        if (!in[b]) continue;
        if (m >= 4 && !(in[(size_t)cy * nx + x] && in[(size_t)y * nx + cx])) continue;          // no corner is cut
        f((int32_t)b, m < 4 ? STEP_AXIAL : STEP_DIAG);
    }
}
}

extern "C" int ssm_route_cells_host(const uint8_t* reach, const uint32_t* dist2, int nx, int ny, int source_cell, const ssm_route_params* params, uint32_t* cost_out,
                                    int32_t* parent_out, ssm_route_info* info)
{
    ssm_route_params P; ssm_route_params_default(&P); if (params) P = *params;
    Setup S;
    { const int r = route_check(nullptr, P, nx, ny, P.cell, &S); if (r) return r; }
    if (!reach || !dist2) return host_fail(nullptr, SSM_E_INVAL, "null argument");
    { const int r = route_source_check(nullptr, reach, nx, ny, source_cell); if (r) return r; }
    const size_t nc = (size_t)nx * ny;
    std::vector<uint8_t> in(nc); std::vector<uint32_t> cost(nc, COST_NONE); std::vector<int32_t> parent(nc, -1);
    for (size_t i = 0; i < nc; i++) in[i] = cell_byte(reach[i], dist2[i], S.comfort2);
    if (source_cell >= 0) {
        // the open cells by cost modulo 127: a cell popped at cost d pushes at d + 10 .. d + 126, never into the bucket being emptied; an entry whose cost fell
        // after it was pushed is skipped when its turn comes
        static const uint32_t NB = MAX_EDGE + 1;
        std::vector<std::vector<int32_t>> bucket(NB);
        size_t open = 1;
        cost[(size_t)source_cell] = 0; bucket[0].push_back(source_cell);
        for (uint32_t d = 0; open; d++) {
            std::vector<int32_t>& B = bucket[d % NB];
            for (size_t k = 0; k < B.size(); k++) {
                const int32_t a = B[k]; open--;
                if (cost[(size_t)a] != d) continue;
                const uint32_t wa = weight_of(in[(size_t)a], S.near_weight);
                for_moves(in.data(), nx, ny, a % nx, a / nx, S.moves, [&](int32_t b, int32_t step) {
                    const uint32_t nd = d + edge_of(step, wa, weight_of(in[(size_t)b], S.near_weight));
                    if (nd < cost[(size_t)b]) { cost[(size_t)b] = nd; bucket[nd % NB].push_back(b); open++; }
                });
            }
            B.clear();
        }
    }
    ssm_route_info I; memset(&I, 0, sizeof I);
    I.far_cell = -1; I.source_cell = source_cell; I.comfort2 = S.comfort2; I.moves = S.moves;
    unsigned long long far = 0; bool any = false;
    for (size_t i = 0; i < nc; i++) {
        if (!in[i]) continue;
        if (cost[i] == COST_NONE) { I.unrouted++; continue; }
        I.routed++; if (in[i] & CELL_NEAR) I.near_cells++;
        const unsigned long long k = far_key(cost[i], (int32_t)i);
        if (!any || k > far) { far = k; any = true; }
        if ((int32_t)i == source_cell) continue;
        unsigned long long best = ssm_clrc::KEY_NONE;
        const uint32_t wc = weight_of(in[i], S.near_weight);
        for_moves(in.data(), nx, ny, (int)(i % (size_t)nx), (int)(i / (size_t)nx), S.moves, [&](int32_t p, int32_t step) {
            if (cost[(size_t)p] == COST_NONE) return;
            best = std::min(best, parent_key(cost[(size_t)p] + edge_of(step, weight_of(in[(size_t)p], S.near_weight), wc), p));
        });
        parent[i] = (int32_t)(best & (unsigned long long)INDEX_MASK);
    }
    if (any) { I.max_cost = (int64_t)(far >> 24); I.far_cell = far_cell_of(far); }
    if (cost_out) memcpy(cost_out, cost.data(), nc * 4);
    if (parent_out) memcpy(parent_out, parent.data(), nc * 4);
    if (info) *info = I;
    return SSM_OK;
}

extern "C" int ssm_route_path_host(const uint32_t* cost, const int32_t* parent, const uint32_t* dist2, int nx, int ny, const ssm_route_params* params, int goal_cx, int goal_cy,
                                   int goal_snap, int max_path, int32_t* cells_out, ssm_route_path_info* path_info)
{
    ssm_route_params P; ssm_route_params_default(&P); if (params) P = *params;
    Setup S;
    { const int r = route_check(nullptr, P, nx, ny, P.cell, &S); if (r) return r; }
    if (!cost || !parent || !dist2) return host_fail(nullptr, SSM_E_INVAL, "null argument");
    { const int r = route_goal_check(nullptr, nx, ny, goal_cx, goal_cy, goal_snap); if (r) return r; }
    if (max_path < 1) return host_fail(nullptr, SSM_E_INVAL, "route: max_path must be at least 1");
    ssm_route_path_info I; route_path_none(&I);
    const ssm_clrc::Setup G = goal_setup(goal_cx, goal_cy, goal_snap);
    unsigned long long key = ssm_clrc::KEY_NONE;
    for (int y = std::max(0, goal_cy - goal_snap); y <= std::min(ny - 1, goal_cy + goal_snap); y++)
        for (int x = std::max(0, goal_cx - goal_snap); x <= std::min(nx - 1, goal_cx + goal_snap); x++)
            if (cost[(size_t)y * nx + x] != COST_NONE) key = std::min(key, ssm_clrc::seed_key(x, y, nx, G));
    int rc = SSM_OK;
    if (key != ssm_clrc::KEY_NONE) {
        const int32_t goal = (int32_t)(key & (unsigned long long)INDEX_MASK);
        const int64_t nc = (int64_t)nx * ny;
        I.goal_cell = goal; I.cost = cost[(size_t)goal]; I.min_d2 = dist2[(size_t)goal];
        // costs strictly fall along parents: the walk ends at the source after fewer than nc steps (the bound only guards arrays that are not a field's)
        for (int32_t a = goal; a >= 0 && I.len < nc; a = parent[(size_t)a]) {
            I.len++;
            I.min_d2 = std::min<int64_t>(I.min_d2, dist2[(size_t)a]);
            if (near_of(dist2[(size_t)a], S.comfort2)) I.near_steps++;
            const int32_t p = parent[(size_t)a];
            if (p < 0 || p >= nc) break;
            if (step_is_diag(a, p, nx)) I.n_diag++; else I.n_axial++;
        }
        if (I.len > max_path) rc = host_fail(nullptr, SSM_E_CAPACITY, "route: the path has more cells than max_path");
        else if (cells_out) {
            int64_t k = I.len;
            for (int32_t a = goal; k > 0; a = parent[(size_t)a]) cells_out[--k] = a;
        }
    }
    if (path_info) *path_info = I;
    return rc;
}
