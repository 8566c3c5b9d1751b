// ssm_clearance_host.cpp -- the clearance map on the CPU: ssm_clearance_cells_host, the parameter defaults and the argument checks the device
// entry points share.  Plain C++ over include/ssm/clearance_core.h with one thread and an algorithm of its own, linear in the cells: a column pass (two sweeps per
// column), then per row the lower envelope of the columns' parabolas with the contract's tie rule built into the integer crossing points, then a flood fill -- where
// the device path evaluates every key of a row (or scans outwards) and labels with a union-find.
#include "ssm_host.h"
using namespace ssm_clrc;

static_assert(sizeof(ssm_clearance_info) == 64, "info is eight 64-bit counts");
static_assert(sizeof(ssm_clearance_params) == 40, "the parameters are 40 bytes");

extern "C" void ssm_clearance_params_default(ssm_clearance_params* p)
{
    if (!p) return;
    p->blocked_mask = 1u << ssm_gridc::OBSTACLE; p->free_mask = 1u << ssm_gridc::DRIVABLE; p->connectivity = 4; p->seed_cx = p->seed_cy = -1; p->seed_snap = 10;
    p->radius = 1.0; p->cell = 1.0;
}
int clearance_check(ssm_ctx* c, const ssm_clearance_params& P, int nx, int ny, double cell, Setup* S)
{
    using ssm_carvec::finite_d;
    if (nx < 1 || ny < 1 || (int64_t)nx * ny > ssm_gridc::MAX_CELLS) return host_fail(c, SSM_E_INVAL, "clearance: at least 1 x 1 and at most 2^24 cells");
    if (nx > MAX_SIDE || ny > MAX_SIDE) return host_fail(c, SSM_E_INVAL, "clearance: a side of the grid may have at most 32768 cells");
    if ((P.blocked_mask | P.free_mask) >> NCLASS) return host_fail(c, SSM_E_INVAL, "clearance: the masks have bits for the cell classes 0 .. 4 only");
    if (P.blocked_mask & P.free_mask) return host_fail(c, SSM_E_INVAL, "clearance: blocked_mask and free_mask must not overlap");
    if (P.connectivity != 4 && P.connectivity != 8) return host_fail(c, SSM_E_INVAL, "clearance: connectivity must be 4 or 8");
    if (!(P.radius >= 0.0 && finite_d(P.radius))) return host_fail(c, SSM_E_INVAL, "clearance: radius must be finite and not negative");
    if (!(cell > 0.0 && finite_d(cell))) return host_fail(c, SSM_E_INVAL, "clearance: the cell size must be finite and positive");
    if (P.seed_snap < 0 || P.seed_snap > MAX_SNAP) return host_fail(c, SSM_E_INVAL, "clearance: seed_snap must be 0 .. 1024 cells");
    const bool none = P.seed_cx == -1 && P.seed_cy == -1;
    if (!none && (P.seed_cx < 0 || P.seed_cy < 0 || P.seed_cx >= nx || P.seed_cy >= ny)) return host_fail(c, SSM_E_INVAL, "clearance: the seed is (-1, -1) or a cell of the grid");
    S->blocked_mask = P.blocked_mask; S->free_mask = P.free_mask; S->r2 = r2_of(P.radius, cell); S->connectivity = P.connectivity;
    S->seed_cx = P.seed_cx; S->seed_cy = P.seed_cy; S->seed_snap = P.seed_snap;
    return SSM_OK;
}

// the column pass: row[i] = the blocked row of cell i's column nearest to it, the lower on a tie, -1 when the column holds none
static void column_pass(const uint8_t* cls, int nx, int ny, uint32_t blocked_mask, std::vector<int32_t>& row)
{
    row.assign((size_t)nx * ny, -1);
    for (int x = 0; x < nx; x++) {
        int32_t lo = -1;
        for (int y = 0; y < ny; y++) { const size_t i = (size_t)y * nx + x; if (in_mask(cls[i], blocked_mask)) lo = y; row[i] = lo; }
        int32_t hi = -1;
        for (int y = ny - 1; y >= 0; y--) { const size_t i = (size_t)y * nx + x; if (in_mask(cls[i], blocked_mask)) hi = y; row[i] = nearer_row(y, row[i], hi); }
    }
}
// The row pass of row cy.  Column p offers the key ((x - p)^2 + g[p], idx[p]) to the cell at x: a parabola.  For p < q the difference of the two squared distances
// is linear in x, so q's key is the smaller one exactly from some integer column t(p, q) on -- the crossing point rounded up, or one past it when the crossing is an
// integer column and p's index wins the tie -- and the classic stack of the lower envelope works on these integers: v the columns on the envelope, z where each
// takes over.
static void row_pass(const int32_t* row, int nx, int cy, uint32_t* dist2, int32_t* nearest, std::vector<int32_t>& v, std::vector<int64_t>& z, std::vector<int64_t>& g, std::vector<int32_t>& idx)
{
    int k = -1;
    for (int q = 0; q < nx; q++) {
        const int32_t r = row[q];
        if (r < 0) continue;
        const int64_t dy = cy - r;
        g[(size_t)q] = dy * dy; idx[(size_t)q] = r * nx + q;
        int64_t t = 0;
        while (k >= 0) {
            const int p = v[(size_t)k];
            const int64_t num = (g[(size_t)q] + (int64_t)q * q) - (g[(size_t)p] + (int64_t)p * p), den = 2 * (int64_t)(q - p);
            const int64_t fl = ssm_gridc::floor_div(num, den);
            const bool exact = fl * den == num;
            t = exact && idx[(size_t)q] < idx[(size_t)p] ? fl : fl + 1;          // q wins from the crossing on when it wins the tie there, otherwise from the next column on
            if (t <= z[(size_t)k]) k--; else break;
        }
        if (k < 0) t = INT64_MIN;
        k++; v[(size_t)k] = q; z[(size_t)k] = t;
    }
    if (k < 0) { for (int x = 0; x < nx; x++) { dist2[x] = D2_NONE; nearest[x] = -1; } return; }
    int j = 0;
    for (int x = 0; x < nx; x++) {
        while (j < k && z[(size_t)j + 1] <= x) j++;
        const int p = v[(size_t)j];
        dist2[x] = (uint32_t)((int64_t)(x - p) * (x - p) + g[(size_t)p]); nearest[x] = idx[(size_t)p];
    }
}

extern "C" int ssm_clearance_cells_host(const uint8_t* cls, int nx, int ny, const ssm_clearance_params* params, uint32_t* dist2_out, int32_t* nearest_out, uint8_t* reach_out,
                                        ssm_clearance_info* info)
{
    ssm_clearance_params P; ssm_clearance_params_default(&P); if (params) P = *params;
    Setup S;
    { const int r = clearance_check(nullptr, P, nx, ny, P.cell, &S); if (r) return r; }
    if (!cls) return host_fail(nullptr, SSM_E_INVAL, "null argument");
    const size_t nc = (size_t)nx * ny;
    std::vector<int32_t> row; std::vector<uint32_t> dist2(nc); std::vector<int32_t> nearest(nc);
    column_pass(cls, nx, ny, S.blocked_mask, row);
    {
        std::vector<int32_t> v((size_t)nx), idx((size_t)nx); std::vector<int64_t> z((size_t)nx + 1), g((size_t)nx);
        for (int y = 0; y < ny; y++) row_pass(row.data() + (size_t)y * nx, nx, y, dist2.data() + (size_t)y * nx, nearest.data() + (size_t)y * nx, v, z, g, idx);
    }
    ssm_clearance_info I; memset(&I, 0, sizeof I);
    I.r2 = S.r2; I.seed_cell = -1;
    std::vector<uint8_t> reach(nc, NOT_TRAVERSABLE);
    unsigned long long seed = KEY_NONE;
    for (size_t i = 0; i < nc; i++) {
        if (in_mask(cls[i], S.blocked_mask)) I.blocked++;
        if (in_mask(cls[i], S.free_mask)) I.free_cells++;
        if (!traversable(cls[i], dist2[i], S.free_mask, S.r2)) continue;
        reach[i] = TRAVERSABLE; I.traversable++;
        if (S.seed_cx >= 0) seed = std::min(seed, seed_key((int32_t)(i % (size_t)nx), (int32_t)(i / (size_t)nx), nx, S));
    }
    if (seed != KEY_NONE) I.seed_cell = (int64_t)(seed & 0xFFFFFFull);
    // the components of the traversable cells: a flood fill from every one not yet seen; the fill that starts at the seed makes its component REACHABLE
    std::vector<uint8_t> seen(nc, 0); std::vector<int32_t> stack;
    static const int DX[8] = {-1, 1, 0, 0, -1, 1, -1, 1}, DY[8] = {0, 0, -1, 1, -1, -1, 1, 1};          // the first four: the 4-neighbourhood
    auto fill = [&](size_t from, bool mark) {
        seen[from] = 1; stack.assign(1, (int32_t)from);
        while (!stack.empty()) {
            const int32_t a = stack.back(); stack.pop_back();
            if (mark) { reach[(size_t)a] = REACHABLE; I.reachable++; I.max_d2_reachable = std::max<int64_t>(I.max_d2_reachable, (int64_t)dist2[(size_t)a]); }
            const int cx = a % nx, cy = a / nx;
            for (int d = 0; d < S.connectivity; d++) {
                const int x = cx + DX[d], y = cy + DY[d];
                if (x < 0 || y < 0 || x >= nx || y >= ny) continue;
                const size_t b = (size_t)y * nx + x;
                if (seen[b] || reach[b] == NOT_TRAVERSABLE) continue;
                seen[b] = 1; stack.push_back((int32_t)b);
            }
        }
    };
    if (I.seed_cell >= 0) { fill((size_t)I.seed_cell, true); I.components++; }
    for (size_t i = 0; i < nc; i++) if (reach[i] != NOT_TRAVERSABLE && !seen[i]) { fill(i, false); I.components++; }
    if (dist2_out) memcpy(dist2_out, dist2.data(), nc * 4);
    if (nearest_out) memcpy(nearest_out, nearest.data(), nc * 4);
    if (reach_out) memcpy(reach_out, reach.data(), nc);
    if (info) *info = I;
    return SSM_OK;
}
