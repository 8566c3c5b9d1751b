// test_route_core.cpp -- the route field on the host (csrc/ssm_route_host.cpp over include/ssm/route_core.h) as a stand-alone program: linked with that source
// alone, it needs neither libssm_hip.so nor a GPU and runs as it is under the CPU sanitizers (-fsanitize=address,undefined).  Checked here, from C++: random inputs
// of many shapes against a restatement written out here (every cell relaxed from its neighbours until nothing changes -- no queue, no buckets; parents and the
// goal's snap by keys over everything), in buffers of exactly the sizes the calls may touch (the sanitizer sees any byte beyond them); the cases of DESIGN.md s.23
// with known outcomes (the open field, the corridor, the pillar, the diagonal gap, the serpentine); comfort2; max_path; invalid arguments.
#include "ssm_hip.h"
#include "ssm/route_core.h"
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>
// what the host sources ask of their surroundings (csrc/ssm_host.h): the error path
static std::string g_err;
int host_fail(ssm_ctx*, int code, const std::string& msg) { g_err = msg; return code; }
using namespace std;

static int failures = 0;
static void check(bool ok, const string& name) { printf("%s %s\n", ok ? "PASS" : "FAIL", name.c_str()); if (!ok) failures++; }
struct Rng { uint64_t s; uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); } double unit() { return (double)(next() % 1000000) / 1000000.0; } };

struct Map {
    int nx, ny; vector<uint8_t> reach; vector<uint32_t> d2;
    Map(int nx_, int ny_, uint8_t r = 2, uint32_t d = 10000) : nx(nx_), ny(ny_), reach((size_t)nx_ * ny_, r), d2((size_t)nx_ * ny_, d) {}
    uint8_t& r(int x, int y) { return reach[(size_t)y * nx + x]; }
    uint32_t& d(int x, int y) { return d2[(size_t)y * nx + x]; }
    int at(int x, int y) const { return y * nx + x; }
};
struct Out { vector<uint32_t> cost; vector<int32_t> parent; ssm_route_info info; int rc; };
static ssm_route_params params(int moves = 8, int near_weight = 2, double comfort = 2.0, double cell = 1.0)
{ ssm_route_params P; ssm_route_params_default(&P); P.moves = moves; P.near_weight = near_weight; P.comfort = comfort; P.cell = cell; return P; }
// buffers of exactly the sizes the call may touch
static Out run(const Map& m, int source, const ssm_route_params& P)
{
    Out o; const size_t nc = (size_t)m.nx * m.ny;
    o.cost.assign(nc, 7); o.parent.assign(nc, -7); memset(&o.info, 0x55, sizeof o.info);
    o.rc = ssm_route_cells_host(m.reach.data(), m.d2.data(), m.nx, m.ny, source, &P, o.cost.data(), o.parent.data(), &o.info);
    return o;
}
struct PathOut { vector<int32_t> cells; ssm_route_path_info info; int rc; };
static PathOut path(const Map& m, const Out& o, const ssm_route_params& P, int gx, int gy, int snap, int max_path)
{
    PathOut p; p.cells.assign((size_t)max_path, -7); memset(&p.info, 0x55, sizeof p.info);
    p.rc = ssm_route_path_host(o.cost.data(), o.parent.data(), m.d2.data(), m.nx, m.ny, &P, gx, gy, snap, max_path, p.cells.data(), &p.info);
    return p;
}
// the restatement: the moves that exist at a cell, then relaxation to a fixed point
static long long comfort2(const ssm_route_params& P) { const double q = P.comfort / P.cell; return q * q < 2147483648.0 ? (long long)floor(q * q) : 1ll << 31; }
struct Edge { int to; long long cost; };
static vector<Edge> moves_at(const Map& m, const ssm_route_params& P, int x, int y)
{
    vector<Edge> e; const long long c2 = comfort2(P);
    auto in = [&](int X, int Y) { return X >= 0 && Y >= 0 && X < m.nx && Y < m.ny && m.reach[(size_t)Y * m.nx + X] == 2; };
    auto w = [&](int X, int Y) { return (long long)m.d2[(size_t)Y * m.nx + X] <= c2 ? 1 + P.near_weight : 1; };
    if (!in(x, y)) return e;
    for (int dy = -1; dy <= 1; dy++) for (int dx = -1; dx <= 1; dx++) {
        if ((!dx && !dy) || (P.moves == 4 && dx && dy) || !in(x + dx, y + dy)) continue;
        if (dx && dy && !(in(x + dx, y) && in(x, y + dy))) continue;
        e.push_back(Edge{(y + dy) * m.nx + x + dx, (dx && dy ? 7 : 5) * (long long)(w(x, y) + w(x + dx, y + dy))});
    }
    return e;
}
static bool restated(const Map& m, int source, const ssm_route_params& P, const Out& o, string* why)
{
    const int nx = m.nx, ny = m.ny; const size_t nc = (size_t)nx * ny; const long long NONE = -1, c2 = comfort2(P);
    vector<long long> cost(nc, NONE);
    if (source >= 0) cost[(size_t)source] = 0;
    for (bool changed = source >= 0; changed;) {
        changed = false;
        for (int y = 0; y < ny; y++) for (int x = 0; x < nx; x++) {
            const size_t i = (size_t)y * nx + x;
            for (const Edge& e : moves_at(m, P, x, y)) {
                if (cost[(size_t)e.to] == NONE) continue;
                const long long v = cost[(size_t)e.to] + e.cost;
                if (cost[i] == NONE || v < cost[i]) { cost[i] = v; changed = true; }
            }
        }
    }
    long long routed = 0, unrouted = 0, near = 0, maxc = 0, far = -1;
    for (int y = 0; y < ny; y++) for (int x = 0; x < nx; x++) {
        const size_t i = (size_t)y * nx + x;
        const uint32_t want = cost[i] == NONE ? UINT32_MAX : (uint32_t)cost[i];
        if (o.cost[i] != want) { *why = "cost at " + to_string(i); return false; }
        long long best = LLONG_MAX;
        if (cost[i] != NONE && (int)i != source) for (const Edge& e : moves_at(m, P, x, y)) if (cost[(size_t)e.to] != NONE) best = min(best, ((cost[(size_t)e.to] + e.cost) << 24) | e.to);
        const int32_t par = best == LLONG_MAX ? -1 : (int32_t)(best & 0xFFFFFF);
        if (o.parent[i] != par) { *why = "parent at " + to_string(i); return false; }
        if (m.reach[i] != 2) continue;
        if (cost[i] == NONE) { unrouted++; continue; }
        routed++; near += (long long)m.d2[i] <= c2;
        if (far < 0 || cost[i] > maxc) { maxc = cost[i]; far = (long long)i; }
    }
    const ssm_route_info& I = o.info;
    if (I.routed != routed || I.unrouted != unrouted || I.near_cells != near || I.max_cost != maxc || I.far_cell != far || I.source_cell != source || I.comfort2 != c2 || I.moves != P.moves) { *why = "info"; return false; }
    return true;
}
// a path against the contract: the snap by a key over every cell, then every property of the walk
static bool path_restated(const Map& m, int source, const ssm_route_params& P, const Out& o, int gx, int gy, int snap, const PathOut& p, string* why)
{
    const long long c2 = comfort2(P);
    long long best = LLONG_MAX;
    for (int y = 0; y < m.ny; y++) for (int x = 0; x < m.nx; x++) {
        const long long d = (long long)(x - gx) * (x - gx) + (long long)(y - gy) * (y - gy);
        if (o.cost[(size_t)y * m.nx + x] != UINT32_MAX && d <= (long long)snap * snap) best = min(best, (d << 24) | (y * m.nx + x));
    }
    const ssm_route_path_info& I = p.info;
    if (best == LLONG_MAX) { if (p.rc != SSM_OK || I.len != 0 || I.goal_cell != -1 || I.cost != -1 || I.min_d2 != -1 || I.n_axial || I.n_diag || I.near_steps) { *why = "no goal cell"; return false; } return true; }
    const int goal = (int)(best & 0xFFFFFF);
    if (p.rc != SSM_OK || I.goal_cell != goal || I.cost != (long long)o.cost[(size_t)goal] || I.len < 1 || p.cells[0] != source || p.cells[(size_t)I.len - 1] != goal) { *why = "ends"; return false; }
    long long sum = 0, axial = 0, diag = 0, near = 0, mind = LLONG_MAX;
    for (long long k = 0; k < I.len; k++) {
        const int a = p.cells[(size_t)k];
        near += (long long)m.d2[(size_t)a] <= c2; mind = min(mind, (long long)m.d2[(size_t)a]);
        if (k + 1 == I.len) break;
        const int b = p.cells[(size_t)k + 1];
        if (o.parent[(size_t)b] != a) { *why = "not the parents' way"; return false; }
        bool found = false;
        for (const Edge& e : moves_at(m, P, a % m.nx, a / m.nx)) if (e.to == b) { sum += e.cost; found = true; (abs(a % m.nx - b % m.nx) + abs(a / m.nx - b / m.nx) == 2 ? diag : axial)++; }
        if (!found) { *why = "a step that is no move"; return false; }
    }
    if (sum != I.cost || axial != I.n_axial || diag != I.n_diag || near != I.near_steps || mind != I.min_d2 || axial + diag != I.len - 1) { *why = "sums"; return false; }
    for (size_t k = (size_t)I.len; k < p.cells.size(); k++) if (p.cells[k] != -7) { *why = "written beyond the path"; return false; }
    return true;
}

static void random_shapes()
{
    static const int shapes[][2] = {{1, 1}, {1, 2}, {2, 1}, {1, 9}, {9, 1}, {2, 2}, {3, 3}, {7, 5}, {5, 7}, {16, 16}, {31, 33}, {33, 31}, {40, 3}, {3, 40}, {65, 2}};
    Rng rng{12345};
    int n = 0, bad = 0; string first;
    for (const auto& s : shapes) for (double fraction : {0.0, 0.15, 0.45, 1.0}) for (int moves : {4, 8}) {
        Map m(s[0], s[1]);
        vector<int> can;
        for (size_t i = 0; i < m.reach.size(); i++) {
            if (rng.unit() < fraction) m.reach[i] = (uint8_t)(rng.next() % 2);
            m.d2[i] = rng.next() % 50 == 0 ? UINT32_MAX : rng.next() % 13;
            if (m.reach[i] == 2) can.push_back((int)i);
        }
        const int source = can.empty() ? -1 : can[rng.next() % can.size()];
        const ssm_route_params P = params(moves, (int)(rng.next() % 9), 0.5 * (double)(rng.next() % 8));
        const Out o = run(m, source, P);
        string why;
        n++;
        if (o.rc != SSM_OK || !restated(m, source, P, o, &why)) { if (!bad++) first = to_string(s[0]) + " x " + to_string(s[1]) + ": " + why; continue; }
        for (int k = 0; k < 4; k++) {
            const int gx = (int)(rng.next() % (uint32_t)m.nx), gy = (int)(rng.next() % (uint32_t)m.ny), snap = (int)(rng.next() % 5);
            const PathOut p = path(m, o, P, gx, gy, snap, m.nx * m.ny);
            if (!path_restated(m, source, P, o, gx, gy, snap, p, &why)) { if (!bad++) first = to_string(s[0]) + " x " + to_string(s[1]) + " path: " + why; break; }
        }
    }
    check(bad == 0, "random inputs == the restatement (" + to_string(n) + " fields, " + to_string(bad) + " bad" + (bad ? ", first " + first : "") + ")");
}

static void planted()
{
    {   // the open field: a chamfer distance
        Map m(21, 17); bool ok = true;
        for (int moves : {4, 8}) {
            const Out o = run(m, m.at(10, 8), params(moves));
            for (int y = 0; y < 17; y++) for (int x = 0; x < 21; x++) {
                const int dx = abs(x - 10), dy = abs(y - 8);
                ok = ok && o.cost[(size_t)m.at(x, y)] == (uint32_t)(moves == 8 ? 10 * max(dx, dy) + 4 * min(dx, dy) : 10 * (dx + dy));
            }
            ok = ok && o.info.far_cell == 0 && o.info.routed == 21 * 17 && o.info.near_cells == 0;
        }
        check(ok, "open field: 10 max + 4 min under 8 moves, 10 (|dx| + |dy|) under 4");
    }
    {   // the corridor
        Map m(21, 3); for (int x = 5; x <= 15; x++) m.d(x, 1) = 1;
        const Out o0 = run(m, m.at(0, 1), params(8, 0)), o1 = run(m, m.at(0, 1), params(8, 1)), o8 = run(m, m.at(0, 1), params(8, 8));
        check(o0.cost[(size_t)m.at(20, 1)] == 200 && o1.cost[(size_t)m.at(20, 1)] == 208 && o8.cost[(size_t)m.at(20, 1)] == 208 && o1.info.comfort2 == 4, "corridor: 200, 208 and 208");
        const PathOut p = path(m, o8, params(8, 8), 20, 1, 0, 63);
        bool row0 = false, row2 = false;
        for (long long k = 0; k < p.info.len; k++) { row0 = row0 || p.cells[(size_t)k] / 21 == 0; row2 = row2 || p.cells[(size_t)k] / 21 == 2; }
        check(p.rc == SSM_OK && row0 && !row2 && p.info.near_steps == 0 && p.info.min_d2 == 10000 && p.info.n_diag == 2 && p.info.n_axial == 18, "corridor: the path leaves through row 0, the lower indices");
    }
    {   // the pillar
        Map m(5, 5); m.r(2, 2) = 0;
        const Out o = run(m, m.at(2, 1), params());
        check(o.cost[(size_t)m.at(2, 3)] == 40 && o.cost[(size_t)m.at(1, 3)] == 30 && o.cost[(size_t)m.at(3, 3)] == 30 && o.parent[(size_t)m.at(2, 3)] == m.at(1, 3), "pillar: two ways of 40, the lower parent");
    }
    {   // the diagonal gap
        Map m(8, 8); for (int x = 0; x < 4; x++) { m.r(x, 3) = 0; m.r(x + 4, 4) = 0; }
        const Out o = run(m, m.at(1, 1), params());
        check(o.info.routed == 28 && o.info.unrouted == 28 && o.cost[(size_t)m.at(3, 4)] == UINT32_MAX && o.parent[(size_t)m.at(3, 4)] == -1 && o.cost[(size_t)m.at(4, 3)] != UINT32_MAX, "diagonal gap: no corner is cut");
    }
    {   // the serpentine
        const int n = 65; Map m(n, n);
        for (int y = 1; y < n; y += 2) for (int x = 0; x < n; x++) m.r(x, y) = (uint8_t)(x == (y % 4 == 1 ? n - 1 : 0) ? 2 : 0);
        const Out o = run(m, 0, params());
        const PathOut p = path(m, o, params(), 64, 64, 0, n * n);
        check(o.info.max_cost == 21760 && o.info.far_cell == m.at(64, 64) && o.info.unrouted == 0 && p.rc == SSM_OK && p.info.len == 2177 && p.info.n_diag == 0, "serpentine 65 x 65: 21760");
    }
    {   // no seed
        Map m(7, 5);
        const Out o = run(m, -1, params());
        const PathOut p = path(m, o, params(), 3, 2, 1024, 35);
        check(o.rc == SSM_OK && o.info.routed == 0 && o.info.unrouted == 35 && o.info.far_cell == -1 && o.info.max_cost == 0 && o.cost == vector<uint32_t>(35, UINT32_MAX) && o.parent == vector<int32_t>(35, -1) &&
              p.rc == SSM_OK && p.info.len == 0 && p.info.goal_cell == -1, "no seed: nothing routed, every output none");
    }
}

static void limits()
{
    Map m(10, 1);
    const ssm_route_params P = params();
    const Out o = run(m, 0, P);
    const PathOut fits = path(m, o, P, 9, 0, 0, 10), shorter = path(m, o, P, 9, 0, 0, 9);
    check(fits.rc == SSM_OK && fits.info.len == 10 && fits.cells[9] == 9 && shorter.rc == SSM_E_CAPACITY && shorter.info.len == 10 && shorter.info.cost == 90 && shorter.cells == vector<int32_t>(9, -7) &&
          g_err.find("max_path") != string::npos, "max_path: exactly as long, and one cell more");
    bool ok = true;
    const double cases[][3] = {{0.0, 1.0, 0}, {2.0, 1.0, 4}, {1.999, 1.0, 3}, {0.2, 0.2, 1}, {0.1999, 0.2, 0}, {1.0, 0.2, 25}, {1e9, 1.0, 2147483648.0}, {46340.95, 1.0, 2147483646.0}, {46341.0, 1.0, 2147483648.0}};
    for (const auto& c : cases) ok = ok && run(m, 0, params(8, 2, c[0], c[1])).info.comfort2 == (int64_t)c[2] && ssm_rtc::comfort2_of(c[0], c[1]) == (int64_t)c[2];
    check(ok, "comfort2 = floor((comfort / cell)^2), saturated at 2^31");
    const double nan = numeric_limits<double>::quiet_NaN(), inf = numeric_limits<double>::infinity();
    int refused = 0, tried = 0;
    for (const ssm_route_params& B : {params(6), params(0), params(8, -1), params(8, 9), params(8, 2, -0.1), params(8, 2, nan), params(8, 2, inf), params(8, 2, 2.0, 0.0), params(8, 2, 2.0, -1.0), params(8, 2, 2.0, nan),
                                      params(8, 2, 2.0, inf)}) {
        tried++; refused += run(m, 0, B).rc == SSM_E_INVAL && g_err.find("route:") == 0;
        tried++; refused += path(m, o, B, 0, 0, 0, 10).rc == SSM_E_INVAL;
    }
    for (int source : {-2, 10, 1 << 24}) { tried++; refused += run(m, source, P).rc == SSM_E_INVAL && g_err.find("source") != string::npos; }
    { Map q(10, 1); q.r(3, 0) = 1; tried++; refused += run(q, 3, P).rc == SSM_E_INVAL; }
    const int goals[][3] = {{10, 0, 0}, {0, 1, 0}, {-1, 0, 0}, {0, -1, 0}, {0, 0, -1}, {0, 0, 1025}};
    for (const auto& gl : goals) { tried++; refused += path(m, o, P, gl[0], gl[1], gl[2], 10).rc == SSM_E_INVAL; }
    ssm_route_path_info PI; int32_t cells[10];
    tried++; refused += ssm_route_path_host(o.cost.data(), o.parent.data(), m.d2.data(), 10, 1, &P, 0, 0, 0, 0, cells, &PI) == SSM_E_INVAL;
    tried++; refused += ssm_route_path_host(nullptr, o.parent.data(), m.d2.data(), 10, 1, &P, 0, 0, 0, 10, cells, &PI) == SSM_E_INVAL;
    tried++; refused += ssm_route_cells_host(nullptr, m.d2.data(), 10, 1, 0, &P, nullptr, nullptr, nullptr) == SSM_E_INVAL;
    tried++; refused += ssm_route_cells_host(m.reach.data(), m.d2.data(), 0, 1, 0, &P, nullptr, nullptr, nullptr) == SSM_E_INVAL;
    tried++; refused += ssm_route_cells_host(m.reach.data(), m.d2.data(), 32769, 1, 0, &P, nullptr, nullptr, nullptr) == SSM_E_INVAL;
    tried++; refused += ssm_route_cells_host(m.reach.data(), m.d2.data(), 4097, 4096, 0, &P, nullptr, nullptr, nullptr) == SSM_E_INVAL;
    check(refused == tried, "invalid arguments are refused (" + to_string(refused) + " of " + to_string(tried) + ")");
    check(ssm_route_cells_host(m.reach.data(), m.d2.data(), 10, 1, 0, nullptr, nullptr, nullptr, nullptr) == SSM_OK && ssm_route_path_host(o.cost.data(), o.parent.data(), m.d2.data(), 10, 1, nullptr, 9, 0, 0, 10, nullptr, &PI) == SSM_OK &&
          PI.len == 10 && path(m, o, P, 9, 0, 1024, 10).rc == SSM_OK, "null parameters are the defaults, every output is optional, the limits are legal");
    {   // the longest side
        Map l(32768, 1);
        const Out lo = run(l, 0, P);
        const PathOut lp = path(l, lo, P, 32767, 0, 0, 32768);
        check(lo.cost[32767] == 327670 && lo.info.far_cell == 32767 && lp.rc == SSM_OK && lp.info.len == 32768 && lp.cells[32767] == 32767 && lp.cells[0] == 0, "1 x 32768: 327670 at the far end, a path of 32768 cells");
    }
    {   // the key helpers
        using namespace ssm_rtc;
        bool k = far_cell_of(far_key(5, 77)) == 77 && far_key(5, 3) > far_key(5, 4) && far_key(6, 4) > far_key(5, 3) && parent_key(9, 2) < parent_key(9, 3) && parent_key(8, 3) < parent_key(9, 2) &&
                 edge_of(STEP_DIAG, 9, 9) == MAX_EDGE && edge_of(STEP_AXIAL, 1, 1) == 10 && step_is_diag(0, 6, 5) && !step_is_diag(0, 5, 5) && !step_is_diag(4, 3, 5) && !step_is_diag(0, 1, 1) && step_is_diag(1, 2, 2) && !step_is_diag(0, 1, 2) && !step_is_diag(1, 3, 2) && step_is_diag(4, 5, 5);
        int sx = 0, sy = 0; for (int mv = 0; mv < 8; mv++) { sx += move_dx(mv); sy += move_dy(mv); k = k && (mv < 4) == ((move_dx(mv) == 0) != (move_dy(mv) == 0)); }
        check(k && sx == 0 && sy == 0, "route_core.h: the keys, the edge and the moves");
    }
}

int main()
{
    random_shapes();
    planted();
    limits();
    printf(failures ? "%d FAILED\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
