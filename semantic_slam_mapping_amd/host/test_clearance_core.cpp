// test_clearance_core.cpp -- the clearance map on the host (csrc/ssm_clearance_host.cpp over include/ssm/clearance_core.h) as a stand-alone program: linked with that
// source alone, it needs neither libssm_hip.so nor a GPU and runs as it is under the CPU sanitizers (-fsanitize=address,undefined).  Checked here, from C++: random
// class images of many shapes against a restatement written out here (every cell against every blocked cell; labels spread until nothing changes -- no separable
// pass, no envelope, no flood fill), in buffers of exactly the sizes the call may touch (the sanitizer sees any byte beyond them); the cases of DESIGN.md s.22 with
// known outcomes (ties, the corridor that one more cell of radius closes, the diagonal gap, the seed's snap); r2; cell_of against the grid's own point_of; invalid
// arguments.
#include "ssm_hip.h"
#include "ssm/clearance_core.h"
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

struct Image {
    int nx, ny; vector<uint8_t> cls;
    Image(int nx_, int ny_, uint8_t fill = 1) : nx(nx_), ny(ny_), cls((size_t)nx_ * ny_, fill) {}
    uint8_t& at(int x, int y) { return cls[(size_t)y * nx + x]; }
};
struct Out { vector<uint32_t> d2; vector<int32_t> near; vector<uint8_t> reach; ssm_clearance_info info; int rc; };
static ssm_clearance_params params(double radius, int conn = 4, int sx = -1, int sy = -1, int snap = 10)
{ ssm_clearance_params P; ssm_clearance_params_default(&P); P.radius = radius; P.connectivity = conn; P.seed_cx = sx; P.seed_cy = sy; P.seed_snap = snap; return P; }
// buffers of exactly the sizes the call may touch
static Out run(const Image& c, const ssm_clearance_params& P)
{
    Out o; const size_t nc = (size_t)c.nx * c.ny;
    o.d2.assign(nc, 7); o.near.assign(nc, -7); o.reach.assign(nc, 77); memset(&o.info, 0x55, sizeof o.info);
    o.rc = ssm_clearance_cells_host(c.cls.data(), c.nx, c.ny, &P, o.d2.data(), o.near.data(), o.reach.data(), &o.info);
    return o;
}
// the restatement
static bool restated(const Image& c, const ssm_clearance_params& P, const Out& o, string* why)
{
    const int nx = c.nx, ny = c.ny; const size_t nc = (size_t)nx * ny;
    auto in = [](uint8_t cls, uint32_t mask) { return cls < 5 && ((mask >> cls) & 1u); };
    const double q = P.radius / P.cell; const long long r2 = q * q < 2147483648.0 ? (long long)floor(q * q) : 1ll << 31;
    vector<long long> lab(nc, -1); long long blocked = 0, freec = 0, trav = 0;
    for (int y = 0; y < ny; y++) for (int x = 0; x < nx; x++) {
        const size_t i = (size_t)y * nx + x;
        unsigned long long best = ~0ull;
        for (int by = 0; by < ny; by++) for (int bx = 0; bx < nx; bx++) {
            if (!in(c.cls[(size_t)by * nx + bx], P.blocked_mask)) continue;
            const unsigned long long d = (unsigned long long)((x - bx) * (x - bx) + (y - by) * (y - by));
            best = min(best, (d << 24) | (unsigned long long)(by * nx + bx));
        }
        const uint32_t d2 = best == ~0ull ? UINT32_MAX : (uint32_t)(best >> 24); const int32_t near = best == ~0ull ? -1 : (int32_t)(best & 0xFFFFFF);
        if (o.d2[i] != d2 || o.near[i] != near) { *why = "dist2 / nearest at " + to_string(i); return false; }
        if (in(c.cls[i], P.blocked_mask)) blocked++;
        if (in(c.cls[i], P.free_mask)) { freec++; if ((long long)d2 > r2) { lab[i] = (long long)i; trav++; } }
    }
    for (bool changed = true; changed;) {
        changed = false;
        for (int y = 0; y < ny; y++) for (int x = 0; x < nx; x++) {
            const size_t i = (size_t)y * nx + x; if (lab[i] < 0) continue;
            for (int dy = -1; dy <= 1; dy++) for (int dx = -1; dx <= 1; dx++) {
                if ((!dx && !dy) || (P.connectivity == 4 && dx && dy)) continue;
                const int X = x + dx, Y = y + dy; if (X < 0 || Y < 0 || X >= nx || Y >= ny) continue;
                const size_t j = (size_t)Y * nx + X;
                if (lab[j] >= 0 && lab[j] < lab[i]) { lab[i] = lab[j]; changed = true; }
            }
        }
    }
    long long comps = 0, seed = -1, reached = 0, far = 0; unsigned long long sk = ~0ull;
    for (size_t i = 0; i < nc; i++) {
        if (lab[i] == (long long)i) comps++;
        if (lab[i] < 0 || P.seed_cx < 0) continue;
        const long long dx = (long long)(i % nx) - P.seed_cx, dy = (long long)(i / nx) - P.seed_cy, d = dx * dx + dy * dy;
        if (d <= (long long)P.seed_snap * P.seed_snap) sk = min(sk, ((unsigned long long)d << 24) | i);
    }
    if (sk != ~0ull) seed = (long long)(sk & 0xFFFFFF);
    for (size_t i = 0; i < nc; i++) {
        const uint8_t r = lab[i] < 0 ? 0 : seed >= 0 && lab[i] == lab[(size_t)seed] ? 2 : 1;
        if (o.reach[i] != r) { *why = "reach at " + to_string(i); return false; }
        if (r == 2) { reached++; far = max(far, (long long)o.d2[i]); }
    }
    const ssm_clearance_info& I = o.info;
    if (I.blocked != blocked || I.free_cells != freec || I.traversable != trav || I.components != comps || I.reachable != reached || I.seed_cell != seed || I.max_d2_reachable != far || I.r2 != r2) {
        *why = "info"; return false;
    }
    return true;
}

int main()
{
    Rng rng{20261021};
    // random class images: shapes with a side of 1, around 32, wider than tall and the reverse; sparse to full; both connectivities; seeds inside, on the rim, none
    {
        const int shapes[][2] = {{1, 1}, {1, 2}, {2, 1}, {1, 40}, {40, 1}, {7, 5}, {31, 33}, {33, 31}, {32, 32}, {45, 9}, {9, 45}};
        const double fills[] = {0.0, 0.01, 0.1, 0.5, 1.0};
        bool all = true; string why, first;
        for (auto& s : shapes) for (double f : fills) for (int conn : {4, 8}) {
            Image c(s[0], s[1]);
            for (auto& v : c.cls) { const uint32_t r = rng.next() % 10; v = rng.unit() < f ? 4 : r < 6 ? 1 : r == 6 ? 2 : r == 7 ? 3 : 0; }
            ssm_clearance_params P = params(0.5 * (rng.next() % 6), conn, (int)(rng.next() % (uint32_t)s[0]), (int)(rng.next() % (uint32_t)s[1]), (int)(rng.next() % 12));
            if (rng.next() % 4 == 0) P.seed_cx = P.seed_cy = -1;
            if (rng.next() % 3 == 0) { P.blocked_mask = 0x11; P.free_mask = 0x06; }
            const Out o = run(c, P);
            if (o.rc != SSM_OK || !restated(c, P, o, &why)) { if (all) first = to_string(s[0]) + " x " + to_string(s[1]) + " fill " + to_string(f) + ": " + why; all = false; }
        }
        check(all, "random class images == the restatement " + first);
    }
    // ties: mirrored about (4, 3) in a row, a column and both diagonals; the centre of a ring; a row blocked at both ends
    {
        const int pairs[][4] = {{2, 3, 6, 3}, {4, 1, 4, 5}, {2, 1, 6, 5}, {6, 1, 2, 5}};
        bool ok = true;
        for (auto& p : pairs) {
            Image c(9, 7); c.at(p[0], p[1]) = 4; c.at(p[2], p[3]) = 4;
            const Out o = run(c, params(0.0));
            ok = ok && o.rc == SSM_OK && o.near[3 * 9 + 4] == p[1] * 9 + p[0] && o.d2[3 * 9 + 4] == (uint32_t)((4 - p[0]) * (4 - p[0]) + (3 - p[1]) * (3 - p[1]));
        }
        check(ok, "two blocked cells mirrored about a cell: the lower index is the nearest");
        Image ring(13, 13);
        for (int y = 0; y < 13; y++) for (int x = 0; x < 13; x++) if ((x - 6) * (x - 6) + (y - 6) * (y - 6) == 25) ring.at(x, y) = 4;
        const Out r = run(ring, params(0.0));
        check(r.rc == SSM_OK && r.d2[6 * 13 + 6] == 25 && r.near[6 * 13 + 6] == 1 * 13 + 6 && r.info.blocked == 12, "the centre of a ring takes the ring's first cell");
        Image row(9, 1); row.at(0, 0) = 4; row.at(8, 0) = 4;
        const Out w = run(row, params(0.0));
        check(w.rc == SSM_OK && w.d2[4] == 16 && w.near[4] == 0 && w.near[5] == 8 && w.near[3] == 0, "a 1-wide row blocked at both ends");
    }
    // nothing blocked, everything blocked, nothing free
    {
        Image c(6, 4);
        Out o = run(c, params(1e9, 4, 2, 2));
        check(o.rc == SSM_OK && o.d2[0] == UINT32_MAX && o.near[23] == -1 && o.info.traversable == 24 && o.info.reachable == 24 && o.info.max_d2_reachable == (int64_t)UINT32_MAX && o.info.r2 == (int64_t)1 << 31,
              "nothing blocked: UINT32_MAX, -1, and every free cell traversable under any radius");
        Image b(6, 4, 4);
        o = run(b, params(1.0, 4, 2, 2));
        check(o.rc == SSM_OK && o.d2[5] == 0 && o.near[5] == 5 && o.info.blocked == 24 && o.info.traversable == 0 && o.info.components == 0 && o.info.seed_cell == -1, "everything blocked");
        Image u(6, 4, 0);
        o = run(u, params(1.0, 4, 2, 2));
        check(o.rc == SSM_OK && o.info.free_cells == 0 && o.info.components == 0 && o.reach[7] == 0, "an empty grid");
    }
    // the corridor (15 x 21, walls in the columns 0 and 14, a pillar at (7, 10)): radius 2 leaves it open on both sides of the pillar, radius 3 closes it
    {
        Image c(15, 21); for (int y = 0; y < 21; y++) { c.at(0, y) = 4; c.at(14, y) = 4; } c.at(7, 10) = 4;
        const Out open = run(c, params(2.0, 4, 7, 2)), closed = run(c, params(3.0, 4, 7, 2));
        check(open.info.components == 1 && open.reach[18 * 15 + 7] == 2 && open.reach[10 * 15 + 3] == 2 && open.reach[10 * 15 + 5] == 0 && open.info.reachable == open.info.traversable, "radius 2 leaves the lane open");
        check(closed.info.components == 2 && closed.reach[18 * 15 + 7] == 1 && closed.reach[2 * 15 + 7] == 2 && closed.reach[10 * 15 + 4] == 0 && closed.info.reachable < closed.info.traversable,
              "one more cell of radius closes it: the lane behind is unreachable, one component more");
        const Out snap = run(c, params(2.0, 4, 7, 10)), none = run(c, params(2.0, 4, 7, 10, 2));
        check(snap.info.seed_cell == 8 * 15 + 6 && snap.reach[8 * 15 + 6] == 2 && none.info.seed_cell == -1 && none.info.reachable == 0 && none.info.traversable == snap.info.traversable,
              "a seed on a blocked cell snaps to the nearest traversable cell, the lowest index among equals; within 2 cells there is none");
    }
    // a diagonal gap
    {
        Image c(8, 8); for (int x = 0; x < 4; x++) c.at(x, 3) = 4; for (int x = 4; x < 8; x++) c.at(x, 4) = 4;
        const Out c4 = run(c, params(0.0, 4, 1, 1)), c8 = run(c, params(0.0, 8, 1, 1));
        check(c4.info.components == 2 && c8.info.components == 1 && c4.reach[6 * 8 + 6] == 1 && c8.reach[6 * 8 + 6] == 2, "a diagonal gap passes under 8 and not under 4");
    }
    // r2 and cell_of
    {
        Image c(3, 3); c.at(1, 1) = 4;
        auto r2 = [&](double radius, double cell) { ssm_clearance_params P = params(radius); P.cell = cell; return run(c, P).info.r2; };
        check(r2(0.0, 1.0) == 0 && r2(1.0, 1.0) == 1 && r2(0.999, 1.0) == 0 && r2(1.001, 1.0) == 1 && r2(1.0, 0.2) == 25 && r2(0.5, 0.2) == 6 && r2(1e9, 1.0) == (int64_t)1 << 31 &&
              r2(1e300, 1e-300) == (int64_t)1 << 31 && ssm_clrc::r2_of(46340.95, 1.0) < ((int64_t)1 << 31), "r2 = floor((radius / cell)^2), saturated at 2^31");
        ssm_grid_params G; memset(&G, 0, sizeof G); G.x0 = -3.1; G.y0 = 0.7; G.cell = 0.3; G.nx = 20; G.ny = 10;
        ssm_gridc::Setup S{G.x0, G.y0, G.cell, -10.0, 10.0, 0, G.nx, G.ny, 0, 1};
        const double M[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        bool ok = true; int inside = 0;
        for (int k = 0; k < 4000; k++) {
            const float x = (float)(-4.0 + 8.0 * rng.unit()), y = (float)(0.0 + 5.0 * rng.unit());
            ssm_gridc::Hit h{-8, -8, 0}; int32_t cx = -9, cy = -9;
            const bool used = ssm_gridc::point_of(x, y, 0.0f, M, S, &h) == ssm_gridc::P_USED, in = ssm_clrc::cell_of(G, (double)x, (double)y, &cx, &cy);
            ok = ok && used == in && (!in || (cx == h.cx && cy == h.cy)); inside += in;
        }
        int32_t cx, cy;
        check(ok && inside > 500 && inside < 3500 && !ssm_clrc::cell_of(G, std::numeric_limits<double>::quiet_NaN(), 1.0, &cx, &cy) && ssm_clrc::cell_of(G, G.x0, G.y0, &cx, &cy) && cx == 0 && cy == 0,
              "cell_of is the grid's own cell");
    }
    // invalid arguments: nothing is written
    {
        Image c(9, 7); c.at(4, 3) = 4;
        auto bad = [&](ssm_clearance_params P) { const Out o = run(c, P); return o.rc == SSM_E_INVAL && o.d2[0] == 7 && o.near[0] == -7 && o.reach[0] == 77 && g_err.rfind("clearance:", 0) == 0; };
        ssm_clearance_params P = params(1.0);
        bool ok = true;
        { auto Q = P; Q.blocked_mask = 1u << 5; ok = ok && bad(Q); }
        { auto Q = P; Q.free_mask = 1u << 31; ok = ok && bad(Q); }
        { auto Q = P; Q.free_mask = 0x12; ok = ok && bad(Q); }
        { auto Q = P; Q.connectivity = 6; ok = ok && bad(Q); }
        { auto Q = P; Q.radius = -1e-9; ok = ok && bad(Q); }
        { auto Q = P; Q.radius = std::numeric_limits<double>::quiet_NaN(); ok = ok && bad(Q); }
        { auto Q = P; Q.radius = std::numeric_limits<double>::infinity(); ok = ok && bad(Q); }
        { auto Q = P; Q.cell = 0.0; ok = ok && bad(Q); }
        { auto Q = P; Q.seed_snap = -1; ok = ok && bad(Q); }
        { auto Q = P; Q.seed_snap = 1025; ok = ok && bad(Q); }
        { auto Q = P; Q.seed_cx = 9; Q.seed_cy = 0; ok = ok && bad(Q); }
        { auto Q = P; Q.seed_cx = 0; Q.seed_cy = 7; ok = ok && bad(Q); }
        { auto Q = P; Q.seed_cx = -1; Q.seed_cy = 0; ok = ok && bad(Q); }
        check(ok, "invalid parameters");
        ssm_clearance_info I;
        check(ssm_clearance_cells_host(nullptr, 9, 7, &P, nullptr, nullptr, nullptr, &I) == SSM_E_INVAL && ssm_clearance_cells_host(c.cls.data(), 0, 7, &P, nullptr, nullptr, nullptr, &I) == SSM_E_INVAL &&
              ssm_clearance_cells_host(c.cls.data(), 32769, 1, &P, nullptr, nullptr, nullptr, &I) == SSM_E_INVAL && ssm_clearance_cells_host(c.cls.data(), 1, 32769, &P, nullptr, nullptr, nullptr, &I) == SSM_E_INVAL &&
              ssm_clearance_cells_host(c.cls.data(), 4097, 4096, &P, nullptr, nullptr, nullptr, &I) == SSM_E_INVAL, "null image, empty, too long and too large grids");
        check(ssm_clearance_cells_host(c.cls.data(), 9, 7, nullptr, nullptr, nullptr, nullptr, nullptr) == SSM_OK && ssm_clearance_cells_host(c.cls.data(), 9, 7, nullptr, nullptr, nullptr, nullptr, &I) == SSM_OK &&
              I.blocked == 1 && I.r2 == 1 && I.seed_cell == -1, "null parameters are the defaults, every output is optional");
        vector<uint8_t> longrow(32768, 1); longrow[0] = 4; vector<uint32_t> d2(32768);
        check(ssm_clearance_cells_host(longrow.data(), 32768, 1, &P, d2.data(), nullptr, nullptr, nullptr) == SSM_OK && d2[32767] == 1073676289u &&
              ssm_clearance_cells_host(longrow.data(), 1, 32768, &P, d2.data(), nullptr, nullptr, nullptr) == SSM_OK && d2[32767] == 1073676289u, "the longest sides: 32767^2");
    }
    printf(failures ? "%d FAILED\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
