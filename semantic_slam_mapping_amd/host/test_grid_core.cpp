// test_grid_core.cpp -- the ground grid on the host (csrc/ssm_grid_host.cpp over include/ssm/grid_core.h) as a stand-alone program: linked with that source,
// csrc/ssm_carve_host.cpp (the pose check) and csrc/ssm_cloud_table.cpp (the point count), it needs neither libssm_hip.so nor a GPU and runs as it is under the CPU
// sanitizers (-fsanitize=address,undefined).  Checked here, from C++: the cases of DESIGN.md s.19 with known outcomes (negative coordinates, points on cell
// borders and on the far edge, heights at the band's limits and at base + step, a negative sum, a label tie, labels without a bin, a cell without LOW points,
// the inputs whose conversion to an integer would be undefined, a 1 x 1 grid, no cloud at all), exact-size buffers (the sanitizer sees any byte beyond them),
// invalid arguments, the colour and height images, the frame helper, and random clouds under random poses against a restatement of the section written out here.
#include "ssm_hip.h"
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

static const double EYE[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
// a point at grid coordinates under the default G and the identity pose: world (gx, -gz, gy)
static ssm_point gp(double gx, double gy, double gz, uint32_t label = 4)
{ ssm_point p; memset(&p, 0, sizeof p); p.x = (float)gx; p.y = (float)-gz; p.z = (float)gy; p.w = 1.0f; p.label = label; p.pad[1] = ~label; return p; }
static ssm_grid_params small()
{ ssm_grid_params P; ssm_grid_params_default(&P); P.x0 = -1.0; P.y0 = -1.0; P.cell = 0.25; P.nx = 8; P.ny = 8; P.step = 0.25; return P; }

struct Out { vector<uint8_t> cls, gl, ol; vector<int32_t> gq, tq; vector<uint32_t> n, nh; vector<ssm_grid_cell> cells; ssm_grid_info info; int rc; };
// buffers of exactly the sizes the call may touch
static Out run(const vector<vector<ssm_point>>& clouds, const vector<double>& Tc, const ssm_grid_params& P)
{
    Out o; const size_t nc = (size_t)max(P.nx, 0) * max(P.ny, 0) <= ((size_t)1 << 24) ? (size_t)max(P.nx, 0) * max(P.ny, 0) : 0;
    o.cls.assign(nc, 7); o.gl.assign(nc, 7); o.ol.assign(nc, 7); o.gq.assign(nc, 7); o.tq.assign(nc, 7); o.n.assign(nc, 7); o.nh.assign(nc, 7); o.cells.resize(nc);
    memset(&o.info, 0, sizeof o.info);
    vector<const ssm_point*> ptrs; vector<int32_t> n;
    for (const auto& c : clouds) { ptrs.push_back(c.empty() ? nullptr : c.data()); n.push_back((int32_t)c.size()); }
    o.rc = ssm_grid_host(ptrs.empty() ? nullptr : ptrs.data(), n.empty() ? nullptr : n.data(), Tc.empty() ? nullptr : Tc.data(), (int)clouds.size(), &P,
                         nc ? o.cls.data() : nullptr, nc ? o.gl.data() : nullptr, nc ? o.ol.data() : nullptr, nc ? o.gq.data() : nullptr, nc ? o.tq.data() : nullptr,
                         nc ? o.n.data() : nullptr, nc ? o.nh.data() : nullptr, nc ? o.cells.data() : nullptr, &o.info);
    return o;
}
static vector<double> eyes(size_t m) { vector<double> T; for (size_t k = 0; k < m; k++) T.insert(T.end(), EYE, EYE + 16); return T; }
static Out run1(const vector<ssm_point>& pts, const ssm_grid_params& P) { return run({pts}, eyes(1), P); }

// the restatement of s.19: long arithmetic written out, no call into the header
static bool restated(const vector<vector<ssm_point>>& clouds, const vector<double>& Tc, const ssm_grid_params& P, const Out& o)
{
    const int nx = P.nx, ny = P.ny; const size_t nc = (size_t)nx * ny;
    struct Cell { long long n = 0, hmin = INT_MAX, hmax = INT_MIN, base = INT_MAX, n_low = 0, n_high = 0, sum = 0, hl[12] = {0}, hh[12] = {0}; };
    vector<Cell> cells(nc);
    struct Used { size_t cell; long long hq; uint32_t label; };
    vector<Used> used;
    long long fin = 0, band = 0, outside = 0, total = 0;
    for (size_t k = 0; k < clouds.size(); k++) {
        double M[3][4]; const double* T = &Tc[16 * k];
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) M[i][j] = (P.G[i * 4] * T[j * 4] + P.G[i * 4 + 1] * T[j * 4 + 1]) + P.G[i * 4 + 2] * T[j * 4 + 2];
            M[i][3] = ((P.G[i * 4] * T[12] + P.G[i * 4 + 1] * T[13]) + P.G[i * 4 + 2] * T[14]) + P.G[i * 4 + 3];
        }
        for (const ssm_point& p : clouds[k]) {
            total++;
            const double x = p.x, y = p.y, z = p.z;
            if (!(isfinite(x) && isfinite(y) && isfinite(z))) continue;
            const double qx = M[0][0] * x + M[0][1] * y + M[0][2] * z + M[0][3], qy = M[1][0] * x + M[1][1] * y + M[1][2] * z + M[1][3], qz = M[2][0] * x + M[2][1] * y + M[2][2] * z + M[2][3];
            if (!(isfinite(qx) && isfinite(qy) && isfinite(qz))) continue;
            fin++;
            if (qz < P.h_min || qz > P.h_max) { band++; continue; }
            const double cx = floor((qx - P.x0) / P.cell), cy = floor((qy - P.y0) / P.cell);
            if (cx < 0 || cx > nx - 1 || cy < 0 || cy > ny - 1) { outside++; continue; }
            const long long hq = llrint(qz * 1024.0);
            const size_t ci = (size_t)cy * nx + (size_t)cx;
            Cell& c = cells[ci]; c.n++; c.hmin = min(c.hmin, hq); c.hmax = max(c.hmax, hq);
            used.push_back({ci, hq, p.label});
        }
    }
    const long long step_q = llrint(P.step * 1024.0);
    for (int cy = 0; cy < ny; cy++) for (int cx = 0; cx < nx; cx++) {
        Cell& c = cells[(size_t)cy * nx + cx]; if (!c.n) continue;
        for (int y = cy - P.ground_radius; y <= cy + P.ground_radius; y++) for (int x = cx - P.ground_radius; x <= cx + P.ground_radius; x++) {
            if (x < 0 || y < 0 || x >= nx || y >= ny) continue;
            const Cell& q = cells[(size_t)y * nx + x]; if (q.n) c.base = min(c.base, q.hmin);
        }
    }
    for (const Used& u : used) {
        Cell& c = cells[u.cell];
        if (u.hq <= c.base + step_q) { c.n_low++; c.sum += u.hq; if (u.label <= 11) c.hl[u.label]++; } else { c.n_high++; if (u.label <= 11) c.hh[u.label]++; }
    }
    long long by_class[5] = {0, 0, 0, 0, 0};
    bool ok = o.rc == SSM_OK;
    for (size_t i = 0; i < nc && ok; i++) {
        const Cell& c = cells[i]; const ssm_grid_cell& g = o.cells[i];
        ok = ok && g.n == c.n && g.hmin == c.hmin && g.hmax == c.hmax && g.base == c.base && g.n_low == c.n_low && g.n_high == c.n_high && g.sum_low == c.sum;
        for (int l = 0; l < 12; l++) ok = ok && g.hist_low[l] == c.hl[l] && g.hist_high[l] == c.hh[l];
        int cls = 0, gl = 255, ol = 255; long long gq = INT_MIN, tq = INT_MIN;
        if (c.n) {
            long long best = 0; for (int l = 0; l < 12; l++) if (c.hl[l] > best) { best = c.hl[l]; gl = l; }
            const bool obst = c.n_high >= P.min_obstacle_points;
            if (obst) { best = 0; for (int l = 0; l < 12; l++) if (c.hh[l] > best) { best = c.hh[l]; ol = l; } }
            gq = c.n_low ? (long long)floor((long double)c.sum / (long double)c.n_low) : c.base;          // (|sum| is small here: exact in a long double)
            tq = c.hmax;
            cls = obst ? 4 : (gl == 4 || gl == 3) ? 1 : gl == 5 ? 2 : 3;
        }
        by_class[cls]++;
        ok = ok && o.cls[i] == cls && o.gl[i] == gl && o.ol[i] == ol && o.gq[i] == gq && o.tq[i] == tq && o.n[i] == c.n && o.nh[i] == c.n_high;
    }
    const ssm_grid_info& I = o.info;
    return ok && I.n_in == total && I.n_finite == fin && I.out_of_band == band && I.outside == outside && I.n_used == (long long)used.size() && I.unobserved == by_class[0] &&
           I.drivable == by_class[1] && I.walkable == by_class[2] && I.other_ground == by_class[3] && I.obstacle == by_class[4];
}
static void pose_of(Rng& r, double T[16])
{
    const double a = (r.unit() - 0.5) * 0.2, b = (r.unit() - 0.5) * 0.2, c = (r.unit() - 0.5) * 0.6;
    const double ca = cos(a), sa = sin(a), cb = cos(b), sb = sin(b), cc = cos(c), sc = sin(c);
    const double R[3][3] = {{cb * cc, sa * sb * cc - ca * sc, ca * sb * cc + sa * sc}, {cb * sc, sa * sb * sc + ca * cc, ca * sb * sc - sa * cc}, {-sb, sa * cb, ca * cb}};
    for (int j = 0; j < 3; j++) { for (int i = 0; i < 3; i++) T[j * 4 + i] = R[i][j]; T[j * 4 + 3] = 0; }
    T[12] = r.unit() - 0.5; T[13] = (r.unit() - 0.5) * 0.2; T[14] = r.unit() - 0.5; T[15] = 1;
}

int main()
{
    const float nan = numeric_limits<float>::quiet_NaN(), inf = numeric_limits<float>::infinity();
    const ssm_grid_params S = small();
    const size_t mid = 4 * 8 + 4;          // the cell of grid (0.1, 0.1)
    {
        const Out o = run1({gp(-1.1, 0, 0), gp(0, -1.2, 0), gp(-1.01, -1.01, 0), gp(-0.6, -0.9, 0)}, S);
        check(o.rc == SSM_OK && o.info.outside == 3 && o.info.n_used == 1 && o.n[0 * 8 + 1] == 1 && o.n[0] == 0, "negative coordinates floor, they do not truncate");
    }
    {
        const Out o = run1({gp(-1.0, 0, 0), gp(-0.75, 0, 0), gp(1.0, 0, 0), gp(0.75, 0, 0), gp(0, -1.0, 0), gp(0, -0.75, 0), gp(0, 1.0, 0), gp(0, 0.75, 0)}, S);
        check(o.rc == SSM_OK && o.info.outside == 2 && o.n[4 * 8 + 0] == 1 && o.n[4 * 8 + 1] == 1 && o.n[4 * 8 + 7] == 1 && o.n[0 * 8 + 4] == 1 && o.n[1 * 8 + 4] == 1 && o.n[7 * 8 + 4] == 1,
              "x0 is inside, a border belongs to the cell above it, x0 + nx cell is outside");
    }
    {
        const Out o = run1({gp(0.1, 0.1, -3.0), gp(0.1, 0.1, 3.0), gp(0.1, 0.1, nextafterf(-3.0f, -10.0f)), gp(0.1, 0.1, nextafterf(3.0f, 10.0f))}, S);
        check(o.rc == SSM_OK && o.info.out_of_band == 2 && o.cells[mid].hmin == -3072 && o.cells[mid].hmax == 3072, "h_min and h_max are inside the band");
    }
    {
        ssm_grid_params P = S; P.ground_radius = 0;
        const Out o = run1({gp(0.1, 0.1, 0, 4), gp(0.1, 0.1, 256 / 1024.0, 4), gp(0.1, 0.1, 257 / 1024.0, 9), gp(0.1, 0.1, 257 / 1024.0, 9), gp(0.1, 0.1, 300 / 1024.0, 9)}, P);
        check(o.rc == SSM_OK && o.cells[mid].n_low == 2 && o.cells[mid].n_high == 3 && o.cells[mid].sum_low == 256 && o.cls[mid] == 4 && o.ol[mid] == 9 && o.gl[mid] == 4 && o.gq[mid] == 128 &&
              o.tq[mid] == 300, "base + step_q is LOW, one unit above is HIGH");
    }
    {
        const Out o = run1({gp(0.1, 0.1, -1 / 1024.0), gp(0.1, 0.1, -2 / 1024.0)}, S);
        check(o.rc == SSM_OK && o.cells[mid].sum_low == -3 && o.gq[mid] == -2, "a negative sum floors");
    }
    {
        const Out o = run1({gp(0.1, 0.1, 0, 7), gp(0.1, 0.1, 0, 7), gp(0.1, 0.1, 0, 2), gp(0.1, 0.1, 0, 2), gp(0.1, 0.1, 1, 9), gp(0.1, 0.1, 1, 9), gp(0.1, 0.1, 1, 8), gp(0.1, 0.1, 1, 8)}, S);
        check(o.rc == SSM_OK && o.gl[mid] == 2 && o.ol[mid] == 8, "the lowest id wins a tie");
    }
    {
        const Out o = run1({gp(0.1, 0.1, 0, 12), gp(0.1, 0.1, 0, 255), gp(0.1, 0.1, 0, 0xFFFFFFFFu), gp(0.1, 0.1, 1, 12), gp(0.1, 0.1, 1, 255), gp(0.1, 0.1, 1, 0xFFFFFFFFu)}, S);
        bool empty = true; for (int l = 0; l < 12; l++) empty = empty && !o.cells[mid].hist_low[l] && !o.cells[mid].hist_high[l];
        check(o.rc == SSM_OK && empty && o.cells[mid].n_low == 3 && o.cells[mid].n_high == 3 && o.gl[mid] == 255 && o.ol[mid] == 255 && o.cls[mid] == 4, "labels above 11 enter no bin");
    }
    {
        const Out o = run1({gp(0.1, 0.1, 0), gp(0.1, 0.1, 0.01), gp(0.35, 0.1, 2.0, 8), gp(0.35, 0.1, 2.1, 8)}, S);
        check(o.rc == SSM_OK && o.cells[mid + 1].n_low == 0 && o.cells[mid + 1].base == 0 && o.gq[mid + 1] == 0 && o.gl[mid + 1] == 255 && o.cls[mid + 1] == 3 && o.tq[mid + 1] == 2150,
              "a cell without LOW points takes base as its ground");
    }
    {
        ssm_grid_params P = S; for (int i = 0; i < 12; i++) P.G[i] *= 1e300;
        P.h_min = -100; P.h_max = 100;
        vector<ssm_point> pts(9, gp(0, 0, 0));
        pts[0].x = nan; pts[1].y = nan; pts[2].z = nan; pts[3].x = inf; pts[4].y = -inf; pts[5].z = inf; pts[6].x = 3e38f; pts[7].z = -3e38f;
        const Out o = run1(pts, P);
        check(o.rc == SSM_OK && o.info.n_in == 9 && o.info.n_finite == 1 && o.info.n_used == 1 && o.n[mid] == 1, "non-finite points and non-finite grid coordinates are rejected");
        ssm_grid_params Q = S; Q.cell = 1e-300; Q.x0 = -1e-300; Q.y0 = -1e-300; Q.nx = 2; Q.ny = 2;          // cell indices far beyond any int: compared as doubles
        const Out q = run1({gp(5, 5, 0), gp(-5, 5, 0), gp(0, 0, 0)}, Q);
        check(q.rc == SSM_OK && q.info.outside == 2 && q.info.n_used == 1 && q.n[3] == 1, "a cell index beyond int is outside, never converted");
    }
    {
        ssm_grid_params P = S; P.nx = 1; P.ny = 1; P.x0 = 0; P.y0 = 0; P.ground_radius = 4;
        const Out o = run1({gp(0.1, 0.1, 0.5), gp(0.3, 0.1, 0)}, P);
        check(o.rc == SSM_OK && o.info.n_used == 1 && o.info.outside == 1 && o.cls[0] == 1 && o.gq[0] == 512 && restated({{gp(0.1, 0.1, 0.5), gp(0.3, 0.1, 0)}}, eyes(1), P, o), "a 1 x 1 grid");
        const Out e = run({}, {}, S);
        bool all = e.rc == SSM_OK && e.info.n_in == 0 && e.info.unobserved == 64;
        for (size_t i = 0; i < 64; i++) all = all && e.cls[i] == 0 && e.gl[i] == 255 && e.ol[i] == 255 && e.gq[i] == INT_MIN && e.tq[i] == INT_MIN && e.n[i] == 0 && e.cells[i].hmin == INT_MAX &&
                                              e.cells[i].hmax == INT_MIN && e.cells[i].base == INT_MAX;
        check(all, "no cloud at all: every cell unobserved");
        const Out e1 = run({{}, {gp(0.1, 0.1, 0)}, {}}, eyes(3), S);
        check(e1.rc == SSM_OK && e1.info.n_in == 1 && e1.n[mid] == 1, "empty clouds beside a full one");
    }
    {   // invalid arguments
        const vector<ssm_point> one = {gp(0.1, 0.1, 0)};
        auto bad = [&](ssm_grid_params P) { return run1(one, P).rc == SSM_E_INVAL; };
        const double dnan = nan, dinf = inf;
        bool ok = true; ssm_grid_params P;
        P = S; P.G[5] = dnan; ok = ok && bad(P);   P = S; P.G[11] = dinf; ok = ok && bad(P);   P = S; P.x0 = dnan; ok = ok && bad(P);   P = S; P.y0 = -dinf; ok = ok && bad(P);
        P = S; P.cell = 0; ok = ok && bad(P);      P = S; P.cell = -1; ok = ok && bad(P);      P = S; P.cell = dnan; ok = ok && bad(P); P = S; P.cell = dinf; ok = ok && bad(P);
        P = S; P.nx = 0; ok = ok && bad(P);        P = S; P.ny = -4; ok = ok && bad(P);        P = S; P.nx = 4097; P.ny = 4096; ok = ok && bad(P);
        P = S; P.h_min = 1; P.h_max = 0; ok = ok && bad(P);   P = S; P.h_min = dnan; ok = ok && bad(P);   P = S; P.h_max = dinf; ok = ok && bad(P);
        P = S; P.h_min = -1048577; ok = ok && bad(P);         P = S; P.h_max = 1048577; ok = ok && bad(P);
        P = S; P.step = -0.01; ok = ok && bad(P);  P = S; P.step = dnan; ok = ok && bad(P);    P = S; P.step = dinf; ok = ok && bad(P);
        P = S; P.ground_radius = -1; ok = ok && bad(P);       P = S; P.ground_radius = 5; ok = ok && bad(P);       P = S; P.min_obstacle_points = 0; ok = ok && bad(P);
        check(ok, "every bad parameter is refused");
        P = S; P.step = 1e300; P.h_min = -1048576; P.h_max = 1048576; P.ground_radius = 4;
        const Out o = run1({gp(0.1, 0.1, 1048576.0), gp(0.1, 0.1, -1048576.0)}, P);
        check(o.rc == SSM_OK && o.cells[mid].hmin == -(1 << 30) && o.cells[mid].hmax == (1 << 30) && o.cells[mid].n_low == 2 && o.gq[mid] == 0, "the limits themselves are legal");
        vector<double> T = eyes(2); T[16 + 13] = dnan;
        check(run({one, one}, T, S).rc == SSM_E_INVAL, "a non-finite pose is refused");
        const ssm_point* twice[2] = {one.data(), one.data()}; int32_t n2[2] = {1, 1}; const vector<double> T2 = eyes(2);
        check(ssm_grid_host(twice, n2, T2.data(), 2, &S, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SSM_E_INVAL && g_err.find("twice") != string::npos,
              "the same cloud twice is refused");
        int32_t neg[2] = {1, -1}, big[2] = {INT_MAX, 1};
        const ssm_point* two[2] = {one.data(), one.data() + 1};
        check(ssm_grid_host(two, neg, T2.data(), 2, &S, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SSM_E_INVAL &&
              ssm_grid_host(two, big, T2.data(), 2, &S, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SSM_E_INVAL && g_err.find("2^31") != string::npos &&
              ssm_grid_host(two, n2, T2.data(), -1, &S, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SSM_E_INVAL &&
              ssm_grid_host(nullptr, n2, T2.data(), 2, &S, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SSM_E_INVAL,
              "a negative count, 2^31 points, m < 0 and null lists are refused");
        ssm_grid_info I;
        check(ssm_grid_host(two, n2, T2.data(), 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &I) == SSM_OK && I.n_in == 1 && I.unobserved == 512 * 512 - 1,
              "null parameters are the defaults, null outputs are skipped");
    }
    {   // the frame helper
        double G[12]; const double up[3] = {0, -1, 0}, fw[3] = {0, 0, 1};
        ssm_grid_params D; ssm_grid_params_default(&D);
        bool ok = ssm_grid_frame_from_up(up, fw, G) == SSM_OK;
        for (int i = 0; i < 12; i++) ok = ok && G[i] == D.G[i];
        check(ok, "the default G is the frame of up 0 -1 0, forward 0 0 1");
        const double z3[3] = {0, 0, 0}, along[3] = {0, -3, 0}, bad[3] = {nan, 0, 1};
        check(ssm_grid_frame_from_up(z3, fw, G) == SSM_E_INVAL && ssm_grid_frame_from_up(up, along, G) == SSM_E_INVAL && ssm_grid_frame_from_up(up, bad, G) == SSM_E_INVAL &&
              ssm_grid_frame_from_up(nullptr, fw, G) == SSM_E_INVAL, "degenerate directions are refused");
    }
    {   // the images: exact-size buffers, forward is up
        const uint8_t cls[6] = {0, 1, 4, 4, 3, 2}, gl[6] = {255, 4, 5, 5, 255, 5}, ol[6] = {255, 255, 1, 255, 255, 255};
        const int32_t gq[6] = {INT_MIN, -3072, -3073, 62462, 62463, 0};
        vector<uint8_t> bgr(18, 9); vector<uint16_t> hh(6, 9);
        ssm_grid_colours(cls, gl, ol, gq, 3, 2, -3.0, bgr.data(), hh.data());
        const uint8_t want[18] = {255, 255, 255, 64, 64, 64, 222, 40, 60,   0, 0, 0, 128, 64, 128, 0, 0, 128};
        const uint16_t wh[6] = {65535, 65535, 3073, 0, 1, 1};
        check(!memcmp(bgr.data(), want, 18) && !memcmp(hh.data(), wh, 12), "the colour and height images");
        ssm_grid_colours(cls, gl, ol, gq, 3, 2, -3.0, nullptr, nullptr);
    }
    {   // random clouds under random poses and frames against the restatement
        Rng r{12345};
        bool ok = true;
        for (int t = 0; t < 30 && ok; t++) {
            ssm_grid_params P; ssm_grid_params_default(&P);
            P.nx = 1 + (int)(r.next() % 20); P.ny = 1 + (int)(r.next() % 20); P.cell = 0.1 + r.unit(); P.x0 = -P.cell * P.nx * r.unit(); P.y0 = -1.0 * r.unit();
            P.h_min = -2.0; P.h_max = 1.0 + r.unit(); P.step = 0.4 * r.unit(); P.ground_radius = (int)(r.next() % 5); P.min_obstacle_points = 1 + (int)(r.next() % 4);
            if (t & 1) { const double up[3] = {r.unit() * 0.2, -1, r.unit() * 0.2}, fw[3] = {r.unit() * 0.2, 0, 1}; ssm_grid_frame_from_up(up, fw, P.G); P.G[3] = r.unit(); P.G[11] = r.unit() - 0.5; }
            const int m = (int)(r.next() % 4);
            vector<vector<ssm_point>> clouds((size_t)m); vector<double> T((size_t)m * 16);
            for (int k = 0; k < m; k++) {
                pose_of(r, &T[(size_t)k * 16]);
                const int n = (int)(r.next() % 400);
                for (int i = 0; i < n; i++) {
                    const double gz = -1.5 + 0.05 * r.unit() + (r.next() % 4 == 0 ? 2.5 * r.unit() : 0.0);
                    clouds[(size_t)k].push_back(gp((r.unit() - 0.5) * P.cell * (P.nx + 2), r.unit() * P.cell * (P.ny + 2) - 1.0, gz, r.next() % 15 == 14 ? 255u : r.next() % 14));
                }
            }
            const Out o = run(clouds, T, P);
            ok = restated(clouds, T, P, o);
            // the order of clouds and points does not matter
            vector<vector<ssm_point>> rev(clouds.rbegin(), clouds.rend()); vector<double> Tr;
            for (int k = m - 1; k >= 0; k--) Tr.insert(Tr.end(), T.begin() + k * 16, T.begin() + k * 16 + 16);
            for (auto& c : rev) reverse(c.begin(), c.end());
            const Out q = run(rev, Tr, P);
            ok = ok && q.rc == SSM_OK && !memcmp(&q.info, &o.info, sizeof o.info) && (o.cells.empty() || !memcmp(q.cells.data(), o.cells.data(), o.cells.size() * sizeof(ssm_grid_cell))) &&
                 q.cls == o.cls && q.gl == o.gl && q.ol == o.ol && q.gq == o.gq && q.tq == o.tq && q.n == o.n && q.nh == o.nh;
        }
        check(ok, "random clouds, poses and frames equal the restatement, in any order");
    }
    printf(failures ? "%d FAILED\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
