// test_carve_core.cpp -- free-space carving on the host (csrc/ssm_carve_host.cpp over include/ssm/carve_core.h) as a stand-alone program: linked with that one
// source, it needs neither libssm_hip.so nor a GPU and runs as it is under the CPU sanitizers (-fsanitize=address,undefined).
// Checked here, from C++: hand-made points with known verdicts, the inputs whose conversion to an integer would be undefined (+-1e30, NaN, infinity, a depth far
// beyond the image's range), windows at the image's corners, counters at 254 / 255, empty clouds, exact-size buffers (the sanitizer sees any byte beyond them),
// invalid arguments, and random clouds under random poses against a restatement of DESIGN.md s.16 written out here.
#include "ssm_hip.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>
// what the host source asks of its surroundings (csrc/ssm_host.h): the error path
static std::string g_err;
int host_fail(ssm_ctx*, int code, const std::string& msg) { g_err = msg; return code; }
using namespace std;

static int failures = 0;
static void check(bool ok, const char* name) { printf("%s %s\n", ok ? "PASS" : "FAIL", name); if (!ok) failures++; }
struct Rng { uint64_t s; uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); } double unit() { return (double)(next() % 1000000) / 1000000.0; } };

static ssm_point pt(float x, float y, float z, uint32_t tag = 0) { ssm_point p; memset(&p, 0, sizeof p); p.x = x; p.y = y; p.z = z; p.w = 1.0f; p.label = tag; p.pad[1] = ~tag; return p; }
static const double EYE[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
static ssm_camera cam0() { ssm_camera c; c.cx = 0; c.cy = 0; c.fx = 64; c.fy = 64; c.scale = 1000; return c; }
static ssm_point at_pixel(double px, double py, float z, uint32_t tag = 0) { return pt((float)(px * z / 64.0), (float)(py * z / 64.0), z, tag); }

struct Out { vector<ssm_point> pts; vector<uint8_t> run_io, verdict, run; ssm_carve_info info; int rc, n; };
// buffers of exactly the sizes the call may touch
static Out run(const vector<uint16_t>& depth, int w, int h, const ssm_camera& cam, const double* Tv, const vector<ssm_point>& in, const double* Tc, const vector<uint8_t>& run_in,
               const ssm_carve_params& P, int cap = -1)
{
    Out o; const int n = (int)in.size();
    o.pts.assign((size_t)(cap < 0 ? n : cap), pt(7, 7, 7)); o.run_io = run_in; o.verdict.assign((size_t)n, 9); o.run.assign((size_t)n, 9); o.n = -1;
    memset(&o.info, 0, sizeof o.info);
    o.rc = ssm_carve_host(depth.data(), w, h, &cam, Tv, in.data(), n, Tc, o.run_io.empty() ? nullptr : o.run_io.data(), &P, o.pts.empty() ? nullptr : o.pts.data(), (int)o.pts.size(), &o.n, &o.info,
                          n ? o.verdict.data() : nullptr, n ? o.run.data() : nullptr);
    return o;
}
// the restatement of s.16: long arithmetic written out, no call into the header
static void rel(const double* Tv, const double* Tc, double M[3][4])
{
    for (int i = 0; i < 3; i++) {
        const double a = Tv[i * 4], b = Tv[i * 4 + 1], c = Tv[i * 4 + 2];
        const double ti = -((a * Tv[12] + b * Tv[13]) + c * Tv[14]);
        for (int j = 0; j < 3; j++) M[i][j] = (a * Tc[j * 4] + b * Tc[j * 4 + 1]) + c * Tc[j * 4 + 2];
        M[i][3] = ((a * Tc[12] + b * Tc[13]) + c * Tc[14]) + ti;
    }
}
static bool restated(const vector<uint16_t>& depth, int w, int h, const ssm_camera& cam, const double* Tv, const vector<ssm_point>& in, const double* Tc, const vector<uint8_t>& run_in,
                     const ssm_carve_params& P, const Out& o)
{
    double M[3][4]; rel(Tv, Tc, M);
    const int n = (int)in.size(), r = P.radius;
    int cnt[4] = {0, 0, 0, 0}, kept = 0;
    vector<ssm_point> kp; vector<uint8_t> kr;
    for (int i = 0; i < n; i++) {
        const double x = in[i].x, y = in[i].y, z = in[i].z;
        int v = 0;
        do {
            if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z)) break;
            const double qx = M[0][0] * x + M[0][1] * y + M[0][2] * z + M[0][3], qy = M[1][0] * x + M[1][1] * y + M[1][2] * z + M[1][3], qz = M[2][0] * x + M[2][1] * y + M[2][2] * z + M[2][3];
            if (!std::isfinite(qx) || !std::isfinite(qy) || !std::isfinite(qz) || qz < P.z_min) break;
            const double px = floor(cam.fx * (qx / qz) + cam.cx + 0.5), py = floor(cam.fy * (qy / qz) + cam.cy + 0.5);
            if (!(px >= r && px <= w - 1 - r && py >= r && py <= h - 1 - r)) break;
            const int ix = (int)px, iy = (int)py;
            long long dmin = 1 << 20;
            for (int yy = iy - r; yy <= iy + r; yy++) for (int xx = ix - r; xx <= ix + r; xx++) dmin = min<long long>(dmin, depth[(size_t)yy * w + xx]);
            if (dmin == 0) break;
            const long long d = depth[(size_t)iy * w + ix];
            const double zs = qz * cam.scale;
            const long long zq = zs < 1125899906842624.0 ? llrint(zs) : 1125899906842624ll;
            const long long tol = llrint(P.tol_abs * cam.scale) + d * P.tol_rel_ppm / 1000000;
            v = zq + tol < dmin ? 3 : (llabs(zq - d) <= tol ? 2 : 1);
        } while (0);
        cnt[v]++;
        int rn = run_in.empty() ? 0 : run_in[i];
        if (v == 3) rn = min(rn + 1, 255); else if (v == 2) rn = 0;
        if (o.verdict[i] != v || o.run[i] != rn) return false;
        if (rn < P.min_votes) { kp.push_back(in[i]); kr.push_back((uint8_t)rn); kept++; }
    }
    const ssm_carve_info& I = o.info;
    if (I.n_in != n || I.n_kept != kept || I.removed != n - kept || I.unknown != cnt[0] || I.occluded != cnt[1] || I.supported != cnt[2] || I.seen_through != cnt[3] || o.n != kept) return false;
    if (kept && memcmp(o.pts.data(), kp.data(), (size_t)kept * sizeof(ssm_point)) != 0) return false;
    if (!run_in.empty() && kept && memcmp(o.run_io.data(), kr.data(), (size_t)kept) != 0) return false;
    return true;
}
static void random_pose(Rng& g, double rot, double trans, double T[16])
{
    const double ax = (g.unit() - 0.5) * rot, ay = (g.unit() - 0.5) * rot, az = (g.unit() - 0.5) * rot;
    const double cx = cos(ax), sx = sin(ax), cy = cos(ay), sy = sin(ay), cz = cos(az), sz = sin(az);
    const double R[3][3] = {{cy * cz, -cy * sz, sy}, {sx * sy * cz + cx * sz, -sx * sy * sz + cx * cz, -sx * cy}, {-cx * sy * cz + sx * sz, cx * sy * sz + sx * cz, cx * cy}};
    memset(T, 0, 16 * sizeof(double));
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) T[j * 4 + i] = R[i][j];
    for (int i = 0; i < 3; i++) T[12 + i] = (g.unit() - 0.5) * trans;
    T[15] = 1.0;
}

int main()
{
    ssm_carve_params D; ssm_carve_params_default(&D);
    check(D.min_votes == 2 && D.radius == 1 && D.tol_abs == 0.05 && D.tol_rel_ppm == 20000 && D.z_min == 0.1, "defaults");
    const ssm_camera cam = cam0();
    const float big = 1.0e30f, nan = numeric_limits<float>::quiet_NaN(), inf = numeric_limits<float>::infinity();
    {   // known verdicts on a flat view at 1 m, 2 m beyond and 0.5 m in front, radius 0 .. 3 at the corners
        const int w = 8, h = 6;
        for (int r = 0; r <= 3; r++) {
            if (2 * r + 1 > h) continue;
            ssm_carve_params P = D; P.radius = r;
            vector<uint16_t> flat((size_t)w * h, 1000);
            vector<ssm_point> in;
            for (int y = -1; y <= h; y++) for (int x = -1; x <= w; x++) in.push_back(at_pixel(x, y, 1.0f, (uint32_t)in.size()));
            Out o = run(flat, w, h, cam, EYE, in, EYE, {}, P);
            bool ok = o.rc == SSM_OK; size_t i = 0;
            for (int y = -1; y <= h; y++) for (int x = -1; x <= w; x++, i++) ok = ok && o.verdict[i] == ((x >= r && x <= w - 1 - r && y >= r && y <= h - 1 - r) ? 2 : 0);
            check(ok && restated(flat, w, h, cam, EYE, in, EYE, {}, P, o), ("every pixel and the ring outside, radius " + to_string(r)).c_str());
        }
        vector<uint16_t> far((size_t)w * h, 3000), near((size_t)w * h, 500);
        vector<ssm_point> one = {at_pixel(3, 3, 1.0f, 5)};
        Out a = run(far, w, h, cam, EYE, one, EYE, {1}, D), b = run(near, w, h, cam, EYE, one, EYE, {1}, D), c = run(far, w, h, cam, EYE, one, EYE, {0}, D);
        check(a.rc == SSM_OK && a.verdict[0] == 3 && a.run[0] == 2 && a.n == 0 && a.info.removed == 1, "seen through for the second time: removed");
        check(b.rc == SSM_OK && b.verdict[0] == 1 && b.run[0] == 1 && b.n == 1 && b.run_io[0] == 1 && memcmp(&b.pts[0], &one[0], sizeof(ssm_point)) == 0, "occluded: the counter stays");
        check(c.rc == SSM_OK && c.verdict[0] == 3 && c.n == 1 && c.run_io[0] == 1, "seen through once: kept");
    }
    {   // what must never reach an integer conversion
        const int w = 8, h = 6;
        vector<uint16_t> flat((size_t)w * h, 1000);
        vector<ssm_point> in = {pt(big, 0, 1), pt(-big, 0, 1), pt(0, big, 1), pt(0, -big, 1), pt(0, 0, big), pt(big, big, big), pt(3.0e38f, 3.0e38f, 3.0e38f), pt(nan, 0, 1), pt(0, nan, 1), pt(0, 0, nan),
                                pt(inf, 0, 1), pt(0, -inf, 1), pt(0, 0, inf), pt(0, 0, -inf), pt(0, 0, 0), pt(0, 0, -1), pt(1e-30f, 1e-30f, 1e-38f), pt(0, 0, 1.0e13f), pt(0, 0, 2.0e12f)};
        ssm_carve_params P = D; P.radius = 0;
        Out o = run(flat, w, h, cam, EYE, in, EYE, {}, P);
        check(o.rc == SSM_OK && o.verdict[4] == 1 && o.verdict[17] == 1 && o.verdict[18] == 1 && o.verdict[0] == 0 && o.verdict[7] == 0 && o.verdict[12] == 0, "1e30, NaN, infinity, a depth beyond 2^50 units");
        check(restated(flat, w, h, cam, EYE, in, EYE, {}, P, o), "... as restated");
        double T[16]; memcpy(T, EYE, sizeof T); T[12] = 1e300; T[14] = -1e300;
        Out q = run(flat, w, h, cam, T, in, EYE, {}, P);
        check(q.rc == SSM_OK && restated(flat, w, h, cam, T, in, EYE, {}, P, q), "a pose at 1e300");
    }
    {   // counters at 254 and 255, every min_votes
        const int w = 8, h = 6;
        vector<uint16_t> far((size_t)w * h, 3000);
        vector<ssm_point> in = {at_pixel(1, 1, 1.0f, 1), at_pixel(2, 1, 1.0f, 2), at_pixel(3, 1, 1.0f, 3)};
        bool ok = true;
        for (int mv : {1, 2, 3, 255}) {
            ssm_carve_params P = D; P.min_votes = mv;
            Out o = run(far, w, h, cam, EYE, in, EYE, {253, 254, 255}, P);
            ok = ok && o.rc == SSM_OK && o.run[0] == 254 && o.run[1] == 255 && o.run[2] == 255 && o.n == (mv == 255 ? 1 : 0) && restated(far, w, h, cam, EYE, in, EYE, {253, 254, 255}, P, o);
        }
        check(ok, "counters saturate at 255");
    }
    {   // empty cloud, capacity, invalid arguments
        const int w = 8, h = 6;
        vector<uint16_t> flat((size_t)w * h, 1000);
        Out e = run(flat, w, h, cam, EYE, {}, EYE, {}, D);
        check(e.rc == SSM_OK && e.n == 0 && e.info.n_in == 0 && e.info.n_kept == 0, "a cloud of size 0");
        vector<ssm_point> in; for (int i = 0; i < 20; i++) in.push_back(at_pixel(1 + i % 6, 1 + i % 4, 1.0f, (uint32_t)i));
        Out c = run(flat, w, h, cam, EYE, in, EYE, vector<uint8_t>(20, 1), D, 5);
        check(c.rc == SSM_E_CAPACITY && c.n == 20 && c.run_io == vector<uint8_t>(20, 1) && c.pts[0].x == 7.0f, "capacity: the count needed, nothing written");
        bool ok = true;
        for (int k = 0; k < 12; k++) {
            ssm_carve_params P = D; ssm_camera cm = cam; double T[16]; memcpy(T, EYE, sizeof T);
            switch (k) {
            case 0: P.min_votes = 0; break;   case 1: P.min_votes = 256; break; case 2: P.radius = -1; break; case 3: P.radius = 4; break;
            case 4: P.tol_abs = nan; break;   case 5: P.tol_abs = -1; break;    case 6: P.tol_rel_ppm = -1; break; case 7: P.z_min = nan; break;
            case 8: cm.scale = 0; break;      case 9: cm.fx = inf; break;       case 10: T[13] = nan; break;   default: P.tol_abs = 1e7; break;
            }
            Out o = run(flat, w, h, cm, T, in, EYE, {}, P);
            ok = ok && o.rc == SSM_E_INVAL && !g_err.empty();
        }
        check(ok, "invalid arguments are refused");
    }
    {   // random clouds, views and poses
        Rng g{0x5EED};
        bool ok = true; long long verdicts[4] = {0, 0, 0, 0};
        for (int t = 0; t < 40 && ok; t++) {
            const int w = 20 + (int)(g.next() % 60), h = 9 + (int)(g.next() % 40), n = (int)(g.next() % 700);
            ssm_camera cm; cm.cx = w / 2.0 - 0.25; cm.cy = h / 2.0 + 0.125; cm.fx = cm.fy = 0.9 * w; cm.scale = t % 3 ? 1000.0 : 5000.0;
            vector<uint16_t> depth((size_t)w * h);
            for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) depth[(size_t)y * w + x] = g.next() % 50 == 0 ? 0 : (uint16_t)((1.5 + 0.5 * (x > w / 2) + 0.004 * g.unit()) * cm.scale);
            double Tv[16], Tc[16]; random_pose(g, 0.1, 0.2, Tv); random_pose(g, 0.1, 0.2, Tc);
            vector<ssm_point> in; vector<uint8_t> rn;
            for (int i = 0; i < n; i++) {
                const double z = 0.05 + 3.0 * g.unit(), u = g.unit() * (w + 4) - 2, v = g.unit() * (h + 4) - 2;
                in.push_back(pt((float)((u - cm.cx) * z / cm.fx), (float)((v - cm.cy) * z / cm.fy), (float)(g.next() % 4 ? z : 1.75 + 0.01 * g.unit()), (uint32_t)i));
                rn.push_back((uint8_t)(g.next() % 7 == 0 ? 250 + g.next() % 6 : g.next() % 3));
            }
            ssm_carve_params P = D; P.radius = t % 4; P.min_votes = 1 + t % 3; P.tol_abs = 0.01 * (t % 5); P.tol_rel_ppm = 5000 * (t % 6); P.z_min = 0.1 * (t % 3);
            Out o = run(depth, w, h, cm, Tv, in, Tc, t % 2 ? rn : vector<uint8_t>(), P);
            ok = o.rc == SSM_OK && restated(depth, w, h, cm, Tv, in, Tc, t % 2 ? rn : vector<uint8_t>(), P, o);
            verdicts[0] += o.info.unknown; verdicts[1] += o.info.occluded; verdicts[2] += o.info.supported; verdicts[3] += o.info.seen_through;
        }
        check(ok, "random clouds against the restatement");
        check(verdicts[0] > 100 && verdicts[1] > 100 && verdicts[2] > 100 && verdicts[3] > 100, "... with every verdict in quantity");
    }
    printf(failures ? "%d FAILED\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
