// test_render_core.cpp -- map rendering on the host (csrc/ssm_render_host.cpp over include/ssm/render_core.h) as a stand-alone program: linked with that source
// and csrc/ssm_carve_host.cpp (the pose check), it needs neither libssm_hip.so nor a GPU and runs as it is under the CPU sanitizers (-fsanitize=address,undefined).
// Checked here, from C++: the case list of DESIGN.md s.17 with known outcomes (two depths on one pixel, equal depths in both orders, zq at 1 and 65535 and just
// outside, z_min / z_max, the inputs whose conversion to an integer would be undefined, centres outside the image, every half width, three clouds of sizes 5, 0
// and 7, no cloud at all), exact-size buffers (the sanitizer sees any byte beyond them), invalid arguments, the comparison's eight categories at +-tol, and
// random clouds under random poses against a restatement of the section written out here.
#include "ssm_hip.h"
#include <algorithm>
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

static ssm_point pt(float x, float y, float z, uint32_t tag = 0)
{ ssm_point p; memset(&p, 0, sizeof p); p.x = x; p.y = y; p.z = z; p.w = 1.0f; p.b = (uint8_t)(tag * 7 + 1); p.g = (uint8_t)(tag * 5 + 2); p.r = (uint8_t)(tag * 3 + 3); p.a = 9; p.label = tag | 0xABCD00u; p.pad[1] = ~tag; return p; }
static const double EYE[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
static ssm_camera cam0(double scale = 1000) { ssm_camera c; c.cx = 0; c.cy = 0; c.fx = 64; c.fy = 64; c.scale = scale; return c; }
static ssm_point at_pixel(double px, double py, float z, uint32_t tag = 0) { return pt((float)(px * z / 64.0), (float)(py * z / 64.0), z, tag); }
static ssm_render_params defaults() { ssm_render_params P; ssm_render_params_default(&P); return P; }

struct Out { vector<uint16_t> depth; vector<uint8_t> bgr, label; vector<int32_t> index; vector<uint64_t> keys; ssm_render_info info; int rc; };
// buffers of exactly the sizes the call may touch
static Out run(int w, int h, const ssm_camera& cam, const double* Tv, const vector<vector<ssm_point>>& clouds, const vector<double>& Tc, const ssm_render_params& P)
{
    Out o; const size_t np = (size_t)max(w, 0) * max(h, 0);
    o.depth.assign(np, 7); o.bgr.assign(np * 3, 7); o.label.assign(np, 7); o.index.assign(np, 7); o.keys.assign(np, 7); memset(&o.info, 0, sizeof o.info);
    vector<const ssm_point*> ptrs; vector<int32_t> n;
    for (const auto& c : clouds) { ptrs.push_back(c.empty() ? nullptr : c.data()); n.push_back((int32_t)c.size()); }
    o.rc = ssm_render_host(w, h, &cam, Tv, ptrs.empty() ? nullptr : ptrs.data(), n.empty() ? nullptr : n.data(), Tc.empty() ? nullptr : Tc.data(), (int)clouds.size(), &P,
                           np ? o.depth.data() : nullptr, np ? o.bgr.data() : nullptr, np ? o.label.data() : nullptr, np ? o.index.data() : nullptr, np ? o.keys.data() : nullptr, &o.info);
    return o;
}
static vector<double> eyes(size_t m) { vector<double> T; for (size_t k = 0; k < m; k++) T.insert(T.end(), EYE, EYE + 16); return T; }
static Out run1(int w, int h, const ssm_camera& cam, const vector<ssm_point>& pts, const ssm_render_params& P) { return run(w, h, cam, EYE, {pts}, eyes(1), P); }

// the restatement of s.17: long arithmetic written out, no call into the header
static void rel(const double* Tv, const double* Tc, double M[3][4])
{
    for (int i = 0; i < 3; i++) {
        const double a = Tv[i * 4], b = Tv[i * 4 + 1], c = Tv[i * 4 + 2];
        const double ti = -((a * Tv[12] + b * Tv[13]) + c * Tv[14]);
        for (int j = 0; j < 3; j++) M[i][j] = (a * Tc[j * 4] + b * Tc[j * 4 + 1]) + c * Tc[j * 4 + 2];
        M[i][3] = ((a * Tc[12] + b * Tc[13]) + c * Tc[14]) + ti;
    }
}
static bool restated(int w, int h, const ssm_camera& cam, const double* Tv, const vector<vector<ssm_point>>& clouds, const vector<double>& Tc, const ssm_render_params& P, const Out& o)
{
    const size_t np = (size_t)w * h;
    vector<uint64_t> keys(np, ~(uint64_t)0); vector<ssm_point> all;
    int visible = 0;
    for (size_t k = 0; k < clouds.size(); k++) {
        double M[3][4]; rel(Tv, &Tc[16 * k], M);
        for (const ssm_point& p : clouds[k]) {
            const uint64_t idx = all.size(); all.push_back(p);
            const double x = p.x, y = p.y, z = p.z;
            if (!(isfinite(x) && isfinite(y) && isfinite(z))) continue;
            const double qx = M[0][0] * x + M[0][1] * y + M[0][2] * z + M[0][3], qy = M[1][0] * x + M[1][1] * y + M[1][2] * z + M[1][3], qz = M[2][0] * x + M[2][1] * y + M[2][2] * z + M[2][3];
            if (!(isfinite(qx) && isfinite(qy) && isfinite(qz)) || qz < P.z_min || qz > P.z_max) continue;
            const double pxd = floor(cam.fx * (qx / qz) + cam.cx + 0.5), pyd = floor(cam.fy * (qy / qz) + cam.cy + 0.5), R = P.max_radius;
            if (!(pxd >= -R && pxd <= w - 1 + R && pyd >= -R && pyd <= h - 1 + R)) continue;
            const double zs = qz * cam.scale;
            if (!(zs < 70000.0)) continue;
            const long long zq = llrint(zs);
            if (zq < 1 || zq > 65535) continue;
            long long s = 0;
            if (P.point_size > 0) { const double t = ((0.5 * cam.fx) * P.point_size) / qz; s = t >= R ? P.max_radius : t >= 1 ? (long long)floor(t) : 0; }
            const long long px = (long long)pxd, py = (long long)pyd;
            bool hit = false;
            for (long long yy = max(py - s, 0LL); yy <= min(py + s, (long long)h - 1); yy++) for (long long xx = max(px - s, 0LL); xx <= min(px + s, (long long)w - 1); xx++) {
                hit = true; uint64_t& a = keys[(size_t)yy * w + xx]; a = min(a, ((uint64_t)zq << 32) | idx);
            }
            visible += hit;
        }
    }
    int covered = 0;
    for (size_t i = 0; i < np; i++) {
        if (o.keys[i] != keys[i]) return false;
        if (keys[i] == ~(uint64_t)0) { if (o.depth[i] != 0 || o.label[i] != 255 || o.index[i] != -1 || o.bgr[3 * i] || o.bgr[3 * i + 1] || o.bgr[3 * i + 2]) return false; continue; }
        covered++;
        const ssm_point& p = all[(uint32_t)keys[i]];
        if (o.depth[i] != (uint16_t)(keys[i] >> 32) || o.index[i] != (int32_t)(uint32_t)keys[i] || o.label[i] != (uint8_t)(p.label & 255) || o.bgr[3 * i] != p.b || o.bgr[3 * i + 1] != p.g || o.bgr[3 * i + 2] != p.r) return false;
    }
    return o.info.n_in == (int)all.size() && o.info.n_visible == visible && o.info.n_covered == covered;
}
static void random_pose(Rng& r, double rot, double trans, double T[16])
{
    const double a[3] = {(r.unit() - 0.5) * rot, (r.unit() - 0.5) * rot, (r.unit() - 0.5) * rot};
    const double th = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), s = th > 1e-12 ? sin(th) / th : 1.0, c = th > 1e-12 ? (1 - cos(th)) / (th * th) : 0.5;
    const double K[3][3] = {{0, -a[2], a[1]}, {a[2], 0, -a[0]}, {-a[1], a[0], 0}};
    memset(T, 0, 16 * sizeof(double)); T[15] = 1;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) {
        double kk = 0; for (int l = 0; l < 3; l++) kk += K[i][l] * K[l][j];
        T[j * 4 + i] = (i == j) + s * K[i][j] + c * kk;
    }
    for (int i = 0; i < 3; i++) T[12 + i] = (r.unit() - 0.5) * trans;
}

int main()
{
    const float nanf_ = numeric_limits<float>::quiet_NaN(), inff = numeric_limits<float>::infinity();
    const double nan_ = numeric_limits<double>::quiet_NaN(), inf_ = numeric_limits<double>::infinity();
    ssm_render_params P = defaults();
    check(P.point_size == 0 && P.max_radius == 3 && P.z_min == 0.1 && P.z_max == 1e9 && P.tol_abs == 0.05 && P.tol_rel_ppm == 20000, "defaults");
    {   // two depths on one pixel; equal depths in both orders
        vector<ssm_point> pts = {at_pixel(4, 3, 2.0f, 1), at_pixel(4, 3, 1.0f, 2), at_pixel(4, 3, 3.0f, 3)};
        Out o = run1(9, 7, cam0(), pts, P);
        check(o.rc == 0 && o.depth[3 * 9 + 4] == 1000 && o.index[3 * 9 + 4] == 1 && o.label[3 * 9 + 4] == 2 && o.info.n_visible == 3 && o.info.n_covered == 1 && restated(9, 7, cam0(), EYE, {pts}, eyes(1), P, o), "nearest wins");
        vector<ssm_point> eq = {at_pixel(4, 3, 1.0f, 1), at_pixel(4, 3, 1.0002f, 2), at_pixel(4, 3, 0.9998f, 3)}, rv(eq.rbegin(), eq.rend());
        Out a = run1(9, 7, cam0(), eq, P), b = run1(9, 7, cam0(), rv, P);
        check(a.index[31] == 0 && b.index[31] == 0 && a.label[31] == 1 && b.label[31] == 3 && a.depth[31] == 1000 && b.depth[31] == 1000, "equal depth: the lowest index wins, in either order");
    }
    {   // zq at 1 and 65535 and just outside (scale 1), z_min and z_max
        ssm_render_params Q = P; Q.z_min = 0;
        const float zs[] = {0.5f, 1.0f, 1.5f, 65535.0f, 65535.25f, 65535.5f, 65536.0f, 70000.0f};
        vector<ssm_point> pts; for (int i = 0; i < 8; i++) pts.push_back(at_pixel(3 + 7 * i, 2, zs[i], (uint32_t)i));
        Out o = run1(67, 5, cam0(1.0), pts, Q);
        const int want[] = {0, 1, 2, 65535, 65535, 0, 0, 0};
        bool ok = o.rc == 0 && o.info.n_visible == 4;
        for (int i = 0; i < 8; i++) ok = ok && o.depth[2 * 67 + 3 + 7 * i] == want[i];
        check(ok && restated(67, 5, cam0(1.0), EYE, {pts}, eyes(1), Q, o), "zq limits");
        Q = P; Q.z_min = 1.0; Q.z_max = 2.0;
        vector<ssm_point> zr = {at_pixel(3, 2, 1.0f), at_pixel(10, 2, nextafterf(1.0f, 0.0f)), at_pixel(17, 2, 2.0f), at_pixel(24, 2, nextafterf(2.0f, 3.0f))};
        o = run1(67, 5, cam0(), zr, Q);
        check(o.rc == 0 && o.depth[2 * 67 + 3] == 1000 && o.depth[2 * 67 + 10] == 0 && o.depth[2 * 67 + 17] == 2000 && o.depth[2 * 67 + 24] == 0 && o.info.n_visible == 2, "z_min and z_max are inside");
    }
    {   // inputs whose conversion to an integer would be undefined
        const float big = 1.0e30f;
        vector<ssm_point> pts = {pt(0, 0, -1), pt(0.01f, 0.01f, -0.5f), pt(0, 0, 0), pt(nanf_, 0, 1), pt(0, nanf_, 1), pt(0, 0, nanf_), pt(inff, 0, 1), pt(0, -inff, 1), pt(0, 0, inff), pt(0, 0, -inff),
                                 pt(big, 0, 1), pt(0, -big, 1), pt(0, 0, big), pt(big, big, big), pt(3.0e38f, 3.0e38f, 3.0e38f), pt(1e-30f, 1e-30f, 1e-38f), at_pixel(3, 3, 1.0f, 5)};
        ssm_render_params Q = P; Q.point_size = 0.1; Q.max_radius = 8;
        Out o = run1(9, 7, cam0(), pts, Q);
        check(o.rc == 0 && o.info.n_visible == 1 && o.info.n_in == 17 && restated(9, 7, cam0(), EYE, {pts}, eyes(1), Q, o), "degenerate points are invisible");
        Q.z_min = 0; Q.z_max = 1e9;
        ssm_camera c = cam0(1e6); c.fx = -1e300; c.cx = 1e300;
        o = run1(9, 7, c, pts, Q);
        check(o.rc == 0 && restated(9, 7, c, EYE, {pts}, eyes(1), Q, o), "an absurd camera");
    }
    {   // centres outside the image; every half width
        ssm_render_params Q = P; Q.point_size = 0.0625; Q.max_radius = 2;          // t = 2 / z
        for (auto wh : {make_pair(9, 7), make_pair(67, 5)}) {
            const int w = wh.first, h = wh.second;
            vector<ssm_point> pts;
            for (float z : {1.0f, 2.0f}) for (int o = 1; o <= 3; o++) for (auto xy : {make_pair(-o, 2), make_pair(w - 1 + o, 2), make_pair(w / 2, -o), make_pair(w / 2, h - 1 + o), make_pair(-o, -o), make_pair(w - 1 + o, h - 1 + o)})
                pts.push_back(at_pixel(xy.first, xy.second, z, (uint32_t)pts.size()));
            Out o = run1(w, h, cam0(), pts, Q);
            check(o.rc == 0 && o.info.n_visible == 18 && o.depth[2 * w] == 1000 && o.depth[2 * w + w - 1] == 1000 && o.depth[w / 2] == 1000 && o.depth[(h - 1) * w + w / 2] == 1000 && o.depth[0] == 1000 &&
                  o.depth[(size_t)w * h - 1] == 1000 && restated(w, h, cam0(), EYE, {pts}, eyes(1), Q, o), "footprints reach in from outside " + to_string(w) + "x" + to_string(h));
        }
        for (int R : {0, 3, 8}) {
            Q = P; Q.point_size = 0.125; Q.max_radius = R;          // t = 4 / z
            const float zs[] = {8.0f, 4.0f, 2.5f, 2.0f, 1.0f, 0.4f}; const int want[] = {0, 1, 1, 2, 4, 10};
            vector<ssm_point> pts; for (int i = 0; i < 6; i++) pts.push_back(at_pixel(5 + 11 * i, 2, zs[i], (uint32_t)i));
            Out o = run1(67, 5, cam0(), pts, Q);
            bool ok = o.rc == 0;
            for (int i = 0; i < 6 && R <= 3; i++) { const int s = min(want[i], R);          // (under 8 the last two splats overlap and the last is clipped: the restatement alone)
                int row = 0; for (int x = 0; x < 67; x++) row += o.index[2 * 67 + x] == i; ok = ok && row == min(2 * s + 1, 67); }
            check(ok && restated(67, 5, cam0(), EYE, {pts}, eyes(1), Q, o), "half widths under max_radius " + to_string(R));
        }
    }
    {   // three clouds of sizes 5, 0 and 7; none at all; one empty
        Rng r{7};
        vector<vector<ssm_point>> cl(3);
        for (int i = 0; i < 5; i++) cl[0].push_back(at_pixel(r.next() % 9, r.next() % 7, 1.0f + 0.25f * (r.next() % 4), (uint32_t)i));
        for (int i = 0; i < 7; i++) cl[2].push_back(at_pixel(r.next() % 9, r.next() % 7, 1.0f + 0.25f * (r.next() % 4), (uint32_t)(5 + i)));
        ssm_render_params Q = P; Q.point_size = 0.04;
        Out o = run(9, 7, cam0(), EYE, cl, eyes(3), Q);
        check(o.rc == 0 && o.info.n_in == 12 && restated(9, 7, cam0(), EYE, cl, eyes(3), Q, o), "clouds of sizes 5, 0, 7");
        o = run(9, 7, cam0(), EYE, {}, {}, P);
        check(o.rc == 0 && o.info.n_in == 0 && o.info.n_covered == 0 && restated(9, 7, cam0(), EYE, {}, {}, P, o), "no cloud");
        o = run(9, 7, cam0(), EYE, {{}}, eyes(1), P);
        check(o.rc == 0 && o.info.n_in == 0 && restated(9, 7, cam0(), EYE, {{}}, eyes(1), P, o), "one empty cloud");
        check(ssm_render_host(9, 7, nullptr, EYE, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SSM_E_INVAL, "a null camera");
        ssm_camera c = cam0();
        check(ssm_render_host(9, 7, &c, EYE, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SSM_OK, "every output may be NULL");
    }
    {   // random clouds under random poses
        Rng r{99};
        bool ok = true; int covered = 0;
        for (int it = 0; it < 40; it++) {
            const int w = it % 2 ? 67 : 23, h = it % 2 ? 5 : 17, m = 1 + it % 3;
            ssm_camera c; c.cx = w / 2.0 - 0.3; c.cy = h / 2.0 + 0.2; c.fx = 0.9 * w; c.fy = 0.8 * w; c.scale = it % 5 == 0 ? 5000 : 1000;
            vector<vector<ssm_point>> cl(m); vector<double> Tc(16 * m); double Tv[16];
            random_pose(r, 0.2, 0.3, Tv);
            for (int k = 0; k < m; k++) {
                random_pose(r, 0.2, 0.3, &Tc[16 * k]);
                const int n = (int)(r.next() % 300);
                for (int i = 0; i < n; i++) { const float z = (float)(0.05 + 6.0 * r.unit()); cl[k].push_back(pt((float)((r.unit() - 0.5) * 1.6 * z), (float)((r.unit() - 0.5) * 1.2 * z), z, r.next())); }
            }
            ssm_render_params Q = P; Q.point_size = it % 4 == 0 ? 0 : 0.02 * (it % 7); Q.max_radius = it % 9; Q.z_min = 0.1 * (it % 3); Q.z_max = it % 6 == 0 ? 3.0 : 1e9;
            Out o = run(w, h, c, Tv, cl, Tc, Q);
            ok = ok && o.rc == 0 && restated(w, h, c, Tv, cl, Tc, Q, o);
            covered += o.info.n_covered;
        }
        check(ok && covered > 1000, "random clouds equal the restatement");
    }
    {   // refusals
        const vector<ssm_point> pts = {at_pixel(4, 3, 1.0f)};
        auto bad = [&](ssm_render_params Q, ssm_camera c = cam0(), int w = 9, int h = 7) { return run1(w, h, c, pts, Q).rc == SSM_E_INVAL; };
        bool ok = true;
        ssm_render_params Q;
        Q = P; Q.max_radius = -1; ok = ok && bad(Q); Q = P; Q.max_radius = 9; ok = ok && bad(Q);
        for (double v : {-0.1, nan_, inf_}) { Q = P; Q.point_size = v; ok = ok && bad(Q); Q = P; Q.z_min = v; ok = ok && bad(Q); Q = P; Q.z_max = v; ok = ok && bad(Q); Q = P; Q.tol_abs = v; ok = ok && bad(Q); }
        Q = P; Q.tol_abs = 2e6; ok = ok && bad(Q); Q = P; Q.tol_rel_ppm = -1; ok = ok && bad(Q); Q = P; Q.tol_rel_ppm = 1000001; ok = ok && bad(Q);
        check(ok, "parameters out of range are refused");
        ok = true;
        for (double s : {0.0, -1.0, nan_, 2e6}) ok = ok && bad(P, cam0(s));
        { ssm_camera c = cam0(); c.fx = nan_; ok = ok && bad(P, c); c = cam0(); c.cy = inf_; ok = ok && bad(P, c); }
        ok = ok && bad(P, cam0(), 0, 7) && bad(P, cam0(), 9, 0) && bad(P, cam0(), -3, 7);
        check(ok, "cameras and sizes out of range are refused");
        ssm_camera c = cam0(); double T[16]; memcpy(T, EYE, sizeof T); T[13] = nan_;
        const ssm_point* pp = pts.data(); int32_t n1 = 1, neg = -1, big[3] = {2147483647, 2147483647, 2}; const ssm_point* p3[3] = {pp, pp, pp}; const vector<double> T3 = eyes(3);
        auto call = [&](const double* Tv, const ssm_point* const* p, const int32_t* n, const double* Tc, int m) { return ssm_render_host(9, 7, &c, Tv, p, n, Tc, m, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr); };
        check(call(EYE, &pp, &n1, EYE, 1) == SSM_OK && call(T, &pp, &n1, EYE, 1) == SSM_E_INVAL && call(EYE, &pp, &n1, T, 1) == SSM_E_INVAL && call(nullptr, &pp, &n1, EYE, 1) == SSM_E_INVAL &&
              call(EYE, &pp, &n1, EYE, -1) == SSM_E_INVAL && call(EYE, nullptr, &n1, EYE, 1) == SSM_E_INVAL && call(EYE, &pp, nullptr, EYE, 1) == SSM_E_INVAL && call(EYE, &pp, &n1, nullptr, 1) == SSM_E_INVAL &&
              call(EYE, &pp, &neg, EYE, 1) == SSM_E_INVAL && call(EYE, p3, big, T3.data(), 3) == SSM_E_INVAL, "poses, null arguments, m < 0 and 2^32 points are refused");
        ssm_camera huge = cam0();
        check(ssm_render_host(8192, 8193, &huge, EYE, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SSM_E_INVAL, "more than 2^26 pixels are refused");
    }
    {   // the comparison: zr = 1000 everywhere but the last three columns; d walks through +-tol (default tolerance 50 + d / 50)
        const int w = 67, h = 2; const size_t np = (size_t)w * h;
        vector<uint16_t> zr(np, 1000), d(np, 1000); vector<uint8_t> lr(np, 4), sem(np * 3), cls(np, 9);
        for (size_t i = 0; i < np; i++) { sem[3 * i] = 128; sem[3 * i + 1] = 64; sem[3 * i + 2] = 128; }          // road = 4
        for (int y = 0; y < h; y++) for (int x = 64; x < w; x++) zr[(size_t)y * w + x] = 0;
        const uint16_t dv[] = {1071, 1072, 1073, 932, 931, 930, 0, 65535, 1};
        for (int i = 0; i < 9; i++) d[i] = dv[i];
        const uint8_t want[] = {4, 2, 2, 4, 3, 3, 1, 2, 3};
        lr[10] = 5; lr[11] = 255; sem[3 * 12] = 1; lr[13] = 255; sem[3 * 13] = 1; lr[14] = 44; lr[15] = 12;         // disagree; unknown on either side and on both; a label that is no class
        ssm_render_compare_info I; memset(&I, 0, sizeof I);
        const int rc = ssm_render_compare_host(zr.data(), lr.data(), w, h, d.data(), sem.data(), 1000.0, nullptr, &I, cls.data());
        bool ok = rc == 0;
        for (int i = 0; i < 9; i++) ok = ok && cls[i] == want[i];
        ok = ok && I.n_pixels == (int64_t)np && I.unrendered == 6 && I.no_depth == 1 && I.in_front == 3 && I.behind == 3 && I.agree == (int64_t)np - 13;
        ok = ok && I.label_disagree == 3 && I.label_unknown == 3 && I.label_agree == I.agree - 6;          // (44 and 12 against road: both "known" bytes, different)
        check(ok, "the comparison's eight categories at +-tol");
        ssm_render_params Q = defaults(); Q.tol_abs = 0; Q.tol_rel_ppm = 0;
        check(ssm_render_compare_host(zr.data(), lr.data(), w, h, d.data(), sem.data(), 1000.0, &Q, &I, nullptr) == 0 && I.agree == (int64_t)np - 6 - 9 && I.in_front == 4 && I.behind == 4, "zero tolerance");
        Q = defaults(); Q.tol_abs = -1;
        check(ssm_render_compare_host(zr.data(), lr.data(), w, h, d.data(), sem.data(), 1000.0, &Q, &I, nullptr) == SSM_E_INVAL && ssm_render_compare_host(zr.data(), lr.data(), w, h, d.data(), sem.data(), 0.0, nullptr, &I, nullptr) == SSM_E_INVAL &&
              ssm_render_compare_host(nullptr, lr.data(), w, h, d.data(), sem.data(), 1000.0, nullptr, &I, nullptr) == SSM_E_INVAL && ssm_render_compare_host(zr.data(), lr.data(), 0, h, d.data(), sem.data(), 1000.0, nullptr, &I, nullptr) == SSM_E_INVAL,
              "the comparison's refusals");
        uint8_t lab[4] = {0, 11, 12, 255}, col[12];
        ssm_render_label_colours(lab, 4, col);
        check(col[0] == 128 && col[1] == 128 && col[2] == 128 && col[3] == 192 && col[4] == 128 && col[5] == 0 && !col[6] && !col[7] && !col[8] && !col[9] && !col[10] && !col[11], "palette colours");
    }
    printf(failures ? "%d FAILED\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
