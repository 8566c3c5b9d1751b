// test_align_core.cpp -- dense alignment on the host (csrc/ssm_align_host.cpp over include/ssm/align_core.h) as a stand-alone program: linked with that source and
// csrc/ssm_carve_host.cpp (the pose check), it needs neither libssm_hip.so nor a GPU and runs as it is under the CPU sanitizers (-fsanitize=address,undefined).
// Checked here, from C++: a room corner ray-cast in this file whose planted translation the alignment removes; exact-size buffers (the sanitizer sees any byte
// beyond them); the same clouds reversed and the same points permuted give the same sums, pose and info; a single fronto-parallel plane is DEGENERATE without
// damping, too few inliers TOO_FEW, a bound below the planted error DIVERGED, and in all three the pose comes back as given; points whose conversion to an
// integer would be undefined; invalid arguments, the overflow bound among them.
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
static const double EYE[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
static ssm_point pt(float x, float y, float z) { ssm_point p; memset(&p, 0, sizeof p); p.x = x; p.y = y; p.z = z; p.w = 1.0f; return p; }
static ssm_align_params defaults() { ssm_align_params P; ssm_align_params_default(&P); P.min_inliers = 50; return P; }

static const int W = 67, H = 47;
static ssm_camera cam0() { ssm_camera c; c.cx = 33.2; c.cy = 20.4; c.fx = 52.0; c.fy = 41.0; c.scale = 1000.0; return c; }
// floor y = 1, wall x = -1.5, back wall z = 4 from the identity pose (corner), or the back wall alone (flat)
static vector<uint16_t> cast(bool corner)
{
    const ssm_camera c = cam0(); vector<uint16_t> d((size_t)W * H);
    for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) {
        const double dx = (x - c.cx) / c.fx, dy = (y - c.cy) / c.fy;
        double t = 4.0;
        if (corner) { if (dy > 0 && 1.0 / dy < t) t = 1.0 / dy; if (dx < 0 && -1.5 / dx < t) t = -1.5 / dx; }
        d[(size_t)y * W + x] = (uint16_t)llrint(t * c.scale);
    }
    return d;
}
static vector<ssm_point> back_project(const vector<uint16_t>& d, int step, int phase)
{
    const ssm_camera c = cam0(); vector<ssm_point> p;
    for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) {
        if ((y * W + x) % step != phase) continue;
        const double z = d[(size_t)y * W + x] / c.scale;
        p.push_back(pt((float)((x - c.cx) * z / c.fx), (float)((y - c.cy) * z / c.fy), (float)z));
    }
    return p;
}
struct Out { int rc; double T[16]; ssm_align_info info; vector<uint8_t> valid; vector<float> normals; vector<ssm_align_iter> rec; int nrec; };
static Out run(const vector<uint16_t>& depth, const double* Tv, const vector<vector<ssm_point>>& clouds, const vector<double>& Tc, const ssm_align_params& P)
{
    Out o; memset(&o.info, 0, sizeof o.info); o.nrec = 0;
    o.valid.assign((size_t)W * H, 7); o.normals.assign((size_t)W * H * 4, 7.0f); o.rec.resize((size_t)max(P.max_iterations, 1));
    for (double& v : o.T) v = 7.0;
    vector<const ssm_point*> ptrs; vector<int32_t> n;
    for (const auto& c : clouds) { ptrs.push_back(c.empty() ? nullptr : c.data()); n.push_back((int32_t)c.size()); }
    const ssm_camera cam = cam0();
    o.rc = ssm_align_host(depth.data(), W, H, &cam, Tv, ptrs.empty() ? nullptr : ptrs.data(), n.empty() ? nullptr : n.data(), Tc.empty() ? nullptr : Tc.data(), (int)clouds.size(),
                          &P, o.T, &o.info, o.valid.data(), o.normals.data(), o.rec.data(), (int)o.rec.size(), &o.nrec);
    return o;
}
static vector<double> eyes(size_t m) { vector<double> T; for (size_t k = 0; k < m; k++) T.insert(T.end(), EYE, EYE + 16); return T; }
static bool same(const Out& a, const Out& b)
{
    if (a.rc != b.rc || a.nrec != b.nrec || memcmp(a.T, b.T, sizeof a.T) || memcmp(&a.info, &b.info, sizeof a.info)) return false;
    for (int i = 0; i < a.nrec; i++) if (memcmp(&a.rec[i], &b.rec[i], sizeof(ssm_align_iter))) return false;
    return true;
}

int main()
{
    const vector<uint16_t> corner = cast(true), flat = cast(false);
    double Tv[16]; memcpy(Tv, EYE, sizeof Tv); Tv[12] = 0.02; Tv[13] = -0.015; Tv[14] = 0.025;          // the view believes it stands 3.5 cm away from where it was cast
    const vector<vector<ssm_point>> clouds = {back_project(corner, 2, 0), {}, back_project(corner, 2, 1)};
    const ssm_align_params P = defaults();
    {
        const Out o = run(corner, Tv, clouds, eyes(3), P);
        const double err = sqrt(o.T[12] * o.T[12] + o.T[13] * o.T[13] + o.T[14] * o.T[14]);
        check(o.rc == SSM_OK && (o.info.status == SSM_ALIGN_CONVERGED || o.info.status == SSM_ALIGN_MAX_ITER), "corner: runs to an accepted end");
        check(err < 0.005, "corner: the planted 3.5 cm are removed (" + to_string(err) + " m left)");
        check(o.info.n_in == (int64_t)(clouds[0].size() + clouds[2].size()) && o.info.tested_first > 0 && o.info.inliers_first <= o.info.tested_first &&
              o.info.tested_first <= o.info.n_in && o.nrec == o.info.iterations, "corner: the counts are ordered");
        check(o.info.chi2_last < o.info.chi2_first, "corner: chi2 falls");
        bool border = true; size_t nvalid = 0;
        for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) {
            const size_t at = (size_t)y * W + x; const float* n = &o.normals[at * 4];
            const bool zero = n[0] == 0 && n[1] == 0 && n[2] == 0;
            if (x == 0 || y == 0 || x == W - 1 || y == H - 1) border = border && !o.valid[at];
            border = border && (o.valid[at] == (zero ? 0 : 1)) && n[3] == 0.0f;
            nvalid += o.valid[at];
        }
        check(border && nvalid > 1000, "corner: the border is invalid, valid == a non-zero normal");
        // order independence
        const Out r = run(corner, Tv, {clouds[2], clouds[1], clouds[0]}, eyes(3), P);
        check(same(o, r), "the clouds reversed: identical sums, pose and info");
        vector<ssm_point> all = clouds[0]; all.insert(all.end(), clouds[2].begin(), clouds[2].end());
        const Out one = run(corner, Tv, {all}, eyes(1), P);
        vector<ssm_point> perm = all; for (size_t i = 0; i < perm.size(); i++) swap(perm[i], perm[(i * 7919 + 13) % perm.size()]);
        check(same(one, run(corner, Tv, {perm}, eyes(1), P)) && same(one, o), "the points permuted and concatenated: identical");
        ssm_align_params S3 = P; S3.stride = 3;
        const Out s3 = run(corner, Tv, {all}, eyes(1), S3);
        check(s3.rc == SSM_OK && s3.info.n_in == (int64_t)((all.size() + 2) / 3), "stride 3 uses every third point");
    }
    {   // statuses that give the pose back
        ssm_align_params D = P; D.damping = 0.0;
        const Out d = run(flat, Tv, {back_project(flat, 1, 0)}, eyes(1), D);
        check(d.rc == SSM_OK && d.info.status == SSM_ALIGN_DEGENERATE && !memcmp(d.T, Tv, sizeof Tv) && !memcmp(d.info.E, EYE, sizeof EYE), "one fronto-parallel plane, no damping: DEGENERATE, pose as given");
        ssm_align_params F = P; F.min_inliers = 1 << 30;
        const Out f = run(corner, Tv, clouds, eyes(3), F);
        check(f.rc == SSM_OK && f.info.status == SSM_ALIGN_TOO_FEW && f.info.iterations == 1 && !memcmp(f.T, Tv, sizeof Tv), "min_inliers above the count: TOO_FEW, pose as given");
        ssm_align_params V = P; V.max_shift = 0.01;
        const Out v = run(corner, Tv, clouds, eyes(3), V);
        check(v.rc == SSM_OK && v.info.status == SSM_ALIGN_DIVERGED && !memcmp(v.T, Tv, sizeof Tv) && !memcmp(v.info.E, EYE, sizeof EYE), "max_shift below the planted error: DIVERGED, pose as given");
        ssm_align_params M1 = P; M1.max_iterations = 1;
        const Out m1 = run(corner, Tv, clouds, eyes(3), M1);
        check(m1.rc == SSM_OK && m1.info.status == SSM_ALIGN_MAX_ITER && m1.info.iterations == 1 && memcmp(m1.T, Tv, sizeof Tv), "max_iterations 1: one step is applied");
        const Out none = run(corner, Tv, {}, {}, P);
        check(none.rc == SSM_OK && none.info.status == SSM_ALIGN_TOO_FEW && none.info.n_in == 0, "no cloud at all");
    }
    {   // inputs whose conversion to an integer would be undefined
        const float big = 1.0e30f, nan = numeric_limits<float>::quiet_NaN(), inf = numeric_limits<float>::infinity();
        vector<ssm_point> bad = {pt(nan, 0, 1), pt(0, inf, 1), pt(0, 0, -inf), pt(big, 0, 1), pt(-big, -big, 1), pt(0, 0, big), pt(3e38f, 3e38f, 3e38f), pt(0, 0, 0), pt(0, 0, -1), pt(1e-30f, 1e-30f, 1e-38f)};
        const Out o = run(corner, Tv, {bad}, eyes(1), P);
        check(o.rc == SSM_OK && o.info.tested_first == 0 && o.info.status == SSM_ALIGN_TOO_FEW, "non-finite and huge points reach no pixel");
    }
    {   // refusals
        const double nan = numeric_limits<double>::quiet_NaN(), inf = numeric_limits<double>::infinity();
        auto refused = [&](ssm_align_params Q) { return run(corner, Tv, clouds, eyes(3), Q).rc == SSM_E_INVAL; };
        bool all = true;
        { ssm_align_params Q = P; Q.max_iterations = 0; all = all && refused(Q); Q.max_iterations = 65; all = all && refused(Q); }
        { ssm_align_params Q = P; Q.stride = 0; all = all && refused(Q); }
        { ssm_align_params Q = P; Q.min_inliers = -1; all = all && refused(Q); }
        for (double bad : {-1.0, nan, inf}) {
            double ssm_align_params::* fields[] = {&ssm_align_params::z_min, &ssm_align_params::z_max, &ssm_align_params::dist_max, &ssm_align_params::delta, &ssm_align_params::damping,
                                                   &ssm_align_params::eps_rot, &ssm_align_params::eps_trans, &ssm_align_params::max_shift, &ssm_align_params::max_angle, &ssm_align_params::tol_abs};
            for (auto f : fields) { ssm_align_params Q = P; Q.*f = bad; all = all && refused(Q); }
        }
        { ssm_align_params Q = P; Q.z_max = 0.05; all = all && refused(Q); }
        { ssm_align_params Q = P; Q.max_angle = 3.2; all = all && refused(Q); }
        { ssm_align_params Q = P; Q.tol_rel_ppm = -1; all = all && refused(Q); Q.tol_rel_ppm = 1000001; all = all && refused(Q); }
        check(all, "every bad parameter is refused");
        ssm_align_params Q = P; Q.z_max = 1.0e9;
        check(refused(Q), "z_max = 1e9: the sums could pass 2^62, refused");
        double Tb[16]; memcpy(Tb, Tv, sizeof Tb); Tb[13] = nan;
        check(run(corner, Tb, clouds, eyes(3), P).rc == SSM_E_INVAL, "a non-finite view pose");
        vector<double> Tc = eyes(3); Tc[16 + 5] = inf;
        check(run(corner, Tv, clouds, Tc, P).rc == SSM_E_INVAL, "a non-finite cloud pose");
        check(run(corner, Tv, {clouds[0], clouds[0]}, eyes(2), P).rc == SSM_OK, "equal clouds in different arrays are two clouds");
        const ssm_camera cam = cam0(); const ssm_point* two[2] = {clouds[0].data(), clouds[0].data()}; const int32_t n2[2] = {5, 5}, nneg[2] = {5, -1};
        const vector<double> T2 = eyes(2); double To[16];
        check(ssm_align_host(corner.data(), W, H, &cam, Tv, two, n2, T2.data(), 2, &P, To, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == SSM_E_INVAL, "the same cloud twice");
        check(ssm_align_host(corner.data(), W, H, &cam, Tv, two, nneg, T2.data(), 2, &P, To, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == SSM_E_INVAL, "a negative count");
        check(ssm_align_host(corner.data(), W, H, &cam, Tv, two, n2, T2.data(), -1, &P, To, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == SSM_E_INVAL, "m < 0");
        check(ssm_align_host(corner.data(), 2, H, &cam, Tv, two, n2, T2.data(), 0, &P, To, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == SSM_E_INVAL, "a view of width 2");
        ssm_camera c0 = cam; c0.fx = 0.0;
        check(ssm_align_host(corner.data(), W, H, &c0, Tv, two, n2, T2.data(), 1, &P, To, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == SSM_E_INVAL, "fx = 0 has no bound");
        ssm_camera cs = cam; cs.scale = 0.0;
        check(ssm_align_host(corner.data(), W, H, &cs, Tv, two, n2, T2.data(), 1, &P, To, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == SSM_E_INVAL, "scale = 0");
        ssm_align_iter one;
        check(ssm_align_host(corner.data(), W, H, &cam, Tv, two, n2, T2.data(), 1, &P, To, nullptr, nullptr, nullptr, &one, 1, nullptr) == SSM_OK, "a record of one entry holds the one iteration of TOO_FEW");
    }
    printf(failures ? "FAILED (%d)\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
