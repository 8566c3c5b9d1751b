// test_sor_core.cpp -- the statistical outlier removal on the host (csrc/ssm_sor_host.cpp over include/ssm/sor_core.h) as a stand-alone program: linked with that
// one source, it needs neither libssm_hip.so nor a GPU and runs as it is under the CPU sanitizers (-fsanitize=address,undefined).
// Checked here, from C++: hand-made clouds with known figures, the ladder's edges (too few points, non-finite points, duplicates, one cell, a raised first
// cell size), invalid arguments, and random clouds under several first cell sizes against a restatement by all pairs and a full sort.
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
struct Rng { uint64_t s; uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); } float unit() { return (float)(next() % 100000) / 100000.0f; } };

static ssm_point pt(float x, float y, float z, uint32_t tag = 0) { ssm_point p; memset(&p, 0, sizeof p); p.x = x; p.y = y; p.z = z; p.w = 1.0f; p.label = tag; p.pad[1] = ~tag; return p; }
struct Out { vector<ssm_point> pts; vector<float> md; vector<uint8_t> keep; ssm_sor_info info; int rc, n; };
static Out run(const vector<ssm_point>& in, int k, double mul, float cell)
{
    Out o; const int n = (int)in.size();
    o.pts.assign((size_t)n + 1, pt(7, 7, 7)); o.md.assign((size_t)n + 1, 7.0f); o.keep.assign((size_t)n + 1, 7); o.n = -1;
    ssm_sor_params P; ssm_sor_params_default(&P); P.mean_k = k; P.stddev_mul = mul; P.cell = cell;
    o.rc = ssm_sor_filter_host(in.data(), n, &P, o.pts.data(), n, &o.n, &o.info, o.md.data(), o.keep.data());
    return o;
}
// the restatement: all pairs, a full sort per point, the sums in plain integers
static bool restated(const vector<ssm_point>& in, int k, double mul, const Out& o)
{
    const int n = (int)in.size();
    vector<int> fin;
    for (int i = 0; i < n; i++) if (std::isfinite(in[i].x) && std::isfinite(in[i].y) && std::isfinite(in[i].z)) fin.push_back(i);
    vector<float> md((size_t)n, 0.0f); vector<uint8_t> keep((size_t)n, 0);
    ssm_sor_info I; memset(&I, 0, sizeof I); I.n_in = n; I.n_finite = (int)fin.size();
    if ((int)fin.size() < k + 1) { I.too_few = 1; for (int i : fin) keep[i] = 1; }
    else {
        vector<float> d2;
        for (int i : fin) {
            d2.clear();
            for (int j : fin) if (j != i) { const float dx = in[i].x - in[j].x, dy = in[i].y - in[j].y, dz = in[i].z - in[j].z; d2.push_back((dx * dx + dy * dy) + dz * dz); }
            sort(d2.begin(), d2.end());
            double s = 0.0;
            for (int t = 0; t < k; t++) s += sqrt((double)d2[t]);
            md[i] = (float)(s / (double)k);
        }
        unsigned __int128 s1 = 0, s2 = 0;
        for (int i : fin) { const uint64_t q = (uint64_t)llrint((double)md[i] * 1048576.0); s1 += q; s2 += (unsigned __int128)q * q; I.sum_q += q; I.sum_q2_lo += (q * q) & 0xFFFFFFFFull; I.sum_q2_hi += (q * q) >> 32; }
        if (((unsigned __int128)I.sum_q2_hi << 32) + I.sum_q2_lo != s2 || I.sum_q != s1) return false;
        const double N = (double)fin.size(), a = (double)I.sum_q / 1048576.0, b = ((double)I.sum_q2_hi * 4294967296.0 + (double)I.sum_q2_lo) / 1048576.0 / 1048576.0;
        I.mean = a / N;
        const double var = (b - a * a / N) / (N - 1.0);
        I.stddev = sqrt(var > 0.0 ? var : 0.0);
        I.threshold = I.mean + mul * I.stddev;
        for (int i : fin) keep[i] = (double)md[i] <= I.threshold;
    }
    vector<ssm_point> kept;
    for (int i = 0; i < n; i++) if (keep[i]) { kept.push_back(in[i]); I.n_kept++; }
    I.levels = o.info.levels;          // the search's own figure: a restatement without a grid has none
    if (o.rc != SSM_OK || o.n != I.n_kept || memcmp(&I, &o.info, sizeof I) != 0) return false;
    if (n && (memcmp(md.data(), o.md.data(), (size_t)n * 4) != 0 || memcmp(keep.data(), o.keep.data(), (size_t)n) != 0)) return false;
    if (o.md[n] != 7.0f || o.keep[n] != 7 || o.pts[n].x != 7.0f) return false;          // nothing written behind the arrays
    return kept.empty() || memcmp(kept.data(), o.pts.data(), kept.size() * sizeof(ssm_point)) == 0;
}
static vector<ssm_point> random_cloud(Rng& r, int n, float scale)
{
    vector<ssm_point> v;
    for (int i = 0; i < n; i++) v.push_back(pt(r.unit() * scale - scale / 3, r.unit() * scale, r.unit() * scale * 0.2f, (uint32_t)i));
    return v;
}

int main()
{
    const float inf = numeric_limits<float>::infinity(), nan = numeric_limits<float>::quiet_NaN();
    {   // four points on a line, k = 1: the mean distance is the gap to the nearer neighbour
        vector<ssm_point> v = {pt(0, 0, 0), pt(1, 0, 0), pt(3, 0, 0), pt(7, 0, 0)};
        Out o = run(v, 1, 0.0, 0.0f);
        check(o.rc == SSM_OK && o.md[0] == 1.0f && o.md[1] == 1.0f && o.md[2] == 2.0f && o.md[3] == 4.0f, "line: nearest gaps");
        check(o.info.sum_q == (uint64_t)8 << 20 && o.info.mean == 2.0 && o.info.sum_q2_hi * 4294967296.0 + o.info.sum_q2_lo == 22.0 * 1048576.0 * 1048576.0, "line: exact sums on the 2^-20 grid");
        check(o.info.threshold == 2.0 && o.n == 3 && o.keep[2] == 1 && o.keep[3] == 0 && o.pts[2].x == 3.0f, "line: d <= mean stays");
        check(restated(v, 1, 0.0, o), "line: restatement");
    }
    {   // all identical: every distance 0, threshold 0, everything stays
        vector<ssm_point> v(40, pt(1.5f, -2, 3));
        Out o = run(v, 30, 1.0, 0.0f);
        check(o.rc == SSM_OK && o.n == 40 && o.info.threshold == 0.0 && o.info.sum_q == 0 && o.info.levels == 1, "identical points");
    }
    {   // too few, and non-finite points
        vector<ssm_point> v = {pt(0, 0, 0, 1), pt(nan, 0, 0, 2), pt(1, 1, 1, 3), pt(0, inf, 0, 4), pt(2, 0, 1, 5), pt(0, 0, -inf, 6)};
        Out o = run(v, 3, 1.0, 0.0f);
        check(o.rc == SSM_OK && o.info.too_few == 1 && o.info.n_finite == 3 && o.n == 3 && o.pts[1].label == 3 && o.pts[2].label == 5 && o.info.levels == 0, "too few: the finite points, in order");
        Out p = run(v, 2, 1.0, 0.0f);
        check(p.info.too_few == 0 && p.keep[1] == 0 && p.keep[3] == 0 && p.keep[5] == 0 && p.md[1] == 0.0f && restated(v, 2, 1.0, p), "k + 1 finite points: filtered");
        Out e = run(vector<ssm_point>(), 30, 1.0, 0.0f);
        check(e.rc == SSM_OK && e.n == 0 && e.info.too_few == 1 && e.info.n_in == 0, "no points");
    }
    {   // random clouds, duplicates among them, k from 1 to 64, under four first cell sizes: one result
        Rng r{99}; bool ok = true, ladder = false;
        const int ks[] = {1, 8, 30, 33, 64};
        for (int rep = 0; rep < 5; rep++) {
            vector<ssm_point> v = random_cloud(r, 300 + 97 * rep, 2.0f + rep);
            for (int i = 0; i < 40; i++) v.push_back(v[(size_t)(r.next() % 200)]);
            v[5].y = nan;
            const float cells[] = {0.0f, 1e-6f, 1.0f, 1e30f};
            int lv[4];
            for (int c = 0; c < 4; c++) { const Out o = run(v, ks[rep], 1.0 + 0.5 * rep, cells[c]); ok = ok && restated(v, ks[rep], 1.0 + 0.5 * rep, o); lv[c] = o.info.levels; }
            ladder = ladder || (lv[1] > lv[3] && lv[3] == 1);
        }
        check(ok, "random clouds under four first cell sizes: restatement");
        check(ladder, "the first cell size changes the ladder and nothing else");
    }
    {   // two clusters farther apart, in cells, than a key axis holds; a cluster of exactly k beside a far one
        Rng r{7};
        vector<ssm_point> v = random_cloud(r, 60, 0.01f), w = random_cloud(r, 60, 0.01f);
        for (ssm_point& p : w) { p.x += 3000.0f; v.push_back(p); }
        check(restated(v, 30, 1.0, run(v, 30, 1.0, 0.001f)), "far clusters: the first cell size is raised");
        vector<ssm_point> a = random_cloud(r, 8, 0.05f), b = random_cloud(r, 50, 0.05f);
        for (ssm_point& p : b) { p.y += 50.0f; a.push_back(p); }
        Out o = run(a, 8, 1.0, 0.01f);
        check(restated(a, 8, 1.0, o) && o.md[0] > 1.0f && o.keep[0] == 0 && o.keep[20] == 1, "a cluster of exactly k needs the far one");
    }
    {   // invalid arguments; a buffer too small
        Rng r{3}; vector<ssm_point> v = random_cloud(r, 50, 1.0f), out(50); int n = -1;
        ssm_sor_params P; ssm_sor_params_default(&P);
        check(P.mean_k == 30 && P.cell == 0.0f && P.stddev_mul == 1.0 && ssm_sor_chunk() >= 64, "defaults");
        bool ok = true;
        P.mean_k = 0; ok = ok && ssm_sor_filter_host(v.data(), 50, &P, out.data(), 50, &n, nullptr, nullptr, nullptr) == SSM_E_INVAL;
        P.mean_k = 65; ok = ok && ssm_sor_filter_host(v.data(), 50, &P, out.data(), 50, &n, nullptr, nullptr, nullptr) == SSM_E_INVAL;
        P.mean_k = 30; P.cell = -1.0f; ok = ok && ssm_sor_filter_host(v.data(), 50, &P, out.data(), 50, &n, nullptr, nullptr, nullptr) == SSM_E_INVAL;
        P.cell = nan; ok = ok && ssm_sor_filter_host(v.data(), 50, &P, out.data(), 50, &n, nullptr, nullptr, nullptr) == SSM_E_INVAL;
        P.cell = 0.0f; P.stddev_mul = nan; ok = ok && ssm_sor_filter_host(v.data(), 50, &P, out.data(), 50, &n, nullptr, nullptr, nullptr) == SSM_E_INVAL;
        ok = ok && ssm_sor_filter_host(nullptr, 50, nullptr, out.data(), 50, &n, nullptr, nullptr, nullptr) == SSM_E_INVAL;
        ok = ok && ssm_sor_filter_host(v.data(), 50, nullptr, out.data(), 50, nullptr, nullptr, nullptr, nullptr) == SSM_E_INVAL && !g_err.empty();
        check(ok, "invalid arguments");
        vector<ssm_point> far = {pt(0, 0, 0), pt(10000, 0, 0), pt(0, 10000, 0), pt(0, 0, 10000)};
        P.stddev_mul = 1.0; P.mean_k = 2;
        check(ssm_sor_filter_host(far.data(), 4, &P, out.data(), 50, &n, nullptr, nullptr, nullptr) == SSM_E_INVAL, "a mean distance off the statistics grid is refused");
        ssm_sor_info I;
        check(ssm_sor_filter_host(v.data(), 50, nullptr, out.data(), 3, &n, &I, nullptr, nullptr) == SSM_E_CAPACITY && n == I.n_kept && n > 3, "a buffer too small: the number needed");
    }
    printf(failures ? "%d FAILED\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
