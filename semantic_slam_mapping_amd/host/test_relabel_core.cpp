// test_relabel_core.cpp -- label fusion on the host (csrc/ssm_relabel_host.cpp over include/ssm/relabel_core.h) as a stand-alone program: linked with that source
// and csrc/ssm_carve_host.cpp (the view and pose checks), it needs neither libssm_hip.so nor a GPU and runs as it is under the CPU sanitizers
// (-fsanitize=address,undefined).
// Checked here, from C++: hand-made points whose result the rule gives (ties, the edge guard, min_votes, unknown labels, a count of 31), the inputs whose
// conversion to an integer would be undefined (+-1e30, NaN, infinity), windows at the image's corners, empty calls, exact-size buffers (the sanitizer sees any
// byte beyond them), invalid arguments, and random clouds under random poses against a restatement of DESIGN.md s.20 written out here.
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
static void check(bool ok, const char* name) { printf("%s %s\n", ok ? "PASS" : "FAIL", name); if (!ok) failures++; }
struct Rng { uint64_t s; uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); } double unit() { return (double)(next() % 1000000) / 1000000.0; } };

static ssm_point pt(float x, float y, float z, uint32_t label) { ssm_point p; memset(&p, 0, sizeof p); p.x = x; p.y = y; p.z = z; p.w = 1.0f; p.label = label; p.pad[1] = ~label; return p; }
static const double EYE[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
static ssm_camera cam0() { ssm_camera c; c.cx = 0; c.cy = 0; c.fx = 64; c.fy = 64; c.scale = 1000; return c; }
static ssm_point at_pixel(double px, double py, float z, uint32_t label) { return pt((float)(px * z / 64.0), (float)(py * z / 64.0), z, label); }

struct Img { int w, h; vector<uint16_t> depth; vector<uint8_t> label; ssm_camera cam; };          // exactly w h entries each
static Img flat(int w, int h, uint16_t d, uint8_t l) { Img v; v.w = w; v.h = h; v.depth.assign((size_t)w * h, d); v.label.assign((size_t)w * h, l); v.cam = cam0(); return v; }
struct Out { vector<uint32_t> label; vector<uint64_t> votes; ssm_relabel_info info; int rc; };
static Out run(const vector<Img>& views, const vector<double>& Tv, const vector<ssm_point>& in, const double* Tc, const ssm_relabel_params& P)
{
    vector<ssm_relabel_host_view> hv;
    for (const Img& v : views) { ssm_relabel_host_view h; h.depth = v.depth.data(); h.label = v.label.data(); h.w = v.w; h.h = v.h; h.cam = v.cam; hv.push_back(h); }
    Out o; const int n = (int)in.size();
    o.label.assign((size_t)n, 777u); o.votes.assign((size_t)n, 777u); memset(&o.info, 0x55, sizeof o.info);
    o.rc = ssm_relabel_host(hv.empty() ? nullptr : hv.data(), Tv.empty() ? nullptr : Tv.data(), (int)views.size(), in.empty() ? nullptr : in.data(), n, Tc, &P,
                            n ? o.label.data() : nullptr, n ? o.votes.data() : nullptr, &o.info);
    return o;
}
static vector<double> eyes(size_t v) { vector<double> T; for (size_t k = 0; k < v; k++) T.insert(T.end(), EYE, EYE + 16); return T; }
static unsigned cnt(uint64_t c, int l) { return (unsigned)(c >> (5 * l)) & 31u; }

// the restatement of s.20 (and of s.16 steps 1-7 inside it): long arithmetic written out, no call into the headers
static bool restated(const vector<Img>& views, const vector<double>& Tv, const vector<ssm_point>& in, const double* Tc, const ssm_relabel_params& P, const Out& o)
{
    const int n = (int)in.size(), r = P.radius;
    ssm_relabel_info I; memset(&I, 0, sizeof I); I.n_in = n;
    for (int i = 0; i < n; i++) {
        int c[12] = {0}; const uint32_t L0 = in[i].label;
        if (L0 <= 11) c[L0] += P.own_weight;
        int ns = 0, nv = 0;
        for (size_t k = 0; k < views.size(); k++) {
            const Img& V = views[k]; const double* T = &Tv[16 * k];
            double M[3][4];
            for (int a = 0; a < 3; a++) {
                const double ra = T[a * 4], rb = T[a * 4 + 1], rc = T[a * 4 + 2];
                const double ti = -((ra * T[12] + rb * T[13]) + rc * T[14]);
                for (int j = 0; j < 3; j++) M[a][j] = (ra * Tc[j * 4] + rb * Tc[j * 4 + 1]) + rc * Tc[j * 4 + 2];
                M[a][3] = ((ra * Tc[12] + rb * Tc[13]) + rc * Tc[14]) + ti;
            }
            const double x = in[i].x, y = in[i].y, z = in[i].z;
            if (!(std::isfinite(x) && std::isfinite(y) && std::isfinite(z))) continue;
            const double qx = M[0][0] * x + M[0][1] * y + M[0][2] * z + M[0][3], qy = M[1][0] * x + M[1][1] * y + M[1][2] * z + M[1][3], qz = M[2][0] * x + M[2][1] * y + M[2][2] * z + M[2][3];
            if (!(std::isfinite(qx) && std::isfinite(qy) && std::isfinite(qz)) || qz < P.z_min) continue;
            const double px = floor(V.cam.fx * (qx / qz) + V.cam.cx + 0.5), py = floor(V.cam.fy * (qy / qz) + V.cam.cy + 0.5);
            if (!(px >= r && px <= V.w - 1 - r && py >= r && py <= V.h - 1 - r)) continue;
            const int ix = (int)px, iy = (int)py;
            long dmin = 65536; bool same = true; const int l = V.label[(size_t)iy * V.w + ix];
            for (int yy = iy - r; yy <= iy + r; yy++) for (int xx = ix - r; xx <= ix + r; xx++) {
                dmin = min(dmin, (long)V.depth[(size_t)yy * V.w + xx]); same = same && V.label[(size_t)yy * V.w + xx] == l;
            }
            if (dmin == 0) continue;
            const long long d = V.depth[(size_t)iy * V.w + ix];
            const double zs = qz * V.cam.scale;
            const long long zq = zs < 1125899906842624.0 ? llrint(zs) : 1125899906842624ll;
            const long long tol = llrint(P.tol_abs * V.cam.scale) + d * P.tol_rel_ppm / 1000000;
            if (zq + tol < dmin || llabs(zq - d) > tol) continue;
            ns++;
            if (l > 11 || (P.edge_guard && !same)) continue;
            c[l]++; nv++;
        }
        int best = 0; for (int l = 0; l < 12; l++) best = max(best, c[l]);
        uint32_t L1 = L0;
        if (best > 0) {
            int winner = -1;
            if (L0 <= 11 && c[L0] == best) winner = (int)L0;
            else for (int l = 11; l >= 0; l--) if (c[l] == best) winner = l;
            if ((uint32_t)winner != L0 && best >= P.min_votes) L1 = (uint32_t)winner;
        }
        uint64_t packed = 0; for (int l = 0; l < 12; l++) packed |= (uint64_t)c[l] << (5 * l);
        if (o.label[i] != L1 || o.votes[i] != packed) { printf("  point %d: label %u (want %u) votes %llx (want %llx)\n", i, o.label[i], L1, (unsigned long long)o.votes[i], (unsigned long long)packed); return false; }
        I.n_supported += ns > 0; I.n_voted += nv > 0; I.pairs_supported += ns; I.pairs_voted += nv;
        if (L1 != L0) { I.n_changed++; I.n_filled += L0 > 11; }
    }
    return o.info.n_in == I.n_in && o.info.n_supported == I.n_supported && o.info.n_voted == I.n_voted && o.info.n_changed == I.n_changed && o.info.n_filled == I.n_filled &&
           o.info.pairs_supported == I.pairs_supported && o.info.pairs_voted == I.pairs_voted;
}
static void pose(Rng& g, double rot, double trans, double T[16])
{
    const double a = (g.unit() - 0.5) * rot, b = (g.unit() - 0.5) * rot, c = (g.unit() - 0.5) * rot;
    const double ca = cos(a), sa = sin(a), cb = cos(b), sb = sin(b), cc = cos(c), sc = sin(c);
    const double R[3][3] = {{cb * cc, -cb * sc, sb}, {sa * sb * cc + ca * sc, -sa * sb * sc + ca * cc, -sa * cb}, {-ca * sb * cc + sa * sc, ca * sb * sc + sa * cc, ca * cb}};
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) T[j * 4 + i] = R[i][j];
    T[3] = T[7] = T[11] = 0; T[12] = (g.unit() - 0.5) * trans; T[13] = (g.unit() - 0.5) * trans; T[14] = (g.unit() - 0.5) * trans; T[15] = 1;
}

int main()
{
    ssm_relabel_params D; ssm_relabel_params_default(&D);
    check(D.radius == 1 && D.edge_guard == 1 && D.own_weight == 1 && D.min_votes == 2 && D.tol_abs == 0.05 && D.tol_rel_ppm == 20000 && D.z_min == 0.1 && D.pad == 0, "defaults");
    ssm_relabel_params_default(nullptr);
    {   // the rule on hand-made points: four flat views, the label under each point set per view
        vector<Img> V(4, flat(30, 7, 1000, 255)); V[3] = flat(34, 9, 1000, 255);
        vector<ssm_point> in; int x = 2;
        auto point = [&](uint32_t L0, int a, int b, int c, int d) { const int l[4] = {a, b, c, d}; for (int k = 0; k < 4; k++) for (int yy = 2; yy <= 4; yy++) for (int xx = x - 1; xx <= x + 1; xx++) V[k].label[(size_t)yy * V[k].w + xx] = (uint8_t)l[k]; in.push_back(at_pixel(x, 3, 1.0f, L0)); x += 3; };
        point(3, 5, 255, 255, 255);          // 0: a 1 : 1 tie, the own label wins
        point(255, 7, 7, 4, 4);              // 1: a tie without an own label: the lowest id
        point(2, 6, 6, 255, 255);            // 2: the second view's vote is withheld by the guard (below)
        V[1].label[(size_t)2 * 30 + (2 + 3 * 2 + 1)] = 8;
        point(255, 5, 255, 255, 255);        // 3: best < min_votes
        point(0xFFFFFF05u, 1, 255, 1, 255);  // 4: upper bytes set: unknown, filled
        point(0, 10, 255, 10, 255);          // 5: overruled
        point(0, 10, 10, 255, 255);          // 6: the second view occludes: no vote
        V[1].depth[(size_t)3 * 30 + (2 + 3 * 6)] = 500;
        point(9, 9, 9, 9, 9);                // 7: agreement
        Out o = run(V, eyes(4), in, EYE, D);
        const uint32_t want[8] = {3, 4, 2, 255, 1, 10, 0, 9};
        bool ok = o.rc == SSM_OK;
        for (int i = 0; i < 8; i++) ok = ok && o.label[i] == want[i];
        check(ok && cnt(o.votes[0], 3) == 1 && cnt(o.votes[0], 5) == 1 && cnt(o.votes[2], 6) == 1 && cnt(o.votes[7], 9) == 5 && o.info.n_changed == 3 && o.info.n_filled == 2, "the rule on hand-made points");
        check(restated(V, eyes(4), in, EYE, D, o), "hand-made points against the restatement");
        ssm_relabel_params P = D; P.edge_guard = 0;
        o = run(V, eyes(4), in, EYE, P);
        check(o.rc == SSM_OK && o.label[2] == 6 && restated(V, eyes(4), in, EYE, P, o), "without the guard the withheld vote flips the result");
    }
    {   // 16 views, own_weight 15: a count of 31; and the tie at 15
        vector<Img> V(16, flat(9, 5, 1000, 3));
        for (int k = 0; k < 16; k++) for (int yy = 1; yy <= 3; yy++) for (int xx = 4; xx <= 6; xx++) V[k].label[(size_t)yy * 9 + xx] = k < 15 ? 11 : 5;
        vector<ssm_point> in = {at_pixel(2, 2, 1.0f, 3), at_pixel(5, 2, 1.0f, 0), at_pixel(2, 2, 1.0f, 4)};
        ssm_relabel_params P = D; P.own_weight = 15;
        Out o = run(V, eyes(16), in, EYE, P);
        check(o.rc == SSM_OK && cnt(o.votes[0], 3) == 31 && o.label[0] == 3 && cnt(o.votes[1], 0) == 15 && cnt(o.votes[1], 11) == 15 && o.label[1] == 0 && o.label[2] == 3 && restated(V, eyes(16), in, EYE, P, o), "a count of 31");
    }
    {   // coordinates whose conversion would be undefined, windows at the corners, radius 0..3
        const float big = 1.0e30f, nan = numeric_limits<float>::quiet_NaN(), inf = numeric_limits<float>::infinity();
        vector<ssm_point> in = {pt(big, 0, 1, 1), pt(-big, 0, 1, 1), pt(0, big, 1, 1), pt(0, 0, big, 1), pt(big, big, big, 1), pt(nan, 0, 1, 1), pt(0, nan, 1, 1), pt(0, 0, nan, 1), pt(inf, 0, 1, 1),
                                pt(0, -inf, 1, 1), pt(0, 0, inf, 1), pt(0, 0, -1, 1), pt(0, 0, 0, 1), pt(3.0e38f, 3.0e38f, 3.0e38f, 1), pt(1e-30f, 1e-30f, 1e-38f, 1)};
        for (int y = -1; y <= 7; y++) for (int x = -1; x <= 9; x++) in.push_back(at_pixel(x, y, 1.0f, 255));
        vector<Img> V(2, flat(9, 7, 1000, 6));
        bool ok = true;
        for (int r = 0; r <= 3; r++) {
            ssm_relabel_params P = D; P.radius = r;
            Out o = run(V, eyes(2), in, EYE, P);
            ok = ok && o.rc == SSM_OK && restated(V, eyes(2), in, EYE, P, o) && o.info.n_filled == (9 - 2 * r) * (7 - 2 * r);
        }
        check(ok, "degenerate coordinates and windows at the image's border");
    }
    {   // empty calls
        vector<Img> V(1, flat(9, 7, 1000, 6));
        vector<ssm_point> in = {at_pixel(3, 3, 1.0f, 2), at_pixel(4, 3, 1.0f, 300)};
        Out o = run({}, {}, in, EYE, D);
        check(o.rc == SSM_OK && o.label[0] == 2 && o.label[1] == 300 && o.votes[0] == (1ull << 10) && o.votes[1] == 0 && o.info.n_in == 2 && o.info.n_changed == 0 && o.info.pairs_supported == 0, "v = 0");
        o = run(V, eyes(1), {}, EYE, D);
        check(o.rc == SSM_OK && o.info.n_in == 0 && o.info.n_supported == 0 && o.info.pairs_voted == 0, "n = 0");
        o = run({}, {}, {}, EYE, D);
        check(o.rc == SSM_OK && o.info.n_in == 0, "v = 0 and n = 0");
        check(ssm_relabel_host(nullptr, nullptr, 0, in.data(), 2, EYE, nullptr, nullptr, nullptr, nullptr) == SSM_E_INVAL, "points without a label_out are refused");
        vector<uint32_t> lab(2); check(ssm_relabel_host(nullptr, nullptr, 0, in.data(), 2, EYE, nullptr, lab.data(), nullptr, nullptr) == SSM_OK && lab[1] == 300, "defaults, no votes, no info");
    }
    {   // refusals
        vector<Img> V(1, flat(9, 7, 1000, 6));
        vector<ssm_point> in = {at_pixel(3, 3, 1.0f, 2)};
        bool ok = true;
        auto bad = [&](ssm_relabel_params P) { ok = ok && run(V, eyes(1), in, EYE, P).rc == SSM_E_INVAL && run({}, {}, in, EYE, P).rc == SSM_E_INVAL; };
        ssm_relabel_params P;
        P = D; P.radius = -1; bad(P); P = D; P.radius = 4; bad(P); P = D; P.edge_guard = 2; bad(P); P = D; P.edge_guard = -1; bad(P); P = D; P.own_weight = 16; bad(P); P = D; P.own_weight = -1; bad(P);
        P = D; P.min_votes = 0; bad(P); P = D; P.min_votes = 32; bad(P); P = D; P.tol_abs = -1; bad(P); P = D; P.tol_abs = numeric_limits<double>::quiet_NaN(); bad(P);
        P = D; P.tol_rel_ppm = -1; bad(P); P = D; P.tol_rel_ppm = 1000001; bad(P); P = D; P.z_min = -0.5; bad(P); P = D; P.z_min = numeric_limits<double>::infinity(); bad(P);
        check(ok, "parameters out of range");
        vector<Img> many(17, V[0]);
        check(run(many, eyes(17), in, EYE, D).rc == SSM_E_INVAL && run(vector<Img>(16, V[0]), eyes(16), in, EYE, D).rc == SSM_OK, "17 views refused, 16 taken");
        vector<double> T = eyes(1); T[13] = numeric_limits<double>::quiet_NaN();
        check(run(V, T, in, EYE, D).rc == SSM_E_INVAL && run(V, eyes(1), in, T.data(), D).rc == SSM_E_INVAL && run(V, eyes(1), in, nullptr, D).rc == SSM_E_INVAL, "non-finite and null poses");
        ok = true;
        for (double s : {0.0, -1.0, 1.0e6 + 1, (double)numeric_limits<double>::quiet_NaN()}) { vector<Img> W = V; W[0].cam.scale = s; ok = ok && run(W, eyes(1), in, EYE, D).rc == SSM_E_INVAL; }
        { vector<Img> W = V; W[0].cam.fx = numeric_limits<double>::infinity(); ok = ok && run(W, eyes(1), in, EYE, D).rc == SSM_E_INVAL; W = V; W[0].w = 0; ok = ok && run(W, eyes(1), in, EYE, D).rc == SSM_E_INVAL; }
        check(ok, "cameras and sizes");
        ssm_relabel_host_view hv; hv.depth = nullptr; hv.label = V[0].label.data(); hv.w = 9; hv.h = 7; hv.cam = cam0();
        uint32_t l1; check(ssm_relabel_host(&hv, EYE, 1, in.data(), 1, EYE, nullptr, &l1, nullptr, nullptr) == SSM_E_INVAL && ssm_relabel_host(nullptr, EYE, 1, in.data(), 1, EYE, nullptr, &l1, nullptr, nullptr) == SSM_E_INVAL &&
              ssm_relabel_host(nullptr, nullptr, -1, in.data(), 1, EYE, nullptr, &l1, nullptr, nullptr) == SSM_E_INVAL && ssm_relabel_host(nullptr, nullptr, 0, in.data(), -1, EYE, nullptr, &l1, nullptr, nullptr) == SSM_E_INVAL, "null views, negative counts");
    }
    {   // the label image
        const uint8_t bgr[] = {128, 128, 128, 0, 0, 128, 192, 128, 0, 192, 128, 1, 0, 0, 0};
        vector<uint8_t> l(5, 9);
        check(ssm_relabel_labels_host(bgr, 5, l.data()) == SSM_OK && l[0] == 0 && l[1] == 1 && l[2] == 11 && l[3] == 255 && l[4] == 255 && ssm_relabel_labels_host(nullptr, 0, nullptr) == SSM_OK &&
              ssm_relabel_labels_host(nullptr, 1, l.data()) == SSM_E_INVAL, "the label image from BGR");
    }
    {   // random clouds, views of several sizes and cameras, random poses and parameters
        Rng g{12345}; bool ok = true; long changed = 0, filled = 0, supported = 0;
        for (int round = 0; round < 40 && ok; round++) {
            const int v = (int)(g.next() % 6), n = (int)(g.next() % 400);
            vector<Img> V; vector<double> Tv((size_t)v * 16);
            for (int k = 0; k < v; k++) {
                const int w = 20 + (int)(g.next() % 40), h = 12 + (int)(g.next() % 20);
                Img im = flat(w, h, 0, 255); im.cam.cx = w / 2.0 - 0.25; im.cam.cy = h / 2.0 + 0.125; im.cam.fx = im.cam.fy = 0.9 * w; im.cam.scale = round % 3 ? 1000 : 5000;
                for (int i = 0; i < w * h; i++) {
                    const int x = i % w;
                    im.depth[i] = g.next() % 50 == 0 ? 0 : (uint16_t)((x * 3 < w ? 2.0 : 3.0) * im.cam.scale + g.next() % 5);
                    im.label[i] = g.next() % 20 == 0 ? 255 : (uint8_t)((x * 8 / w + (g.next() % 15 == 0)) % 12);
                }
                V.push_back(im); pose(g, 0.02, 0.02, &Tv[(size_t)16 * k]);
            }
            double Tc[16]; pose(g, 0.02, 0.02, Tc);
            vector<ssm_point> in;
            for (int i = 0; i < n; i++) {
                const double u = g.unit() * 1.2 - 0.6, w = g.unit() * 0.8 - 0.4; const float z = u * 3 < -0.5 ? 2.0f : 3.0f;
                const uint32_t kind = g.next() % 10; const uint32_t L = kind < 6 ? g.next() % 12 : kind < 8 ? 255u : g.next();
                in.push_back(pt((float)(u * z / 0.9), (float)(w * z / 0.9), z + (float)(g.unit() * 0.02), L));
            }
            ssm_relabel_params P = D; P.radius = (int)(g.next() % 4); P.edge_guard = (int)(g.next() % 2); P.own_weight = (int)(g.next() % 4); P.min_votes = 1 + (int)(g.next() % 3);
            Out o = run(V, Tv, in, Tc, P);
            ok = ok && o.rc == SSM_OK && restated(V, Tv, in, Tc, P, o);
            changed += o.info.n_changed; filled += o.info.n_filled; supported += o.info.pairs_supported;
        }
        printf("  random rounds: %ld supported pairs, %ld changed, %ld filled\n", supported, changed, filled);
        check(ok && supported > 1000 && changed > 100 && filled > 20, "random clouds against the restatement");
    }
    printf(failures ? "%d FAILED\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
