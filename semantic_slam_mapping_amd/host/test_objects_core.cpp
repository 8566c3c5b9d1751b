// test_objects_core.cpp -- object extraction on the host (csrc/ssm_objects_host.cpp over include/ssm/objects_core.h) as a stand-alone program: linked with that
// source, csrc/ssm_grid_host.cpp (the grid), csrc/ssm_carve_host.cpp (the pose check) and csrc/ssm_cloud_table.cpp (the point count), it needs neither
// libssm_hip.so nor a GPU and runs as it is under the CPU sanitizers (-fsanitize=address,undefined).  Checked here, from C++: the cases of DESIGN.md s.21 with known
// outcomes (a diagonal contact under both connectivities, neighbours of different labels, labels outside the mask, the three rejection rules and their order, the
// numbering), exact-size buffers (the sanitizer sees any byte beyond them), the capacity rule, invalid arguments, random cell arrays against a restatement written
// out here (labels spread until nothing changes -- no flood fill), and random clouds: the invariants of stage 2 and its independence of the order.
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

struct Cells {
    int nx, ny; vector<uint8_t> cls, ol; vector<int32_t> gq, tq; vector<uint32_t> nh;
    Cells(int nx_, int ny_) : nx(nx_), ny(ny_), cls((size_t)nx_ * ny_, 1), ol((size_t)nx_ * ny_, 255), gq((size_t)nx_ * ny_, 0), tq((size_t)nx_ * ny_, 1024), nh((size_t)nx_ * ny_, 30) {}
    void set(int x, int y, uint8_t label) { cls[(size_t)y * nx + x] = 4; ol[(size_t)y * nx + x] = label; }
};
struct Out { vector<ssm_object> rec; vector<int32_t> oid; ssm_objects_info info; int n, rc; };
static ssm_objects_params loose(int conn) { ssm_objects_params P; ssm_objects_params_default(&P); P.connectivity = conn; P.min_cells = 1; P.min_points = 0; P.min_height = 0; return P; }
// buffers of exactly the sizes the call may touch
static Out run(const Cells& c, const ssm_objects_params& P, int cap = -1)
{
    Out o; const size_t nc = (size_t)c.nx * c.ny;
    if (cap < 0) cap = (int)nc;
    o.rec.resize((size_t)cap); o.oid.assign(nc, -7); memset(&o.info, 0, sizeof o.info); o.n = -7;
    o.rc = ssm_objects_cells_host(c.cls.data(), c.ol.data(), c.gq.data(), c.tq.data(), c.nh.data(), c.nx, c.ny, &P, cap ? o.rec.data() : nullptr, cap, &o.n, o.oid.data(), &o.info);
    if (o.rc == SSM_OK) o.rec.resize((size_t)o.n);
    return o;
}
// the restatement: every member starts with its own index, then takes the smallest label among itself and its joined neighbours until nothing changes
static bool restated(const Cells& c, const ssm_objects_params& P, const Out& o)
{
    const int nx = c.nx, ny = c.ny; const size_t nc = (size_t)nx * ny;
    vector<long long> lab(nc, -1);
    for (size_t i = 0; i < nc; i++) if (c.cls[i] == 4 && c.ol[i] < 12 && ((P.label_mask >> c.ol[i]) & 1)) lab[i] = (long long)i;
    for (bool changed = true; changed;) {
        changed = false;
        for (int y = 0; y < ny; y++) for (int x = 0; x < nx; x++) {
            const size_t i = (size_t)y * nx + x; if (lab[i] < 0) continue;
            for (int dy = -1; dy <= 1; dy++) for (int dx = -1; dx <= 1; dx++) {
                if ((!dx && !dy) || (P.connectivity == 4 && dx && dy)) continue;
                const int X = x + dx, Y = y + dy; if (X < 0 || Y < 0 || X >= nx || Y >= ny) continue;
                const size_t j = (size_t)Y * nx + X;
                if (lab[j] >= 0 && c.ol[j] == c.ol[i] && lab[j] < lab[i]) { lab[i] = lab[j]; changed = true; }
            }
        }
    }
    const long long hq = llrint(P.min_height * 1024.0);
    long long members = 0, comps = 0, kept = 0, rej[3] = {0, 0, 0};
    bool ok = o.rc == SSM_OK;
    vector<int32_t> want(nc, -1);
    for (size_t r = 0; r < nc && ok; r++) {
        if (lab[r] >= 0) members++;
        if (lab[r] != (long long)r) continue;
        comps++;
        long long cells = 0, pts = 0, x0 = INT_MAX, x1 = INT_MIN, y0 = INT_MAX, y1 = INT_MIN, g = INT_MAX, t = INT_MIN;
        for (size_t i = 0; i < nc; i++) if (lab[i] == (long long)r) {
            cells++; pts += c.nh[i]; x0 = min<long long>(x0, i % nx); x1 = max<long long>(x1, i % nx); y0 = min<long long>(y0, i / nx); y1 = max<long long>(y1, i / nx);
            g = min<long long>(g, c.gq[i]); t = max<long long>(t, c.tq[i]);
        }
        if (cells < P.min_cells) { rej[0]++; continue; }
        if (pts < P.min_points) { rej[1]++; continue; }
        if (t - g < hq) { rej[2]++; continue; }
        ok = ok && kept < (long long)o.rec.size();
        if (!ok) break;
        const ssm_object& q = o.rec[(size_t)kept];
        ok = q.root == (int32_t)r && q.label == c.ol[r] && q.cells == cells && q.cell_points == (uint64_t)pts && q.cx_min == x0 && q.cx_max == x1 && q.cy_min == y0 && q.cy_max == y1 &&
             q.ground_q == g && q.top_q == t && q.n_points == 0 && q.n_label == 0 && q.pad == 0 && q.x_min_q == INT_MAX && q.x_max_q == INT_MIN && q.y_min_q == INT_MAX &&
             q.y_max_q == INT_MIN && q.z_min_q == INT_MAX && q.z_max_q == INT_MIN && q.sum_x == 0 && q.sum_y == 0 && q.sum_z == 0;
        for (size_t i = 0; i < nc; i++) if (lab[i] == (long long)r) want[i] = (int32_t)kept;
        kept++;
    }
    const ssm_objects_info& I = o.info;
    return ok && want == o.oid && o.n == kept && I.member_cells == members && I.components == comps && I.kept == kept && I.rejected_cells == rej[0] && I.rejected_points == rej[1] &&
           I.rejected_height == rej[2] && I.n_in == 0 && I.object_points == 0;
}
// a point at grid coordinates under the default G and the identity pose: world (gx, -gz, gy)
static ssm_point gp(double gx, double gy, double gz, uint32_t label)
{ ssm_point p; memset(&p, 0, sizeof p); p.x = (float)gx; p.y = (float)-gz; p.z = (float)gy; p.w = 1.0f; p.label = label; return p; }
static ssm_grid_params small()
{ ssm_grid_params P; ssm_grid_params_default(&P); P.x0 = -2.0; P.y0 = 0.0; P.cell = 0.25; P.nx = 16; P.ny = 12; P.step = 0.25; P.min_obstacle_points = 2; return P; }

struct Full { vector<ssm_object> rec; vector<int32_t> oid, ids; ssm_objects_info info; int n, rc; };
static Full run_clouds(const vector<vector<ssm_point>>& clouds, const ssm_grid_params& G, const ssm_objects_params& P, int cap = 64)
{
    Full o; size_t total = 0;
    vector<const ssm_point*> ptrs; vector<int32_t> n; vector<double> T;
    for (const auto& c : clouds) { ptrs.push_back(c.empty() ? nullptr : c.data()); n.push_back((int32_t)c.size()); total += c.size(); T.insert(T.end(), EYE, EYE + 16); }
    o.rec.resize((size_t)cap); o.oid.assign((size_t)G.nx * G.ny, -7); o.ids.assign(total, -7); memset(&o.info, 0, sizeof o.info); o.n = -7;
    o.rc = ssm_objects_host(ptrs.empty() ? nullptr : ptrs.data(), n.empty() ? nullptr : n.data(), T.empty() ? nullptr : T.data(), (int)clouds.size(), &G, &P, cap ? o.rec.data() : nullptr, cap,
                            &o.n, o.oid.data(), total ? o.ids.data() : nullptr, &o.info);
    if (o.rc == SSM_OK) o.rec.resize((size_t)o.n);
    return o;
}

int main()
{
    static_assert(sizeof(ssm_object) == 104 && sizeof(ssm_objects_info) == 64, "the records of s.21");
    {
        ssm_objects_params D; ssm_objects_params_default(&D);
        check(D.label_mask == 0xE00u && D.connectivity == 8 && D.min_cells == 2 && D.min_points == 20 && D.min_height == 0.3, "the defaults");
    }
    {
        Cells c(5, 4); c.set(1, 1, 9); c.set(2, 2, 9);
        const Out a = run(c, loose(8)), b = run(c, loose(4));
        check(a.rc == SSM_OK && a.n == 1 && a.rec[0].root == 6 && a.rec[0].cells == 2 && a.oid[6] == 0 && a.oid[12] == 0 && restated(c, loose(8), a), "a diagonal contact is one component under 8");
        check(b.rc == SSM_OK && b.n == 2 && b.rec[0].root == 6 && b.rec[1].root == 12 && b.oid[12] == 1 && restated(c, loose(4), b), "and two under 4");
    }
    {
        Cells c(5, 4); c.set(1, 1, 9); c.set(2, 1, 10); c.set(3, 1, 9); c.set(2, 2, 8); c.set(0, 3, 12); c.cls[3 * 5 + 4] = 4; c.ol[3 * 5 + 4] = 255;
        const Out a = run(c, loose(8));
        check(a.rc == SSM_OK && a.n == 3 && a.info.member_cells == 3 && a.rec[0].label == 9 && a.rec[1].label == 10 && a.rec[2].label == 9 && a.oid[11] == -1 && restated(c, loose(8), a),
              "neighbours of different labels never join; labels outside the mask and above 11 form nothing");
        Cells d(5, 4); d.set(1, 1, 9); d.set(2, 1, 9); d.set(3, 1, 9); d.cls[1 * 5 + 2] = 1;
        check(run(d, loose(8)).n == 2, "a cell that is no obstacle is no member, whatever its label");
    }
    {
        Cells c(9, 7); ssm_objects_params P; ssm_objects_params_default(&P); P.min_height = 0.5;
        fill(c.nh.begin(), c.nh.end(), 10u); fill(c.tq.begin(), c.tq.end(), 512);
        c.set(0, 0, 9); c.set(1, 0, 9);                                                           // kept: 2 cells, 20 points, 512 units
        c.set(4, 0, 9); c.nh[4] = 20;                                                             // one cell
        c.set(0, 2, 9); c.set(1, 2, 9); c.nh[2 * 9] = 9;                                          // 19 points
        c.set(4, 2, 9); c.set(5, 2, 9); c.tq[2 * 9 + 4] = c.tq[2 * 9 + 5] = 511;                  // 511 units
        c.set(0, 4, 9); c.nh[4 * 9] = 1; c.tq[4 * 9] = 3;                                         // fails all three: counted as cells
        c.set(4, 4, 9); c.set(5, 4, 9); c.nh[4 * 9 + 4] = c.nh[4 * 9 + 5] = 2; c.tq[4 * 9 + 4] = c.tq[4 * 9 + 5] = 100;          // points and height: counted as points
        const Out a = run(c, P);
        check(a.rc == SSM_OK && a.n == 1 && a.rec[0].root == 0 && a.info.components == 6 && a.info.rejected_cells == 2 && a.info.rejected_points == 2 && a.info.rejected_height == 1 &&
              restated(c, P, a), "each rejection rule fires alone and the first one that fails is counted");
        int kept = 0; for (int32_t v : a.oid) kept += v == 0;
        check(kept == 2 && *max_element(a.oid.begin(), a.oid.end()) == 0 && *min_element(a.oid.begin(), a.oid.end()) == -1, "object_id is -1 on rejected components");
    }
    {
        Cells c(6, 6); c.set(5, 0, 11); c.set(0, 1, 9); c.set(1, 1, 9); c.set(3, 3, 10); c.set(0, 5, 9); c.set(5, 5, 10);
        const Out a = run(c, loose(8));
        bool ok = a.rc == SSM_OK && a.n == 5;
        const int roots[5] = {5, 6, 21, 30, 35};
        for (int k = 0; k < 5 && ok; k++) ok = a.rec[(size_t)k].root == roots[k] && a.oid[(size_t)roots[k]] == k;
        check(ok, "ids ascend with roots");
        const Out s = run(c, loose(8), 4);
        bool untouched = s.rc == SSM_E_CAPACITY && s.n == 5 && s.info.kept == 0;
        for (int32_t v : s.oid) untouched = untouched && v == -7;
        check(untouched, "cap = K - 1: SSM_E_CAPACITY, *n_out = K, nothing else written");
        check(run(c, loose(8), 5).rc == SSM_OK && run(c, loose(8), 0).rc == SSM_E_CAPACITY, "cap = K is enough, cap = 0 is not");
    }
    {   // invalid arguments
        Cells c(4, 3); c.set(1, 1, 9);
        auto bad = [&](ssm_objects_params P) { return run(c, P).rc == SSM_E_INVAL; };
        const double dnan = numeric_limits<double>::quiet_NaN(), dinf = numeric_limits<double>::infinity();
        bool ok = true; ssm_objects_params P;
        P = loose(8); P.connectivity = 6; ok = ok && bad(P);    P = loose(8); P.connectivity = 0; ok = ok && bad(P);   P = loose(8); P.min_cells = -1; ok = ok && bad(P);
        P = loose(8); P.min_points = -1; ok = ok && bad(P);     P = loose(8); P.min_height = -1e-9; ok = ok && bad(P); P = loose(8); P.min_height = dnan; ok = ok && bad(P);
        P = loose(8); P.min_height = dinf; ok = ok && bad(P);
        check(ok, "every bad parameter is refused");
        P = loose(8); P.min_height = 1e300; P.min_cells = INT_MAX;
        check(run(c, P).rc == SSM_OK && run(c, P).n == 0, "the limits themselves are legal");
        int n = 0; ssm_object rec[12];
        P = loose(8);
        check(ssm_objects_cells_host(nullptr, c.ol.data(), c.gq.data(), c.tq.data(), c.nh.data(), 4, 3, &P, rec, 12, &n, nullptr, nullptr) == SSM_E_INVAL &&
              ssm_objects_cells_host(c.cls.data(), c.ol.data(), c.gq.data(), c.tq.data(), c.nh.data(), 4, 3, &P, rec, 12, nullptr, nullptr, nullptr) == SSM_E_INVAL &&
              ssm_objects_cells_host(c.cls.data(), c.ol.data(), c.gq.data(), c.tq.data(), c.nh.data(), 0, 3, &P, rec, 12, &n, nullptr, nullptr) == SSM_E_INVAL &&
              ssm_objects_cells_host(c.cls.data(), c.ol.data(), c.gq.data(), c.tq.data(), c.nh.data(), 4097, 4096, &P, rec, 12, &n, nullptr, nullptr) == SSM_E_INVAL &&
              ssm_objects_cells_host(c.cls.data(), c.ol.data(), c.gq.data(), c.tq.data(), c.nh.data(), 4, 3, &P, nullptr, 12, &n, nullptr, nullptr) == SSM_E_INVAL,
              "null arguments and impossible sizes are refused");
        check(ssm_objects_cells_host(c.cls.data(), c.ol.data(), c.gq.data(), c.tq.data(), c.nh.data(), 4, 3, &P, rec, 12, &n, nullptr, nullptr) == SSM_OK && n == 1, "null outputs are skipped");
        ssm_grid_params G = small(); G.x0 = 1048576.0 - 3.0;
        check(run_clouds({{gp(0, 1, 0, 9)}}, G, P).rc == SSM_E_INVAL && g_err.find("2^20") != string::npos, "a grid whose extent leaves 2^20 m is refused");
        const vector<ssm_point> one = {gp(0, 1, 0, 9), gp(0, 1, 0, 9)};
        const ssm_point* twice[2] = {one.data(), one.data()}; int32_t n2[2] = {1, 1}, neg[2] = {1, -1}, big[2] = {INT_MAX, 1}; double T2[32]; memcpy(T2, EYE, sizeof EYE); memcpy(T2 + 16, EYE, sizeof EYE);
        const ssm_point* two[2] = {one.data(), one.data() + 1};
        G = small();
        check(ssm_objects_host(twice, n2, T2, 2, &G, &P, rec, 12, &n, nullptr, nullptr, nullptr) == SSM_E_INVAL && g_err.find("twice") != string::npos &&
              ssm_objects_host(two, neg, T2, 2, &G, &P, rec, 12, &n, nullptr, nullptr, nullptr) == SSM_E_INVAL &&
              ssm_objects_host(two, big, T2, 2, &G, &P, rec, 12, &n, nullptr, nullptr, nullptr) == SSM_E_INVAL && g_err.find("2^31") != string::npos &&
              ssm_objects_host(two, n2, T2, 2, &G, &P, rec, 12, nullptr, nullptr, nullptr, nullptr) == SSM_E_INVAL &&
              ssm_objects_host(two, n2, T2, 2, &G, &P, rec, 12, &n, nullptr, nullptr, nullptr) == SSM_OK, "the same cloud twice, a negative count, 2^31 points and a null count are refused");
    }
    {   // random cell arrays against the restatement
        Rng r{2024};
        bool ok = true;
        for (int t = 0; t < 60 && ok; t++) {
            Cells c(1 + (int)(r.next() % 40), 1 + (int)(r.next() % 40));
            const double density = 0.2 + 0.6 * r.unit();
            for (size_t i = 0; i < c.cls.size(); i++) {
                c.cls[i] = (uint8_t)(r.unit() < density ? 4 : r.next() % 4); c.ol[i] = (uint8_t)(r.next() % 6 == 0 ? 255 : 7 + r.next() % 6);
                c.gq[i] = (int32_t)(r.next() % 4000) - 3000; c.tq[i] = c.gq[i] + (int32_t)(r.next() % 2000); c.nh[i] = r.next() % 40;
            }
            ssm_objects_params P; ssm_objects_params_default(&P);
            P.connectivity = t & 1 ? 4 : 8; P.min_cells = (int32_t)(r.next() % 4); P.min_points = (int32_t)(r.next() % 60); P.min_height = r.unit(); P.label_mask = 0xF00u >> (t % 3);
            ok = restated(c, P, run(c, P));
        }
        check(ok, "random cell arrays equal the restatement");
    }
    {   // clouds: two boxes on a ground sheet
        Rng r{77};
        vector<ssm_point> all;
        for (int i = 0; i < 3000; i++) all.push_back(gp(-2.0 + 4.0 * r.unit(), 3.0 * r.unit(), -1.5 + 0.01 * r.unit(), 4));
        for (int i = 0; i < 800; i++) all.push_back(gp(-1.2 + 0.9 * r.unit(), 0.6 + 0.6 * r.unit(), -1.2 + 1.0 * r.unit(), i % 10 ? 9 : 4));          // a car; a tenth of its points say Road
        for (int i = 0; i < 200; i++) all.push_back(gp(1.05 + 0.15 * r.unit(), 2.05 + 0.4 * r.unit(), -1.2 + 1.5 * r.unit(), 10));                    // a pedestrian over two cells
        all.push_back(gp(0, 1, numeric_limits<float>::quiet_NaN(), 9)); all.push_back(gp(50, 1, 0, 9)); all.push_back(gp(0, 1, 9, 9));                   // rejected, outside, out of band
        for (size_t i = all.size() - 1; i > 0; i--) swap(all[i], all[r.next() % (i + 1)]);
        const ssm_grid_params G = small(); ssm_objects_params P; ssm_objects_params_default(&P);
        vector<vector<ssm_point>> clouds = {vector<ssm_point>(all.begin(), all.begin() + 1500), {}, vector<ssm_point>(all.begin() + 1500, all.end())};
        const Full a = run_clouds(clouds, G, P, 2);
        bool ok = a.rc == SSM_OK && a.n == 2 && a.rec[0].label == 9 && a.rec[1].label == 10 && a.info.n_in == (long long)all.size();
        long long assigned = 0;
        for (int k = 0; k < a.n && ok; k++) {
            const ssm_object& o = a.rec[(size_t)k];
            long long cnt = 0; for (int32_t v : a.ids) cnt += v == k;
            assigned += cnt;
            ok = o.n_points == o.cell_points && cnt == o.n_points && o.n_label <= o.n_points && o.z_max_q == o.top_q && o.z_min_q > o.ground_q && o.x_min_q <= o.x_max_q &&
                 o.x_min_q >= (int32_t)llrint((G.x0 + o.cx_min * G.cell) * 1024) && o.x_max_q <= (int32_t)llrint((G.x0 + (o.cx_max + 1) * G.cell) * 1024) &&
                 o.y_min_q >= (int32_t)llrint((G.y0 + o.cy_min * G.cell) * 1024) && o.y_max_q <= (int32_t)llrint((G.y0 + (o.cy_max + 1) * G.cell) * 1024) &&
                 o.sum_x >= (long long)o.n_points * o.x_min_q && o.sum_x <= (long long)o.n_points * o.x_max_q && o.sum_z <= (long long)o.n_points * o.z_max_q;
        }
        check(ok && a.info.object_points == assigned && a.rec[0].n_label < a.rec[0].n_points && a.rec[1].n_label == a.rec[1].n_points, "n_points == cell_points; the boxes lie inside their cells' extent");
        int32_t lo = 0; for (int32_t v : a.ids) lo = min(lo, v);
        check(lo == -1 && (int)a.ids.size() == (int)all.size(), "ids_out is one id per point, -1 for the others");
        // the order of clouds and points does not matter
        vector<vector<ssm_point>> rev(clouds.rbegin(), clouds.rend());
        for (auto& c : rev) reverse(c.begin(), c.end());
        const Full b = run_clouds(rev, G, P, 2);
        vector<int32_t> back(b.ids.rbegin(), b.ids.rend());
        check(b.rc == SSM_OK && b.n == a.n && !memcmp(b.rec.data(), a.rec.data(), (size_t)a.n * sizeof(ssm_object)) && b.oid == a.oid && !memcmp(&b.info, &a.info, sizeof a.info) && back == a.ids,
              "the order of clouds and points changes nothing");
        const Full s = run_clouds(clouds, G, P, 1);
        bool untouched = s.rc == SSM_E_CAPACITY && s.n == 2;
        for (int32_t v : s.oid) untouched = untouched && v == -7;
        for (int32_t v : s.ids) untouched = untouched && v == -7;
        check(untouched, "ssm_objects_host with cap = K - 1 writes nothing but *n_out");
        const Full e = run_clouds({}, G, P, 0);
        check(e.rc == SSM_OK && e.n == 0 && e.info.components == 0 && *max_element(e.oid.begin(), e.oid.end()) == -1, "no cloud at all: no object");
    }
    printf(failures ? "%d FAILED\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
