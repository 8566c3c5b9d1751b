// test_cloud_table.cpp -- the host's half of the cloud-segment table (csrc/ssm_cloud_table.cpp, csrc/cloud_table.h) as a stand-alone program: linked with that one
// source, it needs neither libssm_hip.so nor a GPU and runs as it is under the CPU sanitizers (-fsanitize=address,undefined).
// Checked here: the numbering and the blocks' first clouds against the definition written out -- blk[b] is the ONE cloud k with off[k] <= b T < off[k] + n[k] --
// on the size lists of the GPU tests, on empty clouds in every position, on sizes around the block, on a block that three boundaries cross, on alignment's strided
// counts and on three clouds of 2^30 points (12.6 M blocks: no 32-bit product survives that); the blk buffer is exactly `blocks` ints, so the sanitizer sees a
// write beyond it.  And the point count of the host-array calls against the two loops it replaced, with the stages' bounds on top.
#include "../csrc/ssm_host.h"
#include <cstdio>
using namespace std;

static int failures = 0;
static void check(bool ok, const string& name) { printf("%s %s\n", ok ? "PASS" : "FAIL", name.c_str()); if (!ok) failures++; }

// the table of clouds of these sizes with blocks of T points, against the definition
static bool table_ok(const vector<int32_t>& n, int T)
{
    const int m = (int)n.size();
    vector<CloudSeg> seg((size_t)m);
    for (int k = 0; k < m; k++) { memset(&seg[k], 0, sizeof(CloudSeg)); seg[k].n = n[k]; seg[k].stride = 1; seg[k].off = -7; }
    int64_t blocks = -1;
    const int64_t total = cloud_table_build(seg.data(), m, T, nullptr, &blocks);          // the sizes first, as the library asks for them
    int64_t want = 0;
    bool ok = true;
    for (int k = 0; k < m; k++) { ok = ok && seg[k].off == want && seg[k].n == n[k]; want += n[k]; }
    ok = ok && total == want && blocks == (want + T - 1) / T;
    if (!ok) return false;
    vector<int32_t> blk((size_t)blocks);          // exactly: nothing behind it may be written
    int64_t again = -1;
    if (cloud_table_build(seg.data(), m, T, blk.data(), &again) != total || again != blocks) return false;
    auto holds = [&](int64_t b, int k) { return seg[k].off <= b * T && b * T < seg[k].off + seg[k].n; };
    auto block_ok = [&](int64_t b) {
        if (blk[b] < 0 || blk[b] >= m || !holds(b, blk[b])) return false;
        int owners = 0;
        for (int k = 0; k < m; k++) owners += holds(b, k) ? 1 : 0;          // the quadratic definition: exactly one cloud holds the block's first point
        return owners == 1;
    };
    for (int64_t b = 0; b < blocks; b++) ok = ok && block_ok(b);
    return ok;
}
static string name_of(const char* what, const vector<int32_t>& n, int T)
{
    string s = string(what) + " (";
    for (size_t k = 0; k < n.size(); k++) s += (k ? ", " : "") + to_string(n[k]);
    return s + ") T = " + to_string(T);
}
static void table_case(const char* what, const vector<int32_t>& n, int T = 256) { check(table_ok(n, T), name_of(what, n, T)); }

// the two loops cloud_count and cloud_total_check replaced, as they stood in ssm_render_host.cpp and ssm_align_host.cpp: -1 a negative count, -2 beyond the stage's bound, else the total
static int64_t render_total_before(const vector<int32_t>& n)
{
    int64_t t = 0;
    for (size_t k = 0; k < n.size(); k++) { if (n[k] < 0) return -1; t += n[k]; }
    return t >= ((int64_t)1 << 32) ? -2 : t;
}
static int64_t align_total_before(const ssm_alignc::Setup& S, const vector<int32_t>& n, int stride)
{
    int64_t t = 0;
    for (size_t k = 0; k < n.size(); k++) { if (n[k] < 0) return -1; t += ((int64_t)n[k] + stride - 1) / stride; }
    return ssm_alignc::sums_fit(S, t) ? t : -2;
}
// cloud_total_check under a stage's rule (the bounds of ssm_render_host.cpp and ssm_align_host.cpp), told apart by the message it hands to host_fail
static string g_err;
int host_fail(ssm_ctx*, int code, const std::string& msg) { g_err = msg; return code; }
static int64_t total_now(const CloudRule& R, const vector<int32_t>& n)
{
    int64_t t = -9;
    if (cloud_total_check(nullptr, R, n.data(), (int)n.size(), &t) == SSM_OK) return t;
    return g_err == R.negative_msg ? -1 : -2;
}
static int64_t render_total_now(const vector<int32_t>& n) { return total_now({nullptr, 1, (int64_t)1 << 32, nullptr, "negative", "bound"}, n); }
static int64_t align_total_now(const ssm_alignc::Setup& S, const vector<int32_t>& n, int stride) { return total_now({nullptr, stride, 0, &S, "negative", "bound"}, n); }

int main()
{
    // the size lists of tests/test_gpu_carve.py, test_gpu_render.py and test_gpu_align.py
    for (const vector<int32_t>& n : {vector<int32_t>{0}, {0, 0, 5}, {40, 0, 150, 66, 0, 257, 1}, {256, 256}, {257, 511, 64}}) table_case("gpu test sizes", n);
    table_case("no cloud", {});
    table_case("all clouds empty", {0, 0, 0, 0});
    table_case("empty clouds first", {0, 0, 300, 10});
    table_case("empty clouds last", {300, 10, 0, 0});
    table_case("several empty clouds in a row", {5, 0, 0, 0, 700, 0, 0, 3});
    table_case("an empty cloud on a block boundary", {256, 0, 256, 0, 0, 1});
    for (int T : {64, 256}) {
        table_case("T - 1", {T - 1, T - 1, T - 1}, T); table_case("T", {T, T, T}, T); table_case("T + 1", {T + 1, T + 1, T + 1}, T);
        table_case("sizes around T", {T - 1, T, T + 1, T, T - 1, 1, 2 * T}, T);
        table_case("a cloud boundary on a block boundary", {3 * T, 5, 2 * T - 5, T}, T);
    }
    table_case("one block crossed by three boundaries", {100, 3, 0, 2, 300});
    table_case("one block that holds five clouds", {1, 1, 1, 1, 1});
    table_case("single points and T = 1", {1, 0, 1, 2}, 1);
    // alignment: the points used are every stride-th of a cloud
    for (int stride : {1, 3, 7}) {
        vector<int32_t> n;
        for (int raw : {40, 0, 150, 66, 0, 257, 1, 256 * stride, 256 * stride + 1, 1791}) n.push_back((raw + stride - 1) / stride);
        table_case(("strided counts, stride " + to_string(stride)).c_str(), n);
    }
    // pseudo-random lists
    {
        uint64_t s = 12345; bool ok = true;
        auto next = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); };
        for (int round = 0; round < 200; round++) {
            vector<int32_t> n(next() % 9);
            for (int32_t& v : n) v = next() % 4 == 0 ? 0 : (int32_t)(next() % 600);
            const int T = 1 + next() % 300;
            if (!table_ok(n, T)) { ok = false; printf("     %s\n", name_of("random", n, T).c_str()); }
        }
        check(ok, "200 random lists of up to 8 clouds, T in 1..300");
    }
    // three clouds of 2^30 points: 12.6 M blocks, offsets and products beyond 2^31
    {
        const int32_t big = (int32_t)1 << 30;
        check(table_ok({big, big, big}, 256), "three clouds of 2^30 points, T = 256");
        check(table_ok({big - 1, 0, big, 1, big}, 4096), "2^30 - 1, 0, 2^30, 1, 2^30 points, T = 4096");
    }
    // the point count of the host-array calls (the cases of tests/test_render.py and tests/test_align.py among them)
    {
        const int32_t big = 2147483647;
        ssm_alignc::Setup S{}; S.fx = 60; S.fy = 60; S.cx = 33; S.cy = 17; S.scale = 1000; S.z_min = 0.1; S.z_max = 80.0; S.dist_max = 0.25; S.delta = 0.05; S.w = 67; S.h = 35;
        ssm_alignc::Setup Sfar = S; Sfar.z_max = 1.0e5;
        ssm_alignc::Setup Snone = S; Snone.z_max = 1.0e9;
        const vector<vector<int32_t>> lists = {{}, {0}, {1, 1, 1}, {1, -1, 1}, {-1}, {5, 0, 7}, {big, big, 2}, {big, big, 1}, {big, big, big}, {big}, {0, 0, -3}, {100, 200, 300}};
        bool r_ok = true, a_ok = true;
        for (const vector<int32_t>& n : lists) {
            r_ok = r_ok && render_total_now(n) == render_total_before(n);
            for (int stride : {1, 3, 7, 1 << 20}) for (const ssm_alignc::Setup* s : {&S, &Sfar, &Snone}) a_ok = a_ok && align_total_now(*s, n, stride) == align_total_before(*s, n, stride);
        }
        check(r_ok, "rendering's point count as before");
        check(a_ok, "alignment's point count as before, strides 1, 3, 7, 2^20");
        check(render_total_now({1, -1, 1}) == -1 && render_total_now({big, big, 2}) == -2 && render_total_now({big, big, 1}) == ((int64_t)1 << 32) - 1, "rendering: a negative count, 2^32 exactly, one below");
        check(align_total_now(S, {1, -1, 1}, 1) == -1 && align_total_now(Sfar, {big, big, big}, 1) == -2 && align_total_now(Sfar, {1, 1, 1}, 1) == 3 && align_total_now(Snone, {1}, 1) == -2 &&
              align_total_now(S, {10, 11, 0}, 3) == 8, "alignment: a negative count, the 2^62 bound, the stride");
        int64_t t = -9;
        check(cloud_count(nullptr, 0, 1, &t) && t == 0, "no cloud counts 0");
    }
    printf(failures ? "%d FAILED\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
