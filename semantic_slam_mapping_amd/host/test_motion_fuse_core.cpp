// test_motion_fuse_core.cpp -- the semantic-motion fusion on the host (csrc/ssm_motion_fuse_host.cpp over include/ssm/motion_fuse_core.h) as a stand-alone
// program: linked with that one source, it needs neither libssm_hip.so nor a GPU and runs as it is under the CPU sanitizers (-fsanitize=address,undefined).
// Checked here, from C++: hand-made shapes with known figures, the decision's edges, sizes down to one pixel, strided rows, invalid arguments, and random images
// against a restatement by relaxation (every pixel takes the smallest label around it until nothing changes).
#include "ssm_hip.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
// what the host source asks of its surroundings (csrc/ssm_host.h): the error path
static std::string g_err;
int host_fail(ssm_ctx*, int code, const std::string& msg) { g_err = msg; return code; }
using namespace std;

static int failures = 0;
static void check(bool ok, const char* name) { printf("%s %s\n", ok ? "PASS" : "FAIL", name); if (!ok) failures++; }
struct Rng { uint64_t s; uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); } };
static const uint8_t CAR[3] = {128, 0, 64}, PED[3] = {0, 64, 64}, BIKE[3] = {192, 128, 0};

struct Img {
    int w, h; vector<uint8_t> sem, motion;
    Img(int w_, int h_) : w(w_), h(h_), sem((size_t)w_ * h_ * 3, 128), motion((size_t)w_ * h_, 0) {}
    void set(int x, int y, const uint8_t* c) { memcpy(&sem[((size_t)y * w + x) * 3], c, 3); }
};
struct Out { vector<uint8_t> mask, cand; vector<int32_t> lab, area, ov; ssm_motion_fuse_info info; int rc; };
static Out run(const Img& I, int area_thres, double overlay_thres, bool with_motion = true)
{
    Out o; const size_t px = (size_t)I.w * I.h;
    o.mask.assign(px, 7); o.cand.assign(px, 7); o.lab.assign(px, 7); o.area.assign(px, 7); o.ov.assign(px, 7);
    ssm_motion_fuse_params P; ssm_motion_fuse_params_default(&P); P.area_thres = area_thres; P.overlay_thres = overlay_thres;
    o.rc = ssm_motion_fuse_host(I.sem.data(), with_motion ? I.motion.data() : nullptr, I.w, I.h, I.w * 3, &P, o.mask.data(), &o.info, o.lab.data(), o.area.data(), o.ov.data(), o.cand.data());
    return o;
}
// the restatement: dilation by definition, outside and blobs by relaxation
static bool restated(const Img& I, int area_thres, double overlay_thres, const Out& o)
{
    const int w = I.w, h = I.h; const size_t px = (size_t)w * h;
    vector<uint8_t> always(px, 0), cand(px, 0);
    for (int y = 0; y < h; y++) for (int x = 0; x < w; x++)
        for (int dy = -2; dy <= 2; dy++) for (int dx = -2; dx <= 2; dx++) {
            const int nx = x + dx, ny = y + dy;
            if (nx < 0 || ny < 0 || nx >= w || ny >= h) continue;
            const uint8_t* p = &I.sem[((size_t)ny * w + nx) * 3];
            const bool ped = (p[0] == 0 && p[1] == 64 && p[2] == 64) || (p[0] == 192 && p[1] == 128 && p[2] == 0), car = p[0] == 128 && p[1] == 0 && p[2] == 64;
            if (ped) always[(size_t)y * w + x] = 255;
            if (ped || car) cand[(size_t)y * w + x] = 255;
        }
    vector<uint8_t> outside(px, 0);
    for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) if (!cand[(size_t)y * w + x] && (x == 0 || y == 0 || x == w - 1 || y == h - 1)) outside[(size_t)y * w + x] = 1;
    for (bool ch = true; ch;) {
        ch = false;
        for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) {
            const size_t at = (size_t)y * w + x;
            if (cand[at] || outside[at]) continue;
            if ((x > 0 && outside[at - 1]) || (x + 1 < w && outside[at + 1]) || (y > 0 && outside[at - w]) || (y + 1 < h && outside[at + w])) { outside[at] = 1; ch = true; }
        }
    }
    vector<int32_t> lab(px);
    for (size_t i = 0; i < px; i++) lab[i] = outside[i] ? -1 : (int32_t)i;
    for (bool ch = true; ch;) {
        ch = false;
        for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) {
            const size_t at = (size_t)y * w + x;
            if (lab[at] < 0) continue;
            for (int dy = -1; dy <= 1; dy++) for (int dx = -1; dx <= 1; dx++) {
                const int nx = x + dx, ny = y + dy;
                if (nx < 0 || ny < 0 || nx >= w || ny >= h) continue;
                const int32_t q = lab[(size_t)ny * w + nx];
                if (q >= 0 && q < lab[at]) { lab[at] = q; ch = true; }
            }
        }
    }
    vector<int32_t> area(px, 0), ov(px, 0);
    for (size_t i = 0; i < px; i++) if (lab[i] >= 0) { area[lab[i]]++; if (I.motion[i] == 255) ov[lab[i]]++; }
    ssm_motion_fuse_info info = {0, 0, 0, 0}; vector<uint8_t> mask(px);
    auto conf = [&](int32_t r) { const float f = (float)ov[r] * 1.0f / (float)(area[r] + 1); return area[r] > area_thres && (double)f > overlay_thres; };
    for (size_t i = 0; i < px; i++) {
        if (lab[i] == (int32_t)i) { info.blobs++; info.large += area[i] > area_thres; info.confirmed += conf((int32_t)i); }
        mask[i] = always[i] | ((lab[i] >= 0 && conf(lab[i])) ? 255 : 0);
        info.added += mask[i] && !always[i];
    }
    return o.rc == SSM_OK && mask == o.mask && cand == o.cand && lab == o.lab && area == o.area && ov == o.ov && memcmp(&info, &o.info, sizeof info) == 0;
}

int main()
{
    {   // one Car pixel: a 5 x 5 blob whose label is its first pixel; the area test is `>`
        Img I(20, 20); I.set(9, 9, CAR); fill(I.motion.begin(), I.motion.end(), 255);
        Out a = run(I, 25, 0.5), b = run(I, 24, 0.5);
        const int root = 7 * 20 + 7;
        check(a.rc == SSM_OK && a.info.blobs == 1 && a.lab[root] == root && a.lab[11 * 20 + 11] == root && a.lab[6 * 20 + 7] == -1 && a.area[root] == 25 && a.ov[root] == 25, "box of 25");
        check(a.info.large == 0 && a.info.confirmed == 0 && a.info.added == 0 && b.info.large == 1 && b.info.confirmed == 1 && b.info.added == 25 && b.mask[root] == 255, "area == thres is not large, thres + 1 is");
        check(restated(I, 25, 0.5, a) && restated(I, 24, 0.5, b), "box of 25: restatement");
    }
    {   // 999 pixels, mask_count 1000: 143 hits pass 0.143 in float-then-double, 142 do not; 254 is not motion
        Img I(50, 50);
        for (int y = 5; y < 38; y++) for (int x = 8; x < 31; x++) I.set(x, y, CAR);
        fill(I.motion.begin(), I.motion.end(), 254);
        int hits = 0;
        for (int y = 3; y < 40 && hits < 143; y++) for (int x = 6; x < 33 && hits < 143; x += 3) { I.motion[(size_t)y * 50 + x] = 255; hits++; }
        Out a = run(I, 500, 0.143);
        const int root = 3 * 50 + 6;
        check(hits == 143 && a.area[root] == 999 && a.ov[root] == 143 && a.info.confirmed == 1 && a.info.added == 999, "143 of 1000 is confirmed");
        for (size_t i = 0; i < I.motion.size(); i++) if (I.motion[i] == 255) { I.motion[i] = 254; break; }
        Out b = run(I, 500, 0.143);
        check(b.ov[root] == 142 && b.info.large == 1 && b.info.confirmed == 0 && b.info.added == 0, "142 of 1000 is not");
        check(!(143.0 / 1000.0 > 0.143) && (double)(143.0f * 1.0f / 1000.0f) > 0.143, "the compare is float, then double");
    }
    {   // a ring with a Pedestrian island in its hole is one filled blob; without motion the mask is the island's box alone
        Img I(80, 50);
        for (int x = 10; x < 70; x++) { I.set(x, 6, CAR); I.set(x, 43, CAR); }
        for (int y = 6; y < 44; y++) { I.set(10, y, CAR); I.set(69, y, CAR); }
        I.set(40, 25, PED);
        for (int y = 0; y < 50; y++) for (int x = 0; x < 40; x++) I.motion[(size_t)y * 80 + x] = 255;
        Out a = run(I, 300, 0.4), b = run(I, 300, 0.4, false);
        const int root = 4 * 80 + 8;
        check(a.info.blobs == 1 && a.area[root] == 64 * 42 && a.lab[25 * 80 + 40] == root && a.lab[20 * 80 + 30] == root && a.info.confirmed == 1 && a.info.added == 64 * 42 - 25, "ring with island: one filled blob");
        int set = 0; for (uint8_t m : b.mask) set += m == 255;
        check(b.info.blobs == 1 && b.info.confirmed == 0 && set == 25 && b.mask[25 * 80 + 40] == 255, "no motion: the always-moving classes alone");
        check(restated(I, 300, 0.4, a), "ring with island: restatement");
    }
    {   // a C open towards the image border is not filled
        Img I(60, 40);
        for (int x = 0; x < 30; x++) { I.set(x, 5, BIKE); I.set(x, 34, BIKE); }
        for (int y = 5; y < 35; y++) I.set(30, y, BIKE);
        Out a = run(I, 10, 0.0);
        check(a.info.blobs == 1 && a.lab[20 * 60 + 10] == -1 && a.lab[20 * 60 + 0] == -1 && a.lab[20 * 60 + 30] == 3 * 60, "a hole that touches the border is outside");
        check(restated(I, 10, 0.0, a), "open C: restatement");
    }
    {   // sizes down to one pixel, random content
        Rng r{12345}; bool ok = true;
        const int sizes[][2] = {{1, 1}, {1, 70}, {70, 1}, {2, 2}, {5, 3}, {67, 35}, {64, 16}, {65, 17}, {129, 33}};
        for (auto& s : sizes) for (int rep = 0; rep < 3; rep++) {
            Img I(s[0], s[1]);
            for (int y = 0; y < I.h; y++) for (int x = 0; x < I.w; x++) {
                const uint32_t v = r.next() % 1000;
                if (v < 25) I.set(x, y, v < 3 ? PED : v < 5 ? BIKE : CAR);
                I.motion[(size_t)y * I.w + x] = (r.next() % 3 == 0) ? 255 : (r.next() % 5 == 0 ? 254 : 0);
            }
            ok = ok && restated(I, 30, 0.3, run(I, 30, 0.3));
        }
        check(ok, "random images of nine sizes: restatement");
    }
    {   // strided rows; invalid arguments
        Img I(33, 9); I.set(4, 4, CAR); I.set(20, 3, PED); fill(I.motion.begin(), I.motion.end(), 255);
        Out a = run(I, 5, 0.1);
        const int stride = 33 * 3 + 11; vector<uint8_t> wide((size_t)stride * 9, 0), mask(33 * 9);
        for (int y = 0; y < 9; y++) memcpy(&wide[(size_t)y * stride], &I.sem[(size_t)y * 99], 99);
        ssm_motion_fuse_params P; ssm_motion_fuse_params_default(&P);
        check(P.area_thres == 1000 && P.overlay_thres == 0.143, "defaults");
        P.area_thres = 5; P.overlay_thres = 0.1;
        check(ssm_motion_fuse_host(wide.data(), I.motion.data(), 33, 9, stride, &P, mask.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == SSM_OK && mask == a.mask, "strided rows");
        check(ssm_motion_fuse_host(wide.data(), nullptr, 33, 9, 98, &P, mask.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == SSM_E_INVAL &&
              ssm_motion_fuse_host(nullptr, nullptr, 33, 9, 99, &P, mask.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == SSM_E_INVAL &&
              ssm_motion_fuse_host(wide.data(), nullptr, 0, 9, 99, &P, mask.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == SSM_E_INVAL && !g_err.empty(), "invalid arguments");
    }
    printf(failures ? "%d FAILED\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
