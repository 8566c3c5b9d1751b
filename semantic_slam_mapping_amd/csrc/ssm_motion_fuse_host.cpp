// ssm_motion_fuse_host.cpp -- the semantic-motion fusion on the CPU: ssm_motion_fuse_host, the parameter defaults and the argument check the
// device entry points share.  Plain C++ over include/ssm/motion_fuse_core.h; the blobs are found with two flood fills, which has nothing in common with the
// device's union-find but the contract: the label of a blob is its smallest row-major index, which a row-major scan meets first.
#include "ssm_host.h"
using namespace ssm_mfc;

extern "C" void ssm_motion_fuse_params_default(ssm_motion_fuse_params* p) { if (!p) return; p->area_thres = 1000; p->pad = 0; p->overlay_thres = 0.143; }
extern "C" void ssm_motion_fuse_tile(int32_t wh[2]) { if (!wh) return; wh[0] = TILE_W; wh[1] = TILE_H; }
int mf_check(ssm_ctx* c, int n, int w, int h, size_t stride)
{
    if (n < 0 || w < 1 || h < 1) return host_fail(c, SSM_E_INVAL, "motion_fuse: bad arguments");
    if ((size_t)w * h > ((size_t)1 << 28)) return host_fail(c, SSM_E_INVAL, "motion_fuse: at most 2^28 pixels per frame");
    if (stride < (size_t)w * 3) return host_fail(c, SSM_E_INVAL, "stride smaller than a row");
    if (n > 65535) return host_fail(c, SSM_E_INVAL, "motion_fuse: at most 65535 frames per call");
    return SSM_OK;
}

extern "C" int ssm_motion_fuse_host(const uint8_t* sem, const uint8_t* motion, int w, int h, int stride, const ssm_motion_fuse_params* params, uint8_t* mask,
                                    ssm_motion_fuse_info* info, int32_t* labels, int32_t* area, int32_t* overlap, uint8_t* cand_out)
{
    if (!sem || !mask) return host_fail(nullptr, SSM_E_INVAL, "null argument");
    { const int r = mf_check(nullptr, 1, w, h, (size_t)(stride < 0 ? 0 : stride)); if (r) return r; }
    ssm_motion_fuse_params P; ssm_motion_fuse_params_default(&P); if (params) P = *params;
    const size_t px = (size_t)w * h;
    // the class bits and their 5 x 5 box dilation (two passes of the full 3 x 3), separable
    std::vector<uint8_t> bits(px), rowor(px), always(px), cand(px);
    for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) { const uint8_t* p = sem + (size_t)y * stride + (size_t)x * 3; bits[(size_t)y * w + x] = (uint8_t)class_bits(p[0], p[1], p[2]); }
    for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) {
        int o = 0;
        for (int k = std::max(x - 2, 0); k <= std::min(x + 2, w - 1); k++) o |= bits[(size_t)y * w + k];
        rowor[(size_t)y * w + x] = (uint8_t)o;
    }
    for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) {
        int o = 0;
        for (int k = std::max(y - 2, 0); k <= std::min(y + 2, h - 1); k++) o |= rowor[(size_t)k * w + x];
        always[(size_t)y * w + x] = (o & CLASS_ALWAYS) ? 255 : 0; cand[(size_t)y * w + x] = (o & CLASS_CAND) ? 255 : 0;
    }
    // outside: the zero pixels of cand that reach the image frame over zero pixels, 4-connected
    std::vector<uint8_t> outside(px, 0); std::vector<int32_t> stack;
    auto seed = [&](int x, int y) { const size_t at = (size_t)y * w + x; if (!cand[at] && !outside[at]) { outside[at] = 1; stack.push_back((int32_t)at); } };
    for (int x = 0; x < w; x++) { seed(x, 0); seed(x, h - 1); }
    for (int y = 0; y < h; y++) { seed(0, y); seed(w - 1, y); }
    while (!stack.empty()) {
        const int32_t at = stack.back(); stack.pop_back();
        const int x = at % w, y = at / w;
        if (x > 0) seed(x - 1, y);
        if (x + 1 < w) seed(x + 1, y);
        if (y > 0) seed(x, y - 1);
        if (y + 1 < h) seed(x, y + 1);
    }
    // the blobs: 8-connected sets of what is not outside, in row-major order of their first pixel
    std::vector<int32_t> lab(px, -1), ar(px, 0), ov(px, 0);
    ssm_motion_fuse_info I{0, 0, 0, 0};
    std::vector<uint8_t> conf(px, 0);          // at the root
    for (size_t s = 0; s < px; s++) {
        if (outside[s] || lab[s] >= 0) continue;
        int32_t a = 0, o = 0;
        lab[s] = (int32_t)s; stack.push_back((int32_t)s);
        while (!stack.empty()) {
            const int32_t at = stack.back(); stack.pop_back();
            a++; if (motion && motion_hit(motion[at])) o++;
            const int x = at % w, y = at / w;
            for (int dy = -1; dy <= 1; dy++) for (int dx = -1; dx <= 1; dx++) {
                const int nx = x + dx, ny = y + dy;
                if (nx < 0 || ny < 0 || nx >= w || ny >= h) continue;
                const size_t q = (size_t)ny * w + nx;
                if (outside[q] || lab[q] >= 0) continue;
                lab[q] = (int32_t)s; stack.push_back((int32_t)q);
            }
        }
        ar[s] = a; ov[s] = o;
        I.blobs++; I.large += is_large(a, P.area_thres);
        if (confirmed(a, o, P.area_thres, P.overlay_thres)) { conf[s] = 1; I.confirmed++; }
    }
    for (size_t s = 0; s < px; s++) {
        const uint8_t m = always[s] | ((lab[s] >= 0 && conf[lab[s]]) ? 255 : 0);
        mask[s] = m; I.added += m && !always[s];
    }
    if (info) *info = I;
    if (labels) memcpy(labels, lab.data(), px * 4);
    if (area) memcpy(area, ar.data(), px * 4);
    if (overlap) memcpy(overlap, ov.data(), px * 4);
    if (cand_out) memcpy(cand_out, cand.data(), px);
    return SSM_OK;
}
