// ssm_uvd.hip -- UVDisparity::Process (reference include/uvdisparity.hpp, src/uvdisparity.cpp:842-903, src/stereo.cpp:41-192) behind the C ABI: the moving-object,
// ROI and ground masks and the pitch of stereo frames.  DESIGN.md s.11 is the contract.  A call is three device phases (kernels_uvd.hip) around two host
// steps (ssm_uvd_host.inc), one wait per phase; ssm_uvd_process_host runs the per-pixel stages on the CPU from the same include/ssm/uvd_core.h.
#include "ssm_ctx.h"
#include "../../include/ssm/uvd_core.h"
#include <algorithm>
#include <chrono>
#include <climits>
#include "ssm_uvd_host.inc"

struct ssm_uvd {
    ssm_ctx* c = nullptr;                       // null: a host-only object (ssm_uvd_process_host)
    ssm_uvd_params p{};
    UvdKalman kf1, kf2;
    double rate[ssm_uvdc::MAX_BINS];             // adjustUdisIntense's sigmoid(row, 0.02, 32) per U-disparity row
    std::vector<UvdFrame> frames;               // the last call
    bool record = false;                        // ssm_debug_uvd_record: keep the masks found / merged / kept of every frame for ssm_debug_uvd_stage
    double call_ms[3] = {0, 0, 0};              // the last device call: host step 1, host step 2, the whole call (ssm_debug_uvd_times)
    // device workspaces, sized for (cap_n frames of cap_px pixels, cap_w columns, cap_m matches per frame)
    int cap_n = 0, cap_m = 0, cap_w = 0, cap_h = 0;
    DevBuf<uint8_t> d_vdis, d_uraw, d_uadj, d_uni, d_left, d_moving, d_roi, d_ground; DevBuf<int16_t> d_disp;
    DevBuf<int32_t> d_maxmin, d_coords, d_nmatch, d_probes, d_counts; DevBuf<ssm_uvdc::FrameK> d_K; DevBuf<double> d_rate;
    PinBuf<uint8_t> h_vdis, h_u; PinBuf<int32_t> h_maxmin, h_coords, h_nmatch, h_probes, h_counts; PinBuf<ssm_uvdc::FrameK> h_K;
};

extern "C" void ssm_uvd_params_default(ssm_uvd_params* p) { if (p) uvd_set_defaults(p); }
extern "C" int ssm_uvd_create(ssm_ctx* c, const ssm_uvd_params* params, ssm_uvd** out)
{
    if (!out) return SSM_E_INVAL;
    *out = nullptr;
    if (!params) { if (c) c->err = "uvd: null parameters"; else g_create_err = "uvd: null parameters"; return SSM_E_INVAL; }
    if (!(params->f > 0)) { if (c) c->err = "uvd: the focal length must be positive"; else g_create_err = "uvd: the focal length must be positive"; return SSM_E_INVAL; }
    std::unique_ptr<ssm_uvd> u(new ssm_uvd());
    u->c = c; u->p = *params;
    uvd_rate_table(u->rate);
    if (c) {
        std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
        DALLOC(c, u->d_rate, ssm_uvdc::MAX_BINS);
        HIPCHK(c, hipMemcpyAsync(u->d_rate, u->rate, sizeof u->rate, hipMemcpyHostToDevice, c->main.stream));
        HIPCHK(c, hipStreamSynchronize(c->main.stream));
    }
    *out = u.release();
    return SSM_OK;
}
extern "C" void ssm_uvd_destroy(ssm_uvd* u)
{
    if (!u) return;
    if (u->c) { std::lock_guard<std::mutex> lk(u->c->mu); hipSetDevice(u->c->device); (void)hipStreamSynchronize(u->c->main.stream); }
    delete u;
}
extern "C" int ssm_uvd_reset(ssm_uvd* u)
{
    if (!u) return SSM_E_INVAL;
    std::unique_lock<std::mutex> lk; if (u->c) lk = std::unique_lock<std::mutex>(u->c->mu);
    u->kf1 = UvdKalman(); u->kf2 = UvdKalman();
    return SSM_OK;
}
extern "C" int ssm_debug_uvd_record(ssm_uvd* u, int on) { if (!u) return SSM_E_INVAL; u->record = on != 0; return SSM_OK; }

// ---------------------------------------------------------------- the whole pipeline on the CPU
extern "C" int ssm_uvd_process_host(ssm_uvd* u, const uint8_t* left, const int16_t* disp, int w, int h, int stride, ssm_pmatch* matches, uint8_t* inlier_flags,
                                    int n_matches, uint8_t* moving, uint8_t* roi, uint8_t* ground, ssm_uvd_info* info)
{
    if (!u) return SSM_E_INVAL;
    u->frames.resize(1);
    return uvd_process_host(u->p, u->rate, u->kf1, u->kf2, u->frames[0], left, disp, w, h, stride, matches, inlier_flags, n_matches, moving, roi, ground, info, u->record);
}

// ---------------------------------------------------------------- the device path
static int uvd_reserve(ssm_uvd* u, int n, int w, int h, int cap, bool own_images)
{
    using namespace ssm_uvdc;
    ssm_ctx* c = u->c;
    if (n > u->cap_n || w != u->cap_w || h != u->cap_h) {
        HIPCHK(c, hipStreamSynchronize(c->main.stream));
        const int nn = std::max(n, u->cap_n);
        const size_t px = (size_t)w * h;
        DALLOC(c, u->d_vdis, (size_t)nn * h * MAX_BINS); DALLOC(c, u->h_vdis, (size_t)nn * h * MAX_BINS);
        DALLOC(c, u->d_uraw, (size_t)nn * MAX_BINS * w); DALLOC(c, u->d_uadj, (size_t)nn * MAX_BINS * w); DALLOC(c, u->d_uni, (size_t)nn * MAX_BINS * w);
        DALLOC(c, u->h_u, (size_t)nn * MAX_BINS * w * 2);            // the raw image of every frame, then the adjusted one; the union masks go up through the first half
        DALLOC(c, u->d_moving, nn * px); DALLOC(c, u->d_roi, nn * px); DALLOC(c, u->d_ground, nn * px);
        DALLOC(c, u->d_maxmin, (size_t)nn * 2); DALLOC(c, u->h_maxmin, (size_t)nn * 2); DALLOC(c, u->d_counts, nn); DALLOC(c, u->h_counts, nn);
        DALLOC(c, u->d_K, nn); DALLOC(c, u->h_K, nn); DALLOC(c, u->d_nmatch, nn); DALLOC(c, u->h_nmatch, nn);
        u->d_left.reset(); u->d_disp.reset(); u->cap_m = 0;
        u->cap_n = nn; u->cap_w = w; u->cap_h = h;
    }
    if (cap > u->cap_m) {
        HIPCHK(c, hipStreamSynchronize(c->main.stream));
        const size_t m = (size_t)u->cap_n * cap;
        DALLOC(c, u->d_coords, m * 2); DALLOC(c, u->h_coords, m * 2); DALLOC(c, u->d_probes, m); DALLOC(c, u->h_probes, m);
        u->cap_m = cap;
    }
    if (own_images && !u->d_left) { DALLOC(c, u->d_left, (size_t)u->cap_n * w * h); DALLOC(c, u->d_disp, (size_t)u->cap_n * w * h); }
    return SSM_OK;
}
// lk: the context's lock, held by the caller.  It is released around the two host steps -- they touch only what belongs to the uvd object -- so other threads
// of the context (the mapper, an asynchronous matcher) are not held up by them; a uvd object itself serves one thread at a time
static int uvd_run_dev(std::unique_lock<std::mutex>& lk, ssm_uvd* u, const uint8_t* left_dev, const int16_t* disp_dev, int n, int w, int h, ssm_pmatch* matches, const int32_t* nmatch, uint8_t* flags, int cap,
                       uint8_t* moving_dev, uint8_t* roi_dev, uint8_t* ground_dev, ssm_uvd_info* info)
{
    using namespace ssm_uvdc;
    ssm_ctx* c = u->c; hipStream_t s = c->main.stream;
    const size_t px = (size_t)w * h;
    typedef std::chrono::steady_clock clk;
    auto ms_since = [](clk::time_point a) { return std::chrono::duration<double, std::milli>(clk::now() - a).count(); };
    const clk::time_point t_call = clk::now();
    uint8_t* d_moving = moving_dev ? moving_dev : (uint8_t*)u->d_moving; uint8_t* d_roi = roi_dev ? roi_dev : (uint8_t*)u->d_roi; uint8_t* d_ground = ground_dev ? ground_dev : (uint8_t*)u->d_ground;
    u->frames.resize(n);
    // phase 1: the V-disparity rows and the extremes
    for (int f = 0; f < n; f++) { u->h_maxmin[2 * f] = INT_MIN; u->h_maxmin[2 * f + 1] = INT_MAX; u->h_nmatch[f] = std::min(nmatch[f], cap); }
    HIPCHK(c, hipMemcpyAsync(u->d_maxmin, u->h_maxmin, (size_t)n * 8, hipMemcpyHostToDevice, s));
    prof_begin(c, s, "uvd_vdisp");
    HIPCHK(c, k_uvd_vdisp(disp_dev, n, w, h, u->d_vdis, u->d_maxmin, s));
    prof_end(c, s);
    HIPCHK(c, hipMemcpyAsync(u->h_vdis, u->d_vdis, (size_t)n * h * MAX_BINS, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(u->h_maxmin, u->d_maxmin, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    // host step 1, in frame order: the Kalman filters run through the frames
    clk::time_point t_host = clk::now();
    lk.unlock();
    for (int f = 0; f < n; f++) {
        UvdFrame& F = u->frames[f];
        F.w = w; F.h = h; F.max_disp = u->h_maxmin[2 * f];
        F.v_dis.assign(u->h_vdis + (size_t)f * h * MAX_BINS, u->h_vdis + (size_t)(f + 1) * h * MAX_BINS);
        uvd_host_step1(u->p, u->kf1, u->kf2, F, u->h_maxmin[2 * f + 1], nmatch[f] < 0);
        u->h_K[f] = F.k;
    }
    u->call_ms[0] = ms_since(t_host);
    lk.lock(); hipSetDevice(c->device);
    // phase 2: the masks, the U-disparity images, the probes
    for (int f = 0; f < n; f++) for (int i = 0; i < u->h_nmatch[f]; i++) {
        const ssm_pmatch& m = matches[(size_t)f * cap + i];
        u->h_coords[((size_t)f * cap + i) * 2] = (int)m.u1c; u->h_coords[((size_t)f * cap + i) * 2 + 1] = (int)m.v1c;
    }
    HIPCHK(c, hipMemcpyAsync(u->d_K, u->h_K, (size_t)n * sizeof(FrameK), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(u->d_nmatch, u->h_nmatch, (size_t)n * 4, hipMemcpyHostToDevice, s));
    if (cap) HIPCHK(c, hipMemcpyAsync(u->d_coords, u->h_coords, (size_t)n * cap * 8, hipMemcpyHostToDevice, s));
    prof_begin(c, s, "uvd_classify");
    HIPCHK(c, k_uvd_classify(left_dev, disp_dev, n, w, h, u->d_K, uvd_calib(u->p), uvd_roi(u->p), u->d_rate, d_ground, d_roi, u->d_uraw, u->d_uadj, s));
    HIPCHK(c, k_uvd_probe(d_roi, disp_dev, n, w, h, u->d_coords, u->d_nmatch, cap, u->d_probes, s));
    prof_end(c, s);
    const size_t ustride = (size_t)MAX_BINS * w;
    uint8_t* h_raw = u->h_u; uint8_t* h_adj = u->h_u + (size_t)u->cap_n * ustride;
    for (int f = 0; f < n; f++) {
        if (!u->frames[f].k.run) continue;
        const size_t bytes = (size_t)u->frames[f].k.u_rows * w;
        HIPCHK(c, hipMemcpyAsync(h_raw + f * ustride, u->d_uraw + f * ustride, bytes, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(h_adj + f * ustride, u->d_uadj + f * ustride, bytes, hipMemcpyDeviceToHost, s));
    }
    if (cap) HIPCHK(c, hipMemcpyAsync(u->h_probes, u->d_probes, (size_t)n * cap * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    // host step 2
    t_host = clk::now();
    lk.unlock();
    std::vector<uint8_t> pr(cap ? cap : 1); std::vector<int16_t> pd(cap ? cap : 1);
    for (int f = 0; f < n; f++) {
        UvdFrame& F = u->frames[f];
        if (F.k.run) {
            const size_t bytes = (size_t)F.k.u_rows * w;
            F.u_raw.assign(h_raw + f * ustride, h_raw + f * ustride + bytes); F.u_adj.assign(h_adj + f * ustride, h_adj + f * ustride + bytes);
            const int nm = u->h_nmatch[f];
            for (int i = 0; i < nm; i++) { const int32_t v = u->h_probes[(size_t)f * cap + i]; pr[i] = (uint8_t)(v >> 16); pd[i] = (int16_t)(v & 0xFFFF); }
            uvd_host_step2(u->p, F, matches + (size_t)f * cap, flags + (size_t)f * cap, nm, pr.data(), pd.data(), u->record);
            if (F.k.run) memcpy(h_raw + f * ustride, F.uni.data(), bytes);           // (the raw image has been copied out: its staging carries the union mask up)
        }
        u->h_K[f] = F.k; u->h_counts[f] = 0;
    }
    u->call_ms[1] = ms_since(t_host);
    lk.lock(); hipSetDevice(c->device);
    // phase 3: the moving mask
    HIPCHK(c, hipMemcpyAsync(u->d_K, u->h_K, (size_t)n * sizeof(FrameK), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(u->d_counts, u->h_counts, (size_t)n * 4, hipMemcpyHostToDevice, s));
    for (int f = 0; f < n; f++)
        if (u->frames[f].k.run) HIPCHK(c, hipMemcpyAsync(u->d_uni + f * ustride, h_raw + f * ustride, (size_t)u->frames[f].k.u_rows * w, hipMemcpyHostToDevice, s));
    prof_begin(c, s, "uvd_segment");
    HIPCHK(c, k_uvd_segment(disp_dev, d_roi, u->d_uni, n, w, h, u->d_K, d_moving, u->d_counts, s));
    prof_end(c, s);
    HIPCHK(c, hipMemcpyAsync(u->h_counts, u->d_counts, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    for (int f = 0; f < n; f++) { u->frames[f].info.n_moving = u->h_counts[f]; info[f] = u->frames[f].info; }
    u->call_ms[2] = ms_since(t_call);
    return SSM_OK;
}

extern "C" int ssm_uvd_process_dev(ssm_uvd* u, const uint8_t* left_dev, const int16_t* disp_dev, int n, int w, int h, ssm_pmatch* matches, const int32_t* nmatch,
                                   uint8_t* inlier_flags, int cap, uint8_t* moving_dev, uint8_t* roi_dev, uint8_t* ground_dev, ssm_uvd_info* info)
{
    if (!u || !u->c) return SSM_E_INVAL;
    ssm_ctx* c = u->c; std::unique_lock<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (n < 0 || w < 1 || h < 1 || h > 32767 || cap < 0 || (n > 0 && (!left_dev || !disp_dev || !nmatch || !info)) || (n > 0 && cap > 0 && (!matches || !inlier_flags))) FAIL(c, SSM_E_INVAL, "bad arguments");
    if (n > 65535) FAIL(c, SSM_E_INVAL, "uvd: at most 65535 frames per call");
    if (n == 0) { u->frames.clear(); return SSM_OK; }
    { const int r = uvd_reserve(u, n, w, h, cap, false); if (r) return r; }
    return uvd_run_dev(lk, u, left_dev, disp_dev, n, w, h, matches, nmatch, inlier_flags, cap, moving_dev, roi_dev, ground_dev, info);
}
extern "C" int ssm_uvd_process(ssm_uvd* u, const uint8_t* left, const int16_t* disp, int w, int h, int stride, ssm_pmatch* matches, uint8_t* inlier_flags,
                               int n_matches, uint8_t* moving, uint8_t* roi, uint8_t* ground, ssm_uvd_info* info)
{
    if (!u || !u->c) return SSM_E_INVAL;
    ssm_ctx* c = u->c; std::unique_lock<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (!left || !disp || w < 1 || h < 1 || h > 32767 || stride < w || (n_matches > 0 && (!matches || !inlier_flags)) || !info) FAIL(c, SSM_E_INVAL, "bad arguments");
    { const int r = uvd_reserve(u, 1, w, h, std::max(n_matches, 0), true); if (r) return r; }
    hipStream_t s = c->main.stream;
    HIPCHK(c, hipMemcpy2DAsync(u->d_left, (size_t)w, left, (size_t)stride, (size_t)w, h, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpy2DAsync(u->d_disp, (size_t)w * 2, disp, (size_t)stride * 2, (size_t)w * 2, h, hipMemcpyHostToDevice, s));
    const int32_t nm = n_matches;
    { const int r = uvd_run_dev(lk, u, u->d_left, u->d_disp, 1, w, h, matches, &nm, inlier_flags, std::max(n_matches, 0), nullptr, nullptr, nullptr, info); if (r) return r; }
    const size_t px = (size_t)w * h;
    if (moving) HIPCHK(c, hipMemcpyAsync(moving, u->d_moving, px, hipMemcpyDeviceToHost, s));
    if (roi) HIPCHK(c, hipMemcpyAsync(roi, u->d_roi, px, hipMemcpyDeviceToHost, s));
    if (ground) HIPCHK(c, hipMemcpyAsync(ground, u->d_ground, px, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return SSM_OK;
}

// ---------------------------------------------------------------- what the tests look at
extern "C" int ssm_debug_uvd_images(ssm_uvd* u, int frame, uint8_t* v_dis, uint8_t* u_dis, uint8_t* bin, uint8_t* union_mask)
{
    using namespace ssm_uvdc;
    if (!u || frame < 0 || frame >= (int)u->frames.size()) return SSM_E_INVAL;
    const UvdFrame& F = u->frames[frame];
    if (v_dis) memcpy(v_dis, F.v_dis.data(), F.v_dis.size());
    if (u_dis && !F.u_adj.empty()) memcpy(u_dis, F.u_adj.data(), F.u_adj.size());
    if (bin) {
        memset(bin, 0, (size_t)F.h * MAX_BINS);
        if (!F.bin.empty()) for (int r = 0; r < F.h; r++) memcpy(bin + (size_t)r * MAX_BINS, F.bin.data() + (size_t)r * F.info.v_cols, F.info.v_cols);
    }
    if (union_mask && !F.uni.empty()) memcpy(union_mask, F.uni.data(), F.uni.size());
    return SSM_OK;
}
extern "C" int ssm_debug_uvd_times(ssm_uvd* u, double ms[3])
{
    if (!u || !ms) return SSM_E_INVAL;
    for (int i = 0; i < 3; i++) ms[i] = u->call_ms[i];
    return SSM_OK;
}
extern "C" int ssm_debug_uvd_stage(ssm_uvd* u, int frame, int stage, void* out, size_t cap, size_t* bytes)
{
    if (!u || frame < 0 || frame >= (int)u->frames.size() || !bytes) return SSM_E_INVAL;
    const UvdFrame& F = u->frames[frame];
    std::vector<uint8_t> cat;
    const void* src = nullptr; size_t n = 0;
    auto img = [&](const UvdImg& v) { src = v.data(); n = v.size(); };
    auto list = [&](const std::vector<UvdImg>& l) { for (const UvdImg& v : l) cat.insert(cat.end(), v.begin(), v.end()); src = cat.data(); n = cat.size(); };
    if (stage >= 8 && stage <= 10 && !u->record) return SSM_E_INVAL;          // not recorded: ssm_debug_uvd_record
    switch (stage) {
    case 1: img(F.blur); break;
    case 2: img(F.erode); break;
    case 3: img(F.bin); break;
    case 4: src = F.pts.data(); n = F.pts.size() * 4; break;
    case 5: img(F.u_raw); break;
    case 7: src = F.areas.data(); n = F.areas.size() * 4; break;
    case 8: list(F.found); break;
    case 9: list(F.merged); break;
    case 10: list(F.kept); break;
    default: return SSM_E_INVAL;
    }
    *bytes = n;
    if (!out) return SSM_OK;
    if (n > cap) return SSM_E_CAPACITY;
    if (n) memcpy(out, src, n);
    return SSM_OK;
}
