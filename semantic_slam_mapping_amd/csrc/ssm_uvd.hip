// ssm_uvd.hip -- the device path of UVDisparity::Process (reference include/uvdisparity.hpp, src/uvdisparity.cpp:842-903, src/stereo.cpp:41-192) behind the C ABI:
// the moving-object, ROI and ground masks and the pitch of stereo frames.  DESIGN.md s.11 is the contract.  A call is three device phases (kernels_uvd.hip)
// around two host steps, one wait per phase.  The object, the host steps and ssm_uvd_process_host are ssm_uvd_host.cpp; what an object with a context owns
// on the device is UvdDev here, attached and released through ssm_host.h's hooks.
#include "ssm_ctx.h"
#include "ssm_host.h"
#include <chrono>
#include <climits>

struct UvdDev {
    // device workspaces, sized for (cap_n frames of cap_px pixels, cap_w columns, cap_m matches per frame)
    int cap_n = 0, cap_m = 0, cap_w = 0, cap_h = 0;
    DevBuf<uint8_t> d_vdis, d_uraw, d_uadj, d_uni, d_left, d_moving, d_roi, d_ground; DevBuf<int16_t> d_disp;
    DevBuf<int32_t> d_maxmin, d_coords, d_nmatch, d_probes, d_counts; DevBuf<ssm_uvdc::FrameK> d_K; DevBuf<double> d_rate;
    PinBuf<uint8_t> h_vdis, h_u; PinBuf<int32_t> h_maxmin, h_coords, h_nmatch, h_probes, h_counts; PinBuf<ssm_uvdc::FrameK> h_K;
};
int uvd_dev_attach(ssm_uvd* u)
{
    ssm_ctx* c = u->c; std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    std::unique_ptr<UvdDev> D(new UvdDev());
    DALLOC(c, D->d_rate, ssm_uvdc::MAX_BINS);
    HIPCHK(c, hipMemcpyAsync(D->d_rate, u->rate, sizeof u->rate, hipMemcpyHostToDevice, c->main.stream));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    u->dev = D.release();
    return SSM_OK;
}
void uvd_dev_release(ssm_uvd* u) { { std::lock_guard<std::mutex> lk(u->c->mu); hipSetDevice(u->c->device); (void)hipStreamSynchronize(u->c->main.stream); } delete u->dev; }

// ---------------------------------------------------------------- the device path
static int uvd_reserve(ssm_uvd* u, int n, int w, int h, int cap, bool own_images)
{
    using namespace ssm_uvdc;
    ssm_ctx* c = u->c; UvdDev* D = u->dev;
    if (n > D->cap_n || w != D->cap_w || h != D->cap_h) {
        HIPCHK(c, hipStreamSynchronize(c->main.stream));
        const int nn = std::max(n, D->cap_n);
        const size_t px = (size_t)w * h;
        DALLOC(c, D->d_vdis, (size_t)nn * h * MAX_BINS); DALLOC(c, D->h_vdis, (size_t)nn * h * MAX_BINS);
        DALLOC(c, D->d_uraw, (size_t)nn * MAX_BINS * w); DALLOC(c, D->d_uadj, (size_t)nn * MAX_BINS * w); DALLOC(c, D->d_uni, (size_t)nn * MAX_BINS * w);
        DALLOC(c, D->h_u, (size_t)nn * MAX_BINS * w * 2);            // the raw image of every frame, then the adjusted one; the union masks go up through the first half
        DALLOC(c, D->d_moving, nn * px); DALLOC(c, D->d_roi, nn * px); DALLOC(c, D->d_ground, nn * px);
        DALLOC(c, D->d_maxmin, (size_t)nn * 2); DALLOC(c, D->h_maxmin, (size_t)nn * 2); DALLOC(c, D->d_counts, nn); DALLOC(c, D->h_counts, nn);
        DALLOC(c, D->d_K, nn); DALLOC(c, D->h_K, nn); DALLOC(c, D->d_nmatch, nn); DALLOC(c, D->h_nmatch, nn);
        D->d_left.reset(); D->d_disp.reset(); D->cap_m = 0;
        D->cap_n = nn; D->cap_w = w; D->cap_h = h;
    }
    if (cap > D->cap_m) {
        HIPCHK(c, hipStreamSynchronize(c->main.stream));
        const size_t m = (size_t)D->cap_n * cap;
        DALLOC(c, D->d_coords, m * 2); DALLOC(c, D->h_coords, m * 2); DALLOC(c, D->d_probes, m); DALLOC(c, D->h_probes, m);
        D->cap_m = cap;
    }
    if (own_images && !D->d_left) { DALLOC(c, D->d_left, (size_t)D->cap_n * w * h); DALLOC(c, D->d_disp, (size_t)D->cap_n * w * h); }
    return SSM_OK;
}
// lk: the context's lock, held by the caller.  It is released around the two host steps -- they touch only what belongs to the uvd object -- so other threads
// of the context (the mapper, an asynchronous matcher) are not held up by them; a uvd object itself serves one thread at a time
static int uvd_run_dev(std::unique_lock<std::mutex>& lk, ssm_uvd* u, const uint8_t* left_dev, const int16_t* disp_dev, int n, int w, int h, ssm_pmatch* matches, const int32_t* nmatch, uint8_t* flags, int cap,
                       uint8_t* moving_dev, uint8_t* roi_dev, uint8_t* ground_dev, ssm_uvd_info* info)
{
    using namespace ssm_uvdc;
    ssm_ctx* c = u->c; UvdDev* D = u->dev; hipStream_t s = c->main.stream;
    const size_t px = (size_t)w * h;
    typedef std::chrono::steady_clock clk;
    auto ms_since = [](clk::time_point a) { return std::chrono::duration<double, std::milli>(clk::now() - a).count(); };
    const clk::time_point t_call = clk::now();
    uint8_t* d_moving = moving_dev ? moving_dev : (uint8_t*)D->d_moving; uint8_t* d_roi = roi_dev ? roi_dev : (uint8_t*)D->d_roi; uint8_t* d_ground = ground_dev ? ground_dev : (uint8_t*)D->d_ground;
    u->frames.resize(n);
    // phase 1: the V-disparity rows and the extremes
    for (int f = 0; f < n; f++) { D->h_maxmin[2 * f] = INT_MIN; D->h_maxmin[2 * f + 1] = INT_MAX; D->h_nmatch[f] = std::min(nmatch[f], cap); }
    HIPCHK(c, hipMemcpyAsync(D->d_maxmin, D->h_maxmin, (size_t)n * 8, hipMemcpyHostToDevice, s));
    prof_begin(c, s, "uvd_vdisp");
    HIPCHK(c, k_uvd_vdisp(disp_dev, n, w, h, D->d_vdis, D->d_maxmin, s));
    prof_end(c, s);
    HIPCHK(c, hipMemcpyAsync(D->h_vdis, D->d_vdis, (size_t)n * h * MAX_BINS, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(D->h_maxmin, D->d_maxmin, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    // host step 1, in frame order: the Kalman filters run through the frames
    clk::time_point t_host = clk::now();
    lk.unlock();
    for (int f = 0; f < n; f++) {
        UvdFrame& F = u->frames[f];
        F.w = w; F.h = h; F.max_disp = D->h_maxmin[2 * f];
        F.v_dis.assign(D->h_vdis + (size_t)f * h * MAX_BINS, D->h_vdis + (size_t)(f + 1) * h * MAX_BINS);
        uvd_host_step1(u->p, u->kf1, u->kf2, F, D->h_maxmin[2 * f + 1], nmatch[f] < 0);
        D->h_K[f] = F.k;
    }
    u->call_ms[0] = ms_since(t_host);
    lk.lock(); hipSetDevice(c->device);
    // phase 2: the masks, the U-disparity images, the probes
    for (int f = 0; f < n; f++) for (int i = 0; i < D->h_nmatch[f]; i++) {
        const ssm_pmatch& m = matches[(size_t)f * cap + i];
        D->h_coords[((size_t)f * cap + i) * 2] = (int)m.u1c; D->h_coords[((size_t)f * cap + i) * 2 + 1] = (int)m.v1c;
    }
    HIPCHK(c, hipMemcpyAsync(D->d_K, D->h_K, (size_t)n * sizeof(FrameK), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(D->d_nmatch, D->h_nmatch, (size_t)n * 4, hipMemcpyHostToDevice, s));
    if (cap) HIPCHK(c, hipMemcpyAsync(D->d_coords, D->h_coords, (size_t)n * cap * 8, hipMemcpyHostToDevice, s));
    prof_begin(c, s, "uvd_classify");
    HIPCHK(c, k_uvd_classify(left_dev, disp_dev, n, w, h, D->d_K, uvd_calib(u->p), uvd_roi(u->p), D->d_rate, d_ground, d_roi, D->d_uraw, D->d_uadj, s));
    HIPCHK(c, k_uvd_probe(d_roi, disp_dev, n, w, h, D->d_coords, D->d_nmatch, cap, D->d_probes, s));
    prof_end(c, s);
    const size_t ustride = (size_t)MAX_BINS * w;
    uint8_t* h_raw = D->h_u; uint8_t* h_adj = D->h_u + (size_t)D->cap_n * ustride;
    for (int f = 0; f < n; f++) {
        if (!u->frames[f].k.run) continue;
        const size_t bytes = (size_t)u->frames[f].k.u_rows * w;
        HIPCHK(c, hipMemcpyAsync(h_raw + f * ustride, D->d_uraw + f * ustride, bytes, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(h_adj + f * ustride, D->d_uadj + f * ustride, bytes, hipMemcpyDeviceToHost, s));
    }
    if (cap) HIPCHK(c, hipMemcpyAsync(D->h_probes, D->d_probes, (size_t)n * cap * 4, hipMemcpyDeviceToHost, s));
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
            const int nm = D->h_nmatch[f];
            for (int i = 0; i < nm; i++) { const int32_t v = D->h_probes[(size_t)f * cap + i]; pr[i] = (uint8_t)(v >> 16); pd[i] = (int16_t)(v & 0xFFFF); }
            uvd_host_step2(u->p, F, matches + (size_t)f * cap, flags + (size_t)f * cap, nm, pr.data(), pd.data(), u->record);
            if (F.k.run) memcpy(h_raw + f * ustride, F.uni.data(), bytes);           // (the raw image has been copied out: its staging carries the union mask up)
        }
        D->h_K[f] = F.k; D->h_counts[f] = 0;
    }
    u->call_ms[1] = ms_since(t_host);
    lk.lock(); hipSetDevice(c->device);
    // phase 3: the moving mask
    HIPCHK(c, hipMemcpyAsync(D->d_K, D->h_K, (size_t)n * sizeof(FrameK), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(D->d_counts, D->h_counts, (size_t)n * 4, hipMemcpyHostToDevice, s));
    for (int f = 0; f < n; f++)
        if (u->frames[f].k.run) HIPCHK(c, hipMemcpyAsync(D->d_uni + f * ustride, h_raw + f * ustride, (size_t)u->frames[f].k.u_rows * w, hipMemcpyHostToDevice, s));
    prof_begin(c, s, "uvd_segment");
    HIPCHK(c, k_uvd_segment(disp_dev, d_roi, D->d_uni, n, w, h, D->d_K, d_moving, D->d_counts, s));
    prof_end(c, s);
    HIPCHK(c, hipMemcpyAsync(D->h_counts, D->d_counts, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    for (int f = 0; f < n; f++) { u->frames[f].info.n_moving = D->h_counts[f]; info[f] = u->frames[f].info; }
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
    hipStream_t s = c->main.stream; UvdDev* D = u->dev;
    HIPCHK(c, hipMemcpy2DAsync(D->d_left, (size_t)w, left, (size_t)stride, (size_t)w, h, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpy2DAsync(D->d_disp, (size_t)w * 2, disp, (size_t)stride * 2, (size_t)w * 2, h, hipMemcpyHostToDevice, s));
    const int32_t nm = n_matches;
    { const int r = uvd_run_dev(lk, u, D->d_left, D->d_disp, 1, w, h, matches, &nm, inlier_flags, std::max(n_matches, 0), nullptr, nullptr, nullptr, info); if (r) return r; }
    const size_t px = (size_t)w * h;
    if (moving) HIPCHK(c, hipMemcpyAsync(moving, D->d_moving, px, hipMemcpyDeviceToHost, s));
    if (roi) HIPCHK(c, hipMemcpyAsync(roi, D->d_roi, px, hipMemcpyDeviceToHost, s));
    if (ground) HIPCHK(c, hipMemcpyAsync(ground, D->d_ground, px, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return SSM_OK;
}
