// ssm_motion_fuse.hip -- the device path of the semantic-motion fusion (reference src/mapper.cpp:217-271) behind the C ABI.  DESIGN.md s.14 is the contract.  A call
// is one launch sequence (kernels_motion_fuse.hip) and one wait; the workspaces belong to the context (MfWork) and grow with the largest call.  The host
// function, the defaults and the argument check are ssm_motion_fuse_host.cpp.
#include "ssm_ctx.h"
#include "ssm_host.h"

static int mf_reserve(ssm_ctx* c, int n, int w, int h)
{
    MfWork& M = c->mf;
    const size_t px = (size_t)w * h;
    if (n <= M.cap_n && px <= M.cap_px) return SSM_OK;
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    const size_t nn = (size_t)std::max(n, M.cap_n), pp = std::max(px, M.cap_px);
    M.cap_n = 0; M.cap_px = 0; M.n = 0;
    DALLOC(c, M.always, nn * pp); DALLOC(c, M.cand, nn * pp); DALLOC(c, M.filled, nn * pp);
    DALLOC(c, M.labels, nn * (pp + 1)); DALLOC(c, M.area, nn * pp); DALLOC(c, M.overlap, nn * pp);
    DALLOC(c, M.info, nn * 4); DALLOC(c, M.h_info, nn * 4);
    M.in_sem.reset(); M.in_motion.reset(); M.out_mask.reset();
    M.cap_n = (int)nn; M.cap_px = pp;
    return SSM_OK;
}
int mf_enqueue(ssm_ctx* c, const uint8_t* sem_dev, const uint8_t* motion_dev, const uint8_t* motion_host, int n, int w, int h, const ssm_motion_fuse_params* params,
               uint8_t* mask_dev)
{
    { const int r = mf_check(c, n, w, h, (size_t)w * 3); if (r) return r; }
    if (n == 0) return SSM_OK;
    { const int r = mf_reserve(c, n, w, h); if (r) return r; }
    MfWork& M = c->mf; hipStream_t s = c->main.stream;
    ssm_motion_fuse_params P; ssm_motion_fuse_params_default(&P); if (params) P = *params;
    if (motion_host) {
        if (n != 1) FAIL(c, SSM_E_INVAL, "motion_fuse: a host motion mask goes with one frame");
        if (!M.in_motion) DALLOC(c, M.in_motion, M.cap_px);
        HIPCHK(c, hipMemcpyAsync(M.in_motion, motion_host, (size_t)w * h, hipMemcpyHostToDevice, s));
        motion_dev = M.in_motion;
    }
    prof_begin(c, s, "motion_fuse");
    HIPCHK(c, k_motion_fuse(sem_dev, motion_dev, n, w, h, P.area_thres, P.overlay_thres, M.always, M.cand, M.filled, M.labels, M.area, M.overlap, mask_dev, M.info, s));
    prof_end(c, s);
    M.n = n; M.w = w; M.h = h;
    return SSM_OK;
}
static int mf_fetch_info(ssm_ctx* c, int n, ssm_motion_fuse_info* info)          // with the call's one wait
{
    MfWork& M = c->mf; hipStream_t s = c->main.stream;
    if (info && n > 0) HIPCHK(c, hipMemcpyAsync(M.h_info, M.info, (size_t)n * 16, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    static_assert(sizeof(ssm_motion_fuse_info) == 16, "four counters");
    if (info && n > 0) memcpy(info, M.h_info, (size_t)n * 16);
    return SSM_OK;
}

extern "C" int ssm_motion_fuse_dev(ssm_ctx* c, const uint8_t* sem_dev, const uint8_t* motion_dev, int n, int w, int h, const ssm_motion_fuse_params* params,
                                   uint8_t* mask_dev, ssm_motion_fuse_info* info)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (n > 0 && (!sem_dev || !mask_dev)) FAIL(c, SSM_E_INVAL, "null argument");
    { const int r = mf_enqueue(c, sem_dev, motion_dev, nullptr, n, w, h, params, mask_dev); if (r) return r; }
    return mf_fetch_info(c, n, info);
}
extern "C" int ssm_motion_fuse(ssm_ctx* c, const uint8_t* sem, const uint8_t* motion, int w, int h, int stride, const ssm_motion_fuse_params* params, uint8_t* mask,
                               ssm_motion_fuse_info* info)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (!sem || !mask) FAIL(c, SSM_E_INVAL, "null argument");
    { const int r = mf_check(c, 1, w, h, (size_t)(stride < 0 ? 0 : stride)); if (r) return r; }
    { const int r = mf_reserve(c, 1, w, h); if (r) return r; }
    MfWork& M = c->mf; hipStream_t s = c->main.stream;
    if (!M.in_sem) { DALLOC(c, M.in_sem, M.cap_px * 3); DALLOC(c, M.out_mask, M.cap_px); }
    HIPCHK(c, hipMemcpy2DAsync(M.in_sem, (size_t)w * 3, sem, (size_t)stride, (size_t)w * 3, h, hipMemcpyHostToDevice, s));
    { const int r = mf_enqueue(c, M.in_sem, nullptr, motion, 1, w, h, params, M.out_mask); if (r) return r; }
    HIPCHK(c, hipMemcpyAsync(mask, M.out_mask, (size_t)w * h, hipMemcpyDeviceToHost, s));
    return mf_fetch_info(c, 1, info);
}
extern "C" int ssm_debug_motion_fuse(ssm_ctx* c, int frame, int32_t* labels, int32_t* area, int32_t* overlap, uint8_t* cand)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    MfWork& M = c->mf; hipStream_t s = c->main.stream;
    if (frame < 0 || frame >= M.n) FAIL(c, SSM_E_INVAL, "motion_fuse: no such frame in the last call");
    const size_t px = (size_t)M.w * M.h;
    if (labels) HIPCHK(c, hipMemcpyAsync(labels, M.labels + (size_t)frame * k_mf_label_stride(M.w, M.h), px * 4, hipMemcpyDeviceToHost, s));
    if (area) HIPCHK(c, hipMemcpyAsync(area, M.area + (size_t)frame * px, px * 4, hipMemcpyDeviceToHost, s));
    if (overlap) HIPCHK(c, hipMemcpyAsync(overlap, M.overlap + (size_t)frame * px, px * 4, hipMemcpyDeviceToHost, s));
    if (cand) HIPCHK(c, hipMemcpyAsync(cand, M.cand + (size_t)frame * px, px, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return SSM_OK;
}
