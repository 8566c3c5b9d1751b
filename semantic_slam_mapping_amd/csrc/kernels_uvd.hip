// kernels_uvd.hip -- the per-pixel stages of UVDisparity::Process for n device frames.  All arithmetic is include/ssm/uvd_core.h, which the host
// pipeline of ssm_uvd.hip calls too; the kernels add only the data movement: the V-disparity rows, the ROI / ground masks with the U-disparity columns, the
// match probes and the moving mask.  Counters are integers (LDS and global integer atomics, whose sums and extremes do not depend on order); there is no
// floating-point atomic.  Loads and stores are coalesced per wave; nothing beyond that has been tuned (profiles/r13_uvd.md).
#include "ssm_internal.h"
#include "../../include/ssm/uvd_core.h"
#include <climits>
using namespace ssm_uvdc;

#define UVD_T 256
// one block per (row, frame): the row's 256-bin histogram in LDS, written as the u8 row of the V-disparity image; the frame's largest and smallest raw disparity
__global__ __launch_bounds__(UVD_T) void uvd_vdisp_kernel(const int16_t* __restrict__ disp, int w, int h, uint8_t* __restrict__ v_dis, int32_t* __restrict__ maxmin)
{
    __shared__ int hist[MAX_BINS];
    const int row = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    hist[tid] = 0;
    __syncthreads();
    const int16_t* p = disp + ((size_t)f * h + row) * w;
    int mx = INT_MIN, mn = INT_MAX;
    for (int j = tid; j < w; j += UVD_T) {
        const short d = p[j];
        mx = max(mx, (int)d); mn = min(mn, (int)d);
        const int b = v_bin(d);
        if (b >= 0) atomicAdd(&hist[b], 1);
    }
    for (int o = 32; o > 0; o >>= 1) { mx = max(mx, __shfl_xor(mx, o)); mn = min(mn, __shfl_xor(mn, o)); }
    if ((tid & 63) == 0 && mx >= mn) { atomicMax(&maxmin[2 * f], mx); atomicMin(&maxmin[2 * f + 1], mn); }
    __syncthreads();
    v_dis[((size_t)f * h + row) * MAX_BINS + tid] = hist_u8(hist[tid], hist_scale(w));
}
hipError_t k_uvd_vdisp(const int16_t* disp, int n, int w, int h, uint8_t* v_dis, int32_t* maxmin, hipStream_t s)
{
    static_assert(UVD_T == MAX_BINS, "one thread per bin");
    if (n <= 0) return hipSuccess;
    uvd_vdisp_kernel<<<dim3(h, n), dim3(UVD_T), 0, s>>>(disp, w, h, v_dis, maxmin);
    return hipGetLastError();
}

// one wave per (64-column strip, frame): every lane walks its column top to bottom, writes the two masks and counts the column's U-disparity bins in LDS words
// that only it touches -- no atomics.  Then the u8 scaling and the rate table of adjustUdisIntense
#define UVD_CW 64
__global__ __launch_bounds__(UVD_CW) void uvd_classify_kernel(const uint8_t* __restrict__ left, const int16_t* __restrict__ disp, int w, int h, const FrameK* __restrict__ K,
                                                              Calib c, Roi r, const double* __restrict__ rate, uint8_t* __restrict__ ground, uint8_t* __restrict__ roi,
                                                              uint8_t* __restrict__ u_raw, uint8_t* __restrict__ u_adj)
{
    __shared__ uint16_t bins[MAX_BINS * UVD_CW];         // [bin][lane]: h < 65536
    const int lane = threadIdx.x, f = blockIdx.y, j = blockIdx.x * UVD_CW + lane;
    const FrameK k = K[f];
    if (j >= w) return;
    const size_t base = (size_t)f * h * w + j;
    if (!k.run) {
        for (int i = 0; i < h; i++) { ground[base + (size_t)i * w] = 0; roi[base + (size_t)i * w] = 0; }
        return;
    }
    for (int b = 0; b < k.u_rows; b++) bins[b * UVD_CW + lane] = 0;
    for (int i = 0; i < h; i++) {
        const size_t at = base + (size_t)i * w;
        const short d = disp[at]; const uint8_t in = left[at];
        const uint8_t g = ground_pixel(i, d, in, k.slope, k.v_c);
        const uint8_t ro = roi_pixel(i, j, d, in, k, c, r);
        ground[at] = g; roi[at] = ro;
        const int b = u_bin(d, ro, g);
        if (b >= 0 && b < k.u_rows) bins[b * UVD_CW + lane]++;
    }
    const float scale = hist_scale(h);
    for (int b = 0; b < k.u_rows; b++) {
        const uint8_t raw = hist_u8(bins[b * UVD_CW + lane], scale);
        const size_t at = ((size_t)f * MAX_BINS + b) * w + j;
        u_raw[at] = raw; u_adj[at] = u_adjust(raw, rate[b]);
    }
}
hipError_t k_uvd_classify(const uint8_t* left, const int16_t* disp, int n, int w, int h, const FrameK* K, const Calib& c, const Roi& r, const double* rate,
                          uint8_t* ground, uint8_t* roi, uint8_t* u_raw, uint8_t* u_adj, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    uvd_classify_kernel<<<dim3((w + UVD_CW - 1) / UVD_CW, n), dim3(UVD_CW), 0, s>>>(left, disp, w, h, K, c, r, rate, ground, roi, u_raw, u_adj);
    return hipGetLastError();
}

// what filterInOut reads at each match's (v1c, u1c): the ROI mask and the disparity.  A match outside the image reads roi 0
__global__ void uvd_probe_kernel(const uint8_t* __restrict__ roi, const int16_t* __restrict__ disp, int n, int w, int h, const int32_t* __restrict__ coords,
                                 const int32_t* __restrict__ nmatch, int cap, int32_t* __restrict__ probes)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)n * cap) return;
    const int f = (int)(t / cap), i = (int)(t % cap);
    int32_t out = 0;
    if (i < nmatch[f]) {
        const int u = coords[2 * t], v = coords[2 * t + 1];
        if (u >= 0 && u < w && v >= 0 && v < h) {
            const size_t at = ((size_t)f * h + v) * w + u;
            out = ((int32_t)roi[at] << 16) | (int32_t)(uint16_t)disp[at];
        }
    }
    probes[t] = out;
}
hipError_t k_uvd_probe(const uint8_t* roi, const int16_t* disp, int n, int w, int h, const int32_t* coords, const int32_t* nmatch, int cap, int32_t* probes, hipStream_t s)
{
    const size_t total = (size_t)n * cap;
    if (!total) return hipSuccess;
    uvd_probe_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s>>>(roi, disp, n, w, h, coords, nmatch, cap, probes);
    return hipGetLastError();
}

// segmentation per pixel against the union of the surviving masks, and the frame's count of moving pixels
__global__ __launch_bounds__(UVD_T) void uvd_segment_kernel(const int16_t* __restrict__ disp, const uint8_t* __restrict__ roi, const uint8_t* __restrict__ uni, int w, int h,
                                                            const FrameK* __restrict__ K, uint8_t* __restrict__ moving, int32_t* __restrict__ counts)
{
    const int f = blockIdx.y;
    const FrameK k = K[f];
    const size_t px = (size_t)w * h, base = (size_t)f * px;
    const uint8_t* um = uni + (size_t)f * MAX_BINS * w;
    int mine = 0;
    for (size_t t = (size_t)blockIdx.x * UVD_T + threadIdx.x; t < px; t += (size_t)gridDim.x * UVD_T) {
        uint8_t out = 0;
        if (k.run) { const int j = (int)(t % w); if (moving_test(disp[base + t], roi[base + t], j, um, k.u_rows, w)) out = 255; }
        moving[base + t] = out;
        mine += out != 0;
    }
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&counts[f], mine);
}
hipError_t k_uvd_segment(const int16_t* disp, const uint8_t* roi, const uint8_t* uni, int n, int w, int h, const FrameK* K, uint8_t* moving, int32_t* counts, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    const size_t px = (size_t)w * h;
    const unsigned blocks = (unsigned)((px + UVD_T * 4 - 1) / (UVD_T * 4));
    uvd_segment_kernel<<<dim3(blocks, n), dim3(UVD_T), 0, s>>>(disp, roi, uni, w, h, K, moving, counts);
    return hipGetLastError();
}
