// kernels_render.hip -- map rendering of m clouds in device memory into one pinhole view: the clear of the z-buffer, the splat, the resolve into
// the four images, and the comparison with a frame.  The arithmetic is include/ssm/render_core.h, which the host functions of ssm_render_host.cpp call too.
//
// Splat: one thread per point over the concatenation of the m clouds, found through the cloud-segment table (cloud_table.h).  A point offers its key (quantised
// depth << 32 | index) to every pixel of its clipped footprint with a 64-bit integer atomicMin; the pixel keeps the minimum, so the result does not depend on the
// order the points arrive in.  Resolve: one thread per pixel finds the winner's cloud by bisection of the table and gathers its colour and label.
// Compare: one thread per pixel, the counts summed per wave by ballot, per block through LDS, then one 64-bit integer atomic per count and block.
// Integer atomics only; no grid barrier, no block waits for another.
#include "ssm_internal.h"
#include "../../include/ssm/render_core.h"
using namespace ssm_renderc;

#define RENDER_T 256
#define RENDER_W (RENDER_T / 64)
int k_render_block() { return RENDER_T; }
// A probe build (-DRENDER_PROBE: scripts/render_probe.hip, never the library) counts what the splat kernel does: [0] footprint pixels offered a key, [1] atomics issued
#ifdef RENDER_PROBE
__device__ unsigned long long render_probe_counts[2];
#define RENDER_COUNT(i) atomicAdd(&render_probe_counts[i], 1ull)
#else
#define RENDER_COUNT(i)
#endif

__global__ void __launch_bounds__(RENDER_T)
render_clear_kernel(unsigned long long* __restrict__ keys, int64_t np, int32_t* __restrict__ info, int32_t n_in)
{
    const int64_t i = (int64_t)blockIdx.x * RENDER_T + threadIdx.x;
    if (i < np) keys[i] = KEY_EMPTY;
    if (i == 0) { info[0] = n_in; info[1] = 0; info[2] = 0; info[3] = 0; }
}
__global__ void __launch_bounds__(RENDER_T)
render_splat_kernel(const Setup S, const CloudSeg* __restrict__ seg, const int32_t* __restrict__ blk, int64_t total, unsigned long long* __restrict__ keys,
                    int32_t* __restrict__ info)
{
    const int64_t g = (int64_t)blockIdx.x * RENDER_T + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int k0 = blk[blockIdx.x];
    const bool uniform = cloud_block_uniform<int64_t>(seg, k0, (int64_t)blockIdx.x * RENDER_T, RENDER_T, total);
    bool vis = false;
    if (g < total) {
        const int k = cloud_of<int64_t>(seg, k0, uniform, g);
        const ssm_point* p = seg[k].pts + (g - seg[k].off);
        Splat sp;
        vis = splat_of(p->x, p->y, p->z, seg[k].M, S, &sp);
        if (vis) {
            const unsigned long long key = key_of(sp.zq, (uint32_t)g);
            for (int y = sp.y0; y <= sp.y1; y++) {
                unsigned long long* row = keys + (size_t)y * (size_t)S.w;
                for (int x = sp.x0; x <= sp.x1; x++) {
                    // A plain load first: a point whose key is not smaller than what the pixel holds skips the atomic.  That is safe because a pixel's key only
                    // ever decreases during the kernel: a stale (older, hence larger or equal) value can only cause a superfluous atomic, never a missing one.
                    RENDER_COUNT(0);
                    if (key < row[x]) { RENDER_COUNT(1); atomicMin(row + x, key); }
                }
            }
        }
    }
    const int c = __popcll(__ballot(vis));
    if (lane == 0 && c) atomicAdd(info + 1, c);
}
__global__ void __launch_bounds__(RENDER_T)
render_resolve_kernel(const unsigned long long* __restrict__ keys, int64_t np, const CloudSeg* __restrict__ seg, int m, uint16_t* __restrict__ depth,
                      uint8_t* __restrict__ bgr, uint8_t* __restrict__ label, int32_t* __restrict__ index, int32_t* __restrict__ info)
{
    const int64_t i = (int64_t)blockIdx.x * RENDER_T + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool covered = false;
    if (i < np) {
        const unsigned long long key = keys[i];
        covered = key != KEY_EMPTY;
        uint16_t d = 0; uint32_t c = 0; uint8_t l = 255; int32_t ix = -1;
        if (covered) {
            const int64_t idx = (int64_t)(uint32_t)key;
            int lo = 0, hi = m - 1;                                   // the last cloud whose first point is not behind idx and that is not empty before it
            while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (seg[mid].off <= idx) lo = mid; else hi = mid - 1; }
            // (clouds of size 0 share their off with the next one: bisection lands on the LAST of equal offs, which is the one that holds the point)
            const uint4 w1 = reinterpret_cast<const uint4*>(seg[lo].pts + (idx - seg[lo].off))[1];          // b g r a | label | pad pad
            d = (uint16_t)(key >> 32); c = w1.x & 0xFFFFFFu; l = (uint8_t)(w1.y & 255u); ix = (int32_t)(uint32_t)key;
        }
        depth[i] = d; label[i] = l; index[i] = ix;
        bgr[i * 3] = (uint8_t)c; bgr[i * 3 + 1] = (uint8_t)(c >> 8); bgr[i * 3 + 2] = (uint8_t)(c >> 16);
    }
    const int n = __popcll(__ballot(covered));
    if (lane == 0 && n) atomicAdd(info + 2, n);
}
__global__ void __launch_bounds__(RENDER_T)
render_compare_kernel(const uint16_t* __restrict__ rdepth, const uint8_t* __restrict__ rlabel, const uint16_t* __restrict__ depth, const uint8_t* __restrict__ sem,
                      int64_t np, int64_t tol_abs, int64_t ppm, uint8_t* __restrict__ cls_out, unsigned long long* __restrict__ counts)
{
    __shared__ int cnt_s[RENDER_W][8];
    const int64_t i = (int64_t)blockIdx.x * RENDER_T + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int cls = -1, lab = LABEL_NONE;
    if (i < np) {
        const uint8_t lf = label_of_bgr24((uint32_t)sem[i * 3] | ((uint32_t)sem[i * 3 + 1] << 8) | ((uint32_t)sem[i * 3 + 2] << 16));
        cls = class_of(rdepth[i], depth[i], rlabel[i], lf, tol_abs, ppm, &lab);
        cls_out[i] = (uint8_t)cls;
    }
    // the eight counts of the wave, in the order of ssm_render_compare_info
    const int c0 = __popcll(__ballot(cls == UNRENDERED)), c1 = __popcll(__ballot(cls == NO_DEPTH)), c2 = __popcll(__ballot(cls == IN_FRONT)),
              c3 = __popcll(__ballot(cls == BEHIND)), c4 = __popcll(__ballot(cls == AGREE)), c5 = __popcll(__ballot(lab == LABEL_AGREE)),
              c6 = __popcll(__ballot(lab == LABEL_DISAGREE)), c7 = __popcll(__ballot(lab == LABEL_UNKNOWN));
    if (lane == 0) { int* r = cnt_s[wave]; r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3; r[4] = c4; r[5] = c5; r[6] = c6; r[7] = c7; }
    __syncthreads();
    if (threadIdx.x < 8) {
        int t = 0;
        for (int w = 0; w < RENDER_W; w++) t += cnt_s[w][threadIdx.x];
        if (t) atomicAdd(counts + threadIdx.x, (unsigned long long)t);
    }
}
__global__ void render_counts_clear_kernel(unsigned long long* __restrict__ counts, int64_t np)
{
    if (threadIdx.x < 8) counts[threadIdx.x] = 0;
    if (threadIdx.x == 8) counts[8] = (unsigned long long)np;
}

// ------------------------------------------------------------------ launchers
static inline unsigned render_blocks(int64_t n) { return (unsigned)((n + RENDER_T - 1) / RENDER_T); }
hipError_t k_render(const Setup& S, const CloudSeg* seg, const int32_t* blk, int m, int64_t total, const RenderImgs& T, int32_t* info, hipStream_t s)
{
    const int64_t np = (int64_t)S.w * S.h;
    render_clear_kernel<<<render_blocks(np), RENDER_T, 0, s>>>(T.keys, np, info, (int32_t)(uint32_t)total);
    if (total > 0) render_splat_kernel<<<render_blocks(total), RENDER_T, 0, s>>>(S, seg, blk, total, T.keys, info);
    render_resolve_kernel<<<render_blocks(np), RENDER_T, 0, s>>>(T.keys, np, seg, m, T.depth, T.bgr, T.label, T.index, info);
    return hipGetLastError();
}
hipError_t k_render_compare(const uint16_t* rdepth, const uint8_t* rlabel, const uint16_t* depth, const uint8_t* sem, int64_t np, int64_t tol_abs, int64_t ppm,
                            uint8_t* cls, unsigned long long* counts, hipStream_t s)
{
    render_counts_clear_kernel<<<1, 64, 0, s>>>(counts, np);
    render_compare_kernel<<<render_blocks(np), RENDER_T, 0, s>>>(rdepth, rlabel, depth, sem, np, tol_abs, ppm, cls, counts);
    return hipGetLastError();
}
