// kernels_align.hip -- dense alignment of m clouds in device memory against one view: the view's normal map and one iteration's sums.  The
// arithmetic is include/ssm/align_core.h, which the host function of ssm_align_host.cpp calls too.
//
// Normals: one thread per pixel, a block per 256 pixels of a row (the per-pixel kernels' row tiles), the four neighbours as plain loads.
// Accumulate: one thread per point over the concatenation of the m (strided) clouds, found through the cloud-segment table (cloud_table.h) with chunks of 256
// points as its blocks.  The grid is persistent: at most ALIGN_MAX_BLOCKS blocks, each walking chunks blockIdx.x, + gridDim.x, ...  A lane keeps its 30 sums as 64-bit
// integers in registers over the whole walk; then the wave adds them by xor butterfly, the block through LDS, and 30 threads issue one 64-bit integer atomic
// each.  The terms are integers (align_core.h to_units), so every order of addition gives the same bits: no floating-point atomic, no grid barrier, no block
// waits for another.  Depth and normals are gathered with plain loads; E comes as a kernel argument.
#include "ssm_internal.h"
#include "../../include/ssm/align_core.h"
using namespace ssm_alignc;

#define ALIGN_T 256
#define ALIGN_W (ALIGN_T / 64)
#define ALIGN_MAX_BLOCKS 1024
int k_align_block() { return ALIGN_T; }
extern "C" int64_t ssm_debug_align_pass_points(void) { return (int64_t)ALIGN_T * ALIGN_MAX_BLOCKS; }

struct AlignE { double e[12]; };

__global__ void __launch_bounds__(ALIGN_T)
align_normals_kernel(const uint16_t* __restrict__ depth, const Setup S, Normal* __restrict__ normals)
{
    const int x = blockIdx.x * ALIGN_T + threadIdx.x, y = blockIdx.y;
    if (x >= S.w) return;
    Normal n;
    normal_of(depth, x, y, S, &n);
    normals[(size_t)y * (size_t)S.w + (size_t)x] = n;
}

__global__ void __launch_bounds__(ALIGN_T)
align_accumulate_kernel(const Setup S, const AlignE E, const CloudSeg* __restrict__ seg, const int32_t* __restrict__ blk, int64_t total, int64_t chunks,
                        const uint16_t* __restrict__ depth, const Normal* __restrict__ normals, unsigned long long* __restrict__ sums)
{
    __shared__ int64_t part[ALIGN_W][NSUM];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t acc[NSUM];
#pragma unroll
    for (int q = 0; q < NSUM; q++) acc[q] = 0;
    for (int64_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        const int64_t g = ch * ALIGN_T + threadIdx.x;
        const int k0 = blk[ch];
        const int64_t last = min(total, (ch + 1) * ALIGN_T) - 1;
        const bool uniform = last < seg[k0].off + seg[k0].n;
        if (g < total) {
            const int k = cloud_of<int64_t>(seg, k0, uniform, g);
            const ssm_point* p = seg[k].pts + (g - seg[k].off) * seg[k].stride;
            point_terms(p->x, p->y, p->z, seg[k].M, E.e, depth, normals, S, acc);
        }
    }
#pragma unroll
    for (int q = 0; q < NSUM; q++) {
        long long v = acc[q];
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) v += __shfl_xor(v, s, 64);
        if (lane == 0) part[wave][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < NSUM) {
        int64_t t = 0;
#pragma unroll
        for (int w = 0; w < ALIGN_W; w++) t += part[w][threadIdx.x];
        if (t) atomicAdd(sums + threadIdx.x, (unsigned long long)t);
    }
}

// ------------------------------------------------------------------ launchers
hipError_t k_align_normals(const uint16_t* depth, const Setup& S, void* normals, hipStream_t s)
{
    const dim3 grid((unsigned)((S.w + ALIGN_T - 1) / ALIGN_T), (unsigned)S.h);
    align_normals_kernel<<<grid, ALIGN_T, 0, s>>>(depth, S, reinterpret_cast<Normal*>(normals));
    return hipGetLastError();
}
// sums: NSUM 64-bit integers that the caller has zeroed
hipError_t k_align_accumulate(const Setup& S, const double* E, const CloudSeg* seg, const int32_t* blk, int64_t total, const uint16_t* depth, const void* normals,
                              unsigned long long* sums, hipStream_t s)
{
    if (total <= 0) return hipSuccess;
    AlignE e; for (int k = 0; k < 12; k++) e.e[k] = E[k];
    const int64_t chunks = (total + ALIGN_T - 1) / ALIGN_T;
    const unsigned blocks = (unsigned)(chunks < ALIGN_MAX_BLOCKS ? chunks : ALIGN_MAX_BLOCKS);
    align_accumulate_kernel<<<blocks, ALIGN_T, 0, s>>>(S, e, seg, blk, total, chunks, depth, reinterpret_cast<const Normal*>(normals), sums);
    return hipGetLastError();
}
