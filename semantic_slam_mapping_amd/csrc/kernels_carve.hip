// kernels_carve.hip -- free-space carving of m clouds in device memory under one view: the verdicts, the run counters and the stable compaction
// of points AND counters, per cloud.  The arithmetic is include/ssm/carve_core.h, which the host function of ssm_carve_host.cpp calls too.
//
// One thread per point over the concatenation of the m clouds, found through the cloud-segment table (cloud_table.h), here with 32-bit point numbers: a call
// has 2^30 points at most.  The view's depth image (0.6 - 0.9 MB) is read through plain uint16 loads and stays in L2.  Verdict, counter and keep flag are
// made in registers; the kept are counted per block, one scan over the blocks of the whole concatenation gives every block its offset, and the kept points and
// counters go to a scratch copy in that order -- a block's compacted output would land where EARLIER blocks still read their input, so nothing is compacted in
// place -- from where the last kernel puts cloud k's share, which starts at base[k], back at the front of cloud k.
// Integer atomics only, and only for the info counters; no grid barrier, no block waits for another.
#include "ssm_internal.h"
#include "../../include/ssm/carve_core.h"
#include <cstring>
#include <rocprim/rocprim.hpp>
using namespace ssm_carvec;

#define CARVE_T 256
#define CARVE_W (CARVE_T / 64)
int k_carve_block() { return CARVE_T; }

__device__ inline bool carve_block_uniform(const CloudSeg* __restrict__ seg, int k0, int total) { return cloud_block_uniform<int>(seg, k0, (int)blockIdx.x * CARVE_T, CARVE_T, total); }

__global__ void carve_init_kernel(int32_t* __restrict__ info, int m, uint32_t* __restrict__ block_cnt, int nb)
{
    const int i = blockIdx.x * CARVE_T + threadIdx.x;
    if (i < m * 8) info[i] = 0;
    if (i == 0) block_cnt[nb] = 0;                                // the scan's last entry becomes the total
}
__global__ void __launch_bounds__(CARVE_T)
carve_verdict_kernel(const uint16_t* __restrict__ depth, const Setup S, int min_votes, const CloudSeg* __restrict__ seg, const int32_t* __restrict__ blk, int total,
                     uint8_t* __restrict__ verdict, uint8_t* __restrict__ run_new, uint8_t* __restrict__ keep, uint32_t* __restrict__ block_cnt, int32_t* __restrict__ info)
{
    __shared__ int cnt_s[CARVE_W];
    const int g = blockIdx.x * CARVE_T + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k0 = blk[blockIdx.x];
    const bool uniform = carve_block_uniform(seg, k0, total);
    const bool live = g < total;
    int k = k0, v = UNKNOWN; bool kp = false;
    if (live) {
        k = cloud_of<int>(seg, k0, uniform, g);
        const int local = g - (int)seg[k].off;
        const ssm_point* p = seg[k].pts + local;
        v = verdict_of(p->x, p->y, p->z, seg[k].M, depth, S);
        const uint8_t rn = run_after(seg[k].run[local], v);
        kp = !leaves(rn, min_votes);
        verdict[g] = (uint8_t)v; run_new[g] = rn; keep[g] = kp ? 1 : 0;
    }
    const unsigned long long bk = __ballot(kp);
    if (uniform) {          // one cloud: the wave's five counts through lane 0
        const int c0 = __popcll(__ballot(live && v == UNKNOWN)), c1 = __popcll(__ballot(live && v == OCCLUDED)), c2 = __popcll(__ballot(live && v == SUPPORTED)),
                  c3 = __popcll(__ballot(live && v == SEEN_THROUGH));
        if (lane == 0) {
            int32_t* I = info + k0 * 8;
            if (bk) atomicAdd(I + 1, __popcll(bk));
            if (c0) atomicAdd(I + 2, c0);
            if (c1) atomicAdd(I + 3, c1);
            if (c2) atomicAdd(I + 4, c2);
            if (c3) atomicAdd(I + 5, c3);
        }
    } else if (live) {      // a cloud boundary inside the block: every point counts for its own cloud
        int32_t* I = info + k * 8;
        if (kp) atomicAdd(I + 1, 1);
        atomicAdd(I + 2 + v, 1);
    }
    if (lane == 0) cnt_s[wave] = __popcll(bk);
    __syncthreads();
    if (threadIdx.x == 0) { int t = 0; for (int w = 0; w < CARVE_W; w++) t += cnt_s[w]; block_cnt[blockIdx.x] = (uint32_t)t; }
}
// per cloud: where its kept points start in the scratch copy, and the info fields that follow from the counts
__global__ void carve_base_kernel(const CloudSeg* __restrict__ seg, int m, int32_t* __restrict__ info, uint32_t* __restrict__ base)
{
    if (blockIdx.x || threadIdx.x) return;
    uint32_t at = 0;
    for (int k = 0; k < m; k++) {
        base[k] = at; at += (uint32_t)info[k * 8 + 1];
        info[k * 8 + 0] = seg[k].n; info[k * 8 + 6] = seg[k].n - info[k * 8 + 1];
    }
    base[m] = at;
}
// the stable move into the scratch copy: a kept point goes to its block's offset plus its rank inside the block, all 32 bytes, and its counter beside it
__global__ void __launch_bounds__(CARVE_T)
carve_compact_kernel(const CloudSeg* __restrict__ seg, const int32_t* __restrict__ blk, int total, const uint8_t* __restrict__ keep, const uint8_t* __restrict__ run_new,
                     const uint32_t* __restrict__ block_off, ssm_point* __restrict__ tmp_pts, uint8_t* __restrict__ tmp_run)
{
    __shared__ int cnt_s[CARVE_W];
    const int g = blockIdx.x * CARVE_T + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool kp = g < total && keep[g];
    const unsigned long long b = __ballot(kp);
    if (lane == 0) cnt_s[wave] = __popcll(b);
    __syncthreads();
    if (!kp) return;
    const int k0 = blk[blockIdx.x];
    const int k = cloud_of<int>(seg, k0, carve_block_uniform(seg, k0, total), g);
    uint32_t at = block_off[blockIdx.x] + (uint32_t)__popcll(b & (((unsigned long long)1 << lane) - 1));
    for (int w = 0; w < wave; w++) at += (uint32_t)cnt_s[w];
    const uint4* src = reinterpret_cast<const uint4*>(seg[k].pts + (g - (int)seg[k].off));
    uint4* dst = reinterpret_cast<uint4*>(tmp_pts + at);
    dst[0] = src[0]; dst[1] = src[1];
    tmp_run[at] = run_new[g];
}
// back into the clouds: entry `local` of cloud k is entry base[k] + local of the scratch copy, for local below the cloud's kept count
__global__ void __launch_bounds__(CARVE_T)
carve_store_kernel(const CloudSeg* __restrict__ seg, const int32_t* __restrict__ blk, int total, const uint32_t* __restrict__ base,
                   const ssm_point* __restrict__ tmp_pts, const uint8_t* __restrict__ tmp_run)
{
    const int g = blockIdx.x * CARVE_T + threadIdx.x;
    if (g >= total) return;
    const int k0 = blk[blockIdx.x];
    const int k = cloud_of<int>(seg, k0, carve_block_uniform(seg, k0, total), g);
    const uint32_t local = (uint32_t)(g - (int)seg[k].off), first = base[k];
    if (local >= base[k + 1] - first) return;
    const uint4* src = reinterpret_cast<const uint4*>(tmp_pts + first + local);
    uint4* dst = reinterpret_cast<uint4*>(seg[k].pts + local);
    dst[0] = src[0]; dst[1] = src[1];
    seg[k].run[local] = tmp_run[first + local];
}

// ------------------------------------------------------------------ launchers
static inline int carve_blocks(int n) { return (n + CARVE_T - 1) / CARVE_T; }
size_t k_carve_tmp_bytes(int total)
{
    size_t a = 0;
    (void)rocprim::exclusive_scan(nullptr, a, (const uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t)0, (size_t)carve_blocks(total) + 1, rocprim::plus<uint32_t>(), (hipStream_t)0);
    return a + 256;
}
hipError_t k_carve(const uint16_t* depth, const Setup& S, int min_votes, int m, int total, const CarveBufs& B, hipStream_t s)
{
    const int nb = carve_blocks(total);
    carve_init_kernel<<<carve_blocks(m * 8), CARVE_T, 0, s>>>(B.info, m, B.block_cnt, nb);
    if (total > 0) {
        carve_verdict_kernel<<<nb, CARVE_T, 0, s>>>(depth, S, min_votes, B.seg, B.blk, total, B.verdict, B.run_new, B.keep, B.block_cnt, B.info);
        size_t bytes = B.tmp_bytes;
        const hipError_t e = rocprim::exclusive_scan(B.tmp, bytes, B.block_cnt, B.block_off, (uint32_t)0, (size_t)nb + 1, rocprim::plus<uint32_t>(), s);
        if (e != hipSuccess) return e;
    }
    carve_base_kernel<<<1, 64, 0, s>>>(B.seg, m, B.info, B.base);
    if (total > 0) {
        carve_compact_kernel<<<nb, CARVE_T, 0, s>>>(B.seg, B.blk, total, B.keep, B.run_new, B.block_off, B.tmp_pts, B.tmp_run);
        carve_store_kernel<<<nb, CARVE_T, 0, s>>>(B.seg, B.blk, total, B.base, B.tmp_pts, B.tmp_run);
    }
    return hipGetLastError();
}
