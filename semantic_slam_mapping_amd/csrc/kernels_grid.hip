// kernels_grid.hip -- the ground grid of m clouds in device memory: the clear of the cells, pass A (n, hmin, hmax per cell), the ground kernel
// (base per cell), pass B (LOW / HIGH counts, the sum of the LOW heights, the two label histograms) and the resolve into the output arrays.  The arithmetic is
// include/ssm/grid_core.h, which the host function of ssm_grid_host.cpp calls too.
//
// Passes A and B: one thread per point over the concatenation of the m clouds, found through the cloud-segment table (cloud_table.h); M is wave-uniform in a block
// that lies inside one cloud.  A cell is one 128-byte record (ssm_grid_cell): everything a point touches of its cell lies in one cache line.  Integer atomics only
// (32-bit add / min / max and one 64-bit add), so every result is independent of the order the points arrive in; no grid barrier, no block waits for another.
// Pass A loads hmin and hmax plainly first and skips the atomic where the point cannot change them: both only ever move one way during the kernel, so a stale
// value can only cause a superfluous atomic, never a missing one.  Ground and resolve: one thread per cell; the class counts go per wave by ballot, per block
// through LDS, then one 64-bit integer atomic per count and block.
#include "ssm_internal.h"
#include "../../include/ssm/grid_core.h"
using namespace ssm_gridc;

#define GRID_T 256
#define GRID_W (GRID_T / 64)
int k_grid_block() { return GRID_T; }
// A probe build (-DGRID_PROBE: scripts/grid_probe.hip, never the library) counts the atomics the two passes issue: [0] pass A, [1] pass B
#ifdef GRID_PROBE
__device__ unsigned long long grid_probe_counts[2];
#define GRID_COUNT(i) atomicAdd(&grid_probe_counts[i], 1ull)
#else
#define GRID_COUNT(i)
#endif
static_assert(sizeof(ssm_grid_cell) == 128, "a cell is 128 bytes: eight 16-byte words, the first holds n, hmin, hmax, base");

// info: the ten 64-bit counts of ssm_grid_info
__global__ void __launch_bounds__(GRID_T)
grid_clear_kernel(uint4* __restrict__ words, int64_t nwords, unsigned long long* __restrict__ info, int64_t n_in)
{
    const int64_t i = (int64_t)blockIdx.x * GRID_T + threadIdx.x;
    if (i < nwords) words[i] = (i & 7) == 0 ? make_uint4(0u, (uint32_t)HMIN_EMPTY, (uint32_t)HMAX_EMPTY, (uint32_t)BASE_EMPTY) : make_uint4(0u, 0u, 0u, 0u);
    if (i < 10) info[i] = i == 0 ? (unsigned long long)n_in : 0ull;          // (info[1] counts the rejected points until the call ends)
}
// the point g of the call -> what becomes of it (-1: there is no such point), its cell and height, its label
__device__ inline int grid_point(const Setup& S, const CloudSeg* __restrict__ seg, const int32_t* __restrict__ blk, int64_t total, Hit* h, uint32_t* label)
{
    const int64_t g = (int64_t)blockIdx.x * GRID_T + threadIdx.x;
    const int k0 = blk[blockIdx.x];
    const bool uniform = cloud_block_uniform<int64_t>(seg, k0, (int64_t)blockIdx.x * GRID_T, GRID_T, total);
    if (g >= total) return -1;
    const int k = cloud_of<int64_t>(seg, k0, uniform, g);
    const ssm_point* p = seg[k].pts + (g - seg[k].off);
    *label = p->label;
    return point_of(p->x, p->y, p->z, seg[k].M, S, h);
}
// The points that are NOT used, counted per block: rejected -> info[1] (the launcher's caller turns it into n_finite), out of band -> info[2], outside -> info[3].
// Per wave by ballot, per block through LDS, one atomic per count and block, and none for a count of 0 -- in a cloud whose points are mostly used almost no
// block issues one.  (One atomic per wave and count onto these few words was what bounded pass A: 0.9 ms at 2.3 M points.)  The used points are summed from the
// cells by the resolve kernel.  Every thread of the block calls this.
__device__ inline void grid_count_points(int st, unsigned long long* __restrict__ info)
{
    __shared__ int cnt_s[GRID_W][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = __popcll(__ballot(st == P_REJECTED)), c1 = __popcll(__ballot(st == P_OUT_OF_BAND)), c2 = __popcll(__ballot(st == P_OUTSIDE));
    if (lane == 0) { int* r = cnt_s[wave]; r[0] = c0; r[1] = c1; r[2] = c2; }
    __syncthreads();
    if (threadIdx.x < 3) {
        int t = 0;
        for (int w = 0; w < GRID_W; w++) t += cnt_s[w][threadIdx.x];
        if (t) atomicAdd(info + 1 + threadIdx.x, (unsigned long long)t);
    }
}
__global__ void __launch_bounds__(GRID_T)
grid_pass_a_kernel(const Setup S, const CloudSeg* __restrict__ seg, const int32_t* __restrict__ blk, int64_t total, ssm_grid_cell* __restrict__ cells,
                   unsigned long long* __restrict__ info)
{
    const int lane = threadIdx.x & 63;
    Hit h; uint32_t label;
    const int st = grid_point(S, seg, blk, total, &h, &label);
    if (st == P_USED) {
        ssm_grid_cell* c = cells + ((size_t)h.cy * (size_t)S.nx + (size_t)h.cx);
        GRID_COUNT(0); atomicAdd(&c->n, 1u);
        if (h.hq < c->hmin) { GRID_COUNT(0); atomicMin(&c->hmin, h.hq); }
        if (h.hq > c->hmax) { GRID_COUNT(0); atomicMax(&c->hmax, h.hq); }
    }
    grid_count_points(st, info);
}
// The aggregated forms.  Neighbouring pixels of a cloud fall into the same cell, so adjacent lanes of a wave often hold the same destination.  A RUN is a maximal
// stretch of adjacent lanes with one key; its first lane (the head) issues the run's atomics with the run's count, minimum, maximum or sum.  Integer terms: the
// same bits as one atomic per point.  run_end: the lane behind the run of this lane, from the ballot of the heads.
__device__ inline int grid_run_end(int key, int lane, bool* head)
{
    const int prev = __shfl_up(key, 1);
    *head = lane == 0 || key != prev;
    const unsigned long long heads = __ballot(*head);
    const unsigned long long behind = lane == 63 ? 0ull : heads >> (lane + 1);
    return behind ? lane + 1 + __ffsll((long long)behind) - 1 : 64;
}
__global__ void __launch_bounds__(GRID_T)
grid_pass_a_runs_kernel(const Setup S, const CloudSeg* __restrict__ seg, const int32_t* __restrict__ blk, int64_t total, ssm_grid_cell* __restrict__ cells,
                        unsigned long long* __restrict__ info)
{
    const int lane = threadIdx.x & 63;
    Hit h; uint32_t label;
    const int st = grid_point(S, seg, blk, total, &h, &label);
    const int key = st == P_USED ? h.cy * S.nx + h.cx : -1;          // (nx ny <= 2^24)
    bool head;
    const int end = grid_run_end(key, lane, &head);
    int lo = st == P_USED ? h.hq : HMIN_EMPTY, hi = st == P_USED ? h.hq : HMAX_EMPTY;
    for (int d = 1; d < 64; d <<= 1) {                                // after the step with d a lane holds its run's [lane, lane + 2 d) part
        const int a = __shfl_down(lo, d), b = __shfl_down(hi, d);
        if (lane + d < end) { lo = min(lo, a); hi = max(hi, b); }
    }
    if (head && key >= 0) {
        ssm_grid_cell* c = cells + key;
        GRID_COUNT(0); atomicAdd(&c->n, (uint32_t)(end - lane));
        if (lo < c->hmin) { GRID_COUNT(0); atomicMin(&c->hmin, lo); }
        if (hi > c->hmax) { GRID_COUNT(0); atomicMax(&c->hmax, hi); }
    }
    grid_count_points(st, info);
}
// key: the cell, LOW or HIGH, and the label's bin (12: none) -- what decides every address a point adds to
__global__ void __launch_bounds__(GRID_T)
grid_pass_b_runs_kernel(const Setup S, const CloudSeg* __restrict__ seg, const int32_t* __restrict__ blk, int64_t total, ssm_grid_cell* __restrict__ cells)
{
    const int lane = threadIdx.x & 63;
    Hit h; uint32_t label;
    const bool used = grid_point(S, seg, blk, total, &h, &label) == P_USED;
    int cell = 0; bool low = false; long long sum = 0;
    const int bin = label < (uint32_t)NLABEL ? (int)label : NLABEL;
    if (used) { cell = h.cy * S.nx + h.cx; low = is_low(h.hq, cells[cell].base, S.step_q); sum = h.hq; }
    const int key = used ? (cell << 5) | ((int)low << 4) | bin : -1;          // (cell < 2^24: below 2^29)
    bool head;
    const int end = grid_run_end(key, lane, &head);
    for (int d = 1; d < 64; d <<= 1) {
        const long long a = __shfl_down(sum, d);
        if (lane + d < end) sum += a;
    }
    if (head && used) {
        ssm_grid_cell* c = cells + cell;
        const uint32_t n = (uint32_t)(end - lane);
        if (low) {
            GRID_COUNT(1); atomicAdd(&c->n_low, n);
            GRID_COUNT(1); atomicAdd(reinterpret_cast<unsigned long long*>(&c->sum_low), (unsigned long long)sum);
            if (bin < NLABEL) { GRID_COUNT(1); atomicAdd(&c->hist_low[bin], n); }
        } else {
            GRID_COUNT(1); atomicAdd(&c->n_high, n);
            if (bin < NLABEL) { GRID_COUNT(1); atomicAdd(&c->hist_high[bin], n); }
        }
    }
}
__global__ void __launch_bounds__(GRID_T)
grid_ground_kernel(const Setup S, ssm_grid_cell* __restrict__ cells, int64_t nc)
{
    const int64_t i = (int64_t)blockIdx.x * GRID_T + threadIdx.x;
    if (i >= nc) return;
    if (cells[i].n == 0) return;
    const int cx = (int)(i % S.nx), cy = (int)(i / S.nx);
    const int x0 = max(cx - S.ground_radius, 0), x1 = min(cx + S.ground_radius, S.nx - 1), y0 = max(cy - S.ground_radius, 0), y1 = min(cy + S.ground_radius, S.ny - 1);
    int32_t b = BASE_EMPTY;
    for (int y = y0; y <= y1; y++) {
        const ssm_grid_cell* row = cells + (size_t)y * (size_t)S.nx;
        for (int x = x0; x <= x1; x++) {
            const uint2 w = *reinterpret_cast<const uint2*>(row + x);          // n, hmin
            if (w.x && (int32_t)w.y < b) b = (int32_t)w.y;
        }
    }
    cells[i].base = b;
}
__global__ void __launch_bounds__(GRID_T)
grid_pass_b_kernel(const Setup S, const CloudSeg* __restrict__ seg, const int32_t* __restrict__ blk, int64_t total, ssm_grid_cell* __restrict__ cells)
{
    Hit h; uint32_t label;
    if (grid_point(S, seg, blk, total, &h, &label) != P_USED) return;
    ssm_grid_cell* c = cells + ((size_t)h.cy * (size_t)S.nx + (size_t)h.cx);
    if (is_low(h.hq, c->base, S.step_q)) {
        GRID_COUNT(1); atomicAdd(&c->n_low, 1u);
        GRID_COUNT(1); atomicAdd(reinterpret_cast<unsigned long long*>(&c->sum_low), (unsigned long long)(long long)h.hq);
        if (label < (uint32_t)NLABEL) { GRID_COUNT(1); atomicAdd(&c->hist_low[label], 1u); }
    } else {
        GRID_COUNT(1); atomicAdd(&c->n_high, 1u);
        if (label < (uint32_t)NLABEL) { GRID_COUNT(1); atomicAdd(&c->hist_high[label], 1u); }
    }
}
__global__ void __launch_bounds__(GRID_T)
grid_resolve_kernel(const ssm_grid_cell* __restrict__ cells, int64_t nc, int32_t min_obstacle_points, uint8_t* __restrict__ cls, uint8_t* __restrict__ ground_label,
                    uint8_t* __restrict__ obstacle_label, int32_t* __restrict__ ground_q, int32_t* __restrict__ top_q, uint32_t* __restrict__ n, uint32_t* __restrict__ n_high,
                    unsigned long long* __restrict__ info)
{
    __shared__ uint32_t cnt_s[GRID_W][6];
    const int64_t i = (int64_t)blockIdx.x * GRID_T + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int k = -1; uint32_t used = 0;
    if (i < nc) {
        const ssm_grid_cell c = cells[i];
        const Resolved r = resolve_of(c, min_obstacle_points);
        k = r.cls; used = c.n;
        cls[i] = r.cls; ground_label[i] = r.ground_label; obstacle_label[i] = r.obstacle_label; ground_q[i] = r.ground_q; top_q[i] = r.top_q; n[i] = c.n; n_high[i] = c.n_high;
    }
    const int c0 = __popcll(__ballot(k == UNOBSERVED)), c1 = __popcll(__ballot(k == DRIVABLE)), c2 = __popcll(__ballot(k == WALKABLE)),
              c3 = __popcll(__ballot(k == OTHER_GROUND)), c4 = __popcll(__ballot(k == OBSTACLE));
    for (int d = 32; d; d >>= 1) used += __shfl_down(used, d);          // the used points of the wave's cells (a call has fewer than 2^31)
    if (lane == 0) { uint32_t* r = cnt_s[wave]; r[0] = used; r[1] = (uint32_t)c0; r[2] = (uint32_t)c1; r[3] = (uint32_t)c2; r[4] = (uint32_t)c3; r[5] = (uint32_t)c4; }
    __syncthreads();
    if (threadIdx.x < 6) {          // info[4]: n_used, info[5 .. 9]: the cells by class
        uint32_t t = 0;
        for (int w = 0; w < GRID_W; w++) t += cnt_s[w][threadIdx.x];
        if (t) atomicAdd(info + 4 + threadIdx.x, (unsigned long long)t);
    }
}

// ------------------------------------------------------------------ launcher
static inline unsigned grid_blocks(int64_t n) { return (unsigned)((n + GRID_T - 1) / GRID_T); }
hipError_t k_grid(const Setup& S, const CloudSeg* seg, const int32_t* blk, int64_t total, const GridBufs& T, unsigned long long* info, int form, hipStream_t s)
{
    const int64_t nc = (int64_t)S.nx * S.ny;
    grid_clear_kernel<<<grid_blocks(nc * 8), GRID_T, 0, s>>>(reinterpret_cast<uint4*>(T.cells), nc * 8, info, total);
    if (total > 0) {
        if (form == GRID_FORM_RUNS) grid_pass_a_runs_kernel<<<grid_blocks(total), GRID_T, 0, s>>>(S, seg, blk, total, T.cells, info);
        else grid_pass_a_kernel<<<grid_blocks(total), GRID_T, 0, s>>>(S, seg, blk, total, T.cells, info);
        grid_ground_kernel<<<grid_blocks(nc), GRID_T, 0, s>>>(S, T.cells, nc);
        if (form == GRID_FORM_RUNS) grid_pass_b_runs_kernel<<<grid_blocks(total), GRID_T, 0, s>>>(S, seg, blk, total, T.cells);
        else grid_pass_b_kernel<<<grid_blocks(total), GRID_T, 0, s>>>(S, seg, blk, total, T.cells);
    }
    grid_resolve_kernel<<<grid_blocks(nc), GRID_T, 0, s>>>(T.cells, nc, S.min_obstacle_points, T.cls, T.ground_label, T.obstacle_label, T.ground_q, T.top_q, T.n, T.n_high, info);
    return hipGetLastError();
}
