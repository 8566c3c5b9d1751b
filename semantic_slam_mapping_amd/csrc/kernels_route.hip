// kernels_route.hip -- the route field on the device.  The arithmetic is include/ssm/route_core.h, which the host functions of
// ssm_route_host.cpp call too.
//
// A cost is the minimum over paths of a sum of integers, so it is the fixed point of "a cell's cost is the smallest of its own and every neighbour's cost plus the
// edge between them" started from 0 at the source and COST_NONE elsewhere: every value ever written is the cost of some real path, values only fall, and the
// relaxation may read a neighbour's older or newer value in any order without changing where it ends.  Both forms are that relaxation; they differ in how much
// of it one launch does.
// BEGIN: one thread per cell makes the cell's byte (takes part, is NEAR), copies dist2 into the target and sets the costs.
// FORM 0, the baseline: rt_sweep_kernel, one thread per cell pulls from its neighbours in global memory; RT_BATCH sweeps are queued, then the host reads one
// "changed" word and stops at the first batch that changed nothing (its last sweep read nothing that moved: a fixed point).
// FORM 1: rt_tile_kernel, one block per ACTIVE 32 x 32 tile.  The block stages the tile's costs and weights with a halo of one cell in LDS and relaxes until a
// block-wide vote says that nothing fell -- a loop bounded by the data, since every productive pass lowers at least one of 1024 bounded integers.  It writes back
// the cells that changed, and where one of them lies on the tile's rim it marks the neighbouring tiles that cell touches.  Cells of a tile are written only by
// that tile's block, so a halo read that races with a neighbour's write-back sees the value the neighbour started the round with or the one it ends with; the
// older one at worst costs a round, because the neighbour's rim change marks this tile again.  rt_compact_kernel turns the marks into the next round's list, one
// atomic per wave; the host reads the count and launches that many blocks.  No block waits for another, no grid barrier.
// FINISH: every routed cell's parent, the minimum of the key (cost through p << 24) | p over the moves that exist, and the counts -- per wave by shuffle, per block
// through LDS, one atomic per block and non-zero count, from at most RT_GRID blocks that walk the cells; the farthest cell is one 64-bit atomicMax per block.
// PATH: the goal's snap as the clearance seed's (one thread per cell of the window, a wave minimum, one 64-bit atomicMin per wave that found a routed cell), then
// ONE wave: its first lane follows the parents from the goal, a chain of dependent loads, and the wave turns the cells round.
#include "ssm_internal.h"
using namespace ssm_rtc;

#define RT_T 256
#define RT_W (RT_T / 64)
#define RT_TW 32
#define RT_TH 32
#define RT_PX (RT_TW * RT_TH)
#define RT_K (RT_PX / RT_T)
#define RT_HW (RT_TW + 2)
#define RT_HPX (RT_HW * (RT_TH + 2))
#define RT_GRID 1024
#define RT_BATCH 16
int k_route_tile() { return RT_TW; }
int k_route_batch() { return RT_BATCH; }
int64_t k_route_tiles(int nx, int ny) { return (int64_t)((nx + RT_TW - 1) / RT_TW) * ((ny + RT_TH - 1) / RT_TH); }
static_assert(RT_TW == RT_TH && RT_PX % RT_T == 0 && RT_T % RT_TW == 0, "whole rows of a square tile per pass of the block");

// the marks of a tile's rim: which neighbouring tiles a changed cell touches
enum { WOKE_L = 1, WOKE_R = 2, WOKE_U = 4, WOKE_D = 8, WOKE_UL = 16, WOKE_UR = 32, WOKE_DL = 64, WOKE_DR = 128 };

__device__ __forceinline__ uint32_t rt_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void rt_store(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t rt_lds_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void rt_lds_store(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// ------------------------------------------------------------------ begin
// The first round's tiles: the source's and its up to eight neighbours -- a source on its tile's rim whose neighbours inside the tile take no part changes nothing
// there, so no rim change would ever wake the tile next door
struct RtFirst { int32_t n, tile[9]; };
// one thread per cell (and at least 16 threads: the info's nine words, the ring's two, the first tiles); tiles <= cells
__global__ void __launch_bounds__(RT_T)
rt_begin_kernel(const uint8_t* __restrict__ reach, const uint32_t* __restrict__ dist2, int64_t nc, int64_t tiles, int32_t source, const RtFirst first, long long comfort2,
                uint8_t* __restrict__ in, uint32_t* __restrict__ d2, uint32_t* __restrict__ cost, int32_t* __restrict__ flag, int32_t* __restrict__ list,
                unsigned long long* __restrict__ info, int32_t* __restrict__ ctl)
{
    const int64_t t = (int64_t)blockIdx.x * RT_T + threadIdx.x;
    if (t < 9) info[t] = 0ull;
    if (t < 2) ctl[t] = 0;
    if (t < tiles) { flag[t] = 0; list[t] = t < first.n ? first.tile[t] : 0; }
    if (t >= nc) return;
    const uint32_t d = dist2[t];
    in[t] = cell_byte(reach[t], d, (int64_t)comfort2);
    d2[t] = d;
    cost[t] = t == (int64_t)source ? 0u : COST_NONE;
}

// ------------------------------------------------------------------ form 0
// the smallest of a cell's cost and what its neighbours offer, from global memory.  (cx, cy) takes part with the byte b and the cost c
template <int MOVES>
__device__ __forceinline__ uint32_t rt_pull(const uint8_t* __restrict__ in, const uint32_t* cost, int nx, int ny, int cx, int cy, uint8_t b, uint32_t c, int near_weight)
{
    const uint32_t wc = weight_of(b, near_weight);
    uint32_t best = c;
#pragma unroll
    for (int m = 0; m < MOVES; m++) {
        const int dx = move_dx(m), dy = move_dy(m), x = cx + dx, y = cy + dy;
        if (x < 0 || y < 0 || x >= nx || y >= ny) continue;
        const size_t j = (size_t)y * nx + x;
        const uint8_t bn = in[j];
        if (!bn) continue;
        if (m >= 4 && !(in[(size_t)cy * nx + x] && in[(size_t)y * nx + cx])) continue;          // no corner is cut
        const uint32_t cn = rt_load(cost + j);
        if (cn == COST_NONE) continue;
        best = min(best, cn + edge_of(m < 4 ? STEP_AXIAL : STEP_DIAG, wc, weight_of(bn, near_weight)));
    }
    return best;
}
template <int MOVES>
__global__ void __launch_bounds__(RT_T)
rt_sweep_kernel(const uint8_t* __restrict__ in, uint32_t* cost, int nx, int ny, int64_t nc, int near_weight, int32_t* changed)
{
    const int64_t t = (int64_t)blockIdx.x * RT_T + threadIdx.x;
    bool fell = false;
    if (t < nc) {
        const uint8_t b = in[t];
        if (b) {
            const uint32_t c = rt_load(cost + t);          // (only this thread writes the cell)
            const uint32_t best = rt_pull<MOVES>(in, cost, nx, ny, (int)(t % nx), (int)(t / nx), b, c, near_weight);
            if (best < c) { rt_store(cost + t, best); fell = true; }
        }
    }
    if (__any(fell) && (threadIdx.x & 63) == 0) atomicOr(changed, 1);
}

// ------------------------------------------------------------------ form 1
template <int MOVES>
__global__ void __launch_bounds__(RT_T)
rt_tile_kernel(const uint8_t* __restrict__ in, uint32_t* cost, int nx, int ny, int tiles_x, int tiles_y, int near_weight, const int32_t* __restrict__ list, int32_t* flag)
{
    __shared__ uint32_t cs[RT_HPX];
    __shared__ uint8_t ws[RT_HPX];          // a cell's weight, 0: it does not take part (or lies outside the grid)
    __shared__ int woke_s;
    const int tile = list[blockIdx.x], tile_x = tile % tiles_x, tile_y = tile / tiles_x;
    const int tx0 = tile_x * RT_TW, ty0 = tile_y * RT_TH;
    for (int i = threadIdx.x; i < RT_HPX; i += RT_T) {
        const int gx = tx0 - 1 + i % RT_HW, gy = ty0 - 1 + i / RT_HW;
        uint8_t w = 0; uint32_t c = COST_NONE;
        if (gx >= 0 && gy >= 0 && gx < nx && gy < ny) {
            const size_t g = (size_t)gy * nx + gx;
            const uint8_t b = in[g];
            if (b) { w = (uint8_t)weight_of(b, near_weight); c = rt_load(cost + g); }
        }
        ws[i] = w; cs[i] = c;
    }
    if (threadIdx.x == 0) woke_s = 0;
    __syncthreads();
    uint32_t c0[RT_K];
#pragma unroll
    for (int k = 0; k < RT_K; k++) {
        const int i = threadIdx.x + k * RT_T, h = (i / RT_TW + 1) * RT_HW + i % RT_TW + 1;
        c0[k] = cs[h];
    }
    // to the tile's fixed point: a pass reads its neighbours' costs of this pass or the one before -- either is the cost of a real path
    for (;;) {
        bool fell = false;
#pragma unroll
        for (int k = 0; k < RT_K; k++) {
            const int i = threadIdx.x + k * RT_T, h = (i / RT_TW + 1) * RT_HW + i % RT_TW + 1;
            const uint32_t w = ws[h];
            if (!w) continue;
            const uint32_t c = rt_lds_load(cs + h);
            uint32_t best = c;
#pragma unroll
            for (int m = 0; m < MOVES; m++) {
                const int dx = move_dx(m), dy = move_dy(m), j = h + dy * RT_HW + dx;
                const uint32_t wn = ws[j];
                if (!wn) continue;
                if (m >= 4 && !(ws[h + dx] && ws[h + dy * RT_HW])) continue;          // no corner is cut
                const uint32_t cn = rt_lds_load(cs + j);
                if (cn == COST_NONE) continue;
                best = min(best, cn + edge_of(m < 4 ? STEP_AXIAL : STEP_DIAG, w, wn));
            }
            if (best < c) { rt_lds_store(cs + h, best); fell = true; }
        }
        if (!__syncthreads_or(fell)) break;
    }
    int woke = 0;
#pragma unroll
    for (int k = 0; k < RT_K; k++) {
        const int i = threadIdx.x + k * RT_T, lx = i % RT_TW, ly = i / RT_TW, h = (ly + 1) * RT_HW + lx + 1;
        const uint32_t c = cs[h];
        if (c == c0[k]) continue;
        rt_store(cost + (size_t)(ty0 + ly) * nx + tx0 + lx, c);          // (a cell that changed takes part: it lies inside the grid)
        const bool l = lx == 0, r = lx == RT_TW - 1, u = ly == 0, d = ly == RT_TH - 1;
        woke |= (l ? WOKE_L : 0) | (r ? WOKE_R : 0) | (u ? WOKE_U : 0) | (d ? WOKE_D : 0) | (l && u ? WOKE_UL : 0) | (r && u ? WOKE_UR : 0) | (l && d ? WOKE_DL : 0) | (r && d ? WOKE_DR : 0);
    }
    if (woke) atomicOr(&woke_s, woke);
    __syncthreads();
    if (threadIdx.x < 8 && ((woke_s >> threadIdx.x) & 1)) {
        const int n = threadIdx.x;
        const int dx = (n == 0 || n == 4 || n == 6) ? -1 : (n == 1 || n == 5 || n == 7) ? 1 : 0;
        const int dy = (n == 2 || n == 4 || n == 5) ? -1 : (n == 3 || n == 6 || n == 7) ? 1 : 0;
        const int x = tile_x + dx, y = tile_y + dy;
        if (x >= 0 && y >= 0 && x < tiles_x && y < tiles_y) atomicOr(flag + (size_t)y * tiles_x + x, 1);
    }
}
// the marked tiles -> list, their number -> *count (zero before this launch); the marks are cleared, and *next_count for the round after
__global__ void __launch_bounds__(RT_T)
rt_compact_kernel(int32_t* flag, int tiles, int32_t* __restrict__ list, int32_t* count, int32_t* next_count)
{
    const int t = blockIdx.x * RT_T + threadIdx.x, lane = threadIdx.x & 63;
    const bool f = t < tiles && flag[t] != 0;
    if (f) flag[t] = 0;
    if (t == 0) *next_count = 0;
    const unsigned long long ballot = __ballot(f);
    if (!ballot) return;
    int base = 0;
    if (lane == 0) base = atomicAdd(count, __popcll(ballot));
    base = __shfl(base, 0);
    if (f) list[base + __popcll(ballot & ((1ull << lane) - 1ull))] = t;
}

// ------------------------------------------------------------------ finish
// the block's sum of v -> *slot: per wave by shuffle, per block through LDS, one atomic per block and none for a sum of 0.  Every thread calls this
__device__ inline void rt_block_add(int v, int* cnt_s, unsigned long long* slot)
{
    for (int d = 32; d; d >>= 1) v += __shfl_down(v, d);
    __syncthreads();                                     // (cnt_s may still be read from the previous call)
    if ((threadIdx.x & 63) == 0) cnt_s[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int k = 0; k < RT_W; k++) t += cnt_s[k];
        if (t) atomicAdd(slot, (unsigned long long)t);
    }
}
// info: [0] routed, [1] unrouted, [2] near_cells, [8] the largest far key of a routed cell (the host reads max_cost and far_cell from it when routed > 0)
template <int MOVES>
__global__ void __launch_bounds__(RT_T)
rt_finish_kernel(const uint8_t* __restrict__ in, const uint32_t* __restrict__ cost, int nx, int ny, int64_t nc, int32_t source, int near_weight, int32_t* __restrict__ parent,
                 unsigned long long* __restrict__ info)
{
    __shared__ int cnt_s[RT_W];
    __shared__ unsigned long long far_s[RT_W];
    int routed = 0, unrouted = 0, near = 0; unsigned long long far = 0ull;
    for (int64_t t = (int64_t)blockIdx.x * RT_T + threadIdx.x; t < nc; t += (int64_t)gridDim.x * RT_T) {          // (a block's counts stay below 2^31: at most 2^24 cells in all)
        const uint8_t b = in[t];
        int32_t par = -1;
        if (b) {
            const uint32_t c = cost[t];
            if (c == COST_NONE) unrouted++;
            else {
                routed++; near += (b & CELL_NEAR) ? 1 : 0;
                far = max(far, far_key(c, (int32_t)t));
                if (t != (int64_t)source) {
                    const int cx = (int)(t % nx), cy = (int)(t / nx);
                    const uint32_t wc = weight_of(b, near_weight);
                    unsigned long long best = ssm_clrc::KEY_NONE;
#pragma unroll
                    for (int m = 0; m < MOVES; m++) {
                        const int dx = move_dx(m), dy = move_dy(m), x = cx + dx, y = cy + dy;
                        if (x < 0 || y < 0 || x >= nx || y >= ny) continue;
                        const size_t j = (size_t)y * nx + x;
                        const uint8_t bn = in[j];
                        if (!bn) continue;
                        if (m >= 4 && !(in[(size_t)cy * nx + x] && in[(size_t)y * nx + cx])) continue;
                        const uint32_t cn = cost[j];
                        if (cn == COST_NONE) continue;
                        const unsigned long long key = parent_key(cn + edge_of(m < 4 ? STEP_AXIAL : STEP_DIAG, weight_of(bn, near_weight), wc), (int32_t)j);
                        best = key < best ? key : best;
                    }
                    par = (int32_t)(best & (unsigned long long)INDEX_MASK);          // (a routed cell other than the source has a routed neighbour: its cost came from one)
                }
            }
        }
        parent[t] = par;
    }
    rt_block_add(routed, cnt_s, info + 0);
    rt_block_add(unrouted, cnt_s, info + 1);
    rt_block_add(near, cnt_s, info + 2);
    for (int d = 32; d; d >>= 1) { const unsigned long long o = __shfl_down(far, d); far = o > far ? o : far; }
    if ((threadIdx.x & 63) == 0) far_s[threadIdx.x >> 6] = far;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long m = 0ull;
        for (int k = 0; k < RT_W; k++) m = far_s[k] > m ? far_s[k] : m;
        if (m) atomicMax(info + 8, m);
    }
}

// ------------------------------------------------------------------ the path
// one thread per cell of the (2 snap + 1)^2 window around the goal -> pinfo[7], the smallest key among the window's routed cells within the snap distance
__global__ void __launch_bounds__(RT_T)
rt_snap_kernel(const uint32_t* __restrict__ cost, int nx, int ny, const ssm_clrc::Setup G, unsigned long long* __restrict__ pinfo)
{
    const int side = 2 * G.seed_snap + 1;
    const int64_t t = (int64_t)blockIdx.x * RT_T + threadIdx.x;
    unsigned long long key = ssm_clrc::KEY_NONE;
    if (t < (int64_t)side * side) {
        const int cx = G.seed_cx - G.seed_snap + (int)(t % side), cy = G.seed_cy - G.seed_snap + (int)(t / side);
        if (cx >= 0 && cy >= 0 && cx < nx && cy < ny && cost[(size_t)cy * nx + cx] != COST_NONE) key = ssm_clrc::seed_key(cx, cy, nx, G);
    }
    for (int d = 32; d; d >>= 1) { const unsigned long long o = __shfl_down(key, d); key = o < key ? o : key; }
    if ((threadIdx.x & 63) == 0 && key != ssm_clrc::KEY_NONE) atomicMin(pinfo + 7, key);
}
// one wave.  pinfo: [0] len, [1] goal_cell, [2] cost, [3] n_axial, [4] n_diag, [5] near_steps, [6] min_d2 (ssm_route_path_info), [7] the goal's key.  rev gets the
// first max_path cells of the walk, goal first; path the whole walk, source first, when it has at most max_path cells
__global__ void __launch_bounds__(64)
rt_walk_kernel(const uint32_t* __restrict__ cost, const int32_t* __restrict__ parent, const uint32_t* __restrict__ d2, int nx, int64_t nc, long long comfort2, int max_path,
               int32_t* rev, int32_t* __restrict__ path, unsigned long long* pinfo)
{
    __shared__ long long len_s;
    if (threadIdx.x == 0) {
        const unsigned long long key = pinfo[7];          // (written by rt_snap_kernel, an earlier launch)
        long long len = 0, goal = -1, total = -1, axial = 0, diag = 0, near = 0, min_d2 = -1;
        if (key != ssm_clrc::KEY_NONE) {
            goal = (long long)(key & (unsigned long long)INDEX_MASK);
            total = (long long)cost[goal]; min_d2 = (long long)d2[goal];
            // costs strictly fall along parents: the walk ends at the source after fewer than nc steps
            for (int32_t a = (int32_t)goal; len < nc;) {
                if (len < max_path) rev[len] = a;
                len++;
                const uint32_t dd = d2[a];
                const int32_t p = parent[a];
                min_d2 = min(min_d2, (long long)dd);
                near += near_of(dd, (int64_t)comfort2) ? 1 : 0;
                if (p < 0) break;
                if (step_is_diag(a, p, nx)) diag++; else axial++;
                a = p;
            }
        }
        pinfo[0] = (unsigned long long)len; pinfo[1] = (unsigned long long)goal; pinfo[2] = (unsigned long long)total; pinfo[3] = (unsigned long long)axial;
        pinfo[4] = (unsigned long long)diag; pinfo[5] = (unsigned long long)near; pinfo[6] = (unsigned long long)min_d2;
        len_s = len;
    }
    __syncthreads();          // (the first lane's stores to rev are visible to the wave behind the barrier)
    const long long len = len_s;
    if (len > max_path) return;
    for (long long i = threadIdx.x; i < len; i += 64) path[i] = __hip_atomic_load(rev + (len - 1 - i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------ launchers
static inline unsigned rt_blocks(int64_t n) { return (unsigned)((n + RT_T - 1) / RT_T); }
hipError_t k_route_begin(const uint8_t* reach, const uint32_t* dist2, int nx, int ny, int32_t source, const Setup& S, const RouteBufs& B, unsigned long long* info, int32_t* ctl,
                         int* n_first, hipStream_t s)
{
    const int64_t nc = (int64_t)nx * ny;
    const int tiles_x = (nx + RT_TW - 1) / RT_TW, tiles_y = (ny + RT_TH - 1) / RT_TH;
    RtFirst first; first.n = 0;
    if (source >= 0) {
        const int sx = source % nx / RT_TW, sy = source / nx / RT_TH;
        for (int y = std::max(0, sy - 1); y <= std::min(tiles_y - 1, sy + 1); y++)
            for (int x = std::max(0, sx - 1); x <= std::min(tiles_x - 1, sx + 1); x++) first.tile[first.n++] = y * tiles_x + x;
    }
    *n_first = first.n;
    rt_begin_kernel<<<rt_blocks(std::max<int64_t>(nc, 16)), RT_T, 0, s>>>(reach, dist2, nc, k_route_tiles(nx, ny), source, first, (long long)S.comfort2, B.in, B.d2, B.cost, B.flag, B.list, info,
                                                                         ctl);
    return hipGetLastError();
}
hipError_t k_route_sweeps(int nx, int ny, const Setup& S, const RouteBufs& B, int32_t* changed, hipStream_t s)
{
    const int64_t nc = (int64_t)nx * ny;
    hipError_t e = hipMemsetAsync(changed, 0, 4, s);
    if (e != hipSuccess) return e;
    for (int k = 0; k < RT_BATCH; k++) {
        if (S.moves == 8) rt_sweep_kernel<8><<<rt_blocks(nc), RT_T, 0, s>>>(B.in, B.cost, nx, ny, nc, S.near_weight, changed);
        else rt_sweep_kernel<4><<<rt_blocks(nc), RT_T, 0, s>>>(B.in, B.cost, nx, ny, nc, S.near_weight, changed);
    }
    return hipGetLastError();
}
hipError_t k_route_round(int nx, int ny, const Setup& S, const RouteBufs& B, int n_active, int round, int32_t* ctl, hipStream_t s)
{
    const int tiles_x = (nx + RT_TW - 1) / RT_TW, tiles_y = (ny + RT_TH - 1) / RT_TH, tiles = tiles_x * tiles_y;
    if (n_active < 1 || n_active > tiles) return hipErrorInvalidValue;
    if (S.moves == 8) rt_tile_kernel<8><<<n_active, RT_T, 0, s>>>(B.in, B.cost, nx, ny, tiles_x, tiles_y, S.near_weight, B.list, B.flag);
    else rt_tile_kernel<4><<<n_active, RT_T, 0, s>>>(B.in, B.cost, nx, ny, tiles_x, tiles_y, S.near_weight, B.list, B.flag);
    rt_compact_kernel<<<rt_blocks(tiles), RT_T, 0, s>>>(B.flag, tiles, B.list, ctl + (round & 1), ctl + ((round + 1) & 1));
    return hipGetLastError();
}
hipError_t k_route_finish(int nx, int ny, int32_t source, const Setup& S, const RouteBufs& B, unsigned long long* info, hipStream_t s)
{
    const int64_t nc = (int64_t)nx * ny;
    const unsigned walkers = std::min<unsigned>(rt_blocks(nc), RT_GRID);
    if (S.moves == 8) rt_finish_kernel<8><<<walkers, RT_T, 0, s>>>(B.in, B.cost, nx, ny, nc, source, S.near_weight, B.parent, info);
    else rt_finish_kernel<4><<<walkers, RT_T, 0, s>>>(B.in, B.cost, nx, ny, nc, source, S.near_weight, B.parent, info);
    return hipGetLastError();
}
hipError_t k_route_path(int nx, int ny, const Setup& S, const RouteBufs& B, int goal_cx, int goal_cy, int goal_snap, int max_path, int32_t* rev, int32_t* path, unsigned long long* pinfo,
                        hipStream_t s)
{
    hipError_t e = hipMemsetAsync(pinfo + 7, 0xFF, 8, s);          // KEY_NONE
    if (e != hipSuccess) return e;
    const int side = 2 * goal_snap + 1;
    rt_snap_kernel<<<rt_blocks((int64_t)side * side), RT_T, 0, s>>>(B.cost, nx, ny, goal_setup(goal_cx, goal_cy, goal_snap), pinfo);
    rt_walk_kernel<<<1, 64, 0, s>>>(B.cost, B.parent, B.d2, nx, (int64_t)nx * ny, (long long)S.comfort2, max_path, rev, path, pinfo);
    return hipGetLastError();
}
