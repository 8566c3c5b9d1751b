// kernels_clearance.hip -- the clearance map on the device.  The arithmetic is include/ssm/clearance_core.h, which the host function of
// ssm_clearance_host.cpp calls too.
//
// The distance transform is separable.  COLUMN PASS: the blocked cells of 32 rows of a column become one 32-bit mask (clr_mask_kernel, one thread per column and
// band of 32 rows, loads coalesced across cx); clr_column_kernel then gives every cell the nearest blocked row of its own column -- bit tricks inside the band, the
// nearest non-empty band above and below found by walking the masks, a walk bounded by the number of bands.  ROW PASS, the hot path: a cell's key is the minimum
// over the columns x' of its row of ((cx - x')^2 + dy(x', cy)^2, index of that column's blocked cell).  Form 0 stages the row's column answers through LDS in
// chunks of CLR_CHUNK and every thread evaluates every entry (an LDS broadcast read, a uniform branch on "this column holds nothing").  Form 1 scans outwards
// from cx in global memory and stops once the step k has k^2 above the best squared distance so far (equal still has to be looked at: it may tie with a lower
// index); neighbouring lanes read neighbouring addresses and stop within a step or two of each other.  Both are a minimum of the same keys: the same bits.
// SEED: one thread per cell of the snap window, a wave minimum by shuffles, one 64-bit atomicMin per wave that found a candidate.  LABELLING of the traversable
// mask: kernels_objects.hip's order-independent union-find restated without a label in the join test (a forest per 32 x 32 tile in LDS, rim unions with atomicMin,
// a flatten pass; entries only ever decrease, so every loop is bounded by the data; no block waits for another, no grid barrier).  FINISH: reach and the counts,
// per wave by shuffle, per block through LDS, one atomic per block and non-zero count, from at most CLR_GRID blocks that walk the cells; the seed and its root are
// read on the device.
#include "ssm_internal.h"
#include "../../include/ssm/clearance_core.h"
using namespace ssm_clrc;

#define CLR_T 256
#define CLR_W (CLR_T / 64)
#define CLR_CHUNK 256
#define CLR_BAND 32
#define CLR_TW 32
#define CLR_TH 32
#define CLR_PX (CLR_TW * CLR_TH)
#define CLR_K (CLR_PX / CLR_T)
#define CLR_GRID 1024
int k_clearance_chunk() { return CLR_CHUNK; }
static_assert(CLR_CHUNK == CLR_T, "a block stages one entry per thread");
static_assert(CLR_PX % CLR_T == 0 && CLR_T % CLR_TW == 0, "whole rows of a tile per pass of the block");

// info: [0] blocked, [1] free_cells, [2] traversable, [3] components, [4] reachable, [5] seed_cell, [6] max_d2_reachable, [7] r2 (ssm_clearance_info), [8] the seed's key
__global__ void __launch_bounds__(64)
clr_begin_kernel(unsigned long long* __restrict__ info)
{
    if (threadIdx.x < 8) info[threadIdx.x] = 0ull;
    if (threadIdx.x == 8) info[8] = KEY_NONE;
}

// ------------------------------------------------------------------ column pass
// mask[band nx + cx]: bit j = the cell (cx, 32 band + j) is blocked
__global__ void __launch_bounds__(CLR_T)
clr_mask_kernel(const uint8_t* __restrict__ cls, int nx, int ny, int bands, uint32_t blocked_mask, uint32_t* __restrict__ mask)
{
    const int64_t t = (int64_t)blockIdx.x * CLR_T + threadIdx.x;
    if (t >= (int64_t)bands * nx) return;
    const int cx = (int)(t % nx), band = (int)(t / nx), y0 = band * CLR_BAND, rows = min(CLR_BAND, ny - y0);
    uint32_t m = 0;
    for (int j = 0; j < rows; j++) if (in_mask(cls[(size_t)(y0 + j) * nx + cx], blocked_mask)) m |= 1u << j;
    mask[t] = m;
}
// row[i]: the blocked row of cell i's column nearest to it, the lower on a tie, -1 when the column holds none
__global__ void __launch_bounds__(CLR_T)
clr_column_kernel(const uint32_t* __restrict__ mask, int nx, int ny, int bands, int32_t* __restrict__ row)
{
    const int64_t t = (int64_t)blockIdx.x * CLR_T + threadIdx.x;
    if (t >= (int64_t)bands * nx) return;
    const int cx = (int)(t % nx), band = (int)(t / nx), y0 = band * CLR_BAND, rows = min(CLR_BAND, ny - y0);
    const uint32_t m = mask[t];
    int32_t above = -1, below = -1;                      // the nearest blocked row below the band's first row, and above its last
    for (int b = band - 1; b >= 0; b--) { const uint32_t q = mask[(size_t)b * nx + cx]; if (q) { above = b * CLR_BAND + 31 - __clz((int)q); break; } }
    for (int b = band + 1; b < bands; b++) { const uint32_t q = mask[(size_t)b * nx + cx]; if (q) { below = b * CLR_BAND + __ffs((int)q) - 1; break; } }
    for (int j = 0; j < rows; j++) {
        const uint32_t upto = m & (0xFFFFFFFFu >> (31 - j)), from = m & (0xFFFFFFFFu << j);
        const int32_t lo = upto ? y0 + 31 - __clz((int)upto) : above, hi = from ? y0 + __ffs((int)from) - 1 : below;
        row[(size_t)(y0 + j) * nx + cx] = nearer_row(y0 + j, lo, hi);
    }
}

// ------------------------------------------------------------------ row pass
// form 0: block b covers the cells [CLR_T (b % xblocks), ...) of row b / xblocks; the whole row goes through LDS, CLR_CHUNK columns at a time
__global__ void __launch_bounds__(CLR_T)
clr_row_lds_kernel(const int32_t* __restrict__ row, int nx, int xblocks, uint32_t* __restrict__ dist2, int32_t* __restrict__ nearest)
{
    __shared__ int32_t r_s[CLR_CHUNK];
    const int cy = blockIdx.x / xblocks, cx = (blockIdx.x % xblocks) * CLR_T + threadIdx.x;
    const int32_t* R = row + (size_t)cy * nx;
    uint32_t best = D2_NONE; int32_t at = -1;
    for (int x0 = 0; x0 < nx; x0 += CLR_CHUNK) {
        const int n = min(CLR_CHUNK, nx - x0);
        __syncthreads();                                 // (the previous chunk has been read by every thread)
        if ((int)threadIdx.x < n) r_s[threadIdx.x] = R[x0 + threadIdx.x];
        __syncthreads();
        for (int k = 0; k < n; k++) {
            const int32_t r = r_s[k];                    // (one address for the whole wave: a broadcast, and the branch is uniform)
            if (r < 0) continue;
            const uint32_t d2 = d2_of(cx - (x0 + k), cy - r);
            const int32_t idx = r * nx + x0 + k;
            if (better(d2, idx, best, at)) { best = d2; at = idx; }
        }
    }
    if (cx < nx) { dist2[(size_t)cy * nx + cx] = best; nearest[(size_t)cy * nx + cx] = at; }
}
// form 1: one thread per cell, outwards from its own column; step k looks at cx - k and cx + k; the scan ends before the first step whose k^2 exceeds the best distance
__global__ void __launch_bounds__(CLR_T)
clr_row_scan_kernel(const int32_t* __restrict__ row, int nx, int64_t nc, uint32_t* __restrict__ dist2, int32_t* __restrict__ nearest)
{
    const int64_t t = (int64_t)blockIdx.x * CLR_T + threadIdx.x;
    if (t >= nc) return;
    const int cy = (int)(t / nx), cx = (int)(t % nx);
    const int32_t* R = row + (size_t)cy * nx;
    uint32_t best = D2_NONE; int32_t at = -1;
    const int reach = max(cx, nx - 1 - cx);
    for (int k = 0; k <= reach; k++) {
        if (at >= 0 && (uint32_t)k * (uint32_t)k > best) break;          // (k < 2^15: the square fits)
        const int xl = cx - k, xr = cx + k;
        if (xl >= 0) {
            const int32_t r = R[xl];
            if (r >= 0) { const uint32_t d2 = d2_of(k, cy - r); const int32_t idx = r * nx + xl; if (better(d2, idx, best, at)) { best = d2; at = idx; } }
        }
        if (k > 0 && xr < nx) {
            const int32_t r = R[xr];
            if (r >= 0) { const uint32_t d2 = d2_of(k, cy - r); const int32_t idx = r * nx + xr; if (better(d2, idx, best, at)) { best = d2; at = idx; } }
        }
    }
    dist2[t] = best; nearest[t] = at;
}

// ------------------------------------------------------------------ the seed
// one thread per cell of the (2 snap + 1)^2 window around the seed -> info[8], the smallest key among the window's traversable cells within the snap distance
__global__ void __launch_bounds__(CLR_T)
clr_seed_kernel(const uint8_t* __restrict__ cls, const uint32_t* __restrict__ dist2, int nx, int ny, const Setup S, unsigned long long* __restrict__ info)
{
    const int side = 2 * S.seed_snap + 1;
    const int64_t t = (int64_t)blockIdx.x * CLR_T + threadIdx.x;
    unsigned long long key = KEY_NONE;
    if (t < (int64_t)side * side) {
        const int cx = S.seed_cx - S.seed_snap + (int)(t % side), cy = S.seed_cy - S.seed_snap + (int)(t / side);
        if (cx >= 0 && cy >= 0 && cx < nx && cy < ny) {
            const size_t i = (size_t)cy * nx + cx;
            if (traversable(cls[i], dist2[i], S.free_mask, S.r2)) key = seed_key(cx, cy, nx, S);
        }
    }
    for (int d = 32; d; d >>= 1) { const unsigned long long o = __shfl_down(key, d); key = o < key ? o : key; }
    if ((threadIdx.x & 63) == 0 && key != KEY_NONE) atomicMin(info + 8, key);
}

// ------------------------------------------------------------------ union-find, the parent never above the child (LDS and global alike; as kernels_objects.hip)
__device__ __forceinline__ int clr_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int clr_find(const int* L, int x)
{
    for (int p; (p = clr_load(&L[x])) != x; x = p) {}
    return x;
}
__device__ __forceinline__ void clr_unite(int* L, int a, int b)
{
    for (;;) {
        a = clr_find(L, a); b = clr_find(L, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&L[b], a);
        if (old == b) return;          // b was a root and hangs under a now
        b = old;                       // b had a parent already: that parent and a are to be joined
    }
}
// every tile's forest of its traversable cells; labels[i]: the global index of the tile-local root, -1 on a cell that is not traversable
template <int CONN>
__global__ void __launch_bounds__(CLR_T)
clr_local_kernel(const uint8_t* __restrict__ cls, const uint32_t* __restrict__ dist2, int w, int h, int tiles_x, uint32_t free_mask, long long r2, int32_t* __restrict__ labels)
{
    __shared__ int lab[CLR_PX];
    const int tx0 = (blockIdx.x % tiles_x) * CLR_TW, ty0 = (blockIdx.x / tiles_x) * CLR_TH;
    bool in[CLR_K], fg[CLR_K];
#pragma unroll
    for (int k = 0; k < CLR_K; k++) {
        const int i = threadIdx.x + k * CLR_T, lx = i % CLR_TW, ly = i / CLR_TW, gx = tx0 + lx, gy = ty0 + ly;
        in[k] = gx < w && gy < h;
        fg[k] = false;
        if (in[k]) { const size_t g = (size_t)gy * w + gx; fg[k] = traversable(cls[g], dist2[g], free_mask, (int64_t)r2); }
        lab[i] = fg[k] ? i : -1;
    }
    __syncthreads();
    // (lab[j] >= 0 says "traversable" whatever unions are under way: an entry of a traversable cell never goes negative)
#pragma unroll
    for (int k = 0; k < CLR_K; k++) {
        if (!fg[k]) continue;
        const int i = threadIdx.x + k * CLR_T, lx = i % CLR_TW, ly = i / CLR_TW;
        if (lx > 0 && clr_load(&lab[i - 1]) >= 0) clr_unite(lab, i, i - 1);
        if (ly > 0 && clr_load(&lab[i - CLR_TW]) >= 0) clr_unite(lab, i, i - CLR_TW);
        if (CONN == 8 && ly > 0) {
            if (lx > 0 && clr_load(&lab[i - CLR_TW - 1]) >= 0) clr_unite(lab, i, i - CLR_TW - 1);
            if (lx < CLR_TW - 1 && clr_load(&lab[i - CLR_TW + 1]) >= 0) clr_unite(lab, i, i - CLR_TW + 1);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CLR_K; k++) {
        if (!in[k]) continue;
        const int i = threadIdx.x + k * CLR_T, lx = i % CLR_TW, ly = i / CLR_TW;
        const size_t g = (size_t)(ty0 + ly) * w + tx0 + lx;
        const int r = fg[k] ? clr_find(lab, i) : 0;
        labels[g] = fg[k] ? (ty0 + r / CLR_TW) * w + tx0 + r % CLR_TW : -1;
    }
}
// the rim of every tile: its top row joins the row above, its left column the column to the left (with the diagonals when CONN == 8)
template <int CONN>
__global__ void __launch_bounds__(CLR_T)
clr_merge_kernel(int w, int h, int tiles_x, int32_t* __restrict__ L)
{
    const int tx0 = (blockIdx.x % tiles_x) * CLR_TW, ty0 = (blockIdx.x / tiles_x) * CLR_TH;
    const int tw = min(CLR_TW, w - tx0), th = min(CLR_TH, h - ty0);
    for (int i = threadIdx.x; i < tw + th; i += CLR_T) {
        const bool top = i < tw;
        const int lx = top ? i : 0, ly = top ? 0 : i - tw;
        const int gx = tx0 + lx, gy = ty0 + ly;
        const int a = gy * w + gx;
        if (clr_load(&L[a]) < 0) continue;
        auto F = [&](int q) { return clr_load(&L[q]) >= 0; };          // (q is a cell of the grid: the callers test the borders)
        if (top && gy > 0) {
            const int up = a - w;
            if (F(up)) clr_unite(L, a, up);
            if (CONN == 8) {
                if (gx > 0 && F(up - 1)) clr_unite(L, a, up - 1);
                if (gx + 1 < w && F(up + 1)) clr_unite(L, a, up + 1);
            }
        }
        if (!top && gx > 0) {
            if (F(a - 1)) clr_unite(L, a, a - 1);
            if (CONN == 8) {
                if (gy > 0 && F(a - w - 1)) clr_unite(L, a, a - w - 1);
                if (gy + 1 < h && F(a + w - 1)) clr_unite(L, a, a + w - 1);
            }
        }
    }
}
// the block's sum of v -> *slot: per wave by shuffle, per block through LDS, one atomic per block and none for a sum of 0.  Every thread calls this
__device__ inline void clr_block_add(int v, int* cnt_s, unsigned long long* slot)
{
    for (int d = 32; d; d >>= 1) v += __shfl_down(v, d);
    __syncthreads();                                     // (cnt_s may still be read from the previous call)
    if ((threadIdx.x & 63) == 0) cnt_s[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int k = 0; k < CLR_W; k++) t += cnt_s[k];
        if (t) atomicAdd(slot, (unsigned long long)t);
    }
}
// every cell gets its root as its label; the roots are the components -> info[3].  At most CLR_GRID blocks walk the cells: one atomic per block on one address, and
// thousands of those cost more than the pass itself
__global__ void __launch_bounds__(CLR_T)
clr_flatten_kernel(int64_t nc, int32_t* __restrict__ L, unsigned long long* __restrict__ info)
{
    __shared__ int cnt_s[CLR_W];
    int roots = 0;
    for (int64_t t = (int64_t)blockIdx.x * CLR_T + threadIdx.x; t < nc; t += (int64_t)gridDim.x * CLR_T) {
        const int node = (int)t;
        if (clr_load(&L[node]) < 0) continue;
        const int R = clr_find(L, node);
        if (R == node) roots++;
        else __hip_atomic_store(&L[node], R, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);          // (a chain through this entry reads the old parent or the root: both lead there)
    }
    clr_block_add(roots, cnt_s, info + 3);
}

// ------------------------------------------------------------------ finish
// reach and the counts; labels hold every traversable cell's root by now, so the seed's component is the cells whose label is the seed's.  At most CLR_GRID blocks,
// as in the flatten pass
__global__ void __launch_bounds__(CLR_T)
clr_finish_kernel(const uint8_t* __restrict__ cls, const uint32_t* __restrict__ dist2, const int32_t* __restrict__ labels, int64_t nc, const Setup S, uint8_t* __restrict__ reach,
                  unsigned long long* __restrict__ info)
{
    __shared__ int cnt_s[CLR_W];
    __shared__ uint32_t max_s[CLR_W];
    const unsigned long long key = info[8];              // (written by clr_seed_kernel, an earlier launch; this kernel only reads it)
    const int seed = key == KEY_NONE ? -1 : (int)(key & 0xFFFFFFull);
    const int seed_root = seed >= 0 ? labels[seed] : -1;
    int blocked = 0, free_c = 0, trav = 0, reached = 0; uint32_t far = 0;
    for (int64_t t = (int64_t)blockIdx.x * CLR_T + threadIdx.x; t < nc; t += (int64_t)gridDim.x * CLR_T) {          // (a block's counts stay below 2^31: at most 2^24 cells in all)
        const uint8_t c = cls[t];
        const int l = labels[t];
        const bool tr = l >= 0, re = tr && l == seed_root;
        blocked += in_mask(c, S.blocked_mask); free_c += in_mask(c, S.free_mask); trav += tr; reached += re;
        if (re) far = max(far, dist2[t]);
        reach[t] = (uint8_t)(re ? REACHABLE : tr ? TRAVERSABLE : NOT_TRAVERSABLE);
    }
    clr_block_add(blocked, cnt_s, info + 0);
    clr_block_add(free_c, cnt_s, info + 1);
    clr_block_add(trav, cnt_s, info + 2);
    clr_block_add(reached, cnt_s, info + 4);
    for (int d = 32; d; d >>= 1) far = max(far, (uint32_t)__shfl_down((int)far, d));
    if ((threadIdx.x & 63) == 0) max_s[threadIdx.x >> 6] = far;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t m = 0;
        for (int k = 0; k < CLR_W; k++) m = max(m, max_s[k]);
        if (m) atomicMax(info + 6, (unsigned long long)m);
        if (blockIdx.x == 0) { info[5] = (unsigned long long)(long long)seed; info[7] = (unsigned long long)S.r2; }
    }
}

// ------------------------------------------------------------------ launcher
static inline unsigned clr_blocks(int64_t n) { return (unsigned)((n + CLR_T - 1) / CLR_T); }
size_t k_clearance_mask_words(int nx, int ny) { return (size_t)((ny + CLR_BAND - 1) / CLR_BAND) * (size_t)nx; }
hipError_t k_clearance(const uint8_t* cls, int nx, int ny, const Setup& S, const ClearanceBufs& B, unsigned long long* info, int form, hipStream_t s)
{
    const int64_t nc = (int64_t)nx * ny;
    const int bands = (ny + CLR_BAND - 1) / CLR_BAND, xblocks = (nx + CLR_T - 1) / CLR_T;
    const int tx = (nx + CLR_TW - 1) / CLR_TW, ty = (ny + CLR_TH - 1) / CLR_TH;
    clr_begin_kernel<<<1, 64, 0, s>>>(info);
    clr_mask_kernel<<<clr_blocks((int64_t)bands * nx), CLR_T, 0, s>>>(cls, nx, ny, bands, S.blocked_mask, B.mask);
    clr_column_kernel<<<clr_blocks((int64_t)bands * nx), CLR_T, 0, s>>>(B.mask, nx, ny, bands, B.row);
    if (form == CLEARANCE_FORM_SCAN) clr_row_scan_kernel<<<clr_blocks(nc), CLR_T, 0, s>>>(B.row, nx, nc, B.dist2, B.nearest);
    else clr_row_lds_kernel<<<(unsigned)((int64_t)xblocks * ny), CLR_T, 0, s>>>(B.row, nx, xblocks, B.dist2, B.nearest);
    if (S.seed_cx >= 0) {
        const int side = 2 * S.seed_snap + 1;
        clr_seed_kernel<<<clr_blocks((int64_t)side * side), CLR_T, 0, s>>>(cls, B.dist2, nx, ny, S, info);
    }
    if (S.connectivity == 8) {
        clr_local_kernel<8><<<tx * ty, CLR_T, 0, s>>>(cls, B.dist2, nx, ny, tx, S.free_mask, (long long)S.r2, B.labels);
        clr_merge_kernel<8><<<tx * ty, CLR_T, 0, s>>>(nx, ny, tx, B.labels);
    } else {
        clr_local_kernel<4><<<tx * ty, CLR_T, 0, s>>>(cls, B.dist2, nx, ny, tx, S.free_mask, (long long)S.r2, B.labels);
        clr_merge_kernel<4><<<tx * ty, CLR_T, 0, s>>>(nx, ny, tx, B.labels);
    }
    const unsigned walkers = std::min<unsigned>(clr_blocks(nc), CLR_GRID);
    clr_flatten_kernel<<<walkers, CLR_T, 0, s>>>(nc, B.labels, info);
    clr_finish_kernel<<<walkers, CLR_T, 0, s>>>(cls, B.dist2, B.labels, nc, S, B.reach, info);
    return hipGetLastError();
}
