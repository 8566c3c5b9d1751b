// kernels_objects.hip -- object extraction on the device.  The arithmetic is include/ssm/objects_core.h, which the host functions of
// ssm_objects_host.cpp call too.
//
// Stage 1 labels the member cells of a built grid as kernels_motion_fuse.hip labels pixels: union-find on cell indices in which a parent is never larger than its
// child, so a set's root is its smallest member -- the contract's root.  Two members are joined only when they hold the same label.  (1) every OBJ_TW x OBJ_TH tile
// builds its forest in LDS and writes, per cell, the global index of the tile-local root and the tile-local root itself (loc); (2) the cells on a tile's rim join
// their neighbours in the tile above and to the left with atomicMin on the global labels; (3) every cell follows its chain to the root.  A union ends when an
// atomicMin finds the entry still a root; when it does not, another thread has lowered that entry and the union goes on from the value found, so entries only ever
// decrease and every loop is bounded by the data: no block waits for another, no grid barrier.  An exclusive scan over the cells (rocPRIM) turns roots into
// component indices in ascending root order; the host reads their number and sizes the records.  The figures are pre-reduced per (tile, tile-local root) in LDS,
// then one integer atomic per figure goes onto the component's record; the keep decision, a scan over the components, the compaction and the paint follow.
// Memory: O(cells) integers and O(components) records.
//
// Stage 2: one thread per point over the concatenation of the clouds, found through the cloud-segment table (cloud_table.h) exactly as the grid's passes find it.
// Integer add / min / max atomics onto the object's record -- form 0 one per point and figure; form 1 one per run of adjacent lanes with the same object, the min /
// max atomics skipped where a plain load shows they cannot change anything (a figure only ever moves one way during the kernel, so a stale value can only cause a
// superfluous atomic).  The same bits either way.
#include "ssm_internal.h"
#include "../../include/ssm/objects_core.h"
#include <cstring>          // (for rocPRIM: its texture_cache_iterator.hpp calls memset and includes no header that declares it)
#include <rocprim/rocprim.hpp>
using namespace ssm_objc;

#define OBJ_TW 32
#define OBJ_TH 32
#define OBJ_PX (OBJ_TW * OBJ_TH)
#define OBJ_T 256
#define OBJ_K (OBJ_PX / OBJ_T)
#define OBJ_W (OBJ_T / 64)
int k_objects_tile_w() { return OBJ_TW; }
int k_objects_tile_h() { return OBJ_TH; }
int k_objects_block() { return OBJ_T; }
static_assert(OBJ_PX % OBJ_T == 0 && OBJ_T % OBJ_TW == 0 && OBJ_PX <= 65536, "whole rows of a tile per pass of the block; a tile-local index fits 16 bits");
static_assert(sizeof(ssm_object) == 104, "a record is 104 bytes");
// A probe build (-DOBJECTS_PROBE: scripts/objects_probe.hip, never the library) counts the atomics stage 2 issues
#ifdef OBJECTS_PROBE
__device__ unsigned long long objects_probe_count;
#define OBJ_COUNT() atomicAdd(&objects_probe_count, 1ull)
#else
#define OBJ_COUNT()
#endif

// ------------------------------------------------------------------ union-find, the parent never above the child (LDS and global alike; as kernels_motion_fuse.hip)
__device__ __forceinline__ int obj_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int obj_find(const int* L, int x)
{
    for (int p; (p = obj_load(&L[x])) != x; x = p) {}
    return x;
}
__device__ __forceinline__ void obj_unite(int* L, int a, int b)
{
    for (;;) {
        a = obj_find(L, a); b = obj_find(L, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&L[b], a);
        if (old == b) return;          // b was a root and hangs under a now
        b = old;                       // b had a parent already: that parent and a are to be joined
    }
}

// ------------------------------------------------------------------ stage 1
// info: the eight 64-bit counts of ssm_objects_info; isroot[nc] = 0 closes the scan's input
__global__ void __launch_bounds__(OBJ_T)
obj_begin_kernel(unsigned long long* __restrict__ info, int32_t* __restrict__ isroot, int64_t nc)
{
    if (threadIdx.x < 8) info[threadIdx.x] = 0ull;
    if (threadIdx.x == 8) isroot[nc] = 0;
}
// mem[i]: the cell's label when it is a member, 255 otherwise.  A member never goes negative in lab, so `same` reads the same whatever unions are under way
template <int CONN>
__global__ void __launch_bounds__(OBJ_T)
obj_local_kernel(const ObjectsCells G, uint32_t label_mask, int tiles_x, int32_t* __restrict__ labels, uint16_t* __restrict__ loc, unsigned long long* __restrict__ info)
{
    __shared__ int lab[OBJ_PX];
    __shared__ uint8_t mem[OBJ_PX];
    __shared__ int cnt_s[OBJ_W];
    const int tx0 = (blockIdx.x % tiles_x) * OBJ_TW, ty0 = (blockIdx.x / tiles_x) * OBJ_TH;
    const int w = G.nx, h = G.ny;
    bool in[OBJ_K], fg[OBJ_K];
    int members = 0;
#pragma unroll
    for (int k = 0; k < OBJ_K; k++) {
        const int i = threadIdx.x + k * OBJ_T, lx = i % OBJ_TW, ly = i / OBJ_TW, gx = tx0 + lx, gy = ty0 + ly;
        in[k] = gx < w && gy < h;
        uint8_t l = 255;
        if (in[k]) { const size_t g = (size_t)gy * w + gx; const uint8_t ol = G.obstacle_label[g]; if (member(G.cls[g], ol, label_mask)) l = ol; }
        fg[k] = l != 255;
        members += fg[k];
        mem[i] = l; lab[i] = fg[k] ? i : -1;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < OBJ_K; k++) {
        if (!fg[k]) continue;
        const int i = threadIdx.x + k * OBJ_T, lx = i % OBJ_TW, ly = i / OBJ_TW;
        const uint8_t l = mem[i];
        if (lx > 0 && mem[i - 1] == l) obj_unite(lab, i, i - 1);
        if (ly > 0 && mem[i - OBJ_TW] == l) obj_unite(lab, i, i - OBJ_TW);
        if (CONN == 8 && ly > 0) {
            if (lx > 0 && mem[i - OBJ_TW - 1] == l) obj_unite(lab, i, i - OBJ_TW - 1);
            if (lx < OBJ_TW - 1 && mem[i - OBJ_TW + 1] == l) obj_unite(lab, i, i - OBJ_TW + 1);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < OBJ_K; k++) {
        if (!in[k]) continue;
        const int i = threadIdx.x + k * OBJ_T, lx = i % OBJ_TW, ly = i / OBJ_TW;
        const size_t g = (size_t)(ty0 + ly) * w + tx0 + lx;
        const int r = fg[k] ? obj_find(lab, i) : 0;
        labels[g] = fg[k] ? (ty0 + r / OBJ_TW) * w + tx0 + r % OBJ_TW : -1;
        loc[g] = (uint16_t)r;
    }
    // the member cells: per wave by shuffle, per block through LDS, one atomic per block and none for a count of 0
    for (int d = 32; d; d >>= 1) members += __shfl_down(members, d);
    if ((threadIdx.x & 63) == 0) cnt_s[threadIdx.x >> 6] = members;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int v = 0; v < OBJ_W; v++) t += cnt_s[v];
        if (t) atomicAdd(info + 0, (unsigned long long)t);
    }
}
// the rim of every tile: its top row joins the row above, its left column the column to the left (with the diagonals when CONN == 8) -- where the labels agree
template <int CONN>
__global__ void __launch_bounds__(OBJ_T)
obj_merge_kernel(const uint8_t* __restrict__ ol, int w, int h, int tiles_x, int32_t* __restrict__ L)
{
    const int tx0 = (blockIdx.x % tiles_x) * OBJ_TW, ty0 = (blockIdx.x / tiles_x) * OBJ_TH;
    const int tw = min(OBJ_TW, w - tx0), th = min(OBJ_TH, h - ty0);
    for (int i = threadIdx.x; i < tw + th; i += OBJ_T) {
        const bool top = i < tw;
        const int lx = top ? i : 0, ly = top ? 0 : i - tw;
        const int gx = tx0 + lx, gy = ty0 + ly;
        const int a = gy * w + gx;
        if (obj_load(&L[a]) < 0) continue;
        const uint8_t l = ol[a];
        auto F = [&](int q) { return obj_load(&L[q]) >= 0 && ol[q] == l; };          // (q is a cell of the grid: the callers test the borders)
        if (top && gy > 0) {
            const int up = a - w;
            if (F(up)) obj_unite(L, a, up);
            if (CONN == 8) {
                if (gx > 0 && F(up - 1)) obj_unite(L, a, up - 1);
                if (gx + 1 < w && F(up + 1)) obj_unite(L, a, up + 1);
            }
        }
        if (!top && gx > 0) {
            if (F(a - 1)) obj_unite(L, a, a - 1);
            if (CONN == 8) {
                if (gy > 0 && F(a - w - 1)) obj_unite(L, a, a - w - 1);
                if (gy + 1 < h && F(a + w - 1)) obj_unite(L, a, a + w - 1);
            }
        }
    }
}
// every cell gets its root as its label; isroot: the scan's input
__global__ void __launch_bounds__(OBJ_T)
obj_flatten_kernel(int64_t nc, int32_t* __restrict__ L, int32_t* __restrict__ isroot)
{
    const int64_t t = (int64_t)blockIdx.x * OBJ_T + threadIdx.x;
    if (t >= nc) return;
    const int node = (int)t;
    const int v = obj_load(&L[node]);
    int root = 0;
    if (v >= 0) {
        const int R = obj_find(L, node);
        root = R == node;
        if (!root) __hip_atomic_store(&L[node], R, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);          // (a chain through this entry reads the old parent or the root: both lead there)
    }
    isroot[node] = root;
}
__global__ void __launch_bounds__(OBJ_T)
obj_clear_records_kernel(ssm_object* __restrict__ comp, int32_t C, int32_t* __restrict__ keep)
{
    const int i = blockIdx.x * OBJ_T + threadIdx.x;
    if (i > C) return;
    if (i == C) { keep[C] = 0; return; }
    ssm_object o; clear_cells(&o); clear_points(&o);
    comp[i] = o;
}
// The figures of every tile's part of every component, reduced in LDS at the tile-local root, then one atomic per figure and (tile, tile-local root) onto the
// component's record; the cell that is the component's root names it
__global__ void __launch_bounds__(OBJ_T)
obj_figures_kernel(const ObjectsCells G, int tiles_x, const int32_t* __restrict__ labels, const uint16_t* __restrict__ loc, const int32_t* __restrict__ rank,
                   ssm_object* __restrict__ comp)
{
    __shared__ uint32_t cnt[OBJ_PX], pts[OBJ_PX];
    __shared__ int xlo[OBJ_PX], xhi[OBJ_PX], ylo[OBJ_PX], yhi[OBJ_PX], glo[OBJ_PX], thi[OBJ_PX];
    const int tx0 = (blockIdx.x % tiles_x) * OBJ_TW, ty0 = (blockIdx.x / tiles_x) * OBJ_TH;
    const int w = G.nx, h = G.ny;
#pragma unroll
    for (int k = 0; k < OBJ_K; k++) {
        const int i = threadIdx.x + k * OBJ_T;
        cnt[i] = 0; pts[i] = 0; xlo[i] = ylo[i] = glo[i] = INT32_MAX; xhi[i] = yhi[i] = thi[i] = INT32_MIN;
    }
    __syncthreads();
    int R[OBJ_K];
#pragma unroll
    for (int k = 0; k < OBJ_K; k++) {
        const int i = threadIdx.x + k * OBJ_T, lx = i % OBJ_TW, ly = i / OBJ_TW, gx = tx0 + lx, gy = ty0 + ly;
        R[k] = -1;
        if (!(gx < w && gy < h)) continue;
        const size_t g = (size_t)gy * w + gx;
        R[k] = labels[g];
        if (R[k] < 0) continue;
        const int r = loc[g];
        atomicAdd(&cnt[r], 1u); atomicAdd(&pts[r], G.n_high[g]);          // (a grid holds fewer than 2^31 points, and ssm_debug_objects_cells refuses more: a tile's sum fits)
        atomicMin(&xlo[r], gx); atomicMax(&xhi[r], gx); atomicMin(&ylo[r], gy); atomicMax(&yhi[r], gy);
        atomicMin(&glo[r], G.ground_q[g]); atomicMax(&thi[r], G.top_q[g]);
        if (R[k] == (int)g) { ssm_object* o = comp + rank[g]; o->root = (int32_t)g; o->label = G.obstacle_label[g]; }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < OBJ_K; k++) {
        const int i = threadIdx.x + k * OBJ_T;
        if (R[k] < 0 || cnt[i] == 0) continue;                               // (cnt[i] > 0: i is a tile-local root, and R[k] its component's)
        ssm_object* o = comp + rank[R[k]];
        atomicAdd(&o->cells, cnt[i]); atomicAdd(reinterpret_cast<unsigned long long*>(&o->cell_points), (unsigned long long)pts[i]);
        atomicMin(&o->cx_min, xlo[i]); atomicMax(&o->cx_max, xhi[i]); atomicMin(&o->cy_min, ylo[i]); atomicMax(&o->cy_max, yhi[i]);
        atomicMin(&o->ground_q, glo[i]); atomicMax(&o->top_q, thi[i]);
    }
}
// keep[c]: is component c an object; the rejected ones counted per wave by ballot -> info[3 .. 5]; info[1] = C
__global__ void __launch_bounds__(OBJ_T)
obj_keep_kernel(const ssm_object* __restrict__ comp, int32_t C, const Setup S, int32_t* __restrict__ keep, unsigned long long* __restrict__ info)
{
    const int i = blockIdx.x * OBJ_T + threadIdx.x;
    int v = -1;
    if (i < C) { const ssm_object o = comp[i]; v = verdict_of(o.cells, o.cell_points, o.ground_q, o.top_q, S); keep[i] = v == KEPT; }
    const int c1 = __popcll(__ballot(v == REJECT_CELLS)), c2 = __popcll(__ballot(v == REJECT_POINTS)), c3 = __popcll(__ballot(v == REJECT_HEIGHT));
    if ((threadIdx.x & 63) == 0) {
        if (c1) atomicAdd(info + 3, (unsigned long long)c1);
        if (c2) atomicAdd(info + 4, (unsigned long long)c2);
        if (c3) atomicAdd(info + 5, (unsigned long long)c3);
    }
    if (i == 0) info[1] = (unsigned long long)C;
}
// the kept records, in ascending root order; info[2] = K
__global__ void __launch_bounds__(OBJ_T)
obj_compact_kernel(const ssm_object* __restrict__ comp, int32_t C, const int32_t* __restrict__ keep, const int32_t* __restrict__ kid, ssm_object* __restrict__ objs,
                   unsigned long long* __restrict__ info)
{
    const int i = blockIdx.x * OBJ_T + threadIdx.x;
    if (i < C && keep[i]) objs[kid[i]] = comp[i];
    if (i == 0) info[2] = (unsigned long long)kid[C];
}
// C == 0: keep and kid are not read
__global__ void __launch_bounds__(OBJ_T)
obj_paint_kernel(int64_t nc, const int32_t* __restrict__ labels, const int32_t* __restrict__ rank, const int32_t* __restrict__ keep, const int32_t* __restrict__ kid,
                 int32_t* __restrict__ object_id)
{
    const int64_t t = (int64_t)blockIdx.x * OBJ_T + threadIdx.x;
    if (t >= nc) return;
    const int R = labels[t];
    int id = -1;
    if (R >= 0) { const int c = rank[R]; if (keep[c]) id = kid[c]; }
    object_id[t] = id;
}

// ------------------------------------------------------------------ stage 2
__global__ void __launch_bounds__(OBJ_T)
obj_points_begin_kernel(ssm_object* __restrict__ objs, int32_t K, unsigned long long* __restrict__ info, int64_t n_in)
{
    const int i = blockIdx.x * OBJ_T + threadIdx.x;
    if (i < K) clear_points(objs + i);
    if (i == 0) { info[6] = (unsigned long long)n_in; info[7] = 0ull; }
}
// the point g of the call -> its object (-1: none, or there is no such point), its quantised coordinates, does its label agree
__device__ inline int obj_point(const ssm_gridc::Setup& G, const CloudSeg* __restrict__ seg, const int32_t* __restrict__ blk, int64_t total,
                                const ssm_grid_cell* __restrict__ cells, const int32_t* __restrict__ object_id, const ssm_object* __restrict__ objs, int32_t* __restrict__ point_ids,
                                Hit* h, bool* agrees)
{
    const int64_t g = (int64_t)blockIdx.x * OBJ_T + threadIdx.x;
    const int k0 = blk[blockIdx.x];
    const bool uniform = cloud_block_uniform<int64_t>(seg, k0, (int64_t)blockIdx.x * OBJ_T, OBJ_T, total);
    *agrees = false;
    if (g >= total) return -1;
    const int k = cloud_of<int64_t>(seg, k0, uniform, g);
    const ssm_point* p = seg[k].pts + (g - seg[k].off);
    int id = -1;
    if (point_of(p->x, p->y, p->z, seg[k].M, G, h) == ssm_gridc::P_USED && !ssm_gridc::is_low(h->hq, cells[h->cell].base, G.step_q)) id = object_id[h->cell];
    if (id >= 0) *agrees = p->label == (uint32_t)objs[id].label;
    point_ids[g] = id;
    return id;
}
// the object points of the block -> info[7]: per wave by ballot, per block through LDS, one atomic per block and none for a count of 0.  Every thread calls this
__device__ inline void obj_count_points(int id, unsigned long long* __restrict__ info)
{
    __shared__ int cnt_s[OBJ_W];
    const int c = __popcll(__ballot(id >= 0));
    if ((threadIdx.x & 63) == 0) cnt_s[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int v = 0; v < OBJ_W; v++) t += cnt_s[v];
        if (t) atomicAdd(info + 7, (unsigned long long)t);
    }
}
__global__ void __launch_bounds__(OBJ_T)
obj_points_kernel(const ssm_gridc::Setup G, const CloudSeg* __restrict__ seg, const int32_t* __restrict__ blk, int64_t total, const ssm_grid_cell* __restrict__ cells,
                  const int32_t* __restrict__ object_id, ssm_object* __restrict__ objs, int32_t* __restrict__ point_ids, unsigned long long* __restrict__ info)
{
    Hit h; bool agrees;
    const int id = obj_point(G, seg, blk, total, cells, object_id, objs, point_ids, &h, &agrees);
    if (id >= 0) {
        ssm_object* o = objs + id;
        OBJ_COUNT(); atomicAdd(&o->n_points, 1u);
        if (agrees) { OBJ_COUNT(); atomicAdd(&o->n_label, 1u); }
        OBJ_COUNT(); atomicMin(&o->x_min_q, h.xq); OBJ_COUNT(); atomicMax(&o->x_max_q, h.xq);
        OBJ_COUNT(); atomicMin(&o->y_min_q, h.yq); OBJ_COUNT(); atomicMax(&o->y_max_q, h.yq);
        OBJ_COUNT(); atomicMin(&o->z_min_q, h.zq); OBJ_COUNT(); atomicMax(&o->z_max_q, h.zq);
        OBJ_COUNT(); atomicAdd(reinterpret_cast<unsigned long long*>(&o->sum_x), (unsigned long long)(long long)h.xq);
        OBJ_COUNT(); atomicAdd(reinterpret_cast<unsigned long long*>(&o->sum_y), (unsigned long long)(long long)h.yq);
        OBJ_COUNT(); atomicAdd(reinterpret_cast<unsigned long long*>(&o->sum_z), (unsigned long long)(long long)h.zq);
    }
    obj_count_points(id, info);
}
// A RUN is a maximal stretch of adjacent lanes with one object (kernels_grid.hip grid_run_end); its first lane issues the run's atomics with the run's counts,
// minima, maxima and sums.  Integer terms: the same bits as one atomic per point
__device__ inline int obj_run_end(int key, int lane, bool* head)
{
    const int prev = __shfl_up(key, 1);
    *head = lane == 0 || key != prev;
    const unsigned long long heads = __ballot(*head);
    const unsigned long long behind = lane == 63 ? 0ull : heads >> (lane + 1);
    return behind ? lane + 1 + __ffsll((long long)behind) - 1 : 64;
}
__global__ void __launch_bounds__(OBJ_T)
obj_points_runs_kernel(const ssm_gridc::Setup G, const CloudSeg* __restrict__ seg, const int32_t* __restrict__ blk, int64_t total, const ssm_grid_cell* __restrict__ cells,
                       const int32_t* __restrict__ object_id, ssm_object* __restrict__ objs, int32_t* __restrict__ point_ids, unsigned long long* __restrict__ info)
{
    const int lane = threadIdx.x & 63;
    Hit h; bool agrees;
    const int id = obj_point(G, seg, blk, total, cells, object_id, objs, point_ids, &h, &agrees);
    bool head;
    const int end = obj_run_end(id, lane, &head);
    const bool on = id >= 0;
    int nl = agrees ? 1 : 0;
    int xlo = on ? h.xq : INT32_MAX, xhi = on ? h.xq : INT32_MIN, ylo = on ? h.yq : INT32_MAX, yhi = on ? h.yq : INT32_MIN, zlo = on ? h.zq : INT32_MAX, zhi = on ? h.zq : INT32_MIN;
    long long sx = on ? h.xq : 0, sy = on ? h.yq : 0, sz = on ? h.zq : 0;
    for (int d = 1; d < 64; d <<= 1) {                                // after the step with d a lane holds its run's [lane, lane + 2 d) part
        const int a0 = __shfl_down(nl, d), a1 = __shfl_down(xlo, d), a2 = __shfl_down(xhi, d), a3 = __shfl_down(ylo, d), a4 = __shfl_down(yhi, d), a5 = __shfl_down(zlo, d),
                  a6 = __shfl_down(zhi, d);
        const long long b0 = __shfl_down(sx, d), b1 = __shfl_down(sy, d), b2 = __shfl_down(sz, d);
        if (lane + d < end) {
            nl += a0; xlo = min(xlo, a1); xhi = max(xhi, a2); ylo = min(ylo, a3); yhi = max(yhi, a4); zlo = min(zlo, a5); zhi = max(zhi, a6);
            sx += b0; sy += b1; sz += b2;
        }
    }
    if (head && on) {
        ssm_object* o = objs + id;
        OBJ_COUNT(); atomicAdd(&o->n_points, (uint32_t)(end - lane));
        if (nl) { OBJ_COUNT(); atomicAdd(&o->n_label, (uint32_t)nl); }
        if (xlo < o->x_min_q) { OBJ_COUNT(); atomicMin(&o->x_min_q, xlo); }
        if (xhi > o->x_max_q) { OBJ_COUNT(); atomicMax(&o->x_max_q, xhi); }
        if (ylo < o->y_min_q) { OBJ_COUNT(); atomicMin(&o->y_min_q, ylo); }
        if (yhi > o->y_max_q) { OBJ_COUNT(); atomicMax(&o->y_max_q, yhi); }
        if (zlo < o->z_min_q) { OBJ_COUNT(); atomicMin(&o->z_min_q, zlo); }
        if (zhi > o->z_max_q) { OBJ_COUNT(); atomicMax(&o->z_max_q, zhi); }
        OBJ_COUNT(); atomicAdd(reinterpret_cast<unsigned long long*>(&o->sum_x), (unsigned long long)sx);
        OBJ_COUNT(); atomicAdd(reinterpret_cast<unsigned long long*>(&o->sum_y), (unsigned long long)sy);
        OBJ_COUNT(); atomicAdd(reinterpret_cast<unsigned long long*>(&o->sum_z), (unsigned long long)sz);
    }
    obj_count_points(id, info);
}

// ------------------------------------------------------------------ launchers
static inline unsigned obj_blocks(int64_t n) { return (unsigned)((n + OBJ_T - 1) / OBJ_T); }
size_t k_objects_tmp_bytes(int64_t nc)
{
    size_t b = 0;
    (void)rocprim::exclusive_scan(nullptr, b, (const int32_t*)nullptr, (int32_t*)nullptr, (int32_t)0, (size_t)nc + 1, rocprim::plus<int32_t>(), (hipStream_t)0);
    return b ? b : 1;
}
hipError_t k_objects_label(const ObjectsCells& G, const Setup& S, const ObjectsBufs& B, unsigned long long* info, hipStream_t s)
{
    const int64_t nc = (int64_t)G.nx * G.ny;
    const int tx = (G.nx + OBJ_TW - 1) / OBJ_TW, ty = (G.ny + OBJ_TH - 1) / OBJ_TH;
    obj_begin_kernel<<<1, OBJ_T, 0, s>>>(info, B.isroot, nc);
    if (S.connectivity == 8) {
        obj_local_kernel<8><<<tx * ty, OBJ_T, 0, s>>>(G, S.label_mask, tx, B.labels, B.loc, info);
        obj_merge_kernel<8><<<tx * ty, OBJ_T, 0, s>>>(G.obstacle_label, G.nx, G.ny, tx, B.labels);
    } else {
        obj_local_kernel<4><<<tx * ty, OBJ_T, 0, s>>>(G, S.label_mask, tx, B.labels, B.loc, info);
        obj_merge_kernel<4><<<tx * ty, OBJ_T, 0, s>>>(G.obstacle_label, G.nx, G.ny, tx, B.labels);
    }
    obj_flatten_kernel<<<obj_blocks(nc), OBJ_T, 0, s>>>(nc, B.labels, B.isroot);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t bytes = B.tmp_bytes;
    return rocprim::exclusive_scan(B.tmp, bytes, B.isroot, B.rank, (int32_t)0, (size_t)nc + 1, rocprim::plus<int32_t>(), s);
}
hipError_t k_objects_records(const ObjectsCells& G, const Setup& S, const ObjectsBufs& B, int32_t C, ssm_object* comp, int32_t* keep, int32_t* kid, ssm_object* objs,
                             unsigned long long* info, hipStream_t s)
{
    const int64_t nc = (int64_t)G.nx * G.ny;
    const int tx = (G.nx + OBJ_TW - 1) / OBJ_TW, ty = (G.ny + OBJ_TH - 1) / OBJ_TH;
    if (C > 0) {
        obj_clear_records_kernel<<<obj_blocks((int64_t)C + 1), OBJ_T, 0, s>>>(comp, C, keep);
        obj_figures_kernel<<<tx * ty, OBJ_T, 0, s>>>(G, tx, B.labels, B.loc, B.rank, comp);
        obj_keep_kernel<<<obj_blocks(C), OBJ_T, 0, s>>>(comp, C, S, keep, info);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        size_t bytes = B.tmp_bytes;
        e = rocprim::exclusive_scan(B.tmp, bytes, keep, kid, (int32_t)0, (size_t)C + 1, rocprim::plus<int32_t>(), s);
        if (e != hipSuccess) return e;
        obj_compact_kernel<<<obj_blocks(C), OBJ_T, 0, s>>>(comp, C, keep, kid, objs, info);
    }
    obj_paint_kernel<<<obj_blocks(nc), OBJ_T, 0, s>>>(nc, B.labels, B.rank, keep, kid, B.object_id);
    return hipGetLastError();
}
hipError_t k_objects_points(const ssm_gridc::Setup& G, const CloudSeg* seg, const int32_t* blk, int64_t total, const ssm_grid_cell* cells, const int32_t* object_id,
                            ssm_object* objs, int32_t K, int32_t* point_ids, unsigned long long* info, int form, hipStream_t s)
{
    obj_points_begin_kernel<<<obj_blocks(K > 0 ? K : 1), OBJ_T, 0, s>>>(objs, K, info, total);
    if (total > 0) {
        if (form == OBJECTS_FORM_RUNS) obj_points_runs_kernel<<<obj_blocks(total), OBJ_T, 0, s>>>(G, seg, blk, total, cells, object_id, objs, point_ids, info);
        else obj_points_kernel<<<obj_blocks(total), OBJ_T, 0, s>>>(G, seg, blk, total, cells, object_id, objs, point_ids, info);
    }
    return hipGetLastError();
}
