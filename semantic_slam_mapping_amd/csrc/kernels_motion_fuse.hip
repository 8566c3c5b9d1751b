// kernels_motion_fuse.hip -- the semantic-motion fusion for n device frames: the class images, connected-component labelling of a full frame, the
// per-blob figures and the decision.  The arithmetic is include/ssm/motion_fuse_core.h, which the host function of ssm_motion_fuse_host.cpp calls too.
//
// Labelling is union-find on pixel indices in which a parent is never larger than its child, so a set's root is its smallest member -- the contract's label.
// It runs twice: on the zero pixels of `cand`, 4-connected, with node 0 standing for everything outside the image (a pixel is node index + 1); then on `filled`,
// 8-connected.  Three kernels each time: (1) every MF_TW x MF_TH tile builds its forest in LDS and writes, per pixel, the global index of the tile-local root;
// (2) the pixels on a tile's rim join their neighbours in the next tile -- and, in the first run, the image border joins node 0 -- with atomicMin on the
// global labels; (3) every pixel follows its chain to the root.  A union ends when an atomicMin finds the entry still a root; when it does not, another thread
// has lowered that entry and the union goes on from the value found, so entries only ever decrease and every loop is bounded by the data: no block waits for
// another.  Loads that see an older value of an entry see a former ancestor of the same set, which the atomic then corrects; the result -- one root per set, its
// smallest member -- does not depend on the order.  Counters are integers: per (tile, tile-local root) in LDS, then one atomic per such pair onto the root.
#include "ssm_internal.h"
#include "../../include/ssm/motion_fuse_core.h"
using namespace ssm_mfc;

#define MF_TW TILE_W
#define MF_TH TILE_H
#define MF_PX (MF_TW * MF_TH)
#define MF_T 256
#define MF_K (MF_PX / MF_T)
int k_mf_tile_w() { return MF_TW; }
int k_mf_tile_h() { return MF_TH; }

// ------------------------------------------------------------------ `always` and `cand`: the class bits, dilated by the 5 x 5 box (separable OR, as mask_kernel)
__global__ void __launch_bounds__(MF_T)
mf_class_kernel(const uint8_t* __restrict__ sem, int w, int h, int tiles_x, uint8_t* __restrict__ always, uint8_t* __restrict__ cand)
{
    __shared__ uint8_t m0[MF_TH + 4][MF_TW + 4];
    __shared__ uint8_t m1[MF_TH + 4][MF_TW];
    const int tx0 = (blockIdx.x % tiles_x) * MF_TW, ty0 = (blockIdx.x / tiles_x) * MF_TH;
    const uint8_t* s = sem + (size_t)blockIdx.y * w * h * 3;
    for (int i = threadIdx.x; i < (MF_TH + 4) * (MF_TW + 4); i += MF_T) {
        const int ly = i / (MF_TW + 4), lx = i - ly * (MF_TW + 4);
        const int gx = tx0 + lx - 2, gy = ty0 + ly - 2;
        uint8_t v = 0;
        if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
            const uint8_t* p = s + ((size_t)gy * w + gx) * 3;
            v = (uint8_t)class_bits(p[0], p[1], p[2]);
        }
        m0[ly][lx] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (MF_TH + 4) * MF_TW; i += MF_T) {
        const int ly = i / MF_TW, lx = i - ly * MF_TW;
        const uint8_t* p = &m0[ly][lx];
        m1[ly][lx] = p[0] | p[1] | p[2] | p[3] | p[4];
    }
    __syncthreads();
    const size_t base = (size_t)blockIdx.y * w * h;
    const int lx = threadIdx.x % MF_TW;
    for (int ly = threadIdx.x / MF_TW; ly < MF_TH; ly += MF_T / MF_TW) {
        const int gx = tx0 + lx, gy = ty0 + ly;
        if (gx < w && gy < h) {
            const int o = m1[ly][lx] | m1[ly + 1][lx] | m1[ly + 2][lx] | m1[ly + 3][lx] | m1[ly + 4][lx];
            always[base + (size_t)gy * w + gx] = (o & CLASS_ALWAYS) ? 255 : 0;
            cand[base + (size_t)gy * w + gx] = (o & CLASS_CAND) ? 255 : 0;
        }
    }
}

// ------------------------------------------------------------------ union-find, the parent never above the child (LDS and global alike)
__device__ __forceinline__ int mf_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int mf_find(const int* L, int x)
{
    for (int p; (p = mf_load(&L[x])) != x; x = p) {}
    return x;
}
__device__ __forceinline__ void mf_unite(int* L, int a, int b)
{
    for (;;) {
        a = mf_find(L, a); b = mf_find(L, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&L[b], a);
        if (old == b) return;          // b was a root and hangs under a now
        b = old;                       // b had a parent already (which the smaller of the two replaced or not): that parent and a are to be joined
    }
}

// OUT: foreground = the zero pixels of img, a pixel is node index + 1 and node 0 is the outside; otherwise foreground = the set pixels, node = index, and the
// tile's figures are collected: area / overlap get, at the pixel of every tile-local root, the pixels of its set in this tile / those under motion == 255
template <int CONN, bool OUT>
__global__ void __launch_bounds__(MF_T)
mf_local_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ motion, int w, int h, int tiles_x, size_t lstride, int32_t* __restrict__ labels,
                int32_t* __restrict__ area, int32_t* __restrict__ overlap)
{
    __shared__ int lab[MF_PX];
    __shared__ int cnt[OUT ? 1 : MF_PX], ov[OUT ? 1 : MF_PX];
    const int tx0 = (blockIdx.x % tiles_x) * MF_TW, ty0 = (blockIdx.x / tiles_x) * MF_TH, f = blockIdx.y;
    const size_t px = (size_t)w * h, base = (size_t)f * px;
    int32_t* L = labels + (size_t)f * lstride;
    const int OFF = OUT ? 1 : 0;
    bool in[MF_K], fg[MF_K];
#pragma unroll
    for (int k = 0; k < MF_K; k++) {
        const int i = threadIdx.x + k * MF_T, lx = i % MF_TW, ly = i / MF_TW, gx = tx0 + lx, gy = ty0 + ly;
        in[k] = gx < w && gy < h;
        fg[k] = in[k] && ((img[base + (size_t)gy * w + gx] == 0) == OUT);
        lab[i] = fg[k] ? i : -1;
        if (!OUT) { cnt[i] = 0; ov[i] = 0; }
    }
    if (OUT && blockIdx.x == 0 && threadIdx.x == 0) L[0] = 0;
    __syncthreads();
    // a foreground entry never goes negative, so `>= 0` reads the same whatever unions are under way.  A union is left out where the two pixels are joined
    // through neighbours whose own unions are made anyway (L, U, UL, UR: left, up and the upper diagonals): i - U when i - L, L - UL and UL - U exist; a diagonal
    // when U, or L for the left one, bridges it.  In a uniform region that is one union per pixel instead of two (four)
#pragma unroll
    for (int k = 0; k < MF_K; k++) {
        if (!fg[k]) continue;
        const int i = threadIdx.x + k * MF_T, lx = i % MF_TW, ly = i / MF_TW;
        const bool fL = lx > 0 && mf_load(&lab[i - 1]) >= 0, fU = ly > 0 && mf_load(&lab[i - MF_TW]) >= 0;
        const bool fUL = lx > 0 && ly > 0 && mf_load(&lab[i - MF_TW - 1]) >= 0;
        if (fL) mf_unite(lab, i, i - 1);
        if (fU && !(fL && fUL)) mf_unite(lab, i, i - MF_TW);
        if (CONN == 8 && !fU && ly > 0) {
            if (fUL && !fL) mf_unite(lab, i, i - MF_TW - 1);
            if (lx < MF_TW - 1 && mf_load(&lab[i - MF_TW + 1]) >= 0) mf_unite(lab, i, i - MF_TW + 1);
        }
    }
    __syncthreads();
    int root[MF_K];
#pragma unroll
    for (int k = 0; k < MF_K; k++) {
        root[k] = -1;
        if (!fg[k]) continue;
        const int i = threadIdx.x + k * MF_T, lx = i % MF_TW, ly = i / MF_TW;
        root[k] = mf_find(lab, i);
        if (!OUT) {
            atomicAdd(&cnt[root[k]], 1);
            if (motion && motion_hit(motion[base + (size_t)(ty0 + ly) * w + tx0 + lx])) atomicAdd(&ov[root[k]], 1);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < MF_K; k++) {
        if (!in[k]) continue;
        const int i = threadIdx.x + k * MF_T, lx = i % MF_TW, ly = i / MF_TW;
        const size_t g = (size_t)(ty0 + ly) * w + tx0 + lx;
        L[g + OFF] = fg[k] ? (ty0 + root[k] / MF_TW) * w + tx0 + root[k] % MF_TW + OFF : -1;
        if (!OUT) { const bool r = fg[k] && root[k] == i; area[base + g] = r ? cnt[i] : 0; overlap[base + g] = r ? ov[i] : 0; }
    }
}

// the rim of every tile: its top row joins the row above, its left column the column to the left (with the diagonals when CONN == 8); OUT: what lies on the
// image border joins node 0.  Items: the top row, the left column, then (OUT) the bottom row and the right column of the tile's part of the image
template <int CONN, bool OUT>
__global__ void __launch_bounds__(MF_T)
mf_merge_kernel(int w, int h, int tiles_x, size_t lstride, int32_t* __restrict__ labels)
{
    const int tx0 = (blockIdx.x % tiles_x) * MF_TW, ty0 = (blockIdx.x / tiles_x) * MF_TH, f = blockIdx.y;
    const int tw = min(MF_TW, w - tx0), th = min(MF_TH, h - ty0);
    int32_t* L = labels + (size_t)f * lstride + (OUT ? 1 : 0);          // L[pixel]; node 0 of an OUT run is L[-1]
    int32_t* N = labels + (size_t)f * lstride;                          // N[node]
    const int OFF = OUT ? 1 : 0;
    const int items = OUT ? 2 * (tw + th) : tw + th;
    for (int i = threadIdx.x; i < items; i += MF_T) {
        int lx, ly, kind;
        if (i < tw) { kind = 0; lx = i; ly = 0; }
        else if (i < tw + th) { kind = 1; lx = 0; ly = i - tw; }
        else if (i < 2 * tw + th) { kind = 2; lx = i - tw - th; ly = th - 1; }
        else { kind = 3; lx = tw - 1; ly = i - 2 * tw - th; }
        const int gx = tx0 + lx, gy = ty0 + ly;
        const int a = gy * w + gx;
        if (mf_load(&L[a]) < 0) continue;
        auto F = [&](int q) { return mf_load(&L[q]) >= 0; };
        // as in the tile: a union over the seam is left out where the pair is joined through the previous pixel of the same rim (same tile, so joined to this
        // one already) and ITS union over the seam -- never at the rim's first pixel, so the argument ends there and stays inside one pair of tiles
        if (kind == 0 && gy > 0) {
            const int up = a - w;
            const bool fUp = F(up), fUL = gx > 0 && F(up - 1), fLeft = lx > 0 && F(a - 1);
            if (fUp && !(fLeft && fUL)) mf_unite(N, a + OFF, up + OFF);
            if (CONN == 8) {
                if (fUL && !(lx > 0 && (fUp || fLeft))) mf_unite(N, a + OFF, up - 1 + OFF);
                if (gx + 1 < w && F(up + 1) && !(lx < MF_TW - 1 && fUp)) mf_unite(N, a + OFF, up + 1 + OFF);
            }
        }
        if (kind == 1 && gx > 0) {
            const bool fLf = F(a - 1), fLU = gy > 0 && F(a - w - 1), fAbove = ly > 0 && F(a - w);
            if (fLf && !(fAbove && fLU)) mf_unite(N, a + OFF, a - 1 + OFF);
            if (CONN == 8) {
                if (fLU && !(ly > 0 && (fLf || fAbove))) mf_unite(N, a + OFF, a - w - 1 + OFF);
                if (gy + 1 < h && F(a + w - 1) && !(ly < MF_TH - 1 && fLf)) mf_unite(N, a + OFF, a + w - 1 + OFF);
            }
        }
        if (OUT) {          // the image border joins node 0: the first pixel of every run along a side of the tile does it for the run
            const bool side = kind == 0 ? gy == 0 : kind == 1 ? gx == 0 : kind == 2 ? gy == h - 1 : gx == w - 1;
            const bool prev = (kind & 1) ? (ly > 0 && F(a - w)) : (lx > 0 && F(a - 1));
            if (side && !prev) mf_unite(N, a + OFF, 0);
        }
    }
}

// OUT: filled = 0 where the pixel's root is node 0, else 255 (the labels are not needed again).  Otherwise every pixel gets its root -- the blob's smallest
// index -- as its label, and what the tile-local roots hold of area and overlap goes to the root: one atomic per (tile, tile-local root)
template <bool OUT>
__global__ void __launch_bounds__(MF_T)
mf_flatten_kernel(int w, int h, size_t lstride, int32_t* __restrict__ labels, uint8_t* __restrict__ filled, int32_t* __restrict__ area, int32_t* __restrict__ overlap)
{
    const size_t px = (size_t)w * h, t = (size_t)blockIdx.x * MF_T + threadIdx.x;
    const int f = blockIdx.y;
    if (t >= px) return;
    int32_t* N = labels + (size_t)f * lstride;
    const int node = (int)t + (OUT ? 1 : 0);
    const int v = mf_load(&N[node]);
    if (OUT) { filled[(size_t)f * px + t] = (v >= 0 && mf_find(N, node) == 0) ? 0 : 255; return; }
    if (v < 0) return;
    const int R = mf_find(N, node);
    if (R == node) return;
    __hip_atomic_store(&N[node], R, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);          // (a chain through this entry reads the old parent or the root: both lead there)
    const size_t at = (size_t)f * px + t, to = (size_t)f * px + R;
    const int a = area[at];
    if (a > 0) {            // a tile-local root that is not the blob's: nothing is added INTO such an entry, so plain accesses of it are this thread's alone
        atomicAdd(&area[to], a);
        const int o = overlap[at];
        if (o > 0) atomicAdd(&overlap[to], o);
        area[at] = 0; overlap[at] = 0;
    }
}

// the decision per blob, read at the root by every pixel of it; the output mask; the frame's counters (info: blobs, large, confirmed, added; preset to 0)
__global__ void __launch_bounds__(MF_T)
mf_paint_kernel(int w, int h, size_t lstride, const int32_t* __restrict__ labels, const int32_t* __restrict__ area, const int32_t* __restrict__ overlap,
                const uint8_t* __restrict__ always, int32_t area_thres, double overlay_thres, uint8_t* __restrict__ out, int32_t* __restrict__ info)
{
    __shared__ int sums[4];
    const size_t px = (size_t)w * h, t = (size_t)blockIdx.x * MF_T + threadIdx.x;
    const int f = blockIdx.y;
    if (threadIdx.x < 4) sums[threadIdx.x] = 0;
    __syncthreads();
    int c[4] = {0, 0, 0, 0};
    if (t < px) {
        const size_t base = (size_t)f * px;
        const int R = labels[(size_t)f * lstride + t];
        bool conf = false;
        if (R >= 0) {
            const int a = area[base + R], o = overlap[base + R];
            conf = confirmed(a, o, area_thres, overlay_thres);
            if ((size_t)R == t) { c[0] = 1; c[1] = is_large(a, area_thres); c[2] = conf; }
        }
        const uint8_t al = always[base + t], m = al | (conf ? 255 : 0);
        out[base + t] = m;
        c[3] = m && !al;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        int v = c[j];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&sums[j], v);
    }
    __syncthreads();
    if (threadIdx.x < 4 && sums[threadIdx.x]) atomicAdd(&info[4 * f + threadIdx.x], sums[threadIdx.x]);
}

size_t k_mf_label_stride(int w, int h) { return (size_t)w * h + 1; }
hipError_t k_motion_fuse(const uint8_t* sem, const uint8_t* motion, int n, int w, int h, int32_t area_thres, double overlay_thres, uint8_t* always, uint8_t* cand,
                         uint8_t* filled, int32_t* labels, int32_t* area, int32_t* overlap, uint8_t* mask, int32_t* info, hipStream_t s)
{
    static_assert(MF_PX % MF_T == 0 && MF_T % MF_TW == 0, "whole rows of a tile per pass of the block");
    if (n <= 0) return hipSuccess;
    const int tx = (w + MF_TW - 1) / MF_TW, ty = (h + MF_TH - 1) / MF_TH;
    const size_t px = (size_t)w * h, ls = k_mf_label_stride(w, h);
    const dim3 tiles(tx * ty, n), flat((unsigned)((px + MF_T - 1) / MF_T), n);
    hipError_t e = hipMemsetAsync(info, 0, (size_t)n * 16, s);
    if (e != hipSuccess) return e;
    mf_class_kernel<<<tiles, MF_T, 0, s>>>(sem, w, h, tx, always, cand);
    mf_local_kernel<4, true><<<tiles, MF_T, 0, s>>>(cand, nullptr, w, h, tx, ls, labels, nullptr, nullptr);
    mf_merge_kernel<4, true><<<tiles, MF_T, 0, s>>>(w, h, tx, ls, labels);
    mf_flatten_kernel<true><<<flat, MF_T, 0, s>>>(w, h, ls, labels, filled, nullptr, nullptr);
    mf_local_kernel<8, false><<<tiles, MF_T, 0, s>>>(filled, motion, w, h, tx, ls, labels, area, overlap);
    mf_merge_kernel<8, false><<<tiles, MF_T, 0, s>>>(w, h, tx, ls, labels);
    mf_flatten_kernel<false><<<flat, MF_T, 0, s>>>(w, h, ls, labels, nullptr, area, overlap);
    mf_paint_kernel<<<flat, MF_T, 0, s>>>(w, h, ls, labels, area, overlap, always, area_thres, overlay_thres, mask, info);
    return hipGetLastError();
}
