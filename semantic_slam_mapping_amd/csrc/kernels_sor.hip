// kernels_sor.hip -- the statistical outlier removal of n points in device memory: bounds, the levels of the search ladder, the exact statistics
// and the stable compaction.  The arithmetic is include/ssm/sor_core.h, which the host function of ssm_sor_host.cpp calls too.
//
// One level: every point gets the key of its cell (non-finite points the key behind all cells), rocPRIM orders (key, index) and picks the still unsettled points
// in that order, and sor_search_kernel does the work.  A block has SOR_W waves and takes SOR_W consecutive queries; a wave owns ONE query and keeps its 64 best
// squared distances one per lane, ascending.  That form was chosen over a per-lane register list because it serves every k <= 64 with one instantiation and
// nothing indexed, and because 64 consecutive candidates of a sorted cell are one coalesced line per lane group: the inner loop is a distance, a compare
// against the k-th best and a ballot, and only a group in which some lane passes pays for the merge (bitonic sort of the 64 new, min with the reversed best,
// bitonic merge).  Queries are in key order, so the waves of a block mostly stand in the same cell: the block goes through its queries' cells in rounds,
// smallest key first; in a round the candidates -- the nine key runs around the cell, taken as one list -- stream through a fixed LDS chunk that is loaded once
// and consumed by every wave whose query is in that cell.  One cell may hold every point: the list is never sized to fit.  A query that has seen k others
// and whose k-th distance is within the level's bound is settled and writes its mean distance; the others are counted for the next level.  Integer atomics only,
// no grid barrier, no block waits for another.
#include "ssm_internal.h"
#include "../../include/ssm/sor_core.h"
#include <cstring>
#include <rocprim/rocprim.hpp>
using namespace ssm_sorc;

#define SOR_T 256
#define SOR_W (SOR_T / 64)
int k_sor_block() { return SOR_T; }

__device__ inline int sor_ord(float f) { const int i = __float_as_int(f); return i >= 0 ? i : i ^ 0x7FFFFFFF; }          // order-preserving, as k_voxel_bounds

__global__ void sor_init_kernel(SorHead* __restrict__ head)
{
    SorHead h{};
    for (int a = 0; a < 3; a++) { h.mn[a] = 0x7FFFFFFF; h.mx[a] = (int)0x80000000; }
    *head = h;
}
// the box and the number of the finite points; every point starts with no value, and a non-finite point is never a query
__global__ void __launch_bounds__(SOR_T)
sor_bounds_kernel(const ssm_point* __restrict__ pts, int n, SorHead* __restrict__ head, float* __restrict__ mean_dist, uint8_t* __restrict__ settled)
{
    const int i = blockIdx.x * SOR_T + threadIdx.x;
    int mn[3] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF}, mx[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000}, cnt = 0;
    if (i < n) {
        const float x = pts[i].x, y = pts[i].y, z = pts[i].z;
        const bool f = finite3(x, y, z);
        mean_dist[i] = 0.0f; settled[i] = f ? 0 : 1;
        if (f) { mn[0] = mx[0] = sor_ord(x); mn[1] = mx[1] = sor_ord(y); mn[2] = mx[2] = sor_ord(z); cnt = 1; }
    }
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; a++) { mn[a] = min(mn[a], __shfl_xor(mn[a], o)); mx[a] = max(mx[a], __shfl_xor(mx[a], o)); }
        cnt += __shfl_xor(cnt, o);
    }
    if ((threadIdx.x & 63) == 0 && cnt) {
#pragma unroll
        for (int a = 0; a < 3; a++) { atomicMin(&head->mn[a], mn[a]); atomicMax(&head->mx[a], mx[a]); }
        atomicAdd(&head->n_finite, cnt);
    }
}
__global__ void __launch_bounds__(SOR_T)
sor_keys_kernel(const ssm_point* __restrict__ pts, int n, float lox, float loy, float loz, double c, int top, uint64_t* __restrict__ keys, uint32_t* __restrict__ idx)
{
    const int i = blockIdx.x * SOR_T + threadIdx.x;
    if (i >= n) return;
    const float x = pts[i].x, y = pts[i].y, z = pts[i].z;
    const float lo[3] = {lox, loy, loz};
    keys[i] = !finite3(x, y, z) ? KEY_NONE : top ? 0 : point_key(x, y, z, lo, c);
    idx[i] = (uint32_t)i;
}
// the points in key order (w: the input index) and, in that order, who is still a query
__global__ void __launch_bounds__(SOR_T)
sor_gather_kernel(const ssm_point* __restrict__ pts, int n, const uint32_t* __restrict__ idx, const uint8_t* __restrict__ settled, float4* __restrict__ S, uint8_t* __restrict__ flags)
{
    const int s = blockIdx.x * SOR_T + threadIdx.x;
    if (s >= n) return;
    const uint32_t i = idx[s];
    S[s] = make_float4(pts[i].x, pts[i].y, pts[i].z, __uint_as_float(i));
    flags[s] = settled[i] ? 0 : 1;
}

__device__ inline float sor_sort64(float v, int lane)          // ascending over the wave
{
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1)
#pragma unroll
        for (int j = size >> 1; j > 0; j >>= 1) {
            const float o = __shfl_xor(v, j);
            const bool up = (lane & size) == 0 || size == 64, low = (lane & j) == 0;
            v = (low == up) ? fminf(v, o) : fmaxf(v, o);
        }
    return v;
}
__device__ inline float sor_merge64(float v, int lane)         // a bitonic sequence -> ascending
{
#pragma unroll
    for (int j = 32; j > 0; j >>= 1) { const float o = __shfl_xor(v, j); v = (lane & j) == 0 ? fminf(v, o) : fmaxf(v, o); }
    return v;
}

__global__ void __launch_bounds__(SOR_T)
sor_search_kernel(const float4* __restrict__ S, const uint64_t* __restrict__ keys, int nf, const uint32_t* __restrict__ Q, int k, float r2,
                  int top, float* __restrict__ mean_dist, uint8_t* __restrict__ settled, SorHead* head)
{
    __shared__ float4 chunk[CHUNK];
    __shared__ uint64_t wkey[SOR_W];
    __shared__ int run_lo[9], run_len[9], run_off[10];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nq = (int)head->nq;
    const int qi = blockIdx.x * SOR_W + wave;
    bool done = qi >= nq;
    int qpos = -1; float qx = 0.0f, qy = 0.0f, qz = 0.0f; uint32_t qidx = 0; uint64_t qkey = KEY_NONE;
    if (!done) {
        qpos = (int)Q[qi];
        const float4 q = S[qpos];
        qx = q.x; qy = q.y; qz = q.z; qidx = __float_as_uint(q.w); qkey = top ? 0 : keys[qpos];
    }
    const float inf = __int_as_float(0x7F800000);
    for (;;) {
        if (lane == 0) wkey[wave] = done ? KEY_NONE : qkey;
        __syncthreads();
        uint64_t K = wkey[0];
#pragma unroll
        for (int w = 1; w < SOR_W; w++) K = wkey[w] < K ? wkey[w] : K;
        if (K == KEY_NONE) break;                                     // block-uniform: every query of the block is done
        const bool active = !done && qkey == K;                       // wave-uniform
        if (threadIdx.x < 9) {
            int lo = 0, len = 0;
            if (top) { if (threadIdx.x == 0) len = nf; }
            else {
                const int64_t m = ((int64_t)1 << AXIS_BITS) - 1;
                uint64_t first, last;
                if (key_run((int64_t)(K & m), (int64_t)((K >> AXIS_BITS) & m), (int64_t)(K >> (2 * AXIS_BITS)), (int)threadIdx.x, &first, &last)) {
                    int a = 0, b = nf;                                // lower bound of `first`
                    while (a < b) { const int mid = (a + b) >> 1; if (keys[mid] < first) a = mid + 1; else b = mid; }
                    lo = a; b = nf;                                   // upper bound of `last`
                    while (a < b) { const int mid = (a + b) >> 1; if (keys[mid] <= last) a = mid + 1; else b = mid; }
                    len = a - lo;
                }
            }
            run_lo[threadIdx.x] = lo; run_len[threadIdx.x] = len;
        }
        __syncthreads();
        if (threadIdx.x == 0) { int o = 0; for (int r = 0; r < 9; r++) { run_off[r] = o; o += run_len[r]; } run_off[9] = o; }
        __syncthreads();
        const int total = run_off[9];                                 // the query itself is one of them
        float best = inf, kth = inf;
        for (int base = 0; base < total; base += CHUNK) {
            const int m = min(CHUNK, total - base);
            for (int t = threadIdx.x; t < m; t += SOR_T) {
                const int p = base + t;
                int r = 0;
                while (p >= run_off[r + 1]) r++;                      // p < run_off[9]
                const int g = run_lo[r] + (p - run_off[r]);
                float4 v = S[g];
                v.w = __int_as_float(g);
                chunk[t] = v;
            }
            __syncthreads();
            if (active) {
                for (int t0 = 0; t0 < m; t0 += 64) {
                    const int t = t0 + lane;
                    float d2 = inf;
                    if (t < m) { const float4 v = chunk[t]; if (__float_as_int(v.w) != qpos) d2 = dist2(qx, qy, qz, v.x, v.y, v.z); }
                    if (__any(d2 < kth)) {
                        const float up = sor_sort64(d2, lane);
                        best = sor_merge64(fminf(best, __shfl(up, 63 - lane)), lane);
                        kth = __shfl(best, k - 1);
                    }
                }
            }
            __syncthreads();
        }
        if (active) {
            if (top || (total - 1 >= k && kth <= r2)) {
                const double s = root(best);
                double sum = 0.0;
                for (int t = 0; t < k; t++) sum += __shfl(s, t);
                if (lane == 0) { mean_dist[qidx] = mean_of(sum, k); settled[qidx] = 1; }
            } else if (lane == 0) atomicAdd(&head->remaining, 1);
            done = true;
        }
    }
}

// the three exact sums over the finite points; a value off the grid raises `bad` and adds nothing
__global__ void __launch_bounds__(SOR_T)
sor_stats_kernel(const ssm_point* __restrict__ pts, int n, const float* __restrict__ mean_dist, SorHead* __restrict__ head)
{
    __shared__ unsigned long long part[SOR_W][3];
    __shared__ int bad_s;
    const int i = blockIdx.x * SOR_T + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) bad_s = 0;
    __syncthreads();
    unsigned long long s1 = 0, lo = 0, hi = 0;
    if (i < n && finite3(pts[i].x, pts[i].y, pts[i].z)) {
        const float d = mean_dist[i];
        if (!on_grid(d)) bad_s = 1;
        else { const uint64_t q = quantise(d), q2 = q * q; s1 = q; lo = q2 & 0xFFFFFFFFull; hi = q2 >> 32; }
    }
    for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o); lo += __shfl_xor(lo, o); hi += __shfl_xor(hi, o); }
    if (lane == 0) { part[wave][0] = s1; part[wave][1] = lo; part[wave][2] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < SOR_W; w++) { s1 += part[w][0]; lo += part[w][1]; hi += part[w][2]; }
        if (s1) atomicAdd(&head->s1, s1);
        if (lo) atomicAdd(&head->s2_lo, lo);
        if (hi) atomicAdd(&head->s2_hi, hi);
        if (bad_s) atomicOr(&head->bad, 1);
    }
}
// who stays, and how many of each block
__global__ void __launch_bounds__(SOR_T)
sor_keep_kernel(const ssm_point* __restrict__ pts, int n, const float* __restrict__ mean_dist, double threshold, int too_few, uint8_t* __restrict__ keep, uint32_t* __restrict__ block_cnt)
{
    __shared__ int cnt_s[SOR_W];
    const int i = blockIdx.x * SOR_T + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool kp = false;
    if (i < n) { kp = finite3(pts[i].x, pts[i].y, pts[i].z) && (too_few || keeps(mean_dist[i], threshold)); keep[i] = kp ? 1 : 0; }
    const int c = __popcll(__ballot(kp));
    if (lane == 0) cnt_s[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0; for (int w = 0; w < SOR_W; w++) t += cnt_s[w];
        block_cnt[blockIdx.x] = (uint32_t)t;
        if (blockIdx.x == 0) block_cnt[gridDim.x] = 0;                // the scan's last entry becomes the total
    }
}
// the stable move: a kept point goes to its block's offset plus its rank inside the block, all 32 bytes
__global__ void __launch_bounds__(SOR_T)
sor_compact_kernel(const ssm_point* __restrict__ pts, int n, const uint8_t* __restrict__ keep, const uint32_t* __restrict__ block_off, ssm_point* __restrict__ out)
{
    __shared__ int cnt_s[SOR_W];
    const int i = blockIdx.x * SOR_T + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool kp = i < n && keep[i];
    const unsigned long long b = __ballot(kp);
    if (lane == 0) cnt_s[wave] = __popcll(b);
    __syncthreads();
    if (!kp) return;
    uint32_t at = block_off[blockIdx.x] + (uint32_t)__popcll(b & (((unsigned long long)1 << lane) - 1));
    for (int w = 0; w < wave; w++) at += (uint32_t)cnt_s[w];
    const uint4* src = reinterpret_cast<const uint4*>(pts + i);
    uint4* dst = reinterpret_cast<uint4*>(out + at);
    dst[0] = src[0]; dst[1] = src[1];
}

// ------------------------------------------------------------------ launchers
static inline int sor_blocks(int n) { return (n + SOR_T - 1) / SOR_T; }
size_t k_sor_tmp_bytes(int n)
{
    size_t a = 0, b = 0, c = 0;
    (void)rocprim::radix_sort_pairs(nullptr, a, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n, 0, 64, (hipStream_t)0);
    (void)rocprim::select(nullptr, b, rocprim::counting_iterator<uint32_t>(0), (const uint8_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n, (hipStream_t)0);
    (void)rocprim::exclusive_scan(nullptr, c, (const uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t)0, (size_t)sor_blocks(n) + 1, rocprim::plus<uint32_t>(), (hipStream_t)0);
    return std::max(a, std::max(b, c)) + 256;
}
hipError_t k_sor_begin(const ssm_point* pts, int n, const SorBufs& B, hipStream_t s)
{
    sor_init_kernel<<<1, 1, 0, s>>>(B.head);
    if (n > 0) sor_bounds_kernel<<<sor_blocks(n), SOR_T, 0, s>>>(pts, n, B.head, B.mean_dist, B.settled);
    return hipGetLastError();
}
hipError_t k_sor_level(const ssm_point* pts, int n, int nf, const float lo[3], double c, int top, int k, float r2, int n_query, const SorBufs& B, hipStream_t s)
{
    sor_keys_kernel<<<sor_blocks(n), SOR_T, 0, s>>>(pts, n, lo[0], lo[1], lo[2], c, top, B.keys_a, B.idx_a);
    size_t bytes = B.tmp_bytes;
    hipError_t e = rocprim::radix_sort_pairs(B.tmp, bytes, B.keys_a, B.keys_b, B.idx_a, B.idx_b, (size_t)n, 0, 64, s);
    if (e != hipSuccess) return e;
    sor_gather_kernel<<<sor_blocks(n), SOR_T, 0, s>>>(pts, n, B.idx_b, B.settled, B.sorted, B.flags);
    bytes = B.tmp_bytes;
    e = rocprim::select(B.tmp, bytes, rocprim::counting_iterator<uint32_t>(0), B.flags, B.query, &B.head->nq, (size_t)n, s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(&B.head->remaining, 0, 4, s);
    if (e != hipSuccess) return e;
    sor_search_kernel<<<(n_query + SOR_W - 1) / SOR_W, SOR_T, 0, s>>>(B.sorted, B.keys_b, nf, B.query, k, r2, top, B.mean_dist, B.settled, B.head);
    return hipGetLastError();
}
hipError_t k_sor_stats(const ssm_point* pts, int n, const SorBufs& B, hipStream_t s)
{
    sor_stats_kernel<<<sor_blocks(n), SOR_T, 0, s>>>(pts, n, B.mean_dist, B.head);
    return hipGetLastError();
}
hipError_t k_sor_compact(const ssm_point* pts, int n, double threshold, int too_few, const SorBufs& B, ssm_point* out, hipStream_t s)
{
    const int nb = sor_blocks(n);
    sor_keep_kernel<<<nb, SOR_T, 0, s>>>(pts, n, B.mean_dist, threshold, too_few, B.keep, B.block_cnt);
    size_t bytes = B.tmp_bytes;
    const hipError_t e = rocprim::exclusive_scan(B.tmp, bytes, B.block_cnt, B.block_off, (uint32_t)0, (size_t)nb + 1, rocprim::plus<uint32_t>(), s);
    if (e != hipSuccess) return e;
    sor_compact_kernel<<<nb, SOR_T, 0, s>>>(pts, n, B.keep, B.block_off, out);
    return hipGetLastError();
}
