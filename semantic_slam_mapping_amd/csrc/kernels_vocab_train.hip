// kernels_vocab_train.hip -- vocabulary training on the device: one level of the hierarchical k-majority tree at a time, all nodes of the
// level together.  The arithmetic is include/ssm/vocab_train_core.h.  Integers only; the atomics are integer adds of counts and a 64-bit integer maximum
// (seed_key), whose results do not depend on the order they arrive in; no block waits for another, and every loop ends after at most k or VT_CHUNK trips:
// "has anything changed" is a flag the host reads between launches.
#include "ssm_internal.h"
#include "../../include/ssm/vocab_train_core.h"
using namespace ssm_vt;
#define VT_T VT_CHUNK
static_assert(VT_T == 256, "one thread per descriptor bit");

__device__ __forceinline__ int vt_hamming(const uint4& q0, const uint4& q1, const uint32_t* row)
{
    const uint4 a = *reinterpret_cast<const uint4*>(row), b = *reinterpret_cast<const uint4*>(row + 4);
    return __popc(q0.x ^ a.x) + __popc(q0.y ^ a.y) + __popc(q0.z ^ a.z) + __popc(q0.w ^ a.w) + __popc(q1.x ^ b.x) + __popc(q1.y ^ b.y) + __popc(q1.z ^ b.z) + __popc(q1.w ^ b.w);
}
__device__ __forceinline__ unsigned long long vt_wave_max(unsigned long long x)
{
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)x, s, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(x >> 32), s, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        x = o > x ? o : x;
    }
    return x;
}

// ---- 1. seeding round r ------------------------------------------------------------------------------------------------------------------------------------
// One thread per position.  Centre r of the thread's node is the node's first member (r = 0) or the argmax the previous round left in keys_in; a distance of 0
// there means the node has stopped seeding, and since nothing is written for it any more its later keys stay 0 too.  The thread keeps m = the distance to the
// nearest centre so far and a = that centre (replaced only by a strictly smaller distance: the lowest centre on ties, ssm_vt::nearest), and offers
// seed_key(m, input index) for the next centre.  A wave whose live lanes all sit in one node reduces its keys first and sends one atomic.
__global__ __launch_bounds__(VT_T) void vt_seed_kernel(VtLevel L, int r, const unsigned long long* __restrict__ keys_in, unsigned long long* __restrict__ keys_out)
{
    const int p = blockIdx.x * VT_T + threadIdx.x;
    const bool valid = p < L.N;
    const int v = valid ? L.nodeof[p] : -1;
    bool live = valid;
    unsigned long long key = 0;
    if (valid) {
        const int first = L.start[v];
        uint32_t cidx;
        if (r == 0) cidx = (uint32_t)L.perm[first];
        else { const unsigned long long kin = keys_in[v]; live = seed_key_dist(kin) != 0; cidx = seed_key_index(kin); }
        if (live) {
            const uint32_t idx = (uint32_t)L.perm[p];
            const uint4* q = reinterpret_cast<const uint4*>(L.desc + (size_t)idx * DESC_WORDS);
            const uint4 q0 = q[0], q1 = q[1];
            const uint32_t* c = L.desc + (size_t)cidx * DESC_WORDS;
            int d = vt_hamming(q0, q1, c);
            if (r == 0) { L.m[p] = d; L.a[p] = 0; }
            else { const int mo = L.m[p]; if (d < mo) { L.m[p] = d; L.a[p] = r; } else d = mo; }
            if (p == first) {
                uint4* out = reinterpret_cast<uint4*>(L.centres + ((size_t)v * L.k + r) * DESC_WORDS);
                out[0] = reinterpret_cast<const uint4*>(c)[0]; out[1] = reinterpret_cast<const uint4*>(c)[1];
                L.ncent[v] = r + 1;
            }
            key = seed_key(d, idx);
        }
    }
    if (!keys_out) return;                                       // (uniform: a kernel argument)
    const int v0 = __shfl(v, 0, 64);
    if (__all(!live || v == v0)) {
        const unsigned long long best = vt_wave_max(key);
        if ((threadIdx.x & 63) == 0 && best) atomicMax(&keys_out[v0], best);
    } else if (live) atomicMax(&keys_out[v], key);
}

// ---- 2. centre update --------------------------------------------------------------------------------------------------------------------------------------
// One block per chunk; thread t owns descriptor bit t.  The chunk's rows, nodes and clusters are staged in LDS; the block then walks its VT_CHUNK positions and
// thread t adds bit t of the row into cnt[cluster][t] (its own column: no atomics, no bank conflicts; the row word and the cluster are broadcast reads).  The
// positions of a node are consecutive, so when the node changes the columns are flushed: a node that lies inside the chunk gets its new centres right here
// (32 bits per half wave by a ballot), a node that crosses a chunk boundary adds its columns into its gcnt slot for vt_finish_kernel.
__global__ __launch_bounds__(VT_T) void vt_count_kernel(VtLevel L)
{
    __shared__ __align__(16) uint32_t sdesc[VT_T * DESC_WORDS];
    __shared__ int snode[VT_T], sa[VT_T], scount[MAX_K];
    __shared__ uint32_t cnt[MAX_K * VT_T];
    const int t = threadIdx.x, base = blockIdx.x * VT_T;
    const int cm = L.N - base < VT_T ? L.N - base : VT_T;       // >= 1: the grid is the chunk count
    if (t < cm) {
        const int p = base + t;
        const uint4* q = reinterpret_cast<const uint4*>(L.desc + (size_t)(uint32_t)L.perm[p] * DESC_WORDS);
        reinterpret_cast<uint4*>(sdesc)[t * 2] = q[0]; reinterpret_cast<uint4*>(sdesc)[t * 2 + 1] = q[1];
        snode[t] = L.nodeof[p]; sa[t] = L.a[p];
    }
    for (int j = 0; j < L.k; j++) cnt[j * VT_T + t] = 0;
    int mycount = 0;                                             // thread j < k: the members of cluster j in the current node
    __syncthreads();
    const int w = t >> 5, b = t & 31;
    auto flush = [&](int v) {
        if (t < L.k) scount[t] = mycount;
        mycount = 0;
        __syncthreads();
        const int s = L.start[v], e = L.start[v + 1];
        if (s >= base && e <= base + VT_T) {
            for (int j = 0; j < L.k; j++) {
                const int n = scount[j];
                if (n == 0) continue;                            // (uniform) an empty cluster keeps its centre
                const unsigned long long mask = __ballot(majority_bit((int)cnt[j * VT_T + t], n));
                cnt[j * VT_T + t] = 0;
                if ((t & 63) == 0) { uint32_t* c = L.centres + ((size_t)v * L.k + j) * DESC_WORDS + (t >> 6) * 2; c[0] = (uint32_t)mask; c[1] = (uint32_t)(mask >> 32); }
            }
        } else {
            uint32_t* g = L.gcnt + (size_t)(s / VT_T) * L.k * 257;
            for (int j = 0; j < L.k; j++) {
                const int n = scount[j];
                if (n == 0) continue;
                const uint32_t x = cnt[j * VT_T + t];
                cnt[j * VT_T + t] = 0;
                if (x) atomicAdd(&g[j * 257 + t], x);
                if (t == 0) atomicAdd(&g[j * 257 + 256], (uint32_t)n);
            }
        }
        __syncthreads();
    };
    int cur = snode[0];
    for (int i = 0; i < cm; i++) {
        const int v = snode[i];
        if (v != cur) { flush(cur); cur = v; }                   // (uniform: every thread reads the same snode[i])
        const int j = sa[i];
        cnt[j * VT_T + t] += (sdesc[i * DESC_WORDS + w] >> b) & 1u;
        mycount += t == j;
    }
    flush(cur);
}
__global__ __launch_bounds__(VT_T) void vt_finish_kernel(VtLevel L, const int32_t* __restrict__ strad)
{
    const int t = threadIdx.x, v = strad[blockIdx.x];
    uint32_t* g = L.gcnt + (size_t)(L.start[v] / VT_T) * L.k * 257;
    for (int j = 0; j < L.k; j++) {
        const int n = (int)g[j * 257 + 256];
        if (n == 0) continue;                                    // (uniform)
        const unsigned long long mask = __ballot(majority_bit((int)g[j * 257 + t], n));
        if ((t & 63) == 0) { uint32_t* c = L.centres + ((size_t)v * L.k + j) * DESC_WORDS + (t >> 6) * 2; c[0] = (uint32_t)mask; c[1] = (uint32_t)(mask >> 32); }
        g[j * 257 + t] = 0;
    }
    __syncthreads();                                             // every thread has read the counts
    if (t < L.k) g[t * 257 + 256] = 0;
}

// ---- 3. assignment -----------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VT_T) void vt_assign_kernel(VtLevel L, int pass)
{
    const int p = blockIdx.x * VT_T + threadIdx.x;
    if (p >= L.N) return;
    const int v = L.nodeof[p], nc = L.ncent[v];
    const uint4* q = reinterpret_cast<const uint4*>(L.desc + (size_t)(uint32_t)L.perm[p] * DESC_WORDS);
    const uint4 q0 = q[0], q1 = q[1];
    const uint32_t* c = L.centres + (size_t)v * L.k * DESC_WORDS;
    int best = 0, bd = vt_hamming(q0, q1, c);
    for (int j = 1; j < nc; j++) { const int d = vt_hamming(q0, q1, c + j * DESC_WORDS); if (d < bd) { bd = d; best = j; } }
    if (best != L.a[p]) { L.a[p] = best; L.changed_at[v] = pass; L.flag[0] = 1; }      // (racing stores of one value)
}

// ---- 4. stable partition by cluster ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VT_T) void vt_hist_kernel(VtLevel L, int32_t* __restrict__ hist)
{
    __shared__ int wtot[4][MAX_K];
    const int p = blockIdx.x * VT_T + threadIdx.x, wv = threadIdx.x >> 6;
    const int a = p < L.N ? L.a[p] : -1;
    for (int j = 0; j < L.k; j++) { const unsigned long long mask = __ballot(a == j); if ((threadIdx.x & 63) == 0) wtot[wv][j] = __popcll(mask); }
    __syncthreads();
    if (threadIdx.x < L.k) hist[(size_t)blockIdx.x * L.k + threadIdx.x] = wtot[0][threadIdx.x] + wtot[1][threadIdx.x] + wtot[2][threadIdx.x] + wtot[3][threadIdx.x];
}
__global__ __launch_bounds__(VT_T) void vt_rank_kernel(VtLevel L, const int32_t* __restrict__ prefix, int32_t* __restrict__ rank, int32_t* __restrict__ noderank)
{
    __shared__ int wtot[4][MAX_K];
    const int p = blockIdx.x * VT_T + threadIdx.x, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool valid = p < L.N;
    const int a = valid ? L.a[p] : -1, v = valid ? L.nodeof[p] : 0;
    const bool first = valid && p == L.start[v];
    for (int j = 0; j < L.k; j++) { const unsigned long long mask = __ballot(a == j); if (lane == 0) wtot[wv][j] = __popcll(mask); }
    __syncthreads();
    const unsigned long long below = lane ? ~0ull >> (64 - lane) : 0ull;
    for (int j = 0; j < L.k; j++) {
        const unsigned long long mask = __ballot(a == j);
        int r = prefix[(size_t)blockIdx.x * L.k + j] + __popcll(mask & below);
        for (int x = 0; x < 3; x++) if (x < wv) r += wtot[x][j];
        if (a == j) rank[p] = r;
        if (first) noderank[(size_t)v * L.k + j] = r;
    }
}
__global__ __launch_bounds__(VT_T) void vt_scatter_kernel(VtLevel L, const int32_t* __restrict__ rank, const int32_t* __restrict__ noderank, const int32_t* __restrict__ dest,
                                                          const int32_t* __restrict__ child, int32_t* __restrict__ perm_out, int32_t* __restrict__ nodeof_out)
{
    const int p = blockIdx.x * VT_T + threadIdx.x;
    if (p >= L.N) return;
    const size_t at = (size_t)L.nodeof[p] * L.k + L.a[p];
    const int to = dest[at] + (rank[p] - noderank[at]);
    if (to < 0 || to >= L.N) return;                             // (cannot happen: the host made dest from the same counts)
    perm_out[to] = L.perm[p]; nodeof_out[to] = child[at];
}
__global__ __launch_bounds__(VT_T) void vt_leaves_kernel(VtLevel L, const int32_t* __restrict__ leaf_id, int32_t* __restrict__ leaf_of_feature)
{
    const int p = blockIdx.x * VT_T + threadIdx.x;
    if (p >= L.N) return;
    const int i = L.perm[p], v = L.nodeof[p];
    if ((unsigned)i < (unsigned)L.N && (unsigned)v < (unsigned)L.nn) leaf_of_feature[i] = leaf_id[v];
}

static inline unsigned vt_chunks(const VtLevel& L) { return (unsigned)((L.N + VT_T - 1) / VT_T); }
hipError_t k_vt_seed(const VtLevel& L, int r, const unsigned long long* keys_in, unsigned long long* keys_out, hipStream_t s)
{ hipLaunchKernelGGL(vt_seed_kernel, dim3(vt_chunks(L)), dim3(VT_T), 0, s, L, r, keys_in, keys_out); return hipGetLastError(); }
hipError_t k_vt_count(const VtLevel& L, hipStream_t s) { hipLaunchKernelGGL(vt_count_kernel, dim3(vt_chunks(L)), dim3(VT_T), 0, s, L); return hipGetLastError(); }
hipError_t k_vt_finish(const VtLevel& L, const int32_t* strad, int ns, hipStream_t s)
{ if (ns <= 0) return hipSuccess; hipLaunchKernelGGL(vt_finish_kernel, dim3((unsigned)ns), dim3(VT_T), 0, s, L, strad); return hipGetLastError(); }
hipError_t k_vt_assign(const VtLevel& L, int pass, hipStream_t s) { hipLaunchKernelGGL(vt_assign_kernel, dim3(vt_chunks(L)), dim3(VT_T), 0, s, L, pass); return hipGetLastError(); }
hipError_t k_vt_hist(const VtLevel& L, int32_t* hist, hipStream_t s) { hipLaunchKernelGGL(vt_hist_kernel, dim3(vt_chunks(L)), dim3(VT_T), 0, s, L, hist); return hipGetLastError(); }
hipError_t k_vt_rank(const VtLevel& L, const int32_t* prefix, int32_t* rank, int32_t* noderank, hipStream_t s)
{ hipLaunchKernelGGL(vt_rank_kernel, dim3(vt_chunks(L)), dim3(VT_T), 0, s, L, prefix, rank, noderank); return hipGetLastError(); }
hipError_t k_vt_scatter(const VtLevel& L, const int32_t* rank, const int32_t* noderank, const int32_t* dest, const int32_t* child, int32_t* perm_out, int32_t* nodeof_out, hipStream_t s)
{ hipLaunchKernelGGL(vt_scatter_kernel, dim3(vt_chunks(L)), dim3(VT_T), 0, s, L, rank, noderank, dest, child, perm_out, nodeof_out); return hipGetLastError(); }
hipError_t k_vt_leaves(const VtLevel& L, const int32_t* leaf_id, int32_t* leaf_of_feature, hipStream_t s)
{ hipLaunchKernelGGL(vt_leaves_kernel, dim3(vt_chunks(L)), dim3(VT_T), 0, s, L, leaf_id, leaf_of_feature); return hipGetLastError(); }
