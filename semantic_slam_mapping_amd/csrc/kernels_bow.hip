// kernels_bow.hip -- the device looper (rgbd_tutor::Looper, reference include/looper.h / src/looper.cpp): vocabulary-tree descent, bag-of-words vector per
// frame, L1 scores against the stored frames and the ordered candidate list.  The arithmetic and its summation order are include/ssm/looper_core.h; nothing
// here uses a floating-point atomic, and no result depends on how blocks or waves are scheduled.
#include "ssm_internal.h"
#include "../../include/ssm/looper_core.h"
using namespace ssm_bow;

// ---- 1. word of every descriptor ------------------------------------------------------------------------------------------------------------------------
// Sub-group form: BOW_SG lanes walk the tree for one descriptor; at each node lane s takes the children s, s + BOW_SG, ... (a sibling group is one
// contiguous run of 32-byte rows: the sub-group's loads are adjacent), forms key = distance << 16 | child index and the sub-group takes the minimum key --
// the smallest distance, the EARLIEST child on ties.  The xor steps stay inside the aligned sub-group, whose lanes all run the same trip counts.
#define BOW_SG 16
#define BOW_T 256
__device__ __forceinline__ int hamming_q(const uint4& q0, const uint4& q1, const uint32_t* row)
{
    const uint4 a = *reinterpret_cast<const uint4*>(row), b = *reinterpret_cast<const uint4*>(row + 4);
    return __popc(q0.x ^ a.x) + __popc(q0.y ^ a.y) + __popc(q0.z ^ a.z) + __popc(q0.w ^ a.w) + __popc(q1.x ^ b.x) + __popc(q1.y ^ b.y) + __popc(q1.z ^ b.z) + __popc(q1.w ^ b.w);
}
__global__ __launch_bounds__(BOW_T) void bow_words_sg_kernel(Tree t, const uint8_t* __restrict__ desc, const int32_t* __restrict__ nkp, int n_fixed, int nframes, int cap, int32_t* __restrict__ words)
{
    const long long d = ((long long)blockIdx.x * BOW_T + threadIdx.x) / BOW_SG;
    const int sub = threadIdx.x % BOW_SG;
    if (d >= (long long)nframes * cap) return;
    const int f = (int)(d / cap), i = (int)(d % cap);
    int n = nkp ? nkp[f] : n_fixed; n = n < 0 ? 0 : (n > cap ? cap : n);
    if (i >= n) return;                                           // the whole sub-group leaves together
    const uint4* q = reinterpret_cast<const uint4*>(desc + (size_t)d * DESC_BYTES);
    const uint4 q0 = q[0], q1 = q[1];
    int node = 0;
    for (int lvl = 0; lvl < t.max_depth; lvl++) {
        const int nc = t.n_child[node]; if (nc == 0) break;
        const int first = t.first_child[node];
        unsigned key = 0xFFFFFFFFu;
        for (int c = sub; c < nc; c += BOW_SG) { const unsigned k = ((unsigned)hamming_q(q0, q1, t.desc + (size_t)(first + c) * DESC_WORDS) << 16) | (unsigned)c; key = k < key ? k : key; }
#pragma unroll
        for (int m = 1; m < BOW_SG; m <<= 1) { const unsigned o = (unsigned)__shfl_xor((int)key, m, BOW_SG); key = o < key ? o : key; }
        node = first + (int)(key & 0xFFFFu);
    }
    if (sub == 0) words[d] = t.word[node];
}
// One-lane form: a lane walks the tree for its own descriptor (looper_core.h descend with 16-byte loads); a wave gathers 64 different sibling groups
__global__ __launch_bounds__(BOW_T) void bow_words_lane_kernel(Tree t, const uint8_t* __restrict__ desc, const int32_t* __restrict__ nkp, int n_fixed, int nframes, int cap, int32_t* __restrict__ words)
{
    const long long d = (long long)blockIdx.x * BOW_T + threadIdx.x;
    if (d >= (long long)nframes * cap) return;
    const int f = (int)(d / cap), i = (int)(d % cap);
    int n = nkp ? nkp[f] : n_fixed; n = n < 0 ? 0 : (n > cap ? cap : n);
    if (i >= n) return;
    const uint4* q = reinterpret_cast<const uint4*>(desc + (size_t)d * DESC_BYTES);
    const uint4 q0 = q[0], q1 = q[1];
    int node = 0;
    for (int lvl = 0; lvl < t.max_depth; lvl++) {
        const int nc = t.n_child[node]; if (nc == 0) break;
        const int first = t.first_child[node];
        int best = 0, bd = hamming_q(q0, q1, t.desc + (size_t)first * DESC_WORDS);
#pragma unroll 4
        for (int c = 1; c < nc; c++) { const int dd = hamming_q(q0, q1, t.desc + (size_t)(first + c) * DESC_WORDS); if (dd < bd) { bd = dd; best = c; } }
        node = first + best;
    }
    words[d] = t.word[node];
}
hipError_t k_bow_words(const Tree& t, const uint8_t* desc, const int32_t* nkp, int n_fixed, int nframes, int cap, int32_t* words, int variant, hipStream_t s)
{
    const long long nd = (long long)nframes * cap; if (nd <= 0) return hipSuccess;
    if (variant == 1) bow_words_lane_kernel<<<dim3((unsigned)((nd + BOW_T - 1) / BOW_T)), dim3(BOW_T), 0, s>>>(t, desc, nkp, n_fixed, nframes, cap, words);
    else bow_words_sg_kernel<<<dim3((unsigned)((nd * BOW_SG + BOW_T - 1) / BOW_T)), dim3(BOW_T), 0, s>>>(t, desc, nkp, n_fixed, nframes, cap, words);
    return hipGetLastError();
}

// ---- 2. the vector of a frame: sort the word ids in LDS, run-length them, value = count additions of the weight, normalise ---------------------------------
// One block per frame.  LDS: keys[P] (P = the power of two >= cap, <= 4096) | pos[P + 1] (16 bits: start of run r in keys) | vals[P] doubles
#define BOWF_T 256
__device__ __forceinline__ double wave_tree_sum(double x)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) x = x + __shfl_xor(x, m, 64);
    return x;
}
__global__ __launch_bounds__(BOWF_T) void bow_frame_kernel(const int32_t* __restrict__ words, const double* __restrict__ weight, const int32_t* __restrict__ nkp, int n_fixed, int cap, int P,
                                                           int32_t* __restrict__ st_ids, double* __restrict__ st_vals, int32_t* __restrict__ st_m)
{
    extern __shared__ __align__(16) unsigned char smem[];
    double* vals = reinterpret_cast<double*>(smem);
    uint32_t* keys = reinterpret_cast<uint32_t*>(smem + (size_t)P * 8);
    uint16_t* pos = reinterpret_cast<uint16_t*>(smem + (size_t)P * 12);
    __shared__ int cnt[BOWF_T]; __shared__ int s_nvalid; __shared__ double s_norm;
    const int f = blockIdx.x, tid = threadIdx.x;
    int n = nkp ? nkp[f] : n_fixed; n = n < 0 ? 0 : (n > cap ? cap : n);
    const int32_t* wf = words + (size_t)f * cap;
    for (int i = tid; i < P; i += BOWF_T) {
        uint32_t k = 0xFFFFFFFFu;
        if (i < n) { const int w = wf[i]; if (w >= 0 && weight[w] > 0.0) k = (uint32_t)w; }
        keys[i] = k;
    }
    if (tid == 0) s_nvalid = 0;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += BOWF_T) {
                const int p = i ^ j;
                if (p > i) { const uint32_t a = keys[i], b = keys[p]; const bool up = (i & k) == 0; if ((a > b) == up) { keys[i] = b; keys[p] = a; } }
            }
            __syncthreads();
        }
    // run heads: thread tid owns keys[tid * per .. (tid + 1) * per)
    const int per = P / BOWF_T > 0 ? P / BOWF_T : 1;
    const int i0 = tid * per, i1 = (i0 + per < P) ? i0 + per : P;
    int heads = 0;
    for (int i = i0; i < i1 && i < P; i++) {
        const uint32_t k = keys[i];
        if (k == 0xFFFFFFFFu) continue;
        if (i == 0 || keys[i - 1] != k) heads++;
        if (i == P - 1 || keys[i + 1] == 0xFFFFFFFFu) s_nvalid = i + 1;          // one thread at most
    }
    cnt[tid] = (i0 < P) ? heads : 0;
    __syncthreads();
    for (int s = 1; s < BOWF_T; s <<= 1) { const int v = tid >= s ? cnt[tid - s] : 0; __syncthreads(); cnt[tid] += v; __syncthreads(); }
    const int m = cnt[BOWF_T - 1];
    int r = cnt[tid] - ((i0 < P) ? heads : 0);
    for (int i = i0; i < i1 && i < P; i++) { const uint32_t k = keys[i]; if (k != 0xFFFFFFFFu && (i == 0 || keys[i - 1] != k)) pos[r++] = (uint16_t)i; }
    if (tid == 0) pos[m] = (uint16_t)s_nvalid;
    __syncthreads();
    for (int e = tid; e < m; e += BOWF_T) { const int a = pos[e]; vals[e] = word_value(weight[keys[a]], (int)pos[e + 1] - a); }
    __syncthreads();
    if (tid < 64) {
        double s = 0.0;
        for (int e = tid; e < m; e += 64) s = s + fabs(vals[e]);
        s = wave_tree_sum(s);
        if (tid == 0) s_norm = s;
    }
    __syncthreads();
    const double norm = s_norm;
    int32_t* oi = st_ids + (size_t)f * cap; double* ov = st_vals + (size_t)f * cap;
    for (int e = tid; e < m; e += BOWF_T) { const double v = vals[e]; oi[e] = (int32_t)keys[pos[e]]; ov[e] = norm > 0.0 ? v / norm : v; }
    if (tid == 0) st_m[f] = m;
}
size_t k_bow_frame_lds(int P) { return (size_t)P * 12 + ((size_t)P + 1) * 2 + 14; }
hipError_t k_bow_frame(const int32_t* words, const double* weight, const int32_t* nkp, int n_fixed, int nframes, int cap, int P, int32_t* st_ids, double* st_vals, int32_t* st_m, hipStream_t s)
{
    if (nframes <= 0) return hipSuccess;
    bow_frame_kernel<<<dim3(nframes), dim3(BOWF_T), k_bow_frame_lds(P), s>>>(words, weight, nkp, n_fixed, cap, P, st_ids, st_vals, st_m);
    return hipGetLastError();
}

// ---- 3. append the staged vectors to the database (CSR): frame f goes behind the frames before it.  hdr[0] is set when the database would overflow (the host
// sizes it from an upper bound, so it never should); nothing is written then
__global__ __launch_bounds__(256) void bow_append_kernel(const int32_t* __restrict__ st_ids, const double* __restrict__ st_vals, const int32_t* __restrict__ st_m, int nframes, int cap,
                                                         int32_t* __restrict__ offsets, int e0, int32_t* __restrict__ db_ids, double* __restrict__ db_vals, long long db_cap, int32_t* __restrict__ hdr)
{
    __shared__ int part[256]; __shared__ long long s_base;
    const int f = blockIdx.x, tid = threadIdx.x;
    int s = 0;
    for (int g = tid; g < f; g += 256) s += st_m[g];
    part[tid] = s; __syncthreads();
    for (int k = 128; k > 0; k >>= 1) { if (tid < k) part[tid] += part[tid + k]; __syncthreads(); }
    if (tid == 0) s_base = (long long)offsets[e0] + part[0];
    __syncthreads();
    const long long base = s_base; const int m = st_m[f];
    if (base + m > db_cap) { if (tid == 0) atomicOr(hdr, 1); return; }
    for (int e = tid; e < m; e += 256) { db_ids[base + e] = st_ids[(size_t)f * cap + e]; db_vals[base + e] = st_vals[(size_t)f * cap + e]; }
    if (tid == 0) offsets[e0 + f + 1] = (int32_t)(base + m);
}
hipError_t k_bow_append(const int32_t* st_ids, const double* st_vals, const int32_t* st_m, int nframes, int cap, int32_t* offsets, int e0, int32_t* db_ids, double* db_vals, long long db_cap, int32_t* hdr, hipStream_t s)
{
    if (nframes <= 0) return hipSuccess;
    bow_append_kernel<<<dim3(nframes), dim3(256), 0, s>>>(st_ids, st_vals, st_m, nframes, cap, offsets, e0, db_ids, db_vals, db_cap, hdr);
    return hipGetLastError();
}

// ---- 4. scores: one block per query entry, its vector in LDS (ids | vals); one wave per stored entry at a time, lane l taking that entry's positions l, l + 64, ...
// and looking each word up in the query by binary search.  Lane sums + xor butterfly = looper_core.h score().  The block also counts the query's candidates.
#define BOWS_T 512
__device__ __forceinline__ int query_limit(int q, int against) { return against < 0 ? q + 1 : against; }
__global__ __launch_bounds__(BOWS_T) void bow_score_kernel(const int32_t* __restrict__ offsets, const int32_t* __restrict__ db_ids, const double* __restrict__ db_vals, const int32_t* __restrict__ frame_ids,
                                                           int first, int against, int row, int qcap, double min_score, int min_interval, double* __restrict__ scores, int32_t* __restrict__ counts)
{
    extern __shared__ __align__(16) unsigned char smem[];
    double* qv = reinterpret_cast<double*>(smem);
    int32_t* qi = reinterpret_cast<int32_t*>(smem + (size_t)qcap * 8);
    __shared__ int s_count;
    const int q = first + blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qo = offsets[q]; int mq = offsets[q + 1] - qo; mq = mq > qcap ? qcap : mq;
    for (int i = tid; i < mq; i += BOWS_T) { qi[i] = db_ids[qo + i]; qv[i] = db_vals[qo + i]; }
    if (tid == 0) s_count = 0;
    __syncthreads();
    const int lim = query_limit(q, against), fq = frame_ids[q];
    int mine = 0;
    for (int e = wave; e < lim; e += BOWS_T / 64) {
        const int o0 = offsets[e], o1 = offsets[e + 1];
        double acc = 0.0;
        if (mq > 0)
            for (int j = o0 + lane; j < o1; j += 64) {
                const int w = db_ids[j];
                int lo = 0, hi = mq;
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (qi[mid] < w) lo = mid + 1; else hi = mid; }
                if (lo < mq && qi[lo] == w) acc = acc + score_term(qv[lo], db_vals[j]);
            }
        acc = wave_tree_sum(acc);
        const double sc = (mq > 0 && o1 > o0) ? score_from_sum(acc) : 0.0;
        if (lane == 0) {
            scores[(size_t)blockIdx.x * row + e] = sc;
            int df = frame_ids[e] - fq; df = df < 0 ? -df : df;
            if (sc > min_score && df > min_interval) mine++;
        }
    }
    if (lane == 0 && mine) atomicAdd(&s_count, mine);            // integers: the order does not matter
    __syncthreads();
    if (tid == 0) counts[blockIdx.x] = s_count;
}
// candidates in (query, entry) order: the query's slot range comes from the prefix sum of the counts; inside it the entries are emitted in ascending order
__global__ __launch_bounds__(256) void bow_emit_kernel(const int32_t* __restrict__ frame_ids, const double* __restrict__ scores, const int32_t* __restrict__ counts, int first, int nq, int against, int row,
                                                       double min_score, int min_interval, int32_t* __restrict__ pairs, double* __restrict__ out_scores, int cap, int32_t* __restrict__ hdr)
{
    __shared__ int part[256]; __shared__ int s_base, s_run;
    const int b = blockIdx.x, tid = threadIdx.x, q = first + b;
    int s = 0;
    for (int g = tid; g < b; g += 256) s += counts[g];
    part[tid] = s; __syncthreads();
    for (int k = 128; k > 0; k >>= 1) { if (tid < k) part[tid] += part[tid + k]; __syncthreads(); }
    if (tid == 0) { s_base = part[0]; s_run = 0; if (b == nq - 1) hdr[1] = part[0] + counts[b]; }
    __syncthreads();
    const int base = s_base, lim = query_limit(q, against), fq = frame_ids[q];
    for (int e0 = 0; e0 < lim; e0 += 256) {
        const int e = e0 + tid; bool c = false; double sc = 0.0;
        if (e < lim) { sc = scores[(size_t)b * row + e]; int df = frame_ids[e] - fq; df = df < 0 ? -df : df; c = sc > min_score && df > min_interval; }
        part[tid] = c ? 1 : 0; __syncthreads();
        for (int k = 1; k < 256; k <<= 1) { const int v = tid >= k ? part[tid - k] : 0; __syncthreads(); part[tid] += v; __syncthreads(); }
        const int run = s_run;
        if (c) { const int slot = base + run + part[tid] - 1; if (slot < cap) { pairs[2 * (size_t)slot] = q; pairs[2 * (size_t)slot + 1] = e; out_scores[slot] = sc; } }
        __syncthreads();
        if (tid == 0) s_run = run + part[255];
        __syncthreads();
    }
}
size_t k_bow_score_lds(int qcap) { return (size_t)qcap * 12; }
hipError_t k_bow_score(const int32_t* offsets, const int32_t* db_ids, const double* db_vals, const int32_t* frame_ids, int first, int nq, int against, int row, int qcap,
                       double min_score, int min_interval, double* scores, int32_t* counts, hipStream_t s)
{
    if (nq <= 0) return hipSuccess;
    bow_score_kernel<<<dim3(nq), dim3(BOWS_T), k_bow_score_lds(qcap), s>>>(offsets, db_ids, db_vals, frame_ids, first, against, row, qcap, min_score, min_interval, scores, counts);
    return hipGetLastError();
}
hipError_t k_bow_emit(const int32_t* frame_ids, const double* scores, const int32_t* counts, int first, int nq, int against, int row, double min_score, int min_interval,
                      int32_t* pairs, double* out_scores, int cap, int32_t* hdr, hipStream_t s)
{
    if (nq <= 0) return hipSuccess;
    bow_emit_kernel<<<dim3(nq), dim3(256), 0, s>>>(frame_ids, scores, counts, first, nq, against, row, min_score, min_interval, pairs, out_scores, cap, hdr);
    return hipGetLastError();
}
