// ssm_sor.hip -- the device path of the statistical outlier removal behind the C ABI.  DESIGN.md s.15 is the contract.  A call is the launches of
// kernels_sor.hip on the main stream with one small read between them where the host has to decide: the finite points' box (it fixes the ladder), the number
// of points a level left unsettled (it sizes the next level, and ends the ladder), the three sums (the threshold's sqrt is evaluated on the host, in
// sor_core.h's stats_of) and the number kept.  The workspaces belong to the context (SorWork) and grow with the largest call.  The host function, the defaults
// and the argument check are ssm_sor_host.cpp.
#include "ssm_ctx.h"
#include "ssm_host.h"
using namespace ssm_sorc;

static int sor_reserve(ssm_ctx* c, int n)
{
    SorWork& W = c->sor;
    if (n <= W.cap) return SSM_OK;
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    const size_t m = (size_t)std::max(n, 1024), nb = (m + k_sor_block() - 1) / k_sor_block() + 1;
    W.cap = 0; W.n = 0;
    DALLOC(c, W.head, 1); DALLOC(c, W.h_head, 2);
    DALLOC(c, W.mean_dist, m); DALLOC(c, W.settled, m); DALLOC(c, W.keep, m); DALLOC(c, W.flags, m);
    DALLOC(c, W.keys_a, m); DALLOC(c, W.keys_b, m); DALLOC(c, W.idx_a, m); DALLOC(c, W.idx_b, m); DALLOC(c, W.query, m); DALLOC(c, W.sorted, m);
    DALLOC(c, W.block_cnt, nb); DALLOC(c, W.block_off, nb);
    W.tmp_bytes = k_sor_tmp_bytes((int)m); DALLOC(c, W.tmp, W.tmp_bytes);
    DALLOC(c, W.out, m); W.in.reset();
    W.cap = (int)m;
    return SSM_OK;
}
static inline float sor_unord(int i) { i = i >= 0 ? i : i ^ 0x7FFFFFFF; float f; memcpy(&f, &i, 4); return f; }
static int sor_read_head(ssm_ctx* c, SorHead* h)
{
    SorWork& W = c->sor; hipStream_t s = c->main.stream;
    HIPCHK(c, hipMemcpyAsync(W.h_head, W.head, sizeof(SorHead), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    *h = *W.h_head;
    return SSM_OK;
}
int sor_run(ssm_ctx* c, const ssm_point* d_pts, int n, const ssm_sor_params* params, ssm_sor_info* info)
{
    ssm_sor_params P; ssm_sor_params_default(&P); if (params) P = *params;
    { const int r = sor_check(c, n, P); if (r) return r; }
    SorWork& W = c->sor; hipStream_t s = c->main.stream;
    ssm_sor_info I{}; I.n_in = n;
    W.n = 0; W.levels = 0;
    if (n == 0) { I.too_few = 1; if (info) *info = I; return SSM_OK; }
    { const int r = sor_reserve(c, n); if (r) return r; }
    const SorBufs B{W.head, W.mean_dist, W.settled, W.keep, W.flags, W.keys_a, W.keys_b, W.idx_a, W.idx_b, W.query, W.block_cnt, W.block_off, W.sorted, W.tmp, W.tmp_bytes};
    const int k = P.mean_k;
    SorHead H;
    prof_begin(c, s, "sor");
    HIPCHK(c, k_sor_begin(d_pts, n, B, s));
    { const int r = sor_read_head(c, &H); if (r) return r; }
    const int nf = H.n_finite;
    I.n_finite = nf;
    double threshold = 0.0;
    if (nf < k + 1) I.too_few = 1;
    else {
        float lo[3], hi[3];
        for (int a = 0; a < 3; a++) { lo[a] = sor_unord(H.mn[a]); hi[a] = sor_unord(H.mx[a]); }
        const Plan plan = plan_of(lo, hi, P.cell, nf);
        int nq = nf;
        for (int level = 0; nq > 0; level++) {
            const int top = level >= plan.top;
            W.level_q[level] = nq; W.levels = level + 1;
            const double cl = level_cell(plan.c0, level);
            HIPCHK(c, k_sor_level(d_pts, n, nf, plan.lo, cl, top, k, settle_r2(cl), nq, B, s));
            { const int r = sor_read_head(c, &H); if (r) return r; }
            I.levels = level + 1;
            if (top && H.remaining) FAIL(c, SSM_E_HIP, "sor: the top level left points unsettled");
            nq = H.remaining;
        }
        HIPCHK(c, k_sor_stats(d_pts, n, B, s));
        { const int r = sor_read_head(c, &H); if (r) return r; }
        if (H.bad) { prof_end(c, s); return sor_off_grid(c); }
        I.sum_q = H.s1; I.sum_q2_lo = H.s2_lo; I.sum_q2_hi = H.s2_hi;
        const Stats st = stats_of(nf, I.sum_q, I.sum_q2_lo, I.sum_q2_hi, P.stddev_mul);
        I.mean = st.mean; I.stddev = st.stddev; I.threshold = threshold = st.threshold;
    }
    HIPCHK(c, k_sor_compact(d_pts, n, threshold, I.too_few, B, W.out, s));
    uint32_t* h_kept = reinterpret_cast<uint32_t*>(W.h_head + 1);
    HIPCHK(c, hipMemcpyAsync(h_kept, W.block_off + (n + k_sor_block() - 1) / k_sor_block(), 4, hipMemcpyDeviceToHost, s));
    prof_end(c, s);
    HIPCHK(c, hipStreamSynchronize(s));
    I.n_kept = (int)*h_kept;
    W.n = n;
    if (info) *info = I;
    return SSM_OK;
}

extern "C" int ssm_sor_filter(ssm_ctx* c, const ssm_point* pts, int n, const ssm_sor_params* params, ssm_point* out, int cap, int* n_out, ssm_sor_info* info)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (!n_out || (n > 0 && !pts) || cap < 0) FAIL(c, SSM_E_INVAL, "null argument");
    *n_out = 0;
    SorWork& W = c->sor; hipStream_t s = c->main.stream;
    ssm_sor_info I{};
    if (n > 0) {
        { ssm_sor_params P; ssm_sor_params_default(&P); if (params) P = *params; const int r = sor_check(c, n, P); if (r) return r; }
        { const int r = sor_reserve(c, n); if (r) return r; }
        if (!W.in) DALLOC(c, W.in, W.cap);
        HIPCHK(c, hipMemcpyAsync(W.in, pts, (size_t)n * sizeof(ssm_point), hipMemcpyHostToDevice, s));
    }
    { const int r = sor_run(c, W.in, n, params, &I); if (r) return r; }
    *n_out = I.n_kept;
    if (info) *info = I;
    if (I.n_kept > cap) FAIL(c, SSM_E_CAPACITY, "point buffer too small (need " + std::to_string(I.n_kept) + ")");
    if (I.n_kept == 0) return SSM_OK;
    if (!out) FAIL(c, SSM_E_INVAL, "null argument");
    HIPCHK(c, hipMemcpyAsync(out, W.out, (size_t)I.n_kept * sizeof(ssm_point), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return SSM_OK;
}
extern "C" int ssm_cloud_sor(ssm_ctx* c, ssm_cloud* cl, const ssm_sor_params* params, ssm_sor_info* info)
{
    if (!c || !cl) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (cl->device != c->device) FAIL(c, SSM_E_INVAL, "cloud of another device");
    if (cl->run) FAIL(c, SSM_E_INVAL, "sor: the cloud has run counters of free-space carving (filter first, carve afterwards)");
    ssm_sor_info I{};
    { const int r = sor_run(c, cl->d, cl->n, params, &I); if (r) return r; }
    if (I.n_kept < cl->n) {          // (stable: the kept points only move towards the front, but blocks run in any order, so they go through c->sor.out)
        hipStream_t s = c->main.stream;
        if (I.n_kept > 0) HIPCHK(c, hipMemcpyAsync(cl->d, c->sor.out, (size_t)I.n_kept * sizeof(ssm_point), hipMemcpyDeviceToDevice, s));
        HIPCHK(c, hipStreamSynchronize(s));
        cl->n = I.n_kept;
    }
    if (info) *info = I;
    return SSM_OK;
}
extern "C" int ssm_debug_sor_record(ssm_ctx* c, float* mean_dist, uint8_t* keep, int n)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    SorWork& W = c->sor; hipStream_t s = c->main.stream;
    if (n != W.n) FAIL(c, SSM_E_INVAL, "sor: the last call had another number of points");
    if (n == 0) return SSM_OK;
    if (mean_dist) HIPCHK(c, hipMemcpyAsync(mean_dist, W.mean_dist, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (keep) HIPCHK(c, hipMemcpyAsync(keep, W.keep, (size_t)n, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return SSM_OK;
}
extern "C" int ssm_debug_sor_levels(ssm_ctx* c, int32_t* queries, int cap, int* n_levels)
{
    if (!c || !n_levels || cap < 0 || (cap && !queries)) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    static_assert(sizeof(c->sor.level_q) / sizeof(int) == MAX_LEVELS, "one entry per level");
    *n_levels = c->sor.levels;
    for (int l = 0; l < c->sor.levels && l < cap; l++) queries[l] = c->sor.level_q[l];
    return SSM_OK;
}
