// ssm_align.hip -- the device path of dense alignment behind the C ABI.  DESIGN.md s.18 is the contract.  A view is one upload of the depth image and one launch
// for its normal map.  An alignment is one upload of a small table (the clouds' pointers, sizes, strides and relative poses -- worked out on the host by
// carve_core.h's rel_pose, the same 12 doubles the host function uses -- and each chunk's first cloud) and one clear of the sums' slots; then every iteration is
// ONE launch of kernels_align.hip on the main stream (E travels as a kernel argument), one download of its slot of 30 integers and one wait.  The solve and the
// stopping rules are align_drive of ssm_align_host.cpp, the same function the host path runs.  The table, the slots and the staging of the host-array call
// belong to the context (AlignWork) and grow with the largest call.
#include "ssm_ctx.h"
#include "ssm_host.h"
using namespace ssm_alignc;

enum { SLOT = 32 };          // 64-bit words per iteration's slot (NSUM of them used)

static int align_reserve(ssm_ctx* c, size_t m, size_t nb)
{
    AlignWork& W = c->align;
    if (m <= W.cap_m && nb <= W.cap_b && W.sums) return SSM_OK;
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    const size_t mm = std::max(std::max(m, W.cap_m), (size_t)8), bb = std::max(std::max(nb, W.cap_b), (size_t)1024);
    W.cap_m = 0; W.cap_b = 0;
    const size_t bytes = mm * sizeof(AlignSeg) + bb * 4;
    DALLOC(c, W.table, bytes); DALLOC(c, W.h_table, bytes);
    DALLOC(c, W.sums, (size_t)MAX_ITERATIONS * SLOT); DALLOC(c, W.h_sums, (size_t)MAX_ITERATIONS * SLOT);
    W.cap_m = mm; W.cap_b = bb;
    return SSM_OK;
}
// what every alignment call checks first
static int align_begin(ssm_ctx* c, const ssm_align_view* v, const double* T_view, const ssm_align_params* params, ssm_align_params* P, Setup* S)
{
    if (!v) FAIL(c, SSM_E_INVAL, "null argument");
    if (v->device != c->device) FAIL(c, SSM_E_INVAL, "view of another device");
    ssm_align_params_default(P); if (params) *P = *params;
    P->tol_abs = v->tol_abs; P->tol_rel_ppm = v->tol_rel_ppm;          // the edge gate is the view's
    int r = align_check(c, v->w, v->h, &v->cam, *P, S); if (!r) r = carve_pose_check(c, T_view);
    return r;
}
// segs: pts, n (points used), stride and M filled by the caller; everything from the table's upload to the last iteration's wait
static int align_run(ssm_ctx* c, const ssm_align_view* v, const Setup& S, const ssm_align_params& P, const double* T_view, std::vector<AlignSeg>& segs, int64_t total,
                     double* T_view_out, ssm_align_info* info)
{
    AlignWork& W = c->align; hipStream_t s = c->main.stream;
    const int m = (int)segs.size();
    const int64_t T = k_align_block(), nb = (total + T - 1) / T;
    W.record.clear();
    { const int r = align_reserve(c, (size_t)m, (size_t)nb); if (r) return r; }
    AlignSeg* hs = reinterpret_cast<AlignSeg*>((uint8_t*)W.h_table);
    int32_t* hb = reinterpret_cast<int32_t*>((uint8_t*)W.h_table + (size_t)m * sizeof(AlignSeg));
    int64_t at = 0;
    for (int k = 0; k < m; k++) { segs[k].off = at; hs[k] = segs[k]; at += segs[k].n; }
    for (int64_t b = 0, k = 0; b < nb; b++) { while (b * T >= segs[k].off + segs[k].n) k++; hb[b] = (int32_t)k; }
    const size_t bytes = (size_t)m * sizeof(AlignSeg) + (size_t)nb * 4;
    if (bytes) HIPCHK(c, hipMemcpyAsync(W.table, W.h_table, bytes, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemsetAsync(W.sums, 0, (size_t)P.max_iterations * SLOT * 8, s));
    const AlignSeg* d_seg = W.table.as<AlignSeg>();
    const int32_t* d_blk = reinterpret_cast<const int32_t*>((uint8_t*)W.table + (size_t)m * sizeof(AlignSeg));
    int it = 0, hip_rc = SSM_OK;
    const int r = align_drive(P, total, T_view, [&](const double* E, int64_t* sums) -> int {
        unsigned long long* slot = W.sums + (size_t)it * SLOT; unsigned long long* h_slot = W.h_sums + (size_t)it * SLOT;
        it++;
        prof_begin(c, s, "align_accumulate");
        hipError_t e = k_align_accumulate(S, E, d_seg, d_blk, total, v->depth, v->normals, slot, s);
        prof_end(c, s);
        if (e == hipSuccess) e = hipMemcpyAsync(h_slot, slot, NSUM * 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { c->err = std::string("align: ") + hipGetErrorString(e); hip_rc = SSM_E_HIP; return SSM_E_HIP; }
        memcpy(sums, h_slot, NSUM * 8);
        return SSM_OK;
    }, T_view_out, info, &W.record);
    return r ? (hip_rc ? hip_rc : r) : SSM_OK;
}

extern "C" int ssm_align_view_create(ssm_ctx* c, const uint16_t* depth, int w, int h, const ssm_camera* cam, const ssm_align_params* params, ssm_align_view** view_out)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (!depth || !view_out) FAIL(c, SSM_E_INVAL, "null argument");
    *view_out = nullptr;
    ssm_align_params P; ssm_align_params_default(&P); if (params) P = *params;
    Setup S;
    { const int r = align_check(c, w, h, cam, P, &S); if (r) return r; }
    std::unique_ptr<ssm_align_view> v(new ssm_align_view());
    v->w = w; v->h = h; v->device = c->device; v->cam = *cam; v->tol_abs = P.tol_abs; v->tol_rel_ppm = P.tol_rel_ppm;
    const size_t np = (size_t)w * h;
    DALLOC(c, v->depth, np); DALLOC(c, v->normals, np * sizeof(Normal));
    hipStream_t s = c->main.stream;
    HIPCHK(c, hipMemcpyAsync(v->depth, depth, np * 2, hipMemcpyHostToDevice, s));
    prof_begin(c, s, "align_normals");
    HIPCHK(c, k_align_normals(v->depth, S, v->normals, s));
    prof_end(c, s);
    HIPCHK(c, hipStreamSynchronize(s));
    *view_out = v.release();
    return SSM_OK;
}
extern "C" void ssm_align_view_free(ssm_ctx* c, ssm_align_view* v)
{
    if (!v) return;
    if (c) { std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device); hipStreamSynchronize(c->main.stream); }
    delete v;
}
extern "C" int ssm_align_points(ssm_ctx* c, const ssm_align_view* v, const double* T_view, const ssm_point* const* pts, const int32_t* n, const double* T_clouds, int m,
                                const ssm_align_params* params, double* T_view_out, ssm_align_info* info)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    ssm_align_params P; Setup S;
    { const int r = align_begin(c, v, T_view, params, &P, &S); if (r) return r; }
    if (m < 0 || (m && (!pts || !n || !T_clouds))) FAIL(c, SSM_E_INVAL, "null argument");
    int64_t total = 0, raw = 0;
    { const int r = align_total_check(c, S, n, m, P.stride, &total); if (r) return r; }
    std::vector<AlignSeg> segs((size_t)m);
    for (int k = 0; k < m; k++) {
        if (n[k] && !pts[k]) FAIL(c, SSM_E_INVAL, "null argument");
        for (int j = 0; j < k; j++) if (n[k] && n[j] && pts[j] == pts[k]) FAIL(c, SSM_E_INVAL, "align: the same cloud twice");
        { const int r = carve_pose_check(c, T_clouds + 16 * k); if (r) return r; }
        ssm_carvec::rel_pose(T_view, T_clouds + 16 * k, segs[k].M);
        raw += n[k];
    }
    AlignWork& W = c->align; hipStream_t s = c->main.stream;
    const size_t nn = (size_t)std::max<int64_t>(raw, 1);
    if (nn > W.in_cap) { HIPCHK(c, hipStreamSynchronize(s)); W.in_cap = 0; DALLOC(c, W.in, nn); W.in_cap = nn; }
    size_t at = 0;
    for (int k = 0; k < m; k++) {
        if (n[k]) HIPCHK(c, hipMemcpyAsync(W.in + at, pts[k], (size_t)n[k] * sizeof(ssm_point), hipMemcpyHostToDevice, s));
        segs[k].pts = W.in + at; segs[k].n = (int32_t)(((int64_t)n[k] + P.stride - 1) / P.stride); segs[k].stride = P.stride; at += (size_t)n[k];
    }
    return align_run(c, v, S, P, T_view, segs, total, T_view_out, info);
}
extern "C" int ssm_align_clouds(ssm_ctx* c, const ssm_align_view* v, const double* T_view, ssm_cloud* const* clouds, const double* T_clouds, int m,
                                const ssm_align_params* params, double* T_view_out, ssm_align_info* info)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    ssm_align_params P; Setup S;
    { const int r = align_begin(c, v, T_view, params, &P, &S); if (r) return r; }
    if (m < 0 || (m && (!clouds || !T_clouds))) FAIL(c, SSM_E_INVAL, "null argument");
    std::vector<AlignSeg> segs((size_t)m);
    std::vector<int32_t> n((size_t)m);
    for (int k = 0; k < m; k++) {
        const ssm_cloud* cl = clouds[k];
        if (!cl) FAIL(c, SSM_E_INVAL, "null argument");
        if (cl->device != c->device) FAIL(c, SSM_E_INVAL, "cloud of another device");
        for (int j = 0; j < k; j++) if (clouds[j] == cl) FAIL(c, SSM_E_INVAL, "align: the same cloud twice");
        { const int r = carve_pose_check(c, T_clouds + 16 * k); if (r) return r; }
        ssm_carvec::rel_pose(T_view, T_clouds + 16 * k, segs[k].M);
        n[k] = cl->n;
        segs[k].pts = cl->d; segs[k].n = (int32_t)(((int64_t)cl->n + P.stride - 1) / P.stride); segs[k].stride = P.stride;
    }
    int64_t total = 0;
    { const int r = align_total_check(c, S, n.data(), m, P.stride, &total); if (r) return r; }
    return align_run(c, v, S, P, T_view, segs, total, T_view_out, info);
}
extern "C" int ssm_debug_align_normals(ssm_ctx* c, const ssm_align_view* v, uint8_t* valid, float* normals)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (!v) FAIL(c, SSM_E_INVAL, "null argument");
    if (v->device != c->device) FAIL(c, SSM_E_INVAL, "view of another device");
    const size_t np = (size_t)v->w * v->h;
    std::vector<Normal> nm(np);
    HIPCHK(c, hipMemcpyAsync(nm.data(), v->normals, np * sizeof(Normal), hipMemcpyDeviceToHost, c->main.stream));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    if (normals) memcpy(normals, nm.data(), np * sizeof(Normal));
    if (valid) for (size_t i = 0; i < np; i++) valid[i] = (nm[i].x != 0.0f || nm[i].y != 0.0f || nm[i].z != 0.0f) ? 1 : 0;
    return SSM_OK;
}
extern "C" int ssm_debug_align_record(ssm_ctx* c, ssm_align_iter* record, int cap, int* n_record)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    const AlignWork& W = c->align;
    if (!n_record || cap < 0) FAIL(c, SSM_E_INVAL, "null argument");
    *n_record = (int)W.record.size();
    if (!record) return SSM_OK;
    if ((int)W.record.size() > cap) FAIL(c, SSM_E_CAPACITY, "record buffer too small (need " + std::to_string(W.record.size()) + ")");
    if (!W.record.empty()) memcpy(record, W.record.data(), W.record.size() * sizeof(ssm_align_iter));
    return SSM_OK;
}
