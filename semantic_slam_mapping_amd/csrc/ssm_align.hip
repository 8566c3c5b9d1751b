// ssm_align.hip -- the device path of dense alignment behind the C ABI.  DESIGN.md s.18 is the contract.  A view is one upload of the depth image and one launch
// for its normal map.  An alignment is one upload of the cloud table (cloud_table.h; the relative poses are worked out on the host by carve_core.h's rel_pose,
// the same 12 doubles the host function uses) and one clear of the sums' slots; then every iteration is ONE launch of kernels_align.hip on the main stream (E
// travels as a kernel argument), one download of its slot of 30 integers and one wait.  The solve and the stopping rules are align_drive of ssm_align_host.cpp,
// the same function the host path runs.  The slots belong to the context (AlignWork), and so do the table and the staging of the host-array call
// (CloudTableWork), which grow with the largest call.
#include "ssm_ctx.h"
#include "ssm_host.h"
using namespace ssm_alignc;

enum { SLOT = 32 };          // 64-bit words per iteration's slot (NSUM of them used)

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
static int align_run(ssm_ctx* c, const ssm_align_view* v, const Setup& S, const ssm_align_params& P, const double* T_view, std::vector<CloudSeg>& segs,
                     double* T_view_out, ssm_align_info* info)
{
    AlignWork& W = c->align; hipStream_t s = c->main.stream;
    W.record.clear();
    if (!W.sums) { DALLOC(c, W.h_sums, (size_t)MAX_ITERATIONS * SLOT); DALLOC(c, W.sums, (size_t)MAX_ITERATIONS * SLOT); }
    CloudTable t;
    { const int r = cloud_table_upload(c, segs, k_align_block(), &t); if (r) return r; }
    HIPCHK(c, hipMemsetAsync(W.sums, 0, (size_t)P.max_iterations * SLOT * 8, s));
    int it = 0, hip_rc = SSM_OK;
    // (every iteration ends with a wait, and there is at least one: a return of align_drive without an error leaves nothing in flight)
    const int r = align_drive(P, t.total, T_view, [&](const double* E, int64_t* sums) -> int {
        unsigned long long* slot = W.sums + (size_t)it * SLOT; unsigned long long* h_slot = W.h_sums + (size_t)it * SLOT;
        it++;
        prof_begin(c, s, "align_accumulate");
        hipError_t e = k_align_accumulate(S, E, t.seg, t.blk, t.total, v->depth, v->normals, slot, s);
        prof_end(c, s);
        if (e == hipSuccess) e = hipMemcpyAsync(h_slot, slot, NSUM * 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { c->err = std::string("align: ") + hipGetErrorString(e); hip_rc = SSM_E_HIP; return SSM_E_HIP; }
        memcpy(sums, h_slot, NSUM * 8);
        return SSM_OK;
    }, T_view_out, info, &W.record);
    if (r == SSM_OK) t.in_flight = nullptr;
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
{ free_after_wait(c, v); }
extern "C" int ssm_align_points(ssm_ctx* c, const ssm_align_view* v, const double* T_view, const ssm_point* const* pts, const int32_t* n, const double* T_clouds, int m,
                                const ssm_align_params* params, double* T_view_out, ssm_align_info* info)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    ssm_align_params P; Setup S;
    { const int r = align_begin(c, v, T_view, params, &P, &S); if (r) return r; }
    std::vector<CloudSeg> segs; int64_t total = 0;
    { const int r = cloud_call(c, cloud_arrays(pts, n, T_clouds, m), align_cloud_rule(S, P.stride), T_view, segs, &total); if (r) return r; }
    return align_run(c, v, S, P, T_view, segs, T_view_out, info);
}
extern "C" int ssm_align_clouds(ssm_ctx* c, const ssm_align_view* v, const double* T_view, ssm_cloud* const* clouds, const double* T_clouds, int m,
                                const ssm_align_params* params, double* T_view_out, ssm_align_info* info)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    ssm_align_params P; Setup S;
    { const int r = align_begin(c, v, T_view, params, &P, &S); if (r) return r; }
    std::vector<CloudSeg> segs; int64_t total = 0;
    { const int r = cloud_call(c, cloud_handles(clouds, T_clouds, m), align_cloud_rule(S, P.stride), T_view, segs, &total); if (r) return r; }
    return align_run(c, v, S, P, T_view, segs, T_view_out, info);
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
