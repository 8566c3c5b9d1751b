// ssm_carve.hip -- the device path of free-space carving behind the C ABI.  DESIGN.md s.16 is the contract.  A call is one upload of the cloud table (cloud_table.h;
// the relative poses are worked out on the host by carve_core.h's rel_pose, the same 12 doubles the host function uses), the launches of kernels_carve.hip on the
// main stream, one download of the m infos and ONE wait.  The workspaces belong to the context (CarveWork; the table: CloudTableWork) and grow with the largest
// call; a cloud's run counters belong to the cloud.  The host function, the defaults and the argument check are ssm_carve_host.cpp.
#include "ssm_ctx.h"
#include "ssm_host.h"
using namespace ssm_carvec;

// the verdict / keep / scan scratch for `total` points in m clouds (the cloud table is the context's: ssm_cloud_list.hip)
static int carve_scratch(ssm_ctx* c, int total, int m)
{
    CarveWork& W = c->carve;
    if (total <= W.cap && m <= W.cap_m) return SSM_OK;
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    const size_t n = (size_t)std::max(std::max(total, W.cap), 1024), mm = (size_t)std::max(std::max(m, W.cap_m), 8), nb = (n + k_carve_block() - 1) / k_carve_block() + 1;
    W.cap = 0; W.cap_m = 0;
    DALLOC(c, W.info, mm * 8); DALLOC(c, W.h_info, mm * 8); DALLOC(c, W.base, mm + 1);
    DALLOC(c, W.block_cnt, nb); DALLOC(c, W.block_off, nb);
    DALLOC(c, W.verdict, n); DALLOC(c, W.run_new, n); DALLOC(c, W.keep, n); DALLOC(c, W.tmp_run, n); DALLOC(c, W.tmp_pts, n);
    W.tmp_bytes = k_carve_tmp_bytes((int)n); DALLOC(c, W.tmp, W.tmp_bytes);
    W.cap = (int)n; W.cap_m = (int)mm;
    return SSM_OK;
}
// the clouds of a carving call: no bound here (carve_run has the call's 2^30 with SSM_E_CAPACITY)
static CloudRule carve_cloud_rule(const char* twice_msg) { return {twice_msg, 1, INT64_MAX, nullptr, "null argument", nullptr}; }
// segs: pts, run, n and M filled by the caller; everything from the table's upload to the call's wait
static int carve_run(ssm_ctx* c, const uint16_t* d_depth, const Setup& S, int min_votes, std::vector<CloudSeg>& segs, ssm_carve_info* infos)
{
    CarveWork& W = c->carve; hipStream_t s = c->main.stream;
    const int m = (int)segs.size();
    int64_t total64 = 0;
    for (const CloudSeg& g : segs) total64 += g.n;
    if (total64 > ((int64_t)1 << 30)) FAIL(c, SSM_E_CAPACITY, "carve: more than 2^30 points in one call");
    const int total = (int)total64;
    W.off.assign(1, 0);
    { const int r = carve_scratch(c, total, m); if (r) return r; }
    CloudTable t;
    { const int r = cloud_table_upload(c, segs, k_carve_block(), &t); if (r) return r; }
    for (const CloudSeg& g : segs) W.off.push_back((int)(g.off + g.n));
    const CarveBufs B{t.seg, t.blk, W.info, W.base, W.verdict, W.run_new, W.keep, W.tmp_run, W.block_cnt, W.block_off, W.tmp_pts, W.tmp, W.tmp_bytes};
    prof_begin(c, s, "carve");
    HIPCHK(c, k_carve(d_depth, S, min_votes, m, total, B, s));
    prof_end(c, s);
    HIPCHK(c, hipMemcpyAsync(W.h_info, W.info, (size_t)m * 32, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    t.in_flight = nullptr;
    static_assert(sizeof(ssm_carve_info) == 32, "info is eight ints");
    memcpy(infos, (const int32_t*)W.h_info, (size_t)m * 32);
    return SSM_OK;
}

extern "C" int ssm_carve_view_create(ssm_ctx* c, const uint16_t* depth, int w, int h, const ssm_camera* cam, ssm_carve_view** view_out)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (!depth || !view_out) FAIL(c, SSM_E_INVAL, "null argument");
    *view_out = nullptr;
    { ssm_carve_params P; ssm_carve_params_default(&P); Setup S; const int r = carve_check(c, w, h, cam, P, &S); if (r) return r; }
    std::unique_ptr<ssm_carve_view> v(new ssm_carve_view());
    v->w = w; v->h = h; v->device = c->device; v->cam = *cam;
    DALLOC(c, v->depth, (size_t)w * h);
    HIPCHK(c, hipMemcpyAsync(v->depth, depth, (size_t)w * h * 2, hipMemcpyHostToDevice, c->main.stream));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    *view_out = v.release();
    return SSM_OK;
}
extern "C" void ssm_carve_view_free(ssm_ctx* c, ssm_carve_view* v)
{ free_after_wait(c, v); }
extern "C" int ssm_carve(ssm_ctx* c, const ssm_carve_view* v, const double* T_view, ssm_cloud* const* clouds, const double* T_clouds, int m,
                         const ssm_carve_params* params, ssm_carve_info* infos)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (!v || m < 0 || (m && (!clouds || !T_clouds))) FAIL(c, SSM_E_INVAL, "null argument");
    if (v->device != c->device) FAIL(c, SSM_E_INVAL, "view of another device");
    ssm_carve_params P; ssm_carve_params_default(&P); if (params) P = *params;
    Setup S;
    { int r = carve_check(c, v->w, v->h, &v->cam, P, &S); if (!r) r = carve_pose_check(c, T_view); if (r) return r; }
    std::vector<CloudSeg> segs; int64_t total = 0;
    { const int r = cloud_call(c, cloud_handles(clouds, T_clouds, m), carve_cloud_rule("carve: the same cloud twice in one call"), T_view, segs, &total); if (r) return r; }
    c->carve.off.assign(1, 0);
    if (m == 0) return SSM_OK;
    // a cloud's counters are made by its first view, zero; they become the cloud's only when the whole call has succeeded (a cloud that has counters is refused by
    // ssm_cloud_sor, so a failed call must not leave any behind)
    std::vector<DevBuf<uint8_t>> fresh((size_t)m);
    for (int k = 0; k < m; k++) {
        ssm_cloud* cl = clouds[k];
        if (!cl->run) {
            DALLOC(c, fresh[k], std::max(cl->n, 1));
            HIPCHK(c, hipMemsetAsync(fresh[k], 0, (size_t)std::max(cl->n, 1), c->main.stream));
        }
        segs[k].run = cl->run ? (uint8_t*)cl->run : (uint8_t*)fresh[k];
    }
    std::vector<ssm_carve_info> I((size_t)m);
    {
        const int r = carve_run(c, v->depth, S, P.min_votes, segs, I.data());
        if (r) { hipStreamSynchronize(c->main.stream); return r; }          // (the fresh counters are freed on return: nothing queued may still touch them)
    }
    for (int k = 0; k < m; k++) { if (!clouds[k]->run) clouds[k]->run = std::move(fresh[k]); clouds[k]->n = I[k].n_kept; }
    if (infos) memcpy(infos, I.data(), (size_t)m * sizeof(ssm_carve_info));
    return SSM_OK;
}
extern "C" int ssm_carve_points(ssm_ctx* c, const uint16_t* depth, int w, int h, const ssm_camera* cam, const double* T_view, const ssm_point* pts, int n,
                                const double* T_cloud, uint8_t* run_inout, const ssm_carve_params* params, ssm_point* out, int cap, int* n_out, ssm_carve_info* info)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    ssm_carve_params P; ssm_carve_params_default(&P); if (params) P = *params;
    Setup S;
    { const int r = carve_check(c, w, h, cam, P, &S); if (r) return r; }
    if (!depth || !n_out || n < 0 || (n && !pts) || cap < 0) FAIL(c, SSM_E_INVAL, "null argument");
    { int r = carve_pose_check(c, T_view); if (!r) r = carve_pose_check(c, T_cloud); if (r) return r; }
    *n_out = 0;
    CarveWork& W = c->carve; hipStream_t s = c->main.stream;
    const size_t np = (size_t)w * h, nn = (size_t)std::max(n, 1);
    if (np > W.depth_cap || nn > W.run_cap) HIPCHK(c, hipStreamSynchronize(s));
    if (np > W.depth_cap) { W.depth_cap = 0; DALLOC(c, W.depth, np); W.depth_cap = np; }
    if (nn > W.run_cap) { W.run_cap = 0; DALLOC(c, W.run_in, nn); W.run_cap = nn; }
    HIPCHK(c, hipMemcpyAsync(W.depth, depth, np * 2, hipMemcpyHostToDevice, s));
    if (n && run_inout) HIPCHK(c, hipMemcpyAsync(W.run_in, run_inout, (size_t)n, hipMemcpyHostToDevice, s));
    else HIPCHK(c, hipMemsetAsync(W.run_in, 0, nn, s));
    std::vector<CloudSeg> segs; int64_t total = 0;          // the one cloud, staged like any list of host arrays
    { const int r = cloud_call(c, cloud_arrays(&pts, &n, T_cloud, 1), carve_cloud_rule(nullptr), T_view, segs, &total); if (r) return r; }
    segs[0].run = W.run_in;
    ssm_carve_info I{};
    { const int r = carve_run(c, W.depth, S, P.min_votes, segs, &I); if (r) return r; }
    *n_out = I.n_kept;
    if (info) *info = I;
    if (I.n_kept > cap) FAIL(c, SSM_E_CAPACITY, "point buffer too small (need " + std::to_string(I.n_kept) + ")");
    if (I.n_kept == 0) return SSM_OK;
    if (!out) FAIL(c, SSM_E_INVAL, "null argument");
    HIPCHK(c, hipMemcpyAsync(out, c->clouds.in, (size_t)I.n_kept * sizeof(ssm_point), hipMemcpyDeviceToHost, s));
    if (run_inout) HIPCHK(c, hipMemcpyAsync(run_inout, W.run_in, (size_t)I.n_kept, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return SSM_OK;
}
extern "C" int ssm_debug_carve_record(ssm_ctx* c, int k, uint8_t* verdict, uint8_t* run, int n)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    CarveWork& W = c->carve; hipStream_t s = c->main.stream;
    if (k < 0 || k + 1 >= (int)W.off.size()) FAIL(c, SSM_E_INVAL, "carve: the last call had no such cloud");
    if (n != W.off[k + 1] - W.off[k]) FAIL(c, SSM_E_INVAL, "carve: the cloud had another number of points in the last call");
    if (n == 0) return SSM_OK;
    if (verdict) HIPCHK(c, hipMemcpyAsync(verdict, W.verdict + W.off[k], (size_t)n, hipMemcpyDeviceToHost, s));
    if (run) HIPCHK(c, hipMemcpyAsync(run, W.run_new + W.off[k], (size_t)n, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return SSM_OK;
}
extern "C" int ssm_cloud_run_fetch(ssm_ctx* c, const ssm_cloud* cl, uint8_t* run, int cap)
{
    if (!c || !cl) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (cl->n > cap) FAIL(c, SSM_E_CAPACITY, "counter buffer too small (need " + std::to_string(cl->n) + ")");
    if (cl->n == 0) return SSM_OK;
    if (!run) FAIL(c, SSM_E_INVAL, "null argument");
    if (!cl->run) { memset(run, 0, (size_t)cl->n); return SSM_OK; }
    HIPCHK(c, hipMemcpyAsync(run, cl->run, (size_t)cl->n, hipMemcpyDeviceToHost, c->main.stream));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    return SSM_OK;
}
