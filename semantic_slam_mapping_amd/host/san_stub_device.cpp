// san_stub_device.cpp -- TEST INFRASTRUCTURE for the CPU sanitizer builds of the host layer (make SAN=asan|ubsan|tsan): a stand-in for the handful of
// libssm_hip.so entry points that Mapper / PoseGraph reach, so that the THREADING of the host classes (Mapper::viewer on its own thread against the main
// thread's tryInsertKeyFrame: the place of the reference's unlocked reads, /root/reference/src/mapper.cpp:114-136) can run under ThreadSanitizer in the
// build container, which has no GPU and where sanitizer runtimes and the HIP runtime do not mix.  It computes nothing of the product: the numbers it
// returns are placeholders.  It is linked into test_threads / test_pnp / test_png of a SAN build ONLY -- never into exp_mapping or the library.
#include "ssm_hip.h"
#include "ssm/pnp_core.h"
#include "ssm/looper_core.h"
#include <cstring>
#include <string>
#include <vector>
struct ssm_ctx { ssm_config cfg; std::string err; };
// the looper's vocabulary is host code: the library's own implementation runs under the sanitizers (test_looper).  The device looper is never reached there
// (Looper takes the host path on a thread without a context); its entry points only have to link
static thread_local std::string g_vocab_err;
static int vocab_fail(const std::string& msg) { g_vocab_err = msg; return SSM_E_INVAL; }
#include "../csrc/ssm_vocab.inc"
// likewise the U/V-disparity stage: UVDisparity::Process takes ssm_uvd_process_host on a thread without a context, and that is the library's own host pipeline
// (csrc/ssm_uvd_host.inc over include/ssm/uvd_core.h), which so runs under the sanitizers (test_uvd); the device entry points only have to link
#include "ssm/uvd_core.h"
#include <algorithm>
#include <climits>
#include <cmath>
#include "../csrc/ssm_uvd_host.inc"
// and the pose-graph optimiser: PoseGraph without a context uses ssm_pgo_optimize_host, the library's own host function (csrc/ssm_pgo.hip over
// include/ssm/pgo_core.h), built here without its device half
#define SSM_PGO_HOST_ONLY
static thread_local std::string g_create_err;
#include "../csrc/ssm_pgo.hip"
struct ssm_uvd { ssm_uvd_params p; UvdKalman kf1, kf2; double rate[ssm_uvdc::MAX_BINS]; UvdFrame frame; };
extern "C" {
void ssm_uvd_params_default(ssm_uvd_params* p) { if (p) uvd_set_defaults(p); }
int ssm_uvd_create(ssm_ctx* c, const ssm_uvd_params* params, ssm_uvd** out)
{
    if (!out || !params) return SSM_E_INVAL;
    if (c) { *out = nullptr; return SSM_E_NODEVICE; }
    ssm_uvd* u = new ssm_uvd(); u->p = *params; uvd_rate_table(u->rate); *out = u;
    return SSM_OK;
}
void ssm_uvd_destroy(ssm_uvd* u) { delete u; }
int ssm_uvd_reset(ssm_uvd* u) { if (!u) return SSM_E_INVAL; u->kf1 = UvdKalman(); u->kf2 = UvdKalman(); return SSM_OK; }
int ssm_uvd_process_host(ssm_uvd* u, const uint8_t* left, const int16_t* disp, int w, int h, int stride, ssm_pmatch* matches, uint8_t* inlier_flags, int n_matches,
                         uint8_t* moving, uint8_t* roi, uint8_t* ground, ssm_uvd_info* info)
{
    if (!u) return SSM_E_INVAL;
    return uvd_process_host(u->p, u->rate, u->kf1, u->kf2, u->frame, left, disp, w, h, stride, matches, inlier_flags, n_matches, moving, roi, ground, info, false);
}
int ssm_debug_uvd_record(ssm_uvd*, int) { return SSM_OK; }
int ssm_debug_uvd_times(ssm_uvd*, double*) { return SSM_E_NODEVICE; }
int ssm_vo_estimate(ssm_ctx*, const ssm_pmatch*, int, const ssm_vo_params*, const int32_t*, int, double*, int32_t*, int, int*, int*) { return SSM_E_NODEVICE; }      // (VisualOdometryStereo has to link: test_uvd fills its lists by hand)
int ssm_uvd_process(ssm_uvd*, const uint8_t*, const int16_t*, int, int, int, ssm_pmatch*, uint8_t*, int, uint8_t*, uint8_t*, uint8_t*, ssm_uvd_info*) { return SSM_E_NODEVICE; }
int ssm_uvd_process_dev(ssm_uvd*, const uint8_t*, const int16_t*, int, int, int, ssm_pmatch*, const int32_t*, uint8_t*, int, uint8_t*, uint8_t*, uint8_t*, ssm_uvd_info*) { return SSM_E_NODEVICE; }
// PoseGraph::step reaches the extractor and the matcher through solvePnPLazy; test_posegraph --graph-only never gets there (no neighbours, no looper): they only have to link
int ssm_orb_extract(ssm_ctx*, const uint8_t*, int, int, int, int, const uint16_t*, ssm_keypoint*, uint8_t*, float*, int, int*) { return SSM_E_NODEVICE; }
int ssm_match(ssm_ctx*, const uint8_t*, int, const uint8_t*, int, double, ssm_dmatch*, int, int*) { return SSM_E_NODEVICE; }
int ssm_looper_create(ssm_ctx*, const ssm_vocab*, ssm_looper**) { return SSM_E_NODEVICE; }
void ssm_looper_destroy(ssm_looper*) {}
int ssm_looper_size(const ssm_looper*) { return 0; }
int ssm_looper_add(ssm_looper*, const uint8_t*, int, int) { return SSM_E_NODEVICE; }
int ssm_looper_bow(ssm_looper*, int, int32_t*, double*, int, int*) { return SSM_E_NODEVICE; }
int ssm_looper_scores(ssm_looper*, int, int, double*) { return SSM_E_NODEVICE; }
void ssm_config_default(ssm_config* c) { memset(c, 0, sizeof(*c)); c->width = 640; c->height = 480; c->orb_features = 1000; c->orb_scale = 1.2f; c->orb_levels = 8;
    c->orb_iniThFAST = 20; c->orb_minThFAST = 7; c->knn_match_ratio = 0.8; c->tracker_ref_frames = 5; c->mapper_resolution = 0.1; c->mapper_max_distance = 40;
    c->camera.cx = 318.6; c->camera.cy = 255.3; c->camera.fx = 517.3; c->camera.fy = 516.5; c->camera.scale = 1000.0; c->max_batch = 1; c->voxel_capacity_log2 = 16; }
int ssm_create(int, const ssm_config* cfg, ssm_ctx** out) { *out = new ssm_ctx(); (*out)->cfg = *cfg; return SSM_OK; }
void ssm_destroy(ssm_ctx* c) { delete c; }
const char* ssm_last_error(const ssm_ctx* c) { return c ? c->err.c_str() : (g_vocab_err.empty() ? "stub" : g_vocab_err.c_str()); }
int ssm_orb_capacity(const ssm_ctx*) { return 1024; }
int ssm_backproject(ssm_ctx*, const uint16_t* depth, const uint8_t* rgb, const uint8_t*, int w, int h, const ssm_camera*, const double*, double, ssm_point* out, int cap, int* n_out)
{
    int n = 0;
    for (int v = 0; v < h; v += 4) for (int u = 0; u < w; u += 4) {
        const uint16_t d = depth[(size_t)v * w + u];
        if (!d || n >= cap) continue;
        ssm_point p; memset(&p, 0, sizeof(p)); p.x = u * 0.01f; p.y = v * 0.01f; p.z = d * 0.001f; p.w = 1.f; p.b = rgb[((size_t)v * w + u) * 3]; p.label = 255;
        out[n++] = p;
    }
    *n_out = n; return SSM_OK;
}
// PnPSolver::solvePnP goes to the device block whenever its thread has a context (include/ssm/pnp.h): under the sanitizers the same contract arithmetic
// (pnp_core.h) runs on the host in its place
int ssm_pnp_solve(ssm_ctx*, const float* img, const float* obj, int n, const double cam[4], int min_inliers, double T[16], uint8_t* inliers, int* n_inliers, int* success)
{
    if (n < 0 || n > 65535) return SSM_E_CAPACITY;
    ssm_pnp::Camera c; c.fx = cam[0]; c.fy = cam[1]; c.cx = cam[2]; c.cy = cam[3];
    std::vector<ssm_pnp::Edge> edges((size_t)n + 1); std::vector<unsigned char> inl((size_t)n + 1);
    int ok = 0;
    ssm_pnp::solve(img, obj, n, c, min_inliers, T, inl.data(), edges.data(), &ok);
    int m = 0;
    for (int i = 0; i < n; i++) { if (inliers) inliers[i] = inl[i]; m += inl[i] != 0; }
    if (n_inliers) *n_inliers = m;
    if (success) *success = ok;
    return SSM_OK;
}
// device-resident Mapper entry points: a "cloud" is a host vector here, the map update the same placeholder thinning as ssm_voxel_filter below
struct ssm_cloud { std::vector<ssm_point> p; };
static std::vector<ssm_point> g_vmap;
int ssm_backproject_dev(ssm_ctx* c, const uint16_t* depth, const uint8_t* rgb, const uint8_t* sem, int w, int h, const ssm_camera* cam, double md, ssm_cloud** out)
{
    ssm_cloud* cl = new ssm_cloud(); cl->p.resize((size_t)w * h / 16 + 1); int n = 0;
    ssm_backproject(c, depth, rgb, sem, w, h, cam, nullptr, md, cl->p.data(), (int)cl->p.size(), &n);
    cl->p.resize(n); *out = cl; return SSM_OK;
}
int ssm_cloud_size(const ssm_cloud* cl) { return cl ? (int)cl->p.size() : 0; }
void ssm_cloud_free(ssm_ctx*, ssm_cloud* cl) { delete cl; }
int ssm_cloud_fetch(ssm_ctx*, const ssm_cloud* cl, const double*, ssm_point* out, int cap, int* n_out)
{ *n_out = (int)cl->p.size(); if (*n_out > cap) return SSM_E_CAPACITY; memcpy(out, cl->p.data(), cl->p.size() * sizeof(ssm_point)); return SSM_OK; }
int ssm_viewer_map_update(ssm_ctx*, int rebuild, ssm_cloud* const* clouds, const double*, int n, float, int* n_out)
{
    std::vector<ssm_point> all; if (!rebuild) all = g_vmap;
    for (int i = 0; i < n; i++) all.insert(all.end(), clouds[i]->p.begin(), clouds[i]->p.end());
    g_vmap.clear();
    for (size_t i = 0; i < all.size(); i += 3) g_vmap.push_back(all[i]);
    if (n_out) *n_out = (int)g_vmap.size();
    return SSM_OK;
}
int ssm_viewer_map_release(ssm_ctx*, int) { return SSM_OK; }
int ssm_host_alloc(size_t bytes, void** out) { *out = malloc(bytes ? bytes : 1); return *out ? SSM_OK : SSM_E_NOMEM; }
int ssm_host_free(void* p) { free(p); return SSM_OK; }
int ssm_viewer_map_fetch(ssm_ctx*, ssm_point* out, int cap, int* n_out)
{ *n_out = (int)g_vmap.size(); if (*n_out > cap) return SSM_E_CAPACITY; if (*n_out) memcpy(out, g_vmap.data(), g_vmap.size() * sizeof(ssm_point)); return SSM_OK; }
int ssm_voxel_filter(ssm_ctx*, const ssm_point* pts, int n, float, ssm_point* out, int cap, int* n_out)
{
    int m = 0;
    for (int i = 0; i < n && m < cap; i += 3) out[m++] = pts[i];
    *n_out = m; return SSM_OK;
}
}
