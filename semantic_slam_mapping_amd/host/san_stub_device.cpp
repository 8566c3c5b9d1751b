// san_stub_device.cpp -- TEST INFRASTRUCTURE for the CPU sanitizer builds of the host layer (make SAN=asan|ubsan|tsan): a stand-in for the side of libssm_hip.so
// that owns the context and the device, so that the THREADING of the host classes (Mapper::viewer on its own thread against the main thread's
// tryInsertKeyFrame: the place of the reference's unlocked reads, /root/reference/src/mapper.cpp:114-136) can run under ThreadSanitizer in the build container,
// which has no GPU and where sanitizer runtimes and the HIP runtime do not mix.  The library's host-only sources (the list of csrc/host_sources.mk without
// the ORB planner) are compiled beside it as they are -- the sanitizers see the shipped code -- and get the
// "no device" form of csrc/ssm_host.h's hooks here (the bulk tracker's among them: no tracker is ever created on the stub; its state machine runs under the sanitizers
// in host/test_track.cpp, over hooks of that program's own).  The device entry points compute nothing of the product: placeholders.  Linked into the programs of a SAN build ONLY.
#include "ssm_hip.h"
#include "ssm/pnp_core.h"
#include <cstring>
#include <mutex>
#include <string>
#include <vector>
struct ssm_ctx { ssm_config cfg; std::string err; };
static thread_local std::string g_create_err;
int host_fail(ssm_ctx* c, int code, const std::string& msg) { if (c) c->err = msg; else g_create_err = msg; return code; }
std::unique_lock<std::mutex> host_lock(ssm_ctx*) { return {}; }
namespace ssm_pgc { struct View; }
int uvd_dev_attach(ssm_uvd*) { return SSM_E_NODEVICE; }
void uvd_dev_release(ssm_uvd*) {}
int pgo_dev_attach(ssm_pgo*) { return SSM_E_NODEVICE; }
void pgo_dev_release(ssm_pgo*) {}
int pgo_dev_optimize(ssm_pgo**, int, const ssm_pgc::View*, int) { return SSM_E_NODEVICE; }
int pgo_dev_linearize(ssm_pgo*, const ssm_pgc::View&) { return SSM_E_NODEVICE; }
int pgo_dev_factor_solve(ssm_pgo*, ssm_pgo&, const ssm_pgc::View&, double) { return SSM_E_NODEVICE; }
struct PnpState;
int track_dev_attach(ssm_tracker*) { return SSM_E_NODEVICE; }
void track_dev_release(ssm_tracker*) {}
int track_dev_run(ssm_tracker*, const ssm_seq_out_dev*, int, int, PnpState*, double*, std::vector<ssm_track_info>&) { return SSM_E_NODEVICE; }
extern "C" {
int ssm_sync(ssm_ctx*) { return SSM_E_NODEVICE; }                    // (the bulk tracker's downloads: never reached, see above)
int ssm_memcpy_d2h(ssm_ctx*, void*, const void*, size_t) { return SSM_E_NODEVICE; }
// the device entry points of the stages whose host halves are linked in: never reached (the host classes take the host path on a thread without a context)
int ssm_vo_estimate(ssm_ctx*, const ssm_pmatch*, int, const ssm_vo_params*, const int32_t*, int, double*, int32_t*, int, int*, int*) { return SSM_E_NODEVICE; }      // (VisualOdometryStereo has to link: test_uvd fills its lists by hand)
int ssm_uvd_process(ssm_uvd*, const uint8_t*, const int16_t*, int, int, int, ssm_pmatch*, uint8_t*, int, uint8_t*, uint8_t*, uint8_t*, ssm_uvd_info*) { return SSM_E_NODEVICE; }
int ssm_uvd_process_dev(ssm_uvd*, const uint8_t*, const int16_t*, int, int, int, ssm_pmatch*, const int32_t*, uint8_t*, int, uint8_t*, uint8_t*, uint8_t*, ssm_uvd_info*) { return SSM_E_NODEVICE; }
// PoseGraph::step reaches the extractor and the matcher through solvePnPLazy; test_posegraph --graph-only never gets there (no neighbours, no looper): they only have to link
int ssm_orb_extract(ssm_ctx*, const uint8_t*, int, int, int, int, const uint16_t*, ssm_keypoint*, uint8_t*, float*, int, int*) { return SSM_E_NODEVICE; }
int ssm_match(ssm_ctx*, const uint8_t*, int, const uint8_t*, int, double, ssm_dmatch*, int, int*) { return SSM_E_NODEVICE; }
int ssm_debug_orb_octree(ssm_ctx*, int, const int32_t*, const uint32_t*, const int32_t*, int32_t*, int32_t*, uint32_t*, int32_t*, uint16_t*) { return SSM_E_NODEVICE; }      // (a test hook of the device library: no device here)
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
const char* ssm_last_error(const ssm_ctx* c) { return c ? c->err.c_str() : (g_create_err.empty() ? "stub" : g_create_err.c_str()); }
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
struct ssm_cloud { std::vector<ssm_point> p; std::vector<uint8_t> run; };
static std::vector<ssm_point> g_vmap;
int ssm_backproject_dev(ssm_ctx* c, const uint16_t* depth, const uint8_t* rgb, const uint8_t* sem, int w, int h, const ssm_camera* cam, double md, ssm_cloud** out)
{
    ssm_cloud* cl = new ssm_cloud(); cl->p.resize((size_t)w * h / 16 + 1); int n = 0;
    ssm_backproject(c, depth, rgb, sem, w, h, cam, nullptr, md, cl->p.data(), (int)cl->p.size(), &n);
    cl->p.resize(n); *out = cl; return SSM_OK;
}
// the fused forms (Mapper with motion_semantic_fuse=1): the same placeholders; the fusion itself is the linked host function
int ssm_backproject_fused(ssm_ctx* c, const uint16_t* depth, const uint8_t* rgb, const uint8_t* sem, const uint8_t*, int w, int h, const ssm_camera* cam, const double* T, double md,
                          const ssm_motion_fuse_params*, ssm_point* out, int cap, int* n_out) { return ssm_backproject(c, depth, rgb, sem, w, h, cam, T, md, out, cap, n_out); }
int ssm_backproject_fused_dev(ssm_ctx* c, const uint16_t* depth, const uint8_t* rgb, const uint8_t* sem, const uint8_t*, int w, int h, const ssm_camera* cam, double md,
                              const ssm_motion_fuse_params*, ssm_cloud** out) { return ssm_backproject_dev(c, depth, rgb, sem, w, h, cam, md, out); }
int ssm_motion_fuse(ssm_ctx*, const uint8_t* sem, const uint8_t* motion, int w, int h, int stride, const ssm_motion_fuse_params* params, uint8_t* mask, ssm_motion_fuse_info* info)
{ return ssm_motion_fuse_host(sem, motion, w, h, stride, params, mask, info, nullptr, nullptr, nullptr, nullptr); }
// the outlier removal (Mapper with mapper_outlier_removal=1): the linked host function in the device entry points' place
int ssm_sor_filter(ssm_ctx*, const ssm_point* pts, int n, const ssm_sor_params* params, ssm_point* out, int cap, int* n_out, ssm_sor_info* info)
{ return ssm_sor_filter_host(pts, n, params, out, cap, n_out, info, nullptr, nullptr); }
int ssm_cloud_sor(ssm_ctx*, ssm_cloud* cl, const ssm_sor_params* params, ssm_sor_info* info)
{
    std::vector<ssm_point> out(cl->p.size() + 1); int n = 0;
    const int rc = ssm_sor_filter_host(cl->p.data(), (int)cl->p.size(), params, out.data(), (int)out.size(), &n, info, nullptr, nullptr);
    if (rc == SSM_OK) { out.resize((size_t)n); cl->p.swap(out); }
    return rc;
}
// free-space carving (Mapper with mapper_carve=1): a "view" is a host copy of the depth image, the linked host function in the device entry points' place
struct ssm_carve_view { std::vector<uint16_t> depth; int w, h; ssm_camera cam; };
int ssm_carve_view_create(ssm_ctx*, const uint16_t* depth, int w, int h, const ssm_camera* cam, ssm_carve_view** out)
{ ssm_carve_view* v = new ssm_carve_view(); v->depth.assign(depth, depth + (size_t)w * h); v->w = w; v->h = h; v->cam = *cam; *out = v; return SSM_OK; }
void ssm_carve_view_free(ssm_ctx*, ssm_carve_view* v) { delete v; }
int ssm_carve_points(ssm_ctx*, const uint16_t* depth, int w, int h, const ssm_camera* cam, const double* Tv, const ssm_point* pts, int n, const double* Tc, uint8_t* run,
                     const ssm_carve_params* params, ssm_point* out, int cap, int* n_out, ssm_carve_info* info)
{ return ssm_carve_host(depth, w, h, cam, Tv, pts, n, Tc, run, params, out, cap, n_out, info, nullptr, nullptr); }
int ssm_carve(ssm_ctx*, const ssm_carve_view* v, const double* Tv, ssm_cloud* const* clouds, const double* Tc, int m, const ssm_carve_params* params, ssm_carve_info* infos)
{
    for (int k = 0; k < m; k++) {
        ssm_cloud* cl = clouds[k];
        cl->run.resize(cl->p.size(), 0);
        std::vector<ssm_point> out(cl->p.size() + 1); int n = 0; ssm_carve_info I;
        const int rc = ssm_carve_host(v->depth.data(), v->w, v->h, &v->cam, Tv, cl->p.data(), (int)cl->p.size(), Tc + 16 * k, cl->run.data(), params, out.data(), (int)out.size(), &n, &I, nullptr, nullptr);
        if (rc != SSM_OK) return rc;
        out.resize((size_t)n); cl->p.swap(out); cl->run.resize((size_t)n);
        if (infos) infos[k] = I;
    }
    return SSM_OK;
}
// map rendering (Mapper with mapper_render=1): a "target" is the host images, the linked host functions in the device entry points' place
struct ssm_render_target { int w, h; std::vector<uint16_t> depth; std::vector<uint8_t> bgr, label; std::vector<int32_t> index; };
int ssm_render_target_create(ssm_ctx*, int w, int h, ssm_render_target** out)
{
    if (w < 1 || h < 1) return SSM_E_INVAL;
    ssm_render_target* t = new ssm_render_target(); const size_t np = (size_t)w * h;
    t->w = w; t->h = h; t->depth.assign(np, 0); t->bgr.assign(np * 3, 0); t->label.assign(np, 255); t->index.assign(np, -1); *out = t; return SSM_OK;
}
void ssm_render_target_free(ssm_ctx*, ssm_render_target* t) { delete t; }
int ssm_render_points(ssm_ctx*, ssm_render_target* t, const ssm_camera* cam, const double* Tv, const ssm_point* const* pts, const int32_t* n, const double* Tc, int m,
                      const ssm_render_params* params, ssm_render_info* info)
{ return ssm_render_host(t->w, t->h, cam, Tv, pts, n, Tc, m, params, t->depth.data(), t->bgr.data(), t->label.data(), t->index.data(), nullptr, info); }
int ssm_render_clouds(ssm_ctx* c, ssm_render_target* t, const ssm_camera* cam, const double* Tv, ssm_cloud* const* clouds, const double* Tc, int m, const ssm_render_params* params,
                      ssm_render_info* info)
{
    std::vector<const ssm_point*> pts; std::vector<int32_t> n;
    for (int k = 0; k < m; k++) { pts.push_back(clouds[k]->p.data()); n.push_back((int32_t)clouds[k]->p.size()); }
    return ssm_render_points(c, t, cam, Tv, pts.data(), n.data(), Tc, m, params, info);
}
int ssm_render_fetch(ssm_ctx*, const ssm_render_target* t, uint16_t* depth, uint8_t* bgr, uint8_t* label, int32_t* index)
{
    if (depth) memcpy(depth, t->depth.data(), t->depth.size() * 2);
    if (bgr) memcpy(bgr, t->bgr.data(), t->bgr.size());
    if (label) memcpy(label, t->label.data(), t->label.size());
    if (index) memcpy(index, t->index.data(), t->index.size() * 4);
    return SSM_OK;
}
int ssm_render_compare(ssm_ctx*, ssm_render_target* t, const uint16_t* depth, const uint8_t* sem, double scale, const ssm_render_params* params, ssm_render_compare_info* info, uint8_t* cls)
{ return ssm_render_compare_host(t->depth.data(), t->label.data(), t->w, t->h, depth, sem, scale, params, info, cls); }
// the ground grid (Mapper with mapper_grid=1): a "target" is the host arrays, the linked host function in the device entry points' place
struct ssm_grid_target { int64_t cap; int nx, ny; ssm_grid_params P; std::vector<uint8_t> cls, gl, ol; std::vector<int32_t> gq, tq; std::vector<uint32_t> n, nh; };
int ssm_grid_target_create(ssm_ctx*, int nx, int ny, ssm_grid_target** out)
{
    if (nx < 1 || ny < 1 || (int64_t)nx * ny > ((int64_t)1 << 24)) return SSM_E_INVAL;
    ssm_grid_target* t = new ssm_grid_target(); const size_t nc = (size_t)nx * ny;
    t->cap = (int64_t)nc; t->nx = t->ny = 0; t->cls.resize(nc); t->gl.resize(nc); t->ol.resize(nc); t->gq.resize(nc); t->tq.resize(nc); t->n.resize(nc); t->nh.resize(nc); *out = t; return SSM_OK;
}
void ssm_grid_target_free(ssm_ctx*, ssm_grid_target* t) { delete t; }
int ssm_grid_points(ssm_ctx*, ssm_grid_target* t, const ssm_point* const* pts, const int32_t* n, const double* Tc, int m, const ssm_grid_params* params, ssm_grid_info* info)
{
    ssm_grid_params P; ssm_grid_params_default(&P); if (params) P = *params;
    if (P.nx >= 1 && P.ny >= 1 && (int64_t)P.nx * P.ny > t->cap) return SSM_E_INVAL;
    const int rc = ssm_grid_host(pts, n, Tc, m, &P, t->cls.data(), t->gl.data(), t->ol.data(), t->gq.data(), t->tq.data(), t->n.data(), t->nh.data(), nullptr, info);
    if (rc == SSM_OK) { t->nx = P.nx; t->ny = P.ny; t->P = P; }
    return rc;
}
int ssm_grid_clouds(ssm_ctx* c, ssm_grid_target* t, ssm_cloud* const* clouds, const double* Tc, int m, const ssm_grid_params* params, ssm_grid_info* info)
{
    std::vector<const ssm_point*> pts; std::vector<int32_t> n;
    for (int k = 0; k < m; k++) { pts.push_back(clouds[k]->p.data()); n.push_back((int32_t)clouds[k]->p.size()); }
    return ssm_grid_points(c, t, pts.data(), n.data(), Tc, m, params, info);
}
int ssm_grid_fetch(ssm_ctx*, const ssm_grid_target* t, uint8_t* cls, uint8_t* gl, uint8_t* ol, int32_t* gq, int32_t* tq, uint32_t* n, uint32_t* nh)
{
    const size_t nc = (size_t)t->nx * t->ny;
    if (cls) memcpy(cls, t->cls.data(), nc);
    if (gl) memcpy(gl, t->gl.data(), nc);
    if (ol) memcpy(ol, t->ol.data(), nc);
    if (gq) memcpy(gq, t->gq.data(), nc * 4);
    if (tq) memcpy(tq, t->tq.data(), nc * 4);
    if (n) memcpy(n, t->n.data(), nc * 4);
    if (nh) memcpy(nh, t->nh.data(), nc * 4);
    return SSM_OK;
}
// object extraction (Mapper with mapper_objects=1): a "target" is the host records and image; stage 1 only remembers its parameters, stage 2 runs the linked host
// function (the grid again, then both stages) in the device entry points' place
struct ssm_objects_target { int64_t cap; ssm_objects_params P; std::vector<ssm_object> rec; std::vector<int32_t> oid; };
int ssm_objects_target_create(ssm_ctx*, int nx, int ny, ssm_objects_target** out)
{
    if (nx < 1 || ny < 1 || (int64_t)nx * ny > ((int64_t)1 << 24)) return SSM_E_INVAL;
    ssm_objects_target* t = new ssm_objects_target(); t->cap = (int64_t)nx * ny; ssm_objects_params_default(&t->P); *out = t; return SSM_OK;
}
void ssm_objects_target_free(ssm_ctx*, ssm_objects_target* t) { delete t; }
int ssm_objects_grid(ssm_ctx*, const ssm_grid_target* g, const ssm_objects_params* params, ssm_objects_target* t, ssm_objects_info* info)
{
    if (!g || !t || (int64_t)g->nx * g->ny > t->cap || g->nx < 1) return SSM_E_INVAL;
    ssm_objects_params_default(&t->P); if (params) t->P = *params;
    t->rec.clear(); t->oid.resize((size_t)g->nx * g->ny); int n = 0;          // (a first call with cap 0 gives the count: records per object, never per cell)
    int rc = ssm_objects_cells_host(g->cls.data(), g->ol.data(), g->gq.data(), g->tq.data(), g->nh.data(), g->nx, g->ny, &t->P, nullptr, 0, &n, nullptr, nullptr);
    if (rc != SSM_OK && rc != SSM_E_CAPACITY) return rc;
    t->rec.resize((size_t)n);
    return ssm_objects_cells_host(g->cls.data(), g->ol.data(), g->gq.data(), g->tq.data(), g->nh.data(), g->nx, g->ny, &t->P, t->rec.data(), n, &n, t->oid.data(), info);
}
int ssm_objects_points(ssm_ctx*, const ssm_grid_target* g, ssm_objects_target* t, const ssm_point* const* pts, const int32_t* n, const double* Tc, int m, int32_t* ids, ssm_objects_info* info)
{
    if (!g || !t) return SSM_E_INVAL;
    t->rec.clear(); t->oid.resize((size_t)g->nx * g->ny); int k = 0;
    int rc = ssm_objects_host(pts, n, Tc, m, &g->P, &t->P, nullptr, 0, &k, nullptr, nullptr, nullptr);
    if (rc != SSM_OK && rc != SSM_E_CAPACITY) return rc;
    t->rec.resize((size_t)k);
    return ssm_objects_host(pts, n, Tc, m, &g->P, &t->P, t->rec.data(), k, &k, t->oid.data(), ids, info);
}
int ssm_objects_clouds(ssm_ctx* c, const ssm_grid_target* g, ssm_objects_target* t, ssm_cloud* const* clouds, const double* Tc, int m, ssm_objects_info* info)
{
    std::vector<const ssm_point*> pts; std::vector<int32_t> n;
    for (int k = 0; k < m; k++) { pts.push_back(clouds[k]->p.data()); n.push_back((int32_t)clouds[k]->p.size()); }
    return ssm_objects_points(c, g, t, pts.data(), n.data(), Tc, m, nullptr, info);
}
int ssm_objects_fetch(ssm_ctx*, const ssm_objects_target* t, ssm_object* out, int cap, int* n_out, int32_t* object_id)
{
    if (n_out) *n_out = (int)t->rec.size();
    if (out && (int)t->rec.size() > cap) return SSM_E_CAPACITY;
    if (out && !t->rec.empty()) memcpy(out, t->rec.data(), t->rec.size() * sizeof(ssm_object));
    if (object_id && !t->oid.empty()) memcpy(object_id, t->oid.data(), t->oid.size() * 4);
    return SSM_OK;
}
// the clearance map (Mapper with mapper_clearance=1): a "target" is the host images, the linked host function in the device entry point's place (the cell size the
// grid build's, as on the device)
struct ssm_clearance_target { int64_t cap; int nx, ny; std::vector<uint32_t> d2; std::vector<int32_t> near; std::vector<uint8_t> reach; int64_t seed_cell = -1; double cell = 1.0; };
int ssm_clearance_target_create(ssm_ctx*, int nx, int ny, ssm_clearance_target** out)
{
    if (!out || nx < 1 || ny < 1 || (int64_t)nx * ny > ((int64_t)1 << 24)) return SSM_E_INVAL;
    ssm_clearance_target* t = new ssm_clearance_target(); t->cap = (int64_t)nx * ny; t->nx = t->ny = 0; *out = t; return SSM_OK;
}
void ssm_clearance_target_free(ssm_ctx*, ssm_clearance_target* t) { delete t; }
int ssm_clearance_grid(ssm_ctx*, const ssm_grid_target* g, const ssm_clearance_params* params, ssm_clearance_target* t, ssm_clearance_info* info)
{
    if (!g || !t || g->nx < 1 || (int64_t)g->nx * g->ny > t->cap) return SSM_E_INVAL;
    ssm_clearance_params P; ssm_clearance_params_default(&P); if (params) P = *params;
    P.cell = g->P.cell;
    const size_t nc = (size_t)g->nx * g->ny;
    std::vector<uint32_t> d2(nc); std::vector<int32_t> near(nc); std::vector<uint8_t> reach(nc);
    ssm_clearance_info I;
    const int rc = ssm_clearance_cells_host(g->cls.data(), g->nx, g->ny, &P, d2.data(), near.data(), reach.data(), &I);
    if (rc == SSM_OK) { t->nx = g->nx; t->ny = g->ny; t->d2.swap(d2); t->near.swap(near); t->reach.swap(reach); t->seed_cell = I.seed_cell; t->cell = P.cell; if (info) *info = I; }
    return rc;
}
int ssm_clearance_fetch(ssm_ctx*, const ssm_clearance_target* t, uint32_t* dist2, int32_t* nearest, uint8_t* reach)
{
    if (!t || t->nx < 1) return SSM_E_INVAL;
    const size_t nc = (size_t)t->nx * t->ny;
    if (dist2) memcpy(dist2, t->d2.data(), nc * 4);
    if (nearest) memcpy(nearest, t->near.data(), nc * 4);
    if (reach) memcpy(reach, t->reach.data(), nc);
    return SSM_OK;
}
// the route field (Mapper with mapper_route=1): a "target" is the host field with the copy of dist2 a path query needs, the linked host functions in the device
// entry points' place (the cell size and the source the clearance call's, as on the device)
struct ssm_route_target { int64_t cap; int nx, ny, max_path; ssm_route_params P; std::vector<uint32_t> cost, d2; std::vector<int32_t> parent; };
int ssm_route_target_create(ssm_ctx*, int nx, int ny, int max_path, ssm_route_target** out)
{
    if (!out || nx < 1 || ny < 1 || (int64_t)nx * ny > ((int64_t)1 << 24) || max_path < 1) return SSM_E_INVAL;
    ssm_route_target* t = new ssm_route_target(); t->cap = (int64_t)nx * ny; t->nx = t->ny = 0; t->max_path = max_path; ssm_route_params_default(&t->P); *out = t; return SSM_OK;
}
void ssm_route_target_free(ssm_ctx*, ssm_route_target* t) { delete t; }
int ssm_route_field(ssm_ctx*, const ssm_clearance_target* ct, const ssm_route_params* params, ssm_route_target* t, ssm_route_info* info)
{
    if (!ct || !t || ct->nx < 1 || (int64_t)ct->nx * ct->ny > t->cap) return SSM_E_INVAL;
    ssm_route_params P; ssm_route_params_default(&P); if (params) P = *params;
    P.cell = ct->cell;
    const size_t nc = (size_t)ct->nx * ct->ny;
    std::vector<uint32_t> cost(nc); std::vector<int32_t> parent(nc);
    const int rc = ssm_route_cells_host(ct->reach.data(), ct->d2.data(), ct->nx, ct->ny, (int)ct->seed_cell, &P, cost.data(), parent.data(), info);
    if (rc == SSM_OK) { t->nx = ct->nx; t->ny = ct->ny; t->P = P; t->cost.swap(cost); t->parent.swap(parent); t->d2 = ct->d2; }
    return rc;
}
int ssm_route_path(ssm_ctx*, ssm_route_target* t, int goal_cx, int goal_cy, int goal_snap, int32_t* cells_out, ssm_route_path_info* path_info)
{
    if (!t || t->nx < 1 || !cells_out || !path_info) return SSM_E_INVAL;
    return ssm_route_path_host(t->cost.data(), t->parent.data(), t->d2.data(), t->nx, t->ny, &t->P, goal_cx, goal_cy, goal_snap, t->max_path, cells_out, path_info);
}
int ssm_route_fetch(ssm_ctx*, const ssm_route_target* t, uint32_t* cost, int32_t* parent)
{
    if (!t || t->nx < 1) return SSM_E_INVAL;
    const size_t nc = (size_t)t->nx * t->ny;
    if (cost) memcpy(cost, t->cost.data(), nc * 4);
    if (parent) memcpy(parent, t->parent.data(), nc * 4);
    return SSM_OK;
}
// label fusion (Mapper with mapper_relabel=1): a "view" is a host copy of the depth image and the label image, the linked host function in the device entry points' place
struct ssm_relabel_view { std::vector<uint16_t> depth; std::vector<uint8_t> label; int w, h; ssm_camera cam; };
int ssm_relabel_view_create(ssm_ctx*, const uint16_t* depth, const uint8_t* sem, int w, int h, const ssm_camera* cam, ssm_relabel_view** out)
{
    ssm_relabel_view* v = new ssm_relabel_view(); v->depth.assign(depth, depth + (size_t)w * h); v->label.resize((size_t)w * h); v->w = w; v->h = h; v->cam = *cam;
    ssm_relabel_labels_host(sem, (int64_t)w * h, v->label.data()); *out = v; return SSM_OK;
}
void ssm_relabel_view_free(ssm_ctx*, ssm_relabel_view* v) { delete v; }
int ssm_relabel_points(ssm_ctx*, const ssm_relabel_view* const* views, const double* Tv, int v, const ssm_point* pts, int n, const double* Tc, const ssm_relabel_params* params,
                       uint32_t* label_out, ssm_relabel_info* info)
{
    std::vector<ssm_relabel_host_view> hv;
    for (int k = 0; k < v; k++) { if (!views[k]) return SSM_E_INVAL; ssm_relabel_host_view h; h.depth = views[k]->depth.data(); h.label = views[k]->label.data(); h.w = views[k]->w; h.h = views[k]->h; h.cam = views[k]->cam; hv.push_back(h); }
    return ssm_relabel_host(hv.data(), Tv, v, pts, n, Tc, params, label_out, nullptr, info);
}
int ssm_relabel(ssm_ctx* c, const ssm_relabel_view* const* views, const double* Tv, int v, ssm_cloud* cl, const double* Tc, const ssm_relabel_params* params, ssm_relabel_info* info)
{
    std::vector<uint32_t> lab(cl->p.size() + 1);
    const int rc = ssm_relabel_points(c, views, Tv, v, cl->p.data(), (int)cl->p.size(), Tc, params, lab.data(), info);
    if (rc == SSM_OK) for (size_t i = 0; i < cl->p.size(); i++) cl->p[i].label = lab[i];
    return rc;
}
// dense alignment (Mapper with mapper_align=1): a "view" is a host copy of the depth image, the linked host function in the device entry points' place
struct ssm_align_view { std::vector<uint16_t> depth; int w, h; ssm_camera cam; double tol_abs; int32_t tol_rel_ppm; };
int ssm_align_view_create(ssm_ctx*, const uint16_t* depth, int w, int h, const ssm_camera* cam, const ssm_align_params* params, ssm_align_view** out)
{
    if (w < 3 || h < 3) return SSM_E_INVAL;
    ssm_align_params P; ssm_align_params_default(&P); if (params) P = *params;
    ssm_align_view* v = new ssm_align_view(); v->depth.assign(depth, depth + (size_t)w * h); v->w = w; v->h = h; v->cam = *cam; v->tol_abs = P.tol_abs; v->tol_rel_ppm = P.tol_rel_ppm;
    *out = v; return SSM_OK;
}
void ssm_align_view_free(ssm_ctx*, ssm_align_view* v) { delete v; }
int ssm_align_points(ssm_ctx*, const ssm_align_view* v, const double* Tv, const ssm_point* const* pts, const int32_t* n, const double* Tc, int m, const ssm_align_params* params,
                     double* T_out, ssm_align_info* info)
{
    ssm_align_params P; ssm_align_params_default(&P); if (params) P = *params;
    P.tol_abs = v->tol_abs; P.tol_rel_ppm = v->tol_rel_ppm;
    return ssm_align_host(v->depth.data(), v->w, v->h, &v->cam, Tv, pts, n, Tc, m, &P, T_out, info, nullptr, nullptr, nullptr, 0, nullptr);
}
int ssm_align_clouds(ssm_ctx* c, const ssm_align_view* v, const double* Tv, ssm_cloud* const* clouds, const double* Tc, int m, const ssm_align_params* params, double* T_out,
                     ssm_align_info* info)
{
    std::vector<const ssm_point*> pts; std::vector<int32_t> n;
    for (int k = 0; k < m; k++) { pts.push_back(clouds[k]->p.data()); n.push_back((int32_t)clouds[k]->p.size()); }
    return ssm_align_points(c, v, Tv, pts.data(), n.data(), Tc, m, params, T_out, info);
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
