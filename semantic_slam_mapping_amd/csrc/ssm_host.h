// ssm_host.h -- what the library's host-only sources (csrc/host_sources.mk lists them: plain C++ without a HIP header and without ssm_ctx.h) share with the device
// translation units; ssm_orb_plan.cpp and ssm_map_plan.cpp are host-only sources with headers of their own.  Those sources are compiled once and LINKED into libssm_hip.so, into the
// CPU sanitizer binaries of the host layer and into host/test_vocab_train / host/test_track.  What they need from the side that owns the context and the device are the hooks:
// defined in ssm_abi.hip / ssm_uvd.hip / ssm_pgo.hip / ssm_track.hip / ssm_cloud_list.hip, and as "no device" by a build without one (host/san_stub_device.cpp).  Not installed.
#pragma once
#include "../../include/ssm_hip.h"
#include "../../include/ssm/vocab_train_core.h"
#include "../../include/ssm/uvd_core.h"
#include "../../include/ssm/pgo_core.h"
#include "../../include/ssm/motion_fuse_core.h"
#include "../../include/ssm/sor_core.h"
#include "../../include/ssm/carve_core.h"
#include "../../include/ssm/render_core.h"
#include "../../include/ssm/align_core.h"
#include "../../include/ssm/grid_core.h"
#include "../../include/ssm/objects_core.h"
#include "../../include/ssm/clearance_core.h"
#include "../../include/ssm/route_core.h"
#include "../../include/ssm/relabel_core.h"
#include "../../include/ssm/pnp_core.h"
#include "pnp_state.h"
#include "cloud_table.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>
#define SSM_HIDDEN __attribute__((visibility("hidden")))
// hooks (ssm_abi.hip).  The one error path: the message goes to the context, or without one to what ssm_last_error(NULL) reads on this thread; returns `code`
SSM_HIDDEN int host_fail(ssm_ctx* c, int code, const std::string& msg);
SSM_HIDDEN std::unique_lock<std::mutex> host_lock(ssm_ctx* c);          // the context's lock, held; nothing without a context

// ---------------------------------------------------------------- vocabulary (ssm_vocab.cpp, ssm_vocab_train_host.cpp)
struct ssm_vocab {
    int k = 0, L = 0, scoring = 0, weighting = 0;
    std::vector<int32_t> first_child, n_child, word;      // per node, breadth-first numbering (node 0 = the root)
    std::vector<uint32_t> desc;                           // per node, 8 words
    std::vector<double> weight;                           // per word id
    std::vector<int32_t> file_id;                         // per node: the id it was given under (ssm_vocab_export writes that order back)
    int max_depth = 0;
    ssm_bow::Tree tree() const
    {
        ssm_bow::Tree t; t.first_child = first_child.data(); t.n_child = n_child.data(); t.desc = desc.data(); t.word = word.data(); t.weight = weight.data();
        t.n_nodes = (int)n_child.size(); t.n_words = (int)weight.size(); t.max_depth = max_depth;
        return t;
    }
};
// the tree as ssm_vocab_create takes it: node i has id i + 1, ids are breadth-first (level by level; inside a level by parent id, then by cluster)
struct VtTree {
    std::vector<int32_t> parent; std::vector<uint8_t> leaf; std::vector<uint32_t> desc;
    int add(int parent_id, const uint32_t* d) { parent.push_back(parent_id); leaf.push_back(0); desc.insert(desc.end(), d, d + ssm_vt::DESC_WORDS); return (int)parent.size(); }      // -> the new id
};
SSM_HIDDEN int vt_check(ssm_ctx* c, const uint8_t* desc, const int32_t* n_per_frame, int n_frames, const ssm_vocab_train_params* p, ssm_vocab** out, int* n_out);
SSM_HIDDEN int vt_finish(const VtTree& t, const std::vector<int32_t>& leaf_of_feature, const int32_t* n_per_frame, int n_frames, const ssm_vocab_train_params* p,
                         int32_t* word_of_feature, ssm_vocab_train_report* report, ssm_vocab** out);          // (its ssm_vocab_create cannot fail on a tree built here)
SSM_HIDDEN int vt_kmajority_check(const uint8_t* desc, int n, const int32_t* node_of, const int32_t* cluster_of, int n_nodes, int k, const uint8_t* centres, const int32_t* assign_out);
SSM_HIDDEN int vt_kmajority_host(const uint8_t* desc, int n, const int32_t* node_of, const int32_t* cluster_of, int n_nodes, int k, uint8_t* centres, int32_t* assign_out);

// ---------------------------------------------------------------- U/V-disparity (ssm_uvd_host.cpp)
struct UvdKalman {          // KalmanFilter(2, 1, 0) of uvdisparity.cpp:35-47 whose second state is never observed: a scalar float32 filter
    float x = 0.0f, P = 1.0f;
    void update(float z) { P += 5e-6f; const float K = P / (P + 0.001f); x += K * (z - x); P = (1.0f - K) * P; }
};
typedef std::vector<uint8_t> UvdImg;
struct UvdFrame {           // one frame of the last call: what the host steps produce and ssm_debug_uvd_* hand out
    ssm_uvd_info info{}; ssm_uvdc::FrameK k{};
    int w = 0, h = 0, max_disp = 0;
    UvdImg v_dis, blur, erode, bin;           // v_dis: h x 256; the others h x v_cols
    std::vector<int32_t> pts, areas;
    UvdImg u_raw, u_adj, uni;                 // u_rows x w
    std::vector<UvdImg> found, merged, kept;
};
struct UvdDev;              // the device workspaces of an object with a context: ssm_uvd.hip
struct ssm_uvd {
    ssm_ctx* c = nullptr;                       // null: a host-only object (ssm_uvd_process_host)
    ssm_uvd_params p{};
    UvdKalman kf1, kf2;
    double rate[ssm_uvdc::MAX_BINS];             // adjustUdisIntense's sigmoid(row, 0.02, 32) per U-disparity row
    std::vector<UvdFrame> frames;               // the last call
    bool record = false;                        // ssm_debug_uvd_record: keep the masks found / merged / kept of every frame for ssm_debug_uvd_stage
    double call_ms[3] = {0, 0, 0};              // the last device call: host step 1, host step 2, the whole call (ssm_debug_uvd_times)
    UvdDev* dev = nullptr;
};
SSM_HIDDEN void uvd_host_step1(const ssm_uvd_params& p, UvdKalman& kf1, UvdKalman& kf2, UvdFrame& F, int min_disp, bool skip);
SSM_HIDDEN void uvd_host_step2(const ssm_uvd_params& p, UvdFrame& F, ssm_pmatch* m, uint8_t* flags, int nm, const uint8_t* probe_roi, const int16_t* probe_disp, bool record);
inline ssm_uvdc::Calib uvd_calib(const ssm_uvd_params& p) { return ssm_uvdc::Calib{p.f, p.cu, p.cv, p.base}; }
inline ssm_uvdc::Roi uvd_roi(const ssm_uvd_params& p) { return ssm_uvdc::Roi{p.roi_x, p.roi_y, p.roi_z}; }
SSM_HIDDEN int uvd_dev_attach(ssm_uvd* u);          // hooks (ssm_uvd.hip): ssm_uvd_create with a context -> u->dev; ssm_uvd_destroy of such an object
SSM_HIDDEN void uvd_dev_release(ssm_uvd* u);

// ---------------------------------------------------------------- semantic-motion fusion (ssm_motion_fuse_host.cpp)
SSM_HIDDEN int mf_check(ssm_ctx* c, int n, int w, int h, size_t stride);          // the sizes a call may have (host function and device entry points alike)

// ---------------------------------------------------------------- statistical outlier removal (ssm_sor_host.cpp)
SSM_HIDDEN int sor_check(ssm_ctx* c, int n, const ssm_sor_params& P);          // the arguments a call may have (host function and device entry points alike)
SSM_HIDDEN int sor_off_grid(ssm_ctx* c);                                       // SSM_E_INVAL with the message of a mean distance off the statistics grid

// ---------------------------------------------------------------- the cloud-segment table (ssm_cloud_table.cpp; cloud_table.h)
// seg: m records with n (the points used) filled -> every off; blk (null: not wanted): the cloud of each block of T points' first point; -> the points, *blocks
SSM_HIDDEN int64_t cloud_table_build(CloudSeg* seg, int m, int T, int32_t* blk, int64_t* blocks);
// the points a host-array call uses: the sum of ceil(n[k] / stride) -> *total; false: a negative count
SSM_HIDDEN bool cloud_count(const int32_t* n, int m, int stride, int64_t* total);
// A stage's rule for the clouds of one call.  twice_msg: the refusal of a cloud listed twice (null: allowed, it is only read); stride: every stride-th point is used;
// the bound on the points used: fewer than limit, or with sums (alignment) what align_core.h's sums_fit allows; the stage's messages for a negative count and the bound
struct CloudRule { const char* twice_msg; int stride; int64_t limit; const ssm_alignc::Setup* sums; const char* negative_msg; const char* bound_msg; };
SSM_HIDDEN int cloud_bound_check(ssm_ctx* c, const CloudRule& R, int64_t total);                              // SSM_E_INVAL with R.bound_msg
SSM_HIDDEN int cloud_total_check(ssm_ctx* c, const CloudRule& R, const int32_t* n, int m, int64_t* total);    // cloud_count (SSM_E_INVAL with R.negative_msg), then the bound
// the clouds of a host-array call, per cloud in this order: a null array with a count, the same array twice (both used), the pose (ssm_carve_host.cpp)
SSM_HIDDEN int cloud_arrays_check(ssm_ctx* c, const char* twice_msg, const ssm_point* const* pts, const int32_t* n, const double* T_clouds, int m);
// Where a call's clouds come from: device handles, host arrays with counts, or the context's viewer map as one borrowed cloud at the identity pose (no_map_msg: the
// stage's refusal of a context without one)
struct CloudSource {
    enum Kind { HANDLES, ARRAYS, VIEWER_MAP } kind;
    ssm_cloud* const* clouds; const ssm_point* const* pts; const int32_t* n; const double* T_clouds; int m; const char* no_map_msg;
};
extern SSM_HIDDEN const double CLOUD_EYE[16];
inline CloudSource cloud_handles(ssm_cloud* const* clouds, const double* T_clouds, int m) { return {CloudSource::HANDLES, clouds, nullptr, nullptr, T_clouds, m, nullptr}; }
inline CloudSource cloud_arrays(const ssm_point* const* pts, const int32_t* n, const double* T_clouds, int m) { return {CloudSource::ARRAYS, nullptr, pts, n, T_clouds, m, nullptr}; }
inline CloudSource cloud_viewer_map(const char* no_map_msg) { return {CloudSource::VIEWER_MAP, nullptr, nullptr, nullptr, CLOUD_EYE, 1, no_map_msg}; }
// hooks (ssm_cloud_list.hip).  cloud_call: what every entry point does with its list after its own *_begin -- the null test of the list, then for host arrays the
// counts and the bound before the arrays (cloud_list), for handles the handles and poses (cloud_list) before the bound -> segs (pts, n, stride, M) and *total
SSM_HIDDEN int cloud_call(ssm_ctx* c, const CloudSource& src, const CloudRule& R, const double* T_view, std::vector<CloudSeg>& segs, int64_t* total);
SSM_HIDDEN void host_wait(ssm_ctx* c);          // the context's lock taken, its device made current, its main stream waited for; nothing without a context
// every ssm_*_view_free / ssm_*_target_free: nothing queued may still read the object
template <class T> void free_after_wait(ssm_ctx* c, T* t) { if (!t) return; host_wait(c); delete t; }

// ---------------------------------------------------------------- free-space carving (ssm_carve_host.cpp)
// the arguments a call may have (host function and device entry points alike); S: what the view's size and camera and the parameters become for carve_core.h
SSM_HIDDEN int carve_check(ssm_ctx* c, int w, int h, const ssm_camera* cam, const ssm_carve_params& P, ssm_carvec::Setup* S);
SSM_HIDDEN int carve_pose_check(ssm_ctx* c, const double* T);                  // SSM_E_INVAL for a null or non-finite pose

// ---------------------------------------------------------------- map rendering (ssm_render_host.cpp)
// the arguments a call may have (host functions and device entry points alike); S: what the view's size and camera and the parameters become for render_core.h
SSM_HIDDEN int render_size_check(ssm_ctx* c, int w, int h);
SSM_HIDDEN int render_check(ssm_ctx* c, int w, int h, const ssm_camera* cam, const ssm_render_params& P, ssm_renderc::Setup* S);
SSM_HIDDEN int render_compare_check(ssm_ctx* c, const ssm_render_params& P, double scale, int64_t* tol_abs);      // tol_abs: in depth units
SSM_HIDDEN CloudRule render_cloud_rule();          // a cloud may be listed twice; fewer than 2^32 points

// ---------------------------------------------------------------- ground grid (ssm_grid_host.cpp)
// the arguments a call may have (host function and device entry points alike); S: what the parameters become for grid_core.h
SSM_HIDDEN int grid_check(ssm_ctx* c, const ssm_grid_params& P, ssm_gridc::Setup* S);
SSM_HIDDEN CloudRule grid_cloud_rule();            // no cloud twice; fewer than 2^31 points

// ---------------------------------------------------------------- object extraction (ssm_objects_host.cpp)
// the parameters a call may have (host functions and device entry points alike); S: what they become for objects_core.h
SSM_HIDDEN int objects_check(ssm_ctx* c, const ssm_objects_params& P, ssm_objc::Setup* S);
SSM_HIDDEN int objects_extent_check(ssm_ctx* c, double x0, double y0, double cell, int nx, int ny);      // SSM_E_INVAL for a grid whose extent leaves +-2^20 m
SSM_HIDDEN CloudRule objects_cloud_rule();         // no cloud twice; fewer than 2^31 points (the grid's bound)

// ---------------------------------------------------------------- clearance map (ssm_clearance_host.cpp)
// the grid's size and the parameters a call may have (host function and device entry points alike); cell: the grid's cell size; S: what they become for clearance_core.h
SSM_HIDDEN int clearance_check(ssm_ctx* c, const ssm_clearance_params& P, int nx, int ny, double cell, ssm_clrc::Setup* S);

// ---------------------------------------------------------------- route field (ssm_route_host.cpp)
// the grid's size and the parameters a call may have (host functions and device entry points alike); cell: the clearance map's cell size; S: what they become for
// route_core.h.  The goal of a path query; the source of hand-made inputs (reach on the host); the path info of "no goal cell"
SSM_HIDDEN int route_check(ssm_ctx* c, const ssm_route_params& P, int nx, int ny, double cell, ssm_rtc::Setup* S);
SSM_HIDDEN int route_goal_check(ssm_ctx* c, int nx, int ny, int goal_cx, int goal_cy, int goal_snap);
SSM_HIDDEN int route_source_check(ssm_ctx* c, const uint8_t* reach, int nx, int ny, int source_cell);
SSM_HIDDEN void route_path_none(ssm_route_path_info* I);

// ---------------------------------------------------------------- label fusion (ssm_relabel_host.cpp)
// the number of views and the parameters a call may have (host function and device entry points alike)
SSM_HIDDEN int relabel_check(ssm_ctx* c, int v, const ssm_relabel_params& P);
// one view's size, camera and pose checked -> V->S and V->M (T_cloud: checked by the caller); the image pointers are the caller's to fill
SSM_HIDDEN int relabel_view_fill(ssm_ctx* c, int w, int h, const ssm_camera* cam, const double* T_view, const double* T_cloud, const ssm_relabel_params& P, ssm_relabelc::View* V);

// ---------------------------------------------------------------- dense alignment (ssm_align_host.cpp)
// the arguments a call may have (host function and device entry points alike); S: what the view's size and camera and the parameters become for align_core.h
SSM_HIDDEN int align_check(ssm_ctx* c, int w, int h, const ssm_camera* cam, const ssm_align_params& P, ssm_alignc::Setup* S);
// no cloud twice; the points used after the stride must keep the sums below 2^62 (S must outlive the rule)
SSM_HIDDEN CloudRule align_cloud_rule(const ssm_alignc::Setup& S, int stride);
// the iteration loop of both paths: accumulate(E as 3 x 4 row-major, sums[NSUM]) adds up one iteration (a status other than SSM_OK ends the call with it);
// the solve, the stopping rules, T_view_out and the info are here.  record (may be null) gets one entry per iteration
SSM_HIDDEN int align_drive(const ssm_align_params& P, int64_t n_in, const double* T_view, const std::function<int(const double*, int64_t*)>& accumulate,
                           double* T_view_out, ssm_align_info* info, std::vector<ssm_align_iter>* record);

// ---------------------------------------------------------------- bulk tracker (ssm_track_host.cpp)
struct TrackRef {                         // a member of Tracker::refFrames: what trackRefFrame reads of it
    int64_t gidx = 0; int nkp = 0; double pose[16];
    std::vector<float> pos3d; std::vector<uint8_t> desc;
};
struct TrackDev;            // the chain's stream, event, scratch and state block on the device: ssm_track.hip
struct ssm_tracker {
    ssm_ctx* ctx = nullptr; ssm_tracker_params prm{}; ssm_camera cam{}; double ratio = 0.8;          // cam, ratio: the context's configuration (the attach hook)
    std::string err;
    int state = 0, cnt_lost = 0;          // Tracker::trackerState: 0 NOT_READY, 1 OK, 2 LOST
    double speed[16], last_pose[16];
    std::deque<TrackRef> refs;
    int64_t next_gidx = 0;                // global index of the current call's frame 0: a member with gidx < next_gidx is a frame of an earlier call
    // host copies of one call's outputs
    std::vector<int32_t> nkp, nmatch; std::vector<ssm_keypoint> kps; std::vector<float> pos3d; std::vector<uint8_t> desc; std::vector<ssm_dmatch> matches;
    std::vector<float> img, obj; std::vector<unsigned char> inl; std::vector<ssm_pnp::Edge> edges; std::vector<ssm_dmatch> tmp_matches;
    std::vector<uint8_t> have;            // per frame of the current call: bit 0 = features on the host, bit 1 = match tables on the host
    int blocks = 1;                       // the cluster form of the device chain (kernels_pnp.hip): blocks per chain, chosen by the attach hook
    long device_frames = 0, host_frames = 0;
    bool downgraded = false;              // the cluster form timed out once: one block per chain since (reported by ssm_tracker_last_error)
    int64_t work[4] = {0, 0, 0, 0};       // the device chain's passes over the edges (ssm_tracker_work)
    TrackDev* dev = nullptr;
};
// the state machine's steps that host/test_track.cpp also drives one by one.  track_regular: the deque is the run of frames directly in front of frame f of the
// call, so the device chain may take over there.  track_frame_host: Tracker::updateFrame for frame f on the host -> T_frame (16 doubles), *info
SSM_HIDDEN bool track_regular(const ssm_tracker* t, int f);
SSM_HIDDEN int track_frame_host(ssm_tracker* t, const ssm_seq_out_dev* seq, int f, double* T_frame, ssm_track_info* info);
// hooks (ssm_track.hip); the call's outputs themselves come to the host through the public ABI (ssm_sync, ssm_memcpy_d2h; ssm_match for an on-demand pair).
// attach: ssm_tracker_create -> cam, ratio, blocks, t->dev (SSM_E_INVAL: the context was configured with another tracker_ref_frames).  release: ssm_tracker_destroy.
// run: the chain on frames [f, n) of the call from the block *hs, which comes back as the device left it; the positions of the members with a negative ref_idx are
// read from t->refs (same order as the block).  A cluster (t->blocks > 1) that timed out gives SSM_OK with hs->stopped_at == -1 and nothing else: the caller goes
// on with one block.  Otherwise f < hs->stopped_at <= n, and pose_out[f .. stopped_at) and info (resized to stopped_at - f rows) hold the frames the chain walked
SSM_HIDDEN int track_dev_attach(ssm_tracker* t);
SSM_HIDDEN void track_dev_release(ssm_tracker* t);
SSM_HIDDEN int track_dev_run(ssm_tracker* t, const ssm_seq_out_dev* seq, int f, int n, PnpState* hs, double* pose_out, std::vector<ssm_track_info>& info);

// ---------------------------------------------------------------- pose graph (ssm_pgo_host.cpp)
struct PgoPlan {
    int nf = 0, na = 0; int64_t total = 0;
    std::vector<int32_t> aedge, vslot, svert, csr_off, csr_edge, first, reach; std::vector<int64_t> rowoff;
};
struct PgoDev;              // the device buffer and staging of an object with a context: ssm_pgo.hip
struct ssm_pgo {
    ssm_ctx* c = nullptr;                       // null: a host-only object
    std::vector<int32_t> ids; std::unordered_map<int, int> index;
    std::vector<double> pose; std::vector<uint8_t> fixed;
    std::vector<int32_t> efrom, eto, robust; std::vector<double> Z, zinv, omega;
    size_t cap_bytes = (size_t)1 << 30;
    PgoPlan plan;
    std::vector<double> lin, H, L, b, x, y, d, saved; ssm_pgc::Control ctl{}; ssm_pgc::Report rep{};     // host workspace / the last report
    PgoDev* dev = nullptr;
    double ms[ssm_pgc::NPHASE] = {0, 0, 0, 0, 0};
    int nv() const { return (int)ids.size(); }
    int ne() const { return (int)efrom.size(); }
};
// hooks (ssm_pgo.hip): ssm_pgo_create with a context (sets cap_bytes from the free device memory), ssm_pgo_destroy of such an object, and the device legs of
// ssm_pgo_optimize[_many], ssm_pgo_linearize and ssm_pgo_factor_solve: arguments checked, the graphs planned, hv / v = their host views
SSM_HIDDEN int pgo_dev_attach(ssm_pgo* g);
SSM_HIDDEN void pgo_dev_release(ssm_pgo* g);
SSM_HIDDEN int pgo_dev_optimize(ssm_pgo** graphs, int n, const ssm_pgc::View* hv, int iterations);                  // -> every pose, rep
SSM_HIDDEN int pgo_dev_linearize(ssm_pgo* g, const ssm_pgc::View& v);                                      // -> g->lin, g->H, g->b
SSM_HIDDEN int pgo_dev_factor_solve(ssm_pgo* g, ssm_pgo& t, const ssm_pgc::View& v, double lambda);       // g owns the device memory; -> t.x, t.ctl
