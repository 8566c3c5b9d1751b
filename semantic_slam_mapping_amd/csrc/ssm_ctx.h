// ssm_ctx.h -- the context of libssm_hip.so and what its host-side translation units share (ssm_abi.hip: lifecycle, ORB / matcher / sequence path; ssm_map.hip: voxel map,
// multi-GPU merge, device-resident Mapper; ssm_segnet_abi.hip: Classifier; ssm_stereo_abi.hip: quad matcher, SGBM depth, stereo VO, solvePnP).  Not installed.
#pragma once
#include "ssm_internal.h"
#include "pnp_chain.h"
#include "ssm_map_plan.h"
#include "ssm_seq_plan.h"
#include <rccl/rccl.h>
#include <cmath>
#include <cfloat>
#include <cstring>
#include <cstdlib>
#include <atomic>
#include <memory>
#include <mutex>
#include <type_traits>
#include <utility>
#include <functional>
#include <string>
#include <vector>
#define SSM_HIDDEN __attribute__((visibility("hidden")))

// Owner of ONE device allocation (Pinned: page-locked host memory) of a context, a StereoState, a SegNetState, an OrbWork or an ssm_tracker.  Move-only;
// alloc releases what the buffer held first, reset() and the destructor release it.  It converts to T*, so launches, copies and pointer arithmetic read
// as with a raw pointer.  Nothing here waits for the device: whoever releases a buffer that queued work may still touch synchronises first.
struct DevBufLive { static inline std::atomic<int> buffers{0}; static inline std::atomic<size_t> device_bytes{0}, pinned_bytes{0}; };      // process-wide: ssm_debug_live_allocations
template <class T, bool Pinned = false> class DevBuf {
    T* p = nullptr; size_t nbytes = 0;
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), nbytes(std::exchange(o.nbytes, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); p = std::exchange(o.p, nullptr); nbytes = std::exchange(o.nbytes, 0); } return *this; }
    ~DevBuf() { reset(); }
    operator T*() const { return p; }
    template <class U> U* as() const { return reinterpret_cast<U*>(p); }
    size_t bytes() const { return nbytes; }                     // what alloc asked for; 0: empty
    void reset()
    {
        if (!p) return;
        if (Pinned) (void)hipHostFree(p); else (void)hipFree(p);
        DevBufLive::buffers--; (Pinned ? DevBufLive::pinned_bytes : DevBufLive::device_bytes) -= nbytes;
        p = nullptr; nbytes = 0;
    }
    // SSM_E_NOMEM + the message in c->err (c may be null: no message) when the allocation fails; the buffer is empty then
    int alloc_bytes(ssm_ctx* c, size_t bytes);
    int alloc(ssm_ctx* c, size_t count) { return alloc_bytes(c, (count ? count : 1) * sizeof(std::conditional_t<std::is_void<T>::value, char, T>)); }
};
template <class T> using PinBuf = DevBuf<T, true>;

// Owners of ONE stream / ONE event the library created: move-only, empty by default, converting to the raw handle.  ensure() creates the handle if it is
// missing (streams: hipStreamNonBlocking; events: without timing, for ordering -- the profiling pool asks for timing); reset() and the destructor destroy
// it.  As with DevBuf nothing here waits for the device.  Counted process-wide: ssm_debug_live_handles.
struct HandleLive { static inline std::atomic<int> streams{0}, events{0}; };
class Stream {
    hipStream_t h = nullptr;
public:
    Stream() = default;
    Stream(const Stream&) = delete; Stream& operator=(const Stream&) = delete;
    Stream(Stream&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
    Stream& operator=(Stream&& o) noexcept { if (this != &o) { reset(); h = std::exchange(o.h, nullptr); } return *this; }
    ~Stream() { reset(); }
    operator hipStream_t() const { return h; }
    hipError_t ensure() { if (h) return hipSuccess; const hipError_t e = hipStreamCreateWithFlags(&h, hipStreamNonBlocking); if (e == hipSuccess) HandleLive::streams++; else h = nullptr; return e; }
    void reset() { if (!h) return; (void)hipStreamDestroy(h); HandleLive::streams--; h = nullptr; }
};
class Event {
    hipEvent_t h = nullptr;
public:
    Event() = default;
    Event(const Event&) = delete; Event& operator=(const Event&) = delete;
    Event(Event&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
    Event& operator=(Event&& o) noexcept { if (this != &o) { reset(); h = std::exchange(o.h, nullptr); } return *this; }
    ~Event() { reset(); }
    operator hipEvent_t() const { return h; }
    hipError_t ensure(bool timing = false)
    {
        if (h) return hipSuccess;
        const hipError_t e = timing ? hipEventCreate(&h) : hipEventCreateWithFlags(&h, hipEventDisableTiming);
        if (e == hipSuccess) HandleLive::events++; else h = nullptr;
        return e;
    }
    void reset() { if (!h) return; (void)hipEventDestroy(h); HandleLive::events--; h = nullptr; }
};
// The fan of k_sgbm's forms 0 / 1 (kernels_sgbm.hip sgbm_aggregate): four streams for the scan directions that run beside the caller's stream, forked from and
// joined into it by events on every call, so calls on one lane stay ordered and two lanes never share an event.  Owned by the lane and created at its first
// form-0/1 launch (form 2, the default, needs none); a creation that failed half-way resumes at the next.
struct SgFan {
    Stream s[4]; Event fork, done[4];
    hipError_t ensure()
    {
        hipError_t e = fork.ensure();
        for (int i = 0; i < 4 && e == hipSuccess; i++) { e = s[i].ensure(); if (e == hipSuccess) e = done[i].ensure(); }
        return e;
    }
};
// What belongs to ONE stream of a context: the stream, the event that joins it back into the main stream (lanes_join; unused on the main lane) and the state
// the launchers keep per stream -- passed to them as arguments, created where the lane first needs it.
struct Lane {
    Stream stream; Event joined;
    SgFan sg;                           // k_sgbm, forms 0 / 1
    DevBuf<int> conv_tiles;             // CONV_QUEUE_INTS tile counters of the SegNet conv kernels (ssm_segnet_abi.hip seg_lane_tiles); launches on a stream are ordered, so they share it
};

struct VoxTable {           // tab[slots] | occ[slots] | counter block (32 bytes: count, flags, overflow records, overflow capacity, overflow list address)
    DevBuf<ssm_voxel> tab; uint32_t* occ = nullptr; int32_t* counters = nullptr; int cap_log2 = 0;        // occ, counters: inside tab's allocation
    DevBuf<ssm_voxel> ovf; int ovf_cap = 0;       // the overflow list of the context map (kernels_map.hip vox_overflow_slot); the temporary tables have none
    DevBuf<int32_t> skip;                            // the context map's skip list (kernels_map.hip map_stream2_kernel): blocks of the fused map stage that found the overflow list beyond its high-water mark
    size_t bytes() const { const size_t s = (size_t)1 << cap_log2; return s * sizeof(ssm_voxel) + s * 4 + 32; }
};
// what the context map's protocol (ssm_map_plan.h MapGov) needs on the device and of HIP
struct SSM_HIDDEN MapDev {
    DevBuf<int32_t> redo;                        // the block ids of a redo launch
    PinBuf<int32_t> snap; Event snap_ev[2];      // between the map launches of ssm_seq_process the counters come back through a two-slot ring of asynchronous copies
    std::vector<hipStream_t> launch_streams;     // streams fused launches were queued on
    // the stream that holds the newest work on the context map when that is a side lane of ssm_seq_process (joined into the main stream by an event, so everything queued
    // on the main stream afterwards is ordered behind it): ssm_map_size / ssm_map_export_table_dev read the map there and wait for THAT stream only -- the ORB -> match chain of
    // the call's last sub-batch keeps running.  nullptr: the map's newest work is on the main stream.
    hipStream_t tail = nullptr;
    int own_stream = 1;                          // SSM_MAP_STREAM: two-chain mode runs the map stage on side[1] (0: on the chains' streams in turn)
};
struct StageRec { const char* name; hipEvent_t a, b; };      // a, b: events of the context's profiling pool
// SegNet driving_webdemo: 26 conv layers; op list interleaves pools / unpools
struct SegLayerDef { int cin, cout, h, w; };
static const int SEG_NW = 480, SEG_NH = 360, SEG_NCLS = 12, SEG_LAYERS = 26;
static const SegLayerDef k_seg_layers[SEG_LAYERS] = {
    {3, 64, 360, 480}, {64, 64, 360, 480},                                   // conv1_1 conv1_2 | pool1
    {64, 128, 180, 240}, {128, 128, 180, 240},                               // conv2_x         | pool2
    {128, 256, 90, 120}, {256, 256, 90, 120}, {256, 256, 90, 120},           // conv3_x         | pool3
    {256, 512, 45, 60}, {512, 512, 45, 60}, {512, 512, 45, 60},              // conv4_x         | pool4 (ceil: 23x30)
    {512, 512, 23, 30}, {512, 512, 23, 30}, {512, 512, 23, 30},              // conv5_x         | pool5 (ceil: 12x15)
    {512, 512, 23, 30}, {512, 512, 23, 30}, {512, 512, 23, 30},              // upsample5 | conv5_3_D conv5_2_D conv5_1_D
    {512, 512, 45, 60}, {512, 512, 45, 60}, {512, 256, 45, 60},              // upsample4 | conv4_x_D
    {256, 256, 90, 120}, {256, 256, 90, 120}, {256, 128, 90, 120},           // upsample3 | conv3_x_D
    {128, 128, 180, 240}, {128, 64, 180, 240},                               // upsample2 | conv2_x_D
    {64, 64, 360, 480}, {64, 12, 360, 480}                                   // upsample1 | conv1_2_D conv1_1_D (no BN/ReLU)
};

#define SG_FAIL_WORDS 256
struct StereoState {        // workspace of the stereo path (quad matcher, SGBM depth, stereo VO) for one image geometry, B frames per launch
    int w = 0, h = 0, maxc = 0, B = 0;
    QuadBatch qb{};                          // image slots: 2 sides x (B + 1) pyramids + Scharr derivatives (the kernels' view of pyr, der: stereo_init)
    DevBuf<uint8_t> pyr; DevBuf<int16_t> der;
    GfttWork gw{};                           // goodFeaturesToTrack workspace (kernels_quad.hip): the kernels' view of the buffers below (stereo_init)
    DevBuf<float> g_eig; DevBuf<int> g_cand_at, g_maxord, g_count, g_nkept; DevBuf<uint32_t> g_cand_bits, g_deps; DevBuf<unsigned long long> g_keys, g_kept; DevBuf<uint8_t> g_depn, g_state;
    int keycap = 0; DevBuf<int> ncorner, has_prev;
    DevBuf<int> sg_fail;                     // SG_FAIL_WORDS words: word (sub-batch index mod SG_FAIL_WORDS) is set by that sub-batch's sgbm_sweep when a strip hand-off times out (kernels_sgbm.hip)
    // the depth stage of the most recent sequence call, kept so that sub-batches whose sweep timed out can be repeated in form 1 once the call is known to have
    // failed (ssm_sync / check_device_flags: the caller's input buffers must stay untouched until then, as for any asynchronous call)
    struct { bool valid = false; ssm_stereo_frames_dev in{}; int B = 0; } sg_pending;
    DevBuf<float> pts;                       // [5][B][maxc] (x, y): lc (GFTT corners), rc, rp, lp, lp_direct
    DevBuf<uint8_t> status; DevBuf<float> err;              // ssm_lk_track outputs
    DevBuf<double> tr_all; DevBuf<int32_t> vcount, rand_off, consumed; int vo_iters = 0;   // stereo VO scratch (B x iters hypotheses)
    DevBuf<void> sg_wsN[3]; DevBuf<int> dminN[3];   // SGBM workspaces (sized for the frames per launch actually used): successive sub-batches of a sequence run SGBM on up to three streams, one workspace each
    // sequence outputs (seq_cap frames)
    int seq_cap = 0;
    DevBuf<ssm_pmatch> quad; DevBuf<int32_t> nquad; DevBuf<float> corners; DevBuf<int32_t> ncorners; DevBuf<int16_t> disp; DevBuf<uint16_t> depth;
    DevBuf<double> tr; DevBuf<int32_t> inliers, vo_result;
    bool have_prev = false;                  // slot 0 holds the last frame of the previous sequence call
    bool lk_built = false;                   // slot 1 of both sides holds the pyramids and derivatives of the last ssm_lk_track (ssm_debug_quad_pyramid)
    DevBuf<uint8_t> in_stage;                // device staging of the per-pair host-pointer entry points: PairBlock::stage_bytes (ssm_stereo_abi.hip), up to four packed images
};
struct SegNetState {
    bool set[SEG_LAYERS] = {};
    DevBuf<void> w[SEG_LAYERS]; DevBuf<float> scale[SEG_LAYERS], shift[SEG_LAYERS];
    DevBuf<void> ww[SEG_LAYERS];         // the layer's weights in Winograd F(2, 3) form (kernels_segnet.hip conv3x3_wino_kernel), or null: the direct kernel only
    int cinp[SEG_LAYERS], coutp[SEG_LAYERS], coutstore[SEG_LAYERS];
    int batch = 0;
    DevBuf<void> actA, actB; void* last_logits = nullptr /* actA or actB */; DevBuf<uint8_t> code[5], labels;
    DevBuf<int32_t> pre_xofs, pre_yofs, post_xofs, post_yofs;
    DevBuf<int16_t> pre_xa, pre_ya, post_xa, post_ya;
    DevBuf<uint8_t> d_sem_gen;          // generated colour labels for the sequence path (max_batch frames)
};

// workspace of the ORB front end for B frames (ssm_abi.hip orb_work_alloc): what pyramid .. describe write and read between them
struct OrbWork {
    DevBuf<uint8_t> pyr, blur; DevBuf<int32_t> ncand; int32_t* cellmax = nullptr /* inside ncand's allocation */; DevBuf<cand_t> cand; DevBuf<uint16_t> nodeof;
    DevBuf<uint32_t> sel; DevBuf<int32_t> nsel; DevBuf<uint4> kpaux;
};
// workspace of the semantic-motion fusion (ssm_motion_fuse.hip) for cap_n frames of cap_px pixels; n, w, h: the last call, for ssm_debug_motion_fuse
struct MfWork {
    int cap_n = 0, n = 0, w = 0, h = 0; size_t cap_px = 0;
    DevBuf<uint8_t> always, cand, filled; DevBuf<int32_t> labels, area, overlap, info; PinBuf<int32_t> h_info;
    DevBuf<uint8_t> in_sem, in_motion, out_mask;      // staging of the host-image entry points (one frame)
};
// a key-frame's camera-frame cloud in device memory (ssm_map.hip ssm_backproject_dev; ssm_sor.hip filters it in place): n points at d, carved from cloud_slabs[slab]
// run: the points' run counters of free-space carving (ssm_carve.hip), n bytes made by the cloud's first ssm_carve; empty before
struct ssm_cloud { ssm_point* d = nullptr; int n = 0; int device = 0; int slab = -1; DevBuf<uint8_t> run; };
// a view of free-space carving: a key-frame's depth image in device memory and its camera
struct ssm_carve_view { DevBuf<uint16_t> depth; int w = 0, h = 0, device = 0; ssm_camera cam{}; };
// a render target (ssm_render.hip): the z-buffer and the four images of a w x h view, and the staging of a frame to compare with; rendered: a rendering is in it
struct ssm_render_target {
    int w = 0, h = 0, device = 0; bool rendered = false;
    DevBuf<unsigned long long> keys; DevBuf<uint16_t> depth; DevBuf<uint8_t> bgr, label; DevBuf<int32_t> index;
    DevBuf<uint16_t> f_depth; DevBuf<uint8_t> f_sem, cls;
};
// workspace of map rendering: the info and the comparison's counts
struct RenderWork { DevBuf<int32_t> info; PinBuf<int32_t> h_info; DevBuf<unsigned long long> counts; PinBuf<unsigned long long> h_counts; };
// a grid target (ssm_grid.hip): the raw cells and the seven output arrays for up to cap cells; nx, ny, h_min: the last build's (built: there is one)
struct ssm_grid_target {
    int64_t cap = 0; int nx = 0, ny = 0, device = 0; bool built = false;
    const ssm_ctx* owner = nullptr; ssm_grid_params params{}; int64_t builds = 0, n_in = 0;      // the context that made it; the last build's parameters, number and point count (ssm_objects.hip)
    DevBuf<ssm_grid_cell> cells; DevBuf<uint8_t> cls, ground_label, obstacle_label; DevBuf<int32_t> ground_q, top_q; DevBuf<uint32_t> n, n_high;
};
// workspace of the ground grid: the info
struct GridWork { DevBuf<unsigned long long> info; PinBuf<unsigned long long> h_info; int form = GRID_FORM_DEFAULT; };          // form: ssm_debug_grid_form
// an object target (ssm_objects.hip): the labelling's arrays for up to cap cells, the component and object records (grown by the call that needs more), the
// object_id image.  staged: stage 1 has run (nx, ny, K: its grid and objects); grid, grid_build: the grid target and build it ran on (null: hand-made cells)
struct ssm_objects_target {
    int64_t cap = 0; int nx = 0, ny = 0, device = 0, K = 0; const ssm_ctx* owner = nullptr; bool staged = false;
    const ssm_grid_target* grid = nullptr; int64_t grid_build = 0;
    DevBuf<int32_t> labels, isroot, rank, object_id, keep, kid; DevBuf<uint16_t> loc; DevBuf<uint8_t> tmp; size_t tmp_bytes = 0;
    DevBuf<ssm_object> comp, objs; int32_t comp_cap = 0;
};
// workspace of object extraction: the info, the last stage-2 call's per-point ids (n_ids of them, < 0: none yet), the staging of ssm_debug_objects_cells
struct ObjectsWork {
    DevBuf<unsigned long long> info; PinBuf<unsigned long long> h_info; PinBuf<int32_t> h_count; int form = OBJECTS_FORM_DEFAULT;
    DevBuf<int32_t> ids; int64_t ids_cap = 0, n_ids = -1;
    DevBuf<uint8_t> in_cls, in_label; DevBuf<int32_t> in_ground, in_top; DevBuf<uint32_t> in_high; int64_t in_cap = 0;
};
// a clearance target (ssm_clearance.hip): the column pass's masks and rows, the images and the labels for up to cap cells; staged: a call has run (nx, ny: its grid)
// seed_cell, cell: that call's seed (-1: none) and cell size, what a route field over it starts from (ssm_route.hip)
struct ssm_clearance_target {
    int64_t cap = 0; int nx = 0, ny = 0, device = 0; const ssm_ctx* owner = nullptr; bool staged = false;
    int64_t seed_cell = -1; double cell = 1.0;
    DevBuf<uint32_t> mask, dist2; DevBuf<int32_t> row, nearest, labels; DevBuf<uint8_t> reach;
};
// a route target (ssm_route.hip): the cells' bytes, the dist2 copy, the field and a path's cells for up to cap cells and max_path cells; flag, list: form 1's tile
// marks and active list for tile_cap tiles (grown by the call that needs more).  fielded: a field has run (nx, ny, S, source: its grid, setup and source)
struct ssm_route_target {
    int64_t cap = 0, tile_cap = 0; int nx = 0, ny = 0, device = 0, max_path = 0; const ssm_ctx* owner = nullptr; bool fielded = false;
    ssm_rtc::Setup S{}; int32_t source = -1;
    DevBuf<uint8_t> in; DevBuf<uint32_t> dist2, cost; DevBuf<int32_t> parent, path, rev, flag, list;
};
// workspace of the route field: the info (and the far key behind it), the path info (and the goal's key behind it), the ring of active counts and form 0's changed
// word (ctl[2]), the last field's rounds, the staging of ssm_debug_route_cells
struct RouteWork {
    DevBuf<unsigned long long> info, pinfo; PinBuf<unsigned long long> h_info, h_pinfo; DevBuf<int32_t> ctl; PinBuf<int32_t> h_ctl; int form = ROUTE_FORM_DEFAULT, rounds = 0;
    DevBuf<uint8_t> in_reach; DevBuf<uint32_t> in_dist2; int64_t in_cap = 0;
};
// workspace of the clearance map: the info (and the seed's key behind it), the staging of ssm_debug_clearance_cells
struct ClearanceWork { DevBuf<unsigned long long> info; PinBuf<unsigned long long> h_info; int form = CLEARANCE_FORM_DEFAULT; DevBuf<uint8_t> in_cls; int64_t in_cap = 0; };
// a view of label fusion (ssm_relabel.hip): a key-frame's depth and label images in device memory and its camera; packed: depth | label << 16 per pixel, what
// the vote gathers under the packed form (the default; the depth image is then freed once the view is made), empty under the other (ssm_debug_relabel_form)
struct ssm_relabel_view { DevBuf<uint16_t> depth; DevBuf<uint8_t> label; DevBuf<uint32_t> packed; int w = 0, h = 0, device = 0; const ssm_ctx* owner = nullptr; ssm_camera cam{}; };
// workspace of label fusion for cap points: every point's record of the last device call (n points, n < 0: none yet; ssm_debug_relabel_record), the info, and the
// staging of the host-array call (in_cap points)
struct RelabelWork {
    int cap = 0, n = -1, form = RELABEL_FORM_DEFAULT; size_t in_cap = 0;
    DevBuf<uint64_t> votes; DevBuf<uint32_t> new_label; DevBuf<unsigned long long> info; PinBuf<unsigned long long> h_info; DevBuf<ssm_point> in;
};
// a view of dense alignment (ssm_align.hip): a key-frame's depth image and its normal map (16 bytes per pixel) in device memory, its camera and edge gate
struct ssm_align_view { DevBuf<uint16_t> depth; DevBuf<uint8_t> normals; int w = 0, h = 0, device = 0; ssm_camera cam{}; double tol_abs = 0; int32_t tol_rel_ppm = 0; };
// workspace of dense alignment: one slot of sums per iteration, and the last device call's iterations (ssm_debug_align_record)
struct AlignWork { DevBuf<unsigned long long> sums; PinBuf<unsigned long long> h_sums; std::vector<ssm_align_iter> record; };
// workspace of free-space carving (ssm_carve.hip) for cap points in cap_m clouds; off: the last call's clouds as numbers of their first points (m + 1 entries), for
// ssm_debug_carve_record
struct CarveWork {
    int cap = 0, cap_m = 0; std::vector<int> off;
    DevBuf<int32_t> info; PinBuf<int32_t> h_info; DevBuf<uint32_t> base, block_cnt, block_off; DevBuf<uint8_t> verdict, run_new, keep, tmp_run, tmp; size_t tmp_bytes = 0;
    DevBuf<ssm_point> tmp_pts;
    DevBuf<uint8_t> run_in; DevBuf<uint16_t> depth; size_t run_cap = 0, depth_cap = 0;      // the host-array call's staging beside CloudTableWork::in
};
// The cloud-segment table (cloud_table.h) of the context, for carving, rendering and alignment alike: CloudSeg[m], then the blocks' first clouds, in device memory
// and its pinned mirror, cap bytes each; in: the staging of the points of a host-array call (in_cap points).  Grown by the largest call (ssm_cloud_list.hip).
struct CloudTableWork { size_t cap = 0, in_cap = 0; DevBuf<uint8_t> table; PinBuf<uint8_t> h_table; DevBuf<ssm_point> in; };
// A call's table on the device, as the launchers take it.  in_flight: the stream its upload was queued on, until the call has waited there and says so (null) --
// a return on an error path in between waits here, so the pinned mirror is never rewritten under a copy in flight
struct CloudTable { const CloudSeg* seg; const int32_t* blk; int64_t total, blocks; hipStream_t in_flight = nullptr; ~CloudTable() { if (in_flight) (void)hipStreamSynchronize(in_flight); } };
// workspace of the statistical outlier removal (ssm_sor.hip) for cap points; n: the last call, for ssm_debug_sor_record
struct SorWork {
    int cap = 0, n = 0;
    int levels = 0, level_q[24] = {};      // the last call's ladder: points unsettled when each level began (ssm_debug_sor_levels)
    DevBuf<SorHead> head; PinBuf<SorHead> h_head; DevBuf<float> mean_dist; DevBuf<uint8_t> settled, keep, flags; DevBuf<uint64_t> keys_a, keys_b;
    DevBuf<uint32_t> idx_a, idx_b, query, block_cnt, block_off; DevBuf<float4> sorted; DevBuf<uint8_t> tmp; size_t tmp_bytes = 0;
    DevBuf<ssm_point> in, out;      // the host-array call's staging; out also holds ssm_cloud_sor's kept points before they go back into the cloud
};
// one ORB -> match chain of ssm_seq_process: its workspace, and the event behind its newest ORB + expand (what later sub-batches' matchers wait for)
struct OrbChain { OrbWork work; Event orb_done; };

struct ssm_ctx {
    std::mutex mu;
    int device = 0;
    DeviceInfo dev;                     // CU count and LDS limit of `device`, asked once (ctx_init): what the launchers size grids and dynamic LDS from
    // main: the context's stream, created in ctx_init and never re-pointed; every per-call entry point runs here.
    // side[]: created at first use (ensure_side_streams), forked from and joined into main by every call that uses them (lanes_fork / lanes_join).  Who runs
    // on which: ssm_seq_plan.h SeqLane.
    Lane main, side[3]; Event forked; bool side_ready = false /* ensure_side_streams completed */;
    ssm_config cfg{};
    OrbPlan plan;                       // what cfg fixes of the ORB front end (ssm_orb_plan.h), built by ssm_create; ctx_init uploads its tables
    const OrbGeom& g = plan.g;          // its geometry, under the name every launcher reads
    std::string err;
    int B = 1, R = 5;
    // constant tables
    DevBuf<uint8_t> d_blur_tab; bool blur_mfma = true;                // blur_mfma_kernel's coefficient fragments (kernels_orb.hip); SSM_BLUR_VARIANT=0: the VALU kernel
    DevBuf<int8_t> d_pattern; DevBuf<float> d_pattern_f;            // the BRIEF table as given, and as floats for brief_kernel
    DevBuf<int32_t> d_xofs[SSM_MAX_LEVELS], d_yofs[SSM_MAX_LEVELS]; DevBuf<int16_t> d_xa[SSM_MAX_LEVELS], d_ya[SSM_MAX_LEVELS];
    DevBuf<uint32_t> d_xgrp[SSM_MAX_LEVELS];     // resize4_kernel's per-group constants (null: the level uses the general resize kernel)
    DevBuf<uint32_t> d_xgrp8[SSM_MAX_LEVELS];    // the fused pyramid's 8-pixel groups (null: the level's groups do not fit that layout; it keeps the 4-pixel item)
    // the per-level tables above as the plain pointer arrays the pyramid launchers take (filled where the tables are uploaded: ctx_init)
    struct { const int32_t *xofs[SSM_MAX_LEVELS], *yofs[SSM_MAX_LEVELS]; const int16_t *xa[SSM_MAX_LEVELS], *ya[SSM_MAX_LEVELS]; const void *xgrp[SSM_MAX_LEVELS], *xgrp8[SSM_MAX_LEVELS]; } pyr_tabs = {};
    PyrBandPlan pyr_bands, pyr_bands1;       // resize4_kernel_bands for batches / for the per-frame call (bands == 0: gray_kernel + k_pyramid)
    DevBuf<int32_t> d_band_tab, d_band_tab1; // their band tables (PyrBandPlan::d_tab points here)
    // the ORB -> match chains (a workspace of B frames each): chain[0] serves every entry point that runs on the main lane; ssm_seq_process runs successive
    // sub-batches on up to three chains, each on its own lane (ssm_seq_plan.h); the workspaces of chains 1, 2 are allocated at first use
    OrbChain chain[3];
    DevBuf<int32_t> d_status;           // the ORB scratch-overflow word: one, shared by all chains
    DevBuf<uint8_t> d_mask; DevBuf<int32_t> d_chunk_cnt; DevBuf<int64_t> d_chunk_off, d_total;
    DevBuf<ssm_point> d_points;
    DevBuf<ssm_point> d_vmap; int vmap_n = 0;    // Mapper::viewer's filtered map, device-resident (ssm_viewer_map_update)
    DevBuf<ssm_point> d_vcat;                    // its concatenation buffer
    struct CloudSlab { DevBuf<ssm_point> d; size_t cap = 0, used = 0; int live = 0; };
    bool viewer_fail_next = false;                                           // tests: the next ssm_viewer_map_update fails (ssm_viewer_map_release)
    std::vector<CloudSlab> cloud_slabs;                                      // key-frame clouds (ssm_backproject_dev) are carved from slabs: no hipMalloc per cloud
    // staging for the host-pointer entry points (one frame) + generic scratch
    DevBuf<uint8_t> d_in_img, d_in_sem; DevBuf<uint16_t> d_in_depth; DevBuf<double> d_in_pose;
    DevBuf<uint8_t> d_scratch;
    DevBuf<unsigned long long> d_pnp_xchg; unsigned pnp_epoch = 0;   // ssm_pnp_solve's cluster: the exchange ring (persistent) and the launch number its pass tags start from
    bool pnp_solve_one_block = false;                        // ssm_pnp_solve: a cluster of eight blocks timed out once -> one block per solve from then on
    DevBuf<uint8_t> d_scratch2;
    // sequence outputs
    int seq_cap = 0, prev_n = -1;
    DevBuf<ssm_keypoint> d_kps; DevBuf<uint8_t> d_desc_all; DevBuf<int32_t> d_nkp_all; DevBuf<float> d_pos3d;
    DevBuf<ssm_dmatch> d_matches; DevBuf<int32_t> d_nmatch, d_match_pend, d_npoints; DevBuf<uint8_t> d_hist_tmp;
    DevBuf<uint8_t> d_exp_q, d_exp_t, d_knn; int capT = 0; bool match_mfma = true;   // the matcher's expanded descriptor rows (kernels_match.hip)
    // voxel tables
    MapDiv map_div{}; bool map_div_exact = false;          // cfg.camera's reciprocals and whether the fused map stage may divide by them (k_map_div, once: ctx_init)
    VoxTable map, tmp;
    MapGov gov; MapDev mapdev;                              // the context map grows (map_settle): its protocol's host state, and what that needs of the device
    // multi-GPU: the communicator of ssm_comm_init_rank (one rank per context / GPU) and the gathered counts
    ncclComm_t comm = nullptr; int comm_rank = 0, comm_size = 1; DevBuf<int32_t> d_comm_counts; int comm_counts_cap = 0;
    // SegNet
    std::unique_ptr<SegNetState> seg;
    // quad matcher
    std::unique_ptr<StereoState> stereo; int stereo_B = 16; int stereo_sgbm_streams = 2;      // ssm_config.sgbm_streams 
    int sgbm_form_cfg = 0; long sgbm_fallbacks = 0;                                              // ssm_config.sgbm_form; sub-batches repeated in form 1 after a sweep time-out
    MfWork mf;                                               // semantic-motion fusion: allocated by its first call
    SorWork sor;                                             // statistical outlier removal: allocated by its first call, grown by the largest
    CarveWork carve;                                         // free-space carving: likewise
    RenderWork render;                                       // map rendering: likewise
    AlignWork align;                                         // dense alignment: likewise
    GridWork grid;                                           // ground grid: likewise
    ObjectsWork objects;                                     // object extraction: likewise
    ClearanceWork clearance;                                 // clearance map: likewise
    RouteWork route;                                         // route field: likewise
    RelabelWork relabel;                                     // label fusion: likewise
    CloudTableWork clouds;                                   // the cloud table and host-array staging of the three: likewise
    double vt_level_ms[10] = {0}, vt_total_ms = -1.0;     // wall time of the last ssm_vocab_train per level and in all (ssm_debug_vocab_train_times); < 0: none yet
    // profiling
    bool profiling = false;
    PinBuf<uint8_t> h_pinned;          // host staging for the image-sized host-pointer calls (pageable hipMemcpy is ~1 GB/s)
    // the per-frame entry points (ssm_orb_extract[_async], ssm_match[_async]): a ring of pinned host memory (inputs staged, results landed) and a ring of
    // device memory (result blocks), bump-allocated per call and released by ssm_wait; `pending` = what ssm_wait still has to hand to the callers
    PinBuf<uint8_t> h_ring; DevBuf<uint8_t> d_ring /* both of d_ring.bytes() */; size_t h_ring_off = 0, d_ring_off = 0;
    std::vector<std::function<int(ssm_ctx*)>> pending;
    bool serialize = false;             // profiling mode 2: keep the side work of ssm_seq_process on the context stream (clean per-stage times)
    std::vector<StageRec> recs; std::vector<Event> pool; size_t pool_used = 0;
    std::vector<std::string> stage_names; std::vector<float> stage_ms; std::vector<int> stage_launches;
};

inline Lane& lane(ssm_ctx* c, SeqLane l) { return l == LANE_MAIN ? c->main : c->side[l - LANE_SIDE0]; }

#define FAIL(ctx, code, msg) do { (ctx)->err = (msg); return (code); } while (0)
#define HIPCHK(ctx, expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) { (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e__); return SSM_E_HIP; } } while (0)

#define DALLOC(ctx, buf, n) do { int r__ = (buf).alloc(ctx, (size_t)(n)); if (r__) return r__; } while (0)
#define NCCLCHK(ctx, expr) do { ncclResult_t e__ = (expr); if (e__ != ncclSuccess) { (ctx)->err = std::string(#expr) + ": " + ncclGetErrorString(e__); return SSM_E_COMM; } } while (0)
template <class T, bool Pinned> int DevBuf<T, Pinned>::alloc_bytes(ssm_ctx* c, size_t bytes)
{
    reset();
    void* q = nullptr;
    const hipError_t e = Pinned ? hipHostMalloc(&q, bytes, hipHostMallocDefault) : hipMalloc(&q, bytes);
    if (e != hipSuccess) { if (c) c->err = std::string(Pinned ? "hipHostMalloc(" : "hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e); return SSM_E_NOMEM; }
    p = static_cast<T*>(q); nbytes = bytes;
    DevBufLive::buffers++; (Pinned ? DevBufLive::pinned_bytes : DevBufLive::device_bytes) += bytes;
    return SSM_OK;
}
// ssm_cloud_list.hip.  cloud_list: a call's device clouds or, with clouds null, host arrays (pts, n: counts the caller has checked; queued into the context's
// staging) -> segs with pts, n (the points used: every stride-th), stride and M filled.  Per cloud, in this order: null, a cloud of another device, the same cloud
// twice (twice_msg; null: allowed), its pose.  cloud_table_upload: numbers segs, builds the table for blocks of T points and queues its upload -> *t
SSM_HIDDEN int cloud_list(ssm_ctx* c, const char* twice_msg, const double* T_view, ssm_cloud* const* clouds, const ssm_point* const* pts, const int32_t* n,
                          const double* T_clouds, int m, int stride, std::vector<CloudSeg>& segs);
SSM_HIDDEN int cloud_table_upload(ssm_ctx* c, std::vector<CloudSeg>& segs, int T, CloudTable* t);
// ssm_abi.hip
extern SSM_HIDDEN thread_local std::string g_create_err;
SSM_HIDDEN int ensure_scratch(ssm_ctx* c, size_t bytes, DevBuf<uint8_t>* buf = nullptr);     // buf: c->d_scratch (the default) or c->d_scratch2
SSM_HIDDEN int ensure_pinned(ssm_ctx* c, size_t bytes);
SSM_HIDDEN void prof_begin(ssm_ctx* c, hipStream_t s, const char* name);     // s: the stream the stage's kernels run on
SSM_HIDDEN void prof_end(ssm_ctx* c, hipStream_t s);
SSM_HIDDEN void prof_reset(ssm_ctx* c);                     // a profiling context forgets the stages of the previous call: ssm_get_stage_times then reports this one
SSM_HIDDEN int check_device_flags(ssm_ctx* c, bool with_map);
SSM_HIDDEN int wait_pending(ssm_ctx* c);
SSM_HIDDEN bool host_is_pinned(const void* p);             // page-locked host memory (ssm_host_alloc, hipHostRegister)?
SSM_HIDDEN int ensure_side_streams(ssm_ctx* c);
// fork: the listed side lanes wait for everything queued on the main stream so far; join: the main stream waits for everything queued on them
SSM_HIDDEN int lanes_fork(ssm_ctx* c, const LaneList& lanes);
SSM_HIDDEN int lanes_join(ssm_ctx* c, const LaneList& lanes);
// ssm_map.hip
SSM_HIDDEN int table_alloc(ssm_ctx* c, hipStream_t s, VoxTable& t, int cap_log2, const VoxTable* lists = nullptr);      // lists: the table whose overflow list the counter block names (default: t's own)
SSM_HIDDEN int map_settle(ssm_ctx* c, hipStream_t s, int64_t reserve, int32_t* counters_out = nullptr);
SSM_HIDDEN int map_before_launch(ssm_ctx* c, hipStream_t s, int remaining, int* nq);
SSM_HIDDEN int map_after_launch(ssm_ctx* c, hipStream_t s, int frames, bool inputs_volatile);
SSM_HIDDEN int map_fuse_launch(ssm_ctx* c, hipStream_t s, const MapLaunch& L);      // one launch of the fused map stage on the context map, recorded for a redo
inline void map_on_main(ssm_ctx* c) { c->mapdev.tail = nullptr; }      // the context stream has joined the map's side stream: from here the map's newest work is on it
// ssm_segnet_abi.hip
SSM_HIDDEN int seg_init(ssm_ctx* c);
SSM_HIDDEN int seg_forward_dev(ssm_ctx* c, Lane& lane, const uint8_t* bgr, int n, uint8_t* labels_net, uint8_t* sem_bgr, int flags);
// ssm_stereo_abi.hip
SSM_HIDDEN int sgbm_recover(ssm_ctx* c);
// ssm_sor.hip: the filter on n points in device memory, from the first launch to the call's last wait; the kept points are in c->sor.out, their number in info->n_kept
SSM_HIDDEN int sor_run(ssm_ctx* c, const ssm_point* d_pts, int n, const ssm_sor_params* params, ssm_sor_info* info);
// ssm_motion_fuse.hip: the fusion of n device frames queued on the main stream (no wait); motion_host: one frame's motion mask on the host, staged first (n == 1);
// both null: no motion.  The counters stay in c->mf.info
SSM_HIDDEN int mf_enqueue(ssm_ctx* c, const uint8_t* sem_dev, const uint8_t* motion_dev, const uint8_t* motion_host, int n, int w, int h,
                          const ssm_motion_fuse_params* params, uint8_t* mask_dev);
