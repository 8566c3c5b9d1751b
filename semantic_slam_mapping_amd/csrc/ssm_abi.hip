// ssm_abi.hip -- host side of libssm_hip.so: context, device workspace and the extern "C" entry points (the ORB geometry and plan: ssm_orb_plan.cpp)
// declared in include/ssm_hip.h.  No computation of the path happens on the host: this file only sizes buffers,
// moves caller data and enqueues the kernels of kernels_*.hip on the context stream.  There is NO CPU fallback: if
// HIP is unusable ssm_create fails with SSM_E_NODEVICE / SSM_E_HIP.
#include "ssm_ctx.h"
#include "ssm_host.h"
#include "match_keys.h"
#include <set>

static const int8_t k_default_pattern[1024] = {
#include "orb_pattern.inc"
};
thread_local std::string g_create_err;
// the error path and the lock of the host-only sources (ssm_host.h), which do not know the context
int host_fail(ssm_ctx* c, int code, const std::string& msg) { if (c) c->err = msg; else g_create_err = msg; return code; }
std::unique_lock<std::mutex> host_lock(ssm_ctx* c) { return c ? std::unique_lock<std::mutex>(c->mu) : std::unique_lock<std::mutex>(); }

// ---------------------------------------------------------------- helpers
int ensure_scratch(ssm_ctx* c, size_t bytes, DevBuf<uint8_t>* buf)
{
    DevBuf<uint8_t>& b = buf ? *buf : c->d_scratch;
    if (bytes <= b.bytes()) return SSM_OK;
    if (b) hipStreamSynchronize(c->main.stream);
    return b.alloc(c, bytes);
}
int ensure_pinned(ssm_ctx* c, size_t bytes)
{
    if (bytes <= c->h_pinned.bytes()) return SSM_OK;
    if (c->h_pinned) hipStreamSynchronize(c->main.stream);
    if (c->h_pinned.alloc(c, bytes)) FAIL(c, SSM_E_HIP, "hipHostMalloc failed");
    return SSM_OK;
}
void prof_begin(ssm_ctx* c, hipStream_t s, const char* name)
{
    if (!c->profiling) return;
    auto get = [&]() -> hipEvent_t { if (c->pool_used == c->pool.size()) { c->pool.emplace_back(); (void)c->pool.back().ensure(true); } return c->pool[c->pool_used++]; };
    StageRec r; r.name = name; r.a = get(); r.b = get();
    hipEventRecord(r.a, s);
    c->recs.push_back(r);
}
void prof_end(ssm_ctx* c, hipStream_t s) { if (c->profiling) hipEventRecord(c->recs.back().b, s); }
void prof_reset(ssm_ctx* c) { if (c->profiling) { c->recs.clear(); c->pool_used = 0; } }
hipError_t allow_dynamic_lds(const void* fn, size_t bytes, int limit)
{
    if (bytes <= 48 * 1024) return hipSuccess;
    static std::mutex mu; static std::set<std::pair<int, const void*>> done;
    int dev = 0; (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(mu);
    if (done.count({dev, fn})) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, limit);
    if (e == hipSuccess) done.insert({dev, fn});
    return e;
}

// ORB scratch overflow (d_status) is checked after every ORB entry point; the voxel-table-full flag (counters[1]) belongs to the MAP entry points
// (ssm_sync after ssm_seq_process, ssm_map_*): it is reported once, so that one overflowing call does not fail every later call on the
// context (the map then lacks the dropped points: ssm_map_clear / a larger voxel_capacity_log2 is the remedy the message names)
int check_device_flags(ssm_ctx* c, bool with_map)
{
    int32_t st = 0, cnt[2] = {0, 0};
    HIPCHK(c, hipMemcpy(&st, c->d_status, 4, hipMemcpyDeviceToHost));
    if (st) { hipMemset(c->d_status, 0, 4); FAIL(c, SSM_E_CAPACITY, "ORB scratch capacity exceeded (status " + std::to_string(st) + ")"); }
    if (c->stereo) {
        if (c->stereo->sg_fail) { const int r = sgbm_recover(c); if (r) return r; }
    }
    if (with_map) {
        { const int r = map_settle(c, c->main.stream, 0); if (r) return r; }
        HIPCHK(c, hipMemcpy(cnt, c->map.counters, 8, hipMemcpyDeviceToHost));
        if (cnt[1]) {
            // bit 1 (skipped points: a defined contract, DESIGN.md "voxel key range") is reported once and cleared.  Bit 0 (table full: points were DROPPED,
            // the map is incomplete) stays set on the device until ssm_map_clear, so that ssm_map_size / ssm_map_export* / ssm_voxel_allgather keep
            // refusing the incomplete map (and every rank of an all-gather sees it); this function reports it once per fill.
            if (cnt[1] & 2) { const int32_t keep = cnt[1] & 1; hipMemcpy(c->map.counters + 1, &keep, 4, hipMemcpyHostToDevice); }
            if ((cnt[1] & 1) && !c->gov.full_reported) {
                c->gov.full_reported = true;
                FAIL(c, SSM_E_CAPACITY, "voxel map: contributions were dropped (table and overflow list full between two growth checks): ssm_map_clear and start from a larger voxel_capacity_log2");
            }
            if (cnt[1] & 2) FAIL(c, SSM_E_VOXEL_RANGE, "points with a non-finite coordinate or a voxel index outside (-2^20, 2^20) were skipped (leaf too small for the extent, or a bad pose)");
        }
    }
    return SSM_OK;
}

// ---------------------------------------------------------------- lifecycle
extern "C" void ssm_config_default(ssm_config* c)
{
    memset(c, 0, sizeof(*c));
    c->width = 640; c->height = 480;
    c->orb_features = 2000; c->orb_scale = 1.2f; c->orb_levels = 8; c->orb_iniThFAST = 20; c->orb_minThFAST = 7;   // parameters.txt:66-71
    c->knn_match_ratio = 0.8; c->tracker_ref_frames = 5;                                                            // :72,:81
    c->mapper_resolution = 0.1; c->mapper_max_distance = 40;                                                        // :97-98
    c->camera.cx = 318.6; c->camera.cy = 255.3; c->camera.fx = 517.3; c->camera.fy = 516.5; c->camera.scale = 1000.0;
    c->max_batch = 16; c->voxel_capacity_log2 = 20; c->brief_pattern = nullptr;
    c->voxel_max_capacity_log2 = 28; c->sgbm_form = 0; c->sgbm_streams = 0; c->stereo_batch = 0;
}
extern "C" const char* ssm_version(void) { return "ssm_hip 0.1 (gfx950)"; }
extern "C" const char* ssm_last_error(const ssm_ctx* c) { return c ? c->err.c_str() : g_create_err.c_str(); }

// an ORB workspace for the context's B frames; complete once kpaux is set (ensure_alt)
static int orb_work_alloc(ssm_ctx* c, OrbWork& w)
{
    const OrbGeom& g = c->g; const int B = c->B;
    // pyr + 16: resize4_kernel's 8-byte windows may end past the last row
    DALLOC(c, w.pyr, (size_t)B * g.pyr_bytes + 16); DALLOC(c, w.blur, (size_t)B * g.blur_bytes);
    // the per-level candidate counters and the cell maxima (+ k_fast's retry list) share ONE allocation, counters first: k_fast zeroes both with one fill
    DALLOC(c, w.ncand, k_fast_ncand_pad(B, g) + k_fast_cellmax_ints(B, g)); w.cellmax = w.ncand + k_fast_ncand_pad(B, g);
    DALLOC(c, w.cand, (size_t)B * g.cand_total); DALLOC(c, w.nodeof, (size_t)B * g.cand_total);
    DALLOC(c, w.sel, (size_t)B * g.sel_total); DALLOC(c, w.nsel, (size_t)B * g.nlevels);
    DALLOC(c, w.kpaux, (size_t)B * g.sel_total * 2);             // KpAux + KpRec per slot
    return SSM_OK;
}
// a device buffer of the vector's size, holding its elements
template <class T> static int upload(ssm_ctx* c, DevBuf<T>& d, const std::vector<T>& v)
{
    DALLOC(c, d, v.size());
    HIPCHK(c, hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return SSM_OK;
}
#define UPLOAD(ctx, buf, vec) do { int r__ = upload(ctx, buf, vec); if (r__) return r__; } while (0)
// the streams, the plan's tables on the device (ssm_orb_plan.h OrbPlan, built by ssm_create) and the workspaces
static int ctx_init(ssm_ctx* c)
{
    const ssm_config& cfg = c->cfg; const OrbPlan& P = c->plan; const OrbGeom& g = c->g; const int B = c->B, W = g.W, H = g.H;
    HIPCHK(c, c->main.stream.ensure());
    c->dev.id = c->device;             // (a failed query keeps DeviceInfo's fall-back)
    { int v = 0; if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, c->device) == hipSuccess && v > 0) c->dev.cus = v; }
    { int v = 0; if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device) == hipSuccess && v > 0) c->dev.max_lds = v; }
    c->map_div_exact = k_map_div(cfg.camera, c->map_div);
    const int8_t* pat = cfg.brief_pattern ? cfg.brief_pattern : k_default_pattern;
    { const char* e = getenv("SSM_BLUR_VARIANT"); c->blur_mfma = !(e && atoi(e) == 0); }
    UPLOAD(c, c->d_pattern, std::vector<int8_t>(pat, pat + 1024));
    UPLOAD(c, c->d_blur_tab, P.blur_tab);
    UPLOAD(c, c->d_pattern_f, std::vector<float>(pat, pat + 1024));
    for (int l = 1; l < g.nlevels; l++) {
        UPLOAD(c, c->d_xofs[l], P.xofs[l]); UPLOAD(c, c->d_xa[l], P.xa[l]); UPLOAD(c, c->d_yofs[l], P.yofs[l]); UPLOAD(c, c->d_ya[l], P.ya[l]);
        if (P.streaming[l]) UPLOAD(c, c->d_xgrp[l], P.xgrp[l]);
        if (P.wide_ok[l]) UPLOAD(c, c->d_xgrp8[l], P.xgrp8[l]);
        auto& T = c->pyr_tabs;
        T.xofs[l] = c->d_xofs[l]; T.xa[l] = c->d_xa[l]; T.yofs[l] = c->d_yofs[l]; T.ya[l] = c->d_ya[l]; T.xgrp[l] = c->d_xgrp[l]; T.xgrp8[l] = c->d_xgrp8[l];
    }
    // the fused pyramid's band tables (none where a level needs the general resize kernel)
    for (int k = 0; k < 2; k++) {
        PyrBandPlan& p = k ? c->pyr_bands1 : c->pyr_bands; DevBuf<int32_t>& d = k ? c->d_band_tab1 : c->d_band_tab;
        p = P.bands[k];
        if (!p.bands) continue;
        UPLOAD(c, d, P.band_tab[k]);
        p.d_tab = d;
    }
    { const int r = orb_work_alloc(c, c->chain[0].work); if (r) return r; }
    DALLOC(c, c->d_status, 1); HIPCHK(c, hipMemset(c->d_status, 0, 4));
    const int chunks = backproject_chunks(W, H);
    DALLOC(c, c->d_mask, (size_t)B * W * H); DALLOC(c, c->d_chunk_cnt, (size_t)B * chunks); DALLOC(c, c->d_chunk_off, (size_t)B * chunks);
    DALLOC(c, c->d_total, 2); DALLOC(c, c->d_points, (size_t)B * W * H);
    DALLOC(c, c->d_in_img, (size_t)W * H * 3); DALLOC(c, c->d_in_sem, (size_t)W * H * 3); DALLOC(c, c->d_in_depth, (size_t)W * H); DALLOC(c, c->d_in_pose, 16);
    DALLOC(c, c->map.ovf, VOX_OVF_RECORDS); c->map.ovf_cap = VOX_OVF_RECORDS;
    if (c->mapdev.snap.alloc(c, 16)) FAIL(c, SSM_E_HIP, "hipHostMalloc of the map counter ring failed");
    memset(c->mapdev.snap, 0, 64);
    for (int k = 0; k < 2; k++) HIPCHK(c, c->mapdev.snap_ev[k].ensure());
    c->gov.dims.skip_cap = k_map_fuse_skip_cap(); c->gov.dims.block_records = k_map_fuse_block_records(); c->gov.dims.resident_blocks = k_map_fuse_resident_blocks();
    int r = table_alloc(c, c->main.stream, c->map, cfg.voxel_capacity_log2); if (r) return r;
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    return SSM_OK;
}
extern "C" int ssm_create(int device, const ssm_config* cfg, ssm_ctx** out)
{
    if (!cfg || !out) { g_create_err = "null argument"; return SSM_E_INVAL; }
    *out = nullptr;
    // brief_kernel stages the rows and columns -18 .. +18 around a keypoint: a pattern point (x, y) turned by any angle lands on a coordinate of at most
    // sqrt(x^2 + y^2), which rounds to at most 18 while x^2 + y^2 <= 342 (sqrt(342) = 18.493).  Checked first: no device is needed to refuse a table
    if (cfg->brief_pattern)
        for (int i = 0; i < 512; i++) {
            const int x = cfg->brief_pattern[2 * i], y = cfg->brief_pattern[2 * i + 1];
            if (x * x + y * y > SSM_BRIEF_MAX_R2) {
                g_create_err = "brief_pattern point " + std::to_string(i) + " (" + std::to_string(x) + ", " + std::to_string(y) + "): x^2 + y^2 must be <= " + std::to_string(SSM_BRIEF_MAX_R2);
                return SSM_E_INVAL;
            }
        }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) { g_create_err = std::string("no HIP device: ") + hipGetErrorString(e); return SSM_E_NODEVICE; }
    if (device < 0 || device >= ndev) { g_create_err = "device index out of range"; return SSM_E_INVAL; }
    if ((e = hipSetDevice(device)) != hipSuccess) { g_create_err = std::string("hipSetDevice: ") + hipGetErrorString(e); return SSM_E_HIP; }
    ssm_ctx* c = new ssm_ctx();
    c->device = device; c->cfg = *cfg;
    // the stereo path's knobs come from the configuration (two contexts of a process may differ); the environment variables remain as overrides for ablation runs
    { int b = cfg->stereo_batch > 0 ? cfg->stereo_batch : (cfg->max_batch > 0 ? cfg->max_batch : 1); c->stereo_B = b < 1 ? 1 : b > 128 ? 128 : b; }
    { const int v = cfg->sgbm_streams; if (v > 0) c->stereo_sgbm_streams = v > 3 ? 3 : v; }
    c->sgbm_form_cfg = cfg->sgbm_form;
    { const char* e = getenv("SSM_MAP_STREAM"); c->mapdev.own_stream = e ? atoi(e) : 1; }
    { const char* e = getenv("SSM_MATCH_VARIANT"); c->match_mfma = !(e && atoi(e) == 0); }      // 0: the VALU matcher in the sequence path (A/B runs)
    c->B = cfg->max_batch > 0 ? cfg->max_batch : 1; c->R = cfg->tracker_ref_frames > 0 ? cfg->tracker_ref_frames : 1;
    int r = orb_plan_build(*cfg, c->plan, c->err);
    if (!r && (cfg->voxel_capacity_log2 < 8 || cfg->voxel_capacity_log2 > 28)) { c->err = "voxel_capacity_log2 must be 8..28"; r = SSM_E_INVAL; }
    if (!r && cfg->voxel_max_capacity_log2 != 0 && (cfg->voxel_max_capacity_log2 < cfg->voxel_capacity_log2 || cfg->voxel_max_capacity_log2 > 28)) { c->err = "voxel_max_capacity_log2 must be voxel_capacity_log2..28 (0: 28)"; r = SSM_E_INVAL; }
    if (!r) c->gov.vox_max_log2 = cfg->voxel_max_capacity_log2 ? cfg->voxel_max_capacity_log2 : 28;
    if (!r && !(cfg->mapper_resolution > 0)) { c->err = "mapper_resolution must be > 0"; r = SSM_E_INVAL; }
    if (!r && (cfg->sgbm_form < 0 || cfg->sgbm_form > 3 || cfg->sgbm_streams < 0 || cfg->sgbm_streams > 3 || cfg->stereo_batch < 0)) { c->err = "sgbm_form must be 0..3, sgbm_streams 0..3, stereo_batch >= 0"; r = SSM_E_INVAL; }
    if (!r && c->B > 16384) { c->err = "max_batch must be <= 16384"; r = SSM_E_INVAL; }
    if (!r) r = ctx_init(c);
    if (r) { g_create_err = c->err; ssm_destroy(c); return r; }
    c->cfg.brief_pattern = nullptr;
    *out = c;
    return SSM_OK;
}
// What a destructor cannot order: the device is drained before anything goes (no buffer, stream or event is released while a stream of the context can still
// touch it) and the communicator is torn down; `delete c` then releases every stream, event and buffer the context, its lanes, its StereoState and its
// SegNetState own.  The context's device stays current until it returns.
extern "C" void ssm_destroy(ssm_ctx* c)
{
    if (!c) return;
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    if (c->comm) { ncclCommDestroy(c->comm); c->comm = nullptr; }
    delete c;
}
void ssm_internal_get_config(const ssm_ctx* c, ssm_config* out) { *out = c->cfg; }
int ssm_internal_get_device(const ssm_ctx* c) { return c->device; }
extern "C" int ssm_orb_capacity(const ssm_ctx* c) { return c ? c->g.cap : 0; }
extern "C" void* ssm_stream(ssm_ctx* c) { return c ? (void*)c->main.stream : nullptr; }
extern "C" int ssm_sync(ssm_ctx* c)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    hipSetDevice(c->device);
    c->err.clear();                                               // (after a successful ssm_sync ssm_last_error is empty, or the note of a repeated SGBM sweep)
    { int r = wait_pending(c); if (r) return r; }                 // asynchronous per-frame calls still in flight are completed (their results delivered) too
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    map_on_main(c);                                               // (every stream of the context is idle)
    return check_device_flags(c, true);
}
extern "C" int ssm_set_profiling(ssm_ctx* c, int on) { if (!c) return SSM_E_INVAL; std::lock_guard<std::mutex> lk(c->mu); c->profiling = on != 0; c->serialize = on == 2; return SSM_OK; }
extern "C" int ssm_get_stage_times(ssm_ctx* c, const char** names, float* ms, int* launches, int cap, int* n_out)
{
    if (!c || !n_out) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    hipSetDevice(c->device);
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    c->stage_names.clear(); c->stage_ms.clear(); c->stage_launches.clear();
    for (const StageRec& r : c->recs) {
        float t = 0.f; hipEventElapsedTime(&t, r.a, r.b);
        size_t i = 0;
        for (; i < c->stage_names.size(); i++) if (c->stage_names[i] == r.name) break;
        if (i == c->stage_names.size()) { c->stage_names.push_back(r.name); c->stage_ms.push_back(0.f); c->stage_launches.push_back(0); }
        c->stage_ms[i] += t; c->stage_launches[i] += 1;
    }
    const int n = (int)c->stage_names.size();
    *n_out = n;
    for (int i = 0; i < n && i < cap; i++) { if (names) names[i] = c->stage_names[i].c_str(); if (ms) ms[i] = c->stage_ms[i]; if (launches) launches[i] = c->stage_launches[i]; }
    return SSM_OK;
}

// The side lanes (ssm_ctx::side) are created at first use, not with the context: HIP spreads streams over a few hardware queues in creation order, and a
// context that only serves per-frame calls (the stereo bench runs eight of them) should take ONE slot of that rotation -- with four streams per context
// every context's main stream landed on the same queue (configs[3]: 233 instead of 346-386 frame pairs/s).
int ensure_side_streams(ssm_ctx* c)
{
    if (c->side_ready) return SSM_OK;
    // ensure() creates only what is still missing: a call that failed half-way leaves side_ready false and the next call resumes
    // (Round 5 measured a static split of the machine -- the map stage's stream confined to N compute units, the chains' streams to the rest, hipExtStreamCreateWithCUMask --
    // against the hardware's block-by-block arbitration: -9 %, profiles/r05_cu_split.md.  The switches are gone.)
    HIPCHK(c, c->side[0].stream.ensure());
    HIPCHK(c, c->side[1].stream.ensure()); HIPCHK(c, c->side[1].joined.ensure());
    HIPCHK(c, c->forked.ensure()); HIPCHK(c, c->side[0].joined.ensure());
    for (OrbChain& ch : c->chain) HIPCHK(c, ch.orb_done.ensure());
    HIPCHK(c, c->side[2].stream.ensure()); HIPCHK(c, c->side[2].joined.ensure());
    c->side_ready = true;
    return SSM_OK;
}
int lanes_fork(ssm_ctx* c, const LaneList& lanes)
{
    if (!lanes.n) return SSM_OK;
    HIPCHK(c, hipEventRecord(c->forked, c->main.stream));
    for (int i = 0; i < lanes.n; i++) HIPCHK(c, hipStreamWaitEvent(lane(c, lanes.lane[i]).stream, c->forked, 0));
    return SSM_OK;
}
int lanes_join(ssm_ctx* c, const LaneList& lanes)
{
    for (int i = 0; i < lanes.n; i++) { Lane& l = lane(c, lanes.lane[i]); HIPCHK(c, hipEventRecord(l.joined, l.stream)); HIPCHK(c, hipStreamWaitEvent(c->main.stream, l.joined, 0)); }
    return SSM_OK;
}
static int ensure_alt(ssm_ctx* c)          // the workspaces of chains 1, 2 of ssm_seq_process
{
    for (int k = 1; k < 3; k++) if (!c->chain[k].work.kpaux) { const int r = orb_work_alloc(c, c->chain[k].work); if (r) return r; }
    return SSM_OK;
}
// ---------------------------------------------------------------- the ORB front end for nb frames already on the device, on stream s with workspace w
// level 0 + every level of nb frames into w.pyr: one launch where the geometry has the fused form (plan), gray_kernel + one launch per level otherwise
static int make_pyramid(ssm_ctx* c, hipStream_t s, OrbWork& w, const uint8_t* d_img, int channels, int nb, const PyrBandPlan& plan)
{
    const OrbGeom& g = c->g;
    if (plan.bands) {
        prof_begin(c, s, "pyramid"); HIPCHK(c, k_pyramid_bands(d_img, channels, nb, g, w.pyr, plan, c->pyr_tabs.yofs, c->pyr_tabs.ya, c->pyr_tabs.xgrp, c->pyr_tabs.xgrp8, s)); prof_end(c, s);
        return SSM_OK;
    }
    prof_begin(c, s, "gray");      HIPCHK(c, k_gray(d_img, channels, nb, g, w.pyr, s)); prof_end(c, s);
    prof_begin(c, s, "pyramid");   HIPCHK(c, k_pyramid(nb, g, w.pyr, c->pyr_tabs.xofs, c->pyr_tabs.xa, c->pyr_tabs.yofs, c->pyr_tabs.ya, c->pyr_tabs.xgrp, s)); prof_end(c, s);
    return SSM_OK;
}
// the blurred pyramid of nb frames from w.pyr, by the variant the context was created with (orb_detect, and the two ssm_debug_orb_* hooks)
static int orb_pyr_blur(ssm_ctx* c, hipStream_t s, OrbWork& w, int nb)
{
    const OrbGeom& g = c->g;
    prof_begin(c, s, "blur");      HIPCHK(c, c->blur_mfma ? k_blur_mfma(nb, g, w.pyr, w.blur, c->d_blur_tab, s) : k_blur(nb, g, w.pyr, w.blur, s)); prof_end(c, s);
    return SSM_OK;
}
// run_orb in two halves, because the per-frame call (orb_extract_enqueue) has host work to do between them: everything in front of the one kernel that reads the depth image ...
static int orb_detect(ssm_ctx* c, hipStream_t s, OrbWork& w, const uint8_t* d_img, int channels, int nb)
{
    const OrbGeom& g = c->g;
    { const int r = make_pyramid(c, s, w, d_img, channels, nb, nb > 1 ? c->pyr_bands : c->pyr_bands1); if (r) return r; }
    prof_begin(c, s, "fast");      HIPCHK(c, k_fast(nb, g, w.pyr, w.cand, w.ncand, w.cellmax, s)); prof_end(c, s);
    prof_begin(c, s, "octree");    HIPCHK(c, k_octree(nb, g, w.cand, w.ncand, w.cellmax, w.nodeof, w.sel, w.nsel, c->d_status, s)); prof_end(c, s);
    return orb_pyr_blur(c, s, w, nb);
}
// ... and that kernel
static int orb_describe(ssm_ctx* c, hipStream_t s, OrbWork& w, const uint16_t* d_depth, int nb, ssm_keypoint* kps, uint8_t* desc, float* pos3d, int32_t* nkp,
                        const void* planted_aux = nullptr /* ssm_debug_orb_describe alone */)
{
    prof_begin(c, s, "describe");  HIPCHK(c, k_describe(nb, c->g, w.pyr, w.blur, w.sel, w.nsel, c->d_pattern_f, d_depth, c->cfg.camera, w.kpaux, kps, desc, pos3d, nkp, s, planted_aux)); prof_end(c, s);
    return SSM_OK;
}
static int run_orb(ssm_ctx* c, hipStream_t s, OrbWork& w, const uint8_t* d_img, int channels, const uint16_t* d_depth, int nb,
                   ssm_keypoint* kps, uint8_t* desc, float* pos3d, int32_t* nkp)
{
    const int r = orb_detect(c, s, w, d_img, channels, nb);
    return r ? r : orb_describe(c, s, w, d_depth, nb, kps, desc, pos3d, nkp);
}

extern "C" void ssm_debug_live_allocations(int* buffers, size_t* device_bytes, size_t* pinned_bytes)
{
    if (buffers) *buffers = DevBufLive::buffers.load();
    if (device_bytes) *device_bytes = DevBufLive::device_bytes.load();
    if (pinned_bytes) *pinned_bytes = DevBufLive::pinned_bytes.load();
}

extern "C" void ssm_debug_live_handles(int* streams, int* events)
{
    if (streams) *streams = HandleLive::streams.load();
    if (events) *events = HandleLive::events.load();
}

extern "C" int ssm_debug_pyramid(ssm_ctx* c, const uint8_t* img, int channels, int n, int bands, uint8_t* out, int* bytes)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    const OrbGeom& g = c->g;
    if (bytes) *bytes = g.pyr_bytes;
    if (!img && !out) return SSM_OK;                                     // the size query
    if (!img || !out || (channels != 1 && channels != 3) || n < 1 || n > c->B) FAIL(c, SSM_E_INVAL, "bad arguments");
    { const int r = wait_pending(c); if (r) return r; }
    const size_t ib = (size_t)g.W * g.H * channels;
    { const int r = ensure_scratch(c, ib * n); if (r) return r; }
    HIPCHK(c, hipMemcpyAsync(c->d_scratch, img, ib * n, hipMemcpyHostToDevice, c->main.stream));
    HIPCHK(c, hipMemsetAsync(c->chain[0].work.pyr, 0xA5, (size_t)n * g.pyr_bytes, c->main.stream));      // every byte the pyramid owns must be written
    PyrBandPlan p; DevBuf<int32_t> own_tab;                             // a plan of this call alone and its band table
    if (bands < 0) p.bands = 0;
    else if (bands == 0) p = n > 1 ? c->pyr_bands : c->pyr_bands1;
    else {
        std::vector<int32_t> tab;
        if (!orb_plan_bands(c->plan, bands, tab, p)) FAIL(c, SSM_E_INVAL, "no fused pyramid at this band count");
        UPLOAD(c, own_tab, tab); p.d_tab = own_tab;
    }
    int r = make_pyramid(c, c->main.stream, c->chain[0].work, c->d_scratch, channels, n, p);
    if (bands > 0) { hipStreamSynchronize(c->main.stream); own_tab.reset(); }
    if (r) return r;
    HIPCHK(c, hipMemcpyAsync(out, c->chain[0].work.pyr, (size_t)n * g.pyr_bytes, hipMemcpyDeviceToHost, c->main.stream));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    return SSM_OK;
}

// The two hooks for exact tests of the blur and describe kernels (include/ssm_hip.h).  Both upload n host frames into d_scratch (at offset 0) and build the
// pyramid and the blurred pyramid in the context's first workspace, by the calls orb_detect makes.
static int debug_orb_pyr_blur(ssm_ctx* c, const uint8_t* img, int channels, int n, size_t scratch_bytes)
{
    const OrbGeom& g = c->g; OrbWork& w = c->chain[0].work; hipStream_t s = c->main.stream;
    const size_t ib = (size_t)g.W * g.H * channels * n;
    { const int r = ensure_scratch(c, scratch_bytes > ib ? scratch_bytes : ib); if (r) return r; }
    HIPCHK(c, hipMemcpyAsync(c->d_scratch, img, ib, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemsetAsync(w.blur, 0xA5, (size_t)n * g.blur_bytes, s));                   // every byte that is read back must have been written
    { const int r = make_pyramid(c, s, w, c->d_scratch, channels, n, n > 1 ? c->pyr_bands : c->pyr_bands1); if (r) return r; }
    return orb_pyr_blur(c, s, w, n);
}
extern "C" int ssm_debug_orb_blur(ssm_ctx* c, const uint8_t* img, int channels, int n, uint8_t* out, int* bytes)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    const OrbGeom& g = c->g;
    if (bytes) *bytes = g.pyr_bytes;
    if (!img && !out) return SSM_OK;                                     // the size query
    if (!img || !out || (channels != 1 && channels != 3) || n < 1 || n > c->B) FAIL(c, SSM_E_INVAL, "bad arguments");
    { const int r = wait_pending(c); if (r) return r; }
    { const int r = debug_orb_pyr_blur(c, img, channels, n, 0); if (r) return r; }
    std::vector<uint8_t> tiled((size_t)n * g.blur_bytes);
    HIPCHK(c, hipMemcpyAsync(tiled.data(), c->chain[0].work.blur, tiled.size(), hipMemcpyDeviceToHost, c->main.stream));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    // the tiled layout (blur_off) back into rows of `stride` bytes at img_off, byte by byte on purpose: the layout is part of what the tests check
    for (int f = 0; f < n; f++)
        for (int l = 0; l < g.nlevels; l++) {
            const LevelGeom& L = g.L[l];
            const uint8_t* src = tiled.data() + (size_t)f * g.blur_bytes;
            uint8_t* dst = out + (size_t)f * g.pyr_bytes + L.img_off;
            for (int y = 0; y < L.h; y++)
                for (int x = 0; x < L.stride; x++) dst[(size_t)y * L.stride + x] = src[blur_off(L.boff, L.stride, x, y)];
        }
    return SSM_OK;
}
extern "C" int ssm_debug_orb_describe(ssm_ctx* c, const uint8_t* img, int channels, int n, const uint16_t* depth, const int32_t* nsel, const uint32_t* sel,
                                      const int32_t* moments, int32_t* nkp, ssm_keypoint* kps, uint8_t* desc, float* pos3d, int32_t* moments_out, float* sincos_out)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    const OrbGeom& g = c->g;
    if (!img || !nsel || !nkp || !kps || !desc || !pos3d || !moments_out || !sincos_out || (channels != 1 && channels != 3)) FAIL(c, SSM_E_INVAL, "bad arguments");
    if (n < 1 || n > c->B) FAIL(c, SSM_E_INVAL, "n must be 1..max_batch");
    // the planted selection into the workspace's slot layout; everything is checked here, before the first launch: the kernels rely on it
    struct Aux { int32_t m10, m01; float sn, cs; };                      // KpAux (kernels_orb.hip)
    std::vector<uint32_t> h_sel((size_t)n * g.sel_total, 0u);
    std::vector<Aux> h_aux(moments ? (size_t)n * g.sel_total : 0, Aux{0, 0, 0.f, 0.f});
    size_t total = 0;
    for (int f = 0; f < n; f++)
        for (int l = 0; l < g.nlevels; l++) {
            const LevelGeom& L = g.L[l]; const int k = nsel[f * g.nlevels + l];
            if (k < 0 || k > L.sel_cap) FAIL(c, SSM_E_INVAL, "nsel of frame " + std::to_string(f) + " level " + std::to_string(l) + " outside 0.." + std::to_string(L.sel_cap));
            if (k && !sel) FAIL(c, SSM_E_INVAL, "bad arguments");
            for (int i = 0; i < k; i++, total++) {
                const uint32_t pk = sel[total]; const int x = pk & 4095, y = (pk >> 12) & 4095;
                if (x < SSM_EDGE || x >= L.w - SSM_EDGE || y < SSM_EDGE || y >= L.h - SSM_EDGE)
                    FAIL(c, SSM_E_INVAL, "planted keypoint (" + std::to_string(x) + ", " + std::to_string(y) + ") of frame " + std::to_string(f) + " level " + std::to_string(l) +
                                         " outside [19, w - 19) x [19, h - 19)");
                const size_t slot = (size_t)f * g.sel_total + L.sel_off + i;
                h_sel[slot] = pk;
                if (moments) { h_aux[slot].m10 = moments[2 * total]; h_aux[slot].m01 = moments[2 * total + 1]; }
            }
        }
    { const int r = wait_pending(c); if (r) return r; }
    // d_scratch: [frames][depth][planted aux][nkp][keypoints][descriptors][positions]
    Carve cv;
    const size_t o_img = cv.take<uint8_t>((size_t)g.W * g.H * channels * n), o_dep = cv.take<uint16_t>(depth ? (size_t)g.W * g.H * n : 0), o_aux = cv.take<Aux>(h_aux.size());
    const size_t o_out = cv.take<int32_t>(n), o_kps = cv.take<ssm_keypoint>((size_t)n * g.cap), o_desc = cv.take<uint8_t>((size_t)n * g.cap * 32), o_pos = cv.take<float>((size_t)n * g.cap * 3);
    const size_t bytes = cv.end();
    (void)o_img;                                                         // (offset 0: debug_orb_pyr_blur puts the frames there)
    { const int r = debug_orb_pyr_blur(c, img, channels, n, bytes); if (r) return r; }
    OrbWork& w = c->chain[0].work; hipStream_t s = c->main.stream; uint8_t* d = c->d_scratch;
    if (depth) HIPCHK(c, hipMemcpyAsync(d + o_dep, depth, (size_t)g.W * g.H * n * 2, hipMemcpyHostToDevice, s));
    if (moments) HIPCHK(c, hipMemcpyAsync(d + o_aux, h_aux.data(), h_aux.size() * sizeof(Aux), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(w.sel, h_sel.data(), h_sel.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(w.nsel, nsel, (size_t)n * g.nlevels * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemsetAsync(d + o_out, 0xA5, bytes - o_out, s));        // what the kernels do not write comes back as this byte
    HIPCHK(c, hipMemsetAsync(w.kpaux, 0xA5, (size_t)n * g.sel_total * 32, s));
    { const int r = orb_describe(c, s, w, depth ? reinterpret_cast<const uint16_t*>(d + o_dep) : nullptr, n, reinterpret_cast<ssm_keypoint*>(d + o_kps), d + o_desc,
                                 reinterpret_cast<float*>(d + o_pos), reinterpret_cast<int32_t*>(d + o_out), moments ? d + o_aux : nullptr); if (r) return r; }
    std::vector<Aux> aux((size_t)n * g.sel_total);
    HIPCHK(c, hipMemcpyAsync(nkp, d + o_out, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(kps, d + o_kps, (size_t)n * g.cap * sizeof(ssm_keypoint), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(desc, d + o_desc, (size_t)n * g.cap * 32, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(pos3d, d + o_pos, (size_t)n * g.cap * 12, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(aux.data(), w.kpaux, aux.size() * sizeof(Aux), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    // KpAux is kept per slot: into output order (level by level, the order of `sel`)
    memset(moments_out, 0xA5, (size_t)n * g.cap * 8); memset(sincos_out, 0xA5, (size_t)n * g.cap * 8);
    for (int f = 0; f < n; f++) {
        size_t o = (size_t)f * g.cap;
        for (int l = 0; l < g.nlevels; l++)
            for (int i = 0; i < nsel[f * g.nlevels + l]; i++, o++) {
                const Aux& a = aux[(size_t)f * g.sel_total + g.L[l].sel_off + i];
                moments_out[2 * o] = a.m10; moments_out[2 * o + 1] = a.m01; sincos_out[2 * o] = a.sn; sincos_out[2 * o + 1] = a.cs;
            }
    }
    return SSM_OK;
}
// The hook for exact tests of the quad-tree selection: k_octree alone, as orb_detect launches it, on PLANTED candidate lists and cell maxima in the context's
// first workspace (include/ssm_hip.h).  Everything the kernel relies on is checked here, on the host, before the first launch.
extern "C" int ssm_debug_orb_octree(ssm_ctx* c, int n, const int32_t* ncand, const uint32_t* cand, const int32_t* cellmax, int32_t* geom, int32_t* nsel, uint32_t* sel, int32_t* status,
                                    uint16_t* nodeof)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    const OrbGeom& g = c->g;
    if (geom) {
        for (int l = 0; l < g.nlevels; l++) {
            const LevelGeom& L = g.L[l];
            const int32_t v[SSM_OCTREE_GEOM_LEVEL_INTS] = {L.w, L.h, L.minBX, L.nCols, L.nRows, L.wCell, L.hCell, L.nfeat, L.nIni, L.cand_cap, L.sel_cap};
            memcpy(geom + l * SSM_OCTREE_GEOM_LEVEL_INTS, v, sizeof(v));
        }
        int32_t* t = geom + g.nlevels * SSM_OCTREE_GEOM_LEVEL_INTS;
        t[0] = g.cells_total; t[1] = g.cand_total; t[2] = g.sel_total; t[3] = k_octree_nodes(g);
    }
    if (!ncand && !cand && !cellmax) { if (!geom) FAIL(c, SSM_E_INVAL, "bad arguments"); return SSM_OK; }      // the geometry query
    if (!ncand || !cellmax || !nsel || !sel || !status) FAIL(c, SSM_E_INVAL, "bad arguments");
    if (n < 1 || n > c->B) FAIL(c, SSM_E_INVAL, "n must be 1..max_batch");
    std::vector<cand_t> h_cand((size_t)n * g.cand_total, make_uint2(0u, 0u));
    size_t total = 0;
    for (int f = 0; f < n; f++)
        for (int l = 0; l < g.nlevels; l++) {
            const LevelGeom& L = g.L[l]; const int k = ncand[f * g.nlevels + l];
            const std::string at = " of frame " + std::to_string(f) + " level " + std::to_string(l);
            if (k < 0 || k > L.cand_cap) FAIL(c, SSM_E_INVAL, "ncand" + at + " outside 0.." + std::to_string(L.cand_cap));
            if (k && !cand) FAIL(c, SSM_E_INVAL, "bad arguments");
            const int W = L.maxBX - L.minBX, H = L.maxBY - L.minBY;
            for (int i = 0; i < k; i++, total++) {
                const uint32_t lo = cand[2 * total], hi = cand[2 * total + 1];
                const int x = lo & 4095, y = (lo >> 12) & 4095, cell = (int)(hi >> 14), yin = (hi >> 7) & 127, xin = hi & 127;
                if (x < 3 || x >= W - 3 || y < 3 || y >= H - 3)
                    FAIL(c, SSM_E_INVAL, "planted candidate (" + std::to_string(x) + ", " + std::to_string(y) + ")" + at + " outside the detection window [3, W - 3) x [3, H - 3)");
                if (cell >= L.nCols * L.nRows) FAIL(c, SSM_E_INVAL, "cell " + std::to_string(cell) + at + " outside the level's " + std::to_string(L.nCols * L.nRows) + " cells");
                const int cj = (x - 3) / L.wCell, ci = (y - 3) / L.hCell;                       // fast_tile's cellx / celly
                if (cell != ci * L.nCols + cj || xin != x - cj * L.wCell || yin != y - ci * L.hCell)
                    FAIL(c, SSM_E_INVAL, "rank word of candidate (" + std::to_string(x) + ", " + std::to_string(y) + ")" + at + " does not match its position");
                h_cand[(size_t)f * g.cand_total + L.cand_off + i] = make_uint2(lo, hi);
            }
        }
    for (size_t i = 0; i < (size_t)n * g.cells_total; i++)
        if (cellmax[i] < 0 || cellmax[i] > 255) FAIL(c, SSM_E_INVAL, "cellmax entry " + std::to_string(i) + " outside 0..255");
    { const int r = wait_pending(c); if (r) return r; }
    OrbWork& w = c->chain[0].work; hipStream_t s = c->main.stream;
    HIPCHK(c, hipMemcpyAsync(w.cand, h_cand.data(), h_cand.size() * sizeof(cand_t), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(w.ncand, ncand, (size_t)n * g.nlevels * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(w.cellmax, cellmax, (size_t)n * g.cells_total * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemsetAsync(w.sel, 0xA5, (size_t)n * g.sel_total * 4, s));                  // what the kernel does not write comes back as this byte
    HIPCHK(c, hipMemsetAsync(w.nsel, 0xA5, (size_t)n * g.nlevels * 4, s));
    HIPCHK(c, hipMemsetAsync(w.nodeof, 0xA5, (size_t)n * g.cand_total * 2, s));
    HIPCHK(c, hipMemsetAsync(c->d_status, 0, 4, s));
    HIPCHK(c, k_octree(n, g, w.cand, w.ncand, w.cellmax, w.nodeof, w.sel, w.nsel, c->d_status, s));
    HIPCHK(c, hipMemcpyAsync(nsel, w.nsel, (size_t)n * g.nlevels * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(sel, w.sel, (size_t)n * g.sel_total * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(status, c->d_status, 4, hipMemcpyDeviceToHost, s));
    if (nodeof) HIPCHK(c, hipMemcpyAsync(nodeof, w.nodeof, (size_t)n * g.cand_total * 2, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemsetAsync(c->d_status, 0, 4, s));                                         // nothing planted leaks into the next call
    HIPCHK(c, hipStreamSynchronize(s));
    return SSM_OK;
}

// ---- the per-frame calls of the reference's unchanged loop (Tracker::trackRefFrame: detectFeatures, then match against every reference frame,
// src/track.cpp:140-163 there).  Each call takes ONE block of the pinned ring (inputs staged, results landed) and ONE block of the device ring.  A small struct
// (OrbBlock, MatchBlock) lays the blocks out once per call; the enqueue and the finisher both read its offsets.  Inputs go into the pinned block (one memcpy per
// image / descriptor set), then ONE host-to-device copy per image / per matcher call, the kernels, ONE device-to-host copy of a result block that carries the
// counts with the payload (capacity-sized: no round trip to learn a count first), and a finisher that ssm_wait runs after the stream has drained.  The
// synchronous forms are the asynchronous ones + ssm_wait.
int wait_pending(ssm_ctx* c)
{
    if (c->pending.empty()) {
        // (an enqueue that failed behind its ring_take has advanced the offsets without registering a finisher: drain what may still read the ring, then rewind)
        if (c->h_ring_off || c->d_ring_off) { HIPCHK(c, hipStreamSynchronize(c->main.stream)); c->h_ring_off = 0; c->d_ring_off = 0; }
        return SSM_OK;
    }
    int rc = SSM_OK;
    const hipError_t e = hipStreamSynchronize(c->main.stream);
    if (e != hipSuccess) { c->err = std::string("hipStreamSynchronize: ") + hipGetErrorString(e); rc = SSM_E_HIP; }
    std::vector<std::function<int(ssm_ctx*)>> fins; fins.swap(c->pending);
    for (auto& f : fins) { if (rc == SSM_OK) { const int r = f(c); if (r != SSM_OK) rc = r; } }      // after a failure the later calls' outputs stay untouched
    c->h_ring_off = 0; c->d_ring_off = 0;
    return rc;
}
static int ring_take(ssm_ctx* c, size_t hbytes, size_t dbytes, uint8_t** hp, uint8_t** dp)
{
    hbytes = up256(hbytes); dbytes = up256(dbytes);
    if (c->h_ring_off + hbytes > c->d_ring.bytes() || c->d_ring_off + dbytes > c->d_ring.bytes()) {
        int r = wait_pending(c); if (r) return r;                                // out of room: finish what is in flight (its results are delivered now)
        const size_t need = hbytes > dbytes ? hbytes : dbytes;
        if (need > c->d_ring.bytes()) {
            HIPCHK(c, hipStreamSynchronize(c->main.stream));
            c->h_ring.reset(); c->d_ring.reset();
            const size_t nb = need * 4 > ((size_t)8 << 20) ? need * 4 : ((size_t)8 << 20);
            if (c->h_ring.alloc(c, nb)) FAIL(c, SSM_E_HIP, "hipHostMalloc of the staging ring failed");
            if (c->d_ring.alloc(c, nb)) { c->h_ring.reset(); FAIL(c, SSM_E_HIP, "hipMalloc of the result ring failed"); }
        }
        if (c->h_ring_off + hbytes > c->d_ring.bytes() || c->d_ring_off + dbytes > c->d_ring.bytes()) FAIL(c, SSM_E_HIP, "staging ring: the request does not fit after the wait");
    }
    *hp = c->h_ring + c->h_ring_off; *dp = c->d_ring + c->d_ring_off;
    c->h_ring_off += hbytes; c->d_ring_off += dbytes;
    return SSM_OK;
}
// result block of one ORB extraction with room for ocap keypoints: [n, status, pad to 64 bytes][keypoints][descriptors][positions]
struct OrbBlock {
    size_t kps, desc, pos, bytes;                                       // offsets (n, status at 0) and the size of the block
    explicit OrbBlock(int ocap) : kps(64), desc(kps + (size_t)ocap * sizeof(ssm_keypoint)), pos(desc + (size_t)ocap * 32), bytes(pos + (size_t)ocap * 12) {}
};
// the matrix-core matcher's rows (kernels_match.hip): capT = descriptors per row rounded up to the 32-row tile; expanded rows (each of eq, et); key rows, one per pair
static int match_capT(int cap) { return (cap + 31) & ~31; }
static bool match_mfma_fits(int cap) { return match_key_fits(match_capT(cap)); }      // rows short enough for an exact accumulator key (match_keys.h); longer ones take the VALU matcher
static size_t match_exp_bytes(size_t rows, int capT) { return rows * capT * SSM_MATCH_DESC_BYTES; }
static size_t match_knn_bytes(size_t pairs, int capT) { return pairs * capT * 8; }
// One matrix-core matcher call on rows <= 17 descriptor sets of up to capm descriptors: the query sets first, the train set last, nref = rows - 1 pairs.
//   pinned block: [rows x capm descriptors][counts] .. [what comes back: the result block, or key rows]
//   device block: [the same inputs + counts][eq][et][knn: nref key rows][result block: counts header + nref lists of capm matches], regions 256-aligned
struct MatchBlock {
    static constexpr size_t counts_bytes = 128, res_hdr = 256;         // 32 row counts; nref list lengths
    int rows, nref, capm, capT;
    size_t rowb, inb, expb, knnb, resb;                                 // sizes: one input row, inputs + counts, each of eq / et, knn, result block
    size_t counts, h_res, hbytes;                                       // pinned block (inputs at 0; counts: the same offset in both blocks)
    size_t d_eq, d_et, d_knn, d_res, dbytes;                            // device block (inputs at 0)
    MatchBlock(int rows_, int capm_) : rows(rows_), nref(rows_ - 1), capm(capm_), capT(match_capT(capm_))
    {
        rowb = (size_t)capm * 32; counts = rows * rowb; inb = counts + counts_bytes;
        expb = match_exp_bytes(rows, capT); knnb = up256(match_knn_bytes(nref, capT)); resb = list(nref);
        h_res = (inb + 63) & ~(size_t)63; hbytes = h_res + (resb > knnb ? resb : knnb);
        d_eq = up256(inb); d_et = d_eq + expb; d_knn = d_et + expb; d_res = d_knn + knnb; dbytes = d_res + resb;
    }
    size_t list(int i) const { return res_hdr + (size_t)i * capm * sizeof(ssm_dmatch); }      // list i inside the result block
};
// in_place: the caller's buffers outlive the device work (the synchronous form) -- page-locked inputs are then used where they are
static int orb_extract_enqueue(ssm_ctx* c, const uint8_t* img, int w, int h, int stride, int channels, const uint16_t* depth,
                               ssm_keypoint* kps, uint8_t* desc, float* pos3d, int cap, int* n_out, bool in_place = false)
{
    if (!img || !kps || !desc || !n_out) FAIL(c, SSM_E_INVAL, "null argument");
    if (w != c->g.W || h != c->g.H) FAIL(c, SSM_E_INVAL, "frame size differs from the context configuration");
    if (channels != 1 && channels != 3) FAIL(c, SSM_E_INVAL, "channels must be 1 or 3");
    if (stride < w * channels) FAIL(c, SSM_E_INVAL, "stride smaller than a row");
    const int ocap = c->g.cap;
    const size_t row = (size_t)w * channels, ib = row * h, db = depth ? (size_t)w * h * 2 : 0;
    const OrbBlock B(ocap);
    uint8_t *hp, *dp;
    int r = ring_take(c, ib + db + 64 + B.bytes, B.bytes, &hp, &dp); if (r) return r;
    uint8_t* h_in = hp; uint8_t* h_out = hp + ((ib + db + 63) & ~(size_t)63);
    // round 6: the call is a latency chain (20 launches of 4 - 40 us for one frame + the staging copies).  The depth image is read by the LAST kernel only, and only at
    // the <= cap keypoints: it is staged into the pinned ring while gray .. quad-tree run (after their launches, before the describe launches) and the kernel reads it
    // there, through the ring's device mapping -- no 0.6 MB upload, no staging time in front of the first kernel.  (Measured and dropped: the blur on a side stream
    // beside FAST + the quad-tree -- two cross-stream events cost more than the 17 us they hide: 177 -> 223 us from first to last kernel.)
    const bool img_direct = in_place && (size_t)stride == row && host_is_pinned(img), depth_direct = in_place && depth && host_is_pinned(depth);
    if (img_direct) HIPCHK(c, hipMemcpyAsync(c->d_in_img, img, ib, hipMemcpyHostToDevice, c->main.stream));       // page-locked input (ssm_host_alloc): no staging pass
    else {
        if ((size_t)stride == row) memcpy(h_in, img, ib);
        else for (int y = 0; y < h; y++) memcpy(h_in + (size_t)y * row, img + (size_t)y * stride, row);
        HIPCHK(c, hipMemcpyAsync(c->d_in_img, h_in, ib, hipMemcpyHostToDevice, c->main.stream));
    }
    int32_t* dn = reinterpret_cast<int32_t*>(dp);
    ssm_keypoint* dk = reinterpret_cast<ssm_keypoint*>(dp + B.kps);
    uint8_t* dd = dp + B.desc;
    float* dps = reinterpret_cast<float*>(dp + B.pos);
    r = orb_detect(c, c->main.stream, c->chain[0].work, c->d_in_img, channels, 1); if (r) return r;
    const uint16_t* d_depth = nullptr;
    if (depth) {
        if (!depth_direct) memcpy(h_in + ib, depth, db);       // (the device is busy with the launches above meanwhile)
        void* mapped = nullptr;
        HIPCHK(c, hipHostGetDevicePointer(&mapped, depth_direct ? const_cast<uint16_t*>(depth) : reinterpret_cast<uint16_t*>(h_in + ib), 0));
        d_depth = reinterpret_cast<const uint16_t*>(mapped);
    }
    r = orb_describe(c, c->main.stream, c->chain[0].work, d_depth, 1, dk, dd, dps, dn); if (r) return r;
    HIPCHK(c, hipMemcpyAsync(dn + 1, c->d_status, 4, hipMemcpyDeviceToDevice, c->main.stream));          // the ORB scratch-overflow word travels in the block's header
    HIPCHK(c, hipMemcpyAsync(h_out, dp, B.bytes, hipMemcpyDeviceToHost, c->main.stream));
    c->pending.push_back([=](ssm_ctx* cc) -> int {
        int32_t hdr[2]; memcpy(hdr, h_out, 8);
        if (hdr[1]) { hipMemset(cc->d_status, 0, 4); FAIL(cc, SSM_E_CAPACITY, "ORB scratch capacity exceeded (status " + std::to_string(hdr[1]) + ")"); }
        const int n = hdr[0];
        *n_out = n;
        if (n > cap) FAIL(cc, SSM_E_CAPACITY, "keypoint buffer too small (need " + std::to_string(n) + ")");
        memcpy(kps, h_out + B.kps, sizeof(ssm_keypoint) * (size_t)n);
        memcpy(desc, h_out + B.desc, (size_t)n * 32);
        if (pos3d) memcpy(pos3d, h_out + B.pos, (size_t)n * 12);
        return SSM_OK;
    });
    return SSM_OK;
}
extern "C" int ssm_orb_extract_async(ssm_ctx* c, const uint8_t* img, int w, int h, int stride, int channels, const uint16_t* depth,
                                     ssm_keypoint* kps, uint8_t* desc, float* pos3d, int cap, int* n_out)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    return orb_extract_enqueue(c, img, w, h, stride, channels, depth, kps, desc, pos3d, cap, n_out);
}
extern "C" int ssm_orb_extract(ssm_ctx* c, const uint8_t* img, int w, int h, int stride, int channels, const uint16_t* depth,
                               ssm_keypoint* kps, uint8_t* desc, float* pos3d, int cap, int* n_out)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    int r = orb_extract_enqueue(c, img, w, h, stride, channels, depth, kps, desc, pos3d, cap, n_out, true); if (r) return r;
    return wait_pending(c);
}
extern "C" int ssm_wait(ssm_ctx* c)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    return wait_pending(c);
}

// ---------------------------------------------------------------- matcher, host pointers
// The matrix-core matcher of the sequence path on a short "sequence" through the rings: rows 0 .. nref - 1 are the query sets (Tracker::trackRefFrame's reference
// frames, oldest first), row nref is the train set of every pair (the current frame) -- one upload, one expansion, ONE matrix-core launch for all pairs, one
// download.  The finisher delivers list i = OrbFeature::match(qs[i], t) into outs[i] / n_outs[i]; with idx / dist given (nref == 1) it delivers the two nearest of
// every query instead, decoded from the pair's key row.  The arguments have been checked by the caller; capm = the largest row.
static int match_mfma_enqueue(ssm_ctx* c, const uint8_t* const* qs, const int* nqs, int nref, const uint8_t* t, int nt, int capm, double ratio,
                              ssm_dmatch* const* outs, const int* caps, int* n_outs, int32_t* idx = nullptr, int32_t* dist = nullptr)
{
    const MatchBlock L(nref + 1, capm);
    uint8_t *hp, *dp;
    int r = ring_take(c, L.hbytes, L.dbytes, &hp, &dp); if (r) return r;
    int32_t hn[MatchBlock::counts_bytes / 4] = {0};
    for (int i = 0; i < nref; i++) { if (nqs[i]) memcpy(hp + i * L.rowb, qs[i], (size_t)nqs[i] * 32); hn[i] = nqs[i]; }
    memcpy(hp + nref * L.rowb, t, (size_t)nt * 32); hn[nref] = nt;
    memcpy(hp + L.counts, hn, sizeof(hn));
    const int32_t* dnk = reinterpret_cast<const int32_t*>(dp + L.counts);
    uint8_t* h_res = hp + L.h_res;
    HIPCHK(c, hipMemcpyAsync(dp, hp, L.inb, hipMemcpyHostToDevice, c->main.stream));
    HIPCHK(c, k_match_expand(dp, dnk, 0, L.rows, capm, L.capT, dp + L.d_eq, dp + L.d_et, c->main.stream));
    HIPCHK(c, k_match_seq_mfma(dp + L.d_eq, dp + L.d_et, dnk, 0, 1, nref, nref, ratio, capm, L.capT, match_key_exp(L.capT), dp + L.d_knn,
                               reinterpret_cast<ssm_dmatch*>(dp + L.d_res + L.list(0)), reinterpret_cast<int32_t*>(dp + L.d_res), c->main.stream));
    if (idx) {
        const int nq = nqs[0];
        HIPCHK(c, hipMemcpyAsync(h_res, dp + L.d_knn, (size_t)nq * 8, hipMemcpyDeviceToHost, c->main.stream));
        c->pending.push_back([=](ssm_ctx*) -> int {
            const uint2* hk = reinterpret_cast<const uint2*>(h_res);
            for (int i = 0; i < nq; i++) { idx[2*i] = hk[i].x & 0xFFFF; idx[2*i+1] = hk[i].y & 0xFFFF; dist[2*i] = hk[i].x >> 16; dist[2*i+1] = hk[i].y >> 16; }
            return SSM_OK;
        });
        return SSM_OK;
    }
    // (the last list is copied up to its own capacity: with one pair, the query count)
    HIPCHK(c, hipMemcpyAsync(h_res, dp + L.d_res, L.list(nref - 1) + (size_t)nqs[nref - 1] * sizeof(ssm_dmatch), hipMemcpyDeviceToHost, c->main.stream));
    struct { ssm_dmatch* out[16]; int cap[16]; } to;
    for (int i = 0; i < nref; i++) { to.out[i] = outs[i]; to.cap[i] = caps[i]; }
    c->pending.push_back([=](ssm_ctx* cc) -> int {
        for (int i = 0; i < nref; i++) {
            int32_t n; memcpy(&n, h_res + 4 * (size_t)i, 4);
            if (n < 0) n = 0;
            n_outs[i] = n;
            if (n > to.cap[i]) FAIL(cc, SSM_E_CAPACITY, "match buffer too small (need " + std::to_string(n) + ")");
            memcpy(to.out[i], h_res + L.list(i), sizeof(ssm_dmatch) * (size_t)n);
        }
        return SSM_OK;
    });
    return SSM_OK;
}
// the VALU variant (SSM_MATCH_VARIANT=0, and every pair with more than 32768 descriptors on a side): one pair through d_scratch, complete when the call returns
static int match_valu(ssm_ctx* c, const uint8_t* q, int nq, const uint8_t* t, int nt, double ratio, int32_t* idx, int32_t* dist, ssm_dmatch* out, int cap, int* n_out)
{
    const bool want_knn = idx != nullptr;
    const size_t need = (size_t)(nq + nt) * 32 + sizeof(MatchPair) + (size_t)nq * (16 + 16) + 64;
    int r = ensure_scratch(c, need); if (r) return r;
    uint8_t* dd = c->d_scratch;
    ssm_dmatch* dm = reinterpret_cast<ssm_dmatch*>(dd + (size_t)(nq + nt) * 32);
    int32_t* di = reinterpret_cast<int32_t*>(dm + nq); int32_t* ds = di + 2 * (size_t)nq;
    MatchPair* dp = reinterpret_cast<MatchPair*>(ds + 2 * (size_t)nq); int32_t* dn = reinterpret_cast<int32_t*>(dp + 1);
    MatchPair p; p.qoff = 0; p.nq = nq; p.toff = nq; p.nt = nt; p.out_slot = 0;
    HIPCHK(c, hipMemcpyAsync(dd, q, (size_t)nq * 32, hipMemcpyHostToDevice, c->main.stream));
    HIPCHK(c, hipMemcpyAsync(dd + (size_t)nq * 32, t, (size_t)nt * 32, hipMemcpyHostToDevice, c->main.stream));
    HIPCHK(c, hipMemcpyAsync(dp, &p, sizeof(p), hipMemcpyHostToDevice, c->main.stream));
    HIPCHK(c, k_match_pairs(dd, dp, 1, ratio, nq, dm, dn, want_knn ? di : nullptr, want_knn ? ds : nullptr, c->main.stream));
    int n = 0;
    HIPCHK(c, hipMemcpyAsync(&n, dn, 4, hipMemcpyDeviceToHost, c->main.stream));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    if (want_knn) {
        HIPCHK(c, hipMemcpy(idx, di, (size_t)nq * 8, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(dist, ds, (size_t)nq * 8, hipMemcpyDeviceToHost));
    } else {
        *n_out = n;
        if (n > cap) FAIL(c, SSM_E_CAPACITY, "match buffer too small (need " + std::to_string(n) + ")");
        HIPCHK(c, hipMemcpy(out, dm, sizeof(ssm_dmatch) * n, hipMemcpyDeviceToHost));
    }
    return SSM_OK;
}
// one pair: idx / dist (the two nearest of every query) or out / cap / n_out (the ratio-tested list)
static int match_host(ssm_ctx* c, const uint8_t* q, int nq, const uint8_t* t, int nt, double ratio, int32_t* idx, int32_t* dist, ssm_dmatch* out, int cap, int* n_out)
{
    if (nq < 0 || nt < 0 || (nq && !q) || (nt && !t)) FAIL(c, SSM_E_INVAL, "bad descriptor arguments");
    if (nt < 2) FAIL(c, SSM_E_TOO_FEW_TRAIN, "knnMatch(k=2) needs at least 2 train descriptors");
    if (nt > 65535) FAIL(c, SSM_E_INVAL, "at most 65535 train descriptors per call");
    if (nq == 0) { if (n_out) *n_out = 0; return SSM_OK; }
    if (!c->match_mfma || !match_mfma_fits(nq > nt ? nq : nt)) return match_valu(c, q, nq, t, nt, ratio, idx, dist, out, cap, n_out);
    return match_mfma_enqueue(c, &q, &nq, 1, t, nt, nq > nt ? nq : nt, ratio, &out, &cap, n_out, idx, dist);
}
extern "C" int ssm_hamming_knn2(ssm_ctx* c, const uint8_t* q, int nq, const uint8_t* t, int nt, int32_t* idx, int32_t* dist)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (nq > 0 && (!idx || !dist)) FAIL(c, SSM_E_INVAL, "null output");
    int r = match_host(c, q, nq, t, nt, c->cfg.knn_match_ratio, idx, dist, nullptr, 0, nullptr); if (r) return r;
    return wait_pending(c);
}
extern "C" int ssm_match(ssm_ctx* c, const uint8_t* q, int nq, const uint8_t* t, int nt, double ratio, ssm_dmatch* out, int cap, int* n_out)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (!n_out || (cap > 0 && !out)) FAIL(c, SSM_E_INVAL, "null output");
    int r = match_host(c, q, nq, t, nt, ratio, nullptr, nullptr, out, cap, n_out); if (r) return r;
    return wait_pending(c);
}
extern "C" int ssm_match_async(ssm_ctx* c, const uint8_t* q, int nq, const uint8_t* t, int nt, double ratio, ssm_dmatch* out, int cap, int* n_out)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (!n_out || (cap > 0 && !out)) FAIL(c, SSM_E_INVAL, "null output");
    return match_host(c, q, nq, t, nt, ratio, nullptr, nullptr, out, cap, n_out);       // the VALU variant (SSM_MATCH_VARIANT=0) completes inside the call
}
// Tracker::trackRefFrame's loop `for (pFrame : refFrames) matches = orb.match(pFrame, currentFrame)` (src/track.cpp:150-152 of the reference) as ONE call
static int match_refs_enqueue(ssm_ctx* c, const uint8_t* const* refs, const int* nrefs, int nref, const uint8_t* cur, int ncur, double ratio,
                              ssm_dmatch* const* outs, const int* caps, int* n_outs)
{
    if (nref < 0 || (nref && (!refs || !nrefs || !outs || !caps || !n_outs)) || ncur < 0 || (ncur && !cur)) FAIL(c, SSM_E_INVAL, "bad arguments");
    if (nref == 0) return SSM_OK;
    if (ncur < 2) FAIL(c, SSM_E_TOO_FEW_TRAIN, "knnMatch(k=2) needs at least 2 train descriptors");
    if (ncur > 65535) FAIL(c, SSM_E_INVAL, "at most 65535 train descriptors per call");
    int capm = ncur;
    for (int i = 0; i < nref; i++) { if (nrefs[i] < 0 || (nrefs[i] && !refs[i]) || (caps[i] > 0 && !outs[i])) FAIL(c, SSM_E_INVAL, "bad reference set"); if (nrefs[i] > capm) capm = nrefs[i]; }
    if (c->match_mfma && nref <= 16 && match_mfma_fits(capm)) return match_mfma_enqueue(c, refs, nrefs, nref, cur, ncur, capm, ratio, outs, caps, n_outs);
    for (int i = 0; i < nref; i++) {                                           // the VALU variant, more pairs than one block holds, or rows too long for the accumulator key: pair by pair
        if (nrefs[i] == 0) { n_outs[i] = 0; continue; }
        int r = match_host(c, refs[i], nrefs[i], cur, ncur, ratio, nullptr, nullptr, outs[i], caps[i], &n_outs[i]); if (r) return r;
    }
    return SSM_OK;
}
extern "C" int ssm_match_refs_async(ssm_ctx* c, const uint8_t* const* refs, const int* nrefs, int nref, const uint8_t* cur, int ncur, double ratio,
                                    ssm_dmatch* const* outs, const int* caps, int* n_outs)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    return match_refs_enqueue(c, refs, nrefs, nref, cur, ncur, ratio, outs, caps, n_outs);
}
extern "C" int ssm_match_refs(ssm_ctx* c, const uint8_t* const* refs, const int* nrefs, int nref, const uint8_t* cur, int ncur, double ratio,
                              ssm_dmatch* const* outs, const int* caps, int* n_outs)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    int r = match_refs_enqueue(c, refs, nrefs, nref, cur, ncur, ratio, outs, caps, n_outs); if (r) return r;
    return wait_pending(c);
}

// ---------------------------------------------------------------- mapper front half, host pointers
extern "C" int ssm_moving_mask(ssm_ctx* c, const uint8_t* sem, int w, int h, int stride, uint8_t* mask)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (!sem || !mask) FAIL(c, SSM_E_INVAL, "null argument");
    if (w != c->g.W || h != c->g.H) FAIL(c, SSM_E_INVAL, "frame size differs from the context configuration");
    if (stride < w * 3) FAIL(c, SSM_E_INVAL, "stride smaller than a row");
    HIPCHK(c, hipMemcpy2DAsync(c->d_in_sem, (size_t)w * 3, sem, stride, (size_t)w * 3, h, hipMemcpyHostToDevice, c->main.stream));
    HIPCHK(c, k_moving_mask(c->d_in_sem, 1, w, h, c->d_mask, c->main.stream));
    HIPCHK(c, hipMemcpyAsync(mask, c->d_mask, (size_t)w * h, hipMemcpyDeviceToHost, c->main.stream));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    return SSM_OK;
}
// fused: the mask is the semantic-motion fusion's (ssm_motion_fuse.hip) instead of the class mask
static int backproject_host(ssm_ctx* c, const uint16_t* depth, const uint8_t* rgb, const uint8_t* sem, bool fused, const uint8_t* motion, const ssm_motion_fuse_params* params,
                            int w, int h, const ssm_camera* cam, const double* T, double max_distance, ssm_point* out, int cap, int* n_out)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (!depth || !rgb || !sem || !cam || !n_out || (cap > 0 && !out)) FAIL(c, SSM_E_INVAL, "null argument");
    if (w != c->g.W || h != c->g.H) FAIL(c, SSM_E_INVAL, "frame size differs from the context configuration");
    const size_t np = (size_t)w * h;
    HIPCHK(c, hipMemcpyAsync(c->d_in_depth, depth, np * 2, hipMemcpyHostToDevice, c->main.stream));
    HIPCHK(c, hipMemcpyAsync(c->d_in_img, rgb, np * 3, hipMemcpyHostToDevice, c->main.stream));
    HIPCHK(c, hipMemcpyAsync(c->d_in_sem, sem, np * 3, hipMemcpyHostToDevice, c->main.stream));
    if (T) HIPCHK(c, hipMemcpyAsync(c->d_in_pose, T, 128, hipMemcpyHostToDevice, c->main.stream));
    if (fused) { const int r = mf_enqueue(c, c->d_in_sem, nullptr, motion, 1, w, h, params, c->d_mask); if (r) return r; }
    else HIPCHK(c, k_moving_mask(c->d_in_sem, 1, w, h, c->d_mask, c->main.stream));
    HIPCHK(c, k_backproject(c->d_in_depth, c->d_in_img, c->d_in_sem, c->d_mask, T ? c->d_in_pose : nullptr, 1, w, h, *cam, max_distance,
                            c->d_chunk_cnt, c->d_chunk_off, reinterpret_cast<int32_t*>(c->d_total + 1), c->d_total, c->d_points, c->main.stream));
    int64_t total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, c->d_total, 8, hipMemcpyDeviceToHost, c->main.stream));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    *n_out = (int)total;
    if (total > cap) FAIL(c, SSM_E_CAPACITY, "point buffer too small (need " + std::to_string(total) + ")");
    HIPCHK(c, hipMemcpy(out, c->d_points, sizeof(ssm_point) * (size_t)total, hipMemcpyDeviceToHost));
    return SSM_OK;
}
extern "C" int ssm_backproject(ssm_ctx* c, const uint16_t* depth, const uint8_t* rgb, const uint8_t* sem, int w, int h,
                               const ssm_camera* cam, const double* T, double max_distance, ssm_point* out, int cap, int* n_out)
{
    return backproject_host(c, depth, rgb, sem, false, nullptr, nullptr, w, h, cam, T, max_distance, out, cap, n_out);
}
extern "C" int ssm_backproject_fused(ssm_ctx* c, const uint16_t* depth, const uint8_t* rgb, const uint8_t* sem, const uint8_t* motion, int w, int h,
                                     const ssm_camera* cam, const double* T, double max_distance, const ssm_motion_fuse_params* params, ssm_point* out, int cap, int* n_out)
{
    return backproject_host(c, depth, rgb, sem, true, motion, params, w, h, cam, T, max_distance, out, cap, n_out);
}

// ---------------------------------------------------------------- device-resident sequence path
static int ensure_seq(ssm_ctx* c, int n)
{
    if (n <= c->seq_cap) return SSM_OK;
    const OrbGeom& g = c->g; const int R = c->R;
    // keep the history rows across the re-allocation
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    c->seq_cap = 0;                                                 // (a failure below leaves some of the outputs empty: the next call allocates again)
    c->capT = match_capT(g.cap);
    if (c->match_mfma) {       // expanded rows are rebuilt from the bit descriptors at the start of every call (history) and after every ORB sub-batch
        DALLOC(c, c->d_exp_q, match_exp_bytes(n + R, c->capT)); DALLOC(c, c->d_exp_t, match_exp_bytes(n + R, c->capT)); DALLOC(c, c->d_knn, match_knn_bytes((size_t)n * R, c->capT));
    }
    DALLOC(c, c->d_kps, (size_t)n * g.cap); DALLOC(c, c->d_pos3d, (size_t)n * g.cap * 3);
    DALLOC(c, c->d_matches, (size_t)n * R * g.cap); DALLOC(c, c->d_nmatch, (size_t)n * R); DALLOC(c, c->d_match_pend, (size_t)n * R); DALLOC(c, c->d_npoints, (size_t)n);
    DevBuf<uint8_t> nd; DevBuf<int32_t> nn;                         // the context takes them once the history is across
    DALLOC(c, nd, (size_t)(n + R) * g.cap * 32); DALLOC(c, nn, (size_t)(n + R));
    if (!c->d_hist_tmp) DALLOC(c, c->d_hist_tmp, (size_t)R * g.cap * 32 + (size_t)R * 4);
    if (c->d_desc_all && c->prev_n >= 0) {
        HIPCHK(c, hipMemcpy(nd, c->d_desc_all, (size_t)(c->prev_n + R) * g.cap * 32, hipMemcpyDeviceToDevice));
        HIPCHK(c, hipMemcpy(nn, c->d_nkp_all, (size_t)(c->prev_n + R) * 4, hipMemcpyDeviceToDevice));
    }
    c->d_desc_all = std::move(nd); c->d_nkp_all = std::move(nn); c->seq_cap = n;
    return SSM_OK;
}
// ORB -> expand -> (record, waits) -> match of one sub-batch on its chain's lane
static int seq_front(ssm_ctx* c, const ssm_frames_dev* in, int stages, bool mfma, const SeqStep& st)
{
    const OrbGeom& g = c->g; const int R = c->R, f0 = st.f0, nb = st.nb;
    const size_t npix = (size_t)g.W * g.H, row = (size_t)g.cap * 32;
    uint8_t* desc = c->d_desc_all + (size_t)R * row; int32_t* nkp = c->d_nkp_all + R;
    OrbChain& ch = c->chain[st.chain]; const hipStream_t cs = lane(c, st.lane).stream;
    if (stages & SSM_STAGE_ORB) {
        int r = run_orb(c, cs, ch.work, in->bgr + (size_t)f0 * npix * 3, 3, in->depth ? in->depth + (size_t)f0 * npix : nullptr, nb,
                        c->d_kps + (size_t)f0 * g.cap, desc + (size_t)f0 * row, c->d_pos3d + (size_t)f0 * g.cap * 3, nkp + f0);
        if (r) return r;
        if (mfma) { prof_begin(c, cs, "match"); HIPCHK(c, k_match_expand(c->d_desc_all, c->d_nkp_all, R + f0, nb, g.cap, c->capT, c->d_exp_q, c->d_exp_t, cs)); prof_end(c, cs); }
        if (st.record_orb_done) {
            HIPCHK(c, hipEventRecord(ch.orb_done, cs));
            for (int k = 0; k < st.nwait; k++) HIPCHK(c, hipStreamWaitEvent(cs, c->chain[st.wait_chain[k]].orb_done, 0));
        }
    }
    if (stages & SSM_STAGE_MATCH) {
        prof_begin(c, cs, "match");
        if (mfma) {
            if (!(stages & SSM_STAGE_ORB)) HIPCHK(c, k_match_expand(c->d_desc_all, c->d_nkp_all, R + f0, nb, g.cap, c->capT, c->d_exp_q, c->d_exp_t, cs));
            HIPCHK(c, k_match_seq_mfma(c->d_exp_q, c->d_exp_t, c->d_nkp_all, f0, nb, R, R, c->cfg.knn_match_ratio, g.cap, c->capT, match_key_exp(c->capT), c->d_knn, c->d_matches, c->d_nmatch, cs));
        } else
            HIPCHK(c, k_match_seq(c->d_desc_all, c->d_nkp_all, f0, nb, R, R, c->cfg.knn_match_ratio, g.cap, c->d_matches, c->d_nmatch, c->d_match_pend + (size_t)f0 * R, cs));
        prof_end(c, cs);
    }
    return SSM_OK;
}
// (SegNet ->) map of one sub-batch on its map lane
static int seq_back(ssm_ctx* c, const ssm_frames_dev* in, int stages, const SeqStep& st)
{
    if (st.map_lane == LANE_NONE) return SSM_OK;
    const OrbGeom& g = c->g; const int W = g.W, H = g.H, f0 = st.f0, nb = st.nb; const size_t npix = (size_t)W * H;
    Lane& ml = lane(c, st.map_lane); const hipStream_t s = ml.stream; int r;
    const uint8_t* sem_src = in->sem_bgr ? in->sem_bgr + (size_t)f0 * npix * 3 : nullptr;
    if (stages & SSM_STAGE_SEGNET) {          // Classifier in the loop (the variant commented out at src/rgbdframe.cpp:119-136)
        r = seg_init(c); if (r) return r;
        prof_begin(c, s, "segnet");
        r = seg_forward_dev(c, ml, in->bgr + (size_t)f0 * npix * 3, nb, nullptr, c->seg->d_sem_gen, 0); if (r) return r;
        prof_end(c, s);
        sem_src = c->seg->d_sem_gen;
    }
    // The map of a context grows (map_settle): a launch covers all nb frames when the table is large, fewer while it is small, and the table's counters
    // are looked at between launches (map_before_launch).  Exact integer sums: how the frames are cut into launches does not change the map.
    for (int q0 = 0, nq; (stages & SSM_STAGE_MAP) && q0 < nb; q0 += nq) {
        r = map_before_launch(c, s, nb - q0, &nq); if (r) return r;
        const int g0 = f0 + q0;
        const uint8_t* sem_q = sem_src + (size_t)q0 * npix * 3;
        if ((W & 15) == 0) {         // streaming fused kernels (16 pixels per thread, 16-byte loads)
            prof_begin(c, s, "map_fuse");
            { MapLaunch L; L.depth = in->depth + (size_t)g0 * npix; L.rgb = in->bgr + (size_t)g0 * npix * 3; L.sem = sem_q; L.pose = in->pose ? in->pose + (size_t)g0 * 16 : nullptr;
              L.n = nq; L.w = W; L.h = H; L.npoints = c->d_npoints + g0;
              r = map_fuse_launch(c, s, L); if (r) return r; }
            prof_end(c, s);
        } else {                     // odd widths: mask -> ordered back-projection -> insert
            prof_begin(c, s, "mask");
            HIPCHK(c, k_moving_mask(sem_q, nq, W, H, c->d_mask, s)); prof_end(c, s);
            prof_begin(c, s, "backproject");
            HIPCHK(c, k_backproject(in->depth + (size_t)g0 * npix, in->bgr + (size_t)g0 * npix * 3, sem_q, c->d_mask,
                                    in->pose ? in->pose + (size_t)g0 * 16 : nullptr, nq, W, H, c->cfg.camera, c->cfg.mapper_max_distance,
                                    c->d_chunk_cnt, c->d_chunk_off, c->d_npoints + g0, c->d_total, c->d_points, s)); prof_end(c, s);
            prof_begin(c, s, "voxel_insert");
            HIPCHK(c, k_voxel_insert(c->d_points, c->d_total, (int64_t)nq * (int64_t)npix, (float)c->cfg.mapper_resolution, c->map.tab, c->map.cap_log2, c->map.counters, s));
            prof_end(c, s);
        }
        r = map_after_launch(c, s, nq, (stages & SSM_STAGE_SEGNET) != 0 && (W & 15) == 0); if (r) return r;
    }
    return SSM_OK;
}
extern "C" int ssm_seq_process(ssm_ctx* c, const ssm_frames_dev* in, ssm_seq_out_dev* out)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (!in || in->n < 0) FAIL(c, SSM_E_INVAL, "bad arguments");
    const int stages = in->stages ? in->stages : (SSM_STAGE_ORB | SSM_STAGE_MATCH | SSM_STAGE_MAP);
    if ((stages & (SSM_STAGE_ORB | SSM_STAGE_MATCH)) && !in->bgr) FAIL(c, SSM_E_INVAL, "bgr is required");
    if ((stages & SSM_STAGE_MAP) && (!in->depth || !in->bgr || (!in->sem_bgr && !(stages & SSM_STAGE_SEGNET)))) FAIL(c, SSM_E_INVAL, "bgr, depth and sem_bgr (or SSM_STAGE_SEGNET) are required for the map stage");
    const OrbGeom& g = c->g; const int R = c->R, n = in->n; const hipStream_t s = c->main.stream;
    // fused map launches of an earlier call that nobody has looked at since (no ssm_sync / map read in between): their skipped blocks -- if any -- are run again NOW,
    // while the launch descriptors still point at that call's outputs (ensure_seq below may re-allocate the per-frame point counts)
    if (c->gov.unexamined) { const int r0 = map_settle(c, c->mapdev.tail ? c->mapdev.tail : c->main.stream, 0); if (r0) return r0; }
    int r = ensure_seq(c, n > 0 ? n : 1); if (r) return r;
    c->recs.clear(); c->pool_used = 0;
    // history rows
    const size_t row = (size_t)g.cap * 32;
    if (in->continue_sequence && c->prev_n >= 0) {
        int32_t* tn = reinterpret_cast<int32_t*>(c->d_hist_tmp + (size_t)R * row);
        HIPCHK(c, hipMemcpyAsync(c->d_hist_tmp, c->d_desc_all + (size_t)c->prev_n * row, (size_t)R * row, hipMemcpyDeviceToDevice, s));
        HIPCHK(c, hipMemcpyAsync(tn, c->d_nkp_all + c->prev_n, (size_t)R * 4, hipMemcpyDeviceToDevice, s));
        HIPCHK(c, hipMemcpyAsync(c->d_desc_all, c->d_hist_tmp, (size_t)R * row, hipMemcpyDeviceToDevice, s));
        HIPCHK(c, hipMemcpyAsync(c->d_nkp_all, tn, (size_t)R * 4, hipMemcpyDeviceToDevice, s));
    } else {
        HIPCHK(c, hipMemsetAsync(c->d_nkp_all, 0xFF, (size_t)R * 4, s));     // -1: no such reference frame
    }
    const bool mfma = c->match_mfma && (stages & SSM_STAGE_MATCH) && match_key_fits(c->capT);
    if (mfma) HIPCHK(c, k_match_expand(c->d_desc_all, c->d_nkp_all, 0, R, g.cap, c->capT, c->d_exp_q, c->d_exp_t, s));      // the history rows
    // who runs on which lane, in which order, behind which events: ssm_seq_plan.cpp.  The side lanes start behind everything already queued on the main lane
    // and are joined into it at the end.
    const SeqPlan plan = seq_plan({n, c->B, stages, c->serialize, (g.W & 15) == 0, c->mapdev.own_stream});
    if (plan.needs_side_streams) { r = ensure_side_streams(c); if (r) return r; }
    if (plan.needs_alt_work) { r = ensure_alt(c); if (r) return r; }
    r = lanes_fork(c, plan.forked); if (r) return r;
    for (const SeqStep& st : plan.steps) {
        if (st.map_first) { r = seq_back(c, in, stages, st); if (r) return r; r = seq_front(c, in, stages, mfma, st); if (r) return r; }
        else              { r = seq_front(c, in, stages, mfma, st); if (r) return r; r = seq_back(c, in, stages, st); if (r) return r; }
    }
    r = lanes_join(c, plan.forked); if (r) return r;
    if (stages & SSM_STAGE_MAP) c->mapdev.tail = plan.map_tail == LANE_MAIN ? nullptr : (hipStream_t)lane(c, plan.map_tail).stream;      // MapDev::tail
    c->prev_n = n;
    if (out) {
        out->kps = c->d_kps; out->desc = c->d_desc_all + (size_t)R * row; out->pos3d = c->d_pos3d; out->nkp = c->d_nkp_all + R; out->matches = c->d_matches; out->nmatch = c->d_nmatch;
        out->npoints = c->d_npoints; out->cap = g.cap; out->R = R;
    }
    return SSM_OK;
}


// ---------------------------------------------------------------- utilities
extern "C" int ssm_dev_alloc(ssm_ctx* c, size_t bytes, void** out)
{
    if (!c || !out) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    void* p = nullptr; if (bytes == 0) bytes = 1;
    const hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) FAIL(c, SSM_E_NOMEM, std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e));
    *out = p; return SSM_OK;
}
extern "C" int ssm_dev_free(ssm_ctx* c, void* p)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    if (p) HIPCHK(c, hipFree(p));
    return SSM_OK;
}
extern "C" int ssm_memcpy_h2d(ssm_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->main.stream));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    return SSM_OK;
}
extern "C" int ssm_dev_mem_info(ssm_ctx* c, size_t* free_bytes, size_t* total_bytes)
{
    if (!c || !free_bytes || !total_bytes) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    HIPCHK(c, hipMemGetInfo(free_bytes, total_bytes));
    return SSM_OK;
}
extern "C" int ssm_memcpy_h2d_async(ssm_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->main.stream));
    return SSM_OK;
}
extern "C" int ssm_memcpy_d2h_async(ssm_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->main.stream));
    return SSM_OK;
}
extern "C" int ssm_host_alloc(size_t bytes, void** out)
{
    if (!out || bytes == 0) return SSM_E_INVAL;
    void* p = nullptr;
    const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocPortable);
    if (e != hipSuccess) { (void)hipGetLastError(); g_create_err = std::string("hipHostMalloc: ") + hipGetErrorString(e); return SSM_E_NOMEM; }
    *out = p; return SSM_OK;
}
extern "C" int ssm_host_free(void* p) { if (p && hipHostFree(p) != hipSuccess) { (void)hipGetLastError(); return SSM_E_HIP; } return SSM_OK; }
// is [p, p + bytes) page-locked host memory the device can read (hipHostMalloc / hipHostRegister)?  (an unknown pointer makes hipPointerGetAttributes fail: that is "no")
bool host_is_pinned(const void* p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}
extern "C" int ssm_memcpy_d2h(ssm_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->main.stream));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    return SSM_OK;
}
extern "C" int ssm_synth_frames_dev(ssm_ctx* c, uint64_t seed, int first, int n, int w, int h,
                                    uint8_t* bgr, uint16_t* depth, uint8_t* sem, uint8_t* lab, double* pose)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (n <= 0 || !bgr || !depth || !sem) FAIL(c, SSM_E_INVAL, "bad arguments");
    HIPCHK(c, k_synth(seed, first, n, w, h, bgr, depth, sem, lab, pose, c->main.stream));
    return SSM_OK;
}
