// ssm_route.hip -- the device path of the route field behind the C ABI.  DESIGN.md s.23 is the contract.  A field is the launches of kernels_route.hip on the main
// stream: the begin kernel, then rounds -- between two of them the host reads ONE word, form 1's count of active tiles or form 0's "changed" -- then the finish
// kernel and one download, the info.  A path query is two launches and two downloads, the path info and then its cells.  The field, the cells' bytes and a copy of
// dist2 belong to the route target, so the clearance target is only read; the infos, the control words and the staging of hand-made inputs belong to the context.
// The host functions, the defaults and the argument checks are ssm_route_host.cpp; every refusal is made before a launch.
#include "ssm_ctx.h"
#include "ssm_host.h"
using namespace ssm_rtc;

static int route_target_ok(ssm_ctx* c, const ssm_route_target* t)
{
    if (!t) FAIL(c, SSM_E_INVAL, "null argument");
    if (t->owner != c) FAIL(c, SSM_E_INVAL, "route: target of another context");
    return SSM_OK;
}
static RouteBufs route_bufs(ssm_route_target* t) { return RouteBufs{t->in, t->dist2, t->cost, t->parent, t->flag, t->list}; }
// the stage on reach and dist2 images in device memory, from the first launch to the call's last wait
static int route_run(ssm_ctx* c, ssm_route_target* t, const uint8_t* reach, const uint32_t* dist2, int nx, int ny, int32_t source, const Setup& S, ssm_route_info* info)
{
    RouteWork& W = c->route; hipStream_t s = c->main.stream;
    if (!W.info) { DALLOC(c, W.h_info, 9); DALLOC(c, W.info, 9); DALLOC(c, W.h_pinfo, 8); DALLOC(c, W.pinfo, 8); DALLOC(c, W.h_ctl, 4); DALLOC(c, W.ctl, 4); }
    const int64_t tiles = k_route_tiles(nx, ny);
    if (tiles > t->tile_cap) { HIPCHK(c, hipStreamSynchronize(s)); t->tile_cap = 0; DALLOC(c, t->flag, tiles); DALLOC(c, t->list, tiles); t->tile_cap = tiles; }
    const RouteBufs B = route_bufs(t);
    t->fielded = false; W.rounds = 0;
    prof_begin(c, s, "route_begin");
    int n_first = 0;
    HIPCHK(c, k_route_begin(reach, dist2, nx, ny, source, S, B, W.info, W.ctl, &n_first, s));
    prof_end(c, s);
    prof_begin(c, s, "route_relax");
    if (source >= 0) {
        if (W.form == ROUTE_FORM_SWEEPS) {
            // every batch but the last lowers at least one cost, and costs are bounded integers: the loop ends
            for (;;) {
                HIPCHK(c, k_route_sweeps(nx, ny, S, B, W.ctl + 2, s));
                HIPCHK(c, hipMemcpyAsync(W.h_ctl, W.ctl + 2, 4, hipMemcpyDeviceToHost, s));
                HIPCHK(c, hipStreamSynchronize(s));
                W.rounds++;
                if (!W.h_ctl[0]) break;
            }
        } else {
            // a round with active tiles lowers at least one cost or wakes nobody: likewise
            for (int n_active = n_first, round = 0; n_active > 0; round++) {
                HIPCHK(c, k_route_round(nx, ny, S, B, n_active, round, W.ctl, s));
                HIPCHK(c, hipMemcpyAsync(W.h_ctl, W.ctl + (round & 1), 4, hipMemcpyDeviceToHost, s));
                HIPCHK(c, hipStreamSynchronize(s));
                W.rounds++;
                n_active = W.h_ctl[0];
                if (n_active < 0 || n_active > tiles) FAIL(c, SSM_E_HIP, "route: the device counted more active tiles than the grid has");
            }
        }
    }
    prof_end(c, s);
    prof_begin(c, s, "route_finish");
    HIPCHK(c, k_route_finish(nx, ny, source, S, B, W.info, s));
    prof_end(c, s);
    HIPCHK(c, hipMemcpyAsync(W.h_info, W.info, 72, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    t->fielded = true; t->nx = nx; t->ny = ny; t->S = S; t->source = source;
    if (info) {
        static_assert(sizeof(ssm_route_info) == 64, "info is eight 64-bit counts");
        info->routed = (int64_t)W.h_info[0]; info->unrouted = (int64_t)W.h_info[1]; info->near_cells = (int64_t)W.h_info[2];
        info->max_cost = info->routed ? (int64_t)(W.h_info[8] >> 24) : 0; info->far_cell = info->routed ? (int64_t)far_cell_of(W.h_info[8]) : -1;
        info->source_cell = source; info->comfort2 = S.comfort2; info->moves = S.moves;
    }
    return SSM_OK;
}

extern "C" int ssm_route_target_create(ssm_ctx* c, int nx, int ny, int max_path, ssm_route_target** out)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (!out) FAIL(c, SSM_E_INVAL, "null argument");
    *out = nullptr;
    if (nx < 1 || ny < 1 || (int64_t)nx * ny > ssm_gridc::MAX_CELLS) FAIL(c, SSM_E_INVAL, "route: at least 1 x 1 and at most 2^24 cells");
    if (max_path < 1) FAIL(c, SSM_E_INVAL, "route: max_path must be at least 1");
    std::unique_ptr<ssm_route_target> t(new ssm_route_target());
    const size_t nc = (size_t)nx * ny, np = (size_t)std::min<int64_t>(max_path, (int64_t)nc);          // (no path has more cells than the grid)
    t->cap = (int64_t)nc; t->max_path = max_path; t->device = c->device; t->owner = c;
    DALLOC(c, t->in, nc); DALLOC(c, t->dist2, nc); DALLOC(c, t->cost, nc); DALLOC(c, t->parent, nc); DALLOC(c, t->path, np); DALLOC(c, t->rev, np);
    *out = t.release();
    return SSM_OK;
}
extern "C" void ssm_route_target_free(ssm_ctx* c, ssm_route_target* t)
{ free_after_wait(c, t); }

extern "C" int ssm_route_field(ssm_ctx* c, const ssm_clearance_target* ct, const ssm_route_params* params, ssm_route_target* t, ssm_route_info* info)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    { const int r = route_target_ok(c, t); if (r) return r; }
    if (!ct) FAIL(c, SSM_E_INVAL, "null argument");
    if (ct->owner != c) FAIL(c, SSM_E_INVAL, "route: clearance target of another context");
    if (!ct->staged) FAIL(c, SSM_E_INVAL, "route: no call has run on the clearance target");
    ssm_route_params P; ssm_route_params_default(&P); if (params) P = *params;
    Setup S;
    { const int r = route_check(c, P, ct->nx, ct->ny, ct->cell, &S); if (r) return r; }
    if ((int64_t)ct->nx * ct->ny > t->cap) FAIL(c, SSM_E_INVAL, "route: the grid has more cells than the target");
    return route_run(c, t, ct->reach, ct->dist2, ct->nx, ct->ny, (int32_t)ct->seed_cell, S, info);
}
extern "C" int ssm_debug_route_cells(ssm_ctx* c, ssm_route_target* t, const uint8_t* reach, const uint32_t* dist2, int nx, int ny, int source_cell, const ssm_route_params* params,
                                     ssm_route_info* info)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    { const int r = route_target_ok(c, t); if (r) return r; }
    if (!reach || !dist2) FAIL(c, SSM_E_INVAL, "null argument");
    ssm_route_params P; ssm_route_params_default(&P); if (params) P = *params;
    Setup S;
    { const int r = route_check(c, P, nx, ny, P.cell, &S); if (r) return r; }
    { const int r = route_source_check(c, reach, nx, ny, source_cell); if (r) return r; }
    if ((int64_t)nx * ny > t->cap) FAIL(c, SSM_E_INVAL, "route: the grid has more cells than the target");
    RouteWork& W = c->route; hipStream_t s = c->main.stream;
    const size_t nc = (size_t)nx * ny;
    if ((int64_t)nc > W.in_cap) { HIPCHK(c, hipStreamSynchronize(s)); W.in_cap = 0; DALLOC(c, W.in_reach, nc); DALLOC(c, W.in_dist2, nc); W.in_cap = (int64_t)nc; }
    HIPCHK(c, hipMemcpyAsync(W.in_reach, reach, nc, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(W.in_dist2, dist2, nc * 4, hipMemcpyHostToDevice, s));
    return route_run(c, t, W.in_reach, W.in_dist2, nx, ny, source_cell, S, info);
}
extern "C" int ssm_route_path(ssm_ctx* c, ssm_route_target* t, int goal_cx, int goal_cy, int goal_snap, int32_t* cells_out, ssm_route_path_info* path_info)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    { const int r = route_target_ok(c, t); if (r) return r; }
    if (!cells_out || !path_info) FAIL(c, SSM_E_INVAL, "null argument");
    if (!t->fielded) FAIL(c, SSM_E_INVAL, "route: no field has run on the target");
    { const int r = route_goal_check(c, t->nx, t->ny, goal_cx, goal_cy, goal_snap); if (r) return r; }
    RouteWork& W = c->route; hipStream_t s = c->main.stream;
    const int max_path = (int)std::min<int64_t>(t->max_path, t->cap);          // (what the target's path arrays hold: no path has more cells than the grid)
    prof_begin(c, s, "route_path");
    HIPCHK(c, k_route_path(t->nx, t->ny, t->S, route_bufs(t), goal_cx, goal_cy, goal_snap, max_path, t->rev, t->path, W.pinfo, s));
    prof_end(c, s);
    HIPCHK(c, hipMemcpyAsync(W.h_pinfo, W.pinfo, 56, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    static_assert(sizeof(ssm_route_path_info) == 56, "path info is seven 64-bit counts");
    memcpy(path_info, W.h_pinfo, 56);
    if (path_info->len > max_path) FAIL(c, SSM_E_CAPACITY, "route: the path has more cells than the target's max_path");
    if (path_info->len > 0) {
        HIPCHK(c, hipMemcpyAsync(cells_out, t->path, (size_t)path_info->len * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
    }
    return SSM_OK;
}
extern "C" int ssm_route_fetch(ssm_ctx* c, const ssm_route_target* t, uint32_t* cost, int32_t* parent)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    { const int r = route_target_ok(c, t); if (r) return r; }
    if (!t->fielded) FAIL(c, SSM_E_INVAL, "route: no field has run on the target");
    hipStream_t s = c->main.stream;
    const size_t nc = (size_t)t->nx * t->ny;
    if (cost) HIPCHK(c, hipMemcpyAsync(cost, t->cost, nc * 4, hipMemcpyDeviceToHost, s));
    if (parent) HIPCHK(c, hipMemcpyAsync(parent, t->parent, nc * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return SSM_OK;
}
extern "C" int ssm_debug_route_form(ssm_ctx* c, int form)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (form < -1 || form > ROUTE_FORM_TILES) FAIL(c, SSM_E_INVAL, "route: the form is 0 (sweeps of one thread per cell), 1 (active tiles relaxed to their fixed points) or -1 (the default)");
    c->route.form = form < 0 ? (int)ROUTE_FORM_DEFAULT : form;
    return SSM_OK;
}
extern "C" int ssm_debug_route_rounds(ssm_ctx* c)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    return c->route.rounds;
}
extern "C" int ssm_debug_route_tile(void) { return k_route_tile(); }
extern "C" int ssm_debug_route_batch(void) { return k_route_batch(); }
