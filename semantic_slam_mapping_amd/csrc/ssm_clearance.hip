// ssm_clearance.hip -- the device path of the clearance map behind the C ABI.  DESIGN.md s.22 is the contract.  A call is the launches of kernels_clearance.hip on
// the main stream, ONE download (the info) and one wait; the seed and its root are read on the device.  The images and the labelling's array belong to the target,
// the info and the staging of a hand-made class image to the context.  The host function, the defaults and the argument checks are ssm_clearance_host.cpp; every
// refusal is made before a launch.
#include "ssm_ctx.h"
#include "ssm_host.h"
using namespace ssm_clrc;

static int clearance_target_ok(ssm_ctx* c, const ssm_clearance_target* t)
{
    if (!t) FAIL(c, SSM_E_INVAL, "null argument");
    if (t->owner != c) FAIL(c, SSM_E_INVAL, "clearance: target of another context");
    return SSM_OK;
}
// the stage on a class image in device memory, from the first launch to the call's wait
static int clearance_run(ssm_ctx* c, ssm_clearance_target* t, const uint8_t* cls, int nx, int ny, double cell, const Setup& S, ssm_clearance_info* info)
{
    ClearanceWork& W = c->clearance; hipStream_t s = c->main.stream;
    if (!W.info) { DALLOC(c, W.h_info, 8); DALLOC(c, W.info, 9); }
    const ClearanceBufs B{t->mask, t->row, t->dist2, t->nearest, t->labels, t->reach};
    t->staged = false;
    prof_begin(c, s, "clearance");
    HIPCHK(c, k_clearance(cls, nx, ny, S, B, W.info, W.form, s));
    prof_end(c, s);
    static_assert(sizeof(ssm_clearance_info) == 64, "info is eight 64-bit counts");
    HIPCHK(c, hipMemcpyAsync(W.h_info, W.info, 64, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    t->staged = true; t->nx = nx; t->ny = ny; t->seed_cell = (int64_t)W.h_info[5]; t->cell = cell;          // (the seed and the cell size: what a route field starts from)
    if (info) memcpy(info, W.h_info, 64);
    return SSM_OK;
}

extern "C" int ssm_clearance_target_create(ssm_ctx* c, int nx, int ny, ssm_clearance_target** out)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (!out) FAIL(c, SSM_E_INVAL, "null argument");
    *out = nullptr;
    if (nx < 1 || ny < 1 || (int64_t)nx * ny > ssm_gridc::MAX_CELLS) FAIL(c, SSM_E_INVAL, "clearance: at least 1 x 1 and at most 2^24 cells");
    std::unique_ptr<ssm_clearance_target> t(new ssm_clearance_target());
    const size_t nc = (size_t)nx * ny;
    t->cap = (int64_t)nc; t->device = c->device; t->owner = c;
    // (a grid of nc cells has at most nc columns and, per column, no more bands of 32 rows than cells: nc words hold the masks of every shape the target takes)
    DALLOC(c, t->mask, nc); DALLOC(c, t->row, nc); DALLOC(c, t->dist2, nc); DALLOC(c, t->nearest, nc); DALLOC(c, t->labels, nc); DALLOC(c, t->reach, nc);
    *out = t.release();
    return SSM_OK;
}
extern "C" void ssm_clearance_target_free(ssm_ctx* c, ssm_clearance_target* t)
{ free_after_wait(c, t); }

extern "C" int ssm_clearance_grid(ssm_ctx* c, const ssm_grid_target* g, const ssm_clearance_params* params, ssm_clearance_target* t, ssm_clearance_info* info)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    { const int r = clearance_target_ok(c, t); if (r) return r; }
    if (!g) FAIL(c, SSM_E_INVAL, "null argument");
    if (g->owner != c) FAIL(c, SSM_E_INVAL, "clearance: grid target of another context");
    if (!g->built) FAIL(c, SSM_E_INVAL, "clearance: nothing has been built into the grid target");
    ssm_clearance_params P; ssm_clearance_params_default(&P); if (params) P = *params;
    Setup S;
    { const int r = clearance_check(c, P, g->nx, g->ny, g->params.cell, &S); if (r) return r; }
    if ((int64_t)g->nx * g->ny > t->cap) FAIL(c, SSM_E_INVAL, "clearance: the grid has more cells than the target");
    return clearance_run(c, t, g->cls, g->nx, g->ny, g->params.cell, S, info);
}
extern "C" int ssm_debug_clearance_cells(ssm_ctx* c, ssm_clearance_target* t, const uint8_t* cls, int nx, int ny, const ssm_clearance_params* params, ssm_clearance_info* info)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    { const int r = clearance_target_ok(c, t); if (r) return r; }
    if (!cls) FAIL(c, SSM_E_INVAL, "null argument");
    ssm_clearance_params P; ssm_clearance_params_default(&P); if (params) P = *params;
    Setup S;
    { const int r = clearance_check(c, P, nx, ny, P.cell, &S); if (r) return r; }
    if ((int64_t)nx * ny > t->cap) FAIL(c, SSM_E_INVAL, "clearance: the grid has more cells than the target");
    ClearanceWork& W = c->clearance; hipStream_t s = c->main.stream;
    const size_t nc = (size_t)nx * ny;
    if ((int64_t)nc > W.in_cap) { HIPCHK(c, hipStreamSynchronize(s)); W.in_cap = 0; DALLOC(c, W.in_cls, nc); W.in_cap = (int64_t)nc; }
    HIPCHK(c, hipMemcpyAsync(W.in_cls, cls, nc, hipMemcpyHostToDevice, s));
    return clearance_run(c, t, W.in_cls, nx, ny, P.cell, S, info);
}
extern "C" int ssm_clearance_fetch(ssm_ctx* c, const ssm_clearance_target* t, uint32_t* dist2, int32_t* nearest, uint8_t* reach)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    { const int r = clearance_target_ok(c, t); if (r) return r; }
    if (!t->staged) FAIL(c, SSM_E_INVAL, "clearance: no call has run on the target");
    hipStream_t s = c->main.stream;
    const size_t nc = (size_t)t->nx * t->ny;
    if (dist2) HIPCHK(c, hipMemcpyAsync(dist2, t->dist2, nc * 4, hipMemcpyDeviceToHost, s));
    if (nearest) HIPCHK(c, hipMemcpyAsync(nearest, t->nearest, nc * 4, hipMemcpyDeviceToHost, s));
    if (reach) HIPCHK(c, hipMemcpyAsync(reach, t->reach, nc, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return SSM_OK;
}
extern "C" int ssm_debug_clearance_form(ssm_ctx* c, int form)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (form < -1 || form > CLEARANCE_FORM_SCAN) FAIL(c, SSM_E_INVAL, "clearance: the row pass's form is 0 (the whole row through LDS), 1 (an outward scan) or -1 (the default)");
    c->clearance.form = form < 0 ? (int)CLEARANCE_FORM_DEFAULT : form;
    return SSM_OK;
}
extern "C" int ssm_debug_clearance_chunk(void) { return k_clearance_chunk(); }
