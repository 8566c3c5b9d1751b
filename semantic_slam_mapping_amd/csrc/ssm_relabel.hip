// ssm_relabel.hip -- the device path of label fusion behind the C ABI.  DESIGN.md s.20 is the contract.  A call is the launch of kernels_relabel.hip on the main
// stream with the view records as its argument (the relative poses are worked out on the host by carve_core.h's rel_pose, the same 12 doubles the host function
// uses), one download of the info and ONE wait.  A view's images belong to the view, the records of the last call and the staging of the host-array call to the
// context (RelabelWork), grown by the largest call.  The host function, the defaults and the argument checks are ssm_relabel_host.cpp.
#include "ssm_ctx.h"
#include "ssm_host.h"
using namespace ssm_relabelc;

// what every call checks first: parameters, the views and their poses -> A
static int relabel_begin(ssm_ctx* c, const ssm_relabel_view* const* views, const double* T_views, int v, const double* T_cloud, const ssm_relabel_params* params, RelabelArgs* A)
{
    ssm_relabel_params P; ssm_relabel_params_default(&P); if (params) P = *params;
    { const int r = relabel_check(c, v, P); if (r) return r; }
    if (v && (!views || !T_views)) FAIL(c, SSM_E_INVAL, "null argument");
    { const int r = carve_pose_check(c, T_cloud); if (r) return r; }
    memset(A, 0, sizeof *A);
    A->v = v; A->edge_guard = P.edge_guard; A->own_weight = P.own_weight; A->min_votes = P.min_votes;
    const bool packed = c->relabel.form != RELABEL_FORM_IMAGES;
    for (int k = 0; k < v; k++) {
        const ssm_relabel_view* w = views[k];
        if (!w) FAIL(c, SSM_E_INVAL, "relabel: a null view");
        if (w->owner != c) FAIL(c, SSM_E_INVAL, "relabel: a view of another context");
        for (int j = 0; j < k; j++) if (views[j] == w) FAIL(c, SSM_E_INVAL, "relabel: the same view twice in one call");
        if (packed != (bool)w->packed) FAIL(c, SSM_E_INVAL, "relabel: the view was made under another form");
        const int r = relabel_view_fill(c, w->w, w->h, &w->cam, T_views + 16 * k, T_cloud, P, &A->view[k]); if (r) return r;
        A->view[k].depth = packed ? reinterpret_cast<const uint16_t*>((const uint32_t*)w->packed) : (const uint16_t*)w->depth;
        A->view[k].label = w->label;
    }
    return SSM_OK;
}
// a cloud of this context lies inside the slab of the context's that it names (ssm_map.hip carves every cloud from cloud_slabs)
static bool relabel_owns(const ssm_ctx* c, const ssm_cloud* cl)
{
    if (cl->device != c->device || cl->slab < 0 || (size_t)cl->slab >= c->cloud_slabs.size()) return false;
    const ssm_ctx::CloudSlab& sl = c->cloud_slabs[(size_t)cl->slab];
    const ssm_point* base = sl.d;
    return cl->n >= 0 && cl->d >= base && cl->d + cl->n <= base + sl.cap;
}
// the records for n points
static int relabel_scratch(ssm_ctx* c, int n)
{
    RelabelWork& W = c->relabel;
    if (!W.info) { DALLOC(c, W.h_info, 8); DALLOC(c, W.info, 8); }
    if (n <= W.cap) return SSM_OK;
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    const size_t cap = (size_t)std::max(n, 1024);
    W.cap = 0; W.n = -1;
    DALLOC(c, W.votes, cap); DALLOC(c, W.new_label, cap);
    W.cap = (int)cap;
    return SSM_OK;
}
// everything from the launch to the call's wait; pts: n points in device memory
static int relabel_run(ssm_ctx* c, const RelabelArgs& A, ssm_point* pts, int n, uint32_t* label_out, ssm_relabel_info* info)
{
    RelabelWork& W = c->relabel; hipStream_t s = c->main.stream;
    W.n = -1;
    prof_begin(c, s, "relabel");          // (a stage's time is the SUM over the calls since the records were last reset, as for the sibling stages)
    HIPCHK(c, k_relabel(A, W.form, pts, n, W.votes, W.new_label, W.info, s));
    prof_end(c, s);
    HIPCHK(c, hipMemcpyAsync(W.h_info, W.info, 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    if (label_out && n) HIPCHK(c, hipMemcpyAsync(label_out, W.new_label, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    W.n = n;
    if (info) {
        const unsigned long long* h = W.h_info;
        ssm_relabel_info I{}; I.n_in = n; I.n_supported = (int32_t)h[0]; I.n_voted = (int32_t)h[1]; I.n_changed = (int32_t)h[2]; I.n_filled = (int32_t)h[3];
        I.pairs_supported = (int64_t)h[4]; I.pairs_voted = (int64_t)h[5];
        *info = I;
    }
    return SSM_OK;
}

extern "C" int ssm_relabel_view_create(ssm_ctx* c, const uint16_t* depth, const uint8_t* sem_bgr, int w, int h, const ssm_camera* cam, ssm_relabel_view** view_out)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (!depth || !sem_bgr || !view_out) FAIL(c, SSM_E_INVAL, "null argument");
    *view_out = nullptr;
    { ssm_carve_params P; ssm_carve_params_default(&P); ssm_carvec::Setup S; const int r = carve_check(c, w, h, cam, P, &S); if (r) return r; }
    std::unique_ptr<ssm_relabel_view> v(new ssm_relabel_view());
    v->w = w; v->h = h; v->device = c->device; v->owner = c; v->cam = *cam;
    const size_t np = (size_t)w * h; hipStream_t s = c->main.stream;
    DevBuf<uint8_t> bgr;
    DALLOC(c, v->depth, np); DALLOC(c, v->label, np); DALLOC(c, bgr, np * 3);
    if (c->relabel.form != RELABEL_FORM_IMAGES) DALLOC(c, v->packed, np);
    HIPCHK(c, hipMemcpyAsync(v->depth, depth, np * 2, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(bgr, sem_bgr, np * 3, hipMemcpyHostToDevice, s));
    const hipError_t e = k_relabel_labels(bgr, v->depth, (int64_t)np, v->label, v->packed, s);
    const hipError_t e2 = hipStreamSynchronize(s);          // (the staged BGR image is freed on return: nothing queued may still read it)
    HIPCHK(c, e); HIPCHK(c, e2);
    if (v->packed) v->depth.reset();          // the packed image holds the depths: the vote reads nothing else (the label image stays for ssm_debug_relabel_view)
    *view_out = v.release();
    return SSM_OK;
}
extern "C" void ssm_relabel_view_free(ssm_ctx* c, ssm_relabel_view* v)
{ free_after_wait(c, v); }
extern "C" int ssm_relabel(ssm_ctx* c, const ssm_relabel_view* const* views, const double* T_views, int v, ssm_cloud* cloud, const double* T_cloud,
                           const ssm_relabel_params* params, ssm_relabel_info* info)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (!cloud) FAIL(c, SSM_E_INVAL, "null argument");
    if (!relabel_owns(c, cloud)) FAIL(c, SSM_E_INVAL, "relabel: a cloud of another context");
    RelabelArgs A;
    { int r = relabel_begin(c, views, T_views, v, T_cloud, params, &A); if (!r) r = relabel_scratch(c, cloud->n); if (r) return r; }
    return relabel_run(c, A, cloud->d, cloud->n, nullptr, info);
}
extern "C" int ssm_relabel_points(ssm_ctx* c, const ssm_relabel_view* const* views, const double* T_views, int v, const ssm_point* pts, int n, const double* T_cloud,
                                  const ssm_relabel_params* params, uint32_t* label_out, ssm_relabel_info* info)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    RelabelArgs A;
    { const int r = relabel_begin(c, views, T_views, v, T_cloud, params, &A); if (r) return r; }
    if (n < 0 || (n && (!pts || !label_out))) FAIL(c, SSM_E_INVAL, "null argument");
    { const int r = relabel_scratch(c, n); if (r) return r; }
    RelabelWork& W = c->relabel; hipStream_t s = c->main.stream;
    if ((size_t)n > W.in_cap) {
        HIPCHK(c, hipStreamSynchronize(s));
        const size_t cap = (size_t)std::max(n, 1024);
        W.in_cap = 0; DALLOC(c, W.in, cap); W.in_cap = cap;
    }
    if (n) HIPCHK(c, hipMemcpyAsync(W.in, pts, (size_t)n * sizeof(ssm_point), hipMemcpyHostToDevice, s));
    return relabel_run(c, A, W.in, n, label_out, info);
}
extern "C" int ssm_debug_relabel_record(ssm_ctx* c, uint64_t* votes, uint32_t* new_label, int n)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    RelabelWork& W = c->relabel; hipStream_t s = c->main.stream;
    if (W.n < 0) FAIL(c, SSM_E_INVAL, "relabel: the context has made no call yet");
    if (n != W.n) FAIL(c, SSM_E_INVAL, "relabel: the last call had another number of points");
    if (n == 0) return SSM_OK;
    if (votes) HIPCHK(c, hipMemcpyAsync(votes, W.votes, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    if (new_label) HIPCHK(c, hipMemcpyAsync(new_label, W.new_label, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return SSM_OK;
}
extern "C" int ssm_debug_relabel_view(ssm_ctx* c, const ssm_relabel_view* v, uint8_t* label_out)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (!v || !label_out) FAIL(c, SSM_E_INVAL, "null argument");
    if (v->owner != c) FAIL(c, SSM_E_INVAL, "relabel: a view of another context");
    HIPCHK(c, hipMemcpyAsync(label_out, v->label, (size_t)v->w * v->h, hipMemcpyDeviceToHost, c->main.stream));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    return SSM_OK;
}
extern "C" int ssm_debug_relabel_form(ssm_ctx* c, int form)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (form < -1 || form > RELABEL_FORM_PAIRS) FAIL(c, SSM_E_INVAL, "relabel: the form is 0 (two images), 1 (one packed image), 2 (packed, two views in flight) or -1 (the default)");
    c->relabel.form = form < 0 ? (int)RELABEL_FORM_DEFAULT : form;
    return SSM_OK;
}
