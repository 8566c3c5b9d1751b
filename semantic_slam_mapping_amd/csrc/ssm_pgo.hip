// ssm_pgo.hip -- the device leg of the pose-graph optimiser behind the C ABI (the graph, the plan and every entry point are ssm_pgo_host.cpp): a
// call uploads the host view of each planned graph, launches one block per graph (kernels_pgo.hip) and waits once for the poses and the report.  Inputs and
// workspaces of a graph share ONE device buffer of the object (PgoDev, attached and released through ssm_host.h's hooks), grown by doubling.
#include "ssm_ctx.h"
#include "ssm_host.h"
using namespace ssm_pgc;
struct PgoDev {
    DevBuf<uint8_t> d_buf; size_t d_cap = 0; std::vector<uint8_t> stage;
    DevBuf<View> d_views; int views_cap = 0;
};
int pgo_dev_attach(ssm_pgo* g)
{
    ssm_ctx* c = g->c; std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    size_t fr = 0, tot = 0;
    HIPCHK(c, hipMemGetInfo(&fr, &tot));
    g->cap_bytes = fr / 4; g->dev = new PgoDev();
    return SSM_OK;
}
void pgo_dev_release(ssm_pgo* g) { std::lock_guard<std::mutex> lk(g->c->mu); hipSetDevice(g->c->device); (void)hipStreamSynchronize(g->c->main.stream); delete g->dev; }
// the device twin of a host view: every array at a 16-byte aligned offset of `base`, the inputs first (copied into `stage` when it is given).  Returns the bytes
// needed; *in_bytes = the input part.  with_Hb: H and b are inputs (ssm_pgo_factor_solve)
static size_t device_view(const View& h, size_t csr_n, bool with_Hb, uint8_t* base, std::vector<uint8_t>* stage, View& d, size_t* in_bytes)
{
    size_t off = 0;
    auto put = [&](auto*& dst, const auto* src, size_t count, bool input) {
        typedef std::remove_cv_t<std::remove_pointer_t<std::remove_reference_t<decltype(dst)>>> T;
        const size_t o = (off + 15) & ~(size_t)15, bytes = count * sizeof(T);
        off = o + bytes;
        if (input && stage && bytes) { if (stage->size() < off) stage->resize(off); memcpy(stage->data() + o, src, bytes); }
        dst = reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(base) + o);
    };
    d = h;
    const size_t nv = h.nv, ne = h.ne, nf = h.nf, na = h.na, tot = (size_t)h.env.total;
    put(d.pose, h.pose, nv * 16, true); put(d.efrom, h.efrom, ne, true); put(d.eto, h.eto, ne, true); put(d.robust, h.robust, ne, true);
    put(d.zinv, h.zinv, ne * 16, true); put(d.omega, h.omega, ne * 36, true);
    put(d.aedge, h.aedge, na, true); put(d.vslot, h.vslot, nv, true); put(d.svert, h.svert, nf, true); put(d.csr_off, h.csr_off, nf + 1, true); put(d.csr_edge, h.csr_edge, csr_n, true);
    put(d.env.first, h.env.first, nf, true); put(d.env.rowoff, h.env.rowoff, nf, true); put(d.env.reach, h.env.reach, nf, true);
    if (with_Hb) { put(d.H, h.H, tot, true); put(d.b, h.b, nf * 6, true); }
    off = (off + 15) & ~(size_t)15;
    if (in_bytes) *in_bytes = off;
    if (stage && stage->size() < off) stage->resize(off);
    if (!with_Hb) { put(d.H, h.H, tot, false); put(d.b, h.b, nf * 6, false); }
    put(d.lin, h.lin, na * LIN, false); put(d.L, h.L, tot, false); put(d.x, h.x, nf * 6, false); put(d.y, h.y, nf * 6, false); put(d.d, h.d, nf * 6, false);
    put(d.saved, h.saved, nf * 16, false); put(d.ctl, h.ctl, 1, false); put(d.rep, h.rep, 1, false);
    return ((off + 15) & ~(size_t)15) + 16;
}
// plan -> device buffer -> upload (async on the context stream); dv = the device view.  The context's lock is held
static int pgo_upload(ssm_pgo* g, const View& hv, size_t csr_n, bool with_Hb, View& dv)
{
    ssm_ctx* c = g->c;
    size_t in_bytes = 0;
    const size_t need = device_view(hv, csr_n, with_Hb, nullptr, nullptr, dv, &in_bytes);
    if (need > g->dev->d_cap) {
        HIPCHK(c, hipStreamSynchronize(c->main.stream));
        const size_t cap = std::max(need, 2 * g->dev->d_cap);
        g->dev->d_cap = 0; DALLOC(c, g->dev->d_buf, cap); g->dev->d_cap = cap;
    }
    device_view(hv, csr_n, with_Hb, g->dev->d_buf, &g->dev->stage, dv, &in_bytes);
    if (in_bytes) HIPCHK(c, hipMemcpyAsync(g->dev->d_buf, g->dev->stage.data(), in_bytes, hipMemcpyHostToDevice, c->main.stream));
    return SSM_OK;
}
static int pgo_views(ssm_pgo* g, const View* views, int n)
{
    ssm_ctx* c = g->c;
    if (n > g->dev->views_cap) { HIPCHK(c, hipStreamSynchronize(c->main.stream)); const int cap = std::max(n, 2 * g->dev->views_cap); g->dev->views_cap = 0; DALLOC(c, g->dev->d_views, cap); g->dev->views_cap = cap; }
    HIPCHK(c, hipMemcpyAsync(g->dev->d_views, views, (size_t)n * sizeof(View), hipMemcpyHostToDevice, c->main.stream));
    return SSM_OK;
}
int pgo_dev_optimize(ssm_pgo** graphs, int n, const View* hv, int iterations)
{
    ssm_ctx* c = graphs[0]->c;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    std::vector<View> dv(n);
    for (int i = 0; i < n; i++) { const int r = pgo_upload(graphs[i], hv[i], graphs[i]->plan.csr_edge.size(), false, dv[i]); if (r) return r; }
    { const int r = pgo_views(graphs[0], dv.data(), n); if (r) return r; }
    hipStream_t s = c->main.stream;
    prof_begin(c, s, "pgo");
    HIPCHK(c, k_pgo(graphs[0]->dev->d_views, n, iterations, 0, 0.0, s));
    prof_end(c, s);
    for (int i = 0; i < n; i++) {
        ssm_pgo* g = graphs[i];
        if (g->nv()) HIPCHK(c, hipMemcpyAsync(g->pose.data(), dv[i].pose, (size_t)g->nv() * 128, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(&g->rep, dv[i].rep, sizeof(Report), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(c, hipStreamSynchronize(s));
    return SSM_OK;
}
int pgo_dev_linearize(ssm_pgo* g, const View& v)
{
    const PgoPlan& p = g->plan; ssm_ctx* c = g->c;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    View dv;
    { const int r = pgo_upload(g, v, p.csr_edge.size(), false, dv); if (r) return r; }
    { const int r = pgo_views(g, &dv, 1); if (r) return r; }
    hipStream_t s = c->main.stream;
    HIPCHK(c, k_pgo(g->dev->d_views, 1, 0, 1, 0.0, s));
    HIPCHK(c, hipMemcpyAsync(g->lin.data(), dv.lin, (size_t)p.na * LIN * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(g->H.data(), dv.H, (size_t)p.total * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(g->b.data(), dv.b, (size_t)p.nf * 48, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return SSM_OK;
}
int pgo_dev_factor_solve(ssm_pgo* g, ssm_pgo& t, const View& v, double lambda)
{
    const int nr = t.plan.nf; ssm_ctx* c = g->c;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    View dv;
    { const int r = pgo_upload(g, v, 0, true, dv); if (r) return r; }          // the caller's object owns the device memory
    { const int r = pgo_views(g, &dv, 1); if (r) return r; }
    hipStream_t s = c->main.stream;
    HIPCHK(c, k_pgo(g->dev->d_views, 1, 0, 2, lambda, s));
    HIPCHK(c, hipMemcpyAsync(t.x.data(), dv.x, (size_t)nr * 48, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(&t.ctl, dv.ctl, sizeof(Control), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return SSM_OK;
}
