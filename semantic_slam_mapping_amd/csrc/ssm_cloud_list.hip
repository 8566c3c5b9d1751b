// ssm_cloud_list.hip -- the context's side of the cloud-segment table (cloud_table.h) for carving, rendering, alignment and the ground grid: the
// one skeleton of a call that takes a list of clouds (cloud_call), the check of a call's clouds and poses, the staging of clouds that come as host arrays, and the
// table's upload.  The table and the staging (CloudTableWork) are ONE set for them all:
// every entry point holds the context's lock from its first line to its return and ends with a wait on the main stream, so a call finds nothing of the previous
// one in flight.  The numbering and the blocks are ssm_cloud_table.cpp; the limits on a call's points stay with the stages.
#include "ssm_ctx.h"
#include "ssm_host.h"

const double CLOUD_EYE[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

int cloud_list(ssm_ctx* c, const char* twice_msg, const double* T_view, ssm_cloud* const* clouds, const ssm_point* const* pts, const int32_t* n, const double* T_clouds,
               int m, int stride, std::vector<CloudSeg>& segs)
{
    if (!clouds) { const int r = cloud_arrays_check(c, twice_msg, pts, n, T_clouds, m); if (r) return r; }
    segs.assign((size_t)m, CloudSeg{}); int64_t raw = 0;
    for (int k = 0; k < m; k++) {
        if (clouds) {
            const ssm_cloud* cl = clouds[k];
            if (!cl) FAIL(c, SSM_E_INVAL, "null argument");
            if (cl->device != c->device) FAIL(c, SSM_E_INVAL, "cloud of another device");
            if (twice_msg) for (int j = 0; j < k; j++) if (clouds[j] == cl) FAIL(c, SSM_E_INVAL, twice_msg);
            const int r = carve_pose_check(c, T_clouds + 16 * k); if (r) return r;
        }
        ssm_carvec::rel_pose(T_view, T_clouds + 16 * k, segs[k].M);
        const int32_t nk = clouds ? clouds[k]->n : n[k];
        segs[k].pts = clouds ? clouds[k]->d : nullptr; segs[k].n = (int32_t)(((int64_t)nk + stride - 1) / stride); segs[k].stride = stride;
        raw += nk;
    }
    if (clouds || m == 0) return SSM_OK;
    CloudTableWork& W = c->clouds; hipStream_t s = c->main.stream;
    const size_t nn = (size_t)std::max<int64_t>(raw, 1);
    if (nn > W.in_cap) { HIPCHK(c, hipStreamSynchronize(s)); W.in_cap = 0; DALLOC(c, W.in, nn); W.in_cap = nn; }
    size_t at = 0;
    for (int k = 0; k < m; k++) {
        if (n[k]) HIPCHK(c, hipMemcpyAsync(W.in + at, pts[k], (size_t)n[k] * sizeof(ssm_point), hipMemcpyHostToDevice, s));
        segs[k].pts = W.in + at; at += (size_t)n[k];
    }
    return SSM_OK;
}

int cloud_call(ssm_ctx* c, const CloudSource& src, const CloudRule& R, const double* T_view, std::vector<CloudSeg>& segs, int64_t* total)
{
    const int m = src.m;
    *total = 0;
    if (src.kind == CloudSource::VIEWER_MAP) {
        if (!c->d_vmap || c->vmap_n <= 0) FAIL(c, SSM_E_INVAL, src.no_map_msg);
        ssm_cloud vm; vm.d = c->d_vmap; vm.n = c->vmap_n; vm.device = c->device;             // the map as a list of one cloud: borrowed, nothing of it is owned here
        ssm_cloud* const list[1] = {&vm};
        const int r = cloud_list(c, nullptr, T_view, list, nullptr, nullptr, src.T_clouds, 1, R.stride, segs); if (r) return r;
        *total = segs[0].n;
        return SSM_OK;
    }
    const bool handles = src.kind == CloudSource::HANDLES;
    if (m < 0 || (m && (!src.T_clouds || (handles ? !src.clouds : !src.pts || !src.n)))) FAIL(c, SSM_E_INVAL, "null argument");
    if (!handles) { const int r = cloud_total_check(c, R, src.n, m, total); if (r) return r; }          // the counts before the arrays
    { const int r = cloud_list(c, R.twice_msg, T_view, src.clouds, src.pts, src.n, src.T_clouds, m, R.stride, segs); if (r) return r; }
    if (!handles) return SSM_OK;
    for (const CloudSeg& g : segs) *total += g.n;                                                        // a handle's count is never negative: the bound alone, last
    return cloud_bound_check(c, R, *total);
}

void host_wait(ssm_ctx* c)
{
    if (!c) return;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device); hipStreamSynchronize(c->main.stream);
}

int cloud_table_upload(ssm_ctx* c, std::vector<CloudSeg>& segs, int T, CloudTable* t)
{
    CloudTableWork& W = c->clouds; hipStream_t s = c->main.stream;
    const int m = (int)segs.size();
    t->total = cloud_table_build(segs.data(), m, T, nullptr, &t->blocks);
    const size_t seg_bytes = (size_t)m * sizeof(CloudSeg), bytes = seg_bytes + (size_t)t->blocks * 4;
    if (bytes > W.cap) {
        const size_t grown = std::max(bytes, (size_t)8 * sizeof(CloudSeg) + 1024 * 4);
        HIPCHK(c, hipStreamSynchronize(s)); W.cap = 0; DALLOC(c, W.table, grown); DALLOC(c, W.h_table, grown); W.cap = grown;
    }
    // the one place that carves the buffer: the records, then the blocks' first clouds
    CloudSeg* hs = reinterpret_cast<CloudSeg*>((uint8_t*)W.h_table);
    if (m) memcpy(hs, segs.data(), seg_bytes);
    cloud_table_build(hs, m, T, reinterpret_cast<int32_t*>((uint8_t*)W.h_table + seg_bytes), &t->blocks);
    t->seg = W.table.as<CloudSeg>(); t->blk = reinterpret_cast<const int32_t*>((uint8_t*)W.table + seg_bytes);
    if (bytes) { HIPCHK(c, hipMemcpyAsync(W.table, W.h_table, bytes, hipMemcpyHostToDevice, s)); t->in_flight = s; }
    return SSM_OK;
}
