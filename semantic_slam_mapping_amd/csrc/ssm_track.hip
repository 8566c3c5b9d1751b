// ssm_track.hip -- the device leg of the bulk tracker: what a tracker owns on the device and the hooks (ssm_host.h) through which the host state machine
// (ssm_track_host.cpp) attaches it, releases it and runs the pose chain (kernels_pnp.hip) on a stretch of regular frames.  No access to the context's internals
// (ssm_ctx.h is here for DevBuf, Stream and Event alone).
#include "ssm_ctx.h"
#include "ssm_host.h"
struct TrackDev {         // scratch + the state block, allocated at the first run: t->blocks private slices of the state and of every scratch array, and the cluster's exchange ring
    DevBuf<PnpState> d_state; DevBuf<double> d_pose; DevBuf<ssm_track_info> d_info; DevBuf<float> d_img, d_obj, d_hist;
    DevBuf<uint8_t> d_inl, d_dec; DevBuf<void> d_edges; DevBuf<double2> d_err; int d_cap = 0, d_R = 0, d_n = 0;
    DevBuf<unsigned long long> d_xchg;
    Stream own; Event ev;                 // own_stream: the chain's stream and the event that orders it behind the context's stream
};
#define DCHK(t, call, msg) do { if ((call) != hipSuccess) { (t)->err = (msg); return SSM_E_HIP; } } while (0)
int track_dev_attach(ssm_tracker* t)
{
    const ssm_tracker_params* p = &t->prm; ssm_config cfg; ssm_internal_get_config(t->ctx, &cfg);
    t->cam = cfg.camera; t->ratio = cfg.knn_match_ratio;
    if (cfg.tracker_ref_frames != p->ref_frames) return SSM_E_INVAL;
    // blocks per device chain (kernels_pnp.hip, the cluster form): eight for a chain that has the GPU to itself (latency: -6.5 % per frame; four: -3.4 %); ONE for an
    // own_stream tracker -- those exist to run many chains side by side, where a CU per chain is the efficient form and the blocks of several clusters would
    // have to be resident together.  SSM_PNP_BLOCKS = 1 | 2 | 4 | 8 overrides (same bits in every form).
    { const char* e = getenv("SSM_PNP_BLOCKS"); const int d = p->own_stream ? 1 : 8, g = e ? atoi(e) : (p->blocks > 0 ? p->blocks : d); t->blocks = (g == 1 || g == 2 || g == 4 || g == 8) ? g : d; }
    (void)hipSetDevice(ssm_internal_get_device(t->ctx));           // the raw HIP calls of this file act on the context's device, whatever the calling thread used last
    std::unique_ptr<TrackDev> D(new TrackDev());
    if (p->own_stream && (D->own.ensure() != hipSuccess || D->ev.ensure() != hipSuccess)) return SSM_E_HIP;
    t->dev = D.release();
    return SSM_OK;
}
void track_dev_release(ssm_tracker* t)
{
    (void)hipSetDevice(ssm_internal_get_device(t->ctx)); if (t->dev->own) hipStreamSynchronize(t->dev->own);
    delete t->dev;                                                 // (its stream, event and device buffers with it)
}
static int tracker_ensure_device(ssm_tracker* t, int cap, int R, int n)
{
    TrackDev* D = t->dev;
    if (D->d_state && D->d_cap == cap && D->d_R == R && D->d_n >= n) return SSM_OK;
    ssm_sync(t->ctx);
    D->d_state.reset(); D->d_cap = D->d_R = D->d_n = 0;               // (d_state marks a complete set: a failure below is tried again by the next call)
    const size_t mc = (size_t)R * cap, G = (size_t)t->blocks;          // G private slices of the state and of every scratch array (the cluster form)
    DevBuf<PnpState> st;
    const bool ok = !st.alloc(nullptr, G) && !D->d_pose.alloc(nullptr, (size_t)n * 16) && !D->d_info.alloc(nullptr, (size_t)n) && !D->d_img.alloc(nullptr, G * mc * 2) &&
                    !D->d_obj.alloc(nullptr, G * mc * 3) && !D->d_hist.alloc(nullptr, mc * 3) && !D->d_inl.alloc(nullptr, G * mc) && !D->d_dec.alloc(nullptr, G * mc) &&
                    !D->d_edges.alloc(nullptr, G * mc * k_pnp_edge_bytes()) && !D->d_err.alloc(nullptr, G * mc) && !D->d_xchg.alloc_bytes(nullptr, k_pnp_xchg_bytes());
    if (!ok) { t->err = "device allocation for the pose chain failed"; return SSM_E_NOMEM; }
    D->d_state = std::move(st); D->d_cap = cap; D->d_R = R; D->d_n = n;
    return SSM_OK;
}
// a run of frames on the device: state up, one launch, state and the run's poses down
int track_dev_run(ssm_tracker* t, const ssm_seq_out_dev* seq, int f, int n, PnpState* hs, double* pose_out, std::vector<ssm_track_info>& info)
{
    TrackDev* D = t->dev; const int cap = seq->cap, R = seq->R; (void)hipSetDevice(ssm_internal_get_device(t->ctx));
    { const int rc = tracker_ensure_device(t, cap, R, n); if (rc) return rc; }
    hipStream_t st = (hipStream_t)ssm_stream(t->ctx);
    if (D->own) {                                         // behind everything the context's stream holds now (the call that made `seq`), then on its own
        // (an idle context stream needs no hand-over -- and a marker in its hardware queue would wait behind another tracker's chain whenever the
        // runtime multiplexes the two streams onto one queue)
        if (hipStreamQuery(st) != hipSuccess) { DCHK(t, hipEventRecord(D->ev, st), "stream hand-over failed"); DCHK(t, hipStreamWaitEvent(D->own, D->ev, 0), "stream hand-over failed"); }
        st = D->own;
    }
    for (int r = 0; r < hs->nref; r++) {
        const int idx = hs->ref_idx[r]; const TrackRef& ref = t->refs[r];
        if (idx < 0 && ref.nkp > 0)                       // a frame of the previous call: its positions are no longer on the device
            DCHK(t, hipMemcpyAsync(D->d_hist + (size_t)(idx + R) * cap * 3, ref.pos3d.data(), (size_t)ref.nkp * 12, hipMemcpyHostToDevice, st), "upload of the reference positions failed");
    }
    for (int b = 0; b < t->blocks; b++) DCHK(t, hipMemcpyAsync(D->d_state + b, hs, sizeof(*hs), hipMemcpyHostToDevice, st), "upload of the tracker state failed");
    PnpChainArgs a; a.kps = seq->kps; a.pos3d = seq->pos3d; a.matches = seq->matches; a.nmatch = seq->nmatch; a.hist_pos3d = D->d_hist;
    a.cap = cap; a.R = R; a.f_begin = f; a.f_end = n; a.max_lost = t->prm.max_lost_frame;
    a.cam.fx = t->cam.fx; a.cam.fy = t->cam.fy; a.cam.cx = t->cam.cx; a.cam.cy = t->cam.cy;
    a.state = D->d_state; a.pose_out = D->d_pose; a.info_out = D->d_info; a.img = D->d_img; a.obj = D->d_obj; a.inl = D->d_inl; a.dec = D->d_dec; a.ledges = D->d_edges.as<LEdge>(); a.err = D->d_err; a.edges_in_lds = 0;
    a.blocks = t->blocks; a.xchg = D->d_xchg; a.xfail = reinterpret_cast<unsigned*>(D->d_xchg.as<unsigned char>() + k_pnp_xchg_bytes() - 64);
    DCHK(t, k_pnp_chain(a, st), "pose chain launch failed");
    DCHK(t, hipMemcpyAsync(hs, D->d_state, sizeof(*hs), hipMemcpyDeviceToHost, st), "pose chain failed"); DCHK(t, hipStreamSynchronize(st), "pose chain failed");
    if (hs->stopped_at == -1 && t->blocks > 1) return SSM_OK;          // the cluster's exchange timed out: the caller repeats the range with one block
    const int stop = hs->stopped_at;
#ifdef SSM_PNP_PROF
    fprintf(stderr, "pnp chain %d frames: clocks gather %lld fused %lld algebra %lld chi %lld update %lld solve(total) %lld; fused passes %lld chi passes %lld\n", stop - f, hs->prof[0], hs->prof[1], hs->prof[2], hs->prof[3], hs->prof[4], hs->prof[5], hs->prof[6], hs->prof[7]);
    fprintf(stderr, "  fused: edges + group tree %lld | finish: barrier %lld publish %lld poll %lld barrier %lld sum %lld;  chi: items %lld barrier %lld sums %lld barrier %lld | finish: barrier %lld publish %lld poll %lld row sum %lld barrier %lld\n",
            hs->prof[24], hs->prof[8], hs->prof[9], hs->prof[10], hs->prof[11], hs->prof[12], hs->prof[25], hs->prof[26], hs->prof[27], hs->prof[28], hs->prof[16], hs->prof[17], hs->prof[18], hs->prof[19], hs->prof[20]);
    fprintf(stderr, "  algebra: ldlt %lld exp map %lld publish + barrier %lld\n", hs->prof[29], hs->prof[30], hs->prof[31]);
#endif
    if (stop <= f || stop > n) { t->err = "pose chain returned an invalid frame range"; return SSM_E_HIP; }
    info.resize(stop - f);
    DCHK(t, hipMemcpy(pose_out + (size_t)f * 16, D->d_pose + (size_t)f * 16, (size_t)(stop - f) * 128, hipMemcpyDeviceToHost), "pose download failed");
    DCHK(t, hipMemcpy(info.data(), D->d_info + f, (size_t)(stop - f) * sizeof(ssm_track_info), hipMemcpyDeviceToHost), "info download failed");
    return SSM_OK;
}
