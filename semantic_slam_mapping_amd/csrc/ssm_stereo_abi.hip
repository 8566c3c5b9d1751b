// ssm_stereo_abi.hip -- the stereo path behind the C ABI: QuadFeatureMatch (GFTT + LK), cv::StereoSGBM + the depth conversion, VisualOdometryStereo, and
// PnPSolver::solvePnP for one correspondence list.  Kernels: kernels_quad.hip, kernels_sgbm.hip, kernels_vo.hip, kernels_pnp.hip.
#include "ssm_ctx.h"

// ---------------------------------------------------------------- stereo path: QuadFeatureMatch, StereoSGBM depth, VisualOdometryStereo
// exact: the row stride of the sequence outputs is max_corners, so the sequence path wants exactly that many; the per-call entry points take any workspace that is large enough
static int stereo_init(ssm_ctx* c, int w, int h, int maxc, bool exact = false)
{
    if (c->stereo && c->stereo->w == w && c->stereo->h == h && (exact ? c->stereo->maxc == maxc : c->stereo->maxc >= maxc)) return SSM_OK;
    if (w < 4 || h < 2 || w > 4096 || h > 4096) FAIL(c, SSM_E_INVAL, "stereo path: image size must be at most 4096 x 4096");
    if (maxc < 1 || maxc > 32767) FAIL(c, SSM_E_INVAL, "max_corners must be 1..32767");
    if (c->stereo) { hipDeviceSynchronize(); c->stereo.reset(); }
    // built aside and handed to the context complete: a failure below leaves c->stereo null and the next call builds again
    std::unique_ptr<StereoState> q(new StereoState());
    q->w = w; q->h = h; q->maxc = maxc; q->B = c->stereo_B;
    const int B = q->B;
    QuadBatch& b = q->qb;
    int off = 0;
    for (int l = 0; l < 4; l++) { b.w[l] = l ? (b.w[l-1] + 1) / 2 : w; b.h[l] = l ? (b.h[l-1] + 1) / 2 : h; b.off[l] = off; off += b.w[l] * b.h[l]; off = (off + 15) & ~15; }
    b.slot_elems = (size_t)off; b.B1 = B + 1;
    DALLOC(c, q->pyr, (size_t)2 * b.B1 * b.slot_elems); DALLOC(c, q->der, (size_t)2 * b.B1 * b.slot_elems * 2);
    b.pyr = q->pyr; b.der = q->der;
    const size_t np = (size_t)w * h;
    // candidate list of a frame: 3x3 maxima keep ties, so a plateau of equal eigenvalues makes almost every pixel a candidate; a frame with more than this is
    // selected on the pixel grid instead (gftt_select_pixels), whose kept corners must fit in the list up to max_corners
    q->keycap = w * h / 4 + 1024 > maxc ? w * h / 4 + 1024 : maxc;
    GfttWork& g = q->gw; g.cap = q->keycap;
    DALLOC(c, q->g_eig, (size_t)B * np); DALLOC(c, q->g_cand_at, (size_t)B * np); DALLOC(c, q->g_keys, (size_t)B * q->keycap); DALLOC(c, q->g_kept, (size_t)B * q->keycap);
    DALLOC(c, q->g_deps, (size_t)B * q->keycap * k_quad_gftt_deps_per_candidate()); DALLOC(c, q->g_depn, (size_t)B * q->keycap); DALLOC(c, q->g_state, (size_t)B * q->keycap);
    HIPCHK(c, hipMemset(q->g_cand_at, 0, (size_t)B * np * 4));      // gftt_finish_kernel keeps the map zeroed between calls
    DALLOC(c, q->g_cand_bits, (size_t)B * k_quad_gftt_bits_words(w, h));
    DALLOC(c, q->g_maxord, B); DALLOC(c, q->g_count, B); DALLOC(c, q->g_nkept, B); DALLOC(c, q->sg_fail, SG_FAIL_WORDS); DALLOC(c, q->ncorner, B); DALLOC(c, q->has_prev, B);
    g.eig = q->g_eig; g.cand_at = q->g_cand_at; g.cand_bits = q->g_cand_bits; g.keys = q->g_keys; g.kept = q->g_kept; g.deps = q->g_deps; g.depn = q->g_depn; g.state = q->g_state;
    g.maxord = q->g_maxord; g.count = q->g_count; g.nkept = q->g_nkept;
    HIPCHK(c, hipMemset(q->sg_fail, 0, 4 * SG_FAIL_WORDS));
    DALLOC(c, q->pts, (size_t)5 * B * maxc * 2); DALLOC(c, q->status, maxc); DALLOC(c, q->err, maxc);
    DALLOC(c, q->rand_off, B); DALLOC(c, q->consumed, 1);
    c->stereo = std::move(q);
    return SSM_OK;
}
static int stereo_ensure_seq(ssm_ctx* c, int n)
{
    StereoState* q = c->stereo.get();
    if (n <= q->seq_cap) return SSM_OK;
    HIPCHK(c, hipDeviceSynchronize());
    q->seq_cap = 0;
    const size_t np = (size_t)q->w * q->h;
    DALLOC(c, q->quad, (size_t)n * q->maxc); DALLOC(c, q->nquad, n); DALLOC(c, q->corners, (size_t)n * q->maxc * 2); DALLOC(c, q->ncorners, n);
    DALLOC(c, q->disp, (size_t)n * np); DALLOC(c, q->depth, (size_t)n * np);
    DALLOC(c, q->tr, (size_t)n * 6); DALLOC(c, q->inliers, (size_t)n * q->maxc); DALLOC(c, q->vo_result, (size_t)n * 2);
    q->seq_cap = n;
    return SSM_OK;
}
static int stereo_ensure_vo(ssm_ctx* c, int iters)
{
    StereoState* q = c->stereo.get();
    if (iters <= q->vo_iters) return SSM_OK;
    HIPCHK(c, hipDeviceSynchronize());
    q->vo_iters = 0;
    DALLOC(c, q->tr_all, (size_t)q->B * iters * 6); DALLOC(c, q->vcount, (size_t)q->B * iters);
    q->vo_iters = iters;
    return SSM_OK;
}
static int stereo_ensure_sgbm(ssm_ctx* c, const ssm_sgbm_params& p, int nb, int which = 0)
{
    StereoState* q = c->stereo.get();
    const size_t need = k_sgbm_workspace_bytes(q->w, q->h, p, nb, c->sgbm_form_cfg);
    if (!q->dminN[which]) DALLOC(c, q->dminN[which], 128);
    if (need <= q->sg_wsN[which].bytes()) return SSM_OK;
    HIPCHK(c, hipDeviceSynchronize());
    return q->sg_wsN[which].alloc(c, need);
}
static int sgbm_check_params(ssm_ctx* c, const ssm_sgbm_params* params, int w, int h)
{
    if (!params) FAIL(c, SSM_E_INVAL, "null SGBM parameters");
    const int D = params->numberOfDisparities, SW = params->SADWindowSize > 0 ? params->SADWindowSize : 5;
    if (D <= 0 || D % 16 || D > 128 || D / 16 == 7) FAIL(c, SSM_E_INVAL, "numberOfDisparities must be 16, 32, 48, 64, 80, 96 or 128");
    if (!(SW & 1) || h <= SW || w <= SW) FAIL(c, SSM_E_INVAL, "SADWindowSize must be odd and smaller than the image");
    if ((long long)w * h >= (1ll << 30)) FAIL(c, SSM_E_INVAL, "image too large");
    { int tx; size_t lds; if (!sgbm_cost_geometry(D, SW, &tx, &lds)) FAIL(c, SSM_E_INVAL, "SADWindowSize too large for this numberOfDisparities (the cost kernel keeps SADWindowSize rows of 4 columns x D sums in LDS)"); }
    return SSM_OK;
}
static int quad_size_check(ssm_ctx* c, int w, int h) { if (w < 32 || h < 32) FAIL(c, SSM_E_INVAL, "quad matcher: image size must be 32..4096"); return SSM_OK; }
// the sequence path on device images; the caller holds the context lock
// pair_call: the caller is ssm_quad_track (frame 0 = the previous pair of ONE matcher call: only its pyramids and derivatives are needed -- its corners and tracks
// are nobody's output, and skipping them takes a third off the call: 1.06 -> 0.8 ms at 1241 x 376)
static int stereo_seq_run(ssm_ctx* c, const ssm_stereo_frames_dev* in, ssm_stereo_out_dev* out, bool pair_call = false)
{
    const int n = in->n, w = in->w, h = in->h;
    const int stages = in->stages ? in->stages : (SSM_STEREO_QUAD | SSM_STEREO_DEPTH | SSM_STEREO_VO);
    if (n < 0 || !in->left || !in->right) FAIL(c, SSM_E_INVAL, "bad arguments");
    if ((stages & SSM_STEREO_VO) && !(stages & SSM_STEREO_QUAD)) FAIL(c, SSM_E_INVAL, "SSM_STEREO_VO needs SSM_STEREO_QUAD");
    if ((stages & SSM_STEREO_VO) && (in->ransac_iters < 0 || (in->ransac_iters > 0 && !in->rand_stream))) FAIL(c, SSM_E_INVAL, "the VO stage needs rand_stream (n * ransac_iters * 3 draws)");
    const int maxc = in->max_corners > 0 ? in->max_corners : 1000;
    int r = (stages & SSM_STEREO_QUAD) ? quad_size_check(c, w, h) : SSM_OK; if (r) return r;
    r = stereo_init(c, w, h, maxc, true); if (r) return r;
    StereoState* q = c->stereo.get();
    q->lk_built = false;                                          // (the sub-batch overwrites slot 1)
    if (stages & SSM_STEREO_DEPTH) { r = sgbm_check_params(c, &in->sgbm, w, h); if (r) return r; }
    r = stereo_ensure_seq(c, n > 0 ? n : 1); if (r) return r;
    if (stages & SSM_STEREO_VO) { r = stereo_ensure_vo(c, in->ransac_iters > 0 ? in->ransac_iters : 1); if (r) return r; }
    const int B = q->B;
    if (stages & SSM_STEREO_DEPTH) { r = stereo_ensure_sgbm(c, in->sgbm, n < B ? (n > 0 ? n : 1) : B); if (r) return r; }
    const size_t np = (size_t)w * h;
    const QuadBatch& qb = q->qb;
    const hipStream_t sq = c->main.stream;
    // SGBM beside the quad matcher + VO chain, alternating between lanes with a workspace each: ssm_seq_plan.cpp
    const StereoPlan plan = stereo_plan(n, B, stages, c->serialize, c->stereo_sgbm_streams);
    const int nsg = plan.nsg;
    if (plan.two) { r = ensure_side_streams(c); if (r) return r; }
    for (int k = 1; k < nsg; k++) { r = stereo_ensure_sgbm(c, in->sgbm, B, k); if (r) return r; }
    r = lanes_fork(c, plan.forked); if (r) return r;
    prof_reset(c);
    const bool prev0 = in->continue_sequence && q->have_prev;
    if (stages & SSM_STEREO_VO) HIPCHK(c, hipMemsetAsync(q->consumed, 0, 4, sq));
    for (int f0 = 0; f0 < n; f0 += B) {
        const int nb = n - f0 < B ? n - f0 : B;
        if (stages & SSM_STEREO_QUAD) {
            prof_begin(c, sq, "quad_track");
            // level 0 of the nb frames into slots 1 .. nb of both sides, then the pyramids and derivatives
            HIPCHK(c, hipMemcpy2DAsync(q->pyr + (size_t)(0 * qb.B1 + 1) * qb.slot_elems, qb.slot_elems, in->left + (size_t)f0 * np, np, np, nb, hipMemcpyDeviceToDevice, sq));
            HIPCHK(c, hipMemcpy2DAsync(q->pyr + (size_t)(1 * qb.B1 + 1) * qb.slot_elems, qb.slot_elems, in->right + (size_t)f0 * np, np, np, nb, hipMemcpyDeviceToDevice, sq));
            HIPCHK(c, k_quad_pyramids(qb, nb, sq));
            HIPCHK(c, hipMemsetAsync(q->has_prev, 1, 4 * (size_t)nb, sq));                      // non-zero = true
            if (f0 == 0 && !prev0) HIPCHK(c, hipMemsetAsync(q->has_prev, 0, 4, sq));
            if (!(pair_call && f0 == 0 && nb == 1 && !prev0)) {
            HIPCHK(c, k_quad_gftt(qb, nb, maxc, 0.04, 8.0, q->gw, q->pts, maxc, q->ncorner, sq));      // quadmatcher.cpp:301-308
            HIPCHK(c, k_quad_track(qb, nb, q->pts, maxc, q->ncorner, q->has_prev, q->quad + (size_t)f0 * maxc, q->nquad + f0, sq));
            HIPCHK(c, hipMemcpyAsync(q->corners + (size_t)f0 * maxc * 2, q->pts, (size_t)nb * maxc * 8, hipMemcpyDeviceToDevice, sq));
            HIPCHK(c, hipMemcpyAsync(q->ncorners + f0, q->ncorner, (size_t)nb * 4, hipMemcpyDeviceToDevice, sq));
            }
            // carry: the last frame of the sub-batch becomes slot 0 (images and derivatives, both sides)
            for (int side = 0; side < 2; side++) {
                HIPCHK(c, hipMemcpyAsync(q->pyr + (size_t)(side * qb.B1) * qb.slot_elems, q->pyr + (size_t)(side * qb.B1 + nb) * qb.slot_elems, qb.slot_elems, hipMemcpyDeviceToDevice, sq));
                HIPCHK(c, hipMemcpyAsync(q->der + (size_t)(side * qb.B1) * qb.slot_elems * 2, q->der + (size_t)(side * qb.B1 + nb) * qb.slot_elems * 2, qb.slot_elems * 4, hipMemcpyDeviceToDevice, sq));
            }
            prof_end(c, sq);
        }
        if (stages & SSM_STEREO_VO) {
            prof_begin(c, sq, "vo");
            HIPCHK(c, k_vo_estimate_batch(q->quad + (size_t)f0 * maxc, maxc, q->nquad + f0, nb, in->vo, in->rand_stream, in->ransac_iters, q->consumed, q->rand_off,
                                          q->tr_all, q->vcount, q->tr + (size_t)f0 * 6, q->inliers + (size_t)f0 * maxc, q->vo_result + (size_t)f0 * 2, sq));
            prof_end(c, sq);
        }
        if (stages & SSM_STEREO_DEPTH) {
            const int alt = plan.work(f0 / B);
            Lane& sl = lane(c, plan.lane(f0 / B)); const hipStream_t sg = sl.stream;
            prof_begin(c, sg, "sgbm");                                  // (the stage events on SGBM's stream)
            HIPCHK(c, k_sgbm(in->left + (size_t)f0 * np, in->right + (size_t)f0 * np, w, h, nb, in->sgbm, q->sg_wsN[alt], q->sg_wsN[alt].bytes(), q->disp + (size_t)f0 * np, 0, c->dev, sl.sg, sg,
                             q->sg_fail + (f0 / B) % SG_FAIL_WORDS, c->sgbm_form_cfg, nsg));
            HIPCHK(c, k_sgbm_depth(q->disp + (size_t)f0 * np, w, h, nb, in->baseline, in->cu, in->cv, in->f, in->roix, in->roiy, in->roiz, in->scale, q->dminN[alt], q->depth + (size_t)f0 * np, sg));
            prof_end(c, sg);
        }
    }
    r = lanes_join(c, plan.forked); if (r) return r;
    if (n > 0) q->have_prev = (stages & SSM_STEREO_QUAD) != 0;
    q->sg_pending.valid = (stages & SSM_STEREO_DEPTH) && n > 0;
    if (q->sg_pending.valid) { q->sg_pending.in = *in; q->sg_pending.B = B; }
    if (out) {
        out->quad = q->quad; out->nquad = q->nquad; out->corners = q->corners; out->ncorners = q->ncorners; out->disp = q->disp; out->depth = q->depth;
        out->tr = q->tr; out->inliers = q->inliers; out->vo_result = q->vo_result; out->rand_draws_used = q->consumed; out->max_corners = maxc;
    }
    return SSM_OK;
}
extern "C" int ssm_stereo_batch(const ssm_ctx* c) { return c ? c->stereo_B : 0; }
extern "C" int ssm_stereo_seq_process(ssm_ctx* c, const ssm_stereo_frames_dev* in, ssm_stereo_out_dev* out)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (!in) FAIL(c, SSM_E_INVAL, "null argument");
    return stereo_seq_run(c, in, out);
}
// The pinned area of a per-pair call on images of np pixels.  Going up: [image 0] .. [image 3], packed, which StereoState::in_stage mirrors on the device.  Coming
// back, once the upload has consumed the images: [the sweep's time-out word] .. [disparity, behind two images][depth].
struct PairBlock {
    size_t np, plane, fail = 0, disp, depth, bytes, stage_bytes;  // plane: bytes of the disparity (int16) or depth (uint16) image; stage_bytes: four images (ssm_quad_track)
    explicit PairBlock(size_t np_) : np(np_), plane(np * sizeof(int16_t)), disp(image(2)), depth(disp + plane), bytes(depth + plane), stage_bytes(image(4)) {}
    size_t image(int k) const { return k * np; }
};
// host images -> packed device staging (StereoState::in_stage): slot k of the staging area holds image k ([h][w] bytes each); through pinned memory (a pageable
// copy of a 1241x376 image costs ~1 ms)
static int stereo_stage_images(ssm_ctx* c, const uint8_t* const* imgs, int nimg, int w, int h, int stride)
{
    StereoState* q = c->stereo.get();
    const PairBlock P((size_t)w * h);
    int r = ensure_pinned(c, P.bytes > P.image(nimg) ? P.bytes : P.image(nimg)); if (r) return r;
    if (P.image(nimg) > q->in_stage.bytes()) {
        HIPCHK(c, hipDeviceSynchronize());
        DALLOC(c, q->in_stage, P.stage_bytes);
    }
    HIPCHK(c, hipStreamSynchronize(c->main.stream));               // the previous call's copies out of the staging buffer are done
    for (int k = 0; k < nimg; k++)
        for (int y = 0; y < h; y++) memcpy(c->h_pinned + P.image(k) + (size_t)y * w, imgs[k] + (size_t)y * stride, w);
    HIPCHK(c, hipMemcpyAsync(q->in_stage, c->h_pinned, P.image(nimg), hipMemcpyHostToDevice, c->main.stream));
    return SSM_OK;
}
extern "C" int ssm_quad_track(ssm_ctx* c, const uint8_t* lc, const uint8_t* rc, const uint8_t* lp, const uint8_t* rp, int w, int h, int stride,
                              int max_corners, ssm_pmatch* out, int cap, int* n_out)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (!lc || !rc || !lp || !rp || !n_out || stride < w || max_corners < 1) FAIL(c, SSM_E_INVAL, "bad arguments");
    int r = stereo_init(c, w, h, max_corners, true); if (r) return r;
    // a two-frame sequence: frame 0 = the previous pair, frame 1 = the current pair (left images first, then the right ones)
    const uint8_t* imgs[4] = { lp, lc, rp, rc };
    r = stereo_stage_images(c, imgs, 4, w, h, stride); if (r) return r;
    uint8_t* dev = c->stereo->in_stage;
    ssm_stereo_frames_dev in; memset(&in, 0, sizeof(in));
    in.left = dev; in.right = dev + PairBlock((size_t)w * h).image(2); in.n = 2; in.w = w; in.h = h; in.stages = SSM_STEREO_QUAD; in.max_corners = max_corners;
    ssm_stereo_out_dev o;
    r = stereo_seq_run(c, &in, &o, true); if (r) return r;
    c->stereo->have_prev = false;                                // a per-pair call is not part of a sequence
    int m = 0;
    HIPCHK(c, hipMemcpyAsync(&m, o.nquad + 1, 4, hipMemcpyDeviceToHost, c->main.stream));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    r = check_device_flags(c, false); if (r) return r;
    *n_out = m;
    if (m > cap) FAIL(c, SSM_E_CAPACITY, "pmatch buffer too small (need " + std::to_string(m) + ")");
    if (m > 0) HIPCHK(c, hipMemcpy(out, o.quad + o.max_corners, (size_t)m * sizeof(ssm_pmatch), hipMemcpyDeviceToHost));
    return SSM_OK;
}
// level 0 of a host image into slot 1 of `side` (what the per-call GFTT and LK read)
static int quad_upload_slot1(ssm_ctx* c, int side, const uint8_t* img, int stride)
{
    StereoState* q = c->stereo.get(); q->lk_built = false;
    HIPCHK(c, hipMemcpy2DAsync(q->pyr + (size_t)(side * q->qb.B1 + 1) * q->qb.slot_elems, q->w, img, stride, q->w, q->h, hipMemcpyHostToDevice, c->main.stream));
    return SSM_OK;
}
extern "C" int ssm_gftt(ssm_ctx* c, const uint8_t* img, int w, int h, int stride, int max_corners, double quality, double min_distance,
                        float* pts, int cap, int* n_out)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (!img || !pts || !n_out || stride < w || max_corners < 1 || !(min_distance >= 1.0)) FAIL(c, SSM_E_INVAL, "bad arguments (max_corners >= 1, min_distance >= 1)");
    if (min_distance > 64.0) FAIL(c, SSM_E_INVAL, "min_distance must be <= 64");
    int r = quad_size_check(c, w, h); if (r) return r;
    if (max_corners > 32767) FAIL(c, SSM_E_INVAL, "max_corners must be <= 32767");
    r = stereo_init(c, w, h, max_corners); if (r) return r;
    StereoState* q = c->stereo.get(); const QuadBatch& qb = q->qb;
    r = quad_upload_slot1(c, 0, img, stride); if (r) return r;
    HIPCHK(c, k_quad_gftt(qb, 1, max_corners, quality, min_distance, q->gw, q->pts, q->maxc, q->ncorner, c->main.stream));
    int n = 0;
    HIPCHK(c, hipMemcpyAsync(&n, q->ncorner, 4, hipMemcpyDeviceToHost, c->main.stream));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    r = check_device_flags(c, false); if (r) return r;
    *n_out = n;
    if (n > cap) FAIL(c, SSM_E_CAPACITY, "point buffer too small");
    if (n) HIPCHK(c, hipMemcpy(pts, q->pts, (size_t)n * 8, hipMemcpyDeviceToHost));
    return SSM_OK;
}
extern "C" int ssm_lk_track(ssm_ctx* c, const uint8_t* prev, const uint8_t* next, int w, int h, int stride, const float* prev_pts, int n,
                            float* next_pts, uint8_t* status, float* err, int max_count, double epsilon, double min_eig_threshold)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (!prev || !next || n < 0 || (n && (!prev_pts || !next_pts)) || stride < w || max_count < 1) FAIL(c, SSM_E_INVAL, "bad arguments");
    if (n == 0) return SSM_OK;
    int r = quad_size_check(c, w, h); if (r) return r;
    r = stereo_init(c, w, h, n > 1000 ? n : 1000); if (r) return r;
    StereoState* q = c->stereo.get(); const QuadBatch& qb = q->qb;
    // previous image = (side 0, slot 1), next image = (side 1, slot 1)
    if ((r = quad_upload_slot1(c, 0, prev, stride)) || (r = quad_upload_slot1(c, 1, next, stride))) return r;
    HIPCHK(c, k_quad_pyramids(qb, 1, c->main.stream));
    float* d_in = q->pts; float* d_out = q->pts + (size_t)2 * q->maxc;
    HIPCHK(c, hipMemcpyAsync(d_in, prev_pts, (size_t)n * 8, hipMemcpyHostToDevice, c->main.stream));
    HIPCHK(c, k_quad_lk(qb, d_in, n, d_out, q->status, q->err, max_count, (float)(epsilon * epsilon), (float)min_eig_threshold, c->main.stream));
    HIPCHK(c, hipMemcpyAsync(next_pts, d_out, (size_t)n * 8, hipMemcpyDeviceToHost, c->main.stream));
    if (status) HIPCHK(c, hipMemcpyAsync(status, q->status, n, hipMemcpyDeviceToHost, c->main.stream));
    if (err) HIPCHK(c, hipMemcpyAsync(err, q->err, (size_t)n * 4, hipMemcpyDeviceToHost, c->main.stream));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    c->stereo->have_prev = false;
    c->stereo->lk_built = true;
    return SSM_OK;
}
// what the LK kernels of the last ssm_lk_track read (exact tests of pyrdown_kernel and scharr_kernel on every pixel): one level of slot 1 of `side`
extern "C" int ssm_debug_quad_pyramid(ssm_ctx* c, int side, int level, uint8_t* img, int16_t* der, int* w, int* h)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (side < 0 || side > 1 || level < 0 || level > 3) FAIL(c, SSM_E_INVAL, "bad arguments (side 0..1, level 0..3)");
    StereoState* q = c->stereo.get();
    if (!q || !q->lk_built) FAIL(c, SSM_E_INVAL, "no LK state: ssm_lk_track (n > 0) must be the last stereo call on this context");
    const QuadBatch& qb = q->qb;
    const size_t at = (size_t)(side * qb.B1 + 1) * qb.slot_elems + qb.off[level], np = (size_t)qb.w[level] * qb.h[level];
    if (w) *w = qb.w[level];
    if (h) *h = qb.h[level];
    if (img) HIPCHK(c, hipMemcpyAsync(img, q->pyr + at, np, hipMemcpyDeviceToHost, c->main.stream));
    if (der) HIPCHK(c, hipMemcpyAsync(der, q->der + 2 * at, np * 4, hipMemcpyDeviceToHost, c->main.stream));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    return SSM_OK;
}
extern "C" int ssm_window_match(ssm_ctx* c, const float* kp1, const uint8_t* d1, int n1, const float* kp2, const uint8_t* d2, int n2,
                                int search_width, int search_height, float distance_threshold, ssm_dmatch* out)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (n1 < 0 || n2 < 0 || (n1 && (!kp1 || !d1 || !out)) || (n2 && (!kp2 || !d2))) FAIL(c, SSM_E_INVAL, "bad arguments");
    if (n1 == 0) return SSM_OK;
    Carve k; const size_t o_k1 = k.take<float>(2 * (size_t)n1), o_k2 = k.take<float>(2 * (size_t)n2), o_d1 = k.take<uint8_t>(32 * (size_t)n1), o_d2 = k.take<uint8_t>(32 * (size_t)n2), o_m = k.take<ssm_dmatch>(n1);
    k.take<uint8_t>(256, 1); int r = ensure_scratch(c, k.off); if (r) return r;      // (256 spare)
    uint8_t* p = (uint8_t*)c->d_scratch;
    float* dk1 = (float*)(p + o_k1); float* dk2 = (float*)(p + o_k2); uint8_t* dd1 = p + o_d1; uint8_t* dd2 = p + o_d2; ssm_dmatch* dm = (ssm_dmatch*)(p + o_m);
    HIPCHK(c, hipMemcpyAsync(dk1, kp1, (size_t)n1 * 8, hipMemcpyHostToDevice, c->main.stream)); HIPCHK(c, hipMemcpyAsync(dd1, d1, (size_t)n1 * 32, hipMemcpyHostToDevice, c->main.stream));
    if (n2) { HIPCHK(c, hipMemcpyAsync(dk2, kp2, (size_t)n2 * 8, hipMemcpyHostToDevice, c->main.stream)); HIPCHK(c, hipMemcpyAsync(dd2, d2, (size_t)n2 * 32, hipMemcpyHostToDevice, c->main.stream)); }
    HIPCHK(c, k_quad_window_match(dk1, dd1, n1, dk2, dd2, n2, search_width, search_height, distance_threshold, dm, c->main.stream));
    HIPCHK(c, hipMemcpyAsync(out, dm, (size_t)n1 * 16, hipMemcpyDeviceToHost, c->main.stream));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    return SSM_OK;
}

// ---------------------------------------------------------------- depth from stereo (cv::StereoSGBM + FrameReader's conversion)
extern "C" void ssm_sgbm_params_default(ssm_sgbm_params* p)
{
    if (!p) return;
    p->minDisparity = 0; p->numberOfDisparities = 80; p->SADWindowSize = 11; p->P1 = 4 * 11 * 11; p->P2 = 32 * 11 * 11;       // src/stereo.cpp:16-27
    p->disp12MaxDiff = 1; p->preFilterCap = 63; p->uniquenessRatio = 10; p->speckleWindowSize = 100; p->speckleRange = 32;
}
// cv::StereoSGBM cannot fail (src/stereo.cpp:11-30); form 2's sweep can: its strips wait for each other, and when a hand-off exceeds its spin bound every block
// leaves mid-image with the sub-batch's fail word set.  Called with the streams drained: every sub-batch of the last sequence call whose word is set is computed again
// with form 1 (independent paths, no cross-block waits; the workspace holds its volumes anyway) from the caller's input images, so that the call's disparities and depths
// are the oracle's after all.  Reported through ssm_last_error (a note, the call succeeds) and counted in sgbm_fallbacks.
int sgbm_recover(ssm_ctx* c)
{
    StereoState* q = c->stereo.get();
    int32_t sf[SG_FAIL_WORDS];
    HIPCHK(c, hipMemcpy(sf, q->sg_fail, sizeof(sf), hipMemcpyDeviceToHost));
    bool any = false; for (int k = 0; k < SG_FAIL_WORDS; k++) any = any || sf[k] != 0;
    if (!any) return SSM_OK;
    HIPCHK(c, hipMemset(q->sg_fail, 0, sizeof(sf)));
    if (!q->sg_pending.valid) FAIL(c, SSM_E_HIP, "SGBM sweep: a strip hand-off timed out and the call that launched it is no longer known (the disparities are incomplete)");
    const ssm_stereo_frames_dev& in = q->sg_pending.in; const int B = q->sg_pending.B, w = q->w, h = q->h; const size_t np = (size_t)w * h;
    int redone = 0;
    for (int f0 = 0, bi = 0; f0 < in.n; f0 += B, bi++) {
        if (!sf[bi % SG_FAIL_WORDS]) continue;
        const int nb = in.n - f0 < B ? in.n - f0 : B;
        HIPCHK(c, k_sgbm(in.left + (size_t)f0 * np, in.right + (size_t)f0 * np, w, h, nb, in.sgbm, q->sg_wsN[0], q->sg_wsN[0].bytes(), q->disp + (size_t)f0 * np, 0, c->dev, c->main.sg, c->main.stream, q->sg_fail + bi % SG_FAIL_WORDS, 1, 1));
        HIPCHK(c, k_sgbm_depth(q->disp + (size_t)f0 * np, w, h, nb, in.baseline, in.cu, in.cv, in.f, in.roix, in.roiy, in.roiz, in.scale, q->dminN[0], q->depth + (size_t)f0 * np, c->main.stream));
        redone++;
    }
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    c->sgbm_fallbacks += redone;
    c->err = "note: the SGBM sweep of " + std::to_string(redone) + " sub-batch(es) timed out in a strip hand-off; they were repeated with form 1 (results complete)";
    return SSM_OK;
}
// One host pair through the batched kernels (nb = 1): images staged on the device, disparity (and depth, with `da`) left in the sequence output buffers and brought
// back through the pinned area (PairBlock) together with the sweep kernel's time-out word.  A sweep whose hand-off timed out is repeated once, in form 1 (no
// cross-block waits): the host-pointer entry points repeat it themselves, with a note.  disp may be null with depth.
struct DepthArgs { double baseline, cu, cv, f, roix, roiy, roiz, scale; };
static int sgbm_pair(ssm_ctx* c, const uint8_t* left, const uint8_t* right, int w, int h, int stride, const ssm_sgbm_params* params, int stage,
                     const DepthArgs* da /* null: no conversion */, int16_t* disp, uint16_t* depth)
{
    if (!left || !right || !params || w < 3 || h < 1 || stride < w) FAIL(c, SSM_E_INVAL, "bad arguments");
    int r = sgbm_check_params(c, params, w, h); if (r) return r;
    r = stereo_init(c, w, h, c->stereo && c->stereo->w == w && c->stereo->h == h ? c->stereo->maxc : 1000); if (r) return r;
    if ((r = stereo_ensure_seq(c, 1)) || (r = stereo_ensure_sgbm(c, *params, 1))) return r;
    StereoState* q = c->stereo.get();
    const PairBlock P((size_t)w * h); const hipStream_t s = c->main.stream;
    const uint8_t* imgs[2] = { left, right }; bool repeated = false;
    for (int attempt = 0; ; attempt++) {
        r = stereo_stage_images(c, imgs, 2, w, h, stride); if (r) return r;
        prof_reset(c);                                            // ssm_get_stage_times then reports this call ("sgbm": all kernels of k_sgbm)
        prof_begin(c, s, "sgbm");
        HIPCHK(c, k_sgbm(q->in_stage, q->in_stage + P.image(1), w, h, 1, *params, q->sg_wsN[0], q->sg_wsN[0].bytes(), q->disp, stage, c->dev, c->main.sg, s, q->sg_fail, attempt ? 1 : c->sgbm_form_cfg, 1));
        prof_end(c, s);
        q->sg_pending.valid = false;                              // (the staged pair is this call's, not a sequence call's that sgbm_recover could repeat)
        if (da) HIPCHK(c, k_sgbm_depth(q->disp, w, h, 1, da->baseline, da->cu, da->cv, da->f, da->roix, da->roiy, da->roiz, da->scale, q->dminN[0], q->depth, s));
        if (da) HIPCHK(c, hipMemcpyAsync(c->h_pinned + P.depth, q->depth, P.plane, hipMemcpyDeviceToHost, s));
        if (disp) HIPCHK(c, hipMemcpyAsync(c->h_pinned + P.disp, q->disp, P.plane, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(c->h_pinned + P.fail, q->sg_fail, 4, hipMemcpyDeviceToHost, s));      // (the staged input images at the front of the pinned area are consumed)
        HIPCHK(c, hipStreamSynchronize(s));
        int32_t sf; memcpy(&sf, c->h_pinned + P.fail, 4);
        if (!sf) break;
        HIPCHK(c, hipMemset(q->sg_fail, 0, 4));
        if (attempt) FAIL(c, SSM_E_HIP, "SGBM: the time-out word is set after a form-1 run");
        c->sgbm_fallbacks++; repeated = true;
    }
    if (repeated) c->err = "note: the SGBM sweep of this pair timed out in a strip hand-off and was repeated with form 1 (results complete; " + std::to_string(c->sgbm_fallbacks) + " such repeats on this context so far)";
    if (da) memcpy(depth, c->h_pinned + P.depth, P.plane);
    if (disp) memcpy(disp, c->h_pinned + P.disp, P.plane);
    return SSM_OK;
}
extern "C" int ssm_sgbm(ssm_ctx* c, const uint8_t* left, const uint8_t* right, int w, int h, int stride, const ssm_sgbm_params* params, int stage, int16_t* disp)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (!disp) FAIL(c, SSM_E_INVAL, "null argument");
    c->err.clear();
    return sgbm_pair(c, left, right, w, h, stride, params, stage, nullptr, disp, nullptr);
}
extern "C" int ssm_stereo_depth(ssm_ctx* c, const uint8_t* left, const uint8_t* right, int w, int h, int stride, const ssm_sgbm_params* params,
                                double baseline, double cu, double cv, double f, double roix, double roiy, double roiz, double scale,
                                uint16_t* depth, int16_t* disp)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (!depth) FAIL(c, SSM_E_INVAL, "null argument");
    c->err.clear();
    const DepthArgs da = { baseline, cu, cv, f, roix, roiy, roiz, scale };
    return sgbm_pair(c, left, right, w, h, stride, params, 0, &da, disp, depth);
}
// the SGBM post stages alone (exact tests of the median and of the speckle union-find on constructed maps): n stacked maps through k_sgbm_post
extern "C" int ssm_debug_sgbm_post(ssm_ctx* c, const int16_t* disp, int w, int h, int n, int op, int new_val, int max_size, int max_diff, int16_t* out)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (!disp || !out || w < 1 || h < 1 || n < 1 || op < 1 || op > 3 || max_diff < 0 || new_val < -32768 || new_val > 32767) FAIL(c, SSM_E_INVAL, "bad arguments");
    if (h > 65535 || n > 65535 || (long long)w * h >= (1ll << 30)) FAIL(c, SSM_E_INVAL, "map too large");
    const size_t np = (size_t)w * h * n;
    Carve k; const size_t o_in = k.take<int16_t>(np), o_out = k.take<int16_t>(np), o_parent = k.take<int>(np), o_count = k.take<int>(np);
    int r = ensure_scratch(c, k.end()); if (r) return r;
    uint8_t* p = (uint8_t*)c->d_scratch;
    int16_t* d_in = (int16_t*)(p + o_in); int16_t* d_out = (int16_t*)(p + o_out); int* parent = (int*)(p + o_parent); int* count = (int*)(p + o_count);
    HIPCHK(c, hipMemcpyAsync(d_in, disp, np * 2, hipMemcpyHostToDevice, c->main.stream));
    if (!(op & 1)) HIPCHK(c, hipMemcpyAsync(d_out, d_in, np * 2, hipMemcpyDeviceToDevice, c->main.stream));
    HIPCHK(c, k_sgbm_post(d_in, d_out, w, h, n, op, new_val, max_size, max_diff, parent, count, c->main.stream));
    HIPCHK(c, hipMemcpyAsync(out, d_out, np * 2, hipMemcpyDeviceToHost, c->main.stream));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    return SSM_OK;
}

// ---------------------------------------------------------------- VisualOdometryStereo::estimateMotion
extern "C" int ssm_vo_estimate(ssm_ctx* c, const ssm_pmatch* matches, int n, const ssm_vo_params* params, const int32_t* samples, int iters,
                               double tr[6], int32_t* inliers, int cap, int* n_inliers, int* success)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (n < 0 || iters < 0 || !params || !tr || !n_inliers || !success || (n && !matches) || (iters && !samples)) FAIL(c, SSM_E_INVAL, "bad arguments");
    for (int k = 0; k < 6; k++) tr[k] = 0.0;
    *n_inliers = 0; *success = 0;
    if (n < 6) return SSM_OK;                                 // estimateMotion returns an empty vector (vo_stereo.cpp:61-63)
    for (int k = 0; k < 3 * iters; k++) if (samples[k] < 0 || samples[k] >= n) FAIL(c, SSM_E_INVAL, "sample index out of range");
    Carve k; const size_t o_m = k.take<ssm_pmatch>(n), o_s = k.take<uint8_t>((size_t)iters * 12 + 16), o_tr = k.take<uint8_t>((size_t)iters * 48 + 48), o_cnt = k.take<uint8_t>((size_t)iters * 4 + 16),
                 o_out = k.take<uint8_t>(256), o_inl = k.take<int32_t>(n), o_res = k.take<uint8_t>(256);
    int r = ensure_scratch(c, k.off); if (r) return r;         // (the last region is the 256 bytes of o_res)
    uint8_t* p = (uint8_t*)c->d_scratch; hipStream_t s = c->main.stream;
    HIPCHK(c, hipMemcpyAsync(p + o_m, matches, (size_t)n * sizeof(ssm_pmatch), hipMemcpyHostToDevice, s));
    if (iters) HIPCHK(c, hipMemcpyAsync(p + o_s, samples, (size_t)iters * 12, hipMemcpyHostToDevice, s));
    prof_reset(c);
    prof_begin(c, s, "vo");
    HIPCHK(c, k_vo_estimate((const ssm_pmatch*)(p + o_m), n, *params, (const int32_t*)(p + o_s), iters, (double*)(p + o_tr), (int32_t*)(p + o_cnt),
                            (double*)(p + o_out), (int32_t*)(p + o_inl), (int32_t*)(p + o_res), s));
    prof_end(c, s);
    int32_t res[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(tr, p + o_out, 48, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(res, p + o_res, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    *n_inliers = res[0]; *success = res[1];
    if (inliers && res[0] > 0) {
        if (res[0] > cap) FAIL(c, SSM_E_CAPACITY, "inlier buffer too small (need " + std::to_string(res[0]) + ")");
        HIPCHK(c, hipMemcpy(inliers, p + o_inl, (size_t)res[0] * 4, hipMemcpyDeviceToHost));
    }
    return SSM_OK;
}

// PnPSolver::solvePnP (reference src/pnp.cpp:5-118) for one correspondence list: the solve that the pose chain of kernels_pnp.hip runs per frame.
// Round 6: a cluster of eight blocks per call, like the chain's (every block evaluates an eighth of the lanes' edges in a pass and the blocks trade the partial sums:
// same bits as one block, the per-frame Tracker's largest call 0.53 -> ~0.35 ms); one block after a cluster timed out once (the blocks need eight CUs at the same
// time) or with SSM_PNP_BLOCKS=1.
static int pnp_solve_impl(ssm_ctx* c, const float* img, const float* obj, int n, const double cam[4], int min_inliers, double T[16], uint8_t* inliers, int* n_inliers, int* success, int G)
{
    // ONE upload ([img | obj | header: T in, T out, time-out word, inlier count] staged in pinned memory) and ONE download ([T out .. count | the inlier flags]): the
    // call was three uploads, a fill of the exchange ring and four downloads (0.09 ms of its 0.42).  The cluster's ring lives in the context and is zeroed when its
    // pass numbers wrap, not per call.
    enum : size_t { H_TOUT = 128, H_XFAIL = 256, H_COUNT = 264, HDR = 288 };      // the header: T in 128 | T out 128 | xfail 4, pad 4 | count 4, pad 4 | pad 16
    const size_t ne = (size_t)(n > 0 ? n : 1), slice = up256(ne);
    Carve k; const size_t o_img = k.take<float>(2 * ne, 8), o_obj = k.take<float>(3 * ne, 8), o_hdr = k.take<uint8_t>(HDR, 16), o_inl = k.take<uint8_t>(G * slice, 1), o_dec = k.take<uint8_t>(G * slice, 1),
                 o_le = k.take<uint8_t>(G * slice * k_pnp_edge_bytes()), o_err = k.take<double2>(G * slice);
    const size_t up = o_hdr + HDR, down = HDR - H_TOUT + (size_t)n;            // download: [T out | xfail | count | pad][inl slice 0: n bytes]
    Carve hk; const size_t h_up = hk.take<uint8_t>(up), h_down = hk.take<uint8_t>(down);
    int r = ensure_scratch(c, k.off); if (r) return r;         // (slice is a multiple of 256, so the last region, G * slice * 16 bytes, ends on one)
    r = ensure_pinned(c, hk.end()); if (r) return r;
    if (G > 1) {
        if (!c->d_pnp_xchg) { if (c->d_pnp_xchg.alloc_bytes(c, k_pnp_xchg_bytes())) return SSM_E_HIP; c->pnp_epoch = 0; }
        if (c->pnp_epoch == 0) HIPCHK(c, hipMemsetAsync(c->d_pnp_xchg, 0, k_pnp_xchg_bytes(), c->main.stream));
    }
    uint8_t* p = (uint8_t*)c->d_scratch; hipStream_t s = c->main.stream;
    uint8_t* hu = c->h_pinned + h_up; uint8_t* hd = c->h_pinned + h_down;
    if (n) { memcpy(hu + o_img, img, (size_t)n * 8); memcpy(hu + o_obj, obj, (size_t)n * 12); }
    memset(hu + o_hdr, 0, HDR); memcpy(hu + o_hdr, T, 128);
    { const char* tv = getenv("SSM_PNP_TEST_TIMEOUT"); if (G > 1 && tv && atoi(tv) != 0) { const unsigned one = 1; memcpy(hu + o_hdr + H_XFAIL, &one, 4); } }      // tests: the time-out word set from the start -> the one-block retry
    HIPCHK(c, hipMemcpyAsync(p, hu, up, hipMemcpyHostToDevice, s));
    PnpSolveArgs a; a.img = (const float*)(p + o_img); a.obj = (const float*)(p + o_obj); a.n = n;
    a.cam.fx = cam[0]; a.cam.fy = cam[1]; a.cam.cx = cam[2]; a.cam.cy = cam[3];
    a.T = (double*)(p + o_hdr); a.inl = p + o_inl; a.dec = p + o_dec; a.ledges = (LEdge*)(p + o_le); a.err = (double2*)(p + o_err); a.n_inliers = (int32_t*)(p + o_hdr + H_COUNT); a.edges_in_lds = 0;
    a.blocks = G; a.slice = slice; a.xchg = c->d_pnp_xchg; a.xfail = reinterpret_cast<unsigned*>(p + o_hdr + H_XFAIL);
    a.seq_base = (unsigned)c->pnp_epoch << 20;                  // a solve makes a few thousand passes at most; the ring is zeroed again when the epoch wraps
    if (G > 1) c->pnp_epoch = (c->pnp_epoch + 1) & 4095;
    prof_reset(c);
    prof_begin(c, s, "pnp");
    HIPCHK(c, k_pnp_solve(a, s));
    prof_end(c, s);
    HIPCHK(c, hipMemcpyAsync(hd, p + o_hdr + H_TOUT, down, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    unsigned failed = 0; int32_t m = 0;
    memcpy(&failed, hd + H_XFAIL - H_TOUT, 4); memcpy(&m, hd + H_COUNT - H_TOUT, 4);
    if (G > 1 && failed) { c->pnp_epoch = 0; return 1; }        // an exchange of the cluster timed out: nothing of this attempt is used (and the ring starts clean next time)
    memcpy(T, hd, 128);
    if (inliers && n) memcpy(inliers, hd + HDR - H_TOUT, (size_t)n);
    *n_inliers = m;
    if (success) *success = n > min_inliers;                   // pnp.cpp:115 tests the flag vector's LENGTH (quirk 14)
    return SSM_OK;
}
extern "C" int ssm_pnp_lds_edge_capacity(void) { return (int)k_pnp_lds_edge_capacity(); }
static int pnp_env_blocks() { static const int b = [] { const char* e = getenv("SSM_PNP_BLOCKS"); return e ? atoi(e) : 8; }(); return b; }
// the blocks the context's next ssm_pnp_solve starts with (tests: which form a comparison ran in)
extern "C" int ssm_debug_pnp_solve_blocks(ssm_ctx* c)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    return pnp_env_blocks() == 8 && !c->pnp_solve_one_block ? 8 : 1;
}
extern "C" int ssm_pnp_solve(ssm_ctx* c, const float* img, const float* obj, int n, const double cam[4], int min_inliers, double T[16],
                             uint8_t* inliers, int* n_inliers, int* success)
{
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (n < 0 || !cam || !T || !n_inliers || (n && (!img || !obj))) FAIL(c, SSM_E_INVAL, "bad arguments");
    if (n > 65535) FAIL(c, SSM_E_CAPACITY, "at most 65535 correspondences");
    if (pnp_env_blocks() == 8 && !c->pnp_solve_one_block) {
        const int r = pnp_solve_impl(c, img, obj, n, cam, min_inliers, T, inliers, n_inliers, success, 8);
        if (r <= 0) return r;
        c->pnp_solve_one_block = true;                          // (T is untouched: the retry starts from the caller's initial value)
    }
    return pnp_solve_impl(c, img, obj, n, cam, min_inliers, T, inliers, n_inliers, success, 1);
}
