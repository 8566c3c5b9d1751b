// ssm_track_host.cpp -- ssm_tracker_*: rgbd_tutor::Tracker::updateFrame (reference src/track.cpp:8-36, 140-212) for all frames of an ssm_seq_process call: the tracker's
// host state and its per-frame state machine.  The pose chain is serial by nature (frame f's initial value and its reference poses are frame f-1's results); the PnP
// arithmetic is include/ssm/pnp_core.h, the code the per-frame host class (include/ssm/pnp.h) runs, so both give the same bits.  Plain C++ (ssm_host.h): a call's outputs come
// to the host through the public C ABI (ssm_memcpy_d2h; ssm_match for the on-demand pairs), the regular frames run behind ssm_track.hip's hooks -- host/test_track.cpp supplies both.
#include "ssm_host.h"
#define TFAIL(t, code, msg) do { (t)->err = (msg); return (code); } while (0)
#define TCHK(t, expr) do { int r__ = (expr); if (r__ != SSM_OK) { (t)->err = std::string(#expr) + ": " + ssm_last_error((t)->ctx); return r__; } } while (0)
#define TRY(expr) do { const int r__ = (expr); if (r__ != SSM_OK) return r__; } while (0)
static void iso_identity(double* T) { for (int k = 0; k < 16; k++) T[k] = (k % 5 == 0) ? 1.0 : 0.0; }

extern "C" void ssm_tracker_params_default(ssm_tracker_params* p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p)); p->max_lost_frame = 10; p->ref_frames = 5; p->pnp_min_inliers = 10; p->use_device = 0;
    iso_identity(p->first_pose);
}
extern "C" int ssm_tracker_create(ssm_ctx* ctx, const ssm_tracker_params* p, ssm_tracker** out)
{
    if (!ctx || !p || !out) return SSM_E_INVAL;
    *out = nullptr;
    if (p->ref_frames < 1 || p->ref_frames > SSM_TRACK_MAXREF || p->max_lost_frame < 0) return SSM_E_INVAL;
    std::unique_ptr<ssm_tracker> t(new ssm_tracker()); t->ctx = ctx; t->prm = *p;
    TRY(track_dev_attach(t.get()));
    ssm_tracker_reset(t.get()); *out = t.release();
    return SSM_OK;
}
extern "C" void ssm_tracker_destroy(ssm_tracker* t) { if (!t) return; track_dev_release(t); delete t; }
extern "C" const char* ssm_tracker_last_error(const ssm_tracker* t) { return t ? t->err.c_str() : "null tracker"; }
extern "C" int ssm_tracker_reset(ssm_tracker* t)
{
    if (!t) return SSM_E_INVAL;
    t->state = 0; t->cnt_lost = 0; t->refs.clear(); t->next_gidx = 0;
    iso_identity(t->speed); iso_identity(t->last_pose);
    return SSM_OK;
}
extern "C" int ssm_tracker_stats(const ssm_tracker* t, int64_t* device_frames, int64_t* host_frames)
{
    if (!t) return SSM_E_INVAL;
    if (device_frames) *device_frames = t->device_frames;
    if (host_frames) *host_frames = t->host_frames;
    return SSM_OK;
}
extern "C" int ssm_tracker_work(const ssm_tracker* t, int64_t work[4]) { if (!t || !work) return SSM_E_INVAL; for (int k = 0; k < 4; k++) work[k] = t->work[k]; return SSM_OK; }
// ---- the call's outputs on the host: counts always; features and match tables in bulk (host chain) or per frame when the host path needs one (device chain: need_features / need_matches)
static int begin_call(ssm_tracker* t, const ssm_seq_out_dev* seq, int n)
{
    const int cap = seq->cap, R = seq->R;
    t->nkp.resize(n); t->nmatch.resize((size_t)n * R); t->kps.resize((size_t)n * cap); t->pos3d.resize((size_t)n * cap * 3); t->desc.resize((size_t)n * cap * 32);
    t->matches.resize((size_t)n * R * cap); t->have.assign(n, 0);
    TCHK(t, ssm_sync(t->ctx));
    TCHK(t, ssm_memcpy_d2h(t->ctx, t->nkp.data(), seq->nkp, (size_t)n * 4));
    TCHK(t, ssm_memcpy_d2h(t->ctx, t->nmatch.data(), seq->nmatch, (size_t)n * R * 4));
    if (!t->prm.use_device) {
        TCHK(t, ssm_memcpy_d2h(t->ctx, t->kps.data(), seq->kps, (size_t)n * cap * sizeof(ssm_keypoint)));
        TCHK(t, ssm_memcpy_d2h(t->ctx, t->pos3d.data(), seq->pos3d, (size_t)n * cap * 12));
        TCHK(t, ssm_memcpy_d2h(t->ctx, t->desc.data(), seq->desc, (size_t)n * cap * 32));
        TCHK(t, ssm_memcpy_d2h(t->ctx, t->matches.data(), seq->matches, (size_t)n * R * cap * sizeof(ssm_dmatch)));
        t->have.assign(n, 3);
    }
    const size_t maxcorr = (size_t)R * cap;           // the PnP scratch
    t->img.resize(2 * maxcorr + 2); t->obj.resize(3 * maxcorr + 3); t->inl.resize(maxcorr + 1); t->edges.resize(maxcorr + 1); t->tmp_matches.resize(cap);
    return SSM_OK;
}
static int need_features(ssm_tracker* t, const ssm_seq_out_dev* seq, int f)
{
    if (t->have[f] & 1) return SSM_OK;
    const size_t k = (size_t)(t->nkp[f] > 0 ? t->nkp[f] : 0), at = (size_t)f * seq->cap;
    if (k) {
        TCHK(t, ssm_memcpy_d2h(t->ctx, t->kps.data() + at, seq->kps + at, k * sizeof(ssm_keypoint)));
        TCHK(t, ssm_memcpy_d2h(t->ctx, t->pos3d.data() + at * 3, seq->pos3d + at * 3, k * 12));
        TCHK(t, ssm_memcpy_d2h(t->ctx, t->desc.data() + at * 32, seq->desc + at * 32, k * 32));
    }
    t->have[f] |= 1; return SSM_OK;
}
static int need_matches(ssm_tracker* t, const ssm_seq_out_dev* seq, int f)
{
    const size_t rows = (size_t)seq->R * seq->cap;
    if (!(t->have[f] & 2)) TCHK(t, ssm_memcpy_d2h(t->ctx, t->matches.data() + f * rows, seq->matches + f * rows, rows * sizeof(ssm_dmatch)));
    t->have[f] |= 2; return SSM_OK;
}
// ---- the state machine
// refFrames.push_back(currentFrame); while (size > refFramesSize) pop_front() -- the one place a deque member is made from a call's frame
static int push_ref(ssm_tracker* t, const ssm_seq_out_dev* seq, int f, const double* pose)
{
    TRY(need_features(t, seq, f));
    TrackRef r; r.gidx = t->next_gidx + f; r.nkp = t->nkp[f]; memcpy(r.pose, pose, sizeof(r.pose));
    const size_t at = (size_t)f * seq->cap;
    r.pos3d.assign(t->pos3d.begin() + at * 3, t->pos3d.begin() + at * 3 + (size_t)r.nkp * 3);
    r.desc.assign(t->desc.begin() + at * 32, t->desc.begin() + at * 32 + (size_t)r.nkp * 32);
    t->refs.push_back(std::move(r));
    while ((int)t->refs.size() > t->prm.ref_frames) t->refs.pop_front();
    return SSM_OK;
}
// the deque is REGULAR at frame f when it is the run of frames directly in front of it: every member then has its precomputed match-table slot
bool track_regular(const ssm_tracker* t, int f)
{
    if (t->state != 1 || t->refs.empty()) return false;
    const int64_t G = t->next_gidx + f; const int k = (int)t->refs.size(), R = t->prm.ref_frames;
    for (int r = 0; r < k; r++) { if (t->refs[r].gidx != G - k + r) return false; if (t->nmatch[(size_t)f * R + (R - (k - r))] < 0 && t->nkp[f] >= 2) return false; }
    return true;
}
// the correspondences of frame f with every member of the deque, in deque order then match order (track.cpp:150-163) -> t->img, t->obj, *nc_out
static int gather(ssm_tracker* t, const ssm_seq_out_dev* seq, int f, int* nc_out)
{
    const int cap = seq->cap, R = seq->R; const int64_t G = t->next_gidx + f; int nc = 0;
    for (const TrackRef& ref : t->refs) {
        // orb->match(pFrame, currentFrame): the precomputed table when pFrame is one of the R frames in front of the current one
        const ssm_dmatch* m = nullptr; int nm = 0;
        const int64_t back = G - ref.gidx;           // 1 .. R: slot R - back
        if (back >= 1 && back <= R && t->nmatch[(size_t)f * R + (R - back)] >= 0) {
            TRY(need_matches(t, seq, f));
            nm = t->nmatch[(size_t)f * R + (R - back)]; m = t->matches.data() + ((size_t)f * R + (R - back)) * cap;
        } else if (ref.nkp >= 1 && t->nkp[f] >= 2) {  // an older reference frame (the deque after tracking failures): match the pair now
            TCHK(t, ssm_match(t->ctx, ref.desc.data(), ref.nkp, t->desc.data() + (size_t)f * cap * 32, t->nkp[f], t->ratio, t->tmp_matches.data(), cap, &nm));
            m = t->tmp_matches.data();
        }
        double inv[16]; ssm_pnp::iso_inverse(ref.pose, inv);
        for (int k = 0; k < nm; k++) {
            const float* p = ref.pos3d.data() + (size_t)m[k].queryIdx * 3;
            if (p[0] == 0.f && p[1] == 0.f && p[2] == 0.f) continue;
            double v[3]; ssm_pnp::iso_apply(inv, (double)p[0], (double)p[1], (double)p[2], v);
            t->obj[3 * nc] = (float)v[0]; t->obj[3 * nc + 1] = (float)v[1]; t->obj[3 * nc + 2] = (float)v[2];
            const ssm_keypoint& kp = t->kps[(size_t)f * cap + m[k].trainIdx];
            t->img[2 * nc] = kp.x; t->img[2 * nc + 1] = kp.y;
            nc++;
        }
    }
    *nc_out = nc; return SSM_OK;
}
// one frame on the host (the general case: first frame, lostRecover, a deque that reaches behind the match-table window)
int track_frame_host(ssm_tracker* t, const ssm_seq_out_dev* seq, int f, double* T_frame, ssm_track_info* info)
{
    info->state = 1; info->tracked = 0; info->n_matches = -1; info->n_inliers = 0; t->host_frames++;
    if (t->state == 0) {                                 // initFirstFrame (track.cpp:30-36)
        memcpy(T_frame, t->prm.first_pose, 128);                    // the frame keeps the T_f_w it arrived with; lastPose is not touched (nor by lostRecover)
        TRY(push_ref(t, seq, f, T_frame));
        iso_identity(t->speed);
        t->state = 1; info->tracked = 1;
    } else if (t->state == 2) {                          // lostRecover (track.cpp:202-212)
        memcpy(T_frame, t->refs.back().pose, 128);
        t->refs.clear();
        TRY(push_ref(t, seq, f, T_frame));
        t->state = 1; t->cnt_lost = 0; info->tracked = 1;
    } else {                                             // trackRefFrame (track.cpp:140-200)
        TRY(need_features(t, seq, f));
        ssm_pnp::iso_mul(t->speed, t->refs.back().pose, T_frame);          // currentFrame->setTransform(speed * refFrames.back()->getTransform())
        int nc = 0; TRY(gather(t, seq, f, &nc));
        info->n_matches = nc;
        bool ok = nc >= 15; double T[16];
        if (ok) {
            ssm_pnp::iso_mul(t->speed, t->last_pose, T);                    // T = speed * lastPose
            ssm_pnp::Camera cam; cam.fx = t->cam.fx; cam.fy = t->cam.fy; cam.cx = t->cam.cx; cam.cy = t->cam.cy; int success = 0;
            info->n_inliers = ssm_pnp::solve(t->img.data(), t->obj.data(), nc, cam, t->prm.pnp_min_inliers, T, t->inl.data(), t->edges.data(), &success);
            ok = info->n_inliers >= 15;
        }
        if (!ok) { t->cnt_lost++; if (t->cnt_lost > t->prm.max_lost_frame) t->state = 2; }
        else {
            memcpy(T_frame, T, 128); t->cnt_lost = 0;
            double linv[16]; ssm_pnp::iso_inverse(t->last_pose, linv);
            ssm_pnp::iso_mul(T, linv, t->speed);                            // speed = T * lastPose.inverse()
            memcpy(t->last_pose, T, 128);
            TRY(push_ref(t, seq, f, T));
            info->tracked = 1;
        }
    }
    info->state = t->state; return SSM_OK;
}
// ---- around a run of regular frames on the device
// the chain's state block before a run: speed, lastPose, cntLost and the deque with indices relative to the call (n: "walked every frame")
static void fill_block(const ssm_tracker* t, int n, PnpState* hs)
{
    memset(hs, 0, sizeof(*hs)); memcpy(hs->speed, t->speed, 128); memcpy(hs->last_pose, t->last_pose, 128);
    hs->nref = (int)t->refs.size(); hs->cnt_lost = t->cnt_lost; hs->stopped_at = n;
    for (int r = 0; r < hs->nref; r++) { hs->ref_idx[r] = (int)(t->refs[r].gidx - t->next_gidx); memcpy(hs->ref_pose[r], t->refs[r].pose, 128); }
}
// the host copy of the state after frames [f, hs.stopped_at) ran on the device: the deque in the device's order -- survivors are moved, the features of new members come down now
static int adopt_block(ssm_tracker* t, const ssm_seq_out_dev* seq, int f, const PnpState& hs, int last_state)
{
    memcpy(t->speed, hs.speed, 128); memcpy(t->last_pose, hs.last_pose, 128); t->cnt_lost = hs.cnt_lost; t->state = last_state;
    std::deque<TrackRef> old; old.swap(t->refs);
    for (int r = 0; r < hs.nref; r++) {
        const int64_t g = t->next_gidx + hs.ref_idx[r]; bool found = false;
        for (TrackRef& o : old) if (o.gidx == g) { t->refs.push_back(std::move(o)); found = true; break; }
        if (!found) TRY(push_ref(t, seq, hs.ref_idx[r], hs.ref_pose[r]));
    }
    t->device_frames += hs.stopped_at - f; for (int k = 0; k < 4; k++) t->work[k] += hs.work[k];
    return SSM_OK;
}
extern "C" int ssm_tracker_run(ssm_tracker* t, const ssm_seq_out_dev* seq, int n, double* pose_out, ssm_track_info* info_out)
{
    if (!t) return SSM_E_INVAL;
    if (!seq || n < 0 || (n && !pose_out)) TFAIL(t, SSM_E_INVAL, "bad arguments");
    if (n == 0) return SSM_OK;
    if (seq->R != t->prm.ref_frames || seq->R > SSM_TRACK_MAXREF) TFAIL(t, SSM_E_INVAL, "the sequence was matched with another tracker_ref_frames");
    TRY(begin_call(t, seq, n));
    std::vector<ssm_track_info> inf;
    for (int f = 0; f < n;) {
        if (t->prm.use_device && track_regular(t, f)) {          // a run of frames on the device: state up, one launch, state and the run's poses down
            PnpState hs; fill_block(t, n, &hs);
            TRY(track_dev_run(t, seq, f, n, &hs, pose_out, inf));
            // the cluster's blocks did not meet within the spin bound (they need CUs at the same time: a device kept full by other work for seconds).  Nothing of the
            // tracker's host state has changed yet: the same range again with one block per chain -- same kernel arithmetic, same bits
            if (hs.stopped_at == -1) { t->blocks = 1; t->downgraded = true; continue; }
            if (info_out) memcpy(info_out + f, inf.data(), inf.size() * sizeof(ssm_track_info));
            TRY(adopt_block(t, seq, f, hs, inf.back().state));
            f = hs.stopped_at;
        } else {
            ssm_track_info info; TRY(track_frame_host(t, seq, f, pose_out + (size_t)f * 16, &info));
            if (info_out) info_out[f] = info;
            f++;
        }
    }
    t->next_gidx += n;
    // (a note, the call succeeded: ssm_tracker_last_error is how a downgrade of the device chain shows)
    t->err = t->downgraded ? "note: the pose chain's cluster of blocks timed out in an exchange; this tracker continues with one block per chain (same poses)" : "";
    return SSM_OK;
}
