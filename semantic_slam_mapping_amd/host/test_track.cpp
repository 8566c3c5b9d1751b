// test_track.cpp -- the bulk tracker's host state machine (csrc/ssm_track_host.cpp over csrc/ssm_host.h) as a stand-alone program: it links that one source and
// defines everything the source asks of its surroundings itself, over host arrays -- the public calls it downloads with (ssm_sync, ssm_memcpy_d2h: a memcpy), the
// on-demand matcher (ssm_match: the identity list, counted) and the three hooks of the device leg, with a host model of the chain kernel behind the run hook.  So it
// needs neither libssm_hip.so nor a GPU and runs as it is under the CPU sanitizers (make SAN=asan san).
//
// The "device" arrays follow the conventions of the sequence path (csrc/kernels_match.hip match_seq_kernel, include/ssm_hip.h ssm_seq_out_dev): frame f of a call
// has cap rows of keypoints / positions / descriptors, of which nkp[f] are filled; slot s of frame f holds the list of the pair (f - R + s -> f), query = the
// older frame, ascending queryIdx; its count is -1 when that reference frame does not exist or the current frame has fewer than 2 keypoints (a reference frame
// with 0 keypoints gives 0).  A call that continues a sequence sees the previous call's last R frames as references.
// The model of the chain (csrc/kernels_pnp.hip pnp_chain_kernel): from the state block it walks the frames [f_begin, f_end) while each tracks and stops after the
// first failing one, inclusive; that frame's pose is the prediction speed * refs.back(); its state is 2 when cnt_lost > max_lost; the deque shifts in place, with
// indices relative to the call; the positions of a member with a negative index come from row index + R of the history buffer, which keeps what earlier runs put there.
//
// The scene: 60 points on a plane at constant depth in front of a camera that translates a little per frame, keypoints = their projections, positions = the points
// in the camera's frame (two of them without depth here and there), 14 frames in two calls (8 + 6) with R = 3, cap = 64 and max_lost_frame = 1; frames 4, 9 and 10
// have no keypoints, so 4 fails (the deque then reaches behind the match-table window: on-demand matches), 9 fails, 10 fails and is LOST, 11 recovers.
#include "../csrc/ssm_host.h"
using namespace std;

static int failures = 0;
static void check(bool ok, const char* name) { printf("%s %s\n", ok ? "PASS" : "FAIL", name); if (!ok) failures++; }

enum { NF = 14, NP = 60, CAP = 64, R = 3, N1 = 8 };
static const int TRACKED[NF] = {1, 1, 1, 1, 0, 1, 1, 1, 1, 0, 0, 1, 1, 1};
static const ssm_camera CAM = {318.6, 255.3, 517.3, 516.5, 1000.0};
static bool empty_frame(int f) { return f == 4 || f == 9 || f == 10; }

// ---------------------------------------------------------------- the "device": the whole sequence, and one call's view of it
struct Scene { int32_t nkp[NF]; vector<ssm_keypoint> kps; vector<float> pos3d; vector<uint8_t> desc; };
static Scene S;
static void build_scene()
{
    S.kps.assign((size_t)NF * CAP, ssm_keypoint()); S.pos3d.assign((size_t)NF * CAP * 3, 0.f); S.desc.assign((size_t)NF * CAP * 32, 0);
    for (int f = 0; f < NF; f++) {
        S.nkp[f] = empty_frame(f) ? 0 : NP;
        for (int i = 0; i < S.nkp[f]; i++) {
            const double X = -1.0 + 2.0 * ((i * 37) % NP) / NP, Y = -0.8 + 1.6 * ((i * 11) % NP) / NP, Z = 2.0;          // the world = the first camera's frame
            const double x = X - 0.01 * f, y = Y - 0.005 * f;                                                             // the camera has moved by (0.01, 0.005, 0) f
            ssm_keypoint& k = S.kps[(size_t)f * CAP + i];
            k.x = (float)(CAM.fx * x / Z + CAM.cx); k.y = (float)(CAM.fy * y / Z + CAM.cy); k.size = 31.f; k.angle = 0.f; k.response = 1.f; k.octave = 0; k.class_id = -1;
            float* p = &S.pos3d[((size_t)f * CAP + i) * 3];
            if (!(i == 20 || (i == 7 && f == 2))) { p[0] = (float)x; p[1] = (float)y; p[2] = (float)Z; }                     // (0, 0, 0): no depth at that keypoint
            uint8_t* d = &S.desc[((size_t)f * CAP + i) * 32]; d[0] = (uint8_t)f; d[1] = (uint8_t)i;                          // the matcher below reads the frame from it
        }
    }
}
static int identity_list(int nq, int nt, ssm_dmatch* out)
{
    const int n = min(nq, nt);
    for (int k = 0; k < n; k++) { out[k].queryIdx = k; out[k].trainIdx = k; out[k].imgIdx = 0; out[k].distance = 0.f; }
    return n;
}
struct Call {               // frames [f0, f0 + n) as ssm_seq_process hands them out
    int f0, n; vector<ssm_dmatch> matches; vector<int32_t> nmatch; ssm_seq_out_dev out;
    Call(int f0_, int n_) : f0(f0_), n(n_), matches((size_t)n_ * R * CAP), nmatch((size_t)n_ * R)
    {
        for (int f = 0; f < n; f++) for (int s = 0; s < R; s++) {
            const int cur = f0 + f, ref = cur - R + s;
            nmatch[(size_t)f * R + s] = (ref < 0 || S.nkp[cur] < 2) ? -1 : identity_list(S.nkp[ref], S.nkp[cur], &matches[((size_t)f * R + s) * CAP]);
        }
        out.kps = &S.kps[(size_t)f0 * CAP]; out.desc = &S.desc[(size_t)f0 * CAP * 32]; out.pos3d = &S.pos3d[(size_t)f0 * CAP * 3]; out.nkp = &S.nkp[f0];
        out.matches = matches.data(); out.nmatch = nmatch.data(); out.npoints = nullptr; out.cap = CAP; out.R = R;
    }
};

// ---------------------------------------------------------------- what ssm_track_host.cpp asks of its surroundings
static vector<size_t> g_copies;                     // bytes of every download
static vector<pair<int, int>> g_pairs;              // (reference frame, current frame) of every on-demand match
static bool g_in_model = false;
extern "C" {
int ssm_sync(ssm_ctx*) { return SSM_OK; }
int ssm_memcpy_d2h(ssm_ctx*, void* dst, const void* src, size_t bytes) { g_copies.push_back(bytes); memcpy(dst, src, bytes); return SSM_OK; }
const char* ssm_last_error(const ssm_ctx*) { return ""; }
int ssm_match(ssm_ctx*, const uint8_t* q, int nq, const uint8_t* t, int nt, double, ssm_dmatch* out, int cap, int* n_out)
{
    if (g_in_model || nq < 1 || nt < 2 || min(nq, nt) > cap) return SSM_E_INVAL;          // the chain on the device never matches a pair
    g_pairs.push_back(make_pair((int)q[0], (int)t[0]));
    *n_out = identity_list(nq, nt, out);
    return SSM_OK;
}
}
static int g_blocks = 1, g_timeouts = 0;            // what the attach hook chooses; how many runs still report the cluster's time-out
int track_dev_attach(ssm_tracker* t) { t->cam = CAM; t->ratio = 0.8; t->blocks = g_blocks; return SSM_OK; }
void track_dev_release(ssm_tracker*) {}

static bool bytes_equal(const void* a, const void* b, size_t n) { return memcmp(a, b, n) == 0; }
// every member of the deque has the features of its frame on the host, with that frame's count
static bool deque_complete(const ssm_tracker* t)
{
    for (const TrackRef& r : t->refs) {
        if (r.gidx < 0 || r.gidx >= NF || r.nkp != S.nkp[r.gidx] || r.pos3d.size() != (size_t)r.nkp * 3 || r.desc.size() != (size_t)r.nkp * 32) return false;
        if (r.nkp && (!bytes_equal(r.pos3d.data(), &S.pos3d[(size_t)r.gidx * CAP * 3], r.pos3d.size() * 4) || !bytes_equal(r.desc.data(), &S.desc[(size_t)r.gidx * CAP * 32], r.desc.size()))) return false;
    }
    return true;
}
struct RunRecord { int f, n, blocks; bool deque_ok, aligned; vector<pair<int, int>> rows; PnpState in; int state, cnt_lost; vector<int64_t> gidx; long dev_frames, host_frames; };
static vector<RunRecord> g_runs;
static vector<float> g_hist((size_t)R * CAP * 3, 0.f);          // the device's history rows: they keep what earlier runs uploaded
int track_dev_run(ssm_tracker* t, const ssm_seq_out_dev* seq, int f, int n, PnpState* hs, double* pose_out, vector<ssm_track_info>& info)
{
    RunRecord rec; rec.f = f; rec.n = n; rec.blocks = t->blocks; rec.deque_ok = deque_complete(t); rec.in = *hs;
    rec.state = t->state; rec.cnt_lost = t->cnt_lost; rec.dev_frames = t->device_frames; rec.host_frames = t->host_frames;
    for (const TrackRef& r : t->refs) rec.gidx.push_back(r.gidx);
    rec.aligned = hs->nref == (int)t->refs.size();
    // the history rows go up: the members with a negative index, from t->refs in the block's order
    for (int r = 0; r < hs->nref && rec.aligned; r++) {
        const int idx = hs->ref_idx[r]; const TrackRef& ref = t->refs[r];
        rec.aligned = ref.gidx - t->next_gidx == idx && idx >= -R && idx < f && bytes_equal(ref.pose, hs->ref_pose[r], 128);
        if (idx < 0 && ref.nkp > 0 && rec.aligned) { memcpy(&g_hist[(size_t)(idx + R) * CAP * 3], ref.pos3d.data(), (size_t)ref.nkp * 12); rec.rows.push_back(make_pair(idx + R, (int)ref.gidx)); }
    }
    g_runs.push_back(rec);
    if (!rec.aligned) { t->err = "test: the block does not describe the deque"; return SSM_E_INVAL; }
    if (g_timeouts > 0 && t->blocks > 1) { g_timeouts--; hs->stopped_at = -1; return SSM_OK; }
    // the chain: a tracker of the model's own, made from the BLOCK and the call's device arrays alone, stepped with the host frame function
    ssm_tracker m; m.ctx = t->ctx; m.prm = t->prm; m.cam = t->cam; m.ratio = t->ratio; m.state = 1; m.cnt_lost = hs->cnt_lost;
    memcpy(m.speed, hs->speed, 128); memcpy(m.last_pose, hs->last_pose, 128);
    for (int r = 0; r < hs->nref; r++) {
        const int idx = hs->ref_idx[r];
        const float* rows = idx >= 0 ? seq->pos3d + (size_t)idx * CAP * 3 : &g_hist[(size_t)(idx + R) * CAP * 3];
        TrackRef ref; ref.gidx = idx; ref.nkp = CAP; memcpy(ref.pose, hs->ref_pose[r], 128); ref.pos3d.assign(rows, rows + CAP * 3); ref.desc.assign(CAP * 32, 0);
        m.refs.push_back(ref);
    }
    m.nkp.assign(seq->nkp, seq->nkp + n); m.nmatch.assign(seq->nmatch, seq->nmatch + (size_t)n * R); m.kps.assign(seq->kps, seq->kps + (size_t)n * CAP);
    m.pos3d.assign(seq->pos3d, seq->pos3d + (size_t)n * CAP * 3); m.desc.assign(seq->desc, seq->desc + (size_t)n * CAP * 32);
    m.matches.assign(seq->matches, seq->matches + (size_t)n * R * CAP); m.have.assign(n, 3);
    m.img.resize(2 * R * CAP + 2); m.obj.resize(3 * R * CAP + 3); m.inl.resize(R * CAP + 1); m.edges.resize(R * CAP + 1); m.tmp_matches.resize(CAP);
    vector<double> dpose((size_t)n * 16); vector<ssm_track_info> dinfo(n);
    int stop = n;
    g_in_model = true;
    for (int g = f; g < n; g++) {
        const int rc = track_frame_host(&m, seq, g, &dpose[(size_t)g * 16], &dinfo[g]);
        if (rc != SSM_OK) { g_in_model = false; t->err = "test: the model of the chain failed"; return rc; }
        if (!dinfo[g].tracked) { stop = g + 1; break; }
    }
    g_in_model = false;
    memcpy(hs->speed, m.speed, 128); memcpy(hs->last_pose, m.last_pose, 128); hs->cnt_lost = m.cnt_lost; hs->nref = (int)m.refs.size(); hs->stopped_at = stop;
    for (int r = 0; r < hs->nref; r++) { hs->ref_idx[r] = (int)m.refs[r].gidx; memcpy(hs->ref_pose[r], m.refs[r].pose, 128); }
    hs->work[0] = stop - f; hs->work[1] = 2 * (stop - f); hs->work[2] = hs->work[3] = 1;
    memcpy(pose_out + (size_t)f * 16, &dpose[(size_t)f * 16], (size_t)(stop - f) * 128);
    info.assign(dinfo.begin() + f, dinfo.begin() + stop);
    return SSM_OK;
}

// ---------------------------------------------------------------- the independent walk: a full deque, lists gathered directly, ssm_pnp::solve
struct Result { double pose[NF][16]; ssm_track_info info[NF]; };
static void reference_walk(Result& w)
{
    struct Ref { int f; double pose[16]; };
    int state = 0, cnt_lost = 0;
    double speed[16], last[16], eye[16];
    for (int k = 0; k < 16; k++) eye[k] = speed[k] = last[k] = (k % 5 == 0) ? 1.0 : 0.0;
    vector<Ref> refs;
    const ssm_pnp::Camera cam = {CAM.fx, CAM.fy, CAM.cx, CAM.cy};
    for (int f = 0; f < NF; f++) {
        double T[16]; int tracked = 0, nm = -1, ninl = 0;
        Ref me; me.f = f;
        if (state == 0) { memcpy(T, eye, 128); memcpy(speed, eye, 128); state = 1; tracked = 1; memcpy(me.pose, T, 128); refs.push_back(me); }
        else if (state == 2) { memcpy(T, refs.back().pose, 128); refs.clear(); state = 1; cnt_lost = 0; tracked = 1; memcpy(me.pose, T, 128); refs.push_back(me); }
        else {
            ssm_pnp::iso_mul(speed, refs.back().pose, T);
            vector<float> img, obj;
            for (const Ref& r : refs) {
                if (S.nkp[r.f] < 1 || S.nkp[f] < 2) continue;
                double inv[16]; ssm_pnp::iso_inverse(r.pose, inv);
                for (int q = 0; q < min(S.nkp[r.f], S.nkp[f]); q++) {
                    const float* p = &S.pos3d[((size_t)r.f * CAP + q) * 3];
                    if (p[0] == 0.f && p[1] == 0.f && p[2] == 0.f) continue;
                    double v[3]; ssm_pnp::iso_apply(inv, (double)p[0], (double)p[1], (double)p[2], v);
                    for (int c = 0; c < 3; c++) obj.push_back((float)v[c]);
                    img.push_back(S.kps[(size_t)f * CAP + q].x); img.push_back(S.kps[(size_t)f * CAP + q].y);
                }
            }
            nm = (int)img.size() / 2;
            bool ok = nm >= 15;
            double Ts[16];
            if (ok) {
                ssm_pnp::iso_mul(speed, last, Ts);
                vector<unsigned char> inl(nm + 1); vector<ssm_pnp::Edge> edges(nm + 1); int success = 0;
                ninl = ssm_pnp::solve(img.data(), obj.data(), nm, cam, 10, Ts, inl.data(), edges.data(), &success);
                ok = ninl >= 15;
            }
            if (!ok) { cnt_lost++; if (cnt_lost > 1) state = 2; }
            else {
                memcpy(T, Ts, 128); cnt_lost = 0; tracked = 1;
                double linv[16]; ssm_pnp::iso_inverse(last, linv); ssm_pnp::iso_mul(T, linv, speed); memcpy(last, T, 128);
                memcpy(me.pose, T, 128); refs.push_back(me);
                if ((int)refs.size() > R) refs.erase(refs.begin());
            }
        }
        memcpy(w.pose[f], T, 128);
        w.info[f].state = state; w.info[f].tracked = tracked; w.info[f].n_matches = nm; w.info[f].n_inliers = ninl;
    }
}

// ---------------------------------------------------------------- the tracker over the two calls
static int g_ctx_stand_in;
static ssm_ctx* ctx() { return reinterpret_cast<ssm_ctx*>(&g_ctx_stand_in); }
static ssm_tracker* make_tracker(int use_device, int blocks)
{
    ssm_tracker_params p; ssm_tracker_params_default(&p);
    p.max_lost_frame = 1; p.ref_frames = R; p.use_device = use_device;
    g_blocks = blocks;
    ssm_tracker* t = nullptr;
    return ssm_tracker_create(ctx(), &p, &t) == SSM_OK ? t : nullptr;
}
// both calls; false when one fails or leaves a deque member without its features
static bool run_sequence(ssm_tracker* t, Result& out, size_t* runs_before_second_call = nullptr)
{
    const Call a(0, N1), b(N1, NF - N1);
    memset(&out, 0, sizeof(out));
    if (ssm_tracker_run(t, &a.out, a.n, out.pose[0], out.info) != SSM_OK || !deque_complete(t)) return false;
    if (runs_before_second_call) *runs_before_second_call = g_runs.size();
    return ssm_tracker_run(t, &b.out, b.n, out.pose[N1], out.info + N1) == SSM_OK && deque_complete(t);
}
static bool same_results(const Result& a, const Result& b) { return bytes_equal(a.pose, b.pose, sizeof(a.pose)) && bytes_equal(a.info, b.info, sizeof(a.info)); }
static bool on_demand_pairs_as_expected()
{
    // frames 5, 6 and 7 each find one member behind the window (frame 4 did not join the deque); nothing before frame 5, nothing in the second call
    const vector<pair<int, int>> want = {{1, 5}, {2, 6}, {3, 7}};
    return g_pairs == want;
}

static void test_host_chain(const Result& walk, Result& host)
{
    g_copies.clear(); g_pairs.clear(); g_runs.clear();
    ssm_tracker* t = make_tracker(0, 1);
    check(t && run_sequence(t, host), "host chain: both calls succeed, every deque member complete");
    check(same_results(host, walk), "host chain: every pose and info row has the bytes of the independent walk");
    bool pattern = true; for (int f = 0; f < NF; f++) pattern = pattern && host.info[f].tracked == TRACKED[f];
    check(pattern && host.info[10].state == 2 && host.info[11].state == 1 && host.info[5].n_inliers > 50, "host chain: tracked 1 1 1 1 0 1 1 1 1 0 0 1 1 1, LOST at 10, recovered at 11");
    check(on_demand_pairs_as_expected(), "host chain: on-demand matches for the pairs 1->5, 2->6, 3->7 and no others");
    int64_t dev = -1, hst = -1; ssm_tracker_stats(t, &dev, &hst);
    check(dev == 0 && hst == NF && g_runs.empty() && string(ssm_tracker_last_error(t)).empty(), "host chain: 14 host frames, no device run, no note");
    // per call: the two count arrays, then the four bulk downloads
    const size_t n2 = NF - N1;
    const vector<size_t> want = {N1 * 4, N1 * R * 4, N1 * CAP * sizeof(ssm_keypoint), N1 * CAP * 12, N1 * CAP * 32, N1 * R * CAP * sizeof(ssm_dmatch),
                                 n2 * 4, n2 * R * 4, n2 * CAP * sizeof(ssm_keypoint), n2 * CAP * 12, n2 * CAP * 32, n2 * R * CAP * sizeof(ssm_dmatch)};
    check(g_copies == want, "host chain: six downloads per call, of the bulk sizes");
    ssm_tracker_destroy(t);
}
static void test_device_chain(const Result& host)
{
    g_copies.clear(); g_pairs.clear(); g_runs.clear(); fill(g_hist.begin(), g_hist.end(), 0.f);
    ssm_tracker* t = make_tracker(1, 1);
    Result dev; size_t first2 = 0;
    check(t && run_sequence(t, dev, &first2), "device chain: both calls succeed, every deque member complete");
    check(same_results(dev, host), "device chain: every pose and info row has the bytes of the host chain");
    int64_t nd = -1, nh = -1, work[4] = {0, 0, 0, 0}; ssm_tracker_stats(t, &nd, &nh); ssm_tracker_work(t, work);
    check(nd + nh == NF && nd >= 5, "device chain: device_frames + host_frames == 14, device_frames >= 5");
    check(work[0] == nd && work[1] == 2 * nd && work[2] == (int64_t)g_runs.size(), "device chain: the runs' work counters add up");
    bool ok = !g_runs.empty();
    for (const RunRecord& r : g_runs) ok = ok && r.deque_ok && r.aligned && r.state == 1;
    check(ok, "device chain: at every run the block describes the deque and every member has its features");
    // call 1: frames 1 .. 4 (4 fails); call 2: frames 8, 9 from the members 5, 6, 7 of the first call, then 12, 13 after the recovery
    const vector<pair<int, int>> rows567 = {{0, 5}, {1, 6}, {2, 7}};
    ok = g_runs.size() == 3 && first2 == 1 && g_runs[0].f == 1 && g_runs[0].in.nref == 1 && g_runs[0].rows.empty() && g_runs[1].f == 0 && g_runs[1].in.nref == 3 &&
         g_runs[1].in.ref_idx[0] == -3 && g_runs[1].in.ref_idx[1] == -2 && g_runs[1].in.ref_idx[2] == -1 && g_runs[1].in.cnt_lost == 0 && g_runs[1].rows == rows567 &&
         g_runs[2].f == 4 && g_runs[2].in.nref == 1 && g_runs[2].in.ref_idx[0] == 3 && g_runs[2].rows.empty();
    check(ok, "device chain: three runs; the second call's first one sends up the history rows of the members -3, -2, -1 and no others");
    check(on_demand_pairs_as_expected(), "device chain: the same on-demand matches as the host chain");
    bool small = g_copies.size() > 4;
    for (size_t i = 0; i < g_copies.size(); i++) {
        const size_t b = g_copies[i];
        small = small && (b == N1 * 4 || b == N1 * R * 4 || b == (NF - N1) * 4 || b == (NF - N1) * R * 4 || b == NP * sizeof(ssm_keypoint) || b == NP * 12 || b == NP * 32 || b == R * CAP * sizeof(ssm_dmatch));
    }
    check(small && string(ssm_tracker_last_error(t)).empty(), "device chain: counts, then per-frame fetches of k keypoints and single match tables only; no note");
    ssm_tracker_destroy(t);
}
static void test_retry(const Result& host)
{
    g_pairs.clear(); g_runs.clear(); fill(g_hist.begin(), g_hist.end(), 0.f);
    ssm_tracker* t = make_tracker(1, 8);
    g_timeouts = 1;
    Result dev;
    check(t && run_sequence(t, dev) && g_timeouts == 0, "retry: the calls succeed after one reported time-out");
    bool ok = g_runs.size() == 4;
    if (ok) {
        const RunRecord &a = g_runs[0], &b = g_runs[1];
        ok = a.blocks == 8 && b.blocks == 1 && a.f == b.f && a.n == b.n && bytes_equal(&a.in, &b.in, sizeof(PnpState)) && a.state == b.state && a.cnt_lost == b.cnt_lost &&
             a.gidx == b.gidx && a.dev_frames == b.dev_frames && a.host_frames == b.host_frames && g_runs[3].blocks == 1;
    }
    check(ok, "retry: the same range runs again from the same block with one block per chain; the host state is untouched in between");
    check(same_results(dev, host), "retry: the poses and info rows of the host chain");
    check(string(ssm_tracker_last_error(t)).find("one block per chain") != string::npos, "retry: the downgrade note in ssm_tracker_last_error");
    ssm_tracker_destroy(t);
}
static void test_argument_errors()
{
    ssm_tracker* t = make_tracker(0, 1);
    const Call a(0, N1); double pose[N1 * 16];
    check(t && ssm_tracker_run(t, nullptr, 3, pose, nullptr) == SSM_E_INVAL && string(ssm_tracker_last_error(t)) == "bad arguments", "arguments: a null seq");
    check(t && ssm_tracker_run(t, &a.out, -1, pose, nullptr) == SSM_E_INVAL && string(ssm_tracker_last_error(t)) == "bad arguments", "arguments: n < 0");
    check(t && ssm_tracker_run(t, &a.out, 3, nullptr, nullptr) == SSM_E_INVAL && string(ssm_tracker_last_error(t)) == "bad arguments", "arguments: frames without pose_out");
    ssm_seq_out_dev other = a.out; other.R = R + 1;
    check(t && ssm_tracker_run(t, &other, 3, pose, nullptr) == SSM_E_INVAL && string(ssm_tracker_last_error(t)) == "the sequence was matched with another tracker_ref_frames", "arguments: R different from the tracker's");
    check(t && ssm_tracker_run(t, &a.out, 0, nullptr, nullptr) == SSM_OK && ssm_tracker_run(nullptr, &a.out, 3, pose, nullptr) == SSM_E_INVAL && t->state == 0 && t->next_gidx == 0, "arguments: n == 0 is a call without effect; a null tracker");
    ssm_tracker_destroy(t);
    ssm_tracker_params p; ssm_tracker_params_default(&p);
    for (int rf : {0, -1, 65}) {
        p.ref_frames = rf; t = reinterpret_cast<ssm_tracker*>(&p);
        check(ssm_tracker_create(ctx(), &p, &t) == SSM_E_INVAL && t == nullptr, "arguments: ref_frames outside 1..64 at create");
    }
    p.ref_frames = 64; t = nullptr;
    check(ssm_tracker_create(ctx(), &p, &t) == SSM_OK && t != nullptr && ssm_tracker_create(nullptr, &p, &t) == SSM_E_INVAL, "arguments: ref_frames 64 is accepted; a null context is not");
    ssm_tracker_destroy(t);
    check(string(ssm_tracker_last_error(nullptr)) == "null tracker" && ssm_tracker_reset(nullptr) == SSM_E_INVAL && ssm_tracker_stats(nullptr, nullptr, nullptr) == SSM_E_INVAL, "arguments: null tracker in the small entry points");
}
// track_regular on states made by hand: a call of 6 frames that begins at global frame 10, R = 3, every frame with 60 keypoints and full tables unless said otherwise
static bool regular_case(int state, const vector<int64_t>& gidx, int f, int minus_one_slot = -1, int nkp_f = NP)
{
    ssm_tracker t; t.prm.ref_frames = R; t.state = state; t.next_gidx = 10;
    t.nkp.assign(6, NP); t.nmatch.assign(6 * R, NP);
    t.nkp[f] = nkp_f; if (minus_one_slot >= 0) t.nmatch[(size_t)f * R + minus_one_slot] = -1;
    for (int64_t g : gidx) { TrackRef r; r.gidx = g; r.nkp = NP; t.refs.push_back(r); }
    return track_regular(&t, f);
}
static void test_regular()
{
    check(regular_case(1, {11, 12, 13}, 4) && regular_case(1, {13}, 4) && regular_case(1, {12, 13}, 4), "regular: the one, two or three frames directly in front");
    check(regular_case(1, {8, 9, 10}, 1) && regular_case(1, {7, 8, 9}, 0), "regular: members of the previous call count like any other");
    check(!regular_case(0, {11, 12, 13}, 4) && !regular_case(2, {11, 12, 13}, 4), "regular: not while the state is NOT_READY or LOST");
    check(!regular_case(1, {}, 4), "regular: not with an empty deque");
    check(!regular_case(1, {11, 13}, 4) && !regular_case(1, {11, 12}, 4), "regular: not with a gap in the indices, inside the deque or in front of the frame");
    check(!regular_case(1, {10, 12, 13}, 4) && !regular_case(1, {9}, 4), "regular: not with a member older than R frames");
    check(!regular_case(1, {11, 12, 13}, 4, 1) && !regular_case(1, {13}, 4, 2) && !regular_case(1, {11, 12, 13}, 4, 0, 2), "regular: not when a member's slot is -1 and the frame has at least 2 keypoints");
    check(regular_case(1, {13}, 4, 0) && regular_case(1, {12, 13}, 4, 0), "regular: a -1 slot no member uses does not matter");
    check(regular_case(1, {11, 12, 13}, 4, 1, 1) && regular_case(1, {11, 12, 13}, 4, 2, 0), "regular: a -1 slot of a frame with fewer than 2 keypoints fails on the device like on the host");
}

int main()
{
    build_scene();
    static Result walk, host;
    reference_walk(walk);
    bool pattern = true; for (int f = 0; f < NF; f++) pattern = pattern && walk.info[f].tracked == TRACKED[f];
    check(pattern && walk.info[10].state == 2 && walk.info[11].state == 1, "the independent walk alone: tracked 1 1 1 1 0 1 1 1 1 0 0 1 1 1, LOST at 10, recovered at 11");
    test_host_chain(walk, host);
    test_device_chain(host);
    test_retry(host);
    test_argument_errors();
    test_regular();
    printf(failures ? "%d FAILED\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
