// exp_mapping -- the reference's product driver (experiment/exp_mapping.cpp:18-59) on the MI355X front end: build the
// ParameterReader, Tracker, FrameReader, PoseGraph and Mapper, then loop next() -> updateFrame() -> tryInsertKeyFrame(),
// finally shut the graph and the mapper down.  Differences: no cv::imshow; the frame source is selected by `dataset`
// (synthetic | raw | tum | kitti; the reference hard-codes its FrameReader type); with tum / kitti the poses come from the
// tracker (use_stream_pose defaults to 0 there); prints frames/s at the end.
//
// `exp_mapping <parameters> --batched` (or tracker_batched=1): the same loop with the pose chain in bulk -- frames are queued in chunks of tracker_chunk,
// BatchTracker runs ORB + the match tables for a whole chunk in batched launches and then the Tracker state machine + PnP over it (ssm_tracker_run:
// the poses of the per-frame Tracker, bit for bit), after which the chunk's frames go through tryInsertKeyFrame like in the per-frame loop.
//
// `exp_mapping <parameters> --loops` (or looper=1): every key-frame goes through Looper::add and Looper::getPossibleLoops (include/ssm/looper.h; the vocabulary is
// looper_vocab_file) right after tryInsertKeyFrame accepted it; with --batched the key-frames of a chunk are added in bulk from the chunk's device descriptors and
// queried in one call (BatchLooper).  The summary line then ends with `loop_candidates N loop_fnv H` (FNV-1a over frame id, candidate id and the score's bytes, in
// order: the same in both modes); loops_output=<file> gets one line per candidate.  Without the flag nothing of this runs and no output changes.
// `exp_mapping <parameters> --train-vocab FILE` (or looper_train_vocab=FILE): the ORB descriptors of every accepted key-frame are collected (with --batched they
// come down from the chunk's device tables) and after the sequence a vocabulary is trained from them (trainVocabulary in include/ssm/looper.h: looper_train_k /
// looper_train_L / looper_train_iters) and written to FILE, which a later run names as looper_vocab_file.  The summary line then ends with `vocab_nodes N
// vocab_words W vocab_fnv H` (FNV-1a over the exported arrays: the same in both modes).  The bulk stereo tracker has no descriptors: ignored there.
//
// `exp_mapping <parameters> --moving` (or uv_disparity=1; needs tracker_mode=stereo): the triangulate10D / UVDisparity block of Tracker::estimateVO (reference
// src/track.cpp:66-79; include/ssm/uvdisparity.hpp) runs after every successful stereo VO and fills the frame's moving_mask, roi_mask and ground_mask;
// with --batched one bulk call per chunk does it.  The summary line then carries `moving_pixels N moving_fnv H pitch_fnv P` (the 255-pixels, FNV-1a over the mask
// bytes and over the measured pitches of those frames, in order: the same in both modes).  Without the flag nothing of this runs and no output changes.
//
// `exp_mapping <parameters> --sor` (or mapper_outlier_removal=1): Mapper passes every key-frame's camera-frame cloud through the statistical outlier removal
// (include/ssm/mapper.h) when it makes it.  The summary line then carries `sor_keyframes N sor_in P sor_kept K sor_fnv H`: over the key-frames in order,
// the points before and after the filter and FNV-1a over the kept points (position and colour; the same in both modes).  Without the flag nothing of this runs.
// `exp_mapping <parameters> --carve` (or mapper_carve=1): Mapper applies every key-frame's depth image, as a view, to the clouds of the mapper_carve_window key-frames
// before it (free-space carving: include/ssm/mapper.h).  The summary line then carries `carve_keyframes V carve_tested T carve_removed R carve_fnv H`:
// the views applied, the verdicts given and the points removed over all of them, and FNV-1a over every key-frame's kept count and four verdict counts, in key-frame
// order (the same in both modes: every key-frame is a view exactly once, whatever the viewer thread's timing).  Without the flag nothing of this runs.
// `exp_mapping <parameters> --render [DIR]` (or mapper_render=1, mapper_render_dir=DIR): when the viewer ends, Mapper renders into every key-frame's view the clouds of
// the key-frames around it and compares the rendering with the frame's own depth and semantic image (map rendering: include/ssm/mapper.h); with DIR the
// rendered images are written there as PNG.  The summary line then carries `render_views V render_agree A render_in_front F render_behind B render_label_agree L
// render_label_disagree D render_fnv H`: the views, the sums of those counts over them, and FNV-1a over every view's nine counts in key-frame order (the same in both
// modes: it runs once, at the end).  Without the flag nothing of this runs and the line is as before.
// `exp_mapping <parameters> --relabel` (or mapper_relabel=1): when the viewer ends, every key-frame's cloud takes the labels its neighbouring key-frames agree on (label
// fusion: include/ssm/mapper.h), before the rendering and the grid, and one more map rebuild follows.  The summary line then carries `relabel_keyframes K
// relabel_changed C relabel_filled F relabel_fnv H`: H is FNV-1a over every key-frame's label bytes, in order.  Without the flag nothing of this runs.
// `exp_mapping <parameters> --objects [DIR]` (or mapper_objects=1, mapper_objects_dir=DIR): right after the ground grid, Mapper extracts the labelled obstacle instances
// that stand on it (include/ssm/mapper.h); with DIR objects.txt and objects_id.png are written there.  The summary line then carries
// `objects_found K objects_cells C objects_points P objects_fnv H`: the objects, their cells, their points, and FNV-1a over nx, ny, the records and the object_id image.
// `exp_mapping <parameters> --clearance [DIR]` (or mapper_clearance=1, mapper_clearance_dir=DIR): after the ground grid (and the objects), Mapper computes the grid's
// clearance map (include/ssm/mapper.h); with DIR clearance.png, reach.png and clearance.txt are written there.  The summary line then carries, after
// every other field, `clearance_blocked B clearance_traversable T clearance_reachable R clearance_max_d2 M clearance_fnv H`: H is FNV-1a over dist2, nearest and reach.
// `exp_mapping <parameters> --route [DIR]` (or mapper_route=1, mapper_route_dir=DIR): after the clearance map Mapper computes the route field over it and one path
// (include/ssm/mapper.h); with DIR route.png, route_cost.png and route.txt are written there.  The summary line then carries, after every other field,
// `route_routed N route_max_cost C route_path_len L route_path_cost P route_fnv H`: H is FNV-1a over cost, parent and the path's cells.
// `exp_mapping <parameters> --grid [DIR]` (or mapper_grid=1, mapper_grid_dir=DIR): when the viewer ends, Mapper builds ONE ground grid from every key-frame's cloud at
// its map pose (include/ssm/mapper.h); with DIR grid_colour.png, grid_height.png and grid.txt are written there.  The summary line then carries
// `grid_cells C grid_drivable D grid_walkable W grid_obstacle O grid_fnv H`: the cells of the grid, three of its class counts, and FNV-1a over nx, ny and the fetched
// arrays in the order cls, ground_label, obstacle_label, ground_q, top_q, n, n_high (the same in both modes).  Without the flag nothing of this runs.
// `exp_mapping <parameters> --align` (or mapper_align=1): Mapper aligns every key-frame's depth image to the clouds of the mapper_align_window key-frames before it and
// uses the corrected map pose from there on (dense alignment: include/ssm/mapper.h).  The summary line then carries `align_keyframes N align_accepted A
// align_fnv H`: the key-frames aligned, the alignments accepted, and FNV-1a over every key-frame's status, iteration count, counts and the bytes of its correction D_j,
// in key-frame order (the same in both modes: every key-frame is aligned exactly once).  Without the flag nothing of this runs and the line is as before.
// `exp_mapping <parameters> --fuse-motion` (or motion_semantic_fuse=1; implies --moving, so it needs tracker_mode=stereo too): Mapper gates every key-frame's cloud with
// the semantic-motion fusion of the frame's semantic image and its moving_mask (include/ssm/mapper.h) instead of the class mask alone.  The summary line
// then carries `fused_keyframes K fused_confirmed C fused_added N fused_fnv H`: over the key-frames in order, the blobs confirmed as moving, the mask pixels they add to
// the always-moving classes, and FNV-1a over every fused mask (the same in both modes).  Without the flag nothing of this runs and no output changes.
//
// `exp_mapping <parameters> --ranks N`: the multi-GPU form (BASELINE.json configs[4]; the reference is one process).  The parent starts
// N FRESH processes of itself (`--rank r`, fork + exec of /proc/self/exe) before anything touches HIP -- a forked copy of a process whose HIP / RCCL
// static constructors have already run is not a state either library is tested in; rank r drives GPU r, owns the contiguous frame block [lo, hi) of
// [start_index, end_index), feeds the tracker_ref_frames frames in front of its block to the tracker only (the matcher halo: Tracker::trackRefFrame
// matches against the refFrames deque, src/track.cpp:150-152), maps its key-frames as usual, then inserts their clouds into one context map and calls
// ssm_voxel_allgather (ONE RCCL all-gather behind the C ABI).  Every rank ends with the map of the whole sequence; rank 0 prints it.  The ncclUniqueId
// travels through a file in a private temporary directory (written under another name, then renamed).  The parent reaps with waitpid(-1): the first
// rank that fails (or `rank_timeout_s`, default 900) gets the others killed, so a rank blocked in ncclCommInitRank never outlives its failed peer.
#include "ssm/rgbdframe.h"
#include "ssm/track.h"
#include "ssm/pose_graph.h"
#include "ssm/common_headers.h"
#include "ssm/mapper.h"
#include "ssm/vo_stereo.hpp"
#include "ssm/batch_stereo_tracker.h"
#include "ssm/batch_tracker.h"
#include "ssm/looper.h"
#include <signal.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>
using namespace std;
using namespace rgbd_tutor;

static int run_rank(ParameterReader& parameterReader, int rank, int nranks, const string& id_dir);
static FrameReader::DATASET dataset_type(const ParameterReader& pr)
{
    const string ds = pr.getData<string>("dataset", string("synthetic"));
    return ds == "raw" ? FrameReader::RAW : ds == "tum" ? FrameReader::TUM : ds == "kitti" ? FrameReader::KITTI : FrameReader::SYNTHETIC;
}

// every frame's final T_f_w, in frame order: FNV-1a over the 128 bytes (printed as pose_fnv) and, with trajectory_output=<file>, one text line per frame
// (id, then the 16 column-major doubles as C99 hex floats: exact)
struct Trajectory {
    uint64_t h = 0xCBF29CE484222325ull; ofstream out;
    explicit Trajectory(const string& path) { if (!path.empty()) out.open(path); }
    void add(const RGBDFrame::Ptr& f) {
        const Eigen::Isometry3d T = f->getTransform();
        const unsigned char* b = (const unsigned char*)T.data();
        for (int k = 0; k < 128; k++) { h ^= b[k]; h *= 0x100000001B3ull; }
        if (out.is_open()) { char buf[64]; out << f->id; for (int k = 0; k < 16; k++) { snprintf(buf, sizeof(buf), " %a", T.data()[k]); out << buf; } out << "\n"; }
    }
};

// the loop candidates in the order they were found: count, FNV-1a over (frame id, candidate id, score), and with loops_output=<file> one text line each
struct LoopLog {
    uint64_t h = 0xCBF29CE484222325ull; long n = 0; ofstream out;
    explicit LoopLog(const string& path) { if (!path.empty()) out.open(path); }
    void add(int32_t frame_id, int32_t cand_id, double score) {
        unsigned char b[16]; memcpy(b, &frame_id, 4); memcpy(b + 4, &cand_id, 4); memcpy(b + 8, &score, 8);
        for (int k = 0; k < 16; k++) { h ^= b[k]; h *= 0x100000001B3ull; }
        n++;
        if (out.is_open()) { char buf[64]; snprintf(buf, sizeof(buf), " %a", score); out << frame_id << " " << cand_id << buf << "\n"; }
    }
};

// --moving: the moving masks of the frames UVDisparity::Process ran on, in frame order: the count of moving pixels, FNV-1a over the mask bytes, FNV-1a over the
// measured pitches (the 8 bytes of pitch1)
struct MovingLog {
    uint64_t hm = 0xCBF29CE484222325ull, hp = 0xCBF29CE484222325ull; long long pixels = 0;
    void add(const cv::Mat& mask, double pitch) {
        for (int r = 0; r < mask.rows; r++) { const unsigned char* b = mask.ptr<unsigned char>(r); for (int c = 0; c < mask.cols; c++) { hm ^= b[c]; hm *= 0x100000001B3ull; pixels += b[c] == 255; } }
        unsigned char pb[8]; memcpy(pb, &pitch, 8);
        for (int k = 0; k < 8; k++) { hp ^= pb[k]; hp *= 0x100000001B3ull; }
    }
};

int main(int argc, char** argv)
{
    ParameterReader parameterReader(argc > 1 ? argv[1] : "./parameters.txt");
    int nranks = 1, my_rank = -1; string id_dir;
    bool batched = parameterReader.getData<int>("tracker_batched", 0) != 0;
    for (int i = 2; i < argc; i++) if (string(argv[i]) == "--batched") batched = true;
    bool loops = parameterReader.getData<int>("looper", 0) != 0;
    for (int i = 2; i < argc; i++) if (string(argv[i]) == "--loops") loops = true;
    // --optimize (or pose_graph_optimize=1): PoseGraph keeps the graph and PoseGraph::step() runs SYNCHRONOUSLY -- after every accepted key-frame, or, with
    // pose_graph_step_frames=K > 0, after every K-th frame and at the end (the boundaries of a --batched run with tracker_chunk=K, which steps once per chunk).
    // It implies --loops when a vocabulary is configured; the candidates then come from PoseGraph's own Looper.  The summary line gets
    // `graph_vertices V graph_edges E graph_opts K kf_pose_fnv H` and traj.g2o is written next to map_output.  Off by default: nothing of this runs.
    bool optimize = parameterReader.getData<int>("pose_graph_optimize", 0) != 0;
    for (int i = 2; i < argc; i++) if (string(argv[i]) == "--optimize") optimize = true;
    if (optimize) { parameterReader.set("pose_graph_optimize", "1"); if (!parameterReader.getData<string>("looper_vocab_file", string("")).empty()) loops = true; }
    const int step_frames = parameterReader.getData<int>("pose_graph_step_frames", 0);
    string train_vocab = parameterReader.getData<string>("looper_train_vocab", string(""));
    for (int i = 2; i + 1 < argc; i++) if (string(argv[i]) == "--train-vocab") train_vocab = argv[i + 1];
    bool moving = parameterReader.getData<int>("uv_disparity", 0) != 0;
    for (int i = 2; i < argc; i++) if (string(argv[i]) == "--moving") moving = true;
    bool fuse_motion = parameterReader.getData<int>("motion_semantic_fuse", 0) != 0;
    for (int i = 2; i < argc; i++) if (string(argv[i]) == "--fuse-motion") fuse_motion = true;
    if (fuse_motion) moving = true;
    if (moving) {
        if (parameterReader.getData<string>("tracker_mode", string("rgbd")) != "stereo") { cerr << "exp_mapping: " << (fuse_motion ? "--fuse-motion" : "--moving") << " needs tracker_mode=stereo (the U/V-disparity stage works on the SGBM disparity)" << endl; return 2; }
        parameterReader.set("uv_disparity", "1");
    }
    if (fuse_motion) parameterReader.set("motion_semantic_fuse", "1");
    bool sor = parameterReader.getData<int>("mapper_outlier_removal", 0) != 0;
    for (int i = 2; i < argc; i++) if (string(argv[i]) == "--sor") sor = true;
    if (sor) parameterReader.set("mapper_outlier_removal", "1");
    bool carve = parameterReader.getData<int>("mapper_carve", 0) != 0;
    for (int i = 2; i < argc; i++) if (string(argv[i]) == "--carve") carve = true;
    if (carve) parameterReader.set("mapper_carve", "1");
    bool align = parameterReader.getData<int>("mapper_align", 0) != 0;
    for (int i = 2; i < argc; i++) if (string(argv[i]) == "--align") align = true;
    if (align) parameterReader.set("mapper_align", "1");
    bool render = parameterReader.getData<int>("mapper_render", 0) != 0;
    for (int i = 2; i < argc; i++) if (string(argv[i]) == "--render") {
        render = true;
        if (i + 1 < argc && argv[i + 1][0] != '-') parameterReader.set("mapper_render_dir", argv[i + 1]);          // (the directory is optional: without it no file is written)
    }
    if (render) parameterReader.set("mapper_render", "1");
    bool grid = parameterReader.getData<int>("mapper_grid", 0) != 0;
    for (int i = 2; i < argc; i++) if (string(argv[i]) == "--grid") {
        grid = true;
        if (i + 1 < argc && argv[i + 1][0] != '-') parameterReader.set("mapper_grid_dir", argv[i + 1]);          // (the directory is optional: without it no file is written)
    }
    if (grid) parameterReader.set("mapper_grid", "1");
    bool objects = parameterReader.getData<int>("mapper_objects", 0) != 0;
    for (int i = 2; i < argc; i++) if (string(argv[i]) == "--objects") {
        objects = true;
        if (i + 1 < argc && argv[i + 1][0] != '-') parameterReader.set("mapper_objects_dir", argv[i + 1]);          // (the directory is optional: without it no file is written)
    }
    if (objects) parameterReader.set("mapper_objects", "1");
    bool clearance = parameterReader.getData<int>("mapper_clearance", 0) != 0;
    for (int i = 2; i < argc; i++) if (string(argv[i]) == "--clearance") {
        clearance = true;
        if (i + 1 < argc && argv[i + 1][0] != '-') parameterReader.set("mapper_clearance_dir", argv[i + 1]);          // (the directory is optional: without it no file is written)
    }
    if (clearance) parameterReader.set("mapper_clearance", "1");
    bool route = parameterReader.getData<int>("mapper_route", 0) != 0;
    for (int i = 2; i < argc; i++) if (string(argv[i]) == "--route") {
        route = true;
        if (i + 1 < argc && argv[i + 1][0] != '-') parameterReader.set("mapper_route_dir", argv[i + 1]);          // (the directory is optional: without it no file is written)
    }
    if (route) parameterReader.set("mapper_route", "1");
    bool relabel = parameterReader.getData<int>("mapper_relabel", 0) != 0;
    for (int i = 2; i < argc; i++) if (string(argv[i]) == "--relabel") relabel = true;
    if (relabel) { parameterReader.set("mapper_relabel", "1"); parameterReader.set("mapper_relabel_hash", "1"); }
    MovingLog moving_log;
    for (int i = 2; i + 1 < argc; i++) {
        if (string(argv[i]) == "--ranks") nranks = atoi(argv[i + 1]);
        if (string(argv[i]) == "--rank") my_rank = atoi(argv[i + 1]);
        if (string(argv[i]) == "--id-dir") id_dir = argv[i + 1];
    }
    if (my_rank >= 0) {                                   // a rank process started by the parent below
        if (nranks < 1 || my_rank >= nranks || id_dir.empty()) { cerr << "exp_mapping: --rank needs --ranks N and --id-dir" << endl; return 2; }
        try { return run_rank(parameterReader, my_rank, nranks, id_dir); }
        catch (const exception& e) { cerr << RED << "rank " << my_rank << ": " << e.what() << RESET << endl; return 2; }
    }
    if (nranks > 1 || parameterReader.getData<int>("force_rank_path", 0)) {
        char tmpl[] = "/tmp/ssm_ranks_XXXXXX";
        if (!mkdtemp(tmpl)) { perror("mkdtemp"); return 2; }
        const string dir = tmpl, ranks_s = to_string(nranks);
        vector<pid_t> kids;
        // INVARIANT: nothing above this point creates an ssm::Device (ParameterReader only parses the file): the parent forks and the children exec BEFORE any HIP
        // call.  Never move device work in front of this loop; the counter makes a violation fail here instead of on the node.
        if (ssm::devices_created().load() != 0) { cerr << RED << "exp_mapping: internal error: a device context exists before the ranks are started" << RESET << endl; return 2; }
        for (int r = 0; r < nranks; r++) {
            pid_t p = fork();                                 // no HIP call has happened in this process; the child execs at once
            if (p < 0) { perror("fork"); for (pid_t k : kids) kill(k, SIGKILL); return 2; }
            if (p == 0) {
                const string rs = to_string(r);
                const char* av[] = { argv[0], argv[1], "--ranks", ranks_s.c_str(), "--rank", rs.c_str(), "--id-dir", dir.c_str(), nullptr };
                execv("/proc/self/exe", const_cast<char* const*>(av));
                perror("execv"); _exit(127);
            }
            kids.push_back(p);
        }
        const int timeout_s = parameterReader.getData<int>("rank_timeout_s", 900);
        const auto t0 = chrono::steady_clock::now();
        int rc = 0; size_t alive = kids.size();
        while (alive) {
            int st = 0; const pid_t p = waitpid(-1, &st, WNOHANG);
            if (p > 0) {
                alive--;
                for (pid_t& k : kids) if (k == p) k = -1;
                if (!WIFEXITED(st) || WEXITSTATUS(st)) {
                    if (!rc) { cerr << RED << "exp_mapping: a rank failed (status " << st << "); stopping the others" << RESET << endl; for (pid_t k : kids) if (k > 0) kill(k, SIGKILL); }
                    rc = 1;
                }
                continue;
            }
            if (p < 0 && errno != EINTR) break;
            if (chrono::duration<double>(chrono::steady_clock::now() - t0).count() > timeout_s) {
                if (!rc) { cerr << RED << "exp_mapping: ranks still running after " << timeout_s << " s; killing them" << RESET << endl; for (pid_t k : kids) if (k > 0) kill(k, SIGKILL); }
                rc = 1;
            }
            this_thread::sleep_for(chrono::milliseconds(5));
        }
        unlink((dir + "/nccl_id").c_str()); rmdir(dir.c_str());
        return rc;
    }
    VisualOdometryStereo::parameters voparam;
    double f = parameterReader.getData<double>("camera.fx");
    double c_u = parameterReader.getData<double>("camera.cx");
    double c_v = parameterReader.getData<double>("camera.cy");
    double base = parameterReader.getData<double>("camera.baseline", 0.0);
    double inlier_threshold = parameterReader.getData<double>("inlier_threshold", 6.0);
    voparam.calib.f = f; voparam.calib.cu = c_u;
    voparam.calib.cv = c_v; voparam.base = base;
    voparam.inlier_threshold = inlier_threshold;
    try {
        Tracker::Ptr tracker(new Tracker(parameterReader, voparam));
        const FrameReader::DATASET type = dataset_type(parameterReader);
        const bool batched_stereo = batched && parameterReader.getData<string>("tracker_mode", string("rgbd")) == "stereo";
        if (optimize && batched_stereo) {                  // solvePnPLazy needs ORB features and RGB-D key-frames; the bulk stereo tracker has neither
            cerr << "exp_mapping: --optimize is not available with the bulk stereo tracker (ignored)" << endl;
            optimize = false; parameterReader.set("pose_graph_optimize", "0");
        }
        if (batched_stereo) parameterReader.set("kitti_reader_depth", "0");     // the bulk stereo tracker computes the depth images, a chunk of frames per launch
        FrameReader frameReader(parameterReader, type);
        PoseGraph poseGraph(parameterReader, tracker);
        Mapper mapper(parameterReader, poseGraph);
        const bool use_gt_pose = parameterReader.getData<int>("use_stream_pose", (type == FrameReader::TUM || type == FrameReader::KITTI) ? 0 : 1) != 0;
        int nframes = 0;
        const int frame_period_ms = parameterReader.getData<int>("frame_period_ms", 0);
        Trajectory traj(parameterReader.getData<string>("trajectory_output", string("")));
        LoopLog loop_log(loops ? parameterReader.getData<string>("loops_output", string("")) : string(""));
        if (loops && batched_stereo) cerr << "exp_mapping: --loops needs ORB descriptors; the bulk stereo tracker computes none (ignored)" << endl;
        if (!train_vocab.empty() && batched_stereo) { cerr << "exp_mapping: --train-vocab needs ORB descriptors; the bulk stereo tracker computes none (ignored)" << endl; train_vocab.clear(); }
        vector<vector<uint8_t>> train_sets;                    // --train-vocab: the descriptors of every accepted key-frame, in key-frame order
        TrainedVocabulary trained;
        // `sequence_length` = L > 0: the stream is a concatenation of independent sequences of L frames (synthetic_rigid streams): the tracker starts over at every
        // multiple of L.  `timing_skip_frames`: the rates printed at the end leave out the first frames (context creation, code-object load, first-use allocations).
        const int seq_len = parameterReader.getData<int>("sequence_length", 0), skip = parameterReader.getData<int>("timing_skip_frames", 0);
        // where the loop's wall time goes, the way the reference's drivers time it: FrameReader::next (experiment/exp_mapping.cpp:36), Tracker::updateFrame
        // (experiment/run_tracker.cpp:35-48) / BatchTracker::push, PoseGraph::tryInsertKeyFrame (:47)
        double reader_s = 0, track_s = 0, kf_s = 0; int timed = 0;
        typedef chrono::steady_clock::time_point tp;
        auto now = [] { return chrono::steady_clock::now(); };
        auto sec = [](tp a, tp b) { return chrono::duration<double>(b - a).count(); };
        // reader_preload = 1: every frame is read before the loop starts (frames resident in host memory, like the inputs of bench.py's timed region are resident in HBM):
        // the loop then measures the tracker / mapper side alone.  preload_s is printed.
        vector<RGBDFrame::Ptr> preloaded; size_t pre_i = 0; double preload_s = 0;
        const bool preload = parameterReader.getData<int>("reader_preload", 0) != 0;
        if (preload) { const tp a = now(); while (RGBDFrame::Ptr f = frameReader.next()) preloaded.push_back(f); preload_s = sec(a, now()); }
        auto t0 = now(); tp t_timed0 = t0, t1 = t0;          // t1: the end of the loop (taken before a bulk tracker and its device context are torn down)
        auto read_next = [&]() {
            const tp a = now();
            RGBDFrame::Ptr f;
            if (preload) { if (pre_i < preloaded.size()) { f = preloaded[pre_i]; preloaded[pre_i++] = nullptr; } } else f = frameReader.next();
            if (nframes >= skip && f) reader_s += sec(a, now());
            return f; };
        if (batched && parameterReader.getData<string>("tracker_mode", string("rgbd")) == "rgbd") {
            unique_ptr<BatchTracker> bt; map<int, Eigen::Isometry3d> gt; int lost = 0; int pushed = 0;
            unique_ptr<BatchLooper> bl;                        // (after bt: it lives in the tracker's context and goes first)
            const bool chain = parameterReader.getData<int>("tracker_batched_chain", 1) != 0;
            if (!chain && !use_gt_pose) throw invalid_argument("tracker_batched_chain=0 needs use_stream_pose=1: without the chain nothing computes the poses");
            // (rates: a chunk counts as a whole -- the frames of a flush that started at or after timing_skip_frames, against the time of that flush)
            auto handle = [&](const vector<RGBDFrame::Ptr>& done, bool counted) {
                vector<int> picked;                            // the chunk's key-frames
                for (size_t i = 0; i < done.size(); i++) {
                    const RGBDFrame::Ptr& f = done[i];
                    if (use_gt_pose) f->setTransform(gt[f->id]);
                    gt.erase(f->id);
                    traj.add(f);
                    if (poseGraph.tryInsertKeyFrame(const_cast<RGBDFrame::Ptr&>(f))) picked.push_back((int)i);
                    if (bt->infos[i].state == Tracker::LOST) { cout << "tracker is lost" << endl; lost++; }
                    if (counted) timed++;
                    nframes++;
                }
                if (optimize) { if (!done.empty()) poseGraph.step(); }          // once per chunk; its Looper supplies the candidates
                else if (loops && !picked.empty()) {
                    if (!bl) bl.reset(new BatchLooper(parameterReader, bt->device()));
                    for (const BatchLooper::Candidate& c : bl->addChunk(bt->last_out, done, picked)) loop_log.add(c.frame->id, c.loop->id, c.score);
                }
                if (!train_vocab.empty() && !picked.empty()) {      // the bulk loop keeps no host copy of the descriptors: the key-frames' rows come down per chunk
                    const ssm_seq_out_dev& o = bt->last_out;
                    vector<int32_t> nkp(done.size());
                    bt->device().check(ssm_memcpy_d2h(bt->device().ctx(), nkp.data(), o.nkp, nkp.size() * 4), "ssm_memcpy_d2h");
                    for (int i : picked) {
                        train_sets.emplace_back((size_t)max(0, min(nkp[i], o.cap)) * 32);
                        if (!train_sets.back().empty()) bt->device().check(ssm_memcpy_d2h(bt->device().ctx(), train_sets.back().data(), o.desc + (size_t)i * o.cap * 32, train_sets.back().size()), "ssm_memcpy_d2h");
                    }
                }
            };
            while (RGBDFrame::Ptr frame = read_next()) {
                if (!bt) bt.reset(new BatchTracker(parameterReader, frame->rgb.cols, frame->rgb.rows, frame->T_f_w));
                const bool count = nframes >= skip; const tp a = now();
                if (count && timed == 0 && track_s == 0) t_timed0 = a;
                if (seq_len > 0 && chain && pushed > 0 && pushed % seq_len == 0) { handle(bt->flush(), count); bt->reset(); }     // (without the chain a sequence boundary changes nothing: features and tables only)
                gt[frame->id] = frame->T_f_w;
                pushed++;
                handle(bt->push(frame), count);
                if (count) track_s += sec(a, now());
            }
            const tp a = now(); const bool count = nframes >= skip;
            if (bt) handle(bt->flush(), count);
            if (count) track_s += sec(a, now());
            t1 = now();
            if (!train_vocab.empty()) trained = trainVocabulary(parameterReader, train_sets, bt ? &bt->device() : nullptr, train_vocab);      // (while the tracker's context lives)
            cout << "batched tracker: chunk " << (bt ? bt->chunk() : 0) << " lost " << lost << endl;
        } else if (batched_stereo) {
            // Tracker::estimateVO + FrameReader's SGBM depth in bulk (include/ssm/batch_stereo_tracker.h): quad matcher, depth and ego-motion of a chunk per launch
            unique_ptr<BatchStereoTracker> bs; int lost = 0;
            auto handle = [&](const vector<RGBDFrame::Ptr>& done, bool counted) {
                for (size_t i = 0; i < done.size(); i++) {
                    const RGBDFrame::Ptr& f = done[i];
                    traj.add(f);
                    if (moving && bs->infos[i].uv) moving_log.add(f->moving_mask, bs->infos[i].pitch1);       // (before the key-frame gate: Mapper overwrites a key-frame's mask)
                    poseGraph.tryInsertKeyFrame(const_cast<RGBDFrame::Ptr&>(f));
                    if (bs->infos[i].state == Tracker::LOST) { cout << "tracker is lost" << endl; lost++; }
                    if (counted) timed++;
                    nframes++;
                }
            };
            while (RGBDFrame::Ptr frame = read_next()) {
                if (!bs) bs.reset(new BatchStereoTracker(parameterReader, voparam, frame->img_lc.cols, frame->img_lc.rows));
                const bool count = nframes >= skip; const tp a = now();
                if (count && timed == 0 && track_s == 0) t_timed0 = a;
                handle(bs->push(frame), count);
                if (count) track_s += sec(a, now());
            }
            const tp a = now(); const bool count = nframes >= skip;
            if (bs) handle(bs->flush(), count);
            if (count) track_s += sec(a, now());
            t1 = now();
            cout << "batched stereo tracker: chunk " << (bs ? bs->chunk() : 0) << " lost " << lost << endl;
        } else {
        unique_ptr<Looper> looper; if (loops && !optimize) looper.reset(new Looper(parameterReader));
        while (RGBDFrame::Ptr frame = read_next()) {
            if (nframes == skip) { t_timed0 = now(); tracker->timing = Tracker::Timing(); }
            if (seq_len > 0 && nframes > 0 && nframes % seq_len == 0) tracker->reset();
            Eigen::Isometry3d gt = frame->T_f_w;
            const tp a = now();
            tracker->updateFrame(frame);
            const tp b = now();
            if (use_gt_pose) frame->setTransform(gt);           // synthetic stream: poses are given, the tracker only produces features/matches
            traj.add(frame);
            if (moving && !frame->moving_mask.empty()) moving_log.add(frame->moving_mask, tracker->pitch1);
            const bool inserted = poseGraph.tryInsertKeyFrame(frame);
            if (inserted && !train_vocab.empty()) { const cv::Mat d = frame->getAllDescriptors(); train_sets.emplace_back(d.data, d.data + (size_t)d.rows * 32); }
            if (inserted && looper) {
                looper->add(frame);
                looper->getPossibleLoops(frame);
                for (int i : looper->last_indices) loop_log.add(frame->id, looper->frameAt(i)->id, looper->last_scores[i]);
            }
            if (optimize && (step_frames > 0 ? (nframes + 1) % step_frames == 0 : inserted)) poseGraph.step();
            if (nframes >= skip) { track_s += sec(a, b); kf_s += sec(b, now()); timed++; }
            if (tracker->getState() == Tracker::LOST) cout << "tracker is lost" << endl;
            nframes++;
            if (frame_period_ms > 0) this_thread::sleep_for(chrono::milliseconds(frame_period_ms));      // a camera's frame period (measurements of the viewer thread under a paced stream)
        }
        if (optimize && step_frames > 0) poseGraph.step();                 // the frames after the last boundary (a --batched run's final flush)
        t1 = now();
        if (!train_vocab.empty()) trained = trainVocabulary(parameterReader, train_sets, OrbFeature::lastDevice(), train_vocab); }
        if (optimize) for (const PoseGraph::LoopCandidate& c : poseGraph.loopCandidates) loop_log.add(c.frame, c.loop, c.score);
        const double s = sec(t0, t1), s_timed = sec(t_timed0, t1);
        mapper.SaveMap();
        poseGraph.shutdown();
        this_thread::sleep_for(chrono::milliseconds(parameterReader.getData<int>("mapper_drain_ms", 300)));
        mapper.shutdown();
        cout << "frames " << nframes << " keyframes " << poseGraph.keyframes.size() << " map_updates " << mapper.updates()
             << " map_points " << (mapper.getGlobalMap() ? mapper.getGlobalMap()->points.size() : 0) << " pose_fnv " << hex << traj.h << dec << " host_loop_fps " << nframes / s;
        // the rates of the frames after timing_skip_frames: loop_fps = the whole loop (reader included); tracker_fps = frames / time inside updateFrame (or BatchTracker::push /
        // flush) -- what experiment/run_tracker.cpp:35-48 times; the *_ms are per frame
        if (moving) cout << " moving_pixels " << moving_log.pixels << " moving_fnv " << hex << moving_log.hm << " pitch_fnv " << moving_log.hp << dec;
        if (fuse_motion) {      // (the viewer thread has ended: the Mapper's device is this thread's now)
            uint64_t h = 0xCBF29CE484222325ull; long long confirmed = 0, added = 0;
            for (RGBDFrame::Ptr& kf : poseGraph.keyframes) {
                ssm_motion_fuse_info I{};
                const cv::Mat m = mapper.semantic_motion_fuse(kf, &I);
                confirmed += I.confirmed; added += I.added;
                for (int r = 0; r < m.rows; r++) { const unsigned char* b = m.ptr<unsigned char>(r); for (int c = 0; c < m.cols; c++) { h ^= b[c]; h *= 0x100000001B3ull; } }
            }
            cout << " fused_keyframes " << poseGraph.keyframes.size() << " fused_confirmed " << confirmed << " fused_added " << added << " fused_fnv " << hex << h << dec;
        }
        if (sor) {              // (the viewer thread has ended; a key-frame it never reached gets its cloud here, by the host route -- the same bytes)
            uint64_t h = 0xCBF29CE484222325ull; long long n_in = 0, n_kept = 0;
            for (RGBDFrame::Ptr& kf : poseGraph.keyframes) {
                mapper.generatePointCloud(kf);
                ssm_sor_info I{};
                if (!mapper.sorInfoOf(kf, &I)) { cerr << "exp_mapping: a key-frame's cloud was not filtered" << endl; return 3; }
                n_in += I.n_in; n_kept += I.n_kept;
                for (const Mapper::PointT& p : kf->pointcloud->points) { const unsigned char* b = (const unsigned char*)&p; for (int k = 0; k < 20; k++) { if (k == 12) k = 16; h ^= b[k]; h *= 0x100000001B3ull; } }
            }
            cout << " sor_keyframes " << poseGraph.keyframes.size() << " sor_in " << n_in << " sor_kept " << n_kept << " sor_fnv " << hex << h << dec;
        }
        if (carve) {            // (the viewer thread made every key-frame a view before it ended)
            if (mapper.viewerFailed) { cerr << "exp_mapping: the viewer stopped before every key-frame was applied" << endl; return 3; }
            uint64_t h = 0xCBF29CE484222325ull; long long tested = 0, removed = 0;
            for (RGBDFrame::Ptr& kf : poseGraph.keyframes) {
                ssm_carve_info I{};
                mapper.carveInfoOf(kf, &I);               // (the last key-frame's cloud has seen no view: zeros)
                tested += (long long)I.unknown + I.occluded + I.supported + I.seen_through; removed += I.removed;
                const int32_t v[5] = {I.n_kept, I.unknown, I.occluded, I.supported, I.seen_through};
                const unsigned char* b = (const unsigned char*)v;
                for (size_t k = 0; k < sizeof v; k++) { h ^= b[k]; h *= 0x100000001B3ull; }
            }
            cout << " carve_keyframes " << mapper.carvedViews() << " carve_tested " << tested << " carve_removed " << removed << " carve_fnv " << hex << h << dec;
        }
        if (align) {            // (the viewer thread aligned every key-frame before it ended)
            if (mapper.viewerFailed) { cerr << "exp_mapping: the viewer stopped before every key-frame was aligned" << endl; return 3; }
            uint64_t h = 0xCBF29CE484222325ull;
            for (RGBDFrame::Ptr& kf : poseGraph.keyframes) {
                ssm_align_info I{}; Eigen::Isometry3d D;
                if (!mapper.alignInfoOf(kf, &I, &D)) { cerr << "exp_mapping: a key-frame was not aligned" << endl; return 3; }
                const int64_t v[7] = {I.status, I.iterations, I.n_in, I.tested_first, I.inliers_first, I.tested_last, I.inliers_last};
                const unsigned char* b = (const unsigned char*)v;
                for (size_t k = 0; k < sizeof v; k++) { h ^= b[k]; h *= 0x100000001B3ull; }
                b = (const unsigned char*)D.data();
                for (size_t k = 0; k < 16 * sizeof(double); k++) { h ^= b[k]; h *= 0x100000001B3ull; }
            }
            cout << " align_keyframes " << mapper.alignedKeyframes() << " align_accepted " << mapper.acceptedAlignments() << " align_fnv " << hex << h << dec;
        }
        if (render) {           // (the viewer thread rendered every key-frame's view as it ended)
            if (mapper.viewerFailed) { cerr << "exp_mapping: the viewer stopped before every view was rendered" << endl; return 3; }
            uint64_t h = 0xCBF29CE484222325ull; long long agree = 0, in_front = 0, behind = 0, lab_agree = 0, lab_dis = 0;
            for (RGBDFrame::Ptr& kf : poseGraph.keyframes) {
                ssm_render_compare_info I{};
                mapper.renderInfoOf(kf, &I);
                agree += I.agree; in_front += I.in_front; behind += I.behind; lab_agree += I.label_agree; lab_dis += I.label_disagree;
                const unsigned char* b = (const unsigned char*)&I;
                for (size_t k = 0; k < sizeof I; k++) { h ^= b[k]; h *= 0x100000001B3ull; }
            }
            cout << " render_views " << mapper.renderedViews() << " render_agree " << agree << " render_in_front " << in_front << " render_behind " << behind
                 << " render_label_agree " << lab_agree << " render_label_disagree " << lab_dis << " render_fnv " << hex << h << dec;
        }
        if (relabel) {          // (the viewer thread relabelled every key-frame's cloud as it ended)
            if (mapper.viewerFailed) { cerr << "exp_mapping: the viewer stopped before the clouds were relabelled" << endl; return 3; }
            long long changed = 0, filled = 0;
            for (RGBDFrame::Ptr& kf : poseGraph.keyframes) { ssm_relabel_info I{}; mapper.relabelInfoOf(kf, &I); changed += I.n_changed; filled += I.n_filled; }
            cout << " relabel_keyframes " << mapper.relabelledKeyframes() << " relabel_changed " << changed << " relabel_filled " << filled << " relabel_fnv " << hex
                 << mapper.relabelLabelFnv() << dec;
        }
        if (grid) {             // (the viewer thread built the grid of every key-frame's cloud as it ended)
            if (mapper.viewerFailed) { cerr << "exp_mapping: the viewer stopped before the ground grid was built" << endl; return 3; }
            const Mapper::GridInfo& G = mapper.gridInfo();
            vector<uint8_t> cls, gl, ol; vector<int32_t> gq, tq; vector<uint32_t> gn, gh;
            mapper.gridFetch(&cls, &gl, &ol, &gq, &tq, &gn, &gh);
            uint64_t h = 0xCBF29CE484222325ull;           // FNV-1a over nx, ny and the arrays: cls, ground_label, obstacle_label, ground_q, top_q, n, n_high
            auto eat = [&h](const void* p, size_t bytes) { const unsigned char* b = (const unsigned char*)p; for (size_t k = 0; k < bytes; k++) { h ^= b[k]; h *= 0x100000001B3ull; } };
            const int32_t shape[2] = {mapper.gridParams().nx, mapper.gridParams().ny};
            eat(shape, sizeof shape);
            eat(cls.data(), cls.size()); eat(gl.data(), gl.size()); eat(ol.data(), ol.size()); eat(gq.data(), gq.size() * 4); eat(tq.data(), tq.size() * 4); eat(gn.data(), gn.size() * 4);
            eat(gh.data(), gh.size() * 4);
            cout << " grid_cells " << cls.size() << " grid_drivable " << G.counts.drivable << " grid_walkable " << G.counts.walkable << " grid_obstacle " << G.counts.obstacle
                 << " grid_fnv " << hex << h << dec;
        }
        if (objects) {          // (the viewer thread extracted the objects right after the grid as it ended)
            if (mapper.viewerFailed) { cerr << "exp_mapping: the viewer stopped before the objects were extracted" << endl; return 3; }
            const Mapper::ObjectsInfo& O = mapper.objectsInfo();
            vector<ssm_object> rec; vector<int32_t> oid;
            mapper.objectsFetch(&rec, &oid);
            uint64_t h = 0xCBF29CE484222325ull;           // FNV-1a over nx, ny, the records and the object_id image
            auto eat = [&h](const void* p, size_t bytes) { const unsigned char* b = (const unsigned char*)p; for (size_t k = 0; k < bytes; k++) { h ^= b[k]; h *= 0x100000001B3ull; } };
            const int32_t shape[2] = {mapper.gridParams().nx, mapper.gridParams().ny};
            eat(shape, sizeof shape); eat(rec.data(), rec.size() * sizeof(ssm_object)); eat(oid.data(), oid.size() * 4);
            uint64_t cells = 0; for (const ssm_object& o : rec) cells += o.cells;
            cout << " objects_found " << rec.size() << " objects_cells " << cells << " objects_points " << O.counts.object_points << " objects_fnv " << hex << h << dec;
        }
        if (timed > 0) {
            const Tracker::Timing& tt = tracker->timing; const double fr = tt.frames > 0 ? (double)tt.frames : 1.0;
            cout << " timed_frames " << timed << " loop_fps " << timed / s_timed << " tracker_fps " << (track_s > 0 ? timed / track_s : 0.0) << " reader_ms " << reader_s * 1e3 / timed
                 << " preload_s " << preload_s << " tracker_ms " << track_s * 1e3 / timed << " keyframe_ms " << kf_s * 1e3 / timed << " detect_ms " << tt.detect_ms / fr << " match_ms " << tt.match_ms / fr << " pnp_ms " << tt.pnp_ms / fr;
        }
        // final_map_fnv = K > 0: the clouds of the first K key-frames fused into ONE context map (what `globalMap += cloud` over all key-frames + one VoxelGrid pass holds,
        // src/mapper.cpp:121-158), FNV-1a of its centroids -- unlike map_points above it does not depend on the viewer thread's update schedule, so two runs (per-frame
        // and --batched, 1 or N ranks) can be compared by it
        if (const int fm = parameterReader.getData<int>("final_map_fnv", 0); fm > 0 && !poseGraph.keyframes.empty()) {
            ssm::Device dev(parameterReader.deviceConfig(frameReader.width, frameReader.height));
            int used = 0;
            for (RGBDFrame::Ptr& kf : poseGraph.keyframes) {
                if (used++ >= fm) break;
                Mapper::PointCloud::Ptr c = mapper.generatePointCloud(kf);
                if (!c->points.empty()) dev.check(ssm_map_insert(dev.ctx(), reinterpret_cast<const ssm_point*>(c->points.data()), (int)c->points.size()), "ssm_map_insert");
            }
            int nvox = 0; dev.check(ssm_map_size(dev.ctx(), &nvox), "ssm_map_size");
            vector<ssm_point> m((size_t)max(nvox, 1));
            dev.check(ssm_map_export(dev.ctx(), m.data(), (int)m.size(), &nvox), "ssm_map_export");
            uint64_t h = 0xCBF29CE484222325ull;
            for (int i = 0; i < nvox; i++) { const unsigned char* b = (const unsigned char*)&m[i]; for (int k = 0; k < 24; k++) { h ^= b[k]; h *= 0x100000001B3ull; } }
            cout << " map_voxels " << nvox << " map_fnv " << hex << h << dec;
        }
        if (loops) cout << " loop_candidates " << loop_log.n << " loop_fnv " << hex << loop_log.h << dec;
        if (!train_vocab.empty()) cout << " vocab_nodes " << trained.nodes << " vocab_words " << trained.words << " vocab_fnv " << hex << trained.fnv << dec;
        if (optimize) {
            uint64_t h = 0xCBF29CE484222325ull;                           // FNV-1a over the key-frames' final poses, in key-frame order
            for (RGBDFrame::Ptr& kf : poseGraph.keyframes) { const Eigen::Isometry3d T = kf->getTransform(); const unsigned char* b = (const unsigned char*)T.data(); for (int k = 0; k < 128; k++) { h ^= b[k]; h *= 0x100000001B3ull; } }
            cout << " graph_vertices " << poseGraph.graphVertices() << " graph_edges " << poseGraph.graphEdges() << " graph_opts " << poseGraph.globalOpts + poseGraph.localOpts
                 << " kf_pose_fnv " << hex << h << dec;
            const string mo = parameterReader.getData<string>("map_output", string(""));
            const size_t slash = mo.find_last_of('/');
            poseGraph.save((slash == string::npos ? string("") : mo.substr(0, slash + 1)) + "traj.g2o");
        }
        if (clearance) {          // (the viewer thread mapped the clearance right after the grid as it ended; these fields come after every other)
            if (mapper.viewerFailed) { cerr << "exp_mapping: the viewer stopped before the clearance map was made" << endl; return 3; }
            const Mapper::ClearanceInfo& K = mapper.clearanceInfo();
            vector<uint32_t> d2; vector<int32_t> nearest; vector<uint8_t> reach;
            mapper.clearanceFetch(&d2, &nearest, &reach);
            uint64_t h = 0xCBF29CE484222325ull;           // FNV-1a over dist2, nearest and reach
            auto eat = [&h](const void* p, size_t bytes) { const unsigned char* b = (const unsigned char*)p; for (size_t k = 0; k < bytes; k++) { h ^= b[k]; h *= 0x100000001B3ull; } };
            eat(d2.data(), d2.size() * 4); eat(nearest.data(), nearest.size() * 4); eat(reach.data(), reach.size());
            cout << " clearance_blocked " << K.counts.blocked << " clearance_traversable " << K.counts.traversable << " clearance_reachable " << K.counts.reachable << " clearance_max_d2 "
                 << K.counts.max_d2_reachable << " clearance_fnv " << hex << h << dec;
        }
        if (route) {          // (the viewer thread routed right after the clearance map as it ended; these fields come after every other, the clearance map's included)
            if (mapper.viewerFailed) { cerr << "exp_mapping: the viewer stopped before the route field was made" << endl; return 3; }
            const Mapper::RouteInfo& R = mapper.routeInfo();
            vector<uint32_t> cost; vector<int32_t> parent;
            mapper.routeFetch(&cost, &parent);
            const vector<int32_t>& path = mapper.routePath();
            uint64_t h = 0xCBF29CE484222325ull;           // FNV-1a over cost, parent and the path
            auto eat = [&h](const void* p, size_t bytes) { const unsigned char* b = (const unsigned char*)p; for (size_t k = 0; k < bytes; k++) { h ^= b[k]; h *= 0x100000001B3ull; } };
            eat(cost.data(), cost.size() * 4); eat(parent.data(), parent.size() * 4); eat(path.data(), path.size() * 4);
            cout << " route_routed " << R.counts.routed << " route_max_cost " << R.counts.max_cost << " route_path_len " << R.path.len << " route_path_cost " << R.path.cost << " route_fnv "
                 << hex << h << dec;
        }
        cout << endl;
    } catch (const exception& e) { cerr << RED << "exp_mapping: " << e.what() << RESET << endl; return 2; }
    return 0;
}

// one rank of `--ranks N` (its own process, its own GPU)
static int run_rank(ParameterReader& parameterReader, int rank, int nranks, const string& id_dir)
{
    ssm::default_device() = rank;
    VisualOdometryStereo::parameters voparam;
    voparam.calib.f = parameterReader.getData<double>("camera.fx"); voparam.calib.cu = parameterReader.getData<double>("camera.cx");
    voparam.calib.cv = parameterReader.getData<double>("camera.cy"); voparam.base = parameterReader.getData<double>("camera.baseline", 0.0);
    voparam.inlier_threshold = parameterReader.getData<double>("inlier_threshold", 6.0);
    const int first = parameterReader.getData<int>("start_index", 0), last = parameterReader.getData<int>("end_index", 100), total = last - first;
    const int R = parameterReader.getData<int>("tracker_ref_frames", 5);
    const int base = total / nranks, rem = total % nranks;                       // contiguous blocks, earlier ranks take the remainder (sharding.frame_block)
    const int lo = first + rank * base + min(rank, rem), hi = lo + base + (rank < rem ? 1 : 0);
    const int halo_lo = max(first, lo - R);
    Tracker::Ptr tracker(new Tracker(parameterReader, voparam));
    const FrameReader::DATASET type = dataset_type(parameterReader);
    FrameReader frameReader(parameterReader, type);
    const bool use_gt_pose = parameterReader.getData<int>("use_stream_pose", (type == FrameReader::TUM || type == FrameReader::KITTI) ? 0 : 1) != 0;
    PoseGraph poseGraph(parameterReader, tracker);
    Mapper mapper(parameterReader, poseGraph);
    auto t0 = chrono::steady_clock::now();
    int nframes = 0;
    for (int i = halo_lo; i < hi; i++) {
        RGBDFrame::Ptr frame = frameReader.get(i);
        if (!frame) break;
        Eigen::Isometry3d gt = frame->T_f_w;
        tracker->updateFrame(frame);
        if (use_gt_pose) frame->setTransform(gt);
        if (i < lo) continue;                                                   // halo frame: the previous rank maps it
        poseGraph.tryInsertKeyFrame(frame);
        nframes++;
    }
    const double loop_s = chrono::duration<double>(chrono::steady_clock::now() - t0).count();
    poseGraph.shutdown();
    this_thread::sleep_for(chrono::milliseconds(parameterReader.getData<int>("mapper_drain_ms", 300)));
    mapper.shutdown();
    // ---- the merge: this rank's key-frame clouds into one context map, then ONE all-gather of the voxel tables
    ssm_config cfg = parameterReader.deviceConfig(frameReader.width, frameReader.height);
    ssm::Device dev(cfg);
    unsigned char id[SSM_COMM_ID_BYTES];
    const string id_path = id_dir + "/nccl_id";
    if (rank == 0) {
        dev.check(ssm_comm_get_unique_id(id), "ssm_comm_get_unique_id");
        const string tmp = id_path + ".tmp";
        FILE* f = fopen(tmp.c_str(), "wb");
        if (!f || fwrite(id, 1, sizeof(id), f) != sizeof(id) || fclose(f) || rename(tmp.c_str(), id_path.c_str())) throw runtime_error("cannot publish the communicator id in " + id_dir);
    } else {
        for (;;) {                                                               // the parent kills this process if rank 0 dies first
            FILE* f = fopen(id_path.c_str(), "rb");
            if (f) { const size_t got = fread(id, 1, sizeof(id), f); fclose(f); if (got == sizeof(id)) break; }
            this_thread::sleep_for(chrono::milliseconds(2));
        }
    }
    dev.check(ssm_comm_init_rank(dev.ctx(), nranks, rank, id), "ssm_comm_init_rank");
    size_t local_points = 0;
    for (RGBDFrame::Ptr& kf : poseGraph.keyframes) {
        Mapper::PointCloud::Ptr c = mapper.generatePointCloud(kf);
        local_points += c->points.size();
        dev.check(ssm_map_insert(dev.ctx(), reinterpret_cast<const ssm_point*>(c->points.data()), (int)c->points.size()), "ssm_map_insert");
    }
    dev.check(ssm_voxel_allgather(dev.ctx(), nullptr), "ssm_voxel_allgather");
    int nvox = 0; dev.check(ssm_map_size(dev.ctx(), &nvox), "ssm_map_size");
    vector<ssm_point> merged((size_t)max(nvox, 1));
    dev.check(ssm_map_export(dev.ctx(), merged.data(), (int)merged.size(), &nvox), "ssm_map_export");
    uint64_t h = 0xCBF29CE484222325ull;                                          // FNV-1a of the merged map: identical on every rank and for every N
    for (int i = 0; i < nvox; i++) { const unsigned char* b = (const unsigned char*)&merged[i]; for (int k = 0; k < 24; k++) { h ^= b[k]; h *= 0x100000001B3ull; } }
    dev.check(ssm_comm_finalize(dev.ctx()), "ssm_comm_finalize");
    cout << "rank " << rank << "/" << nranks << " frames [" << lo << "," << hi << ") halo " << lo - halo_lo << " keyframes " << poseGraph.keyframes.size() << " local_points " << local_points
         << " merged_voxels " << nvox << " map_fnv " << hex << h << dec << " host_loop_fps " << nframes / loop_s << endl;
    const string out = parameterReader.getData<string>("map_output", string(""));
    if (rank == 0 && !out.empty()) {
        Mapper::PointCloud pc; pc.points.resize(nvox); memcpy((void*)pc.points.data(), merged.data(), (size_t)nvox * sizeof(ssm_point)); pc.width = nvox;
        Mapper::writePCD(out, pc);
    }
    return 0;
}
