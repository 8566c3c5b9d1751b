// test_posegraph -- rgbd_tutor::PoseGraph with pose_graph_optimize=1 (include/ssm/pose_graph.h) on a synthetic sequence that revisits its start: the frames of the
// seeded stream forwards, then the same images backwards under new ids, every pose pushed off by a drift that grows with the frame's position.  step() runs after
// every accepted key-frame, as exp_mapping --optimize does.  Usage: test_posegraph <parameters> <vocabulary.txt> <scratch directory>.  Device calls (ORB, matcher):
// runs under -m gpu; the optimiser itself runs wherever PoseGraph puts it (the device when pose_graph_device=1).
// `test_posegraph --graph-only <parameters>` makes no device call: the gate with the graph behind it (vertices, state edges, save) and the optimiser's host
// function on a drifting circle with a loop edge.  That is what the host layer's sanitizer builds run (scripts/run_sanitizers.sh).
#include "ssm/rgbdframe.h"
#include "ssm/pose_graph.h"
#include <cstdio>
using namespace std;
using namespace rgbd_tutor;

static int g_fail = 0;
#define CHECK(name, cond) do { if (cond) printf("PASS %s\n", name); else { printf("FAIL %s (%s:%d)\n", name, __FILE__, __LINE__); g_fail++; } } while (0)

#ifndef SSM_POSEGRAPH_GRAPH_ONLY          // (the sanitizer builds link a stub instead of the library: the part with device calls is left out there)
static RGBDFrame::Ptr revisit(const RGBDFrame::Ptr& f, int id)
{
    RGBDFrame::Ptr g(new RGBDFrame);
    g->id = id; g->rgb = f->rgb.clone(); g->depth = f->depth.clone(); g->semantic = f->semantic.clone(); g->camera = f->camera; g->T_f_w = f->T_f_w;
    return g;
}
static double pose_diff(const Eigen::Isometry3d& a, const Eigen::Isometry3d& b) { double m = 0; for (int k = 0; k < 16; k++) m = max(m, fabs(a.data()[k] - b.data()[k])); return m; }

static int run(ParameterReader& para, const string& scratch, bool device)
{
    para.set("pose_graph_optimize", "1"); para.set("pose_graph_device", device ? "1" : "0");
    const int n = 12;
    para.set("start_index", "0"); para.set("end_index", to_string(n));
    VisualOdometryStereo::parameters voparam;
    Tracker::Ptr tracker(new Tracker(para, voparam));
    FrameReader reader(para, FrameReader::SYNTHETIC);
    PoseGraph pg(para, tracker);
    vector<RGBDFrame::Ptr> seq;
    while (RGBDFrame::Ptr f = reader.next()) seq.push_back(f);
    CHECK("stream_frames", (int)seq.size() == n);
    for (int k = n - 1; k >= 0; k--) seq.push_back(revisit(seq[k], 2 * n - 1 - k));
    vector<Eigen::Isometry3d> at_insert; int steps_that_optimised = 0;
    for (size_t k = 0; k < seq.size(); k++) {
        RGBDFrame::Ptr f = seq[k];
        Eigen::Isometry3d T = f->T_f_w;
        tracker->updateFrame(f);
        T(0, 3) += 0.004 * (double)k; T(2, 3) -= 0.002 * (double)k;          // the drift: the revisit does not come back to where it started
        f->setTransform(T);
        if (pg.tryInsertKeyFrame(f)) { at_insert.push_back(f->getTransform()); if (pg.step()) steps_that_optimised++; }
    }
    printf("%s: keyframes %zu vertices %d edges %d nearby %d loop %d candidates %zu opts %d + %d adjust %d (%d ok)\n", device ? "device" : "host", pg.keyframes.size(), pg.graphVertices(),
           pg.graphEdges(), pg.nearbyEdges, pg.loopEdges, pg.loopCandidates.size(), pg.globalOpts, pg.localOpts, pg.adjustCalls, pg.adjusted);
    CHECK("optimiser_where_asked", pg.onDevice() == device);
    CHECK("a_vertex_per_keyframe", pg.graphVertices() == (int)pg.keyframes.size() && pg.keyframes.size() > 12);
    CHECK("state_edge_per_keyframe_plus_the_rest", pg.graphEdges() == (int)pg.keyframes.size() - 1 + pg.nearbyEdges + pg.loopEdges);
    CHECK("nearby_edges_added", pg.nearbyEdges > 0);
    CHECK("loop_candidates_and_edges_added", !pg.loopCandidates.empty() && pg.loopEdges > 0);
    CHECK("optimised_at_least_once", pg.globalOpts + pg.localOpts >= 1 && steps_that_optimised == pg.globalOpts + pg.localOpts);
    CHECK("report_of_the_last_optimise", pg.lastReport.iterations >= 1 && pg.lastReport.active_edges > 0);
    CHECK("adjust_called", pg.adjustCalls == pg.globalOpts + pg.localOpts && pg.adjustCalls >= 1 && tracker->hasCurrentFrame());      // (the per-frame tracker has a current frame: Tracker::adjust itself ran)
    CHECK("adjust_reanchored_the_current_frame", pg.adjusted >= 1);
    double moved = 0; for (size_t i = 0; i < pg.keyframes.size(); i++) moved = max(moved, pose_diff(pg.keyframes[i]->getTransform(), at_insert[i]));
    CHECK("a_keyframe_pose_changed", moved > 1e-6);
    CHECK("the_first_keyframe_is_fixed", pose_diff(pg.keyframes[0]->getTransform(), at_insert[0]) == 0);
    CHECK("edge_bookkeeping", pg.isEdgeExist(pg.keyframes[1]->id, pg.keyframes[0]->id) && pg.isEdgeExist(pg.keyframes[0]->id, pg.keyframes[1]->id) && pg.isEdgeExist(7, 7) && !pg.isEdgeExist(0, 1000));
    const string path = scratch + (device ? "/traj_device.g2o" : "/traj_host.g2o");
    pg.save(path);
    ssm_pgo* back = nullptr; int nv = 0, ne = 0;
    CHECK("g2o_loads_back", ssm_pgo_create(nullptr, &back) == SSM_OK && ssm_pgo_load_g2o(back, path.c_str(), 1) == SSM_OK && ssm_pgo_size(back, &nv, &ne) == SSM_OK
                            && nv == pg.graphVertices() && ne == pg.graphEdges());
    ssm_pgo_destroy(back);
    uint64_t h = 0xCBF29CE484222325ull;
    for (auto& kf : pg.keyframes) { const Eigen::Isometry3d T = kf->getTransform(); const unsigned char* b = (const unsigned char*)T.data(); for (int k = 0; k < 128; k++) { h ^= b[k]; h *= 0x100000001B3ull; } }
    printf("kf_pose_fnv %llx\n", (unsigned long long)h);
    return (int)(h & 0x7fffffff);
}

#endif
// no device call: PoseGraph's bookkeeping and ssm_pgo_optimize_host
static void graph_only(const char* parameters)
{
    ParameterReader para(parameters);
    para.set("pose_graph_optimize", "1"); para.set("pose_graph_device", "0"); para.set("nearby_keyframes", "0"); para.set("keyframe_min_translation", "0.5");
    VisualOdometryStereo::parameters voparam;
    Tracker::Ptr tracker(new Tracker(para, voparam));
    PoseGraph pg(para, tracker);
    for (int k = 0; k < 9; k++) { RGBDFrame::Ptr f(new RGBDFrame); f->id = 10 + k; f->T_f_w(0, 3) = 0.3 * k; pg.tryInsertKeyFrame(f); }       // every second frame passes the gate
    CHECK("graph_only_vertices_and_state_edges", pg.keyframes.size() == 5 && pg.graphVertices() == 5 && pg.graphEdges() == 4 && pg.newFrames.size() == 4 && !pg.onDevice());
    CHECK("graph_only_edge_lookup", pg.isEdgeExist(10, 12) && pg.isEdgeExist(12, 10) && !pg.isEdgeExist(10, 14));
    CHECK("graph_only_step_without_neighbours", !pg.step() && pg.newFrames.empty() && pg.globalOpts + pg.localOpts == 0);
    // the optimiser's host function: twelve poses on a circle, the chain drifts, one loop edge says where the last one really is
    ssm_pgo* g = nullptr;
    CHECK("graph_only_create", ssm_pgo_create(nullptr, &g) == SSM_OK);
    const int n = 12; vector<Eigen::Isometry3d> truth(n), est(n);
    for (int k = 0; k < n; k++) {
        const double a = 2 * M_PI * k / n, c = cos(a + M_PI / 2), s = sin(a + M_PI / 2);
        Eigen::Isometry3d T; T(0, 0) = c; T(0, 1) = -s; T(1, 0) = s; T(1, 1) = c; T(0, 3) = 10 * cos(a); T(1, 3) = 10 * sin(a);
        truth[k] = T; est[k] = T; est[k](0, 3) += 0.05 * k; est[k](2, 3) += 0.02 * k;
        ssm_pgo_add_vertex(g, k, est[k].data(), k == 0);
    }
    for (int k = 1; k < n; k++) { const Eigen::Isometry3d Z = est[k - 1].inverse() * est[k]; ssm_pgo_add_edge(g, k - 1, k, Z.data(), nullptr, 1); }
    for (int k = 2; k < n; k++) { const Eigen::Isometry3d Z = truth[k - 2].inverse() * truth[k]; ssm_pgo_add_edge(g, k - 2, k, Z.data(), nullptr, 1); }
    { const Eigen::Isometry3d Z = truth[n - 1].inverse() * truth[0]; ssm_pgo_add_edge(g, n - 1, 0, Z.data(), nullptr, 1); }
    ssm_pgo_report rep;
    CHECK("graph_only_optimize_host", ssm_pgo_optimize_host(g, 10, &rep) == SSM_OK && rep.iterations >= 2 && rep.active_vertices == n - 1 && rep.chi2_after[rep.iterations - 1] < 0.1 * rep.chi2_before[0]);
    ssm_pgo_set_mode(g, 1);
    CHECK("graph_only_local_mode", ssm_pgo_optimize_host(g, 3, &rep) == SSM_OK && rep.active_vertices == 5);
    double x[36], H[72 * 2], b[12]; int32_t first[2] = {0, 0}; int ok = 0;
    for (int i = 0; i < 144; i++) H[i] = 0;
    for (int i = 0; i < 12; i++) { b[i] = 1 + i; H[i < 6 ? 6 * i + i : 36 + 12 * (i - 6) + i] = 2 + i; }
    CHECK("graph_only_factor_solve", ssm_pgo_factor_solve(g, 0, 2, first, H, b, 0.0, x, &ok) == SSM_OK && ok == 1 && x[0] == 0.5 && x[11] == 12.0 / 13.0);
    ssm_pgo_destroy(g);
}

int main(int argc, char** argv)
{
    if (argc == 3 && string(argv[1]) == "--graph-only") {
        try { graph_only(argv[2]); } catch (const exception& e) { printf("FAIL exception: %s\n", e.what()); g_fail++; }
        printf(g_fail ? "%d FAILED\n" : "ALL PASSED\n", g_fail);
        return g_fail ? 1 : 0;
    }
#ifdef SSM_POSEGRAPH_GRAPH_ONLY
    fprintf(stderr, "usage: %s --graph-only <parameters>\n", argv[0]); return 2;
#else
    if (argc < 4) { fprintf(stderr, "usage: %s <parameters> <vocabulary.txt> <scratch directory>\n", argv[0]); return 2; }
    try {
        ParameterReader para(argv[1]);
        para.set("looper_vocab_file", argv[2]); para.set("looper_min_sim_score", "0.05"); para.set("looper_min_interval", "3");
        para.set("nearby_keyframes", "3"); para.set("loop_accumulate_error", "4.0"); para.set("local_accumulate_error", "1.0");
        {   // the switch off: the class as it was
            ParameterReader off(argv[1]);
            VisualOdometryStereo::parameters voparam;
            Tracker::Ptr tracker(new Tracker(off, voparam));
            PoseGraph pg(off, tracker);
            RGBDFrame::Ptr a(new RGBDFrame), b(new RGBDFrame); a->id = 0; b->id = 1; b->T_f_w(0, 3) = 1.0;
            CHECK("off_gate_still_works", pg.tryInsertKeyFrame(a) && pg.tryInsertKeyFrame(b) && pg.keyframes.size() == 2);
            CHECK("off_no_graph_no_step", !pg.optimizing() && pg.graphVertices() == 0 && pg.graphEdges() == 0 && pg.newFrames.empty() && !pg.step() && !pg.looper && !pg.pnp);
        }
        const int hd = run(para, argv[3], true);
        const int hh = run(para, argv[3], false);
        CHECK("device_and_host_optimiser_give_the_same_keyframe_poses", hd == hh);
    } catch (const exception& e) { printf("FAIL exception: %s\n", e.what()); g_fail++; }
    printf(g_fail ? "%d FAILED\n" : "ALL PASSED\n", g_fail);
    return g_fail ? 1 : 0;
#endif
}
