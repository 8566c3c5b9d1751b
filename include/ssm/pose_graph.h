// ssm/pose_graph.h -- rgbd_tutor::PoseGraph (reference include/pose_graph.h, src/pose_graph.cpp): the keyframe gate and the shared `keyframes` list, and --
// behind pose_graph_optimize=1 (not a reference parameter; 0, the default, is the class as it was: no vertex, no edge, no optimiser object) -- the graph the
// reference keeps in g2o: vertices and edges in an ssm_pgo object (include/ssm/pgo_core.h), step() = one pass of mainLoop's body
// (pose_graph.cpp:96-302): nearby edges by solvePnPLazy, Looper::add + getPossibleLoops -> loop edges, the local / loop chi2 accumulators, the global or local
// optimize(10) against loop_accumulate_error / local_accumulate_error, setTransform on the key-frames, refFrame = keyframes.back(), Tracker::adjust.
// mainLoop() is the reference's thread body around step(); the constructor does not start it (exp_mapping --optimize calls step() synchronously, so that a run
// is reproducible).  The stereo override inside mainLoop (QuadFeatureMatch with DES_SIFT) is not built: edges carry info.T of PnP.  The optimiser runs on the
// device when the thread has a context (pose_graph_device=1, the default) and on the host otherwise: the same bits.  shutdown() sets the flag Mapper::viewer
// reads and wakes mainLoop.
#pragma once
#include "common_headers.h"
#include <atomic>
#include <condition_variable>
#include "track.h"
#include "looper.h"
namespace rgbd_tutor {
class PoseGraph {
public:
    typedef map<int, int> EdgeID;
    struct LoopCandidate { int frame, loop; double score; };
    PoseGraph(const ParameterReader& para, shared_ptr<Tracker>& t) : parameterReader(para), tracker(t) {
        keyframe_min_translation = para.getData<double>("keyframe_min_translation", 5.5);
        keyframe_min_rotation = para.getData<double>("keyframe_min_rotation", 2.5);
        optimize_on = para.getData<int>("pose_graph_optimize", 0) != 0;
        if (!optimize_on) return;
        nearbyFrames = para.getData<int>("nearby_keyframes", 5);
        loopAccuError = para.getData<double>("loop_accumulate_error", 4.0);
        localAccuError = para.getData<double>("local_accumulate_error", 1.0);
        use_device = para.getData<int>("pose_graph_device", 1) != 0;
        pnp = make_shared<PnPSolver>(para, *tracker->orbFeature());
        if (!para.getData<string>("looper_vocab_file", string("")).empty()) looper = make_shared<Looper>(para);
    }
    ~PoseGraph() { if (pgo) ssm_pgo_destroy(pgo); }
    PoseGraph(const PoseGraph&) = delete; PoseGraph& operator=(const PoseGraph&) = delete;
    // pose_graph.cpp:11-77: first frame always; afterwards when the motion w.r.t. the last keyframe is large enough
    bool tryInsertKeyFrame(RGBDFrame::Ptr& frame) {
        lastFrame = frame;
        if (keyframes.size() == 0) {
            unique_lock<mutex> lck(keyframes_mutex); keyframes.push_back(frame); refFrame = frame;
            if (optimize_on) { addVertex(frame->id, frame->T_f_w, true); vertexIdx.push_back(frame->id); }
            return true;
        }
        Eigen::Isometry3d delta = frame->getTransform().inverse() * refFrame->getTransform();
        if (norm_translate(delta) > keyframe_min_translation || norm_rotate(delta) > keyframe_min_rotation) {
            unique_lock<mutex> lck(keyframes_mutex);
            if (optimize_on) {
                newFrames.push_back(frame);
                addVertex(frame->id, frame->getTransform(), false); vertexIdx.push_back(frame->id);
            }
            keyframes.push_back(frame);
            if (optimize_on) {                                 // the edge to refFrame "from state": the tracker's own estimate (vertex 0 = the new frame, as the reference sets it)
                addEdge(frame->id, refFrame->id, frame->getTransform().inverse() * refFrame->getTransform());
                EdgeID id; id[refFrame->id] = frame->id; edges[id] = nEdges - 1;
            }
            refFrame = frame;
            if (optimize_on) keyframe_updated.notify_one();
            return true;
        }
        return false;
    }
    // one pass of mainLoop's body over the key-frames inserted since the last pass.  Returns true when it optimised
    bool step() {
        if (!optimize_on) return false;
        unique_lock<mutex> lck(keyframes_mutex);
        vector<RGBDFrame::Ptr> newFrames_copy = newFrames;
        newFrames.clear();
        for (auto nf : newFrames_copy) {
            for (int i = 0; i < nearbyFrames; i++) {
                const int idx = (int)keyframes.size() - i - 2;
                if (idx < 0) break;
                RGBDFrame::Ptr pf = keyframes[idx];
                if (isEdgeExist(nf->id, pf->id)) continue;
                ensureFeatures(nf); ensureFeatures(pf);
                PNP_INFORMATION info;
                if (pnp->solvePnPLazy(pf, nf, info, false) == false) continue;
                addEdge(nf->id, pf->id, info.T);
                localAccumulatedError += lastEdgeChi2();
                EdgeID id; id[nf->id] = pf->id; edges[id] = nEdges - 1;
                nearbyEdges++;
            }
            if (!looper) continue;
            ensureFeatures(nf);
            looper->add(nf);
            vector<RGBDFrame::Ptr> possibleLoops = looper->getPossibleLoops(nf);
            for (int i : looper->last_indices) loopCandidates.push_back({nf->id, looper->frameAt(i)->id, looper->last_scores[i]});
            for (auto pf : possibleLoops) {
                if (isEdgeExist(nf->id, pf->id)) continue;
                ensureFeatures(pf);
                PNP_INFORMATION info;
                if (pnp->solvePnPLazy(pf, nf, info, false) == true) {
                    addEdge(nf->id, pf->id, info.T);
                    EdgeID id; id[nf->id] = pf->id; edges[id] = nEdges - 1;
                    loopAccumulatedError += lastEdgeChi2();
                    loopEdges++;
                }
            }
        }
        bool doOptimize = false;
        if (loopAccumulatedError > loopAccuError) {
            optimize(false);
            for (auto kf : keyframes) applyEstimate(kf);
            localAccumulatedError = 0; loopAccumulatedError = 0; doOptimize = true; globalOpts++;
        } else if (localAccumulatedError > localAccuError) {
            optimize(true);
            for (int i = (int)keyframes.size() - 1; i > 0 && (size_t)i > keyframes.size() - 6; i--) applyEstimate(keyframes[i]);
            localAccumulatedError = 0; doOptimize = true; localOpts++;
        }
        if (doOptimize) {
            refFrame = keyframes.back();
            // Tracker::adjust re-anchors the tracker's current frame on refFrame; a bulk tracker has no current frame in `tracker`, and the same arithmetic then runs
            // here on the last frame that went through the gate (which is what the per-frame tracker's current frame is)
            if (tracker->hasCurrentFrame()) { adjustCalls++; if (tracker->adjust(refFrame)) adjusted++; }
            else if (lastFrame) {
                ensureFeatures(refFrame); ensureFeatures(lastFrame);
                PNP_INFORMATION info; adjustCalls++;
                if (pnp->solvePnPLazy(refFrame, lastFrame, info)) { lastFrame->setTransform(info.T * refFrame->getTransform()); adjusted++; }
            }
        }
        return doOptimize;
    }
    // the reference's thread body: waits for tryInsertKeyFrame's notification, then one step
    void mainLoop() {
        while (!shutDownFlag) {
            { unique_lock<mutex> lck(keyframe_updated_mutex); keyframe_updated.wait_for(lck, chrono::milliseconds(50)); }
            if (shutDownFlag) break;
            bool any; { unique_lock<mutex> lck(keyframes_mutex); any = !newFrames.empty(); }
            if (any) step();
        }
    }
    bool isEdgeExist(const int vertex1, const int vertex2) const {
        if (vertex1 == vertex2) return true;
        EdgeID e1, e2; e1[vertex1] = vertex2; e2[vertex2] = vertex1;
        return edges.find(e1) != edges.end() || edges.find(e2) != edges.end();
    }
    // optimizer.save(filename): the g2o text file (VERTEX_SE3:QUAT, FIX, EDGE_SE3:QUAT)
    void save(const string& filename) { if (pgo) check(ssm_pgo_save_g2o(pgo, filename.c_str()), "ssm_pgo_save_g2o"); }
    void shutdown() { shutDownFlag = true; keyframe_updated.notify_all(); }
    int graphVertices() const { return (int)vertexIdx.size(); }
    int graphEdges() const { return nEdges; }
    bool optimizing() const { return optimize_on; }
    bool onDevice() const { return pgo_dev != nullptr; }
    vector<RGBDFrame::Ptr> keyframes;
    vector<RGBDFrame::Ptr> newFrames;               // key-frames that step() has not seen yet
    mutex keyframes_mutex;
    std::atomic<bool> shutDownFlag{false};          // read by Mapper::viewer on its thread
    vector<int> vertexIdx;                          // vertex ids in insertion order
    map<EdgeID, int> edges;                         // -> the edge's number in the optimiser
    shared_ptr<Looper> looper = nullptr;            // null: no vocabulary configured, no loop edges
    shared_ptr<PnPSolver> pnp = nullptr;
    vector<LoopCandidate> loopCandidates;           // what getPossibleLoops returned, in order (exp_mapping's loop log)
    int nearbyEdges = 0, loopEdges = 0, globalOpts = 0, localOpts = 0;
    int adjustCalls = 0, adjusted = 0;              // Tracker::adjust (or its arithmetic on the last gated frame) was run / re-anchored the frame
    ssm_pgo_report lastReport{};
protected:
    void check(int rc, const char* what) { if (rc != SSM_OK) throw ssm::DeviceError(rc, string(what) + ": " + ssm_last_error(pgo_dev ? pgo_dev->ctx() : nullptr)); }
    void ensurePgo() {
        if (pgo) return;
        pgo_dev = use_device ? OrbFeature::lastDevice() : nullptr;     // the context this thread has when the first vertex arrives, or none: the host function
        check(ssm_pgo_create(pgo_dev ? pgo_dev->ctx() : nullptr, &pgo), "ssm_pgo_create");
    }
    void addVertex(int id, const Eigen::Isometry3d& T, bool fixed) { ensurePgo(); check(ssm_pgo_add_vertex(pgo, id, T.data(), fixed ? 1 : 0), "ssm_pgo_add_vertex"); }
    void addEdge(int from, int to, const Eigen::Isometry3d& Z) { check(ssm_pgo_add_edge(pgo, from, to, Z.data(), nullptr, 1), "ssm_pgo_add_edge"); nEdges++; }
    double lastEdgeChi2() { double c = 0; check(ssm_pgo_edge_chi2(pgo, nEdges - 1, &c), "ssm_pgo_edge_chi2"); return c; }
    void optimize(bool local) {
        check(ssm_pgo_set_mode(pgo, local ? 1 : 0), "ssm_pgo_set_mode");
        check(pgo_dev ? ssm_pgo_optimize(pgo, 10, &lastReport) : ssm_pgo_optimize_host(pgo, 10, &lastReport), "ssm_pgo_optimize");
        const int n = (int)vertexIdx.size(); int got = 0;
        est_ids.resize(n); est.resize((size_t)n * 16);
        check(ssm_pgo_get_poses(pgo, est_ids.data(), est.data(), n, &got), "ssm_pgo_get_poses");
        est_of.clear(); for (int i = 0; i < got; i++) est_of[est_ids[i]] = i;
    }
    void applyEstimate(const RGBDFrame::Ptr& kf) {
        auto it = est_of.find(kf->id);
        if (it == est_of.end()) return;
        Eigen::Isometry3d T; for (int k = 0; k < 16; k++) T.matrix().data()[k] = est[(size_t)it->second * 16 + k];
        kf->setTransform(T);
    }
    void ensureFeatures(RGBDFrame::Ptr& f) { if (f->features.empty()) tracker->orbFeature()->detectFeatures(f); }     // (a bulk tracker's frames carry no host features)
    const ParameterReader& parameterReader;
    shared_ptr<Tracker> tracker;
    RGBDFrame::Ptr refFrame, lastFrame;
    double keyframe_min_translation = 0.3, keyframe_min_rotation = 0.3;
    bool optimize_on = false, use_device = true;
    int nearbyFrames = 5, nEdges = 0;
    double loopAccuError = 4.0, localAccuError = 1.0, loopAccumulatedError = 0.0, localAccumulatedError = 0.0;
    ssm_pgo* pgo = nullptr; ssm::Device* pgo_dev = nullptr;
    vector<int32_t> est_ids; vector<double> est; map<int, int> est_of;
    mutex keyframe_updated_mutex; condition_variable keyframe_updated;
};
}  // namespace rgbd_tutor
