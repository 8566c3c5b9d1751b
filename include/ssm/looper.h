// ssm/looper.h -- rgbd_tutor::Looper (reference include/looper.h, src/looper.cpp): the DBoW2 bag-of-words loop detector, same constructor and methods.
// add() computes frame->bowVec (vocab.transform; the FeatureVector the reference computes and drops is not built), getPossibleLoops() scores the frame against
// every stored frame: score > min_sim_score && abs(pf->id - frame->id) > min_interval, in database order.  When the calling thread has a device context (the one
// its OrbFeature used last) the vectors and scores come from the device looper of libssm_hip.so (ssm_looper_*), otherwise from the host functions
// (ssm_vocab_transform_host / ssm_bow_score_host); both run the arithmetic of include/ssm/looper_core.h and give the same bits.
// BatchLooper is the bulk form for BatchTracker: the key-frames of a chunk go from the chunk's device descriptors (ssm_seq_out_dev) into the database and
// their candidates come back from one query.
#pragma once
#include "common_headers.h"
#include "device.h"
#include "orb.h"
#include "rgbdframe.h"
namespace rgbd_tutor {
namespace looper_detail {
inline ssm_vocab* load_vocab(const ParameterReader& para) {
    const string vocab_file = para.getData<string>("looper_vocab_file");
    ssm_vocab* v = nullptr;
    const int rc = ssm_vocab_load_text(vocab_file.c_str(), &v);
    if (rc != SSM_OK) throw ssm::DeviceError(rc, string("Looper: ") + ssm_last_error(nullptr));
    return v;
}
}  // namespace looper_detail
class Looper {
public:
    Looper(const ParameterReader& para) : parameterReader(para) {
        cout << "loading vocabulary file, this may take a while..." << endl;
        vocab = looper_detail::load_vocab(para);
        cout << "load ok." << endl;
        min_sim_score = para.getData<float>("looper_min_sim_score", min_sim_score);
        min_interval = para.getData<float>("looper_min_interval", min_interval);
        on_device = para.getData<int>("looper_device", 1) != 0;          // (not a reference parameter) 0: always the host path; same bits either way
    }
    ~Looper() { if (dl) ssm_looper_destroy(dl); ssm_vocab_destroy(vocab); }
    Looper(const Looper&) = delete; Looper& operator=(const Looper&) = delete;
    void add(RGBDFrame::Ptr& frame) {
        cv::Mat desps = frame->getAllDescriptors();
        const int n = desps.rows;
        if (frames.empty() && !dl && on_device && OrbFeature::lastDevice()) {     // the database lives in ONE context: the one this thread has when the first frame arrives
            dev = OrbFeature::lastDevice();
            dev->check(ssm_looper_create(dev->ctx(), vocab, &dl), "ssm_looper_create");
        }
        vector<int32_t> ids((size_t)n + 1); vector<double> vals((size_t)n + 1); int m = 0;
        if (dl) {
            dev->check(ssm_looper_add(dl, desps.data, n, frame->id), "ssm_looper_add");
            dev->check(ssm_looper_bow(dl, ssm_looper_size(dl) - 1, ids.data(), vals.data(), n, &m), "ssm_looper_bow");
            entry_of[frame.get()] = ssm_looper_size(dl) - 1;
        } else {
            const int rc = ssm_vocab_transform_host(vocab, desps.data, n, nullptr, ids.data(), vals.data(), n, &m);
            if (rc != SSM_OK) throw ssm::DeviceError(rc, "ssm_vocab_transform_host");
        }
        frame->bowVec.clear();
        for (int i = 0; i < m; i++) frame->bowVec.emplace_hint(frame->bowVec.end(), (unsigned)ids[i], vals[i]);
        frames.push_back(frame);
    }
    vector<RGBDFrame::Ptr> getPossibleLoops(const RGBDFrame::Ptr& frame) {
        vector<RGBDFrame::Ptr> result;
        const size_t nf = frames.size();
        last_scores.assign(nf, 0.0); last_indices.clear();
        auto it = dl ? entry_of.find(frame.get()) : entry_of.end();
        if (it != entry_of.end()) { if (nf) dev->check(ssm_looper_scores(dl, it->second, (int)nf, last_scores.data()), "ssm_looper_scores"); }
        else {                                                  // the host path (also a frame that was never added: the reference scores whatever bowVec it carries)
            vector<int32_t> qi, pi; vector<double> qv, pv; flatten(frame->bowVec, qi, qv);
            for (size_t i = 0; i < nf; i++) { flatten(frames[i]->bowVec, pi, pv); ssm_bow_score_host(qi.data(), qv.data(), (int)qi.size(), pi.data(), pv.data(), (int)pi.size(), &last_scores[i]); }
        }
        for (size_t i = 0; i < nf; i++) {
            RGBDFrame::Ptr pf = frames[i];
            if (last_scores[i] > min_sim_score && abs(pf->id - frame->id) > min_interval) { result.push_back(pf); last_indices.push_back((int)i); }
        }
        return result;
    }
    void save() {}
    void load() {}
    bool onDevice() const { return dl != nullptr; }
    const RGBDFrame::Ptr& frameAt(int i) const { return frames[i]; }     // database entry i (not in the reference's class)
    vector<double> last_scores;                   // of the most recent getPossibleLoops: score(frame, frames[i]) (not in the reference's class)
    vector<int> last_indices;                     // and the database index i of every frame it returned
protected:
    static void flatten(const BowVector& b, vector<int32_t>& ids, vector<double>& vals) { ids.clear(); vals.clear(); for (auto& kv : b) { ids.push_back((int32_t)kv.first); vals.push_back(kv.second); } }
    ssm_vocab* vocab = nullptr;
    ssm_looper* dl = nullptr; ssm::Device* dev = nullptr; map<const RGBDFrame*, int> entry_of;
    vector<RGBDFrame::Ptr> frames;
    const ParameterReader& parameterReader;
    float min_sim_score = 0.01;
    float min_interval = 10;
    bool on_device = true;
};

// Looper::add + Looper::getPossibleLoops for the key-frames of a BatchTracker chunk, in bulk: the descriptors stay on the device
class BatchLooper {
public:
    struct Candidate { RGBDFrame::Ptr frame, loop; double score; };
    BatchLooper(const ParameterReader& para, ssm::Device& device) : dev(device) {
        ssm_vocab* v = looper_detail::load_vocab(para);
        const int rc = ssm_looper_create(dev.ctx(), v, &dl);
        ssm_vocab_destroy(v);
        dev.check(rc, "ssm_looper_create");
        min_sim_score = para.getData<float>("looper_min_sim_score", min_sim_score);
        min_interval = para.getData<float>("looper_min_interval", min_interval);
    }
    ~BatchLooper() { if (dl) ssm_looper_destroy(dl); }
    BatchLooper(const BatchLooper&) = delete; BatchLooper& operator=(const BatchLooper&) = delete;
    // out / done: a flush's device tables and its frames (BatchTracker::last_out, the vector flush() returned); picked: ascending indices into done (the key-frames).
    // Every run of consecutive picked frames is one ssm_looper_add_dev; one ssm_looper_query then gives what add + getPossibleLoops per key-frame would
    vector<Candidate> addChunk(const ssm_seq_out_dev& out, const vector<RGBDFrame::Ptr>& done, const vector<int>& picked) {
        vector<Candidate> res;
        if (picked.empty()) return res;
        const int first = ssm_looper_size(dl);
        for (size_t a = 0; a < picked.size();) {
            size_t b = a + 1; while (b < picked.size() && picked[b] == picked[b - 1] + 1) b++;
            vector<int32_t> ids; for (size_t k = a; k < b; k++) { ids.push_back(done[picked[k]]->id); frames.push_back(done[picked[k]]); }
            dev.check(ssm_looper_add_dev(dl, out.desc + (size_t)picked[a] * out.cap * 32, out.nkp + picked[a], (int)(b - a), out.cap, ids.data()), "ssm_looper_add_dev");
            a = b;
        }
        const int n = (int)picked.size();
        vector<int32_t> pairs(2 * 1024); vector<double> sc(1024); int m = 0;
        int rc = ssm_looper_query(dl, first, n, -1, (double)min_sim_score, (int)floorf(min_interval), pairs.data(), sc.data(), (int)sc.size(), &m);
        if (rc == SSM_E_CAPACITY) { pairs.resize((size_t)2 * m); sc.resize(m); rc = ssm_looper_query(dl, first, n, -1, (double)min_sim_score, (int)floorf(min_interval), pairs.data(), sc.data(), (int)sc.size(), &m); }
        dev.check(rc, "ssm_looper_query");
        for (int i = 0; i < m; i++) res.push_back(Candidate{frames[pairs[2 * i]], frames[pairs[2 * i + 1]], sc[i]});
        return res;
    }
    int size() const { return ssm_looper_size(dl); }
protected:
    ssm::Device& dev; ssm_looper* dl = nullptr; vector<RGBDFrame::Ptr> frames;
    float min_sim_score = 0.01;
    float min_interval = 10;
};
}  // namespace rgbd_tutor
