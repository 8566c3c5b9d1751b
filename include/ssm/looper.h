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
// Vocabulary training (not in the reference, which loads ORBvoc.txt): a hierarchical k-majority tree from the descriptors of a sequence's
// key-frames (desc_sets[f]: 32 bytes per descriptor of key-frame f), with looper_train_k / looper_train_L / looper_train_iters (10 / 5 / 32), written to
// `file` in the text format looper_vocab_file names.  dev: the device trainer of that context; null: the host function -- the same bytes either way.
struct TrainedVocabulary { int nodes = 0, words = 0; uint64_t fnv = 0; ssm_vocab_train_report report{}; };      // fnv: FNV-1a over the exported parent, is_leaf, descriptor and weight arrays
inline TrainedVocabulary trainVocabulary(const ParameterReader& para, const vector<vector<uint8_t>>& desc_sets, ssm::Device* dev, const string& file) {
    ssm_vocab_train_params p; ssm_vocab_train_params_default(&p);
    p.k = para.getData<int>("looper_train_k", p.k); p.L = para.getData<int>("looper_train_L", p.L); p.max_iters = para.getData<int>("looper_train_iters", p.max_iters);
    vector<uint8_t> all; vector<int32_t> npf;
    for (const vector<uint8_t>& d : desc_sets) { npf.push_back((int32_t)(d.size() / 32)); all.insert(all.end(), d.begin(), d.begin() + (d.size() / 32) * 32); }
    TrainedVocabulary tv; ssm_vocab* v = nullptr;
    if (all.empty()) throw ssm::DeviceError(SSM_E_INVAL, "trainVocabulary: no descriptors (no key-frame was accepted)");
    const int rc = dev ? ssm_vocab_train(dev->ctx(), all.data(), npf.data(), (int)npf.size(), &p, nullptr, &tv.report, &v)
                       : ssm_vocab_train_host(all.data(), npf.data(), (int)npf.size(), &p, nullptr, &tv.report, &v);
    if (rc != SSM_OK) throw ssm::DeviceError(rc, string("trainVocabulary: ") + ssm_last_error(dev ? dev->ctx() : nullptr));
    int32_t info[6]; ssm_vocab_info(v, info);
    tv.nodes = info[2]; tv.words = info[3];
    const int n = tv.nodes - 1;
    vector<int32_t> parent((size_t)n); vector<uint8_t> leaf((size_t)n), desc((size_t)n * 32); vector<double> weight((size_t)n);
    int rc2 = ssm_vocab_export(v, parent.data(), leaf.data(), desc.data(), weight.data(), n);
    uint64_t h = 0xCBF29CE484222325ull;
    auto eat = [&h](const void* q, size_t bytes) { const unsigned char* b = (const unsigned char*)q; for (size_t i = 0; i < bytes; i++) { h ^= b[i]; h *= 0x100000001B3ull; } };
    eat(parent.data(), (size_t)n * 4); eat(leaf.data(), (size_t)n); eat(desc.data(), (size_t)n * 32); eat(weight.data(), (size_t)n * 8);
    tv.fnv = h;
    if (rc2 == SSM_OK) rc2 = ssm_vocab_save_text(v, file.c_str());
    ssm_vocab_destroy(v);
    if (rc2 != SSM_OK) throw ssm::DeviceError(rc2, string("trainVocabulary: ") + ssm_last_error(nullptr));
    return tv;
}
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
