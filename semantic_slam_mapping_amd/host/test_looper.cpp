// test_looper -- rgbd_tutor::Looper (include/ssm/looper.h) on its HOST path: no device call (this thread never creates a context, so Looper::add takes
// ssm_vocab_transform_host and getPossibleLoops ssm_bow_score_host).  Usage: test_looper <scratch directory> [vocabulary.txt]
// The small vocabularies are written here; the optional second argument is a larger one written by the caller (tests/test_looper.py).
#include "ssm/looper.h"
#include <array>
#include <cstdio>
using namespace std;
using namespace rgbd_tutor;

static int g_fail = 0;
#define CHECK(name, cond) do { if (cond) printf("PASS %s\n", name); else { printf("FAIL %s (%s:%d)\n", name, __FILE__, __LINE__); g_fail++; } } while (0)

static uint32_t g_rng = 12345u;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }
static void rand_desc(uint8_t* d) { for (int i = 0; i < 32; i++) d[i] = (uint8_t)(rnd() & 255); }

static RGBDFrame::Ptr make_frame(int id, const vector<array<uint8_t, 32>>& desc)
{
    RGBDFrame::Ptr f(new RGBDFrame); f->id = id;
    for (auto& d : desc) { Feature ft; ft.descriptor.create(1, 32, CV_8UC1); memcpy(ft.descriptor.data, d.data(), 32); f->features.push_back(ft); }
    return f;
}
// a one-level vocabulary of two words: word 0 = all-zero bytes (weight w0), word 1 = all-255 bytes (weight w1)
static string write_two_words(const string& dir, double w0, double w1)
{
    const string path = dir + "/two_words.txt";
    FILE* f = fopen(path.c_str(), "w");
    fprintf(f, "2 1 0 0\n");
    for (int n = 0; n < 2; n++) { fprintf(f, "0 1"); for (int i = 0; i < 32; i++) fprintf(f, " %d", n ? 255 : 0); fprintf(f, " %.17g\n", n ? w1 : w0); }
    fclose(f);
    return path;
}
static vector<int> ids_of(const vector<RGBDFrame::Ptr>& v) { vector<int> r; for (auto& f : v) r.push_back(f->id); return r; }

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s <scratch directory> [vocabulary.txt]\n", argv[0]); return 2; }
    const string dir = argv[1];
    { FILE* f = fopen((dir + "/looper_params.txt").c_str(), "w"); if (!f) { perror("scratch directory"); return 2; } fprintf(f, "looper_min_interval=10\n"); fclose(f); }
    array<uint8_t, 32> zero{}, ones{}; ones.fill(255);

    // ---- exact scores: identical one-word frames score 1.0; non-contiguous ids; both comparisons are strict
    {
        ParameterReader para(dir + "/looper_params.txt");
        para.set("looper_vocab_file", write_two_words(dir, 2.0, 3.0));
        para.set("looper_min_sim_score", "0.5"); para.set("looper_min_interval", "10");
        Looper lp(para);
        const int ids[6] = {3, 17, 40, 41, 13, 100};
        vector<RGBDFrame::Ptr> fr;
        for (int i = 0; i < 6; i++) { fr.push_back(make_frame(ids[i], {zero})); lp.add(fr.back()); }
        CHECK("host_path_without_a_context", !lp.onDevice());
        CHECK("bow_vector_of_one_word", fr[0]->bowVec.size() == 1 && fr[0]->bowVec.begin()->first == 0u && fr[0]->bowVec.begin()->second == 1.0);
        // frame id 3 against {3, 17, 40, 41, 13, 100}: |d| = 0, 14, 37, 38, 10, 97 -> 10 is not > 10; database order
        CHECK("noncontiguous_ids_and_strict_interval", ids_of(lp.getPossibleLoops(fr[0])) == vector<int>({17, 40, 41, 100}));
        CHECK("scores_are_exactly_one", lp.last_scores.size() == 6 && lp.last_scores[1] == 1.0 && lp.last_scores[5] == 1.0);
        // an OLDER frame queried after later ones were added sees them all: id 17 against ... |d| = 14, 0, 23, 24, 4, 83
        CHECK("older_frame_after_later_adds", ids_of(lp.getPossibleLoops(fr[1])) == vector<int>({3, 40, 41, 100}));
        CHECK("interval_uses_ids_not_positions", ids_of(lp.getPossibleLoops(fr[4])) == vector<int>({40, 41, 100}));      // id 13: |d| = 10, 4, 27, 28, 0, 87
        para.set("looper_min_sim_score", "1");
        Looper strict(para);
        for (auto& f : fr) strict.add(f);
        CHECK("strict_score_comparison", strict.getPossibleLoops(fr[0]).empty() && strict.last_scores[1] == 1.0);             // 1.0 > 1.0f is false
        // a frame that was never added is scored by the vector it carries
        RGBDFrame::Ptr stray = make_frame(500, {ones});
        CHECK("frame_without_a_vector_scores_zero", lp.getPossibleLoops(stray).empty() && lp.last_scores[0] == 0.0);
    }
    // ---- the threshold is a float: a score between (double)0.015f = 0.01499999966.. and 0.015 is a candidate
    {
        const double t = 0.0149999998;                                     // word 0's share of a frame that holds one feature of each word
        ParameterReader para(dir + "/looper_params.txt");
        para.set("looper_vocab_file", write_two_words(dir, t, 1.0 - t));
        para.set("looper_min_sim_score", "0.015"); para.set("looper_min_interval", "10");
        Looper lp(para);
        RGBDFrame::Ptr a = make_frame(0, {zero}), b = make_frame(50, {zero, ones});
        lp.add(b); lp.add(a);
        vector<RGBDFrame::Ptr> c = lp.getPossibleLoops(a);
        const double s = lp.last_scores[0];
        printf("score %.17g  (double)0.015f %.17g\n", s, (double)0.015f);
        CHECK("score_lies_between_the_float_and_the_double_threshold", s > (double)0.015f && s < 0.015);
        CHECK("float_threshold_makes_it_a_candidate", ids_of(c) == vector<int>({50}));
    }
    // ---- a larger vocabulary: the class against the C functions it is made of
    if (argc > 2) {
        ParameterReader para(dir + "/looper_params.txt");
        para.set("looper_vocab_file", argv[2]); para.set("looper_min_sim_score", "0.05"); para.set("looper_min_interval", "2");
        Looper lp(para);
        ssm_vocab* v = nullptr;
        if (ssm_vocab_load_text(argv[2], &v) != SSM_OK) { printf("FAIL load %s\n", ssm_last_error(nullptr)); return 1; }
        vector<vector<array<uint8_t, 32>>> sets(12);
        for (int f = 0; f < 12; f++) {
            sets[f].resize(300);
            for (auto& d : sets[f]) rand_desc(d.data());
            if (f >= 8) for (int i = 0; i < 150; i++) sets[f][i] = sets[f - 8][i];        // revisits of frames 0 .. 3
        }
        vector<RGBDFrame::Ptr> fr; bool vec_ok = true, cand_ok = true; int ncand = 0;
        vector<vector<int32_t>> vi(12); vector<vector<double>> vv(12);
        for (int f = 0; f < 12; f++) {
            fr.push_back(make_frame(10 * f, sets[f])); lp.add(fr.back());
            vi[f].resize(300); vv[f].resize(300); int m = 0;
            ssm_vocab_transform_host(v, sets[f][0].data(), 300, nullptr, vi[f].data(), vv[f].data(), 300, &m);
            vi[f].resize(m); vv[f].resize(m);
            vec_ok = vec_ok && fr[f]->bowVec.size() == (size_t)m;
            int i = 0; for (auto& kv : fr[f]->bowVec) { vec_ok = vec_ok && i < m && (int32_t)kv.first == vi[f][i] && kv.second == vv[f][i]; i++; }
            vector<int> want;
            for (int e = 0; e <= f; e++) { double s = 0; ssm_bow_score_host(vi[f].data(), vv[f].data(), (int)vi[f].size(), vi[e].data(), vv[e].data(), (int)vi[e].size(), &s); if (s > (double)0.05f && abs(10 * e - 10 * f) > 2) want.push_back(10 * e); }
            cand_ok = cand_ok && ids_of(lp.getPossibleLoops(fr[f])) == want; ncand += (int)want.size();
        }
        CHECK("bow_vectors_equal_transform_host", vec_ok);
        CHECK("candidates_equal_score_host", cand_ok && ncand >= 4);
        ssm_vocab_destroy(v);
    }
    printf(g_fail ? "%d FAILED\n" : "ALL PASSED\n", g_fail);
    return g_fail ? 1 : 0;
}
