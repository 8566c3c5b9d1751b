// test_vocab_train.cpp -- vocabulary training on the host (csrc/ssm_vocab_train_host.cpp over include/ssm/vocab_train_core.h, with the vocabulary object of
// csrc/ssm_vocab.cpp) as a stand-alone program: it is linked with the library's own host sources, so it needs neither libssm_hip.so nor a GPU and runs
// as it is under the CPU sanitizers (make SAN=asan san, or -fsanitize=address,undefined).  Checked here, from C++: every training descriptor comes back to the
// word it was trained into (ssm_vocab_transform_host), the report and the weights are what the exported tree says, export -> create and save -> load give the
// same bits, degenerate and invalid inputs, and the one-pass function with an empty cluster and an exact half split.
#include "ssm_hip.h"
#include "ssm/vocab_train_core.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <unistd.h>
// what the host sources ask of their surroundings (csrc/ssm_host.h): the error path; and the one function checked here that the C ABI reaches only with a context argument
static std::string g_err;
int host_fail(ssm_ctx*, int code, const std::string& msg) { g_err = msg; return code; }
int vt_kmajority_host(const uint8_t* desc, int n, const int32_t* node_of, const int32_t* cluster_of, int n_nodes, int k, uint8_t* centres, int32_t* assign_out);
using namespace std;

static int failures = 0;
static void check(bool ok, const char* name) { printf("%s %s\n", ok ? "PASS" : "FAIL", name); if (!ok) failures++; }
struct Rng { uint64_t s; uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); } };
struct Arrays { vector<int32_t> parent; vector<uint8_t> leaf, desc; vector<double> weight; };
static Arrays exported(const ssm_vocab* v)
{
    int32_t info[6]; ssm_vocab_info(v, info);
    const int n = info[2] - 1;
    Arrays a; a.parent.resize(n); a.leaf.resize(n); a.desc.resize((size_t)n * 32); a.weight.resize(n);
    if (ssm_vocab_export(v, a.parent.data(), a.leaf.data(), a.desc.data(), a.weight.data(), n) != SSM_OK) a.parent.clear();
    return a;
}
static bool same(const Arrays& a, const Arrays& b)
{
    return a.parent == b.parent && a.leaf == b.leaf && a.desc == b.desc && a.weight.size() == b.weight.size() && memcmp(a.weight.data(), b.weight.data(), a.weight.size() * 8) == 0;
}
// train, then everything that must hold for any input
static bool train_and_verify(const vector<uint8_t>& desc, const vector<int32_t>& npf, int k, int L, int iters, const string& tmp, ssm_vocab_train_report* rep_out = nullptr)
{
    const int N = (int)(desc.size() / 32), F = (int)npf.size();
    ssm_vocab_train_params p{k, L, iters}; ssm_vocab_train_report rep; ssm_vocab* v = nullptr;
    vector<int32_t> wof((size_t)N, -1);
    if (ssm_vocab_train_host(desc.data(), npf.data(), F, &p, wof.data(), &rep, &v) != SSM_OK) return false;
    if (rep_out) *rep_out = rep;
    bool ok = true;
    int32_t info[6]; ssm_vocab_info(v, info);
    ok = ok && info[0] == k && info[1] == L && info[2] == rep.nodes && info[3] == rep.words && rep.levels >= 1 && rep.levels <= L;
    // own leaf
    vector<int32_t> back((size_t)N), ids((size_t)N + 1); vector<double> vals((size_t)N + 1); int m = 0;
    ok = ok && ssm_vocab_transform_host(v, desc.data(), N, back.data(), ids.data(), vals.data(), N, &m) == SSM_OK && back == wof;
    // weights from the counts
    const Arrays a = exported(v);
    vector<int32_t> seen((size_t)rep.words, -1), ni((size_t)rep.words, 0);
    size_t at = 0;
    for (int f = 0; f < F; f++) for (int i = 0; i < npf[f]; i++, at++) { const int w = wof[at]; if (w < 0 || w >= rep.words) return false; if (seen[w] != f) { seen[w] = f; ni[w]++; } }
    int word = 0, deepest = 0; vector<int> depth(a.parent.size() + 1, 0);
    for (size_t i = 0; i < a.parent.size(); i++) {
        depth[i + 1] = depth[a.parent[i]] + 1; if (depth[i + 1] > deepest) deepest = depth[i + 1];
        ok = ok && a.parent[i] <= (int)i && (i == 0 || a.parent[i] >= a.parent[i - 1]);                 // breadth-first ids: parents never go back
        if (a.leaf[i]) { ok = ok && ni[word] >= 1 && a.weight[i] == log((double)F / (double)ni[word]); word++; } else ok = ok && a.weight[i] == 0.0;
    }
    ok = ok && word == rep.words && deepest == rep.levels;
    // export -> create, save -> load
    ssm_vocab* v2 = nullptr; ssm_vocab* v3 = nullptr;
    ok = ok && ssm_vocab_create(k, L, 0, 0, a.parent.data(), a.leaf.data(), a.desc.data(), a.weight.data(), (int)a.parent.size(), &v2) == SSM_OK && same(exported(v2), a);
    ok = ok && ssm_vocab_save_text(v, tmp.c_str()) == SSM_OK && ssm_vocab_load_text(tmp.c_str(), &v3) == SSM_OK && same(exported(v3), a);
    ssm_vocab_destroy(v); ssm_vocab_destroy(v2); ssm_vocab_destroy(v3);
    return ok;
}

int main(int argc, char** argv)
{
    const string tmp = string(argc > 1 ? argv[1] : (getenv("TMPDIR") ? getenv("TMPDIR") : "/tmp")) + "/ssm_test_vocab_train_" + to_string((long)getpid()) + ".txt";
    Rng rng{12345};
    {   // random descriptors, empty frames first, in the middle and last
        vector<int32_t> npf = {0, 400, 350, 0, 0, 500, 250, 300, 450, 0};
        int N = 0; for (int x : npf) N += x;
        vector<uint8_t> d((size_t)N * 32); for (uint8_t& b : d) b = (uint8_t)rng.next();
        ssm_vocab_train_report rep;
        check(train_and_verify(d, npf, 6, 3, 32, tmp, &rep), "random_descriptors_with_empty_frames");
        check(rep.capped_nodes == 0 && rep.passes[0] >= 1 && rep.passes[3] == 0, "report_passes");
        check(train_and_verify(d, npf, 20, 2, 32, tmp), "widest_tree");
        check(train_and_verify(d, npf, 2, 10, 32, tmp), "deepest_tree");
        check(train_and_verify(d, npf, 6, 3, 1, tmp, &rep) && rep.capped_nodes > 0, "one_pass_caps_nodes");
    }
    {   // low entropy: one random byte, the rest zero -- equal descriptors, ties, leaves above L
        vector<int32_t> npf = {300, 300, 300};
        vector<uint8_t> d((size_t)900 * 32, 0); for (int i = 0; i < 900; i++) d[(size_t)i * 32] = (uint8_t)rng.next();
        ssm_vocab_train_report rep;
        check(train_and_verify(d, npf, 10, 5, 32, tmp, &rep) && rep.words <= 256, "low_entropy");
    }
    {   // N = 1 and all descriptors equal: the root's only child is the word, weight 0
        vector<uint8_t> one(32); for (uint8_t& b : one) b = (uint8_t)rng.next();
        ssm_vocab_train_report rep;
        check(train_and_verify(one, {1}, 10, 5, 32, tmp, &rep) && rep.nodes == 2 && rep.words == 1 && rep.levels == 1, "single_descriptor");
        vector<uint8_t> many; for (int i = 0; i < 9; i++) many.insert(many.end(), one.begin(), one.end());
        check(train_and_verify(many, {4, 5}, 3, 4, 32, tmp, &rep) && rep.nodes == 2 && rep.words == 1, "all_equal");
    }
    {   // invalid arguments
        vector<uint8_t> d(64 * 32, 1); const int32_t npf[2] = {32, 32}, neg[2] = {70, -6}, zero[1] = {0}; ssm_vocab* v = nullptr;
        const ssm_vocab_train_params bad[5] = {{1, 5, 32}, {21, 5, 32}, {10, 0, 32}, {10, 11, 32}, {10, 5, 0}};
        bool ok = true;
        for (const ssm_vocab_train_params& p : bad) ok = ok && ssm_vocab_train_host(d.data(), npf, 2, &p, nullptr, nullptr, &v) == SSM_E_INVAL && v == nullptr;
        ssm_vocab_train_params p; ssm_vocab_train_params_default(&p);
        ok = ok && p.k == 10 && p.L == 5 && p.max_iters == 32;
        ok = ok && ssm_vocab_train_host(d.data(), neg, 2, &p, nullptr, nullptr, &v) == SSM_E_INVAL && ssm_vocab_train_host(d.data(), zero, 1, &p, nullptr, nullptr, &v) == SSM_E_INVAL;
        ok = ok && ssm_vocab_train_host(d.data(), npf, 0, &p, nullptr, nullptr, &v) == SSM_E_INVAL && ssm_vocab_train_host(nullptr, npf, 2, &p, nullptr, nullptr, &v) == SSM_E_INVAL;
        ok = ok && ssm_vocab_train_host(d.data(), npf, 2, &p, nullptr, nullptr, nullptr) == SSM_E_INVAL;
        check(ok, "invalid_arguments");
    }
    {   // one pass on a made-up state: cluster 1 is empty and keeps its centre; cluster 0 splits 1 : 1 in every bit, which gives all ones
        vector<uint8_t> d(4 * 32); for (int i = 0; i < 32; i++) { d[i] = 0x0F; d[32 + i] = 0xF0; d[64 + i] = 0x00; d[96 + i] = 0x01; }
        const int32_t node_of[4] = {0, 0, 0, 0}, cluster_of[4] = {0, 0, 2, 2}; int32_t out[4];
        vector<uint8_t> c(3 * 32); for (uint8_t& b : c) b = (uint8_t)rng.next();
        const vector<uint8_t> c0 = c;
        bool ok = vt_kmajority_host(d.data(), 4, node_of, cluster_of, 1, 3, c.data(), out) == SSM_OK;
        for (int i = 0; i < 32; i++) ok = ok && c[i] == 0xFF && c[32 + i] == c0[32 + i] && c[64 + i] == 0x01;
        ok = ok && out[2] == 2 && out[3] == 2;
        const int32_t scattered[4] = {0, 1, 0, 1};
        ok = ok && vt_kmajority_host(d.data(), 4, scattered, cluster_of, 2, 3, c.data(), out) == SSM_E_INVAL;
        check(ok, "one_pass_empty_cluster_and_half_split");
    }
    remove(tmp.c_str());
    printf("%s\n", failures ? "SOME FAILED" : "ALL PASSED");
    return failures ? 1 : 0;
}
