// ssm_vocab_train_host.cpp -- vocabulary training on the host (ssm_vocab_train_host, the host half of ssm_debug_vocab_kmajority) and what the device trainer
// (ssm_vocab_train.hip) shares with it: the argument checks, the tree under construction and its last step (word ids, TF-IDF weights, the vocabulary).  Plain
// C++ without any device call, over include/ssm/vocab_train_core.h; linked into the library and, as it is, into host/test_vocab_train (ssm_host.h).
#include "ssm_host.h"
int vt_check(ssm_ctx* c, const uint8_t* desc, const int32_t* n_per_frame, int n_frames, const ssm_vocab_train_params* p, ssm_vocab** out, int* n_out)
{
    if (out) *out = nullptr;
    if (!desc || !n_per_frame || !p || !out) return host_fail(c, SSM_E_INVAL, "vocabulary training: null argument");
    if (n_frames < 1) return host_fail(c, SSM_E_INVAL, "vocabulary training: no frames");
    if (p->k < 2 || p->k > ssm_vt::MAX_K || p->L < 1 || p->L > ssm_vt::MAX_L || p->max_iters < 1) return host_fail(c, SSM_E_INVAL, "vocabulary training: k must be in [2, 20], L in [1, 10] and max_iters >= 1");
    long long n = 0;
    for (int f = 0; f < n_frames; f++) { if (n_per_frame[f] < 0) return host_fail(c, SSM_E_INVAL, "vocabulary training: a negative descriptor count"); n += n_per_frame[f]; if (n > ssm_vt::MAX_N) break; }
    if (n < 1 || n > ssm_vt::MAX_N) return host_fail(c, SSM_E_INVAL, "vocabulary training: the descriptor count must be in [1, 2^26]");
    *n_out = (int)n;
    return SSM_OK;
}
// the finished tree + the leaf (node id) every training descriptor ended in -> word ids in leaf order, Ni per word, weights, the vocabulary
int vt_finish(const VtTree& t, const std::vector<int32_t>& leaf_of_feature, const int32_t* n_per_frame, int n_frames, const ssm_vocab_train_params* p,
              int32_t* word_of_feature, ssm_vocab_train_report* report, ssm_vocab** out)
{
    const int n = (int)t.parent.size();
    std::vector<int32_t> word_of_id((size_t)n + 1, -1); int words = 0;
    for (int i = 0; i < n; i++) if (t.leaf[i]) word_of_id[i + 1] = words++;
    std::vector<int32_t> seen((size_t)words, -1), ni((size_t)words, 0);
    size_t at = 0;
    for (int f = 0; f < n_frames; f++) for (int i = 0; i < n_per_frame[f]; i++, at++) {
        const int w = word_of_id[leaf_of_feature[at]];
        if (word_of_feature) word_of_feature[at] = w;
        if (seen[w] != f) { seen[w] = f; ni[w]++; }
    }
    std::vector<double> weight((size_t)n, 0.0);
    for (int i = 0; i < n; i++) if (t.leaf[i]) weight[i] = ssm_vt::idf_weight(n_frames, ni[word_of_id[i + 1]]);
    if (report) { report->nodes = n + 1; report->words = words; }
    return ssm_vocab_create(p->k, p->L, 0, 0, t.parent.data(), t.leaf.data(), reinterpret_cast<const uint8_t*>(t.desc.data()), weight.data(), n, out);
}
// one pass of step 4 for one node: members mem[0 .. n) (indices into D), clusters a[] in and out, nc centres C in and out -> did an assignment change
static bool vt_pass(const uint32_t* D, const int32_t* mem, int n, int32_t* a, uint32_t* C, int nc, std::vector<int32_t>& ones)
{
    using namespace ssm_vt;
    int count[MAX_K] = {0};
    ones.assign((size_t)nc * DESC_BITS, 0);
    for (int i = 0; i < n; i++) {
        const uint32_t* d = D + (size_t)mem[i] * DESC_WORDS; int32_t* o = &ones[(size_t)a[i] * DESC_BITS];
        count[a[i]]++;
        for (int w = 0; w < DESC_WORDS; w++) for (uint32_t x = d[w]; x; x &= x - 1) o[w * 32 + __builtin_ctz(x)]++;
    }
    for (int j = 0; j < nc; j++) {
        if (!count[j]) continue;                                    // an empty cluster keeps its centre
        for (int w = 0; w < DESC_WORDS; w++) { uint32_t x = 0; for (int b = 0; b < 32; b++) x |= (uint32_t)majority_bit(ones[(size_t)j * DESC_BITS + w * 32 + b], count[j]) << b; C[j * DESC_WORDS + w] = x; }
    }
    bool changed = false;
    for (int i = 0; i < n; i++) { const int na = nearest(C, nc, D + (size_t)mem[i] * DESC_WORDS, nullptr); if (na != a[i]) { a[i] = na; changed = true; } }
    return changed;
}
extern "C" void ssm_vocab_train_params_default(ssm_vocab_train_params* p) { if (p) { p->k = 10; p->L = 5; p->max_iters = 32; } }
extern "C" int ssm_vocab_train_host(const uint8_t* desc, const int32_t* n_per_frame, int n_frames, const ssm_vocab_train_params* p, int32_t* word_of_feature,
                                    ssm_vocab_train_report* report, ssm_vocab** out)
{
    using namespace ssm_vt;
    int N = 0;
    { const int rc = vt_check(nullptr, desc, n_per_frame, n_frames, p, out, &N); if (rc) return rc; }
    if (report) memset(report, 0, sizeof(*report));
    std::vector<uint32_t> D((size_t)N * DESC_WORDS); memcpy(D.data(), desc, (size_t)N * 32);
    struct Node { int id; std::vector<int32_t> mem; };
    std::vector<Node> cur(1); cur[0].id = 0; cur[0].mem.resize((size_t)N); for (int i = 0; i < N; i++) cur[0].mem[i] = i;
    VtTree t; std::vector<int32_t> leaf_of((size_t)N, 0), a, m, ones; int levels = 0, capped = 0;
    for (int l = 0; !cur.empty(); l++) {
        if (l > 0) levels = l;
        std::vector<Node> nxt; int level_passes = 0;
        for (Node& nd : cur) {
            const int n = (int)nd.mem.size(); const int32_t* mem = nd.mem.data();
            bool is_word = l == p->L;
            if (!is_word && nd.id != 0) { is_word = true; for (int i = 1; i < n && is_word; i++) is_word = memcmp(&D[(size_t)mem[i] * DESC_WORDS], &D[(size_t)mem[0] * DESC_WORDS], 32) == 0; }
            if (is_word) { t.leaf[nd.id - 1] = 1; for (int i = 0; i < n; i++) leaf_of[mem[i]] = nd.id; continue; }
            // seeding: farthest point
            uint32_t C[MAX_K * DESC_WORDS]; int nc = 1;
            memcpy(C, &D[(size_t)mem[0] * DESC_WORDS], 32);
            m.resize((size_t)n); a.resize((size_t)n);
            for (int i = 0; i < n; i++) m[i] = ssm_bow::hamming(&D[(size_t)mem[i] * DESC_WORDS], C);
            for (int j = 1; j < p->k; j++) {
                unsigned long long key = 0;
                for (int i = 0; i < n; i++) { const unsigned long long q = seed_key(m[i], (uint32_t)mem[i]); if (q > key) key = q; }
                if (seed_key_dist(key) == 0) break;
                memcpy(C + j * DESC_WORDS, &D[(size_t)seed_key_index(key) * DESC_WORDS], 32); nc++;
                for (int i = 0; i < n; i++) { const int d = ssm_bow::hamming(&D[(size_t)mem[i] * DESC_WORDS], C + j * DESC_WORDS); if (d < m[i]) m[i] = d; }
            }
            for (int i = 0; i < n; i++) a[i] = nearest(C, nc, &D[(size_t)mem[i] * DESC_WORDS], nullptr);
            int passes = 0;
            for (int it = 1; it <= p->max_iters; it++) {
                passes = it;
                if (!vt_pass(D.data(), mem, n, a.data(), C, nc, ones)) break;
                if (it == p->max_iters) capped++;
            }
            if (passes > level_passes) level_passes = passes;
            // children: the clusters that are not empty, in cluster order
            int count[MAX_K] = {0}; for (int i = 0; i < n; i++) count[a[i]]++;
            int child_at[MAX_K];
            for (int j = 0; j < nc; j++) if (count[j]) { child_at[j] = (int)nxt.size(); nxt.push_back(Node{t.add(nd.id, C + j * DESC_WORDS), {}}); nxt.back().mem.reserve((size_t)count[j]); }
            for (int i = 0; i < n; i++) nxt[child_at[a[i]]].mem.push_back(mem[i]);
        }
        if (report && l < MAX_L) report->passes[l] = level_passes;
        cur.swap(nxt);
    }
    if (report) { report->levels = levels; report->capped_nodes = capped; }
    return vt_finish(t, leaf_of, n_per_frame, n_frames, p, word_of_feature, report, out);
}
int vt_kmajority_check(const uint8_t* desc, int n, const int32_t* node_of, const int32_t* cluster_of, int n_nodes, int k, const uint8_t* centres, const int32_t* assign_out)
{
    if (n < 1 || n > ssm_vt::MAX_N || n_nodes < 1 || k < 1 || k > ssm_vt::MAX_K || !desc || !node_of || !cluster_of || !centres || !assign_out) return SSM_E_INVAL;
    for (int i = 0; i < n; i++) if (node_of[i] < 0 || node_of[i] >= n_nodes || cluster_of[i] < 0 || cluster_of[i] >= k || (i && node_of[i] < node_of[i - 1])) return SSM_E_INVAL;
    return SSM_OK;
}
int vt_kmajority_host(const uint8_t* desc, int n, const int32_t* node_of, const int32_t* cluster_of, int n_nodes, int k, uint8_t* centres, int32_t* assign_out)
{
    using namespace ssm_vt;
    { const int rc = vt_kmajority_check(desc, n, node_of, cluster_of, n_nodes, k, centres, assign_out); if (rc) return rc; }
    std::vector<uint32_t> D((size_t)n * DESC_WORDS); memcpy(D.data(), desc, (size_t)n * 32);
    std::vector<int32_t> mem, a, ones;
    for (int i = 0; i < n;) {
        int e = i; while (e < n && node_of[e] == node_of[i]) e++;
        mem.clear(); a.clear(); for (int q = i; q < e; q++) { mem.push_back(q); a.push_back(cluster_of[q]); }
        uint32_t C[MAX_K * DESC_WORDS]; memcpy(C, centres + (size_t)node_of[i] * k * 32, (size_t)k * 32);
        vt_pass(D.data(), mem.data(), e - i, a.data(), C, k, ones);
        memcpy(centres + (size_t)node_of[i] * k * 32, C, (size_t)k * 32);
        for (int q = i; q < e; q++) assign_out[q] = a[q - i];
        i = e;
    }
    return SSM_OK;
}
