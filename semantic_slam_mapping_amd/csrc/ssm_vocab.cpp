// ssm_vocab.cpp -- the vocabulary of the looper (ssm_vocab_*, ssm_bow_score_host): a host object, plain C++ without any device call, over
// include/ssm/looper_core.h.  Linked into the library and, as it is, into the CPU sanitizer builds of the host layer and host/test_vocab_train (ssm_host.h).
#include "ssm_host.h"
#include <cerrno>
#include <cstdlib>
extern "C" int ssm_vocab_create(int k, int L, int scoring, int weighting, const int32_t* parent, const uint8_t* is_leaf, const uint8_t* desc, const double* weight, int n, ssm_vocab** out)
{
    if (!out) return host_fail(nullptr, SSM_E_INVAL, "null argument");
    *out = nullptr;
    if (n < 0 || (n > 0 && (!parent || !is_leaf || !desc || !weight))) return host_fail(nullptr, SSM_E_INVAL, "null argument");
    if (k < 0 || k > 20 || L < 1 || L > 10) return host_fail(nullptr, SSM_E_INVAL, "vocabulary: k must be in [0, 20] and L in [1, 10]");
    if (scoring != 0 || weighting != 0) return host_fail(nullptr, SSM_E_INVAL, "vocabulary: only scoring 0 (L1_NORM) with weighting 0 (TF_IDF) is supported");
    if (n == 0) return host_fail(nullptr, SSM_E_INVAL, "vocabulary: the root has no children");
    // file ids: 0 = the root, node i of the arrays = id i + 1
    std::vector<int32_t> cnt((size_t)n + 1, 0), start((size_t)n + 2, 0);
    for (int i = 0; i < n; i++) {
        if (parent[i] < 0 || parent[i] > i) return host_fail(nullptr, SSM_E_INVAL, "vocabulary: node " + std::to_string(i + 1) + " names parent " + std::to_string(parent[i]) + ", which is not an earlier node");
        if (parent[i] > 0 && is_leaf[parent[i] - 1]) return host_fail(nullptr, SSM_E_INVAL, "vocabulary: leaf node " + std::to_string(parent[i]) + " has children");
        cnt[parent[i]]++;
    }
    for (int i = 0; i < n; i++) if (!is_leaf[i] && cnt[i + 1] == 0) return host_fail(nullptr, SSM_E_INVAL, "vocabulary: node " + std::to_string(i + 1) + " is neither a leaf nor has children");
    for (int i = 0; i <= n; i++) { if (cnt[i] > 65535) return host_fail(nullptr, SSM_E_INVAL, "vocabulary: more than 65535 children under one node"); start[i + 1] = start[i] + cnt[i]; }
    std::vector<int32_t> kids((size_t)n), fill(start.begin(), start.end() - 1);
    for (int i = 0; i < n; i++) kids[fill[parent[i]]++] = i + 1;                    // the children of every id, in file order
    std::vector<int32_t> word_of_id((size_t)n + 1, -1); int nwords = 0;
    for (int i = 0; i < n; i++) if (is_leaf[i]) word_of_id[i + 1] = nwords++;
    ssm_vocab* v = new ssm_vocab(); v->k = k; v->L = L; v->scoring = scoring; v->weighting = weighting;
    v->first_child.assign((size_t)n + 1, 0); v->n_child.assign((size_t)n + 1, 0); v->word.assign((size_t)n + 1, -1); v->desc.assign(((size_t)n + 1) * 8, 0u); v->weight.assign((size_t)nwords, 0.0);
    std::vector<int32_t> order; order.reserve((size_t)n + 1); order.push_back(0);     // breadth-first: order[new index] = file id
    std::vector<int32_t> depth((size_t)n + 1, 0);
    for (size_t at = 0; at < order.size(); at++) {
        const int id = order[at];
        v->n_child[at] = cnt[id]; v->first_child[at] = cnt[id] ? (int32_t)order.size() : 0;
        for (int c = 0; c < cnt[id]; c++) { depth[order.size()] = depth[at] + 1; order.push_back(kids[start[id] + c]); }
        if (depth[at] > v->max_depth) v->max_depth = depth[at];
        if (id > 0) {
            memcpy(&v->desc[at * 8], desc + (size_t)(id - 1) * 32, 32);
            v->word[at] = word_of_id[id];
            if (word_of_id[id] >= 0) v->weight[word_of_id[id]] = weight[id - 1];
        }
    }
    v->file_id = order;
    *out = v;
    return SSM_OK;
}
extern "C" int ssm_vocab_export(const ssm_vocab* v, int32_t* parent, uint8_t* is_leaf, uint8_t* desc, double* weight, int cap)
{
    if (!v || cap < 0) return SSM_E_INVAL;
    const int nn = (int)v->n_child.size();
    if (cap < nn - 1) return SSM_E_CAPACITY;
    for (int at = 0; at < nn; at++) {
        for (int c = 0; c < v->n_child[at]; c++) if (parent) parent[v->file_id[v->first_child[at] + c] - 1] = v->file_id[at];
        if (at == 0) continue;
        const int i = v->file_id[at] - 1;
        if (is_leaf) is_leaf[i] = v->n_child[at] == 0;
        if (desc) memcpy(desc + (size_t)i * 32, &v->desc[(size_t)at * 8], 32);
        if (weight) weight[i] = v->word[at] >= 0 ? v->weight[v->word[at]] : 0.0;
    }
    return SSM_OK;
}
extern "C" int ssm_vocab_save_text(const ssm_vocab* v, const char* path)
{
    if (!v || !path) return host_fail(nullptr, SSM_E_INVAL, "null argument");
    const int n = (int)v->n_child.size() - 1;
    std::vector<int32_t> parent((size_t)n); std::vector<uint8_t> leaf((size_t)n), desc((size_t)n * 32); std::vector<double> weight((size_t)n);
    { const int rc = ssm_vocab_export(v, parent.data(), leaf.data(), desc.data(), weight.data(), n); if (rc) return rc; }
    FILE* f = fopen(path, "wb");
    if (!f) return host_fail(nullptr, SSM_E_INVAL, std::string("vocabulary: cannot write ") + path);
    fprintf(f, "%d %d %d %d\n", v->k, v->L, v->scoring, v->weighting);
    for (int i = 0; i < n; i++) {
        fprintf(f, "%d %d", parent[i], (int)leaf[i]);
        for (int b = 0; b < 32; b++) fprintf(f, " %d", (int)desc[(size_t)i * 32 + b]);
        fprintf(f, " %.17g\n", weight[i]);                       // 17 significant digits give every double back
    }
    const bool bad = ferror(f) != 0;
    if (fclose(f) != 0 || bad) return host_fail(nullptr, SSM_E_INVAL, std::string("vocabulary: write error on ") + path);
    return SSM_OK;
}
extern "C" int ssm_vocab_load_text(const char* path, ssm_vocab** out)
{
    if (!out) return host_fail(nullptr, SSM_E_INVAL, "null argument");
    *out = nullptr;
    if (!path) return host_fail(nullptr, SSM_E_INVAL, "null argument");
    FILE* f = fopen(path, "rb");
    if (!f) return host_fail(nullptr, SSM_E_INVAL, std::string("vocabulary: cannot open ") + path);
    std::string text; { char buf[1 << 16]; size_t got; while ((got = fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, got); }
    fclose(f);
    std::vector<int32_t> parent; std::vector<uint8_t> leaf, desc; std::vector<double> weight;
    long hdr[4] = {0, 0, 0, 0}; bool have_hdr = false; long lineno = 0;
    const char* p = text.c_str(); const char* end = p + text.size();
    while (p < end) {
        const char* eol = (const char*)memchr(p, '\n', (size_t)(end - p)); if (!eol) eol = end;
        lineno++;
        const char* q = p; while (q < eol && (*q == ' ' || *q == '\t' || *q == '\r')) q++;
        if (q < eol) {
            const std::string where = "vocabulary: malformed line " + std::to_string(lineno);
            // (a number ends at white space or at the end of the line: `1.5` is not the integer 1; strtol / strtod never run into the next line, the newline stops them)
            auto next_long = [&](long& v) { while (q < eol && (*q == ' ' || *q == '\t')) q++; if (q >= eol) return false; char* e; errno = 0; v = strtol(q, &e, 10); if (e == q || e > eol || errno || (e < eol && *e != ' ' && *e != '\t' && *e != '\r')) return false; q = e; return true; };
            if (!have_hdr) {
                for (int i = 0; i < 4; i++) if (!next_long(hdr[i])) return host_fail(nullptr, SSM_E_INVAL, where);
                have_hdr = true;
            } else {
                long pa, lf, b;
                if (!next_long(pa) || !next_long(lf) || pa < 0 || pa > 0x7FFFFFFE) return host_fail(nullptr, SSM_E_INVAL, where);
                parent.push_back((int32_t)pa); leaf.push_back(lf > 0 ? 1 : 0);
                for (int i = 0; i < 32; i++) { if (!next_long(b) || b < 0 || b > 255) return host_fail(nullptr, SSM_E_INVAL, where); desc.push_back((uint8_t)b); }
                while (q < eol && (*q == ' ' || *q == '\t')) q++;
                if (q >= eol) return host_fail(nullptr, SSM_E_INVAL, where);
                char* e; errno = 0; const double w = strtod(q, &e); if (e == q || e > eol) return host_fail(nullptr, SSM_E_INVAL, where);
                q = e; weight.push_back(w);
            }
            while (q < eol && (*q == ' ' || *q == '\t' || *q == '\r')) q++;
            if (q != eol) return host_fail(nullptr, SSM_E_INVAL, where);
        }
        p = eol + 1;
    }
    if (!have_hdr) return host_fail(nullptr, SSM_E_INVAL, "vocabulary: empty file");
    if (hdr[0] < 0 || hdr[0] > 20 || hdr[1] < 1 || hdr[1] > 10 || hdr[2] < 0 || hdr[2] > 5 || hdr[3] < 0 || hdr[3] > 3) return host_fail(nullptr, SSM_E_INVAL, "vocabulary: bad header (k L scoring weighting)");
    return ssm_vocab_create((int)hdr[0], (int)hdr[1], (int)hdr[2], (int)hdr[3], parent.data(), leaf.data(), desc.data(), weight.data(), (int)parent.size(), out);
}
extern "C" void ssm_vocab_destroy(ssm_vocab* v) { delete v; }
extern "C" int ssm_vocab_info(const ssm_vocab* v, int32_t info[6])
{
    if (!v || !info) return SSM_E_INVAL;
    info[0] = v->k; info[1] = v->L; info[2] = (int32_t)v->n_child.size(); info[3] = (int32_t)v->weight.size(); info[4] = v->scoring; info[5] = v->weighting;
    return SSM_OK;
}
extern "C" int ssm_vocab_transform_host(const ssm_vocab* v, const uint8_t* desc, int n, int32_t* word_of_feature, int32_t* ids, double* vals, int cap, int* n_out)
{
    if (!v || n < 0 || (n > 0 && !desc) || !n_out || cap < 0 || (cap > 0 && (!ids || !vals))) return SSM_E_INVAL;
    const ssm_bow::Tree t = v->tree();
    std::vector<int32_t> words; words.reserve((size_t)n);
    for (int i = 0; i < n; i++) {
        uint32_t q[8]; memcpy(q, desc + (size_t)i * 32, 32);
        const int w = t.word[ssm_bow::descend(t, q)];
        if (word_of_feature) word_of_feature[i] = w;
        if (w >= 0 && t.weight[w] > 0.0) words.push_back(w);
    }
    std::sort(words.begin(), words.end());
    std::vector<int32_t> oi(words.size() + 1); std::vector<double> ov(words.size() + 1);
    const int m = ssm_bow::bow_from_sorted_words(words.data(), (int)words.size(), t.weight, oi.data(), ov.data());
    *n_out = m;
    if (m > cap) return SSM_E_CAPACITY;
    if (m) { memcpy(ids, oi.data(), (size_t)m * 4); memcpy(vals, ov.data(), (size_t)m * 8); }
    return SSM_OK;
}
extern "C" int ssm_bow_score_host(const int32_t* ids1, const double* v1, int n1, const int32_t* ids2, const double* v2, int n2, double* score)
{
    if (!score || n1 < 0 || n2 < 0 || (n1 > 0 && (!ids1 || !v1)) || (n2 > 0 && (!ids2 || !v2))) return SSM_E_INVAL;
    *score = ssm_bow::score(ids1, v1, n1, ids2, v2, n2);
    return SSM_OK;
}
