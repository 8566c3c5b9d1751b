// ssm_vocab_train.hip -- vocabulary training behind the C ABI: the device trainer (the host function is ssm_vocab_train_host.cpp), which grows
// the tree level by level with the kernels of kernels_vocab_train.hip.  Per level the host reads back what it needs to build the tree (centres seeded, members per
// cluster, the centres) and the "an assignment changed" flag after every pass; the descriptors, the permutation and the assignments never leave the device.
#include "ssm_ctx.h"
#include "ssm_host.h"
#include <chrono>

namespace {
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// the buffers of one training run
struct VtRun {
    DevBuf<uint32_t> desc, centres, gcnt;
    DevBuf<int32_t> perm[2], nodeof[2], start, m, a, ncent, changed_at, flag, strad, hist, prefix, rank, noderank, dest, child, leaf_id, leaf_of;
    DevBuf<unsigned long long> keys[2];
};
template <class T> int up(ssm_ctx* c, DevBuf<T>& b, const std::vector<T>& h)
{
    DALLOC(c, b, h.size());
    if (!h.empty()) HIPCHK(c, hipMemcpyAsync(b, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, c->main.stream));
    return SSM_OK;
}
template <class T> int down(ssm_ctx* c, std::vector<T>& h, const T* d, size_t n)
{
    h.resize(n);
    if (n) HIPCHK(c, hipMemcpyAsync(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost, c->main.stream));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    return SSM_OK;
}
// the nodes that cross a chunk boundary
std::vector<int32_t> straddlers(const std::vector<int32_t>& start)
{
    std::vector<int32_t> s;
    for (size_t v = 0; v + 1 < start.size(); v++) if (start[v + 1] > start[v] && start[v] / VT_CHUNK != (start[v + 1] - 1) / VT_CHUNK) s.push_back((int32_t)v);
    return s;
}
// one pass of step 4 on the level, enqueued: centre update, then assignment
int pass_enqueue(ssm_ctx* c, const VtLevel& L, const int32_t* strad, int ns, int pass)
{
    hipStream_t s = c->main.stream;
    HIPCHK(c, k_vt_count(L, s));
    HIPCHK(c, k_vt_finish(L, strad, ns, s));
    HIPCHK(c, hipMemsetAsync(L.flag, 0, 4, s));
    HIPCHK(c, k_vt_assign(L, pass, s));
    return SSM_OK;
}
}  // namespace

extern "C" int ssm_vocab_train(ssm_ctx* c, const uint8_t* desc, const int32_t* n_per_frame, int n_frames, const ssm_vocab_train_params* p, int32_t* word_of_feature,
                               ssm_vocab_train_report* report, ssm_vocab** out)
{
    using namespace ssm_vt;
    if (!c) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    int N = 0;
    { const int rc = vt_check(c, desc, n_per_frame, n_frames, p, out, &N); if (rc) return rc; }
    if (report) memset(report, 0, sizeof(*report));
    hipStream_t s = c->main.stream;
    const double t_begin = now_ms();
    for (double& x : c->vt_level_ms) x = 0.0;
    c->vt_total_ms = -1.0;
    const int k = p->k, chunks = (N + VT_CHUNK - 1) / VT_CHUNK;
    VtRun R;
    DALLOC(c, R.desc, (size_t)N * DESC_WORDS);
    HIPCHK(c, hipMemcpyAsync(R.desc, desc, (size_t)N * 32, hipMemcpyHostToDevice, s));
    for (int i = 0; i < 2; i++) { DALLOC(c, R.perm[i], N); DALLOC(c, R.nodeof[i], N); }
    DALLOC(c, R.m, N); DALLOC(c, R.a, N); DALLOC(c, R.rank, N); DALLOC(c, R.flag, 1);
    DALLOC(c, R.gcnt, (size_t)chunks * k * 257); DALLOC(c, R.hist, (size_t)chunks * k);
    HIPCHK(c, hipMemsetAsync(R.gcnt, 0, (size_t)chunks * k * 257 * 4, s));
    for (int i = 0; i < 2; i++) { HIPCHK(c, hipMemsetAsync(R.nodeof[i], 0, (size_t)N * 4, s)); HIPCHK(c, hipMemsetAsync(R.perm[i], 0, (size_t)N * 4, s)); }
    { std::vector<int32_t> id((size_t)N); for (int i = 0; i < N; i++) id[i] = i; HIPCHK(c, hipMemcpyAsync(R.perm[0], id.data(), (size_t)N * 4, hipMemcpyHostToDevice, s)); HIPCHK(c, hipStreamSynchronize(s)); }
    // the level's nodes in position order: the tree id of each (0 = the root) and whether it is a word carried along from a level above (its members stay in
    // place: one cluster, nothing changes, no child in the tree)
    std::vector<int32_t> start{0, N}, tid{0}; std::vector<uint8_t> carried{0};
    VtTree t; int levels = 0, capped = 0, cur = 0;
    std::vector<int32_t> h_ncent, h_hist, h_prefix, h_noderank, h_changed, h_dest, h_child; std::vector<uint32_t> h_centres;
    for (int l = 0; l < p->L; l++) {
        const double t_level = now_ms();
        const int nn = (int)tid.size();
        { const int rc = up(c, R.start, start); if (rc) return rc; }
        DALLOC(c, R.centres, (size_t)nn * k * DESC_WORDS); DALLOC(c, R.ncent, nn); DALLOC(c, R.changed_at, nn); DALLOC(c, R.noderank, (size_t)nn * k);
        DALLOC(c, R.keys[0], nn); DALLOC(c, R.keys[1], nn);
        HIPCHK(c, hipMemsetAsync(R.changed_at, 0, (size_t)nn * 4, s));
        HIPCHK(c, hipMemsetAsync(R.noderank, 0, (size_t)nn * k * 4, s));
        VtLevel Lv{}; Lv.desc = R.desc; Lv.N = N; Lv.k = k; Lv.nn = nn; Lv.perm = R.perm[cur]; Lv.nodeof = R.nodeof[cur]; Lv.start = R.start; Lv.m = R.m; Lv.a = R.a;
        Lv.centres = R.centres; Lv.ncent = R.ncent; Lv.gcnt = R.gcnt; Lv.changed_at = R.changed_at; Lv.flag = R.flag;
        // seeding: k rounds, the argmax of round r in keys[r & 1]
        for (int r = 0; r < k; r++) {
            unsigned long long* ko = r < k - 1 ? (unsigned long long*)R.keys[r & 1] : nullptr;
            if (ko) HIPCHK(c, hipMemsetAsync(ko, 0, (size_t)nn * 8, s));
            HIPCHK(c, k_vt_seed(Lv, r, r ? (const unsigned long long*)R.keys[(r - 1) & 1] : nullptr, ko, s));
        }
        { const int rc = down(c, h_ncent, (const int32_t*)R.ncent, (size_t)nn); if (rc) return rc; }
        // a node is split when it is the root or has members that differ (two centres were seeded); the others are words
        bool any_split = false;
        for (int v = 0; v < nn; v++) if (!carried[v] && (tid[v] == 0 || h_ncent[v] >= 2)) any_split = true;
        if (!any_split) break;
        levels = l + 1;
        // step 4: passes until none changes an assignment (a converged node is a fixed point, so the level iterates as a whole)
        const std::vector<int32_t> strad = straddlers(start);
        { const int rc = up(c, R.strad, strad); if (rc) return rc; }
        int passes = 0;
        for (int it = 1; it <= p->max_iters; it++) {
            { const int rc = pass_enqueue(c, Lv, R.strad, (int)strad.size(), it); if (rc) return rc; }
            int32_t changed = 0;
            HIPCHK(c, hipMemcpyAsync(&changed, R.flag, 4, hipMemcpyDeviceToHost, s)); HIPCHK(c, hipStreamSynchronize(s));
            passes = it;
            if (!changed) break;
        }
        if (report) report->passes[l] = passes;
        { const int rc = down(c, h_changed, (const int32_t*)R.changed_at, (size_t)nn); if (rc) return rc; }
        for (int v = 0; v < nn; v++) capped += h_changed[v] == p->max_iters;
        // members per (node, cluster): chunk histogram, its prefix over the chunks (host: chunks x k numbers), ranks
        HIPCHK(c, k_vt_hist(Lv, R.hist, s));
        { const int rc = down(c, h_hist, (const int32_t*)R.hist, (size_t)chunks * k); if (rc) return rc; }
        h_prefix.resize((size_t)chunks * k); int32_t total[MAX_K] = {0};
        for (int ch = 0; ch < chunks; ch++) for (int j = 0; j < k; j++) { h_prefix[(size_t)ch * k + j] = total[j]; total[j] += h_hist[(size_t)ch * k + j]; }
        { const int rc = up(c, R.prefix, h_prefix); if (rc) return rc; }
        HIPCHK(c, k_vt_rank(Lv, R.prefix, R.rank, R.noderank, s));
        { const int rc = down(c, h_noderank, (const int32_t*)R.noderank, (size_t)nn * k); if (rc) return rc; }
        { const int rc = down(c, h_centres, (const uint32_t*)R.centres, (size_t)nn * k * DESC_WORDS); if (rc) return rc; }
        // the next level's nodes
        std::vector<int32_t> nstart, ntid; std::vector<uint8_t> ncarried;
        h_dest.assign((size_t)nn * k, 0); h_child.assign((size_t)nn * k, 0);
        int at = 0;
        for (int v = 0; v < nn; v++) {
            const bool split = !carried[v] && (tid[v] == 0 || h_ncent[v] >= 2);
            if (!carried[v] && !split) t.leaf[tid[v] - 1] = 1;
            for (int j = 0; j < k; j++) {
                const int cnt = (v + 1 < nn ? h_noderank[(size_t)(v + 1) * k + j] : total[j]) - h_noderank[(size_t)v * k + j];
                if (cnt <= 0) continue;
                h_dest[(size_t)v * k + j] = at; h_child[(size_t)v * k + j] = (int32_t)ntid.size();
                nstart.push_back(at); at += cnt;
                ntid.push_back(split ? t.add(tid[v], &h_centres[((size_t)v * k + j) * DESC_WORDS]) : tid[v]); ncarried.push_back(split ? 0 : 1);
            }
        }
        nstart.push_back(at);
        if (at != N) FAIL(c, SSM_E_HIP, "vocabulary training: the device member counts do not add up");
        { const int rc = up(c, R.dest, h_dest); if (rc) return rc; }
        { const int rc = up(c, R.child, h_child); if (rc) return rc; }
        HIPCHK(c, k_vt_scatter(Lv, R.rank, R.noderank, R.dest, R.child, R.perm[cur ^ 1], R.nodeof[cur ^ 1], s));
        HIPCHK(c, hipStreamSynchronize(s));
        cur ^= 1; start.swap(nstart); tid.swap(ntid); carried.swap(ncarried);
        c->vt_level_ms[l] = now_ms() - t_level;
    }
    // every node of the last level is a word
    for (size_t v = 0; v < tid.size(); v++) if (!carried[v] && tid[v] > 0) t.leaf[tid[v] - 1] = 1;
    { const int rc = up(c, R.leaf_id, tid); if (rc) return rc; }
    DALLOC(c, R.leaf_of, N);
    VtLevel Lv{}; Lv.N = N; Lv.k = k; Lv.nn = (int)tid.size(); Lv.perm = R.perm[cur]; Lv.nodeof = R.nodeof[cur];
    HIPCHK(c, k_vt_leaves(Lv, R.leaf_id, R.leaf_of, s));
    std::vector<int32_t> leaf_of;
    { const int rc = down(c, leaf_of, (const int32_t*)R.leaf_of, (size_t)N); if (rc) return rc; }
    if (report) { report->levels = levels; report->capped_nodes = capped; }
    const int rc = vt_finish(t, leaf_of, n_per_frame, n_frames, p, word_of_feature, report, out);
    c->vt_total_ms = now_ms() - t_begin;
    return rc;
}

extern "C" int ssm_debug_vocab_kmajority(ssm_ctx* c, const uint8_t* desc, int n, const int32_t* node_of, const int32_t* cluster_of, int n_nodes, int k, uint8_t* centres, int32_t* assign_out)
{
    using namespace ssm_vt;
    if (!c) return vt_kmajority_host(desc, n, node_of, cluster_of, n_nodes, k, centres, assign_out);
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (vt_kmajority_check(desc, n, node_of, cluster_of, n_nodes, k, centres, assign_out)) FAIL(c, SSM_E_INVAL, "bad arguments");
    hipStream_t s = c->main.stream;
    const int chunks = (n + VT_CHUNK - 1) / VT_CHUNK;
    std::vector<int32_t> start((size_t)n_nodes + 1, 0), id((size_t)n), nc((size_t)n_nodes, k);
    for (int i = 0; i < n; i++) { start[node_of[i] + 1]++; id[i] = i; }
    for (int v = 0; v < n_nodes; v++) start[v + 1] += start[v];
    const std::vector<int32_t> strad = straddlers(start);
    VtRun R;
    DALLOC(c, R.desc, (size_t)n * DESC_WORDS); DALLOC(c, R.centres, (size_t)n_nodes * k * DESC_WORDS); DALLOC(c, R.gcnt, (size_t)chunks * k * 257);
    DALLOC(c, R.nodeof[0], n); DALLOC(c, R.a, n); DALLOC(c, R.changed_at, n_nodes); DALLOC(c, R.flag, 1);
    HIPCHK(c, hipMemcpyAsync(R.desc, desc, (size_t)n * 32, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(R.centres, centres, (size_t)n_nodes * k * 32, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(R.nodeof[0], node_of, (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(R.a, cluster_of, (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemsetAsync(R.gcnt, 0, (size_t)chunks * k * 257 * 4, s));
    HIPCHK(c, hipMemsetAsync(R.changed_at, 0, (size_t)n_nodes * 4, s));
    { int rc = up(c, R.perm[0], id); if (!rc) rc = up(c, R.start, start); if (!rc) rc = up(c, R.ncent, nc); if (!rc) rc = up(c, R.strad, strad); if (rc) return rc; }
    VtLevel Lv{}; Lv.desc = R.desc; Lv.N = n; Lv.k = k; Lv.nn = n_nodes; Lv.perm = R.perm[0]; Lv.nodeof = R.nodeof[0]; Lv.start = R.start; Lv.a = R.a;
    Lv.centres = R.centres; Lv.ncent = R.ncent; Lv.gcnt = R.gcnt; Lv.changed_at = R.changed_at; Lv.flag = R.flag;
    { const int rc = pass_enqueue(c, Lv, R.strad, (int)strad.size(), 1); if (rc) return rc; }
    HIPCHK(c, hipMemcpyAsync(centres, R.centres, (size_t)n_nodes * k * 32, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(assign_out, R.a, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return SSM_OK;
}
extern "C" int ssm_debug_vocab_train_times(ssm_ctx* c, double level_ms[10], double* total_ms)
{
    if (!c || !level_ms || !total_ms) return SSM_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->vt_total_ms < 0) FAIL(c, SSM_E_INVAL, "no ssm_vocab_train has completed on this context");
    for (int l = 0; l < ssm_vt::MAX_L; l++) level_ms[l] = c->vt_level_ms[l];
    *total_ms = c->vt_total_ms;
    return SSM_OK;
}
