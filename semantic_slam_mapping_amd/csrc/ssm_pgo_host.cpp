// ssm_pgo_host.cpp -- the host half of the pose-graph optimiser (reference src/pose_graph.cpp:82-305) behind the C ABI.  DESIGN.md s.12 is the contract.  The graph
// lives on the host; a call plans the active set (integer work: the active edges, the unknown blocks in insertion order, the per-block incident-edge CSR, the
// block envelope), then either walks include/ssm/pgo_core.h's run<> on the CPU (ssm_pgo_optimize_host) or hands the host view to the device leg (ssm_pgo.hip,
// through ssm_host.h's hooks).  Plain C++ without any device call: linked into the library and, as it is, into the CPU sanitizer builds of the host layer.
#include "ssm_host.h"
using namespace ssm_pgc;
static_assert(sizeof(Report) == sizeof(ssm_pgo_report) && (int)SSM_PGO_MAX_ITERS == (int)MAX_ITERS && (int)SSM_PGO_MAX_TRIALS == (int)MAX_TRIALS && (int)SSM_PGO_PHASES == (int)NPHASE, "ssm_pgo_report is pgo_core.h's Report");

// rowoff, reach and the scalar count of the envelope whose block row r starts at block column first[r]
static void env_build(PgoPlan& p)
{
    const int nf = p.nf;
    p.rowoff.assign(nf, 0); p.reach.resize(nf); p.total = 0;
    for (int r = 0; r < nf; r++) { p.rowoff[r] = p.total; p.total += (int64_t)36 * (r - p.first[r] + 1); p.reach[r] = r; }
    // reach[c] = max r with first[r] <= c: rows in descending order claim the columns that no later row reaches
    std::vector<int32_t> lo(nf);
    int32_t m = nf;
    for (int r = nf - 1; r >= 0; r--) { lo[r] = std::min<int32_t>(p.first[r], m); m = lo[r]; }       // lo[r] = min first over rows >= r
    for (int c = 0, r = 0; c < nf; c++) {                                                             // the last r with lo[r] <= c (lo ascends with r)
        if (r < c) r = c;
        while (r + 1 < nf && lo[r + 1] <= c) r++;
        p.reach[c] = r;
    }
}
static void plan_build(ssm_pgo* g)
{
    PgoPlan& p = g->plan; const int nv = g->nv(), ne = g->ne();
    p.aedge.clear(); p.vslot.assign(nv, -1); p.svert.clear(); p.csr_edge.clear();
    std::vector<uint8_t> touched(nv, 0);
    for (int e = 0; e < ne; e++) if (!g->fixed[g->efrom[e]] || !g->fixed[g->eto[e]]) { p.aedge.push_back(e); touched[g->efrom[e]] = touched[g->eto[e]] = 1; }
    for (int v = 0; v < nv; v++) if (!g->fixed[v] && touched[v]) { p.vslot[v] = (int)p.svert.size(); p.svert.push_back(v); }
    p.na = (int)p.aedge.size(); p.nf = (int)p.svert.size();
    p.csr_off.assign(p.nf + 1, 0); p.first.resize(p.nf);
    for (int r = 0; r < p.nf; r++) p.first[r] = r;
    for (int q = 0; q < p.na; q++) {
        const int a = p.vslot[g->efrom[p.aedge[q]]], b = p.vslot[g->eto[p.aedge[q]]];
        if (a >= 0) p.csr_off[a + 1]++;
        if (b >= 0) p.csr_off[b + 1]++;
        if (a >= 0 && b >= 0) { const int hi = std::max(a, b), lo = std::min(a, b); p.first[hi] = std::min(p.first[hi], lo); }
    }
    for (int r = 0; r < p.nf; r++) p.csr_off[r + 1] += p.csr_off[r];
    p.csr_edge.resize(p.csr_off[p.nf]);
    std::vector<int32_t> fill(p.csr_off.begin(), p.csr_off.end() - 1);
    for (int q = 0; q < p.na; q++) {
        const int a = p.vslot[g->efrom[p.aedge[q]]], b = p.vslot[g->eto[p.aedge[q]]];
        if (a >= 0) p.csr_edge[fill[a]++] = q;
        if (b >= 0) p.csr_edge[fill[b]++] = q;
    }
    env_build(p);
}
static View host_view(ssm_pgo* g)
{
    const PgoPlan& p = g->plan; View v{};
    v.nv = g->nv(); v.ne = g->ne(); v.nf = p.nf; v.na = p.na;
    g->lin.resize((size_t)LIN * p.na + 1); g->H.resize(p.total + 1); g->L.resize(p.total + 1);
    for (std::vector<double>* w : {&g->b, &g->x, &g->y, &g->d}) w->resize((size_t)6 * p.nf + 1);
    g->saved.resize((size_t)16 * p.nf + 1);
    v.pose = g->pose.data(); v.efrom = g->efrom.data(); v.eto = g->eto.data(); v.robust = g->robust.data(); v.zinv = g->zinv.data(); v.omega = g->omega.data();
    v.aedge = p.aedge.data(); v.vslot = p.vslot.data(); v.svert = p.svert.data(); v.csr_off = p.csr_off.data(); v.csr_edge = p.csr_edge.data();
    v.env.nf = p.nf; v.env.total = p.total; v.env.first = p.first.data(); v.env.rowoff = p.rowoff.data(); v.env.reach = p.reach.data();
    v.lin = g->lin.data(); v.H = g->H.data(); v.L = g->L.data(); v.b = g->b.data(); v.x = g->x.data(); v.y = g->y.data(); v.d = g->d.data(); v.saved = g->saved.data();
    v.ctl = &g->ctl; v.rep = &g->rep;
    return v;
}
static int pgo_cap_check(ssm_pgo* g)
{
    if ((size_t)g->plan.total * 16 > g->cap_bytes)
        return host_fail(g->c, SSM_E_CAPACITY, "pgo: the envelope needs " + std::to_string((size_t)g->plan.total * 16) + " bytes, the cap is " + std::to_string(g->cap_bytes));
    return SSM_OK;
}
static void report_finish(ssm_pgo* g, ssm_pgo_report* out)
{
    g->rep.active_vertices = g->plan.nf; g->rep.active_edges = g->plan.na; g->rep.envelope_scalars = g->plan.total;
    if (g->plan.na == 0 || g->plan.nf == 0) { g->rep.iterations = 0; g->rep.lambda = 0; }
    for (int it = g->rep.iterations; it < MAX_ITERS; it++) {
        g->rep.trials[it] = 0; g->rep.accepted[it] = 0; g->rep.chi2_before[it] = g->rep.chi2_after[it] = 0;
        for (int t = 0; t < MAX_TRIALS; t++) g->rep.gain[it][t] = 0;
    }
    for (int it = 0; it < g->rep.iterations; it++) for (int t = g->rep.trials[it]; t < MAX_TRIALS; t++) g->rep.gain[it][t] = 0;
    for (int k = 0; k < NPHASE; k++) g->ms[k] = (double)g->rep.clocks[k] * 1e-5;          // wall_clock64: 100 MHz
    if (out) memcpy(out, &g->rep, sizeof *out);
}

extern "C" int ssm_pgo_create(ssm_ctx* c, ssm_pgo** out)
{
    if (!out) return SSM_E_INVAL;
    *out = nullptr;
    std::unique_ptr<ssm_pgo> g(new ssm_pgo());
    g->c = c;
    if (c) { const int r = pgo_dev_attach(g.get()); if (r) return r; }
    *out = g.release();
    return SSM_OK;
}
extern "C" void ssm_pgo_destroy(ssm_pgo* g)
{
    if (!g) return;
    if (g->c) pgo_dev_release(g);
    delete g;
}
extern "C" int ssm_pgo_clear(ssm_pgo* g)
{
    if (!g) return SSM_E_INVAL;
    g->ids.clear(); g->index.clear(); g->pose.clear(); g->fixed.clear(); g->efrom.clear(); g->eto.clear(); g->robust.clear(); g->Z.clear(); g->zinv.clear(); g->omega.clear();
    return SSM_OK;
}
static bool pose_ok(const double* T) { for (int k = 0; k < 16; k++) if (!std::isfinite(T[k])) return false; return true; }
extern "C" int ssm_pgo_add_vertex(ssm_pgo* g, int id, const double T[16], int fixed)
{
    if (!g || !T) return SSM_E_INVAL;
    if (g->index.count(id)) return host_fail(g->c, SSM_E_INVAL, "pgo: vertex " + std::to_string(id) + " exists");
    if (!pose_ok(T)) return host_fail(g->c, SSM_E_INVAL, "pgo: a pose that is not finite");
    g->index[id] = g->nv(); g->ids.push_back(id); g->pose.insert(g->pose.end(), T, T + 16); g->fixed.push_back(fixed != 0);
    return SSM_OK;
}
extern "C" int ssm_pgo_add_edge(ssm_pgo* g, int id_from, int id_to, const double Z[16], const double* info21, int robust)
{
    if (!g || !Z) return SSM_E_INVAL;
    const auto a = g->index.find(id_from), b = g->index.find(id_to);
    if (a == g->index.end() || b == g->index.end()) return host_fail(g->c, SSM_E_INVAL, "pgo: an edge names the unknown vertex " + std::to_string(a == g->index.end() ? id_from : id_to));
    if (id_from == id_to) return host_fail(g->c, SSM_E_INVAL, "pgo: an edge from a vertex to itself");
    if (!pose_ok(Z)) return host_fail(g->c, SSM_E_INVAL, "pgo: a measurement that is not finite");
    double om[36], zi[16];
    for (int k = 0; k < 36; k++) om[k] = 0.0;
    if (info21) { int q = 0; for (int r = 0; r < 6; r++) for (int cc = r; cc < 6; cc++) { if (!std::isfinite(info21[q])) return host_fail(g->c, SSM_E_INVAL, "pgo: an information entry that is not finite"); om[6 * r + cc] = om[6 * cc + r] = info21[q++]; } }
    else for (int r = 0; r < 6; r++) om[7 * r] = 100.0;
    ssm_pnp::iso_inverse(Z, zi);
    g->efrom.push_back(a->second); g->eto.push_back(b->second); g->robust.push_back(robust != 0);
    g->Z.insert(g->Z.end(), Z, Z + 16); g->zinv.insert(g->zinv.end(), zi, zi + 16); g->omega.insert(g->omega.end(), om, om + 36);
    return SSM_OK;
}
extern "C" int ssm_pgo_set_fixed(ssm_pgo* g, int id, int fixed)
{
    if (!g) return SSM_E_INVAL;
    const auto a = g->index.find(id);
    if (a == g->index.end()) return host_fail(g->c, SSM_E_INVAL, "pgo: unknown vertex " + std::to_string(id));
    g->fixed[a->second] = fixed != 0;
    return SSM_OK;
}
extern "C" int ssm_pgo_set_mode(ssm_pgo* g, int local)
{
    if (!g) return SSM_E_INVAL;
    const size_t n = g->ids.size();
    if (!local) { for (size_t i = 0; i < n; i++) g->fixed[i] = i == 0; return SSM_OK; }
    for (size_t i = 0; i < n; i++) g->fixed[i] = 1;
    for (int i = (int)n - 1; i > 0 && (size_t)i > n - 6; i--) g->fixed[i] = 0;         // pose_graph.cpp:272: n < 6 wraps and frees nothing
    return SSM_OK;
}
extern "C" int ssm_pgo_set_pose(ssm_pgo* g, int id, const double T[16])
{
    if (!g || !T) return SSM_E_INVAL;
    const auto a = g->index.find(id);
    if (a == g->index.end()) return host_fail(g->c, SSM_E_INVAL, "pgo: unknown vertex " + std::to_string(id));
    if (!pose_ok(T)) return host_fail(g->c, SSM_E_INVAL, "pgo: a pose that is not finite");
    std::copy(T, T + 16, g->pose.begin() + 16 * (size_t)a->second);
    return SSM_OK;
}
extern "C" int ssm_pgo_get_poses(const ssm_pgo* g, int32_t* ids, double* T, int cap, int* n_out)
{
    if (!g) return SSM_E_INVAL;
    if (n_out) *n_out = g->nv();
    if (!ids && !T) return SSM_OK;
    if (cap < g->nv()) return host_fail(g->c, SSM_E_CAPACITY, "pgo: " + std::to_string(g->nv()) + " vertices");
    if (ids) std::copy(g->ids.begin(), g->ids.end(), ids);
    if (T) std::copy(g->pose.begin(), g->pose.end(), T);
    return SSM_OK;
}
extern "C" int ssm_pgo_size(const ssm_pgo* g, int* vertices, int* edges)
{
    if (!g) return SSM_E_INVAL;
    if (vertices) *vertices = g->nv();
    if (edges) *edges = g->ne();
    return SSM_OK;
}
extern "C" int ssm_pgo_edge_chi2(const ssm_pgo* g, int edge, double* chi2)
{
    if (!g || !chi2) return SSM_E_INVAL;
    if (edge < 0 || edge >= g->ne()) return host_fail(g->c, SSM_E_INVAL, "pgo: no edge " + std::to_string(edge));
    double e[6];
    edge_error(g->zinv.data() + 16 * (size_t)edge, g->pose.data() + 16 * (size_t)g->efrom[edge], g->pose.data() + 16 * (size_t)g->eto[edge], e);
    *chi2 = quad_form(g->omega.data() + 36 * (size_t)edge, e);
    return SSM_OK;
}
extern "C" int ssm_pgo_set_envelope_cap(ssm_pgo* g, size_t bytes) { if (!g) return SSM_E_INVAL; g->cap_bytes = bytes; return SSM_OK; }

extern "C" int ssm_pgo_optimize_host(ssm_pgo* g, int iterations, ssm_pgo_report* report)
{
    if (!g || iterations < 0 || iterations > MAX_ITERS) return SSM_E_INVAL;
    plan_build(g);
    { const int r = pgo_cap_check(g); if (r) return r; }
    const View v = host_view(g);
    run<HostExec>(v, iterations);
    report_finish(g, report);
    return SSM_OK;
}
extern "C" int ssm_pgo_optimize_many(ssm_pgo** graphs, int n, int iterations, ssm_pgo_report* reports)
{
    if (!graphs || n < 1 || iterations < 0 || iterations > MAX_ITERS) return SSM_E_INVAL;
    for (int i = 0; i < n; i++) if (!graphs[i]) return SSM_E_INVAL;
    ssm_ctx* c = graphs[0]->c;
    if (!c) return host_fail(graphs[0]->c, SSM_E_NODEVICE, "pgo: a host-only object has no device path");
    for (int i = 0; i < n; i++) {
        if (graphs[i]->c != c) return host_fail(graphs[0]->c, SSM_E_INVAL, "pgo: the graphs of one call belong to one context");
        for (int j = 0; j < i; j++) if (graphs[j] == graphs[i]) return host_fail(graphs[0]->c, SSM_E_INVAL, "pgo: a graph is listed twice");
    }
    for (int i = 0; i < n; i++) { plan_build(graphs[i]); const int r = pgo_cap_check(graphs[i]); if (r) return r; }       // nothing is queued before every graph fits
    std::vector<View> hv(n);
    for (int i = 0; i < n; i++) hv[i] = host_view(graphs[i]);
    { const int r = pgo_dev_optimize(graphs, n, hv.data(), iterations); if (r) return r; }
    for (int i = 0; i < n; i++) report_finish(graphs[i], reports ? reports + i : nullptr);
    return SSM_OK;
}
extern "C" int ssm_pgo_optimize(ssm_pgo* g, int iterations, ssm_pgo_report* report) { return ssm_pgo_optimize_many(&g, 1, iterations, report); }

extern "C" int ssm_pgo_envelope(ssm_pgo* g, int32_t* first, int cap, int* nr_out, int64_t* scalars_out)
{
    if (!g) return SSM_E_INVAL;
    plan_build(g);
    if (nr_out) *nr_out = g->plan.nf;
    if (scalars_out) *scalars_out = g->plan.total;
    if (first) { if (cap < g->plan.nf) return host_fail(g->c, SSM_E_CAPACITY, "pgo: " + std::to_string(g->plan.nf) + " block rows"); std::copy(g->plan.first.begin(), g->plan.first.end(), first); }
    return SSM_OK;
}
extern "C" int ssm_pgo_active(ssm_pgo* g, int* vertices, int* edges)
{
    if (!g) return SSM_E_INVAL;
    plan_build(g);
    if (vertices) *vertices = g->plan.nf;
    if (edges) *edges = g->plan.na;
    return SSM_OK;
}
extern "C" int ssm_debug_pgo_lm_update(int scaled, double state[2], double chi, double chi_new, int solved, const double x[6], const double b[6], double out[2])
{
    if (!state || !x || !b || !out) return SSM_E_INVAL;
    LmState st; st.lambda = state[0]; st.nu = state[1];
    double gain = 0; bool acc;
    if (!scaled) acc = ssm_pnp::lm_update(st, chi, chi_new, solved != 0, x, b, gain);
    else { double scale = 0; for (int j = 0; j < 6; j++) scale += x[j] * (st.lambda * x[j] + b[j]); acc = lm_update_scaled(st, chi, chi_new, solved != 0, scale, gain); }
    state[0] = st.lambda; state[1] = st.nu; out[0] = gain; out[1] = acc ? 1.0 : 0.0;
    return SSM_OK;
}
extern "C" int ssm_pgo_linearize(ssm_pgo* g, int device, double* e, double* Ji, double* Jj, double* w, double* H, double* b)
{
    if (!g) return SSM_E_INVAL;
    if (device && !g->c) return host_fail(g->c, SSM_E_NODEVICE, "pgo: a host-only object has no device path");
    plan_build(g);
    { const int r = pgo_cap_check(g); if (r) return r; }
    const View v = host_view(g);
    const PgoPlan& p = g->plan;
    if (p.na == 0 || p.nf == 0) return SSM_OK;
    if (!device) linearize_assemble<HostExec>(v, false);
    else { const int r = pgo_dev_linearize(g, v); if (r) return r; }
    for (int q = 0; q < p.na; q++) {
        const double* l = g->lin.data() + (size_t)LIN * q;
        if (e) std::copy(l, l + 6, e + 6 * (size_t)q);
        if (Ji) std::copy(l + 6, l + 42, Ji + 36 * (size_t)q);
        if (Jj) std::copy(l + 42, l + 78, Jj + 36 * (size_t)q);
        if (w) w[q] = l[78];
    }
    if (H) std::copy(g->H.begin(), g->H.begin() + p.total, H);
    if (b) std::copy(g->b.begin(), g->b.begin() + (size_t)6 * p.nf, b);
    return SSM_OK;
}
extern "C" int ssm_pgo_factor_solve(ssm_pgo* g, int device, int nr, const int32_t* first, const double* H, const double* b, double lambda, double* x, int* ok)
{
    if (!g || nr < 1 || !first || !H || !b || !x || !ok) return SSM_E_INVAL;
    if (device && !g->c) return host_fail(g->c, SSM_E_NODEVICE, "pgo: a host-only object has no device path");
    for (int r = 0; r < nr; r++) if (first[r] < 0 || first[r] > r) return host_fail(g->c, SSM_E_INVAL, "pgo: first[" + std::to_string(r) + "] is outside 0 .. " + std::to_string(r));
    // a plan of its own: nr unknown blocks, no vertices, no edges
    ssm_pgo t; t.c = g->c; t.cap_bytes = g->cap_bytes;
    PgoPlan& p = t.plan; p.nf = nr; p.na = 0; p.first.assign(first, first + nr); p.csr_off.assign(nr + 1, 0); p.svert.assign(nr, 0);
    env_build(p);
    { const int r = pgo_cap_check(&t); if (r) return r; }
    View v = host_view(&t);
    std::copy(H, H + p.total, t.H.begin()); std::copy(b, b + (size_t)6 * nr, t.b.begin());
    if (!device) factor_solve<HostExec>(v, lambda);
    else { const int r = pgo_dev_factor_solve(g, t, v, lambda); if (r) return r; }
    std::copy(t.x.begin(), t.x.begin() + (size_t)6 * nr, x);
    *ok = t.ctl.ok;
    return SSM_OK;
}
extern "C" int ssm_pgo_times(const ssm_pgo* g, double ms[SSM_PGO_PHASES])
{
    if (!g || !ms) return SSM_E_INVAL;
    for (int k = 0; k < NPHASE; k++) ms[k] = g->ms[k];
    return SSM_OK;
}

extern "C" int ssm_pgo_save_g2o(const ssm_pgo* g, const char* path)
{
    if (!g || !path) return SSM_E_INVAL;
    FILE* f = fopen(path, "w");
    if (!f) return host_fail(g->c, SSM_E_INVAL, std::string("pgo: cannot write ") + path);
    auto tq = [&](const double* T) {
        double R[9], q[4]; iso_rot(T, R); rot_to_quat(R, q);
        const double n = quat_norm(q), sg = q[3] / n < 0 ? -1.0 : 1.0;
        fprintf(f, " %.17g %.17g %.17g %.17g %.17g %.17g %.17g", T[12], T[13], T[14], sg * (q[0] / n), sg * (q[1] / n), sg * (q[2] / n), sg * (q[3] / n));
    };
    for (int v = 0; v < g->nv(); v++) { fprintf(f, "VERTEX_SE3:QUAT %d", g->ids[v]); tq(g->pose.data() + 16 * (size_t)v); fputc('\n', f); }
    for (int v = 0; v < g->nv(); v++) if (g->fixed[v]) fprintf(f, "FIX %d\n", g->ids[v]);
    for (int e = 0; e < g->ne(); e++) {
        fprintf(f, "EDGE_SE3:QUAT %d %d", g->ids[g->efrom[e]], g->ids[g->eto[e]]); tq(g->Z.data() + 16 * (size_t)e);
        for (int r = 0; r < 6; r++) for (int cc = r; cc < 6; cc++) fprintf(f, " %.17g", g->omega[36 * (size_t)e + 6 * r + cc]);
        fputc('\n', f);
    }
    const bool bad = ferror(f) != 0;
    if (fclose(f) != 0 || bad) return host_fail(g->c, SSM_E_INVAL, std::string("pgo: writing ") + path + " failed");
    return SSM_OK;
}
extern "C" int ssm_pgo_load_g2o(ssm_pgo* g, const char* path, int robust)
{
    if (!g || !path) return SSM_E_INVAL;
    FILE* f = fopen(path, "r");
    if (!f) return host_fail(g->c, SSM_E_INVAL, std::string("pgo: cannot read ") + path);
    ssm_pgo_clear(g);
    std::vector<char> line(4096);
    int ln = 0, rc = SSM_OK;
    auto bad = [&](const char* what) { rc = host_fail(g->c, SSM_E_INVAL, std::string("pgo: ") + path + " line " + std::to_string(ln) + ": " + what); };
    auto pose7 = [](const double* p, double* T) {
        const double n = quat_norm(p + 3);
        quat_iso(p[3] / n, p[4] / n, p[5] / n, p[6] / n, p, T);
    };
    while (rc == SSM_OK && fgets(line.data(), (int)line.size(), f)) {
        ln++;
        char tag[64]; int used = 0;
        if (sscanf(line.data(), " %63s%n", tag, &used) != 1) continue;             // a blank line
        const char* rest = line.data() + used;
        double p[28]; int a = 0, b = 0, m = 0;
        if (!strcmp(tag, "VERTEX_SE3:QUAT")) {
            if (sscanf(rest, "%d %lf %lf %lf %lf %lf %lf %lf", &a, p, p + 1, p + 2, p + 3, p + 4, p + 5, p + 6) != 8 || !(quat_norm(p + 3) > 0)) { bad("a malformed vertex"); break; }
            double T[16]; pose7(p, T);
            if (ssm_pgo_add_vertex(g, a, T, 0) != SSM_OK) { bad("a vertex that cannot be added"); break; }
        } else if (!strcmp(tag, "FIX")) {
            if (sscanf(rest, "%d", &a) != 1 || ssm_pgo_set_fixed(g, a, 1) != SSM_OK) { bad("FIX of an unknown vertex"); break; }
        } else if (!strcmp(tag, "EDGE_SE3:QUAT")) {
            if (sscanf(rest, "%d %d%n", &a, &b, &used) != 2) { bad("a malformed edge"); break; }
            rest += used;
            for (m = 0; m < 28; m++) { int u = 0; if (sscanf(rest, "%lf%n", p + m, &u) != 1) break; rest += u; }
            if (m != 28 || !(quat_norm(p + 3) > 0)) { bad("a malformed edge"); break; }
            double Z[16]; pose7(p, Z);
            if (ssm_pgo_add_edge(g, a, b, Z, p + 7, robust) != SSM_OK) { bad("an edge that cannot be added"); break; }
        } else bad("an unsupported tag");
    }
    fclose(f);
    if (rc != SSM_OK) ssm_pgo_clear(g);
    return rc;
}
