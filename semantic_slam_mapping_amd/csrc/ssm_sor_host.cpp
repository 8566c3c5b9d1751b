// ssm_sor_host.cpp -- the statistical outlier removal on the CPU: ssm_sor_filter_host, the parameter defaults and the argument check the device
// entry points share.  Plain C++ over include/ssm/sor_core.h with one thread.  It walks the same ladder of grids as the device path (sort by cell key, nine key
// runs per cell, the unsettled points climb), with a heap per query where the device keeps a sorted wave: the two have the contract in common, not the code.
#include "ssm_host.h"
using namespace ssm_sorc;

extern "C" void ssm_sor_params_default(ssm_sor_params* p) { if (!p) return; p->mean_k = 30; p->cell = 0.0f; p->stddev_mul = 1.0; }
extern "C" int ssm_sor_chunk(void) { return CHUNK; }
int sor_check(ssm_ctx* c, int n, const ssm_sor_params& P)
{
    if (n < 0) return host_fail(c, SSM_E_INVAL, "sor: bad arguments");
    if (P.mean_k < 1 || P.mean_k > MAX_K) return host_fail(c, SSM_E_INVAL, "sor: mean_k must be 1..64");
    if (!(P.cell >= 0.0f) || !finite1(P.cell)) return host_fail(c, SSM_E_INVAL, "sor: cell must be finite and not negative");
    if (!(std::fabs(P.stddev_mul) <= DBL_MAX)) return host_fail(c, SSM_E_INVAL, "sor: stddev_mul must be finite");
    return SSM_OK;
}
int sor_off_grid(ssm_ctx* c) { return host_fail(c, SSM_E_INVAL, "sor: a mean neighbour distance of 4096 m or more does not fit the statistics grid"); }

extern "C" int ssm_sor_filter_host(const ssm_point* pts, int n, const ssm_sor_params* params, ssm_point* out, int cap, int* n_out, ssm_sor_info* info,
                                   float* mean_dist, uint8_t* keep)
{
    ssm_sor_params P; ssm_sor_params_default(&P); if (params) P = *params;
    { const int r = sor_check(nullptr, n, P); if (r) return r; }
    if (!n_out || (n && !pts) || cap < 0) return host_fail(nullptr, SSM_E_INVAL, "null argument");
    const int k = P.mean_k;
    ssm_sor_info I{}; I.n_in = n;
    std::vector<float> md((size_t)n, 0.0f); std::vector<uint8_t> kp((size_t)n, 0);
    std::vector<int32_t> fin;          // the finite points, by input index
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    for (int i = 0; i < n; i++) {
        const float v[3] = {pts[i].x, pts[i].y, pts[i].z};
        if (!finite3(v[0], v[1], v[2])) continue;
        for (int a = 0; a < 3; a++) { if (fin.empty() || v[a] < lo[a]) lo[a] = v[a]; if (fin.empty() || v[a] > hi[a]) hi[a] = v[a]; }
        fin.push_back(i);
    }
    const int nf = (int)fin.size();
    I.n_finite = nf;
    if (nf < k + 1) {
        I.too_few = 1;
        for (int i : fin) kp[i] = 1;
    } else {
        const Plan plan = plan_of(lo, hi, P.cell, nf);
        std::vector<uint8_t> settled((size_t)nf, 0);
        std::vector<std::pair<uint64_t, int32_t>> order((size_t)nf);
        std::vector<float> sx((size_t)nf), sy((size_t)nf), sz((size_t)nf); std::vector<uint64_t> skey((size_t)nf);
        float heap[MAX_K];
        int left = nf;
        for (int level = 0; left > 0; level++) {
            const bool top = level >= plan.top;
            const double c = level_cell(plan.c0, level);
            const float r2 = settle_r2(c);
            for (int j = 0; j < nf; j++) { const ssm_point& p = pts[fin[j]]; order[j] = {top ? 0 : point_key(p.x, p.y, p.z, plan.lo, c), j}; }
            if (!top) std::sort(order.begin(), order.end());
            for (int s = 0; s < nf; s++) { const ssm_point& p = pts[fin[order[s].second]]; sx[s] = p.x; sy[s] = p.y; sz[s] = p.z; skey[s] = order[s].first; }
            int run_lo[9], run_hi[9], nrun = 0; uint64_t cell_key = KEY_NONE;
            for (int s = 0; s < nf; s++) {
                const int j = order[s].second;
                if (settled[j]) continue;
                if (top) { run_lo[0] = 0; run_hi[0] = nf; nrun = 1; }
                else if (skey[s] != cell_key) {          // the queries of one cell share its nine runs
                    cell_key = skey[s]; nrun = 0;
                    const int64_t m = ((int64_t)1 << AXIS_BITS) - 1, cx = (int64_t)(cell_key & m), cy = (int64_t)((cell_key >> AXIS_BITS) & m), cz = (int64_t)(cell_key >> (2 * AXIS_BITS));
                    for (int r = 0; r < 9; r++) {
                        uint64_t first, last;
                        if (!key_run(cx, cy, cz, r, &first, &last)) continue;
                        run_lo[nrun] = (int)(std::lower_bound(skey.begin(), skey.end(), first) - skey.begin());
                        run_hi[nrun] = (int)(std::upper_bound(skey.begin(), skey.end(), last) - skey.begin());
                        if (run_hi[nrun] > run_lo[nrun]) nrun++;
                    }
                }
                int have = 0; int64_t seen = -1;          // (the point itself is in its own cell's run)
                for (int r = 0; r < nrun; r++) {
                    seen += run_hi[r] - run_lo[r];
                    for (int t = run_lo[r]; t < run_hi[r]; t++) {
                        if (t == s) continue;
                        const float d2 = dist2(sx[s], sy[s], sz[s], sx[t], sy[t], sz[t]);
                        if (have < k) { heap[have++] = d2; std::push_heap(heap, heap + have); }
                        else if (d2 < heap[0]) { std::pop_heap(heap, heap + k); heap[k - 1] = d2; std::push_heap(heap, heap + k); }
                    }
                }
                if (!top && !(seen >= k && heap[0] <= r2)) continue;
                std::sort_heap(heap, heap + k);
                double sum = 0.0;
                for (int t = 0; t < k; t++) sum += root(heap[t]);
                md[fin[j]] = mean_of(sum, k); settled[j] = 1; left--;
            }
            I.levels = level + 1;
        }
        for (int i : fin) {
            if (!on_grid(md[i])) return sor_off_grid(nullptr);
            const uint64_t q = quantise(md[i]), q2 = q * q;
            I.sum_q += q; I.sum_q2_lo += q2 & 0xFFFFFFFFull; I.sum_q2_hi += q2 >> 32;
        }
        const Stats st = stats_of(nf, I.sum_q, I.sum_q2_lo, I.sum_q2_hi, P.stddev_mul);
        I.mean = st.mean; I.stddev = st.stddev; I.threshold = st.threshold;
        for (int i : fin) kp[i] = keeps(md[i], st.threshold) ? 1 : 0;
    }
    for (int i = 0; i < n; i++) I.n_kept += kp[i];
    *n_out = I.n_kept;
    if (info) *info = I;
    if (mean_dist && n) memcpy(mean_dist, md.data(), (size_t)n * 4);
    if (keep && n) memcpy(keep, kp.data(), (size_t)n);
    if (I.n_kept > cap) return host_fail(nullptr, SSM_E_CAPACITY, "point buffer too small (need " + std::to_string(I.n_kept) + ")");
    if (I.n_kept && !out) return host_fail(nullptr, SSM_E_INVAL, "null argument");
    for (int i = 0, o = 0; i < n; i++) if (kp[i]) out[o++] = pts[i];
    return SSM_OK;
}
