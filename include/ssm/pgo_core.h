// ssm/pgo_core.h -- the arithmetic of the pose-graph optimiser (reference src/pose_graph.cpp:82-305: a g2o graph of VertexSE3 / EdgeSE3 with Huber kernels,
// OptimizationAlgorithmLevenberg over a sparse Cholesky) as plain functions on plain arrays, shared by
//   * ssm_pgo_optimize_host (the CPU, one thread),
//   * ssm_pgo_optimize / ssm_pgo_optimize_many (one 1024-thread block per graph, csrc/kernels_pgo.hip),
// so that both give the same bits.  g2o (un-vendored, absent) is restated; DESIGN.md s.12 is the contract.  The whole optimisation is ONE function template,
// run<X>(View): X says who executes it (X::tid(), X::nt(), X::sync(), X::lane_sum()).  Every number has one owner thread and one written order of operations,
// so how the elements are spread over threads does not show in the result.  Both sides are built -ffp-contract=off; everything is +, -, *, /, sqrt in IEEE double.
#pragma once
#include "pnp_core.h"
// the per-edge routines are calls on the device: inlined into the one-block kernel their 6 x 6 temporaries compete with the solver loops for its 128 registers
#if defined(__HIP_DEVICE_COMPILE__)
#  define SSM_PGO_CALL __attribute__((noinline))
#else
#  define SSM_PGO_CALL
#endif
namespace ssm_pgc {
using ssm_pnp::LmState;
enum { LANES = ssm_pnp::LANES, GROUP = ssm_pnp::GROUP, NGROUP = ssm_pnp::NGROUP, MAX_ITERS = 32, MAX_TRIALS = 10, LIN = 80 /* doubles per linearised edge */,
       NPHASE = 5 /* linearise, assemble, factor + solves, update + chi2, decide */ };

// ---- poses: 4 x 4 column-major isometries (compat.h); rotations inside the functions are row-major 3 x 3
SSM_HD void iso_rot(const double* T, double* R) { for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) R[3 * r + c] = T[c * 4 + r]; }
// v = (t, qx, qy, qz): w = sqrt(1 - |q|^2) or 0 when that is not positive; R of the quaternion (x, y, z, w) as Eigen::Quaterniond::toRotationMatrix writes it
SSM_HD void quat_iso(double x, double y, double z, double w, const double* t, double* T)
{
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    for (int k = 0; k < 16; k++) T[k] = 0.0;
    T[0] = 1 - (tyy + tzz); T[4] = txy - twz; T[8] = txz + twy;
    T[1] = txy + twz; T[5] = 1 - (txx + tzz); T[9] = tyz - twx;
    T[2] = txz - twy; T[6] = tyz + twx; T[10] = 1 - (txx + tyy);
    T[12] = t[0]; T[13] = t[1]; T[14] = t[2]; T[15] = 1.0;
}
SSM_HD void from_mqt(const double* v, double* T)
{
    const double x = v[3], y = v[4], z = v[5];
    const double w2 = 1.0 - ((x * x + y * y) + z * z);
    quat_iso(x, y, z, w2 > 0 ? sqrt(w2) : 0.0, v, T);
}
// Eigen's Quaterniond(Matrix3d): branch 3 = trace > 0, branch i = the largest diagonal entry is R(i, i).  q = (x, y, z, w), not normalised
SSM_HD int rot_to_quat(const double* R, double* q)
{
    const double t = (R[0] + R[4]) + R[8];
    if (t > 0) {
        double s = sqrt(t + 1.0); q[3] = 0.5 * s; s = 0.5 / s;
        q[0] = (R[7] - R[5]) * s; q[1] = (R[2] - R[6]) * s; q[2] = (R[3] - R[1]) * s;
        return 3;
    }
    int i = 0; if (R[4] > R[0]) i = 1; if (R[8] > R[4 * i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    double s = sqrt(((R[4 * i] - R[4 * j]) - R[4 * k]) + 1.0); q[i] = 0.5 * s; s = 0.5 / s;
    q[3] = (R[3 * k + j] - R[3 * j + k]) * s; q[j] = (R[3 * j + i] + R[3 * i + j]) * s; q[k] = (R[3 * k + i] + R[3 * i + k]) * s;
    return i;
}
// the derivative of rot_to_quat's branch `br` at R in the direction dR
SSM_HD void rot_to_quat_d(const double* R, const double* dR, int br, double* dq)
{
    if (br == 3) {
        const double u = ((R[0] + R[4]) + R[8]) + 1.0, s = sqrt(u), f = 0.5 / s, du = (dR[0] + dR[4]) + dR[8], df = -0.25 / (s * u) * du;
        dq[3] = 0.25 / s * du;
        dq[0] = (dR[7] - dR[5]) * f + (R[7] - R[5]) * df; dq[1] = (dR[2] - dR[6]) * f + (R[2] - R[6]) * df; dq[2] = (dR[3] - dR[1]) * f + (R[3] - R[1]) * df;
        return;
    }
    const int i = br, j = (i + 1) % 3, k = (j + 1) % 3;
    const double u = ((R[4 * i] - R[4 * j]) - R[4 * k]) + 1.0, s = sqrt(u), f = 0.5 / s, du = (dR[4 * i] - dR[4 * j]) - dR[4 * k], df = -0.25 / (s * u) * du;
    dq[i] = 0.25 / s * du;
    dq[3] = (dR[3 * k + j] - dR[3 * j + k]) * f + (R[3 * k + j] - R[3 * j + k]) * df;
    dq[j] = (dR[3 * j + i] + dR[3 * i + j]) * f + (R[3 * j + i] + R[3 * i + j]) * df;
    dq[k] = (dR[3 * k + i] + dR[3 * i + k]) * f + (R[3 * k + i] + R[3 * i + k]) * df;
}
SSM_HD double quat_norm(const double* q) { return sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]); }
// t, then the xyz of R's quaternion, normalised, negated when w < 0.  Returns the branch
SSM_HD int to_mqt(const double* T, double* v)
{
    double R[9], q[4]; iso_rot(T, R);
    const int br = rot_to_quat(R, q);
    const double n = quat_norm(q), sg = q[3] / n < 0 ? -1.0 : 1.0;
    v[0] = T[12]; v[1] = T[13]; v[2] = T[14];
    for (int k = 0; k < 3; k++) v[3 + k] = sg * (q[k] / n);
    return br;
}
// e = toMQT(Z^-1 Xi^-1 Xj)
SSM_HD void edge_error(const double* Zinv, const double* Xi, const double* Xj, double* e)
{
    double Ii[16], B[16], E[16];
    ssm_pnp::iso_inverse(Xi, Ii); ssm_pnp::iso_mul(Ii, Xj, B); ssm_pnp::iso_mul(Zinv, B, E);
    to_mqt(E, e);
}
// e^T Om e, Om a full symmetric 6 x 6
SSM_HD double quad_form(const double* Om, const double* e)
{
    double s = 0;
    for (int r = 0; r < 6; r++) { double t = 0; for (int c = 0; c < 6; c++) t += Om[6 * r + c] * e[c]; s += e[r] * t; }
    return s;
}
SSM_PGO_CALL SSM_HD double edge_rho(const double* Zinv, const double* Xi, const double* Xj, const double* Om, int robust, double* w)
{
    double e[6]; edge_error(Zinv, Xi, Xj, e);
    const double e2 = quad_form(Om, e);
    double r0 = e2, r1 = 1.0;
    if (robust) ssm_pnp::huber(e2, 1.0, r0, r1);
    if (w) *w = r1;
    return r0;
}
// e and the exact derivatives of e with respect to the updates of Xi and Xj (X <- X fromMQT(d)) at d = 0; Ji, Jj row-major 6 x 6
SSM_PGO_CALL SSM_HD void edge_linearize(const double* Zinv, const double* Xi, const double* Xj, double* e, double* Ji, double* Jj)
{
    double Ii[16], B[16], E[16];
    ssm_pnp::iso_inverse(Xi, Ii); ssm_pnp::iso_mul(Ii, Xj, B); ssm_pnp::iso_mul(Zinv, B, E);
    double RA[9], RB[9], RE[9], q[4];
    iso_rot(Zinv, RA); iso_rot(B, RB); iso_rot(E, RE);
    const int br = rot_to_quat(RE, q);
    const double n = quat_norm(q), sg = q[3] / n < 0 ? -1.0 : 1.0;
    const double qn[4] = {q[0] / n, q[1] / n, q[2] / n, q[3] / n};
    e[0] = E[12]; e[1] = E[13]; e[2] = E[14];
    for (int k = 0; k < 3; k++) e[3 + k] = sg * qn[k];
    for (int k = 0; k < 36; k++) { Ji[k] = 0.0; Jj[k] = 0.0; }
    const double tb[3] = {B[12], B[13], B[14]};
    const double S2[9] = {0, -2 * tb[2], 2 * tb[1], 2 * tb[2], 0, -2 * tb[0], -2 * tb[1], 2 * tb[0], 0};
    double RS[9]; ssm_pnp::mat3_mul(RA, S2, RS);
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) { Ji[6 * r + c] = -RA[3 * r + c]; Ji[6 * r + 3 + c] = RS[3 * r + c]; Jj[6 * r + c] = RE[3 * r + c]; }
    for (int k = 0; k < 3; k++) {
        // d R(fromMQT(d)) / d q_k at 0 = 2 [e_k]x
        double G[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        const int a = (k + 1) % 3, b = (k + 2) % 3;
        G[3 * b + a] = 2.0; G[3 * a + b] = -2.0;
        double M[9], dRi[9], dRj[9], dq[4];
        ssm_pnp::mat3_mul(RA, G, M); ssm_pnp::mat3_mul(M, RB, dRi);
        for (int m = 0; m < 9; m++) dRi[m] = -dRi[m];
        ssm_pnp::mat3_mul(RE, G, dRj);
        for (int side = 0; side < 2; side++) {
            rot_to_quat_d(RE, side ? dRj : dRi, br, dq);
            const double dot = ((qn[0] * dq[0] + qn[1] * dq[1]) + qn[2] * dq[2]) + qn[3] * dq[3];
            double* J = side ? Jj : Ji;
            for (int r = 0; r < 3; r++) J[6 * (3 + r) + 3 + k] = sg * ((dq[r] - qn[r] * dot) / n);
        }
    }
}
// entry (a, b) of Ja^T (w Om) Jb, and entry a of Ja^T (w Om) e
SSM_HD double contrib_entry(const double* Ja, int a, const double* Om, double w, const double* Jb, int b)
{
    double s = 0;
    for (int r = 0; r < 6; r++) { double t = 0; for (int c = 0; c < 6; c++) t += (w * Om[6 * r + c]) * Jb[6 * c + b]; s += Ja[6 * r + a] * t; }
    return s;
}
SSM_HD double contrib_rhs(const double* Ja, int a, const double* Om, double w, const double* e)
{
    double s = 0;
    for (int r = 0; r < 6; r++) { double t = 0; for (int c = 0; c < 6; c++) t += (w * Om[6 * r + c]) * e[c]; s += Ja[6 * r + a] * t; }
    return s;
}
// ssm_pnp::lm_update with the sum x . (lambda x + b) over ALL unknowns handed in (lm_update adds six terms in a loop; here the sum is a lane sum)
SSM_HD bool lm_update_scaled(LmState& s, double chi, double chi_new, bool solved, double scale, double& gain)
{
    if (!solved) chi_new = DBL_MAX;
    gain = chi - chi_new;
    scale += 1e-3; gain /= scale;
    if (gain > 0 && isfinite(chi_new)) {
        const double t = 2 * gain - 1;
        double alpha = 1. - t * t * t; alpha = alpha < 2. / 3. ? alpha : 2. / 3.;
        s.lambda *= alpha > 1. / 3. ? alpha : 1. / 3.; s.nu = 2;
        return true;
    }
    s.lambda *= s.nu; s.nu *= 2;
    return false;
}

struct Report {
    int32_t iterations, active_vertices, active_edges, solve_failures;
    int64_t envelope_scalars;
    double lambda;
    int32_t trials[MAX_ITERS];
    uint32_t accepted[MAX_ITERS];           // bit t: trial t of the iteration was accepted
    double chi2_before[MAX_ITERS], chi2_after[MAX_ITERS], gain[MAX_ITERS][MAX_TRIALS];
    int64_t clocks[NPHASE];
};
// The envelope of the system of nf unknown blocks: block row r keeps the block columns first[r] .. r as a 6 x (6 (r - first[r] + 1)) rectangle of scalars at
// rowoff[r], scalar row by scalar row (the entries right of the diagonal are not used).  reach[c]: the last block row whose envelope holds block column c.
struct Envelope { int nf; int64_t total /* scalars */; const int32_t* first; const int64_t* rowoff; const int32_t* reach; };
SSM_HD int env_start(const Envelope& v, int i) { return 6 * v.first[i / 6]; }
SSM_HD int64_t env_at(const Envelope& v, int i, int j) { const int r = i / 6; return v.rowoff[r] + (int64_t)(i - 6 * r) * (6 * (r - v.first[r] + 1)) + (j - 6 * v.first[r]); }
// ctl: the block's control words; one writer, read after a sync
struct Control { int32_t ok, accepted, stop, pad; double lambda, nu, chi, chi_new, gain, scale; };
struct View {
    int nv, ne, nf, na;
    double* pose;                           // nv x 16, in / out
    const int32_t *efrom, *eto, *robust;    // ne: vertex indices
    const double *zinv, *omega;             // ne x 16: the inverse measurements; ne x 36: the information matrices, full
    const int32_t *aedge;                   // na: the active edges, ascending
    const int32_t *vslot, *svert;           // nv: the vertex's unknown block or -1; nf: the block's vertex
    const int32_t *csr_off, *csr_edge;      // nf + 1; positions in aedge of the block's incident active edges, ascending
    Envelope env;
    double *lin;                            // na x LIN: e[6], Ji[36], Jj[36], w
    double *H, *L;                          // the assembled envelope; the factor
    double *b, *x, *y, *d;                  // 6 nf each
    double *saved;                          // nf x 16
    Control* ctl; Report* rep;
};

// (H + lambda I) x = b on the envelope: un-pivoted scalar L D L^T, d_j = a_jj - sum_k l_jk^2 d_k, l_ij = (a_ij - sum_k l_ik l_jk d_k) / d_j, k ascending from
// the envelope start; y_i = b_i - sum_k l_ik y_k (k ascending); y_i / d_i; x_i = y_i - sum_k l_ki x_k (k DEscending from the last row that reaches column i).
// One column at a time, the rows of the column spread over the threads.  v.ctl->ok = 0 on a pivot that is not > 0 (x is then all zero).
template <class X> SSM_HD void factor_solve(const View& v, double lambda)
{
    const Envelope& E = v.env; const int N = 6 * v.nf;
    if (X::tid() == 0) v.ctl->ok = 1;
    X::sync();
    for (int j = 0; j < N; j++) {
        const int cj = j / 6, rmax = 6 * E.reach[cj] + 5, sj = env_start(E, j);
        for (int i = j + X::tid(); i <= rmax; i += X::nt()) {
            const int si = env_start(E, i);
            if (si > j) continue;
            double s = v.H[env_at(E, i, j)]; if (i == j) s += lambda;
            const int64_t oi = env_at(E, i, si) - si, oj = env_at(E, j, sj) - sj;
            // the chain is serial, its terms are not: eight products at a time, so that their 24 loads are in flight together; then subtracted in order
            int k = si > sj ? si : sj;
            for (; k + 8 <= j; k += 8) {
                double p[8];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
                for (int u = 0; u < 8; u++) p[u] = v.L[oi + k + u] * v.L[oj + k + u] * v.d[k + u];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
                for (int u = 0; u < 8; u++) s -= p[u];
            }
            for (; k < j; k++) s -= v.L[oi + k] * v.L[oj + k] * v.d[k];
            if (i == j) { v.d[j] = s; if (!(s > 0)) v.ctl->ok = 0; }
            else v.L[oi + j] = s;
        }
        X::sync();
        if (!v.ctl->ok) break;
        const double dj = v.d[j];
        for (int i = j + 1 + X::tid(); i <= rmax; i += X::nt()) {
            const int si = env_start(E, i);
            if (si > j) continue;
            const int64_t oi = env_at(E, i, si) - si;
            v.L[oi + j] = v.L[oi + j] / dj;
        }
        X::sync();
    }
    if (!v.ctl->ok) { for (int i = X::tid(); i < N; i += X::nt()) v.x[i] = 0.0; X::sync(); return; }
    for (int i = X::tid(); i < N; i += X::nt()) v.y[i] = v.b[i];
    X::sync();
    for (int k = 0; k < N; k++) {
        const int rmax = 6 * E.reach[k / 6] + 5; const double yk = v.y[k];
        for (int i = k + 1 + X::tid(); i <= rmax; i += X::nt()) {
            const int si = env_start(E, i);
            if (si > k) continue;
            v.y[i] -= v.L[env_at(E, i, si) - si + k] * yk;
        }
        X::sync();
    }
    for (int i = X::tid(); i < N; i += X::nt()) v.x[i] = v.y[i] / v.d[i];
    X::sync();
    for (int k = N - 1; k > 0; k--) {
        const int sk = env_start(E, k); const double xk = v.x[k]; const int64_t ok = env_at(E, k, sk) - sk;
        for (int i = sk + X::tid(); i < k; i += X::nt()) v.x[i] -= v.L[ok + i] * xk;
        X::sync();
    }
}
template <class X> SSM_HD double active_chi2(const View& v)
{
    return X::lane_sum(v.na, [&](int p) {
        const int e = v.aedge[p];
        return edge_rho(v.zinv + 16 * (size_t)e, v.pose + 16 * (size_t)v.efrom[e], v.pose + 16 * (size_t)v.eto[e], v.omega + 36 * (size_t)e, v.robust[e], nullptr);
    });
}
// linearise the active edges and assemble H (lower block envelope) and b: a block of H or b is the sum of its edges' contributions in ascending edge index
template <class X> SSM_HD void linearize_assemble(const View& v, bool stamp)
{
    const Envelope& E = v.env; const int N = 6 * v.nf;
    const long long t0 = X::clock();
    for (int p = X::tid(); p < v.na; p += X::nt()) {
        const int e = v.aedge[p]; double* l = v.lin + (size_t)LIN * p;
        const double* Xi = v.pose + 16 * (size_t)v.efrom[e]; const double* Xj = v.pose + 16 * (size_t)v.eto[e];
        edge_linearize(v.zinv + 16 * (size_t)e, Xi, Xj, l, l + 6, l + 42);
        double w = 1.0;
        if (v.robust[e]) { double r0; ssm_pnp::huber(quad_form(v.omega + 36 * (size_t)e, l), 1.0, r0, w); }
        l[78] = w; l[79] = 0.0;
    }
    const int64_t total = E.total;
    for (int64_t q = X::tid(); q < total; q += X::nt()) v.H[q] = 0.0;
    X::sync();
    const long long t1 = X::clock();
    for (int t = X::tid(); t < v.nf * 36; t += X::nt()) {
        const int r = t / 36, a = (t % 36) / 6, c = t % 6, vr = v.svert[r];
        for (int q = v.csr_off[r]; q < v.csr_off[r + 1]; q++) {
            const int p = v.csr_edge[q], e = v.aedge[p]; const double* l = v.lin + (size_t)LIN * p; const double* Om = v.omega + 36 * (size_t)e;
            const bool from = v.efrom[e] == vr;
            const double* Jr = from ? l + 6 : l + 42; const double* Jo = from ? l + 42 : l + 6;
            if (c <= a) v.H[env_at(E, 6 * r + a, 6 * r + c)] += contrib_entry(Jr, a, Om, l[78], Jr, c);
            const int o = v.vslot[from ? v.eto[e] : v.efrom[e]];
            if (o >= 0 && o < r) v.H[env_at(E, 6 * r + a, 6 * o + c)] += contrib_entry(Jr, a, Om, l[78], Jo, c);
        }
    }
    for (int t = X::tid(); t < N; t += X::nt()) {
        const int r = t / 6, a = t % 6, vr = v.svert[r];
        double s = 0.0;
        for (int q = v.csr_off[r]; q < v.csr_off[r + 1]; q++) {
            const int p = v.csr_edge[q], e = v.aedge[p]; const double* l = v.lin + (size_t)LIN * p;
            s -= contrib_rhs(v.efrom[e] == vr ? l + 6 : l + 42, a, v.omega + 36 * (size_t)e, l[78], l);
        }
        v.b[t] = s;
    }
    X::sync();
    if (stamp && X::tid() == 0) { const long long t2 = X::clock(); v.rep->clocks[0] += t1 - t0; v.rep->clocks[1] += t2 - t1; }
}
// SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg (tau 1e-5, at most 10 trials) on the active edges
template <class X> SSM_HD void run(const View& v, int iterations)
{
    const Envelope& E = v.env; const int N = 6 * v.nf;
    Control* c = v.ctl; Report* R = v.rep;
    if (X::tid() == 0) { c->lambda = 0; c->nu = 2; c->stop = 0; R->iterations = 0; R->solve_failures = 0; R->lambda = 0; for (int k = 0; k < NPHASE; k++) R->clocks[k] = 0; }
    X::sync();
    if (v.na == 0 || v.nf == 0) return;
    for (int it = 0; it < iterations; it++) {
        const double chi0 = active_chi2<X>(v);
        linearize_assemble<X>(v, true);
        if (X::tid() == 0) {
            c->chi = chi0; R->chi2_before[it] = chi0; R->accepted[it] = 0;
            if (it == 0) { double mx = 0; for (int j = 0; j < N; j++) { const double dg = fabs(v.H[env_at(E, j, j)]); if (dg > mx) mx = dg; } c->lambda = 1e-5 * mx; c->nu = 2; }
        }
        X::sync();
        int trials = 0; double gain = 0;
        do {
            long long t0 = X::clock();
            for (int t = X::tid(); t < v.nf * 16; t += X::nt()) v.saved[t] = v.pose[16 * (size_t)v.svert[t / 16] + t % 16];
            const double lambda = c->lambda;
            factor_solve<X>(v, lambda);
            const bool ok = c->ok != 0;
            long long t1 = X::clock();
            if (ok) for (int r = X::tid(); r < v.nf; r += X::nt()) {
                double D[16], P[16]; double* T = v.pose + 16 * (size_t)v.svert[r];
                from_mqt(v.x + 6 * r, D); ssm_pnp::iso_mul(T, D, P);
                for (int k = 0; k < 16; k++) T[k] = P[k];
            }
            X::sync();
            const double chi_new = active_chi2<X>(v);
            const double scale = X::lane_sum(N, [&](int j) { return v.x[j] * (lambda * v.x[j] + v.b[j]); });
            long long t2 = X::clock();
            if (X::tid() == 0) {
                LmState st; st.lambda = c->lambda; st.nu = c->nu;
                double g; const bool acc = lm_update_scaled(st, c->chi, chi_new, ok, scale, g);
                c->lambda = st.lambda; c->nu = st.nu; c->gain = g; c->accepted = acc; c->chi_new = chi_new; c->scale = scale;
                if (acc) { c->chi = chi_new; R->accepted[it] |= 1u << trials; }
                if (!ok) R->solve_failures++;
                R->gain[it][trials] = g;
            }
            X::sync();
            const bool acc = c->accepted != 0; gain = c->gain; const bool lam_ok = isfinite(c->lambda);
            if (!acc) { for (int t = X::tid(); t < v.nf * 16; t += X::nt()) v.pose[16 * (size_t)v.svert[t / 16] + t % 16] = v.saved[t]; }
            X::sync();
            if (X::tid() == 0) { const long long t3 = X::clock(); R->clocks[2] += t1 - t0; R->clocks[3] += t2 - t1; R->clocks[4] += t3 - t2; }
            trials++;
            if (!acc && !lam_ok) break;
        } while (gain < 0 && trials < MAX_TRIALS);
        if (X::tid() == 0) { R->trials[it] = trials; R->chi2_after[it] = c->chi; R->iterations = it + 1; R->lambda = c->lambda; }
        X::sync();
        if (trials == MAX_TRIALS || gain == 0) break;
    }
}

// ---- the host executor: one thread walks every loop; the lane sums are pnp_core.h's tree
struct HostExec {
    static int tid() { return 0; }
    static int nt() { return 1; }
    static void sync() {}
    static long long clock() { return 0; }
    template <class Term> static double lane_sum(int n, Term term)
    {
        double r;
        ssm_pnp::lane_sum<1>(n, [&](int i, double* acc) { acc[0] += term(i); }, &r);
        return r;
    }
};
}  // namespace ssm_pgc
