// align_core.h -- the arithmetic of dense alignment: projective point-to-plane ICP of the points of m posed clouds against a key-frame's depth
// image (the VIEW).  Compiled for host and device like carve_core.h and render_core.h: csrc/kernels_align.hip and the host function of csrc/ssm_align_host.cpp
// call the same functions, so device == host bit for bit.  Every translation unit that includes this is built with -ffp-contract=off.  The relative poses are
// carve_core.h's rel_pose (host only, evaluated ONCE per call and cloud; both paths are handed their 12 doubles).  What is here: the view's normal map (one
// pixel), one point's contribution to the normal equations as 64-bit integers, and the bound that keeps their sums inside 63 bits.  The solve (pnp_core.h's
// solve_ldlt and pose_oplus) runs on the host on both paths: ssm_align_host.cpp align_drive.  The reference has no such step.
//
// STORED FORMAT of the view: per pixel one Normal of 16 bytes, three floats -- the double normal rounded ONCE -- and a zero pad; an invalid pixel holds (0, 0, 0).
// The vertex is not stored: both paths recompute it in double from the depth image (vertex_of), which is cheaper than another 24 bytes per gather.
// SUMS: every real-valued contribution becomes an integer once, llrint(term * 2^S) in double, S = S_HB for the 21 + 6 entries of H and b and S_CHI for the
// robustified chi2, and is added as int64: exact, hence independent of order, block shape and launch geometry.
#pragma once
#include "carve_core.h"
#include "pnp_core.h"

namespace ssm_alignc {

enum { MAX_ITER = 0, CONVERGED = 1, TOO_FEW = 2, DEGENERATE = 3, DIVERGED = 4 };          // ssm_align_info.status
enum { S_HB = 20, S_CHI = 30 };
enum { NH = 21, NB = 6, I_B = 21, I_CHI = 27, I_TESTED = 28, I_INLIER = 29, NSUM = 30 };  // the layout of one iteration's sums
static const int MAX_ITERATIONS = 64;
static const int MAX_STRIDE = 1 << 20;
static const int64_t MAX_PIXELS = (int64_t)1 << 26;
static const double SUM_LIMIT = 4611686018427387904.0;          // 2^62

struct Normal { float x, y, z, pad; };
// what a call's parameters and the view's camera become once
struct Setup { double fx, fy, cx, cy, scale, z_min, z_max, dist_max, delta; int32_t w, h; int64_t tol_abs, ppm; };

using ssm_carvec::finite_d;

// the vertex of pixel (x, y) with depth d (> 0): ((x - cx) z / fx, (y - cy) z / fy, z), z = d / scale
CARVE_HD void vertex_of(int x, int y, int32_t d, const Setup& S, double* V)
{
    const double z = (double)d / S.scale;
    V[0] = (((double)x - S.cx) * z) / S.fx; V[1] = (((double)y - S.cy) * z) / S.fy; V[2] = z;
}
// s.16's tolerance at depth d, and the depth-edge gate of one neighbour
CARVE_HD bool edge_ok(int32_t d, int32_t dn, const Setup& S)
{
    if (dn <= 0) return false;
    const int64_t tol = S.tol_abs + ((int64_t)d * S.ppm) / 1000000;
    const int64_t diff = dn > d ? (int64_t)(dn - d) : (int64_t)(d - dn);
    return diff <= tol;
}
// the normal of pixel (x, y) of the view; false (and a zero normal in *out): the pixel is invalid
CARVE_HD bool normal_of(const uint16_t* depth, int x, int y, const Setup& S, Normal* out)
{
    out->x = 0.0f; out->y = 0.0f; out->z = 0.0f; out->pad = 0.0f;
    if (x < 1 || y < 1 || x > S.w - 2 || y > S.h - 2) return false;
    const uint16_t* row = depth + (size_t)y * (size_t)S.w + (size_t)x;
    const int32_t d = row[0];
    if (d == 0) return false;
    const int32_t dl = row[-1], dr = row[1], du = row[-(ptrdiff_t)S.w], dd = row[S.w];
    if (!(edge_ok(d, dl, S) && edge_ok(d, dr, S) && edge_ok(d, du, S) && edge_ok(d, dd, S))) return false;
    double Vl[3], Vr[3], Vu[3], Vd[3], V[3];
    vertex_of(x - 1, y, dl, S, Vl); vertex_of(x + 1, y, dr, S, Vr); vertex_of(x, y - 1, du, S, Vu); vertex_of(x, y + 1, dd, S, Vd); vertex_of(x, y, d, S, V);
    const double a0 = Vr[0] - Vl[0], a1 = Vr[1] - Vl[1], a2 = Vr[2] - Vl[2];
    const double b0 = Vd[0] - Vu[0], b1 = Vd[1] - Vu[1], b2 = Vd[2] - Vu[2];
    const double c0 = a1 * b2 - a2 * b1, c1 = a2 * b0 - a0 * b2, c2 = a0 * b1 - a1 * b0;
    const double len2 = (c0 * c0 + c1 * c1) + c2 * c2;
    if (!(finite_d(len2) && len2 > 0.0)) return false;
    const double len = sqrt(len2);
    double n0 = c0 / len, n1 = c1 / len, n2 = c2 / len;
    const double dot = (n0 * V[0] + n1 * V[1]) + n2 * V[2];
    if (!(finite_d(dot)) || dot == 0.0) return false;
    if (dot > 0.0) { n0 = -n0; n1 = -n1; n2 = -n2; }
    const float f0 = (float)n0, f1 = (float)n1, f2 = (float)n2;
    if (f0 == 0.0f && f1 == 0.0f && f2 == 0.0f) return false;
    out->x = f0; out->y = f1; out->z = f2;
    return true;
}

CARVE_HD int64_t to_units(double term, int s) { return (int64_t)llrint(term * (double)((int64_t)1 << s)); }

// the contribution of the point (x, y, z) of a cloud whose relative pose is M (3 x 4, row-major) under the increment E (3 x 4, row-major): added to acc[NSUM]
CARVE_HD void point_terms(float xf, float yf, float zf, const double* M, const double* E, const uint16_t* depth, const Normal* normals, const Setup& S, int64_t* acc)
{
    const double x = (double)xf, y = (double)yf, z = (double)zf;
    if (!(finite_d(x) && finite_d(y) && finite_d(z))) return;
    const double ax = M[0] * x + M[1] * y + M[2] * z + M[3];
    const double ay = M[4] * x + M[5] * y + M[6] * z + M[7];
    const double az = M[8] * x + M[9] * y + M[10] * z + M[11];
    const double qx = E[0] * ax + E[1] * ay + E[2] * az + E[3];
    const double qy = E[4] * ax + E[5] * ay + E[6] * az + E[7];
    const double qz = E[8] * ax + E[9] * ay + E[10] * az + E[11];
    if (!(finite_d(qx) && finite_d(qy) && finite_d(qz)) || qz < S.z_min || qz > S.z_max) return;
    const double u = S.fx * (qx / qz) + S.cx, v = S.fy * (qy / qz) + S.cy;
    const double pxd = floor(u + 0.5), pyd = floor(v + 0.5);
    // (the comparisons are false for NaN; only a value inside the image ever becomes an int)
    if (!(pxd >= 0.0 && pxd <= (double)(S.w - 1) && pyd >= 0.0 && pyd <= (double)(S.h - 1))) return;
    const int px = (int)pxd, py = (int)pyd;
    const size_t at = (size_t)py * (size_t)S.w + (size_t)px;
    const Normal nf = normals[at];
    if (nf.x == 0.0f && nf.y == 0.0f && nf.z == 0.0f) return;
    acc[I_TESTED] += 1;
    double V[3]; vertex_of(px, py, (int32_t)depth[at], S, V);
    const double n0 = (double)nf.x, n1 = (double)nf.y, n2 = (double)nf.z;
    const double r = (n0 * (qx - V[0]) + n1 * (qy - V[1])) + n2 * (qz - V[2]);
    if (!(fabs(r) <= S.dist_max)) return;
    double rho0, w; ssm_pnp::huber(r * r, S.delta, rho0, w);
    const double J[6] = {qy * n2 - qz * n1, qz * n0 - qx * n2, qx * n1 - qy * n0, n0, n1, n2};
    const double wr = -(w * r);
    acc[I_INLIER] += 1;
    acc[I_CHI] += to_units(rho0, S_CHI);
    int q = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int a = 0; a < 6; a++) {
        const double wj = w * J[a];
        acc[I_B + a] += to_units(wr * J[a], S_HB);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int c = 0; c <= a; c++) { acc[q] += to_units(wj * J[c], S_HB); q++; }
    }
}

// host only: the largest magnitude one point can add to any sum, in units.  A point that contributes projects inside the image, so |q.x / q.z| <= tx and
// |q.y / q.z| <= ty with tx = (max(|cx|, |w - 1 - cx|) + 0.5) / |fx| (ty alike), and q.z <= z_max: |q| <= Q = z_max sqrt(1 + tx^2 + ty^2).  The stored normal is a
// unit vector rounded to float, |n| <= 1 + 2^-22, so every entry of J = [q x n, n] is at most Jm = max(Q, 1) (1 + 2^-22); the weight is at most 1, |r| <= dist_max
// and rho0 <= r^2.  Hence |H term| <= Jm^2, |b term| <= dist_max Jm, chi2 term <= dist_max^2; one more unit covers llrint.  Non-finite: no bound (fx or fy 0).
inline double term_bound_units(const Setup& S)
{
    const double tx = (fmax(fabs(S.cx), fabs((double)(S.w - 1) - S.cx)) + 0.5) / fabs(S.fx), ty = (fmax(fabs(S.cy), fabs((double)(S.h - 1) - S.cy)) + 0.5) / fabs(S.fy);
    const double Q = S.z_max * sqrt(1.0 + tx * tx + ty * ty);
    const double Jm = fmax(Q, 1.0) * (1.0 + 1.0 / 4194304.0);
    const double hb = fmax(Jm * Jm, S.dist_max * Jm) * (double)((int64_t)1 << S_HB), chi = (S.dist_max * S.dist_max) * (double)((int64_t)1 << S_CHI);
    return fmax(hb, chi) + 1.0;
}
inline bool sums_fit(const Setup& S, int64_t n_points)
{
    const double b = term_bound_units(S);
    return finite_d(b) && (double)n_points * b < SUM_LIMIT;
}

}      // namespace ssm_alignc
