// carve_core.h -- the arithmetic of free-space carving: a later key-frame's depth image (the VIEW) judges the points of an earlier key-frame's
// camera-frame cloud, and a point the view has seen through min_votes times in a row leaves its cloud.  Compiled for host and device like sor_core.h and
// motion_fuse_core.h: csrc/kernels_carve.hip and the host function of csrc/ssm_carve_host.cpp call the same functions, so device == host bit for bit.  Every
// translation unit that includes this is built with -ffp-contract=off.  What is here: the relative pose (host only, evaluated ONCE per view and cloud; both paths
// are handed its 12 doubles), the verdict of one point and the update of its run counter.  The reference has no such step.
#pragma once
#include <stdint.h>
#include <math.h>
#include <float.h>
#if defined(__HIPCC__)
#define CARVE_HD __host__ __device__ inline
#else
#define CARVE_HD inline
#endif

namespace ssm_carvec {

enum { UNKNOWN = 0, OCCLUDED = 1, SUPPORTED = 2, SEEN_THROUGH = 3 };
static const int MAX_RADIUS = 3;
static const int MAX_RUN = 255;
static const double ZQ_LIMIT = 1125899906842624.0;      // 2^50 depth units: q.z * scale saturates here before it becomes an integer (a depth is below 2^16, a tolerance below 2^41)
static const double TOL_ABS_MAX = 1.0e6;                // metres
static const double SCALE_MAX = 1.0e6;                  // depth units per metre
static const int32_t PPM_MAX = 1000000;

CARVE_HD bool finite_d(double v) { return fabs(v) <= DBL_MAX; }          // false for NaN

// what a call's parameters and the view's camera become once: everything a point's verdict reads besides the 12 doubles and the depth image
struct Setup { double fx, fy, cx, cy, scale, z_min; int32_t w, h, r; int64_t tol_abs, ppm; };
CARVE_HD int64_t tol_abs_units(double tol_abs, double scale) { return (int64_t)llrint(tol_abs * scale); }

// host only: T_rel = inverse(T_view) . T_cloud of two rigid 4x4 poses (column-major, as Eigen stores them) -> 12 doubles, row-major 3x4 [R | t].
// inverse(T_view) = (Ri, ti) with Ri = Rv^T and ti[i] = -((Ri[i][0] tv[0] + Ri[i][1] tv[1]) + Ri[i][2] tv[2]); then
// R[i][j] = (Ri[i][0] Rc[0][j] + Ri[i][1] Rc[1][j]) + Ri[i][2] Rc[2][j] and t[i] = ((Ri[i][0] tc[0] + Ri[i][1] tc[1]) + Ri[i][2] tc[2]) + ti[i]
inline void rel_pose(const double Tv[16], const double Tc[16], double M[12])
{
    for (int i = 0; i < 3; i++) {
        const double a = Tv[i * 4 + 0], b = Tv[i * 4 + 1], c = Tv[i * 4 + 2];          // row i of Rv^T = column i of Rv
        const double ti = -((a * Tv[12] + b * Tv[13]) + c * Tv[14]);
        for (int j = 0; j < 3; j++) M[i * 4 + j] = (a * Tc[j * 4 + 0] + b * Tc[j * 4 + 1]) + c * Tc[j * 4 + 2];
        M[i * 4 + 3] = ((a * Tc[12] + b * Tc[13]) + c * Tc[14]) + ti;
    }
}

// the verdict of the point (x, y, z) of a cloud whose relative pose is M, under the view `depth` (w x h, row-major, device or host memory alike), and the pixel
// it was decided at: (*px_out, *py_out) is written for every verdict but UNKNOWN-before-the-window (then both stay as they were).  Label fusion
// (relabel_core.h) reads the view's label there; verdict_of below is this function with the pixel dropped
CARVE_HD int verdict_at(float xf, float yf, float zf, const double* M, const uint16_t* depth, const Setup& S, int* px_out, int* py_out)
{
    const double x = (double)xf, y = (double)yf, z = (double)zf;
    if (!(finite_d(x) && finite_d(y) && finite_d(z))) return UNKNOWN;
    const double qx = M[0] * x + M[1] * y + M[2] * z + M[3];
    const double qy = M[4] * x + M[5] * y + M[6] * z + M[7];
    const double qz = M[8] * x + M[9] * y + M[10] * z + M[11];
    if (!(finite_d(qx) && finite_d(qy) && finite_d(qz)) || qz < S.z_min) return UNKNOWN;
    const double u = S.fx * (qx / qz) + S.cx, v = S.fy * (qy / qz) + S.cy;
    const double pxd = floor(u + 0.5), pyd = floor(v + 0.5);
    const double r = (double)S.r;
    // (the comparisons are false for NaN; only a value inside the image ever becomes an int)
    if (!(pxd >= r && pxd <= (double)(S.w - 1) - r && pyd >= r && pyd <= (double)(S.h - 1) - r)) return UNKNOWN;
    const int px = (int)pxd, py = (int)pyd;
    *px_out = px; *py_out = py;
    int32_t dmin = 65536;
    for (int dy = -S.r; dy <= S.r; dy++) {
        const uint16_t* row = depth + (size_t)(py + dy) * (size_t)S.w + (size_t)(px - S.r);
        for (int dx = 0; dx <= 2 * S.r; dx++) { const int32_t e = row[dx]; dmin = e < dmin ? e : dmin; }
    }
    if (dmin == 0) return UNKNOWN;
    const int64_t d = depth[(size_t)py * (size_t)S.w + (size_t)px];
    const double zs = qz * S.scale;
    const int64_t zq = zs < ZQ_LIMIT ? (int64_t)llrint(zs) : (int64_t)ZQ_LIMIT;
    const int64_t tol = S.tol_abs + (d * S.ppm) / 1000000;
    if (zq + tol < (int64_t)dmin) return SEEN_THROUGH;
    const int64_t diff = zq > d ? zq - d : d - zq;
    return diff <= tol ? SUPPORTED : OCCLUDED;
}
CARVE_HD int verdict_of(float xf, float yf, float zf, const double* M, const uint16_t* depth, const Setup& S)
{
    int px = 0, py = 0;
    return verdict_at(xf, yf, zf, M, depth, S, &px, &py);
}
CARVE_HD uint8_t run_after(uint8_t run, int verdict)
{
    if (verdict == SEEN_THROUGH) return run < MAX_RUN ? (uint8_t)(run + 1) : (uint8_t)MAX_RUN;
    if (verdict == SUPPORTED) return 0;
    return run;
}
CARVE_HD bool leaves(uint8_t run, int min_votes) { return (int)run >= min_votes; }

}      // namespace ssm_carvec
