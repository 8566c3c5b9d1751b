// grid_core.h -- the arithmetic of the ground grid: the points of m posed clouds are dropped into a horizontal grid of square cells; per cell the
// ground height is the lowest point of its neighbourhood, the cell's points split into LOW (ground) and HIGH (standing on it), and the cell gets a state, two
// majority labels, two heights and a class.  Compiled for host and device like render_core.h: csrc/kernels_grid.hip and the host function of
// csrc/ssm_grid_host.cpp call the same functions, so device == host bit for bit.  Every translation unit that includes this is built with -ffp-contract=off.
// Every accumulator is an integer: the result does not depend on the order of points or clouds.  The reference has no such step.
#pragma once
#include "carve_core.h"
#include "../ssm_hip.h"

namespace ssm_gridc {

static const int NLABEL = 12;
static const int MAX_GROUND_RADIUS = 4;
static const int64_t MAX_CELLS = (int64_t)1 << 24;
static const int64_t MAX_POINTS = (int64_t)1 << 31;             // a call with this many points or more is refused: |sum_low| < 2^61
static const double H_LIMIT = 1048576.0;                        // |h_min|, |h_max| <= 2^20 m: |hq| <= 2^30
static const double H_UNIT = 1024.0;                            // heights are integers in units of 2^-10 m
enum { UNOBSERVED = 0, DRIVABLE = 1, WALKABLE = 2, OTHER_GROUND = 3, OBSTACLE = 4 };          // a cell's class
enum { P_REJECTED = 0, P_OUT_OF_BAND = 1, P_OUTSIDE = 2, P_USED = 3 };                          // what becomes of a point
enum { LABEL_ROAD_MARKING = 3, LABEL_ROAD = 4, LABEL_PAVEMENT = 5, LABEL_NONE = 255 };
static const int32_t Q_NONE = INT32_MIN;                        // the heights of an unobserved cell
static const int32_t HMIN_EMPTY = INT32_MAX, HMAX_EMPTY = INT32_MIN, BASE_EMPTY = INT32_MAX;          // the raw accumulators of a cell no point fell into

// what a call's parameters become once
struct Setup { double x0, y0, cell, h_min, h_max; int64_t step_q; int32_t nx, ny, ground_radius, min_obstacle_points; };
struct Hit { int32_t cx, cy, hq; };
// step in height units; two heights of the band differ by at most 2^31 units, so a step of 2^32 m and more is as good as 2^42 units (and stays an integer)
inline int64_t step_units(double step) { return step >= 4294967296.0 ? (int64_t)1 << 42 : (int64_t)llrint(step * H_UNIT); }

// host only: M = G . T_cloud (G row-major 3 x 4 [R | t], T_cloud column-major 4 x 4) -> 12 doubles, row-major 3 x 4:
// M[i][j] = (G[i][0] T[0][j] + G[i][1] T[1][j]) + G[i][2] T[2][j], and for j = 3 the same + G[i][3] last
inline void grid_pose(const double G[12], const double Tc[16], double M[12])
{
    for (int i = 0; i < 3; i++) {
        const double a = G[i * 4 + 0], b = G[i * 4 + 1], c = G[i * 4 + 2];
        for (int j = 0; j < 3; j++) M[i * 4 + j] = (a * Tc[j * 4 + 0] + b * Tc[j * 4 + 1]) + c * Tc[j * 4 + 2];
        M[i * 4 + 3] = ((a * Tc[12] + b * Tc[13]) + c * Tc[14]) + G[i * 4 + 3];
    }
}
// host only: G for a world whose up and forward directions are given (plain doubles, this operation order): z = up / |up| with |up| = sqrt((u0 u0 + u1 u1) + u2 u2);
// d = (f0 z0 + f1 z1) + f2 z2; y = f - d z, normalised the same way; x = y cross z with x0 = y1 z2 - y2 z1, x1 = y2 z0 - y0 z2, x2 = y0 z1 - y1 z0.  The rows of G are
// x, y, z, its translation 0.  false: a non-finite entry, an up of length 0, or a forward along up
inline bool frame_from_up(const double up[3], const double fw[3], double G[12])
{
    using ssm_carvec::finite_d;
    for (int i = 0; i < 3; i++) if (!(finite_d(up[i]) && finite_d(fw[i]))) return false;
    const double lu = sqrt((up[0] * up[0] + up[1] * up[1]) + up[2] * up[2]);
    if (!(lu > 0.0 && finite_d(lu))) return false;
    const double z[3] = {up[0] / lu, up[1] / lu, up[2] / lu};
    const double d = (fw[0] * z[0] + fw[1] * z[1]) + fw[2] * z[2];
    const double yr[3] = {fw[0] - d * z[0], fw[1] - d * z[1], fw[2] - d * z[2]};
    const double ly = sqrt((yr[0] * yr[0] + yr[1] * yr[1]) + yr[2] * yr[2]);
    if (!(ly > 0.0 && finite_d(ly))) return false;
    const double y[3] = {yr[0] / ly, yr[1] / ly, yr[2] / ly};
    const double x[3] = {y[1] * z[2] - y[2] * z[1], y[2] * z[0] - y[0] * z[2], y[0] * z[1] - y[1] * z[0]};
    for (int j = 0; j < 3; j++) { G[j] = x[j]; G[4 + j] = y[j]; G[8 + j] = z[j]; }
    G[3] = G[7] = G[11] = 0.0;
    for (int i = 0; i < 12; i++) if (!finite_d(G[i])) return false;
    return true;
}

// what becomes of the point (x, y, z) of a cloud whose grid pose is M; P_USED: *out is its cell and quantised height
CARVE_HD int point_of(float xf, float yf, float zf, const double* M, const Setup& S, Hit* out)
{
    using ssm_carvec::finite_d;
    const double x = (double)xf, y = (double)yf, z = (double)zf;
    if (!(finite_d(x) && finite_d(y) && finite_d(z))) return P_REJECTED;
    const double qx = M[0] * x + M[1] * y + M[2] * z + M[3];
    const double qy = M[4] * x + M[5] * y + M[6] * z + M[7];
    const double qz = M[8] * x + M[9] * y + M[10] * z + M[11];
    if (!(finite_d(qx) && finite_d(qy) && finite_d(qz))) return P_REJECTED;
    if (!(S.h_min <= qz && qz <= S.h_max)) return P_OUT_OF_BAND;
    const double cxd = floor((qx - S.x0) / S.cell), cyd = floor((qy - S.y0) / S.cell);
    // (the comparison is made as doubles and is false for NaN; only a value that passes ever becomes an int)
    if (!(cxd >= 0.0 && cxd <= (double)(S.nx - 1) && cyd >= 0.0 && cyd <= (double)(S.ny - 1))) return P_OUTSIDE;
    out->cx = (int32_t)cxd; out->cy = (int32_t)cyd;
    out->hq = (int32_t)llrint(qz * H_UNIT);                      // (|qz| <= 2^20: |hq| <= 2^30)
    return P_USED;
}
CARVE_HD bool is_low(int32_t hq, int32_t base, int64_t step_q) { return (int64_t)hq <= (int64_t)base + step_q; }
// floor toward minus infinity of a / b, b > 0
CARVE_HD int64_t floor_div(int64_t a, int64_t b) { int64_t q = a / b; if (a % b != 0 && a < 0) q--; return q; }
// the fullest bin, the lowest id on a tie, 255 when all are zero
CARVE_HD uint8_t majority_of(const uint32_t* hist)
{
    uint32_t best = 0; uint8_t l = LABEL_NONE;
    for (int i = 0; i < NLABEL; i++) if (hist[i] > best) { best = hist[i]; l = (uint8_t)i; }
    return l;
}
struct Resolved { uint8_t cls, ground_label, obstacle_label; int32_t ground_q, top_q; };
CARVE_HD Resolved resolve_of(const ssm_grid_cell& c, int32_t min_obstacle_points)
{
    Resolved r;
    if (c.n == 0) { r.cls = UNOBSERVED; r.ground_label = r.obstacle_label = LABEL_NONE; r.ground_q = r.top_q = Q_NONE; return r; }
    const bool obstacle = c.n_high >= (uint32_t)min_obstacle_points;
    r.ground_q = c.n_low ? (int32_t)floor_div(c.sum_low, (int64_t)c.n_low) : c.base;
    r.top_q = c.hmax;
    r.ground_label = majority_of(c.hist_low);
    r.obstacle_label = obstacle ? majority_of(c.hist_high) : (uint8_t)LABEL_NONE;
    r.cls = obstacle ? OBSTACLE : (r.ground_label == LABEL_ROAD || r.ground_label == LABEL_ROAD_MARKING) ? DRIVABLE : r.ground_label == LABEL_PAVEMENT ? WALKABLE : OTHER_GROUND;
    return r;
}

}      // namespace ssm_gridc
