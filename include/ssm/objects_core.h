// objects_core.h -- the arithmetic of object extraction: the OBSTACLE cells of a built ground grid (grid_core.h) whose label is one of the wanted
// classes form connected components; a component with enough cells, points and height is an object, and every HIGH point of the grid's clouds that fell into one of
// its cells is a point of it.  Compiled for host and device like grid_core.h: csrc/kernels_objects.hip and the host functions of csrc/ssm_objects_host.cpp call the
// same functions, so device == host bit for bit.  Every translation unit that includes this is built with -ffp-contract=off.  Every figure is an integer: nothing
// depends on the order of cells, points or clouds.  The reference has no such step.
#pragma once
#include "grid_core.h"

namespace ssm_objc {

static const double XY_LIMIT = 1048576.0;                       // the grid's extent stays within +-2^20 m: |x_q|, |y_q| <= 2^30 (a little rounding included)
static const double Q_UNIT = 1024.0;                            // coordinates are integers in units of 2^-10 m, as the grid's heights
enum { KEPT = 0, REJECT_CELLS = 1, REJECT_POINTS = 2, REJECT_HEIGHT = 3 };

// what a call's parameters become once
struct Setup { uint32_t label_mask; int32_t connectivity, min_cells, min_points; int64_t min_height_q; };
// min_height in height units; a component's height is below 2^32 units, so 2^22 m and more is as good as 2^42 units (and stays an integer)
inline int64_t height_units(double min_height) { return min_height >= 4194304.0 ? (int64_t)1 << 42 : (int64_t)llrint(min_height * Q_UNIT); }
// does the grid's extent [x0, x0 + nx cell] x [y0, y0 + ny cell] stay within the limit?  (false for a non-finite corner)
inline bool extent_fits(double x0, double y0, double cell, int nx, int ny)
{
    const double x1 = x0 + (double)nx * cell, y1 = y0 + (double)ny * cell;
    return fabs(x0) <= XY_LIMIT && fabs(x1) <= XY_LIMIT && fabs(y0) <= XY_LIMIT && fabs(y1) <= XY_LIMIT;
}

// is the cell one of those that form components?
CARVE_HD bool member(uint8_t cls, uint8_t obstacle_label, uint32_t label_mask)
{ return cls == ssm_gridc::OBSTACLE && obstacle_label < ssm_gridc::NLABEL && ((label_mask >> obstacle_label) & 1u) != 0; }
// the first rule a component fails, in this order: cells, points, height
CARVE_HD int verdict_of(uint32_t cells, uint64_t cell_points, int32_t ground_q, int32_t top_q, const Setup& S)
{
    if ((int64_t)cells < (int64_t)S.min_cells) return REJECT_CELLS;
    if (cell_points < (uint64_t)S.min_points) return REJECT_POINTS;
    if ((int64_t)top_q - (int64_t)ground_q < S.min_height_q) return REJECT_HEIGHT;
    return KEPT;
}
// a record before anything is added to it
CARVE_HD void clear_cells(ssm_object* o)
{
    o->root = -1; o->label = -1; o->cells = 0; o->cell_points = 0; o->cx_min = o->cy_min = INT32_MAX; o->cx_max = o->cy_max = INT32_MIN;
    o->ground_q = INT32_MAX; o->top_q = INT32_MIN;
}
CARVE_HD void clear_points(ssm_object* o)
{
    o->n_points = 0; o->n_label = 0; o->pad = 0; o->x_min_q = o->y_min_q = o->z_min_q = INT32_MAX; o->x_max_q = o->y_max_q = o->z_max_q = INT32_MIN;
    o->sum_x = o->sum_y = o->sum_z = 0;
}

struct Hit { int32_t cell, hq, xq, yq, zq; };
// What becomes of the point (x, y, z) of a cloud whose grid pose is M under the grid's setup G: grid_core.h's status; P_USED: its cell (cy nx + cx), its quantised
// height and its quantised grid coordinates.  qx, qy, qz are grid_core.h point_of's expressions restated: the same bits, so the same cell and height.
CARVE_HD int point_of(float xf, float yf, float zf, const double* M, const ssm_gridc::Setup& G, Hit* out)
{
    ssm_gridc::Hit h;
    const int st = ssm_gridc::point_of(xf, yf, zf, M, G, &h);
    if (st != ssm_gridc::P_USED) return st;
    const double x = (double)xf, y = (double)yf, z = (double)zf;
    const double qx = M[0] * x + M[1] * y + M[2] * z + M[3];
    const double qy = M[4] * x + M[5] * y + M[6] * z + M[7];
    const double qz = M[8] * x + M[9] * y + M[10] * z + M[11];
    out->cell = h.cy * G.nx + h.cx; out->hq = h.hq;
    out->xq = (int32_t)llrint(qx * Q_UNIT); out->yq = (int32_t)llrint(qy * Q_UNIT); out->zq = (int32_t)llrint(qz * Q_UNIT);          // (|qx|, |qy| within the extent, |qz| <= 2^20)
    return st;
}

}      // namespace ssm_objc
