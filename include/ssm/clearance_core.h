// clearance_core.h -- the arithmetic of the clearance map: from the class image of a built ground grid (grid_core.h) every cell gets the exact
// squared Euclidean distance, in cells, to the nearest BLOCKED cell and that cell's index; the free cells farther than a vehicle radius from everything blocked
// are TRAVERSABLE, and those connected to a seed cell are REACHABLE.  Compiled for host and device like objects_core.h: csrc/kernels_clearance.hip and the host
// function of csrc/ssm_clearance_host.cpp call the same functions, so device == host bit for bit.  Every figure the kernels see is an integer: nothing depends on
// the order of cells.  The reference has no such step.
#pragma once
#include "grid_core.h"

namespace ssm_clrc {

static const int NCLASS = 5;                                    // grid_core.h's cell classes 0 .. 4
static const int MAX_SIDE = 32768;                              // nx, ny <= 2^15: dx^2 + dy^2 <= 2 (2^15 - 1)^2 < 2^31
static const int MAX_SNAP = 1024;                               // seed_snap <= 2^10: a snap distance squared fits the key as well
static const int64_t R2_MAX = (int64_t)1 << 31;                 // r2 saturates here: above every distance a grid can hold
static const uint32_t D2_NONE = UINT32_MAX;                     // dist2 when no cell is blocked (nearest is then -1)
static const unsigned long long KEY_NONE = ~0ull;               // the key of "no cell"
enum { NOT_TRAVERSABLE = 0, TRAVERSABLE = 1, REACHABLE = 2 };   // reach

// what a call's parameters become once
struct Setup { uint32_t blocked_mask, free_mask; int64_t r2; int32_t connectivity, seed_cx, seed_cy, seed_snap; };

// host only: r2 = floor((radius / cell)^2), saturated at 2^31 (radius >= 0 and cell > 0, both finite: the callers check)
inline int64_t r2_of(double radius, double cell)
{
    const double q = radius / cell, q2 = q * q;
    if (!(q2 < 2147483648.0)) return R2_MAX;
    return (int64_t)floor(q2);
}
// host only: the cell of the point (x, y) of the grid frame -- grid_core.h point_of's floor expressions restated; false: outside the grid (or not a number)
inline bool cell_of(const ssm_grid_params& P, double x, double y, int32_t* cx, int32_t* cy)
{
    const double cxd = floor((x - P.x0) / P.cell), cyd = floor((y - P.y0) / P.cell);
    if (!(cxd >= 0.0 && cxd <= (double)(P.nx - 1) && cyd >= 0.0 && cyd <= (double)(P.ny - 1))) return false;
    *cx = (int32_t)cxd; *cy = (int32_t)cyd;
    return true;
}

CARVE_HD bool in_mask(uint8_t cls, uint32_t mask) { return cls < NCLASS && ((mask >> cls) & 1u) != 0; }
// the squared distance of two cells dx columns and dy rows apart (|dx|, |dy| < 2^15)
CARVE_HD uint32_t d2_of(int32_t dx, int32_t dy) { return (uint32_t)(dx * dx) + (uint32_t)(dy * dy); }
// what the minimum is taken of: the squared distance above the 24 bits of the cell index
CARVE_HD unsigned long long key_of(uint32_t d2, int32_t index) { return ((unsigned long long)d2 << 24) | (unsigned long long)(uint32_t)index; }
// is (d2, index) a smaller key than (best_d2, best_index)?  (the 32-bit form of key_of(a) < key_of(b); best_index < 0: nothing yet)
CARVE_HD bool better(uint32_t d2, int32_t index, uint32_t best_d2, int32_t best_index)
{ return best_index < 0 || d2 < best_d2 || (d2 == best_d2 && index < best_index); }
// the nearer of two blocked rows of one column as seen from row cy: lo <= cy (-1: none), hi >= cy (-1: none); the lower row on a tie
CARVE_HD int32_t nearer_row(int32_t cy, int32_t lo, int32_t hi)
{
    if (lo < 0) return hi;
    if (hi < 0) return lo;
    return cy - lo <= hi - cy ? lo : hi;
}
CARVE_HD bool traversable(uint8_t cls, uint32_t dist2, uint32_t free_mask, int64_t r2) { return in_mask(cls, free_mask) && (int64_t)dist2 > r2; }
// the seed's key of the cell (cx, cy): KEY_NONE when it is farther than seed_snap from the seed (the caller has tested that it is traversable)
CARVE_HD unsigned long long seed_key(int32_t cx, int32_t cy, int32_t nx, const Setup& S)
{
    const int32_t dx = cx - S.seed_cx, dy = cy - S.seed_cy;
    if (dx < -S.seed_snap || dx > S.seed_snap || dy < -S.seed_snap || dy > S.seed_snap) return KEY_NONE;
    const uint32_t d2 = d2_of(dx, dy);
    if (d2 > (uint32_t)(S.seed_snap * S.seed_snap)) return KEY_NONE;
    return key_of(d2, cy * nx + cx);
}

}      // namespace ssm_clrc
