// route_core.h -- the arithmetic of the route field: over the REACHABLE cells of a clearance map (clearance_core.h: reach == 2) every cell gets the
// cost of the cheapest path from the clearance call's seed cell, the SOURCE, and the neighbour that path arrives through; a goal is then answered by following
// those parents.  Compiled for host and device like clearance_core.h: csrc/kernels_route.hip and the host functions of csrc/ssm_route_host.cpp call the same
// functions, so device == host bit for bit.  Every figure the kernels see is an integer and both outputs are minima: nothing depends on the order of cells, moves
// or rounds.  The reference has no such step.
//
// Why a cost never overflows: a path that attains a minimum is simple, so it has at most 2^24 - 1 edges (grid_core.h MAX_CELLS cells); an edge costs at most
// STEP_DIAG (1 + MAX_NEAR_WEIGHT) 2 = 7 . 9 . 2 = 126; the product is 2 113 929 090 < 2^31.  So a cost fits 31 bits, cost + edge fits 32, and a parent's key
// ((cost + edge) << 24) | index fits 56.
#pragma once
#include "clearance_core.h"

namespace ssm_rtc {

static const uint32_t COST_NONE = UINT32_MAX;                   // the cost of a cell no path reaches
static const int32_t STEP_AXIAL = 5, STEP_DIAG = 7;             // 7 / 5 = 1.4: the chamfer pair nearest sqrt(2) in one digit
static const int32_t MAX_NEAR_WEIGHT = 8;
static const uint32_t MAX_EDGE = (uint32_t)STEP_DIAG * 2u * (1u + (uint32_t)MAX_NEAR_WEIGHT);      // 126
static const int32_t INDEX_MASK = (1 << 24) - 1;
static_assert((uint64_t)MAX_EDGE * (uint64_t)INDEX_MASK < ((uint64_t)1 << 31), "the longest simple path at the dearest edge stays below 2^31");
// what a cell's byte in the kernels holds: bit 0 the cell takes part (reach == 2), bit 1 it is NEAR (dist2 <= comfort2)
enum { CELL_IN = 1, CELL_NEAR = 2 };

// what a call's parameters become once
struct Setup { int32_t moves, near_weight; int64_t comfort2; };

// host only: comfort2 = floor((comfort / cell)^2), saturated like the clearance map's r2
inline int64_t comfort2_of(double comfort, double cell) { return ssm_clrc::r2_of(comfort, cell); }

CARVE_HD bool near_of(uint32_t dist2, int64_t comfort2) { return (int64_t)dist2 <= comfort2; }
CARVE_HD uint8_t cell_byte(uint8_t reach, uint32_t dist2, int64_t comfort2)
{ return reach == ssm_clrc::REACHABLE ? (uint8_t)(CELL_IN | (near_of(dist2, comfort2) ? CELL_NEAR : 0)) : (uint8_t)0; }
// the weight of a cell that takes part
CARVE_HD uint32_t weight_of(uint8_t byte, int32_t near_weight) { return 1u + ((byte & CELL_NEAR) ? (uint32_t)near_weight : 0u); }
// the cost of the move between two adjacent cells of weights wa and wb: symmetric, 10 .. 126
CARVE_HD uint32_t edge_of(int32_t step, uint32_t wa, uint32_t wb) { return (uint32_t)step * (wa + wb); }
// what a parent is the minimum of: the cost of arriving through p above the 24 bits of p's index
CARVE_HD unsigned long long parent_key(uint32_t cost_through, int32_t index) { return ((unsigned long long)cost_through << 24) | (unsigned long long)(uint32_t)index; }
// what far_cell is the MAXIMUM of: the cost above the index counted from the top, so that the lowest index wins among equal costs
CARVE_HD unsigned long long far_key(uint32_t cost, int32_t index) { return ((unsigned long long)cost << 24) | (unsigned long long)(uint32_t)(INDEX_MASK - index); }
CARVE_HD int32_t far_cell_of(unsigned long long key) { return INDEX_MASK - (int32_t)(key & (unsigned long long)INDEX_MASK); }
// the eight moves, the axial ones first: moves == 4 takes the first four
CARVE_HD int32_t move_dx(int m) { return m == 0 ? -1 : m == 1 ? 1 : m < 4 ? 0 : (m & 1) ? 1 : -1; }
CARVE_HD int32_t move_dy(int m) { return m < 2 ? 0 : m == 2 ? -1 : m == 3 ? 1 : m < 6 ? -1 : 1; }
// a step of a path between the adjacent cells a and b of a grid nx wide: is it diagonal?  (a difference of nx is a step along a column, also when nx == 1; a
// difference of 1 is a step along a row only inside one row: with nx == 2 the cells (1, y) and (0, y + 1) differ by 1 as well)
CARVE_HD bool step_is_diag(int32_t a, int32_t b, int32_t nx) { const int32_t d = a < b ? b - a : a - b; return d != nx && !(d == 1 && a / nx == b / nx); }
// the goal's snap as a clearance seed (clearance_core.h seed_key is the rule): the fields seed_key reads
CARVE_HD ssm_clrc::Setup goal_setup(int32_t goal_cx, int32_t goal_cy, int32_t goal_snap)
{
    ssm_clrc::Setup G;
    G.blocked_mask = 0; G.free_mask = 0; G.r2 = 0; G.connectivity = 8; G.seed_cx = goal_cx; G.seed_cy = goal_cy; G.seed_snap = goal_snap;
    return G;
}

}      // namespace ssm_rtc
