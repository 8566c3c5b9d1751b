"""Named inputs for the route field's tests, shared by the CPU tests (the host functions against the restatement) and the GPU tests (the device
against the host functions).  A case is a dictionary: reach (ny x nx uint8 as the clearance map gives it: 2 takes part), dist2 (ny x nx uint32), source ((cx, cy) or
None), params (keywords of ssm.route_params), goals (a list of dict(goal=(cx, cy), snap=s) with, where known, want=dict(path info fields)) and, where the outcome
is known by construction, `want`: facts the tests assert on what the library gives.  dist2 is data to this stage: a case may plant any value."""
import numpy as np

NONE = 0xFFFFFFFF          # COST_NONE, and the clearance map's dist2 where nothing is blocked
FAR = 10000                # a planted dist2 above every comfort2 the cases use but the saturated one


def field(nx, ny, reach=2, dist2=FAR):
    return np.full((ny, nx), reach, np.uint8), np.full((ny, nx), dist2, np.uint32)


def idx(cx, cy, nx):
    return cy * nx + cx


def case(reach, dist2, source, params=None, goals=(), want=None):
    return dict(reach=reach, dist2=dist2, source=source, params=dict(params or {}), goals=list(goals), want=want or {})


def no_seed():
    r, d = field(7, 5); r[0, :3] = 1
    return case(r, d, None, want=dict(info=dict(routed=0, unrouted=32, near_cells=0, max_cost=0, far_cell=-1, source_cell=-1), cost_all=NONE, parent_all=-1),
                goals=[dict(goal=(3, 2), snap=1024, want=dict(len=0, goal_cell=-1, cost=-1, min_d2=-1))])


def tiny(nx, ny):
    r, d = field(nx, ny)
    n = nx * ny
    return case(r, d, (0, 0), want=dict(info=dict(routed=n, unrouted=0, max_cost=10 * (n - 1), far_cell=n - 1, source_cell=0), cost=np.arange(n, dtype=np.uint32).reshape(ny, nx) * 10),
                goals=[dict(goal=(nx - 1, ny - 1), snap=0, want=dict(len=n, goal_cell=n - 1, cost=10 * (n - 1), n_axial=n - 1, n_diag=0))])


def source_alone():
    """the source's eight neighbours take no part; the cells beyond them do, and no path leads there"""
    r, d = field(7, 7); r[2:5, 2:5] = 1; r[3, 3] = 2
    return case(r, d, (3, 3), want=dict(info=dict(routed=1, unrouted=40, max_cost=0, far_cell=idx(3, 3, 7)), parent_all=-1),
                goals=[dict(goal=(3, 3), snap=0, want=dict(len=1, cost=0, n_axial=0, n_diag=0)), dict(goal=(0, 0), snap=2, want=dict(len=0))])


def open_field(moves):
    """nothing in the way and nothing near: a chamfer distance from the source"""
    nx, ny, sx, sy = 21, 17, 10, 8
    r, d = field(nx, ny)
    ys, xs = np.mgrid[0:ny, 0:nx]
    dx, dy = abs(xs - sx), abs(ys - sy)
    cost = 10 * np.maximum(dx, dy) + 4 * np.minimum(dx, dy) if moves == 8 else 10 * (dx + dy)
    return case(r, d, (sx, sy), dict(moves=moves), want=dict(cost=cost.astype(np.uint32), info=dict(routed=nx * ny, unrouted=0, near_cells=0, far_cell=0, moves=moves)),
                goals=[dict(goal=(0, 0), snap=0, want=dict(cost=int(cost[0, 0]), len=11 if moves == 8 else 19, n_diag=8 if moves == 8 else 0))])


def corridor(near_weight):
    """3 x 21, the middle row NEAR in the columns 5 .. 15: with a raised weight the cheapest way leaves the middle row by a diagonal, runs along an outer row and comes
    back -- 40 + 14 + 100 + 14 + 40 = 208 against 310 straight through -- and of the two mirror-image ways the parents choose row 0, the lower indices"""
    r, d = field(21, 3); d[1, 5:16] = 1
    cost = 200 if near_weight == 0 else 208
    return case(r, d, (0, 1), dict(near_weight=near_weight, comfort=2.0), want=dict(info=dict(comfort2=4), cost_at=[((20, 1), cost)], corridor=near_weight > 0),
                goals=[dict(goal=(20, 1), snap=0, want=dict(cost=cost, goal_cell=idx(20, 1, 21), min_d2=FAR if near_weight else 1, near_steps=0 if near_weight else 11))])


def pillar():
    """a pillar between the source (2, 1) and the cell (2, 3): a way of 40 round either side (no diagonal passes the pillar's corners), and the parent of the meeting
    cell is (1, 3), the lower index"""
    r, d = field(5, 5); r[2, 2] = 0
    return case(r, d, (2, 1), want=dict(cost_at=[((2, 3), 40), ((1, 3), 30), ((3, 3), 30)], parent_at=[((2, 3), idx(1, 3, 5))]))


def diagonal_gap():
    """two rooms that touch only across the diagonal (4, 3) -- (3, 4), clearance_cases.diagonal_gap: one component under 8-connectivity, but the move would cut
    two corners, so the far room is not routed"""
    r, d = field(8, 8); r[3, 0:4] = 0; r[4, 4:8] = 0
    return case(r, d, (1, 1), want=dict(info=dict(unrouted=int((r[4:] == 2).sum()), routed=int((r[:4] == 2).sum())), cost_at=[((3, 4), NONE), ((4, 2), 10 * 3 + 4 * 1)]))


def tile_corner_gap():
    """64 x 64: walls in column 32 and, left of it, row 32, open only where they would meet -- the four cells round the corner that four 32 x 32 tiles share.  Every
    way out of the source's tile passes there, the cheapest to (32, 32) by the diagonal from (31, 31)"""
    r, d = field(64, 64)
    r[:31, 32] = 0; r[33:, 32] = 0; r[32, :31] = 0
    return case(r, d, (5, 5), want=dict(info=dict(unrouted=0, routed=int((r == 2).sum())), cost_at=[((31, 31), 14 * 26), ((32, 32), 14 * 27), ((32, 31), 14 * 26 + 10), ((31, 32), 14 * 26 + 10)],
                                         parent_at=[((32, 32), idx(31, 31, 64))]))


def source_on_rim():
    """64 x 64: the source (32, 31) sits in a corner of its 32 x 32 tile and its two neighbours inside that tile take no part -- every way out begins in another
    tile, so a tile-local relaxation of the source's tile alone changes nothing"""
    r, d = field(64, 64); r[31, 33] = 0; r[30, 32] = 0; r[30, 33] = 0
    return case(r, d, (32, 31), want=dict(info=dict(unrouted=0, routed=64 * 64 - 3), cost_at=[((31, 31), 10), ((32, 32), 10), ((31, 30), 20), ((34, 31), 40)]))


def serpentine(n=65):
    """every other row is a wall with one gap, at alternating ends: one way of (n - 1) / 2 + 1 rows of n - 1 steps and two steps per turn, all axial (a diagonal
    round a wall's end would cut its corner)"""
    r, d = field(n, n)
    for y in range(1, n, 2):
        r[y, :] = 0
        r[y, n - 1 if y % 4 == 1 else 0] = 2
    rows = (n + 1) // 2
    steps = rows * (n - 1) + (rows - 1) * 2
    last_x = n - 1 if ((n - 1) // 2) % 2 == 0 else 0
    return case(r, d, (0, 0), want=dict(info=dict(unrouted=0, routed=steps + 1, max_cost=10 * steps, far_cell=idx(last_x, n - 1, n))),
                goals=[dict(goal=(last_x, n - 1), snap=0, want=dict(len=steps + 1, cost=10 * steps, n_diag=0))])


def spiral(n=65):
    """a corridor one cell wide wound inwards from (0, 0), one cell of wall between its turns: one way, all axial"""
    open_ = np.zeros((n, n), bool)
    x, y, dx, dy = 0, 0, 1, 0
    open_[0, 0] = True
    order = [(0, 0)]
    inside = lambda a, b: 0 <= a < n and 0 <= b < n  # noqa: E731
    while True:
        for _ in range(2):
            ax, ay, bx, by = x + dx, y + dy, x + 2 * dx, y + 2 * dy
            if inside(ax, ay) and not open_[ay, ax] and (not inside(bx, by) or not open_[by, bx]):
                break
            dx, dy = -dy, dx
        else:
            break
        x, y = ax, ay
        open_[y, x] = True
        order.append((x, y))
    r, d = field(n, n, 0); r[open_] = 2
    steps = len(order) - 1
    return case(r, d, (0, 0), want=dict(info=dict(unrouted=0, routed=steps + 1, max_cost=10 * steps, far_cell=idx(x, y, n))),
                goals=[dict(goal=(x, y), snap=0, want=dict(len=steps + 1, cost=10 * steps, n_diag=0))])


def comb():
    """a spine along row 0 and a tooth down every other column: dead ends, every one routed"""
    nx, ny = 33, 20
    r, d = field(nx, ny, 0); r[0, :] = 2; r[:, ::2] = 2
    d[:] = 1          # everything NEAR: every weight is raised alike
    return case(r, d, (0, 0), dict(near_weight=3, comfort=1.0), want=dict(info=dict(unrouted=0, near_cells=int((r == 2).sum()), far_cell=idx(32, 19, nx), max_cost=40 * (32 + 19)),
                                                                            cost_at=[((32, 19), 5 * 8 * (32 + 19))]))


def u_trap():
    """the source inside a U that opens away from the goal: the way leads out of the mouth and round"""
    r, d = field(21, 21)
    r[5:16, 15] = 0; r[5, 5:16] = 0; r[15, 5:16] = 0          # the U's bottom (column 15) and arms (rows 5 and 15), its mouth towards column 0
    return case(r, d, (12, 10), goals=[dict(goal=(18, 10), snap=0)], want=dict(info=dict(unrouted=0), cost_at=[((14, 10), 20)]))


def random_fill(nx, ny, fraction, seed, **params):
    """cells that take no part at the given fraction (reach 0 or 1), planted dist2 of 0 .. 12 and now and then "nothing blocked"; the source: the cell that takes part
    nearest the middle, the lowest index among equals"""
    rng = np.random.default_rng(seed)
    r = np.full((ny, nx), 2, np.uint8)
    out = rng.random((ny, nx)) < fraction
    r[out] = rng.integers(0, 2, (ny, nx), dtype=np.uint8)[out]
    d = rng.integers(0, 13, (ny, nx)).astype(np.uint32)
    d[rng.random((ny, nx)) < 0.02] = NONE
    ys, xs = np.mgrid[0:ny, 0:nx]
    key = ((((xs - nx // 2) ** 2 + (ys - ny // 2) ** 2).astype(np.int64) << 24) | (ys * nx + xs))[r == 2]
    source = None if key.size == 0 else (int(key.min() & 0xFFFFFF) % nx, int(key.min() & 0xFFFFFF) // nx)
    return case(r, d, source, params, goals=[dict(goal=(0, 0), snap=1024), dict(goal=(nx - 1, ny - 1), snap=3), dict(goal=(nx // 2, ny // 2), snap=0)])


def weights(near_weight):
    return random_fill(40, 37, 0.2, 31, near_weight=near_weight, comfort=2.5)


def comfort_zero():
    """comfort2 == 0: only a planted dist2 of 0 is NEAR"""
    cs = random_fill(33, 31, 0.1, 32, comfort=0.0, near_weight=8)
    cs["want"] = dict(info=dict(comfort2=0))
    return cs


def comfort_saturated():
    """comfort2 == 2^31: every dist2 but "nothing blocked" is NEAR"""
    cs = random_fill(33, 31, 0.1, 33, comfort=1e9, cell=0.5, near_weight=5)
    cs["want"] = dict(info=dict(comfort2=1 << 31))
    return cs


def goal_snaps():
    """column 4 takes no part but in row 0.  The goal (4, 2) has the routed cells (3, 2) and (5, 2) one cell away: the lower index wins; with a snap of 0 it finds
    nothing; a goal that is routed snaps onto itself whatever the snap distance"""
    r, d = field(9, 5); r[1:, 4] = 0
    return case(r, d, (0, 0), goals=[dict(goal=(4, 2), snap=1, want=dict(goal_cell=idx(3, 2, 9))), dict(goal=(4, 2), snap=0, want=dict(len=0, goal_cell=-1)),
                                     dict(goal=(6, 3), snap=0, want=dict(goal_cell=idx(6, 3, 9))), dict(goal=(6, 3), snap=1024, want=dict(goal_cell=idx(6, 3, 9))),
                                     dict(goal=(4, 4), snap=1, want=dict(goal_cell=idx(3, 4, 9))), dict(goal=(4, 3), snap=2, want=dict(goal_cell=idx(3, 3, 9)))])


def row_of_ten():
    """1 x 10 cells: the path to the far end has exactly 10 cells -- a max_path of 10 holds it, one of 9 does not"""
    r, d = field(10, 1)
    return case(r, d, (0, 0), goals=[dict(goal=(9, 0), snap=0, want=dict(len=10, cost=90, n_axial=9))])


def cases():
    out = dict(no_seed=no_seed, source_alone=source_alone, pillar=pillar, diagonal_gap=diagonal_gap, tile_corner_gap=tile_corner_gap, source_on_rim=source_on_rim, serpentine=serpentine, spiral=spiral, comb=comb,
               u_trap=u_trap, comfort_zero=comfort_zero, comfort_saturated=comfort_saturated, goal_snaps=goal_snaps, row_of_ten=row_of_ten)
    for nx, ny in ((1, 1), (1, 2), (2, 1)):
        out["tiny_%dx%d" % (nx, ny)] = lambda nx=nx, ny=ny: tiny(nx, ny)
    for m in (4, 8):
        out["open_field_%d" % m] = lambda m=m: open_field(m)
    for w in (0, 1, 8):
        out["corridor_weight_%d" % w] = lambda w=w: corridor(w)
    for w in (0, 8):
        out["near_weight_%d" % w] = lambda w=w: weights(w)
    for name, f in (("5", 0.05), ("30", 0.3), ("60", 0.6)):
        out["random_%s_percent" % name] = lambda f=f: random_fill(65, 65, f, int(f * 100) + 3)
    return out


FILLS = (0.0, 0.1, 0.4)
# beside the clearance tests' shapes: two cells wide or high, where the cells (1, y) and (0, y + 1) are diagonal neighbours with adjacent indices
EXTRA_SHAPES = ((2, 2), (2, 9), (9, 2))
