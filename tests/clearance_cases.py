"""Named class images for the clearance map's tests, shared by the CPU tests (the host function against the restatement) and the GPU tests (the
device against the host function).  A case is a dictionary: cls (ny x nx uint8 of grid classes: 0 unobserved, 1 drivable, 2 walkable, 3 other ground, 4 obstacle),
params (keywords of ssm.clearance_params) and, where the outcome is known by construction, `want`: facts the tests assert on what the library gives."""
import numpy as np

U, D, W, G, O = 0, 1, 2, 3, 4


def grid(nx, ny, fill=D):
    return np.full((ny, nx), fill, np.uint8)


def idx(cx, cy, nx):
    return cy * nx + cx


def empty_grid():
    return dict(cls=grid(7, 5, U), params=dict(seed=(3, 2)), want=dict(info=dict(blocked=0, free_cells=0, traversable=0, components=0, reachable=0, seed_cell=-1, max_d2_reachable=0)))


def nothing_blocked():
    """every cell is as far as can be from nothing: UINT32_MAX, which counts as itself in max_d2_reachable"""
    return dict(cls=grid(9, 6), params=dict(seed=(4, 3), radius=3.0),
                want=dict(info=dict(blocked=0, free_cells=54, traversable=54, components=1, reachable=54, seed_cell=idx(4, 3, 9), max_d2_reachable=0xFFFFFFFF), d2_all=0xFFFFFFFF, nearest_all=-1))


def everything_blocked():
    return dict(cls=grid(6, 9, O), params=dict(seed=(2, 2)), want=dict(info=dict(blocked=54, free_cells=0, traversable=0, components=0, reachable=0, seed_cell=-1), d2_all=0))


def one_blocked(where):
    nx, ny = 9, 7
    cx, cy = dict(sw=(0, 0), se=(nx - 1, 0), nw=(0, ny - 1), ne=(nx - 1, ny - 1), middle=(nx // 2, ny // 2))[where]
    c = grid(nx, ny); c[cy, cx] = O
    ys, xs = np.mgrid[0:ny, 0:nx]
    return dict(cls=c, params=dict(radius=0.0), want=dict(d2=((xs - cx) ** 2 + (ys - cy) ** 2).astype(np.uint32), nearest_all=idx(cx, cy, nx)))


def mirrored(how):
    """two blocked cells mirrored about the cell (4, 3): the one with the lower index is the nearest"""
    nx, ny = 9, 7
    a, b = dict(horizontal=((2, 3), (6, 3)), vertical=((4, 1), (4, 5)), diagonal=((2, 1), (6, 5)), antidiagonal=((6, 1), (2, 5)))[how]
    c = grid(nx, ny); c[a[1], a[0]] = O; c[b[1], b[0]] = O
    return dict(cls=c, params=dict(radius=0.0), want=dict(at=[((4, 3), (4 - a[0]) ** 2 + (3 - a[1]) ** 2, idx(a[0], a[1], nx))]))


def ring_centre():
    """four blocked cells at distance 3 from (5, 5), each in another column and row: the lowest index wins"""
    nx, ny = 11, 11
    c = grid(nx, ny)
    for x, y in ((5, 2), (2, 5), (8, 5), (5, 8)):
        c[y, x] = O
    return dict(cls=c, params=dict(radius=0.0), want=dict(at=[((5, 5), 9, idx(5, 2, nx))]))


def ring():
    """every cell at squared distance 25 from (6, 6) is blocked (the twelve lattice points of that circle)"""
    nx, ny = 13, 13
    c = grid(nx, ny)
    ys, xs = np.mgrid[0:ny, 0:nx]
    c[(xs - 6) ** 2 + (ys - 6) ** 2 == 25] = O
    return dict(cls=c, params=dict(radius=0.0), want=dict(at=[((6, 6), 25, idx(6, 1, nx))]))


def row_blocked_at_both_ends():
    nx = 9
    c = grid(nx, 1); c[0, 0] = O; c[0, nx - 1] = O
    return dict(cls=c, params=dict(radius=0.0), want=dict(at=[((4, 0), 16, 0), ((5, 0), 9, 8), ((3, 0), 9, 0)]))


def corridor(radius, **kw):
    """A corridor 15 cells wide and 21 long, walls in the columns 0 and 14, one pillar at (7, 10); cell = 1 m.  A cell clears the walls when its column is at least
    r + 1 cells from both (d2 > r^2 with integer distances), and the pillar when (cx - 7)^2 + (cy - 10)^2 > r^2.  radius 2: the columns 3 .. 11 clear the walls, and in
    the pillar's row the columns 3, 4, 10 and 11 clear the pillar -- the lane is open on both sides.  radius 3: the columns 4 .. 10 clear the walls, the pillar's row
    needs |cx - 7| >= 4: no cell of row 10 is traversable and the lane is cut in two."""
    nx, ny = 15, 21
    c = grid(nx, ny); c[:, 0] = O; c[:, nx - 1] = O; c[10, 7] = O
    return dict(cls=c, params=dict(dict(radius=radius, seed=(7, 2)), **kw))


def corridor_open():
    return dict(corridor(2.0), want=dict(info=dict(components=1, r2=4), reach_at=[((7, 18), 2), ((3, 10), 2), ((11, 10), 2), ((5, 10), 0), ((2, 5), 0)]))


def corridor_closed():
    return dict(corridor(3.0), want=dict(info=dict(components=2, r2=9), reach_at=[((7, 18), 1), ((7, 2), 2), ((4, 10), 0), ((10, 10), 0), ((4, 9), 2), ((4, 11), 1)]))


def diagonal_gap():
    """two rooms that touch only across the diagonal (4, 3) -- (3, 4): one component under 8, two under 4"""
    c = grid(8, 8); c[3, 0:4] = O; c[4, 4:8] = O
    return dict(cls=c, params=dict(radius=0.0, seed=(1, 1)))


def seed_snaps():
    """the seed on the pillar: the traversable cells nearest to it are the eight knight's moves away, d2 = 5 > r2 = 4 -- of them (6, 8) has the lowest index"""
    return dict(corridor(2.0, seed=(7, 10)), want=dict(info=dict(seed_cell=idx(6, 8, 15), components=1)))


def seed_finds_nothing():
    """within 2 cells of the pillar nothing is farther than 2 cells from it: no seed, nothing reachable, every traversable cell 1"""
    return dict(corridor(2.0, seed=(7, 10), seed_snap=2), want=dict(info=dict(seed_cell=-1, reachable=0, max_d2_reachable=0)))


def snap_tie():
    """the seed in a wall of unobserved cells, one free cell to its left and one to its right: the left one has the lower index"""
    c = grid(9, 5); c[:, 4] = U
    return dict(cls=c, params=dict(radius=0.0, seed=(4, 2), seed_snap=1), want=dict(info=dict(seed_cell=idx(3, 2, 9), components=2, reachable=20)))


def checkerboard(nx=33, ny=31):
    ys, xs = np.mgrid[0:ny, 0:nx]
    c = grid(nx, ny); c[(xs + ys) % 2 == 0] = O
    return dict(cls=c, params=dict(radius=0.0, seed=(1, 0), connectivity=8))


def random_fill(nx, ny, fraction, seed, **kw):
    """blocked cells at the given fraction; the others mostly drivable, some of every other class"""
    rng = np.random.default_rng(seed)
    c = rng.choice(np.array([D, D, D, D, D, D, W, G, U], np.uint8), size=(ny, nx))
    c[rng.random((ny, nx)) < fraction] = O
    return dict(cls=c, params=dict(dict(radius=1.5, seed=(nx // 2, ny // 2), seed_snap=10), **kw))


def other_masks():
    """walkable cells count as free, unobserved ones as blocked"""
    cs = random_fill(40, 37, 0.05, 11)
    cs["params"].update(blocked=[O, U], free=[D, W], radius=1.0)
    return cs


def cases():
    out = dict(empty_grid=empty_grid, nothing_blocked=nothing_blocked, everything_blocked=everything_blocked, ring_centre=ring_centre, ring=ring,
               row_blocked_at_both_ends=row_blocked_at_both_ends, corridor_open=corridor_open, corridor_closed=corridor_closed, diagonal_gap=diagonal_gap, seed_snaps=seed_snaps,
               seed_finds_nothing=seed_finds_nothing, snap_tie=snap_tie, checkerboard=checkerboard, other_masks=other_masks)
    for w in ("sw", "se", "nw", "ne", "middle"):
        out["one_blocked_" + w] = lambda w=w: one_blocked(w)
    for h in ("horizontal", "vertical", "diagonal", "antidiagonal"):
        out["mirrored_" + h] = lambda h=h: mirrored(h)
    for name, f in (("0.1", 0.001), ("5", 0.05), ("50", 0.5)):
        out["random_%s_percent" % name] = lambda f=f: random_fill(65, 65, f, int(f * 1000) + 3)
        out["random_%s_percent_conn8" % name] = lambda f=f: random_fill(63, 65, f, int(f * 1000) + 4, connectivity=8, radius=2.5)
    return out


SHAPES = ((1, 1), (1, 2), (2, 1), (31, 33), (32, 32), (33, 31), (63, 65), (64, 64), (65, 63), (1, 257), (257, 1), (300, 7))
