"""The case lists of object extraction's tests, shared by tests/test_objects.py (host functions against the restatement tests/objects_ref.py) and
tests/test_gpu_objects.py (device against host functions).  A CELL CASE is dict(cls, obstacle_label, ground_q, top_q, n_high: ny x nx arrays, params); a pattern
of members is a ny x nx array of labels (255: no member), from which cell_case() makes the arrays with seeded heights and counts so that every figure differs from
cell to cell.  A CLOUD CASE is dict(clouds, T_clouds, grid, params): a ground sheet with boxes standing on it, built from grid coordinates (grid_cases.gp)."""
import numpy as np
import grid_cases as GC

OBSTACLE = 4
LOOSE = dict(min_cells=1, min_points=0, min_height=0.0)          # every component is kept: the labelling alone


def cell_case(labels, params=None, seed=0, ground_q=None, top_q=None, n_high=None):
    labels = np.ascontiguousarray(labels, np.uint8)
    rng = np.random.default_rng(seed + labels.size)
    cls = np.where(labels != 255, OBSTACLE, rng.integers(0, 4, labels.shape)).astype(np.uint8)
    gq = rng.integers(-2000, 200, labels.shape).astype(np.int32) if ground_q is None else np.ascontiguousarray(ground_q, np.int32)
    tq = (gq + rng.integers(0, 3000, labels.shape)).astype(np.int32) if top_q is None else np.ascontiguousarray(top_q, np.int32)
    nh = rng.integers(0, 60, labels.shape).astype(np.uint32) if n_high is None else np.ascontiguousarray(n_high, np.uint32)
    return dict(cls=cls, obstacle_label=labels, ground_q=gq, top_q=tq, n_high=nh, params=dict(LOOSE if params is None else params))


def empty(nx, ny, tw, th):
    return np.full((ny, nx), 255, np.uint8)


def full(nx, ny, tw, th):
    return np.full((ny, nx), 9, np.uint8)


def checkerboard(nx, ny, tw, th):
    y, x = np.mgrid[0:ny, 0:nx]
    return np.where((x + y) % 2 == 0, 10, 255).astype(np.uint8)


def column_stripes(nx, ny, tw, th):
    y, x = np.mgrid[0:ny, 0:nx]
    return (9 + x % 2).astype(np.uint8)


def row_stripes(nx, ny, tw, th):
    y, x = np.mgrid[0:ny, 0:nx]
    return (10 + y % 2).astype(np.uint8)


def serpentine(nx, ny, tw, th):
    """one cell wide: every other row full, joined at alternating ends"""
    L = np.full((ny, nx), 255, np.uint8)
    L[0::2, :] = 11
    for k, y in enumerate(range(1, ny, 2)):
        if y + 1 < ny:
            L[y, nx - 1 if k % 2 == 0 else 0] = 11
    return L


def spiral(nx, ny, tw, th):
    """one cell wide, inwards, a free cell between the turns: walk ahead while the next cell is free and the one behind it too, else turn right"""
    L = np.full((ny, nx), 255, np.uint8)
    inside = lambda x, y: 0 <= x < nx and 0 <= y < ny  # noqa: E731
    x = y = d = turns = 0
    L[0, 0] = 9
    while turns < 2:
        dx, dy = ((1, 0), (0, 1), (-1, 0), (0, -1))[d]
        if inside(x + dx, y + dy) and L[y + dy, x + dx] == 255 and not (inside(x + 2 * dx, y + 2 * dy) and L[y + 2 * dy, x + 2 * dx] != 255):
            x += dx; y += dy; L[y, x] = 9; turns = 0
        else:
            d = (d + 1) % 4; turns += 1
    return L


def u_shape(nx, ny, tw, th):
    """two arms down the first and last columns that meet only in the last row: the root (cell 0) has to reach the far arm back through earlier tiles"""
    L = np.full((ny, nx), 255, np.uint8)
    L[:, 0] = 10; L[:, nx - 1] = 10; L[ny - 1, :] = 10
    return L


def rings(nx, ny, tw, th):
    y, x = np.mgrid[0:ny, 0:nx]
    d = np.minimum(np.minimum(x, nx - 1 - x), np.minimum(y, ny - 1 - y))
    return (9 + d % 2).astype(np.uint8)


def tile_corner(nx, ny, tw, th):
    """two members that touch only diagonally, across the corner where four tiles meet (or as near to it as the grid reaches); and the other diagonal"""
    L = np.full((ny, nx), 255, np.uint8)
    x, y = min(tw, nx - 1), min(th, ny - 1)
    if x >= 1 and y >= 1:
        L[y - 1, x - 1] = 9; L[y, x] = 9
        if x + 2 < nx and y >= 1:
            L[y, x + 1] = 11; L[y - 1, x + 2] = 11
    return L


def random_fill(density, seed):
    def make(nx, ny, tw, th):
        rng = np.random.default_rng(seed * 1000 + nx * 7 + ny)
        return np.where(rng.random((ny, nx)) < density, rng.integers(9, 12, (ny, nx)), 255).astype(np.uint8)
    return make


def patterns():
    p = dict(empty=empty, full=full, checkerboard=checkerboard, column_stripes=column_stripes, row_stripes=row_stripes, serpentine=serpentine, spiral=spiral, u_shape=u_shape,
             rings=rings, tile_corner=tile_corner)
    for d in (0.3, 0.6):
        for s in (1, 2, 3):
            p[f"random_{int(d * 10)}_{s}"] = random_fill(d, s)
    return p


def shapes(tw, th):
    """1 x 1, 1 x 200, 200 x 1, every combination of tile - 1, tile, tile + 1 per axis, and 2 tiles + 2 by 2 tiles + 3"""
    return [(1, 1), (1, 200), (200, 1)] + [(tw + a, th + b) for a in (-1, 0, 1) for b in (-1, 0, 1)] + [(2 * tw + 2, 2 * th + 3)]


# ---- small cell cases with known outcomes (5 wide, 4 high unless said)
def _blank(nx=5, ny=4):
    return np.full((ny, nx), 255, np.uint8)


def diagonal_contact():
    L = _blank(); L[1, 1] = 9; L[2, 2] = 9
    return cell_case(L)


def different_labels():
    L = _blank(); L[1, 1:3] = 9; L[1, 3] = 10; L[2, 1] = 9; L[2, 2] = 10          # the 10s touch diagonally, and each touches a 9 along an edge
    return cell_case(L)


def label_outside_mask():
    L = _blank(); L[0, :] = 4; L[1, :] = 8; L[2, 0:2] = 9; L[3, :] = 12
    c = cell_case(L)
    c["cls"][:] = OBSTACLE
    return c


def not_an_obstacle():
    L = _blank(); L[1, 1:4] = 9
    c = cell_case(L)
    c["cls"][1, 2] = 1          # the label is there, the class is not: the cell is no member and cuts the row in two
    return c


def rejections():
    """four components of label 9 in a 9 x 7 grid under min_cells 2, min_points 20, min_height 0.5 (512 units): A kept; B fails the cells alone; C the points
    alone; D the height alone; E fails all three and counts as cells; F fails points and height and counts as points"""
    L = _blank(9, 7)
    gq = np.zeros((7, 9), np.int32); tq = np.full((7, 9), 512, np.int32); nh = np.full((7, 9), 10, np.uint32)
    L[0, 0:2] = 9                                            # A: 2 cells, 20 points, 512
    L[0, 4] = 9; nh[0, 4] = 20                               # B: 1 cell
    L[2, 0:2] = 9; nh[2, 0] = 9                              # C: 19 points
    L[2, 4:6] = 9; tq[2, 4:6] = 511                          # D: 511
    L[4, 0] = 9; nh[4, 0] = 1; tq[4, 0] = 3                  # E
    L[4, 4:6] = 9; nh[4, 4:6] = 2; tq[4, 4:6] = 100          # F
    L[6, 0:3] = 9; gq[6, 0] = -5; tq[6, 2] = 507; tq[6, 0:2] = 100          # G: kept through the min and max of different cells (507 - -5 = 512)
    return cell_case(L, dict(min_cells=2, min_points=20, min_height=0.5), ground_q=gq, top_q=tq, n_high=nh)


def ids_ascend():
    L = _blank(6, 6); L[0, 5] = 11; L[1, 0:2] = 9; L[3, 3] = 10; L[5, 0] = 9; L[5, 5] = 10
    return cell_case(L)


def cell_cases():
    return dict(diagonal_contact=diagonal_contact, different_labels=different_labels, label_outside_mask=label_outside_mask, not_an_obstacle=not_an_obstacle,
                rejections=rejections, ids_ascend=ids_ascend)


# ---- cloud cases
GRID = dict(x0=-3.0, y0=0.0, cell=0.25, nx=24, ny=20, h_min=-3.0, h_max=3.0, step=0.25, ground_radius=1, min_obstacle_points=3)


def box(rng, x0, x1, y0, y1, z0, z1, n, label, other=0.0):
    """n points inside a box of the grid frame; a fraction `other` of them carries another label"""
    lab = np.where(rng.random(n) < other, rng.integers(0, 14, n), label)
    return GC.gp(rng.uniform(x0, x1, n), rng.uniform(y0, y1, n), rng.uniform(z0, z1, n), lab)


def street(seed, m=3, n_ground=4000, poses=False):
    """a ground sheet at height -1.5 m (Road, Pavement at the sides), a car, a pedestrian, a bike lying flat (too low to be kept), a fence (not in the mask) and a
    second car touching the first only diagonally -- spread over m clouds in random order"""
    rng = np.random.default_rng(seed)
    gx = rng.uniform(-3.2, 3.2, n_ground); gy = rng.uniform(-0.2, 5.2, n_ground)
    parts = [GC.gp(gx, gy, rng.normal(-1.5, 0.01, n_ground), np.where(np.abs(gx) < 2.0, 4, 5)),
             box(rng, -1.95, -0.8, 1.05, 1.95, -1.2, 0.0, 1500, 9, 0.1),           # a car: cells x 4 .. 8, y 4 .. 7
             box(rng, -0.7, -0.55, 2.05, 2.2, -1.2, -0.5, 300, 9),                # a second car in cell (9, 8): it touches the first only diagonally
             box(rng, 1.05, 1.2, 3.05, 3.2, -1.2, 0.2, 200, 10),                  # a pedestrian in one cell
             box(rng, 1.55, 2.2, 0.55, 0.7, -1.24, -1.225, 120, 11),              # a bike lying flat: HIGH (above base + step), but below the default min_height
             box(rng, -2.9, -2.6, 0.1, 4.9, -1.2, -0.3, 900, 8)]                  # a fence: label 8 is not in the default mask
    pts = np.concatenate(parts)
    pts = pts[rng.permutation(len(pts))]
    cuts = np.sort(rng.integers(0, len(pts) + 1, m - 1)) if m > 1 else []
    clouds = [c.copy() for c in np.split(pts, cuts)]
    T = [GC.EYE] * m
    if poses:                                                    # the clouds live in their own frames: T_k p_k is the world point
        T = [GC.pose(*rng.normal(0, 0.05, 3), rng.normal(0, 0.5, 3)) for _ in range(m)]
        for c, Tk in zip(clouds, T):
            w = np.stack([c["x"], c["y"], c["z"]], 1).astype(np.float64)
            l = (w - Tk[:3, 3]) @ Tk[:3, :3]
            c["x"], c["y"], c["z"] = l[:, 0], l[:, 1], l[:, 2]
    return dict(clouds=clouds, T_clouds=T, grid=dict(GRID), params=dict(min_cells=1))


def cloud_cases():
    return dict(street_m1=lambda: street(1, 1), street_m3=lambda: street(2, 3), street_posed=lambda: street(3, 4, poses=True),
                street_conn4=lambda: dict(street(4, 2), params=dict(min_cells=1, connectivity=4)),
                street_defaults=lambda: dict(street(5, 2), params={}),
                street_fence=lambda: dict(street(6, 3), params=dict(labels=[8], min_cells=3)),
                no_clouds=lambda: dict(clouds=[], T_clouds=[], grid=dict(GRID), params={}),
                no_objects=lambda: dict(clouds=[GC.gp([0.1, 0.2], [1.0, 1.1], -1.5)], T_clouds=[GC.EYE], grid=dict(GRID), params={}))
