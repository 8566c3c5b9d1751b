"""The case list of the ground grid's tests, shared by tests/test_grid.py (host function against the numpy restatement) and tests/test_gpu_grid.py
(device against host function).  A case is dict(clouds, T_clouds, params).  With the default G a world point (x, y, z) lands at grid (x, z, -y); gp() builds
points from grid coordinates.  Cells and origins are powers of two where a case sits exactly on a border, so the coordinates are exact in float32."""
import numpy as np
import grid_ref as R

EYE = np.eye(4)


def gp(gx, gy, gz, label=4):
    """points at grid coordinates under the default G and the identity pose"""
    gx, gy, gz, label = np.broadcast_arrays(np.asarray(gx, np.float64), np.asarray(gy, np.float64), np.asarray(gz, np.float64), np.asarray(label, np.int64))
    p = np.zeros(gx.size, R.POINT_DTYPE)
    p["x"] = gx.ravel(); p["y"] = -gz.ravel(); p["z"] = gy.ravel(); p["w"] = 1.0; p["label"] = label.ravel().astype(np.uint32)
    p["b"] = 10; p["g"] = 20; p["r"] = 30
    return p


def case(clouds, params, T_clouds=None):
    clouds = list(clouds)
    return dict(clouds=clouds, T_clouds=[EYE] * len(clouds) if T_clouds is None else list(T_clouds), params=params)


SMALL = dict(x0=-1.0, y0=-1.0, cell=0.25, nx=8, ny=8, h_min=-3.0, h_max=3.0, step=0.25)


def pose(rx, ry, rz, t):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]); Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]); Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4); T[:3, :3] = Rz @ Ry @ Rx; T[:3, 3] = t
    return T


def random_cloud(rng, n, spread=(6.0, 6.0), labels=14):
    """a ground sheet with noise and some points standing on it, labels 0..labels-1 (12 and 13 enter no bin), a few of them 255"""
    gx = rng.uniform(-spread[0], spread[0], n); gy = rng.uniform(0.0, 2 * spread[1], n)
    gz = rng.normal(-1.5, 0.03, n)
    tall = rng.random(n) < 0.3
    gz[tall] += rng.uniform(0.2, 2.5, int(tall.sum()))
    lab = rng.integers(0, labels, n)
    lab[rng.random(n) < 0.05] = 255
    return gp(gx, gy, gz, lab)


def negative_coords():
    # (q.x - x0) / cell in (-1, 0): floor gives -1 (outside), truncation would give cell 0; likewise in y; and one point inside at a negative world coordinate
    return case([gp([-1.1, 0.0, -1.01, -0.6], [0.0, -1.2, -1.01, -0.9], 0.0)], SMALL)


def borders():
    # exactly at x0 (cell 0), on the border of cells 0 | 1 (cell 1), on the last border x0 + nx cell (outside), and the same in y
    xs = [-1.0, -0.75, 1.0, 0.75, 0.0, 0.0, 0.0, 0.0]
    ys = [0.0, 0.0, 0.0, 0.0, -1.0, -0.75, 1.0, 0.75]
    return case([gp(xs, ys, 0.0)], SMALL)


def band_limits():
    lo, hi = np.float32(-3.0), np.float32(3.0)
    gz = [lo, hi, np.nextafter(lo, np.float32(-10)), np.nextafter(hi, np.float32(10)), 0.0]
    return case([gp(0.1, 0.1, np.array(gz, np.float64))], SMALL)


def step_boundary():
    # base 0; base + step_q = 256 exactly is LOW, 257 is HIGH (3 of them: the cell becomes an obstacle)
    gz = np.array([0, 256, 257, 257, 300], np.float64) / 1024.0
    return case([gp(0.1, 0.1, gz, [4, 4, 9, 9, 9])], dict(SMALL, ground_radius=0))


def negative_sum():
    # sum_low = -3 over 2 points: floor -2, truncation -1
    return case([gp(0.1, 0.1, np.array([-1, -2], np.float64) / 1024.0)], SMALL)


def label_tie():
    # LOW: labels 7 7 2 2 -> 2; HIGH: 9 9 8 8 6 -> 8
    gz = [0, 0, 0, 0, 1, 1, 1, 1, 1]
    return case([gp(0.1, 0.1, np.array(gz, np.float64), [7, 7, 2, 2, 9, 9, 8, 8, 6])], SMALL)


def labels_without_bin():
    # labels 12, 255 and 2^32 - 1 enter no bin, LOW and HIGH
    gz = [0, 0, 0, 1, 1, 1]
    return case([gp(0.1, 0.1, np.array(gz, np.float64), [12, 255, 0xFFFFFFFF, 12, 255, 0xFFFFFFFF])], SMALL)


def n_low_zero():
    # the neighbour's points lie 2 m above this cell's: every one of them is HIGH, ground_q falls back to base
    return case([gp([0.1, 0.1, 0.35, 0.35], 0.1, [0.0, 0.01, 2.0, 2.1], [4, 4, 8, 8])], SMALL)


def nonfinite():
    p = gp([0.1] * 9, 0.1, 0.0)
    nan, inf = np.float32("nan"), np.float32("inf")
    p["x"][0] = nan; p["y"][1] = nan; p["z"][2] = nan; p["x"][3] = inf; p["y"][4] = -inf; p["z"][5] = inf
    p["x"][6] = 3e38          # finite, but 1e300 x is not
    p["z"][7] = -3e38
    p["x"][8] = p["y"][8] = p["z"][8] = 0.0
    G = 1e300 * np.array(R.DEFAULTS["G"], np.float64)
    return case([p], dict(SMALL, G=G, h_min=-100.0, h_max=100.0))


def _sheet(nx, ny, cell, x0, y0, seed):
    """one point in the middle of every cell, each at its own height"""
    rng = np.random.default_rng(seed)
    cx, cy = np.meshgrid(np.arange(nx), np.arange(ny))
    gz = rng.permutation(nx * ny).astype(np.float64) / 64.0 - 1.0
    return gp(x0 + (cx.ravel() + 0.5) * cell, y0 + (cy.ravel() + 0.5) * cell, gz, (cx.ravel() + cy.ravel()) % 12)


def radius(r):
    def make():
        P = dict(x0=-1.0, y0=0.0, cell=0.5, nx=5, ny=4, h_min=-3.0, h_max=3.0, step=0.125, ground_radius=r, min_obstacle_points=1)
        return case([_sheet(5, 4, 0.5, -1.0, 0.0, 5)], P)
    return make


def shape(nx, ny):
    def make():
        P = dict(x0=-0.5, y0=0.0, cell=0.125, nx=nx, ny=ny, h_min=-3.0, h_max=3.0, step=0.125, ground_radius=2, min_obstacle_points=2)
        rng = np.random.default_rng(nx * 100 + ny)
        n = 40 * nx * ny
        pts = gp(rng.uniform(-0.6, -0.4 + nx * 0.125, n), rng.uniform(-0.1, 0.1 + ny * 0.125, n), rng.normal(0, 0.2, n), rng.integers(0, 13, n))
        return case([pts[:n // 2], pts[n // 2:]], P)
    return make


def one_cell():
    rng = np.random.default_rng(3)
    n = 300
    return case([gp(rng.uniform(0.01, 0.24, n), rng.uniform(0.26, 0.49, n), rng.normal(-0.5, 0.3, n), rng.integers(0, 12, n))], SMALL)


def obstacle_threshold():
    # two cells: n_high = min_obstacle_points - 1 stays ground, n_high = min_obstacle_points is an obstacle
    gx = [0.1] * 4 + [0.6] * 5
    gz = [0, 1, 1, 0] + [0, 1, 1, 1, 0]
    return case([gp(gx, 0.1, np.array(gz, np.float64), [4] * 4 + [5, 9, 9, 9, 5])], dict(SMALL, ground_radius=0))


def classes():
    # one cell per ground label 0..11 and 255, an obstacle, and the rest unobserved
    gx = -1.0 + (np.arange(14) % 8 + 0.5) * 0.25; gy = -1.0 + (np.arange(14) // 8 + 0.5) * 0.25
    lab = list(range(12)) + [255, 4]
    pts = gp(gx, gy, 0.0, lab)
    tall = gp([gx[13]] * 3, [gy[13]] * 3, 1.0, [9, 9, 255])
    return case([pts, tall], dict(SMALL, ground_radius=0))


def posed(seed, sizes, nx, ny, **kw):
    def make():
        rng = np.random.default_rng(seed)
        clouds = [random_cloud(rng, n) for n in sizes]
        Ts = [pose(*rng.normal(0, 0.05, 3), rng.normal(0, 0.5, 3)) for _ in sizes]
        return case(clouds, dict(dict(x0=-8.0, y0=-3.0, cell=0.8, nx=nx, ny=ny, h_min=-2.0, h_max=0.5, min_obstacle_points=2), **kw), Ts)
    return make


def tilted_frame():
    # a world whose up is not an axis: G from the frame helper's restatement, with a translation
    rng = np.random.default_rng(17)
    G = R.frame_from_up([0.1, -1.0, 0.05], [0.0, 0.1, 1.0]); G[:, 3] = [0.3, -0.2, 1.4]
    return case([random_cloud(rng, 900), random_cloud(rng, 500)], dict(G=G, x0=-8.0, y0=-2.0, cell=0.6, nx=23, ny=21, h_min=-1.0, h_max=2.0, ground_radius=3, min_obstacle_points=2),
                [pose(0.02, -0.03, 0.01, [0.1, 0.2, 0.3]), pose(-0.02, 0.3, 0.0, [1.0, 0.0, 2.0])])


def empty_m0():
    return case([], SMALL)


def empty_m1():
    return case([gp([], [], [])], SMALL)


def cases():
    c = dict(negative_coords=negative_coords, borders=borders, band_limits=band_limits, step_boundary=step_boundary, negative_sum=negative_sum, label_tie=label_tie,
             labels_without_bin=labels_without_bin, n_low_zero=n_low_zero, nonfinite=nonfinite, radius_0=radius(0), radius_1=radius(1), radius_2=radius(2),
             grid_1x1=shape(1, 1), grid_1x7=shape(1, 7), grid_9x1=shape(9, 1), grid_7x3=shape(7, 3), one_cell=one_cell, obstacle_threshold=obstacle_threshold,
             classes=classes, posed_m3=posed(1, (700, 0, 900), 19, 17), posed_m7=posed(2, (65, 0, 1, 300, 191, 64, 257), 17, 19, ground_radius=4, step=0.1),
             tilted_frame=tilted_frame, empty_m0=empty_m0, empty_m1=empty_m1)
    return c
