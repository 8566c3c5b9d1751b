"""Free-space carving restated from DESIGN.md s.16 in numpy float64 and Python integers, and the case list the CPU and GPU tests share.  Written from the section,
not from include/ssm/carve_core.h: the relative pose by the rigid inverse in the section's operation order, one vectorised float64 pass up to the pixel, then
plain Python integers per point.  `carve` also hands out what each verdict was decided on (pixel, zq, tol, d, dmin), so that tests/test_carve.py can assert
that the case list still hits the boundaries it was written for."""
import numpy as np

POINT_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("z", "f4"), ("w", "f4"), ("b", "u1"), ("g", "u1"), ("r", "u1"), ("a", "u1"), ("label", "u4"), ("pad", "u4", (2,))])
UNKNOWN, OCCLUDED, SUPPORTED, SEEN_THROUGH = 0, 1, 2, 3
INFO_FIELDS = ("n_in", "n_kept", "unknown", "occluded", "supported", "seen_through", "removed")
DEFAULTS = dict(min_votes=2, radius=1, tol_abs=0.05, tol_rel_ppm=20000, z_min=0.1)
ZQ_LIMIT = 2 ** 50
EYE = np.eye(4)


def cloud(xyz, seed=1):
    """points with every byte set: a kept point must come back whole"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    p = np.zeros(len(xyz), POINT_DTYPE)
    p["x"], p["y"], p["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    p["w"] = 1.0
    for f in "bgra":
        p[f] = rng.integers(0, 256, len(xyz))
    p["label"] = np.arange(len(xyz), dtype=np.uint32) * 2654435761 % 4294967291
    p["pad"] = rng.integers(0, 2 ** 32, (len(xyz), 2), dtype=np.uint64).astype(np.uint32)
    return p


def rel_pose(T_view, T_cloud):
    """inverse(T_view) . T_cloud -> 3 x 4, the rigid inverse (R^T, -R^T t), every sum left to right"""
    Tv = [[float(v) for v in row] for row in np.asarray(T_view, np.float64)]
    Tc = [[float(v) for v in row] for row in np.asarray(T_cloud, np.float64)]
    M = np.zeros((3, 4))
    for i in range(3):
        a, b, c = Tv[0][i], Tv[1][i], Tv[2][i]          # row i of R^T
        ti = -((a * Tv[0][3] + b * Tv[1][3]) + c * Tv[2][3])
        for j in range(3):
            M[i, j] = (a * Tc[0][j] + b * Tc[1][j]) + c * Tc[2][j]
        M[i, 3] = ((a * Tc[0][3] + b * Tc[1][3]) + c * Tc[2][3]) + ti
    return M


def carve(depth, camera, T_view, pts, T_cloud, run=None, **params):
    """-> dict(points, run_kept, verdict, run, info, why): verdict and run are every point's (run: after the update, before the compaction)"""
    P = dict(DEFAULTS, **params)
    cx, cy, fx, fy, scale = (float(v) for v in camera)
    depth = np.asarray(depth, np.uint16)
    h, w = depth.shape
    n = len(pts)
    r = int(P["radius"])
    run = np.zeros(n, np.uint8) if run is None else np.asarray(run, np.uint8)
    M = rel_pose(T_view, T_cloud)
    x, y, z = (pts[f].astype(np.float64) for f in "xyz")
    with np.errstate(all="ignore"):
        q = [M[i, 0] * x + M[i, 1] * y + M[i, 2] * z + M[i, 3] for i in range(3)]
        ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & np.isfinite(q[0]) & np.isfinite(q[1]) & np.isfinite(q[2])
        ok &= ~(q[2] < float(P["z_min"]))
        u = fx * (q[0] / q[2]) + cx
        v = fy * (q[1] / q[2]) + cy
        px = np.floor(u + 0.5)
        py = np.floor(v + 0.5)
        ok &= (px >= r) & (px <= w - 1 - r) & (py >= r) & (py <= h - 1 - r)          # (false for NaN)
    tol_abs = round(float(P["tol_abs"]) * scale)          # half-even, as llrint
    verdict = np.zeros(n, np.uint8)
    why = [None] * n
    dep = depth.tolist()
    for i in np.nonzero(ok)[0]:
        ix, iy = int(px[i]), int(py[i])
        win = [dep[yy][xx] for yy in range(iy - r, iy + r + 1) for xx in range(ix - r, ix + r + 1)]
        dmin = min(win)
        if dmin == 0:
            why[i] = dict(px=ix, py=iy, zero=True)
            continue
        d = dep[iy][ix]
        zs = float(q[2][i]) * scale
        zq = round(zs) if zs < ZQ_LIMIT else ZQ_LIMIT
        tol = tol_abs + (d * int(P["tol_rel_ppm"])) // 1000000
        why[i] = dict(px=ix, py=iy, zq=zq, tol=tol, d=d, dmin=dmin, zero=False)
        verdict[i] = SEEN_THROUGH if zq + tol < dmin else SUPPORTED if abs(zq - d) <= tol else OCCLUDED
    new = run.astype(np.int64)
    new = np.where(verdict == SEEN_THROUGH, np.minimum(new + 1, 255), np.where(verdict == SUPPORTED, 0, new)).astype(np.uint8)
    keep = new < int(P["min_votes"])
    info = dict(n_in=n, n_kept=int(keep.sum()), unknown=int((verdict == UNKNOWN).sum()), occluded=int((verdict == OCCLUDED).sum()),
                supported=int((verdict == SUPPORTED).sum()), seen_through=int((verdict == SEEN_THROUGH).sum()), removed=int(n - keep.sum()))
    return dict(points=pts[keep], run_kept=new[keep], verdict=verdict, run=new, info=info, why=why, q=q)


# ------------------------------------------------------------------ the case list
F = 64.0          # focal length of the hand-made cases: x = px z / 64 is exact in float32, so the pixel is known by construction


def cam0(scale=1000.0):
    return (0.0, 0.0, F, F, scale)          # (cx, cy, fx, fy, scale)


def at_pixel(px, py, z):
    """the camera-frame point that projects to exactly (px, py) at depth z under cam0 (px, py may end in .5: a tie)"""
    return [px * z / F, py * z / F, z]


def case(depth, pts, camera=None, T_view=EYE, T_cloud=EYE, run=None, **params):
    return dict(depth=np.asarray(depth, np.uint16), camera=camera or cam0(), T_view=np.asarray(T_view, np.float64), T_cloud=np.asarray(T_cloud, np.float64),
                pts=pts if isinstance(pts, np.ndarray) and pts.dtype == POINT_DTYPE else cloud(pts), run=run, params=params)


def every_pixel(w, h, r):
    """one point per pixel and a ring of points one pixel outside, flat depth: the window rule alone decides"""
    def make():
        xy = [(x, y) for y in range(-1, h + 1) for x in range(-1, w + 1)]
        return case(np.full((h, w), 1000), [at_pixel(x, y, 1.0) for x, y in xy], radius=r)
    return make


def ties():
    w, h = 8, 6
    dep = np.full((h, w), 3000)
    dep[:, 1::2] = 1000                                  # odd columns support a point at 1 m, even columns are seen through
    dep2 = np.full((h, w), 3000)
    dep2[1::2, :] = 1000
    pts = [at_pixel(x + 0.5, 2, 1.0) for x in range(-1, w)] + [at_pixel(x + 0.25, 2, 1.0) for x in range(w)] + [at_pixel(x + 0.75, 2, 1.0) for x in range(w - 1)]
    return case(dep, pts, radius=0), case(dep2, [at_pixel(3, y + 0.5, 1.0) for y in range(-1, h)] + [at_pixel(3, y + 0.4375, 1.0) for y in range(h)], radius=0)


def degenerate():
    big = 1.0e30
    nan, inf = float("nan"), float("inf")
    below = float(np.nextafter(np.float32(0.125), np.float32(0)))
    pts = [[0, 0, -1.0], [0.01, 0.01, -0.5], [0, 0, 0.0], [0.0, 0.0, -0.0], at_pixel(2, 2, 0.125), [2 * below / F, 2 * below / F, below], at_pixel(2, 2, 0.25),
           [big, 0, 1], [-big, 0, 1], [0, big, 1], [0, -big, 1], [0, 0, big], [big, big, big], [-big, -big, big], [3.0e38, 3.0e38, 3.0e38],
           [nan, 0, 1], [0, nan, 1], [0, 0, nan], [nan, nan, nan], [inf, 0, 1], [0, -inf, 1], [0, 0, inf], [0, 0, -inf], [1e-30, 1e-30, 1e-38], at_pixel(3, 3, 1.0)]
    return case(np.full((6, 8), 1000), pts, radius=0, z_min=0.125)


def z_min_default():
    """float32(0.1) widened is just above the double 0.1: a point at z_min is tested, the float below it is not"""
    z = np.float32(0.1)
    b = np.nextafter(z, np.float32(0))
    return case(np.full((6, 8), 100), [[0, 0, z], [0, 0, b], [0, 0, np.float32(0.2)]], radius=0)


def zero_corner(r):
    def make():
        w, h = 70, 9
        dep = np.full((h, w), 1000)
        centres = [(10, 4), (20, 4), (30, 4), (40, 4), (50, 4), (60, 4)]
        dep[4 - r, 10 - r] = 0; dep[4 + r, 20 + r] = 0; dep[4 - r, 30 + r] = 0; dep[4 + r, 40 - r] = 0          # the four corners of four windows
        if 60 + r + 1 < w:
            dep[4, 60 + r + 1] = 0                         # just outside the sixth window
        if 4 - r - 1 >= 0:
            dep[4 - r - 1, 50] = 0                         # and just above the fifth
        return case(dep, [at_pixel(x, y, 1.0) for x, y in centres], radius=r)
    return make


def thresholds(r, ppm):
    """points at 1 m (zq = 1000) over pixels whose depth walks through both decisions, at the centre (r = 0) or with the minimum in the window's corner"""
    def make():
        w, h = 70, 9
        dep = np.full((h, w), 5000)
        pts = []
        if r == 0:
            for x, d in enumerate(list(range(925, 955)) + list(range(1045, 1080)), 4):
                dep[4, x] = d
                pts.append(at_pixel(x, 4, 1.0))
            assert x < w
        else:          # the window's minimum, in its corner, decides SEEN_THROUGH over a centre of 1200; a flat window decides SUPPORTED / OCCLUDED
            x = 4
            for dm in (1049, 1050, 1051, 1052, 1072, 1073, 1074, 1075, 1076, 1077):
                dep[4 - r:4 + r + 1, x - r:x + r + 1] = 1200
                dep[4 - r, x + r] = dm
                pts.append(at_pixel(x, 4, 1.0))
                x += 2 * r + 1
            for d in (929, 930, 931, 932, 933, 948, 949, 950, 951):
                dep[4 - r:4 + r + 1, x - r:x + r + 1] = d
                pts.append(at_pixel(x, 4, 1.0))
                x += 2 * r + 1
            assert x - r - 1 < w
        return case(dep, pts, radius=r, tol_rel_ppm=ppm)
    return make


def counters(min_votes):
    """every verdict on counters 0, 1, 2, 254 and 255"""
    def make():
        w, h = 70, 9
        dep = np.full((h, w), 1000)
        dep[:, 20:40] = 3000          # seen through
        dep[:, 40:60] = 500           # occludes
        runs = [0, 1, 2, 254, 255]
        pts, run = [], []
        for k, x0 in enumerate((2, 22, 42)):
            for j, rn in enumerate(runs):
                pts.append(at_pixel(x0 + 3 * j, 4, 1.0)); run.append(rn)
        for rn in runs:
            pts.append([0, 0, -1.0]); run.append(rn)          # unknown
        return case(dep, pts, run=np.uint8(run), min_votes=min_votes)
    return make


def all_or_nothing(seen):
    def make():
        w, h = 70, 9
        xy = [(x, y) for y in range(1, h - 1) for x in range(1, w - 1)]
        return case(np.full((h, w), 3000 if seen else 1000), [at_pixel(x, y, 1.0) for x, y in xy], min_votes=1)
    return make


def pose(rng, rot=0.05, trans=0.3):
    """a rigid pose near the identity: Rodrigues of a small random vector, a random translation"""
    a = rng.normal(0, rot, 3)
    th = float(np.linalg.norm(a))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]]) / max(th, 1e-12)
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = rng.normal(0, trans, 3)
    return T


def scene_depth(w, h, seed, holes=True):
    """a wall with a step, a near box, noise and holes, in millimetres"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    d = 4000 + 6.0 * (xx - w / 2) + rng.normal(0, 6, (h, w))
    d[:, : w // 3] -= 1200
    d[h // 3: 2 * h // 3, w // 2: w // 2 + max(w // 6, 2)] = 1500 + rng.normal(0, 4, (h // 3 * 2 - h // 3, max(w // 6, 2)))
    d = np.clip(d, 300, 60000).astype(np.uint16)
    if holes:
        d[rng.random((h, w)) < 0.02] = 0
    return d


def backproject(depth, camera, stride=1):
    """the camera-frame cloud of a depth image (float32, as RGBDFrame::project2dTo3d gives it), zero depths left out"""
    cx, cy, fx, fy, scale = camera
    h, w = depth.shape
    yy, xx = np.mgrid[0:h:stride, 0:w:stride]
    d = depth[::stride, ::stride]
    m = d > 0
    z = d[m].astype(np.float64) / scale
    x = (xx[m] - cx) * z / fx
    y = (yy[m] - cy) * z / fy
    return np.stack([x, y, z], 1).astype(np.float32)


def posed(w, h, seed, n_max=None, **params):
    """the cloud of one key-frame judged by the depth image of a later one a little way off: every verdict in quantity, no pixel known by construction"""
    def make():
        rng = np.random.default_rng(seed)
        camera = (w / 2 - 0.3, h / 2 + 0.2, 0.9 * w, 0.9 * w, 1000.0)
        Tc, Tv = pose(rng, 0.01, 0.03), pose(rng, 0.01, 0.03)          # (a little way: the two depth images show the same surfaces, up to the motion)
        d0 = scene_depth(w, h, seed)
        d1 = scene_depth(w, h, seed + 1)
        xyz = backproject(d0, camera)
        if n_max is not None and len(xyz) > n_max:
            xyz = xyz[np.sort(rng.choice(len(xyz), n_max, replace=False))]
        run = rng.integers(0, 3, len(xyz)).astype(np.uint8)
        return case(d1, cloud(xyz, seed), camera=camera, T_view=Tv, T_cloud=Tc, run=run, **params)
    return make


def cases():
    """name -> a function that makes the case (a dict: depth, camera, T_view, T_cloud, pts, run, params)"""
    c = {}
    for (w, h) in ((8, 6), (70, 9)):
        for r in (0, 1, 3):
            if 2 * r + 1 <= min(w, h):
                c[f"every_pixel_{w}x{h}_r{r}"] = every_pixel(w, h, r)
    c["ties_u"] = lambda: ties()[0]
    c["ties_v"] = lambda: ties()[1]
    c["degenerate"] = degenerate
    c["z_min_default"] = z_min_default
    for r in (1, 3):
        c[f"zero_corner_r{r}"] = zero_corner(r)
    for r in (0, 1):
        for ppm in (0, 20000):
            c[f"thresholds_r{r}_ppm{ppm}"] = thresholds(r, ppm)
    for mv in (1, 2, 3):
        c[f"counters_votes{mv}"] = counters(mv)
    c["all_removed"] = all_or_nothing(True)
    c["nothing_removed"] = all_or_nothing(False)
    c["posed_70x9"] = posed(70, 9, 3)
    c["posed_70x9_r3"] = posed(70, 9, 4, radius=3, min_votes=1)
    c["posed_160x120"] = posed(160, 120, 5, n_max=3000)
    c["posed_160x120_r0_votes3"] = posed(160, 120, 6, n_max=3000, radius=0, min_votes=3, tol_abs=0.02, tol_rel_ppm=5000)
    return c


def run_case(cs):
    return carve(cs["depth"], cs["camera"], cs["T_view"], cs["pts"], cs["T_cloud"], cs["run"], **cs["params"])
