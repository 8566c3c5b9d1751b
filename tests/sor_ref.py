"""numpy restatement of the statistical outlier removal by brute force, and the case list tests/test_sor.py and tests/test_gpu_sor.py share.

Independent of include/ssm/sor_core.h: all pairs in float32 ((dx*dx + dy*dy) + dz*dz with float differences), a partition for the k smallest, their
float64 roots summed one after the other in ascending order, Python integers for the three sums.  There is no grid here, so `levels` -- the one info field
that describes the search and not its result -- is not restated; every other field is.
"""
import math
import numpy as np

POINT_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("z", "f4"), ("w", "f4"), ("b", "u1"), ("g", "u1"), ("r", "u1"),
                        ("a", "u1"), ("label", "u4"), ("pad", "u4", (2,))])
INFO_FIELDS = ("n_in", "n_finite", "n_kept", "too_few", "sum_q", "sum_q2_lo", "sum_q2_hi", "mean", "stddev", "threshold")
D_LIMIT = 4096.0


def sor(points, mean_k=30, stddev_mul=1.0):
    """-> dict(points, mean_dist, keep, info); ValueError where the library answers SSM_E_INVAL (a mean distance off the statistics grid)"""
    n, k = len(points), int(mean_k)
    xyz = np.stack([points["x"], points["y"], points["z"]], axis=1).astype(np.float32) if n else np.zeros((0, 3), np.float32)
    fin = np.isfinite(xyz).all(axis=1)
    F = xyz[fin]
    nf = len(F)
    md, keep = np.zeros(n, np.float32), np.zeros(n, np.uint8)
    info = dict(n_in=n, n_finite=nf, n_kept=0, too_few=0, sum_q=0, sum_q2_lo=0, sum_q2_hi=0, mean=0.0, stddev=0.0, threshold=0.0)
    if nf < k + 1:
        info["too_few"] = 1
        keep[fin] = 1
    else:
        d = np.empty(nf, np.float32)
        step = max(1, (1 << 22) // nf)
        with np.errstate(over="ignore"):
            for a in range(0, nf, step):
                b = min(nf, a + step)
                dx = F[a:b, None, 0] - F[None, :, 0]
                dy = F[a:b, None, 1] - F[None, :, 1]
                dz = F[a:b, None, 2] - F[None, :, 2]
                d2 = (dx * dx + dy * dy) + dz * dz
                assert d2.dtype == np.float32
                d2[np.arange(b - a), np.arange(a, b)] = np.inf          # the point itself; an exact duplicate stays, with 0
                part = np.partition(d2, k - 1, axis=1)[:, :k]
                part.sort(axis=1)
                r = np.sqrt(part.astype(np.float64))
                s = np.zeros(b - a, np.float64)
                for t in range(k):
                    s = s + r[:, t]
                d[a:b] = (s / np.float64(k)).astype(np.float32)
        if not (d < np.float32(D_LIMIT)).all():
            raise ValueError("a mean distance off the statistics grid")
        s1 = lo = hi = 0
        for v in d:
            q = int(np.rint(float(v) * 1048576.0))          # half-even
            s1 += q
            lo += (q * q) & 0xFFFFFFFF
            hi += (q * q) >> 32
        a = float(s1) * (1.0 / 1048576.0)
        b = (float(hi) * 4294967296.0 + float(lo)) * (1.0 / 1048576.0) * (1.0 / 1048576.0)
        mean = a / float(nf)
        var = (b - a * a / float(nf)) / float(nf - 1)
        sd = math.sqrt(var if var > 0.0 else 0.0)
        thr = mean + float(stddev_mul) * sd
        info.update(sum_q=s1, sum_q2_lo=lo, sum_q2_hi=hi, mean=mean, stddev=sd, threshold=thr)
        md[fin] = d
        keep[fin] = (d.astype(np.float64) <= thr).astype(np.uint8)
    info["n_kept"] = int(keep.sum())
    return dict(points=points[keep == 1], mean_dist=md, keep=keep, info=info)


# ---------------------------------------------------------------------------------------------------------------- the cases
def cloud(xyz, seed=0):
    """points of POINT_DTYPE at xyz with every other byte set, so that a kept point can be checked in all its 32 bytes"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    rng = np.random.default_rng(1000 + seed)
    p = np.zeros(len(xyz), POINT_DTYPE)
    p["x"], p["y"], p["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    p["w"] = 1.0
    for f in ("b", "g", "r", "a"):
        p[f] = rng.integers(0, 256, len(xyz))
    p["label"] = rng.integers(0, 12, len(xyz))
    p["pad"] = rng.integers(0, 2 ** 32, (len(xyz), 2), dtype=np.uint64).astype(np.uint32)
    return p


def _uniform(n, seed, lo=0.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(np.float32)


def backprojected(w, h, seed=7, speckles=0):
    """a synthetic depth frame through the pinhole model: a floor, a back wall and two boxes, depth in millimetres as the sensor gives it; `speckles` pixels
    get a depth of their own, well in front of the scene.  -> (points in pixel order, the indices of the speckles' points)"""
    rng = np.random.default_rng(seed)
    fx = fy = 517.0 * w / 640.0
    cx, cy = w / 2.0 - 0.5, h / 2.0 - 0.5
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    z = np.full((h, w), 12.0)                                     # the wall
    below = v > cy + 1
    z[below] = np.minimum(z[below], 1.4 * fy / (v[below] - cy))  # the floor, 1.4 m under the camera
    for (x0, x1, y0, y1, zz) in ((0.15, 0.35, 0.3, 0.8, 3.0), (0.6, 0.8, 0.45, 0.9, 5.5)):
        z[int(y0 * h):int(y1 * h), int(x0 * w):int(x1 * w)] = np.minimum(z[int(y0 * h):int(y1 * h), int(x0 * w):int(x1 * w)], zz)
    depth = np.rint(z * 1000.0 + rng.normal(0.0, 2.0, (h, w))).astype(np.int64)
    depth[rng.random((h, w)) < 0.02] = 0                          # holes
    sp = rng.choice(w * h, speckles, replace=False) if speckles else np.zeros(0, np.int64)
    depth.reshape(-1)[sp] = rng.integers(900, 1500, len(sp))
    valid = depth.reshape(-1) > 0
    zf = (depth.reshape(-1)[valid] / 1000.0).astype(np.float32)
    xf = ((u.reshape(-1)[valid] - cx) * zf / fx).astype(np.float32)
    yf = ((v.reshape(-1)[valid] - cy) * zf / fy).astype(np.float32)
    at = np.cumsum(valid) - 1
    return cloud(np.stack([xf, yf, zf], axis=1), seed), at[sp]


def planted(seed=3):
    """a jittered plane of 2000 points and 12 points planted far above it -> (points, the planted indices)"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(50), np.arange(40)), axis=-1).reshape(-1, 2) * 0.02
    xyz = np.concatenate([g + rng.normal(0, 0.002, g.shape), rng.normal(0, 0.002, (len(g), 1))], axis=1)
    far = np.stack([rng.uniform(0, 1.0, 12), rng.uniform(0, 0.8, 12), rng.uniform(0.5, 3.0, 12)], axis=1)
    at = np.sort(rng.choice(len(xyz) + 12, 12, replace=False))
    full = np.zeros((len(xyz) + 12, 3))
    mask = np.zeros(len(full), bool)
    mask[at] = True
    full[mask], full[~mask] = far, xyz
    return cloud(full, seed), at


def cases(chunk):
    """name -> function -> (points, mean_k, stddev_mul, cell).  chunk: ssm_sor_chunk(), the device search's LDS chunk"""
    K = 30
    c = {}
    for n in (0, 1, K, K + 1, K + 2, 63, 64, 65):
        c[f"n_{n}"] = lambda n=n: (cloud(_uniform(n, 10 + n), n), K, 1.0, 0.0)
    c["random_3000"] = lambda: (cloud(_uniform(3000, 1)), K, 1.0, 0.0)
    c["identical"] = lambda: (cloud(np.tile(np.float32([[0.25, -1.5, 3.0]]), (100, 1))), K, 1.0, 0.0)

    def duplicates():
        a = _uniform(150, 2)
        return cloud(np.concatenate([a, a[:90], a[:40], _uniform(60, 3)])), K, 1.0, 0.0
    c["duplicates"] = duplicates

    def non_finite():
        a = _uniform(300, 4)
        a[17, 0] = np.nan
        a[120, 2] = np.inf
        a[299, 1] = -np.inf
        return cloud(a), K, 1.0, 0.0
    c["non_finite"] = non_finite
    c["non_finite_too_few"] = lambda: (cloud(np.float32([[0, 0, 0], [np.nan, 0, 0], [1, 1, 1], [0, np.inf, 0], [2, 0, 1]])), 3, 1.0, 0.0)
    c["negative"] = lambda: (cloud(_uniform(400, 5, -5.0, -1.0)), K, 1.0, 0.0)

    def lattice():          # every coordinate an exact multiple of the cell size, on both sides of zero
        g = np.stack(np.meshgrid(np.arange(-4, 4), np.arange(-4, 4), np.arange(-4, 4)), axis=-1).reshape(-1, 3) * 0.25
        return cloud(g), K, 1.0, 0.25
    c["cell_multiples"] = lattice

    def doubling_line():    # gaps that double: every level of the ladder settles a few
        x = 0.001 * (2.0 ** np.arange(22) - 1.0)          # up to 2 km: the mean distances stay on the statistics grid
        return cloud(np.stack([x, np.zeros(22), np.zeros(22)], axis=1)), 8, 1.0, 0.001
    c["doubling_line"] = doubling_line

    def far_clusters():     # farther apart, in cells, than a key axis holds: the first cell size is raised
        a, b = _uniform(100, 6, 0.0, 0.01), _uniform(100, 7, 0.0, 0.01)
        b[:, 0] += 3000.0
        return cloud(np.concatenate([a, b])), K, 1.0, 0.001
    c["far_clusters"] = far_clusters

    def k_cluster():        # exactly k points beside a far cluster: each needs one neighbour from over there, which only the top level sees
        a, b = _uniform(K, 8, 0.0, 0.05), _uniform(100, 9, 0.0, 0.05)
        b[:, 1] += 50.0
        return cloud(np.concatenate([a, b])), K, 1.0, 0.01
    c["k_cluster_beside_far"] = k_cluster
    # one cell that holds every point: the candidate list is longer than the LDS chunk
    c["one_cell"] = lambda: (cloud(_uniform(max(5000, 9 * chunk + 392), 11, 0.0, 0.5)), K, 1.0, 1.0)
    for k in (1, 8, 30, 32, 33, 50, 64):
        c[f"k_{k}"] = lambda k=k: (cloud(_uniform(500, 12)), k, 1.0, 0.0)
    for m in (0.0, 1.0, 2.5):
        c[f"mul_{m}"] = lambda m=m: (cloud(_uniform(500, 13)), K, m, 0.0)
    c["frame_160x120"] = lambda: (backprojected(160, 120, speckles=20)[0], K, 1.0, 0.0)
    return c


CELLS = (0.0, 1e-6, 1.0, 1e30)          # automatic, tiny, 1 and huge: the first cell size is a tuning parameter and changes no output
