"""The ground grid restated in numpy, independently of include/ssm/grid_core.h: float64 arithmetic in the section's operation order (numpy does
not contract a * b + c), integer accumulators, Python's floor division.  run() returns what ssm_grid_host returns -- the seven cell arrays, the raw cells, the
info -- and per point what became of it, for the case list's own properties."""
import numpy as np

POINT_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("z", "f4"), ("w", "f4"), ("b", "u1"), ("g", "u1"), ("r", "u1"), ("a", "u1"), ("label", "u4"), ("pad", "u4", (2,))])
CELL_DTYPE = np.dtype([("n", "u4"), ("hmin", "i4"), ("hmax", "i4"), ("base", "i4"), ("n_low", "u4"), ("n_high", "u4"), ("sum_low", "i8"), ("hist_low", "u4", (12,)),
                       ("hist_high", "u4", (12,))])
ARRAYS = ("cls", "ground_label", "obstacle_label", "ground_q", "top_q", "n", "n_high")
INFO_FIELDS = ("n_in", "n_finite", "out_of_band", "outside", "n_used", "unobserved", "drivable", "walkable", "other_ground", "obstacle")
DEFAULTS = dict(G=[[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0]], x0=-51.2, y0=-10.0, cell=0.2, nx=512, ny=512, h_min=-3.0, h_max=3.0, step=0.3, ground_radius=1,
                min_obstacle_points=3)
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
REJECTED, OUT_OF_BAND, OUTSIDE, USED = 0, 1, 2, 3
UNOBSERVED, DRIVABLE, WALKABLE, OTHER_GROUND, OBSTACLE = 0, 1, 2, 3, 4
EYE = np.eye(4)


def grid_pose(G, T):
    """M = G . T, 3 x 4: the products summed left to right, G's translation added last"""
    G = np.asarray(G, np.float64).reshape(3, 4); T = np.asarray(T, np.float64)
    M = np.zeros((3, 4))
    for i in range(3):
        a, b, c = G[i, 0], G[i, 1], G[i, 2]
        for j in range(3):
            M[i, j] = (a * T[0, j] + b * T[1, j]) + c * T[2, j]
        M[i, 3] = ((a * T[0, 3] + b * T[1, 3]) + c * T[2, 3]) + G[i, 3]
    return M


def frame_from_up(up, forward):
    up = np.asarray(up, np.float64); f = np.asarray(forward, np.float64)
    lu = np.sqrt((up[0] * up[0] + up[1] * up[1]) + up[2] * up[2])
    z = up / lu
    d = (f[0] * z[0] + f[1] * z[1]) + f[2] * z[2]
    yr = f - d * z
    ly = np.sqrt((yr[0] * yr[0] + yr[1] * yr[1]) + yr[2] * yr[2])
    y = yr / ly
    x = np.array([y[1] * z[2] - y[2] * z[1], y[2] * z[0] - y[0] * z[2], y[0] * z[1] - y[1] * z[0]])
    G = np.zeros((3, 4))
    G[0, :3], G[1, :3], G[2, :3] = x, y, z
    return G


def step_units(step):
    return 1 << 42 if step >= 4294967296.0 else int(np.rint(np.float64(step) * 1024.0))


def points_of(cloud, M, P):
    """per point of one cloud: status, cell x, cell y (as doubles), quantised height"""
    x, y, z = (cloud[k].astype(np.float64) for k in "xyz")
    with np.errstate(all="ignore"):
        q = [M[r, 0] * x + M[r, 1] * y + M[r, 2] * z + M[r, 3] for r in range(3)]
        fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & np.isfinite(q[0]) & np.isfinite(q[1]) & np.isfinite(q[2])
        band = (P["h_min"] <= q[2]) & (q[2] <= P["h_max"])
        cxd = np.floor((q[0] - P["x0"]) / P["cell"]); cyd = np.floor((q[1] - P["y0"]) / P["cell"])
        inside = (cxd >= 0) & (cxd <= P["nx"] - 1) & (cyd >= 0) & (cyd <= P["ny"] - 1)
        hq = np.where(fin & band, np.rint(np.where(fin & band, q[2], 0.0) * 1024.0), 0.0).astype(np.int64)
    st = np.where(~fin, REJECTED, np.where(~band, OUT_OF_BAND, np.where(~inside, OUTSIDE, USED)))
    return st, cxd, cyd, hq


def majority(hist):
    best, lab = 0, 255
    for i in range(12):
        if hist[i] > best:
            best, lab = int(hist[i]), i
    return lab


def run(clouds, T_clouds, params):
    P = dict(DEFAULTS, **params)
    nx, ny, R = P["nx"], P["ny"], P["ground_radius"]
    step_q = step_units(P["step"])
    cells = np.zeros((ny, nx), CELL_DTYPE)
    cells["hmin"] = I32_MAX; cells["hmax"] = I32_MIN; cells["base"] = I32_MAX
    info = dict.fromkeys(INFO_FIELDS, 0)
    per_cloud = []
    for cl, T in zip(clouds, T_clouds):
        st, cxd, cyd, hq = points_of(cl, grid_pose(P["G"], T), P)
        per_cloud.append(dict(status=st, cxd=cxd, cyd=cyd, hq=hq, low=np.zeros(len(cl), bool)))
        info["n_in"] += len(cl); info["n_finite"] += int((st != REJECTED).sum()); info["out_of_band"] += int((st == OUT_OF_BAND).sum())
        info["outside"] += int((st == OUTSIDE).sum()); info["n_used"] += int((st == USED).sum())
        u = st == USED
        cx, cy = cxd[u].astype(np.int64), cyd[u].astype(np.int64)
        np.add.at(cells["n"], (cy, cx), 1); np.minimum.at(cells["hmin"], (cy, cx), hq[u]); np.maximum.at(cells["hmax"], (cy, cx), hq[u])
    for cy, cx in np.argwhere(cells["n"] > 0):
        win = cells[max(cy - R, 0):min(cy + R, ny - 1) + 1, max(cx - R, 0):min(cx + R, nx - 1) + 1]
        cells["base"][cy, cx] = win["hmin"][win["n"] > 0].min()
    for cl, pc in zip(clouds, per_cloud):
        u = np.flatnonzero(pc["status"] == USED)
        cx, cy = pc["cxd"][u].astype(np.int64), pc["cyd"][u].astype(np.int64)
        hq = pc["hq"][u]; lab = cl["label"][u].astype(np.int64)
        low = hq <= cells["base"][cy, cx].astype(np.int64) + step_q
        pc["low"][u] = low
        np.add.at(cells["n_low"], (cy[low], cx[low]), 1); np.add.at(cells["sum_low"], (cy[low], cx[low]), hq[low]); np.add.at(cells["n_high"], (cy[~low], cx[~low]), 1)
        kl, kh = low & (lab <= 11), ~low & (lab <= 11)
        np.add.at(cells["hist_low"], (cy[kl], cx[kl], lab[kl]), 1); np.add.at(cells["hist_high"], (cy[kh], cx[kh], lab[kh]), 1)
    out = {"cls": np.zeros((ny, nx), np.uint8), "ground_label": np.full((ny, nx), 255, np.uint8), "obstacle_label": np.full((ny, nx), 255, np.uint8),
           "ground_q": np.full((ny, nx), I32_MIN, np.int32), "top_q": np.full((ny, nx), I32_MIN, np.int32), "n": cells["n"].copy(), "n_high": cells["n_high"].copy()}
    for cy, cx in np.argwhere(cells["n"] > 0):
        c = cells[cy, cx]
        obstacle = int(c["n_high"]) >= P["min_obstacle_points"]
        out["ground_q"][cy, cx] = int(c["sum_low"]) // int(c["n_low"]) if c["n_low"] else int(c["base"])          # Python's // floors
        out["top_q"][cy, cx] = c["hmax"]
        gl = majority(c["hist_low"])
        out["ground_label"][cy, cx] = gl
        if obstacle:
            out["obstacle_label"][cy, cx] = majority(c["hist_high"])
        out["cls"][cy, cx] = OBSTACLE if obstacle else DRIVABLE if gl in (3, 4) else WALKABLE if gl == 5 else OTHER_GROUND
    for k, name in enumerate(INFO_FIELDS[5:]):
        info[name] = int((out["cls"] == k).sum())
    out["cells"] = cells; out["info"] = info; out["points"] = per_cloud
    return out


def colours(cls, ground_label, obstacle_label, ground_q, h_min, palette):
    """the BGR and the 16-bit height image; palette: 12 BGR triples"""
    ny, nx = cls.shape
    bgr = np.zeros((ny, nx, 3), np.uint8); height = np.zeros((ny, nx), np.uint16)
    h0 = int(np.rint(np.float64(h_min) * 1024.0))
    for r in range(ny):
        for x in range(nx):
            cy = ny - 1 - r
            if cls[cy, x] == UNOBSERVED:
                continue
            if cls[cy, x] == OBSTACLE:
                bgr[r, x] = palette[obstacle_label[cy, x]] if obstacle_label[cy, x] < 12 else (255, 255, 255)
            else:
                bgr[r, x] = palette[ground_label[cy, x]] if ground_label[cy, x] < 12 else (64, 64, 64)
            height[r, x] = min(max(int(ground_q[cy, x]) - h0, 0), 65534) + 1
    return bgr, height
