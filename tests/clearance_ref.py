"""A numpy / scipy restatement of the clearance map by brute force, for the tests: dist2 and nearest are the minimum, over ALL blocked cells, of the
key (d2 << 24) | index -- every cell against every blocked cell, no separable pass --; the traversable cells come from the masks and r2, their components from
scipy.ndimage.label, the seed from the minimum of its own key.  Small grids only (the work is cells x blocked cells)."""
import math
import numpy as np
from scipy import ndimage

UINT32_MAX = 0xFFFFFFFF
DEFAULTS = dict(blocked_mask=1 << 4, free_mask=1 << 1, connectivity=4, seed_cx=-1, seed_cy=-1, seed_snap=10, radius=1.0, cell=1.0)
INFO_FIELDS = ("blocked", "free_cells", "traversable", "components", "reachable", "seed_cell", "max_d2_reachable", "r2")


def params_of(kw):
    """the binding's keywords -> the eight fields"""
    P = dict(DEFAULTS)
    for k, v in kw.items():
        if k in ("blocked", "free"):
            P[k + "_mask"] = sum({1 << int(c) for c in v})
        elif k == "seed":
            P["seed_cx"], P["seed_cy"] = (-1, -1) if v is None else (int(v[0]), int(v[1]))
        else:
            assert k in DEFAULTS, k
            P[k] = v
    return P


def r2_of(radius, cell):
    q = float(radius) / float(cell)
    q2 = q * q
    return 1 << 31 if not q2 < 2147483648.0 else int(math.floor(q2))


def in_mask(cls, mask):
    cls = np.asarray(cls, np.int64)
    return (cls < 5) & (((mask >> np.minimum(cls, 31)) & 1) != 0)


def distance(blocked):
    """blocked: ny x nx bool -> (dist2 uint32, nearest int32), every cell against every blocked cell"""
    ny, nx = blocked.shape
    by, bx = np.nonzero(blocked)
    d2 = np.full((ny, nx), UINT32_MAX, np.uint32); near = np.full((ny, nx), -1, np.int32)
    if len(by) == 0:
        return d2, near
    bidx = (by * nx + bx).astype(np.int64)
    xs = np.arange(nx, dtype=np.int64)
    for y in range(ny):
        dd = (xs[:, None] - bx[None, :]) ** 2 + (y - by[None, :]) ** 2
        key = ((dd << 24) | bidx[None, :]).min(axis=1)
        d2[y] = (key >> 24).astype(np.uint32); near[y] = (key & 0xFFFFFF).astype(np.int32)
    return d2, near


def run(cls, **kw):
    """-> (dist2, nearest, reach, info) as ssm_clearance_cells_host gives them"""
    P = params_of(kw)
    cls = np.ascontiguousarray(cls, np.uint8)
    ny, nx = cls.shape
    blocked = in_mask(cls, P["blocked_mask"]); free = in_mask(cls, P["free_mask"])
    r2 = r2_of(P["radius"], P["cell"])
    d2, near = distance(blocked)
    trav = free & (d2.astype(np.int64) > r2)
    structure = np.ones((3, 3), int) if P["connectivity"] == 8 else ndimage.generate_binary_structure(2, 1)
    lab, ncomp = ndimage.label(trav, structure=structure)
    seed_cell = -1
    if P["seed_cx"] >= 0:
        ys, xs = np.nonzero(trav)
        dd = (xs.astype(np.int64) - P["seed_cx"]) ** 2 + (ys.astype(np.int64) - P["seed_cy"]) ** 2
        ok = dd <= P["seed_snap"] ** 2
        if ok.any():
            seed_cell = int((((dd[ok] << 24) | (ys[ok] * nx + xs[ok])).min()) & 0xFFFFFF)
    reach = trav.astype(np.uint8)
    if seed_cell >= 0:
        reach[lab == lab.ravel()[seed_cell]] = 2
    reached = reach == 2
    info = dict(blocked=int(blocked.sum()), free_cells=int(free.sum()), traversable=int(trav.sum()), components=int(ncomp), reachable=int(reached.sum()), seed_cell=seed_cell,
                max_d2_reachable=int(d2[reached].max()) if reached.any() else 0, r2=r2)
    return d2, near, reach, info
