"""Object extraction restated in numpy / scipy, independently of include/ssm/objects_core.h: the components are scipy.ndimage.label's, one label
value at a time; a root is the smallest linear index of a component; the figures come from numpy reductions over each component's cells and points.  cells() is
what ssm_objects_cells_host returns, run() what ssm_objects_host returns (the grid is tests/grid_ref.py's)."""
import numpy as np
from scipy import ndimage
import grid_ref as GR

OBJECT_DTYPE = np.dtype([("root", "i4"), ("label", "i4"), ("cells", "u4"), ("n_points", "u4"), ("cell_points", "u8"), ("cx_min", "i4"), ("cx_max", "i4"), ("cy_min", "i4"),
                         ("cy_max", "i4"), ("ground_q", "i4"), ("top_q", "i4"), ("x_min_q", "i4"), ("x_max_q", "i4"), ("y_min_q", "i4"), ("y_max_q", "i4"), ("z_min_q", "i4"),
                         ("z_max_q", "i4"), ("n_label", "u4"), ("pad", "u4"), ("sum_x", "i8"), ("sum_y", "i8"), ("sum_z", "i8")])
INFO_FIELDS = ("member_cells", "components", "kept", "rejected_cells", "rejected_points", "rejected_height", "n_in", "object_points")
DEFAULTS = dict(label_mask=(1 << 9) | (1 << 10) | (1 << 11), connectivity=8, min_cells=2, min_points=20, min_height=0.3)
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
STRUCTURE = {4: [[0, 1, 0], [1, 1, 1], [0, 1, 0]], 8: [[1, 1, 1], [1, 1, 1], [1, 1, 1]]}


def height_units(min_height):
    return 1 << 42 if min_height >= 4194304.0 else int(np.rint(np.float64(min_height) * 1024.0))


def params_of(params):
    P = dict(DEFAULTS, **params)
    if "labels" in P:
        P["label_mask"] = sum({1 << int(l) for l in P.pop("labels")})
    return P


def empty_record():
    o = np.zeros((), OBJECT_DTYPE)
    for f in ("x_min_q", "y_min_q", "z_min_q"):
        o[f] = I32_MAX
    for f in ("x_max_q", "y_max_q", "z_max_q"):
        o[f] = I32_MIN
    return o


def cells(cls, obstacle_label, ground_q, top_q, n_high, **params):
    """-> (records of the kept components in ascending root order, object_id, info, every component's (root, verdict))"""
    P = params_of(params)
    ny, nx = cls.shape
    found = []
    for lab in range(12):
        if not (P["label_mask"] >> lab) & 1:
            continue
        part, n = ndimage.label((cls == GR.OBSTACLE) & (obstacle_label == lab), structure=STRUCTURE[P["connectivity"]])
        for k in range(1, n + 1):
            at = np.flatnonzero(part.ravel() == k)
            found.append((int(at.min()), lab, at))
    found.sort(key=lambda f: f[0])
    info = dict.fromkeys(INFO_FIELDS, 0)
    info["components"] = len(found); info["member_cells"] = sum(len(f[2]) for f in found)
    object_id = np.full((ny, nx), -1, np.int32)
    records, verdicts = [], []
    for root, lab, at in found:
        o = empty_record()
        cy, cx = at // nx, at % nx
        o["root"] = root; o["label"] = lab; o["cells"] = len(at); o["cell_points"] = int(n_high.ravel()[at].astype(np.int64).sum())
        o["cx_min"], o["cx_max"], o["cy_min"], o["cy_max"] = cx.min(), cx.max(), cy.min(), cy.max()
        o["ground_q"] = ground_q.ravel()[at].min(); o["top_q"] = top_q.ravel()[at].max()
        if len(at) < P["min_cells"]:
            v = "rejected_cells"
        elif int(o["cell_points"]) < P["min_points"]:
            v = "rejected_points"
        elif int(o["top_q"]) - int(o["ground_q"]) < height_units(P["min_height"]):
            v = "rejected_height"
        else:
            v = "kept"
            object_id.ravel()[at] = len(records)
            records.append(o)
        info[v] += 1
        verdicts.append((root, v))
    rec = np.array(records, OBJECT_DTYPE) if records else np.zeros(0, OBJECT_DTYPE)
    return rec, object_id, info, verdicts


def run(clouds, T_clouds, grid, **params):
    """-> (records, object_id, the per-point ids of the concatenation, info, the grid's restatement)"""
    G = dict(GR.DEFAULTS, **grid)
    g = GR.run(clouds, T_clouds, G)
    rec, object_id, info, _ = cells(g["cls"], g["obstacle_label"], g["ground_q"], g["top_q"], g["n_high"], **params)
    info["n_in"] = g["info"]["n_in"]
    ids_all = []
    for cl, T, pc in zip(clouds, T_clouds, g["points"]):
        M = GR.grid_pose(G["G"], T)
        x, y, z = (cl[k].astype(np.float64) for k in "xyz")
        ids = np.full(len(cl), -1, np.int32)
        u = np.flatnonzero((pc["status"] == GR.USED) & ~pc["low"])
        cell_id = object_id[pc["cyd"][u].astype(np.int64), pc["cxd"][u].astype(np.int64)]
        ids[u] = cell_id
        on = u[cell_id >= 0]
        with np.errstate(all="ignore"):
            q = [np.rint((M[r, 0] * x[on] + M[r, 1] * y[on] + M[r, 2] * z[on] + M[r, 3]) * 1024.0).astype(np.int64) for r in range(3)]
        for k in range(len(rec)):
            mine = ids[on] == k
            if not mine.any():
                continue
            o = rec[k]
            o["n_points"] += int(mine.sum()); o["n_label"] += int((cl["label"][on][mine].astype(np.int64) == int(o["label"])).sum())
            for a, name in enumerate("xyz"):
                v = q[a][mine]
                o[name + "_min_q"] = min(int(o[name + "_min_q"]), int(v.min())); o[name + "_max_q"] = max(int(o[name + "_max_q"]), int(v.max()))
                o["sum_" + name] += int(v.sum())
        info["object_points"] += len(on)
        ids_all.append(ids)
    ids_all = np.concatenate(ids_all) if ids_all else np.zeros(0, np.int32)
    return rec, object_id, ids_all, info, g
