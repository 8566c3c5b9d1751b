"""Label fusion restated from DESIGN.md s.20 in numpy and Python integers, and the case list the CPU and GPU tests share.  Written from the section, not from
include/ssm/relabel_core.h: whether a view supports a point, and at which pixel, is tests/carve_ref.py's restatement of s.16 (steps 1-7); the vote, the twelve
counters (a plain list here, packed only at the end) and the decision are plain Python per point.  `relabel` also hands out what each point's result was decided
on, so that tests/test_relabel.py can assert that the case list still holds the situations it was written for."""
import json
import os
import numpy as np
import carve_ref
from carve_ref import POINT_DTYPE, SUPPORTED, EYE, at_pixel, cam0

PALETTE = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "palette.json")))["palette_bgr"]
INFO_FIELDS = ("n_in", "n_supported", "n_voted", "n_changed", "n_filled", "pairs_supported", "pairs_voted")
DEFAULTS = dict(radius=1, edge_guard=1, own_weight=1, min_votes=2, tol_abs=0.05, tol_rel_ppm=20000, z_min=0.1)


def labels_of_bgr(sem):
    """h x w x 3 -> h x w: the palette's class, 255 for every other colour"""
    sem = np.asarray(sem, np.uint8)
    out = np.full(sem.shape[:2], 255, np.uint8)
    for l, c in enumerate(PALETTE):
        out[(sem == np.uint8(c)).all(axis=2)] = l
    return out


def bgr_of_labels(label, stray=(1, 2, 3)):
    """a semantic image whose label image is `label`: 255 becomes a colour outside the palette"""
    label = np.asarray(label)
    sem = np.zeros(label.shape + (3,), np.uint8)
    sem[:] = stray
    for l, c in enumerate(PALETTE):
        sem[label == l] = c
    return sem


def relabel(views, T_views, pts, T_cloud, **params):
    """views: dicts (depth, label, camera) -> dict(labels, votes, info, why): why[i] = dict(counts, guarded: views whose vote only the edge guard withheld)"""
    P = dict(DEFAULTS, **params)
    n, r = len(pts), int(P["radius"])
    counts = [[0] * 12 for _ in range(n)]
    guarded = [[] for _ in range(n)]
    sup = np.zeros(n, np.int64); voted = np.zeros(n, np.int64)
    L0 = [int(v) for v in pts["label"]]
    for i in range(n):
        if L0[i] <= 11:
            counts[i][L0[i]] += int(P["own_weight"])
    for k, (V, T) in enumerate(zip(views, T_views)):
        res = carve_ref.carve(V["depth"], V["camera"], T, pts, T_cloud, min_votes=1, radius=r, tol_abs=P["tol_abs"], tol_rel_ppm=P["tol_rel_ppm"], z_min=P["z_min"])
        lab = np.asarray(V["label"], np.uint8)
        for i in np.nonzero(res["verdict"] == SUPPORTED)[0]:
            sup[i] += 1
            px, py = res["why"][i]["px"], res["why"][i]["py"]
            l = int(lab[py, px])
            if l > 11:
                continue
            if int(P["edge_guard"]) and not (lab[py - r:py + r + 1, px - r:px + r + 1] == l).all():
                guarded[i].append(k)
                continue
            counts[i][l] += 1
            voted[i] += 1
    labels = np.array(L0, np.uint32).reshape(n)
    for i in range(n):
        best = max(counts[i])
        if best == 0:
            continue
        winner = L0[i] if L0[i] <= 11 and counts[i][L0[i]] == best else counts[i].index(best)
        if winner != L0[i] and best >= int(P["min_votes"]):
            labels[i] = winner
    votes = np.array([sum(c << (5 * l) for l, c in enumerate(cs)) for cs in counts], np.uint64).reshape(n)
    changed = labels != pts["label"]
    info = dict(n_in=n, n_supported=int((sup > 0).sum()), n_voted=int((voted > 0).sum()), n_changed=int(changed.sum()), n_filled=int((changed & (pts["label"] > 11)).sum()),
                pairs_supported=int(sup.sum()), pairs_voted=int(voted.sum()))
    return dict(labels=labels, votes=votes, info=info, why=[dict(counts=counts[i], guarded=guarded[i]) for i in range(n)])


# ------------------------------------------------------------------ the case list
def view(depth, label, camera=None):
    depth = np.asarray(depth, np.uint16); label = np.asarray(label, np.uint8)
    assert depth.shape == label.shape
    return dict(depth=depth, label=label, camera=camera or cam0())


def case(views, pts, T_views=None, T_cloud=EYE, **params):
    return dict(views=views, T_views=[np.asarray(T, np.float64) for T in (T_views if T_views is not None else [EYE] * len(views))], pts=pts,
                T_cloud=np.asarray(T_cloud, np.float64), params=params)


def labelled(xyz, labels, seed=1):
    p = carve_ref.cloud(xyz, seed)
    p["label"] = np.asarray(labels, np.uint32)
    return p


U = 255          # a view's unknown label


def constructed(edge_guard=1):
    """hand-made points over four flat views (the fourth of another size): each point's 3 x 3 window in each view is painted for one situation"""
    def make():
        sizes = [(40, 9), (40, 9), (40, 9), (48, 11)]
        dep = [np.full((h, w), 1000) for w, h in sizes]
        lab = [np.full((h, w), U) for w, h in sizes]
        pts, own, names = [], [], []

        def point(name, L0, votes, corner=None, depth=None):
            x = 2 + 3 * len(pts)
            assert x + 1 < 40
            for k, l in enumerate(votes):
                lab[k][3:6, x - 1:x + 2] = l
            if corner is not None:
                k, l = corner
                lab[k][3, x + 1] = l
            if depth is not None:
                k, d = depth
                dep[k][4, x] = d
            pts.append(at_pixel(x, 4, 1.0)); own.append(L0); names.append(name)

        point("tie_own_wins", 3, [5, U, U, U])
        point("tie_lowest_id", U, [7, 7, 4, 4])
        point("tie_lowest_id_own_loses", 9, [7, 4, 7, 4])
        point("edge_guard", 2, [6, 6, U, U], corner=(1, 8))
        point("below_min_votes", U, [5, U, U, U])
        point("cloud_label_12", 12, [1, 1, U, U])
        point("cloud_label_upper_bytes", 0xFFFFFF05, [U, 1, U, 1])
        point("overruled", 0, [10, U, 10, U])
        point("occluded_view_does_not_vote", 0, [10, 10, U, U], depth=(1, 500))
        point("seen_through_view_does_not_vote", 0, [10, U, U, 10], depth=(3, 3000))
        point("agreement", 11, [11, 11, 11, 11])
        point("nothing", U, [U, U, U, U])
        pts.append([0, 0, -1.0]); own.append(4); names.append("behind")
        cs = case([view(d, l) for d, l in zip(dep, lab)], labelled(pts, own), edge_guard=edge_guard)
        cs["names"] = names
        return cs
    return make


def saturated():
    """16 views, own_weight 15: a count reaches 31"""
    w, h = 22, 5
    labs = [np.full((h, w), U) for _ in range(16)]
    pts, own = [], []
    for j, (L0, l) in enumerate(((3, 3), (3, 8), (U, 2), (6, U), (0, 11), (200, 0))):
        x = 2 + 3 * j
        for lab in labs:
            lab[1:4, x - 1:x + 2] = l
        pts.append(at_pixel(x, 2, 1.0)); own.append(L0)
    labs[15][1:4, 13:16] = 5          # the fifth point: 15 views for 11, one for 5, 15 of its own for 0: a tie at 15, and the own label wins it
    return case([view(np.full((h, w), 1000), lab) for lab in labs], labelled(pts, own), own_weight=15)


def blocky(rng, w, h, block, p_unknown):
    g = rng.integers(0, 12, ((h + block - 1) // block, (w + block - 1) // block))
    g[rng.random(g.shape) < p_unknown] = U
    return np.kron(g, np.ones((block, block), np.int64))[:h, :w]


def posed(w, h, seed, v, n_max=None, half=False, block=6, noise_p=0.05, **params):
    """a cloud and v views a little way off whose label images mostly agree with each other and half of the time with the cloud; with `half` the last view has
    half the size and a camera to match"""
    def make():
        rng = np.random.default_rng(seed)
        camera = (w / 2 - 0.3, h / 2 + 0.2, 0.9 * w, 0.9 * w, 1000.0)
        d0 = carve_ref.scene_depth(w, h, seed)
        truth = blocky(rng, w, h, block, 0.1)
        yy, xx = np.mgrid[0:h, 0:w]
        m = d0 > 0
        xyz = carve_ref.backproject(d0, camera)
        own = truth[m].copy()
        flip = rng.random(len(own))
        own[flip < 0.25] = rng.integers(0, 12, int((flip < 0.25).sum()))
        own[(flip >= 0.25) & (flip < 0.4)] = rng.choice([U, 12, 4096, 0xFFFFFF00], int(((flip >= 0.25) & (flip < 0.4)).sum()))
        if n_max is not None and len(xyz) > n_max:
            pick = np.sort(rng.choice(len(xyz), n_max, replace=False))
            xyz, own = xyz[pick], own[pick]
        views, Ts = [], []
        for k in range(v):
            lab = truth.copy()
            noise = rng.random((h, w))
            lab[noise < noise_p] = rng.integers(0, 12, int((noise < noise_p).sum()))
            lab[noise > 1 - 0.6 * noise_p] = U
            d = d0.copy()
            d[rng.random((h, w)) < 0.02] = 0
            if half and k == v - 1:
                views.append(view(d[::2, ::2], lab[::2, ::2], (camera[0] / 2, camera[1] / 2, camera[2] / 2, camera[3] / 2, camera[4])))
            else:
                views.append(view(d, lab, camera))
            Ts.append(carve_ref.pose(rng, 0.002, 0.004))
        return case(views, labelled(xyz, own, seed), T_views=Ts, T_cloud=carve_ref.pose(rng, 0.002, 0.004), **params)
    return make


def cases():
    """name -> a function that makes the case (a dict: views, T_views, pts, T_cloud, params)"""
    c = {}
    c["constructed"] = constructed(1)
    c["constructed_no_guard"] = constructed(0)
    c["saturated"] = saturated
    c["posed_70x9"] = posed(70, 9, 3, 3)
    c["posed_70x9_r0_votes1"] = posed(70, 9, 4, 2, radius=0, min_votes=1, own_weight=0)
    c["posed_160x120"] = posed(160, 120, 5, 5, n_max=3000, half=True)
    c["posed_160x120_r3"] = posed(160, 120, 6, 4, n_max=2000, block=24, noise_p=0.002, radius=3, min_votes=3, own_weight=2, tol_abs=0.02, tol_rel_ppm=5000)
    return c


def run_case(cs):
    return relabel(cs["views"], cs["T_views"], cs["pts"], cs["T_cloud"], **cs["params"])
