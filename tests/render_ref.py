"""Map rendering restated from DESIGN.md s.17 in numpy float64 and Python integers, and the case list the CPU and GPU tests share.  Written from the section, not
from include/ssm/render_core.h: the relative pose by the rigid inverse in the section's operation order (tests/carve_ref.py has it), one vectorised float64 pass
up to the pixel, then plain Python integers per point and per pixel.  `render` also hands out what every point's splat was (centre, half width, zq), so that
tests/test_render.py can assert that the case list still hits the boundaries it was written for."""
import json
import os
import numpy as np
import carve_ref as CR

POINT_DTYPE = CR.POINT_DTYPE
EYE = CR.EYE
F = CR.F
DEFAULTS = dict(point_size=0.0, max_radius=3, z_min=0.1, z_max=1.0e9, tol_abs=0.05, tol_rel_ppm=20000)
INFO_FIELDS = ("n_in", "n_visible", "n_covered")
COMPARE_FIELDS = ("unrendered", "no_depth", "in_front", "behind", "agree", "label_agree", "label_disagree", "label_unknown", "n_pixels")
UNRENDERED, NO_DEPTH, IN_FRONT, BEHIND, AGREE = range(5)
EMPTY = 2 ** 64 - 1
PALETTE = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "palette.json")))["palette_bgr"]


def cloud(xyz, seed=1):
    """points with every byte set; the labels' low bytes are classes 0..11, 255 and a few others, under random upper bytes"""
    p = CR.cloud(xyz, seed)
    rng = np.random.default_rng(seed + 1000)
    low = rng.choice(np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 255, 255, 44], np.uint32), len(p))
    p["label"] = low + 256 * rng.integers(0, 2 ** 24, len(p)).astype(np.uint32)
    return p


def render(w, h, camera, T_view, clouds, T_clouds, **params):
    """-> dict(depth, bgr, label, index, keys, info, splats): splats[i] is None for an invisible point, else dict(px, py, s, zq) -- the footprint may still be empty"""
    P = dict(DEFAULTS, **params)
    cx, cy, fx, fy, scale = (float(v) for v in camera)
    R = int(P["max_radius"])
    keys = [EMPTY] * (w * h)
    splats = []
    n_visible = 0
    first = 0
    half = (0.5 * fx) * float(P["point_size"])
    for pts, Tc in zip(clouds, T_clouds):
        M = CR.rel_pose(T_view, Tc)
        x, y, z = (pts[f].astype(np.float64) for f in "xyz")
        with np.errstate(all="ignore"):
            q = [M[i, 0] * x + M[i, 1] * y + M[i, 2] * z + M[i, 3] for i in range(3)]
            ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & np.isfinite(q[0]) & np.isfinite(q[1]) & np.isfinite(q[2])
            ok &= ~(q[2] < float(P["z_min"])) & ~(q[2] > float(P["z_max"]))
            u = fx * (q[0] / q[2]) + cx
            v = fy * (q[1] / q[2]) + cy
            px = np.floor(u + 0.5)
            py = np.floor(v + 0.5)
            ok &= (px >= -R) & (px <= w - 1 + R) & (py >= -R) & (py <= h - 1 + R)          # (false for NaN)
            zs = q[2] * scale
        for i in range(len(pts)):
            splats.append(None)
            if not ok[i] or not zs[i] < 65537.0:
                continue
            zq = round(float(zs[i]))          # half-even, as llrint
            if zq < 1 or zq > 65535:
                continue
            s = 0
            if float(P["point_size"]) > 0:
                t = half / float(q[2][i])
                s = R if t >= R else int(np.floor(t)) if t >= 1 else 0
            ix, iy = int(px[i]), int(py[i])
            splats[-1] = dict(px=ix, py=iy, s=s, zq=zq, qz=float(q[2][i]))
            key = (zq << 32) | (first + i)
            hit = False
            for yy in range(max(iy - s, 0), min(iy + s, h - 1) + 1):
                for xx in range(max(ix - s, 0), min(ix + s, w - 1) + 1):
                    hit = True
                    if key < keys[yy * w + xx]:
                        keys[yy * w + xx] = key
            n_visible += hit
        first += len(pts)
    allp = np.concatenate(list(clouds)) if len(clouds) else np.zeros(0, POINT_DTYPE)
    depth = np.zeros(w * h, np.uint16); bgr = np.zeros((w * h, 3), np.uint8); label = np.full(w * h, 255, np.uint8); index = np.full(w * h, -1, np.int32)
    for p, key in enumerate(keys):
        if key == EMPTY:
            continue
        i = key & 0xFFFFFFFF
        depth[p] = key >> 32; index[p] = i; label[p] = int(allp["label"][i]) & 255
        bgr[p] = (allp["b"][i], allp["g"][i], allp["r"][i])
    info = dict(n_in=first, n_visible=int(n_visible), n_covered=int((depth > 0).sum()))
    return dict(depth=depth.reshape(h, w), bgr=bgr.reshape(h, w, 3), label=label.reshape(h, w), index=index.reshape(h, w),
                keys=np.array(keys, np.uint64).reshape(h, w), info=info, splats=splats)


def label_of_bgr(sem):
    lab = np.full(sem.shape[:2], 255, np.uint8)
    for l, c in enumerate(PALETTE):
        lab[(sem == np.array(c, np.uint8)).all(-1)] = l
    return lab


def compare(rdepth, rlabel, depth, sem, scale, **params):
    """-> (counts, class image, per-pixel tolerance)"""
    P = dict(DEFAULTS, **params)
    tol_abs = round(float(P["tol_abs"]) * float(scale))
    lf = label_of_bgr(sem)
    h, w = rdepth.shape
    cls = np.zeros((h, w), np.uint8); tol = np.zeros((h, w), np.int64)
    c = dict.fromkeys(COMPARE_FIELDS, 0)
    c["n_pixels"] = w * h
    for y in range(h):
        for x in range(w):
            zr, d, lr, l = int(rdepth[y, x]), int(depth[y, x]), int(rlabel[y, x]), int(lf[y, x])
            if zr == 0:
                k = UNRENDERED
            elif d == 0:
                k = NO_DEPTH
            else:
                t = tol_abs + (d * int(P["tol_rel_ppm"])) // 1000000
                tol[y, x] = t
                k = IN_FRONT if zr + t < d else BEHIND if zr > d + t else AGREE
                if k == AGREE:
                    c["label_agree" if lr == l and lr != 255 else "label_disagree" if lr != 255 and l != 255 else "label_unknown"] += 1
            cls[y, x] = k
            c[COMPARE_FIELDS[k]] += 1
    return c, cls, tol


# ------------------------------------------------------------------ the case list
def case(w, h, clouds, T_clouds=None, camera=None, T_view=EYE, frame=None, seed=1, **params):
    clouds = [c if isinstance(c, np.ndarray) and c.dtype == POINT_DTYPE else cloud(c, seed + k) for k, c in enumerate(clouds)]
    T_clouds = [EYE] * len(clouds) if T_clouds is None else T_clouds
    return dict(w=w, h=h, camera=camera or CR.cam0(), T_view=np.asarray(T_view, np.float64), clouds=clouds, T_clouds=[np.asarray(T, np.float64) for T in T_clouds],
                params=params, frame=frame, seed=seed)


at = CR.at_pixel


def two_depths():
    return case(9, 7, [[at(4, 3, 2.0), at(4, 3, 1.0), at(4, 3, 3.0), at(2, 2, 1.5)]])


def equal_zq(rev):
    def make():
        pts = cloud([at(4, 3, 1.0), at(4, 3, 1.0002), at(4, 3, 0.9998), at(6, 1, 2.0), at(6, 1, 2.0)], 5)          # all three round to 1000
        return case(9, 7, [pts[::-1].copy() if rev else pts])
    return make


def zq_limits():
    """scale 1: zq = llrint(z) -- 0.5 -> 0 (out), 1 -> 1, 1.5 -> 2, 65535, 65535.25 -> 65535, 65535.5 -> 65536 (out), 65536 (out), 70000 (out)"""
    zs = [0.5, 1.0, 1.5, 65535.0, 65535.25, 65535.5, 65536.0, 70000.0, 0.25]
    return case(67, 5, [[at(3 + 7 * i, 2, z) for i, z in enumerate(zs)]], camera=CR.cam0(1.0), z_min=0.0)


def z_range():
    one, two = np.float32(1.0), np.float32(2.0)
    zs = [one, np.nextafter(one, np.float32(0)), two, np.nextafter(two, np.float32(3)), np.float32(1.5)]
    return case(67, 5, [[at(3 + 7 * i, 2, z) for i, z in enumerate(zs)]], z_min=1.0, z_max=2.0)


def degenerate():
    nan, inf, big = float("nan"), float("inf"), 1.0e30
    pts = [[0, 0, -1.0], [0.01, 0.01, -0.5], [0, 0, 0.0], [nan, 0, 1], [0, nan, 1], [0, 0, nan], [inf, 0, 1], [0, -inf, 1], [0, 0, inf], [0, 0, -inf], [big, 0, 1], [0, -big, 1],
           [0, 0, big], [big, big, big], [3.0e38, 3.0e38, 3.0e38], [1e-30, 1e-30, 1e-38], at(3, 3, 1.0)]
    return case(9, 7, [pts], point_size=0.1)


def borders(w, h):
    """fx = 64, point_size 1/16: t = 2 / z.  Centres 1 and 2 pixels outside each border and the corner at z = 1 (s = 2: reach in), 3 outside (beyond max_radius = 2),
    and 2 outside at z = 2 (s = 1: the footprint is empty)"""
    def make():
        pts = []
        for z in (1.0, 2.0):
            for o in (1, 2, 3):
                pts += [at(-o, 2, z), at(w - 1 + o, 2, z), at(w // 2, -o, z), at(w // 2, h - 1 + o, z), at(-o, -o, z), at(w - 1 + o, h - 1 + o, z)]
        pts += [at(0, 0, 1.0), at(w - 1, h - 1, 1.25)]
        return case(w, h, [pts], point_size=0.0625, max_radius=2)
    return make


def sizes(max_radius):
    """t = 32 point_size / z = 4 / z: z = 8 -> 0.5 (s 0), 4 -> 1, 2.5 -> 1.6 (s 1), 2 -> 2, 1 -> 4, 0.4 -> 10 (the cap)"""
    def make():
        zs = [8.0, 4.0, 2.5, 2.0, 1.0, 0.4]
        return case(67, 5, [[at(5 + 11 * i, 2, z) for i, z in enumerate(zs)]], point_size=0.125, max_radius=max_radius)
    return make


def posed(w, h, seed, m=1, n_max=None, **params):
    """the clouds of m key-frames a little way off each other seen from one more: nothing known by construction"""
    def make():
        rng = np.random.default_rng(seed)
        camera = (w / 2 - 0.3, h / 2 + 0.2, 0.9 * w, 0.9 * w, 1000.0)
        rot = 0.02 if h >= 100 else 0.004          # (a 5-pixel-high view loses everything under a larger rotation)
        clouds, Ts = [], []
        for k in range(m):
            xyz = CR.backproject(CR.scene_depth(w, h, seed + k), camera)
            if n_max is not None and len(xyz) > n_max:
                xyz = xyz[np.sort(rng.choice(len(xyz), n_max, replace=False))]
            clouds.append(cloud(xyz, seed + k)); Ts.append(CR.pose(rng, rot, 0.05))
        return case(w, h, clouds, Ts, camera=camera, T_view=CR.pose(rng, rot, 0.05), seed=seed, **params)
    return make


def three_clouds():
    rng = np.random.default_rng(9)
    a = [at(rng.integers(0, 9), rng.integers(0, 7), 1.0 + 0.25 * rng.integers(0, 4)) for _ in range(5)]
    b = [at(rng.integers(0, 9), rng.integers(0, 7), 1.0 + 0.25 * rng.integers(0, 4)) for _ in range(7)]
    return case(9, 7, [a, np.zeros(0, POINT_DTYPE), b], point_size=0.04)


def empty(m):
    return lambda: case(9, 7, [np.zeros(0, POINT_DTYPE)] * m)


def categories():
    """one point per pixel at 1 m (zq 1000), three columns left empty, under a frame whose depth walks through every class: with the default tolerance
    (50 + d / 50) d = 1071 agrees and 1072 is in front, d = 932 agrees and 931 is behind.  Labels: equal, different, unknown on either side"""
    w, h = 67, 5
    xy = [(x, y) for y in range(h) for x in range(w) if x < 64]
    pts = cloud([at(x, y, 1.0) for x, y in xy], 7)
    dep = np.full((h, w), 1000, np.uint16)
    dep[0, :8] = [1071, 1072, 1073, 1200, 932, 931, 930, 500]
    dep[1, :4] = 0
    dep[2, 60:] = [1071, 1072, 931, 932, 0, 1000, 1000]
    lab = np.full((h, w), 255, np.uint8)
    lr = (pts["label"] & 255).astype(np.uint8)
    for i, (x, y) in enumerate(xy):
        lab[y, x] = lr[i] if (x + y) % 3 == 0 and lr[i] < 12 else (int(lr[i]) + 1) % 12 if (x + y) % 3 == 1 else 255
    sem = np.zeros((h, w, 3), np.uint8)
    pal = np.array(PALETTE, np.uint8)
    sem[lab < 12] = pal[lab[lab < 12]]
    sem[lab == 255] = (1, 2, 3)
    return case(w, h, [pts], frame=(dep, sem))


def cases():
    """name -> a function that makes the case (a dict: w, h, camera, T_view, clouds, T_clouds, params, frame)"""
    c = {"two_depths": two_depths, "equal_zq": equal_zq(False), "equal_zq_reversed": equal_zq(True), "zq_limits": zq_limits, "z_range": z_range, "degenerate": degenerate,
         "borders_9x7": borders(9, 7), "borders_67x5": borders(67, 5), "sizes_r0": sizes(0), "sizes_r3": sizes(3), "sizes_r8": sizes(8),
         "posed_67x5": posed(67, 5, 3, point_size=0.01), "posed_9x7_m2": posed(9, 7, 4, m=2), "posed_160x120_m3": posed(160, 120, 5, m=3, n_max=700, point_size=0.06, max_radius=2),
         "three_clouds": three_clouds, "empty_m0": empty(0), "empty_m1": empty(1), "categories": categories}
    return c


def frame_of(cs, ref):
    """the frame a case is compared with: its own, or one made from the rendering -- the rendered depth moved by up to 150 units with holes, labels mostly the
    rendered ones"""
    if cs["frame"] is not None:
        return cs["frame"]
    rng = np.random.default_rng(cs["seed"] + 77)
    h, w = ref["depth"].shape
    d = ref["depth"].astype(np.int64) + rng.integers(-150, 151, (h, w))
    d[ref["depth"] == 0] = rng.integers(0, 3000, int((ref["depth"] == 0).sum()))
    d = np.clip(d, 0, 65535).astype(np.uint16)
    d[rng.random((h, w)) < 0.1] = 0
    lab = np.where(rng.random((h, w)) < 0.7, ref["label"], rng.integers(0, 13, (h, w))).astype(np.uint8)
    sem = np.full((h, w, 3), 9, np.uint8)
    pal = np.array(PALETTE, np.uint8)
    sem[lab < 12] = pal[lab[lab < 12]]
    return d, sem


def run_case(cs):
    ref = render(cs["w"], cs["h"], cs["camera"], cs["T_view"], cs["clouds"], cs["T_clouds"], **cs["params"])
    dep, sem = frame_of(cs, ref)
    ref["frame"] = (dep, sem)
    ref["counts"], ref["class"], ref["tol"] = compare(ref["depth"], ref["label"], dep, sem, cs["camera"][4], **cs["params"])
    return ref
