"""The describe stage of the ORB front end (orientation moments, angle, sin / cos, keypoint record, position, steered BRIEF) restated in
vectorised numpy for PLANTED keypoints, and the case list the CPU and GPU tests share.  The moments are explicit sums over the disc of pyref.umax_table(); the
angle is pyref.fast_atan2 and the sin / cos pair pyref.contract_sincos, called per distinct value; the steered BRIEF does np.float32 products and sums in the
order of pyref.orb_descriptor (px*b + py*a, px*a - py*b, round half to even).  tests/test_orb_describe_ref.py holds it to oracle/orb.c and pyref on the CPU
and asserts that the case list still reaches the edges it was written for; tests/test_gpu_orb_describe.py holds ssm_debug_orb_describe to it, byte for byte."""
import collections
import math
import os
import re
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import pyref                  # noqa: E402

f32 = np.float32
EDGE, HALF, REACH = 19, 15, 18
MAX_R2 = 342                  # SSM_BRIEF_MAX_R2: sqrt(342) = 18.493 rounds to 18
FIELDS = ("m10", "m01", "angle", "sn", "cs", "x", "y", "size", "response", "octave", "class_id", "desc", "pos3d")
UMAX = pyref.umax_table()

Level = collections.namedtuple("Level", "w h stride img_off sel_cap sf")


def geometry(w, h, nlevels, nfeatures, scale=1.2):
    """the levels of a configuration: size, row stride (rows padded to 16 bytes), offset in one frame's pyramid buffer, slots (features + 3), scale factor"""
    sf, inv, feat = pyref.level_params(nfeatures, scale, nlevels)
    out, off = [], 0
    for l in range(nlevels):
        lw, lh = pyref.cv_round(float(f32(f32(w) * inv[l]))), pyref.cv_round(float(f32(f32(h) * inv[l])))
        stride = (lw + 15) & ~15
        out.append(Level(lw, lh, stride, off, feat[l] + 3, sf[l]))
        off += stride * lh
    return out


def pyramid_bytes(geom):
    return geom[-1].img_off + geom[-1].stride * geom[-1].h


def level_views(buf, geom):
    """one frame's buffer (ssm_debug_pyramid / ssm_debug_orb_blur) -> per level the (h, stride) array"""
    return [buf[L.img_off:L.img_off + L.stride * L.h].reshape(L.h, L.stride) for L in geom]


def default_pattern():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(HERE, "..", "oracle", "orb_pattern.inc")).read(), flags=re.S)
    return np.array([int(x) for x in re.findall(r"-?\d+", txt)], np.int8).reshape(256, 4)


def pack(x, y, score=0):
    return (np.asarray(x, np.uint32) | (np.asarray(y, np.uint32) << np.uint32(12)) | (np.asarray(score, np.uint32) << np.uint32(24))).astype(np.uint32)


# ---------------------------------------------------------------- the restatement
def disc_moments(img, xs, ys):
    """(m10, m01) over the radius-15 disc: row v holds u = -umax[|v|] .. umax[|v|]"""
    xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    r = np.arange(-HALF, HALF + 1)
    mask = np.abs(r)[None, :] <= np.array([UMAX[abs(v)] for v in r])[:, None]                # [v, u]
    p = img[ys[:, None, None] + r[None, :, None], xs[:, None, None] + r[None, None, :]].astype(np.int64) * mask
    return (p * r[None, None, :]).sum((1, 2)).astype(np.int32), (p * r[None, :, None]).sum((1, 2)).astype(np.int32)


_atan, _sincos = {}, {}


def angles(m10, m01):
    out = np.zeros(len(m10), f32)
    for i, k in enumerate(zip(m01.tolist(), m10.tolist())):
        if k not in _atan:
            _atan[k] = pyref.fast_atan2(f32(k[0]), f32(k[1]))
        out[i] = _atan[k]
    return out


def sincos(angle_deg):
    sn, cs = np.zeros(len(angle_deg), f32), np.zeros(len(angle_deg), f32)
    for i, a in enumerate(angle_deg):
        k = a.tobytes()
        if k not in _sincos:
            _sincos[k] = pyref.contract_sincos(f32(f32(a) * f32(math.pi / float(f32(180.0)))))
        sn[i], cs[i] = _sincos[k]
    return sn, cs


def steer(pattern, sn, cs):
    """the rounded steered coordinates (yy, xx), each (keypoints, 256, 2): point e of comparison i"""
    p = np.asarray(pattern, np.int8).reshape(256, 2, 2).astype(f32)
    px, py = p[None, :, :, 0], p[None, :, :, 1]
    b, a = sn.astype(f32)[:, None, None], cs.astype(f32)[:, None, None]
    yy = np.rint((px * b).astype(f32) + (py * a).astype(f32)).astype(np.int64)
    xx = np.rint((px * a).astype(f32) - (py * b).astype(f32)).astype(np.int64)
    return yy, xx


def brief(blur, xs, ys, sn, cs, pattern):
    yy, xx = steer(pattern, sn, cs)
    t = blur[np.asarray(ys, np.int64)[:, None, None] + yy, np.asarray(xs, np.int64)[:, None, None] + xx]
    return np.packbits(t[:, :, 0] < t[:, :, 1], axis=1, bitorder="little")


def describe(levels, blurs, geom, plants, pattern, cam, depth=None, moments=None):
    """One frame.  levels / blurs: per level the image and the blurred image; plants: per level an (k, 3) array of (x, y, score); moments: None or the planted
    (m10, m01) of all keypoints in output order.  Returns the fields of FIELDS plus "level", "px", "py" (where each keypoint was planted), in output order."""
    out = {k: [] for k in ("m10", "m01", "level", "px", "py", "desc")}
    for l, (L, pl) in enumerate(zip(geom, plants)):
        pl = np.asarray(pl, np.int64).reshape(-1, 3)
        m10, m01 = disc_moments(levels[l], pl[:, 0], pl[:, 1])
        out["m10"].append(m10); out["m01"].append(m01); out["level"].append(np.full(len(pl), l, np.int32)); out["px"].append(pl[:, 0]); out["py"].append(pl[:, 1])
    cat = {k: np.concatenate(v) if v else np.zeros(0, np.int64) for k, v in out.items() if k != "desc"}
    n = len(cat["level"])
    if moments is not None:
        moments = np.asarray(moments, np.int32).reshape(n, 2)
        cat["m10"], cat["m01"] = moments[:, 0].copy(), moments[:, 1].copy()
    cat["angle"] = angles(cat["m10"], cat["m01"])
    cat["sn"], cat["cs"] = sincos(cat["angle"])
    desc = np.zeros((n, 32), np.uint8)
    for l in range(len(geom)):
        s = cat["level"] == l
        if s.any():
            desc[s] = brief(blurs[l], cat["px"][s], cat["py"][s], cat["sn"][s], cat["cs"][s], pattern)
    cat["desc"] = desc
    sf = np.array([L.sf for L in geom], f32)[cat["level"]] if n else np.zeros(0, f32)
    x, y = cat["px"].astype(f32), cat["py"].astype(f32)
    up = cat["level"] != 0
    x = np.where(up, (x * sf).astype(f32), x); y = np.where(up, (y * sf).astype(f32), y)
    cat["x"], cat["y"], cat["size"] = x, y, (f32(31) * sf).astype(f32)
    scores = np.concatenate([np.asarray(pl, np.int64).reshape(-1, 3)[:, 2] for pl in plants]) if n else np.zeros(0, np.int64)
    cat["response"] = scores.astype(f32); cat["octave"] = cat["level"].astype(np.int32); cat["class_id"] = np.full(n, -1, np.int32)
    pos = np.zeros((n, 3), f32)
    if depth is not None and n:
        cx, cy, fx, fy, scale = cam
        u, v = x.astype(np.int64), y.astype(np.int64)                        # float -> int truncation
        d = depth[v, u]
        z = (d.astype(np.float64) / scale).astype(f32)
        px = ((u.astype(np.float64) - cx) * z.astype(np.float64) / fx).astype(f32); py = ((v.astype(np.float64) - cy) * z.astype(np.float64) / fy).astype(f32)
        pos = np.where((d != 0)[:, None], np.stack([px, py, z], 1), f32(0)).astype(f32)
    cat["pos3d"] = pos
    return cat


def first_difference(got, ref, n):
    """None, or (field, index of the first keypoint that differs in it, got, expected), bit for bit (a float field compares as its bytes)"""
    for k in FIELDS if n else ():
        g, r = np.ascontiguousarray(got[k][:n]), np.ascontiguousarray(ref[k][:n])
        assert g.dtype == r.dtype and g.shape == r.shape, (k, g.dtype, r.dtype, g.shape, r.shape)
        gb, rb = g.view(np.uint8).reshape(n, -1), r.view(np.uint8).reshape(n, -1)
        bad = np.flatnonzero((gb != rb).any(1))
        if len(bad):
            return k, int(bad[0]), g[bad[0]].tolist(), r[bad[0]].tolist()
    return None


# ---------------------------------------------------------------- the case list
# (w, h, levels) of tests/test_gpu_orb_describe.py: the headline shape, KITTI's (w % 4 == 1), a stride with a half-filled 32-column unit, one tiny level
GEOMS = [(640, 480, 8), (1241, 376, 8), (644, 484, 8), (176, 88, 1)]
NFEAT = 200                   # orb_features there: full levels stay cheap


def noise_image(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def window_corners(w, h):
    return [(EDGE, EDGE), (w - EDGE - 1, EDGE), (EDGE, h - EDGE - 1), (w - EDGE - 1, h - EDGE - 1)]


def border_points(w, h):
    """the legal extremes of a level: the window's corners, then every residue of x mod 16 at the left and the right border on the first and the last
    row, and the same transposed"""
    pts = window_corners(w, h)
    lo, hi = list(range(EDGE, EDGE + 16)), None
    for n_, other, flip in ((w, h, False), (h, w, True)):
        hi = list(range(n_ - EDGE - 16, n_ - EDGE))
        for a in lo + hi:
            for b in (EDGE, other - EDGE - 1):
                pts.append((b, a) if flip else (a, b))
    seen, out = set(), []
    for p in pts:
        if p not in seen:
            seen.add(p); out.append(p)
    return out


def max_moment():
    """the largest |m10| (= the largest |m01|: the disc is symmetric) an image can give: a half disc of 255"""
    return 255 * sum(sum(range(1, UMAX[abs(v)] + 1)) for v in range(-HALF, HALF + 1))


def moment_region(m10, m01):
    """where atan2(m01, m10) lies: "origin", an axis "+x" "+y" "-x" "-y", a diagonal "d0" .. "d3" (45, 135, 225, 315 degrees), or the open octant "o0" .. "o7" """
    if m10 == 0 and m01 == 0:
        return "origin"
    if m01 == 0:
        return "+x" if m10 > 0 else "-x"
    if m10 == 0:
        return "+y" if m01 > 0 else "-y"
    if abs(m10) == abs(m01):
        return "d%d" % ((0 if m01 > 0 else 3) if m10 > 0 else (1 if m01 > 0 else 2))
    return "o%d" % (int(math.floor(math.degrees(math.atan2(m01, m10)) % 360.0 / 45.0)))


REGIONS = ["origin", "+x", "+y", "-x", "-y", "d0", "d1", "d2", "d3"] + ["o%d" % i for i in range(8)]


def moment_cases(n_random=3000, seed=5):
    """(m10, m01) pairs for the planted sweep of fast_atan2 / contract_sincos: every octant and every boundary between them, the pairs next to a boundary,
    unit vectors, the origin, the largest magnitudes an image can give, the pair whose angle rounds to 360.0f, and random ones"""
    M = max_moment()
    out = [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)]
    for k in (1, 2, 3, 7, 1000, 65537, M):
        for sx in (1, -1):
            for sy in (1, -1):
                out += [(sx * k, sy * k), (sx * k, sy * (k + 1)), (sx * k, sy * (k - 1)), (sx * (k + 1), sy * k), (sx * (k - 1), sy * k)]
        out += [(k, 0), (-k, 0), (0, k), (0, -k)]
    out += [(M, M), (M, -M), (-M, M), (-M, -M), (M, 1), (M, -1), (-M, 1), (-M, -1), (1, M), (-1, M), (1, -M), (-1, -M)]
    out += [(10_000_000, -1), (1 << 30, -1), (10_000_000, 1), (-10_000_000, -1), (-10_000_000, 1)]          # 360 - tiny rounds to 360.0f; its neighbours
    for deg in range(0, 360, 5):                                                                            # an even sweep (the steering of the BRIEF tests)
        out.append((int(round(1e5 * math.cos(math.radians(deg + 0.5)))), int(round(1e5 * math.sin(math.radians(deg + 0.5))))))
    rng = np.random.default_rng(seed)
    r = rng.integers(-M, M + 1, (n_random, 2))
    small = rng.integers(-40, 41, (n_random // 6, 2))
    return np.array(out + r.tolist() + small.tolist(), np.int32)


def ring_points():
    return [(x, y) for x in range(-REACH, REACH + 1) for y in range(-REACH, REACH + 1) if 300 < x * x + y * y <= MAX_R2]


def ring_pattern(seed=11):
    """256 comparisons between points of the ring 300 < x^2 + y^2 <= 342: every point of the ring occurs, (+-13, +-13) and (+-18, 0), (0, +-18) among them"""
    pts = ring_points()
    rng = np.random.default_rng(seed)
    a = [pts[i % len(pts)] for i in range(256)]
    b = []
    for i in range(256):
        j = int(rng.integers(len(pts)))
        while pts[j] == a[i]:
            j = int(rng.integers(len(pts)))
        b.append(pts[j])
    return np.array([[p[0], p[1], q[0], q[1]] for p, q in zip(a, b)], np.int8)


def random_pattern(seed=12):
    """256 comparisons between random points inside the bound"""
    rng = np.random.default_rng(seed)
    pts = [(x, y) for x in range(-REACH, REACH + 1) for y in range(-REACH, REACH + 1) if x * x + y * y <= MAX_R2]
    idx = rng.integers(0, len(pts), (256, 2))
    idx[:, 1] = np.where(idx[:, 0] == idx[:, 1], (idx[:, 1] + 1) % len(pts), idx[:, 1])
    return np.array([[*pts[i], *pts[j]] for i, j in idx], np.int8)


def ring_moments():
    """planted moments whose angles steer the ring pattern: every 2.5 degrees, the axes and the diagonals included"""
    out = []
    for i in range(144):
        t = math.radians(2.5 * i)
        out.append((int(round(1e5 * math.cos(t))), int(round(1e5 * math.sin(t)))))
    return np.array(out, np.int32)


def slot_shapes(geom):
    """name -> per-level counts, for one frame: the shapes the slot bookkeeping is walked through"""
    nl = len(geom)
    caps = [L.sel_cap for L in geom]
    shapes = {"none": [0] * nl, "last_only": [0] * (nl - 1) + [1], "full": list(caps), "full_minus_one": [c - 1 for c in caps]}
    shapes["alternating"] = [c if l % 2 == 0 else l % 4 // 2 for l, c in enumerate(caps)]       # full, 0, full, 1, ...: a full level's last slots beside an empty and a 1-keypoint level
    if nl == 8:
        shapes["sparse"] = [1, 0, 3, 0, 0, 2, 0, 5]
    for total in (3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33):
        # spread over the levels so that level boundaries fall inside a group of 4 and of 8: counts 1, 2, 3, 1, 2, 3 ... until the total is used up
        cnt, left, l = [0] * nl, total, 0
        while left:
            k = min(left, 1 + l % 3, caps[l % nl] - cnt[l % nl])
            cnt[l % nl] += k; left -= k; l += 1
        shapes["total_%d" % total] = cnt
    return shapes
