"""A plain numpy restatement of UVDisparity::Process (reference src/uvdisparity.cpp:842-903) and of triangulate10D, correct3DPoints and setImageROI
(src/stereo.cpp:41-192), function by function, in float32 / float64 where the reference uses them and Python integers for Otsu.  It shares no code with
include/ssm/uvd_core.h: the tests compare the library with it.  OpenCV's calls are restated as DESIGN.md s.11 pins them.  Also the seeded scene generator."""
import math
import numpy as np

F32, F64 = np.float32, np.float64
TOO_LARGE, NO_LINE, SKIPPED = 1, 2, 4
PMATCH = np.dtype([("u1p", "f4"), ("v1p", "f4"), ("i1p", "i4"), ("u2p", "f4"), ("v2p", "f4"), ("i2p", "i4"), ("u1c", "f4"), ("v1c", "f4"),
                   ("i1c", "i4"), ("u2c", "f4"), ("v2c", "f4"), ("i2c", "i4"), ("dis_c", "i2"), ("dis_p", "i2")])
DEFAULT_PARAMS = dict(f=718.8560, cu=607.1928, cv=185.2157, base=0.532331858, roi_x=20.0, roi_y=5.0, roi_z=40.0,
                      min_intense=32, min_disparity_raw=64, min_area=40, inlier_tolerance=3)


def cv_round(x):
    """cvRound: round half to even"""
    return np.rint(x).astype(np.int64)


class Kalman:
    """KalmanFilter(2, 1, 0) of uvdisparity.cpp:35-47, whose second state is never observed: a scalar float32 filter"""

    def __init__(self):
        self.x, self.P = F32(0), F32(1)

    def update(self, z):
        self.P = F32(self.P + F32(5e-6))
        K = F32(self.P / F32(self.P + F32(0.001)))
        self.x = F32(self.x + F32(K * F32(F32(z) - self.x)))
        self.P = F32(F32(F32(1) - K) * self.P)


# ---------------------------------------------------------------- calVDisparity (uvdisparity.cpp:277-334)
def cal_v_disparity(disp):
    rows, cols = disp.shape
    max_dis = float(disp.max()) / 16
    v_cols = max(int(math.ceil(max_dis)), 0)
    v_int = np.zeros((rows, v_cols + 1), np.int64)             # one column more: the bin `id == v_cols`, a write past the row in the reference -- dropped
    for i in range(rows):
        d = disp[i][disp[i] > 0]
        dis = cv_round(d.astype(F32) / F32(16.0))
        np.add.at(v_int[i], np.clip(dis, 0, v_cols), 1)
    v_int = v_int[:, :v_cols]
    scale = F32(255 * 1.0) / F32(cols)
    return (v_int.astype(F32) * scale).astype(np.int64).astype(np.uint8), v_cols


# ---------------------------------------------------------------- Pitch_Classify (uvdisparity.cpp:368-528)
def gaussian_blur3(img):
    p = np.pad(img.astype(np.int64), 1, mode="reflect")       # reflect-101
    k = (1, 2, 1)
    s = sum(k[a] * k[b] * p[a:a + img.shape[0], b:b + img.shape[1]] for a in range(3) for b in range(3))
    return ((s + 8) >> 4).astype(np.uint8)


def erode3(img):
    p = np.pad(img, 1, mode="constant", constant_values=255)
    return np.min([p[a:a + img.shape[0], b:b + img.shape[1]] for a in range(3) for b in range(3)], axis=0).astype(np.uint8)


def otsu(img):
    hist = [int(x) for x in np.bincount(img.ravel(), minlength=256)]
    N, S = sum(hist), sum(i * h for i, h in enumerate(hist))
    best, best_num, best_den, n1, s1 = 0, 0, 1, 0, 0
    for t in range(256):
        n1 += hist[t]; s1 += t * hist[t]
        n2, s2 = N - n1, S - s1
        if n1 == 0 or n2 == 0:
            continue
        num, den = (s1 * n2 - s2 * n1) ** 2, n1 * n2
        if num * best_den > best_num * den:
            best, best_num, best_den = t, num, den
    return best


def point_list(bin_img):
    pts = []
    rows, cols = bin_img.shape
    for i in range(26, cols):
        for j in range(rows - 1, -1, -1):
            if bin_img[j, i] == 255:
                pts.append((i, j))
                k = j
                while k > max(j - 30, 0):
                    if bin_img[k, i] == 255:
                        pts.append((i, k))
                    k -= 1
                break
    return pts


def fit_line(pts):
    p = np.asarray(pts, F64)
    w = float(len(pts))
    x = y = x2 = y2 = xy = 0.0
    for px, py in p:
        x += px; y += py; x2 += px * px; y2 += py * py; xy += px * py
    x /= w; y /= w; x2 /= w; y2 /= w; xy /= w
    dx2, dy2, dxy = F32(x2 - x * x), F32(y2 - y * y), F32(xy - x * y)
    t = F32(F32(math.atan2(float(F32(2) * dxy), float(F32(dx2 - dy2)))) / F32(2))
    return np.array([F32(math.cos(float(t))), F32(math.sin(float(t))), F32(x), F32(y)], F32)


def line_to_ground(line, cv, f):
    """slope (float), V_C (double), theta (double) of uvdisparity.cpp:441-455"""
    a, b = F32(line[0]), F32(line[1])
    x0, y0 = int(cv_round(line[2])), int(cv_round(line[3]))
    with np.errstate(all="ignore"):
        slope = F32(b / a)
        V_C = float(F32(F32(y0) - F32(slope * F32(x0))))
        theta = math.atan((cv - V_C) / f)
    return slope, V_C, theta


def ground_distance(disp, slope, V_C):
    rows, cols = disp.shape
    v = np.repeat(np.arange(rows, dtype=F32)[:, None], cols, 1)
    d = disp.astype(F32) / F32(16.0)
    with np.errstate(all="ignore"):
        t = (v - (F32(slope) * d).astype(F32)).astype(F32)
        return (t.astype(F64) - V_C).astype(F32), d


def classify_ground(disp, left, slope, V_C):
    distance, d = ground_distance(disp, slope, V_C)
    ch9 = np.where(d > F32(8.0), np.where(distance > F32(-14.0), 0, left), 0)
    return ch9.astype(np.uint8)


# ---------------------------------------------------------------- triangulate10D, correct3DPoints, setImageROI (stereo.cpp:41-192)
def triangulate(disp, P):
    rows, cols = disp.shape
    d = disp.astype(F64)
    j = np.repeat(np.arange(cols, dtype=F64)[None, :], rows, 0)
    i = np.repeat(np.arange(rows, dtype=F64)[:, None], cols, 1)
    with np.errstate(all="ignore"):
        pw = P["base"] / (1.0 * d)
        px = ((j - P["cu"]) * pw) * 16.0
        py = ((i - P["cv"]) * pw) * 16.0
        pz = (P["f"] * pw) * 16.0
    missing = disp == disp.min()
    px[missing] = np.inf; py[missing] = np.inf; pz[missing] = np.inf
    with np.errstate(all="ignore"):
        return px.astype(F32), py.astype(F32), pz.astype(F32)


def roi_mask_of(disp, left, P, pitch):
    """-> (roi mask, the smallest distance of a decided comparison from its bound)"""
    xp, yp, zp = triangulate(disp, P)
    cos_p, sin_p = math.cos(pitch), math.sin(pitch)
    dr = cv_round(disp.astype(F32) / F32(16.0))
    with np.errstate(all="ignore"):
        y2 = (cos_p * yp.astype(F64) + sin_p * zp.astype(F64)).astype(F32)
        z2 = (cos_p * zp.astype(F64) - sin_p * yp.astype(F64)).astype(F32)
        outside = (xp.astype(F64) > P["roi_x"]) | (y2.astype(F64) > P["roi_y"]) | (z2.astype(F64) > P["roi_z"])
        valid = (dr > 0) & (dr < 100)
        margins = np.minimum(np.minimum(np.abs(xp.astype(F64) - P["roi_x"]), np.abs(y2.astype(F64) - P["roi_y"])), np.abs(z2.astype(F64) - P["roi_z"]))
    ch6 = np.where(valid & ~outside, left, 0).astype(np.uint8)
    m = margins[valid & np.isfinite(margins)]
    return ch6, (float(m.min()) if m.size else np.inf)


# ---------------------------------------------------------------- filterInOut (uvdisparity.cpp:68-190)
def filter_in_out(matches, flags, roi_mask, disp, P):
    """-> (matches with dis_c recorded, flags with bit 1 set where the match is erased)"""
    m, fl = matches.copy(), (flags & 1).astype(np.uint8)
    rows, cols = roi_mask.shape
    for i in range(len(m)):
        uc, vc = int(m["u1c"][i]), int(m["v1c"][i])
        inside = 0 <= uc < cols and 0 <= vc < rows
        keep = inside and roi_mask[vc, uc] > 0
        if keep and fl[i] == 0:
            d = float(max(F32(F32(uc) - m["u2c"][i]), F32(1.0)))
            xc = (uc - P["cu"]) * P["base"] / d
            keep = xc > -3000
        if keep:
            m["dis_c"][i] = disp[vc, uc]
        else:
            fl[i] |= 2
    return m, fl


# ---------------------------------------------------------------- calUDisparity, adjustUdisIntense (uvdisparity.cpp:195-274, 807-837)
def cal_u_disparity(disp, roi_mask, ground_mask):
    rows, cols = disp.shape
    u_rows = max(int(math.ceil(float(disp.max()) / 16)), 0) + 1
    u_int = np.zeros((u_rows, cols), np.int64)
    for i in range(rows):
        for j in range(cols):
            d = int(disp[i, j])
            if d > 0:
                dis = int(cv_round(F64(d // 16)))
                if roi_mask[i, j] > 0 and ground_mask[i, j] > 0 and dis > 0:
                    u_int[dis, j] += 1
    scale = F32(255 * 1.0) / F32(rows)
    return (u_int.astype(F32) * scale).astype(np.int64).astype(np.uint8)


def sigmoid(t, scale, rng):
    return rng * 1.0 / (1 + math.exp(t * scale))


def adjust_u(u_dis, scale=0.02, rng=32):
    out = u_dis.copy()
    for j in range(u_dis.shape[0]):
        rate = sigmoid(float(j), scale, rng)
        new = (u_dis[j].astype(F32) * F32(1.0)).astype(F64) * rate
        out[j] = np.minimum(cv_round(new), 255).astype(np.uint8)
    return out


# ---------------------------------------------------------------- findAllMasks, mergeMasks, verifyByInliers, segmentation
def flood_fill(img, seed_row, seed_col, lo, hi):
    """FIXED_RANGE | MASK_ONLY, 8-connected: the component of {lo <= p <= hi} around the seed"""
    rows, cols = img.shape
    mask = np.zeros((rows, cols), np.uint8)
    ok = (img.astype(np.int64) >= lo) & (img.astype(np.int64) <= hi)
    queue, head = [(seed_row, seed_col)], 0
    mask[seed_row, seed_col] = 255
    while head < len(queue):
        r, c = queue[head]; head += 1
        for rr in range(max(r - 1, 0), min(r + 2, rows)):
            for cc in range(max(c - 1, 0), min(c + 2, cols)):
                if not mask[rr, cc] and ok[rr, cc]:
                    mask[rr, cc] = 255; queue.append((rr, cc))
    return mask, len(queue)


def find_all_masks(matches, flags, u_dis, P):
    areas, masks = [], []
    for i in range(len(matches)):
        if flags[i] != 0:                     # the outliers that filterInOut kept
            continue
        u, d = int(matches["u1c"][i]), int(matches["dis_c"][i])
        if d > P["min_disparity_raw"]:
            dis = int(cv_round(F32(d) / F32(16.0)))
            utense = int(u_dis[dis, u])
            if utense > P["min_intense"]:
                low = math.floor(0.5 * utense) if 0.5 * utense > P["min_intense"] else abs(utense - P["min_intense"])
                up = 255 - utense
                mask, area = flood_fill(u_dis, dis, u, utense - low, utense + up)
                areas.append(area)
                if area > P["min_area"]:
                    masks.append(mask)
    return areas, masks


def merge_masks(masks):
    masks = [m.copy() for m in masks]
    a = 0
    while a < len(masks):
        b = a + 1
        while b < len(masks):
            if (masks[a] & masks[b]).any():
                masks[a] = masks[a] | masks[b]
                del masks[b]
            else:
                b += 1
        a += 1
    return masks


def verify_by_inliers(masks, matches, flags, tolerance):
    kept = []
    for mask in masks:
        n = 0
        for i in range(len(matches)):
            if flags[i] != 1:
                continue
            u = int(matches["u1c"][i]); dis = int(cv_round(F32(matches["dis_c"][i]) / F32(16.0)))
            if dis > 0 and mask[dis, u] != 0:
                n += 1
        if n < tolerance:
            kept.append(mask)
    return kept


def segmentation(disp, roi_mask, masks):
    moving = np.zeros(disp.shape, np.uint8)
    dis_real = (disp.astype(F32) / F32(16.0)).astype(F64)
    for mask in masks:
        for i in range(1, mask.shape[0]):
            for j in range(1, mask.shape[1]):
                if mask[i, j] != 0:
                    hit = (np.abs(dis_real[:, j] - i) < 1.5) & (roi_mask[:, j] > 0)
                    moving[hit, j] = 255
    return moving


# ---------------------------------------------------------------- Process
def process(kf1, kf2, left, disp, matches, flags, P, line=None, skip=False):
    """UVDisparity::Process on one frame -> dict of every stage.  line: use this fitted line (4 floats) for everything after fitLine, so that a last-bit
    difference of atan2 between two callers of libm cannot move a discrete outcome (the line itself is compared on its own)"""
    rows, cols = disp.shape
    zero = np.zeros((rows, cols), np.uint8)
    out = dict(status=0, moving=zero, roi=zero, ground=zero, matches=matches.copy(), flags=(flags & 1).astype(np.uint8), n_moving=0, pitch_filtered=kf1.x)
    if skip:
        out["status"] = SKIPPED
        return out
    v_dis, v_cols = cal_v_disparity(disp)
    out.update(v_dis=v_dis, v_cols=v_cols, u_rows=v_cols + 1)
    if int(disp.max()) > 255 * 16:
        out["status"] = TOO_LARGE
        return out
    if v_cols <= 26:
        out["status"] = NO_LINE
        return out
    blur = gaussian_blur3(v_dis); ero = erode3(blur); thr = otsu(ero)
    bin_img = np.where(ero > thr, 255, 0).astype(np.uint8)
    pts = point_list(bin_img)
    out.update(blur=blur, erode=ero, otsu=thr, bin=bin_img, pts=pts)
    if len(pts) < 2:
        out["status"] = NO_LINE
        return out
    own_line = fit_line(pts)
    out["line"] = own_line
    slope, V_C, theta = line_to_ground(own_line if line is None else np.asarray(line, F32), P["cv"], P["f"])
    z = F32(theta)
    kf1.update(z); kf2.update(z)
    out.update(slope=slope, v_c=V_C, pitch_measured=z, pitch_filtered=kf1.x)
    ground = classify_ground(disp, left, slope, V_C)
    distance, d = ground_distance(disp, slope, V_C)
    gm = np.abs(distance[d > F32(8.0)].astype(F64) + 14.0)
    roi, roi_margin = roi_mask_of(disp, left, P, float(kf1.x))
    out.update(ground=ground, roi=roi, ground_margin=float(gm.min()) if gm.size else np.inf, roi_margin=roi_margin)
    m, fl = filter_in_out(matches, flags, roi, disp, P)
    u_raw = cal_u_disparity(disp, roi, ground); u_adj = adjust_u(u_raw)
    areas, found = find_all_masks(m, fl, u_adj, P)
    merged = merge_masks(found) if found else []
    kept = verify_by_inliers(merged, m, fl, P["inlier_tolerance"]) if found else []
    moving = segmentation(disp, roi, kept)
    uni = np.zeros(u_adj.shape, np.uint8)
    for k in kept:
        uni |= k
    out.update(matches=m, flags=fl, u_raw=u_raw, u_adj=u_adj, areas=areas, found=found, merged=merged, kept=kept, union=uni, moving=moving,
               n_moving=int((moving == 255).sum()))
    return out


# ---------------------------------------------------------------- scenes
SCENE_PARAMS = dict(DEFAULT_PARAMS, f=100.0, cu=80.3, cv=40.0, base=1.0, roi_x=20.0, roi_y=5.0, roi_z=40.0)


def make_scene(seed, w=160, h=96, slope=1.0, v_h=40, boxes=((56, 48, 30, 40),), outliers_on=(0,), n_out=3, inliers_on=(), n_in=3, n_ground_inliers=6,
               noise=True, holes=6, zero_pixels=40, exact_max=False, all_invalid=False, too_large=False, border_matches=False, cu=None):
    """A ground plane d(v) = slope (v - v_h) with rectangular obstacles (first column, width, top row, disparity) standing on it, invalid holes (-16), +-1/16
    noise, a left image with some zero pixels, and a pmatch list: n_out outliers on each box of outliers_on, n_in inliers on each box of inliers_on, inliers on
    the ground.  -> (left, disp, matches, inlier flags)"""
    rng = np.random.RandomState(seed)
    rows = np.arange(h)
    ground = np.where(rows > v_h, np.round(16.0 * slope * (rows - v_h)), -16).astype(np.int64)
    disp = np.repeat(ground[:, None], w, 1)
    placed = []
    for (x0, bw, top, d) in boxes:
        bottom = min(int(round(v_h + d / slope)), h - 1)          # the row where the ground has the box's disparity
        disp[top:bottom + 1, x0:x0 + bw] = 16 * d
        placed.append((x0, bw, top, bottom, d))
    if noise:
        disp = np.where(disp > 0, disp + rng.randint(-1, 2, disp.shape), disp)
    if exact_max:
        disp = np.minimum(disp, 16 * (int(disp.max()) // 16))
    for _ in range(holes):
        y, x = rng.randint(0, h - 4), rng.randint(0, w - 6)
        disp[y:y + 3, x:x + 5] = -16
    if all_invalid:
        disp[:] = -16
    if too_large:
        disp[h // 2, w // 2] = 256 * 16 + 5
    left = rng.randint(1, 256, (h, w)).astype(np.uint8)
    left.ravel()[rng.choice(w * h, zero_pixels, replace=False)] = 0
    disp = disp.astype(np.int16)
    pts = []
    for b in outliers_on:
        x0, bw, top, bottom, d = placed[b]
        pts += [(x0 + 2 + rng.randint(0, bw - 4), top + 1 + rng.randint(0, 20), 0) for _ in range(n_out)]
    for b in inliers_on:
        x0, bw, top, bottom, d = placed[b]
        pts += [(x0 + 2 + rng.randint(0, bw - 4), top + 1 + rng.randint(0, 20), 1) for _ in range(n_in)]
    for _ in range(n_ground_inliers):
        pts.append((rng.randint(0, w), rng.randint(min(v_h + 30, h - 1), h), 1))
    if border_matches:
        pts += [(0, 0, 0), (w - 1, h - 1, 0), (0, h - 1, 1), (w - 1, 0, 1), (w - 1, h // 2, 0), (0, h // 2, 0)]
    m = np.zeros(len(pts), PMATCH); fl = np.zeros(len(pts), np.uint8)
    for i, (u, v, inl) in enumerate(pts):
        d = max(int(disp[v, u]), 16) / 16.0
        m["u1c"][i], m["v1c"][i], m["u2c"][i], m["v2c"][i] = u, v, u - d, v
        m["u1p"][i], m["v1p"][i], m["u2p"][i], m["v2p"][i] = u + 1, v, u + 1 - d, v
        m["i1c"][i] = m["i2c"][i] = m["i1p"][i] = m["i2p"][i] = i
        fl[i] = inl
    return left, disp, m, fl


def scene_params(w=160, h=96, **kw):
    return dict(SCENE_PARAMS, **kw)


# the scenes of the tests' condition list: name -> (make_scene keywords, parameter overrides)
SCENES = {
    "moving": (dict(seed=1), {}),
    "verified_away": (dict(seed=2, inliers_on=(0,), n_in=4), {}),
    "merge": (dict(seed=3, boxes=((20, 40, 30, 40), (100, 40, 40, 30)), outliers_on=(0, 0, 1), n_out=2), {}),
    "exact_max": (dict(seed=4, exact_max=True, boxes=((56, 48, 30, 37),)), {}),
    "no_line": (dict(seed=5, slope=0.4, boxes=((56, 48, 30, 12),)), {}),
    "all_invalid": (dict(seed=6, all_invalid=True), {}),
    "too_large": (dict(seed=7, too_large=True), {}),
}


def build_scene(name, **over):
    kw, pk = SCENES[name]
    kw = dict(kw, **over)
    left, disp, m, fl = make_scene(**kw)
    return left, disp, m, fl, scene_params(**pk)
