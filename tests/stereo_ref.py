"""Plain references for two parallel kernels of the stereo path, written from the algorithms' definitions and sharing no code with oracle/:
cv::goodFeaturesToTrack's corner selection on a min-eigenvalue map, cv::filterSpeckles, and cv::medianBlur 3x3 on int16.

The GFTT reference also reports the properties the edge-case inputs are built to have: the candidate count, the largest number of stronger
candidates within minDistance of one candidate (gftt_deps_kernel keeps 32 of them; more send the candidate to the window re-scan), and the number of
rounds of local decisions the parallel selection needs (the deps kernel decides round 1, GFTT_ROUNDS = 12 launches follow, the finish kernel loops
over the rest).  The case builders here are shared by tests/test_stereo_ref.py (reference == oracle, and each case's property) and
tests/test_gpu_stereo_edges.py (GPU == oracle)."""
import numpy as np

GFTT_DEPS = 32          # dependency list length of kernels_quad.hip
SPK_TW, SPK_TH = 64, 16  # speckle tile of sgbm_post.inc


# ------------------------------------------------------------------ goodFeaturesToTrack selection
def gftt_candidates(eig, quality):
    """interior pixels with v > float(max * quality) that equal the 3x3 maximum of the thresholded map (ties kept), strongest first:
    value descending, then raster index ascending.  Returns (ys, xs, values)."""
    eig = np.asarray(eig, np.float32); h, w = eig.shape
    if h < 3 or w < 3:
        return np.zeros(0, int), np.zeros(0, int), np.zeros(0, np.float32)
    thr = np.float32(max(float(eig.max()), 0.0) * quality)
    t = np.where(eig > thr, eig, np.float32(0))
    m = np.zeros((h - 2, w - 2), np.float32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            m = np.maximum(m, t[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx])
    core = eig[1:-1, 1:-1]
    ys, xs = np.nonzero((core > thr) & (core == m))
    ys = ys + 1; xs = xs + 1
    v = eig[ys, xs]
    order = np.lexsort((ys * w + xs, -v.astype(np.float64)))
    return ys[order], xs[order], v[order]


def _md2(min_distance):
    return float(np.float32(min_distance * min_distance))       # float(minDistance^2); squared integer offsets are exact in float


def gftt_select(eig, max_corners, quality, min_distance):
    """the greedy walk: a candidate is kept unless a kept one lies at float(dx)^2 + float(dy)^2 < float(md)^2; stop at max_corners (<= 0: all).
    Returns the (x, y) float32 list, like ssm_gftt."""
    ys, xs, _ = gftt_candidates(eig, quality)
    md2 = _md2(min_distance); cell = max(1, int(np.ceil(min_distance)))
    grid = {}
    out = []
    for y, x in zip(ys.tolist(), xs.tolist()):
        cy, cx = y // cell, x // cell
        ok = True
        for gy in (cy - 1, cy, cy + 1):
            for gx in (cx - 1, cx, cx + 1):
                for ky, kx in grid.get((gy, gx), ()):
                    if (x - kx) ** 2 + (y - ky) ** 2 < md2:
                        ok = False; break
                if not ok: break
            if not ok: break
        if ok:
            grid.setdefault((cy, cx), []).append((y, x)); out.append((x, y))
            if 0 < max_corners == len(out):
                break
    return np.array(out, np.float32).reshape(-1, 2)


def gftt_properties(eig, quality, min_distance):
    """candidates, max_stronger (most stronger candidates within minDistance of one candidate) and rounds: the synchronous round schedule of the
    parallel selection -- round 1 keeps every candidate without a stronger one within minDistance; in each later round an undecided candidate is
    rejected if a stronger neighbour was kept in an earlier round, and kept if all its stronger neighbours were decided (rejected) before.  Also
    `kept`: the round schedule's result in strength order, which must equal the greedy walk's (checked here)."""
    ys, xs, _ = gftt_candidates(eig, quality)
    h, w = np.asarray(eig).shape
    nc = len(ys)
    rank = np.full((h, w), -1, np.int64); rank[ys, xs] = np.arange(nc)
    md2 = _md2(min_distance); rad = int(np.ceil(min_distance))
    src, dst = [], []
    for dy in range(-rad, rad + 1):
        for dx in range(-rad, rad + 1):
            if (dx == 0 and dy == 0) or dx * dx + dy * dy >= md2:
                continue
            yy, xx = ys + dy, xs + dx
            inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            nb = np.full(nc, -1, np.int64); nb[inside] = rank[yy[inside], xx[inside]]
            sel = (nb >= 0) & (nb < np.arange(nc))                   # a stronger candidate
            src.append(np.nonzero(sel)[0]); dst.append(nb[sel])
    src = np.concatenate(src) if src else np.zeros(0, np.int64); dst = np.concatenate(dst) if dst else np.zeros(0, np.int64)
    nstr = np.bincount(src, minlength=nc)
    state = np.ones(nc, np.int8)                                    # 1 undecided, 2 kept, 3 rejected
    rounds = 0
    while (state == 1).any():
        rounds += 1
        ns = state[dst]
        kept_nb = np.bincount(src, weights=(ns == 2), minlength=nc) > 0
        open_nb = np.bincount(src, weights=(ns == 1), minlength=nc) > 0
        und = state == 1
        new = state.copy()
        new[und & kept_nb] = 3
        new[und & ~kept_nb & ~open_nb] = 2
        assert (new != state).any(), "no progress"
        state = new
    kept = np.nonzero(state == 2)[0]
    walk = gftt_select(eig, 0, quality, min_distance)
    pts = np.stack([xs[kept], ys[kept]], 1).astype(np.float32).reshape(-1, 2)
    assert np.array_equal(pts, walk), "round schedule and greedy walk disagree"
    return dict(candidates=nc, max_stronger=int(nstr.max()) if nc else 0, rounds=rounds, kept=len(kept), pts=walk)


# ------------------------------------------------------------------ filterSpeckles and the int16 median
def speckle_components(img, new_val, max_diff):
    """4-connected components of pixels != new_val whose neighbours differ by <= max_diff: (labels with -1 at new_val, component sizes)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    a = np.asarray(img, np.int16).astype(np.int64); h, w = a.shape
    valid = a != new_val
    idx = np.arange(h * w).reshape(h, w)
    e0, e1 = [], []
    for p, q, vp, vq in ((idx[:, :-1], idx[:, 1:], a[:, :-1], a[:, 1:]), (idx[:-1, :], idx[1:, :], a[:-1, :], a[1:, :])):
        link = (vp != new_val) & (vq != new_val) & (np.abs(vp - vq) <= max_diff)
        e0.append(p[link]); e1.append(q[link])
    e0 = np.concatenate(e0); e1 = np.concatenate(e1)
    g = coo_matrix((np.ones(len(e0), np.int8), (e0, e1)), shape=(h * w, h * w))
    _, lab = connected_components(g, directed=False)
    lab = lab.reshape(h, w)
    _, comp = np.unique(lab[valid], return_inverse=True)
    labels = np.full((h, w), -1, np.int64); labels[valid] = comp
    sizes = np.bincount(comp) if comp.size else np.zeros(0, np.int64)
    return labels, sizes


def filter_speckles(img, new_val, max_size, max_diff):
    labels, sizes = speckle_components(img, new_val, max_diff)
    out = np.array(img, np.int16, copy=True)
    small = np.zeros(len(sizes) + 1, bool); small[:-1] = sizes <= max_size
    out[small[labels] & (labels >= 0)] = new_val
    return out


def median3_s16(img):
    a = np.asarray(img, np.int16)
    p = np.pad(a, 1, mode="edge")
    h, w = a.shape
    st = np.stack([p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)])
    return np.sort(st, axis=0)[4].astype(np.int16)


def tiles_of(mask):
    """the speckle tiles (64 x 16) a set of pixels touches"""
    ys, xs = np.nonzero(mask)
    return set(zip((ys // SPK_TH).tolist(), (xs // SPK_TW).tolist()))


# ------------------------------------------------------------------ GFTT inputs (uint8 images; the eigenvalue map is the oracle's)
def dots(h, w, pts, vals, bg=50):
    img = np.full((h, w), bg, np.uint8)
    for (y, x), v in zip(pts, vals):
        img[y, x] = v
    return img


def gftt_cases():
    """name -> (image, max_corners, quality, min_distance, property check on gftt_properties' dict)"""
    c = {}
    # chains: each dot depends only on its stronger right-hand neighbour (spacing 6 < md 9 < 12); decisions alternate kept / rejected along the row
    pts = [(y, 10 + 6 * k) for y in (16, 40) for k in range(64)]
    c["chain_rising"] = (dots(56, 400, pts, [60 + 2 * k for y in (16, 40) for k in range(64)]), 0, 0.001, 9.0, lambda p: p["rounds"] >= 64)
    c["chain_falling"] = (dots(56, 400, pts, [186 - 2 * k for y in (16, 40) for k in range(64)]), 0, 0.001, 9.0, lambda p: p["rounds"] >= 64)
    # dense clusters: dots of drawn contrast on a 4-px grid (every dot a candidate), minDistance 15 (bit-image scan) and 24 (full scan): more than 32
    # stronger candidates inside a window
    rng = np.random.default_rng(7)
    pts = [(y, x) for y in range(4, 76, 4) for x in range(4, 124, 4)]
    c["cluster_md15"] = (dots(80, 128, pts, rng.integers(120, 250, len(pts))), 0, 0.001, 15.0, lambda p: p["max_stronger"] > GFTT_DEPS)
    c["cluster_md24"] = (dots(80, 128, pts, rng.integers(120, 250, len(pts))), 0, 0.001, 24.0, lambda p: p["max_stronger"] > 2 * GFTT_DEPS)
    # large windows (rad > 15: the deps kernel's full scan); dots at exactly 16 px sit on the boundary of minDistance 16 (kept) and 15.5 (kept)
    pts = [(y, x) for y in range(6, 120, 8) for x in range(6, 250, 8)]
    field = dots(128, 256, pts, rng.integers(100, 250, len(pts)))
    for md in (15.5, 16.0, 31.5, 64.0):
        c[f"window_md{md}"] = (field, 0, 0.001, md, lambda p: p["max_stronger"] > 0)
    pairs = dots(64, 128, [(30, 20), (30, 36), (10, 60), (26, 60), (40, 90), (50, 102)], [200, 190, 180, 170, 160, 150])     # 16^2, 16^2, 12^2 + 10^2 = 244
    c["pairs_md16.0"] = (pairs, 0, 0.001, 16.0, lambda p: p["kept"] == 5 and p["candidates"] == 6)
    c["pairs_md15.5"] = (pairs, 0, 0.001, 15.5, lambda p: p["kept"] == 6)
    # exact ties: identical dots, the order falls back to the raster index; max_corners cuts inside the tied run
    pts = [(y, x) for y in range(5, 60, 5) for x in range(5, 120, 5)]
    tied = dots(64, 128, pts, [200] * len(pts))
    c["ties"] = (tied, 0, 0.01, 7.0, lambda p: p["candidates"] == len(pts) and p["kept"] > 40)
    c["ties_cut"] = (tied, 37, 0.01, 7.0, lambda p: p["kept"] > 37)
    c["ties_md1"] = (tied, 100, 0.01, 1.0, lambda p: p["kept"] == len(pts))
    # plateaus: 2 x 2-pixel checkerboard cells -- nearly every pixel a candidate, more than the w*h/4 + 1024 list of the GPU (which is that long
    # while max_corners is below it); minDistance 1 keeps more corners than the list holds
    c["plateau_64x48_md8"] = (checker(48, 64), 1000, 0.01, 8.0, lambda p: p["candidates"] > 64 * 48 // 4 + 1024 and p["rounds"] > 13)
    c["plateau_64x48_md1"] = (checker(48, 64), 1500, 0.01, 1.0, lambda p: p["candidates"] > 64 * 48 // 4 + 1024 and p["kept"] > 64 * 48 // 4 + 1024)
    c["plateau_64x48_md1.5"] = (checker(48, 64), 1000, 0.01, 1.5, lambda p: p["candidates"] > 64 * 48 // 4 + 1024)
    return c


def checker(h, w, cell=2, lo=30, hi=220, box=None):
    """cell x cell checkerboard (over `box` = (y0, y1, x0, x1) of a smooth textured frame, or everywhere)"""
    yy, xx = np.mgrid[:h, :w]
    cb = np.where(((yy // cell) + (xx // cell)) % 2 == 0, lo, hi).astype(np.uint8)
    if box is None:
        return cb
    img = (100 + 40 * np.sin(yy / 7.0) * np.cos(xx / 11.0) + 20 * np.sin(xx / 3.3)).astype(np.uint8)
    y0, y1, x0, x1 = box
    img[y0:y1, x0:x1] = cb[y0:y1, x0:x1]
    return img


# ------------------------------------------------------------------ speckle / median inputs (int16 maps)
NV = -16            # newVal of the default SGBM parameters: (minDisparity - 1) * 16


def comb(h, w, teeth_x, val=100, nv=NV):
    """1-px vertical teeth that meet only in the last row"""
    a = np.full((h, w), nv, np.int16)
    for x in teeth_x:
        a[:, x] = val
    a[h - 1, min(teeth_x):max(teeth_x) + 1] = val
    return a


def spiral(h, w, nv=NV, step=0, base=100, maxv=32000):
    """a 1-px inward spiral path (arms 1 px apart); values rise by `step` along it (wrapping below maxv)"""
    a = np.full((h, w), nv, np.int16)
    seen = np.zeros((h, w), bool)
    inside = lambda y, x: 0 <= y < h and 0 <= x < w
    y, x, d, k, turns = 0, 0, 0, 0, 0
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    while True:
        seen[y, x] = True; a[y, x] = base + (k * step) % (maxv - base); k += 1
        for _ in range(2):
            dy, dx = dirs[d]
            ny, nx = y + dy, x + dx
            if inside(ny, nx) and not seen[ny, nx] and not (inside(ny + dy, nx + dx) and seen[ny + dy, nx + dx]):
                break
            d = (d + 1) % 4
        else:
            return a
        y, x = ny, nx


def serpentine(h, w, nv=NV, step=0, base=100, period=4000):
    """a 1-px path along every other row, turning at alternate ends; values zig-zag by `step` along it"""
    a = np.full((h, w), nv, np.int16)
    k = 0
    for y in range(0, h, 2):
        xs = range(w) if (y // 2) % 2 == 0 else range(w - 1, -1, -1)
        for x in xs:
            t = k % (2 * period); a[y, x] = base + step * (t if t < period else 2 * period - t); k += 1
        if y + 1 < h:
            x = w - 1 if (y // 2) % 2 == 0 else 0
            t = k % (2 * period); a[y + 1, x] = base + step * (t if t < period else 2 * period - t); k += 1
    return a


def block(h, w, y0, x0, bh, bw, extra=0, val=200, nv=NV, a=None):
    """a bh x bw block (+ `extra` pixels continuing its last row) of one value"""
    a = np.full((h, w), nv, np.int16) if a is None else a
    a[y0:y0 + bh, x0:x0 + bw] = val
    if extra:
        a[y0 + bh, x0:x0 + extra] = val
    return a


def speckle_cases():
    """name -> (maps n x h x w (frames are independent: different maps may be stacked), new_val, max_size, max_diff, property check on (labels, sizes)
    of frame 0)"""
    c = {}
    rng = np.random.default_rng(11)
    one = lambda p: len(p[1]) == 1
    t = comb(40, 260, [10, 70, 130, 250])
    c["comb_cols_removed"] = (t[None], NV, int((t != NV).sum()), 0, lambda p: one(p) and len({tx for _, tx in tiles_of(p[0] >= 0)}) == 4)
    c["comb_cols_kept"] = (t[None], NV, int((t != NV).sum()) - 1, 0, one)
    t = comb(70, 40, [3, 20, 37]).T.copy()                               # teeth = rows in tile rows 0, 1, 2; they meet in the last column
    c["comb_rows"] = (t[None], NV, int((t != NV).sum()), 0, lambda p: one(p) and len({ty for ty, _ in tiles_of(p[0] >= 0)}) == 3)
    t = spiral(65, 127)
    c["spiral_const"] = (t[None], NV, int((t != NV).sum()), 0, lambda p: one(p) and len(tiles_of(p[0] >= 0)) == 10)
    t = spiral(65, 127, step=3)
    c["spiral_ramp"] = (t[None], NV, int((t != NV).sum()), 3, lambda p: one(p) and int(p[0].max()) == 0)
    t = serpentine(376, 1241, step=5)
    c["serpentine_1241x376"] = (t[None], NV, int((t != NV).sum()), 5, lambda p: one(p) and len(tiles_of(p[0] >= 0)) == 20 * 24)
    c["serpentine_split"] = (t[None], NV, int((t != NV).sum()) // 2, 4, lambda p: len(p[1]) > 1000)
    # components of exactly max_size (removed) and max_size + 1 (kept) pixels inside one tile, across a vertical edge, across a tile corner
    h, w = 40, 140
    a = block(h, w, 2, 2, 10, 10)                                        # 100 px, tile (0, 0)
    a = block(h, w, 2, 20, 10, 10, extra=1, val=300, a=a)                # 101 px, tile (0, 0)
    a = block(h, w, 20, 59, 10, 10, val=400, a=a)                        # 100 px over tiles (1, 0) and (1, 1)
    a = block(h, w, 20, 90, 10, 10, extra=1, val=500, a=a)               # 101 px inside tile (1, 1)
    a = block(h, w, 11, 123, 10, 10, val=600, a=a)                       # 100 px over four tiles (x 123..132 crosses 128, y 11..20 crosses 16)
    b = block(h, w, 11, 123, 10, 10, extra=1, val=600, a=a.copy())       # 101 px over four tiles
    c["exact_size"] = (np.stack([a, b]), NV, 100, 0, lambda p: sorted(p[1].tolist()) == [100, 100, 100, 101, 101])
    # neighbours differing by exactly max_diff join, by max_diff + 1 they split; across a tile edge
    a = np.full((20, 130), NV, np.int16); a[2:12, 58:64] = 1000; a[2:12, 64:70] = 1000 + 32          # 60 + 60 joined: 120 > 100
    a[14:19, 58:64] = 2000; a[14:19, 64:70] = 2000 + 33                                             # 30 + 30 split: each <= 100
    c["max_diff_edge"] = (a[None], NV, 100, 32, lambda p: sorted(p[1].tolist()) == [30, 30, 120])
    # new_val pixels cut a component in two halves that are each small
    a = block(32, 128, 4, 40, 20, 40, val=700); a[:, 60] = NV
    c["new_val_cut"] = (a[None], NV, 500, 0, lambda p: sorted(p[1].tolist()) == [380, 400])
    # int16 extremes next to each other and next to new_val; new_val at the extremes
    a = np.full((17, 65), 32767, np.int16); a[:, ::2] = -32768; a[5:9, 30:40] = NV
    c["extremes_split"] = (a[None], NV, 8, 100, lambda p: len(p[1]) >= 65)
    c["extremes_joined"] = (a[None], NV, 1000, 65535, lambda p: len(p[1]) == 1 and p[1][0] == 17 * 65 - 40)
    b = a.copy(); b[3, :] = -32768
    c["extremes_nv_min"] = (b[None], -32768, 5, 0, lambda p: len(p[1]) > 30)
    c["extremes_nv_max"] = (b[None], 32767, 5, 0, lambda p: max(p[1]) > 500)
    # max_diff 0 and dense random maps over a few values, at tile-edge sizes
    for hh, ww in ((1, 1), (1, 1241), (15, 63), (16, 64), (17, 65), (376, 1), (16, 127), (376, 1241)):
        m = rng.choice(np.array([NV, 10, 11, 13, 20], np.int16), size=(hh, ww), p=[0.1, 0.3, 0.3, 0.2, 0.1])
        c[f"dense_{hh}x{ww}_d0"] = (m[None], NV, 4, 0, lambda p: True)
        c[f"dense_{hh}x{ww}_d2"] = (m[None], NV, 6, 2, lambda p: True)
    # frames stacked in one launch: frame k's last row and frame k+1's first row would join if the per-frame forests leaked into each other
    a = np.full((3, 17, 65), NV, np.int16); a[0, -1, :] = 900; a[1, 0, :] = 900; a[1, -1, :] = 900; a[2, 0, :] = 900
    c["frames_do_not_join"] = (a, NV, 100, 0, lambda p: sorted(p[1].tolist()) == [65])
    return c
