"""Planted frames for the fused map stage of the sequence path (map_stream2_kernel in csrc/kernels_map.hip): the case table of tests/test_gpu_map_planted.py and a
plain numpy restatement of the gates of Mapper::generatePointCloud, which tests/test_map_cases.py holds to the oracle (oracle/mapper.c) and to the table's own
claims.  Host only, seeded, deterministic; nothing outside this file is read.

A case = a configuration (frame size, camera, leaf, mapper_max_distance: one context per configuration on the GPU side) + n frames (camera image, depth,
semantic image) + the poses (or none) + what the case claims about itself (`claims`, checked on the CPU).

What the context refuses (build_geometry in csrc/ssm_orb_plan.cpp: frames of 64 .. 4000 pixels a side, and a pyramid level of at least 76 x 76 for the ORB border)
bounds the geometries: the widest frame of the table has 250 words of 16 pixels per row (4000 pixels), not the 256 the kernel's bit image is sized for, and the
narrowest 5 (80 pixels), the lowest 76 rows.  REFUSED lists what was tried beyond that (widths 16, 32, 4064, 4080, 4096, 4112, heights 1, 2, 3, 5):
tests/test_map_cases.py asserts that the plan still refuses them, so that a context that learns to take them cannot leave this table behind."""
import zlib
from collections import namedtuple
from fractions import Fraction

import numpy as np

PALETTE = np.array([[128, 128, 128], [0, 0, 128], [128, 192, 192], [0, 69, 255], [128, 64, 128], [222, 40, 60], [0, 128, 128], [128, 128, 192],
                    [128, 64, 64], [128, 0, 64], [0, 64, 64], [192, 128, 0]], np.uint8)      # BGR, SegNet driving_webdemo id order (tests/golden/palette.json)
SKY, POLE, PEDESTRIAN, CYCLIST = 0, 2, 10, 11
GATED = (SKY, POLE, CYCLIST)                     # mapper.cpp:41-55
MOVING = (PEDESTRIAN, CYCLIST)                   # mapper.cpp:189-216
KEEPABLE = (1, 3, 4, 5, 6, 7, 8, 9)
STRAY = (7, 7, 7)                                # a colour outside the palette: label 255

CAM = (318.6, 255.3, 517.3, 516.5, 1000.0)                                      # tests/conftest.py CAM
CAM_DIV = (318.6, 255.3, float(np.nextafter(512.0, 0.0)), 516.5, 1000.0)        # fx with an all-ones significand: k_map_div refuses it, FASTDIV = false
CAM_5K = (127.37, 47.81, 211.913, 209.377, 5000.0)                              # scale 5000, nothing round, the principal point inside a 256 x 96 frame

Cfg = namedtuple("Cfg", "W H cam leaf maxd")
MS_CH, MS2_CB_WORDS = 3, 3 * 256 + 6 * 256       # csrc/kernels_map.hip
BLOCK_WORDS = MS_CH * 256                        # 16-pixel words of one block: 12288 pixels
WAVE = 1024                                      # pixels of one wave and chunk

# (width, height, why) the context refuses; see the module docstring.  (k_map_fuse's own check refuses fewer than 2 and more than 256 words per row -- at 1 the
# kernel's row reciprocal ceil(2^32 / wpr) would not fit its 32 bits -- but no call can reach it with such a frame.)
REFUSED = [(16, 96, "1 word per row"), (32, 96, "2 words per row"), (64, 96, "4 words per row: the ORB border"), (256, 1, "height"), (256, 2, "height"),
           (256, 3, "height"), (256, 5, "height"), (4064, 131, "254 words per row"), (4080, 96, "255 words per row"), (4096, 96, "256 words per row"),
           (4112, 96, "257 words per row: beyond the kernel's bit image")]
TOO_WIDE = (4112, 96)                            # a multiple of 16 above 4096


class Case:
    def __init__(self, name, cfg, bgr, dep, sem, poses=None, **claims):
        n = len(dep)
        assert bgr.shape == (n, cfg.H, cfg.W, 3) and dep.shape == (n, cfg.H, cfg.W) and sem.shape == bgr.shape, name
        assert bgr.dtype == np.uint8 and dep.dtype == np.uint16 and sem.dtype == np.uint8, name
        assert poses is None or len(poses) == n, name
        self.name, self.cfg, self.n, self.bgr, self.dep, self.sem, self.poses, self.claims = name, cfg, n, bgr, dep, np.ascontiguousarray(sem), poses, claims

    def __repr__(self):
        return "Case(%s, %d x %d x %d)" % (self.name, self.cfg.W, self.cfg.H, self.n)


# ---------------------------------------------------------------- the gates, restated
def hash_slot(b, g, r):
    """slot of the kernel's perfect hash of the palette: (bgr * 0x7589a82b) >> 28 on b | g << 8 | r << 16"""
    return ((int(b) | int(g) << 8 | int(r) << 16) * 0x7589a82b & 0xFFFFFFFF) >> 28


def label_image(sem):
    """[..., 3] BGR -> label ids 0 .. 11, 255 for anything else"""
    lab = np.full(sem.shape[:-1], 255, np.uint8)
    for i, p in enumerate(PALETTE):
        lab[(sem == p).all(-1)] = i
    return lab


def dilate5(m):
    """5 x 5 box dilate of a [n, H, W] boolean image, every frame on its own; nothing outside a frame contributes"""
    n, H, W = m.shape
    p = np.zeros((n, H + 4, W + 4), bool)
    p[:, 2:-2, 2:-2] = m
    out = np.zeros_like(m)
    for dy in range(5):
        for dx in range(5):
            out |= p[:, dy:dy + H, dx:dx + W]
    return out


def keep_mask(case):
    """the pixels Mapper::generatePointCloud emits (mapper.cpp:21-92): [n, H, W] bool"""
    lab = label_image(case.sem)
    d = case.dep.astype(np.float64)
    keep = (case.dep != 0) & (d <= case.cfg.maxd * case.cfg.cam[4])
    keep &= ~np.isin(lab, GATED)
    keep &= ~dilate5(np.isin(lab, MOVING))
    return keep


def wave_counts(case):
    """kept pixels of every aligned 1024-pixel span of every frame (what one wave of the kernel compacts in one chunk): [n, ceil(W H / 1024)]"""
    k = keep_mask(case).reshape(case.n, -1)
    pad = -k.shape[1] % WAVE
    return np.pad(k, ((0, 0), (0, pad))).reshape(case.n, -1, WAVE).sum(-1)


def bit_image_words(wpr, h):
    """per block of a wpr x h frame: the 16-pixel words of the kernel's LDS bit image, (ry1 - ry0 + 1) * wpr -- the block's rows plus two above and below"""
    words = wpr * h
    bw0 = np.arange(0, words, BLOCK_WORDS)
    ry0 = bw0 // wpr - 2
    ry1 = (np.minimum(bw0 + BLOCK_WORDS, words) - 1) // wpr + 2
    return (ry1 - ry0 + 1) * wpr


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))       # exact, rounded once


_scale_ok = {}


def map_div_ok(cam):
    """k_map_div: true when the kernel may replace its three divisions by Markstein's reciprocal form"""
    def plain(f):
        b = int(np.float64(f).view(np.uint64))
        return f > 0 and 0 < (b >> 52 & 0x7FF) < 0x7FF and b & 0xFFFFFFFFFFFFF != 0xFFFFFFFFFFFFF
    scale = float(cam[4])
    if not (plain(scale) and plain(cam[2]) and plain(cam[3])):
        return False
    if scale not in _scale_ok:                                   # every depth through d / scale, as the host does once per camera
        r, ok = 1.0 / scale, True
        for d in range(65536):
            q = float(d) * r
            q = _fma(_fma(-q, scale, float(d)), r, q)
            q = _fma(_fma(-q, scale, float(d)), r, q)
            if q != float(d) / scale:
                ok = False
                break
        _scale_ok[scale] = ok
    return _scale_ok[scale]


def significand_all_ones(f):
    return int(np.float64(f).view(np.uint64)) & 0xFFFFFFFFFFFFF == 0xFFFFFFFFFFFFF


# ---------------------------------------------------------------- frame builders
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _mm(cfg, d):
    """a depth in millimetres -> the camera's depth unit"""
    return np.asarray(np.asarray(d, np.float64) * (cfg.cam[4] / 1000.0)).astype(np.uint16)


def _keepable(cfg, n, rng, block=4):
    """n frames of which every pixel passes every gate: random camera colours, depths of 0.6 .. 3 m, labels from KEEPABLE in block x block patches"""
    W, H = cfg.W, cfg.H
    bgr = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    dep = _mm(cfg, rng.integers(600, 3000, (n, H, W)))
    ids = rng.choice(np.array(KEEPABLE), (n, (H + block - 1) // block, (W + block - 1) // block))
    ids = np.repeat(np.repeat(ids, block, axis=1), block, axis=2)[:, :H, :W]
    return bgr, dep, PALETTE[ids]


def _rigid(rng, angle, t):
    a = rng.normal(size=3); a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4); T[:3, :3] = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K; T[:3, 3] = t
    return T


def _shift(x, y, z):
    T = np.eye(4); T[:3, 3] = (x, y, z)
    return T


def mixed(name, cfg, n, poses="random"):
    """frames like the fuzz test's: holes and far pixels in the depth, all 12 classes in patches of 1, 3 and 8 pixels (the moving ones rare, so that most of
    the frame survives their dilate), 5 % stray colours, a rigid pose per frame"""
    rng = _rng(name)
    W, H = cfg.W, cfg.H
    bgr = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    dep = _mm(cfg, rng.integers(300, 9000, (n, H, W)))
    dep[rng.random((n, H, W)) < 0.3] = 0
    far = min(int(cfg.maxd * cfg.cam[4]) + 1, 65535)
    dep[rng.random((n, H, W)) < 0.1] = far
    sem = np.zeros((n, H, W, 3), np.uint8)
    p = np.array([3 if i in KEEPABLE else 2 if i in (SKY, POLE) else 0.15 for i in range(12)]); p /= p.sum()
    for f in range(n):
        block = (1, 3, 8)[f % 3]
        ids = rng.choice(12, ((H + block - 1) // block, (W + block - 1) // block), p=p)
        sem[f] = PALETTE[np.repeat(np.repeat(ids, block, axis=0), block, axis=1)[:H, :W]]
    s = rng.random((n, H, W)) < 0.05
    sem[s] = rng.integers(0, 256, (int(s.sum()), 3), dtype=np.uint8)
    if isinstance(poses, str):
        poses = [_rigid(rng, rng.random() * 0.6, rng.normal(size=3) * 2) for _ in range(n)]
    return Case(name, cfg, bgr, dep, sem, poses)


# ---- kept pixels per wave
COUNTS = (0, 1, 2, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193, 1023, 1024)
LAYOUTS = ("first", "last")


def _wave_offsets(V, layout, rng=None):
    """which of a wave's 1024 row-major pixels are kept.  first: the first V (the first lanes' words); last: V spread evenly with the wave's last pixel among them
    (the last word holds the last kept pixel); random: any V"""
    if layout == "first":
        return np.arange(V)
    if layout == "last":
        return WAVE - 1 - (np.arange(V) * WAVE // max(V, 1))[::-1]
    return np.sort(rng.permutation(WAVE)[:V])


def waves(name, cfg):
    """3 frames of 256 x 96 = 72 waves.  Waves 0 .. 14 keep exactly COUNTS pixels in layout `first`, waves 15 .. 29 the same in layout `last`, the rest a random
    count at random places.  A pixel that is not kept fails ONE gate, in turn: no depth, too far, sky.  Depths of kept pixels step by 53 mm inside 1.65 .. 1.95 m:
    neighbours fall into different voxels at leaf 0.02 and, mostly, into the same at 0.4."""
    assert (cfg.W, cfg.H) == (256, 96)
    rng = _rng(name)
    n, per = 3, 256 * 96 // WAVE
    bgr, dep, sem = _keepable(cfg, n, rng)
    dep, sem = dep.reshape(n, per, WAVE), sem.reshape(n, per, WAVE, 3)
    far = 65535
    assert far > cfg.maxd * cfg.cam[4]
    planted, counts = {}, np.zeros((n, per), np.int64)
    for g in range(n * per):
        f, w = divmod(g, per)
        if g < 2 * len(COUNTS):
            V, layout = COUNTS[g % len(COUNTS)], LAYOUTS[g // len(COUNTS)]
            planted[(V, layout)] = (f, w)
        else:
            V, layout = int(rng.integers(0, WAVE + 1)), "random"
        off = _wave_offsets(V, layout, rng)
        assert len(off) == V and len(set(off.tolist())) == V and (V == 0 or (0 <= off.min() and off.max() < WAVE))
        keep = np.zeros(WAVE, bool); keep[off] = True
        o = np.arange(WAVE)
        dep[f, w] = _mm(cfg, 1650 + (o + 7 * g) * 53 % 300)
        gone = np.flatnonzero(~keep)
        dep[f, w, gone[0::3]] = 0
        dep[f, w, gone[1::3]] = far
        sem[f, w, gone[2::3]] = PALETTE[SKY]
        counts[f, w] = V
    return Case(name, cfg, bgr, dep.reshape(n, 96, 256), sem.reshape(n, 96, 256, 3), [_shift(0, 0, 0), _rigid(rng, 0.3, (0.5, -0.25, 1.0)), _shift(0.013, 0.007, -0.011)],
                planted=planted, counts=counts)


# ---- runs inside one lane's share
RUN_PATTERNS = ("AAAA", "AB", "ABA", "ABCD", "A?B")


def run_pattern(kind, P, labs):
    """labels of the P consecutive kept pixels of one lane (255: a stray colour)"""
    A, B, Cc, D = labs
    if kind == "AAAA":
        return [A] * P
    if kind == "AB":
        return [A] * (P // 2) + [B] * (P - P // 2)
    if kind == "ABA":
        return [A] * 5 + [B] * 5 + [A] * (P - 10)
    if kind == "ABCD":
        return [(A, B, Cc, D)[i * 4 // P] for i in range(P)]
    return [A] * 5 + [255] * 2 + [B] * (P - 7)


def runs(name, cfg):
    """2 frames of 256 x 96 at ONE depth (2 m: 3.9 mm a pixel, a voxel of leaf 0.4 spans a hundred pixels).  Frame 0 keeps every pixel (V = 1024, P = 16 a lane),
    frame 1 all but the last 64 of every wave (V = 960, P = 15, odd: the second pixel of a lane's last loop trip is past its share).  Lane i of a wave owns
    pixels [i P, (i + 1) P) of it; wave w repeats RUN_PATTERNS[w % 5] with period P, so every lane's share holds exactly that pattern."""
    assert (cfg.W, cfg.H) == (256, 96)
    rng = _rng(name)
    n, per = 2, 256 * 96 // WAVE
    bgr, dep, sem = _keepable(cfg, n, rng)
    dep[:] = _mm(cfg, 2000)
    dep, sem = dep.reshape(n, per, WAVE), sem.reshape(n, per, WAVE, 3)
    shares = {}
    for f in range(n):
        V = WAVE if f == 0 else WAVE - 64
        P = (V + 63) // 64
        dep[f, :, V:] = 0
        for w in range(per):
            kind = RUN_PATTERNS[w % 5]
            labs = [KEEPABLE[(w + 3 * j) % len(KEEPABLE)] for j in range(4)]
            assert len(set(labs)) == 4
            pat = np.array(run_pattern(kind, P, labs))
            lab = np.resize(pat, V)
            sem[f, w, :V] = np.where((lab == 255)[:, None], np.array(STRAY, np.uint8), PALETTE[np.minimum(lab, 11)])
            shares[(f, w)] = (kind, P, V, pat)
    return Case(name, cfg, bgr, dep.reshape(n, 96, 256), sem.reshape(n, 96, 256, 3), None, shares=shares)


def one_voxel(name, cfg):
    """2 frames of 256 x 96, every pixel kept, a pose that moves the whole cloud inside ONE voxel of the (50 m) leaf: each block adds its 12288 pixels to one slot
    of its LDS table.  Frame 0 votes 8 and 9 (the two 16-bit halves of one packed histogram word, 5 : 3), frame 1 votes 1 and 4 (an odd and an even label in two
    words, 3 : 5)."""
    assert (cfg.W, cfg.H) == (256, 96)
    rng = _rng(name)
    bgr, dep, sem = _keepable(cfg, 2, rng)
    o = np.arange(256 * 96).reshape(96, 256)
    sem[0] = PALETTE[np.where(o % 8 < 5, 8, 9)]
    sem[1] = PALETTE[np.where(o % 8 < 3, 1, 4)]
    votes = {8: 256 * 96 * 5 // 8, 9: 256 * 96 * 3 // 8, 1: 256 * 96 * 3 // 8, 4: 256 * 96 * 5 // 8}
    return Case(name, cfg, bgr, dep, sem, [_shift(10, 10, 0), _shift(10, 10, 0)], votes=votes)


def flat(name, cfg):
    """1 frame of 256 x 96 at 0.6 m: a block's 12288 pixels cover 0.3 x 0.06 m, far fewer than 256 voxels of leaf 0.02 -- the block table never fills"""
    bgr, dep, sem = _keepable(cfg, 1, _rng(name))
    dep[:] = _mm(cfg, 600)
    return Case(name, cfg, bgr, dep, sem, [_shift(0, 0, 0)])


# ---- the 5 x 5 dilate
BOUNDARY_DX = {-2: (-28,), -1: (-17,), 0: (-6, 5), 1: (16,), 2: (27,)}      # row offset from the boundary's row -> column offsets from the boundary's column


def block_boundary_plants(W, H):
    """(x, y) of the pixels planted around every boundary between two blocks of the kernel (a block ends in the middle of a row unless its 768 words are whole
    rows): the two rows on each side of the boundary's row and that row itself, on it one pixel in the upper block's words and one in the lower block's -- every
    one in a column of its own, 11 pixels from the next, so that no two 5 x 5 neighbourhoods touch and each masked pixel has ONE cause"""
    wpr, out = W // 16, []
    for bw in range(BLOCK_WORDS, wpr * H, BLOCK_WORDS):
        r, xw = divmod(bw, wpr)
        out += [((16 * xw + dx) % W, r + dy) for dy in range(-2, 3) for dx in BOUNDARY_DX[dy] if 0 <= r + dy < H]
    return out


def dilate(name, cfg, swap=0):
    """3 frames, every pixel keepable but for SINGLE pedestrian / cyclist pixels (alternating; the other way round with `swap`), no two closer than 5 pixels in
    both directions, whose 5 x 5 neighbourhoods the kernel must drop:
    frame 0: columns 0 1 2 13 14 15 16 17 18 W-3 W-2 W-1 (the frame's edges and the seam between two 16-pixel words), one row each, and the frame's LAST two rows;
    frame 1: rows 0 1 2 H-3 H-2 H-1 and the corners, and so the frame's FIRST two rows: nothing of frame 0's last rows may mask frame 1's first, nor the reverse;
    frame 2: block_boundary_plants alone -- what such a pixel masks on the other side of the boundary lies in the rows that the other block classifies as its
    halo, and nothing else in the frame masks it."""
    rng = _rng(name)
    W, H = cfg.W, cfg.H
    bgr, dep, sem = _keepable(cfg, 3, rng)
    xs = [0, 1, 2, 13, 14, 15, 16, 17, 18, W - 3, W - 2, W - 1]
    ys = [0, 1, 2, H - 3, H - 2, H - 1]
    a = [(x, (4 + 7 * i) % H) for i, x in enumerate(xs)] + [(40, H - 1), (W // 2 + 20, H - 2)]
    b = [(20 + 9 * j, y) for j, y in enumerate(ys)] + [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
    c = block_boundary_plants(W, H)
    planted = []
    for f, pts in ((0, a), (1, b), (2, c)):
        for i, (x, y) in enumerate(pts):
            sem[f, y, x] = PALETTE[MOVING[(i + swap) % 2]]
            planted.append((f, x, y))
    return Case(name, cfg, bgr, dep, sem, [_shift(0, 0, 0)] * 3, planted=planted, xs=xs, ys=ys, boundary=c)


# ---- the label lookup
def slot_colours():
    """for each of the 16 slots of the kernel's hash a colour that is NOT of the palette and hashes there (the first of a seeded stream)"""
    rng, out = _rng("slot colours"), {}
    pal = {tuple(p) for p in PALETTE.tolist()}
    while len(out) < 16:
        c = tuple(int(v) for v in rng.integers(0, 256, 3))
        if c not in pal and c != (1, 0, 0):
            out.setdefault(hash_slot(*c), c)
    return [out[s] for s in range(16)]


def label_colours(with_moving):
    pal = [tuple(p) for p in PALETTE.tolist()]
    near = []
    for p in pal:
        for ch in range(3):
            for dv in (-1, 1):
                q = list(p); q[ch] += dv
                if 0 <= q[ch] <= 255:
                    near.append(tuple(q))
    cols = [p for i, p in enumerate(pal) if with_moving or i not in MOVING] + near + slot_colours() + [(1, 0, 0), (0, 0, 0), (255, 255, 255)]
    return np.array(cols, np.uint8)


def labels(name, cfg):
    """2 frames: every colour of label_colours(), one a pixel, round and round (a list length prime to 16 would not matter: the rows shift it).  Frame 0 leaves out
    the two moving colours themselves (not their neighbours one channel off, which must NOT mask anything), frame 1 has them too."""
    rng = _rng(name)
    bgr, dep, sem = _keepable(cfg, 2, rng)
    for f in range(2):
        cols = label_colours(bool(f))
        i = np.arange(cfg.W * cfg.H).reshape(cfg.H, cfg.W)
        sem[f] = cols[(i + 3 * (i // cfg.W)) % len(cols)]
    return Case(name, cfg, bgr, dep, sem, None)


# ---- the depth gate
def dmax_of(cfg):
    """the largest integer depth the gate keeps: floor(max_distance * scale), at most 65535"""
    return min(int(np.floor(cfg.maxd * cfg.cam[4])), 65535)


def depth_gate(name, cfg):
    """1 frame, every pixel keepable but for its depth, which runs through 0, 1, dmax - 1, dmax, dmax + 1, 65535 (and a few ordinary ones)"""
    rng = _rng(name)
    bgr, dep, sem = _keepable(cfg, 1, rng)
    dm = dmax_of(cfg)
    vals = sorted({0, 1, dm - 1, dm, min(dm + 1, 65535), 65535, dm // 2, dm // 3})
    i = np.arange(cfg.W * cfg.H).reshape(cfg.H, cfg.W)
    dep[0] = np.array(vals, np.uint16)[(i + 5 * (i // cfg.W)) % len(vals)]
    return Case(name, cfg, bgr, dep, sem, None, values=vals)


# ---------------------------------------------------------------- the table
MAXD_FRACTION = 3.3003           # x 1000 = 3300.3000000000002: not an integer, the gate keeps d <= 3300
MAXD_BELOW = 1.005               # x 1000 = 1004.9999999999999: just BELOW an integer, the gate keeps d <= 1004 and drops 1005 (the oracle compares in double)
G0 = Cfg(256, 96, CAM, 0.02, 40.0)
G_COARSE = Cfg(256, 96, CAM, 0.4, 40.0)
G_ONE = Cfg(256, 96, CAM, 50.0, 40.0)
G_DIV = Cfg(256, 96, CAM_DIV, 0.02, 40.0)
G_5K = Cfg(256, 96, CAM_5K, 0.02, 7.77)
G_D40 = Cfg(256, 96, CAM, 0.1, 40.0)            # (the depth cases reach from 1 mm to 65 m: at leaf 0.02 pcl::VoxelGrid refuses so wide a box, and so does the oracle)
G_FRACTION = Cfg(256, 96, CAM, 0.1, MAXD_FRACTION)
G_BELOW = Cfg(256, 96, CAM, 0.1, MAXD_BELOW)
G_CLAMP = Cfg(256, 96, CAM, 0.1, 100.0)


def _cam_for(W, H):
    return (W / 2 - 0.37, H / 2 + 0.21, 431.7, 437.9, 1000.0)


# widths (16-pixel words per row): 250, the widest the context takes, where block 13 of a frame starts 234 words into a row and spans five rows -- the largest bit
# image a context can ask for, 9 rows x 250 = 2250 of the 2304 words; 249 (odd, as wide); 41 (odd: rows start in the middle of waves and chunks) with an odd
# height; 11 x 88 = 968 words, no multiple of 64, 256 or 768 (the round-4 finding recorded in the kernel); 5 x 76, the smallest frame the context takes
WIDE = Cfg(4000, 76, _cam_for(4000, 76), 0.1, 40.0)
WIDTHS = [WIDE, Cfg(3984, 77, _cam_for(3984, 77), 0.1, 40.0), Cfg(656, 77, _cam_for(656, 77), 0.1, 40.0), Cfg(176, 88, _cam_for(176, 88), 0.1, 40.0),
          Cfg(80, 76, _cam_for(80, 76), 0.05, 40.0)]
ORDERED = Cfg(250, 90, _cam_for(250, 90), 0.1, 40.0)          # W % 16 != 0: mask -> ordered back-projection -> insert, through the same call

DILATE = [("dilate", G0), ("dilate 176 x 88", WIDTHS[3]), ("dilate 656 x 77", WIDTHS[2]), ("dilate 80 x 76", WIDTHS[4])]
_table = []


def table():
    """every case, built once"""
    if _table:
        return _table
    t = _table
    t += [waves("waves", G0), waves("waves, coarse", G_COARSE), waves("waves, division", G_DIV), waves("waves, scale 5000", G_5K)]
    t += [runs("runs", G_COARSE), runs("runs, fine", G0), one_voxel("one voxel", G_ONE), flat("flat", G0)]
    for nm, cfg in DILATE:
        t += [dilate(nm, cfg), dilate(nm + ", swapped", cfg, swap=1)]
    t += [labels("labels", G0), labels("labels, division", G_DIV)]
    t += [depth_gate("depth 40 m", G_D40), depth_gate("depth 3.3003 m", G_FRACTION), depth_gate("depth 1.005 m", G_BELOW), depth_gate("depth 100 m", G_CLAMP),
          depth_gate("depth 7.77 m, scale 5000", G_5K)]
    t += [mixed("mixed", G0, 3), mixed("mixed, division", G_DIV, 3), mixed("mixed, scale 5000", G_5K, 3), mixed("mixed, coarse", G_COARSE, 3)]
    t += [mixed("no pose", G0, 3, poses=None), mixed("no pose, division", G_DIV, 2, poses=None)]
    r = _rng("poses")
    t += [mixed("poses", G0, 3, poses=[np.eye(4), _rigid(r, 2.5, (-1.0, -2.0, -3.0)), _rigid(r, 1.9, (-0.5, -0.5, -4.0))])]
    for cfg in WIDTHS:
        t.append(mixed("width %d x %d" % (cfg.W, cfg.H), cfg, 1 if cfg.W > 1000 else 3))
    t.append(mixed("ordered 250 x 90", ORDERED, 3))
    # out of range: frame 1 wholly (voxel index about 1.5e6 at leaf 0.02), frame 2 partly (x index around 2^20, which is 20971.52 m: the camera looks at negative x, so the shift is 20973.5), frame 0 not at all; and a frame
    # whose indices saturate the float -> int conversion
    t.append(mixed("out of range", G0, 3, poses=[np.eye(4), _shift(30000.0, 0, 0), _shift(20973.5, 0, 0)]))
    t.append(mixed("out of range, saturating", G0, 2, poses=[_shift(1e12, -1e12, 1e12), np.eye(4)]))
    for c in t[-2:]:
        c.claims["out_of_range"] = True
    assert len({c.name for c in t}) == len(t)
    return t


def groups():
    """configuration -> its cases, in table order"""
    g = {}
    for c in table():
        g.setdefault(c.cfg, []).append(c)
    return g


def case(name):
    return next(c for c in table() if c.name == name)
