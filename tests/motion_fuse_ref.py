"""An independent restatement of the semantic-motion fusion in numpy + scipy.ndimage, and the case list the CPU and the GPU tests share.

The restatement uses scipy's morphology and labelling, nothing of the library: binary_dilation by the 5 x 5 box, binary_fill_holes (its default structure
is the 4-connected cross: a hole is what the 4-connected background cannot reach from outside the image), label with the full 3 x 3 structure, and the
per-label minimum index, pixel count and count of motion == 255.  The one float operation is written with numpy's float32.

A case is (sem, motion or None, area_thres, overlay_thres).  Shapes are drawn in CLASS pixels; what the fusion labels is their 5 x 5 dilation, so a lone class
pixel is a 5 x 5 box, boxes whose centres are 5 apart touch, and a zero corridor one pixel wide is a band of 5 class-free pixels."""
import numpy as np
from scipy import ndimage

CAR, PED, BIKE = (128, 0, 64), (0, 64, 64), (192, 128, 0)
BOX5, FULL3 = np.ones((5, 5), bool), np.ones((3, 3), bool)


def fuse(sem, motion, area_thres, overlay_thres):
    """-> dict(mask, always, cand, labels, area, overlap, info)"""
    sem = np.asarray(sem, np.uint8)
    h, w = sem.shape[:2]
    b, g, r = (sem[..., i].astype(np.int32) for i in range(3))
    is_ = lambda c: (b == c[0]) & (g == c[1]) & (r == c[2])  # noqa: E731
    alw = is_(PED) | is_(BIKE)
    always = ndimage.binary_dilation(alw, structure=BOX5)
    cand = ndimage.binary_dilation(alw | is_(CAR), structure=BOX5)
    filled = ndimage.binary_fill_holes(cand)
    lab, k = ndimage.label(filled, structure=FULL3)
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    ids = np.arange(1, k + 1)
    hit = np.zeros((h, w), bool) if motion is None else (np.asarray(motion) == 255)
    roots = np.asarray(ndimage.minimum(idx, lab, ids), np.int64).reshape(-1) if k else np.zeros(0, np.int64)
    areas = np.asarray(ndimage.sum(np.ones((h, w)), lab, ids), np.int64).reshape(-1) if k else np.zeros(0, np.int64)
    overs = np.asarray(ndimage.sum(hit, lab, ids), np.int64).reshape(-1) if k else np.zeros(0, np.int64)
    overlay = (overs.astype(np.float32) * np.float32(1.0) / (areas + 1).astype(np.float32)).astype(np.float32)
    large = areas > area_thres
    conf = large & (overlay.astype(np.float64) > np.float64(overlay_thres))
    labels = np.full((h, w), -1, np.int32)
    labels[lab > 0] = roots[lab[lab > 0] - 1]
    area = np.zeros(h * w, np.int32); overlap = np.zeros(h * w, np.int32)
    area[roots] = areas; overlap[roots] = overs
    conf_px = np.zeros((h, w), bool)
    conf_px[lab > 0] = conf[lab[lab > 0] - 1]
    mask = np.where(always | conf_px, 255, 0).astype(np.uint8)
    info = dict(blobs=int(k), large=int(large.sum()), confirmed=int(conf.sum()), added=int((conf_px & ~always).sum()))
    return dict(mask=mask, always=np.where(always, 255, 0).astype(np.uint8), cand=np.where(cand, 255, 0).astype(np.uint8), labels=labels,
                area=area.reshape(h, w), overlap=overlap.reshape(h, w), info=info)


# ---------------------------------------------------------------- cases
def blank(w, h):
    sem = np.zeros((h, w, 3), np.uint8)
    sem[:] = (128, 128, 128)          # Sky: no class of interest
    return sem


def paint(sem, ys, xs, colour=CAR):
    sem[ys, xs] = colour
    return sem


def random_case(w, h, seed, density=0.02, thres=30):
    """sparse class pixels (mostly Car): boxes that merge into blobs with holes; motion 255 on about a third of the image, 254 on some of the rest"""
    rng = np.random.default_rng(seed)
    sem = blank(w, h)
    u = rng.random((h, w))
    sem[u < density] = CAR
    sem[u < density * 0.15] = PED
    sem[(u >= density * 0.15) & (u < density * 0.25)] = BIKE
    m = rng.random((h, w))
    motion = np.where(m < 0.35, 255, np.where(m < 0.5, 254, 0)).astype(np.uint8)
    return sem, motion, thres, 0.3


def lattice(w, h):
    """class pixels at (5 i + 2, 5 j + 2), i + j even: 5 x 5 boxes in a checkerboard.  They touch at their corners only: one 8-connected blob, and the zero
    boxes between them are 4-connected to nothing (inside the image they are holes)"""
    sem = blank(w, h)
    for j in range(h // 5):
        for i in range(w // 5):
            if (i + j) % 2 == 0:
                sem[5 * j + 2, 5 * i + 2] = CAR
    motion = np.zeros((h, w), np.uint8); motion[::2] = 255
    return sem, motion, 100, 0.3


def diagonals(tw, th):
    """chains of boxes that touch corner to corner exactly at tile corners: down-right through (tw, th), down-left through (2 tw, th)"""
    w, h = 3 * tw + 7, 3 * th + 9
    sem = blank(w, h)
    for k in range(-2, 3):
        for cx, cy in ((tw - 3 + 5 * k, th - 3 + 5 * k), (2 * tw + 2 - 5 * k, th - 3 + 5 * k)):
            if 0 <= cx < w and 0 <= cy < h:
                sem[cy, cx] = CAR
    motion = np.full((h, w), 255, np.uint8)
    return sem, motion, 50, 0.5


def serpentine_zeros(tw, th):
    """everything is class except a band of 5 around a serpentine path: the zeros are a corridor one pixel wide that winds over several tiles and ends on the
    image border -- a long 4-connected chain to the outside.  A second corridor, closed, is a hole"""
    w, h = 3 * tw + 5, 3 * th + 3
    free = np.zeros((h, w), bool)
    rows = list(range(4, h - 16, 6))
    for k, y in enumerate(rows):
        free[y, 8:w - 8] = True
        if k + 1 < len(rows):
            x = w - 9 if k % 2 == 0 else 8
            free[y:rows[k + 1] + 1, x] = True
    free[rows[0], :9] = True                    # the open end
    free[h - 6, 8:w - 8] = True                 # the closed corridor
    sem = blank(w, h)
    sem[~ndimage.binary_dilation(free, structure=BOX5)] = CAR
    motion = np.zeros((h, w), np.uint8); motion[:, ::3] = 255
    return sem, motion, 100, 0.2


def serpentine_blob(tw, th):
    """a class path one pixel wide, winding with 3-pixel gaps that open onto the left and right border in turn: one snake-shaped blob over several tiles
    (long 8-connected chains), the gaps outside"""
    w, h = 3 * tw + 5, 3 * th + 3
    sem = blank(w, h)
    rows = list(range(2, h - 2, 8))
    for k, y in enumerate(rows):
        sem[y, 2:w - 2] = CAR if k % 2 == 0 else PED
        if k + 1 < len(rows):
            sem[y:rows[k + 1] + 1, w - 3 if k % 2 == 0 else 2] = CAR
    motion = np.zeros((h, w), np.uint8); motion[h // 2:] = 255
    return sem, motion, 200, 0.4


def ring_with_island(tw, th):
    w, h = 2 * tw + 9, 2 * th + 11
    sem = blank(w, h)
    sem[6, 10:w - 10] = CAR; sem[h - 7, 10:w - 10] = CAR; sem[6:h - 6, 10] = CAR; sem[6:h - 6, w - 11] = CAR
    sem[h // 2, w // 2] = PED                    # the island: part of the ring's blob, and always moving
    motion = np.zeros((h, w), np.uint8); motion[:, :w // 2] = 255
    return sem, motion, 300, 0.4


def diagonal_ring(tw, th):
    """boxes touching corner to corner in a closed diamond: 4-connected zeros cannot leave it, so the inside is a hole"""
    w, h = tw + 30, 75
    sem = blank(w, h)
    cx, cy, r = w // 2, 37, 6
    for k in range(r):
        for sx, sy in ((cx + 5 * k, cy - 5 * (r - k)), (cx + 5 * (r - k), cy + 5 * k), (cx - 5 * k, cy + 5 * (r - k)), (cx - 5 * (r - k), cy - 5 * k)):
            sem[sy, sx] = CAR
    motion = np.full((h, w), 255, np.uint8)
    return sem, motion, 500, 0.9


def cross(tw, th):
    """a blob that touches all four borders"""
    w, h = 2 * tw + 3, 2 * th + 5
    sem = blank(w, h)
    sem[h // 2, :] = CAR; sem[:, w // 2] = CAR
    return sem, np.full((h, w), 255, np.uint8), 100, 0.5


def border_hole(tw, th):
    """a C whose opening is the image border: the zeros inside reach the frame, so they are outside, not a hole -- next to a closed ring of the same size"""
    w, h = 2 * tw + 20, th + 30
    sem = blank(w, h)
    sem[5, 0:30] = CAR; sem[h - 6, 0:30] = CAR; sem[5:h - 5, 30] = CAR
    sem[5, 50:90] = CAR; sem[h - 6, 50:90] = CAR; sem[5:h - 5, 50] = CAR; sem[5:h - 5, 89] = CAR
    return sem, np.full((h, w), 255, np.uint8), 100, 0.5


def merging_boxes():
    """centres 5 apart: the boxes touch and are one blob; 6 apart: two blobs"""
    sem = blank(60, 20)
    sem[8, 10] = CAR; sem[8, 15] = CAR; sem[8, 35] = CAR; sem[8, 41] = BIKE
    return sem, np.full((20, 60), 255, np.uint8), 30, 0.5


def area_edge(thres):
    """one box of 25 pixels, all under motion"""
    sem = blank(20, 20); sem[9, 9] = CAR
    return sem, np.full((20, 20), 255, np.uint8), thres, 0.5


def overlap_edge(hits):
    """a blob of 999 pixels (mask_count 1000) with `hits` pixels under motion == 255 and all the others under 254"""
    sem = blank(50, 50)
    sem[5:38, 8:31] = CAR                       # 33 x 23 class pixels -> 37 x 27 = 999
    motion = np.full((50, 50), 254, np.uint8)
    blob = np.argwhere(ndimage.binary_dilation((sem[..., 0] == 128) & (sem[..., 2] == 64), structure=BOX5))
    assert len(blob) == 999
    for y, x in blob[::7][:hits]:
        motion[y, x] = 255
    return sem, motion, 500, 0.143


def full_size(w, h, seed):
    """cars as filled rectangles and outlines, pedestrians, class noise; motion over some of the cars"""
    rng = np.random.default_rng(seed)
    sem, motion = blank(w, h), np.zeros((h, w), np.uint8)
    for k in range(14):
        x0, y0 = int(rng.integers(0, w - 40)), int(rng.integers(0, h - 30))
        bw, bh = int(rng.integers(20, 200)), int(rng.integers(15, 120))
        x1, y1 = min(w, x0 + bw), min(h, y0 + bh)
        if k % 3 == 2:
            sem[y0:y1, x0] = CAR; sem[y0:y1, x1 - 1] = CAR; sem[y0, x0:x1] = CAR; sem[y1 - 1, x0:x1] = CAR
        else:
            sem[y0:y1, x0:x1] = CAR if k % 5 else PED
        if k % 2 == 0:
            motion[y0:(y0 + y1) // 2 + 3, x0:x1] = 255
    u = rng.random((h, w))
    sem[u < 0.002] = CAR
    motion[rng.random((h, w)) < 0.05] = 255
    return sem, motion, 1000, 0.143


def cases(tw, th):
    """name -> builder, for a device tile of tw x th"""
    c = {}
    for name, (w, h) in {"1x1": (1, 1), "1x70": (1, 70), "70x1": (70, 1), "67x35": (67, 35), "2tiles+1": (2 * tw + 1, 2 * th + 1)}.items():
        c["size_" + name] = lambda w=w, h=h: random_case(w, h, 1000 + w * 7 + h)
    for dw in (-1, 0, 1):
        for dh in (-1, 0, 1):
            c[f"size_tile{dw:+d}x{dh:+d}"] = lambda dw=dw, dh=dh: random_case(tw + dw, th + dh, 50 + 3 * dw + dh)
    c["size_1x1_car"] = lambda: (paint(blank(1, 1), 0, 0), np.full((1, 1), 255, np.uint8), 0, 0.4)
    c["all_zero"] = lambda: (blank(tw + 9, th + 5), np.full((th + 5, tw + 9), 255, np.uint8), 10, 0.1)
    c["all_set"] = lambda: (paint(blank(tw + 9, th + 5), slice(None), slice(None)), np.full((th + 5, tw + 9), 255, np.uint8), 10, 0.1)
    c["no_motion"] = lambda: random_case(2 * tw + 3, 2 * th + 3, 77)[:1] + (None, 30, 0.3)
    c["lattice"] = lambda: lattice(2 * tw + 11, 3 * th + 4)
    c["diagonals"] = lambda: diagonals(tw, th)
    c["serpentine_zeros"] = lambda: serpentine_zeros(tw, th)
    c["serpentine_blob"] = lambda: serpentine_blob(tw, th)
    c["ring_with_island"] = lambda: ring_with_island(tw, th)
    c["diagonal_ring"] = lambda: diagonal_ring(tw, th)
    c["cross"] = lambda: cross(tw, th)
    c["border_hole"] = lambda: border_hole(tw, th)
    c["merging_boxes"] = merging_boxes
    c["area_eq_thres"] = lambda: area_edge(25)
    c["area_thres_plus_1"] = lambda: area_edge(24)
    c["overlap_143"] = lambda: overlap_edge(143)
    c["overlap_142"] = lambda: overlap_edge(142)
    return c


FULL = {"640x480": lambda: full_size(640, 480, 5), "1241x376": lambda: full_size(1241, 376, 6)}
BATCH = lambda: [random_case(67, 35, s, density=d) for s, d in ((11, 0.02), (12, 0.05), (13, 0.01))]  # noqa: E731
