"""The FAST quick test on the GPU (fast_tile's column-group walk, ssm_fq::quick4, the right-edge mask) at its decision boundary, against
oracle/orb.c byte for byte.  The image is a lattice of isolated 7 x 7 stamps on a flat background b (bands of b = 21, 128, 234: b +- d stays a
byte), on a 13-px pitch (co-prime with the 30-px cells): each stamp has 9 contiguous ring pixels at b + d or b - d around a centre at b, in all 16
arc rotations, bright and dark, with d = t and t + 1 for both thresholds -- the centre of a stamp has S = d exactly, so it is a corner at t for
d = t + 1 and none for d = t, and the compass test sees values exactly at and one above c +- t.  The left part of the image carries d = iniThFAST,
iniThFAST + 1 (every cell there has a corner at iniThFAST: pass 1), the right part d = minThFAST, minThFAST + 1 (cells empty at iniThFAST: pass 2).
Geometries: 176 x 88 with one level (the smallest the tiles support: short tiles, fewer than 32 groups) and 641 x 479 with 8 levels (remainder
tiles, odd rows, every row count modulo 3).  On the oracle's output alone: keypoints exist, some below iniThFAST and some at or above it, and
no keypoint of the level the stamps are drawn on (octave 0: higher octaves see resampled stamps, which are no 9-arcs at b +- d any more) lies
within 3 px of a stamp with d == t."""
import numpy as np
import pytest

from conftest import CAM, SEED

pytestmark = pytest.mark.gpu

INI, MIN = 20, 7          # ssm_config_default's iniThFAST, minThFAST
PITCH = 13
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]
GEOMS = [(176, 88, 1, 1.2), (641, 479, 8, 1.2)]


def _lattice(w, h):
    """-> image, stamps as rows (cx, cy, d, t, b, rotation, bright)"""
    band = 3 * PITCH
    img = np.zeros((h, w), np.uint8)
    for y in range(h):
        img[y] = (21, 128, 234)[(y // band) % 3]
    stamps = []
    for iy, cy in enumerate(range(6, h - 6, PITCH)):
        if (cy % band) < 3 or (cy % band) >= band - 3:          # a stamp stays inside one band
            continue
        for ix, cx in enumerate(range(6, w - 6, PITCH)):
            t = INI if cx < w * 5 // 8 else MIN
            d = t + (ix + iy) % 2
            k = ix // 2 + 5 * iy
            rot, bright, b = k % 16, (k // 16 + ix) % 2, int(img[cy, cx])
            for j in range(9):
                dx, dy = RING[(rot + j) % 16]
                img[cy + dy, cx + dx] = b + d if bright else b - d
            stamps.append((cx, cy, d, t, b, rot, bright))
    return img, np.array(stamps)


def _reference(oracle, w, h, levels, scale):
    img, stamps = _lattice(w, h)
    ok, od = oracle.orb_extract(img, nfeatures=600, scale=scale, nlevels=levels)
    assert len(ok) > 0
    assert ok["response"].min() < INI <= ok["response"].max()                 # both passes contribute
    at_t = stamps[stamps[:, 2] == stamps[:, 3]]
    k0 = ok[ok["octave"] == 0]
    assert len(k0) > 0 and len(at_t) > 0
    dist = np.maximum(np.abs(k0["x"][:, None] - at_t[None, :, 0]), np.abs(k0["y"][:, None] - at_t[None, :, 1]))
    assert dist.min() > 3 + 3, dist.min()                                     # 3 px from the 7 x 7 stamp = 6 from its centre
    # the stamps inside the FAST window of level 0 cover what the docstring lists (the small geometry holds only a part of it)
    inside = stamps[(stamps[:, 0] >= 19) & (stamps[:, 0] < w - 19) & (stamps[:, 1] >= 19) & (stamps[:, 1] < h - 19)]
    assert {int(d) for d in inside[:, 2]} == {MIN, MIN + 1, INI, INI + 1}
    if w > 600:
        assert len({(int(s[2]), int(s[5]), int(s[6])) for s in inside}) == 4 * 16 * 2
        assert len({(int(s[2]), int(s[4])) for s in inside}) == 4 * 3
    return img, ok, od


def _compare(oracle, gk, gd, gp, ok, od, depth):
    assert len(gk) == len(ok)
    for f in ("x", "y", "size", "response", "octave", "class_id", "angle"):
        assert np.array_equal(gk[f], ok[f]), f
    assert np.array_equal(gd, od)
    for i in range(len(ok)):
        assert oracle.project2dTo3d(depth, CAM, int(ok["x"][i]), int(ok["y"][i])).tobytes() == gp[i].tobytes(), i


def _ctx(w, h, levels, scale, batch):
    import semantic_slam_mapping_amd as ssm
    return ssm.Context(0, width=w, height=h, orb_levels=levels, orb_scale=scale, orb_features=600, max_batch=batch, voxel_capacity_log2=18,
                       camera=CAM)


@pytest.mark.parametrize("w,h,levels,scale", GEOMS)
def test_stamps_at_the_thresholds_match_oracle(oracle, w, h, levels, scale):
    img, ok, od = _reference(oracle, w, h, levels, scale)
    depth = oracle.synth_frame(SEED, 2, w, h)[1]
    c = _ctx(w, h, levels, scale, 1)
    try:
        gk, gd, gp = c.detect_features(img, depth)
        _compare(oracle, gk, gd, gp, ok, od, depth)
    finally:
        c.close()


def test_stamps_at_the_thresholds_batched_match_oracle(oracle):
    """the same image as a batch of 3 frames through the sequence path"""
    w, h, levels, scale = GEOMS[1]
    n = 3
    img, ok, od = _reference(oracle, w, h, levels, scale)
    c = _ctx(w, h, levels, scale, n)
    bufs = [c.dev_alloc(n * w * h * 3), c.dev_alloc(n * w * h * 2), c.dev_alloc(n * w * h * 3), c.dev_alloc(n * 128)]
    try:
        c.synth_frames_dev(SEED, 0, n, *bufs)                  # depth, semantics and poses of a synthetic sequence
        bgr = np.stack([np.repeat(img[:, :, None], 3, axis=2)] * n)
        assert np.array_equal(oracle.bgr2gray(bgr[0]), img)
        c.h2d(bufs[0], bgr)
        depth = c.d2h(bufs[1], (n, h, w), np.uint16)
        c.map_clear()
        out = c.seq_process(*bufs, n); c.sync()
        res = c.seq_fetch(out, n)
        for i in range(n):
            k = int(res["nkp"][i])
            _compare(oracle, res["kps"][i, :k], res["desc"][i, :k], res["pos3d"][i, :k], ok, od, depth[i])
    finally:
        for p in bufs:
            c.dev_free(p)
        c.close()
