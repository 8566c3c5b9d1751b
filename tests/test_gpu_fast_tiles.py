"""ORB on the fitted FAST tiles (build_geometry / fast_tile) against oracle/orb.c, byte for byte (keypoints, angles, descriptors, 3-D positions),
on geometries whose windows the tiles fit in different ways: the headline 640 x 480, KITTI's 1241 x 376, odd widths and heights, a tiny frame and
other scale factors.  The images:
  * synthetic frames;
  * low texture: 5 x 5 squares 12 levels above the background every 23 px plus 0/1 noise -- no corner reaches iniThFAST, so every keypoint comes
    from pass 2 (fast_need_kernel + fast_retry_kernel at minThFAST);
  * a patchwork of noise blocks on that low-texture image: cells with corners at iniThFAST next to empty ones inside one tile, so pass 2 runs on
    some cells of a tile only (the emptyrow mask);
  * noise: position lists longer than 512 per tile and many maxima per tile.
Single frames through ssm_orb_extract, and batches of 1, 3 and 250 frames through the sequence path.  The staging-overflow path runs the same tests
again in a subprocess with a 16-entry staging area.
  * plateaus: a cell whose only pixels above iniThFAST are the end of a 2-px-wide bar -- six pixels of one score, none of them a local maximum.  The cell
    maximum the quad-tree reads is the maximum over KEPT maxima, so that cell counts as empty at iniThFAST and is tried again at minThFAST, where a faint
    square beside the bar gives it a keypoint; once well inside a FAST tile, once with the tile boundary between the plateau's two columns."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import CAM, SEED

pytestmark = pytest.mark.gpu

INI = 20          # ssm_config_default's iniThFAST

GEOMS = [(640, 480, 8, 1.2), (1241, 376, 8, 1.2), (641, 479, 8, 1.2), (642, 482, 5, 1.2), (176, 88, 1, 1.2), (640, 480, 5, 1.5),
         (640, 480, 3, 2.0), (640, 480, 8, 1.1)]


def _low_texture(w, h, rng):
    img = np.full((h, w), 100, np.uint8)
    for y in range(0, h - 5, 23):
        for x in range(0, w - 5, 23):
            img[y:y + 5, x:x + 5] = 112
    return (img + rng.integers(0, 2, img.shape)).astype(np.uint8)


def _images(oracle, w, h):
    rng = np.random.default_rng(w * 31 + h)
    low = _low_texture(w, h, rng)
    patch = low.copy()
    for y in range(0, h, 72):
        for x in range((y // 72) % 2 * 48, w, 96):
            patch[y:y + 36, x:x + 36] = rng.integers(0, 256, patch[y:y + 36, x:x + 36].shape)
    noise = rng.integers(0, 256, (h, w), dtype=np.uint8)
    synth = oracle.bgr2gray(oracle.synth_frame(SEED, 2, w, h)[0])
    return [("synthetic", synth), ("low_texture", low), ("patchwork", patch), ("noise", noise)]


def _reference(oracle, images, levels, scale):
    ref = {}
    for name, img in images:
        ok, od = oracle.orb_extract(img, nfeatures=600, scale=scale, nlevels=levels)
        assert len(ok) > 0, name
        if name == "low_texture":                   # pass 2 made every keypoint
            assert ok["response"].max() < INI, ok["response"].max()
        if name == "patchwork":                     # both passes made keypoints
            assert ok["response"].max() >= INI and ok["response"].min() < INI
        ref[name] = (ok, od)
    return ref


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
def test_orb_on_fitted_fast_tiles_matches_oracle(oracle, w, h, levels, scale):
    images = _images(oracle, w, h)
    ref = _reference(oracle, images, levels, scale)
    depth = oracle.synth_frame(SEED, 2, w, h)[1]
    c = _ctx(w, h, levels, scale, 1)
    try:
        for name, img in images:
            gk, gd, gp = c.detect_features(img, depth)
            _compare(oracle, gk, gd, gp, *ref[name], depth)
    finally:
        c.close()


@pytest.mark.parametrize("w,h,levels,scale", [(641, 479, 8, 1.2), (1241, 376, 8, 1.2), (642, 482, 5, 1.2)])
@pytest.mark.parametrize("n", [1, 3, 250])
def test_batched_orb_on_fitted_fast_tiles_matches_oracle(oracle, w, h, levels, scale, n):
    """the sequence path: n frames per call (one ORB launch chain over the batch), frame i = image i % 4 as BGR, its own synthetic depth"""
    images = _images(oracle, w, h)
    ref = _reference(oracle, images, levels, scale)
    c = _ctx(w, h, levels, scale, n)
    bufs = [c.dev_alloc(n * w * h * 3), c.dev_alloc(n * w * h * 2), c.dev_alloc(n * w * h * 3), c.dev_alloc(n * 128)]
    try:
        c.synth_frames_dev(SEED, 0, n, *bufs)                  # depth, semantics and poses of a synthetic sequence
        bgr = np.stack([np.repeat(images[i % 4][1][:, :, None], 3, axis=2) for i in range(n)])
        assert all(np.array_equal(oracle.bgr2gray(bgr[i]), images[i % 4][1]) for i in range(4 if n >= 4 else n))
        c.h2d(bufs[0], bgr)
        depth = c.d2h(bufs[1], (n, h, w), np.uint16)
        c.map_clear()
        out = c.seq_process(*bufs, n); c.sync()
        res = c.seq_fetch(out, n)
        for i in range(n):
            k = int(res["nkp"][i])
            _compare(oracle, res["kps"][i, :k], res["desc"][i, :k], res["pos3d"][i, :k], *ref[images[i % 4][0]], depth[i])
    finally:
        for p in bufs:
            c.dev_free(p)
        c.close()


# ---- a plateau above iniThFAST: level 0 of 640 x 480 has cells of 31 x 32 positions from (19, 19) on
PLATEAU_W, PLATEAU_H, CELL_W, CELL_H = 640, 480, 31, 32
PLATEAU_SEED = 3              # the 0 / 1 noise around the squares decides which of their equal corners is a maximum: chosen on the CPU, asserted below


def _plateau_spots(c=None):
    """(cell column, cell row, the bar's first column, the square's first column): cell (1, 2) lies inside the first FAST tile; cell (7, 6) is cut by a tile
    boundary, and the bar stands on it: one column of the plateau in either tile"""
    import semantic_slam_mapping_amd as ssm
    cfg = ssm.default_config(width=PLATEAU_W, height=PLATEAU_H, orb_levels=8, orb_scale=1.2, orb_features=600, max_batch=1)
    lib, n = ssm.load(), ctypes.c_int(0)
    assert lib.ssm_debug_fast_plan(ctypes.byref(cfg), None, 0, ctypes.byref(n), None) == 0
    t = np.zeros((n.value, 16), np.int32)
    assert lib.ssm_debug_fast_plan(ctypes.byref(cfg), t.ctypes.data, n.value, ctypes.byref(n), None) == 0
    t = t[t[:, 0] == 0]
    assert (t[0, 13], t[0, 14]) == (PLATEAU_W, PLATEAU_H)
    xe = sorted(set(t[:, 1].tolist()) | set(t[:, 2].tolist()))          # the tiles' interiors are [x0, x1): column x1 - 1 and column x1 belong to different tiles
    inside, split = (1, 2, 70, 55), (7, 6, 260, 240)
    x0 = 19 + inside[0] * CELL_W
    assert not [e for e in xe if x0 - 1 <= e <= x0 + CELL_W]             # no tile edge in or beside the first cell
    x0 = 19 + split[0] * CELL_W
    assert split[2] + 1 in xe and x0 < split[2] and split[2] + 1 < x0 + CELL_W - 1
    return [inside, split]


def _plateau_image(spots):
    rng = np.random.default_rng(PLATEAU_SEED)
    img = _low_texture(PLATEAU_W, PLATEAU_H, rng)
    for cj, ci, bx, sx in spots:                                         # nothing but the bar and the square in the cell and 7 px around it
        x0, y0 = 19 + cj * CELL_W, 19 + ci * CELL_H
        img[y0 - 7:y0 + CELL_H + 7, x0 - 7:x0 + CELL_W + 7] = 100
    for cj, ci, bx, sx in spots:
        x0, y0 = 19 + cj * CELL_W, 19 + ci * CELL_H
        img[0:y0 + 12, bx:bx + 2] = 180                                  # the bar comes down from the top of the image and ends inside the cell
        img[y0 + 21:y0 + 26, sx:sx + 5] = 112                            # _low_texture's square, with its 0 / 1 noise
        img[y0 + 18:y0 + 29, sx - 3:sx + 8] += rng.integers(0, 2, (11, 11)).astype(np.uint8)
    return img


@pytest.fixture(scope="module")
def plateau(oracle):
    """the image, its oracle extraction, and the CPU proof that it is what the test is about"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import pyref
    spots = _plateau_spots()
    img = _plateau_image(spots)
    ok, od, stages = oracle.orb_extract(img, nfeatures=600, want_stages=True)
    k0 = ok[ok["octave"] == 0]
    for cj, ci, bx, sx in spots:
        x0, y0 = 19 + cj * CELL_W, 19 + ci * CELL_H
        S = np.array([[pyref.fast_S(img, x, y) for x in range(x0, x0 + CELL_W)] for y in range(y0, y0 + CELL_H)])
        ys, xs = np.nonzero(S > INI)
        # exactly a plateau: 2 x 3 pixels of one score at the bar's end ...
        assert sorted(zip((xs + x0).tolist(), (ys + y0).tolist())) == sorted((x, y) for x in (bx, bx + 1) for y in range(y0 + 9, y0 + 12)), (cj, ci)
        assert len(set(S[ys, xs].tolist())) == 1 and S[ys[0], xs[0]] == 80
        for y, x in zip(ys, xs):                                         # ... none of them above all its neighbours in the cell
            nb = [S[yy, xx] for yy in range(y - 1, y + 2) for xx in range(x - 1, x + 2) if (yy, xx) != (y, x)]
            assert max(nb) >= S[y, x]
        inc = k0[(k0["x"] >= x0) & (k0["x"] < x0 + CELL_W) & (k0["y"] >= y0) & (k0["y"] < y0 + CELL_H)]
        assert len(inc) >= 1 and inc["response"].max() < INI, (cj, ci)   # the cell's keypoints come from the pass at minThFAST
        c = stages[0]["cand"]
        assert ((c[:, 0] >= x0) & (c[:, 0] < x0 + CELL_W) & (c[:, 1] >= y0) & (c[:, 1] < y0 + CELL_H) & (c[:, 2] >= INI)).sum() == 0
    return img, ok, od


def test_fast_plateau_cell_is_retried_at_the_minimum_threshold(oracle, plateau):
    img, ok, od = plateau
    depth = oracle.synth_frame(SEED, 2, PLATEAU_W, PLATEAU_H)[1]
    c = _ctx(PLATEAU_W, PLATEAU_H, 8, 1.2, 1)
    try:
        gk, gd, gp = c.detect_features(img, depth)
        _compare(oracle, gk, gd, gp, ok, od, depth)
    finally:
        c.close()


def test_fast_plateau_cell_inside_a_sequence_batch(oracle, plateau):
    img, ok, od = plateau
    w, h, n = PLATEAU_W, PLATEAU_H, 3
    low = _low_texture(w, h, np.random.default_rng(9))
    lk, ld = oracle.orb_extract(low, nfeatures=600)
    frames = [(img, ok, od), (low, lk, ld), (img, ok, od)]
    c = _ctx(w, h, 8, 1.2, n)
    bufs = [c.dev_alloc(n * w * h * 3), c.dev_alloc(n * w * h * 2), c.dev_alloc(n * w * h * 3), c.dev_alloc(n * 128)]
    try:
        c.synth_frames_dev(SEED, 0, n, *bufs)
        bgr = np.stack([np.repeat(f[0][:, :, None], 3, axis=2) for f in frames])
        assert all(np.array_equal(oracle.bgr2gray(bgr[i]), frames[i][0]) for i in range(n))
        c.h2d(bufs[0], bgr)
        depth = c.d2h(bufs[1], (n, h, w), np.uint16)
        c.map_clear()
        out = c.seq_process(*bufs, n); c.sync()
        res = c.seq_fetch(out, n)
        for i in range(n):
            k = int(res["nkp"][i])
            _compare(oracle, res["kps"][i, :k], res["desc"][i, :k], res["pos3d"][i, :k], frames[i][1], frames[i][2], depth[i])
    finally:
        for p in bufs:
            c.dev_free(p)
        c.close()


def test_fast_tiles_stage_overflow_path_in_subprocess():
    """the per-candidate global path of tiles with more maxima than the staging area holds, forced with SSM_FAST_STAGE_CAP=16"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SSM_FAST_STAGE_CAP="16")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_fast_tiles.py"), "-x", "-q", "-m", "gpu",
                        "-k", "matches_oracle and not 250"], capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in r.stdout and "deselected" in r.stdout
