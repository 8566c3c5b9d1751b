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
again in a subprocess with a 16-entry staging area."""
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


def test_fast_tiles_stage_overflow_path_in_subprocess():
    """the per-candidate global path of tiles with more maxima than the staging area holds, forced with SSM_FAST_STAGE_CAP=16"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SSM_FAST_STAGE_CAP="16")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_fast_tiles.py"), "-x", "-q", "-m", "gpu",
                        "-k", "matches_oracle and not 250"], capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in r.stdout and "deselected" in r.stdout
