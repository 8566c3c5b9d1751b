"""The fused pyramid kernel (resize4_kernel_bands: gray + every level in one launch, one block per horizontal band of a frame) against gray_kernel +
one resize launch per level: the whole pyramid buffer of every frame, byte for byte -- row padding and the borders FAST never looks at included
(ssm_debug_pyramid: bands < 0 runs the per-level launches, 0 what the ORB calls run, > 0 the fused kernel at that band count).  Then ORB end to end
against oracle/orb.c on the same geometries."""
import ctypes as C

import numpy as np
import pytest

from conftest import CAM, SEED

pytestmark = pytest.mark.gpu


def _ctx(w, h, levels, batch):
    import semantic_slam_mapping_amd as ssm
    return ssm.Context(0, width=w, height=h, orb_levels=levels, orb_features=600, max_batch=batch, voxel_capacity_log2=12, camera=CAM)


def _pyramid(c, img, bands):
    n = img.shape[0]; ch = 1 if img.ndim == 3 else 3
    img = np.ascontiguousarray(img, np.uint8)
    nbytes = C.c_int(0)
    c._chk(c.lib.ssm_debug_pyramid(c.h, None, ch, n, bands, None, C.byref(nbytes)))         # the size of one frame's buffer
    out = np.zeros((n, nbytes.value), np.uint8)
    c._chk(c.lib.ssm_debug_pyramid(c.h, img.ctypes.data, ch, n, bands, out.ctypes.data, C.byref(nbytes)))
    return out


def _frames(oracle, w, h, n, gray):
    rng = np.random.default_rng(w * 7 + h * 13 + n)
    out = []
    for i in range(n):
        bgr = oracle.synth_frame(SEED, i % 8, w, h)[0] if i < 8 else rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        out.append(oracle.bgr2gray(bgr) if gray else bgr)
    return np.stack(out)


# (w, h, levels): the headline 640 x 480; KITTI's 1241 x 376; widths that are not multiples of 16 (644) or of 4 (642, 1241); a tiny frame
GEOMS = [(640, 480, 8), (1241, 376, 8), (644, 484, 8), (642, 482, 5), (640, 480, 1), (640, 480, 2), (176, 88, 1)]


@pytest.mark.parametrize("w,h,levels", GEOMS)
@pytest.mark.parametrize("gray", [False, True])
def test_fused_pyramid_matches_per_level_launches(oracle, w, h, levels, gray):
    c = _ctx(w, h, levels, 3)
    try:
        for n in (1, 3):
            img = _frames(oracle, w, h, n, gray)
            ref = _pyramid(c, img, -1)
            assert not np.array_equal(ref, np.full_like(ref, 0xA5))
            got = _pyramid(c, img, 0)
            assert np.array_equal(got, ref), (n, np.flatnonzero((got != ref).any(0))[:8])
            # band counts: one band (no halo), a few, and so many that a band's halo spans several bands
            for bands in (1, 7, 40, 64):
                try:
                    got = _pyramid(c, img, bands)
                except Exception as e:          # fewer rows than bands at the coarsest level, or level buffers too large for one block
                    assert "no fused pyramid" in str(e), e
                    continue
                assert np.array_equal(got, ref), (n, bands, np.flatnonzero((got != ref).any(0))[:8])
    finally:
        c.close()


@pytest.mark.parametrize("gray", [False, True])
def test_fused_pyramid_full_batch(oracle, gray):
    c = _ctx(640, 480, 8, 250)
    try:
        img = _frames(oracle, 640, 480, 250, gray)
        ref = _pyramid(c, img, -1)
        got = _pyramid(c, img, 0)
        assert np.array_equal(got, ref), np.flatnonzero((got != ref).any(1))[:8]
    finally:
        c.close()


@pytest.mark.parametrize("w,h,levels", [g for g in GEOMS if g[:2] != (640, 480)])
def test_orb_on_fused_pyramid_matches_oracle(oracle, w, h, levels):
    c = _ctx(w, h, levels, 1)
    try:
        for i in (0, 3):
            bgr = oracle.synth_frame(SEED, i, w, h)[0]
            for img in (bgr, oracle.bgr2gray(bgr)):
                gk, gd, _ = c.detect_features(img)
                ok, od = oracle.orb_extract(oracle.bgr2gray(bgr), nfeatures=600, nlevels=levels)
                assert len(gk) == len(ok)
                for f in ("x", "y", "size", "response", "octave", "class_id", "angle"):
                    assert np.array_equal(gk[f], ok[f]), f
                assert np.array_equal(gd, od)
    finally:
        c.close()
