"""The blurred pyramid of the ORB front end on every pixel: blur_mfma_kernel (the default) and blur_kernel (SSM_BLUR_VARIANT=0) read back through
ssm_debug_orb_blur, which un-tiles the device layout on the host, against oracle.gaussian7 of every level of the DEVICE pyramid (ssm_debug_pyramid; the resize
has its own tests).  Every pixel [0, w) x [0, h) of every level must be equal, the padding columns [w, stride) zero, and the two variants
equal each other byte for byte.  Geometries: strides with a partial dword, a half-filled 32-column unit and a strip with one active wave; heights of exactly
two 58-row steps, one row more, and a last step shorter than its 6-row halo; one column past a strip at the smallest level the planner accepts.  Images:
noise, the extremes 0 / 255 flat, as checkerboards and as stripes (the row sums and both byte planes of the second matrix product at their ends), and single
pixels at every corner, border middle, 58-row seam and 128-column seam, one at a time, so that a wrong tap or a wrong reflection shows alone."""
import numpy as np
import pytest

import orb_describe_ref as R
from conftest import CAM

pytestmark = pytest.mark.gpu

# (w, h, levels)
GEOMS = [(640, 480, 8), (1241, 376, 8), (644, 484, 8), (642, 482, 5), (176, 116, 1), (176, 117, 1), (176, 121, 1), (176, 88, 1), (129, 76, 1)]
BATCHES = (1, 3, 9)


def _images(w, h):
    """[(name, gray image)]"""
    rng = np.random.default_rng(w * 5 + h)
    yy, xx = np.mgrid[0:h, 0:w]
    out = [("random", rng.integers(0, 256, (h, w), dtype=np.uint8)), ("zeros", np.zeros((h, w), np.uint8)), ("full", np.full((h, w), 255, np.uint8)),
           ("checker1", (((xx + yy) & 1) * 255).astype(np.uint8)), ("checker2", ((((xx >> 1) + (yy >> 1)) & 1) * 255).astype(np.uint8)),
           ("rows", ((yy & 1) * 255).astype(np.uint8)), ("columns", ((xx & 1) * 255).astype(np.uint8)),
           ("rows_inv", (((yy + 1) & 1) * 255).astype(np.uint8)), ("columns_inv", (((xx + 1) & 1) * 255).astype(np.uint8))]
    spots = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, 0), (w // 2, h - 1), (0, h // 2), (w - 1, h // 2)]
    spots += [(w // 2 - 7, y) for y in (57, 58, 59)] + [(x, h // 2 + 3) for x in (127, 128)]       # a row seam alone, a column seam alone ...
    spots += [(x, y) for y in (57, 58, 59) for x in (127, 128, w - 1)]                             # ... and where they meet
    for x, y in dict.fromkeys(spots):
        a = np.zeros((h, w), np.uint8); a[y, x] = 255; out.append(("one_255_at_%d_%d" % (x, y), a))
        a = np.full((h, w), 255, np.uint8); a[y, x] = 0; out.append(("one_0_at_%d_%d" % (x, y), a))
    out.append(("random2", rng.integers(0, 256, (h, w), dtype=np.uint8)))
    return out


def _batches(n):
    """the images dealt into calls of 1, 3 and 9 frames, every size at least once"""
    out, i, k = [], 0, 0
    while i < n:
        b = min(BATCHES[min(k, 2)], n - i)
        out.append((i, i + b)); i += b; k += 1
    assert {b - a for a, b in out} >= set(BATCHES)
    return out


def _blurred(monkeypatch, variant, w, h, levels, imgs):
    """(pyramids, blurred pyramids) of all images, through calls of 1, 3 and 9 frames on a context of that blur variant"""
    import semantic_slam_mapping_amd as ssm
    monkeypatch.setenv("SSM_BLUR_VARIANT", str(variant))
    c = ssm.Context(0, width=w, height=h, orb_levels=levels, orb_features=R.NFEAT, max_batch=9, voxel_capacity_log2=12, camera=CAM)
    try:
        pyr, blur = [], []
        for a, b in _batches(len(imgs)):
            batch = np.stack(imgs[a:b])
            blur.append(c.debug_orb_blur(batch)); pyr.append(c.debug_pyramid(batch))
        return np.concatenate(pyr), np.concatenate(blur)
    finally:
        c.close()


@pytest.mark.parametrize("w,h,levels", GEOMS)
def test_blur_of_every_pixel_matches_gaussian7(oracle, monkeypatch, w, h, levels):
    geom = R.geometry(w, h, levels, R.NFEAT)
    named = _images(w, h)
    names, imgs = [n for n, _ in named], [a for _, a in named]
    got = {}
    for variant in (1, 0):
        pyr, blur = _blurred(monkeypatch, variant, w, h, levels, imgs)
        assert pyr.shape == blur.shape == (len(imgs), R.pyramid_bytes(geom))
        got[variant] = blur
        for f in range(len(imgs)):
            for l, (L, src, out) in enumerate(zip(geom, R.level_views(pyr[f], geom), R.level_views(blur[f], geom))):
                if l == 0:
                    assert np.array_equal(src[:, :L.w], imgs[f])
                ref = oracle.gaussian7(src[:, :L.w])
                bad = np.argwhere(out[:, :L.w] != ref)
                assert not len(bad), "variant %d: first difference at (frame %d %s, level %d, x %d, y %d): %d, expected %d; %d pixels of the level differ" % (
                    variant, f, names[f], l, bad[0][1], bad[0][0], out[bad[0][0], bad[0][1]], ref[bad[0][0], bad[0][1]], len(bad))
                pad = np.argwhere(out[:, L.w:] != 0)
                assert not len(pad), "variant %d: padding column not zero at (frame %d %s, level %d, x %d, y %d)" % (variant, f, names[f], l, L.w + pad[0][1], pad[0][0])
    assert np.array_equal(got[0], got[1])
