"""The fused pyramid's level loop (8 pixels x 4 rows per item, each source row's horizontal pass shared by the output rows that blend it; the
4-pixel item on levels whose groups do not fit four dwords) against gray_kernel + one resize launch per level: whole pyramid buffers, byte for
byte (ssm_debug_pyramid: bands < 0 runs the per-level launches, 0 what the ORB calls run, > 0 the fused kernel at that band count).  Geometries
and scale factors are those of tests/test_pyramid_items.py, so both items run -- at scale 1.5 inside one launch; BGR and gray input; batches of
1, 3 and 250; band counts whose halos span several bands.  The constructed images aim at a wrong row reuse: a shared source row taken from the
wrong output row shows wherever neighbouring source rows differ, which random frames test everywhere and the patterns test in isolation
(one odd row among constant rows, 1-pixel stripes both ways, distinct last rows for the min(syA + 1, sh - 1) clamp)."""
import ctypes as C

import numpy as np
import pytest

from conftest import CAM

pytestmark = pytest.mark.gpu

SIZES = [(640, 480), (1241, 376), (644, 484), (642, 482), (176, 88)]
SCALES = [1.1, 1.2, 1.25, 1.3, 1.5]
BANDS = [1, 7, 8, 32, 40, 64]


def _plan(w, h, levels, scale, bands):
    """(band count of the fused plan or 0, mask of the levels that run the 8-pixel item), None where the configuration is refused: host only"""
    import semantic_slam_mapping_amd as ssm
    from semantic_slam_mapping_amd._lib import Config
    lib = ssm.load()
    cfg = Config()
    lib.ssm_config_default(C.byref(cfg))
    cfg.width, cfg.height, cfg.orb_levels, cfg.orb_scale, cfg.orb_features = w, h, levels, scale, 600
    n = C.c_int(0)
    limits = np.zeros(16 + 3 * 12, np.int32)
    if lib.ssm_debug_pyramid_plan(C.byref(cfg), bands, None, 0, C.byref(n), None, limits.ctypes.data) != 0:
        return None
    return int(limits[0]), int(limits[9])


def _levels(w, h, scale):
    """the most levels (<= 8) the configuration is accepted with"""
    return max(lv for lv in range(1, 9) if _plan(w, h, lv, scale, 0) is not None)


def _ctx(w, h, levels, scale, batch):
    import semantic_slam_mapping_amd as ssm
    return ssm.Context(0, width=w, height=h, orb_levels=levels, orb_scale=scale, orb_features=600, max_batch=batch, voxel_capacity_log2=12, camera=CAM)


def _pyramid(c, img, bands):
    n = img.shape[0]; ch = 1 if img.ndim == 3 else 3
    img = np.ascontiguousarray(img, np.uint8)
    nbytes = C.c_int(0)
    c._chk(c.lib.ssm_debug_pyramid(c.h, None, ch, n, bands, None, C.byref(nbytes)))
    out = np.zeros((n, nbytes.value), np.uint8)
    c._chk(c.lib.ssm_debug_pyramid(c.h, img.ctypes.data, ch, n, bands, out.ctypes.data, C.byref(nbytes)))
    return out


def _patterns(w, h, rng):
    """gray images (h, w) built to catch a wrong row reuse"""
    out = []
    a = np.full((h, w), 40, np.uint8); a[h // 2] = 250; a[7] = 0; out.append(a)                       # constant rows, one odd row (two places)
    a = np.zeros((h, w), np.uint8); a[::2] = 255; out.append(a)                                       # horizontal 1-pixel stripes
    a = np.zeros((h, w), np.uint8); a[:, ::2] = 255; out.append(a)                                    # vertical 1-pixel stripes
    a = np.repeat(((np.arange(h) * 37) % 251).astype(np.uint8)[:, None], w, 1); out.append(a)         # every row its own constant
    a = np.full((h, w), 128, np.uint8); a[-6:] = rng.integers(0, 256, (6, w), dtype=np.uint8); out.append(a)   # distinct last rows (the clamp)
    a = np.zeros((h, w), np.uint8); a[-1] = 255; a[:, -1] = 255; out.append(a)                        # last row and last column alone
    return out


def _inputs(w, h, n, gray, rng):
    pats = _patterns(w, h, rng)
    frames = []
    for i in range(n):
        if i % 2 == 0 or n == 1:
            g = pats[(i // 2) % len(pats)] if n > 1 else None
        else:
            g = None
        if g is None:
            frames.append(rng.integers(0, 256, (h, w) if gray else (h, w, 3), dtype=np.uint8))
        else:
            frames.append(g if gray else np.stack([g, np.roll(g, 1, 0), g], -1))                      # (channels differ: the conversion is not a copy)
    return np.stack(frames)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("w,h", SIZES)
def test_fused_rows_match_per_level_launches(w, h, scale):
    levels = _levels(w, h, scale)
    rng = np.random.default_rng(w * 31 + h * 17 + int(scale * 100))
    c = _ctx(w, h, levels, scale, 7)
    try:
        for gray in (False, True):
            imgs = [_inputs(w, h, 1, gray, rng), _inputs(w, h, 3, gray, rng)]
            pats = _patterns(w, h, rng)
            imgs.append(np.stack(pats) if gray else np.stack([np.stack([g, np.roll(g, 1, 0), g], -1) for g in pats]))
            imgs.append(imgs[-1][1:2])                                                                # a pattern through the one-frame plan
            for img in imgs:
                n = img.shape[0]
                ref = _pyramid(c, img, -1)
                assert not np.array_equal(ref, np.full_like(ref, 0xA5))
                for bands in [0] + BANDS:
                    fused = _plan(w, h, levels, scale, bands if bands else (0 if n > 1 else -1))
                    if fused[0] == 0:                          # no fused form at this count: the explicit request is refused, the default runs the per-level launches
                        if bands:
                            with pytest.raises(Exception, match="no fused pyramid"):
                                _pyramid(c, img, bands)
                            continue
                    got = _pyramid(c, img, bands)
                    assert np.array_equal(got, ref), (gray, n, bands, hex(fused[1]), np.flatnonzero((got != ref).any(0))[:8])
    finally:
        c.close()


def test_both_items_run_in_this_sweep():
    """host only: the sweep above runs the 8-pixel item and the 4-pixel item, and one launch with both"""
    masks = {}
    for w, h in SIZES:
        for s in SCALES:
            lv = _levels(w, h, s)
            nb, wide = _plan(w, h, lv, s, 8)
            if nb:
                masks[(w, h, s)] = (wide, (1 << lv) - 2)
    assert any(m == full and full for m, full in masks.values())                   # every level wide
    assert any(m == 0 and full for m, full in masks.values())                      # every level narrow
    assert any(0 < m < full for m, full in masks.values())                         # both in one launch
    assert masks[(640, 480, 1.2)] == (0xFE, 0xFE)


@pytest.mark.parametrize("scale", [1.2, 1.5])
@pytest.mark.parametrize("gray", [False, True])
def test_fused_rows_full_batch(gray, scale):
    w, h = 640, 480
    levels = _levels(w, h, scale)
    rng = np.random.default_rng(250 + gray)
    c = _ctx(w, h, levels, scale, 250)
    try:
        base = _inputs(w, h, 14, gray, rng)
        img = np.concatenate([base] * 18)[:250]
        ref = _pyramid(c, img, -1)
        got = _pyramid(c, img, 0)
        assert np.array_equal(got, ref), np.flatnonzero((got != ref).any(1))[:8]
    finally:
        c.close()
