"""The fused pyramid's work items (resize4_kernel_bands), read on the host through ssm_debug_pyramid_plan: no GPU.  The entry lists the items of
every (band, level) with the decomposition the kernel itself uses (pyr_items / pyr_item_run in csrc/ssm_orb_plan.h; the plan itself is csrc/ssm_orb_plan.cpp).  For each geometry, level count,
band count and scale factor: the items of a (band, level) cover each (comp row, column group) exactly once; every source row an item reads lies
inside the band's comp rows of the level below; every LDS byte its windows read, and every byte it writes, lies inside the level buffer the plan
allocates, and the windows do hold the pixels the x tables point at; a level is given the 8-pixel item exactly where every 8-pixel group fits
four dwords (checked here from the resize offsets, computed without the library), the 4-pixel item otherwise.  Both items must occur among the
fused plans, and so must geometries without a fused plan: a run that only ever saw one path fails."""
import ctypes as C

import numpy as np
import pytest

SIZES = [(640, 480), (1241, 376), (644, 484), (642, 482), (176, 88)]
SCALES = [1.1, 1.2, 1.25, 1.3, 1.5]
BANDS = [1, 7, 8, 32, 40, 64]
MAX_LEVELS = 12
SEEN = {}          # (w, h, scale) -> set of what its plans showed: 4, 8 (pixels per item of a fused level), "none" (no fused plan)


def _plan(w, h, levels, scale, bands):
    import semantic_slam_mapping_amd as ssm
    lib = ssm.load()
    from semantic_slam_mapping_amd._lib import Config
    cfg = Config()
    lib.ssm_config_default(C.byref(cfg))
    cfg.width, cfg.height, cfg.orb_levels, cfg.orb_scale, cfg.orb_features = w, h, levels, scale, 600
    n = C.c_int(0)
    limits = np.zeros(16 + 3 * MAX_LEVELS, np.int32)
    rc = lib.ssm_debug_pyramid_plan(C.byref(cfg), bands, None, 0, C.byref(n), None, limits.ctypes.data)
    if rc != 0:
        return None                                   # the configuration itself is refused (levels too small for ORB)
    items = np.zeros((n.value, 12), np.int32)
    tab = np.zeros((max(int(limits[0]), 1), levels, 4), np.int32)
    if limits[0]:
        assert lib.ssm_debug_pyramid_plan(C.byref(cfg), bands, items.ctypes.data, len(items), C.byref(n), tab.ctypes.data, None) == 0
        assert n.value == len(items)
    if len(items):
        assert lib.ssm_debug_pyramid_plan(C.byref(cfg), bands, items.ctypes.data, n.value - 1, C.byref(n), None, None) != 0
    return items, tab, limits


def _offsets(ssize, dsize):
    """cv::resize INTER_LINEAR source offsets (the left neighbour of every destination pixel)"""
    d = np.arange(dsize, dtype=np.float64)
    f = ((d + 0.5) * (1.0 / (dsize / ssize)) - 0.5).astype(np.float32)
    return np.clip(np.floor(f).astype(np.int64), 0, ssize - 1)


def _fits(xo, px):
    """every group of px pixels: each pixel's pair (offset, offset + 1) inside the 8 bytes of its dword pair, counted from the first pixel's offset"""
    for x0 in range(0, len(xo), px):
        off = xo[x0:x0 + px] - xo[x0]
        off[4:] -= 4
        if (off < 0).any() or (off > 6).any():
            return False
    return True


def test_plan_rejects_bad_arguments():
    import semantic_slam_mapping_amd as ssm
    lib = ssm.load()
    n = C.c_int(0)
    assert lib.ssm_debug_pyramid_plan(None, 8, None, 0, C.byref(n), None, None) != 0
    from semantic_slam_mapping_amd._lib import Config
    cfg = Config()
    lib.ssm_config_default(C.byref(cfg))
    assert lib.ssm_debug_pyramid_plan(C.byref(cfg), 8, None, 0, None, None, None) != 0


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("w,h", SIZES)
def test_items_cover_each_level_once_inside_lds(w, h, scale):
    seen = SEEN.setdefault((w, h, scale), set())
    accepted = 0
    for levels in range(1, 9):
        for bands in BANDS:
            got = _plan(w, h, levels, scale, bands)
            if got is None:
                continue
            accepted += 1
            items, tab, limits = got
            nb, lds, buf1, slack, threads, max_lds, nl, has4, fits8, wide = (int(v) for v in limits[:10])
            assert nl == levels
            geo = [tuple(int(v) for v in limits[16 + 3 * l:19 + 3 * l]) for l in range(levels)]
            xo = [None] + [_offsets(geo[l - 1][0], geo[l][0]) for l in range(1, levels)]
            yo = [None] + [_offsets(geo[l - 1][1], geo[l][1]) for l in range(1, levels)]
            # the layout checks, from the offsets alone
            for l in range(1, levels):
                assert bool(has4 >> l & 1) == _fits(xo[l], 4), (levels, l)
                assert bool(fits8 >> l & 1) == (_fits(xo[l], 4) and _fits(xo[l], 8)), (levels, l)
            if nb == 0:                                # no fused plan: a level needs the general resize kernel, too few rows, or too much LDS
                assert len(items) == 0
                seen.add("none")
                continue
            assert nb == bands and all(has4 >> l & 1 for l in range(1, levels))
            assert wide == fits8                       # a level that fails the 8-pixel layout keeps the 4-pixel item, every other level is wide
            assert lds <= max_lds and buf1 % 16 == 0 and 0 < buf1 <= lds
            cap = (buf1, lds - buf1)                   # bytes of the even / odd levels' buffer
            # band rows: own rows partition each level; comp rows hold them and the source rows of the comp rows above
            for l in range(levels):
                lh = geo[l][1]
                assert tab[0, l, 2] == 0 and tab[nb - 1, l, 3] == lh - 1
                assert (tab[1:, l, 2] == tab[:-1, l, 3] + 1).all() and (tab[:, l, 2] <= tab[:, l, 3]).all()
                assert (tab[:, l, 0] <= tab[:, l, 2]).all() and (tab[:, l, 1] >= tab[:, l, 3]).all()
                assert (tab[:, l, 0] >= 0).all() and (tab[:, l, 1] < lh).all()
                assert ((tab[:, l, 1] - tab[:, l, 0] + 1) * geo[l][2] + slack <= cap[l & 1]).all()
            assert (items[:, 0] >= 1).all() and (items[:, 0] < levels).all() and (items[:, 1] >= 0).all() and (items[:, 1] < nb).all()
            for l in range(1, levels):
                IL = items[items[:, 0] == l]
                (sw, sh, sstride), (dw, dh, dstride) = geo[l - 1], geo[l]
                px = 8 if wide >> l & 1 else 4
                seen.add(px)
                assert (IL[:, 2] == px).all()
                groups = dstride // px
                b, gi, ylo, yhi, slo, shi, rlo, rhi, wlo, whi = (IL[:, k].astype(np.int64) for k in (1, 3, 4, 5, 6, 7, 8, 9, 10, 11))
                clo, chi = tab[b, l, 0].astype(np.int64), tab[b, l, 1].astype(np.int64)
                plo, phi = tab[b, l - 1, 0].astype(np.int64), tab[b, l - 1, 1].astype(np.int64)
                assert (gi >= 0).all() and (gi < groups).all()
                assert (ylo <= yhi).all() and (yhi - ylo < 4).all() and (ylo >= clo).all() and (yhi <= chi).all()
                # each (comp row, column group) exactly once
                off = np.concatenate([[0], np.cumsum((tab[:, l, 1] - tab[:, l, 0] + 1).astype(np.int64) * groups)])
                count = np.zeros(off[-1], np.int32)
                for j in range(4):
                    m = ylo + j <= yhi
                    np.add.at(count, off[b[m]] + (ylo[m] + j - clo[m]) * groups + gi[m], 1)
                assert (count == 1).all(), (levels, bands, l, np.flatnonzero(count != 1)[:8])
                # the source rows: those the y offsets name, inside the band's comp rows of the level below
                assert (slo == yo[l][ylo]).all() and (shi == np.minimum(yo[l][yhi] + 1, sh - 1)).all()
                assert (slo >= plo).all() and (shi <= phi).all()
                # the windows: inside the source level's buffer, and holding each pixel's pair of the first and the last source row
                assert (rlo >= 0).all() and (rhi <= cap[(l - 1) & 1]).all() and (rlo % 4 == 0).all()
                x0 = px * gi
                real = x0 < dw
                x1 = np.minimum(x0 + px, dw) - 1
                first, last = xo[l][np.where(real, x0, 0)], xo[l][np.where(real, x1, 0)]
                assert (rlo[real] <= (slo - plo)[real] * sstride + first[real]).all()
                assert (rhi[real] >= (shi - plo)[real] * sstride + last[real] + 2).all()
                assert (rhi - rlo == (shi - slo) * sstride + (16 if px == 8 else 12)).all()
                # the stores: the item's px bytes of each of its rows, inside the level's own buffer
                assert (wlo == (ylo - clo) * dstride + px * gi).all() and (whi == (yhi - clo) * dstride + px * gi + px).all()
                assert (wlo >= 0).all() and (whi <= cap[l & 1] - slack).all()
    assert accepted > 0


def test_both_items_and_unfused_geometries_were_seen():
    """(after the sweep above, in file order) the sweep's fused plans used the 8-pixel item and the 4-pixel item, and some geometry had no
    fused plan: scale 1.2 (ORB's) must be wide on every level, scale 1.5 narrow on some"""
    if len(SEEN) < len(SIZES) * len(SCALES):
        for w, h in SIZES:
            for s in SCALES:
                if (w, h, s) not in SEEN:
                    test_items_cover_each_level_once_inside_lds(w, h, s)
    allseen = set().union(*SEEN.values())
    assert {4, 8, "none"} <= allseen, allseen
    assert 4 not in SEEN[(640, 480, 1.2)] and 8 in SEEN[(640, 480, 1.2)]
    assert 4 in set().union(*(SEEN[(w, h, 1.5)] for w, h in SIZES))
