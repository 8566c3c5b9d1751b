"""The FAST tile plan (build_geometry in csrc/ssm_orb_plan.cpp: tiles fitted to each level's FAST window), read on the host through ssm_debug_fast_plan: no GPU.
For each geometry: every position of every level's window [19, w - 19) x [19, h - 19) lies in exactly one tile interior and is quick-tested
by it; the scored rectangles are the interiors plus their NMS neighbours inside the window; no scored rectangle touches more than 8 x 8 cells;
each tile fits the kernel's LDS arrays; no scored position reads a staged word that was clamped.  The LDS the built FAST kernels take is read
from the gfx950 code object inside libssm_hip.so (kernel descriptors), not from a formula."""
import ctypes as C
import struct

import numpy as np
import pytest

EDGE = 19
LDS_BUDGET = 19968          # fast_kernel's LDS before the fitted plan
LDS_PER_CU = 160 * 1024     # 8 blocks (32 waves) per CU need <= 20480 B each

# (w, h, levels, scale factor): the headline 640 x 480; KITTI's 1241 x 376; odd widths and heights; a tiny frame; the scale factors and level
# counts of the ORB tests with other scale factors
GEOMS = [(640, 480, 8, 1.2), (1241, 376, 8, 1.2), (644, 484, 8, 1.2), (642, 482, 5, 1.2), (641, 479, 8, 1.2), (176, 88, 1, 1.2),
         (640, 480, 1, 1.2), (640, 480, 2, 1.2), (640, 480, 5, 1.5), (640, 480, 3, 2.0), (640, 480, 8, 1.1), (1241, 376, 5, 1.3)]


def _plan(w, h, levels, scale):
    import semantic_slam_mapping_amd as ssm
    lib = ssm.load()
    from semantic_slam_mapping_amd._lib import Config
    cfg = Config()
    lib.ssm_config_default(C.byref(cfg))
    cfg.width, cfg.height, cfg.orb_levels, cfg.orb_scale, cfg.orb_features = w, h, levels, scale, 600
    n = C.c_int(0)
    limits = np.zeros(6, np.int32)
    assert lib.ssm_debug_fast_plan(C.byref(cfg), None, 0, C.byref(n), limits.ctypes.data) == 0
    tiles = np.zeros((n.value, 16), np.int32)
    assert lib.ssm_debug_fast_plan(C.byref(cfg), tiles.ctypes.data, n.value, C.byref(n), None) == 0
    if n.value > 1:
        assert lib.ssm_debug_fast_plan(C.byref(cfg), tiles.ctypes.data, n.value - 1, C.byref(n), None) != 0
    return tiles, limits


def test_plan_rejects_bad_arguments():
    import semantic_slam_mapping_amd as ssm
    lib = ssm.load()
    n = C.c_int(0)
    assert lib.ssm_debug_fast_plan(None, None, 0, C.byref(n), None) != 0
    from semantic_slam_mapping_amd._lib import Config
    cfg = Config()
    lib.ssm_config_default(C.byref(cfg))
    cfg.orb_levels = 0
    assert lib.ssm_debug_fast_plan(C.byref(cfg), None, 0, C.byref(n), None) != 0


@pytest.mark.parametrize("w,h,levels,scale", GEOMS)
def test_fast_tiles_cover_each_window_once(w, h, levels, scale):
    tiles, limits = _plan(w, h, levels, scale)
    lds, max_groups, max_rows, pw, ph, stage = (int(v) for v in limits)
    assert lds <= LDS_BUDGET                          # the arrays fast_tile declares (the built kernels: test_built_fast_kernels_lds)
    assert stage * 8 <= pw * ph                       # the candidate staging area reuses the pixel tile
    assert sorted(set(tiles[:, 0])) == list(range(levels))
    for l in range(levels):
        T = tiles[tiles[:, 0] == l]
        lw, lh, stride = (int(v) for v in T[0, 13:16])
        interior = np.zeros((lh, lw), np.int32)
        tested = np.zeros((lh, lw), np.int32)
        for (_, x0, x1, y0, y1, xs0, xs1, ys0, ys1, groups, rows, ncx, ncy, _, _, _) in T.tolist():
            assert EDGE <= x0 < x1 <= lw - EDGE and EDGE <= y0 < y1 <= lh - EDGE
            interior[y0:y1, x0:x1] += 1
            # the scored rectangle: interior + 1 on each side, clipped to the window
            assert (xs0, xs1, ys0, ys1) == (max(x0 - 1, EDGE), min(x1 + 1, lw - EDGE), max(y0 - 1, EDGE), min(y1 + 1, lh - EDGE))
            tested[ys0:ys1, xs0:xs1] += 1
            # work items: 4-column groups from xs0 on, only the last one partly outside
            assert groups == (xs1 - xs0 + 3) // 4 and 4 * groups - (xs1 - xs0) < 4 and rows == ys1 - ys0
            assert 1 <= groups <= max_groups and 1 <= rows <= max_rows
            # cells: ORBextractor's grid over [EDGE - 3, w - EDGE + 3), counted from EDGE (the same numbers, derived here without the library)
            width, height = lw - 2 * EDGE + 6, lh - 2 * EDGE + 6
            wcell, hcell = -(-width // (width // 30)), -(-height // (height // 30))
            assert (ncx, ncy) == ((xs1 - 1 - EDGE) // wcell - (xs0 - EDGE) // wcell + 1, (ys1 - 1 - EDGE) // hcell - (ys0 - EDGE) // hcell + 1)
            assert ncx <= 8 and ncy <= 8                # (cells are >= 30 px, so in practice <= 6 x 3)
            # staged pixels: rows [ys0 - 3, ys0 + rows + 3), nine 16-byte words from xs0 - 4 on; a word is clamped when it would leave the row.  The
            # ring of the scored positions reaches 3 pixels, the quick test's dwords 4 past the last position of a group
            assert rows + 6 <= ph and 4 * groups + 8 <= pw
            assert ys0 - 3 >= 0 and ys1 + 2 <= lh - 1
            assert xs0 - 4 >= 0
            reads_to = xs1 - 1 + 3                      # the last pixel a scored position reads
            word = (reads_to - (xs0 - 4)) // 16
            assert xs0 - 4 + 16 * word + 16 <= stride
        window = np.zeros((lh, lw), bool)
        window[EDGE:lh - EDGE, EDGE:lw - EDGE] = True
        assert (interior[window] == 1).all() and (interior[~window] == 0).all()
        assert (tested[window] >= 1).all() and (tested[~window] == 0).all()
    if (w, h, levels, scale) == (640, 480, 8, 1.2):
        assert len(tiles) == 227


def test_fitted_tiles_waste_little():
    """quick-tested positions per window position at 640 x 480 (the headline): the interiors partition the window, the aprons add the rest"""
    tiles, _ = _plan(640, 480, 8, 1.2)
    window = sum((int(t[13]) - 2 * EDGE) * (int(t[14]) - 2 * EDGE) for t in {(r[0], r[13], r[14]): r for r in tiles.tolist()}.values())
    tested = int(((tiles[:, 6] - tiles[:, 5]) * (tiles[:, 8] - tiles[:, 7])).sum())
    items = int((tiles[:, 9] * tiles[:, 10]).sum()) * 4
    assert tested / window < 1.12 and items / window < 1.15, (tested / window, items / window)


def _kernel_lds(path):
    """group_segment_fixed_size (static LDS bytes) of every gfx950 kernel in the offload bundles of a HIP shared library: the first dword of the
    kernel's descriptor (symbol <kernel>.kd) in the code object"""
    f = open(path, "rb").read()

    def sections(elf):
        shoff, = struct.unpack_from("<Q", elf, 0x28)
        shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
        return [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]

    def elf_sections_named(elf, name):
        secs = sections(elf)
        shstr = secs[struct.unpack_from("<H", elf, 0x3E)[0]]
        for sh in secs:
            nm = elf[shstr[4] + sh[0]:elf.index(b"\0", shstr[4] + sh[0])].decode()
            if nm == name:
                yield sh

    fat = next(elf_sections_named(f, ".hip_fatbin"))
    blob = f[fat[4]:fat[4] + fat[5]]
    out = {}
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    pos = blob.find(magic)
    while pos >= 0:
        n, = struct.unpack_from("<Q", blob, pos + 24)
        q = pos + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, q)
            triple = blob[q + 24:q + 24 + tl].decode()
            q += 24 + tl
            if "gfx950" not in triple:
                continue
            elf = blob[pos + off:pos + off + size]
            assert elf[:4] == b"\x7fELF", "compressed or unknown code object"
            secs = sections(elf)
            symtab = next(elf_sections_named(elf, ".symtab"))
            strtab = secs[symtab[6]]
            for k in range(symtab[5] // 24):
                st_name, st_info, st_other, st_shndx, st_value, st_size = struct.unpack_from("<IBBHQQ", elf, symtab[4] + 24 * k)
                name = elf[strtab[4] + st_name:elf.index(b"\0", strtab[4] + st_name)].decode()
                if name.endswith(".kd") and 0 < st_shndx < len(secs):
                    sh = secs[st_shndx]
                    out[name[:-3]] = struct.unpack_from("<I", elf, sh[4] + st_value - sh[3])[0]
        pos = blob.find(magic, pos + 1)
    return out


def test_built_fast_kernels_lds():
    """the FAST kernels as built: fast_kernel within its LDS before the fitted plan, both it and the retry kernel within 8 blocks per CU"""
    from semantic_slam_mapping_amd._lib import LIB_PATH
    lds = _kernel_lds(LIB_PATH)
    fast = [v for k, v in lds.items() if k.startswith("_Z11fast_kernel")]
    retry = [v for k, v in lds.items() if k.startswith("_Z17fast_retry_kernel")]
    assert len(fast) == 1 and len(retry) == 1, sorted(lds)[:20]
    assert fast[0] <= LDS_BUDGET and LDS_PER_CU // fast[0] >= 8 and LDS_PER_CU // retry[0] >= 8, (fast, retry)
