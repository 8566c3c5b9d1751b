// ssm_orb_plan.h -- the geometry of the ORB front end and its plan: everything that is computed from an ssm_config before the first kernel runs.  No HIP
// header: the kernels and the context take it through ssm_internal.h, the planner (ssm_orb_plan.cpp) and host/test_orb_plan.cpp are plain C++.  Not installed.
#pragma once
#include "../../include/ssm_hip.h"
#include <stdint.h>
#include <stddef.h>
#include <cmath>
#include <string>
#include <vector>
#ifndef SSM_HIDDEN
#define SSM_HIDDEN __attribute__((visibility("hidden")))
#endif
#ifndef SSM_HD                 // as in include/ssm/*_core.h
#  if defined(__HIPCC__)
#    define SSM_HD __host__ __device__ inline
#  else
#    define SSM_HD inline
#  endif
#endif

#define SSM_MAX_LEVELS 12
#define SSM_EDGE 19            // ORBextractor EDGE_THRESHOLD
#define SSM_HALF_PATCH 15
#define SSM_PATCH 31
#define SSM_MAX_NODES 1024     // quad-tree nodes held in LDS per (frame, level)

inline int cv_round_f(float v) { return (int)lrint((double)v); }

struct LevelGeom {
    int w, h, stride;          // level image; rows padded to a multiple of 16 bytes
    int img_off;               // byte offset inside one frame's pyramid buffer (16-B aligned)
    int nCols, nRows, wCell, hCell;   // FAST cell grid (ComputeKeyPointsOctTree, W = 30)
    int cell_off;              // first flattened cell id of this level
    int tile_off, tiles_x;     // 128x32 tiles of the whole level image in the flattened grid (blur_kernel)
    int ftile_off, ftiles_x;   // FAST tiles of this level: they cover [SSM_EDGE, w - SSM_EDGE) x [SSM_EDGE, h - SSM_EDGE) only, the positions FAST may report
    int ftw, fth;              // FAST tile interior (<= FT_W x FT_H), fitted to that window: ftile_rect
    int nfeat;                 // mnFeaturesPerLevel
    int cand_off, cand_cap;    // entries inside one frame's candidate buffer
    int sel_off, sel_cap;      // slots inside one frame's selected-keypoint staging (nfeat + 3)
    int minBX, minBY, maxBX, maxBY;
    int nIni;                  // quad-tree root nodes
    float hX;                  // root node width
    float sf;                  // mvScaleFactor[level]
    uint32_t mulTX, fmulTX;    // ceil(2^32 / tiles_x), ceil(2^32 / ftiles_x): same use
    int boff;                  // byte offset of the level inside one frame's BLURRED pyramid (tiled: see blur_off)
    int bt_off, bt_x, bt_units_off;   // blur_mfma_kernel: first 128-column strip of the level, strips of the level, first 32-column unit table
    uint32_t mulW, mulH;       // ceil(2^32 / wCell), ceil(2^32 / hCell): floor(n / cell) == __umulhi(n, mul) for n < 4096 (exact: n * (mul * cell - 2^32) < 2^32)
};
// The blurred pyramid is stored in tiles of 8 rows x 16 columns (128 bytes = one cache line): its only reader, brief_kernel, gathers 37 x 37 patches,
// and a patch covers ~25 such lines instead of the ~47 it touches in a row-major image (a 37-byte row segment drags in a whole 128-byte line).
// Offset of the 16-byte word that holds (x, y): rows padded to a multiple of 8.
SSM_HD int blur_off(int boff, int stride, int x, int y) { return boff + (((y >> 3) * (stride >> 4) + (x >> 4)) << 7) + ((y & 7) << 4) + (x & 15); }
// FAST tiles (fast_kernel): the interiors partition the window [SSM_EDGE, w - SSM_EDGE) x [SSM_EDGE, h - SSM_EDGE) of a level; a block quick-tests
// the interior plus a 1-position apron (the NMS neighbours) clipped to the window, as 4-column groups counted from the apron's first column
#define FT_W 126              // interior, at most: the scored width (+ 2) is 32 groups of 4
#define FT_H 32
#define FT_SW (FT_W + 2)      // scored positions per row / rows, at most
#define FT_SH (FT_H + 2)
#define FT_PW 144             // staged pixel row: [xs0 - 4, xs0 + 140) = nine 16-byte words
#define FT_PH (FT_SH + 6)     // staged rows: [ys0 - 3, ys0 + FT_SH + 3)
#define FT_SST 132            // score rows: [xs0 - 1, xs0 + 131), FT_SH + 2 of them
#define FT_BW 32              // pass-bit image: one byte (the 4 positions of a group) per group, 32 bytes per scored row
#define FT_STAGE ((FT_PH * FT_PW) / 8)   // candidates staged per tile: as many as fit in the pixel tile they replace (720)
// the LDS arrays fast_tile declares (the compiler may pad; tests/test_fast_tiling.py reads what the built kernels take from the code object)
#define FT_LDS_BYTES (4 * 8 + FT_PH * FT_PW + (FT_SH + 2) * FT_SST + 2 * FT_SW * FT_SH + 2 * (FT_SW + 2) + 2 * (FT_SH + 2) + 4 * 64 + 4 * 4 + 4 * 3)
// interior [x0, x1) x [y0, y1) of FAST tile (tx, ty) of a level
SSM_HD void ftile_rect(const LevelGeom& L, int tx, int ty, int& x0, int& x1, int& y0, int& y1)
{
    x0 = SSM_EDGE + tx * L.ftw; x1 = x0 + L.ftw < L.w - SSM_EDGE ? x0 + L.ftw : L.w - SSM_EDGE;
    y0 = SSM_EDGE + ty * L.fth; y1 = y0 + L.fth < L.h - SSM_EDGE ? y0 + L.fth : L.h - SSM_EDGE;
}
struct OrbGeom {
    int nlevels, W, H;
    int pyr_bytes;             // one frame's pyramid (all levels)
    int cells_total, cand_total, sel_total, tiles_total, ftiles_total;
    int blur_bytes;            // one frame's blurred pyramid
    int bt_total, bt_units_total;   // blur_mfma_kernel strips (= blocks) per frame, 32-column unit tables
    int cap;                   // output keypoints per frame (orb_features + 3*levels)
    int ini_th, min_th;
    int umax[SSM_HALF_PATCH + 1];
    LevelGeom L[SSM_MAX_LEVELS];
};

// the pyramid in one launch (kernels_orb.hip resize4_kernel_bands: gray + every level, one block per (band, frame)); the plan is built once per geometry and band count
#ifndef PB_T
#define PB_T 1024             // (512 threads: 154 us against 150 at B = 8)
#endif
#ifndef PB_BANDS
#define PB_BANDS 8             // bands per frame in batches (640 x 480: 79 KB of LDS, two blocks per CU); measured per 250 frames with the 8-pixel items: 8 bands 150 us, 12: 173, 16: 208 (4-pixel items: 176, 197, 208)
#endif
#define PB_MAX_LDS (80 * 1024)     // two blocks per CU at least
struct PyrBandArgs {
    const void* xg[SSM_MAX_LEVELS]; const int32_t* yofs[SSM_MAX_LEVELS]; const int16_t* ya[SSM_MAX_LEVELS]; uint32_t mulq0, mulg[SSM_MAX_LEVELS]; int buf1;
    uint32_t wide;                 // bit l: level l's items are 8 pixels wide (xg[l] = its XGroup8 table); clear: 4 pixels (XGroup)
};
SSM_HD int pyr_wide(const PyrBandArgs& t, int l) { return (int)(t.wide >> l) & 1; }
struct PyrBandPlan { int bands = 0; size_t lds = 0; void* d_tab = nullptr; PyrBandArgs args = {}; };     // bands == 0: no fused form (k_gray + k_pyramid)
// The work items of one (band, level) of the fused kernel: column groups of 4 or 8 pixels x the y tables' 4-row blocks, counted from
// the block that holds the band's first comp row.  Item i = (block, group) = (i / groups, i % groups), the division by the plan's reciprocal mulg.
// The kernel and ssm_debug_pyramid_plan (ssm_orb_plan.cpp, which lists the items for the tests) both take the decomposition from here.
struct PyrItems { int groups, c0, nblk, items; };
SSM_HD PyrItems pyr_items(int stride, int wide, int comp_lo, int comp_hi)
{
    PyrItems it; it.groups = stride >> (wide ? 3 : 2); it.c0 = comp_lo & ~3; it.nblk = ((comp_hi - it.c0) >> 2) + 1;
    it.items = it.groups * it.nblk;
    return it;
}
SSM_HD int pyr_item_run(int i, uint32_t mulg) { return (int)(((uint64_t)(uint32_t)i * mulg) >> 32); }      // exact: i * groups < 2^32
#define PYR_SLACK 16               // bytes behind each level buffer: a window of the last source row may end past it (pyramid_xgroups, ssm_orb_plan.cpp, bounds it)
#define BLUR_ROWS 58           // output rows of one blur_mfma block (64 input rows)

// ---- the planner (ssm_orb_plan.cpp) ----
// cv::resize INTER_LINEAR 8u fixed point: per destination pixel the left source neighbour and the (1 - f, f) pair in 1/2048
SSM_HIDDEN void resize_tables(int ssize, int dsize, std::vector<int32_t>& ofs, std::vector<int16_t>& coef);
// the per-group x constants of one level: XGroup (4 pixels, 8 dwords) and XGroup8 (8 pixels, 12 dwords), and whether every group of the level fits the
// layout the kernels assume (fits4: each pixel's pair inside 8 bytes from the first pixel's left neighbour; fits8: pixels 0 - 3 inside those 8 bytes,
// pixels 4 - 7 inside the 8 bytes from 4 on, and no coefficient pair -- ya: the level's y pairs -- above 2048 in sum, which bounds a result by 255)
void pyramid_xgroups(const std::vector<int32_t>& xo, const std::vector<int16_t>& xa, const std::vector<int16_t>& ya, int dw, int dstride, int sstride,
                     std::vector<uint32_t>& xg4, std::vector<uint32_t>& xg8, bool& fits4, bool& fits8);
// tab: bands x levels x (comp_lo, comp_hi, own_lo, own_hi); false: no fused form at this band count.  streaming[l]: level l has the 4-pixel table,
// wide_ok[l]: it also fits the 8-pixel layout
bool pyramid_band_choose(const OrbGeom& g, const std::vector<int32_t>* yofs, const bool* streaming, const bool* wide_ok, bool batch, std::vector<int32_t>& tab, PyrBandPlan& p);
bool pyramid_band_plan(const OrbGeom& g, const std::vector<int32_t>* yofs, const bool* streaming, const bool* wide_ok, int bands, std::vector<int32_t>& tab, PyrBandPlan& p);
int pyramid_block_threads();       // PB_T
// blur_mfma_kernel's coefficient fragments
size_t blur_mfma_table_bytes(const OrbGeom& g);
void blur_mfma_tables(const OrbGeom& g, void* host_out);

// What an ssm_config fixes of the ORB front end: the geometry, and per level l >= 1 the resize tables as the device gets them (the y tables padded to a multiple
// of four rows: resize4_kernel reads them four rows at a time), the 4-pixel and 8-pixel group tables and whether the level has them (streaming: the 4-pixel
// layout fits; wide_ok: the 8-pixel one too -- a table without its flag is not uploaded), the fused pyramid's band plans with their band tables ([0]: batches,
// [1]: the one-frame call; bands == 0 where a level needs the general resize kernel) and the blur coefficient table.  Built once per context (ssm_create)
// and by the two debug entries that list a plan for the tests.
struct OrbPlan {
    OrbGeom g{};
    std::vector<int32_t> xofs[SSM_MAX_LEVELS], yofs[SSM_MAX_LEVELS]; std::vector<int16_t> xa[SSM_MAX_LEVELS], ya[SSM_MAX_LEVELS];
    std::vector<uint32_t> xgrp[SSM_MAX_LEVELS], xgrp8[SSM_MAX_LEVELS]; bool streaming[SSM_MAX_LEVELS] = {}, wide_ok[SSM_MAX_LEVELS] = {};
    PyrBandPlan bands[2]; std::vector<int32_t> band_tab[2];
    std::vector<uint8_t> blur_tab;
};
// SSM_E_INVAL + the reason in err where the configuration is refused; p is empty then (g.nlevels == 0)
SSM_HIDDEN int orb_plan_build(const ssm_config& cfg, OrbPlan& p, std::string& err);
// the band plan of p's geometry at an explicit band count (ssm_debug_pyramid, ssm_debug_pyramid_plan with bands > 0); false: no fused form there
SSM_HIDDEN bool orb_plan_bands(const OrbPlan& p, int bands, std::vector<int32_t>& tab, PyrBandPlan& out);
