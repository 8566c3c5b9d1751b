// ssm_orb_plan.cpp -- the plan of the ORB front end (ssm_orb_plan.h): geometry, resize and group tables, the fused pyramid's bands, the blur coefficients, and the
// two debug entries that list a plan for the tests.  Host arithmetic only, plain C++: built once into libssm_hip.so; host/test_orb_plan.cpp links this file alone.
#include "ssm_orb_plan.h"
#include "../../include/ssm/fast_quick_core.h"
#include <algorithm>
#include <cstring>

// ---------------------------------------------------------------- geometry (mirrors ORBextractor ctor / ComputePyramid)
// the scored positions [s0, s1) = [max(a - 1, EDGE), min(b + 1, n - EDGE)) of a FAST tile interior [a, b) along one axis (the interior + its NMS neighbours inside
// the window) and the cells (of size `cell`, counted from origin + 3) they touch: the same rectangle and cells as fast_tile
struct FastScored { int s0, s1, cells; };
static FastScored fast_scored(int a, int b, int n, int origin, int cell)
{
    const int s0 = a - 1 > SSM_EDGE ? a - 1 : SSM_EDGE, s1 = b + 1 < n - SSM_EDGE ? b + 1 : n - SSM_EDGE;
    return {s0, s1, (s1 - 1 - origin - 3) / cell - (s0 - origin - 3) / cell + 1};
}
static int build_geometry(const ssm_config& c, OrbGeom& g, std::string& err)
{
    memset(&g, 0, sizeof(g));
    if (c.orb_levels < 1 || c.orb_levels > SSM_MAX_LEVELS) { err = "orb_levels must be 1..12"; return SSM_E_INVAL; }
    if (c.orb_features < 1) { err = "orb_features must be >= 1"; return SSM_E_INVAL; }
    if (c.orb_iniThFAST < 1 || c.orb_minThFAST < 1 || c.orb_minThFAST > 254 || c.orb_iniThFAST > 254) { err = "FAST thresholds must be 1..254"; return SSM_E_INVAL; }
    if (c.width < 64 || c.height < 64 || c.width > 4000 || c.height > 4000) { err = "frame size must be 64..4000"; return SSM_E_INVAL; }
    if (!(c.orb_scale > 1.0f)) { err = "orb_scale must be > 1"; return SSM_E_INVAL; }
    g.nlevels = c.orb_levels; g.W = c.width; g.H = c.height; g.ini_th = c.orb_iniThFAST; g.min_th = c.orb_minThFAST;
    const double scaleFactor = (double)c.orb_scale;
    float sf[SSM_MAX_LEVELS], inv[SSM_MAX_LEVELS];
    sf[0] = 1.0f;
    for (int i = 1; i < g.nlevels; i++) sf[i] = (float)(sf[i-1] * scaleFactor);
    for (int i = 0; i < g.nlevels; i++) inv[i] = 1.0f / sf[i];
    int feat[SSM_MAX_LEVELS];
    {
        const float factor = (float)(1.0f / scaleFactor);
        float nd = c.orb_features * (1 - factor) / (1 - (float)pow((double)factor, (double)g.nlevels));
        int sum = 0;
        for (int l = 0; l < g.nlevels - 1; l++) { feat[l] = cv_round_f(nd); sum += feat[l]; nd *= factor; }
        feat[g.nlevels-1] = c.orb_features - sum > 0 ? c.orb_features - sum : 0;
    }
    {
        const int vmax = (int)floor(SSM_HALF_PATCH * sqrt(2.0) / 2 + 1), vmin = (int)ceil(SSM_HALF_PATCH * sqrt(2.0) / 2);
        const double hp2 = SSM_HALF_PATCH * SSM_HALF_PATCH;
        int um[SSM_HALF_PATCH + 2] = {0};
        for (int v = 0; v <= vmax; ++v) um[v] = (int)lrint(sqrt(hp2 - v * v));
        for (int v = SSM_HALF_PATCH, v0 = 0; v >= vmin; --v) { while (um[v0] == um[v0 + 1]) ++v0; um[v] = v0; ++v0; }
        for (int v = 0; v <= SSM_HALF_PATCH; v++) g.umax[v] = um[v];
    }
    int off = 0, cells = 0, cands = 0, sels = 0, tiles = 0, ftiles = 0, btiles = 0, bunits = 0, boff = 0;
    for (int l = 0; l < g.nlevels; l++) {
        LevelGeom& L = g.L[l];
        L.w = cv_round_f((float)c.width * inv[l]); L.h = cv_round_f((float)c.height * inv[l]);
        if (L.w < 2 * SSM_EDGE + 8 + 30 || L.h < 2 * SSM_EDGE + 8 + 30) { err = "pyramid level too small for the ORB border; lower orb_levels"; return SSM_E_INVAL; }
        L.stride = (L.w + 15) & ~15; L.img_off = off; off += L.stride * L.h; L.boff = boff; boff += L.stride * ((L.h + 7) & ~7);      /* rows 16-B aligned: wide loads/stores everywhere */
        L.minBX = SSM_EDGE - 3; L.minBY = SSM_EDGE - 3; L.maxBX = L.w - SSM_EDGE + 3; L.maxBY = L.h - SSM_EDGE + 3;
        const float width = (float)(L.maxBX - L.minBX), height = (float)(L.maxBY - L.minBY);
        L.nCols = (int)(width / 30.f); L.nRows = (int)(height / 30.f);
        L.wCell = (int)ceilf(width / L.nCols); L.hCell = (int)ceilf(height / L.nRows);
        if (L.wCell < 17 || L.hCell < 5) { err = "FAST cell too small"; return SSM_E_INVAL; }   /* FAST tiles: at most 8 x 8 cells (checked below) */
        L.mulW = (uint32_t)(((1ull << 32) + L.wCell - 1) / L.wCell); L.mulH = (uint32_t)(((1ull << 32) + L.hCell - 1) / L.hCell);
        L.cell_off = cells; cells += L.nCols * L.nRows;
        L.tiles_x = (L.w + 127) / 128; L.mulTX = (uint32_t)(((1ull << 32) + L.tiles_x - 1) / L.tiles_x); L.tile_off = tiles; tiles += L.tiles_x * ((L.h + 31) / 32);
        /* FAST reports nothing within SSM_EDGE of the border: its tiles cover that window only, as few as fit and all but the last of each row and
           column of one size (640x480, 8 levels: 227 tiles; interiors 121 x 32 at level 0), so that little of a tile lies outside the window */
        {
            const int fw = L.w - 2 * SSM_EDGE, fh = L.h - 2 * SSM_EDGE;
            const int kx = (fw + FT_W - 1) / FT_W, ky = (fh + FT_H - 1) / FT_H;
            L.ftw = (fw + kx - 1) / kx; L.fth = (fh + ky - 1) / ky;
            L.ftiles_x = (fw + L.ftw - 1) / L.ftw;
            L.fmulTX = (uint32_t)(((1ull << 32) + L.ftiles_x - 1) / L.ftiles_x); L.ftile_off = ftiles; ftiles += L.ftiles_x * ((fh + L.fth - 1) / L.fth);
            /* the scored rectangle of a tile (interior + apron) touches at most 8 x 8 cells: pass 2's emptyrow bytes and the 64 lmax slots of fast_tile */
            for (int x0 = SSM_EDGE; x0 < L.w - SSM_EDGE; x0 += L.ftw)
                if (fast_scored(x0, x0 + L.ftw, L.w, L.minBX, L.wCell).cells > 8) { err = "FAST tile spans more than 8 cell columns"; return SSM_E_INVAL; }
            for (int y0 = SSM_EDGE; y0 < L.h - SSM_EDGE; y0 += L.fth)
                if (fast_scored(y0, y0 + L.fth, L.h, L.minBY, L.hCell).cells > 8) { err = "FAST tile spans more than 8 cell rows"; return SSM_E_INVAL; }
        }
        L.bt_x = (L.stride + 127) / 128; L.bt_off = btiles; btiles += L.bt_x; L.bt_units_off = bunits; bunits += (L.stride + 31) / 32;
        if (L.nCols * L.nRows >= (1 << 17)) { err = "too many FAST cells"; return SSM_E_INVAL; }
        L.nfeat = feat[l];
        if (L.nfeat + 3 > SSM_MAX_NODES - 8) { err = "too many features per level for the LDS quad-tree (max 1013 per level)"; return SSM_E_INVAL; }
        L.cand_off = cands; L.cand_cap = ((L.w + 1) / 2 + L.nCols + 1) * ((L.h + 1) / 2 + L.nRows + 1); cands += L.cand_cap;
        if (L.cand_cap > 65535 * 16) { err = "level too large"; return SSM_E_INVAL; }
        L.sel_off = sels; L.sel_cap = L.nfeat + 3; sels += L.sel_cap;
        int nIni = (int)roundf((float)(L.maxBX - L.minBX) / (float)(L.maxBY - L.minBY)); if (nIni < 1) nIni = 1;
        L.nIni = nIni; L.hX = (float)(L.maxBX - L.minBX) / nIni;
        if (4 * nIni + 8 > SSM_MAX_NODES) { err = "aspect ratio too extreme"; return SSM_E_INVAL; }
        L.sf = sf[l];
    }
    g.bt_total = btiles; g.bt_units_total = bunits; g.blur_bytes = boff;
    g.pyr_bytes = off; g.tiles_total = tiles; g.ftiles_total = ftiles; g.cells_total = cells; g.cand_total = cands; g.sel_total = sels;
    g.cap = c.orb_features + 3 * g.nlevels;
    return SSM_OK;
}
void resize_tables(int ssize, int dsize, std::vector<int32_t>& ofs, std::vector<int16_t>& coef)
{
    ofs.resize(dsize); coef.resize(2 * dsize);
    const double inv_scale = (double)dsize / ssize, scale = 1.0 / inv_scale;
    for (int d = 0; d < dsize; d++) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)floorf(f);
        f -= (float)s;
        if (s < 0) { f = 0.f; s = 0; }
        if (s >= ssize - 1) { f = 0.f; s = ssize - 1; }
        ofs[d] = s;
        coef[2*d] = (int16_t)cv_round_f((1.f - f) * 2048.f); coef[2*d+1] = (int16_t)cv_round_f(f * 2048.f);
    }
}

// ---------------------------------------------------------------- the fused pyramid's bands and group tables, the blur coefficients
int pyramid_block_threads() { return PB_T; }
// the band count of a geometry: PB_BANDS per frame for batches, 32 for the one-frame call (one frame on more CUs); more bands where the level
// buffers would not fit; none where a level needs the general resize kernel (p.bands stays 0).  The 8-pixel items are for batches, where the kernel is
// bound by instruction issue; the one-frame call keeps the 4-pixel items on every level (shorter dependent chains per thread: measured 17.0 us against
// 18.9 with the 8-pixel items, profiles/r10_pyramid_rows.md)
bool pyramid_band_choose(const OrbGeom& g, const std::vector<int32_t>* yofs, const bool* streaming, const bool* wide_ok, bool batch, std::vector<int32_t>& tab, PyrBandPlan& p)
{
    static const int cand[2][8] = {{PB_BANDS, 12, 16, 24, 32, 48, 64, 0}, {32, 48, 64, 0}};
    for (int i = 0; i < 8 && cand[batch ? 0 : 1][i]; i++)
        if (cand[batch ? 0 : 1][i] >= (batch ? PB_BANDS : 0) && pyramid_band_plan(g, yofs, streaming, batch ? wide_ok : nullptr, cand[batch ? 0 : 1][i], tab, p)) return true;
    return false;
}
// The band rows of every (band, level) for `bands` bands, from the host's y tables (yofs[l]: level l's source rows in level l-1).  false: the geometry
// has no fused form at this band count (a level without the streaming x tables, fewer rows than bands, or level buffers beyond PB_MAX_LDS).
bool pyramid_band_plan(const OrbGeom& g, const std::vector<int32_t>* yofs, const bool* streaming, const bool* wide_ok, int bands, std::vector<int32_t>& tab, PyrBandPlan& p)
{
    const int L = g.nlevels;
    if (bands < 1) return false;
    for (int l = 0; l < L; l++) if (g.L[l].h < bands || (l > 0 && !streaming[l])) return false;
    tab.assign((size_t)bands * L * 4, 0);
    size_t need[2] = {0, 0};
    for (int b = 0; b < bands; b++) {
        int lo = 0, hi = -1;
        for (int l = L - 1; l >= 0; l--) {
            const int h = g.L[l].h, olo = (int)((int64_t)b * h / bands), ohi = (int)((int64_t)(b + 1) * h / bands) - 1;
            int clo = olo, chi = ohi;
            if (l < L - 1) {                                               // the source rows of comp(l + 1): [yofs[lo], min(yofs[hi] + 1, h - 1)]
                clo = std::min(clo, yofs[l + 1][lo]); chi = std::max(chi, std::min(yofs[l + 1][hi] + 1, h - 1));
            }
            int32_t* e = &tab[((size_t)b * L + l) * 4];
            e[0] = clo; e[1] = chi; e[2] = olo; e[3] = ohi;
            need[l & 1] = std::max(need[l & 1], (size_t)(chi - clo + 1) * g.L[l].stride);
            lo = clo; hi = chi;
        }
    }
    // PYR_SLACK bytes behind each buffer: a window starts at the 4-aligned address at or below a source byte of its row (<= stride - 4 from the row's
    // start) and is 12 (4-pixel item, three dwords) or 16 bytes long (8-pixel item, four), so in a buffer's last row it ends up to 8 / 12 bytes past it
    const size_t buf1 = (need[0] + PYR_SLACK + 15) & ~(size_t)15, lds = buf1 + need[1] + PYR_SLACK;
    if (lds > PB_MAX_LDS) return false;
    memset(&p.args, 0, sizeof(p.args));
    p.args.buf1 = (int)buf1;
    const int q0 = g.L[0].stride >> 4;                                     // level 0's items: 16 pixels
    p.args.mulq0 = (uint32_t)(((1ull << 32) + q0 - 1) / q0);
    for (int l = 1; l < L; l++) {
        const int wide = wide_ok && wide_ok[l] ? 1 : 0;
        const int gr = g.L[l].stride >> (wide ? 3 : 2);
        p.args.wide |= (uint32_t)wide << l;
        p.args.mulg[l] = (uint32_t)(((1ull << 32) + gr - 1) / gr);
    }
    p.bands = bands; p.lds = lds;
    return true;
}
void pyramid_xgroups(const std::vector<int32_t>& xo, const std::vector<int16_t>& xa, const std::vector<int16_t>& ya, int dw, int dstride, int sstride,
                     std::vector<uint32_t>& xg4, std::vector<uint32_t>& xg8, bool& fits4, bool& fits8)
{
    const int g4 = dstride / 4, g8 = dstride / 8;
    xg4.assign((size_t)g4 * 8, 0u); xg8.assign((size_t)g8 * 12, 0u); fits4 = fits8 = true;
    auto pair = [&](int x) { return (uint32_t)(uint16_t)xa[2 * x] | ((uint32_t)(uint16_t)xa[2 * x + 1] << 16); };
    for (int x = 0; x < dw; x++) if (xa[2 * x] < 0 || xa[2 * x + 1] < 0 || xa[2 * x] + xa[2 * x + 1] > 2048) fits8 = false;
    for (size_t y = 0; 2 * y + 1 < ya.size(); y++) if (ya[2 * y] < 0 || ya[2 * y + 1] < 0 || ya[2 * y] + ya[2 * y + 1] > 2048) fits8 = false;
    for (int q = 0; q < g4; q++) {
        uint32_t* e = &xg4[(size_t)q * 8];
        const int x0 = 4 * q;
        if (x0 >= dw) continue;                                               // padding group: coefficients 0 -> zeros, window at 0
        const int base = xo[x0];
        e[4] = (uint32_t)base;
        for (int k = 0; k < 4 && x0 + k < dw; k++) {
            const int off = xo[x0 + k] - base;
            if (off < 0 || off > 6) fits4 = false;
            e[k] = pair(x0 + k);
            e[5] |= (uint32_t)(off & 15) << (4 * k);
        }
        if ((base & ~3) + 12 > sstride + PYR_SLACK) fits4 = false;            // (cannot happen: base < sstride)
    }
    for (int q = 0; q < g8; q++) {
        uint32_t* e = &xg8[(size_t)q * 12];
        const int x0 = 8 * q;
        if (x0 >= dw) continue;
        const int base = xo[x0];
        e[8] = (uint32_t)base;
        for (int k = 0; k < 8 && x0 + k < dw; k++) {
            const int off = xo[x0 + k] - base - (k < 4 ? 0 : 4);              // from the pixel's dword pair: (0, 1) of the normalised window or (1, 2)
            if (off < 0 || off > 6) fits8 = false;
            e[k] = pair(x0 + k);
            e[9] |= (uint32_t)(off & 15) << (4 * k);
        }
        if ((base & ~3) + 16 > sstride + PYR_SLACK) fits8 = false;
    }
}
size_t blur_mfma_table_bytes(const OrbGeom& g) { return (size_t)(128 + 128 * g.bt_units_total) * 16; }
void blur_mfma_tables(const OrbGeom& g, void* host_out)
{
    static const int tc[7] = {18, 34, 49, 55, 49, 34, 18};
    int8_t* o = reinterpret_cast<int8_t*>(host_out);
    auto refl = [](int i, int n) { i = i < 0 ? -i : i; i = i >= n ? 2 * n - 2 - i : i; return i < 0 ? 0 : (i >= n ? n - 1 : i); };
    for (int which = 0; which < 2; which++)                       // column pass: B[k][n], k in the accumulator's row order: element j of lane half h = row 8 (j >> 2) + 4 h + (j & 3)
        for (int lane = 0; lane < 64; lane++)
            for (int j = 0; j < 16; j++) {
                const int n = lane & 31, h = lane >> 5, k = 8 * (j >> 2) + 4 * h + (j & 3) + 32 * which, d = k - n;
                o[(which * 64 + lane) * 16 + j] = (int8_t)((d >= 0 && d <= 6) ? tc[d] : 0);
            }
    // row pass, per level and unit: entry [K half s][lane = 32 h + n][j] is the coefficient of input column x_in = 32 u - 16 + k, k = 32 s + 16 h + j, in output
    // column x_out = 32 u + n: the taps that reach x_in, directly or reflected (each tap is added where it lands; every other entry is 0)
    memset(o + 128 * 16, 0, (size_t)128 * g.bt_units_total * 16);
    for (int l = 0; l < g.nlevels; l++) {
        const LevelGeom& L = g.L[l];
        for (int u = 0; u < (L.stride + 31) / 32; u++)
            for (int n = 0; n < 32 && 32 * u + n < L.w; n++)
                for (int t = 0; t < 7; t++) {
                    const int k = refl(32 * u + n + t - 3, L.w) - (32 * u - 16);
                    if (k < 0 || k >= 64) continue;
                    const int s = k >> 5, h = (k >> 4) & 1, j = k & 15;
                    o[((size_t)(128 + (L.bt_units_off + u) * 128 + s * 64 + 32 * h + n)) * 16 + j] += (int8_t)tc[t];
                }
    }
}

// ---------------------------------------------------------------- the plan
int orb_plan_build(const ssm_config& cfg, OrbPlan& p, std::string& err)
{
    p = OrbPlan();
    { const int r = build_geometry(cfg, p.g, err); if (r) { p = OrbPlan(); return r; } }
    const OrbGeom& g = p.g;
    p.blur_tab.resize(blur_mfma_table_bytes(g)); blur_mfma_tables(g, p.blur_tab.data());
    for (int l = 1; l < g.nlevels; l++) {
        std::vector<int32_t>& yo = p.yofs[l]; std::vector<int16_t>& ya = p.ya[l];
        resize_tables(g.L[l-1].w, g.L[l].w, p.xofs[l], p.xa[l]); resize_tables(g.L[l-1].h, g.L[l].h, yo, ya);
        // per 4-pixel group (the streaming kernel takes a group's source bytes with one 8-byte load per row) and per 8-pixel group (the fused kernel:
        // four LDS dwords per row): the (a0, a1) pairs, the byte offset of the first pixel's left neighbour and each pixel's offset from it
        bool fits = false, fits8 = false;
        pyramid_xgroups(p.xofs[l], p.xa[l], ya, g.L[l].w, g.L[l].stride, g.L[l-1].stride, p.xgrp[l], p.xgrp8[l], fits, fits8);
        while (yo.size() & 3) { yo.push_back(yo.back()); ya.push_back(ya[ya.size() - 2]); ya.push_back(ya[ya.size() - 2]); }   // resize4_kernel reads the y tables four rows at a time
        p.streaming[l] = fits; p.wide_ok[l] = fits && fits8;
    }
    // the fused pyramid's band tables (none where a level needs the general resize kernel); the planner reads rows 0 .. h - 1 of the y tables only
    for (int k = 0; k < 2; k++) if (!pyramid_band_choose(g, p.yofs, p.streaming, p.wide_ok, k == 0, p.band_tab[k], p.bands[k])) p.band_tab[k].clear();
    return SSM_OK;
}
bool orb_plan_bands(const OrbPlan& p, int bands, std::vector<int32_t>& tab, PyrBandPlan& out) { return pyramid_band_plan(p.g, p.yofs, p.streaming, p.wide_ok, bands, tab, out); }

// ---------------------------------------------------------------- the plan as the tests read it (no context, no device)
extern "C" int ssm_debug_fast_plan(const ssm_config* cfg, int32_t* tiles, int cap, int* ntiles, int32_t* limits)
{
    if (!cfg || !ntiles) return SSM_E_INVAL;
    OrbPlan P; std::string err;
    { const int r = orb_plan_build(*cfg, P, err); if (r) return r; }
    const OrbGeom& g = P.g;
    if (limits) { const int32_t v[6] = {FT_LDS_BYTES, FT_SW / 4, FT_SH, FT_PW, FT_PH, FT_STAGE}; memcpy(limits, v, sizeof(v)); }
    *ntiles = g.ftiles_total;
    if (!tiles) return SSM_OK;
    if (cap < g.ftiles_total) return SSM_E_INVAL;
    for (int l = 0; l < g.nlevels; l++) {
        const LevelGeom& L = g.L[l];
        const int ntl = (l + 1 < g.nlevels ? g.L[l+1].ftile_off : g.ftiles_total) - L.ftile_off;
        for (int t = 0; t < ntl; t++) {
            int x0, x1, y0, y1;
            ftile_rect(L, t % L.ftiles_x, t / L.ftiles_x, x0, x1, y0, y1);
            const FastScored sx = fast_scored(x0, x1, L.w, L.minBX, L.wCell), sy = fast_scored(y0, y1, L.h, L.minBY, L.hCell);
            const int32_t v[16] = {l, x0, x1, y0, y1, sx.s0, sx.s1, sy.s0, sy.s1, (sx.s1 - sx.s0 + 3) / 4, sy.s1 - sy.s0, sx.cells, sy.cells, L.w, L.h, L.stride};
            memcpy(tiles + 16 * (size_t)(L.ftile_off + t), v, sizeof(v));
        }
    }
    return SSM_OK;
}

// fast_tile's quick test (ssm_fq::quick4) on n groups of four positions: words = n x (C, P, Nx, U, D), out = n pass nibbles
extern "C" int ssm_debug_fast_quick(const uint32_t* words, int n, int threshold, int valid, uint8_t* out)
{
    if (!words || !out || n < 0 || threshold < 0 || threshold > 255 || valid < 1 || valid > 4) return SSM_E_INVAL;
    const uint32_t th2 = ssm_fq::pack_threshold(threshold), keep = ssm_fq::keep_mask(valid);
    for (int i = 0; i < n; i++) { const uint32_t* w = words + 5 * (size_t)i; out[i] = (uint8_t)ssm_fq::quick4(w[0], w[1], w[2], w[3], w[4], th2, keep); }
    return SSM_OK;
}

extern "C" int ssm_debug_pyramid_plan(const ssm_config* cfg, int bands, int32_t* items, int cap, int* nitems, int32_t* band_tab, int32_t* limits)
{
    if (!cfg || !nitems) return SSM_E_INVAL;
    OrbPlan P; std::string err;
    { const int r = orb_plan_build(*cfg, P, err); if (r) return r; }
    const OrbGeom& g = P.g; const int L = g.nlevels;
    const std::vector<int32_t>* xall = P.xofs; const std::vector<int32_t>* yall = P.yofs; const bool* streaming = P.streaming; const bool* wide_ok = P.wide_ok;
    // bands > 0: that band count; 0 / < 0: the plan a context uses for batches / for the one-frame call
    PyrBandPlan p; std::vector<int32_t> tab; bool ok;
    if (bands > 0) ok = orb_plan_bands(P, bands, tab, p);
    else { const int k = bands == 0 ? 0 : 1; p = P.bands[k]; tab = P.band_tab[k]; ok = p.bands > 0; }
    if (limits) {
        int32_t v[16 + 3 * SSM_MAX_LEVELS] = {ok ? p.bands : 0, (int32_t)p.lds, p.args.buf1, PYR_SLACK, pyramid_block_threads(), PB_MAX_LDS, L};
        for (int l = 1; l < L; l++) { v[7] |= (streaming[l] ? 1 : 0) << l; v[8] |= (wide_ok[l] ? 1 : 0) << l; }
        if (ok) v[9] = (int32_t)p.args.wide;
        for (int l = 0; l < L; l++) { v[16 + 3 * l] = g.L[l].w; v[17 + 3 * l] = g.L[l].h; v[18 + 3 * l] = g.L[l].stride; }
        memcpy(limits, v, sizeof(v));
    }
    *nitems = 0;
    if (!ok) return SSM_OK;                                              // no fused form: limits[0] == 0
    if (band_tab) memcpy(band_tab, tab.data(), tab.size() * 4);
    int n = 0;
    for (int b = 0; b < p.bands; b++)
        for (int l = 1; l < L; l++) {
            const int32_t* rs = &tab[((size_t)b * L + l - 1) * 4]; const int32_t* r = &tab[((size_t)b * L + l) * 4];
            const LevelGeom& A = g.L[l-1]; const LevelGeom& B = g.L[l];
            const int wide = pyr_wide(p.args, l), px = wide ? 8 : 4;
            const PyrItems it = pyr_items(B.stride, wide, r[0], r[1]);
            for (int i = 0; i < it.items; i++, n++) {
                if (!items) continue;
                if (n >= cap) return SSM_E_INVAL;
                /* the rows and windows of item i, as resize4_kernel_bands walks them */
                const int blk = pyr_item_run(i, p.args.mulg[l]), gi = i - blk * it.groups;
                const int x0 = px * gi, base = x0 < B.w ? xall[l][x0] : 0;
                int ylo = 1 << 30, yhi = -1, slo = 1 << 30, shi = -1, rlo = 1 << 30, rhi = -(1 << 30);
                    for (int j = 0; j < 4; j++) {
                        const int y = it.c0 + 4 * blk + j;
                        if (y < r[0] || y > r[1]) continue;
                        ylo = std::min(ylo, y); yhi = std::max(yhi, y);
                        const int sy[2] = {yall[l][y], std::min(yall[l][y] + 1, A.h - 1)};
                        for (int k = 0; k < 2; k++) {
                            const int e = (sy[k] - rs[0]) * A.stride + base;
                            slo = std::min(slo, sy[k]); shi = std::max(shi, sy[k]);
                            rlo = std::min(rlo, e & ~3); rhi = std::max(rhi, (e & ~3) + (wide ? 16 : 12));
                        }
                    }
                const int32_t v[12] = {l, b, px, gi, ylo, yhi, slo, shi, rlo, rhi, (ylo - r[0]) * B.stride + px * gi, (yhi - r[0]) * B.stride + px * gi + px};
                memcpy(items + 12 * (size_t)n, v, sizeof(v));
            }
        }
    *nitems = n;
    return SSM_OK;
}
