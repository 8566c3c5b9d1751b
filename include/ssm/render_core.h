// render_core.h -- the arithmetic of map rendering: the points of m posed clouds are splatted, z-buffered, into a pinhole view, and the rendering is
// compared per pixel with a key-frame's own depth and semantic image.  Compiled for host and device like carve_core.h: csrc/kernels_render.hip and the host
// functions of csrc/ssm_render_host.cpp call the same functions, so device == host bit for bit.  Every translation unit that includes this is built with
// -ffp-contract=off.  The relative pose is carve_core.h's rel_pose (host only, evaluated ONCE per view and cloud; both paths are handed its 12 doubles), the
// comparison's tolerance is carving's.  What is here: a point's splat (centre pixel, half width, quantised depth), its key, the class of a pixel of the
// comparison, and the 12-class palette in both directions.  The reference has no such step.
#pragma once
#include "carve_core.h"

namespace ssm_renderc {

static const int MAX_RADIUS = 8;
static const int64_t MAX_PIXELS = (int64_t)1 << 26;
static const uint64_t KEY_EMPTY = ~(uint64_t)0;                 // a pixel no point has reached
enum { UNRENDERED = 0, NO_DEPTH = 1, IN_FRONT = 2, BEHIND = 3, AGREE = 4 };          // the class image's values
enum { LABEL_NONE = 0, LABEL_AGREE = 1, LABEL_DISAGREE = 2, LABEL_UNKNOWN = 3 };     // among the AGREE pixels

// what a call's parameters and the view's camera become once.  half: (0.5 fx) point_size, the numerator of a splat's half width
struct Setup { double fx, fy, cx, cy, scale, z_min, z_max, point_size, half; int32_t w, h, max_radius, pad; };
struct Splat { int32_t x0, x1, y0, y1; uint32_t zq; };          // the footprint, clipped to the image (inclusive), and the quantised depth

// the splat of the point (x, y, z) of a cloud whose relative pose is M; false: the point is invisible
CARVE_HD bool splat_of(float xf, float yf, float zf, const double* M, const Setup& S, Splat* out)
{
    using ssm_carvec::finite_d;
    const double x = (double)xf, y = (double)yf, z = (double)zf;
    if (!(finite_d(x) && finite_d(y) && finite_d(z))) return false;
    const double qx = M[0] * x + M[1] * y + M[2] * z + M[3];
    const double qy = M[4] * x + M[5] * y + M[6] * z + M[7];
    const double qz = M[8] * x + M[9] * y + M[10] * z + M[11];
    if (!(finite_d(qx) && finite_d(qy) && finite_d(qz)) || qz < S.z_min || qz > S.z_max) return false;
    const double u = S.fx * (qx / qz) + S.cx, v = S.fy * (qy / qz) + S.cy;
    const double pxd = floor(u + 0.5), pyd = floor(v + 0.5);
    const double r = (double)S.max_radius;
    // (the comparisons are false for NaN; only a value that passes ever becomes an int)
    if (!(pxd >= -r && pxd <= (double)(S.w - 1) + r && pyd >= -r && pyd <= (double)(S.h - 1) + r)) return false;
    const int px = (int)pxd, py = (int)pyd;
    const double zs = qz * S.scale;                               // (0 <= qz <= z_max <= 1e9 and scale <= 1e6: below 2^63)
    if (!(zs < 65536.0)) return false;
    const long long zq = llrint(zs);
    if (zq < 1 || zq > 65535) return false;
    int s = 0;
    if (S.point_size > 0.0) {
        const double t = S.half / qz;                             // (qz > 0 here: zq >= 1)
        s = t >= r ? S.max_radius : t >= 1.0 ? (int)floor(t) : 0;          // (t below 1, a negative one under a mirrored camera included, is one pixel)
    }
    const int x0 = px - s > 0 ? px - s : 0, x1 = px + s < S.w - 1 ? px + s : S.w - 1;
    const int y0 = py - s > 0 ? py - s : 0, y1 = py + s < S.h - 1 ? py + s : S.h - 1;
    if (x0 > x1 || y0 > y1) return false;
    out->x0 = x0; out->x1 = x1; out->y0 = y0; out->y1 = y1; out->zq = (uint32_t)zq;
    return true;
}
// nearest wins; at equal quantised depth the lowest index of the concatenation wins
CARVE_HD uint64_t key_of(uint32_t zq, uint32_t idx) { return ((uint64_t)zq << 32) | (uint64_t)idx; }

// the class of one pixel: zr the rendered depth, d the frame's, lr / lf the labels; *lab gets LABEL_NONE unless the class is AGREE
CARVE_HD int class_of(uint16_t zr, uint16_t d16, uint8_t lr, uint8_t lf, int64_t tol_abs, int64_t ppm, int* lab)
{
    *lab = LABEL_NONE;
    if (zr == 0) return UNRENDERED;
    if (d16 == 0) return NO_DEPTH;
    const int64_t d = d16, z = zr;
    const int64_t tol = tol_abs + (d * ppm) / 1000000;           // carving's tolerance (carve_core.h verdict_of), tol_abs from tol_abs_units
    if (z + tol < d) return IN_FRONT;
    if (z > d + tol) return BEHIND;
    *lab = (lr == lf && lr != 255) ? LABEL_AGREE : (lr != 255 && lf != 255) ? LABEL_DISAGREE : LABEL_UNKNOWN;
    return AGREE;
}

// the project's 12-class palette (tests/golden/palette.json; the table of kernels_map.hip's label_of_bgr24), b | g << 8 | r << 16
CARVE_HD uint32_t bgr24_of_label(uint32_t label)
{
    switch (label) {
        case 0: return 128u | (128u << 8) | (128u << 16);   case 1: return 0u | (0u << 8) | (128u << 16);
        case 2: return 128u | (192u << 8) | (192u << 16);   case 3: return 0u | (69u << 8) | (255u << 16);
        case 4: return 128u | (64u << 8) | (128u << 16);    case 5: return 222u | (40u << 8) | (60u << 16);
        case 6: return 0u | (128u << 8) | (128u << 16);     case 7: return 128u | (128u << 8) | (192u << 16);
        case 8: return 128u | (64u << 8) | (64u << 16);     case 9: return 128u | (0u << 8) | (64u << 16);
        case 10: return 0u | (64u << 8) | (64u << 16);      case 11: return 192u | (128u << 8) | (0u << 16);
    }
    return 0;          // 255 and everything else: black
}
CARVE_HD uint8_t label_of_bgr24(uint32_t bgr)
{
    for (uint32_t l = 0; l < 12; l++) if (bgr24_of_label(l) == bgr) return (uint8_t)l;
    return 255;
}

}      // namespace ssm_renderc
