// uvd_core.h -- the per-pixel arithmetic of UVDisparity::Process (reference src/uvdisparity.cpp:842-903) and of the three functions of src/stereo.cpp it
// depends on (triangulate10D :41-118, correct3DPoints :127-181, setImageROI :183-192), compiled for host and device like looper_core.h and pnp_core.h:
// csrc/kernels_uvd.hip and the host pipeline of csrc/ssm_uvd_host.cpp call the same functions, so device == host bit for bit.  Operand types are
// restated as the reference writes them; the functions use IEEE + - * /, conversions and round-to-nearest-even only, and every translation unit that includes
// this is built with -ffp-contract=off.  cos, sin, atan, atan2 and exp never appear here: the host evaluates them and hands the numbers over (FrameK, the rate
// table).  The 10-channel xyz image is never materialised: channels 0-2, 5, 6 and 9 are computed where they are consumed.
#pragma once
#include <stdint.h>
#include <math.h>
#if defined(__HIPCC__)
#define UVD_HD __host__ __device__ inline
#else
#define UVD_HD inline
#endif

namespace ssm_uvdc {

enum { STATUS_TOO_LARGE = 1, STATUS_NO_LINE = 2, STATUS_SKIPPED = 4 };       // ssm_uvd_info.status
static const int MAX_BINS = 256;            // disparities 0 < d / 16 <= 255: one row of the V-disparity image, one column of the U-disparity image
static const int MAX_RAW = 255 * 16;        // a frame whose largest raw disparity is above this sets STATUS_TOO_LARGE

struct Calib { double f, cu, cv, base; };                 // CalibPars
struct Roi { double x_max, y_max, z_max; };               // ROI3D
// what host step 1 hands to the per-pixel stages of one frame
struct FrameK {
    double v_c, cos_p, sin_p;       // the ground line's intercept (uvdisparity.cpp:447); cos / sin of Kalman filter 1's state (stereo.cpp:130-131)
    float slope;                    // b / a (uvdisparity.cpp:478-481)
    int32_t u_rows, min_disp;       // cvCeil(max / 16) + 1 (uvdisparity.cpp:202); the frame's smallest raw disparity (stereo.cpp:58)
    int32_t run;                    // 0: the frame produces zero masks (skipped, NO_LINE, TOO_LARGE); host step 2 clears it when no mask survives
};

// cvRound: round half to even (the SSE2 cvtsd2si path of OpenCV 2.4)
UVD_HD int cv_round(double v) { return (int)rint(v); }

// triangulate10D, channels 0-2 (stereo.cpp:78-88): double products with 16.0f, cast to float
UVD_HD void triangulate(int i, int j, short d, int min_disp, const Calib& c, float& x, float& y, float& z)
{
    const double pw = c.base / (1.0 * static_cast<double>(d));
    double px = ((static_cast<double>(j) - c.cu) * pw) * 16.0f;
    double py = ((static_cast<double>(i) - c.cv) * pw) * 16.0f;
    double pz = (c.f * pw) * 16.0f;
    if ((int)d == min_disp) { px = INFINITY; py = INFINITY; pz = INFINITY; }        // fabs(d - minDisparity) <= FLT_EPSILON on integers
    x = (float)px; y = (float)py; z = (float)pz;
}
// channel 5
UVD_HD float disparity_real(short d) { return (float)d / 16.0f; }

// correct3DPoints + setImageROI (stereo.cpp:143-176, :183-192): the pixel stays in the ROI mask (with its intensity) when this holds
UVD_HD bool roi_gate(float xp, float yp, float zp, short d, double cos_p, double sin_p, const Roi& r)
{
    const int dr = cv_round(disparity_real(d));
    if (!(dr > 0 && dr < 100)) return false;
    const float y2 = (float)(cos_p * yp + sin_p * zp);
    const float z2 = (float)(cos_p * zp - sin_p * yp);
    return !(xp > r.x_max || y2 > r.y_max || z2 > r.z_max);
}
UVD_HD uint8_t roi_pixel(int i, int j, short d, uint8_t intensity, const FrameK& k, const Calib& c, const Roi& r)
{
    float x, y, z;
    triangulate(i, j, d, k.min_disp, c, x, y, z);
    return roi_gate(x, y, z, d, k.cos_p, k.sin_p, r) ? intensity : (uint8_t)0;
}

// Pitch_Classify's per-pixel part (uvdisparity.cpp:478-508): the two d branches are identical, so d > 8 decides.  `distance` is what the tests bound away from -14
UVD_HD float ground_distance(int i, short d, float slope, double v_c)
{
    const float v = (float)i, dd = disparity_real(d);
    return (float)((v - slope * dd) - v_c);
}
UVD_HD uint8_t ground_pixel(int i, short d, uint8_t intensity, float slope, double v_c)       // channel 9 through convertScaleAbs: the pixel's intensity where it is an obstacle
{
    if (!(disparity_real(d) > 8.0f)) return 0;
    return ground_distance(i, d, slope, v_c) > -14.0f ? (uint8_t)0 : intensity;
}

// calVDisparity's bin (uvdisparity.cpp:305-310): -1 = no count.  The clamp to v_cols only ever moves a value onto v_cols itself, one past the row's end: the
// count is dropped, which host step 1 does by clearing the columns from v_cols on
UVD_HD int v_bin(short d)
{
    if (!(d > 0)) return -1;
    const int dis = cv_round(d / 16.0f);
    return dis < MAX_BINS ? dis : -1;
}
// calUDisparity's bin (uvdisparity.cpp:216-225): the integer division of cvRound(d / 16); -1 = no count
UVD_HD int u_bin(short d, uint8_t roi, uint8_t ground)
{
    if (!(d > 0)) return -1;
    const int dis = cv_round(d / 16);
    return (roi > 0 && ground > 0 && dis > 0 && dis < MAX_BINS) ? dis : -1;
}
// the u8 images (uvdisparity.cpp:236-247, :319-333): scale = 255 * 1.0f / rows (U) or / cols (V)
UVD_HD float hist_scale(int extent) { return 255 * 1.0f / extent; }
UVD_HD uint8_t hist_u8(int count, float scale) { return (uint8_t)(int)(count * scale); }
// adjustUdisIntense (uvdisparity.cpp:820-831): rate = the row's entry of the sigmoid table
UVD_HD uint8_t u_adjust(uint8_t intense, double rate)
{
    const double intense_new = (int)intense * 1.0f * rate;
    const int v = cv_round(intense_new);
    return v > 255 ? (uint8_t)255 : (uint8_t)v;
}

// segmentation (uvdisparity.cpp:906-963) per pixel (k, j), j >= 1: some row i >= 1 of the union mask has column j set with |disp / 16.0f - i| < 1.5.
// uni: u_rows x w bytes
UVD_HD bool moving_test(short d, uint8_t roi, int j, const uint8_t* uni, int u_rows, int w)
{
    if (!(roi > 0) || j < 1) return false;
    const double dis_real = (d / 16.0f);
    int lo = (int)dis_real - 2, hi = (int)dis_real + 2;          // every i with |dis_real - i| < 1.5 lies in here
    if (lo < 1) lo = 1;
    if (hi > u_rows - 1) hi = u_rows - 1;
    for (int i = lo; i <= hi; i++)
        if (uni[(size_t)i * w + j] != 0 && fabs(dis_real - i) < 1.5) return true;
    return false;
}

}  // namespace ssm_uvdc
