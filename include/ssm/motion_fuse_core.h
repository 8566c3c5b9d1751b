// motion_fuse_core.h -- the arithmetic of the semantic-motion fusion (reference src/mapper.cpp:217-271, with the Car class of src/mapper.cpp~:146-229), compiled
// for host and device like uvd_core.h and pgo_core.h: csrc/kernels_motion_fuse.hip and the host function of csrc/ssm_motion_fuse_host.cpp call the same functions,
// so device == host bit for bit.  Everything is integer except the one float division of the overlap test, which is written with the
// reference's operand types: float / float, widened to double for the compare.  Every translation unit that includes this is built with -ffp-contract=off.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define MF_HD __host__ __device__ inline
#else
#define MF_HD inline
#endif

namespace ssm_mfc {

// the tile of the device labelling (csrc/kernels_motion_fuse.hip): blobs are labelled inside TILE_W x TILE_H tiles in LDS and joined over the tile borders in
// global memory.  The host function has no tiles; the constants are here because the tests place their sizes and shapes around them (ssm_motion_fuse_tile)
static const int TILE_W = 64, TILE_H = 16;
enum { CLASS_ALWAYS = 1, CLASS_CAND = 2 };

// the classes of one BGR pixel of the semantic image: Pedestrian (0,64,64) and Bicyclist (192,128,0) always move (mapper.cpp:196-197) and are candidates too;
// Car (128,0,64) is a candidate only (mapper.cpp~:163)
MF_HD int class_bits(int b, int g, int r)
{
    if ((b == 0 && g == 64 && r == 64) || (b == 192 && g == 128 && r == 0)) return CLASS_ALWAYS | CLASS_CAND;
    if (b == 128 && g == 0 && r == 64) return CLASS_CAND;
    return 0;
}
// only the motion mask's 255 counts as motion (the mask is 0 / 255; countNonZero of mask & motion, mapper.cpp:252-254)
MF_HD int motion_hit(uint8_t m) { return m == 255; }
MF_HD int is_large(int32_t area, int32_t area_thres) { return area > area_thres; }
// mapper.cpp:255-258: `float overlay = countNonZero(overlap) * 1.0f / mask_count; if (area > thres && overlay > overlay_thres)` with mask_count one more than
// the blob's pixels (the reference counts from 1) and overlay_thres a double: the quotient is rounded to float first, then compared in double
MF_HD int confirmed(int32_t area, int32_t overlap, int32_t area_thres, double overlay_thres)
{
    const int32_t mask_count = area + 1;
    const float overlay = (float)overlap * 1.0f / (float)mask_count;
    return is_large(area, area_thres) && (double)overlay > overlay_thres;
}

}      // namespace ssm_mfc
