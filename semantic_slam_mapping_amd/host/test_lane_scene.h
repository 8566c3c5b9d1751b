// test_lane_scene.h -- the ray-cast scene of test_align, test_grid and test_relabel: a KITTI-layout camera (400 x 120) drives N key-frames of STEP metres down a
// lane of half-width LANE on the ground plane y = GROUND, pavement beside it, one box on the right.
#pragma once
#include "test_mapper_common.h"
static const int W = 400, H = 120, N = 8;
static const double STEP = 0.5, GROUND = 1.6, BOX_LO[3] = {1.5, 0.4, 9.0}, BOX_HI[3] = {3.0, 1.6, 12.0}, LANE = 1.0;
enum { HIT_NONE = 0, HIT_ROAD = 1, HIT_PAVEMENT = 2, HIT_BOX = 3 };
// the depth image from a camera at (0, 0, z0) looking along +z: the ground y = GROUND and the box; beyond 65 m: no depth.  hit (may be null): what every pixel's ray met
static inline void cast(double z0, const CAMERA_INTRINSIC_PARAMETERS& cam, cv::Mat& depth, vector<uint8_t>* hit = nullptr)
{
    depth.create(H, W, CV_16UC1);
    if (hit) hit->assign((size_t)W * H, HIT_NONE);
    const double o[3] = {0.0, 0.0, z0};
    for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) {
        const double dir[3] = {(x - cam.cx) / cam.fx, (y - cam.cy) / cam.fy, 1.0};
        double best = 1e30; int what = HIT_NONE;
        if (dir[1] > 0) { best = (GROUND - o[1]) / dir[1]; what = fabs(o[0] + best * dir[0]) < LANE ? HIT_ROAD : HIT_PAVEMENT; }
        double near = -1e30, far = 1e30;
        for (int a = 0; a < 3; a++) {
            if (dir[a] == 0.0) { if (o[a] < BOX_LO[a] || o[a] > BOX_HI[a]) { near = 1e30; } continue; }
            double t0 = (BOX_LO[a] - o[a]) / dir[a], t1 = (BOX_HI[a] - o[a]) / dir[a];
            if (t0 > t1) swap(t0, t1);
            near = max(near, t0); far = min(far, t1);
        }
        if (near <= far && near > 1e-6 && near < best) { best = near; what = HIT_BOX; }
        const double units = best * cam.scale;
        const bool ok = units >= 1.0 && units <= 65535.0;
        depth.ptr<uint16_t>(y)[x] = ok ? (uint16_t)llrint(units) : (uint16_t)0;
        if (hit) (*hit)[(size_t)y * W + x] = ok ? (uint8_t)what : (uint8_t)HIT_NONE;
    }
}
