// test_clearance_stub.cpp -- the clearance entry points of san_stub_device.cpp (what Mapper with mapper_clearance=1 calls in a CPU sanitizer build of the host layer)
// as a stand-alone program: linked with the stub and the library's host-only sources, no libssm_hip.so, no GPU; also built with -fsanitize=address,undefined.  A
// grid is built into the stub's grid target from hand-made clouds, the clearance call runs on it, and the fetched images and the info must be those of
// ssm_clearance_cells_host on the fetched class image under the grid's cell size; a target smaller than the grid; a fetch before any call.
#include "ssm_hip.h"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace std;
static int failures = 0;
static void check(bool ok, const char* name) { printf("%s %s\n", ok ? "PASS" : "FAIL", name); if (!ok) failures++; }
static const double EYE[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
// a point at grid coordinates under the default G and the identity pose: world (gx, -gz, gy)
static ssm_point gp(double gx, double gy, double gz, uint32_t label)
{ ssm_point p; memset(&p, 0, sizeof p); p.x = (float)gx; p.y = (float)-gz; p.z = (float)gy; p.w = 1.0f; p.label = label; return p; }

int main()
{
    ssm_config cfg; ssm_config_default(&cfg);
    ssm_ctx* ctx = nullptr;
    if (ssm_create(0, &cfg, &ctx) != SSM_OK) { printf("FAIL ssm_create\n"); return 1; }
    ssm_grid_params G; ssm_grid_params_default(&G); G.x0 = -2.0; G.y0 = 0.0; G.cell = 0.25; G.nx = 16; G.ny = 12; G.step = 0.25; G.min_obstacle_points = 2;
    vector<ssm_point> a, b;
    for (int i = 0; i < 2000; i++) a.push_back(gp(-2.0 + 4.0 * (i % 200) / 200.0, 3.0 * (i / 200) / 10.0 + 0.01, -1.5 + 0.001 * (i % 7), 4));          // the road
    for (int i = 0; i < 600; i++) b.push_back(gp(-1.2 + 0.9 * (i % 30) / 30.0, 0.6 + 0.6 * (i / 30) / 20.0, -1.2 + 0.05 * (i % 19), 9));                   // a car on it
    const ssm_point* pts[2] = {a.data(), b.data()}; const int32_t n[2] = {(int32_t)a.size(), (int32_t)b.size()}; double T[32]; memcpy(T, EYE, sizeof EYE); memcpy(T + 16, EYE, sizeof EYE);
    const size_t nc = (size_t)G.nx * G.ny;
    ssm_grid_target* gt = nullptr; ssm_clearance_target *ct = nullptr, *small = nullptr;
    check(ssm_grid_target_create(ctx, G.nx, G.ny, &gt) == SSM_OK && ssm_clearance_target_create(ctx, G.nx, G.ny, &ct) == SSM_OK && ssm_clearance_target_create(ctx, 4, 4, &small) == SSM_OK &&
          ssm_clearance_target_create(ctx, 0, 4, &small) == SSM_E_INVAL, "targets");
    vector<uint32_t> d2(nc, 7), wd2(nc); vector<int32_t> near(nc, -7), wnear(nc); vector<uint8_t> reach(nc, 77), wreach(nc), cls(nc);
    check(ssm_clearance_fetch(ctx, ct, d2.data(), near.data(), reach.data()) == SSM_E_INVAL && d2[0] == 7, "a fetch before any call");
    ssm_grid_info GI;
    check(ssm_grid_points(ctx, gt, pts, n, T, 2, &G, &GI) == SSM_OK && ssm_grid_fetch(ctx, gt, cls.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SSM_OK, "the grid");
    ssm_clearance_params P; ssm_clearance_params_default(&P); P.radius = 0.5; P.seed_cx = 8; P.seed_cy = 1; P.cell = 99.0;          // (the grid's cell size counts, not this one)
    ssm_clearance_params H = P; H.cell = G.cell;
    ssm_clearance_info I, WI;
    check(ssm_clearance_cells_host(cls.data(), G.nx, G.ny, &H, wd2.data(), wnear.data(), wreach.data(), &WI) == SSM_OK && WI.blocked > 0 && WI.r2 == 4 && WI.reachable > 0 && WI.reachable < WI.free_cells,
          "the scene holds a blocked car on a road, part of which is reachable");
    printf("scene: %lld blocked, %lld free, %lld traversable, %lld reachable, %lld components\n", (long long)WI.blocked, (long long)WI.free_cells, (long long)WI.traversable, (long long)WI.reachable, (long long)WI.components);
    check(ssm_clearance_grid(ctx, gt, &P, small, &I) == SSM_E_INVAL && ssm_clearance_grid(ctx, gt, &P, ct, &I) == SSM_OK && memcmp(&I, &WI, sizeof I) == 0, "the call, and a target smaller than the grid");
    check(ssm_clearance_fetch(ctx, ct, d2.data(), near.data(), reach.data()) == SSM_OK && d2 == wd2 && near == wnear && reach == wreach && ssm_clearance_fetch(ctx, ct, nullptr, nullptr, nullptr) == SSM_OK,
          "the fetched images are the host function's");
    P.connectivity = 5;
    check(ssm_clearance_grid(ctx, gt, &P, ct, &I) == SSM_E_INVAL && ssm_clearance_fetch(ctx, ct, d2.data(), nullptr, nullptr) == SSM_OK && d2 == wd2, "a refused call leaves the target as it was");
    ssm_clearance_target_free(ctx, ct); ssm_clearance_target_free(ctx, small); ssm_grid_target_free(ctx, gt); ssm_destroy(ctx);
    printf(failures ? "%d FAILED\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
