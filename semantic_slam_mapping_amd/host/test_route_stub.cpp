// test_route_stub.cpp -- the route entry points of san_stub_device.cpp (what Mapper with mapper_route=1 calls in a CPU sanitizer build of the host layer) as a
// stand-alone program: linked with the stub and the library's host-only sources, no libssm_hip.so, no GPU; also built with -fsanitize=address,undefined.  A grid is
// built into the stub's grid target from hand-made clouds, the clearance call runs on it, the route field on that; the fetched field, the info and a path must be
// those of the host functions on the fetched clearance images from the clearance call's seed under the grid's cell size; a target smaller than the grid; a fetch
// and a path before any field; a path longer than max_path.
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
    ssm_grid_target* gt = nullptr; ssm_clearance_target* ct = nullptr; ssm_route_target *rt = nullptr, *small = nullptr, *brief = nullptr;
    check(ssm_grid_target_create(ctx, G.nx, G.ny, &gt) == SSM_OK && ssm_clearance_target_create(ctx, G.nx, G.ny, &ct) == SSM_OK && ssm_route_target_create(ctx, G.nx, G.ny, (int)nc, &rt) == SSM_OK &&
          ssm_route_target_create(ctx, 4, 4, 16, &small) == SSM_OK && ssm_route_target_create(ctx, G.nx, G.ny, 3, &brief) == SSM_OK && ssm_route_target_create(ctx, 0, 4, 4, &small) == SSM_E_INVAL &&
          ssm_route_target_create(ctx, 4, 4, 0, &small) == SSM_E_INVAL, "targets");
    vector<uint32_t> cost(nc, 7), wcost(nc), d2(nc); vector<int32_t> parent(nc, -7), wparent(nc), cells(nc, -7), wcells(nc, -7); vector<uint8_t> reach(nc), cls(nc);
    ssm_route_path_info PI, WPI;
    check(ssm_route_fetch(ctx, rt, cost.data(), parent.data()) == SSM_E_INVAL && cost[0] == 7 && ssm_route_path(ctx, rt, 0, 0, 0, cells.data(), &PI) == SSM_E_INVAL, "a fetch and a path before any field");
    ssm_grid_info GI;
    check(ssm_grid_points(ctx, gt, pts, n, T, 2, &G, &GI) == SSM_OK && ssm_grid_fetch(ctx, gt, cls.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SSM_OK, "the grid");
    ssm_clearance_params CP; ssm_clearance_params_default(&CP); CP.radius = 0.5; CP.seed_cx = 8; CP.seed_cy = 1;
    ssm_clearance_info CI;
    ssm_route_params P; ssm_route_params_default(&P); P.comfort = 1.0; P.near_weight = 3; P.cell = 99.0;          // (the clearance call's cell size counts, not this one)
    ssm_route_info I, WI;
    check(ssm_route_field(ctx, ct, &P, rt, &I) == SSM_E_INVAL, "a field before any clearance call");
    check(ssm_clearance_grid(ctx, gt, &CP, ct, &CI) == SSM_OK && ssm_clearance_fetch(ctx, ct, d2.data(), nullptr, reach.data()) == SSM_OK && CI.seed_cell >= 0 && CI.reachable > 0, "the clearance map");
    ssm_route_params H = P; H.cell = G.cell;
    check(ssm_route_cells_host(reach.data(), d2.data(), G.nx, G.ny, (int)CI.seed_cell, &H, wcost.data(), wparent.data(), &WI) == SSM_OK && WI.routed > 1 && WI.routed + WI.unrouted == CI.reachable &&
          WI.comfort2 == 16 && WI.near_cells > 0 && WI.near_cells < WI.routed, "the scene routes round a car, some of the way near it");
    printf("scene: %lld routed, %lld unrouted, %lld near, max cost %lld at %lld\n", (long long)WI.routed, (long long)WI.unrouted, (long long)WI.near_cells, (long long)WI.max_cost, (long long)WI.far_cell);
    check(ssm_route_field(ctx, ct, &P, small, &I) == SSM_E_INVAL && ssm_route_field(ctx, ct, &P, rt, &I) == SSM_OK && memcmp(&I, &WI, sizeof I) == 0, "the call, and a target smaller than the grid");
    check(ssm_route_fetch(ctx, rt, cost.data(), parent.data()) == SSM_OK && cost == wcost && parent == wparent && ssm_route_fetch(ctx, rt, nullptr, nullptr) == SSM_OK, "the fetched field is the host function's");
    const int fx = (int)(WI.far_cell % G.nx), fy = (int)(WI.far_cell / G.nx);
    check(ssm_route_path_host(wcost.data(), wparent.data(), d2.data(), G.nx, G.ny, &H, fx, fy, 0, (int)nc, wcells.data(), &WPI) == SSM_OK && WPI.len > 3 && WPI.cost == WI.max_cost &&
          ssm_route_path(ctx, rt, fx, fy, 0, cells.data(), &PI) == SSM_OK && memcmp(&PI, &WPI, sizeof PI) == 0 && cells == wcells && cells[0] == (int32_t)CI.seed_cell &&
          cells[(size_t)PI.len - 1] == (int32_t)WI.far_cell, "the path to the farthest cell is the host function's");
    check(ssm_route_field(ctx, ct, &P, brief, &I) == SSM_OK && ssm_route_path(ctx, brief, fx, fy, 0, cells.data(), &PI) == SSM_E_CAPACITY && PI.len == WPI.len && cells == wcells, "a path longer than max_path");
    P.moves = 5;
    check(ssm_route_field(ctx, ct, &P, rt, &I) == SSM_E_INVAL && ssm_route_fetch(ctx, rt, cost.data(), nullptr) == SSM_OK && cost == wcost, "a refused call leaves the target as it was");
    ssm_route_target_free(ctx, rt); ssm_route_target_free(ctx, small); ssm_route_target_free(ctx, brief); ssm_clearance_target_free(ctx, ct); ssm_grid_target_free(ctx, gt); ssm_destroy(ctx);
    printf(failures ? "%d FAILED\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
