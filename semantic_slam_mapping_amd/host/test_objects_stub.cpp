// test_objects_stub.cpp -- the object-extraction entry points of san_stub_device.cpp (what Mapper with mapper_objects=1 calls in a CPU sanitizer build of the host
// layer) as a stand-alone program: linked with the stub and the library's host-only sources, no libssm_hip.so, no GPU; also built with
// -fsanitize=address,undefined.  A grid is built into the stub's grid target from hand-made clouds, stage 1 and stage 2 run on host arrays and on stub "clouds", and
// the fetched records, image and info must be those of ssm_objects_host; the capacity rule of the fetch; a target smaller than the grid.
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
    ssm_objects_params P; ssm_objects_params_default(&P);
    vector<ssm_point> a, b;
    for (int i = 0; i < 2000; i++) a.push_back(gp(-2.0 + 4.0 * (i % 200) / 200.0, 3.0 * (i / 200) / 10.0 + 0.01, -1.5 + 0.001 * (i % 7), 4));          // the ground
    for (int i = 0; i < 600; i++) b.push_back(gp(-1.2 + 0.9 * (i % 30) / 30.0, 0.6 + 0.6 * (i / 30) / 20.0, -1.2 + 0.05 * (i % 19), i % 9 ? 9 : 5));          // a car
    for (int i = 0; i < 100; i++) b.push_back(gp(1.1 + 0.001 * i, 2.1 + 0.001 * i, -1.2 + 0.012 * i, 10));                                                  // a pedestrian in one cell: rejected
    const ssm_point* pts[2] = {a.data(), b.data()}; const int32_t n[2] = {(int32_t)a.size(), (int32_t)b.size()}; double T[32]; memcpy(T, EYE, sizeof EYE); memcpy(T + 16, EYE, sizeof EYE);
    const size_t nc = (size_t)G.nx * G.ny, total = a.size() + b.size();
    vector<ssm_object> want(nc); vector<int32_t> want_id(nc), want_ids(total); ssm_objects_info WI; int K = 0;
    const int rc0 = ssm_objects_host(pts, n, T, 2, &G, &P, want.data(), (int)nc, &K, want_id.data(), want_ids.data(), &WI);
    printf("scene: rc %d, %d kept of %lld components (%lld / %lld / %lld rejected), %lld object points\n", rc0, K, (long long)WI.components, (long long)WI.rejected_cells, (long long)WI.rejected_points,
           (long long)WI.rejected_height, (long long)WI.object_points);
    check(ssm_objects_host(pts, n, T, 2, &G, &P, want.data(), (int)nc, &K, want_id.data(), want_ids.data(), &WI) == SSM_OK && K == 1 && WI.rejected_cells == 1 && want[0].n_points > 100 &&
          want[0].n_label < want[0].n_points, "the scene holds one kept object and one rejected component");
    ssm_grid_target* gt = nullptr; ssm_objects_target *ot = nullptr, *small = nullptr;
    check(ssm_grid_target_create(ctx, G.nx, G.ny, &gt) == SSM_OK && ssm_objects_target_create(ctx, G.nx, G.ny, &ot) == SSM_OK && ssm_objects_target_create(ctx, 4, 4, &small) == SSM_OK &&
          ssm_objects_target_create(ctx, 0, 4, &small) == SSM_E_INVAL, "targets");
    ssm_grid_info GI;
    check(ssm_grid_points(ctx, gt, pts, n, T, 2, &G, &GI) == SSM_OK && GI.n_in == (int64_t)total, "the grid");
    ssm_objects_info I1, I2;
    check(ssm_objects_grid(ctx, gt, &P, small, &I1) == SSM_E_INVAL && ssm_objects_grid(ctx, gt, &P, ot, &I1) == SSM_OK && I1.components == WI.components && I1.kept == 1 && I1.rejected_cells == 1,
          "stage 1, and a target smaller than the grid");
    vector<ssm_object> got(1); vector<int32_t> got_id(nc, -7), ids(total, -7); int k = -7;
    check(ssm_objects_fetch(ctx, ot, got.data(), 1, &k, got_id.data()) == SSM_OK && k == 1 && got[0].root == want[0].root && got[0].cells == want[0].cells && got[0].n_points == 0 &&
          got_id == want_id, "stage 1's records have no points yet");
    check(ssm_objects_points(ctx, gt, ot, pts, n, T, 2, ids.data(), &I2) == SSM_OK && memcmp(&I2, &WI, sizeof WI) == 0 && ids == want_ids, "stage 2 on host arrays");
    check(ssm_objects_fetch(ctx, ot, nullptr, 0, &k, nullptr) == SSM_OK && k == 1 && ssm_objects_fetch(ctx, ot, got.data(), 0, &k, nullptr) == SSM_E_CAPACITY && k == 1 &&
          ssm_objects_fetch(ctx, ot, got.data(), 1, &k, got_id.data()) == SSM_OK && memcmp(got.data(), want.data(), sizeof(ssm_object)) == 0 && got_id == want_id, "the fetch and its capacity rule");
    // stub "clouds": what the stub's back-projection makes of a depth image (its points carry no label, so they form no object)
    vector<uint16_t> depth(64 * 48, 1500); vector<uint8_t> rgb(64 * 48 * 3, 7);
    ssm_cloud* cl = nullptr;
    check(ssm_backproject_dev(ctx, depth.data(), rgb.data(), rgb.data(), 64, 48, &cfg.camera, 40.0, &cl) == SSM_OK && ssm_cloud_size(cl) > 0, "a stub cloud");
    ssm_cloud* list[1] = {cl};
    check(ssm_grid_clouds(ctx, gt, list, EYE, 1, &G, &GI) == SSM_OK && ssm_objects_grid(ctx, gt, &P, ot, &I1) == SSM_OK && I1.kept == 0 &&
          ssm_objects_clouds(ctx, gt, ot, list, EYE, 1, &I2) == SSM_OK && I2.kept == 0 && I2.n_in == ssm_cloud_size(cl) && I2.object_points == 0 &&
          ssm_objects_fetch(ctx, ot, got.data(), 1, &k, got_id.data()) == SSM_OK && k == 0, "stage 2 on stub clouds");
    ssm_cloud_free(ctx, cl); ssm_objects_target_free(ctx, ot); ssm_objects_target_free(ctx, small); ssm_grid_target_free(ctx, gt); ssm_destroy(ctx);
    printf(failures ? "%d FAILED\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
