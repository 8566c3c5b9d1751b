// grid_probe.hip -- a PROBE build of the ground grid's kernels (csrc/kernels_grid.hip compiled with -DGRID_PROBE, which adds two debug counters; the library never
// has them): how many atomics pass A and pass B issue in each accumulate form, for a scene scripts/grid_bench.py writes.
// Build (by the script): hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -DGRID_PROBE scripts/grid_probe.hip -o scripts/grid_probe
// Usage: grid_probe <scene file>  ->  one JSON line.  The scene file: int32 m, 0; ssm_grid_params; then per cloud int32 n, int32 0, 16 doubles pose, n points.
// Its timings mean nothing (the counters are atomics of their own).
#include "../semantic_slam_mapping_amd/csrc/kernels_grid.hip"
#include "../semantic_slam_mapping_amd/csrc/ssm_cloud_table.cpp"          // the table's builder, as the library links it
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(r_)); return 1; } } while (0)

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: grid_probe <scene file>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t hd[2]; ssm_grid_params P;
    if (fread(hd, 4, 2, f) != 2 || fread(&P, sizeof P, 1, f) != 1) { fprintf(stderr, "short scene file\n"); return 2; }
    const int m = hd[0];
    if (m < 1 || m > 64 || P.nx < 1 || P.ny < 1 || (int64_t)P.nx * P.ny > MAX_CELLS || !(P.cell > 0) || P.ground_radius < 0 || P.ground_radius > MAX_GROUND_RADIUS || !(P.step >= 0)) {
        fprintf(stderr, "bad scene file\n"); return 2;
    }
    Setup S; S.x0 = P.x0; S.y0 = P.y0; S.cell = P.cell; S.h_min = P.h_min; S.h_max = P.h_max; S.step_q = step_units(P.step); S.nx = P.nx; S.ny = P.ny;
    S.ground_radius = P.ground_radius; S.min_obstacle_points = P.min_obstacle_points;
    std::vector<CloudSeg> segs((size_t)m, CloudSeg{}); std::vector<ssm_point*> dev((size_t)m, nullptr);
    for (int k = 0; k < m; k++) {
        int32_t n[2]; double Tc[16];
        if (fread(n, 4, 2, f) != 2 || fread(Tc, 8, 16, f) != 16 || n[0] < 0 || n[0] > (1 << 24)) { fprintf(stderr, "bad cloud %d\n", k); return 2; }
        std::vector<ssm_point> pts((size_t)n[0]);
        if (n[0] && fread(pts.data(), sizeof(ssm_point), (size_t)n[0], f) != (size_t)n[0]) { fprintf(stderr, "short cloud %d\n", k); return 2; }
        CK(hipMalloc((void**)&dev[k], (size_t)std::max(n[0], 1) * sizeof(ssm_point)));
        if (n[0]) CK(hipMemcpy(dev[k], pts.data(), (size_t)n[0] * sizeof(ssm_point), hipMemcpyHostToDevice));
        segs[k].pts = dev[k]; segs[k].n = n[0]; segs[k].stride = 1;
        grid_pose(P.G, Tc, segs[k].M);
    }
    fclose(f);
    int64_t nb = 0;
    const int64_t total = cloud_table_build(segs.data(), m, GRID_T, nullptr, &nb), nc = (int64_t)P.nx * P.ny;
    std::vector<int32_t> blk((size_t)nb + 1, 0);
    cloud_table_build(segs.data(), m, GRID_T, blk.data(), &nb);
    CloudSeg* d_seg; int32_t* d_blk; unsigned long long* d_info; GridBufs T;
    CK(hipMalloc((void**)&d_seg, segs.size() * sizeof(CloudSeg))); CK(hipMalloc((void**)&d_blk, blk.size() * 4)); CK(hipMalloc((void**)&d_info, 80));
    CK(hipMalloc((void**)&T.cells, nc * sizeof(ssm_grid_cell))); CK(hipMalloc((void**)&T.cls, nc)); CK(hipMalloc((void**)&T.ground_label, nc)); CK(hipMalloc((void**)&T.obstacle_label, nc));
    CK(hipMalloc((void**)&T.ground_q, nc * 4)); CK(hipMalloc((void**)&T.top_q, nc * 4)); CK(hipMalloc((void**)&T.n, nc * 4)); CK(hipMalloc((void**)&T.n_high, nc * 4));
    CK(hipMemcpy(d_seg, segs.data(), segs.size() * sizeof(CloudSeg), hipMemcpyHostToDevice)); CK(hipMemcpy(d_blk, blk.data(), blk.size() * 4, hipMemcpyHostToDevice));
    unsigned long long cnt[2][2]; long long info[10] = {0};          // (info[1] is the count of rejected points here: the library's caller converts it)
    for (int form = 0; form < 2; form++) {
        const unsigned long long zero[2] = {0, 0};
        CK(hipMemcpyToSymbol(HIP_SYMBOL(grid_probe_counts), zero, 16));
        CK(k_grid(S, d_seg, d_blk, total, T, d_info, form, 0));
        CK(hipDeviceSynchronize());
        CK(hipMemcpyFromSymbol(cnt[form], HIP_SYMBOL(grid_probe_counts), 16)); CK(hipMemcpy(info, d_info, 80, hipMemcpyDeviceToHost));
    }
    printf("{\"points\": %lld, \"used\": %lld, \"cells_hit\": %lld, \"a_points\": %llu, \"b_points\": %llu, \"a_runs\": %llu, \"b_runs\": %llu}\n", (long long)total, info[4],
           (long long)(nc - info[5]), cnt[0][0], cnt[0][1], cnt[1][0], cnt[1][1]);
    for (ssm_point* p : dev) (void)hipFree(p);
    for (void* p : {(void*)d_seg, (void*)d_blk, (void*)d_info, (void*)T.cells, (void*)T.cls, (void*)T.ground_label, (void*)T.obstacle_label, (void*)T.ground_q, (void*)T.top_q, (void*)T.n,
                    (void*)T.n_high}) (void)hipFree(p);
    return 0;
}
