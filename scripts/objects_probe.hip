// objects_probe.hip -- a PROBE build of object extraction's kernels (csrc/kernels_objects.hip compiled with -DOBJECTS_PROBE, which adds one debug counter; the
// library never has it): how many atomics the point pass (stage 2) issues in each accumulate form, for a scene scripts/objects_bench.py writes.
// Build (by the script): hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -DOBJECTS_PROBE scripts/objects_probe.hip -o scripts/objects_probe
// Usage: objects_probe <scene file>  ->  one JSON line.  The scene file: int32 m, nx, ny, K; ssm_grid_params; nx ny raw cells (ssm_grid_cell) of the built grid;
// nx ny int32 object_id; K records (ssm_object) as stage 1 left them; then per cloud int32 n, int32 0, 16 doubles pose, n points.  The grid and stage 1 are the
// host functions' (the script calls them): only the point pass runs here.  Its timings mean nothing (the counter is an atomic of its own).
#include "../semantic_slam_mapping_amd/csrc/kernels_objects.hip"
#include "../semantic_slam_mapping_amd/csrc/ssm_cloud_table.cpp"          // the table's builder, as the library links it
int host_fail(ssm_ctx*, int code, const std::string&) { return code; }          // what the host source asks of its surroundings (csrc/ssm_host.h): nothing fails here
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(r_)); return 1; } } while (0)

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: objects_probe <scene file>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t hd[4]; ssm_grid_params P;
    if (fread(hd, 4, 4, f) != 4 || fread(&P, sizeof P, 1, f) != 1) { fprintf(stderr, "short scene file\n"); return 2; }
    const int m = hd[0], K = hd[3];
    if (m < 1 || m > 64 || hd[1] != P.nx || hd[2] != P.ny || P.nx < 1 || P.ny < 1 || (int64_t)P.nx * P.ny > ssm_gridc::MAX_CELLS || K < 0 || (int64_t)K > (int64_t)P.nx * P.ny || !(P.cell > 0) ||
        !(P.step >= 0)) { fprintf(stderr, "bad scene file\n"); return 2; }
    const size_t nc = (size_t)P.nx * P.ny;
    ssm_gridc::Setup S; S.x0 = P.x0; S.y0 = P.y0; S.cell = P.cell; S.h_min = P.h_min; S.h_max = P.h_max; S.step_q = ssm_gridc::step_units(P.step); S.nx = P.nx; S.ny = P.ny;
    S.ground_radius = P.ground_radius; S.min_obstacle_points = P.min_obstacle_points;
    std::vector<ssm_grid_cell> cells(nc); std::vector<int32_t> oid(nc); std::vector<ssm_object> objs((size_t)K + 1);
    if (fread(cells.data(), sizeof(ssm_grid_cell), nc, f) != nc || fread(oid.data(), 4, nc, f) != nc || (K && fread(objs.data(), sizeof(ssm_object), (size_t)K, f) != (size_t)K)) {
        fprintf(stderr, "short scene file\n"); return 2;
    }
    for (size_t i = 0; i < nc; i++) if (oid[i] < -1 || oid[i] >= K) { fprintf(stderr, "bad object_id\n"); return 2; }          // (the kernel indexes the records with it)
    std::vector<CloudSeg> segs((size_t)m, CloudSeg{}); std::vector<ssm_point*> dev((size_t)m, nullptr);
    for (int k = 0; k < m; k++) {
        int32_t n[2]; double Tc[16];
        if (fread(n, 4, 2, f) != 2 || fread(Tc, 8, 16, f) != 16 || n[0] < 0 || n[0] > (1 << 24)) { fprintf(stderr, "bad cloud %d\n", k); return 2; }
        std::vector<ssm_point> pts((size_t)n[0]);
        if (n[0] && fread(pts.data(), sizeof(ssm_point), (size_t)n[0], f) != (size_t)n[0]) { fprintf(stderr, "short cloud %d\n", k); return 2; }
        CK(hipMalloc((void**)&dev[k], (size_t)std::max(n[0], 1) * sizeof(ssm_point)));
        if (n[0]) CK(hipMemcpy(dev[k], pts.data(), (size_t)n[0] * sizeof(ssm_point), hipMemcpyHostToDevice));
        segs[k].pts = dev[k]; segs[k].n = n[0]; segs[k].stride = 1;
        ssm_gridc::grid_pose(P.G, Tc, segs[k].M);
    }
    fclose(f);
    int64_t nb = 0;
    const int64_t total = cloud_table_build(segs.data(), m, OBJ_T, nullptr, &nb);
    std::vector<int32_t> blk((size_t)nb + 1, 0);
    cloud_table_build(segs.data(), m, OBJ_T, blk.data(), &nb);
    CloudSeg* d_seg; int32_t *d_blk, *d_oid, *d_ids; unsigned long long* d_info; ssm_grid_cell* d_cells; ssm_object* d_objs;
    CK(hipMalloc((void**)&d_seg, segs.size() * sizeof(CloudSeg))); CK(hipMalloc((void**)&d_blk, blk.size() * 4)); CK(hipMalloc((void**)&d_info, 64));
    CK(hipMalloc((void**)&d_cells, nc * sizeof(ssm_grid_cell))); CK(hipMalloc((void**)&d_oid, nc * 4)); CK(hipMalloc((void**)&d_objs, objs.size() * sizeof(ssm_object)));
    CK(hipMalloc((void**)&d_ids, (size_t)std::max<int64_t>(total, 1) * 4));
    CK(hipMemcpy(d_seg, segs.data(), segs.size() * sizeof(CloudSeg), hipMemcpyHostToDevice)); CK(hipMemcpy(d_blk, blk.data(), blk.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_cells, cells.data(), nc * sizeof(ssm_grid_cell), hipMemcpyHostToDevice)); CK(hipMemcpy(d_oid, oid.data(), nc * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_objs, objs.data(), objs.size() * sizeof(ssm_object), hipMemcpyHostToDevice)); CK(hipMemset(d_info, 0, 64));
    unsigned long long cnt[2] = {0, 0}; long long info[8] = {0}; std::vector<ssm_object> got[2];
    for (int form = 0; form < 2; form++) {
        const unsigned long long zero = 0;
        CK(hipMemcpyToSymbol(HIP_SYMBOL(objects_probe_count), &zero, 8));
        CK(k_objects_points(S, d_seg, d_blk, total, d_cells, d_oid, d_objs, K, d_ids, d_info, form, 0));
        CK(hipDeviceSynchronize());
        CK(hipMemcpyFromSymbol(&cnt[form], HIP_SYMBOL(objects_probe_count), 8)); CK(hipMemcpy(info, d_info, 64, hipMemcpyDeviceToHost));
        got[form].resize(objs.size()); CK(hipMemcpy(got[form].data(), d_objs, objs.size() * sizeof(ssm_object), hipMemcpyDeviceToHost));
    }
    const bool same = memcmp(got[0].data(), got[1].data(), (size_t)K * sizeof(ssm_object)) == 0;
    printf("{\"points\": %lld, \"object_points\": %lld, \"objects\": %d, \"atomics_points\": %llu, \"atomics_runs\": %llu, \"forms_agree\": %s}\n", (long long)total, info[7], K, cnt[0], cnt[1],
           same ? "true" : "false");
    for (ssm_point* p : dev) (void)hipFree(p);
    for (void* p : {(void*)d_seg, (void*)d_blk, (void*)d_info, (void*)d_cells, (void*)d_oid, (void*)d_objs, (void*)d_ids}) (void)hipFree(p);
    return same ? 0 : 1;
}
