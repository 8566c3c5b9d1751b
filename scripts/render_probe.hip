// render_probe.hip -- a PROBE build of the splat kernel (csrc/kernels_render.hip compiled with -DRENDER_PROBE, which adds two debug counters; the library never
// has them): how many footprint pixels were offered a key and how many atomics were issued after the plain load, for a scene scripts/render_bench.py writes.
// Build (by the script): hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -DRENDER_PROBE scripts/render_probe.hip -o scripts/render_probe
// Usage: render_probe <scene file>  ->  one JSON line.  The scene file: int32 w, h, m, 0; 5 doubles camera (cx cy fx fy scale); 16 doubles T_view;
// ssm_render_params; then per cloud int32 n, int32 0, 16 doubles pose, n points.  Its timings mean nothing (the counters are atomics of their own).
#include "../semantic_slam_mapping_amd/csrc/kernels_render.hip"
#include "../semantic_slam_mapping_amd/csrc/ssm_cloud_table.cpp"          // the table's builder, as the library links it
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(r_)); return 1; } } while (0)

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: render_probe <scene file>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t hd[4]; double cam[5], Tv[16]; ssm_render_params P;
    if (fread(hd, 4, 4, f) != 4 || fread(cam, 8, 5, f) != 5 || fread(Tv, 8, 16, f) != 16 || fread(&P, sizeof P, 1, f) != 1) { fprintf(stderr, "short scene file\n"); return 2; }
    const int w = hd[0], h = hd[1], m = hd[2];
    if (w < 1 || h < 1 || (int64_t)w * h > MAX_PIXELS || m < 1 || m > 64 || P.max_radius < 0 || P.max_radius > MAX_RADIUS) { fprintf(stderr, "bad scene file\n"); return 2; }
    Setup S; S.cx = cam[0]; S.cy = cam[1]; S.fx = cam[2]; S.fy = cam[3]; S.scale = cam[4]; S.z_min = P.z_min; S.z_max = P.z_max; S.point_size = P.point_size;
    S.half = (0.5 * S.fx) * P.point_size; S.w = w; S.h = h; S.max_radius = P.max_radius; S.pad = 0;
    std::vector<CloudSeg> segs((size_t)m, CloudSeg{}); std::vector<ssm_point*> dev((size_t)m, nullptr);
    for (int k = 0; k < m; k++) {
        int32_t n[2]; double Tc[16];
        if (fread(n, 4, 2, f) != 2 || fread(Tc, 8, 16, f) != 16 || n[0] < 0 || n[0] > (1 << 24)) { fprintf(stderr, "bad cloud %d\n", k); return 2; }
        std::vector<ssm_point> pts((size_t)n[0]);
        if (n[0] && fread(pts.data(), sizeof(ssm_point), (size_t)n[0], f) != (size_t)n[0]) { fprintf(stderr, "short cloud %d\n", k); return 2; }
        CK(hipMalloc((void**)&dev[k], (size_t)std::max(n[0], 1) * sizeof(ssm_point)));
        if (n[0]) CK(hipMemcpy(dev[k], pts.data(), (size_t)n[0] * sizeof(ssm_point), hipMemcpyHostToDevice));
        segs[k].pts = dev[k]; segs[k].n = n[0]; segs[k].stride = 1;
        ssm_carvec::rel_pose(Tv, Tc, segs[k].M);
    }
    fclose(f);
    int64_t nb = 0;
    const int64_t total = cloud_table_build(segs.data(), m, RENDER_T, nullptr, &nb), np = (int64_t)w * h;
    std::vector<int32_t> blk((size_t)nb + 1, 0);
    cloud_table_build(segs.data(), m, RENDER_T, blk.data(), &nb);
    CloudSeg* d_seg; int32_t *d_blk, *d_info; RenderImgs T;
    CK(hipMalloc((void**)&d_seg, segs.size() * sizeof(CloudSeg))); CK(hipMalloc((void**)&d_blk, blk.size() * 4)); CK(hipMalloc((void**)&d_info, 16));
    CK(hipMalloc((void**)&T.keys, np * 8)); CK(hipMalloc((void**)&T.depth, np * 2)); CK(hipMalloc((void**)&T.bgr, np * 3)); CK(hipMalloc((void**)&T.label, np)); CK(hipMalloc((void**)&T.index, np * 4));
    CK(hipMemcpy(d_seg, segs.data(), segs.size() * sizeof(CloudSeg), hipMemcpyHostToDevice)); CK(hipMemcpy(d_blk, blk.data(), blk.size() * 4, hipMemcpyHostToDevice));
    unsigned long long zero[2] = {0, 0}, cnt[2]; int32_t info[4];
    CK(hipMemcpyToSymbol(HIP_SYMBOL(render_probe_counts), zero, 16));
    CK(k_render(S, d_seg, d_blk, m, total, T, d_info, 0));
    CK(hipDeviceSynchronize());
    CK(hipMemcpyFromSymbol(cnt, HIP_SYMBOL(render_probe_counts), 16)); CK(hipMemcpy(info, d_info, 16, hipMemcpyDeviceToHost));
    printf("{\"points\": %lld, \"visible\": %d, \"covered\": %d, \"offered\": %llu, \"atomics\": %llu}\n", (long long)total, info[1], info[2], cnt[0], cnt[1]);
    for (ssm_point* p : dev) (void)hipFree(p);
    for (void* p : {(void*)d_seg, (void*)d_blk, (void*)d_info, (void*)T.keys, (void*)T.depth, (void*)T.bgr, (void*)T.label, (void*)T.index}) (void)hipFree(p);
    return 0;
}
