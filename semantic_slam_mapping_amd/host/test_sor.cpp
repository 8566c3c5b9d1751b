// test_sor -- the statistical outlier removal through Mapper on the device (run by tests/test_gpu_sor_host.py under -m gpu): mapper_outlier_removal=0 leaves the
// clouds as they were; with 1 the device-map route (deviceCloud + ssm_cloud_fetch) and the host route (generatePointCloud) give the same bytes, which are those of
// ssm_sor_filter on the unfiltered camera-frame cloud, transformed afterwards -- with and without motion_semantic_fuse -- and the depth speckles planted in the
// scene are gone.  Prints one "PASS name" / "FAIL name" line per check; exit code = number of failures.
#include "test_mapper_common.h"
static void box(cv::Mat& img, int x0, int y0, int x1, int y1, int b, int g, int r)
{
    for (int y = y0; y < y1; y++) for (int x = x0; x < x1; x++) { unsigned char* p = img.ptr<unsigned char>(y) + 3 * x; p[0] = (unsigned char)b; p[1] = (unsigned char)g; p[2] = (unsigned char)r; }
}
static const int SPECKLES = 200;
static const float SPECKLE_Z = 1.0f;          // world z of everything but the speckles is below this (the scene ends 1.6 m from the camera, the pose lowers z by 1.5)
// frame 0 of the synthetic stream with a road, a driving car under the motion mask and a pedestrian, and SPECKLES pixels whose depth lies 3 to 4 m out, far behind the scene
static RGBDFrame::Ptr scene(FrameReader& reader)
{
    reader.reset();
    RGBDFrame::Ptr f = reader.next();
    const int w = f->semantic.cols, h = f->semantic.rows;
    box(f->semantic, 0, 0, w, h, 128, 64, 128);
    box(f->semantic, 100, 200, 220, 300, 128, 0, 64);
    box(f->semantic, 300, 100, 320, 160, 0, 64, 64);
    f->moving_mask.create(h, w, CV_8UC1);
    memset(f->moving_mask.data, 0, (size_t)w * h);
    for (int y = 190; y < 260; y++) memset(f->moving_mask.ptr<unsigned char>(y) + 90, 255, 140);
    uint64_t s = 2024;
    for (int i = 0; i < SPECKLES; i++) {
        s = s * 6364136223846793005ull + 1442695040888963407ull; const int x = (int)((s >> 33) % (uint64_t)w);
        s = s * 6364136223846793005ull + 1442695040888963407ull; const int y = (int)((s >> 33) % (uint64_t)h);
        s = s * 6364136223846793005ull + 1442695040888963407ull; f->depth.ptr<uint16_t>(y)[x] = (uint16_t)(3000 + (s >> 33) % 1000);
    }
    Eigen::Isometry3d T = Eigen::Isometry3d::Identity();
    T(0, 0) = 0.8; T(0, 1) = -0.6; T(1, 0) = 0.6; T(1, 1) = 0.8; T(0, 3) = 0.25; T(2, 3) = -1.5;
    f->setTransform(T);
    return f;
}
static size_t speckles_in(const vector<ssm_point>& c) { size_t n = 0; for (const ssm_point& p : c) n += p.z > SPECKLE_Z; return n; }
// the filter on a camera-frame cloud, then the pose: pcl::transformPointCloud's arithmetic as Mapper::generatePointCloud applies it
static vector<ssm_point> filtered_then_posed(ssm::Device& d, vector<ssm_point> cam, const Eigen::Isometry3d& T, const ssm_sor_params& P, ssm_sor_info* I)
{
    vector<ssm_point> out(max(cam.size(), (size_t)1)); int n = 0;
    d.check(ssm_sor_filter(d.ctx(), cam.data(), (int)cam.size(), &P, out.data(), (int)out.size(), &n, I), "ssm_sor_filter");
    out.resize((size_t)n);
    const double* t = T.data();
    for (ssm_point& p : out) {
        const double x = p.x, y = p.y, z = p.z;
        p.x = (float)(t[0] * x + t[4] * y + t[8] * z + t[12]); p.y = (float)(t[1] * x + t[5] * y + t[9] * z + t[13]); p.z = (float)(t[2] * x + t[6] * y + t[10] * z + t[14]);
    }
    return out;
}

int main(int argc, char** argv)
{
    ParameterReader para(argc > 1 ? argv[1] : "./parameters.txt");
    try {
        FrameReader reader(para, FrameReader::SYNTHETIC);
        VisualOdometryStereo::parameters vo;
        Tracker::Ptr tracker(new Tracker(para, vo));
        PoseGraph pg(para, tracker);
        ParameterReader on = para; on.set("mapper_outlier_removal", "1");
        ParameterReader on_fused = on; on_fused.set("motion_semantic_fuse", "1");
        ParameterReader k8 = on; k8.set("mapper_sor_mean_k", "8"); k8.set("mapper_sor_stddev", "2.5");
        QuietMapper off_m(para, pg), on_m(on, pg), fused_m(on_fused, pg), k8_m(k8, pg);
        CHECK("switch_defaults_to_off", !off_m.removesOutliers() && on_m.removesOutliers() && fused_m.removesOutliers() && fused_m.fusesMotion() && !on_m.fusesMotion());

        // what the calls that exist give for the scene: the unfiltered clouds, in the camera frame and posed
        RGBDFrame::Ptr f = scene(reader);
        const int w = f->depth.cols, h = f->depth.rows; const double md = para.getData<double>("mapper_max_distance", 40.0);
        ssm::Device& d = on_m.dev_(w, h);
        ssm_camera cam; cam.cx = f->camera.cx; cam.cy = f->camera.cy; cam.fx = f->camera.fx; cam.fy = f->camera.fy; cam.scale = f->camera.scale;
        const Eigen::Isometry3d T = f->getTransform();
        vector<ssm_point> plain((size_t)w * h), plain_cam((size_t)w * h), fused_cam((size_t)w * h); int n = 0;
        d.check(ssm_backproject(d.ctx(), f->depth.ptr<uint16_t>(), f->rgb.data, f->semantic.data, w, h, &cam, T.data(), md, plain.data(), (int)plain.size(), &n), "ssm_backproject");
        plain.resize((size_t)n);
        d.check(ssm_backproject(d.ctx(), f->depth.ptr<uint16_t>(), f->rgb.data, f->semantic.data, w, h, &cam, nullptr, md, plain_cam.data(), (int)plain_cam.size(), &n), "ssm_backproject");
        plain_cam.resize((size_t)n);
        ssm_motion_fuse_params FP; ssm_motion_fuse_params_default(&FP);
        d.check(ssm_backproject_fused(d.ctx(), f->depth.ptr<uint16_t>(), f->rgb.data, f->semantic.data, f->moving_mask.data, w, h, &cam, nullptr, md, &FP, fused_cam.data(), (int)fused_cam.size(), &n), "ssm_backproject_fused");
        fused_cam.resize((size_t)n);
        CHECK("scene_has_speckles", plain.size() > 1000 && speckles_in(plain) > (size_t)SPECKLES / 2 && fused_cam.size() < plain_cam.size());

        CHECK("switch_off_host_route_as_before", same(off_m.viaHost(scene(reader)), plain));
        CHECK("switch_off_device_route_as_before", same(off_m.viaDevice(scene(reader)), plain));
        ssm_sor_info I{}, If{}, I8{};
        ssm_sor_params P; ssm_sor_params_default(&P);
        const vector<ssm_point> want = filtered_then_posed(d, plain_cam, T, P, &I), want_fused = filtered_then_posed(d, fused_cam, T, P, &If);
        RGBDFrame::Ptr fh = scene(reader);
        const vector<ssm_point> hostc = on_m.viaHost(fh), devc = on_m.viaDevice(scene(reader));
        CHECK("switch_on_routes_agree", same(hostc, devc));
        CHECK("switch_on_is_the_filter_on_the_unfiltered_cloud", same(hostc, want) && want.size() < plain.size() && want.size() > plain.size() / 2);
        ssm_sor_info Ih{};
        CHECK("switch_on_records_the_filter_figures", on_m.sorInfoOf(fh, &Ih) && memcmp(&Ih, &I, sizeof I) == 0 && Ih.n_in == (int)plain.size() && Ih.n_kept == (int)want.size() && !off_m.sorInfoOf(fh, nullptr));
        CHECK("filtered_once_per_key_frame", same(on_m.viaHost(fh), want) && on_m.cloudsComputed == 2);          // the second call transforms the cached, filtered cloud
        const vector<ssm_point> hostf = fused_m.viaHost(scene(reader)), devf = fused_m.viaDevice(scene(reader));
        CHECK("switch_on_with_fusion_routes_agree", same(hostf, devf));
        CHECK("switch_on_with_fusion_is_the_filter_on_the_fused_cloud", same(hostf, want_fused) && want_fused.size() < want.size());
        P.mean_k = 8; P.stddev_mul = 2.5;
        const vector<ssm_point> want8 = filtered_then_posed(d, plain_cam, T, P, &I8);
        RGBDFrame::Ptr f8 = scene(reader);
        const vector<ssm_point> host8 = k8_m.viaHost(f8), dev8 = k8_m.viaDevice(scene(reader));
        ssm_sor_info J{}; k8_m.sorInfoOf(f8, &J);
        CHECK("mean_k_and_stddev_come_from_the_parameters", same(host8, want8) && same(dev8, want8) && memcmp(&J, &I8, sizeof J) == 0 && I8.threshold != I.threshold);
        CHECK("speckles_leave_the_map", speckles_in(want) == 0 && speckles_in(want_fused) == 0 && speckles_in(hostc) == 0 && speckles_in(devf) == 0);
    } catch (const exception& e) { cout << "FAIL exception " << e.what() << endl; fails++; }
    cout << (fails ? "FAILED" : "ALL PASSED") << endl;
    return fails;
}
