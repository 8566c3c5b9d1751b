// test_motion_fuse -- the semantic-motion fusion through Mapper on the device (run by tests/test_gpu_motion_fuse_host.py under -m gpu): motion_semantic_fuse=0 leaves
// the clouds as they were, 1 with an empty moving_mask too, and with a mask the device-map route (deviceCloud + ssm_cloud_fetch) and the host route
// (generatePointCloud) give the same bytes, which are those of ssm_backproject_fused -- without the moving car, with the parked one.
// Prints one "PASS name" / "FAIL name" line per check; exit code = number of failures.
#include "test_mapper_common.h"
static void box(cv::Mat& sem, int x0, int y0, int x1, int y1, int b, int g, int r)
{
    for (int y = y0; y < y1; y++) for (int x = x0; x < x1; x++) { unsigned char* p = sem.ptr<unsigned char>(y) + 3 * x; p[0] = (unsigned char)b; p[1] = (unsigned char)g; p[2] = (unsigned char)r; }
}
// frame 0 of the synthetic stream with a semantic image made here: road, a driving car (under the motion mask), a parked car (not), a pedestrian
static RGBDFrame::Ptr scene(FrameReader& reader, bool with_mask)
{
    reader.reset();
    RGBDFrame::Ptr f = reader.next();
    const int w = f->semantic.cols, h = f->semantic.rows;
    box(f->semantic, 0, 0, w, h, 128, 64, 128);
    box(f->semantic, 100, 200, 220, 300, 128, 0, 64);
    box(f->semantic, 400, 220, 520, 320, 128, 0, 64);
    box(f->semantic, 300, 100, 320, 160, 0, 64, 64);
    if (with_mask) {
        f->moving_mask.create(h, w, CV_8UC1);
        memset(f->moving_mask.data, 0, (size_t)w * h);
        for (int y = 190; y < 260; y++) memset(f->moving_mask.ptr<unsigned char>(y) + 90, 255, 140);
    }
    Eigen::Isometry3d T = Eigen::Isometry3d::Identity();
    T(0, 0) = 0.8; T(0, 1) = -0.6; T(1, 0) = 0.6; T(1, 1) = 0.8; T(0, 3) = 0.25; T(2, 3) = -1.5;
    f->setTransform(T);
    return f;
}

int main(int argc, char** argv)
{
    ParameterReader para(argc > 1 ? argv[1] : "./parameters.txt");
    try {
        FrameReader reader(para, FrameReader::SYNTHETIC);
        VisualOdometryStereo::parameters vo;
        Tracker::Ptr tracker(new Tracker(para, vo));
        PoseGraph pg(para, tracker);
        ParameterReader on = para; on.set("motion_semantic_fuse", "1");
        QuietMapper off_m(para, pg), on_m(on, pg);
        CHECK("switch_defaults_to_off", !off_m.fusesMotion() && on_m.fusesMotion());
        // what the calls that exist give for the scene
        RGBDFrame::Ptr f = scene(reader, true);
        const int w = f->depth.cols, h = f->depth.rows; const double md = para.getData<double>("mapper_max_distance", 40.0);
        ssm::Device& d = on_m.dev_(w, h);
        ssm_camera cam; cam.cx = f->camera.cx; cam.cy = f->camera.cy; cam.fx = f->camera.fx; cam.fy = f->camera.fy; cam.scale = f->camera.scale;
        const Eigen::Isometry3d T = f->getTransform();
        vector<ssm_point> plain((size_t)w * h), fused((size_t)w * h); int n = 0;
        d.check(ssm_backproject(d.ctx(), f->depth.ptr<uint16_t>(), f->rgb.data, f->semantic.data, w, h, &cam, T.data(), md, plain.data(), (int)plain.size(), &n), "ssm_backproject");
        plain.resize((size_t)n);
        ssm_motion_fuse_params P; ssm_motion_fuse_params_default(&P);
        d.check(ssm_backproject_fused(d.ctx(), f->depth.ptr<uint16_t>(), f->rgb.data, f->semantic.data, f->moving_mask.data, w, h, &cam, T.data(), md, &P, fused.data(), (int)fused.size(), &n), "ssm_backproject_fused");
        fused.resize((size_t)n);
        CHECK("scene_has_points_to_lose", plain.size() > 1000 && fused.size() < plain.size());

        CHECK("switch_off_host_route_as_before", same(off_m.viaHost(scene(reader, true)), plain));
        CHECK("switch_off_device_route_as_before", same(off_m.viaDevice(scene(reader, true)), plain));
        CHECK("switch_on_empty_mask_host_route_as_before", same(on_m.viaHost(scene(reader, false)), plain));
        CHECK("switch_on_empty_mask_device_route_as_before", same(on_m.viaDevice(scene(reader, false)), plain));
        const vector<ssm_point> hostc = on_m.viaHost(scene(reader, true)), devc = on_m.viaDevice(scene(reader, true));
        CHECK("switch_on_routes_agree", same(hostc, devc));
        CHECK("switch_on_is_the_fused_backprojection", same(hostc, fused));

        // the mask under the reference's name: the driving car is confirmed, the parked one is not; off: the class mask
        ssm_motion_fuse_info I{};
        const cv::Mat m_on = on_m.semantic_motion_fuse(f, &I), m_off = off_m.semantic_motion_fuse(f);
        vector<uint8_t> cls((size_t)w * h);
        d.check(ssm_moving_mask(d.ctx(), f->semantic.data, w, h, w * 3, cls.data()), "ssm_moving_mask");
        CHECK("fuse_off_is_the_class_mask", memcmp(m_off.data, cls.data(), cls.size()) == 0);
        const unsigned char* mo = m_on.data;
        CHECK("driving_car_confirmed_parked_car_kept", I.blobs == 3 && I.large == 3 && I.confirmed == 1 && I.added == 124 * 104 && mo[(size_t)250 * w + 160] == 255 &&
              mo[(size_t)270 * w + 460] == 0 && mo[(size_t)130 * w + 310] == 255 && cls[(size_t)250 * w + 160] == 0);
        size_t lost = 0;            // pixels the fusion adds to the mask that had a point: a depth inside the range (their classes, Car and Road, are mapped)
        for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) {
            const uint16_t dz = f->depth.ptr<uint16_t>(y)[x];
            if (mo[(size_t)y * w + x] == 255 && cls[(size_t)y * w + x] == 0 && dz != 0 && (double)dz <= md * cam.scale) lost++;
        }
        CHECK("fused_cloud_loses_exactly_the_confirmed_blob", lost > 0 && plain.size() - fused.size() == lost);
    } catch (const exception& e) { cout << "FAIL exception " << e.what() << endl; fails++; }
    cout << (fails ? "FAILED" : "ALL PASSED") << endl;
    return fails;
}
