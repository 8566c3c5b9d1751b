// test_render -- map rendering through Mapper on the device (run by tests/test_gpu_render_host.py under -m gpu) on the scene of host/test_carve.cpp: a KITTI-layout
// stereo sequence (argv[2]) in which a box keeps its place in the image while the camera moves sideways -- every frame leaves a copy of it in the map -- and is GONE
// from frame argv[3] on.  Every frame is taken as a key-frame; argv[4] is a directory for the rendered images.  mapper_render=0 leaves everything as it was; with 1
// the device route (deviceCloud + ssm_render_clouds) and the host route (frame->pointcloud + ssm_render_points) give the same nine counts per view, which are those of
// ssm_render_host + ssm_render_compare_host on the same clouds, view after view; the PNG files read back as the arrays ssm_render_fetch gives; and with
// mapper_carve=1 the views after the box left see strictly fewer map points in front of the measured surface inside the box's rectangle than without: carved points
// are the ones later views see through, which is what `in_front` counts.  Prints one "PASS name" / "FAIL name" line per check; exit code = failures.
#include "test_mapper_common.h"
// the scene of tests/test_gpu_uvd_host.py: the box covers rows 30..95, columns 150..229 in every image that has it
static const int BOX_R0 = 30, BOX_R1 = 96, BOX_C0 = 150, BOX_C1 = 230; static const double BASELINE = 0.532331858;
static string png(const string& dir, size_t j, const char* what) { char b[64]; snprintf(b, sizeof b, "/render_%06d_%s.png", (int)j, what); return dir + b; }

int main(int argc, char** argv)
{
    if (argc < 5) { cerr << "usage: test_render <parameters> <sequence directory> <first frame without the box> <output directory>" << endl; return 2; }
    const size_t U = (size_t)atoi(argv[3]);
    const string out_dir = argv[4];
    ParameterReader para(argv[1]);
    para.set("data_source", argv[2]); para.set("start_index", "0"); para.set("end_index", "100"); para.set("tracker_mode", "stereo");
    para.set("image_width", "400"); para.set("image_height", "120"); para.set("orb_levels", "3"); para.set("orb_features", "300");
    para.set("camera.baseline", "0.532331858"); para.set("camera.roix", "2000"); para.set("camera.roiy", "2000"); para.set("camera.roiz", "4000");
    para.set("uv_disparity", "0"); para.set("motion_semantic_fuse", "0");          // the gates are off: the box reaches the clouds
    VisualOdometryStereo::parameters vp; vp.calib.f = para.getData<double>("camera.fx"); vp.calib.cu = para.getData<double>("camera.cx"); vp.calib.cv = para.getData<double>("camera.cy");
    vp.base = BASELINE; vp.inlier_threshold = 2.0;
    try {
        auto load = [&]() {          // the sequence, tracked: fresh frames each time (the host route keeps a frame's cloud in the frame)
            vector<RGBDFrame::Ptr> kfs;
            Tracker tracker(para, vp); FrameReader rd(para, FrameReader::KITTI);
            while (RGBDFrame::Ptr f = rd.next()) { tracker.updateFrame(f); kfs.push_back(f); }
            return kfs;
        };
        Tracker::Ptr tracker(new Tracker(para, vp));
        PoseGraph pg(para, tracker);
        ParameterReader on = para; on.set("mapper_render", "1"); on.set("mapper_render_point_size", "0.02"); on.set("mapper_render_max_radius", "2");
        ParameterReader on_dir = on; on_dir.set("mapper_render_dir", out_dir + "/plain");
        ParameterReader on_host = on; on_host.set("mapper_device_map", "0");
        ParameterReader carve_dir = on; carve_dir.set("mapper_carve", "1"); carve_dir.set("mapper_render_dir", out_dir + "/carved");
        ParameterReader carve_host = on_host; carve_host.set("mapper_carve", "1");
        QuietMapper off_m(para, pg), dev_m(on_dir, pg), host_m(on_host, pg), cdev_m(carve_dir, pg), chost_m(carve_host, pg);
        CHECK("switch_defaults_to_off", !off_m.rendersViews() && dev_m.rendersViews() && host_m.rendersViews() && off_m.renderedViews() == 0);
        vector<RGBDFrame::Ptr> k0 = load(), kd = load(), kh = load(), kcd = load(), kch = load();
        const size_t n = k0.size();
        CHECK("sequence_has_frames", n >= 6 && kd.size() == n && kh.size() == n && kcd.size() == n && kch.size() == n && U >= 2 && U + 1 < n);
        if (n < 3) { cout << "FAILED" << endl; return fails ? fails : 1; }
        const int w = k0[0]->depth.cols, h = k0[0]->depth.rows; const double md = para.getData<double>("mapper_max_distance", 40.0);
        const ssm_camera cam = Mapper::cameraOf(k0[0]);
        ssm::Device& d = off_m.dev_(w, h);

        // switch off: the clouds are what the calls that exist give, and nothing is recorded
        vector<vector<ssm_point>> plain(n);
        bool off_same = true;
        for (size_t i = 0; i < n; i++) {
            plain[i].resize((size_t)w * h); int m = 0;
            d.check(ssm_backproject(d.ctx(), k0[i]->depth.ptr<uint16_t>(), k0[i]->rgb.data, k0[i]->semantic.data, w, h, &cam, nullptr, md, plain[i].data(), (int)plain[i].size(), &m), "ssm_backproject");
            plain[i].resize((size_t)m);
            off_same = off_same && same(off_m.cloudNow(k0[i]), plain[i]);
        }
        CHECK("switch_off_clouds_as_before", off_same && !off_m.renderInfoOf(k0[0], nullptr));

        // the two routes, without and with carving (carving first, as the viewer does it)
        cdev_m.carveUpTo(kcd); chost_m.carveUpTo(kch);
        dev_m.renderAll(kd); host_m.renderAll(kh); cdev_m.renderAll(kcd); chost_m.renderAll(kch);
        CHECK("every_key_frame_is_a_view_once", dev_m.renderedViews() == (int)n && host_m.renderedViews() == (int)n && cdev_m.renderedViews() == (int)n && chost_m.renderedViews() == (int)n);
        bool clouds_untouched = true;
        for (size_t i = 0; i < n; i++) clouds_untouched = clouds_untouched && same(dev_m.cloudNow(kd[i]), plain[i]) && same(host_m.cloudNow(kh[i]), plain[i]) && same(cdev_m.cloudNow(kcd[i]), chost_m.cloudNow(kch[i]));
        CHECK("rendering_changes_no_cloud", clouds_untouched);

        // the host functions on the same clouds, view after view
        ssm_render_params P; ssm_render_params_default(&P); P.point_size = 0.02; P.max_radius = 2;
        const int window = 5;
        auto host_counts = [&](const vector<RGBDFrame::Ptr>& kfs, const vector<vector<ssm_point>>& clouds, size_t j, vector<uint8_t>* cls_out, vector<uint16_t>* dep_out) {
            vector<const ssm_point*> pts; vector<int32_t> cnt; vector<double> poses;
            for (size_t i = j > (size_t)window ? j - window : 0; i < n && i <= j + window; i++) {
                if (i == j) continue;
                pts.push_back(clouds[i].data()); cnt.push_back((int32_t)clouds[i].size());
                const Eigen::Isometry3d T = kfs[i]->getTransform(); poses.insert(poses.end(), T.data(), T.data() + 16);
            }
            const size_t np = (size_t)w * h;
            vector<uint16_t> dep(np); vector<uint8_t> lab(np), cls(np);
            const Eigen::Isometry3d Tv = kfs[j]->getTransform();
            if (ssm_render_host(w, h, &cam, Tv.data(), pts.data(), cnt.data(), poses.data(), (int)pts.size(), &P, dep.data(), nullptr, lab.data(), nullptr, nullptr, nullptr) != SSM_OK) throw runtime_error("ssm_render_host failed");
            ssm_render_compare_info I{};
            if (ssm_render_compare_host(dep.data(), lab.data(), w, h, kfs[j]->depth.ptr<uint16_t>(), kfs[j]->semantic.data, cam.scale, &P, &I, cls.data()) != SSM_OK) throw runtime_error("ssm_render_compare_host failed");
            if (cls_out) cls_out->swap(cls);
            if (dep_out) dep_out->swap(dep);
            return I;
        };
        vector<vector<ssm_point>> carved(n);
        for (size_t i = 0; i < n; i++) carved[i] = chost_m.cloudNow(kch[i]);
        bool routes = true, composed = true, counted = true;
        long long front[2] = {0, 0}, front_box[2] = {0, 0}, agree[2] = {0, 0};
        for (size_t j = 0; j < n; j++) {
            ssm_render_compare_info a{}, b{}, ca{}, cb{};
            const bool have = dev_m.renderInfoOf(kd[j], &a) && host_m.renderInfoOf(kh[j], &b) && cdev_m.renderInfoOf(kcd[j], &ca) && chost_m.renderInfoOf(kch[j], &cb);
            routes = routes && have && memcmp(&a, &b, sizeof a) == 0 && memcmp(&ca, &cb, sizeof ca) == 0;
            vector<uint8_t> cls[2];
            const ssm_render_compare_info want = host_counts(k0, plain, j, &cls[0], nullptr), cwant = host_counts(k0, carved, j, &cls[1], nullptr);
            composed = composed && memcmp(&a, &want, sizeof a) == 0 && memcmp(&ca, &cwant, sizeof ca) == 0;
            counted = counted && a.n_pixels == (int64_t)w * h && a.unrendered + a.no_depth + a.in_front + a.behind + a.agree == a.n_pixels && a.label_agree + a.label_disagree + a.label_unknown == a.agree;
            cout << "view " << j << ": agree " << a.agree << " / " << ca.agree << ", in front " << a.in_front << " / " << ca.in_front << ", behind " << a.behind << " / " << ca.behind
                 << ", unrendered " << a.unrendered << " / " << ca.unrendered << " (without / with carving)" << endl;
            // the class images the device route wrote, inside the box's rectangle, in the views after the box left
            for (int c = 0; c < 2; c++) {
                const cv::Mat m = ssm::imreadPNG(png(out_dir + (c ? "/carved" : "/plain"), j, "class"), -1);
                bool ok = !m.empty() && m.rows == h && m.cols == w && m.type() == CV_8UC1;
                for (int y = 0; ok && y < h; y++) ok = memcmp(m.ptr<uint8_t>(y), &cls[c][(size_t)y * w], (size_t)w) == 0;
                composed = composed && ok;
                if (!ok || j < U) continue;
                front[c] += c ? ca.in_front : a.in_front; agree[c] += c ? ca.agree : a.agree;
                for (int y = BOX_R0; y < BOX_R1; y++) for (int x = BOX_C0; x < BOX_C1; x++) front_box[c] += m.ptr<uint8_t>(y)[x] == 2;
            }
        }
        CHECK("routes_give_the_same_counts", routes);
        CHECK("counts_are_the_host_functions_view_after_view", composed);
        CHECK("counts_add_up", counted);
        cout << "views " << U << ".." << n - 1 << ", in front inside the box's rectangle: " << front_box[0] << " without carving, " << front_box[1] << " with; in front in all: " << front[0] << " / " << front[1]
             << "; agree: " << agree[0] << " / " << agree[1] << endl;
        CHECK("the_box_left_a_trail_in_front_of_later_views", front_box[0] > 0);
        CHECK("carving_leaves_strictly_fewer_points_in_front_inside_the_box", front_box[1] < front_box[0]);

        // the files: what ssm_render_fetch gives for the view, the label image through the palette
        bool files = true;
        for (size_t j = 0; j < n; j += 3) for (int c = 0; c < 2; c++) {
            cv::Mat dep, bgr, lab, col;
            (c ? cdev_m : dev_m).fetchView(c ? kcd : kd, j, dep, bgr, lab);
            col.create(h, w, CV_8UC3); ssm_render_label_colours(lab.data, (int64_t)w * h, col.data);
            const string dir = out_dir + (c ? "/carved" : "/plain");
            files = files && same_mat(ssm::imreadPNG(png(dir, j, "depth"), -1), dep) && same_mat(ssm::imreadPNG(png(dir, j, "bgr"), -1), bgr) && same_mat(ssm::imreadPNG(png(dir, j, "label"), -1), col);
            vector<uint16_t> hd;
            host_counts(k0, c ? carved : plain, j, nullptr, &hd);
            files = files && memcmp(hd.data(), dep.ptr<uint16_t>(), hd.size() * 2) == 0;
        }
        CHECK("the_written_images_read_back_as_fetched", files);

        // a Mapper whose viewer runs: the rendering happens when the thread ends, whatever updates it made; the published map is as without the switch
        {
            Mapper::PointCloud::Ptr maps[2]; bool views = true, equal = true;
            for (int c = 0; c < 2; c++) {
                PoseGraph g(para, tracker);
                g.keyframes = load();
                Mapper m(c ? on : para, g);
                for (int t = 0; t < 20000 && m.updates() < 1 && !m.viewerFailed; t++) this_thread::sleep_for(chrono::milliseconds(1));
                maps[c] = m.getGlobalMap();
                m.shutdown();
                if (m.viewerFailed || m.deviceMapFellBack) throw runtime_error("the viewer failed");
                views = views && m.renderedViews() == (c ? (int)n : 0);
                for (size_t j = 0; c && j < n; j++) { ssm_render_compare_info a{}, b{}; equal = equal && m.renderInfoOf(g.keyframes[j], &a) && dev_m.renderInfoOf(kd[j], &b) && memcmp(&a, &b, sizeof a) == 0; }
            }
            bool same_map = maps[0] && maps[1] && maps[0]->points.size() == maps[1]->points.size() && maps[0]->points.size() > 1000;
            if (same_map) {
                static_assert(sizeof(Mapper::PointT) == sizeof(ssm_point), "a map point is an ssm_point");
                vector<ssm_point> a(maps[0]->points.size()), b(a.size());
                memcpy((void*)a.data(), (const void*)maps[0]->points.data(), a.size() * sizeof(ssm_point)); memcpy((void*)b.data(), (const void*)maps[1]->points.data(), b.size() * sizeof(ssm_point));
                same_map = same(a, b);
            }
            CHECK("the_viewer_renders_as_it_ends", views && equal);
            CHECK("the_published_map_is_as_without_the_switch", same_map);
        }
    } catch (const exception& e) { cout << "FAIL exception " << e.what() << endl; fails++; }
    cout << (fails ? "FAILED" : "ALL PASSED") << endl;
    return fails;
}
