// test_align -- dense alignment through Mapper on the device (run by tests/test_gpu_align_host.py under -m gpu).  The scene is made here, analytically, in KITTI's
// layout: a camera 1.6 m above a ground plane drives forward half a metre per key-frame past a box that stands beside the lane; every depth image is ray-cast from
// the TRUE pose (depth units of 1 mm), and every key-frame is handed to the Mapper with a pose that carries a planted, cumulative error of 3 cm of height, 4 mrad of
// pitch and 3 mrad of roll per key-frame -- the directions the ground plane constrains (tests/test_align.py shows on the CPU that a ground plane leaves sliding
// along the road, sideways and yaw without any constraint; the box adds a weak one; NO error is planted there and those directions are not judged).
// mapper_align=0 leaves everything as it was; with 1 the device route (deviceCloud + ssm_align_clouds) and the host route (frame->pointcloud + ssm_align_points) give
// the same info, correction and map pose per key-frame, which are those of ssm_align_host replayed here view after view; every accepted key-frame's map pose is
// closer to the truth than the planted pose in height, pitch and roll; over all views the rendering yardstick (ssm_render_compare through mapper_render=1) agrees
// on strictly more pixels and has strictly fewer in front of or behind the measured surface than without the switch; mapper_carve=1 on top runs and both routes
// agree; and a Mapper whose viewer thread runs aligns every key-frame exactly once.  Prints one "PASS name" / "FAIL name" line per check; exit code = failures.
#include "test_lane_scene.h"

static const double PLANT_TY = 0.03, PLANT_RX = 0.004, PLANT_RZ = 0.003;          // per key-frame, cumulative
// Rz(rz) Rx(rx) and a translation
static Eigen::Isometry3d se3(double rx, double rz, double tx, double ty, double tz)
{
    const double cx = cos(rx), sx = sin(rx), cz = cos(rz), sz = sin(rz);
    const double Rx[3][3] = {{1, 0, 0}, {0, cx, -sx}, {0, sx, cx}}, Rz[3][3] = {{cz, -sz, 0}, {sz, cz, 0}, {0, 0, 1}};
    Eigen::Isometry3d T;
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) { double s = 0; for (int k = 0; k < 3; k++) s += Rz[r][k] * Rx[k][c]; T(r, c) = s; }
    T(0, 3) = tx; T(1, 3) = ty; T(2, 3) = tz;
    return T;
}

int main(int argc, char** argv)
{
    if (argc < 2) { cerr << "usage: test_align <parameters>" << endl; return 2; }
    ParameterReader para(argv[1]);
    para.set("image_width", "400"); para.set("image_height", "120"); para.set("orb_levels", "3"); para.set("orb_features", "300");
    para.set("camera.cx", "200.0"); para.set("camera.cy", "40.0"); para.set("camera.fx", "300.0"); para.set("camera.fy", "300.0"); para.set("camera.scale", "1000.0");
    para.set("uv_disparity", "0"); para.set("motion_semantic_fuse", "0");
    VisualOdometryStereo::parameters vp; vp.calib.f = 300.0; vp.calib.cu = 200.0; vp.calib.cv = 40.0; vp.base = 0.5;
    try {
        const CAMERA_INTRINSIC_PARAMETERS camera = para.getCamera();
        vector<Eigen::Isometry3d> truth, planted;
        for (int j = 0; j < N; j++) { truth.push_back(se3(0, 0, 0, 0, STEP * j)); planted.push_back(truth[j] * se3(PLANT_RX * j, PLANT_RZ * j, 0, PLANT_TY * j, 0)); }
        auto load = [&]() {          // the sequence: fresh frames each time (the host route keeps a frame's cloud in the frame)
            vector<RGBDFrame::Ptr> kfs;
            for (int j = 0; j < N; j++) {
                RGBDFrame::Ptr f(new RGBDFrame);
                f->id = j; f->camera = camera;
                cast(STEP * j, camera, f->depth);
                f->rgb.create(H, W, CV_8UC3); f->semantic.create(H, W, CV_8UC3);
                for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) {
                    uint8_t* c = f->rgb.ptr<uint8_t>(y) + 3 * x; c[0] = (uint8_t)(x + j); c[1] = (uint8_t)(y * 2); c[2] = (uint8_t)(x ^ y);
                    uint8_t* s = f->semantic.ptr<uint8_t>(y) + 3 * x; s[0] = 128; s[1] = 64; s[2] = 128;          // class 4 of the palette: nothing that moves
                }
                f->setTransform(planted[j]);
                kfs.push_back(f);
            }
            return kfs;
        };
        Tracker::Ptr tracker(new Tracker(para, vp));
        PoseGraph pg(para, tracker);
        ParameterReader rend = para; rend.set("mapper_render", "1"); rend.set("mapper_render_point_size", "0.02"); rend.set("mapper_render_max_radius", "2");
        ParameterReader on = rend; on.set("mapper_align", "1");
        ParameterReader on_host = on; on_host.set("mapper_device_map", "0");
        ParameterReader carve_on = on; carve_on.set("mapper_carve", "1");
        ParameterReader carve_host = on_host; carve_host.set("mapper_carve", "1");
        QuietMapper off_m(rend, pg), dev_m(on, pg), host_m(on_host, pg), cdev_m(carve_on, pg), chost_m(carve_host, pg);
        CHECK("switch_defaults_to_off", !off_m.aligns() && dev_m.aligns() && host_m.aligns() && off_m.alignedKeyframes() == 0);
        vector<RGBDFrame::Ptr> k0 = load(), kd = load(), kh = load(), kcd = load(), kch = load();
        const size_t n = k0.size();
        const double md = para.getData<double>("mapper_max_distance", 40.0);
        ssm_camera cam; cam.cx = camera.cx; cam.cy = camera.cy; cam.fx = camera.fx; cam.fy = camera.fy; cam.scale = camera.scale;
        ssm::Device& d = off_m.dev_(W, H);

        // switch off: the clouds are what the calls that exist give, the poses are the key-frames' own, nothing is recorded
        vector<vector<ssm_point>> plain(n);
        bool off_same = true;
        for (size_t i = 0; i < n; i++) {
            plain[i].resize((size_t)W * H); int m = 0;
            d.check(ssm_backproject(d.ctx(), k0[i]->depth.ptr<uint16_t>(), k0[i]->rgb.data, k0[i]->semantic.data, W, H, &cam, nullptr, md, plain[i].data(), (int)plain[i].size(), &m), "ssm_backproject");
            plain[i].resize((size_t)m);
            off_same = off_same && same(off_m.cloudNow(k0[i]), plain[i]) && same_pose(off_m.mapPoseOf(k0[i]), k0[i]->getTransform()) && plain[i].size() > 10000;
        }
        off_m.alignUpTo(k0);          // (what the viewer never does with the switch off; mapPoseOf must still ignore it)
        CHECK("switch_off_clouds_and_poses_as_before", off_same && same_pose(off_m.mapPoseOf(k0[3]), k0[3]->getTransform()));

        // the two routes
        dev_m.alignUpTo(kd); host_m.alignUpTo(kh);
        const int acc0 = dev_m.acceptedAlignments();
        dev_m.alignUpTo(kd);
        CHECK("every_key_frame_is_aligned_exactly_once", dev_m.alignedKeyframes() == (int)n && host_m.alignedKeyframes() == (int)n && dev_m.acceptedAlignments() == acc0);
        bool routes = true, untouched = true, tfw = true;
        for (size_t j = 0; j < n; j++) {
            ssm_align_info a{}, b{}; Eigen::Isometry3d Da, Db; bool aa = false, ab = false;
            routes = routes && dev_m.alignInfoOf(kd[j], &a, &Da, &aa) && host_m.alignInfoOf(kh[j], &b, &Db, &ab) && memcmp(&a, &b, sizeof a) == 0 && same_pose(Da, Db) && aa == ab &&
                     same_pose(dev_m.mapPoseOf(kd[j]), host_m.mapPoseOf(kh[j]));
            untouched = untouched && same(dev_m.cloudNow(kd[j]), plain[j]) && same(host_m.cloudNow(kh[j]), plain[j]);
            tfw = tfw && same_pose(kd[j]->getTransform(), planted[j]) && same_pose(kh[j]->getTransform(), planted[j]);
        }
        CHECK("routes_give_the_same_info_correction_and_map_pose", routes);
        CHECK("alignment_changes_no_cloud", untouched);
        CHECK("the_key_frames_own_poses_are_not_written", tfw);

        // ssm_align_host replayed view after view: D_prev . P_j as the start, the clouds of the window at their map poses
        ssm_align_params P; ssm_align_params_default(&P);
        bool composed = true, closer = true; int accepted = 0;
        Eigen::Isometry3d D; vector<Eigen::Isometry3d> map_pose;
        for (size_t j = 0; j < n; j++) {
            const Eigen::Isometry3d start = D * planted[j];
            Eigen::Isometry3d mp = start; ssm_align_info I; memset(&I, 0, sizeof I); bool acc = false;
            if (j > 0) {
                vector<const ssm_point*> pts; vector<int32_t> cnt; vector<double> poses;
                for (size_t i = j > 5 ? j - 5 : 0; i < j; i++) { pts.push_back(plain[i].data()); cnt.push_back((int32_t)plain[i].size()); poses.insert(poses.end(), map_pose[i].data(), map_pose[i].data() + 16); }
                double To[16];
                if (ssm_align_host(k0[j]->depth.ptr<uint16_t>(), W, H, &cam, start.data(), pts.data(), cnt.data(), poses.data(), (int)pts.size(), &P, To, &I, nullptr, nullptr, nullptr, 0, nullptr) != SSM_OK)
                    throw runtime_error("ssm_align_host failed");
                acc = I.status == SSM_ALIGN_CONVERGED || (I.status == SSM_ALIGN_MAX_ITER && I.inliers_last >= P.min_inliers);
                if (acc) { for (int c = 0; c < 4; c++) for (int r = 0; r < 4; r++) mp(r, c) = To[c * 4 + r]; D = mp * planted[j].inverse(); }
            }
            map_pose.push_back(mp);
            ssm_align_info a{}; Eigen::Isometry3d Da; bool aa = false;
            composed = composed && dev_m.alignInfoOf(kd[j], &a, &Da, &aa) && memcmp(&a, &I, sizeof a) == 0 && aa == acc && same_pose(Da, D) && same_pose(dev_m.mapPoseOf(kd[j]), mp);
            const Eigen::Isometry3d ep = truth[j].inverse() * planted[j], em = truth[j].inverse() * mp;
            cout << "key-frame " << j << ": status " << I.status << " iterations " << I.iterations << " inliers " << I.inliers_first << " -> " << I.inliers_last << (acc ? " accepted" : " not accepted")
                 << "; height / pitch / roll error planted " << ep(1, 3) << " " << ep(2, 1) << " " << ep(1, 0) << ", map pose " << em(1, 3) << " " << em(2, 1) << " " << em(1, 0) << endl;
            if (acc) { accepted++; closer = closer && fabs(em(1, 3)) < fabs(ep(1, 3)) && fabs(em(2, 1)) < fabs(ep(2, 1)) && fabs(em(1, 0)) < fabs(ep(1, 0)); }
        }
        CHECK("alignment_is_the_host_function_view_after_view", composed);
        CHECK("every_later_key_frame_is_accepted", accepted == (int)n - 1 && dev_m.acceptedAlignments() == accepted);
        CHECK("accepted_map_poses_are_closer_to_the_truth_in_height_pitch_and_roll", closer);

        // the yardstick of s.17 over all views, without and with the switch
        off_m.renderAll(k0); dev_m.renderAll(kd); host_m.renderAll(kh);
        long long agree[2] = {0, 0}, off_surface[2] = {0, 0}; bool render_routes = true;
        for (size_t j = 0; j < n; j++) {
            ssm_render_compare_info a{}, b{}, c{};
            if (!(off_m.renderInfoOf(k0[j], &a) && dev_m.renderInfoOf(kd[j], &b) && host_m.renderInfoOf(kh[j], &c))) throw runtime_error("a view was not rendered");
            agree[0] += a.agree; agree[1] += b.agree; off_surface[0] += a.in_front + a.behind; off_surface[1] += b.in_front + b.behind;
            render_routes = render_routes && memcmp(&b, &c, sizeof b) == 0;
        }
        cout << "all views: agree " << agree[0] << " without / " << agree[1] << " with mapper_align=1; in front + behind " << off_surface[0] << " / " << off_surface[1] << endl;
        CHECK("the_yardstick_agrees_on_strictly_more_pixels", agree[1] > agree[0]);
        CHECK("the_yardstick_has_strictly_fewer_pixels_off_the_surface", off_surface[1] < off_surface[0]);
        CHECK("rendering_uses_the_map_poses_on_both_routes", render_routes);

        // with carving on top, key-frame by key-frame as the viewer does it (j aligned, then j a carving view); both routes agree
        cdev_m.alignCarveUpTo(kcd); chost_m.alignCarveUpTo(kch);
        bool carve_routes = cdev_m.carvedViews() == (int)n - 1 && chost_m.carvedViews() == (int)n - 1; long long removed = 0;
        for (size_t j = 0; j < n; j++) {
            ssm_carve_info a{}, b{}; ssm_align_info x{}, y{};
            const bool ha = cdev_m.carveInfoOf(kcd[j], &a), hb = chost_m.carveInfoOf(kch[j], &b);
            carve_routes = carve_routes && ha == hb && memcmp(&a, &b, sizeof a) == 0 && same(cdev_m.cloudNow(kcd[j]), chost_m.cloudNow(kch[j])) &&
                           cdev_m.alignInfoOf(kcd[j], &x) && chost_m.alignInfoOf(kch[j], &y) && memcmp(&x, &y, sizeof x) == 0 && same_pose(cdev_m.mapPoseOf(kcd[j]), chost_m.mapPoseOf(kch[j]));
            removed += a.removed;
        }
        cout << "with mapper_carve=1: " << removed << " points removed over all clouds" << endl;
        CHECK("with_carving_both_routes_agree", carve_routes);

        // a Mapper whose viewer runs: every key-frame is aligned exactly once, before the thread ends, whatever updates it made
        {
            PoseGraph g(para, tracker);
            g.keyframes = load();
            Mapper m(on, g);
            for (int t = 0; t < 20000 && m.updates() < 1 && !m.viewerFailed; t++) this_thread::sleep_for(chrono::milliseconds(1));
            Mapper::PointCloud::Ptr map = m.getGlobalMap();
            m.shutdown();
            if (m.viewerFailed || m.deviceMapFellBack) throw runtime_error("the viewer failed");
            bool equal = m.alignedKeyframes() == (int)n && m.acceptedAlignments() == accepted;
            for (size_t j = 0; j < n; j++) { ssm_align_info a{}, b{}; equal = equal && m.alignInfoOf(g.keyframes[j], &a) && dev_m.alignInfoOf(kd[j], &b) && memcmp(&a, &b, sizeof a) == 0 && same_pose(m.mapPoseOf(g.keyframes[j]), dev_m.mapPoseOf(kd[j])); }
            CHECK("the_viewer_aligns_every_key_frame_once", equal && map && map->points.size() > 1000);
        }
    } catch (const exception& e) { cout << "FAIL exception " << e.what() << endl; fails++; }
    cout << (fails ? "FAILED" : "ALL PASSED") << endl;
    return fails;
}
