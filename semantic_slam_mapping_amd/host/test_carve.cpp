// test_carve -- free-space carving through Mapper on the device (run by tests/test_gpu_carve_host.py under -m gpu) on a KITTI-layout stereo sequence (argv[2]): the
// scene of tests/test_gpu_uvd_host.py (k = 0.05: the static scene slides by 2 pixels per frame at the box's disparity), in which the box keeps its place in the image
// while the camera moves sideways -- every frame leaves a copy of it in the map -- and is GONE from frame argv[3] on: "a car that stood for some key-frames and drove
// away".  Every frame is taken as a key-frame.  mapper_carve=0 leaves the clouds as they were; with 1 the device route (deviceCloud + ssm_carve) and the host route
// (frame->pointcloud + ssm_carve_points) give the same bytes and figures, which are those of ssm_carve_host applied view after view to the uncarved clouds.  The box's
// points are decided per point from the scene's rectangle, its disparity and the shift of 2 (j - i) pixels: every point that two later views show in front of valid,
// farther ground is gone, whole copies with them; with a window of 1 no view can vote twice and every point deep inside the box stays.  A Mapper whose viewer runs
// through a rebuild publishes a map without a voxel in the trail.  Prints one "PASS name" / "FAIL name" line per check; exit code = failures.
#include "test_mapper_common.h"
#include <set>
#include <array>
// the scene of tests/test_gpu_uvd_host.py: the box covers rows 30..95, columns 150..229 at disparity 40 in every image
static const int BOX_R0 = 30, BOX_R1 = 96, BOX_C0 = 150, BOX_C1 = 230; static const double BOX_DISP = 40.0, BASELINE = 0.532331858;
static bool in_box(const ssm_point& p, const ssm_camera& c)
{
    const double u = c.fx * p.x / p.z + c.cx, v = c.fy * p.y / p.z + c.cy, zb = c.fx * BASELINE / BOX_DISP;
    return v >= BOX_R0 + 2 && v < BOX_R1 - 2 && u >= BOX_C0 + 2 && u < BOX_C1 - 2 && fabs(p.z - zb) < 0.03 * zb;          // (one disparity step is 2.5 % there)
}
static const int SHIFT = 2, ROW0 = 32, ROW1 = 86;          // pixels per frame at the box's disparity (k x 40); the rows where the ground behind the box is at disparity <= 35: 14 % farther
static int px_u(const ssm_point& p, const ssm_camera& c) { return (int)lrint(c.fx * p.x / p.z + c.cx); }
static int px_v(const ssm_point& p, const ssm_camera& c) { return (int)lrint(c.fy * p.y / p.z + c.cy); }
// does view `v` show valid depth, farther than the box by 10 %, in the 5 x 5 pixels around (u, y)?  (the window of the verdict is 3 x 3: one pixel of slack for the pose)
static bool far_ground(const RGBDFrame::Ptr& v, int u, int y, const ssm_camera& c)
{
    const double zb = c.fx * BASELINE / BOX_DISP * c.scale;
    if (u < 2 || y < 2 || u + 2 >= v->depth.cols || y + 2 >= v->depth.rows) return false;
    for (int dy = -2; dy <= 2; dy++) for (int dx = -2; dx <= 2; dx++) if (!(v->depth.ptr<uint16_t>(y + dy)[u + dx] > 1.1 * zb)) return false;
    return true;
}
// the voxels of a published map that lie in the trail: at the box's depth, in the rows where nothing else is at that depth, between the first and the last copy
static size_t trail_voxels(const Mapper::PointCloud::Ptr& m, const ssm_camera& c, double x_first, double x_last)
{
    if (!m) return 0;
    const double zb = c.fx * BASELINE / BOX_DISP, y0 = (ROW0 + 2 - c.cy) * zb / c.fy, y1 = (ROW1 - 3 - c.cy) * zb / c.fy;
    const double x0 = (BOX_C0 + 2 - c.cx) * zb / c.fx + x_first, x1 = (BOX_C1 - 3 - c.cx) * zb / c.fx + x_last;
    size_t n = 0;
    for (const Mapper::PointT& p : m->points) n += fabs(p.z - zb) < 0.25 && p.y >= y0 && p.y <= y1 && p.x >= x0 && p.x <= x1;
    return n;
}
static size_t box_points(const vector<ssm_point>& c, const ssm_camera& cam) { size_t n = 0; for (const ssm_point& p : c) n += in_box(p, cam); return n; }

int main(int argc, char** argv)
{
    if (argc < 4) { cerr << "usage: test_carve <parameters> <sequence directory> <first frame without the box>" << endl; return 2; }
    const size_t U = (size_t)atoi(argv[3]);
    ParameterReader para(argv[1]);
    para.set("data_source", argv[2]); para.set("start_index", "0"); para.set("end_index", "100"); para.set("tracker_mode", "stereo");
    para.set("image_width", "400"); para.set("image_height", "120"); para.set("orb_levels", "3"); para.set("orb_features", "300");
    para.set("camera.baseline", "0.532331858"); para.set("camera.roix", "2000"); para.set("camera.roiy", "2000"); para.set("camera.roiz", "4000");
    para.set("uv_disparity", "0"); para.set("motion_semantic_fuse", "0");          // the gates are off: the box reaches the clouds
    VisualOdometryStereo::parameters vp; vp.calib.f = para.getData<double>("camera.fx"); vp.calib.cu = para.getData<double>("camera.cx"); vp.calib.cv = para.getData<double>("camera.cy");
    vp.base = BASELINE; vp.inlier_threshold = 2.0;
    try {
        // the sequence, tracked: fresh frames each time (the host route keeps a frame's cloud in the frame)
        auto load = [&]() {
            vector<RGBDFrame::Ptr> kfs;
            Tracker tracker(para, vp); FrameReader rd(para, FrameReader::KITTI);
            while (RGBDFrame::Ptr f = rd.next()) { tracker.updateFrame(f); kfs.push_back(f); }
            return kfs;
        };
        Tracker::Ptr tracker(new Tracker(para, vp));
        PoseGraph pg(para, tracker);
        ParameterReader on = para; on.set("mapper_carve", "1");
        ParameterReader on_host = on; on_host.set("mapper_device_map", "0");
        QuietMapper off_m(para, pg), dev_m(on, pg), host_m(on_host, pg);
        CHECK("switch_defaults_to_off", !off_m.carves() && dev_m.carves() && host_m.carves());
        vector<RGBDFrame::Ptr> k0 = load(), kd = load(), kh = load();
        const size_t n = k0.size();
        CHECK("sequence_has_frames", n >= 6 && kd.size() == n && kh.size() == n);
        if (n < 3) { cout << "FAILED" << endl; return fails ? fails : 1; }
        bool poses = true;
        for (size_t i = 0; i < n; i++) {
            const Eigen::Isometry3d a = k0[i]->getTransform(), b = kd[i]->getTransform(), c = kh[i]->getTransform();
            poses = poses && memcmp(a.data(), b.data(), 16 * sizeof(double)) == 0 && memcmp(a.data(), c.data(), 16 * sizeof(double)) == 0;
        }
        CHECK("tracking_is_repeatable", poses);
        const int w = k0[0]->depth.cols, h = k0[0]->depth.rows; const double md = para.getData<double>("mapper_max_distance", 40.0);
        const ssm_camera cam = Mapper::cameraOf(k0[0]);
        ssm::Device& d = off_m.dev_(w, h);

        // what the calls that exist give: the uncarved camera-frame clouds
        vector<vector<ssm_point>> plain(n);
        bool off_same = true, box_everywhere = true;
        for (size_t i = 0; i < n; i++) {
            plain[i].resize((size_t)w * h); int m = 0;
            d.check(ssm_backproject(d.ctx(), k0[i]->depth.ptr<uint16_t>(), k0[i]->rgb.data, k0[i]->semantic.data, w, h, &cam, nullptr, md, plain[i].data(), (int)plain[i].size(), &m), "ssm_backproject");
            plain[i].resize((size_t)m);
            off_same = off_same && same(off_m.deviceRoute(k0[i]), plain[i]) && same(off_m.hostRoute(k0[i]), plain[i]);
            box_everywhere = box_everywhere && (i < U ? box_points(plain[i], cam) > 1000 : box_points(plain[i], cam) < 50);
            cout << "key-frame " << i << " at x " << k0[i]->getTransform().data()[12] << ": " << m << " points, " << box_points(plain[i], cam) << " of the box" << endl;
        }
        CHECK("switch_off_clouds_as_before", off_same && !off_m.carveInfoOf(k0[0], nullptr));
        CHECK("without_carving_the_box_is_in_every_cloud_until_it_leaves", box_everywhere && U >= 2 && U + 1 < n);

        // the two routes
        dev_m.carveUpTo(kd); host_m.carveUpTo(kh);
        bool routes = dev_m.carvedViews() == (int)n - 1 && host_m.carvedViews() == (int)n - 1, infos = true;
        vector<vector<ssm_point>> carved(n);
        for (size_t i = 0; i < n; i++) {
            carved[i] = host_m.hostRoute(kh[i]);
            routes = routes && same(dev_m.deviceRoute(kd[i]), carved[i]);
            ssm_carve_info a{}, b{};
            const bool ha = dev_m.carveInfoOf(kd[i], &a), hb = host_m.carveInfoOf(kh[i], &b);
            infos = infos && ha == hb && ha == (i + 1 < n) && memcmp(&a, &b, sizeof a) == 0;
        }
        CHECK("routes_agree", routes);
        CHECK("routes_record_the_same_figures", infos);

        // the host function, view after view, on the uncarved clouds
        ssm_carve_params P; ssm_carve_params_default(&P);
        const int window = 5;
        vector<vector<ssm_point>> want = plain; vector<vector<uint8_t>> run(n);
        for (size_t i = 0; i < n; i++) run[i].assign(plain[i].size(), 0);
        vector<ssm_carve_info> sum(n); for (size_t i = 0; i < n; i++) { memset(&sum[i], 0, sizeof sum[i]); sum[i].n_in = sum[i].n_kept = (int)plain[i].size(); }
        for (size_t j = 1; j < n; j++) for (size_t i = j > (size_t)window ? j - window : 0; i < j; i++) {
            vector<ssm_point> out(max(want[i].size(), (size_t)1)); int m = 0; ssm_carve_info I{};
            const Eigen::Isometry3d Tv = k0[j]->getTransform(), Tc = k0[i]->getTransform();
            const int rc = ssm_carve_host(k0[j]->depth.ptr<uint16_t>(), w, h, &cam, Tv.data(), want[i].data(), (int)want[i].size(), Tc.data(), run[i].data(), &P, out.data(), (int)out.size(), &m, &I, nullptr, nullptr);
            if (rc != SSM_OK) throw runtime_error("ssm_carve_host failed");
            out.resize((size_t)m); want[i].swap(out); run[i].resize((size_t)m);
            sum[i].n_kept = I.n_kept; sum[i].unknown += I.unknown; sum[i].occluded += I.occluded; sum[i].supported += I.supported; sum[i].seen_through += I.seen_through; sum[i].removed += I.removed;
        }
        bool composed = true, counters = true;
        for (size_t i = 0; i < n; i++) {
            composed = composed && same(carved[i], want[i]);
            ssm_carve_info b{}; if (host_m.carveInfoOf(kh[i], &b)) composed = composed && memcmp(&b, &sum[i], sizeof b) == 0;
            const vector<uint8_t>* r = host_m.runOf(kh[i]);
            counters = counters && (i + 1 == n ? r == nullptr : (r && *r == run[i]));
        }
        CHECK("carving_is_the_host_function_view_after_view", composed);
        CHECK("counters_stay_beside_the_host_clouds", counters);

        // the box, point by point.  Copy i of the box stands still in the world, so view j shows it 2 (j - i) pixels to the left of where key-frame i saw it.  A view
        // from frame U on has no box: where it has valid depth, the ground behind (rows 32..85: disparity <= 35 against the box's 40, 14 % farther, the tolerance is
        // 5 cm + 2 %) is seen THROUGH the copy.  A point that two such views of its window show so has two votes in a row (nothing in between can support it) and
        // must be gone.  The validity of the views' depth is read from their images; nothing is read from what carving did
        bool all_gone = true, most = true; size_t rest_in = 0, rest_lost = 0, box_lost = 0;
        for (size_t i = 0; i < n; i++) {
            set<pair<int, int>> left;
            for (const ssm_point& p : carved[i]) left.insert({px_u(p, cam), px_v(p, cam)});
            size_t b0 = 0, must = 0, still = 0;
            for (const ssm_point& p : plain[i]) {
                if (!in_box(p, cam)) continue;
                b0++;
                const int u = px_u(p, cam), v = px_v(p, cam);
                if (v < ROW0 || v >= ROW1) continue;
                int votes = 0;
                for (size_t j = max(i + 1, U); j < n && j <= i + (size_t)window; j++) votes += far_ground(k0[j], u - SHIFT * (int)(j - i), v, cam);
                if (votes >= 2) { must++; still += left.count({u, v}); }
            }
            const size_t b1 = box_points(carved[i], cam);
            cout << "key-frame " << i << ": kept " << carved[i].size() << " of " << plain[i].size() << ", of the box " << b1 << " of " << b0 << "; " << must << " must go, " << still << " of them still there" << endl;
            all_gone = all_gone && still == 0;
            // rows 32..85 are 54 of the box's 66 rows, and a textured ground plane without a foreground object gives SGBM nothing to lose: at least half of every copy
            if (i < U) most = most && 2 * must >= b0 && 2 * (b0 - b1) >= b0;
            rest_in += plain[i].size() - b0; rest_lost += (plain[i].size() - carved[i].size()) - (b0 - b1); box_lost += b0 - b1;
        }
        CHECK("every_box_point_two_later_views_see_through_is_gone", all_gone);
        CHECK("every_copy_of_the_box_loses_most_of_its_points", most && box_lost > 0);

        // with a window of 1 a cloud is judged once: by a view that still has the box (the copy, 2 pixels off, is behind it: supported), or by view U alone (one vote).
        // Every point at least 12 pixels inside the box's sides must stay
        {
            ParameterReader w1 = on_host; w1.set("mapper_carve_window", "1");
            QuietMapper w1_m(w1, pg);
            vector<RGBDFrame::Ptr> k1 = load();
            w1_m.carveUpTo(k1);
            bool stay = k1.size() == n; size_t deep = 0;
            for (size_t i = 0; i < U && stay; i++) {
                set<pair<int, int>> left;
                for (const ssm_point& p : w1_m.hostRoute(k1[i])) left.insert({px_u(p, cam), px_v(p, cam)});
                for (const ssm_point& p : plain[i]) {
                    const int u = px_u(p, cam), v = px_v(p, cam);
                    if (!in_box(p, cam) || v < ROW0 || v >= ROW1 || u < BOX_C0 + 12 || u >= BOX_C1 - 12) continue;
                    deep++; stay = stay && left.count({u, v}) == 1;
                }
            }
            CHECK("with_a_window_of_one_nothing_deep_inside_the_box_leaves", stay && deep > 1000);
        }

        // the published map: a Mapper whose viewer finds all the key-frames, makes every one a view and then runs its first update, a REBUILD from every second key-frame
        {
            Mapper::PointCloud::Ptr maps[2];
            for (int c = 0; c < 2; c++) {
                PoseGraph g(para, tracker);
                g.keyframes = load();
                Mapper m(c ? on : para, g);
                for (int t = 0; t < 20000 && m.updates() < 1 && !m.viewerFailed; t++) this_thread::sleep_for(chrono::milliseconds(1));
                maps[c] = m.getGlobalMap();
                m.shutdown();
                if (m.viewerFailed || m.deviceMapFellBack) throw runtime_error("the viewer failed");
            }
            const double x0 = k0[0]->getTransform().data()[12], x1 = k0[U - 1]->getTransform().data()[12];
            const size_t t_off = trail_voxels(maps[0], cam, x0, x1), t_on = trail_voxels(maps[1], cam, x0, x1);
            // what the rebuild may publish: the points the carved clouds of its key-frames (every second one) still hold, in the world.  A voxel's centroid lies in the
            // cell of the points it was made of, so every voxel in the trail must have such a point within one cell's diagonal; a voxel where carving took
            // everything has none
            vector<array<float, 3>> kept;
            for (size_t i = 0; i < n; i += 2) {
                const Eigen::Isometry3d T = k0[i]->getTransform(); const double* t = T.data();
                for (const ssm_point& p : carved[i]) {
                    const double x = p.x, y = p.y, z = p.z;
                    kept.push_back({(float)(t[0] * x + t[4] * y + t[8] * z + t[12]), (float)(t[1] * x + t[5] * y + t[9] * z + t[13]), (float)(t[2] * x + t[6] * y + t[10] * z + t[14])});
                }
            }
            const double zb = cam.fx * BASELINE / BOX_DISP, diag2 = 3 * 0.1 * 0.1 * 1.01;
            size_t orphans = 0;
            if (maps[1]) for (const Mapper::PointT& v : maps[1]->points) {
                if (!(fabs(v.z - zb) < 0.25)) continue;
                bool near = false;
                for (size_t q = 0; q < kept.size() && !near; q++) { const double dx = kept[q][0] - v.x, dy = kept[q][1] - v.y, dz = kept[q][2] - v.z; near = dx * dx + dy * dy + dz * dz <= diag2; }
                orphans += !near;
            }
            size_t survivors = 0;
            for (size_t i = 0; i < U; i += 2) for (const ssm_point& p : carved[i]) survivors += in_box(p, cam) && px_v(p, cam) >= ROW0 + 2 && px_v(p, cam) < ROW1 - 2;
            cout << "voxels in the trail: " << t_off << " without carving, " << t_on << " with; " << survivors << " box points survive there; " << orphans << " voxels at the box's depth without a kept point; map " << (maps[0] ? maps[0]->points.size() : 0) << " / " << (maps[1] ? maps[1]->points.size() : 0) << endl;
            // (one copy of the box is 76 x 50 pixels of 13 mm at 6.9 m: about 1.0 m x 0.65 m, 60 voxels of 0.1 m)
            CHECK("without_carving_the_trail_is_in_the_published_map", t_off >= 50);
            CHECK("after_the_rebuild_no_voxel_is_left_in_the_trail", maps[1] && maps[1]->points.size() > 1000 && t_on < t_off && t_on <= survivors && orphans == 0);
        }
        CHECK("the_last_key_frame_is_whole", same(carved[n - 1], plain[n - 1]));
        const double share = rest_in ? (double)rest_lost / (double)rest_in : 1.0;
        cout << "outside the box: lost " << rest_lost << " of " << rest_in << " points, share " << share << "; of the box: " << box_lost << endl;
        // the bound is reasoned, not measured: a static point can only go where the stereo depth of two later views in a row is wrong by more than the tolerance
        // (5 cm + 2 %) -- the band of a few pixels around the box's outline where SGBM smears the depth edge: 2 (66 + 80) pixels of outline, 4 wide, in 400 x 120
        // pixels are 2.4 %; twice that is the limit
        CHECK("the_static_scene_loses_a_small_share", share < 0.05);
    } catch (const exception& e) { cout << "FAIL exception " << e.what() << endl; fails++; }
    cout << (fails ? "FAILED" : "ALL PASSED") << endl;
    return fails;
}
