// test_grid -- the ground grid through Mapper on the device (run by tests/test_gpu_grid_host.py under -m gpu).  The scene is the analytic KITTI-layout scene of
// test_align.cpp: a camera 1.6 m above a ground plane drives forward half a metre per key-frame past a box that stands beside the lane; every depth image is
// ray-cast from the key-frame's TRUE pose (depth units of 1 mm), which is also the pose the Mapper gets.  The semantic images are painted here: the plane within
// the lane (|x| < 1 m) is Road, the plane beyond it Pavement, the box Car.  mapper_grid=0 leaves everything as it was; with 1 the device route (deviceCloud +
// ssm_grid_clouds) and the host route (frame->pointcloud + ssm_grid_points) give the same bytes, which are those of ssm_grid_host on the fetched clouds; the
// written PNG files and grid.txt read back as the fetched arrays and the spec; and against the scene's truth every observed cell inside the box's footprint is an
// obstacle labelled Car, every observed lane cell away from the box is drivable, every such pavement cell walkable, and its ground height lies within the
// quantisation bound of DESIGN.md s.19 of the true plane.  With mapper_carve=1 and mapper_align=1 on top it still builds and both routes agree; and a Mapper
// whose viewer thread runs builds the same grid as it ends.  The grid uses 0.5 m cells and ground_radius 3: the window (3.5 m) is wider than the box (1.5 m),
// which the neighbourhood minimum needs to find the ground beside an obstacle whose top is seen from above (limits).
// Prints one "PASS name" / "FAIL name" line per check; exit code = failures.
#include "test_lane_scene.h"
struct Grid { ssm_grid_params P{}; Mapper::GridInfo info; vector<uint8_t> cls, gl, ol; vector<int32_t> gq, tq; vector<uint32_t> n, nh; };
static Grid grid_of(const Mapper& m) { Grid g; g.P = m.gridParams(); g.info = m.gridInfo(); m.gridFetch(&g.cls, &g.gl, &g.ol, &g.gq, &g.tq, &g.n, &g.nh); return g; }
static bool same_grid(const Grid& a, const Grid& b)
{
    return a.info.built && b.info.built && memcmp(&a.P, &b.P, sizeof a.P) == 0 && memcmp(&a.info.counts, &b.info.counts, sizeof a.info.counts) == 0 && a.cls == b.cls && a.gl == b.gl &&
           a.ol == b.ol && a.gq == b.gq && a.tq == b.tq && a.n == b.n && a.nh == b.nh;
}


int main(int argc, char** argv)
{
    if (argc < 3) { cerr << "usage: test_grid <parameters> <output directory>" << endl; return 2; }
    ParameterReader para(argv[1]);
    const string out_dir = argv[2];
    para.set("image_width", "400"); para.set("image_height", "120"); para.set("orb_levels", "3"); para.set("orb_features", "300");
    para.set("camera.cx", "200.0"); para.set("camera.cy", "40.0"); para.set("camera.fx", "300.0"); para.set("camera.fy", "300.0"); para.set("camera.scale", "1000.0");
    para.set("uv_disparity", "0"); para.set("motion_semantic_fuse", "0");
    VisualOdometryStereo::parameters vp; vp.calib.f = 300.0; vp.calib.cu = 200.0; vp.calib.cv = 40.0; vp.base = 0.5;
    try {
        const CAMERA_INTRINSIC_PARAMETERS camera = para.getCamera();
        auto load = [&]() {          // the sequence: fresh frames each time (the host route keeps a frame's cloud in the frame)
            vector<RGBDFrame::Ptr> kfs;
            for (int j = 0; j < N; j++) {
                RGBDFrame::Ptr f(new RGBDFrame);
                f->id = j; f->camera = camera;
                vector<uint8_t> hit;
                cast(STEP * j, camera, f->depth, &hit);
                f->rgb.create(H, W, CV_8UC3); f->semantic.create(H, W, CV_8UC3);
                for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) {
                    uint8_t* c = f->rgb.ptr<uint8_t>(y) + 3 * x; c[0] = (uint8_t)(x + j); c[1] = (uint8_t)(y * 2); c[2] = (uint8_t)(x ^ y);
                    uint8_t* s = f->semantic.ptr<uint8_t>(y) + 3 * x;
                    const int what = hit[(size_t)y * W + x];          // palette colours (BGR): Road 4, Pavement 5, Car 9
                    if (what == HIT_PAVEMENT) { s[0] = 222; s[1] = 40; s[2] = 60; } else if (what == HIT_BOX) { s[0] = 128; s[1] = 0; s[2] = 64; } else { s[0] = 128; s[1] = 64; s[2] = 128; }
                }
                Eigen::Isometry3d T = Eigen::Isometry3d::Identity(); T(2, 3) = STEP * j;
                f->setTransform(T);
                kfs.push_back(f);
            }
            return kfs;
        };
        Tracker::Ptr tracker(new Tracker(para, vp));
        PoseGraph pg(para, tracker);
        ParameterReader on = para; on.set("mapper_grid", "1"); on.set("mapper_grid_cell", "0.5"); on.set("mapper_grid_ground_radius", "3");
        ParameterReader on_files = on; on_files.set("mapper_grid_dir", out_dir);          // (the device route writes the files)
        ParameterReader on_host = on; on_host.set("mapper_device_map", "0");
        ParameterReader all_on = on; all_on.set("mapper_carve", "1"); all_on.set("mapper_align", "1");
        ParameterReader all_host = all_on; all_host.set("mapper_device_map", "0");
        QuietMapper off_m(para, pg), dev_m(on_files, pg), host_m(on_host, pg), adev_m(all_on, pg), ahost_m(all_host, pg);
        CHECK("switch_defaults_to_off", !off_m.buildsGrid() && dev_m.buildsGrid() && host_m.buildsGrid() && !off_m.gridInfo().built && !dev_m.gridInfo().built);
        vector<RGBDFrame::Ptr> k0 = load(), kd = load(), kh = load(), kad = load(), kah = load();
        const size_t n = k0.size();
        const double md = para.getData<double>("mapper_max_distance", 40.0);
        ssm_camera cam; cam.cx = camera.cx; cam.cy = camera.cy; cam.fx = camera.fx; cam.fy = camera.fy; cam.scale = camera.scale;
        ssm::Device& d = off_m.dev_(W, H);

        // switch off: the clouds are what the calls that exist give, and nothing is built
        vector<vector<ssm_point>> plain(n);
        bool off_same = true;
        for (size_t i = 0; i < n; i++) {
            plain[i].resize((size_t)W * H); int m = 0;
            d.check(ssm_backproject(d.ctx(), k0[i]->depth.ptr<uint16_t>(), k0[i]->rgb.data, k0[i]->semantic.data, W, H, &cam, nullptr, md, plain[i].data(), (int)plain[i].size(), &m), "ssm_backproject");
            plain[i].resize((size_t)m);
            off_same = off_same && same(off_m.cloudNow(k0[i]), plain[i]) && plain[i].size() > 10000;
        }
        vector<uint8_t> none;
        CHECK("switch_off_clouds_as_before_and_no_grid", off_same && !off_m.gridInfo().built && !off_m.gridFetch(&none, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) && none.empty());

        // the two routes, and the host function on the fetched clouds
        dev_m.buildGrid(kd); host_m.buildGrid(kh);
        const Grid gd = grid_of(dev_m), gh = grid_of(host_m);
        CHECK("routes_give_the_same_bytes", same_grid(gd, gh));
        bool untouched = true;
        for (size_t j = 0; j < n; j++) untouched = untouched && same(dev_m.cloudNow(kd[j]), plain[j]) && same(host_m.cloudNow(kh[j]), plain[j]);
        CHECK("the_grid_changes_no_cloud", untouched);
        const ssm_grid_params P = gd.P;
        const size_t nc = (size_t)P.nx * P.ny;
        cout << "grid: " << P.nx << " x " << P.ny << " cells of " << P.cell << " m from (" << P.x0 << ", " << P.y0 << "); used " << gd.info.counts.n_used << " of " << gd.info.counts.n_in
             << " points; drivable " << gd.info.counts.drivable << " walkable " << gd.info.counts.walkable << " other " << gd.info.counts.other_ground << " obstacle " << gd.info.counts.obstacle << endl;
        // the extent: the positions (x = 0, z = 0 .. 3.5) widened by max_distance, in whole cells
        const bool extent = P.x0 == floor(-md / P.cell) * P.cell && P.y0 == floor(-md / P.cell) * P.cell && P.nx == (int)(ceil(md / P.cell) - floor(-md / P.cell)) &&
                            P.ny == (int)(ceil((STEP * (N - 1) + md) / P.cell) - floor(-md / P.cell)) && P.cell == 0.5 && P.ground_radius == 3;
        CHECK("the_extent_is_the_key_frames_box_widened_by_max_distance", extent);
        {
            Grid g; g.P = P; g.info.built = true;
            g.cls.resize(nc); g.gl.resize(nc); g.ol.resize(nc); g.gq.resize(nc); g.tq.resize(nc); g.n.resize(nc); g.nh.resize(nc);
            vector<const ssm_point*> pts; vector<int32_t> cnt; vector<double> poses;
            for (size_t i = 0; i < n; i++) { pts.push_back(plain[i].data()); cnt.push_back((int32_t)plain[i].size()); const Eigen::Isometry3d T = k0[i]->getTransform(); poses.insert(poses.end(), T.data(), T.data() + 16); }
            if (ssm_grid_host(pts.data(), cnt.data(), poses.data(), (int)n, &P, g.cls.data(), g.gl.data(), g.ol.data(), g.gq.data(), g.tq.data(), g.n.data(), g.nh.data(), nullptr, &g.info.counts) != SSM_OK)
                throw runtime_error("ssm_grid_host failed");
            CHECK("the_grid_is_the_host_function_on_the_fetched_clouds", same_grid(gd, g));
        }

        // the files
        {
            cv::Mat col, hgt; col.create(P.ny, P.nx, CV_8UC3); hgt.create(P.ny, P.nx, CV_16UC1);
            ssm_grid_colours(gd.cls.data(), gd.gl.data(), gd.ol.data(), gd.gq.data(), P.nx, P.ny, P.h_min, col.data, hgt.ptr<uint16_t>());
            const cv::Mat rc = ssm::imreadPNG(out_dir + "/grid_colour.png", -1), rh = ssm::imreadPNG(out_dir + "/grid_height.png", -1);
            bool ok = !rc.empty() && !rh.empty() && rc.rows == P.ny && rc.cols == P.nx && rc.type() == CV_8UC3 && rh.rows == P.ny && rh.cols == P.nx && rh.type() == CV_16UC1;
            for (int y = 0; ok && y < P.ny; y++) ok = memcmp(rc.ptr<uint8_t>(y), col.ptr<uint8_t>(y), (size_t)P.nx * 3) == 0 && memcmp(rh.ptr<uint8_t>(y), hgt.ptr<uint8_t>(y), (size_t)P.nx * 2) == 0;
            ifstream txt(out_dir + "/grid.txt");
            string key; double x0 = 0, y0 = 0, cell = 0, h_min = 0, G[12]; int nx = 0, ny = 0;
            bool read = bool(txt >> key >> x0) && key == "x0" && bool(txt >> key >> y0) && key == "y0" && bool(txt >> key >> cell) && key == "cell" && bool(txt >> key >> nx) && key == "nx" &&
                        bool(txt >> key >> ny) && key == "ny" && bool(txt >> key >> h_min) && key == "h_min" && bool(txt >> key) && key == "G";
            for (int i = 0; read && i < 12; i++) read = bool(txt >> G[i]) && G[i] == P.G[i];
            CHECK("the_written_files_read_back_as_the_fetched_arrays_and_the_spec", ok && read && x0 == P.x0 && y0 == P.y0 && cell == P.cell && nx == P.nx && ny == P.ny && h_min == P.h_min);
        }

        // against the scene's truth.  A cell (cx, cy) is the square [x0 + cx cell, + cell] x [y0 + cy cell, + cell] of the ground (grid x = world x, grid y = world z)
        {
            const int R = P.ground_radius + 1;
            const int bx0 = (int)floor((BOX_LO[0] - P.x0) / P.cell), bx1 = (int)ceil((BOX_HI[0] - P.x0) / P.cell) - 1, by0 = (int)floor((BOX_LO[2] - P.y0) / P.cell),
                      by1 = (int)ceil((BOX_HI[2] - P.y0) / P.cell) - 1;          // the cells the footprint touches
            const double plane_q = -GROUND * 1024.0, tan_max = (H - 1 - camera.cy) / camera.fy;
            long long in_box = 0, box_ok = 0, lane = 0, lane_ok = 0, pave = 0, pave_ok = 0, height_ok = 0; double worst = 0, worst_bound = 0, margin = -1e30;
            for (int cy = 0; cy < P.ny; cy++) for (int cx = 0; cx < P.nx; cx++) {
                const size_t i = (size_t)cy * P.nx + cx;
                if (gd.cls[i] == 0) continue;
                const double xa = P.x0 + cx * P.cell, xb = xa + P.cell, ya = P.y0 + cy * P.cell, yb = ya + P.cell;
                if (xa >= BOX_LO[0] && xb <= BOX_HI[0] && ya >= BOX_LO[2] && yb <= BOX_HI[2]) { in_box++; box_ok += gd.cls[i] == 4 && gd.ol[i] == 9; continue; }
                if (cx >= bx0 - R && cx <= bx1 + R && cy >= by0 - R && cy <= by1 + R) continue;          // within ground_radius + 1 cells of the footprint: not judged
                const bool is_lane = xa >= -LANE && xb <= LANE, is_pave = xb <= -LANE || xa >= LANE;
                if (!is_lane && !is_pave) continue;
                if (is_lane) { lane++; lane_ok += gd.cls[i] == 1; } else { pave++; pave_ok += gd.cls[i] == 2; }
                // The bound, in height units of 2^-10 m.  A ground pixel's depth is rounded to 1 / scale m, half a unit at most; its height is depth
                // times the row's tangent, and the tangent under which a key-frame at forward distance dz sees the plane is GROUND / dz, so the height is off by at
                // most 1024 (0.5 / scale) t with t the largest such tangent over the key-frames that can see any of the cell (its far edge at dz >= GROUND / tan_max,
                // tan_max the bottom row's, which also caps t).  Rounding the height to a unit adds 0.5, the floor of the mean up to 1, float32 coordinates (|y| < 2 m:
                // 2^-23 relative) 0.01.
                double t = 0;
                for (int j = 0; j < N; j++) if (yb - STEP * j >= GROUND / tan_max) t = max(t, min(tan_max, GROUND / max(ya - STEP * j, 1e-9)));
                if (t == 0) t = tan_max;
                const double bound = 1024.0 * (0.5 / camera.scale) * t + 0.5 + 1.0 + 0.01, err = fabs((double)gd.gq[i] - plane_q);
                height_ok += err <= bound;
                if (err - bound > margin) { margin = err - bound; worst = err; worst_bound = bound; }
            }
            cout << "truth: " << in_box << " cells inside the box's footprint, " << box_ok << " of them obstacles labelled Car; " << lane << " lane cells, " << lane_ok << " drivable; " << pave
                 << " pavement cells, " << pave_ok << " walkable; " << height_ok << " of " << lane + pave << " ground heights within the bound (closest call: off by " << worst << " units, bound "
                 << worst_bound << ")" << endl;
            CHECK("cells_inside_the_box_are_obstacles_labelled_car", in_box > 0 && box_ok == in_box);
            CHECK("lane_cells_are_drivable", lane > 0 && lane_ok == lane);
            CHECK("pavement_cells_are_walkable", pave > 0 && pave_ok == pave);
            CHECK("ground_heights_lie_within_the_quantisation_bound_of_the_plane", lane + pave > 0 && height_ok == lane + pave);
        }

        // with carving and alignment on top, key-frame by key-frame as the viewer does it, then the grid; both routes agree
        adev_m.alignCarveUpTo(kad); ahost_m.alignCarveUpTo(kah);
        adev_m.buildGrid(kad); ahost_m.buildGrid(kah);
        const Grid ad = grid_of(adev_m), ah = grid_of(ahost_m);
        cout << "with mapper_carve=1 and mapper_align=1: used " << ad.info.counts.n_used << " of " << ad.info.counts.n_in << " points, obstacle cells " << ad.info.counts.obstacle << endl;
        CHECK("with_carving_and_alignment_both_routes_agree", same_grid(ad, ah) && ad.info.counts.n_used > 10000 && adev_m.carvedViews() == (int)n - 1 && adev_m.alignedKeyframes() == (int)n);

        // a Mapper whose viewer runs builds the same grid as it ends
        {
            PoseGraph g(para, tracker);
            g.keyframes = load();
            Mapper m(on, g);
            for (int t = 0; t < 20000 && m.updates() < 1 && !m.viewerFailed; t++) this_thread::sleep_for(chrono::milliseconds(1));
            Mapper::PointCloud::Ptr map = m.getGlobalMap();
            m.shutdown();
            if (m.viewerFailed || m.deviceMapFellBack) throw runtime_error("the viewer failed");
            CHECK("the_viewer_builds_the_grid_as_it_ends", same_grid(grid_of(m), gd) && map && map->points.size() > 1000);
        }
        // an extent beyond 2^24 cells is skipped with a notice
        {
            ParameterReader tiny = on_host; tiny.set("mapper_grid_cell", "0.01");
            QuietMapper m(tiny, pg);
            vector<RGBDFrame::Ptr> k = load();
            m.buildGrid(k);
            CHECK("an_extent_beyond_the_cell_limit_is_skipped", !m.gridInfo().built && m.gridInfo().skipped && m.gridParams().nx == 0);
        }
    } catch (const exception& e) { cout << "FAIL exception " << e.what() << endl; fails++; }
    cout << (fails ? "FAILED" : "ALL PASSED") << endl;
    return fails;
}
