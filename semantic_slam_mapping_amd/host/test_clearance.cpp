// test_clearance -- the clearance map through Mapper on the device (run by tests/test_gpu_clearance_host.py under -m gpu).  The scene is the shared lane scene as
// it is (test_lane_scene.h): the lane Road, the sides Pavement, the box Car; every depth image is ray-cast from the key-frame's TRUE pose, which the Mapper gets.
// mapper_clearance=0 leaves everything as it was -- clouds, grid, objects, the published map, no clearance map; with 1 the device route and the host route to the
// clouds give the same bytes, which are those of ssm_clearance_cells_host on the fetched class image; no traversable cell lies within r2 of an obstacle cell; every
// reachable cell is drivable and connected to the seed; the seed is the snapped cell of the last key-frame's camera; the lane cells that geometry says must be
// reachable are (derived below); the three files read back as the fetched arrays; a grid built only for the clearance map writes no grid file; with
// mapper_objects=1, carving and alignment on top both routes still agree; and a Mapper whose viewer thread runs makes the same map as it ends.  The grid uses 0.5 m
// cells and ground_radius 3 as test_grid.cpp does.  Prints one "PASS name" / "FAIL name" line per check; exit code = failures.
#include "test_lane_scene.h"
#include <sys/stat.h>
struct Clearance { ssm_grid_params P{}; Mapper::ClearanceInfo info; vector<uint32_t> d2; vector<int32_t> nearest; vector<uint8_t> reach; };
static Clearance clearance_of(const Mapper& m) { Clearance c; c.P = m.gridParams(); c.info = m.clearanceInfo(); m.clearanceFetch(&c.d2, &c.nearest, &c.reach); return c; }
static bool same_clearance(const Clearance& a, const Clearance& b)
{
    return a.info.built && b.info.built && memcmp(&a.P, &b.P, sizeof a.P) == 0 && memcmp(&a.info.counts, &b.info.counts, sizeof a.info.counts) == 0 && a.info.seed_cx == b.info.seed_cx &&
           a.info.seed_cy == b.info.seed_cy && a.d2 == b.d2 && a.nearest == b.nearest && a.reach == b.reach;
}
static bool exists(const string& path) { struct stat st; return stat(path.c_str(), &st) == 0; }

int main(int argc, char** argv)
{
    if (argc < 3) { cerr << "usage: test_clearance <parameters> <output directory>" << endl; return 2; }
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
        ParameterReader grid_only = para; grid_only.set("mapper_grid", "1"); grid_only.set("mapper_grid_cell", "0.5"); grid_only.set("mapper_grid_ground_radius", "3"); grid_only.set("mapper_objects", "1");
        ParameterReader on = grid_only; on.set("mapper_clearance", "1");
        ParameterReader on_files = on; on_files.set("mapper_clearance_dir", out_dir);          // (the device route writes the files)
        ParameterReader on_host = on; on_host.set("mapper_device_map", "0");
        ParameterReader all_on = on; all_on.set("mapper_carve", "1"); all_on.set("mapper_align", "1");
        ParameterReader all_host = all_on; all_host.set("mapper_device_map", "0");
        ParameterReader no_grid = on; no_grid.set("mapper_grid", "0"); no_grid.set("mapper_objects", "0"); no_grid.set("mapper_grid_dir", out_dir + "/none");
        QuietMapper off_m(grid_only, pg), dev_m(on_files, pg), host_m(on_host, pg), adev_m(all_on, pg), ahost_m(all_host, pg), ng_m(no_grid, pg);
        CHECK("switch_defaults_to_off", !off_m.mapsClearance() && dev_m.mapsClearance() && host_m.mapsClearance() && !off_m.clearanceInfo().built && !dev_m.clearanceInfo().built);
        vector<RGBDFrame::Ptr> k0 = load(), kd = load(), kh = load(), kad = load(), kah = load(), kn = load();
        const size_t n = k0.size();
        const double md = para.getData<double>("mapper_max_distance", 40.0);
        ssm_camera cam; cam.cx = camera.cx; cam.cy = camera.cy; cam.fx = camera.fx; cam.fy = camera.fy; cam.scale = camera.scale;
        ssm::Device& d = off_m.dev_(W, H);
        vector<vector<ssm_point>> plain(n);
        for (size_t i = 0; i < n; i++) {
            plain[i].resize((size_t)W * H); int m = 0;
            d.check(ssm_backproject(d.ctx(), k0[i]->depth.ptr<uint16_t>(), k0[i]->rgb.data, k0[i]->semantic.data, W, H, &cam, nullptr, md, plain[i].data(), (int)plain[i].size(), &m), "ssm_backproject");
            plain[i].resize((size_t)m);
        }

        // switch off: the grid, the objects and the clouds are what they are with the switch on, there is no clearance map
        off_m.buildGrid(k0); dev_m.buildGrid(kd); host_m.buildGrid(kh);
        vector<uint8_t> cls;
        {
            vector<uint8_t> a[3], b[3]; vector<int32_t> aq[2], bq[2]; vector<uint32_t> an[2], bn[2]; vector<ssm_object> ra, rb; vector<int32_t> ia_, ib_; vector<uint32_t> none;
            off_m.gridFetch(&a[0], &a[1], &a[2], &aq[0], &aq[1], &an[0], &an[1]); dev_m.gridFetch(&b[0], &b[1], &b[2], &bq[0], &bq[1], &bn[0], &bn[1]);
            off_m.objectsFetch(&ra, &ia_); dev_m.objectsFetch(&rb, &ib_);
            const ssm_grid_params pa = off_m.gridParams(), pb = dev_m.gridParams(); const ssm_grid_info ia = off_m.gridInfo().counts, ib = dev_m.gridInfo().counts;
            const ssm_objects_info oa = off_m.objectsInfo().counts, ob = dev_m.objectsInfo().counts;
            bool same_clouds = true;
            for (size_t j = 0; j < n; j++) same_clouds = same_clouds && same(off_m.cloudNow(k0[j]), plain[j]) && same(dev_m.cloudNow(kd[j]), plain[j]) && same(host_m.cloudNow(kh[j]), plain[j]);
            CHECK("switch_off_grid_objects_and_clouds_as_before_and_no_clearance", off_m.gridInfo().built && memcmp(&pa, &pb, sizeof pa) == 0 && memcmp(&ia, &ib, sizeof ia) == 0 && a[0] == b[0] && a[1] == b[1] &&
                  a[2] == b[2] && aq[0] == bq[0] && aq[1] == bq[1] && an[0] == bn[0] && an[1] == bn[1] && same_clouds && memcmp(&oa, &ob, sizeof oa) == 0 && ra.size() == rb.size() && ra.size() == 1 &&
                  memcmp(ra.data(), rb.data(), sizeof(ssm_object)) == 0 && ia_ == ib_ && !off_m.clearanceInfo().built && !off_m.clearanceFetch(&none, nullptr, nullptr) && none.empty());
            cls = b[0];
        }

        // the two routes, and the host function on the fetched class image
        const Clearance cd = clearance_of(dev_m), ch = clearance_of(host_m);
        CHECK("routes_give_the_same_bytes", same_clearance(cd, ch));
        const ssm_grid_params P = cd.P;
        const int nx = P.nx, ny = P.ny;
        const size_t nc = (size_t)nx * ny;
        const ssm_clearance_info I = cd.info.counts;
        {
            Clearance g; g.P = P; g.info = cd.info; g.d2.resize(nc); g.nearest.resize(nc); g.reach.resize(nc);
            ssm_clearance_params C; ssm_clearance_params_default(&C); C.cell = P.cell; C.seed_cx = cd.info.seed_cx; C.seed_cy = cd.info.seed_cy;
            if (ssm_clearance_cells_host(cls.data(), nx, ny, &C, g.d2.data(), g.nearest.data(), g.reach.data(), &g.info.counts) != SSM_OK) throw runtime_error("ssm_clearance_cells_host failed");
            CHECK("the_map_is_the_host_function_on_the_fetched_class_image", cls.size() == nc && same_clearance(cd, g));
        }
        cout << "clearance: " << nx << " x " << ny << " cells of " << P.cell << " m, r2 " << I.r2 << ", " << I.blocked << " blocked, " << I.free_cells << " free, " << I.traversable << " traversable in "
             << I.components << " components, " << I.reachable << " reachable, seed cell " << I.seed_cell << " (camera cell " << cd.info.seed_cx << ", " << cd.info.seed_cy << "), max d2 reachable "
             << I.max_d2_reachable << endl;
        // every obstacle cell against every traversable cell; the reachable set is the 4-connected fill of the traversable cells from the seed
        {
            vector<int> obst; for (size_t i = 0; i < nc; i++) if (cls[i] == 4) obst.push_back((int)i);
            bool clear = I.r2 == 4 && !obst.empty(), drivable = true; long long trav = 0, closest = 1ll << 40;
            for (size_t i = 0; i < nc; i++) {
                if (cd.reach[i] == 0) continue;
                trav++; drivable = drivable && cls[i] == 1;
                for (int o : obst) { const long long dx = (long long)(i % nx) - o % nx, dy = (long long)(i / nx) - o / nx, dd = dx * dx + dy * dy; closest = min(closest, dd); clear = clear && dd > I.r2; }
            }
            cout << "the traversable cell closest to an obstacle cell is at d2 = " << closest << " (must exceed r2 = " << I.r2 << ")" << endl;
            CHECK("no_traversable_cell_lies_within_r2_of_an_obstacle_cell", clear && trav == I.traversable && trav > 0);
            vector<uint8_t> seen(nc, 0); vector<int> stack; long long filled = 0;
            if (I.seed_cell >= 0 && cd.reach[(size_t)I.seed_cell]) { seen[(size_t)I.seed_cell] = 1; stack.push_back((int)I.seed_cell); }
            while (!stack.empty()) {
                const int a = stack.back(); stack.pop_back(); filled++;
                const int x = a % nx, y = a / nx, nb[4][2] = {{x - 1, y}, {x + 1, y}, {x, y - 1}, {x, y + 1}};
                for (auto& q : nb) { if (q[0] < 0 || q[1] < 0 || q[0] >= nx || q[1] >= ny) continue; const size_t b = (size_t)q[1] * nx + q[0]; if (!seen[b] && cd.reach[b]) { seen[b] = 1; stack.push_back((int)b); } }
            }
            bool match = filled == I.reachable && filled > 0;
            for (size_t i = 0; i < nc; i++) match = match && (cd.reach[i] == 2) == (seen[i] != 0);
            CHECK("every_reachable_cell_is_drivable_and_connected_to_the_seed", drivable && match);
        }
        // the seed: the last key-frame's camera stands at world (0, 0, STEP (N - 1)), grid (0, STEP (N - 1)); its own cell is unobserved (the lowest pixel row sees
        // the ground from GROUND fy / (H - 1 - cy) = 6.08 m ahead), so the seed snaps to the traversable cell with the smallest (d2, index) within 10 cells
        {
            int32_t cx = -1, cy = -1;
            const bool in = ssm_clrc::cell_of(P, 0.0, STEP * (N - 1), &cx, &cy);
            unsigned long long best = ~0ull;
            for (size_t i = 0; i < nc; i++) {
                if (!cd.reach[i]) continue;
                const long long dx = (long long)(i % nx) - cx, dy = (long long)(i / nx) - cy, dd = dx * dx + dy * dy;
                if (dd <= 100) best = min(best, ((unsigned long long)dd << 24) | i);
            }
            cout << "camera cell " << cx << ", " << cy << " (class " << (in ? (int)cls[(size_t)cy * nx + cx] : -1) << "), seed " << I.seed_cell % nx << ", " << I.seed_cell / nx << " at d2 = " << (best >> 24) << endl;
            CHECK("the_seed_is_the_snapped_cell_of_the_last_keyframes_camera", in && cx == cd.info.seed_cx && cy == cd.info.seed_cy && best != ~0ull && (long long)(best & 0xFFFFFF) == I.seed_cell &&
                  cd.reach[(size_t)I.seed_cell] == 2);
        }
        // TRUTH, derived from the scene.  Grid x is world x, grid y world z; x0 and y0 are multiples of the cell, 0.5 m.  The lane is |x| < 1: the four columns
        // [-1, -0.5) .. [0.5, 1).  The only thing that stands is the box, x 1.5 .. 3, z 9 .. 12; test_objects shows its obstacle cells within one cell of that
        // footprint, so no obstacle cell has a column left of [1, 1.5).  From the two left lane columns, [-1, -0.5) and [-0.5, 0), that is at least 3 columns away:
        // d2 >= 9 > r2 = floor((1.0 / 0.5)^2) = 4, so every DRIVABLE cell of these two columns is traversable.  Camera 0 (z = 0) sees the ground where its pixel
        // rows are at most a cell apart: two neighbouring rows v, v + 1 below the horizon meet the ground at z = GROUND fy / (v - cy), GROUND fy = 480, so the gap
        // 480 / ((v - cy)(v + 1 - cy)) is below 0.5 m for v - cy >= 31, i.e. up to z = 480 / 31 = 15.4 m, and the lowest row (v - cy = 79) starts at 6.08 m: every
        // cell of these columns with 6.5 <= z < 15 holds ground points of the lane, labelled Road, and is DRIVABLE.  They form two unbroken columns, the seed
        // snaps into the lane at its near end (the camera looks along the lane), hence ALL of them must be reachable.  And beside the box the lane's right column
        // [0.5, 1) is at most 2 columns from the box's left face (an obstacle cell in column [1, 1.5) or [1.5, 2)): d2 <= 4, not traversable, for 9.5 <= z < 11.5.
        {
            const int c0 = (int)floor((-1.0 - P.x0) / P.cell), c3 = c0 + 3, r0 = (int)floor((6.5 - P.y0) / P.cell), r1 = (int)floor((15.0 - P.y0) / P.cell), b0 = (int)floor((9.5 - P.y0) / P.cell),
                      b1 = (int)floor((11.5 - P.y0) / P.cell);
            int must = 0, are = 0, shut = 0, rows = 0;
            for (int y = r0; y < r1; y++) for (int x = c0; x < c0 + 2; x++) { must++; are += cd.reach[(size_t)y * nx + x] == 2; }
            for (int y = b0; y < b1; y++) { rows++; shut += cd.reach[(size_t)y * nx + c3] == 0 && cls[(size_t)y * nx + c3] == 1; }
            cout << "lane cells that must be reachable: " << must << ", reachable: " << are << "; cells of the lane's right column beside the box: " << rows << ", drivable and not traversable: " << shut << endl;
            CHECK("the_lane_cells_that_must_be_reachable_are", must == 2 * (r1 - r0) && must > 30 && are == must);
            CHECK("beside_the_box_the_lanes_right_column_is_closed", rows == 4 && shut == rows);
        }

        // the files
        {
            const cv::Mat cm = ssm::imreadPNG(out_dir + "/clearance.png", -1), rm = ssm::imreadPNG(out_dir + "/reach.png", -1);
            bool ok = !cm.empty() && cm.rows == ny && cm.cols == nx && cm.type() == CV_16UC1 && !rm.empty() && rm.rows == ny && rm.cols == nx && rm.type() == CV_8UC1;
            for (int r = 0; ok && r < ny; r++) for (int x = 0; ok && x < nx; x++) {
                const size_t i = (size_t)(ny - 1 - r) * nx + x;
                const double v = cd.d2[i] == UINT32_MAX ? 65535.0 : min(65535.0, floor(sqrt((double)cd.d2[i]) * P.cell * 100.0));
                ok = (double)cm.ptr<uint16_t>(r)[x] == v && (int)rm.ptr<uint8_t>(r)[x] == (cd.reach[i] == 2 ? 255 : cd.reach[i] == 1 ? 128 : 0);
            }
            ifstream txt(out_dir + "/clearance.txt");
            const char* names[8] = {"blocked", "free_cells", "traversable", "components", "reachable", "seed_cell", "max_d2_reachable", "r2"};
            const int64_t want[8] = {I.blocked, I.free_cells, I.traversable, I.components, I.reachable, I.seed_cell, I.max_d2_reachable, I.r2};
            bool read = true; string name; long long v;
            for (int k = 0; k < 8; k++) read = read && (txt >> name >> v) && name == names[k] && v == want[k];
            read = read && !(txt >> name);
            CHECK("the_written_files_read_back_as_the_fetched_arrays", ok && read);
        }

        // a grid built only for the clearance map: the same map, no grid file
        mkdir((out_dir + "/none").c_str(), 0755);
        ng_m.buildGrid(kn);
        CHECK("without_mapper_grid_the_grid_is_built_for_the_clearance_map_and_no_grid_file_is_written", same_clearance(clearance_of(ng_m), cd) && !ng_m.objectsInfo().built && !exists(out_dir + "/none/grid.txt") &&
              !exists(out_dir + "/none/grid_colour.png"));

        // with the objects, carving and alignment on top, key-frame by key-frame as the viewer does it; both routes agree
        adev_m.alignCarveUpTo(kad); ahost_m.alignCarveUpTo(kah);
        adev_m.buildGrid(kad); ahost_m.buildGrid(kah);
        const Clearance ad = clearance_of(adev_m), ah = clearance_of(ahost_m);
        cout << "with mapper_objects=1, mapper_carve=1 and mapper_align=1: " << ad.info.counts.traversable << " traversable, " << ad.info.counts.reachable << " reachable" << endl;
        CHECK("with_objects_carving_and_alignment_both_routes_agree", same_clearance(ad, ah) && ad.info.counts.reachable > 0 && adev_m.objectsInfo().built && ahost_m.objectsInfo().built &&
              adev_m.carvedViews() == (int)n - 1 && adev_m.alignedKeyframes() == (int)n);

        // a Mapper whose viewer runs makes the same map as it ends; and the map it publishes is, byte for byte, the map of a Mapper with the switch off
        {
            auto viewer = [&](const ParameterReader& p, Clearance* found) {
                PoseGraph g(para, tracker);
                g.keyframes = load();
                Mapper m(p, g);
                for (int t = 0; t < 20000 && m.updates() < 1 && !m.viewerFailed; t++) this_thread::sleep_for(chrono::milliseconds(1));
                m.shutdown();
                if (m.viewerFailed || m.deviceMapFellBack) throw runtime_error("the viewer failed");
                if (found) *found = clearance_of(m);
                Mapper::PointCloud::Ptr map = m.getGlobalMap();
                vector<ssm_point> pts;
                if (map) for (const auto& q : map->points) pts.push_back(*reinterpret_cast<const ssm_point*>(&q));
                return pts;
            };
            Clearance found;
            const vector<ssm_point> map_on = viewer(on, &found), map_off = viewer(grid_only, nullptr), map_plain = viewer(para, nullptr);
            CHECK("the_viewer_maps_the_clearance_as_it_ends", same_clearance(found, cd));
            CHECK("switch_off_the_published_map_as_before", map_on.size() > 1000 && same(map_on, map_off) && same(map_on, map_plain));
        }
    } catch (const exception& e) { cout << "FAIL exception " << e.what() << endl; fails++; }
    cout << (fails ? "FAILED" : "ALL PASSED") << endl;
    return fails;
}
