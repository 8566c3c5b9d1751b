// test_route -- the route field through Mapper on the device (run by tests/test_gpu_route_host.py under -m gpu).  The scene is the shared lane scene as it is
// (test_lane_scene.h), set up as test_clearance.cpp does: 0.5 m cells, ground_radius 3, every depth image ray-cast from the key-frame's TRUE pose.
// mapper_route=0 leaves everything as it was -- clouds, grid, objects, clearance map, the published map, no route; with 1 the device route and the host route to the
// clouds give the same bytes, which are those of ssm_route_cells_host and ssm_route_path_host on the fetched reach and dist2 from the clearance call's seed; every
// reachable cell is routed or counted unrouted; the path to the lane's far end passes the box where geometry says it must (derived below); the three files read
// back as the fetched arrays; a grid and a clearance map built only for the route write no file of their own; with objects, carving and alignment on top both
// routes still agree; and a Mapper whose viewer thread runs makes the same field as it ends.  Prints one "PASS name" / "FAIL name" line per check; exit code = failures.
#include "test_lane_scene.h"
#include <sys/stat.h>
struct Route { ssm_grid_params P{}; Mapper::RouteInfo info; vector<uint32_t> cost; vector<int32_t> parent, path; };
static Route route_of(const Mapper& m) { Route r; r.P = m.gridParams(); r.info = m.routeInfo(); m.routeFetch(&r.cost, &r.parent); r.path = m.routePath(); return r; }
static bool same_route(const Route& a, const Route& b)
{
    return a.info.built && b.info.built && memcmp(&a.P, &b.P, sizeof a.P) == 0 && memcmp(&a.info.counts, &b.info.counts, sizeof a.info.counts) == 0 &&
           memcmp(&a.info.path, &b.info.path, sizeof a.info.path) == 0 && a.info.goal_cx == b.info.goal_cx && a.info.goal_cy == b.info.goal_cy && a.cost == b.cost && a.parent == b.parent && a.path == b.path;
}
static bool exists(const string& path) { struct stat st; return stat(path.c_str(), &st) == 0; }
static const double GOAL_X = -0.25, GOAL_Y = 14.75, COMFORT = 1.5;          // the far end of the lane's second column from the left, in the grid frame

int main(int argc, char** argv)
{
    if (argc < 3) { cerr << "usage: test_route <parameters> <output directory>" << endl; return 2; }
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
        ParameterReader base = para; base.set("mapper_grid", "1"); base.set("mapper_grid_cell", "0.5"); base.set("mapper_grid_ground_radius", "3"); base.set("mapper_objects", "1");
        base.set("mapper_clearance", "1");
        ParameterReader on = base; on.set("mapper_route", "1"); on.set("mapper_route_comfort", to_string(COMFORT)); on.set("mapper_route_goal_x", to_string(GOAL_X));
        on.set("mapper_route_goal_y", to_string(GOAL_Y)); on.set("mapper_route_goal_snap", "0");
        ParameterReader on_files = on; on_files.set("mapper_route_dir", out_dir);          // (the device route writes the files)
        ParameterReader on_host = on; on_host.set("mapper_device_map", "0");
        ParameterReader all_on = on; all_on.set("mapper_carve", "1"); all_on.set("mapper_align", "1");
        ParameterReader all_host = all_on; all_host.set("mapper_device_map", "0");
        ParameterReader alone = on; alone.set("mapper_grid", "0"); alone.set("mapper_objects", "0"); alone.set("mapper_clearance", "0"); alone.set("mapper_grid_dir", out_dir + "/none");
        alone.set("mapper_clearance_dir", out_dir + "/none");
        ParameterReader no_goal = base; no_goal.set("mapper_route", "1"); no_goal.set("mapper_route_comfort", to_string(COMFORT));
        QuietMapper off_m(base, pg), dev_m(on_files, pg), host_m(on_host, pg), adev_m(all_on, pg), ahost_m(all_host, pg), al_m(alone, pg), far_m(no_goal, pg);
        CHECK("switch_defaults_to_off", !off_m.mapsRoute() && dev_m.mapsRoute() && host_m.mapsRoute() && !off_m.routeInfo().built && !dev_m.routeInfo().built);
        vector<RGBDFrame::Ptr> k0 = load(), kd = load(), kh = load(), kad = load(), kah = load(), kn = load(), kf = load();
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

        // switch off: the grid, the objects, the clearance map and the clouds are what they are with the switch on, there is no route
        off_m.buildGrid(k0); dev_m.buildGrid(kd); host_m.buildGrid(kh);
        vector<uint32_t> d2; vector<uint8_t> reach;
        {
            vector<uint8_t> a[3], b[3]; vector<int32_t> aq[2], bq[2]; vector<uint32_t> an[2], bn[2]; vector<ssm_object> ra, rb; vector<int32_t> ia_, ib_; vector<uint32_t> none;
            off_m.gridFetch(&a[0], &a[1], &a[2], &aq[0], &aq[1], &an[0], &an[1]); dev_m.gridFetch(&b[0], &b[1], &b[2], &bq[0], &bq[1], &bn[0], &bn[1]);
            off_m.objectsFetch(&ra, &ia_); dev_m.objectsFetch(&rb, &ib_);
            vector<uint32_t> ca; vector<int32_t> na, nb; vector<uint8_t> rca;
            off_m.clearanceFetch(&ca, &na, &rca); dev_m.clearanceFetch(&d2, &nb, &reach);
            const ssm_grid_params pa = off_m.gridParams(), pb = dev_m.gridParams(); const ssm_grid_info ia = off_m.gridInfo().counts, ib = dev_m.gridInfo().counts;
            const ssm_objects_info oa = off_m.objectsInfo().counts, ob = dev_m.objectsInfo().counts; const ssm_clearance_info qa = off_m.clearanceInfo().counts, qb = dev_m.clearanceInfo().counts;
            bool same_clouds = true;
            for (size_t j = 0; j < n; j++) same_clouds = same_clouds && same(off_m.cloudNow(k0[j]), plain[j]) && same(dev_m.cloudNow(kd[j]), plain[j]) && same(host_m.cloudNow(kh[j]), plain[j]);
            CHECK("switch_off_grid_objects_clearance_and_clouds_as_before_and_no_route", off_m.gridInfo().built && memcmp(&pa, &pb, sizeof pa) == 0 && memcmp(&ia, &ib, sizeof ia) == 0 && a[0] == b[0] &&
                  a[1] == b[1] && a[2] == b[2] && aq[0] == bq[0] && aq[1] == bq[1] && an[0] == bn[0] && an[1] == bn[1] && same_clouds && memcmp(&oa, &ob, sizeof oa) == 0 && ra.size() == rb.size() &&
                  ra.size() == 1 && memcmp(ra.data(), rb.data(), sizeof(ssm_object)) == 0 && ia_ == ib_ && off_m.clearanceInfo().built && memcmp(&qa, &qb, sizeof qa) == 0 && ca == d2 && na == nb &&
                  rca == reach && !off_m.routeInfo().built && !off_m.routeFetch(&none, nullptr) && none.empty() && off_m.routePath().empty());
        }

        // the two routes, and the host functions on the fetched clearance images
        const Route rd = route_of(dev_m), rh = route_of(host_m);
        CHECK("routes_give_the_same_bytes", same_route(rd, rh));
        const ssm_grid_params P = rd.P;
        const int nx = P.nx, ny = P.ny;
        const size_t nc = (size_t)nx * ny;
        const ssm_route_info I = rd.info.counts; const ssm_route_path_info PI = rd.info.path;
        const ssm_clearance_info CI = dev_m.clearanceInfo().counts;
        ssm_route_params R; ssm_route_params_default(&R); R.comfort = COMFORT; R.cell = P.cell;
        int32_t gx = -1, gy = -1;
        const bool goal_in = ssm_clrc::cell_of(P, GOAL_X, GOAL_Y, &gx, &gy);
        {
            Route g; g.P = P; g.info = rd.info; g.cost.resize(nc); g.parent.resize(nc); g.path.assign((size_t)(4 * (nx + ny)), -1);
            if (ssm_route_cells_host(reach.data(), d2.data(), nx, ny, (int)CI.seed_cell, &R, g.cost.data(), g.parent.data(), &g.info.counts) != SSM_OK) throw runtime_error("ssm_route_cells_host failed");
            if (ssm_route_path_host(g.cost.data(), g.parent.data(), d2.data(), nx, ny, &R, gx, gy, 0, (int)g.path.size(), g.path.data(), &g.info.path) != SSM_OK) throw runtime_error("ssm_route_path_host failed");
            g.path.resize((size_t)g.info.path.len);
            CHECK("the_field_and_the_path_are_the_host_functions_on_the_fetched_clearance_map", reach.size() == nc && goal_in && gx == rd.info.goal_cx && gy == rd.info.goal_cy && same_route(rd, g));
        }
        cout << "route: " << nx << " x " << ny << " cells of " << P.cell << " m, comfort2 " << I.comfort2 << ", " << I.routed << " routed, " << I.unrouted << " unrouted, " << I.near_cells
             << " near, max cost " << I.max_cost << " at cell " << I.far_cell % nx << ", " << I.far_cell / nx << ", source " << I.source_cell % nx << ", " << I.source_cell / nx << "; path to " << gx << ", "
             << gy << ": " << PI.len << " cells, cost " << PI.cost << ", " << PI.n_axial << " axial, " << PI.n_diag << " diagonal, " << PI.near_steps << " near, min d2 " << PI.min_d2 << endl;
        // every reachable cell is routed or counted: the scene's 286
        {
            long long routed = 0, reachable = 0;
            for (size_t i = 0; i < nc; i++) { reachable += reach[i] == 2; routed += rd.cost[i] != UINT32_MAX; if (rd.cost[i] != UINT32_MAX && reach[i] != 2) routed = -(1ll << 40); }
            CHECK("all_286_reachable_cells_are_routed_or_counted_unrouted", CI.reachable == 286 && reachable == 286 && I.routed + I.unrouted == 286 && routed == I.routed && I.source_cell == CI.seed_cell &&
                  I.comfort2 == 9 && I.moves == 8);
        }
        // TRUTH, derived from the scene before looking (test_clearance.cpp derives the map underneath: x0 and y0 are multiples of the 0.5 m cell, the lane's four
        // columns are [-1, -0.5) .. [0.5, 1), the seed snaps to (80, 92), the two left lane columns are reachable for 6.5 <= z < 15, and beside the box, 9.5 <= z <
        // 11.5, the right column is closed).  The goal (-0.25, 14.75) is a cell of the second column from the left inside that reachable stretch, and the clearance map
        // is 4-connected, so a way of axial moves leads there: the goal is ROUTED and the path ends on it.  Beside the box the box's left face puts an obstacle cell
        // into column [1, 1.5) or [1.5, 2).  (a) The closed right column is on no path.  (b) The third column, [0, 0.5), is 2 or 3 columns from that obstacle: d2 <= 9
        // = comfort2 = floor((1.5 / 0.5)^2), NEAR, weight 3; the leftmost column is 4 or 5 away, d2 >= 16, never NEAR.  A cell of the third column beside the box
        // costs its two edges at least 2 . 5 . 2 = 20 more than a cell that is not NEAR, while moving over to the leftmost column and back costs at most four
        // diagonals in place of axial steps, 4 . 4 = 16: so beside the box the cheapest path keeps to the lane's two LEFT columns.  (c) No path is cheaper than the
        // chamfer distance of the straight line, 10 max + 4 min, since every edge costs at least its step times 2.
        {
            const int c0 = (int)floor((-1.0 - P.x0) / P.cell), c3 = c0 + 3, b0 = (int)floor((9.5 - P.y0) / P.cell), b1 = (int)floor((11.5 - P.y0) / P.cell);
            const int sx = (int)(I.source_cell % nx), sy = (int)(I.source_cell / nx), dx = abs(gx - sx), dy = abs(gy - sy);
            int beside = 0, left = 0, closed = 0;
            for (int32_t c : rd.path) {
                const int x = c % nx, y = c / nx;
                if (y < b0 || y >= b1) continue;
                beside++; left += x == c0 || x == c0 + 1; closed += x == c3;
            }
            cout << "DERIVED: source 80, 92; the goal routed; beside the box (rows " << b0 << " .. " << b1 - 1 << ") every path cell in columns " << c0 << " or " << c0 + 1 << ", none in column " << c3
                 << "; cost >= " << 10 * max(dx, dy) + 4 * min(dx, dy) << ".  OBSERVED: source " << sx << ", " << sy << "; goal cell " << PI.goal_cell % nx << ", " << PI.goal_cell / nx << "; " << beside
                 << " path cells beside the box, " << left << " in the two left columns, " << closed << " in the closed column; cost " << PI.cost << endl;
            CHECK("the_path_starts_at_the_snapped_seed_and_ends_on_the_goal", sx == 80 && sy == 92 && PI.goal_cell == (int64_t)gy * nx + gx && PI.len == (int64_t)rd.path.size() && PI.len > 1 &&
                  rd.path.front() == (int32_t)I.source_cell && rd.path.back() == (int32_t)PI.goal_cell && PI.n_axial + PI.n_diag == PI.len - 1);
            CHECK("the_path_passes_the_box_through_the_lanes_two_left_columns", beside >= b1 - b0 && b1 - b0 == 4 && left == beside);
            CHECK("the_path_holds_none_of_the_closed_cells_beside_the_box", closed == 0);
            CHECK("the_path_costs_at_least_the_chamfer_cost_of_the_straight_line", PI.cost >= 10 * max(dx, dy) + 4 * min(dx, dy) && PI.cost == (int64_t)rd.cost[(size_t)PI.goal_cell]);
        }

        // the files
        {
            const cv::Mat rm = ssm::imreadPNG(out_dir + "/route.png", -1), cm = ssm::imreadPNG(out_dir + "/route_cost.png", -1);
            bool ok = !cm.empty() && cm.rows == ny && cm.cols == nx && cm.type() == CV_16UC1 && !rm.empty() && rm.rows == ny && rm.cols == nx && rm.type() == CV_8UC1;
            vector<uint8_t> on_path(nc, 0); for (int32_t c : rd.path) on_path[(size_t)c] = 1;
            for (int r = 0; ok && r < ny; r++) for (int x = 0; ok && x < nx; x++) {
                const size_t i = (size_t)(ny - 1 - r) * nx + x;
                ok = (uint32_t)cm.ptr<uint16_t>(r)[x] == (rd.cost[i] == UINT32_MAX ? 65535u : min<uint32_t>(65534u, rd.cost[i])) &&
                     (int)rm.ptr<uint8_t>(r)[x] == (on_path[i] ? 64 : reach[i] == 2 ? 255 : reach[i] == 1 ? 128 : 0);
            }
            ifstream txt(out_dir + "/route.txt");
            const char* names[15] = {"routed", "unrouted", "near_cells", "max_cost", "far_cell", "source_cell", "comfort2", "moves", "len", "goal_cell", "cost", "n_axial", "n_diag", "near_steps", "min_d2"};
            const int64_t want[15] = {I.routed, I.unrouted, I.near_cells, I.max_cost, I.far_cell, I.source_cell, I.comfort2, I.moves, PI.len, PI.goal_cell, PI.cost, PI.n_axial, PI.n_diag, PI.near_steps, PI.min_d2};
            bool read = true; string name; long long v, x, y;
            for (int k = 0; k < 15; k++) read = read && (txt >> name >> v) && name == names[k] && v == want[k];
            for (int32_t c : rd.path) read = read && (txt >> x >> y) && x == c % nx && y == c / nx;
            read = read && !(txt >> name);
            CHECK("the_written_files_read_back_as_the_fetched_arrays", ok && read);
        }

        // a grid and a clearance map built only for the route: the same field, no grid file, no clearance file
        mkdir((out_dir + "/none").c_str(), 0755);
        al_m.buildGrid(kn);
        CHECK("without_grid_and_clearance_both_are_built_for_the_route_and_write_no_file", same_route(route_of(al_m), rd) && !al_m.objectsInfo().built && !exists(out_dir + "/none/grid.txt") &&
              !exists(out_dir + "/none/clearance.txt") && !exists(out_dir + "/none/reach.png"));
        // without a goal the path leads to far_cell, the farthest place the vehicle can drive to
        far_m.buildGrid(kf);
        {
            const Route rf = route_of(far_m);
            CHECK("without_a_goal_the_path_leads_to_the_farthest_cell", rf.info.built && rf.cost == rd.cost && rf.parent == rd.parent && rf.info.path.goal_cell == I.far_cell && rf.info.path.cost == I.max_cost &&
                  !rf.path.empty() && rf.path.back() == (int32_t)I.far_cell && rf.info.goal_cx == (int32_t)(I.far_cell % nx) && rf.info.goal_cy == (int32_t)(I.far_cell / nx));
        }

        // with the objects, carving and alignment on top, key-frame by key-frame as the viewer does it; both routes agree
        adev_m.alignCarveUpTo(kad); ahost_m.alignCarveUpTo(kah);
        adev_m.buildGrid(kad); ahost_m.buildGrid(kah);
        const Route ad = route_of(adev_m), ah = route_of(ahost_m);
        cout << "with mapper_objects=1, mapper_carve=1 and mapper_align=1: " << ad.info.counts.routed << " routed, path of " << ad.info.path.len << " cells" << endl;
        CHECK("with_objects_carving_and_alignment_both_routes_agree", same_route(ad, ah) && ad.info.counts.routed > 0 && adev_m.objectsInfo().built && ahost_m.objectsInfo().built &&
              adev_m.carvedViews() == (int)n - 1 && adev_m.alignedKeyframes() == (int)n);

        // a Mapper whose viewer runs makes the same field as it ends; and the map it publishes is, byte for byte, the map of a Mapper with the switch off
        {
            auto viewer = [&](const ParameterReader& p, Route* found) {
                PoseGraph g(para, tracker);
                g.keyframes = load();
                Mapper m(p, g);
                for (int t = 0; t < 20000 && m.updates() < 1 && !m.viewerFailed; t++) this_thread::sleep_for(chrono::milliseconds(1));
                m.shutdown();
                if (m.viewerFailed || m.deviceMapFellBack) throw runtime_error("the viewer failed");
                if (found) *found = route_of(m);
                Mapper::PointCloud::Ptr map = m.getGlobalMap();
                vector<ssm_point> pts;
                if (map) for (const auto& q : map->points) pts.push_back(*reinterpret_cast<const ssm_point*>(&q));
                return pts;
            };
            Route found;
            const vector<ssm_point> map_on = viewer(on, &found), map_off = viewer(base, nullptr), map_plain = viewer(para, nullptr);
            CHECK("the_viewer_routes_as_it_ends", same_route(found, rd));
            CHECK("switch_off_the_published_map_as_before", map_on.size() > 1000 && same(map_on, map_off) && same(map_on, map_plain));
        }
    } catch (const exception& e) { cout << "FAIL exception " << e.what() << endl; fails++; }
    cout << (fails ? "FAILED" : "ALL PASSED") << endl;
    return fails;
}
