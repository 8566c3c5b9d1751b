// test_objects -- object extraction through Mapper on the device (run by tests/test_gpu_objects_host.py under -m gpu).  The scene is the shared lane scene as it is
// (test_lane_scene.h): the lane Road, the sides Pavement, the box Car; every depth image is ray-cast from the key-frame's TRUE pose, which the Mapper gets.
// mapper_objects=0 leaves everything as it was -- clouds, grid, the published map, no objects; with 1 the device route (deviceCloud + ssm_objects_clouds) and the host route
// (frame->pointcloud + ssm_objects_points) give the same bytes, which are those of ssm_objects_host on the fetched clouds; exactly one object, a Vehicle, is found;
// its cell box lies within one cell of the box's true footprint; its refined box lies inside the true box widened by a bound derived below from the depth unit,
// float32 and the 2^-10 m quantisation; every one of its points is labelled Vehicle; objects.txt and objects_id.png read back as objectsFetch; with mapper_carve=1
// and mapper_align=1 on top both routes still agree; a Mapper whose viewer thread runs finds the same object as it ends; and with mapper_grid=0 the grid is built
// for the objects but no grid file is written.  The grid uses 0.5 m cells and ground_radius 3 as test_grid.cpp does.
// Prints one "PASS name" / "FAIL name" line per check; exit code = failures.
#include "test_lane_scene.h"
#include <sys/stat.h>
struct Objects { ssm_grid_params P{}; Mapper::ObjectsInfo info; vector<ssm_object> rec; vector<int32_t> oid; };
static Objects objects_of(const Mapper& m) { Objects o; o.P = m.gridParams(); o.info = m.objectsInfo(); m.objectsFetch(&o.rec, &o.oid); return o; }
static bool same_objects(const Objects& a, const Objects& b)
{
    return a.info.built && b.info.built && memcmp(&a.P, &b.P, sizeof a.P) == 0 && memcmp(&a.info.counts, &b.info.counts, sizeof a.info.counts) == 0 && a.rec.size() == b.rec.size() &&
           (a.rec.empty() || memcmp(a.rec.data(), b.rec.data(), a.rec.size() * sizeof(ssm_object)) == 0) && a.oid == b.oid;
}
static bool exists(const string& path) { struct stat st; return stat(path.c_str(), &st) == 0; }

int main(int argc, char** argv)
{
    if (argc < 3) { cerr << "usage: test_objects <parameters> <output directory>" << endl; return 2; }
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
        ParameterReader grid_only = para; grid_only.set("mapper_grid", "1"); grid_only.set("mapper_grid_cell", "0.5"); grid_only.set("mapper_grid_ground_radius", "3");
        ParameterReader on = grid_only; on.set("mapper_objects", "1");
        ParameterReader on_files = on; on_files.set("mapper_objects_dir", out_dir);          // (the device route writes the files)
        ParameterReader on_host = on; on_host.set("mapper_device_map", "0");
        ParameterReader all_on = on; all_on.set("mapper_carve", "1"); all_on.set("mapper_align", "1");
        ParameterReader all_host = all_on; all_host.set("mapper_device_map", "0");
        ParameterReader no_grid = on; no_grid.set("mapper_grid", "0"); no_grid.set("mapper_grid_dir", out_dir + "/none");
        QuietMapper off_m(grid_only, pg), dev_m(on_files, pg), host_m(on_host, pg), adev_m(all_on, pg), ahost_m(all_host, pg), ng_m(no_grid, pg);
        CHECK("switch_defaults_to_off", !off_m.extractsObjects() && dev_m.extractsObjects() && host_m.extractsObjects() && !off_m.objectsInfo().built && !dev_m.objectsInfo().built);
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

        // switch off: the grid is what it is with the switch on, there are no objects
        off_m.buildGrid(k0); dev_m.buildGrid(kd); host_m.buildGrid(kh);
        {
            vector<uint8_t> a[3], b[3]; vector<int32_t> aq[2], bq[2]; vector<uint32_t> an[2], bn[2]; vector<ssm_object> none; vector<int32_t> none_id;
            off_m.gridFetch(&a[0], &a[1], &a[2], &aq[0], &aq[1], &an[0], &an[1]); dev_m.gridFetch(&b[0], &b[1], &b[2], &bq[0], &bq[1], &bn[0], &bn[1]);
            const ssm_grid_params pa = off_m.gridParams(), pb = dev_m.gridParams(); const ssm_grid_info ia = off_m.gridInfo().counts, ib = dev_m.gridInfo().counts;
            bool same_clouds = true;
            for (size_t j = 0; j < n; j++) same_clouds = same_clouds && same(off_m.cloudNow(k0[j]), plain[j]) && same(dev_m.cloudNow(kd[j]), plain[j]) && same(host_m.cloudNow(kh[j]), plain[j]);
            CHECK("switch_off_grid_and_clouds_as_before_and_no_objects", off_m.gridInfo().built && memcmp(&pa, &pb, sizeof pa) == 0 && memcmp(&ia, &ib, sizeof ia) == 0 && a[0] == b[0] && a[1] == b[1] &&
                  a[2] == b[2] && aq[0] == bq[0] && aq[1] == bq[1] && an[0] == bn[0] && an[1] == bn[1] && same_clouds && !off_m.objectsInfo().built && !off_m.objectsFetch(&none, &none_id) && none.empty());
        }

        // the two routes, and the host function on the fetched clouds
        const Objects od = objects_of(dev_m), oh = objects_of(host_m);
        CHECK("routes_give_the_same_bytes", same_objects(od, oh));
        const ssm_grid_params P = od.P;
        const size_t nc = (size_t)P.nx * P.ny;
        {
            Objects g; g.P = P; g.info.built = true; g.rec.resize(nc); g.oid.resize(nc); int K = 0;
            vector<const ssm_point*> pts; vector<int32_t> cnt; vector<double> poses;
            for (size_t i = 0; i < n; i++) { pts.push_back(plain[i].data()); cnt.push_back((int32_t)plain[i].size()); const Eigen::Isometry3d T = k0[i]->getTransform(); poses.insert(poses.end(), T.data(), T.data() + 16); }
            ssm_objects_params OP; ssm_objects_params_default(&OP);
            if (ssm_objects_host(pts.data(), cnt.data(), poses.data(), (int)n, &P, &OP, g.rec.data(), (int)nc, &K, g.oid.data(), nullptr, &g.info.counts) != SSM_OK) throw runtime_error("ssm_objects_host failed");
            g.rec.resize((size_t)K);
            CHECK("the_objects_are_the_host_function_on_the_fetched_clouds", same_objects(od, g));
        }
        const ssm_objects_info I = od.info.counts;
        cout << "objects: " << I.member_cells << " member cells, " << I.components << " components, " << I.kept << " kept (" << I.rejected_cells << " / " << I.rejected_points << " / "
             << I.rejected_height << " rejected by cells / points / height), " << I.object_points << " of " << I.n_in << " points" << endl;
        CHECK("exactly_one_object_and_it_is_a_vehicle", od.rec.size() == 1 && od.rec[0].label == 9 && I.kept == 1);
        if (od.rec.size() == 1) {
            const ssm_object& o = od.rec[0];
            // the cells the true footprint touches (grid x = world x, grid y = world z)
            const int bx0 = (int)floor((BOX_LO[0] - P.x0) / P.cell), bx1 = (int)ceil((BOX_HI[0] - P.x0) / P.cell) - 1, by0 = (int)floor((BOX_LO[2] - P.y0) / P.cell),
                      by1 = (int)ceil((BOX_HI[2] - P.y0) / P.cell) - 1;
            cout << "cell box: x " << o.cx_min << " .. " << o.cx_max << " (footprint " << bx0 << " .. " << bx1 << "), y " << o.cy_min << " .. " << o.cy_max << " (footprint " << by0 << " .. " << by1 << "), "
                 << o.cells << " cells" << endl;
            CHECK("the_cell_box_lies_within_one_cell_of_the_true_footprint", abs(o.cx_min - bx0) <= 1 && abs(o.cx_max - bx1) <= 1 && abs(o.cy_min - by0) <= 1 && abs(o.cy_max - by1) <= 1);
            // The bound, in units of 2^-10 m.  A box pixel's depth is rounded to 1 / scale m: half a depth unit at most along z, and that times the pixel's tangent
            // along x and y (|tan_x| <= max(cx, W - 1 - cx) / fx, |tan_y| <= max(cy, H - 1 - cy) / fy).  The point's float32 coordinates (|c| < 16 m: 2^-24 relative,
            // 2^-20 m) and the back-projection's float32 products stay below 0.01 unit; the true poses are translations by multiples of 0.5 m, exact in a double.
            // Rounding to a unit adds 0.5.
            const double half = 1024.0 * 0.5 / camera.scale, tx = max(camera.cx, W - 1 - camera.cx) / camera.fx, ty = max(camera.cy, H - 1 - camera.cy) / camera.fy;
            const double bound_x = half * tx + 0.5 + 0.01, bound_y = half + 0.5 + 0.01, bound_z = half * ty + 0.5 + 0.01;          // grid x, grid y (depth), height
            const double lo[3] = {BOX_LO[0] * 1024.0, BOX_LO[2] * 1024.0, -BOX_HI[1] * 1024.0}, hi[3] = {BOX_HI[0] * 1024.0, BOX_HI[2] * 1024.0, -BOX_LO[1] * 1024.0};          // height = -y
            const double got_lo[3] = {(double)o.x_min_q, (double)o.y_min_q, (double)o.z_min_q}, got_hi[3] = {(double)o.x_max_q, (double)o.y_max_q, (double)o.z_max_q};
            const double bound[3] = {bound_x, bound_y, bound_z};
            bool inside = true; double slack = -1e30;
            for (int a = 0; a < 3; a++) {
                inside = inside && got_lo[a] >= lo[a] - bound[a] && got_hi[a] <= hi[a] + bound[a] && got_lo[a] <= got_hi[a];
                slack = max(slack, max(lo[a] - got_lo[a], got_hi[a] - hi[a]));
            }
            cout << "refined box (units of 2^-10 m): x " << o.x_min_q << " .. " << o.x_max_q << ", y " << o.y_min_q << " .. " << o.y_max_q << ", height " << o.z_min_q << " .. " << o.z_max_q
                 << "; bounds " << bound_x << " / " << bound_y << " / " << bound_z << "; largest excursion beyond the true box " << slack << " units" << endl;
            CHECK("the_refined_box_lies_inside_the_true_box_widened_by_the_derived_bound", inside);
            CHECK("every_object_point_is_labelled_vehicle_and_is_a_high_point_of_its_cells", o.n_label == o.n_points && o.n_points == o.cell_points && o.n_points > 1000 && (int64_t)o.n_points == I.object_points);
            const double cxm = (double)o.sum_x / o.n_points, cym = (double)o.sum_y / o.n_points;
            CHECK("the_centroid_lies_in_the_refined_box", cxm >= o.x_min_q && cxm <= o.x_max_q && cym >= o.y_min_q && cym <= o.y_max_q);
        }

        // the files
        {
            const cv::Mat img = ssm::imreadPNG(out_dir + "/objects_id.png", -1);
            bool ok = !img.empty() && img.rows == P.ny && img.cols == P.nx && img.type() == CV_16UC1;
            for (int r = 0; ok && r < P.ny; r++) for (int x = 0; ok && x < P.nx; x++) ok = (int)img.ptr<uint16_t>(r)[x] == od.oid[(size_t)(P.ny - 1 - r) * P.nx + x] + 1;
            ifstream txt(out_dir + "/objects.txt");
            size_t lines = 0; bool read = true; int id; string name; unsigned cells, points; double v[11];
            while (txt >> id >> name >> cells >> points) {
                for (double& x : v) read = read && bool(txt >> x);
                read = read && lines < od.rec.size();
                if (!read) break;
                const ssm_object& o = od.rec[lines];
                read = id == (int)lines && name == "Vehicle" && cells == o.cells && points == o.n_points && v[0] == o.x_min_q / 1024.0 && v[1] == o.x_max_q / 1024.0 && v[2] == o.y_min_q / 1024.0 &&
                       v[3] == o.y_max_q / 1024.0 && v[4] == o.z_min_q / 1024.0 && v[5] == o.z_max_q / 1024.0 && v[6] == (double)o.sum_x / o.n_points / 1024.0 &&
                       v[7] == (double)o.sum_y / o.n_points / 1024.0 && v[8] == (double)o.sum_z / o.n_points / 1024.0 && v[9] == o.ground_q / 1024.0 &&
                       v[10] == o.top_q / 1024.0;
                lines++;
            }
            CHECK("the_written_files_read_back_as_the_fetched_records_and_image", ok && read && lines == od.rec.size());
        }

        // a grid built only for the objects: the same objects, no grid file
        mkdir((out_dir + "/none").c_str(), 0755);
        ng_m.buildGrid(kn);
        CHECK("without_mapper_grid_the_grid_is_built_for_the_objects_and_no_grid_file_is_written", same_objects(objects_of(ng_m), od) && !exists(out_dir + "/none/grid.txt") &&
              !exists(out_dir + "/none/grid_colour.png"));

        // with carving and alignment on top, key-frame by key-frame as the viewer does it; both routes agree
        adev_m.alignCarveUpTo(kad); ahost_m.alignCarveUpTo(kah);
        adev_m.buildGrid(kad); ahost_m.buildGrid(kah);
        const Objects ad = objects_of(adev_m), ah = objects_of(ahost_m);
        cout << "with mapper_carve=1 and mapper_align=1: " << ad.rec.size() << " object(s), " << ad.info.counts.object_points << " points" << endl;
        CHECK("with_carving_and_alignment_both_routes_agree", same_objects(ad, ah) && ad.rec.size() >= 1 && ad.rec[0].label == 9 && adev_m.carvedViews() == (int)n - 1 && adev_m.alignedKeyframes() == (int)n);

        // a Mapper whose viewer runs finds the same object as it ends; and the map it publishes is, byte for byte, the map of a Mapper with the switch off (all
        // eight key-frames are there before the thread starts, so both make the same one update: a rebuild)
        {
            auto viewer = [&](const ParameterReader& p, Objects* found) {
                PoseGraph g(para, tracker);
                g.keyframes = load();
                Mapper m(p, g);
                for (int t = 0; t < 20000 && m.updates() < 1 && !m.viewerFailed; t++) this_thread::sleep_for(chrono::milliseconds(1));
                m.shutdown();
                if (m.viewerFailed || m.deviceMapFellBack) throw runtime_error("the viewer failed");
                if (found) *found = objects_of(m);
                Mapper::PointCloud::Ptr map = m.getGlobalMap();
                vector<ssm_point> pts;
                if (map) for (const auto& q : map->points) pts.push_back(*reinterpret_cast<const ssm_point*>(&q));
                return pts;
            };
            Objects found;
            const vector<ssm_point> map_on = viewer(on, &found), map_off = viewer(grid_only, nullptr), map_plain = viewer(para, nullptr);
            CHECK("the_viewer_extracts_the_objects_as_it_ends", same_objects(found, od));
            CHECK("switch_off_the_published_map_as_before", map_on.size() > 1000 && same(map_on, map_off) && same(map_on, map_plain));
        }
    } catch (const exception& e) { cout << "FAIL exception " << e.what() << endl; fails++; }
    cout << (fails ? "FAILED" : "ALL PASSED") << endl;
    return fails;
}
