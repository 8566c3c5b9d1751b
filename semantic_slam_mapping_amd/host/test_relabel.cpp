// test_relabel -- label fusion through Mapper on the device (run by tests/test_gpu_relabel_host.py under -m gpu).  The scene is the analytic KITTI-layout scene of
// test_grid.cpp: a camera 1.6 m above a ground plane drives forward half a metre per key-frame past a box beside the lane; every depth image is ray-cast from the
// key-frame's TRUE pose, which is also the pose the Mapper gets; lane Road, sides Pavement, box Car.  Label noise is planted where its effect can be derived:
// key-frame 3's semantic image has a band of columns on the left painted Tree and a band painted a colour outside the palette, key-frame 5 the same on the right;
// straight motion keeps the two corrupted regions of the scene apart.  Truth is the label of what the point's own ray met.  mapper_relabel=0 leaves everything as it
// was; with 1 the device route (deviceCloud + ssm_relabel) and the host route (frame->pointcloud + ssm_relabel_points) give the same bytes, those of ssm_relabel_host
// replayed cloud after cloud; every band point of clouds 3 and 5 with at least two voting views ends with its true label; no point that carried its true label
// loses it; wrong + unknown labels fall strictly.  With mapper_render=1 the views other than 3 and 5 keep every geometric count, label_disagree does not rise and
// label_agree rises strictly.  With mapper_grid=1 Tree ground labels fall, to none where no Tree point is left.  The published map after the final rebuild holds no Tree.  Carving and alignment on top: both routes agree.
// Prints one "PASS name" / "FAIL name" line per check; exit code = failures.
#include "test_lane_scene.h"


static const int TREE = 6, BAND[2][4] = {{20, 60, 70, 100}, {300, 340, 350, 380}};          // per corrupted key-frame: Tree columns [a, b), unknown columns [c, d)
static int corrupted(int j) { return j == 3 ? 0 : j == 5 ? 1 : -1; }
static uint32_t truth_of(int hit) { return hit == HIT_ROAD ? 4u : hit == HIT_PAVEMENT ? 5u : hit == HIT_BOX ? 9u : 255u; }
struct Seq { vector<RGBDFrame::Ptr> kfs; vector<vector<uint8_t>> hit; };

int main(int argc, char** argv)
{
    if (argc < 2) { cerr << "usage: test_relabel <parameters>" << endl; return 2; }
    ParameterReader para(argv[1]);
    para.set("image_width", "400"); para.set("image_height", "120"); para.set("orb_levels", "3"); para.set("orb_features", "300");
    para.set("camera.cx", "200.0"); para.set("camera.cy", "40.0"); para.set("camera.fx", "300.0"); para.set("camera.fy", "300.0"); para.set("camera.scale", "1000.0");
    para.set("uv_disparity", "0"); para.set("motion_semantic_fuse", "0");
    VisualOdometryStereo::parameters vp; vp.calib.f = 300.0; vp.calib.cu = 200.0; vp.calib.cv = 40.0; vp.base = 0.5;
    try {
        const CAMERA_INTRINSIC_PARAMETERS camera = para.getCamera();
        auto load = [&](int from = 0) {          // key-frames from .. N - 1, fresh frames each time; the corrupted ones are the scene's frames 3 and 5 whatever `from`
            Seq s;
            for (int j = from; j < N; j++) {
                RGBDFrame::Ptr f(new RGBDFrame);
                f->id = j; f->camera = camera;
                vector<uint8_t> hit;
                cast(STEP * j, camera, f->depth, &hit);
                f->rgb.create(H, W, CV_8UC3); f->semantic.create(H, W, CV_8UC3);
                const int band = corrupted(j);
                for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) {
                    uint8_t* c = f->rgb.ptr<uint8_t>(y) + 3 * x; c[0] = (uint8_t)(x + j); c[1] = (uint8_t)(y * 2); c[2] = (uint8_t)(x ^ y);
                    uint8_t* s3 = f->semantic.ptr<uint8_t>(y) + 3 * x;
                    const int what = hit[(size_t)y * W + x];          // palette colours (BGR): Road 4, Pavement 5, Car 9, Tree 6
                    if (what == HIT_PAVEMENT) { s3[0] = 222; s3[1] = 40; s3[2] = 60; } else if (what == HIT_BOX) { s3[0] = 128; s3[1] = 0; s3[2] = 64; } else { s3[0] = 128; s3[1] = 64; s3[2] = 128; }
                    if (band >= 0 && x >= BAND[band][0] && x < BAND[band][1]) { s3[0] = 0; s3[1] = 128; s3[2] = 128; }
                    if (band >= 0 && x >= BAND[band][2] && x < BAND[band][3]) { s3[0] = 1; s3[1] = 2; s3[2] = 3; }
                }
                Eigen::Isometry3d T = Eigen::Isometry3d::Identity(); T(2, 3) = STEP * j;
                f->setTransform(T);
                s.kfs.push_back(f); s.hit.push_back(hit);
            }
            return s;
        };
        Tracker::Ptr tracker(new Tracker(para, vp));
        PoseGraph pg(para, tracker);
        ParameterReader on = para; on.set("mapper_relabel", "1"); on.set("mapper_relabel_hash", "1");
        ParameterReader on_host = on; on_host.set("mapper_device_map", "0");
        ParameterReader ren_off = para; ren_off.set("mapper_render", "1");
        ParameterReader ren_on = on; ren_on.set("mapper_render", "1");
        ParameterReader all_on = on; all_on.set("mapper_carve", "1"); all_on.set("mapper_align", "1");
        ParameterReader all_host = all_on; all_host.set("mapper_device_map", "0");
        QuietMapper off_m(para, pg), dev_m(on, pg), host_m(on_host, pg), roff_m(ren_off, pg), ron_m(ren_on, pg), adev_m(all_on, pg), ahost_m(all_host, pg);
        CHECK("switch_defaults_to_off", off_m.relabelLabelFnv() == 0 && !off_m.relabels() && dev_m.relabels() && host_m.relabels() && off_m.relabelledKeyframes() == 0);
        Seq s0 = load(), sd = load(), sh = load();
        const size_t n = s0.kfs.size();
        const double md = para.getData<double>("mapper_max_distance", 40.0);
        ssm_camera cam; cam.cx = camera.cx; cam.cy = camera.cy; cam.fx = camera.fx; cam.fy = camera.fy; cam.scale = camera.scale;
        ssm::Device& d = off_m.dev_(W, H);

        // switch off: the clouds are what the calls that exist give
        vector<vector<ssm_point>> plain(n);
        bool off_same = true;
        for (size_t i = 0; i < n; i++) {
            plain[i].resize((size_t)W * H); int m = 0;
            d.check(ssm_backproject(d.ctx(), s0.kfs[i]->depth.ptr<uint16_t>(), s0.kfs[i]->rgb.data, s0.kfs[i]->semantic.data, W, H, &cam, nullptr, md, plain[i].data(), (int)plain[i].size(), &m), "ssm_backproject");
            plain[i].resize((size_t)m);
            off_same = off_same && same(off_m.cloudNow(s0.kfs[i]), plain[i]) && plain[i].size() > 10000;
        }
        ssm_relabel_info none{};
        CHECK("switch_off_clouds_as_before", off_same && off_m.relabelledKeyframes() == 0 && !off_m.relabelInfoOf(s0.kfs[0], &none));

        // the host replay: ssm_relabel_host cloud after cloud, the views the key-frames' images within the window
        ssm_relabel_params P; ssm_relabel_params_default(&P);
        const int win = 5;
        vector<vector<uint8_t>> lab(n);
        for (size_t j = 0; j < n; j++) { lab[j].resize((size_t)W * H); ssm_relabel_labels_host(s0.kfs[j]->semantic.data, (int64_t)W * H, lab[j].data()); }
        vector<vector<uint32_t>> want(n); vector<vector<uint64_t>> votes(n); vector<ssm_relabel_info> winfo(n);
        for (size_t i = 0; i < n; i++) {
            vector<ssm_relabel_host_view> hv; vector<double> poses;
            for (size_t j = i > (size_t)win ? i - win : 0; j <= min(n - 1, i + win); j++) {
                if (j == i) continue;
                ssm_relabel_host_view v; v.depth = s0.kfs[j]->depth.ptr<uint16_t>(); v.label = lab[j].data(); v.w = W; v.h = H; v.cam = cam; hv.push_back(v);
                const Eigen::Isometry3d T = s0.kfs[j]->getTransform(); poses.insert(poses.end(), T.data(), T.data() + 16);
            }
            const Eigen::Isometry3d Tc = s0.kfs[i]->getTransform();
            want[i].resize(plain[i].size()); votes[i].resize(plain[i].size());
            if (ssm_relabel_host(hv.data(), poses.data(), (int)hv.size(), plain[i].data(), (int)plain[i].size(), Tc.data(), &P, want[i].data(), votes[i].data(), &winfo[i]) != SSM_OK)
                throw runtime_error("ssm_relabel_host failed");
        }
        dev_m.relabelAll(sd.kfs); host_m.relabelAll(sh.kfs);
        bool routes = true, replay = true, rest = true, infos = true;
        vector<vector<ssm_point>> fused(n);
        for (size_t i = 0; i < n; i++) {
            fused[i] = dev_m.cloudNow(sd.kfs[i]);
            const vector<ssm_point> hc = host_m.cloudNow(sh.kfs[i]);
            routes = routes && same(fused[i], hc);
            replay = replay && fused[i].size() == plain[i].size();
            for (size_t k = 0; replay && k < plain[i].size(); k++) {
                replay = fused[i][k].label == want[i][k];
                ssm_point q = fused[i][k]; q.label = plain[i][k].label; rest = rest && memcmp(&q, &plain[i][k], sizeof q) == 0;
            }
            ssm_relabel_info a{}, b{};
            infos = infos && dev_m.relabelInfoOf(sd.kfs[i], &a) && host_m.relabelInfoOf(sh.kfs[i], &b) && memcmp(&a, &winfo[i], sizeof a) == 0 && memcmp(&b, &winfo[i], sizeof b) == 0;
        }
        CHECK("routes_give_the_same_bytes", routes && dev_m.relabelLabelFnv() == host_m.relabelLabelFnv() && dev_m.relabelLabelFnv() != 0);
        CHECK("the_labels_are_the_host_function_replayed_cloud_after_cloud", replay && infos);
        CHECK("only_the_label_bytes_change", rest);
        CHECK("every_cloud_once_and_at_most_2_window_plus_1_views_alive", dev_m.relabelledKeyframes() == (int)n && host_m.relabelledKeyframes() == (int)n && dev_m.relabelMaxViewsAlive() <= 2 * win + 1 &&
              dev_m.relabelMaxViewsAlive() == (int)min(n, (size_t)2 * win + 1));

        // against the scene's truth: a point's pixel is its own ray's
        long long band_pts = 0, band_two = 0, band_ok = 0, true_before = 0, true_lost = 0, wrong0 = 0, unk0 = 0, wrong1 = 0, unk1 = 0;
        for (size_t i = 0; i < n; i++) for (size_t k = 0; k < plain[i].size(); k++) {
            const ssm_point& p = plain[i][k];
            const int x = (int)floor((double)p.x / p.z * camera.fx + camera.cx + 0.5), y = (int)floor((double)p.y / p.z * camera.fy + camera.cy + 0.5);
            if (x < 0 || x >= W || y < 0 || y >= H) throw runtime_error("a point outside its own image");
            const uint32_t t = truth_of(s0.hit[i][(size_t)y * W + x]), L0 = p.label, L1 = fused[i][k].label;
            wrong0 += L0 <= 11 && L0 != t; unk0 += L0 > 11; wrong1 += L1 <= 11 && L1 != t; unk1 += L1 > 11;
            if (L0 == t) { true_before++; true_lost += L1 != t; }
            const int band = corrupted((int)i);
            if (band >= 0 && ((x >= BAND[band][0] && x < BAND[band][1]) || (x >= BAND[band][2] && x < BAND[band][3]))) {
                band_pts++;
                int voting = 0; for (int l = 0; l < 12; l++) voting += (int)((votes[i][k] >> (5 * l)) & 31);
                if (L0 <= 11) voting -= P.own_weight;
                if (voting >= 2) { band_two++; band_ok += L1 == t; }
            }
        }
        cout << "truth: wrong labels " << wrong0 << " -> " << wrong1 << ", unknown labels " << unk0 << " -> " << unk1 << "; " << band_pts << " band points, " << band_two
             << " with at least two voting views, " << band_ok << " of them true afterwards; " << true_before << " true labels before, " << true_lost << " lost" << endl;
        CHECK("band_points_with_two_voting_views_end_true", band_two > 1000 && band_ok == band_two);
        CHECK("no_true_label_is_lost", true_before > 100000 && true_lost == 0);
        CHECK("wrong_and_unknown_labels_fall_strictly", wrong0 > 0 && unk0 > 0 && wrong1 + unk1 < wrong0 + unk0);

        // the rendering: geometry and so every z-buffer winner is unchanged; over the views other than 3 and 5 the label counts can only improve
        {
            Seq a = load(), b = load();
            roff_m.renderAll(a.kfs);
            ron_m.relabelAll(b.kfs); ron_m.renderAll(b.kfs);
            bool geo = true, total = true, dis = true; long long agree0 = 0, agree1 = 0, dis0 = 0, dis1 = 0;
            for (size_t i = 0; i < n; i++) {
                if (corrupted((int)i) >= 0) continue;
                ssm_render_compare_info x{}, y{};
                if (!roff_m.renderInfoOf(a.kfs[i], &x) || !ron_m.renderInfoOf(b.kfs[i], &y)) throw runtime_error("a view was not rendered");
                geo = geo && x.unrendered == y.unrendered && x.no_depth == y.no_depth && x.in_front == y.in_front && x.behind == y.behind && x.agree == y.agree && x.n_pixels == y.n_pixels;
                total = total && x.label_agree + x.label_disagree + x.label_unknown == y.label_agree + y.label_disagree + y.label_unknown;
                dis = dis && y.label_disagree <= x.label_disagree;
                agree0 += x.label_agree; agree1 += y.label_agree; dis0 += x.label_disagree; dis1 += y.label_disagree;
            }
            cout << "rendering (views other than 3 and 5): label_agree " << agree0 << " -> " << agree1 << ", label_disagree " << dis0 << " -> " << dis1 << endl;
            CHECK("rendering_geometric_counts_identical", geo && total);
            CHECK("rendering_label_disagree_does_not_rise_and_agree_rises", dis && agree1 > agree0);
        }
        // carving and alignment on top: both routes agree
        {
            Seq a = load(), b = load();
            adev_m.alignCarveUpTo(a.kfs); ahost_m.alignCarveUpTo(b.kfs);
            adev_m.relabelAll(a.kfs); ahost_m.relabelAll(b.kfs);
            bool ok = adev_m.relabelledKeyframes() == (int)n; long long changed = 0;
            for (size_t i = 0; i < n; i++) { ok = ok && same(adev_m.cloudNow(a.kfs[i]), ahost_m.cloudNow(b.kfs[i])); ssm_relabel_info I{}; adev_m.relabelInfoOf(a.kfs[i], &I); changed += I.n_changed; }
            CHECK("with_carving_and_alignment_both_routes_agree", ok && changed > 0 && adev_m.relabelLabelFnv() == ahost_m.relabelLabelFnv());
        }
        // the ground grid sees the fused labels (0.5 m cells, ground_radius 3 as in test_grid.cpp): every key-frame's cloud goes in, 3 and 5 included.  Without the
        // switch some cells' ground label is Tree.  With it the rule promises: fewer such cells, and none among the cells that hold no point still labelled Tree
        // (a band point that fewer than two views vote on keeps its label; with two it ends true, checked above).  A point's cell is grid_core.h's: under the default
        // G and a pose that only translates along z, floor((x - x0) / cell) and floor((z + t_z - y0) / cell) in double
        {
            ParameterReader g_off = para; g_off.set("mapper_grid", "1"); g_off.set("mapper_grid_cell", "0.5"); g_off.set("mapper_grid_ground_radius", "3");
            ParameterReader g_on = g_off; g_on.set("mapper_relabel", "1");
            ParameterReader g_host = g_on; g_host.set("mapper_device_map", "0");
            QuietMapper goff_m(g_off, pg), gon_m(g_on, pg), ghost_m(g_host, pg);
            Seq a = load(), b = load(), c = load();
            goff_m.buildGrid(a.kfs);
            gon_m.relabelAll(b.kfs); gon_m.buildGrid(b.kfs);
            ghost_m.relabelAll(c.kfs); ghost_m.buildGrid(c.kfs);
            vector<uint8_t> gl0, gl1, gl2, cls0, cls1;
            if (!goff_m.gridFetch(&cls0, &gl0, nullptr, nullptr, nullptr, nullptr, nullptr) || !gon_m.gridFetch(&cls1, &gl1, nullptr, nullptr, nullptr, nullptr, nullptr) ||
                !ghost_m.gridFetch(nullptr, &gl2, nullptr, nullptr, nullptr, nullptr, nullptr)) throw runtime_error("a grid was not built");
            const ssm_grid_params G = gon_m.gridParams();
            vector<uint8_t> still((size_t)G.nx * G.ny, 0);          // cells that hold a point still labelled Tree after the fusion
            for (size_t i = 0; i < n; i++) for (size_t k = 0; k < fused[i].size(); k++) {
                if (fused[i][k].label != (uint32_t)TREE) continue;
                const double cx = floor(((double)fused[i][k].x - G.x0) / G.cell), cy = floor(((double)fused[i][k].z + STEP * (double)i - G.y0) / G.cell);
                if (cx >= 0 && cx < G.nx && cy >= 0 && cy < G.ny) still[(size_t)cy * G.nx + (size_t)cx] = 1;
            }
            long long t0 = 0, t1 = 0, t1_clean = 0, excused = 0;
            for (size_t q = 0; q < gl1.size(); q++) { t0 += cls0[q] != 0 && gl0[q] == TREE; t1 += cls1[q] != 0 && gl1[q] == TREE; t1_clean += cls1[q] != 0 && gl1[q] == TREE && !still[q]; excused += still[q]; }
            cout << "ground grid: " << t0 << " cells with ground label Tree without the switch, " << t1 << " with it (" << excused << " cells hold a point still labelled Tree)" << endl;
            CHECK("grid_routes_give_the_same_ground_labels", gl1 == gl2 && gl0.size() == gl1.size() && memcmp(&G, &goff_m.gridParams(), sizeof G) == 0);
            CHECK("some_ground_labels_are_tree_without_the_switch", t0 > 0);
            CHECK("tree_ground_labels_fall_and_none_is_left_where_no_tree_point_is", t1 < t0 && t1_clean == 0);
        }
        // the published map after the final rebuild.  A rebuild takes every second key-frame: of the 8 key-frames those are 0, 2, 4, 6 -- none of them corrupted, so
        // this check (the issue's) guards only against the fusion INTRODUCING Tree: the map holds none with the switch off either, which is asserted too.
        // From key-frame 1 on (1 .. 7) the corrupted frames are among those a rebuild takes: there the Tree voxels must fall strictly -- not to zero: a band point
        // that fewer than two views vote on (it leaves the later views' images, and key-frame 3 then has two earlier views only) keeps its label by the rule
        {
            auto trees = [&](const ParameterReader& p, int from) {
                PoseGraph g(para, tracker);
                g.keyframes = load(from).kfs;
                Mapper m(p, g);
                for (int t = 0; t < 20000 && m.updates() < 1 && !m.viewerFailed; t++) this_thread::sleep_for(chrono::milliseconds(1));
                m.shutdown();
                if (m.viewerFailed || m.deviceMapFellBack) throw runtime_error("the viewer failed");
                Mapper::PointCloud::Ptr map = m.getGlobalMap();
                long long t6 = 0;
                for (const auto& q : map->points) t6 += reinterpret_cast<const ssm_point*>(&q)->label == (uint32_t)TREE;
                return make_pair(t6, (long long)map->points.size());
            };
            const auto all = trees(on, 0), all_host = trees(on_host, 0), all_off = trees(para, 0);
            const auto off = trees(para, 1), with = trees(on, 1), with_host = trees(on_host, 1);
            cout << "published map, key-frames 0 .. 7: " << all.first << " of " << all.second << " voxels labelled Tree with the switch; key-frames 1 .. 7: " << off.first << " of " << off.second
                 << " without the switch, " << with.first << " of " << with.second << " with it" << endl;
            CHECK("the_published_map_holds_no_tree_after_the_final_rebuild", all.first == 0 && all_host.first == 0 && all_off.first == 0 && all.second > 1000 && all_host.second == all.second && all_off.second == all.second);
            CHECK("tree_voxels_fall_where_a_rebuild_takes_the_corrupted_frames", off.first > 0 && with.first < off.first && with_host.first == with.first && with.second == off.second);
        }
    } catch (const exception& e) { cout << "FAIL exception " << e.what() << endl; fails++; }
    cout << (fails ? "FAILED" : "ALL PASSED") << endl;
    return fails;
}
