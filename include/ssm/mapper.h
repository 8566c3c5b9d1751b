// ssm/mapper.h -- rgbd_tutor::Mapper (reference include/mapper.h:15-70, src/mapper.cpp): the viewer thread that turns
// key-frames into the global voxel map.  generatePointCloud (+ semantic_motion_fuse) and the pcl::VoxelGrid filter run
// on the GPU through ssm_backproject / ssm_voxel_filter; the schedule of Mapper::viewer (src/mapper.cpp:109-162) is
// kept: every 15th update rebuilds from every 2nd key-frame, otherwise the last <= 5 key-frames are added, then one
// VoxelGrid pass over the whole map.  Differences, all deliberate: no PCL visualiser window (mapper_render=1 writes rendered views as PNG instead, see below); key-frames are read under
// keyframes_mutex (the reference polls them unlocked, mapper.cpp:114-136); the PCD path comes from `map_output`
// instead of a hard-coded absolute path (mapper.cpp:167).  The unsigned wrap of `i > keyframes.size()-6`
// (mapper.cpp:134: with fewer than 6 key-frames the incremental branch adds nothing) IS reproduced unless
// mapper_fix_incremental=1.
// Round 4: the viewer's map lives on the DEVICE (mapper_device_map, default 1).  The reference (and this class before) makes a host copy of every chosen
// key-frame's cloud, transforms it in a host loop, concatenates on the host and pushes the WHOLE map through the filter on every update.  Now a key-frame's
// camera-frame cloud is made once and stays in HBM (ssm_backproject_dev: the device form of frame->pointcloud, mapper.cpp:17-20), an update transforms
// the chosen clouds by their current poses, adds the previous centroids and filters, all on the device (ssm_viewer_map_update), and only the map that is
// published (globalMap / the PCD) is downloaded.  Same bytes: the filter's sums are exact integers, independent of the order of the points.
// motion_semantic_fuse=1 (default 0: the class exactly as before): the mask that gates a key-frame's cloud is the semantic-motion fusion's (DESIGN.md s.14;
// reference src/mapper.cpp:217-271, commented out there for want of a motion mask): Car joins the maybe-moving classes, and a blob of them leaves the map only
// when it is large (motion_area_thres) and enough of it (motion_overlay_portion_thres) lies under frame->moving_mask, which UVDisparity fills (uv_disparity=1).
// A frame whose moving_mask is empty is gated as before.  Both routes to a cloud take the fused form of their call.
// mapper_outlier_removal=1 (default 0: the clouds exactly as before): a key-frame's camera-frame cloud goes through the statistical outlier removal (DESIGN.md s.15;
// pcl::StatisticalOutlierRemoval with mapper_sor_mean_k 30 and mapper_sor_stddev 1.0 as reference src/mapper.cpp:137-146 sets it up, commented out there for its cost
// on a CPU) ONCE, when the cloud is made, on both routes: deviceCloud through ssm_cloud_sor, generatePointCloud through ssm_sor_filter -- the same bytes.  The
// reference's block filters the world-frame copy, in the incremental branch only, and again at every update.  Here the rebuild branch sees the same filtered clouds as
// the incremental one and no cloud is filtered twice; a rigid transform changes the distances between points only by its rounding, so what the filter removes is the
// same up to points whose value sits within that rounding of the threshold.
// mapper_carve=1 (default 0: nothing of this runs, every cloud and every map exactly as before): free-space carving (the reference has no such
// step).  Every key-frame j is a VIEW exactly once, in ascending j, before the viewer selects the clouds of an update and once more when the viewer ends (so every
// key-frame has been applied however the thread was scheduled): its depth image judges the clouds of key-frames j - mapper_carve_window .. j - 1, which are made on
// demand; the poses are read at that moment.  A point seen through mapper_carve_votes views in a row leaves its cloud for good.  Both routes give the same bytes:
// deviceCloud / ssm_carve (one call per view: the view's depth image is uploaded, applied to all its clouds and freed -- it is never needed again, so no view lives
// for `window` key-frames) and frame->pointcloud / ssm_carve_points with the counters kept beside the cloud (carveRun).  The two do not mix: when the device-resident
// update fails with the switch on, the counters of the freed device clouds are gone, so the viewer stops (viewerFailed) instead of falling back to the host path.
// Carved points leave the PUBLISHED map at the next rebuild (every 15th update): an incremental update carries the previous centroids.  The schedule is unchanged.
// mapper_render=1 (default 0: nothing of this runs, every cloud, map and figure exactly as before): map rendering (the project's stand-in for the
// reference's visualiser window, and the yardstick of the three switches above).  When the viewer ends -- after the last carveUpTo, before the device clouds are
// freed -- every key-frame j is a VIEW once, in ascending j: the clouds of the key-frames i != j with |i - j| <= mapper_render_window, in their final state
// (filtered and carved as the other switches left them; made on demand) and at the poses read at that moment, are splatted z-buffered into j's camera, and the
// rendering is compared per pixel with j's own depth and semantic image: a leave-one-out reprojection figure (renderInfoOf).  It runs once, at the end, so it does
// not depend on the viewer's update schedule.  Both routes give the same bytes: deviceCloud / ssm_render_clouds and frame->pointcloud / ssm_render_points (the host
// route when mapper_device_map=0 or after the device-resident update fell back).  With mapper_render_dir set every view writes render_%06d_depth.png (16 bit),
// _bgr.png, _label.png (palette colours) and _class.png (0 unrendered, 1 no depth, 2 in front, 3 behind, 4 agree) there, %06d the key-frame's number.
// mapper_align=1 (default 0: nothing of this runs, every cloud, map and figure exactly as before): dense alignment (the reference has no such
// step).  Every key-frame j is aligned exactly once, in ascending j, before it becomes a carving view (with mapper_carve=1 the two alternate key-frame by key-frame:
// j is aligned against the clouds as the views before j left them) and before an update reads its pose: its depth image is the
// VIEW, the clouds of key-frames j - mapper_align_window .. j - 1 (made on demand) at their MAP POSES are aligned to it by point-to-plane ICP, from the start pose
// D_prev . P_j -- P_j the key-frame's pose as the Mapper hands poses on (mapper_invert_pose applied), D_prev the last accepted world-frame correction, so drift
// the next key-frame shares is carried forward.  An alignment is accepted when it converged or reached max_iterations with at least min_inliers inliers; it then
// defines D_j = T_out . inverse(P_j), any other outcome gives D_j = D_prev.  The map pose D_j . P_j is what the Mapper uses wherever it read the key-frame's pose:
// the map update, carveUpTo and the rendering.  RGBDFrame::T_f_w, the tracker and the pose graph are not written, and the map pose is FIXED when the key-frame is
// aligned: a pose-graph correction that arrives later does not recompute it (a limit).  Both routes give the same bytes: deviceCloud /
// ssm_align_clouds and frame->pointcloud / ssm_align_points.
// mapper_grid=1 (default 0: nothing of this runs, every cloud, map and figure exactly as before): the ground grid (the reference has no such step).
// When the viewer ends -- after the rendering, before the device clouds are freed -- ONE grid is built from EVERY key-frame's cloud, in its final state (filtered
// and carved as the other switches left it; made on demand) and at its map pose (mapPoseOf).  The extent is not a parameter: the bounding box, in the grid frame,
// of the key-frames' map positions, widened by mapper_max_distance, x0 and y0 snapped down and the far edge up to whole cells; beyond 2^24 cells the build is
// skipped with a notice (gridInfo().skipped).  mapper_grid_cell, _step, _ground_radius, _min_obstacle_points, _h_min, _h_max set the spec, mapper_grid_up and
// mapper_grid_forward (three numbers each, default `0 -1 0` and `0 0 1`) the grid frame.  Both routes give the same bytes: deviceCloud / ssm_grid_clouds and
// frame->pointcloud / ssm_grid_points.  With mapper_grid_dir set the build writes grid_colour.png, grid_height.png (16 bit) and grid.txt (x0, y0, cell, nx, ny,
// h_min, G: what georeferences the images) there.
// mapper_objects=1 (default 0: nothing of this runs, every cloud, map, grid and figure exactly as before): object extraction (the reference has
// no such step).  Right after buildGrid, on the same grid target and cloud list, extractObjects labels the grid's obstacle cells of the wanted classes into
// components (ssm_objects_grid) and assigns the clouds' HIGH points to the kept ones (ssm_objects_clouds / ssm_objects_points: both routes give the same bytes).
// The grid is built for it even with mapper_grid=0; then no grid files are written.  mapper_objects_labels (a list of label ids, default `9 10 11`: Vehicle,
// Pedestrian, Bike), _connectivity, _min_cells, _min_points, _min_height set the rule.  objectsInfo(), objectsFetch(records, object_id); with mapper_objects_dir
// set the call writes objects.txt (one line per object: id, label name, cells, points, the box and the centroid in metres of the grid frame, ground and top
// height) and objects_id.png (16 bit, id + 1, 0 where there is no object; row r is cell row ny - 1 - r as in the grid's images).
// mapper_clearance=1 (default 0: nothing of this runs, every cloud, map, grid, object and figure exactly as before): the clearance map (the
// reference has no such step).  In buildGrid, after the grid (and after the objects when both are on), on the same grid target, mapClearance gives every cell the
// squared distance to the nearest blocked cell and marks the free cells a vehicle of mapper_clearance_radius (1.0 m) can occupy and those of them connected to
// the seed (ssm_clearance_grid).  The grid is built for it even with mapper_grid=0; then no grid files are written.  mapper_clearance_blocked and
// mapper_clearance_free (lists of cell classes, default `4` and `1`), _connectivity (4), _seed_snap (10 cells) set the rule.  The seed is the cell of the last
// key-frame's camera centre at its map pose, through the grid's G and ssm_clrc::cell_of; a centre outside the grid means no seed.  clearanceInfo(),
// clearanceFetch(dist2, nearest, reach); with mapper_clearance_dir set the call writes clearance.png (16 bit: min(65535, floor(sqrt(dist2) cell 100)) centimetres,
// 65535 where nothing is blocked), reach.png (8 bit: 0 / 128 / 255) and clearance.txt (the info, one `name value` per line); image row r is cell row ny - 1 - r as
// in the grid's images.
// mapper_relabel=1 (default 0: nothing of this runs, every cloud, map and figure exactly as before): label fusion (the reference has no such step).
// When the viewer ends -- after the last alignCarveUpTo, before the rendering and the ground grid, which then see the fused labels -- relabelAll lets the key-frames
// j != i with |i - j| <= mapper_relabel_window (5; at most 8: a call takes 16 views) vote on the labels of key-frame i's cloud, at the map poses (mapPoseOf), every
// cloud exactly once in ascending order.  The views are the key-frames' depth and semantic IMAGES, never other clouds, so the order does not matter.  View objects
// are made when first needed and freed once no later cloud needs them: at most 2 window + 1 are alive.  mapper_relabel_radius, _edge_guard, _own_weight, _votes set
// the rule; the tolerances are carving's parameters.  Both routes give the same bytes: deviceCloud / ssm_relabel and frame->pointcloud / ssm_relabel_points.  Then
// ONE more map update with rebuild = true runs through the update code of the loop (updateMap), so the published and saved map carries fused labels whatever the
// thread's timing was.  relabelInfoOf(frame), relabelledKeyframes(); with mapper_relabel_hash=1 also relabelLabelFnv() (the driver's relabel_fnv).
#pragma once
#include "common_headers.h"
#include <atomic>
#include <iomanip>
#include <map>
#include <unordered_map>
#include "device.h"
#include "pose_graph.h"
#include "rgbdframe.h"
#include "png_io.h"
#include "clearance_core.h"
namespace rgbd_tutor {
class Mapper {
public:
    typedef pcl::PointXYZRGBA PointT;
    typedef pcl::PointCloud<PointT> PointCloud;
    Mapper(const ParameterReader& para, PoseGraph& graph) : parameterReader(para), poseGraph(graph) {
        resolution = para.getData<double>("mapper_resolution", 0.1);
        max_distance = para.getData<double>("mapper_max_distance", 40.0);
        area_thres = para.getData<int>("motion_area_thres", 1000);
        overlay_portion_thres = para.getData<double>("motion_overlay_portion_thres", 0.143);
        fuse_motion = para.getData<int>("motion_semantic_fuse", 0) != 0;
        fix_incremental = para.getData<int>("mapper_fix_incremental", 0) != 0;
        invert_pose = para.getData<int>("mapper_invert_pose", 0) != 0;          // the commented alternative at mapper.cpp:89
        map_output = para.getData<string>("map_output", string(""));
        device_map = para.getData<int>("mapper_device_map", 1) != 0;
        outlier_removal = para.getData<int>("mapper_outlier_removal", 0) != 0;
        sor_mean_k = para.getData<int>("mapper_sor_mean_k", 30);
        sor_stddev = para.getData<double>("mapper_sor_stddev", 1.0);
        carve = para.getData<int>("mapper_carve", 0) != 0;
        carve_window = para.getData<int>("mapper_carve_window", 5);                 // the reach of the reference's "last five" loop (mapper.cpp:134)
        ssm_carve_params_default(&carve_params);
        carve_params.min_votes = para.getData<int>("mapper_carve_votes", carve_params.min_votes);
        carve_params.radius = para.getData<int>("mapper_carve_radius", carve_params.radius);
        carve_params.tol_abs = para.getData<double>("mapper_carve_tol_abs", carve_params.tol_abs);
        carve_params.tol_rel_ppm = para.getData<int>("mapper_carve_tol_rel_ppm", carve_params.tol_rel_ppm);
        render = para.getData<int>("mapper_render", 0) != 0;
        render_window = para.getData<int>("mapper_render_window", 5);
        render_dir = para.getData<string>("mapper_render_dir", string(""));
        ssm_render_params_default(&render_params);
        render_params.point_size = para.getData<double>("mapper_render_point_size", render_params.point_size);
        render_params.max_radius = para.getData<int>("mapper_render_max_radius", render_params.max_radius);
        align = para.getData<int>("mapper_align", 0) != 0;
        align_window = para.getData<int>("mapper_align_window", 5);
        ssm_align_params_default(&align_params);
        align_params.max_iterations = para.getData<int>("mapper_align_max_iterations", align_params.max_iterations);
        align_params.stride = para.getData<int>("mapper_align_stride", align_params.stride);
        align_params.z_min = para.getData<double>("mapper_align_z_min", align_params.z_min);
        align_params.z_max = para.getData<double>("mapper_align_z_max", align_params.z_max);
        align_params.dist_max = para.getData<double>("mapper_align_dist_max", align_params.dist_max);
        align_params.delta = para.getData<double>("mapper_align_delta", align_params.delta);
        align_params.damping = para.getData<double>("mapper_align_damping", align_params.damping);
        align_params.eps_rot = para.getData<double>("mapper_align_eps_rot", align_params.eps_rot);
        align_params.eps_trans = para.getData<double>("mapper_align_eps_trans", align_params.eps_trans);
        align_params.min_inliers = para.getData<int>("mapper_align_min_inliers", align_params.min_inliers);
        align_params.max_shift = para.getData<double>("mapper_align_max_shift", align_params.max_shift);
        align_params.max_angle = para.getData<double>("mapper_align_max_angle", align_params.max_angle);
        align_params.tol_abs = para.getData<double>("mapper_align_tol_abs", align_params.tol_abs);
        align_params.tol_rel_ppm = para.getData<int>("mapper_align_tol_rel_ppm", align_params.tol_rel_ppm);
        relabel = para.getData<int>("mapper_relabel", 0) != 0;
        relabel_window = para.getData<int>("mapper_relabel_window", 5);
        relabel_hash = para.getData<int>("mapper_relabel_hash", 0) != 0;          // relabelLabelFnv() is wanted: costs one fetch of every cloud on the device route
        ssm_relabel_params_default(&relabel_params);
        relabel_params.radius = para.getData<int>("mapper_relabel_radius", relabel_params.radius);
        relabel_params.edge_guard = para.getData<int>("mapper_relabel_edge_guard", relabel_params.edge_guard);
        relabel_params.own_weight = para.getData<int>("mapper_relabel_own_weight", relabel_params.own_weight);
        relabel_params.min_votes = para.getData<int>("mapper_relabel_votes", relabel_params.min_votes);
        relabel_params.tol_abs = carve_params.tol_abs; relabel_params.tol_rel_ppm = carve_params.tol_rel_ppm; relabel_params.z_min = carve_params.z_min;
        if (relabel && (relabel_window < 0 || relabel_window > 8)) throw std::runtime_error("Mapper: mapper_relabel_window must be 0..8 (a call takes 16 views)");
        grid = para.getData<int>("mapper_grid", 0) != 0;
        grid_dir = para.getData<string>("mapper_grid_dir", string(""));
        ssm_grid_params_default(&grid_params);
        grid_params.cell = para.getData<double>("mapper_grid_cell", grid_params.cell);
        grid_params.step = para.getData<double>("mapper_grid_step", grid_params.step);
        grid_params.ground_radius = para.getData<int>("mapper_grid_ground_radius", grid_params.ground_radius);
        grid_params.min_obstacle_points = para.getData<int>("mapper_grid_min_obstacle_points", grid_params.min_obstacle_points);
        grid_params.h_min = para.getData<double>("mapper_grid_h_min", grid_params.h_min);
        grid_params.h_max = para.getData<double>("mapper_grid_h_max", grid_params.h_max);
        objects = para.getData<int>("mapper_objects", 0) != 0;
        clearance = para.getData<int>("mapper_clearance", 0) != 0;
        route = para.getData<int>("mapper_route", 0) != 0;
        if (grid || objects || clearance || route) {          // (the objects, the clearance map and the route field stand on a grid of the same frame, whether or not the grid itself is wanted)
            double up[3] = {0, -1, 0}, fw[3] = {0, 0, 1};
            auto three = [&](const char* key, double* v) {
                auto it = para.data.find(key);
                if (it == para.data.end()) return;
                istringstream ss(it->second);
                if (!(ss >> v[0] >> v[1] >> v[2])) throw std::runtime_error(string("Mapper: ") + key + " takes three numbers");
            };
            three("mapper_grid_up", up); three("mapper_grid_forward", fw);
            if (ssm_grid_frame_from_up(up, fw, grid_params.G) != SSM_OK) throw std::runtime_error("Mapper: mapper_grid_up and mapper_grid_forward do not span a frame");
        }
        objects_dir = para.getData<string>("mapper_objects_dir", string(""));
        ssm_objects_params_default(&objects_params);
        objects_params.connectivity = para.getData<int>("mapper_objects_connectivity", objects_params.connectivity);
        objects_params.min_cells = para.getData<int>("mapper_objects_min_cells", objects_params.min_cells);
        objects_params.min_points = para.getData<int>("mapper_objects_min_points", objects_params.min_points);
        objects_params.min_height = para.getData<double>("mapper_objects_min_height", objects_params.min_height);
        {
            auto it = para.data.find("mapper_objects_labels");
            if (it != para.data.end()) {
                istringstream ss(it->second); int l; objects_params.label_mask = 0;
                while (ss >> l) { if (l < 0 || l > 11) throw std::runtime_error("Mapper: mapper_objects_labels takes label ids 0..11"); objects_params.label_mask |= 1u << l; }
            }
        }
        clearance_dir = para.getData<string>("mapper_clearance_dir", string(""));
        ssm_clearance_params_default(&clearance_params);
        clearance_params.radius = para.getData<double>("mapper_clearance_radius", clearance_params.radius);
        clearance_params.connectivity = para.getData<int>("mapper_clearance_connectivity", clearance_params.connectivity);
        clearance_params.seed_snap = para.getData<int>("mapper_clearance_seed_snap", clearance_params.seed_snap);
        for (int which = 0; which < 2; which++) {
            auto it = para.data.find(which ? "mapper_clearance_free" : "mapper_clearance_blocked");
            if (it == para.data.end()) continue;
            istringstream ss(it->second); int l; uint32_t mask = 0;
            while (ss >> l) { if (l < 0 || l > 4) throw std::runtime_error("Mapper: mapper_clearance_blocked and mapper_clearance_free take cell classes 0..4"); mask |= 1u << l; }
            (which ? clearance_params.free_mask : clearance_params.blocked_mask) = mask;
        }
        route_dir = para.getData<string>("mapper_route_dir", string(""));
        ssm_route_params_default(&route_params);
        route_params.moves = para.getData<int>("mapper_route_moves", route_params.moves);
        route_params.near_weight = para.getData<int>("mapper_route_near_weight", route_params.near_weight);
        route_params.comfort = para.getData<double>("mapper_route_comfort", route_params.comfort);
        route_goal_snap = para.getData<int>("mapper_route_goal_snap", 10);
        route_max_path = para.getData<int>("mapper_route_max_path", 0);          // 0: 4 (nx + ny) of the grid that is built
        route_has_goal = para.data.find("mapper_route_goal_x") != para.data.end() && para.data.find("mapper_route_goal_y") != para.data.end();
        route_goal_x = para.getData<double>("mapper_route_goal_x", 0.0); route_goal_y = para.getData<double>("mapper_route_goal_y", 0.0);
        test_fail_update = para.getData<int>("mapper_test_fail_update", -1);        // tests: the device-resident update with this number fails (-> the host path from there on)
        viewerThread = make_shared<thread>(bind(&Mapper::viewer, this));
    }
    void shutdown() { shutdownFlag = true; if (viewerThread != nullptr && viewerThread->joinable()) viewerThread->join(); }
    void SaveMap() {}                                                          // empty in the reference too (mapper.cpp:179-187)
    PointCloud::Ptr getGlobalMap() { unique_lock<mutex> lck(mapMutex); return globalMap; }
    int updates() const { return cntGlobalUpdate.load(); }

    // viewer thread (src/mapper.cpp:96-171)
    void viewer() {
        PointCloud::Ptr map(new PointCloud);
        try {
        while (!shutdownFlag) {
            const vector<RGBDFrame::Ptr> kfs = keyframesNow();
            if (kfs.size() <= (size_t)keyframe_size) { this_thread::sleep_for(chrono::milliseconds(1)); continue; }
            auto t0 = chrono::steady_clock::now();
            alignCarveUpTo(kfs);
            updateMap(kfs, cntGlobalUpdate % 15 == 0, map, t0);
        }
        if (align || carve) {                           // the key-frames that came after the last update are aligned and are views too: the final state does not depend on this thread's timing
            alignCarveUpTo(keyframesNow());
        }
        if (relabel) {                                  // every cloud takes the label its neighbouring views agree on; then one rebuild, so the map carries the fused labels
            const vector<RGBDFrame::Ptr> kfs = keyframesNow();
            auto t0 = chrono::steady_clock::now();
            relabelAll(kfs);
            if (!kfs.empty()) updateMap(kfs, true, map, t0);          // (without a key-frame there is no map to rebuild)
        }
        if (render) renderAll(keyframesNow());          // every key-frame is a view of the clouds around it, in their final state
        if (grid || objects || clearance || route) buildGrid(keyframesNow()); // one ground grid of every key-frame's cloud, in its final state; the objects that stand on it; its clearance map
        } catch (const std::exception& e) {             // a device error on this thread must not std::terminate the process: report it and stop mapping
            cerr << "Mapper::viewer stopped: " << e.what() << endl; viewerFailed = true;
        }
        if (poseGraph.shutDownFlag && !map_output.empty()) { writePCD(map_output, *map); cout << "Map saved!" << endl; }
        for (auto& kv : devClouds) ssm_cloud_free(dev ? dev->ctx() : nullptr, kv.second);      // the device clouds belong to this thread's context
        devClouds.clear();
    }
    // one map update (the body of the viewer's loop, src/mapper.cpp:121-171): the key-frames it adds, the device or the host route, the published map and the two lines
    void updateMap(const vector<RGBDFrame::Ptr>& kfs, const bool rebuild, PointCloud::Ptr& map, chrono::steady_clock::time_point t0) {
        {
            // the key-frames this update adds (mapper.cpp:121-141)
            vector<RGBDFrame::Ptr> sel;
            if (rebuild) { for (size_t i = 0; i < kfs.size(); i += 2) sel.push_back(kfs[i]); }
            else if (fix_incremental) { for (int i = (int)kfs.size() - 1; i >= 0 && i > (int)kfs.size() - 6; i--) sel.push_back(kfs[i]); }
            else { for (int i = (int)kfs.size() - 1; i >= 0 && (size_t)i > kfs.size() - 6; i--) sel.push_back(kfs[i]); }      // size_t wrap as in mapper.cpp:134
            bool on_device = false;
            if (device_map) {
                // clouds stay in HBM; transform + concatenation + VoxelGrid on the device, one download of the filtered map.  Every key-frame's cloud stays resident
                // until the viewer ends (the reference keeps frame->pointcloud in host RAM): when the device runs out of memory on a long sequence -- or any
                // other device error hits this path -- the update is done on the host instead, and so are all later ones: `map` holds the last published map,
                // which is byte for byte what the host schedule would hold at this point, so the switch changes no bits
                try {
                    ssm::Device& d = device(sel.empty() ? 0 : sel[0]->depth.cols, sel.empty() ? 0 : sel[0]->depth.rows);
                    CloudList L = cloudsOf(sel);
                    int nmap = 0;
                    if (test_fail_update >= 0 && cntGlobalUpdate == test_fail_update) d.check(ssm_viewer_map_release(d.ctx(), 1), "ssm_viewer_map_release");
                    d.check(ssm_viewer_map_update(d.ctx(), rebuild ? 1 : 0, L.cl.data(), L.poses.data(), L.m, (float)resolution, &nmap), "ssm_viewer_map_update");
                    PointCloud::Ptr fetched(new PointCloud);
                    fetched->points.resize((size_t)nmap);
                    int got = 0;
                    d.check(ssm_viewer_map_fetch(d.ctx(), reinterpret_cast<ssm_point*>(fetched->points.data()), nmap, &got), "ssm_viewer_map_fetch");
                    fetched->points.resize((size_t)got); fetched->width = got;
                    map->swap(*fetched);
                    cntGlobalUpdate++;
                    keyframe_size = (int)kfs.size();
                    on_device = true;
                } catch (const std::exception& e) {
                    if (carve) { cerr << "Mapper: the device-resident map update failed with mapper_carve=1; the clouds' run counters cannot follow to the host path" << endl; throw; }
                    cerr << "Mapper: the device-resident map update failed (" << e.what() << "); this and the following updates run on the host path" << endl;
                    for (auto& kv : devClouds) ssm_cloud_free(dev ? dev->ctx() : nullptr, kv.second);
                    devClouds.clear(); device_map = false; deviceMapFellBack = true;
                    if (dev) ssm_viewer_map_release(dev->ctx(), 0);      // the slabs of the freed clouds and the update's buffers go back to the device: the host path's own device work (ssm_backproject, ssm_voxel_filter) needs the room
                }
            }
            if (on_device) {
            } else {
                if (rebuild) map->clear();
                for (const RGBDFrame::Ptr& f : sel) *map += *generatePointCloud(f);
                cntGlobalUpdate++;
                PointCloud::Ptr tmp = voxelFilter(map);
                keyframe_size = (int)kfs.size();
                map->swap(*tmp);
            }
            { unique_lock<mutex> lck(mapMutex); globalMap.reset(new PointCloud(*map)); }
            const double ms = chrono::duration<double, milli>(chrono::steady_clock::now() - t0).count();
            cout << "points in global map: " << map->points.size() << endl;
            cout << "Mapping cost time: " << ms << "ms" << endl;
        }
    }
    // the device form of frame->pointcloud: made once per key-frame, kept in HBM (viewer thread only)
    ssm_cloud* deviceCloud(const RGBDFrame::Ptr& frame) {
        auto it = devClouds.find(frame.get());
        if (it != devClouds.end()) return it->second;
        ssm::Device& d = device(frame->depth.cols, frame->depth.rows);
        const int w = frame->depth.cols, h = frame->depth.rows;
        const ssm_camera cam = cameraOf(frame);
        ssm_cloud* cl = nullptr;
        if (fuse_motion) {
            const ssm_motion_fuse_params P = fuseParams();
            d.check(ssm_backproject_fused_dev(d.ctx(), frame->depth.ptr<uint16_t>(), frame->rgb.data, frame->semantic.data, motionOf(frame), w, h, &cam, max_distance, &P, &cl), "ssm_backproject_fused_dev");
        } else
        d.check(ssm_backproject_dev(d.ctx(), frame->depth.ptr<uint16_t>(), frame->rgb.data, frame->semantic.data, w, h, &cam, max_distance, &cl), "ssm_backproject_dev");
        if (outlier_removal) {
            const ssm_sor_params P = sorParams(); ssm_sor_info I{};
            const int rc = ssm_cloud_sor(d.ctx(), cl, &P, &I);
            if (rc != SSM_OK) ssm_cloud_free(d.ctx(), cl);
            d.check(rc, "ssm_cloud_sor");
            sorInfo[frame.get()] = I;
        }
        devClouds[frame.get()] = cl;
        cloudsComputed++;
        return cl;
    }
    static ssm_camera cameraOf(const RGBDFrame::Ptr& f) {                      // a frame's camera as the library takes it
        ssm_camera cam; cam.cx = f->camera.cx; cam.cy = f->camera.cy; cam.fx = f->camera.fx; cam.fy = f->camera.fy; cam.scale = f->camera.scale;
        return cam;
    }
    // binary PCD, FIELDS x y z rgba (what pcl::PCDWriter::write emits for PointXYZRGBA)
    static bool writePCD(const string& path, const PointCloud& c) {
        ofstream out(path, ios::binary);
        if (!out) return false;
        out << "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgba\nSIZE 4 4 4 4\nTYPE F F F U\nCOUNT 1 1 1 1\n"
            << "WIDTH " << c.points.size() << "\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS " << c.points.size() << "\nDATA binary\n";
        for (const PointT& p : c.points) { out.write((const char*)&p.x, 12); out.write((const char*)&p.b, 4); }
        return (bool)out;
    }
    // src/mapper.cpp:12-94.  Like the reference, the gated camera-frame cloud is computed ONCE per frame (moving-class mask, gated unprojection,
    // camera colour: ssm_backproject with T = NULL) and cached in frame->pointcloud (mapper.cpp:17-20); every call returns a copy transformed by the
    // frame's current pose (pcl::transformPointCloud, mapper.cpp:91: x' = float(t00 x + t01 y + t02 z + t03) in double, left to right -- the same
    // arithmetic ssm_backproject applies on the device when it is given T, so both routes give identical bits; -ffp-contract=off in host/Makefile)
    PointCloud::Ptr generatePointCloud(const RGBDFrame::Ptr& frame) {
        hostCloud(frame);
        const Eigen::Isometry3d T = mapPoseOf(frame);
        const double* t = T.data();                                            // column-major
        PointCloud::Ptr tmp(new PointCloud(*frame->pointcloud));
        for (PointT& p : tmp->points) {
            const double x = p.x, y = p.y, z = p.z;
            p.x = (float)(t[0] * x + t[4] * y + t[8] * z + t[12]);
            p.y = (float)(t[1] * x + t[5] * y + t[9] * z + t[13]);
            p.z = (float)(t[2] * x + t[6] * y + t[10] * z + t[14]);
        }
        tmp->is_dense = false;
        return tmp;
    }
    // the first half of generatePointCloud: frame->pointcloud, made once
    void hostCloud(const RGBDFrame::Ptr& frame) {
        if (frame->pointcloud == nullptr) {
            ssm::Device& d = device(frame->depth.cols, frame->depth.rows);
            const int w = frame->depth.cols, h = frame->depth.rows;
            const ssm_camera cam = cameraOf(frame);
            PointCloud::Ptr pc(new PointCloud());
            pc->points.resize((size_t)w * h);
            int n = 0;
            if (fuse_motion) {
                const ssm_motion_fuse_params P = fuseParams();
                d.check(ssm_backproject_fused(d.ctx(), frame->depth.ptr<uint16_t>(), frame->rgb.data, frame->semantic.data, motionOf(frame), w, h, &cam, nullptr, max_distance, &P,
                                              reinterpret_cast<ssm_point*>(pc->points.data()), w * h, &n), "ssm_backproject_fused");
            } else
            d.check(ssm_backproject(d.ctx(), frame->depth.ptr<uint16_t>(), frame->rgb.data, frame->semantic.data, w, h, &cam, nullptr, max_distance,
                                    reinterpret_cast<ssm_point*>(pc->points.data()), w * h, &n), "ssm_backproject");
            if (outlier_removal) {
                const ssm_sor_params P = sorParams(); ssm_sor_info I{};
                vector<ssm_point> kept((size_t)max(n, 1)); int nk = 0;
                d.check(ssm_sor_filter(d.ctx(), reinterpret_cast<const ssm_point*>(pc->points.data()), n, &P, kept.data(), (int)kept.size(), &nk, &I), "ssm_sor_filter");
                if (nk > 0) memcpy((void*)pc->points.data(), kept.data(), (size_t)nk * sizeof(ssm_point));
                n = nk;
                sorInfo[frame.get()] = I;
            }
            pc->points.resize(n); pc->points.shrink_to_fit(); pc->width = n; pc->is_dense = false;
            frame->pointcloud = pc;
            cloudsComputed++;
        }
    }
    // free-space carving: the key-frames kfs[carved ..] become views, one after the other, each of the clouds of the `carve_window` key-frames before it.  The
    // viewer thread calls this; once that has ended its owner may (the host route then: the device clouds went with the thread)
    void carveUpTo(const vector<RGBDFrame::Ptr>& kfs, size_t upto = (size_t)-1) {
        for (; carved < min(kfs.size(), upto); carved++) {
            const size_t j = carved, first = j > (size_t)max(carve_window, 0) ? j - (size_t)max(carve_window, 0) : 0;
            if (first == j) continue;
            const RGBDFrame::Ptr& vf = kfs[j];
            const int w = vf->depth.cols, h = vf->depth.rows;
            ssm::Device& d = device(w, h);
            const ssm_camera cam = cameraOf(vf);
            const Eigen::Isometry3d Tv = mapPoseOf(vf);
            const vector<RGBDFrame::Ptr> before(kfs.begin() + first, kfs.begin() + j);
            const int m = (int)(j - first);
            vector<ssm_carve_info> infos((size_t)m);
            vector<double> poses = posesOf(before);
            if (device_map) {
                CloudList L = cloudsOf(before);
                Owned<ssm_carve_view, ssm_carve_view_free> view(d.ctx());
                d.check(ssm_carve_view_create(d.ctx(), vf->depth.ptr<uint16_t>(), w, h, &cam, &view.t), "ssm_carve_view_create");
                d.check(ssm_carve(d.ctx(), view.t, Tv.data(), L.cl.data(), poses.data(), m, &carve_params, infos.data()), "ssm_carve");
            } else {
                for (size_t i = first; i < j; i++) {
                    hostCloud(kfs[i]);
                    PointCloud& pc = *kfs[i]->pointcloud;
                    const int n = (int)pc.points.size();
                    vector<uint8_t>& run = carveRun[kfs[i].get()];
                    run.resize((size_t)n, 0);
                    vector<ssm_point> kept((size_t)max(n, 1)); int nk = 0;
                    d.check(ssm_carve_points(d.ctx(), vf->depth.ptr<uint16_t>(), w, h, &cam, Tv.data(), reinterpret_cast<const ssm_point*>(pc.points.data()), n, &poses[(i - first) * 16],
                                             run.data(), &carve_params, kept.data(), (int)kept.size(), &nk, &infos[i - first]), "ssm_carve_points");
                    if (nk > 0) memcpy((void*)pc.points.data(), kept.data(), (size_t)nk * sizeof(ssm_point));
                    pc.points.resize((size_t)nk); pc.width = nk; run.resize((size_t)nk);
                }
            }
            for (size_t i = first; i < j; i++) {
                const ssm_carve_info& I = infos[i - first];
                auto it = carveInfo.find(kfs[i].get());
                if (it == carveInfo.end()) it = carveInfo.emplace(kfs[i].get(), ssm_carve_info{I.n_in, I.n_in, 0, 0, 0, 0, 0, 0}).first;
                ssm_carve_info& A = it->second;
                A.n_kept = I.n_kept; A.unknown += I.unknown; A.occluded += I.occluded; A.supported += I.supported; A.seen_through += I.seen_through; A.removed += I.removed;
            }
            carveViews++;
        }
    }
    // dense alignment: the key-frames kfs[aligned ..] are aligned, one after the other, each as the view of the clouds of the `align_window` key-frames before it at
    // their map poses.  The viewer thread calls this; once that has ended its owner may (the host route then: the device clouds went with the thread)
    void alignUpTo(const vector<RGBDFrame::Ptr>& kfs, size_t upto = (size_t)-1) {
        for (; aligned < min(kfs.size(), upto); aligned++) {
            const size_t j = aligned, first = j > (size_t)max(align_window, 0) ? j - (size_t)max(align_window, 0) : 0;
            const RGBDFrame::Ptr& vf = kfs[j];
            const Eigen::Isometry3d Pj = invert_pose ? vf->getTransform().inverse() : vf->getTransform();
            const Eigen::Isometry3d start = alignD * Pj;
            AlignResult R; R.D = alignD; R.map_pose = start; memset(&R.info, 0, sizeof R.info); R.accepted = false;
            if (first < j) {
                const int w = vf->depth.cols, h = vf->depth.rows;
                ssm::Device& d = device(w, h);
                const ssm_camera cam = cameraOf(vf);
                CloudList L = cloudsOf(vector<RGBDFrame::Ptr>(kfs.begin() + first, kfs.begin() + j));
                Owned<ssm_align_view, ssm_align_view_free> view(d.ctx());
                d.check(ssm_align_view_create(d.ctx(), vf->depth.ptr<uint16_t>(), w, h, &cam, &align_params, &view.t), "ssm_align_view_create");
                double To[16];
                if (device_map) d.check(ssm_align_clouds(d.ctx(), view.t, start.data(), L.cl.data(), L.poses.data(), L.m, &align_params, To, &R.info), "ssm_align_clouds");
                else d.check(ssm_align_points(d.ctx(), view.t, start.data(), L.pts.data(), L.n.data(), L.poses.data(), L.m, &align_params, To, &R.info), "ssm_align_points");
                R.accepted = R.info.status == SSM_ALIGN_CONVERGED || (R.info.status == SSM_ALIGN_MAX_ITER && R.info.inliers_last >= (int64_t)align_params.min_inliers);
                if (R.accepted) {
                    Eigen::Isometry3d out; for (int c = 0; c < 4; c++) for (int r = 0; r < 4; r++) out(r, c) = To[c * 4 + r];
                    R.map_pose = out; R.D = out * Pj.inverse(); alignD = R.D; alignAccepted++;
                }
            }
            alignResult[vf.get()] = R;
        }
    }
    // what the viewer does with the key-frames so far: with both switches on, key-frame by key-frame -- j is aligned against the clouds as the views before j left
    // them, then j is a carving view -- so the result does not depend on how many key-frames arrive between two updates
    void alignCarveUpTo(const vector<RGBDFrame::Ptr>& kfs) {
        if (align && carve) { for (size_t k = min(aligned, carved) + 1; k <= kfs.size(); k++) { alignUpTo(kfs, k); carveUpTo(kfs, k); } }
        else if (align) alignUpTo(kfs);
        else if (carve) carveUpTo(kfs);
    }
    struct AlignResult { Eigen::Isometry3d D, map_pose; ssm_align_info info; bool accepted; };
    bool aligns() const { return align; }
    int alignedKeyframes() const { return (int)aligned; }                    // key-frames aligned so far (the first has no earlier cloud: it keeps its pose)
    int acceptedAlignments() const { return alignAccepted; }
    // a key-frame's alignment (not while the viewer thread runs); false: not aligned yet, or the switch is off.  D: its world-frame correction D_j
    bool alignInfoOf(const RGBDFrame::Ptr& frame, ssm_align_info* info, Eigen::Isometry3d* D = nullptr, bool* accepted = nullptr) const {
        AlignResult R;
        if (!infoOf(alignResult, frame, &R)) return false;
        if (info) *info = R.info;
        if (D) *D = R.D;
        if (accepted) *accepted = R.accepted;
        return true;
    }
    // the pose the Mapper uses for a key-frame: its map pose D_j . P_j once it has been aligned, else its pose as before (mapper_invert_pose applied)
    Eigen::Isometry3d mapPoseOf(const RGBDFrame::Ptr& frame) const {
        if (align) { auto it = alignResult.find(frame.get()); if (it != alignResult.end()) return it->second.map_pose; }
        return invert_pose ? frame->getTransform().inverse() : frame->getTransform();
    }
    // map rendering: every key-frame of kfs is a view once, of the clouds of the key-frames within `render_window` of it (itself left out), compared with its own
    // depth and semantic image.  The viewer thread calls this as it ends; once that has ended its owner may (the host route then: the device clouds went with the thread)
protected:
    // a device object of the library with the context it is freed in; freed on every way out
    template <class T, void (*Free)(ssm_ctx*, T*)> struct Owned {
        ssm_ctx* ctx = nullptr; T* t = nullptr;
        explicit Owned(ssm_ctx* c = nullptr) : ctx(c) {}
        Owned(const Owned&) = delete; Owned& operator=(const Owned&) = delete;
        ~Owned() { reset(); }
        void reset() { if (t) Free(ctx, t); t = nullptr; }
    };
public:
    struct RenderTarget : Owned<ssm_render_target, ssm_render_target_free> { int w = 0, h = 0; };        // the device images, of the size of the current view
    // the rendering of view j alone: the clouds around key-frame j into the target, which is made or remade when the view has another size
    void renderView(const vector<RGBDFrame::Ptr>& kfs, size_t j, RenderTarget& target, ssm_render_info* info = nullptr) {
        const size_t win = (size_t)max(render_window, 0);
        {
            const RGBDFrame::Ptr& vf = kfs[j];
            const int w = vf->depth.cols, h = vf->depth.rows;
            ssm::Device& d = device(w, h);
            const ssm_camera cam = cameraOf(vf);
            const Eigen::Isometry3d Tv = mapPoseOf(vf);
            if (!target.t || target.w != w || target.h != h) {
                target.reset();
                target.ctx = d.ctx(); target.w = w; target.h = h;
                d.check(ssm_render_target_create(d.ctx(), w, h, &target.t), "ssm_render_target_create");
            }
            vector<RGBDFrame::Ptr> around;
            for (size_t i = j > win ? j - win : 0; i < kfs.size() && i <= j + win; i++) if (i != j) around.push_back(kfs[i]);
            CloudList L = cloudsOf(around);
            ssm_render_info R{};
            if (device_map) d.check(ssm_render_clouds(d.ctx(), target.t, &cam, Tv.data(), L.cl.data(), L.poses.data(), L.m, &render_params, &R), "ssm_render_clouds");
            else d.check(ssm_render_points(d.ctx(), target.t, &cam, Tv.data(), L.pts.data(), L.n.data(), L.poses.data(), L.m, &render_params, &R), "ssm_render_points");
            if (info) *info = R;
        }
    }
    void renderAll(const vector<RGBDFrame::Ptr>& kfs) {
        RenderTarget target;
        renderInfo.clear(); renderViews = 0;
        for (size_t j = 0; j < kfs.size(); j++) {
            renderView(kfs, j, target);
            const RGBDFrame::Ptr& vf = kfs[j];
            const int w = vf->depth.cols, h = vf->depth.rows;
            ssm::Device& d = device(w, h);
            const double scale = vf->camera.scale;
            ssm_render_compare_info I{};
            cv::Mat cls; if (!render_dir.empty()) cls.create(h, w, CV_8UC1);
            d.check(ssm_render_compare(d.ctx(), target.t, vf->depth.ptr<uint16_t>(), vf->semantic.data, scale, &render_params, &I, cls.empty() ? nullptr : cls.data), "ssm_render_compare");
            renderInfo[vf.get()] = I;
            renderViews++;
            if (!render_dir.empty()) {
                cv::Mat dep, bgr, lab, col;
                dep.create(h, w, CV_16UC1); bgr.create(h, w, CV_8UC3); lab.create(h, w, CV_8UC1); col.create(h, w, CV_8UC3);
                d.check(ssm_render_fetch(d.ctx(), target.t, dep.ptr<uint16_t>(), bgr.data, lab.data, nullptr), "ssm_render_fetch");
                ssm_render_label_colours(lab.data, (int64_t)w * h, col.data);
                char stem[32]; snprintf(stem, sizeof stem, "/render_%06d", (int)j);
                const string base = render_dir + stem;
                if (!(ssm::imwritePNG(base + "_depth.png", dep) && ssm::imwritePNG(base + "_bgr.png", bgr) && ssm::imwritePNG(base + "_label.png", col) && ssm::imwritePNG(base + "_class.png", cls)))
                    throw std::runtime_error("Mapper: cannot write the rendered images to " + render_dir);
            }
        }
    }
    bool rendersViews() const { return render; }
    int renderedViews() const { return renderViews; }                        // views rendered by the last renderAll
    // the comparison of the rendering into a key-frame's view with the frame's own images (not while the viewer thread runs); false: not rendered, or the switch is off
    bool renderInfoOf(const RGBDFrame::Ptr& frame, ssm_render_compare_info* info) const { return infoOf(renderInfo, frame, info); }
    // the ground grid: ONE grid of the clouds of every key-frame of kfs at their map poses.  The viewer thread calls this as it ends; once that has ended its owner
    // may (the host route then: the device clouds went with the thread)
    struct GridInfo { bool built = false, skipped = false; ssm_grid_info counts{}; };          // skipped: the extent exceeded 2^24 cells (or there was no key-frame)
    typedef Owned<ssm_grid_target, ssm_grid_target_free> GridTarget;          // the device accumulators and outputs
    void buildGrid(const vector<RGBDFrame::Ptr>& kfs) {
        objectsState = ObjectsInfo(); objectRecords.clear(); objectIds.clear();
        clearanceState = ClearanceInfo(); clearanceD2.clear(); clearanceNearest.clear(); clearanceReach.clear();
        routeState = RouteInfo(); routeCost.clear(); routeParent.clear(); routeCells.clear();
        gridState = GridInfo(); gridSpec = grid_params; gridSpec.nx = gridSpec.ny = 0;
        gridCls.clear(); gridGroundLabel.clear(); gridObstacleLabel.clear(); gridGroundQ.clear(); gridTopQ.clear(); gridN.clear(); gridNHigh.clear();
        if (kfs.empty()) { gridState.skipped = true; return; }
        // the extent: the key-frames' map positions in the grid frame, widened by max_distance, in whole cells
        ssm_grid_params P = grid_params;
        double lo[2] = {HUGE_VAL, HUGE_VAL}, hi[2] = {-HUGE_VAL, -HUGE_VAL};
        for (const RGBDFrame::Ptr& f : kfs) {
            const Eigen::Isometry3d T = mapPoseOf(f);
            for (int i = 0; i < 2; i++) {
                const double g = ((P.G[i * 4] * T(0, 3) + P.G[i * 4 + 1] * T(1, 3)) + P.G[i * 4 + 2] * T(2, 3)) + P.G[i * 4 + 3];
                lo[i] = min(lo[i], g); hi[i] = max(hi[i], g);
            }
        }
        const double cx0 = floor((lo[0] - max_distance) / P.cell), cx1 = ceil((hi[0] + max_distance) / P.cell), cy0 = floor((lo[1] - max_distance) / P.cell),
                     cy1 = ceil((hi[1] + max_distance) / P.cell);
        const double nxd = max(cx1 - cx0, 1.0), nyd = max(cy1 - cy0, 1.0);
        if (!(nxd * nyd <= 16777216.0) || !std::isfinite(cx0) || !std::isfinite(cy0)) {          // (false for NaN too)
            cerr << "Mapper: the ground grid would have " << nxd << " x " << nyd << " cells, more than 2^24: not built" << endl;
            gridState.skipped = true; return;
        }
        P.x0 = cx0 * P.cell; P.y0 = cy0 * P.cell; P.nx = (int)nxd; P.ny = (int)nyd;
        const int w = kfs[0]->depth.cols, h = kfs[0]->depth.rows;
        ssm::Device& d = device(w, h);
        GridTarget target(d.ctx());
        d.check(ssm_grid_target_create(d.ctx(), P.nx, P.ny, &target.t), "ssm_grid_target_create");
        ssm_grid_info I{};
        CloudList L = cloudsOf(kfs);          // (the poses are those the extent was made from: nothing moved them in between)
        if (device_map) d.check(ssm_grid_clouds(d.ctx(), target.t, L.cl.data(), L.poses.data(), L.m, &P, &I), "ssm_grid_clouds");
        else d.check(ssm_grid_points(d.ctx(), target.t, L.pts.data(), L.n.data(), L.poses.data(), L.m, &P, &I), "ssm_grid_points");
        const size_t nc = (size_t)P.nx * P.ny;
        gridCls.resize(nc); gridGroundLabel.resize(nc); gridObstacleLabel.resize(nc); gridGroundQ.resize(nc); gridTopQ.resize(nc); gridN.resize(nc); gridNHigh.resize(nc);
        d.check(ssm_grid_fetch(d.ctx(), target.t, gridCls.data(), gridGroundLabel.data(), gridObstacleLabel.data(), gridGroundQ.data(), gridTopQ.data(), gridN.data(), gridNHigh.data()),
                "ssm_grid_fetch");
        gridSpec = P; gridState.counts = I; gridState.built = true;
        if (objects) extractObjects(d, target.t, L, P);
        if (clearance || route) mapClearance(d, target.t, P, mapPoseOf(kfs.back()));          // (the route field has the clearance map built for it, which then writes no file)
        if ((grid || !(objects || clearance || route)) && !grid_dir.empty()) {          // (a grid built only for the objects, the clearance map or the route field writes no grid files)
            cv::Mat col, hgt; col.create(P.ny, P.nx, CV_8UC3); hgt.create(P.ny, P.nx, CV_16UC1);
            ssm_grid_colours(gridCls.data(), gridGroundLabel.data(), gridObstacleLabel.data(), gridGroundQ.data(), P.nx, P.ny, P.h_min, col.data, hgt.ptr<uint16_t>());
            ofstream txt(grid_dir + "/grid.txt");
            txt << setprecision(17) << "x0 " << P.x0 << "\ny0 " << P.y0 << "\ncell " << P.cell << "\nnx " << P.nx << "\nny " << P.ny << "\nh_min " << P.h_min << "\nG";
            for (int i = 0; i < 12; i++) txt << " " << P.G[i];
            txt << "\n";
            txt.close();
            if (!(txt && ssm::imwritePNG(grid_dir + "/grid_colour.png", col) && ssm::imwritePNG(grid_dir + "/grid_height.png", hgt)))
                throw std::runtime_error("Mapper: cannot write the ground grid to " + grid_dir);
        }
    }
    bool buildsGrid() const { return grid; }
    // object extraction: both stages on the grid target buildGrid has just built and the cloud list it was built from (the same clouds at the same poses)
    struct ObjectsInfo { bool built = false; ssm_objects_info counts{}; };
    typedef Owned<ssm_objects_target, ssm_objects_target_free> ObjectsTarget;
    static const char* labelName(int l) {
        static const char* names[12] = {"Sky", "Building", "Pole", "Road_Marking", "Road", "Pavement", "Tree", "Sign_Symbol", "Fence", "Vehicle", "Pedestrian", "Bike"};
        return l >= 0 && l < 12 ? names[l] : "Unknown";
    }
    template <class List /* CloudList, declared below */> void extractObjects(ssm::Device& d, ssm_grid_target* grid_target, const List& L, const ssm_grid_params& P) {
        ObjectsTarget target(d.ctx());
        d.check(ssm_objects_target_create(d.ctx(), P.nx, P.ny, &target.t), "ssm_objects_target_create");
        ssm_objects_info I{};
        d.check(ssm_objects_grid(d.ctx(), grid_target, &objects_params, target.t, &I), "ssm_objects_grid");
        if (device_map) d.check(ssm_objects_clouds(d.ctx(), grid_target, target.t, L.cl.data(), L.poses.data(), L.m, &I), "ssm_objects_clouds");
        else d.check(ssm_objects_points(d.ctx(), grid_target, target.t, L.pts.data(), L.n.data(), L.poses.data(), L.m, nullptr, &I), "ssm_objects_points");
        int K = 0;
        d.check(ssm_objects_fetch(d.ctx(), target.t, nullptr, 0, &K, nullptr), "ssm_objects_fetch");
        objectRecords.resize((size_t)K); objectIds.resize((size_t)P.nx * P.ny);
        d.check(ssm_objects_fetch(d.ctx(), target.t, objectRecords.data(), K, &K, objectIds.data()), "ssm_objects_fetch");
        objectsState.counts = I; objectsState.built = true;
        if (!objects_dir.empty()) {
            ofstream txt(objects_dir + "/objects.txt");
            txt << setprecision(17);
            for (int k = 0; k < K; k++) {
                const ssm_object& o = objectRecords[(size_t)k];
                const double n = o.n_points ? (double)o.n_points : 1.0;
                txt << k << " " << labelName(o.label) << " " << o.cells << " " << o.n_points << " " << o.x_min_q / 1024.0 << " " << o.x_max_q / 1024.0 << " " << o.y_min_q / 1024.0 << " "
                    << o.y_max_q / 1024.0 << " " << o.z_min_q / 1024.0 << " " << o.z_max_q / 1024.0 << " " << (double)o.sum_x / n / 1024.0 << " " << (double)o.sum_y / n / 1024.0 << " "
                    << (double)o.sum_z / n / 1024.0 << " " << o.ground_q / 1024.0 << " " << o.top_q / 1024.0 << "\n";
            }
            txt.close();
            cv::Mat img; img.create(P.ny, P.nx, CV_16UC1);
            for (int r = 0; r < P.ny; r++) for (int x = 0; x < P.nx; x++) {
                const int32_t id = objectIds[(size_t)(P.ny - 1 - r) * P.nx + x];
                img.ptr<uint16_t>(r)[x] = (uint16_t)(id < 0 ? 0 : min(id + 1, 65535));
            }
            if (!(txt && ssm::imwritePNG(objects_dir + "/objects_id.png", img))) throw std::runtime_error("Mapper: cannot write the objects to " + objects_dir);
        }
    }
    bool extractsObjects() const { return objects; }
    // the clearance map of the grid buildGrid has just built, on the same grid target; camera: the map pose of the last key-frame, whose centre is the seed
    struct ClearanceInfo { bool built = false; int32_t seed_cx = -1, seed_cy = -1; ssm_clearance_info counts{}; };          // seed_cx, seed_cy: the camera's cell (-1, -1: outside the grid)
    typedef Owned<ssm_clearance_target, ssm_clearance_target_free> ClearanceTarget;
    void mapClearance(ssm::Device& d, ssm_grid_target* grid_target, const ssm_grid_params& P, const Eigen::Isometry3d& camera) {
        ssm_clearance_params C = clearance_params;
        double g[2];
        for (int i = 0; i < 2; i++) g[i] = ((P.G[i * 4] * camera(0, 3) + P.G[i * 4 + 1] * camera(1, 3)) + P.G[i * 4 + 2] * camera(2, 3)) + P.G[i * 4 + 3];
        if (!ssm_clrc::cell_of(P, g[0], g[1], &C.seed_cx, &C.seed_cy)) C.seed_cx = C.seed_cy = -1;
        ClearanceTarget target(d.ctx());
        d.check(ssm_clearance_target_create(d.ctx(), P.nx, P.ny, &target.t), "ssm_clearance_target_create");
        ssm_clearance_info I{};
        d.check(ssm_clearance_grid(d.ctx(), grid_target, &C, target.t, &I), "ssm_clearance_grid");
        const size_t nc = (size_t)P.nx * P.ny;
        clearanceD2.resize(nc); clearanceNearest.resize(nc); clearanceReach.resize(nc);
        d.check(ssm_clearance_fetch(d.ctx(), target.t, clearanceD2.data(), clearanceNearest.data(), clearanceReach.data()), "ssm_clearance_fetch");
        clearanceState.counts = I; clearanceState.seed_cx = C.seed_cx; clearanceState.seed_cy = C.seed_cy; clearanceState.built = true;
        if (route) mapRoute(d, target.t, P);          // (while the clearance target lives: the field reads it on the device)
        if (clearance && !clearance_dir.empty()) {
            cv::Mat cm, rm; cm.create(P.ny, P.nx, CV_16UC1); rm.create(P.ny, P.nx, CV_8UC1);
            for (int r = 0; r < P.ny; r++) for (int x = 0; x < P.nx; x++) {
                const size_t i = (size_t)(P.ny - 1 - r) * P.nx + x;
                const uint32_t d2 = clearanceD2[i];
                const double v = d2 == UINT32_MAX ? 65535.0 : floor(sqrt((double)d2) * P.cell * 100.0);
                cm.ptr<uint16_t>(r)[x] = (uint16_t)(v < 65535.0 ? v : 65535.0);
                rm.ptr<uint8_t>(r)[x] = (uint8_t)(clearanceReach[i] == 2 ? 255 : clearanceReach[i] == 1 ? 128 : 0);
            }
            ofstream txt(clearance_dir + "/clearance.txt");
            txt << "blocked " << I.blocked << "\nfree_cells " << I.free_cells << "\ntraversable " << I.traversable << "\ncomponents " << I.components << "\nreachable " << I.reachable
                << "\nseed_cell " << I.seed_cell << "\nmax_d2_reachable " << I.max_d2_reachable << "\nr2 " << I.r2 << "\n";
            txt.close();
            if (!(txt && ssm::imwritePNG(clearance_dir + "/clearance.png", cm) && ssm::imwritePNG(clearance_dir + "/reach.png", rm)))
                throw std::runtime_error("Mapper: cannot write the clearance map to " + clearance_dir);
        }
    }
    // mapper_route=1 (default 0: nothing of this runs, every cloud, map, grid, object, clearance result, file and figure exactly as before): the route field
    // (the reference has no such step) over the clearance map mapClearance has just made, on the device (ssm_route_field), then ONE path: to the cell
    // of (mapper_route_goal_x, _goal_y), metres in the grid frame, through ssm_clrc::cell_of -- a goal outside the grid is refused -- or, without a goal, to
    // far_cell, the farthest place the vehicle can drive to.  mapper_route_moves (8), _near_weight (2), _comfort (2.0 m), _goal_snap (10 cells), _max_path
    // (4 (nx + ny)).  routeInfo(), routePathInfo(), routeFetch(cost, parent), routePath(); with mapper_route_dir set the call writes route.png (8 bit: reach.png's
    // values with the path's cells at 64), route_cost.png (16 bit: min(65534, cost), 65535 for no cost) and route.txt (both infos as `name value` lines, then one
    // `cx cy` per path cell); image row r is cell row ny - 1 - r as in the grid's images
    struct RouteInfo { bool built = false; int32_t goal_cx = -1, goal_cy = -1; ssm_route_info counts{}; ssm_route_path_info path{}; };          // goal_cx, goal_cy: the goal asked for (-1, -1: nothing routed)
    typedef Owned<ssm_route_target, ssm_route_target_free> RouteTarget;
    void mapRoute(ssm::Device& d, ssm_clearance_target* clearance_target, const ssm_grid_params& P) {
        const int max_path = route_max_path > 0 ? route_max_path : 4 * (P.nx + P.ny);
        RouteTarget target(d.ctx());
        d.check(ssm_route_target_create(d.ctx(), P.nx, P.ny, max_path, &target.t), "ssm_route_target_create");
        ssm_route_info I{};
        d.check(ssm_route_field(d.ctx(), clearance_target, &route_params, target.t, &I), "ssm_route_field");
        const size_t nc = (size_t)P.nx * P.ny;
        routeCost.resize(nc); routeParent.resize(nc);
        d.check(ssm_route_fetch(d.ctx(), target.t, routeCost.data(), routeParent.data()), "ssm_route_fetch");
        int32_t gx = -1, gy = -1, snap = route_goal_snap;
        if (route_has_goal) { if (!ssm_clrc::cell_of(P, route_goal_x, route_goal_y, &gx, &gy)) throw std::runtime_error("Mapper: mapper_route_goal_x, _goal_y lie outside the grid"); }
        else if (I.far_cell >= 0) { gx = (int32_t)(I.far_cell % P.nx); gy = (int32_t)(I.far_cell / P.nx); snap = 0; }
        ssm_route_path_info PI{}; PI.goal_cell = -1; PI.cost = -1; PI.min_d2 = -1;
        routeCells.assign((size_t)min<int64_t>(max_path, (int64_t)nc), -1);
        if (gx >= 0) {
            d.check(ssm_route_path(d.ctx(), target.t, gx, gy, snap, routeCells.data(), &PI), "ssm_route_path");
            routeCells.resize((size_t)PI.len);
        } else routeCells.clear();
        routeState.counts = I; routeState.path = PI; routeState.goal_cx = gx; routeState.goal_cy = gy; routeState.built = true;
        if (!route_dir.empty()) {
            cv::Mat rm, cm; rm.create(P.ny, P.nx, CV_8UC1); cm.create(P.ny, P.nx, CV_16UC1);
            vector<uint8_t> on(nc, 0);
            for (int32_t c : routeCells) on[(size_t)c] = 1;
            for (int r = 0; r < P.ny; r++) for (int x = 0; x < P.nx; x++) {
                const size_t i = (size_t)(P.ny - 1 - r) * P.nx + x;
                rm.ptr<uint8_t>(r)[x] = (uint8_t)(on[i] ? 64 : clearanceReach[i] == 2 ? 255 : clearanceReach[i] == 1 ? 128 : 0);
                cm.ptr<uint16_t>(r)[x] = (uint16_t)(routeCost[i] == UINT32_MAX ? 65535u : min<uint32_t>(65534u, routeCost[i]));
            }
            ofstream txt(route_dir + "/route.txt");
            txt << "routed " << I.routed << "\nunrouted " << I.unrouted << "\nnear_cells " << I.near_cells << "\nmax_cost " << I.max_cost << "\nfar_cell " << I.far_cell << "\nsource_cell "
                << I.source_cell << "\ncomfort2 " << I.comfort2 << "\nmoves " << I.moves << "\nlen " << PI.len << "\ngoal_cell " << PI.goal_cell << "\ncost " << PI.cost << "\nn_axial "
                << PI.n_axial << "\nn_diag " << PI.n_diag << "\nnear_steps " << PI.near_steps << "\nmin_d2 " << PI.min_d2 << "\n";
            for (int32_t c : routeCells) txt << c % P.nx << " " << c / P.nx << "\n";
            txt.close();
            if (!(txt && ssm::imwritePNG(route_dir + "/route.png", rm) && ssm::imwritePNG(route_dir + "/route_cost.png", cm)))
                throw std::runtime_error("Mapper: cannot write the route field to " + route_dir);
        }
    }
    bool mapsRoute() const { return route; }
    // the last mapRoute (not while the viewer thread runs): the goal, both infos; the field of the grid gridParams() describes; the path's cells, source first
    const RouteInfo& routeInfo() const { return routeState; }
    const ssm_route_path_info& routePathInfo() const { return routeState.path; }
    bool routeFetch(vector<uint32_t>* cost, vector<int32_t>* parent) const {
        if (!routeState.built) return false;
        if (cost) *cost = routeCost;
        if (parent) *parent = routeParent;
        return true;
    }
    const vector<int32_t>& routePath() const { return routeCells; }
    bool mapsClearance() const { return clearance; }
    // the last mapClearance (not while the viewer thread runs): what happened, the seed and the counts; the images of the grid gridParams() describes
    const ClearanceInfo& clearanceInfo() const { return clearanceState; }
    bool clearanceFetch(vector<uint32_t>* dist2, vector<int32_t>* nearest, vector<uint8_t>* reach) const {
        if (!clearanceState.built) return false;
        if (dist2) *dist2 = clearanceD2;
        if (nearest) *nearest = clearanceNearest;
        if (reach) *reach = clearanceReach;
        return true;
    }
    // the last extractObjects (not while the viewer thread runs): what happened and the counts; the records and the object_id image of the grid gridParams() describes
    const ObjectsInfo& objectsInfo() const { return objectsState; }
    bool objectsFetch(vector<ssm_object>* records, vector<int32_t>* object_id) const {
        if (!objectsState.built) return false;
        if (records) *records = objectRecords;
        if (object_id) *object_id = objectIds;
        return true;
    }
    // the last buildGrid (not while the viewer thread runs): what happened and the counts; the spec actually used (nx = ny = 0 when nothing was built); the arrays,
    // nx ny entries each, cell (cx, cy) at cy nx + cx -- each pointer may be null; false: nothing was built
    const GridInfo& gridInfo() const { return gridState; }
    const ssm_grid_params& gridParams() const { return gridSpec; }
    bool gridFetch(vector<uint8_t>* cls, vector<uint8_t>* ground_label, vector<uint8_t>* obstacle_label, vector<int32_t>* ground_q, vector<int32_t>* top_q, vector<uint32_t>* n,
                   vector<uint32_t>* n_high) const {
        if (!gridState.built) return false;
        if (cls) *cls = gridCls;
        if (ground_label) *ground_label = gridGroundLabel;
        if (obstacle_label) *obstacle_label = gridObstacleLabel;
        if (ground_q) *ground_q = gridGroundQ;
        if (top_q) *top_q = gridTopQ;
        if (n) *n = gridN;
        if (n_high) *n_high = gridNHigh;
        return true;
    }
    // label fusion: every key-frame's cloud, once, in ascending order, under the key-frames around it (their images, at the map poses).  The viewer thread calls
    // this as it ends; once that has ended its owner may (the host route then: the device clouds went with the thread)
    void relabelAll(const vector<RGBDFrame::Ptr>& kfs) {
        relabelInfo.clear(); relabelled = 0; relabelFnv = relabel_hash ? 0xCBF29CE484222325ull : 0;
        if (kfs.empty()) return;
        const size_t n = kfs.size(), win = (size_t)max(relabel_window, 0);
        ssm::Device& d = device(kfs[0]->depth.cols, kfs[0]->depth.rows);
        std::map<size_t, Owned<ssm_relabel_view, ssm_relabel_view_free>> views;          // the view objects alive
        for (size_t i = 0; i < n; i++) {
            const size_t first = i > win ? i - win : 0, last = min(n - 1, i + win);
            views.erase(views.begin(), views.lower_bound(first));          // a view below the window of cloud i is below that of every later cloud
            vector<const ssm_relabel_view*> list; vector<double> poses;
            for (size_t j = first; j <= last; j++) {
                if (j == i) continue;
                auto& view = views[j];
                if (!view.t) {
                    const RGBDFrame::Ptr& f = kfs[j];
                    const ssm_camera cam = cameraOf(f);
                    view.ctx = d.ctx();
                    d.check(ssm_relabel_view_create(d.ctx(), f->depth.ptr<uint16_t>(), f->semantic.data, f->depth.cols, f->depth.rows, &cam, &view.t), "ssm_relabel_view_create");
                }
                list.push_back(view.t);
                const Eigen::Isometry3d T = mapPoseOf(kfs[j]);
                poses.insert(poses.end(), T.data(), T.data() + 16);
            }
            relabelViewsAlive = max(relabelViewsAlive, (int)views.size());
            const Eigen::Isometry3d Tc = mapPoseOf(kfs[i]);
            ssm_relabel_info I{};
            if (device_map) {
                d.check(ssm_relabel(d.ctx(), list.data(), poses.data(), (int)list.size(), deviceCloud(kfs[i]), Tc.data(), &relabel_params, &I), "ssm_relabel");
            } else {
                hostCloud(kfs[i]);
                PointCloud& pc = *kfs[i]->pointcloud;
                const int np = (int)pc.points.size();
                vector<uint32_t> lab((size_t)max(np, 1));
                ssm_point* pts = reinterpret_cast<ssm_point*>(pc.points.data());
                d.check(ssm_relabel_points(d.ctx(), list.data(), poses.data(), (int)list.size(), pts, np, Tc.data(), &relabel_params, lab.data(), &I), "ssm_relabel_points");
                for (int k = 0; k < np; k++) pts[k].label = lab[(size_t)k];
            }
            if (relabel_hash) {          // the labels as they are now (the device route: one fetch of the cloud), only when somebody reads the hash
                vector<ssm_point> now((size_t)max(I.n_in, 1)); int got = 0;
                if (device_map) d.check(ssm_cloud_fetch(d.ctx(), deviceCloud(kfs[i]), nullptr, now.data(), (int)now.size(), &got), "ssm_cloud_fetch");
                else { got = I.n_in; if (got) memcpy((void*)now.data(), kfs[i]->pointcloud->points.data(), (size_t)got * sizeof(ssm_point)); }
                for (int k = 0; k < got; k++) {
                    const unsigned char* b = (const unsigned char*)&now[(size_t)k].label;
                    for (int q = 0; q < 4; q++) { relabelFnv ^= b[q]; relabelFnv *= 0x100000001B3ull; }
                }
            }
            relabelInfo[kfs[i].get()] = I;
            relabelled++;
        }
    }
    bool relabels() const { return relabel; }
    int relabelledKeyframes() const { return relabelled; }                    // clouds relabelled by the last relabelAll
    uint64_t relabelLabelFnv() const { return relabelFnv; }                    // mapper_relabel_hash=1: FNV-1a over every key-frame's label bytes after the last relabelAll, in order; else 0
    int relabelMaxViewsAlive() const { return relabelViewsAlive; }            // the most view objects alive at once so far (2 window + 1 at most)
    // what label fusion did to a key-frame's cloud (not while the viewer thread runs); false: relabelAll has not reached it, or the switch is off
    bool relabelInfoOf(const RGBDFrame::Ptr& frame, ssm_relabel_info* info) const { return infoOf(relabelInfo, frame, info); }
    bool carves() const { return carve; }
    int carvedViews() const { return carveViews; }                            // views applied so far (a first key-frame has no earlier cloud and is none)
    // what carving did to a key-frame's cloud over all the views applied to it: n_in its size before the first, n_kept its size now, the verdicts and `removed` summed
    // (not while the viewer thread runs); false: no view has been applied to it, or the switch is off
    bool carveInfoOf(const RGBDFrame::Ptr& frame, ssm_carve_info* info) const { return infoOf(carveInfo, frame, info); }
    // src/mapper.cpp:189-271 under its own name: the mask that gates the frame's cloud.  motion_semantic_fuse=0: the always-moving classes, dilated (what
    // ssm_moving_mask gives); 1: fused with frame->moving_mask.  info: the fusion's counters.  Uses the Mapper's device: not while the viewer thread runs
    cv::Mat semantic_motion_fuse(const RGBDFrame::Ptr& frame, ssm_motion_fuse_info* info = nullptr) {
        const int w = frame->semantic.cols, h = frame->semantic.rows;
        ssm::Device& d = device(w, h);
        cv::Mat mask; mask.create(h, w, CV_8UC1);
        const ssm_motion_fuse_params P = fuseParams();
        d.check(ssm_motion_fuse(d.ctx(), frame->semantic.data, fuse_motion ? motionOf(frame) : nullptr, w, h, w * 3, &P, mask.data, info), "ssm_motion_fuse");
        return mask;
    }
    bool fusesMotion() const { return fuse_motion; }
    bool removesOutliers() const { return outlier_removal; }
    // the filter's figures for a key-frame whose cloud has been made (either route; not while the viewer thread runs); false: no cloud yet, or the switch is off
    bool sorInfoOf(const RGBDFrame::Ptr& frame, ssm_sor_info* info) const { return infoOf(sorInfo, frame, info); }
    std::atomic<bool> viewerFailed{false};
    std::atomic<bool> deviceMapFellBack{false};                              // the device-resident map update failed once: host path since (same bits)
    int cloudsComputed = 0;                                                    // device back-projections so far (each frame costs one)
    PointCloud::Ptr voxelFilter(const PointCloud::Ptr& in) {                  // pcl::VoxelGrid::filter, mapper.cpp:154-155
        PointCloud::Ptr out(new PointCloud());
        if (in->points.empty()) return out;
        ssm::Device& d = device(0, 0);
        out->points.resize(in->points.size());
        int n = 0;
        int rc = ssm_voxel_filter(d.ctx(), reinterpret_cast<const ssm_point*>(in->points.data()), (int)in->points.size(), (float)resolution,
                                  reinterpret_cast<ssm_point*>(out->points.data()), (int)out->points.size(), &n);
        if (rc == SSM_E_VOXEL_RANGE) { *out = *in; return out; }              // PCL: "Leaf size is too small ..." -> output = input
        d.check(rc, "ssm_voxel_filter");
        out->points.resize(n); out->width = n;
        return out;
    }
protected:
    vector<RGBDFrame::Ptr> keyframesNow() { unique_lock<mutex> lck(poseGraph.keyframes_mutex); return poseGraph.keyframes; }
    template <class Map, class Info> static bool infoOf(const Map& m, const RGBDFrame::Ptr& frame, Info* info) {
        auto it = m.find(frame.get());
        if (it == m.end()) return false;
        if (info) *info = it->second;
        return true;
    }
    // the clouds of some key-frames as a library call takes them: handles (the device route) or arrays and counts (the host route), and the m map poses
    struct CloudList { vector<ssm_cloud*> cl; vector<const ssm_point*> pts; vector<int32_t> n; vector<double> poses; int m = 0; };
    vector<double> posesOf(const vector<RGBDFrame::Ptr>& fs) const {           // the map poses of these key-frames as 16 m doubles, read now
        vector<double> poses;
        for (const RGBDFrame::Ptr& f : fs) { const Eigen::Isometry3d T = mapPoseOf(f); poses.insert(poses.end(), T.data(), T.data() + 16); }
        return poses;
    }
    // by the Mapper's current route: the poses read first, then the clouds made on demand, in the order given
    CloudList cloudsOf(const vector<RGBDFrame::Ptr>& fs) {
        CloudList L; L.poses = posesOf(fs); L.m = (int)fs.size();
        for (const RGBDFrame::Ptr& f : fs) {
            if (device_map) L.cl.push_back(deviceCloud(f));
            else { hostCloud(f); L.pts.push_back(reinterpret_cast<const ssm_point*>(f->pointcloud->points.data())); L.n.push_back((int32_t)f->pointcloud->points.size()); }
        }
        return L;
    }
    ssm_sor_params sorParams() const { ssm_sor_params P; ssm_sor_params_default(&P); P.mean_k = sor_mean_k; P.stddev_mul = sor_stddev; return P; }
    ssm_motion_fuse_params fuseParams() const { ssm_motion_fuse_params P; ssm_motion_fuse_params_default(&P); P.area_thres = area_thres; P.overlay_thres = overlay_portion_thres; return P; }
    // the frame's motion mask when UVDisparity left one of the semantic image's size (packed rows), else none
    static const uint8_t* motionOf(const RGBDFrame::Ptr& f) {
        const cv::Mat& m = f->moving_mask;
        return (!m.empty() && m.cols == f->semantic.cols && m.rows == f->semantic.rows && m.isContinuous()) ? m.data : nullptr;
    }
    ssm::Device& device(int w, int h) {
        if (!dev) { if (w == 0) { w = 640; h = 480; } dev.reset(new ssm::Device(parameterReader.deviceConfig(w, h))); }
        return *dev;
    }
    shared_ptr<thread> viewerThread = nullptr;
    const ParameterReader& parameterReader;
    PoseGraph& poseGraph;
    unique_ptr<ssm::Device> dev;
    PointCloud::Ptr globalMap; mutex mapMutex;
    int keyframe_size = 0; std::atomic<int> cntGlobalUpdate{0};       // read by other threads (updates()): atomic -- the reference's plain int is a data race
    double resolution = 0.8, max_distance = 8.0;
    std::atomic<bool> shutdownFlag{false};                           // set by shutdown() on another thread (ThreadSanitizer finding, profiles/r03_sanitizers.log)
    bool fix_incremental = false, invert_pose = false, device_map = true, fuse_motion = false; int test_fail_update = -1;
    std::unordered_map<const RGBDFrame*, ssm_cloud*> devClouds;       // key-frame -> its camera-frame cloud in device memory (held until the viewer ends)
    int area_thres = 1000; double overlay_portion_thres = 0.143;
    bool outlier_removal = false; int sor_mean_k = 30; double sor_stddev = 1.0;
    bool carve = false; int carve_window = 5; ssm_carve_params carve_params{}; size_t carved = 0; int carveViews = 0;
    std::unordered_map<const RGBDFrame*, vector<uint8_t>> carveRun;      // host route: the run counters beside frame->pointcloud
    std::unordered_map<const RGBDFrame*, ssm_carve_info> carveInfo;      // key-frame -> what the views did to its cloud (viewer thread, or its owner once that has ended)
    bool align = false; int align_window = 5, alignAccepted = 0; ssm_align_params align_params{}; size_t aligned = 0;
    Eigen::Isometry3d alignD = Eigen::Isometry3d::Identity();            // D_prev: the last accepted world-frame correction
    std::unordered_map<const RGBDFrame*, AlignResult> alignResult;       // key-frame -> its alignment and map pose (viewer thread, or its owner once that has ended)
    bool render = false; int render_window = 5, renderViews = 0; string render_dir; ssm_render_params render_params{};
    std::unordered_map<const RGBDFrame*, ssm_render_compare_info> renderInfo;      // key-frame -> its view's comparison (viewer thread, or its owner once that has ended)
    bool relabel = false; int relabel_window = 5, relabelled = 0, relabelViewsAlive = 0; ssm_relabel_params relabel_params{}; bool relabel_hash = false; uint64_t relabelFnv = 0;
    std::unordered_map<const RGBDFrame*, ssm_relabel_info> relabelInfo;  // key-frame -> what the views did to its labels (viewer thread, or its owner once that has ended)
    bool clearance = false; string clearance_dir; ssm_clearance_params clearance_params{}; ClearanceInfo clearanceState;
    bool route = false, route_has_goal = false; string route_dir; ssm_route_params route_params{}; int route_goal_snap = 10, route_max_path = 0; double route_goal_x = 0, route_goal_y = 0;
    RouteInfo routeState; vector<uint32_t> routeCost; vector<int32_t> routeParent, routeCells;      // the last mapRoute's field and path
    vector<uint32_t> clearanceD2; vector<int32_t> clearanceNearest; vector<uint8_t> clearanceReach;      // the last mapClearance's images
    bool objects = false; string objects_dir; ssm_objects_params objects_params{}; ObjectsInfo objectsState; vector<ssm_object> objectRecords; vector<int32_t> objectIds;
    bool grid = false; string grid_dir; ssm_grid_params grid_params{}, gridSpec{}; GridInfo gridState;
    vector<uint8_t> gridCls, gridGroundLabel, gridObstacleLabel; vector<int32_t> gridGroundQ, gridTopQ; vector<uint32_t> gridN, gridNHigh;      // the last build's arrays
    std::unordered_map<const RGBDFrame*, ssm_sor_info> sorInfo;          // key-frame -> what the filter did to its cloud (viewer thread, or its owner once that has ended)
    string map_output;
};
}  // namespace rgbd_tutor
