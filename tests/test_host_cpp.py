"""The C++ host layer (include/ssm/*.h: the reference's class names over the C ABI) and the exp_mapping driver."""
import os
import subprocess
import sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "semantic_slam_mapping_amd", "host")


def test_host_layer_builds_and_keeps_reference_names():
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL)
    assert os.path.exists(os.path.join(HOST, "exp_mapping")) and os.path.exists(os.path.join(HOST, "test_host"))
    inc = os.path.join(ROOT, "include", "ssm")
    # same class / method names and argument order as the reference headers (SURVEY.md s.8b "signatures to keep")
    want = {
        "orb.h": ["class OrbFeature", "OrbFeature(const ParameterReader& para)", "void detectFeatures(RGBDFrame::Ptr& frame) const",
                  "vector<cv::DMatch> match(const RGBDFrame::Ptr& frame1, const RGBDFrame::Ptr& frame2) const"],
        "track.h": ["class Tracker", "Tracker(const ParameterReader& para, VisualOdometryStereo::parameters param)",
                    "Eigen::Isometry3d updateFrame(RGBDFrame::Ptr& newFrame)", "trackerState getState() const", "bool adjust(const RGBDFrame::Ptr& ref)"],
        "mapper.h": ["class Mapper", "Mapper(const ParameterReader& para, PoseGraph& graph)", "void shutdown()", "void viewer()", "void SaveMap()",
                     "PointCloud::Ptr generatePointCloud(const RGBDFrame::Ptr& frame)"],
        "rgbdframe.h": ["class RGBDFrame", "cv::Point3f project2dTo3d(int u, int v) const", "cv::Mat getAllDescriptors() const",
                        "void setTransform(const Eigen::Isometry3d& T)", "Eigen::Isometry3d getTransform()", "class FrameReader", "RGBDFrame::Ptr next()"],
        "pose_graph.h": ["bool tryInsertKeyFrame(RGBDFrame::Ptr& frame)", "vector<RGBDFrame::Ptr> keyframes"],
        "parameter_reader.h": ["class ParameterReader", "T getData(const string& key) const", "CAMERA_INTRINSIC_PARAMETERS getCamera() const"],
        "quadmatcher.hpp": ["class QuadFeatureMatch", "void init(int detector_type, int descriptor_type)", "void detectFeature()", "void extractDescriptor()",
                            "void circularMatching()", "vector<pmatch> quadmatches", "struct pmatch"],
        "segnet.h": ["class Classifier", "Classifier()", "std::vector<Prediction> Classify(const cv::Mat& img, int N = 1)"],
        "vo_stereo.hpp": ["class VisualOdometry", "class VisualOdometryStereo : public VisualOdometry", "bool Process(QuadFeatureMatch& quadmatcher)", "cv::Mat getMotion()",
                          "int getNumberOfInliers()", "std::vector<int> getInlierIndices()", "quadmatches_inlier", "std::vector<int> getRandomSample(int N, int num)"],
        "stereo.h": ["void calDisparity_SGBM(const cv::Mat& img_L, const cv::Mat& img_R, cv::Mat& disp)"],
        "pnp.h": ["bool solvePnP(const vector<cv::Point2f>& img, const vector<cv::Point3f>& obj", "bool solvePnPLazy("],
    }
    for f, needles in want.items():
        src = open(os.path.join(inc, f)).read()
        for n in needles:
            assert n in src, (f, n)


def _write_png_set(d):
    """the files semantic_slam_mapping_amd/host/test_png.cpp expects, written by PIL (an independent encoder)"""
    import numpy as np
    from PIL import Image
    W, H = 37, 23
    y, x = np.mgrid[0:H, 0:W]
    px = lambda c: ((7 * x + 13 * y + 29 * c) & 255).astype(np.uint8)
    Image.fromarray(np.stack([px(0), px(1), px(2)], -1), "RGB").save(os.path.join(d, "rgb.png"))
    Image.fromarray(px(0), "L").save(os.path.join(d, "gray.png"))
    Image.fromarray(((257 * x + 31 * y) & 65535).astype(np.uint16)).save(os.path.join(d, "depth.png"))          # mode I;16 -> 16-bit gray PNG
    Image.fromarray(np.stack([px(0), px(1), px(2), px(3)], -1), "RGBA").save(os.path.join(d, "rgba.png"))
    pal = Image.fromarray(((x + y) % 12).astype(np.uint8), "P")
    pal.putpalette(sum(([i * 20, i * 20 + 1, (i * 20 + 2) & 255] for i in range(12)), []) + [0] * (768 - 36))
    pal.save(os.path.join(d, "pal.png"))
    open(os.path.join(d, "garbage.png"), "wb").write(b"\x89PNG\r\n\x1a\n" + bytes(range(64)))


def test_png_reader(tmp_path):
    """the PNG decoder behind FrameReader's TUM / KITTI modes (the slice of cv::imread the reference uses): host only"""
    subprocess.run(["make", "-C", HOST, "test_png"], check=True, stdout=subprocess.DEVNULL)
    _write_png_set(str(tmp_path))
    out = subprocess.run([os.path.join(HOST, "test_png"), str(tmp_path)], capture_output=True, text=True)
    assert "ALL PASSED" in out.stdout and out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("PASS ") == 9


@pytest.mark.gpu
def test_frame_reader_tum_and_kitti_layouts(tmp_path):
    """FrameReader::TUM (associate.txt + colour / 16-bit depth PNGs) and FrameReader::KITTI (image_2 / image_3 pairs, depth by
    SGBM on the GPU) on small synthetic datasets written here"""
    import numpy as np
    from PIL import Image
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL)
    rng = np.random.default_rng(5)
    tum = tmp_path / "tum"; (tum / "rgb").mkdir(parents=True); (tum / "depth").mkdir()
    lines = []
    for i in range(3):
        Image.fromarray(rng.integers(0, 256, (480, 640, 3), dtype=np.uint8), "RGB").save(tum / "rgb" / f"{i}.png")
        Image.fromarray(np.full((480, 640), 1000 + i, np.uint16)).save(tum / "depth" / f"{i}.png")
        lines.append(f"{i}.0 rgb/{i}.png {i}.0 depth/{i}.png")
    (tum / "associate.txt").write_text("\n".join(lines) + "\n")
    kitti = tmp_path / "kitti"; (kitti / "image_2").mkdir(parents=True); (kitti / "image_3").mkdir()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_sgbm import stereo_pair
    for i in range(3):
        left, right, _ = stereo_pair(120, 400, 20 + i, planes=((24, None),))
        Image.fromarray(left, "L").save(kitti / "image_2" / f"{i:06d}.png"); Image.fromarray(right, "L").save(kitti / "image_3" / f"{i:06d}.png")
    # a coherent stereo sequence for the bulk stereo tracker: one textured plane (disparity 24) moving by 2 px per image, with a 150-px jump at image 4
    seq = tmp_path / "kitti_seq"; (seq / "image_2").mkdir(parents=True); (seq / "image_3").mkdir()
    left, right, _ = stereo_pair(120, 400 + 400, 31, planes=((24, None),))
    for i in range(9):
        s0 = 2 * i + (150 if i >= 4 else 0)
        Image.fromarray(np.ascontiguousarray(left[:, s0:s0 + 400]), "L").save(seq / "image_2" / f"{i:06d}.png")
        Image.fromarray(np.ascontiguousarray(right[:, s0:s0 + 400]), "L").save(seq / "image_3" / f"{i:06d}.png")
    out = subprocess.run([os.path.join(HOST, "test_host"), os.path.join(HOST, "parameters_test.txt"), str(tum), str(kitti), str(seq)], capture_output=True, text=True)
    assert "PASS frame_reader_tum" in out.stdout and "PASS frame_reader_kitti" in out.stdout and "PASS tracker_stereo_mode_runs_estimateVO" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
    assert "PASS bulk_stereo_tracker_equals_per_frame_tracker" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


@pytest.mark.gpu
def test_host_classes_on_gpu(tmp_path):
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL)
    wfile = str(tmp_path / "ssm_test_segnet.ssmw")
    subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "export_ssmw.py"), wfile], check=True)
    # the same weights as a .caffemodel: convolution (weight, bias) + caffe-segnet BN (scale, shift) blobs whose folding gives back (scale, shift)
    import numpy as np
    from semantic_slam_mapping_amd import caffemodel as cm
    from semantic_slam_mapping_amd.segnet_model import make_weights
    layers = []
    for name, (w, sc, sh) in zip(cm.LAYER_NAMES, make_weights(1234)):
        if name == "conv1_1_D":                     # no BN behind the classifier layer: scale must be 1 there, so fold it into the weights
            layers.append((name, "Convolution", [(w * sc[:, None, None, None]).astype(np.float32), sh])); continue
        layers.append((name, "Convolution", [w, np.zeros(len(sc), np.float32)])); layers.append((name + "_bn", "BN", [sc.reshape(1, -1, 1, 1), sh.reshape(1, -1, 1, 1)]))
    cfile = str(tmp_path / "ssm_test_segnet.caffemodel")
    open(cfile, "wb").write(cm.encode_caffemodel(layers))
    # conv1_1_D of the .ssmw twin gets the same folded weights, so that both files describe the same network bit for bit
    ws = make_weights(1234); w, sc, sh = ws[-1]; ws[-1] = ((w * sc[:, None, None, None]).astype(np.float32), np.ones_like(sc), sh)
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from export_ssmw import write_ssmw
    write_ssmw(wfile, ws)
    r = subprocess.run([os.path.join(HOST, "test_host"), os.path.join(HOST, "parameters_test.txt"), wfile], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, SSM_TEST_CAFFEMODEL=cfile))
    print(r.stdout[-3000:], r.stderr[-2000:])
    os.remove(cfile)
    assert "ALL PASSED" in r.stdout and r.returncode == 0
    assert r.stdout.count("PASS ") >= 20 and "PASS classifier_from_caffemodel_equals_ssmw" in r.stdout


@pytest.mark.gpu
def test_exp_mapping_driver_on_gpu():
    r = subprocess.run([os.path.join(HOST, "exp_mapping"), os.path.join(HOST, "parameters_test.txt")], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    last = [l for l in r.stdout.splitlines() if l.startswith("frames ")][-1].split()
    stats = dict(zip(last[0::2], last[1::2]))
    assert int(stats["frames"]) == 8 and int(stats["keyframes"]) == 8 and int(stats["map_updates"]) >= 1 and int(stats["map_points"]) > 500


@pytest.mark.gpu
def test_exp_mapping_rank_path_on_gpu(tmp_path):
    """`exp_mapping --ranks N` (C++ host, RCCL behind the C ABI): on this 1-GPU box the rank path runs with one rank (force_rank_path): fork before HIP,
    halo + block loop, key-frame clouds into a context map, ssm_voxel_allgather through a 1-rank communicator.  The FNV of the merged map must equal
    the one of the same eight frames fused through the python mirror of the C ABI."""
    import numpy as np
    import semantic_slam_mapping_amd as ssm
    from conftest import CAM, SEED
    prm = tmp_path / "p.txt"
    prm.write_text(open(os.path.join(HOST, "parameters_test.txt")).read().replace("map_output=/tmp/ssm_test_map.pcd", f"map_output={tmp_path}/merged.pcd") + "\nforce_rank_path=1\n")
    r = subprocess.run([os.path.join(HOST, "exp_mapping"), str(prm), "--ranks", "1"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    line = [l for l in r.stdout.splitlines() if l.startswith("rank 0/1 ")][-1].split()
    st = dict(zip(line[2::2], line[3::2]))
    assert st["frames"] == "[0,8)" and st["halo"] == "0" and int(st["keyframes"]) == 8
    assert os.path.getsize(tmp_path / "merged.pcd") > 1000                    # rank 0 wrote the merged map as binary PCD
    c = ssm.Context(0, orb_features=1000, max_batch=1, voxel_capacity_log2=18, camera=CAM)
    try:
        W, H = 640, 480
        bufs = [c.dev_alloc(W * H * 3), c.dev_alloc(W * H * 2), c.dev_alloc(W * H * 3), c.dev_alloc(128)]
        c.map_clear(); total = 0
        for f in range(8):
            c.synth_frames_dev(SEED, f, 1, *bufs)
            bgr = c.d2h(bufs[0], (H, W, 3), np.uint8); dep = c.d2h(bufs[1], (H, W), np.uint16); sem = c.d2h(bufs[2], (H, W, 3), np.uint8)
            T = c.d2h(bufs[3], 16, np.float64).reshape(4, 4).T
            pts = c.generate_point_cloud(dep, bgr, sem, T); total += len(pts)
            c.map_insert(pts)
        m = c.map_export()
        h = 0xCBF29CE484222325
        for b in m.view(np.uint8).reshape(len(m), 32)[:, :24].reshape(-1).tolist():
            h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
        assert int(st["local_points"]) == total and int(st["merged_voxels"]) == len(m) and int(st["map_fnv"], 16) == h
    finally:
        c.close()


def _run_exp_mapping(prm_text, tmp_path, name, *flags):
    prm = tmp_path / f"{name}.txt"
    prm.write_text(prm_text)
    r = subprocess.run([os.path.join(HOST, "exp_mapping"), str(prm), *flags], capture_output=True, text=True, timeout=600)
    print(r.stdout[-1500:], r.stderr[-1500:])
    assert r.returncode == 0
    last = [l for l in r.stdout.splitlines() if l.startswith("frames ")][-1].split()
    st = dict(zip(last[0::2], last[1::2]))
    st["_stderr"] = r.stderr
    return st


@pytest.mark.gpu
def test_exp_mapping_batched_equals_per_frame_on_gpu(tmp_path):
    """exp_mapping --batched (BatchTracker: ssm_seq_process + ssm_tracker_run over chunks of frames) against the per-frame loop with the poses coming
    from the tracker (use_stream_pose=0): the trajectory files must be identical byte for byte (C99 hex floats), and so the key-frame gate"""
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL)
    base = open(os.path.join(HOST, "parameters_test.txt")).read().replace("end_index=8", "end_index=26").replace("map_output=/tmp/ssm_test_map.pcd", f"map_output={tmp_path}/map.pcd")
    base += "\nuse_stream_pose=0\ntracker_chunk=10\nssm_max_batch=4\n"
    a = _run_exp_mapping(base + f"trajectory_output={tmp_path}/per_frame.txt\n", tmp_path, "a")
    b = _run_exp_mapping(base + f"trajectory_output={tmp_path}/batched.txt\n", tmp_path, "b", "--batched")
    ta, tb = open(tmp_path / "per_frame.txt").read(), open(tmp_path / "batched.txt").read()
    assert len(ta.splitlines()) == 26 and ta == tb
    assert a["pose_fnv"] == b["pose_fnv"] and a["keyframes"] == b["keyframes"] and int(a["frames"]) == int(b["frames"]) == 26


@pytest.mark.gpu
def test_exp_mapping_batched_stereo_equals_per_frame_on_gpu(tmp_path):
    """exp_mapping --batched with tracker_mode = stereo on a KITTI-layout directory (BatchStereoTracker: quad matcher, SGBM depth and stereo VO of a chunk of
    frames per launch, the reader leaves the depth to it) against the per-frame loop (FrameReader::KITTI computes the depth, Tracker::estimateVO per frame):
    identical trajectory files, key-frames and map"""
    import numpy as np
    from PIL import Image
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_sgbm import stereo_pair
    seq = tmp_path / "kitti"; (seq / "image_2").mkdir(parents=True); (seq / "image_3").mkdir()
    left, right, _ = stereo_pair(120, 800, 41, planes=((24, None),))
    n_img = 12
    for i in range(n_img):
        s0 = 3 * i
        L = np.ascontiguousarray(left[:, s0:s0 + 400]); R = np.ascontiguousarray(right[:, s0:s0 + 400])
        Image.fromarray(np.stack([L, L, L], -1), "RGB").save(seq / "image_2" / f"{i:06d}.png"); Image.fromarray(R, "L").save(seq / "image_3" / f"{i:06d}.png")
    base = open(os.path.join(HOST, "parameters_test.txt")).read().replace("end_index=8", "end_index=50").replace("dataset=synthetic", "dataset=kitti")
    base = base.replace("map_output=/tmp/ssm_test_map.pcd", f"map_output={tmp_path}/map.pcd")
    base += (f"\ndata_source={seq}\ntracker_mode=stereo\nimage_width=400\nimage_height=120\norb_levels=3\norb_features=300\ncamera.baseline=0.532331858\n"
             "camera.roix=2000\ncamera.roiy=2000\ncamera.roiz=4000\ninlier_threshold=2.0\ntracker_chunk=4\nssm_max_batch=3\nmapper_drain_ms=1000\n")
    a = _run_exp_mapping(base + f"trajectory_output={tmp_path}/per_frame.txt\n", tmp_path, "a")
    b = _run_exp_mapping(base + f"trajectory_output={tmp_path}/batched.txt\n", tmp_path, "b", "--batched")
    ta, tb = open(tmp_path / "per_frame.txt").read(), open(tmp_path / "batched.txt").read()
    assert len(ta.splitlines()) == n_img - 1 and ta == tb
    assert a["pose_fnv"] == b["pose_fnv"] and a["keyframes"] == b["keyframes"] and int(a["frames"]) == int(b["frames"]) == n_img - 1


@pytest.mark.gpu
def test_exp_mapping_tum_end_to_end_on_gpu(tmp_path):
    """BASELINE configs[0] end to end on a TUM-layout directory written here (associate.txt + colour / 16-bit depth PNGs, camera.scale 5000; reference
    src/rgbdframe.cpp:199-227, experiment/exp_mapping.cpp:36-47): a RIGID scene -- a textured fronto-parallel plane at 2 m, the camera translating so that
    the image moves by (2, 1) px per frame -- through FrameReader::TUM, the Tracker (poses from PnP), the key-frame gate and the Mapper thread.
    The trajectory must follow the known motion within the PnP tolerance; every voxel of the written PCD must be a voxel of the python-side map of
    the same frames at the tracked poses (the viewer thread's update schedule decides which key-frames are in the last map: a subset)."""
    import numpy as np
    from PIL import Image
    import semantic_slam_mapping_amd as ssm
    from oracle.binding import Oracle
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL)
    N, W, H, Z0, DX, DY, SCALE = 20, 640, 480, 2.0, 2, 1, 5000.0
    fx, fy, cx, cy = 517.3, 516.5, 318.6, 255.3
    bgr0 = Oracle().synth_frame(0x5EED0000, 7)[0]
    d = tmp_path / "tum"; (d / "rgb").mkdir(parents=True); (d / "depth").mkdir()
    lines, frames = [], []
    for k in range(N):
        bgr = np.roll(np.roll(bgr0, k * DX, axis=1), k * DY, axis=0).copy()
        dep = np.full((H, W), int(Z0 * SCALE), np.uint16)
        Image.fromarray(bgr[:, :, ::-1].copy(), "RGB").save(d / "rgb" / f"{k}.png"); Image.fromarray(dep).save(d / "depth" / f"{k}.png")
        lines.append(f"{k}.0 rgb/{k}.png {k}.0 depth/{k}.png"); frames.append((bgr, dep))
    (d / "associate.txt").write_text("\n".join(lines) + "\n")
    prm = open(os.path.join(HOST, "parameters_test.txt")).read()
    prm = prm.replace("end_index=8", f"end_index={N}").replace("dataset=synthetic", "dataset=tum").replace("camera.scale=1000.0", f"camera.scale={SCALE}")
    prm = prm.replace("map_output=/tmp/ssm_test_map.pcd", f"map_output={tmp_path}/map.pcd")
    prm += f"\ndata_source={d}\ntrajectory_output={tmp_path}/traj.txt\nmapper_drain_ms=1500\n"
    st = _run_exp_mapping(prm, tmp_path, "tum")
    assert int(st["frames"]) == N and int(st["keyframes"]) >= 5 and int(st["map_updates"]) >= 1
    # ---- trajectory against the known motion.  The true pose of frame k is x_cam = x_world + k (DX Z0 / fx, DY Z0 / fy, 0); for a fronto-parallel
    # plane seen through a 64-degree lens a small rotation about y and a translation along x are nearly the same image motion, so the criterion is the one
    # PnP minimises: the plane's points (frame 0 = world, identity pose) must re-project to where the image content moved, (u + k DX, v + k DY)
    T = {}
    for ln in open(tmp_path / "traj.txt"):
        p = ln.split(); T[int(p[0])] = np.array([float.fromhex(v) for v in p[1:]]).reshape(4, 4).T
    assert sorted(T) == list(range(N)) and np.array_equal(T[0], np.eye(4))
    uu, vv = np.meshgrid(np.arange(60, 560, 50.0), np.arange(60, 400, 50.0))
    Xw = np.stack([(uu - cx) * Z0 / fx, (vv - cy) * Z0 / fy, np.full_like(uu, Z0), np.ones_like(uu)], 0).reshape(4, -1)
    drift = []
    for k in range(N):
        Xc = T[k] @ Xw
        err = np.hypot(fx * Xc[0] / Xc[2] + cx - (uu.reshape(-1) + k * DX), fy * Xc[1] / Xc[2] + cy - (vv.reshape(-1) + k * DY))
        # the reference's own bias is inside this bound: 3-D positions are unprojected at TRUNCATED pixel coordinates (include/orb.h:50), ~0.5 px per axis
        # against the sub-pixel 2-D side, and every frame inherits the offsets of the reference frames it is solved against (odometry drift)
        drift.append(err.max())
        assert err.max() < 1.0 + 0.3 * k, (k, drift, T[k][:3, 3])
        assert np.abs(T[k][:3, :3] - np.eye(3)).max() < 2e-2 and abs(T[k][2, 3]) < 2e-2, k
    print("re-projection error per frame [px]:", [round(float(v), 2) for v in drift])
    assert np.hypot(T[N - 1][0, 3] - (N - 1) * DX * Z0 / fx, T[N - 1][1, 3] - (N - 1) * DY * Z0 / fy) < 0.05 and T[N - 1][0, 3] > 0.1
    # ---- the PCD against the python-side map of the same frames at those poses
    raw = open(tmp_path / "map.pcd", "rb").read()
    hdr, body = raw.split(b"DATA binary\n", 1)
    npts = int([l for l in hdr.decode().splitlines() if l.startswith("POINTS")][0].split()[1])
    pts = np.frombuffer(body, np.dtype([("xyz", "<f4", 3), ("rgba", "<u4")]), npts)
    assert npts == int(st["map_points"]) > 500
    c = ssm.Context(0, orb_features=1000, max_batch=1, voxel_capacity_log2=18, camera=(cx, cy, fx, fy, SCALE))
    try:
        vox = set()
        inv = np.float32(1.0) / np.float32(0.1)
        for k, (bgr, dep) in enumerate(frames):
            cloud = c.generate_point_cloud(dep, bgr, np.zeros_like(bgr), T[k])
            xyz = np.stack([cloud["x"], cloud["y"], cloud["z"]], 1)
            vox.update(map(tuple, np.floor(xyz * inv).astype(np.int64).tolist()))
        mine = set(map(tuple, np.floor(pts["xyz"] * inv).astype(np.int64).tolist()))
        assert mine <= vox and len(mine) > 0.3 * len(vox)
    finally:
        c.close()


@pytest.mark.gpu
def test_mapper_falls_back_to_the_host_path_with_the_same_map(tmp_path):
    """Mapper::viewer keeps its map on the device; when a device-resident update fails (out of memory on a long sequence) it frees its device clouds,
    gives the slabs and the update's buffers back (ssm_viewer_map_release) and continues on the host path from the last published map -- the same bits.  The third
    update is made to fail (mapper_test_fail_update); a paced stream (one frame per 25 ms: the viewer takes every key-frame as it arrives, so the update schedule is the
    same in both runs) gives the PCD of a run that used the host path from the start (mapper_device_map = 0), byte for byte"""
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL)
    base = open(os.path.join(HOST, "parameters_test.txt")).read().replace("end_index=8", "end_index=24").replace("keyframe_min_translation=0.005", "keyframe_min_translation=0.02")
    base += "\nsynthetic_rigid=1\nsequence_length=24\nframe_period_ms=25\nmapper_drain_ms=400\n"
    def run(name, extra):
        txt = base.replace("map_output=/tmp/ssm_test_map.pcd", f"map_output={tmp_path}/{name}.pcd") + extra
        st = _run_exp_mapping(txt, tmp_path, name)
        return st, open(tmp_path / f"{name}.pcd", "rb").read()
    sa, a = run("host", "mapper_device_map=0\n")
    sb, b = run("dev", "mapper_device_map=1\nmapper_test_fail_update=2\n")
    assert "device-resident map update failed" in sb["_stderr"] and "device-resident map update failed" not in sa["_stderr"]
    assert sa["keyframes"] == sb["keyframes"] and int(sa["map_updates"]) == int(sb["map_updates"]) >= 4
    assert len(a) > 1000 and a == b


def test_sanitizer_builds_of_oracle_and_host_layer(tmp_path):
    """CPU sanitizers: the oracle's driver under ASan + UBSan, and the host layer's thread test (PoseGraph + Mapper::viewer + a polling
    thread, device calls into host/san_stub_device.cpp) under ThreadSanitizer.  scripts/run_sanitizers.sh runs the full matrix and writes
    profiles/r03_sanitizers.log; this keeps the two most telling legs in the CPU suite."""
    ORACLE = os.path.join(ROOT, "oracle")
    for san in ("asan", "ubsan"):
        r = subprocess.run(["make", "-s", "-C", ORACLE, f"SAN={san}", "san"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "san_check OK" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout[-800:] + r.stderr[-2000:]
    subprocess.run(["make", "-s", "-C", HOST, "SAN=tsan", "test_threads_tsan"], check=True, capture_output=True, timeout=600)
    r = subprocess.run([os.path.join(HOST, "test_threads_tsan"), os.path.join(HOST, "parameters_test.txt"), str(tmp_path / "threads.pcd")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout and "ThreadSanitizer" not in r.stderr, r.stdout[-500:] + r.stderr[-3000:]
