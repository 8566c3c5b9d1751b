"""The semantic-motion fusion through the C++ host classes on a real MI355X: host/test_motion_fuse.cpp (Mapper with motion_semantic_fuse off, on with an empty
moving_mask, on with a mask: both routes to a key-frame's cloud) and the exp_mapping driver's --fuse-motion mode per frame and --batched, on the synthetic
KITTI-layout stereo sequence of tests/test_gpu_uvd_host.py with label images added: the box that does not follow the ego-motion and a second, static region are
both painted in the Car colour."""
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "semantic_slam_mapping_amd", "host")
pytestmark = pytest.mark.gpu
STATIC = (slice(40, 90), slice(300, 360))          # rows, columns of the parked car
ROAD_RGB, CAR_RGB = (128, 64, 128), (64, 0, 128)    # PNG channel order; the library reads BGR


def test_mapper_switch_and_both_cloud_routes():
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(HOST, "test_motion_fuse"), os.path.join(HOST, "parameters_test.txt")], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:], out.stderr[-2000:])
    for name in ("switch_defaults_to_off", "scene_has_points_to_lose", "switch_off_host_route_as_before", "switch_off_device_route_as_before",
                 "switch_on_empty_mask_host_route_as_before", "switch_on_empty_mask_device_route_as_before", "switch_on_routes_agree",
                 "switch_on_is_the_fused_backprojection", "fuse_off_is_the_class_mask", "driving_car_confirmed_parked_car_kept",
                 "fused_cloud_loses_exactly_the_confirmed_blob"):
        assert "PASS " + name in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
    assert out.returncode == 0 and "ALL PASSED" in out.stdout


def test_exp_mapping_fuse_motion_is_the_same_per_frame_and_batched(tmp_path):
    """--fuse-motion appends fused_keyframes / fused_confirmed / fused_added / fused_fnv to the summary line, the same for the per-frame loop and --batched;
    without it the line is as before.  The driving box is confirmed in some key-frame; the parked car never is, so its pixels stay in the map"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from PIL import Image
    from test_host_cpp import _run_exp_mapping
    from test_gpu_uvd_host import write_sequence, scene_disparity, W, H
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL)
    seq = tmp_path / "kitti"
    n_img = 9
    write_sequence(seq, n_img, rgb_left=True)
    _, box = scene_disparity()
    sem = np.zeros((H, W, 3), np.uint8); sem[:] = ROAD_RGB
    sem[box] = CAR_RGB; sem[STATIC] = CAR_RGB
    (seq / "segnet_0").mkdir()
    for i in range(n_img):
        Image.fromarray(sem, "RGB").save(seq / "segnet_0" / f"{i:06d}.png")
    base = open(os.path.join(HOST, "parameters_test.txt")).read().replace("end_index=8", "end_index=50").replace("dataset=synthetic", "dataset=kitti")
    base = base.replace("map_output=/tmp/ssm_test_map.pcd", f"map_output={tmp_path}/map.pcd")
    base += (f"\ndata_source={seq}\ntracker_mode=stereo\nimage_width=400\nimage_height=120\norb_levels=3\norb_features=300\ncamera.baseline=0.532331858\n"
             "camera.roix=2000\ncamera.roiy=2000\ncamera.roiz=4000\ninlier_threshold=2.0\ntracker_chunk=3\nssm_max_batch=3\nmapper_drain_ms=1000\n")
    a = _run_exp_mapping(base, tmp_path, "a", "--fuse-motion")
    b = _run_exp_mapping(base, tmp_path, "b", "--fuse-motion", "--batched")
    c = _run_exp_mapping(base, tmp_path, "c", "--moving")
    fields = ("fused_keyframes", "fused_confirmed", "fused_added", "fused_fnv")
    assert all(k in a for k in fields) and not any(k in c for k in fields)
    assert [a[k] for k in fields] == [b[k] for k in fields]
    assert a["pose_fnv"] == b["pose_fnv"] == c["pose_fnv"] and int(a["frames"]) == int(b["frames"]) == n_img - 1
    assert (a["moving_pixels"], a["moving_fnv"]) == (c["moving_pixels"], c["moving_fnv"])      # --fuse-motion implies --moving and changes nothing of it
    kf, confirmed, added = int(a["fused_keyframes"]), int(a["fused_confirmed"]), int(a["fused_added"])
    box_px = (box.sum(0) > 0).sum() + 4, (box.sum(1) > 0).sum() + 4          # the box, dilated by the 5 x 5 window
    assert kf == int(a["keyframes"]) > 0 and 0 < confirmed <= kf             # the driving box in some key-frame, and never the parked car as well
    assert added == confirmed * box_px[0] * box_px[1]                        # every added pixel is the box's: the parked car's stay in the map
    prm = tmp_path / "rgbd.txt"
    prm.write_text(open(os.path.join(HOST, "parameters_test.txt")).read())
    r = subprocess.run([os.path.join(HOST, "exp_mapping"), str(prm), "--fuse-motion"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--fuse-motion needs tracker_mode=stereo" in r.stderr
