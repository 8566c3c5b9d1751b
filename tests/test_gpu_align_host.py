"""Dense alignment through the C++ host classes on a real MI355X: host/test_align.cpp (Mapper with mapper_align off and on, both routes to the clouds, against
ssm_align_host view after view, on an analytic KITTI-layout scene whose key-frame poses carry a planted cumulative error in height, pitch and roll -- the
directions a ground plane constrains, tests/test_align.py test_the_road_constrains_height_pitch_and_roll; map poses against the truth; the rendering yardstick
without and with the switch; carving on top) and the exp_mapping driver's --align mode per frame and --batched."""
import os
import subprocess
import sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "semantic_slam_mapping_amd", "host")
pytestmark = pytest.mark.gpu
FIELDS = ("align_keyframes", "align_accepted", "align_fnv")


def test_mapper_switch_both_routes_truth_and_yardstick():
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(HOST, "test_align"), os.path.join(HOST, "parameters_test.txt")], capture_output=True, text=True, timeout=300)
    print(out.stdout[-5000:], out.stderr[-2000:])
    for name in ("switch_defaults_to_off", "switch_off_clouds_and_poses_as_before", "every_key_frame_is_aligned_exactly_once", "routes_give_the_same_info_correction_and_map_pose",
                 "alignment_changes_no_cloud", "the_key_frames_own_poses_are_not_written", "alignment_is_the_host_function_view_after_view", "every_later_key_frame_is_accepted",
                 "accepted_map_poses_are_closer_to_the_truth_in_height_pitch_and_roll", "the_yardstick_agrees_on_strictly_more_pixels",
                 "the_yardstick_has_strictly_fewer_pixels_off_the_surface", "rendering_uses_the_map_poses_on_both_routes", "with_carving_both_routes_agree",
                 "the_viewer_aligns_every_key_frame_once"):
        assert "PASS " + name in out.stdout, out.stdout[-5000:] + out.stderr[-2000:]
    assert out.returncode == 0 and "ALL PASSED" in out.stdout


def driver_setup(tmp_path):
    """the synthetic KITTI-layout stereo sequence of tests/test_gpu_uvd_host.py and the driver's parameters for it -> (the parameter text, the driver's runner)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_host_cpp import _run_exp_mapping
    from test_gpu_uvd_host import write_sequence
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL)
    seq = tmp_path / "kitti"
    write_sequence(seq, 9, rgb_left=True)
    base = open(os.path.join(HOST, "parameters_test.txt")).read().replace("end_index=8", "end_index=50").replace("dataset=synthetic", "dataset=kitti")
    base = base.replace("map_output=/tmp/ssm_test_map.pcd", f"map_output={tmp_path}/map.pcd")
    base += (f"\ndata_source={seq}\ntracker_mode=stereo\nimage_width=400\nimage_height=120\norb_levels=3\norb_features=300\ncamera.baseline=0.532331858\n"
             "camera.roix=2000\ncamera.roiy=2000\ncamera.roiz=4000\ninlier_threshold=2.0\ntracker_chunk=3\nssm_max_batch=3\nmapper_drain_ms=1000\n")
    return base, _run_exp_mapping


def test_exp_mapping_align_is_the_same_per_frame_and_batched(tmp_path):
    """--align appends its three fields to the summary line, the same for the per-frame loop and --batched; without the flag the line has none of them and
    everything else on it is the same"""
    base, _run_exp_mapping = driver_setup(tmp_path)
    a = _run_exp_mapping(base, tmp_path, "a", "--align")
    b = _run_exp_mapping(base, tmp_path, "b", "--align", "--batched")
    c = _run_exp_mapping(base, tmp_path, "c")
    assert all(k in a for k in FIELDS) and all(k in b for k in FIELDS) and not any(k in c for k in FIELDS)
    assert [a[k] for k in FIELDS] == [b[k] for k in FIELDS]
    assert a["pose_fnv"] == b["pose_fnv"] == c["pose_fnv"] and a["keyframes"] == b["keyframes"] == c["keyframes"] and int(a["frames"]) == 8
    assert int(a["align_keyframes"]) == int(a["keyframes"]) > 1 and 0 <= int(a["align_accepted"]) < int(a["align_keyframes"])
    assert [k for k in a if not k.startswith("align_")] == list(c)          # the flag only appends its three fields


def test_exp_mapping_align_with_carve_is_the_same_per_frame_and_batched(tmp_path):
    """--align --carve: key-frame by key-frame the Mapper aligns, then carves, so the per-frame loop and --batched (three key-frames arrive at once) agree on both
    switches' fields"""
    base, _run_exp_mapping = driver_setup(tmp_path)
    ac = _run_exp_mapping(base, tmp_path, "ac", "--align", "--carve")
    bc = _run_exp_mapping(base, tmp_path, "bc", "--align", "--carve", "--batched")
    carve = ("carve_keyframes", "carve_tested", "carve_removed", "carve_fnv")
    assert [ac[k] for k in FIELDS + carve] == [bc[k] for k in FIELDS + carve] and int(ac["align_keyframes"]) == int(ac["keyframes"]) and int(ac["carve_keyframes"]) == int(ac["keyframes"]) - 1
