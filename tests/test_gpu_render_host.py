"""Map rendering through the C++ host classes on a real MI355X, on the scene of tests/test_gpu_carve_host.py (a box that keeps its place in the image while the
camera moves, so every frame leaves a copy of it, and that is gone from frame 4 on): host/test_render.cpp (Mapper with mapper_render off and on, both routes to the
clouds, against the host functions view after view; the written PNG files; with carving strictly fewer map points in front of the measured surface where the box
stood) and the exp_mapping driver's --render mode per frame and --batched."""
import os
import subprocess
import sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "semantic_slam_mapping_amd", "host")
pytestmark = pytest.mark.gpu
FIELDS = ("render_views", "render_agree", "render_in_front", "render_behind", "render_label_agree", "render_label_disagree", "render_fnv")


def test_mapper_switch_both_routes_files_and_carving(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_carve_host import write_leaving_sequence, BOX_GONE_FROM
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL)
    seq = tmp_path / "seq"
    write_leaving_sequence(seq, 11)
    out_dir = tmp_path / "out"
    (out_dir / "plain").mkdir(parents=True); (out_dir / "carved").mkdir()
    out = subprocess.run([os.path.join(HOST, "test_render"), os.path.join(HOST, "parameters_test.txt"), str(seq), str(BOX_GONE_FROM), str(out_dir)], capture_output=True, text=True, timeout=300)
    print(out.stdout[-5000:], out.stderr[-2000:])
    for name in ("switch_defaults_to_off", "sequence_has_frames", "switch_off_clouds_as_before", "every_key_frame_is_a_view_once", "rendering_changes_no_cloud",
                 "routes_give_the_same_counts", "counts_are_the_host_functions_view_after_view", "counts_add_up", "the_box_left_a_trail_in_front_of_later_views",
                 "carving_leaves_strictly_fewer_points_in_front_inside_the_box", "the_written_images_read_back_as_fetched", "the_viewer_renders_as_it_ends",
                 "the_published_map_is_as_without_the_switch"):
        assert "PASS " + name in out.stdout, out.stdout[-5000:] + out.stderr[-2000:]
    assert out.returncode == 0 and "ALL PASSED" in out.stdout
    assert len(os.listdir(out_dir / "plain")) == 4 * 10 == len(os.listdir(out_dir / "carved"))          # four images per view


def test_exp_mapping_render_is_the_same_per_frame_and_batched(tmp_path):
    """--render appends its seven fields to the summary line, the same for the per-frame loop and --batched; without the flag the line has none of them and
    everything else on it is the same; with a directory the images of every view are there"""
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
    png = tmp_path / "png"
    png.mkdir()
    a = _run_exp_mapping(base, tmp_path, "a", "--render", str(png))
    b = _run_exp_mapping(base, tmp_path, "b", "--render", "--batched")
    c = _run_exp_mapping(base, tmp_path, "c")
    assert all(k in a for k in FIELDS) and all(k in b for k in FIELDS) and not any(k in c for k in FIELDS)
    assert [a[k] for k in FIELDS] == [b[k] for k in FIELDS]
    assert a["pose_fnv"] == b["pose_fnv"] == c["pose_fnv"] and a["keyframes"] == b["keyframes"] == c["keyframes"] and int(a["frames"]) == 8
    views = int(a["render_views"])
    assert views == int(a["keyframes"]) > 1 and int(a["render_agree"]) > 0 and int(a["render_label_agree"]) + int(a["render_label_disagree"]) <= int(a["render_agree"])
    assert [k for k in a if not k.startswith("render_")] == list(c)          # the flag only appends its fields
    assert sorted(os.listdir(png)) == sorted(f"render_{j:06d}_{what}.png" for j in range(views) for what in ("depth", "bgr", "label", "class"))
