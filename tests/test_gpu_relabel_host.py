"""Label fusion through the C++ host classes on a real MI355X: host/test_relabel.cpp (Mapper with mapper_relabel off and on, both routes to the clouds against
ssm_relabel_host replayed cloud after cloud, and the truth of the analytic KITTI-layout scene of host/test_grid.cpp with label noise planted in key-frames 3 and 5;
the rendering's label counts; carving and alignment on top; the published map after the final rebuild) and the exp_mapping driver's --relabel mode per frame and
--batched."""
import os
import subprocess
import sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "semantic_slam_mapping_amd", "host")
pytestmark = pytest.mark.gpu
FIELDS = ("relabel_keyframes", "relabel_changed", "relabel_filled", "relabel_fnv")


def test_mapper_switch_both_routes_and_truth():
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(HOST, "test_relabel"), os.path.join(HOST, "parameters_test.txt")], capture_output=True, text=True, timeout=300)
    print(out.stdout[-5000:], out.stderr[-2000:])
    for name in ("switch_defaults_to_off", "switch_off_clouds_as_before", "routes_give_the_same_bytes", "the_labels_are_the_host_function_replayed_cloud_after_cloud",
                 "only_the_label_bytes_change", "every_cloud_once_and_at_most_2_window_plus_1_views_alive", "band_points_with_two_voting_views_end_true",
                 "no_true_label_is_lost", "wrong_and_unknown_labels_fall_strictly", "rendering_geometric_counts_identical",
                 "rendering_label_disagree_does_not_rise_and_agree_rises", "with_carving_and_alignment_both_routes_agree", "grid_routes_give_the_same_ground_labels",
                 "some_ground_labels_are_tree_without_the_switch", "tree_ground_labels_fall_and_none_is_left_where_no_tree_point_is",
                 "the_published_map_holds_no_tree_after_the_final_rebuild", "tree_voxels_fall_where_a_rebuild_takes_the_corrupted_frames"):
        assert "PASS " + name in out.stdout, out.stdout[-5000:] + out.stderr[-2000:]
    assert out.returncode == 0 and "ALL PASSED" in out.stdout


def test_exp_mapping_relabel_is_the_same_per_frame_and_batched(tmp_path):
    """--relabel appends its four fields to the summary line, the same for the per-frame loop and --batched; without the flag the line has none of them and
    everything else on it is the same"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_align_host import driver_setup
    base, _run_exp_mapping = driver_setup(tmp_path)
    a = _run_exp_mapping(base, tmp_path, "a", "--relabel")
    b = _run_exp_mapping(base, tmp_path, "b", "--relabel", "--batched")
    c = _run_exp_mapping(base, tmp_path, "c")
    assert all(k in a for k in FIELDS) and all(k in b for k in FIELDS) and not any(k in c for k in FIELDS)
    assert [a[k] for k in FIELDS] == [b[k] for k in FIELDS]
    assert a["pose_fnv"] == b["pose_fnv"] == c["pose_fnv"] and a["keyframes"] == b["keyframes"] == c["keyframes"] and int(a["frames"]) == 8
    assert [k for k in a if not k.startswith("relabel_")] == list(c)          # the flag only appends its fields
    assert int(a["relabel_keyframes"]) == int(a["keyframes"]) > 0 and int(a["relabel_filled"]) <= int(a["relabel_changed"])
