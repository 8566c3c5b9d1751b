"""The ground grid through the C++ host classes on a real MI355X: host/test_grid.cpp (Mapper with mapper_grid off and on, both routes to the clouds, against
ssm_grid_host on the fetched clouds, the written files, and the truth of an analytic KITTI-layout scene -- a ground plane whose lane is painted Road and whose
sides Pavement, a box painted Car beside the lane, 8 key-frames ray-cast from their true poses; carving and alignment on top; the viewer thread; an extent beyond
the cell limit) and the exp_mapping driver's --grid mode per frame and --batched."""
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "semantic_slam_mapping_amd", "host")
pytestmark = pytest.mark.gpu
FIELDS = ("grid_cells", "grid_drivable", "grid_walkable", "grid_obstacle", "grid_fnv")


def test_mapper_switch_both_routes_files_and_truth(tmp_path):
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(HOST, "test_grid"), os.path.join(HOST, "parameters_test.txt"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(out.stdout[-5000:], out.stderr[-2000:])
    for name in ("switch_defaults_to_off", "switch_off_clouds_as_before_and_no_grid", "routes_give_the_same_bytes", "the_grid_changes_no_cloud",
                 "the_extent_is_the_key_frames_box_widened_by_max_distance", "the_grid_is_the_host_function_on_the_fetched_clouds",
                 "the_written_files_read_back_as_the_fetched_arrays_and_the_spec", "cells_inside_the_box_are_obstacles_labelled_car", "lane_cells_are_drivable",
                 "pavement_cells_are_walkable", "ground_heights_lie_within_the_quantisation_bound_of_the_plane", "with_carving_and_alignment_both_routes_agree",
                 "the_viewer_builds_the_grid_as_it_ends", "an_extent_beyond_the_cell_limit_is_skipped"):
        assert "PASS " + name in out.stdout, out.stdout[-5000:] + out.stderr[-2000:]
    assert out.returncode == 0 and "ALL PASSED" in out.stdout
    assert sorted(os.listdir(tmp_path)) == ["grid.txt", "grid_colour.png", "grid_height.png"]


def test_exp_mapping_grid_is_the_same_per_frame_and_batched(tmp_path):
    """--grid appends its five fields to the summary line, the same for the per-frame loop and --batched; without the flag the line has none of them and
    everything else on it is the same; with a directory the two images and grid.txt are there, and the images have the grid's shape"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_align_host import driver_setup
    base, _run_exp_mapping = driver_setup(tmp_path)
    png = tmp_path / "grid"
    png.mkdir()
    a = _run_exp_mapping(base, tmp_path, "a", "--grid", str(png))
    b = _run_exp_mapping(base, tmp_path, "b", "--grid", "--batched")
    c = _run_exp_mapping(base, tmp_path, "c")
    assert all(k in a for k in FIELDS) and all(k in b for k in FIELDS) and not any(k in c for k in FIELDS)
    assert [a[k] for k in FIELDS] == [b[k] for k in FIELDS]
    assert a["pose_fnv"] == b["pose_fnv"] == c["pose_fnv"] and a["keyframes"] == b["keyframes"] == c["keyframes"] and int(a["frames"]) == 8
    assert [k for k in a if not k.startswith("grid_")] == list(c)          # the flag only appends its fields
    assert int(a["grid_cells"]) > 0 and 0 < int(a["grid_drivable"]) + int(a["grid_walkable"]) + int(a["grid_obstacle"]) <= int(a["grid_cells"])
    assert sorted(os.listdir(png)) == ["grid.txt", "grid_colour.png", "grid_height.png"]
    spec = dict(line.split(None, 1) for line in open(png / "grid.txt").read().strip().split("\n"))
    assert int(spec["nx"]) * int(spec["ny"]) == int(a["grid_cells"]) and float(spec["cell"]) == 0.2 and len(spec["G"].split()) == 12
    assert np.allclose(np.array(spec["G"].split(), float).reshape(3, 4), [[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0]])
