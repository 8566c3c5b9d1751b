"""The clearance map through the C++ host classes on a real MI355X: host/test_clearance.cpp (Mapper with mapper_clearance off and on, both routes to the clouds,
against ssm_clearance_cells_host on the fetched class image, no traversable cell within r2 of an obstacle, the reachable set against a fill from the seed, the
seed's snap, the truth derived from the shared lane scene -- which lane cells must be reachable and which are closed beside the box --, the written files, a grid
built only for the clearance map, objects, carving and alignment on top, the viewer thread) and the exp_mapping driver's --clearance mode per frame and --batched."""
import os
import subprocess
import sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "semantic_slam_mapping_amd", "host")
pytestmark = pytest.mark.gpu
FIELDS = ("clearance_blocked", "clearance_traversable", "clearance_reachable", "clearance_max_d2", "clearance_fnv")


def test_mapper_switch_both_routes_files_and_truth(tmp_path):
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(HOST, "test_clearance"), os.path.join(HOST, "parameters_test.txt"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(out.stdout[-5000:], out.stderr[-2000:])
    for name in ("switch_defaults_to_off", "switch_off_grid_objects_and_clouds_as_before_and_no_clearance", "routes_give_the_same_bytes", "the_map_is_the_host_function_on_the_fetched_class_image",
                 "no_traversable_cell_lies_within_r2_of_an_obstacle_cell", "every_reachable_cell_is_drivable_and_connected_to_the_seed", "the_seed_is_the_snapped_cell_of_the_last_keyframes_camera",
                 "the_lane_cells_that_must_be_reachable_are", "beside_the_box_the_lanes_right_column_is_closed", "the_written_files_read_back_as_the_fetched_arrays",
                 "without_mapper_grid_the_grid_is_built_for_the_clearance_map_and_no_grid_file_is_written", "with_objects_carving_and_alignment_both_routes_agree",
                 "the_viewer_maps_the_clearance_as_it_ends", "switch_off_the_published_map_as_before"):
        assert "PASS " + name in out.stdout, out.stdout[-5000:] + out.stderr[-2000:]
    assert out.returncode == 0 and "ALL PASSED" in out.stdout
    assert sorted(os.listdir(tmp_path)) == ["clearance.png", "clearance.txt", "none", "reach.png"] and os.listdir(tmp_path / "none") == []


def test_exp_mapping_clearance_is_the_same_per_frame_and_batched(tmp_path):
    """--clearance appends its five fields to the END of the summary line, the same for the per-frame loop and --batched; without the flag the line has none of them
    and everything else on it is the same; with a directory the three files are there and no grid file; with --grid and --objects on top the same map"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_align_host import driver_setup
    base, _run_exp_mapping = driver_setup(tmp_path)
    files = tmp_path / "clearance"
    files.mkdir()
    a = _run_exp_mapping(base, tmp_path, "a", "--clearance", str(files))
    b = _run_exp_mapping(base, tmp_path, "b", "--clearance", "--batched")
    c = _run_exp_mapping(base, tmp_path, "c")
    print("driver scene:", {k: a[k] for k in FIELDS})
    assert all(k in a for k in FIELDS) and all(k in b for k in FIELDS) and not any(k in c for k in FIELDS)
    assert [a[k] for k in FIELDS] == [b[k] for k in FIELDS]
    assert a["pose_fnv"] == b["pose_fnv"] == c["pose_fnv"] and a["keyframes"] == b["keyframes"] == c["keyframes"] and int(a["frames"]) == 8
    fields = lambda st: [k for k in st if k != "_stderr"]  # noqa: E731
    assert [k for k in a if not k.startswith("clearance_")] == list(c) and fields(a)[-5:] == list(FIELDS)          # the flag only appends its fields, after the others
    assert int(a["clearance_reachable"]) <= int(a["clearance_traversable"]) and int(a["clearance_blocked"]) > 0
    assert sorted(os.listdir(files)) == ["clearance.png", "clearance.txt", "reach.png"]
    txt = dict(ln.split() for ln in open(files / "clearance.txt").read().strip().split("\n"))
    assert list(txt) == ["blocked", "free_cells", "traversable", "components", "reachable", "seed_cell", "max_d2_reachable", "r2"]
    assert (txt["blocked"], txt["traversable"], txt["reachable"], txt["max_d2_reachable"]) == tuple(a[k] for k in FIELDS[:4])
    g = _run_exp_mapping(base, tmp_path, "g", "--clearance", "--grid", "--objects")
    assert [g[k] for k in FIELDS] == [a[k] for k in FIELDS] and "grid_fnv" in g and "objects_fnv" in g and fields(g)[-5:] == list(FIELDS)
