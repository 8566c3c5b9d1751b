"""The route field through the C++ host classes on a real MI355X: host/test_route.cpp (Mapper with mapper_route off and on, both routes to the clouds, against
ssm_route_cells_host and ssm_route_path_host on the fetched clearance map, the scene's 286 reachable cells routed or counted, the truth derived from the shared lane
scene -- where the path passes the box --, the written files, a grid and a clearance map built only for the route, the path to the farthest cell, objects, carving and
alignment on top, the viewer thread) and the exp_mapping driver's --route mode per frame and --batched."""
import os
import subprocess
import sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "semantic_slam_mapping_amd", "host")
pytestmark = pytest.mark.gpu
FIELDS = ("route_routed", "route_max_cost", "route_path_len", "route_path_cost", "route_fnv")


def test_mapper_switch_both_routes_files_and_truth(tmp_path):
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(HOST, "test_route"), os.path.join(HOST, "parameters_test.txt"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(out.stdout[-5000:], out.stderr[-2000:])
    for name in ("switch_defaults_to_off", "switch_off_grid_objects_clearance_and_clouds_as_before_and_no_route", "routes_give_the_same_bytes",
                 "the_field_and_the_path_are_the_host_functions_on_the_fetched_clearance_map", "all_286_reachable_cells_are_routed_or_counted_unrouted",
                 "the_path_starts_at_the_snapped_seed_and_ends_on_the_goal", "the_path_passes_the_box_through_the_lanes_two_left_columns", "the_path_holds_none_of_the_closed_cells_beside_the_box",
                 "the_path_costs_at_least_the_chamfer_cost_of_the_straight_line", "the_written_files_read_back_as_the_fetched_arrays",
                 "without_grid_and_clearance_both_are_built_for_the_route_and_write_no_file", "without_a_goal_the_path_leads_to_the_farthest_cell",
                 "with_objects_carving_and_alignment_both_routes_agree", "the_viewer_routes_as_it_ends", "switch_off_the_published_map_as_before"):
        assert "PASS " + name in out.stdout, out.stdout[-5000:] + out.stderr[-2000:]
    assert out.returncode == 0 and "ALL PASSED" in out.stdout
    assert sorted(os.listdir(tmp_path)) == ["none", "route.png", "route.txt", "route_cost.png"] and os.listdir(tmp_path / "none") == []


def test_exp_mapping_route_is_the_same_per_frame_and_batched(tmp_path):
    """--route appends its five fields to the END of the summary line, the same for the per-frame loop and --batched; without the flag the line has none of them and
    everything else on it is the same; with a directory the three files are there and no grid or clearance file; with --clearance, --grid and --objects on top the
    same field, its fields still last"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_align_host import driver_setup
    base, _run_exp_mapping = driver_setup(tmp_path)
    files = tmp_path / "route"
    files.mkdir()
    a = _run_exp_mapping(base, tmp_path, "a", "--route", str(files))
    b = _run_exp_mapping(base, tmp_path, "b", "--route", "--batched")
    c = _run_exp_mapping(base, tmp_path, "c")
    print("driver scene:", {k: a[k] for k in FIELDS})
    assert all(k in a for k in FIELDS) and all(k in b for k in FIELDS) and not any(k in c for k in FIELDS)
    assert [a[k] for k in FIELDS] == [b[k] for k in FIELDS]
    assert a["pose_fnv"] == b["pose_fnv"] == c["pose_fnv"] and a["keyframes"] == b["keyframes"] == c["keyframes"] and int(a["frames"]) == 8
    fields = lambda st: [k for k in st if k != "_stderr"]  # noqa: E731
    assert [k for k in a if not k.startswith("route_")] == list(c) and fields(a)[-5:] == list(FIELDS)          # the flag only appends its fields, after the others
    assert sorted(os.listdir(files)) == ["route.png", "route.txt", "route_cost.png"]
    txt = [ln.split() for ln in open(files / "route.txt").read().strip().split("\n")]
    assert [t[0] for t in txt[:15]] == ["routed", "unrouted", "near_cells", "max_cost", "far_cell", "source_cell", "comfort2", "moves", "len", "goal_cell", "cost", "n_axial", "n_diag", "near_steps",
                                        "min_d2"]
    info = dict(txt[:15])
    assert (info["routed"], info["max_cost"], info["len"], info["cost"]) == tuple(a[k] for k in FIELDS[:4]) and len(txt) == 15 + int(info["len"])
    g = _run_exp_mapping(base, tmp_path, "g", "--route", "--clearance", "--grid", "--objects")
    assert [g[k] for k in FIELDS] == [a[k] for k in FIELDS] and "grid_fnv" in g and "objects_fnv" in g and "clearance_fnv" in g and fields(g)[-5:] == list(FIELDS)
