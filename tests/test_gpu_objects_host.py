"""Object extraction through the C++ host classes on a real MI355X: host/test_objects.cpp (Mapper with mapper_objects off and on, both routes to the clouds,
against ssm_objects_host on the fetched clouds, the truth of the shared lane scene -- the lane Road, the sides Pavement, the box Car, 8 key-frames ray-cast from
their true poses: one Vehicle, its cell box and its refined box against the true box --, the written files, a grid built only for the objects, carving and
alignment on top, the viewer thread) and the exp_mapping driver's --objects mode per frame and --batched."""
import os
import subprocess
import sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "semantic_slam_mapping_amd", "host")
pytestmark = pytest.mark.gpu
FIELDS = ("objects_found", "objects_cells", "objects_points", "objects_fnv")


def test_mapper_switch_both_routes_files_and_truth(tmp_path):
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(HOST, "test_objects"), os.path.join(HOST, "parameters_test.txt"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(out.stdout[-5000:], out.stderr[-2000:])
    for name in ("switch_defaults_to_off", "switch_off_grid_and_clouds_as_before_and_no_objects", "routes_give_the_same_bytes", "the_objects_are_the_host_function_on_the_fetched_clouds",
                 "exactly_one_object_and_it_is_a_vehicle", "the_cell_box_lies_within_one_cell_of_the_true_footprint",
                 "the_refined_box_lies_inside_the_true_box_widened_by_the_derived_bound", "every_object_point_is_labelled_vehicle_and_is_a_high_point_of_its_cells",
                 "the_centroid_lies_in_the_refined_box", "the_written_files_read_back_as_the_fetched_records_and_image",
                 "without_mapper_grid_the_grid_is_built_for_the_objects_and_no_grid_file_is_written", "with_carving_and_alignment_both_routes_agree",
                 "the_viewer_extracts_the_objects_as_it_ends", "switch_off_the_published_map_as_before"):
        assert "PASS " + name in out.stdout, out.stdout[-5000:] + out.stderr[-2000:]
    assert out.returncode == 0 and "ALL PASSED" in out.stdout
    assert sorted(os.listdir(tmp_path)) == ["none", "objects.txt", "objects_id.png"] and os.listdir(tmp_path / "none") == []


def test_exp_mapping_objects_is_the_same_per_frame_and_batched(tmp_path):
    """--objects appends its four fields to the summary line, the same for the per-frame loop and --batched; without the flag the line has none of them and
    everything else on it is the same; with a directory objects.txt and objects_id.png are there and no grid file.  The stereo sequence of this test carries no
    semantic labels, so its obstacle cells have none and it yields NO object under any rule (observed: 38 obstacle cells, 0 objects): the counts here are those
    of an empty list, which is what is asserted; test_exp_mapping_objects_on_the_labelled_stream below is the driver run that finds some"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_align_host import driver_setup
    base, _run_exp_mapping = driver_setup(tmp_path)
    files = tmp_path / "objects"
    files.mkdir()
    a = _run_exp_mapping(base, tmp_path, "a", "--objects", str(files))
    b = _run_exp_mapping(base, tmp_path, "b", "--objects", "--batched")
    c = _run_exp_mapping(base, tmp_path, "c")
    assert all(k in a for k in FIELDS) and all(k in b for k in FIELDS) and not any(k in c for k in FIELDS)
    assert [a[k] for k in FIELDS] == [b[k] for k in FIELDS]
    assert a["pose_fnv"] == b["pose_fnv"] == c["pose_fnv"] and a["keyframes"] == b["keyframes"] == c["keyframes"] and int(a["frames"]) == 8
    assert [k for k in a if not k.startswith("objects_")] == list(c)          # the flag only appends its fields
    assert (int(a["objects_found"]), int(a["objects_cells"]), int(a["objects_points"])) == (0, 0, 0)
    assert sorted(os.listdir(files)) == ["objects.txt", "objects_id.png"] and open(files / "objects.txt").read() == ""
    # under the loosest rule -- every label, one cell, one point, no height -- every labelled obstacle cell of the driver's scene belongs to an object
    loose = base + "mapper_objects_labels=0 1 2 3 4 5 6 7 8 9 10 11\nmapper_objects_min_cells=1\nmapper_objects_min_points=1\nmapper_objects_min_height=0\n"
    la = _run_exp_mapping(loose, tmp_path, "la", "--objects")
    lb = _run_exp_mapping(loose, tmp_path, "lb", "--objects", "--batched")
    print("driver scene:", {k: a[k] for k in FIELDS}, "loosest rule:", {k: la[k] for k in FIELDS})
    assert [la[k] for k in FIELDS] == [lb[k] for k in FIELDS] and la["pose_fnv"] == a["pose_fnv"]
    assert int(la["objects_found"]) == 0          # (no label, no member cell)
    g = _run_exp_mapping(base, tmp_path, "g", "--objects", "--grid")          # with the grid's own switch on top: the same objects, the grid's fields as without --objects
    assert [g[k] for k in FIELDS] == [a[k] for k in FIELDS] and "grid_fnv" in g


def test_exp_mapping_objects_on_the_labelled_stream(tmp_path):
    """the driver on its synthetic RGB-D stream, whose semantic images carry the twelve classes: under a rule that takes every label the summary line reports
    objects, their cells and points, objects.txt has one line per object whose cells and points add up to the line's, and objects_id.png is there"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_host_cpp import _run_exp_mapping
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL)
    files = tmp_path / "objects"
    files.mkdir()
    base = open(os.path.join(HOST, "parameters_test.txt")).read().replace("map_output=/tmp/ssm_test_map.pcd", f"map_output={tmp_path}/map.pcd")
    base += "\nmapper_objects_labels=0 1 2 3 4 5 6 7 8 9 10 11\nmapper_objects_min_cells=1\nmapper_objects_min_points=1\nmapper_objects_min_height=0\n"
    a = _run_exp_mapping(base, tmp_path, "a", "--objects", str(files))
    c = _run_exp_mapping(base, tmp_path, "c")
    print("synthetic stream:", {k: a[k] for k in FIELDS})
    assert [k for k in a if not k.startswith("objects_")] == list(c) and a["pose_fnv"] == c["pose_fnv"]
    lines = [ln.split() for ln in open(files / "objects.txt").read().strip().split("\n")]
    assert int(a["objects_found"]) == len(lines) > 0 and [int(ln[0]) for ln in lines] == list(range(len(lines)))
    assert sum(int(ln[2]) for ln in lines) == int(a["objects_cells"]) and sum(int(ln[3]) for ln in lines) == int(a["objects_points"]) > 0
    assert all(len(ln) == 15 for ln in lines) and sorted(os.listdir(files)) == ["objects.txt", "objects_id.png"]
