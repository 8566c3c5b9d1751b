"""Free-space carving through the C++ host classes on a real MI355X, on the synthetic KITTI-layout stereo sequence of tests/test_gpu_uvd_host.py (a box that keeps
its place in the image while the camera moves, so every frame leaves a copy of it) with the moving-object gates off: host/test_carve.cpp on that scene with the box
gone from frame 4 on (Mapper with mapper_carve off and on, both routes to the clouds, against the host function view after view; the box's points decided per point
by construction; the published map after a rebuild) and the exp_mapping driver's --carve mode per frame and --batched on the scene as it is."""
import os
import subprocess
import sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "semantic_slam_mapping_amd", "host")
pytestmark = pytest.mark.gpu
FIELDS = ("carve_keyframes", "carve_tested", "carve_removed", "carve_fnv")


BOX_GONE_FROM = 4          # the first frame without the box (frame f shows image f + 1)


def write_leaving_sequence(d, n_img, k=0.05, seed=77):
    """test_gpu_uvd_host.write_sequence's scene and texture with one difference: from image BOX_GONE_FROM + 1 on there is no box, the ground and the background behind
    it show.  While it is there it keeps its place in the image, so each frame leaves a copy of it 2 pixels (k x its disparity) further along"""
    import numpy as np
    from PIL import Image
    from test_gpu_uvd_host import scene_disparity, W, H
    rng = np.random.default_rng(seed)
    tex = rng.integers(0, 256, (H, W + 400)).astype(np.float32)
    kern = np.array([1, 4, 6, 4, 1], np.float32); kern /= kern.sum()
    for ax in (0, 1):
        tex = np.apply_along_axis(lambda r: np.convolve(r, kern, mode="same"), ax, tex)
    tex = (tex - tex.min()) / (tex.max() - tex.min()) * 255
    fill = rng.integers(0, 256, (H, W)).astype(np.uint8)
    with_box, box = scene_disparity()
    v = np.arange(H)[:, None]
    without = np.where(v > 20, 6 + np.round(0.45 * (v - 20)), 6).astype(np.int32) * np.ones((1, W), np.int32)
    (d / "image_2").mkdir(parents=True); (d / "image_3").mkdir()
    x = np.arange(W)[None, :].astype(np.float64)
    for i in range(n_img):
        there = i <= BOX_GONE_FROM
        dmap = with_box if there else without
        s = x - dmap + np.where(box & there, 0.0, i * k * dmap) + 100.0
        left = np.stack([np.interp(s[r], np.arange(tex.shape[1]), tex[r]) for r in range(H)]).round().astype(np.uint8)
        right = fill.copy()
        for r in range(H):
            xr = np.arange(W) - dmap[r]
            ok = xr >= 0
            right[r, xr[ok]] = left[r, ok]
        Image.fromarray(np.stack([left, left, left], -1), "RGB").save(d / "image_2" / f"{i:06d}.png"); Image.fromarray(right, "L").save(d / "image_3" / f"{i:06d}.png")


def test_mapper_switch_and_both_cloud_routes(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL)
    seq = tmp_path / "seq"
    write_leaving_sequence(seq, 11)
    out = subprocess.run([os.path.join(HOST, "test_carve"), os.path.join(HOST, "parameters_test.txt"), str(seq), str(BOX_GONE_FROM)], capture_output=True, text=True, timeout=300)
    print(out.stdout[-4000:], out.stderr[-2000:])
    for name in ("switch_defaults_to_off", "sequence_has_frames", "tracking_is_repeatable", "switch_off_clouds_as_before", "without_carving_the_box_is_in_every_cloud_until_it_leaves",
                 "routes_agree", "routes_record_the_same_figures", "carving_is_the_host_function_view_after_view", "counters_stay_beside_the_host_clouds",
                 "every_box_point_two_later_views_see_through_is_gone", "every_copy_of_the_box_loses_most_of_its_points",
                 "with_a_window_of_one_nothing_deep_inside_the_box_leaves", "without_carving_the_trail_is_in_the_published_map",
                 "after_the_rebuild_no_voxel_is_left_in_the_trail", "the_last_key_frame_is_whole", "the_static_scene_loses_a_small_share"):
        assert "PASS " + name in out.stdout, out.stdout[-4000:] + out.stderr[-2000:]
    assert out.returncode == 0 and "ALL PASSED" in out.stdout


def test_exp_mapping_carve_is_the_same_per_frame_and_batched(tmp_path):
    """--carve appends carve_keyframes / carve_tested / carve_removed / carve_fnv to the summary line, the same for the per-frame loop and --batched; without the
    flag the line has none of them and everything else on it is the same"""
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
    a = _run_exp_mapping(base, tmp_path, "a", "--carve")
    b = _run_exp_mapping(base, tmp_path, "b", "--carve", "--batched")
    c = _run_exp_mapping(base, tmp_path, "c")
    assert all(k in a for k in FIELDS) and all(k in b for k in FIELDS) and not any(k in c for k in FIELDS)
    assert [a[k] for k in FIELDS] == [b[k] for k in FIELDS]
    assert a["pose_fnv"] == b["pose_fnv"] == c["pose_fnv"] and a["keyframes"] == b["keyframes"] == c["keyframes"] and int(a["frames"]) == 8
    kf, tested, removed = int(a["carve_keyframes"]), int(a["carve_tested"]), int(a["carve_removed"])
    assert kf == int(a["keyframes"]) - 1 > 0 and 0 < removed < tested
    assert [k for k in a if not k.startswith("carve_")] == list(c)          # the flag only appends its four fields
