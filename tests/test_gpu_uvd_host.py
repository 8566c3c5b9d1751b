"""The U/V-disparity stage through the C++ host classes on a real MI355X: host/test_uvd.cpp (Tracker with uv_disparity=1 against BatchStereoTracker, chunks
that split the sequence; uv_disparity=0 leaves everything as it was) and the exp_mapping driver's --moving mode per frame and --batched, on a synthetic
KITTI-layout stereo sequence written here: a ground plane whose disparity grows with the row, a far background, and a box that does not follow the
ego-motion."""
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "semantic_slam_mapping_amd", "host")
pytestmark = pytest.mark.gpu
W, H = 400, 120


def scene_disparity():
    """rows above 20: background (6); below: the ground, 6 + 0.45 (v - 20), up to 51; a box of disparity 40 standing where the ground has 40"""
    v = np.arange(H)[:, None]
    d = np.where(v > 20, 6 + np.round(0.45 * (v - 20)), 6).astype(np.int32) * np.ones((1, W), np.int32)
    box = np.zeros((H, W), bool)
    box[30:96, 150:230] = True
    d[box] = 40
    return d, box


def write_sequence(d, n_img, rgb_left=False, k=0.05, seed=77, jump_at=None):
    """n_img stereo pairs under d/image_2, d/image_3: the static scene's texture slides by k x disparity per image (a sideways camera translation), the box keeps
    its place in the image -- it moves with the camera, so its features are outliers of the ego-motion.  The right image is the left one warped by the disparity"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    tex = rng.integers(0, 256, (H, W + 400)).astype(np.float32)
    kern = np.array([1, 4, 6, 4, 1], np.float32); kern /= kern.sum()
    for ax in (0, 1):
        tex = np.apply_along_axis(lambda r: np.convolve(r, kern, mode="same"), ax, tex)
    tex = (tex - tex.min()) / (tex.max() - tex.min()) * 255
    fill = rng.integers(0, 256, (H, W)).astype(np.uint8)
    dmap, box = scene_disparity()
    (d / "image_2").mkdir(parents=True); (d / "image_3").mkdir()
    x = np.arange(W)[None, :].astype(np.float64)
    for i in range(n_img):
        s = x - dmap + np.where(box, 0.0, i * k * dmap) + 100.0 + (150.0 if jump_at is not None and i >= jump_at else 0.0)   # (jump_at: the whole view jumps by 150 px)
        left = np.stack([np.interp(s[r], np.arange(tex.shape[1]), tex[r]) for r in range(H)]).round().astype(np.uint8)
        right = fill.copy()
        for r in range(H):
            xr = np.arange(W) - dmap[r]
            ok = xr >= 0
            right[r, xr[ok]] = left[r, ok]
        L = np.stack([left, left, left], -1) if rgb_left else left
        Image.fromarray(L, "RGB" if rgb_left else "L").save(d / "image_2" / f"{i:06d}.png"); Image.fromarray(right, "L").save(d / "image_3" / f"{i:06d}.png")


def test_tracker_and_bulk_tracker_give_the_same_masks(tmp_path):
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL)
    seq = tmp_path / "seq"
    write_sequence(seq, 7)
    jump = tmp_path / "seq_jump"
    write_sequence(jump, 9, jump_at=4)
    out = subprocess.run([os.path.join(HOST, "test_uvd"), os.path.join(HOST, "parameters_test.txt"), str(seq), str(jump)], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:], out.stderr[-2000:])
    for name in ("uvd_sequence_has_six_frames", "uvd_tracker_and_bulk_tracker_give_the_same_masks_and_pitches", "uvd_stage_ran_and_found_a_ground_line",
                 "uvd_poses_do_not_depend_on_the_stage", "uvd_off_leaves_the_masks_empty", "uvd_some_frame_keeps_a_mask",
                 "uvd_bulk_tracker_redo_path_equals_per_frame_tracker"):
        assert "PASS " + name in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
    assert out.returncode == 0 and "ALL PASSED" in out.stdout


def test_exp_mapping_moving_is_the_same_per_frame_and_batched(tmp_path):
    """--moving appends moving_pixels / moving_fnv / pitch_fnv to the summary line, the same for the per-frame loop and --batched; without it the line is as before"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_host_cpp import _run_exp_mapping
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL)
    seq = tmp_path / "kitti"
    write_sequence(seq, 9, rgb_left=True)
    base = open(os.path.join(HOST, "parameters_test.txt")).read().replace("end_index=8", "end_index=50").replace("dataset=synthetic", "dataset=kitti")
    base = base.replace("map_output=/tmp/ssm_test_map.pcd", f"map_output={tmp_path}/map.pcd")
    base += (f"\ndata_source={seq}\ntracker_mode=stereo\nimage_width=400\nimage_height=120\norb_levels=3\norb_features=300\ncamera.baseline=0.532331858\n"
             "camera.roix=2000\ncamera.roiy=2000\ncamera.roiz=4000\ninlier_threshold=2.0\ntracker_chunk=3\nssm_max_batch=3\nmapper_drain_ms=1000\n")
    a = _run_exp_mapping(base, tmp_path, "a", "--moving")
    b = _run_exp_mapping(base, tmp_path, "b", "--moving", "--batched")
    c = _run_exp_mapping(base, tmp_path, "c")
    assert "moving_fnv" in a and "moving_fnv" not in c
    assert (a["moving_pixels"], a["moving_fnv"], a["pitch_fnv"]) == (b["moving_pixels"], b["moving_fnv"], b["pitch_fnv"])
    assert a["pose_fnv"] == b["pose_fnv"] == c["pose_fnv"] and int(a["frames"]) == int(b["frames"]) == 8
    assert a["pitch_fnv"] != "cbf29ce484222325"              # the stage ran on some frame
    assert int(a["moving_pixels"]) > 0                       # and some frame keeps a mask: the segment phase of the bulk call has work
    prm = tmp_path / "rgbd.txt"
    prm.write_text(open(os.path.join(HOST, "parameters_test.txt")).read())
    r = subprocess.run([os.path.join(HOST, "exp_mapping"), str(prm), "--moving"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "needs tracker_mode=stereo" in r.stderr
