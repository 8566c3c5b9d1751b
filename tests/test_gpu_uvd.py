"""The U/V-disparity moving-object stage on a real MI355X (ssm_uvd_*, csrc/kernels_uvd.hip): device == ssm_uvd_process_host byte for byte -- the three
masks, both intermediate images, the binary image, the union mask, every recorded stage, the edited matches and the whole ssm_uvd_info (floats by bits).
Both sides run include/ssm/uvd_core.h; tests/test_uvd.py ties the host function to the independent restatement."""
import os
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import uvd_ref as R  # noqa: E402
from conftest import CAM  # noqa: E402

pytestmark = pytest.mark.gpu
STAGES = (1, 2, 3, 4, 5, 7, 8, 9, 10)


@pytest.fixture(scope="module")
def gctx():
    import semantic_slam_mapping_amd as ssm
    c = ssm.Context(0, orb_features=500, max_batch=1, voxel_capacity_log2=12, camera=CAM)
    yield c
    c.close()


def small_scene(w, h, v_h, box, seed, slope=1.0, **kw):
    """a scene of another size: the horizon v_h and one box (first column, width, top row, disparity); the principal point sits on the horizon"""
    left, disp, m, fl = R.make_scene(seed, w=w, h=h, v_h=v_h, slope=slope, boxes=(box,), **kw)
    return left, disp, m, fl, R.scene_params(cu=w / 2 + 0.3, cv=float(v_h))


def host_sequence(P, frames):
    """frames: (left, disp, matches, flags, skip) -> what one host-only object gives for them in order, with images and stages"""
    import semantic_slam_mapping_amd as ssm
    u = ssm.UVDisparity(None, record=True, **P)
    out = []
    for left, disp, m, fl, skip in frames:
        r = u.process_host(left, disp, m, fl, skip=skip)
        h, w = disp.shape
        r["images"] = u.images(0, w, h); r["stages"] = {s: u.stage(0, s) for s in STAGES}
        out.append(r)
    u.close()
    return out


def assert_frame_equal(got, ref, what):
    for k in ("moving", "roi", "ground"):
        if got.get(k) is not None:
            assert np.array_equal(got[k], ref[k]), (what, k)
    assert got["info"].tobytes() == ref["info"].tobytes(), (what, got["info"], ref["info"])
    for k in ("v_dis", "u_dis", "bin", "union"):
        assert np.array_equal(got["images"][k], ref["images"][k]), (what, k)
    for s in STAGES:
        assert got["stages"][s].tobytes() == ref["stages"][s].tobytes(), (what, s)
    assert got["matches"].tobytes() == ref["matches"].tobytes() and np.array_equal(got["inlier_flags"], ref["inlier_flags"]), what


def device_one(u, left, disp, m, fl, skip=False):
    r = u.process(left, disp, m, fl, skip=skip)
    h, w = disp.shape
    r["images"] = u.images(0, w, h); r["stages"] = {s: u.stage(0, s) for s in STAGES}
    return r


@pytest.mark.parametrize("name", list(R.SCENES))
def test_every_condition_scene_equals_host(gctx, name):
    import semantic_slam_mapping_amd as ssm
    left, disp, m, fl, P = R.build_scene(name, border_matches=True)
    ref = host_sequence(P, [(left, disp, m, fl, False)])[0]
    u = ssm.UVDisparity(gctx, record=True, **P)
    assert_frame_equal(device_one(u, left, disp, m, fl), ref, name)
    u.close()
    if name == "moving":
        assert ref["info"]["n_masks_kept"] >= 1 and ref["info"]["n_moving"] > 0 and (ref["inlier_flags"] & 2).any()


SIZES = {
    "67x50_strided": (67, 50, 8, (10, 30, 4, 30), 5),
    "130x37_strided": (130, 37, 2, (40, 44, 1, 29), 3),
    "64x33": (64, 33, 1, (8, 40, 0, 28), 0),
}


@pytest.mark.parametrize("name", list(SIZES))
def test_sizes_around_the_tiles(gctx, name):
    """just above one and two 64-lane tiles with an odd width and stride > w; exactly one tile.  Matches on columns 0 and w - 1, rows 0 and h - 1"""
    import semantic_slam_mapping_amd as ssm
    w, h, v_h, box, pad = SIZES[name]
    left, disp, m, fl, P = small_scene(w, h, v_h, box, seed=21, border_matches=True, n_ground_inliers=3, holes=2, zero_pixels=9)
    ref = host_sequence(P, [(left, disp, m, fl, False)])[0]
    assert ref["info"]["status"] == 0 and ref["info"]["v_cols"] > 26
    wl = np.full((h, w + pad), 77, np.uint8); wd = np.full((h, w + pad), 31000, np.int16)
    wl[:, :w] = left; wd[:, :w] = disp
    u = ssm.UVDisparity(gctx, record=True, **P)
    assert_frame_equal(device_one(u, wl[:, :w], wd[:, :w], m, fl), ref, name)
    u.reset()
    ref0 = host_sequence(P, [(left, disp, None, None, False)])[0]
    assert_frame_equal(device_one(u, left, disp, None, None), ref0, name + " without matches")
    u.close()


@pytest.mark.parametrize("ndisp", (48, 80, 128))
def test_bin_counts(gctx, ndisp):
    import semantic_slam_mapping_amd as ssm
    slope = (ndisp - 1) / 55.0                   # the bottom row (55 below the horizon) reaches ndisp - 1
    d_box = int(0.7 * ndisp)
    left, disp, m, fl, P = small_scene(160, 96, 40, (56, 48, 30, d_box), seed=30 + ndisp, slope=slope, border_matches=True)
    ref = host_sequence(P, [(left, disp, m, fl, False)])[0]
    assert ref["info"]["status"] == 0 and ndisp - 2 <= ref["info"]["v_cols"] <= ndisp
    u = ssm.UVDisparity(gctx, record=True, **P)
    assert_frame_equal(device_one(u, left, disp, m, fl), ref, ndisp)
    u.close()


def seeds_on_the_border_scene():
    """boxes that touch columns 0 and w - 1, outliers on those columns: flood fills that start on the U-disparity image's border"""
    left, disp, m, fl = R.make_scene(40, boxes=((0, 40, 30, 40), (120, 40, 30, 33)), outliers_on=(0, 1), n_out=2)
    k = np.flatnonzero(fl == 0)
    m["u1c"][k[0]] = 0; m["u1c"][k[2]] = 159
    for i in (k[0], k[2]):
        m["u2c"][i] = m["u1c"][i] - max(int(disp[int(m["v1c"][i]), int(m["u1c"][i])]), 16) / 16.0
    return left, disp, m, fl, R.scene_params()


def test_seeds_on_the_image_border(gctx):
    import semantic_slam_mapping_amd as ssm
    left, disp, m, fl, P = seeds_on_the_border_scene()
    ref = host_sequence(P, [(left, disp, m, fl, False)])[0]
    assert ref["info"]["n_seeds"] >= 2 and ref["images"]["union"][:, 0].any() and ref["images"]["union"][:, 159].any()
    u = ssm.UVDisparity(gctx, record=True, **P)
    assert_frame_equal(device_one(u, left, disp, m, fl), ref, "border seeds")
    u.close()


def bulk_run(gctx, u, frames, w, h, null_masks=False):
    """frames through ssm_uvd_process_dev in one call -> per-frame results shaped like device_one's"""
    n = len(frames)
    cap = max([len(f[2]) for f in frames] + [1])
    M = np.zeros((n, cap), R.PMATCH); FL = np.zeros((n, cap), np.uint8); NM = np.zeros(n, np.int32)
    for i, (left, disp, m, fl, skip) in enumerate(frames):
        M[i, :len(m)] = m; FL[i, :len(fl)] = fl; NM[i] = -1 if skip else len(m)
    px = w * h
    d_left, d_disp = gctx.dev_alloc(n * px), gctx.dev_alloc(n * px * 2)
    gctx.h2d(d_left, np.stack([f[0] for f in frames])); gctx.h2d(d_disp, np.stack([f[1] for f in frames]))
    d_masks = [None] * 3 if null_masks else [gctx.dev_alloc(n * px) for _ in range(3)]
    info, M2, FL2 = u.process_dev(d_left, d_disp, n, w, h, M, NM, FL, *d_masks)
    masks = [None] * 3 if null_masks else [gctx.d2h(p, (n, h, w), np.uint8) for p in d_masks]
    out = []
    for i in range(n):
        k = len(frames[i][2])
        out.append(dict(moving=None if null_masks else masks[0][i], roi=None if null_masks else masks[1][i], ground=None if null_masks else masks[2][i], info=info[i],
                        matches=M2[i, :k], inlier_flags=FL2[i, :k], images=u.images(i, w, h), stages={s: u.stage(i, s) for s in STAGES}))
    for p in [d_left, d_disp] + [p for p in d_masks if p is not None]:
        gctx.dev_free(p)
    return out


def test_bulk_equals_one_at_a_time_and_host(gctx):
    """n = 1, n = 3 and n = 5: a skipped frame and a NO_LINE frame in the middle, a frame with cap matches beside one with none; the frames of a bulk call equal
    the same frames one at a time through a second object, and the host; NULL mask pointers; ssm_uvd_reset"""
    import semantic_slam_mapping_amd as ssm
    P = R.scene_params()
    S = {n: R.build_scene(n)[:4] for n in ("moving", "merge", "no_line", "exact_max", "verified_away")}
    none = (np.zeros(0, R.PMATCH), np.zeros(0, np.uint8))
    seqs = [
        [S["moving"] + (False,)],
        [S["moving"] + (False,), S["merge"] + (True,), S["exact_max"] + (False,)],
        [S["merge"] + (False,), S["no_line"] + (False,), S["verified_away"] + (False,)],
        [S["verified_away"] + (False,), S["exact_max"][:2] + none + (False,), S["no_line"] + (False,), S["moving"] + (True,), S["merge"] + (False,)],
    ]
    u, u1 = ssm.UVDisparity(gctx, record=True, **P), ssm.UVDisparity(gctx, record=True, **P)
    for frames in seqs:
        ref = host_sequence(P, frames)
        u.reset(); u1.reset()
        got = bulk_run(gctx, u, frames, 160, 96)
        for i, f in enumerate(frames):
            assert_frame_equal(got[i], ref[i], (len(frames), i))
            assert_frame_equal(device_one(u1, *f), ref[i], (len(frames), i, "one at a time"))
        statuses = [int(r["info"]["status"]) for r in ref]
        assert statuses == [R.SKIPPED if f[4] else (R.NO_LINE if f[1] is S["no_line"][1] else 0) for f in frames]
    # the same again without reset: the filters carry on, so the pitch differs; with reset and NULL masks: the first result
    frames = seqs[1]
    ref = host_sequence(P, frames)
    u.reset()
    a = bulk_run(gctx, u, frames, 160, 96)
    b = bulk_run(gctx, u, frames, 160, 96)
    assert a[0]["info"]["pitch_filtered"] != b[0]["info"]["pitch_filtered"] and a[0]["info"]["pitch_measured"] == b[0]["info"]["pitch_measured"]
    u.reset()
    c = bulk_run(gctx, u, frames, 160, 96, null_masks=True)
    for i in range(len(frames)):
        assert_frame_equal(c[i], ref[i], ("null masks", i))
    u.close(); u1.close()


def test_kitti_size_two_frames(gctx):
    """1241 x 376 once, n = 2: 20 column strips (the last with 25 columns), 376 rows, 80 disparities"""
    import semantic_slam_mapping_amd as ssm
    w, h = 1241, 376
    frames = []
    for seed in (51, 52):
        left, disp, m, fl = R.make_scene(seed, w=w, h=h, v_h=170, slope=0.38, boxes=((300, 150, 120, 45), (800, 200, 150, 30)), outliers_on=(0, 1), n_out=4,
                                         inliers_on=(1,) if seed == 52 else (), n_in=5, n_ground_inliers=40, holes=60, zero_pixels=500, border_matches=True)
        frames.append((left, disp, m, fl, False))
    P = R.scene_params(f=718.856, cu=607.1928, cv=170.0, base=0.54, roi_x=20.0, roi_y=5.0, roi_z=40.0)
    ref = host_sequence(P, frames)
    assert ref[0]["info"]["status"] == 0 and ref[0]["info"]["v_cols"] > 60 and ref[0]["info"]["n_masks_kept"] >= 1 and ref[0]["info"]["n_moving"] > 0
    u = ssm.UVDisparity(gctx, record=True, **P)
    got = bulk_run(gctx, u, frames, w, h)
    for i in range(2):
        assert_frame_equal(got[i], ref[i], ("kitti", i))
    u.close()


def test_destroy_returns_every_allocation(gctx):
    import semantic_slam_mapping_amd as ssm
    left, disp, m, fl, P = R.build_scene("moving")
    gctx.sync()
    before = ssm.live_allocations()
    u = ssm.UVDisparity(gctx, record=True, **P)
    device_one(u, left, disp, m, fl)
    bulk_run(gctx, u, [(left, disp, m, fl, False)] * 2, 160, 96, null_masks=True)
    assert ssm.live_allocations()[0] > before[0]
    u.close()
    assert ssm.live_allocations() == before
