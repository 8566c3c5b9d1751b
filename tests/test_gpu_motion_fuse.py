"""The semantic-motion fusion on a real MI355X (ssm_motion_fuse*, csrc/kernels_motion_fuse.hip): device == ssm_motion_fuse_host byte for byte -- the mask, the
labels, the per-blob figures, the candidate image and the counters -- on the case list of tests/motion_fuse_ref.py, whose sizes and shapes sit around the
exported tile of the device labelling; per-frame and batched; and the equalities with the calls that exist: without motion the mask is ssm_moving_mask's and
the fused back-projection is ssm_backproject's, with motion it drops exactly the points under the fused mask.  tests/test_motion_fuse.py ties the host
function to the scipy restatement."""
import os
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import motion_fuse_ref as R  # noqa: E402
from conftest import CAM  # noqa: E402

pytestmark = pytest.mark.gpu
W, H = 640, 480
CASES = list(R.cases(64, 16))
_host = {}


@pytest.fixture(scope="module")
def gctx():
    import semantic_slam_mapping_amd as ssm
    c = ssm.Context(0, width=W, height=H, orb_features=500, max_batch=1, voxel_capacity_log2=12, camera=CAM)
    yield c
    c.close()


def host_of(key, case):
    """what the host function gives for a case, computed once"""
    if key not in _host:
        import semantic_slam_mapping_amd as ssm
        _host[key] = ssm.motion_fuse_host(*case, record=True)
    return _host[key]


def assert_equal(got, ref, what):
    for k in ("cand", "labels", "area", "overlap"):
        assert np.array_equal(got[2][k], ref[2][k]), (what, k)
    assert dict(got[1]) == dict(ref[1]), (what, got[1], ref[1])
    assert np.array_equal(got[0], ref[0]), (what, "mask")


@pytest.mark.parametrize("name", CASES + list(R.FULL))
def test_device_equals_host(gctx, name):
    import semantic_slam_mapping_amd as ssm
    case = (R.FULL[name] if name in R.FULL else R.cases(*ssm.motion_fuse_tile())[name])()
    assert_equal(gctx.motion_fuse(*case, record=True), host_of(name, case), name)


def test_batch_of_different_frames(gctx):
    """n = 3 through the device-resident call: every frame equals the host function on that frame (frame offsets of every workspace); then a smaller and a larger
    call on the same context (the workspaces are reused, then grown)"""
    frames = R.BATCH()
    sem = np.stack([f[0] for f in frames]); motion = np.stack([f[1] for f in frames])
    at, ot = frames[0][2], frames[0][3]
    mask, info, rec = gctx.motion_fuse(sem, motion, at, ot, record=True)
    for i, f in enumerate(frames):
        ref = host_of(("batch", i), (f[0], f[1], at, ot))
        assert_equal((mask[i], {k: int(info[i][k]) for k in info.dtype.names}, rec[i]), ref, i)
    assert len({m.tobytes() for m in mask}) == 3
    mask0, info0 = gctx.motion_fuse(sem[:1], None, at, ot)
    assert np.array_equal(mask0[0], host_of(("batch0", 0), (frames[0][0], None, at, ot))[0]) and int(info0[0]["confirmed"]) == 0
    big = R.random_case(131, 70, 99)
    sem5 = np.stack([big[0]] * 5); mot5 = np.stack([big[1]] * 5)
    mask5, info5 = gctx.motion_fuse(sem5, mot5, big[2], big[3])
    ref = host_of("big", big)
    assert all(np.array_equal(m, ref[0]) for m in mask5) and all(int(i["blobs"]) == ref[1]["blobs"] for i in info5)


def scene():
    """a 640 x 480 frame: class regions, a motion mask over some of them, depth everywhere"""
    sem, motion, _, _ = R.full_size(W, H, 21)
    sem[(sem == 128).all(-1)] = (128, 64, 128)          # Road in the place of Sky, which the back-projection drops whatever the mask says
    rng = np.random.default_rng(3)
    depth = rng.integers(500, 9000, (H, W)).astype(np.uint16)
    depth[rng.random((H, W)) < 0.1] = 0
    rgb = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    return sem, motion, depth, rgb


def test_without_motion_it_is_the_moving_mask(gctx):
    sem, motion, depth, rgb = scene()
    want = gctx.moving_mask(sem)
    assert want.any()
    for m in (None, np.zeros((H, W), np.uint8), np.full((H, W), 254, np.uint8)):
        mask, info = gctx.motion_fuse(sem, m)
        assert np.array_equal(mask, want) and info["confirmed"] == 0 and info["added"] == 0 and info["blobs"] > 0


def test_backproject_fused(gctx):
    sem, motion, depth, rgb = scene()
    T = np.eye(4); T[:3, 3] = (0.5, -0.25, 2.0)
    plain = gctx.generate_point_cloud(depth, rgb, sem, T)
    assert gctx.backproject_fused(depth, rgb, sem, None, T).tobytes() == plain.tobytes()
    cl = gctx.backproject_fused(depth, rgb, sem, None, device=True)
    ref = gctx.backproject_dev(depth, rgb, sem)
    assert gctx.cloud_fetch(cl, T).tobytes() == gctx.cloud_fetch(ref, T).tobytes() == plain.tobytes()
    gctx.cloud_free(cl); gctx.cloud_free(ref)
    # with motion: exactly the points under the fused mask go.  A point keeps its pixel's colour, so with a colour image that encodes the pixel index the
    # surviving pixels can be read off the cloud
    idx = np.arange(W * H, dtype=np.uint32).reshape(H, W)
    code = np.stack([idx & 255, (idx >> 8) & 255, idx >> 16], -1).astype(np.uint8)
    mask, info = gctx.motion_fuse(sem, motion)
    always = gctx.moving_mask(sem)
    assert info["confirmed"] > 0 and info["added"] == int(((mask == 255) & (always == 0)).sum()) > 0
    pix = lambda pts: pts["b"].astype(np.int64) | (pts["g"].astype(np.int64) << 8) | (pts["r"].astype(np.int64) << 16)  # noqa: E731
    before = gctx.generate_point_cloud(depth, code, sem, T)
    fused = gctx.backproject_fused(depth, code, sem, motion, T)
    keep = mask.reshape(-1)[pix(before)] == 0
    assert 0 < keep.sum() < len(before) and fused.tobytes() == before[keep].tobytes()
    cl = gctx.backproject_fused(depth, code, sem, motion, device=True)
    assert gctx.cloud_fetch(cl, T).tobytes() == fused.tobytes()
    gctx.cloud_free(cl)
