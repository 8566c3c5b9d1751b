"""The statistical outlier removal on a real MI355X (ssm_sor_filter, ssm_cloud_sor, csrc/kernels_sor.hip): device == ssm_sor_filter_host byte for byte -- the
kept points, every point's mean distance, the keep flags and every info field, the levels of the ladder included -- on the case list of tests/sor_ref.py and
under the four first cell sizes; on back-projected frames of key-frame size (device against host only: tests/test_sor.py ties the host function to the
brute force); on one context after a larger and before a larger call; and on a device-resident cloud.  The double sqrt of the contract is decided here: the
mean distances are compared as bits."""
import os
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sor_ref as R  # noqa: E402
from conftest import CAM  # noqa: E402

pytestmark = pytest.mark.gpu
W, H = 640, 480
CASES = list(R.cases(512))
_host = {}


@pytest.fixture(scope="module")
def gctx():
    import semantic_slam_mapping_amd as ssm
    c = ssm.Context(0, width=W, height=H, orb_features=500, max_batch=1, voxel_capacity_log2=12, camera=CAM)
    yield c
    c.close()


def case_of(name):
    import semantic_slam_mapping_amd as ssm
    return R.cases(ssm.sor_chunk())[name]()


def host_of(key, pts, k, mul, cell):
    """what the host function gives, computed once"""
    if key not in _host:
        import semantic_slam_mapping_amd as ssm
        _host[key] = ssm.sor_filter_host(pts, k, mul, cell, record=True)
    return _host[key]


def assert_equal(got, ref, what):
    assert dict(got[1]) == dict(ref[1]), (what, got[1], ref[1])
    assert np.array_equal(got[2]["mean_dist"].view(np.uint32), ref[2]["mean_dist"].view(np.uint32)), (what, "mean_dist")
    assert np.array_equal(got[2]["keep"], ref[2]["keep"]), (what, "keep")
    assert got[0].tobytes() == ref[0].tobytes(), (what, "points")


@pytest.mark.parametrize("name", CASES)
def test_device_equals_host(gctx, name):
    pts, k, mul, cell = case_of(name)
    got = gctx.sor_filter(pts, k, mul, cell, record=True)
    assert_equal(got, host_of(name, pts, k, mul, cell), name)
    assert got[0].tobytes() == pts[got[2]["keep"] == 1].tobytes()          # a kept point is untouched in all 32 bytes, and in its place


@pytest.mark.parametrize("name", ["random_3000", "duplicates", "non_finite", "doubling_line", "far_clusters", "k_cluster_beside_far", "cell_multiples", "k_64", "frame_160x120"])
def test_first_cell_sizes(gctx, name):
    pts, k, mul, _ = case_of(name)
    base = host_of(name, pts, k, mul, case_of(name)[3])
    for cell in R.CELLS:
        got = gctx.sor_filter(pts, k, mul, cell, record=True)
        assert_equal(got, host_of((name, cell), pts, k, mul, cell), f"{name} cell {cell}")
        assert got[0].tobytes() == base[0].tobytes() and np.array_equal(got[2]["mean_dist"].view(np.uint32), base[2]["mean_dist"].view(np.uint32))


@pytest.mark.parametrize("size", [(640, 480), (1241, 376)])
def test_key_frame_sizes(gctx, size):
    pts, speckles = R.backprojected(size[0], size[1], seed=size[0], speckles=200)
    got = gctx.sor_filter(pts, record=True)
    assert_equal(got, host_of(size, pts, 30, 1.0, 0.0), str(size))
    assert 0.8 * len(pts) < got[1]["n_kept"] < len(pts) and got[2]["keep"][speckles].mean() < 0.2


def test_small_after_large_and_large_after_small():
    """the workspaces are reused by a smaller call and grown by a larger one (a context of its own: the first call sizes them)"""
    import semantic_slam_mapping_amd as ssm
    c = ssm.Context(0, width=W, height=H, orb_features=500, max_batch=1, voxel_capacity_log2=12, camera=CAM)
    try:
        for name in ("k_8", "random_3000", "n_31", "one_cell", "n_0", "duplicates"):
            pts, k, mul, cell = case_of(name)
            assert_equal(c.sor_filter(pts, k, mul, cell, record=True), host_of(name, pts, k, mul, cell), name)
    finally:
        c.close()


def test_cloud_sor_is_the_filter_on_the_backprojection(gctx):
    """ssm_cloud_sor on the cloud of ssm_backproject_dev, fetched, is ssm_sor_filter on the output of ssm_backproject"""
    from oracle.binding import Oracle
    bgr, dep, sem, _, T = Oracle().synth_frame(0x5EED0000, 0)
    dep = dep.copy()
    rng = np.random.default_rng(5)
    at = rng.choice(dep.size, 300, replace=False)
    dep.reshape(-1)[at] = rng.integers(400, 700, 300)          # depth speckles
    plain = gctx.generate_point_cloud(dep, bgr, sem)
    want = gctx.sor_filter(plain, record=True)
    cl = gctx.backproject_dev(dep, bgr, sem)
    try:
        assert gctx.cloud_size(cl) == len(plain)
        info, rec = gctx.cloud_sor(cl, record=True)
        assert info == want[1] and gctx.cloud_size(cl) == info["n_kept"] < len(plain)
        assert np.array_equal(rec["keep"], want[2]["keep"]) and np.array_equal(rec["mean_dist"].view(np.uint32), want[2]["mean_dist"].view(np.uint32))
        assert gctx.cloud_fetch(cl).tobytes() == want[0].tobytes()
        assert gctx.cloud_fetch(cl, T).tobytes() == gctx.generate_point_cloud(dep, bgr, sem, T)[rec["keep"] == 1].tobytes()          # the pose is applied after the filter
    finally:
        gctx.cloud_free(cl)


def test_refusals_on_the_device(gctx):
    import semantic_slam_mapping_amd as ssm
    pts = R.cloud(R._uniform(100, 20))
    for kw in (dict(mean_k=0), dict(mean_k=65), dict(cell=-1.0), dict(stddev_mul=float("nan"))):
        with pytest.raises(ssm.SsmError) as e:
            gctx.sor_filter(pts, **kw)
        assert e.value.code == -1, kw
    far = R.cloud(np.float32([[0, 0, 0], [10000, 0, 0], [0, 10000, 0], [0, 0, 10000], [10000, 10000, 0]]))
    with pytest.raises(ssm.SsmError) as e:
        gctx.sor_filter(far, mean_k=2)
    assert e.value.code == -1
    out, info = gctx.sor_filter(pts)          # and the context goes on
    assert info["n_kept"] == len(out) > 0
