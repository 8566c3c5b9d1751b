"""Free-space carving on a real MI355X (ssm_carve, ssm_carve_points, csrc/kernels_carve.hip): device == ssm_carve_host byte for byte -- the kept points, the
kept counters, every point's verdict and counter before the compaction and every info field -- on the case list of tests/carve_ref.py (tests/test_carve.py ties
the host function to the restatement), at the sizes around a wave and a block, on 1, 2 and 7 device-resident clouds whose boundaries fall inside a wave and
inside a block and whose sizes include 0, over several views in sequence, at key-frame size, on one context after a larger and before a larger call, and after
ssm_cloud_sor."""
import os
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import carve_ref as R  # noqa: E402
from conftest import CAM  # noqa: E402

pytestmark = pytest.mark.gpu
W, H = 640, 480
BLOCK = 256          # csrc/kernels_carve.hip CARVE_T
CASES = list(R.cases())
CAM8 = (CAM[0] / 8, CAM[1] / 8, CAM[2] / 8, CAM[3] / 8, CAM[4])
_memo = {}


@pytest.fixture(scope="module")
def gctx():
    import semantic_slam_mapping_amd as ssm
    c = ssm.Context(0, width=W, height=H, orb_features=500, max_batch=1, voxel_capacity_log2=12, camera=CAM)
    yield c
    c.close()


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def host(cs, pts=None, run=None, **kw):
    import semantic_slam_mapping_amd as ssm
    return ssm.carve_host(cs["depth"], cs["camera"], cs["T_view"], cs["pts"] if pts is None else pts, cs["T_cloud"], cs["run"] if run is None else run, record=True,
                          **dict(cs["params"], **kw))


def dev(c, cs, pts=None, run=None, **kw):
    return c.carve_points(cs["depth"], cs["camera"], cs["T_view"], cs["pts"] if pts is None else pts, cs["T_cloud"], cs["run"] if run is None else run, record=True,
                          **dict(cs["params"], **kw))


def assert_equal(got, ref, what):
    assert dict(got[2]) == dict(ref[2]), (what, got[2], ref[2])
    assert np.array_equal(got[3]["verdict"], ref[3]["verdict"]), (what, "verdict")
    assert np.array_equal(got[3]["run"], ref[3]["run"]), (what, "run")
    assert got[0].tobytes() == ref[0].tobytes(), (what, "points")
    assert np.array_equal(got[1], ref[1]), (what, "kept counters")


@pytest.mark.parametrize("name", CASES)
def test_device_equals_host(gctx, name):
    cs = memo(name, R.cases()[name])
    assert_equal(dev(gctx, cs), memo(("host", name), lambda: host(cs)), name)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1])
def test_sizes_around_a_wave_and_a_block(gctx, n):
    cs = memo("posed_160x120", R.cases()["posed_160x120"])
    pts, run = cs["pts"][100:100 + n], cs["run"][100:100 + n]
    for mv in (1, 2, 3):
        got = dev(gctx, cs, pts, run, min_votes=mv)
        assert_equal(got, host(cs, pts, run, min_votes=mv), (n, mv))
        assert got[2]["n_in"] == n


# ---- device-resident clouds
def scene(c):
    """a 640 x 480 scene, the pixels that become points (row-major, as the cloud has them), and colour / semantic images (road everywhere: no moving class)"""
    def make():
        d = R.scene_depth(W, H, 21)
        bgr = np.random.default_rng(2).integers(0, 256, (H, W, 3), dtype=np.uint8)
        sem = np.full((H, W, 3), (128, 64, 128), np.uint8)
        p = c.generate_point_cloud(d, bgr, sem)
        z = p["z"].astype(np.float64)
        at = np.rint(p["y"] * CAM[3] / z + CAM[1]).astype(np.int64) * W + np.rint(p["x"] * CAM[2] / z + CAM[0]).astype(np.int64)
        assert len(at) > 0.9 * W * H and (np.diff(at) > 0).all() and (d.reshape(-1)[at] > 0).all()
        return d, at, bgr, sem
    return memo("scene", make)


def sparse_cloud(c, k, seed):
    """a device cloud of exactly k points of the scene (spread over the image), and the same points on the host"""
    d, nz, bgr, sem = scene(c)
    dep = np.zeros_like(d)
    if k:
        at = np.sort(np.random.default_rng(seed).choice(nz, k, replace=False))
        dep.reshape(-1)[at] = d.reshape(-1)[at]
    cl = c.backproject_dev(dep, bgr, sem)
    pts = c.cloud_fetch(cl)
    assert c.cloud_size(cl) == k == len(pts)
    return cl, pts.copy()


def views(c, n):
    """n later views of the scene at an eighth of its size: the scene itself with more noise, one with a near wall (occludes), one far (seen through)"""
    d = scene(c)[0]
    rng = np.random.default_rng(9)
    out = []
    for i in range(n):
        v = d[::8, ::8].astype(np.int64)
        if i % 3 == 0:
            v = v + 900 * (np.arange(v.shape[1]) % 16 < 9)          # stripes of the scene pushed back: seen through there, supported between
        elif i % 3 == 1:
            v = v + rng.integers(-60, 60, v.shape)
        else:
            v[:, 30:50] = 900                                      # a near wall
        v = np.clip(v, 1, 65535).astype(np.uint16)
        v[d[::8, ::8] == 0] = 0
        out.append((v, R.pose(rng, 0.004, 0.02)))
    return out


@pytest.mark.parametrize("sizes", [(300,), (100, 93), (40, 0, 150, 66, 0, 257, 1), (0,), (0, 0, 5), (BLOCK, BLOCK), (BLOCK + 1, 2 * BLOCK - 1, 64)])
def test_clouds_in_sequence(gctx, sizes):
    """m clouds under four views in a row: after every view each cloud, its counters, the record and the info are the host function's on that cloud alone"""
    import semantic_slam_mapping_amd as ssm
    rng = np.random.default_rng(len(sizes))
    clouds, hp, hr, poses = [], [], [], []
    try:
        for k, n in enumerate(sizes):
            cl, pts = sparse_cloud(gctx, n, 100 + k)
            clouds.append(cl); hp.append(pts); hr.append(np.zeros(n, np.uint8)); poses.append(R.pose(rng, 0.004, 0.02))
        assert all((gctx.cloud_run(cl) == 0).all() for cl in clouds)
        removed = 0
        for dep, Tv in views(gctx, 4):
            view = gctx.carve_view(dep, CAM8)
            try:
                infos, recs = gctx.carve(view, Tv, clouds, poses, record=True)
            finally:
                gctx.carve_view_free(view)
            for k, cl in enumerate(clouds):
                p, r, info, rec = ssm.carve_host(dep, CAM8, Tv, hp[k], poses[k], hr[k], record=True)
                assert infos[k] == info, (k, infos[k], info)
                assert np.array_equal(recs[k]["verdict"], rec["verdict"]) and np.array_equal(recs[k]["run"], rec["run"]), k
                assert gctx.cloud_size(cl) == info["n_kept"] and gctx.cloud_fetch(cl).tobytes() == p.tobytes() and np.array_equal(gctx.cloud_run(cl), r), k
                hp[k], hr[k] = p, r
                removed += info["removed"]
        if sum(sizes) > 200:
            assert removed > 0 and sum(len(p) for p in hp) > 0
    finally:
        for cl in clouds:
            gctx.cloud_free(cl)


def test_see_through_support_see_through_keeps_the_point(gctx):
    pts = R.cloud([R.at_pixel(3, 3, 1.0), R.at_pixel(5, 3, 1.0)])
    far, near = np.full((6, 8), 3000, np.uint16), np.full((6, 8), 1000, np.uint16)
    mixed = far.copy()
    mixed[:, :4] = 1000          # supports the first point only
    p, run, info = gctx.carve_points(far, R.cam0(), R.EYE, pts, R.EYE)
    assert len(p) == 2 and run.tolist() == [1, 1]
    p, run, info = gctx.carve_points(mixed, R.cam0(), R.EYE, p, R.EYE, run)
    assert p.tobytes() == pts[:1].tobytes() and run.tolist() == [0] and info["removed"] == 1          # seen through twice: gone; supported: cleared
    p, run, info = gctx.carve_points(far, R.cam0(), R.EYE, p, R.EYE, run)
    assert len(p) == 1 and run.tolist() == [1]


def full_frame(w, h):
    def make():
        camera = (w / 2 - 0.3, h / 2 + 0.2, 0.8 * w, 0.8 * w, 1000.0)
        rng = np.random.default_rng(w)
        d0, d1 = R.scene_depth(w, h, w), R.scene_depth(w, h, w + 1)
        d1[:, w // 4: w // 3] += 1500          # a part of the scene has moved back: seen through
        pts = R.cloud(R.backproject(d0, camera), 3)
        cs = R.case(d1, pts, camera=camera, T_view=R.pose(rng, 0.004, 0.02), T_cloud=R.pose(rng, 0.004, 0.02), run=rng.integers(0, 2, len(pts)).astype(np.uint8))
        return cs, host(cs)
    return memo(("full", w, h), make)


@pytest.mark.parametrize("size", [(640, 480), (1241, 376)])
def test_key_frame_sizes(gctx, size):
    cs, ref = full_frame(*size)
    assert_equal(dev(gctx, cs), ref, str(size))
    info = ref[2]
    assert info["n_in"] > 0.9 * size[0] * size[1] and min(info[f] for f in ("unknown", "occluded", "supported", "seen_through", "removed")) > 0 and info["n_kept"] > 0.5 * info["n_in"]


def test_small_after_large_and_large_after_small():
    """the workspaces are reused by a smaller call and grown by a larger one (a context of its own: the first call sizes them)"""
    import semantic_slam_mapping_amd as ssm
    c = ssm.Context(0, width=W, height=H, orb_features=500, max_batch=1, voxel_capacity_log2=12, camera=CAM)
    try:
        for name in ("counters_votes2", "posed_160x120", "degenerate", (640, 480), "every_pixel_8x6_r0", "posed_70x9", (1241, 376), "all_removed"):
            if isinstance(name, tuple):
                cs, ref = full_frame(*name)
            else:
                cs = memo(name, R.cases()[name]); ref = memo(("host", name), lambda: host(cs))
            assert_equal(dev(c, cs), ref, str(name))
    finally:
        c.close()


def test_cloud_sor_then_carving_is_the_host_composition(gctx):
    """ssm_cloud_sor, then ssm_carve, on a device cloud == ssm_sor_filter_host, then ssm_carve_host; a cloud that has counters is refused by ssm_cloud_sor"""
    import semantic_slam_mapping_amd as ssm
    d, nz, bgr, sem = scene(gctx)
    dep = np.zeros_like(d)
    dep[::4, ::4] = d[::4, ::4]
    rng = np.random.default_rng(5)
    dep.reshape(-1)[rng.choice(nz, 200, replace=False)] = 500          # speckles for the filter
    plain = gctx.generate_point_cloud(dep, bgr, sem)
    filtered = ssm.sor_filter_host(plain)[0]
    (vd, Tv), Tc = views(gctx, 1)[0], R.pose(rng, 0.004, 0.02)
    want = ssm.carve_host(vd, CAM8, Tv, filtered, Tc, min_votes=1)
    cl = gctx.backproject_dev(dep, bgr, sem)
    view = gctx.carve_view(vd, CAM8)
    try:
        gctx.cloud_sor(cl)
        assert gctx.cloud_size(cl) == len(filtered) < len(plain)
        infos = gctx.carve(view, Tv, [cl], [Tc], min_votes=1)
        assert infos[0] == want[2] and 0 < infos[0]["n_kept"] < len(filtered)
        assert gctx.cloud_fetch(cl).tobytes() == want[0].tobytes() and np.array_equal(gctx.cloud_run(cl), want[1])
        with pytest.raises(ssm.SsmError) as e:
            gctx.cloud_sor(cl)
        assert e.value.code == -1
        assert gctx.cloud_fetch(cl).tobytes() == want[0].tobytes()
    finally:
        gctx.carve_view_free(view)
        gctx.cloud_free(cl)


def test_refusals_on_the_device(gctx):
    import semantic_slam_mapping_amd as ssm
    cs = memo("posed_70x9", R.cases()["posed_70x9"])
    for kw in (dict(min_votes=0), dict(min_votes=256), dict(radius=4), dict(radius=-1), dict(tol_abs=float("nan")), dict(tol_rel_ppm=-1), dict(z_min=float("inf"))):
        with pytest.raises(ssm.SsmError) as e:
            dev(gctx, cs, **kw)
        assert e.value.code == -1, kw
    cl, _ = sparse_cloud(gctx, 10, 1)
    view = gctx.carve_view(cs["depth"], cs["camera"])
    try:
        bad = np.eye(4)
        bad[0, 0] = float("nan")
        for args, kw in (((view, bad, [cl], [R.EYE]), {}), ((view, R.EYE, [cl], [bad]), {}), ((view, R.EYE, [cl, cl], [R.EYE, R.EYE]), {}), ((view, R.EYE, [cl], [R.EYE]), dict(radius=5))):
            with pytest.raises(ssm.SsmError) as e:
                gctx.carve(*args, **kw)
            assert e.value.code == -1
        assert gctx.cloud_size(cl) == 10 and gctx.carve(view, R.EYE, [], []) == []
        with pytest.raises(ssm.SsmError):
            gctx.carve_view(cs["depth"], (0, 0, 64, 64, 0.0))
    finally:
        gctx.carve_view_free(view)
        gctx.cloud_free(cl)
    assert_equal(dev(gctx, cs), memo(("host", "posed_70x9"), lambda: host(cs)), "the context goes on")
