"""Dense alignment on a real MI355X (ssm_align_view_create, ssm_align_points, ssm_align_clouds, csrc/kernels_align.hip): device == ssm_align_host byte for
byte -- the view's valid mask and normals, every iteration's raw sums, counts and E through ssm_debug_align_record, the final E, T_view_out and every info
field -- on the case list of tests/align_cases.py (tests/test_align.py ties the host function to the restatement), at the sizes around a wave and a block and
one point beyond a pass of the persistent grid, on 1, 2, 3 and 7 device-resident clouds whose boundaries fall inside a wave and inside a block and whose sizes
include 0, in reversed order, at stride 1 and 3, at key-frame size, after ssm_cloud_sor and ssm_carve, with the clouds unchanged, on a reused context, and
the refusals."""
import os
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import align_ref as A  # noqa: E402
import align_cases as AC  # noqa: E402
import carve_ref as CR  # noqa: E402
from conftest import CAM  # noqa: E402

pytestmark = pytest.mark.gpu
W, H = 640, 480
BLOCK = 256          # csrc/kernels_align.hip ALIGN_T
CASES = list(AC.cases())
CAM4 = (CAM[0] / 4, CAM[1] / 4, CAM[2] / 4, CAM[3] / 4, CAM[4])
LOOSE = dict(min_inliers=20, max_iterations=5)
_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


@pytest.fixture(scope="module")
def c():
    import semantic_slam_mapping_amd as ssm
    x = ssm.Context(0, width=W, height=H, orb_features=500, max_batch=1, voxel_capacity_log2=12, camera=CAM)
    yield x
    x.close()


def host(cs, clouds=None, **kw):
    import semantic_slam_mapping_amd as ssm
    cl = cs["clouds"] if clouds is None else clouds
    return ssm.align_host(cs["depth"], cs["camera"], cs["T_view"], cl, cs["T_clouds"][:len(cl)], **dict(cs["params"], **kw))


def assert_equal(got, rec, ref, what, normals=None):
    """got: the device call's {T_view, info}; rec: its record; normals: (valid, normals) of its view"""
    if normals is not None:
        assert np.array_equal(normals[0], ref["valid"]), what
        assert normals[1].tobytes() == ref["normals"].tobytes(), what
    assert len(rec) == len(ref["record"]) == got["info"]["iterations"], (what, len(rec), len(ref["record"]))
    for it in range(len(rec)):
        assert rec[it]["sums"].tolist() == ref["record"][it]["sums"].tolist(), (what, it, rec[it]["sums"].tolist(), ref["record"][it]["sums"].tolist())
        assert rec[it]["E"].tobytes() == ref["record"][it]["E"].tobytes(), (what, it)
    for f in A.INFO_FIELDS:
        assert got["info"][f] == ref["info"][f], (what, f, got["info"][f], ref["info"][f])
    assert got["info"]["E"].tobytes() == ref["info"]["E"].tobytes(), what
    assert got["T_view"].tobytes() == ref["T_view"].tobytes(), what


def dev_points(c, cs, clouds=None, check_normals=True, **kw):
    """the case through ssm_align_points on a view of its own -> (result, record, (valid, normals))"""
    cl = cs["clouds"] if clouds is None else clouds
    P = dict(cs["params"], **kw)
    gate = {k: P[k] for k in ("tol_abs", "tol_rel_ppm") if k in P}
    v = c.align_view(cs["depth"], cs["camera"], **gate)
    try:
        got = c.align_points(v, cs["T_view"], cl, cs["T_clouds"][:len(cl)], **P)
        return got, c.align_record(), c.align_normals(v) if check_normals else None
    finally:
        c.align_view_free(v)


@pytest.mark.parametrize("name", CASES)
def test_device_equals_host(c, name):
    cs = memo(name, AC.cases()[name])
    ref = memo(("host", name), lambda: host(cs))
    got, rec, nm = dev_points(c, cs)
    assert_equal(got, rec, ref, name, nm)


def pass_points():
    import semantic_slam_mapping_amd as ssm
    return int(ssm.load().ssm_debug_align_pass_points())


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, "pass+1"])
@pytest.mark.parametrize("stride", [1, 3])
def test_sizes_around_a_wave_a_block_and_a_pass(c, n, stride):
    cs = memo("room_67x35", AC.cases()["room_67x35"])
    base = np.concatenate(cs["clouds"])
    if n == "pass+1":
        n = pass_points() * stride + 1          # one used point more than the persistent grid covers in one pass
        assert pass_points() == 1024 * BLOCK
        kw = dict(LOOSE, max_iterations=2)
    else:
        n = n * stride
        kw = dict(LOOSE)
    pts = [np.resize(base[37::13], n) if n else base[:0]]          # (spread over the image, repeated beyond 358 points)
    ref = host(cs, pts, stride=stride, **kw)
    got, rec, _ = dev_points(c, cs, pts, check_normals=False, stride=stride, **kw)
    assert_equal(got, rec, ref, (n, stride))
    assert got["info"]["n_in"] == (n + stride - 1) // stride and (n < 63 * stride or got["info"]["tested_first"] > 0)


# ---- device-resident clouds
def scene(c):
    """a 640 x 480 scene, the pixels that become points, and colour / semantic images (palette colours, no moving class)"""
    def make():
        import render_ref as R
        d = CR.scene_depth(W, H, 21)
        rng = np.random.default_rng(2)
        bgr = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        pal = np.array(R.PALETTE, np.uint8)
        sem = pal[np.array([1, 4, 5, 6, 8])[rng.integers(0, 5, (H // 8, W // 8))]].repeat(8, 0).repeat(8, 1)
        nz = np.nonzero(d.reshape(-1))[0]
        return d, nz, bgr, np.ascontiguousarray(sem)
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


def view160(c):
    d = scene(c)[0]
    return np.ascontiguousarray(d[::4, ::4])


@pytest.mark.parametrize("sizes", [(300,), (100, 93), (40, 0, 150), (40, 0, 150, 66, 0, 257, 1), (0,), (0, 0, 5), (BLOCK, BLOCK), (BLOCK + 1, 2 * BLOCK - 1, 64)])
def test_device_clouds(c, sizes):
    """m device clouds against a 160 x 120 view == the host function on the fetched points, at stride 1 and 3; in reversed order the result is identical; the
    clouds themselves are untouched"""
    import semantic_slam_mapping_amd as ssm
    rng = np.random.default_rng(len(sizes) + sum(sizes))
    clouds, hp, poses = [], [], []
    dep = view160(c)
    v = c.align_view(dep, CAM4)
    try:
        for k, n in enumerate(sizes):
            cl, pts = sparse_cloud(c, n, 100 + k)
            clouds.append(cl); hp.append(pts); poses.append(CR.pose(rng, 0.004, 0.02))
        Tv = CR.pose(rng, 0.004, 0.02)
        for stride in (1, 3):
            kw = dict(LOOSE, stride=stride)
            ref = ssm.align_host(dep, CAM4, Tv, hp, poses, **kw)
            got = c.align_clouds(v, Tv, clouds, poses, **kw)
            rec = c.align_record()
            assert_equal(got, rec, ref, (sizes, stride), c.align_normals(v) if stride == 1 else None)
            assert got["info"]["n_in"] == sum((n + stride - 1) // stride for n in sizes) and (sum(sizes) < 200 or got["info"]["tested_first"] > 0)
            rev = c.align_clouds(v, Tv, clouds[::-1], poses[::-1], **kw)
            assert_equal(rev, c.align_record(), ref, (sizes, stride, "reversed"))
        assert [c.cloud_size(cl) for cl in clouds] == list(sizes)
        assert all(c.cloud_fetch(cl).tobytes() == p.tobytes() for cl, p in zip(clouds, hp))
    finally:
        c.align_view_free(v)
        for cl in clouds:
            c.cloud_free(cl)


def test_after_outlier_removal_and_after_carving_and_clouds_unchanged(c):
    """the clouds as ssm_cloud_sor and one ssm_carve leave them (shrunk in place, run counters set) align as the host function aligns their fetched points, and
    alignment changes neither their size, their bytes nor their run counters"""
    import semantic_slam_mapping_amd as ssm
    d, nz, bgr, sem = scene(c)
    rng = np.random.default_rng(5)
    clouds, poses = [], []
    dep = view160(c)
    v = c.align_view(dep, CAM4)
    try:
        for k in range(2):
            dk = np.zeros_like(d)
            dk[k::4, k::4] = d[k::4, k::4]
            dk.reshape(-1)[rng.choice(nz, 200, replace=False)] = 500          # speckles for the filter
            clouds.append(c.backproject_dev(dk, bgr, sem)); poses.append(CR.pose(rng, 0.004, 0.02))
        Tv = CR.pose(rng, 0.004, 0.02)
        before = [c.cloud_size(cl) for cl in clouds]
        for cl in clouds:
            c.cloud_sor(cl)
        assert all(c.cloud_size(cl) < b for cl, b in zip(clouds, before))
        hp = [c.cloud_fetch(cl).copy() for cl in clouds]
        got = c.align_clouds(v, Tv, clouds, poses, **LOOSE)
        assert_equal(got, c.align_record(), ssm.align_host(dep, CAM4, Tv, hp, poses, **LOOSE), "after sor")
        assert got["info"]["inliers_first"] > 1000
        far = np.clip(d[::8, ::8].astype(np.int64) + 900 * (np.arange(W // 8) % 16 < 9), 1, 65535).astype(np.uint16)          # stripes pushed back: seen through there
        cv = c.carve_view(far, (CAM[0] / 8, CAM[1] / 8, CAM[2] / 8, CAM[3] / 8, CAM[4]))
        try:
            infos = c.carve(cv, Tv, clouds, poses, min_votes=1)
        finally:
            c.carve_view_free(cv)
        assert all(0 < i["n_kept"] < len(p) for i, p in zip(infos, hp))
        hp = [c.cloud_fetch(cl).copy() for cl in clouds]
        runs = [c.cloud_run(cl).copy() for cl in clouds]
        got = c.align_clouds(v, Tv, clouds, poses, **LOOSE)
        assert_equal(got, c.align_record(), ssm.align_host(dep, CAM4, Tv, hp, poses, **LOOSE), "after carving")
        assert [c.cloud_size(cl) for cl in clouds] == [len(p) for p in hp]
        assert all(c.cloud_fetch(cl).tobytes() == p.tobytes() for cl, p in zip(clouds, hp))
        assert all(np.array_equal(c.cloud_run(cl), r) for cl, r in zip(clouds, runs))
    finally:
        c.align_view_free(v)
        for cl in clouds:
            c.cloud_free(cl)


def full_frame(w, h):
    """a full cloud of a key-frame's size against a view of that size: the room at 640 x 480, the road under KITTI's camera at 1241 x 376"""
    def make():
        if w == 640:
            camera, scn, Tt, Tc = (319.5, 239.5, 520.0, 520.0, 1000.0), AC.ROOM, AC.VIEW, AC.NEAR[0]
        else:
            camera, scn, Tt, Tc = (607.2, 185.2, 718.9, 718.9, 1000.0), AC.ROAD, AC.se3(ry=0.02, tz=0.8), AC.se3()
        cs = AC.make(scn, w, h, camera, Tt, AC.se3(rx=0.004, ry=-0.005, ty=0.02, tz=0.03), [Tc], max_iterations=3)
        return cs, host(cs)
    return memo(("full", w, h), make)


@pytest.mark.parametrize("size", [(640, 480), (1241, 376)])
def test_key_frame_sizes(c, size):
    cs, ref = full_frame(*size)
    got, rec, nm = dev_points(c, cs)
    assert_equal(got, rec, ref, str(size), nm)
    # (a guard of the scene, not of the library: a cloud of most of the frame, most of which the view tests)
    assert ref["info"]["n_in"] > 0.4 * size[0] * size[1] and ref["info"]["inliers_first"] > 0.5 * ref["info"]["n_in"], ref["info"]


def test_small_after_large_and_a_second_view():
    """the context's table and staging are reused by a smaller call and grown by a larger one; two views live side by side (a context of its own: the first
    call sizes the workspaces)"""
    import semantic_slam_mapping_amd as ssm
    x = ssm.Context(0, width=W, height=H, orb_features=500, max_batch=1, voxel_capacity_log2=12, camera=CAM)
    try:
        assert len(x.align_record()) == 0
        small = memo("room_67x35", AC.cases()["room_67x35"]); rs = memo(("host", "room_67x35"), lambda: host(small))
        big, rb = full_frame(640, 480)
        v1 = x.align_view(small["depth"], small["camera"]); v2 = x.align_view(big["depth"], big["camera"])
        try:
            for cs, ref, v in ((small, rs, v1), (big, rb, v2), (small, rs, v1), (big, rb, v2)):
                got = x.align_points(v, cs["T_view"], cs["clouds"], cs["T_clouds"], **cs["params"])
                assert_equal(got, x.align_record(), ref, "reuse", x.align_normals(v))
        finally:
            x.align_view_free(v1); x.align_view_free(v2)
    finally:
        x.close()


def test_refusals_on_the_device(c):
    import semantic_slam_mapping_amd as ssm
    cs = memo("room_67x35", AC.cases()["room_67x35"])
    nan = float("nan")
    for kw in (dict(max_iterations=0), dict(max_iterations=65), dict(stride=0), dict(z_min=-1.0), dict(z_max=float("inf")), dict(dist_max=nan), dict(delta=-1.0), dict(damping=nan),
               dict(min_inliers=-1), dict(max_angle=4.0), dict(z_max=1.0e9)):
        with pytest.raises(ssm.SsmError) as e:
            dev_points(c, cs, check_normals=False, **kw)
        assert e.value.code == -1, kw
    for kw in (dict(tol_abs=nan), dict(tol_abs=-1.0), dict(tol_rel_ppm=-1), dict(tol_rel_ppm=1000001)):
        with pytest.raises(ssm.SsmError) as e:
            c.align_view(cs["depth"], cs["camera"], **kw)
        assert e.value.code == -1, kw
    for cam in ((0, 0, 64, 64, 0.0), (0, 0, nan, 64, 1000.0), (0, 0, 64, 64, 2e6)):
        with pytest.raises(ssm.SsmError) as e:
            c.align_view(cs["depth"], cam)
        assert e.value.code == -1, cam
    for shape in ((2, 67), (35, 2)):
        with pytest.raises(ssm.SsmError) as e:
            c.align_view(np.zeros(shape, np.uint16), cs["camera"])
        assert e.value.code == -1, shape
    bad = np.eye(4)
    bad[0, 0] = nan
    cl, pts = sparse_cloud(c, 10, 1)
    v = c.align_view(cs["depth"], cs["camera"])
    try:
        for args in ((v, bad, [cl], [np.eye(4)]), (v, np.eye(4), [cl], [bad]), (v, np.eye(4), [cl, cl], [np.eye(4), np.eye(4)])):
            with pytest.raises(ssm.SsmError) as e:
                c.align_clouds(*args, **LOOSE)
            assert e.value.code == -1
        with pytest.raises(ssm.SsmError) as e:
            c.align_points(v, np.eye(4), [pts, pts], [np.eye(4), np.eye(4)], **LOOSE)          # one array twice
        assert e.value.code == -1
        with pytest.raises(ssm.SsmError) as e:
            c.align_points(v, bad, [pts], [np.eye(4)], **LOOSE)
        assert e.value.code == -1
        none = c.align_clouds(v, np.eye(4), [], [], **LOOSE)
        assert none["info"]["status"] == A.TOO_FEW and none["info"]["n_in"] == 0 and len(c.align_record()) == 1
    finally:
        c.align_view_free(v)
        c.cloud_free(cl)
    got, rec, nm = dev_points(c, cs)
    assert_equal(got, rec, memo(("host", "room_67x35"), lambda: host(cs)), "the context goes on", nm)
