"""The ground grid on a real MI355X (ssm_grid_points, ssm_grid_clouds, ssm_grid_viewer_map, csrc/kernels_grid.hip): device == ssm_grid_host byte for byte -- the
raw cells through ssm_debug_grid_cells, the seven fetched arrays, the info -- on the case list of tests/grid_cases.py (tests/test_grid.py ties the host function
to the restatement), at the point counts around a wave and a block, on 1, 2, 3 and 7 device-resident clouds whose boundaries fall inside a wave and inside a
block and whose sizes include 0, in reversed order, with thousands of points in one cell and two cells alternating lane by lane, after ssm_cloud_sor and
ssm_carve, on the viewer's map, on targets of several sizes on one context, a small build after a large one into one target, and once at full size."""
import os
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import grid_ref as R  # noqa: E402
import grid_cases as GC  # noqa: E402
import carve_ref as CR  # noqa: E402
from conftest import CAM  # noqa: E402

pytestmark = pytest.mark.gpu
W, H = 640, 480
BLOCK = 256          # csrc/kernels_grid.hip GRID_T
CASES = list(GC.cases())
# the wall scene of the carving tests under the default G: x across, depth forward, image rows become heights -- many points of one cloud per cell
WALL = dict(x0=-4.0, y0=0.0, cell=0.125, nx=64, ny=56, h_min=-3.0, h_max=3.0, ground_radius=2)
_memo = {}


class Ctx:
    """a context and its grid targets, one per size"""
    def __init__(self):
        import semantic_slam_mapping_amd as ssm
        self.c = ssm.Context(0, width=W, height=H, orb_features=500, max_batch=1, voxel_capacity_log2=12, camera=CAM)
        self.targets = {}

    def target(self, nx, ny):
        if (nx, ny) not in self.targets:
            self.targets[(nx, ny)] = self.c.grid_target(nx, ny)
        return self.targets[(nx, ny)]

    def close(self):
        for t in self.targets.values():
            self.c.grid_target_free(t)
        self.c.close()


@pytest.fixture(scope="module")
def g():
    x = Ctx()
    yield x
    x.close()


FORMS = [0, 1]          # csrc/kernels_grid.hip: one atomic per point and address; one per run of adjacent lanes with the same destination


@pytest.fixture
def form(request, g):
    """the accumulate form of the builds of one test, the default again afterwards"""
    g.c.grid_form(request.param)
    yield request.param
    g.c.grid_form(-1)


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def host(cs, clouds=None, **kw):
    import semantic_slam_mapping_amd as ssm
    cl = cs["clouds"] if clouds is None else clouds
    return ssm.grid_host(cl, cs["T_clouds"][:len(cl)], cells=True, **dict(cs["params"], **kw))


def dev(g, cs, clouds=None, target=None, **kw):
    cl = cs["clouds"] if clouds is None else clouds
    P = dict(cs["params"], **kw)
    return g.c.grid_points(g.target(P["nx"], P["ny"]) if target is None else target, cl, cs["T_clouds"][:len(cl)], cells=True, **P)


def assert_equal(got, ref, what):
    assert got["info"] == ref["info"], (what, got["info"], ref["info"])
    assert got["cells"].dtype == ref["cells"].dtype and got["cells"].shape == ref["cells"].shape, what
    if got["cells"].tobytes() != ref["cells"].tobytes():
        for f in ref["cells"].dtype.names:
            assert np.array_equal(got["cells"][f], ref["cells"][f]), (what, "cells." + f, np.argwhere(got["cells"][f] != ref["cells"][f])[:5])
    for f in R.ARRAYS:
        assert got[f].dtype == ref[f].dtype and got[f].shape == ref[f].shape and got[f].tobytes() == ref[f].tobytes(), (what, f, np.argwhere(got[f] != ref[f])[:5])


@pytest.mark.parametrize("form", FORMS, indirect=True)
@pytest.mark.parametrize("name", CASES)
def test_device_equals_host(g, name, form):
    cs = memo(name, GC.cases()[name])
    assert_equal(dev(g, cs), memo(("host", name), lambda: host(cs)), name)


def wall_points():
    """the carving tests' 160 x 120 wall scene as one host cloud with labels, under a pose"""
    def make():
        rng = np.random.default_rng(4)
        xyz = CR.backproject(CR.scene_depth(160, 120, 3), (79.7, 60.2, 128.0, 128.0, 1000.0))
        pts = np.zeros(len(xyz), R.POINT_DTYPE)
        pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
        pts["label"] = rng.integers(0, 13, len(pts))
        return GC.case([pts], WALL, [CR.pose(rng, 0.01, 0.05)])
    return memo("wall", make)


@pytest.mark.parametrize("form", FORMS, indirect=True)
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1])
def test_sizes_around_a_wave_and_a_block(g, n, form):
    cs = wall_points()
    pts = [cs["clouds"][0][5000:5000 + n]]
    got = dev(g, cs, pts)
    assert_equal(got, host(cs, pts), n)
    assert got["info"]["n_in"] == n == got["info"]["n_used"]


# ---- device-resident clouds
def scene(c):
    """a 640 x 480 scene, the pixels that become points, and colour / semantic images (palette colours, no moving class)"""
    def make():
        import json
        d = CR.scene_depth(W, H, 21)
        rng = np.random.default_rng(2)
        bgr = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        pal = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "palette.json")))["palette_bgr"], np.uint8)
        sem = pal[np.array([1, 4, 5, 6, 8])[rng.integers(0, 5, (H // 8, W // 8))]].repeat(8, 0).repeat(8, 1)          # (classes the back-projection neither gates nor masks)
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


@pytest.mark.parametrize("sizes", [(300,), (100, 93), (40, 0, 150), (40, 0, 150, 66, 0, 257, 1), (0,), (0, 0, 5), (BLOCK, BLOCK), (BLOCK + 1, 2 * BLOCK - 1, 64)])
@pytest.mark.parametrize("form", FORMS, indirect=True)
def test_device_clouds(g, sizes, form):
    """m device clouds == the host function on the fetched points; the same clouds reversed give everything identical"""
    import semantic_slam_mapping_amd as ssm
    c = g.c
    rng = np.random.default_rng(len(sizes) + sum(sizes))
    clouds, hp, poses = [], [], []
    try:
        for k, n in enumerate(sizes):
            cl, pts = sparse_cloud(c, n, 100 + k)
            clouds.append(cl); hp.append(pts); poses.append(CR.pose(rng, 0.01, 0.05))
        P = dict(WALL, cell=0.25, nx=32, ny=28)
        t = g.target(32, 28)
        got = c.grid_clouds(t, clouds, poses, cells=True, **P)
        ref = ssm.grid_host(hp, poses, cells=True, **P)
        assert_equal(got, ref, sizes)
        assert got["info"]["n_in"] == sum(sizes) and (sum(sizes) < 5 or got["info"]["n_used"] > 0)
        if sum(sizes) >= 300:
            assert (got["n"] > 1).any() and {int(x) for x in np.unique(got["ground_label"])} & {1, 4, 5, 6, 8}
        assert_equal(c.grid_clouds(t, clouds[::-1], poses[::-1], cells=True, **P), ref, (sizes, "reversed"))
    finally:
        for cl in clouds:
            c.cloud_free(cl)


@pytest.mark.parametrize("form", FORMS, indirect=True)
def test_many_points_in_one_cell_and_two_cells_alternating(g, form):
    """the shapes where an aggregated accumulation could go wrong: 4096 points of one cloud in ONE cell, heights and labels varied so LOW and HIGH and every bin
    are hit; and two cells alternating lane by lane"""
    rng = np.random.default_rng(11)
    n = 4096
    gz = np.where(rng.random(n) < 0.5, rng.normal(-1.0, 0.02, n), rng.uniform(-0.5, 2.0, n))
    lab = rng.integers(0, 14, n)
    one = GC.case([GC.gp(rng.uniform(0.01, 0.24, n), rng.uniform(0.26, 0.49, n), gz, lab)], GC.SMALL)
    got = dev(g, one)
    assert_equal(got, host(one), "one cell")
    assert got["n"][5, 4] == n and (got["n"] > 0).sum() == 1 and got["cells"]["n_low"][5, 4] > 1000 and got["cells"]["n_high"][5, 4] > 1000
    assert got["cells"]["sum_low"][5, 4] < 0 and (got["cells"]["hist_low"][5, 4] > 0).all() and (got["cells"]["hist_high"][5, 4] > 0).all()
    gx = np.where(np.arange(n) % 2 == 0, 0.1, 0.6)
    two = GC.case([GC.gp(gx, 0.1, gz, lab)], dict(GC.SMALL, ground_radius=0))
    got = dev(g, two)
    assert_equal(got, host(two), "two cells")
    assert got["n"][4, 4] == got["n"][4, 6] == n // 2 and (got["n"] > 0).sum() == 2
    # runs of 1, 2, 3 ... 64 and more equal cells in a row, across wave and block borders
    runs = np.repeat(np.arange(90) % 8, np.arange(1, 91))
    three = GC.case([GC.gp(-0.9 + 0.25 * runs, 0.1, gz[:len(runs)], lab[:len(runs)]), GC.gp(0.1, 0.1, gz[:77], lab[:77])], GC.SMALL)
    assert_equal(dev(g, three), host(three), "runs")


@pytest.mark.parametrize("form", FORMS, indirect=True)
def test_after_outlier_removal_and_after_carving(g, form):
    """the clouds as ssm_cloud_sor and one ssm_carve leave them (shrunk in place) give the grid of their fetched points, and the grid changes nothing of them"""
    import semantic_slam_mapping_amd as ssm
    c = g.c
    d, nz, bgr, sem = scene(c)
    rng = np.random.default_rng(5)
    clouds, poses = [], []
    try:
        for k in range(2):
            dep = np.zeros_like(d)
            dep[k::4, k::4] = d[k::4, k::4]
            dep.reshape(-1)[rng.choice(nz, 200, replace=False)] = 500          # speckles for the filter
            clouds.append(c.backproject_dev(dep, bgr, sem)); poses.append(CR.pose(rng, 0.004, 0.02))
        Tv = CR.pose(rng, 0.004, 0.02)
        t = g.target(64, 56)
        before = [c.cloud_size(cl) for cl in clouds]
        for cl in clouds:
            c.cloud_sor(cl)
        after_sor = [c.cloud_size(cl) for cl in clouds]
        assert all(a < b for a, b in zip(after_sor, before))
        hp = [c.cloud_fetch(cl).copy() for cl in clouds]
        assert_equal(c.grid_clouds(t, clouds, poses, cells=True, **WALL), ssm.grid_host(hp, poses, cells=True, **WALL), "after sor")
        assert [c.cloud_fetch(cl).tobytes() for cl in clouds] == [p.tobytes() for p in hp]
        far = np.clip(d[::8, ::8].astype(np.int64) + 900 * (np.arange(W // 8) % 16 < 9), 1, 65535).astype(np.uint16)          # stripes pushed back: seen through there
        view = c.carve_view(far, (CAM[0] / 8, CAM[1] / 8, CAM[2] / 8, CAM[3] / 8, CAM[4]))
        try:
            infos = c.carve(view, Tv, clouds, poses, min_votes=2)          # (two votes: the survivors keep non-zero run counters)
            assert all(i["n_kept"] == n for i, n in zip(infos, after_sor)) and all(c.cloud_run(cl).any() for cl in clouds)
            infos = c.carve(view, Tv, clouds, poses, min_votes=2)
        finally:
            c.carve_view_free(view)
        assert all(0 < i["n_kept"] < n for i, n in zip(infos, after_sor))
        hp = [c.cloud_fetch(cl).copy() for cl in clouds]
        runs = [c.cloud_run(cl).copy() for cl in clouds]
        assert [len(p) for p in hp] == [i["n_kept"] for i in infos]
        got = c.grid_clouds(t, clouds, poses, cells=True, **WALL)
        assert_equal(got, ssm.grid_host(hp, poses, cells=True, **WALL), "after carving")
        assert got["info"]["n_in"] == sum(len(p) for p in hp) and got["info"]["n_used"] > 1000
        assert [c.cloud_size(cl) for cl in clouds] == [len(p) for p in hp]
        assert [c.cloud_fetch(cl).tobytes() for cl in clouds] == [p.tobytes() for p in hp]
        assert [c.cloud_run(cl).tobytes() for cl in clouds] == [r.tobytes() for r in runs]
    finally:
        for cl in clouds:
            c.cloud_free(cl)


def test_viewer_map(g):
    import semantic_slam_mapping_amd as ssm
    c = g.c
    rng = np.random.default_rng(8)
    clouds, poses = [], []
    try:
        for k, n in enumerate((3000, 2500)):
            clouds.append(sparse_cloud(c, n, 40 + k)[0]); poses.append(CR.pose(rng, 0.004, 0.02))
        n = c.viewer_map_update(clouds, poses, rebuild=True)
        pts = c.viewer_map_fetch(n)
        assert 0 < len(pts) == n
        got = c.grid_viewer_map(g.target(64, 56), cells=True, **WALL)
        assert_equal(got, ssm.grid_host([pts], [np.eye(4)], cells=True, **WALL), "viewer map")
        assert got["info"]["n_in"] == n and got["info"]["n_used"] > 1000
    finally:
        for cl in clouds:
            c.cloud_free(cl)


def street(k, w=W, h=H):
    """a camera 1.5 m above a ground plane looking along it (y down, z forward): road within 3 m of the axis, pavement beyond, a wall 30 m ahead, a box on the
    road; labelled, as one host cloud in the camera frame"""
    f, cx, cy = 0.8 * w, w / 2 - 0.3, h / 2 + 0.2
    rng = np.random.default_rng(900 + k)
    v, u = np.mgrid[0:h, 0:w]
    with np.errstate(divide="ignore"):
        z = np.where(v > cy, 1.5 * f / np.maximum(v - cy, 1e-9), 1e9)
    wall = z > 30.0
    z = np.where(wall, 30.0, z)
    box = (u > 0.62 * w) & (u < 0.75 * w) & (v > 0.4 * h) & (z > 6.0)
    z = np.where(box, 6.0, z) + rng.normal(0, 0.004, (h, w))
    x = (u - cx) * z / f
    pts = np.zeros(w * h, R.POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = x.ravel(), ((v - cy) * z / f).ravel(), z.ravel()
    pts["label"] = np.where(box, 9, np.where(wall, 1, np.where(np.abs(x) < 3.0, 4, 5))).ravel()
    return pts


def full_size():
    """five 640 x 480 clouds of the street, two metres apart, into the default 512 x 512 cells of 0.2 m"""
    def make():
        rng = np.random.default_rng(640)
        clouds, poses = [], []
        for k in range(5):
            T = CR.pose(rng, 0.005, 0.02)
            T[2, 3] += 2.0 * k
            clouds.append(street(k)); poses.append(T)
        cs = GC.case(clouds, dict(R.DEFAULTS), poses)
        return cs, host(cs)
    return memo("full", make)


@pytest.mark.parametrize("form", FORMS, indirect=True)
def test_full_size(g, form):
    cs, ref = full_size()
    got = dev(g, cs)
    assert_equal(got, ref, "full size")
    I = ref["info"]
    # (a guard of the scene, not of the library: full clouds, most of them used, thousands of cells hit, some of them by hundreds of points)
    assert I["n_in"] == 5 * W * H and I["n_used"] > 0.5 * I["n_in"] and I["out_of_band"] > 0 and ref["n"].max() > 500
    assert min(I["drivable"], I["walkable"], I["obstacle"]) > 100 and I["unobserved"] < 512 * 512 - 5000


def test_small_after_large_and_targets_of_several_sizes():
    """the context's table and staging are reused by a smaller call and grown by a larger one; targets of several sizes live side by side; a second, smaller build
    into a target -- fewer points, fewer cells -- starts from cleared cells (a context of its own: the first call sizes the workspaces)"""
    import semantic_slam_mapping_amd as ssm
    x = Ctx()
    try:
        with pytest.raises(ssm.SsmError) as e:
            x.c.grid_viewer_map(x.target(8, 8), **GC.SMALL)          # no viewer map yet
        assert e.value.code == -1
        with pytest.raises(ssm.SsmError) as e:
            x.c.grid_fetch(x.target(8, 8))                           # nothing built yet
        assert e.value.code == -1
        for name in ("borders", "posed_m3", "nonfinite", "full", "posed_m7", "grid_1x7", "empty_m0", "classes"):
            if name == "full":
                cs, ref = full_size()
            else:
                cs = memo(name, GC.cases()[name]); ref = memo(("host", name), lambda: host(cs))
            assert_equal(dev(x, cs), ref, name)
        # into the 512 x 512 target again: the wall scene, then a few points into a 9 x 5 corner of it -- nothing of the earlier builds may stay
        big = x.target(512, 512)
        cs = wall_points()
        full = dev(x, cs, target=big)
        assert_equal(full, host(cs), "wall into the large target")
        few = [cs["clouds"][0][:40]]
        kw = dict(nx=9, ny=5, x0=-4.0, y0=0.0, cell=1.0)
        got = dev(x, cs, few, target=big, **kw)
        assert_equal(got, host(cs, few, **kw), "second build")
        assert got["cls"].shape == (5, 9) and 0 < got["info"]["n_used"] <= 40 < full["info"]["n_used"]
        with pytest.raises(ssm.SsmError) as e:
            dev(x, cs, few, target=x.target(11, 4), **kw)            # 45 cells, the target has 44
        assert e.value.code == -1
    finally:
        x.close()


def test_refusals_on_the_device(g):
    import semantic_slam_mapping_amd as ssm
    c = g.c
    cs = memo("posed_m3", GC.cases()["posed_m3"])
    nan, inf = float("nan"), float("inf")
    Gn = np.array(R.DEFAULTS["G"], np.float64); Gn[0, 0] = nan
    for kw in (dict(G=Gn), dict(x0=nan), dict(y0=inf), dict(cell=0.0), dict(cell=-1.0), dict(cell=nan), dict(h_min=1.0, h_max=0.0), dict(h_min=-1048577.0), dict(h_max=1048577.0),
               dict(h_max=nan), dict(step=-0.1), dict(step=nan), dict(step=inf), dict(ground_radius=-1), dict(ground_radius=5), dict(min_obstacle_points=0)):
        with pytest.raises(ssm.SsmError) as e:
            dev(g, cs, **kw)
        assert e.value.code == -1, kw
    t = g.target(19, 17)
    for kw in (dict(nx=0), dict(ny=0), dict(nx=-1), dict(nx=20), dict(nx=4097, ny=4096)):
        with pytest.raises(ssm.SsmError) as e:
            dev(g, cs, target=t, **kw)
        assert e.value.code == -1, kw
    bad = np.eye(4)
    bad[0, 0] = nan
    cl, _ = sparse_cloud(c, 10, 1)
    cl2, _ = sparse_cloud(c, 0, 2)
    try:
        for clouds, poses in (([cl], [bad]), ([cl, cl], [R.EYE, R.EYE]), ([cl, cl2, cl], [R.EYE] * 3)):
            with pytest.raises(ssm.SsmError) as e:
                c.grid_clouds(t, clouds, poses, **cs["params"])
            assert e.value.code == -1
        with pytest.raises(ssm.SsmError) as e:
            c.grid_points(t, [cs["clouds"][0], cs["clouds"][0]], [R.EYE, R.EYE], **cs["params"])
        assert e.value.code == -1
        with pytest.raises(ssm.SsmError) as e:
            c.grid_points(t, [cs["clouds"][0]], [bad], **cs["params"])
        assert e.value.code == -1
        assert c.grid_clouds(t, [], [], **cs["params"])["info"]["unobserved"] == 19 * 17
        assert c.grid_clouds(t, [cl2, cl], [R.EYE, R.EYE], **cs["params"])["info"]["n_in"] == 10
        for nx, ny in ((0, 7), (9, 0), (4097, 4096)):
            with pytest.raises(ssm.SsmError) as e:
                c.grid_target(nx, ny)
            assert e.value.code == -1
        for f in (-2, 2):
            with pytest.raises(ssm.SsmError) as e:
                c.grid_form(f)
            assert e.value.code == -1
    finally:
        c.cloud_free(cl); c.cloud_free(cl2)
    assert_equal(dev(g, cs), memo(("host", "posed_m3"), lambda: host(cs)), "the context goes on")
