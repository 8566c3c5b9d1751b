"""Object extraction on a real MI355X (csrc/kernels_objects.hip behind ssm_objects_grid / _clouds / _points / _viewer_map / _fetch): device == the host functions
byte for byte (tests/test_objects.py ties those to the numpy restatement).  Stage 1 through ssm_debug_objects_cells against ssm_objects_cells_host on the patterns
of tests/objects_cases.py at the grid sizes around the labelling's tile, under both connectivities.  Stage 2 under both accumulate forms against ssm_objects_host:
records, object_id, per-point ids and info -- at the point counts around a wave and a block, on 1, 2, 3 and 7 device clouds (sizes 0, boundaries inside a wave and
a block, reversed), with thousands of points of one object, two objects alternating lane by lane, runs of 1 .. 90, after ssm_cloud_sor and ssm_carve, on the
viewer's map, at full size, and every refusal."""
import os
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import objects_ref as R  # noqa: E402
import objects_cases as OC  # noqa: E402
import grid_cases as GC  # noqa: E402
import grid_ref as GR  # noqa: E402
import carve_ref as CR  # noqa: E402
import test_gpu_grid as TG  # noqa: E402          (its scenes: the wall, the street, the sparse device clouds)
from conftest import CAM  # noqa: E402

pytestmark = pytest.mark.gpu
W, H = 640, 480
BLOCK = 256          # csrc/kernels_objects.hip OBJ_T
ARR = ("cls", "obstacle_label", "ground_q", "top_q", "n_high")
FORMS = [0, 1]       # one atomic per point and figure; one per run of adjacent lanes with the same object
_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


class Ctx:
    """a context, its grid targets and its object targets, one per size"""
    def __init__(self):
        import semantic_slam_mapping_amd as ssm
        self.c = ssm.Context(0, width=W, height=H, orb_features=500, max_batch=1, voxel_capacity_log2=12, camera=CAM)
        self.grids, self.objs = {}, {}

    def grid(self, nx, ny):
        if (nx, ny) not in self.grids:
            self.grids[(nx, ny)] = self.c.grid_target(nx, ny)
        return self.grids[(nx, ny)]

    def obj(self, nx, ny):
        if (nx, ny) not in self.objs:
            self.objs[(nx, ny)] = self.c.objects_target(nx, ny)
        return self.objs[(nx, ny)]

    def close(self):
        for t in self.objs.values():
            self.c.objects_target_free(t)
        for t in self.grids.values():
            self.c.grid_target_free(t)
        self.c.close()


@pytest.fixture(scope="module")
def g():
    x = Ctx()
    yield x
    x.close()


@pytest.fixture
def form(request, g):
    g.c.objects_form(request.param)
    yield request.param
    g.c.objects_form(-1)


def equal_records(got, ref, what):
    assert got.dtype == ref.dtype == R.OBJECT_DTYPE and got.shape == ref.shape, (what, got.shape, ref.shape)
    for f in R.OBJECT_DTYPE.names:
        assert np.array_equal(got[f], ref[f]), (what, f, got[f][:8], ref[f][:8])
    assert got.tobytes() == ref.tobytes(), what


# ---------------------------------------------------------------- stage 1
def tile():
    import semantic_slam_mapping_amd as ssm
    lib = ssm.load()
    return lib.ssm_debug_objects_tile_w(), lib.ssm_debug_objects_tile_h()


def cells_equal(g, cs, target, what):
    import semantic_slam_mapping_amd as ssm
    a = [cs[k] for k in ARR]
    rec, oid, info = ssm.objects_cells_host(*a, **cs["params"])
    ginfo = g.c.objects_cells(target, *a, **cs["params"])
    got, goid = g.c.objects_fetch(target)
    assert ginfo == info, (what, ginfo, info)
    equal_records(got, rec, what)
    assert goid.dtype == np.int32 and goid.shape == oid.shape and np.array_equal(goid, oid), (what, np.argwhere(goid != oid)[:5])
    return info


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("pattern", list(OC.patterns()))
def test_labelling_on_the_patterns(g, pattern, conn):
    tw, th = tile()
    target = g.obj(2 * tw + 2, 2 * th + 3)          # one target for every shape: each is a smaller grid than the one before or after it
    for nx, ny in OC.shapes(tw, th):
        cs = OC.cell_case(OC.patterns()[pattern](nx, ny, tw, th), dict(OC.LOOSE, connectivity=conn))
        info = cells_equal(g, cs, target, (pattern, conn, nx, ny))
        assert info["member_cells"] == int((cs["obstacle_label"] != 255).sum())
        if pattern in ("serpentine", "spiral", "u_shape") or (pattern == "checkerboard" and conn == 8 and min(nx, ny) > 1):
            assert info["components"] == 1, (pattern, nx, ny)
        if pattern == "checkerboard" and conn == 4:
            assert info["components"] == info["member_cells"]


@pytest.mark.parametrize("name", list(OC.cell_cases()))
def test_labelling_on_the_cases(g, name):
    cs = OC.cell_cases()[name]()
    ny, nx = cs["cls"].shape
    for conn in (4, 8):
        cells_equal(g, dict(cs, params=dict(cs["params"], connectivity=conn)), g.obj(nx, ny), (name, conn))
    if name == "rejections":
        info = cells_equal(g, cs, g.obj(nx, ny), name)
        assert (info["kept"], info["rejected_cells"], info["rejected_points"], info["rejected_height"]) == (2, 2, 2, 1)


def test_small_grid_after_a_large_one(g):
    """a second, smaller labelling into one target -- fewer cells, fewer components -- leaves nothing of the first; and a large one again"""
    tw, th = tile()
    target = g.obj(4 * tw + 1, 3 * th + 1)
    big = OC.cell_case(OC.random_fill(0.5, 9)(4 * tw + 1, 3 * th + 1, tw, th), dict(OC.LOOSE, connectivity=4))
    small = OC.cell_case(OC.random_fill(0.5, 8)(7, 5, tw, th))
    n_big = cells_equal(g, big, target, "large")["components"]
    n_small = cells_equal(g, small, target, "small")["components"]
    assert n_big > 10 * n_small > 0
    cells_equal(g, OC.cell_case(OC.empty(3, 3, tw, th)), target, "empty")
    cells_equal(g, big, target, "large again")


# ---------------------------------------------------------------- stage 2
LOOSE_GRID = dict(OC.GRID, min_obstacle_points=2)


def chain_points(g, clouds, T, grid, params, what):
    """the device chain on host arrays == ssm_objects_host: the grid, stage 1, stage 2 -> the host's records"""
    import semantic_slam_mapping_amd as ssm
    c = g.c
    gt, ot = g.grid(grid["nx"], grid["ny"]), g.obj(grid["nx"], grid["ny"])
    rec, oid, ids, info = ssm.objects_host(clouds, T, grid=grid, **params)
    c.grid_points(gt, clouds, T, **grid)
    info1 = c.objects_grid(gt, ot, **params)
    assert {k: v for k, v in info1.items() if k not in ("n_in", "object_points")} == {k: v for k, v in info.items() if k not in ("n_in", "object_points")}, (what, info1, info)
    first, _ = c.objects_fetch(ot)
    assert (first["n_points"] == 0).all() and (first["x_min_q"] == GR.I32_MAX).all() and (first["z_max_q"] == GR.I32_MIN).all() and (first["sum_y"] == 0).all()
    gids, ginfo = c.objects_points(gt, ot, clouds, T)
    got, goid = c.objects_fetch(ot)
    assert ginfo == info, (what, ginfo, info)
    equal_records(got, rec, what)
    assert np.array_equal(goid, oid) and gids.dtype == np.int32 and np.array_equal(gids, ids), (what, np.flatnonzero(gids != ids)[:5])
    assert np.array_equal(c.objects_point_ids(len(ids)), ids), what
    assert np.array_equal(got["n_points"], got["cell_points"].astype(np.uint32)), what          # the invariant
    return rec, info


@pytest.mark.parametrize("form", FORMS, indirect=True)
@pytest.mark.parametrize("name", list(OC.cloud_cases()))
def test_device_equals_host(g, name, form):
    cs = memo(name, OC.cloud_cases()[name])
    chain_points(g, cs["clouds"], cs["T_clouds"], cs["grid"], cs["params"], name)


@pytest.mark.parametrize("form", FORMS, indirect=True)
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1])
def test_sizes_around_a_wave_and_a_block(g, n, form):
    cs = memo("street_m1", OC.cloud_cases()["street_m1"])
    pts = [cs["clouds"][0][:n]]          # (the cloud is shuffled: ground and boxes from the first points on)
    rec, info = chain_points(g, pts, [GC.EYE], LOOSE_GRID, OC.LOOSE, n)
    assert info["n_in"] == n and (n < 63 or info["object_points"] > 0)


@pytest.mark.parametrize("form", FORMS, indirect=True)
def test_one_object_two_objects_alternating_and_runs(g, form):
    """the shapes where an aggregated accumulation could go wrong: 4096 points of ONE object in a row; two objects alternating lane by lane; runs of 1, 2, ... 90
    points of one object, across wave and block borders, with points of no object between them"""
    rng = np.random.default_rng(21)
    ground = GC.gp(rng.uniform(-3.0, 3.0, 6000), rng.uniform(0.0, 5.0, 6000), rng.normal(-1.5, 0.005, 6000), 4)
    n = 4096
    lab = np.where(rng.random(n) < 0.2, rng.integers(0, 14, n), 9)
    one = GC.gp(rng.uniform(-1.99, -1.01, n), rng.uniform(1.01, 1.99, n), rng.uniform(-1.2, 0.5, n), lab)
    rec, info = chain_points(g, [ground, one], [GC.EYE] * 2, OC.GRID, dict(labels=[9]), "one object")
    assert len(rec) == 1 and rec[0]["n_points"] == n and 0 < rec[0]["n_label"] < n and rec[0]["sum_x"] < 0 < rec[0]["sum_y"]
    gx = np.where(np.arange(n) % 2 == 0, rng.uniform(-1.99, -1.51, n), rng.uniform(1.01, 1.49, n))
    two = GC.gp(gx, rng.uniform(1.01, 1.49, n), rng.uniform(-1.2, 0.5, n), np.where(np.arange(n) % 2 == 0, 9, 10))
    rec, info = chain_points(g, [two, ground], [GC.EYE] * 2, OC.GRID, {}, "two objects")
    assert rec["n_points"].tolist() == [n // 2, n // 2] and rec["label"].tolist() == [9, 10] and rec["n_label"].tolist() == [n // 2, n // 2]
    which = np.repeat(np.arange(90) % 3, np.arange(1, 91))          # object A, object B, no object (a ground point) in runs of 1 .. 90
    m = len(which)
    gx = np.where(which == 0, rng.uniform(-1.99, -1.51, m), np.where(which == 1, rng.uniform(1.01, 1.49, m), rng.uniform(-0.5, 0.5, m)))
    gz = np.where(which == 2, -1.5, rng.uniform(-1.2, 0.5, m))
    runs = GC.gp(gx, rng.uniform(1.01, 1.49, m), gz, np.where(which == 0, 9, np.where(which == 1, 11, 4)))
    rec, info = chain_points(g, [ground[:77], runs, ground[77:]], [GC.EYE] * 3, OC.GRID, {}, "runs")
    assert rec["label"].tolist() == [9, 11] and rec["n_points"].tolist() == [int((which == 0).sum()), int((which == 1).sum())]


# ---- device-resident clouds: the grid tests' wall scene, whose labels are Building, Road, Pavement, Tree and Fence -- the objects are of the standing three
WALL_OBJECTS = dict(labels=[1, 6, 8], min_cells=1, min_points=5, min_height=0.1)


def chain_clouds(g, clouds, poses, hp, grid, params, what):
    """the device chain on device clouds == ssm_objects_host on their fetched points"""
    import semantic_slam_mapping_amd as ssm
    c = g.c
    gt, ot = g.grid(grid["nx"], grid["ny"]), g.obj(grid["nx"], grid["ny"])
    rec, oid, ids, info = ssm.objects_host(hp, poses, grid=grid, **params)
    c.grid_clouds(gt, clouds, poses, **grid)
    c.objects_grid(gt, ot, **params)
    ginfo = c.objects_clouds(gt, ot, clouds, poses)
    got, goid = c.objects_fetch(ot)
    assert ginfo == info, (what, ginfo, info)
    equal_records(got, rec, what)
    assert np.array_equal(goid, oid) and np.array_equal(c.objects_point_ids(len(ids)), ids), what
    return rec, ids, info


@pytest.mark.parametrize("sizes", [(3000,), (1000, 930), (400, 0, 1500), (400, 0, 1500, 660, 0, 257, 1), (0,), (0, 0, 5), (BLOCK, BLOCK), (BLOCK + 1, 2 * BLOCK - 1, 64)])
@pytest.mark.parametrize("form", FORMS, indirect=True)
def test_device_clouds(g, sizes, form):
    """m device clouds == the host function on the fetched points; the same clouds reversed give identical records, and the ids follow their clouds"""
    c = g.c
    rng = np.random.default_rng(len(sizes) + sum(sizes))
    clouds, hp, poses = [], [], []
    try:
        for k, n in enumerate(sizes):
            cl, pts = TG.sparse_cloud(c, n, 100 + k)
            clouds.append(cl); hp.append(pts); poses.append(CR.pose(rng, 0.01, 0.05))
        P = dict(TG.WALL, cell=0.25, nx=32, ny=28)
        rec, ids, info = chain_clouds(g, clouds, poses, hp, P, WALL_OBJECTS, sizes)
        assert info["n_in"] == sum(sizes) and (sum(sizes) < 1900 or (len(rec) > 0 and info["object_points"] > 50))
        rec2, ids2, info2 = chain_clouds(g, clouds[::-1], poses[::-1], hp[::-1], P, WALL_OBJECTS, (sizes, "reversed"))
        equal_records(rec2, rec, (sizes, "reversed against forward"))
        assert info2 == info
        off = np.cumsum([0] + list(sizes))
        assert np.array_equal(ids2, np.concatenate([ids[off[k]:off[k + 1]] for k in range(len(sizes))][::-1]))
    finally:
        for cl in clouds:
            c.cloud_free(cl)


@pytest.mark.parametrize("form", FORMS, indirect=True)
def test_after_outlier_removal_and_after_carving(g, form):
    """the clouds as ssm_cloud_sor and one ssm_carve leave them (shrunk in place) give the objects of their fetched points, and nothing of them changes"""
    c = g.c
    d, nz, bgr, sem = TG.scene(c)
    rng = np.random.default_rng(5)
    clouds, poses = [], []
    try:
        for k in range(2):
            dep = np.zeros_like(d)
            dep[k::4, k::4] = d[k::4, k::4]
            dep.reshape(-1)[rng.choice(nz, 200, replace=False)] = 500          # speckles for the filter
            clouds.append(c.backproject_dev(dep, bgr, sem)); poses.append(CR.pose(rng, 0.004, 0.02))
        Tv = CR.pose(rng, 0.004, 0.02)
        for cl in clouds:
            c.cloud_sor(cl)
        hp = [c.cloud_fetch(cl).copy() for cl in clouds]
        rec, ids, info = chain_clouds(g, clouds, poses, hp, TG.WALL, WALL_OBJECTS, "after sor")
        assert len(rec) > 0 and info["object_points"] > 1000
        assert [c.cloud_fetch(cl).tobytes() for cl in clouds] == [p.tobytes() for p in hp]
        far = np.clip(d[::8, ::8].astype(np.int64) + 900 * (np.arange(W // 8) % 16 < 9), 1, 65535).astype(np.uint16)          # stripes pushed back: seen through there
        view = c.carve_view(far, (CAM[0] / 8, CAM[1] / 8, CAM[2] / 8, CAM[3] / 8, CAM[4]))
        try:
            c.carve(view, Tv, clouds, poses, min_votes=2)
            infos = c.carve(view, Tv, clouds, poses, min_votes=2)
        finally:
            c.carve_view_free(view)
        assert all(0 < i["n_kept"] < len(p) for i, p in zip(infos, hp))
        hp = [c.cloud_fetch(cl).copy() for cl in clouds]
        runs = [c.cloud_run(cl).copy() for cl in clouds]
        rec, ids, info = chain_clouds(g, clouds, poses, hp, TG.WALL, WALL_OBJECTS, "after carving")
        assert len(rec) > 0 and info["n_in"] == sum(len(p) for p in hp)
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
            clouds.append(TG.sparse_cloud(c, n, 40 + k)[0]); poses.append(CR.pose(rng, 0.004, 0.02))
        n = c.viewer_map_update(clouds, poses, rebuild=True)
        pts = c.viewer_map_fetch(n)
        gt, ot = g.grid(64, 56), g.obj(64, 56)
        rec, oid, ids, info = ssm.objects_host([pts], [np.eye(4)], grid=TG.WALL, **WALL_OBJECTS)
        c.grid_viewer_map(gt, **TG.WALL)
        c.objects_grid(gt, ot, **WALL_OBJECTS)
        ginfo = c.objects_viewer_map(gt, ot)
        got, goid = c.objects_fetch(ot)
        assert ginfo == info and info["n_in"] == n and info["object_points"] > 100
        equal_records(got, rec, "viewer map")
        assert np.array_equal(goid, oid) and np.array_equal(c.objects_point_ids(n), ids)
    finally:
        for cl in clouds:
            c.cloud_free(cl)


def full_size(w, h):
    """five w x h clouds of the grid tests' street (a box labelled Vehicle on the road), two metres apart, into the default 512 x 512 cells of 0.2 m"""
    def make():
        import semantic_slam_mapping_amd as ssm
        rng = np.random.default_rng(w)
        clouds, poses = [], []
        for k in range(5):
            T = CR.pose(rng, 0.005, 0.02)
            T[2, 3] += 2.0 * k
            clouds.append(TG.street(k, w, h)); poses.append(T)
        return clouds, poses, ssm.objects_host(clouds, poses, grid=dict(GR.DEFAULTS))
    return memo(("full", w, h), make)


@pytest.mark.parametrize("form", FORMS, indirect=True)
@pytest.mark.parametrize("size", [(640, 480), (1241, 376)])
def test_full_size(g, size, form):
    clouds, poses, ref = full_size(*size)
    rec, info = chain_points(g, clouds, poses, dict(GR.DEFAULTS), {}, size)
    # (a guard of the scene, not of the library: full clouds, the box found as a Vehicle with thousands of points)
    assert info["n_in"] == 5 * size[0] * size[1] and info["kept"] >= 1 and (rec["label"] == 9).all() and rec["n_points"].max() > 5000


def test_refusals_on_the_device(g):
    import semantic_slam_mapping_amd as ssm
    c = g.c
    cs = memo("street_m3", OC.cloud_cases()["street_m3"])
    G = cs["grid"]
    gt, ot = g.grid(G["nx"], G["ny"]), g.obj(G["nx"], G["ny"])

    def refused(call, word=None):
        with pytest.raises(ssm.SsmError) as e:
            call()
        assert e.value.code == -1 and (word is None or word in str(e.value)), (str(e.value), word)

    fresh_g, fresh_o = c.grid_target(8, 8), c.objects_target(8, 8)
    other = Ctx()          # a second context on the same GPU
    cl, _ = TG.sparse_cloud(c, 10, 1)
    try:
        refused(lambda: c.objects_grid(fresh_g, fresh_o), "nothing has been built")
        refused(lambda: c.objects_fetch(fresh_o), "no cells")
        c.grid_points(gt, cs["clouds"], cs["T_clouds"], **G)
        refused(lambda: c.objects_points(gt, fresh_o, cs["clouds"], cs["T_clouds"]), "ssm_objects_grid comes first")
        nan, inf = float("nan"), float("inf")
        for kw in (dict(connectivity=6), dict(connectivity=0), dict(min_cells=-1), dict(min_points=-1), dict(min_height=-0.1), dict(min_height=nan), dict(min_height=inf)):
            refused(lambda: c.objects_grid(gt, ot, **kw), "objects:")
        refused(lambda: c.objects_grid(gt, None), "null")
        refused(lambda: c.objects_grid(None, ot), "null")
        refused(lambda: c.objects_grid(gt, fresh_o), "more cells")
        refused(lambda: c.objects_grid(gt, other.obj(G["nx"], G["ny"])), "another context")
        refused(lambda: c.objects_grid(other.grid(G["nx"], G["ny"]), ot), "another context")
        assert other.c.lib.ssm_objects_fetch(other.c.h, ot, None, 0, None, None) == -1 and "another context" in other.c.lib.ssm_last_error(other.c.h).decode()
        far = dict(G, x0=1048576.0 - 3.0)
        c.grid_points(gt, cs["clouds"], cs["T_clouds"], **far)
        refused(lambda: c.objects_grid(gt, ot), "2^20")
        # stage 2: before stage 1 on this build, after a rebuild, with other clouds, the same cloud twice, a bad pose, the cells of hand-made arrays
        c.grid_points(gt, cs["clouds"], cs["T_clouds"], **G)
        c.objects_grid(gt, ot, **cs["params"])
        c.objects_points(gt, ot, cs["clouds"], cs["T_clouds"])
        refused(lambda: c.objects_points(gt, ot, cs["clouds"][:2], cs["T_clouds"][:2]), "the grid was built from")
        refused(lambda: c.objects_clouds(gt, ot, [cl, cl], [GC.EYE] * 2), "twice")
        refused(lambda: c.objects_clouds(gt, ot, [cl], [GC.EYE]), "the grid was built from")
        bad = np.eye(4); bad[0, 0] = nan
        refused(lambda: c.objects_points(gt, ot, cs["clouds"], [bad] + list(cs["T_clouds"][1:])))
        refused(lambda: c.objects_viewer_map(gt, ot))
        refused(lambda: other.c.objects_points(gt, ot, cs["clouds"], cs["T_clouds"]), "another context")
        # the same host array twice: the counts are checked first, so the grid is one of a cloud and its copy -- the list of the cloud twice has that grid's count
        one = cs["clouds"][0]
        c.grid_points(gt, [one, one.copy()], [GC.EYE] * 2, **G)
        c.objects_grid(gt, ot, **cs["params"])
        refused(lambda: c.objects_points(gt, ot, [one, one], [GC.EYE] * 2), "twice")
        c.grid_points(gt, cs["clouds"], cs["T_clouds"], **G)
        refused(lambda: c.objects_points(gt, ot, cs["clouds"], cs["T_clouds"]), "built again")
        other_g = c.grid_target(G["nx"], G["ny"])
        try:
            c.grid_points(other_g, cs["clouds"], cs["T_clouds"], **G)
            c.objects_grid(gt, ot, **cs["params"])
            refused(lambda: c.objects_points(other_g, ot, cs["clouds"], cs["T_clouds"]), "ssm_objects_grid comes first")
        finally:
            c.grid_target_free(other_g)
        small = OC.ids_ascend()
        c.objects_cells(ot, *[small[k] for k in ARR], **small["params"])
        refused(lambda: c.objects_points(gt, ot, cs["clouds"], cs["T_clouds"]), "ssm_objects_grid comes first")
        refused(lambda: c.objects_cells(fresh_o, *[np.zeros((9, 8), t) for t in (np.uint8, np.uint8, np.int32, np.int32, np.uint32)]), "at most the target's")
        # the bound on a call's points (objects_cloud_rule: checked from the counts, before an array is touched), a negative count and null lists, through the raw ABI
        import ctypes as C
        lib, one = c.lib, cs["clouds"][0]
        T2 = np.ascontiguousarray(np.tile(np.eye(4).reshape(16), 2))
        two = (C.c_void_p * 2)(one.ctypes.data, one[1:].ctypes.data)
        arr = (C.c_void_p * 2)(cl, cl)

        def raw_points(pts, cnt, T, m):
            cnt = None if cnt is None else np.ascontiguousarray(cnt, np.int32)
            rc = lib.ssm_objects_points(c.h, gt, ot, pts, None if cnt is None else cnt.ctypes.data, None if T is None else T.ctypes.data, m, None, None)
            return rc, lib.ssm_last_error(c.h).decode()

        c.grid_points(gt, cs["clouds"], cs["T_clouds"], **G)
        c.objects_grid(gt, ot, **cs["params"])
        rc, msg = raw_points(two, [2 ** 31 - 1, 1], T2, 2)          # 2^31 exactly
        assert rc == -1 and msg == "objects: 2^31 points or more in one call", msg
        rc, msg = raw_points(two, [2 ** 31 - 2, 1], T2, 2)          # one fewer passes the bound and is refused for what it is: not the grid's clouds
        assert rc == -1 and "the grid was built from" in msg, msg
        rc, msg = raw_points(two, [1, -1], T2, 2)
        assert rc == -1 and msg == "objects: a negative point count", msg
        for pts, cnt, T, m in ((None, [1, 1], T2, 2), (two, None, T2, 2), (two, [1, 1], None, 2), (two, [1, 1], T2, -1)):
            rc, msg = raw_points(pts, cnt, T, m)
            assert rc == -1 and msg == "null argument", msg
        for a, T, m in ((None, T2, 2), (arr, None, 2), (arr, T2, -1)):
            assert lib.ssm_objects_clouds(c.h, gt, ot, a, None if T is None else T.ctypes.data, m, None) == -1 and lib.ssm_last_error(c.h).decode() == "null argument"
        assert lib.ssm_objects_clouds(c.h, gt, ot, (C.c_void_p * 2)(cl, None), T2.ctypes.data, 2, None) == -1 and lib.ssm_last_error(c.h).decode() == "null argument"
        assert lib.ssm_objects_viewer_map(c.h, gt, None, None) == -1 and lib.ssm_objects_viewer_map(c.h, None, ot, None) == -1
        assert lib.ssm_objects_points(c.h, None, ot, two, np.ones(2, np.int32).ctypes.data, T2.ctypes.data, 2, None, None) == -1
        # hand-made cells whose n_high sum to 2^31: no built grid holds that many points, and the device adds a tile's in 32 bits
        big = OC.ids_ascend()
        big["n_high"][:] = 0; big["n_high"][0, 0] = 2 ** 31 - 1
        c.objects_cells(ot, *[big[k] for k in ARR], **big["params"])          # 2^31 - 1 is legal
        big["n_high"][0, 1] = 1
        refused(lambda: c.objects_cells(ot, *[big[k] for k in ARR], **big["params"]), "fewer than 2^31")
        for f in (-2, 2):
            refused(lambda: c.objects_form(f), "form")
        for nx, ny in ((0, 7), (9, 0), (4097, 4096)):
            refused(lambda: c.objects_target(nx, ny), "2^24")
        refused(lambda: c.objects_point_ids(3), "the last call assigned")
        with pytest.raises(ssm.SsmError) as e:          # the capacity rule of the fetch
            c.objects_fetch(ot, cap=4)
        assert e.value.code == -4 and "need 5" in str(e.value)
        assert len(c.objects_fetch(ot, cap=5)[0]) == 5
    finally:
        c.cloud_free(cl); c.grid_target_free(fresh_g); c.objects_target_free(fresh_o); other.close()
    chain_points(g, cs["clouds"], cs["T_clouds"], G, cs["params"], "the context goes on")
