"""What the entry points that take a list of clouds refuse, and with which words (csrc/ssm_cloud_list.hip): ssm_render_points / _clouds /
_viewer_map, ssm_grid_points / _clouds / _viewer_map, ssm_align_points / _clouds, ssm_carve and ssm_carve_points, called through ctypes on the loaded library,
because the Python API cannot express a negative count or a null array.  Every row is (the call, the status, the message of ssm_last_error); the pairs are
literals recorded from the library as it stood before the entry points shared one skeleton, so the order of refusals -- what a call that is wrong in two ways
reports -- is pinned: the target's or view's refusals first; host arrays: the count before a null or repeated array; handles: the handle, its repetition and its
pose before the count.  Every bad call is refused on the host before any launch.  The shapes are the smallest that reach the code: an 8 x 8 view, a 2 x 2 grid,
clouds of 0 and 3 points."""
import ctypes as C
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAM8 = (4.0, 4.0, 8.0, 8.0, 1000.0)
INVAL = -1
NULL = "null argument"
POSE = "carve: a pose is not finite"
GRID = dict(nx=2, ny=2, x0=-1.0, y0=0.0, cell=1.0)
TWICE = {"render": None, "grid": "grid: the same cloud twice", "align": "align: the same cloud twice", "carve": "carve: the same cloud twice in one call"}
NEGATIVE = {s: s + ": a negative point count" for s in ("render", "grid", "align")}
STAGES = ("render", "grid", "align")


def poses(m, nan_at=None):
    T = np.tile(np.eye(4).reshape(16), (max(m, 1), 1))
    if nan_at is not None:
        T[nan_at, 13] = np.nan
    return np.ascontiguousarray(T)


class Rig:
    """one context, one target or view per stage, the clouds and the host arrays of every row"""
    def __init__(self):
        import semantic_slam_mapping_amd as ssm
        from semantic_slam_mapping_amd import _lib
        from semantic_slam_mapping_amd.api import grid_params, align_params, _render_params
        self.L = _lib
        self.c = ssm.Context(0, width=640, height=480, orb_features=500, max_batch=1, voxel_capacity_log2=12, camera=(318.6, 255.3, 517.3, 516.5, 1000.0))
        self.lib, self.h = self.c.lib, self.c.h
        self.cam = _lib.Camera(*CAM8)
        depth = np.full((8, 8), 1000, np.uint16)
        self.rt = self.c.render_target(8, 8); self.gt = self.c.grid_target(2, 2)
        self.cv = self.c.carve_view(depth, CAM8); self.av = self.c.align_view(depth, CAM8)
        self.gp = grid_params(**GRID); self.ap = align_params(); self.rp = _render_params({})
        self.eye = np.ascontiguousarray(np.eye(4).reshape(16))
        self.nan_view = self.eye.copy(); self.nan_view[12] = np.nan
        self.depth = depth
        self.cl = [self.cloud(k, at) for k, at in ((0, 0), (3, 0), (3, 3), (3, 1), (3, 2))]          # [0]: empty; [3], [4]: carving's own, it writes to its clouds
        self.pts = [np.ascontiguousarray(self.c.cloud_fetch(self.cl[i]).copy()) for i in (1, 2)]
        assert [len(p) for p in self.pts] == [3, 3]

    def cloud(self, k, row):
        """k points of the 8 x 8 view's row `row + 2`, as a device cloud: backproject_dev takes frames of the context's size only (and a context none below 64 x 64),
        so the 8 x 8 frame is the corner of an otherwise empty 640 x 480 one"""
        d = np.zeros((480, 640), np.uint16); d[row + 2, 2:2 + k] = 1000
        img = np.zeros((480, 640, 3), np.uint8); img[..., 1] = 200
        return self.c.backproject_dev(d, img, np.zeros((480, 640, 3), np.uint8), CAM8)

    def close(self):
        self.c.render_target_free(self.rt); self.c.grid_target_free(self.gt); self.c.carve_view_free(self.cv); self.c.align_view_free(self.av)
        for cl in self.cl:
            self.c.cloud_free(cl)
        self.c.close()

    def err(self):
        return (self.lib.ssm_last_error(self.h) or b"").decode()

    @staticmethod
    def ptr(a):
        return None if a is None else a.ctypes.data

    # the three forms of every stage; target / view: the stage's own unless given (None: a null one)
    def points(self, stage, pts, n, T, m, target="own", T_view=None):
        pa = None if pts is None else (C.c_void_p * max(len(pts), 1))(*[None if p is None else p.ctypes.data for p in pts])
        na = None if n is None else np.ascontiguousarray(n, np.int32)
        tv = self.ptr(self.eye if T_view is None else T_view)
        if stage == "render":
            return self.lib.ssm_render_points(self.h, self.rt if target == "own" else target, C.byref(self.cam), tv, pa, self.ptr(na), self.ptr(T), m, C.byref(self.rp),
                                              C.byref(self.L.RenderInfo()))
        if stage == "grid":
            return self.lib.ssm_grid_points(self.h, self.gt if target == "own" else target, pa, self.ptr(na), self.ptr(T), m, C.byref(self.gp), C.byref(self.L.GridInfo()))
        out = np.zeros(16)
        return self.lib.ssm_align_points(self.h, self.av if target == "own" else target, tv, pa, self.ptr(na), self.ptr(T), m, C.byref(self.ap), self.ptr(out),
                                         C.byref(self.L.AlignInfo()))

    def clouds(self, stage, cl, T, m, target="own", T_view=None):
        ca = None if cl is None else (C.c_void_p * max(len(cl), 1))(*cl)
        tv = self.ptr(self.eye if T_view is None else T_view)
        if stage == "render":
            return self.lib.ssm_render_clouds(self.h, self.rt if target == "own" else target, C.byref(self.cam), tv, ca, self.ptr(T), m, C.byref(self.rp), C.byref(self.L.RenderInfo()))
        if stage == "grid":
            return self.lib.ssm_grid_clouds(self.h, self.gt if target == "own" else target, ca, self.ptr(T), m, C.byref(self.gp), C.byref(self.L.GridInfo()))
        if stage == "align":
            out = np.zeros(16)
            return self.lib.ssm_align_clouds(self.h, self.av if target == "own" else target, tv, ca, self.ptr(T), m, C.byref(self.ap), self.ptr(out), C.byref(self.L.AlignInfo()))
        infos = (self.L.CarveInfo * max(m, 1))()
        return self.lib.ssm_carve(self.h, self.cv if target == "own" else target, tv, ca, self.ptr(T), m, None, infos)

    def viewer_map(self, stage):
        if stage == "render":
            return self.lib.ssm_render_viewer_map(self.h, self.rt, C.byref(self.cam), self.ptr(self.eye), C.byref(self.rp), C.byref(self.L.RenderInfo()))
        return self.lib.ssm_grid_viewer_map(self.h, self.gt, C.byref(self.gp), C.byref(self.L.GridInfo()))

    def carve_points(self, pts, n, T_cloud, T_view=None, depth="own"):
        out = np.zeros(4, self.pts[0].dtype); n_out = C.c_int(-7)
        d = self.depth if depth == "own" else depth
        return self.lib.ssm_carve_points(self.h, self.ptr(d), 8, 8, C.byref(self.cam), self.ptr(self.eye if T_view is None else T_view), self.ptr(pts), n, self.ptr(T_cloud), None,
                                         None, self.ptr(out), len(out), C.byref(n_out), C.byref(self.L.CarveInfo()))


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


def refused(rig, rc, msg):
    assert (rc, rig.err()) == (INVAL, msg)


def points_rows(stage):
    """(name, pts, n, poses, m, keywords) -> (status, message); p, q: the two host arrays"""
    twice = TWICE[stage]
    return [
        ("m = -1", ["p"], [3], poses(1), -1, {}, NULL),
        ("null pts", None, [3], poses(1), 1, {}, NULL),
        ("null n", ["p"], None, poses(1), 1, {}, NULL),
        ("null T_clouds", ["p"], [3], None, 1, {}, NULL),
        ("a negative count wins over the null array", [None], [-1], poses(1), 1, {}, NEGATIVE[stage]),
        ("a negative count in second place", ["p", None], [3, -5], poses(2), 2, {}, NEGATIVE[stage]),
        ("a null array with a count", [None], [2], poses(1), 1, {}, NULL),
        ("a null array without a count is no array", [None], [0], poses(1), 1, {}, None),
        ("the same array twice", ["p", "p"], [3, 3], poses(2), 2, {}, twice),
        ("the same array twice, one of them unused", ["p", "p"], [3, 0], poses(2), 2, {}, None),
        ("a NaN in the second pose", ["p", "q"], [3, 3], poses(2, 1), 2, {}, POSE),
        ("the null array of the first cloud before the pose of the second", [None, "q"], [2, 3], poses(2, 1), 2, {}, NULL),
        ("a null target or view wins over the list", [None], [-1], poses(1), 1, {"target": None}, NULL),
        ("no cloud", ["p"], [0], poses(1), 0, {}, None),
        ("no cloud and null lists", None, None, None, 0, {}, None),
        ("one cloud of 3 points", ["p"], [3], poses(1), 1, {}, None),
    ] + ([("a NaN in T_view wins over the list", [None], [-1], poses(1), 1, {"T_view": "nan"}, POSE)] if stage != "grid" else [])


@pytest.mark.parametrize("stage", STAGES)
def test_points_forms(rig, stage):
    arrays = {"p": rig.pts[0], "q": rig.pts[1], None: None}
    for name, pts, n, T, m, kw, msg in points_rows(stage):
        kw = dict(kw)
        if kw.get("T_view") == "nan":
            kw["T_view"] = rig.nan_view
        rc = rig.points(stage, None if pts is None else [arrays[p] for p in pts], n, T, m, **kw)
        print(stage, name, rc, rig.err() if rc else "")
        assert (rc, rig.err() if rc else None) == ((INVAL, msg) if msg else (0, None)), name


def clouds_rows(stage):
    twice = TWICE[stage]
    a, b = (3, 4) if stage == "carve" else (1, 2)          # indices into Rig.cl
    return [
        ("m = -1", [a], poses(1), -1, {}, NULL),
        ("null clouds", None, poses(1), 1, {}, NULL),
        ("null T_clouds", [a], None, 1, {}, NULL),
        ("a null handle in second place", [a, None], poses(2), 2, {}, NULL),
        ("the same handle twice", [a, a], poses(2), 2, {}, twice),
        ("a NaN in the second pose", [a, b], poses(2, 1), 2, {}, POSE),
        ("the repeated handle before its pose", [a, a], poses(2, 1), 2, {}, twice or POSE),
        ("the pose of the first before the null handle of the second", [a, None], poses(2, 0), 2, {}, POSE),
        ("a null target or view wins over the list", [a, b], poses(2, 1), 2, {"target": None}, NULL),
        ("a NaN in T_view wins over the list", [a, None], poses(2), 2, {"T_view": "nan"}, NULL if stage == "grid" else POSE),
        ("no cloud", [a], poses(1), 0, {}, None),
        ("no cloud and null lists", None, None, 0, {}, None),
        ("an empty cloud", [0], poses(1), 1, {}, None),
        ("one cloud of 3 points", [a], poses(1), 1, {}, None),
        ("two clouds, one of them empty", [0, b], poses(2), 2, {}, None),
    ]


@pytest.mark.parametrize("stage", STAGES + ("carve",))
def test_clouds_forms(rig, stage):
    for name, cl, T, m, kw, msg in clouds_rows(stage):
        kw = dict(kw)
        if kw.get("T_view") == "nan":
            kw["T_view"] = rig.nan_view
        rc = rig.clouds(stage, None if cl is None else [None if i is None else rig.cl[i] for i in cl], T, m, **kw)
        print(stage, name, rc, rig.err() if rc else "")
        assert (rc, rig.err() if rc else None) == ((INVAL, msg) if msg else (0, None)), name
    if stage == "carve":          # the call that was accepted left the constant view's verdicts in its clouds, the refused ones nothing
        assert [rig.c.cloud_size(rig.cl[i]) for i in (0, 3, 4)] == [0, 3, 3]


def test_carve_points(rig):
    p = rig.pts[0]
    rows = [
        ("a negative count", None, -1, rig.eye, {}, NULL),
        ("a null array with a count", None, 2, rig.eye, {}, NULL),
        ("a null depth image", p, 3, rig.eye, {"depth": None}, NULL),
        ("a null pose of the cloud", p, 3, None, {}, NULL),
        ("a NaN in the cloud's pose", p, 3, rig.nan_view, {}, POSE),
        ("a NaN in T_view", p, 3, rig.eye, {"T_view": rig.nan_view}, POSE),
        ("no point", None, 0, rig.eye, {}, None),
        ("3 points", p, 3, rig.eye, {}, None),
    ]
    for name, pts, n, T, kw, msg in rows:
        rc = rig.carve_points(pts, n, T, **kw)
        print("carve_points", name, rc, rig.err() if rc else "")
        assert (rc, rig.err() if rc else None) == ((INVAL, msg) if msg else (0, None)), name


def test_viewer_map(rig):
    """without a map: each stage's message.  With the map of one cloud: the call equals the same map's points, fetched and given back as one cloud at the identity pose,
    byte for byte (the map has no handle of its own that a _clouds call could take)"""
    c = rig.c
    c._chk(rig.lib.ssm_viewer_map_release(rig.h, 0))
    for stage in ("render", "grid"):
        refused(rig, rig.viewer_map(stage), stage + ": the context holds no viewer map")
    eye = np.eye(4)
    n = c.viewer_map_update([rig.cl[1]], [eye], rebuild=True)
    assert n > 0
    pts = c.viewer_map_fetch(n).copy()
    for stage in ("render", "grid"):
        assert rig.viewer_map(stage) == 0
    a = c.render_viewer_map(rig.rt, CAM8, eye, keys=True); b = c.render_points(rig.rt, CAM8, eye, [pts], [eye], keys=True)
    assert a["info"] == b["info"] and a["info"]["n_covered"] > 0
    assert all(a[k].tobytes() == b[k].tobytes() for k in ("depth", "bgr", "label", "index", "keys"))
    a = c.grid_viewer_map(rig.gt, cells=True, **GRID); b = c.grid_points(rig.gt, [pts], [eye], cells=True, **GRID)
    assert a["info"] == b["info"] and a["info"]["n_used"] == n
    assert all(a[k].tobytes() == b[k].tobytes() for k in ("cells", "cls", "ground_label", "obstacle_label", "ground_q", "top_q", "n", "n_high"))
    c._chk(rig.lib.ssm_viewer_map_release(rig.h, 0))
