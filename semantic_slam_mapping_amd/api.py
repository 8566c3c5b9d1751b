"""Python mirror of the reference's operator interface over the C ABI.

Names follow the reference: ``detect_features`` = OrbFeature::detectFeatures (include/orb.h:32-53), ``match`` =
OrbFeature::match (src/orb.cpp:16-29), ``moving_mask`` = Mapper::semantic_motion_fuse (src/mapper.cpp:189-216),
``generate_point_cloud`` = Mapper::generatePointCloud (src/mapper.cpp:12-94), ``voxel_filter`` = pcl::VoxelGrid as
used in Mapper::viewer (src/mapper.cpp:154-155).
"""
import ctypes as C
import numpy as np
from . import _lib
from ._lib import Camera, Config, FramesDev, SeqOutDev, SgbmParams, VoParams, StereoFramesDev, StereoOutDev, TrackerParams, UvdParams, UvdInfo, VocabTrainParams, VocabTrainReport, MotionFuseParams, MotionFuseInfo, SorParams, SorInfo, CarveParams, CarveInfo, RenderParams, RenderInfo, RenderCompareInfo, AlignParams, AlignInfo, GridParams, GridInfo, ObjectsParams, ObjectsInfo, ClearanceParams, ClearanceInfo, RouteParams, RouteInfo, RoutePathInfo, RelabelParams, RelabelInfo, RelabelHostView

KEYPOINT_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("size", "f4"), ("angle", "f4"), ("response", "f4"),
                           ("octave", "i4"), ("class_id", "i4")])
DMATCH_DTYPE = np.dtype([("queryIdx", "i4"), ("trainIdx", "i4"), ("imgIdx", "i4"), ("distance", "f4")])
POINT_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("z", "f4"), ("w", "f4"), ("b", "u1"), ("g", "u1"), ("r", "u1"),
                        ("a", "u1"), ("label", "u4"), ("pad", "u4", (2,))])
VOXEL_DTYPE = np.dtype([("key", "i8"), ("sx", "i8"), ("sy", "i8"), ("sz", "i8"), ("sr", "u8"), ("sg", "u8"),
                        ("sb", "u8"), ("n", "u8"), ("hist", "u4", (12,))])
PMATCH_DTYPE = np.dtype([("u1p", "f4"), ("v1p", "f4"), ("i1p", "i4"), ("u2p", "f4"), ("v2p", "f4"), ("i2p", "i4"), ("u1c", "f4"), ("v1c", "f4"),
                         ("i1c", "i4"), ("u2c", "f4"), ("v2c", "f4"), ("i2c", "i4"), ("dis_c", "i2"), ("dis_p", "i2")])
VO_PARAMS_DTYPE = np.dtype([("f", "f8"), ("cu", "f8"), ("cv", "f8"), ("base", "f8"), ("inlier_threshold", "f8"), ("reweighting", "i4"), ("pad", "i4")])
assert PMATCH_DTYPE.itemsize == 52
assert KEYPOINT_DTYPE.itemsize == 28 and DMATCH_DTYPE.itemsize == 16 and POINT_DTYPE.itemsize == 32 and VOXEL_DTYPE.itemsize == 112

STAGE_ORB, STAGE_MATCH, STAGE_MAP, STAGE_SEGNET = 1, 2, 4, 8
STEREO_QUAD, STEREO_DEPTH, STEREO_VO = 1, 2, 4
COMM_ID_BYTES = 128
SEG_NET_W, SEG_NET_H, SEG_CLASSES = 480, 360, 12


class GlibcRand:
    """The rand() stream VisualOdometry::getRandomSample draws from (srand(0) in the constructor, src/vo.cpp:17): glibc's TYPE_3 additive
    feedback generator, private to the object like in include/ssm/vo_stereo.hpp.  `draws(k)` returns the next k raw outputs (what the batched
    stereo path takes as rand_stream); `rewind(k)` gives unused draws back (frames with fewer than 6 quad matches draw nothing)."""

    def __init__(self, seed=0):
        seed = seed or 1
        r = [seed & 0xFFFFFFFF]
        for i in range(1, 31):
            hi, lo = divmod(r[i - 1] if r[i - 1] < 2 ** 31 else r[i - 1] - 2 ** 32, 127773)
            w = 16807 * lo - 2836 * hi
            if w < 0:
                w += 2147483647
            r.append(w & 0xFFFFFFFF)
        for i in range(31, 34):
            r.append(r[i - 31])
        self._r = r                      # the whole history is kept: rewinding is an index move
        self._pos = 34
        for _ in range(310):
            self._step()
        self._out = []                   # outputs from position _base on
        self._taken = 0

    def _step(self):
        r = self._r
        r.append((r[-3] + r[-31]) & 0xFFFFFFFF)
        return r[-1] >> 1

    def draws(self, k):
        while len(self._out) < self._taken + k:
            self._out.append(self._step())
        a = np.array(self._out[self._taken:self._taken + k], np.uint32)
        self._taken += k
        return a

    def rewind(self, k):
        assert 0 <= k <= self._taken
        self._taken -= k


class SsmError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"ssm error {code}: {msg}")
        self.code = code


def default_config(**kw):
    lib = _lib.load()
    cfg = Config()
    lib.ssm_config_default(C.byref(cfg))
    cam = kw.pop("camera", None)
    if cam is not None:
        cfg.camera = Camera(*cam)
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise KeyError(k)
        setattr(cfg, k, v)
    return cfg


def live_allocations():
    """(buffers, device bytes, pinned host bytes) the library itself holds right now, process-wide: ssm_debug_live_allocations"""
    n, d, p = C.c_int(0), C.c_size_t(0), C.c_size_t(0)
    _lib.load().ssm_debug_live_allocations(C.byref(n), C.byref(d), C.byref(p))
    return n.value, d.value, p.value


def live_handles():
    """(streams, events) the library itself holds right now, process-wide: ssm_debug_live_handles"""
    s, e = C.c_int(0), C.c_int(0)
    _lib.load().ssm_debug_live_handles(C.byref(s), C.byref(e))
    return s.value, e.value


def _ptr(a):
    return a.ctypes.data if a is not None else None


MOTION_FUSE_INFO_DTYPE = np.dtype([("blobs", "i4"), ("large", "i4"), ("confirmed", "i4"), ("added", "i4")])


def motion_fuse_tile():
    """(width, height) of the device labelling's tile: ssm_motion_fuse_tile"""
    wh = (C.c_int32 * 2)()
    _lib.load().ssm_motion_fuse_tile(C.byref(wh))
    return wh[0], wh[1]


def _mf_images(sem, motion):
    sem = np.ascontiguousarray(sem, np.uint8)
    if sem.ndim < 3 or sem.shape[-1] != 3:
        raise ValueError("sem: H x W x 3 (or n x H x W x 3)")
    if motion is not None:
        motion = np.ascontiguousarray(motion, np.uint8)
        if motion.shape != sem.shape[:-1]:
            raise ValueError("motion: the shape of sem without its channels")
    return sem, motion


def motion_fuse_host(sem, motion=None, area_thres=1000, overlay_thres=0.143, record=False):
    """the semantic-motion fusion on the CPU (ssm_motion_fuse_host, no GPU): -> (mask, info), or with record (mask, info, {labels, area, overlap, cand})"""
    sem, motion = _mf_images(sem, motion)
    h, w = sem.shape[:2]
    P = MotionFuseParams(int(area_thres), 0, float(overlay_thres)); I = MotionFuseInfo()
    mask = np.zeros((h, w), np.uint8)
    rec = {k: np.zeros((h, w), np.int32) for k in ("labels", "area", "overlap")} if record else {}
    if record:
        rec["cand"] = np.zeros((h, w), np.uint8)
    lib = _lib.load()
    rc = lib.ssm_motion_fuse_host(_ptr(sem), _ptr(motion), w, h, w * 3, C.byref(P), _ptr(mask), C.byref(I), _ptr(rec.get("labels")), _ptr(rec.get("area")),
                                  _ptr(rec.get("overlap")), _ptr(rec.get("cand")))
    if rc != 0:
        raise SsmError(rc, lib.ssm_last_error(None).decode())
    info = {k: getattr(I, k) for k in MOTION_FUSE_INFO_DTYPE.names}
    return (mask, info, rec) if record else (mask, info)


SOR_INFO_FIELDS = ("n_in", "n_finite", "n_kept", "too_few", "levels", "sum_q", "sum_q2_lo", "sum_q2_hi", "mean", "stddev", "threshold")


def pnp_lds_edge_capacity():
    """the largest number of correspondences whose edge list Context.pnp_solve keeps in LDS: ssm_pnp_lds_edge_capacity"""
    return _lib.load().ssm_pnp_lds_edge_capacity()


def sor_chunk():
    """candidates per LDS chunk of the device search: ssm_sor_chunk"""
    return _lib.load().ssm_sor_chunk()


def _sor_points(points):
    points = np.ascontiguousarray(points)
    if points.dtype != POINT_DTYPE or points.ndim != 1:
        raise ValueError("points: a 1-D array of POINT_DTYPE")
    return points


def sor_filter_host(points, mean_k=30, stddev_mul=1.0, cell=0.0, record=False):
    """the statistical outlier removal on the CPU (ssm_sor_filter_host, no GPU): -> (points, info), or with record (points, info, {mean_dist, keep})"""
    points = _sor_points(points)
    n = len(points)
    P = SorParams(int(mean_k), float(cell), float(stddev_mul)); I = SorInfo()
    out = np.zeros(n, POINT_DTYPE); got = C.c_int(0)
    rec = {"mean_dist": np.zeros(n, np.float32), "keep": np.zeros(n, np.uint8)} if record else {}
    lib = _lib.load()
    rc = lib.ssm_sor_filter_host(_ptr(points), n, C.byref(P), _ptr(out), n, C.byref(got), C.byref(I), _ptr(rec.get("mean_dist")), _ptr(rec.get("keep")))
    if rc != 0:
        raise SsmError(rc, lib.ssm_last_error(None).decode())
    info = {k: getattr(I, k) for k in SOR_INFO_FIELDS}
    return (out[:got.value], info, rec) if record else (out[:got.value], info)


CARVE_INFO_FIELDS = ("n_in", "n_kept", "unknown", "occluded", "supported", "seen_through", "removed")
CARVE_DEFAULTS = dict(min_votes=2, radius=1, tol_abs=0.05, tol_rel_ppm=20000, z_min=0.1)


def _carve_params(kw):
    bad = set(kw) - set(CARVE_DEFAULTS)
    if bad:
        raise TypeError("unknown carving parameters: " + ", ".join(sorted(bad)))
    p = dict(CARVE_DEFAULTS, **kw)
    return CarveParams(int(p["min_votes"]), int(p["radius"]), float(p["tol_abs"]), int(p["tol_rel_ppm"]), 0, float(p["z_min"]))


def _cm16(T):
    """a 4 x 4 pose as the ABI's 16 column-major doubles"""
    T = np.asarray(T, np.float64)
    if T.shape != (4, 4):
        raise ValueError("a pose is a 4 x 4 matrix")
    return np.ascontiguousarray(T.T).reshape(16)


RENDER_INFO_FIELDS = ("n_in", "n_visible", "n_covered")
RENDER_COMPARE_FIELDS = ("unrendered", "no_depth", "in_front", "behind", "agree", "label_agree", "label_disagree", "label_unknown", "n_pixels")
RENDER_DEFAULTS = dict(point_size=0.0, max_radius=3, z_min=0.1, z_max=1.0e9, tol_abs=0.05, tol_rel_ppm=20000)


def _render_params(kw):
    bad = set(kw) - set(RENDER_DEFAULTS)
    if bad:
        raise TypeError("unknown rendering parameters: " + ", ".join(sorted(bad)))
    p = dict(RENDER_DEFAULTS, **kw)
    return RenderParams(float(p["point_size"]), int(p["max_radius"]), 0, float(p["z_min"]), float(p["z_max"]), float(p["tol_abs"]), int(p["tol_rel_ppm"]), 0)


def _pack_clouds(clouds, T_clouds, host):
    """a list of clouds and their poses as the ABI takes them: host arrays (host=True) -> (the arrays kept alive, pointer array, sizes, poses, m); device
    handles -> (the handles, pointer array, None, poses, m).  The poses are m x 16 column-major doubles"""
    clouds = [_sor_points(c) for c in clouds] if host else list(clouds)
    m = len(clouds)
    if len(T_clouds) != m:
        raise ValueError("one pose per cloud")
    ptrs = (C.c_void_p * max(m, 1))(*([c.ctypes.data for c in clouds] if host else clouds))
    n = np.ascontiguousarray([len(c) for c in clouds] + ([] if m else [0]), np.int32) if host else None
    Tc = np.ascontiguousarray(np.stack([_cm16(T) for T in T_clouds]) if m else np.zeros((1, 16)))
    return clouds, ptrs, n, Tc, m


def _render_images(w, h, keys):
    out = {"depth": np.zeros((h, w), np.uint16), "bgr": np.zeros((h, w, 3), np.uint8), "label": np.zeros((h, w), np.uint8), "index": np.zeros((h, w), np.int32)}
    if keys:
        out["keys"] = np.zeros((h, w), np.uint64)
    return out


def render_host(w, h, camera, T_view, clouds, T_clouds, keys=False, **params):
    """map rendering on the CPU (ssm_render_host, no GPU): the points of `clouds` (host arrays of POINT_DTYPE at the poses T_clouds) into the w x h view (camera =
    (cx, cy, fx, fy, scale), T_view) -> {depth, bgr, label, index, info}, with keys=True also the raw z-buffer"""
    keep, ptrs, n, Tc, m = _pack_clouds(clouds, T_clouds, True)
    P = _render_params(params); I = RenderInfo(); cam = Camera(*camera)
    out = _render_images(int(w), int(h), keys) if w >= 1 and h >= 1 and w * h <= 1 << 26 else _render_images(1, 1, keys)
    lib = _lib.load()
    rc = lib.ssm_render_host(int(w), int(h), C.byref(cam), _ptr(_cm16(T_view)), ptrs, _ptr(n), _ptr(Tc), m, C.byref(P), _ptr(out["depth"]), _ptr(out["bgr"]), _ptr(out["label"]),
                             _ptr(out["index"]), _ptr(out.get("keys")), C.byref(I))
    if rc != 0:
        raise SsmError(rc, lib.ssm_last_error(None).decode())
    out["info"] = {k: getattr(I, k) for k in RENDER_INFO_FIELDS}
    return out


def _compare_frame(shape, depth, sem):
    depth = np.ascontiguousarray(depth, np.uint16); sem = np.ascontiguousarray(sem, np.uint8)
    if depth.shape != shape or sem.shape != shape + (3,):
        raise ValueError("the frame's images must have the rendering's size")
    return depth, sem


def render_compare_host(rendered_depth, rendered_label, depth, sem, scale, class_image=False, **params):
    """the rendering (its depth and label images) against a frame's depth and semantic BGR image on the CPU (ssm_render_compare_host) -> the nine counts, or with
    class_image (counts, the class image)"""
    rd = np.ascontiguousarray(rendered_depth, np.uint16); rl = np.ascontiguousarray(rendered_label, np.uint8)
    h, w = rd.shape
    if rl.shape != (h, w):
        raise ValueError("depth and label of one rendering")
    depth, sem = _compare_frame((h, w), depth, sem)
    P = _render_params(params); I = RenderCompareInfo()
    cls = np.zeros((h, w), np.uint8) if class_image else None
    lib = _lib.load()
    rc = lib.ssm_render_compare_host(_ptr(rd), _ptr(rl), w, h, _ptr(depth), _ptr(sem), float(scale), C.byref(P), C.byref(I), _ptr(cls))
    if rc != 0:
        raise SsmError(rc, lib.ssm_last_error(None).decode())
    info = {k: getattr(I, k) for k in RENDER_COMPARE_FIELDS}
    return (info, cls) if class_image else info


def label_colours(label):
    """a label image -> its BGR image through the project's 12-class palette (255 and anything else: black)"""
    label = np.ascontiguousarray(label, np.uint8)
    out = np.zeros(label.shape + (3,), np.uint8)
    _lib.load().ssm_render_label_colours(_ptr(label), label.size, _ptr(out))
    return out


GRID_INFO_FIELDS = ("n_in", "n_finite", "out_of_band", "outside", "n_used", "unobserved", "drivable", "walkable", "other_ground", "obstacle")
GRID_ARRAYS = (("cls", np.uint8), ("ground_label", np.uint8), ("obstacle_label", np.uint8), ("ground_q", np.int32), ("top_q", np.int32), ("n", np.uint32), ("n_high", np.uint32))
GRID_CELL_DTYPE = np.dtype([("n", "u4"), ("hmin", "i4"), ("hmax", "i4"), ("base", "i4"), ("n_low", "u4"), ("n_high", "u4"), ("sum_low", "i8"),
                            ("hist_low", "u4", (12,)), ("hist_high", "u4", (12,))])
GRID_FIELDS = ("G", "x0", "y0", "cell", "nx", "ny", "h_min", "h_max", "step", "ground_radius", "min_obstacle_points")


def grid_params(**kw):
    """the ground grid's parameters (ssm_grid_params): the library's defaults (ssm_grid_params_default) with the given fields replaced; G: 3 x 4, world -> grid"""
    bad = set(kw) - set(GRID_FIELDS)
    if bad:
        raise TypeError("unknown grid parameters: " + ", ".join(sorted(bad)))
    P = GridParams()
    _lib.load().ssm_grid_params_default(C.byref(P))
    for k, v in kw.items():
        if k == "G":
            G = np.ascontiguousarray(v, np.float64)
            if G.size != 12:
                raise ValueError("G is a 3 x 4 matrix")
            P.G = (C.c_double * 12)(*G.reshape(12))
        else:
            setattr(P, k, int(v) if k in ("nx", "ny", "ground_radius", "min_obstacle_points") else float(v))
    return P


def grid_frame_from_up(up, forward):
    """G (3 x 4, translation 0) for a world whose up and forward directions are given (ssm_grid_frame_from_up)"""
    up = np.ascontiguousarray(up, np.float64); fw = np.ascontiguousarray(forward, np.float64)
    if up.shape != (3,) or fw.shape != (3,):
        raise ValueError("up and forward are three numbers each")
    G = np.zeros((3, 4))
    lib = _lib.load()
    rc = lib.ssm_grid_frame_from_up(_ptr(up), _ptr(fw), _ptr(G))
    if rc != 0:
        raise SsmError(rc, lib.ssm_last_error(None).decode())
    return G


def _grid_arrays(nx, ny, cells):
    ok = nx >= 1 and ny >= 1 and nx * ny <= 1 << 24
    shape = (ny, nx) if ok else (1, 1)
    out = {k: np.zeros(shape, t) for k, t in GRID_ARRAYS}
    if cells:
        out["cells"] = np.zeros(shape, GRID_CELL_DTYPE)
    return out


def grid_host(clouds, T_clouds, cells=False, **params):
    """the ground grid on the CPU (ssm_grid_host, no GPU): the points of `clouds` (host arrays of POINT_DTYPE at the poses T_clouds) -> {cls, ground_label,
    obstacle_label, ground_q, top_q, n, n_high: ny x nx arrays, info}, with cells=True also the raw accumulators (GRID_CELL_DTYPE)"""
    keep, ptrs, n, Tc, m = _pack_clouds(clouds, T_clouds, True)
    P = grid_params(**params); I = GridInfo()
    out = _grid_arrays(P.nx, P.ny, cells)
    lib = _lib.load()
    rc = lib.ssm_grid_host(ptrs, _ptr(n), _ptr(Tc), m, C.byref(P), *[_ptr(out[k]) for k, _ in GRID_ARRAYS], _ptr(out.get("cells")), C.byref(I))
    if rc != 0:
        raise SsmError(rc, lib.ssm_last_error(None).decode())
    out["info"] = {k: getattr(I, k) for k in GRID_INFO_FIELDS}
    return out


def grid_colours(cls, ground_label, obstacle_label, ground_q, h_min=-3.0):
    """the cell arrays (ny x nx) -> (the BGR image, the 16-bit height image), forward up (ssm_grid_colours)"""
    cls = np.ascontiguousarray(cls, np.uint8); gl = np.ascontiguousarray(ground_label, np.uint8); ol = np.ascontiguousarray(obstacle_label, np.uint8)
    gq = np.ascontiguousarray(ground_q, np.int32)
    if cls.ndim != 2 or gl.shape != cls.shape or ol.shape != cls.shape or gq.shape != cls.shape:
        raise ValueError("four ny x nx arrays of one grid")
    ny, nx = cls.shape
    bgr = np.zeros((ny, nx, 3), np.uint8); height = np.zeros((ny, nx), np.uint16)
    _lib.load().ssm_grid_colours(_ptr(cls), _ptr(gl), _ptr(ol), _ptr(gq), nx, ny, float(h_min), _ptr(bgr), _ptr(height))
    return bgr, height


OBJECTS_INFO_FIELDS = ("member_cells", "components", "kept", "rejected_cells", "rejected_points", "rejected_height", "n_in", "object_points")
OBJECTS_FIELDS = ("label_mask", "connectivity", "min_cells", "min_points", "min_height")
OBJECT_DTYPE = np.dtype([("root", "i4"), ("label", "i4"), ("cells", "u4"), ("n_points", "u4"), ("cell_points", "u8"), ("cx_min", "i4"), ("cx_max", "i4"), ("cy_min", "i4"),
                         ("cy_max", "i4"), ("ground_q", "i4"), ("top_q", "i4"), ("x_min_q", "i4"), ("x_max_q", "i4"), ("y_min_q", "i4"), ("y_max_q", "i4"), ("z_min_q", "i4"),
                         ("z_max_q", "i4"), ("n_label", "u4"), ("pad", "u4"), ("sum_x", "i8"), ("sum_y", "i8"), ("sum_z", "i8")])


def objects_params(**kw):
    """object extraction's parameters (ssm_objects_params): the library's defaults (ssm_objects_params_default) with the given fields replaced; labels=[ids] sets
    label_mask from a list of label ids"""
    bad = set(kw) - set(OBJECTS_FIELDS) - {"labels"}
    if bad:
        raise TypeError("unknown object parameters: " + ", ".join(sorted(bad)))
    P = ObjectsParams()
    _lib.load().ssm_objects_params_default(C.byref(P))
    for k, v in kw.items():
        if k == "labels":
            P.label_mask = sum({1 << int(l) for l in v if 0 <= int(l) < 32})
        elif k == "min_height":
            P.min_height = float(v)
        else:
            setattr(P, k, int(v))
    return P


def _objects_info(I):
    return {k: getattr(I, k) for k in OBJECTS_INFO_FIELDS}


def objects_cells_host(cls, obstacle_label, ground_q, top_q, n_high, cap=None, **params):
    """stage 1 of object extraction on the CPU (ssm_objects_cells_host, no GPU) from the ny x nx cell arrays of a grid -> (records of OBJECT_DTYPE, the object_id
    image, info); cap: the record buffer's size (default: enough)"""
    arr = [np.ascontiguousarray(a, t) for a, t in ((cls, np.uint8), (obstacle_label, np.uint8), (ground_q, np.int32), (top_q, np.int32), (n_high, np.uint32))]
    if arr[0].ndim != 2 or any(a.shape != arr[0].shape for a in arr):
        raise ValueError("five ny x nx arrays of one grid")
    ny, nx = arr[0].shape
    P = objects_params(**params); I = ObjectsInfo(); n = C.c_int(0)
    cap = nx * ny if cap is None else int(cap)
    out = np.zeros(max(cap, 1), OBJECT_DTYPE); ids = np.full((ny, nx), -2, np.int32)
    lib = _lib.load()
    rc = lib.ssm_objects_cells_host(*[_ptr(a) for a in arr], nx, ny, C.byref(P), _ptr(out), cap, C.byref(n), _ptr(ids), C.byref(I))
    if rc != 0:
        raise SsmError(rc, lib.ssm_last_error(None).decode())
    return out[:n.value].copy(), ids, _objects_info(I)


def objects_host(clouds, T_clouds, grid=None, cap=None, **params):
    """the ground grid, then both stages of object extraction, on the CPU (ssm_objects_host, no GPU): `clouds` (host arrays of POINT_DTYPE at the poses T_clouds),
    grid: the grid's parameters as a dictionary -> (records, the object_id image, the per-point object ids of the concatenation, info)"""
    keep, ptrs, n, Tc, m = _pack_clouds(clouds, T_clouds, True)
    G = grid_params(**(grid or {})); P = objects_params(**params); I = ObjectsInfo(); k = C.c_int(0)
    ok = G.nx >= 1 and G.ny >= 1 and G.nx * G.ny <= 1 << 24
    shape = (G.ny, G.nx) if ok else (1, 1)
    cap = min(shape[0] * shape[1], 1 << 20) if cap is None else int(cap)
    out = np.zeros(max(cap, 1), OBJECT_DTYPE); oid = np.full(shape, -2, np.int32); ids = np.full(max(int(n[:m].sum()), 1), -2, np.int32)
    lib = _lib.load()
    rc = lib.ssm_objects_host(ptrs, _ptr(n), _ptr(Tc), m, C.byref(G), C.byref(P), _ptr(out), cap, C.byref(k), _ptr(oid), _ptr(ids), C.byref(I))
    if rc != 0:
        raise SsmError(rc, lib.ssm_last_error(None).decode())
    return out[:k.value].copy(), oid, ids[:int(n[:m].sum())].copy(), _objects_info(I)


CLEARANCE_INFO_FIELDS = ("blocked", "free_cells", "traversable", "components", "reachable", "seed_cell", "max_d2_reachable", "r2")
CLEARANCE_FIELDS = ("blocked_mask", "free_mask", "connectivity", "seed_cx", "seed_cy", "seed_snap", "radius", "cell")


def clearance_params(**kw):
    """the clearance map's parameters (ssm_clearance_params): the library's defaults (ssm_clearance_params_default) with the given fields replaced; blocked=[ids] and
    free=[ids] set the masks from lists of cell classes, seed=(cx, cy) the seed cell"""
    bad = set(kw) - set(CLEARANCE_FIELDS) - {"blocked", "free", "seed"}
    if bad:
        raise TypeError("unknown clearance parameters: " + ", ".join(sorted(bad)))
    P = ClearanceParams()
    _lib.load().ssm_clearance_params_default(C.byref(P))
    for k, v in kw.items():
        if k in ("blocked", "free"):
            setattr(P, k + "_mask", sum({1 << int(c) for c in v if 0 <= int(c) < 32}))
        elif k == "seed":
            P.seed_cx, P.seed_cy = (-1, -1) if v is None else (int(v[0]), int(v[1]))
        elif k in ("radius", "cell"):
            setattr(P, k, float(v))
        else:
            setattr(P, k, int(v))
    return P


def _clearance_info(I):
    return {k: getattr(I, k) for k in CLEARANCE_INFO_FIELDS}


def _clearance_cls(cls):
    a = np.ascontiguousarray(cls, np.uint8)
    if a.ndim != 2:
        raise ValueError("a ny x nx array of cell classes")
    return a


def clearance_cells_host(cls, **params):
    """the clearance map on the CPU (ssm_clearance_cells_host, no GPU) from the ny x nx class image of a grid -> (dist2 uint32, nearest int32, reach uint8, info)"""
    a = _clearance_cls(cls)
    ny, nx = a.shape
    P = clearance_params(**params); I = ClearanceInfo()
    d2 = np.zeros((ny, nx), np.uint32); near = np.full((ny, nx), -2, np.int32); reach = np.full((ny, nx), 255, np.uint8)
    lib = _lib.load()
    rc = lib.ssm_clearance_cells_host(_ptr(a), nx, ny, C.byref(P), _ptr(d2), _ptr(near), _ptr(reach), C.byref(I))
    if rc != 0:
        raise SsmError(rc, lib.ssm_last_error(None).decode())
    return d2, near, reach, _clearance_info(I)


ROUTE_INFO_FIELDS = ("routed", "unrouted", "near_cells", "max_cost", "far_cell", "source_cell", "comfort2", "moves")
ROUTE_PATH_INFO_FIELDS = ("len", "goal_cell", "cost", "n_axial", "n_diag", "near_steps", "min_d2")
ROUTE_FIELDS = ("moves", "near_weight", "comfort", "cell")
COST_NONE = 0xFFFFFFFF


def route_params(**kw):
    """the route field's parameters (ssm_route_params): the library's defaults (ssm_route_params_default) with the given fields replaced"""
    bad = set(kw) - set(ROUTE_FIELDS)
    if bad:
        raise TypeError("unknown route parameters: " + ", ".join(sorted(bad)))
    P = RouteParams()
    _lib.load().ssm_route_params_default(C.byref(P))
    for k, v in kw.items():
        setattr(P, k, float(v) if k in ("comfort", "cell") else int(v))
    return P


def _route_info(I):
    return {k: getattr(I, k) for k in ROUTE_INFO_FIELDS}


def _route_path_info(I):
    return {k: getattr(I, k) for k in ROUTE_PATH_INFO_FIELDS}


def _route_inputs(reach, dist2, source):
    """-> (reach uint8, dist2 uint32, the source as a cell index or -1); source: None, an index or (cx, cy)"""
    r = np.ascontiguousarray(reach, np.uint8); d = np.ascontiguousarray(dist2, np.uint32)
    if r.ndim != 2 or d.shape != r.shape:
        raise ValueError("two ny x nx arrays of one grid")
    if source is None:
        return r, d, -1
    if isinstance(source, (tuple, list)):
        return r, d, int(source[1]) * r.shape[1] + int(source[0])
    return r, d, int(source)


def route_cells_host(reach, dist2, source=None, **params):
    """the route field on the CPU (ssm_route_cells_host, no GPU) from the ny x nx reach and dist2 images of a clearance map and the source cell (None, an index or
    (cx, cy)) -> (cost uint32, parent int32, info)"""
    r, d, src = _route_inputs(reach, dist2, source)
    ny, nx = r.shape
    P = route_params(**params); I = RouteInfo()
    cost = np.zeros((ny, nx), np.uint32); parent = np.full((ny, nx), -2, np.int32)
    lib = _lib.load()
    rc = lib.ssm_route_cells_host(_ptr(r), _ptr(d), nx, ny, src, C.byref(P), _ptr(cost), _ptr(parent), C.byref(I))
    if rc != 0:
        raise SsmError(rc, lib.ssm_last_error(None).decode())
    return cost, parent, _route_info(I)


def route_path_host(cost, parent, dist2, goal, goal_snap=0, max_path=None, **params):
    """a path on the CPU (ssm_route_path_host) from a field's ny x nx cost and parent images and the clearance map's dist2 to the goal (cx, cy) -> (the path's cell
    indices int32, source first, path info).  A path longer than max_path (default: the cells of the grid) raises SsmError with code SSM_E_CAPACITY; its `info`
    attribute holds the path info"""
    c = np.ascontiguousarray(cost, np.uint32); p = np.ascontiguousarray(parent, np.int32); d = np.ascontiguousarray(dist2, np.uint32)
    if c.ndim != 2 or p.shape != c.shape or d.shape != c.shape:
        raise ValueError("three ny x nx arrays of one grid")
    ny, nx = c.shape
    max_path = nx * ny if max_path is None else int(max_path)
    P = route_params(**params); I = RoutePathInfo()
    cells = np.full(max(max_path, 1), -2, np.int32)
    lib = _lib.load()
    rc = lib.ssm_route_path_host(_ptr(c), _ptr(p), _ptr(d), nx, ny, C.byref(P), int(goal[0]), int(goal[1]), int(goal_snap), max_path, _ptr(cells), C.byref(I))
    if rc != 0:
        e = SsmError(rc, lib.ssm_last_error(None).decode()); e.info = _route_path_info(I)
        raise e
    return cells[:I.len].copy(), _route_path_info(I)


RELABEL_INFO_FIELDS = ("n_in", "n_supported", "n_voted", "n_changed", "n_filled", "pairs_supported", "pairs_voted")
RELABEL_FIELDS = ("radius", "edge_guard", "own_weight", "min_votes", "tol_abs", "tol_rel_ppm", "z_min")


def relabel_params(**kw):
    """label fusion's parameters (ssm_relabel_params): the library's defaults (ssm_relabel_params_default) with the given fields replaced"""
    bad = set(kw) - set(RELABEL_FIELDS)
    if bad:
        raise TypeError("unknown label-fusion parameters: " + ", ".join(sorted(bad)))
    P = RelabelParams()
    _lib.load().ssm_relabel_params_default(C.byref(P))
    for k, v in kw.items():
        setattr(P, k, float(v) if k in ("tol_abs", "z_min") else int(v))
    return P


def relabel_labels_host(sem_bgr):
    """the label image of a semantic BGR image (h x w x 3 uint8) on the CPU (ssm_relabel_labels_host): the palette's class, 255 for any other colour"""
    sem = np.ascontiguousarray(sem_bgr, np.uint8)
    if sem.ndim != 3 or sem.shape[2] != 3:
        raise ValueError("sem_bgr: h x w x 3")
    out = np.zeros(sem.shape[:2], np.uint8)
    lib = _lib.load()
    rc = lib.ssm_relabel_labels_host(_ptr(sem), sem.shape[0] * sem.shape[1], _ptr(out))
    if rc != 0:
        raise SsmError(rc, lib.ssm_last_error(None).decode())
    return out


def _relabel_poses(T_views):
    v = len(T_views)
    return np.ascontiguousarray(np.stack([_cm16(T) for T in T_views]) if v else np.zeros((1, 16)))


def _relabel_info(I):
    return {k: getattr(I, k) for k in RELABEL_INFO_FIELDS}


def relabel_host(views, T_views, points, T_cloud, **params):
    """label fusion on the CPU (ssm_relabel_host, no GPU): views is a list of (depth h x w uint16, label h x w uint8, camera = (cx, cy, fx, fy, scale)) at the world
    poses T_views; they vote on the labels of `points`, a cloud at T_cloud -> (labels, votes, info): every point's label afterwards and its packed counts"""
    points = _sor_points(points)
    n, v = len(points), len(views)
    if len(T_views) != v:
        raise ValueError("one pose per view")
    keep = []; arr = (RelabelHostView * max(v, 1))()
    for k, (depth, label, camera) in enumerate(views):
        depth = np.ascontiguousarray(depth, np.uint16); label = np.ascontiguousarray(label, np.uint8)
        if depth.ndim != 2 or label.shape != depth.shape:
            raise ValueError("a view's depth and label images have one size")
        keep.append((depth, label))
        arr[k] = RelabelHostView(depth.ctypes.data, label.ctypes.data, depth.shape[1], depth.shape[0], Camera(*camera))
    P = relabel_params(**params); I = RelabelInfo()
    labels = np.zeros(n, np.uint32); votes = np.zeros(n, np.uint64)
    lib = _lib.load()
    Tv, Tc = _relabel_poses(T_views), _cm16(T_cloud)          # (named: a pointer does not keep its array alive)
    rc = lib.ssm_relabel_host(arr, _ptr(Tv), v, _ptr(points), n, _ptr(Tc), C.byref(P), _ptr(labels), _ptr(votes), C.byref(I))
    if rc != 0:
        raise SsmError(rc, lib.ssm_last_error(None).decode())
    return labels, votes, _relabel_info(I)


ALIGN_STATUS = ("max_iterations", "converged", "too_few", "degenerate", "diverged")
ALIGN_INFO_FIELDS = ("status", "iterations", "n_in", "tested_first", "inliers_first", "tested_last", "inliers_last", "chi2_first", "chi2_last")
ALIGN_DEFAULTS = dict(max_iterations=10, stride=1, z_min=0.1, z_max=80.0, dist_max=0.25, delta=0.05, damping=1.0e-6, eps_rot=1.0e-4, eps_trans=1.0e-4, min_inliers=1000,
                      max_shift=1.0, max_angle=0.2, tol_abs=0.05, tol_rel_ppm=20000)
ALIGN_NSUM = 30
ALIGN_ITER_DTYPE = np.dtype([("sums", np.int64, (ALIGN_NSUM,)), ("E", np.float64, (12,))])
ALIGN_MAX_ITERATIONS = 64


def align_params(**kw):
    """the parameters of dense alignment as the ABI's struct: ALIGN_DEFAULTS with kw on top"""
    bad = set(kw) - set(ALIGN_DEFAULTS)
    if bad:
        raise TypeError("unknown alignment parameters: " + ", ".join(sorted(bad)))
    p = dict(ALIGN_DEFAULTS, **kw)
    return AlignParams(int(p["max_iterations"]), int(p["stride"]), float(p["z_min"]), float(p["z_max"]), float(p["dist_max"]), float(p["delta"]), float(p["damping"]),
                       float(p["eps_rot"]), float(p["eps_trans"]), int(p["min_inliers"]), 0, float(p["max_shift"]), float(p["max_angle"]), float(p["tol_abs"]),
                       int(p["tol_rel_ppm"]), 0)


def _align_info(I):
    out = {k: getattr(I, k) for k in ALIGN_INFO_FIELDS}
    out["E"] = np.array(I.E, np.float64).reshape(4, 4).T.copy()
    return out


def align_host(depth, camera, T_view, clouds, T_clouds, **params):
    """dense alignment on the CPU (ssm_align_host, no GPU): the points of `clouds` (host arrays of POINT_DTYPE at the poses T_clouds) against the view `depth`
    (uint16, camera = (cx, cy, fx, fy, scale)) from the pose T_view -> {T_view, info, valid, normals (h x w x 4 floats), record (one ALIGN_ITER_DTYPE entry per
    iteration)}"""
    depth = np.ascontiguousarray(depth, np.uint16)
    if depth.ndim != 2:
        raise ValueError("a depth image is h x w")
    h, w = depth.shape
    keep, ptrs, n, Tc, m = _pack_clouds(clouds, T_clouds, True)
    P = align_params(**params); I = AlignInfo(); cam = Camera(*camera)
    valid = np.zeros((h, w), np.uint8); normals = np.zeros((h, w, 4), np.float32); rec = np.zeros(ALIGN_MAX_ITERATIONS, ALIGN_ITER_DTYPE); nrec = C.c_int(0)
    T_out = np.zeros(16)
    lib = _lib.load()
    rc = lib.ssm_align_host(_ptr(depth), w, h, C.byref(cam), _ptr(_cm16(T_view)), ptrs, _ptr(n), _ptr(Tc), m, C.byref(P), _ptr(T_out), C.byref(I), _ptr(valid), _ptr(normals),
                            _ptr(rec), len(rec), C.byref(nrec))
    if rc != 0:
        raise SsmError(rc, lib.ssm_last_error(None).decode())
    return {"T_view": T_out.reshape(4, 4).T.copy(), "info": _align_info(I), "valid": valid, "normals": normals, "record": rec[:nrec.value].copy()}


def _carve_run(run, n):
    run = np.zeros(n, np.uint8) if run is None else np.array(run, np.uint8)          # (a copy: the call compacts it in place)
    if run.shape != (n,):
        raise ValueError("run: one uint8 per point")
    return run


def _carve_info(I):
    return {k: getattr(I, k) for k in CARVE_INFO_FIELDS}


def carve_host(depth, camera, T_view, points, T_cloud, run=None, record=False, **params):
    """free-space carving on the CPU (ssm_carve_host, no GPU): the view (depth, camera = (cx, cy, fx, fy, scale), T_view) judges `points` of a cloud at T_cloud whose run
    counters are `run` (None: zero) -> (points, run, info), or with record (points, run, info, {verdict, run}: every point's, before the compaction)"""
    depth = np.ascontiguousarray(depth, np.uint16); points = _sor_points(points)
    h, w = depth.shape
    n = len(points)
    P = _carve_params(params); I = CarveInfo(); cam = Camera(*camera)
    Tv, Tc = _cm16(T_view), _cm16(T_cloud)
    run = _carve_run(run, n)
    out = np.zeros(n, POINT_DTYPE); got = C.c_int(0)
    rec = {"verdict": np.zeros(n, np.uint8), "run": np.zeros(n, np.uint8)} if record else {}
    lib = _lib.load()
    rc = lib.ssm_carve_host(_ptr(depth), w, h, C.byref(cam), _ptr(Tv), _ptr(points), n, _ptr(Tc), _ptr(run), C.byref(P), _ptr(out), n, C.byref(got), C.byref(I),
                            _ptr(rec.get("verdict")), _ptr(rec.get("run")))
    if rc != 0:
        raise SsmError(rc, lib.ssm_last_error(None).decode())
    res = (out[:got.value], run[:got.value], _carve_info(I))
    return res + (rec,) if record else res


def _rows(a):
    """an 8-bit image whose pixels are adjacent inside a row: a row-strided 2-D view passes as it is (the ABI takes the row stride), anything else is packed"""
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 2 or a.shape[1] == 0 or a.strides[1] != 1 or a.strides[0] < a.shape[1]:
        a = np.ascontiguousarray(a, np.uint8)
    return a


TRACK_INFO_DTYPE = np.dtype([("state", "i4"), ("tracked", "i4"), ("n_matches", "i4"), ("n_inliers", "i4")])


class Tracker:
    """ssm_tracker: Tracker::updateFrame (RGB-D mode, src/track.cpp:8-36,140-212) for all frames of a seq_process call -- the bulk consumer of the
    match tables.  run(out, n) -> (poses n x 4 x 4 = T_f_w per frame, info structured array)."""

    def __init__(self, ctx, max_lost_frame=10, pnp_min_inliers=10, use_device=False, first_pose=None, own_stream=False, blocks=0):
        self.ctx = ctx; self.lib = ctx.lib
        p = TrackerParams()
        self.lib.ssm_tracker_params_default(C.byref(p))
        p.max_lost_frame = max_lost_frame; p.ref_frames = ctx.R; p.pnp_min_inliers = pnp_min_inliers; p.use_device = int(use_device); p.own_stream = int(own_stream); p.blocks = int(blocks)
        if first_pose is not None:
            fp = np.ascontiguousarray(np.asarray(first_pose, np.float64).reshape(4, 4).T).reshape(16)       # column-major
            for i in range(16):
                p.first_pose[i] = float(fp[i])
        h = C.c_void_p()
        rc = self.lib.ssm_tracker_create(ctx.h, C.byref(p), C.byref(h))
        if rc != 0:
            raise SsmError(rc, "ssm_tracker_create")
        self.h = h

    def reset(self):
        self.lib.ssm_tracker_reset(self.h)

    def run(self, seq_out, n):
        poses = np.zeros((max(n, 1), 16), np.float64); info = np.zeros(max(n, 1), TRACK_INFO_DTYPE)
        rc = self.lib.ssm_tracker_run(self.h, C.byref(seq_out), n, _ptr(poses), _ptr(info))
        if rc != 0:
            raise SsmError(rc, (self.lib.ssm_tracker_last_error(self.h) or b"").decode())
        return poses[:n].reshape(n, 4, 4).transpose(0, 2, 1).copy(), info[:n]

    def last_error(self):
        """the last call's error text, or a note (a downgrade of the device chain to one block) after a call that succeeded"""
        return (self.lib.ssm_tracker_last_error(self.h) or b"").decode()

    def stats(self):
        """(frames solved by the device chain, frames solved by the host path)"""
        a, b = C.c_int64(0), C.c_int64(0)
        self.lib.ssm_tracker_stats(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def work(self):
        """device chain so far: (Levenberg iterations, chi2 passes, edges evaluated by the iterations' fused passes, edges evaluated by the chi2 passes)"""
        w = (C.c_int64 * 4)()
        self.lib.ssm_tracker_work(self.h, C.byref(w))
        return tuple(int(x) for x in w)

    def close(self):
        if self.h:
            self.lib.ssm_tracker_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Vocabulary:
    """ssm_vocab: a DBoW2 TemplatedVocabulary<FORB> (L1_NORM / TF_IDF), a host object that needs no GPU.  Vocabulary(path) loads DBoW2's text format;
    Vocabulary.from_arrays(k, L, parent, is_leaf, desc, weight) builds one from the per-node arrays (node i has id i + 1, id 0 is the root)."""

    def __init__(self, path=None, _handle=None):
        self.lib = _lib.load()
        if _handle is None:
            h = C.c_void_p()
            rc = self.lib.ssm_vocab_load_text(str(path).encode(), C.byref(h))
            if rc != 0:
                raise SsmError(rc, (self.lib.ssm_last_error(None) or b"").decode())
            _handle = h
        self.h = _handle
        info = (C.c_int32 * 6)()
        self.lib.ssm_vocab_info(self.h, C.byref(info))
        self.k, self.L, self.nodes, self.words, self.scoring, self.weighting = (int(x) for x in info)

    @classmethod
    def from_arrays(cls, k, L, parent, is_leaf, desc, weight, scoring=0, weighting=0):
        lib = _lib.load()
        parent = np.ascontiguousarray(parent, np.int32); is_leaf = np.ascontiguousarray(is_leaf, np.uint8)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32); weight = np.ascontiguousarray(weight, np.float64)
        assert len(parent) == len(is_leaf) == len(desc) == len(weight)
        h = C.c_void_p()
        rc = lib.ssm_vocab_create(k, L, scoring, weighting, _ptr(parent), _ptr(is_leaf), _ptr(desc), _ptr(weight), len(parent), C.byref(h))
        if rc != 0:
            raise SsmError(rc, (lib.ssm_last_error(None) or b"").decode())
        return cls(_handle=h)

    @classmethod
    def train(cls, desc_sets, k=10, L=5, max_iters=32, ctx=None):
        """A vocabulary from the descriptor sets of a sequence (one n_f x 32 array per frame; empty ones allowed): the hierarchical k-majority tree of
        DESIGN.md s.13.  ctx None: the host function; else the device trainer of that context -- the same bytes either way.  The result carries
        `report` (nodes, words, levels, capped_nodes, passes per level) and `word_of_feature` (the word each training descriptor was trained into)."""
        lib = _lib.load()
        sets = [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in desc_sets]
        npf = np.array([len(d) for d in sets], np.int32)
        desc = np.ascontiguousarray(np.concatenate(sets)) if sets else np.zeros((0, 32), np.uint8)
        p = VocabTrainParams(int(k), int(L), int(max_iters)); rep = VocabTrainReport(); h = C.c_void_p()
        wof = np.zeros(max(len(desc), 1), np.int32)
        if ctx is None:
            rc = lib.ssm_vocab_train_host(_ptr(desc), _ptr(npf), len(npf), C.byref(p), _ptr(wof), C.byref(rep), C.byref(h))
        else:
            rc = lib.ssm_vocab_train(ctx.h, _ptr(desc), _ptr(npf), len(npf), C.byref(p), _ptr(wof), C.byref(rep), C.byref(h))
        if rc != 0:
            raise SsmError(rc, (lib.ssm_last_error(ctx.h if ctx is not None else None) or b"").decode())
        v = cls(_handle=h)
        v.report = {"nodes": rep.nodes, "words": rep.words, "levels": rep.levels, "capped_nodes": rep.capped_nodes, "passes": [int(x) for x in rep.passes]}
        v.word_of_feature = wof[:len(desc)]
        return v

    def arrays(self):
        """-> (parent, is_leaf, desc, weight) as from_arrays takes them: ssm_vocab_export"""
        n = self.nodes - 1
        parent = np.zeros(n, np.int32); leaf = np.zeros(n, np.uint8); desc = np.zeros((n, 32), np.uint8); weight = np.zeros(n, np.float64)
        rc = self.lib.ssm_vocab_export(self.h, _ptr(parent), _ptr(leaf), _ptr(desc), _ptr(weight), n)
        if rc != 0:
            raise SsmError(rc, "ssm_vocab_export")
        return parent, leaf, desc, weight

    def save(self, path):
        """DBoW2's text format, as Vocabulary(path) reads it; the weights come back bit for bit"""
        rc = self.lib.ssm_vocab_save_text(self.h, str(path).encode())
        if rc != 0:
            raise SsmError(rc, (self.lib.ssm_last_error(None) or b"").decode())

    def transform(self, desc, cap=None):
        """vocab.transform on the host -> (word id of every feature, vector ids, vector values)"""
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(desc); cap = n if cap is None else cap
        wof = np.zeros(max(n, 1), np.int32); ids = np.zeros(max(cap, 1), np.int32); vals = np.zeros(max(cap, 1), np.float64); m = C.c_int(0)
        rc = self.lib.ssm_vocab_transform_host(self.h, _ptr(desc), n, _ptr(wof), _ptr(ids), _ptr(vals), cap, C.byref(m))
        if rc != 0:
            e = SsmError(rc, "ssm_vocab_transform_host"); e.needed = m.value
            raise e
        return wof[:n], ids[:m.value].copy(), vals[:m.value].copy()

    def score(self, ids1, v1, ids2, v2):
        """vocab.score(v1, v2) on the host: v1 the query frame, v2 the stored frame"""
        ids1 = np.ascontiguousarray(ids1, np.int32); v1 = np.ascontiguousarray(v1, np.float64); ids2 = np.ascontiguousarray(ids2, np.int32); v2 = np.ascontiguousarray(v2, np.float64)
        s = C.c_double(0)
        rc = self.lib.ssm_bow_score_host(_ptr(ids1), _ptr(v1), len(ids1), _ptr(ids2), _ptr(v2), len(ids2), C.byref(s))
        if rc != 0:
            raise SsmError(rc, "ssm_bow_score_host")
        return s.value

    def close(self):
        if getattr(self, "h", None):
            self.lib.ssm_vocab_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def vocab_kmajority(desc, node_of, cluster_of, centres, ctx=None):
    """ssm_debug_vocab_kmajority: one k-majority pass (centre update, then assignment) on a made-up state.  centres: n_nodes x k x 32 -> (new centres, new clusters)"""
    lib = _lib.load()
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32); node_of = np.ascontiguousarray(node_of, np.int32); cluster_of = np.ascontiguousarray(cluster_of, np.int32)
    centres = np.array(centres, np.uint8, order="C"); n_nodes, k = centres.shape[0], centres.shape[1]
    assert centres.shape == (n_nodes, k, 32) and len(node_of) == len(cluster_of) == len(desc)
    out = np.zeros(max(len(desc), 1), np.int32)
    rc = lib.ssm_debug_vocab_kmajority(ctx.h if ctx is not None else None, _ptr(desc), len(desc), _ptr(node_of), _ptr(cluster_of), n_nodes, k, _ptr(centres), _ptr(out))
    if rc != 0:
        raise SsmError(rc, "ssm_debug_vocab_kmajority")
    return centres, out[:len(desc)]


class Looper:
    """ssm_looper: rgbd_tutor::Looper on the device -- the vocabulary tree and the database of the added frames' bag-of-words vectors live in the context's
    device memory.  add = Looper::add of one frame, add_dev the same for the frames of a seq_process call, query = Looper::getPossibleLoops in bulk."""

    def __init__(self, ctx, vocab):
        self.ctx = ctx; self.lib = ctx.lib
        h = C.c_void_p()
        ctx._chk(self.lib.ssm_looper_create(ctx.h, vocab.h, C.byref(h)))
        self.h = h

    def __len__(self):
        return self.lib.ssm_looper_size(self.h)

    def clear(self):
        self.ctx._chk(self.lib.ssm_looper_clear(self.h))

    def add(self, desc, frame_id):
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        self.ctx._chk(self.lib.ssm_looper_add(self.h, _ptr(desc), len(desc), int(frame_id)))

    def add_dev(self, seq_out, n, frame_ids):
        """the n frames of a seq_process output (device descriptors and counts as they are); enqueued, not waited for"""
        ids = np.ascontiguousarray(frame_ids, np.int32)
        assert len(ids) == n
        self.ctx._chk(self.lib.ssm_looper_add_dev(self.h, seq_out.desc, seq_out.nkp, n, seq_out.cap, _ptr(ids)))

    def bow(self, entry, cap=None):
        cap = self.ctx.cap if cap is None else cap
        ids = np.zeros(max(cap, 1), np.int32); vals = np.zeros(max(cap, 1), np.float64); m = C.c_int(0)
        self.ctx._chk(self.lib.ssm_looper_bow(self.h, entry, _ptr(ids), _ptr(vals), cap, C.byref(m)))
        return ids[:m.value].copy(), vals[:m.value].copy()

    def scores(self, entry, against=-1):
        out = np.zeros(max(entry + 1 if against < 0 else against, 1), np.float64)
        self.ctx._chk(self.lib.ssm_looper_scores(self.h, entry, against, _ptr(out)))
        return out[:entry + 1 if against < 0 else against]

    def query(self, first, n, min_sim_score, min_interval, against=-1, cap=None):
        """-> (pairs m x 2 [query entry, candidate entry], scores m), sorted by (query, candidate).  cap=None: retried once with the count the library reports"""
        auto = cap is None
        cap = 4096 if auto else cap
        while True:
            pairs = np.zeros((max(cap, 1), 2), np.int32); sc = np.zeros(max(cap, 1), np.float64); m = C.c_int(0)
            rc = self.lib.ssm_looper_query(self.h, first, n, against, float(min_sim_score), int(min_interval), _ptr(pairs), _ptr(sc), cap, C.byref(m))
            if rc == -4 and auto and m.value > cap:
                cap = m.value
                continue
            if rc != 0:
                e = SsmError(rc, (self.lib.ssm_last_error(self.ctx.h) or b"").decode()); e.needed = m.value
                raise e
            return pairs[:m.value].copy(), sc[:m.value].copy()

    def close(self):
        """before the context's close(): a looper that outlives its context is dropped without a call into it"""
        if getattr(self, "h", None):
            if self.ctx.h:
                self.lib.ssm_looper_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


UVD_INFO_DTYPE = np.dtype([("status", "i4"), ("v_cols", "i4"), ("u_rows", "i4"), ("otsu_threshold", "i4"), ("n_line_points", "i4"), ("slope", "f4"), ("v_c", "f8"),
                           ("pitch_measured", "f4"), ("pitch_filtered", "f4"), ("n_seeds", "i4"), ("n_masks_found", "i4"), ("n_masks_merged", "i4"),
                           ("n_masks_kept", "i4"), ("n_moving", "i4"), ("line", "f4", (4,)), ("pad", "i4")])
assert UVD_INFO_DTYPE.itemsize == C.sizeof(UvdInfo) == 80
UVD_TOO_LARGE, UVD_NO_LINE, UVD_SKIPPED = 1, 2, 4
UVD_STAGE_BLUR, UVD_STAGE_ERODE, UVD_STAGE_BIN, UVD_STAGE_POINTS, UVD_STAGE_U_RAW, UVD_STAGE_AREAS, UVD_STAGE_FOUND, UVD_STAGE_MERGED, UVD_STAGE_KEPT = 1, 2, 3, 4, 5, 7, 8, 9, 10


class UVDisparity:
    """ssm_uvd: UVDisparity::Process (src/uvdisparity.cpp:842-903) -- the moving-object, ROI and ground masks and the pitch of stereo frames from the left
    image, the SGBM disparity (x16) and the quad matches with their VO inlier flags.  UVDisparity(ctx) runs the per-pixel stages on the device;
    UVDisparity(None) is a host-only object whose process_host needs no GPU.  Keyword arguments are fields of ssm_uvd_params (SetCalibPars, SetROI3D,
    SetUSegmentPars, SetInlierTolerance).  matches / inlier_flags come back edited the way filterInOut edits the VO's lists: flag bit 1 (value 2) = erased."""

    def __init__(self, ctx=None, record=False, **kw):
        """record: keep every flood-fill mask of a frame for stage() (ssm_debug_uvd_record; the tests)"""
        self.ctx = ctx; self.lib = ctx.lib if ctx is not None else _lib.load()
        p = UvdParams()
        self.lib.ssm_uvd_params_default(C.byref(p))
        for k, v in kw.items():
            if not hasattr(p, k):
                raise KeyError(k)
            setattr(p, k, v)
        self.params = p
        h = C.c_void_p()
        rc = self.lib.ssm_uvd_create(ctx.h if ctx is not None else None, C.byref(p), C.byref(h))
        if rc != 0:
            raise SsmError(rc, (self.lib.ssm_last_error(ctx.h if ctx is not None else None) or b"").decode())
        self.h = h
        if record:
            self.lib.ssm_debug_uvd_record(self.h, 1)

    def _chk(self, rc):
        if rc != 0:
            raise SsmError(rc, (self.lib.ssm_last_error(self.ctx.h) or b"").decode() if self.ctx is not None else "ssm_uvd")

    def reset(self):
        self._chk(self.lib.ssm_uvd_reset(self.h))

    def _one(self, fn, left, disp, matches, inlier_flags, skip):
        left = np.asarray(left, np.uint8); disp = np.asarray(disp, np.int16)
        if left.strides[1] != 1 or disp.strides[1] != 2 or disp.strides[0] != 2 * left.strides[0]:
            left = np.ascontiguousarray(left); disp = np.ascontiguousarray(disp)
        h, w = left.shape
        assert disp.shape == (h, w)
        m = np.ascontiguousarray(matches if matches is not None else np.zeros(0, PMATCH_DTYPE), PMATCH_DTYPE).copy()
        fl = np.ascontiguousarray(inlier_flags if inlier_flags is not None else np.zeros(0, np.uint8), np.uint8).copy()
        assert len(m) == len(fl)
        out = {k: np.zeros((h, w), np.uint8) for k in ("moving", "roi", "ground")}
        info = np.zeros(1, UVD_INFO_DTYPE)
        self._chk(fn(self.h, _ptr(left), _ptr(disp), w, h, left.strides[0], _ptr(m) if len(m) else None, _ptr(fl) if len(fl) else None, -1 if skip else len(m),
                     _ptr(out["moving"]), _ptr(out["roi"]), _ptr(out["ground"]), _ptr(info)))
        out.update(info=info[0], matches=m, inlier_flags=fl)
        return out

    def process(self, left, disp, matches=None, inlier_flags=None, skip=False):
        """one pair through the device path -> dict(moving, roi, ground, info, matches, inlier_flags).  left / disp may be views with a common row stride"""
        return self._one(self.lib.ssm_uvd_process, left, disp, matches, inlier_flags, skip)

    def process_host(self, left, disp, matches=None, inlier_flags=None, skip=False):
        """the same on the CPU (no GPU needed): the same bits"""
        return self._one(self.lib.ssm_uvd_process_host, left, disp, matches, inlier_flags, skip)

    def process_dev(self, left_dev, disp_dev, n, w, h, matches, nmatch, inlier_flags, moving_dev=None, roi_dev=None, ground_dev=None):
        """n device frames (packed); matches (n x cap), nmatch (n; < 0 skips the frame) and inlier_flags (n x cap) are host arrays -> (info, matches, inlier_flags)"""
        m = np.ascontiguousarray(matches, PMATCH_DTYPE).reshape(n, -1).copy(); fl = np.ascontiguousarray(inlier_flags, np.uint8).reshape(n, -1).copy()
        nm = np.ascontiguousarray(nmatch, np.int32)
        cap = m.shape[1]
        assert fl.shape == m.shape and len(nm) == n
        info = np.zeros(max(n, 1), UVD_INFO_DTYPE)
        self._chk(self.lib.ssm_uvd_process_dev(self.h, left_dev, disp_dev, n, w, h, _ptr(m) if cap else None, _ptr(nm), _ptr(fl) if cap else None, cap, moving_dev, roi_dev, ground_dev, _ptr(info)))
        return info[:n], m, fl

    def images(self, frame, w, h):
        """the intermediate images of a frame of the last call: v_dis and bin (h x 256), u_dis and union (256 x w; u_rows rows used)"""
        out = dict(v_dis=np.zeros((h, 256), np.uint8), u_dis=np.zeros((256, w), np.uint8), bin=np.zeros((h, 256), np.uint8), union=np.zeros((256, w), np.uint8))
        self._chk(self.lib.ssm_debug_uvd_images(self.h, frame, _ptr(out["v_dis"]), _ptr(out["u_dis"]), _ptr(out["bin"]), _ptr(out["union"])))
        return out

    def stage(self, frame, stage):
        """one recorded stage of a frame of the last call as bytes (UVD_STAGE_*; the point list and the areas are int32)"""
        n = C.c_size_t(0)
        self._chk(self.lib.ssm_debug_uvd_stage(self.h, frame, stage, None, 0, C.byref(n)))
        buf = np.zeros(max(n.value, 1), np.uint8)
        self._chk(self.lib.ssm_debug_uvd_stage(self.h, frame, stage, _ptr(buf), n.value, C.byref(n)))
        buf = buf[:n.value]
        return buf.view(np.int32) if stage in (UVD_STAGE_POINTS, UVD_STAGE_AREAS) else buf

    def times(self):
        """host wall time of the last device call in ms: (host step 1, host step 2, the whole call)"""
        t = (C.c_double * 3)()
        self._chk(self.lib.ssm_debug_uvd_times(self.h, C.byref(t)))
        return tuple(float(x) for x in t)

    def close(self):
        """before the context's close(), like a Looper"""
        if getattr(self, "h", None):
            if self.ctx is None or self.ctx.h:
                self.lib.ssm_uvd_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One ssm_ctx: device workspace + stream on one GPU."""

    def __init__(self, device=0, cfg=None, **kw):
        self.lib = _lib.load()
        pattern = kw.pop("brief_pattern", None)             # a 256 x 4 int8 table (x0, y0, x1, y1): copied by ssm_create, kept alive until then
        self.cfg = cfg if cfg is not None else default_config(**kw)
        self._pattern_keep = None
        if pattern is not None:
            self._pattern_keep = np.ascontiguousarray(pattern, np.int8).reshape(1024)
            self.cfg.brief_pattern = self._pattern_keep.ctypes.data
        self._inflight = []                 # output buffers of asynchronous calls that have not been waited for
        h = C.c_void_p()
        rc = self.lib.ssm_create(device, C.byref(self.cfg), C.byref(h))
        if rc != 0:
            raise SsmError(rc, (self.lib.ssm_last_error(None) or b"").decode())
        self.h = h
        self.cap = self.lib.ssm_orb_capacity(self.h)
        self.W, self.H = self.cfg.width, self.cfg.height
        self.R = max(1, self.cfg.tracker_ref_frames)

    def close(self):
        if getattr(self, "h", None):
            self.lib.ssm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise SsmError(rc, (self.lib.ssm_last_error(self.h) or b"").decode())

    # ---- OrbFeature
    def detect_features(self, img, depth=None):
        img = np.ascontiguousarray(img, np.uint8)
        ch = 1 if img.ndim == 2 else img.shape[2]
        h, w = img.shape[:2]
        if depth is not None:
            depth = np.ascontiguousarray(depth, np.uint16)
        kps = np.zeros(self.cap, KEYPOINT_DTYPE)
        desc = np.zeros((self.cap, 32), np.uint8)
        pos = np.zeros((self.cap, 3), np.float32)
        n = C.c_int(0)
        self._chk(self.lib.ssm_orb_extract(self.h, _ptr(img), w, h, img.strides[0], ch, _ptr(depth), _ptr(kps), _ptr(desc),
                                           _ptr(pos), self.cap, C.byref(n)))
        return kps[:n.value], desc[:n.value], pos[:n.value]

    # ---- asynchronous per-frame calls: results are in the returned holders after wait()
    def detect_features_async(self, img, depth=None):
        """ssm_orb_extract_async: returns a holder h; after ctx.wait(), h() gives (keypoints, descriptors, positions)"""
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape[:2]; ch = 1 if img.ndim == 2 else img.shape[2]
        depth = None if depth is None else np.ascontiguousarray(depth, np.uint16)
        kps = np.zeros(self.cap, KEYPOINT_DTYPE); desc = np.zeros((self.cap, 32), np.uint8); pos = np.zeros((self.cap, 3), np.float32)
        n = C.c_int(-1)
        self._inflight.append((kps, desc, pos, n))      # the C finisher writes into these at the next wait (explicit, or implied by a full ring / ssm_sync): they must outlive the holder
        self._chk(self.lib.ssm_orb_extract_async(self.h, _ptr(img), w, h, img.strides[0], ch, _ptr(depth), _ptr(kps), _ptr(desc), _ptr(pos), self.cap, C.byref(n)))
        return lambda: (kps[:n.value], desc[:n.value], pos[:n.value])

    def match_async(self, q, t, ratio=None):
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32); t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        out = np.zeros(max(len(q), 1), DMATCH_DTYPE); n = C.c_int(-1)
        r = self.cfg.knn_match_ratio if ratio is None else ratio
        self._inflight.append((out, n))
        self._chk(self.lib.ssm_match_async(self.h, _ptr(q), len(q), _ptr(t), len(t), r, _ptr(out), len(out), C.byref(n)))
        return lambda: out[:n.value]

    def match_refs(self, refs, cur, ratio=None):
        """ssm_match_refs: [match(r, cur) for r in refs] in one launch"""
        refs = [np.ascontiguousarray(r, np.uint8).reshape(-1, 32) for r in refs]; cur = np.ascontiguousarray(cur, np.uint8).reshape(-1, 32)
        k = len(refs)
        outs = [np.zeros(max(len(r), 1), DMATCH_DTYPE) for r in refs]
        pr = (C.c_void_p * max(k, 1))(*[r.ctypes.data for r in refs]); po = (C.c_void_p * max(k, 1))(*[o.ctypes.data for o in outs])
        nr = (C.c_int * max(k, 1))(*[len(r) for r in refs]); caps = (C.c_int * max(k, 1))(*[len(o) for o in outs]); n = (C.c_int * max(k, 1))()
        self._chk(self.lib.ssm_match_refs(self.h, pr, nr, k, _ptr(cur), len(cur), self.cfg.knn_match_ratio if ratio is None else ratio, po, caps, n))
        return [o[:n[i]] for i, o in enumerate(outs)]

    def wait(self):
        try:
            self._chk(self.lib.ssm_wait(self.h))
        finally:
            self._inflight.clear()

    def knn2(self, q, t):
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        idx = np.zeros((len(q), 2), np.int32)
        dist = np.zeros((len(q), 2), np.int32)
        self._chk(self.lib.ssm_hamming_knn2(self.h, _ptr(q), len(q), _ptr(t), len(t), _ptr(idx), _ptr(dist)))
        return idx, dist

    def match(self, q, t, ratio=None):
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        out = np.zeros(max(len(q), 1), DMATCH_DTYPE)
        n = C.c_int(0)
        r = self.cfg.knn_match_ratio if ratio is None else ratio
        self._chk(self.lib.ssm_match(self.h, _ptr(q), len(q), _ptr(t), len(t), r, _ptr(out), len(out), C.byref(n)))
        return out[:n.value]

    # ---- QuadFeatureMatch (stereo)
    def quad_track(self, lc, rc, lp, rp, max_corners=1000):
        ims = [np.ascontiguousarray(a, np.uint8) for a in (lc, rc, lp, rp)]
        h, w = ims[0].shape
        out = np.zeros(max_corners, PMATCH_DTYPE); n = C.c_int(0)
        self._chk(self.lib.ssm_quad_track(self.h, _ptr(ims[0]), _ptr(ims[1]), _ptr(ims[2]), _ptr(ims[3]), w, h, w, max_corners, _ptr(out), len(out), C.byref(n)))
        return out[:n.value]

    # ---- device-resident batched stereo path (configs[3])
    def stereo_batch(self):
        return self.lib.ssm_stereo_batch(self.h)

    def stereo_seq_process(self, left_dev, right_dev, n, w, h, continue_sequence=False, stages=0, max_corners=1000, sgbm=None,
                           baseline=0.0, cu=0.0, cv=0.0, f=1.0, roix=0.0, roiy=0.0, roiz=0.0, scale=1.0,
                           vo=None, ransac_iters=200, rand_stream_dev=None):
        """ssm_stereo_seq_process on n device frame pairs: quad matcher (frame f against f - 1), SGBM depth, stereo VO.  vo = (f, cu, cv, base,
        inlier_threshold, reweighting); rand_stream_dev = device pointer to n * ransac_iters * 3 raw rand() draws (GlibcRand.draws)."""
        fr = StereoFramesDev()
        fr.left, fr.right, fr.n, fr.w, fr.h = left_dev, right_dev, n, w, h
        fr.continue_sequence, fr.stages, fr.max_corners = int(continue_sequence), stages, max_corners
        sp = self.sgbm_params() if sgbm is None else np.ascontiguousarray(sgbm, np.int32)
        fr.sgbm = SgbmParams(*[int(v) for v in sp])
        fr.baseline, fr.cu, fr.cv, fr.f, fr.roix, fr.roiy, fr.roiz, fr.scale = baseline, cu, cv, f, roix, roiy, roiz, scale
        if vo is not None:
            fr.vo = VoParams(vo[0], vo[1], vo[2], vo[3], vo[4], int(vo[5]), 0)
        fr.ransac_iters = ransac_iters
        fr.rand_stream = rand_stream_dev
        out = StereoOutDev()
        self._chk(self.lib.ssm_stereo_seq_process(self.h, C.byref(fr), C.byref(out)))
        return out

    def stereo_seq_fetch(self, out, n, w, h, stages=7):
        """Copy the outputs of stereo_seq_process back to the host (test helper)."""
        mc = out.max_corners
        res = {}
        if stages & STEREO_QUAD:
            res["nquad"] = self.d2h(out.nquad, n, np.int32); res["quad"] = self.d2h(out.quad, (n, mc), PMATCH_DTYPE)
            res["ncorners"] = self.d2h(out.ncorners, n, np.int32); res["corners"] = self.d2h(out.corners, (n, mc, 2), np.float32)
        if stages & STEREO_DEPTH:
            res["disp"] = self.d2h(out.disp, (n, h, w), np.int16); res["depth"] = self.d2h(out.depth, (n, h, w), np.uint16)
        if stages & STEREO_VO:
            res["tr"] = self.d2h(out.tr, (n, 6), np.float64); res["inliers"] = self.d2h(out.inliers, (n, mc), np.int32)
            res["vo_result"] = self.d2h(out.vo_result, (n, 2), np.int32); res["rand_draws_used"] = int(self.d2h(out.rand_draws_used, 1, np.int32)[0])
        return res

    @staticmethod
    def sgbm_params(**kw):
        """cv::StereoSGBM fields as src/stereo.cpp:11-30 sets them; override by keyword"""
        d = dict(minDisparity=0, numberOfDisparities=80, SADWindowSize=11, P1=None, P2=None, disp12MaxDiff=1, preFilterCap=63, uniquenessRatio=10,
                 speckleWindowSize=100, speckleRange=32)
        d.update(kw)
        if d["P1"] is None: d["P1"] = 4 * d["SADWindowSize"] ** 2
        if d["P2"] is None: d["P2"] = 32 * d["SADWindowSize"] ** 2
        return np.array([d[k] for k in ("minDisparity", "numberOfDisparities", "SADWindowSize", "P1", "P2", "disp12MaxDiff", "preFilterCap", "uniquenessRatio",
                                        "speckleWindowSize", "speckleRange")], np.int32)

    def sgbm(self, left, right, params=None, raw=False):
        """cv::StereoSGBM::operator(): int16 disparity x16 ((minDisparity-1)*16 = invalid); raw=True stops before medianBlur / filterSpeckles"""
        left = np.ascontiguousarray(left, np.uint8); right = np.ascontiguousarray(right, np.uint8); h, w = left.shape
        params = self.sgbm_params() if params is None else np.ascontiguousarray(params, np.int32)
        disp = np.zeros((h, w), np.int16)
        self._chk(self.lib.ssm_sgbm(self.h, _ptr(left), _ptr(right), w, h, left.strides[0], _ptr(params), int(raw), _ptr(disp)))
        return disp

    def stereo_depth(self, left, right, baseline, cu, cv, f, roix, roiy, roiz, scale, params=None):
        """FrameReader's KITTI depth step (src/rgbdframe.cpp:81-116): (depth u16, disparity int16)"""
        left = np.ascontiguousarray(left, np.uint8); right = np.ascontiguousarray(right, np.uint8); h, w = left.shape
        params = self.sgbm_params() if params is None else np.ascontiguousarray(params, np.int32)
        depth = np.zeros((h, w), np.uint16); disp = np.zeros((h, w), np.int16)
        self._chk(self.lib.ssm_stereo_depth(self.h, _ptr(left), _ptr(right), w, h, left.strides[0], _ptr(params), baseline, cu, cv, f, roix, roiy, roiz, scale,
                                            _ptr(depth), _ptr(disp)))
        return depth, disp

    def vo_estimate(self, matches, f, cu, cv, base, samples, inlier_threshold=2.0, reweighting=True):
        """VisualOdometryStereo::estimateMotion on quad matches: (success, tr[6], inlier indices)"""
        m = np.ascontiguousarray(matches, PMATCH_DTYPE); samples = np.ascontiguousarray(samples, np.int32).reshape(-1, 3)
        prm = np.array([(f, cu, cv, base, inlier_threshold, int(reweighting), 0)], VO_PARAMS_DTYPE)
        tr = np.zeros(6, np.float64); inl = np.zeros(max(len(m), 1), np.int32); n = C.c_int(0); ok = C.c_int(0)
        self._chk(self.lib.ssm_vo_estimate(self.h, _ptr(m), len(m), _ptr(prm), _ptr(samples), len(samples), _ptr(tr), _ptr(inl), len(inl), C.byref(n), C.byref(ok)))
        return bool(ok.value), tr, inl[:n.value].copy()

    def pnp_solve(self, img, obj, cam, T0, min_inliers=10):
        """PnPSolver::solvePnP (src/pnp.cpp:5-118) on the device: img n x 2 pixels in frame 2, obj n x 3 points in frame 1's camera frame, cam = (fx, fy, cx, cy),
        T0 = 4 x 4 initial transform.  Returns (success, T 4 x 4, inlier flags uint8[n] as pnp.cpp keeps them, number of set flags)."""
        img = np.ascontiguousarray(img, np.float32).reshape(-1, 2); obj = np.ascontiguousarray(obj, np.float32).reshape(-1, 3)
        assert len(img) == len(obj)
        camv = np.ascontiguousarray(cam, np.float64).reshape(4)
        T = np.ascontiguousarray(np.asarray(T0, np.float64).reshape(4, 4).T).copy()          # column-major
        inl = np.zeros(max(len(img), 1), np.uint8); n = C.c_int(0); ok = C.c_int(0)
        self._chk(self.lib.ssm_pnp_solve(self.h, _ptr(img), _ptr(obj), len(img), _ptr(camv), int(min_inliers), _ptr(T), _ptr(inl), C.byref(n), C.byref(ok)))
        return bool(ok.value), T.T.copy(), inl[:len(img)].copy(), n.value

    def pnp_solve_blocks(self):
        """8 or 1: the blocks the next pnp_solve starts with (ssm_debug_pnp_solve_blocks; 1 once a cluster of eight has timed out on this context)"""
        return self.lib.ssm_debug_pnp_solve_blocks(self.h)

    def gftt(self, img, max_corners=1000, quality=0.04, min_distance=8.0):
        img = np.ascontiguousarray(img, np.uint8); h, w = img.shape
        pts = np.zeros((max_corners, 2), np.float32); n = C.c_int(0)
        self._chk(self.lib.ssm_gftt(self.h, _ptr(img), w, h, img.strides[0], max_corners, quality, min_distance, _ptr(pts), max_corners, C.byref(n)))
        return pts[:n.value]

    def lk_track(self, prev, nxt, pts, max_count=200, epsilon=0.01, min_eig=1e-6):
        prev, nxt = _rows(prev), _rows(nxt); h, w = prev.shape
        if nxt.shape != prev.shape:
            raise ValueError("lk_track: the two images differ in size")
        if nxt.strides[0] != prev.strides[0]:                       # (the ABI takes one row stride for both images)
            prev = np.ascontiguousarray(prev); nxt = np.ascontiguousarray(nxt)
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        out = np.zeros_like(pts); st = np.zeros(len(pts), np.uint8); err = np.zeros(len(pts), np.float32)
        self._chk(self.lib.ssm_lk_track(self.h, _ptr(prev), _ptr(nxt), w, h, prev.strides[0], _ptr(pts), len(pts), _ptr(out), _ptr(st), _ptr(err), max_count, epsilon, min_eig))
        return out, st, err

    def debug_quad_pyramid(self, side, level):
        """level 0 .. 3 of the LK pyramid of the last lk_track (side 0 = previous image, 1 = next) and its Scharr (dx, dy) pairs: (uint8 h x w, int16 h x w x 2)"""
        w = C.c_int(0); h = C.c_int(0)
        self._chk(self.lib.ssm_debug_quad_pyramid(self.h, side, level, None, None, C.byref(w), C.byref(h)))
        img = np.zeros((h.value, w.value), np.uint8); der = np.zeros((h.value, w.value, 2), np.int16)
        self._chk(self.lib.ssm_debug_quad_pyramid(self.h, side, level, _ptr(img), _ptr(der), C.byref(w), C.byref(h)))
        return img, der

    def _debug_frames(self, img):
        img = np.ascontiguousarray(img, np.uint8)
        if img.ndim not in (3, 4) or img.shape[1:3] != (self.H, self.W) or (img.ndim == 4 and img.shape[3] != 3):
            raise ValueError("frames must be (n, H, W) gray or (n, H, W, 3) BGR of the context's size")
        return img, (1 if img.ndim == 3 else 3)

    def debug_pyramid(self, img, bands=0):
        """ssm_debug_pyramid: the pyramid buffers (n, bytes) of n frames, (n, H, W) gray or (n, H, W, 3) BGR"""
        img, ch = self._debug_frames(img)
        nbytes = C.c_int(0)
        self._chk(self.lib.ssm_debug_pyramid(self.h, None, ch, len(img), bands, None, C.byref(nbytes)))
        out = np.zeros((len(img), nbytes.value), np.uint8)
        self._chk(self.lib.ssm_debug_pyramid(self.h, _ptr(img), ch, len(img), bands, _ptr(out), C.byref(nbytes)))
        return out

    def debug_orb_blur(self, img):
        """ssm_debug_orb_blur: the blurred pyramids (n, bytes) of n frames, un-tiled into debug_pyramid's layout"""
        img, ch = self._debug_frames(img)
        nbytes = C.c_int(0)
        self._chk(self.lib.ssm_debug_orb_blur(self.h, None, ch, len(img), None, C.byref(nbytes)))
        out = np.zeros((len(img), nbytes.value), np.uint8)
        self._chk(self.lib.ssm_debug_orb_blur(self.h, _ptr(img), ch, len(img), _ptr(out), C.byref(nbytes)))
        return out

    def debug_orb_describe(self, img, nsel, sel, depth=None, moments=None):
        """ssm_debug_orb_describe: the describe stage on planted keypoints.  nsel (n, levels) counts; sel: the packed words x | y << 12 | score << 24 of all
        frames, frame by frame and level by level; depth (n, H, W) uint16 or None; moments (len(sel), 2) planted (m10, m01) or None.  Returns a dict of
        whole (n, capacity, ...) arrays: nkp, kps, desc, pos3d, moments (m10, m01), sincos (sin, cos); records from nkp[f] on hold the bytes 0xA5"""
        img, ch = self._debug_frames(img)
        n = len(img)
        nsel = np.ascontiguousarray(nsel, np.int32); sel = np.ascontiguousarray(sel, np.uint32).reshape(-1)
        if nsel.shape != (n, self.cfg.orb_levels) or (nsel >= 0).all() and int(nsel.sum()) != len(sel):
            raise ValueError("nsel must be (n, levels) and sum to len(sel)")
        if depth is not None:
            depth = np.ascontiguousarray(depth, np.uint16)
            if depth.shape != (n, self.H, self.W):
                raise ValueError("depth must be (n, H, W)")
        if moments is not None:
            moments = np.ascontiguousarray(moments, np.int32)
            if moments.shape != (len(sel), 2):
                raise ValueError("moments must be (len(sel), 2)")
        m = max(n, 1)
        out = {"nkp": np.zeros(m, np.int32), "kps": np.zeros((m, self.cap), KEYPOINT_DTYPE), "desc": np.zeros((m, self.cap, 32), np.uint8),
               "pos3d": np.zeros((m, self.cap, 3), np.float32), "moments": np.zeros((m, self.cap, 2), np.int32), "sincos": np.zeros((m, self.cap, 2), np.float32)}
        self._chk(self.lib.ssm_debug_orb_describe(self.h, _ptr(img), ch, n, _ptr(depth), _ptr(nsel), _ptr(sel), _ptr(moments), _ptr(out["nkp"]), _ptr(out["kps"]),
                                                  _ptr(out["desc"]), _ptr(out["pos3d"]), _ptr(out["moments"]), _ptr(out["sincos"])))
        return out

    OCTREE_GEOM_FIELDS = ("w", "h", "minB", "nCols", "nRows", "wCell", "hCell", "nfeat", "nIni", "cand_cap", "sel_cap")

    def debug_orb_octree_geometry(self):
        """ssm_debug_orb_octree's geometry query: {"levels": [per level a dict of OCTREE_GEOM_FIELDS], "cells_total", "cand_total", "sel_total", "nodes"}"""
        nl, k = self.cfg.orb_levels, len(self.OCTREE_GEOM_FIELDS)
        g = np.zeros(nl * k + 4, np.int32)
        self._chk(self.lib.ssm_debug_orb_octree(self.h, 0, None, None, None, _ptr(g), None, None, None, None))
        out = {"levels": [dict(zip(self.OCTREE_GEOM_FIELDS, (int(v) for v in g[l * k:(l + 1) * k]))) for l in range(nl)]}
        out.update(zip(("cells_total", "cand_total", "sel_total", "nodes"), (int(v) for v in g[nl * k:])))
        return out

    def debug_orb_octree(self, ncand, cand, cellmax, want_nodeof=False):
        """ssm_debug_orb_octree: the quad-tree selection alone on planted candidates.  ncand (n, levels) counts; cand (sum(ncand), 2) uint32 words
        (x | y << 12 | score << 24, cell << 14 | yInCell << 7 | xInCell) of all frames, frame by frame and level by level, in buffer order; cellmax
        (n, cells_total).  Returns (nsel (n, levels), sel (n, sel_total) -- slots that were not written hold 0xA5A5A5A5 --, status), and with want_nodeof
        a fourth element: the global node-id scratch (n, cand_total) uint16 after the launch, 0xA5A5 where the kernel did not write"""
        geo = self.debug_orb_octree_geometry()
        ncand = np.ascontiguousarray(ncand, np.int32); cand = np.ascontiguousarray(cand, np.uint32).reshape(-1, 2); cellmax = np.ascontiguousarray(cellmax, np.int32)
        n = len(ncand)
        if ncand.ndim != 2 or ncand.shape[1] != self.cfg.orb_levels or cellmax.shape != (n, geo["cells_total"]) or (ncand >= 0).all() and int(ncand.sum()) != len(cand):
            raise ValueError("ncand must be (n, levels) and sum to len(cand); cellmax (n, cells_total)")
        m = max(n, 1)
        nsel = np.zeros((m, self.cfg.orb_levels), np.int32); sel = np.zeros((m, geo["sel_total"]), np.uint32); status = np.zeros(1, np.int32)
        nodeof = np.zeros((m, geo["cand_total"]), np.uint16) if want_nodeof else None
        self._chk(self.lib.ssm_debug_orb_octree(self.h, n, _ptr(ncand), _ptr(cand), _ptr(cellmax), None, _ptr(nsel), _ptr(sel), _ptr(status), _ptr(nodeof)))
        return (nsel, sel, int(status[0]), nodeof) if want_nodeof else (nsel, sel, int(status[0]))

    def window_match(self, kp1, d1, kp2, d2, sw, sh, thr):
        kp1 = np.ascontiguousarray(kp1, np.float32).reshape(-1, 2); kp2 = np.ascontiguousarray(kp2, np.float32).reshape(-1, 2)
        d1 = np.ascontiguousarray(d1, np.uint8).reshape(-1, 32); d2 = np.ascontiguousarray(d2, np.uint8).reshape(-1, 32)
        out = np.zeros(max(len(kp1), 1), DMATCH_DTYPE)
        self._chk(self.lib.ssm_window_match(self.h, _ptr(kp1), _ptr(d1), len(kp1), _ptr(kp2), _ptr(d2), len(kp2), sw, sh, thr, _ptr(out)))
        return out[:len(kp1)]

    # ---- Classifier (SegNet)
    def segnet_layers(self):
        out = []
        for l in range(self.lib.ssm_segnet_num_layers()):
            a, b, h, w = C.c_int(), C.c_int(), C.c_int(), C.c_int()
            self.lib.ssm_segnet_layer_shape(l, C.byref(a), C.byref(b), C.byref(h), C.byref(w))
            out.append((a.value, b.value, h.value, w.value))
        return out

    def segnet_set_layer(self, layer, weight, scale, shift):
        w = np.ascontiguousarray(weight, np.float32); sc = np.ascontiguousarray(scale, np.float32); sh = np.ascontiguousarray(shift, np.float32)
        self._chk(self.lib.ssm_segnet_set_layer(self.h, layer, _ptr(w), _ptr(sc), _ptr(sh)))

    def classify(self, bgr, want_sem=True):
        """Classifier::Classify: returns (labels 360x480 u8, colour-label image at frame size or None)"""
        bgr = np.ascontiguousarray(bgr, np.uint8)
        h, w = bgr.shape[:2]
        labels = np.zeros((SEG_NET_H, SEG_NET_W), np.uint8)
        sem = np.zeros((h, w, 3), np.uint8) if want_sem else None
        self._chk(self.lib.ssm_segnet_forward(self.h, _ptr(bgr), w, h, bgr.strides[0], _ptr(labels), _ptr(sem)))
        return labels, sem

    def segnet_logits(self):
        out = np.zeros((SEG_NET_H, SEG_NET_W, SEG_CLASSES), np.float32)
        self._chk(self.lib.ssm_segnet_logits(self.h, _ptr(out)))
        return out

    def segnet_debug_conv(self, layer, x_hwc_f16):
        cin, cout, _, _ = self.segnet_layers()[layer]
        x = np.ascontiguousarray(x_hwc_f16, np.float16); h, w, c = x.shape
        assert c == (cin + 15) // 16 * 16
        out = np.zeros((h, w, (cout + 15) // 16 * 16), np.float16)
        self._chk(self.lib.ssm_segnet_debug_op(self.h, 0, layer, _ptr(x), h, w, _ptr(out), None))
        return out[:, :, :cout]

    def segnet_debug_conv_pool(self, layer, x_hwc_f16):
        """conv + BN + ReLU + 2x2 max-pool of `layer` through the fused kernel the network uses: (pooled, codes)."""
        cin, cout, _, _ = self.segnet_layers()[layer]
        x = np.ascontiguousarray(x_hwc_f16, np.float16); h, w, c = x.shape
        ci16, co16 = (cin + 15) & ~15, (cout + 15) & ~15
        xin = np.zeros((h, w, ci16), np.float16); xin[:, :, :c] = x
        out = np.zeros(((h + 1) // 2, (w + 1) // 2, co16), np.float16); code = np.zeros(out.shape, np.uint8)
        self._chk(self.lib.ssm_segnet_debug_op(self.h, 3, layer, _ptr(xin), h, w, _ptr(out), _ptr(code)))
        return out[:, :, :cout], code[:, :, :cout]

    def segnet_debug_unpool_conv(self, layer, pooled_hwc_f16, code, h, w):
        """un-pool (to h x w) + conv + BN + ReLU of `layer` through the fused kernel the network uses."""
        cin, cout, _, _ = self.segnet_layers()[layer]
        x = np.ascontiguousarray(pooled_hwc_f16, np.float16); ph, pw, c = x.shape
        ci16, co16 = (cin + 15) & ~15, (cout + 15) & ~15
        xin = np.zeros((ph, pw, ci16), np.float16); xin[:, :, :c] = x
        cin_code = np.zeros((ph, pw, ci16), np.uint8); cin_code[:, :, :c] = code
        out = np.zeros((h, w, co16), np.float16)
        self._chk(self.lib.ssm_segnet_debug_op(self.h, 4, layer, _ptr(xin), h, w, _ptr(out), _ptr(cin_code)))
        return out[:, :, :cout]

    def segnet_debug_conv_argmax(self, layer, x_hwc_f16):
        """conv + scale / shift of the last layer with the class ArgMax in its epilogue (the kernel ssm_segnet_forward_dev's labels come from): labels [h][w]"""
        cin, cout, _, _ = self.segnet_layers()[layer]
        x = np.ascontiguousarray(x_hwc_f16, np.float16); h, w, c = x.shape
        xin = np.zeros((h, w, (cin + 15) & ~15), np.float16); xin[:, :, :c] = x
        labels = np.full((h, w), 255, np.uint8); dummy = np.zeros(1, np.float16)
        self._chk(self.lib.ssm_segnet_debug_op(self.h, 5, layer, _ptr(xin), h, w, _ptr(dummy), _ptr(labels)))
        return labels

    def debug_sgbm_post(self, disp, op, new_val=-16, max_size=100, max_diff=32):
        """int16 maps (h x w, or n x h x w: one launch over all n) through SGBM's last steps: op bit 0 = medianBlur 3x3, bit 1 = filterSpeckles"""
        d = np.ascontiguousarray(disp, np.int16); d3 = d.reshape((-1,) + d.shape[-2:]); n, h, w = d3.shape
        out = np.empty_like(d3)
        self._chk(self.lib.ssm_debug_sgbm_post(self.h, _ptr(d3), w, h, n, op, new_val, max_size, max_diff, _ptr(out)))
        return out.reshape(d.shape)

    def segnet_debug_pool(self, x_hwc_f16):
        x = np.ascontiguousarray(x_hwc_f16, np.float16); h, w, c = x.shape
        out = np.zeros(((h + 1) // 2, (w + 1) // 2, c), np.float16); code = np.zeros(out.shape, np.uint8)
        self._chk(self.lib.ssm_segnet_debug_op(self.h, 1, c, _ptr(x), h, w, _ptr(out), _ptr(code)))
        return out, code

    def segnet_debug_unpool(self, x_hwc_f16, code, h, w):
        x = np.ascontiguousarray(x_hwc_f16, np.float16); code = np.ascontiguousarray(code, np.uint8); c = x.shape[2]
        out = np.zeros((h, w, c), np.float16)
        self._chk(self.lib.ssm_segnet_debug_op(self.h, 2, c, _ptr(x), h, w, _ptr(out), _ptr(code)))
        return out

    def segnet_forward_dev(self, bgr_dev, n, labels_dev=None, sem_dev=None, flags=0):
        self._chk(self.lib.ssm_segnet_forward_dev(self.h, bgr_dev, n, labels_dev, sem_dev, flags))

    # ---- Mapper
    def moving_mask(self, sem):
        sem = np.ascontiguousarray(sem, np.uint8)
        h, w = sem.shape[:2]
        mask = np.zeros((h, w), np.uint8)
        self._chk(self.lib.ssm_moving_mask(self.h, _ptr(sem), w, h, sem.strides[0], _ptr(mask)))
        return mask

    def motion_fuse(self, sem, motion=None, area_thres=1000, overlay_thres=0.143, record=False):
        """the semantic-motion fusion on the device.  sem H x W x 3 (host-image call) or n x H x W x 3 (the batched device-resident call, through temporary device
        buffers): -> (mask, info), info a dict or a MOTION_FUSE_INFO_DTYPE array of n; record adds {labels, area, overlap, cand} (a list of n for a batch)"""
        sem, motion = _mf_images(sem, motion)
        P = MotionFuseParams(int(area_thres), 0, float(overlay_thres))
        h, w = sem.shape[-3:-1]

        def recorded(f):
            rec = {k: np.zeros((h, w), np.int32) for k in ("labels", "area", "overlap")}
            rec["cand"] = np.zeros((h, w), np.uint8)
            self._chk(self.lib.ssm_debug_motion_fuse(self.h, f, _ptr(rec["labels"]), _ptr(rec["area"]), _ptr(rec["overlap"]), _ptr(rec["cand"])))
            return rec
        if sem.ndim == 3:
            mask = np.zeros((h, w), np.uint8); I = MotionFuseInfo()
            self._chk(self.lib.ssm_motion_fuse(self.h, _ptr(sem), _ptr(motion), w, h, w * 3, C.byref(P), _ptr(mask), C.byref(I)))
            info = {k: getattr(I, k) for k in MOTION_FUSE_INFO_DTYPE.names}
            return (mask, info, recorded(0)) if record else (mask, info)
        n = sem.shape[0]
        info = np.zeros(n, MOTION_FUSE_INFO_DTYPE)
        bufs = [self.dev_alloc(sem.nbytes), self.dev_alloc(n * w * h), self.dev_alloc(n * w * h) if motion is not None else None]
        try:
            self.h2d(bufs[0], sem)
            if motion is not None:
                self.h2d(bufs[2], motion)
            self._chk(self.lib.ssm_motion_fuse_dev(self.h, bufs[0], bufs[2], n, w, h, C.byref(P), bufs[1], _ptr(info)))
            mask = self.d2h(bufs[1], (n, h, w), np.uint8)
            rec = [recorded(f) for f in range(n)] if record else None
        finally:
            for b in bufs:
                if b is not None:
                    self.dev_free(b)
        return (mask, info, rec) if record else (mask, info)

    def _sor_record(self, n):
        rec = {"mean_dist": np.zeros(n, np.float32), "keep": np.zeros(n, np.uint8)}
        self._chk(self.lib.ssm_debug_sor_record(self.h, _ptr(rec["mean_dist"]), _ptr(rec["keep"]), n))
        return rec

    def sor_filter(self, points, mean_k=30, stddev_mul=1.0, cell=0.0, record=False):
        """the statistical outlier removal on the device (ssm_sor_filter): -> (points, info), or with record (points, info, {mean_dist, keep})"""
        points = _sor_points(points)
        n = len(points)
        P = SorParams(int(mean_k), float(cell), float(stddev_mul)); I = SorInfo()
        out = np.zeros(n, POINT_DTYPE); got = C.c_int(0)
        self._chk(self.lib.ssm_sor_filter(self.h, _ptr(points), n, C.byref(P), _ptr(out), n, C.byref(got), C.byref(I)))
        info = {k: getattr(I, k) for k in SOR_INFO_FIELDS}
        return (out[:got.value], info, self._sor_record(n)) if record else (out[:got.value], info)

    def sor_levels(self):
        """the ladder of the last device call: the points still unsettled when each level began (ssm_debug_sor_levels)"""
        q = np.zeros(24, np.int32); n = C.c_int(0)
        self._chk(self.lib.ssm_debug_sor_levels(self.h, _ptr(q), len(q), C.byref(n)))
        return q[:n.value].tolist()

    def cloud_sor(self, cloud, mean_k=30, stddev_mul=1.0, cell=0.0, record=False):
        """the same on a device-resident cloud (backproject_dev's handle), which shrinks in place: -> info, or with record (info, {mean_dist, keep})"""
        n = self.lib.ssm_cloud_size(cloud)
        P = SorParams(int(mean_k), float(cell), float(stddev_mul)); I = SorInfo()
        self._chk(self.lib.ssm_cloud_sor(self.h, cloud, C.byref(P), C.byref(I)))
        info = {k: getattr(I, k) for k in SOR_INFO_FIELDS}
        return (info, self._sor_record(n)) if record else info

    def carve_view(self, depth, camera=None):
        """a view of free-space carving: the depth image goes to the device and stays (ssm_carve_view_create) -> an opaque handle (carve_view_free it)"""
        depth = np.ascontiguousarray(depth, np.uint16)
        h, w = depth.shape
        cam = Camera(*camera) if camera is not None else self.cfg.camera
        v = C.c_void_p()
        self._chk(self.lib.ssm_carve_view_create(self.h, _ptr(depth), w, h, C.byref(cam), C.byref(v)))
        return v.value

    def carve_view_free(self, view):
        self.lib.ssm_carve_view_free(self.h, view)

    def _carve_record(self, k, n):
        rec = {"verdict": np.zeros(n, np.uint8), "run": np.zeros(n, np.uint8)}
        self._chk(self.lib.ssm_debug_carve_record(self.h, k, _ptr(rec["verdict"]), _ptr(rec["run"]), n))
        return rec

    def carve(self, view, T_view, clouds, T_clouds, record=False, **params):
        """one view against device-resident clouds (backproject_dev's handles), which shrink in place (ssm_carve) -> the infos, or with record (infos, [{verdict, run}])"""
        sizes = [self.cloud_size(cl) for cl in clouds]
        _, arr, _, Tc, m = _pack_clouds(clouds, T_clouds, False)
        P = _carve_params(params); infos = (CarveInfo * max(m, 1))()
        self._chk(self.lib.ssm_carve(self.h, view, _ptr(_cm16(T_view)), arr, _ptr(Tc), m, C.byref(P), infos))
        out = [_carve_info(infos[k]) for k in range(m)]
        return (out, [self._carve_record(k, sizes[k]) for k in range(m)]) if record else out

    def cloud_run(self, cloud):
        """the run counters of a device-resident cloud (ssm_cloud_run_fetch)"""
        n = self.cloud_size(cloud)
        run = np.zeros(max(n, 1), np.uint8)
        self._chk(self.lib.ssm_cloud_run_fetch(self.h, cloud, _ptr(run), len(run)))
        return run[:n]

    def carve_points(self, depth, camera, T_view, points, T_cloud, run=None, record=False, **params):
        """carve_host's call through the device (ssm_carve_points): -> (points, run, info), or with record (points, run, info, {verdict, run})"""
        depth = np.ascontiguousarray(depth, np.uint16); points = _sor_points(points)
        h, w = depth.shape
        n = len(points)
        P = _carve_params(params); I = CarveInfo(); cam = Camera(*camera)
        Tv, Tc = _cm16(T_view), _cm16(T_cloud)
        run = _carve_run(run, n)
        out = np.zeros(n, POINT_DTYPE); got = C.c_int(0)
        self._chk(self.lib.ssm_carve_points(self.h, _ptr(depth), w, h, C.byref(cam), _ptr(Tv), _ptr(points), n, _ptr(Tc), _ptr(run), C.byref(P), _ptr(out), n, C.byref(got), C.byref(I)))
        res = (out[:got.value], run[:got.value], _carve_info(I))
        return res + (self._carve_record(0, n),) if record else res

    def render_target(self, w, h):
        """the device z-buffer and images of a w x h view, reused across renderings (ssm_render_target_create) -> an opaque handle (render_target_free it)"""
        t = C.c_void_p()
        self._chk(self.lib.ssm_render_target_create(self.h, int(w), int(h), C.byref(t)))
        self._render_sizes = getattr(self, "_render_sizes", {})
        self._render_sizes[t.value] = (int(w), int(h))
        return t.value

    def render_target_free(self, target):
        self._render_sizes.pop(target, None)
        self.lib.ssm_render_target_free(self.h, target)

    def _render_result(self, target, I, keys):
        w, h = self._render_sizes[target]
        out = _render_images(w, h, keys)
        self._chk(self.lib.ssm_render_fetch(self.h, target, _ptr(out["depth"]), _ptr(out["bgr"]), _ptr(out["label"]), _ptr(out["index"])))
        if keys:
            self._chk(self.lib.ssm_debug_render_keys(self.h, target, _ptr(out["keys"])))
        out["info"] = {k: getattr(I, k) for k in RENDER_INFO_FIELDS}
        return out

    def render_points(self, target, camera, T_view, clouds, T_clouds, keys=False, **params):
        """render_host's call through the device (ssm_render_points) -> {depth, bgr, label, index, info}, with keys=True also the raw z-buffer"""
        keep, ptrs, n, Tc, m = _pack_clouds(clouds, T_clouds, True)
        P = _render_params(params); I = RenderInfo(); cam = Camera(*camera) if camera is not None else self.cfg.camera
        self._chk(self.lib.ssm_render_points(self.h, target, C.byref(cam), _ptr(_cm16(T_view)), ptrs, _ptr(n), _ptr(Tc), m, C.byref(P), C.byref(I)))
        return self._render_result(target, I, keys)

    def render_clouds(self, target, camera, T_view, clouds, T_clouds, keys=False, **params):
        """device-resident clouds (backproject_dev's handles) at the poses T_clouds into the view (ssm_render_clouds); nothing is uploaded but the poses"""
        _, arr, _, Tc, m = _pack_clouds(clouds, T_clouds, False)
        P = _render_params(params); I = RenderInfo(); cam = Camera(*camera) if camera is not None else self.cfg.camera
        self._chk(self.lib.ssm_render_clouds(self.h, target, C.byref(cam), _ptr(_cm16(T_view)), arr, _ptr(Tc), m, C.byref(P), C.byref(I)))
        return self._render_result(target, I, keys)

    def render_viewer_map(self, target, camera, T_view, keys=False, **params):
        """the map the last viewer_map_update left on the device, at the identity pose (ssm_render_viewer_map)"""
        P = _render_params(params); I = RenderInfo(); cam = Camera(*camera) if camera is not None else self.cfg.camera
        self._chk(self.lib.ssm_render_viewer_map(self.h, target, C.byref(cam), _ptr(_cm16(T_view)), C.byref(P), C.byref(I)))
        return self._render_result(target, I, keys)

    def render_compare(self, target, depth, sem, scale=None, class_image=False, **params):
        """the target's last rendering against a frame's depth and semantic BGR image, on the device (ssm_render_compare) -> the nine counts, or with class_image
        (counts, the class image)"""
        w, h = self._render_sizes[target]
        depth, sem = _compare_frame((h, w), depth, sem)
        P = _render_params(params); I = RenderCompareInfo()
        cls = np.zeros((h, w), np.uint8) if class_image else None
        self._chk(self.lib.ssm_render_compare(self.h, target, _ptr(depth), _ptr(sem), float(self.cfg.camera.scale if scale is None else scale), C.byref(P), C.byref(I), _ptr(cls)))
        info = {k: getattr(I, k) for k in RENDER_COMPARE_FIELDS}
        return (info, cls) if class_image else info

    def grid_target(self, nx, ny):
        """the device accumulators and outputs for ground grids of up to nx * ny cells, reused across builds (ssm_grid_target_create) -> an opaque handle
        (grid_target_free it)"""
        t = C.c_void_p()
        self._chk(self.lib.ssm_grid_target_create(self.h, int(nx), int(ny), C.byref(t)))
        self._grid_sizes = getattr(self, "_grid_sizes", {})
        self._grid_sizes[t.value] = None
        return t.value

    def grid_target_free(self, target):
        self._grid_sizes.pop(target, None)
        self.lib.ssm_grid_target_free(self.h, target)

    def grid_form(self, form):
        """how later builds accumulate (ssm_debug_grid_form): 0 one atomic per point, 1 one per run of adjacent lanes with the same destination, -1 the default"""
        self._chk(self.lib.ssm_debug_grid_form(self.h, int(form)))

    def grid_fetch(self, target):
        """the arrays of the target's last build (ssm_grid_fetch) -> {cls, ground_label, obstacle_label, ground_q, top_q, n, n_high}, ny x nx each"""
        nx, ny = self._grid_sizes[target] or (1, 1)
        out = _grid_arrays(nx, ny, False)
        self._chk(self.lib.ssm_grid_fetch(self.h, target, *[_ptr(out[k]) for k, _ in GRID_ARRAYS]))
        return out

    def grid_cells(self, target):
        """the raw per-cell accumulators and base of the target's last build (ssm_debug_grid_cells), ny x nx of GRID_CELL_DTYPE"""
        nx, ny = self._grid_sizes[target] or (1, 1)
        cells = np.zeros((ny, nx), GRID_CELL_DTYPE)
        self._chk(self.lib.ssm_debug_grid_cells(self.h, target, _ptr(cells)))
        return cells

    def _grid_result(self, target, P, I, cells):
        self._grid_sizes[target] = (P.nx, P.ny)
        out = self.grid_fetch(target)
        if cells:
            out["cells"] = self.grid_cells(target)
        out["info"] = {k: getattr(I, k) for k in GRID_INFO_FIELDS}
        return out

    def grid_points(self, target, clouds, T_clouds, cells=False, **params):
        """grid_host's call through the device (ssm_grid_points) -> the same dictionary"""
        keep, ptrs, n, Tc, m = _pack_clouds(clouds, T_clouds, True)
        P = grid_params(**params); I = GridInfo()
        self._chk(self.lib.ssm_grid_points(self.h, target, ptrs, _ptr(n), _ptr(Tc), m, C.byref(P), C.byref(I)))
        return self._grid_result(target, P, I, cells)

    def grid_clouds(self, target, clouds, T_clouds, cells=False, **params):
        """device-resident clouds (backproject_dev's handles) at the poses T_clouds into the grid (ssm_grid_clouds); nothing is uploaded but the poses"""
        _, arr, _, Tc, m = _pack_clouds(clouds, T_clouds, False)
        P = grid_params(**params); I = GridInfo()
        self._chk(self.lib.ssm_grid_clouds(self.h, target, arr, _ptr(Tc), m, C.byref(P), C.byref(I)))
        return self._grid_result(target, P, I, cells)

    def grid_viewer_map(self, target, cells=False, **params):
        """the map the last viewer_map_update left on the device, at the identity pose (ssm_grid_viewer_map)"""
        P = grid_params(**params); I = GridInfo()
        self._chk(self.lib.ssm_grid_viewer_map(self.h, target, C.byref(P), C.byref(I)))
        return self._grid_result(target, P, I, cells)

    def objects_target(self, nx, ny):
        """the device labels, records and object_id image of object extraction for grids of up to nx * ny cells (ssm_objects_target_create) -> an opaque handle
        (objects_target_free it)"""
        t = C.c_void_p()
        self._chk(self.lib.ssm_objects_target_create(self.h, int(nx), int(ny), C.byref(t)))
        self._objects_sizes = getattr(self, "_objects_sizes", {})
        self._objects_sizes[t.value] = None
        return t.value

    def objects_target_free(self, target):
        self._objects_sizes.pop(target, None)
        self.lib.ssm_objects_target_free(self.h, target)

    def objects_form(self, form):
        """how later stage-2 calls accumulate (ssm_debug_objects_form): 0 one atomic per point and figure, 1 one per run of adjacent lanes with the same object,
        -1 the default"""
        self._chk(self.lib.ssm_debug_objects_form(self.h, int(form)))

    def objects_grid(self, grid_target, target, **params):
        """stage 1 on the grid target's last build (ssm_objects_grid) -> info"""
        P = objects_params(**params); I = ObjectsInfo()
        self._chk(self.lib.ssm_objects_grid(self.h, grid_target, C.byref(P), target, C.byref(I)))
        self._objects_sizes[target] = self._grid_sizes[grid_target]
        return _objects_info(I)

    def objects_cells(self, target, cls, obstacle_label, ground_q, top_q, n_high, **params):
        """hand-made ny x nx cell arrays uploaded and stage 1 run on them (ssm_debug_objects_cells) -> info"""
        arr = [np.ascontiguousarray(a, t) for a, t in ((cls, np.uint8), (obstacle_label, np.uint8), (ground_q, np.int32), (top_q, np.int32), (n_high, np.uint32))]
        if arr[0].ndim != 2 or any(a.shape != arr[0].shape for a in arr):
            raise ValueError("five ny x nx arrays of one grid")
        ny, nx = arr[0].shape
        P = objects_params(**params); I = ObjectsInfo()
        self._chk(self.lib.ssm_debug_objects_cells(self.h, target, *[_ptr(a) for a in arr], nx, ny, C.byref(P), C.byref(I)))
        self._objects_sizes[target] = (nx, ny)
        return _objects_info(I)

    def objects_clouds(self, grid_target, target, clouds, T_clouds):
        """stage 2 on the device clouds the grid was built from, at the same poses (ssm_objects_clouds) -> info"""
        _, arr, _, Tc, m = _pack_clouds(clouds, T_clouds, False)
        I = ObjectsInfo()
        self._chk(self.lib.ssm_objects_clouds(self.h, grid_target, target, arr, _ptr(Tc), m, C.byref(I)))
        return _objects_info(I)

    def objects_points(self, grid_target, target, clouds, T_clouds):
        """stage 2 on host arrays, through the device (ssm_objects_points) -> (the per-point object ids of the concatenation, info)"""
        keep, ptrs, n, Tc, m = _pack_clouds(clouds, T_clouds, True)
        total = int(n[:m].sum())
        ids = np.full(max(total, 1), -2, np.int32); I = ObjectsInfo()
        self._chk(self.lib.ssm_objects_points(self.h, grid_target, target, ptrs, _ptr(n), _ptr(Tc), m, _ptr(ids), C.byref(I)))
        return ids[:total].copy(), _objects_info(I)

    def objects_viewer_map(self, grid_target, target):
        """stage 2 on the map the last viewer_map_update left on the device (ssm_objects_viewer_map) -> info"""
        I = ObjectsInfo()
        self._chk(self.lib.ssm_objects_viewer_map(self.h, grid_target, target, C.byref(I)))
        return _objects_info(I)

    def objects_fetch(self, target, cap=None):
        """the records of the target's last stage 1 with the point figures of its last stage 2, and the object_id image (ssm_objects_fetch) -> (records of
        OBJECT_DTYPE, ny x nx int32); cap: the record buffer's size (default: enough)"""
        size = self._objects_sizes[target]          # None: nothing was labelled into the target through this binding -- the image's size is not known, so it is not fetched
        n = C.c_int(0)
        if cap is None:
            self._chk(self.lib.ssm_objects_fetch(self.h, target, None, 0, C.byref(n), None))
            cap = n.value
        out = np.zeros(max(int(cap), 1), OBJECT_DTYPE); oid = np.full((size[1], size[0]), -2, np.int32) if size else None
        self._chk(self.lib.ssm_objects_fetch(self.h, target, _ptr(out), int(cap), C.byref(n), _ptr(oid)))
        return out[:n.value].copy(), oid

    def objects_point_ids(self, n):
        """the per-point object ids of the context's last stage-2 call (ssm_debug_objects_point_ids)"""
        ids = np.full(max(int(n), 1), -2, np.int32)
        self._chk(self.lib.ssm_debug_objects_point_ids(self.h, _ptr(ids), int(n)))
        return ids[:int(n)].copy()

    def clearance_target(self, nx, ny):
        """the device images and labels of the clearance map for grids of up to nx * ny cells (ssm_clearance_target_create) -> an opaque handle (clearance_target_free
        it)"""
        t = C.c_void_p()
        self._chk(self.lib.ssm_clearance_target_create(self.h, int(nx), int(ny), C.byref(t)))
        self._clearance_sizes = getattr(self, "_clearance_sizes", {})
        self._clearance_sizes[t.value] = None
        return t.value

    def clearance_target_free(self, target):
        self._clearance_sizes.pop(target, None)
        self.lib.ssm_clearance_target_free(self.h, target)

    def clearance_form(self, form):
        """the row pass of later calls (ssm_debug_clearance_form): 0 the whole row staged through LDS, 1 an outward scan, -1 the default"""
        self._chk(self.lib.ssm_debug_clearance_form(self.h, int(form)))

    def clearance_grid(self, grid_target, target, **params):
        """the clearance map of the grid target's last build (ssm_clearance_grid) -> info"""
        P = clearance_params(**params); I = ClearanceInfo()
        self._chk(self.lib.ssm_clearance_grid(self.h, grid_target, C.byref(P), target, C.byref(I)))
        self._clearance_sizes[target] = self._grid_sizes[grid_target]
        return _clearance_info(I)

    def clearance_cells(self, target, cls, **params):
        """a hand-made ny x nx class image uploaded and the stage run on it (ssm_debug_clearance_cells) -> info"""
        a = _clearance_cls(cls)
        ny, nx = a.shape
        P = clearance_params(**params); I = ClearanceInfo()
        self._chk(self.lib.ssm_debug_clearance_cells(self.h, target, _ptr(a), nx, ny, C.byref(P), C.byref(I)))
        self._clearance_sizes[target] = (nx, ny)
        return _clearance_info(I)

    def clearance_fetch(self, target):
        """the images of the target's last call (ssm_clearance_fetch) -> (dist2 uint32, nearest int32, reach uint8), ny x nx each"""
        nx, ny = self._clearance_sizes[target]
        d2 = np.zeros((ny, nx), np.uint32); near = np.full((ny, nx), -2, np.int32); reach = np.full((ny, nx), 255, np.uint8)
        self._chk(self.lib.ssm_clearance_fetch(self.h, target, _ptr(d2), _ptr(near), _ptr(reach)))
        return d2, near, reach

    def route_target(self, nx, ny, max_path=None):
        """the device field and path arrays of the route field for grids of up to nx * ny cells and paths of up to max_path cells (default 4 (nx + ny))
        (ssm_route_target_create) -> an opaque handle (route_target_free it)"""
        max_path = 4 * (int(nx) + int(ny)) if max_path is None else int(max_path)
        t = C.c_void_p()
        self._chk(self.lib.ssm_route_target_create(self.h, int(nx), int(ny), max_path, C.byref(t)))
        self._route_sizes = getattr(self, "_route_sizes", {})
        self._route_sizes[t.value] = (None, max_path)
        return t.value

    def route_target_free(self, target):
        self._route_sizes.pop(target, None)
        self.lib.ssm_route_target_free(self.h, target)

    def route_form(self, form):
        """how later fields relax (ssm_debug_route_form): 0 sweeps of one thread per cell in batches, 1 active tiles relaxed to their fixed points, -1 the default"""
        self._chk(self.lib.ssm_debug_route_form(self.h, int(form)))

    def route_rounds(self):
        """how many times the last field asked the device whether it was done (ssm_debug_route_rounds)"""
        return self.lib.ssm_debug_route_rounds(self.h)

    def route_field(self, clearance_target, target, **params):
        """the route field over the clearance target's last result (ssm_route_field) -> info"""
        P = route_params(**params); I = RouteInfo()
        self._chk(self.lib.ssm_route_field(self.h, clearance_target, C.byref(P), target, C.byref(I)))
        self._route_sizes[target] = (self._clearance_sizes[clearance_target], self._route_sizes[target][1])
        return _route_info(I)

    def route_cells(self, target, reach, dist2, source=None, **params):
        """hand-made ny x nx reach and dist2 images uploaded and the stage run on them (ssm_debug_route_cells); source: None, a cell index or (cx, cy) -> info"""
        r, d, src = _route_inputs(reach, dist2, source)
        ny, nx = r.shape
        P = route_params(**params); I = RouteInfo()
        self._chk(self.lib.ssm_debug_route_cells(self.h, target, _ptr(r), _ptr(d), nx, ny, src, C.byref(P), C.byref(I)))
        self._route_sizes[target] = ((nx, ny), self._route_sizes[target][1])
        return _route_info(I)

    def route_path(self, target, goal, goal_snap=0):
        """a path of the target's field to the goal (cx, cy) (ssm_route_path) -> (the path's cell indices int32, source first, path info).  A path longer than the
        target's max_path raises SsmError with code SSM_E_CAPACITY; its `info` attribute holds the path info"""
        I = RoutePathInfo()
        cells = np.full(max(getattr(self, "_route_sizes", {}).get(target, (None, 1))[1], 1), -2, np.int32)          # (a handle this binding does not know: the library refuses it)
        rc = self.lib.ssm_route_path(self.h, target, int(goal[0]), int(goal[1]), int(goal_snap), _ptr(cells), C.byref(I))
        if rc != 0:
            e = SsmError(rc, (self.lib.ssm_last_error(self.h) or b"").decode()); e.info = _route_path_info(I)
            raise e
        return cells[:I.len].copy(), _route_path_info(I)

    def route_fetch(self, target, shape=None):
        """the images of the target's field (ssm_route_fetch) -> (cost uint32, parent int32), ny x nx each.  shape: (nx, ny) of a field that was not made through this
        binding (a call on the library itself); otherwise the binding remembers it"""
        known = getattr(self, "_route_sizes", {}).get(target, (None, 1))[0]
        if shape is None and known is None:
            self._chk(self.lib.ssm_route_fetch(self.h, target, None, None))          # (no field, or a handle of another context: the library refuses with its own message)
            raise ValueError("route_fetch: the field was not made through this binding; pass shape=(nx, ny)")
        nx, ny = known if shape is None else (int(shape[0]), int(shape[1]))
        cost = np.zeros((ny, nx), np.uint32); parent = np.full((ny, nx), -2, np.int32)
        self._chk(self.lib.ssm_route_fetch(self.h, target, _ptr(cost), _ptr(parent)))
        return cost, parent

    def relabel_view(self, depth, sem_bgr, camera=None):
        """a view of label fusion: the depth image goes to the device and the label image is made there from the semantic BGR image (ssm_relabel_view_create) -> an
        opaque handle (relabel_view_free it)"""
        depth = np.ascontiguousarray(depth, np.uint16); sem = np.ascontiguousarray(sem_bgr, np.uint8)
        h, w = depth.shape
        if sem.shape != (h, w, 3):
            raise ValueError("sem_bgr: h x w x 3, the depth image's size")
        cam = Camera(*camera) if camera is not None else self.cfg.camera
        v = C.c_void_p()
        self._chk(self.lib.ssm_relabel_view_create(self.h, _ptr(depth), _ptr(sem), w, h, C.byref(cam), C.byref(v)))
        self._relabel_sizes = getattr(self, "_relabel_sizes", {})
        self._relabel_sizes[v.value] = (w, h)
        return v.value

    def relabel_view_free(self, view):
        getattr(self, "_relabel_sizes", {}).pop(view, None)
        self.lib.ssm_relabel_view_free(self.h, view)

    def relabel_view_labels(self, view):
        """the view's label image as the device made it (ssm_debug_relabel_view)"""
        w, h = self._relabel_sizes[view]
        out = np.zeros((h, w), np.uint8)
        self._chk(self.lib.ssm_debug_relabel_view(self.h, view, _ptr(out)))
        return out

    def relabel_form(self, form):
        """how later views are stored and read (ssm_debug_relabel_form): 0 a depth and a label image, 1 one packed word per pixel, 2 packed with two views in flight, -1 the default"""
        self._chk(self.lib.ssm_debug_relabel_form(self.h, int(form)))

    def relabel_record(self, n):
        """every point's packed counts and label after the context's last device call over n points (ssm_debug_relabel_record) -> (votes, labels)"""
        votes = np.zeros(n, np.uint64); labels = np.zeros(n, np.uint32)
        self._chk(self.lib.ssm_debug_relabel_record(self.h, _ptr(votes), _ptr(labels), n))
        return votes, labels

    def relabel(self, views, T_views, cloud, T_cloud, **params):
        """the views (relabel_view's handles at the world poses T_views) vote on the labels of a device-resident cloud (backproject_dev's handle) at T_cloud, which
        changes in place (ssm_relabel) -> info"""
        v = len(views)
        if len(T_views) != v:
            raise ValueError("one pose per view")
        arr = (C.c_void_p * max(v, 1))(*views)
        P = relabel_params(**params); I = RelabelInfo()
        Tv, Tc = _relabel_poses(T_views), _cm16(T_cloud)
        self._chk(self.lib.ssm_relabel(self.h, arr, _ptr(Tv), v, cloud, _ptr(Tc), C.byref(P), C.byref(I)))
        return _relabel_info(I)

    def relabel_points(self, views, T_views, points, T_cloud, **params):
        """relabel_host's call through the device (ssm_relabel_points), views as for relabel -> (labels, info)"""
        points = _sor_points(points)
        n, v = len(points), len(views)
        if len(T_views) != v:
            raise ValueError("one pose per view")
        arr = (C.c_void_p * max(v, 1))(*views)
        P = relabel_params(**params); I = RelabelInfo()
        labels = np.zeros(n, np.uint32)
        Tv, Tc = _relabel_poses(T_views), _cm16(T_cloud)
        self._chk(self.lib.ssm_relabel_points(self.h, arr, _ptr(Tv), v, _ptr(points), n, _ptr(Tc), C.byref(P), _ptr(labels), C.byref(I)))
        return labels, _relabel_info(I)

    def align_view(self, depth, camera=None, **params):
        """a view of dense alignment: the depth image goes to the device and its normal map is built there (ssm_align_view_create; params: the edge gate) -> an
        opaque handle (align_view_free it)"""
        depth = np.ascontiguousarray(depth, np.uint16)
        h, w = depth.shape
        cam = Camera(*camera) if camera is not None else self.cfg.camera
        P = align_params(**params); v = C.c_void_p()
        self._chk(self.lib.ssm_align_view_create(self.h, _ptr(depth), w, h, C.byref(cam), C.byref(P), C.byref(v)))
        self._align_sizes = getattr(self, "_align_sizes", {})
        self._align_sizes[v.value] = (w, h)
        return v.value

    def align_view_free(self, view):
        self._align_sizes.pop(view, None)
        self.lib.ssm_align_view_free(self.h, view)

    def align_normals(self, view):
        """the view's valid mask and normals as align_host gives them (ssm_debug_align_normals) -> (valid, normals)"""
        w, h = self._align_sizes[view]
        valid = np.zeros((h, w), np.uint8); normals = np.zeros((h, w, 4), np.float32)
        self._chk(self.lib.ssm_debug_align_normals(self.h, view, _ptr(valid), _ptr(normals)))
        return valid, normals

    def align_record(self):
        """the iterations of the context's last device alignment (ssm_debug_align_record): ALIGN_ITER_DTYPE entries"""
        rec = np.zeros(ALIGN_MAX_ITERATIONS, ALIGN_ITER_DTYPE); n = C.c_int(0)
        self._chk(self.lib.ssm_debug_align_record(self.h, _ptr(rec), len(rec), C.byref(n)))
        return rec[:n.value].copy()

    def align_points(self, view, T_view, clouds, T_clouds, **params):
        """align_host's call through the device (ssm_align_points) -> {T_view, info}"""
        keep, ptrs, n, Tc, m = _pack_clouds(clouds, T_clouds, True)
        P = align_params(**params); I = AlignInfo(); T_out = np.zeros(16)
        self._chk(self.lib.ssm_align_points(self.h, view, _ptr(_cm16(T_view)), ptrs, _ptr(n), _ptr(Tc), m, C.byref(P), _ptr(T_out), C.byref(I)))
        return {"T_view": T_out.reshape(4, 4).T.copy(), "info": _align_info(I)}

    def align_clouds(self, view, T_view, clouds, T_clouds, **params):
        """device-resident clouds (backproject_dev's handles) at the poses T_clouds against the view (ssm_align_clouds); the clouds are not modified"""
        _, arr, _, Tc, m = _pack_clouds(clouds, T_clouds, False)
        P = align_params(**params); I = AlignInfo(); T_out = np.zeros(16)
        self._chk(self.lib.ssm_align_clouds(self.h, view, _ptr(_cm16(T_view)), arr, _ptr(Tc), m, C.byref(P), _ptr(T_out), C.byref(I)))
        return {"T_view": T_out.reshape(4, 4).T.copy(), "info": _align_info(I)}

    def backproject_fused(self, depth, rgb, sem, motion=None, T=None, camera=None, max_distance=None, area_thres=1000, overlay_thres=0.143, device=False):
        """generate_point_cloud with the fused mask (ssm_backproject_fused); device=True: backproject_dev's form, -> an opaque cloud handle (cloud_free it)"""
        depth = np.ascontiguousarray(depth, np.uint16); rgb = np.ascontiguousarray(rgb, np.uint8)
        sem, motion = _mf_images(sem, motion)
        h, w = depth.shape
        cam = Camera(*camera) if camera is not None else self.cfg.camera
        md = self.cfg.mapper_max_distance if max_distance is None else max_distance
        P = MotionFuseParams(int(area_thres), 0, float(overlay_thres))
        if device:
            cl = C.c_void_p()
            self._chk(self.lib.ssm_backproject_fused_dev(self.h, _ptr(depth), _ptr(rgb), _ptr(sem), _ptr(motion), w, h, C.byref(cam), md, C.byref(P), C.byref(cl)))
            return cl.value
        Tc = None if T is None else np.ascontiguousarray(np.asarray(T, np.float64).reshape(4, 4).T)
        out = np.zeros(w * h, POINT_DTYPE)
        n = C.c_int(0)
        self._chk(self.lib.ssm_backproject_fused(self.h, _ptr(depth), _ptr(rgb), _ptr(sem), _ptr(motion), w, h, C.byref(cam), _ptr(Tc), md, C.byref(P),
                                                 _ptr(out), len(out), C.byref(n)))
        return out[:n.value]

    def generate_point_cloud(self, depth, rgb, sem, T=None, camera=None, max_distance=None):
        depth = np.ascontiguousarray(depth, np.uint16)
        rgb = np.ascontiguousarray(rgb, np.uint8)
        sem = np.ascontiguousarray(sem, np.uint8)
        h, w = depth.shape
        cam = Camera(*camera) if camera is not None else self.cfg.camera
        md = self.cfg.mapper_max_distance if max_distance is None else max_distance
        Tc = None if T is None else np.ascontiguousarray(np.asarray(T, np.float64).reshape(4, 4).T)  # column-major
        out = np.zeros(w * h, POINT_DTYPE)
        n = C.c_int(0)
        self._chk(self.lib.ssm_backproject(self.h, _ptr(depth), _ptr(rgb), _ptr(sem), w, h, C.byref(cam), _ptr(Tc), md,
                                           _ptr(out), len(out), C.byref(n)))
        return out[:n.value]

    # ---- device-resident Mapper: key-frame clouds and the viewer's map stay in HBM (ssm_backproject_dev / ssm_viewer_map_*)
    def backproject_dev(self, depth, rgb, sem, camera=None, max_distance=None):
        """camera-frame cloud of one frame, left on the device: returns an opaque handle (cloud_free it)"""
        depth = np.ascontiguousarray(depth, np.uint16); rgb = np.ascontiguousarray(rgb, np.uint8); sem = np.ascontiguousarray(sem, np.uint8)
        h, w = depth.shape
        cam = Camera(*camera) if camera is not None else self.cfg.camera
        md = self.cfg.mapper_max_distance if max_distance is None else max_distance
        cl = C.c_void_p()
        self._chk(self.lib.ssm_backproject_dev(self.h, _ptr(depth), _ptr(rgb), _ptr(sem), w, h, C.byref(cam), md, C.byref(cl)))
        return cl.value

    def cloud_size(self, cloud):
        return self.lib.ssm_cloud_size(cloud)

    def cloud_fetch(self, cloud, T=None):
        n = self.cloud_size(cloud)
        out = np.zeros(max(n, 1), POINT_DTYPE); m = C.c_int(0)
        Tc = None if T is None else np.ascontiguousarray(np.asarray(T, np.float64).reshape(4, 4).T)
        self._chk(self.lib.ssm_cloud_fetch(self.h, cloud, _ptr(Tc), _ptr(out), len(out), C.byref(m)))
        return out[:m.value]

    def cloud_free(self, cloud):
        self.lib.ssm_cloud_free(self.h, cloud)

    def viewer_map_update(self, clouds, poses, rebuild=False, leaf=None):
        """Mapper::viewer's update on the device: map <- VoxelGrid((rebuild ? nothing : previous map) + sum poses[i] * clouds[i]); returns the voxel count"""
        leaf = self.cfg.mapper_resolution if leaf is None else leaf
        arr = (C.c_void_p * max(len(clouds), 1))(*clouds)
        P = np.ascontiguousarray(np.stack([np.asarray(T, np.float64).reshape(4, 4).T.reshape(16) for T in poses]) if len(poses) else np.zeros((1, 16)))
        n = C.c_int(0)
        self._chk(self.lib.ssm_viewer_map_update(self.h, int(rebuild), arr, _ptr(P), len(clouds), leaf, C.byref(n)))
        return n.value

    def viewer_map_fetch(self, n):
        out = np.zeros(max(n, 1), POINT_DTYPE); m = C.c_int(0)
        self._chk(self.lib.ssm_viewer_map_fetch(self.h, _ptr(out), len(out), C.byref(m)))
        return out[:m.value]

    def voxel_filter(self, pts, leaf=None, cap=None):
        pts = np.ascontiguousarray(pts, POINT_DTYPE)
        leaf = self.cfg.mapper_resolution if leaf is None else leaf
        out = np.zeros(cap if cap is not None else max(len(pts), 1), POINT_DTYPE)
        n = C.c_int(0)
        self._chk(self.lib.ssm_voxel_filter(self.h, _ptr(pts), len(pts), leaf, _ptr(out), len(out), C.byref(n)))
        return out[:n.value]

    def map_clear(self):
        self._chk(self.lib.ssm_map_clear(self.h))

    def map_insert(self, pts):
        pts = np.ascontiguousarray(pts, POINT_DTYPE)
        self._chk(self.lib.ssm_map_insert(self.h, _ptr(pts), len(pts)))

    def map_stats(self):
        """(log2 slots, times grown, blocks of the map kernel run again, overflow-list records): ssm_map_stats"""
        st = (C.c_int64 * 4)()
        self._chk(self.lib.ssm_map_stats(self.h, st))
        return tuple(int(v) for v in st)

    def map_size(self):
        n = C.c_int(0)
        self._chk(self.lib.ssm_map_size(self.h, C.byref(n)))
        return n.value

    def map_export(self):
        out = np.zeros(max(self.map_size(), 1), POINT_DTYPE)
        n = C.c_int(0)
        self._chk(self.lib.ssm_map_export(self.h, _ptr(out), len(out), C.byref(n)))
        return out[:n.value]

    def map_export_table(self):
        out = np.zeros(max(self.map_size(), 1), VOXEL_DTYPE)
        n = C.c_int(0)
        self._chk(self.lib.ssm_map_export_table(self.h, _ptr(out), len(out), C.byref(n)))
        return out[:n.value]

    def map_merge_table(self, tab):
        tab = np.ascontiguousarray(tab, VOXEL_DTYPE)
        self._chk(self.lib.ssm_map_merge_table(self.h, _ptr(tab), len(tab)))

    def map_export_table_dev(self, dptr, cap):
        n = C.c_int(0)
        self._chk(self.lib.ssm_map_export_table_dev(self.h, dptr, cap, C.byref(n)))
        return n.value

    def map_merge_table_dev(self, dptr, n):
        self._chk(self.lib.ssm_map_merge_table_dev(self.h, dptr, n))

    # ---- multi-GPU: the communicator lives in the context (RCCL inside libssm_hip.so, no torch on the data path)
    def comm_unique_id(self):
        """rank 0: ncclGetUniqueId as SSM_COMM_ID_BYTES bytes, to be shipped to every rank"""
        buf = (C.c_ubyte * COMM_ID_BYTES)()
        self._chk(self.lib.ssm_comm_get_unique_id(buf))
        return bytes(buf)

    def comm_init_rank(self, nranks, rank, unique_id):
        assert len(unique_id) == COMM_ID_BYTES
        buf = (C.c_ubyte * COMM_ID_BYTES).from_buffer_copy(unique_id)
        self._chk(self.lib.ssm_comm_init_rank(self.h, nranks, rank, buf))

    def comm_finalize(self):
        self._chk(self.lib.ssm_comm_finalize(self.h))

    def voxel_allgather(self, rccl_comm=None):
        """merge the context maps of all ranks: one RCCL all-gather of the voxel tables + re-insertion of the remote ones"""
        self._chk(self.lib.ssm_voxel_allgather(self.h, rccl_comm))

    # ---- device-resident sequence path
    def dev_alloc(self, nbytes):
        p = C.c_void_p()
        self._chk(self.lib.ssm_dev_alloc(self.h, nbytes, C.byref(p)))
        return p.value

    def dev_free(self, p):
        self._chk(self.lib.ssm_dev_free(self.h, p))

    def host_alloc(self, shape, dtype):
        """a numpy array in page-locked host memory (ssm_host_alloc): such inputs are read by the device where they are.  Free it with host_free(array)."""
        shape = tuple(int(v) for v in np.atleast_1d(shape)); dt = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * dt.itemsize
        p = C.c_void_p()
        self._chk(self.lib.ssm_host_alloc(max(nbytes, 1), C.byref(p)))
        arr = np.frombuffer((C.c_char * nbytes).from_address(p.value), dtype=dt).reshape(shape)
        self._pinned = getattr(self, "_pinned", {}); self._pinned[arr.ctypes.data] = p.value
        return arr

    def host_free(self, arr):
        p = self._pinned.pop(arr.ctypes.data)
        self._chk(self.lib.ssm_host_free(C.c_void_p(p)))

    def mem_info(self):
        """(free, total) bytes of the context's device"""
        f, t = C.c_size_t(0), C.c_size_t(0)
        self._chk(self.lib.ssm_dev_mem_info(self.h, C.byref(f), C.byref(t)))
        return f.value, t.value

    def h2d(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        self._chk(self.lib.ssm_memcpy_h2d(self.h, dptr, _ptr(arr), arr.nbytes))

    def d2h(self, dptr, shape, dtype):
        out = np.zeros(shape, dtype)
        if out.nbytes:
            self._chk(self.lib.ssm_memcpy_d2h(self.h, _ptr(out), dptr, out.nbytes))
        return out

    def synth_frames_dev(self, seed, first, n, bgr, depth, sem, pose, labels=None):
        self._chk(self.lib.ssm_synth_frames_dev(self.h, seed, first, n, self.W, self.H, bgr, depth, sem, labels, pose))

    def seq_process(self, bgr, depth, sem, pose, n, continue_sequence=False, stages=0):
        fr = FramesDev(bgr, depth, sem, pose, n, int(continue_sequence), stages)
        out = SeqOutDev()
        self._chk(self.lib.ssm_seq_process(self.h, C.byref(fr), C.byref(out)))
        return out

    def sync(self):
        try:
            self._chk(self.lib.ssm_sync(self.h))
        finally:
            self._inflight.clear()

    def last_error(self):
        """ssm_last_error: the last failing call's text, or a "note: ..." a successful call left (an SGBM sweep repeated in form 1)"""
        return (self.lib.ssm_last_error(self.h) or b"").decode()

    def set_profiling(self, on):
        self._chk(self.lib.ssm_set_profiling(self.h, int(on)))

    def stage_times(self):
        names = (C.c_char_p * 32)()
        ms = (C.c_float * 32)()
        ln = (C.c_int * 32)()
        n = C.c_int(0)
        self._chk(self.lib.ssm_get_stage_times(self.h, names, ms, ln, 32, C.byref(n)))
        return {names[i].decode(): (ms[i], ln[i]) for i in range(min(n.value, 32))}

    def seq_fetch(self, out, n):
        """Copy the outputs of seq_process back to the host (test helper)."""
        cap, R = out.cap, out.R
        res = {
            "nkp": self.d2h(out.nkp, n, np.int32),
            "kps": self.d2h(out.kps, (n, cap), KEYPOINT_DTYPE),
            "desc": self.d2h(out.desc, (n, cap, 32), np.uint8),
            "pos3d": self.d2h(out.pos3d, (n, cap, 3), np.float32),
            "nmatch": self.d2h(out.nmatch, (n, R), np.int32),
            "matches": self.d2h(out.matches, (n, R, cap), DMATCH_DTYPE),
            "npoints": self.d2h(out.npoints, n, np.int32),
        }
        return res


PGO_MAX_ITERS, PGO_MAX_TRIALS, PGO_PHASES = 32, 10, 5
PGO_REPORT_DTYPE = np.dtype([("iterations", "i4"), ("active_vertices", "i4"), ("active_edges", "i4"), ("solve_failures", "i4"), ("envelope_scalars", "i8"), ("lambda", "f8"),
                             ("trials", "i4", (PGO_MAX_ITERS,)), ("accepted", "u4", (PGO_MAX_ITERS,)), ("chi2_before", "f8", (PGO_MAX_ITERS,)), ("chi2_after", "f8", (PGO_MAX_ITERS,)),
                             ("gain", "f8", (PGO_MAX_ITERS, PGO_MAX_TRIALS)), ("clocks", "i8", (PGO_PHASES,))])
assert PGO_REPORT_DTYPE.itemsize == 32 + 4 * 32 * 2 + 8 * 32 * 2 + 8 * 320 + 40


class PoseGraphOptimizer:
    """ssm_pgo: PoseGraph's optimiser (src/pose_graph.cpp:82-305) -- SE3 vertices, SE3 edges with Huber kernels, Levenberg over a block-envelope L D L^T
    (DESIGN.md s.12).  PoseGraphOptimizer(ctx) has the device path (optimize, one 1024-thread block per graph); PoseGraphOptimizer(None) is a host-only
    object whose optimize_host needs no GPU.  Both give the same bits.  Poses are 4 x 4 matrices in the usual row-major numpy form."""

    def __init__(self, ctx=None, envelope_cap=None):
        self.ctx = ctx; self.lib = ctx.lib if ctx is not None else _lib.load()
        h = C.c_void_p()
        rc = self.lib.ssm_pgo_create(ctx.h if ctx is not None else None, C.byref(h))
        if rc != 0:
            raise SsmError(rc, (self.lib.ssm_last_error(ctx.h if ctx is not None else None) or b"").decode())
        self.h = h
        if envelope_cap is not None:
            self.set_envelope_cap(envelope_cap)

    def _chk(self, rc):
        if rc != 0:
            raise SsmError(rc, (self.lib.ssm_last_error(self.ctx.h if self.ctx is not None else None) or b"").decode())

    @staticmethod
    def _cm(T):
        """a 4 x 4 matrix as the ABI's 16 column-major doubles"""
        T = np.asarray(T, np.float64)
        assert T.shape == (4, 4)
        return np.ascontiguousarray(T.T).reshape(16)

    def clear(self):
        self._chk(self.lib.ssm_pgo_clear(self.h))

    def add_vertex(self, vid, T, fixed=False):
        self._chk(self.lib.ssm_pgo_add_vertex(self.h, int(vid), _ptr(self._cm(T)), int(bool(fixed))))

    def add_edge(self, id_from, id_to, Z, info=None, robust=True):
        """info: None (100 I), a 6 x 6 symmetric matrix, or the 21 upper-triangle entries row by row"""
        i21 = None
        if info is not None:
            info = np.asarray(info, np.float64)
            i21 = np.ascontiguousarray(info[np.triu_indices(6)] if info.shape == (6, 6) else info.reshape(21))
        self._chk(self.lib.ssm_pgo_add_edge(self.h, int(id_from), int(id_to), _ptr(self._cm(Z)), _ptr(i21) if i21 is not None else None, int(bool(robust))))

    def set_fixed(self, vid, fixed=True):
        self._chk(self.lib.ssm_pgo_set_fixed(self.h, int(vid), int(bool(fixed))))

    def set_mode(self, local):
        """False: every vertex free but the first; True: only the last five free (fewer than six vertices: none)"""
        self._chk(self.lib.ssm_pgo_set_mode(self.h, int(bool(local))))

    def set_pose(self, vid, T):
        self._chk(self.lib.ssm_pgo_set_pose(self.h, int(vid), _ptr(self._cm(T))))

    def set_envelope_cap(self, nbytes):
        self._chk(self.lib.ssm_pgo_set_envelope_cap(self.h, int(nbytes)))

    def size(self):
        v, e = C.c_int(0), C.c_int(0)
        self._chk(self.lib.ssm_pgo_size(self.h, C.byref(v), C.byref(e)))
        return v.value, e.value

    def poses(self):
        """(ids, n x 4 x 4 poses) in insertion order"""
        n = self.size()[0]
        ids = np.zeros(max(n, 1), np.int32); T = np.zeros((max(n, 1), 16))
        k = C.c_int(0)
        self._chk(self.lib.ssm_pgo_get_poses(self.h, _ptr(ids), _ptr(T), n, C.byref(k)))
        return ids[:n], np.ascontiguousarray(T[:n].reshape(n, 4, 4).transpose(0, 2, 1))

    def edge_chi2(self, edge):
        v = C.c_double(0)
        self._chk(self.lib.ssm_pgo_edge_chi2(self.h, int(edge), C.byref(v)))
        return v.value

    def _opt(self, fn, iterations):
        rep = np.zeros(1, PGO_REPORT_DTYPE)
        self._chk(fn(self.h, int(iterations), _ptr(rep)))
        return rep[0]

    def optimize(self, iterations=10):
        """on the device -> the report (PGO_REPORT_DTYPE)"""
        return self._opt(self.lib.ssm_pgo_optimize, iterations)

    def optimize_host(self, iterations=10):
        """the same on the CPU (no GPU needed): the same bits"""
        return self._opt(self.lib.ssm_pgo_optimize_host, iterations)

    @staticmethod
    def optimize_many(graphs, iterations=10):
        """the graphs (of one context) as the blocks of one launch -> their reports"""
        g0 = graphs[0]
        hs = (C.c_void_p * len(graphs))(*[g.h for g in graphs])
        rep = np.zeros(len(graphs), PGO_REPORT_DTYPE)
        g0._chk(g0.lib.ssm_pgo_optimize_many(hs, len(graphs), int(iterations), _ptr(rep)))
        return rep

    def envelope(self):
        """(first block column of every block row, scalars) of the current active set"""
        n, tot = C.c_int(0), C.c_int64(0)
        self._chk(self.lib.ssm_pgo_envelope(self.h, None, 0, C.byref(n), C.byref(tot)))
        first = np.zeros(max(n.value, 1), np.int32)
        self._chk(self.lib.ssm_pgo_envelope(self.h, _ptr(first), n.value, C.byref(n), C.byref(tot)))
        return first[:n.value], tot.value

    def linearize(self, device=False):
        """dict(e, Ji, Jj, w of the active edges; H: the assembled envelope; b; first) at the current estimate"""
        first, tot = self.envelope()
        rep_v, rep_e = len(first), self.active()[1]
        out = dict(e=np.zeros((rep_e, 6)), Ji=np.zeros((rep_e, 6, 6)), Jj=np.zeros((rep_e, 6, 6)), w=np.zeros(rep_e), H=np.zeros(max(tot, 1)), b=np.zeros(6 * rep_v + 1))
        self._chk(self.lib.ssm_pgo_linearize(self.h, int(bool(device)), *[_ptr(out[k]) for k in ("e", "Ji", "Jj", "w", "H", "b")]))
        out["H"] = out["H"][:tot]; out["b"] = out["b"][:6 * rep_v]; out["first"] = first
        return out

    def active(self):
        """(active free vertices, active edges) of the current graph; the last report and times stay"""
        v, e = C.c_int(0), C.c_int(0)
        self._chk(self.lib.ssm_pgo_active(self.h, C.byref(v), C.byref(e)))
        return v.value, e.value

    def factor_solve(self, first, H, b, lam, device=False):
        """(H + lam I) x = b on a caller-given envelope -> (x, ok)"""
        first = np.ascontiguousarray(first, np.int32); H = np.ascontiguousarray(H, np.float64); b = np.ascontiguousarray(b, np.float64)
        nr = len(first)
        assert len(b) == 6 * nr and len(H) == 36 * int(np.sum(np.arange(nr) - first + 1))
        x = np.zeros(6 * nr); ok = C.c_int(0)
        self._chk(self.lib.ssm_pgo_factor_solve(self.h, int(bool(device)), nr, _ptr(first), _ptr(H), _ptr(b), float(lam), _ptr(x), C.byref(ok)))
        return x, bool(ok.value)

    def times(self):
        """ms of the last device call per phase: linearise, assemble, factor + solves, update + chi2, decide"""
        t = (C.c_double * 5)()
        self._chk(self.lib.ssm_pgo_times(self.h, C.byref(t)))
        return tuple(float(x) for x in t)

    def save_g2o(self, path):
        self._chk(self.lib.ssm_pgo_save_g2o(self.h, str(path).encode()))

    def load_g2o(self, path, robust=True):
        self._chk(self.lib.ssm_pgo_load_g2o(self.h, str(path).encode(), int(bool(robust))))

    def close(self):
        """before the context's close(), like a Looper"""
        if getattr(self, "h", None):
            if self.ctx is None or self.ctx.h:
                self.lib.ssm_pgo_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
