"""The scenes and the case list the CPU and GPU tests of dense alignment share.  Every scene is analytic: planes and one axis-aligned box,
ray-cast into uint16 depth from known camera-to-world poses; clouds are other poses' depth images back-projected to float32 camera-frame points.  A case is
dict(depth, camera, T_view, T_true, clouds, T_clouds, params): T_true is the pose the view was cast from, T_view the perturbed pose handed to the alignment."""
import math
import numpy as np
import carve_ref as CR

POINT_DTYPE = CR.POINT_DTYPE


def se3(rx=0.0, ry=0.0, rz=0.0, tx=0.0, ty=0.0, tz=0.0):
    """a pose from three small rotations (about x, then y, then z) and a translation"""
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = (tx, ty, tz)
    return T


# a room corner seen from inside (camera: x right, y down, z forward): floor y = 1, left wall x = -1.5, back wall z = 4, and a box standing on the floor
ROOM = dict(planes=[((0.0, 1.0, 0.0), 1.0), ((1.0, 0.0, 0.0), -1.5), ((0.0, 0.0, 1.0), 4.0)], box=((0.1, 0.35, 2.4), (0.9, 1.0, 3.1)))
# a road: the ground y = 1.6 alone, and a box beside the lane
ROAD = dict(planes=[((0.0, 1.0, 0.0), 1.6)], box=((1.5, 0.4, 9.0), (3.0, 1.6, 12.0)))
WALL = dict(planes=[((0.0, 0.0, 1.0), 2.0)], box=None)          # one plane in front of the identity camera: fronto-parallel


def ray_cast(scene, T, camera, w, h):
    """the scene's uint16 depth image (camera-frame z, rounded to depth units; 0: nothing hit or out of range) from the camera-to-world pose T"""
    cx, cy, fx, fy, scale = (float(v) for v in camera)
    ys, xs = np.mgrid[0:h, 0:w]
    dc = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones((h, w))], -1)          # camera-frame direction with z = 1: the ray parameter IS the depth
    R, o = np.asarray(T)[:3, :3], np.asarray(T)[:3, 3]
    dw = dc @ R.T
    best = np.full((h, w), np.inf)
    with np.errstate(all="ignore"):
        for n, d in scene["planes"]:
            n = np.asarray(n, np.float64)
            t = (d - n @ o) / (dw @ n)
            best = np.where((t > 1e-6) & (t < best), t, best)
        if scene["box"] is not None:
            lo, hi = (np.asarray(v, np.float64) for v in scene["box"])
            t0 = (lo - o) / dw
            t1 = (hi - o) / dw
            near = np.minimum(t0, t1).max(-1)
            far = np.maximum(t0, t1).min(-1)
            hit = (near <= far) & (near > 1e-6)
            best = np.where(hit & (near < best), near, best)
    z = np.where(np.isfinite(best), best, 0.0) * scale
    z = np.where((z >= 1) & (z <= 65535), np.rint(z), 0)
    return z.astype(np.uint16)


def back_project(depth, camera, seed=1):
    """every pixel with depth as a float32 camera-frame point (row-major), every byte of the point set"""
    cx, cy, fx, fy, scale = (float(v) for v in camera)
    ys, xs = np.nonzero(depth)
    z = depth[ys, xs].astype(np.float64) / scale
    return CR.cloud(np.stack([(xs - cx) * z / fx, (ys - cy) * z / fy, z], -1), seed)


def make(scene, w, h, camera, T_true, planted, cloud_poses, **params):
    T_true = np.asarray(T_true, np.float64)
    clouds = [back_project(ray_cast(scene, Tc, camera, w, h), camera, seed=3 + i) for i, Tc in enumerate(cloud_poses)]
    return dict(depth=ray_cast(scene, T_true, camera, w, h), camera=camera, T_true=T_true, T_view=T_true @ np.asarray(planted, np.float64), clouds=clouds,
                T_clouds=[np.asarray(Tc, np.float64) for Tc in cloud_poses], params=params)


VIEW = se3(ry=-0.25, rx=-0.3, tx=0.2, ty=0.05, tz=0.3)          # looks down into the corner: all three planes and the box in sight
NEAR = [se3(ry=-0.2, rx=-0.28, tx=0.3, tz=0.2), se3(ry=-0.3, rx=-0.33, tx=0.1, ty=0.02, tz=0.45)]
SMALL = (33.2, 17.4, 48.0, 47.0, 1000.0)          # cx, cy, fx, fy, scale of the 67 x 35 cases
LOOSE = dict(min_inliers=50)
PLANTED = se3(rx=0.01, ry=-0.015, rz=0.008, tx=0.02, ty=-0.015, tz=0.025)


def cases():
    c = {}
    c["room_67x35"] = lambda: make(ROOM, 67, 35, SMALL, VIEW, PLANTED, NEAR, **LOOSE)
    c["room_67x35_stride3"] = lambda: make(ROOM, 67, 35, SMALL, VIEW, PLANTED, NEAR, stride=3, **LOOSE)
    # a tight band: most residuals of the planted error lie beyond delta, some beyond dist_max
    c["tail_and_far"] = lambda: make(ROOM, 67, 35, SMALL, VIEW, se3(tx=0.03, ty=0.02, tz=-0.04, ry=0.01), NEAR, dist_max=0.04, delta=0.01, max_iterations=4, **LOOSE)
    # clouds seen from well to the side: many of their points leave the view's image
    c["outside"] = lambda: make(ROOM, 67, 35, SMALL, VIEW, PLANTED, [se3(ry=0.35, rx=-0.3, tx=-0.6, tz=0.2), se3(ry=-0.7, rx=-0.1, tx=0.5, tz=0.8)], **LOOSE)
    # a mirrored camera (fx < 0): s.16 allows any finite focal length
    c["mirrored_fx"] = lambda: make(ROOM, 67, 35, (33.2, 17.4, -48.0, 47.0, 1000.0), VIEW, PLANTED, NEAR, **LOOSE)
    # a tighter edge gate: more of the box's silhouette and of the steep wall becomes invalid
    c["tight_gate"] = lambda: make(ROOM, 67, 35, SMALL, VIEW, PLANTED, NEAR, tol_abs=0.08, tol_rel_ppm=0, **LOOSE)
    # three clouds, the middle one empty; z range cuts the back wall off
    def three():
        cs = make(ROOM, 67, 35, SMALL, VIEW, PLANTED, NEAR + [se3(ry=-0.22, rx=-0.3, tx=0.25)], z_max=3.5, z_min=1.0, **LOOSE)
        cs["clouds"][1] = cs["clouds"][1][:0]
        return cs
    c["three_clouds_z_range"] = three
    c["empty_m0"] = lambda: dict(make(ROOM, 67, 35, SMALL, VIEW, np.eye(4), [], **LOOSE))
    def degenerate_points():
        cs = make(ROOM, 67, 35, SMALL, VIEW, PLANTED, NEAR[:1], **LOOSE)
        p = cs["clouds"][0]
        big, nan, inf = 1.0e30, float("nan"), float("inf")
        bad = CR.cloud([[nan, 0, 1], [0, inf, 1], [0, 0, -inf], [big, 0, 1], [0, 0, big], [3e38, 3e38, 3e38], [0, 0, 0], [0, 0, -1]], 9)
        cs["clouds"][0] = np.concatenate([bad[:4], p, bad[4:]])
        return cs
    c["degenerate_points"] = degenerate_points
    return c


# ---- the convergence scene: larger, several planted errors well inside dist_max
CONV_CAM = (80.3, 59.6, 140.0, 141.0, 1000.0)
CONV_PLANTED = {"small": se3(rx=0.004, ry=-0.006, rz=0.003, tx=0.01, ty=-0.008, tz=0.012),
                "medium": se3(rx=-0.012, ry=0.015, rz=-0.01, tx=-0.03, ty=0.025, tz=0.03),
                "large": se3(rx=0.02, ry=0.025, rz=0.015, tx=0.05, ty=-0.04, tz=-0.05)}


def convergence_case(name):
    return make(ROOM, 160, 120, CONV_CAM, VIEW, CONV_PLANTED[name], NEAR, max_iterations=20)
