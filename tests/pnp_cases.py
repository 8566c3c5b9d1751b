"""Named inputs for PnPSolver::solvePnP (include/ssm/pnp_core.h, oracle/pnp.c, tests/golden/pyref.py::pnp_solve, csrc/kernels_pnp.hip) and a census of the
solver paths they reach.  numpy only: the CPU comparison (test_pnp_cases.py) and the device comparison (test_gpu_pnp_paths.py) share this list, so that what the
device is shown to restate is known by name: every length of a Levenberg iteration's run of trials, both early terminations, every number of rounds, the
bookkeeping quirk and the fourth round with edges already out.

A case is (img n x 2 float32, obj n x 3 float32, T0 4 x 4, min_inliers).  FINITE cases run through all restatements; NONFINITE ones reach x / 0, inf - inf or NaN,
which is plain IEEE in the contract but raises in pyref's Python floats, so they are compared between the C oracle, the host class and the device only; SIZE
cases are too long for pyref."""
import collections
import os
import sys
import numpy as np
from test_pnp import CAM, _case, _pose, ROOT

if os.path.join(ROOT, "tests", "golden") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

Case = collections.namedtuple("Case", "name build reaches")      # reaches: the events (pyref.pnp_solve's `events`) the case is named for
MIN_INLIERS = 10                                                   # pnp_min_inliers of host/parameters_test.txt: the host program reads it from there
TGT = _pose(0.03, -0.05, 0.02, (0.04, -0.03, 0.06))               # the pose _case projects with
EVENTS = tuple("streak_%d" % k for k in range(1, 11)) + ("ten_trials", "tenth_trial_accepted", "gain_zero", "all_10_iterations", "rounds_1", "rounds_2", "rounds_3",
                                                         "rounds_4", "remarked_outlier", "robust_off_round_with_outliers")
NOT_REACHED = ("pivot_failed",)     # counted by pyref, reached by no finite case here: H + lambda I with lambda = 1e-5 max diag H keeps its pivots positive on finite data


def project(X, T):
    p = (T[:3, :3] @ np.asarray(X, np.float64).T).T + T[:3, 3]
    return np.stack([CAM[2] * p[:, 0] / p[:, 2] + CAM[0], CAM[3] * p[:, 1] / p[:, 2] + CAM[1]], 1)


def _box(rng, n):
    return np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(1.0, 4.0, n)], 1).astype(np.float32)


def _pack(uv, X, T0):
    return np.ascontiguousarray(uv, np.float32), np.ascontiguousarray(X, np.float32), np.asarray(T0, np.float64), MIN_INLIERS


def drawn(seed, n, outlier_every, zero_every, noise):
    """test_pnp._case with the start value rule of the existing tests: identity for odd seeds, near the answer for even ones"""
    def build():
        img, obj, _ = _case(seed, n, outlier_every, zero_every, noise)
        return _pack(img, obj, np.eye(4) if seed % 2 else _pose(0.01, 0.0, -0.01, (0.01, 0.0, 0.02)))
    return build


def _collinear():
    s = np.linspace(-1.0, 1.0, 30)
    X = (np.array([0.1, -0.2, 2.5]) + s[:, None] * np.array([0.8, 0.3, 0.5])).astype(np.float32)
    return _pack(project(X, TGT), X, np.eye(4))


def _identical():
    X = np.tile(np.array([[0.3, -0.2, 2.0]], np.float32), (40, 1))
    return _pack(project(X, TGT), X, np.eye(4))


def _far():
    rng = np.random.default_rng(31)
    X = _box(rng, 40); X[:, 2] += np.float32(1000.0)
    return _pack(project(X, TGT), X, np.eye(4))


def _scaled(s):
    def build():
        rng = np.random.default_rng(32)
        X = (_box(rng, 40).astype(np.float64) * s).astype(np.float32)
        T = TGT.copy(); T[:3, 3] *= s
        return _pack(project(X, T), X, np.eye(4))
    return build


def _planar():
    rng = np.random.default_rng(33)
    X = _box(rng, 60); X[:, 2] = np.float32(2.0)
    return _pack(project(X, TGT) + 1.0 * rng.standard_normal((60, 2)), X, np.eye(4))


def _random_pixels():
    rng = np.random.default_rng(34)
    X = _box(rng, 50)
    return _pack(np.stack([rng.uniform(0, 640, 50), rng.uniform(0, 480, 50)], 1), X, np.eye(4))


def _start(T0, seed=35, n=40):
    def build():
        rng = np.random.default_rng(seed)
        X = _box(rng, n)
        return _pack(project(X, TGT), X, T0)
    return build


def _few(n):
    def build():
        rng = np.random.default_rng(40 + n)
        X = _box(rng, n)
        return _pack(project(X, TGT), X, np.eye(4))
    return build


def _depth_on_4_of_60():
    rng = np.random.default_rng(36)
    X = _box(rng, 60); uv = project(X, TGT)
    keep = np.zeros(60, bool); keep[[5, 17, 18, 59]] = True
    X[~keep] = 0
    return _pack(uv, X, np.eye(4))


def _no_depth():
    rng = np.random.default_rng(37)
    X = _box(rng, 50); uv = project(X, TGT); X[:] = 0
    return _pack(uv, X, np.eye(4))


FINITE = [
    # seeded draws: chosen by a scan of seeds 100 .. 159 so that together they reach every event (test_pnp_cases.py::test_census proves it)
    Case("draw_101_ten_trials_three_rounds", drawn(101, 21, 5, 4, 0.5), ("ten_trials", "streak_10", "rounds_3", "remarked_outlier")),
    Case("draw_136_ten_trials_four_rounds", drawn(136, 36, 5, 4, 0.5), ("ten_trials", "rounds_4", "robust_off_round_with_outliers", "streak_4", "streak_5", "streak_7")),
    Case("draw_139_streaks_of_5", drawn(139, 26, 3, 7, 0.5), ("streak_5", "streak_2", "streak_3", "gain_zero", "rounds_3")),
    Case("draw_125_robust_off_with_outliers", drawn(125, 43, 5, 4, 1.0), ("robust_off_round_with_outliers", "rounds_4", "streak_8", "all_10_iterations")),
    Case("draw_105_streak_9", drawn(105, 63, 3, 7, 1.5), ("streak_9", "rounds_2", "remarked_outlier")),
    Case("draw_155_ten_trials_in_round_2", drawn(155, 30, 3, 7, 3.0), ("ten_trials", "rounds_2")),
    Case("draw_102_streaks_3_6_7_8", drawn(102, 30, 3, 7, 0.5), ("streak_3", "streak_6", "streak_7", "streak_8")),
    Case("draw_110_near_start", drawn(110, 33, 5, 2, 1.5), ("streak_5", "streak_7", "gain_zero")),
    # (found by a scan of seeds 100 .. 899 with the draw rule of the scan above: the one draw of 65 with ten_trials whose result changes when the limit is ignored)
    Case("draw_368_tenth_trial_accepted", drawn(368, 50, 3, 4, 1.0), ("ten_trials", "tenth_trial_accepted", "rounds_3")),
    # (the same from the identity start, so that the tracker's chain runs it too: odd seeds 901 .. 4499 gave ten such draws)
    Case("draw_2211_tenth_trial_accepted_twice", drawn(2211, 28, 5, 7, 1.0), ("ten_trials", "tenth_trial_accepted", "streak_9", "rounds_4", "robust_off_round_with_outliers")),
]
GEOMETRIC = [
    Case("collinear", _collinear, ("gain_zero", "rounds_4")),
    Case("identical_40", _identical, ("gain_zero",)),
    Case("far_1km", _far, ("all_10_iterations",)),
    Case("scaled_1e6", _scaled(1e6), ("rounds_2",)),
    Case("scaled_1e-6", _scaled(1e-6), ("rounds_1",)),
    Case("planar_noise_1px", _planar, ("streak_10", "ten_trials", "robust_off_round_with_outliers")),
    Case("random_pixels", _random_pixels, ("rounds_1",)),
    Case("start_rotated_1rad", _start(_pose(0.0, 1.0, 0.0, (0.0, 0.0, 0.0))), ("rounds_1",)),
    Case("start_rotated_3.1rad", _start(_pose(0.0, 0.0, 3.1, (0.0, 0.0, 0.0))), ("rounds_1",)),
    Case("start_6m_behind", _start(_pose(0.0, 0.0, 0.0, (0.0, 0.0, -8.0))), ("rounds_1",)),
    Case("exact_at_solution", _start(TGT), ("gain_zero", "streak_7")),
] + [Case("edges_%d" % n, _few(n), ("rounds_1",) if n < 5 else ("rounds_4",)) for n in range(1, 7)] + [
    Case("depth_on_4_of_60", _depth_on_4_of_60, ("rounds_1", "streak_9")),
    Case("no_depth_50", _no_depth, ("rounds_1",)),
]


# The pixels of these cases are the projections at the START pose, so the sound edges begin (and, when no step is ever accepted, stay) as inliers and the flag
# list shows what the solver decided about the one edge that is not sound.
def _with_edge(X_edge, seed=50):
    def build():
        rng = np.random.default_rng(seed)
        X = _box(rng, 24); uv = project(X, np.eye(4)) + 0.3 * rng.standard_normal((24, 2))
        X[7] = X_edge
        return _pack(uv, X, np.eye(4))
    return build


def _z0_at_start():
    rng = np.random.default_rng(51)
    X = _box(rng, 24); X[:, 2] += np.float32(3.0); X[7, 2] = np.float32(2.0)      # R = I, t_z = -2: 0 x + 0 y + 1 * 2 + (-2) is exactly 0
    T0 = _pose(0.0, 0.0, 0.0, (0.0, 0.0, -2.0))
    uv = project(X[np.arange(24) != 7], T0) + 0.3 * rng.standard_normal((23, 2))
    return _pack(np.insert(uv, 7, (300.0, 200.0), 0), X, T0)


def _times_1e30():
    rng = np.random.default_rng(52)
    X = _box(rng, 24); uv = project(X, TGT)
    return _pack(uv, X.astype(np.float64) * 1e30, np.eye(4))


def _inf_pixel():
    rng = np.random.default_rng(53)
    X = _box(rng, 24); uv = project(X, np.eye(4)) + 0.3 * rng.standard_normal((24, 2)); uv[11, 0] = np.inf
    return _pack(uv, X, np.eye(4))


NONFINITE = [
    Case("z0_under_identity", _with_edge((1.0, 1.0, 0.0)), ()),
    Case("z0_at_start_pose", _z0_at_start, ()),
    Case("huge_over_tiny", _with_edge((1e19, 1e19, 1e-19)), ()),
    Case("points_times_1e30", _times_1e30, ()),
    Case("nan_coordinate", _with_edge((0.5, np.nan, 2.0)), ()),
    Case("inf_pixel", _inf_pixel, ()),
]


def _size(n, zero_every):
    def build():
        img, obj, _ = _case(60, n, 9, zero_every, 0.4)
        return _pack(img, obj, np.eye(4))
    return build


SIZE = [Case("n65535", _size(65535, 0), ()), Case("n65535_depthless_rows", _size(65535, 7), ())]


def sized(n):
    """a draw of n correspondences, every one with depth (for the sizes around the LDS capacity of the device's edge list)"""
    return Case("n%d" % n, _size(n, 0), ())


WRAP = Case("draw_201_12_points", drawn(201, 12, 4, 0, 0.5), ())      # the short solve that is repeated until the device's pass numbers wrap


def same_pose(a, b):
    """equal bytes, or NaN in the same entries (IEEE leaves a NaN's sign and payload open)"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


_built = {}


def get(case):
    """the case's arrays, built once; callers do not modify them"""
    if case.name not in _built:
        img, obj, T0, mi = case.build()
        img.setflags(write=False); obj.setflags(write=False); T0.setflags(write=False)
        _built[case.name] = (img, obj, T0, mi)
    return _built[case.name]


def padded(case, n=9000):
    """the case followed by depth-less rows up to n: the pose and the leading flags do not change (a passing edge marks its POSITION, which is below the
    number of edges), and the device keeps an edge list of that length in global memory instead of LDS"""
    img, obj, T0, mi = get(case)
    k = n - len(img)
    assert k > 0
    return np.concatenate([img, np.full((k, 2), 100.0, np.float32)]), np.concatenate([obj, np.zeros((k, 3), np.float32)]), T0, mi


_pyref = {}


def pyref_result(case):
    """(ok, T, inliers, events) of the Python restatement, computed once per case"""
    if case.name not in _pyref:
        import pyref
        img, obj, T0, mi = get(case)
        ev = {}
        ok, T, inl = pyref.pnp_solve(img, obj, CAM, T0, min_inliers=mi, events=ev)
        _pyref[case.name] = (ok, T, inl, ev)
    return _pyref[case.name]


def census(cases):
    tot = collections.Counter()
    for c in cases:
        tot.update(pyref_result(c)[3])
    return tot
