"""GPU tests of the route field: through ssm_debug_route_cells the device must equal ssm_route_cells_host and ssm_route_path_host byte for byte --
cost, parent, every info field, the path and its info -- in BOTH forms (sweeps; active tiles) and under both `moves`: on the shared cases of tests/route_cases.py, at
grid sizes around the 32 x 32 tile, on the longest legal sides, at 512 x 512 and on a 129 x 129 serpentine, a small call after a large one into one target, several
goals against one field, max_path, on a built grid after ssm_clearance_grid (which the route call leaves as it was), and every refusal.  The host functions themselves
are checked against the restatement in tests/test_route.py."""
import os
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import route_cases as RC  # noqa: E402
import clearance_cases as CC  # noqa: E402
import objects_cases as OC  # noqa: E402
from conftest import CAM  # noqa: E402

pytestmark = pytest.mark.gpu
FORMS = [0, 1]       # sweeps of one thread per cell in batches; active tiles relaxed to their fixed points
_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


class Ctx:
    """a context and its route targets, one per size and max_path"""
    def __init__(self):
        import semantic_slam_mapping_amd as ssm
        self.c = ssm.Context(0, width=640, height=480, orb_features=500, max_batch=1, voxel_capacity_log2=12, camera=CAM)
        self.targets = {}

    def target(self, nx, ny, max_path=None):
        max_path = nx * ny if max_path is None else max_path
        if (nx, ny, max_path) not in self.targets:
            self.targets[(nx, ny, max_path)] = self.c.route_target(nx, ny, max_path)
        return self.targets[(nx, ny, max_path)]

    def close(self):
        for t in self.targets.values():
            self.c.route_target_free(t)
        self.c.close()


@pytest.fixture(scope="module")
def g():
    x = Ctx()
    yield x
    x.close()


@pytest.fixture
def form(request, g):
    g.c.route_form(request.param)
    yield request.param
    g.c.route_form(-1)


def host_field(cs, **kw):
    import semantic_slam_mapping_amd as ssm
    return ssm.route_cells_host(cs["reach"], cs["dist2"], cs["source"], **dict(cs["params"], **kw))


def equal(got, want, what):
    for name, a, b, t in zip(("cost", "parent"), got, want[:2], (np.uint32, np.int32)):
        assert a.dtype == b.dtype == t and a.shape == b.shape, (what, name, a.dtype, a.shape, b.shape)
        bad = np.argwhere(a != b)
        assert len(bad) == 0, (what, name, len(bad), bad[:4].tolist(), [int(a[tuple(i)]) for i in bad[:4]], [int(b[tuple(i)]) for i in bad[:4]])
        assert a.tobytes() == b.tobytes()


def device_equals_host(g, cs, target, what, want=None, goals=None, **kw):
    """the device on the case's images == the host functions (the field computed once per case and parameters where the caller keeps it), every goal of the case
    against that one field -> the host's field"""
    import semantic_slam_mapping_amd as ssm
    params = dict(cs["params"], **kw)
    if want is None:
        want = ssm.route_cells_host(cs["reach"], cs["dist2"], cs["source"], **params)
    info = g.c.route_cells(target, cs["reach"], cs["dist2"], cs["source"], **params)
    assert info == want[2], (what, info, want[2])
    assert g.c.route_rounds() >= 1 if info["routed"] else g.c.route_rounds() == 0, (what, g.c.route_rounds())
    equal(g.c.route_fetch(target), want, what)
    for gl in (cs["goals"] if goals is None else goals):
        a = g.c.route_path(target, gl["goal"], gl["snap"])
        b = ssm.route_path_host(want[0], want[1], cs["dist2"], gl["goal"], gl["snap"], **params)
        assert a[0].dtype == np.int32 and np.array_equal(a[0], b[0]) and a[1] == b[1], (what, gl, a[1], b[1])
    return want


@pytest.mark.parametrize("form", FORMS, indirect=True)
@pytest.mark.parametrize("name", list(RC.cases()))
def test_cases(g, name, form):
    cs = RC.cases()[name]()
    ny, nx = cs["reach"].shape
    for moves in (4, 8):
        want = memo((name, moves), lambda: host_field(cs, moves=moves))
        device_equals_host(g, cs, g.target(nx, ny), (name, moves, form), want, moves=moves)
    info = g.c.route_cells(g.target(nx, ny), cs["reach"], cs["dist2"], cs["source"], **cs["params"])
    for k, v in cs["want"].get("info", {}).items():
        assert info[k] == v, (name, k, info[k], v)
    for gl in cs["goals"]:
        pi = g.c.route_path(g.target(nx, ny), gl["goal"], gl["snap"])[1]
        for k, v in gl.get("want", {}).items():
            assert pi[k] == v, (name, gl["goal"], k, pi[k], v)


@pytest.mark.parametrize("form", FORMS, indirect=True)
@pytest.mark.parametrize("shape", CC.SHAPES + RC.EXTRA_SHAPES, ids=lambda s: "%dx%d" % s)
def test_sizes(g, shape, form):
    """around the 32 x 32 tile, one cell wide and one cell high: one target for every fill of a shape"""
    nx, ny = shape
    target = g.target(nx, ny)
    for fraction in RC.FILLS:
        cs = memo(("fill", shape, fraction), lambda: RC.random_fill(nx, ny, fraction, nx * 7 + ny))
        for moves in (4, 8):
            want = memo(("fill", shape, fraction, moves), lambda: host_field(cs, moves=moves))
            device_equals_host(g, cs, target, (shape, fraction, moves, form), want, moves=moves)


@pytest.mark.parametrize("form", FORMS, indirect=True)
@pytest.mark.parametrize("shape", [(32768, 1), (1, 32768)], ids=lambda s: "%dx%d" % s)
def test_longest_sides(g, shape, form):
    """open from end to end: 327670 at the far end, a path of 32768 cells"""
    nx, ny = shape
    r, d = RC.field(nx, ny)
    cs = RC.case(r, d, (0, 0), goals=[dict(goal=(nx - 1, ny - 1), snap=0), dict(goal=(nx // 2, ny // 2), snap=5)])
    want = memo(("long", shape), lambda: host_field(cs))
    device_equals_host(g, cs, g.target(nx, ny), (shape, form), want)
    assert int(want[0].ravel()[-1]) == 327670 and want[2]["far_cell"] == 32767
    cells, pi = g.c.route_path(g.target(nx, ny), (nx - 1, ny - 1), 0)
    assert pi["len"] == 32768 and pi["cost"] == 327670 and np.array_equal(cells, np.arange(32768))


FILLS_512 = [("open", 0.0), ("5%", 0.05), ("30%", 0.3)]


@pytest.mark.parametrize("form", FORMS, indirect=True)
@pytest.mark.parametrize("name,fraction", FILLS_512, ids=[n for n, _ in FILLS_512])
def test_512(g, name, fraction, form):
    cs = memo(("512", name), lambda: RC.random_fill(512, 512, fraction, 20 + int(fraction * 100), comfort=1.5))
    want = memo(("512 host", name), lambda: host_field(cs))
    device_equals_host(g, cs, g.target(512, 512), (name, form), want)
    assert want[2]["routed"] > 100000 and want[2]["near_cells"] > 0
    if name == "30%":
        want4 = memo(("512 host 4", name), lambda: host_field(cs, moves=4))
        device_equals_host(g, cs, g.target(512, 512), (name, form, 4), want4, moves=4)
        # (a diagonal move needs both cells beside it, so whatever 8 moves reach, 4 moves reach too: the same cells, dearer)
        assert 0 < want4[2]["unrouted"] == want[2]["unrouted"] and want4[2]["routed"] == want[2]["routed"] and want4[2]["max_cost"] > want[2]["max_cost"]


@pytest.mark.parametrize("form", FORMS, indirect=True)
def test_serpentine_129(g, form):
    """the worst case of both forms in small: one way through every cell of 65 rows, 5 x 5 tiles"""
    cs = memo("serpentine 129", lambda: RC.serpentine(129))
    want = memo("serpentine 129 host", lambda: host_field(cs))
    device_equals_host(g, cs, g.target(129, 129), ("serpentine", form), want)
    for k, v in cs["want"]["info"].items():
        assert want[2][k] == v, (k, want[2][k], v)
    assert want[2]["max_cost"] == 10 * (65 * 128 + 64 * 2)


@pytest.mark.parametrize("form", FORMS, indirect=True)
def test_small_call_after_a_large_one(g, form):
    """a second, smaller call into one target leaves nothing of the first; another shape of as many cells; and the large one again"""
    target = g.target(131, 97)
    big = RC.random_fill(131, 97, 0.2, 9)
    small = RC.random_fill(7, 5, 0.2, 8)
    n_big = device_equals_host(g, big, target, "large")[2]["routed"]
    n_small = device_equals_host(g, small, target, "small")[2]["routed"]
    assert n_big > 10 * n_small > 0
    device_equals_host(g, RC.no_seed(), target, "no seed")
    device_equals_host(g, RC.random_fill(97, 131, 0.2, 10), target, "transposed")
    device_equals_host(g, big, target, "large again")


def test_several_goals_against_one_field(g):
    """one field, many goals: each path is the host's, and none disturbs the field"""
    import semantic_slam_mapping_amd as ssm
    cs = RC.random_fill(97, 61, 0.25, 5)
    rng = np.random.default_rng(6)
    goals = [dict(goal=(int(x), int(y)), snap=int(s)) for x, y, s in zip(rng.integers(0, 97, 24), rng.integers(0, 61, 24), rng.integers(0, 9, 24))]
    target = g.target(97, 61)
    want = device_equals_host(g, cs, target, "goals", goals=goals)
    equal(g.c.route_fetch(target), want, "after the goals")
    found = [ssm.route_path_host(want[0], want[1], cs["dist2"], gl["goal"], gl["snap"], **cs["params"])[1]["len"] for gl in goals]
    assert sum(1 for n in found if n > 0) >= 12 and sum(1 for n in found if n == 0) >= 1


def test_max_path(g):
    """a path of exactly max_path cells is written; one cell more is SSM_E_CAPACITY with the length needed"""
    import semantic_slam_mapping_amd as ssm
    cs = RC.row_of_ten()
    fits, short = g.target(10, 1, 10), g.target(10, 1, 9)
    g.c.route_cells(fits, cs["reach"], cs["dist2"], cs["source"])
    cells, info = g.c.route_path(fits, (9, 0))
    assert info["len"] == 10 and cells.tolist() == list(range(10))
    g.c.route_cells(short, cs["reach"], cs["dist2"], cs["source"])
    with pytest.raises(ssm.SsmError) as e:
        g.c.route_path(short, (9, 0))
    assert e.value.code == -4 and e.value.info["len"] == 10 and e.value.info["cost"] == 90 and "max_path" in str(e.value)
    cells, info = g.c.route_path(short, (8, 0))          # the target goes on
    assert info["len"] == 9 and cells.tolist() == list(range(9))


@pytest.mark.parametrize("form", FORMS, indirect=True)
def test_built_grid(g, form):
    """ssm_grid_points on the shared street scene, ssm_clearance_grid, then ssm_route_field == the host function on ssm_clearance_fetch's reach and dist2 from the
    clearance call's seed (the cell size the grid's); the clearance and grid targets are as they were, and the field outlives a second clearance call"""
    import semantic_slam_mapping_amd as ssm
    c = g.c
    cs = memo("street_m3", OC.cloud_cases()["street_m3"])
    G = cs["grid"]
    gt, ct, rt = c.grid_target(G["nx"], G["ny"]), c.clearance_target(G["nx"], G["ny"]), g.target(G["nx"], G["ny"])
    try:
        built = c.grid_points(gt, cs["clouds"], cs["T_clouds"], **G)
        cell = ssm.grid_params(**G).cell
        for cp in (dict(radius=cell * 1.5, seed=(G["nx"] // 2, 1), seed_snap=20), dict(radius=0.0, connectivity=8, blocked=[4, 0], free=[1, 2, 3], seed=(0, 0), seed_snap=1024)):
            cinfo = c.clearance_grid(gt, ct, **cp)
            d2, near, reach = c.clearance_fetch(ct)
            assert cinfo["seed_cell"] >= 0 and cinfo["reachable"] > 10
            for rp in (dict(comfort=cell * 3, near_weight=4), dict(moves=4, comfort=0.0)):
                want = ssm.route_cells_host(reach, d2, cinfo["seed_cell"], cell=cell, **rp)
                info = c.route_field(ct, rt, cell=123.0, **rp)          # (the parameters' own cell size plays no part after a clearance call)
                assert info == want[2] and info["routed"] + info["unrouted"] == cinfo["reachable"] and info["source_cell"] == cinfo["seed_cell"], (info, want[2], cinfo)
                equal(c.route_fetch(rt), want, ("built grid", cp, rp))
                far = (info["far_cell"] % G["nx"], info["far_cell"] // G["nx"])
                a = c.route_path(rt, far, 0); b = ssm.route_path_host(want[0], want[1], d2, far, 0, cell=cell, **rp)
                assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[1]["cost"] == info["max_cost"]
            after = c.clearance_fetch(ct)
            assert all(np.array_equal(x, y) for x, y in zip(after, (d2, near, reach)))
        again = c.grid_fetch(gt)
        assert all(np.array_equal(again[k], built[k]) for k in again)
        # the route target keeps what a path needs: another clearance call on the same target does not change the path
        c.clearance_grid(gt, ct, radius=cell * 1.5, seed=(G["nx"] // 2, 1), seed_snap=20)
        a2 = c.route_path(rt, far, 0)
        assert np.array_equal(a2[0], a[0]) and a2[1] == a[1]
    finally:
        c.clearance_target_free(ct); c.grid_target_free(gt)


def test_refusals_on_the_device(g):
    import semantic_slam_mapping_amd as ssm
    c = g.c
    cs = RC.goal_snaps()          # 9 x 5
    t = g.target(9, 5)
    args = (cs["reach"], cs["dist2"], cs["source"])

    def refused(call, word=None):
        with pytest.raises(ssm.SsmError) as e:
            call()
        assert e.value.code == -1 and (word is None or word in str(e.value)), (str(e.value), word)

    fresh_c, fresh_t, small = c.clearance_target(9, 5), c.route_target(9, 5), c.route_target(4, 4)
    other = Ctx()          # a second context on the same GPU
    try:
        refused(lambda: c.route_field(fresh_c, t), "no call has run on the clearance target")
        refused(lambda: c.route_path(fresh_t, (0, 0)), "no field")
        refused(lambda: c.route_fetch(fresh_t), "no field")
        refused(lambda: c.route_fetch(fresh_t, shape=(9, 5)), "no field")
        nan, inf = float("nan"), float("inf")
        bad = (dict(moves=6), dict(moves=0), dict(near_weight=-1), dict(near_weight=9), dict(comfort=-0.1), dict(comfort=nan), dict(comfort=inf), dict(cell=0.0), dict(cell=nan), dict(cell=inf))
        for kw in bad:
            refused(lambda: c.route_cells(t, *args, **kw), "route:")
        refused(lambda: c.route_cells(None, *args), "null")
        refused(lambda: c.route_cells(small, *args), "more cells")
        refused(lambda: c.route_cells(t, cs["reach"], cs["dist2"], (4, 2)), "source")
        refused(lambda: c.route_cells(t, cs["reach"], cs["dist2"], 45), "source")
        refused(lambda: c.route_cells(other.target(9, 5), *args), "another context")
        refused(lambda: other.c.route_cells(t, *args), "another context")
        r = np.ascontiguousarray(cs["reach"]); d = np.ascontiguousarray(cs["dist2"])
        assert c.lib.ssm_debug_route_cells(c.h, t, None, d.ctypes.data, 9, 5, 0, None, None) == -1 and c.lib.ssm_last_error(c.h).decode() == "null argument"
        assert c.lib.ssm_debug_route_cells(c.h, t, r.ctypes.data, None, 9, 5, 0, None, None) == -1 and c.lib.ssm_last_error(c.h).decode() == "null argument"
        assert c.lib.ssm_route_target_create(c.h, 9, 5, 10, None) == -1
        for nx, ny in ((0, 5), (9, 0), (-1, 5)):
            assert c.lib.ssm_debug_route_cells(c.h, t, r.ctypes.data, d.ctypes.data, nx, ny, 0, None, None) == -1
        big = g.target(32768, 1)
        for nx, ny in ((32769, 1), (1, 32769)):          # (the host arrays are not read: the sides are refused first)
            assert c.lib.ssm_debug_route_cells(c.h, big, r.ctypes.data, d.ctypes.data, nx, ny, 0, None, None) == -1 and "32768" in c.lib.ssm_last_error(c.h).decode()
        for nx, ny in ((0, 5), (9, 0), (4097, 4096)):
            refused(lambda: c.route_target(nx, ny), "2^24")
        for mp in (0, -1):
            refused(lambda: c.route_target(9, 5, mp), "max_path")
        # a field and its path queries
        c.route_cells(t, *args)
        for goal, snap, word in (((9, 0), 0, "goal"), ((0, 5), 0, "goal"), ((-1, 0), 0, "goal"), ((0, -1), 0, "goal"), ((0, 0), -1, "goal_snap"), ((0, 0), 1025, "goal_snap")):
            refused(lambda: c.route_path(t, goal, snap), word)
        refused(lambda: c.route_path(None, (0, 0)), "null")
        refused(lambda: other.c.route_path(t, (0, 0)), "another context")
        cells = np.zeros(45, np.int32)
        assert c.lib.ssm_route_path(c.h, t, 0, 0, 0, None, None) == -1 and c.lib.ssm_last_error(c.h).decode() == "null argument"
        assert c.lib.ssm_route_path(c.h, t, 0, 0, 0, cells.ctypes.data, None) == -1
        assert other.c.lib.ssm_route_fetch(other.c.h, t, None, None) == -1 and "another context" in other.c.lib.ssm_last_error(other.c.h).decode()
        assert c.lib.ssm_route_fetch(c.h, t, None, None) == 0          # every output is optional
        # after a clearance call: a route target smaller than the grid, of another context; a clearance target of another context
        cc = CC.corridor_open()
        ct = c.clearance_target(15, 21)
        try:
            c.clearance_cells(ct, cc["cls"], **cc["params"])
            refused(lambda: c.route_field(ct, small), "more cells")
            refused(lambda: c.route_field(ct, None), "null")
            refused(lambda: c.route_field(None, t), "null")
            rt = g.target(15, 21)
            refused(lambda: c.route_field(ct, other.target(15, 21)), "another context")
            other.c._clearance_sizes = {ct: (15, 21)}
            refused(lambda: other.c.route_field(ct, other.target(15, 21)), "another context")
            refused(lambda: c.route_field(ct, rt, moves=5), "moves")
            refused(lambda: c.route_field(ct, rt, comfort=-1.0), "comfort")
            info = c.route_field(ct, rt)
            assert info["routed"] > 0 and info["source_cell"] == 2 * 15 + 7
        finally:
            c.clearance_target_free(ct)
        for f in (-2, 2):
            refused(lambda: c.route_form(f), "form")
    finally:
        c.clearance_target_free(fresh_c); c.route_target_free(fresh_t); c.route_target_free(small); other.close()
    device_equals_host(g, cs, t, "the context goes on")
