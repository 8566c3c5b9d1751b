"""CPU tests of the route field: ssm_route_cells_host and ssm_route_path_host -- the contract's arithmetic of include/ssm/route_core.h, one thread,
no GPU, Dijkstra with a bucket queue -- against the restatement tests/route_ref.py (an explicit edge list and scipy's Dijkstra, parents by brute force) byte for byte
(cost, parent, every info field, the path and its info) on the shared cases of tests/route_cases.py and on random fills at the clearance tests' shapes, under both
`moves`; the cases' own claims; path properties; the field over a real clearance map; refusals; comfort2; the host functions as stand-alone C++ programs, also under
AddressSanitizer + UndefinedBehaviorSanitizer; and the new kernels' register use."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import route_ref as R  # noqa: E402
import route_cases as RC  # noqa: E402
import clearance_cases as CC  # noqa: E402

HOST = os.path.join(ROOT, "semantic_slam_mapping_amd", "host")
NONE = RC.NONE


def host(cs, **kw):
    import semantic_slam_mapping_amd as ssm
    return ssm.route_cells_host(cs["reach"], cs["dist2"], cs["source"], **dict(cs["params"], **kw))


def ref(cs, **kw):
    return R.run(cs["reach"], cs["dist2"], cs["source"], **dict(cs["params"], **kw))


def equal(got, want, what):
    for name, g, w, t in zip(("cost", "parent"), got[:2], want[:2], (np.uint32, np.int32)):
        assert g.dtype == w.dtype == t and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:4].tolist(), [int(g[tuple(b)]) for b in bad[:4]], [int(w[tuple(b)]) for b in bad[:4]])
        assert g.tobytes() == w.tobytes()
    assert got[2] == want[2], (what, got[2], want[2])


def paths_equal(cs, got, want, what, **kw):
    """every goal of the case: the host's path on the host's field == the restatement's on its own"""
    import semantic_slam_mapping_amd as ssm
    params = dict(cs["params"], **kw)
    for g in cs["goals"]:
        a = ssm.route_path_host(got[0], got[1], cs["dist2"], g["goal"], g["snap"], **params)
        b = R.path(want[0], want[1], cs["dist2"], g["goal"], g["snap"], **params)
        assert a[0].dtype == np.int32 and np.array_equal(a[0], b[0]) and a[1] == b[1], (what, g, a[1], b[1])
        R.check_path(a[0], a[1], cs["reach"], cs["dist2"], cs["source"], **params)


def check_want(cs, out, what):
    """the facts a case knows about itself, on what the library gave"""
    cost, parent, info = out
    want = cs["want"]
    for k, v in want.get("info", {}).items():
        assert info[k] == v, (what, k, info[k], v)
    if "cost_all" in want:
        assert (cost == want["cost_all"]).all(), what
    if "parent_all" in want:
        assert (parent == want["parent_all"]).all(), what
    if "cost" in want:
        assert np.array_equal(cost, want["cost"]), what
    for (cx, cy), v in want.get("cost_at", []):
        assert int(cost[cy, cx]) == v, (what, cx, cy, int(cost[cy, cx]), v)
    for (cx, cy), v in want.get("parent_at", []):
        assert int(parent[cy, cx]) == v, (what, cx, cy, int(parent[cy, cx]), v)


def check_goals(cs, path_of, what):
    """the facts a case knows about its goals; path_of(goal, snap) -> (cells, path info)"""
    for g in cs["goals"]:
        cells, info = path_of(g["goal"], g["snap"])
        for k, v in g.get("want", {}).items():
            assert info[k] == v, (what, g["goal"], g["snap"], k, info[k], v)
        R.check_path(cells, info, cs["reach"], cs["dist2"], cs["source"], **cs["params"])
        if cs["want"].get("corridor"):
            nx = cs["reach"].shape[1]
            rows = cells // nx
            assert (rows != 1).any() and set(rows[rows != 1].tolist()) == {0}, (what, cells.tolist())          # it leaves the middle row through row 0, never row 2


def test_layouts_and_defaults():
    import semantic_slam_mapping_amd as ssm
    from semantic_slam_mapping_amd._lib import RouteParams, RouteInfo, RoutePathInfo
    assert C.sizeof(RouteInfo) == 64 and C.sizeof(RoutePathInfo) == 56 and C.sizeof(RouteParams) == 24
    P = ssm.route_params()
    assert [getattr(P, k) for k in R.DEFAULTS] == list(R.DEFAULTS.values()) and (P.moves, P.near_weight, P.comfort, P.cell) == (8, 2, 2.0, 1.0)
    with pytest.raises(TypeError):
        ssm.route_params(move=4)
    lib = ssm.load()
    assert lib.ssm_debug_route_tile() == 32 and lib.ssm_debug_route_batch() >= 1


@pytest.mark.parametrize("name", list(RC.cases()))
def test_host_equals_restatement_on_the_cases(name):
    import semantic_slam_mapping_amd as ssm
    cs = RC.cases()[name]()
    assert cs["reach"].shape[0] <= 65 and cs["reach"].shape[1] <= 65
    for moves in (4, 8):
        got, want = host(cs, moves=moves), ref(cs, moves=moves)
        equal(got, want, (name, moves))
        paths_equal(cs, got, want, (name, moves), moves=moves)
    out = host(cs)
    check_want(cs, out, name)
    check_goals(cs, lambda goal, snap: ssm.route_path_host(out[0], out[1], cs["dist2"], goal, snap, **cs["params"]), name)


@pytest.mark.parametrize("shape", [s for s in CC.SHAPES + RC.EXTRA_SHAPES if s[0] * s[1] <= 65 * 65], ids=lambda s: "%dx%d" % s)
def test_host_equals_restatement_at_the_shapes(shape):
    nx, ny = shape
    for fraction in RC.FILLS:
        cs = RC.random_fill(nx, ny, fraction, nx * 7 + ny)
        for moves in (4, 8):
            got, want = host(cs, moves=moves), ref(cs, moves=moves)
            equal(got, want, (shape, fraction, moves))
            paths_equal(cs, got, want, (shape, fraction, moves), moves=moves)


def test_cases_are_what_they_are_for():
    """the properties the cases are for, on what the LIBRARY gives"""
    import semantic_slam_mapping_amd as ssm
    K = RC.cases()
    # every NEAR cell costs: with the weight raised the corridor's way is 8 dearer, and no dearer however high the weight -- it avoids every NEAR cell
    costs = [int(host(K["corridor_weight_%d" % w]())[0][1, 20]) for w in (0, 1, 8)]
    assert costs == [200, 208, 208]
    p = host(K["pillar"]())
    assert p[0][3, 1] == p[0][3, 3] == 30 and p[1][3, 2] == 16          # two ways of one cost: the lower index
    g = K["diagonal_gap"]()
    out = host(g)
    assert out[2]["unrouted"] == 28 and (out[0][5:] == NONE).all() and (out[1][5:] == -1).all()
    # the same from a real clearance map under 8-connectivity: the component holds both rooms, the route only the seed's
    cg = CC.diagonal_gap()
    d2, _, reach, cinfo = ssm.clearance_cells_host(cg["cls"], **dict(cg["params"], connectivity=8))
    assert cinfo["components"] == 1 and cinfo["reachable"] == 56
    f = ssm.route_cells_host(reach, d2, cinfo["seed_cell"], comfort=0.0)
    assert f[2]["routed"] == 28 and f[2]["unrouted"] == 28 and f[2]["routed"] + f[2]["unrouted"] == cinfo["reachable"]
    f4 = ssm.route_cells_host(*ssm.clearance_cells_host(cg["cls"], **dict(cg["params"], connectivity=4))[2::-2], source=cinfo["seed_cell"], comfort=0.0)
    assert f4[2]["unrouted"] == 0 and f4[2]["routed"] == 28          # under 4-connectivity the clearance map itself stops at the gap
    s = host(K["serpentine"]())
    assert s[2]["max_cost"] == 21760
    for name in K:
        cs = K[name]()
        cost, parent, info = host(cs)
        inn = cs["reach"] == 2
        assert ((cost != NONE) <= inn).all() and info["routed"] + info["unrouted"] == int(inn.sum()) and info["routed"] == int((cost != NONE).sum())
        assert ((parent >= 0) == ((cost != NONE) & (cost != 0))).all()
        if info["routed"]:
            ny, nx = cost.shape
            rc = np.flatnonzero((parent >= 0).ravel())
            assert (cost.ravel()[parent.ravel()[rc]] < cost.ravel()[rc]).all()          # costs strictly fall along parents
            assert info["max_cost"] == int(cost[cost != NONE].max()) and int(cost.ravel()[info["far_cell"]]) == info["max_cost"]
            assert int(cost.ravel()[info["source_cell"]]) == 0 and int((cost == 0).sum()) == 1


def test_comfort2():
    """comfort2 = floor((comfort / cell)^2), saturated at 2^31"""
    cs = RC.row_of_ten()
    for comfort, cell, want in ((0.0, 1.0, 0), (2.0, 1.0, 4), (1.999, 1.0, 3), (0.2, 0.2, 1), (0.1999, 0.2, 0), (1.0, 0.2, 25), (3.0, 1.5, 4), (1e9, 1.0, 1 << 31), (46340.95, 1.0, 2147483646),
                               (46341.0, 1.0, 1 << 31), (1e300, 1e-300, 1 << 31)):
        info = host(cs, comfort=comfort, cell=cell)[2]
        assert info["comfort2"] == want == R.comfort2_of(comfort, cell), (comfort, cell, info["comfort2"], want)
    r, d = RC.field(10, 1); d[0, 3] = 4; d[0, 4] = 5; d[0, 5] = NONE
    near = lambda **kw: __import__("semantic_slam_mapping_amd").route_cells_host(r, d, 0, **kw)[2]["near_cells"]  # noqa: E731
    assert near(comfort=2.0) == 1 and near(comfort=2.3) == 2 and near(comfort=1e9) == 9 and near(comfort=110.0) == 9          # a cell exactly comfort away is NEAR; "nothing blocked" never is


def test_max_path():
    """a path of exactly max_path cells is written; one cell more is SSM_E_CAPACITY with the length needed and no cell written"""
    import semantic_slam_mapping_amd as ssm
    from semantic_slam_mapping_amd._lib import RoutePathInfo
    cs = RC.row_of_ten()
    cost, parent, _ = host(cs)
    cells, info = ssm.route_path_host(cost, parent, cs["dist2"], (9, 0), max_path=10)
    assert info["len"] == 10 and cells.tolist() == list(range(10))
    with pytest.raises(ssm.SsmError) as e:
        ssm.route_path_host(cost, parent, cs["dist2"], (9, 0), max_path=9)
    assert e.value.code == -4 and e.value.info["len"] == 10 and e.value.info["cost"] == 90 and "max_path" in str(e.value)
    lib = ssm.load()
    out = np.full(12, -7, np.int32); I = RoutePathInfo(); P = ssm.route_params()
    assert lib.ssm_route_path_host(cost.ctypes.data, parent.ctypes.data, cs["dist2"].ctypes.data, 10, 1, C.byref(P), 9, 0, 0, 9, out.ctypes.data, C.byref(I)) == -4 and (out == -7).all()
    assert lib.ssm_route_path_host(cost.ctypes.data, parent.ctypes.data, cs["dist2"].ctypes.data, 10, 1, C.byref(P), 4, 0, 0, 5, out.ctypes.data, C.byref(I)) == 0
    assert out.tolist() == [0, 1, 2, 3, 4] + [-7] * 7 and I.len == 5
    assert lib.ssm_route_path_host(cost.ctypes.data, parent.ctypes.data, cs["dist2"].ctypes.data, 10, 1, None, 9, 0, 0, 1, None, C.byref(I)) == -4 and I.len == 10          # only the info


def test_refusals():
    import semantic_slam_mapping_amd as ssm
    from semantic_slam_mapping_amd._lib import RouteInfo, RoutePathInfo
    lib = ssm.load()
    cs = RC.goal_snaps()          # 9 x 5, column 4 takes no part below row 0
    nan, inf = float("nan"), float("inf")
    bad = (dict(moves=6), dict(moves=0), dict(moves=-8), dict(near_weight=-1), dict(near_weight=9), dict(comfort=-0.1), dict(comfort=nan), dict(comfort=inf), dict(cell=0.0), dict(cell=-1.0),
           dict(cell=nan), dict(cell=inf))
    for kw in bad:
        with pytest.raises(ssm.SsmError) as e:
            host(cs, **kw)
        assert e.value.code == -1 and "route:" in str(e.value), kw
    cost, parent, _ = host(cs)
    for kw in bad:
        with pytest.raises(ssm.SsmError) as e:
            ssm.route_path_host(cost, parent, cs["dist2"], (0, 0), **kw)
        assert e.value.code == -1 and "route:" in str(e.value), kw
    for kw in (dict(moves=4), dict(near_weight=0), dict(near_weight=8), dict(comfort=0.0), dict(comfort=1e300), dict(cell=1e-300)):
        host(cs, **kw)          # the limits themselves are legal
    for source in ((4, 2), 45, -2, (4, 4), 1 << 24):          # a cell that takes no part; outside the grid
        with pytest.raises(ssm.SsmError) as e:
            ssm.route_cells_host(cs["reach"], cs["dist2"], source)
        assert e.value.code == -1 and "source" in str(e.value), source
    for goal, snap, word in (((9, 0), 0, "goal"), ((0, 5), 0, "goal"), ((-1, 0), 0, "goal"), ((0, -1), 0, "goal"), ((0, 0), -1, "goal_snap"), ((0, 0), 1025, "goal_snap")):
        with pytest.raises(ssm.SsmError) as e:
            ssm.route_path_host(cost, parent, cs["dist2"], goal, snap)
        assert e.value.code == -1 and word in str(e.value), (goal, snap)
    with pytest.raises(ssm.SsmError) as e:
        ssm.route_path_host(cost, parent, cs["dist2"], (0, 0), max_path=0)
    assert e.value.code == -1 and "max_path" in str(e.value)
    ssm.route_path_host(cost, parent, cs["dist2"], (8, 4), 1024)
    r = np.ascontiguousarray(cs["reach"]); d = np.ascontiguousarray(cs["dist2"]); P = ssm.route_params(); I = RouteInfo(); J = RoutePathInfo()
    c = np.zeros(45, np.uint32); p = np.zeros(45, np.int32)
    call = lambda rr, dd, nx, ny, params=C.byref(P): lib.ssm_route_cells_host(rr, dd, nx, ny, 0, params, c.ctypes.data, p.ctypes.data, C.byref(I))  # noqa: E731
    assert call(None, d.ctypes.data, 9, 5) == -1 and "null" in lib.ssm_last_error(None).decode()
    assert call(r.ctypes.data, None, 9, 5) == -1 and "null" in lib.ssm_last_error(None).decode()
    for nx, ny in ((0, 5), (9, 0), (-1, 5), (4097, 4096)):
        assert call(r.ctypes.data, d.ctypes.data, nx, ny) == -1 and "2^24" in lib.ssm_last_error(None).decode()
    for nx, ny in ((32769, 1), (1, 32769)):
        assert call(r.ctypes.data, d.ctypes.data, nx, ny) == -1 and "32768" in lib.ssm_last_error(None).decode()
    assert call(r.ctypes.data, d.ctypes.data, 9, 5, None) == 0          # null parameters: the defaults
    assert lib.ssm_route_cells_host(r.ctypes.data, d.ctypes.data, 9, 5, 0, C.byref(P), None, None, None) == 0          # every output is optional
    for args in ((None, parent.ctypes.data, d.ctypes.data), (cost.ctypes.data, None, d.ctypes.data), (cost.ctypes.data, parent.ctypes.data, None)):
        assert lib.ssm_route_path_host(*args, 9, 5, C.byref(P), 0, 0, 0, 45, p.ctypes.data, C.byref(J)) == -1 and "null" in lib.ssm_last_error(None).decode()


def test_longest_sides_on_the_host():
    """1 x 32768 and 32768 x 1 open: 327670 at the far end, a path of 32768 cells"""
    import semantic_slam_mapping_amd as ssm
    for nx, ny in ((32768, 1), (1, 32768)):
        r, d = RC.field(nx, ny)
        cost, parent, info = ssm.route_cells_host(r, d, 0)
        assert int(cost.ravel()[-1]) == 327670 == info["max_cost"] and info["far_cell"] == 32767 and info["routed"] == 32768
        cells, pi = ssm.route_path_host(cost, parent, d, (nx - 1, ny - 1))
        assert pi["len"] == 32768 and pi["n_axial"] == 32767 and pi["n_diag"] == 0 and np.array_equal(cells, np.arange(32768))


def test_host_functions_as_programs_and_under_sanitizers():
    """host/test_route_core.cpp: a stand-alone program (its own main, no library, no device) over the host functions, built plainly and with
    -fsanitize=address,undefined; host/test_route_stub.cpp: the sanitizer builds' stand-in entry points, likewise"""
    for target in ("test_route_core", "test_route_core_san", "test_route_stub", "test_route_stub_san"):
        subprocess.run(["make", "-s", "-C", HOST, target], check=True, capture_output=True, timeout=600)
        r = subprocess.run([os.path.join(HOST, target)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "ALL PASSED" in r.stdout and "FAIL" not in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


def test_kernels_neither_spill_nor_use_scratch():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    from test_abi import _resource_usage
    usage = _resource_usage("kernels_route.hip")
    names = ("rt_begin_kernel", "rt_sweep_kernelILi4E", "rt_sweep_kernelILi8E", "rt_tile_kernelILi4E", "rt_tile_kernelILi8E", "rt_compact_kernel", "rt_finish_kernelILi4E",
             "rt_finish_kernelILi8E", "rt_snap_kernel", "rt_walk_kernel")
    for n in names:
        hit = [k for k in usage if n in k]
        assert len(hit) == 1, (n, sorted(usage))
        u = usage[hit[0]]
        assert u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0 and u.get("ScratchSize [bytes/lane]", 0) == 0, (hit[0], u)
