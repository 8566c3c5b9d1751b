"""CPU tests of the clearance map: ssm_clearance_cells_host -- the contract's arithmetic of include/ssm/clearance_core.h, one thread, no GPU,
a column pass and a lower envelope per row -- against the brute-force numpy / scipy restatement tests/clearance_ref.py byte for byte (dist2, nearest, reach, every info
field) on the shared cases of tests/clearance_cases.py; against scipy's exact Euclidean distance transform at 512 x 512; the cases' own properties; refusals; r2; the
host function as a stand-alone C++ program, also under AddressSanitizer + UndefinedBehaviorSanitizer; and the new kernels' register use."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clearance_ref as R  # noqa: E402
import clearance_cases as CC  # noqa: E402

HOST = os.path.join(ROOT, "semantic_slam_mapping_amd", "host")


def host(cs, **kw):
    import semantic_slam_mapping_amd as ssm
    return ssm.clearance_cells_host(cs["cls"], **dict(cs["params"], **kw))


def ref(cs, **kw):
    return R.run(cs["cls"], **dict(cs["params"], **kw))


def equal(got, want, what):
    for name, g, w, t in zip(("dist2", "nearest", "reach"), got[:3], want[:3], (np.uint32, np.int32, np.uint8)):
        assert g.dtype == w.dtype == t and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:4].tolist(), [int(g[tuple(b)]) for b in bad[:4]], [int(w[tuple(b)]) for b in bad[:4]])
        assert g.tobytes() == w.tobytes()
    assert got[3] == want[3], (what, got[3], want[3])


def check_want(cs, out, what):
    """the facts a case knows about itself, on what the library gave"""
    d2, near, reach, info = out
    want = cs.get("want", {})
    nx = cs["cls"].shape[1]
    for k, v in want.get("info", {}).items():
        assert info[k] == v, (what, k, info[k], v)
    if "d2_all" in want:
        assert (d2 == want["d2_all"]).all(), what
    if "nearest_all" in want:
        assert (near == want["nearest_all"]).all(), what
    if "d2" in want:
        assert np.array_equal(d2, want["d2"]), what
    for (cx, cy), dd, at in want.get("at", []):
        assert (int(d2[cy, cx]), int(near[cy, cx])) == (dd, at), (what, cx, cy, int(d2[cy, cx]), int(near[cy, cx]))
    for (cx, cy), r in want.get("reach_at", []):
        assert int(reach[cy, cx]) == r, (what, cx, cy, int(reach[cy, cx]))


def test_layouts_and_defaults():
    import semantic_slam_mapping_amd as ssm
    from semantic_slam_mapping_amd._lib import ClearanceParams, ClearanceInfo
    assert C.sizeof(ClearanceInfo) == 64 and C.sizeof(ClearanceParams) == 40
    P = ssm.clearance_params()
    D = R.DEFAULTS
    assert [getattr(P, k) for k in D] == list(D.values()) and (P.blocked_mask, P.free_mask, P.connectivity, P.seed_cx, P.seed_cy, P.seed_snap, P.radius) == (16, 2, 4, -1, -1, 10, 1.0)
    P = ssm.clearance_params(blocked=[4, 0, 4], free=[1, 2], seed=(3, 5))
    assert (P.blocked_mask, P.free_mask, P.seed_cx, P.seed_cy) == (17, 6, 3, 5)
    with pytest.raises(TypeError):
        ssm.clearance_params(radios=1)


@pytest.mark.parametrize("name", list(CC.cases()))
def test_host_equals_restatement_on_the_cases(name):
    cs = CC.cases()[name]()
    assert cs["cls"].shape[0] <= 65 and cs["cls"].shape[1] <= 65
    for conn in (4, 8):
        equal(host(cs, connectivity=conn), ref(cs, connectivity=conn), (name, conn))
    check_want(cs, host(cs), name)


@pytest.mark.parametrize("shape", [s for s in CC.SHAPES if s[0] * s[1] <= 65 * 65])
def test_host_equals_restatement_at_the_shapes(shape):
    nx, ny = shape
    for fraction in (0.0, 0.02, 0.3, 1.0):
        cs = CC.random_fill(nx, ny, fraction, nx * 7 + ny, radius=1.0)
        for conn in (4, 8):
            equal(host(cs, connectivity=conn), ref(cs, connectivity=conn), (shape, fraction, conn))


@pytest.mark.parametrize("fraction,seed", [(0.001, 1), (0.05, 2), (0.5, 3), (0.0001, 4), (0.2, 5)])
def test_distances_equal_scipy_at_512(fraction, seed):
    """dist2 == the d2 recomputed from the indices of scipy.ndimage.distance_transform_edt (exact; its nearest cell differs on ties, so that is not compared); every
    nearest is a blocked cell at exactly dist2"""
    from scipy import ndimage
    cs = CC.random_fill(512, 512, fraction, seed)
    d2, near, reach, info = host(cs)
    blocked = cs["cls"] == CC.O
    assert blocked.any() and info["blocked"] == int(blocked.sum())
    iy, ix = ndimage.distance_transform_edt(~blocked, return_distances=False, return_indices=True)
    ys, xs = np.mgrid[0:512, 0:512]
    want = (iy - ys).astype(np.int64) ** 2 + (ix - xs).astype(np.int64) ** 2
    assert np.array_equal(d2.astype(np.int64), want), int((d2 != want).sum())
    ny_, nx_ = near // 512, near % 512
    assert blocked[ny_, nx_].all() and np.array_equal((ny_ - ys).astype(np.int64) ** 2 + (nx_ - xs).astype(np.int64) ** 2, want)
    # among the blocked cells at exactly dist2 the lowest index: spot-checked by brute force on a sample of cells
    by, bx = np.nonzero(blocked)
    rng = np.random.default_rng(seed)
    for cy, cx in rng.integers(0, 512, (40, 2)):
        dd = (bx - cx).astype(np.int64) ** 2 + (by - cy).astype(np.int64) ** 2
        assert int(near[cy, cx]) == int(((dd << 24) | (by * 512 + bx)).min() & 0xFFFFFF), (cy, cx)


def test_cases_are_what_they_are_for():
    """the properties the cases are for, on what the LIBRARY gives"""
    K = CC.cases()
    o, c = host(K["corridor_open"]()), host(K["corridor_closed"]())
    assert o[3]["components"] == 1 and c[3]["components"] == o[3]["components"] + 1          # one more cell of radius closes the lane: one component more
    assert o[2][18, 7] == 2 and c[2][18, 7] == 1 and c[3]["reachable"] < c[3]["traversable"] and o[3]["reachable"] == o[3]["traversable"]
    assert not (c[2][10] != 0).any() and (o[2][10] == 2).sum() == 4
    g = K["diagonal_gap"]()
    assert host(g, connectivity=8)[3]["components"] == 1 and host(g, connectivity=4)[3]["components"] == 2
    r8, r4 = host(g, connectivity=8)[2], host(g, connectivity=4)[2]
    assert r8[6, 6] == 2 and r4[6, 6] == 1 and r4[1, 1] == 2 and r4[4, 3] == 1 and r8[4, 3] == 2
    s = host(K["seed_snaps"]())
    assert K["seed_snaps"]()["cls"][10, 7] == CC.O and s[3]["seed_cell"] == 8 * 15 + 6 and s[2][8, 6] == 2 and s[3]["reachable"] == s[3]["traversable"] > 0
    n = host(K["seed_finds_nothing"]())
    assert n[3]["seed_cell"] == -1 and n[3]["reachable"] == 0 and n[3]["traversable"] == s[3]["traversable"] and set(np.unique(n[2])) == {0, 1}
    t = host(K["snap_tie"]())
    assert t[3]["seed_cell"] == 2 * 9 + 3 and (t[2][:, :4] == 2).all() and (t[2][:, 5:] == 1).all() and (t[2][:, 4] == 0).all()
    assert host(K["snap_tie"](), seed_snap=0)[3]["seed_cell"] == -1          # the seed's own cell is not free
    cb = K["checkerboard"]()
    assert host(cb, connectivity=4)[3]["components"] == host(cb)[3]["traversable"] and host(cb, connectivity=8)[3]["components"] == 1
    assert host(cb, radius=1.0)[3]["traversable"] == 0 and host(cb, radius=0.99)[3]["traversable"] > 0          # every free cell is exactly one cell from a blocked one
    for name in K:
        cs = K[name]()
        d2, near, reach, info = host(cs)
        P = R.params_of(cs["params"])
        blocked = R.in_mask(cs["cls"], P["blocked_mask"])
        assert ((d2 == 0) == blocked).all() and info["reachable"] <= info["traversable"] <= info["free_cells"] and info["reachable"] == int((reach == 2).sum())
        if blocked.any():
            assert (near[blocked] == np.flatnonzero(blocked.ravel())).all() and blocked.ravel()[near.ravel()].all()


def test_r2():
    """r2 = floor((radius / cell)^2), saturated at 2^31"""
    cs = CC.one_blocked("middle")
    for radius, cell, want in ((0.0, 1.0, 0), (1.0, 1.0, 1), (0.999, 1.0, 0), (1.001, 1.0, 1), (0.2, 0.2, 1), (0.1999, 0.2, 0), (0.2001, 0.2, 1), (1.0, 0.2, 25), (0.5, 0.2, 6), (3.0, 1.5, 4),
                               (1e9, 1.0, 1 << 31), (46340.95, 1.0, 2147483646), (46341.0, 1.0, 1 << 31), (1e300, 1e-300, 1 << 31)):
        info = host(cs, radius=radius, cell=cell)[3]
        assert info["r2"] == want == R.r2_of(radius, cell), (radius, cell, info["r2"], want)
    # a cell exactly r away is not traversable, one beyond it is
    d2, _, reach, info = host(cs, radius=2.0)
    assert info["r2"] == 4 and ((reach != 0) == (d2 > 4)).all() and (d2 == 4).any() and (d2 == 5).any()
    assert host(cs, radius=1e9)[3]["traversable"] == 0 and host(CC.nothing_blocked(), radius=1e9)[3]["traversable"] == 54          # nothing blocked: UINT32_MAX is above every r2


def test_refusals():
    import semantic_slam_mapping_amd as ssm
    lib = ssm.load()
    cs = CC.one_blocked("middle")          # 9 x 7
    nan, inf = float("nan"), float("inf")
    bad = (dict(blocked_mask=1 << 5), dict(free_mask=1 << 5), dict(free_mask=0x80000000), dict(blocked_mask=6, free_mask=2), dict(blocked=[4], free=[4]), dict(connectivity=6), dict(connectivity=0),
           dict(connectivity=-4), dict(radius=-0.1), dict(radius=nan), dict(radius=inf), dict(cell=0.0), dict(cell=-1.0), dict(cell=nan), dict(cell=inf), dict(seed_snap=-1), dict(seed_snap=1025),
           dict(seed=(9, 0)), dict(seed=(0, 7)), dict(seed=(-1, 0)), dict(seed=(0, -1)), dict(seed=(-2, -2)), dict(seed=(100, 100)))
    for kw in bad:
        with pytest.raises(ssm.SsmError) as e:
            host(cs, **kw)
        assert e.value.code == -1 and "clearance:" in str(e.value), kw
    for kw in (dict(blocked_mask=0), dict(free_mask=0), dict(blocked_mask=0x1D, free_mask=2), dict(radius=0.0), dict(radius=1e300), dict(seed_snap=0), dict(seed_snap=1024), dict(seed=(8, 6)),
               dict(seed=(0, 0)), dict(seed=None)):
        host(cs, **kw)          # the limits themselves are legal
    from semantic_slam_mapping_amd._lib import ClearanceInfo
    P = ssm.clearance_params(); a = np.ascontiguousarray(cs["cls"]); I = ClearanceInfo()
    d2 = np.zeros(63, np.uint32); near = np.zeros(63, np.int32); reach = np.zeros(63, np.uint8)
    call = lambda cls, nx, ny, p=C.byref(P): lib.ssm_clearance_cells_host(cls, nx, ny, p, d2.ctypes.data, near.ctypes.data, reach.ctypes.data, C.byref(I))  # noqa: E731
    assert call(None, 9, 7) == -1 and "null" in lib.ssm_last_error(None).decode()
    for nx, ny in ((0, 7), (9, 0), (-1, 7), (4097, 4096)):
        assert call(a.ctypes.data, nx, ny) == -1
    for nx, ny in ((32769, 1), (1, 32769), (32769, 512)):
        assert call(a.ctypes.data, nx, ny) == -1 and ("32768" in lib.ssm_last_error(None).decode() or "2^24" in lib.ssm_last_error(None).decode())
    assert call(a.ctypes.data, 32769, 1) == -1 and "32768" in lib.ssm_last_error(None).decode()
    assert call(a.ctypes.data, 9, 7, None) == 0          # null parameters: the defaults
    assert lib.ssm_clearance_cells_host(a.ctypes.data, 9, 7, C.byref(P), None, None, None, None) == 0          # every output is optional
    long_row = np.full((1, 32768), CC.D, np.uint8); long_row[0, 0] = CC.O
    d2 = ssm.clearance_cells_host(long_row)[0]
    assert int(d2[0, -1]) == 32767 ** 2 == 1073676289 and int(ssm.clearance_cells_host(long_row.T.copy())[0][-1, 0]) == 32767 ** 2          # the longest side and the largest distance


def test_host_function_as_a_program_and_under_sanitizers():
    """host/test_clearance_core.cpp: a stand-alone program (its own main, no library, no device) over the host function, built plainly and with
    -fsanitize=address,undefined; host/test_clearance_stub.cpp: the sanitizer builds' stand-in entry points, likewise"""
    for target in ("test_clearance_core", "test_clearance_core_san", "test_clearance_stub", "test_clearance_stub_san"):
        subprocess.run(["make", "-s", "-C", HOST, target], check=True, capture_output=True, timeout=600)
        r = subprocess.run([os.path.join(HOST, target)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "ALL PASSED" in r.stdout and "FAIL" not in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


def test_kernels_neither_spill_nor_use_scratch():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    from test_abi import _resource_usage
    usage = _resource_usage("kernels_clearance.hip")
    names = ("clr_begin_kernel", "clr_mask_kernel", "clr_column_kernel", "clr_row_lds_kernel", "clr_row_scan_kernel", "clr_seed_kernel", "clr_local_kernelILi4E", "clr_local_kernelILi8E",
             "clr_merge_kernelILi4E", "clr_merge_kernelILi8E", "clr_flatten_kernel", "clr_finish_kernel")
    for n in names:
        hit = [k for k in usage if n in k]
        assert len(hit) == 1, (n, sorted(usage))
        u = usage[hit[0]]
        assert u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0 and u.get("ScratchSize [bytes/lane]", 0) == 0, (hit[0], u)
