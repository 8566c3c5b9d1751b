"""CPU tests of free-space carving: ssm_carve_host -- the contract's arithmetic of include/ssm/carve_core.h, one thread, no GPU -- against the
numpy restatement tests/carve_ref.py exactly (verdicts, counters before and after the compaction, the kept points, every info field) on the shared case list;
the list's own properties (each verdict occurs, each boundary of the section is hit on both sides); two views in sequence; refusals; the host function as a
stand-alone C++ program, also under AddressSanitizer + UndefinedBehaviorSanitizer; and the new kernels' register use."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import carve_ref as R  # noqa: E402

HOST = os.path.join(ROOT, "semantic_slam_mapping_amd", "host")
CASES = list(R.cases())
_cache = {}


def ref_of(name):
    """-> (case, restatement), computed once and shared"""
    if name not in _cache:
        cs = R.cases()[name]()
        _cache[name] = (cs, R.run_case(cs))
    return _cache[name]


def host_call(cs, **kw):
    import semantic_slam_mapping_amd as ssm
    return ssm.carve_host(cs["depth"], cs["camera"], cs["T_view"], cs["pts"], cs["T_cloud"], cs["run"], record=True, **dict(cs["params"], **kw))


def equal_to_ref(got, ref, what=""):
    pts, run, info, rec = got
    assert np.array_equal(rec["verdict"], ref["verdict"]), (what, "verdict", np.nonzero(rec["verdict"] != ref["verdict"])[0][:10])
    assert np.array_equal(rec["run"], ref["run"]), (what, "run")
    for f in R.INFO_FIELDS:
        assert info[f] == ref["info"][f], (what, f, info[f], ref["info"][f])
    assert pts.tobytes() == ref["points"].tobytes(), (what, "points")
    assert np.array_equal(run, ref["run_kept"]), (what, "kept counters")


@pytest.mark.parametrize("name", CASES)
def test_host_equals_restatement(name):
    cs, ref = ref_of(name)
    pts0, run0 = cs["pts"].copy(), None if cs["run"] is None else cs["run"].copy()
    got = host_call(cs)
    equal_to_ref(got, ref, name)
    assert cs["pts"].tobytes() == pts0.tobytes() and (run0 is None or np.array_equal(cs["run"], run0))
    info = got[2]
    assert info["n_in"] == len(cs["pts"]) and info["n_kept"] == len(got[0]) == len(got[1]) and info["removed"] == info["n_in"] - info["n_kept"]
    assert info["unknown"] + info["occluded"] + info["supported"] + info["seen_through"] == info["n_in"]


def _why(name):
    cs, ref = ref_of(name)
    return cs, ref, [y for y in ref["why"] if y is not None and not y["zero"]]


def test_cases_are_what_they_are_for():
    """the shapes of the case list do what their names say (this guards the list, not the library)"""
    seen = set()
    for name in CASES:
        seen |= set(ref_of(name)[1]["verdict"].tolist())
    assert seen == {0, 1, 2, 3}
    # the window rule: a pixel exactly r from a border is judged, one at r - 1 is not; the four corners and the ring outside the image are there
    for (w, h) in ((8, 6), (70, 9)):
        for r in (0, 1, 3):
            name = f"every_pixel_{w}x{h}_r{r}"
            if name not in CASES:
                assert 2 * r + 1 > min(w, h)
                continue
            cs, ref = ref_of(name)
            v = ref["verdict"].reshape(h + 2, w + 2)
            xx, yy = np.meshgrid(np.arange(-1, w + 1), np.arange(-1, h + 1))
            border = np.minimum(np.minimum(xx, w - 1 - xx), np.minimum(yy, h - 1 - yy))
            assert ((v == R.SUPPORTED) == (border >= r)).all() and ((v == R.UNKNOWN) == (border < r)).all()
            assert (border == r).any() and (border == r - 1).any() and (border == -1).sum() == 2 * (w + 2) + 2 * h
    # ties: u + 0.5 a whole number goes to the pixel above; -0.5 lands on pixel 0
    cs, ref = ref_of("ties_u")
    assert [y["px"] for y in ref["why"][:9] if y] == list(range(0, 8)) and ref["why"][8] is None          # x + 0.5 -> x + 1; 7.5 -> 8 is outside
    assert ref["verdict"][0] == R.SEEN_THROUGH and ref["verdict"][1] == R.SUPPORTED                          # -0.5 -> column 0 (even: 3 m), 0.5 -> column 1 (odd: 1 m)
    assert [y["px"] for y in ref["why"][9:17]] == list(range(8)) and [y["px"] for y in ref["why"][17:]] == list(range(1, 8))
    cs, ref = ref_of("ties_v")
    assert [y["py"] for y in ref["why"][:7] if y] == list(range(0, 6)) and ref["why"][6] is None and [y["py"] for y in ref["why"][7:]] == list(range(6))
    # behind the camera, at z_min and just below it, +-1e30, NaN and infinity
    cs, ref = ref_of("degenerate")
    v = ref["verdict"]
    assert (v[:4] == R.UNKNOWN).all() and v[4] == R.SEEN_THROUGH and v[5] == R.UNKNOWN and v[6] == R.SEEN_THROUGH and ref["why"][4]["px"] == 2
    assert float(ref["q"][2][4]) == cs["params"]["z_min"] and float(ref["q"][2][5]) < cs["params"]["z_min"]
    assert (v[7:11] == R.UNKNOWN).all() and v[11] == R.OCCLUDED and ref["why"][11]["zq"] == R.ZQ_LIMIT and (v[15:23] == R.UNKNOWN).all() and v[24] == R.SUPPORTED
    cs, ref = ref_of("z_min_default")
    assert ref["verdict"].tolist() == [R.SUPPORTED, R.UNKNOWN, R.OCCLUDED]
    # a zero in the window's corner only -> UNKNOWN; a zero just outside the window does not count
    for r in (1, 3):
        cs, ref = ref_of(f"zero_corner_r{r}")
        assert ref["verdict"].tolist() == [0, 0, 0, 0, 2, 2] and (cs["depth"] == 0).sum() == 6
        for i in range(4):
            x, y = ref["why"][i]["px"], ref["why"][i]["py"]
            win = cs["depth"][y - r:y + r + 1, x - r:x + r + 1]
            assert (win == 0).sum() == 1 and win[0 if i in (0, 2) else -1, 0 if i in (0, 3) else -1] == 0
    # zq + tol against dmin, |zq - d| against tol: both sides of both
    for name in [n for n in CASES if n.startswith("thresholds")]:
        cs, ref, why = _why(name)
        edge = {y["zq"] + y["tol"] - y["dmin"] for y in why}
        assert {0, -1} <= edge, (name, sorted(edge))
        not_seen = {abs(y["zq"] - y["d"]) - y["tol"] for y in why if not y["zq"] + y["tol"] < y["dmin"]}
        assert {0, 1} <= not_seen, (name, sorted(not_seen))
        if "_r1_" in name:
            assert any(y["dmin"] < y["d"] for y in why)
        if name.endswith("ppm20000"):
            assert all(y["tol"] > 50 for y in why)
    # counters
    for mv in (1, 2, 3):
        cs, ref = ref_of(f"counters_votes{mv}")
        assert ref["verdict"].tolist() == [2] * 5 + [3] * 5 + [1] * 5 + [0] * 5
        assert ref["run"].tolist() == [0] * 5 + [1, 2, 3, 255, 255] + [0, 1, 2, 254, 255] * 2
        assert ref["info"]["n_kept"] == 5 + sum(x < mv for x in [1, 2, 3, 255, 255] + [0, 1, 2, 254, 255] * 2)
    assert ref_of("all_removed")[1]["info"]["n_kept"] == 0 and ref_of("all_removed")[1]["info"]["n_in"] > 256
    assert ref_of("nothing_removed")[1]["info"]["removed"] == 0
    for name in [n for n in CASES if n.startswith("posed")]:
        info = ref_of(name)[1]["info"]
        fields = ("unknown", "occluded", "supported", "seen_through", "removed", "n_kept") if name in ("posed_70x9", "posed_160x120") else ("unknown", "occluded", "removed", "n_kept")
        assert min(info[f] for f in fields) > 0, (name, info)


def test_relative_pose_is_the_rigid_inverse():
    rng = np.random.default_rng(11)
    for _ in range(5):
        Tv, Tc = R.pose(rng, 0.7, 5.0), R.pose(rng, 0.7, 5.0)
        assert np.allclose(R.rel_pose(Tv, Tc), (np.linalg.inv(Tv) @ Tc)[:3], atol=1e-12)


def test_two_views_in_sequence():
    """see-through, support, see-through keeps the point (the run is cleared in between); see-through twice removes it"""
    import semantic_slam_mapping_amd as ssm
    pts = R.cloud([R.at_pixel(3, 3, 1.0), R.at_pixel(5, 3, 1.0)])
    far, near = np.full((6, 8), 3000, np.uint16), np.full((6, 8), 1000, np.uint16)
    mixed = far.copy()
    mixed[:, :4] = 1000          # supports the first point only (the window of the second, columns 4..6, is all far)
    p, run, info = ssm.carve_host(far, R.cam0(), R.EYE, pts, R.EYE)
    assert len(p) == 2 and run.tolist() == [1, 1] and info["seen_through"] == 2
    p, run, info = ssm.carve_host(mixed, R.cam0(), R.EYE, p, R.EYE, run)
    assert p.tobytes() == pts[:1].tobytes() and run.tolist() == [0] and info["removed"] == 1 and info["supported"] == 1
    p, run, info = ssm.carve_host(far, R.cam0(), R.EYE, p, R.EYE, run)
    assert len(p) == 1 and run.tolist() == [1]
    p, run, info = ssm.carve_host(near, R.cam0(), R.EYE, p, R.EYE, run)
    assert len(p) == 1 and run.tolist() == [0]


def test_refusals():
    import semantic_slam_mapping_amd as ssm
    from semantic_slam_mapping_amd._lib import CarveParams, CarveInfo, Camera
    lib = ssm.load()
    cs, _ = ref_of("posed_70x9")
    nan, inf = float("nan"), float("inf")
    for kw in (dict(min_votes=0), dict(min_votes=256), dict(radius=-1), dict(radius=4), dict(tol_abs=-0.01), dict(tol_abs=nan), dict(tol_abs=inf), dict(tol_abs=2e6),
               dict(tol_rel_ppm=-1), dict(tol_rel_ppm=1000001), dict(z_min=-0.1), dict(z_min=nan), dict(z_min=inf)):
        with pytest.raises(ssm.SsmError) as e:
            host_call(cs, **kw)
        assert e.value.code == -1, kw          # SSM_E_INVAL
    for cam in ((0, 0, 64, 64, 0.0), (0, 0, 64, 64, -1.0), (0, 0, 64, 64, nan), (0, 0, nan, 64, 1000.0), (inf, 0, 64, 64, 1000.0), (0, 0, 64, 64, 2e6)):
        with pytest.raises(ssm.SsmError) as e:
            ssm.carve_host(cs["depth"], cam, R.EYE, cs["pts"], R.EYE)
        assert e.value.code == -1, cam
    bad = np.eye(4)
    bad[1, 3] = nan
    for Tv, Tc in ((bad, R.EYE), (R.EYE, bad)):
        with pytest.raises(ssm.SsmError) as e:
            ssm.carve_host(cs["depth"], cs["camera"], Tv, cs["pts"], Tc)
        assert e.value.code == -1
    with pytest.raises(TypeError):
        ssm.carve_host(cs["depth"], cs["camera"], R.EYE, cs["pts"], R.EYE, votes=2)
    P = CarveParams(); lib.ssm_carve_params_default(C.byref(P))
    assert (P.min_votes, P.radius, P.tol_abs, P.tol_rel_ppm, P.z_min) == tuple(R.DEFAULTS[k] for k in ("min_votes", "radius", "tol_abs", "tol_rel_ppm", "z_min"))
    pts, dep = cs["pts"], cs["depth"]
    n = len(pts)
    h, w = dep.shape
    cam = Camera(*cs["camera"]); T = np.ascontiguousarray(np.eye(4).reshape(16))
    out = np.zeros(n, R.POINT_DTYPE); got = C.c_int(0); I = CarveInfo()
    call = lambda d, ww, hh, cm, tv, p, nn, tc, o, cap, g, info=None: lib.ssm_carve_host(d, ww, hh, cm, tv, p, nn, tc, None, None, o, cap, g, info, None, None)  # noqa: E731
    ok = (dep.ctypes.data, w, h, C.byref(cam), T.ctypes.data, pts.ctypes.data, n, T.ctypes.data, out.ctypes.data, n, C.byref(got))
    assert call(*ok, C.byref(I)) == 0 and got.value == I.n_kept > 5
    for i, v in ((0, None), (1, 0), (2, -1), (3, None), (4, None), (5, None), (6, -1), (7, None), (9, -1), (10, None)):
        a = list(ok)
        a[i] = v
        assert call(*a) == -1, i
    a = list(ok)
    a[9] = 5
    J = CarveInfo()
    assert call(*a, C.byref(J)) == -4 and got.value == J.n_kept == I.n_kept          # SSM_E_CAPACITY, with the count needed
    a = list(ok)
    a[8] = None
    assert call(*a) == -1


def test_host_function_as_a_program_and_under_sanitizers():
    """host/test_carve_core.cpp: a stand-alone program (its own main, no library, no device) over the host function, built plainly and with
    -fsanitize=address,undefined"""
    for target in ("test_carve_core", "test_carve_core_san"):
        subprocess.run(["make", "-s", "-C", HOST, target], check=True, capture_output=True, timeout=600)
        r = subprocess.run([os.path.join(HOST, target)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "ALL PASSED" in r.stdout and "FAIL" not in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


def test_kernels_neither_spill_nor_use_scratch():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    from test_abi import _resource_usage
    usage = _resource_usage("kernels_carve.hip")
    for n in ("carve_init_kernel", "carve_verdict_kernel", "carve_base_kernel", "carve_compact_kernel", "carve_store_kernel"):
        hit = [k for k in usage if n in k]
        assert len(hit) == 1, (n, sorted(usage))
        u = usage[hit[0]]
        assert u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0 and u.get("ScratchSize [bytes/lane]", 0) == 0, (hit[0], u)
