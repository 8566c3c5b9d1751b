"""CPU tests of dense alignment: ssm_align_host -- the contract's arithmetic of include/ssm/align_core.h and the solve of
csrc/ssm_align_host.cpp, one thread, no GPU -- against the numpy restatement tests/align_ref.py byte for byte (valid mask, normals, every iteration's sums and
counts and the E it used, the final E, T_view_out, every info field) on the shared case list; the list's own properties; order independence; every status;
every refusal; convergence against the truth of an analytic scene; the host function as a stand-alone C++ program, also under AddressSanitizer +
UndefinedBehaviorSanitizer; and the new kernels' register use."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import align_ref as A  # noqa: E402
import align_cases as AC  # noqa: E402

HOST = os.path.join(ROOT, "semantic_slam_mapping_amd", "host")
CASES = list(AC.cases())
_cache = {}


def ref_of(name):
    """-> (case, restatement), computed once and shared"""
    if name not in _cache:
        cs = AC.cases()[name]()
        _cache[name] = (cs, A.align(cs["depth"], cs["camera"], cs["T_view"], cs["clouds"], cs["T_clouds"], why=True, **cs["params"]))
    return _cache[name]


def host_align(cs, **kw):
    import semantic_slam_mapping_amd as ssm
    return ssm.align_host(cs["depth"], cs["camera"], cs["T_view"], cs["clouds"], cs["T_clouds"], **dict(cs["params"], **kw))


def equal_to_ref(got, ref, what=""):
    """got: align_host's or the device's result (valid / normals are compared when present)"""
    if "valid" in got:
        assert np.array_equal(got["valid"], ref["valid"]), what
        assert got["normals"].dtype == np.float32 and got["normals"].tobytes() == ref["normals"].tobytes(), what
    assert len(got["record"]) == len(ref["record"]), (what, len(got["record"]), len(ref["record"]))
    for it, (g, r) in enumerate(zip(got["record"], ref["record"])):
        assert g["sums"].tolist() == list(r["sums"]), (what, it)
        assert g["E"].tobytes() == np.ascontiguousarray(r["E"], np.float64).tobytes(), (what, it)
    for f in A.INFO_FIELDS:
        assert got["info"][f] == ref["info"][f], (what, f, got["info"][f], ref["info"][f])
    assert got["info"]["E"].tobytes() == ref["info"]["E"].tobytes(), what
    assert got["T_view"].tobytes() == ref["T_view"].tobytes(), what


def same_result(a, b):
    assert a["T_view"].tobytes() == b["T_view"].tobytes() and a["info"]["E"].tobytes() == b["info"]["E"].tobytes()
    assert all(a["info"][f] == b["info"][f] for f in A.INFO_FIELDS)
    assert a["record"].tobytes() == b["record"].tobytes()


@pytest.mark.parametrize("name", CASES)
def test_host_equals_restatement(name):
    cs, ref = ref_of(name)
    before = [c.tobytes() for c in cs["clouds"]]
    equal_to_ref(host_align(cs), ref, name)
    assert [c.tobytes() for c in cs["clouds"]] == before


def test_cases_are_what_they_are_for():
    """the shapes of the case list do what their names say (this guards the list, not the library)"""
    count = lambda ref: dict(zip(A.WHY, np.bincount(np.concatenate(ref["why"]) if ref["why"] else np.zeros(0, int), minlength=len(A.WHY)).tolist()))  # noqa: E731
    cs, ref = ref_of("room_67x35")
    assert cs["depth"].shape == (35, 67)          # an odd width
    c = count(ref)
    assert c["outside"] > 0 and c["invalid"] > 0 and c["quadratic"] > 1000 and ref["info"]["status"] == A.CONVERGED
    # a depth edge crosses the view: the box's silhouette has depth on both sides and no normal
    v, d = ref["valid"].astype(bool), cs["depth"].astype(np.int64)
    inner = np.zeros_like(v); inner[1:-1, 1:-1] = True
    jump = np.zeros_like(v); jump[:, 1:] |= np.abs(d[:, 1:] - d[:, :-1]) > 500
    assert (jump & inner & (d > 0) & ~v).sum() > 20 and not (jump & v).any()
    assert not v[0].any() and not v[-1].any() and not v[:, 0].any() and not v[:, -1].any()
    lens = np.linalg.norm(ref["normals"][..., :3].astype(np.float64), axis=-1)
    assert np.allclose(lens[v], 1.0, atol=1e-6) and (lens[~v] == 0).all() and (ref["normals"][..., 3] == 0).all()
    cs3, ref3 = ref_of("room_67x35_stride3")
    assert cs3["params"]["stride"] == 3 and ref3["info"]["n_in"] == sum((len(p) + 2) // 3 for p in cs3["clouds"]) < ref["info"]["n_in"] == sum(len(p) for p in cs["clouds"])
    c = count(ref_of("tail_and_far")[1])
    assert c["far"] > 100 and c["tail"] > 100 and c["quadratic"] > 100
    c = count(ref_of("outside")[1])
    assert c["outside"] > c["quadratic"] > 0
    cs, ref = ref_of("mirrored_fx")
    assert cs["camera"][2] < 0 and ref["info"]["status"] == A.CONVERGED and A.pose_error(ref["T_view"], cs["T_true"])[0] < 0.2 * A.pose_error(cs["T_view"], cs["T_true"])[0]
    assert ref_of("tight_gate")[1]["valid"].sum() < ref_of("room_67x35")[1]["valid"].sum()
    cs, ref = ref_of("three_clouds_z_range")
    assert [len(p) > 0 for p in cs["clouds"]] == [True, False, True] and count(ref)["z_range"] > 100
    assert ref_of("empty_m0")[1]["info"]["n_in"] == 0 and ref_of("empty_m0")[1]["info"]["status"] == A.TOO_FEW
    c = count(ref_of("degenerate_points")[1])
    assert c["not_finite"] == 3 and c["z_range"] >= 4


def test_order_independence():
    """the same clouds reversed and the same points permuted: identical sums, pose and info"""
    cs, ref = ref_of("room_67x35")
    base = host_align(cs)
    rev = dict(cs, clouds=cs["clouds"][::-1], T_clouds=cs["T_clouds"][::-1])
    same_result(host_align(rev), base)
    rng = np.random.default_rng(5)
    perm = dict(cs, clouds=[p[rng.permutation(len(p))] for p in cs["clouds"]])
    same_result(host_align(perm), base)
    equal_to_ref(host_align(perm), ref, "permuted")


def test_every_status():
    import semantic_slam_mapping_amd as ssm
    cs, ref = ref_of("room_67x35")
    unchanged = lambda r: r["T_view"].tobytes() == np.asarray(cs["T_view"], np.float64).tobytes() and np.array_equal(r["info"]["E"], np.eye(4))  # noqa: E731
    assert ref["info"]["status"] == A.CONVERGED and ref["info"]["iterations"] < 10
    for kw, status in ((dict(max_iterations=2), A.MAX_ITER), (dict(min_inliers=10 ** 6), A.TOO_FEW), (dict(max_shift=0.01), A.DIVERGED), (dict(max_angle=0.005), A.DIVERGED)):
        r = A.align(cs["depth"], cs["camera"], cs["T_view"], cs["clouds"], cs["T_clouds"], **dict(cs["params"], **kw))
        got = host_align(cs, **kw)
        equal_to_ref(got, r, str(kw))
        assert got["info"]["status"] == status, (kw, got["info"])
        assert unchanged(got) == (status != A.MAX_ITER)
    # DEGENERATE: a single fronto-parallel plane leaves three directions without any constraint; without damping the third pivot is exactly zero
    cam = AC.SMALL
    flat = dict(depth=AC.ray_cast(AC.WALL, np.eye(4), cam, 67, 35), camera=cam, T_view=AC.se3(tz=0.02), clouds=[AC.back_project(AC.ray_cast(AC.WALL, np.eye(4), cam, 67, 35), cam)],
                T_clouds=[np.eye(4)], params=dict(min_inliers=50, damping=0.0))
    r = A.align(flat["depth"], cam, flat["T_view"], flat["clouds"], flat["T_clouds"], **flat["params"])
    got = ssm.align_host(flat["depth"], cam, flat["T_view"], flat["clouds"], flat["T_clouds"], **flat["params"])
    equal_to_ref(got, r, "flat")
    assert got["info"]["status"] == A.DEGENERATE and got["info"]["inliers_last"] > 1000 and got["T_view"].tobytes() == flat["T_view"].tobytes()
    assert ssm.align_host(flat["depth"], cam, flat["T_view"], flat["clouds"], flat["T_clouds"], min_inliers=50)["info"]["status"] != A.DEGENERATE          # damping makes every pivot positive


def test_refusals():
    import semantic_slam_mapping_amd as ssm
    from semantic_slam_mapping_amd._lib import AlignParams, Camera
    lib = ssm.load()
    cs, _ = ref_of("room_67x35")
    nan, inf = float("nan"), float("inf")
    bad = [dict(max_iterations=0), dict(max_iterations=65), dict(stride=0), dict(stride=(1 << 20) + 1), dict(min_inliers=-1), dict(z_max=0.05), dict(max_angle=3.2),
           dict(tol_abs=2e6), dict(tol_rel_ppm=-1), dict(tol_rel_ppm=1000001)]
    for f in ("z_min", "z_max", "dist_max", "delta", "damping", "eps_rot", "eps_trans", "max_shift", "max_angle", "tol_abs"):
        bad += [{f: -0.01}, {f: nan}, {f: inf}]
    for kw in bad:
        with pytest.raises(ssm.SsmError) as e:
            host_align(cs, **kw)
        assert e.value.code == -1, kw          # SSM_E_INVAL
    for cam in ((0, 0, 64, 64, 0.0), (0, 0, 64, 64, -1.0), (0, 0, 64, 64, nan), (0, 0, nan, 64, 1000.0), (inf, 0, 64, 64, 1000.0), (0, 0, 64, 64, 2e6), (0, 0, 0.0, 64, 1000.0)):
        with pytest.raises(ssm.SsmError) as e:
            ssm.align_host(cs["depth"], cam, cs["T_view"], cs["clouds"], cs["T_clouds"], min_inliers=50)
        assert e.value.code == -1, cam
    badT = np.eye(4)
    badT[1, 3] = nan
    for Tv, Tc in ((badT, cs["T_clouds"]), (cs["T_view"], [cs["T_clouds"][0], badT])):
        with pytest.raises(ssm.SsmError) as e:
            ssm.align_host(cs["depth"], cs["camera"], Tv, cs["clouds"], Tc, min_inliers=50)
        assert e.value.code == -1
    for shape in ((2, 67), (35, 2), (1 << 13, (1 << 13) + 1)):
        with pytest.raises(ssm.SsmError) as e:
            ssm.align_host(np.zeros(shape, np.uint16), cs["camera"], cs["T_view"], [], [])
        assert e.value.code == -1, shape
    with pytest.raises(TypeError):
        host_align(cs, radius=2)
    P = AlignParams(); lib.ssm_align_params_default(C.byref(P))
    assert {k: getattr(P, k) for k in A.DEFAULTS} == A.DEFAULTS == ssm.api.ALIGN_DEFAULTS
    # the overflow bound: the default z_max leaves room for 5 x 467 k points under KITTI's field of view; z_max = 1e9 does not for any point count above zero
    assert host_align(cs)["info"]["n_in"] > 0
    with pytest.raises(ssm.SsmError) as e:
        host_align(cs, z_max=1.0e9)
    assert e.value.code == -1 and "2^62" in str(e.value)
    # m < 0, a negative count, the same cloud twice, and a point count too large for the bound (refused before a point is read)
    cam = Camera(*cs["camera"]); T = np.ascontiguousarray(np.eye(4).reshape(16)); T3 = np.ascontiguousarray(np.tile(T, 3)); To = np.zeros(16)
    dep = np.ascontiguousarray(cs["depth"])
    one, two, three = (cs["clouds"][0][i * 100:(i + 1) * 100].copy() for i in range(3))
    ptrs = (C.c_void_p * 3)(one.ctypes.data, two.ctypes.data, three.ctypes.data)
    Pk = ssm.align_params(min_inliers=50)

    def call(n, m, ptrs=ptrs, P=Pk):
        return lib.ssm_align_host(dep.ctypes.data, 67, 35, C.byref(cam), T.ctypes.data, ptrs, np.ascontiguousarray(n, np.int32).ctypes.data, T3.ctypes.data, m, C.byref(P), To.ctypes.data,
                                  None, None, None, None, 0, None)
    assert call([1, 1, 1], 3) == 0 and call([1, 1, 1], 0) == 0
    assert call([1, 1, 1], -1) == -1 and call([1, -1, 1], 3) == -1
    assert call([1, 1, 1], 3, ptrs=(C.c_void_p * 3)(one.ctypes.data, two.ctypes.data, one.ctypes.data)) == -1
    big = 2 ** 31 - 1
    assert call([big, big, big], 3, P=ssm.align_params(min_inliers=50, z_max=1.0e5)) == -1          # 6.4e9 points x (1.4e5 m)^2 x 2^20 units is beyond 2^62
    assert call([1, 1, 1], 3, P=ssm.align_params(min_inliers=50, z_max=1.0e5)) == 0


def test_kitti_sized_call_fits_the_sums():
    """5 x 467 k points at z_max = 80 m under KITTI's camera stay below 2^62 with the scales of the header (DESIGN.md s.18 derives it)"""
    cam = (607.2, 185.2, 718.9, 718.9, 1000.0)
    w, h = 1241, 376
    tx, ty = (max(abs(cam[0]), abs(w - 1 - cam[0])) + 0.5) / abs(cam[2]), (max(abs(cam[1]), abs(h - 1 - cam[1])) + 0.5) / abs(cam[3])
    jm = 80.0 * (1 + tx * tx + ty * ty) ** 0.5 * (1 + 2.0 ** -22)
    units = max(jm * jm, 0.25 * jm) * 2.0 ** A.S_HB + 1
    assert 5 * 467000 * units < 2.0 ** 62 / 100          # two decades of room
    assert 5 * 467000 * (0.25 ** 2 * 2.0 ** A.S_CHI + 1) < 2.0 ** 62


# what tests/align_ref.py alone reaches on the convergence scene (python tests/align_ref.py is not needed: the numbers are re-derived below and compared):
# final pose error against truth, metres and radians, for each planted error; the smallest eigenvalue of the final H is 787.7 with 33170 inliers
RESTATEMENT_FINAL = {"small": (1.443e-4, 0.948e-4), "medium": (1.447e-4, 0.945e-4), "large": (1.445e-4, 0.950e-4)}
# The floor of that error is the scene's quantisation: depth is cast in units of 1 mm and a point is associated with the nearest pixel's vertex, not with the
# surface under its own ray.  The restatement's 0.14 mm is a seventh of one depth unit.  The host function must equal the restatement bit for bit, so a margin
# above 1 only leaves room for the documented one-place difference a transcendental could make in the pose; a factor of two keeps the bound (0.29 mm, 0.19
# mrad) under a third of one depth unit, i.e. still below what the quantisation of a single pixel amounts to.
MARGIN = 2.0


@pytest.mark.parametrize("name", list(AC.CONV_PLANTED))
def test_convergence_against_truth(name):
    import semantic_slam_mapping_amd as ssm
    cs = AC.convergence_case(name)
    ref = A.align(cs["depth"], cs["camera"], cs["T_view"], cs["clouds"], cs["T_clouds"], **cs["params"])
    rt, rr = A.pose_error(ref["T_view"], cs["T_true"])
    assert abs(rt - RESTATEMENT_FINAL[name][0]) < 1e-6 and abs(rr - RESTATEMENT_FINAL[name][1]) < 1e-6, (rt, rr)          # the recorded figures are the restatement's
    assert np.linalg.eigvalsh(ref["H"])[0] > 700
    got = ssm.align_host(cs["depth"], cs["camera"], cs["T_view"], cs["clouds"], cs["T_clouds"], **cs["params"])
    pt, pr = A.pose_error(cs["T_view"], cs["T_true"])
    gt, gr = A.pose_error(got["T_view"], cs["T_true"])
    print(name, "planted", pt, pr, "restatement", rt, rr, "host", gt, gr)
    assert got["info"]["status"] == A.CONVERGED
    assert gt < pt and gr < pr
    assert gt <= MARGIN * RESTATEMENT_FINAL[name][0] and gr <= MARGIN * RESTATEMENT_FINAL[name][1]
    equal_to_ref(got, ref, name)


def test_the_road_constrains_height_pitch_and_roll():
    """which directions the Mapper test (host/test_align.cpp) may judge: a ground plane alone leaves sliding along the road (t_z), sideways (t_x) and yaw (r_y)
    without any constraint -- the three smallest eigenvalues of H vanish and their eigenvectors have no part in height (t_y), pitch (r_x) or roll (r_z) -- and
    the box beside the lane constrains sliding along the road and yaw through its faces but leaves sideways motion almost free (its eigenvalue stays below a
    twentieth of the next one).  So the planted error of that test lives in height, pitch and roll only, and sliding, sideways motion and yaw are not judged."""
    cam = (200.0, 40.0, 300.0, 300.0, 1000.0)
    w, h = 400, 120
    T0, T1 = AC.se3(), AC.se3(tz=0.5)

    def H_of(scene):
        d0 = AC.ray_cast(scene, T0, cam, w, h)
        d0[d0 > 40000] = 0
        ref = A.align(AC.ray_cast(scene, T1, cam, w, h), cam, T1, [AC.back_project(d0, cam)], [T0], max_iterations=1)
        assert ref["info"]["inliers_first"] > 10000
        return np.linalg.eigh(ref["H"])
    ev, vec = H_of(dict(planes=AC.ROAD["planes"], box=None))
    judged, free = [0, 2, 4], [1, 3, 5]          # delta = (omega, upsilon): r_x r_y r_z t_x t_y t_z
    assert (ev[:3] < 1e-4 * ev[3]).all() and ev[3] > 100          # (zero but for the depth quantisation of the normals)
    assert np.abs(vec[judged, :3]).max() < 1e-3 and np.abs(vec[free, 3:]).max() < 1e-3
    ev, vec = H_of(AC.ROAD)
    print("with the box:", ev)
    assert ev[0] > 1.0 and ev[0] < 0.05 * ev[1]
    assert np.abs(vec[judged, 0]).max() < 1e-3 and abs(vec[3, 0]) > 0.9          # the weakest direction is sideways motion (with a little yaw), nothing judged


def test_host_function_as_a_program_and_under_sanitizers():
    """host/test_align_core.cpp: a stand-alone program (its own main, no library, no device) over the host function, built plainly and with
    -fsanitize=address,undefined"""
    for target in ("test_align_core", "test_align_core_san"):
        subprocess.run(["make", "-s", "-C", HOST, target], check=True, capture_output=True, timeout=600)
        r = subprocess.run([os.path.join(HOST, target)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "ALL PASSED" in r.stdout and "FAIL" not in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


def test_kernels_neither_spill_nor_use_scratch():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    from test_abi import _resource_usage
    usage = _resource_usage("kernels_align.hip")
    for n in ("align_normals_kernel", "align_accumulate_kernel"):
        hit = [k for k in usage if n in k]
        assert len(hit) == 1, (n, sorted(usage))
        u = usage[hit[0]]
        assert u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0 and u.get("ScratchSize [bytes/lane]", 0) == 0, (hit[0], u)
