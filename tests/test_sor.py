"""CPU tests of the statistical outlier removal: ssm_sor_filter_host -- the contract's arithmetic of include/ssm/sor_core.h over a ladder of
grids, one thread, no GPU -- against the brute-force restatement tests/sor_ref.py exactly (mean_dist, keep, the kept points, every info field a brute force
has) on the shared case list; the first cell size as a pure tuning parameter; planted outliers; refusals; the host function as a stand-alone C++ program, also
under AddressSanitizer + UndefinedBehaviorSanitizer; and the new kernels' register use."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sor_ref as R  # noqa: E402

HOST = os.path.join(ROOT, "semantic_slam_mapping_amd", "host")
_cache = {}


def chunk():
    import semantic_slam_mapping_amd as ssm
    return ssm.sor_chunk()


def ref_of(name):
    """-> (case, restatement), computed once and shared"""
    if name not in _cache:
        case = R.cases(chunk())[name]()
        _cache[name] = (case, R.sor(case[0], case[1], case[2]))
    return _cache[name]


def equal_to_ref(got, ref, what=""):
    pts, info, rec = got
    assert np.array_equal(rec["mean_dist"].view(np.uint32), ref["mean_dist"].view(np.uint32)), what + " mean_dist"
    assert np.array_equal(rec["keep"], ref["keep"]), what + " keep"
    for f in R.INFO_FIELDS:
        assert info[f] == ref["info"][f], (what, f, info[f], ref["info"][f])
    assert pts.tobytes() == ref["points"].tobytes(), what + " points"


CASES = list(R.cases(512))          # the names do not depend on the chunk


def test_chunk_constant_is_exported():
    assert chunk() >= 64 and sorted(R.cases(chunk())) == sorted(CASES)
    assert len(ref_of("one_cell")[0][0]) > 2 * chunk()


@pytest.mark.parametrize("name", CASES)
def test_host_equals_restatement(name):
    import semantic_slam_mapping_amd as ssm
    (pts, k, mul, cell), ref = ref_of(name)
    pts0 = pts.copy()
    got = ssm.sor_filter_host(pts, k, mul, cell, record=True)
    equal_to_ref(got, ref)
    assert pts.tobytes() == pts0.tobytes()
    info = got[1]
    assert info["n_in"] == len(pts) and info["n_kept"] == len(got[0]) and (info["levels"] >= 1) == (not info["too_few"])


@pytest.mark.parametrize("name", ["random_3000", "duplicates", "non_finite", "doubling_line", "far_clusters", "k_cluster_beside_far", "cell_multiples", "k_64", "frame_160x120"])
def test_first_cell_size_changes_no_output(name):
    import semantic_slam_mapping_amd as ssm
    (pts, k, mul, _), ref = ref_of(name)
    levels = set()
    for cell in R.CELLS:
        got = ssm.sor_filter_host(pts, k, mul, cell, record=True)
        equal_to_ref(got, ref, f"cell {cell}")
        levels.add(got[1]["levels"])
    assert len(levels) > 1          # the ladder did differ


def test_cases_are_what_they_are_for():
    """the shapes of the case list do what their names say (this guards the list, not the library)"""
    import semantic_slam_mapping_amd as ssm
    r = ref_of("identical")[1]
    assert r["info"]["threshold"] == 0.0 and r["keep"].all()
    assert ref_of("n_30")[1]["info"]["too_few"] == 1 and ref_of("n_31")[1]["info"]["too_few"] == 0 and ref_of("n_0")[1]["info"]["too_few"] == 1
    r = ref_of("non_finite")[1]
    assert r["info"]["n_finite"] == 297 and not r["keep"][[17, 120, 299]].any()
    r = ref_of("non_finite_too_few")[1]
    assert r["info"]["too_few"] == 1 and list(r["keep"]) == [1, 0, 1, 0, 1]
    (pts, k, mul, cell), _ = ref_of("doubling_line")
    assert ssm.sor_filter_host(pts, k, mul, cell)[1]["levels"] >= 15
    (pts, k, mul, cell), _ = ref_of("far_clusters")
    assert (pts["x"].max() - pts["x"].min()) / cell > 2 ** 21
    (pts, k, mul, cell), r = ref_of("k_cluster_beside_far")
    assert (r["mean_dist"][:k] > 1.0).all() and (r["mean_dist"][k:] < 0.1).all() and not r["keep"][:k].any()
    assert 0 < ref_of("mul_0.0")[1]["info"]["n_kept"] < ref_of("mul_1.0")[1]["info"]["n_kept"] < ref_of("mul_2.5")[1]["info"]["n_kept"]
    assert 0 < ref_of("frame_160x120")[1]["info"]["n_kept"] < ref_of("frame_160x120")[1]["info"]["n_finite"]


def test_planted_outliers_are_removed():
    import semantic_slam_mapping_amd as ssm
    pts, at = R.planted()
    out, info, rec = ssm.sor_filter_host(pts, record=True)
    assert not rec["keep"][at].any()
    plane = np.ones(len(pts), bool)
    plane[at] = False
    assert rec["keep"][plane].mean() > 0.9 and info["n_kept"] == rec["keep"].sum()
    assert out.tobytes() == pts[rec["keep"] == 1].tobytes()


def test_refusals():
    import semantic_slam_mapping_amd as ssm
    from semantic_slam_mapping_amd._lib import SorParams, SorInfo
    lib = ssm.load()
    pts = R.cloud(R._uniform(100, 20))
    for kw in (dict(mean_k=0), dict(mean_k=65), dict(mean_k=-3), dict(cell=-1.0), dict(cell=float("nan")), dict(cell=float("inf")), dict(stddev_mul=float("nan")), dict(stddev_mul=float("inf"))):
        with pytest.raises(ssm.SsmError) as e:
            ssm.sor_filter_host(pts, **kw)
        assert e.value.code == -1, kw          # SSM_E_INVAL
    far = R.cloud(np.float32([[0, 0, 0], [10000, 0, 0], [0, 10000, 0], [0, 0, 10000], [10000, 10000, 0]]))          # mean distances beyond the statistics grid
    with pytest.raises(ssm.SsmError) as e:
        ssm.sor_filter_host(far, mean_k=2)
    assert e.value.code == -1
    with pytest.raises(ValueError):
        R.sor(far, 2, 1.0)
    P = SorParams(); lib.ssm_sor_params_default(C.byref(P))
    assert (P.mean_k, P.cell, P.stddev_mul) == (30, 0.0, 1.0)
    out = np.zeros(100, R.POINT_DTYPE); got = C.c_int(0); I = SorInfo()
    assert lib.ssm_sor_filter_host(None, 100, None, out.ctypes.data, 100, C.byref(got), None, None, None) == -1
    assert lib.ssm_sor_filter_host(pts.ctypes.data, 100, None, out.ctypes.data, 100, None, None, None, None) == -1
    assert lib.ssm_sor_filter_host(pts.ctypes.data, -1, None, out.ctypes.data, 100, C.byref(got), None, None, None) == -1
    assert lib.ssm_sor_filter_host(pts.ctypes.data, 100, None, out.ctypes.data, 5, C.byref(got), C.byref(I), None, None) == -4 and got.value == I.n_kept > 5      # SSM_E_CAPACITY
    assert lib.ssm_sor_filter_host(pts.ctypes.data, 100, None, out.ctypes.data, 100, C.byref(got), None, None, None) == 0 and got.value == I.n_kept


def test_host_function_as_a_program_and_under_sanitizers():
    """host/test_sor_core.cpp: a stand-alone program (its own main, no library, no device) over the host function, built plainly and with
    -fsanitize=address,undefined"""
    for target in ("test_sor_core", "test_sor_core_san"):
        subprocess.run(["make", "-s", "-C", HOST, target], check=True, capture_output=True, timeout=600)
        r = subprocess.run([os.path.join(HOST, target)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "ALL PASSED" in r.stdout and "FAIL" not in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


def test_kernels_neither_spill_nor_use_scratch():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    from test_abi import _resource_usage
    usage = _resource_usage("kernels_sor.hip")
    for n in ("sor_bounds_kernel", "sor_keys_kernel", "sor_gather_kernel", "sor_search_kernel", "sor_stats_kernel", "sor_keep_kernel", "sor_compact_kernel"):
        hit = [k for k in usage if n in k]
        assert len(hit) == 1, (n, sorted(usage))
        u = usage[hit[0]]
        assert u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0 and u.get("ScratchSize [bytes/lane]", 0) == 0, (hit[0], u)
