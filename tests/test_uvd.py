"""CPU tests of the U/V-disparity moving-object stage: ssm_uvd_process_host -- the whole of UVDisparity::Process from include/ssm/uvd_core.h
and the host steps, no GPU -- against the numpy restatement tests/uvd_ref.py, stage by stage.  Integer outputs are compared exactly.  The fitted line and
the pitches are compared within 1e-6 relative (both sides call libm on float inputs; one ulp of atan2 is not a defect); so that no discrete outcome can hinge
on that ulp the later stages of the restatement are fed the library's line, and the tests assert that no pixel's ground distance lies within 1e-4 of -14 and
no ROI comparison within 1e-6 of its bound."""
import os
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import uvd_ref as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "uvd.npz")
HOST = os.path.join(ROOT, "semantic_slam_mapping_amd", "host")
_cache = {}


def run_scene(name):
    """-> (library outputs incl. images and stages, restatement outputs, scene) of a scene of the condition list, computed once"""
    if name not in _cache:
        import semantic_slam_mapping_amd as ssm
        left, disp, m, fl, P = R.build_scene(name)
        u = ssm.UVDisparity(None, record=True, **P)
        got = u.process_host(left, disp, m, fl)
        h, w = disp.shape
        got["images"] = u.images(0, w, h)
        got["stages"] = {s: u.stage(0, s) for s in (1, 2, 3, 4, 5, 7, 8, 9, 10)}
        u.close()
        info = got["info"]
        ref = R.process(R.Kalman(), R.Kalman(), left, disp, m, fl, P, line=info["line"] if info["status"] == 0 else None)
        _cache[name] = (got, ref, (left, disp, m, fl, P))
    return _cache[name]


def same_bits(a, b):
    return np.asarray(a, np.float32).tobytes() == np.asarray(b, np.float32).tobytes()


def masks_of(buf, rows, cols):
    return buf.reshape(-1, rows, cols)


@pytest.mark.parametrize("name", list(R.SCENES))
def test_host_equals_restatement_stage_by_stage(name):
    got, ref, (left, disp, m, fl, P) = run_scene(name)
    info, img, st = got["info"], got["images"], got["stages"]
    h, w = disp.shape
    assert info["status"] == ref["status"]
    for k in ("moving", "roi", "ground"):
        assert np.array_equal(got[k], ref[k]), k
    assert info["n_moving"] == ref["n_moving"] == int((got["moving"] == 255).sum())
    if ref["status"] == R.SKIPPED:
        return
    vc = ref["v_cols"]
    assert info["v_cols"] == vc and info["u_rows"] == vc + 1
    if ref["status"] == R.TOO_LARGE:
        return
    assert np.array_equal(img["v_dis"][:, :vc], ref["v_dis"]) and not img["v_dis"][:, vc:].any()
    if "bin" not in ref:
        assert ref["status"] == R.NO_LINE and not got["moving"].any() and not got["roi"].any() and not got["ground"].any()
        return
    assert np.array_equal(st[1].reshape(h, vc), ref["blur"])
    assert np.array_equal(st[2].reshape(h, vc), ref["erode"])
    assert info["otsu_threshold"] == ref["otsu"]
    assert np.array_equal(st[3].reshape(h, vc), ref["bin"]) and np.array_equal(img["bin"][:, :vc], ref["bin"])
    assert st[4].reshape(-1, 2).tolist() == [list(p) for p in ref["pts"]] and info["n_line_points"] == len(ref["pts"])
    assert ref["status"] == 0
    # floats: the line on its own, the pitches through the library's line
    np.testing.assert_allclose(info["line"], ref["line"], rtol=1e-6)
    assert same_bits(info["slope"], ref["slope"]) and info["v_c"] == ref["v_c"]
    np.testing.assert_allclose(info["pitch_measured"], ref["pitch_measured"], rtol=1e-6)
    np.testing.assert_allclose(info["pitch_filtered"], ref["pitch_filtered"], rtol=1e-6)
    # no discrete outcome near its bound
    assert ref["ground_margin"] >= 1e-4 and ref["roi_margin"] >= 1e-6
    ur = vc + 1
    assert np.array_equal(st[5].reshape(ur, w), ref["u_raw"])
    assert np.array_equal(img["u_dis"][:ur], ref["u_adj"])
    assert got["matches"].tobytes() == ref["matches"].tobytes() and np.array_equal(got["inlier_flags"], ref["flags"])
    assert st[7].tolist() == ref["areas"] and info["n_seeds"] == len(ref["areas"])
    for sid, key, field in ((8, "found", "n_masks_found"), (9, "merged", "n_masks_merged"), (10, "kept", "n_masks_kept")):
        mk = masks_of(st[sid], ur, w)
        assert len(mk) == len(ref[key]) == info[field], key
        for a, b in zip(mk, ref[key]):
            assert np.array_equal(a, b), key
    assert np.array_equal(img["union"][:ur], ref["union"])


def test_scene_conditions():
    """the scenes do what the condition list asks of them, by the restatement alone"""
    ref = {n: run_scene(n)[1] for n in R.SCENES}
    px = 160 * 96
    assert ref["moving"]["status"] == 0 and len(ref["moving"]["kept"]) >= 1 and 0.01 * px <= ref["moving"]["n_moving"] <= 0.5 * px
    assert len(ref["verified_away"]["merged"]) > len(ref["verified_away"]["kept"])                      # a mask removed by verifyByInliers
    assert len(ref["merge"]["areas"]) >= 2 and len(ref["merge"]["found"]) > len(ref["merge"]["merged"])  # two seeds whose masks merge
    disp = run_scene("exact_max")[2][1]
    assert int(disp.max()) % 16 == 0 and (R.cv_round(disp[disp > 0].astype(np.float32) / np.float32(16)) == ref["exact_max"]["v_cols"]).any()   # the dropped bin
    assert ref["exact_max"]["status"] == 0
    assert 0 < ref["no_line"]["v_cols"] <= 26 and ref["no_line"]["status"] == R.NO_LINE
    assert int(run_scene("all_invalid")[2][1].max()) <= 0 and ref["all_invalid"]["status"] == R.NO_LINE
    assert int(run_scene("too_large")[2][1].max()) > 255 * 16 and ref["too_large"]["status"] == R.TOO_LARGE
    # some match is erased by filterInOut, some outlier survives it
    fl = ref["moving"]["flags"]
    assert (fl == 0).any() and (fl == 1).any()


def test_kalman_sequence_is_exact():
    """five frames through one object: a skipped frame and a NO_LINE frame leave both filters where they were; reset starts them again"""
    import semantic_slam_mapping_amd as ssm
    names = ["moving", "merge", "no_line", "exact_max", "verified_away"]
    P = R.scene_params()
    u = ssm.UVDisparity(None, record=True, **P)
    k1, k2 = R.Kalman(), R.Kalman()
    first = None
    for i, n in enumerate(names):
        left, disp, m, fl, _ = R.build_scene(n)
        skip = i == 1
        got = u.process_host(left, disp, m, fl, skip=skip)
        info = got["info"]
        before = k1.x
        ref = R.process(k1, k2, left, disp, m, fl, P, line=info["line"] if info["status"] == 0 else None, skip=skip)
        assert info["status"] == ref["status"] == (R.SKIPPED if skip else R.NO_LINE if n == "no_line" else 0)
        assert same_bits(info["pitch_filtered"], ref["pitch_filtered"]) and same_bits(info["pitch_filtered"], k1.x)
        if info["status"]:
            assert same_bits(k1.x, before) and not got["moving"].any() and not got["roi"].any() and not got["ground"].any()
        else:
            assert same_bits(info["pitch_measured"], ref["pitch_measured"]) and not same_bits(k1.x, before)
            assert np.array_equal(got["roi"], ref["roi"]) and np.array_equal(got["moving"], ref["moving"])       # the ROI mask depends on the filtered pitch
        first = first if first is not None else info["pitch_filtered"]
    assert same_bits(k1.x, k2.x)
    u.reset()
    left, disp, m, fl, _ = R.build_scene(names[0])
    assert same_bits(u.process_host(left, disp, m, fl)["info"]["pitch_filtered"], first)
    u.close()


def test_strided_input_and_null_outputs():
    import semantic_slam_mapping_amd as ssm
    left, disp, m, fl, P = R.build_scene("moving")
    h, w = disp.shape
    wide_l = np.full((h, w + 7), 99, np.uint8); wide_d = np.full((h, w + 7), 32000, np.int16)          # what lies beyond w must not be read
    wide_l[:, :w] = left; wide_d[:, :w] = disp
    u = ssm.UVDisparity(None, record=True, **P)
    a = u.process_host(left, disp, m, fl)
    u.reset()
    b = u.process_host(wide_l[:, :w], wide_d[:, :w], m, fl)
    for k in ("moving", "roi", "ground"):
        assert np.array_equal(a[k], b[k])
    assert a["info"].tobytes() == b["info"].tobytes()
    info = np.zeros(1, ssm.UVD_INFO_DTYPE)
    lc, dc = np.ascontiguousarray(left), np.ascontiguousarray(disp)
    assert u.lib.ssm_uvd_process_host(u.h, lc.ctypes.data, dc.ctypes.data, w, h, w, None, None, 0, None, None, None, info.ctypes.data) == 0
    assert u.lib.ssm_uvd_process_host(u.h, lc.ctypes.data, dc.ctypes.data, w, h, w - 1, None, None, 0, None, None, None, info.ctypes.data) == -1
    assert u.lib.ssm_uvd_process(u.h, lc.ctypes.data, dc.ctypes.data, w, h, w, None, None, 0, None, None, None, info.ctypes.data) == -1      # a host-only object has no device path
    u.close()


def test_golden_fixture():
    import semantic_slam_mapping_amd as ssm
    g = np.load(GOLDEN)
    for name in ("moving", "verified_away"):
        left, disp, m, fl, P = R.build_scene(name)
        assert np.array_equal(g[name + "_disp"], disp) and np.array_equal(g[name + "_left"], left)         # the generator still makes the committed scene
        u = ssm.UVDisparity(None, record=True, **P)
        got = u.process_host(left, disp, m, fl)
        img = u.images(0, disp.shape[1], disp.shape[0])
        u.close()
        for k in ("moving", "roi", "ground"):
            assert np.array_equal(got[k], g[f"{name}_{k}"]), k
        ur = int(g[name + "_ints"][1]) + 1
        assert np.array_equal(img["u_dis"][:ur], g[name + "_u_adj"]) and np.array_equal(img["union"][:ur], g[name + "_union"])
        info = got["info"]
        assert [int(info[k]) for k in ("status", "v_cols", "otsu_threshold", "n_line_points", "n_seeds", "n_masks_found", "n_masks_merged", "n_masks_kept", "n_moving")] == g[name + "_ints"].tolist()
        np.testing.assert_allclose([info["slope"], info["v_c"], info["pitch_measured"], info["pitch_filtered"]], g[name + "_floats"], rtol=1e-6)
        assert np.array_equal(got["inlier_flags"], g[name + "_flags"]) and np.array_equal(got["matches"]["dis_c"], g[name + "_dis_c"])


def test_params_default_is_the_reference():
    import ctypes as C
    import semantic_slam_mapping_amd as ssm
    from semantic_slam_mapping_amd._lib import UvdParams
    p = UvdParams()
    ssm.load().ssm_uvd_params_default(C.byref(p))
    assert (p.min_intense, p.min_disparity_raw, p.min_area, p.inlier_tolerance) == (32, 64, 40, 3)        # USegmentPars(), include/track.h:100
    assert (p.f, p.cu, p.cv, p.base, p.roi_x, p.roi_y, p.roi_z) == (718.8560, 607.1928, 185.2157, 0.532331858, 20, 5, 40)      # parameters.txt
    code = '#include "ssm_hip.h"\n#include <stdio.h>\nint main(){printf("%zu %zu", sizeof(ssm_uvd_params), sizeof(ssm_uvd_info));return 0;}'
    import subprocess, tempfile
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "layout")
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe], input=code, text=True, check=True)
        sizes = subprocess.run([exe], capture_output=True, text=True).stdout.split()
    from semantic_slam_mapping_amd._lib import UvdInfo
    assert sizes == [str(C.sizeof(UvdParams)), str(C.sizeof(UvdInfo))] and C.sizeof(UvdInfo) == ssm.UVD_INFO_DTYPE.itemsize


def test_host_header_keeps_the_reference_names():
    """include/ssm/uvdisparity.hpp and the Tracker members: the reference's class, method names and argument order (include/uvdisparity.hpp, include/track.h:135-138)"""
    inc = os.path.join(ROOT, "include", "ssm")
    want = {
        "uvdisparity.hpp": ["class UVDisparity", "struct USegmentPars", "struct ROI3D", "struct CalibPars", "inline void SetCalibPars(CalibPars& calib_par)",
                            "inline void SetROI3D(ROI3D& roi_3d)", "inline void SetUSegmentPars(int min_intense, int min_disparity_raw, int min_area)",
                            "inline void SetOutThreshold(double out_th)", "inline void SetInlierTolerance(int inlier_tolerance)", "inline void SetMinAdjustIntense(int min_adjust_intense)",
                            "cv::Mat Process(cv::Mat& img_L, cv::Mat& disp_sgbm, VisualOdometryStereo& vo, cv::Mat& xyz, cv::Mat& roi_mask, cv::Mat& ground_mask, double& pitch1, double& pitch2)",
                            "USegmentPars() : min_intense(32), min_disparity_raw(64), min_area(40)", "double x_max, y_max, z_max", "double f, c_x, c_y, b"],
        "track.h": ["ROI3D roi_3d = ROI3D(30, 10, 30);", "CalibPars calib_;", "UVDisparity uv_disparity;", "double pitch1 = 0, pitch2 = 0;", 'getData<int>("uv_disparity", 0)'],
        "batch_stereo_tracker.h": ["ssm_uvd_process_dev(", 'getData<int>("uv_disparity", 0)'],
        "uvd_core.h": ["triangulate", "roi_gate", "ground_pixel", "v_bin", "u_bin", "hist_u8", "u_adjust", "moving_test"],
    }
    for f, needles in want.items():
        src = open(os.path.join(inc, f)).read()
        for n in needles:
            assert n in src, (f, n)


def test_host_class_on_its_host_path_and_under_sanitizers():
    """host/test_uvd without arguments: class UVDisparity on a thread without a device context (ssm_uvd_process_host; no device call), as built against the
    library and, with AddressSanitizer and UndefinedBehaviorSanitizer, against the stub device that compiles the library's own host pipeline"""
    import subprocess
    subprocess.run(["make", "-s", "-C", HOST, "test_uvd"], check=True, capture_output=True, timeout=600)
    runs = [os.path.join(HOST, "test_uvd")]
    for san in ("asan", "ubsan"):
        subprocess.run(["make", "-s", "-C", HOST, f"SAN={san}", f"test_uvd_{san}"], check=True, capture_output=True, timeout=600)
        runs.append(os.path.join(HOST, f"test_uvd_{san}"))
    for exe in runs:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "ALL PASSED" in r.stdout and r.stdout.count("PASS ") == 7, r.stdout[-1500:] + r.stderr[-3000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
