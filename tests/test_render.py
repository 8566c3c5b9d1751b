"""CPU tests of map rendering: ssm_render_host and ssm_render_compare_host -- the contract's arithmetic of include/ssm/render_core.h, one thread,
no GPU -- against the numpy restatement tests/render_ref.py exactly (every output array, the raw keys, every info field and count, the class image) on the
shared case list; the list's own properties (each boundary of the section is hit on both sides); refusals; the palette; the host functions and the PNG writer
as stand-alone C++ programs, the former also under AddressSanitizer + UndefinedBehaviorSanitizer; and the new kernels' register use."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import render_ref as R  # noqa: E402

HOST = os.path.join(ROOT, "semantic_slam_mapping_amd", "host")
CASES = list(R.cases())
_cache = {}


def ref_of(name):
    """-> (case, restatement), computed once and shared"""
    if name not in _cache:
        cs = R.cases()[name]()
        _cache[name] = (cs, R.run_case(cs))
    return _cache[name]


def host_render(cs, **kw):
    import semantic_slam_mapping_amd as ssm
    return ssm.render_host(cs["w"], cs["h"], cs["camera"], cs["T_view"], cs["clouds"], cs["T_clouds"], keys=True, **dict(cs["params"], **kw))


def equal_to_ref(got, ref, what=""):
    for f in ("keys", "depth", "bgr", "label", "index"):
        assert got[f].dtype == ref[f].dtype and np.array_equal(got[f], ref[f]), (what, f, np.argwhere(got[f] != ref[f])[:5])
    for f in R.INFO_FIELDS:
        assert got["info"][f] == ref["info"][f], (what, f, got["info"][f], ref["info"][f])


@pytest.mark.parametrize("name", CASES)
def test_host_equals_restatement(name):
    import semantic_slam_mapping_amd as ssm
    cs, ref = ref_of(name)
    before = [c.tobytes() for c in cs["clouds"]]
    got = host_render(cs)
    equal_to_ref(got, ref, name)
    assert [c.tobytes() for c in cs["clouds"]] == before
    dep, sem = ref["frame"]
    cmp_params = {k: v for k, v in cs["params"].items() if k in ("tol_abs", "tol_rel_ppm")}
    counts, cls = ssm.render_compare_host(got["depth"], got["label"], dep, sem, cs["camera"][4], class_image=True, **cmp_params)
    assert counts == ref["counts"], (name, counts, ref["counts"])
    assert np.array_equal(cls, ref["class"])
    assert sum(counts[f] for f in R.COMPARE_FIELDS[:5]) == counts["n_pixels"] == cs["w"] * cs["h"]
    assert counts["label_agree"] + counts["label_disagree"] + counts["label_unknown"] == counts["agree"]
    assert ssm.render_compare_host(got["depth"], got["label"], dep, sem, cs["camera"][4], **cmp_params) == counts


def test_cases_are_what_they_are_for():
    """the shapes of the case list do what their names say (this guards the list, not the library)"""
    cs, ref = ref_of("two_depths")
    assert ref["depth"][3, 4] == 1000 and ref["index"][3, 4] == 1 and ref["info"] == dict(n_in=4, n_visible=4, n_covered=2)
    for name, winner in (("equal_zq", 0), ("equal_zq_reversed", 2)):
        cs, ref = ref_of(name)
        assert {s["zq"] for s in ref["splats"][:3] + ref["splats"][2:5]} == {1000, 2000} and ref["index"][3, 4] == winner and ref["depth"][3, 4] == 1000
    cs, ref = ref_of("zq_limits")
    assert [None if s is None else s["zq"] for s in ref["splats"]] == [None, 1, 2, 65535, 65535, None, None, None, None]
    assert sorted(ref["depth"][ref["depth"] > 0].tolist()) == [1, 2, 65535, 65535]
    cs, ref = ref_of("z_range")
    assert [s is not None for s in ref["splats"]] == [True, False, True, False, True]
    cs, ref = ref_of("degenerate")
    assert all(s is None for s in ref["splats"][:16]) and ref["splats"][16] is not None and ref["info"]["n_visible"] == 1
    for name in ("borders_9x7", "borders_67x5"):
        cs, ref = ref_of(name)
        w, h = cs["w"], cs["h"]
        sp = ref["splats"]
        # z = 1: 1 and 2 outside reach in (s = 2), 3 outside is beyond max_radius; z = 2 (s = 1): 1 outside reaches in, 2 outside has an empty footprint
        assert all(s is not None and s["s"] == 2 for s in sp[:12]) and all(s is None for s in sp[12:18])
        assert all(s is not None and s["s"] == 1 for s in sp[18:30]) and all(s is None for s in sp[30:36])
        outside = lambda s: s["px"] < 0 or s["px"] > w - 1 or s["py"] < 0 or s["py"] > h - 1          # noqa: E731
        assert all(outside(s) for s in sp[:12] + sp[18:30])
        assert ref["info"]["n_visible"] == 12 + 6 + 2 and ref["info"]["n_in"] == 38
        for i, (x, y) in ((0, (0, 2)), (1, (w - 1, 2)), (2, (w // 2, 0)), (3, (w // 2, h - 1)), (4, (0, 0)), (5, (w - 1, h - 1))):
            assert ref["depth"][y, x] == 1000, (name, i)          # each border and both corners are reached from outside
    for r, want in ((0, [0, 0, 0, 0, 0, 0]), (3, [0, 1, 1, 2, 3, 3]), (8, [0, 1, 1, 2, 4, 8])):
        cs, ref = ref_of(f"sizes_r{r}")
        assert [s["s"] for s in ref["splats"]] == want
    for name in ("posed_67x5", "posed_9x7_m2", "posed_160x120_m3"):
        cs, ref = ref_of(name)
        info = ref["info"]
        assert 0 < info["n_covered"] and 0 < info["n_visible"] <= info["n_in"] and (info["n_visible"] < info["n_in"] or cs["h"] < 100), (name, info)
        assert not np.allclose(cs["T_view"], np.eye(4)) and not np.allclose(cs["T_clouds"][0], np.eye(4))
    cs, ref = ref_of("posed_160x120_m3")
    assert len(set((ref["index"][ref["index"] >= 0] // 700).tolist())) == 3 and {s["s"] for s in ref["splats"] if s} >= {1, 2}
    cs, ref = ref_of("three_clouds")
    assert [len(c) for c in cs["clouds"]] == [5, 0, 7] and (ref["index"] >= 5).any() and ((ref["index"] >= 0) & (ref["index"] < 5)).any()
    for name in ("empty_m0", "empty_m1"):
        cs, ref = ref_of(name)
        assert ref["info"] == dict(n_in=0, n_visible=0, n_covered=0) and (ref["keys"] == R.EMPTY).all() and (ref["index"] == -1).all() and (ref["label"] == 255).all()
        assert ref["counts"]["unrendered"] == cs["w"] * cs["h"]
    cs, ref = ref_of("categories")
    assert min(ref["counts"].values()) > 0, ref["counts"]
    dep = cs["frame"][0].astype(np.int64)
    zr = ref["depth"].astype(np.int64)
    judged = (zr > 0) & (dep > 0)
    front = (dep - zr - ref["tol"])[judged]          # > 0: in front
    behind = (zr - dep - ref["tol"])[judged]         # > 0: behind
    assert {0, 1} <= set(front.tolist()) and {0, 1} <= set(behind.tolist())
    assert ref["class"][0, :8].tolist() == [4, 2, 2, 2, 4, 3, 3, 3]
    seen = set()
    for name in CASES:
        seen |= set(np.unique(ref_of(name)[1]["class"]).tolist())
    assert seen == {0, 1, 2, 3, 4}


def test_label_colours_are_the_palette():
    import semantic_slam_mapping_amd as ssm
    lab = np.arange(256, dtype=np.uint8).reshape(4, 64)
    col = ssm.label_colours(lab)
    assert col.shape == (4, 64, 3) and col.dtype == np.uint8
    want = np.zeros((256, 3), np.uint8)
    want[:12] = np.array(R.PALETTE, np.uint8)
    assert np.array_equal(col.reshape(256, 3), want)
    assert np.array_equal(R.label_of_bgr(col)[0, :12], np.arange(12))          # the inverse of the lookup the comparison uses


def test_refusals():
    import semantic_slam_mapping_amd as ssm
    from semantic_slam_mapping_amd._lib import RenderParams, Camera
    lib = ssm.load()
    cs, _ = ref_of("posed_9x7_m2")
    nan, inf = float("nan"), float("inf")
    for kw in (dict(max_radius=-1), dict(max_radius=9), dict(point_size=-0.1), dict(point_size=nan), dict(point_size=inf), dict(z_min=-0.1), dict(z_min=nan), dict(z_min=inf),
               dict(z_max=-1.0), dict(z_max=nan), dict(z_max=inf), dict(tol_abs=-0.01), dict(tol_abs=nan), dict(tol_abs=inf), dict(tol_abs=2e6), dict(tol_rel_ppm=-1),
               dict(tol_rel_ppm=1000001)):
        with pytest.raises(ssm.SsmError) as e:
            host_render(cs, **kw)
        assert e.value.code == -1, kw          # SSM_E_INVAL
    for cam in ((0, 0, 64, 64, 0.0), (0, 0, 64, 64, -1.0), (0, 0, 64, 64, nan), (0, 0, nan, 64, 1000.0), (inf, 0, 64, 64, 1000.0), (0, 0, 64, 64, 2e6)):
        with pytest.raises(ssm.SsmError) as e:
            ssm.render_host(9, 7, cam, R.EYE, cs["clouds"], cs["T_clouds"])
        assert e.value.code == -1, cam
    bad = np.eye(4)
    bad[1, 3] = nan
    for Tv, Tc in ((bad, cs["T_clouds"]), (R.EYE, [cs["T_clouds"][0], bad])):
        with pytest.raises(ssm.SsmError) as e:
            ssm.render_host(9, 7, cs["camera"], Tv, cs["clouds"], Tc)
        assert e.value.code == -1
    for w, h in ((0, 7), (9, 0), (-1, 7), (1 << 13, (1 << 13) + 1)):
        with pytest.raises(ssm.SsmError) as e:
            ssm.render_host(w, h, cs["camera"], R.EYE, cs["clouds"], cs["T_clouds"])
        assert e.value.code == -1, (w, h)
    with pytest.raises(TypeError):
        ssm.render_host(9, 7, cs["camera"], R.EYE, cs["clouds"], cs["T_clouds"], radius=2)
    P = RenderParams(); lib.ssm_render_params_default(C.byref(P))
    assert (P.point_size, P.max_radius, P.z_min, P.z_max, P.tol_abs, P.tol_rel_ppm) == tuple(R.DEFAULTS[k] for k in ("point_size", "max_radius", "z_min", "z_max", "tol_abs", "tol_rel_ppm"))
    # m < 0, a negative count, and 2^32 points in all (refused before a point is read)
    cam = Camera(*cs["camera"]); T = np.ascontiguousarray(np.eye(4).reshape(16)); T3 = np.ascontiguousarray(np.tile(T, 3))
    one = cs["clouds"][0]
    ptrs = (C.c_void_p * 3)(one.ctypes.data, one.ctypes.data, one.ctypes.data)
    call = lambda n, m: lib.ssm_render_host(9, 7, C.byref(cam), T.ctypes.data, ptrs, np.ascontiguousarray(n, np.int32).ctypes.data, T3.ctypes.data, m, None, None, None, None, None, None, None)  # noqa: E731
    assert call([1, 1, 1], 3) == 0 and call([1, 1, 1], 0) == 0
    assert call([1, 1, 1], -1) == -1 and call([1, -1, 1], 3) == -1
    big = 2 ** 31 - 1
    assert call([big, big, 2], 3) == -1          # 2^32 exactly
    # the comparison
    rd = np.zeros((7, 9), np.uint16); rl = np.zeros((7, 9), np.uint8); sem = np.zeros((7, 9, 3), np.uint8)
    assert ssm.render_compare_host(rd, rl, rd, sem, 1000.0)["unrendered"] == 63
    for kw, scale in ((dict(tol_abs=-1.0), 1000.0), (dict(tol_abs=nan), 1000.0), (dict(tol_rel_ppm=-1), 1000.0), (dict(tol_rel_ppm=1000001), 1000.0), ({}, 0.0), ({}, nan), ({}, 2e6)):
        with pytest.raises(ssm.SsmError) as e:
            ssm.render_compare_host(rd, rl, rd, sem, scale, **kw)
        assert e.value.code == -1, (kw, scale)
    with pytest.raises(ValueError):
        ssm.render_compare_host(rd, rl, rd[:3], sem, 1000.0)


def test_host_functions_as_a_program_and_under_sanitizers():
    """host/test_render_core.cpp: a stand-alone program (its own main, no library, no device) over the host functions, built plainly and with
    -fsanitize=address,undefined"""
    for target in ("test_render_core", "test_render_core_san"):
        subprocess.run(["make", "-s", "-C", HOST, target], check=True, capture_output=True, timeout=600)
        r = subprocess.run([os.path.join(HOST, target)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "ALL PASSED" in r.stdout and "FAIL" not in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


def test_png_writer_round_trips():
    """host/test_png_write.cpp: imwritePNG then imreadPNG on 8-bit 1- and 3-channel and 16-bit images, widths 1 and 67 among them; also under the sanitizers"""
    for target in ("test_png_write", "test_png_write_san"):
        subprocess.run(["make", "-s", "-C", HOST, target], check=True, capture_output=True, timeout=600)
        r = subprocess.run([os.path.join(HOST, target)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "ALL PASSED" in r.stdout and "FAIL" not in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


def test_kernels_neither_spill_nor_use_scratch():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    from test_abi import _resource_usage
    usage = _resource_usage("kernels_render.hip")
    for n in ("render_clear_kernel", "render_splat_kernel", "render_resolve_kernel", "render_compare_kernel", "render_counts_clear_kernel"):
        hit = [k for k in usage if n in k]
        assert len(hit) == 1, (n, sorted(usage))
        u = usage[hit[0]]
        assert u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0 and u.get("ScratchSize [bytes/lane]", 0) == 0, (hit[0], u)
