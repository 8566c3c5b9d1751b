"""CPU tests of the semantic-motion fusion: ssm_motion_fuse_host -- the contract's arithmetic of include/ssm/motion_fuse_core.h with two flood
fills, no GPU -- against the scipy restatement tests/motion_fuse_ref.py byte for byte (mask, labels, area, overlap, cand, counters) on the shared case list;
what the shapes of that list are there for, asserted on the restatement itself; the host function as a stand-alone C++ program, also under AddressSanitizer +
UndefinedBehaviorSanitizer; and the new kernels' register use."""
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import motion_fuse_ref as R  # noqa: E402

HOST = os.path.join(ROOT, "semantic_slam_mapping_amd", "host")
_cache = {}


def tile():
    import semantic_slam_mapping_amd as ssm
    return ssm.motion_fuse_tile()


def ref_of(name):
    """-> (case, restatement), computed once and shared"""
    if name not in _cache:
        table = R.FULL if name in R.FULL else R.cases(*tile())
        case = table[name]()
        _cache[name] = (case, R.fuse(*case))
    return _cache[name]


def equal_to_ref(got, ref):
    mask, info, rec = got
    assert np.array_equal(rec["cand"], ref["cand"]), "cand"
    assert np.array_equal(rec["labels"], ref["labels"]), "labels"
    assert np.array_equal(rec["area"], ref["area"]), "area"
    assert np.array_equal(rec["overlap"], ref["overlap"]), "overlap"
    assert info == ref["info"], (info, ref["info"])
    assert np.array_equal(mask, ref["mask"]), "mask"


CASES = list(R.cases(64, 16))          # the names do not depend on the tile


def test_tile_constant_is_exported():
    tw, th = tile()
    assert tw >= 8 and th >= 8 and sorted(R.cases(tw, th)) == sorted(CASES)


@pytest.mark.parametrize("name", CASES + list(R.FULL))
def test_host_equals_restatement(name):
    import semantic_slam_mapping_amd as ssm
    (sem, motion, at, ot), ref = ref_of(name)
    equal_to_ref(ssm.motion_fuse_host(sem, motion, at, ot, record=True), ref)
    # a superset of the always-moving mask, which is the whole answer without motion
    assert not (ref["always"] & ~ref["mask"]).any()
    mask0, info0 = ssm.motion_fuse_host(sem, None, at, ot)
    assert np.array_equal(mask0, ref["always"]) and info0["confirmed"] == 0 and info0["added"] == 0 and info0["blobs"] == ref["info"]["blobs"]


def test_cases_are_what_they_are_for():
    """the shapes of the case list do what their names say (on the restatement: this guards the list, not the library)"""
    tw, th = tile()
    blobs = lambda n: ref_of(n)[1]["info"]["blobs"]  # noqa: E731
    r = ref_of("lattice")[1]
    assert blobs("lattice") == 1 and (r["labels"] >= 0).sum() > (r["cand"] == 255).sum()          # corner contacts join; the enclosed zero boxes are filled
    zeros = r["cand"] == 0
    from scipy import ndimage
    assert ndimage.label(zeros)[1] > 20                                                            # 4-connected, the zero boxes are all separate
    assert blobs("diagonals") == 2
    r = ref_of("diagonal_ring")[1]
    assert blobs("diagonal_ring") == 1 and (r["labels"] >= 0).sum() > (r["cand"] == 255).sum() + 100   # the diamond's inside is a hole, and filled
    r = ref_of("ring_with_island")[1]
    assert blobs("ring_with_island") == 1 and r["info"]["added"] > 0
    assert blobs("cross") == 1 and blobs("merging_boxes") == 3 and blobs("serpentine_blob") == 1
    r = ref_of("serpentine_zeros")[1]
    corridor = r["labels"] < 0
    assert blobs("serpentine_zeros") >= 1 and corridor.sum() > 3 * tw and ndimage.label(corridor)[1] == 1 and (r["cand"] == 0).sum() > corridor.sum()
    r = ref_of("border_hole")[1]
    assert blobs("border_hole") == 2 and sorted(r["area"][r["area"] > 0])[0] < sorted(r["area"][r["area"] > 0])[1]      # the C is not filled, the ring is
    assert ref_of("all_zero")[1]["info"]["blobs"] == 0 and ref_of("all_set")[1]["info"] == dict(blobs=1, large=1, confirmed=1, added=(th + 5) * (tw + 9))
    # the decision's edges
    assert ref_of("area_eq_thres")[1]["info"] == dict(blobs=1, large=0, confirmed=0, added=0)
    assert ref_of("area_thres_plus_1")[1]["info"] == dict(blobs=1, large=1, confirmed=1, added=25)
    (sem, motion, at, ot), r = ref_of("overlap_143")
    assert r["area"].max() == 999 and r["overlap"].max() == 143 and (motion == 254).sum() > 0 and r["info"]["confirmed"] == 1
    r = ref_of("overlap_142")[1]
    assert r["overlap"].max() == 142 and r["info"]["confirmed"] == 0 and r["info"]["large"] == 1
    assert np.float64(np.float32(143) / np.float32(1000)) > 0.143 and not (143 / 1000 > 0.143)     # float, then double: the contract's compare


def test_strided_rows_and_arguments():
    import ctypes as C
    import semantic_slam_mapping_amd as ssm
    from semantic_slam_mapping_amd._lib import MotionFuseParams, MotionFuseInfo
    (sem, motion, at, ot), ref = ref_of("size_67x35")
    h, w = sem.shape[:2]
    wide = np.full((h, w * 3 + 13), 7, np.uint8)
    wide[:, :w * 3] = sem.reshape(h, w * 3)
    lib = ssm.load()
    P = MotionFuseParams(at, 0, ot); I = MotionFuseInfo(); mask = np.zeros((h, w), np.uint8)
    assert lib.ssm_motion_fuse_host(wide.ctypes.data, motion.ctypes.data, w, h, wide.strides[0], C.byref(P), mask.ctypes.data, C.byref(I), None, None, None, None) == 0
    assert np.array_equal(mask, ref["mask"]) and I.confirmed == ref["info"]["confirmed"]
    assert lib.ssm_motion_fuse_host(wide.ctypes.data, None, w, h, w * 3 - 1, C.byref(P), mask.ctypes.data, None, None, None, None, None) == -1      # SSM_E_INVAL
    assert lib.ssm_motion_fuse_host(None, None, w, h, w * 3, None, mask.ctypes.data, None, None, None, None, None) == -1
    lib.ssm_motion_fuse_params_default(C.byref(P))
    assert (P.area_thres, P.overlay_thres) == (1000, 0.143)


def test_host_function_as_a_program_and_under_sanitizers():
    """host/test_motion_fuse_core.cpp: a stand-alone program (its own main, no library, no device) over the host function, built plainly and with
    -fsanitize=address,undefined"""
    for target in ("test_motion_fuse_core", "test_motion_fuse_core_san"):
        subprocess.run(["make", "-s", "-C", HOST, target], check=True, capture_output=True, timeout=600)
        r = subprocess.run([os.path.join(HOST, target)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "ALL PASSED" in r.stdout and "FAIL" not in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


def test_kernels_neither_spill_nor_use_scratch():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    from test_abi import _resource_usage
    usage = _resource_usage("kernels_motion_fuse.hip")
    names = ["mf_class_kernel", "mf_local_kernelILi4ELb1E", "mf_local_kernelILi8ELb0E", "mf_merge_kernelILi4ELb1E", "mf_merge_kernelILi8ELb0E",
             "mf_flatten_kernelILb1E", "mf_flatten_kernelILb0E", "mf_paint_kernel"]
    for n in names:
        hit = [k for k in usage if n in k]
        assert len(hit) == 1, (n, sorted(usage))
        u = usage[hit[0]]
        assert u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0 and u.get("ScratchSize [bytes/lane]", 0) == 0, (hit[0], u)
