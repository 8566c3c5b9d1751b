"""bench.py's command line and the --dump-outputs conversion, without a GPU: synthetic outputs of the shapes ssm_seq_process / ssm_stereo_seq_process
return (the device side of the dump runs in test_gpu_parity.py::test_bench_plain_line_and_output_dump)."""
import numpy as np
import pytest

import bench
from semantic_slam_mapping_amd.api import DMATCH_DTYPE, KEYPOINT_DTYPE, PMATCH_DTYPE, VOXEL_DTYPE


def _garbage(rng, shape, dtype):
    """bytes of any value (NaN and Inf included), like device memory past a frame's count"""
    dtype = np.dtype(dtype)
    return np.frombuffer(rng.integers(0, 256, int(np.prod(shape)) * dtype.itemsize, dtype=np.uint8).tobytes(), dtype=dtype).reshape(shape)


def test_plain_run_is_the_default_and_steps_are_checked():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    assert bench.parse_args(["--full", "--dump-outputs", "d"]).full is True
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_rgbd_dump_keeps_valid_rows_only_and_fits(tmp_path):
    rng = np.random.default_rng(3)
    F, cap, R = 1000, 1024, 5
    res = {"nkp": rng.integers(0, cap + 1, F).astype(np.int32), "kps": _garbage(rng, (F, cap), KEYPOINT_DTYPE), "desc": _garbage(rng, (F, cap, 32), np.uint8),
           "pos3d": _garbage(rng, (F, cap, 3), np.float32), "nmatch": rng.integers(-1, cap, (F, R)).astype(np.int32),
           "matches": _garbage(rng, (F, R, cap), DMATCH_DTYPE), "npoints": rng.integers(0, 300000, F).astype(np.int32)}
    for nvox in (0, 5000, 300000):
        vox = _garbage(rng, (nvox,), VOXEL_DTYPE)
        out = bench.rgbd_outputs(res, vox.tobytes(), R)
        assert all(a.dtype in (np.float32, np.float64) for a in out.values())
        assert sum(a.nbytes for a in out.values()) <= bench.DUMP_LIMIT_BYTES
        assert len(out["voxels"]) == min(nvox, 65536) and out["voxels"].shape[1] == 28
    idx = out["sample_frames"].astype(np.int64)
    assert np.array_equal(idx, bench.dump_sample(F, 32)) and len(idx) == 32 and np.all(np.diff(idx) > 0)
    for j, f in enumerate(idx):
        k = res["nkp"][f]
        assert np.all(out["descriptors"][j, k:] == 0) and np.array_equal(out["descriptors"][j, :k], res["desc"][f, :k].astype(np.float32))
        assert np.all(out["keypoints"][j, k:] == 0) and np.array_equal(out["keypoints"][j, :k, 5], res["kps"][f, :k]["octave"].astype(np.float32))
        for r in range(R):
            m = max(int(res["nmatch"][f, r]), 0)
            assert np.all(out["matches"][j, r, m:] == 0)
            assert np.array_equal(out["matches"][j, r, :m, 1], res["matches"][f, r, :m]["trainIdx"].astype(np.float32))
    assert np.array_equal(out["nkp"], res["nkp"].astype(np.float64)) and out["nmatch"].shape == (F, R)
    bench.write_outputs(str(tmp_path / "d"), out)
    assert np.array_equal(np.load(tmp_path / "d" / "voxels.npy"), out["voxels"])


def test_int64_fields_survive_the_float64_dump():
    v = np.array([0, -1, 2 ** 62 + 12345, -2 ** 63, 2 ** 63 - 1], np.int64)
    hi, lo = bench.split_int64(v).T
    assert ((hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)).view(np.int64).tolist() == v.tolist()


def test_stereo_dump_fits(tmp_path):
    rng = np.random.default_rng(4)
    F, mc, h, w = 256, 1000, 376, 1241
    res = {"nquad": rng.integers(-1, mc, F).astype(np.int32), "quad": _garbage(rng, (F, mc), PMATCH_DTYPE), "ncorners": rng.integers(0, mc, F).astype(np.int32),
           "corners": _garbage(rng, (F, mc, 2), np.float32), "disp": rng.integers(-16, 1280, (F, h, w)).astype(np.int16),
           "depth": rng.integers(0, 65535, (F, h, w)).astype(np.uint16), "tr": rng.standard_normal((F, 6)), "inliers": _garbage(rng, (F, mc), np.int32),
           "vo_result": np.stack([rng.integers(0, mc, F), rng.integers(0, 2, F)], 1).astype(np.int32), "rand_draws_used": 0}
    out = bench.stereo_outputs(res)
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert sum(a.nbytes for a in out.values()) <= bench.DUMP_LIMIT_BYTES
    for j, f in enumerate(out["sample_frames"].astype(np.int64)):
        assert np.all(out["quad"][j, max(res["nquad"][f], 0):] == 0) and np.all(out["corners"][j, res["ncorners"][f]:] == 0)
        assert np.all(out["inliers"][j, res["vo_result"][f, 0]:] == 0)
        assert np.array_equal(out["disparity"][j], res["disp"][f].astype(np.float32)) and np.array_equal(out["depth"][j], res["depth"][f].astype(np.float32))
    bench.write_outputs(str(tmp_path / "s"), out)


def test_dump_over_the_limit_is_refused(tmp_path):
    with pytest.raises(SystemExit):
        bench.write_outputs(str(tmp_path / "x"), {"big": np.zeros(bench.DUMP_LIMIT_BYTES // 8 + 1, np.float64)})
