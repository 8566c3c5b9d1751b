"""exp_mapping --train-vocab on the GPU (host/exp_mapping.cpp, trainVocabulary in include/ssm/looper.h): on the synthetic sequence that revisits its start (the
one tests/test_gpu_pgo_host.py drives: parameters_test.txt with 40 frames) the driver collects the key-frames' ORB descriptors, trains a vocabulary and writes
it; the per-frame loop (descriptors from the frames) and the --batched loop (descriptors brought down from the chunk's device tables) must write the same file
and print the same vocab_nodes / vocab_words / vocab_fnv; the flag and the key looper_train_vocab are the same thing; the file loads, its arrays hash to the
printed vocab_fnv, and a second run with --loops and that file as looper_vocab_file finds loop candidates."""
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
HOST = os.path.join(ROOT, "semantic_slam_mapping_amd", "host")
TRAIN = "\nlooper_train_k=10\nlooper_train_L=3\nlooper_train_iters=32\ntracker_chunk=10\nssm_max_batch=4\n"


def _run_driver(tmp_path, name, extra, flags):
    d = tmp_path / name
    d.mkdir()
    prm = d / "parameters.txt"
    base = open(os.path.join(HOST, "parameters_test.txt")).read().replace("end_index=8", "end_index=40").replace("map_output=/tmp/ssm_test_map.pcd", f"map_output={d}/map.pcd")
    prm.write_text(base + extra)
    r = subprocess.run([os.path.join(HOST, "exp_mapping"), str(prm), *flags], capture_output=True, text=True, timeout=600)
    print(r.stdout[-1500:], r.stderr[-1500:])
    assert r.returncode == 0
    return r.stdout


def _field(out, key):
    toks = out.split()
    return toks[toks.index(key) + 1]


def _fnv(*arrays):
    h = 0xCBF29CE484222325
    for a in arrays:
        for b in np.ascontiguousarray(a).tobytes():
            h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_driver_trains_writes_and_the_looper_uses_it(tmp_path):
    import semantic_slam_mapping_amd as ssm
    fa, fb, fk = (str(tmp_path / f"voc_{x}.txt") for x in "abk")
    plain = _run_driver(tmp_path, "plain", TRAIN, [])
    a = _run_driver(tmp_path, "perframe", TRAIN, ["--train-vocab", fa])
    b = _run_driver(tmp_path, "batched", TRAIN, ["--batched", "--train-vocab", fb])
    k = _run_driver(tmp_path, "key", TRAIN + f"looper_train_vocab={fk}\n", [])
    assert "vocab_nodes" not in plain
    for key in ("frames", "keyframes", "pose_fnv"):
        assert _field(a, key) == _field(plain, key), key                     # training changes nothing else
    for key in ("keyframes", "vocab_nodes", "vocab_words", "vocab_fnv"):
        assert _field(a, key) == _field(b, key) == _field(k, key), key
    assert open(fa, "rb").read() == open(fb, "rb").read() == open(fk, "rb").read()
    v = ssm.Vocabulary(fa)
    assert (v.k, v.L) == (10, 3) and v.nodes == int(_field(a, "vocab_nodes")) and v.words == int(_field(a, "vocab_words")) and v.words > 100
    assert _fnv(*v.arrays()) == int(_field(a, "vocab_fnv"), 16)
    v.close()
    loops = _run_driver(tmp_path, "loops", TRAIN + f"looper_vocab_file={fa}\nlooper_min_sim_score=0.05\nlooper_min_interval=3\n", ["--loops"])
    assert int(_field(loops, "loop_candidates")) > 0
