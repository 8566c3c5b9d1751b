"""The schedule of the sequence calls (csrc/ssm_seq_plan.cpp: which lane every ORB -> match chain, the map stage and SGBM of a sub-batch run on, which chains'
events a matcher waits for, which lanes a call forks and joins) from C++, without the library: host/test_seq_plan.cpp links that one source and checks its
decision tables and, with the two executors' loops restated over model streams and events, the ordering the plans give over every shape.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "semantic_slam_mapping_amd", "host")


def test_standalone_seq_plan_program():
    """(the same source builds with -fsanitize=address, undefined and thread: make SAN=... san in host/)"""
    exe = os.path.join(HOST, "test_seq_plan")
    assert os.path.exists(exe), "host/test_seq_plan is missing: build() makes it"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-6000:], r.stderr[-2000:])
    assert r.returncode == 0 and "ALL PASSED" in r.stdout and "FAIL" not in r.stdout


def test_seq_plan_program_under_sanitizers():
    """the stand-alone program (its own main, no library, no device) built with -fsanitize=address,undefined"""
    subprocess.run(["make", "-s", "-C", HOST, "test_seq_plan_san"], check=True, capture_output=True, timeout=600)
    r = subprocess.run([os.path.join(HOST, "test_seq_plan_san")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout and "FAIL" not in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
