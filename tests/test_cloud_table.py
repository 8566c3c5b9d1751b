"""CPU test of the cloud-segment table's host half (csrc/ssm_cloud_table.cpp): the numbering of a call's points, each block's first cloud and the
point count of the host-array calls, as a stand-alone C++ program, also under AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "semantic_slam_mapping_amd", "host")


def test_builder_as_a_program_and_under_sanitizers():
    """host/test_cloud_table.cpp: a stand-alone program (its own main, no library, no device) over the builder, built plainly and with
    -fsanitize=address,undefined"""
    for target in ("test_cloud_table", "test_cloud_table_san"):
        subprocess.run(["make", "-s", "-C", HOST, target], check=True, capture_output=True, timeout=600)
        r = subprocess.run([os.path.join(HOST, target)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "ALL PASSED" in r.stdout and "FAIL" not in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
