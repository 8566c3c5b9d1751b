"""CPU test of the matrix-core matcher's key arithmetic (csrc/match_keys.h): the exponent the launchers choose for every row length, the bounds that keep
the accumulator exact, the switch to the VALU matcher above 32768 descriptors, and the kernel's running pair in f32 against a sorted list -- as a stand-alone C++ program
in the host test build, also under AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "semantic_slam_mapping_amd", "host")


def test_key_arithmetic_as_a_program_and_under_sanitizers():
    """host/test_match_keys.cpp: a stand-alone program (its own main, no library, no device), built plainly and with -fsanitize=address,undefined"""
    for target in ("test_match_keys", "test_match_keys_san"):
        subprocess.run(["make", "-s", "-C", HOST, target], check=True, capture_output=True, timeout=600)
        r = subprocess.run([os.path.join(HOST, target)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "ALL PASSED" in r.stdout and "FAIL" not in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
