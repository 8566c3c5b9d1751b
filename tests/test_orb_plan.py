"""The ORB planner (csrc/ssm_orb_plan.cpp: geometry, resize and group tables, the fused pyramid's bands, the blur table) from C++, without the library:
host/test_orb_plan.cpp links that one source and sweeps the configurations of test_pyramid_items.py and test_fast_tiling.py.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_standalone_planner_program():
    """(the same source builds with -fsanitize=address, undefined and thread: scripts/run_sanitizers.sh)"""
    exe = os.path.join(ROOT, "semantic_slam_mapping_amd", "host", "test_orb_plan")
    assert os.path.exists(exe), "host/test_orb_plan is missing: build() makes it"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "ALL PASSED" in r.stdout and "FAIL" not in r.stdout
