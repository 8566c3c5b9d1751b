"""The bulk tracker's host state machine (csrc/ssm_track_host.cpp: the lazy downloads, initFirstFrame / lostRecover / trackRefFrame over the deque, the state
block before and after a run on the device, the cluster's downgrade) from C++, without the library: host/test_track.cpp links that one source and supplies the
downloads, the on-demand matcher and the device leg's hooks over host arrays, with a host model of the chain kernel behind the run hook.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_standalone_tracker_program():
    """(the same source builds with -fsanitize=address, undefined and thread: scripts/run_sanitizers.sh)"""
    exe = os.path.join(ROOT, "semantic_slam_mapping_amd", "host", "test_track")
    assert os.path.exists(exe), "host/test_track is missing: build() makes it"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-6000:], r.stderr[-2000:])
    assert r.returncode == 0 and "ALL PASSED" in r.stdout and "FAIL" not in r.stdout
