"""hip_bridge::FrameTrackerT's incremental map mode (include/svo_dropin/frame_tracker_batch.h: setIncrementalMap) on the CPU, on
the self-contained twins of android_svo_amd/host/svo_host.h against a mock of the svo_hip_tracker_* entry points that records
the calls: one svo_hip_tracker_add_candidates for a grown candidate list, one svo_hip_tracker_promote_last_frame for a new
keyframe, the full upload after a refused call, and the unchanged call sequence with the mode off.  Built plain and with the
address / undefined-behaviour sanitizers (a stand-alone host program).  The GPU run of the same template is
tests/test_gpu_map_growth.py::test_host_twin_incremental_equals_default."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_frame_tracker_bridge_against_a_mock_device(tmp_path, flags):
    exe = tmp_path / "tracker_mock_test"
    src = os.path.join(ROOT, "tests", "host_mock", "tracker_mock_test.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, "-I" + os.path.join(ROOT, "include"), src, "-o", str(exe), "-lpthread"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tracker mock test OK" in r.stdout
