"""hip_bridge::FrameTrackerT::setPointCompaction (include/svo_dropin/frame_tracker_batch.h) on the CPU, on the self-contained twins
(android_svo_amd/host/svo_host.h), against a mock of the svo_hip_tracker_* entry points that records the calls and keeps a point
table with a capacity: option off, a capacity refusal ends in the full upload as before; option on, the bridge compacts once,
repeats the call once, uploads nothing and sends the new indices afterwards; a second refusal, a refused compaction and a device
that kept other points than the host holds end in the full upload; a refused promotion takes the same path.  Built plain and
with the address / undefined-behaviour sanitizers (a stand-alone host program).  The GPU run of the same template is
tests/test_gpu_map_compaction.py::test_host_twin_compacts_points."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_point_compaction_bridge_against_a_mock_device(tmp_path, flags):
    exe = tmp_path / "tracker_compact_mock_test"
    src = os.path.join(ROOT, "tests", "host_mock", "tracker_compact_mock_test.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, "-I" + os.path.join(ROOT, "include"), src, "-o", str(exe), "-lpthread"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tracker compaction mock test OK" in r.stdout
