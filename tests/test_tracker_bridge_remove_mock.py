"""hip_bridge::FrameTrackerT::keyframeRemoved (include/svo_dropin/frame_tracker_batch.h) and the removal functions of the
self-contained twins (android_svo_amd/host/svo_host.h: Map::safeDeleteFrame and what it calls) on the CPU, against a mock of the
svo_hip_tracker_* entry points that records the calls: one svo_hip_tracker_remove_keyframe for a keyframe that left, the
renumbered keyframes in what follows, the freed slot reused, the full upload after a refusal or after counts that disagree, and
mapChanged() with the mode off.  Built plain and with the address / undefined-behaviour sanitizers (a stand-alone host program).
The GPU run of the same template is tests/test_gpu_map_removal.py::test_host_twin_removes_keyframes_in_place."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_keyframe_removal_bridge_against_a_mock_device(tmp_path, flags):
    exe = tmp_path / "tracker_remove_mock_test"
    src = os.path.join(ROOT, "tests", "host_mock", "tracker_remove_mock_test.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, "-I" + os.path.join(ROOT, "include"), src, "-o", str(exe), "-lpthread"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tracker removal mock test OK" in r.stdout
