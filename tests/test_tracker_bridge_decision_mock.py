"""hip_bridge::FrameTrackerT::finishFrame (include/svo_dropin/frame_tracker_batch.h) on the CPU, on the self-contained twins
(android_svo_amd/host/svo_host.h), against a mock of the svo_hip_tracker_* entry points that records the calls: the structure step
and the keyframe decision are one device call and no optimize_structure call; positions and Point::last_structure_optim_ are
applied; the furthest keyframe's index is translated to the right frame before and after a keyframeRemoved; need_new_kf = -1
surfaces as overlap_valid == false; a refused device call returns false with the objects untouched.  Built plain and with the
address / undefined-behaviour sanitizers (a stand-alone host program).  The GPU run of the same template is
tests/test_gpu_keyframe_decision.py::test_host_twin_decides_on_the_device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_decision_bridge_against_a_mock_device(tmp_path, flags):
    exe = tmp_path / "tracker_decision_mock_test"
    src = os.path.join(ROOT, "tests", "host_mock", "tracker_decision_mock_test.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, "-I" + os.path.join(ROOT, "include"), src, "-o", str(exe), "-lpthread"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tracker decision mock test OK" in r.stdout
