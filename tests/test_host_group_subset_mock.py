"""hip_bridge::FrameTrackerGroupT::trackSome (include/svo_dropin/frame_tracker_batch.h) on the CPU against a mock device
(tests/host_mock_subset/group_subset_mock_test.cpp, on the mock tracker and the small world of
tests/host_mock/tracker_mock_test.cpp): ONE svo_hip_tracker_group_track_some call with the active list and the images in its
order; prepare, fetch and apply on the cameras of the call only; the entries of `out` and `overlap_kfs` of a camera that sits
out left alone.  Built plain and with the address / undefined-behaviour sanitizers (a stand-alone host program).  The GPU run
of the same template is tests/test_gpu_group_subset_cpp.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_track_some_against_a_mock_device(tmp_path, flags):
    exe = tmp_path / "group_subset_mock_test"
    src = os.path.join(ROOT, "tests", "host_mock_subset", "group_subset_mock_test.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, "-I" + os.path.join(ROOT, "include"), src, "-o", str(exe), "-lpthread"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "group subset mock test OK" in r.stdout
