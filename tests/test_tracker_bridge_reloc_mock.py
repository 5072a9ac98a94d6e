"""hip_bridge::FrameTrackerT::relocalize / setDeviceRelocalisation (include/svo_dropin/frame_tracker_batch.h) on the CPU, on the
self-contained twins (android_svo_amd/host/svo_host.h), against a mock of the svo_hip_tracker_* entry points that records the
calls: an accepted relocalisation is one device call and no upload; a refused gate leaves the gate's pose on the new frame; no
close keyframe changes nothing; a refusal of the device ends in the upload of the keyframe as last frame, as before; with the
switch off the new entry point is never called.  Built plain and with the address / undefined-behaviour sanitizers (a stand-alone
host program).  The GPU run of the same template is tests/test_gpu_relocalise.py::test_host_twin_relocalises."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_relocalisation_bridge_against_a_mock_device(tmp_path, flags):
    exe = tmp_path / "tracker_reloc_mock_test"
    src = os.path.join(ROOT, "tests", "host_mock", "tracker_reloc_mock_test.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, "-I" + os.path.join(ROOT, "include"), src, "-o", str(exe), "-lpthread"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tracker relocalisation mock test OK" in r.stdout
