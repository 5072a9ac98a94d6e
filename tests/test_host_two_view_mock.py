"""hip_bridge::KltInitT::computeTwoViews / computeTwoView (include/svo_dropin/klt_init_hip.h), the bridge of the bootstrap's two-view
stage, and the C++ twin's second half of addSecondFrame (svo::initialization::KltInit in android_svo_amd/host/svo_host.h: pose,
Points and Features in both frames in the reference's order, the map's flatten) on the CPU against a mock of the svo_hip_klt_*
entry points (tests/host_mock/klt_two_view_mock_test.cpp): call sequences, the status gate and the list contents.  A
stand-alone host program, built plain and with the address / undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_compute_two_views_against_a_mock_device(tmp_path, flags):
    exe = tmp_path / "klt_two_view_mock_test"
    src = os.path.join(ROOT, "tests", "host_mock", "klt_two_view_mock_test.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, "-I" + os.path.join(ROOT, "include"), src, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "klt two view mock test OK" in r.stdout
