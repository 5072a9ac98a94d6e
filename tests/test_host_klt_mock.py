"""hip_bridge::KltInitT (include/svo_dropin/klt_init_hip.h), the bootstrap's bridge, on the CPU against a mock of the
svo_hip_klt_* entry points (tests/host_mock/klt_init_mock_test.cpp): call sequences, FAILURE / NO_KEYFRAME / SUCCESS at the
gates' boundaries, the lists after erasures over several frames, refused calls.  A stand-alone host program, built plain and
with the address / undefined-behaviour sanitizers, at the reference's language level.  The GPU run of the same template is
tests/test_gpu_klt_cpp.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_klt_init_against_a_mock_device(tmp_path, flags):
    exe = tmp_path / "klt_init_mock_test"
    src = os.path.join(ROOT, "tests", "host_mock", "klt_init_mock_test.cpp")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", *flags, "-I" + os.path.join(ROOT, "include"), src, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "klt init mock test OK" in r.stdout
