"""The split hip_bridge::DeviceSeedMirror (include/svo_dropin/depth_filter_batch.h) on the CPU against the mock device of
tests/host_mock/mirror_mock_test.cpp, reused by inclusion: update() -- now the composition of three phases -- makes the device
calls it made before the split, in the same order; updateCameras() over several mirrors makes exactly ONE device call and
collects in camera order, every camera ending as its twin does through update().  Built plain, -std=c++11 as the reference."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_split_mirror_and_the_one_call_for_several_mirrors_against_a_mock_device(tmp_path):
    exe = tmp_path / "mirror_cameras_mock_test"
    src = os.path.join(ROOT, "tests", "host_mock_cameras", "mirror_cameras_mock_test.cpp")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), src, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mirror mock test OK" in r.stdout and "mirror cameras mock test OK" in r.stdout
