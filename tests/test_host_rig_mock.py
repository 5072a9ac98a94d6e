"""The camera-rig paths of the bridges on the CPU against a mock device (tests/host_mock_rig/rig_mock_test.cpp, on the mock seed
batches of tests/host_mock/mirror_mock_test.cpp): hip_bridge::updateCameraRig over three cameras with distinct models makes ONE
svo_hip_seed_batch_update_rig_async call per pass and every camera's model travels with its pass; hip_bridge::FrameTrackerGroupT
creates its group with svo_hip_tracker_group_create_rig, member c given cams[c]; equal cameras still take the calls they always
took.  Built plain, -std=c++11 as the reference."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rig_bridges_against_a_mock_device(tmp_path):
    exe = tmp_path / "rig_mock_test"
    src = os.path.join(ROOT, "tests", "host_mock_rig", "rig_mock_test.cpp")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), src, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rig mock test OK" in r.stdout
