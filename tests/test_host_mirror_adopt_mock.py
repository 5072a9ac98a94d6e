"""hip_bridge::DeviceSeedMirror::adopt and the device-grid mode of update() (include/svo_dropin/depth_filter_batch.h) on the CPU
against a mock of the svo_hip_seed_batch_* entry points: a batch born on the device is never uploaded, its events reach the
right list entries, age-out / foreign erasures / recycled list nodes / syncToHost work on it as on an uploaded batch; a
keyframe's pass in the device-grid mode runs with report_updated = 0 and is followed by one svo_hip_seed_batch_mark_updated
call.  Compiled with the reference's language level (-std=c++11), and once more as the same stand-alone program with the
address and undefined-behaviour sanitizers.  The GPU run of the same template is tests/test_gpu_keyframe_seeds.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_mock", "mirror_adopt_mock_test.cpp")


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_adopted_batches_and_the_device_grid_mode_against_a_mock_device(tmp_path, flags):
    exe = tmp_path / "mirror_adopt_mock_test"
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror"] + flags + ["-I" + os.path.join(ROOT, "include"), SRC, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mirror adopt mock test OK" in r.stdout
