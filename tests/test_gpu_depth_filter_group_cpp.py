"""svo::DepthFilterGroup (android_svo_amd/host/svo_host.h) on the GPU through svo_host_demo's `filtergroup` mode: three cameras,
each with its own scene, six frames and two keyframes at frames of its own; the group runs every step's updateSeeds of all
cameras as ONE device pass (hip_bridge::updateCameras -> svo_hip_seed_batch_update_cameras_async) over one shared keyframe
cache and one shared current-frame cache.  Per camera the sequence of convergence callbacks (feature, point position bitwise,
sigma2), the final seed list with its device state and the detector grid equal those of a lone unthreaded DepthFilter fed the
same frames."""
import os
import subprocess

import numpy as np
import pytest

from android_svo_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "android_svo_amd", "host", "svo_host_demo")
W, H, LEVELS, N_FRAMES, N_CAMS = 320, 240, 5, 6, 3
KEYFRAMES = ((0, 1), (0, 2), (0, 3))            # per camera: two keyframes, the second at a frame of its own
N_SEEDS = ((150, 90), (257, 40), (64, 300))     # per camera and keyframe
SIGMA2_THRESH = 60.0                            # Options::seed_convergence_sigma2_thresh: seeds converge from the third update on


def _write(path, arr, dtype):
    np.ascontiguousarray(arr, dtype=dtype).tofile(path)


def _write_case(case):
    cam = synth.Camera.default(W, H)
    _write(case / "manifest.bin", [W, H, cam.fx, cam.fy, cam.cx, cam.cy, LEVELS, N_FRAMES, N_CAMS], np.float64)
    _write(case / "depth_mean_min.bin", [2.2, 1.0], np.float64)
    _write(case / "options.bin", [3, SIGMA2_THRESH], np.float64)
    for c in range(N_CAMS):
        cd = case / ("cam%d" % c)
        cd.mkdir()
        rng = np.random.default_rng(600 + c)
        scene = synth.PlaneScene(seed=600 + c, depth=2.0, tilt=(rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)))
        T = synth.se3_from_twist(rng.uniform(-0.05, 0.05, 3), rng.uniform(-0.02, 0.02, 3))
        step = rng.normal(size=3) * [1.0, 1.0, 0.25]
        step /= np.linalg.norm(step)
        for k in range(N_FRAMES):
            if k:
                T = synth.se3_mul(synth.se3_from_twist(step * rng.uniform(0.025, 0.06), rng.uniform(-0.004, 0.004, 3)), T)
            for l, im in enumerate(synth.build_pyramid(scene.render(cam, T))[:LEVELS]):
                _write(cd / ("frame_%d_L%d.bin" % (k, l)), im, np.uint8)
            _write(cd / ("frame_%d_pose.bin" % k), T, np.float64)
        _write(cd / "keyframes.bin", KEYFRAMES[c], np.float64)
        for j, n in enumerate(N_SEEDS[c]):
            px = np.stack([rng.integers(24, W - 24, n), rng.integers(24, H - 24, n)], axis=1).astype(np.float64)
            level = rng.choice(np.asarray((0, 0, 0, 1, 2), dtype=np.int32), size=n)
            px = px - (px % (1 << level)[:, None])
            _write(cd / ("kf%d_px.bin" % j), px, np.float64)
            _write(cd / ("kf%d_f.bin" % j), synth.cam2world(cam, px), np.float64)
            _write(cd / ("kf%d_level.bin" % j), level, np.int32)


def test_depth_filter_group_equals_three_lone_depth_filters(tmp_path):
    assert os.path.exists(DEMO), "build() must have produced android_svo_amd/host/svo_host_demo"
    case, out = tmp_path / "case", tmp_path / "out"
    case.mkdir(); out.mkdir()
    _write_case(case)
    p = subprocess.run([DEMO, str(case), str(out), "filtergroup"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "filtergroup OK" in p.stdout, p.stdout + p.stderr
    n_passes, n_batches, kf_uploads = np.fromfile(out / "group_summary.bin", np.float64)
    assert n_passes == N_FRAMES
    assert n_batches >= N_CAMS * (N_FRAMES - 1)                # every camera had a batch in the pass from its second frame on
    assert kf_uploads == 2 * N_CAMS                            # the shared keyframe cache: every keyframe uploaded once, none evicted
    seen_frames = set()
    for c in range(N_CAMS):
        lone = {k: (out / ("lone_cam%d_%s.bin" % (c, k))).read_bytes() for k in ("conv", "seeds", "grid")}
        group = {k: (out / ("group_cam%d_%s.bin" % (c, k))).read_bytes() for k in ("conv", "seeds", "grid")}
        conv = np.frombuffer(lone["conv"], np.float64).reshape(-1, 5)
        seeds = np.frombuffer(lone["seeds"], np.float64).reshape(-1, 5)
        grid = np.frombuffer(lone["grid"], np.uint8)
        # the scenario does something: seeds converge, the second keyframe's stay with a device state of their own, the
        # keyframe frame marked the grid
        assert len(conv) >= 20 and (conv[:, 0] < N_SEEDS[c][0]).any(), (c, len(conv))
        second = seeds[seeds[:, 0] >= N_SEEDS[c][0]]
        assert len(second) >= 5 and ((second[:, 1] != 10.0) | (second[:, 2] != 10.0)).any()     # a, b moved: the second keyframe's seeds were updated
        assert len(conv) + len(seeds) <= sum(N_SEEDS[c])
        assert grid.any()
        for k in ("conv", "seeds", "grid"):
            assert group[k] == lone[k], (c, k)
        seen_frames.add(lone["conv"])
    assert len(seen_frames) == N_CAMS                          # the cameras' outcomes differ from each other
