"""The C++ host twins over a camera rig (tests/rig_case.py: cameras A, B and the distorted C, one image size), through
svo_host_demo:

  trackgroup 3 rig   svo::FrameTrackerGroup created with a model per camera (hip_bridge::FrameTrackerGroupT ->
                     svo_hip_tracker_group_create_rig), every camera on a sequence of its own: every file a world writes --
                     poses, features, counters, the map after the run -- equals, byte for byte, what a lone svo::FrameTracker
                     with that camera wrote for the same case;
  filtergroup rig    svo::DepthFilterGroup (hip_bridge::updateCameraRig -> svo_hip_seed_batch_update_rig_async): per camera the
                     sequence of convergence callbacks, the final seed list and the detector grid equal those of a lone
                     DepthFilter whose frames carry the same camera."""
import os
import subprocess

import numpy as np
import pytest

import rig_case as rc
import tracking_chain as tc
from android_svo_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "android_svo_amd", "host", "svo_host_demo")
ENV = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")


def _write(path, arr, dtype):
    np.ascontiguousarray(arr, dtype=dtype).tofile(path)


def _dist(cam):
    return list(getattr(cam, "dist", None) or [0.0] * 5)


# ---- the trackers
N_TRACK_FRAMES = 9


def _write_track_case(case, seq):
    """the case files of svo_host_demo's `track` mode (tests/test_gpu_host_cpp.py) for a rig camera's sequence: one keyframe whose
    features hold the map points, frame 5 becomes a keyframe"""
    mp = tc.sequence_map(seq)
    cam, n = seq["cam"], len(seq["px0"])
    cs = dict(mp, obs_point=np.arange(n, dtype=np.int32), kf_ftr_obs=np.arange(n, dtype=np.int32), cand_obs=np.zeros(0, np.int32))
    frames = [seq["pyrs"][k][0] for k in range(1, N_TRACK_FRAMES)]
    _write(case / "track_manifest.bin",
           [cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy, 1, n, n, n, 0, len(frames), tc.CELL, tc.MAX_FTS, 40, 2, 1024, 0, 0, 5, -1], np.float64)
    _write(case / "track_dist.bin", _dist(cam), np.float64)
    _write(case / "kf_0_img.bin", seq["pyrs"][0][0], np.uint8)
    _write(case / "kf_pose.bin", cs["T_kf_w"], np.float64)
    for name, dt in (("pt_pos", np.float64), ("pt_type", np.int32), ("pt_n_failed", np.int32), ("pt_n_succeeded", np.int32), ("pt_obs_offset", np.int32),
                     ("obs_point", np.int32), ("obs_kf", np.int32), ("obs_px", np.float64), ("obs_f", np.float64), ("obs_level", np.int32),
                     ("obs_edgelet", np.uint8), ("obs_grad", np.float64), ("kf_ftr_offset", np.int32), ("kf_ftr_obs", np.int32), ("cand_obs", np.int32)):
        _write(case / (name + ".bin"), cs[name], dt)
    for k, img in enumerate(frames):
        _write(case / ("trk_frame_%d.bin" % k), img, np.uint8)


def test_cpp_tracker_rig_equals_three_lone_trackers(tmp_path):
    assert os.path.exists(DEMO), "build() must have produced android_svo_amd/host/svo_host_demo"
    case, outg = tmp_path / "case", tmp_path / "outg"
    case.mkdir(); outg.mkdir()
    for w, name in enumerate(rc.NAMES):
        (case / ("cam%d" % w)).mkdir()
        _write_track_case(case / ("cam%d" % w), rc.sequence(name, n_frames=N_TRACK_FRAMES, n_map=600))
    p = subprocess.run([DEMO, str(case), str(outg), "trackgroup", "3", "rig"], capture_output=True, text=True, timeout=300, env=ENV)
    assert p.returncode == 0 and "trackgroup OK (3 worlds, a rig)" in p.stdout, p.stdout + p.stderr
    poses = []
    for w in range(3):
        out = tmp_path / ("out%d" % w)
        out.mkdir()
        p = subprocess.run([DEMO, str(case / ("cam%d" % w)), str(out), "track"], capture_output=True, text=True, timeout=300, env=ENV)
        assert p.returncode == 0, p.stdout + p.stderr
        names = sorted(f for f in os.listdir(out) if f.startswith("track_") and f.endswith(".bin"))
        assert len(names) > 10
        for f in names:
            if f != "track_uploads.bin":
                assert (out / f).read_bytes() == (outg / ("g%d" % w) / f).read_bytes(), (w, f)
        poses.append(np.fromfile(out / "track_poses.bin", np.float64).reshape(-1, 7))
        stats = np.fromfile(out / "track_stats.bin", np.float64).reshape(-1, 9)
        assert len(poses[-1]) == N_TRACK_FRAMES - 1 and (stats[:, 1] >= 50).all(), (w, stats[:, 1])        # every frame tracked
        err = np.array([synth.pose_error(a, t) for a, t in zip(poses[-1], rc.sequence(rc.NAMES[w], n_frames=N_TRACK_FRAMES, n_map=600)["truth"][1:])])
        assert err[:, 0].max() < 2e-3 and err[:, 1].max() < 5e-3, (w, err.max(axis=0))                     # ... with the right camera
    assert len({p.tobytes() for p in poses}) == 3


# ---- the depth filters
W, H, LEVELS, N_FRAMES = rc.WIDTH, rc.HEIGHT, rc.LEVELS, 6
KEYFRAMES = ((0, 1), (0, 2), (0, 3))            # per camera: two keyframes, the second at a frame of its own
N_SEEDS = ((150, 90), (257, 40), (64, 300))     # per camera and keyframe
SIGMA2_THRESH = 60.0                            # Options::seed_convergence_sigma2_thresh: seeds converge from the third update on


def _write_filter_case(case):
    """the case files of `filtergroup` (tests/test_gpu_depth_filter_group_cpp.py), every camera rendering and observing with its
    own model (cam<c>/camera.bin)"""
    a = rc.camera("A", W, H)
    _write(case / "manifest.bin", [W, H, a.fx, a.fy, a.cx, a.cy, LEVELS, N_FRAMES, 3], np.float64)
    _write(case / "depth_mean_min.bin", [2.2, 1.0], np.float64)
    _write(case / "options.bin", [3, SIGMA2_THRESH], np.float64)
    for c, name in enumerate(rc.NAMES):
        cam = rc.camera(name, W, H)
        cd = case / ("cam%d" % c)
        cd.mkdir()
        _write(cd / "camera.bin", [cam.fx, cam.fy, cam.cx, cam.cy] + _dist(cam), np.float64)
        rng = np.random.default_rng(700 + c)
        scene = synth.PlaneScene(seed=700 + c, depth=2.0, tilt=(rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)))
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
            _write(cd / ("kf%d_f.bin" % j), rc.bearings(cam, px), np.float64)
            _write(cd / ("kf%d_level.bin" % j), level, np.int32)


def test_cpp_depth_filter_rig_equals_three_lone_depth_filters(tmp_path):
    assert os.path.exists(DEMO), "build() must have produced android_svo_amd/host/svo_host_demo"
    case, out = tmp_path / "case", tmp_path / "out"
    case.mkdir(); out.mkdir()
    _write_filter_case(case)
    p = subprocess.run([DEMO, str(case), str(out), "filtergroup", "rig"], capture_output=True, text=True, timeout=300, env=ENV)
    assert p.returncode == 0 and "filtergroup OK (a rig)" in p.stdout, p.stdout + p.stderr
    n_passes, n_batches, kf_uploads = np.fromfile(out / "group_summary.bin", np.float64)
    assert n_passes == N_FRAMES and n_batches >= 3 * (N_FRAMES - 1) and kf_uploads == 6
    seen = set()
    for c in range(3):
        lone = {k: (out / ("lone_cam%d_%s.bin" % (c, k))).read_bytes() for k in ("conv", "seeds", "grid")}
        group = {k: (out / ("group_cam%d_%s.bin" % (c, k))).read_bytes() for k in ("conv", "seeds", "grid")}
        conv = np.frombuffer(lone["conv"], np.float64).reshape(-1, 5)
        # the scenario does something with every camera's model: seeds converge, the keyframe frame marked the grid
        assert len(conv) >= 20 and np.frombuffer(lone["grid"], np.uint8).any(), (c, len(conv))
        for k in ("conv", "seeds", "grid"):
            assert group[k] == lone[k], (c, k)
        seen.add(lone["conv"])
    assert len(seen) == 3
