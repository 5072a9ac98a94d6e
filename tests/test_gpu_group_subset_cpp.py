"""svo_host_demo `trackgroup 3 staggered`: three worlds on svo::FrameTrackerGroup whose cameras do not advance together -- world w
takes part in every (w + 1)-th call of the group, through hip_bridge::FrameTrackerGroupT::trackSome
(svo_hip_tracker_group_track_some), and sits the others out -- against the same schedule replayed through
TrackerGroup.track_some: every world's poses, features and match counts, frame by frame and bit for bit (both sides hand the
C-ABI the same tables and the same lists, so the SparseImgAlign kernel takes the same shape in every call)."""
import os
import subprocess

import numpy as np
import pytest

import tracking_chain as tc
from test_gpu_host_cpp import DEMO, _write_track_case
from android_svo_amd import hip

pytestmark = pytest.mark.gpu

N_WORLDS, N_FRAMES = 3, 7


def test_cpp_staggered_group_equals_the_python_replay(tmp_path):
    assert os.path.exists(DEMO), "build() must have produced android_svo_amd/host/svo_host_demo"
    case, out = tmp_path / "case", tmp_path / "out"
    case.mkdir(); out.mkdir()
    seq = tc.make_sequence(n_frames=N_FRAMES)
    mp = tc.sequence_map(seq)
    n = len(seq["px0"])
    cs = dict(mp, obs_point=np.arange(n, dtype=np.int32), kf_ftr_obs=np.arange(n, dtype=np.int32), cand_obs=np.zeros(0, np.int32))
    cfg = dict(grid_size=tc.CELL, max_fts=tc.MAX_FTS, quality_min_fts=40, klt_min_level=2, max_frame_features=1024)
    frames = [seq["pyrs"][k][0] for k in range(1, N_FRAMES)]
    _write_track_case(case, cs, frames, cfg, last_kf=0)
    p = subprocess.run([DEMO, str(case), str(out), "trackgroup", str(N_WORLDS), "staggered"], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert p.returncode == 0 and "trackgroup OK (3 worlds, staggered)" in p.stdout, p.stdout + p.stderr
    # the calls the demo made: world w in every (w + 1)-th one until its frames ran out
    sched = np.fromfile(out / "group_schedule.bin", np.float64).reshape(-1, 1 + N_WORLDS)
    done, want_sched, t = [0] * N_WORLDS, [], 0
    while min(done) < len(frames):
        act = [w for w in range(N_WORLDS) if done[w] < len(frames) and t % (w + 1) == 0]
        if act:
            want_sched.append([t] + [1.0 if w in act else 0.0 for w in range(N_WORLDS)])
            for w in act:
                done[w] += 1
        t += 1
    np.testing.assert_array_equal(sched, np.array(want_sched))
    assert {sum(row[1:]) for row in want_sched} == {1.0, 2.0, 3.0} and want_sched[0][1:] == [1.0] * N_WORLDS      # one, two and all three in a call
    # the same schedule through the Python mirror
    ctx = hip.Context(0)
    grp = hip.TrackerGroup(ctx, seq["cam"], N_WORLDS, max_keyframes=3, grid_size=tc.CELL, max_fts=tc.MAX_FTS, klt_min_level=2, max_frame_features=1024)
    for trk in grp.cameras:
        trk.upload_keyframe(0, seq["pyrs"][0][0])
        trk.set_map(mp)
        trk.set_last_frame(seq["T0"], seq["px0"], seq["f0"], np.arange(n, dtype=np.int32), kf_slot=0)
    rd = lambda w, name, dt: np.fromfile(out / ("g%d" % w) / name, dtype=dt)
    poses = [rd(w, "track_poses.bin", np.float64).reshape(-1, 7) for w in range(N_WORLDS)]
    stats = [rd(w, "track_stats.bin", np.float64).reshape(-1, 9) for w in range(N_WORLDS)]
    assert all(len(ps) == len(frames) for ps in poses)
    done = [0] * N_WORLDS
    for row in want_sched:
        act = [w for w in range(N_WORLDS) if row[1 + w]]
        grp.track_some(act, [frames[done[w]] for w in act])
        for w in act:
            k, r = done[w], grp.cameras[w].last_result()
            np.testing.assert_array_equal(poses[w][k], r["T_f_w"], err_msg="world %d frame %d" % (w, k))
            assert stats[w][k, 0] == len(r["feat_px"]) and stats[w][k, 1] == r["n_matches"] >= 50 and stats[w][k, 2] == r["n_trials"]
            assert stats[w][k, 3] == int(r["result"].sia_n_tracked) and stats[w][k, 5] == int(r["result"].pose.num_obs)
            np.testing.assert_array_equal(rd(w, "track_feat_%d_px.bin" % k, np.float64).reshape(-1, 2), r["feat_px"])
            np.testing.assert_array_equal(rd(w, "track_feat_%d_point.bin" % k, np.int32), r["feat_point"])
            np.testing.assert_array_equal(rd(w, "track_feat_%d_level.bin" % k, np.int32), r["feat_level"])
            done[w] += 1
    assert done == [len(frames)] * N_WORLDS
    grp.destroy(); ctx.close()
