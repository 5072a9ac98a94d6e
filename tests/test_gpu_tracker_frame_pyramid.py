"""svo_hip_tracker_last_frame_pyramid: the pyramid batch that holds the last frames of a tracker's group, borrowed, so that a
depth pass of the group's cameras (svo_hip_seed_batch_update_cameras_async) reads the frames the group has just tracked and
the group's keyframe batch -- no image upload, no pyramid build of its own.  A group of three cameras over the map-growth
scenario's frames, every camera a few frames ahead of the previous one."""
import functools

import numpy as np
import pytest

import map_growth_scenario as sc
import tracking_chain as tc
from android_svo_amd import hip, seedsynth, synth

pytestmark = pytest.mark.gpu

CFG = dict(max_keyframes=4, grid_size=tc.CELL, max_fts=tc.MAX_FTS, klt_min_level=2, max_frame_features=1024, max_items=1024)
N_CAMS, N_SEEDS = 3, 200
_scenario = functools.lru_cache(maxsize=None)(sc.make)


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


def _start(trk, seq):
    trk.upload_keyframe(0, seq["pyrs"][0][0])
    trk.set_map(tc.sequence_map(seq))
    trk.set_last_frame(seq["T0"], seq["px0"], seq["f0"], np.arange(len(seq["px0"]), dtype=np.int32), kf_slot=0)


def _seeds(cam, c):
    """seeds of camera c on keyframe 0: corners on integer pixels of their level, the Seed constructor's state"""
    rng = np.random.default_rng(900 + c)
    px = np.stack([rng.integers(40, cam.width - 40, N_SEEDS), rng.integers(40, cam.height - 40, N_SEEDS)], axis=1).astype(np.float64)
    level = rng.choice(np.asarray((0, 0, 0, 1, 2), dtype=np.int32), size=N_SEEDS)
    px = px - (px % (1 << level)[:, None])
    a, b, mu, zr, s2 = seedsynth.seed_ctor(2.4, 1.1, N_SEEDS)
    return px, synth.cam2world(cam, px), level.astype(np.int32), a, b, mu, zr, (s2 * np.float32(0.02)).astype(np.float32)


def test_no_last_frame_is_a_state_error_and_a_lone_trackers_slot_is_0(ctx):
    seq = _scenario()["seq"]
    trk = hip.Tracker(ctx, seq["cam"], **CFG)
    with pytest.raises(hip.SvoHipError, match=r"\(-4\)"):                        # SVO_HIP_ERR_STATE
        trk.last_frame_pyramid()
    _start(trk, seq)
    trk.track(seq["pyrs"][1][0])
    pyr, slot = trk.last_frame_pyramid()
    assert slot == 0 and pyr.batch == 1 and (pyr.width, pyr.height) == (seq["cam"].width, seq["cam"].height)
    for l in range(pyr.n_levels):
        assert pyr.download_level(0, l).tobytes() == seq["pyrs"][1][l].tobytes(), l
    pyr.destroy()                                                              # a borrowed view: the tracker keeps its batch
    trk.track(seq["pyrs"][2][0])
    trk.destroy()


def test_group_frames_and_a_depth_pass_over_the_borrowed_batches(ctx):
    seq = _scenario()["seq"]
    cam = seq["cam"]
    grp = hip.TrackerGroup(ctx, cam, N_CAMS, **CFG)
    for t in grp.cameras:
        _start(t, seq)
    K = CFG["max_keyframes"]
    kf_hand = hip.Pyramid(ctx, cam.width, cam.height, 5, N_CAMS * K)
    cf_hand = hip.Pyramid(ctx, cam.width, cam.height, 5, N_CAMS)
    for c in range(N_CAMS):
        kf_hand.upload(c * K, seq["pyrs"][0])
    seeds = [_seeds(cam, c) for c in range(N_CAMS)]
    borrowed_b = [hip.ResidentSeeds(ctx, *s) for s in seeds]
    hand_b = [hip.ResidentSeeds(ctx, *s) for s in seeds]
    n_events = 0
    for k in range(1, 4):
        frames = [k + 2 * c for c in range(N_CAMS)]                              # the cameras see different frames
        grp.track([seq["pyrs"][f][0] for f in frames])
        poses = [np.array(t.last_result()["T_f_w"], dtype=np.float64) for t in grp.cameras]
        views = [t.last_frame_pyramid() for t in grp.cameras]
        assert [s for _, s in views] == list(range(N_CAMS))
        assert len({p.h.value for p, _ in views}) == 1                         # one batch for the group
        cur = views[0][0]
        assert cur.batch == N_CAMS
        for c, f in enumerate(frames):
            for l in range(cur.n_levels):
                assert cur.download_level(c, l).tobytes() == seq["pyrs"][f][l].tobytes(), (k, c, l)
            cf_hand.upload(c, seq["pyrs"][f])
        kf = grp.cameras[0].keyframe_pyramids()
        assert kf.batch == N_CAMS * K
        keyframe = k == 2

        def passes(batches, slots):
            return [([batches[c]], [c * K], seq["T0"][None, :], slots[c], poses[c], keyframe and c != 1) for c in range(N_CAMS)]
        hip.ResidentSeeds.update_cameras_async(passes(borrowed_b, [s for _, s in views]), kf, cur, cam)
        got = [rs.collect() for rs in borrowed_b]
        hip.ResidentSeeds.update_cameras_async(passes(hand_b, list(range(N_CAMS))), kf_hand, cf_hand, cam)
        want = [rs.collect() for rs in hand_b]
        for c in range(N_CAMS):
            assert got[c][0].tobytes() == want[c][0].tobytes() and np.array_equal(got[c][1], want[c][1]), (k, c)
            assert borrowed_b[c].status().tobytes() == hand_b[c].status().tobytes()
            d, e = borrowed_b[c].download(), hand_b[c].download()
            assert all(d[key].tobytes() == e[key].tobytes() for key in d), (k, c)
            n_events += len(got[c][0])
        if k == 1:
            assert int((borrowed_b[0].status() >= hip.SEED_UPDATED).sum()) > N_SEEDS // 2  # the pass does find the seeds in the tracked frame
    assert n_events > N_SEEDS
    for rs in borrowed_b + hand_b:
        rs.destroy()
    kf_hand.destroy(); cf_hand.destroy()
    grp.destroy()
