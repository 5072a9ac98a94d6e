"""svo_hip_tracker_group_create_rig: a tracker group whose cameras each have their OWN camera model (tests/rig_case.py: A, B and
the distorted C, one image size).  What is checked: every camera's outcome is, bit for bit and frame after frame, what a lone
svo_hip_tracker created with that camera's model gives on the same inputs -- poses, the frame's features, match and trial
counts, overlap lists, the map's point counters -- in the default mode (feature counts in one SparseImgAlign shape class) and
with SVO_HIP_SIA_REDUCTION_TILE_ORDER on maps of 150 / 420 / 600 points; in another camera order; after a promotion and a
relocalisation through the cameras' own handles, finished by svo_hip_tracker_group_finish_frames; that three equal cameras
through the rig call are the group svo_hip_tracker_group_create makes; and what the call refuses.  That a wrong camera model
would show in these bytes is established on the oracle (tests/test_rig_inputs_cpu.py)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import rig_case as rc
import tracking_chain as tc
from android_svo_amd import hip

pytestmark = pytest.mark.gpu

CFG = dict(max_keyframes=4, max_points=1024, max_obs=4096, max_kf_features=2048, max_candidates=16, max_items=1024,
           max_frame_features=1024, grid_size=tc.CELL, max_fts=tc.MAX_FTS, klt_min_level=2)                  # tests/test_gpu_tracker_group.py
KEYS = ("T_f_w", "T_f_w_sia", "feat_px", "feat_f", "feat_level", "feat_point", "feat_type", "feat_grad", "type", "n_failed", "n_succeeded")
FRAMES = list(range(1, 9))
TILE = (hip.SIA_OPT_REDUCTION, hip.SIA_REDUCTION_TILE_ORDER)


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


def _start(trk, seq, mp):
    n = len(seq["px0"])
    trk.upload_keyframe(0, seq["pyrs"][0][0])
    trk.set_map(mp)
    trk.set_last_frame(seq["T0"], seq["px0"], seq["f0"], np.arange(n, dtype=np.int32), kf_slot=0)


def _same(a, b, what):
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)
    assert a["n_matches"] == b["n_matches"] and a["n_trials"] == b["n_trials"] and a["map_changed"] == b["map_changed"], what
    assert list(a["overlap_kf"]) == list(b["overlap_kf"]) and list(a["overlap_count"]) == list(b["overlap_count"]), what


def _img(seq, k):
    return seq["pyrs"][k][0]


def _lone_runs(ctx, seqs, tile_order):
    """every sequence through a lone tracker with the sequence's camera: [camera][frame] results"""
    out = []
    for seq in seqs:
        trk = hip.Tracker(ctx, seq["cam"], **CFG)
        if tile_order:
            trk.set_sia_option(*TILE)
        _start(trk, seq, tc.sequence_map(seq))
        out.append([trk.track(_img(seq, k)) for k in FRAMES])
        trk.destroy()
    return out


def _group_runs(ctx, seqs, cam_or_cams, tile_order):
    grp = hip.TrackerGroup(ctx, cam_or_cams, len(seqs), **CFG)
    if tile_order:
        grp.set_sia_option(*TILE)
    for t, seq in zip(grp.cameras, seqs):
        _start(t, seq, tc.sequence_map(seq))
    out = [[] for _ in seqs]
    for k in FRAMES:
        res = grp.track([_img(seq, k) for seq in seqs])
        for c, t in enumerate(grp.cameras):
            out[c].append(t.last_result())
            assert list(res[c].T_f_w) == list(out[c][-1]["T_f_w"])
    grp.destroy()
    return out


# n_map per camera: one SparseImgAlign shape class in the default mode (as tests/test_gpu_tracker_group.py: 600 beside 530), any
# sizes with the tile-order sums
MAPS = {False: {"A": 600, "B": 530, "C": 600}, True: {"A": 150, "B": 420, "C": 600}}


@pytest.fixture(scope="module")
def lone(ctx):
    cache = {}

    def get(tile_order):
        if tile_order not in cache:
            seqs = {n: rc.sequence(n, n_map=MAPS[tile_order][n]) for n in rc.NAMES}
            cache[tile_order] = (seqs, dict(zip(rc.NAMES, _lone_runs(ctx, [seqs[n] for n in rc.NAMES], tile_order))))
        return cache[tile_order]
    return get


@pytest.mark.parametrize("order", ["ABC", "CAB"])
@pytest.mark.parametrize("tile_order", [False, True])
def test_rig_cameras_track_as_lone_trackers_with_their_models(ctx, lone, tile_order, order):
    seqs, want = lone(tile_order)
    got = _group_runs(ctx, [seqs[n] for n in order], [seqs[n]["cam"] for n in order], tile_order)
    for c, n in enumerate(order):
        for step in range(len(FRAMES)):
            _same(got[c][step], want[n][step], (order, n, step))
        assert got[c][-1]["n_matches"] >= 50
    assert len({want[n][-1]["T_f_w"].tobytes() for n in rc.NAMES}) == 3                 # (the cameras really did different things)


def test_three_equal_cameras_are_the_group_of_one_model(ctx):
    """svo_hip_tracker_group_create is the rig call with its camera repeated"""
    seq_a = rc.sequence("A", n_map=600)
    seqs = [seq_a, rc.sequence("A", n_map=530), seq_a]
    want = _group_runs(ctx, seqs, seq_a["cam"], False)
    got = _group_runs(ctx, seqs, [seq_a["cam"]] * 3, False)
    for c in range(3):
        for step in range(len(FRAMES)):
            _same(got[c][step], want[c][step], (c, step))


def _grid_of(ctx, trk):
    g = hip.DetectorGrid(ctx, rc.TRACK_WIDTH, rc.TRACK_HEIGHT, tc.CELL)
    trk.mark_last_frame(g)
    out = g.download()
    g.free()
    return out


def _selection(r, n=20):
    return [int(p) for p in r["feat_point"] if p >= 0][:n]


def _eventful(ctx, trackers, track):
    """three frames; camera 0 promotes its last frame, camera 1 relocalises against its closest keyframe (Map::getClosestKeyframe
    projects the keyframes' key points with the camera's model), two more frames; then the grids the last frames mark and the
    maps.  track(k) -> every camera's result of frame k.  Returns (results [camera][frame], closest keyframe, features of the
    relocalised last frame, grids, maps)."""
    out = [[] for _ in trackers]
    for k in (1, 2, 3):
        for c, r in enumerate(track(k)):
            out[c].append(r)
    assert trackers[0].promote_last_frame(1) == (1, 0)
    near = trackers[1].closest_keyframe(None)
    assert near["kf_index"] == 0
    n_feat = trackers[1].last_frame_from_keyframe(near["kf_index"])
    for k in (4, 5):
        for c, r in enumerate(track(k)):
            out[c].append(r)
    return out, near, n_feat, [_grid_of(ctx, t) for t in trackers], [t.download_map() for t in trackers]


def _same_bytes(a, b, what):
    assert sorted(a) == sorted(b), what
    for key in a:
        assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), (what, key)


def test_promotion_relocalisation_and_finish_frames_use_each_cameras_model(ctx):
    seqs = [rc.sequence(n, n_map=MAPS[True][n]) for n in rc.NAMES]
    # ---- lone trackers with the cameras' models
    lone_trks = [hip.Tracker(ctx, seq["cam"], **CFG) for seq in seqs]
    for trk, seq in zip(lone_trks, seqs):
        trk.set_sia_option(*TILE)
        _start(trk, seq, tc.sequence_map(seq))
    want, want_near, want_n, want_grids, want_maps = _eventful(ctx, lone_trks, lambda k: [t.track(_img(s, k)) for t, s in zip(lone_trks, seqs)])
    want_fin = [t.finish_frame(_selection(want[c][-1]), n_iter=5, kf_select_min_dist=0.12) for c, t in enumerate(lone_trks)]
    for trk in lone_trks:
        trk.destroy()
    # ---- the rig
    grp = hip.TrackerGroup(ctx, [s["cam"] for s in seqs], 3, **CFG)
    grp.set_sia_option(*TILE)
    for t, seq in zip(grp.cameras, seqs):
        _start(t, seq, tc.sequence_map(seq))

    def track(k):
        grp.track([_img(seq, k) for seq in seqs])
        return [t.last_result() for t in grp.cameras]
    got, near, n_feat, grids, maps = _eventful(ctx, grp.cameras, track)
    fin = grp.finish_frames([(_selection(got[c][-1]), 5) for c in range(3)], kf_select_min_dist=0.12)
    grp.destroy()
    assert near == want_near and n_feat == want_n
    for c in range(3):
        for i, (a, b) in enumerate(zip(got[c], want[c])):
            _same(a, b, (c, i))
        assert grids[c].any() and grids[c].tobytes() == want_grids[c].tobytes(), c          # svo_hip_tracker_mark_last_frame
        _same_bytes(maps[c], want_maps[c], ("map", c))
        assert fin[c][0].tobytes() == want_fin[c][0].tobytes() and fin[c][1].tobytes() == want_fin[c][1].tobytes(), c
        _same_bytes(fin[c][2], want_fin[c][2], ("decision", c))
    assert any(1 in list(r["overlap_kf"]) for r in got[0][3:])                            # camera 0's new keyframe took part


@pytest.mark.parametrize("case", ["width", "height", "null_cams", "no_cameras", "a_camera_the_lone_tracker_refuses"])
def test_refusals_create_nothing(ctx, case):
    cams = [rc.camera(n, rc.TRACK_WIDTH, rc.TRACK_HEIGHT) for n in rc.NAMES]
    n = 3
    if case == "width":
        cams[2] = rc.camera("C", rc.TRACK_WIDTH + 16, rc.TRACK_HEIGHT)
    elif case == "height":
        cams[1] = dataclasses.replace(cams[1], height=rc.TRACK_HEIGHT - 2)
    elif case == "no_cameras":
        n = 0
    elif case == "a_camera_the_lone_tracker_refuses":                             # trk_check_config: at least 17 x 17, checked for every camera
        cams = [dataclasses.replace(cams[0], width=16), dataclasses.replace(cams[1], width=16)]
        n = 2
    cfg = hip.CTrackerConfig()
    ctx.check(ctx.lib.svo_hip_tracker_default_config(C.byref(cfg)), "tracker_default_config")
    for k, v in CFG.items():
        setattr(cfg, k, v)
    ccams = (hip.CCamera * len(cams))(*[hip.make_camera(m) for m in cams])
    before = ctx.info()
    h = C.c_void_p(0x1234)
    rcode = ctx.lib.svo_hip_tracker_group_create_rig(ctx.h, None if case == "null_cams" else ccams, C.byref(cfg), n, C.byref(h))
    assert rcode == -1                                                           # SVO_HIP_ERR_INVALID
    assert not h.value                                                           # no group
    after = ctx.info()
    assert (after["allocator_calls"], after["free_calls"]) == (before["allocator_calls"], before["free_calls"]), (before, after)
    if case in ("width", "height"):
        with pytest.raises(hip.SvoHipError, match=r"\(-1\)"):
            hip.TrackerGroup(ctx, cams, 3, **CFG)
