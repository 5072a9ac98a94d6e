"""svo_hip_tracker_finish_frame / svo_hip_tracker_group_finish_frames: the structure step and the keyframe decision (scene depth,
needNewKf, Map::getFurthestKeyframe) in one device call, against the numpy models of tests/keyframe_decision_reference.py
(tests/test_keyframe_decision_model.py pins those to the C++ twins and their std::nth_element) and against
svo_hip_tracker_optimize_structure on a twin tracker.  Integers are compared exactly, doubles with == (bit equality for every
value but a zero) or byte by byte."""
import ctypes as C
import math

import numpy as np
import pytest

import keyframe_decision_reference as kd
import map_growth_reference as mg
import map_removal_scenario as ms
import tracking_chain as tc
from test_gpu_map_growth import _same, _start
from test_gpu_relocalise import CFG as SEQ_CFG, _img, _lead
from android_svo_amd import hip, synth

pytestmark = pytest.mark.gpu

STATE, INVALID = r"\(-4\)", r"\(-1\)"
MAX_FEAT, MAX_KF = 2816, 256
SMALL = dict(max_keyframes=MAX_KF, max_points=4096, max_obs=64, max_kf_features=64, max_candidates=8, max_items=16, max_frame_features=MAX_FEAT,
             n_levels=1, klt_max_level=0, klt_min_level=0, n_pyr_levels=1, max_fts=16, grid_size=8)
CAM = synth.Camera(32, 32, 30.0, 30.0, 15.5, 15.5)               # the smallest the tracker takes is 17 x 17; no frame is tracked here
COUNTS = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, MAX_FEAT)


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small(ctx):
    trk = hip.Tracker(ctx, CAM, **SMALL)
    yield trk
    trk.destroy()


@pytest.fixture(scope="module")
def seq():
    return tc.make_sequence(n_frames=8, n_map=600)


def _assert_decision(got, want, what):
    for k in ("n_depths", "n_nan_depths", "overlap_valid", "need_new_kf", "blocking_kf", "furthest_kf"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("depth_mean", "depth_min", "furthest_distance"):
        assert got[k] == want[k] or (math.isnan(got[k]) and math.isnan(want[k])), (what, k, got[k], want[k])
    assert np.asarray(got["pos"]).tobytes() == np.asarray(want["pos"], dtype=np.float64).tobytes(), (what, "pos")


def _same_decision(a, b, what):
    _assert_decision(a, b, what)
    for k in ("depth_mean", "depth_min", "furthest_distance"):
        assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), (what, k)


def _set_frame(trk, tables, T, feat):
    trk.set_map(tables)
    n = len(feat)
    trk.set_last_frame(T, np.zeros((n, 2)), np.tile([0.0, 0.0, 1.0], (n, 1)), feat, img=np.zeros((CAM.height, CAM.width), np.uint8))


# ---- the depth part alone
@pytest.mark.parametrize("kind", kd.DEPTH_KINDS)
@pytest.mark.parametrize("n", COUNTS)
def test_scene_depth_against_the_model(small, n, kind):
    tables, T, feat = kd.depth_case(n, kind, max_features=MAX_FEAT)
    assert len(feat) <= MAX_FEAT and int((feat >= 0).sum()) == n and (n in (0, MAX_FEAT) or (feat < 0).any())
    _set_frame(small, tables, T, feat)
    pos, it, got = small.finish_frame([])
    want = kd.decision(tables, T, feat, None, 0.12)
    print(n, kind, got["n_depths"], got["n_nan_depths"], got["depth_mean"], want["depth_mean"], got["depth_min"], want["depth_min"])
    assert len(pos) == 0 and len(it) == 0
    assert want["n_depths"] + want["n_nan_depths"] == n and want["n_nan_depths"] == (1 if kind == "nan" and n else 0)
    _assert_decision(got, want, (n, kind))
    if n == 0:
        assert math.isnan(got["depth_mean"]) and got["depth_min"] == kd.DBL_MAX
    assert got["need_new_kf"] == -1 and got["overlap_valid"] == 0                 # no frame was tracked: no overlap list


# ---- the furthest keyframe
@pytest.mark.parametrize("n_kf", [1, 2, 64, 65, MAX_KF])
def test_furthest_keyframe_against_the_model(small, n_kf):
    tables = kd.line_map(n_kf)
    for T in (np.array([0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]), synth.se3_from_twist([-0.25 * (n_kf - 1) - 0.3, 0.1, 0.0], [0.01, 0.02, -0.01])):
        _set_frame(small, tables, T, np.array([0], np.int32))
        got = small.finish_frame([])[2]
        want = kd.decision(tables, T, [0], None, 0.12)
        _assert_decision(got, want, n_kf)
        assert got["furthest_kf"] in (0, n_kf - 1) and got["furthest_distance"] > 0.0
    assert got["furthest_kf"] == 0 or n_kf == 1                                    # the second frame sits behind the last keyframe


def test_furthest_keyframe_tie_and_none(small):
    tables, T = kd.tie_map()
    _set_frame(small, tables, T, np.array([0], np.int32))
    got = small.finish_frame([])[2]
    _assert_decision(got, kd.decision(tables, T, [0], None, 0.12), "tie")
    assert (got["furthest_kf"], got["furthest_distance"]) == (1, 2.0)              # keyframe 3 is as far: the lower index wins
    tables, T = kd.coincident_map()
    _set_frame(small, tables, T, np.array([0], np.int32))
    got = small.finish_frame([])[2]
    _assert_decision(got, kd.decision(tables, T, [0], None, 0.12), "coincident")
    assert (got["furthest_kf"], got["furthest_distance"]) == (-1, 0.0)


# ---- after a tracked frame
def _selection(r, n=20):
    return [int(p) for p in r["feat_point"] if p >= 0][:n]


def _living_points(tables, feat_point):
    """feat_point with the points that have been deleted since set to -1 (what a removal does to the device's last frame)"""
    fp = np.array(feat_point, dtype=np.int32)
    has = fp >= 0
    fp[has] = np.where(tables["pt_type"][fp[has]] == synth.TYPE_DELETED, -1, fp[has])
    return fp


def _model_after(trk, r, min_dist, valid=True):
    """the model's decision on the device's tables as they are now, for the tracked frame r"""
    tables = trk.download_map()
    return kd.decision(tables, r["T_f_w"], _living_points(tables, r["feat_point"]), list(r["overlap_kf"]) if valid else None, min_dist)


@pytest.fixture(scope="module")
def tracked(ctx, seq):
    """twin trackers after the same lead-up (two keyframes, frame 5 tracked last): X finishes the frame with the new call, Y with
    svo_hip_tracker_optimize_structure; both track frame 6 afterwards"""
    x, rs = _lead(ctx, seq)
    y, rs_y = _lead(ctx, seq)
    r = rs[-1]
    sel = _selection(r)
    before = x.download_map()
    pos_x, it_x, dec = x.finish_frame(sel, n_iter=5, kf_select_min_dist=0.12)
    after = x.download_map()
    pos_y, it_y = y.optimize_structure(sel, n_iter=5)
    out = dict(x=x, y=y, r=r, sel=sel, before=before, after=after, pos_x=pos_x, it_x=it_x, pos_y=pos_y, it_y=it_y, dec=dec)
    yield out
    x.destroy()
    y.destroy()


def test_decision_after_a_tracked_frame(tracked):
    s = tracked
    r, dec = s["r"], s["dec"]
    want = kd.decision(s["after"], r["T_f_w"], r["feat_point"], list(r["overlap_kf"]), 0.12)
    print(dec, len(r["overlap_kf"]))
    _assert_decision(dec, want, "tracked frame")
    # (this also shows that the device's last frame holds exactly the features with feat_point >= 0)
    assert dec["n_depths"] == int((r["feat_point"] >= 0).sum()) >= 50 and dec["overlap_valid"] == 1 and len(r["overlap_kf"]) >= 1
    assert dec["furthest_kf"] >= 0 and 0.5 < dec["depth_mean"] < 10.0 and dec["depth_min"] <= dec["depth_mean"]


def test_positions_equal_optimize_structure_and_the_call_only_reads(tracked, seq):
    s = tracked
    assert len(s["sel"]) == 20 and s["it_x"].min() >= 1
    assert s["pos_x"].tobytes() == s["pos_y"].tobytes() and s["it_x"].tobytes() == s["it_y"].tobytes()
    a, b = mg.normalised(s["before"]), mg.normalised(s["after"])
    for k in mg.TABLES:
        if k != "pt_pos":
            assert a[k].tobytes() == b[k].tobytes(), k
    others = np.ones(len(a["pt_pos"]), bool)
    others[s["sel"]] = False
    assert a["pt_pos"][others].tobytes() == b["pt_pos"][others].tobytes() and b["pt_pos"][s["sel"]].tobytes() == s["pos_x"].tobytes()
    assert a["pt_pos"][s["sel"]].tobytes() != s["pos_x"].tobytes()
    mg.assert_tables_equal(s["after"], s["y"].download_map())
    # n == 0: no structure step, the same decision, nothing written
    pos, it, dec = s["x"].finish_frame([], kf_select_min_dist=0.12)
    assert len(pos) == 0
    _same_decision(dec, s["dec"], "n == 0")
    mg.assert_tables_equal(s["x"].download_map(), s["after"])
    # the result block of the tracked frame is where it was, and the next frame equals the twin's
    assert s["x"].last_result()["feat_point"].tobytes() == s["r"]["feat_point"].tobytes()
    _same(s["x"].track(_img(seq, 6)), s["y"].track(_img(seq, 6)), "the next frame")


def test_the_boundary_of_the_decision(ctx, seq):
    x, rs = _lead(ctx, seq)
    r = rs[-1]
    tables = x.download_map()
    mean = kd.scene_depth(tables, r["T_f_w"], r["feat_point"])[2]
    overlap = list(r["overlap_kf"])
    flips = [float(kd.flip_distance(tables, r["T_f_w"], k, mean)) for k in overlap]
    k_star = overlap[int(np.argmin(flips))]
    lo = hi = min(flips)
    for _ in range(4):                                                             # (the model says where the answer flips: a few ulps
        lo, hi = float(np.nextafter(lo, -np.inf)), float(np.nextafter(hi, np.inf))  # around the real-valued boundary)
        if kd.need_new_kf(tables, r["T_f_w"], overlap, mean, lo)[0] == 1 and kd.need_new_kf(tables, r["T_f_w"], overlap, mean, hi)[0] == 0:
            break
    below, above = x.finish_frame([], kf_select_min_dist=lo)[2], x.finish_frame([], kf_select_min_dist=hi)[2]
    print("flips", flips, "lo", lo.hex(), "hi", hi.hex(), below["need_new_kf"], above["need_new_kf"], above["blocking_kf"])
    _assert_decision(below, kd.decision(tables, r["T_f_w"], r["feat_point"], overlap, lo), "below")
    _assert_decision(above, kd.decision(tables, r["T_f_w"], r["feat_point"], overlap, hi), "above")
    assert (below["need_new_kf"], below["blocking_kf"]) == (1, -1) and (above["need_new_kf"], above["blocking_kf"]) == (0, k_star)
    far = x.finish_frame([], kf_select_min_dist=1e6)[2]                            # everything blocks: the FIRST of the list is named
    assert (far["need_new_kf"], far["blocking_kf"]) == (0, overlap[0])
    x.destroy()


# ---- the state rules
def test_overlap_valid_follows_the_state(ctx, seq):
    cam = seq["cam"]
    x, rs = _lead(ctx, seq)
    r = rs[-1]
    d0 = x.finish_frame([])[2]
    assert d0["overlap_valid"] == 1 and d0["need_new_kf"] in (0, 1)
    # kept, with the same decision: new candidates, renumbered points, optimised positions
    x.add_candidates(pos=[[0.1, 0.2, 2.0]], kf_index=[0], px=[[30.0, 40.0]], f=[[0.0, 0.0, 1.0]], level=[0])
    _same_decision(x.finish_frame([])[2], d0, "add_candidates")
    assert x.compact_points()["n_points"] <= len(r["type"]) + 1
    _same_decision(x.finish_frame([])[2], d0, "compact_points")
    r6 = x.track(_img(seq, 6))
    d6 = x.finish_frame([])[2]
    _assert_decision(d6, _model_after(x, r6, 0.12), "frame 6")
    assert d6["overlap_valid"] == 1
    # cleared: the frame becomes a keyframe; a keyframe leaves (and the furthest one is named in the new numbering)
    assert x.promote_last_frame(2)[0] == 2
    d = x.finish_frame([])[2]
    assert (d["overlap_valid"], d["need_new_kf"], d["blocking_kf"]) == (0, -1, -1) and d["n_depths"] == d6["n_depths"]
    r7 = x.track(_img(seq, 7))
    d7 = x.finish_frame([])[2]
    _assert_decision(d7, _model_after(x, r7, 0.12), "frame 7")
    assert d7["overlap_valid"] == 1 and x.map_sizes()["n_kf"] == 3
    x.remove_keyframe(0)
    d = x.finish_frame([])[2]
    _assert_decision(d, _model_after(x, r7, 0.12, valid=False), "after the removal")
    assert x.map_sizes()["n_kf"] == 2 and d["need_new_kf"] == -1 and 0 <= d["furthest_kf"] < 2
    r7 = x.track(_img(seq, 7))
    assert x.finish_frame([])[2]["overlap_valid"] == 1
    # cleared: a new map, a last frame from the host, a last frame from a keyframe
    x.set_map(dict(x.download_map(), cam=cam))
    assert x.finish_frame([])[2]["need_new_kf"] == -1
    x.set_last_frame(r7["T_f_w"], r7["feat_px"], r7["feat_f"], r7["feat_point"], kf_slot=1)
    d = x.finish_frame([])[2]
    _assert_decision(d, kd.decision(x.download_map(), r7["T_f_w"], r7["feat_point"], None, 0.12), "set_last_frame")
    assert d["overlap_valid"] == 0 and d["n_depths"] == int((r7["feat_point"] >= 0).sum())
    x.track(_img(seq, 7))
    assert x.finish_frame([])[2]["overlap_valid"] == 1
    assert x.last_frame_from_keyframe(1) > 0
    assert x.finish_frame([])[2]["overlap_valid"] == 0
    x.destroy()


def test_overlap_valid_after_a_relocalisation(ctx, seq):
    x, rs = _lead(ctx, seq)
    T5 = rs[-1]["T_f_w"].copy()
    rx = x.relocalize(_img(seq, 6), T5)
    assert rx["reloc"].accepted == 1
    d = x.finish_frame([])[2]
    _assert_decision(d, _model_after(x, rx, 0.12), "accepted relocalisation")
    assert d["overlap_valid"] == 1
    rx = x.relocalize(_img(seq, 7), rx["T_f_w"], min_tracked=10 ** 6)              # the gate refuses
    assert rx["reloc"].accepted == 0 and rx["reloc"].kf_index >= 0
    d = x.finish_frame([])[2]
    assert (d["overlap_valid"], d["need_new_kf"], d["n_depths"]) == (0, -1, 0) and math.isnan(d["depth_mean"])
    x.destroy()


# ---- refusals
def test_refusals_change_nothing(ctx, seq):
    fresh = hip.Tracker(ctx, CAM, **SMALL)
    with pytest.raises(hip.SvoHipError, match=STATE):
        fresh.finish_frame([])                                                     # no map
    fresh.set_map(kd.line_map(2))
    with pytest.raises(hip.SvoHipError, match=STATE):
        fresh.finish_frame([])                                                     # no last frame
    fresh.destroy()
    x, rs = _lead(ctx, seq)
    sel = _selection(rs[-1])
    before, d0 = x.download_map(), x.finish_frame([])[2]
    n_points = before["n_points"]
    bad = [lambda: x.finish_frame(sel, kf_select_min_dist=float("nan")), lambda: x.finish_frame(sel, kf_select_min_dist=-0.01),
           lambda: x.finish_frame(sel, n_iter=-1), lambda: x.finish_frame(list(range(65))), lambda: x.finish_frame([sel[0], sel[1], sel[0]]),
           lambda: x.finish_frame([sel[0], n_points]), lambda: x.finish_frame([-1])]
    for i, call in enumerate(bad):
        with pytest.raises(hip.SvoHipError, match=INVALID):
            call()
    pt = np.array(sel, np.int32)
    pos = np.zeros((len(sel), 3))
    rc = ctx.lib.svo_hip_tracker_finish_frame(x.h, len(pt), pt.ctypes.data_as(C.POINTER(C.c_int32)), 5, pos.ctypes.data_as(C.POINTER(C.c_double)), None,
                                              C.c_double(0.12), None)              # decision == NULL
    assert rc == -1 and not pos.any()
    mg.assert_tables_equal(x.download_map(), before)
    _same_decision(x.finish_frame([])[2], d0, "after the refusals")
    assert x.finish_frame(sel, kf_select_min_dist=0.0)[2]["need_new_kf"] == 1       # zero is a distance: nothing is nearer
    x.destroy()


# ---- the group
def test_group_equals_the_lone_calls(ctx):
    cs = ms.small_case()
    cfg = dict(max_keyframes=cs["n_kf"], grid_size=cs["cell_size"])
    img = cs["cur_pyr"][0]

    def prepare(c, trk):
        """camera c's map and last frame (3: a map, no last frame)"""
        for k in range(cs["n_kf"]):
            trk.upload_keyframe(k, cs["kf_pyr"][k][0])
        trk.set_map(cs)
        if c == 0:
            trk.last_frame_from_keyframe(1)
        elif c == 1:
            trk.set_last_frame(cs["T_cur_w"], np.zeros((0, 2)), np.zeros((0, 3)), np.zeros(0, np.int32), img=img)
            trk.remove_keyframe(2)
            trk.last_frame_from_keyframe(3)
        elif c == 2:
            pts = np.array([5, -1, 7, 9, -1, 11, 200], np.int32)
            trk.set_last_frame(cs["T_cur_w"], np.zeros((len(pts), 2)), np.tile([0.0, 0.0, 1.0], (len(pts), 1)), pts, img=img)

    def living(trk, n):
        m = trk.download_map()
        has_obs = np.flatnonzero(np.diff(m["pt_obs_offset"]) >= 2)
        return [int(p) for p in has_obs[:n]]

    grp = hip.TrackerGroup(ctx, cs["cam"], 4, **cfg)
    lone = [hip.Tracker(ctx, cs["cam"], **cfg) for _ in range(3)]
    for c in range(4):
        prepare(c, grp.cameras[c])
    for c in range(3):
        prepare(c, lone[c])
    req = [(living(grp.cameras[0], 20), 5), (living(grp.cameras[1], 7), 3), None, None]
    maps0 = [grp.cameras[c].download_map() for c in range(3)]
    # a bad request for camera 2 refuses the whole call: cameras 0 and 1 are untouched
    for bad in ([0, 0], [cs["n_points"]]):
        with pytest.raises(hip.SvoHipError, match=INVALID):
            grp.finish_frames([req[0], req[1], bad, None])
    with pytest.raises(hip.SvoHipError, match=INVALID):
        grp.finish_frames([req[0], req[1], None, [1]])                             # a camera that sits out has nothing to optimise
    with pytest.raises(hip.SvoHipError, match=INVALID):
        grp.finish_frames(req, kf_select_min_dist=float("nan"))
    for c in range(3):
        mg.assert_tables_equal(grp.cameras[c].download_map(), maps0[c])
    out = grp.finish_frames(req, kf_select_min_dist=0.12)
    assert out[3][2] is None and all(out[c][2] is not None for c in range(3))      # camera_ok = 1, 1, 1, 0
    n_depths = []
    for c in range(3):
        pts, n_iter = req[c] if req[c] is not None else ([], 0)
        pos, it, dec = lone[c].finish_frame(pts, n_iter=n_iter, kf_select_min_dist=0.12)
        assert out[c][0].tobytes() == pos.tobytes() and out[c][1].tobytes() == it.tobytes(), c
        _same_decision(out[c][2], dec, ("camera", c))
        _same_decision(grp.cameras[c].finish_frame([], kf_select_min_dist=0.12)[2], dec, ("camera's own handle", c))
        mg.assert_tables_equal(grp.cameras[c].download_map(), lone[c].download_map())
        m = grp.cameras[c].download_map()
        _assert_decision(dec, kd.decision(m, _last_pose(cs, m, c), _last_points(cs, m, c), None, 0.12), ("model", c))
        n_depths.append(dec["n_depths"])
    assert len(set(n_depths)) == 3 and n_depths[2] == 5 and len(out[0][0]) == 20 and len(out[1][0]) == 7
    assert [len(o[0]) for o in out[2:]] == [0, 0]
    none = grp.finish_frames(None, kf_select_min_dist=0.12)                         # no structure step anywhere
    for c in range(3):
        _same_decision(none[c][2], out[c][2], ("requests = NULL", c))
    with pytest.raises(hip.SvoHipError, match=STATE):
        grp.cameras[3].finish_frame([])
    for t in lone:
        t.destroy()
    grp.destroy()


def test_group_after_tracked_frames(ctx, seq):
    """the overlap list through the group's kernel: two cameras track two frames together, one call finishes both"""
    grp = hip.TrackerGroup(ctx, seq["cam"], 2, **SEQ_CFG)
    mp = tc.sequence_map(seq)
    for cam in grp.cameras:
        _start(cam, seq, mp)
    for k in (1, 2):
        grp.track([_img(seq, k), _img(seq, k)])
    rs = [cam.last_result() for cam in grp.cameras]
    out = grp.finish_frames([(_selection(rs[0]), 5), None], kf_select_min_dist=0.12)
    assert len(out[0][0]) == 20 and len(out[1][0]) == 0
    for c in range(2):
        dec = out[c][2]
        _assert_decision(dec, _model_after(grp.cameras[c], rs[c], 0.12), ("camera", c))
        _same_decision(grp.cameras[c].finish_frame([], kf_select_min_dist=0.12)[2], dec, ("camera's own handle", c))
        assert dec["overlap_valid"] == 1 and dec["need_new_kf"] in (0, 1) and dec["n_depths"] >= 50
    assert grp.cameras[0].download_map()["pt_pos"].tobytes() != grp.cameras[1].download_map()["pt_pos"].tobytes()
    far = grp.finish_frames(None, kf_select_min_dist=1e6)
    assert all((far[c][2]["need_new_kf"], far[c][2]["blocking_kf"]) == (0, int(rs[c]["overlap_kf"][0])) for c in range(2))
    grp.destroy()


def _last_pose(cs, m, c):
    return m["T_kf_w"][1] if c == 0 else m["T_kf_w"][3] if c == 1 else cs["T_cur_w"]


def _last_points(cs, m, c):
    """the points of the camera's last frame: the living entries of the keyframe's feature row, or the list set by hand"""
    if c == 2:
        return np.array([5, -1, 7, 9, -1, 11, 200], np.int32)
    import relocalise_reference as rl
    k = 1 if c == 0 else 3
    return rl.last_frame_from_keyframe(dict(m, cam=cs["cam"]), k)["point"]


# ---- the host twin
def test_host_twin_decides_on_the_device(tmp_path):
    """hip_bridge::FrameTrackerT::finishFrame on the C++ twins (svo_host_demo track incremental kf_every 2 max_kfs 3, manifest field
    21 = kf_select_min_dist): every frame is finished by one device call, the host twins decide again on the objects and both
    decisions are written to track_decision.bin; the keyframe that leaves the bounded map is the one the device named (the run
    throws if Map::getFurthestKeyframe names another).  Without the field -- or with it at zero -- the mode is off."""
    import os
    import subprocess
    from test_gpu_host_cpp import DEMO, _write, _write_track_case
    assert os.path.exists(DEMO)
    n_frames = 11
    seq = tc.make_sequence(n_frames=n_frames + 1)
    mp = tc.sequence_map(seq)
    n = len(seq["px0"])
    cs = dict(mp, obs_point=np.arange(n, dtype=np.int32), kf_ftr_obs=np.arange(n, dtype=np.int32), cand_obs=np.zeros(0, np.int32))
    cfg = dict(grid_size=tc.CELL, max_fts=tc.MAX_FTS, quality_min_fts=40, klt_min_level=2, max_frame_features=1024, keyframe_at=1)
    outs = {}
    for tag, field in (("off", None), ("zero", 0.0), ("on", 0.12)):
        case, out = tmp_path / ("case_" + tag), tmp_path / ("out_" + tag)
        case.mkdir()
        out.mkdir()
        _write_track_case(case, cs, [seq["pyrs"][k][0] for k in range(1, n_frames + 1)], cfg, last_kf=0)
        manifest = np.fromfile(case / "track_manifest.bin")
        assert len(manifest) == 21                                                 # the new field is the next one
        if field is not None:
            _write(case / "track_manifest.bin", list(manifest) + [field], np.float64)
        p = subprocess.run([DEMO, str(case), str(out), "track", "incremental", "kf_every", "2", "max_kfs", "3"], capture_output=True, text=True,
                           timeout=300, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
        assert p.returncode == 0, p.stdout + p.stderr
        outs[tag] = out
    names = sorted(os.listdir(outs["off"]))
    assert "track_decision.bin" not in names and names == sorted(os.listdir(outs["zero"]))
    for f in names:
        assert (outs["off"] / f).read_bytes() == (outs["zero"] / f).read_bytes(), f
    assert sorted(os.listdir(outs["on"])) == sorted(names + ["track_decision.bin"])
    dec = np.fromfile(outs["on"] / "track_decision.bin").reshape(n_frames, 13)
    print(dec)
    assert dec[:, :6].tobytes() == dec[:, 6:12].tobytes()                          # the device's decision is the host's, bit for bit
    assert (dec[:, 12] == np.arange(1, n_frames + 1)).all()                        # one device decision per frame
    assert (dec[:, 0] == 1).all() and (dec[:, 3] == 1).all() and (dec[:, 2] <= dec[:, 1]).all() and (dec[:, 5] >= 0).all()
    assert set(dec[:, 4]) <= {0.0, 1.0}
    removed = np.fromfile(outs["on"] / "track_removed.bin")
    assert int((removed >= 0).sum()) >= 3 and (removed[removed >= 0] == dec[removed >= 0, 5]).all()      # ... and it is the one that left
    assert (np.fromfile(outs["on"] / "track_uploads.bin") == 1).all()
    stats = np.fromfile(outs["on"] / "track_stats.bin").reshape(n_frames, 9)
    assert (stats[:, 1] >= 40).all() and (stats[:, 4] == 1).all()
