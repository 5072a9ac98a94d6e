"""A keyframe leaves the device map in place: svo_hip_tracker_remove_keyframe against the model of tests/map_removal_reference.py
(Map::safeDeleteFrame restated on the index tables) and against a tracker that gets the model's tables through
svo_hip_tracker_set_map under the same point numbering.  Every comparison is exact: integers equal, doubles byte-equal.

Tracker X uses the call, tracker Y today's path: set_map of the model's tables and, where the model says the last frame loses
points, set_last_frame with those features at -1.  tests/test_map_removal_model.py establishes on the CPU that on every removal
used here the reference's re-selection rule and the device's give the same key points; the constructed tie case, where they do
not, holds the device to its own."""
import os
import subprocess

import numpy as np
import pytest

import map_growth_reference as mg
import map_growth_scenario as sc
import map_removal_reference as mr
import map_removal_scenario as ms
import tracking_chain as tc
from test_gpu_map_growth import _frames, _same, _start, _wide_tracker, _with_counters
from android_svo_amd import hip, synth

pytestmark = pytest.mark.gpu

CFG = dict(max_keyframes=3, grid_size=tc.CELL, max_fts=tc.MAX_FTS, klt_min_level=2, max_frame_features=1024)


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases():
    return dict(small=ms.small_case(), wide=ms.wide_case(), tie=ms.tie_case())


def _map_tracker(ctx, cs, images=True, **cfg):
    """a tracker that holds the case's map (and, with images, its keyframes and current frame as _wide_tracker sets them up)"""
    if images:
        return _wide_tracker(ctx, cs, cs["kf_key_point"], **cfg)
    trk = hip.Tracker(ctx, cs["cam"], max_keyframes=cs["n_kf"], grid_size=cs["cell_size"], **cfg)
    trk.set_map(cs)
    return trk


def _sizes(t):
    t = mg.normalised(t)
    return dict(n_kf=t["n_kf"], n_ftr=len(t["kf_ftr_point"]), n_points=t["n_points"], n_obs=len(t["obs_kf"]), n_candidates=len(t["cand_point"]))


def _counts(info):
    return dict(slot=info["slot"], n_deleted_points=len(info["deleted_points"]), n_deleted_candidates=len(info["deleted_candidates"]))


# ---- 1. the tables
@pytest.mark.parametrize("fam,k", ms.REMOVALS + (("tie", 1),), ids=["%s-%d" % r for r in ms.REMOVALS] + ["tie-1"])
def test_tables_after_a_removal(ctx, cases, fam, k):
    cs = cases[fam]
    trk = _map_tracker(ctx, cs, images=False)
    got = trk.remove_keyframe(k)
    dl, sizes = trk.download_map(), trk.map_sizes()
    trk.destroy()
    # the tie case is where the device's rule (once per keyframe) and the reference's part: the device is held to its own
    model, info = mr.remove_keyframe(cs, k, rekey="once" if fam == "tie" else "per_deletion")
    assert got == _counts(info) and sizes == _sizes(model)
    mg.assert_tables_equal(dl, model)
    if fam == "tie":
        assert (mr.remove_keyframe(cs, k)[0]["kf_key_point"] != dl["kf_key_point"]).sum() == 1


# ---- 2. and 3. the wide case: its first frame deletes points, then a keyframe leaves, then two more frames
def _wide_frames(cs):
    _, kw, _ = ms.wide_args()
    scene = synth.PlaneScene(seed=kw.get("seed", 31), depth=2.0, tilt=(0.08, -0.05))
    step = synth.se3_from_twist([0.012, -0.006, 0.004], [0.002, -0.003, 0.001])
    T2 = synth.se3_mul(step, cs["T_cur_w"])
    return [scene.render(cs["cam"], T2), scene.render(cs["cam"], synth.se3_mul(step, T2))]


@pytest.fixture(scope="module")
def wide_first(ctx, cases):
    """an untouched tracker on the wide case: its tables, its first frame (which deletes points) and the tables after it"""
    cs = cases["wide"]
    trk = _map_tracker(ctx, cs, max_fts=ms.wide_args()[2])
    before = trk.download_map()
    r = trk.track(cs["cur_pyr"][0])
    after = trk.download_map()
    trk.destroy()
    assert r["map_changed"] == 1
    unl = (r["type"] == synth.TYPE_DELETED) & (cs["pt_type"] != synth.TYPE_DELETED)
    assert unl.sum() >= 10 and (after["kf_key_point"] != before["kf_key_point"]).any()         # a re-selection was owed
    return dict(before=before, r=r, unlinked=unl, tables=_with_counters(cs, r))


def _wide_model(cs, wf, k):
    tables = dict(wf["tables"], cam=cs["cam"])
    model, info = mr.remove_keyframe(tables, k, unlinked=wf["unlinked"], last_point=wf["r"]["feat_point"])
    once = mr.remove_keyframe(tables, k, unlinked=wf["unlinked"], rekey="once")[0]
    assert np.array_equal(model["kf_key_point"], once["kf_key_point"])                           # both rules agree here too
    return model, info


@pytest.mark.parametrize("k", [1, 6])
def test_tables_after_deletions_by_tracking(ctx, cases, wide_first, k):
    cs, wf = cases["wide"], wide_first
    trk = _map_tracker(ctx, cs, max_fts=ms.wide_args()[2])
    _same(trk.track(cs["cur_pyr"][0]), wf["r"], "first frame")
    got = trk.remove_keyframe(k)                                                                 # (the owed re-selection is still pending)
    dl, sizes = trk.download_map(), trk.map_sizes()
    trk.destroy()
    model, info = _wide_model(cs, wf, k)
    assert got == _counts(info) and sizes == _sizes(model)
    mg.assert_tables_equal(dl, model)
    gone = wf["unlinked"].copy()
    gone[info["deleted_points"] + info["deleted_candidates"]] = True
    mr.check_invariants(dl, gone)
    assert len(dl["cand_point"]) < len(cs["cand_point"]) - len(info["deleted_candidates"])      # candidates the frame deleted left the list too


@pytest.mark.parametrize("k,loses", [(0, False), (6, True)])
def test_next_frames_after_a_removal(ctx, cases, wide_first, k, loses):
    """the last frame is no keyframe here; with k = 6 some of its features lose their point all the same"""
    cs, wf = cases["wide"], wide_first
    model, info = _wide_model(cs, wf, k)
    assert bool(info["last_lost"]) == loses and (not loses or len(info["last_lost"]) >= 5)
    frames = _wide_frames(cs)
    out = []
    for in_place in (True, False):
        trk = _map_tracker(ctx, cs, max_fts=ms.wide_args()[2])
        r = trk.track(cs["cur_pyr"][0])
        if in_place:
            assert trk.remove_keyframe(k) == _counts(info)
        else:
            trk.set_map(model)
            if loses:
                pts = r["feat_point"].copy()
                pts[info["last_lost"]] = -1
                trk.set_last_frame(r["T_f_w"], r["feat_px"], r["feat_f"], pts, img=cs["cur_pyr"][0])
        out.append([trk.track(f) for f in frames] + [trk.download_map()])
        trk.destroy()
    for i in range(len(frames)):
        _same(out[0][i], out[1][i], ("frame", i))
        assert out[0][i]["n_matches"] >= 50
    mg.assert_tables_equal(out[0][-1], out[1][-1])


# ---- 3. and 4. the steady state: a map of three keyframes at most that keeps running on one upload
def _new_candidates(s, T_kf):
    """the held-back points once more, a tenth of a millimetre off, as seeds of the keyframe with pose T_kf"""
    cam, held = s["seq"]["cam"], s["cand"]
    px = tc.project(cam, T_kf, held["pos"])
    ok = (px[:, 0] >= 8) & (px[:, 0] < cam.width - 8) & (px[:, 1] >= 8) & (px[:, 1] < cam.height - 8)
    n = int(ok.sum())
    return dict(pos=held["pos"][ok] + 1e-4, kf_index=np.zeros(n, np.int32), px=px[ok], f=synth.cam2world(cam, px[ok]), level=np.zeros(n, np.int32))


def _steady_x(trk, s, track=None):
    """track, promote, (candidates), track, promote, remove keyframe 0, track, (candidates of the keyframe that is now 0), track,
    promote into the freed slot, track -- through the in-place calls"""
    seq = s["seq"]
    track = track or (lambda frames: _frames(trk, seq, frames))
    out = dict(f12=track((1, 2)))
    out["promote1"] = trk.promote_last_frame(1)
    out["first"] = trk.add_candidates(**s["cand"])
    out["f34"] = track((3, 4))
    out["promote2"] = trk.promote_last_frame(2)
    out["map_full"] = trk.download_map()
    with pytest.raises(hip.SvoHipError, match=r"\(-1\)"):                                        # max_keyframes: no room without the removal
        trk.promote_last_frame(0)
    out["remove"] = trk.remove_keyframe(0)
    out["last_after_remove"] = trk.last_result()
    out["map_removed"], out["sizes_removed"] = trk.download_map(), trk.map_sizes()
    out["f5"] = track((5,))
    out["first2"] = trk.add_candidates(**_new_candidates(s, out["f12"][-1]["T_f_w"]))
    out["map_added"] = trk.download_map()
    out["f6"] = track((6,))
    out["promote3"] = trk.promote_last_frame(out["remove"]["slot"])
    out["map_final"] = trk.download_map()
    out["f78"] = track((7, 8))
    return out


FRAME_PARTS = ("f12", "f34", "f5", "f6", "f78")


@pytest.fixture(scope="module")
def scen():
    return sc.make()


@pytest.fixture(scope="module")
def steady(ctx, scen):
    seq, cam, base_map = scen["seq"], scen["seq"]["cam"], scen["base_map"]
    x = hip.Tracker(ctx, cam, **CFG)
    _start(x, scen["base"], base_map)
    X = _steady_x(x, scen)
    x.destroy()
    y = hip.Tracker(ctx, cam, **CFG)
    _start(y, scen["base"], base_map)
    Y = dict(f12=_frames(y, seq, (1, 2)))
    m1, _ = mg.promote(base_map, Y["f12"][-1], 1, cam)
    m2, Y["first"] = mg.append_candidates(m1, **scen["cand"])
    y.keyframe_from_last_frame(1)
    y.set_map(m2)
    Y["f34"] = _frames(y, seq, (3, 4))
    r = Y["f34"][-1]
    Y["map_full"], Y["n_promoted2"] = mg.promote(m2, r, 2, cam)
    unl = Y["map_full"]["pt_type"] == synth.TYPE_DELETED                                        # (the base map has no deleted point)
    Y["map_removed"], Y["info"] = mr.remove_keyframe(Y["map_full"], 0, unlinked=unl, cam=cam, last_point=r["feat_point"])
    once = mr.remove_keyframe(Y["map_full"], 0, unlinked=unl, cam=cam, rekey="once")[0]
    assert np.array_equal(once["kf_key_point"], Y["map_removed"]["kf_key_point"])
    y.keyframe_from_last_frame(2)
    y.set_map(Y["map_removed"])
    pts = r["feat_point"].copy()
    pts[Y["info"]["last_lost"]] = -1
    y.set_last_frame(r["T_f_w"], r["feat_px"], r["feat_f"], pts, kf_slot=2)
    Y["f5"] = _frames(y, seq, (5,))
    Y["map_added"], Y["first2"] = mg.append_candidates(_with_counters(Y["map_removed"], Y["f5"][-1]), **_new_candidates(scen, Y["f12"][-1]["T_f_w"]))
    y.set_map(Y["map_added"])
    Y["f6"] = _frames(y, seq, (6,))
    slot = Y["info"]["slot"]
    Y["map_final"], Y["n_promoted3"] = mg.promote(Y["map_added"], Y["f6"][-1], slot, cam)
    y.keyframe_from_last_frame(slot)
    y.set_map(Y["map_final"])
    Y["f78"] = _frames(y, seq, (7, 8))
    y.destroy()
    return X, Y


def test_last_keyframe_loses_points_with_the_removed_one(steady):
    """a point seen only by the removed keyframe and by the promoted last frame is deleted, and the last frame's feature loses it:
    the frames that follow equal those of a tracker whose last frame was set again without those points"""
    X, Y = steady
    info, r, full = Y["info"], Y["f34"][-1], Y["map_full"]
    lost = r["feat_point"][info["last_lost"]]
    assert len(lost) >= 5 and set(lost.tolist()) <= set(info["deleted_points"])
    for p in lost:                                                                               # seen by keyframe 2 (the last frame) and keyframe 0 only
        assert full["obs_kf"][full["pt_obs_offset"][p]:full["pt_obs_offset"][p + 1]].tolist() == [2, 0]
    for part in ("f5", "f6"):
        for i, (a, b) in enumerate(zip(X[part], Y[part])):
            _same(a, b, (part, i))
        assert all(a["n_matches"] >= 50 and not set(a["feat_point"].tolist()) & set(lost.tolist()) for a in X[part])
    _same(X["last_after_remove"], X["f34"][-1], "the result block of the last tracked frame is not rewritten")


def test_steady_state_on_one_upload(steady):
    X, Y = steady
    info = Y["info"]
    assert X["first"] == Y["first"] and X["first2"] == Y["first2"] == Y["map_removed"]["n_points"]
    assert X["promote1"] == (1, 0) and X["promote2"] == (2, Y["n_promoted2"]) and Y["n_promoted2"] >= 5
    # the removal: points of all three kinds, candidates, both remaining keyframes choose key points again
    assert X["remove"] == _counts(info) and X["remove"]["slot"] == 0 and X["sizes_removed"] == _sizes(Y["map_removed"])
    assert len(info["deleted_points"]) >= 100 and len(info["deleted_candidates"]) >= 50 and set(info["rekeys"]) == {1, 2}
    n_obs = np.diff(Y["map_full"]["pt_obs_offset"])
    assert all((n_obs == n).sum() >= 20 for n in (1, 2, 3))
    # the freed slot takes the next keyframe, which is keyframe 2 again
    assert X["promote3"] == (2, Y["n_promoted3"]) and Y["n_promoted3"] >= 5
    assert X["map_final"]["kf_slot"].tolist() == [1, 2, 0]
    for name in ("map_full", "map_removed", "map_added", "map_final"):
        mg.assert_tables_equal(X[name], Y[name])
    # candidates appended after the removal: seeds of the keyframe that was 1 and is 0 now
    added = Y["map_added"]
    new = np.arange(Y["first2"], added["n_points"])
    assert len(new) >= 100 and (X["map_added"]["obs_kf"][added["pt_obs_offset"][new]] == 0).all()
    assert X["map_added"]["cand_point"].tolist() == new.tolist()                                 # (the removal had emptied the list)
    for part in FRAME_PARTS:
        for i, (a, b) in enumerate(zip(X[part], Y[part])):
            _same(a, b, (part, i))
    assert all(2 in list(r["overlap_kf"]) for r in X["f78"]) and all(r["n_matches"] >= 50 for r in X["f78"])


# ---- 5. refusals
def test_refusals_change_nothing(ctx, cases, wide_first, steady, scen):
    cs, wf = cases["wide"], wide_first
    trk = hip.Tracker(ctx, cs["cam"], max_keyframes=cs["n_kf"], grid_size=cs["cell_size"], quality_min_fts=20, max_fts=ms.wide_args()[2])
    with pytest.raises(hip.SvoHipError, match=r"\(-4\)"):                                        # no map
        trk.remove_keyframe(0)
    trk.destroy()
    trk = _map_tracker(ctx, cs, max_fts=ms.wide_args()[2])
    for k in (-1, cs["n_kf"]):
        with pytest.raises(hip.SvoHipError, match=r"\(-1\)"):
            trk.remove_keyframe(k)
        assert trk.map_sizes() == _sizes(cs)
    mg.assert_tables_equal(trk.download_map(), wf["before"])
    _same(trk.track(cs["cur_pyr"][0]), wf["r"], "after refusals")
    trk.destroy()
    # the only keyframe stays
    seq = scen["seq"]
    trk = hip.Tracker(ctx, seq["cam"], **CFG)
    _start(trk, scen["base"], scen["base_map"])
    with pytest.raises(hip.SvoHipError, match=r"\(-1\)"):
        trk.remove_keyframe(0)
    assert trk.map_sizes() == _sizes(scen["base_map"])
    mg.assert_tables_equal(trk.download_map(), scen["base_map"])
    _same(trk.track(seq["pyrs"][1][0]), steady[0]["f12"][0], "the only keyframe")
    trk.destroy()


# ---- 6. a camera of a group
def test_group_camera_removes_a_keyframe(ctx, scen):
    """camera 0 of a group goes through the steady-state chain, camera 1 tracks on its one keyframe: each equals its lone tracker
    under the same calls (the sums of SparseImgAlign grouped by tile on both sides, so that nothing depends on the company)"""
    seq, full_map = scen["seq"], tc.sequence_map(scen["seq"])
    tile = (hip.SIA_OPT_REDUCTION, hip.SIA_REDUCTION_TILE_ORDER)
    cfg = dict(CFG, max_items=1024)
    lone0 = hip.Tracker(ctx, seq["cam"], **cfg)
    lone0.set_sia_option(*tile)
    _start(lone0, scen["base"], scen["base_map"])
    want0 = _steady_x(lone0, scen)
    lone0.destroy()
    lone1 = hip.Tracker(ctx, seq["cam"], **cfg)
    lone1.set_sia_option(*tile)
    _start(lone1, seq, full_map)
    want1 = _frames(lone1, seq, range(1, sc.N_FRAMES))
    map1 = lone1.download_map()
    lone1.destroy()
    grp = hip.TrackerGroup(ctx, seq["cam"], 2, **cfg)
    grp.set_sia_option(*tile)
    _start(grp.cameras[0], scen["base"], scen["base_map"])
    _start(grp.cameras[1], seq, full_map)
    got1 = []

    def track(frames):
        out = []
        for k in frames:
            grp.track([seq["pyrs"][k][0]] * 2)
            out.append(grp.cameras[0].last_result())
            got1.append(grp.cameras[1].last_result())
        return out
    got0 = _steady_x(grp.cameras[0], scen, track=track)
    for name in ("promote1", "first", "promote2", "remove", "sizes_removed", "first2", "promote3"):
        assert got0[name] == want0[name], name
    assert got0["remove"]["n_deleted_points"] >= 100
    for part in FRAME_PARTS:
        for i, (a, b) in enumerate(zip(got0[part], want0[part])):
            _same(a, b, (0, part, i))
    for name in ("map_full", "map_removed", "map_added", "map_final"):
        mg.assert_tables_equal(got0[name], want0[name])
    for i, (a, b) in enumerate(zip(got1, want1)):
        _same(a, b, (1, i))
    mg.assert_tables_equal(grp.cameras[1].download_map(), map1)
    assert grp.cameras[1].map_sizes()["n_kf"] == 1
    grp.destroy()


# ---- 7. the C++ host twin
def _track_files(d):
    return sorted(f for f in os.listdir(d) if f.startswith("track_") and f.endswith(".bin"))


@pytest.mark.parametrize("max_kfs,kf_every,keyframe_at,n_frames,min_removals", [(3, 2, 1, 11, 3), (10, 1, 0, 30, 20)], ids=["three", "ten"])
def test_host_twin_removes_keyframes_in_place(tmp_path, max_kfs, kf_every, keyframe_at, n_frames, min_removals):
    """hip_bridge::FrameTrackerT on the C++ twins (svo_host_demo track incremental kf_every E max_kfs N): every E-th frame becomes
    a keyframe, the map holds N at most, the furthest one leaves when a new one joins (FrameHandlerMono::processFrame :303-308).
    With keyframeRemoved the map is uploaded once; every file the demo writes about the tracked frames is byte for byte what the
    same run writes when each removal flattens and uploads the map again (full_remove).  "ten" is Config::maxNKfs()'s own bound:
    thirty keyframes in a row, from the tenth on each with a removal, the pyramid slots 0..10 going round."""
    from test_gpu_host_cpp import DEMO, _write_track_case
    assert os.path.exists(DEMO)
    seq = tc.make_sequence(n_frames=n_frames + 1)
    mp = tc.sequence_map(seq)
    n = len(seq["px0"])
    cs = dict(mp, obs_point=np.arange(n, dtype=np.int32), kf_ftr_obs=np.arange(n, dtype=np.int32), cand_obs=np.zeros(0, np.int32))
    cfg = dict(grid_size=tc.CELL, max_fts=tc.MAX_FTS, quality_min_fts=40, klt_min_level=2, max_frame_features=1024, keyframe_at=keyframe_at)
    case = tmp_path / "case"
    case.mkdir()
    _write_track_case(case, cs, [seq["pyrs"][k][0] for k in range(1, n_frames + 1)], cfg, last_kf=0)
    common = ["incremental", "kf_every", str(kf_every), "max_kfs", str(max_kfs)]
    outs = []
    for extra in (common, common + ["full_remove"]):
        out = tmp_path / ("out_" + extra[-1])
        out.mkdir()
        p = subprocess.run([DEMO, str(case), str(out), "track"] + extra, capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
        assert p.returncode == 0, p.stdout + p.stderr
        outs.append(out)
    names = _track_files(outs[0])
    assert len(names) > 10 and names == _track_files(outs[1])
    for f in names:
        if f != "track_uploads.bin":
            assert (outs[0] / f).read_bytes() == (outs[1] / f).read_bytes(), f
    removed = np.fromfile(outs[0] / "track_removed.bin")
    n_removed = int((removed >= 0).sum())
    assert n_removed >= min_removals, removed
    size = np.fromfile(outs[0] / "track_map_size.bin")
    assert size[0] == max_kfs and size[2] >= 50                                                  # the bound holds, the map is alive
    stats = np.fromfile(outs[0] / "track_stats.bin").reshape(n_frames, 9)
    assert (stats[:, 1] >= 40).all() and (stats[:, 4] == 1).all()                                # every frame matched and was refined
    up = np.fromfile(outs[0] / "track_uploads.bin")
    assert len(up) == n_frames and (up == 1).all(), up
    full = np.fromfile(outs[1] / "track_uploads.bin")
    assert full[-1] >= n_removed and (np.diff(full) >= 0).all(), full
