"""Relocalisation against a keyframe of the device map: svo_hip_tracker_closest_keyframe, svo_hip_tracker_last_frame_from_keyframe
and svo_hip_tracker_relocalize against the numpy models of tests/relocalise_reference.py (tests/test_relocalise_model.py
establishes the models' own properties on the CPU), against the composition the older entry points allow -- host flatten,
svo_hip_tracker_set_last_frame, a separate SparseImgAlign solver for the gate, svo_hip_tracker_track -- and against the oracle.
Comparisons with the model and with the composition are exact: integers equal, doubles byte-equal."""
import numpy as np
import pytest

import map_compaction_reference as mc
import map_growth_reference as mg
import map_removal_reference as mr
import map_removal_scenario as ms
import relocalise_reference as rl
import tracking_chain as tc
from test_gpu_map_growth import _fields, _frames, _same, _start
from test_gpu_map_removal import _map_tracker
from android_svo_amd import hip, synth

pytestmark = pytest.mark.gpu

CFG = dict(max_keyframes=4, grid_size=tc.CELL, max_fts=tc.MAX_FTS, klt_min_level=2, max_frame_features=1024)
STATE, INVALID = r"\(-4\)", r"\(-1\)"


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases():
    return dict(small=ms.small_case(), wide=ms.wide_case(), tie=rl.tie_map()[0])


def _tile_order(trk):
    trk.set_sia_option(hip.SIA_OPT_REDUCTION, hip.SIA_REDUCTION_TILE_ORDER)
    return trk


def _reloc_fields(r):
    return _fields(r["reloc"])


# ---- 4. the closest keyframe
@pytest.mark.parametrize("fam", ["small", "wide", "tie"])
def test_closest_keyframe_against_the_model(ctx, cases, fam):
    cs = cases[fam]
    trk = _map_tracker(ctx, cs, images=False)
    poses = rl.probes(cs) + ([rl.tie_map()[1]] if fam == "tie" else [])
    seen = set()
    for i, T in enumerate(poses):
        for exclude in (-1, i % cs["n_kf"]):
            want, got = rl.closest_keyframe(cs, T, exclude), trk.closest_keyframe(T, exclude)
            print(fam, i, exclude, got, want["kf_index"], want["n_close"], want["distance"])
            assert (got["kf_index"], got["n_close"]) == (want["kf_index"], want["n_close"]), (fam, i, exclude)
            assert np.float64(got["distance"]).tobytes() == np.float64(want["distance"]).tobytes(), (fam, i, exclude)
            seen.add(got["kf_index"])
    assert -1 in seen and len(seen) >= 3
    if fam == "tie":
        T = rl.tie_map()[1]
        assert trk.closest_keyframe(T)["kf_index"] == 0 and trk.closest_keyframe(T, 0)["kf_index"] == 1      # the lower index wins the tie
    # the pose of the device's last frame
    with pytest.raises(hip.SvoHipError, match=STATE):
        trk.closest_keyframe(None)
    T = poses[1]
    trk.set_last_frame(T, np.zeros((0, 2)), np.zeros((0, 3)), np.zeros(0, np.int32), img=np.zeros((cs["cam"].height, cs["cam"].width), np.uint8))
    assert trk.closest_keyframe(None) == trk.closest_keyframe(T)
    trk.destroy()
    fresh = hip.Tracker(ctx, cs["cam"], max_keyframes=2, max_fts=120, max_frame_features=128)
    with pytest.raises(hip.SvoHipError, match=STATE):
        fresh.closest_keyframe(poses[0])
    fresh.destroy()


# ---- 5. the last frame from a keyframe
def _small_compacted(cs):
    removed, info = mr.remove_keyframe(cs, 2)
    dead = np.zeros(cs["n_points"], bool)
    dead[info["deleted_points"] + info["deleted_candidates"]] = True
    assert dead.sum() >= 30
    return dict(mc.compact_points(removed, dead, cam=cs["cam"])[0], cam=cs["cam"])


def _x_and_y(ctx, cs, k, compacted):
    """X: the call under test; Y: the same tables through set_map, the last frame from the host flatten of the model.  Both
    track the case's current image.  Returns (n_features, flatten, X's result and map, Y's)."""
    x, y = _tile_order(_map_tracker(ctx, cs)), _tile_order(_map_tracker(ctx, cs))
    tables = cs
    if compacted:
        x.remove_keyframe(2)
        x.compact_points()
        tables = _small_compacted(cs)
        y.set_map(tables)
    n = x.last_frame_from_keyframe(k)
    with pytest.raises(hip.SvoHipError, match=STATE):
        x.promote_last_frame(2)                                                    # not a tracked frame
    flat = rl.flatten_keyframe(tables, k)
    y.set_last_frame(flat["T_f_w"], flat["px"], flat["f"], flat["point"], kf_slot=int(tables["kf_slot"][k]))
    out = []
    for trk in (x, y):
        out.append((trk.track(cs["cur_pyr"][0]), trk.download_map()))
        trk.destroy()
    return n, flat, out[0], out[1]


@pytest.fixture(scope="module")
def small_tracked(ctx, cases):
    """{k: X's (result, map)} of the small case, for the group test"""
    return {}


@pytest.mark.parametrize("k", range(5))
def test_last_frame_from_keyframe_equals_the_old_path(ctx, cases, small_tracked, k):
    cs = cases["small"]
    n, flat, X, Y = _x_and_y(ctx, cs, k, compacted=False)
    model = rl.last_frame_from_keyframe(cs, k)
    assert n == len(model["point"]) == len(flat["point"]) >= 20
    _same(X[0], Y[0], ("small", k))
    mg.assert_tables_equal(X[1], Y[1])
    assert X[0]["result"].sia_n_tracked > 10
    small_tracked[k] = X


@pytest.mark.parametrize("k", range(4))
def test_last_frame_from_keyframe_after_removal_and_compaction(ctx, cases, k):
    cs = cases["small"]
    n, flat, X, Y = _x_and_y(ctx, cs, k, compacted=True)
    assert n == len(rl.last_frame_from_keyframe(_small_compacted(cs), k)["point"]) == len(flat["point"]) >= 20
    _same(X[0], Y[0], ("small after removal and compaction", k))
    mg.assert_tables_equal(X[1], Y[1])


def test_unlinked_points_are_dropped_from_the_last_frame(ctx, cases):
    """the wide case's first frame deletes points: their row entries are still in the tables when the last frame becomes a
    keyframe that holds some of them"""
    cs = cases["wide"]
    max_fts = ms.wide_args()[2]
    x, y = _tile_order(_map_tracker(ctx, cs, max_fts=max_fts)), _tile_order(_map_tracker(ctx, cs, max_fts=max_fts))
    r = x.track(cs["cur_pyr"][0])
    _same(y.track(cs["cur_pyr"][0]), r, "first frame")
    unl = (r["type"] == synth.TYPE_DELETED) & (cs["pt_type"] != synth.TYPE_DELETED)
    tables = x.download_map()
    rows_hit = [k for k in range(cs["n_kf"]) if unl[tables["kf_ftr_point"][tables["kf_ftr_offset"][k]:tables["kf_ftr_offset"][k + 1]]].any()]
    assert unl.sum() >= 10 and rows_hit
    k = rows_hit[0]
    model = rl.last_frame_from_keyframe(tables, k, unl)
    row = tables["kf_ftr_offset"][k + 1] - tables["kf_ftr_offset"][k]
    assert x.last_frame_from_keyframe(k) == len(model["point"]) < row
    y.set_last_frame(model["T_f_w"], model["px"], model["f"], model["point"], kf_slot=int(tables["kf_slot"][k]))
    _same(x.track(cs["cur_pyr"][0]), y.track(cs["cur_pyr"][0]), "second frame, from the keyframe")
    mg.assert_tables_equal(x.download_map(), y.download_map())
    x.destroy()
    y.destroy()


def test_last_frame_from_keyframe_refusals(ctx, cases):
    cs = cases["small"]
    rows = np.diff(cs["kf_ftr_offset"])
    cfg = dict(max_fts=20, max_frame_features=int(rows.max()) - 1)
    trk, twin = _map_tracker(ctx, cs, **cfg), _map_tracker(ctx, cs, **cfg)
    before = trk.download_map()
    for k in (int(rows.argmax()), -1, cs["n_kf"]):                                 # a row above max_frame_features, two indices out of range
        with pytest.raises(hip.SvoHipError, match=INVALID):
            trk.last_frame_from_keyframe(k)
        mg.assert_tables_equal(trk.download_map(), before)
    # the device's last frame is still the one that was set: the next frame equals an undisturbed tracker's
    r = trk.track(cs["cur_pyr"][0])
    _same(r, twin.track(cs["cur_pyr"][0]), "the frame after the refusals")
    unl = (r["type"] == synth.TYPE_DELETED) & (cs["pt_type"] != synth.TYPE_DELETED)
    small = int(rows.argmin())
    assert trk.last_frame_from_keyframe(small) == len(rl.last_frame_from_keyframe(cs, small, unl)["point"]) <= cfg["max_frame_features"]
    trk.destroy()
    twin.destroy()
    fresh = hip.Tracker(ctx, cs["cam"], max_keyframes=2, max_fts=120, max_frame_features=128)
    with pytest.raises(hip.SvoHipError, match=STATE):
        fresh.last_frame_from_keyframe(0)
    fresh.destroy()


def test_a_group_camera_relocalises_with_the_group(ctx, cases, small_tracked):
    cs = cases["small"]
    if not all(k in small_tracked for k in (1, 3)):
        for k in (1, 3):
            small_tracked[k] = _x_and_y(ctx, cs, k, compacted=False)[2]
    grp = hip.TrackerGroup(ctx, cs["cam"], 2, max_keyframes=cs["n_kf"], grid_size=cs["cell_size"], quality_min_fts=20)
    _tile_order(grp.cameras[0])
    for cam in grp.cameras:
        for k in range(cs["n_kf"]):
            cam.upload_keyframe(k, cs["kf_pyr"][k][0])
        cam.set_map(cs)
        cam.set_last_frame(cs["T_cur_w"], np.zeros((0, 2)), np.zeros((0, 3)), np.zeros(0, np.int32), img=cs["cur_pyr"][0])
    with pytest.raises(hip.SvoHipError, match=STATE):
        grp.cameras[0].relocalize(cs["cur_pyr"][0], cs["T_cur_w"])
    assert grp.cameras[0].closest_keyframe(cs["T_cur_w"]) == grp.cameras[1].closest_keyframe(None)
    for c, k in enumerate((1, 3)):
        assert grp.cameras[c].last_frame_from_keyframe(k) == len(rl.last_frame_from_keyframe(cs, k)["point"])
    grp.track([cs["cur_pyr"][0], cs["cur_pyr"][0]])
    for c, k in enumerate((1, 3)):
        _same(grp.cameras[c].last_result(), small_tracked[k][0], ("camera", c))
        mg.assert_tables_equal(grp.cameras[c].download_map(), small_tracked[k][1])
    grp.destroy()


# ---- 6. relocalisation on the sequence
@pytest.fixture(scope="module")
def seq():
    return tc.make_sequence(n_frames=8, n_map=600)


KF_FRAME = (0, 3)            # the frames the two keyframes of the lead-up are


def _lead(ctx, seq):
    """frames 1-3 from keyframe 0, frame 3 promoted (two keyframes on one upload), frames 4-5.  Returns (tracker, results)."""
    trk = hip.Tracker(ctx, seq["cam"], **CFG)
    _start(trk, seq, tc.sequence_map(seq))
    rs = _frames(trk, seq, (1, 2, 3))
    assert trk.promote_last_frame(1) == (1, 0)
    rs += _frames(trk, seq, (4, 5))
    return trk, rs


def _unlinked(rs):
    return rs[-1]["type"] == synth.TYPE_DELETED          # (every point was uploaded as TYPE_UNKNOWN)


def _img(seq, k):
    return seq["pyrs"][k][0]


@pytest.fixture(scope="module")
def scenario(ctx, seq):
    """the accepted relocalisation of frame 6 (X), and the composition of the older entry points (the model's keyframe, a separate
    solver for the gate, the twin Y that tracks frame 6 from the host flatten)"""
    cam = seq["cam"]
    x, rs = _lead(ctx, seq)
    T5 = rs[-1]["T_f_w"].copy()
    tables = dict(x.download_map(), cam=cam)
    unl = _unlinked(rs)
    want = rl.closest_keyframe(tables, T5)
    kf = want["kf_index"]
    feats = rl.last_frame_from_keyframe(tables, kf, unl)
    # ---- the gate through a solver of its own
    ref, cur = hip.Pyramid(ctx, cam.width, cam.height, 5, 1), hip.Pyramid(ctx, cam.width, cam.height, 5, 1)
    ref.upload_level0_and_build(0, _img(seq, KF_FRAME[kf]))
    cur.upload_level0_and_build(0, _img(seq, 6))
    n = len(feats["point"])
    fp = synth.FramePair(cam, seq["pyrs"][KF_FRAME[kf]], seq["pyrs"][6], feats["px"], feats["f"], tables["pt_pos"][feats["point"]],
                         np.ones(n, np.uint8), feats["T_f_w"], seq["truth"][6], T5)
    sia = hip.SparseImgAlign(ctx, 1, CFG["max_frame_features"])
    sia.set_frames(ref, cur)
    sia.upload_pair(0, fp)
    sia.run(1, sia.params(max_level=4, min_level=2, n_iter=30, eps=1e-6, early_stop=True))
    gate = sia.download(0)
    sia.destroy(); ref.destroy(); cur.destroy()
    # ---- the twin
    y, rs_y = _lead(ctx, seq)
    for a, b in zip(rs, rs_y):
        _same(a, b, "lead-up")
    y.set_last_frame(feats["T_f_w"], feats["px"], feats["f"], feats["point"], kf_slot=int(tables["kf_slot"][kf]))
    ry = y.track(_img(seq, 6))
    map_y = y.download_map()
    y.destroy()
    # ---- the call
    rx = x.relocalize(_img(seq, 6), T5)
    map_x = x.download_map()
    return dict(x=x, rs=rs, T5=T5, tables=tables, unl=unl, want=want, feats=feats, fp=fp, gate=gate, rx=rx, ry=ry, map_x=map_x, map_y=map_y)


def test_relocalize_equals_the_composition(scenario):
    s = scenario
    rel, gate = s["rx"]["reloc"], s["gate"]
    print("keyframe", rel.kf_index, "n_close", rel.n_close, "gate n_tracked", rel.gate_n_tracked, "iters", list(rel.gate_iters),
          "n_features", len(s["feats"]["point"]), "n_matches", s["rx"].get("n_matches"))
    assert (rel.kf_index, rel.n_close) == (s["want"]["kf_index"], s["want"]["n_close"]) and s["want"]["n_close"] == 2
    assert rel.accepted == 1 and rel.gate_n_tracked == gate.n_tracked > 30 and rel.gate_stop == gate.stop
    assert list(rel.gate_iters) == list(gate.iters) and sum(rel.gate_iters) >= 3
    assert bytes(rel.T_f_w_gate) == bytes(gate.T_cur_w)
    assert bytes(rel.T_f_w_gate) != s["rx"]["T_f_w_sia"].tobytes()                  # the chain aligned again, from the keyframe's pose
    _same(s["rx"], s["ry"], "the relocalised frame")
    mg.assert_tables_equal(s["map_x"], s["map_y"])
    assert s["rx"]["n_matches"] >= 50


def test_relocalize_against_the_oracle(scenario, seq):
    from oracle import orc
    s = scenario
    kf = s["want"]["kf_index"]
    o = orc.sparse_img_align(s["fp"], max_level=4, min_level=2, n_iter=30, early_stop=True)
    rot, trans = synth.pose_error(np.array(s["rx"]["reloc"].T_f_w_gate), np.array(o.T_cur_w))
    print("gate vs oracle: %.3e rad %.3e m, tracked %d / %d" % (rot, trans, s["rx"]["reloc"].gate_n_tracked, o.n_tracked))
    assert rot < 1e-4 and trans < 1e-3 and s["rx"]["reloc"].gate_n_tracked == o.n_tracked
    t = s["tables"]
    mp = dict(t, cell_size=tc.CELL, kf_pyr=[seq["pyrs"][f] for f in KF_FRAME])
    state = {"pt_type": t["pt_type"].copy(), "pt_n_failed": t["pt_n_failed"].copy(), "pt_n_succeeded": t["pt_n_succeeded"].copy(),
             "unlinked": s["unl"].astype(np.uint8)}
    f = s["feats"]
    ro = tc.oracle_track_frame(orc, mp, state, dict(T=f["T_f_w"], px=f["px"], f=f["f"], point=f["point"]), seq["pyrs"][KF_FRAME[kf]],
                               seq["pyrs"][6], 2)
    for name in ("T_f_w_sia", "T_f_w"):
        rot, trans = synth.pose_error(s["rx"][name], ro[name])
        print("%s vs oracle: %.3e rad %.3e m" % (name, rot, trans))
        assert rot < 1e-4 and trans < 1e-3, name
    assert int(s["rx"]["n_matches"]) == int(ro["n_matches"]) and s["rx"]["result"].sia_n_tracked == ro["sia_n_tracked"]


def test_the_relocalised_frame_is_a_tracked_one(scenario, seq):
    x = scenario["x"]
    assert x.promote_last_frame(2)[0] == 2
    r7 = x.track(_img(seq, 7))
    assert r7["n_matches"] >= 50 and 2 in list(r7["overlap_kf"])
    x.destroy()


# ---- 7. the gate's boundary and the refused state
def _same_reloc(a, b, what):
    assert _reloc_fields(a) == _reloc_fields(b), what
    assert ("result" in a) == ("result" in b), what
    if "result" in a:
        _same(a, b, what)


def test_the_gate_boundary_and_the_refused_state(ctx, seq, scenario):
    s = scenario
    G = int(s["rx"]["reloc"].gate_n_tracked)
    # ---- min_tracked = G is refused
    a, _ = _lead(ctx, seq)
    before, sizes = a.download_map(), a.map_sizes()
    ra = a.relocalize(_img(seq, 6), s["T5"], min_tracked=G)
    assert ra["reloc"].accepted == 0 and "result" not in ra
    gate_of = lambda r: {k: v for k, v in _reloc_fields(r).items() if k != "accepted"}
    assert gate_of(ra) == gate_of(s["rx"])
    mg.assert_tables_equal(a.download_map(), before)                               # tables and point counters
    assert a.map_sizes() == sizes
    with pytest.raises(hip.SvoHipError, match=STATE):
        a.promote_last_frame(2)                                                    # the last frame has no features to promote
    # ---- the refused state: the new image, no features, the gate's pose
    T_gate = np.array(ra["reloc"].T_f_w_gate)
    assert a.closest_keyframe(None) == a.closest_keyframe(T_gate)
    ra7 = a.relocalize(_img(seq, 7), None)
    b, _ = _lead(ctx, seq)
    rb7 = b.relocalize(_img(seq, 7), T_gate)
    assert ra7["reloc"].accepted == 1
    _same_reloc(ra7, rb7, "frame 7 after the refusal")
    mg.assert_tables_equal(a.download_map(), b.download_map())
    a.destroy()
    b.destroy()
    # ---- min_tracked = G - 1 is accepted
    c, _ = _lead(ctx, seq)
    rc = c.relocalize(_img(seq, 6), s["T5"], min_tracked=G - 1)
    assert rc["reloc"].accepted == 1
    assert gate_of(rc) == gate_of(s["rx"])
    _same(rc, s["rx"], "accepted at G - 1")
    # ---- the keyframe named by the caller
    d, _ = _lead(ctx, seq)
    rd = d.relocalize(_img(seq, 6), s["T5"], kf_index=s["want"]["kf_index"])
    assert rd["reloc"].n_close == 0
    _same(rd, s["rx"], "the keyframe given")
    other = 1 - s["want"]["kf_index"]
    assert c.relocalize(_img(seq, 7), None, exclude_kf=s["want"]["kf_index"], min_tracked=10 ** 6)["reloc"].kf_index == other
    c.destroy()
    d.destroy()


def test_a_keyframe_without_living_features_is_refused(ctx, seq):
    """after the lead-up every point has its observation in keyframe 0 and at most one in keyframe 1: removing keyframe 0 deletes
    every point of its row (Map::safeDeleteFrame: at most two observations), which is every point"""
    trk, rs = _lead(ctx, seq)
    got = trk.remove_keyframe(0)
    sizes = trk.map_sizes()
    assert got["n_deleted_points"] == len(seq["px0"]) - int(_unlinked(rs).sum()) and sizes["n_kf"] == 1 and sizes["n_ftr"] == 0
    before = trk.download_map()
    r = trk.relocalize(_img(seq, 6), rs[-1]["T_f_w"], kf_index=0, min_tracked=0)
    rel = r["reloc"]
    assert (rel.kf_index, rel.accepted, rel.gate_n_tracked) == (0, 0, 0) and "result" not in r
    assert bytes(rel.T_f_w_gate) == rs[-1]["T_f_w"].tobytes()                       # run() returns 0 and leaves the pose alone
    mg.assert_tables_equal(trk.download_map(), before)
    assert trk.map_sizes() == sizes
    # its key points went with the points: it is not close from anywhere
    assert trk.closest_keyframe(rs[-1]["T_f_w"]) == dict(kf_index=-1, n_close=0, distance=0.0)
    trk.destroy()


def test_no_close_keyframe_changes_nothing(ctx, seq, scenario):
    s = scenario
    away = synth.se3_mul(synth.se3_from_twist([0.0, 0.0, 0.0], [0.0, np.pi, 0.0]), s["T5"])
    assert rl.closest_keyframe(s["tables"], away)["kf_index"] == -1
    trk, rs = _lead(ctx, seq)
    before, last = trk.download_map(), trk.last_result()
    r = trk.relocalize(_img(seq, 7), away)
    assert (r["reloc"].kf_index, r["reloc"].n_close, r["reloc"].accepted) == (-1, 0, 0) and "result" not in r
    mg.assert_tables_equal(trk.download_map(), before)
    _same(trk.last_result(), last, "the last tracked frame")
    # the device's last frame is kept: frame 6 tracks as on a tracker that never made the call
    twin, _ = _lead(ctx, seq)
    _same(trk.track(_img(seq, 6)), twin.track(_img(seq, 6)), "frame 6 after the call that found nothing")
    trk.destroy()
    twin.destroy()


def test_relocalize_refusals(ctx, seq):
    trk, rs = _lead(ctx, seq)
    before, last = trk.download_map(), trk.last_result()
    T5 = rs[-1]["T_f_w"]
    with pytest.raises(hip.SvoHipError, match=INVALID):
        trk.relocalize(_img(seq, 6), T5, kf_index=2)
    with pytest.raises(hip.SvoHipError, match=INVALID):
        trk.relocalize(_img(seq, 6), T5, min_tracked=-1)
    mg.assert_tables_equal(trk.download_map(), before)
    twin, _ = _lead(ctx, seq)
    _same(trk.track(_img(seq, 6)), twin.track(_img(seq, 6)), "frame 6 after the refusals")
    trk.destroy()
    twin.destroy()
    fresh = hip.Tracker(ctx, seq["cam"], **CFG)
    with pytest.raises(hip.SvoHipError, match=STATE):
        fresh.relocalize(_img(seq, 6), T5)
    fresh.upload_keyframe(0, _img(seq, 0))
    fresh.set_map(tc.sequence_map(seq))
    with pytest.raises(hip.SvoHipError, match=STATE):
        fresh.relocalize(_img(seq, 6), None)                                       # no pose given, no last frame
    r = fresh.relocalize(_img(seq, 1), seq["T0"])                                  # a tracker whose first frame is a relocalisation
    assert r["reloc"].accepted == 1 and r["reloc"].kf_index == 0 and r["n_matches"] >= 50
    fresh.destroy()


# ---- 8. the host twin
def test_host_twin_relocalises(tmp_path, ctx, seq):
    """svo::relocalizeFrame of android_svo_amd/host/svo_host.h through hip_bridge::FrameTrackerT::relocalize with the switch on, on
    the scenario above: frames 1-3, frame 3 becomes a keyframe in place, frames 4-5, frame 6 is relocalised (the device chooses
    the keyframe), frame 7 is tracked from it.  Poses, features and the gate equal the Python-driven run bit for bit, and the map
    is uploaded once."""
    import os
    import subprocess
    from test_gpu_host_cpp import DEMO, _write_track_case
    assert os.path.exists(DEMO), "build() must have produced android_svo_amd/host/svo_host_demo"
    case, out = tmp_path / "case", tmp_path / "out"
    case.mkdir(); out.mkdir()
    mp = tc.sequence_map(seq)
    n = len(seq["px0"])
    cs = dict(mp, obs_point=np.arange(n, dtype=np.int32), kf_ftr_obs=np.arange(n, dtype=np.int32), cand_obs=np.zeros(0, np.int32))
    cfg = dict(grid_size=tc.CELL, max_fts=tc.MAX_FTS, quality_min_fts=40, klt_min_level=2, max_frame_features=1024, keyframe_at=2)
    _write_track_case(case, cs, [_img(seq, k) for k in range(1, 8)], cfg, last_kf=0)
    p = subprocess.run([DEMO, str(case), str(out), "track", "incremental", "reloc_at", "5"], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert p.returncode == 0, p.stdout + p.stderr
    rd = lambda name, dt: np.fromfile(out / name, dtype=dt)
    trk, rs = _lead(ctx, seq)
    r6 = trk.relocalize(_img(seq, 6), rs[-1]["T_f_w"])
    rs = rs + [r6, trk.track(_img(seq, 7))]
    trk.destroy()
    rel = rd("track_reloc.bin", np.float64)
    want = r6["reloc"]
    print("host twin:", rel[:6].tolist())
    assert rel[:6].tolist() == [0.0, float(want.kf_index), 1.0, float(want.gate_n_tracked), 1.0, float(want.n_close)]   # RESULT_NO_KEYFRAME
    assert rel[6:].tobytes() == bytes(want.T_f_w_gate)
    poses, stats = rd("track_poses.bin", np.float64).reshape(-1, 7), rd("track_stats.bin", np.float64).reshape(-1, 9)
    assert len(poses) == 7
    for k, r in enumerate(rs):
        assert poses[k].tobytes() == r["T_f_w"].tobytes(), ("frame", k + 1)
        assert stats[k, 0] == len(r["feat_px"]) and stats[k, 1] == r["n_matches"] and stats[k, 3] == int(r["result"].sia_n_tracked), ("frame", k + 1)
        assert rd("track_feat_%d_px.bin" % k, np.float64).tobytes() == r["feat_px"].tobytes(), ("frame", k + 1)
        assert rd("track_feat_%d_point.bin" % k, np.int32).tolist() == r["feat_point"].tolist(), ("frame", k + 1)
    assert rd("track_uploads.bin", np.float64).tolist() == [1.0] * 7                 # the map went up once
