"""The device map grows in place: svo_hip_tracker_add_candidates (converged seeds become point candidates at the tails of the
tables) and svo_hip_tracker_promote_last_frame (the tracked frame becomes a keyframe from what the device holds of it), against
the numpy model of tests/map_growth_reference.py and against a tracker that gets the model's tables through svo_hip_tracker_set_map
under the same point numbering.  Every comparison is exact: integers equal, doubles byte-equal.

In the scenario tests tracker X uses the new calls and tracker Y today's path (set_map of the model's tables, which keeps the
last frame for a map with the same numbering)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import map_growth_reference as mg
import map_growth_scenario as sc
import tracking_chain as tc
from test_oracle_reproject_map import CASES, GOLD
from android_svo_amd import hip, synth

pytestmark = pytest.mark.gpu

CFG = dict(max_keyframes=4, grid_size=tc.CELL, max_fts=tc.MAX_FTS, klt_min_level=2, max_frame_features=1024)
KEYS = ("T_f_w", "T_f_w_sia", "feat_px", "feat_f", "feat_level", "feat_point", "feat_type", "feat_grad", "type", "n_failed", "n_succeeded")
COUNTERS = (("pt_type", "type"), ("pt_n_failed", "n_failed"), ("pt_n_succeeded", "n_succeeded"))


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


_scenario = functools.lru_cache(maxsize=None)(sc.make)                          # (also read when the module is collected: PAD_TARGETS)


@pytest.fixture(scope="module")
def scen():
    return _scenario()


def _fields(st, prefix=""):
    """a ctypes record as {field: the bytes of its value} (nested records flattened, explicit padding fields left out)"""
    out = {}
    for name, tp in st._fields_:
        v = getattr(st, name)
        if name.startswith("pad"):
            continue
        if hasattr(v, "_fields_"):
            out.update(_fields(v, prefix + name + "."))
        else:
            out[prefix + name] = bytes(v) if hasattr(v, "__len__") else bytes(tp(v))
    return out


def _same(a, b, what):
    """every field of the track result and every feature array"""
    for k in KEYS:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)
    fa, fb = _fields(a["result"]), _fields(b["result"])
    assert fa == fb, (what, [k for k in fa if fa[k] != fb[k]])
    assert list(a["overlap_kf"]) == list(b["overlap_kf"]) and list(a["overlap_count"]) == list(b["overlap_count"]), what


def _start(trk, seq, mp):
    n = len(seq["px0"])
    trk.upload_keyframe(0, seq["pyrs"][0][0])
    trk.set_map(mp)
    trk.set_last_frame(seq["T0"], seq["px0"], seq["f0"], np.arange(n, dtype=np.int32), kf_slot=0)


def _frames(trk, seq, frames):
    return [trk.track(seq["pyrs"][k][0]) for k in frames]


def _with_counters(tables, r):
    """the tables with the point counters of track result r (for the points it covers)"""
    t = mg.normalised(tables)
    for name, key in COUNTERS:
        t[name][:len(r[key])] = r[key]
    return t


F_HEAD, F_MID, F_TAIL = range(1, sc.APPEND_AFTER + 1), range(sc.APPEND_AFTER + 1, sc.PROMOTE_AT + 1), range(sc.PROMOTE_AT + 1, sc.N_FRAMES)


def _run_x(trk, s, track=None, last=None):
    """the scenario through the new calls.  track(frames) -> results (default: the lone tracker's own call)"""
    seq = s["seq"]
    track = track or (lambda frames: _frames(trk, seq, frames))
    out = dict(head=track(F_HEAD))
    out["first"] = trk.add_candidates(**s["cand"])
    out["last_after_add"] = trk.last_result()
    out["map_after_add"] = trk.download_map()
    out["mid"] = track(F_MID)
    out["promote"] = trk.promote_last_frame(1)
    out["map_after_promote"] = trk.download_map()
    out["sizes"] = trk.map_sizes()
    out["tail"] = track(F_TAIL)
    return out


@pytest.fixture(scope="module")
def grown(ctx, scen):
    """X and Y through the whole scenario, once: frames 1-2, the candidates, frames 3-5, the promotion, frames 6-8"""
    seq, base, mp = scen["seq"], scen["base"], scen["base_map"]
    x = hip.Tracker(ctx, seq["cam"], **CFG)
    _start(x, base, mp)
    X = _run_x(x, scen)
    x.destroy()
    y = hip.Tracker(ctx, seq["cam"], **CFG)
    _start(y, base, mp)
    Y = dict(head=_frames(y, seq, F_HEAD))
    model_add, first = mg.append_candidates(mp, **scen["cand"])
    Y["model_add"] = _with_counters(model_add, Y["head"][-1])           # types and counters from the last result, the new points 1 / 0 / 0
    Y["first"] = first
    y.set_map(Y["model_add"])
    Y["mid"] = _frames(y, seq, F_MID)
    Y["model_promote"], Y["n_promoted"] = mg.promote(model_add, Y["mid"][-1], 1, seq["cam"])
    y.keyframe_from_last_frame(1)
    y.set_map(Y["model_promote"])
    Y["tail"] = _frames(y, seq, F_TAIL)
    y.destroy()
    return X, Y


def test_append_candidates(grown, scen):
    X, Y = grown
    n_new = len(scen["cand"]["kf_index"])
    assert X["first"] == Y["first"] == scen["base_map"]["n_points"] and n_new >= 100
    for i, (a, b) in enumerate(zip(X["head"] + X["mid"], Y["head"] + Y["mid"])):
        _same(a, b, ("frame", i + 1))
    mg.assert_tables_equal(X["map_after_add"], Y["model_add"])
    assert any((r["feat_point"] >= X["first"]).any() for r in X["mid"])         # a later feature refers to an appended point
    assert len(X["mid"][-1]["type"]) == X["first"] + n_new


def test_promote_without_candidates(ctx):
    """tests/test_gpu_tracker.py::test_last_frame_becomes_a_keyframe's scenario: X promotes on the device, Y keeps the pyramid
    and uploads tracking_chain's grown map"""
    seq = tc.make_sequence(n_frames=sc.N_FRAMES)
    mp = tc.sequence_map(seq)
    got = []
    for promote in (True, False):
        trk = hip.Tracker(ctx, seq["cam"], **CFG)
        _start(trk, seq, mp)
        rs = _frames(trk, seq, range(1, sc.PROMOTE_AT + 1))
        mp2 = tc.map_with_tracked_frame_as_keyframe(seq, mp, rs[-1])
        if promote:
            assert trk.promote_last_frame(1) == (1, 0)
        else:
            trk.keyframe_from_last_frame(1)
            trk.set_map(mp2)
        dl = trk.download_map()
        mg.assert_tables_equal(dl, mp2)
        rs += _frames(trk, seq, F_TAIL)
        got.append(rs)
        trk.destroy()
    for i, (a, b) in enumerate(zip(*got)):
        _same(a, b, ("frame", i + 1))
    assert any(1 in list(r["overlap_kf"]) for r in got[0][sc.PROMOTE_AT:])      # the new keyframe took part in the reprojection


def test_promote_with_candidates(grown, scen):
    X, Y = grown
    kf_index, n_promoted = X["promote"]
    n_new = len(scen["cand"]["kf_index"])
    assert kf_index == 1 and n_promoted == Y["n_promoted"] >= 5 and n_new - n_promoted >= 5
    dl, model = X["map_after_promote"], Y["model_promote"]
    mg.assert_tables_equal(dl, model)
    # (what that equality covers, spelled out on the download)
    fp = X["mid"][-1]["feat_point"]
    promoted = [int(p) for p in Y["model_add"]["cand_point"] if p in set(fp[fp >= 0].tolist())]
    assert len(promoted) == n_promoted
    assert (dl["pt_type"][promoted] == synth.TYPE_UNKNOWN).all() and not dl["pt_n_failed"][promoted].any()
    assert len(dl["cand_point"]) == n_new - n_promoted and not set(promoted) & set(dl["cand_point"].tolist())
    n_base = scen["base_map"]["n_points"]
    np.testing.assert_array_equal(dl["kf_ftr_point"][:dl["kf_ftr_offset"][1]], np.concatenate([np.arange(n_base), promoted]))
    assert (dl["obs_kf"][dl["pt_obs_offset"][fp[fp >= 0]]] == 1).all()         # newest observation first
    assert X["sizes"] == dict(n_kf=2, n_ftr=len(model["kf_ftr_point"]), n_points=n_base + n_new, n_obs=len(model["obs_kf"]),
                              n_candidates=n_new - n_promoted)
    for i, (a, b) in enumerate(zip(X["tail"], Y["tail"])):
        _same(a, b, ("frame", sc.PROMOTE_AT + 1 + i))
    assert any(1 in list(r["overlap_kf"]) for r in X["tail"])


def _padding(seq, n):
    """n candidates without an observation (kf_index -1) that no frame of the sequence sees: in the first keyframe's frame they
    sit at (100, 0, 1) -- dozens of focal lengths right of the image in every frame of the sequence (x / z from 100 to 34).  (A
    place BEHIND the camera would not do: the reprojector, like the reference's, projects without a depth test, and a point on
    the optical axis behind the camera lands in the middle of the image.)"""
    pos = synth.se3_act(synth.se3_inv(seq["T0"]), np.array([100.0, 0.0, 1.0]))
    return dict(pos=np.tile(pos, (n, 1)), kf_index=np.full(n, -1, np.int32), px=np.zeros((n, 2)), f=np.tile([0.0, 0.0, 1.0], (n, 1)),
                level=np.zeros(n, np.int32))


def _scenario_points(s):
    return s["base_map"]["n_points"] + len(s["cand"]["kf_index"])


# point-table sizes on both sides of trk_promote_kernel's block of 1024 threads (its loops over the points and the candidates take
# one round in the scenario's own map); a size the scenario's own points already exceed cannot be padded to
PAD_TARGETS = [n for n in (1023, 1024, 1025, 2049) if n > _scenario_points(_scenario())]


def test_padded_targets_beyond_one_block():
    assert 1025 in PAD_TARGETS and 2049 in PAD_TARGETS


@pytest.mark.parametrize("target", PAD_TARGETS)
def test_promote_beyond_one_block(ctx, scen, grown, target):
    """the scenario with the point table padded to `target` rows before the frames that precede the promotion: the padding changes
    no tracked frame, the promotion gives the model's tables, and the next frame is the one a tracker with the model's tables
    uploaded gives"""
    seq, base, mp, cand = scen["seq"], scen["base"], scen["base_map"], scen["cand"]
    X0, Y0 = grown                                                              # (the unpadded scenario)
    n_real, n_new = _scenario_points(scen), len(cand["kf_index"])
    pad = _padding(seq, target - n_real)
    cfg = dict(CFG, max_points=target, max_candidates=n_new + target - n_real, max_obs=2 * target)
    after = sc.PROMOTE_AT + 1

    def unpadded(r):
        """r with its point counters cut to the scenario's own points; the padding's: untouched candidates that failed to
        project three times (Reprojector::reprojectMap adds 3 for a candidate outside the frame)"""
        assert len(r["type"]) == target and (r["type"][n_real:] == synth.TYPE_CANDIDATE).all() and not r["n_succeeded"][n_real:].any()
        return dict(r, **{k: r[k][:n_real] for k in ("type", "n_failed", "n_succeeded")})
    x = hip.Tracker(ctx, seq["cam"], **cfg)
    _start(x, base, mp)
    _frames(x, seq, F_HEAD)
    assert x.add_candidates(**cand) == X0["first"]
    assert x.add_candidates(**pad) == n_real
    mid = _frames(x, seq, F_MID)
    for i, (a, b) in enumerate(zip(mid, X0["mid"])):
        _same(unpadded(a), b, ("padded frame", sc.APPEND_AFTER + 1 + i))
    assert (mid[-1]["n_failed"][n_real:] == 3 * len(F_MID)).all()
    model_add, first = mg.append_candidates(mg.append_candidates(mp, **cand)[0], **pad)
    model, n_promoted = mg.promote(model_add, mid[-1], 1, seq["cam"])
    assert first == n_real and model["n_points"] == target
    assert x.promote_last_frame(1) == (1, n_promoted) and n_promoted == Y0["n_promoted"]
    mg.assert_tables_equal(x.download_map(), model)
    assert x.map_sizes() == dict(n_kf=2, n_ftr=len(model["kf_ftr_point"]), n_points=target, n_obs=len(model["obs_kf"]),
                                 n_candidates=len(model["cand_point"]))
    assert len(model["cand_point"]) == n_new - n_promoted + target - n_real
    nxt = x.track(seq["pyrs"][after][0])
    x.destroy()
    y = hip.Tracker(ctx, seq["cam"], **cfg)
    _start(y, base, mp)
    head = _frames(y, seq, F_HEAD)
    y.set_map(_with_counters(model_add, head[-1]))
    _same(_frames(y, seq, F_MID)[-1], mid[-1], "set_map twin before the promotion")
    y.keyframe_from_last_frame(1)
    y.set_map(model)
    _same(nxt, y.track(seq["pyrs"][after][0]), ("frame", after))
    y.destroy()


def test_last_result_after_add_candidates(grown, scen):
    """svo_hip_tracker_last_result returns the tracked frame's counters for the points the frame had, whatever the map gained since"""
    X, _ = grown
    _same(X["last_after_add"], X["head"][-1], "last_result")
    assert len(X["last_after_add"]["type"]) == scen["base_map"]["n_points"]


def _wide_tracker(ctx, cs, key, **cfg):
    trk = hip.Tracker(ctx, cs["cam"], max_keyframes=cs["n_kf"], grid_size=cs["cell_size"], quality_min_fts=20, **cfg)
    for k in range(cs["n_kf"]):
        trk.upload_keyframe(k, cs["kf_pyr"][k][0])
    trk.set_map(dict(cs, kf_slot=np.arange(cs["n_kf"], dtype=np.int32), kf_key_point=key))
    trk.set_last_frame(cs["T_cur_w"], np.zeros((0, 2)), np.zeros((0, 3)), np.zeros(0, np.int32), img=cs["cur_pyr"][0])
    return trk


def test_append_after_deletions(ctx):
    """the "wide" map case: its first frame deletes points (map_changed, a re-selection of key points is owed); candidates
    appended then leave every pre-existing table range as it was, and the owed re-selection is what it would have been"""
    tag, kw, max_fts = [c for c in CASES if c[0] == "wide"][0]
    cs = synth.make_map_case(**kw)
    key = np.load(GOLD)[tag + "_kf_key_point"]
    # new candidates: copies of the first 20 of the list (their seed features, their positions a millimetre off)
    src = cs["cand_point"][:20]
    so = cs["pt_obs_offset"][src]
    new = dict(pos=cs["pt_pos"][src] + 1e-3, kf_index=cs["obs_kf"][so], px=cs["obs_px"][so], f=cs["obs_f"][so], level=cs["obs_level"][so],
               edgelet=cs["obs_edgelet"][so], grad=cs["obs_grad"][so])

    def tracked(append):
        trk = _wide_tracker(ctx, cs, key, max_fts=max_fts)
        assert trk.track(cs["cur_pyr"][0])["map_changed"] == 1
        if append:
            assert trk.add_candidates(**new) == cs["n_points"]
        return trk
    # ---- the tables before and after the append
    maps = []
    for append in (False, True):
        trk = tracked(append)
        maps.append(trk.download_map())
        trk.destroy()
    before, after = maps
    for k in mg.TABLES:
        n = len(before[k])
        assert after[k][:n].tobytes() == before[k].tobytes(), k
    assert (before["pt_type"] == synth.TYPE_DELETED).sum() > (cs["pt_type"] == synth.TYPE_DELETED).sum()
    assert after["n_points"] == before["n_points"] + 20 and len(after["cand_point"]) == len(before["cand_point"]) + 20
    assert after["obs_edgelet"][len(before["obs_kf"]):].tobytes() == np.asarray(new["edgelet"], np.uint8).tobytes()
    # ---- the re-selection the deletions owe runs in front of the next frame: the append in between does not disturb it.  The next
    # frame: the same scene a small step further (the same image twice would make the alignment's update exactly zero, for which
    # SE3::exp returns a NaN translation -- in the reference too)
    scene = synth.PlaneScene(seed=kw.get("seed", 31), depth=2.0, tilt=(0.08, -0.05))
    img2 = scene.render(cs["cam"], synth.se3_mul(synth.se3_from_twist([0.012, -0.006, 0.004], [0.002, -0.003, 0.001]), cs["T_cur_w"]))
    keys, nxt = [], []
    for append in (False, True):
        trk = tracked(append)
        nxt.append(trk.track(img2))
        keys.append(trk.download_key_points(cs["n_kf"]))
        trk.destroy()
    np.testing.assert_array_equal(keys[0], keys[1])
    assert (keys[0] != key).any()                                                # (the deletions did cost a key feature)
    assert nxt[1]["n_matches"] >= nxt[0]["n_matches"] > 20


REFUSALS = ("add_points", "add_obs", "add_candidates", "add_kf_index", "add_level", "promote_keyframes", "promote_obs", "promote_kf_features",
            "promote_slot_taken", "promote_slot_range", "promote_set_last_frame")


@pytest.fixture(scope="module")
def untouched(ctx, scen):
    """the base map's tracker through frames 1-3, nothing in between"""
    seq = scen["seq"]
    trk = hip.Tracker(ctx, seq["cam"], **CFG)
    _start(trk, scen["base"], scen["base_map"])
    rs = _frames(trk, seq, range(1, sc.APPEND_AFTER + 2))
    sizes = trk.map_sizes()
    trk.destroy()
    return rs, sizes


@pytest.mark.parametrize("case", REFUSALS)
def test_refusals_change_nothing(ctx, scen, untouched, case):
    """one over each capacity, an index out of range, a last frame that was not tracked, an occupied slot: the call is refused,
    the tables are as they were and the next frame is an untouched tracker's"""
    seq, cand = scen["seq"], scen["cand"]
    rs, z = untouched
    n_new = len(cand["kf_index"])
    m = int((rs[sc.APPEND_AFTER - 1]["feat_point"] >= 0).sum())                  # the features with a point of the frame to promote
    assert z["n_candidates"] == 0 and m > 20
    cfg = dict(CFG)
    code, call = -1, None
    add = lambda **kw: (lambda t: t.add_candidates(**dict(cand, **kw)))
    if case == "add_points":
        cfg["max_points"], call = z["n_points"] + n_new - 1, add()
    elif case == "add_obs":
        cfg["max_obs"], call = z["n_obs"] + n_new - 1, add()
    elif case == "add_candidates":
        cfg["max_candidates"], call = n_new - 1, add()
    elif case == "add_kf_index":
        kf = cand["kf_index"].copy()
        kf[-1] = z["n_kf"]
        call = add(kf_index=kf)
    elif case == "add_level":
        lv = cand["level"].copy()
        lv[n_new // 2] = 5                                                       # n_levels
        call = add(level=lv)
    elif case == "promote_keyframes":
        cfg["max_keyframes"], call = 1, (lambda t: t.promote_last_frame(0))       # (slot 0 is also taken; slot 1 would be out of range)
    elif case == "promote_obs":
        cfg["max_obs"], call = z["n_obs"] + m - 1, (lambda t: t.promote_last_frame(1))
    elif case == "promote_kf_features":
        cfg["max_kf_features"], call = z["n_ftr"] + m - 1, (lambda t: t.promote_last_frame(1))      # no candidates: no seed entries to allow for
    elif case == "promote_slot_taken":
        call = lambda t: t.promote_last_frame(0)
    elif case == "promote_slot_range":
        call = lambda t: t.promote_last_frame(CFG["max_keyframes"])
    elif case == "promote_set_last_frame":
        code = -4

        def call(t):
            r = rs[sc.APPEND_AFTER - 1]
            t.set_last_frame(r["T_f_w"], r["feat_px"], r["feat_f"], r["feat_point"], img=seq["pyrs"][sc.APPEND_AFTER][0])
            t.promote_last_frame(1)
    trk = hip.Tracker(ctx, seq["cam"], **cfg)
    _start(trk, scen["base"], scen["base_map"])
    head = _frames(trk, seq, F_HEAD)
    _same(head[-1], rs[sc.APPEND_AFTER - 1], case)
    before = trk.download_map()
    with pytest.raises(hip.SvoHipError, match=r"\(%d\)" % code):
        call(trk)
    assert trk.map_sizes() == z
    mg.assert_tables_equal(trk.download_map(), before)
    _same(trk.track(seq["pyrs"][sc.APPEND_AFTER + 1][0]), rs[sc.APPEND_AFTER], case)
    trk.destroy()


def test_exact_capacities_are_accepted(ctx, scen, untouched, grown):
    """the other side of the capacity tests above: with exactly the room the calls ask for, both go through and give the same map"""
    seq, cand = scen["seq"], scen["cand"]
    _, z = untouched
    X, _ = grown
    n_new = len(cand["kf_index"])
    m = int((X["mid"][-1]["feat_point"] >= 0).sum())
    trk = hip.Tracker(ctx, seq["cam"], **dict(CFG, max_points=z["n_points"] + n_new, max_candidates=n_new, max_keyframes=2,
                                              max_obs=z["n_obs"] + n_new + m, max_kf_features=z["n_ftr"] + m + min(m, n_new)))
    _start(trk, scen["base"], scen["base_map"])
    _frames(trk, seq, F_HEAD)
    assert trk.add_candidates(**cand) == z["n_points"]
    _frames(trk, seq, F_MID)
    assert trk.promote_last_frame(1) == X["promote"]
    mg.assert_tables_equal(trk.download_map(), X["map_after_promote"])
    trk.destroy()


def test_group_camera_grows_its_map(ctx, scen):
    """camera 0 of a group gets the candidates and the promotion, camera 1 nothing: each equals its lone tracker under the same
    calls (the sums of SparseImgAlign grouped by tile on both sides, so that nothing depends on the company)"""
    seq, full_map = scen["seq"], tc.sequence_map(scen["seq"])
    tile = (hip.SIA_OPT_REDUCTION, hip.SIA_REDUCTION_TILE_ORDER)
    cfg = dict(CFG, max_items=1024)
    lone0 = hip.Tracker(ctx, seq["cam"], **cfg)
    lone0.set_sia_option(*tile)
    _start(lone0, scen["base"], scen["base_map"])
    want0 = _run_x(lone0, scen)
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
    got0 = _run_x(grp.cameras[0], scen, track=track)
    assert got0["first"] == want0["first"] and got0["promote"] == want0["promote"] and got0["sizes"] == want0["sizes"]
    for part in ("head", "mid", "tail"):
        for i, (a, b) in enumerate(zip(got0[part], want0[part])):
            _same(a, b, (0, part, i))
    _same(got0["last_after_add"], want0["last_after_add"], "last_after_add")
    mg.assert_tables_equal(got0["map_after_add"], want0["map_after_add"])
    mg.assert_tables_equal(got0["map_after_promote"], want0["map_after_promote"])
    for i, (a, b) in enumerate(zip(got1, want1)):
        _same(a, b, (1, i))
    mg.assert_tables_equal(grp.cameras[1].download_map(), map1)
    assert grp.cameras[1].map_sizes()["n_kf"] == 1
    grp.destroy()


def _demo_pair(tmp_path, cs, frames, cfg, **last):
    """svo_host_demo's track mode over one case, with and without `incremental`; returns the two output directories"""
    from test_gpu_host_cpp import DEMO, _write_track_case
    assert os.path.exists(DEMO)
    case = tmp_path / "case"
    case.mkdir()
    _write_track_case(case, cs, frames, cfg, **last)
    outs = []
    for extra in ([], ["incremental"]):
        out = tmp_path / ("out_" + "_".join(extra or ["default"]))
        out.mkdir()
        p = subprocess.run([DEMO, str(case), str(out), "track"] + extra, capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
        assert p.returncode == 0, p.stdout + p.stderr
        outs.append(out)
    return outs


def _same_track_files(a_dir, b_dir):
    names = sorted(f for f in os.listdir(a_dir) if f.startswith("track_") and f.endswith(".bin"))
    assert len(names) > 10 and names == sorted(f for f in os.listdir(b_dir) if f.startswith("track_") and f.endswith(".bin"))
    for f in names:
        if f != "track_uploads.bin":
            assert (a_dir / f).read_bytes() == (b_dir / f).read_bytes(), f


@pytest.mark.parametrize("which", ["new_candidate", "keyframe"])
def test_host_twin_incremental_equals_default(tmp_path, which):
    """hip_bridge::FrameTrackerT on the C++ twins (svo_host_demo track): with setIncrementalMap the map is uploaded once --
    the candidate the depth filter's thread adds, and the frame that becomes a keyframe, reach the device in place -- and every
    file the demo writes about the tracked frames is byte for byte what the default path (a full upload for either) writes."""
    if which == "new_candidate":
        # tests/test_gpu_host_cpp.py::test_cpp_frame_tracker_on_a_map_with_deletions' case: deletions in the first frame, a
        # candidate behind the tracker's back after the second
        tag, kw, max_fts = [c for c in CASES if c[0] == "wide"][0]
        cs = synth.make_map_case(**kw)
        cfg = dict(grid_size=cs["cell_size"], max_fts=max_fts, quality_min_fts=20, klt_min_level=2, max_frame_features=2048,
                   structure_optim_max_pts=20, new_candidate_at=1)
        scene = synth.PlaneScene(seed=kw.get("seed", 31), depth=2.0, tilt=(0.08, -0.05))
        step = synth.se3_from_twist([0.012, -0.006, 0.004], [0.002, -0.003, 0.001])
        T2 = synth.se3_mul(step, cs["T_cur_w"])
        frames = [cs["cur_pyr"][0], scene.render(cs["cam"], T2), scene.render(cs["cam"], synth.se3_mul(step, T2))]
        default, incremental = _demo_pair(tmp_path, cs, frames, cfg, last_kf=-1, last_img=cs["cur_pyr"][0], last_pose=cs["T_cur_w"])
        want_default = [1, 1, 2]
    else:
        # tests/test_gpu_host_cpp.py::test_cpp_frame_tracker_promotes_a_frame_to_keyframe's case
        seq = tc.make_sequence(n_frames=sc.N_FRAMES)
        mp = tc.sequence_map(seq)
        n = len(seq["px0"])
        cs = dict(mp, obs_point=np.arange(n, dtype=np.int32), kf_ftr_obs=np.arange(n, dtype=np.int32), cand_obs=np.zeros(0, np.int32))
        cfg = dict(grid_size=tc.CELL, max_fts=tc.MAX_FTS, quality_min_fts=40, klt_min_level=2, max_frame_features=1024, keyframe_at=4)
        default, incremental = _demo_pair(tmp_path, cs, [seq["pyrs"][k][0] for k in range(1, sc.N_FRAMES)], cfg, last_kf=0)
        want_default = [1, 1, 1, 1, 1, 2, 2, 2]
    _same_track_files(default, incremental)
    np.testing.assert_array_equal(np.fromfile(default / "track_uploads.bin"), want_default)
    up = np.fromfile(incremental / "track_uploads.bin")
    assert len(up) == len(want_default) and (up == 1).all()
