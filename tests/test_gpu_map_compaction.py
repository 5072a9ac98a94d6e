"""The points of the device map are renumbered in place: svo_hip_tracker_compact_points against the numpy model of
tests/map_compaction_reference.py (tests/test_map_compaction_model.py establishes the model's own properties on the CPU) and
against trackers that make the same calls without it.  Every comparison is exact: integers equal, doubles byte-equal.

Tracker X compacts, tracker Z does not; a point index of Z is translated with the old_to_new arrays X's compactions returned."""
import os
import subprocess

import numpy as np
import pytest

import map_compaction_reference as mc
import map_growth_reference as mg
import map_removal_reference as mr
import map_removal_scenario as ms
import tracking_chain as tc
from test_gpu_map_growth import KEYS, _fields, _frames, _same, _start
from test_gpu_map_removal import CFG, _map_tracker, _new_candidates, _sizes
from test_gpu_map_removal import cases, ctx, scen, wide_first  # noqa: F401  (fixtures)
from android_svo_amd import hip, synth

pytestmark = pytest.mark.gpu


# ---- 1. the tables at the smallest shapes that can go wrong: one chunk of the in-place walk is 1024 points
CAM = synth.Camera(320, 240, 250.0, 250.0, 159.5, 119.5)
SIZES = (1, 2, 1023, 1024, 1025, 2049, 3073)


def _patterns(P):
    """{name: dead[P]} -- the patterns that exist at this size, each distinct mask once"""
    idx = np.arange(P)
    pats = dict(none=idx < 0, all_but_one=idx != P // 2, first=idx == 0, last=idx == P - 1, every_other=idx % 2 == 0)
    if P > 1025:
        pats["straddle_1024"] = (idx >= 1019) & (idx < 1031)             # one dead run across the first chunk boundary
    if P >= 2049:
        pats["run_of_a_chunk_and_more"] = (idx >= 5) & (idx < 5 + 1030)  # living rows move down by more than a chunk
    out, seen = {}, set()
    for name, d in pats.items():
        if d.tobytes() not in seen:
            seen.add(d.tobytes())
            out[name] = d
    return out


def _two_keyframe_map(P, dead, seed):
    """Two keyframes.  Keyframe 1's row holds exactly the points of `dead`, each with its one observation there: removing keyframe 1
    deletes them (Map::safeDeleteFrame: at most two observations).  The others have one observation in keyframe 0; every fifth of
    them is a point candidate (no row entry), the rest form keyframe 0's row, five of them its key points."""
    rng = np.random.default_rng(seed)
    alive = np.where(~dead)[0]
    is_cand = np.zeros(P, bool)
    is_cand[alive[2::5]] = True
    row0 = alive[~is_cand[alive]]
    row0 = row0[rng.permutation(len(row0))].astype(np.int32)             # (row order is not point order)
    row1 = np.where(dead)[0][::-1].astype(np.int32)
    key = np.full((2, 5), -1, np.int32)
    key[0, :min(5, len(row0))] = row0[:5]
    key[1, :min(3, len(row1))] = row1[:3]
    px = np.stack([rng.uniform(0, 320, P), rng.uniform(0, 240, P)], axis=1)
    T = np.array([[0, 0, 0, 0, 0, 0, 1], [0.1, 0, 0, 0, 0, 0, 1]], np.float64)
    return dict(cam=CAM, cell_size=20, n_kf=2, n_points=P, kf_slot=np.array([0, 1], np.int32), T_kf_w=T, kf_key_point=key,
                kf_ftr_offset=np.array([0, len(row0), len(row0) + len(row1)], np.int32), kf_ftr_point=np.concatenate([row0, row1]),
                pt_pos=rng.uniform(-1, 1, (P, 3)), pt_type=np.where(is_cand, synth.TYPE_CANDIDATE, 2 + (np.arange(P) % 2)).astype(np.int32),
                pt_n_failed=rng.integers(0, 9, P).astype(np.int32), pt_n_succeeded=rng.integers(0, 9, P).astype(np.int32),
                pt_obs_offset=np.arange(P + 1, dtype=np.int32), obs_kf=dead.astype(np.int32), obs_px=px,
                obs_f=np.ascontiguousarray(synth.cam2world(CAM, px)), obs_level=(np.arange(P) % 3).astype(np.int32),
                obs_edgelet=(np.arange(P) % 7 == 0).astype(np.uint8), obs_grad=rng.uniform(-1, 1, (P, 2)),
                cand_point=np.where(is_cand)[0][::-1].astype(np.int32))


@pytest.mark.parametrize("P", SIZES)
def test_tables_at_small_shapes(ctx, P):
    trk = hip.Tracker(ctx, CAM, max_keyframes=2, max_points=P, max_obs=P, max_kf_features=P, max_candidates=P, max_fts=120, max_frame_features=128)
    pats = _patterns(P)
    assert len(pats) >= (1 if P == 1 else 3)
    for i, (name, dead) in enumerate(pats.items()):
        cs = _two_keyframe_map(P, dead, seed=100 * P + i)
        trk.set_map(cs)
        got = trk.remove_keyframe(1)
        removed, info = mr.remove_keyframe(cs, 1)
        assert got["n_deleted_points"] == dead.sum() == len(info["deleted_points"]) and got["n_deleted_candidates"] == 0, name
        before = trk.download_map()
        mg.assert_tables_equal(before, removed)
        c = trk.compact_points()
        dl, sizes = trk.download_map(), trk.map_sizes()
        model, minfo = mc.compact_points(removed, dead)
        assert c["n_points"] == minfo["n_points"] == P - dead.sum(), name
        assert c["old_to_new"].dtype == np.int32 and c["old_to_new"].tolist() == minfo["old_to_new"].tolist(), name
        assert sizes == _sizes(model), (name, sizes)
        mg.assert_tables_equal(dl, model)
        if name == "none":
            mg.assert_tables_equal(dl, before)                                                   # every table keeps its bytes
        again = trk.compact_points()                                                             # nothing is dead any more
        assert again["old_to_new"].tolist() == list(range(c["n_points"])) and trk.map_sizes() == sizes, name
        mg.assert_tables_equal(trk.download_map(), model)
    trk.destroy()


def test_a_map_without_points(ctx):
    trk = hip.Tracker(ctx, CAM, max_keyframes=2, max_fts=120, max_frame_features=128)
    empty = {k: np.zeros(0) for k in mg.TABLES}
    trk.set_map(empty)
    c = trk.compact_points()
    assert c["n_points"] == 0 and len(c["old_to_new"]) == 0
    assert trk.map_sizes() == dict(n_kf=0, n_ftr=0, n_points=0, n_obs=0, n_candidates=0)
    trk.destroy()


# ---- 2. the maps of tests/test_gpu_map_removal.py
@pytest.mark.parametrize("fam,k", ms.REMOVALS, ids=["%s-%d" % r for r in ms.REMOVALS])
def test_tables_after_a_removal(ctx, cases, fam, k):
    """the removal deletes points and candidates; the re-selection it owes the other keyframes is still pending when the points
    are renumbered"""
    cs = cases[fam]
    trk = _map_tracker(ctx, cs, images=False)
    trk.remove_keyframe(k)
    c = trk.compact_points()
    dl, sizes = trk.download_map(), trk.map_sizes()
    trk.destroy()
    removed, info = mr.remove_keyframe(cs, k)
    dead = np.zeros(cs["n_points"], bool)
    dead[info["deleted_points"] + info["deleted_candidates"]] = True
    model, minfo = mc.compact_points(removed, dead)
    assert dead.sum() >= 30 and (bool(info["rekeys"]) or (fam, k) in (("small", 1), ("small", 4)))      # a re-selection is owed
    assert c["n_points"] == minfo["n_points"] and c["old_to_new"].tolist() == minfo["old_to_new"].tolist() and sizes == _sizes(model)
    mg.assert_tables_equal(dl, model)
    mc.check_set_map_indices(dl, max_kf=cs["n_kf"], n_levels=5)


@pytest.mark.parametrize("k", [None, 1, 6])
def test_tables_after_deletions_by_tracking(ctx, cases, wide_first, k):
    """the wide case's first frame deletes points: they are unlinked with their observations, row entries, candidate entries and
    key-point entries still in the tables, and a re-selection is owed.  Compacted at once (k None) or after a removal."""
    cs, wf = cases["wide"], wide_first
    trk = _map_tracker(ctx, cs, max_fts=ms.wide_args()[2])
    r = trk.track(cs["cur_pyr"][0])
    _same(r, wf["r"], "first frame")
    if k is not None:
        trk.remove_keyframe(k)
    c = trk.compact_points()
    dl, sizes = trk.download_map(), trk.map_sizes()
    _same(trk.last_result(), r, "the result block of the last tracked frame is not rewritten")
    trk.destroy()
    tables, dead = dict(wf["tables"], cam=cs["cam"]), wf["unlinked"].copy()
    key = tables["kf_key_point"]
    assert dead[key[key >= 0]].any() and dead[tables["cand_point"]].any() and dead[tables["kf_ftr_point"]].any()
    if k is not None:
        tables, info = mr.remove_keyframe(tables, k, unlinked=dead, last_point=r["feat_point"])
        dead[info["deleted_points"] + info["deleted_candidates"]] = True
    model, minfo = mc.compact_points(tables, dead, cam=cs["cam"], last_point=r["feat_point"])
    assert (k is None) == bool(minfo["rekeyed"])                                                 # paid by the compaction, or by the removal before it
    assert c["n_points"] == minfo["n_points"] and c["old_to_new"].tolist() == minfo["old_to_new"].tolist() and sizes == _sizes(model)
    mg.assert_tables_equal(dl, model)
    mc.check_set_map_indices(dl, max_kf=cs["n_kf"], n_levels=5)


# ---- 3. and 4. compaction is unobservable; it makes room
def _mapped(m, a):
    a = np.asarray(a)
    return np.where(a >= 0, m[np.maximum(a, 0)], -1).astype(np.int32)


def _steady(trk, s, compact=(), refused_append=False, track=None):
    """the steady sequence of tests/test_gpu_map_removal.py, two steps longer: track, promote, candidates, track, promote, remove,
    [compact 0], track, (candidates refused), [compact 1 before / 2 after the second append], track, promote, track, remove,
    promote, track.  out["m"]: a point index of the tracker that never compacts -> this tracker's."""
    seq = s["seq"]
    track = track or (lambda frames: _frames(trk, seq, frames))
    out = dict(compactions=[])

    def compaction(n_before):
        c = trk.compact_points()
        assert len(c["old_to_new"]) == n_before
        out["compactions"].append(c)
        return c["old_to_new"]
    out["f12"] = track((1, 2))
    out["promote1"] = trk.promote_last_frame(1)
    out["first"] = trk.add_candidates(**s["cand"])
    out["f34"] = track((3, 4))
    out["promote2"] = trk.promote_last_frame(2)
    out["remove"] = trk.remove_keyframe(0)
    n_z = trk.map_sizes()["n_points"]                                                            # (nothing was compacted yet: Z's count)
    m = np.arange(n_z, dtype=np.int32)
    if 0 in compact:
        m = compaction(n_z)
        out["last_after_compaction"] = trk.last_result()
    out["map_removed"], out["sizes_removed"] = trk.download_map(), trk.map_sizes()
    out["f5"] = track((5,))
    new = _new_candidates(s, out["f12"][-1]["T_f_w"])
    n_new = len(new["kf_index"])
    if refused_append:
        with pytest.raises(hip.SvoHipError, match=r"\(-1\)"):                                    # max_points
            trk.add_candidates(**new)
        assert trk.map_sizes() == out["sizes_removed"]
    if 1 in compact:
        m = _mapped(compaction(trk.map_sizes()["n_points"]), m)
    out["first2"] = trk.add_candidates(**new)
    m = np.concatenate([m, out["first2"] + np.arange(n_new, dtype=np.int32)])                    # Z's new points follow its n_z
    if 2 in compact:
        m = _mapped(compaction(trk.map_sizes()["n_points"]), m)
    out["n_z_added"], out["n_new"] = n_z + n_new, n_new
    out["map_added"], out["sizes_added"] = trk.download_map(), trk.map_sizes()
    out["f6"] = track((6,))
    out["promote3"] = trk.promote_last_frame(out["remove"]["slot"])
    out["f7"] = track((7,))
    out["remove2"] = trk.remove_keyframe(0)
    out["promote4"] = trk.promote_last_frame(out["remove2"]["slot"])
    out["f8"] = track((8,))
    out["m"] = m
    out["map_final"], out["sizes_final"] = trk.download_map(), trk.map_sizes()
    return out


LATER = ("f5", "f6", "f7", "f8")


def _same_mapped(x, z, m, what):
    """track result x of a tracker that compacted == z of one that did not, z's point indices translated by m"""
    alive = m[:len(z["type"])] >= 0
    assert alive.sum() == len(x["type"]) and m[:len(z["type"])][alive].tolist() == list(range(alive.sum())), what
    for k in KEYS:
        want = z[k]
        if k == "feat_point":
            want = _mapped(m, z[k])
            assert (want >= 0).sum() == (z[k] >= 0).sum(), what                                  # no feature lies on a dead point
        elif k in ("type", "n_failed", "n_succeeded"):
            want = z[k][alive]
        assert x[k].shape == want.shape and x[k].tobytes() == want.tobytes(), (what, k)
    fx, fz = _fields(x["result"]), _fields(z["result"])
    assert fx == fz, (what, [k for k in fx if fx[k] != fz[k]])


@pytest.fixture(scope="module")
def runs(ctx, scen):
    """Z: no compaction.  X: compacts after the removal and again after the second append.  C: max_points too small for the
    second append until it compacts."""
    cam = scen["seq"]["cam"]

    def run(cfg, **kw):
        trk = hip.Tracker(ctx, cam, **cfg)
        _start(trk, scen["base"], scen["base_map"])
        out = _steady(trk, scen, **kw)
        pts = out["f8"][-1]["feat_point"]
        out["opt_points"] = pts[pts >= 0][:20]
        out["opt"] = trk.optimize_structure(out["opt_points"])
        trk.destroy()
        return out
    Z = run(CFG)
    X = run(CFG, compact=(0, 2))
    # the capacity: between the largest living count of the sequence and the final uncompacted n_points
    # (every point is alive until the first removal, so the largest living count is the count before it; X is fully compacted
    # after its second append: the living count there)
    cap = Z["sizes_removed"]["n_points"]
    assert X["sizes_added"]["n_points"] <= cap < Z["sizes_added"]["n_points"], (X["sizes_added"], cap, Z["sizes_added"])
    C = run(dict(CFG, max_points=cap), compact=(1,), refused_append=True)
    return dict(Z=Z, X=X, C=C, cap=cap)


def test_compaction_is_unobservable(runs):
    Z, X = runs["Z"], runs["X"]
    m = X["m"]
    c0, c2 = X["compactions"]
    assert (c0["old_to_new"] < 0).sum() >= 150 and c0["n_points"] == X["sizes_removed"]["n_points"] < Z["sizes_removed"]["n_points"]
    _same(X["last_after_compaction"], X["f34"][-1], "last_result right after a compaction returns the frame as it was tracked")
    for name in ("f12", "f34"):
        for i, (a, b) in enumerate(zip(X[name], Z[name])):
            _same(a, b, (name, i))
    # ---- every later frame, its point indices translated; the second compaction renumbers what frame 5 deleted (if anything)
    _same_mapped(X["f5"][0], Z["f5"][0], c0["old_to_new"], "f5")
    for name in ("f6", "f7", "f8"):
        _same_mapped(X[name][0], Z[name][0], m, name)
        assert X[name][0]["n_matches"] >= 50
    # ---- the appends, the later removal and the promotions
    assert X["first"] == Z["first"] and X["first2"] == c0["n_points"] and Z["first2"] == Z["sizes_removed"]["n_points"]
    assert m[Z["first2"]] == c2["old_to_new"][X["first2"]]
    for name in ("promote1", "promote2", "remove", "promote3", "remove2", "promote4"):
        assert X[name] == Z[name], name
    print("second removal:", Z["remove2"], "promotions:", Z["promote3"], Z["promote4"])
    assert Z["remove2"]["n_deleted_points"] >= 1 and Z["promote3"][1] >= 5
    # ---- optimize_structure on the same points under both numberings
    assert len(Z["opt_points"]) == 20 and _mapped(m, Z["opt_points"]).tolist() == X["opt_points"].tolist()
    assert X["opt"][0].tobytes() == Z["opt"][0].tobytes() and X["opt"][1].tolist() == Z["opt"][1].tolist()
    # ---- the tables: X's are the model's compaction of Z's
    for name, mm in (("map_removed", c0["old_to_new"]), ("map_added", m), ("map_final", m)):
        zt = Z[name]
        mm = mm[:zt["n_points"]]
        model, info = mc.compact_points(zt, mm < 0)
        assert info["old_to_new"].tolist() == mm.tolist(), name
        mg.assert_tables_equal(X[name], model)
    assert X["sizes_final"] == _sizes(X["map_final"]) and X["sizes_final"]["n_points"] < Z["sizes_final"]["n_points"]
    assert X["sizes_final"]["n_obs"] <= Z["sizes_final"]["n_obs"] and X["sizes_final"]["n_ftr"] <= Z["sizes_final"]["n_ftr"]


def test_compaction_makes_room(runs):
    """max_points = the uncompacted count before the second append: the append is refused, and accepted after compact_points()"""
    Z, C = runs["Z"], runs["C"]
    m = C["m"]
    assert C["sizes_removed"] == Z["sizes_removed"] and C["sizes_removed"]["n_points"] == runs["cap"]
    assert C["first2"] == C["compactions"][0]["n_points"] and C["first2"] + C["n_new"] <= runs["cap"] < Z["first2"] + Z["n_new"]
    for name in ("f6", "f7", "f8"):
        _same_mapped(C[name][0], Z[name][0], m, name)
    for name in ("promote3", "remove2", "promote4"):
        assert C[name] == Z[name], name
    for name in ("map_added", "map_final"):
        model, info = mc.compact_points(Z[name], m[:Z[name]["n_points"]] < 0)
        assert info["old_to_new"].tolist() == m[:Z[name]["n_points"]].tolist()
        mg.assert_tables_equal(C[name], model)
    assert C["opt"][0].tobytes() == Z["opt"][0].tobytes()


# ---- 5. refusals and groups
def test_no_map_is_refused(ctx, scen):
    trk = hip.Tracker(ctx, scen["seq"]["cam"], **CFG)
    with pytest.raises(hip.SvoHipError, match=r"tracker_compact_points.*\(-4\)"):
        trk.compact_points()
    with pytest.raises(hip.SvoHipError, match=r"\(-4\)"):                                        # still no map
        trk.map_sizes()
    _start(trk, scen["base"], scen["base_map"])                                                  # ... and nothing else changed
    r = trk.track(scen["seq"]["pyrs"][1][0])
    trk.destroy()
    ref = hip.Tracker(ctx, scen["seq"]["cam"], **CFG)
    _start(ref, scen["base"], scen["base_map"])
    _same(r, ref.track(scen["seq"]["pyrs"][1][0]), "after the refusal")
    ref.destroy()


def test_group_camera_compacts(ctx, scen):
    """camera 1 of a group goes through the sequence with compactions, camera 0 tracks on its one keyframe: camera 0's frames are
    those of a group whose camera 1 never compacts, camera 1's those of a lone tracker that compacts (the sums of SparseImgAlign
    grouped by tile on every side, so that nothing depends on the company)"""
    seq, full_map = scen["seq"], tc.sequence_map(scen["seq"])
    tile = (hip.SIA_OPT_REDUCTION, hip.SIA_REDUCTION_TILE_ORDER)
    cfg = dict(CFG, max_items=1024)
    lone = hip.Tracker(ctx, seq["cam"], **cfg)
    lone.set_sia_option(*tile)
    _start(lone, scen["base"], scen["base_map"])
    want1 = _steady(lone, scen, compact=(0, 2))
    lone.destroy()

    def group(compact):
        grp = hip.TrackerGroup(ctx, seq["cam"], 2, **cfg)
        grp.set_sia_option(*tile)
        _start(grp.cameras[0], seq, full_map)
        _start(grp.cameras[1], scen["base"], scen["base_map"])
        got0 = []

        def track(frames):
            out = []
            for k in frames:
                grp.track([seq["pyrs"][k][0]] * 2)
                got0.append(grp.cameras[0].last_result())
                out.append(grp.cameras[1].last_result())
            return out
        got1 = _steady(grp.cameras[1], scen, compact=compact, track=track)
        map0 = grp.cameras[0].download_map()
        grp.destroy()
        return got0, map0, got1
    got0, map0, got1 = group((0, 2))
    und0, und_map0, _ = group(())
    assert len(got0) == len(und0) == 8
    for i, (a, b) in enumerate(zip(got0, und0)):
        _same(a, b, (0, i))
    mg.assert_tables_equal(map0, und_map0)
    for name in ("f12", "f34") + LATER:
        for i, (a, b) in enumerate(zip(got1[name], want1[name])):
            _same(a, b, (1, name, i))
    for name in ("promote1", "first", "promote2", "remove", "first2", "promote3", "remove2", "promote4", "sizes_final"):
        assert got1[name] == want1[name], name
    assert [c["old_to_new"].tolist() for c in got1["compactions"]] == [c["old_to_new"].tolist() for c in want1["compactions"]]
    assert (got1["compactions"][0]["old_to_new"] < 0).sum() >= 150
    for name in ("map_removed", "map_added", "map_final"):
        mg.assert_tables_equal(got1[name], want1[name])


# ---- 6. the C++ host twin
# The chain's map has no depth filter behind it: `new_seeds S` makes every new keyframe seed S candidates, which is what lets
# n_points grow at all.  The roomy run (default max_points) writes map_points_room.bin = [the largest number of living points
# plus candidates waiting to be appended at the end of a frame, the rows of the device's point tables at the end].  The test
# takes max_points for the bounded runs from the first number as that run wrote it, and requires the second to be at least
# twice that, so that the bounded run has to compact at least twice.  Measured on an MI355X: [680, 1760]; with max_points 680
# the run with `compact` renumbers three times on its one upload, the run without uploads the map four times.
NEW_SEEDS = 40
N_TWIN_FRAMES = 30
TWIN_ARGS = ["incremental", "kf_every", "1", "max_kfs", "3", "new_seeds", str(NEW_SEEDS)]


def _twin_case(tmp_path):
    from test_gpu_host_cpp import _write_track_case
    seq = tc.make_sequence(n_frames=N_TWIN_FRAMES + 1)
    mp = tc.sequence_map(seq)
    n = len(seq["px0"])
    cs = dict(mp, obs_point=np.arange(n, dtype=np.int32), kf_ftr_obs=np.arange(n, dtype=np.int32), cand_obs=np.zeros(0, np.int32))
    cfg = dict(grid_size=tc.CELL, max_fts=tc.MAX_FTS, quality_min_fts=40, klt_min_level=2, max_frame_features=1024, keyframe_at=0)
    case = tmp_path / "case"
    case.mkdir()
    _write_track_case(case, cs, [seq["pyrs"][k][0] for k in range(1, N_TWIN_FRAMES + 1)], cfg, last_kf=0)
    return case


def _run_twin(case, out, extra):
    from test_gpu_host_cpp import DEMO
    assert os.path.exists(DEMO)
    out.mkdir()
    p = subprocess.run([DEMO, str(case), str(out), "track"] + TWIN_ARGS + extra, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert p.returncode == 0, (extra, p.stdout + p.stderr)
    return out


def test_host_twin_compacts_points(tmp_path):
    """hip_bridge::FrameTrackerT on the C++ twins (svo_host_demo track incremental kf_every 1 max_kfs 3 new_seeds S): thirty
    keyframes in a row, each seeding candidates, the map bounded at three keyframes.  With max_points at what the living points
    need and `compact` the map is uploaded once, the points are renumbered in place at least twice, and every file the demo writes
    about the tracked frames is byte for byte what the run with the default max_points writes.  Without `compact` the same
    bound costs full uploads."""
    n_frames = N_TWIN_FRAMES
    case = _twin_case(tmp_path)
    read = lambda tag, name: np.fromfile(outs[tag] / name)
    outs = dict(roomy=_run_twin(case, tmp_path / "out_roomy", []))
    room = read("roomy", "map_points_room.bin")
    max_points = int(room[0])
    assert room[1] >= 2 * max_points, room
    outs["compact"] = _run_twin(case, tmp_path / "out_compact", ["max_points", str(max_points), "compact"])
    outs["bounded"] = _run_twin(case, tmp_path / "out_bounded", ["max_points", str(max_points)])
    print("map_points_room.bin of the roomy run:", room, "compactions:", read("compact", "map_compactions.bin")[-1],
          "uploads without compact:", read("bounded", "track_uploads.bin")[-1])
    names = sorted(f for f in os.listdir(outs["roomy"]) if f.startswith("track_") and f.endswith(".bin"))
    assert len(names) > 10
    for tag in ("compact", "bounded"):
        assert names == sorted(f for f in os.listdir(outs[tag]) if f.startswith("track_") and f.endswith(".bin"))
        for f in names:
            if f != "track_uploads.bin":
                assert (outs["roomy"] / f).read_bytes() == (outs[tag] / f).read_bytes(), (tag, f)
    stats = read("roomy", "track_stats.bin").reshape(n_frames, 9)
    assert (stats[:, 1] >= 40).all() and (stats[:, 4] == 1).all()                                # every frame matched and was refined
    assert (read("roomy", "track_uploads.bin") == 1).all() and (read("roomy", "map_compactions.bin") == 0).all()
    up, comp = read("compact", "track_uploads.bin"), read("compact", "map_compactions.bin")
    assert len(up) == n_frames and (up == 1).all(), up
    assert comp[-1] >= 2 and (np.diff(comp) >= 0).all(), comp
    assert read("compact", "map_points_room.bin")[1] <= max_points
    assert read("bounded", "track_uploads.bin")[-1] > 1 and (read("bounded", "map_compactions.bin") == 0).all()
