"""The planning and replay kernels of the tracking chain (trk_plan_body / trk_replay_body, csrc/svo_track_chain.h) on the
constructed map families of tests/reproject_families.py: grids of 2048 and of more cells (cell counters in LDS / in global
memory, a scan of more counters than threads), frames of 2047, 2048, 2049 and 2600 items (sort keys in LDS / in global memory),
a cell of several hundred candidates, keyframe selections of 1, 16, 17 and 256 keyframes under reproj_max_n_kfs 1, 10 and 16
with exact distance ties, a point on each side of every comparison, and the cut of the cell loop.

Every case runs through a lone tracker (the by-value kernels) against the oracle's Reprojector::reprojectMap, which
tests/test_reproject_families_cpu.py pins to the reference's own compiled code on these very cases: every integer equal,
pixels and gradients bitwise, the item count equal to the numpy predicate's.  A case that changes the map is tracked a second
time and compared with the oracle run on the carried state.  Then the same cases through the table kernels: cameras of one
group that take different cases in one launch, and a subset call -- bit-equal to their lone trackers."""
import numpy as np
import pytest

import reproject_families as rf
from test_gpu_tracker_invariance import _same, _tile_order
from test_oracle_reproject_map import check_map_result, rekey_expected
from test_reproject_families_cpu import NAMES, as_fixture
from android_svo_amd import hip, synth
from oracle import orc

pytestmark = pytest.mark.gpu

CAPS = dict(max_points=4096, max_obs=8192, max_kf_features=8192, max_candidates=1024)
NO_FEATURES = (np.zeros((0, 2)), np.zeros((0, 3)), np.zeros(0, np.int32))


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


def _config(cs, max_keyframes=None):
    c = cs["cfg"]
    return dict(CAPS, max_keyframes=max_keyframes or max(cs["n_kf"], 1), grid_size=cs["cell_size"], max_fts=c["max_fts"],
                quality_min_fts=c["quality_min_fts"], reproj_max_n_kfs=c["reproj_max_n_kfs"], max_items=c["max_items"])


def _load(trk, cs):
    """the case's keyframes, map and -- as a last frame without features, so that SparseImgAlign::run returns at once and the new
    frame keeps the pose it was given -- the case's pose"""
    for k in range(cs["n_kf"]):                     # (keyframes that share an image upload the same array again: 256 tiny images)
        trk.upload_keyframe(int(cs["kf_slot"][k]), cs["kf_pyr"][k][0])
    trk.set_map(cs)
    trk.set_last_frame(cs["T_cur_w"], *NO_FEATURES, img=cs["cur_pyr"][0])


def _check(cs, r, ro, before, n_kept):
    """one tracked frame against the oracle's result `ro` for the map state `before`"""
    name, cam = cs["name"], cs["cam"]
    np.testing.assert_array_equal(r["T_f_w_sia"], cs["T_cur_w"])
    assert r["result"].items_overflow == 0
    assert int(r["result"].n_candidates) == n_kept, name
    n = len(ro["feat_point"])
    assert r["result"].n_features == n, name
    refined_expected = int(ro["n_matches"]) >= cs["cfg"]["quality_min_fts"] and n > 0
    dropped = r["feat_point"] < 0
    po = None
    if refined_expected:
        # the features as the reprojector made them: before the pose refinement drops observations
        po, hp = orc.pose_optimize(abs(cam.fx), cs["T_cur_w"], orc.cam2world(cam, ro["feat_px"]), cs["pt_pos"][ro["feat_point"]], ro["feat_level"],
                                   np.ones(n, np.uint8))
        np.testing.assert_array_equal(dropped, ~hp.astype(bool))
    else:
        assert not dropped.any(), name
    newly = (r["type"] == synth.TYPE_DELETED) & (before["pt_type"] != synth.TYPE_DELETED)
    res = dict(r, feat_point=np.where(dropped, ro["feat_point"], r["feat_point"]), unlinked=(newly | (before["unlinked"] == 1)).astype(np.uint8))
    check_map_result(as_fixture(name, ro), name, res)
    assert r["map_changed"] == int(((ro["unlinked"] == 1) & (before["unlinked"] == 0)).any()), name
    np.testing.assert_array_equal(r["feat_f"], orc.cam2world(cam, ro["feat_px"]) if n else np.zeros((0, 3)))
    if refined_expected and po.ran:
        rot, trans = synth.pose_error(r["T_f_w"], np.array(po.T_f_w))
        assert rot < 1e-9 and trans < 1e-9, (name, rot, trans)
        assert r["result"].pose.num_obs == po.num_obs
    else:
        # processFrame returns before the refinement: the frame keeps the last frame's pose, nothing of the refinement is valid
        np.testing.assert_array_equal(r["T_f_w"], cs["T_cur_w"])
        pose = r["result"].pose
        assert pose.ran == 0 and pose.num_obs == 0 and pose.n_iter_done == 0 and pose.error_init == 0.0 and pose.error_final == 0.0
        np.testing.assert_array_equal(np.array(pose.T_f_w), r["T_f_w_sia"])


_lone = {}


def lone_run(ctx, name, max_keyframes=None):
    """the case through a lone tracker: [first frame, second frame], both checked against the oracle; run once per case"""
    key = (name, max_keyframes)
    if key in _lone:
        return _lone[key]
    cs = rf.case_named(name)
    ro = rf.oracle_result(cs)
    trk = hip.Tracker(ctx, cs["cam"], **_config(cs, max_keyframes))
    _tile_order(trk)
    assert trk.n_cells == rf.grid(cs)[2]
    _load(trk, cs)
    r1 = trk.track(cs["cur_pyr"][0])
    before = rf.fresh_state(cs)
    _check(cs, r1, ro, before, rf.plan(cs)["n_kept"])
    # a second frame at the same pose over the map as the first one left it on the device: counters moved, points promoted;
    # where the map changed, unlinked points in the feature lists and the candidate list and key features chosen again
    state = rf.state_of(ro)
    deleted = state["unlinked"].astype(bool)
    key2 = rekey_expected(cs, cs["kf_key_point"], deleted)
    np.testing.assert_array_equal(trk.download_key_points(cs["n_kf"]), key2)
    n_kept2 = rf.plan(dict(cs, kf_key_point=key2), state)["n_kept"]
    ro2 = orc.reproject_map(cs, key2, max_fts=cs["cfg"]["max_fts"], max_n_kfs=cs["cfg"]["reproj_max_n_kfs"], state=rf.state_of(ro))
    trk.set_last_frame(cs["T_cur_w"], *NO_FEATURES, img=cs["cur_pyr"][0])
    r2 = trk.track(cs["cur_pyr"][0])
    _check(cs, r2, ro2, state, n_kept2)
    trk.destroy()
    _lone[key] = [r1, r2]
    return _lone[key]


@pytest.mark.parametrize("name", NAMES)
def test_family_case_through_a_lone_tracker(ctx, name):
    r1, r2 = lone_run(ctx, name)
    cs = rf.case_named(name)
    pl = rf.plan(cs)
    # the path the case is named for, as the device saw it
    if name.startswith("cells_"):
        assert (rf.grid(cs)[2] > rf.LDS_CELLS) == (name != "cells_lds_2048")
    if name.startswith("items_"):
        assert int(r1["result"].n_candidates) == int(name.split("_")[1]) == pl["n_kept"]
    if name in ("crowded", "boundaries", "cut_none") or name.startswith(("cells_", "items_")):
        assert r1["map_changed"] == 1
    if name in ("cut_max_fts_0", "cut_in_last_match") or name.startswith("kf_"):
        assert r1["map_changed"] == 0
    assert (r2["n_succeeded"] >= r1["n_succeeded"]).all() and (r2["n_succeeded"] > r1["n_succeeded"]).any()
    if name == "cut_quality_above":
        assert r1["n_matches"] == cs["cfg"]["quality_min_fts"] - 1 and r1["result"].pose.ran == 0
    if name == "cut_none":
        assert r1["n_matches"] == cs["cfg"]["quality_min_fts"] and r1["result"].pose.ran == 1


def _group_of(ctx, names, max_keyframes):
    cases = [rf.case_named(n) for n in names]
    cfgs = [_config(cs, max_keyframes) for cs in cases]
    assert all(c == cfgs[0] for c in cfgs) and len({(cs["cam"].width, cs["cam"].height) for cs in cases}) == 1
    grp = hip.TrackerGroup(ctx, cases[0]["cam"], len(cases), **cfgs[0])
    _tile_order(grp.cameras[0])
    for cam, cs in zip(grp.cameras, cases):
        _load(cam, cs)
    return grp, cases


GROUPS = {"items": (["items_2047", "items_2048", "items_2049", "items_2600"], 4),
          "kf_m16": (["kf_n1_m16", "kf_n256_m16", "kf_n16_m16", "kf_n17_m16"], 256),
          "kf_m1": (["kf_n17_m1", "kf_n1_m1", "kf_n256_m1"], 256),
          "cut_and_boundaries": (["cut_none", "boundaries"], 3)}


@pytest.mark.parametrize("tag", list(GROUPS))
def test_cameras_of_a_group_take_different_cases_in_one_launch(ctx, tag):
    """the table kernels: every camera bit-equal to its lone tracker -- in the group call, and in a call over a subset of the cameras
    (the others keep their frame)"""
    names, max_kf = GROUPS[tag]
    if tag == "cut_and_boundaries":                 # one configuration per group: the two cases differ in nothing but the map
        assert _config(rf.case_named("cut_none"), 3) == _config(rf.case_named("boundaries"), 3)
    want = [lone_run(ctx, n, max_kf) for n in names]
    grp, cases = _group_of(ctx, names, max_kf)
    if tag == "items":
        kept = [rf.plan(cs)["n_kept"] for cs in cases]
        assert min(kept) <= rf.LDS_ITEMS < max(kept)                   # both homes of the sort keys in one launch
    grp.track([cs["cur_pyr"][0] for cs in cases])
    for c, cam in enumerate(grp.cameras):
        _same(cam.last_result(), want[c][0], (tag, names[c], "group call"))
    # a subset call: some cameras track their second frame (for "items" one on each side of the limit), the others sit the call out
    some = [1, 3] if tag == "items" else [len(names) - 1] if len(names) == 2 else [0, len(names) - 1]
    for c in some:
        grp.cameras[c].set_last_frame(cases[c]["T_cur_w"], *NO_FEATURES, img=cases[c]["cur_pyr"][0])
    grp.track_some(some, [cases[c]["cur_pyr"][0] for c in some])
    for c, cam in enumerate(grp.cameras):
        _same(cam.last_result(), want[c][1 if c in some else 0], (tag, names[c], "subset call"))
    grp.destroy()
