"""What the tracker remembers on the host about the device's last frame (svo_track.hip: host_set_last, frame_tracked, gate_refused,
map_accepted, points_renumbered), seen through the calls whose answer depends on it -- the consequences no other file pins.  One
tracker on the small map case of tests/map_removal_scenario.py per test; a frame is "tracked" by the case's current image."""
import ctypes as C

import numpy as np
import pytest

import map_growth_reference as mg
import map_removal_scenario as ms
from test_gpu_map_growth import _same
from test_gpu_map_removal import _map_tracker
from android_svo_amd import hip

pytestmark = pytest.mark.gpu

STATE = r"\(-4\)"
REMOVED_KF = 2                                        # (tests/test_gpu_map_compaction.py: its removal deletes >= 30 points)


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cs():
    return ms.small_case()


def _tracked(ctx, cs):
    trk = _map_tracker(ctx, cs)
    return trk, trk.track(cs["cur_pyr"][0])


def _no_tracked_frame(trk):
    """the two calls that need the last frame to be a tracked one refuse, and change nothing"""
    before = trk.download_map()
    with pytest.raises(hip.SvoHipError, match=STATE):
        trk.last_result()
    with pytest.raises(hip.SvoHipError, match=STATE):
        trk.promote_last_frame(0)
    mg.assert_tables_equal(trk.download_map(), before)


def test_a_last_frame_the_host_made_is_not_a_tracked_one(ctx, cs):
    fresh = _map_tracker(ctx, cs)                                                  # (its last frame was set by the host)
    _no_tracked_frame(fresh)
    fresh.destroy()
    trk, r = _tracked(ctx, cs)
    _same(trk.last_result(), r, "after the tracked frame")
    # svo_hip_tracker_set_last_frame
    trk.set_last_frame(r["T_f_w"], r["feat_px"], r["feat_f"], r["feat_point"], kf_slot=0)
    _no_tracked_frame(trk)
    r2 = trk.track(cs["cur_pyr"][0])
    _same(trk.last_result(), r2, "tracked again")
    # svo_hip_tracker_last_frame_from_keyframe
    assert trk.last_frame_from_keyframe(1) > 0
    _no_tracked_frame(trk)
    r3 = trk.track(cs["cur_pyr"][0])
    _same(trk.last_result(), r3, "tracked a third time")
    # a relocalisation whose gate refuses: the last frame is the new image without features
    rx = trk.relocalize(cs["cur_pyr"][0], None, min_tracked=10 ** 6)
    assert rx["reloc"].accepted == 0 and rx["reloc"].kf_index >= 0
    _no_tracked_frame(trk)
    assert trk.finish_frame([])[2]["n_depths"] == 0
    trk.destroy()


def _removed_and_compacted(ctx, cs):
    """a tracked frame, then a removal that deletes points and the renumbering.  Returns (tracker, the frame, old_to_new)."""
    trk, r = _tracked(ctx, cs)
    assert trk.remove_keyframe(REMOVED_KF)["n_deleted_points"] >= 30
    c = trk.compact_points()
    assert c["n_points"] < len(r["type"]) == len(c["old_to_new"])
    return trk, r, c["old_to_new"]


def test_last_result_after_a_compaction_has_the_tracked_frames_layout(ctx, cs):
    trk, r, _ = _removed_and_compacted(ctx, cs)
    P = len(r["type"])                                                             # n_points when the frame was tracked
    assert trk.map_sizes()["n_points"] < P
    # straight through the C-ABI into buffers with room to spare: exactly P counters each, under the old numbering
    out = [np.full(P + 8, -7, np.int32) for _ in range(3)]
    res = hip.CTrackResult()
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    rc = ctx.lib.svo_hip_tracker_last_result(trk.h, C.byref(res), None, None, None, None, None, None, ptr(out[0]), ptr(out[1]), ptr(out[2]))
    assert rc == 0 and res.n_features == r["result"].n_features
    for got, key in zip(out, ("type", "n_failed", "n_succeeded")):
        assert got[:P].tobytes() == r[key].tobytes() and (got[P:] == -7).all(), key
    _same(trk.last_result(), r, "the wrapper's view")
    trk.destroy()


def _first_points(tables, n):
    """the tables cut down to their first n points: a valid map for svo_hip_tracker_set_map"""
    t = mg.normalised(tables)
    n_obs = int(t["pt_obs_offset"][n])
    out = dict(t, n_points=n, pt_obs_offset=t["pt_obs_offset"][:n + 1], cand_point=t["cand_point"][t["cand_point"] < n],
               kf_ftr_point=np.where(t["kf_ftr_point"] < n, t["kf_ftr_point"], -1), kf_key_point=np.where(t["kf_key_point"] < n, t["kf_key_point"], -1))
    for k in ("pt_pos", "pt_type", "pt_n_failed", "pt_n_succeeded"):
        out[k] = t[k][:n]
    for k in ("obs_kf", "obs_px", "obs_f", "obs_level", "obs_edgelet", "obs_grad"):
        out[k] = t[k][:n_obs]
    return out


def test_set_map_after_a_compaction_checks_the_renumbered_bound(ctx, cs):
    """after the renumbering the largest point the last frame refers to is the kernel's answer under the new numbering, not what the
    result block (old numbering) says: a map with exactly that many points keeps the last frame, one point fewer does not"""
    trk, r, o2n = _removed_and_compacted(ctx, cs)
    fp = r["feat_point"][r["feat_point"] >= 0]
    living = o2n[fp][o2n[fp] >= 0]                                                 # (a feature whose point was deleted has lost it)
    bound = int(living.max())
    assert len(living) >= 20 and bound < int(fp.max())                             # the two numberings give different answers
    tables = dict(trk.download_map(), cam=cs["cam"])
    trk.set_map(_first_points(tables, bound + 1))
    d = trk.finish_frame([])[2]                                                    # needs the last frame, reads only
    assert d["overlap_valid"] == 0 and d["n_depths"] == len(living)
    _same(trk.last_result(), r, "the result block is the tracked frame's still")
    trk.set_map(_first_points(tables, bound))
    with pytest.raises(hip.SvoHipError, match=STATE):
        trk.finish_frame([])
    with pytest.raises(hip.SvoHipError, match=STATE):
        trk.track(cs["cur_pyr"][0])                                                # asks for svo_hip_tracker_set_last_frame
    trk.set_last_frame(cs["T_cur_w"], np.zeros((0, 2)), np.zeros((0, 3)), np.zeros(0, np.int32), img=cs["cur_pyr"][0])
    assert trk.track(cs["cur_pyr"][0])["result"].n_features >= 0
    trk.destroy()
