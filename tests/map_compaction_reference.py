"""What renumbering the points does to the index tables of hip.Tracker.set_map -- the yardstick of
tests/test_map_compaction_model.py (CPU) and tests/test_gpu_map_compaction.py (device), in the dict-of-numpy style of
map_growth_reference / map_removal_reference.  Written from the semantics of svo_hip_tracker_compact_points in include/svo_hip.h:

    * a point is dead exactly when `unlinked` says so (the device's pt_unlinked: deleted by a tracked frame or by a removal).
      Its type does not decide: set_map unlinks nothing, so a point uploaded as TYPE_DELETED is a living row;
    * the re-selection of key points that the deletions still owe (a keyframe one of whose key points is dead) comes first, on the
      rows as they were: Frame::setKeyPoints as map_removal_reference.set_key_points states it;
    * living points keep their order, old_to_new[p] = the number of living points below p, -1 for a dead point;
    * the output is what a host flatten under the new numbering writes: no row, no observation, no feature-row entry and no
      candidate entry of a dead point, -1 entries dropped, every order kept, every index mapped.

The function returns a new dict and leaves its input alone."""
import numpy as np

import map_removal_reference as mr
from map_growth_reference import TABLES, assert_tables_equal, normalised  # noqa: F401  (re-exported)


def compact_points(tables, unlinked, cam=None, last_point=None):
    """unlinked[n_points]: the dead points.  cam: for the owed re-selection (default tables["cam"]; needed only when a key point is
    dead).  last_point: the points of the last frame's features.  Returns (tables, info); info: n_points, old_to_new (int32),
    last_point (mapped: -1 stays, a dead point becomes -1; None when not given), rekeyed (keyframes that chose again)."""
    t = normalised(tables)
    K, P = t["n_kf"], t["n_points"]
    dead = np.asarray(unlinked, bool).copy()
    assert dead.shape == (P,)
    off, obs_kf = t["pt_obs_offset"] if P else np.zeros(1, np.int32), t["obs_kf"]
    rows = [[int(p) for p in t["kf_ftr_point"][t["kf_ftr_offset"][j]:t["kf_ftr_offset"][j + 1]] if p >= 0 and not dead[p]] for j in range(K)]
    key = [[int(p) for p in t["kf_key_point"][j]] for j in range(K)]
    # ---- the owed re-selection
    rekeyed = [j for j in range(K) if any(p >= 0 and dead[p] for p in key[j])]
    if rekeyed:
        cam = cam if cam is not None else tables["cam"]
        obs_in = [dict() for _ in range(K)]                             # keyframe -> {point: its (first) observation there}
        for p in range(P):
            for o in range(off[p], off[p + 1]):
                obs_in[obs_kf[o]].setdefault(p, o)
        for j in rekeyed:
            mr.set_key_points(cam, key[j], rows[j], dead, lambda p, j=j: t["obs_px"][obs_in[j][p]] if p in obs_in[j] else None)
    # ---- the new numbering
    alive = ~dead
    old_to_new = np.where(alive, np.cumsum(alive) - 1, -1).astype(np.int32)
    m = lambda p: int(old_to_new[p]) if p >= 0 else -1
    n_obs = np.diff(off)
    keep_obs = np.repeat(alive, n_obs)
    out = dict(t)
    for c in ("pt_pos", "pt_type", "pt_n_failed", "pt_n_succeeded"):
        out[c] = t[c][alive]
    out["pt_obs_offset"] = np.concatenate([[0], np.cumsum(n_obs[alive])]).astype(np.int32)
    for c in ("obs_kf", "obs_px", "obs_f", "obs_level", "obs_edgelet", "obs_grad"):
        out[c] = t[c][keep_obs]
    out["kf_ftr_offset"] = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32) if K else t["kf_ftr_offset"]
    out["kf_ftr_point"] = np.array([m(p) for r in rows for p in r], np.int32)
    out["kf_key_point"] = np.array([[m(p) for p in kj] for kj in key], np.int32).reshape(-1, 5)
    out["cand_point"] = np.array([m(int(p)) for p in t["cand_point"] if p >= 0 and alive[p]], np.int32)
    out = normalised(out)
    info = dict(n_points=int(alive.sum()), old_to_new=old_to_new, rekeyed=rekeyed,
                last_point=None if last_point is None else np.array([m(int(p)) for p in np.asarray(last_point)], np.int32))
    return out, info


def relabel(tables, old_to_new):
    """point indices of tables whose dead points are already out of every list (canonical tables) mapped by old_to_new, the rows
    of the pt_* tables left where they are: what is left to compare when only the numbering differs"""
    t = normalised(tables)
    o2n = np.asarray(old_to_new, np.int32)
    mp = lambda a: np.where(a >= 0, o2n[np.maximum(a, 0)], -1).astype(np.int32)
    return dict(t, kf_ftr_point=mp(t["kf_ftr_point"]), kf_key_point=mp(t["kf_key_point"]), cand_point=mp(t["cand_point"]))


def check_set_map_indices(tables, max_kf=None, n_levels=None):
    """the index checks svo_hip_tracker_set_map makes on the host, on numpy tables"""
    t = normalised(tables)
    K, P = t["n_kf"], t["n_points"]
    n_ftr = int(t["kf_ftr_offset"][K]) if K else 0
    n_obs = int(t["pt_obs_offset"][P]) if P else 0
    assert len(t["kf_ftr_point"]) == n_ftr and len(t["obs_kf"]) == n_obs
    assert K == 0 or (len(t["kf_ftr_offset"]) == K + 1 and t["kf_ftr_offset"][0] >= 0 and (np.diff(t["kf_ftr_offset"]) >= 0).all())
    assert (t["kf_slot"] >= 0).all() and (max_kf is None or (t["kf_slot"] < max_kf).all())
    assert (t["kf_key_point"] >= -1).all() and (t["kf_key_point"] < P).all()
    assert (t["kf_ftr_point"] >= -1).all() and (t["kf_ftr_point"] < P).all()
    assert P == 0 or (len(t["pt_obs_offset"]) == P + 1 and t["pt_obs_offset"][0] >= 0 and (np.diff(t["pt_obs_offset"]) >= 0).all())
    assert (t["pt_type"] >= 0).all() and (t["pt_type"] <= 3).all()
    assert (t["obs_kf"] >= 0).all() and (t["obs_kf"] < K).all() and (t["obs_level"] >= 0).all()
    assert n_levels is None or (t["obs_level"] < n_levels).all()
    assert (t["cand_point"] >= -1).all() and (t["cand_point"] < P).all()
    for c in ("pt_pos", "pt_n_failed", "pt_n_succeeded"):
        assert len(t[c]) == P, c
    for c in ("obs_px", "obs_f", "obs_level", "obs_edgelet", "obs_grad"):
        assert len(t[c]) == n_obs, c
