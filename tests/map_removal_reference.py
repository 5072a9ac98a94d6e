"""What removing a keyframe does to the index tables of hip.Tracker.set_map -- a list/numpy restatement of the reference's object
code, the yardstick of tests/test_map_removal_model.py (CPU) and tests/test_gpu_map_removal.py (device):

    remove_keyframe     Map::safeDeleteFrame (S/map.cpp:41-64) with removePtFrameRef (:66-80), safeDeletePoint (:82-93), deletePoint
                        (:95-99), Point::deleteFrameRef (S/point.cpp:75-86), MapPointCandidates::removeFrameCandidates /
                        deleteCandidate (S/map.cpp:271-285, :297-304) and Frame::removeKeyPoint / setKeyPoints / checkKeyPoints
                        (S/frame.cpp:84-162) on the keyframes that lose a key feature

Tables are dicts of numpy arrays (map_growth_reference's); the function returns a new dict and leaves its input alone.  The
output is canonical: what a host flatten under the same point numbering writes -- an unlinked point has no observations, is in no
feature row and not in the candidate list."""
import numpy as np

from android_svo_amd import synth
from map_growth_reference import TABLES, _DTYPE, _SHAPE, assert_tables_equal, normalised  # noqa: F401  (re-exported)


def _raw_value(cu, cv, j, x, y):
    """what checkKeyPoints compares in slot j, larger = better (slot 0: the distance from the centre, negated)"""
    return -max(abs(x - cu), abs(y - cv)) if j == 0 else (x - cu) * (y - cv)


def _contends(cu, cv, j, x, y):
    """the quadrant tests of checkKeyPoints; the two left quadrants test x against cv as the reference does (S/frame.cpp:129,138)"""
    return (True, x >= cu and y >= cv, x >= cu and y < cv, x < cv and y < cv, x < cv and y >= cv)[j]


def set_key_points(cam, cur, row, dead, px_of):
    """Frame::setKeyPoints: key features whose point is gone are cleared, then every feature of `row` (fts_ order) that still has
    a point runs checkKeyPoints -- an empty slot takes the first contender, an incumbent stays unless strictly beaten.
    cur: the five key points (point index or -1), changed in place; px_of(p) = the pixel of p's feature in this keyframe."""
    cu, cv = cam.width // 2, cam.height // 2
    for j in range(5):
        if cur[j] >= 0 and (dead[cur[j]] or px_of(cur[j]) is None):
            cur[j] = -1
    for p in row:
        if dead[p] or px_of(p) is None:
            continue
        x, y = px_of(p)
        for j in range(5):
            if not _contends(cu, cv, j, x, y):
                continue
            if cur[j] < 0 or _raw_value(cu, cv, j, x, y) > _raw_value(cu, cv, j, *px_of(cur[j])):
                cur[j] = p


def remove_keyframe(tables, k, unlinked=None, rekey="per_deletion", cam=None, last_point=None):
    """Keyframe k leaves the map.  unlinked[n_points]: points earlier frames deleted (the device's pt_unlinked): their features
    have no point; the re-selection of key points those deletions owe is applied first, on the rows as they were, once per
    keyframe.  rekey: "per_deletion" = the reference (setKeyPoints at every removeKeyPoint hit while keyframe k's row is walked
    in order), "once" = the device (the keyframes that lost a key feature choose again once, afterwards).  cam: default
    tables["cam"].  last_point: the points of the last frame's features (info["last_lost"] = the features that lose theirs).
    Returns (tables, info); info: deleted_points, deleted_candidates (point indices, in the order of deletion), slot (the
    pyramid slot freed), rekeys {keyframe index BEFORE the removal: number of re-selections}, last_lost."""
    assert rekey in ("per_deletion", "once")
    cam = cam if cam is not None else tables["cam"]
    t = normalised(tables)
    K, P = t["n_kf"], t["n_points"]
    assert 0 <= k < K and K > 1
    off, obs_kf = t["pt_obs_offset"], t["obs_kf"]
    dead = np.zeros(P, bool) if unlinked is None else np.asarray(unlinked, bool).copy()
    obs = [[] if dead[p] else list(range(off[p], off[p + 1])) for p in range(P)]
    rows = [[int(p) for p in t["kf_ftr_point"][t["kf_ftr_offset"][j]:t["kf_ftr_offset"][j + 1]] if p >= 0 and not dead[p]] for j in range(K)]
    key = [[int(p) for p in t["kf_key_point"][j]] for j in range(K)]
    obs_in = [dict() for _ in range(K)]                                 # keyframe -> {point: its (first) observation there}
    for p in range(P):
        for o in range(off[p], off[p + 1]):
            obs_in[obs_kf[o]].setdefault(p, o)

    def choose_again(j):
        set_key_points(cam, key[j], rows[j], dead, lambda p: t["obs_px"][obs_in[j][p]] if p in obs_in[j] else None)

    if unlinked is not None:                                            # owed by the last frame's deletions
        for j in range(K):
            if any(p >= 0 and dead[p] for p in key[j]):
                choose_again(j)
    rekeys, lost = {}, set()

    def remove_key_point(j, p):                                         # Frame::removeKeyPoint (keyframe k's own are going anyway)
        if j == k or p not in key[j]:
            return
        key[j] = [-1 if q == p else q for q in key[j]]
        if rekey == "per_deletion":
            rekeys[j] = rekeys.get(j, 0) + 1
            choose_again(j)
        else:
            lost.add(j)

    deleted_points, deleted_candidates = [], []
    for p in rows[k]:                                                   # Map::removePtFrameRef over fts_
        if dead[p]:
            continue                                                    # ftr->point == NULL
        if len(obs[p]) <= 2:                                            # Map::safeDeletePoint
            dead[p] = True
            for o in obs[p]:
                remove_key_point(int(obs_kf[o]), p)
            obs[p] = []
            t["pt_type"][p] = synth.TYPE_DELETED
            deleted_points.append(p)
        else:                                                           # Point::deleteFrameRef
            hit = [o for o in obs[p] if obs_kf[o] == k][:1]
            obs[p] = [o for o in obs[p] if o not in hit]
    for j in sorted(lost):
        rekeys[j] = 1
        choose_again(j)
    left = []
    for p in t["cand_point"]:                                           # MapPointCandidates::removeFrameCandidates
        p = int(p)
        if p < 0 or dead[p]:
            continue                                                    # (an entry the host's list no longer holds)
        if obs[p] and obs_kf[obs[p][-1]] == k:                          # it->second->frame == frame: deleteCandidate
            dead[p] = True
            obs[p] = []
            t["pt_type"][p] = synth.TYPE_DELETED
            deleted_candidates.append(p)
        else:
            left.append(p)
    # ---- the tables a host flatten writes now
    keep_kf = [j for j in range(K) if j != k]
    new_rows = [[p for p in rows[j] if not dead[p]] for j in keep_kf]
    flat = [o for p in range(P) for o in obs[p] if obs_kf[o] != k]      # (an observation in a frame that is no keyframe is skipped)
    out = dict(t)
    out["pt_obs_offset"] = np.concatenate([[0], np.cumsum([sum(1 for o in obs[p] if obs_kf[o] != k) for p in range(P)])]).astype(np.int32)
    for c in ("obs_kf", "obs_px", "obs_f", "obs_level", "obs_edgelet", "obs_grad"):
        out[c] = t[c][flat] if len(flat) else t[c][:0]
    out["obs_kf"] = np.where(out["obs_kf"] > k, out["obs_kf"] - 1, out["obs_kf"]).astype(np.int32)
    out["kf_slot"], out["T_kf_w"] = t["kf_slot"][keep_kf], t["T_kf_w"][keep_kf]
    out["kf_key_point"] = np.array([key[j] for j in keep_kf], np.int32).reshape(-1, 5)
    out["kf_ftr_offset"] = np.concatenate([[0], np.cumsum([len(r) for r in new_rows])]).astype(np.int32)
    out["kf_ftr_point"] = np.array([p for r in new_rows for p in r], np.int32)
    out["cand_point"] = np.array(left, np.int32)
    gone = set(deleted_points) | set(deleted_candidates)
    info = dict(deleted_points=deleted_points, deleted_candidates=deleted_candidates, slot=int(t["kf_slot"][k]), rekeys=rekeys,
                last_lost=[] if last_point is None else [i for i, p in enumerate(np.asarray(last_point)) if int(p) in gone])
    return normalised(out), info


def unlinked_of(tables):
    """which points of canonical tables are unlinked as far as the tables can tell: TYPE_DELETED without an observation"""
    t = normalised(tables)
    return (t["pt_type"] == synth.TYPE_DELETED) & (np.diff(t["pt_obs_offset"]) == 0)


def check_invariants(tables, unlinked):
    """the CSR invariants of canonical tables: no index out of range, no unlinked point in a row, in the candidate list or with an
    observation, the sizes consistent"""
    t = normalised(tables)
    K, P = t["n_kf"], t["n_points"]
    n_obs, n_ftr = len(t["obs_kf"]), len(t["kf_ftr_point"])
    assert len(t["kf_ftr_offset"]) == K + 1 and t["kf_ftr_offset"][0] == 0 and t["kf_ftr_offset"][-1] == n_ftr
    assert len(t["pt_obs_offset"]) == P + 1 and t["pt_obs_offset"][0] == 0 and t["pt_obs_offset"][-1] == n_obs
    assert (np.diff(t["kf_ftr_offset"]) >= 0).all() and (np.diff(t["pt_obs_offset"]) >= 0).all()
    assert len(t["T_kf_w"]) == len(t["kf_key_point"]) == K
    for c in ("obs_px", "obs_f", "obs_level", "obs_edgelet", "obs_grad"):
        assert len(t[c]) == n_obs, c
    assert n_obs == 0 or (t["obs_kf"].min() >= 0 and t["obs_kf"].max() < K)
    assert n_ftr == 0 or (t["kf_ftr_point"].min() >= 0 and t["kf_ftr_point"].max() < P)
    assert len(set(t["kf_slot"].tolist())) == K
    unl = np.asarray(unlinked, bool)
    assert not unl[t["kf_ftr_point"]].any() and not unl[t["cand_point"]].any()
    assert not np.diff(t["pt_obs_offset"])[unl].any()
    assert (t["cand_point"] >= 0).all() and (t["cand_point"] < P).all()
    key = t["kf_key_point"]
    assert (key >= -1).all() and (key < P).all() and not unl[key[key >= 0]].any()
    for j in range(K):                                                  # a feature row and the observations agree
        row = t["kf_ftr_point"][t["kf_ftr_offset"][j]:t["kf_ftr_offset"][j + 1]]
        seen = np.repeat(np.arange(P), np.diff(t["pt_obs_offset"]))[t["obs_kf"] == j]
        assert set(row.tolist()) <= set(seen.tolist()), j
        assert set(key[j][key[j] >= 0].tolist()) <= set(row.tolist()), j
