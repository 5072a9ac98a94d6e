"""What FrameHandlerMono::processFrame decides behind the structure step, on the index tables of hip.Tracker.set_map -- a numpy
restatement of the reference's object code, the yardstick of tests/test_keyframe_decision_model.py (CPU, pinned there to the C++
twins and their std::nth_element) and of tests/test_gpu_keyframe_decision.py (device):

    scene_depth        frame_utils::getSceneDepth (S/frame.cpp:200-221) with vk::getMedian (I/math_utils.h:125-131)
    need_new_kf        FrameHandlerMono::needNewKf (S/frame_handler_mono.cpp:391-403)
    furthest_keyframe  Map::getFurthestKeyframe (S/map.cpp:156-169)
    decision           the three together, as svo_hip_kf_decision reports them

Poses go through synth.se3_act / synth.se3_inv, which perform svo_device_math.h's operations in the same order; tables are the
dicts of tests/map_growth_reference.py.  What the reference leaves undefined is defined as the library defines it: depth_mean is
NaN without a depth and when a depth is NaN."""
import math

import numpy as np

from android_svo_amd import synth

DBL_MAX = float(np.finfo(np.float64).max)


def frame_pos(T_f_w):
    """Frame::pos(): the translation of T_f_w^-1"""
    return synth.se3_inv(np.asarray(T_f_w, dtype=np.float64))[:3]


def scene_depth(tables, T_f_w, feat_point):
    """(n_depths, n_nan_depths, depth_mean, depth_min) over the features with a point, in feature order"""
    T = np.asarray(T_f_w, dtype=np.float64)
    pos = np.asarray(tables["pt_pos"], dtype=np.float64).reshape(-1, 3)
    z, n_nan = [], 0
    depth_min = DBL_MAX
    for p in feat_point:
        if p < 0:
            continue
        d = float(synth.se3_act(T, pos[int(p)])[2])
        if d != d:
            n_nan += 1                         # (fmin skips it)
            continue
        z.append(d)
        depth_min = d if d < depth_min else depth_min
    depth_mean = sorted(z)[len(z) // 2] if z and n_nan == 0 else math.nan
    return len(z), n_nan, depth_mean, depth_min


def rel_pos(tables, T_f_w, kf):
    """new_frame_->w2f(kf->pos())"""
    Tk = np.asarray(tables["T_kf_w"], dtype=np.float64).reshape(-1, 7)[int(kf)]
    return synth.se3_act(np.asarray(T_f_w, dtype=np.float64), frame_pos(Tk))


def need_new_kf(tables, T_f_w, overlap_kf, depth_mean, min_dist):
    """(need_new_kf, blocking_kf): false at the first overlap keyframe inside the box"""
    d = np.float64(min_dist)
    with np.errstate(divide="ignore", invalid="ignore"):
        for kf in overlap_kf:
            r = rel_pos(tables, T_f_w, kf)
            m = np.float64(depth_mean)
            if abs(r[0]) / m < d and abs(r[1]) / m < d * np.float64(0.8) and abs(r[2]) / m < d * np.float64(1.3):
                return 0, int(kf)
    return 1, -1


def furthest_keyframe(tables, pos):
    """(kf_index, distance): dist > maxdist from 0.0 in keyframe order"""
    Tk = np.asarray(tables["T_kf_w"], dtype=np.float64).reshape(-1, 7)
    best, maxdist = -1, 0.0
    for k in range(len(Tk)):
        c = frame_pos(Tk[k])
        dx, dy, dz = c[0] - pos[0], c[1] - pos[1], c[2] - pos[2]
        dist = float(np.sqrt(dx * dx + dy * dy + dz * dz))
        if dist > maxdist:
            best, maxdist = k, dist
    return best, maxdist


def decision(tables, T_f_w, feat_point, overlap_kf, min_dist):
    """svo_hip_kf_decision as a dict; overlap_kf = None: the overlap list is not valid"""
    n, n_nan, mean, dmin = scene_depth(tables, T_f_w, feat_point)
    pos = frame_pos(T_f_w)
    need, blocking = (-1, -1) if overlap_kf is None else need_new_kf(tables, T_f_w, overlap_kf, mean, min_dist)
    far, dist = furthest_keyframe(tables, pos)
    return dict(n_depths=n, n_nan_depths=n_nan, depth_mean=mean, depth_min=dmin, overlap_valid=0 if overlap_kf is None else 1,
                need_new_kf=need, blocking_kf=blocking, furthest_kf=far, furthest_distance=dist, pos=pos)


def flip_distance(tables, T_f_w, kf, depth_mean):
    """the kf_select_min_dist at which keyframe kf starts to block: the box test holds for d > max of the three scaled ratios
    (as real numbers; the caller probes nextafter on both sides)"""
    r = rel_pos(tables, T_f_w, kf)
    m = np.float64(depth_mean)
    return max(abs(r[0]) / m, abs(r[1]) / m / 0.8, abs(r[2]) / m / 1.3)


# ---- small maps for the furthest keyframe and the depths (identity rotations, translations exact in binary)
def _tables(kf_centres, pt_pos):
    K, P = len(kf_centres), len(pt_pos)
    T = np.zeros((K, 7))
    T[:, 6] = 1.0
    T[:, :3] = -np.asarray(kf_centres, dtype=np.float64).reshape(K, 3)      # identity rotation: pos() = -t, exactly
    i32 = lambda *s: np.zeros(s, np.int32)
    return dict(kf_slot=np.arange(K, dtype=np.int32), T_kf_w=T, kf_key_point=np.full((K, 5), -1, np.int32), kf_ftr_offset=i32(K + 1),
                kf_ftr_point=i32(0), pt_pos=np.asarray(pt_pos, dtype=np.float64).reshape(P, 3), pt_type=np.full(P, 2, np.int32),
                pt_n_failed=i32(P), pt_n_succeeded=i32(P), pt_obs_offset=i32(P + 1), obs_kf=i32(0), obs_px=np.zeros((0, 2)),
                obs_f=np.zeros((0, 3)), obs_level=i32(0), cand_point=i32(0), n_kf=K, n_points=P)


def line_map(n_kf, n_points=1):
    """n_kf keyframes at (0.25 k, 0, 0); the furthest from a frame near the origin is the last one"""
    return _tables([(0.25 * k, 0.0, 0.0) for k in range(n_kf)], np.tile([0.0, 0.0, 2.0], (n_points, 1)))


def tie_map():
    """(tables, T_f_w): keyframes 1 and 3 are both exactly 2 away from the frame at (1, 0, 0): the lower index wins"""
    return _tables([(1.5, 0.0, 0.0), (3.0, 0.0, 0.0), (1.0, 0.5, 0.0), (-1.0, 0.0, 0.0), (1.0, 0.0, 1.0)], [(0.0, 0.0, 2.0)]), \
        np.array([-1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])


def coincident_map():
    """(tables, T_f_w): every keyframe sits at the frame's position: no furthest keyframe"""
    return _tables([(1.0, 0.5, 0.0)] * 3, [(0.0, 0.0, 2.0)]), np.array([-1.0, -0.5, 0.0, 0.0, 0.0, 0.0, 1.0])


DEPTH_KINDS = ("random", "duplicates", "equal", "behind", "nan")


def depth_case(n_with_point, kind, seed=0, max_features=None):
    """(tables, T_f_w, feat_point): n_with_point features with a point, point-less ones interleaved, over a one-keyframe map whose
    point depths follow `kind`.  The frame is rotated and shifted, so every depth goes through the whole se3_act."""
    rng = np.random.default_rng(1000 * n_with_point + 17 * DEPTH_KINDS.index(kind) + seed)
    n = n_with_point
    P = max(n, 1)
    z = rng.uniform(1.0, 4.0, P)
    if kind == "duplicates" and n >= 2:                       # a run of equal depths that straddles the rank, every value repeated
        z = np.round(z * 4.0) / 4.0
        order = np.argsort(z)
        z[order[max(0, n // 2 - 2):n // 2 + 2]] = z[order[n // 2]]
    elif kind == "equal":
        z[:] = 2.5
    elif kind == "behind":
        z = rng.uniform(-3.0, 3.0, P)
    pos_f = np.stack([rng.uniform(-1.0, 1.0, P), rng.uniform(-1.0, 1.0, P), z], axis=1)
    T = synth.se3_from_twist([0.1, -0.2, 0.05], [0.02, -0.03, 0.01]) if kind not in ("duplicates", "equal") else \
        np.array([0.25, -0.5, 0.125, 0.0, 0.0, 0.0, 1.0])     # (identity rotation: equal depths stay equal, exactly)
    Tinv = synth.se3_inv(T)
    pos_w = np.array([synth.se3_act(Tinv, p) for p in pos_f]).reshape(P, 3)
    if kind in ("duplicates", "equal"):
        pos_w[:, 2] = z - T[2]                                # z_f = t_z + z_w exactly, for these binary fractions
    if kind == "nan" and n >= 1:
        pos_w[int(rng.integers(0, n))] = np.nan
    tables = _tables([(0.0, 0.0, 0.0)], pos_w)
    # feature list: the points in a shuffled order, a point-less feature after every third one (as long as there is room)
    pts = list(rng.permutation(n).astype(int))
    feat = []
    for i, p in enumerate(pts):
        feat.append(p)
        if i % 3 == 0 and (max_features is None or len(feat) + (len(pts) - i - 1) < max_features):
            feat.append(-1)
    return tables, T, np.array(feat, dtype=np.int32)


def overlap_families(seed=5):
    """[(name, tables, T_f_w, overlap_kf, depth_mean, min_dist, want (need, blocking))]: both outcomes of needNewKf, each axis
    deciding alone, a block by the first and by a later overlap keyframe, an empty list.  Frame at the origin looking along z with
    a small rotation; depth 2; d = 0.12: the box is |x| < 0.24, |y| < 0.192, |z| < 0.312."""
    rng = np.random.default_rng(seed)
    T = synth.se3_from_twist([0.0, 0.0, 0.0], [0.004, -0.003, 0.002])
    far = (1.0, 1.0, 1.0)
    fams = []

    def add(name, centres, overlap, want):
        centres = [tuple(np.asarray(c) + rng.uniform(-1e-3, 1e-3, 3)) for c in centres]
        fams.append((name, _tables(centres, [(0.0, 0.0, 2.0)]), T, list(overlap), 2.0, 0.12, want))

    add("empty overlap list", [far, far], [], (1, -1))
    add("all outside", [far, (0.5, 0.0, 0.0), (0.0, -0.4, 0.0)], [2, 0, 1], (1, -1))
    add("x decides alone", [(0.26, 0.1, 0.2)], [0], (1, -1))
    add("y decides alone", [(0.1, 0.21, 0.2)], [0], (1, -1))
    add("z decides alone", [(0.1, 0.1, 0.33)], [0], (1, -1))
    add("inside, first blocks", [(0.1, 0.1, 0.2), far], [0, 1], (0, 0))
    add("inside, a later one blocks", [far, (0.26, 0.0, 0.0), (-0.2, 0.15, -0.3), (0.0, 0.0, 0.0)], [0, 1, 2, 3], (0, 2))
    add("order of the list, not of the map", [(0.05, 0.0, 0.0), (0.0, 0.05, 0.0), far], [2, 1, 0], (0, 1))
    return fams
