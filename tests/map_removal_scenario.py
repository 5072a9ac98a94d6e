"""The map cases the keyframe-removal tests share (tests/test_map_removal_model.py on the CPU, tests/test_gpu_map_removal.py on the
device): a small map of five keyframes every one of which is removed in turn, the "wide" case of tests/test_oracle_reproject_map.py
(nine keyframes, the key points the reference's own code chose) with keyframes 1 and 6 removed, and a hand-made map of two
keyframes with integer pixels on which the reference's and the device's re-selection rules differ in one slot.  320 x 240 images."""
import numpy as np

from android_svo_amd import synth
from test_oracle_reproject_map import CASES, GOLD

REMOVALS = tuple(("small", k) for k in range(5)) + (("wide", 1), ("wide", 6))


def fresh_key_points(cs):
    """Frame::setKeyPoints from five empty slots on every keyframe of a synth.make_map_case map, as point indices"""
    out = []
    for j in range(cs["n_kf"]):
        o = cs["kf_ftr_obs"][cs["kf_ftr_offset"][j]:cs["kf_ftr_offset"][j + 1]]
        e = synth.key_points(cs["cam"], cs["obs_px"][o], np.ones(len(o), bool))
        out.append(np.where(e >= 0, cs["obs_point"][o][np.maximum(e, 0)], -1))
    return np.array(out, np.int32).reshape(-1, 5)


def small_case():
    cs = synth.make_map_case(seed=33, n_kf=5, n_points=300, n_candidates=40, cell_size=20)
    return dict(cs, kf_slot=np.arange(cs["n_kf"], dtype=np.int32), kf_key_point=fresh_key_points(cs))


def wide_args():
    return [c for c in CASES if c[0] == "wide"][0]


def wide_case():
    tag, kw, _ = wide_args()
    cs = synth.make_map_case(**kw)
    return dict(cs, kf_slot=np.arange(cs["n_kf"], dtype=np.int32), kf_key_point=np.load(GOLD)[tag + "_kf_key_point"].astype(np.int32))


def tie_case():
    """Keyframe 0 sees four points, all in the lower right quadrant (cu, cv = 160, 120), in fts_ order:
        0  (170, 180)  product 600                       seen by keyframe 0 only
        1  (190, 140)  product 600, the incumbent of slot 1, closest to the centre but for point 3
        2  (200, 150)  product 1200                      seen by keyframes 0 and 1: deleted with keyframe 1, second
        3  (161, 121)  the incumbent of slot 0           seen by keyframes 0 and 1: deleted with keyframe 1, first
    Removing keyframe 1 deletes 3, then 2.  The reference chooses again at each: after 3, point 2 takes slot 1 from the living
    incumbent 1; after 2, the empty slot goes to the first of the tied 0 and 1, which is 0.  Choosing once, afterwards, leaves
    the incumbent 1 in its slot: the tie with 0 does not unseat it."""
    cam = synth.Camera(320, 240, 250.0, 250.0, 159.5, 119.5)
    px0 = np.array([[170, 180], [190, 140], [200, 150], [161, 121]], np.float64)
    px1 = np.array([[150, 100], [141, 90]], np.float64)                  # points 2 and 3 in keyframe 1
    T = np.array([[0, 0, 0, 0, 0, 0, 1], [0.1, 0, 0, 0, 0, 0, 1]], np.float64)
    obs_px = np.array([px0[0], px0[1], px1[0], px0[2], px1[1], px0[3]])  # newest observation first
    obs_kf = np.array([0, 0, 1, 0, 1, 0], np.int32)
    f0 = synth.cam2world(cam, px0)
    n_obs = len(obs_kf)
    return dict(cam=cam, cell_size=20, n_kf=2, n_points=4, kf_slot=np.array([0, 1], np.int32), T_kf_w=T,
                kf_key_point=np.array([[3, 1, -1, -1, -1], [3, 2, -1, -1, -1]], np.int32), kf_ftr_offset=np.array([0, 4, 6], np.int32),
                kf_ftr_point=np.array([0, 1, 2, 3, 3, 2], np.int32), pt_pos=2.0 * f0 / f0[:, 2:3],
                pt_type=np.full(4, synth.TYPE_UNKNOWN, np.int32), pt_n_failed=np.zeros(4, np.int32), pt_n_succeeded=np.zeros(4, np.int32),
                pt_obs_offset=np.array([0, 1, 2, 4, 6], np.int32), obs_kf=obs_kf, obs_px=obs_px, obs_f=np.ascontiguousarray(synth.cam2world(cam, obs_px)),
                obs_level=np.zeros(n_obs, np.int32), obs_edgelet=np.zeros(n_obs, np.uint8), obs_grad=np.tile([1.0, 0.0], (n_obs, 1)),
                cand_point=np.zeros(0, np.int32))
