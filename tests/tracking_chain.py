"""The per-frame data path of FrameHandlerMono::processFrame (S/frame_handler_mono.cpp:171-244) as a chain over a synthetic
sequence, with pluggable stages (HIP or oracle); shared by tests/test_gpu_sequence.py and tests/test_oracle_sequence.py.

    new_frame.T_f_w = last_frame.T_f_w                                   (:175)
    SparseImgAlign(kltMaxLevel=4, kltMinLevel, 30).run(last_frame, new)  (:186-188)   last frame's features = what the
                                                                                      reprojector created in it (:217-223)
    Reprojector::reprojectMap: map points of the keyframe into the grid, one match per cell (reprojector.cpp:149-241)
    pose_optimizer::optimizeGaussNewton on the matched features          (:226-229)
(optimizeStructure is left out: with one keyframe every point has a single observation, nothing to refine.)"""
import numpy as np

from android_svo_amd import synth

CELL = 30           # Config::gridSize()
MAX_FTS = 120       # Config::maxFts()


def make_sequence(n_frames=20, n_map=600, orbit=False, width=640, height=480, focal=None, border=48):
    """orbit: instead of moving on, the camera walks the first 20 poses of the path back and forth (0 .. 19 .. 0 .. 19 ...), so
    that a sequence of any length keeps the keyframe's map in view.
    width, height, focal: the camera (focal None: synth.Camera.default's); border: how far from the image border the map's
    features in keyframe 0 stay."""
    rng = np.random.default_rng(2024)
    cam = synth.Camera.default(width, height)
    if focal is not None:
        cam.fx = cam.fy = float(focal)
    scene = synth.PlaneScene(seed=77, depth=2.2, tilt=(0.06, -0.04))
    T0 = synth.se3_from_twist([0.01, -0.02, 0.0], [0.004, -0.003, 0.002])
    step_t, step_r = np.array([0.012, 0.004, -0.003]), np.array([0.0015, -0.0025, 0.002])
    truth = [T0]
    for _ in range(1, min(n_frames, 20) if orbit else n_frames):
        wob = rng.uniform(-0.002, 0.002, 3)
        truth.append(synth.se3_mul(synth.se3_from_twist(step_t + wob, step_r + 0.2 * wob), truth[-1]))
    if orbit:
        path = truth
        idx = []
        for k in range(n_frames):
            r = k % 38
            idx.append(r if r <= 19 else 38 - r)
        base = [synth.build_pyramid(scene.render(cam, T)) for T in path]
        truth = [path[j] for j in idx]
        pyrs = [base[j] for j in idx]
    if not orbit:
        pyrs = [synth.build_pyramid(scene.render(cam, T)) for T in truth]
    px0 = synth.grid_features(cam, n_map, rng, border=border)      # the map: points seen in keyframe 0
    f0 = synth.cam2world(cam, px0)
    pos = scene.intersect(cam, T0, px0[:, 0], px0[:, 1])
    return dict(cam=cam, truth=truth, pyrs=pyrs, px0=px0, f0=f0, pos=pos, T0=T0)


def project(cam, T, pos):
    Xc = np.stack([synth.se3_act(T, p) for p in pos])
    return np.stack([cam.fx * Xc[:, 0] / Xc[:, 2] + cam.cx, cam.fy * Xc[:, 1] / Xc[:, 2] + cam.cy], axis=1)


def cells(cam, px_pred):
    """Reprojector::reprojectPoint: points whose projection is at least 8 px inside the image, bucketed by grid cell in
    map order (reprojector.cpp:246-259)."""
    gc, gr = -(-cam.width // CELL), -(-cam.height // CELL)
    pxi = px_pred.astype(np.int64)
    inside = (pxi[:, 0] >= 8) & (pxi[:, 0] < cam.width - 8) & (pxi[:, 1] >= 8) & (pxi[:, 1] < cam.height - 8)
    cell = (px_pred[:, 1] / CELL).astype(np.int64) * gc + (px_pred[:, 0] / CELL).astype(np.int64)
    idx = np.where(inside)[0]
    lists = [idx[cell[idx] == c] for c in range(gc * gr)]
    off = np.zeros(gc * gr + 1, dtype=np.int32)
    for c, r in enumerate(lists):
        off[c + 1] = off[c] + len(r)
    ids = np.concatenate(lists) if off[-1] else np.zeros(0, dtype=np.int64)
    return off, ids.astype(np.int64)


def run_chain(seq, stages, min_level, perturb_each_frame=0.0):
    """stages: object with align(fp, k, min_level) -> (T, n_tracked); reproject(k, T_sia, off, ids, px_pred) -> dict;
    refine(T_sia, f, pos, level, hp) -> (T, hp_out).  Returns per-frame poses, match counts and matched point ids."""
    cam, truth, pyrs, px0, f0, pos, T0 = (seq[k] for k in ("cam", "truth", "pyrs", "px0", "f0", "pos", "T0"))
    T = T0.copy()
    px, f, p3 = px0.copy(), f0.copy(), pos.copy()
    poses, n_matches, winners = [], [], []
    for k in range(1, len(truth)):
        n = len(px)
        fp = synth.FramePair(cam, pyrs[k - 1], pyrs[k], px, f, p3, np.ones(n, dtype=np.uint8), T, truth[k], T)   # init = last pose (:175)
        T_sia, n_tracked = stages.align(fp, k, min_level)
        assert n_tracked > 50
        px_pred = project(cam, T_sia, pos)
        off, ids = cells(cam, px_pred)
        res = stages.reproject(k, T_sia, off, ids, px_pred)
        win = res["cell_winner"][res["cell_winner"] >= 0]
        assert len(win) >= 50                                              # Config::qualityMinFts()
        px_m, sl = res["px_cur"][win], res["search_level"][win].astype(np.int32)
        f_m = synth.cam2world(cam, px_m)
        T_new, hp_out = stages.refine(T_sia, f_m, pos[ids[win]], sl, np.ones(len(win), dtype=np.uint8))
        keep = hp_out.astype(bool)
        assert keep.sum() >= 20                                            # sfba_n_edges_final (:231)
        T = np.array(T_new)
        T[0] += perturb_each_frame                                         # sensitivity probe: disturb the handed-over pose
        px, f, p3 = px_m[keep], f_m[keep], pos[ids[win]][keep]
        poses.append(T.copy())
        n_matches.append(int(res["n_matches"]))
        winners.append(ids[win][keep])
    return poses, n_matches, winners


class OracleStages:
    def __init__(self, seq):
        from oracle import orc
        self.orc, self.seq = orc, seq
        self.zeros = np.zeros(len(seq["px0"]), dtype=np.int32)

    def align(self, fp, k, min_level):
        o = self.orc.sparse_img_align(fp, max_level=4, min_level=min_level, n_iter=30, early_stop=True)
        return np.array(o.T_cur_w), o.n_tracked

    def reproject(self, k, T_sia, off, ids, px_pred):
        s = self.seq
        z = self.zeros[ids]
        return self.orc.reproject_cells(s["cam"], [s["pyrs"][0]], s["T0"][None, :], s["pyrs"][k], T_sia, off, z, s["px0"][ids], s["f0"][ids], z,
                                        s["pos"][ids], np.zeros(len(ids), np.uint8), np.tile([1.0, 0.0], (len(ids), 1)),
                                        np.zeros(len(ids), np.uint8), px_pred[ids], max_fts=MAX_FTS)

    def refine(self, T_sia, f, pos, level, hp):
        r, hp_out = self.orc.pose_optimize(abs(self.seq["cam"].fx), T_sia, f, pos, level, hp)
        return np.array(r.T_f_w), hp_out


# ---- the same chain through the whole-frame entry (svo_hip_tracker_track) and its oracle composition ---------------------
def sequence_map(seq):
    """The map of make_sequence as the index tables the tracker / orc.reproject_map take: ONE keyframe (frame 0) whose
    features are the map points in map order, one observation per point, no candidates."""
    cam, px0, f0, pos = seq["cam"], seq["px0"], seq["f0"], seq["pos"]
    n = len(px0)
    key_ftr = synth.key_points(cam, px0, np.ones(n, bool))
    return dict(cam=cam, cell_size=CELL, n_kf=1, n_points=n, kf_pyr=[seq["pyrs"][0]], kf_slot=np.zeros(1, np.int32), T_kf_w=seq["T0"][None, :].copy(),
                kf_key_point=key_ftr[None, :].copy(),          # feature index == point index here
                kf_ftr_offset=np.array([0, n], np.int32), kf_ftr_point=np.arange(n, dtype=np.int32), pt_pos=pos.copy(),
                pt_type=np.full(n, synth.TYPE_UNKNOWN, np.int32), pt_n_failed=np.zeros(n, np.int32), pt_n_succeeded=np.zeros(n, np.int32),
                pt_obs_offset=np.arange(n + 1, dtype=np.int32), obs_kf=np.zeros(n, np.int32), obs_px=px0.copy(), obs_f=f0.copy(),
                obs_level=np.zeros(n, np.int32), obs_edgelet=np.zeros(n, np.uint8), obs_grad=np.tile([1.0, 0.0], (n, 1)),
                cand_point=np.zeros(0, np.int32))


def oracle_track_frame(orc, mp, state, last, last_pyr, cur_pyr, min_level, max_fts=MAX_FTS, quality_min_fts=40):
    """One frame of FrameHandlerMono::processFrame (:175-229) composed from the oracle's pieces; `last` = dict(T, px, f,
    point) of the previous frame, `state` = the map's point counters (updated in place).  Returns the same dict layout
    as hip.Tracker.track."""
    cam = mp["cam"]
    pt = last["point"]
    pos = np.where(pt[:, None] >= 0, mp["pt_pos"][np.maximum(pt, 0)], np.array([0.0, 0.0, 1.0]))
    fp = synth.FramePair(cam, last_pyr, cur_pyr, last["px"], last["f"], pos, (pt >= 0).astype(np.uint8), last["T"], last["T"], last["T"])
    o = orc.sparse_img_align(fp, max_level=4, min_level=min_level, n_iter=30, early_stop=True)
    T_sia = np.array(o.T_cur_w)
    cs = dict(mp, cur_pyr=cur_pyr)
    r = orc.reproject_map(cs, mp["kf_key_point"], T_cur_w=T_sia, max_fts=max_fts, state=state)
    # Feature(frame, px, level): f = cam2world(px).  (synth.cam2world is the vectorised form of the oracle's: equal bit for bit)
    f_m = synth.cam2world(cam, r["feat_px"]) if len(r["feat_px"]) else np.zeros((0, 3))
    out = dict(r, T_f_w_sia=T_sia, feat_f=f_m, sia_n_tracked=o.n_tracked)
    if r["n_matches"] < quality_min_fts:
        out["T_f_w"] = np.array(last["T"])
        return out
    po, hp = orc.pose_optimize(abs(cam.fx), T_sia, f_m, mp["pt_pos"][r["feat_point"]], r["feat_level"], np.ones(len(f_m), np.uint8))
    out["T_f_w"] = np.array(po.T_f_w)
    out["feat_point"] = np.where(hp.astype(bool), r["feat_point"], -1).astype(np.int32)
    out["pose"] = po
    return out


def run_tracker_chain(seq, track, min_level, stop_when_lost=False):
    """track(k, last) -> result dict (hip.Tracker.track layout) for frame k; the chain feeds on its own outputs.
    stop_when_lost: end the chain (instead of failing) at the frame processFrame would report RESULT_FAILURE for."""
    last = dict(T=seq["T0"].copy(), px=seq["px0"].copy(), f=seq["f0"].copy(), point=np.arange(len(seq["px0"]), dtype=np.int32))
    poses, n_matches, winners, feats = [], [], [], []
    for k in range(1, len(seq["truth"])):
        r = track(k, last)
        keep = r["feat_point"] >= 0
        if stop_when_lost and (r["n_matches"] < 50 or keep.sum() < 20):
            break
        assert r["n_matches"] >= 50                                        # Config::qualityMinFts()
        assert keep.sum() >= 20                                            # sfba_n_edges_final (:231)
        last = dict(T=r["T_f_w"].copy(), px=r["feat_px"], f=r["feat_f"], point=r["feat_point"])
        poses.append(r["T_f_w"].copy())
        n_matches.append(int(r["n_matches"]))
        winners.append(r["feat_point"][keep])
        feats.append(r["feat_px"].copy())
    return poses, n_matches, winners, feats


def map_with_tracked_frame_as_keyframe(seq, mp, r):
    """sequence_map grown by one keyframe: the tracked frame of result r (hip.Tracker.track layout) becomes keyframe 1
    (FrameHandlerMono::processFrame :284-330: setKeyframe, point->addFrameRef(feature) for every feature with a point,
    map_.addKeyframe).  Its features with a point are new observations of those points, pushed to the FRONT of Point::obs_
    (S/point.cpp:52-55); point numbering and counters as the frame left them."""
    cam = seq["cam"]
    n = len(seq["px0"])
    keep = r["feat_point"] >= 0
    kp, kpx, kf_, klv = r["feat_point"][keep], r["feat_px"][keep], r["feat_f"][keep], r["feat_level"][keep]
    obs_kf, obs_px, obs_f, obs_level, off = [], [], [], [], [0]
    new_obs_of = {int(p): i for i, p in enumerate(kp)}
    for p in range(n):
        if p in new_obs_of:
            i = new_obs_of[p]
            obs_kf.append(1); obs_px.append(kpx[i]); obs_f.append(kf_[i]); obs_level.append(int(klv[i]))
        obs_kf.append(0); obs_px.append(seq["px0"][p]); obs_f.append(seq["f0"][p]); obs_level.append(0)
        off.append(len(obs_kf))
    key1 = synth.key_points(cam, kpx, np.ones(len(kp), bool))
    return dict(mp, n_kf=2, kf_slot=np.array([0, 1], np.int32), T_kf_w=np.stack([seq["T0"], r["T_f_w"]]),
                kf_key_point=np.stack([mp["kf_key_point"][0], np.where(key1 >= 0, kp[np.maximum(key1, 0)], -1)]).astype(np.int32),
                kf_ftr_offset=np.array([0, n, n + len(kp)], np.int32), kf_ftr_point=np.concatenate([np.arange(n), kp]).astype(np.int32),
                pt_type=r["type"], pt_n_failed=r["n_failed"], pt_n_succeeded=r["n_succeeded"],
                pt_obs_offset=np.array(off, np.int32), obs_kf=np.array(obs_kf, np.int32), obs_px=np.array(obs_px), obs_f=np.array(obs_f),
                obs_level=np.array(obs_level, np.int32), obs_edgelet=np.zeros(len(obs_kf), np.uint8), obs_grad=np.tile([1.0, 0.0], (len(obs_kf), 1)))

