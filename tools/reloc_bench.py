#!/usr/bin/env python3
"""Time of one relocalisation against a keyframe of the device map, two ways, on the scenario of tests/test_gpu_relocalise.py
(tracking_chain's sequence: frames 1-3, frame 3 promoted, frames 4-5, frame 6 relocalised from frame 5's pose, accepted):

    relocalize   svo_hip_tracker_relocalize: keyframe choice, gate and the tracked frame in one call, nothing flattened
    composed     what the older entry points allow: the keyframe's features flattened on the host (here the numpy model, timed
                 on its own: a C++ host walks fts_ instead), svo_hip_tracker_set_last_frame from the keyframe's slot, a separate
                 SparseImgAlign solver with its own pyramids for the gate, svo_hip_tracker_track

Medians over --repeat calls after --warmup.  Diagnostic; not run by the driver.  Prints one JSON line.

    python tools/reloc_bench.py [--repeat 25] [--warmup 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import relocalise_reference as rl  # noqa: E402
import tracking_chain as tc  # noqa: E402
from android_svo_amd import hip, synth  # noqa: E402

CFG = dict(max_keyframes=4, grid_size=tc.CELL, max_fts=tc.MAX_FTS, klt_min_level=2, max_frame_features=1024)


def lead(ctx, seq):
    trk = hip.Tracker(ctx, seq["cam"], **CFG)
    n = len(seq["px0"])
    trk.upload_keyframe(0, seq["pyrs"][0][0])
    trk.set_map(tc.sequence_map(seq))
    trk.set_last_frame(seq["T0"], seq["px0"], seq["f0"], np.arange(n, dtype=np.int32), kf_slot=0)
    rs = [trk.track(seq["pyrs"][k][0]) for k in (1, 2, 3)]
    trk.promote_last_frame(1)
    rs += [trk.track(seq["pyrs"][k][0]) for k in (4, 5)]
    return trk, rs


def median_us(fn, repeat, warmup):
    ts = []
    for i in range(warmup + repeat):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(ts[warmup:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    ctx = hip.Context(0)
    seq = tc.make_sequence(n_frames=8, n_map=600)
    cam, img6 = seq["cam"], seq["pyrs"][6][0]
    # ---- one call
    x, rs = lead(ctx, seq)
    T5 = rs[-1]["T_f_w"].copy()
    first = x.relocalize(img6, T5)
    assert first["reloc"].accepted == 1
    t_call = median_us(lambda: x.relocalize(img6, T5, want_points=False), a.repeat, a.warmup)
    # ---- the composed path (the keyframe the model chooses on the tables as they were after frame 5)
    y, rs = lead(ctx, seq)
    tables = dict(y.download_map(), cam=cam)
    unl = rs[-1]["type"] == synth.TYPE_DELETED
    kf = rl.closest_keyframe(tables, T5)["kf_index"]
    assert kf == first["reloc"].kf_index
    t_flatten = median_us(lambda: rl.last_frame_from_keyframe(tables, kf, unl), 5, 1)
    ft = rl.last_frame_from_keyframe(tables, kf, unl)
    ref, cur = hip.Pyramid(ctx, cam.width, cam.height, 5, 1), hip.Pyramid(ctx, cam.width, cam.height, 5, 1)
    ref.upload_level0_and_build(0, seq["pyrs"][(0, 3)[kf]][0])
    sia = hip.SparseImgAlign(ctx, 1, CFG["max_frame_features"])
    sia.set_frames(ref, cur)
    n = len(ft["point"])
    fp = synth.FramePair(cam, None, None, ft["px"], ft["f"], tables["pt_pos"][ft["point"]], np.ones(n, np.uint8), ft["T_f_w"], T5, T5)
    prm = sia.params(max_level=4, min_level=2, n_iter=30, eps=1e-6, early_stop=True)
    slot = int(tables["kf_slot"][kf])

    def composed():
        y.set_last_frame(ft["T_f_w"], ft["px"], ft["f"], ft["point"], kf_slot=slot)
        cur.upload_level0_and_build(0, img6)
        sia.upload_pair(0, fp)
        sia.run(1, prm)
        if sia.download(0).n_tracked > 30:
            y.track(img6, want_points=False)
    t_comp = median_us(composed, a.repeat, a.warmup)
    print(json.dumps({"bench": "relocalise", "repeat": a.repeat, "relocalize_us": round(t_call, 1), "composed_device_calls_us": round(t_comp, 1),
                      "host_flatten_numpy_us": round(t_flatten, 1), "n_features": n, "gate_n_tracked": int(first["reloc"].gate_n_tracked)}))
    for o in (sia, ref, cur, x, y):
        o.destroy()
    ctx.close()


if __name__ == "__main__":
    main()
