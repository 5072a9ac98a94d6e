#!/usr/bin/env python3
"""Diagnostic: wall time of svo_hip_tracker_finish_frame (structure step + keyframe decision, one launch, one wait) beside
svo_hip_tracker_optimize_structure for the same 20-point selection, at 120, 1200 and max_frame_features features of the last
frame; the C++ twins doing the same decision on the host; and svo_hip_tracker_group_finish_frames at 8 and 64 cameras beside the
per-camera svo_hip_tracker_optimize_structure loop.  Every figure is the median of individually timed calls after a warm-up; the
calls go through ctypes with buffers made once, so the Python side costs both forms the same.  Prints one JSON document."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from android_svo_amd import hip  # noqa: E402
import tracking_chain as tc  # noqa: E402

WARM, REPS = 50, 1000
MAX_FEAT = 2816
CFG = dict(max_keyframes=4, max_points=2048, max_obs=8192, max_kf_features=4096, max_candidates=256, max_items=1024, grid_size=tc.CELL,
           max_fts=tc.MAX_FTS, klt_min_level=2, max_frame_features=MAX_FEAT)
I32, F64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)


def median_us(call, reps=REPS):
    for _ in range(WARM):
        call()
    t = np.empty(reps)
    for i in range(reps):
        t0 = time.perf_counter()
        call()
        t[i] = time.perf_counter() - t0
    return round(float(np.median(t)) * 1e6, 2), round(float(np.percentile(t, 10)) * 1e6, 2), round(float(np.percentile(t, 90)) * 1e6, 2)


def start(trk, seq, mp, n_feat):
    """the map of the sequence and a last frame of n_feat features, every one with a point (the indices go round)"""
    n = len(seq["px0"])
    idx = np.arange(n_feat) % n
    trk.upload_keyframe(0, seq["pyrs"][0][0])
    trk.set_map(mp)
    trk.set_last_frame(seq["T0"], seq["px0"][idx], seq["f0"][idx], idx.astype(np.int32), kf_slot=0)


def host_twins(seq, mp, counts):
    """the C++ twins' decision (tests/host_mock/keyframe_decision_twin.cpp, -O2) on the same frames: median microseconds"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_keyframe_decision_model as tm
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe, txt = os.path.join(tmp, "twin"), os.path.join(tmp, "cases.txt")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "host_mock", "keyframe_decision_twin.cpp"), "-o", exe, "-lpthread"])
        n = len(seq["px0"])
        with open(txt, "w") as fh:
            for c in counts:
                tm._write_case(fh, "features_%d" % c, mp, seq["T0"], np.arange(c) % n, [0], 2.0, 0.12)
        r = subprocess.run([exe, txt, "2000"], capture_output=True, text=True, check=True)
        for line in r.stdout.split("\n")[:-1]:
            w = line.split()
            out[w[0]] = float(w[-1])
    return out


def main():
    ctx = hip.Context(0)
    lib = ctx.lib
    seq = tc.make_sequence(n_frames=3, n_map=600)
    mp = tc.sequence_map(seq)
    sel = np.arange(20, dtype=np.int32) * 7
    pos, it = np.zeros((64, 3)), np.zeros(64, np.int32)
    dec = hip.CKfDecision()
    out = {"what": "median (p10, p90) microseconds per call", "reps": REPS, "lone": {}, "group": {}}
    counts = (120, 1200, MAX_FEAT)
    for n_feat in counts:
        trk = hip.Tracker(ctx, seq["cam"], **CFG)
        start(trk, seq, mp, n_feat)
        structure = lambda: lib.svo_hip_tracker_optimize_structure(trk.h, 20, sel.ctypes.data_as(I32), 5, pos.ctypes.data_as(F64), it.ctypes.data_as(I32))
        finish = lambda: lib.svo_hip_tracker_finish_frame(trk.h, 20, sel.ctypes.data_as(I32), 5, pos.ctypes.data_as(F64), it.ctypes.data_as(I32),
                                                         C.c_double(0.12), C.byref(dec))
        decide = lambda: lib.svo_hip_tracker_finish_frame(trk.h, 0, None, 5, None, None, C.c_double(0.12), C.byref(dec))
        assert structure() == 0 and finish() == 0 and decide() == 0
        out["lone"]["features_%d" % n_feat] = {"optimize_structure": median_us(structure), "finish_frame": median_us(finish),
                                               "finish_frame_without_structure_step": median_us(decide), "n_depths": int(dec.n_depths),
                                               "iterations_of_the_first_points": it[:5].tolist()}
        trk.destroy()
    # after a tracked frame: the overlap list is valid
    trk = hip.Tracker(ctx, seq["cam"], **CFG)
    start(trk, seq, mp, len(seq["px0"]))
    r = trk.track(seq["pyrs"][1][0])
    s2 = np.array([int(p) for p in r["feat_point"] if p >= 0][:20], np.int32)
    structure = lambda: lib.svo_hip_tracker_optimize_structure(trk.h, len(s2), s2.ctypes.data_as(I32), 5, pos.ctypes.data_as(F64), it.ctypes.data_as(I32))
    finish = lambda: lib.svo_hip_tracker_finish_frame(trk.h, len(s2), s2.ctypes.data_as(I32), 5, pos.ctypes.data_as(F64), it.ctypes.data_as(I32),
                                                     C.c_double(0.12), C.byref(dec))
    out["lone"]["tracked_frame"] = {"optimize_structure": median_us(structure), "finish_frame": median_us(finish), "n_depths": int(dec.n_depths),
                                    "overlap_valid": int(dec.overlap_valid), "need_new_kf": int(dec.need_new_kf)}
    trk.destroy()
    out["host_twins_decision_only"] = host_twins(seq, mp, counts)
    for n_cams in (8, 64):
        grp = hip.TrackerGroup(ctx, seq["cam"], n_cams, **dict(CFG, max_frame_features=1024))
        for cam in grp.cameras:
            start(cam, seq, mp, len(seq["px0"]))
        req = (hip.CStructureRequest * n_cams)()
        bufs = [(np.zeros((64, 3)), np.zeros(64, np.int32)) for _ in range(n_cams)]
        for c in range(n_cams):
            req[c] = hip.CStructureRequest(20, sel.ctypes.data_as(I32), 5, bufs[c][0].ctypes.data_as(F64), bufs[c][1].ctypes.data_as(I32))
        decs, ok = (hip.CKfDecision * n_cams)(), (C.c_int32 * n_cams)()
        handles = [cam.h for cam in grp.cameras]

        def loop():
            for c in range(n_cams):
                lib.svo_hip_tracker_optimize_structure(handles[c], 20, sel.ctypes.data_as(I32), 5, bufs[c][0].ctypes.data_as(F64), bufs[c][1].ctypes.data_as(I32))
        group = lambda: lib.svo_hip_tracker_group_finish_frames(grp.h, req, C.c_double(0.12), decs, ok)
        assert group() == 0 and all(ok)
        a, b = median_us(loop, 300), median_us(group, 300)
        out["group"]["cameras_%d" % n_cams] = {"optimize_structure_loop": a, "group_finish_frames": b, "ratio_of_medians": round(a[0] / b[0], 2)}
        grp.destroy()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
