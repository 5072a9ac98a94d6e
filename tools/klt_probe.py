#!/usr/bin/env python3
"""Diagnostic: wall time of one svo_hip_klt_track call, host side included (job table, launches, the one synchronisation, the
result blocks), for 1, 8 and 64 cameras x 400 features at 640 x 480.  Every timed call is the first frame after a reference:
the references are set again (untimed) before it, so the tracker starts from zero flow on an image whose content has moved by
(3.3, 2.6) px and runs its real iteration counts.  A run times REPS such calls after a warm-up and keeps their median; the
figure of a shape is the median of RUNS runs, with the spread of the run medians beside it.  Writes profiles/klt_probe.json.

No CPU Lucas-Kanade is measured beside it: OpenCV is not available where this library is developed, so the figures stand alone
(they are NOT a speed-up)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from android_svo_amd import hip, synth  # noqa: E402
import klt_reference as K  # noqa: E402

W, H, N_FEAT, RUNS, WARM = 640, 480, 400, 5, 5
SHAPES = [(1, 200), (8, 100), (64, 30)]          # (cameras, timed calls per run)


def main():
    ctx = hip.Context(0)
    prev, cur = K.sinusoid_texture(W, H, 3), K.sinusoid_texture(W, H, 3, (3.3, 2.6))
    rng = np.random.RandomState(5)
    px = np.stack([rng.uniform(20, W - 21, N_FEAT), rng.uniform(20, H - 21, N_FEAT)], axis=1).astype(np.float32)
    f = synth.cam2world(synth.Camera.default(W, H), px.astype(np.float64))
    pyr = hip.Pyramid(ctx, W, H, 1, 2)
    pyr.upload_level0_batch_and_build(0, [prev, cur])
    cam = hip.make_camera(synth.Camera.default(W, H))
    out = dict(width=W, height=H, features_per_camera=N_FEAT, runs=RUNS, shapes=[],
               note="time per svo_hip_klt_track call in microseconds, host side included; unmeasured against any CPU LK")
    for n_cams, reps in SHAPES:
        klt = hip.KltTracker(ctx, W, H, n_cams, N_FEAT)
        cams_a, slots_a = (C.c_int * n_cams)(*range(n_cams)), (C.c_int * n_cams)(*([1] * n_cams))
        models, res = (hip.CCamera * n_cams)(*([cam] * n_cams)), (hip.CKltResult * n_cams)()

        def one():
            for c in range(n_cams):
                klt.set_reference(c, pyr, 0, px, f)
            t0 = time.perf_counter()
            rc = ctx.lib.svo_hip_klt_track(klt.h, n_cams, cams_a, pyr.h, slots_a, models, res)
            dt = time.perf_counter() - t0
            ctx.check(rc, "klt_track")
            return dt
        medians = []
        for _ in range(RUNS):
            for _ in range(WARM):
                one()
            medians.append(float(np.median([one() for _ in range(reps)])) * 1e6)
        tracked = [r.n_tracked for r in res]
        out["shapes"].append(dict(cameras=n_cams, calls_per_run=reps, call_us_median=round(float(np.median(medians)), 1),
                                  call_us_run_medians=[round(m, 1) for m in medians],
                                  us_per_camera=round(float(np.median(medians)) / n_cams, 1), n_tracked=[min(tracked), max(tracked)]))
        klt.destroy()
    pyr.destroy()
    ctx.close()
    path = os.path.join(ROOT, "profiles", "klt_probe.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
