#!/usr/bin/env python3
"""Diagnostic: wall time of one svo_hip_klt_two_view call, host side included (job table, the two launches, the one synchronisation,
the result blocks), at 400 correspondences x 1024 hypotheses for 1, 8 and 64 cameras.  The lists are the `outliers-400-30-0.0`
family case of tests/two_view_cases.py (status OK, 280 inliers) in every camera.  A run times REPS calls after a warm-up and keeps
their median; the figure of a shape is the median of RUNS runs, with the run medians beside it.  Beside it go the single-core
time of the host twin (tests/host_mock/two_view_twin.cpp, g++ -O2 -ffp-contract=off, the same inline functions) for one camera
on the machine the probe runs on, and the time of svo_hip_klt_track for the same camera counts from profiles/klt_probe.json.
Writes profiles/two_view_probe.json.  `--cpu-only` measures the twin alone (no GPU needed)."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import two_view_cases as TC  # noqa: E402
from test_two_view_twin_cpu import write_case  # noqa: E402

CASE, RUNS, WARM = "outliers-400-30-0.0", 5, 5
SHAPES = [(1, 200), (8, 100), (64, 30)]          # (cameras, timed calls per run)


def twin_ms(case, runs=RUNS):
    """median single-core time of the host twin for one camera, in milliseconds"""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "two_view_twin")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unknown-pragmas",
                               os.path.join(ROOT, "tests", "host_mock", "two_view_twin.cpp"), "-o", exe])
        write_case(os.path.join(tmp, "c.bin"), case)
        args = [exe] + [os.path.join(tmp, "c.bin"), os.path.join(tmp, "r.bin")] * (runs + 1)
        out = subprocess.run(args, capture_output=True, text=True, check=True).stdout
    t = [float(v) for v in re.findall(r"time_ms ([0-9.]+)", out)]
    assert len(t) == runs + 1
    return float(np.median(t[1:])), t[1:]


def main():
    case = TC.case(CASE)
    n = len(case["f_ref"])
    ms, all_ms = twin_ms(case)
    out = dict(case=CASE, correspondences=n, hypotheses=case["params"]["n_hypotheses"], runs=RUNS,
               host_twin=dict(what="tests/host_mock/two_view_twin.cpp, one camera, one core, g++ -O2 -ffp-contract=off", ms_median=ms, ms_runs=all_ms),
               note="time per svo_hip_klt_two_view call in microseconds, host side included")
    if "--cpu-only" in sys.argv:
        print(json.dumps(out))
        return
    from android_svo_amd import hip, synth
    ctx = hip.Context(0)
    cam = hip.make_camera(synth.Camera(TC.W, TC.H, TC.FX, TC.FY, TC.CX, TC.CY))
    pyr = hip.Pyramid(ctx, TC.W, TC.H, 1, 1)
    pyr.upload_level0_and_build(0, np.zeros((TC.H, TC.W), np.uint8))
    try:
        klt_probe = {s["cameras"]: s["call_us_median"] for s in json.load(open(os.path.join(ROOT, "profiles", "klt_probe.json")))["shapes"]}
    except Exception:
        klt_probe = {}
    prm = hip.CTwoViewParams()
    ctx.check(ctx.lib.svo_hip_two_view_default_params(C.byref(prm)), "two_view_default_params")
    out["shapes"] = []
    for n_cams, reps in SHAPES:
        klt = hip.KltTracker(ctx, TC.W, TC.H, n_cams, n)
        for c in range(n_cams):
            klt.set_reference(c, pyr, 0, np.zeros((0, 2), np.float32), np.zeros((0, 3)))
            klt.set_lists(c, case["px_ref"], case["px_cur"], case["f_ref"], case["f_cur"])
        cams_a = (C.c_int * n_cams)(*range(n_cams))
        models, res = (hip.CCamera * n_cams)(*([cam] * n_cams)), (hip.CTwoViewResult * n_cams)()

        def one():
            t0 = time.perf_counter()
            rc = ctx.lib.svo_hip_klt_two_view(klt.h, n_cams, cams_a, models, None, C.byref(prm), res)
            dt = time.perf_counter() - t0
            ctx.check(rc, "klt_two_view")
            return dt * 1e6

        for _ in range(WARM):
            one()
        meds = [float(np.median([one() for _ in range(reps)])) for _ in range(RUNS)]
        assert all(r.status == 0 and r.n_inliers == 280 for r in res)
        us = float(np.median(meds))
        out["shapes"].append(dict(cameras=n_cams, calls_per_run=reps, call_us_median=round(us, 1), call_us_run_medians=[round(m, 1) for m in meds],
                                  us_per_camera=round(us / n_cams, 1), host_twin_us_for_these_cameras=round(ms * 1e3 * n_cams, 1),
                                  klt_track_call_us=klt_probe.get(n_cams)))
        klt.destroy()
    pyr.destroy()
    ctx.close()
    json.dump(out, open(os.path.join(ROOT, "profiles", "two_view_probe.json"), "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
