"""What the depth filter's pass costs a host with MANY cameras: N cameras x 3 batches x 300 seeds, 640x480, no keyframe frames,
host-side time per frame set with the collects included, of
  (a) the loop of svo_hip_seed_batch_update_group_async + collects per camera, and
  (b) the one svo_hip_seed_batch_update_cameras_async call + collects, at the default small-pass limit (8192 records: the
      six-launch form from 8 cameras on) and with the limit at 16 384 (the two-launch form still at 8 cameras).
Median of 200 frame sets after 20 warm-ups; one process per leg, the legs alternating; leg (a) also on another build of the
library (the parent commit's: --parent-lib, through SVO_HIP_LIB).  -> profiles/r18_df_cameras_probe.json

  python tools/df_cameras_probe.py [--parent-lib build/libsvo_hip_parent.so] [--rounds 3] [--out profiles/r18_df_cameras_probe.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAMERAS = (1, 8, 64)
N_BATCHES, N_SEEDS, WARM, SETS = 3, 300, 20, 200
N_SCENES = 4                    # distinct scenes, reused round the cameras (the timing does not depend on which image a slot holds)


def leg(which, n_cams):
    import numpy as np
    from android_svo_amd import hip, seedsynth
    ctx = hip.Context(0)
    scenes = [seedsynth.make_multi_keyframe_case((N_SEEDS,) * N_BATCHES, seed=50 + s) for s in range(min(N_SCENES, n_cams))]
    cam = scenes[0].cam
    kf = hip.Pyramid(ctx, 640, 480, 5, n_cams * N_BATCHES)
    cf = hip.Pyramid(ctx, 640, 480, 5, n_cams)
    batches, slots, T_refs, T_curs = [], [], [], []
    for c in range(n_cams):
        mk = scenes[c % len(scenes)]
        cf.upload(c, mk.cur_pyr)
        for k, sc in enumerate(mk.keyframes):
            kf.upload(c * N_BATCHES + k, sc.ref_pyr)
        # the constructor's variance; most seeds converge or turn NaN within the first sets (seeds_alive_at_end is recorded: the
        # legs end alike), so the figure is that of a launch- and collect-bound pass
        batches.append([hip.ResidentSeeds(ctx, sc.px, sc.f, sc.level, sc.a, sc.b, sc.mu, sc.z_range, sc.sigma2) for sc in mk.keyframes])
        slots.append([c * N_BATCHES + k for k in range(N_BATCHES)])
        T_refs.append(np.stack([sc.T_ref_w for sc in mk.keyframes]))
        T_curs.append(mk.T_cur_w)

    def per_camera():
        for c in range(n_cams):
            hip.ResidentSeeds.update_group_async(batches[c], kf, slots[c], cf, c, cam, T_refs[c], T_curs[c])
            for r in batches[c]:
                r.collect_raw()

    passes = [(batches[c], slots[c], T_refs[c], c, T_curs[c], False) for c in range(n_cams)]

    def one_call():
        hip.ResidentSeeds.update_cameras_async(passes, kf, cf, cam)
        for b in batches:
            for r in b:
                r.collect_raw()

    if which == "b16k":
        ctx.set_small_pass_limit(16384)       # the two-launch form wherever the pass has at most 16 384 records (8 cameras: 12 288)
    fn = per_camera if which == "a" else one_call
    for _ in range(WARM):
        fn()
    ts = []
    for _ in range(SETS):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    alive = sum(r.n_alive() for b in batches for r in b)
    print(json.dumps({"leg": which, "cameras": n_cams, "median_us": 1e6 * ts[len(ts) // 2], "best_us": 1e6 * ts[0],
                      "p90_us": 1e6 * ts[int(0.9 * len(ts))], "seeds_alive_at_end": alive, "lib": hip.LIB_PATH}), flush=True)


def child(which, n_cams, lib):
    env = dict(os.environ)
    env.pop("SVO_HIP_LIB", None)
    if lib:
        env["SVO_HIP_LIB"] = os.path.abspath(lib)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", which, "--cameras", str(n_cams)], env=env, capture_output=True,
                       text=True, timeout=280)
    if r.returncode != 0:
        raise SystemExit("leg %s with %d cameras failed (%d):\n%s" % (which, n_cams, r.returncode, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("a", "b", "b16k"))
    ap.add_argument("--cameras", type=int, default=8)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_df_cameras_probe.json"))
    args = ap.parse_args()
    if args.leg:
        leg(args.leg, args.cameras)
        return
    legs = [("a_loop_per_camera", "a", None), ("b_one_call", "b", None), ("b_one_call_small_pass_limit_16384", "b16k", None)]
    if args.parent_lib:
        legs.append(("a_loop_per_camera_parent_library", "a", args.parent_lib))
    result = {"what": "host-side us per frame set (collects included), %d batches x %d seeds per camera, 640x480, no keyframe frames; "
                      "median of %d sets after %d warm-ups per process, %d processes per leg, legs alternating" %
                      (N_BATCHES, N_SEEDS, SETS, WARM, args.rounds), "cameras": {}}
    for n in CAMERAS:
        runs = {name: [] for name, _, _ in legs}
        for _ in range(args.rounds):
            for name, which, lib in legs:
                runs[name].append(child(which, n, lib))
        row = {}
        for name, rs in runs.items():
            med = sorted(r["median_us"] for r in rs)
            row[name] = {"process_medians_us": [round(r["median_us"], 1) for r in rs], "median_us": round(med[len(med) // 2], 1),
                         "best_us": round(min(r["best_us"] for r in rs), 1),
                         "seeds_alive_at_end": sorted({r["seeds_alive_at_end"] for r in rs})}       # the legs did the same work: one value
        row["same_seeds_alive_in_every_leg"] = len({tuple(v["seeds_alive_at_end"]) for v in row.values()}) == 1
        row["b_over_a"] = round(row["b_one_call"]["median_us"] / row["a_loop_per_camera"]["median_us"], 3)
        result["cameras"][str(n)] = row
        print("%2d cameras: %s" % (n, json.dumps(row)), flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
