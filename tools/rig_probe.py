"""What a camera model per camera costs the many-camera paths, against another build of the library (the parent commit's:
--parent-lib, through SVO_HIP_LIB).  Host-side time, one process per leg, parent and this tree alternating `--rounds` times:

  seed pass      N cameras x 3 batches x 300 seeds, 640x480, no keyframe frames, one svo_hip_seed_batch_update_cameras_async call
                 + collects per frame set (the leg of tools/df_cameras_probe.py); us per frame set, 200 sets after 20 warm-ups
  tracker group  N cameras through svo_hip_tracker_group_track over a 20-frame sequence (the group leg of tools/chain_bench.py);
                 frames/s of every pass over the sequence, 6 passes after a warm-up pass

Both through the OLD entry points (one model for all cameras), at 1, 8 and 64 cameras: per process the median and the 10th / 90th
percentile of its samples; per build the median of the process medians and, for the parent, the band [lowest p10, highest p90].
For the record the same legs once on this tree with three distinct camera models (tests/rig_case.py: A, B, C round the cameras,
every camera on images of its own model) through the rig entry points.  -> profiles/r19_rig_probe.json

  python tools/rig_probe.py --parent-lib build/libsvo_hip_parent.so [--rounds 2] [--out profiles/r19_rig_probe.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CAMERAS = (1, 8, 64)
N_BATCHES, N_SEEDS, WARM, SETS = 3, 300, 20, 200
GROUP_PASSES = 6


def _summary(samples, **more):
    s = sorted(samples)
    return dict(more, median=s[len(s) // 2], p10=s[int(0.1 * len(s))], p90=s[min(int(0.9 * len(s)), len(s) - 1)], n=len(s))


def seed_leg(n_cams, rig):
    import numpy as np
    import rig_case as rc
    from android_svo_amd import hip, seedsynth
    ctx = hip.Context(0)
    names = rc.NAMES if rig else ("A",)
    models = [rc.camera(n, 640, 480) if rig else None for n in names]
    scenes = []
    for s, m in enumerate(models):
        mk = seedsynth.make_multi_keyframe_case((N_SEEDS,) * N_BATCHES, seed=50 + s, cam=m)
        if rig:
            for sc in mk.keyframes:
                sc.f = rc.bearings(m, sc.px)
        scenes.append(mk)
    kf = hip.Pyramid(ctx, 640, 480, 5, n_cams * N_BATCHES)
    cf = hip.Pyramid(ctx, 640, 480, 5, n_cams)
    batches, passes, cams = [], [], []
    for c in range(n_cams):
        mk = scenes[c % len(scenes)]
        cf.upload(c, mk.cur_pyr)
        for k, sc in enumerate(mk.keyframes):
            kf.upload(c * N_BATCHES + k, sc.ref_pyr)
        batches.append([hip.ResidentSeeds(ctx, sc.px, sc.f, sc.level, sc.a, sc.b, sc.mu, sc.z_range, sc.sigma2) for sc in mk.keyframes])
        passes.append((batches[c], [c * N_BATCHES + k for k in range(N_BATCHES)], np.stack([sc.T_ref_w for sc in mk.keyframes]), c, mk.T_cur_w, False))
        cams.append(mk.cam)

    def one_call():
        hip.ResidentSeeds.update_cameras_async(passes, kf, cf, cams if rig else cams[0])
        for b in batches:
            for r in b:
                r.collect_raw()
    for _ in range(WARM):
        one_call()
    ts = []
    for _ in range(SETS):
        t0 = time.perf_counter()
        one_call()
        ts.append(1e6 * (time.perf_counter() - t0))
    print(json.dumps(_summary(ts, unit="us per frame set", seeds_alive_at_end=sum(r.n_alive() for b in batches for r in b), lib=hip.LIB_PATH)), flush=True)


def group_leg(n_cams, rig):
    import numpy as np
    import rig_case as rc
    import tracking_chain as tc
    from android_svo_amd import hip
    ctx = hip.Context(0)
    seqs = [rc.sequence(n, n_frames=20, n_map=600) for n in rc.NAMES] if rig else [tc.make_sequence(n_frames=20)]
    cfg = dict(max_keyframes=2, max_points=1024, max_obs=1024, max_kf_features=1024, max_candidates=16, max_items=1024,
               max_frame_features=1024, grid_size=tc.CELL, max_fts=tc.MAX_FTS, klt_min_level=2)
    mine = [seqs[c % len(seqs)] for c in range(n_cams)]
    maps = [tc.sequence_map(s) for s in seqs]
    grp = hip.TrackerGroup(ctx, [s["cam"] for s in mine] if rig else seqs[0]["cam"], n_cams, **cfg)
    bufs = [t.image_buffer() for t in grp.cameras]
    for t, s in zip(grp.cameras, mine):
        t.upload_keyframe(0, s["pyrs"][0][0])
    rates, last = [], None
    for rep in range(GROUP_PASSES + 1):
        for c, (t, s) in enumerate(zip(grp.cameras, mine)):
            t.set_map(maps[c % len(seqs)])
            t.set_last_frame(s["T0"], s["px0"], s["f0"], np.arange(len(s["px0"]), dtype=np.int32), kf_slot=0)
        ctx.sync()
        t0 = time.perf_counter()
        t_copy = 0.0
        for k in range(1, 20):
            tc0 = time.perf_counter()
            for b, s in zip(bufs, mine):
                b[:] = s["pyrs"][k][0]
            t_copy += time.perf_counter() - tc0                    # (the camera pipeline's write into the buffer: not the tracker's time)
            res = grp.track(bufs)
        if rep > 0:
            rates.append(n_cams * 19 / (time.perf_counter() - t0 - t_copy))
        poses = [list(r.T_f_w) for r in res]
        assert last is None or poses == last                       # every pass ends where the first did
        last = poses
        assert all(int(r.n_matches) >= 50 for r in res)
    grp.destroy()
    print(json.dumps(_summary(rates, unit="frames per s", lib=hip.LIB_PATH)), flush=True)


def child(kind, n_cams, rig, lib):
    env = dict(os.environ)
    env.pop("SVO_HIP_LIB", None)
    if lib:
        env["SVO_HIP_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", kind, "--cameras", str(n_cams)] + (["--rig"] if rig else [])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=280)
    if r.returncode != 0:
        raise SystemExit("leg %s with %d cameras failed (%d):\n%s" % (kind, n_cams, r.returncode, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("seed", "group"))
    ap.add_argument("--cameras", type=int, default=8)
    ap.add_argument("--rig", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_rig_probe.json"))
    args = ap.parse_args()
    if args.leg:
        (seed_leg if args.leg == "seed" else group_leg)(args.cameras, args.rig)
        return
    if not args.parent_lib:
        raise SystemExit("--parent-lib: the parent commit's libsvo_hip.so")
    result = {"what": __doc__.split("\n\n")[1].strip(), "rounds": args.rounds, "legs": {}}
    for kind in ("seed", "group"):
        for n in CAMERAS:
            runs = {"parent": [], "this_tree": []}
            for _ in range(args.rounds):
                runs["parent"].append(child(kind, n, False, args.parent_lib))
                runs["this_tree"].append(child(kind, n, False, None))
            rig = child(kind, n, True, None)
            med = lambda rs: sorted(r["median"] for r in rs)[len(rs) // 2]
            band = [min(r["p10"] for r in runs["parent"]), max(r["p90"] for r in runs["parent"])]
            row = {"unit": rig["unit"], "parent_process_medians": [round(r["median"], 1) for r in runs["parent"]],
                   "this_tree_process_medians": [round(r["median"], 1) for r in runs["this_tree"]], "parent_median": round(med(runs["parent"]), 1),
                   "parent_p10_p90_band": [round(v, 1) for v in band], "this_tree_median": round(med(runs["this_tree"]), 1),
                   "this_tree_over_parent": round(med(runs["this_tree"]) / med(runs["parent"]), 4),
                   "this_tree_median_inside_parent_band": band[0] <= med(runs["this_tree"]) <= band[1],
                   "three_distinct_cameras_rig_entry": {k: round(rig[k], 1) for k in ("median", "p10", "p90")}}
            result["legs"]["%s_%d_cameras" % (kind, n)] = row
            print("%s %2d cameras: %s" % (kind, n, json.dumps(row)), flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
