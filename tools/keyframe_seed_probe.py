"""Host-side cost of one keyframe of the depth filter: the device calls of this tree against the composition of the older
entry points.

One keyframe = updateSeeds(kf) with its grid marks (depth_filter.cpp:302-306) + initializeSeeds(kf) (:129-151):

  new   pass with report_updated = 0 + svo_hip_seed_batch_mark_updated + collect, svo_hip_grid_mark_px over the existing
        features, svo_hip_seed_batch_create_detected (grid cleared behind it)
  old   pass with report_updated = 1 + collect (every updated seed an event), the host sets the grid bytes from the events and
        from the existing features, svo_hip_detect_features with that grid, svo_hip_seed_batch_create of the new seeds

Rows: 3 batches of about 300 seeds with 120 existing features at 640x480, and one 100 k-seed batch.  Each leg runs in a
process of its own, the legs alternate, and the old leg may load another build of the library (SVO_HIP_LIB, as tools/ab.sh):

    python tools/keyframe_seed_probe.py --old-lib build/libsvo_hip_parent.so --out profiles/r14_keyframe_seed_probe.json

Median of --reps keyframes (at least 200) after --warmup, microseconds.  No test asserts a time."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CELL, N_EXISTING = 30, 120


def leg(which: str, row: str, reps: int, warmup: int) -> dict:
    import numpy as np
    from android_svo_amd import hip, seedsynth
    ctx = hip.Context(0)
    sizes = (300, 310, 290) if row == "3x300" else (100000,)
    mk = seedsynth.make_multi_keyframe_case(sizes, seed=31)
    cam, K = mk.cam, len(sizes)
    kf = hip.Pyramid(ctx, cam.width, cam.height, 5, K + 1)
    cf = hip.Pyramid(ctx, cam.width, cam.height, 5, 1)
    cf.upload(0, mk.cur_pyr)
    kf.upload(K, mk.cur_pyr)                                  # the new keyframe's own slot
    for k, s in enumerate(mk.keyframes):
        kf.upload(k, s.ref_pyr)
    T_refs = np.stack([s.T_ref_w for s in mk.keyframes])
    slots = list(range(K))
    existing = np.floor(np.random.default_rng(1).uniform([0, 0], [cam.width, cam.height], (N_EXISTING, 2)))
    cols, rows = hip.detect_grid(cam.width, cam.height, CELL)
    grid = hip.DetectorGrid(ctx, cam.width, cam.height, CELL) if which == "new" else None
    times, n_new = [], 0
    for rep in range(warmup + reps):
        # fresh seeds every keyframe (not timed): the pass must find seeds to update
        batches = [hip.ResidentSeeds(ctx, s.px, s.f, s.level, s.a, s.b, s.mu, s.z_range, (s.sigma2 * np.float32(0.02)).astype(np.float32))
                   for s in mk.keyframes]
        ctx.sync()
        t0 = time.perf_counter()
        if which == "new":
            hip.ResidentSeeds.update_group_async(batches, kf, slots, cf, 0, cam, T_refs, mk.T_cur_w, report_updated=False)
            grid.mark_updated(batches)
            for b in batches:
                b.collect_raw()
            grid.mark_px(existing)
            rs, feats = hip.ResidentSeeds.from_detection(ctx, kf, K, cam, 2.2, 1.0, cell_size=CELL, grid=grid, clear_grid=True)
            n_new = len(feats["px"])
        else:
            hip.ResidentSeeds.update_group_async(batches, kf, slots, cf, 0, cam, T_refs, mk.T_cur_w, report_updated=True)
            occ = np.zeros(rows * cols, np.uint8)
            for b in batches:
                ev, _ = b.collect()
                pc = ev["px_cur"][ev["status"] >= hip.SEED_UPDATED]
                k = (pc[:, 1] / CELL).astype(np.int64) * cols + (pc[:, 0] / CELL).astype(np.int64)
                occ[k[(k >= 0) & (k < rows * cols)]] = 1
            occ[(existing[:, 1] / CELL).astype(np.int64) * cols + (existing[:, 0] / CELL).astype(np.int64)] = 1
            px, f, lvl, _ = hip.detect_features(ctx, kf, K, cam, n_pyr_levels=3, cell_size=CELL, occupancy=occ)
            a, b_, mu, zr, s2 = seedsynth.seed_ctor(2.2, 1.0, len(px))
            rs = hip.ResidentSeeds(ctx, px, f, lvl, a, b_, mu, zr, s2) if len(px) else None
            n_new = len(px)
        dt = time.perf_counter() - t0
        if rep >= warmup:
            times.append(dt * 1e6)
        for b in batches + ([rs] if rs is not None else []):
            b.destroy()
    t = np.sort(np.array(times))
    return dict(leg=which, row=row, reps=reps, median_us=float(np.median(t)), p10_us=float(t[len(t) // 10]), p90_us=float(t[(9 * len(t)) // 10]),
                new_seeds=int(n_new), lib=os.path.basename(hip.LIB_PATH))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old-lib", default=None, help="library the old leg loads (default: this tree's)")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2, help="alternations of the two legs per row")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None)
    ap.add_argument("--row", default=None)
    a = ap.parse_args()
    if a.leg:                                                 # a child process: one leg of one row
        print(json.dumps(leg(a.leg, a.row, a.reps, a.warmup)))
        return
    assert a.reps >= 200, "median of at least 200 keyframes"
    results = []
    for row in ("3x300", "1x100k"):
        for _ in range(a.rounds):
            for which in ("old", "new"):
                env = dict(os.environ)
                if which == "old" and a.old_lib:
                    env["SVO_HIP_LIB"] = os.path.abspath(a.old_lib)
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", which, "--row", row, "--reps", str(a.reps),
                                      "--warmup", str(a.warmup)], env=env, capture_output=True, text=True, timeout=900)
                if out.returncode != 0:
                    sys.stderr.write(out.stdout + out.stderr)
                    sys.exit(1)
                results.append(json.loads(out.stdout.strip().splitlines()[-1]))
                print(results[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(dict(what="host-side microseconds of one keyframe of the depth filter (tools/keyframe_seed_probe.py)", runs=results), fh, indent=1)


if __name__ == "__main__":
    main()
