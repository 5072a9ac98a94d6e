#!/usr/bin/env python3
"""Diagnostic: what SIA_REDUCTION_TILE_ORDER costs in every shape class of the fused SparseImgAlign kernel.  One batch of 512
pairs per patch count (fixed work, L4-L0, 30 evaluations per level), each count chosen so that the launch takes one shape
(waves per pair, tiles of the older wave); per shape the rate with the default per-wave sums, with the tile-order sums, and
the ratio of the two times.  Prints one line per shape.

--tiny puts a 12-patch frame into slot 0, so that the launches take the instances whose workgroups may form exact Hessian rows.

    python tools/reduction_shapes.py [--pairs 512] [--tiny]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from android_svo_amd import hip, synth  # noqa: E402

# patches -> tiles per SIMD -> tiles of the older wave (8 waves) / of every wave (4 waves)
COUNTS = [(200, "8,1,1", "4,1,1"), (500, "8,1,1", "4,2,2"), (1000, "8,2,2", "4,4,2"), (1200, "8,3,2", None), (2000, "8,4,2", None),
          (2500, "8,5,2", None), (2816, "8,6,2", None)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=512)
    ap.add_argument("--tiny", action="store_true")
    args = ap.parse_args()
    ctx = hip.Context(0)
    B, n_scenes = args.pairs, 8
    for n, shape8, shape4 in COUNTS:
        fps = [synth.make_frame_pair(seed=12345 + i, n_features=n) for i in range(n_scenes)]
        tiny = synth.make_frame_pair(seed=12344, n_features=12) if args.tiny else None
        cam = fps[0].cam
        ref = hip.Pyramid(ctx, cam.width, cam.height, 5, B)
        cur = hip.Pyramid(ctx, cam.width, cam.height, 5, B)
        sia = hip.SparseImgAlign(ctx, B, n)
        sia.set_frames(ref, cur)
        for s in range(B):
            fp = tiny if (tiny is not None and s == 0) else fps[s % n_scenes]
            ref.upload(s, fp.ref_pyr)
            cur.upload(s, fp.cur_pyr)
            sia.upload_pair(s, fp)
        prm = sia.params(max_level=4, min_level=0, n_iter=30, eps=1e-6, early_stop=False)

        def ms_per_step(steps=10):
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.15:
                sia.run(B, prm)
                ctx.sync()
            best = 1e9
            for _ in range(3):
                t0 = time.perf_counter()
                for _ in range(steps):
                    sia.run(B, prm)
                ctx.sync()
                best = min(best, (time.perf_counter() - t0) / steps * 1e3)
            return best
        for waves, shape in ((8, shape8), (4, shape4)):
            if shape is None:
                continue
            sia.set_option(hip.SIA_OPT_WAVES, waves)
            t = {}
            for rnd in range(2):                                    # interleaved twice: the better of each
                for name, mode in (("per_wave", hip.SIA_REDUCTION_PER_WAVE), ("tile_order", hip.SIA_REDUCTION_TILE_ORDER)):
                    sia.set_option(hip.SIA_OPT_REDUCTION, mode)
                    t[name] = min(t.get(name, 1e9), ms_per_step())
            print("%4d patches  <%s%s>  per-wave %.3f ms/step (%.1f k frames/s)  tile-order %.3f ms/step (%.1f k frames/s)  time ratio %.3f" %
                  (n, shape, ", exact rows" if args.tiny else "", t["per_wave"], B / t["per_wave"], t["tile_order"], B / t["tile_order"], t["tile_order"] / t["per_wave"]), flush=True)
        for o in (sia, ref, cur):
            o.destroy()


if __name__ == "__main__":
    main()
