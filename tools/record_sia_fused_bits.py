"""Record what the fused SparseImgAlign kernel returns, bit for bit, for a fixed set of small launches:

    python tools/record_sia_fused_bits.py [out.npz]        (default: tests/golden/sia_fused_parent_bits.npz; needs the GPU)

Run it with the library of the commit whose bits are to be kept BEFORE a change to the kernel that must not move them;
tests/test_gpu_fused_parent_bits.py then holds the changed kernel to the recording.  The cases (also what the test runs):
one-pair launches on 160 x 120 images, levels 2..0, 4 evaluations, fixed work and the reference's exits, one frame per
tiles-per-wave class the launcher can pick, default and tile-order sums; and one 600-pair launch of 130-patch frames, which
takes the 4-wave shape.  The bits depend on the compiler's code for the library's own arithmetic only where the library
leaves it a choice (it builds with -ffp-contract=off), and on the ROCm version's device library (sqrt, division): a
recording is tied to the ROCm version that made it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from android_svo_amd import hip, synth  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "sia_fused_parent_bits.npz")
WIDTH, HEIGHT = 160, 120
MAX_LEVEL, MIN_LEVEL, N_ITER = 2, 0, 4
# 8-wave shape, tiles on the older wave of a SIMD: 1 (a handful of patches: the exact-rows instance), 1 (one full tile), 1 (three
# tiles), then 2, 3, 4 (7 per SIMD), 4 (8 per SIMD) and 6
NS = [5, 64, 130, 600, 1100, 1600, 2000, 2600]
STOPS = [("fixed", False), ("exits", True)]
REDUCTIONS = [("per_wave", hip.SIA_REDUCTION_PER_WAVE), ("tile_order", hip.SIA_REDUCTION_TILE_ORDER)]
MANY_PAIRS, MANY_N, MANY_DISTINCT = 600, 130, 4          # >= 2 pairs per CU: the 4-wave shape


def make_pair(n, variant=0):
    # border 10: at level 2 (40 x 30) the outermost features are outside the 3-pixel border, so the stale-patch and the
    # outside-the-image paths run; every seventh feature of the larger frames has no point
    return synth.make_frame_pair(seed=9000 + 7 * n + variant, width=WIDTH, height=HEIGHT, n_features=n, border=10,
                                 null_point_every=7 if n >= 130 else 0)


def result_words(r):
    """every field of svo_hip_sia_result as uint64 words (a NaN keeps its bits)"""
    return np.concatenate([
        np.array(r.T_cur_w, dtype=np.float64).view(np.uint64), np.array([r.n_tracked], dtype=np.uint64),
        np.array(r.H, dtype=np.float64).view(np.uint64), np.array([r.chi2], dtype=np.float64).view(np.uint64),
        np.array([r.stop], dtype=np.int64).view(np.uint64), np.array(r.iters, dtype=np.int64).view(np.uint64),
        np.array([r.n_precompute_patches, r.n_residual_patches], dtype=np.uint64)])


def solve(ctx, fps, reduction, early_stop):
    """one launch over fps -> [len(fps)][words]"""
    cam = fps[0].cam
    n = len(fps)
    ref = hip.Pyramid(ctx, cam.width, cam.height, 5, n)
    cur = hip.Pyramid(ctx, cam.width, cam.height, 5, n)
    sia = hip.SparseImgAlign(ctx, n, max(len(fp.px) for fp in fps))
    try:
        sia.set_option(hip.SIA_OPT_REDUCTION, reduction)
        sia.set_frames(ref, cur)
        for i, fp in enumerate(fps):
            ref.upload(i, fp.ref_pyr)
            cur.upload(i, fp.cur_pyr)
            sia.upload_pair(i, fp)
        sia.run(n, sia.params(max_level=MAX_LEVEL, min_level=MIN_LEVEL, n_iter=N_ITER, eps=1e-6, early_stop=early_stop))
        assert sia.last_run_mode() == 1, "not a run of the fused kernel"
        return np.stack([result_words(r) for r in sia.download_all(n)])
    finally:
        for o in (sia, ref, cur):
            o.destroy()


def run_cases(ctx):
    """{case name: uint64 [pairs][words]} for every case of the fixture"""
    out = {}
    for n in NS:
        fp = make_pair(n)
        for sname, early in STOPS:
            for rname, red in REDUCTIONS:
                out["one_n%d_%s_%s" % (n, sname, rname)] = solve(ctx, [fp], red, early)
    distinct = [make_pair(MANY_N, 1 + v) for v in range(MANY_DISTINCT)]
    out["many_n%d_x%d" % (MANY_N, MANY_PAIRS)] = solve(ctx, [distinct[i % MANY_DISTINCT] for i in range(MANY_PAIRS)],
                                                      hip.SIA_REDUCTION_PER_WAVE, False)
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    ctx = hip.Context(0)
    cases = run_cases(ctx)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **cases)
    print("recorded %d cases (%d result records) -> %s, %d bytes" % (len(cases), sum(len(v) for v in cases.values()), path,
                                                                    os.path.getsize(path)))


if __name__ == "__main__":
    main()
