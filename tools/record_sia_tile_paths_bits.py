"""Record what the fused SparseImgAlign kernel returns, bit for bit, on the paths of its tile loop that scalar bookkeeping decides:

    python tools/record_sia_tile_paths_bits.py [out.npz]   (default: tests/golden/sia_fused_tile_paths_parent_bits.npz; needs the GPU)

Run it with the library of the commit whose bits are to be kept BEFORE a change to the tile loop that must not move them;
tests/test_gpu_fused_tile_paths.py then holds the changed kernel to the recording.  Like tools/record_sia_fused_bits.py:
160 x 120 images, levels 2..0, 4 evaluations per level, fixed work and the reference's exits, per-wave and tile-order sums.
The cases (also what the test runs):

  * tile counts: for each 8-wave shape with 1 to 4 tiles on a wave, a frame whose tile count leaves some waves a tile short
    (65, 577, 1089, 1601 patches) and one that fills the shape exactly (512, 1024, 1536, 2048), so that the number of tiles a
    wave has takes every value from 0 to the shape's tiles per wave on some wave, on older and on younger waves of a SIMD;
  * a changing in-image set: frames whose initial pose is off by several pixels, so that patches cross the 3-pixel border
    between two evaluations of one level (drift_pairs; the CPU oracle shows the change, see the test);
  * the 4-wave shape: one launch of 600 pairs of 130 patches, started off the same way.

A record is every field of svo_hip_sia_result plus Jres_ and x_ of the last evaluation, as uint64 words.  The recorded bits
are tied to the ROCm version that made them (see tools/record_sia_fused_bits.py)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from android_svo_amd import hip, synth  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "sia_fused_tile_paths_parent_bits.npz")
WIDTH, HEIGHT = 160, 120
MAX_LEVEL, MIN_LEVEL, N_ITER = 2, 0, 4
NS_SHORT = [65, 577, 1089, 1601]          # 2, 10, 18, 26 tiles: one, two, ... tiles on the first waves only
NS_FULL = [512, 1024, 1536, 2048]         # 8, 16, 24, 32 tiles: every wave of the shape has 1, 2, 3, 4
STOPS = [("fixed", False), ("exits", True)]
REDUCTIONS = [("per_wave", hip.SIA_REDUCTION_PER_WAVE), ("tile_order", hip.SIA_REDUCTION_TILE_ORDER)]
# A lone frame never leaves an OLDER wave of a two-, three- or four-tile shape short (its tiles come first).  So each of those
# shapes is also launched with its full frame in slot 0, which picks the shape, and smaller frames behind it: with 2, 6, 10,
# 13 and 18 tiles the older waves of some SIMD have 0, 1, 2, 3 and 4 of their tiles and the younger ones 0, 1 or 2.
MIXED = {1024: [65, 330], 1536: [65, 330, 577], 2048: [65, 330, 800, 1089]}
# (patches, seed variant, translation offset of the initial pose along x and y in metres)
DRIFT = [(600, 0, (0.05, -0.03)), (1100, 1, (-0.12, 0.05)), (1601, 2, (0.04, 0.04))]
MANY_PAIRS, MANY_N, MANY_DISTINCT = 600, 130, 4          # >= 2 pairs per CU: the 4-wave shape
WORDS = 7 + 1 + 36 + 1 + 1 + 8 + 2 + 6 + 6               # svo_hip_sia_result, Jres_, x_


def make_pair(n, variant=0):
    # border 10: at level 2 (40 x 30) the outermost features are outside the 3-pixel border; every seventh has no point
    return synth.make_frame_pair(seed=31000 + 7 * n + variant, width=WIDTH, height=HEIGHT, n_features=n, border=10,
                                 null_point_every=7 if n >= 130 else 0)


def drift_pair(n, variant, offset):
    """a pair whose initial pose is the reference pose moved sideways: the first evaluations of the coarsest level pull the
    patches along the image border back by whole pixels, in and out of the image"""
    fp = make_pair(n, 100 + variant)
    fp.T_cur_w_init = synth.se3_mul(synth.se3_from_twist(np.array([offset[0], offset[1], 0.0]), np.zeros(3)), fp.T_ref_w)
    return fp


def drift_pairs():
    return [drift_pair(n, v, off) for n, v, off in DRIFT]


def result_words(r, jres, x):
    """every field of svo_hip_sia_result, then Jres_ and x_ of the last evaluation, as uint64 words (a NaN keeps its bits)"""
    return np.concatenate([
        np.array(r.T_cur_w, dtype=np.float64).view(np.uint64), np.array([r.n_tracked], dtype=np.uint64),
        np.array(r.H, dtype=np.float64).view(np.uint64), np.array([r.chi2], dtype=np.float64).view(np.uint64),
        np.array([r.stop], dtype=np.int64).view(np.uint64), np.array(r.iters, dtype=np.int64).view(np.uint64),
        np.array([r.n_precompute_patches, r.n_residual_patches], dtype=np.uint64),
        np.array(jres, dtype=np.float64).view(np.uint64), np.array(x, dtype=np.float64).view(np.uint64)])


def solve(ctx, fps, reduction, early_stop, last_step_of=None):
    """one launch over fps -> [len(fps)][WORDS]; Jres_ and x_ are fetched for the slots in last_step_of (default: all), the
    others carry zeros there"""
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
        slots = set(range(n) if last_step_of is None else last_step_of)
        zero = np.zeros(6)
        rows = []
        for i, r in enumerate(sia.download_all(n)):
            jres, x = sia.download_last_step(i) if i in slots else (zero, zero)
            rows.append(result_words(r, jres, x))
        return np.stack(rows)
    finally:
        for o in (sia, ref, cur):
            o.destroy()


def case_names():
    names = ["tiles_n%d_%s_%s" % (n, s, r) for n in NS_SHORT + NS_FULL for s, _ in STOPS for r, _ in REDUCTIONS]
    names += ["mixed_n%d_%s_%s" % (n, s, r) for n in MIXED for s, _ in STOPS for r, _ in REDUCTIONS]
    names += ["drift_n%d_%s_%s" % (n, s, r) for n, _, _ in DRIFT for s, _ in STOPS for r, _ in REDUCTIONS]
    return names + ["many_n%d_x%d" % (MANY_N, MANY_PAIRS)]


def run_cases(ctx):
    """{case name: uint64 [pairs][WORDS]} for every case of the fixture"""
    out = {}
    for n in NS_SHORT + NS_FULL:
        fp = make_pair(n)
        for sname, early in STOPS:
            for rname, red in REDUCTIONS:
                out["tiles_n%d_%s_%s" % (n, sname, rname)] = solve(ctx, [fp], red, early)
    for n, small in MIXED.items():
        fps = [make_pair(n)] + [make_pair(m, 50) for m in small]
        for sname, early in STOPS:
            for rname, red in REDUCTIONS:
                out["mixed_n%d_%s_%s" % (n, sname, rname)] = solve(ctx, fps, red, early)
    for (n, _, _), fp in zip(DRIFT, drift_pairs()):
        for sname, early in STOPS:
            for rname, red in REDUCTIONS:
                out["drift_n%d_%s_%s" % (n, sname, rname)] = solve(ctx, [fp], red, early)
    distinct = [drift_pair(MANY_N, 10 + v, (0.08 - 0.05 * v, 0.03 * v - 0.04)) for v in range(MANY_DISTINCT)]
    out["many_n%d_x%d" % (MANY_N, MANY_PAIRS)] = solve(ctx, [distinct[i % MANY_DISTINCT] for i in range(MANY_PAIRS)],
                                                      hip.SIA_REDUCTION_PER_WAVE, False, last_step_of=range(2 * MANY_DISTINCT))
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
