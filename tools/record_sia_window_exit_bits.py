"""Record what the fused SparseImgAlign kernel returns, bit for bit, on the ways a level can END: the reference's |x| <= eps
exit for every kind of eps, and the n_iter bound, in every kernel shape class:

    python tools/record_sia_window_exit_bits.py [out.npz]   (default: tests/golden/sia_fused_window_exit_parent_bits.npz; needs the GPU)

Run it with the library of the commit whose bits are to be kept BEFORE a change to how the end of a level is decided or handed
to the other waves; tests/test_gpu_fused_window_exits.py then holds the changed kernel to the recording.  It records what
tools/record_sia_window_bits.py and tools/record_sia_fused_bits.py do not: eps = 0, +inf, a negative value and NaN, and the
levels that end by n_iter, in the one-, three- and six-tile shapes and in the 4-wave shape, with Jres_ and x_.

160 x 120 images, levels 2..0, n_iter 4, per-wave and tile-order sums.  Frames of 40, 1100 and 2600 patches, one pair per
launch (8 waves; one, three and six tiles on the older wave of a SIMD), and a 600-pair launch of 130-patch frames (4 waves,
four distinct frames: only the first record of each is kept, the recorder and the test check that the others repeat them).
Kinds:

  eps0 / epsinf / epsneg / epsnan   the reference's exits with eps = 0, +inf, -0.5 and NaN.  +inf ends every level after
                                    one evaluation; the three others can never be reached by a finite update, so the level
                                    ends by "error increased" or by n_iter
  fixed                             fixed work: every level ends by n_iter
  exits_tiny                        the reference's exits with eps = 1e-300: some level ends by n_iter with early stop on

A record is every field of svo_hip_sia_result as words followed by Jres_ and x_ of the last evaluation
(tools/record_sia_window_bits.py).  What makes a case what it claims to be is asserted by the test on the CPU oracle.  Like
the other recordings, this one is tied to the ROCm version."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from android_svo_amd import hip          # noqa: E402
import record_sia_fused_bits as rec      # noqa: E402
import record_sia_window_bits as win     # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "sia_fused_window_exit_parent_bits.npz")
REDUCTIONS = rec.REDUCTIONS
N_WORDS = win.N_WORDS
N_ITER = 4
ONE_NS = [40, 1100, 2600]
MANY_PAIRS, MANY_N, MANY_DISTINCT = rec.MANY_PAIRS, rec.MANY_N, rec.MANY_DISTINCT
KINDS = {
    "eps0": dict(eps=0.0, early_stop=True),
    "epsinf": dict(eps=float("inf"), early_stop=True),
    "epsneg": dict(eps=-0.5, early_stop=True),
    "epsnan": dict(eps=float("nan"), early_stop=True),
    "fixed": dict(eps=1e-6, early_stop=False),
    "exits_tiny": dict(eps=1e-300, early_stop=True),
}
SHAPES = ["n%d" % n for n in ONE_NS] + ["many_n%d_x%d" % (MANY_N, MANY_PAIRS)]
CASE_IDS = ["%s_%s_%s" % (s, k, r) for s in SHAPES for k in KINDS for r, _ in REDUCTIONS]


def params(kind):
    return dict(max_level=2, min_level=0, n_iter=N_ITER, **KINDS[kind])


def frames():
    """{shape: [frame pairs]} (one pair, or the distinct pairs of the 600-pair launch)"""
    out = {"n%d" % n: [rec.make_pair(n, 3)] for n in ONE_NS}
    out[SHAPES[-1]] = [rec.make_pair(MANY_N, 11 + v) for v in range(MANY_DISTINCT)]
    return out


def solve(ctx, fps, n_pairs, reduction, prm):
    """one launch of n_pairs pairs (fps repeated) -> ([results], uint64 [n_pairs][N_WORDS])"""
    cam = fps[0].cam
    ref = hip.Pyramid(ctx, cam.width, cam.height, 5, n_pairs)
    cur = hip.Pyramid(ctx, cam.width, cam.height, 5, n_pairs)
    sia = hip.SparseImgAlign(ctx, n_pairs, max(len(fp.px) for fp in fps))
    try:
        sia.set_option(hip.SIA_OPT_REDUCTION, reduction)
        sia.set_frames(ref, cur)
        for i in range(n_pairs):
            fp = fps[i % len(fps)]
            ref.upload(i, fp.ref_pyr)
            cur.upload(i, fp.cur_pyr)
            sia.upload_pair(i, fp)
        sia.run(n_pairs, sia.params(**prm))
        assert sia.last_run_mode() == 1, "not a run of the fused kernel"
        res = sia.download_all(n_pairs)
        words = []
        for i, r in enumerate(res):
            jres, x = sia.download_last_step(i)
            words.append(np.concatenate([rec.result_words(r), jres.view(np.uint64), x.view(np.uint64)]))
        return res, np.stack(words)
    finally:
        for o in (sia, ref, cur):
            o.destroy()


def run_cases(ctx, the_frames=None):
    """{case id: ([results of the distinct pairs], uint64 [distinct pairs][N_WORDS])}; every further pair of the 600-pair launch
    must repeat the record of the frame it carries"""
    the_frames = the_frames or frames()
    out = {}
    for shape in SHAPES:
        fps = the_frames[shape]
        n_pairs = MANY_PAIRS if len(fps) > 1 else 1
        for kind in KINDS:
            for rname, red in REDUCTIONS:
                res, words = solve(ctx, fps, n_pairs, red, params(kind))
                for i in range(n_pairs):
                    assert np.array_equal(words[i], words[i % len(fps)]), (shape, kind, rname, "pair %d differs from its frame's first" % i)
                out["%s_%s_%s" % (shape, kind, rname)] = (res[:len(fps)], words[:len(fps)])
    assert list(out) == CASE_IDS
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    ctx = hip.Context(0)
    got = run_cases(ctx)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **{k: w for k, (_, w) in got.items()})
    for k, (res, _) in got.items():
        print("%-40s stop %d iters %s tracked %d" % (k, res[0].stop, list(res[0].iters)[:3], res[0].n_tracked))
    print("recorded %d cases -> %s, %d bytes" % (len(got), path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
