"""Record what the fused SparseImgAlign kernel returns, bit for bit, on frames that take wave 0 through every way out of
the serial window between the two barriers of an evaluation:

    python tools/record_sia_window_bits.py [out.npz]     (default: tests/golden/sia_fused_window_parent_bits.npz; needs the GPU)

Run it with the library of the commit whose bits are to be kept BEFORE a change to the window that must not move them;
tests/test_gpu_fused_window_paths.py then holds the changed kernel to the recording.  tools/record_sia_fused_bits.py records
four evaluations of ordinary frames, which never leave the usual path (small update angle, H unchanged, no exit).  The
cases here (160 x 120 images, one pair per launch, per-wave and tile-order sums):

  large_*   an update with theta^2 > 0.25 (the library path of SE3::exp): a frame of at most 16 patches, one level, fixed work;
            large_n12_of_2600 is the 12-patch frame followed by 2588 features without a point, which the solve skips: the
            launch takes the shape with six tiles per wave, whose large-angle branch is written differently
  nan_*     a solve that turns NaN (stop_, rollback): one patch of a 64-patch frame lies 1e-160 in front of the reference
            camera, so its Jacobian overflows and H is not finite -- the reference's isnan(x[0]) exit at every level; and the
            one-patch frame, whose zero update has theta == 0 (NaN translation, as in the reference)
  exits_*   the reference's exits, levels 2..0, 64 and 130 patches: eps = 0 leaves only "error increased" (rollback), eps = 1e-2
            stops on |x| <= eps
  fixed_*   fixed work, 8 evaluations per level, 130 and 600 patches, border 10: the set of patches outside the image changes
            between evaluations and H is factored again

A record is every field of svo_hip_sia_result as words (record_sia_fused_bits.result_words) followed by Jres_ and x_ of the
last evaluation.  The CPU-side properties that make a case what it claims to be (a large step, a NaN stop, an early exit) are
asserted by the test against the oracle, not here.  Like the other recording, this one is tied to the ROCm version."""
import dataclasses
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from android_svo_amd import hip, synth  # noqa: E402
import record_sia_fused_bits as rec      # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "sia_fused_window_parent_bits.npz")
WIDTH, HEIGHT = rec.WIDTH, rec.HEIGHT
REDUCTIONS = rec.REDUCTIONS
N_WORDS = 7 + 1 + 36 + 1 + 1 + 8 + 2 + 6 + 6
IDENTITY = np.array([0, 0, 0, 0, 0, 0, 1.0])


def _pair(seed, n):
    return synth.make_frame_pair(seed=seed, width=WIDTH, height=HEIGHT, n_features=n, border=10,
                                 null_point_every=7 if n >= 130 else 0)


def overflow_pair(seed=7300, n=64):
    """identity poses (T_cur_from_ref starts exactly at the identity, so the patch projects onto its own feature) and one
    point 1e-160 along its bearing: 1/z^2 overflows in the patch's Jacobian"""
    fp = _pair(seed, n)
    pos = fp.pos.copy()
    pos[n // 2] = fp.f[n // 2] * 1e-160
    return dataclasses.replace(fp, T_ref_w=IDENTITY.copy(), T_cur_w_init=IDENTITY.copy(), pos=pos)


def padded_pair(seed, n, n_total):
    """the n-patch frame followed by n_total - n features that have no point"""
    fp, pad = _pair(seed, n), _pair(9000 + 7 * n_total, n_total)
    k = n_total - n
    return dataclasses.replace(fp, px=np.concatenate([fp.px, pad.px[:k]]), f=np.ascontiguousarray(np.concatenate([fp.f, pad.f[:k]])),
                               pos=np.ascontiguousarray(np.concatenate([fp.pos, pad.pos[:k]])),
                               has_point=np.concatenate([fp.has_point, np.zeros(k, dtype=np.uint8)]))


@dataclasses.dataclass
class Case:
    name: str
    kind: str               # large / nan / exits / fixed
    fp: object
    prm: dict               # max_level, min_level, n_iter, eps, early_stop


CASE_NAMES = ["large_n12", "large_n16", "large_n12_of_2600", "nan_overflow_fixed", "nan_overflow_exits", "nan_one_patch",
              "exits_worse_n64", "exits_eps_n64", "exits_worse_n130", "exits_eps_n130", "fixed_n130", "fixed_n600"]


def cases():
    """the cases, in the order of CASE_NAMES (builds the synthetic frames: call it from a fixture, not at import)"""
    out = []
    for seed, n in ((7000, 12), (7001, 16)):
        out.append(Case("large_n%d" % n, "large", _pair(seed, n), dict(max_level=2, min_level=2, n_iter=6, eps=1e-6, early_stop=False)))
    out.append(Case("large_n12_of_2600", "large", padded_pair(7000, 12, 2600), dict(max_level=2, min_level=2, n_iter=6, eps=1e-6, early_stop=False)))
    for early in (False, True):
        tag = "exits" if early else "fixed"
        out.append(Case("nan_overflow_%s" % tag, "nan", overflow_pair(), dict(max_level=2, min_level=0, n_iter=4, eps=1e-6, early_stop=early)))
    out.append(Case("nan_one_patch", "nan", _pair(42, 1), dict(max_level=2, min_level=0, n_iter=4, eps=1e-6, early_stop=True)))
    for n in (64, 130):
        out.append(Case("exits_worse_n%d" % n, "exits", _pair(7200, n), dict(max_level=2, min_level=0, n_iter=30, eps=0.0, early_stop=True)))
        out.append(Case("exits_eps_n%d" % n, "exits", _pair(7200, n), dict(max_level=2, min_level=0, n_iter=30, eps=1e-2, early_stop=True)))
    for n in (130, 600):
        out.append(Case("fixed_n%d" % n, "fixed", _pair(9000 + 7 * n, n), dict(max_level=2, min_level=0, n_iter=8, eps=1e-6, early_stop=False)))
    assert [c.name for c in out] == CASE_NAMES
    return out


def solve(ctx, case, reduction):
    """one one-pair launch -> (svo_hip_sia_result, words)"""
    fp = case.fp
    ref = hip.Pyramid(ctx, fp.cam.width, fp.cam.height, 5, 1)
    cur = hip.Pyramid(ctx, fp.cam.width, fp.cam.height, 5, 1)
    sia = hip.SparseImgAlign(ctx, 1, len(fp.px))
    try:
        sia.set_option(hip.SIA_OPT_REDUCTION, reduction)
        sia.set_frames(ref, cur)
        ref.upload(0, fp.ref_pyr)
        cur.upload(0, fp.cur_pyr)
        sia.upload_pair(0, fp)
        sia.run(1, sia.params(**case.prm))
        assert sia.last_run_mode() == 1, "not a run of the fused kernel"
        r = sia.download(0)
        jres, x = sia.download_last_step(0)
        return r, np.concatenate([rec.result_words(r), jres.view(np.uint64), x.view(np.uint64)])
    finally:
        for o in (sia, ref, cur):
            o.destroy()


def run_cases(ctx, the_cases=None):
    """{case_reduction: (result, uint64 [N_WORDS])}"""
    return {"%s_%s" % (c.name, rname): solve(ctx, c, red) for c in (the_cases or cases()) for rname, red in REDUCTIONS}


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    ctx = hip.Context(0)
    got = run_cases(ctx)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **{k: w for k, (_, w) in got.items()})
    for k, (r, _) in sorted(got.items()):
        print("%-36s stop %d iters %s tracked %d T %s" % (k, r.stop, list(r.iters)[:3], r.n_tracked, np.array(r.T_cur_w)[[0, 3]]))
    print("recorded %d cases -> %s, %d bytes" % (len(got), path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
