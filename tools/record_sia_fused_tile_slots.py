"""Record what the fused SparseImgAlign kernel returns, bit for bit, wherever the bookkeeping of its tile loop takes part: which
tile a wave reads from LDS and which from memory, the patches counted as measurements, and the note that the set of patches
outside the current image changed:

    python tools/record_sia_fused_tile_slots.py [out.npz]   (default: tests/golden/sia_fused_tile_slots_parent_bits.npz; needs the GPU)

Run it with the library of the commit whose bits are to be kept BEFORE a change to that bookkeeping;
tests/test_gpu_fused_tile_slots.py then holds the changed kernel to the recording.  640 x 480 images, 4 evaluations per level,
levels 4..2 and 4..0, fixed work and the reference's exits, per-wave and tile-order sums.  The cases (also what the test runs):

  * frames of 40, 130, 600, 1100, 1600, 2000, 2500 and 2816 patches, two pairs per launch: one to six tiles on the older wave
    of a SIMD.  The three- and four-tile shapes (1100, 1600, 2000) run with the extra LDS tiles the launcher gives them and
    without any (SIA_OPT_EXTRA_LDS 0);
  * "out": the 2000-patch frame (four tiles on every wave: positions 0 and 2 are LDS tiles, 1 and 3 memory tiles) started from
    poses that are off sideways, so that patches along the image border are outside the current image at the first
    evaluation and come back, or leave, at a later one.  out_changes() counts on the CPU oracle, per pose, the patches whose
    state changes at the first and at later evaluations of the coarsest level on each of the four tile positions; the counts
    are part of the recording, and all of them must be positive;
  * one launch of 600 pairs of 130 patches (four distinct frames): the 4-wave shape.

A record is every field of svo_hip_sia_result plus Jres_ and x_ of the last evaluation, as uint64 words.  The recorded bits
are tied to the ROCm version that made them (see tools/record_sia_fused_bits.py)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from android_svo_amd import hip, synth        # noqa: E402
import record_sia_tile_paths_bits as paths    # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "sia_fused_tile_slots_parent_bits.npz")
WIDTH, HEIGHT = 640, 480
MAX_LEVEL, N_ITER = 4, 4
LEVELS = [("l42", 2), ("l40", 0)]                        # (name, min_level)
NS = [40, 130, 600, 1100, 1600, 2000, 2500, 2816]        # tiles on the older wave of a SIMD: 1, 1, 2, 3, 4, 4, 5, 6
NS_EXTRA = [1100, 1600, 2000]                            # shapes that keep a third LDS tile on some waves
STOPS = paths.STOPS
REDUCTIONS = paths.REDUCTIONS
WORDS = paths.WORDS
OUT_N = 2000
# translation of the initial pose against the reference pose, metres along x and y (the plane is about 2 m away: 0.1 m is about
# a pixel and a half of level 4)
OUT_POSES = [(0.08, 0.0), (-0.06, 0.05)]
MANY_PAIRS, MANY_N, MANY_DISTINCT = 600, 130, 4          # >= 2 pairs per CU: the 4-wave shape
COUNTS_KEY = "out_changes"
ZERO6 = np.zeros(6)


def make_pair(n, variant=0):
    # border 48: the outermost features sit on the 3-pixel border of level 4 (40 x 30); every seventh has no point
    return synth.make_frame_pair(seed=47000 + 7 * n + variant, width=WIDTH, height=HEIGHT, n_features=n, border=48,
                                 null_point_every=7 if n >= 130 else 0)


def out_pair(offset, variant):
    fp = make_pair(OUT_N, 200 + variant)
    fp.T_cur_w_init = synth.se3_mul(synth.se3_from_twist(np.array([offset[0], offset[1], 0.0]), np.zeros(3)), fp.T_ref_w)
    return fp


def out_pairs():
    return [out_pair(off, v) for v, off in enumerate(OUT_POSES)]


def tile_position(i):
    """position, in its wave's tile loop, of patch i of a frame whose waves all own four tiles: tile t is tile t >> 2 of
    SIMD t & 3, the older wave takes the SIMD's first four and the younger one the four that follow"""
    return ((i // 64) >> 2) % 4


def outside_level(fp, level, T_cur_w):
    """bool [n]: patches with a point whose reference patch is inside the level's image and whose projection with pose T_cur_w
    is not -- the set the kernel takes out of H -- and the number of patches inside"""
    cam = fp.cam
    scale = np.float32(1.0 / (1 << level))
    cols, rows = cam.width >> level, cam.height >> level
    ref_pos = synth.se3_inv(fp.T_ref_w)[:3]
    T = synth.se3_mul(T_cur_w, synth.se3_inv(fp.T_ref_w))
    ur = np.floor(fp.px.astype(np.float32) * scale).astype(np.int64)
    valid = (fp.has_point != 0) & (ur[:, 0] - 3 >= 0) & (ur[:, 1] - 3 >= 0) & (ur[:, 0] < cols - 3) & (ur[:, 1] < rows - 3)
    depth = np.linalg.norm(fp.pos - ref_pos, axis=1)
    xyz = np.stack([synth.se3_act(T, p) for p in fp.f * depth[:, None]])
    u = ((cam.fx * xyz[:, 0] / xyz[:, 2] + cam.cx).astype(np.float32) * scale).astype(np.float64)
    v = ((cam.fy * xyz[:, 1] / xyz[:, 2] + cam.cy).astype(np.float32) * scale).astype(np.float64)
    ui, vi = np.floor(u), np.floor(v)
    inside = valid & (ui - 3 >= 0) & (vi - 3 >= 0) & (ui < cols - 3) & (vi < rows - 3)
    return valid & ~inside, int(inside.sum())


def out_changes(fps=None):
    """int64 [poses][2][4]: per pose, the patches whose outside-the-image state changes at the first evaluation of level 4
    ([0]) and at its later evaluations ([1]) on tile positions 0..3.  The poses of the evaluations are the CPU oracle's (fixed
    work, 0 .. N_ITER - 1 updates on that level); its count of measurements confirms each set."""
    from oracle import orc
    fps = fps or out_pairs()
    counts = np.zeros((len(fps), 2, 4), dtype=np.int64)
    pos = np.array([tile_position(i) for i in range(OUT_N)])
    for a, fp in enumerate(fps):
        before = np.zeros(OUT_N, dtype=bool)               # a level starts with no patch marked
        seen = 0
        for m in range(N_ITER):
            T = fp.T_cur_w_init
            if m > 0:
                r = orc.sparse_img_align(fp, max_level=MAX_LEVEL, min_level=MAX_LEVEL, n_iter=m, early_stop=False)
                T = np.array(r.T_cur_w)
                seen = int(r.n_residual_patches)
            now, n_inside = outside_level(fp, MAX_LEVEL, T)
            r1 = orc.sparse_img_align(fp, max_level=MAX_LEVEL, min_level=MAX_LEVEL, n_iter=m + 1, early_stop=False)
            assert int(r1.n_residual_patches) - seen == n_inside, (a, m, int(r1.n_residual_patches) - seen, n_inside)
            changed = now != before
            for p in range(4):
                counts[a, 0 if m == 0 else 1, p] += int((changed & (pos == p)).sum())
            before = now
    return counts


def solve_all(ctx, fps, n_pairs, extra_lds=None, keep=None):
    """fps repeated over n_pairs slots, uploaded once -> {"<levels>_<stop>_<reduction>": uint64 [keep or n_pairs][WORDS]}; with
    keep, every further pair must repeat the record of the frame it carries"""
    cam = fps[0].cam
    ref = hip.Pyramid(ctx, cam.width, cam.height, 5, n_pairs)
    cur = hip.Pyramid(ctx, cam.width, cam.height, 5, n_pairs)
    sia = hip.SparseImgAlign(ctx, n_pairs, max(len(fp.px) for fp in fps))
    out = {}
    try:
        sia.set_frames(ref, cur)
        if extra_lds is not None:
            sia.set_option(hip.SIA_OPT_EXTRA_LDS, extra_lds)
        for i in range(n_pairs):
            fp = fps[i % len(fps)]
            ref.upload(i, fp.ref_pyr)
            cur.upload(i, fp.cur_pyr)
        for lname, min_level in LEVELS:
            for sname, early in STOPS:
                for rname, red in REDUCTIONS:
                    sia.set_option(hip.SIA_OPT_REDUCTION, red)
                    for i in range(n_pairs):
                        sia.upload_pair(i, fps[i % len(fps)])
                    sia.run(n_pairs, sia.params(max_level=MAX_LEVEL, min_level=min_level, n_iter=N_ITER, eps=1e-6, early_stop=early))
                    assert sia.last_run_mode() == 1, "not a run of the fused kernel"
                    res = sia.download_all(n_pairs)
                    n_keep = keep or n_pairs
                    rows = [paths.result_words(r, *sia.download_last_step(i)) for i, r in enumerate(res[:n_keep])]
                    for i in range(n_keep, n_pairs):             # (on the fields of svo_hip_sia_result)
                        again = paths.result_words(res[i], ZERO6, ZERO6)[:-12]
                        assert np.array_equal(again, rows[i % len(fps)][:-12]), "pair %d differs from its frame's first" % i
                    out["%s_%s_%s" % (lname, sname, rname)] = np.stack(rows)
        return out
    finally:
        for o in (sia, ref, cur):
            o.destroy()


def settings():
    return ["%s_%s_%s" % (l, s, r) for l, _ in LEVELS for s, _ in STOPS for r, _ in REDUCTIONS]


def case_names():
    names = ["n%d_%s" % (n, s) for n in NS for s in settings()]
    names += ["n%d_noextra_%s" % (n, s) for n in NS_EXTRA for s in settings()]
    names += ["out%d_%s" % (a, s) for a in range(len(OUT_POSES)) for s in settings()]
    return names + ["many_n%d_x%d_%s" % (MANY_N, MANY_PAIRS, s) for s in settings()]


def run_cases(ctx):
    """{case name: uint64 [pairs][WORDS]} for every case of the fixture"""
    out = {}
    for n in NS:
        fps = [make_pair(n), make_pair(n, 1)]
        out.update({"n%d_%s" % (n, s): w for s, w in solve_all(ctx, fps, 2).items()})
        if n in NS_EXTRA:
            out.update({"n%d_noextra_%s" % (n, s): w for s, w in solve_all(ctx, fps, 2, extra_lds=0).items()})
    for a, fp in enumerate(out_pairs()):
        # (the pose under test in both slots next to an ordinary pair: three pairs per launch)
        out.update({"out%d_%s" % (a, s): w for s, w in solve_all(ctx, [fp, make_pair(OUT_N), fp], 3).items()})
    distinct = [make_pair(MANY_N, 10 + v) for v in range(MANY_DISTINCT)]
    out.update({"many_n%d_x%d_%s" % (MANY_N, MANY_PAIRS, s): w
                for s, w in solve_all(ctx, distinct, MANY_PAIRS, keep=MANY_DISTINCT).items()})
    assert sorted(out) == sorted(case_names())
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    counts = out_changes()
    print("patches whose outside-the-image state changes, [pose][first / later evaluation][tile position]:\n%s" % counts)
    assert (counts > 0).all(), "a pose leaves a tile position without a change"
    ctx = hip.Context(0)
    cases = run_cases(ctx)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **cases, **{COUNTS_KEY: counts})
    print("recorded %d cases (%d result records) -> %s, %d bytes" % (len(cases), sum(len(v) for v in cases.values()), path,
                                                                    os.path.getsize(path)))


if __name__ == "__main__":
    main()
