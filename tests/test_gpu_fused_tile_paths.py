"""The paths of the fused SparseImgAlign kernel's tile loop that its scalar bookkeeping decides, against a recording, bit for bit.

tests/golden/sia_fused_tile_paths_parent_bits.npz was written by tools/record_sia_tile_paths_bits.py with the library of the
commit before the tile loop's priority schedule, its outside-the-image bookkeeping and the code behind the loop were
reworked -- changes that touch no arithmetic operation, no summation order and no barrier, so every field of
svo_hip_sia_result and Jres_ / x_ of the last evaluation have to keep their bits.  The cases are the tool's (160 x 120 images,
levels 2..0, 4 evaluations, fixed work and the reference's exits, per-wave and tile-order sums):

  * tile counts that leave waves a tile short and tile counts that fill the 1-, 2-, 3- and 4-tile shapes exactly, alone and
    as small frames riding in a larger frame's launch, so that a wave's number of tiles takes every value from 0 to the
    shape's tiles per wave, on older and on younger waves of a SIMD;
  * frames started several pixels off, whose in-image patch set changes between two evaluations of one level (shown on the
    CPU oracle below);
  * one 600-pair launch of 130-patch frames: the 4-wave shape.

The recorded bits are tied to the ROCm version that recorded them (ROCm 7.2.0 here); see tests/test_gpu_fused_parent_bits.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))

import record_sia_tile_paths_bits as rec  # noqa: E402

FIXTURE = "sia_fused_tile_paths_parent_bits.npz"
CASES = rec.case_names()


@pytest.fixture(scope="module")
def got():
    from android_svo_amd import hip
    ctx = hip.Context(0)
    out = rec.run_cases(ctx)
    ctx.close()
    return out


def _tiles_on_waves(n_shape, n):
    """(tiles an older wave has, tiles a younger wave has) per SIMD for a frame of n patches in the 8-wave shape that a launch
    whose largest frame has n_shape patches takes (launch_fused_shape / tile_of in svo_sia.hip)"""
    per_simd = (-(-n_shape // 64) + 3) // 4
    tpw = (per_simd + 1) // 2
    tiles = -(-n // 64)
    old = [sum(1 for k in range(tpw) if s + 4 * k < tiles) for s in range(4)]
    young = [sum(1 for k in range(per_simd - tpw) if s + 4 * (tpw + k) < tiles) for s in range(4)]
    return tpw, per_simd - tpw, old, young


def test_every_tile_count_of_a_wave_occurs():
    """the guard of the tile-count cases: what the frames were chosen for, worked out from the launcher's tile map"""
    seen = {}
    for n in rec.NS_SHORT + rec.NS_FULL:
        tpw, ty, old, young = _tiles_on_waves(n, n)
        seen.setdefault(tpw, [set(), set()])
        seen[tpw][0].update(old)
        seen[tpw][1].update(young)
    for n_shape, small in rec.MIXED.items():
        for n in small:
            tpw, ty, old, young = _tiles_on_waves(n_shape, n)
            seen[tpw][0].update(old)
            seen[tpw][1].update(young)
    assert sorted(seen) == [1, 2, 3, 4]
    for tpw, (old, young) in seen.items():
        assert old == set(range(tpw + 1)), (tpw, old)            # an older wave with 0, 1, ..., all of its tiles
        assert young >= {0, 1} and max(young) == tpw, (tpw, young)   # a younger wave short of a tile, and a full one
    for n in rec.NS_FULL:                                            # the full frames fill their shape exactly
        tpw, ty, old, young = _tiles_on_waves(n, n)
        assert old == [tpw] * 4 and young == [ty] * 4 and ty == tpw


def test_the_drift_frames_change_their_in_image_set_between_evaluations():
    """no GPU needed: the oracle, run on one level with 1, 2, 3 and 4 evaluations, counts different numbers of in-image patches
    in evaluations after the first one -- the set changes between two evaluations of a level, not only when the level starts"""
    from oracle import orc
    changed = 0
    for (n, _, _), fp in zip(rec.DRIFT, rec.drift_pairs()):
        total = [0]
        for m in range(1, rec.N_ITER + 1):
            r = orc.sparse_img_align(fp, max_level=rec.MAX_LEVEL, min_level=rec.MAX_LEVEL, n_iter=m, early_stop=False)
            total.append(int(r.n_residual_patches))
        per_evaluation = np.diff(total)
        assert (per_evaluation > 0).all()
        if len(set(per_evaluation[1:].tolist())) > 1:               # evaluations 2, 3, 4 see different sets
            changed += 1
    assert changed >= 2


def test_the_fixture_holds_exactly_these_cases(golden):
    assert sorted(golden(FIXTURE).files) == sorted(CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_every_field_keeps_the_recorded_bits(golden, got, case):
    want = golden(FIXTURE)[case]
    assert want.dtype == np.uint64 and want.shape == got[case].shape
    assert want.shape[1] == rec.WORDS                                   # svo_hip_sia_result, Jres_, x_
    differing = np.argwhere(want != got[case])
    assert differing.size == 0, "pairs / words that differ: %s" % differing[:8].tolist()


def test_the_cases_do_something(golden):
    """the guard of the test above: the recorded runs tracked patches, took the evaluations asked for and left a last step"""
    g = golden(FIXTURE)
    for n in rec.NS_SHORT + rec.NS_FULL:
        w = g["tiles_n%d_fixed_per_wave" % n][0]
        iters = w[46:54].view(np.int64)
        assert list(iters[:3]) == [rec.N_ITER] * 3 and not iters[3:].any()
        assert 0 < int(w[54]) <= 3 * n and int(w[55]) > 0
        assert np.isfinite(w[56:68].view(np.float64)).all() and w[56:68].any()
    many = g["many_n%d_x%d" % (rec.MANY_N, rec.MANY_PAIRS)]
    assert many.shape == (rec.MANY_PAIRS, rec.WORDS)
    assert np.array_equal(many[:rec.MANY_DISTINCT, :56], many[rec.MANY_DISTINCT:2 * rec.MANY_DISTINCT, :56])
