"""The fused SparseImgAlign kernel wherever the bookkeeping of its tile loop takes part, bit for bit against a recording of the
commit before the LDS tile plan became a constant in the evaluation (tools/record_sia_fused_tile_slots.py ->
tests/golden/sia_fused_tile_slots_parent_bits.npz): which tile a wave reads from LDS and which from memory, the patches it
counts as measurements, and its note that a tile's outside-the-image set changed.

The cases are the tool's: 640 x 480 images, 4 evaluations per level, levels 4..2 and 4..0, fixed work and the reference's exits,
per-wave and tile-order sums; two-pair launches of frames of 40, 130, 600, 1100, 1600, 2000, 2500 and 2816 patches (one to six
tiles on the older wave of a SIMD; the three- and four-tile shapes with and without their extra LDS tiles), a 600-pair launch
of 130-patch frames (the 4-wave shape), and the 2000-patch frame started from poses that are off sideways.  Every field of
svo_hip_sia_result plus Jres_ and x_ of the last evaluation must keep its recorded bits.

What makes the sideways poses what they claim to be is counted on the CPU oracle (no GPU needed): with each of them, patches
change their outside-the-image state at the first evaluation of the coarsest level and at a later one on each of the four tile
positions of a wave -- 0 and 2 are LDS tiles, 1 and 3 memory tiles -- and the counts are those stored with the recording.

The recorded bits are tied to the ROCm version that recorded them (see tests/test_gpu_fused_parent_bits.py)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))

import record_sia_fused_tile_slots as rec  # noqa: E402

FIXTURE = "sia_fused_tile_slots_parent_bits.npz"
CASES = rec.case_names()


@pytest.fixture(scope="module")
def got():
    from android_svo_amd import hip
    ctx = hip.Context(0)
    out = rec.run_cases(ctx)      # (asserts that every pair of the 600-pair launch repeats its frame's record)
    ctx.close()
    return out


def test_the_fixture_holds_exactly_these_cases(golden):
    assert sorted(golden(FIXTURE).files) == sorted(CASES + [rec.COUNTS_KEY])


def test_the_frames_take_every_tiles_per_wave_class():
    """the launcher's tile map (launch_fused_shape in svo_sia.hip): tiles of the older wave of a SIMD"""
    tpw = [(((-(-n // 64)) + 3) // 4 + 1) // 2 for n in rec.NS]
    assert tpw == [1, 1, 2, 3, 4, 4, 5, 6]
    assert rec.NS[-1] == 44 * 64                                   # the largest frame the kernel takes
    assert all(t in (3, 4) for t, n in zip(tpw, rec.NS) if n in rec.NS_EXTRA)
    # the frame of the sideways poses fills its shape: four tiles on every wave, so a patch's tile position is tile_position()
    assert -(-rec.OUT_N // 64) == 32
    assert rec.MANY_PAIRS >= 512 and -(-rec.MANY_N // 64) <= 4     # at least two pairs per CU, one tile per wave: 4 waves


def test_each_sideways_pose_moves_patches_out_on_every_tile_position(golden):
    counts = rec.out_changes()
    print("patches whose outside-the-image state changes, [pose][first / later evaluation][tile position]:\n%s" % counts)
    assert counts.shape == (len(rec.OUT_POSES), 2, 4)
    assert (counts >= 1).all()
    np.testing.assert_array_equal(counts, golden(FIXTURE)[rec.COUNTS_KEY])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_every_field_keeps_the_recorded_bits(golden, got, case):
    want = golden(FIXTURE)[case]
    words = got[case]
    assert want.dtype == np.uint64 and want.shape == words.shape and words.shape[1] == rec.WORDS
    differing = np.argwhere(want != words)
    assert differing.size == 0, "(pair, word) that differ: %s" % differing[:8].tolist()


@pytest.mark.gpu
def test_the_cases_are_not_degenerate(got):
    """every launch tracked patches and finished its levels; the two slots of a sideways pose agree with each other"""
    for case, words in got.items():
        assert (words[:, 7] > 0).all(), (case, "n_tracked")
        if case.startswith("out"):
            assert np.array_equal(words[0], words[2]), case
