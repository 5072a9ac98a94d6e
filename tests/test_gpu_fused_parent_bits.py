"""The fused SparseImgAlign kernel against a recording of its own results, bit for bit.

tests/golden/sia_fused_parent_bits.npz was written by tools/record_sia_fused_bits.py with the library of the commit before
the kernel's scalar state, the pre-doubled quaternion and the once-halved weights were reworked -- changes that reorder no
sum and round nothing differently, so every field of svo_hip_sia_result has to keep its bits.  The cases are the tool's:
one-pair launches on 160 x 120 images (levels 2..0, 4 evaluations, fixed work and the reference's exits) with one frame per
tiles-per-wave class of the launcher (5, 64, 130, 600, 1100, 1600, 2000 and 2600 patches), under the default and the
tile-order sums, and one 600-pair launch of 130-patch frames for the 4-wave shape.

The recorded bits are tied to the ROCm version that recorded them (ROCm 7.2.0 here: its device library's sqrt and division
and its compiler's code for the one-lane solve).  After a toolchain change that moves them, record again with the unchanged
library sources and say so in the commit."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))

import record_sia_fused_bits as rec  # noqa: E402

CASES = ["one_n%d_%s_%s" % (n, s, r) for n in rec.NS for s, _ in rec.STOPS for r, _ in rec.REDUCTIONS] + \
        ["many_n%d_x%d" % (rec.MANY_N, rec.MANY_PAIRS)]


@pytest.fixture(scope="module")
def got():
    from android_svo_amd import hip
    ctx = hip.Context(0)
    out = rec.run_cases(ctx)
    ctx.close()
    return out


def test_the_fixture_holds_exactly_these_cases(golden):
    assert sorted(golden("sia_fused_parent_bits.npz").files) == sorted(CASES)


@pytest.mark.parametrize("case", CASES)
def test_every_field_keeps_the_recorded_bits(golden, got, case):
    want = golden("sia_fused_parent_bits.npz")[case]
    assert want.dtype == np.uint64 and want.shape == got[case].shape
    assert want.shape[1] == 7 + 1 + 36 + 1 + 1 + 8 + 2                  # every field of svo_hip_sia_result
    differing = np.argwhere(want != got[case])
    assert differing.size == 0, "pairs / words that differ: %s" % differing[:8].tolist()


def test_the_cases_do_something(golden):
    """the guard of the test above: the recorded runs tracked patches, moved the pose and took the evaluations asked for"""
    g = golden("sia_fused_parent_bits.npz")
    for n in rec.NS:
        w = g["one_n%d_fixed_per_wave" % n][0]
        iters = w[46:54].view(np.int64)
        assert list(iters[:3]) == [rec.N_ITER] * 3 and not iters[3:].any()
        assert 0 < int(w[54]) <= 3 * n                                    # patches precomputed over the three levels
        assert int(w[55]) > 0
