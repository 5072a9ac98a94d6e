"""The fused SparseImgAlign kernel on every way a level can end, bit for bit against a recording of the commit before the
|x| <= eps test moved onto the lanes that hold x and the H comparison onto a lane mask (tools/record_sia_window_exit_bits.py ->
tests/golden/sia_fused_window_exit_parent_bits.npz), and against the CPU oracle.

tests/test_gpu_fused_window_paths.py pins the ways OUT of the serial window (large steps, NaN stops, "error increased",
|x| <= 1e-2); the cases here are the tool's: eps = 0, +inf, a negative value and NaN, fixed work, and the reference's exits on
levels that end by n_iter, each on frames of 40, 1100 and 2600 patches (one, three and six tiles on the older wave of a SIMD)
and in a 600-pair launch of 130-patch frames (the 4-wave shape), under per-wave and tile-order sums.  Every field of
svo_hip_sia_result plus Jres_ and x_ of the last evaluation must keep its recorded bits, in every pair of the 600-pair
launch.  What makes a case what it claims to be is asserted on the CPU oracle: eps = +inf leaves every level after one
evaluation; a negative or NaN eps is never reached and the run is the eps = 0 run, which leaves by "error increased" or by
n_iter; fixed work ends every level by n_iter, and with the reference's exits on at least one level does.  The discrete
fields are held to the oracle, the pose to the tolerance of tests/test_gpu_parity.py.

The recorded bits are tied to the ROCm version that recorded them (see tests/test_gpu_fused_parent_bits.py)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))

import record_sia_window_exit_bits as ex  # noqa: E402
from android_svo_amd import synth         # noqa: E402
from oracle import orc                    # noqa: E402

FIXTURE = "sia_fused_window_exit_parent_bits.npz"
LEVELS = slice(0, 3)


def shape_kind(case):
    shape = max((s for s in ex.SHAPES if case.startswith(s + "_")), key=len)
    kind = max((k for k in ex.KINDS if case[len(shape) + 1:].startswith(k + "_")), key=len)
    return shape, kind


@pytest.fixture(scope="module")
def frames():
    return ex.frames()


@pytest.fixture(scope="module")
def got(frames):
    from android_svo_amd import hip
    ctx = hip.Context(0)
    out = ex.run_cases(ctx, frames)          # (asserts that every pair of the 600-pair launch repeats its frame's record)
    ctx.close()
    return out


@pytest.fixture(scope="module")
def oracle(frames):
    return {(s, k): [orc.sparse_img_align(fp, **ex.params(k)) for fp in frames[s]] for s in ex.SHAPES for k in ex.KINDS}


def test_the_fixture_holds_exactly_these_cases(golden):
    assert sorted(golden(FIXTURE).files) == sorted(ex.CASE_IDS)


@pytest.mark.parametrize("case", ex.CASE_IDS)
def test_every_field_keeps_the_recorded_bits(golden, got, case):
    want = golden(FIXTURE)[case]
    _, words = got[case]
    assert want.dtype == np.uint64 and want.shape == words.shape and words.shape[1] == ex.N_WORDS
    differing = np.argwhere(want != words)
    assert differing.size == 0, "(pair, word) that differ: %s" % differing[:8].tolist()


def test_the_frames_take_the_shapes_they_are_meant_for(frames):
    assert [len(frames[s][0].px) for s in ex.SHAPES[:3]] == [40, 1100, 2600]
    assert all(len(fp.px) == 130 for fp in frames[ex.SHAPES[3]]) and ex.MANY_PAIRS == 600


@pytest.mark.parametrize("shape", ex.SHAPES)
def test_each_case_leaves_its_levels_by_the_rule_it_claims_in_the_oracle(oracle, shape):
    n_iter = ex.N_ITER
    for i, zero in enumerate(oracle[(shape, "eps0")]):
        it0 = list(zero.iters)[LEVELS]
        print(shape, i, "iterations per level with eps = 0:", it0)
        assert zero.stop == 0 and all(1 <= k <= n_iter for k in it0)
        # eps = +inf: |x| <= eps at the first evaluation of every level
        inf = oracle[(shape, "epsinf")][i]
        assert inf.stop == 0 and list(inf.iters)[LEVELS] == [1, 1, 1]
        # a negative or NaN eps (and 1e-300) is never reached by a finite update: the run is the eps = 0 run
        for kind in ("epsneg", "epsnan", "exits_tiny"):
            o = oracle[(shape, kind)][i]
            assert o.stop == 0 and list(o.iters) == list(zero.iters), (shape, kind, i)
            np.testing.assert_array_equal(np.array(o.T_cur_w), np.array(zero.T_cur_w))
        # the n_iter bound ends every level of fixed work
        assert list(oracle[(shape, "fixed")][i].iters)[LEVELS] == [n_iter] * 3
    # with the reference's exits on, some level of the shape ends by the bound -- the done flag set by n_iter, not by an exit --
    # and some level by "error increased" (shorter than n_iter)
    assert any(max(list(o.iters)[LEVELS]) == n_iter for o in oracle[(shape, "eps0")])
    assert any(min(list(o.iters)[LEVELS]) < n_iter for o in oracle[(shape, "eps0")])


@pytest.mark.parametrize("case", ex.CASE_IDS)
def test_discrete_fields_equal_the_oracle_and_the_pose_is_close(got, oracle, case):
    res, _ = got[case]
    for i, (r, o) in enumerate(zip(res, oracle[shape_kind(case)])):
        assert int(r.stop) == int(o.stop), (case, i, r.stop, o.stop)
        assert list(r.iters) == list(o.iters), (case, i, list(r.iters), list(o.iters))
        assert r.n_tracked == o.n_tracked, (case, i, r.n_tracked, o.n_tracked)
        rot, trans = synth.pose_error(np.array(r.T_cur_w), np.array(o.T_cur_w))
        print(case, i, "pose against the oracle: %.3e rad %.3e m" % (rot, trans))
        assert rot < 1e-4 and trans < 1e-3, (case, i, rot, trans)
