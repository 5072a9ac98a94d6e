"""The fused SparseImgAlign kernel on every way out of the serial window between an evaluation's two barriers, bit for bit
against a recording of the commit before the window's large-angle branch became a self-contained cold function and its
scalars stopped living across the two cold calls (tools/record_sia_window_bits.py ->
tests/golden/sia_fused_window_parent_bits.npz), and against the CPU oracle.

The recording of tests/test_gpu_fused_parent_bits.py is four evaluations of ordinary frames: small update angles, H
unchanged after the first evaluation of a level, no exit.  The cases here are the tool's -- large_* (theta^2 > 0.25; one of
them in a 2600-feature frame, for the large-angle branch of the shapes with five and six tiles per wave), nan_*
(stop_ and rollback; theta == 0), exits_* ("error increased" and |x| <= eps), fixed_* (H factored again) -- each under
per-wave and tile-order sums, on 160 x 120 images.  Every field of svo_hip_sia_result plus Jres_ and x_ of the last
evaluation must keep its recorded bits.  What makes a case what it claims to be is asserted on the CPU oracle, so that a
change to the synthetic frames cannot quietly take a case off its path; exits_* and fixed_* must also agree with the oracle
(stop, iters, tracked patches; pose within the tolerance of tests/test_gpu_parity.py), large_* and nan_* in the discrete
fields only: the reference wanders there.

The recorded bits are tied to the ROCm version that recorded them (see tests/test_gpu_fused_parent_bits.py)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))

import record_sia_window_bits as win  # noqa: E402
from android_svo_amd import synth     # noqa: E402
from oracle import orc                # noqa: E402

FIXTURE = "sia_fused_window_parent_bits.npz"
IDS = ["%s_%s" % (n, r) for n in win.CASE_NAMES for r, _ in win.REDUCTIONS]
LARGE = [n for n in win.CASE_NAMES if n.startswith("large_")]
N_RESULT_WORDS = win.N_WORDS - 12                         # then Jres_ (6) and x_ (6)


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in win.cases()}


@pytest.fixture(scope="module")
def got(cases):
    from android_svo_amd import hip
    ctx = hip.Context(0)
    out = win.run_cases(ctx, list(cases.values()))
    ctx.close()
    return out


@pytest.fixture(scope="module")
def oracle(cases):
    return {c.name: orc.sparse_img_align(c.fp, **c.prm) for c in cases.values()}


def test_the_fixture_holds_exactly_these_cases(golden):
    assert sorted(golden(FIXTURE).files) == sorted(IDS)


@pytest.mark.parametrize("case", IDS)
def test_every_field_keeps_the_recorded_bits(golden, got, case):
    want = golden(FIXTURE)[case]
    _, words = got[case]
    assert want.dtype == np.uint64 and want.shape == words.shape == (win.N_WORDS,)
    differing = np.flatnonzero(want != words)
    assert differing.size == 0, "words that differ: %s" % differing[:8].tolist()


@pytest.mark.parametrize("name", LARGE)
def test_large_cases_take_a_large_step_in_the_oracle(cases, name):
    """some update of the oracle's run turns the pose by more than 0.5 rad: theta^2 > 0.25, the library path of SE3::exp"""
    case = cases[name]
    poses = [np.array(case.fp.T_cur_w_init)]
    for k in range(1, case.prm["n_iter"] + 1):
        poses.append(np.array(orc.sparse_img_align(case.fp, **dict(case.prm, n_iter=k)).T_cur_w))
    steps = [synth.pose_error(a, b)[0] for a, b in zip(poses[1:], poses[:-1])]
    print("rotation per evaluation [rad]:", ["%.3f" % s for s in steps])
    assert np.isfinite(steps).all() and max(steps) > 0.5


@pytest.mark.parametrize("case", ["%s_%s" % (n, r) for n in LARGE for r, _ in win.REDUCTIONS])
def test_large_cases_take_a_large_step_on_the_device(got, case):
    """... and the kernel's own last update is one: |omega|^2 of the x_ it reports is above 0.25"""
    x = got[case][1][N_RESULT_WORDS + 6:].view(np.float64)
    theta2 = float(x[3] * x[3] + x[4] * x[4] + x[5] * x[5])
    print(case, "theta^2 of the last update: %.3f" % theta2)
    assert theta2 > 0.25


def test_the_padded_large_case_runs_the_six_tile_shape(cases):
    assert len(cases["large_n12_of_2600"].fp.px) == 2600 and int(cases["large_n12_of_2600"].fp.has_point.sum()) == 12


def test_nan_cases_stop_in_the_oracle(cases, oracle):
    for c in cases.values():
        if c.name.startswith("nan_overflow"):
            o = oracle[c.name]
            assert o.stop == 1 and list(o.iters)[:3] == [1, 1, 1]           # isnan(x[0]) at the first evaluation of every level
            np.testing.assert_array_equal(np.array(o.T_cur_w), win.IDENTITY)   # ... and the pose rolled back each time
    assert np.isnan(np.array(oracle["nan_one_patch"].T_cur_w)[:3]).all()      # theta == 0: the reference's 0/0


def test_exit_cases_leave_early_in_the_oracle(cases, oracle):
    for c in cases.values():
        if c.kind == "exits":
            o = oracle[c.name]
            levels = list(o.iters)[c.prm["min_level"]:c.prm["max_level"] + 1]
            assert o.stop == 0 and min(levels) < c.prm["n_iter"], (c.name, levels)
            if c.prm["eps"] > 0:
                # the first (coarsest) level follows the eps = 0 run of the same frame until one of them leaves, and eps = 0
                # leaves only when the error increases: leaving earlier than that run is leaving by |x| <= eps
                top = c.prm["max_level"]
                assert o.iters[top] < oracle[c.name.replace("_eps_", "_worse_")].iters[top], (c.name, levels)


@pytest.mark.parametrize("case", IDS)
def test_discrete_fields_equal_the_oracle_and_the_pose_where_it_is_stable(cases, got, oracle, case):
    c = cases[max((n for n in cases if case.startswith(n + "_")), key=len)]
    r, _ = got[case]
    o = oracle[c.name]
    assert int(r.stop) == int(o.stop), (case, r.stop, o.stop)
    assert list(r.iters) == list(o.iters), (case, list(r.iters), list(o.iters))
    assert r.n_tracked == o.n_tracked, (case, r.n_tracked, o.n_tracked)
    if c.kind in ("exits", "fixed"):
        rot, trans = synth.pose_error(np.array(r.T_cur_w), np.array(o.T_cur_w))
        print(case, "pose against the oracle: %.3e rad %.3e m" % (rot, trans))
        assert rot < 1e-4 and trans < 1e-3, (case, rot, trans)
