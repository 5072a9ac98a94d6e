"""What tests/test_gpu_sia_odd_sizes.py rests on, established with the CPU oracle and tests/sia_odd_cases.py alone:

  * the sizes give odd row strides, level starts that needed rounding and corner patches that end one byte past their level;
  * the oracle accepts every planted feature at the last valid column / row / corner and rejects the one next to it, at both
    sides, in the reference image and (T_cur == T_ref) in the current image;
  * the furthest byte any feature makes the kernels read lies inside the allocation, in the last slot of the batch too;
  * the rendered scenes used for pose parity are well posed on the oracle, the degenerate ones are degenerate."""
import numpy as np
import pytest

import sia_odd_cases as so
from android_svo_amd import synth
from oracle import orc


def test_the_sizes_have_odd_strides_and_rounded_level_offsets():
    assert set(so.SIZES) >= {(346, 260), (202, 134), (100, 68), (346, 261)}
    for w, h in so.SIZES:
        offs, pyr_bytes = so.level_offsets(w, h)
        cols = [w >> l for l in range(so.N_LEVELS)]
        assert any(c % 2 for c in cols[1:4]), cols                                  # a level with an odd stride and room for a patch
        ends = [offs[l] + (w >> l) * (h >> l) for l in range(so.N_LEVELS)]
        assert any(e % 16 for e in ends[:-1])                                       # a level start that had to be rounded up
        assert all(o % 16 == 0 for o in offs) and pyr_bytes % 16 == 0 and pyr_bytes >= ends[-1]
        # rows of an odd-stride level start at every alignment of the 8-byte loads
        l_odd = next(l for l in range(so.N_LEVELS) if cols[l] % 2)
        assert {(offs[l_odd] + r * cols[l_odd]) % 8 for r in range(h >> l_odd)} == set(range(8))
    assert so.patch_levels(346, 260) == so.patch_levels(346, 261) == so.patch_levels(202, 134) == [0, 1, 2, 3, 4]
    assert so.patch_levels(100, 68) == [0, 1, 2, 3]                                 # level 4 is 6x4: no room for a patch
    assert (261 >> 1) == (260 >> 1) and 261 % 2 == 1                                # the odd height: level 0's last row is dropped


@pytest.mark.parametrize("size", so.SIZES, ids=so.size_id)
def test_planted_features_meet_the_limits_on_the_oracle(size):
    w, h = size
    for level in so.patch_levels(w, h):
        fp, n_rand, want = so.noise_case(w, h, level)
        cols, rows = so.level_dims(w, h, level)
        spec = so.planted(w, h, level)
        assert {(cols - 4, rows - 4, 1), (cols - 3, rows - 3, 0), (3, 3, 1), (2, 2, 0)} <= set(spec)
        assert [a for (_, _, a) in spec] == [int(so.accepted(w, h, level, u, v)) for (u, v, _) in spec]
        assert sum(a for (_, _, a) in spec) == 8 and len(spec) == 16
        u, v = so.integer_positions(fp, level)
        np.testing.assert_array_equal(u[n_rand:], np.repeat([s[0] for s in spec], len(so.FRACS)))
        np.testing.assert_array_equal(v[n_rand:], np.repeat([s[1] for s in spec], len(so.FRACS)))
        T_cfr = synth.se3_mul(fp.T_cur_w_init, synth.se3_inv(fp.T_ref_w))
        out28, n_meas, cache, jac, vis = orc.sia_single_eval(fp, level, T_cfr, want_caches=True)
        np.testing.assert_array_equal(vis[n_rand:], want)                           # accepted / rejected exactly at the limits
        rule = np.array([so.accepted(w, h, level, int(a), int(b)) for a, b in zip(u, v)]) & (fp.has_point == 1)
        np.testing.assert_array_equal(vis, rule.astype(np.uint8))
        assert (fp.has_point[:n_rand] == 0).sum() > 10
        # T_cur == T_ref: every patch accepted in the reference image is accepted in the current image, the planted ones at the
        # same limits
        assert n_meas == 16 * int(vis.sum())
        assert np.isfinite(out28).all() and out28[27] > 0
        # the bytes: the bottom-right corner patch ends one byte past its level, and nothing leaves the allocation
        offs, pyr_bytes = so.level_offsets(w, h)
        for slot in (0, so.BATCH - 1):
            last, alloc = so.furthest_read(w, h, level, cols - 4, rows - 4, slot)
            assert last == slot * pyr_bytes + offs[level] + cols * rows
            assert last <= (slot + 1) * pyr_bytes < alloc
            worst = max(so.furthest_read(w, h, level, int(a), int(b), slot)[0] for a, b in zip(u, v))
            assert worst < alloc, (level, slot, worst, alloc)


@pytest.mark.parametrize("size", so.SIZES + (so.WIDE_SHORT,), ids=so.size_id)
def test_loads_of_rejected_patches_stay_inside_the_allocation_at_every_level(size):
    """the full runs visit levels without room for a patch (100x68 level 4 is 6x4, 752x64 level 4 is 47x4): every patch is
    rejected there and its loads go to offset 0 of the level"""
    w, h = size
    offs, pyr_bytes = so.level_offsets(w, h)
    for level in range(so.N_LEVELS):
        for batch in (1, so.BATCH):
            last, alloc = so.furthest_read(w, h, level, 0, 0, batch - 1, batch)
            assert last < alloc, (level, last, alloc)
    last, alloc = so.furthest_read(w, h, 4, 0, 0, 0, 1)
    if size == (100, 68):
        assert last - offs[4] == 43 and pyr_bytes - offs[4] == 32 and last >= pyr_bytes    # it does reach into the tail slack
        assert so.tail_slack(w, h) == 64
    if size == so.WIDE_SHORT:
        # 64 bytes of slack would not hold these loads: svo_hip_pyramid_create allocates what they need
        assert last - offs[4] == 289 and pyr_bytes - offs[4] == 192 and last >= pyr_bytes + 64
        assert so.tail_slack(w, h) == 98 and alloc == pyr_bytes + 98 and last == alloc - 1
    else:
        assert so.tail_slack(w, h) == 64


@pytest.mark.parametrize("case", so.POSE_CASES, ids=so.run_id)
def test_pose_cases_are_well_posed_on_the_oracle(case):
    w, h, mx, mn = case
    fp = so.scene(w, h)
    assert len(fp.px) == so.SCENE_FEATURES
    o = so.oracle_run(w, h, mx, mn)
    T = np.array(o.T_cur_w)
    print("%s: tracked %d, iters %s, %.2e rad from the truth" % (so.run_id(case), o.n_tracked, list(o.iters)[:5], synth.pose_error(T, fp.T_cur_w_true)[0]))
    assert o.n_tracked >= 150
    assert not np.isnan(T).any()
    assert o.iters[mn] < 30                                                        # the finest level stops before its budget
    assert synth.pose_error(T, fp.T_cur_w_true)[0] < 0.02
    assert so.well_posed(o, fp, mn)
    # features within 4 px of the border: patches are rejected at the coarse levels and accepted at the fine ones
    assert 0 < o.n_precompute_patches < (mx - mn + 1) * so.SCENE_FEATURES


@pytest.mark.parametrize("case", so.DEGENERATE_CASES + (so.WIDE_SHORT_CASE,), ids=so.run_id)
def test_degenerate_cases_are_degenerate_on_the_oracle(case):
    w, h, mx, mn = case
    o = so.oracle_run(w, h, mx, mn)
    print("%s: tracked %d, pre %d, stop %d, iters %s, pose %s" % (so.run_id(case), o.n_tracked, o.n_precompute_patches, o.stop, list(o.iters)[:5],
                                                              np.array(o.T_cur_w)))
    assert o.n_tracked == 0
    assert not so.well_posed(o, so.scene(w, h), mn)


def test_ragged_batch_inputs():
    w, h = so.RAGGED_SIZE
    fps = [so.scene(w, h, n) for n in so.RAGGED_FEATURES]
    assert [len(fp.px) for fp in fps] == list(so.RAGGED_FEATURES) == [200, 17, 0]
    assert so.well_posed(so.oracle_run(w, h, 4, 0, 200), fps[0], 0)
