"""The conditions tests/test_gpu_seed_arithmetic.py and tests/test_gpu_odd_pyramids.py rest on, established with the CPU
oracle and tests/seed_reference.py alone -- so that the GPU tests cannot pass vacuously:

  * on every updateSeed input family the typed numpy evaluation (behind the reference's NaN guard) reproduces the oracle
    to the bit on at least 99.9 % of the seeds (observed: all of them), the life family reaches the regime where
    sigma2 = E[x^2] - mu^2 cancels below zero, every special block does what seed_reference.SPECIAL_BLOCKS says;
  * on every computeTau family the NaN pattern of the oracle equals that of a numpy float64 evaluation, and the
    degenerate families are degenerate (NaN shares);
  * the finalize-glue scenes take the clamp branch, converge and merely update at least 300 seeds in every frame;
  * every odd-pyramid depth-filter scene covers the statuses, the multi-chunk search and the direct-align path."""
import numpy as np
import pytest

import seed_reference as sr


@pytest.mark.parametrize("family", ["life", "fresh"])
def test_typed_evaluation_reproduces_the_oracle_on_the_families(family):
    args = {"life": sr.gen_life, "fresh": sr.gen_fresh}[family]()
    assert len(args[0]) == 40000 and all(v.dtype == np.float32 for v in args)
    o = sr.oracle_update_seed(*args)
    np.testing.assert_array_equal(o[3], args[5])                                   # z_range is never written
    got = sr.update_seed_guarded(*args)
    same = sr.state_same_bits(got, (o[0], o[1], o[2], o[4]))
    assert same.mean() >= 0.999, same.mean()                                       # observed: 40 000 of 40 000
    sr.assert_remainder_close(got, (o[0], o[1], o[2], o[4]), same, family)
    with np.errstate(all="ignore"):
        e = [v.astype(np.float64) for v in sr.update_seed_exact(*args)]
    ok = np.isfinite(e[0]) & np.isfinite(e[2]) & np.isfinite(e[3]) & (e[3] > 0)
    assert ok.mean() > 0.99                                                        # the calibrated bound has its samples
    if family == "life":
        x, tau2, a, b, mu, z_range, sigma2 = args
        sig = np.sqrt(sigma2.astype(np.float64))
        assert (sig < z_range / 200.0).mean() > 0.1 and (sig > z_range / 10.0).mean() > 0.1     # both sides of convergence
        assert (np.abs(x - mu) > 30 * np.sqrt(sigma2.astype(np.float64) + tau2)).mean() > 0.1   # outliers tens of sigma away
        assert 0.002 < (o[4] < 0).mean() < 0.02, (o[4] < 0).mean()                 # the cancellation regime (observed 0.6 %)
        assert a.min() < 1e-2 and a.max() > 1e2 and tau2.min() < 1e-9 and tau2.max() > 0.1


def test_special_blocks_on_the_oracle():
    args, blocks = sr.gen_special()
    assert len(blocks) == 15 and all(sl.stop - sl.start >= 256 for _, _, _, sl in blocks)
    o = sr.oracle_update_seed(*args)
    out4 = (o[0], o[1], o[2], o[4])
    sr.check_special_blocks(args, blocks, out4, "oracle")
    got = sr.update_seed_guarded(*args)
    sr.check_special_blocks(args, blocks, got, "typed")
    assert sr.state_same_bits(got, out4).all()                                     # every block bit-equal behind the guard
    with np.errstate(all="ignore"):
        unguarded = sr.update_seed_typed(*args)
    assert not sr.state_same_bits(unguarded, out4)[blocks[0][3]].any()             # ... and the guard is what does it


@pytest.mark.parametrize("family", sr.TAU_FAMILIES)
def test_tau_families_nan_pattern_on_the_oracle(family):
    t, f, z = sr.tau_flat(*sr.gen_tau(family))
    assert len(z) >= 20000
    np.testing.assert_allclose(np.linalg.norm(f, axis=1), 1.0, rtol=0, atol=1e-15)
    o = sr.oracle_compute_tau(t, f, z, sr.PX_ERROR_ANGLE)
    with np.errstate(all="ignore"):
        d = sr.compute_tau_np(t, f, z, sr.PX_ERROR_ANGLE, np.float64)
    np.testing.assert_array_equal(np.isnan(o), np.isnan(d))
    assert not np.isinf(o).any()
    share = np.isnan(o).mean()
    lo, hi = {"wide": (0.0, 0.0), "t_par_f": (0.02, 0.2), "t_eq_cf": (0.2, 0.8), "t_zero": (1.0, 1.0), "at_camera": (0.2, 0.8)}[family]
    assert lo <= share <= hi, share                       # observed 0, 6.7 %, 48 %, 100 %, 49 %
    if family != "t_zero":
        fin = ~np.isnan(o)
        err = np.abs(o - d)[fin] / (np.abs(o[fin]) + z[fin])
        assert np.percentile(err, 99.9) < 1e-10 and err.max() < 1e-7, (np.percentile(err, 99.9), err.max())
    if family == "wide":
        assert 0.1 < (o < 0).mean() < 0.9                 # both signs of tau occur


@pytest.mark.parametrize("baseline", sr.GLUE_BASELINES)
def test_glue_scene_branch_counts(baseline):
    sc = sr.glue_case(baseline)
    assert len(sc.px) == 2048 and sc.cam.width == 320 and sc.cam.height == 240
    state = (sc.a, sc.b, sc.mu, sc.sigma2)
    for frame in range(sr.GLUE_FRAMES):
        o, state = sr.oracle_pass(sc, state)
        counts = np.bincount(o["status"], minlength=6)
        n_clamp = int(sr.clamp_mask(sc, o).sum())
        assert counts[4] >= 300 and counts[3] >= 300, (frame, counts)              # converged / merely updated
        if baseline == 0.004:
            assert n_clamp >= 300, (frame, n_clamp)                                # observed 588 .. 618
        else:
            assert n_clamp == 0                                                    # the ordinary baseline never clamps


@pytest.mark.parametrize("size", sr.ODD_SIZES)
def test_odd_pyramid_scene_branch_counts(size):
    oc = sr.odd_df_case(*size)
    sc = oc.sc
    assert 1500 <= len(sc.px) <= 3000
    shapes = [im.shape[::-1] for im in sc.ref_pyr]
    assert shapes[0] == size and len(shapes) == 5 and any(w % 2 for w, _ in shapes[1:3])   # an odd row stride on a seed level
    o, _ = sr.oracle_pass(sc, (sc.a, sc.b, sc.mu, sc.sigma2), T_cur_w=oc.T_cur_w)
    counts, n_multi, n_direct = sr.odd_branch_counts(o)
    assert (counts[:4] >= sr.ODD_MIN_STATUS).all(), counts
    assert n_multi >= sr.ODD_MIN_MULTI and n_direct >= sr.ODD_MIN_DIRECT, (n_multi, n_direct)
    # matches land within a patch of the image edge, on every level the search runs on
    upd = o["status"] >= 3
    px = o["px_cur"][upd]
    edge = np.minimum(np.minimum(px[:, 0], size[0] - 1 - px[:, 0]), np.minimum(px[:, 1], size[1] - 1 - px[:, 1]))
    for lvl in np.unique(o["search_level"][upd]):
        at = o["search_level"][upd] == lvl
        assert (edge[at] < 10 * (1 << int(lvl))).any(), (lvl, edge[at].min())
