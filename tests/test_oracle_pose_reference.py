"""CPU only: the conditions tests/test_gpu_pose_refine.py rests on, proved on the oracle and the extended-precision
reference of tests/pose_reference.py alone -- every input family reaches the regime it is named for, oracle and reference
take the same number of iterations and make the same outlier decisions in every well-posed case, the oracle's distance
to the reference (which sets the GPU test's bounds) stays far below what a wrong operand produces, no committed seed is
excluded as undecidable, and the shared assertions reject three deliberately wrong stand-ins for a device result.

The oracle's largest distance to the reference per family, measured here (pose in rad / m, the others relative; the
table of DESIGN.md "Pose refinement: size classes and their tests" holds the kernel's beside it):

  family        rot       trans     error_init  error_final  cov
  classes       1.5e-16   2.1e-16   2.0e-14     1.0e-13      2.8e-14
  class_count   6.3e-17   2.6e-16   2.0e-14     7.6e-14      1.7e-14
  ties          4.2e-17   1.4e-16   8.4e-15     1.5e-13      3.7e-14
  threshold     3.6e-17   1.2e-16   1.1e-14     6.1e-15      1.1e-14
  exits         1.2e-16   2.8e-16   2.6e-15     7.2e-14      1.2e-14
  large_steps   4.2e-17   7.5e-17   3.0e-16     1.8e-13      1.3e-14
  perfect       2.2e-17   4.8e-17   -           -            -"""
import dataclasses

import numpy as np
import pytest

import pose_reference as pr

WELL_POSED = ("classes", "class_count", "ties", "threshold", "exits", "large_steps", "perfect")


def _all(name):
    cases, refs = pr.family(name)
    return cases, refs, pr.oracle_family(name)


def _find(name, text):
    cases, refs, orcs = _all(name)
    k = [c.name for c in cases].index(text)
    return cases[k], refs[k], orcs[k]


# ---- every family reaches its regime ---------------------------------------------------------------------------------
def test_classes_sit_on_both_sides_of_every_split():
    cases, refs = pr.family("classes")
    sizes = sorted({len(c.level) for c in cases})
    assert sizes == sorted(pr.CLASS_SIZES)
    for lo in (64, 128, 256, 2048):                              # block_rank_select 4|2|1, rank|radix, register cache|workspace
        assert lo in sizes and lo + 1 in sizes
    assert all(r.result.ran == 1 for r in refs)
    beyond = [c for c in cases if len(c.level) > 2048]
    assert all(c.has_point[2048:].any() for c in beyond)         # the workspace path holds observations


def test_class_count_cases_are_what_they_say():
    cases, refs = pr.family("class_count")
    n_obs = {c.name: c.n_obs for c in cases}
    assert n_obs["class_count n=256 with 3 observations"] == 3 and n_obs["class_count n=257 with 8 observations"] == 8
    c = cases[2]
    assert len(c.level) == 2600 and not c.has_point[:2048].any() and c.n_obs > 400
    c = cases[3]
    assert len(c.level) == 2600 and not c.has_point[2048:].any() and c.n_obs > 1500
    c = cases[4]
    assert len(c.level) == 300 and not c.has_point[[0, 256]].any() and c.n_obs > 250


def test_ties_put_all_three_medians_inside_runs_of_equal_keys():
    cases, refs = pr.family("ties")
    assert {len(c.level) for c in cases} == {64, 129, 300, 2305}
    assert {c.n_obs % 2 for c in cases} == {0, 1}
    for c, r in zip(cases, refs):
        assert min(r.tie_runs) >= 2, (c.name, r.tie_runs)


def test_threshold_family_works_near_the_outlier_threshold():
    cases, refs = pr.family("threshold")
    for c, r in zip(cases[:-1], refs[:-1]):
        assert c.n_obs == 545 and 80 <= r.result.n_deleted <= 100, (c.name, r.result.n_deleted)
        assert r.thresh_dist.min() < 5e-3, (c.name, r.thresh_dist.min())
    c, r = cases[-1], refs[-1]
    entry = c.has_point != 0
    close = entry & (r.thresh_dist < 1e-6)
    assert (close & (r.result.has_point == 0)).sum() >= 3 and (close & (r.result.has_point != 0)).sum() >= 3
    assert not r.near_thresh.any()                               # and every one of them is still decidable


def test_every_exit_occurs():
    cases, refs = pr.family("exits")
    kinds = {r.exit for r in refs}
    assert kinds == {"converged", "chi2", "n_iter"}
    chi2 = [r for c, r in zip(cases, refs) if "all outliers" in c.name and r.exit == "chi2"]
    assert len(chi2) >= 3 and all(r.result.n_iter_done == 7 for r in chi2)      # after the scale switch at iteration 5
    done = {c.n_iter: r.result.n_iter_done for c, r in zip(cases, refs) if c.name.startswith("exits n_iter=")}
    assert done == {0: 0, 1: 1, 5: 5, 6: 6, 10: done[10]} and 6 < done[10] <= 10
    deleted = {c.reproj_thresh: r.result.n_deleted for c, r in zip(cases, refs) if "reproj_thresh" in c.name}
    assert deleted[1e9] == 0 < deleted[2.0] < deleted[0.5]
    (c,), (r,) = pr.family("perfect")
    assert r.exit == "converged" and r.result.n_iter_done == 1 and r.result.n_deleted == 0
    assert r.result.error_final * 0 == 0 and r.result.error_final < 1e-10        # rounding noise


def test_large_steps_lie_on_both_sides_of_the_series_limit():
    cases, refs = pr.family("large_steps")
    th = np.array([t for r in refs for t in r.theta_sq])
    assert (th > 0.25).any() and ((th > 0.05) & (th <= 0.25)).sum() >= 3, th
    assert all(r.exit == "converged" for r in refs)


# ---- the oracle against the reference --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WELL_POSED + ("ill_posed",))
def test_oracle_passes_the_exact_and_discrete_checks(name):
    for c, r, o in zip(*_all(name)):
        pr.check_exact(c, r, o)
        if c.well_posed:
            assert o.n_iter_done == r.result.n_iter_done, c.name
            pr.check_discrete(c, r, o)


def test_ill_posed_cases_are_ill_posed():
    cases, refs = pr.family("ill_posed")
    assert [c.n_obs for c in cases[:3]] == [1, 2, 3] and not any(c.well_posed for c in cases)


def test_oracle_distance_sets_bounds_that_bite(capsys):
    """The bound of a family is MARGIN x max(the oracle's distance, FLOOR).  It has to stay below what a wrong operand
    produces -- 1e-12 in the pose for a dropped inlier at these sizes -- or the GPU test proves nothing."""
    rows = []
    for name in WELL_POSED:
        cases, refs, orcs = _all(name)
        worst = pr.family_distances(cases, refs, orcs)
        bounds = pr.family_bounds(cases, refs, orcs)
        rows.append("%-12s " % name + " ".join("%s %.1e" % (k, worst[k]) for k in pr.QUANTITIES if k in worst))
        assert bounds["rot"] < 1e-14 and bounds["trans"] < 1e-14, (name, bounds)
        for k in ("error_init", "error_final", "cov"):
            assert k not in bounds or bounds[k] < 1e-11, (name, k, bounds[k])
        for c, r, o in zip(cases, refs, orcs):
            pr.check_continuous(c, r, o, bounds, o)              # the oracle is inside its own bounds, n_iter = 0 included
    with capsys.disabled():
        print("\noracle against the extended reference, largest distance per family:\n  " + "\n  ".join(rows))


def test_exclusion_cap():
    for name in WELL_POSED:
        cases, refs = pr.family(name)
        excluded, n = pr.exclusion_cap(cases, refs)
        assert excluded <= 1 and excluded <= 0.05 * n, (name, excluded, n)
        assert excluded == 0, (name, "the committed seeds keep every case decidable")
    cases, refs = pr.family("threshold")
    for c, r in zip(cases, refs):
        assert r.near_thresh.sum() <= 0.01 * c.n_obs and r.near_thresh.sum() == 0, c.name


# ---- the assertions bite: three wrong stand-ins for a device result --------------------------------------------------
def test_standin_with_one_inlier_dropped_from_the_sums_fails():
    c, r, o = _find("classes", "classes n=257 null_every=0")
    cases, refs, orcs = _all("classes")
    bounds = pr.family_bounds(cases, refs, orcs)
    inlier = int(np.where((c.has_point != 0) & (r.result.has_point != 0))[0][40])
    bad = pr.refine(c, drop_in_sums=inlier).result
    pr.check_exact(c, r, bad)                                    # counts, scale and guards are all right ...
    d = pr.distances(c, r, bad)
    assert d["rot"] > 1e-12 or d["trans"] > 1e-12, d             # ... the pose is off by what the issue expects
    with pytest.raises(AssertionError):
        pr.check_continuous(c, r, bad, bounds)
    pr.check_all(c, r, o, bounds)                                # the oracle passes the same call


def test_standin_with_a_feature_of_the_neighbouring_slot_fails():
    c, r, o = _find("classes", "classes n=256 null_every=0")
    nb, _, _ = _find("classes", "classes n=257 null_every=0")
    cases, refs, orcs = _all("classes")
    bounds = pr.family_bounds(cases, refs, orcs)
    k = int(np.where((c.has_point != 0) & (r.result.has_point != 0))[0][100])
    wrong = dataclasses.replace(c, f=c.f.copy(), pos=c.pos.copy(), level=c.level.copy())
    wrong.f[k], wrong.pos[k], wrong.level[k] = nb.f[k], nb.pos[k], nb.level[k]
    bad = pr.refine(wrong).result
    with pytest.raises(AssertionError):
        pr.check_all(c, r, bad, bounds)


def test_standin_with_the_lower_median_fails():
    c, r, o = _find("classes", "classes n=256 null_every=0")
    assert c.n_obs % 2 == 0
    cases, refs, orcs = _all("classes")
    bounds = pr.family_bounds(cases, refs, orcs)
    bad = pr.refine(c, lower_median=True).result
    with pytest.raises(AssertionError, match="estimated_scale"):
        pr.check_exact(c, r, bad)
    for field in ("error_init", "error_final"):                  # the right result with one wrong median of squared errors
        one = dataclasses.replace(r.result, **{field: getattr(bad, field)})
        pr.check_exact(c, r, one)
        with pytest.raises(AssertionError, match=field):
            pr.check_continuous(c, r, one, bounds)
