"""tests/klt_reference.py, the numpy definition of the bootstrap's KLT tracker, on the CPU: its pyramid and derivatives against
scipy, the level rule, the tracker against analytic ground truth, the regimes the GPU tests' inputs reach (the conditions
tests/test_gpu_klt.py rests on), and the upper median against numpy.partition."""
import functools

import numpy as np
import pytest
from scipy import ndimage

import klt_reference as K

SIZES = [(346, 260), (173, 130), (33, 31)]


@pytest.mark.parametrize("w,h", SIZES)
def test_pyr_down_against_scipy(w, h):
    img = np.random.RandomState(w).randint(0, 256, (h, w)).astype(np.uint8)
    k = np.array([1, 4, 6, 4, 1], dtype=np.int64)
    full = ndimage.correlate1d(ndimage.correlate1d(img.astype(np.int64), k, axis=0, mode="mirror"), k, axis=1, mode="mirror")
    want = ((full[::2, ::2] + 128) >> 8).astype(np.uint8)
    got = K.pyr_down(img)
    assert got.shape == ((h + 1) // 2, (w + 1) // 2) and got.dtype == np.uint8
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("w,h", SIZES)
def test_scharr_against_scipy(w, h):
    img = np.random.RandomState(h).randint(0, 256, (h, w)).astype(np.int64)
    smooth, diff = np.array([3, 10, 3], dtype=np.int64), np.array([-1, 0, 1], dtype=np.int64)
    dx = ndimage.correlate1d(ndimage.correlate1d(img, smooth, axis=0, mode="mirror"), diff, axis=1, mode="mirror")
    dy = ndimage.correlate1d(ndimage.correlate1d(img, diff, axis=0, mode="mirror"), smooth, axis=1, mode="mirror")
    gx, gy = K.scharr(img)
    np.testing.assert_array_equal(gx, dx)
    np.testing.assert_array_equal(gy, dy)
    assert np.abs(gx).max() < 2 ** 15 and np.abs(gy).max() < 2 ** 15


def test_level_rule():
    assert K.n_levels_for(640, 480) == 4          # 40 x 30 is refused
    assert K.n_levels_for(346, 260) == 4
    assert K.n_levels_for(160, 120) == 2
    # The specification's rule ("level l + 1 exists only if its width > W and its height > W", which is OpenCV's
    # `sz.width <= winSize.width || sz.height <= winSize.height` stop) gives 62 x 62 a second level of 31 x 31, since 31 > 30;
    # the "62 x 62 -> 1" of the issue's case list contradicts that rule.  The rule is what is built and asserted, and the
    # smallest single-level square next to it.
    assert K.n_levels_for(62, 62) == 2
    assert K.n_levels_for(60, 60) == 1 and K.n_levels_for(61, 60) == 1 and K.n_levels_for(31, 31) == 1
    assert K.n_levels_for(4000, 3000) == 5        # maxLevel 4 ends it
    assert [p.shape for p in K.build_pyramid(np.zeros((260, 346), np.uint8))] == [(260, 346), (130, 173), (65, 87), (33, 44)]


# ---- ground truth: a texture of 40 sinusoids sampled analytically at shifted coordinates.  Bound: 3 x what this model
# measures on these seeds (0.0104 px at 160 x 120, 0.0623 px at 346 x 260); an error above 0.25 px would
# mean the model is wrong.
GT = [(160, 120, (0.37, -0.81)), (160, 120, (3.3, 2.6)), (346, 260, (0.37, -0.81)), (346, 260, (3.3, 2.6)), (346, 260, (-7.25, 5.5))]
GT_BOUND = {(160, 120): 3 * 0.0104, (346, 260): 3 * 0.0623}


@pytest.mark.parametrize("w,h,shift", GT)
def test_ground_truth_shift(w, h, shift):
    prev, cur = K.sinusoid_texture(w, h, 3), K.sinusoid_texture(w, h, 3, shift)
    rng = np.random.RandomState(5)
    n = 60
    px = np.stack([rng.uniform(20.5, w - 21.5, n), rng.uniform(20.5, h - 21.5, n)], axis=1).astype(np.float32)
    status, out = K.track(K.build_pyramid(prev), K.build_pyramid(cur), px, px.copy())
    err = float(np.abs(out.astype(np.float64) - px - np.array(shift)).max())
    print("%d x %d shift %s: max error %.4f px" % (w, h, shift, err))
    assert status.all()
    assert err < 0.25, "the model is wrong"
    assert err <= GT_BOUND[(w, h)]


# ---- the regimes the GPU tests' inputs reach
@functools.lru_cache(maxsize=None)
def traces():
    tr = []
    for (w, h, n) in [(160, 120, 64), (346, 260, 257), (640, 480, 128)]:
        prev, cur, px = K.gpu_case(w, h, n, 11)
        t = []
        r = K.track_klt(K.build_pyramid(prev), K.build_pyramid(cur), px, px.copy(), trace=t)
        tr.append((px, r, t))
    prev, cur, px, flow = K.flow_case(160, 120, 11)
    t = []
    r = K.track_klt(K.build_pyramid(prev), K.build_pyramid(cur), px, flow, trace=t)
    tr.append((px, r, t))
    return tr


def test_every_exit_is_reached():
    counts = np.zeros(7, dtype=int)
    for _, _, t in traces():
        counts += np.bincount([e for _, _, e in t], minlength=7)
    print(dict(zip(K.EXIT_NAMES, counts)))
    assert (counts > 0).all(), dict(zip(K.EXIT_NAMES, counts))


def test_lost_at_a_coarse_level_and_found_at_level_0():
    found = 0
    for _, r, t in traces():
        lost = {k for k, level, e in t if level > 0 and e in (K.EXIT_MINEIG, K.EXIT_PREV_OOB, K.EXIT_CUR_OOB)}
        found += sum(1 for k in lost if r["status"][k])
    assert found > 0
    # the planted one: the middle of the region whose Gaussian level is exactly constant, lost to minEig at level 1
    px, r, t = traces()[1]
    k = int(np.flatnonzero((px == np.array([80.0, 80.0], dtype=np.float32)).all(axis=1))[0])
    assert (k, 1, K.EXIT_MINEIG) in t and r["status"][k] == 1


def test_integer_window_corners_give_the_corner_weights():
    assert K._weights(np.float32(0), np.float32(0)) == (16384, 0, 0, 0)
    for px, r, _ in traces()[:3]:
        # prevPt - 14.5 is an integer for x.5 coordinates: a = b = 0 at (w - 40.5, h - 30.5), a = 0 alone at (w / 2 + 0.5, 37.25)
        half = np.float32(14.5)
        frac = (px - half) - np.floor(px - half)
        assert ((frac == 0).all(axis=1) & (r["status"] == 1)).any()
        assert ((frac[:, 0] == 0) ^ (frac[:, 1] == 0)).any()


def test_flat_rectangle_features_fail_min_eig_at_level_0():
    for (w, h), (px, r, t) in zip([(160, 120), (346, 260), (640, 480)], traces()[:3]):
        k = int(np.flatnonzero((px == np.array([w // 2, h // 2], dtype=np.float32)).all(axis=1))[0])
        assert (k, 0, K.EXIT_MINEIG) in t and r["status"][k] == 0


@pytest.mark.parametrize("n", [0, 1, 2, 3, 10, 11, 64, 257])
def test_upper_median(n):
    rng = np.random.RandomState(n)
    for v in (rng.uniform(0, 5, n), np.round(rng.uniform(0, 3, n)), np.full(n, 1.25)):      # runs of equal values across the rank
        m = K.upper_median(v)
        if n == 0:
            assert np.isnan(m)
        else:
            assert m == np.partition(v, n // 2)[n // 2]
