"""What the rewritten decisions of the fused SparseImgAlign kernel's serial window rest on, checked in numpy (no GPU).

The kernel decides two things between an evaluation's barriers with one compare per lane and a scalar test of the lane
mask (android_svo_amd/csrc/svo_sia.hip, WIN_DECIDE):

  * the reference's |x| <= eps exit (nlls_solver_impl.hpp:97-98 with vk::norm_max): "the maximum of the |x_i| that are not
    NaN, starting from -1, is <= eps".  Old form: the running maximum on scalars, then one comparison.  New form: lane
    i < 6 holds |x_i|, lane 6 holds -1; a lane is bad when its value is not NaN and not <= eps; the exit is taken when no
    lane is bad.
  * "H is bit for bit the H of the previous evaluation" on the 21 lanes that hold H.  Old form: every lane forms
    `lane >= 21 || bits equal` and the wave asks whether any lane says no.  New form: every lane compares its bits, and the
    mask of the lanes that differ is cut to its low 21 bits.

Both pairs of forms are written out here as the kernel has them and compared on every special value in every position."""
import itertools

import numpy as np

TINY = np.nextafter(0.0, 1.0)                     # smallest subnormal
SPECIALS = [np.nan, np.inf, -np.inf, 0.0, -0.0, TINY, -TINY, 2.2250738585072014e-308, 1.0, -3.5, 1e-7]


def eps_exit_old(x, eps):
    """norm_max as the reference writes it (a > max on doubles: false for a NaN), then max <= eps"""
    mxn = -1.0
    for xi in x:
        a = abs(float(xi))
        if a > mxn:
            mxn = a
    return bool(mxn <= eps)


def eps_exit_new(x, eps):
    """lanes 0..5: |x_i|, lane 6: -1; bad = not NaN and not <= eps; taken when the mask of bad lanes, cut to 7 bits, is 0"""
    lane = np.arange(64)
    xi = np.where(lane < 6, np.resize(np.asarray(x, dtype=np.float64), 64), 123.0)     # (lanes >= 6 hold something else)
    w = np.where(lane < 6, np.abs(xi), -1.0)
    with np.errstate(invalid="ignore"):
        bad = ~(w <= eps) & (w == w)
    mask = sum(1 << int(i) for i in np.flatnonzero(bad))
    return (mask & 0x7F) == 0


def eps_values(x):
    finite = [abs(v) for v in x if v == v]
    mx = max(finite) if finite else 0.0
    return [0.0, -0.0, TINY, mx, np.nextafter(mx, np.inf), np.nextafter(mx, -np.inf), np.inf, -np.inf, -0.5, -1.0,
            np.nextafter(-1.0, -np.inf), np.nextafter(-1.0, 0.0), -2.0, np.nan]


def test_eps_exit_forms_agree_with_a_special_value_in_every_position():
    base = np.array([1e-3, -2e-3, 3e-4, -5e-5, 6e-5, 7e-6])
    n = 0
    for pos in range(6):
        for s in SPECIALS:
            x = base.copy()
            x[pos] = s
            for eps in eps_values(x):
                assert eps_exit_old(x, eps) == eps_exit_new(x, eps), (x.tolist(), eps)
                n += 1
    assert n == 6 * len(SPECIALS) * 14


def test_eps_exit_forms_agree_on_every_vector_of_special_values():
    vals = [np.nan, np.inf, -0.0, -1.5]          # (-inf, +0.0 and the subnormals: one position at a time, above)
    for x in itertools.product(vals, repeat=6):
        for eps in (0.0, TINY, 1.5, np.nextafter(1.5, 0.0), np.inf, -0.5, -1.0, -2.0, np.nan):
            assert eps_exit_old(x, eps) == eps_exit_new(x, eps), (x, eps)


def test_eps_exit_what_follows_for_the_odd_eps():
    x = np.array([1e-3, -2e-3, 3e-4, -5e-5, 6e-5, 7e-6])
    nan6 = np.full(6, np.nan)
    for f in (eps_exit_old, eps_exit_new):
        assert f(x, 2e-3) and not f(x, np.nextafter(2e-3, 0.0))           # |x|max exactly, and its neighbour below
        assert f(x, np.inf) and not f(x, np.nan) and not f(x, -0.5) and not f(x, 0.0)
        assert f(np.zeros(6), 0.0) and f(-np.zeros(6), 0.0) and f(np.zeros(6), -0.0)
        # the all-NaN vector leaves the maximum at -1: the exit is taken for every eps >= -1, a negative one included
        assert f(nan6, 0.0) and f(nan6, -0.5) and f(nan6, -1.0) and not f(nan6, np.nextafter(-1.0, -np.inf)) and not f(nan6, np.nan)
        assert not f(np.array([np.inf, 0, 0, 0, 0, 0]), 1e300) and f(np.array([np.inf, 0, 0, 0, 0, 0]), np.inf)
        assert f(np.array([np.nan, 1e-9, 0, 0, 0, 0]), 1e-9)               # a NaN component does not count


def h_same_old(v_bits, prev_bits):
    lane = np.arange(64)
    h_same = (lane >= 21) | (v_bits == prev_bits)
    return not bool((~h_same).any())                                       # __ballot(!h_same) == 0


def h_same_new(v_bits, prev_bits):
    differ = v_bits != prev_bits
    mask = sum(1 << int(i) for i in np.flatnonzero(differ))                # __ballot(bits differ)
    return (mask & 0x1FFFFF) == 0


def test_h_comparison_forms_agree_on_single_word_differences_and_signed_zero():
    rng = np.random.default_rng(5)
    base = rng.standard_normal(64)
    base[3] = 0.0
    base[40] = np.nan
    prev = base.view(np.uint64).copy()
    assert h_same_old(prev.copy(), prev) and h_same_new(prev.copy(), prev)
    for lane in range(64):
        for bit in (0, 31, 32, 63):                                         # low word only, high word only
            v = prev.copy()
            v[lane] ^= np.uint64(1) << np.uint64(bit)
            assert h_same_old(v, prev) == h_same_new(v, prev) == (lane >= 21), (lane, bit)
    # -0.0 against +0.0 is a difference (bits, not values), a NaN against the same NaN is none
    v = prev.copy()
    v[3] = np.array([-0.0]).view(np.uint64)[0]
    assert not h_same_old(v, prev) and not h_same_new(v, prev)
    nanv = prev.copy()
    nanv[7] = np.array([np.nan]).view(np.uint64)[0]
    assert h_same_old(nanv.copy(), nanv) and h_same_new(nanv.copy(), nanv)
    # lanes 21.. (Jres, chi2, counts) differ at every evaluation and do not count
    v = prev.copy()
    v[21:] ^= np.uint64(0xFFFF)
    assert h_same_old(v, prev) and h_same_new(v, prev)
