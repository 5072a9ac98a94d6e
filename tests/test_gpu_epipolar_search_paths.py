"""df_search_block (svo_depth_search.h) on the constructed families of tests/epipolar_families.py, through
hip.epipolar_match_batch, against the oracle's findEpipolarMatchDirect seed by seed.  Which path of the kernel each family
reaches is asserted on the CPU (tests/test_epipolar_families_cpu.py); here every family runs in several arrangements of its
seeds over the waves -- as built, reversed, interleaved with seeds of other paths, cut off inside a wave -- and a seed's
outputs must not depend on the arrangement."""
import numpy as np
import pytest

from android_svo_amd import hip

import epipolar_families as ef

pytestmark = pytest.mark.gpu

FIELDS = ("ok", "depth", "px_cur", "search_level", "epi_length", "n_zmssd", "n_align_iters")
TRUNCATIONS = (1, 3, 5, 15, 17)


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


def _assert_px_bits_equal(got, want):
    """bitwise equality of two float64 arrays (NaN payloads included)"""
    np.testing.assert_array_equal(np.ascontiguousarray(got, dtype=np.float64).view(np.uint64),
                                  np.ascontiguousarray(want, dtype=np.float64).view(np.uint64))


def _upload(ctx, case):
    kf = hip.Pyramid(ctx, ef.W, ef.H, ef.N_LEVELS, case.n_ref_slots)
    cf = hip.Pyramid(ctx, ef.W, ef.H, ef.N_LEVELS, 1)
    for slot in range(case.n_ref_slots):        # the slots that are not the case's hold the inverted image
        kf.upload(slot, case.ref_pyr if slot == case.ref_slot else [255 - im for im in case.ref_pyr])
    cf.upload(0, case.cur_pyr)
    return kf, cf


def _run(ctx, kf, cf, case):
    prm = hip.depth_filter_params(n_pyr_levels=ef.N_LEVELS, max_epi_search_steps=case.max_steps)
    return hip.epipolar_match_batch(ctx, kf, case.ref_slot, cf, 0, case.cam, case.T_ref_w, case.T_cur_w, case.px, case.f, case.level,
                                    case.d_est, case.d_min, case.d_max, prm)


def _assert_equals_oracle(out, case, what):
    want = ef.oracle_results(case)
    assert len(want) <= 200
    ok = np.array([r.ok for r, _ in want], dtype=bool)
    label = "%s (%s)" % (case.name, what)
    np.testing.assert_array_equal(out["ok"], ok, err_msg=label)
    for key, field in (("search_level", "search_level"), ("n_zmssd", "n_zmssd"), ("n_align_iters", "n_align_iters")):
        np.testing.assert_array_equal(out[key], np.array([getattr(r, field) for r, _ in want]), err_msg="%s: %s %s" % (label, key, case.tags))
    _assert_px_bits_equal(out["px_cur"][ok], np.array([list(r.px_cur) for r, _ in want]).reshape(-1, 2)[ok])
    np.testing.assert_allclose(out["epi_length"], np.array([r.epi_length for r, _ in want]), rtol=1e-12, err_msg=label)
    np.testing.assert_allclose(out["depth"][ok], np.array([r.depth for r, _ in want])[ok], rtol=1e-12, err_msg=label)
    assert (out["depth"][~ok] == 0).all(), label


def _assert_same_bits(out, rows, base, base_rows, what):
    """rows `rows` of one run against rows `base_rows` of another: every output array bit for bit"""
    for k in FIELDS:
        a, b = out[k][rows], base[k][base_rows]
        if a.dtype == np.float64:
            _assert_px_bits_equal(a, b)
        else:
            np.testing.assert_array_equal(a, b, err_msg="%s: %s" % (what, k))


@pytest.mark.parametrize("name", list(ef.FAMILIES))
def test_search_paths_against_the_oracle(ctx, name):
    n_seeds = 0
    for case in ef.family(name):
        kf, cf = _upload(ctx, case)
        n = case.n
        n_seeds += n
        base = _run(ctx, kf, cf, case)
        _assert_equals_oracle(base, case, "as built")
        # reversed
        rev = np.arange(n)[::-1]
        out = _run(ctx, kf, cf, case.subset(rev))
        _assert_same_bits(out, np.arange(n), base, rev, case.name + " reversed")
        # every second seed a filler of another path: the four seeds of every wave differ
        mixed = ef.with_fillers(case)
        out = _run(ctx, kf, cf, mixed)
        _assert_equals_oracle(out, mixed, "with fillers")
        _assert_same_bits(out, np.arange(0, 2 * n, 2), base, np.arange(n), case.name + " with fillers")
        # cut off inside a wave (the case's seeds repeated where it has fewer)
        for k in TRUNCATIONS:
            idx = np.arange(k) % n
            out = _run(ctx, kf, cf, case.subset(idx))
            _assert_same_bits(out, np.arange(k), base, idx, "%s truncated to %d" % (case.name, k))
        kf.destroy(); cf.destroy()
    assert 16 <= n_seeds <= 64
