"""SVO_HIP_SIA_REDUCTION_TILE_ORDER: every result of a frame pair is a function of that frame pair alone.

In the fused SparseImgAlign kernel's default mode the 29 sums of an evaluation are grouped by the wave that owns a frame's
tiles, and the tile-to-wave map is the kernel shape of the launch -- chosen from the launch's largest frame and its size.  In
the opt-in mode they are grouped by tile and added in tile order.  Checked here, always as EQUAL BYTES in every field of
svo_hip_sia_result (pose, n_tracked, H, chi2, stop, iters and the two patch counters; a NaN pose of a 5- or 12-patch frame
equals itself): the same pair alone, in company, in another slot and under every kernel shape the diagnostic options can
force; that the default mode does differ on these inputs (otherwise they would exercise one grouping only); what the mode
refuses; that it still gives the reference's answer; that the default is untouched by the option's existence."""
import itertools

import numpy as np
import pytest

from android_svo_amd import hip, synth

pytestmark = pytest.mark.gpu

# (features, seed, null_point_every)
SIZES = [(5, 31, 0), (12, 32, 5), (100, 33, 0), (420, 34, 7), (600, 35, 0), (1200, 36, 11), (2000, 37, 0), (2816, 38, 13)]
NS = [s[0] for s in SIZES]
STOPS = [(True, 30), (False, 6)]        # (early_stop, n_iter): the reference's exits / a fixed evaluation count
TORD = {hip.SIA_OPT_REDUCTION: hip.SIA_REDUCTION_TILE_ORDER}


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pairs():
    return {n: synth.make_frame_pair(seed=seed, n_features=n, null_point_every=npe) for n, seed, npe in SIZES}


def _bytes(r):
    """every field of svo_hip_sia_result, as bytes (no padding: a NaN compares equal to itself)"""
    return b"".join(np.ascontiguousarray(a).tobytes() for a in (
        np.array(r.T_cur_w, dtype=np.float64).view(np.uint64), np.array([r.n_tracked], dtype=np.uint64),
        np.array(r.H, dtype=np.float64).view(np.uint64), np.array([r.chi2], dtype=np.float64).view(np.uint64),
        np.array([r.stop], dtype=np.int32), np.array(r.iters, dtype=np.int32),
        np.array([r.n_precompute_patches, r.n_residual_patches], dtype=np.uint64)))


class _Batch:
    """a batch of frame pairs on the device, solved as often as wanted under changing options"""

    def __init__(self, ctx, fps, options):
        cam = fps[0].cam
        self.n = len(fps)
        self.ref = hip.Pyramid(ctx, cam.width, cam.height, 5, self.n)
        self.cur = hip.Pyramid(ctx, cam.width, cam.height, 5, self.n)
        self.sia = hip.SparseImgAlign(ctx, self.n, max(max(len(fp.px) for fp in fps), 1))
        for o, v in options.items():
            self.sia.set_option(o, v)
        self.sia.set_frames(self.ref, self.cur)
        for i, fp in enumerate(fps):
            self.ref.upload(i, fp.ref_pyr)
            self.cur.upload(i, fp.cur_pyr)
            self.sia.upload_pair(i, fp)

    def solve(self, stop):
        early, n_iter = stop
        self.sia.run(self.n, self.sia.params(max_level=4, min_level=0, n_iter=n_iter, eps=1e-6, early_stop=early))
        out = [_bytes(r) for r in self.sia.download_all(self.n)]
        assert self.sia.last_run_mode() == 1             # every accepted run of the mode is a run of the fused kernel
        return out

    def free(self):
        for o in (self.sia, self.ref, self.cur):
            o.destroy()


def _solve(ctx, fps, options, stop):
    b = _Batch(ctx, fps, options)
    try:
        return b.solve(stop)
    finally:
        b.free()


@pytest.fixture(scope="module")
def lone(ctx, pairs):
    """every pair solved alone in the mode: {(n, stop): bytes}"""
    out = {}
    for n in NS:
        b = _Batch(ctx, [pairs[n]], TORD)
        for stop in STOPS:
            out[(n, stop)] = b.solve(stop)[0]
        b.free()
    return out


# the companies of test 1: all eight, and batches whose largest frame has 420, 1200 and 2816 patches
COMPANIES = [NS, [420, 5, 12, 100], [1200, 600, 5, 420, 100, 12], [2816, 2000, 5, 100, 600, 12]]


def test_a_pair_alone_equals_the_pair_in_company(ctx, pairs, lone):
    for members in COMPANIES:
        for stop in STOPS:
            got = _solve(ctx, [pairs[n] for n in members], TORD, stop)
            for slot, n in enumerate(members):
                assert got[slot] == lone[(n, stop)], (members, stop, n)


def test_a_pair_in_the_first_and_in_the_last_slot(ctx, pairs, lone):
    for members in (NS + NS[::-1], [2000] + NS[:6] + [2000], [420, 2816, 100, 420]):
        for stop in STOPS:
            got = _solve(ctx, [pairs[n] for n in members], TORD, stop)
            assert got[0] == got[-1], (members, stop)
            for slot, n in enumerate(members):
                assert got[slot] == lone[(n, stop)], (members, stop, slot)


def _shape_options(n):
    """every combination of SVO_HIP_SIA_OPT_WAVES / _OLD_TILES / _EXTRA_LDS that svo_hip_sia_set_option accepts and the shape
    choice honours for a launch whose largest frame has n patches (an override outside these ranges is ignored by it)"""
    per_simd = (max((n + 63) // 64, 1) + 3) // 4
    waves = [0, 8] + ([4] if per_simd <= 4 else [])
    old = [0] + [t for t in range(1, 7) if (per_simd + 1) // 2 <= t <= per_simd]
    out = []
    for w, t in itertools.product(waves, old):
        tpw = t or max((per_simd + 1) // 2, 1)
        extra = [-1, 0, 1, 2, 3] if (w != 4 and tpw in (3, 4)) else [-1]
        out += [(w, t, e) for e in extra]
    return out


def test_a_pair_under_every_kernel_shape(ctx, pairs, lone):
    n_shapes = 0
    for n in NS:
        b = _Batch(ctx, [pairs[n]], TORD)
        for w, t, e in _shape_options(n):
            b.sia.set_option(hip.SIA_OPT_WAVES, w)
            b.sia.set_option(hip.SIA_OPT_OLD_TILES, t)
            b.sia.set_option(hip.SIA_OPT_EXTRA_LDS, e)
            for stop in STOPS:
                assert b.solve(stop)[0] == lone[(n, stop)], (n, w, t, e, stop)
            n_shapes += 1
        b.free()
    assert n_shapes > 40
    # a small pair beside a large one under the large one's forced shapes: the small pair's tiles land on other waves
    b = _Batch(ctx, [pairs[420], pairs[1200]], TORD)
    for w, t, e in _shape_options(1200):
        b.sia.set_option(hip.SIA_OPT_WAVES, w)
        b.sia.set_option(hip.SIA_OPT_OLD_TILES, t)
        b.sia.set_option(hip.SIA_OPT_EXTRA_LDS, e)
        got = b.solve(STOPS[0])
        assert got[0] == lone[(420, STOPS[0])] and got[1] == lone[(1200, STOPS[0])], (w, t, e)
    b.free()


@pytest.mark.parametrize("arith", [hip.SIA_ARITH_FAST, hip.SIA_ARITH_MOMENTS_F32])
def test_other_arithmetic_levels_are_refused_not_ignored(ctx, pairs, arith):
    """the mode's kernels exist for SVO_HIP_SIA_ARITH_EXACT; another level with the mode set is a state error"""
    for members in ([600], [12, 600]):               # (a batch with a tiny frame takes the instance that reads the level at run time)
        b = _Batch(ctx, [pairs[n] for n in members], {**TORD, hip.SIA_OPT_ARITH: arith})
        with pytest.raises(hip.SvoHipError, match=r"\(-4\)"):
            b.solve(STOPS[0])
        b.sia.set_option(hip.SIA_OPT_ARITH, hip.SIA_ARITH_EXACT)
        b.solve(STOPS[0])
        b.free()


def test_the_default_mode_does_depend_on_the_company(ctx, pairs):
    """The guard of the tests above: in the default mode at least one of these pairs gets other bits in company than alone.
    If none did, the inputs would exercise one grouping only and the equalities above would show nothing."""
    per_wave = {hip.SIA_OPT_REDUCTION: hip.SIA_REDUCTION_PER_WAVE}
    alone = {(n, stop): _solve(ctx, [pairs[n]], per_wave, stop)[0] for n in NS for stop in STOPS}
    differing = []
    for members in COMPANIES:
        for stop in STOPS:
            got = _solve(ctx, [pairs[n] for n in members], per_wave, stop)
            differing += [(tuple(members), stop, n) for slot, n in enumerate(members) if got[slot] != alone[(n, stop)]]
    print("default mode, pairs whose bits depend on their company:", len(differing), differing[:6])
    assert differing


def test_what_the_mode_refuses(ctx, pairs):
    fp = pairs[600]
    b = _Batch(ctx, [fp], TORD)
    for bad in (2, -1):
        with pytest.raises(hip.SvoHipError, match=r"\(-1\)"):
            b.sia.set_option(hip.SIA_OPT_REDUCTION, bad)
    want = b.solve(STOPS[0])[0]                       # (the refused values left the mode set)
    refusals = [(hip.SIA_OPT_MODE, hip.SIA_MODE_STREAM, hip.SIA_MODE_AUTO),
                (hip.SIA_OPT_METHOD, hip.SIA_METHOD_LEVENBERG_MARQUARDT, hip.SIA_METHOD_GAUSS_NEWTON),
                (hip.SIA_OPT_SCALE_ESTIMATOR, hip.SIA_SCALE_TDIST, hip.SIA_SCALE_UNIT),
                (hip.SIA_OPT_CHI2, hip.SIA_CHI2_REFERENCE_ORDER, hip.SIA_CHI2_PER_PATCH)]
    for opt, val, back in refusals:
        b.sia.set_option(opt, val)
        with pytest.raises(hip.SvoHipError, match=r"\(-4\)"):
            b.solve(STOPS[0])
        b.sia.set_option(opt, back)
        assert b.solve(STOPS[0])[0] == want
    # a robust cost set the reference's way (scale estimator + weight function)
    b.sia.set_robust_cost_function(hip.SIA_SCALE_MAD, hip.SIA_WEIGHT_TUKEY)
    with pytest.raises(hip.SvoHipError, match=r"\(-4\)"):
        b.solve(STOPS[0])
    b.free()
    # a frame above 2816 patches would take the streaming kernels
    big = synth.make_frame_pair(seed=39, n_features=3000)
    b = _Batch(ctx, [big], TORD)
    with pytest.raises(hip.SvoHipError, match=r"\(-4\)"):
        b.solve(STOPS[0])
    b.sia.set_option(hip.SIA_OPT_REDUCTION, hip.SIA_REDUCTION_PER_WAVE)
    b.sia.run(1, b.sia.params())
    assert b.sia.last_run_mode() == 0
    b.free()


def _ref_cases():
    from oracle import gen_golden
    return gen_golden.SIA_REF_CASES


@pytest.mark.parametrize("case", _ref_cases(), ids=[c[0] for c in _ref_cases()])
def test_the_mode_against_the_reference_run(ctx, golden, case):
    """the assertions of tests/test_gpu_parity.py::test_sparse_img_align_against_reference_run and
    ::test_fixed_work_mode_against_the_reference_members for the fused mode, with the same tolerances, in the mode: it
    regroups f64 additions and nothing else.  (The case above 2816 patches is one the fused kernel does not take -- those two
    tests run it through the streaming kernels -- so in the mode it has to be refused, and that is what is asserted for it.)"""
    from oracle import gen_golden
    name, kw, max_level, min_level, n_iter = case
    g = golden("sia_ref.npz")
    fp = gen_golden.make_sia_case(kw)
    b = _Batch(ctx, [fp], TORD)
    sia = b.sia
    if len(fp.px) > 2816:
        with pytest.raises(hip.SvoHipError, match=r"\(-4\)"):
            sia.run(1, sia.params(max_level=max_level, min_level=min_level, n_iter=n_iter, eps=1e-6, early_stop=True))
        b.free()
        return
    sia.run(1, sia.params(max_level=max_level, min_level=min_level, n_iter=n_iter, eps=1e-6, early_stop=True))
    assert sia.last_run_mode() == 1
    r = sia.download(0)
    rot, trans = synth.pose_error(np.array(r.T_cur_w), g[name + "_T"])
    assert rot < 1e-4 and trans < 1e-3, (rot, trans)            # north_star tolerance
    assert rot < 2e-5 and trans < 5e-5, (rot, trans)            # what chi2-order exit flips can cost at most here
    assert r.n_tracked == int(g[name + "_n_tracked"])
    assert int(r.stop) == int(g[name + "_stop"])
    if len(fp.px):
        same_iters = all(r.iters[l] == int(g[name + "_iter"][l]) + 1 for l in range(min_level, max_level + 1))
        if same_iters:                                          # same evaluation sequence: everything agrees closely
            assert rot < 1e-7 and trans < 1e-7, (rot, trans)
            H = np.array(r.H)
            assert np.abs(H - g[name + "_H"]).max() <= 1e-6 * np.abs(g[name + "_H"]).max()
        # the fixed-work form
        sia.run(1, sia.params(max_level=max_level, min_level=min_level, n_iter=n_iter, eps=1e-6, early_stop=False))
        assert sia.last_run_mode() == 1
        r = sia.download(0)
        assert all(r.iters[level] == n_iter for level in range(min_level, max_level + 1))
        assert r.n_tracked == int(g[name + "_fw_n_tracked"])
        rot, trans = synth.pose_error(np.array(r.T_cur_w), g[name + "_fw_T"])
        assert rot < 1e-7 and trans < 1e-7, (rot, trans)
        H = np.array(r.H)
        assert np.abs(H - g[name + "_fw_H"]).max() <= 1e-6 * np.abs(g[name + "_fw_H"]).max()
        assert abs(r.chi2 - float(g[name + "_fw_chi2"])) <= 1e-4 * float(g[name + "_fw_chi2"])
    b.free()


def test_the_default_is_untouched_by_setting_it(ctx, pairs):
    members = [1200, 600, 5, 420]
    fps = [pairs[n] for n in members]
    for stop in STOPS:
        never = _solve(ctx, fps, {}, stop)
        assert _solve(ctx, fps, {hip.SIA_OPT_REDUCTION: hip.SIA_REDUCTION_PER_WAVE}, stop) == never
        b = _Batch(ctx, fps, TORD)                        # ... and by having been in the mode before
        b.solve(stop)
        b.sia.set_option(hip.SIA_OPT_REDUCTION, hip.SIA_REDUCTION_PER_WAVE)
        assert b.solve(stop) == never
        b.free()
