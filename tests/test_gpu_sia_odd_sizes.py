"""SparseImgAlign (csrc/svo_sia.hip, the streaming kernels and the fused kernel) on pyramids with odd row strides, odd-aligned
row starts, level offsets that needed rounding and an odd height: 346x260, 202x134, 100x68 (seed_reference.ODD_SIZES) and
346x261.  The kernels read image rows with unaligned 8-byte loads, 7 rows per reference patch and 5 per current patch; a patch
in the last valid column reads past its row's end, in the last valid row and column one byte past its level -- into the
16-byte rounding gap, the next level, the next slot or the allocation's tail slack.  tests/sia_odd_cases.py derives those
bytes and tests/test_sia_odd_inputs_cpu.py proves on the CPU that they stay inside the allocation, that the planted features
sit at the limits and that the scenes compared by pose are well posed."""
import numpy as np
import pytest

import sia_odd_cases as so
from android_svo_amd import hip, synth
from oracle import orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(params=["fused", "fused_m32", "fused4", "stream"])
def sia_mode(request):
    """the four implementations every run()-level parity test of tests/test_gpu_parity.py is executed against (the fixture of
    that file): the fused kernel with 8 waves, with the opt-in f32 gradient moments, with 4 waves, and the streaming kernels"""
    old = dict(hip.SIA_DEFAULT_OPTIONS)
    hip.SIA_DEFAULT_OPTIONS.clear()
    if request.param == "stream":
        hip.SIA_DEFAULT_OPTIONS[hip.SIA_OPT_MODE] = hip.SIA_MODE_STREAM
    if request.param == "fused4":
        hip.SIA_DEFAULT_OPTIONS[hip.SIA_OPT_WAVES] = 4
    if request.param == "fused_m32":
        hip.SIA_DEFAULT_OPTIONS[hip.SIA_OPT_ARITH] = hip.SIA_ARITH_MOMENTS_F32
    yield request.param
    hip.SIA_DEFAULT_OPTIONS.clear()
    hip.SIA_DEFAULT_OPTIONS.update(old)


def _upload(ctx, fps, max_feat):
    cam = fps[0].cam
    ref = hip.Pyramid(ctx, cam.width, cam.height, so.N_LEVELS, len(fps))
    cur = hip.Pyramid(ctx, cam.width, cam.height, so.N_LEVELS, len(fps))
    sia = hip.SparseImgAlign(ctx, len(fps), max_feat)
    sia.set_frames(ref, cur)
    for i, fp in enumerate(fps):
        ref.upload(i, fp.ref_pyr)
        cur.upload(i, fp.cur_pyr)
        sia.upload_pair(i, fp)
    return ref, cur, sia


def _free(*objs):
    for o in objs:
        o.destroy()


def _rel(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(want).max())


def _sums(out28):
    H = np.zeros((6, 6))
    k = 0
    for i in range(6):
        for j in range(i, 6):
            H[i, j] = H[j, i] = out28[k]
            k += 1
    return H, out28[21:27], out28[27]


@pytest.mark.parametrize("size", so.SIZES, ids=so.size_id)
def test_single_evaluations_at_every_level(ctx, size):
    """One evaluation (precomputeReferencePatches + computeResiduals at T_cur == T_ref) per level that has room for a patch, on
    random-noise images with 200 random features and the planted ones of sia_odd_cases.planted -- the last accepted and the
    first rejected position at every side and corner --, in slot 0 and in the last slot of a batch of 3.  Against
    orc.sia_single_eval: visible / valid flags equal, the reference-patch cache bit-equal (streaming and fused), dx and dy of
    the fused patch dump bit-equal to the streaming caches, H, Jres and chi2 within 1e-11 relative (f64 sums in a different
    order; chi2 with the sum in the reference's order, SIA_CHI2_REFERENCE_ORDER), n_tracked equal.  The default chi2 (f32 within a
    patch, f64 over the patches) is held to the rounding bound of the two f32 sums, (n_meas + 18) * 2^-24.

    Observed on the MI355X, largest relative difference over levels, slots and sizes: H 2.8e-15 and Jres 2.6e-15 (streaming),
    H 2.8e-15 and Jres 2.4e-15 (fused), chi2 in the reference's order 0 (bit-equal everywhere), default chi2 1.5e-6."""
    w, h = size
    worst = dict(H=0.0, Jres=0.0, chi2_ref_order=0.0, chi2_default=0.0, H_fused=0.0, Jres_fused=0.0)
    for level in so.patch_levels(w, h):
        fp, n_rand, want_planted = so.noise_case(w, h, level)
        other = so.noise_case(w, h, level, seed=1)[0]
        n = len(fp.px)
        T_cfr = synth.se3_mul(fp.T_cur_w_init, synth.se3_inv(fp.T_ref_w))
        out28, nm, cache, _, ovis = orc.sia_single_eval(fp, level, T_cfr, want_caches=True)
        Ho, Jo, chi2_o = _sums(out28)
        v = ovis == 1
        assert v.sum() >= 8 and (~v).sum() >= 8
        ref, cur, sia = _upload(ctx, [fp, other, fp], n)
        slots = (0, so.BATCH - 1)
        prm = sia.params(max_level=level, min_level=level, n_iter=1, early_stop=False)
        # ---- the streaming kernels, step by step: they keep the per-pixel caches in memory
        sia.begin(so.BATCH, prm)
        sia.level_begin(level)
        sia.accumulate()
        sia.solve_update()
        sia.finish()
        stream = {}
        for s in slots:
            s_ref, s_dx, s_dy, s_vis = sia.download_caches(s, n)
            np.testing.assert_array_equal(s_vis, ovis, err_msg="level %d slot %d" % (level, s))
            np.testing.assert_array_equal(s_vis[n_rand:], want_planted)
            assert s_ref[v].tobytes() == cache[v].tobytes(), (level, s)
            r = sia.download(s)
            jres, _ = sia.download_last_step(s)
            worst["H"] = max(worst["H"], _rel(np.array(r.H).reshape(6, 6), Ho))
            worst["Jres"] = max(worst["Jres"], _rel(jres, Jo))
            assert _rel(np.array(r.H).reshape(6, 6), Ho) <= 1e-11, (level, s)
            assert _rel(jres, Jo) <= 1e-11, (level, s)
            assert r.n_tracked == nm // 16 == int(v.sum()), (level, s)
            assert r.n_precompute_patches == int(v.sum())
            d = abs(r.chi2 - chi2_o) / chi2_o
            worst["chi2_default"] = max(worst["chi2_default"], d)
            assert d <= (nm + 18) * 2.0 ** -24, (level, s, d)
            stream[s] = (s_ref, s_dx, s_dy)
        # ---- the reference patches as the fused kernel forms them
        for s in slots:
            f_ref, f_dx, f_dy, f_valid = sia.download_fused_patches(s, n, level)
            np.testing.assert_array_equal(f_valid, ovis, err_msg="level %d slot %d" % (level, s))
            assert f_ref[v].tobytes() == cache[v].tobytes(), (level, s)
            assert f_dx[v].tobytes() == stream[s][1][v].tobytes() and f_dy[v].tobytes() == stream[s][2][v].tobytes(), (level, s)
        # ---- the same evaluation through svo_hip_sia_run: the fused kernel
        sia.run(so.BATCH, prm)
        assert sia.last_run_mode() == 1
        for s in slots:
            r = sia.download(s)
            jres, _ = sia.download_last_step(s)
            worst["H_fused"] = max(worst["H_fused"], _rel(np.array(r.H).reshape(6, 6), Ho))
            worst["Jres_fused"] = max(worst["Jres_fused"], _rel(jres, Jo))
            assert _rel(np.array(r.H).reshape(6, 6), Ho) <= 1e-11, (level, s)
            assert _rel(jres, Jo) <= 1e-11, (level, s)
            assert r.n_tracked == nm // 16 and r.n_precompute_patches == int(v.sum()), (level, s)
            assert abs(r.chi2 - chi2_o) / chi2_o <= (nm + 18) * 2.0 ** -24, (level, s)
        # ---- ... and with chi2 added up in the reference's order
        sia.set_option(hip.SIA_OPT_CHI2, hip.SIA_CHI2_REFERENCE_ORDER)
        sia.run(so.BATCH, prm)
        for s in slots:
            r = sia.download(s)
            d = abs(r.chi2 - chi2_o) / chi2_o
            worst["chi2_ref_order"] = max(worst["chi2_ref_order"], d)
            assert d <= 1e-11, (level, s, r.chi2, chi2_o)
            assert _rel(np.array(r.H).reshape(6, 6), Ho) <= 1e-11 and r.n_tracked == nm // 16, (level, s)
        _free(sia, ref, cur)
    print("single evaluations %dx%d: largest relative differences %s" % (w, h, {k: "%.2e" % x for k, x in worst.items()}))


@pytest.mark.parametrize("case", so.POSE_CASES, ids=so.run_id)
def test_full_runs_pose_parity(ctx, sia_mode, case):
    """svo_hip_sia_run on rendered scenes (make_frame_pair, 200 features up to 4 px from the border) that the oracle alone solves
    well (tests/test_sia_odd_inputs_cpu.py): n_precompute_patches, n_tracked, stop and the iteration count of every level
    equal to orc.sparse_img_align, the pose within the project's tolerance, rot < 1e-4 rad and trans < 1e-3 m.

    Observed on the MI355X, largest pose difference (the reference's arithmetic: fused, fused4, stream | the opt-in f32 moments):
        346x260 L4-L0   1.6e-13 rad 3.1e-13 m | 9.2e-09 rad 1.9e-08 m
        346x260 L4-L2   1.6e-13 rad 3.1e-13 m | 4.8e-09 rad 9.6e-09 m
        346x261 L4-L0   3.3e-13 rad 6.5e-13 m | 1.7e-08 rad 3.4e-08 m
        202x134 L3-L0   4.1e-09 rad 7.9e-09 m | 2.8e-08 rad 5.6e-08 m
    with every integer equal in every mode."""
    w, h, mx, mn = case
    fp = so.scene(w, h)
    o = so.oracle_run(w, h, mx, mn)
    assert so.well_posed(o, fp, mn)
    ref, cur, sia = _upload(ctx, [fp], len(fp.px))
    sia.run(1, sia.params(max_level=mx, min_level=mn))
    r = sia.download(0)
    rot, trans = synth.pose_error(np.array(r.T_cur_w), np.array(o.T_cur_w))
    print("full run %s %s: pose difference %.3e rad %.3e m, iters %s vs %s, tracked %d vs %d" %
          (so.run_id(case), sia_mode, rot, trans, list(r.iters)[:5], list(o.iters)[:5], r.n_tracked, o.n_tracked))
    assert sia.last_run_mode() == (0 if sia_mode == "stream" else 1)
    assert r.n_precompute_patches == o.n_precompute_patches
    assert r.n_tracked == o.n_tracked
    assert r.stop == o.stop
    assert list(r.iters)[:so.N_LEVELS] == list(o.iters)[:so.N_LEVELS]
    assert rot < 1e-4 and trans < 1e-3, (rot, trans)
    _free(sia, ref, cur)


@pytest.mark.parametrize("case", so.DEGENERATE_CASES + (so.WIDE_SHORT_CASE,), ids=so.run_id)
def test_full_runs_from_a_level_too_small_to_solve(ctx, sia_mode, case):
    """100x68 and 202x134 from level 4 (6x4 and 12x8 pixels: no patch, or a handful): the solve degenerates on the oracle too, so
    the pose is not compared (as in test_random_small_configs_fuzz); both sides report the same n_precompute_patches and
    n_tracked == 0.  752x64 from level 4 (47x4) is the shape whose rejected patches load furthest past the pyramid: the
    allocation's tail slack is sized for it (svo_hip_pyramid_create; the arithmetic is in tests/sia_odd_cases.py)."""
    w, h, mx, mn = case
    fp = so.scene(w, h)
    o = so.oracle_run(w, h, mx, mn)
    ref, cur, sia = _upload(ctx, [fp], len(fp.px))
    sia.run(1, sia.params(max_level=mx, min_level=mn))
    r = sia.download(0)
    print("degenerate run %s %s: pre %d vs %d, tracked %d vs %d" % (so.run_id(case), sia_mode, r.n_precompute_patches, o.n_precompute_patches,
                                                                r.n_tracked, o.n_tracked))
    assert r.n_precompute_patches == o.n_precompute_patches
    assert r.n_tracked == o.n_tracked == 0
    _free(sia, ref, cur)


def test_ragged_batch(ctx, sia_mode):
    """three pairs of 346x260 with 200, 17 and 0 features in one launch: the 200-feature slot equals its own oracle run as in
    test_full_runs_pose_parity, the 17-feature slot reports the oracle's integer work (its pose only if the oracle run is well
    posed, which it is not), the empty slot keeps its pose.

    Observed on the MI355X: the 200-feature slot 1.6e-13 rad 3.1e-13 m from its oracle run (9.2e-09 rad 1.9e-08 m with the opt-in
    f32 moments), as when it is solved alone."""
    w, h = so.RAGGED_SIZE
    fps = [so.scene(w, h, n) for n in so.RAGGED_FEATURES]
    ref, cur, sia = _upload(ctx, fps, max(so.RAGGED_FEATURES))
    sia.run(len(fps), sia.params())
    res = sia.download_all(len(fps))
    for i, n in enumerate(so.RAGGED_FEATURES[:2]):
        o = so.oracle_run(w, h, 4, 0, n)
        assert res[i].n_precompute_patches == o.n_precompute_patches, i
        if not so.well_posed(o, fps[i], 0):
            assert i == 1
            continue
        rot, trans = synth.pose_error(np.array(res[i].T_cur_w), np.array(o.T_cur_w))
        print("ragged batch %s slot %d: pose difference %.3e rad %.3e m" % (sia_mode, i, rot, trans))
        assert res[i].n_tracked == o.n_tracked and res[i].stop == o.stop
        assert list(res[i].iters)[:so.N_LEVELS] == list(o.iters)[:so.N_LEVELS]
        assert rot < 1e-4 and trans < 1e-3, (i, rot, trans)
    assert res[2].n_tracked == 0 and res[2].n_precompute_patches == 0
    np.testing.assert_array_equal(np.array(res[2].T_cur_w), fps[2].T_cur_w_init)
    _free(sia, ref, cur)
