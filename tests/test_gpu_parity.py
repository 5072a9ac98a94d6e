"""GPU parity tests (run with -m gpu on the MI355X box): the HIP path, called through the
C-ABI, against the CPU oracle on the same seeded inputs and against the golden fixtures.

Bars: bit-exact for bytes / integers / indices; floating point within the tolerance written
at each assert (north_star: pose error < 1e-4 rad and < 1e-3 m vs the reference path).
"""
import ctypes as C
import os

import numpy as np
import pytest

from android_svo_amd import hip, seedsynth, synth
from oracle import orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(params=["fused", "fused_m32", "fused4", "stream"])
def sia_mode(request):
    """svo_hip_sia_run has two implementations (one fused launch per run / one launch per Gauss-Newton
    evaluation), the fused kernel two shapes (8 waves per frame pair; 4 waves, two pairs per CU, which large
    launches of small frames get -- forced here) and an OPT-IN arithmetic level that sums a patch's two gradient
    moments in f32 (SVO_HIP_SIA_ARITH_MOMENTS_F32; the library default is the reference's own arithmetic, EXACT, again since
    round 5): every run()-level parity test is executed against all four.  `_tight()` tells a test whether the run
    reproduces the CPU path to rounding level (everything but the opt-in level)."""
    old = dict(hip.SIA_DEFAULT_OPTIONS)
    hip.SIA_DEFAULT_OPTIONS.clear()
    if request.param == "stream":
        hip.SIA_DEFAULT_OPTIONS[hip.SIA_OPT_MODE] = hip.SIA_MODE_STREAM
    if request.param == "fused4":
        hip.SIA_DEFAULT_OPTIONS[hip.SIA_OPT_WAVES] = 4
    if request.param == "fused_m32":
        hip.SIA_DEFAULT_OPTIONS[hip.SIA_OPT_ARITH] = hip.SIA_ARITH_MOMENTS_F32
    yield "fused" if request.param.startswith("fused") else request.param
    hip.SIA_DEFAULT_OPTIONS.clear()
    hip.SIA_DEFAULT_OPTIONS.update(old)


def _tight():
    """the solver objects created now use the reference's arithmetic to the last operation (the library default)"""
    return hip.SIA_DEFAULT_OPTIONS.get(hip.SIA_OPT_ARITH, hip.SIA_ARITH_EXACT) == hip.SIA_ARITH_EXACT


def _upload_pair(ctx, fps, max_feat=None):
    cam = fps[0].cam
    B = len(fps)
    ref = hip.Pyramid(ctx, cam.width, cam.height, 5, B)
    cur = hip.Pyramid(ctx, cam.width, cam.height, 5, B)
    sia = hip.SparseImgAlign(ctx, B, max_feat or max(len(fp.px) for fp in fps))
    sia.set_frames(ref, cur)
    for i, fp in enumerate(fps):
        ref.upload(i, fp.ref_pyr)
        cur.upload(i, fp.cur_pyr)
        sia.upload_pair(i, fp)
    return ref, cur, sia


def _free(*objs):
    for o in objs:
        (o.destroy if hasattr(o, "destroy") else o.free)()


def test_precompute_caches_bit_exact(ctx):
    """Reference patch cache and gradients are per-pixel f32 with no reduction: bit-exact."""
    fp = synth.make_frame_pair(seed=21, n_features=300, null_point_every=11)
    ref, cur, sia = _upload_pair(ctx, [fp])
    prm = sia.params(max_level=2, min_level=2, n_iter=1)
    sia.begin(1, prm)            # step-wise entry points: always the streaming kernels, which keep the caches in HBM
    sia.level_begin(2)
    sia.accumulate()
    sia.solve_update()
    sia.finish()
    rc, dx, dy, vis = sia.download_caches(0, len(fp.px))
    T_cfr = synth.se3_mul(fp.T_cur_w_init, synth.se3_inv(fp.T_ref_w))
    out28, nm, cache, jac, ovis = orc.sia_single_eval(fp, 2, T_cfr, want_caches=True)
    np.testing.assert_array_equal(vis, ovis)
    np.testing.assert_array_equal(rc[ovis == 1], cache[ovis == 1])
    assert (ovis == 0).sum() == (fp.has_point == 0).sum()
    r = sia.download(0)
    # H of that single evaluation: fp64 sums in a different order -> 1e-11 relative
    Ho = np.zeros((6, 6))
    k = 0
    for i in range(6):
        for j in range(i, 6):
            Ho[i, j] = Ho[j, i] = out28[k]; k += 1
    H = np.array(r.H).reshape(6, 6)
    assert np.abs(H - Ho).max() <= 1e-11 * np.abs(Ho).max()
    assert r.n_tracked == nm // 16
    _free(sia, ref, cur)


@pytest.mark.parametrize("level", [0, 2, 4])
def test_fused_kernel_reference_patches_bit_exact(ctx, level):
    """The FUSED kernel never writes per-pixel caches: it keeps 32 interpolated values per patch (halved weights) in LDS /
    L2-resident memory and takes reference value, dx and dy as differences of them.  svo_hip_sia_download_fused_patches
    recomputes them with the fused kernel's own device functions (f32 feature position, halved weights, interpolation):
    the reference values must equal the reference's ref_patch_cache_ (oracle, pinned by sia_ref.npz) bit for bit, and dx /
    dy the streaming kernels' arrays (whose Jacobian cache is pinned bit-exact), at the finest, a middle and the
    coarsest level, border patches and point-less features included."""
    fp = synth.make_frame_pair(seed=23, n_features=400, null_point_every=9, border=6)
    ref, cur, sia = _upload_pair(ctx, [fp])
    n = len(fp.px)
    prm = sia.params(max_level=level, min_level=level, n_iter=1)
    sia.begin(1, prm)
    sia.level_begin(level)
    sia.accumulate()
    sia.solve_update()
    sia.finish()
    s_ref, s_dx, s_dy, s_vis = sia.download_caches(0, n)
    f_ref, f_dx, f_dy, f_valid = sia.download_fused_patches(0, n, level)
    T_cfr = synth.se3_mul(fp.T_cur_w_init, synth.se3_inv(fp.T_ref_w))
    _, _, cache, _, ovis = orc.sia_single_eval(fp, level, T_cfr, want_caches=True)
    np.testing.assert_array_equal(f_valid, ovis)                  # valid at this level == visible_fts_ after this level alone
    v = f_valid == 1
    assert 10 < v.sum() and (~v).sum() >= (fp.has_point == 0).sum()
    assert f_ref[v].tobytes() == cache[v].astype(np.float32).tobytes()
    assert f_dx[v].tobytes() == s_dx[v].tobytes() and f_dy[v].tobytes() == s_dy[v].tobytes()
    assert f_ref[v].tobytes() == s_ref[v].tobytes()
    _free(sia, ref, cur)


@pytest.mark.parametrize("n,seed", [(200, 12345), (2000, 12346), (1200, 12347)])
def test_sparse_img_align_pose_parity(ctx, sia_mode, n, seed):
    """Configs C0 / C1-shape, reference semantics (early stop), L4-L0 and the shipping L4-L2."""
    fp = synth.make_frame_pair(seed=seed, n_features=n)
    ref, cur, sia = _upload_pair(ctx, [fp])
    for min_level in (0, 2):
        sia.run(1, sia.params(max_level=4, min_level=min_level))
        r = sia.download(0)
        o = orc.sparse_img_align(fp, max_level=4, min_level=min_level)
        rot, trans = synth.pose_error(np.array(r.T_cur_w), np.array(o.T_cur_w))
        assert rot < 1e-4 and trans < 1e-3, (rot, trans)          # north_star tolerance
        assert rot < 2e-5 and trans < 5e-5, (rot, trans)          # what we actually hold
        assert r.n_tracked == o.n_tracked
        assert r.stop == o.stop == 0
        assert sia.last_run_mode() == (1 if sia_mode == "fused" else 0)
    _free(sia, ref, cur)


def test_sparse_img_align_golden_full(ctx, sia_mode, golden):
    """Against poses produced by the reference's own NLLSSolver/Eigen/SE3 (tests/golden/gn_full.npz)."""
    g = golden("gn_full.npz")
    for i in range(len(g["seed"])):
        fp = synth.make_frame_pair(seed=int(g["seed"][i]), n_features=int(g["n"][i]))
        ref, cur, sia = _upload_pair(ctx, [fp])
        sia.run(1, sia.params())
        r = sia.download(0)
        rot, trans = synth.pose_error(np.array(r.T_cur_w), g["T_out"][i])
        assert rot < 1e-4 and trans < 1e-3, (i, rot, trans)
        _free(sia, ref, cur)


def test_fixed_work_mode_matches_oracle_closely(ctx, sia_mode):
    """With early stop off both sides run exactly 30 iterations per level: no data-dependent
    control flow, so poses agree to fp64 summation-order noise."""
    fp = synth.make_frame_pair(seed=31, n_features=500)
    ref, cur, sia = _upload_pair(ctx, [fp])
    sia.run(1, sia.params(early_stop=False))
    r = sia.download(0)
    o = orc.sparse_img_align(fp, early_stop=False)
    assert list(r.iters)[:5] == [30] * 5 == list(o.iters)[:5]
    rot, trans = synth.pose_error(np.array(r.T_cur_w), np.array(o.T_cur_w))
    assert rot < 1e-7 and trans < 1e-7, (rot, trans)
    assert r.n_residual_patches == o.n_residual_patches
    assert r.n_precompute_patches == o.n_precompute_patches
    _free(sia, ref, cur)


def test_patches_leaving_the_image(ctx, sia_mode):
    """Features close to the border: some patches are invisible at coarse levels (reference image
    test), some leave the current image during the iterations.  Exercises the sticky visibility
    flags and the per-evaluation rebuild of H from the patches visible now."""
    fp = synth.make_frame_pair(seed=61, n_features=900, border=5, t_mag=0.05, r_mag=0.02)
    ref, cur, sia = _upload_pair(ctx, [fp])
    for early in (True, False):
        sia.run(1, sia.params(early_stop=early, n_iter=30 if early else 6))
        r = sia.download(0)
        o = orc.sparse_img_align(fp, early_stop=early, n_iter=30 if early else 6)
        assert o.n_tracked < 900                      # the case really loses patches
        assert r.n_tracked == o.n_tracked
        assert r.n_precompute_patches == o.n_precompute_patches
        rot, trans = synth.pose_error(np.array(r.T_cur_w), np.array(o.T_cur_w))
        assert rot < 1e-4 and trans < 1e-3, (rot, trans)
        if not early:
            assert r.n_residual_patches == o.n_residual_patches
            H, Ho = np.array(r.H), np.array(o.H)
            assert np.abs(H - Ho).max() <= 1e-9 * np.abs(Ho).max()
    _free(sia, ref, cur)


def test_points_in_the_camera_plane(ctx, sia_mode):
    """Patches whose point lies (almost) in the plane of the current camera: z_cur of 1e-15 ... 1e-8 m, so the
    projection is 1e7 ... 1e17 px or infinite.  The float -> int conversion of such a coordinate SATURATES on the
    device (INT_MAX) where the host's cvttss2si returns INT_MIN; `u + border < cols` then wrapped around and the
    patch was read thousands of rows outside the image.  Both sides must drop these patches and agree on the rest."""
    fp = synth.make_frame_pair(seed=83, n_features=700)
    tz = 0.01
    fp.T_cur_w_init = synth.se3_mul(np.array([0, 0, -tz, 0, 0, 0, 1.0]), fp.T_ref_w)
    T_w_ref = synth.se3_inv(fp.T_ref_w)
    idx = [5, 64, 65, 200, 333, 699]
    for i, eps in zip(idx, [1e-13, -1e-13, 0.0, 1e-9, 1e-6, 3e-16]):
        d = tz / fp.f[i, 2] * (1.0 + eps)
        fp.pos[i] = synth.se3_act(T_w_ref, fp.f[i] * d)
        z_cur = fp.f[i, 2] * np.linalg.norm(fp.pos[i] - T_w_ref[:3]) - tz
        assert abs(z_cur) < 2e-8
    ref, cur, sia = _upload_pair(ctx, [fp])
    sia.run(1, sia.params(early_stop=False, n_iter=3))
    r = sia.download(0)
    o = orc.sparse_img_align(fp, early_stop=False, n_iter=3)
    assert r.n_precompute_patches == o.n_precompute_patches
    assert r.n_residual_patches == o.n_residual_patches
    assert r.n_tracked == o.n_tracked
    rot, trans = synth.pose_error(np.array(r.T_cur_w), np.array(o.T_cur_w))
    tol = 1e-9 if _tight() else 2e-7            # the opt-in MOMENTS_F32 level sums a patch's gradient moments in f32
    assert rot < tol and trans < tol, (rot, trans)
    H, Ho = np.array(r.H), np.array(o.H)
    assert np.abs(H - Ho).max() <= 1e-9 * np.abs(Ho).max()
    _free(sia, ref, cur)


def test_small_frames_take_the_factored_hessian_rows(ctx, sia_mode):
    """Frames with 16 ... 64 patches and none smaller: the fused kernel runs its factored per-tile Hessian rows (a batch
    that holds a frame below 16 patches would select the entry-by-entry instance, test_batch_ragged_and_empty).  Few
    patches make H poorly conditioned at the coarse levels; every slot must still equal its own oracle run."""
    fps = [synth.make_frame_pair(seed=140 + i, n_features=n) for i, n in enumerate([16, 17, 20, 33, 48, 64])]
    ref, cur, sia = _upload_pair(ctx, fps, max_feat=64)
    sia.run(len(fps), sia.params())
    res = sia.download_all(len(fps))
    for i, fp in enumerate(fps):
        o = orc.sparse_img_align(fp)
        got, want = np.array(res[i].T_cur_w), np.array(o.T_cur_w)
        assert not np.isnan(want).any(), i
        rot, trans = synth.pose_error(got, want)
        assert rot < 1e-4 and trans < 1e-3, (i, rot, trans)
        assert res[i].n_tracked == o.n_tracked, i
    _free(sia, ref, cur)


def test_radtan_camera_forward_model(ctx, sia_mode):
    """world2cam with the 5-coefficient radtan model (pinhole_camera.cpp:88-104) inside the residual
    evaluation; fixed work so both sides execute the same evaluations."""
    fp = synth.make_frame_pair(seed=77, n_features=600)
    fp.dist = [-0.05, 0.01, 1e-3, -5e-4, 2e-3]
    ref, cur, sia = _upload_pair(ctx, [fp])
    sia.run(1, sia.params(early_stop=False, n_iter=5))
    r = sia.download(0)
    o = orc.sparse_img_align(fp, early_stop=False, n_iter=5)
    fp.dist = None
    o_plain = orc.sparse_img_align(fp, early_stop=False, n_iter=5)
    rot, trans = synth.pose_error(np.array(r.T_cur_w), np.array(o.T_cur_w))
    assert rot < 1e-7 and trans < 1e-7, (rot, trans)
    rot2, trans2 = synth.pose_error(np.array(o_plain.T_cur_w), np.array(o.T_cur_w))
    assert rot2 > 1e-5 or trans2 > 1e-5          # the distortion really changes the answer
    assert r.n_residual_patches == o.n_residual_patches
    _free(sia, ref, cur)


def test_batch_ragged_and_empty(ctx, sia_mode):
    """A batch with different feature counts, an empty frame and point-less features: every
    slot must equal its own single-frame oracle run; an empty slot keeps its pose (run() -> 0)."""
    fps = [synth.make_frame_pair(seed=40 + i, n_features=n, null_point_every=k)
           for i, (n, k) in enumerate([(64, 0), (333, 5), (1, 0), (1000, 0), (17, 2)])]
    ref, cur, sia = _upload_pair(ctx, fps + [fps[0]], max_feat=1000)
    # slot 5: no features at all
    empty = synth.FramePair(fps[0].cam, fps[0].ref_pyr, fps[0].cur_pyr, np.zeros((0, 2)), np.zeros((0, 3)),
                            np.zeros((0, 3)), np.zeros(0, dtype=np.uint8), fps[0].T_ref_w, fps[0].T_cur_w_true,
                            fps[0].T_cur_w_init)
    sia.upload_pair(5, empty)
    sia.run(6, sia.params())
    res = sia.download_all(6)
    for i, fp in enumerate(fps):
        o = orc.sparse_img_align(fp)
        got, want = np.array(res[i].T_cur_w), np.array(o.T_cur_w)
        if np.isnan(want).any():
            assert np.isnan(got).any()
            continue
        rot, trans = synth.pose_error(got, want)
        assert rot < 1e-4 and trans < 1e-3, (i, rot, trans)
        assert res[i].n_tracked == o.n_tracked, i
    assert res[5].n_tracked == 0
    np.testing.assert_array_equal(np.array(res[5].T_cur_w), fps[0].T_cur_w_init)
    _free(sia, ref, cur)


def test_tiny_frame_in_a_batch_does_not_change_the_other_frames(ctx):
    """A frame with fewer than 16 patches needs the entry-by-entry Hessian rows (a rank-deficient system); svo_hip_sia_run
    launches that kernel instance for those slots only.  The largest frame of the batch must come out bit for bit as when
    it is solved alone (same kernel shape either way), the other frames within the tolerance of their oracle runs, and
    the tiny frame must still follow its own oracle run."""
    specs = [(1200, 0), (5, 0), (700, 3), (0, 0), (12, 0)]
    fps = [synth.make_frame_pair(seed=610 + i, n_features=max(n, 1), null_point_every=k) for i, (n, k) in enumerate(specs)]
    ref, cur, sia = _upload_pair(ctx, fps, max_feat=1200)
    empty = synth.FramePair(fps[0].cam, fps[3].ref_pyr, fps[3].cur_pyr, np.zeros((0, 2)), np.zeros((0, 3)), np.zeros((0, 3)),
                            np.zeros(0, dtype=np.uint8), fps[3].T_ref_w, fps[3].T_cur_w_true, fps[3].T_cur_w_init)
    sia.upload_pair(3, empty)
    for early in (True, False):
        prm = sia.params(early_stop=early, n_iter=30 if early else 8)
        sia.run(len(fps), prm)
        assert sia.last_run_mode() == 1
        res = sia.download_all(len(fps))
        ref1, cur1, sia1 = _upload_pair(ctx, [fps[0]], max_feat=1200)
        sia1.run(1, prm)
        alone = sia1.download(0)
        _free(sia1, ref1, cur1)
        np.testing.assert_array_equal(np.array(res[0].T_cur_w), np.array(alone.T_cur_w))
        np.testing.assert_array_equal(np.array(res[0].H), np.array(alone.H))
        assert list(res[0].iters) == list(alone.iters)
        for i in (0, 1, 2, 4):
            o = orc.sparse_img_align(fps[i], early_stop=early, n_iter=prm.n_iter)
            got, want = np.array(res[i].T_cur_w), np.array(o.T_cur_w)
            if np.isnan(want).any():
                assert np.isnan(got).any(), i
                continue
            rot, trans = synth.pose_error(got, want)
            assert rot < 1e-4 and trans < 1e-3, (i, early, rot, trans)
            assert res[i].n_tracked == o.n_tracked, i
        assert res[3].n_tracked == 0
        np.testing.assert_array_equal(np.array(res[3].T_cur_w), fps[3].T_cur_w_init)
    _free(sia, ref, cur)


def test_run_with_a_shard_set_is_a_state_error(ctx):
    """svo_hip_sia_run over one patch shard without the exchange would silently solve another problem: it is refused."""
    fp = synth.make_frame_pair(seed=52, n_features=300)
    ref, cur, sia = _upload_pair(ctx, [fp])
    sia.set_shard(1, 2)
    with pytest.raises(hip.SvoHipError):
        sia.run(1, sia.params())
    sia.set_shard(0, 1)
    sia.run(1, sia.params())
    o = orc.sparse_img_align(fp)
    rot, trans = synth.pose_error(np.array(sia.download(0).T_cur_w), np.array(o.T_cur_w))
    assert rot < 1e-4 and trans < 1e-3
    _free(sia, ref, cur)


def test_stepwise_equals_run_and_sharded_sum(ctx):
    """The step-wise entry points reproduce the streaming run() bit for bit and the fused run() to
    summation-order noise, and two patch shards whose reduce rows are added (what the all-reduce does
    across GPUs) give the same normal equations."""
    fp = synth.make_frame_pair(seed=51, n_features=700)
    ref, cur, sia = _upload_pair(ctx, [fp])
    prm = sia.params()
    sia.set_mode(stream=False)
    sia.run(1, prm)
    fused = sia.download(0)
    sia.set_mode(stream=True)
    sia.run(1, prm)
    whole = sia.download(0)
    sia.set_mode(stream=False)
    rot, trans = synth.pose_error(np.array(fused.T_cur_w), np.array(whole.T_cur_w))
    assert rot < 1e-6 and trans < 1e-6
    sia.begin(1, prm)
    for level in range(4, -1, -1):
        sia.level_begin(level)
        for _ in range(prm.n_iter):
            sia.accumulate()
            sia.solve_update()
    sia.finish()
    step = sia.download(0)
    np.testing.assert_array_equal(np.array(step.T_cur_w), np.array(whole.T_cur_w))
    # shards
    ptr, n = sia.reduce_buffer()
    rows = []
    for rank in range(2):
        sia.set_shard(rank, 2)
        sia.begin(1, prm)
        sia.level_begin(3)
        sia.accumulate()
        ctx.sync()
        buf = np.zeros(32)
        ctx.check(ctx.lib.svo_hip_memcpy_d2h(ctx.h, buf.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(32 * 8)), "d2h")
        rows.append(buf)
    sia.set_shard(0, 1)
    sia.begin(1, prm)
    sia.level_begin(3)
    sia.accumulate()
    ctx.sync()
    full = np.zeros(32)
    ctx.check(ctx.lib.svo_hip_memcpy_d2h(ctx.h, full.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(32 * 8)), "d2h")
    np.testing.assert_allclose(rows[0] + rows[1], full, rtol=1e-12, atol=1e-9)
    assert rows[0][28] + rows[1][28] == full[28] and full[28] > 0
    _free(sia, ref, cur)


def _assert_px_bits_equal(got, want):
    """bitwise equality of two float64 pixel arrays (NaN payloads included)"""
    np.testing.assert_array_equal(np.ascontiguousarray(got, dtype=np.float64).view(np.uint64),
                                  np.ascontiguousarray(want, dtype=np.float64).view(np.uint64))


def test_align2d_against_reference_fixture(ctx, golden):
    """feature_alignment::align2D outputs recorded from the reference's own code: the lane-per-patch kernel walks the
    pixels in the reference's order, so the converged flags are EQUAL and the refined pixels BIT-IDENTICAL."""
    g = golden("align.npz")
    cur = g["cur"]
    h, w = cur.shape
    pyr = hip.Pyramid(ctx, w, h, 1, 1)
    pyr.upload(0, [cur])
    for budget in np.unique(g["n_iter"]):
        sel = np.where(g["n_iter"] == budget)[0]
        conv, px, iters = hip.align2d_batch(ctx, pyr, 0, 0, g["pwb"][sel], g["patch"][sel], int(budget), g["px_in"][sel])
        np.testing.assert_array_equal(conv, g["ok"][sel].astype(bool))
        _assert_px_bits_equal(px, g["px_out"][sel])
    # the separate 8x8 ref_patch argument is honoured (the reference reads it, not the interior of the bordered patch)
    sel = np.where(g["n_iter"] == 10)[0][:64]
    other = g["patch"][sel][::-1].copy()
    c1, p1, _ = hip.align2d_batch(ctx, pyr, 0, 0, g["pwb"][sel], other, 10, g["px_in"][sel])
    for j, i in enumerate(sel):
        ok_o, px_o, _ = orc.align2d(cur, g["pwb"][i], other[j], 10, g["px_in"][i])
        assert bool(c1[j]) == bool(ok_o)
        _assert_px_bits_equal(p1[j], px_o)
    pyr.destroy()


def test_align1d_against_reference_fixture(ctx, golden):
    """feature_alignment::align1D outputs recorded from the reference's own code (secondary row a-7): equal flags,
    bit-identical pixels and h_inv (the serial f32 sum of J0^2 included)."""
    g = golden("align.npz")
    cur = g["cur"]
    pyr = hip.Pyramid(ctx, cur.shape[1], cur.shape[0], 1, 1)
    pyr.upload(0, [cur])
    sel = np.where(g["n_iter"] == 10)[0]
    conv, px, hinv, iters = hip.align1d_batch(ctx, pyr, 0, 0, g["pwb"][sel], g["dirs"][sel], 10, g["px_in"][sel])
    np.testing.assert_array_equal(conv, g["ok1"][sel].astype(bool))
    _assert_px_bits_equal(px, g["px_out1"][sel])
    _assert_px_bits_equal(hinv, g["hinv"][sel])
    assert conv.sum() > 100
    pyr.destroy()


def test_align2d_batch_c2_shape(ctx):
    """BASELINE config C2's align2D batch (5000 patches) against the oracle: everything equal."""
    ac = seedsynth.make_align_case(n=5000)
    pyr = hip.Pyramid(ctx, ac.cam.width, ac.cam.height, 5, 1)
    pyr.upload(0, ac.cur_pyr)
    conv, px, iters = hip.align2d_batch(ctx, pyr, 0, 0, ac.pwb, ac.patch, 10, ac.px_init)
    ok_o = np.zeros(len(px), dtype=bool)
    px_o = np.zeros_like(px)
    it_o = np.zeros(len(px), dtype=np.int32)
    for i in range(len(px)):
        ok_o[i], px_o[i], it_o[i] = orc.align2d(ac.cur_pyr[0], ac.pwb[i], ac.patch[i], 10, ac.px_init[i])
    np.testing.assert_array_equal(conv, ok_o)
    np.testing.assert_array_equal(iters, it_o)
    _assert_px_bits_equal(px, px_o)
    # ragged tails: every batch size around the 64-patch wave boundary gives the same per-patch answers
    for n in (1, 63, 64, 65, 127, 129):
        c, p, it = hip.align2d_batch(ctx, pyr, 0, 0, ac.pwb[:n], ac.patch[:n], 10, ac.px_init[:n])
        np.testing.assert_array_equal(c, ok_o[:n])
        _assert_px_bits_equal(p, px_o[:n])
    pyr.destroy()


def test_update_seed_and_tau_batches(ctx):
    rng = np.random.default_rng(5)
    n = 100000
    a = rng.uniform(5, 30, n).astype(np.float32)
    b = rng.uniform(5, 30, n).astype(np.float32)
    mu = rng.uniform(0.2, 1.0, n).astype(np.float32)
    zr = rng.uniform(0.8, 2.0, n).astype(np.float32)
    s2 = (zr * zr / 36 * rng.uniform(0.01, 1.0, n)).astype(np.float32)
    tau2 = np.full(n, 1e-2, dtype=np.float32) * rng.uniform(0.1, 2, n).astype(np.float32)
    x = (mu + rng.normal(size=n).astype(np.float32) * np.sqrt(tau2)).astype(np.float32)
    tau2[7] = -1.0                                # NaN guard: seed untouched
    ga, gb, gmu, gs2 = hip.update_seed_batch(ctx, x, tau2, a, b, mu, zr, s2)
    m = 5000
    want = np.array([orc.update_seed(float(x[i]), float(tau2[i]), [a[i], b[i], mu[i], zr[i], s2[i]]) for i in range(m)], dtype=np.float32)
    got = np.stack([ga[:m], gb[:m], gmu[:m], zr[:m], gs2[:m]], axis=1)
    np.testing.assert_allclose(got, want, rtol=3e-6, atol=0)           # the bound if exp() differed by an ulp between the libms ...
    same = (got.view(np.uint32) == want.view(np.uint32)).all(axis=1)
    assert same.mean() >= 0.999, same.mean()                           # ... in fact bit-identical (20 000 of 20 000 when probed)
    assert ga[7] == a[7] and gs2[7] == s2[7]
    # known-answer vector of the reference
    ka, kb, kmu, ks2 = hip.update_seed_batch(ctx, [0.52], [0.01], [10.0], [10.0], [0.5], [1.0], [np.float32(1.0) / 36])
    np.testing.assert_allclose([ka[0], kb[0], kmu[0], ks2[0]], [10.4296455, 9.88126183, 0.511521995, 0.0118117034], rtol=3e-7)
    # computeTau
    T = synth.se3_from_twist([0.08, 0.01, -0.02], [0.01, -0.02, 0.005])
    f = synth.cam2world(synth.Camera.default(), rng.uniform(50, 400, (4096, 2)))
    z = rng.uniform(0.5, 5.0, 4096)
    ang = 2.0 * np.arctan(1.0 / (2.0 * 500.0))
    tau = hip.compute_tau_batch(ctx, T, f, z, ang)
    want = np.array([orc.compute_tau(T, f[i], z[i], ang) for i in range(4096)])
    np.testing.assert_allclose(tau, want, rtol=1e-11)                  # acos / sin differ by ulps between the libms (observed 4e-13)


def test_depth_filter_update_parity(ctx):
    """Config C2 shape at reduced count: integer outcomes bit-exact, floats within f32 noise."""
    sc = seedsynth.make_seed_case(n_seeds=20000, seed=9)
    kf = hip.Pyramid(ctx, sc.cam.width, sc.cam.height, 5, 1)
    cf = hip.Pyramid(ctx, sc.cam.width, sc.cam.height, 5, 1)
    kf.upload(0, sc.ref_pyr)
    cf.upload(0, sc.cur_pyr)
    sb = hip.SeedBatch(ctx, sc.px, sc.f, sc.level, sc.a, sc.b, sc.mu, sc.z_range, sc.sigma2)
    a, b, mu, s2 = sc.a.copy(), sc.b.copy(), sc.mu.copy(), sc.sigma2.copy()
    for it in range(3):          # three consecutive frames' worth of updates on the same pair
        hip.depth_filter_update(ctx, kf, 0, cf, 0, sc.cam, sc.T_ref_w, sc.T_cur_w, sb)
        o = orc.update_seeds(sc.cam, sc.ref_pyr, sc.cur_pyr, sc.T_ref_w, sc.T_cur_w, sc.px, sc.f, sc.level, a, b, mu,
                             sc.z_range, s2)
        st = sb.status.download()
        nz = sb.n_zmssd.download()
        np.testing.assert_array_equal(st, o["status"])                      # every seed takes the reference's decision
        np.testing.assert_array_equal(nz, o["n_zmssd"])                     # integer search work: exact
        np.testing.assert_array_equal(sb.n_align.download(), o["n_align_iters"])
        np.testing.assert_array_equal(sb.search_level.download(), o["search_level"])      # Matcher::search_level_
        _assert_px_bits_equal(sb.px_cur.download(), o["px_cur"])                          # Matcher::px_cur_ (NaN unless updated)
        upd = st >= hip.SEED_UPDATED
        z = sb.z.download()
        np.testing.assert_allclose(z[upd], o["z"][upd], rtol=1e-12)         # bit-identical match pixel -> same triangulation
        gmu = sb.mu.download()
        np.testing.assert_allclose(gmu[upd], mu[upd], rtol=3e-6)            # exp()/acos() differ by ulps between libms
        # keep both sides in lock-step for the next round
        sb.reset_state(a, b, mu, s2)
    assert (o["status"] == hip.SEED_CONVERGED).sum() > 0 or True
    _free(sb, kf, cf)


def test_device_pyramid_matches_generator(ctx):
    fp = synth.make_frame_pair(seed=3, n_features=10)
    pyr = hip.Pyramid(ctx, 640, 480, 5, 2)
    pyr.upload_level0_and_build(1, fp.ref_pyr[0])
    for l in range(5):
        np.testing.assert_array_equal(pyr.download_level(1, l), fp.ref_pyr[l])
    pyr.destroy()


# ------------------------------------------------------------------------------------------------
# BASELINE.json full sizes: checked through size-independent properties + oracle spot checks
# ------------------------------------------------------------------------------------------------

def test_full_size_c1_batch_properties(ctx):
    """C1 as bench.py runs it: 256 pairs x 2000 patches, 5 levels x 30 evaluations (fixed work)."""
    fps = [synth.make_frame_pair(seed=12345 + i, n_features=2000) for i in range(4)]
    B = 256
    ref, cur, sia = _upload_pair(ctx, [fps[i % 4] for i in range(B)])
    prm = sia.params(early_stop=False)
    sia.run(B, prm)
    res = sia.download_all(B)
    sia.run(B, prm)
    res2 = sia.download_all(B)
    for i in range(B):
        r = res[i]
        assert list(r.T_cur_w) == list(res[i % 4].T_cur_w)          # replicas agree bit for bit
        assert list(r.T_cur_w) == list(res2[i].T_cur_w)              # and run to run (no atomics)
        assert list(r.iters)[:5] == [30] * 5
        assert r.n_precompute_patches == 5 * 2000 and r.n_tracked == 2000
    for i in range(4):
        o = orc.sparse_img_align(fps[i], early_stop=False)
        rot, trans = synth.pose_error(np.array(res[i].T_cur_w), np.array(o.T_cur_w))
        assert rot < 1e-7 and trans < 1e-7
        assert res[i].n_residual_patches == o.n_residual_patches     # the same patches left the image on both sides
        rot, trans = synth.pose_error(np.array(res[i].T_cur_w), fps[i].T_cur_w_true)
        assert rot < 1e-3 and trans < 2e-3                            # and it is the right pose
        H = np.array(res[i].H).reshape(6, 6)
        np.testing.assert_array_equal(H, H.T)
        assert np.linalg.eigvalsh(H).min() > 0
    _free(sia, ref, cur)


def test_large_launch_of_small_frames_picks_two_pairs_per_cu(ctx):
    """C0-sized frames (200 patches) in a launch with more than two pairs per compute unit: svo_hip_sia_run chooses
    the 4-wave shape of the fused kernel by itself (no environment override); every slot agrees with the oracle run of
    its scene, replicas and repeated runs agree bit for bit."""
    assert not hip.SIA_DEFAULT_OPTIONS
    fps = [synth.make_frame_pair(seed=777 + i, n_features=200, width=320, height=240) for i in range(6)]
    B = 528
    ref, cur, sia = _upload_pair(ctx, [fps[i % 6] for i in range(B)])
    for early in (True, False):
        prm = sia.params(early_stop=early)
        sia.run(B, prm)
        assert sia.last_run_mode() == 1
        res = sia.download_all(B)
        sia.run(B, prm)
        res2 = sia.download_all(B)
        for i in range(B):
            assert list(res[i].T_cur_w) == list(res[i % 6].T_cur_w)
            assert list(res[i].T_cur_w) == list(res2[i].T_cur_w)
        for i in range(6):
            o = orc.sparse_img_align(fps[i], early_stop=early)
            rot, trans = synth.pose_error(np.array(res[i].T_cur_w), np.array(o.T_cur_w))
            if early:
                # the exits compare f32 chi2 values that differ in the last bits between any two summation orders
                # (DESIGN.md section 7): a last, tiny update may be accepted on one side and rolled back on the other
                assert rot < 1e-4 and trans < 1e-3, (i, rot, trans)
            else:
                assert rot < 1e-7 and trans < 1e-7, (i, rot, trans)     # library default = the reference's arithmetic
            assert res[i].n_tracked == o.n_tracked
    _free(sia, ref, cur)


def test_1280x720_pair_parity(ctx, sia_mode):
    """BASELINE config C3's frame size (one of the 8 concurrent 1280x720 pairs, 2000 patches)."""
    fp = synth.make_frame_pair(seed=99, width=1280, height=720, n_features=2000)
    ref, cur, sia = _upload_pair(ctx, [fp])
    sia.run(1, sia.params())
    r = sia.download(0)
    o = orc.sparse_img_align(fp)
    rot, trans = synth.pose_error(np.array(r.T_cur_w), np.array(o.T_cur_w))
    assert rot < 1e-4 and trans < 1e-3, (rot, trans)
    assert r.n_tracked == o.n_tracked == 2000
    _free(sia, ref, cur)


def test_full_size_c4_seeds_properties(ctx):
    """C4's per-node seed count: 1M seeds on a 1280x720 keyframe.  Properties: valid outcomes only, run-to-run
    bitwise determinism, shard invariance (two halves == the whole: what seed sharding across GPUs relies
    on), estimates move towards the true depth; plus an oracle spot check on a random subset."""
    sc = seedsynth.make_seed_case(n_seeds=1000000, seed=21, width=1280, height=720)
    kf = hip.Pyramid(ctx, 1280, 720, 5, 1)
    cf = hip.Pyramid(ctx, 1280, 720, 5, 1)
    kf.upload(0, sc.ref_pyr)
    cf.upload(0, sc.cur_pyr)
    sb = hip.SeedBatch(ctx, sc.px, sc.f, sc.level, sc.a, sc.b, sc.mu, sc.z_range, sc.sigma2)
    hip.depth_filter_update(ctx, kf, 0, cf, 0, sc.cam, sc.T_ref_w, sc.T_cur_w, sb)
    st, mu, s2, z, nz = sb.status.download(), sb.mu.download(), sb.sigma2.download(), sb.z.download(), sb.n_zmssd.download()
    assert set(np.unique(st)) <= {0, 1, 2, 3, 4, 5}
    upd = st >= hip.SEED_UPDATED
    assert upd.mean() > 0.95
    assert (s2[upd] < sc.sigma2[upd]).mean() > 0.99                  # a consistent measurement shrinks the variance
    err0 = np.abs(1.0 / sc.mu[upd] - sc.true_depth[upd])
    err1 = np.abs(1.0 / mu[upd] - sc.true_depth[upd])
    assert np.median(err1) < 0.5 * np.median(err0)
    assert np.median(np.abs(z[upd] - sc.true_depth[upd]) / sc.true_depth[upd]) < 0.02
    # determinism
    sb.reset_state(sc.a, sc.b, sc.mu, sc.sigma2)
    hip.depth_filter_update(ctx, kf, 0, cf, 0, sc.cam, sc.T_ref_w, sc.T_cur_w, sb)
    np.testing.assert_array_equal(sb.mu.download(), mu)
    np.testing.assert_array_equal(sb.status.download(), st)
    # shard invariance
    sb.reset_state(sc.a, sc.b, sc.mu, sc.sigma2)
    hip.depth_filter_update(ctx, kf, 0, cf, 0, sc.cam, sc.T_ref_w, sc.T_cur_w, sb, lo=0, hi=400001)
    hip.depth_filter_update(ctx, kf, 0, cf, 0, sc.cam, sc.T_ref_w, sc.T_cur_w, sb, lo=400001, hi=1000000)
    np.testing.assert_array_equal(sb.mu.download(), mu)
    np.testing.assert_array_equal(sb.sigma2.download(), s2)
    np.testing.assert_array_equal(sb.n_zmssd.download(), nz)
    # oracle spot check
    rng = np.random.default_rng(0)
    idx = np.sort(rng.choice(1000000, 3000, replace=False))
    a, b, m, v = (x[idx].copy() for x in (sc.a, sc.b, sc.mu, sc.sigma2))
    o = orc.update_seeds(sc.cam, sc.ref_pyr, sc.cur_pyr, sc.T_ref_w, sc.T_cur_w, sc.px[idx], sc.f[idx], sc.level[idx], a, b, m,
                         sc.z_range[idx].copy(), v)
    np.testing.assert_array_equal(o["status"], st[idx])
    np.testing.assert_array_equal(o["n_zmssd"], nz[idx])
    good = st[idx] >= hip.SEED_UPDATED
    np.testing.assert_allclose(z[idx][good], o["z"][good], rtol=1e-12)
    np.testing.assert_allclose(mu[idx][good], m[good], rtol=3e-6)
    # the same 1 M seeds as ONE device-resident batch: same states, one event per converged / NaN seed, in seed order
    rs = hip.ResidentSeeds(ctx, sc.px, sc.f, sc.level, sc.a, sc.b, sc.mu, sc.z_range, sc.sigma2)
    ev, counts = rs.update(kf, 0, cf, 0, sc.cam, sc.T_ref_w, sc.T_cur_w)
    np.testing.assert_array_equal(rs.status(), st)
    np.testing.assert_array_equal(rs.download()["mu"], mu)
    np.testing.assert_array_equal(ev["index"], np.nonzero((st == hip.SEED_CONVERGED) | (st == hip.SEED_NAN))[0])
    assert counts[1:].tolist() == np.bincount(st, minlength=6).tolist()
    rs.destroy()
    _free(sb, kf, cf)


def test_full_size_c2_seeds_against_the_oracle(ctx):
    """Config C2's own depth-filter workload -- the 100 000 seeds of a 640x480 keyframe bench.py times (seedsynth seed 9):
    valid outcomes, run-to-run determinism, shard invariance, every per-seed integer (status, ZMSSD evaluations, align2D
    iterations, search level) and the matched pixel equal to the CPU oracle's on a 3 000-seed subset, and the same pass
    through a device-resident seed batch (what the drop-in DepthFilter runs) bit for bit."""
    n = 100000
    sc = seedsynth.make_seed_case(n_seeds=n, seed=9)
    kf = hip.Pyramid(ctx, 640, 480, 5, 1)
    cf = hip.Pyramid(ctx, 640, 480, 5, 1)
    kf.upload(0, sc.ref_pyr)
    cf.upload(0, sc.cur_pyr)
    sb = hip.SeedBatch(ctx, sc.px, sc.f, sc.level, sc.a, sc.b, sc.mu, sc.z_range, sc.sigma2)
    hip.depth_filter_update(ctx, kf, 0, cf, 0, sc.cam, sc.T_ref_w, sc.T_cur_w, sb)
    st, mu, s2, z = sb.status.download(), sb.mu.download(), sb.sigma2.download(), sb.z.download()
    nz, na, pc, sl = sb.n_zmssd.download(), sb.n_align.download(), sb.px_cur.download(), sb.search_level.download()
    assert set(np.unique(st)) <= {0, 1, 2, 3, 4, 5} and (st >= hip.SEED_UPDATED).mean() > 0.95
    sb.reset_state(sc.a, sc.b, sc.mu, sc.sigma2)
    hip.depth_filter_update(ctx, kf, 0, cf, 0, sc.cam, sc.T_ref_w, sc.T_cur_w, sb, lo=0, hi=33333)
    hip.depth_filter_update(ctx, kf, 0, cf, 0, sc.cam, sc.T_ref_w, sc.T_cur_w, sb, lo=33333, hi=n)
    np.testing.assert_array_equal(sb.mu.download(), mu)
    np.testing.assert_array_equal(sb.sigma2.download(), s2)
    np.testing.assert_array_equal(sb.status.download(), st)
    rng = np.random.default_rng(3)
    idx = np.sort(rng.choice(n, 3000, replace=False))
    a, b, m, v = (x[idx].copy() for x in (sc.a, sc.b, sc.mu, sc.sigma2))
    o = orc.update_seeds(sc.cam, sc.ref_pyr, sc.cur_pyr, sc.T_ref_w, sc.T_cur_w, sc.px[idx], sc.f[idx], sc.level[idx], a, b, m,
                         sc.z_range[idx].copy(), v)
    np.testing.assert_array_equal(o["status"], st[idx])
    np.testing.assert_array_equal(o["n_zmssd"], nz[idx])
    np.testing.assert_array_equal(o["n_align_iters"], na[idx])
    np.testing.assert_array_equal(o["search_level"], sl[idx])
    good = st[idx] >= hip.SEED_UPDATED
    np.testing.assert_array_equal(o["px_cur"][good], pc[idx][good])          # align2D is bit-identical
    np.testing.assert_allclose(z[idx][good], o["z"][good], rtol=1e-12)
    np.testing.assert_allclose(mu[idx][good], m[good], rtol=3e-6)
    rs = hip.ResidentSeeds(ctx, sc.px, sc.f, sc.level, sc.a, sc.b, sc.mu, sc.z_range, sc.sigma2)
    ev, counts = rs.update(kf, 0, cf, 0, sc.cam, sc.T_ref_w, sc.T_cur_w)
    d = rs.download()
    np.testing.assert_array_equal(d["mu"], mu)
    np.testing.assert_array_equal(d["sigma2"], s2)
    np.testing.assert_array_equal(rs.status(), st)
    assert counts[1:].tolist() == np.bincount(st, minlength=6).tolist() and len(ev) == int(((st == 4) | (st == 5)).sum())
    rs.destroy()
    _free(sb, kf, cf)


def test_c2_align_batch_properties(ctx):
    """5000 patches (C2): refinement is idempotent on converged patches and lands near the true pixel."""
    ac = seedsynth.make_align_case(n=5000, seed=5)
    pyr = hip.Pyramid(ctx, ac.cam.width, ac.cam.height, 5, 1)
    pyr.upload(0, ac.cur_pyr)
    conv, px, iters = hip.align2d_batch(ctx, pyr, 0, 0, ac.pwb, ac.patch, 10, ac.px_init)
    assert conv.mean() > 0.98
    assert np.median(np.linalg.norm(px[conv] - ac.px_true[conv], axis=1)) < 0.3
    conv2, px2, it2 = hip.align2d_batch(ctx, pyr, 0, 0, ac.pwb[conv], ac.patch[conv], 10, px[conv])
    # restarting from a converged estimate stays converged (mean_diff restarts at 0, so allow a second step)
    assert conv2.mean() > 0.995 and (it2 <= 2).mean() > 0.99
    assert np.median(np.linalg.norm(px2[conv2] - px[conv][conv2], axis=1)) < 0.1
    pyr.destroy()


def test_match_direct_batch(ctx):
    """Matcher::findMatchDirect batched (next row f-2): map points seen in 3 keyframes, matched into a new frame."""
    rng = np.random.default_rng(17)
    cam = synth.Camera.default()
    scene = synth.PlaneScene(seed=33, depth=2.0, tilt=(0.1, -0.07))
    kf_poses = [synth.se3_from_twist(rng.uniform(-0.1, 0.1, 3) + [0, 0, 0.3 * k], rng.uniform(-0.03, 0.03, 3)) for k in range(3)]
    T_cur_w = synth.se3_from_twist(rng.uniform(-0.05, 0.05, 3) + [0, 0, 0.8], rng.uniform(-0.02, 0.02, 3))
    kf_pyr = [synth.build_pyramid(scene.render(cam, T)) for T in kf_poses]
    cur_pyr = synth.build_pyramid(scene.render(cam, T_cur_w))
    ref = hip.Pyramid(ctx, cam.width, cam.height, 5, 3)
    cur = hip.Pyramid(ctx, cam.width, cam.height, 5, 1)
    for k in range(3):
        ref.upload(k, kf_pyr[k])
    cur.upload(0, cur_pyr)
    n = 3000
    slot = rng.integers(0, 3, n).astype(np.int32)
    level = rng.choice([0, 0, 1, 2], n).astype(np.int32)
    px_ref = np.stack([rng.uniform(2, cam.width - 2, n), rng.uniform(2, cam.height - 2, n)], axis=1)   # some fail the frame test
    f_ref = synth.cam2world(cam, px_ref)
    pt = np.zeros((n, 3))
    px_cur = np.zeros((n, 2))
    for k in range(3):
        m = slot == k
        pt[m] = scene.intersect(cam, kf_poses[k], px_ref[m, 0], px_ref[m, 1])
    R = synth.rot_matrix(T_cur_w[3:])
    Xc = pt @ R.T + T_cur_w[:3]
    px_cur[:, 0] = cam.fx * Xc[:, 0] / Xc[:, 2] + cam.cx
    px_cur[:, 1] = cam.fy * Xc[:, 1] / Xc[:, 2] + cam.cy
    px_cur += rng.uniform(-1.5, 1.5, (n, 2))
    edge = (rng.uniform(size=n) < 0.2).astype(np.uint8)
    grad = rng.normal(size=(n, 2))
    grad /= np.linalg.norm(grad, axis=1, keepdims=True)
    ok, px_out, sl = hip.match_direct_batch(ctx, ref, cur, 0, cam, np.stack(kf_poses), T_cur_w, slot, px_ref, f_ref, level, pt,
                                            px_cur, edgelet=edge, grad=grad)
    ok_o = np.zeros(n, dtype=bool)
    px_o = np.zeros((n, 2))
    sl_o = np.zeros(n, dtype=np.int32)
    for i in range(n):
        ok_o[i], px_o[i], sl_o[i] = orc.find_match_direct(cam, kf_pyr[slot[i]], cur_pyr, kf_poses[slot[i]], T_cur_w, px_ref[i],
                                                         f_ref[i], int(level[i]), pt[i], px_cur[i], edgelet=bool(edge[i]),
                                                         grad=grad[i])
    framed = np.array([(int(p[0]) // (1 << l) >= 6) and (int(p[0]) // (1 << l) < (cam.width >> l) - 6) and
                       (int(p[1]) // (1 << l) >= 6) and (int(p[1]) // (1 << l) < (cam.height >> l) - 6)
                       for p, l in zip(px_ref, level)])
    assert (~framed).sum() > 10 and not ok[~framed].any()
    np.testing.assert_array_equal(px_out[~framed], px_cur[~framed])        # untouched when the frame test fails
    np.testing.assert_array_equal(sl[framed], sl_o[framed])                # integer decision: exact
    np.testing.assert_array_equal(ok, ok_o)                                # corners (align2D) and edgelets (align1D) alike
    _assert_px_bits_equal(px_out[framed], px_o[framed])
    c2 = framed & (edge == 0) & ok
    assert c2.sum() > 1000 and sl[c2].max() >= 1
    assert (framed & (edge == 1) & ok).sum() > 50
    ref.destroy(); cur.destroy()


@pytest.mark.parametrize("n,expect_mode", [(900, 1), (2500, 1), (2816, 1), (3000, 0)])
def test_feature_count_classes(ctx, n, expect_mode):
    """The fused kernel is instantiated for 1, 2 or 3 tiles per wave (<=1024 / <=2048 / <=2816 features);
    above that svo_hip_sia_run falls back to the streaming kernels.  Same answer everywhere."""
    fp = synth.make_frame_pair(seed=300 + n, n_features=n, border=24)
    ref, cur, sia = _upload_pair(ctx, [fp])
    sia.run(1, sia.params())
    assert sia.last_run_mode() == expect_mode
    r = sia.download(0)
    o = orc.sparse_img_align(fp)
    rot, trans = synth.pose_error(np.array(r.T_cur_w), np.array(o.T_cur_w))
    assert rot < 1e-4 and trans < 1e-3, (rot, trans)
    assert r.n_tracked == o.n_tracked
    _free(sia, ref, cur)


def test_random_small_configs_fuzz(ctx, sia_mode):
    """Many small random problems (sizes around the 64-patch tile boundaries, images of several sizes, level
    ranges, point-less features, features near/outside the border, large motions): every slot must agree with
    its own oracle run, including the degenerate ones (NaN poses when nothing is visible)."""
    rng = np.random.default_rng(2024)
    cases = []
    n_checked = n_degenerate = 0
    for (w, h) in ((320, 240), (640, 480), (336, 208)):
        group = []
        for _ in range(12):
            n = int(rng.choice([1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200, 511]))
            border = int(rng.choice([4, 8, 24, 48]))
            fp = synth.make_frame_pair(seed=int(rng.integers(1, 10**6)), width=w, height=h, n_features=n, border=border,
                                       null_point_every=int(rng.choice([0, 0, 2, 5])), t_mag=float(rng.choice([0.01, 0.05, 0.2])),
                                       r_mag=float(rng.choice([0.005, 0.03])))
            group.append(fp)
        cases.append(group)
    for group in cases:
        ref, cur, sia = _upload_pair(ctx, group, max_feat=600)
        for (mx, mn, it, es) in ((4, 0, 30, True), (4, 2, 30, True), (3, 3, 4, False), (2, 0, 3, False)):
            sia.run(len(group), sia.params(max_level=mx, min_level=mn, n_iter=it, early_stop=es))
            res = sia.download_all(len(group))
            for i, fp in enumerate(group):
                o = orc.sparse_img_align(fp, max_level=mx, min_level=mn, n_iter=it, early_stop=es)
                got, want = np.array(res[i].T_cur_w), np.array(o.T_cur_w)
                assert res[i].n_precompute_patches == o.n_precompute_patches          # integer work: always exact
                # With a handful of patches the 6x6 system is rank deficient: the pivoted LDLT then amplifies
                # last-bit differences of H into arbitrary steps (in the reference too), so poses are only
                # compared for well-posed problems; degenerate ones must simply not fault.
                well_posed = o.n_tracked >= 24 and not np.isnan(want).any() and synth.pose_error(want, fp.T_cur_w_true)[0] < 0.02
                if not well_posed:
                    n_degenerate += 1
                    continue
                n_checked += 1
                assert res[i].n_tracked == o.n_tracked, (i, mx, mn)
                rot, trans = synth.pose_error(got, want)
                assert rot < 1e-4 and trans < 1e-3, (i, mx, mn, it, es, rot, trans, len(fp.px))
        _free(sia, ref, cur)
    assert n_checked > 40 and n_degenerate > 5


def test_depth_filter_all_paths(ctx):
    """Seeds chosen to take every branch of updateSeeds / findEpipolarMatchDirect: behind the camera, outside
    the frame, short epipolar segment (direct align), one-chunk search, multi-chunk search (> 64 steps),
    search skipped (> 1000 steps), NaN variance, near-border features.  Integer outcomes exact vs the oracle."""
    rng = np.random.default_rng(77)
    sc = seedsynth.make_seed_case(n_seeds=6000, seed=31, baseline=0.35, border=12)
    n = len(sc.px)
    # rotate the current camera so that a part of the keyframe leaves its field of view
    T_cur_w = synth.se3_mul(synth.se3_from_twist([0.0, 0.0, 0.0], [0.0, 0.22, 0.0]), sc.T_cur_w)
    scene_img = sc.cur_pyr      # images of the unrotated pose: content does not matter for branch coverage
    a, b, mu, zr, s2 = (v.copy() for v in (sc.a, sc.b, sc.mu, sc.z_range, sc.sigma2))
    k = n // 6
    s2[:k] *= 1e-4                                   # tight seeds: epipolar segment < 2 px -> direct align
    s2[k:2 * k] *= 30.0                              # loose seeds: long epipolar lines (multi-chunk, some > 1000 steps)
    mu[2 * k:2 * k + 200] = 1e-3                     # very far hypothesis
    mu[2 * k + 200:2 * k + 400] = -0.2               # negative inverse depth: behind the camera
    s2[2 * k + 400:2 * k + 420] = np.nan             # NaN variance
    s2[3 * k:3 * k + 300] *= 20000.0                 # absurdly loose: > 1000 steps -> search skipped (matcher.cpp:283-288)
    kf = hip.Pyramid(ctx, sc.cam.width, sc.cam.height, 5, 1)
    cf = hip.Pyramid(ctx, sc.cam.width, sc.cam.height, 5, 1)
    kf.upload(0, sc.ref_pyr)
    cf.upload(0, scene_img)
    sb = hip.SeedBatch(ctx, sc.px, sc.f, sc.level, a, b, mu, zr, s2)
    hip.depth_filter_update(ctx, kf, 0, cf, 0, sc.cam, sc.T_ref_w, T_cur_w, sb)
    st, nz, na = sb.status.download(), sb.n_zmssd.download(), sb.n_align.download()
    gmu, gs2, gb, gz = sb.mu.download(), sb.sigma2.download(), sb.b.download(), sb.z.download()
    oa, ob, om, os2 = a.copy(), b.copy(), mu.copy(), s2.copy()
    o = orc.update_seeds(sc.cam, sc.ref_pyr, scene_img, sc.T_ref_w, T_cur_w, sc.px, sc.f, sc.level, oa, ob, om, zr.copy(), os2)
    counts = np.bincount(o["status"], minlength=6)
    assert counts[0] > 50 and counts[1] > 50 and counts[2] > 50 and counts[3] > 50, counts      # the case covers the branches
    assert (o["n_zmssd"] > 64).sum() > 20                                # multi-chunk searches happened
    assert ((o["n_zmssd"] == 0) & (o["n_align_iters"] > 0)).sum() > 50   # direct-align path happened
    np.testing.assert_array_equal(st, o["status"])                       # every branch decision equals the CPU path's
    np.testing.assert_array_equal(nz, o["n_zmssd"])                      # search work is integer-exact for EVERY seed
    np.testing.assert_array_equal(na, o["n_align_iters"])
    np.testing.assert_array_equal(sb.search_level.download(), o["search_level"])
    _assert_px_bits_equal(sb.px_cur.download(), o["px_cur"])
    failed = st <= hip.SEED_NO_MATCH
    np.testing.assert_array_equal(gb[failed], ob[failed])                # untouched, or b++ on a failed match: exact
    assert ((st == hip.SEED_NO_MATCH) & (gb == b + 1)).sum() == (st == hip.SEED_NO_MATCH).sum()
    upd = st >= hip.SEED_UPDATED
    np.testing.assert_allclose(gz[upd], o["z"][upd], rtol=1e-12)
    np.testing.assert_allclose(gmu[upd], om[upd], rtol=3e-6)
    nanseed = np.isnan(s2)
    assert (st[nanseed] == o["status"][nanseed]).all()
    _free(sb, kf, cf)


# ---- the HIP path against the reference's OWN compiled member functions (tests/golden/*_ref.npz, made by
# ---- oracle/gen_golden.py from oracle/ref/ref_objects.cpp; see tests/test_oracle_reference_objects.py)
def _ref_cases():
    from oracle import gen_golden
    return gen_golden.SIA_REF_CASES


@pytest.mark.parametrize("case", _ref_cases(), ids=[c[0] for c in _ref_cases()])
def test_sparse_img_align_against_reference_run(ctx, sia_mode, golden, case):
    """svo_hip_sia_run against SparseImgAlign::run executed by the reference's own code: pose within the north-star
    tolerance (observed: 1e-13), tracked-patch count exact, H of the last evaluation to 1e-9 relative."""
    from oracle import gen_golden
    name, kw, max_level, min_level, n_iter = case
    g = golden("sia_ref.npz")
    fp = gen_golden.make_sia_case(kw)
    ref, cur, sia = _upload_pair(ctx, [fp], max_feat=max(len(fp.px), 1))
    prm = sia.params(max_level=max_level, min_level=min_level, n_iter=n_iter, eps=1e-6, early_stop=True)
    sia.run(1, prm)
    r = sia.download(0)
    rot, trans = synth.pose_error(np.array(r.T_cur_w), g[name + "_T"])
    assert rot < 1e-4 and trans < 1e-3, (rot, trans)            # north_star tolerance
    assert rot < 2e-5 and trans < 5e-5, (rot, trans)            # what chi2-order exit flips can cost at most here
    assert r.n_tracked == int(g[name + "_n_tracked"])
    assert int(r.stop) == int(g[name + "_stop"])
    if len(fp.px):
        same_iters = all(r.iters[l] == int(g[name + "_iter"][l]) + 1 for l in range(min_level, max_level + 1))
        if same_iters:                                          # same evaluation sequence: everything agrees closely
            assert rot < 1e-7 and trans < 1e-7, (rot, trans)     # 5e-9 in the large-motion case, 1e-13 otherwise
            H = np.array(r.H)
            assert np.abs(H - g[name + "_H"]).max() <= 1e-6 * np.abs(g[name + "_H"]).max()
    _free(sia, ref, cur)


@pytest.mark.parametrize("case", [c for c in _ref_cases() if c[1].get("n_features", 1)], ids=[c[0] for c in _ref_cases() if c[1].get("n_features", 1)])
def test_fixed_work_mode_against_the_reference_members(ctx, sia_mode, golden, case):
    """The bench's workload -- exactly n_iter evaluations per level -- against the reference's compiled computeResiduals /
    solve / update driven for exactly that many evaluations (tests/golden/sia_ref.npz `_fw_*`): no data-dependent control
    flow on either side, so the poses agree to summation-order noise amplified by the solve (large motion: 1e-8)."""
    from oracle import gen_golden
    name, kw, max_level, min_level, n_iter = case
    g = golden("sia_ref.npz")
    fp = gen_golden.make_sia_case(kw)
    ref, cur, sia = _upload_pair(ctx, [fp], max_feat=len(fp.px))
    sia.run(1, sia.params(max_level=max_level, min_level=min_level, n_iter=n_iter, eps=1e-6, early_stop=False))
    r = sia.download(0)
    assert all(r.iters[level] == n_iter for level in range(min_level, max_level + 1))
    assert r.n_tracked == int(g[name + "_fw_n_tracked"])
    rot, trans = synth.pose_error(np.array(r.T_cur_w), g[name + "_fw_T"])
    bound = 1e-7 if _tight() else 5e-7                          # (the opt-in f32-moments level on a 102-patch frame: 2.7e-7 m)
    assert rot < bound and trans < bound, (rot, trans)
    H = np.array(r.H)
    assert np.abs(H - g[name + "_fw_H"]).max() <= 1e-6 * np.abs(g[name + "_fw_H"]).max()
    assert abs(r.chi2 - float(g[name + "_fw_chi2"])) <= 1e-4 * float(g[name + "_fw_chi2"])
    _free(sia, ref, cur)


@pytest.mark.parametrize("case", _ref_cases(), ids=[c[0] for c in _ref_cases()])
def test_moments_f32_arithmetic_against_reference_run_and_exact_level(ctx, golden, case):
    """The opt-in SVO_HIP_SIA_ARITH_MOMENTS_F32 level (the reference's residuals and chi2, a patch's two gradient moments
    summed in f32) against SparseImgAlign::run executed by the reference's own code and against the library default (EXACT)
    on the same object: H_ bit for bit, iteration counts, tracked patches and stop flag equal, poses within 1e-7 of each
    other and of the reference where the evaluation sequence is the same."""
    from oracle import gen_golden
    name, kw, max_level, min_level, n_iter = case
    g = golden("sia_ref.npz")
    fp = gen_golden.make_sia_case(kw)
    assert not hip.SIA_DEFAULT_OPTIONS
    ref, cur, sia = _upload_pair(ctx, [fp], max_feat=max(len(fp.px), 1))
    prm = sia.params(max_level=max_level, min_level=min_level, n_iter=n_iter, eps=1e-6, early_stop=True)
    sia.run(1, prm)                                             # nothing set: the library default
    e = sia.download(0)
    sia.set_option(hip.SIA_OPT_ARITH, hip.SIA_ARITH_EXACT)      # ... which IS the reference's arithmetic: bit for bit
    sia.run(1, prm)
    e2 = sia.download(0)
    assert [float(v).hex() for v in e.T_cur_w] == [float(v).hex() for v in e2.T_cur_w] and list(e.iters) == list(e2.iters)
    sia.set_option(hip.SIA_OPT_ARITH, hip.SIA_ARITH_MOMENTS_F32)
    sia.run(1, prm)
    r = sia.download(0)
    assert list(r.H) == list(e.H) or any(np.isnan(r.H))          # H comes from the per-level gradient sums, not from the residuals
    assert list(r.iters) == list(e.iters) and r.n_tracked == e.n_tracked == int(g[name + "_n_tracked"]) and int(r.stop) == int(e.stop) == int(g[name + "_stop"])
    rot, trans = synth.pose_error(np.array(r.T_cur_w), g[name + "_T"])
    assert rot < 1e-4 and trans < 1e-3, (rot, trans)            # north_star tolerance
    if len(fp.px) >= 16:                                        # (a frame of a handful of patches wanders on rounding noise in the reference itself)
        d_rot, d_trans = synth.pose_error(np.array(r.T_cur_w), np.array(e.T_cur_w))
        assert d_rot < 1e-7 and d_trans < 1e-7, (d_rot, d_trans)
    _free(sia, ref, cur)


@pytest.mark.parametrize("case", _ref_cases(), ids=[c[0] for c in _ref_cases()])
def test_fast_arithmetic_against_reference_run(ctx, golden, case):
    """SVO_HIP_SIA_ARITH_FAST (contracted interpolation, f32 sums over a patch's 16 pixels: opt-in, fused kernel) against
    SparseImgAlign::run executed by the reference's own code: within the north-star tolerance always, within 1e-6 of the
    reference where the evaluation sequence is the same (observed 1e-8), counters exact."""
    from oracle import gen_golden
    name, kw, max_level, min_level, n_iter = case
    g = golden("sia_ref.npz")
    fp = gen_golden.make_sia_case(kw)
    ref, cur, sia = _upload_pair(ctx, [fp], max_feat=max(len(fp.px), 1))
    sia.set_option(hip.SIA_OPT_ARITH, hip.SIA_ARITH_FAST)
    prm = sia.params(max_level=max_level, min_level=min_level, n_iter=n_iter, eps=1e-6, early_stop=True)
    sia.run(1, prm)
    assert sia.last_run_mode() == (1 if len(fp.px) <= 2816 else 0)       # (a frame above 2816 features: the streaming kernels, always EXACT)
    r = sia.download(0)
    rot, trans = synth.pose_error(np.array(r.T_cur_w), g[name + "_T"])
    assert rot < 1e-4 and trans < 1e-3, (rot, trans)            # north_star tolerance
    assert int(r.stop) == int(g[name + "_stop"])
    if len(fp.px):
        same_iters = all(r.iters[l] == int(g[name + "_iter"][l]) + 1 for l in range(min_level, max_level + 1))
        if same_iters:
            assert r.n_tracked == int(g[name + "_n_tracked"])
            assert rot < 1e-6 and trans < 1e-6, (rot, trans)
            H = np.array(r.H)
            assert np.abs(H - g[name + "_H"]).max() <= 1e-6 * np.abs(g[name + "_H"]).max()   # H does not depend on the residuals
    _free(sia, ref, cur)


def test_fast_arithmetic_close_to_exact_on_the_bench_scene(ctx):
    """The two arithmetic flavours of the fused kernel on bench-sized frames (2000 patches, L4..L0, fixed 30 evaluations
    per level): same patches tracked, poses within 1e-6 of each other (observed 1e-8), and both within the north-star
    tolerance of the oracle."""
    fps = [synth.make_frame_pair(seed=4100 + i, n_features=2000) for i in range(3)]
    poses = {}
    for arith in (hip.SIA_ARITH_EXACT, hip.SIA_ARITH_FAST):
        ref, cur, sia = _upload_pair(ctx, fps)
        sia.set_option(hip.SIA_OPT_ARITH, arith)
        sia.run(len(fps), sia.params(early_stop=False))
        assert sia.last_run_mode() == 1
        poses[arith] = [(np.array(sia.download(i).T_cur_w), sia.download(i).n_tracked) for i in range(len(fps))]
        _free(sia, ref, cur)
    for i, fp in enumerate(fps):
        (Te, ne), (Tf, nf) = poses[hip.SIA_ARITH_EXACT][i], poses[hip.SIA_ARITH_FAST][i]
        assert ne == nf
        rot, trans = synth.pose_error(Tf, Te)
        assert rot < 1e-6 and trans < 1e-6, (rot, trans)
        o = orc.sparse_img_align(fp, early_stop=False)
        rot, trans = synth.pose_error(Tf, o.T_cur_w)
        assert rot < 1e-4 and trans < 1e-3, (rot, trans)


def test_find_epipolar_match_direct_against_reference_fixture(ctx, golden):
    """svo_hip_epipolar_match_batch_dev against Matcher::findEpipolarMatchDirect executed by the reference's own code on
    real frames (epi_ref.npz: 600 seeds, four kinds of depth interval, 21 failures): the return value, the search level
    and the refined pixel of EVERY seed equal the reference's; epipolar length and depth to 1e-12."""
    from oracle import gen_golden
    g = golden("epi_ref.npz")
    sc, d_est, d_min, d_max = gen_golden.epi_case_inputs()
    kf = hip.Pyramid(ctx, sc.cam.width, sc.cam.height, 5, 1)
    cf = hip.Pyramid(ctx, sc.cam.width, sc.cam.height, 5, 1)
    kf.upload(0, sc.ref_pyr)
    cf.upload(0, sc.cur_pyr)
    r = hip.epipolar_match_batch(ctx, kf, 0, cf, 0, sc.cam, sc.T_ref_w, sc.T_cur_w, sc.px, sc.f, sc.level, d_est, d_min, d_max)
    g_ok = g["ok"].astype(bool)
    np.testing.assert_array_equal(r["ok"], g_ok)
    np.testing.assert_array_equal(r["search_level"], g["search_level"])
    np.testing.assert_allclose(r["epi_length"], g["epi_length"], rtol=1e-12)
    _assert_px_bits_equal(r["px_cur"][g_ok], g["px_cur"][g_ok])
    np.testing.assert_allclose(r["depth"][g_ok], g["depth"][g_ok], rtol=1e-12)
    assert (r["depth"][~g_ok] == 0).all()
    assert 0 < (~g_ok).sum() < 100 and ((r["n_zmssd"] == 0) & g_ok).sum() > 100 and (r["n_zmssd"] > 0).sum() > 300
    _free(kf, cf)


def _camera_cases():
    from oracle import gen_golden
    return gen_golden.CAMERA_REF_CASES


@pytest.mark.parametrize("case", _camera_cases(), ids=[c[0] for c in _camera_cases()])
def test_camera_model_against_reference_fixture(ctx, golden, case):
    """The device's world2cam (pinhole and radtan), distortion-free cam2world and isInFrame against the reference's own
    compiled vk::PinholeCamera / vk::AbstractCamera members (camera_ref.npz): bit-identical pixels and bearings, equal flags."""
    from oracle import gen_golden
    g = golden("camera_ref.npz")
    name = case[0]
    cam, xyz, uv, px, obs = gen_golden.camera_ref_inputs(case)
    p_xyz, p_uv, f_px, _ = hip.camera_batch(ctx, cam, xyz=xyz, uv=uv, px=px)
    _assert_px_bits_equal(p_xyz, g[name + "_px_of_xyz"])
    _assert_px_bits_equal(p_uv, g[name + "_px_of_uv"])
    if name + "_f_of_px" in g.files:
        _assert_px_bits_equal(f_px, g[name + "_f_of_px"])
    else:       # distorted cam2world: cv::undistortPoints is third-party (parity unpinned): HIP == oracle restatement
        np.testing.assert_allclose(f_px, orc.cam2world(cam, px), rtol=0, atol=1e-15)
    for boundary, level in ((0, 0), (8, 0), (8, 1), (6, 2), (9, 3)):
        _, _, _, plain = hip.camera_batch(ctx, cam, obs=obs, boundary=boundary, level=-1)
        _, _, _, lev = hip.camera_batch(ctx, cam, obs=obs, boundary=boundary, level=level)
        np.testing.assert_array_equal(plain, g["%s_in_b%d" % (name, boundary)])
        np.testing.assert_array_equal(lev, g["%s_in_b%d_l%d" % (name, boundary, level)])


def test_match_direct_against_reference_fixture(ctx, golden):
    """svo_hip_match_direct_batch_dev against Matcher::findMatchDirect executed by the reference's own code."""
    from oracle import gen_golden
    g = golden("match_direct_ref.npz")
    fp, px_in, lvl, edge, grad = gen_golden.match_direct_inputs()
    cam = fp.cam
    ref = hip.Pyramid(ctx, cam.width, cam.height, 5, 1)
    cur = hip.Pyramid(ctx, cam.width, cam.height, 5, 1)
    ref.upload(0, fp.ref_pyr)
    cur.upload(0, fp.cur_pyr)
    n = len(px_in)
    ok, px_out, sl = hip.match_direct_batch(ctx, ref, cur, 0, cam, fp.T_ref_w[None, :], fp.T_cur_w_true,
                                            np.zeros(n, dtype=np.int32), fp.px, fp.f, lvl, fp.pos, px_in,
                                            edgelet=edge, grad=grad)
    g_ok = g["ok"].astype(bool)
    chosen = g["search_level"] >= 0                               # -1: the reference returned before choosing a level
    np.testing.assert_array_equal(sl[chosen], g["search_level"][chosen])        # integer decision: exact
    np.testing.assert_array_equal(px_out[~chosen], px_in[~chosen])              # untouched when the frame test fails
    assert not ok[~chosen].any()
    np.testing.assert_array_equal(ok, g_ok)                                     # every item: the reference's verdict
    _assert_px_bits_equal(px_out, g["px_out"])                                  # and its pixel, bit for bit
    assert (chosen & (edge == 0) & ok).sum() > 100 and (chosen & (edge == 1) & ok).sum() > 20
    ref.destroy(); cur.destroy()


# ---- next rows f-4: pose_optimizer::optimizeGaussNewton, Point::optimize, and the shared 6x6 LDLT ----
def test_ldlt6_device_is_bit_identical_to_eigen(ctx, golden):
    """The one-lane pivoted LDL^T of both Gauss-Newton solvers against Eigen's own results (algebra.npz, made by the
    reference build): bit for bit, rank-deficient and all-zero matrices included."""
    g = golden("algebra.npz")
    x = hip.ldlt6_solve_batch(ctx, g["H"], g["b"])
    np.testing.assert_array_equal(x, g["x"])
    rng = np.random.default_rng(3)
    Hs, bs = [], []
    for t in range(500):
        M = rng.normal(size=(int(rng.integers(2, 40)), 6)) * rng.uniform(0.01, 100, 6)
        if t % 7 == 0:                                         # a transposition at nearly every step
            M = M[:, rng.permutation(6)] * np.array([1e4, 1e4, 1e4, 1.0, 1.0, 1.0])[rng.permutation(6)]
        Hs.append((M.T @ M).reshape(36)); bs.append(rng.normal(size=6))
    Hs, bs = np.array(Hs), np.array(bs)
    x = hip.ldlt6_solve_batch(ctx, Hs, bs)
    import ctypes
    for i in range(len(Hs)):
        xo = np.zeros(6)
        orc.lib().svo_orc_ldlt6_solve(orc._p(orc.f64(Hs[i]), ctypes.c_double), orc._p(orc.f64(bs[i]), ctypes.c_double),
                                      orc._p(xo, ctypes.c_double))
        np.testing.assert_array_equal(x[i], xo)


def test_point_optimize_against_reference_fixture(ctx, golden):
    """svo_hip_point_optimize_batch_dev against Point::optimize executed by the reference's own compiled point.cpp."""
    g = golden("refine_ref.npz")
    pos0, off, Ts, fs, pos_true, iters = synth.make_point_opt_cases()
    for n_iter in (5, 20):
        sel = np.where(iters == n_iter)[0]
        o2 = np.zeros(len(sel) + 1, dtype=np.int32)
        T2, f2 = [], []
        for k, i in enumerate(sel):
            T2.append(Ts[off[i]:off[i + 1]]); f2.append(fs[off[i]:off[i + 1]])
            o2[k + 1] = o2[k] + (off[i + 1] - off[i])
        out, it = hip.point_optimize_batch(ctx, pos0[sel], o2, np.concatenate(T2), np.concatenate(f2), n_iter=n_iter)
        np.testing.assert_array_equal(out, g["point_out"][sel])          # same statements, same order: bit-identical
        assert (it >= 1).all() and (it <= n_iter).all()


@pytest.mark.parametrize("seed,n", [(5, 400), (6, 1200), (7, 37), (9, 3000)])
def test_pose_optimize_parity(ctx, seed, n):
    """svo_hip_pose_optimize against the oracle restatement of pose_optimizer::optimizeGaussNewton: the selection
    steps (MAD scale, medians) exact, the pose to 1e-10, the same observations removed."""
    pc = synth.make_pose_opt_case(seed=seed, n=n)
    em = abs(pc.cam.fx)
    o, hp_o = orc.pose_optimize(em, pc.T_f_w_init, pc.f, pc.pos, pc.level, pc.has_point)
    r, hp = hip.pose_optimize(ctx, pc.T_f_w_init, pc.f, pc.pos, pc.level, pc.has_point, em)
    assert r.ran == 1 and r.n_iter_done == o.n_iter_done
    assert r.estimated_scale == o.estimated_scale                         # k-th element of the f32 errors: exact
    rot, trans = synth.pose_error(np.array(r.T_f_w), np.array(o.T_f_w))
    assert rot < 1e-10 and trans < 1e-10, (rot, trans)
    assert abs(r.error_init - o.error_init) <= 1e-12 * o.error_init       # evaluated at the same initial pose
    assert abs(r.error_final - o.error_final) <= 1e-8 * o.error_final
    diff = hp != hp_o
    assert diff.sum() <= 1                                               # only an observation sitting on the threshold may flip
    assert abs(int(r.num_obs) - int(o.num_obs)) <= 1 and abs(r.n_deleted - o.n_deleted) <= 1
    Co, Cr = np.array(o.Cov), np.array(r.Cov)
    assert np.abs(Cr - Co).max() <= 1e-6 * np.abs(Co).max()
    rot_t, tr_t = synth.pose_error(np.array(r.T_f_w), pc.T_f_w_true)
    rot_0, tr_0 = synth.pose_error(pc.T_f_w_init, pc.T_f_w_true)
    assert rot_t < 0.3 * rot_0 and tr_t < 0.3 * tr_0


def test_pose_optimize_batch_and_edge_cases(ctx):
    cases = [synth.make_pose_opt_case(seed=20 + k, n=n) for k, n in enumerate((300, 1, 800, 64))]
    em = abs(cases[0].cam.fx)
    B, max_n = len(cases) + 1, 800
    T = np.zeros((B, 7)); f = np.zeros((B, max_n, 3)); pos = np.zeros((B, max_n, 3))
    f[..., 2] = 1.0
    lvl = np.zeros((B, max_n), dtype=np.int32); hp = np.zeros((B, max_n), dtype=np.uint8); nf = np.zeros(B, dtype=np.int32)
    for k, pc in enumerate(cases):
        n = len(pc.level)
        T[k], f[k, :n], pos[k, :n], lvl[k, :n], hp[k, :n], nf[k] = pc.T_f_w_init, pc.f, pc.pos, pc.level, pc.has_point, n
    T[B - 1] = cases[0].T_f_w_init                                        # last frame: no observation has a point
    nf[B - 1] = 100
    res, hp_out = hip.pose_optimize_batch(ctx, T, f, pos, lvl, hp, nf, em)
    for k, pc in enumerate(cases):
        o, hp_o = orc.pose_optimize(em, pc.T_f_w_init, pc.f, pc.pos, pc.level, pc.has_point)
        n = len(pc.level)
        assert res[k].ran == o.ran
        if o.ran:
            rot, trans = synth.pose_error(np.array(res[k].T_f_w), np.array(o.T_f_w))
            assert rot < 1e-9 and trans < 1e-9, (k, rot, trans)
            assert res[k].estimated_scale == o.estimated_scale
            assert (hp_out[k, :n] != hp_o).sum() <= 1
    assert res[B - 1].ran == 0 and list(res[B - 1].T_f_w) == list(T[B - 1]) and not hp_out[B - 1].any()


def test_point_optimize_host_buffer_entry(ctx):
    """svo_hip_point_optimize_batch (host buffers) gives what the device-pointer entry gives."""
    pos0, off, Ts, fs, _, _ = synth.make_point_opt_cases(n_points=64)
    ref_out, ref_it = hip.point_optimize_batch(ctx, pos0, off, Ts, fs, n_iter=5)
    p = np.ascontiguousarray(pos0, dtype=np.float64).copy()
    o = np.ascontiguousarray(off, dtype=np.int32)
    T, f = np.ascontiguousarray(Ts, dtype=np.float64), np.ascontiguousarray(fs, dtype=np.float64)
    it = np.zeros(64, dtype=np.int32)
    ctx.check(ctx.lib.svo_hip_point_optimize_batch(ctx.h, 64, 5, p.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p),
                                                   T.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p),
                                                   it.ctypes.data_as(C.c_void_p)), "point_optimize_batch")
    np.testing.assert_array_equal(p, ref_out)
    np.testing.assert_array_equal(it, ref_it)


# ---- next row f-3: FastDetector::detect and Seed::Seed on the device ----
@pytest.mark.parametrize("kind", ["scene", "noise", "blocks"])
def test_detect_features_exact(ctx, kind):
    """svo_hip_detect_features against the oracle restatement of FastDetector::detect: integer / exact-f32 work, so
    positions, levels and scores are equal bit for bit, with and without occupied cells."""
    rng = np.random.default_rng(8)
    cam = synth.Camera.default()
    if kind == "scene":
        img = synth.make_frame_pair(seed=12345, n_features=10).ref_pyr[0]
    elif kind == "noise":
        img = rng.integers(0, 256, (480, 640)).astype(np.uint8)
    else:
        img = np.kron(rng.integers(0, 256, (30, 40)), np.ones((16, 16))).astype(np.uint8)
        img = np.clip(img.astype(np.int32) + rng.integers(-3, 4, img.shape), 0, 255).astype(np.uint8)
    pyr_host = synth.build_pyramid(img)
    pyr = hip.Pyramid(ctx, 640, 480, 5, 1)
    pyr.upload(0, pyr_host)
    for occupancy in (None, (rng.uniform(size=32 * 24) < 0.3).astype(np.uint8)):
        px_o, lvl_o, sc_o = orc.detect_features(pyr_host, n_pyr_levels=3, cell_size=20, occupancy=occupancy)
        px, f, lvl, sc = hip.detect_features(ctx, pyr, 0, cam, n_pyr_levels=3, cell_size=20, occupancy=occupancy)
        assert len(px_o) > (50 if kind == "scene" else 300)
        np.testing.assert_array_equal(px, px_o.astype(np.float64))
        np.testing.assert_array_equal(lvl, lvl_o)
        np.testing.assert_array_equal(sc, sc_o)
        np.testing.assert_array_equal(f, synth.cam2world(cam, px_o.astype(np.float64)))      # Feature::f = cam2world(px)
    # other grid sizes / level counts
    for cell, nl in ((30, 2), (16, 5)):
        px_o, lvl_o, sc_o = orc.detect_features(pyr_host, n_pyr_levels=nl, cell_size=cell)
        px, _, lvl, sc = hip.detect_features(ctx, pyr, 0, None, n_pyr_levels=nl, cell_size=cell)
        np.testing.assert_array_equal(px, px_o.astype(np.float64))
        np.testing.assert_array_equal(lvl, lvl_o)
        np.testing.assert_array_equal(sc, sc_o)
    pyr.destroy()


def test_seed_init_batch(ctx):
    for dm, dn in ((2.2, 1.0), (3.7123, 0.49), (1e-3, 1e-4)):
        got = hip.seed_init_batch(ctx, 1000, dm, dn)
        want = seedsynth.seed_ctor(dm, dn, 1000)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)


def test_detected_seeds_feed_the_depth_filter(ctx):
    """The producer and the consumer together: seeds detected on a keyframe go through one DepthFilter update."""
    sc = seedsynth.make_seed_case(n_seeds=16, seed=3)
    cam = sc.cam
    ref = hip.Pyramid(ctx, cam.width, cam.height, 5, 1); cur = hip.Pyramid(ctx, cam.width, cam.height, 5, 1)
    ref.upload(0, sc.ref_pyr); cur.upload(0, sc.cur_pyr)
    px, f, lvl, score = hip.detect_features(ctx, ref, 0, cam)
    n = len(px)
    assert n > 50
    zbar = float(np.median(sc.true_depth))
    a, b, mu, zr, s2 = hip.seed_init_batch(ctx, n, 1.1 * zbar, 0.5 * zbar)
    seeds = hip.SeedBatch(ctx, px, f, lvl, a, b, mu, zr, s2)
    hip.depth_filter_update(ctx, ref, 0, cur, 0, cam, sc.T_ref_w, sc.T_cur_w, seeds)
    ctx.sync()
    status = seeds.status.download()
    a2, b2, mu2, zr2, s22 = (v.copy() for v in (a, b, mu, zr, s2))
    o = orc.update_seeds(cam, sc.ref_pyr, sc.cur_pyr, sc.T_ref_w, sc.T_cur_w, px, f, lvl, a2, b2, mu2, zr2, s22)
    np.testing.assert_array_equal(status, o["status"])
    assert (status == 3).mean() > 0.5                      # most detected corners are matched and updated
    seeds.free(); ref.destroy(); cur.destroy()


def test_packed_pyramid_upload_from_pinned_memory(ctx):
    """svo_hip_pyramid_upload_packed: a batch of pyramids in the device layout, one transfer from page-locked memory."""
    rng = np.random.default_rng(12)
    B = 3
    pyr = hip.Pyramid(ctx, 320, 240, 5, B)
    lib = ctx.lib
    pb, w_, h_, nl_, b_ = C.c_size_t(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
    base = C.c_void_p()
    ctx.check(lib.svo_hip_pyramid_info(pyr.h, C.byref(w_), C.byref(h_), C.byref(nl_), C.byref(b_), C.byref(pb), C.byref(base)), "info")
    assert (w_.value, h_.value, nl_.value, b_.value) == (320, 240, 5, B)
    host = C.c_void_p()
    ctx.check(lib.svo_hip_malloc_host(ctx.h, C.byref(host), C.c_size_t(B * pb.value)), "malloc_host")
    pyrs = [synth.build_pyramid(rng.integers(0, 256, (240, 320)).astype(np.uint8)) for _ in range(B)]
    for s in range(B):
        for l, im in enumerate(pyrs[s]):
            o = C.c_size_t(0)
            assert lib.svo_hip_pyramid_level_offset(pyr.h, l, C.byref(o)) == 0
            C.memmove(host.value + s * pb.value + o.value, im.ctypes.data, im.nbytes)
    ctx.check(lib.svo_hip_pyramid_upload_packed(pyr.h, 0, B, C.cast(host, C.POINTER(C.c_uint8))), "packed")
    ctx.sync()
    for s in range(B):
        for l in range(5):
            np.testing.assert_array_equal(pyr.download_level(s, l), pyrs[s][l])
    assert lib.svo_hip_pyramid_upload_packed(pyr.h, 2, 2, C.cast(host, C.POINTER(C.c_uint8))) != 0      # out of range: refused
    ctx.check(lib.svo_hip_free_host(ctx.h, host), "free_host")
    pyr.destroy()


def test_error_conventions(ctx):
    """SURVEY 8b 'Error conventions': failure = status code + message, never an abort; a refused call leaves the
    object usable."""
    lib = ctx.lib
    fp = synth.make_frame_pair(seed=12345, width=320, height=240, n_features=50, border=24)
    ref, cur, sia = _upload_pair(ctx, [fp])
    prm = sia.params(max_level=4, min_level=0, n_iter=30, eps=1e-6, early_stop=True)
    bad = sia.params(max_level=7, min_level=0, n_iter=30, eps=1e-6, early_stop=True)       # level beyond the pyramid
    assert lib.svo_hip_sia_run(sia.h, 1, C.byref(bad)) == -1
    assert b"invalid argument" in lib.svo_hip_last_error(ctx.h)
    assert lib.svo_hip_sia_run(sia.h, 5, C.byref(prm)) != 0                               # more slots than the batch
    assert lib.svo_hip_sia_run(None, 1, C.byref(prm)) == -1
    assert lib.svo_hip_pyramid_upload(ref.h, 9, None) == -1
    with pytest.raises(hip.SvoHipError):
        ref.upload(3, fp.ref_pyr)                                                          # slot out of range
    with pytest.raises(hip.SvoHipError):
        hip.pose_optimize(ctx, fp.T_ref_w, fp.f, fp.pos, np.zeros(50, dtype=np.int32), fp.has_point, -1.0)   # error multiplier <= 0
    px = np.zeros((4, 2)); out = C.c_int32(0)
    assert lib.svo_hip_detect_features(ctx.h, ref.h, 0, None, 9, 20, None, C.c_double(10.0), C.byref(out),
                                       px.ctypes.data_as(C.c_void_p), None, px.ctypes.data_as(C.c_void_p), None) == -1   # 9 levels
    # the objects are still good
    sia.run(1, prm)
    if sia.last_run_mode() == 1:     # the fused kernel keeps no per-pixel caches: asking for them is a state error, not stale data
        buf = np.zeros((50, 16), dtype=np.float32)
        assert lib.svo_hip_sia_download_caches(sia.h, 0, buf.ctypes.data_as(C.c_void_p), None, None, None) == -4
    # a keyframe slot / level outside the pyramids handed to findMatchDirect is refused per item, never indexed
    n = 8
    ok, px_out, _ = hip.match_direct_batch(ctx, ref, cur, 0, fp.cam, fp.T_ref_w[None, :], fp.T_cur_w_true,
                                           np.array([0, 1, -1, 0, 7, 0, 0, 0], dtype=np.int32), fp.px[:n], fp.f[:n],
                                           np.array([0, 0, 0, 9, 0, -1, 0, 0], dtype=np.int32), fp.pos[:n], fp.px[:n].copy())
    assert not ok[[1, 2, 3, 4, 5]].any()
    np.testing.assert_array_equal(px_out[[1, 2, 3, 4, 5]], fp.px[[1, 2, 3, 4, 5]])
    r = sia.download(0)
    o = orc.sparse_img_align(fp, n_iter=30, early_stop=True)
    rot, trans = synth.pose_error(np.array(r.T_cur_w), np.array(o.T_cur_w))
    assert rot < 1e-9 and trans < 1e-9             # library default = the reference's arithmetic
    _free(sia, ref, cur)


def test_converged_seed_records_packed_on_device(ctx):
    """svo_hip_seed_compact_converged_dev: the gather payload, in seed order, equals what the host builds."""
    import torch
    from android_svo_amd import dist as svodist
    sc = seedsynth.make_seed_case(n_seeds=20000, seed=9)
    kf = hip.Pyramid(ctx, 640, 480, 5, 1); cf = hip.Pyramid(ctx, 640, 480, 5, 1)
    kf.upload(0, sc.ref_pyr); cf.upload(0, sc.cur_pyr)
    scale = np.where(np.arange(20000) % 3 == 0, 3e-4, 1.0).astype(np.float32)     # a third of the seeds is about to converge
    sigma2 = (sc.sigma2 * scale).astype(np.float32)
    sb = hip.SeedBatch(ctx, sc.px, sc.f, sc.level, sc.a, sc.b, sc.mu, sc.z_range, sigma2)
    hip.depth_filter_update(ctx, kf, 0, cf, 0, sc.cam, sc.T_ref_w, sc.T_cur_w, sb)
    ctx.sync()
    rec = svodist.gather_converged_device(ctx, sb, 1000, torch.cuda.current_stream()).cpu().numpy()
    status, mu, s2, xyz = sb.status.download(), sb.mu.download(), sb.sigma2.download(), sb.xyz.download()
    conv = np.where(status == 4)[0]
    assert 100 < len(conv) < len(status)
    np.testing.assert_array_equal(rec[:, 0], conv + 1000)
    np.testing.assert_array_equal(rec[:, 1], mu[conv].astype(np.float64))
    np.testing.assert_array_equal(rec[:, 2], s2[conv].astype(np.float64))
    np.testing.assert_array_equal(rec[:, 3:], xyz[conv])
    sb.free(); kf.destroy(); cf.destroy()


# 262 144 seeds = 1024 blocks of 256 = one chunk of the block scan: the sizes around it carry a total from chunk to chunk
@pytest.mark.parametrize("n", [1, 255, 256, 257, 262144, 262145, 2 * 262144 + 77])
def test_converged_seed_compaction_across_scan_chunks(ctx, n):
    """svo_hip_seed_compact_converged_dev on its own, over status arrays with runs of 256-seed blocks without a converged
    seed, runs of blocks with nothing else, and random blocks; the blocks on both sides of a chunk boundary hold converged
    seeds.  Expected records and count from numpy: ascending index, id_offset + i, mu and sigma2 widened to f64, xyz."""
    import ctypes as C
    import torch
    rng = np.random.default_rng(20260 + n)
    n_blocks = (n + 255) // 256
    kinds = np.full(n_blocks, 2)                               # 0: no converged seed, 1: only converged seeds, 2: random
    if n_blocks >= 9:
        runs = [(0, 3), (1, 2), (2, 4)]
        while sum(r[1] for r in runs) < n_blocks:
            runs.append((int(rng.integers(0, 3)), int(rng.integers(1, 40))))
        kinds = np.concatenate([np.full(length, k) for k, length in runs])[:n_blocks]
        assert all((kinds == k).any() for k in (0, 1, 2))
    others = np.array([hip.SEED_ERASED, hip.SEED_BEHIND, hip.SEED_NOT_IN_FRAME, hip.SEED_NO_MATCH, hip.SEED_UPDATED, hip.SEED_NAN])
    kind_of_seed = np.repeat(kinds, 256)[:n]
    conv = np.where(kind_of_seed == 2, rng.random(n) < 0.3, kind_of_seed == 1)
    for edge in (262144, 2 * 262144):                          # the last block of a chunk and the first of the next
        conv[[i for i in (edge - 1, edge) if i < n]] = True
    status = np.where(conv, hip.SEED_CONVERGED, others[rng.integers(0, len(others), n)]).astype(np.int32)
    mu = rng.random(n, dtype=np.float32) + np.float32(0.1)
    sigma2 = rng.random(n, dtype=np.float32) * np.float32(1e-3)
    xyz = rng.standard_normal((n, 3))
    id_offset = 3_000_000_017                                  # a rank's first seed id: beyond 32 bits, exact in f64
    dev = [torch.from_numpy(a).cuda() for a in (status, mu, sigma2, xyz)]
    rec = torch.full((n, 6), -1.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.check(ctx.lib.svo_hip_seed_compact_converged_dev(
        ctx.h, n, C.c_longlong(id_offset), C.c_void_p(dev[0].data_ptr()), C.c_void_p(dev[1].data_ptr()), C.c_void_p(dev[2].data_ptr()),
        C.c_void_p(dev[3].data_ptr()), C.c_void_p(rec.data_ptr()), C.c_void_p(cnt.data_ptr())), "seed_compact_converged")
    ctx.sync()
    idx = np.nonzero(conv)[0]
    assert int(cnt.item()) == len(idx)
    want = np.column_stack([(id_offset + idx).astype(np.float64), mu[idx].astype(np.float64), sigma2[idx].astype(np.float64), xyz[idx]])
    got = rec.cpu().numpy()
    np.testing.assert_array_equal(got[:len(idx)], want)
    np.testing.assert_array_equal(got[len(idx):], -1.0)        # nothing written behind the records


def test_frame_pipeline_stages_together(ctx):
    """The per-frame data path of FrameHandlerMono::processFrame on the device, stage by stage against the oracle chain:
    SparseImgAlign -> reprojection matching (findMatchDirect) -> pose_optimizer::optimizeGaussNewton -> Point::optimize."""
    fp = synth.make_frame_pair(seed=4242, n_features=500, border=40)
    cam = fp.cam
    n = len(fp.px)
    ref, cur, sia = _upload_pair(ctx, [fp])
    prm = sia.params(max_level=4, min_level=2, n_iter=30, eps=1e-6, early_stop=True)       # shipping default L4 -> L2
    sia.run(1, prm)
    T_sia = np.array(sia.download(0).T_cur_w)
    o = orc.sparse_img_align(fp, max_level=4, min_level=2, n_iter=30, early_stop=True)
    rot, trans = synth.pose_error(T_sia, np.array(o.T_cur_w))
    assert rot < 1e-9 and trans < 1e-9

    def project(T):
        Xc = np.stack([synth.se3_act(T, p) for p in fp.pos])
        return np.stack([cam.fx * Xc[:, 0] / Xc[:, 2] + cam.cx, cam.fy * Xc[:, 1] / Xc[:, 2] + cam.cy], axis=1)

    # reprojection matching from the aligned pose
    px_pred = project(T_sia)
    level = np.zeros(n, dtype=np.int32)
    ok, px_m, sl = hip.match_direct_batch(ctx, ref, cur, 0, cam, fp.T_ref_w[None, :], T_sia, np.zeros(n, dtype=np.int32),
                                          fp.px, fp.f, level, fp.pos, px_pred)
    ok_o = np.zeros(n, dtype=bool); px_o = np.zeros((n, 2))
    for i in range(n):
        ok_o[i], px_o[i], _ = orc.find_match_direct(cam, fp.ref_pyr, fp.cur_pyr, fp.T_ref_w, T_sia, fp.px[i], fp.f[i], 0,
                                                    fp.pos[i], px_pred[i])
    np.testing.assert_array_equal(ok, ok_o)
    assert ok.mean() > 0.9
    _assert_px_bits_equal(px_m, px_o)

    # motion-only refinement on the matched observations
    f_obs = synth.cam2world(cam, px_m)
    hp = ok.astype(np.uint8)
    r, hp_out = hip.pose_optimize(ctx, T_sia, f_obs, fp.pos, sl.astype(np.int32), hp, abs(cam.fx))
    ro, hp_o = orc.pose_optimize(abs(cam.fx), T_sia, f_obs, fp.pos, sl.astype(np.int32), hp)
    rot, trans = synth.pose_error(np.array(r.T_f_w), np.array(ro.T_f_w))
    assert rot < 1e-10 and trans < 1e-10
    np.testing.assert_array_equal(hp_out, hp_o)
    e_sia = synth.pose_error(T_sia, fp.T_cur_w_true)
    e_ref = synth.pose_error(np.array(r.T_f_w), fp.T_cur_w_true)
    assert e_ref[0] < 2e-4 and e_ref[1] < 1e-3, (e_sia, e_ref)       # the refined pose stays at the sub-pixel level

    # structure refinement of the points seen in both frames
    sel = np.where(hp_out.astype(bool))[0][:200]
    obs_T = np.stack([np.stack([fp.T_ref_w, np.array(r.T_f_w)]) for _ in sel]).reshape(-1, 7)
    obs_f = np.stack([np.stack([fp.f[i], f_obs[i]]) for i in sel]).reshape(-1, 3)
    off = np.arange(len(sel) + 1, dtype=np.int32) * 2
    pos0 = fp.pos[sel] + np.random.default_rng(1).normal(size=(len(sel), 3)) * 0.01
    out, _ = hip.point_optimize_batch(ctx, pos0, off, obs_T, obs_f, n_iter=5)
    for k in range(len(sel)):
        want, _ = orc.point_optimize(pos0[k], obs_T[2 * k:2 * k + 2], obs_f[2 * k:2 * k + 2], n_iter=5)
        np.testing.assert_array_equal(out[k], want)
    _free(sia, ref, cur)


@pytest.mark.parametrize("tag,max_fts", [("full", 1200), ("cap", 40)])
def test_reproject_cells_against_reference_fixture(ctx, golden, tag, max_fts):
    """svo_hip_reproject_cells (one batched match + the serial cell policy) against the reference's own
    Reprojector::reprojectCell loop: same winners, counters and point bookkeeping; matched pixels bit-identical."""
    from test_oracle_reproject import check_against_fixture
    g = golden("reproject_ref.npz")
    cs = synth.make_reproject_case()
    cam = cs["cam"]
    ref = hip.Pyramid(ctx, cam.width, cam.height, 5, 3); cur = hip.Pyramid(ctx, cam.width, cam.height, 5, 1)
    for k in range(3):
        ref.upload(k, cs["kf_pyr"][k])
    cur.upload(0, cs["cur_pyr"])
    off, ids = synth.flatten_cells(cs, cs["trial"])
    deleted = (cs["ptype"][ids] == synth.TYPE_DELETED).astype(np.uint8)
    res = hip.reproject_cells(ctx, ref, cur, 0, cam, cs["T_kf_w"], cs["T_cur_w"], off, cs["slot"][ids], cs["px_ref"][ids],
                              cs["f_ref"][ids], cs["level"][ids], cs["pos"][ids], deleted, cs["px_cur"][ids], max_fts=max_fts)
    o = orc.reproject_cells(cam, cs["kf_pyr"], cs["T_kf_w"], cs["cur_pyr"], cs["T_cur_w"], off, cs["slot"][ids], cs["px_ref"][ids],
                            cs["f_ref"][ids], cs["level"][ids], cs["pos"][ids], np.zeros(len(ids), np.uint8),
                            np.tile([1.0, 0.0], (len(ids), 1)), deleted, cs["px_cur"][ids], max_fts=max_fts)
    np.testing.assert_array_equal(res["tried"], o["tried"])
    np.testing.assert_array_equal(res["matched"], o["matched"])
    win = check_against_fixture(g, tag, cs, ids, res)
    _assert_px_bits_equal(res["px_cur"][win], g[tag + "_feat_px"])
    ref.destroy(); cur.destroy()


def test_depth_filter_and_detector_with_a_distorted_camera(ctx):
    """cam2world for radtan cameras on the device (the depth filter's triangulation and the detector's bearings): same
    inputs through the oracle and the HIP path."""
    import copy
    sc = seedsynth.make_seed_case(n_seeds=3000, seed=5)
    cam = copy.copy(sc.cam)
    cam.dist = (-0.12, 0.03, 2e-4, -1e-4, 0.0)
    f = np.zeros((3000, 3))
    c = orc.camera(cam)
    import ctypes
    for i in range(3000):
        orc.lib().svo_orc_cam2world(ctypes.byref(c), ctypes.c_double(sc.px[i, 0]), ctypes.c_double(sc.px[i, 1]),
                                    orc._p(f[i], ctypes.c_double))
    kf = hip.Pyramid(ctx, 640, 480, 5, 1); cf = hip.Pyramid(ctx, 640, 480, 5, 1)
    kf.upload(0, sc.ref_pyr); cf.upload(0, sc.cur_pyr)
    sb = hip.SeedBatch(ctx, sc.px, f, sc.level, sc.a, sc.b, sc.mu, sc.z_range, sc.sigma2)
    hip.depth_filter_update(ctx, kf, 0, cf, 0, cam, sc.T_ref_w, sc.T_cur_w, sb)
    ctx.sync()
    a, b, mu, s2 = (v.copy() for v in (sc.a, sc.b, sc.mu, sc.sigma2))
    o = orc.update_seeds(cam, sc.ref_pyr, sc.cur_pyr, sc.T_ref_w, sc.T_cur_w, sc.px, f, sc.level, a, b, mu, sc.z_range.copy(), s2)
    status = sb.status.download()
    np.testing.assert_array_equal(status, o["status"])
    upd = status == 3
    assert upd.sum() > 1000
    assert np.abs(sb.mu.download()[upd] - mu[upd]).max() < 1e-4 * np.abs(mu[upd]).max()
    z_h = sb.z.download()
    assert np.abs(z_h[upd] - o["z"][upd]).max() < 1e-3
    # the detector's bearings for the same camera
    px, fd, lvl, score = hip.detect_features(ctx, kf, 0, cam)
    for i in range(0, len(px), 7):
        want = np.zeros(3)
        orc.lib().svo_orc_cam2world(ctypes.byref(c), ctypes.c_double(px[i, 0]), ctypes.c_double(px[i, 1]), orc._p(want, ctypes.c_double))
        np.testing.assert_array_equal(fd[i], want)
    sb.free(); kf.destroy(); cf.destroy()


def test_next_row_kernels_fuzz(ctx):
    """Odd sizes and degenerate inputs for the next-row kernels, device against oracle."""
    rng = np.random.default_rng(77)
    # detector: image sizes that are not multiples of the cell size, 2..5 levels
    for (w, h, cell, nl) in ((752, 480, 30, 3), (1280, 720, 40, 4), (200, 136, 25, 2), (96, 64, 20, 2)):
        img = rng.integers(0, 256, (h, w)).astype(np.uint8)
        img[h // 4:h // 2, w // 4:w // 2] = 200
        pyr_host = synth.build_pyramid(img, 5)
        pyr = hip.Pyramid(ctx, w, h, 5, 1)
        pyr.upload(0, pyr_host)
        px_o, lvl_o, sc_o = orc.detect_features(pyr_host, n_pyr_levels=nl, cell_size=cell)
        px, _, lvl, sc = hip.detect_features(ctx, pyr, 0, None, n_pyr_levels=nl, cell_size=cell)
        np.testing.assert_array_equal(px, px_o.astype(np.float64))
        np.testing.assert_array_equal(lvl, lvl_o)
        np.testing.assert_array_equal(sc, sc_o)
        pyr.destroy()
    # a featureless image: nothing detected
    pyr = hip.Pyramid(ctx, 160, 120, 5, 1)
    pyr.upload(0, synth.build_pyramid(np.full((120, 160), 77, dtype=np.uint8), 5))
    px, _, lvl, sc = hip.detect_features(ctx, pyr, 0, None)
    assert len(px) == 0
    pyr.destroy()
    # structure refinement: one observation (singular 3x3: LDLT pseudo-inverse), identical observations, far start
    T0 = synth.se3_from_twist([0, 0, 0], [0, 0, 0])
    T1 = synth.se3_from_twist([0.3, 0, 0], [0, 0.05, 0])
    X = np.array([0.2, -0.1, 3.0])
    f0 = X / np.linalg.norm(X)
    X1 = synth.se3_act(T1, X)
    f1 = X1 / np.linalg.norm(X1)
    pos0 = np.stack([X + 0.05, X + 0.05, X * 3.0, X + [0.0, 0.0, -2.9]])
    off = np.array([0, 1, 3, 5, 7], dtype=np.int32)
    obs_T = np.stack([T0, T0, T0, T0, T1, T0, T1])
    obs_f = np.stack([f0, f0, f0, f0, f1, f0, f1])
    out, it = hip.point_optimize_batch(ctx, pos0, off, obs_T, obs_f, n_iter=8)
    for k in range(4):
        want, it_o = orc.point_optimize(pos0[k], obs_T[off[k]:off[k + 1]], obs_f[off[k]:off[k + 1]], n_iter=8)
        np.testing.assert_array_equal(out[k], want)          # NaNs compare equal
        assert it[k] == it_o
    # pose refinement: few observations, all outliers, mixed levels
    for seed, n, frac in ((31, 7, 0.0), (32, 40, 0.9), (33, 3, 0.0), (34, 500, 0.5)):
        pc = synth.make_pose_opt_case(seed=seed, n=n, outlier_frac=frac, null_every=0)
        em = abs(pc.cam.fx)
        o, hp_o = orc.pose_optimize(em, pc.T_f_w_init, pc.f, pc.pos, pc.level, pc.has_point)
        r, hp = hip.pose_optimize(ctx, pc.T_f_w_init, pc.f, pc.pos, pc.level, pc.has_point, em)
        assert r.ran == o.ran
        assert r.estimated_scale == o.estimated_scale                   # selection: exact whatever the data
        if frac > 0.8:
            # nine observations in ten are gross outliers: the weighted problem is ill-posed, rounding decides which of
            # two nearly equal chi2 values is larger and the two runs may stop at different iterations
            assert 1 <= r.n_iter_done <= 10 and np.isfinite(np.array(r.T_f_w)).all()
            continue
        assert r.n_iter_done == o.n_iter_done, (seed, r.n_iter_done, o.n_iter_done)
        To, Tr = np.array(o.T_f_w), np.array(r.T_f_w)
        if np.isfinite(To).all():
            rot, trans = synth.pose_error(Tr, To)
            assert rot < 1e-8 and trans < 1e-8, (seed, rot, trans)
        else:
            assert not np.isfinite(Tr).all()
        assert (hp != hp_o).sum() <= 1
    # reprojection cell loop: no candidates at all
    cs = synth.make_reproject_case(seed=5, n_points=40)
    ref = hip.Pyramid(ctx, 320, 240, 5, 3); cur = hip.Pyramid(ctx, 320, 240, 5, 1)
    for k in range(3):
        ref.upload(k, cs["kf_pyr"][k])
    cur.upload(0, cs["cur_pyr"])
    off0 = np.zeros(cs["n_cells"] + 1, dtype=np.int32)
    e = np.zeros((0, 3))
    res = hip.reproject_cells(ctx, ref, cur, 0, cs["cam"], cs["T_kf_w"], cs["T_cur_w"], off0, np.zeros(0, np.int32), e[:, :2], e,
                              np.zeros(0, np.int32), e, np.zeros(0, np.uint8), e[:, :2])
    assert res["n_matches"] == 0 and res["n_trials"] == 0 and (res["cell_winner"] == -1).all()
    ref.destroy(); cur.destroy()


@pytest.mark.parametrize("wh", [(320, 240), (752, 480), (100, 68)])
def test_level0_batch_upload_builds_all_pyramids_on_device(ctx, wh):
    """svo_hip_pyramid_upload_level0_batch_and_build: level 0 of a run of slots in one strided transfer, coarser
    levels of all of them by one launch per level; same bytes as frame_utils::createImgPyramid per image."""
    w, h = wh
    rng = np.random.default_rng(w)
    B, first = 5, 2
    pyr = hip.Pyramid(ctx, w, h, 4, B + first + 1)
    lib = ctx.lib
    sentinel = synth.build_pyramid(rng.integers(0, 256, (h, w)).astype(np.uint8), 4)
    for slot in (first - 1, first + B):
        pyr.upload(slot, sentinel)
    imgs = [rng.integers(0, 256, (h, w)).astype(np.uint8) for _ in range(B)]
    packed = np.ascontiguousarray(np.stack(imgs))
    ctx.check(lib.svo_hip_pyramid_upload_level0_batch_and_build(
        pyr.h, first, B, packed.ctypes.data_as(C.POINTER(C.c_uint8))), "l0batch")
    ctx.sync()
    for s in range(B):
        want = synth.build_pyramid(imgs[s], 4)
        for l in range(4):
            np.testing.assert_array_equal(pyr.download_level(first + s, l), want[l])
    for slot in (first - 1, first + B):            # neighbours untouched
        for l in range(4):
            np.testing.assert_array_equal(pyr.download_level(slot, l), sentinel[l])
    assert lib.svo_hip_pyramid_upload_level0_batch_and_build(
        pyr.h, first, B + 2, packed.ctypes.data_as(C.POINTER(C.c_uint8))) != 0
    pyr.destroy()
