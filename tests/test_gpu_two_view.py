"""svo_two_view_impl.h (svo_hip_klt_two_view / _download_two_view / _set_lists) against the numpy model of
tests/two_view_reference.py, BY BITS, on every family tests/test_two_view_model_cpu.py proves the inputs reach: result block,
hypothesis counts, mask, inlier list, xyz, poses, points and map_tables.  Then the launch boundaries of the hypothesis kernel,
batch invariance (alone, one of 3 with three camera models, one of 17 in permuted order, 16 of 17), the real chain behind
set_reference + track, the first map through Tracker.set_map, repeated calls, the allocator and the refusals.  All through
set_lists on a 160 x 120 handle unless stated: the stage reads no image.  Every NaN counts as the same NaN."""
import numpy as np
import pytest

import klt_reference as K
import two_view_cases as C
import two_view_reference as M
from android_svo_amd import hip, synth

pytestmark = pytest.mark.gpu

CAM = synth.Camera(C.W, C.H, C.FX, C.FY, C.CX, C.CY)
RESULT_INTS = ("status", "n_in", "hypothesis", "hypothesis_count", "candidate", "candidate_count", "n_inliers", "n_points")
RESULT_F64 = ("depth_median", "scale", "T_cur_from_ref", "T_cur_w")


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


def new_handle(ctx, n_cameras=1, max_features=1024):
    """a handle whose cameras all have a reference (an image that is never read, no features)"""
    pyr = hip.Pyramid(ctx, C.W, C.H, 1, 1)
    pyr.upload_level0_and_build(0, np.zeros((C.H, C.W), np.uint8))
    klt = hip.KltTracker(ctx, C.W, C.H, n_cameras, max_features)
    for c in range(n_cameras):
        klt.set_reference(c, pyr, 0, np.zeros((0, 2), np.float32), np.zeros((0, 3)))
    pyr.destroy()
    return klt


@pytest.fixture(scope="module")
def klt(ctx):
    k = new_handle(ctx, 17)
    yield k
    k.destroy()


def bits(a):
    a = np.ascontiguousarray(a, np.float64)
    return np.where(np.isnan(a), np.uint64(0x7FF8000000000000), a.view(np.uint64))


def set_case(klt, camera, c):
    klt.set_lists(camera, c["px_ref"], c["px_cur"], c["f_ref"], c["f_cur"])


def assert_equal_by_bits(res, dl, want, counts=True):
    for k in RESULT_INTS:
        assert res[k] == want[k], (k, res[k], want[k])
    for k in RESULT_F64:
        np.testing.assert_array_equal(bits(res[k]), bits(want[k]), err_msg=k)
    assert dl["n"] == want["n_in"] and dl["n_inliers"] == want["n_inliers"] and dl["n_points"] == want["n_points"]
    if counts:
        np.testing.assert_array_equal(dl["counts"], want["counts"])
    for k in ("mask", "inliers", "point_index"):
        np.testing.assert_array_equal(dl[k], want[k], err_msg=k)
    np.testing.assert_array_equal(bits(dl["point_pos"]), bits(want["point_pos"]))
    assert (dl["xyz_in_cur"] is None) == (want["xyz_in_cur"] is None)
    if want["xyz_in_cur"] is not None:
        np.testing.assert_array_equal(bits(dl["xyz_in_cur"]), bits(want["xyz_in_cur"]))


def assert_tables_equal(got, want):
    for k, v in want.items():
        g = np.asarray(got[k])
        assert g.shape == np.asarray(v).shape, k
        if g.dtype.kind == "f":
            np.testing.assert_array_equal(bits(g), bits(v), err_msg=k)
        else:
            np.testing.assert_array_equal(g, v, err_msg=k)


@pytest.mark.parametrize("name", C.NAMES)
def test_family_equals_the_model_by_bits(klt, name):
    c, want = C.case(name), C.model(name)
    set_case(klt, 0, c)
    T = None if c["T_ref_w"] is None else c["T_ref_w"][None]
    res = klt.two_view([0], [CAM], T, **c["params"])[0]
    assert_equal_by_bits(res, klt.download_two_view(0), want)
    if want["status"] == M.OK:
        assert_tables_equal(klt.map_tables(0, res, c["T_ref_w"]), M.map_tables(want))


def test_hypothesis_launch_boundaries(klt):
    c = C.case("volume-65")
    set_case(klt, 0, c)
    prev = None
    for H in (1, 63, 64, 65, 256, 257, 1024, 4096):
        p = dict(c["params"], n_hypotheses=H)
        want = M.two_view(c["f_ref"], c["f_cur"], c["px_ref"], c["px_cur"], C.FX, C.W, C.H, **p)
        res = klt.two_view([0], [CAM], **p)[0]
        dl = klt.download_two_view(0)
        assert len(dl["counts"]) == H
        assert_equal_by_bits(res, dl, want)
        if prev is not None:
            np.testing.assert_array_equal(dl["counts"][:len(prev)], prev)           # H1 < H2: the first H1 counts are identical
        prev = dl["counts"]


def test_batch_invariance(ctx, klt):
    names = ["outliers-200-45-0.3", "border", "volume-257", "pose-0.5", "gates-39", "median-nan", "volume-8", "gates-n7", "gates-identical",
             "volume-1024", "median-negative", "outliers-400-30-0.0", "gates-cheirality", "volume-63", "volume-64", "volume-65", "median-run"]
    assert len(names) == 17
    # three camera models: another focal length (another threshold), another image size (another border outcome)
    cams = [CAM, synth.Camera(C.W, C.H, 1.25 * C.FX, C.FY, C.CX, C.CY), synth.Camera(C.W - 12, C.H - 9, C.FX, C.FY, C.CX, C.CY)]

    def want(i):
        c, cam = C.case(names[i]), cams[i % 3]
        return M.two_view(c["f_ref"], c["f_cur"], c["px_ref"], c["px_cur"], cam.fx, cam.width, cam.height, T_ref_w=c["T_ref_w"], **prm)

    prm = dict(M.default_params(), min_inliers=8)
    T = np.stack([M.IDENTITY if C.case(nm)["T_ref_w"] is None else C.case(nm)["T_ref_w"] for nm in names])
    wants = [want(i) for i in range(17)]
    for i, nm in enumerate(names):
        set_case(klt, i, C.case(nm))
    # alone
    alone = {}
    for i in (0, 1, 2):
        res = klt.two_view([i], [cams[i % 3]], T[i:i + 1], **prm)[0]
        alone[i] = (res, klt.download_two_view(i))
        assert_equal_by_bits(*alone[i], wants[i])
    assert wants[2]["n_points"] < 257                                              # the smaller image's border gate decided
    # one of 3, one of 17 in permuted order, 16 of the 17
    for order in ([0, 1, 2], [int(i) for i in np.random.default_rng(5).permutation(17)], [i for i in range(17) if i != 4][::-1]):
        res = klt.two_view(order, [cams[i % 3] for i in order], T[order], **prm)
        for r, i in zip(res, order):
            assert_equal_by_bits(r, klt.download_two_view(i), wants[i])
    # a single listed camera of the big handle: the others' results stay
    res = klt.two_view([9], [cams[0]], T[9:10], **prm)[0]
    assert_equal_by_bits(res, klt.download_two_view(9), wants[9])
    assert_equal_by_bits(alone[1][0], klt.download_two_view(1), wants[1])


def test_real_chain_equals_set_lists(ctx):
    """set_reference + track on test_gpu_klt.py's image case, then two_view: equal to set_lists(download()) + two_view on a second
    handle.  No accuracy claim: the scene is planar."""
    w, h, n = 160, 120, 65
    prev, cur, px = K.gpu_case(w, h, n, 11)
    px = np.ascontiguousarray(px[:n])
    cam = synth.Camera(w, h, 0.78 * w, 0.8 * w, w / 2 - 0.5, h / 2 + 1.25)
    f = hip.camera_batch(ctx, cam, px=px.astype(np.float64))[2]
    pyr = hip.Pyramid(ctx, w, h, 1, 2)
    pyr.upload_level0_batch_and_build(0, [prev, cur])
    a, b = hip.KltTracker(ctx, w, h, 1, 128), hip.KltTracker(ctx, w, h, 2, 128)
    try:
        a.set_reference(0, pyr, 0, px, f)
        with pytest.raises(hip.SvoHipError):
            a.two_view([0], [cam])                                                 # no track since set_reference
        tr = a.track([0], pyr, [1], [cam])[0]
        lists = a.download(0)
        assert tr["n_tracked"] == lists["n"] >= 8
        ra = a.two_view([0], [cam], min_inliers=8)[0]
        da = a.download_two_view(0)
        b.set_reference(1, pyr, 0, px[:0], f[:0])
        b.set_lists(1, lists["px_ref"], lists["px_cur"], lists["f_ref"], lists["f_cur"])
        rb = b.two_view([1], [cam], min_inliers=8)[0]
        assert_equal_by_bits(rb, b.download_two_view(1), dict(ra, **{k: da[k] for k in ("counts", "mask", "inliers", "point_index", "point_pos", "xyz_in_cur")}))
        want = M.two_view(lists["f_ref"], lists["f_cur"], lists["px_ref"], lists["px_cur"], cam.fx, w, h, min_inliers=8)
        assert_equal_by_bits(ra, da, want)
    finally:
        a.destroy(); b.destroy(); pyr.destroy()


def test_first_map_through_set_map(ctx, klt):
    c, want = C.case("pose-0.5"), C.model("pose-0.5")
    set_case(klt, 3, c)
    res = klt.two_view([3], [CAM], c["T_ref_w"][None], **c["params"])[0]
    mp = klt.map_tables(3, res, c["T_ref_w"])
    assert_tables_equal(mp, M.map_tables(want))
    trk = hip.Tracker(ctx, CAM, max_keyframes=2, max_fts=120, max_frame_features=1024)
    try:
        trk.set_map(mp)
        assert trk.map_sizes() == dict(n_kf=2, n_ftr=2 * want["n_points"], n_points=want["n_points"], n_obs=2 * want["n_points"], n_candidates=0)
        assert_tables_equal(trk.download_map(), mp)
    finally:
        trk.destroy()


def test_repeated_calls_lists_untouched_no_allocation(ctx, klt):
    c, want = C.case("outliers-200-30-0.3"), C.model("outliers-200-30-0.3")
    set_case(klt, 5, c)
    before = klt.download(5)
    first = klt.two_view([5], [CAM], **c["params"])[0]
    d1 = klt.download_two_view(5)
    info0 = ctx.info()
    for _ in range(10):
        again = klt.two_view([5], [CAM], **c["params"])[0]
    info1 = ctx.info()
    assert info1["allocator_calls"] == info0["allocator_calls"] and info1["free_calls"] == info0["free_calls"]
    assert_equal_by_bits(first, d1, want)
    assert_equal_by_bits(again, klt.download_two_view(5), want)
    after = klt.download(5)
    for k in ("px_ref", "px_cur", "f_ref", "f_cur", "index"):
        assert before[k].tobytes() == after[k].tobytes(), k
    assert after["n"] == 200 and (after["index"] == np.arange(200)).all()


def test_refusals_leave_lists_and_results_unchanged(ctx, klt):
    c, want = C.case("volume-65"), C.model("volume-65")
    set_case(klt, 6, c)
    res = klt.two_view([6], [CAM], **c["params"])[0]
    lists = klt.download(6)
    bad = [dict(cameras=[17]), dict(cameras=[-1]), dict(cameras=[6, 6]), dict(n_hypotheses=0), dict(n_hypotheses=4097), dict(reproj_thresh=0.0),
           dict(reproj_thresh=float("nan")), dict(map_scale=-1.0), dict(min_inliers=-1)]
    for b in bad:
        cams = b.pop("cameras", [6])
        with pytest.raises(hip.SvoHipError):
            klt.two_view(cams, [CAM] * len(cams), **dict(c["params"], **b))
    fresh = hip.KltTracker(ctx, C.W, C.H, 2, 64)
    try:
        for call in (lambda: fresh.two_view([0], [CAM]), lambda: fresh.set_lists(0, c["px_ref"][:8], c["px_cur"][:8], c["f_ref"][:8], c["f_cur"][:8]),
                     lambda: fresh.download_two_view(0)):
            with pytest.raises(hip.SvoHipError):                                      # no reference / no result
                call()
    finally:
        fresh.destroy()
    with pytest.raises(hip.SvoHipError):
        klt.set_lists(6, np.zeros((1025, 2), np.float32), np.zeros((1025, 2), np.float32), np.zeros((1025, 3)), np.zeros((1025, 3)))
    assert_equal_by_bits(res, klt.download_two_view(6), want)
    after = klt.download(6)
    for k in ("px_ref", "px_cur", "f_ref", "f_cur", "index"):
        assert lists[k].tobytes() == after[k].tobytes(), k
