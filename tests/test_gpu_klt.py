"""svo_klt.hip (the bootstrap's KLT tracker: svo_hip_klt_*) against the numpy model of tests/klt_reference.py, BY BITS: Gaussian
pyramid levels byte-equal; status equal and px_cur bit-equal on every family tests/test_klt_model_cpu.py proves the inputs
reach (random, border, flat, out-of-range, integer coordinates, lost at a coarse level, initial flow leaving the range);
f_cur bit-equal to svo_hip_camera_batch on the same pixels; disparities, median and surviving indices equal to the model.
Shapes: 160 x 120 (2 levels), 346 x 260 (4 levels, odd widths 173 / 87 / 44), one 640 x 480 case; 1, 63, 64, 65, 257 features
(wave and block edges).  Every array svo_hip_klt_download fills carries guard elements (hip.KltTracker.download)."""
import functools

import numpy as np
import pytest

import klt_reference as K
from android_svo_amd import hip, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


def camera_for(w, h, k=0):
    return synth.Camera(w, h, 0.78 * w + 3.5 * k, 0.8 * w - 2.25 * k, w / 2 - 0.5 + k, h / 2 + 1.25 - k)


def radtan_camera(w, h):
    c = camera_for(w, h, 2)
    c.dist = (-0.28, 0.07, 2e-4, -1e-4, 0.0)
    return c


def bearings(px):
    """any unit vectors: f_ref is carried, never computed"""
    f = np.concatenate([np.asarray(px, dtype=np.float64) * 1e-3, np.ones((len(px), 1))], axis=1)
    return f / np.linalg.norm(f, axis=1)[:, None]


@functools.lru_cache(maxsize=None)
def case(w, h, n, seed=11):
    prev, cur, px = K.gpu_case(w, h, max(n, 24), seed)
    if n < 24:
        px = px[3:3 + n]                        # (40, 50): a feature that is tracked
    return prev, cur, np.ascontiguousarray(px[:n])


@functools.lru_cache(maxsize=None)
def model(w, h, n, seed=11):
    prev, cur, px = case(w, h, n, seed)
    return K.track_klt(K.build_pyramid(prev), K.build_pyramid(cur), px, px.copy())


def upload(ctx, imgs):
    h, w = imgs[0].shape
    pyr = hip.Pyramid(ctx, w, h, 1, len(imgs))
    pyr.upload_level0_batch_and_build(0, list(imgs))
    return pyr


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def assert_lists(ctx, got, res, ref, f_ref_in, cam, n_in):
    """the camera's downloaded lists and call result against a klt_reference.track_klt result"""
    assert res["n_in"] == n_in and res["n_tracked"] == len(ref["keep"]) == got["n"]
    np.testing.assert_array_equal(got["index"], ref["keep"].astype(np.int32))
    np.testing.assert_array_equal(bits(got["px_ref"]), bits(ref["px_ref"]))
    np.testing.assert_array_equal(bits(got["px_cur"]), bits(ref["px_cur"]))
    np.testing.assert_array_equal(bits(got["f_ref"]), bits(f_ref_in[ref["keep"]]))
    np.testing.assert_array_equal(bits(got["disparity"]), bits(ref["disparity"]))
    assert bits(np.float64(res["disparity_median"]).reshape(1))[0] == bits(np.float64(ref["median"]).reshape(1))[0]
    if got["n"]:
        f_want = hip.camera_batch(ctx, cam, px=got["px_cur"].astype(np.float64))[2]
        np.testing.assert_array_equal(bits(got["f_cur"]), bits(f_want))


@pytest.mark.parametrize("w,h,levels", [(160, 120, 2), (346, 260, 4), (640, 480, 4)])
def test_gaussian_pyramid_levels_byte_equal(ctx, w, h, levels):
    prev, cur, px = case(w, h, 24)
    pp, pc = K.build_pyramid(prev), K.build_pyramid(cur)
    pyr = upload(ctx, [prev, cur])
    klt = hip.KltTracker(ctx, w, h, 2, 64)
    try:
        assert klt.level_shapes() == [p.shape for p in pp] and len(pp) == levels
        for c in (0, 1):
            klt.set_reference(c, pyr, 0, px, bearings(px))
        res = klt.track([1], pyr, [1], [camera_for(w, h)])
        assert res[0]["n_levels"] == levels
        for l in range(levels):
            assert klt.download_level(0, l).tobytes() == pp[l].tobytes(), l
            assert klt.download_level(1, l).tobytes() == pp[l].tobytes(), l
            if l:
                assert klt.download_level(1, l, current=True).tobytes() == pc[l].tobytes(), l
    finally:
        klt.destroy()
        pyr.destroy()


@pytest.mark.parametrize("w,h,n", [(160, 120, 1), (160, 120, 63), (160, 120, 64), (346, 260, 65), (346, 260, 257), (640, 480, 128)])
def test_one_frame_bit_equal_to_the_model(ctx, w, h, n):
    prev, cur, px = case(w, h, n)
    ref = model(w, h, n)
    cam = camera_for(w, h)
    pyr = upload(ctx, [prev, cur])
    klt = hip.KltTracker(ctx, w, h, 1, n)                  # max_features = n: the arrays are full
    try:
        f = bearings(px)
        klt.set_reference(0, pyr, 0, px, f)
        res = klt.track([0], pyr, [1], [cam])[0]
        got = klt.download(0)
        print("n %d tracked %d (model %d) median %r" % (n, res["n_tracked"], len(ref["keep"]), res["disparity_median"]))
        assert_lists(ctx, got, res, ref, f, cam, n)
    finally:
        klt.destroy()
        pyr.destroy()


def test_initial_flow_that_leaves_the_range(ctx):
    w, h = 160, 120
    prev, cur, px, flow = K.flow_case(w, h, 11)
    ref = K.track_klt(K.build_pyramid(prev), K.build_pyramid(cur), px, flow)
    assert 0 < len(ref["keep"]) < len(px)
    cam = camera_for(w, h)
    pyr = upload(ctx, [prev, cur])
    klt = hip.KltTracker(ctx, w, h, 1, 64)
    try:
        f = bearings(px)
        klt.set_reference(0, pyr, 0, px, f)
        klt.set_flow(0, flow)
        res = klt.track([0], pyr, [1], [cam])[0]
        assert_lists(ctx, klt.download(0), res, ref, f, cam, len(px))
    finally:
        klt.destroy()
        pyr.destroy()


def test_three_frames_shrinking_lists_and_carried_flow(ctx):
    w, h, n = 160, 120, 65
    prev, _, px = case(w, h, n)
    shifts = [(1.7, -0.9), (3.9, -2.2), (6.5, -3.1)]
    frames = []
    for s in shifts:
        im = K.sinusoid_texture(w, h, 11, s)
        im[h // 2 - 20:h // 2 + 20, w // 2 - 20:w // 2 + 20] = 90
        frames.append(im)
    cam = camera_for(w, h)
    pyr = upload(ctx, [prev] + frames)
    klt = hip.KltTracker(ctx, w, h, 1, 80)
    try:
        f = bearings(px)
        klt.set_reference(0, pyr, 0, px, f)
        pp = K.build_pyramid(prev)
        m_ref, m_cur, m_idx, counts = px, px.copy(), np.arange(n), []
        for i, im in enumerate(frames):
            r = K.track_klt(pp, K.build_pyramid(im), m_ref, m_cur)
            m_idx = m_idx[r["keep"]]
            res = klt.track([0], pyr, [1 + i], [cam])[0]
            got = klt.download(0)
            want = dict(r, keep=m_idx)
            assert_lists(ctx, got, res, want, f, cam, len(m_ref))
            m_ref, m_cur = r["px_ref"], r["px_cur"]
            counts.append(len(m_idx))
        print("tracked per frame:", counts)
        assert counts[0] < n and counts[-1] <= counts[0]
    finally:
        klt.destroy()
        pyr.destroy()


def test_a_camera_whose_features_are_all_lost(ctx):
    w, h = 160, 120
    prev, cur, _ = case(w, h, 24)
    px = np.array([[w + 40, 5], [-70, 10], [80, 60], [w + 90.5, h + 80]], dtype=np.float32)   # (80, 60): the flat rectangle
    ref = K.track_klt(K.build_pyramid(prev), K.build_pyramid(cur), px, px.copy())
    assert len(ref["keep"]) == 0
    pyr = upload(ctx, [prev, cur])
    klt = hip.KltTracker(ctx, w, h, 2, 16)
    try:
        klt.set_reference(0, pyr, 0, px, bearings(px))
        klt.set_reference(1, pyr, 0, px[:0], bearings(px[:0]))                     # n = 0 is legal
        for _ in range(2):                                                         # the second call starts from empty lists
            res = klt.track([0, 1], pyr, [1, 1], [camera_for(w, h)] * 2)
            assert [r["n_tracked"] for r in res] == [0, 0] and all(np.isnan(r["disparity_median"]) for r in res)
            assert klt.download(0)["n"] == 0 and klt.download(1)["n"] == 0
        assert res[0]["n_in"] == 0
    finally:
        klt.destroy()
        pyr.destroy()


def test_set_reference_detected_equals_detect_then_set_reference(ctx):
    w, h = 346, 260
    prev, cur, _ = case(w, h, 24)
    cam = camera_for(w, h)
    full = hip.Pyramid(ctx, w, h, 3, 2)
    full.upload_level0_batch_and_build(0, [prev, cur])
    a, b = hip.KltTracker(ctx, w, h, 1, 512), hip.KltTracker(ctx, w, h, 1, 512)
    try:
        px, f, _, _ = hip.detect_features(ctx, full, 0, cam, n_pyr_levels=3, cell_size=20, detection_threshold=10.0)
        n = a.set_reference_detected(0, full, 0, cam, 3, 20, 10.0)
        assert n == len(px) > 50
        b.set_reference(0, full, 0, px.astype(np.float32), f)
        ra, rb = a.track([0], full, [1], [cam])[0], b.track([0], full, [1], [cam])[0]
        assert ra == rb and ra["n_in"] == n
        da, db = a.download(0), b.download(0)
        for key in da:
            assert np.asarray(da[key]).tobytes() == np.asarray(db[key]).tobytes(), key
        # a detection with more features than the handle holds is refused once the count is known
        small = hip.KltTracker(ctx, w, h, 1, 8)
        with pytest.raises(hip.SvoHipError, match=r"\(-1\)"):
            small.set_reference_detected(0, full, 0, cam, 3, 20, 10.0)
        with pytest.raises(hip.SvoHipError, match=r"\(-4\)"):
            small.track([0], full, [1], [cam])
        small.destroy()
    finally:
        a.destroy()
        b.destroy()
        full.destroy()


def _rig(w, h):
    return [camera_for(w, h, 0), radtan_camera(w, h), camera_for(w, h, 5)]


def test_three_camera_models_subsets_and_order(ctx):
    w, h, n = 160, 120, 65
    prev, cur, px = case(w, h, n)
    _, cur2, _ = K.gpu_case(w, h, 24, 11, shift=(-2.3, 1.1))
    cams = _rig(w, h)
    pxs = [px, px[::-1].copy(), px[5:50].copy()]
    pyr = upload(ctx, [prev, cur, cur2])
    grp = hip.KltTracker(ctx, w, h, 3, 80)
    own = [hip.KltTracker(ctx, w, h, 1, 80) for _ in range(3)]
    try:
        for c in range(3):
            grp.set_reference(c, pyr, 0, pxs[c], bearings(pxs[c]))
            own[c].set_reference(0, pyr, 0, pxs[c], bearings(pxs[c]))

        def step(cameras, slots):
            res = grp.track(cameras, pyr, slots, [cams[c] for c in cameras])
            for i, c in enumerate(cameras):
                assert res[i] == own[c].track([0], pyr, [slots[i]], [cams[c]])[0], c
            for c in range(3):                      # the cameras not listed are untouched as well
                dg, do = grp.download(c), own[c].download(0)
                for key in dg:
                    assert np.asarray(dg[key]).tobytes() == np.asarray(do[key]).tobytes(), (c, key)
            return res

        r = step([0, 1, 2], [1, 1, 2])
        assert all(x["n_tracked"] > 0 for x in r)
        step([1], [2])                              # 1 of 3
        step([2, 0], [1, 2])                        # 2 of 3, reversed
        # the radtan camera's bearings are the distorted model's
        d = grp.download(1)
        np.testing.assert_array_equal(bits(d["f_cur"]), bits(hip.camera_batch(ctx, cams[1], px=d["px_cur"].astype(np.float64))[2]))
        assert not np.array_equal(d["f_cur"], hip.camera_batch(ctx, cams[0], px=d["px_cur"].astype(np.float64))[2])
    finally:
        grp.destroy()
        for o in own:
            o.destroy()
        pyr.destroy()


def test_seventeen_cameras_in_one_call(ctx):
    w, h, n = 160, 120, 63
    prev, cur, px = case(w, h, n)
    ref = model(w, h, n)
    cam = camera_for(w, h)
    pyr = upload(ctx, [prev, cur])
    klt = hip.KltTracker(ctx, w, h, 17, 64)
    try:
        f = bearings(px)
        for c in range(17):
            m = n - 2 * c                           # a different count per camera: the first m features
            klt.set_reference(c, pyr, 0, px[:m], f[:m])
        res = klt.track(list(range(17)), pyr, [1] * 17, [cam] * 17)
        for c in range(17):
            m = n - 2 * c
            keep = ref["keep"][ref["keep"] < m]
            sel = np.flatnonzero(ref["keep"] < m)
            disp = ref["disparity"][sel]
            want = dict(keep=keep, px_ref=ref["px_ref"][sel], px_cur=ref["px_cur"][sel], disparity=disp, median=K.upper_median(disp))
            assert_lists(ctx, klt.download(c), res[c], want, f, cam, m)
    finally:
        klt.destroy()
        pyr.destroy()


def test_reads_a_tracker_groups_frame_batch(ctx):
    import map_growth_scenario as sc
    import tracking_chain as tc
    seq = sc.make()["seq"]
    cam = seq["cam"]
    w, h = cam.width, cam.height
    grp = hip.TrackerGroup(ctx, cam, 2, max_keyframes=4, grid_size=tc.CELL, max_fts=tc.MAX_FTS, klt_min_level=2, max_frame_features=1024,
                           max_items=1024)
    klt = hip.KltTracker(ctx, w, h, 2, 64)
    first = upload(ctx, [seq["pyrs"][0][0]])
    try:
        for t in grp.cameras:
            t.upload_keyframe(0, seq["pyrs"][0][0])
            t.set_map(tc.sequence_map(seq))
            t.set_last_frame(seq["T0"], seq["px0"], seq["f0"], np.arange(len(seq["px0"]), dtype=np.int32), kf_slot=0)
        frames = [1, 2]
        grp.track([seq["pyrs"][fr][0] for fr in frames])
        views = [t.last_frame_pyramid() for t in grp.cameras]
        px = np.ascontiguousarray(seq["px0"][:40], dtype=np.float32)
        f = bearings(px)
        pp = K.build_pyramid(seq["pyrs"][0][0])
        for c in range(2):
            klt.set_reference(c, first, 0, px, f)
        res = klt.track([0, 1], views[0][0], [views[0][1], views[1][1]], [cam, cam])
        for c in range(2):
            ref = K.track_klt(pp, K.build_pyramid(seq["pyrs"][frames[c]][0]), px, px.copy())
            assert_lists(ctx, klt.download(c), res[c], ref, f, cam, len(px))
    finally:
        klt.destroy()
        first.destroy()
        grp.destroy()


def test_no_allocator_call_over_ten_warm_calls(ctx):
    w, h, n = 160, 120, 64
    prev, cur, px = case(w, h, n)
    pyr = upload(ctx, [prev, cur])
    klt = hip.KltTracker(ctx, w, h, 2, 64)
    try:
        for c in range(2):
            klt.set_reference(c, pyr, 0, px, bearings(px))
        cams = [camera_for(w, h)] * 2
        klt.track([0, 1], pyr, [1, 1], cams)
        before = ctx.info()
        for i in range(10):
            klt.track([0, 1] if i % 2 else [1], pyr, [1, 0] if i % 2 else [1], cams if i % 2 else cams[:1])
        after = ctx.info()
        assert after["allocator_calls"] == before["allocator_calls"] and after["free_calls"] == before["free_calls"]
    finally:
        klt.destroy()
        pyr.destroy()


def test_every_refusal_leaves_the_state_unchanged(ctx):
    w, h, n = 160, 120, 64
    prev, cur, px = case(w, h, n)
    cam = camera_for(w, h)
    pyr = upload(ctx, [prev, cur])
    other_size = hip.Pyramid(ctx, 176, 144, 1, 1)
    ctx2 = hip.Context(0)
    other_ctx = hip.Pyramid(ctx2, w, h, 1, 2)
    a, b = hip.KltTracker(ctx, w, h, 3, 64), hip.KltTracker(ctx, w, h, 3, 64)
    inval, state = r"\(-1\)", r"\(-4\)"
    try:
        for wrong in (2, 31):
            with pytest.raises(hip.SvoHipError, match=inval):
                hip.KltTracker(ctx, w, h, 1, 64, win_size=wrong)
        f = bearings(px)
        for k in (a, b):
            for c in (0, 1):
                k.set_reference(c, pyr, 0, px, f)
        refusals = [
            (inval, lambda: a.track([0, 3], pyr, [1, 1], [cam, cam])),              # camera out of range
            (inval, lambda: a.track([-1], pyr, [1], [cam])),
            (inval, lambda: a.track([0, 0], pyr, [1, 1], [cam, cam])),              # listed twice
            (inval, lambda: a.track([0], other_size, [0], [cam])),                  # a pyramid of another size
            (inval, lambda: a.track([0], other_ctx, [1], [cam])),                   # ... of another context
            (inval, lambda: a.track([0], None, [1], [cam])),
            (inval, lambda: a.track([0, 1], pyr, [1, 2], [cam, cam])),              # slot out of range
            (inval, lambda: a.track([], pyr, [], [])),
            (state, lambda: a.track([0, 2], pyr, [1, 1], [cam, cam])),              # camera 2 has no reference
            (state, lambda: a.download(2)),
            (state, lambda: a.set_flow(2, px)),
            (inval, lambda: a.set_flow(0, px[:10])),                                # not the camera's count
            (inval, lambda: a.set_reference(0, pyr, 0, np.zeros((65, 2), np.float32), np.zeros((65, 3)))),   # n > max_features
            (inval, lambda: a.set_reference(3, pyr, 0, px, f)),
            (inval, lambda: a.set_reference(0, pyr, 2, px, f)),
            (inval, lambda: a.set_reference(0, other_size, 0, px, f)),
            (inval, lambda: a.set_reference(0, None, 0, px, f)),
            (inval, lambda: a.set_reference_detected(0, pyr, 0, cam, 1, 20, -1.0)),  # the detector's refusals
            (inval, lambda: a.set_reference_detected(0, pyr, 0, None, 1, 20, 10.0)),
            (inval, lambda: a.set_reference_detected(0, pyr, 0, cam, 2, 20, 10.0)),  # more levels than the pyramid has
        ]
        for code, call in refusals:
            with pytest.raises(hip.SvoHipError, match=code):
                call()
        ra, rb = a.track([1, 0], pyr, [1, 1], [cam, cam]), b.track([1, 0], pyr, [1, 1], [cam, cam])
        assert ra == rb and ra[0]["n_tracked"] == len(model(w, h, n)["keep"])
        for c in (0, 1):
            da, db = a.download(c), b.download(c)
            for key in da:
                assert np.asarray(da[key]).tobytes() == np.asarray(db[key]).tobytes(), (c, key)
    finally:
        a.destroy()
        b.destroy()
        other_size.destroy()
        other_ctx.destroy()
        pyr.destroy()
        ctx2.close()
