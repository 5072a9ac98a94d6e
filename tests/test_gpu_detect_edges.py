"""svo_detect.hip against the plain-numpy reference of tests/detect_reference.py on the scenes built there: arcs of 8, 9, 10 and
16 ring pixels at every start position and in both polarities with the misses exactly at t, arcs next to the image border,
equal Shi-Tomasi scores within a level and across hand-built levels, plateaus of equal FAST scores, pixel differences of
exactly 10 and 11, thresholds that are no whole number (the reference's phantom features), that sit on a returned score, inf,
NaN and -0.0, levels without an interior pixel, one-pixel cells, every slot of a pyramid batch, the device-pointer entry with
its optional outputs absent, and a small grid on scratch a large grid has just used.

Everything is integer or exact f32 work: positions, levels and scores are compared with assert_array_equal, no tolerance.
tests/test_oracle_detect_edges.py proves on the CPU that each scene reaches the branch it is named for."""
import ctypes as C

import numpy as np
import pytest

from android_svo_amd import hip, synth

import detect_reference as dr

pytestmark = pytest.mark.gpu

CASES = dr.cases()


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


def camera_for(pyr_host):
    h, w = pyr_host[0].shape
    return synth.Camera(w, h, 91.5, 88.25, w / 2 - 0.5, h / 2 + 1.25)


def check(ctx, pyr, slot, pyr_host, nl, cell, occ, thr, cam=None):
    """one detection on the device against the reference; returns the number of features"""
    px_r, lvl_r, sc_r = dr.detect(pyr_host, nl, cell, occ, thr)
    px, f, lvl, sc = hip.detect_features(ctx, pyr, slot, cam, n_pyr_levels=nl, cell_size=cell, occupancy=occ,
                                         detection_threshold=thr)
    print("n = %d (reference %d)" % (len(px), len(px_r)))
    np.testing.assert_array_equal(px, px_r.astype(np.float64))
    np.testing.assert_array_equal(lvl, lvl_r)
    np.testing.assert_array_equal(sc.view(np.uint32), sc_r.view(np.uint32))
    if cam is not None:
        np.testing.assert_array_equal(f, synth.cam2world(cam, px_r.astype(np.float64)))  # Feature::f = cam2world(px), phantoms too
    return len(px)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_scene_against_the_reference(ctx, case):
    _, pyr_host, nl, cell, occ, thr = case
    h, w = pyr_host[0].shape
    pyr = hip.Pyramid(ctx, w, h, nl, 1)
    pyr.upload(0, pyr_host)
    try:
        check(ctx, pyr, 0, pyr_host, nl, cell, occ, thr, camera_for(pyr_host))
        check(ctx, pyr, 0, pyr_host, nl, cell, occ, thr, None)
    finally:
        pyr.destroy()


def detect_dev(ctx, pyr, slot, nl, cell, thr):
    """svo_hip_detect_features_dev with score_dev, f_dev and cam all NULL"""
    gc, gr = hip.detect_grid(pyr.width, pyr.height, cell)
    nc = gc * gr
    d_n, d_px, d_lvl = ctx.empty((1,), np.int32), ctx.empty((nc, 2), np.float64), ctx.empty((nc,), np.int32)
    try:
        ctx.check(ctx.lib.svo_hip_detect_features_dev(ctx.h, pyr.h, slot, None, nl, cell, None, C.c_double(thr), C.c_void_p(d_n.ptr),
                                                      C.c_void_p(d_px.ptr), None, C.c_void_p(d_lvl.ptr), None), "detect_features_dev")
        ctx.sync()
        n = int(d_n.download()[0])
        assert 0 <= n <= nc
        return d_px.download()[:n], d_lvl.download()[:n]
    finally:
        for d in (d_n, d_px, d_lvl):
            d.free()


def test_slots_device_entry_and_scratch_reuse(ctx):
    """three scenes in the three slots of one pyramid batch, each detected after all were uploaded; the device-pointer entry
    without its optional outputs; a 6-cell grid right after a 6800-cell grid on the same scratch"""
    scenes = dr.slot_scenes()
    pyr = hip.Pyramid(ctx, 100, 68, 3, 3)
    try:
        for s in (2, 0, 1):
            pyr.upload(s, scenes[s])
        n = []
        for s in (1, 2, 0):
            for cell, thr in dr.SLOT_RUNS:
                n.append(check(ctx, pyr, s, scenes[s], 3, cell, None, thr, camera_for(scenes[s])))
                px_r, lvl_r, _ = dr.detect(scenes[s], 3, cell, None, thr)
                px, lvl = detect_dev(ctx, pyr, s, 3, cell, thr)
                np.testing.assert_array_equal(px, px_r.astype(np.float64))
                np.testing.assert_array_equal(lvl, lvl_r)
        assert len(set(n)) > 3                                                       # the slots do hold different scenes
        for s in (0, 1, 2):
            for cell, thr in dr.SLOT_GRID_SEQUENCE:
                check(ctx, pyr, s, scenes[s], 3, cell, None, thr)
    finally:
        pyr.destroy()


def test_negative_threshold_is_refused(ctx):
    """the per-cell key orders non-negative floats only: a negative threshold is an invalid argument for both entry points,
    nothing is launched, and the context goes on working"""
    lib = ctx.lib
    hf = dr.half_flat_scene()
    pyr = hip.Pyramid(ctx, 100, 68, 3, 1)
    pyr.upload(0, hf)
    try:
        px = np.full((20, 2), -7.0)
        lvl = np.full(20, -7, dtype=np.int32)
        out = C.c_int32(-7)
        for thr in (-1.0, -1e-300, float("-inf")):
            assert lib.svo_hip_detect_features(ctx.h, pyr.h, 0, None, 3, 20, None, C.c_double(thr), C.byref(out),
                                               px.ctypes.data_as(C.c_void_p), None, lvl.ctypes.data_as(C.c_void_p), None) == -1
            assert b"invalid argument" in lib.svo_hip_last_error(ctx.h)
            assert out.value == -7 and (px == -7.0).all() and (lvl == -7).all()      # the outputs are untouched
            with pytest.raises(hip.SvoHipError):
                detect_dev(ctx, pyr, 0, 3, 20, thr)
        assert check(ctx, pyr, 0, hf, 3, 20, None, 10.0) > 5                         # the context is still usable
        assert check(ctx, pyr, 0, hf, 3, 20, None, -0.0) > 5
    finally:
        pyr.destroy()
