"""The tracker and a tracker group on images the one-launch pyramid kernel does not take: 346x260 (per-level build, scalar
branch) and 352x260 (vector branch).  svo_hip_tracker_track then copies every camera's page-locked image into its slot of the
frame batch (hipMemcpyAsync from level0_mapped + k * mapped_stride) and builds the levels one by one; SparseImgAlign, the
reprojector -- on a 12 x 9 grid whose last column and row are cut, ceil(width / grid_size) -- and the pose refinement run on
pyramids with odd strides.  tests/test_tracker_odd_inputs_cpu.py proves on the CPU that the oracle's chain keeps its matches at
these sizes and that matches fall into the last grid column and row."""
import numpy as np
import pytest

import tracker_odd_cases as toc
import tracking_chain as tc
from test_gpu_tracker_invariance import CFG, _same, _start, _tile_order
from android_svo_amd import hip, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


def _assert_pyramid(pyr, slot, want, what):
    assert (pyr.width, pyr.height) == (want[0].shape[1], want[0].shape[0])
    for l in range(pyr.n_levels):
        assert pyr.download_level(slot, l).tobytes() == want[l].tobytes(), (what, slot, l)


@pytest.mark.parametrize("size", toc.SIZES, ids=toc.size_id)
def test_lone_tracker_against_the_oracle_chain(ctx, size):
    """8 frames, 600 map points, L4-L2: winners and n_matches equal to tc.oracle_track_frame in every frame, poses within
    rot < 1e-4 rad and trans < 1e-3 m, and after every frame last_frame_pyramid() equal to synth.build_pyramid of that frame byte
    for byte at all levels (the copy out of the mapped image plus the per-level build).

    Observed on the MI355X, largest pose difference over the 7 tracked frames: 346x260 2.9e-16 rad 6.0e-16 m (36 matches in the
    last grid column, 25 in the last row), 352x260 9.3e-15 rad 7.2e-16 m (56 and 23)."""
    w, h = size
    seq = toc.sequence(w, h)
    want = toc.oracle_sequence(w, h)
    trk = hip.Tracker(ctx, seq["cam"], **CFG)
    assert (trk.grid_cols, trk.grid_rows) == toc.grid_dims(w, h) == (12, 9)
    _start(trk, seq, tc.sequence_map(seq))
    worst = np.zeros(2)
    n_edge = np.zeros(2, dtype=np.int64)
    for k in range(1, toc.N_FRAMES):
        r, o = trk.track(seq["pyrs"][k][0]), want[k - 1]
        assert r["n_matches"] == o["n_matches"] >= 50, k
        np.testing.assert_array_equal(r["feat_point"], o["feat_point"], err_msg="frame %d" % k)      # the winners, cell by cell
        worst = np.maximum(worst, synth.pose_error(r["T_f_w"], o["T_f_w"]))
        n_edge += toc.edge_matches(w, h, r["feat_px"])
        pyr, slot = trk.last_frame_pyramid()
        assert slot == 0 and pyr.batch == 1 and pyr.n_levels == 5
        _assert_pyramid(pyr, 0, seq["pyrs"][k], k)
    print("tracker %dx%d against the oracle chain: largest pose difference %.3e rad %.3e m, %d matches in the last grid column, %d in the last row" %
          (w, h, worst[0], worst[1], n_edge[0], n_edge[1]))
    assert worst[0] < 1e-4 and worst[1] < 1e-3, worst
    assert (n_edge >= 1).all()
    trk.destroy()


@pytest.mark.parametrize("size", toc.SIZES, ids=toc.size_id)
def test_image_in_the_tracker_buffer_tracks_the_same(ctx, size):
    """frames passed from caller memory and frames written into image_buffer() give bit-equal poses, matches and features (as
    tests/test_gpu_tracker.py::test_image_in_the_tracker_buffer_tracks_the_same at 640x480), here through the copy"""
    seq = toc.sequence(*size)
    mp = tc.sequence_map(seq)
    outs = []
    for through_buffer in (False, True):
        trk = hip.Tracker(ctx, seq["cam"], **CFG)
        _start(trk, seq, mp)
        buf = trk.image_buffer()
        assert buf.shape == (size[1], size[0]) and buf.dtype == np.uint8
        frames = []
        for k in range(1, toc.N_FRAMES):
            if through_buffer:
                buf[:] = seq["pyrs"][k][0]
                r = trk.track(buf)
            else:
                buf[:] = 0                                   # whatever the buffer held is overwritten by the call's own copy
                r = trk.track(seq["pyrs"][k][0])
            frames.append((r["T_f_w"].tobytes(), r["T_f_w_sia"].tobytes(), r["n_matches"], r["feat_px"].tobytes(), r["feat_point"].tobytes()))
        outs.append(frames)
        trk.destroy()
    assert outs[0] == outs[1]
    assert all(f[2] >= 50 for f in outs[0])


@pytest.mark.parametrize("size", toc.SIZES, ids=toc.size_id)
def test_group_of_three_cameras_seeing_different_frames(ctx, size):
    """A TrackerGroup of 3 cameras, every camera two frames ahead of the one before (tests/test_gpu_tracker_frame_pyramid.py):
    each camera's result equals a lone tracker's over the same frames, field by field and bit for bit
    (tests/test_gpu_tracker_invariance.py's comparison, SIA_REDUCTION_TILE_ORDER on both), and each camera's slot of the
    borrowed frame batch holds its own frame's pyramid -- the k * mapped_stride of the copy."""
    seq = toc.sequence(*size)
    mp = tc.sequence_map(seq)
    want = []
    for c in range(toc.N_CAMS):
        trk = hip.Tracker(ctx, seq["cam"], **CFG)
        _tile_order(trk)
        _start(trk, seq, mp)
        want.append([trk.track(seq["pyrs"][toc.group_frames(k)[c]][0]) for k in toc.GROUP_STEPS])
        trk.destroy()
    assert all(r["n_matches"] >= 50 for rs in want for r in rs)
    grp = hip.TrackerGroup(ctx, seq["cam"], toc.N_CAMS, **CFG)
    _tile_order(grp)
    for t in grp.cameras:
        _start(t, seq, mp)
    for i, k in enumerate(toc.GROUP_STEPS):
        frames = toc.group_frames(k)
        grp.track([seq["pyrs"][f][0] for f in frames])
        views = [t.last_frame_pyramid() for t in grp.cameras]
        assert [s for _, s in views] == list(range(toc.N_CAMS))
        assert len({p.h.value for p, _ in views}) == 1 and views[0][0].batch == toc.N_CAMS      # one batch for the group
        for c, f in enumerate(frames):
            _same(grp.cameras[c].last_result(), want[c][i], (size, k, c))
            _assert_pyramid(views[0][0], c, seq["pyrs"][f], (k, c))
    grp.destroy()
