"""svo_hip_tracker_set_sia_option(SVO_HIP_SIA_OPT_REDUCTION, SVO_HIP_SIA_REDUCTION_TILE_ORDER): a camera of a group equals its
lone tracker whatever the other cameras of the group hold.  In the default mode that holds only while the group's largest last
frame puts the SparseImgAlign kernel into the shape the lone tracker gets
(tests/test_gpu_tracker_group.py::test_a_camera_whose_first_frame_falls_into_another_shape_class asserts a tolerance there);
with the mode set on the lone tracker and on the group it is equality, frame after frame, of every field of
svo_hip_track_result and of the frame's features and the map's counters."""
import ctypes as C

import numpy as np
import pytest

import tracking_chain as tc
from android_svo_amd import hip

pytestmark = pytest.mark.gpu

CFG = dict(max_keyframes=4, max_points=1024, max_obs=4096, max_kf_features=2048, max_candidates=16, max_items=1024,
           max_frame_features=1024, grid_size=tc.CELL, max_fts=tc.MAX_FTS, klt_min_level=2)
KEYS = ("T_f_w", "T_f_w_sia", "feat_px", "feat_f", "feat_level", "feat_point", "feat_type", "feat_grad", "type", "n_failed", "n_succeeded")


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def seqs():
    return {n: tc.make_sequence(n_frames=9, n_map=n) for n in (150, 420, 600)}


def _start(trk, seq, mp):
    n = len(seq["px0"])
    trk.upload_keyframe(0, seq["pyrs"][0][0])
    trk.set_map(mp)
    trk.set_last_frame(seq["T0"], seq["px0"], seq["f0"], np.arange(n, dtype=np.int32), kf_slot=0)


def _fields(st):
    """every field of a ctypes structure as bytes, nested structures field by field (padding is not a field, nor is the member
    the header declares as padding and nobody writes)"""
    out = []
    for name, _ in st._fields_:
        if name == "pad_":
            continue
        v = getattr(st, name)
        out.append((name, _fields(v) if isinstance(v, C.Structure) else bytes(v) if isinstance(v, C.Array) else repr(v).encode()
                    if not isinstance(v, float) else np.float64(v).tobytes()))
    return out


def _same(a, b, what):
    for (name, x), (_, y) in zip(_fields(a["result"]), _fields(b["result"])):
        assert x == y, (what, "svo_hip_track_result." + name)
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)
    assert a["n_matches"] == b["n_matches"] and a["n_trials"] == b["n_trials"] and a["map_changed"] == b["map_changed"], what
    assert list(a["overlap_kf"]) == list(b["overlap_kf"]) and list(a["overlap_count"]) == list(b["overlap_count"]), what


def _tile_order(obj):
    obj.set_sia_option(hip.SIA_OPT_REDUCTION, hip.SIA_REDUCTION_TILE_ORDER)


def test_a_camera_in_another_shape_class_equals_its_lone_tracker(ctx, seqs):
    """600 beside 420 map points (10 against 7 tiles on the first frame), frames 1 to 4: no tolerance"""
    seq_a, seq_b = seqs[600], seqs[420]
    mp_a, mp_b = tc.sequence_map(seq_a), tc.sequence_map(seq_b)
    trk = hip.Tracker(ctx, seq_b["cam"], **CFG)
    _tile_order(trk)
    _start(trk, seq_b, mp_b)
    want = [trk.track(seq_b["pyrs"][k][0]) for k in range(1, 5)]
    trk.destroy()
    grp = hip.TrackerGroup(ctx, seq_a["cam"], 2, **CFG)
    _tile_order(grp.cameras[1])                      # one camera's handle: the solver is the group's
    _start(grp.cameras[0], seq_a, mp_a)
    _start(grp.cameras[1], seq_b, mp_b)
    for k in range(1, 5):
        grp.track([seq_a["pyrs"][k][0], seq_b["pyrs"][k][0]])
        _same(grp.cameras[1].last_result(), want[k - 1], k)
    grp.destroy()


def test_three_cameras_of_three_sizes_one_of_them_promoting_a_keyframe(ctx, seqs):
    sizes = (150, 420, 600)
    promoting = 1                                    # camera 1 turns its fifth frame into keyframe 1 and goes on with a two-keyframe map
    maps = {n: tc.sequence_map(seqs[n]) for n in sizes}

    def lone(n, promote):
        seq = seqs[n]
        trk = hip.Tracker(ctx, seq["cam"], **CFG)
        _tile_order(trk)
        _start(trk, seq, maps[n])
        rs = [trk.track(seq["pyrs"][k][0]) for k in range(1, 6)]
        if promote:
            trk.keyframe_from_last_frame(1)
            trk.set_map(tc.map_with_tracked_frame_as_keyframe(seq, maps[n], rs[-1]))
        rs += [trk.track(seq["pyrs"][k][0]) for k in range(6, 9)]
        trk.destroy()
        return rs
    want = [lone(n, c == promoting) for c, n in enumerate(sizes)]
    grp = hip.TrackerGroup(ctx, seqs[sizes[0]]["cam"], len(sizes), **CFG)
    _tile_order(grp)
    for t, n in zip(grp.cameras, sizes):
        _start(t, seqs[n], maps[n])
    got = [[] for _ in sizes]
    for k in range(1, 9):
        if k == 6:
            t, n = grp.cameras[promoting], sizes[promoting]
            t.keyframe_from_last_frame(1)
            t.set_map(tc.map_with_tracked_frame_as_keyframe(seqs[n], maps[n], got[promoting][-1]))
        grp.track([seqs[n]["pyrs"][k][0] for n in sizes])
        for c in range(len(sizes)):
            got[c].append(grp.cameras[c].last_result())
    for c in range(len(sizes)):
        for i, (a, b) in enumerate(zip(got[c], want[c])):
            _same(a, b, (sizes[c], i))
    assert any(1 in list(r["overlap_kf"]) for r in got[promoting][5:])          # the new keyframe took part
    grp.destroy()


def test_only_the_reduction_option_can_be_set_on_a_tracker(ctx, seqs):
    trk = hip.Tracker(ctx, seqs[150]["cam"], **CFG)
    with pytest.raises(hip.SvoHipError, match=r"\(-1\)"):
        trk.set_sia_option(hip.SIA_OPT_ARITH, hip.SIA_ARITH_FAST)
    with pytest.raises(hip.SvoHipError, match=r"\(-1\)"):
        trk.set_sia_option(hip.SIA_OPT_REDUCTION, 2)
    trk.set_sia_option(hip.SIA_OPT_REDUCTION, hip.SIA_REDUCTION_PER_WAVE)
    trk.destroy()
