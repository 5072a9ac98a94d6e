"""What the camera-rig GPU tests rest on, established with the CPU oracle alone: the inputs of tests/rig_case.py can tell a wrong
camera model from the right one.  For every ordered pair of rig cameras c != d and every batch of camera c, the oracle's
update_seeds pass with camera d's MODEL (same images, poses and seeds) differs from the pass with camera c's own in the status
or in the bits of mu of at least three seeds -- the project's bar for "a wrong rule shows".  So a device pass that handed a job
another camera's intrinsics, distortion or pixel error angle could not go unnoticed in a byte comparison.  A condition on the
committed scene seeds of rig_case.py, not on any device code.  Likewise for the tracked sequences: the oracle's tracking step of
a camera's first frame with another camera's model gives another pose or another match count."""
import numpy as np
import pytest

import rig_case as rc
import tracking_chain as tc


@pytest.mark.parametrize("name", [a.name for a in rc.ARRANGEMENTS])
def test_another_cameras_model_changes_three_seeds_of_every_batch(name):
    arr = rc.BY_NAME[name]
    own = rc.oracle_first_pass(name)
    n_checked = 0
    for c, mk in enumerate(rc.cameras(arr)):
        for other in rc.NAMES:
            if other == arr.order[c]:
                continue
            wrong_cam = rc.camera(other, rc.WIDTH, rc.HEIGHT)
            for k, sc in enumerate(mk.keyframes):
                wrong = rc.oracle_pass(wrong_cam, sc, mk.cur_pyr, mk.T_cur_w)
                changed = int(((wrong["status"] != own[c][k]["status"]) | (wrong["mu"].view(np.uint32) != own[c][k]["mu"].view(np.uint32))).sum())
                print("%s: camera %s batch %d (%d seeds) with the model of %s: %d seeds change" % (name, arr.order[c], k, len(sc.px), other, changed))
                assert changed >= 3, (name, arr.order[c], k, other, changed)
                n_checked += 1
    assert n_checked == 2 * sum(len(z) for z in arr.sizes)


def test_own_model_updates_seeds():
    """the right model is not just another wrong one: with its own camera every batch of three or more seeds updates some"""
    for arr in rc.ARRANGEMENTS:
        for c, cam in enumerate(rc.oracle_first_pass(arr.name)):
            for k, o in enumerate(cam):
                assert int((o["status"] >= 3).sum()) >= min(3, len(o["status"]) // 4), (arr.name, c, k)


def test_the_cameras_and_arrangements_are_what_the_gpu_tests_promise():
    a, b, c = (rc.camera(n, 640, 480) for n in rc.NAMES)
    assert (a.fx, a.fy, a.cx, a.cy) == (500.0, 500.0, 319.5, 239.5) and getattr(a, "dist", None) is None
    assert (b.fx, b.fy, b.cx, b.cy) == (430.0, 445.0, 305.25, 252.25) and getattr(b, "dist", None) is None
    assert (c.fx, c.fy, c.cx, c.cy) == (560.0, 540.0, 333.5, 229.0) and c.dist == (-0.12, 0.03, 2e-4, -1e-4, 0.0)
    by = rc.BY_NAME
    assert dict(zip(by["sizes_around_a_block"].order, by["sizes_around_a_block"].sizes)) == {"A": (255, 256, 257), "B": (300,), "C": (64, 31)}
    assert by["sizes_around_a_block_reversed_slots"].reversed_slots and by["sizes_around_a_block_reversed_slots"].sizes == by["sizes_around_a_block"].sizes
    assert list(zip(by["two_cameras_sit_out"].order, by["two_cameras_sit_out"].sizes)) == [("B", ()), ("C", (150, 100)), ("A", ())]
    assert (by["one_camera"].order, by["one_camera"].sizes) == (("C",), ((300,),))


def _oracle_first_frame(seq, cam):
    """tc.oracle_track_frame of the sequence's frame 1 from keyframe 0, the tracker holding camera model `cam`"""
    from oracle import orc
    mp = dict(tc.sequence_map(seq), cam=cam)
    n = len(seq["px0"])
    state = {"pt_type": mp["pt_type"].copy(), "pt_n_failed": mp["pt_n_failed"].copy(), "pt_n_succeeded": mp["pt_n_succeeded"].copy(),
             "unlinked": np.zeros(n, np.uint8)}
    last = dict(T=seq["T0"].copy(), px=seq["px0"].copy(), f=seq["f0"].copy(), point=np.arange(n, dtype=np.int32))
    return tc.oracle_track_frame(orc, mp, state, last, seq["pyrs"][0], seq["pyrs"][1], 2)


@pytest.mark.parametrize("name", rc.NAMES)
def test_another_cameras_model_changes_the_tracked_frame(name):
    seq = rc.sequence(name)
    own = _oracle_first_frame(seq, seq["cam"])
    assert own["n_matches"] >= 50 and (own["feat_point"] >= 0).sum() >= 20        # the camera tracks its own sequence
    for other in rc.NAMES:
        if other == name:
            continue
        wrong = _oracle_first_frame(seq, rc.camera(other, rc.TRACK_WIDTH, rc.TRACK_HEIGHT))
        print("camera %s with the model of %s: %d matches (own %d)" % (name, other, wrong["n_matches"], own["n_matches"]))
        assert wrong["T_f_w"].tobytes() != own["T_f_w"].tobytes() or wrong["n_matches"] != own["n_matches"], (name, other)
