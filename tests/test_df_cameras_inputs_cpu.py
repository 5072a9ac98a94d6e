"""What tests/test_gpu_seed_cameras.py rests on, established with the CPU oracle alone (oracle/orc.py:update_seeds): the cameras
of every arrangement differ enough.  For every ordered pair of cameras c != d, camera c's batches passed against camera d's
current image and pose end with another status for at least one seed in ten of EVERY batch (counted among the seeds the GPU
test does not erase by hand) -- so a pass that picked the wrong current slot, or the wrong camera's pose, could not go
unnoticed in a comparison of statuses.  A condition on the committed seeds of df_cameras_case.py, not on any device code."""
import numpy as np
import pytest

import df_cameras_case as dc


def kept(arr, c, k, n):
    keep = np.ones(n, bool)
    if arr.erase_seventh:
        keep[np.arange(5, n, 7)] = False
    return keep


@pytest.mark.parametrize("name", [a.name for a in dc.ARRANGEMENTS])
def test_another_cameras_frame_changes_a_tenth_of_every_batch(name):
    arr = dc.BY_NAME[name]
    cams = dc.cameras(arr)
    own = dc.oracle_first_pass(name)
    n_checked = 0
    for c, mk in enumerate(cams):
        for d, other in enumerate(cams):
            if d == c:
                continue
            for k, sc in enumerate(mk.keyframes):
                wrong = dc.oracle_pass(mk.cam, sc, other.cur_pyr, other.T_cur_w)
                keep = kept(arr, c, k, len(sc.px))
                changed = int((wrong["status"] != own[c][k]["status"])[keep].sum())
                print("%s: camera %d batch %d (%d seeds) against camera %d: %d statuses change" % (name, c, k, len(sc.px), d, changed))
                assert 10 * changed >= len(sc.px), (name, c, k, d, changed, len(sc.px))
                n_checked += 1
    if len(cams) > 1:
        assert n_checked == (len(cams) - 1) * sum(len(mk.keyframes) for mk in cams)


def test_the_arrangements_cover_what_the_gpu_test_promises():
    by = dc.BY_NAME
    assert sorted({len(a.sizes) for a in dc.ARRANGEMENTS} & {1, 2, 3, 9}) == [1, 2, 3, 9]
    assert by["three_cameras_0_2_0"].sizes == ((), (150, 100), ())
    assert sum(len(s) for s in by["nine_cameras_two_batches"].sizes) == 18
    s70 = [n for cam in by["seventy_small_jobs"].sizes for n in cam]
    assert len(s70) == 70 and min(s70) == 1 and max(s70) == 40
    assert sorted(n for cam in by["sizes_around_a_block"].sizes for n in cam) == [1, 255, 256, 257, 700]
    assert by["one_batch_of_4097"].sizes[0] == (4097,)
    assert all(len(set(a.seeds)) == len(a.seeds) == len(a.sizes) for a in dc.ARRANGEMENTS)      # every camera its own scene
