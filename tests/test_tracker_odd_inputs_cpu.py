"""What tests/test_gpu_tracker_odd_sizes.py rests on, with the CPU oracle alone: at 346x260, 352x260, 344x260 and 346x261 the
oracle's tracking chain keeps at least 50 matches in every frame on a 12 x 9 grid whose last column and row are cut, matches
do fall into that column and into that row, and the frames the cameras of the group test see (each camera two frames ahead of the one
before, straight from keyframe 0) are tracked too.  The two device sizes are not tiled: the tracker's frames go through the copy
from the page-locked image and the per-level build."""
import numpy as np
import pytest

import pyramid_size_cases as ps
import tracker_odd_cases as toc
import tracking_chain as tc


def test_default_sequence_is_unchanged_by_the_new_keywords():
    a = tc.make_sequence(n_frames=2, n_map=50)
    b = tc.make_sequence(n_frames=2, n_map=50, width=640, height=480, focal=None, border=48)
    assert (a["cam"].width, a["cam"].height, a["cam"].fx, a["cam"].fy, a["cam"].cx, a["cam"].cy) == (640, 480, 500.0, 500.0, 319.5, 239.5)
    for k in ("px0", "f0", "pos", "T0"):
        assert a[k].tobytes() == b[k].tobytes()
    assert all(x[0].tobytes() == y[0].tobytes() for x, y in zip(a["pyrs"], b["pyrs"]))
    c = tc.make_sequence(n_frames=1, n_map=50, width=346, height=260, focal=300.0)
    assert (c["cam"].width, c["cam"].height, c["cam"].fx, c["cam"].fy) == (346, 260, 300.0, 300.0) and c["pyrs"][0][0].shape == (260, 346)


def test_the_device_sizes_take_the_copy_and_the_per_level_build():
    assert ps.level_paths(346, 260, 5) == ("scalar",) * 4
    assert ps.level_paths(352, 260, 5) == ("vector", "vector", "vector", "scalar")
    for w, h in toc.SIZES:
        assert not ps.tiled(w, h, 5)
        assert toc.grid_dims(w, h) == (12, 9) and w % tc.CELL != 0 and h % tc.CELL != 0      # a partial last column and row


@pytest.mark.parametrize("size", toc.CPU_SIZES, ids=toc.size_id)
def test_oracle_chain_keeps_its_matches_and_reaches_the_last_cells(size):
    w, h = size
    res = toc.oracle_sequence(w, h)
    assert len(res) == toc.N_FRAMES - 1
    n_matches = [int(r["n_matches"]) for r in res]
    edge = np.array([toc.edge_matches(w, h, r["feat_px"]) for r in res])
    print("%dx%d: matches %s, in the last column %d, in the last row %d" % (w, h, n_matches, edge[:, 0].sum(), edge[:, 1].sum()))
    assert min(n_matches) >= 50                                                  # Config::qualityMinFts()
    assert all((r["feat_point"] >= 0).sum() >= 20 for r in res)
    assert edge[:, 0].sum() >= 1 and edge[:, 1].sum() >= 1                          # the cut last column AND the cut last row
    assert toc.grid_dims(w, h) == (12, 9)


@pytest.mark.parametrize("size", toc.SIZES, ids=toc.size_id)
def test_the_group_cameras_frames_are_tracked_on_the_oracle(size):
    seq = toc.sequence(*size)
    for c in range(toc.N_CAMS):
        frames = [toc.group_frames(k)[c] for k in toc.GROUP_STEPS]
        assert max(frames) < toc.N_FRAMES
        res = toc.oracle_chain(seq, frames)
        assert min(int(r["n_matches"]) for r in res) >= 50, (c, [int(r["n_matches"]) for r in res])
    assert len({tuple(toc.group_frames(k)) for k in toc.GROUP_STEPS}) == len(toc.GROUP_STEPS)
    assert all(len(set(toc.group_frames(k))) == toc.N_CAMS for k in toc.GROUP_STEPS)      # the cameras see different frames
