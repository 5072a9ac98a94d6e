"""The detector's edge-case scenes on the CPU: tests/detect_reference.py (plain numpy, by the definitions) against the C
restatement in oracle/svo_oracle.c, on every scene, threshold and occupancy that tests/test_gpu_detect_edges.py runs on the
device; and, asserted of the reference alone, that every scene still reaches the branch it was built for."""
import numpy as np
import pytest

from oracle import orc

import detect_reference as dr
from test_oracle_detect import _brute_force_fast

CASES = dr.cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_reference_equals_the_oracle(case):
    _, pyr, nl, cell, occ, thr = case
    px, lvl, sc = dr.detect(pyr, nl, cell, occ, thr)
    px_o, lvl_o, sc_o = orc.detect_features(pyr, n_pyr_levels=nl, cell_size=cell, occupancy=occ, detection_threshold=thr)
    assert len(px) == len(px_o)
    np.testing.assert_array_equal(px, px_o)
    np.testing.assert_array_equal(lvl, lvl_o)
    np.testing.assert_array_equal(sc, sc_o)


def test_reference_equals_the_oracle_on_the_slot_runs():
    n = set()
    for pyr in dr.slot_scenes():
        for cell, thr in dr.SLOT_RUNS + dr.SLOT_GRID_SEQUENCE:
            px, lvl, sc = dr.detect(pyr, 3, cell, None, thr)
            px_o, lvl_o, sc_o = orc.detect_features(pyr, n_pyr_levels=3, cell_size=cell, detection_threshold=thr)
            np.testing.assert_array_equal(px, px_o)
            np.testing.assert_array_equal(lvl, lvl_o)
            np.testing.assert_array_equal(sc, sc_o)
            n.add((len(px), int(px.sum())))
    assert len(n) > 10                                                               # the slots hold different scenes


def test_reference_fast_equals_the_oracle_on_every_level():
    seen = set()
    for name, pyr, nl, _, _, _ in CASES:
        if id(pyr) in seen:
            continue
        seen.add(id(pyr))
        for L in range(nl):
            xs, ys, ss = dr.fast_keypoints(pyr[L])
            xo, yo, so = orc.fast(pyr[L], 10)
            np.testing.assert_array_equal(xs, xo, err_msg=name)
            np.testing.assert_array_equal(ys, yo, err_msg=name)
            np.testing.assert_array_equal(ss, so, err_msg=name)


def test_vectorised_fast_equals_the_pixel_loop():
    """fast_keypoints against the pixel-by-pixel evaluation of the same definition (tests/test_oracle_detect.py)"""
    for img in (dr.tiny_scene()[0], dr.quantised_scene()[0][:24, :32], dr.plateaus_scene()[0][:24, :32], dr.arcs_scene(11, 10)[0][:30, :60]):
        xs, ys, ss = dr.fast_keypoints(img)
        want = _brute_force_fast(img, 10)
        assert [(int(x), int(y), int(s)) for x, y, s in zip(xs, ys, ss)] == [(x, y, int(s)) for x, y, s in want]


def test_reference_shi_tomasi_equals_the_pinned_one(golden):
    g = golden("shitomasi_ref.npz")
    for name in ("scene", "noise"):
        img = g[name + "_img"]
        got = np.array([dr.shi_tomasi(img, int(u), int(v)) for u, v in g[name + "_uv"]], dtype=np.float32)
        np.testing.assert_array_equal(got, g[name + "_score"])


# ---- the scenes reach what they were built for ------------------------------------------------------------------------
@pytest.mark.parametrize("hit,miss", dr.ARC_HIT_MISS)
def test_arcs_scene(hit, miss):
    """all 96 arcs of 9, 10 and 16 pixels are corners with score hit - 1 and are returned at their exact centre, whatever
    the start position and polarity; none of the 32 arcs of 8 pixels is a corner"""
    pyr = dr.arcs_scene(hit, miss)
    assert pyr[0].shape == (107, 213)
    stamps = dr.arc_stamps()
    assert len(stamps) == 128 and len({(s, n, p) for _, _, s, n, p in stamps}) == 128
    if miss:
        d = np.abs(pyr[0].astype(int) - 100)
        assert (d == miss).sum() == sum(16 - n for _, _, _, n, _ in stamps)          # the misses sit exactly at t
    scores = dr.fast_scores(pyr[0])
    xs, ys, ss = dr.fast_keypoints(pyr[0])
    kp = {(int(x), int(y)): int(s) for x, y, s in zip(xs, ys, ss)}
    px, lvl, sc = dr.detect(pyr, 1, dr.ARC_CELL, None, 0.0)
    got = {(int(x), int(y)) for x, y in px}
    n_long = 0
    for cx, cy, start, length, polarity in stamps:
        if length >= 9:
            assert kp.get((cx, cy)) == hit - 1, (start, length, polarity)
            assert (cx, cy) in got, (start, length, polarity)
            n_long += 1
        else:
            assert scores[cy, cx] == 0 and (cx, cy) not in got, (start, length, polarity)
    assert n_long == 96


def test_border_scene():
    """at each edge of the image one of the arcs 3, 4 and 5 px from it is returned and one is dropped, though FAST finds all"""
    pyr = dr.border_scene()
    xs, ys, _ = dr.fast_keypoints(pyr[0])
    kp = {(int(x), int(y)) for x, y in zip(xs, ys)}
    px, _, _ = dr.detect(pyr, 1, dr.ARC_CELL, None, 0.0)
    got = {(int(x), int(y)) for x, y in px}
    for edge in ("left", "right", "top", "bottom"):
        mine = [(cx, cy, d) for cx, cy, e, d in dr.border_stamps() if e == edge]
        assert sorted(d for _, _, d in mine) == [3, 4, 5]
        assert all((cx, cy) in kp for cx, cy, _ in mine)                             # the FAST border rule lets them in
        assert all(dr.shi_tomasi(pyr[0], cx, cy) == 0 for cx, cy, d in mine if d < 5)
        assert any((cx, cy) in got for cx, cy, _ in mine) and any((cx, cy) not in got for cx, cy, _ in mine)


@pytest.mark.parametrize("cell", (40, 20, 25))
def test_ties_scene(cell):
    pyr = dr.ties_scene()
    assert [l.shape for l in pyr] == [(68, 100), (34, 50), (17, 25)]
    ties, cross, first = dr.tie_cells(pyr, 3, cell)
    print("ties scene, cell %d: %d tie cells, %d of them across levels" % (cell, ties, cross))
    assert ties >= 2 and cross >= 2
    px, lvl, sc = dr.detect(pyr, 3, cell, None, 10.0)
    gc, _ = dr.grid(100, 68, cell)
    won = {(int(y) // cell) * gc + int(x) // cell: (int(l), int(x) >> l, int(y) >> l, s) for (x, y), l, s in zip(px, lvl, sc)}
    for k, (L, x, y, st) in first.items():
        assert won[k] == (L, x, y, st)                                               # the first met in (level, row-major) order


def test_plateaus_scene():
    """score 254 occurs, and neighbouring corners with equal scores exist of which neither survives the strict 3x3 test"""
    img = dr.plateaus_scene()[0]
    assert set(np.unique(img)) == {0, 255}
    sc = dr.fast_scores(img)
    assert (sc == 254).any()
    xs, ys, _ = dr.fast_keypoints(img)
    kp = {(int(x), int(y)) for x, y in zip(xs, ys)}
    pairs = 0
    for dy, dx in ((0, 1), (1, 0), (1, 1), (1, -1)):
        a = sc[3:-4, 4:-4]
        b = sc[3 + dy:sc.shape[0] - 4 + dy, 4 + dx:sc.shape[1] - 4 + dx]
        for y, x in zip(*np.nonzero((a > 0) & (a == b))):
            pairs += 1
            assert (x + 4, y + 3) not in kp and (x + 4 + dx, y + 3 + dy) not in kp
    assert pairs >= 10


def test_quantised_scene():
    """differences of exactly 10 (no hit) and 11 (a hit) are everywhere, and corners of the lowest score exist"""
    img = dr.quantised_scene()[0].astype(int)
    assert set(np.unique(img)) == {89, 90, 100, 110, 111}
    d = np.abs(img[:, 1:] - img[:, :-1])
    assert (d == 10).sum() > 500 and (d == 11).sum() > 100
    sc = dr.fast_scores(img.astype(np.uint8))
    assert (sc == 10).sum() > 10
    px, _, _ = dr.detect(dr.quantised_scene(), 3, 20, None, 0.0)
    assert len(px) >= 10


def test_half_flat_scene():
    hf = dr.half_flat_scene()
    n_cells = 20
    base = dr.detect(hf, 3, 20, None, 10.0)
    assert 5 <= len(base[0]) < n_cells                                               # the flat half has no corner
    # phantoms: one per cell without a winner, at (0,0), level 0, score float32(threshold)
    for thr in dr.PHANTOM_THRESHOLDS:
        assert float(np.float32(thr)) > thr
        for occ in (None, np.ones(n_cells, dtype=np.uint8), (np.arange(n_cells) % 3 == 0).astype(np.uint8)):
            px, lvl, sc = dr.detect(hf, 3, 20, occ, thr)
            ph = sc == np.float32(thr)
            n_empty = dr.cells_without_winner(hf, 3, 20, occ, thr)
            assert ph.sum() == n_empty >= 8
            assert (px[ph] == 0).all() and (lvl[ph] == 0).all()
            assert (sc[~ph] > np.float32(thr)).all() and len(px) == n_cells          # every cell yields something
            if occ is not None and occ.all():
                assert ph.all()
    # a threshold that rounds down: none
    assert float(np.float32(0.9)) < 0.9
    px, lvl, sc = dr.detect(hf, 3, 20, None, 0.9)
    assert len(px) == n_cells - dr.cells_without_winner(hf, 3, 20, None, 0.9) and px.any(axis=1).all()
    # strictness at a threshold that is a real score
    s = dr.half_flat_median_score()
    assert (base[2] == s).sum() == 1
    at = dr.detect(hf, 3, 20, None, float(s))
    below = dr.detect(hf, 3, 20, None, float(np.nextafter(s, np.float32(0))))
    assert s not in at[2] and s in below[2] and len(below[0]) == len(at[0]) + 1
    # inf and nan: nothing; -0.0 as 0.0; everything occupied: nothing
    for thr in (float("inf"), float("nan")):
        assert len(dr.detect(hf, 3, 20, None, thr)[0]) == 0
    for a, b in zip(dr.detect(hf, 3, 20, None, -0.0), dr.detect(hf, 3, 20, None, 0.0)):
        np.testing.assert_array_equal(a, b)
    assert len(dr.detect(hf, 3, 20, np.ones(n_cells, dtype=np.uint8), 10.0)[0]) == 0
    assert [c[5] for c in CASES if c[0].startswith("half-flat-") and c[4] is None][:7] == [10.0, 20.0, 0.0, 10.1, 0.1, 1e-3, 0.9]


def test_tiny_scene():
    pyr = dr.tiny_scene()
    assert [l.shape for l in pyr] == [(12, 20), (6, 10), (3, 5)]
    assert len(dr.fast_keypoints(pyr[1])[0]) == 0 and len(dr.fast_keypoints(pyr[2])[0]) == 0
    for cell, n_cells in ((40, 1), (1, 240)):
        px, lvl, sc = dr.detect(pyr, 3, cell, None, 0.0)
        assert len(px) >= 1 and (lvl == 0).all()                                     # a real feature in the smallest image
        px, lvl, sc = dr.detect(pyr, 3, cell, None, 10.1)
        assert len(px) == n_cells                                                    # a feature or a phantom in every cell
