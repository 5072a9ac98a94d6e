"""The model of tests/seed_init_reference.py on the oracle alone (no device): what tests/test_gpu_keyframe_seeds.py rests on.

The case: seedsynth.make_seed_case(n_seeds=64, seed=3) at two image sizes; seeds detected on its reference pyramid (3 levels,
threshold 10.0), constructed with (1.1, 0.5) x the median true depth, one updateSeeds pass ref -> cur, the case's own 64
pixels as the keyframe's existing features.  The conditions below make the GPU comparison meaningful: the seed marks and the
feature marks each change what the detector finds, they overlap, and seeds without a match -- whose px_cur must not be
looked at -- are present."""
import numpy as np
import pytest

import seed_init_reference as si
from android_svo_amd import seedsynth, synth
from oracle import orc

CASES = [(640, 480, 30), (346, 260, 20)]


def model_case(width, height, cell):
    sc = seedsynth.make_seed_case(n_seeds=64, seed=3, width=width, height=height)
    px, level, _ = orc.detect_features(sc.ref_pyr, n_pyr_levels=3, cell_size=cell, detection_threshold=10.0)
    px = px.astype(np.float64)
    f = synth.cam2world(sc.cam, px)
    zbar = float(np.median(sc.true_depth))
    a, b, mu, zr, s2 = seedsynth.seed_ctor(1.1 * zbar, 0.5 * zbar, len(px))
    out = orc.update_seeds(sc.cam, sc.ref_pyr, sc.cur_pyr, sc.T_ref_w, sc.T_cur_w, px, f, level, a, b, mu, zr, s2)
    return dict(sc=sc, cell=cell, px=px, f=f, level=level, zbar=zbar, state=(a, b, mu, zr, s2), status=out["status"],
                px_cur=out["px_cur"])


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "%dx%d_c%d" % c)
def case(request):
    return model_case(*request.param)


def test_marks_change_the_detection_and_unmatched_seeds_are_present(case):
    sc, cell = case["sc"], case["cell"]
    cols, rows = si.grid_dims(sc.cam.width, sc.cam.height, cell)
    seeds = si.mark_updated(np.zeros((rows, cols), np.uint8), case["status"], case["px_cur"], cell)
    feats = si.mark_px(np.zeros((rows, cols), np.uint8), sc.px, cell)
    n_seed_cells, n_both = int(seeds.sum()), int((seeds & feats).sum())
    free = si.keyframe_sequence(sc.cam, sc.cur_pyr, cell, 3, 10.0, 1.1 * case["zbar"], 0.5 * case["zbar"])
    only = si.keyframe_sequence(sc.cam, sc.cur_pyr, cell, 3, 10.0, 1.1 * case["zbar"], 0.5 * case["zbar"], existing_px=sc.px)
    full = si.keyframe_sequence(sc.cam, sc.cur_pyr, cell, 3, 10.0, 1.1 * case["zbar"], 0.5 * case["zbar"],
                                seed_passes=[(case["status"], case["px_cur"])], existing_px=sc.px)
    n = [len(free["px"]), len(only["px"]), len(full["px"])]
    no_match = case["status"] == si.SEED_NO_MATCH
    n_bad = int((no_match & ~np.isfinite(case["px_cur"]).all(axis=1)).sum())
    print("seed-marked cells %d, marked by both %d, detections free / features only / full grid %s, NO_MATCH with a "
          "non-finite px_cur %d" % (n_seed_cells, n_both, n, n_bad))
    assert n_seed_cells >= 50
    assert n_both >= 10
    assert n[0] > n[1] > n[2]
    assert n[2] >= 30
    assert n_bad >= 2
    assert np.array_equal(full["grid"], seeds | feats)
    # no new feature in an occupied cell, and the constructor state of n seeds
    k = (full["px"][:, 1] // cell).astype(int) * cols + (full["px"][:, 0] // cell).astype(int)
    assert not full["grid"].reshape(-1)[k].any()
    assert all(len(full[key]) == n[2] for key in ("a", "b", "mu", "z_range", "sigma2"))


@pytest.mark.parametrize("cell,cols,rows", [(30, 22, 16), (20, 18, 13), (7, 1, 1)])
def test_truncation_rule_and_defined_behaviour(cell, cols, rows):
    c, W = float(cell), float(cell * cols)
    n_cells = cols * rows
    cell_of = lambda u, v: si.cell_of(u, v, cell, cols, rows)
    assert cell_of(0.0, 0.0) == 0 and cell_of(c - 1e-9, c - 1e-9) == 0
    # truncation towards zero: (-cell, 0) belongs to column / row 0
    assert cell_of(-0.5, 0.5) == 0 and cell_of(0.5, -0.5) == 0 and cell_of(-(c - 1e-9), 0.0) == 0
    # exactly on a boundary: the next cell
    assert cell_of(c, 0.0) == (1 if n_cells > 1 else None)
    assert cell_of(0.0, c) == (cols if rows > 1 else None)
    # column -1 is the previous row's last cell while the flat index is valid, as in the reference
    assert cell_of(-c, c) == (cols - 1 if rows > 1 else (0 if cols == 1 else None))
    assert cell_of(-c, 0.0) is None and cell_of(0.0, -c) is None
    # beyond the width with a valid flat index: the next row's cell
    assert cell_of(W, 0.0) == (cols if rows > 1 else None)
    assert cell_of(W, c * (rows - 1)) is None and cell_of(0.0, c * rows) is None
    assert cell_of(0.0, c * rows - 1e-9) == cols * (rows - 1)
    # undefined in the reference, nothing here
    for bad in (np.nan, np.inf, -np.inf, 1e300, -1e300, c * 2147483648.0, -c * 2147483649.0):
        assert cell_of(bad, 1.0) is None and cell_of(1.0, bad) is None
    assert cell_of(c * 2147483647.0, 0.0) is None                  # a valid int, an index outside the grid
    # the edge list the GPU test uses marks something and skips something
    edge = si.edge_pixels(cell, cols, rows)
    hit = [si.cell_of(u, v, cell, cols, rows) is not None for u, v in edge]
    assert any(hit) and not all(hit)


def test_marking_is_idempotent_and_only_adds():
    rng = np.random.default_rng(5)
    cell, cols, rows = 20, 18, 13
    px = np.concatenate([si.edge_pixels(cell, cols, rows), rng.uniform(-40, 400, (500, 2))])
    once = si.mark_px(np.zeros((rows, cols), np.uint8), px, cell)
    twice = si.mark_px(once.copy(), px, cell)
    assert np.array_equal(once, twice) and set(np.unique(once)) == {0, 1}
    pre = (rng.uniform(size=(rows, cols)) < 0.3).astype(np.uint8)
    got = si.mark_px(pre.copy(), px, cell)
    assert np.array_equal(got, pre | once)
    # mark_updated looks at the status alone
    status = rng.integers(-1, 6, len(px)).astype(np.int32)
    want = si.mark_px(np.zeros((rows, cols), np.uint8), px[status >= si.SEED_UPDATED], cell)
    assert np.array_equal(si.mark_updated(np.zeros((rows, cols), np.uint8), status, px, cell), want)
    assert np.array_equal(si.mark_px(np.zeros((rows, cols), np.uint8), np.zeros((0, 2)), cell), np.zeros((rows, cols), np.uint8))
