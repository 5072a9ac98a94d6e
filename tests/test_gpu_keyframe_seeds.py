"""A new keyframe's seeds are detected and created on the device: the device detector grid (svo_hip_grid_mark_px[_dev],
svo_hip_seed_batch_mark_updated, svo_hip_tracker_mark_last_frame) and svo_hip_seed_batch_create_detected, against the numpy
model of tests/seed_init_reference.py (tests/test_seed_init_model.py establishes the model's own properties on the CPU),
against svo_hip_detect_features / svo_hip_seed_batch_create, and against batches that run with report_updated = 1.
Every comparison is exact.  Every grid sits between two 64-byte guards that must come back unchanged."""
import ctypes as C
import functools

import numpy as np
import pytest

import map_growth_reference as mg
import map_growth_scenario as sc
import seed_init_reference as si
import tracking_chain as tc
from test_gpu_map_growth import _frames, _same, _start
from test_gpu_map_removal import CFG
from test_seed_init_model import CASES, model_case
from android_svo_amd import hip, seedsynth, synth

pytestmark = pytest.mark.gpu

GUARD = 64


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


class GuardedGrid:
    """a DetectorGrid inside a larger allocation: [64 guard bytes][rows * cols][64 guard bytes]"""

    def __init__(self, ctx, width, height, cell, pre=None):
        cols, rows = hip.detect_grid(width, height, cell)
        self.nc = cols * rows
        self.guard = ((np.arange(GUARD) * 37 + 11) % 251 + 2).astype(np.uint8)            # (never 0 or 1)
        init = np.zeros(self.nc, np.uint8) if pre is None else np.asarray(pre, np.uint8).reshape(-1)
        self.buf = ctx.to_device(np.concatenate([self.guard, init, self.guard]))
        self.grid = hip.DetectorGrid(ctx, width, height, cell, ptr=self.buf.ptr + GUARD)

    def read(self):
        raw = self.buf.download()
        assert np.array_equal(raw[:GUARD], self.guard) and np.array_equal(raw[GUARD + self.nc:], self.guard), "guard bytes written"
        return raw[GUARD:GUARD + self.nc].reshape(self.grid.rows, self.grid.cols)

    def free(self):
        self.buf.free()


def _pyramid(ctx, levels, n_levels=5):
    h, w = levels[0].shape
    p = hip.Pyramid(ctx, w, h, n_levels, 1)
    p.upload(0, levels[:n_levels])
    return p


# ---- 1. marking pixels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["dev", "host"])
@pytest.mark.parametrize("width,height,cell", [(640, 480, 30), (346, 260, 20), (7, 7, 7)])
def test_mark_px_equals_the_model(ctx, width, height, cell, form):
    cols, rows = hip.detect_grid(width, height, cell)
    assert (cols, rows) == {30: (22, 16), 20: (18, 13), 7: (1, 1)}[cell]
    rng = np.random.default_rng(cell)
    rand = np.stack([rng.uniform(-2 * cell, width + 2 * cell, 10000), rng.uniform(-2 * cell, height + 2 * cell, 10000)], axis=1)
    rand[::3] = np.floor(rand[::3])                                                        # FAST corners are integers
    edge = si.edge_pixels(cell, cols, rows)
    inside = np.stack([rng.uniform(0, width, 65), rng.uniform(0, height, 65)], axis=1)

    def run(px, pre=None):
        g = GuardedGrid(ctx, width, height, cell, pre)
        if form == "dev":
            d = ctx.to_device(np.ascontiguousarray(px).reshape(-1, 2)) if len(px) else hip.DeviceView(ctx, 0, (0, 2), np.float64)
            g.grid.mark_px(d)
            got = g.read()
            if len(px):
                d.free()
        else:
            g.grid.mark_px(px)
            got = g.read()
        g.free()
        want = si.mark_px(np.zeros((rows, cols), np.uint8) if pre is None else np.asarray(pre, np.uint8).reshape(rows, cols).copy(), px, cell)
        assert np.array_equal(got, want), (len(px), np.argwhere(got != want)[:5])
        return got
    for n in (0, 1, 64, 65):
        got = run(inside[:n])
        assert got.sum() == len({si.cell_of(u, v, cell, cols, rows) for u, v in inside[:n]})
    run(edge)
    whole = np.concatenate([edge, rand])                  # more pixels than one launch has threads: the grid-stride loop wraps
    assert len(whole) > 32 * 256
    got = run(whole)
    assert got.sum() >= min(cols * rows, 50) and set(np.unique(got)) <= {0, 1}
    # a pre-set grid is only ever added to
    pre = (rng.uniform(size=rows * cols) < 0.3).astype(np.uint8)
    few = rand[:40]
    got = run(few, pre)
    assert np.array_equal(got, pre.reshape(rows, cols) | si.mark_px(np.zeros((rows, cols), np.uint8), few, cell))


def test_mark_px_refusals(ctx):
    g = GuardedGrid(ctx, 640, 480, 30)
    px = np.zeros((4, 2))
    lib, P = ctx.lib, C.c_void_p
    for fn in (lib.svo_hip_grid_mark_px, lib.svo_hip_grid_mark_px_dev):
        assert fn(ctx.h, 4, P(g.buf.ptr) if fn is lib.svo_hip_grid_mark_px_dev else px.ctypes.data_as(P), 30, 22, 16, None) == -1
        assert fn(ctx.h, -1, None, 30, 22, 16, P(g.grid.ptr)) == -1
        assert fn(ctx.h, 4, None, 30, 22, 16, P(g.grid.ptr)) == -1
        for dims in ((0, 22, 16), (30, 0, 16), (30, 22, 0), (-30, 22, 16)):
            assert fn(ctx.h, 0, None, *dims, P(g.grid.ptr)) == -1
        assert fn(None, 0, None, 30, 22, 16, P(g.grid.ptr)) == -1
        assert fn(ctx.h, 0, None, 30, 22, 16, P(g.grid.ptr)) == 0
    assert not g.read().any()
    g.free()


# ---- 2. marking the seeds a pass updated ---------------------------------------------------------------------------------
def _seed_case(ctx, n, width, height):
    s = seedsynth.make_seed_case(n_seeds=n, seed=21, width=width, height=height)
    s2 = (s.sigma2 * np.float32(0.0045)).astype(np.float32)
    return s, _pyramid(ctx, s.ref_pyr), _pyramid(ctx, s.cur_pyr), s2


@pytest.mark.parametrize("n,width,height,cell", [(1500, 640, 480, 30), (600, 346, 260, 20)])
def test_mark_updated_equals_the_events_of_a_reporting_twin(ctx, n, width, height, cell):
    """Three passes; the pass and the marking both enqueued before the collect.  After every pass the grid is the model over the
    px_cur of the events of a twin batch run with report_updated = 1.  Before pass 1 every seed that marked one of a chosen
    set of cells is erased: what marked them is gone, and the stale px_cur of an erased seed marks nothing."""
    s, kf, cf, s2 = _seed_case(ctx, n, width, height)
    cols, rows = hip.detect_grid(width, height, cell)
    make = lambda: hip.ResidentSeeds(ctx, s.px, s.f, s.level, s.a, s.b, s.mu, s.z_range, s2)
    rs, twin = make(), make()
    chosen, n_conv = None, []
    for frame in range(3):
        g = GuardedGrid(ctx, width, height, cell)
        rs.update_async(kf, 0, cf, 0, s.cam, s.T_ref_w, s.T_cur_w, report_updated=False)
        g.grid.mark_updated([rs])
        ev, counts = rs.collect()
        got = g.read()
        tev, tcounts = twin.update(kf, 0, cf, 0, s.cam, s.T_ref_w, s.T_cur_w, report_updated=True)
        assert np.array_equal(counts, tcounts) and (tev["status"] >= hip.SEED_UPDATED).all()
        assert ev.tobytes() == tev[tev["status"] != hip.SEED_UPDATED].tobytes()            # the quiet pass reports convergence / NaN as ever
        want = si.mark_px(np.zeros((rows, cols), np.uint8), tev["px_cur"], cell)
        assert np.array_equal(got, want), (frame, np.argwhere(got != want)[:5])
        # legal after the collect too, until the next update: the same marks
        g2 = GuardedGrid(ctx, width, height, cell)
        g2.grid.mark_updated([rs])
        assert np.array_equal(g2.read(), want)
        g2.free()
        n_conv.append(int(counts[hip.SEED_CONVERGED + 1]))
        print("pass %d: status counts %s, cells marked %d" % (frame, list(counts), int(want.sum())))
        if frame == 0:
            assert counts[hip.SEED_UPDATED + 1] + counts[hip.SEED_CONVERGED + 1] >= n // 2 and counts[hip.SEED_NO_MATCH + 1] >= 1
            marked = np.flatnonzero(want.reshape(-1))
            chosen = marked[::max(1, len(marked) // 40)][:40]
            k = np.array([-1 if c is None else c for c in (si.cell_of(u, v, cell, cols, rows) for u, v in tev["px_cur"])])
            gone = tev["index"][np.isin(k, chosen)]
            assert len(gone) >= len(chosen)
            rs.erase(gone)
            twin.erase(gone)
        else:
            clear = chosen[want.reshape(-1)[chosen] == 0]
            assert len(clear) >= 20 and not got.reshape(-1)[clear].any()                   # (a condition on the inputs, then the check)
            assert counts[0] >= len(chosen)                                                # the pass held erased seeds
        g.free()
    assert n_conv[1] >= 100                                                                # pass 2 ran over that many more erased seeds
    # a batch that has not run a pass marks nothing
    fresh = make()
    g = GuardedGrid(ctx, width, height, cell)
    g.grid.mark_updated([fresh])
    assert not g.read().any()
    g.free()
    for o in (rs, twin, fresh):
        o.destroy()
    kf.destroy(); cf.destroy()


@pytest.mark.parametrize("small_limit", [16384, 0])
@pytest.mark.parametrize("sizes", [(500, 1, 255, 256, 700), (300,) * 11])
def test_mark_updated_over_several_batches(ctx, sizes, small_limit):
    """one call over all batches (more than one set of 8 for 11) against one call per batch and against the model"""
    mk = seedsynth.make_multi_keyframe_case(sizes, seed=31)
    K, cell = len(sizes), 30
    cols, rows = hip.detect_grid(mk.cam.width, mk.cam.height, cell)
    kf = hip.Pyramid(ctx, mk.cam.width, mk.cam.height, 5, K)
    cf = _pyramid(ctx, mk.cur_pyr)
    quiet, twin = [], []
    for k, s in enumerate(mk.keyframes):
        kf.upload(k, s.ref_pyr)
        s2 = (s.sigma2 * np.float32(0.02)).astype(np.float32)
        for lst in (quiet, twin):
            lst.append(hip.ResidentSeeds(ctx, s.px, s.f, s.level, s.a, s.b, s.mu, s.z_range, s2))
    T_refs = np.stack([s.T_ref_w for s in mk.keyframes])
    ctx.set_small_pass_limit(small_limit)
    try:
        for frame in range(2):
            one, per = GuardedGrid(ctx, 640, 480, cell), GuardedGrid(ctx, 640, 480, cell)
            hip.ResidentSeeds.update_group_async(quiet, kf, list(range(K)), cf, 0, mk.cam, T_refs, mk.T_cur_w, report_updated=False)
            one.grid.mark_updated(quiet)
            for b in quiet:
                per.grid.mark_updated([b])
            for b in quiet:
                b.collect()
            hip.ResidentSeeds.update_group_async(twin, kf, list(range(K)), cf, 0, mk.cam, T_refs, mk.T_cur_w, report_updated=True)
            want = np.zeros((rows, cols), np.uint8)
            for b in twin:
                si.mark_px(want, b.collect()[0]["px_cur"], cell)
            assert np.array_equal(one.read(), want) and np.array_equal(per.read(), want) and want.sum() > 100, frame
            one.free(); per.free()
    finally:
        ctx.set_small_pass_limit(8192)
    for b in quiet + twin:
        b.destroy()
    kf.destroy(); cf.destroy()


def test_mark_updated_refusals(ctx):
    s, kf, cf, s2 = _seed_case(ctx, 300, 346, 260)
    other = hip.Context(0)
    a = hip.ResidentSeeds(ctx, s.px, s.f, s.level, s.a, s.b, s.mu, s.z_range, s2)
    b = hip.ResidentSeeds(other, s.px, s.f, s.level, s.a, s.b, s.mu, s.z_range, s2)
    a.update(kf, 0, cf, 0, s.cam, s.T_ref_w, s.T_cur_w)
    g = GuardedGrid(ctx, 346, 260, 20)
    fn, P = ctx.lib.svo_hip_seed_batch_mark_updated, C.c_void_p
    hs = lambda *bs: (C.c_void_p * len(bs))(*[x.h if x is not None else None for x in bs])
    assert fn(2, hs(a, b), 20, 18, 13, P(g.grid.ptr)) == -1                                # batches of different contexts
    assert fn(2, hs(a, None), 20, 18, 13, P(g.grid.ptr)) == -1
    assert fn(1, hs(None), 20, 18, 13, P(g.grid.ptr)) == -1
    assert fn(0, hs(a), 20, 18, 13, P(g.grid.ptr)) == -1
    assert fn(1, None, 20, 18, 13, P(g.grid.ptr)) == -1
    assert fn(1, hs(a), 20, 18, 13, None) == -1
    for dims in ((0, 18, 13), (20, 0, 13), (20, 18, 0), (20, -18, 13)):
        assert fn(1, hs(a), *dims, P(g.grid.ptr)) == -1
    ctx.sync()
    assert not g.read().any()                                                              # nothing was enqueued
    assert fn(1, hs(a), 20, 18, 13, P(g.grid.ptr)) == 0
    assert g.read().any()
    g.free()
    a.destroy(); b.destroy()
    other.close()
    kf.destroy(); cf.destroy()


# ---- 3. the tracker's last frame -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scenario():
    """tests/test_gpu_map_growth.py's scenario with every tenth map point a centimetre off: the alignment still finds those
    features, the pose refinement drops their points -- the frames hold features without a point"""
    s = sc.make()
    pos = s["base_map"]["pt_pos"].copy()
    pos[3::10, 0] += 0.01
    return dict(s, base_map=dict(s["base_map"], pt_pos=pos))


TCELL = 30


def _tracker_marks(ctx, trk, px):
    """the grid svo_hip_tracker_mark_last_frame leaves (over a pre-set cell that must stay) == the model over px"""
    cam = trk.cam
    cols, rows = hip.detect_grid(cam.width, cam.height, TCELL)
    pre = np.zeros((rows, cols), np.uint8)
    pre[rows - 1, cols - 1] = 1
    g = GuardedGrid(ctx, cam.width, cam.height, TCELL, pre)
    trk.mark_last_frame(g.grid)
    got = g.read()
    g.free()
    want = si.mark_px(pre.copy(), px, TCELL)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    return int(want.sum())


def _tracker_run(ctx, s, mark, track=None, trk=None):
    """track, promote, candidates, track, promote, remove, compact, track -- with the grid marked after every step, or never"""
    seq = s["seq"]
    own = trk is None
    if own:
        trk = hip.Tracker(ctx, seq["cam"], **CFG)
        _start(trk, s["base"], s["base_map"])
    track = track or (lambda frames: _frames(trk, seq, frames))
    out = dict(marked=[], pointless=[])

    def check(r, what):
        if mark:
            out["marked"].append((what, _tracker_marks(ctx, trk, r["feat_px"])))
            out["pointless"].append(int((r["feat_point"] < 0).sum()))
    out["f12"] = track((1, 2))
    check(out["f12"][-1], "tracked")
    out["promote1"] = trk.promote_last_frame(1)
    check(out["f12"][-1], "promoted")
    trk.add_candidates(**s["cand"])
    out["f34"] = track((3, 4))
    check(out["f34"][-1], "tracked")
    out["promote2"] = trk.promote_last_frame(2)
    out["remove"] = trk.remove_keyframe(0)
    check(out["f34"][-1], "removed")
    out["compact"] = trk.compact_points()
    check(out["f34"][-1], "compacted")
    out["map"] = trk.download_map()
    out["f5"] = track((5,))
    check(out["f5"][-1], "tracked")
    if own:
        trk.destroy()
    return out


@pytest.fixture(scope="module")
def tracker_runs(ctx):
    s = _scenario()
    return _tracker_run(ctx, s, True), _tracker_run(ctx, s, False)


def test_tracker_marks_every_feature_of_its_last_frame(tracker_runs):
    X, _ = tracker_runs
    assert [w for w, _ in X["marked"]] == ["tracked", "promoted", "tracked", "removed", "compacted", "tracked"]
    assert all(n >= 30 for _, n in X["marked"])
    # features whose point the pose refinement dropped (pose_optimizer.cpp:154-157) stay in fts_ and were marked with the others
    print("features without a point per marked frame:", X["pointless"])
    assert max(X["pointless"]) >= 1
    assert X["remove"]["n_deleted_points"] >= 1 and X["compact"]["n_points"] < len(X["compact"]["old_to_new"])


def test_tracker_marking_only_reads(tracker_runs):
    X, Z = tracker_runs
    for part in ("f12", "f34", "f5"):
        for i, (a, b) in enumerate(zip(X[part], Z[part])):
            _same(a, b, (part, i))
    assert X["promote1"] == Z["promote1"] and X["promote2"] == Z["promote2"] and X["remove"] == Z["remove"]
    assert np.array_equal(X["compact"]["old_to_new"], Z["compact"]["old_to_new"])
    mg.assert_tables_equal(X["map"], Z["map"])


def test_tracker_marks_a_given_last_frame_and_refuses_without_one(ctx):
    s = _scenario()
    seq = s["seq"]
    trk = hip.Tracker(ctx, seq["cam"], **CFG)
    g = GuardedGrid(ctx, seq["cam"].width, seq["cam"].height, TCELL)
    with pytest.raises(hip.SvoHipError, match=r"\(-4\)"):
        trk.mark_last_frame(g.grid)
    assert not g.read().any()
    _start(trk, s["base"], s["base_map"])                  # svo_hip_tracker_set_last_frame
    assert _tracker_marks(ctx, trk, s["base"]["px0"]) >= 30
    # a frame given with pixels outside the image and without points
    px = np.concatenate([si.edge_pixels(TCELL, g.grid.cols, g.grid.rows)[:19], s["base"]["px0"][:7]])
    trk.set_last_frame(s["base"]["T0"], px, np.tile([0.0, 0.0, 1.0], (len(px), 1)), np.full(len(px), -1, np.int32), kf_slot=0)
    _tracker_marks(ctx, trk, px)
    fn, P = ctx.lib.svo_hip_tracker_mark_last_frame, C.c_void_p
    assert fn(trk.h, TCELL, g.grid.cols, g.grid.rows, None) == -1 and fn(None, TCELL, g.grid.cols, g.grid.rows, P(g.grid.ptr)) == -1
    for dims in ((0, 22, 16), (30, 0, 16), (30, 22, -1)):
        assert fn(trk.h, *dims, P(g.grid.ptr)) == -1
    assert not g.read().any()
    g.free()
    trk.destroy()


def test_group_camera_marks_as_its_lone_twin(ctx):
    s = _scenario()
    seq = s["seq"]
    tile = (hip.SIA_OPT_REDUCTION, hip.SIA_REDUCTION_TILE_ORDER)
    cfg = dict(CFG, max_items=1024)
    lone = hip.Tracker(ctx, seq["cam"], **cfg)
    lone.set_sia_option(*tile)
    _start(lone, s["base"], s["base_map"])
    want = _frames(lone, seq, (1, 2))
    n_lone = _tracker_marks(ctx, lone, want[-1]["feat_px"])
    lone.destroy()
    grp = hip.TrackerGroup(ctx, seq["cam"], 2, **cfg)
    grp.set_sia_option(*tile)
    _start(grp.cameras[0], seq, tc.sequence_map(seq))
    _start(grp.cameras[1], s["base"], s["base_map"])
    for k in (1, 2):
        grp.track([seq["pyrs"][k][0]] * 2)
    got = grp.cameras[1].last_result()
    _same(got, want[-1], "group camera 1")
    assert _tracker_marks(ctx, grp.cameras[1], got["feat_px"]) == n_lone
    _tracker_marks(ctx, grp.cameras[0], grp.cameras[0].last_result()["feat_px"])
    grp.destroy()


# ---- 4. seeds created from a detection -------------------------------------------------------------------------------------
def _image(kind):
    rng = np.random.default_rng(8)
    if kind == "noise":
        return rng.integers(0, 256, (480, 640)).astype(np.uint8)
    img = np.kron(rng.integers(0, 256, (30, 40)), np.ones((16, 16))).astype(np.uint8)
    return np.clip(img.astype(np.int32) + rng.integers(-3, 4, img.shape), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _model(width, height, cell):
    return model_case(width, height, cell)


def _detect_case(kind):
    """(camera, the pyramid to detect on, the pyramid and poses of the passes, depth_mean, depth_min)"""
    if kind.startswith("model"):
        m = _model(*CASES[0 if kind == "model640" else 1])
        s = m["sc"]
        return s.cam, s.ref_pyr, s.cur_pyr, s.T_ref_w, s.T_cur_w, 1.1 * m["zbar"], 0.5 * m["zbar"]
    s = _model(*CASES[0])["sc"]
    pyr = synth.build_pyramid(_image(kind))
    return s.cam, pyr, pyr, s.T_ref_w, s.T_cur_w, 2.2, 1.0


def _same_batches(a, b, what):
    assert np.array_equal(a.status(), b.status()), what
    d, e = a.download(), b.download()
    for key in d:
        assert d[key].tobytes() == e[key].tobytes(), (what, key)
    assert a.n_alive() == b.n_alive(), what


DETECT = [("model640", 30, 3), ("model346", 20, 3), ("noise", 20, 3), ("noise", 16, 5), ("blocks", 30, 2), ("blocks", 20, 3)]


@pytest.mark.parametrize("with_grid", [False, True])
@pytest.mark.parametrize("kind,cell,n_levels", DETECT)
def test_seeds_created_from_a_detection(ctx, kind, cell, n_levels, with_grid):
    cam, det_pyr, cur_pyr, T_ref_w, T_cur_w, depth_mean, depth_min = _detect_case(kind)
    cols, rows = hip.detect_grid(cam.width, cam.height, cell)
    kf, cf = _pyramid(ctx, det_pyr), _pyramid(ctx, cur_pyr)
    occ = (np.random.default_rng(cell).uniform(size=rows * cols) < 0.3).astype(np.uint8) if with_grid else None
    px, f, lvl, score = hip.detect_features(ctx, kf, 0, cam, n_pyr_levels=n_levels, cell_size=cell, occupancy=occ)
    before = ctx.info()["seed_blocks_in_use"]
    g = GuardedGrid(ctx, cam.width, cam.height, cell, occ) if with_grid else None
    rs, feats = hip.ResidentSeeds.from_detection(ctx, kf, 0, cam, depth_mean, depth_min, n_pyr_levels=n_levels, cell_size=cell,
                                                 grid=g.grid if g else None, clear_grid=False)
    assert rs is not None and rs.n == len(px) >= 30 and ctx.info()["seed_blocks_in_use"] == before + 1
    for key, want in (("px", px), ("f", f), ("level", lvl), ("score", score)):
        assert feats[key].dtype == want.dtype and feats[key].tobytes() == want.tobytes(), key
    if g:
        assert np.array_equal(g.read().reshape(-1), occ)                                   # clear_occupancy = 0: the grid stays
        k = (px[:, 1] // cell).astype(int) * cols + (px[:, 0] // cell).astype(int)
        assert not occ[k].any()
    a, b, mu, zr, s2 = seedsynth.seed_ctor(depth_mean, depth_min, rs.n)
    d = rs.download()
    assert (d["alive"] == 1).all() and (rs.status() == hip.SEED_ERASED).all() and rs.n_alive() == rs.n
    for key, want in (("a", a), ("b", b), ("mu", mu), ("sigma2", s2)):
        assert d[key].tobytes() == want.tobytes(), key
    twin = hip.ResidentSeeds(ctx, px, f, lvl, a, b, mu, zr, s2)
    n_updated = 0
    for frame in range(3):
        kw = dict(report_updated=frame == 1)
        got = rs.update(kf, 0, cf, 0, cam, T_ref_w, T_cur_w, **kw)
        want = twin.update(kf, 0, cf, 0, cam, T_ref_w, T_cur_w, **kw)
        assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]), frame
        _same_batches(rs, twin, frame)
        n_updated += int(got[1][hip.SEED_UPDATED + 1])
    if kind.startswith("model"):
        assert n_updated >= 30                                                             # (z_range is compared through these updates)
    # erase and a further pass work on it as on any batch
    rs.erase([0, rs.n - 1]); twin.erase([0, rs.n - 1])
    assert rs.update(kf, 0, cf, 0, cam, T_ref_w, T_cur_w)[0].tobytes() == twin.update(kf, 0, cf, 0, cam, T_ref_w, T_cur_w)[0].tobytes()
    _same_batches(rs, twin, "erased")
    rs.destroy(); twin.destroy()
    assert ctx.info()["seed_blocks_in_use"] == before
    if g:
        g.free()
    kf.destroy(); cf.destroy()


@pytest.mark.parametrize("small_limit", [16384, 0])
def test_detected_batch_inside_a_grouped_pass(ctx, small_limit):
    cam, det_pyr, cur_pyr, T_ref_w, T_cur_w, depth_mean, depth_min = _detect_case("model640")
    s = _model(*CASES[0])["sc"]
    kf, cf = _pyramid(ctx, det_pyr), _pyramid(ctx, cur_pyr)
    px, f, lvl, _ = hip.detect_features(ctx, kf, 0, cam, n_pyr_levels=3, cell_size=30)
    ctor = seedsynth.seed_ctor(depth_mean, depth_min, len(px))
    ordinary = lambda: hip.ResidentSeeds(ctx, s.px, s.f, s.level, s.a, s.b, s.mu, s.z_range, s.sigma2)
    det, _ = hip.ResidentSeeds.from_detection(ctx, kf, 0, cam, depth_mean, depth_min, n_pyr_levels=3, cell_size=30)
    X, Y = [ordinary(), det], [ordinary(), hip.ResidentSeeds(ctx, px, f, lvl, *ctor)]
    T_refs = np.stack([T_ref_w, T_ref_w])
    ctx.set_small_pass_limit(small_limit)
    try:
        for frame in range(3):
            out = []
            for grp in (X, Y):
                hip.ResidentSeeds.update_group_async(grp, kf, [0, 0], cf, 0, cam, T_refs, T_cur_w, report_updated=frame == 2)
                out.append([b.collect() for b in grp])
            for k in range(2):
                assert out[0][k][0].tobytes() == out[1][k][0].tobytes() and np.array_equal(out[0][k][1], out[1][k][1]), (frame, k)
                _same_batches(X[k], Y[k], (frame, k))
    finally:
        ctx.set_small_pass_limit(8192)
    for b in X + Y:
        b.destroy()
    kf.destroy(); cf.destroy()


def test_detection_without_features_and_phantom_features(ctx):
    cam = _model(*CASES[0])["sc"].cam
    flat = _pyramid(ctx, synth.build_pyramid(np.full((480, 640), 90, np.uint8)))
    noise = _pyramid(ctx, synth.build_pyramid(_image("noise")))
    before = ctx.info()["seed_blocks_in_use"]
    rs, feats = hip.ResidentSeeds.from_detection(ctx, flat, 0, cam, 2.2, 1.0, cell_size=30)
    assert rs is None and all(len(v) == 0 for v in feats.values())
    g = GuardedGrid(ctx, 640, 480, 30, np.ones(22 * 16, np.uint8))
    rs, feats = hip.ResidentSeeds.from_detection(ctx, noise, 0, cam, 2.2, 1.0, cell_size=30, grid=g.grid, clear_grid=True)
    assert rs is None and len(feats["px"]) == 0
    assert not g.read().any()                                                              # clear_occupancy = 1: zeroed behind the detection
    assert ctx.info()["seed_blocks_in_use"] == before
    # clear_occupancy on a detection that finds features; the features are those of the grid as it was
    occ = (np.random.default_rng(3).uniform(size=22 * 16) < 0.5).astype(np.uint8)
    g.grid.upload(occ)
    rs, feats = hip.ResidentSeeds.from_detection(ctx, noise, 0, cam, 2.2, 1.0, cell_size=30, grid=g.grid, clear_grid=True)
    px, _, _, _ = hip.detect_features(ctx, noise, 0, cam, cell_size=30, occupancy=occ)
    assert feats["px"].tobytes() == px.tobytes() and len(px) >= 100 and not g.read().any()
    rs.destroy()
    g.free()
    # threshold 10.1 on a constant image: every cell yields the reference's Feature(px (0,0), level 0)
    rs, feats = hip.ResidentSeeds.from_detection(ctx, flat, 0, cam, 2.2, 1.0, cell_size=30, detection_threshold=10.1)
    px, f, lvl, score = hip.detect_features(ctx, flat, 0, cam, cell_size=30, detection_threshold=10.1)
    assert rs.n == 22 * 16 == len(px) and not feats["px"].any() and not feats["level"].any() and (feats["score"] == np.float32(10.1)).all()
    for key, want in (("px", px), ("f", f), ("level", lvl), ("score", score)):
        assert feats[key].tobytes() == want.tobytes(), key
    d = rs.download()
    a, b, mu, zr, s2 = seedsynth.seed_ctor(2.2, 1.0, rs.n)
    assert (d["alive"] == 1).all() and all(d[k].tobytes() == w.tobytes() for k, w in (("a", a), ("b", b), ("mu", mu), ("sigma2", s2)))
    rs.destroy()
    assert ctx.info()["seed_blocks_in_use"] == before
    flat.destroy(); noise.destroy()


def test_create_detected_cycles_do_not_allocate(ctx):
    cam, det_pyr, _, _, _, depth_mean, depth_min = _detect_case("model640")
    kf = _pyramid(ctx, det_pyr)
    g = GuardedGrid(ctx, 640, 480, 30)
    first = None
    for cycle in range(11):
        if cycle == 1:
            before = ctx.info()
        g.grid.mark_px(np.array([[100.0, 100.0], [300.0, 200.0]]))
        rs, feats = hip.ResidentSeeds.from_detection(ctx, kf, 0, cam, depth_mean, depth_min, cell_size=30, grid=g.grid)
        first = first if first is not None else feats["px"]
        assert feats["px"].tobytes() == first.tobytes()
        rs.destroy()
    after = ctx.info()
    assert after["allocator_calls"] == before["allocator_calls"] and after["free_calls"] == before["free_calls"], (before, after)
    assert not g.read().any()
    g.free()
    kf.destroy()


def test_create_detected_refusals_take_no_block(ctx):
    """every refusal of svo_hip_detect_features_dev, and the missing camera: SVO_HIP_ERR_INVALID, no batch, no block"""
    cam = _model(*CASES[0])["sc"].cam
    pyr = _pyramid(ctx, synth.build_pyramid(_image("noise")), n_levels=3)
    big = hip.Pyramid(ctx, 4096, 4096, 1, 1)                                               # 2^24 pixels: beyond the cells' keys
    c = hip.make_camera(cam)
    g = GuardedGrid(ctx, 640, 480, 30, np.ones(22 * 16, np.uint8))
    before = ctx.info()
    px = np.zeros((22 * 16, 2))

    def call(pyr_h=pyr.h, slot=0, cam_p=C.byref(c), n_levels=3, cell=30, thr=10.0, ctx_h=ctx.h, n_p=True, out_p=True):
        h, n = C.c_void_p(), C.c_int32(-7)
        rc = ctx.lib.svo_hip_seed_batch_create_detected(ctx_h, pyr_h, slot, cam_p, n_levels, cell, C.c_void_p(g.grid.ptr), 1, C.c_double(thr),
                                                        C.c_double(2.2), C.c_double(1.0), C.byref(h) if out_p else None,
                                                        C.byref(n) if n_p else None, px.ctypes.data_as(C.c_void_p), None, None, None)
        assert not h.value
        return rc
    assert call(pyr_h=None) == -1
    assert call(slot=-1) == -1 and call(slot=1) == -1
    assert call(n_levels=0) == -1 and call(n_levels=4) == -1
    assert call(cell=0) == -1 and call(cell=-5) == -1
    assert call(thr=-1.0) == -1 and call(thr=-1e-300) == -1
    assert call(cam_p=None) == -1
    assert call(pyr_h=big.h, n_levels=1, cell=4096) == -1
    assert call(ctx_h=None) == -1 and call(n_p=False) == -1 and call(out_p=False) == -1
    after = ctx.info()
    assert after == before, (before, after)
    assert g.read().all()                                                                  # (nor was the grid cleared)
    assert call(thr=float("nan")) == 0                                                     # NaN: no feature, as svo_hip_detect_features
    assert ctx.info()["seed_blocks_in_use"] == before["seed_blocks_in_use"]
    g.free()
    pyr.destroy(); big.destroy()


# ---- 5. the whole keyframe ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,height,cell", CASES)
def test_whole_keyframe_equals_the_model_sequence(ctx, width, height, cell):
    """updateSeeds marks, setExistingFeatures marks, initializeSeeds detects and resets: the seeds of the model test's keyframe
    updated against the current frame, the case's 64 pixels as the frame's features, the new seeds detected on the current frame"""
    m = _model(width, height, cell)
    s, dm, dn = m["sc"], 1.1 * m["zbar"], 0.5 * m["zbar"]
    kf, cf = _pyramid(ctx, s.ref_pyr), _pyramid(ctx, s.cur_pyr)
    g = GuardedGrid(ctx, width, height, cell)
    old, feats0 = hip.ResidentSeeds.from_detection(ctx, kf, 0, s.cam, dm, dn, cell_size=cell)
    assert feats0["px"].tobytes() == m["px"].tobytes() and np.array_equal(feats0["level"], m["level"])
    old.update_async(kf, 0, cf, 0, s.cam, s.T_ref_w, s.T_cur_w, report_updated=False)
    g.grid.mark_updated([old])
    g.grid.mark_px(s.px)
    seen = g.read()                                                                        # the grid as the detector sees it
    old.collect()
    new, feats = hip.ResidentSeeds.from_detection(ctx, cf, 0, s.cam, dm, dn, cell_size=cell, grid=g.grid, clear_grid=True)
    assert not g.read().any()
    # (the model case's own state arrays hold the seeds AFTER the oracle's pass: the twin starts from the constructor's)
    twin = hip.ResidentSeeds(ctx, m["px"], m["f"], m["level"], *seedsynth.seed_ctor(dm, dn, len(m["px"])))
    tev, _ = twin.update(kf, 0, cf, 0, s.cam, s.T_ref_w, s.T_cur_w, report_updated=True)
    status = np.full(len(m["px"]), hip.SEED_NO_MATCH, np.int32)
    px_cur = np.full((len(m["px"]), 2), np.nan)
    status[tev["index"]], px_cur[tev["index"]] = tev["status"], tev["px_cur"]
    want = si.keyframe_sequence(s.cam, s.cur_pyr, cell, 3, 10.0, dm, dn, seed_passes=[(status, px_cur)], existing_px=s.px)
    assert np.array_equal(seen, want["grid"])
    assert feats["px"].tobytes() == want["px"].tobytes() and np.array_equal(feats["level"], want["level"])
    assert feats["score"].tobytes() == want["score"].tobytes() and new.n == len(want["px"]) >= 30
    assert feats["f"].tobytes() == np.ascontiguousarray(synth.cam2world(s.cam, want["px"])).tobytes()
    d = new.download()
    assert all(d[k].tobytes() == want[k].tobytes() for k in ("a", "b", "mu", "sigma2")) and (d["alive"] == 1).all()
    # the device's pass marks what the oracle's pass marks (the model test's own grid)
    oracle = si.keyframe_sequence(s.cam, s.cur_pyr, cell, 3, 10.0, dm, dn, seed_passes=[(m["status"], m["px_cur"])], existing_px=s.px)
    print("new seeds %d; grid cells that differ from the oracle pass's grid: %d" % (new.n, int((oracle["grid"] != seen).sum())))
    for o in (old, new, twin):
        o.destroy()
    g.free()
    kf.destroy(); cf.destroy()


# ---- 6. the C++ host twin ------------------------------------------------------------------------------------------------------
KF_AT, N_FRAMES, N_EXISTING, KF_CELL = (0, 3, 6), 9, 120, 30


@functools.lru_cache(maxsize=None)
def _twin_case():
    rng = np.random.default_rng(4)
    cam = synth.Camera.default()
    scene = synth.PlaneScene(seed=4, depth=2.0, tilt=(0.08, 0.05))
    T0 = synth.se3_from_twist([0.02, -0.01, 0.0], [0.01, 0.005, -0.01])
    direction = np.array([1.0, 0.3, 0.1]) / np.linalg.norm([1.0, 0.3, 0.1])
    poses = [T0] + [synth.se3_mul(synth.se3_from_twist(direction * 0.035 * k, rng.uniform(-0.004, 0.004, 3)), T0) for k in range(1, N_FRAMES)]
    pyrs = [synth.build_pyramid(scene.render(cam, T)) for T in poses]
    X = scene.intersect(cam, T0, np.array([cam.width / 2.0]), np.array([cam.height / 2.0]))
    zbar = float(np.linalg.norm(X - synth.se3_inv(T0)[:3], axis=1)[0])
    existing = [np.floor(np.stack([rng.uniform(0, cam.width, N_EXISTING), rng.uniform(0, cam.height, N_EXISTING)], axis=1)) for _ in KF_AT]
    return dict(cam=cam, poses=poses, pyrs=pyrs, depth=(1.1 * zbar, 0.5 * zbar), existing=existing)


def _write_twin_case(case, tw):
    from test_gpu_host_cpp import _write
    cam = tw["cam"]
    _write(case / "manifest.bin", [cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy, 5, N_FRAMES], np.float64)
    for k in range(N_FRAMES):
        _write(case / ("frame_%d_pose.bin" % k), tw["poses"][k], np.float64)
        for l in range(5):
            _write(case / ("frame_%d_L%d.bin" % (k, l)), tw["pyrs"][k][l], np.uint8)
    _write(case / "depth_mean_min.bin", tw["depth"], np.float64)
    _write(case / "kf_params.bin", [3, KF_CELL, 10.0], np.float64)
    _write(case / "kf_list.bin", KF_AT, np.float64)
    for j, px in enumerate(tw["existing"]):
        _write(case / ("kf_existing_%d.bin" % j), px, np.float64)


def _replay_twin(ctx, tw, threaded):
    """the keyframe protocol through the Python mirror: per keyframe (the grid the detector saw, px, level), the callbacks
    (seed id, xyz_world, sigma2) in list order, and per ordinary frame the seeds on the device"""
    cam = tw["cam"]
    kfp = hip.Pyramid(ctx, cam.width, cam.height, 5, len(KF_AT))
    cur = hip.Pyramid(ctx, cam.width, cam.height, 5, 1)
    g = GuardedGrid(ctx, cam.width, cam.height, KF_CELL)
    batches, kfs, conv, frames = [], [], [], []          # batches: [ResidentSeeds, first seed id, keyframe's frame index, slot]

    def update(k, mark):
        live = [b for b in batches if b[0].n_alive() > 0]
        if not live:
            return 0
        cur.upload(0, tw["pyrs"][k])
        hip.ResidentSeeds.update_group_async([b[0] for b in live], kfp, [b[3] for b in live], cur, 0, cam,
                                             np.stack([tw["poses"][b[2]] for b in live]), tw["poses"][k], report_updated=False)
        if mark:
            g.grid.mark_updated([b[0] for b in live])
        n = sum(b[0].n_alive() for b in live)
        for b in live:
            ev, _ = b[0].collect()
            for e in ev[ev["status"] == hip.SEED_CONVERGED]:
                conv.append(np.concatenate([[float(b[1] + e["index"])], e["xyz_world"], [float(e["sigma2"])]]))
        return n
    n_ids = 0
    for k in range(N_FRAMES):
        if k in KF_AT:
            j = KF_AT.index(k)
            if threaded:
                update(k, True)
            g.grid.mark_px(tw["existing"][j])
            seen = g.read().copy()
            kfp.upload(j, tw["pyrs"][k])
            rs, feats = hip.ResidentSeeds.from_detection(ctx, kfp, j, cam, float(np.float32(tw["depth"][0])), float(np.float32(tw["depth"][1])), cell_size=KF_CELL,
                                                         grid=g.grid, clear_grid=True)
            kfs.append((seen, feats["px"], feats["level"]))
            if rs is not None:
                batches.append([rs, n_ids, k, j])
            n_ids += len(feats["px"])
        else:
            frames.append((k, update(k, False)))
    for b in batches:
        b[0].destroy()
    g.free(); kfp.destroy(); cur.destroy()
    return kfs, np.array(conv).reshape(-1, 5), frames


@pytest.mark.parametrize("threaded", [False, True], ids=["unthreaded", "threaded"])
def test_host_twin_makes_a_keyframes_seeds_on_the_device(ctx, tmp_path, threaded):
    """svo_host_demo keyframes: DepthFilter::addKeyframe without features (enableDeviceSeedInit) against the same run with the
    features detected by the caller on a host DetectorGrid and handed in, and against a replay through the Python mirror:
    per-keyframe grids, seeds and every convergence callback byte for byte; after a keyframe the next frame uploads nothing
    with device seeds and the keyframe's seeds without."""
    import os
    import subprocess
    from test_gpu_host_cpp import DEMO
    assert os.path.exists(DEMO), "build() must have produced android_svo_amd/host/svo_host_demo"
    tw = _twin_case()
    case = tmp_path / "case"
    case.mkdir()
    _write_twin_case(case, tw)
    outs = {}
    for flag in ("device_seeds", "host"):
        out = tmp_path / flag
        out.mkdir()
        args = [DEMO, str(case), str(out), "keyframes"] + (["device_seeds"] if flag == "device_seeds" else []) + (["threaded"] if threaded else [])
        p = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        outs[flag] = out
    kfs, conv, frames = _replay_twin(ctx, tw, threaded)
    names = ["kf_counts.bin", "conv.bin"] + ["kf%d_%s.bin" % (j, w) for j in range(len(KF_AT)) for w in ("grid", "px", "level")]
    for name in names:
        assert (outs["device_seeds"] / name).read_bytes() == (outs["host"] / name).read_bytes(), name
    counts = np.fromfile(outs["device_seeds"] / "kf_counts.bin")
    assert len(counts) == len(KF_AT) and (counts >= 30).all()
    for j, (seen, px, level) in enumerate(kfs):
        assert (outs["device_seeds"] / ("kf%d_grid.bin" % j)).read_bytes() == seen.tobytes(), j
        assert (outs["device_seeds"] / ("kf%d_px.bin" % j)).read_bytes() == px.tobytes(), j
        assert (outs["device_seeds"] / ("kf%d_level.bin" % j)).read_bytes() == level.tobytes(), j
        marked_by_seeds = int(seen.sum()) - int(si.mark_px(np.zeros_like(seen), tw["existing"][j], KF_CELL).sum())
        assert (marked_by_seeds > 20) if (threaded and j > 0) else (marked_by_seeds == 0), (j, marked_by_seeds)
    got = np.fromfile(outs["device_seeds"] / "conv.bin").reshape(-1, 5)
    assert got.tobytes() == conv.tobytes() and len(conv) >= 20
    # the frame after a keyframe: nothing uploaded with device seeds, the keyframe's seeds without
    rows = {f: np.fromfile(outs[f] / "frames.bin").reshape(-1, 3) for f in outs}
    assert np.array_equal(rows["device_seeds"][:, :2], rows["host"][:, :2])
    assert [int(r[0]) for r in rows["host"]] == [k for k, _ in frames] and [int(r[1]) for r in rows["host"]] == [n for _, n in frames]
    assert not rows["device_seeds"][:, 2].any()
    after_kf = {k + 1: int(counts[j]) for j, k in enumerate(KF_AT)}
    assert [int(r[2]) for r in rows["host"]] == [after_kf.get(int(r[0]), 0) for r in rows["host"]]
