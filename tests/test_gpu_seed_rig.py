"""svo_hip_seed_batch_update_rig_async: the seed batches of the cameras of a RIG -- each with its own camera model (intrinsics,
distortion, and the pixel error angle they imply), current frame, pose and keyframe flag -- through one set of launches.  The
reference is the existing pass per camera with that camera's model (svo_hip_seed_batch_update_group_async in the six-launch form)
on twin batches: events, status counts, status(), px_cur as the detector grid sees it, every array of download() and n_alive()
equal BYTES per batch over three frames, in both forms of the call.  The first frame is also held against the CPU oracle under
the bars of tests/test_gpu_seed_cameras.py.  The cameras' models differ enough for a wrong one to show
(tests/test_rig_inputs_cpu.py).  Three equal cameras through the rig call equal svo_hip_seed_batch_update_cameras_async."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import rig_case as rc
from android_svo_amd import hip

pytestmark = pytest.mark.gpu

FORMS = (16384, 0)                       # svo_hip_df_set_small_pass_limit: the two-launch form for all arrangements, and off


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.set_small_pass_limit(8192)


class Rig:
    """An arrangement on the device: ONE keyframe pyramid batch for all cameras (camera c's keyframe s in slot c * K + s, as a
    tracker group keeps them), one batch of current frames (camera c in slot c), or both in reversed order."""

    def __init__(self, ctx, arr):
        self.ctx, self.arr = ctx, arr
        self.cams = rc.cameras(arr)
        self.models = [mk.cam for mk in self.cams]
        n, self.K = len(self.cams), max(1, max(len(z) for z in arr.sizes))
        self.kf = hip.Pyramid(ctx, rc.WIDTH, rc.HEIGHT, rc.LEVELS, n * self.K)
        self.cf = hip.Pyramid(ctx, rc.WIDTH, rc.HEIGHT, rc.LEVELS, n)
        rev = arr.reversed_slots
        self.cur_slot = [n - 1 - c if rev else c for c in range(n)]
        self.ref_slots = [[c * self.K + (self.K - 1 - k if rev else k) for k in range(len(mk.keyframes))] for c, mk in enumerate(self.cams)]
        for c, mk in enumerate(self.cams):
            self.cf.upload(self.cur_slot[c], mk.cur_pyr)
            for k, sc in enumerate(mk.keyframes):
                self.kf.upload(self.ref_slots[c][k], sc.ref_pyr)
        self.T_refs = [np.stack([sc.T_ref_w for sc in mk.keyframes]) if mk.keyframes else np.zeros((0, 7)) for mk in self.cams]
        self.sets = []

    def twins(self):
        """a fresh set of the arrangement's batches: [camera][batch]"""
        s = [[hip.ResidentSeeds(self.ctx, sc.px, sc.f, sc.level, sc.a, sc.b, sc.mu, sc.z_range, rc.sigma2_of(sc)) for sc in mk.keyframes]
             for mk in self.cams]
        self.sets.append(s)
        return s

    def camera_pass(self, batches, c, keyframe):
        return (batches[c], self.ref_slots[c], self.T_refs[c], self.cur_slot[c], self.cams[c].T_cur_w, keyframe)

    def per_camera(self, batches, flags, models=None):
        """the reference: one grouped pass per camera with the camera's model, six-launch form"""
        self.ctx.set_small_pass_limit(0)
        for c, mk in enumerate(self.cams):
            if batches[c]:
                hip.ResidentSeeds.update_group_async(batches[c], self.kf, self.ref_slots[c], self.cf, self.cur_slot[c], (models or self.models)[c],
                                                     self.T_refs[c], mk.T_cur_w, report_updated=flags[c])
        return [[rs.collect() for rs in cam] for cam in batches]

    def rig_call(self, batches, flags, only=None, models=None):
        cams = list(range(len(self.cams))) if only is None else only
        hip.ResidentSeeds.update_cameras_async([self.camera_pass(batches, c, flags[c]) for c in cams], self.kf, self.cf,
                                               [(models or self.models)[c] for c in cams], ctx=self.ctx)

    def grid_of(self, batches_of_camera):
        """the detector grid svo_hip_seed_batch_mark_updated leaves: what reads px_cur and the statuses on the device"""
        g = hip.DetectorGrid(self.ctx, rc.WIDTH, rc.HEIGHT, 10)
        g.mark_updated(batches_of_camera)
        self.ctx.sync()
        out = g.download()
        g.free()
        return out

    def destroy(self):
        for s in self.sets:
            for cam in s:
                for rs in cam:
                    rs.destroy()
        self.kf.destroy(); self.cf.destroy()


def same_batch(got, want, got_out, want_out, where):
    assert np.array_equal(got_out[1], want_out[1]), where                       # status histogram
    assert got_out[0].tobytes() == want_out[0].tobytes(), where                 # events (index, status, mu, sigma2, xyz_world, px_cur)
    assert got.status().tobytes() == want.status().tobytes(), where
    d, e = got.download(), want.download()
    assert sorted(d) == ["a", "alive", "b", "mu", "sigma2"]
    for key in d:
        assert d[key].tobytes() == e[key].tobytes(), (where, key)
    assert got.n_alive() == want.n_alive(), where


@pytest.mark.parametrize("small_limit", FORMS)
@pytest.mark.parametrize("name", [a.name for a in rc.ARRANGEMENTS])
def test_rig_pass_equals_one_pass_per_camera_with_its_model(ctx, name, small_limit):
    rig = Rig(ctx, rc.BY_NAME[name])
    try:
        n_cams = len(rig.cams)
        want_b, got_b = rig.twins(), rig.twins()
        n_reported = 0
        for frame in range(3):
            flags = [True] * n_cams if frame == 1 else [False] * n_cams        # frame 1 is every camera's keyframe: px_cur of all updated seeds
            want = rig.per_camera(want_b, flags)
            ctx.set_small_pass_limit(small_limit)
            rig.rig_call(got_b, flags)
            assert all(rs.pending() for cam in got_b for rs in cam)
            got = [[rs.collect() for rs in cam] for cam in got_b]
            for c in range(n_cams):
                for k in range(len(want_b[c])):
                    same_batch(got_b[c][k], want_b[c][k], got[c][k], want[c][k], (name, frame, c, k))
                    n_reported += int((got[c][k][0]["status"] == hip.SEED_UPDATED).sum())
                if want_b[c]:
                    assert rig.grid_of(got_b[c]).tobytes() == rig.grid_of(want_b[c]).tobytes(), (name, frame, c)      # px_cur
            if frame == 0:
                _first_pass_against_the_oracle(rig, got_b, name)
        assert n_reported > 0
    finally:
        rig.destroy()


def _first_pass_against_the_oracle(rig, batches, name):
    """the bars of tests/test_gpu_seed_cameras.py: statuses equal, mu equal for all but a few seeds in a thousand (over the
    arrangement: its batches go down to 31 seeds)"""
    oracle = rc.oracle_first_pass(name)
    n_same = n_all = 0
    for c, mk in enumerate(rig.cams):
        for k, sc in enumerate(mk.keyframes):
            o = oracle[c][k]
            st, d = batches[c][k].status(), batches[c][k].download()
            assert np.array_equal(st, o["status"]), (name, c, k)
            n_same += int((d["mu"] == o["mu"]).sum())
            n_all += len(sc.px)
    assert n_same >= 0.995 * n_all, (name, n_same, n_all)


@pytest.fixture()
def abc(ctx):
    rig = Rig(ctx, rc.BY_NAME["sizes_around_a_block"])
    yield rig
    rig.destroy()


def test_three_equal_cameras_equal_the_cameras_call(ctx, abc):
    """the old entry point is the rig call with one model repeated: same scenes, every camera given camera A's model"""
    rig = abc
    same = [rig.models[0]] * 3
    for small_limit in FORMS:
        want_b, got_b = rig.twins(), rig.twins()
        for frame in range(2):
            flags = [frame == 1, False, frame == 1]
            ctx.set_small_pass_limit(small_limit)
            hip.ResidentSeeds.update_cameras_async([rig.camera_pass(want_b, c, flags[c]) for c in range(3)], rig.kf, rig.cf, rig.models[0], ctx=ctx)
            want = [[rs.collect() for rs in cam] for cam in want_b]
            rig.rig_call(got_b, flags, models=same)
            got = [[rs.collect() for rs in cam] for cam in got_b]
            for c in range(3):
                for k in range(len(want_b[c])):
                    same_batch(got_b[c][k], want_b[c][k], got[c][k], want[c][k], (small_limit, frame, c, k))


def test_two_rig_calls_back_to_back_for_disjoint_batches(ctx, abc):
    """nothing is collected between the calls: the second must not rewrite the first one's job and camera tables while they
    are in flight"""
    rig = abc
    want_b, got_b = rig.twins(), rig.twins()
    for small_limit in FORMS:
        for frame in range(2):
            flags = [frame == 1, False, True]
            want = rig.per_camera(want_b, flags)
            ctx.set_small_pass_limit(small_limit)
            rig.rig_call(got_b, flags, only=[2, 0])
            rig.rig_call(got_b, flags, only=[1])
            assert all(rs.pending() for cam in got_b for rs in cam)
            got = [[rs.collect() for rs in cam] for cam in got_b]
            for c in range(3):
                for k in range(len(want_b[c])):
                    same_batch(got_b[c][k], want_b[c][k], got[c][k], want[c][k], (small_limit, frame, c, k))


def test_ten_warm_rig_calls_make_no_allocator_call(ctx, abc):
    rig = abc
    b = rig.twins()
    flags = [False] * 3
    for small_limit in FORMS:
        ctx.set_small_pass_limit(small_limit)
        rig.rig_call(b, flags)                                                  # the warm-up call
        [rs.collect() for cam in b for rs in cam]
        before = ctx.info()
        for _ in range(10):
            rig.rig_call(b, flags)
            [rs.collect() for cam in b for rs in cam]
        after = ctx.info()
        assert after["allocator_calls"] == before["allocator_calls"] and after["free_calls"] == before["free_calls"], (before, after)


def numpy_marks(batches_of_camera, cell=10):
    """setGridOccpuancy of every seed a pass updated (status >= UPDATED), from the batches' events of a keyframe pass"""
    gc, gr = hip.detect_grid(rc.WIDTH, rc.HEIGHT, cell)
    grid = np.zeros(gc * gr, np.uint8)
    for ev in batches_of_camera:
        px = ev["px_cur"][ev["status"] >= hip.SEED_UPDATED]
        k = (px[:, 1] / cell).astype(np.int64) * gc + (px[:, 0] / cell).astype(np.int64)
        grid[k[(k >= 0) & (k < len(grid))]] = 1
    return grid


def test_mark_updated_behind_a_rig_pass(ctx, abc):
    """svo_hip_seed_batch_mark_updated enqueued BEHIND the rig pass while it is pending: every camera's grid is the numpy model
    over the events of its keyframe pass"""
    rig = abc
    for small_limit in FORMS:
        b = rig.twins()
        ctx.set_small_pass_limit(small_limit)
        rig.rig_call(b, [True] * 3)
        gs = [hip.DetectorGrid(ctx, rc.WIDTH, rc.HEIGHT, 10) for _ in range(3)]
        for c in range(3):
            gs[c].mark_updated(b[c])
        assert all(rs.pending() for cam in b for rs in cam)
        events = [[rs.collect()[0] for rs in cam] for cam in b]
        ctx.sync()
        grids = [g.download().ravel() for g in gs]
        [g.free() for g in gs]
        for c in range(3):
            want = numpy_marks(events[c])
            assert want.any() and np.array_equal(grids[c], want), (small_limit, c)
        assert grids[0].tobytes() != grids[1].tobytes()                         # the cameras see different scenes


@pytest.mark.parametrize("case", ["width", "height", "size_of_a_camera_that_sits_out", "all_cameras_of_another_size", "null_cams"])
def test_refusals_enqueue_nothing_and_leave_the_batches_collectable(ctx, abc, case):
    rig = abc
    b = rig.twins()
    rig.rig_call(b, [False] * 3)                                                # the previous pass, not collected yet
    passes = [rig.camera_pass(b, c, False) for c in range(3)]
    models = list(rig.models)
    if case == "width":
        models[1] = dataclasses.replace(models[1], width=models[1].width + 16)
    elif case == "height":
        models[2] = rc.camera("C", rc.WIDTH, rc.HEIGHT - 8)
    elif case == "size_of_a_camera_that_sits_out":
        passes[1] = ([], [], np.zeros((0, 7)), 1, rig.cams[1].T_cur_w, False)
        models[1] = dataclasses.replace(models[1], height=models[1].height + 2)
    elif case == "all_cameras_of_another_size":                                 # equal among themselves, not the pyramids' size
        models = [rc.camera(n, rc.WIDTH + 16, rc.HEIGHT) for n in rig.arr.order]
    # (with a pass pending on every batch a call that got past the camera checks would answer SVO_HIP_ERR_STATE (-4) instead)
    fresh = rig.twins()
    fresh_passes = [rig.camera_pass(fresh, c, False) for c in range(3)]
    if case == "size_of_a_camera_that_sits_out":
        fresh_passes[1] = passes[1]
    if case == "null_cams":
        arr = (hip.CSeedCameraPass * 1)()
        prm = hip.depth_filter_params()
        assert ctx.lib.svo_hip_seed_batch_update_rig_async(ctx.h, 1, arr, rig.kf.h, rig.cf.h, None, C.byref(prm)) == -1
        assert ctx.lib.svo_hip_seed_batch_update_rig_async(ctx.h, 0, arr, rig.kf.h, rig.cf.h, None, C.byref(prm)) == -1
    else:
        with pytest.raises(hip.SvoHipError, match=r"\(-1\)"):                  # SVO_HIP_ERR_INVALID
            hip.ResidentSeeds.update_cameras_async(fresh_passes, rig.kf, rig.cf, models, ctx=ctx)
    assert not any(rs.pending() for cam in fresh for rs in cam)
    assert all((rs.status() == hip.SEED_ERASED).all() for cam in fresh for rs in cam)       # no pass ran on the fresh batches
    # the batches of the previous pass are still collectable, with the results of that pass
    twin = rig.twins()
    want = rig.per_camera(twin, [False] * 3)
    got = [[rs.collect() for rs in cam] for cam in b]
    for c in range(3):
        for k in range(len(b[c])):
            same_batch(b[c][k], twin[c][k], got[c][k], want[c][k], (case, c, k))
    # ... and a well-formed rig call takes the fresh batches afterwards
    rig.rig_call(fresh, [False] * 3)
    for cam in fresh:
        for rs in cam:
            rs.collect()
