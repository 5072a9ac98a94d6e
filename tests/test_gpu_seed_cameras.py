"""svo_hip_seed_batch_update_cameras_async: the seed batches of SEVERAL cameras -- each with its own current frame, pose and
keyframe flag -- through one set of launches over a job table in device memory.  The reference is the existing pass per camera
(svo_hip_seed_batch_update_group_async in the six-launch form) on twin batches: events, status counts, status(), every array of
download() and n_alive() equal BYTES per batch over three frames, in both forms of the new call, and equal again when a camera
goes through the new call alone.  The first frame is also held against the CPU oracle.  The cameras' scenes differ enough for a
wrong current slot to show in the statuses (tests/test_df_cameras_inputs_cpu.py).

Both forms for every arrangement, with one limit the interface sets: the two-launch form takes at most 16 384 records
(svo_hip_df_set_small_pass_limit), and the 70 jobs of `seventy_small_jobs` are 70 x 256 = 17 920, so that arrangement runs the
six-launch form under both values of FORMS.  `sixty_one_block_jobs` (60 jobs, 15 360 records) is the largest job count the
two-launch kernels can see, and they see it."""
import dataclasses

import numpy as np
import pytest

import df_cameras_case as dc
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
        self.cams = dc.cameras(arr)
        self.cam = self.cams[0].cam
        n, self.K = len(self.cams), max(1, max(len(z) for z in arr.sizes))
        self.kf = hip.Pyramid(ctx, dc.WIDTH, dc.HEIGHT, dc.LEVELS, n * self.K)
        self.cf = hip.Pyramid(ctx, dc.WIDTH, dc.HEIGHT, dc.LEVELS, n)
        rev = arr.reversed_slots
        self.cur_slot = [n - 1 - c if rev else c for c in range(n)]
        self.ref_slots = [[c * self.K + (self.K - 1 - k if rev else k) for k in range(len(mk.keyframes))] for c, mk in enumerate(self.cams)]
        for c, mk in enumerate(self.cams):
            self.cf.upload(self.cur_slot[c], mk.cur_pyr)
            for k, sc in enumerate(mk.keyframes):
                self.kf.upload(self.ref_slots[c][k], sc.ref_pyr)
        self.T_refs = [np.stack([sc.T_ref_w for sc in mk.keyframes]) if mk.keyframes else np.zeros((0, 7)) for mk in self.cams]
        self.sets = []

    def erased(self, c, k):
        n = len(self.cams[c].keyframes[k].px)
        if self.arr.wholly_erased == (c, k):
            return np.arange(n)
        return np.arange(5, n, 7) if self.arr.erase_seventh else np.zeros(0, int)

    def twins(self):
        """a fresh set of the arrangement's batches: [camera][batch]"""
        s = []
        for c, mk in enumerate(self.cams):
            s.append([hip.ResidentSeeds(self.ctx, sc.px, sc.f, sc.level, sc.a, sc.b, sc.mu, sc.z_range, dc.sigma2_of(sc)) for sc in mk.keyframes])
            for k, rs in enumerate(s[-1]):
                if len(self.erased(c, k)):
                    rs.erase(self.erased(c, k))
        self.sets.append(s)
        return s

    def camera_pass(self, batches, c, keyframe):
        return (batches[c], self.ref_slots[c], self.T_refs[c], self.cur_slot[c], self.cams[c].T_cur_w, keyframe)

    def per_camera(self, batches, flags):
        """the reference: one grouped pass per camera, six-launch form"""
        self.ctx.set_small_pass_limit(0)
        for c, mk in enumerate(self.cams):
            if batches[c]:
                hip.ResidentSeeds.update_group_async(batches[c], self.kf, self.ref_slots[c], self.cf, self.cur_slot[c], self.cam, self.T_refs[c],
                                                     mk.T_cur_w, report_updated=flags[c])
        return [[rs.collect() for rs in cam] for cam in batches]

    def one_call(self, batches, flags, only=None):
        cams = range(len(self.cams)) if only is None else only
        hip.ResidentSeeds.update_cameras_async([self.camera_pass(batches, c, flags[c]) for c in cams], self.kf, self.cf, self.cam, ctx=self.ctx)

    def destroy(self):
        for s in self.sets:
            for cam in s:
                for rs in cam:
                    rs.destroy()
        self.kf.destroy(); self.cf.destroy()


def same_batch(got, want, got_out, want_out, where):
    assert np.array_equal(got_out[1], want_out[1]), where                       # status counts
    assert got_out[0].tobytes() == want_out[0].tobytes(), where                 # events
    assert got.status().tobytes() == want.status().tobytes(), where
    d, e = got.download(), want.download()
    assert sorted(d) == ["a", "alive", "b", "mu", "sigma2"]
    for key in d:
        assert d[key].tobytes() == e[key].tobytes(), (where, key)
    assert got.n_alive() == want.n_alive(), where


def state_of(batches):
    return [[(rs.status().tobytes(), {k: v.tobytes() for k, v in rs.download().items()}, rs.n_alive()) for rs in cam] for cam in batches]


@pytest.mark.parametrize("small_limit", FORMS)
@pytest.mark.parametrize("name", [a.name for a in dc.ARRANGEMENTS])
def test_one_call_for_all_cameras_equals_one_pass_per_camera(ctx, name, small_limit):
    arr = dc.BY_NAME[name]
    rig = Rig(ctx, arr)
    try:
        n_cams = len(rig.cams)
        want_b, got_b, alone_b = rig.twins(), rig.twins(), rig.twins()
        n_events = n_reported = 0
        for frame in range(3):
            flags = [frame == 1 and c in (0, 2) for c in range(n_cams)]        # on frame 1 cameras 0 and 2 are keyframes
            want = rig.per_camera(want_b, flags)
            ctx.set_small_pass_limit(small_limit)
            rig.one_call(got_b, flags)
            assert all(rs.pending() for cam in got_b for rs in cam)
            got = [[rs.collect() for rs in cam] for cam in got_b]
            alone = []
            for c in range(n_cams):                                            # every camera through the new call alone
                rig.one_call(alone_b, flags, only=[c])
                alone.append([rs.collect() for rs in alone_b[c]])
            for c in range(n_cams):
                for k in range(len(want_b[c])):
                    same_batch(got_b[c][k], want_b[c][k], got[c][k], want[c][k], (name, "all", frame, c, k))
                    same_batch(alone_b[c][k], want_b[c][k], alone[c][k], want[c][k], (name, "alone", frame, c, k))
                    n_events += len(got[c][k][0])
                    n_reported += int((got[c][k][0]["status"] == hip.SEED_UPDATED).sum())
                    if not flags[c]:
                        assert not (got[c][k][0]["status"] == hip.SEED_UPDATED).any()      # only a keyframe's camera reports updated seeds
            if frame == 0:
                _first_pass_against_the_oracle(rig, got_b, got, name)
        if arr.sizes[0] and arr.wholly_erased != (0, 0):
            assert n_events >= n_reported > 0                                  # camera 0's keyframe frame reported its updated seeds
    finally:
        rig.destroy()


def _first_pass_against_the_oracle(rig, batches, out, name):
    """as test_erased_seeds_are_left_alone_and_first_pass_matches_the_oracle: statuses equal, erased seeds untouched, mu equal
    for all but a few seeds in a thousand (over the arrangement: its batches go down to one seed)"""
    oracle = dc.oracle_first_pass(name)
    n_same = n_all = 0
    for c, mk in enumerate(rig.cams):
        for k, sc in enumerate(mk.keyframes):
            o, erased = oracle[c][k], rig.erased(c, k)
            keep = np.ones(len(sc.px), bool)
            keep[erased] = False
            st, d = batches[c][k].status(), batches[c][k].download()
            assert (st[erased] == hip.SEED_ERASED).all() and out[c][k][1][0] == len(erased), (name, c, k)
            assert np.array_equal(st[keep], o["status"][keep]), (name, c, k)
            assert np.array_equal(d["mu"][erased], sc.mu[erased]) and np.array_equal(d["sigma2"][erased], dc.sigma2_of(sc)[erased])
            assert not np.isin(out[c][k][0]["index"], erased).any()
            n_same += int((d["mu"][keep] == o["mu"][keep]).sum())
            n_all += int(keep.sum())
    assert n_same >= 0.995 * n_all, (name, n_same, n_all)


@pytest.fixture()
def small_rig(ctx):
    rig = Rig(ctx, dc.BY_NAME["shared_keyframe_batch"])
    yield rig
    rig.destroy()


def test_two_calls_back_to_back_for_disjoint_batches(ctx, small_rig):
    """nothing is collected between the calls: the second must not rewrite the first one's table while it is in flight"""
    rig = small_rig
    want_b, got_b = rig.twins(), rig.twins()
    for small_limit in FORMS:
        for frame in range(2):
            flags = [frame == 1, False]
            want = rig.per_camera(want_b, flags)
            ctx.set_small_pass_limit(small_limit)
            rig.one_call(got_b, flags, only=[1])
            rig.one_call(got_b, flags, only=[0])
            assert all(rs.pending() for cam in got_b for rs in cam)
            got = [[rs.collect() for rs in cam] for cam in got_b]
            for c in range(2):
                for k in range(len(want_b[c])):
                    same_batch(got_b[c][k], want_b[c][k], got[c][k], want[c][k], (small_limit, frame, c, k))


@pytest.mark.parametrize("case", ["pending", "named_twice", "cur_slot", "ref_slot", "other_context", "image_size"])
def test_refusals_leave_everything_as_it_was(ctx, small_rig, case):
    rig = small_rig
    b = rig.twins()
    before = state_of(b)
    passes = [list(rig.camera_pass(b, c, False)) for c in range(2)]
    cam, other, pending = rig.cam, None, None
    if case == "pending":
        pending = b[1][1]
        pending.update_async(rig.kf, rig.ref_slots[1][1], rig.cf, rig.cur_slot[1], rig.cam, rig.T_refs[1][1], rig.cams[1].T_cur_w)
    elif case == "named_twice":
        passes[1][0] = [b[1][0], b[0][1]]                                       # camera 0's second batch also under camera 1
    elif case == "cur_slot":
        passes[1][3] = rig.cf.batch
    elif case == "ref_slot":
        passes[0][1] = [rig.ref_slots[0][0], rig.kf.batch]
    elif case == "other_context":
        other = hip.Context(0)
        sc = rig.cams[1].keyframes[0]
        foreign = hip.ResidentSeeds(other, sc.px, sc.f, sc.level, sc.a, sc.b, sc.mu, sc.z_range, dc.sigma2_of(sc))
        passes[1][0] = [foreign, b[1][1]]
    elif case == "image_size":
        cam = dataclasses.replace(rig.cam, width=rig.cam.width + 16)
    with pytest.raises(hip.SvoHipError) as err:
        hip.ResidentSeeds.update_cameras_async([tuple(p) for p in passes], rig.kf, rig.cf, cam, ctx=ctx)
    assert "(%d)" % (-4 if case == "pending" else -1) in str(err.value), str(err.value)     # SVO_HIP_ERR_STATE / SVO_HIP_ERR_INVALID
    assert [rs.pending() for camb in b for rs in camb] == [rs is pending for camb in b for rs in camb]
    if pending is not None:                                                     # (its own pass, enqueued before, is not the call's doing)
        pending.collect()
        after = state_of(b)
        after[1][1] = before[1][1]
    else:
        after = state_of(b)
    assert after == before
    if other is not None:
        foreign.destroy()
        other.close()
    # ... and the same batches are accepted by a well-formed call afterwards
    hip.ResidentSeeds.update_cameras_async([rig.camera_pass(b, 0, False)], rig.kf, rig.cf, rig.cam, ctx=ctx)
    for rs in b[0]:
        rs.collect()


def test_error_codes(ctx, small_rig):
    """SVO_HIP_ERR_STATE for a batch whose pass is not collected, SVO_HIP_ERR_INVALID for a null argument; no batch at all is
    SVO_HIP_OK without a launch"""
    import ctypes as C
    rig = small_rig
    b = rig.twins()
    lib = ctx.lib
    ccam, prm = hip.make_camera(rig.cam), hip.depth_filter_params()
    one = (hip.CSeedCameraPass * 1)()
    assert lib.svo_hip_seed_batch_update_cameras_async(ctx.h, 1, one, rig.kf.h, rig.cf.h, C.byref(ccam), C.byref(prm)) == 0     # n_batches 0
    assert lib.svo_hip_seed_batch_update_cameras_async(ctx.h, 0, one, rig.kf.h, rig.cf.h, C.byref(ccam), C.byref(prm)) == 0
    assert lib.svo_hip_seed_batch_update_cameras_async(ctx.h, 1, None, rig.kf.h, rig.cf.h, C.byref(ccam), C.byref(prm)) == -1
    assert lib.svo_hip_seed_batch_update_cameras_async(ctx.h, 1, one, None, rig.cf.h, C.byref(ccam), C.byref(prm)) == -1
    assert lib.svo_hip_seed_batch_update_cameras_async(None, 1, one, rig.kf.h, rig.cf.h, C.byref(ccam), C.byref(prm)) == -1
    assert not any(rs.pending() for camb in b for rs in camb)
    rig.one_call(b, [False, False], only=[0])
    with pytest.raises(hip.SvoHipError, match=r"\(-4\)"):
        rig.one_call(b, [False, False])
    assert [rs.pending() for rs in b[1]] == [False, False]
    for rs in b[0]:
        rs.collect()


def test_1024_jobs_are_taken_and_1025_refused():
    """a context of its own: 1025 one-seed batches under one camera"""
    ctx = hip.Context(0)
    arr = dc.BY_NAME["shared_keyframe_batch"]
    mk = dc.cameras(arr)[0]
    sc = mk.keyframes[0]
    kf = hip.Pyramid(ctx, dc.WIDTH, dc.HEIGHT, dc.LEVELS, 1)
    cf = hip.Pyramid(ctx, dc.WIDTH, dc.HEIGHT, dc.LEVELS, 1)
    kf.upload(0, sc.ref_pyr)
    cf.upload(0, mk.cur_pyr)
    s2 = dc.sigma2_of(sc)
    i = int(np.nonzero(dc.oracle_first_pass(arr.name)[0][0]["status"] == hip.SEED_UPDATED)[0][0])       # a seed the pass updates and keeps
    one = slice(i, i + 1)
    bs = [hip.ResidentSeeds(ctx, sc.px[one], sc.f[one], sc.level[one], sc.a[one], sc.b[one], sc.mu[one], sc.z_range[one], s2[one]) for _ in range(1025)]
    T = np.tile(sc.T_ref_w, (1025, 1))
    with pytest.raises(hip.SvoHipError):
        hip.ResidentSeeds.update_cameras_async([(bs, [0] * 1025, T, 0, mk.T_cur_w, False)], kf, cf, mk.cam)
    assert not any(rs.pending() for rs in bs)
    assert all((rs.status() == hip.SEED_ERASED).all() for rs in bs[::64])        # no pass yet
    hip.ResidentSeeds.update_cameras_async([(bs[:512], [0] * 512, T[:512], 0, mk.T_cur_w, False),
                                            (bs[512:1024], [0] * 512, T[512:1024], 0, mk.T_cur_w, True)], kf, cf, mk.cam)
    out = [rs.collect() for rs in bs[:1024]]
    want = dc.oracle_first_pass(arr.name)[0][0]["status"][i]
    assert all(rs.status()[0] == want for rs in bs[:1024])
    assert all(len(o[0]) == (1 if k >= 512 else 0) for k, o in enumerate(out))   # the second camera's frame is a keyframe
    assert not bs[1024].pending()
    for rs in bs:
        rs.destroy()
    kf.destroy(); cf.destroy()
    ctx.close()


def test_ten_warm_calls_make_no_allocator_call(ctx):
    rig = Rig(ctx, dc.BY_NAME["nine_cameras_two_batches"])
    try:
        b = rig.twins()
        flags = [False] * len(rig.cams)
        for small_limit in FORMS:
            ctx.set_small_pass_limit(small_limit)
            rig.one_call(b, flags)                                             # the warm-up call
            [rs.collect() for cam in b for rs in cam]
            before = ctx.info()
            for _ in range(10):
                rig.one_call(b, flags)
                [rs.collect() for cam in b for rs in cam]
            after = ctx.info()
            assert after["allocator_calls"] == before["allocator_calls"] and after["free_calls"] == before["free_calls"], (before, after)
    finally:
        rig.destroy()


def test_mark_updated_behind_a_cameras_pass(ctx, small_rig):
    """svo_hip_seed_batch_mark_updated reads status and px_cur of the batches: the grid after a pass of all cameras is the grid
    after the passes per camera"""
    rig = small_rig
    want_b = rig.twins()
    flags = [True, True]
    def marked(enqueue, batches):
        """the grids of the two cameras, the marks enqueued BEHIND the pass while it is still pending (what the mirror does:
        stream order, no wait in between), the collects afterwards"""
        enqueue()
        assert all(rs.pending() for cam in batches for rs in cam)
        gs = [hip.DetectorGrid(ctx, dc.WIDTH, dc.HEIGHT, 10) for _ in range(2)]
        for c in range(2):
            gs[c].mark_updated(batches[c])
        assert all(rs.pending() for cam in batches for rs in cam)
        [rs.collect() for cam in batches for rs in cam]
        ctx.sync()
        out = [g.download() for g in gs]
        [g.free() for g in gs]
        return out

    def per_camera_async():
        ctx.set_small_pass_limit(0)
        for c in range(2):
            hip.ResidentSeeds.update_group_async(want_b[c], rig.kf, rig.ref_slots[c], rig.cf, rig.cur_slot[c], rig.cam, rig.T_refs[c],
                                                 rig.cams[c].T_cur_w, report_updated=True)
    grids = [marked(per_camera_async, want_b)]
    for small_limit in FORMS:
        twins = rig.twins()
        ctx.set_small_pass_limit(small_limit)
        grids.append(marked(lambda: rig.one_call(twins, flags), twins))
    for c in range(2):
        assert grids[0][c].tobytes() == grids[2][c].tobytes()
    for c in range(2):
        assert grids[0][c].any() and grids[0][c].tobytes() == grids[1][c].tobytes()
    assert grids[0][0].tobytes() != grids[0][1].tobytes()                       # the cameras see different scenes
