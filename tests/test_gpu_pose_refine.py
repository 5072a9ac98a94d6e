"""pose_refine_kernel (android_svo_amd/csrc/svo_refine.hip) in every size class, through every exit and with medians inside
runs of equal keys, against the extended-precision reference of tests/pose_reference.py; batches of all classes at once
against the same frames run alone, bit for bit; and point_refine_kernel at its block boundaries.
tests/test_oracle_pose_reference.py proves on the CPU that the inputs reach the regimes they are named for, that no case
is excluded as undecidable, and that the assertions used here reject a dropped inlier, a feature of the neighbouring slot
and the lower median.

Every case: ran, estimated_scale (bit-equal to the reference; the perfect-data case excepted), the slots without a point
untouched, num_obs + n_deleted == n_obs.  Well-posed cases: n_iter_done and every outlier decision equal to the
reference's, and the distance of pose, error_init, error_final and Cov to the reference within
MARGIN (8) x max(the oracle's largest distance to the same reference over the family, 2^-50), computed from the oracle
where the test runs.  Largest distances per family (pose in rad / m, the others relative; "-" = not compared):

                oracle (CPU)                                          kernel (MI355X)
  family        rot      trans    e_init   e_final  cov               rot      trans    e_init   e_final  cov
  classes       1.5e-16  2.1e-16  2.0e-14  1.0e-13  2.8e-14           6.7e-17  1.3e-16  2.0e-14  1.0e-13  4.9e-15
  class_count   6.3e-17  2.6e-16  2.0e-14  7.6e-14  1.7e-14           6.2e-17  1.1e-16  2.0e-14  7.6e-14  1.9e-15
  ties          4.2e-17  1.4e-16  8.4e-15  1.5e-13  3.7e-14           6.4e-17  1.4e-16  8.4e-15  1.1e-13  2.2e-15
  threshold     3.6e-17  1.2e-16  1.1e-14  6.1e-15  1.1e-14           3.7e-17  1.0e-16  1.1e-14  1.2e-14  2.5e-15
  exits         1.2e-16  2.8e-16  2.6e-15  7.2e-14  1.2e-14           1.3e-16  4.2e-16  2.6e-15  2.9e-14  9.0e-15
  large_steps   4.2e-17  7.5e-17  3.0e-16  1.8e-13  1.3e-14           4.9e-17  1.3e-16  3.0e-16  2.1e-13  4.2e-15
  perfect       2.2e-17  4.8e-17  -        -        -                 2.2e-17  4.8e-17  -        -        -"""
import ctypes as C

import numpy as np
import pytest

from android_svo_amd import hip, synth
from oracle import orc

import pose_reference as pr

pytestmark = pytest.mark.gpu

PAD = 64                                         # guard elements behind every array of a padded launch
RES_BYTES = C.sizeof(hip.CPoseOptResult)


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


def gpu_alone(ctx, c):
    r, hp = hip.pose_optimize(ctx, c.T_f_w_init, c.f, c.pos, c.level, c.has_point, pr.EM, reproj_thresh=c.reproj_thresh, n_iter=c.n_iter)
    return r, hp


def record_bits(r):
    """every field of a result record as integers (NaNs compare by their bits); the padding word is not a result"""
    d = lambda v: np.array(v, dtype=np.float64).reshape(-1).view(np.uint64).tolist()
    return (r.ran, r.n_iter_done, r.n_deleted, int(r.num_obs), d(r.T_f_w), d(r.estimated_scale), d(r.error_init), d(r.error_final), d(r.Cov))


# ---- one frame per launch, every family ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pr.FAMILIES))
def test_family_against_the_extended_reference(ctx, name):
    cases, refs = pr.family(name)
    orcs = pr.oracle_family(name)
    bounds = pr.family_bounds(cases, refs, orcs)
    got = []
    for c in cases:
        r, hp = gpu_alone(ctx, c)
        got.append(pr.Result.of(r, hp))
    worst = pr.family_distances(cases, refs, got)
    print("\n%-12s kernel " % name + " ".join("%s %.1e" % (k, worst[k]) for k in pr.QUANTITIES if k in worst))
    print("%-12s bound  " % name + " ".join("%s %.1e" % (k, bounds[k]) for k in pr.QUANTITIES if k in bounds))
    for c, r, g, o in zip(cases, refs, got, orcs):
        pr.check_all(c, r, g, bounds, o)


def test_run_to_run_bit_equality(ctx):
    """the header comment's claim: the same frame twice gives the same bits (tree-ordered sums, no atomics on data)"""
    for c in pr.family("classes")[0][-4:] + pr.family("ties")[0][1:3]:
        a, hp_a = gpu_alone(ctx, c)
        b, hp_b = gpu_alone(ctx, c)
        assert record_bits(a) == record_bits(b) and np.array_equal(hp_a, hp_b), c.name


# ---- batches ---------------------------------------------------------------------------------------------------------
BATCH_MAX_N = 2400
BATCH_SIZES = (2305, 7, 256, 257, 64, 2049)
PADDINGS = (dict(f=-9.87654321e99, level=0x5A5A5A5A, has_point=0xA5),
            dict(f=np.nan, level=31, has_point=1))          # a row read past n_k would count these as observations


def batch_frames():
    cases = {len(c.level): c for c in pr.family("classes")[0] if "null_every=11" in c.name}
    frames = [cases[n] for n in BATCH_SIZES]
    empty = synth.make_pose_opt_case(seed=300, n=100)
    empty.has_point[:] = 0
    frames.append(pr.Case("batch frame without any point", empty.T_f_w_init, empty.f, empty.pos, empty.level, empty.has_point))
    frames.append(pr.Case("batch frame with n = 0", cases[64].T_f_w_init, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0, np.int32),
                          np.zeros(0, np.uint8)))
    return frames


def batch_padded(ctx, frames, max_n, padding):
    """svo_hip_pose_optimize_batch_dev with everything beyond n_k in every row, PAD elements behind every array and one
    record behind the results filled with sentinels; asserts that all of them come back unchanged; returns (records,
    has_point rows cut to n_k)"""
    B = len(frames)
    f = np.full((B * max_n + PAD, 3), padding["f"])
    pos = np.full((B * max_n + PAD, 3), padding["f"])
    lvl = np.full(B * max_n + PAD, padding["level"], dtype=np.int32)
    hp = np.full(B * max_n + PAD, padding["has_point"], dtype=np.uint8)
    T = np.full((B + 1, 7), padding["f"])
    nf = np.full(B + PAD, 12345, dtype=np.int32)
    for k, c in enumerate(frames):
        n = len(c.level)
        sl = slice(k * max_n, k * max_n + n)
        f[sl], pos[sl], lvl[sl], hp[sl], T[k], nf[k] = c.f, c.pos, c.level, c.has_point, c.T_f_w_init, n
    res = np.full((B + 1) * RES_BYTES, 0xC3, dtype=np.uint8)
    host = [T, f, pos, lvl, hp, nf, res]
    d = [ctx.to_device(v) for v in host]
    ctx.check(ctx.lib.svo_hip_pose_optimize_batch_dev(
        ctx.h, B, max_n, C.c_void_p(d[5].ptr), C.c_void_p(d[0].ptr), C.c_void_p(d[1].ptr), C.c_void_p(d[2].ptr), C.c_void_p(d[3].ptr),
        C.c_void_p(d[4].ptr), C.c_double(pr.EM), C.c_double(2.0), 10, C.c_void_p(d[6].ptr)), "pose_optimize_batch")
    back = [v.download() for v in d]
    for v in d:
        v.free()
    for name, h, b in zip(("T_f_w", "f", "pos", "level", "n_feat"), (T, f, pos, lvl, nf), (back[0], back[1], back[2], back[3], back[5])):
        assert h.tobytes() == b.tobytes(), "input %s was written" % name
    hp_back, res_back = back[4], back[6]
    rows = []
    for k, c in enumerate(frames):
        n = len(c.level)
        assert (hp_back[k * max_n + n:(k + 1) * max_n] == padding["has_point"]).all(), "has_point[%d, n_k:] was written" % k
        rows.append(hp_back[k * max_n:k * max_n + n].copy())
    assert (hp_back[B * max_n:] == padding["has_point"]).all(), "guard behind has_point was written"
    assert (res_back[B * RES_BYTES:] == 0xC3).all(), "guard record behind the results was written"
    recs = [hip.CPoseOptResult.from_buffer_copy(res_back[k * RES_BYTES:(k + 1) * RES_BYTES].tobytes()) for k in range(B)]
    return recs, rows


@pytest.fixture(scope="module")
def alone(ctx):
    frames = batch_frames()
    return frames, [gpu_alone(ctx, c) for c in frames]


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_batch_of_all_classes_equals_the_frames_run_alone(ctx, alone, order):
    """One launch with every class (the workspace path in slot 0 and in slot B - 1 / 5), a frame without any point and one
    with n = 0: every record, Cov included, and every has_point row bit-equal to the frame run alone, whatever lies in the
    padding behind the rows."""
    frames, singles = alone
    idx = list(range(len(frames)))
    if order == "reversed":
        idx.reverse()
    runs = [batch_padded(ctx, [frames[i] for i in idx], BATCH_MAX_N, p) for p in PADDINGS]
    for recs, rows in runs:
        for slot, i in enumerate(idx):
            r1, hp1 = singles[i]
            assert record_bits(recs[slot]) == record_bits(r1), (order, slot, frames[i].name)
            assert np.array_equal(rows[slot], hp1), (order, slot, frames[i].name)
    for c, (r1, hp1) in zip(frames[-2:], singles[-2:]):
        assert r1.ran == 0 and list(r1.T_f_w) == list(c.T_f_w_init) and not hp1.any()


def test_batch_through_the_python_entry(ctx, alone):
    """hip.pose_optimize_batch (zero padding) gives the same records"""
    frames, singles = alone
    B = len(frames)
    T = np.zeros((B, 7)); f = np.zeros((B, BATCH_MAX_N, 3)); pos = np.zeros((B, BATCH_MAX_N, 3))
    f[..., 2] = 1.0
    lvl = np.zeros((B, BATCH_MAX_N), dtype=np.int32); hp = np.zeros((B, BATCH_MAX_N), dtype=np.uint8); nf = np.zeros(B, dtype=np.int32)
    for k, c in enumerate(frames):
        n = len(c.level)
        T[k], f[k, :n], pos[k, :n], lvl[k, :n], hp[k, :n], nf[k] = c.T_f_w_init, c.f, c.pos, c.level, c.has_point, n
    res, hp_out = hip.pose_optimize_batch(ctx, T, f, pos, lvl, hp, nf, pr.EM)
    for k, (c, (r1, hp1)) in enumerate(zip(frames, singles)):
        assert record_bits(res[k]) == record_bits(r1), c.name
        assert np.array_equal(hp_out[k, :len(c.level)], hp1) and not hp_out[k, len(c.level):].any(), c.name


# ---- point_refine_kernel: one lane per point, 64-lane blocks -----------------------------------------------------------
@pytest.mark.parametrize("n_points", [63, 64, 65, 129])
def test_point_refine_at_block_boundaries(ctx, n_points):
    """Launches that end just before, at and just behind a block boundary, a point without any observation between two
    normal ones, guard elements behind pos and iters: bit-equal to the oracle's Point::optimize."""
    pos0, off, Ts, fs, _, _ = synth.make_point_opt_cases(seed=60 + n_points, n_points=n_points)
    hole = n_points // 2                                     # obs_offset[hole] == obs_offset[hole + 1]
    keep = np.ones(len(Ts), bool)
    keep[off[hole]:off[hole + 1]] = False
    cnt = np.diff(off)
    cnt[hole] = 0
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    Ts, fs = np.ascontiguousarray(Ts[keep]), np.ascontiguousarray(fs[keep])
    sent_p, sent_i = -9.87654321e99, -77
    p = np.full((n_points + PAD, 3), sent_p)
    p[:n_points] = pos0
    dp, di = ctx.to_device(p), ctx.to_device(np.full(n_points + PAD, sent_i, dtype=np.int32))
    do, dT, dF = ctx.to_device(off), ctx.to_device(Ts), ctx.to_device(fs)
    ctx.check(ctx.lib.svo_hip_point_optimize_batch_dev(ctx.h, n_points, 8, C.c_void_p(dp.ptr), C.c_void_p(do.ptr), C.c_void_p(dT.ptr),
                                                       C.c_void_p(dF.ptr), C.c_void_p(di.ptr)), "point_optimize_batch")
    out, it = dp.download(), di.download()
    same_inputs = do.download().tobytes() == off.tobytes() and dT.download().tobytes() == Ts.tobytes() and dF.download().tobytes() == fs.tobytes()
    for v in (dp, di, do, dT, dF):
        v.free()
    assert same_inputs
    assert (out[n_points:] == sent_p).all() and (it[n_points:] == sent_i).all(), "guard elements were written"
    for k in range(n_points):
        want, it_o = orc.point_optimize(pos0[k], Ts[off[k]:off[k + 1]], fs[off[k]:off[k + 1]], n_iter=8)
        assert out[k].tobytes() == want.tobytes() and it[k] == it_o, (k, out[k], want, it[k], it_o)
    assert it[hole] == 1 and out[hole].tobytes() == pos0[hole].tobytes()      # no observation: a zero step, taken once
