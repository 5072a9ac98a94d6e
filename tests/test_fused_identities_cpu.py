"""The two exact identities the fused SparseImgAlign kernel's tile loop rests on, checked bit for bit in numpy (IEEE
arithmetic, one rounding per operation, no fused multiply-add: what the library's -ffp-contract=off code does).

1. cross(2 q, p) == 2 cross(q, p): se3_act_q2 (svo_device_math.h) takes the doubled vector part of the pose quaternion,
   formed once per evaluation, instead of doubling q x p for every patch.  A factor of two commutes with every product and
   every difference as long as nothing overflows or turns subnormal.
2. (0.5f a) b == 0.5f (a b): lpp_project and fused_ref_weights (svo_sia.hip) halve one factor of the four interpolation
   weights instead of the four products.  The factors are sub-pixel fractions of positions >= 3 and their complements to
   one: multiples of 2^-22 in [0, 1]."""
import numpy as np


def _cross(a, b):
    """cross3 of svo_device_math.h: a product, a product, a difference per component"""
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                     a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _quaternions_and_points():
    rng = np.random.default_rng(20240917)
    n = 100000
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    # and unit quaternions of small rotations, as between two consecutive frames
    v = rng.normal(size=(20000, 3))
    v *= (10.0 ** rng.uniform(-6, -1, size=(20000, 1))) / np.linalg.norm(v, axis=1, keepdims=True)
    small = np.concatenate([v, np.sqrt(1.0 - (v * v).sum(axis=1, keepdims=True))], axis=1)
    p_small = rng.normal(size=(20000, 3)) * 10.0 ** rng.uniform(-3, 3, size=(20000, 1))
    p = rng.normal(size=(n, 3))
    p *= (10.0 ** rng.uniform(-3, 3, size=(n, 1))) / np.linalg.norm(p, axis=1, keepdims=True)
    # axis-aligned quaternions and points, zero components (of either sign), in every combination
    axes = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1], [0, 0, 0], [-0.0, 0.0, -0.0],
                     [1, 1, 0], [0, 1, -1], [1, 0, 1]], dtype=np.float64)
    qa = np.repeat(axes, len(axes), axis=0)
    pa = np.tile(axes, (len(axes), 1))
    scales = np.array([1e-3, 1.0, 1e3])
    qs = np.concatenate([q[:, :3]] + [qa * np.sqrt(0.5)] * len(scales) + [qa] * len(scales))
    ps = np.concatenate([p] + [pa * s for s in scales] * 2)
    # some random cases with single components zeroed
    m = 3000
    qz, pz = q[:m, :3].copy(), p[:m].copy()
    qz[np.arange(m), rng.integers(0, 3, m)] = 0.0
    pz[np.arange(m), rng.integers(0, 3, m)] = 0.0
    return np.concatenate([qs, qz, q[:m, :3], small[:, :3]]), np.concatenate([ps, p[:m], pz, p_small])


def test_cross_of_the_doubled_quaternion_is_the_doubled_cross():
    q, p = _quaternions_and_points()
    assert q.dtype == np.float64 and p.dtype == np.float64 and len(q) == len(p) > 100000
    norms = np.linalg.norm(p[:100000], axis=1)
    assert norms.min() < 2e-3 and norms.max() > 5e2
    q2 = q + q                                                     # as the kernel forms it
    got = _cross(q2, p)
    c = _cross(q, p)
    want = c + c                                                   # so3_rotate: uv = uv + uv
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))          # bit for bit, signed zeros included
    assert np.array_equal(q2.view(np.uint64), (2.0 * q).view(np.uint64))


def _fractions():
    """2^10 multiples of 2^-22 in [0, 1): the ends, the neighbours of the powers of two, and random ones"""
    rng = np.random.default_rng(7)
    k = [0, 1, 2, 3, (1 << 22) - 1, (1 << 22) - 2, 1 << 21, (1 << 21) - 1, (1 << 21) + 1]
    for e in range(1, 21):
        k += [1 << e, (1 << e) + 1, (1 << e) - 1]
    k = sorted(set(k))
    more = [int(v) for v in dict.fromkeys(rng.integers(0, 1 << 22, size=4096).tolist()) if v not in set(k)]
    k = np.array(k + more[: 1024 - len(k)], dtype=np.int64)
    assert len(k) == 1024 and len(set(k.tolist())) == 1024
    return (k.astype(np.float64) * 2.0 ** -22).astype(np.float32)


def test_halving_one_factor_is_halving_the_product():
    f = _fractions()
    assert f.dtype == np.float32 and f[0] == 0.0 and np.float32(1.0 - 2.0 ** -22) in f
    assert np.array_equal(f.astype(np.float64) * 2.0 ** 22, np.round(f.astype(np.float64) * 2.0 ** 22))
    half = np.float32(0.5)
    one = np.float32(1.0)
    # the factors of the four weights: su, 1 - su (exact in f32: a multiple of 2^-22 in (0, 1]) on one axis, sv, 1 - sv on the other
    for a in (f, one - f):
        for b in (f, one - f):
            A, B = a[:, None], b[None, :]                         # all pairs
            got = (half * A) * B
            want = half * (A * B)
            assert got.dtype == np.float32 and got.shape == (1024, 1024)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(((one - f).astype(np.float64)), 1.0 - f.astype(np.float64))     # 1 - su is exact
