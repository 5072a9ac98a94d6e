"""The bootstrap's two-view stage restated in numpy: the definition the kernels of csrc/svo_two_view_impl.h are held to by bits.

KltHomographyInit::addSecondFrame from the call of computeFundamental to the creation of the points
(S/initialization.cpp:77-138, 260-329).  cv::findFundamentalMat(FM_RANSAC) and cv::recoverPose are OpenCV code that is not in
the reference's tree; they get a written definition here (DESIGN.md section 7 lists the departures).  From (R, t) on it is the
reference's own arithmetic restated line by line: vk::computeInliers, Quaterniond(R), the depth median, the SE3 products.

Everything is scalar f64 with every operation rounded on its own: numpy expressions are elementwise (no np.sum, no np.dot
-- every sum is written out in its order), the scalar stages use Python floats and math.sqrt.  One function per stage.
"""
import math

import numpy as np

OK, TOO_FEW, NO_MODEL, CHEIRALITY, FEW_INLIERS = range(5)
STATUS_NAMES = ["OK", "TOO_FEW", "NO_MODEL", "CHEIRALITY", "FEW_INLIERS"]
MAX_HYPOTHESES = 4096
SVD_SWEEPS = 12
SQRT2 = 1.4142135623730951
NAN = float("nan")
IDENTITY = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
U64 = np.uint64


def default_params():
    return dict(reproj_thresh=2.0, min_inliers=40, map_scale=1.0, n_hypotheses=1024, seed=0)


# ---- normalised coordinates: vk::project2d rounded as cv::Point2f rounds it (:274-278) ---------------------------------
def normalised(f_ref, f_cur):
    """[n][4] f32: x_ref, y_ref, x_cur, y_cur."""
    f_ref, f_cur = np.asarray(f_ref, np.float64).reshape(-1, 3), np.asarray(f_cur, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.stack([f_ref[:, 0] / f_ref[:, 2], f_ref[:, 1] / f_ref[:, 2], f_cur[:, 0] / f_cur[:, 2], f_cur[:, 1] / f_cur[:, 2]],
                        axis=1).astype(np.float32)


# ---- sampling --------------------------------------------------------------------------------------------------------
def _mix(seed, h, k):
    with np.errstate(over="ignore"):
        z = U64(seed & 0xFFFFFFFFFFFFFFFF) * U64(0x9E3779B97F4A7C15) + h.astype(U64) * U64(0xBF58476D1CE4E5B9) + U64(k) * U64(0x94D049BB133111EB)
        z = z ^ (z >> U64(30)); z = z * U64(0xBF58476D1CE4E5B9)
        z = z ^ (z >> U64(27)); z = z * U64(0x94D049BB133111EB)
        z = z ^ (z >> U64(31))
    return z


def sample(seed, n_hypotheses, n):
    """[H][8] ascending: draw k of hypothesis h is a function of (seed, h, k, n) alone.  The upper word of a 64-bit mix is scaled
    to the n - k positions still free and shifted past the earlier picks in ascending order; exactly 8 draws, no rejection."""
    h = np.arange(n_hypotheses, dtype=np.int64)
    s = np.zeros((n_hypotheses, 8), dtype=np.int64)
    for k in range(8):
        r = _mix(seed, h, k) >> U64(32)
        v = ((r * U64(n - k)) >> U64(32)).astype(np.int64)
        for i in range(k):
            v = v + (v >= s[:, i])
        s[:, k] = v
        s[:, :k + 1] = np.sort(s[:, :k + 1], axis=1)
    return s


# ---- one hypothesis (vectorised over hypotheses; every operation elementwise) ------------------------------------------
def solve_hypotheses(xy, samples):
    """Hartley normalisation, the 8 x 9 system x_cur^T F x_ref = 0, its null vector by Gaussian elimination with complete
    pivoting (first maximum in row-major order), de-normalisation.  -> (F [H][9] row-major, valid [H]).  F is NOT projected to
    rank 2 before scoring."""
    H = len(samples)
    p = xy[samples].astype(np.float64)                    # [H][8][4]
    idx = np.arange(H)
    with np.errstate(all="ignore"):
        c = np.zeros((H, 4))
        for i in range(8):
            c = c + p[:, i, :]
        c = c * 0.125
        d1, d2 = np.zeros(H), np.zeros(H)
        for i in range(8):
            ax, ay = p[:, i, 0] - c[:, 0], p[:, i, 1] - c[:, 1]
            bx, by = p[:, i, 2] - c[:, 2], p[:, i, 3] - c[:, 3]
            d1 = d1 + np.sqrt(ax * ax + ay * ay)
            d2 = d2 + np.sqrt(bx * bx + by * by)
        d1, d2 = d1 * 0.125, d2 * 0.125
        valid = (d1 > 0) & (d1 < np.inf) & (d2 > 0) & (d2 < np.inf)
        s1, s2 = SQRT2 / d1, SQRT2 / d2
        A = np.zeros((H, 8, 9))
        for i in range(8):
            u1, v1 = (p[:, i, 0] - c[:, 0]) * s1, (p[:, i, 1] - c[:, 1]) * s1
            u2, v2 = (p[:, i, 2] - c[:, 2]) * s2, (p[:, i, 3] - c[:, 3]) * s2
            A[:, i, 0], A[:, i, 1], A[:, i, 2] = u2 * u1, u2 * v1, u2
            A[:, i, 3], A[:, i, 4], A[:, i, 5] = v2 * u1, v2 * v1, v2
            A[:, i, 6], A[:, i, 7], A[:, i, 8] = u1, v1, 1.0
        perm = np.tile(np.arange(9), (H, 1))
        for k in range(8):
            best = np.full(H, -1.0)
            pr, pc = np.full(H, k), np.full(H, k)
            for r in range(k, 8):
                for cc in range(k, 9):
                    a = np.abs(A[:, r, cc])
                    up = a > best
                    best, pr, pc = np.where(up, a, best), np.where(up, r, pr), np.where(up, cc, pc)
            valid = valid & (best > 0) & (best < np.inf)
            t = A[idx, k, :].copy(); A[idx, k, :] = A[idx, pr, :]; A[idx, pr, :] = t
            t = A[idx, :, k].copy(); A[idx, :, k] = A[idx, :, pc]; A[idx, :, pc] = t
            t = perm[idx, k].copy(); perm[idx, k] = perm[idx, pc]; perm[idx, pc] = t
            piv = A[:, k, k]
            for r in range(k + 1, 8):
                m = A[:, r, k] / piv
                for cc in range(k + 1, 9):
                    A[:, r, cc] = A[:, r, cc] - m * A[:, k, cc]
        x = np.ones((H, 9))
        for k in range(7, -1, -1):
            s = A[:, k, 8].copy()
            for j in range(7, k, -1):
                s = s + A[:, k, j] * x[:, j]
            x[:, k] = -s / A[:, k, k]
        g = np.zeros((H, 9))
        for j in range(9):
            g[idx, perm[:, j]] = x[:, j]
        t1x, t1y, t2x, t2y = s1 * c[:, 0], s1 * c[:, 1], s2 * c[:, 2], s2 * c[:, 3]
        m = np.zeros((H, 9))
        for r in range(3):
            m[:, 3 * r] = g[:, 3 * r] * s1
            m[:, 3 * r + 1] = g[:, 3 * r + 1] * s1
            m[:, 3 * r + 2] = (g[:, 3 * r + 2] - g[:, 3 * r] * t1x) - g[:, 3 * r + 1] * t1y
        F = np.zeros((H, 9))
        for cc in range(3):
            F[:, cc] = s2 * m[:, cc]
            F[:, 3 + cc] = s2 * m[:, 3 + cc]
            F[:, 6 + cc] = (m[:, 6 + cc] - t2x * m[:, cc]) - t2y * m[:, 3 + cc]
    return F, valid


def thr2(reproj_thresh, error_multiplier2):
    t = float(reproj_thresh) / float(error_multiplier2)
    return t * t


def epi_inliers(F, xy, t2):
    """cv::findFundamentalMat's FM_RANSAC error, the larger of the two squared point-to-epipolar-line distances, against t2;
    a NaN is no inlier.  F [..., 9] broadcasts against the correspondences: -> flags [..., n]."""
    F = np.asarray(F, np.float64)[..., None, :]
    x1, y1, x2, y2 = (xy[:, i].astype(np.float64) for i in range(4))
    with np.errstate(all="ignore"):
        a = (F[..., 0] * x1 + F[..., 1] * y1) + F[..., 2]
        b = (F[..., 3] * x1 + F[..., 4] * y1) + F[..., 5]
        c = (F[..., 6] * x1 + F[..., 7] * y1) + F[..., 8]
        d2 = (x2 * a + y2 * b) + c
        e2 = (d2 * d2) * (1.0 / (a * a + b * b))
        a1 = (F[..., 0] * x2 + F[..., 3] * y2) + F[..., 6]
        b1 = (F[..., 1] * x2 + F[..., 4] * y2) + F[..., 7]
        c1 = (F[..., 2] * x2 + F[..., 5] * y2) + F[..., 8]
        d1 = (x1 * a1 + y1 * b1) + c1
        e1 = (d1 * d1) * (1.0 / (a1 * a1 + b1 * b1))
        return (e1 <= t2) & (e2 <= t2)


def score_hypotheses(F, valid, xy, t2, chunk=256):
    """the integer inlier count of every hypothesis, -1 for an invalid one"""
    counts = np.full(len(F), -1, dtype=np.int32)
    for h0 in range(0, len(F), chunk):
        counts[h0:h0 + chunk] = epi_inliers(F[h0:h0 + chunk], xy, t2).sum(axis=1)          # an integer count
    counts[~valid] = -1
    return counts


def winner(counts):
    """the highest count, the lowest index among equals; -1 when every hypothesis is invalid"""
    h = int(np.argmax(counts))
    return h if counts[h] >= 0 else -1


# ---- the scalar stages: Python floats -------------------------------------------------------------------------------------
# The orders of Eigen's compiled code, found against tests/golden/two_view_ref.npz (tests/test_two_view_golden_cpu.py).
# Vector3d::dot: a packet of two, then the third term -- (a0 + a1) + a2.  Matrix3d * Vector3d: rows 0 and 1 as one packet over
# the columns, (c0 v0 + c1 v1) + c2 v2; row 2 is the scalar unroller's a0 + (a1 + a2).  R.transpose() * v: the scalar unroller.
def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _matvec(R, v):
    return [_dot3(R[0:3], v), _dot3(R[3:6], v), R[6] * v[0] + (R[7] * v[1] + R[8] * v[2])]


def rotation_matrix(T):
    """row-major 3 x 3 of the rotation (I/SO3.h:391-406)"""
    x, y, z, w = T[3], T[4], T[5], T[6]
    x2, y2, z2 = x * x, y * y, z * z
    xy, xz, yz = x * y, x * z, y * z
    wx, wy, wz = w * x, w * y, w * z
    return [1.0 - 2.0 * (y2 + z2), 2.0 * (xy - wz), 2.0 * (xz + wy), 2.0 * (xy + wz), 1.0 - 2.0 * (x2 + z2), 2.0 * (yz - wx),
            2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (x2 + y2)]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _jacobi_pair(wp, wq, vp, vq):
    alpha, beta, gamma = _dot3(wp, wp), _dot3(wq, wq), _dot3(wp, wq)
    if not (gamma != 0.0):
        return
    zeta = _div(beta - alpha, 2.0 * gamma)
    root = _sqrt(1.0 + zeta * zeta)
    t = _div(1.0, zeta + root) if zeta >= 0.0 else _div(-1.0, root - zeta)
    c = _div(1.0, _sqrt(1.0 + t * t))
    s = c * t
    for i in range(3):
        a, b = wp[i], wq[i]
        wp[i], wq[i] = c * a - s * b, s * a + c * b
        e, f = vp[i], vq[i]
        vp[i], vq[i] = c * e - s * f, s * e + c * f


def _div(a, b):                                            # IEEE division: inf and NaN instead of an exception
    return float(np.float64(a) / np.float64(b)) if b == 0.0 or b != b else a / b


def _sqrt(a):
    return math.sqrt(a) if a >= 0.0 and a != math.inf else float(np.sqrt(np.float64(a)))


def decompose(F):
    """cv::recoverPose's role: one-sided Jacobi SVD of F (SVD_SWEEPS sweeps over the column pairs (0,1), (0,2), (1,2)), the two
    largest singular directions, u3 = u1 x u2, v3 = v1 x v2 (both factors have determinant +1; dropping the smallest singular
    value is the projection to rank 2).  -> (R1 = U W V^T, R2 = U W^T V^T, u3), rotations row-major lists of 9."""
    F = [float(v) for v in F]
    with np.errstate(all="ignore"):
        w = [[F[3 * i + j] for i in range(3)] for j in range(3)]          # column j
        v = [[1.0 if i == j else 0.0 for i in range(3)] for j in range(3)]
        for _ in range(SVD_SWEEPS):
            _jacobi_pair(w[0], w[1], v[0], v[1])
            _jacobi_pair(w[0], w[2], v[0], v[2])
            _jacobi_pair(w[1], w[2], v[1], v[2])
        sg = [_sqrt(_dot3(w[j], w[j])) for j in range(3)]
        for a, b in ((0, 1), (0, 2), (1, 2)):
            if sg[b] > sg[a]:
                w[a], w[b], v[a], v[b], sg[a], sg[b] = w[b], w[a], v[b], v[a], sg[b], sg[a]
        for j in range(2):
            w[j] = [_div(w[j][i], sg[j]) for i in range(3)]
        w[2], v[2] = _cross(w[0], w[1]), _cross(v[0], v[1])
        R1 = [(w[1][i] * v[0][j] - w[0][i] * v[1][j]) + w[2][i] * v[2][j] for i in range(3) for j in range(3)]
        R2 = [(w[0][i] * v[1][j] - w[1][i] * v[0][j]) + w[2][i] * v[2][j] for i in range(3) for j in range(3)]
    return R1, R2, list(w[2])


def candidate(c, R1, R2, u3):
    """candidate c of (R1, +u3), (R1, -u3), (R2, +u3), (R2, -u3)"""
    return (R1 if c < 2 else R2), ([-x for x in u3] if c & 1 else list(u3))


def triangulate(R, t, f_cur, f_ref):
    """vk::triangulateFeatureNonLin(R, t, feature1 = f_cur, feature2 = f_ref) (S/math_utils.cpp:15-32) for all correspondences:
    -> (lambda0, lambda1, xyz [n][3]).  A.inverse() is Eigen's 2 x 2 formula."""
    f1 = [f_cur[:, i] for i in range(3)]
    fr = [f_ref[:, i] for i in range(3)]
    with np.errstate(all="ignore"):
        f2 = _matvec(R, fr)
        b0, b1 = _dot3(t, f1), _dot3(t, f2)
        a00, a10 = _dot3(f1, f1), _dot3(f1, f2)
        a01, a11 = -a10, -_dot3(f2, f2)
        invdet = 1.0 / (a00 * a11 - a10 * a01)
        i00, i10, i01, i11 = a11 * invdet, -a10 * invdet, -a01 * invdet, a00 * invdet
        l0 = i00 * b0 + i01 * b1
        l1 = i10 * b0 + i11 * b1
        xyz = np.stack([(l0 * f1[i] + (t[i] + l1 * f2[i])) / 2.0 for i in range(3)], axis=1)
    return l0, l1, xyz


def cheirality_counts(R1, R2, u3, f_cur, f_ref, mask):
    out = []
    for c in range(4):
        R, t = candidate(c, R1, R2, u3)
        l0, l1, _ = triangulate(R, t, f_cur[mask], f_ref[mask])
        out.append(int(((l0 > 0.0) & (l1 > 0.0)).sum()))
    return out


def _reproj_error(f1, f2, em2):
    ex = f1[0] / f1[2] - f2[0] / f2[2]
    ey = f1[1] / f1[2] - f2[1] / f2[2]
    return em2 * np.sqrt(ex * ex + ey * ey)


def compute_inliers(R, t, f_cur, f_ref, reproj_thresh, error_multiplier2):
    """vk::computeInliers(f_cur, f_ref, R, t, ...) (S/math_utils.cpp:66-96): -> (xyz_in_cur [n][3], inlier flags).  The
    !(e1 > thresh || e2 > thresh) form is kept: a NaN error is an inlier."""
    _, _, xyz = triangulate(R, t, f_cur, f_ref)
    with np.errstate(all="ignore"):
        x = [xyz[:, i] for i in range(3)]
        e1 = _reproj_error([f_cur[:, i] for i in range(3)], x, error_multiplier2)
        d = [x[i] - t[i] for i in range(3)]
        q = [R[i] * d[0] + (R[3 + i] * d[1] + R[6 + i] * d[2]) for i in range(3)]          # R^T d
        e2 = _reproj_error([f_ref[:, i] for i in range(3)], q, error_multiplier2)
        return xyz, ~((e1 > reproj_thresh) | (e2 > reproj_thresh))


def quaternion(R):
    """Eigen's Quaterniond(R): {x, y, z, w}"""
    q = [0.0] * 4
    t = R[0] + (R[4] + R[8])
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (R[7] - R[5]) * t, (R[2] - R[6]) * t, (R[3] - R[1]) * t
    else:
        i = 0
        if R[4] > R[0]:
            i = 1
        if R[8] > R[4 * i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = _sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0)
        q[i] = 0.5 * t
        t = _div(0.5, t)
        q[3] = (R[3 * k + j] - R[3 * j + k]) * t
        q[j] = (R[3 * j + i] + R[3 * i + j]) * t
        q[k] = (R[3 * k + i] + R[3 * i + k]) * t
    return q


def so3_rotate(q, p):
    uv = _cross(q, p)
    uv = [uv[0] + uv[0], uv[1] + uv[1], uv[2] + uv[2]]
    quv = _cross(q, uv)
    return [(p[i] + q[3] * uv[i]) + quv[i] for i in range(3)]


def se3_mul(A, B):
    a, b = A[3:], B[3:]
    x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1]
    y = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2]
    z = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0]
    w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]
    rt = so3_rotate(a, B[:3])
    return [A[0] + rt[0], A[1] + rt[1], A[2] + rt[2], x, y, z, w]


def se3_inverse(T):
    qi = [-T[3], -T[4], -T[5], T[6]]
    rt = so3_rotate(qi, T[:3])
    return [-rt[0], -rt[1], -rt[2]] + qi


def se3_act(T, p):
    r = so3_rotate(T[3:], p)
    return [T[0] + r[0], T[1] + r[1], T[2] + r[2]]


def depth_key(z):
    u = np.asarray(z, np.float64).view(U64)
    return np.where(u >> U64(63), ~u, u | U64(0x8000000000000000))


def depth_median(z):
    """the order statistic of rank n / 2 (vk::getMedian) of ALL depths; a NaN among them gives NaN; negative depths order as
    numbers (the keys of svo_track_frame_end.h)"""
    z = np.asarray(z, np.float64)
    if np.isnan(z).any():
        return NAN
    k = np.sort(depth_key(z))[len(z) // 2]
    u = (k & U64(0x7FFFFFFFFFFFFFFF)) if (k >> U64(63)) else ~k
    return float(np.array([u], U64).view(np.float64)[0])


def second_pose(T_cur_from_ref, T_ref_w, scale):
    """:108-118 -> (T_cur_w with the rescaled translation, T_world_cur)"""
    T_cur_w = se3_mul(T_cur_from_ref, T_ref_w)
    ref_pos, cur_pos = se3_inverse(T_ref_w)[:3], se3_inverse(T_cur_w)[:3]
    p = [ref_pos[i] + scale * (cur_pos[i] - ref_pos[i]) for i in range(3)]
    r = _matvec(rotation_matrix(T_cur_w), p)            # -T_f_w_.rotation_matrix() * (...): an Eigen matrix-vector product
    T_cur_w = [-r[0], -r[1], -r[2]] + T_cur_w[3:]
    return T_cur_w, se3_inverse(T_cur_w)


def in_frame(px, width, height):
    """isInFrame(px.cast<int>(), 10) (:123): the cast truncates toward zero"""
    i = np.trunc(np.asarray(px, np.float32).astype(np.float64)).astype(np.int64)
    return (i[:, 0] >= 10) & (i[:, 0] < width - 10) & (i[:, 1] >= 10) & (i[:, 1] < height - 10)


# ---- the whole stage -------------------------------------------------------------------------------------------------------
def two_view(f_ref, f_cur, px_ref, px_cur, error_multiplier2, width, height, T_ref_w=None, reproj_thresh=2.0, min_inliers=40,
             map_scale=1.0, n_hypotheses=1024, seed=0):
    """-> dict with the result block (status, n_in, hypothesis, hypothesis_count, candidate, candidate_count, n_inliers, n_points,
    depth_median, scale, T_cur_from_ref, T_cur_w), counts [H], mask [n], inliers, xyz_in_cur [n][3] (None before the cheirality
    gate is passed), point_index, point_pos, and the inputs map_tables needs."""
    assert 1 <= n_hypotheses <= MAX_HYPOTHESES
    f_ref, f_cur = np.ascontiguousarray(f_ref, np.float64).reshape(-1, 3), np.ascontiguousarray(f_cur, np.float64).reshape(-1, 3)
    px_ref, px_cur = np.ascontiguousarray(px_ref, np.float32).reshape(-1, 2), np.ascontiguousarray(px_cur, np.float32).reshape(-1, 2)
    n = len(f_ref)
    T_ref_w = [float(v) for v in (IDENTITY if T_ref_w is None else T_ref_w)]
    nan7 = np.full(7, NAN)
    res = dict(status=OK, n_in=n, hypothesis=-1, hypothesis_count=-1, candidate=-1, candidate_count=0, n_inliers=0, n_points=0,
               depth_median=NAN, scale=NAN, T_cur_from_ref=nan7.copy(), T_cur_w=nan7.copy(), counts=np.zeros(0, np.int32),
               mask=np.zeros(n, np.uint8), inliers=np.zeros(0, np.int32), xyz_in_cur=None, point_index=np.zeros(0, np.int32),
               point_pos=np.zeros((0, 3)), f_ref=f_ref, f_cur=f_cur, px_ref=px_ref, px_cur=px_cur, T_ref_w=np.array(T_ref_w))
    if n < 8:
        res["status"] = TOO_FEW
        return res
    xy = normalised(f_ref, f_cur)
    t2 = thr2(reproj_thresh, error_multiplier2)
    F, valid = solve_hypotheses(xy, sample(seed, n_hypotheses, n))
    res["counts"] = counts = score_hypotheses(F, valid, xy, t2)
    h = winner(counts)
    if h < 0:
        res["status"] = NO_MODEL
        return res
    res["hypothesis"], res["hypothesis_count"] = h, int(counts[h])
    mask = epi_inliers(F[h], xy, t2)
    res["mask"] = mask.astype(np.uint8)
    R1, R2, u3 = decompose(F[h])
    cc = cheirality_counts(R1, R2, u3, f_cur, f_ref, mask)
    cand = 0
    for c in range(1, 4):
        if cc[c] > cc[cand]:
            cand = c
    res["candidate"], res["candidate_count"] = cand, cc[cand]
    if float(cc[cand]) < float(n) * 0.5:                  # the gate of :305
        res["status"] = CHEIRALITY
        return res
    R, t = candidate(cand, R1, R2, u3)
    res["R"], res["t"] = np.array(R), np.array(t)
    xyz, inl = compute_inliers(R, t, f_cur, f_ref, float(reproj_thresh), float(error_multiplier2))
    res["xyz_in_cur"] = xyz
    T_cur_from_ref = list(t) + quaternion(R)
    res["T_cur_from_ref"] = np.array(T_cur_from_ref)
    res["depth_median"] = median = depth_median(xyz[:, 2])
    inliers = np.nonzero(inl)[0].astype(np.int32)
    if len(inliers) < min_inliers:                        # the gate of :85
        res["status"] = FEW_INLIERS
        return res
    res["inliers"], res["n_inliers"] = inliers, len(inliers)
    with np.errstate(all="ignore"):
        res["scale"] = scale = float(np.float64(map_scale) / np.float64(median))
        T_cur_w, T_world_cur = second_pose(T_cur_from_ref, T_ref_w, scale)
        res["T_cur_w"] = np.array(T_cur_w)
        z = xyz[inliers, 2]
        keep = in_frame(px_cur[inliers], width, height) & in_frame(px_ref[inliers], width, height) & (z > 0.0)
        pts = inliers[keep]
        p = [xyz[pts, i] * scale for i in range(3)]
        pos = se3_act(T_world_cur, p)
    res["point_index"], res["n_points"] = pts, len(pts)
    res["point_pos"] = np.stack(pos, axis=1).reshape(-1, 3) if len(pts) else np.zeros((0, 3))
    return res


TYPE_UNKNOWN = 2


def map_tables(res, kf_slots=(0, 1)):
    """The index tables hip.FrameTracker.set_map takes (:117-138): two keyframes (ref, cur), every point of type unknown with its
    two observations in Point::obs_ order -- addFrameRef pushes to the front, cur is added first and ref second, so the list
    reads [ref, cur] --, level 0, no edgelets, kf_ftr_point of each frame in creation order, no candidates."""
    assert res["status"] == OK
    idx = np.asarray(res["point_index"], np.int64)
    m = len(idx)
    obs_px = np.empty((2 * m, 2))
    obs_f = np.empty((2 * m, 3))
    obs_px[0::2], obs_px[1::2] = res["px_ref"][idx].astype(np.float64), res["px_cur"][idx].astype(np.float64)
    obs_f[0::2], obs_f[1::2] = res["f_ref"][idx], res["f_cur"][idx]
    pts = np.arange(m, dtype=np.int32)
    return dict(kf_slot=np.array(kf_slots, np.int32), T_kf_w=np.stack([np.asarray(res["T_ref_w"], np.float64), np.asarray(res["T_cur_w"], np.float64)]),
                kf_key_point=np.full((2, 5), -1, np.int32), kf_ftr_offset=np.array([0, m, 2 * m], np.int32),
                kf_ftr_point=np.concatenate([pts, pts]), pt_pos=np.asarray(res["point_pos"], np.float64).reshape(m, 3),
                pt_type=np.full(m, TYPE_UNKNOWN, np.int32), pt_n_failed=np.zeros(m, np.int32), pt_n_succeeded=np.zeros(m, np.int32),
                pt_obs_offset=(2 * np.arange(m + 1)).astype(np.int32), obs_kf=np.tile(np.array([0, 1], np.int32), m), obs_px=obs_px, obs_f=obs_f,
                obs_level=np.zeros(2 * m, np.int32), obs_edgelet=np.zeros(2 * m, np.uint8), obs_grad=np.tile(np.array([1.0, 0.0]), (2 * m, 1)),
                cand_point=np.zeros(0, np.int32))
