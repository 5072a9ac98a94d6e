"""An extended-precision evaluation of pose_optimizer::optimizeGaussNewton (S/pose_optimizer.cpp:31-181) as
oracle/svo_oracle.c:svo_orc_pose_optimize states it, the seeded input families the pose-refinement tests share, and the
assertions both of them put a result through (tests/test_oracle_pose_reference.py on the CPU, tests/test_gpu_pose_refine.py
on the GPU).  Not collected as a test.

  * refine: the algorithm in numpy.longdouble, vectorised over the observations.  Typed pieces stay typed -- the f32
    errors of the MAD scale, 1.48f, the f32 Tukey weight of float32(sqrt(sq) / scale), the f64 constants 0.85 / em and
    reproj_thresh / em -- everything else (residuals, Jacobians, the 28 sums, a hand-written 6x6 elimination, SE3::exp
    by its Taylor series, the covariance as the inverse of the last evaluated A em^2) is carried to ~1e-19.  Besides the
    result it returns what a test needs to decide whether a comparison means anything: the relative distance of every
    chi2 test from its boundary, of every final error from the outlier threshold, of every sqrt(sq) / scale from the
    nearest f32 rounding boundary, theta^2 and max |dT| of every step, and the length of the run of equal keys each of
    the three medians falls into.
  * FAMILIES: classes (one frame on either side of every split of block_rank_select, of the rank / radix switch and of
    the register cache), class_count (the class chosen by n far from the observation count), ties (all three medians
    inside runs of equal keys), threshold (observations near and, in one built case, within 1e-6 of the outlier
    threshold on both sides), exits (every way out of the loop, n_iter and reproj_thresh settings), large_steps (theta^2
    on both sides of 0.25), perfect (rounding-noise errors) and ill_posed (discrete checks only).
  * check_exact / check_discrete / distances / family_bounds / check_continuous: the assertions.  The continuous bound of
    a family is MARGIN x max(the oracle's own largest distance to this reference over the family, FLOOR): it is derived
    from the reference's error, never from the kernel's.

Not built: an input whose Tukey weights are all zero from iteration 5 on.  It does not reach the NaN-dT exit: with A = 0
and b = 0 Eigen's LDLT (and the oracle's and the kernel's restatement of it) returns dT = 0 through its pseudo-inverse of
D, the chi2 test passes, SE3::exp runs at theta == 0 and its unguarded 0 / 0 makes the translation NaN, the loop leaves
through the convergence test and every later quantity is NaN with medians that depend on how the selection orders NaNs.
A plain elimination yields 0 / 0 for dT instead and restores T_old, so this reference and the oracle disagree there."""
import dataclasses

import numpy as np

from android_svo_amd import synth

L, F32, F64 = np.longdouble, np.float32, np.float64
assert np.finfo(L).nmant >= 63, "numpy.longdouble is not extended precision on this platform"

EM = 500.0                                   # cam->errorMultiplier2() of synth.Camera.default()
EPS = 0.0000000001                           # I/global.h:91
MARGIN, FLOOR = 8.0, 2.0 ** -50              # continuous bound = MARGIN * max(oracle's distance over the family, FLOOR)
CHI2_UNDECIDABLE = 1e-9                      # a chi2 test this close (relative) to its boundary: the case is undecidable
THRESH_UNDECIDABLE = 1e-9                    # a final error this close (relative) to the threshold: the observation is
F32_UNDECIDABLE = 2.0 ** -44                 # sqrt(sq) / scale this close (relative) to an f32 rounding boundary: the case is
QUANTITIES = ("rot", "trans", "error_init", "error_final", "cov")


@dataclasses.dataclass
class Result:
    """what svo_hip_pose_opt_result / svo_orc_pose_opt_result carry, plus has_point after the outlier test"""
    ran: int
    n_iter_done: int
    n_deleted: int
    num_obs: int
    T_f_w: np.ndarray
    estimated_scale: float
    error_init: float
    error_final: float
    Cov: np.ndarray
    has_point: np.ndarray

    @staticmethod
    def of(r, has_point):
        return Result(int(r.ran), int(r.n_iter_done), int(r.n_deleted), int(r.num_obs), np.array(r.T_f_w, dtype=F64),
                      float(r.estimated_scale), float(r.error_init), float(r.error_final), np.array(r.Cov, dtype=F64),
                      np.array(has_point, dtype=np.uint8))


@dataclasses.dataclass
class Case:
    name: str
    T_f_w_init: np.ndarray
    f: np.ndarray
    pos: np.ndarray
    level: np.ndarray
    has_point: np.ndarray
    reproj_thresh: float = 2.0
    n_iter: int = 10
    perfect: bool = False          # errors are rounding noise: only the discrete results and the pose are compared
    ill_posed: bool = False        # oracle and reference disagree grossly: only the exact checks

    @property
    def n_obs(self):
        return int((self.has_point != 0).sum())

    @property
    def well_posed(self):
        return not self.ill_posed and self.n_obs >= 7


@dataclasses.dataclass
class Ref:
    result: Result                 # rounded to f64
    T: np.ndarray                  # longdouble
    exit: str                      # "n_iter" | "converged" | "chi2" | "nan" | "none" (no observation)
    chi2_margin: list              # per iteration > 0: |new_chi2 - 1.2 chi2| / (1.2 chi2)
    thresh_dist: np.ndarray        # per feature slot: |sqrt(sq_final) - thresh| / thresh (inf where no observation)
    f32_dist: list                 # per iteration: min over the observations with a non-zero weight in reach
    theta_sq: list
    max_dT: list
    tie_runs: tuple                # keys equal to the median of (f32 errors, sq_init, sq_final)
    undecidable: bool              # as a whole: a chi2 test or an f32 rounding too close to call
    near_thresh: np.ndarray        # per feature slot: the outlier decision is too close to call


# ---- the algorithm ---------------------------------------------------------------------------------------------------
def _rot(q, p):
    """I/SO3.h:478-483: p + w uv + q x uv, uv = 2 (q x p)"""
    uv = np.cross(q[:3], p)
    uv = uv + uv
    return p + q[3] * uv + np.cross(q[:3], uv)


def _quat_mul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                     a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
                     a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]], dtype=L)


def _errors(T, f, pos, s):
    xyz = T[:3] + _rot(T[3:], pos)
    e = np.stack([f[:, 0] / f[:, 2] - xyz[:, 0] / xyz[:, 2], f[:, 1] / f[:, 2] - xyz[:, 1] / xyz[:, 2]], axis=1) * s[:, None]
    return e, xyz


def solve_elim(A, B):
    """A X = B by elimination with partial pivoting, in the precision of A (a zero pivot divides by zero as it stands)"""
    n = A.shape[0]
    M = np.concatenate([A, B.reshape(n, -1)], axis=1).copy()
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if p != k:
            M[[k, p]] = M[[p, k]]
        M[k] = M[k] / M[k, k]
        for i in range(n):
            if i != k:
                M[i] = M[i] - M[i, k] * M[k]
    return M[:, n:].reshape(B.shape)


def _series(z, first_k, n_terms=40):
    """sum over k >= 0 of (-z)^k / (2k + first_k)!"""
    term = L(1)
    for j in range(2, first_k + 1):
        term = term / L(j)
    total = term
    for k in range(1, n_terms):
        term = -term * z / (L(2 * k + first_k - 1) * L(2 * k + first_k))
        total = total + term
    return total


def se3_exp(d):
    """I/SE3.h:153-182 with the trigonometric factors by their Taylor series (no cancellation at small angles); the NaN
    translation at theta == 0 stays"""
    p, r = d[:3], d[3:]
    z = r @ r
    if z <= L(10):
        c1 = _series(z, 2)                       # (1 - cos t) / t^2
        c2 = _series(z, 3)                       # (t - sin t) / t^3
        imag = _series(z / 4, 1) / 2             # sin(t / 2) / t
        real = _series(z / 4, 0)                 # cos(t / 2)
    else:
        t = np.sqrt(z)
        c1, c2, imag, real = (1 - np.cos(t)) / z, (t - np.sin(t)) / (z * t), np.sin(t / 2) / t, np.cos(t / 2)
    if z == 0:
        c1 = c2 = L(np.nan)
    rxp = np.cross(r, p)
    return np.concatenate([p + c1 * rxp + c2 * np.cross(r, rxp), imag * r, [real]]).astype(L)


def tukey_weight_f32(x):
    """TukeyWeightFunction::value with DEFAULT_B (S/robust_cost.cpp:87-106) on a float32 array, every operation in float32"""
    b = F32(8.6851)
    b_square = b * b
    x_square = x * x
    tmp = F32(1.0) - x_square / b_square
    return np.where(x_square <= b_square, tmp * tmp, F32(0.0)).astype(F32)


def _f32_boundary_distance(x, xf):
    """relative distance of the longdouble x from the nearest midpoint between two neighbouring float32 numbers"""
    lo, hi = np.nextafter(xf, F32(-np.inf)), np.nextafter(xf, F32(np.inf))
    m_lo, m_hi = (xf.astype(L) + lo.astype(L)) / 2, (xf.astype(L) + hi.astype(L)) / 2
    return np.minimum(np.abs(x - m_lo), np.abs(x - m_hi)) / np.maximum(np.abs(x), L(1e-300))


def refine(case, em=EM, lower_median=False, drop_in_sums=None):
    """The reference evaluation of one case.  lower_median / drop_in_sums make deliberately WRONG stand-ins for the tests
    of the assertions: index (n_obs - 1) // 2 for the three medians; one observation left out of the Gauss-Newton sums."""
    with np.errstate(all="ignore"):
        return _refine(case, em, lower_median, drop_in_sums)


def _refine(case, em, lower_median, drop_in_sums):
    n = len(case.level)
    obs = np.where(np.asarray(case.has_point) != 0)[0]
    n_obs = len(obs)
    T = np.asarray(case.T_f_w_init, dtype=F64).astype(L)
    hp = np.array(case.has_point, dtype=np.uint8)
    if n_obs == 0:
        res = Result(0, 0, 0, 0, T.astype(F64), 0.0, 0.0, 0.0, np.zeros(36), hp)
        return Ref(res, T, "none", [], np.full(n, np.inf), [], [], [], (0, 0, 0), False, np.zeros(n, bool))
    f, pos = np.asarray(case.f, dtype=F64)[obs].astype(L), np.asarray(case.pos, dtype=F64)[obs].astype(L)
    s = (1.0 / (1 << np.asarray(case.level)[obs].astype(np.int64))).astype(L)
    kmed = (n_obs - 1) // 2 if lower_median else n_obs // 2
    # :51-66 scale of the error
    e, _ = _errors(T, f, pos, s)
    err32 = np.sqrt(e[:, 0] ** 2 + e[:, 1] ** 2).astype(F32)
    med32 = np.sort(err32)[kmed]
    estimated_scale = F64(F32(1.48) * med32)
    tie_err = int((err32 == med32).sum())
    # :70-138
    T_old = T.copy()
    chi2 = L(0)
    A = np.zeros((6, 6), dtype=L)
    sq_init = None
    exit_kind, n_done = "n_iter", 0
    chi2_margin, f32_dist, theta_sq, max_dT = [], [], [], []
    scale = L(estimated_scale)
    for it in range(case.n_iter):
        if it == 5:
            scale = L(F64(0.85) / F64(em))
        e, xyz = _errors(T, f, pos, s)
        sq = e[:, 0] ** 2 + e[:, 1] ** 2
        if it == 0:
            sq_init = sq
        x, y, zi = xyz[:, 0], xyz[:, 1], 1 / xyz[:, 2]
        zi2 = zi * zi
        zero, j02, j12 = np.zeros_like(x), x * zi2, y * zi2
        J0 = np.stack([-zi, zero, j02, y * j02, -(1 + x * j02), y * zi], axis=1) * s[:, None]
        J1 = np.stack([zero, -zi, j12, 1 + y * j12, -(y * j02), -x * zi], axis=1) * s[:, None]
        xs = np.sqrt(sq) / scale
        xf = xs.astype(F32)
        w32 = tukey_weight_f32(xf)
        w = w32.astype(L)
        in_reach = xf <= F32(8.7)                       # beyond: the weight is zero whichever way x rounds
        f32_dist.append(float(_f32_boundary_distance(xs, xf)[in_reach].min()) if in_reach.any() else np.inf)
        if drop_in_sums is not None:
            w = w.copy()
            w[np.searchsorted(obs, drop_in_sums)] = 0
        A = (J0 * w[:, None]).T @ J0 + (J1 * w[:, None]).T @ J1
        b = -((J0 * (e[:, 0] * w)[:, None]).sum(axis=0) + (J1 * (e[:, 1] * w)[:, None]).sum(axis=0))
        new_chi2 = (sq * w).sum()
        dT = solve_elim(A, b)
        n_done = it + 1
        if it > 0:
            chi2_margin.append(float(abs(new_chi2 - chi2 * L(1.2)) / (chi2 * L(1.2))))
        if (it > 0 and new_chi2 > chi2 * L(1.2)) or np.isnan(dT[0]):
            exit_kind = "nan" if np.isnan(dT[0]) else "chi2"
            T = T_old
            break
        theta_sq.append(float(dT[3:] @ dT[3:]))
        max_dT.append(float(np.abs(dT).max()))
        E = se3_exp(dT)
        T_old = T
        T = np.concatenate([E[:3] + _rot(E[3:], T[:3]), _quat_mul(E[3:], T[3:])])
        chi2 = new_chi2
        if np.abs(dT).max() <= L(EPS):
            exit_kind = "converged"
            break
    cov = solve_elim(A * L(em) ** 2, np.eye(6, dtype=L))
    # :144-159
    thresh = L(F64(case.reproj_thresh) / F64(em))
    e, _ = _errors(T, f, pos, s)
    sq_final = e[:, 0] ** 2 + e[:, 1] ** 2
    deleted = np.sqrt(sq_final) > thresh
    hp[obs[deleted]] = 0
    thresh_dist = np.full(n, np.inf)
    thresh_dist[obs] = (np.abs(np.sqrt(sq_final) - thresh) / thresh).astype(F64)
    near = thresh_dist < THRESH_UNDECIDABLE
    # :161-166
    med_f = np.sort(sq_final)[kmed]
    error_final = np.sqrt(med_f) * L(em)
    tie_f = int((sq_final == med_f).sum())
    if sq_init is not None:
        med_i = np.sort(sq_init)[kmed]
        error_init = np.sqrt(med_i) * L(em)
        tie_i = int((sq_init == med_i).sum())
    else:
        error_init, tie_i = L(0), 0
    n_del = int(deleted.sum())
    res = Result(1, n_done, n_del, n_obs - n_del, T.astype(F64), float(estimated_scale * F64(em)), float(error_init),
                 float(error_final), cov.astype(F64).reshape(36), hp)
    undecidable = bool((len(chi2_margin) and min(chi2_margin) < CHI2_UNDECIDABLE) or
                       (len(f32_dist) and min(f32_dist) < F32_UNDECIDABLE))
    return Ref(res, T, exit_kind, chi2_margin, thresh_dist, f32_dist, theta_sq, max_dT, (tie_err, tie_i, tie_f), undecidable, near)


# ---- the assertions --------------------------------------------------------------------------------------------------
def _bits(v):
    return np.array(v, dtype=F64).view(np.uint64)


def check_exact(case, ref, got):
    """what holds bit for bit in every case, ill-posed ones included"""
    n_obs = case.n_obs
    entry = np.asarray(case.has_point) != 0
    assert got.ran == (1 if n_obs else 0), (case.name, "ran", got.ran)
    assert not got.has_point[~entry].any(), (case.name, "a slot without a point on entry was written")
    assert set(np.unique(got.has_point[entry])) <= {0, 1}, (case.name, "has_point values")
    if not n_obs:
        assert got.num_obs == 0 and got.n_deleted == 0 and _bits(got.T_f_w).tolist() == _bits(case.T_f_w_init).tolist(), case.name
        return
    assert got.num_obs + got.n_deleted == n_obs, (case.name, "num_obs + n_deleted", got.num_obs, got.n_deleted, n_obs)
    assert got.n_deleted == int((entry & (got.has_point == 0)).sum()), (case.name, "n_deleted against has_point")
    if not case.perfect:
        assert _bits(got.estimated_scale) == _bits(ref.result.estimated_scale), \
            (case.name, "estimated_scale", got.estimated_scale, ref.result.estimated_scale)


def check_discrete(case, ref, got):
    """well-posed cases: the iteration count and every outlier decision the reference can call"""
    if ref.undecidable:
        return
    r = ref.result
    assert got.n_iter_done == r.n_iter_done, (case.name, "n_iter_done", got.n_iter_done, r.n_iter_done, ref.exit)
    dec = (np.asarray(case.has_point) != 0) & ~ref.near_thresh
    wrong = np.where(dec & (got.has_point != r.has_point))[0]
    assert len(wrong) == 0, (case.name, "outlier decisions differ at", wrong[:8].tolist(), ref.thresh_dist[wrong[:8]].tolist())
    open_ = int(ref.near_thresh.sum())
    assert abs(got.n_deleted - r.n_deleted) <= open_ and abs(got.num_obs - r.num_obs) <= open_, (case.name, got.n_deleted, r.n_deleted)


def distances(case, ref, got):
    """{quantity: distance of `got` to the reference}; quantities that carry no information in this case are left out"""
    r = ref.result
    rot, trans = synth.pose_error(got.T_f_w, r.T_f_w)
    d = {"rot": rot, "trans": trans}
    if case.perfect:
        return d
    if case.n_iter > 0:
        d["error_init"] = abs(got.error_init - r.error_init) / r.error_init
        d["cov"] = float(np.abs(got.Cov - r.Cov).max() / np.abs(r.Cov).max())
    d["error_final"] = abs(got.error_final - r.error_final) / r.error_final
    return {k: (float(v) if np.isfinite(v) else np.inf) for k, v in d.items()}


def comparable(case, ref):
    return case.well_posed and not ref.undecidable


def family_distances(cases, refs, results):
    """{quantity: the largest distance over the family's comparable cases}"""
    worst = {}
    for c, r, g in zip(cases, refs, results):
        if comparable(c, r):
            for k, v in distances(c, r, g).items():
                worst[k] = max(worst.get(k, 0.0), v)
    return worst


def family_bounds(cases, refs, oracle_results):
    return {k: MARGIN * max(v, FLOOR) for k, v in family_distances(cases, refs, oracle_results).items()}


def check_continuous(case, ref, got, bounds, oracle_result=None):
    """the distance of `got` to the reference within the family's bounds; with no iteration the covariance is the inverse
    of the zero matrix: non-finite wherever the oracle's is"""
    if not comparable(case, ref):
        return {}
    d = distances(case, ref, got)
    for k, v in d.items():
        assert v <= bounds[k], (case.name, k, v, bounds[k])
    if case.n_iter == 0 and not case.perfect:
        assert got.error_init == 0.0, (case.name, "error_init without an iteration")
        if oracle_result is not None:
            assert not np.isfinite(got.Cov[~np.isfinite(oracle_result.Cov)]).any(), (case.name, "Cov without an iteration")
    return d


def check_all(case, ref, got, bounds, oracle_result=None):
    check_exact(case, ref, got)
    if case.well_posed:
        check_discrete(case, ref, got)
        return check_continuous(case, ref, got, bounds, oracle_result)
    return {}


def exclusion_cap(cases, refs):
    """(cases excluded as undecidable as a whole, well-posed cases): at most 1 and at most 5 % may be"""
    wp = [(c, r) for c, r in zip(cases, refs) if c.well_posed]
    return sum(1 for c, r in wp if r.undecidable), len(wp)


# ---- the input families ----------------------------------------------------------------------------------------------
def _case(name, pc, **kw):
    return Case(name, pc.T_f_w_init.copy(), pc.f.copy(), pc.pos.copy(), pc.level.copy(), pc.has_point.copy(), **kw)


CLASS_SIZES = (7, 63, 64, 65, 127, 128, 129, 255, 256, 257, 2047, 2048, 2049, 2305)


def gen_classes():
    out = []
    for k, n in enumerate(CLASS_SIZES):
        for ne in (11, 0):
            out.append(_case("classes n=%d null_every=%d" % (n, ne), synth.make_pose_opt_case(seed=100 + 2 * k + (ne == 0), n=n, null_every=ne)))
    return out


def gen_class_count():
    out = []
    pc = synth.make_pose_opt_case(seed=140, n=256, null_every=0)
    pc.has_point[:] = 0
    pc.has_point[[0, 100, 255]] = 1
    out.append(_case("class_count n=256 with 3 observations", pc))
    pc = synth.make_pose_opt_case(seed=141, n=257, null_every=0, outlier_frac=0.0)
    pc.has_point[:] = 0
    pc.has_point[[0, 37, 64, 100, 128, 200, 255, 256]] = 1
    out.append(_case("class_count n=257 with 8 observations", pc))
    pc = synth.make_pose_opt_case(seed=142, n=2600)
    pc.has_point[:2048] = 0
    out.append(_case("class_count n=2600, observations only beyond 2048", pc))
    pc = synth.make_pose_opt_case(seed=143, n=2600)
    pc.has_point[2048:] = 0
    out.append(_case("class_count n=2600, observations only below 2048", pc))
    pc = synth.make_pose_opt_case(seed=144, n=300)
    pc.has_point[[0, 256]] = 0
    out.append(_case("class_count n=300, thread 0 without a point", pc))
    return out


TIE_PERIOD = 23


def gen_ties():
    out = []
    for k, (n, ne) in enumerate(((64, 0), (129, 0), (300, 11), (2305, 11))):
        pc = synth.make_pose_opt_case(seed=150 + k, n=n, null_every=ne)
        idx = np.arange(n) % TIE_PERIOD
        pc.f, pc.pos, pc.level = np.ascontiguousarray(pc.f[idx]), np.ascontiguousarray(pc.pos[idx]), np.ascontiguousarray(pc.level[idx])
        out.append(_case("ties n=%d n_obs=%d" % (n, int(pc.has_point.sum())), pc))
    return out


THRESHOLD_SEEDS = (160, 161, 162)
NEAR_DELTA = 5e-7                            # the built case puts observations at thresh (1 +- NEAR_DELTA)
NEAR_SLOTS = 8


def _near_threshold_case(seed=163):
    """Eight inliers of a threshold case moved so that their FINAL error lies at reproj_thresh / em (1 +- 5e-7): the
    measurement is rescaled along its final residual at the reference's final pose, and the step repeated (the final pose
    moves a little with the measurements) until all of them sit within 1e-6 on their side."""
    pc = synth.make_pose_opt_case(seed=seed, n=600, px_noise=1.0, outlier_frac=0.05)
    case = _case("threshold built within 1e-6", pc)
    ref = refine(case)
    slots = np.where((case.has_point != 0) & (ref.result.has_point != 0) & (ref.thresh_dist < 0.8) & (ref.thresh_dist > 0.3))[0][:NEAR_SLOTS]
    target = 1.0 + NEAR_DELTA * np.where(np.arange(len(slots)) % 2 == 0, 1.0, -1.0)
    thresh = L(F64(case.reproj_thresh) / F64(EM))
    for _ in range(6):
        T = ref.T
        f, pos = case.f[slots].astype(L), case.pos[slots].astype(L)
        s = (1.0 / (1 << case.level[slots].astype(np.int64))).astype(L)
        e, xyz = _errors(T, f, pos, s)
        norm = np.sqrt(e[:, 0] ** 2 + e[:, 1] ** 2)
        proj = np.stack([xyz[:, 0] / xyz[:, 2], xyz[:, 1] / xyz[:, 2]], axis=1)
        uv = proj + e / s[:, None] * (thresh * target.astype(L) / norm)[:, None]
        fn = np.concatenate([uv, np.ones((len(slots), 1), dtype=L)], axis=1)
        case.f[slots] = (fn / np.sqrt((fn ** 2).sum(axis=1))[:, None]).astype(F64)
        ref = refine(case)
    return case


def gen_threshold():
    out = [_case("threshold seed=%d" % sd, synth.make_pose_opt_case(seed=sd, n=600, px_noise=1.0, outlier_frac=0.05)) for sd in THRESHOLD_SEEDS]
    out.append(_near_threshold_case())
    return out


ALL_OUTLIER_SEEDS = (170, 171, 172, 173, 174, 175)


def gen_exits():
    out = [_case("exits all outliers seed=%d" % sd, synth.make_pose_opt_case(seed=sd, n=150, outlier_frac=1.0)) for sd in ALL_OUTLIER_SEEDS]
    for n_iter in (0, 1, 5, 6, 10):
        out.append(_case("exits n_iter=%d" % n_iter, synth.make_pose_opt_case(seed=180, n=200), n_iter=n_iter))
    for rt in (0.5, 2.0, 1e9):
        out.append(_case("exits reproj_thresh=%g" % rt, synth.make_pose_opt_case(seed=181, n=200), reproj_thresh=rt))
    return out


def gen_perfect():
    pc = synth.make_pose_opt_case(seed=185, n=200, px_noise=0.0, outlier_frac=0.0, pose_err=(0.0, 0.0))
    return [_case("perfect data from the true pose", pc, perfect=True)]


LARGE_STEP_SEEDS = (190, 191, 192, 193, 194, 195)


def gen_large_steps():
    return [_case("large_steps seed=%d" % sd, synth.make_pose_opt_case(seed=sd, n=300, px_noise=0.1, outlier_frac=0.0, pose_err=(0.02, 0.8)))
            for sd in LARGE_STEP_SEEDS]


def gen_ill_posed():
    out = []
    for k in (1, 2, 3):
        pc = synth.make_pose_opt_case(seed=200 + k, n=40, null_every=0)
        pc.has_point[:] = 0
        pc.has_point[[5, 17, 33][:k]] = 1
        out.append(_case("ill_posed n_obs=%d" % k, pc, ill_posed=True))
    out.append(_case("ill_posed diverging", synth.make_pose_opt_case(seed=204, n=200, pose_err=(1.5, 0.5)), ill_posed=True))
    return out


FAMILIES = {"classes": gen_classes, "class_count": gen_class_count, "ties": gen_ties, "threshold": gen_threshold,
            "exits": gen_exits, "perfect": gen_perfect, "large_steps": gen_large_steps, "ill_posed": gen_ill_posed}

_cache = {}


def family(name):
    """(cases, references) of a family, computed once per process; neither is to be modified"""
    if name not in _cache:
        cases = FAMILIES[name]()
        _cache[name] = (cases, [refine(c) for c in cases])
    return _cache[name]


def oracle_family(name):
    """the oracle's results of a family, computed once per process"""
    if ("orc", name) not in _cache:
        _cache[("orc", name)] = oracle_results(family(name)[0])
    return _cache[("orc", name)]


def oracle_results(cases, em=EM):
    from oracle import orc
    out = []
    for c in cases:
        o, hp = orc.pose_optimize(em, c.T_f_w_init, c.f, c.pos, c.level, c.has_point, reproj_thresh=c.reproj_thresh, n_iter=c.n_iter)
        out.append(Result.of(o, hp))
    return out
