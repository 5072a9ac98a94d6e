"""Independent evaluations of DepthFilter::updateSeed / computeTau (S/depth_filter.cpp:359-416) and the seeded input
families the seed-arithmetic tests share (tests/test_oracle_seed_independent.py, tests/test_oracle_seed_edges.py on the
CPU; tests/test_gpu_seed_arithmetic.py, tests/test_gpu_odd_pyramids.py on the GPU).  Not collected as a test.

  * update_seed_typed / update_seed_exact / compute_tau_np: the two functions statement by statement in numpy, once with
    the C++ promotion rules written out and once in extended precision;
  * update_seed_guarded: the typed evaluation behind the reference's NaN guard (depth_filter.cpp:370-371);
  * gen_life / gen_fresh / gen_special: seed states and measurements where a seed spends its life, at its birth, and at
    the special values (NaN, inf, zero, negative, subnormal) of every input;
  * gen_tau: five families of (translation, bearing, depth) for computeTau, from well-conditioned to degenerate;
  * glue_case / odd_df_case / odd_align_case: the scenes the finalize-glue and odd-pyramid tests run, with the branch
    counts the CPU test proves on the oracle alone.

Everything is generated from fixed seeds; the CPU test establishes that the oracle alone meets every condition the GPU
tests rely on, so that those cannot pass vacuously."""
import dataclasses

import numpy as np

from android_svo_amd import seedsynth, synth
from oracle import orc

F32, F64 = np.float32, np.float64
SQRT_2_PI = 1.41421356237309505            # depth_filter.cpp:360 -- sqrt(2), not sqrt(2 pi): kept
PI = 3.14159265                            # I/global.h:92


def update_seed_typed(x, tau2, a, b, mu, z_range, sigma2):
    """depth_filter.cpp:368-391 on float32 arrays; every line keeps the type the C++ expression has"""
    d = lambda v: v.astype(F64)
    f = lambda v: v.astype(F32)
    norm_scale = np.sqrt(sigma2 + tau2)                                          # float
    s2 = f(1.0 / (1.0 / d(sigma2) + 1.0 / d(tau2)))                              # 1. literals: double, truncated
    m = s2 * (mu / sigma2 + x / tau2)                                            # float
    exponent = -0.5 * ((d(x) - d(mu)) / d(norm_scale)) ** 2                      # normal_pdf: all double
    pdf = (1.0 / (d(norm_scale) * SQRT_2_PI)) * np.exp(exponent)
    C1 = f(d(a / (a + b)) * pdf)
    C2 = f(d(b / (a + b)) * 1.0 / d(z_range))
    nc = C1 + C2
    C1 = C1 / nc
    C2 = C2 / nc
    ab = a + b                                                                   # float
    ff = f(d(C1) * (d(a) + 1.0) / (d(ab) + 1.0) + d(C2 * a) / (d(ab) + 1.0))
    e = f(d(C1) * (d(a) + 1.0) * (d(a) + 2.0) / ((d(ab) + 1.0) * (d(ab) + 2.0)) +
          d(C2 * a * (a + F32(1.0)) / ((ab + F32(1.0)) * (ab + F32(2.0)))))
    mu_new = C1 * m + C2 * mu
    sigma2_new = C1 * (s2 + m * m) + C2 * (sigma2 + mu * mu) - mu_new * mu_new
    a_new = (e - ff) / (ff - e / ff)
    b_new = a_new * (F32(1.0) - ff) / ff
    return a_new, b_new, mu_new, sigma2_new


def update_seed_guarded(x, tau2, a, b, mu, z_range, sigma2):
    """update_seed_typed behind the reference's guard: `if (std::isnan(norm_scale)) return;` leaves the seed untouched"""
    with np.errstate(all="ignore"):
        na, nb, nmu, ns2 = update_seed_typed(x, tau2, a, b, mu, z_range, sigma2)
        skip = np.isnan(np.sqrt(sigma2 + tau2))
    return np.where(skip, a, na), np.where(skip, b, nb), np.where(skip, mu, nmu), np.where(skip, sigma2, ns2)


def update_seed_exact(x, tau2, a, b, mu, z_range, sigma2):
    L = np.longdouble
    x, tau2, a, b, mu, z_range, sigma2 = (v.astype(L) for v in (x, tau2, a, b, mu, z_range, sigma2))
    ns = np.sqrt(sigma2 + tau2)
    s2 = 1 / (1 / sigma2 + 1 / tau2)
    m = s2 * (mu / sigma2 + x / tau2)
    pdf = (1 / (ns * L(SQRT_2_PI))) * np.exp(-0.5 * ((x - mu) / ns) ** 2)
    C1 = a / (a + b) * pdf
    C2 = b / (a + b) / z_range
    nc = C1 + C2
    C1, C2 = C1 / nc, C2 / nc
    ff = C1 * (a + 1) / (a + b + 1) + C2 * a / (a + b + 1)
    e = C1 * (a + 1) * (a + 2) / ((a + b + 1) * (a + b + 2)) + C2 * a * (a + 1) / ((a + b + 1) * (a + b + 2))
    mu_new = C1 * m + C2 * mu
    sigma2_new = C1 * (s2 + m * m) + C2 * (sigma2 + mu * mu) - mu_new * mu_new
    a_new = (e - ff) / (ff - e / ff)
    return a_new, a_new * (1 - ff) / ff, mu_new, sigma2_new


def compute_tau_np(t, f, z, px_error_angle, dtype):
    """depth_filter.cpp:396-416"""
    t, f, z = t.astype(dtype), f.astype(dtype), z.astype(dtype)
    a = f * z[:, None] - t
    t_norm = np.sqrt((t * t).sum(axis=1))
    a_norm = np.sqrt((a * a).sum(axis=1))
    alpha = np.arccos((f * t).sum(axis=1) / t_norm)
    beta = np.arccos((a * -t).sum(axis=1) / (t_norm * a_norm))
    beta_plus = beta + dtype(px_error_angle)
    gamma_plus = dtype(PI) - alpha - beta_plus
    return t_norm * np.sin(beta_plus) / np.sin(gamma_plus) - z


# ---- the oracle over arrays -----------------------------------------------------------------------------------------
def oracle_update_seed(x, tau2, a, b, mu, z_range, sigma2):
    """orc.update_seed seed by seed; returns (a, b, mu, z_range, sigma2) as float32 arrays"""
    got = np.array([orc.update_seed(x[i], tau2[i], (a[i], b[i], mu[i], z_range[i], sigma2[i])) for i in range(len(x))],
                   dtype=F32).reshape(len(x), 5)
    return tuple(np.ascontiguousarray(got[:, k]) for k in range(5))


def oracle_compute_tau(t, f, z, px_error_angle):
    """orc.compute_tau element by element; t [n,3] (only the translation of T_ref_cur enters computeTau)"""
    T = np.zeros(7)
    T[6] = 1.0
    out = np.empty(len(z))
    for i in range(len(z)):
        T[:3] = t[i]
        out[i] = orc.compute_tau(T, f[i], z[i], px_error_angle)
    return out


def same_bits(got, want):
    """elementwise: equal bit patterns, two NaNs counting as equal whatever their payload"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.dtype in (F32, F64)
    u = np.uint32 if got.dtype == F32 else np.uint64
    return (got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))


def state_same_bits(got4, want4):
    """per seed: a, b, mu and sigma2 all bit-equal (NaN == NaN)"""
    return np.logical_and.reduce([same_bits(g, w) for g, w in zip(got4, want4)])


def assert_remainder_close(got4, want4, same, what=""):
    """The rule for seeds whose state is not bit-equal to the oracle's: equal NaN pattern, mu within rtol 3e-6 (the
    project's figure for a last-bit exp difference), |sigma2 difference| <= 3e-6 (mu^2 + |sigma2|)"""
    r = ~same
    for g, w, name in zip(got4, want4, ("a", "b", "mu", "sigma2")):
        np.testing.assert_array_equal(np.isnan(g[r]), np.isnan(w[r]), err_msg="%s NaN pattern of %s" % (what, name))
    gmu, wmu, gs2, ws2 = (v[r].astype(F64) for v in (got4[2], want4[2], got4[3], want4[3]))
    fin = np.isfinite(wmu) & np.isfinite(ws2)
    np.testing.assert_allclose(gmu[fin], wmu[fin], rtol=3e-6, atol=0, err_msg=what + " mu")
    assert (np.abs(gs2 - ws2)[fin] <= 3e-6 * (wmu[fin] ** 2 + np.abs(ws2[fin]))).all(), what + " sigma2"
    for g, w in ((gmu, wmu), (gs2, ws2)):            # infinities: the same ones
        np.testing.assert_array_equal(g[np.isinf(w)], w[np.isinf(w)], err_msg=what + " infinities")


def error_stats(got4, exact4, ok):
    """The statistics tests/test_oracle_seed_independent.py defines, of a float32 result (a, b, mu, sigma2) against the
    extended-precision one on the seeds `ok`: relative error of mu; error of sigma2 relative to mu^2 + sigma2
    (sigma2 = E[x^2] - mu^2 cancels in f32); relative errors of a and b over their cancellation factor |a| + |b| + 1.
    Returns {name: (99.9th percentile, maximum)}"""
    ga, gb, gmu, gs2 = (v.astype(F64)[ok] for v in got4)
    ea, eb, emu, es2 = (v[ok] for v in exact4)
    rel = lambda g, e: np.abs(g - e) / np.maximum(np.abs(e), 1e-30)
    amp = np.abs(ea) + np.abs(eb) + 1.0
    errs = {"mu": rel(gmu, emu), "sigma2": np.abs(gs2 - es2) / (emu ** 2 + es2), "a": rel(ga, ea) / amp, "b": rel(gb, eb) / amp}
    return {k: (float(np.percentile(v, 99.9)), float(v.max())) for k, v in errs.items()}


# ---- updateSeed input families ----------------------------------------------------------------------------------------
SEED_ARGS = ("x", "tau2", "a", "b", "mu", "z_range", "sigma2")


def life_state(n, rng, mu=None):
    """where a seed spends its life: a, b over six decades, sigma from z_range/6 to z_range/400 (past the convergence test
    at z_range/200), tau2 over ten decades, measurements from well inside one sigma to 400 sigma away"""
    a = (10.0 ** rng.uniform(-3, 3, n)).astype(F32)
    b = (10.0 ** rng.uniform(-3, 3, n)).astype(F32)
    if mu is None:
        mu = rng.uniform(0.05, 5.0, n)
    mu = np.asarray(mu).astype(F32)
    z_range = rng.uniform(0.2, 20.0, n).astype(F32)
    sigma2 = (z_range.astype(F64) ** 2 / 10.0 ** rng.uniform(np.log10(36.0), np.log10(160000.0), n)).astype(F32)
    return a, b, mu, z_range, sigma2


def gen_life(n=40000, seed=101):
    rng = np.random.default_rng(seed)
    a, b, mu, z_range, sigma2 = life_state(n, rng)
    tau2 = (10.0 ** rng.uniform(-10, 0, n)).astype(F32)
    x = (mu + rng.normal(0, 1, n) * np.sqrt(sigma2.astype(F64) + tau2) * rng.choice([0.3, 1.0, 4.0, 40.0, 400.0], n)).astype(F32)
    return x, tau2, a, b, mu, z_range, sigma2


def gen_fresh(n=40000, seed=102):
    """a seed's first measurement (Seed::Seed: a = b = 10, sigma2 = z_range^2 / 36)"""
    rng = np.random.default_rng(seed)
    a = np.full(n, 10, F32)
    b = np.full(n, 10, F32)
    z_range = rng.uniform(0.2, 20.0, n).astype(F32)
    sigma2 = (z_range * z_range / F32(36)).astype(F32)
    mu = (rng.uniform(0.3, 0.9, n) * z_range).astype(F32)
    tau2 = (10.0 ** rng.uniform(-8, -1, n)).astype(F32)
    x = (mu + rng.normal(0, 1, n) * np.sqrt(sigma2.astype(F64) + tau2) * rng.choice([0.3, 1.0, 4.0], n)).astype(F32)
    return x, tau2, a, b, mu, z_range, sigma2


# (input, value, what the reference's arithmetic makes of the block): "untouched" = the NaN guard returns and no float is
# written; otherwise one letter per written float (a, b, mu, sigma2): N = NaN in every seed of the block, . = in none,
# ? = in some (the subnormals: x / tau2 or mu / sigma2 overflows, and inf - inf follows where m stays finite).  A zero
# variance poisons m = s2 * (mu / sigma2 + x / tau2) = 0 * inf and with it mu and sigma2; a = 0 or b = 0 makes e = f^2 and
# (e - f) / (f - e / f) = 0 / 0, which poisons a and b; a NaN measurement poisons everything.
SPECIAL_BLOCKS = (
    ("tau2", -1.0, "untouched"), ("tau2", 0.0, "..NN"), ("tau2", np.nan, "untouched"), ("tau2", np.inf, "...."), ("tau2", 1e-42, "..?N"),
    ("sigma2", np.nan, "untouched"), ("sigma2", 0.0, "..NN"), ("sigma2", -1e-9, "...."), ("sigma2", 1e-42, "..?N"),
    ("x", np.nan, "NNNN"), ("x", np.inf, "..NN"), ("x", -0.5, "...."),
    ("z_range", np.inf, "...."), ("a", 0.0, "NN.."), ("b", 0.0, "NN.."))
SPECIAL_BLOCK = 256


def gen_special(seed=103):
    """One block of SPECIAL_BLOCK seeds per entry of SPECIAL_BLOCKS over an otherwise benign state (the distribution of
    tests/test_oracle_seed_independent.py); returns the seven arrays and [(name, value, expectation, slice)]"""
    rng = np.random.default_rng(seed)
    n = SPECIAL_BLOCK * len(SPECIAL_BLOCKS)
    v = dict(a=rng.uniform(2, 40, n).astype(F32), b=rng.uniform(2, 40, n).astype(F32), mu=rng.uniform(0.2, 2.0, n).astype(F32),
             z_range=rng.uniform(0.5, 4.0, n).astype(F32))
    v["sigma2"] = (v["z_range"] * v["z_range"] / rng.uniform(36, 4000, n)).astype(F32)
    v["tau2"] = (10.0 ** rng.uniform(-6, -1, n)).astype(F32)
    v["x"] = (v["mu"] + rng.normal(0, 1, n) * np.sqrt(v["sigma2"] + v["tau2"])).astype(F32)
    blocks = []
    for k, (name, value, expect) in enumerate(SPECIAL_BLOCKS):
        sl = slice(k * SPECIAL_BLOCK, (k + 1) * SPECIAL_BLOCK)
        v[name][sl] = F32(value)
        blocks.append((name, value, expect, sl))
    return tuple(v[k] for k in SEED_ARGS), blocks


# ---- computeTau input families ----------------------------------------------------------------------------------------
TAU_FAMILIES = ("wide", "t_par_f", "t_eq_cf", "t_zero", "at_camera")
TAU_GROUPS, TAU_PER_GROUP = 200, 100                        # the kernel takes ONE translation per launch: 200 launches of 100
PX_ERROR_ANGLE = 2.0 * np.arctan(1.0 / (2.0 * 500.0))


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def gen_tau(family, seed=200):
    """(t [G,3], f [G,m,3], z [G,m]) float64: G translations with m unit bearings and depths each (compute_tau_kernel takes
    one translation per launch, so where a family ties t to f the bearings are built around the translation).
      wide       |t| = 10^U(-4, 0.5), z = 10^U(-2, 2), random bearings
      t_par_f    bearings within 10^U(-9, -2) of +-t / |t|: the acos arguments at +-1
      t_eq_cf    t = c f exactly (f = the rounded normalize(t), t recomputed from it)
      t_zero     no baseline
      at_camera  the point at the other camera centre: t = f z (1 + eps), eps = 0 or +-10^U(-16, -3)"""
    rng = np.random.default_rng(seed + TAU_FAMILIES.index(family))
    G, m = TAU_GROUPS, TAU_PER_GROUP
    tdir = _unit(rng.normal(size=(G, 3)))
    tlen = 10.0 ** rng.uniform(-4, 0.5, G)
    t = tdir * tlen[:, None]
    f = _unit(rng.normal(size=(G, m, 3)))
    z = 10.0 ** rng.uniform(-2, 2, (G, m))
    if family == "t_par_f":
        eps = 10.0 ** rng.uniform(-9, -2, (G, m, 1))
        f = _unit(tdir[:, None, :] + eps * rng.normal(size=(G, m, 3))) * rng.choice([-1.0, 1.0], (G, m, 1))
    elif family == "t_eq_cf":
        f = np.broadcast_to(_unit(tdir)[:, None, :], (G, m, 3)).copy()
        c = tlen * rng.choice([-1.0, 1.0], G)
        t = f[:, 0, :] * c[:, None]
    elif family == "t_zero":
        t = np.zeros((G, 3))
    elif family == "at_camera":
        f = np.broadcast_to(_unit(tdir)[:, None, :], (G, m, 3)).copy()
        z = np.broadcast_to(10.0 ** rng.uniform(-2, 2, (G, 1)), (G, m)).copy()
        eps = np.where(rng.uniform(size=G) < 0.3, 0.0, rng.choice([-1.0, 1.0], G) * 10.0 ** rng.uniform(-16, -3, G))
        t = f[:, 0, :] * (z[:, 0] * (1.0 + eps))[:, None]
        z = z * (1.0 + np.where(rng.uniform(size=(G, m)) < 0.5, 0.0, rng.choice([-1.0, 1.0], (G, m)) * 10.0 ** rng.uniform(-16, -3, (G, m))))
    return np.ascontiguousarray(t), np.ascontiguousarray(f), np.ascontiguousarray(z)


def tau_flat(t, f, z):
    """the per-element view of a family: t [n,3], f [n,3], z [n]"""
    G, m = z.shape
    return np.repeat(t, m, axis=0), f.reshape(G * m, 3), z.reshape(G * m)


# ---- scenes -----------------------------------------------------------------------------------------------------------
GLUE_BASELINES = (0.08, 0.004)
GLUE_FRAMES = 6


def glue_case(baseline, n=2048, seed=9):
    """The finalize glue (1/z -> f32, tau_inverse^2 -> f32, the 1e-7 clamp, updateSeed, the convergence test) on a 320x240
    scene: seed states per the life recipe with mu centred on 1 / true depth (2 % noise) so that matches happen.  With
    baseline 0.004 tau exceeds z for a large part of the seeds and max(1e-7, z - tau) clamps."""
    sc = seedsynth.make_seed_case(n_seeds=n, seed=seed, width=320, height=240, baseline=baseline, border=24)
    rng = np.random.default_rng(1000 + seed)
    n = len(sc.px)
    mu = (1.0 / sc.true_depth) * (1.0 + 0.02 * rng.normal(size=n))
    sc.a, sc.b, sc.mu, sc.z_range, sc.sigma2 = life_state(n, rng, mu=mu)
    return sc


def T_ref_cur_of(sc, T_cur_w=None):
    return synth.se3_mul(sc.T_ref_w, synth.se3_inv(sc.T_cur_w if T_cur_w is None else T_cur_w))


def clamp_mask(sc, o, T_cur_w=None):
    """seeds of an oracle pass `o` whose finalize takes the clamp branch: matched, and z - tau < 1e-7"""
    T = T_ref_cur_of(sc, T_cur_w)
    pea = 2.0 * np.arctan(1.0 / (2.0 * abs(sc.cam.fx)))
    out = np.zeros(len(sc.px), bool)
    for i in np.where(o["status"] >= 3)[0]:
        out[i] = not (1e-7 < o["z"][i] - orc.compute_tau(T, sc.f[i], o["z"][i], pea))
    return out


def oracle_pass(sc, state, T_cur_w=None, cur_pyr=None):
    """orc.update_seeds on copies of state = (a, b, mu, sigma2); returns (outputs, new state)"""
    a, b, mu, s2 = (np.ascontiguousarray(v, dtype=F32).copy() for v in state)
    o = orc.update_seeds(sc.cam, sc.ref_pyr, sc.cur_pyr if cur_pyr is None else cur_pyr, sc.T_ref_w,
                         sc.T_cur_w if T_cur_w is None else T_cur_w, sc.px, sc.f, sc.level, a, b, mu, sc.z_range.copy(), s2)
    return o, (a, b, mu, s2)


ODD_SIZES = ((346, 260), (202, 134), (100, 68))
ODD_MIN_STATUS, ODD_MIN_MULTI, ODD_MIN_DIRECT = 50, 20, 20      # what every size reaches on the oracle (statuses 0..3 each)


@dataclasses.dataclass
class OddCase:
    sc: seedsynth.SeedCase
    T_cur_w: np.ndarray        # the rotated current pose the pass runs with (the images are those of sc.T_cur_w)


# n seeds, scene seed, baseline, border, rotation of the current pose [rad], levels.  The camera keeps its 500 px focal
# length at every size, so baseline and rotation shrink with the image: with the 0.35 / 0.22 rad of the 640x480 test the
# tight block leaves the field of view and no seed takes the direct-align path.
_ODD_RECIPE = {
    (346, 260): dict(n=3000, seed=31, baseline=0.18, border=7, rot=0.06, levels=(0, 0, 0, 1, 2)),
    (202, 134): dict(n=2400, seed=32, baseline=0.10, border=7, rot=0.04, levels=(0, 0, 0, 1, 2)),
    (100, 68): dict(n=1500, seed=33, baseline=0.10, border=7, rot=0.02, levels=(0, 0, 1)),
}


def odd_df_case(width, height):
    """The branch-covering state recipe of test_depth_filter_all_paths scaled down to an image whose pyramid levels have
    odd widths: tight (direct align), loose (multi-chunk), far, negative mu, NaN variance and absurdly loose blocks; a
    rotated current pose so that seeds leave the frame; a border small enough that patches touch the image edge."""
    r = _ODD_RECIPE[(width, height)]
    sc = seedsynth.make_seed_case(n_seeds=r["n"], seed=r["seed"], width=width, height=height, baseline=r["baseline"],
                                  border=r["border"], levels=r["levels"])
    n = len(sc.px)
    T_cur_w = synth.se3_mul(synth.se3_from_twist([0.0, 0.0, 0.0], [0.0, r["rot"], 0.0]), sc.T_cur_w)
    k = n // 6
    q = max(60, n // 30)
    s2, mu = sc.sigma2, sc.mu
    s2[:k] *= 1e-4                                   # tight: epipolar segment < 2 px -> direct align
    s2[k:2 * k] *= 30.0                              # loose: long epipolar lines (multi-chunk searches)
    mu[2 * k:2 * k + q] = 1e-3                       # very far hypothesis
    mu[2 * k + q:2 * k + 2 * q] = -0.2               # negative inverse depth: behind the camera
    s2[2 * k + 2 * q:2 * k + 2 * q + 20] = np.nan    # NaN variance
    s2[3 * k:3 * k + q] *= 20000.0                   # absurdly loose: > 1000 steps -> search skipped
    return OddCase(sc, T_cur_w)


def odd_branch_counts(o):
    """(status histogram [6], multi-chunk searches, direct-align seeds) of an oracle pass"""
    return (np.bincount(o["status"], minlength=6), int((o["n_zmssd"] > 64).sum()),
            int(((o["n_zmssd"] == 0) & (o["n_align_iters"] > 0)).sum()))


def odd_align_case(width, height, level, n=600):
    """seedsynth.make_align_case patches of one pyramid level of an odd-sized image: returns (AlignCase, level image,
    pwb, patch, px_init, dirs) with the patches cut from THAT level around integer centres, a part of them within 5-8 px
    of the right and bottom borders (the closest a 10x10 bordered patch and the kernels' row loads get to the row end
    and to the end of the level)"""
    ac = seedsynth.make_align_case(n=n, seed=40 + level, width=width, height=height)
    rng = np.random.default_rng(900 + 10 * level + width)
    img = ac.cur_pyr[level]
    h, w = img.shape
    cx = rng.integers(6, w - 5, n)
    cy = rng.integers(6, h - 5, n)
    e = n // 4
    cx[:e] = w - rng.integers(5, 9, e)               # 5-8 px from the right border
    cy[e:2 * e] = h - rng.integers(5, 9, e)          # ... the bottom border
    cx[2 * e:2 * e + e // 2] = w - rng.integers(5, 9, e // 2)      # ... the bottom-right corner: the end of the level
    cy[2 * e:2 * e + e // 2] = h - rng.integers(5, 9, e // 2)
    iy = cy[:, None, None] + np.arange(-5, 5)[None, :, None]
    ix = cx[:, None, None] + np.arange(-5, 5)[None, None, :]
    noisy = img[iy, ix].astype(np.int64) + rng.integers(-3, 4, (n, 10, 10))     # residuals do not vanish at the optimum
    pwb = np.ascontiguousarray(np.clip(noisy, 0, 255).astype(np.uint8).reshape(n, 100))
    patch = np.ascontiguousarray(pwb.reshape(n, 10, 10)[:, 1:9, 1:9].reshape(n, 64))
    px_init = np.stack([cx, cy], axis=1) + rng.uniform(-1.5, 1.5, (n, 2))
    dirs = _unit(rng.normal(size=(n, 2))).astype(F32)
    return ac, img, pwb, patch, np.ascontiguousarray(px_init), np.ascontiguousarray(dirs)


def check_special_blocks(inputs, blocks, out4, what=""):
    """the expectation of every special block on a result (a, b, mu, sigma2): untouched blocks bit for bit, NaN blocks NaN"""
    before = (inputs[2], inputs[3], inputs[4], inputs[6])
    for name, value, expect, sl in blocks:
        tag = "%s %s = %r" % (what, name, value)
        for k, field in enumerate(("a", "b", "mu", "sigma2")):
            if expect == "untouched":
                np.testing.assert_array_equal(out4[k][sl].view(np.uint32), before[k][sl].view(np.uint32), err_msg=tag + ": " + field)
            elif expect[k] == "N":
                assert np.isnan(out4[k][sl]).all(), (tag, field)
            elif expect[k] == ".":
                assert not np.isnan(out4[k][sl]).any(), (tag, field)
            else:
                assert np.isnan(out4[k][sl]).any() and not np.isnan(out4[k][sl]).all(), (tag, field)
