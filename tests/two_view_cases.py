"""The input families of the two-view tests (tests/test_two_view_model_cpu.py proves what each reaches; the twin and the GPU tests
run the same cases): correspondences from a synthetic 3-D VOLUME -- depths spread over a factor of three, a known (R, t),
exact bearings -- with constructed outliers, gate boundaries, border pixels, median cases, poses and degenerate scenes."""
import functools

import numpy as np

import two_view_reference as M

W, H = 160, 120
FX, FY, CX, CY = 0.78 * W, 0.8 * W, W / 2 - 0.5, H / 2 + 1.25
THRESH_PX = 2.0
OUTLIER_PX = 20 * THRESH_PX              # a constructed outlier is at least this far from its epipolar line in both images


def rot(w):
    w = np.asarray(w, float)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


R_TRUE = rot([0.02, -0.05, 0.03])
T_TRUE = np.array([0.35, 0.06, 0.04])


def unproject(px):
    px = np.asarray(px, float)
    f = np.stack([(px[:, 0] - CX) / FX, (px[:, 1] - CY) / FY, np.ones(len(px))], axis=1)
    return f / np.linalg.norm(f, axis=1)[:, None]


def project(X):
    return np.stack([FX * X[:, 0] / X[:, 2] + CX, FY * X[:, 1] / X[:, 2] + CY], axis=1)


def epi_dist_px(px_ref, px_cur, R=R_TRUE, t=T_TRUE):
    """the distances in pixels of each point from the epipolar line of its partner, (in cur, in ref)"""
    Kinv = np.array([[1 / FX, 0, -CX / FX], [0, 1 / FY, -CY / FY], [0, 0, 1]])
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Fm = Kinv.T @ tx @ R @ Kinv
    x1 = np.concatenate([px_ref, np.ones((len(px_ref), 1))], axis=1)
    x2 = np.concatenate([px_cur, np.ones((len(px_cur), 1))], axis=1)
    l2, l1 = x1 @ Fm.T, x2 @ Fm
    d = np.abs(np.sum(l2 * x2, axis=1))
    return d / np.hypot(l2[:, 0], l2[:, 1]), d / np.hypot(l1[:, 0], l1[:, 1])


def volume(rng, n, R=R_TRUE, t=T_TRUE, planar=False, margin=12.0):
    """n true correspondences: (px_ref, px_cur) f32, exact unit bearings of the 3-D points, depths 2..6 in the first frame"""
    pr, pc, fr, fc = [], [], [], []
    while len(pr) < n:
        m = 4 * n
        p = np.stack([rng.uniform(margin, W - margin, m), rng.uniform(margin, H - margin, m)], axis=1)
        depth = np.full(m, 4.0) if planar else rng.uniform(2.0, 6.0, m)
        b = unproject(p)
        X = b * (depth / b[:, 2])[:, None]
        Xc = X @ R.T + t
        q = project(Xc)
        ok = (q[:, 0] >= margin) & (q[:, 0] < W - margin) & (q[:, 1] >= margin) & (q[:, 1] < H - margin)
        for i in np.nonzero(ok)[0][:n - len(pr)]:
            pr.append(p[i]); pc.append(q[i]); fr.append(X[i] / np.linalg.norm(X[i])); fc.append(Xc[i] / np.linalg.norm(Xc[i]))
    return np.array(pr), np.array(pc), np.array(fr), np.array(fc)


def outliers(rng, n):
    """n constructed outliers: random pixel pairs at least OUTLIER_PX from their epipolar lines in BOTH images"""
    pr, pc = [], []
    while len(pr) < n:
        a = np.stack([rng.uniform(12, W - 12, 256), rng.uniform(12, H - 12, 256)], axis=1)
        b = np.stack([rng.uniform(12, W - 12, 256), rng.uniform(12, H - 12, 256)], axis=1)
        d2, d1 = epi_dist_px(a, b)
        for i in np.nonzero((d1 >= OUTLIER_PX) & (d2 >= OUTLIER_PX))[0][:n - len(pr)]:
            pr.append(a[i]); pc.append(b[i])
    pr, pc = np.array(pr).reshape(-1, 2), np.array(pc).reshape(-1, 2)
    return pr, pc, unproject(pr), unproject(pc)


def make(scene_seed, n_in, n_out=0, noise=0.0, R=R_TRUE, t=T_TRUE, planar=False, T_ref_w=None, **params):
    rng = np.random.default_rng(scene_seed)
    pr, pc, fr, fc = volume(rng, n_in, R, t, planar)
    if noise:
        pr = pr + rng.uniform(-noise, noise, pr.shape)
        pc = pc + rng.uniform(-noise, noise, pc.shape)
        fr, fc = unproject(pr), unproject(pc)
    truth = np.ones(n_in + n_out, bool)
    if n_out:
        o = outliers(rng, n_out)
        pr, pc, fr, fc = (np.concatenate([a, b]) for a, b in zip((pr, pc, fr, fc), o))
        truth[n_in:] = False
        perm = rng.permutation(n_in + n_out)
        pr, pc, fr, fc, truth = pr[perm], pc[perm], fr[perm], fc[perm], truth[perm]
    prm = M.default_params()
    prm.update(params)
    return dict(px_ref=np.ascontiguousarray(pr, np.float32), px_cur=np.ascontiguousarray(pc, np.float32), f_ref=np.ascontiguousarray(fr),
                f_cur=np.ascontiguousarray(fc), truth=truth, T_ref_w=T_ref_w, params=prm, R=R, t=t, expect=M.OK)


def _volume(n):
    return make(100 + n, n, min_inliers=min(40, n))


def _outliers(n, frac, noise):
    n_out = int(round(n * frac))
    # the sampler's seed of the noisy 45 % case at n = 400 was chosen on the CPU: with seed 0 the best of its 1024 minimal
    # samples is not the true model (1 - (1 - w^8)^1024 is 0.99 only for w >= 0.51)
    seed = 5 if (n, frac, noise) == (400, 0.45, 0.3) else 0
    return make(7 + n + int(frac * 100) + int(noise * 10), n - n_out, n_out, noise, seed=seed)


def _gate_few():
    c = make(3, 7)
    c["expect"] = M.TOO_FEW
    return c


def _gate_identical():
    c = make(4, 60)
    for k in ("px_ref", "px_cur", "f_ref", "f_cur"):
        c[k][:] = c[k][0]
    c["expect"] = M.NO_MODEL
    return c


def _gate_cheirality():
    c = make(5, 80, 120)
    c["expect"] = M.CHEIRALITY
    return c


def _gate_inliers(k):
    c = make(6, k, 70 - k)
    c["expect"] = M.OK if k >= 40 else M.FEW_INLIERS
    return c


def _border():
    """the pixels of the first features are replaced (the gate of :123 reads the pixels alone): truncation to 9 / 10 and
    width - 11 / width - 10, likewise for the height, in either image.  (The singular 2 x 2 system is border-singular's.)"""
    c = make(8, 120)
    edge = [(9.99, 60.0), (10.0, 60.0), (W - 10.5, 60.0), (W - 10.0, 60.0), (80.0, 9.5), (80.0, 10.25), (80.0, H - 10.01), (80.0, H - 10.0)]
    want = [False, True, True, False, False, True, True, False]
    for i, e in enumerate(edge):
        c["px_ref"][i] = e
        c["px_cur"][8 + i] = e
    c["border_rows"], c["border_in"] = list(range(16)), want + want
    return c


def _border_singular():
    """the issue's pair of identical bearings stands for a singular 2 x 2 system; identical bearings are singular only under
    R = I, which cannot be arranged before R is known, so the singular system is reached with a zero bearing instead:
    a00 = a10 = 0, det = 0, invdet = inf, xyz = NaN.  An inlier under the reference's comparison that yields no point."""
    c = make(8, 120)
    c["f_cur"][16] = 0.0
    c["truth"][16] = False
    c["nan_row"] = 16
    return c


def _median(kind):
    if kind == "even":
        return make(9, 100)
    if kind == "odd":
        return make(9, 101)
    if kind == "run":                                # copies of one correspondence: a run of equal depths
        c = make(10, 90)
        z = M.two_view(c["f_ref"], c["f_cur"], c["px_ref"], c["px_cur"], FX, W, H)["xyz_in_cur"][:, 2]
        k = int(np.argsort(z)[45])                   # 45 depths below the twelve equal ones: rank 101 / 2 lies among them
        for key in ("px_ref", "px_cur", "f_ref", "f_cur"):
            c[key] = np.concatenate([c[key], np.repeat(c[key][k:k + 1], 11, axis=0)])
        c["truth"] = np.concatenate([c["truth"], np.ones(11, bool)])
        return c
    if kind == "negative":
        return make(11, 120, 60)
    c = make(12, 100)                                # one NaN depth
    c["f_cur"][17] = np.nan
    c["truth"][17] = False
    c["nan_row"] = 17
    return c


def _pose(map_scale):
    T = np.array([0.4, -0.2, 1.5, 0.0, 0.0, 0.0, 1.0])
    q = np.array([0.1, -0.2, 0.05, 0.97])
    T[3:] = q / np.linalg.norm(q)
    return make(13, 150, 30, T_ref_w=T, map_scale=map_scale)


def _degenerate(kind):
    if kind == "planar":
        c = make(14, 150, planar=True)
    else:
        c = make(15, 150, t=np.zeros(3))
    c["expect"] = None
    return c


FAMILIES = {}
for _n in (8, 9, 63, 64, 65, 257, 400, 1024):
    FAMILIES["volume-%d" % _n] = functools.partial(_volume, _n)
for _n in (200, 400):
    for _f in (0.30, 0.45):
        for _s in (0.0, 0.3):
            FAMILIES["outliers-%d-%d-%s" % (_n, int(_f * 100), _s)] = functools.partial(_outliers, _n, _f, _s)
FAMILIES.update({"gates-n7": _gate_few, "gates-identical": _gate_identical, "gates-cheirality": _gate_cheirality,
                 "gates-39": functools.partial(_gate_inliers, 39), "gates-40": functools.partial(_gate_inliers, 40), "border": _border,
                 "border-singular": _border_singular})
for _k in ("even", "odd", "run", "negative", "nan"):
    FAMILIES["median-" + _k] = functools.partial(_median, _k)
FAMILIES.update({"pose-1.0": functools.partial(_pose, 1.0), "pose-0.5": functools.partial(_pose, 0.5),
                 "degenerate-planar": functools.partial(_degenerate, "planar"), "degenerate-rotation": functools.partial(_degenerate, "rotation")})
NAMES = list(FAMILIES)


@functools.lru_cache(maxsize=None)
def case(name):
    return FAMILIES[name]()


@functools.lru_cache(maxsize=None)
def model(name):
    """the model's result of a family case, computed once and shared"""
    c = case(name)
    return M.two_view(c["f_ref"], c["f_cur"], c["px_ref"], c["px_cur"], FX, W, H, T_ref_w=c["T_ref_w"], **c["params"])
