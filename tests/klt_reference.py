"""The bootstrap's KLT tracker restated in numpy: the definition the device kernels of csrc/svo_klt.hip are held to by bits.

cv::calcOpticalFlowPyrLK as KltHomographyInit::trackKlt calls it (S/initialization.cpp:180-226: 30 x 30 window, maxLevel 4,
30 iterations, eps 0.001, minEigThreshold 1e-4, OPTFLOW_USE_INITIAL_FLOW), written down from the algorithm OpenCV 4.5.4
implements (DESIGN.md section 7 lists the departures), and the erasures / bearings / disparities / upper median around it.

Every "float" is an IEEE f32 value and every operation is rounded on its own: all constants are wrapped in np.float32 so that
no intermediate is promoted.  The five window sums are exact integers, converted to f32 once (through f64, which holds them
exactly).  Two comparisons are evaluated in f64 as OpenCV does: delta.ddot(delta) <= eps * eps.
"""
import numpy as np

F = np.float32
FLT_EPSILON = F(1.1920929e-07)
K5 = np.array([1, 4, 6, 4, 1], dtype=np.int64)

# the exits of a feature at a level (regime counting in tests/test_klt_model_cpu.py)
EXIT_EPS, EXIT_OSC, EXIT_MAXCOUNT, EXIT_MINEIG, EXIT_PREV_OOB, EXIT_CUR_OOB, EXIT_FINAL_ROUND = range(7)
EXIT_NAMES = ["eps", "oscillation", "maxCount", "minEig/D", "previous window out of range", "current window out of range",
              "final rounding test"]


def default_params():
    return dict(win_size=30, max_level=4, max_iter=30, eps=1e-3, min_eig_threshold=1e-4)


def _reflect101(i, n):
    i = np.asarray(i).copy()
    while True:
        lo, hi = i < 0, i >= n
        if not (lo.any() or hi.any()):
            return i
        i[lo] = -i[lo]
        i[hi] = 2 * n - 2 - i[hi]


def pyr_down(img):
    """One Gaussian level: dst = (sum k_i k_j src(r(2x+j), r(2y+i)) + 128) >> 8, size ((w+1)/2, (h+1)/2)."""
    src = np.asarray(img, dtype=np.int64)
    h, w = src.shape
    dh, dw = (h + 1) // 2, (w + 1) // 2
    acc = np.zeros((dh, dw), dtype=np.int64)
    ys, xs = 2 * np.arange(dh), 2 * np.arange(dw)
    for i in range(-2, 3):
        rows = src[_reflect101(ys + i, h)]
        for j in range(-2, 3):
            acc += K5[i + 2] * K5[j + 2] * rows[:, _reflect101(xs + j, w)]
    return ((acc + 128) >> 8).astype(np.uint8)


def n_levels_for(width, height, win_size=30, max_level=4):
    """Levels 0..L of the Gaussian pyramid: level l+1 exists only while its width and its height exceed the window."""
    n, w, h = 1, width, height
    while n <= max_level:
        w, h = (w + 1) // 2, (h + 1) // 2
        if not (w > win_size and h > win_size):
            break
        n += 1
    return n


def build_pyramid(img, win_size=30, max_level=4):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    levels = [img]
    for _ in range(n_levels_for(img.shape[1], img.shape[0], win_size, max_level) - 1):
        levels.append(pyr_down(levels[-1]))
    return levels


def scharr(img):
    """(dx, dy) of one level with reflect-101 neighbours, int64 (the values fit int16)."""
    s = np.asarray(img, dtype=np.int64)
    h, w = s.shape
    up, dn = s[_reflect101(np.arange(h) - 1, h)], s[_reflect101(np.arange(h) + 1, h)]
    t0 = 3 * (up + dn) + 10 * s
    t1 = dn - up
    xl, xr = _reflect101(np.arange(w) - 1, w), _reflect101(np.arange(w) + 1, w)
    dx = t0[:, xr] - t0[:, xl]
    dy = 3 * (t1[:, xr] + t1[:, xl]) + 10 * t1
    return dx, dy


def _descale(v, n):
    return (v + (1 << (n - 1))) >> n


def _weights(a, b):
    one, s = F(1), F(16384)
    w00 = int(np.rint((one - a) * (one - b) * s))
    w01 = int(np.rint(a * (one - b) * s))
    w10 = int(np.rint((one - a) * b * s))
    return w00, w01, w10, 16384 - w00 - w01 - w10


def _in_range(fx, fy, W, cols, rows):
    # on the floats, before any conversion: a NaN or an infinity is out of range
    return bool(fx >= -W and fx < cols and fy >= -W and fy < rows)


def _to_f32(s):
    return F(np.float64(int(s)))


class _Level:
    """A level's images padded by the window: reflect-101 for image samples, zero for derivatives."""

    def __init__(self, prev, cur, W):
        self.rows, self.cols = prev.shape
        self.pad = W + 1
        p = self.pad
        ry, rx = _reflect101(np.arange(-p, self.rows + p), self.rows), _reflect101(np.arange(-p, self.cols + p), self.cols)
        self.P = np.asarray(prev, dtype=np.int64)[ry][:, rx]
        self.J = np.asarray(cur, dtype=np.int64)[ry][:, rx]
        dx, dy = scharr(prev)
        self.DX = np.pad(dx, p)
        self.DY = np.pad(dy, p)

    def interp(self, A, ix, iy, w, W, shift):
        y0, x0 = iy + self.pad, ix + self.pad
        a = A[y0:y0 + W + 1, x0:x0 + W + 1]
        return _descale(w[0] * a[:-1, :-1] + w[1] * a[:-1, 1:] + w[2] * a[1:, :-1] + w[3] * a[1:, 1:], shift)


def track(prev_pyr, cur_pyr, px_ref, px_cur, params=None, trace=None):
    """calcOpticalFlowPyrLK over all features.  Returns (status u8 [n], px_cur f32 [n, 2]).  trace: a list that receives
    (feature, level, exit) for every exit taken."""
    prm = default_params() if params is None else params
    W = int(prm["win_size"])
    half = F((W - 1) * 0.5)
    eps2 = float(prm["eps"]) * float(prm["eps"])
    min_eig = F(prm["min_eig_threshold"])
    L = min(int(prm["max_level"]), len(prev_pyr) - 1)
    lv = [_Level(prev_pyr[l], cur_pyr[l], W) for l in range(L + 1)]
    px_ref = np.asarray(px_ref, dtype=F).reshape(-1, 2)
    out = np.array(px_cur, dtype=F).reshape(-1, 2).copy()
    n = len(px_ref)
    status = np.ones(n, dtype=np.uint8)

    def note(k, level, what):
        if trace is not None:
            trace.append((k, level, what))

    with np.errstate(all="ignore"):
        for k in range(n):
            cx, cy = out[k]
            for level in range(L, -1, -1):
                g = lv[level]
                sc = F(1.0 / (1 << level))
                px, py = px_ref[k, 0] * sc, px_ref[k, 1] * sc
                if level == L:
                    nx, ny = cx * sc, cy * sc
                else:
                    nx, ny = cx * F(2), cy * F(2)
                cx, cy = nx, ny
                px, py = px - half, py - half
                fx, fy = np.floor(px), np.floor(py)
                if not _in_range(fx, fy, W, g.cols, g.rows):
                    if level == 0:
                        status[k] = 0
                    note(k, level, EXIT_PREV_OOB)
                    continue
                ix, iy = int(fx), int(fy)
                w = _weights(px - fx, py - fy)
                I = g.interp(g.P, ix, iy, w, W, 9)
                Ix = g.interp(g.DX, ix, iy, w, W, 14)
                Iy = g.interp(g.DY, ix, iy, w, W, 14)
                s20 = F(2.0 ** -20)
                A11, A12, A22 = _to_f32((Ix * Ix).sum()) * s20, _to_f32((Ix * Iy).sum()) * s20, _to_f32((Iy * Iy).sum()) * s20
                D = A11 * A22 - A12 * A12
                t = A11 - A22
                eig = (A22 + A11 - np.sqrt(t * t + F(4) * A12 * A12)) / F(2 * W * W)
                if eig < min_eig or D < FLT_EPSILON:
                    if level == 0:
                        status[k] = 0
                    note(k, level, EXIT_MINEIG)
                    continue
                D = F(1) / D
                nx, ny = nx - half, ny - half
                pdx, pdy = F(0), F(0)
                how = EXIT_MAXCOUNT
                for j in range(int(prm["max_iter"])):
                    fx, fy = np.floor(nx), np.floor(ny)
                    if not _in_range(fx, fy, W, g.cols, g.rows):
                        if level == 0:
                            status[k] = 0
                        how = EXIT_CUR_OOB
                        break
                    jx, jy = int(fx), int(fy)
                    diff = g.interp(g.J, jx, jy, _weights(nx - fx, ny - fy), W, 9) - I
                    b1, b2 = _to_f32((diff * Ix).sum()) * s20, _to_f32((diff * Iy).sum()) * s20
                    dx, dy = (A12 * b2 - A22 * b1) * D, (A12 * b1 - A11 * b2) * D
                    nx, ny = nx + dx, ny + dy
                    cx, cy = nx + half, ny + half
                    if float(dx) * float(dx) + float(dy) * float(dy) <= eps2:
                        how = EXIT_EPS
                        break
                    if j > 0 and abs(dx + pdx) < F(0.01) and abs(dy + pdy) < F(0.01):
                        cx, cy = cx - dx * F(0.5), cy - dy * F(0.5)
                        how = EXIT_OSC
                        break
                    pdx, pdy = dx, dy
                note(k, level, how)
                if status[k] and level == 0:
                    qx, qy = np.rint(cx - half), np.rint(cy - half)
                    if not _in_range(qx, qy, W, g.cols, g.rows):
                        status[k] = 0
                        note(k, level, EXIT_FINAL_ROUND)
            out[k] = (cx, cy)
    return status, out


def upper_median(v):
    """vk::getMedian: the order statistic of rank floor(n / 2); NaN for an empty list."""
    v = np.asarray(v, dtype=np.float64)
    if len(v) == 0:
        return float("nan")
    return float(np.sort(v)[len(v) // 2])


def track_klt(prev_pyr, cur_pyr, px_ref, px_cur, params=None, trace=None):
    """trackKlt (:203-225): the tracker, then the erasures.  Returns a dict with the surviving px_ref / px_cur (f32), keep
    (indices into the input), disparity (f64) and its upper median."""
    status, out = track(prev_pyr, cur_pyr, px_ref, px_cur, params, trace)
    keep = np.flatnonzero(status)
    ref = np.asarray(px_ref, dtype=F).reshape(-1, 2)[keep]
    cur = out[keep]
    d = (ref - cur).astype(np.float64)           # float differences, then double
    disp = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    return dict(status=status, px_all=out, keep=keep, px_ref=ref, px_cur=cur, disparity=disp, median=upper_median(disp))


# ---- test inputs shared by the CPU and the GPU tests -------------------------------------------------------------------
def sinusoid_texture(width, height, seed, shift=(0.0, 0.0), n_waves=40):
    """A texture of n_waves random sinusoids (|frequency| <= 0.35 rad/px) sampled analytically at (x - shift): the image
    content moves by +shift."""
    rng = np.random.RandomState(seed)
    fx, fy = rng.uniform(-0.35, 0.35, n_waves), rng.uniform(-0.35, 0.35, n_waves)
    ph, amp = rng.uniform(0, 2 * np.pi, n_waves), rng.uniform(0.5, 1.0, n_waves)
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    x, y = x - shift[0], y - shift[1]
    v = np.zeros((height, width))
    for i in range(n_waves):
        v += amp[i] * np.sin(fx[i] * x + fy[i] * y + ph[i])
    v = 127.5 + v * (100.0 / np.sqrt(n_waves))
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def gpu_case(width, height, n, seed, shift=(1.7, -0.9), flat=True):
    """The image pair and features of one GPU test case (n >= 24).  Random points around the whole image, and planted ones:
    the corners (0,0), (w-1,h-1); a point beyond the image (w+40, 5); integer window corners (x.5 coordinates: weights a = 0, b = 0); points on
    a flat 40 x 40 rectangle painted into both images (minEig at level 0); points whose window leaves the range while it
    moves with the content (right and top edge); and, where the image has room (width >= 300), a point in the middle of a
    100 x 100 region painted with 100 + P[x % 4] + Q[y % 4], P = [0, 40, 0, -40], Q = [0, 30, 0, -30]: the Gaussian level
    above it is exactly constant there (6 p0 + 4 (p1 + p3) + 2 p2 is the same at every even x), so the feature is lost at
    level 1 and found again at level 0."""
    assert n >= 24
    prev = sinusoid_texture(width, height, seed)
    cur = sinusoid_texture(width, height, seed, shift)
    rx, ry = width // 2 - 20, height // 2 - 20
    special = [(0, 0), (width - 1, height - 1), (width + 40, 5), (40, 50), (width // 2 + 0.5, 37.25)]
    if flat:
        prev[ry:ry + 40, rx:rx + 40] = 90
        cur[ry:ry + 40, rx:rx + 40] = 90
        special += [(rx + 20, ry + 20), (rx + 19.5, ry + 21.25)]
    if width >= 300:
        y, x = np.mgrid[0:100, 0:100]
        pat = (100 + np.array([0, 40, 0, -40])[x % 4] + np.array([0, 30, 0, -30])[y % 4]).astype(np.uint8)
        prev[30:130, 30:130] = pat
        cur[30:130, 30:130] = pat
        special += [(80.0, 80.0), (79.5, 81.25)]
    special += [(width - 3.5, height / 2), (14.0, 14.0), (5.25, height - 9.0), (width - 40.5, height - 30.5)]
    special += [(width + 13.9, height * t) for t in (0.2, 0.45, 0.7, 0.9)]
    special += [(width * t, -15.2) for t in (0.15, 0.4, 0.6, 0.85)]
    special += [(width + 14.3, height * 0.33), (width * 0.5, -15.45)]
    rng = np.random.RandomState(seed + 1000)
    px = np.stack([rng.uniform(-2, width + 2, n), rng.uniform(-2, height + 2, n)], axis=1).astype(F)
    px[:len(special)] = np.array(special, dtype=F)
    return prev, cur, px


def flow_case(width, height, seed, shift=(1.7, -0.9)):
    """Features that start with an initial flow (OPTFLOW_USE_INITIAL_FLOW with a motion prior, or the flow a previous frame
    left): reference points 8 px inside the right / bottom edge whose current window starts at the edge of the legal range,
    so that it leaves the range inside the loop or fails the final rounding test.  Returns prev, cur, px_ref, px_cur0."""
    prev, cur, _ = gpu_case(width, height, 24, seed, shift)
    ref, c0 = [], []
    for i in range(12):
        y = height * (0.15 + 0.06 * i)
        ref.append((width - 8.0, y))
        c0.append((width + 13.6 + 0.08 * i, y))
    for i in range(12):
        x = width * (0.15 + 0.06 * i)
        ref.append((x, height - 8.0))
        c0.append((x, height + 13.6 + 0.08 * i))
    return prev, cur, np.array(ref, dtype=F), np.array(c0, dtype=F)
