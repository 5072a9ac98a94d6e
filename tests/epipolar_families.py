"""Constructed inputs for Matcher::findEpipolarMatchDirect that reach, by construction, the data-dependent paths of the
search kernel (df_search_block), and the kernel's path conditions restated as predicates over the oracle's trace.

Plain numpy, no GPU.  A family is a list of Case objects (a case = one camera, one pair of pyramids, one pair of poses, n
seeds: what one call of hip.epipolar_match_batch takes).  The predicates only say which path a seed takes -- the tests use
them to assert that a family reaches what it claims, never to compute an expected result (that is the oracle's).

Geometry used throughout: the reference frame is the world (T_ref_w = identity), so T_cur_ref = T_cur_w.  A reference
bearing f (unit vector) at distance d is the point f*d; with a pure translation t the point of z-depth z = f.z*d lands
fx*|t|/z level-0 pixels from the reference pixel ("disparity"), which is how the depth intervals below are chosen.
The levels of a pyramid here are independent images: the search reads cur[search_level] and ref[level_ref] only.
"""
import dataclasses
import math
from typing import List

import numpy as np

from android_svo_amd import synth

W, H, N_LEVELS = 160, 120, 3
ZMSSD_THRESHOLD = 128000
IDENTITY = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])


@dataclasses.dataclass
class Case:
    name: str
    cam: synth.Camera
    ref_pyr: List[np.ndarray]
    cur_pyr: List[np.ndarray]
    T_cur_w: np.ndarray
    px: np.ndarray
    level: np.ndarray
    d_est: np.ndarray
    d_min: np.ndarray
    d_max: np.ndarray
    tags: List[str]
    max_steps: int = 1000
    ref_slot: int = 0                    # the reference pyramid's slot in a batch of n_ref_slots (the others hold another image)
    n_ref_slots: int = 1
    T_ref_w: np.ndarray = dataclasses.field(default_factory=lambda: IDENTITY.copy())
    f: np.ndarray = None

    def __post_init__(self):
        self.px = np.ascontiguousarray(self.px, dtype=np.float64).reshape(-1, 2)
        self.level = np.ascontiguousarray(self.level, dtype=np.int32)
        self.d_est, self.d_min, self.d_max = (np.ascontiguousarray(v, dtype=np.float64) for v in (self.d_est, self.d_min, self.d_max))
        if self.f is None:
            self.f = synth.cam2world(self.cam, self.px)
        n = len(self.px)
        assert len(self.level) == len(self.d_est) == len(self.d_min) == len(self.d_max) == len(self.tags) == n
        for l in range(N_LEVELS):
            assert self.ref_pyr[l].shape == self.cur_pyr[l].shape == (H >> l, W >> l) and self.ref_pyr[l].dtype == np.uint8

    @property
    def n(self):
        return len(self.px)

    @property
    def T_cur_ref(self):
        return self.T_cur_w.copy()       # T_ref_w is the identity

    def subset(self, idx, name=None):
        idx = np.asarray(idx, dtype=np.int64)
        return dataclasses.replace(self, name=name or self.name, px=self.px[idx], f=self.f[idx], level=self.level[idx],
                                   d_est=self.d_est[idx], d_min=self.d_min[idx], d_max=self.d_max[idx],
                                   tags=[self.tags[i] for i in idx])


class _Seeds:
    """collects the per-seed arrays of a case"""

    def __init__(self):
        self.px, self.level, self.d_est, self.d_min, self.d_max, self.tags = [], [], [], [], [], []

    def add(self, px, level, d_est, d_min, d_max, tag):
        self.px.append(px); self.level.append(level); self.d_est.append(d_est); self.d_min.append(d_min)
        self.d_max.append(d_max); self.tags.append(tag)

    def case(self, name, cam, ref_pyr, cur_pyr, T_cur_w, **kw):
        return Case(name, cam, ref_pyr, cur_pyr, np.asarray(T_cur_w, dtype=np.float64), np.array(self.px), self.level, self.d_est,
                    self.d_min, self.d_max, self.tags, **kw)


def _fz(cam, px):
    return float(synth.cam2world(cam, np.asarray(px, dtype=np.float64).reshape(1, 2))[0, 2])


def texture(rng, h, w):
    """noise with structure at two scales (the alignment needs gradients, the ZMSSD a distinct minimum)"""
    coarse = np.kron(rng.integers(0, 256, ((h + 1) // 2, (w + 1) // 2)), np.ones((2, 2), dtype=np.int64))[:h, :w]
    fine = rng.integers(0, 256, (h, w))
    return np.ascontiguousarray((0.65 * coarse + 0.35 * fine).astype(np.uint8))


def _textures(rng):
    return [texture(rng, H >> l, W >> l) for l in range(N_LEVELS)]


def _pose(t, theta_z=0.0):
    return np.array([t[0], t[1], t[2], 0.0, 0.0, math.sin(theta_z / 2), math.cos(theta_z / 2)]) if theta_z else \
        np.array([t[0], t[1], t[2], 0.0, 0.0, 0.0, 1.0])


# ---- numpy restatement of the search plan (for fillers and for the predicates; not a reference) --------------------
def project(cam, T_cur_ref, f, d):
    p = synth.se3_act(T_cur_ref, np.asarray(f) * d)
    return np.array([cam.fx * p[0] / p[2] + cam.cx, cam.fy * p[1] / p[2] + cam.cy])


def epi_length0(cam, T_cur_ref, f, d_min, d_max):
    """length of the epipolar segment in level-0 pixels"""
    return float(np.linalg.norm(project(cam, T_cur_ref, f, d_min) - project(cam, T_cur_ref, f, d_max)))


def with_fillers(case: Case) -> Case:
    """`case` interleaved one-to-one with seeds of other paths: a short segment (path 0), a very long one (path 2 where the
    pose allows) and a segment of three steps, in turn -- so that the four seeds of every wave differ."""
    s = _Seeds()
    T = case.T_cur_ref
    for j in range(case.n):
        s.add(case.px[j], case.level[j], case.d_est[j], case.d_min[j], case.d_max[j], case.tags[j])
        px = np.array([44.0 + 7 * (j % 11), 34.0 + 9 * (j % 7)])
        f = synth.cam2world(case.cam, px.reshape(1, 2))[0]
        kind = j % 3
        if kind == 0:
            s.add(px, 0, 2.0, 1.999, 2.001, "filler:short")
        elif kind == 1:
            s.add(px, 0, 2.0, 0.02, 50.0, "filler:long")
        else:
            lo, hi = 0.05, 2.5                                 # bisect d_min for a segment of 2.05 level-0 pixels
            for _ in range(80):
                mid = 0.5 * (lo + hi)
                if epi_length0(case.cam, T, f, mid, 2.5) > 2.05:
                    lo = mid
                else:
                    hi = mid
            s.add(px, 0, 2.0, hi, 2.5, "filler:3step")
    return s.case(case.name + "+fillers", case.cam, case.ref_pyr, case.cur_pyr, case.T_cur_w, max_steps=case.max_steps,
                  ref_slot=case.ref_slot, n_ref_slots=case.n_ref_slots)


# ---- predicates over the trace -------------------------------------------------------------------------------------
def evaluated(trace):
    return trace["score"] >= 0


def risky_chunks(trace, search_level, margin=None):
    """per 16-chunk: does a candidate lie within 1e-7 px of a rounding boundary of (int)(px / 2^L + 0.5), in x or y
    (the kernel then replays the serial uv chain for the chunk).  With `margin`, also asserts that the answer is the same
    for limits of 1e-7 -+ margin (the kernel tests uv0 + i*step, the trace holds the chain: they differ by ~1e-10 px)."""
    t = trace["px"] / float(1 << search_level) + 0.5
    dist = np.abs(t - np.rint(t))

    def chunks(limit):
        risky = (dist <= limit).any(axis=1)
        return [bool(risky[c:c + 16].any()) for c in range(0, len(trace), 16)]
    if margin is not None:
        assert chunks(1e-7 - margin) == chunks(1e-7 + margin)
    return chunks(1e-7)


def chunk_boxes(trace):
    """per 16-chunk: (width, height) in pixels of the bounding box of the evaluated candidates' 8x8 patches, None without any"""
    out = []
    for c in range(0, len(trace), 16):
        t = trace[c:c + 16]
        ev = evaluated(t)
        if not ev.any():
            out.append(None)
            continue
        x, y = t["pxi"][ev, 0], t["pxi"][ev, 1]
        out.append((int(x.max() - x.min()) + 8, int(y.max() - y.min()) + 8))
    return out


def tie_indices(trace):
    """indices of the evaluated candidates that share the minimum score"""
    ev = evaluated(trace)
    if not ev.any():
        return np.zeros(0, dtype=np.int64)
    m = trace["score"][ev].min()
    return np.nonzero(ev & (trace["score"] == m))[0]


def footprint(case: Case, i: int, search_level: int, n_pyr_levels: int = N_LEVELS):
    """Phase A of the kernel for seed i: the f32 inverse warp, the source box of the 10x10 patch and whether the kernel
    copies it into its 32x32 window (use_win) or gathers from memory.  A_cur_ref comes from the oracle's
    getWarpMatrixAffine; everything after it is formed here as the kernel forms it."""
    import ctypes as C
    from oracle import orc
    c = orc.camera(case.cam)
    A = np.zeros(4)
    T, px, f = orc.f64(case.T_cur_ref), orc.f64(case.px[i]), orc.f64(case.f[i])
    orc.lib().svo_orc_get_warp_matrix_affine(C.byref(c), C.byref(c), orc._p(px, C.c_double), orc._p(f, C.c_double),
                                             C.c_double(case.d_est[i]), orc._p(T, C.c_double), C.c_int(int(case.level[i])),
                                             orc._p(A, C.c_double))
    with np.errstate(all="ignore"):
        det = A[0] * A[3] - A[2] * A[1]
        invdet = np.float64(1.0) / det
        f32 = np.float32
        a00, a01, a10, a11 = f32(A[3] * invdet), f32(-A[1] * invdet), f32(-A[2] * invdet), f32(A[0] * invdet)
        lr = int(case.level[i])
        prx, pry = f32(f32(case.px[i, 0]) / f32(1 << lr)), f32(f32(case.px[i, 1]) / f32(1 << lr))
        out = {"D": float(det), "nan": bool(np.isnan(a00)), "use_win": False, "ww": None, "wh": None, "wx0": None, "wy0": None}
        lscale = f32(1 << search_level)
        qx, qy = [], []
        for cx, cy in ((-5, -5), (4, -5), (-5, 4), (4, 4)):
            ppx, ppy = f32(cx) * lscale, f32(cy) * lscale
            qx.append(f32(f32(a00 * ppx) + f32(a01 * ppy)) + prx)
            qy.append(f32(f32(a10 * ppx) + f32(a11 * ppy)) + pry)
        xmin, xmax, ymin, ymax = min(qx), max(qx), min(qy), max(qy)
        if out["nan"] or not (xmin > -1e6 and ymin > -1e6 and xmax < 1e6 and ymax < 1e6):
            return out
        rcols, rrows = case.cam.width >> lr, case.cam.height >> lr
        wx0, wy0 = max(int(math.floor(xmin)), 0), max(int(math.floor(ymin)), 0)
        wx1, wy1 = min(int(math.floor(xmax)), rcols - 2) + 1, min(int(math.floor(ymax)), rrows - 2) + 1
        ww, wh = wx1 - wx0 + 1, wy1 - wy0 + 1
        out.update(ww=ww, wh=wh, wx0=wx0, wy0=wy0, use_win=bool(0 < ww <= 32 and 0 < wh <= 32))
        # bytes the window fill reads past the end of the level (rows of 32 bytes from column wx0)
        out["overrun"] = max(0, (wy1 * rcols + wx0 + 31) - (rcols * rrows - 1)) if out["use_win"] else 0
    return out


# ---- what the search does, recomputed from a trace -- and four wrong variants of it ---------------------------------
def outcome(trace, variant=None):
    """(found, n_zmssd, winning index) of the search loop over a trace.  variant None = the reference's rule (the first of
    equal minima wins, strictly below the threshold, a candidate equal to its predecessor is skipped).  The wrong variants:
    "last_tie", "le_threshold", "no_dedupe_at_chunk" (candidate 16k is not compared with candidate 16k-1) and "late_tail"
    (every chunk after the first starts one step late: index i carries the candidate of index i+1)."""
    pxi, score, in_frame = trace["pxi"].copy(), trace["score"].copy(), trace["in_frame"].copy()
    n = len(trace)
    known = np.ones(n, dtype=bool)                 # is the score of (pxi) known from the trace
    if variant == "late_tail":
        for i in range(16, n):
            if i + 1 < n:
                pxi[i], score[i], in_frame[i] = trace["pxi"][i + 1], trace["score"][i + 1], trace["in_frame"][i + 1]
            else:
                known[i] = False
    by_px = {}
    for i in range(n):
        if trace["score"][i] >= 0:
            by_px[(int(trace["pxi"][i, 0]), int(trace["pxi"][i, 1]))] = int(trace["score"][i])
    last = (0, 0)
    best, best_i, n_eval = None, -1, 0
    for i in range(n):
        if not known[i]:
            continue
        p = (int(pxi[i, 0]), int(pxi[i, 1]))
        dup = p == last
        if variant == "no_dedupe_at_chunk" and i % 16 == 0:
            dup = False
        last = p
        if dup or not in_frame[i]:
            continue
        n_eval += 1
        s = by_px[p]                               # a pixel that is in frame has been scored somewhere in the trace
        below = s <= ZMSSD_THRESHOLD if variant == "le_threshold" else s < ZMSSD_THRESHOLD
        if below and (best is None or s < best or (variant == "last_tie" and s == best)):
            best, best_i = s, i
    return best is not None, n_eval, best_i


# ---- family: chunk_edges ---------------------------------------------------------------------------------------------
CHUNK_COUNTS = (3, 15, 16, 17, 31, 32, 33, 48, 49)


def _lateral_seed(s, cam, fxb, px_ref, level, D_B, D_A, D_true, tag):
    """a seed of a pure x- or y-translation of fx*|t| = fxb: the segment runs from disparity D_B (far end, d_max) to D_A
    (near end, d_min) level-0 pixels, the depth estimate sits at disparity D_true"""
    fz = _fz(cam, px_ref)
    s.add(px_ref, level, fxb / (fz * D_true), fxb / (fz * D_A), fxb / (fz * D_B), tag)


def chunk_edges():
    """Pure x-translation over a fronto-parallel textured plane (z = 2: 15 px of disparity), search level 0.  Segment
    lengths put n_steps + 1 at each of CHUNK_COUNTS (tags "count:N"), the reference pixel's sub-pixel position puts
    candidate 16 (32) on the same integer pixel as candidate 15 (31) or on the next one (tags "dup16", "nodup16", ...).
    Segments shorter than 2 px (tag "below2": path 0) fill one whole wave, seeds 24..27.  A second case runs with max_epi_search_steps = 40 around that limit (paths 1 and 2)."""
    rng = np.random.default_rng(101)
    cam = synth.Camera(W, H, 150.0, 150.0, 79.5, 59.5)
    b, fxb = 0.2, 30.0
    ref = _textures(rng)
    cur = [np.ascontiguousarray(np.roll(ref[l], 15 >> l, axis=1)) for l in range(N_LEVELS)]

    def add(s, row, N, dup_at=None, dup=False, length=None):
        n_steps = N - 1
        L = length if length is not None else (2.05 if n_steps == 2 else (n_steps + 0.5) * 0.7)
        D_B = 3.75 if L >= 14 else 15.0 - L / 2
        x = 20.0 + (row * 7) % 50
        tag = "count:%d" % N
        if dup_at is not None:
            step = L / n_steps
            x_prev = x + D_B + (dup_at - 2) * step               # candidate i sits at x + D_B + (i - 1) * step
            want = 0.1 if dup else 0.6                           # fraction of x_prev + 0.5: the next one rounds to the same / the next pixel
            x += (want - (x_prev + 0.5) % 1.0) % 1.0
            tag += ":%sdup%d" % ("" if dup else "no", dup_at)
        _lateral_seed(s, cam, fxb, np.array([x, 12.0 + 4 * row]), 0, D_B, D_B + L, 15.0, tag)

    s = _Seeds()
    row = 0
    for N in CHUNK_COUNTS:
        variants = [(None, False)]
        if N == 16:
            variants = [(None, False), (None, False)]
        if N >= 17:
            variants = [(16, True), (16, False)]
        if N >= 33:
            variants += [(32, True), (32, False)]
        for dup_at, dup in variants:
            add(s, row, N, dup_at, dup)
            row += 1
    add(s, row, 3, length=2.0 + 1e-9); s.tags[-1] = "count:3"; row += 1
    add(s, row, 3, length=1.95); s.tags[-1] = "below2"; row += 1
    # seeds 24..27: a whole wave without a search (any_search false) between waves that search
    assert len(s.px) == 24
    for k, length in enumerate((2.0 - 1e-9, 1.0, 1.95, 0.3)):
        add(s, 2 + 5 * k, 3, length=length); s.tags[-1] = "below2"
    add(s, 9, 17); add(s, 13, 33)
    main =s.case("chunk_edges", cam, ref, cur, _pose((b, 0, 0)))
    s = _Seeds()
    add(s, 3, 41); add(s, 7, 42); s.tags[-1] = "path2"; add(s, 11, 44, length=30.5); s.tags[-1] = "path2"; add(s, 15, 17)
    add(s, 19, 41, 32, True); add(s, 22, 40, 16, False)
    limit = s.case("chunk_edges_max40", cam, ref, cur, _pose((b, 0, 0)), max_steps=40)
    return [main, limit]


# ---- family: ties -----------------------------------------------------------------------------------------------------
def ties():
    """Reference and current level images of period 8 px along x (the current one = the reference shifted by 3): the ZMSSD
    of a candidate repeats exactly 8 px further on, so the minimum is shared by two or three candidates.  The far end of
    the segment is placed so that the first two of them fall into one chunk ("same") or into two ("cross"); search levels
    0 and 1.  A second case has a constant current image (every score equal) and a reference that is constant on its left."""
    rng = np.random.default_rng(202)
    cam = synth.Camera(W, H, 150.0, 150.0, 79.5, 59.5)
    b, fxb, shift = 0.4, 60.0, 3
    ref = []
    for l in range(N_LEVELS):
        h, w = H >> l, W >> l
        ref.append(np.ascontiguousarray(np.tile(rng.integers(0, 256, (h, 8)), (1, w // 8)).astype(np.uint8)))
    cur = [np.ascontiguousarray(np.roll(ref[l], shift, axis=1)) for l in range(N_LEVELS)]
    L = 24.85                                                       # level pixels: 36 candidates, three chunks
    s = _Seeds()
    for lvl, n_same, n_cross in ((0, 4, 4), (1, 3, 3)):
        sc = 1 << lvl
        for j in range(n_same + n_cross):
            same = j < n_same
            off = 1 if same else 5                                   # first match `off` level px after the far end
            D_B = ((shift - off) % 8 + 8) * sc
            x = (24 + 5 * j if lvl == 0 else 10 + j) * sc            # integer pixel of the reference level
            y = (20 + 9 * j if lvl == 0 else 12 + 5 * j) * sc
            _lateral_seed(s, cam, fxb, np.array([float(x), float(y)]), lvl, D_B, D_B + L * sc, D_B + off * sc,
                          "%s:L%d" % ("same" if same else "cross", lvl))
    periodic = s.case("ties", cam, ref, cur, _pose((b, 0, 0)))
    rng = np.random.default_rng(203)
    ref_c = _textures(rng)
    for l in range(N_LEVELS):
        ref_c[l][:, :(64 >> l)] = 77
    cur_c = [np.full((H >> l, W >> l), 77, dtype=np.uint8) for l in range(N_LEVELS)]
    s = _Seeds()
    for (x, y, lvl) in ((20.0, 30.0, 0), (33.0, 50.0, 0), (41.0, 71.0, 0), (24.0, 40.0, 1), (100.0, 30.0, 0), (80.0, 64.0, 1)):
        sc = 1 << lvl
        if x > 64:                                                   # textured reference patch: every score equal and non-zero
            _lateral_seed(s, cam, fxb, np.array([x, y]), lvl, 2.0 * sc, 2.0 * sc + L * sc, 9.0 * sc, "const_cur:L%d" % lvl)
        else:
            _lateral_seed(s, cam, fxb, np.array([x, y]), lvl, 10.0 * sc, 10.0 * sc + L * sc, 15.0 * sc, "const:L%d" % lvl)
    const = s.case("ties_const", cam, ref_c, cur_c, _pose((b, 0, 0)))
    return [periodic, const]


# ---- family: threshold ------------------------------------------------------------------------------------------------
# integer 8x8 difference patterns d (the listed values, zeros elsewhere) whose ZMSSD sum(d*d) - (sum d)^2 / 64 against the
# patch itself is exactly the key: |sum d| <= 1, so the truncating division contributes 0.  (A zero-sum pattern has an
# even sum of squares -- the two odd scores need sum d = +-1.)
THRESHOLD_PATTERNS = {
    127999: (200, -200, 120, -120, 80, -80, 40, -40, -45, -3, 18, 29),
    128000: (200, -200, 120, -120, 80, -80, 40, -40, 40, -40),
    128001: (200, -200, 120, -120, 80, -80, 40, -40, -40, 1, 40),
}


def threshold():
    """Noise images, identity warp (integer reference pixel, equal depth, level 0: the patch is the reference's bytes).
    The 8x8 block at the true position of the current image is the patch plus a pattern of THRESHOLD_PATTERNS, so the
    best score of the segment is exactly 127999, 128000 or 128001 (tags "score:N")."""
    rng = np.random.default_rng(303)
    cam = synth.Camera(W, H, 150.0, 150.0, 79.5, 59.5)
    b, fxb = 0.2, 30.0
    ref = [np.ascontiguousarray(rng.integers(0, 256, (H >> l, W >> l)).astype(np.uint8)) for l in range(N_LEVELS)]
    cur = [np.ascontiguousarray(rng.integers(0, 256, (H >> l, W >> l)).astype(np.uint8)) for l in range(N_LEVELS)]
    keys = sorted(THRESHOLD_PATTERNS)
    s = _Seeds()
    for j in range(18):
        key = keys[j % 3]
        vals = THRESHOLD_PATTERNS[key]
        assert sum(v * v for v in vals) - (sum(vals) ** 2) // 64 == key and abs(sum(vals)) <= 1
        d = np.zeros(64, dtype=np.int64)
        d[rng.permutation(64)[:len(vals)]] = vals
        d = d.reshape(8, 8)
        A = rng.integers(np.maximum(0, -d), np.minimum(255, 255 - d) + 1)      # noise like the background, with room for d
        assert A.min() >= 0 and A.max() <= 255 and (A + d).min() >= 0 and (A + d).max() <= 255
        xr, yr = (20 if j % 2 == 0 else 90), 12 + 12 * (j // 2)
        xt = xr + 15
        ref[0][yr - 4:yr + 4, xr - 4:xr + 4] = A
        cur[0][yr - 4:yr + 4, xt - 4:xt + 4] = A + d
        _lateral_seed(s, cam, fxb, np.array([float(xr), float(yr)]), 0, 9.3, 9.3 + 12.25, 15.0, "score:%d" % key)
    return [s.case("threshold", cam, ref, cur, _pose((b, 0, 0)))]


# ---- family: replay ---------------------------------------------------------------------------------------------------
REPLAY_PATTERNS = {"all": [True, True, True], "risky_clear": [True, False, False], "clear_risky": [False, True, True]}


def _replay_case(orient, lvl, pattern):
    """Identity rotation, translation along x ("h") or y ("v"); every reference feature on the row py = cy (column px = cx),
    so that its bearing has f.y == 0 (f.x == 0) exactly and the segment is a row (column) of the image -- up to the tiny
    translation across it that the partial patterns add.  With c = the principal point's coordinate across the segment,
    t = c / 2^L + 0.5 is an integer for "all" (every candidate on a rounding boundary: every chunk replays the chain), and
    2.5e-7 below one for the other two, where the cross translation moves t by fy * ty / z / 2^L along the segment: from
    clear to within 1e-7 ("clear_risky": the first chunk is fast, the second rebuilds the chain) or the other way round.
    All seeds of a case share z_min and z_max, so they share the pattern.  40 candidates = chunks of 16, 16, 8.
    The current image holds a copy of each seed's reference patch 22 or 31 level px along the segment (chunk 1 or 2)."""
    sc = 1 << lvl
    m = (60 if orient == "h" else 80) // sc
    delta = 0.0 if pattern == "all" else 2.5e-7
    c_cross = sc * (m - 0.5 - delta)
    cam = synth.Camera(W, H, 150.0, 150.0, 79.5, c_cross) if orient == "h" else synth.Camera(W, H, 150.0, 150.0, c_cross, 59.5)
    b = 0.2 * sc
    fxb = 150.0 * b
    D_B, D_A = 7.3 * sc, (7.3 + 27.65) * sc          # (not 7.5: with integer reference pixels candidate 1 would sit on a boundary along the segment)
    z_max, z_min = fxb / D_B, fxb / D_A
    t_cross = {"all": 0.0, "clear_risky": 2.3e-7 * sc * z_min / 150.0, "risky_clear": 1.9e-7 * sc * z_max / 150.0}[pattern]
    T = _pose((b, t_cross, 0)) if orient == "h" else _pose((t_cross, b, 0))
    rng = np.random.default_rng(400 + 10 * lvl + (0 if orient == "h" else 5) + list(REPLAY_PATTERNS).index(pattern))
    ref = [np.ascontiguousarray(rng.integers(0, 256, (H >> l, W >> l)).astype(np.uint8)) for l in range(N_LEVELS)]
    cur = [np.ascontiguousarray(rng.integers(0, 256, (H >> l, W >> l)).astype(np.uint8)) for l in range(N_LEVELS)]
    h, w = H >> lvl, W >> lvl
    # stripes along the segment's normal, plus a small ramp along the normal (the alignment needs a gradient both ways):
    # sampling half-way between two rows then gives the same stripes
    along_n = w if orient == "h" else h
    g = rng.integers(0, 240, along_n)
    hbg = rng.integers(0, 240, along_n)
    s = _Seeds()
    # (reference position, disparity of the copy) in level px along the segment: the copies do not overlap
    starts = {("h", 0): ((20, 22), (41, 31), (63, 22)), ("h", 1): ((9, 22), (11, 31), (30, 22)),
              ("v", 0): ((12, 22), (27, 31), (50, 22)), ("v", 1): ((6, 22), (7, 31), (17, 31))}[(orient, lvl)]
    for a, D_true in starts:
        hbg[a + D_true - 5:a + D_true + 5] = g[a - 5:a + 5]
        px = np.array([float(a * sc), cam.cy]) if orient == "h" else np.array([cam.cx, float(a * sc)])
        fz = _fz(cam, px)
        s.add(px, lvl, fxb / (D_true * sc) / fz, z_min / fz, z_max / fz, "%s:%s:L%d" % (pattern, orient, lvl))
    ramp_n = h if orient == "h" else w
    ramp = (3 * np.arange(ramp_n)) % 11
    if orient == "h":
        ref[lvl] = np.ascontiguousarray((g[None, :] + ramp[:, None]).astype(np.uint8))
        cur[lvl] = np.ascontiguousarray((hbg[None, :] + ramp[:, None]).astype(np.uint8))
    else:
        ref[lvl] = np.ascontiguousarray((g[:, None] + ramp[None, :]).astype(np.uint8))
        cur[lvl] = np.ascontiguousarray((hbg[:, None] + ramp[None, :]).astype(np.uint8))
    return s.case("replay_%s_%s_L%d" % (pattern, orient, lvl), cam, ref, cur, T)


def replay():
    return [_replay_case(o, l, p) for o in ("h", "v") for l in (0, 1) for p in REPLAY_PATTERNS]


# ---- family: warp_windows ---------------------------------------------------------------------------------------------
def _render_plane(cam, ref_pyr, T_cur_ref, z0):
    """the current pyramid of a fronto-parallel plane z = z0 of the reference frame textured with ref_pyr (level l with the
    level's intrinsics), for a pose that rotates about z and translates: bilinear, 0 outside"""
    R = synth.rot_matrix(T_cur_ref[3:])
    t = T_cur_ref[:3]
    out = []
    for l, img in enumerate(ref_pyr):
        sc = float(1 << l)
        fx, fy, cx, cy = cam.fx / sc, cam.fy / sc, cam.cx / sc, cam.cy / sc
        h, w = img.shape
        ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
        zc = z0 + t[2]
        pc = np.stack([(xs - cx) / fx * zc, (ys - cy) / fy * zc, np.full_like(xs, zc)], axis=-1) - t
        pr = pc @ R                                               # R^T (p_c - t)
        u, v = fx * pr[..., 0] / pr[..., 2] + cx, fy * pr[..., 1] / pr[..., 2] + cy
        ok = (u >= 0) & (v >= 0) & (u < w - 1) & (v < h - 1)
        u0, v0 = np.where(ok, np.floor(u), 0).astype(np.int64), np.where(ok, np.floor(v), 0).astype(np.int64)
        a, bb = u - u0, v - v0
        im = img.astype(np.float64)
        val = (1 - a) * (1 - bb) * im[v0, u0] + a * (1 - bb) * im[v0, u0 + 1] + (1 - a) * bb * im[v0 + 1, u0] + a * bb * im[v0 + 1, u0 + 1]
        out.append(np.ascontiguousarray(np.where(ok, val, 0).astype(np.uint8)))
    return out


WARP_ANGLES = (0, 45, 90, 180)
# (level_ref, determinant of A_cur_ref aimed at): both sides of the search-level thresholds 3 and 12
WARP_SWEEP = ((0, 0.64), (1, 2.9), (1, 3.1), (2, 2.9), (2, 3.1), (2, 11.9), (2, 12.1))
# scale r = z / (z + tz) of the warp for level_ref 0: the 10x10 patch covers 9 / r source pixels -- windows of 31, 32, 33, 38 columns
WARP_FAR_SCALES = (0.31, 0.298, 0.2885, 0.25)


def warp_windows():
    """The current camera moved back along z (and turned about z by WARP_ANGLES), so that the warp A_cur_ref = r * 2^level_ref
    * R(theta), r = z / (z + tz) with z the depth estimate: determinants on both sides of 3 and 12 ("sweep" cases, tz = 0.5)
    and source footprints on both sides of the 32-pixel window ("far" cases, tz = 3).  One sweep case also carries depth
    estimates of 0 (NaN inverse warp) and 1e-12 next to the healthy seeds."""
    cam = synth.Camera(W, H, 150.0, 150.0, 79.5, 59.5)
    cases = []
    for k, deg in enumerate(WARP_ANGLES):
        th = math.radians(deg)
        rng = np.random.default_rng(500 + k)
        ref = _textures(rng)
        # sweep
        tz, b, z0 = 0.5, 0.1, 2.0
        T = _pose((b, 0.0, tz), th)
        s = _Seeds()
        for j, (lr, D) in enumerate(WARP_SWEEP):
            r = math.sqrt(D / 4 ** lr)
            z = tz * r / (1 - r)
            px = np.array([72.0 + 4 * j, 56.0 + 2 * j])
            d = z / _fz(cam, px)
            s.add(px, lr, d, 0.8 * d, 1.3 * d, "sweep:lr%d:D%.1f:rot%d" % (lr, D, deg))
        if deg == 0:
            s.add(np.array([70.0, 64.0]), 0, 0.0, 1.5, 3.0, "nan_warp")
            s.add(np.array([84.0, 52.0]), 1, 0.0, 1.8, 2.2, "nan_warp")
            s.add(np.array([90.0, 66.0]), 0, 1e-12, 1.5, 3.0, "tiny_depth")
        cases.append(s.case("warp_sweep_rot%d" % deg, cam, ref, _render_plane(cam, ref, T, z0), T))
        # far
        tz, b, z0 = 3.0, 0.3, 1.2
        T = _pose((b, 0.0, tz), th)
        s = _Seeds()
        for j, r in enumerate(WARP_FAR_SCALES):
            z = tz * r / (1 - r)
            px = np.array([80.0 + 2 * j, 60.0 - j])
            d = z / _fz(cam, px)
            s.add(px, 0, d, 0.7 * d, 1.6 * d, "far:r%.4f:rot%d" % (r, deg))
        cases.append(s.case("warp_far_rot%d" % deg, cam, ref, _render_plane(cam, ref, T, z0), T))
    return cases


# ---- family: borders --------------------------------------------------------------------------------------------------
def borders():
    """Segments that enter or leave the frame band (8 px inside the search level's image) through each of its four sides at
    search levels 0, 1 and 2, reference features 3 px from each side of their level (samples outside the image: zeros; the
    window's corner clamped to 0), and -- its own case -- a reference feature at the bottom-right corner of level 2 of the
    last slot of a two-slot reference pyramid, whose window fill reads past the end of that level."""
    cam = synth.Camera(W, H, 150.0, 150.0, 79.5, 59.5)
    tnorm, fxb, D_true = 0.4, 60.0, 9
    cases = []
    for k, (sx, sy) in enumerate(((1, 0), (-1, 0), (0, 1), (0, -1))):
        rng = np.random.default_rng(600 + k)
        ref = _textures(rng)
        cur = [np.ascontiguousarray(np.roll(ref[l], (D_true * sy, D_true * sx), axis=(0, 1))) for l in range(N_LEVELS)]
        s = _Seeds()
        for lvl in range(N_LEVELS):
            sc = 1 << lvl
            n_al, n_cr = ((W, H) if sx else (H, W))
            n_al, n_cr = n_al >> lvl, n_cr >> lvl
            for kind, a_ref, D_B, D_A in (("enter", 3.3, 2.0, 11.0), ("leave", n_al - 22.3, 8.0, 19.0)):
                cross = n_cr / 2 + 1.7
                if sx + sy < 0:
                    a_ref = (n_al - 1) - a_ref
                p = np.array([a_ref, cross]) * sc if sx else np.array([cross, a_ref]) * sc
                _lateral_seed(s, cam, fxb, p, lvl, D_B * sc, D_A * sc, float(D_true * sc), "%s:L%d:dir%+d%+d" % (kind, lvl, sx, sy))
        # a reference feature in the corner of level 0: zeros on two sides, no candidate inside the band
        a_ref = 3.3 if sx + sy > 0 else (W if sx else H) - 1 - 3.3
        p = np.array([a_ref, 3.6]) if sx else np.array([3.6, a_ref])
        _lateral_seed(s, cam, fxb, p, 0, 2.0, 11.0, float(D_true), "corner:L0:dir%+d%+d" % (sx, sy))
        cases.append(s.case("borders_dir%+d%+d" % (sx, sy), cam, ref, cur, _pose((tnorm * sx, tnorm * sy, 0))))
    # the last bytes of the reference allocation: level 2 (40x30) of slot 1 of 2; the segment runs up and to the left into the band
    rng = np.random.default_rng(610)
    ref = _textures(rng)
    cur = [np.ascontiguousarray(np.roll(ref[l], (-7, -10), axis=(0, 1))) for l in range(N_LEVELS)]
    s = _Seeds()
    for (x2, y2) in ((36.5, 26.5), (35.25, 25.75)):
        px = np.array([x2, y2]) * 4
        fz = _fz(cam, px)
        s.add(px, 2, fxb / (10.0 * 4) / fz, fxb / (19.0 * 4) / fz, fxb / (8.0 * 4) / fz, "last_slot_corner:L2")
    cases.append(s.case("borders_last_slot", cam, ref, cur, _pose((-0.4, -0.28, 0)), ref_slot=1, n_ref_slots=2))
    return cases


FAMILIES = {"chunk_edges": chunk_edges, "ties": ties, "threshold": threshold, "replay": replay, "warp_windows": warp_windows,
            "borders": borders}

_cache = {}


def family(name) -> List[Case]:
    if name not in _cache:
        _cache[name] = FAMILIES[name]()
    return _cache[name]


_oracle_cache = {}


def oracle_results(case: Case):
    """[(EpiResult, trace)] of the oracle for every seed of a case (computed once per case object)"""
    from oracle import orc
    key = id(case)
    if key not in _oracle_cache:
        _oracle_cache[key] = (case, [orc.find_epipolar_match(case.cam, case.ref_pyr, case.cur_pyr, case.T_cur_ref, case.px[i], case.f[i],
                                                             int(case.level[i]), case.d_est[i], case.d_min[i], case.d_max[i],
                                                             n_pyr_levels=N_LEVELS, max_steps=case.max_steps, trace=True)
                                     for i in range(case.n)])
    return _oracle_cache[key][1]
