"""An independent reference of FastDetector::detect (S/feature_detection.cpp:77-122) in plain numpy, and the scenes the
detector's edge-case tests run (tests/test_oracle_detect_edges.py on the CPU, tests/test_gpu_detect_edges.py on the device).
Nothing here comes from oracle/svo_oracle.c:

  fast_scores       FAST-9/16 by its definition: a pixel 3 or more from every edge is a corner if 9 contiguous pixels of
                    its 16-pixel ring (with wrap-around) are all darker than v - t or all brighter than v + t; its score
                    is the largest threshold at which that still holds, found by raising the threshold one by one
  fast_keypoints    3x3 non-maximum suppression, strict, over scores that are 0 where there is no corner; row-major
  shi_tomasi        vk::shiTomasiScore (S/vision.cpp:113-154): integer gradient sums, then the reference's f32 operations
                    in its order, with the border rule that returns 0
  detect            the sequential loop: levels in order, corners row-major, one float32 score per cell that starts at
                    float32(threshold) and is replaced on a strict >, the final test against the double threshold

The final test is where the reference has a quirk that is kept: Corner::score is a float, detection_threshold a double.
For a threshold whose f32 rounding lies above it (10.1, 0.1, 1e-3) every cell that found no winner still passes
`score > detection_threshold` and yields Feature(px (0,0), level 0), with score float32(threshold): a phantom."""
import functools

import numpy as np

from android_svo_amd import synth

DX = (0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1)
DY = (3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3)
FAST_T = 10                                      # cv::FAST(img, kp, 10, true)   (:91-94)


# ---- FAST -------------------------------------------------------------------------------------------------------------
def _arc9(hit):
    """hit [16, n] bool -> [n] bool: some 9 contiguous ring positions (with wrap-around) are all set"""
    out = np.zeros(hit.shape[1], dtype=bool)
    for s in range(16):
        run = hit[s].copy()
        for j in range(1, 9):
            run &= hit[(s + j) % 16]
        out |= run
    return out


def fast_scores(img, t=FAST_T):
    """[h, w] int32: the FAST score of every pixel, 0 where it is no corner at threshold t"""
    img = np.asarray(img, dtype=np.uint8)
    h, w = img.shape
    score = np.zeros((h, w), dtype=np.int32)
    if h < 7 or w < 7:
        return score                                                             # no pixel is 3 from every edge
    v = img[3:h - 3, 3:w - 3].astype(np.int32).ravel()
    d = np.stack([v - img[3 + DY[k]:h - 3 + DY[k], 3 + DX[k]:w - 3 + DX[k]].astype(np.int32).ravel() for k in range(16)])
    best = np.zeros(v.shape, dtype=np.int32)
    alive = np.arange(len(v))
    s = t
    while len(alive) and s <= 255:               # raise the threshold while some pixel is still a corner
        da = d[:, alive]
        still = _arc9(da > s) | _arc9(da < -s)
        alive = alive[still]
        best[alive] = s
        s += 1
    score[3:h - 3, 3:w - 3] = best.reshape(h - 6, w - 6)
    return score


def fast_keypoints(img, t=FAST_T):
    """(xs, ys, scores) of the corners that survive the strict 3x3 suppression, in row-major order"""
    sc = fast_scores(img, t)
    h, w = sc.shape
    keep = sc > 0
    pad = np.zeros((h + 2, w + 2), dtype=np.int32)
    pad[1:-1, 1:-1] = sc
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if (dx, dy) != (0, 0):
                keep &= sc > pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    ys, xs = np.nonzero(keep)                    # row-major
    return xs.astype(np.int32), ys.astype(np.int32), sc[ys, xs]


# ---- Shi-Tomasi -------------------------------------------------------------------------------------------------------
def shi_tomasi(img, u, v):
    """vk::shiTomasiScore(img, u, v) as np.float32"""
    f32 = np.float32
    rows, cols = img.shape
    x_min, x_max, y_min, y_max = u - 4, u + 4, v - 4, v + 4
    if x_min < 1 or x_max >= cols - 1 or y_min < 1 or y_max >= rows - 1:
        return f32(0.0)
    im = img.astype(np.int64)
    dx = im[y_min:y_max, x_min + 1:x_max + 1] - im[y_min:y_max, x_min - 1:x_max - 1]
    dy = im[y_min + 1:y_max + 1, x_min:x_max] - im[y_min - 1:y_max - 1, x_min:x_max]
    sxx, syy, sxy = int((dx * dx).sum()), int((dy * dy).sum()), int((dx * dy).sum())
    assert max(sxx, syy, abs(sxy)) < 1 << 24     # so the reference's running f32 sums are these integers, exactly
    dXX = f32(np.float64(f32(sxx)) / (2.0 * 64))                                 # float = float / double
    dYY = f32(np.float64(f32(syy)) / (2.0 * 64))
    dXY = f32(np.float64(f32(sxy)) / (2.0 * 64))
    tr = f32(dXX + dYY)
    det = f32(f32(dXX * dYY) - f32(dXY * dXY))
    arg = f32(f32(tr * tr) - f32(f32(4) * det))
    with np.errstate(invalid="ignore"):
        root = np.sqrt(arg)                      # sqrt(float), correctly rounded; NaN below 0 compares false everywhere
    return f32(0.5 * np.float64(f32(tr - root)))


# ---- FastDetector::detect ---------------------------------------------------------------------------------------------
_CANDIDATES = {}


def candidates(pyr, n_pyr_levels):
    """Every FAST corner of the first n_pyr_levels levels in the loop's order: a list of (level, x, y, shi_tomasi).
    Cached per pyramid (the levels' bytes are the key): grid, occupancy and threshold do not enter."""
    key = (n_pyr_levels,) + tuple((l.shape, l.tobytes()) for l in pyr[:n_pyr_levels])
    if key not in _CANDIDATES:
        out = []
        for L in range(n_pyr_levels):
            img = np.ascontiguousarray(pyr[L], dtype=np.uint8)
            xs, ys, _ = fast_keypoints(img)
            out += [(L, int(x), int(y), shi_tomasi(img, int(x), int(y))) for x, y in zip(xs, ys)]
        _CANDIDATES[key] = out
    return _CANDIDATES[key]


def grid(width, height, cell_size):
    return -(-width // cell_size), -(-height // cell_size)                       # ceil, :31-32


def cell_of(x, y, level, cell_size, grid_cols):
    f32 = np.float32                             # cv::KeyPoint::pt is float: (xy.y*scale)/cell_size_ is a float division
    return int(f32(y) * f32(1 << level) / f32(cell_size)) * grid_cols + int(f32(x) * f32(1 << level) / f32(cell_size))


def detect(pyr, n_pyr_levels=3, cell_size=20, occupancy=None, detection_threshold=10.0, trace=None):
    """-> px [n,2] int32 (level-0 pixel), level [n] int32, score [n] float32, in cell order.
    trace, if a dict, receives for every cell the list of (level, x, y, score) that reached the score comparison."""
    h, w = pyr[0].shape
    gc, gr = grid(w, h, cell_size)
    thr = float(detection_threshold)             # the double
    corners = [(0, 0, np.float32(thr), 0) for _ in range(gc * gr)]               # Corner(0, 0, detection_threshold, 0, 0.0f)
    for L, x, y, st in candidates(pyr, n_pyr_levels):
        k = cell_of(x, y, L, cell_size, gc)
        if occupancy is not None and occupancy[k]:
            continue
        if trace is not None:
            trace.setdefault(k, []).append((L, x, y, st))
        if st > corners[k][2]:                   # float against float, strict
            corners[k] = (x << L, y << L, st, L)
    keep = [c for c in corners if float(c[2]) > thr]                             # float against the double, strict
    px = np.array([(c[0], c[1]) for c in keep], dtype=np.int32).reshape(-1, 2)
    return px, np.array([c[3] for c in keep], dtype=np.int32), np.array([c[2] for c in keep], dtype=np.float32)


def cells_without_winner(pyr, n_pyr_levels, cell_size, occupancy, detection_threshold):
    """the number of cells whose score is still float32(threshold) after the loop"""
    trace = {}
    detect(pyr, n_pyr_levels, cell_size, occupancy, detection_threshold, trace)
    h, w = pyr[0].shape
    gc, gr = grid(w, h, cell_size)
    t32 = np.float32(detection_threshold)
    return sum(1 for k in range(gc * gr) if not any(c[3] > t32 for c in trace.get(k, [])))


def tie_cells(pyr, n_pyr_levels, cell_size, detection_threshold=10.0):
    """(cells where 2 or more corners share the cell's best score, those of them where the sharers span levels,
    {cell: first sharer in loop order})"""
    trace = {}
    detect(pyr, n_pyr_levels, cell_size, None, detection_threshold, trace)
    ties, cross, first = 0, 0, {}
    for k, cs in trace.items():
        best = max(c[3] for c in cs)
        if not best > np.float32(detection_threshold):
            continue
        sharers = [c for c in cs if c[3] == best]
        if len(sharers) >= 2:
            ties += 1
            cross += len({c[0] for c in sharers}) >= 2
            first[k] = sharers[0]
    return ties, cross, first


# ---- scenes -----------------------------------------------------------------------------------------------------------
ARC_LENGTHS = (8, 9, 10, 16)
ARC_CELL = 13
ARC_W, ARC_H = 213, 107
ARC_HIT_MISS = ((40, 10), (11, 10), (11, 0))


def stamp(img, cx, cy, start, length, polarity, hit, miss):
    """A FAST ring around (cx, cy): `length` pixels from ring position `start` on (with wrap-around) differ from the centre
    by `hit`, the others by `miss`; polarity +1 makes the ring darker than the centre, -1 brighter."""
    v = int(img[cy, cx])
    for k in range(16):
        inside = (k - start) % 16 < length
        img[cy + DY[k], cx + DX[k]] = v - polarity * (hit if inside else miss)


def arc_stamps():
    """the 128 (cx, cy, start, length, polarity) of the arcs scene: one per 13-px cell, 16 per row"""
    out = []
    for row, (polarity, length) in enumerate((p, n) for p in (1, -1) for n in ARC_LENGTHS):
        for start in range(16):
            out.append((ARC_CELL * start + 6, ARC_CELL * row + 6, start, length, polarity))
    return out


def arcs_scene(hit, miss):
    img = np.full((ARC_H, ARC_W), 100, dtype=np.uint8)
    for cx, cy, start, length, polarity in arc_stamps():
        stamp(img, cx, cy, start, length, polarity, hit, miss)
    return [img]


BORDER_W, BORDER_H = 107, 81


def border_stamps():
    """(cx, cy, edge, distance): arcs whose centres lie 3, 4 and 5 px from each image edge, one per 13-px cell and both
    polarities in turn.  FAST takes a centre 3 px from the edge; vk::shiTomasiScore returns 0 closer than 5 px."""
    out = []
    for i, dist in enumerate((3, 4, 5)):
        along = 26 + 13 * i + 6                  # cells 2, 3, 4 along the edge: clear of the corners of the image
        out.append((dist, along, "left", dist))
        out.append((BORDER_W - 1 - dist, along, "right", dist))
        out.append((along, dist, "top", dist))
        out.append((along, BORDER_H - 1 - dist, "bottom", dist))
    return out


def border_scene(hit=40, miss=10):
    img = np.full((BORDER_H, BORDER_W), 100, dtype=np.uint8)
    for i, (cx, cy, _, _) in enumerate(border_stamps()):
        stamp(img, cx, cy, (5 * i) % 16, 9 + i % 3, 1 if i % 2 else -1, hit, miss)
    return [img]


def ties_scene():
    """A 20x20 motif tiled over 100 x 68; levels 1 and 2 are crops of level 0, so the same corners, with the same
    Shi-Tomasi scores, come up again in other levels and in other cells of the same level."""
    motif = np.random.default_rng(5).integers(0, 256, (20, 20)).astype(np.uint8)
    motif[6:13, 6:13] = 240
    img = np.ascontiguousarray(np.tile(motif, (4, 5))[:68, :100])
    return [img, np.ascontiguousarray(img[:34, :50]), np.ascontiguousarray(img[:17, :25])]


def plateaus_scene():
    rng = np.random.default_rng(11)
    img = np.kron(rng.integers(0, 2, (34, 50)) * 255, np.ones((2, 2), dtype=np.int64)).astype(np.uint8)
    return synth.build_pyramid(img, 3)


def quantised_scene():
    rng = np.random.default_rng(12)
    img = rng.choice(np.array([89, 90, 100, 110, 111], dtype=np.uint8), (68, 100))
    return synth.build_pyramid(img, 3)


def half_flat_scene():
    rng = np.random.default_rng(13)
    img = np.full((68, 100), 90, dtype=np.uint8)
    img[:, :50] = rng.integers(0, 256, (68, 50))
    return synth.build_pyramid(img, 3)


def tiny_scene():
    rng = np.random.default_rng(14)
    img = rng.integers(0, 256, (12, 20)).astype(np.uint8)
    img[3:8, 6:12] = 255
    return synth.build_pyramid(img, 3)           # 20x12, 10x6, 5x3: only level 0 has pixels 3 from every edge


@functools.lru_cache(maxsize=None)
def half_flat_median_score():
    """the median score returned on half-flat at the default threshold: a threshold that sits on a real score"""
    _, _, sc = detect(half_flat_scene(), 3, 20, None, 10.0)
    return np.sort(sc)[len(sc) // 2]


def half_flat_thresholds():
    s = half_flat_median_score()
    return [10.0, 20.0, 0.0, 10.1, 0.1, 1e-3, 0.9, float(s), float(np.nextafter(s, np.float32(0))), float("inf"),
            float("nan"), -0.0]


PHANTOM_THRESHOLDS = (10.1, 0.1, 1e-3)


def slot_scenes():
    """three 100 x 68 pyramids of 3 levels for the three slots of one batch"""
    return [ties_scene(), half_flat_scene(), quantised_scene()]


SLOT_RUNS = ((20, 10.0), (20, 10.1), (25, 0.0))                                  # (cell_size, threshold) on every slot
SLOT_GRID_SEQUENCE = ((1, 10.0), (40, 10.0), (1, 10.1), (40, 10.1), (13, 0.0))   # 6800 cells, then 6 on the same scratch


def cases():
    """Every (name, pyramid, n_pyr_levels, cell_size, occupancy, detection_threshold) both test files run."""
    out = []
    for hit, miss in ARC_HIT_MISS:
        out.append(("arcs-%d-%d" % (hit, miss), arcs_scene(hit, miss), 1, ARC_CELL, None, 0.0))
    out.append(("border", border_scene(), 1, ARC_CELL, None, 0.0))
    ties = ties_scene()
    for cell in (40, 20, 25):
        out.append(("ties-%d" % cell, ties, 3, cell, None, 10.0))
    out.append(("plateaus", plateaus_scene(), 3, 20, None, 10.0))
    out.append(("plateaus-0", plateaus_scene(), 3, 20, None, 0.0))
    out.append(("quantised", quantised_scene(), 3, 20, None, 0.0))
    hf = half_flat_scene()
    for thr in half_flat_thresholds():
        out.append(("half-flat-%r" % thr, hf, 3, 20, None, thr))
    ones = np.ones(20, dtype=np.uint8)
    out.append(("half-flat-occupied-10.0", hf, 3, 20, ones, 10.0))
    out.append(("half-flat-occupied-10.1", hf, 3, 20, ones, 10.1))
    some = (np.arange(20) % 3 == 0).astype(np.uint8)
    out.append(("half-flat-some-occupied-10.1", hf, 3, 20, some, 10.1))
    tiny = tiny_scene()
    for cell in (40, 1):
        for thr in (0.0, 10.0, 10.1):
            out.append(("tiny-%d-%r" % (cell, thr), tiny, 3, cell, None, thr))
    return out
