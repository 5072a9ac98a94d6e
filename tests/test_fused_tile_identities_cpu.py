"""What the scalar bookkeeping of the fused SparseImgAlign kernel's tile loop (svo_sia.hip) rests on where a select or a
shorter schedule took the place of branches, checked in numpy / plain Python on every case or on adversarial values:

1. the sign-and-scale factor of the wave reduction, selected on the two 32-bit words of 2 jscale instead of by a chain of f64
   conditionals: the same double, bit for bit, for every row j and every jscale;
2. the H row read by every lane with a clamped index instead of under an exec mask: lanes 0..20 read the same entry and add
   the same values in the same order, and no lane reads outside the row;
3. the priority schedule as three events (raise at tile 0, one drop): the priority a wave runs at in every half tile is what
   the per-tile schedule gave, for every shape and every number of tiles of the younger wave; at the heads of tiles that do
   not exist it differs in exactly one case, the one the kernel's comment names."""
import numpy as np


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def _jscales():
    rng = np.random.default_rng(99)
    # fx / 2^level of real cameras, and the ends of the range: tiny, huge, subnormal, zero, negative
    real = [f / 2.0 ** lv for f in (315.5, 254.32, 458.654, 1234.5678, 80.0) for lv in range(5)]
    odd = [0.0, -0.0, 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308 / 4, -315.5, 1.0, 0.5, 3.0, np.pi]
    return np.concatenate([real, odd, rng.normal(size=2000) * 10.0 ** rng.uniform(-300, 300, size=2000)])


def test_the_reduction_factor_selected_by_words_is_the_conditional_chain():
    js = _jscales()
    assert len(js) > 2000 and (js == 0).any() and (np.abs(js) < 1e-300).any() and (np.abs(js) > 1e300).any()
    with np.errstate(over="ignore"):
        pos2 = 2.0 * js
        neg2 = -2.0 * js
    hi = (_bits(pos2) >> np.uint64(32)).astype(np.uint32)
    lo = (_bits(pos2) & np.uint64(0xffffffff)).astype(np.uint32)
    # -(2 jscale): the sign bit flipped, the low word equal (infinities included)
    assert np.array_equal(_bits(neg2), _bits(pos2) ^ np.uint64(1 << 63))
    for j in range(8):
        want = pos2 if j in (0, 1, 4) else neg2 if j < 6 else np.full_like(js, 4.0 if j == 6 else 1.0)
        flip = np.uint32(((0x2c >> j) & 1) << 31)
        if j < 6:
            got_hi, got_lo = hi ^ flip, lo
        else:
            got_hi = np.full(len(js), 0x40100000 if j == 6 else 0x3ff00000, dtype=np.uint32)
            got_lo = np.zeros(len(js), dtype=np.uint32)
        got = (got_hi.astype(np.uint64) << np.uint64(32)) | got_lo.astype(np.uint64)
        assert np.array_equal(got, _bits(want)), j
    assert [(0x2c >> j) & 1 for j in range(8)] == [0, 0, 1, 1, 0, 1, 0, 0]


def test_the_clamped_row_read_gives_lanes_0_to_20_the_same_sums():
    rng = np.random.default_rng(5)
    lanes = np.arange(64)
    for tpw, roww in ((1, 21), (2, 21), (3, 21), (4, 21), (4, 29)):
        nw = 8
        s_th = rng.normal(size=nw * tpw * roww) * 10.0 ** rng.uniform(-8, 8, size=nw * tpw * roww)
        s_th[rng.integers(0, len(s_th), 40)] = 0.0
        s_th[rng.integers(0, len(s_th), 40)] = -0.0               # a row that is -0.0: 0.0 + -0.0 = +0.0 on both paths
        s_th[rng.integers(0, len(s_th), 10)] = np.inf
        for wave in range(nw):
            acc_masked = np.zeros(64)
            acc_all = np.zeros(64)
            for k in range(tpw):
                base = (wave * tpw + k) * roww
                idx = base + np.where(lanes < 21, lanes, 0)
                assert idx.min() >= base and idx.max() < base + 21 and idx.max() < len(s_th)   # inside this tile's H row
                acc_masked = np.where(lanes < 21, acc_masked + np.where(lanes < 21, s_th[base + np.minimum(lanes, 20)], 0.0), acc_masked)
                acc_all = acc_all + s_th[idx]
            assert np.array_equal(_bits(acc_masked[:21]), _bits(acc_all[:21]))


def _old_plan(tpw, my_tiles, young):
    fav, half = (5 * my_tiles) // 8, ((5 * my_tiles) // 8 if (5 * my_tiles) % 8 >= 4 else -1)
    plan = 0
    if young:
        for k in range(tpw):
            plan |= ((1 if (k < fav or k == half) else 0x100) << k) | ((0x10000 << k) if k == half else 0)
    return plan


def _new_plan(tpw, my_tiles, young):
    fav, half = (5 * my_tiles) // 8, ((5 * my_tiles) // 8 if (5 * my_tiles) % 8 >= 4 else -1)
    plan = 0
    if young and (fav > 0 or half == 0):
        plan = 1
        for k in range(tpw):
            plan |= ((0x100 << k) if (k > 0 and half < 0 and k == fav) else 0) | ((0x10000 << k) if k == half else 0)
    return plan


def _run_old(plan, tpw, n_have, heads=None):
    """priority in the two halves of every computed tile; the head of a tile runs whether the tile exists or not (heads: the
    priority behind every tile's head is appended)"""
    prio, out = 0, []
    for k in range(tpw):
        if plan & (1 << k):
            prio = 1
        elif plan & (0x100 << k):
            prio = 0
        if heads is not None:
            heads.append(prio)
        if k >= n_have:
            continue
        first = prio
        if plan & (0x10000 << k):
            prio = 0
        out.append((first, prio))
    return out


def _run_new(plan, tpw, n_have, heads=None):
    prio, out = 0, []
    for k in range(tpw):
        if k == 0 and plan & 1:
            prio = 1
        if k > 0 and plan & (0x100 << k):
            prio = 0
        if heads is not None:
            heads.append(prio)
        if k >= n_have:
            continue
        first = prio
        if plan & (0x10000 << k):
            prio = 0
        out.append((first, prio))
    return out


def test_the_three_event_priority_schedule_runs_every_half_tile_at_the_same_priority():
    n = 0
    for tpw in range(1, 7):
        for my_tiles in range(0, tpw + 1):
            for young in (False, True):
                old, new = _old_plan(tpw, my_tiles, young), _new_plan(tpw, my_tiles, young)
                if not young:
                    assert old == 0 and new == 0
                for n_have in range(0, tpw + 1):
                    assert _run_old(old, tpw, n_have) == _run_new(new, tpw, n_have), (tpw, my_tiles, n_have)
                    n += 1
                # the raised tiles are the first ones and there is at most one drop: what the three events assume
                halves = [p for pair in _run_old(old, tpw, tpw) for p in pair]
                assert halves == sorted(halves, reverse=True)
    assert n == 2 * sum((t + 1) ** 2 for t in range(1, 7))
    # the default shape: 4 tiles on the younger wave, 2.5 of them favoured
    assert _run_new(_new_plan(4, 4, True), 4, 4) == [(1, 1), (1, 1), (1, 0), (0, 0)]
    assert _run_new(_new_plan(4, 3, True), 4, 3) == [(1, 1), (1, 0), (0, 0)]


def test_heads_of_missing_tiles_differ_only_behind_a_missing_half_way_drop():
    """the heads of tiles that do not exist still run (projection, row loads).  Their priority is the per-tile schedule's
    except behind a half-way drop whose tile does not exist: the three-event schedule stays raised there until the loop ends"""
    differing = 0
    for tpw in range(1, 7):
        for my_tiles in range(0, tpw + 1):
            half = (5 * my_tiles) // 8 if (5 * my_tiles) % 8 >= 4 else -1
            for n_have in range(0, tpw + 1):
                ho, hn = [], []
                _run_old(_old_plan(tpw, my_tiles, True), tpw, n_have, ho)
                _run_new(_new_plan(tpw, my_tiles, True), tpw, n_have, hn)
                for k in range(tpw):
                    if half >= 0 and half >= n_have and k > half:
                        assert (ho[k], hn[k]) == (0, 1), (tpw, my_tiles, n_have, k)
                        differing += 1
                    else:
                        assert ho[k] == hn[k], (tpw, my_tiles, n_have, k)
    assert differing > 0
