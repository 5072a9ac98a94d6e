"""Inputs for SparseImgAlign on pyramids whose levels have odd row strides, odd-aligned row starts and rounded level offsets
(tests/test_gpu_sia_odd_sizes.py; tests/test_sia_odd_inputs_cpu.py proves on the CPU that they reach what they claim).

Which bytes the kernels read (csrc/svo_sia.hip), in a pyramid batch laid out by svo_hip_pyramid_create: slot s at
s * pyr_bytes, level l at level_offset[l] inside it, every level start rounded up to 16 bytes, pyr_bytes = the rounded
end of the last level, allocation = pyr_bytes * batch + tail_slack (at least 64 bytes).

  * Reference patch, accepted when 3 <= u <= cols-4 and 3 <= v <= rows-4 (u, v the integer parts of the feature's position on
    the level): 7 rows of 8 bytes (load_row8) from (v-3) * cols + (u-3).  The last byte lies at (v+3) * cols + (u+4) from the
    level's start, i.e. at most (rows-1) * cols + cols = rows * cols for the patch in the bottom-right corner: ONE byte past
    the level.  (The arithmetic uses columns u-3 .. u+3 only; byte 7 of a row segment is loaded and never used.)  That byte
    is the first byte of the rounding gap or, when rows * cols is a multiple of 16, of the next level; behind the last level
    of a slot it is the first byte of the next slot, and in the last slot of the batch
        (batch-1) * pyr_bytes + level_offset[last] + rows * cols <= batch * pyr_bytes < batch * pyr_bytes + 64:
    inside the allocation, in its tail slack at the latest.
  * Current patch, accepted under the same rule: 5 rows of 8 bytes from (v-2) * cols + (u-2), last byte at
    (v+2) * cols + (u+5) <= (rows-2) * cols + cols + 1: inside the level.
  * A patch that is NOT accepted still has its loads issued, from offset 0 of the level: 7 rows of 8 bytes, last byte at
    6 * cols + 7.  On a level with fewer than 7 rows that is past the level; what matters is the last level of the last slot,
    where it must stay inside the tail slack: 100x68 level 4 is 6x4 = 24 bytes in a 32-byte block and the read ends at byte
    43, twelve bytes into the slack.  On a wide and short last level 64 bytes of slack are not enough -- 752x64: level 4 is
    47x4 = 188 bytes in a 192-byte block, the read ends at byte 289 --, which is why svo_hip_pyramid_create sizes the slack as
    max(64, 6 * cols_last + 8 - block_last) (tail_slack() below mirrors it; WIDE_SHORT is the case that needs it).

furthest_read() evaluates exactly this, and the CPU test asserts it for every planted and every random feature of every case
in the last slot of a batch of BATCH, so the GPU tests never rely on an out-of-range read being harmless."""
import functools

import numpy as np

import seed_reference as sr
from android_svo_amd import synth

SIZES = tuple(sr.ODD_SIZES) + ((346, 261),)
N_LEVELS = 5
BATCH = 3                      # the single evaluations run in slot 0 and in slot BATCH-1
N_RANDOM = 200
FRACS = (0.0, 0.5, 0.9375)     # sub-pixel parts of the planted positions (exact in binary: px * 2^-level is exact)
WIDE_SHORT = (752, 64)         # its level 4 is 47x4: the loads of rejected patches end 98 bytes past the pyramid


def size_id(s):
    return "%dx%d" % tuple(s[:2])


def level_dims(w, h, level):
    return w >> level, h >> level


def patch_levels(w, h):
    """the levels that have room for a reference patch (7 x 7 pixels)"""
    return [l for l in range(N_LEVELS) if (w >> l) >= 7 and (h >> l) >= 7]


def level_offsets(w, h, n_levels=N_LEVELS):
    """svo_hip_pyramid_create: (level_offset[0 .. n_levels-1], pyr_bytes)"""
    off, offs = 0, []
    for l in range(n_levels):
        offs.append(off)
        off = (off + (w >> l) * (h >> l) + 15) & ~15
    return offs, off


def tail_slack(w, h, n_levels=N_LEVELS):
    """svo_hip_pyramid_create: the bytes allocated behind the last slot"""
    cols = w >> (n_levels - 1)
    block = (cols * (h >> (n_levels - 1)) + 15) & ~15
    return max(64, 6 * cols + 8 - block)


def accepted(w, h, level, u_i, v_i):
    cols, rows = level_dims(w, h, level)
    return 3 <= u_i <= cols - 4 and 3 <= v_i <= rows - 4


def furthest_read(w, h, level, u_i, v_i, slot, batch=BATCH):
    """(offset of the last byte the kernels read for a feature at integer position (u_i, v_i) of `level` in `slot`, counted
    from the start of the allocation; size of the allocation)"""
    offs, pyr_bytes = level_offsets(w, h)
    cols, _ = level_dims(w, h, level)
    base = slot * pyr_bytes + offs[level]
    if accepted(w, h, level, u_i, v_i):
        last = (v_i + 3) * cols + (u_i - 3) + 7          # the reference footprint; the current one ends before it
    else:
        last = 6 * cols + 7                              # loads from offset 0, result unused
    return base + last, pyr_bytes * batch + tail_slack(w, h)


def planted(w, h, level):
    """[(u_i, v_i, accepted)]: the last accepted and the first rejected integer position at every side and corner of the level"""
    cols, rows = level_dims(w, h, level)
    um, vm = (cols - 1) // 2, (rows - 1) // 2
    return [(cols - 4, vm, 1), (cols - 3, vm, 0), (3, vm, 1), (2, vm, 0),
            (um, rows - 4, 1), (um, rows - 3, 0), (um, 3, 1), (um, 2, 0),
            (cols - 4, rows - 4, 1), (cols - 3, rows - 3, 0), (cols - 4, rows - 3, 0), (cols - 3, rows - 4, 0),
            (3, 3, 1), (2, 2, 0), (3, rows - 4, 1), (cols - 4, 3, 1)]


@functools.lru_cache(maxsize=None)
def noise_case(w, h, level, seed=0):
    """A frame pair of random-noise images with N_RANDOM random features (every eleventh without a point) followed by the
    planted ones of `level` at every sub-pixel part of FRACS, T_cur_w_init == T_ref_w: the current-image positions are the
    reference positions and meet the same limits.  Returns (FramePair, n_random, expected acceptance of the planted ones)."""
    rng = np.random.default_rng(7000 + 10 * w + level + 100003 * seed)
    cam = synth.Camera.default(w, h)
    ref = synth.build_pyramid(rng.integers(0, 256, (h, w)).astype(np.uint8))
    cur = synth.build_pyramid(rng.integers(0, 256, (h, w)).astype(np.uint8))
    px = np.stack([rng.uniform(0, w, N_RANDOM), rng.uniform(0, h, N_RANDOM)], axis=1)
    spec = planted(w, h, level)
    plant = np.array([[(u + fr) * (1 << level), (v + fr) * (1 << level)] for (u, v, _) in spec for fr in FRACS])
    want = np.array([a for (_, _, a) in spec for _ in FRACS], dtype=np.uint8)
    px = np.ascontiguousarray(np.concatenate([px, plant]))
    n = len(px)
    has_point = np.ones(n, dtype=np.uint8)
    has_point[:N_RANDOM:11] = 0
    f = np.ascontiguousarray(synth.cam2world(cam, px))
    T_ref_w = synth.se3_from_twist(rng.uniform(-0.05, 0.05, 3), rng.uniform(-0.02, 0.02, 3))
    T_w_ref = synth.se3_inv(T_ref_w)
    depth = rng.uniform(1.0, 3.0, n)
    pos = np.ascontiguousarray(np.stack([synth.se3_act(T_w_ref, f[i] * depth[i]) for i in range(n)]))
    fp = synth.FramePair(cam, ref, cur, px, f, pos, has_point, T_ref_w, T_ref_w.copy(), T_ref_w.copy())
    return fp, N_RANDOM, want


def integer_positions(fp, level):
    s = np.float32(1.0 / (1 << level))
    u = np.floor((fp.px[:, 0] * s).astype(np.float32)).astype(np.int64)
    v = np.floor((fp.px[:, 1] * s).astype(np.float32)).astype(np.int64)
    return u, v


# ---- full runs on rendered scenes ---------------------------------------------------------------------------------------
SCENE_SEED, SCENE_FEATURES = 5, 200
# (width, height, max_level, min_level): the oracle alone is well posed (tests/test_sia_odd_inputs_cpu.py) -> poses compared
POSE_CASES = ((346, 260, 4, 0), (346, 260, 4, 2), (346, 261, 4, 0), (202, 134, 3, 0))
# started on a level of 12x8 / 6x4 pixels: the solve degenerates, only the integer work is compared
DEGENERATE_CASES = ((100, 68, 4, 0), (202, 134, 4, 0))
WIDE_SHORT_CASE = WIDE_SHORT + (4, 0)      # level 4 has no room for a patch at all: every load goes to offset 0
RAGGED_SIZE, RAGGED_FEATURES = (346, 260), (200, 17, 0)


def run_id(c):
    return "%dx%d_L%d-L%d" % tuple(c)


@functools.lru_cache(maxsize=None)
def scene(w, h, n_features=SCENE_FEATURES, seed=SCENE_SEED):
    if n_features == 0:
        fp = scene(w, h)
        return synth.FramePair(fp.cam, fp.ref_pyr, fp.cur_pyr, np.zeros((0, 2)), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0, dtype=np.uint8),
                               fp.T_ref_w, fp.T_cur_w_true, fp.T_cur_w_init)
    return synth.make_frame_pair(seed=seed, width=w, height=h, n_features=n_features, border=4)


@functools.lru_cache(maxsize=None)
def oracle_run(w, h, max_level, min_level, n_features=SCENE_FEATURES):
    """orc.sparse_img_align of scene(): computed once, shared by the tests of every mode, never modified"""
    from oracle import orc
    return orc.sparse_img_align(scene(w, h, n_features), max_level=max_level, min_level=min_level)


def well_posed(o, fp, min_level, n_iter=30):
    """the rule under which poses are compared: at least 150 of 200 tracked, no NaN, the finest level stops before its budget,
    less than 0.02 rad from the true pose"""
    T = np.array(o.T_cur_w)
    return bool(o.n_tracked >= 150 and not np.isnan(T).any() and o.iters[min_level] < n_iter and
                synth.pose_error(T, fp.T_cur_w_true)[0] < 0.02)
