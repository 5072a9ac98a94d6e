"""Inputs of the many-camera depth-filter pass (svo_hip_seed_batch_update_cameras_async): per arrangement the cameras, each with
its own scene, current frame, pose and keyframes (seedsynth.make_multi_keyframe_case with the camera's own seed, 320x240, 5
levels), and per batch the oracle's first pass.  tests/test_df_cameras_inputs_cpu.py establishes that the cameras differ
enough for a wrong current slot to show; tests/test_gpu_seed_cameras.py runs the arrangements on the device."""
import dataclasses
import functools
from typing import Tuple

import numpy as np

from android_svo_amd import seedsynth

WIDTH, HEIGHT, LEVELS, BORDER = 320, 240, 5, 24
SIGMA2_SCALE = np.float32(0.02)            # as tests/test_gpu_seed_batch.py's grouped test: seeds converge within three frames


def _sizes_70():
    """70 batch sizes in 1..40, every camera of seven with ten of them"""
    rng = np.random.default_rng(70)
    s = rng.integers(4, 41, 70)
    s[3], s[25], s[41] = 1, 2, 40
    return tuple(tuple(int(v) for v in s[10 * c:10 * c + 10]) for c in range(7))


def _sizes_60():
    """60 batches of one 256-record block each (20..256 seeds), ten a camera: 15 360 records, the most jobs the two-launch form
    can be given (svo_hip_df_set_small_pass_limit takes at most 16 384 records)"""
    return tuple(tuple(20 + (37 * (10 * c + k)) % 237 for k in range(10)) for c in range(6))


@dataclasses.dataclass(frozen=True)
class Arrangement:
    name: str
    sizes: Tuple[Tuple[int, ...], ...]     # per camera the sizes of its batches (none: the camera sits the pass out)
    seeds: Tuple[int, ...]                 # per camera the seed of its scene
    reversed_slots: bool = False           # current slots and every camera's keyframe slots in reversed order
    erase_seventh: bool = False            # a seventh of every batch's seeds erased by hand before the first pass
    wholly_erased: Tuple[int, int] = None  # (camera, batch) erased as a whole


# The seeds are the ones tests/test_df_cameras_inputs_cpu.py accepts: with any other camera's current image and pose at least one
# seed in ten of every batch ends with another status.
ARRANGEMENTS = (
    Arrangement("one_camera_one_batch", ((300,),), (401,)),
    Arrangement("two_cameras_three_batches", ((120, 90, 64), (200, 31, 257)), (402, 403), erase_seventh=True),
    Arrangement("three_cameras_0_2_0", ((), (150, 100), ()), (404, 405, 406)),
    Arrangement("nine_cameras_two_batches", ((100, 60),) * 9, tuple(range(410, 419))),
    Arrangement("seventy_small_jobs", _sizes_70(), (420, 421, 422, 425, 426, 429, 432)),
    Arrangement("sixty_one_block_jobs", _sizes_60(), (450, 451, 452, 453, 454, 455)),
    Arrangement("sizes_around_a_block", ((1, 255, 256), (257, 700)), (430, 431), erase_seventh=True),
    Arrangement("one_batch_of_4097", ((4097,), (50,)), (432, 433)),
    Arrangement("reversed_slots", ((80, 40), (33, 90), (64, 17)), (434, 435, 436), reversed_slots=True),
    Arrangement("shared_keyframe_batch", ((70, 130), (90, 20)), (437, 438)),
    Arrangement("camera_with_a_wholly_erased_batch", ((100,), (40,), (80,)), (439, 440, 441), wholly_erased=(1, 0)),
)
BY_NAME = {a.name: a for a in ARRANGEMENTS}


@functools.lru_cache(maxsize=None)
def camera_case(seed: int, sizes: Tuple[int, ...]):
    """The camera's scene, current frame and keyframes.  A camera without batches still has a current frame (one keyframe is
    made for it and not used)."""
    mk = seedsynth.make_multi_keyframe_case(sizes if sizes else (1,), seed=seed, width=WIDTH, height=HEIGHT, border=BORDER)
    if not sizes:
        mk.keyframes.clear()
    return mk


def cameras(arr: Arrangement):
    return [camera_case(s, z) for s, z in zip(arr.seeds, arr.sizes)]


def sigma2_of(sc):
    return (sc.sigma2 * SIGMA2_SCALE).astype(np.float32)


def oracle_pass(cam, sc, cur_pyr, T_cur_w):
    """oracle/orc.py:update_seeds of one batch against a current frame; the batch's state is not changed.  Returns the outputs
    and the updated (mu, sigma2)."""
    from oracle import orc
    a, b, mu, s2 = sc.a.copy(), sc.b.copy(), sc.mu.copy(), sigma2_of(sc)
    o = orc.update_seeds(cam, sc.ref_pyr, cur_pyr, sc.T_ref_w, T_cur_w, sc.px, sc.f, sc.level, a, b, mu, sc.z_range, s2)
    o["mu"], o["sigma2"] = mu, s2
    return o


@functools.lru_cache(maxsize=None)
def oracle_first_pass(name: str):
    """per camera, per batch: the oracle's pass against the camera's own current frame (computed once, shared, left unchanged)"""
    arr = BY_NAME[name]
    return tuple(tuple(oracle_pass(mk.cam, sc, mk.cur_pyr, mk.T_cur_w) for sc in mk.keyframes) for mk in cameras(arr))
