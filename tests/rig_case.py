"""Inputs of the camera-rig tests: three cameras of ONE image size with clearly different models, every camera on a scene of its
own that it renders and observes with its own model.

    camera   fx   fy   cx            cy            distortion
    A        500  500  w/2 - 0.5     h/2 - 0.5     none
    B        430  445  w/2 - 14.75   h/2 + 12.25   none
    C        560  540  w/2 + 13.5    h/2 - 11      radtan, the coefficients of test_depth_filter_and_detector_with_a_distorted_camera

Seed passes (svo_hip_seed_batch_update_rig_async): per arrangement the cameras in the arrangement's order, each with its current
frame, pose and keyframes (seedsynth.make_multi_keyframe_case with the camera, 320x240, 5 levels; the bearings of a distorted
camera are the oracle's cam2world), and per batch the oracle's first pass with the camera's own model.
tests/test_rig_inputs_cpu.py establishes that a pass with another camera's model shows; tests/test_gpu_seed_rig.py runs the
arrangements on the device.

Tracked sequences (svo_hip_tracker_group_create_rig): `sequence(name)`, the sequence of tests/tracking_chain.py rendered and
observed by rig camera `name` over a scene of its own (640x480), for tests/test_gpu_tracker_rig.py and the C++ twins of
tests/test_gpu_rig_cpp.py."""
import dataclasses
import functools
from typing import Tuple

import numpy as np

from android_svo_amd import seedsynth, synth

DIST_C = (-0.12, 0.03, 2e-4, -1e-4, 0.0)
NAMES = ("A", "B", "C")


def camera(name: str, width: int, height: int) -> synth.Camera:
    w, h = float(width), float(height)
    if name == "A":
        return synth.Camera(width, height, 500.0, 500.0, w / 2 - 0.5, h / 2 - 0.5)
    if name == "B":
        return synth.Camera(width, height, 430.0, 445.0, w / 2 - 14.75, h / 2 + 12.25)
    assert name == "C"
    cam = synth.Camera(width, height, 560.0, 540.0, w / 2 + 13.5, h / 2 - 11.0)
    cam.dist = DIST_C                        # (hip.make_camera, orc.camera and synth.PlaneScene read the attribute)
    return cam


def bearings(cam, px):
    """Feature::f of the pixels: the oracle's cam2world where the model has distortion (synth.cam2world is the plain pinhole
    model, bit-equal to the oracle's for a camera without)"""
    if getattr(cam, "dist", None) is None:
        return synth.cam2world(cam, px)
    from oracle import orc
    return np.ascontiguousarray(orc.cam2world(cam, px))


# ---- seed passes ----------------------------------------------------------------------------------------------------------
WIDTH, HEIGHT, LEVELS, BORDER = 320, 240, 5, 24
SIGMA2_SCALE = np.float32(0.02)            # as tests/df_cameras_case.py: seeds converge within three frames


@dataclasses.dataclass(frozen=True)
class Arrangement:
    name: str
    order: Tuple[str, ...]                 # the cameras of the pass, in pass order
    sizes: Tuple[Tuple[int, ...], ...]     # per camera the sizes of its batches (none: the camera sits the pass out)
    seeds: Tuple[int, ...]                 # per camera the seed of its scene
    reversed_slots: bool = False           # current slots and every camera's keyframe slots in reversed order


# The scene seeds are ones tests/test_rig_inputs_cpu.py accepts: with either other camera's model at least three seeds of every
# batch end with another status or other bits of mu.
ARRANGEMENTS = (
    Arrangement("sizes_around_a_block", ("A", "B", "C"), ((255, 256, 257), (300,), (64, 31)), (501, 502, 503)),
    Arrangement("sizes_around_a_block_reversed_slots", ("A", "B", "C"), ((255, 256, 257), (300,), (64, 31)), (501, 502, 503), reversed_slots=True),
    Arrangement("two_cameras_sit_out", ("B", "C", "A"), ((), (150, 100), ()), (504, 505, 506)),
    Arrangement("one_camera", ("C",), ((300,),), (507,)),
)
BY_NAME = {a.name: a for a in ARRANGEMENTS}


@functools.lru_cache(maxsize=None)
def camera_case(cam_name: str, seed: int, sizes: Tuple[int, ...]):
    """The camera's scene, current frame and keyframes.  A camera without batches still has a current frame (one keyframe is
    made for it and not used)."""
    cam = camera(cam_name, WIDTH, HEIGHT)
    mk = seedsynth.make_multi_keyframe_case(sizes if sizes else (1,), seed=seed, width=WIDTH, height=HEIGHT, border=BORDER, cam=cam)
    for sc in mk.keyframes:
        sc.f = bearings(cam, sc.px)
    if not sizes:
        mk.keyframes.clear()
    return mk


def cameras(arr: Arrangement):
    return [camera_case(n, s, z) for n, s, z in zip(arr.order, arr.seeds, arr.sizes)]


def sigma2_of(sc):
    return (sc.sigma2 * SIGMA2_SCALE).astype(np.float32)


def oracle_pass(cam, sc, cur_pyr, T_cur_w):
    """oracle/orc.py:update_seeds of one batch with camera model `cam`; the batch's state is not changed.  Returns the outputs
    and the updated (mu, sigma2)."""
    from oracle import orc
    a, b, mu, s2 = sc.a.copy(), sc.b.copy(), sc.mu.copy(), sigma2_of(sc)
    o = orc.update_seeds(cam, sc.ref_pyr, cur_pyr, sc.T_ref_w, T_cur_w, sc.px, sc.f, sc.level, a, b, mu, sc.z_range, s2)
    o["mu"], o["sigma2"] = mu, s2
    return o


@functools.lru_cache(maxsize=None)
def oracle_first_pass(name: str):
    """per camera, per batch: the oracle's pass with the camera's own model (computed once, shared, left unchanged)"""
    return tuple(tuple(oracle_pass(mk.cam, sc, mk.cur_pyr, mk.T_cur_w) for sc in mk.keyframes) for mk in cameras(BY_NAME[name]))


# ---- tracked sequences ------------------------------------------------------------------------------------------------------
# Every rig camera on a rendered sequence of its own (640x480, the path of tests/tracking_chain.py: make_sequence with the
# camera's model and a scene of its own), keyframe 0's features as the map.
TRACK_WIDTH, TRACK_HEIGHT = 640, 480
TRACK_SCENES = {"A": 601, "B": 602, "C": 603}


@functools.lru_cache(maxsize=None)
def sequence(cam_name: str, n_frames: int = 9, n_map: int = 600):
    """the dict of tracking_chain.make_sequence for rig camera `cam_name`"""
    rng = np.random.default_rng(2024)
    cam = camera(cam_name, TRACK_WIDTH, TRACK_HEIGHT)
    scene = synth.PlaneScene(seed=TRACK_SCENES[cam_name], depth=2.2, tilt=(0.06, -0.04))
    T0 = synth.se3_from_twist([0.01, -0.02, 0.0], [0.004, -0.003, 0.002])
    step_t, step_r = np.array([0.012, 0.004, -0.003]), np.array([0.0015, -0.0025, 0.002])
    truth = [T0]
    for _ in range(1, n_frames):
        wob = rng.uniform(-0.002, 0.002, 3)
        truth.append(synth.se3_mul(synth.se3_from_twist(step_t + wob, step_r + 0.2 * wob), truth[-1]))
    pyrs = [synth.build_pyramid(scene.render(cam, T)) for T in truth]
    px0 = synth.grid_features(cam, n_map, rng)           # the map: points seen in keyframe 0
    f0 = bearings(cam, px0)
    pos = scene.intersect(cam, T0, px0[:, 0], px0[:, 1])
    return dict(cam=cam, truth=truth, pyrs=pyrs, px0=px0, f0=f0, pos=pos, T0=T0)
