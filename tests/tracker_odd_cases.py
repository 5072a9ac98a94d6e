"""Inputs for the tracker on images the one-launch pyramid kernel does not take (tests/test_gpu_tracker_odd_sizes.py;
tests/test_tracker_odd_inputs_cpu.py holds the CPU side): the sequence of tracking_chain.make_sequence at 346x260 (the
per-level build runs its scalar branch) and 352x260 (its vector branch), with the map spread up to 9 px from the image border
so that matches fall into the cut last column and row of the 12 x 9 reprojection grid (30 px cells)."""
import functools

import numpy as np

import tracking_chain as tc

SIZES = ((346, 260), (352, 260))          # scalar build / vector build (tests/pyramid_size_cases.py)
CPU_SIZES = SIZES + ((344, 260), (346, 261))
N_FRAMES, N_MAP, BORDER, MIN_LEVEL = 8, 600, 9, 2
N_CAMS = 3
GROUP_STEPS = (1, 2, 3)


def size_id(s):
    return "%dx%d" % tuple(s)


def group_frames(k):
    """the frames the cameras of the group see at step k: every camera two frames ahead of the one before"""
    return [k + 2 * c for c in range(N_CAMS)]


@functools.lru_cache(maxsize=None)
def sequence(w, h):
    return tc.make_sequence(n_frames=N_FRAMES, n_map=N_MAP, width=w, height=h, border=BORDER)


def oracle_chain(seq, frames, min_level=MIN_LEVEL):
    """the oracle's frame function (tc.oracle_track_frame) over seq's frames `frames`, starting from keyframe 0 as last frame;
    returns the per-frame result dicts"""
    from oracle import orc
    mp = tc.sequence_map(seq)
    n = len(seq["px0"])
    state = {"pt_type": mp["pt_type"].copy(), "pt_n_failed": mp["pt_n_failed"].copy(), "pt_n_succeeded": mp["pt_n_succeeded"].copy(),
             "unlinked": np.zeros(n, np.uint8)}
    last = dict(T=seq["T0"].copy(), px=seq["px0"].copy(), f=seq["f0"].copy(), point=np.arange(n, dtype=np.int32))
    prev, out = 0, []
    for k in frames:
        r = tc.oracle_track_frame(orc, mp, state, last, seq["pyrs"][prev], seq["pyrs"][k], min_level)
        last = dict(T=r["T_f_w"].copy(), px=r["feat_px"], f=r["feat_f"], point=r["feat_point"])
        prev = k
        out.append(r)
    return out


@functools.lru_cache(maxsize=None)
def oracle_sequence(w, h):
    """the whole sequence, frame after frame: computed once and shared, never modified"""
    return oracle_chain(sequence(w, h), list(range(1, N_FRAMES)))


def grid_dims(w, h):
    return -(-w // tc.CELL), -(-h // tc.CELL)


def edge_matches(w, h, feat_px):
    """how many of a frame's features lie in the last (cut) column, and in the last row, of the reprojection grid"""
    gc, gr = grid_dims(w, h)
    return int(((feat_px[:, 0] / tc.CELL).astype(np.int64) == gc - 1).sum()), int(((feat_px[:, 1] / tc.CELL).astype(np.int64) == gr - 1).sum())
