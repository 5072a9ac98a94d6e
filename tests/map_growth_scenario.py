"""The scenario the map-growth tests share (tests/test_map_growth_model.py on the CPU, tests/test_gpu_map_growth.py on the
device): tracking_chain's 9-frame sequence with the map points of the image's left third held back.  Tracking starts on the
map without them; after frame 2 they arrive as point candidates (seeds of keyframe 0 that converged); frame 5 becomes a
keyframe.  Their cells hold no competing regular point, so the reprojector matches some of them -- and, with maxFts = 120
ending the cell loop early, leaves others unmatched."""
import numpy as np

import tracking_chain as tc

N_FRAMES = 9
APPEND_AFTER = 2         # the candidates arrive after this frame
PROMOTE_AT = 5           # this frame becomes keyframe 1


def make():
    seq = tc.make_sequence(n_frames=N_FRAMES)
    held = seq["px0"][:, 0] < seq["cam"].width / 3.0
    base = dict(seq, px0=seq["px0"][~held].copy(), f0=seq["f0"][~held].copy(), pos=seq["pos"][~held].copy())
    cand = dict(pos=seq["pos"][held].copy(), kf_index=np.zeros(int(held.sum()), np.int32), px=seq["px0"][held].copy(), f=seq["f0"][held].copy(),
                level=np.zeros(int(held.sum()), np.int32))
    return dict(seq=seq, base=base, base_map=tc.sequence_map(base), cand=cand)


def first_last(seq):
    n = len(seq["px0"])
    return dict(T=seq["T0"].copy(), px=seq["px0"].copy(), f=seq["f0"].copy(), point=np.arange(n, dtype=np.int32))


def as_last(r):
    return dict(T=r["T_f_w"].copy(), px=r["feat_px"], f=r["feat_f"], point=r["feat_point"])


def snapshot(r):
    """a track result whose counter arrays no longer follow the chain's state"""
    return dict(r, type=r["type"].copy(), n_failed=r["n_failed"].copy(), n_succeeded=r["n_succeeded"].copy())
