"""The size list of tests/pyramid_size_cases.py reaches what it claims to reach, from the arithmetic of the sizes alone, and
the reference of tests/test_gpu_pyramid_build_sizes.py (synth.build_pyramid) is the oracle's vk::halfSample level by level."""
import ctypes as C

import numpy as np
import pytest

import pyramid_size_cases as ps
from android_svo_amd import synth
from oracle import orc


@pytest.mark.parametrize("case", ps.CASES, ids=ps.case_id)
def test_every_case_takes_the_path_it_is_listed_for(case):
    w, h, nl, want = case
    assert ps.level_paths(w, h, nl) == want
    assert (w >> (nl - 1)) > 0 and (h >> (nl - 1)) > 0               # svo_hip_pyramid_create accepts it
    if "strip" in want:
        assert w % 16 == 0 and h % 16 == 0 and w <= ps.PYR_STRIP_MAX_W and 2 <= nl <= 5
        assert 16 * w + 4 * w + w + w // 4 + 64 <= 64 * 1024         # the strip's LDS: within a workgroup's 64 KiB
    else:
        assert nl == 1 or w % 16 != 0 or h % 16 != 0 or w > ps.PYR_STRIP_MAX_W
    for l, path in enumerate(want, start=1):
        wi = w >> (l - 1)
        if path == "vector":
            assert wi % 8 == 0 and (wi // 2) % 4 == 0                # aligned 8-byte loads, whole 4-byte stores
        if path == "scalar":
            assert wi % 8 != 0


def test_the_list_holds_every_class():
    by = {c[:3]: c[3] for c in ps.CASES}
    assert len(by) == len(ps.CASES)
    # scalar at every level, odd stride, odd height
    for size in ((346, 260, 5), (346, 261, 5)):
        assert set(by[size]) == {"scalar"}
        assert [(size[0] >> l) % 2 for l in range(1, 5)] == [1, 0, 1, 1]          # 173, 86, 43, 21
    assert 261 % 2 == 1 and (261 >> 1) == (260 >> 1)
    # not tiled because of the height alone; vector then scalar in one build
    assert 352 % 16 == 0 and 260 % 16 != 0 and by[(352, 260, 5)] == ("vector", "vector", "vector", "scalar")
    assert by[(328, 248, 4)] == ("vector", "scalar", "scalar") and 328 % 16 != 0 and 248 % 16 != 0
    # one row of 3 quads, odd height
    assert by[(24, 17, 2)] == ("vector",) and (24 >> 1) == 12 and ((12 + 3) >> 2) == 3 and 17 % 2 == 1
    # too wide for the strip kernel although tiled otherwise
    assert 2064 % 16 == 0 and 32 % 16 == 0 and 2064 > ps.PYR_STRIP_MAX_W and by[(2064, 32, 5)][:2] == ("vector", "vector")
    # the strip kernel's extremes and early returns
    assert (16 >> 4) == 1 and by[(16, 16, 5)] == ("strip",) * 4
    assert 2048 == ps.PYR_STRIP_MAX_W and by[(2048, 16, 5)] == ("strip",) * 4 and 16 // 16 == 1   # one strip
    assert by[(352, 256, 1)] == () and by[(352, 256, 2)] == ("strip",) and by[(352, 256, 3)] == ("strip",) * 2
    # every path appears next to every other in at least one per-level build
    assert {p for c in ps.CASES for p in c[3]} == {"strip", "vector", "scalar"}


@pytest.mark.parametrize("case", ps.CASES, ids=ps.case_id)
def test_reference_pyramid_is_the_oracles_half_sample(case):
    w, h, nl, _ = case
    L = orc.lib()
    pyr = synth.build_pyramid(ps.image(w, h), nl)
    assert len(pyr) == nl
    for l in range(1, nl):
        wi, hi = w >> (l - 1), h >> (l - 1)
        assert pyr[l].shape == (hi >> 1, wi >> 1) == (h >> l, w >> l)
        out = np.zeros((hi >> 1, wi >> 1), dtype=np.uint8)
        L.svo_orc_half_sample(pyr[l - 1].ctypes.data_as(C.POINTER(C.c_uint8)), wi, hi, out.ctypes.data_as(C.POINTER(C.c_uint8)))
        np.testing.assert_array_equal(pyr[l], out)
