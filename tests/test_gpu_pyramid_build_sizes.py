"""The device pyramid build (svo_pyramid_build_levels, csrc/svo_ctx.hip) at one image size per path of that function, byte for
byte against synth.build_pyramid (the oracle's vk::halfSample level by level: tests/test_pyramid_size_classes_cpu.py, which
also proves from the sizes that each case takes the path it is listed for).  The images are random bytes, so a byte read from
or written to the wrong place changes the result.

    346x260, 346x261   scalar tail of half_sample_kernel at every level; odd row strides; an odd height
    352x260            not tiled (the height): the 8-byte / 4-byte vector branch for 352 -> 176 -> 88 -> 44, scalar for 44 -> 22
    328x248 (4 levels) vector for 328 -> 164, scalar below
    24x17 (2 levels)   vector, an output row of 12 bytes = 3 quads
    2064x32            width above PYR_STRIP_MAX_W: the per-level kernels, vector for the first two levels
    16x16, 2048x16     pyramid_strip_kernel at its narrowest (level 4 is one pixel wide) and widest
    352x256 with 1, 2, 3 levels   nothing to build; the strip kernel's early returns"""
import numpy as np
import pytest

import pyramid_size_cases as ps
from android_svo_amd import hip, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


def _assert_slot(pyr, slot, want, what):
    for l in range(pyr.n_levels):
        got = pyr.download_level(slot, l)
        assert got.shape == want[l].shape
        np.testing.assert_array_equal(got, want[l], err_msg="%s: slot %d level %d" % (what, slot, l))


@pytest.mark.parametrize("case", ps.CASES, ids=ps.case_id)
def test_upload_level0_and_build(ctx, case):
    """svo_hip_pyramid_upload_level0_and_build into the middle slot of three: every level equal to the reference, the slots on
    either side (sentinel pyramids) untouched."""
    w, h, nl, _ = case
    pyr = hip.Pyramid(ctx, w, h, nl, 3)
    sentinel = synth.build_pyramid(ps.image(w, h, 99), nl)
    for slot in (0, 2):
        pyr.upload(slot, sentinel)
    img = ps.image(w, h)
    pyr.upload_level0_and_build(1, img)
    _assert_slot(pyr, 1, synth.build_pyramid(img, nl), ps.case_id(case))
    for slot in (0, 2):
        _assert_slot(pyr, slot, sentinel, "sentinel")
    pyr.destroy()


@pytest.mark.parametrize("case", ps.CASES, ids=ps.case_id)
def test_upload_level0_batch_and_build(ctx, case):
    """svo_hip_pyramid_upload_level0_batch_and_build: 3 slots of a batch of 5 (blockIdx.z and the slot stride of every kernel),
    sentinel pyramids in the slots on either side, which must stay byte-equal."""
    w, h, nl, _ = case
    pyr = hip.Pyramid(ctx, w, h, nl, 5)
    sentinel = synth.build_pyramid(ps.image(w, h, 99), nl)
    for slot in (0, 4):
        pyr.upload(slot, sentinel)
    imgs = [ps.image(w, h, k) for k in range(3)]
    pyr.upload_level0_batch_and_build(1, imgs)
    for k in range(3):
        _assert_slot(pyr, 1 + k, synth.build_pyramid(imgs[k], nl), ps.case_id(case))
    for slot in (0, 4):
        _assert_slot(pyr, slot, sentinel, "sentinel")
    pyr.destroy()
