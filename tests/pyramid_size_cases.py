"""Image sizes for the device pyramid build (svo_pyramid_build_levels, csrc/svo_ctx.hip), one per path of that function:

    strip     pyramid_strip_kernel, one launch: width % 16 == 0, width <= PYR_STRIP_MAX_W, height % 16 == 0, 2..5 levels
    vector    half_sample_kernel, 8-byte loads and a 4-byte store: a level whose input has w % 8 == 0
    scalar    half_sample_kernel, byte by byte: every other level
    nothing   n_levels == 1

tests/test_pyramid_size_classes_cpu.py asserts from the sizes alone that every case reaches the path it is listed for, so an
edit of this list cannot silently lose a class; tests/test_gpu_pyramid_build_sizes.py builds them on the device."""
import numpy as np

PYR_STRIP_MAX_W = 2048          # csrc/svo_ctx.hip

# (width, height, n_levels, the path of the build from level l-1 to level l, for l = 1 .. n_levels-1)
CASES = (
    (346, 260, 5, ("scalar", "scalar", "scalar", "scalar")),       # odd row stride from level 1 on
    (346, 261, 5, ("scalar", "scalar", "scalar", "scalar")),       # ... and an odd height: the last input row is dropped
    (352, 260, 5, ("vector", "vector", "vector", "scalar")),       # not tiled because of the height; 352 -> 176 -> 88 -> 44, then 44 -> 22
    (328, 248, 4, ("vector", "scalar", "scalar")),                 # 328 -> 164, then 164 % 8 == 4
    (24, 17, 2, ("vector",)),                                      # an output row of 12 bytes = 3 quads, odd height
    (2064, 32, 5, ("vector", "vector", "scalar", "scalar")),       # width % 16 == 0 but above PYR_STRIP_MAX_W: per level
    (16, 16, 5, ("strip",) * 4),                                   # the strip kernel's narrowest: level 4 is one pixel
    (2048, 16, 5, ("strip",) * 4),                                 # ... and widest
    (352, 256, 1, ()),                                             # nothing to build
    (352, 256, 2, ("strip",)),                                     # the strip kernel's early returns
    (352, 256, 3, ("strip",) * 2),
)


def case_id(case):
    return "%dx%d_L%d" % case[:3]


def tiled(width, height, n_levels):
    """the condition under which svo_pyramid_build_levels launches pyramid_strip_kernel (pyr_bytes % 16 == 0 always holds:
    level offsets are rounded up to 16)"""
    return width % 16 == 0 and width <= PYR_STRIP_MAX_W and height % 16 == 0 and 2 <= n_levels <= 5


def level_paths(width, height, n_levels):
    """the path svo_pyramid_build_levels takes for each level 1 .. n_levels-1, from the sizes alone"""
    if n_levels < 2:
        return ()
    if tiled(width, height, n_levels):
        return ("strip",) * (n_levels - 1)
    out = []
    for l in range(1, n_levels):
        w = width >> (l - 1)
        # half_sample_kernel's own test: (w & 7) == 0 && ((w >> 1) & 3) == 0 -- the second follows from the first
        out.append("vector" if w % 8 == 0 and (w >> 1) % 4 == 0 else "scalar")
    return tuple(out)


def image(width, height, k=0):
    """random bytes: any misplaced byte changes the result"""
    return np.random.default_rng(1000 * width + height + 7919 * k).integers(0, 256, (height, width)).astype(np.uint8)
