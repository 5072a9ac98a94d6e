"""align2d_quad / align1d_quad (csrc/svo_align_device.h), the affine-warp stage at the head of df_search_block
(csrc/svo_depth_search.h) and md_geometry_item (csrc/svo_match_device.h) through their three entry points -- svo_hip_align2d_batch,
svo_hip_align1d_batch_dev, svo_hip_match_direct_batch_dev -- on the constructed families of tests/align_families.py: borders at entry
on both sides of every comparison and after the first iterations through every side, every exit class under budgets 0, 1, 2 and 10,
align1D's rollback, degenerate and full-contrast Hessians, the last legal pixel of every level in the last slot of a pyramid batch, a
separate ref_patch; the reference frame test on both sides of its four comparisons, det(A) just under and just over 3, 12 and 48 under
n_pyr_levels 1, 3 and 5, warps whose footprint fits the 32x32 LDS window and warps that fall back to direct loads, windows clipped at
every border, NaN and infinite inverse warps, edgelets.

Everything is compared with the oracle, which tests/test_align_families_cpu.py pins to the reference's compiled code and to a NumPy
model on these very cases: `converged` / `ok`, the iteration counts and the search levels equal, pixels and h_inv equal BY BITS, a
rejected findMatchDirect item's px_cur untouched.  Nothing is measured: there is no tolerance.  Then composition: every case as a batch
of one, all together, permuted, prefixes on both sides of the 4-per-wave, 16-per-workgroup and 256-thread edges, and one probe patch at
each of the 16 positions of a workgroup among neighbours that stop at iteration 0, go NaN or run the whole budget (the loops are left on
a wave-wide ballot) -- bit-equal per item in every one.

NaN outputs are compared by bits first; where the CPU's and the GPU's NaN differ in sign or payload, "is NaN" is compared for those
elements only and the case is recorded (test_nan_bit_patterns_are_reported prints the list).  Recorded on an MI355X against the x86-64
oracle: none -- every NaN the device wrote had the bits of the oracle's."""
import ctypes as C

import numpy as np
import pytest

import align_families as af
from android_svo_amd import hip

pytestmark = pytest.mark.gpu

SLOT = 1                      # the cases run on the LAST slot of a batch of 2 (slot 0 holds another image)
PREFIXES = (1, 3, 4, 5, 15, 16, 17, 255, 256, 257)
NAN_BITS_DIFFER = set()


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pyrs(ctx):
    out = {}
    for which in ("main", "odd"):
        cur = af.images(which)[3]
        h, w = cur[0].shape
        p = hip.Pyramid(ctx, w, h, af.N_LEVELS, 2)
        p.upload(0, af.other_image(which))
        p.upload(SLOT, cur)
        out[which] = p
    yield out
    for p in out.values():
        p.destroy()


@pytest.fixture(scope="module")
def md(ctx):
    """the keyframe pyramids (three slots) and one slot per distinct current image of the match groups"""
    cam, _, kf_poses, kf_pyr = af.md_scene()
    ref = hip.Pyramid(ctx, af.W, af.H, af.N_LEVELS, af.N_KF)
    for k in range(af.N_KF):
        ref.upload(k, kf_pyr[k])
    images, slot_of = [], {}
    for g in af.md_groups():
        for j, im in enumerate(images):
            if im is g.cur_pyr:
                slot_of[g.name] = j
                break
        else:
            slot_of[g.name] = len(images)
            images.append(g.cur_pyr)
    cur = hip.Pyramid(ctx, af.W, af.H, af.N_LEVELS, len(images))
    for j, im in enumerate(images):
        cur.upload(j, im)
    yield dict(cam=cam, ref=ref, cur=cur, slot_of=slot_of, T_ref_w=np.stack(kf_poses))
    ref.destroy()
    cur.destroy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_bits(name, got, want):
    """bitwise equality of float64 values (test_gpu_parity._assert_px_bits_equal); elements that are NaN on both sides may differ in
    sign or payload, and the case is recorded"""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    differ = _bits(got) != _bits(want)
    if differ.any():
        assert np.isnan(got[differ]).all() and np.isnan(want[differ]).all(), (name, got, want)
        NAN_BITS_DIFFER.add(name)


# ---- the entry points over a list of cases ----------------------------------------------------------------------------------------------
_expected = {}


def expected(c):
    if c.name not in _expected:
        _expected[c.name] = af.oracle_align(c)
    return _expected[c.name]


def run_align(ctx, pyrs, cases, null_patch=False):
    """cases of one (kind, image, level, n_iter) through one call -> [(ok, px, iters[, h_inv])]"""
    c0 = cases[0]
    assert all((c.kind, c.image, c.level, c.n_iter) == (c0.kind, c0.image, c0.level, c0.n_iter) for c in cases)
    n = len(cases)
    pwb = np.stack([c.pwb for c in cases]).astype(np.uint8)
    px = np.stack([c.px for c in cases]).astype(np.float64)
    pyr = pyrs[c0.image]
    if c0.kind == "1d":
        ok, p, h, it = hip.align1d_batch(ctx, pyr, SLOT, c0.level, pwb, np.stack([c.dir for c in cases]), c0.n_iter, px)
        return [(bool(ok[i]), p[i], int(it[i]), h[i]) for i in range(n)]
    if not null_patch:
        ok, p, it = hip.align2d_batch(ctx, pyr, SLOT, c0.level, pwb, np.stack([c.ref_patch for c in cases]), c0.n_iter, px)
    else:                       # ref_patch == NULL: the kernel takes the interior of the bordered patch
        pwb, p = np.ascontiguousarray(pwb.reshape(n, 100)), np.ascontiguousarray(px).copy()
        ok, it = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.int32)
        ctx.check(ctx.lib.svo_hip_align2d_batch(ctx.h, pyr.h, SLOT, c0.level, n, pwb.ctypes.data_as(C.POINTER(C.c_uint8)), None, c0.n_iter,
                                                p.ctypes.data_as(C.POINTER(C.c_double)), ok.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                it.ctypes.data_as(C.POINTER(C.c_int32))), "align2d_batch")
    return [(bool(ok[i]), p[i], int(it[i])) for i in range(n)]


def check_align(cases, got, what):
    for c, g in zip(cases, got):
        w = expected(c)
        assert g[0] == bool(w[0]) and g[2] == int(w[2]), (what, c.name, g, w)
        _assert_bits(c.name, g[1], w[1])
        if c.kind == "1d":
            _assert_bits(c.name, [g[3]], [w[3]])


def run_md(ctx, md, g, idx=None, edgelet="array"):
    a = g.arrays(idx)
    e = a["edgelet"] if edgelet == "array" else None if edgelet is None else np.zeros_like(a["edgelet"])
    ok, px, sl = hip.match_direct_batch(ctx, md["ref"], md["cur"], md["slot_of"][g.name], md["cam"], md["T_ref_w"], g.T_cur_w, a["slot"], a["px_ref"],
                                        a["f_ref"], a["level"], a["pt"], a["px_cur"], edgelet=e, grad=a["grad"] if e is not None else None,
                                        n_pyr_levels=g.n_pyr_levels, align_max_iter=10)
    return [(bool(ok[i]), px[i], int(sl[i])) for i in range(len(ok))]


_md_expected = {}


def md_expected(g, it):
    if it.name not in _md_expected:
        _md_expected[it.name] = af.md_oracle(g, it)
    return _md_expected[it.name]


def check_md(g, items, got, what):
    for it, r in zip(items, got):
        w = md_expected(g, it)
        assert r[0] == bool(w[0]) and r[2] == int(w[2]), (what, it.name, r, w)
        _assert_bits(it.name, r[1], w[1])
        if it.reach.get("framed") is False:                 # rejected: px_cur untouched, to the bit
            assert not r[0] and np.array_equal(_bits(r[1]), _bits(it.px_cur)), (what, it.name)


# ---- the families -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(af.align_families()))
def test_alignment_family(ctx, pyrs, family):
    cases = af.align_families()[family]
    for key, group in af.align_groups(cases).items():
        for kind in ("2d", "1d"):
            sub = [c for c in group if c.kind == kind]
            if not sub:
                continue
            check_align(sub, run_align(ctx, pyrs, sub), "family call")
            plain = [c for c in sub if c.patch is None]
            if kind == "2d" and plain:
                check_align(plain, run_align(ctx, pyrs, plain, null_patch=True), "ref_patch == NULL")
    if family == "a2d_refpatch":
        # the separate patch is what the residuals read: the same cases with the interior instead give another answer
        other = [af.dataclasses.replace(c, name=c.name + "+interior", patch=None) for c in cases]
        got, base = run_align(ctx, pyrs, other), run_align(ctx, pyrs, cases)
        check_align(other, got, "interior")
        assert all(not np.array_equal(_bits(a[1]), _bits(b[1])) for a, b in zip(got, base))


@pytest.mark.parametrize("name", [g.name for g in af.md_groups()])
def test_match_direct_group(ctx, md, name):
    g = af.md_group_named(name)
    got = run_md(ctx, md, g)
    check_md(g, g.items, got, "group call")
    levels = [r[2] for r in got]
    if name.startswith("md_zoom"):
        assert set(levels) == set(range(g.n_pyr_levels))                  # every level up to the cap n_pyr_levels - 1, none above
    corners = [i for i, it in enumerate(g.items) if not it.edgelet]
    if corners:
        # edgelet == NULL is an all-zero edgelet array: the corner items agree with the mixed call, and the two forms with each other
        null, zero = run_md(ctx, md, g, corners, edgelet=None), run_md(ctx, md, g, corners, edgelet="zeros")
        check_md(g, [g.items[i] for i in corners], null, "edgelet == NULL")
        for a, b in zip(null, zero):
            assert a[0] == b[0] and a[2] == b[2] and np.array_equal(_bits(a[1]), _bits(b[1]))


# ---- composition ------------------------------------------------------------------------------------------------------------------------
def _pool(kind):
    """the cases one call can take together: the main image, level 0, a budget of 10"""
    return [c for c in af.align_cases(kind) if (c.image, c.level, c.n_iter) == ("main", 0, 10)]


def _padded(pool, n):
    return [pool[i % len(pool)] for i in range(n)]


@pytest.mark.parametrize("kind", ["2d", "1d"])
def test_alignment_composition(ctx, pyrs, kind):
    pool = _pool(kind)
    assert len(pool) >= 30
    for c in pool:
        check_align([c], run_align(ctx, pyrs, [c]), "batch of one")
    check_align(pool, run_align(ctx, pyrs, pool), "all together")
    perm = [pool[i] for i in np.random.default_rng(3).permutation(len(pool))]
    check_align(perm, run_align(ctx, pyrs, perm), "permuted")
    for n in PREFIXES:
        batch = _padded(pool, n)
        check_align(batch, run_align(ctx, pyrs, batch), "prefix %d" % n)
    # every call of the other (image, level, budget) combinations once more as batches of one
    pooled = {c.name for c in pool}
    for c in af.align_cases(kind):
        if c.name not in pooled:
            check_align([c], run_align(ctx, pyrs, [c]), "batch of one")


@pytest.mark.parametrize("kind", ["2d", "1d"])
def test_alignment_probe_at_every_position_of_a_workgroup(ctx, pyrs, kind):
    """16 patches per workgroup (one wave, four lanes per patch); the iteration loop is left when no lane of the wave runs any more.  One
    probe -- it runs the whole budget and converges on its last iteration -- at each of the 16 positions, among neighbours that stop
    before the first iteration, go NaN after it, or run the whole budget without converging."""
    tag = "a2d" if kind == "2d" else "a1d"
    probe = af.align_case_named(tag + "_exit/b10_last")
    stop0 = af.align_case_named(tag + "_border/main_L0_u3")
    nan = af.align_case_named("a2d_hessian/flat" if kind == "2d" else "a1d_dir/zero")
    full = af.align_case_named(tag + "_exit/b10_spent")
    assert expected(probe)[2] == 10 and expected(stop0)[2] == 0 and np.isnan(expected(nan)[1]).all() and expected(full)[2] == 10
    for pos in range(16):
        for neighbours in ((stop0,), (nan,), (full,), (stop0, nan, full)):
            batch = [neighbours[i % len(neighbours)] for i in range(16)]
            batch[pos] = probe
            check_align(batch, run_align(ctx, pyrs, batch), "probe at %d" % pos)


def test_match_direct_composition(ctx, md):
    g = af.md_group_named("md_base")
    n_items = len(g.items)
    for i in range(n_items):
        check_md(g, [g.items[i]], run_md(ctx, md, g, [i]), "batch of one")
    perm = [int(i) for i in np.random.default_rng(4).permutation(n_items)]
    check_md(g, [g.items[i] for i in perm], run_md(ctx, md, g, perm), "permuted")
    for n in PREFIXES:
        idx = [i % n_items for i in range(n)]
        check_md(g, [g.items[i] for i in idx], run_md(ctx, md, g, idx), "prefix %d" % n)
    for grp in af.md_groups():                          # the other groups: every item alone
        if grp.name != "md_base":
            for i in range(len(grp.items)):
                check_md(grp, [grp.items[i]], run_md(ctx, md, grp, [i]), "batch of one")


def test_match_direct_probe_at_every_position_of_a_workgroup(ctx, md):
    """the warp stage takes 4 items per wave and 16 per workgroup, the alignment 16 per wave: a corner probe that runs several iterations
    at each of the 16 positions among rejected items, NaN warps, current pixels outside the frame and edgelets"""
    g = af.md_group_named("md_base")
    index = {it.name: i for i, it in enumerate(g.items)}
    probe = next(i for i, it in enumerate(g.items) if it.reach.get("interleaved") and not it.edgelet and md_expected(g, it)[0] and
                 af.md_trace(g, it)["align"]["iters"] >= 2)
    kinds = [index["md_base/frame_L0_left_out"], index["md_base/nan_point_at_ref_centre"], index["md_base/cur_px_outside_left"],
             index["md_base/edgelet_grad_x"], index["md_base/edgelet_zero_grad"]]
    for pos in range(16):
        for neighbours in ([kinds[0]], [kinds[1]], kinds):
            idx = [neighbours[i % len(neighbours)] for i in range(16)]
            idx[pos] = probe
            check_md(g, [g.items[i] for i in idx], run_md(ctx, md, g, idx), "probe at %d" % pos)


def test_nan_bit_patterns_are_reported():
    """runs last: the cases whose NaN outputs differed from the oracle's in sign or payload (see the module docstring)"""
    print("cases with NaN outputs of other bits than the oracle's:", sorted(NAN_BITS_DIFFER) or "none")
