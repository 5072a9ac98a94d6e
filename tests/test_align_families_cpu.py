"""The constructed families of tests/align_families.py for align2D, align1D and findMatchDirect, without a GPU:

  * reach -- every case reaches what it is named for, asserted from the trace of the NumPy model (tests/align_reference.py): the exit
    reason and iteration, the rollback iteration, the side an estimate leaves through, the window-or-direct choice of the warp stage, the
    clipped side and the zeroed samples, the search level and the side of its threshold;
  * the model (scalar f32 NumPy in the reference's order) and its findMatchDirect composition equal the oracle by bits on every case;
  * the oracle is pinned to the reference's own compiled align2D / align1D / findMatchDirect on every case but the ones listed by name
    in af.ORACLE_ONLY and af.DEVICE_CONTRACT (tests/golden/align_paths_ref.npz, made by oracle/gen_golden.py --align-paths-only: results
    only, the inputs are regenerated here and guarded by CRCs);
  * the comparison used on the GPU (flags, iteration counts and search levels equal, pixels and h_inv by bits) rejects nine wrong
    stand-ins, each on a named case.

NaN sample coordinates: an input of the public entry CAN give an infinite, not NaN, inverse warp -- an exactly singular A with four
non-zero entries (the current camera's centre in the plane of the reference patch, rolled: af._singular_groups finds two such poses).
The inverse is then (+-inf), the sample coordinates inf * 0 and inf - inf = NaN, which pass the reference's range test; the reference
interpolates there (a read outside its image).  The device zeroes such samples, and so does the oracle since this suite
(svo_orc_warp_affine, oracle/README.md); test_infinite_inverse_warp_zeroes_the_patch holds both to it.

tests/test_gpu_align_paths.py runs the same cases through the three device entry points."""
import os

import numpy as np
import pytest

import align_families as af
import align_reference as ar
from oracle import orc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "align_paths_ref.npz")
FAMILIES = list(af.align_families())
GROUPS = [g.name for g in af.md_groups()]
MUTATIONS = ("jres_tree", "min_update_le", "border_right_bottom", "rollback_no_restore", "rollback_at_0", "warp_clamp", "level_cap", "frame_px", "h_half")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_align(got, want):
    """the GPU comparison for one alignment: got / want = (ok, px, iters[, h_inv]); pixels and h_inv by bits"""
    return bool(got[0]) == bool(want[0]) and np.array_equal(bits(got[1]), bits(want[1])) and int(got[2]) == int(want[2]) and \
        (len(want) < 4 or np.array_equal(bits(got[3]), bits(want[3])))


def same_match(got, want):
    """the GPU comparison for one findMatchDirect item: (ok, px_cur, search_level)"""
    return bool(got[0]) == bool(want[0]) and np.array_equal(bits(got[1]), bits(want[1])) and int(got[2]) == int(want[2])


def model_tuple(c, mut=()):
    m = af.model_align(c, mut)
    return (m["ok"], m["px"], m["iters"]) + ((m["h_inv"],) if c.kind == "1d" else ())


def trace_tuple(g, it, mut=()):
    t = af.md_trace(g, it, mut)
    return t["ok"], t["px_cur"], t["search_level"]


# ---- the fixture --------------------------------------------------------------------------------------------------------------------
def test_only_the_named_cases_are_left_out_of_the_reference_comparison():
    g = np.load(GOLD)
    assert af.ORACLE_ONLY == ("md_base/nan_point_at_ref_centre", "md_base/nan_point_at_ref_centre_edgelet", "md_zoom_n3/nan_point_in_cur_plane",
                              "md_singular_0/inf_warp", "md_singular_0/inf_warp_edgelet", "md_singular_1/inf_warp", "md_singular_1/inf_warp_edgelet")
    assert af.DEVICE_CONTRACT == ("md_base/slot_minus_1", "md_base/slot_n_kf")
    for kind in ("2d", "1d"):
        assert list(g["align%s_names" % kind]) == [c.name for c in af.align_cases(kind)]               # no alignment case is left out
    everything = [it.name for grp in af.md_groups() for it in grp.items]
    recorded = [n for grp in af.md_groups() if grp.name + "_names" in g.files for n in g[grp.name + "_names"]]
    assert recorded == [n for n in everything if n not in af.ORACLE_ONLY + af.DEVICE_CONTRACT]
    assert set(af.ORACLE_ONLY + af.DEVICE_CONTRACT) <= set(everything)
    # what the left-out cases are: NaN or infinite inverse warps, and slots outside the range -- nothing else
    for grp in af.md_groups():
        for it in grp.items:
            if it.name in af.ORACLE_ONLY:
                assert it.reach.get("warp_nan") or it.reach.get("warp_inf"), it.name
            if it.name in af.DEVICE_CONTRACT:
                assert not 0 <= it.slot < af.N_KF, it.name
    assert os.path.getsize(GOLD) < 64 * 1024


@pytest.mark.parametrize("kind", ["2d", "1d"])
def test_oracle_alignment_against_reference_fixture(kind):
    g = np.load(GOLD)
    cases = af.align_cases(kind)
    assert af.align_input_crc(cases) == [int(v) for v in g["align%s_crc" % kind]], "the family code no longer reproduces the inputs the fixture was recorded on"
    for i, c in enumerate(cases):
        o = af.oracle_align(c)
        assert bool(o[0]) == bool(g["align%s_ok" % kind][i]), c.name
        assert np.array_equal(bits(o[1]), bits(g["align%s_px" % kind][i])), (c.name, o[1], g["align%s_px" % kind][i])
        if kind == "1d":
            assert np.array_equal(bits(o[3]), bits(g["align1d_hinv"][i])), (c.name, o[3], g["align1d_hinv"][i])


@pytest.mark.parametrize("name", [n for n in GROUPS if not n.startswith("md_singular")])
def test_oracle_match_direct_against_reference_fixture(name):
    g = np.load(GOLD)
    grp = af.md_group_named(name)
    assert af.md_input_crc(grp) == [int(v) for v in g[name + "_crc"]], "the family code no longer reproduces the inputs the fixture was recorded on"
    items = [it for it in grp.items if it.name not in af.ORACLE_ONLY + af.DEVICE_CONTRACT]
    assert [it.name for it in items] == list(g[name + "_names"])
    for i, it in enumerate(items):
        ok, px, sl = af.md_oracle(grp, it)
        assert ok == bool(g[name + "_ok"][i]), it.name
        assert np.array_equal(bits(px), bits(g[name + "_px"][i])), (it.name, px, g[name + "_px"][i])
        if g[name + "_sl"][i] >= 0:                       # (the harness leaves -1 where the frame test fails)
            assert sl == g[name + "_sl"][i], it.name
        else:
            assert not ok and np.array_equal(bits(px), bits(it.px_cur)), it.name


# ---- the model is the oracle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_model_equals_oracle_by_bits(family):
    for c in af.align_families()[family]:
        assert same_align(model_tuple(c), af.oracle_align(c)), c.name


@pytest.mark.parametrize("name", GROUPS)
def test_match_direct_composition_equals_oracle_by_bits(name):
    grp = af.md_group_named(name)
    for it in grp.items:
        if 0 <= it.slot < af.N_KF:
            assert same_match(trace_tuple(grp, it), af.md_oracle(grp, it)), it.name


def test_model_warp_equals_the_oracles_warp():
    """the f32 warp of the composition against svo_orc_warp_affine, patch by patch (the composition above could hide a patch difference
    behind an alignment that does not run)"""
    import ctypes as C
    cam, _, kf_poses, kf_pyr = af.md_scene()
    n = 0
    for grp in af.md_groups():
        for it in grp.items:
            t = af.md_trace(grp, it) if 0 <= it.slot < af.N_KF else {}
            if not t.get("framed"):
                continue
            A = ar.warp_matrix(cam, kf_poses[it.slot], grp.T_cur_w, it.px_ref, it.f_ref, it.level, it.pt)
            img = kf_pyr[it.slot][it.level]
            out = np.full(100, 7, dtype=np.uint8)
            a, p = orc.f64(A), orc.f64(it.px_ref)
            wrote = orc.lib().svo_orc_warp_affine(orc._p(a, C.c_double), orc._p(img, C.c_uint8), img.shape[1], img.shape[0], orc._p(p, C.c_double),
                                                  C.c_int(it.level), C.c_int(t["search_level"]), C.c_int(5), orc._p(out, C.c_uint8))
            assert bool(wrote) == (not t["warp_nan"]), it.name
            if wrote:
                np.testing.assert_array_equal(out, t["pwb"], it.name)
                n += 1
    assert n > 100


# ---- reach: alignment ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_alignment_cases_reach_what_they_are_named_for(family):
    for c in af.align_families()[family]:
        m, r = af.model_align(c), c.reach
        rows, cols = c.img.shape
        for key in ("exit", "exit_iter", "iters"):
            if key in r:
                assert m[key] == r[key], (c.name, key, m[key], r[key])
        if "entry" in r:                                   # both sides of one comparison of the border test, at entry
            u_r, v_r = int(np.floor(np.float32(c.px[0]))), int(np.floor(np.float32(c.px[1])))
            assert {"left": u_r in (3, 4), "top": v_r in (3, 4), "right": u_r in (cols - 5, cols - 4), "bottom": v_r in (rows - 5, rows - 4)}[r["entry"]]
            assert (ar.side_of(c.px, cols, rows) == "") == r["inside"] == (m["iters"] >= 1), c.name
            if not r["inside"]:
                assert ar.side_of(c.px, cols, rows) == r["entry"]
        if r.get("cast_decides"):                          # floor() of the double says the opposite of floor() of its f32 cast
            inside64 = 4 <= np.floor(c.px[0]) < cols - 4 and 4 <= np.floor(c.px[1]) < rows - 4
            assert inside64 != r["inside"] and (m["iters"] >= 1) == r["inside"], c.name
        if r.get("later"):
            assert m["exit_iter"] >= 2 and not m["ok"] and ar.side_of(m["px"], cols, rows) == r["side"], c.name
            assert all(ar.side_of(p, cols, rows) == "" for p in m["trace"][:-1])            # inside until then
            assert ar.side_of(m["trace"][-1], cols, rows) == r["side"]
        if r.get("exit") == "budget" and c.n_iter == 0:
            assert not m["ok"] and np.array_equal(m["px"], np.float32(c.px).astype(np.float64)) and not np.array_equal(m["px"], c.px), c.name
        if r.get("hessian") == "flat":
            assert not m["H"][[0, 1, 2, 4, 5]].any() and np.isnan(m["px"]).all()
        if r.get("hessian") == "x_only":
            H = m["H"].astype(np.float64).reshape(3, 3)
            assert H[0, 0] > 0 and H[0, 2] != 0 and not H[1].any() and np.isnan(m["px"]).all()
        if r.get("hessian") == "contrast":                 # the largest gradients there are, and the sums exact whatever the order
            dx, dy = ar._jacobians(c.pwb)
            assert np.abs(np.concatenate([dx, dy])).max() == 127.5 and m["iters"] >= 1
            for k, terms in ((0, dx * dx), (1, dx * dy), (2, dx), (4, dy * dy), (5, dy)):
                t64 = terms.astype(np.float64)
                assert float(m["H"][k]) == t64.sum() == float(np.float32(t64.reshape(4, 16).sum(axis=1).astype(np.float32).sum()))
        if r.get("last_pixel"):
            assert int(np.floor(c.px[0])) == cols - 5 and int(np.floor(c.px[1])) == rows - 5 and (m["iters"] >= 1) == r["inside"]
            assert np.array_equal(c.pwb, af.cut(c.img, cols - 5, rows - 5))
        if r.get("separate_patch"):
            assert not np.array_equal(c.patch, af.interior(c.pwb)) and m["iters"] >= 2
            assert not same_align(model_tuple(c), model_tuple(af.dataclasses.replace(c, patch=None))), c.name
        if r.get("chi2_0_large"):
            assert m["chi2"][0] > 64 * 20.0 ** 2 and len(m["chi2"]) >= 3                    # rms residual over 20 grey levels, and the run goes on
        if r.get("exit") == "rollback":
            k = r["exit_iter"]
            assert k >= 1 and m["chi2"][k] > m["chi2"][k - 1] and all(m["chi2"][j] <= m["chi2"][j - 1] for j in range(1, k))
            u, v = m["trace"][k]                            # the estimate entering the iteration that rolls back, minus the step = the one before
            assert not m["ok"] and not np.array_equal(m["px"], np.array([u, v], dtype=np.float64))
        if r.get("h_inv_inf"):
            assert m["H00"] == 0 and np.isinf(m["h_inv"]) and np.isnan(m["px"]).all()
        if r.get("h_inv_contrast"):                        # H(0,0) is NOT exact here: summed in another order it differs
            serial = _h00(c, tree=False)
            assert serial == m["H00"] and np.isfinite(m["h_inv"])
    if family == "a1d_hinv":
        inexact = [c.name for c in af.align_families()[family] if _h00(c, tree=True) != af.model_align(c)["H00"]]
        assert len(inexact) >= 2, inexact                  # the order matters on these templates: a tree sum gives another H(0,0)


def _h00(c, tree):
    """H(0,0) of align1D for the case's template and direction: the serial f32 sum, or the same terms as a 4 x 16 tree"""
    b = np.asarray(c.pwb, dtype=np.int64).reshape(10, 10)
    gx, gy = (b[1:9, 2:10] - b[1:9, 0:8]).reshape(64), (b[2:10, 1:9] - b[0:8, 1:9]).reshape(64)
    dv = [np.float32(0.5 * np.float64(np.float32(c.dir[0]) * np.float32(gx[k]) + np.float32(c.dir[1]) * np.float32(gy[k]))) for k in range(64)]
    return ar._serial([d * d for d in dv], False, tree)


def test_exit_classes_cover_every_budget():
    """budgets 0, 1, 2 and 10; converged at iteration 1, strictly inside the budget, on exactly the last allowed iteration, and the budget
    spent -- distinguished by the trace, for align2D (levels 0 to 2) and align1D"""
    for kind, fam in (("2d", "a2d_exit"), ("1d", "a1d_exit")):
        seen = set()
        for c in af.align_families()[fam]:
            m = af.model_align(c)
            if m["exit"] == "converged":
                cls = "first" if m["exit_iter"] == 0 else "last" if m["exit_iter"] == c.n_iter - 1 else "inside"
                if m["exit_iter"] == 0 and c.n_iter == 1:
                    seen.add((1, "last"))
                assert m["iters"] == m["exit_iter"] + 1 and m["ok"]
            else:
                assert m["exit"] == "budget" and m["iters"] == c.n_iter and not m["ok"], c.name
                cls = "spent"
            seen.add((c.n_iter, cls))
        want = {(0, "spent"), (1, "last"), (2, "last"), (2, "spent"), (10, "first"), (10, "inside"), (10, "last"), (10, "spent")}
        if kind == "2d":
            want |= {(1, "spent"), (2, "first")}
            assert {c.level for c in af.align_families()[fam]} == {0, 1, 2}
        assert want <= seen, (kind, want - seen)
        # a converged run on the last allowed iteration and a spent budget differ in nothing but the flag: both ran n_iter iterations
        last = next(c for c in af.align_families()[fam] if c.n_iter == 10 and c.reach.get("exit_iter") == 9 and c.reach["exit"] == "converged")
        spent = next(c for c in af.align_families()[fam] if c.n_iter == 10 and c.reach["exit"] == "budget")
        assert af.oracle_align(last)[2] == af.oracle_align(spent)[2] == 10 and af.oracle_align(last)[0] and not af.oracle_align(spent)[0]


def test_directions_and_levels_are_covered():
    dirs = {c.reach["direction"]: c.dir for c in af.align_families()["a1d_dir"]}
    assert set(dirs) == {"x", "y", "minus_x", "diagonal", "non_unit", "zero"}
    assert abs(np.hypot(*dirs["non_unit"].astype(np.float64)) - 1) > 0.5 and not dirs["zero"].any() and dirs["diagonal"][0] == dirs["diagonal"][1] > 0
    assert {c.level for c in af.align_families()["a2d_border"]} == {0, 1, 2}
    assert [c.level for c in af.align_families()["a2d_last"]] == [0, 1, 2, 3, 4]
    assert {c.reach["side"] for c in af.align_families()["a2d_leaves"]} == {c.reach["side"] for c in af.align_families()["a1d_leaves"]} == {"left", "top", "right", "bottom"}
    assert {(c.image, c.level) for c in af.align_families()["odd"] if c.kind == "2d"} == {("odd", 0), ("odd", 1), ("odd", 2)}


# ---- reach: findMatchDirect ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GROUPS)
def test_match_items_reach_what_they_are_named_for(name):
    grp = af.md_group_named(name)
    cam = af.md_scene()[0]
    for it in grp.items:
        r = it.reach
        if r.get("rejected") == "slot":
            assert not 0 <= it.slot < af.N_KF
            continue
        t = af.md_trace(grp, it)
        if "framed" in r:
            assert t["framed"] == r["framed"], it.name
            if r.get("rejected") == "level":
                assert it.level == af.N_LEVELS
            else:
                assert it.px_ref[0] != int(it.px_ref[0]) or it.px_ref[1] != int(it.px_ref[1])       # a non-integer px_ref
                k = ("left", "top", "right", "bottom").index(r["side"])
                assert t["cmp4"][k] == r["framed"] and all(t["cmp4"][j] for j in range(4) if j != k), it.name    # this comparison decides
            if not r["framed"]:
                assert not t["ok"] and np.array_equal(bits(t["px_cur"]), bits(it.px_cur))
                continue
        if "threshold" in r:
            thr, det = r["threshold"], t["det"]
            assert (det > thr) == r["over"] and abs(det - thr) < 1e-3 * thr, (it.name, det)
            uncapped = {3.0: 0, 12.0: 1, 48.0: 2}[thr] + (1 if r["over"] else 0)
            assert t["search_level"] == min(uncapped, grp.n_pyr_levels - 1), (it.name, t["search_level"])
        if "det_min" in r:                                 # det far over 3 while the level is capped
            assert t["det"] > r["det_min"] and t["search_level"] == grp.n_pyr_levels - 1 and t["det"] / 4 ** t["search_level"] > 3.0, it.name
        if "det_max" in r:
            assert t["det"] < r["det_max"]
        if "source" in r:
            fp = t["footprint"]
            assert fp["source"] == r["source"] and sorted(fp["clipped"]) == sorted(r["clipped"]), (it.name, fp)
            assert (fp["ww"] <= ar.WIN and fp["wh"] <= ar.WIN) == (fp["source"] == "window")
        if r.get("zeroed"):
            assert 0 < t["n_zero"] < 100 and t["align"]["iters"] >= 1, it.name
        if r.get("warp_nan"):
            assert t["warp_nan"] and not t["pwb"].any() and not t["ok"] and np.isnan(t["px_cur"]).all() and t["align"]["exit"] == "nonfinite", it.name
        if r.get("warp_inf"):
            a, _ = ar.inverse_warp(ar.warp_matrix(cam, af.md_scene()[2][0], grp.T_cur_w, it.px_ref, it.f_ref, 0, it.pt), it.px_ref, 0)
            assert np.isinf(a).all() and not t["warp_nan"] and t["n_zero"] == 100 and not t["ok"] and np.isnan(t["px_cur"]).all(), it.name
        if r.get("cur_outside"):
            assert t["align"]["exit"] == "border" and t["align"]["exit_iter"] == 0 and not t["ok"]
            want = np.float32(it.px_cur / (1 << t["search_level"])).astype(np.float64) * (1 << t["search_level"])
            assert np.array_equal(bits(t["px_cur"]), bits(want)) and not np.array_equal(t["px_cur"], it.px_cur), it.name
        if r.get("zero_dir"):
            assert it.edgelet and not it.grad.any() and np.isnan(t["px_cur"]).all() and not t["ok"]
    if name == "md_base":
        inter = [it for it in grp.items if it.reach.get("interleaved")]
        assert [it.edgelet for it in inter] == [j % 2 == 1 for j in range(len(inter))] and len(inter) >= 16
        oks = [af.md_oracle(grp, it)[0] for it in inter]
        assert sum(o for o, it in zip(oks, inter) if it.edgelet) >= 4 and sum(o for o, it in zip(oks, inter) if not it.edgelet) >= 8
        levels = {(it.level, it.reach["side"], it.reach["framed"]) for it in grp.items if "side" in it.reach}
        assert len(levels) == 3 * 4 * 2
    if name.startswith("md_zoom"):
        levels = {af.md_trace(grp, it)["search_level"] for it in grp.items}
        assert levels == set(range(grp.n_pyr_levels)), (name, levels)                        # every level up to the cap, and none above
        assert {it.level for it in grp.items} == {0, 2}
        if grp.n_pyr_levels > 1:                           # search_level > 0: lscale widens the footprint
            it = next(i for i in grp.items if i.reach.get("over") and i.reach["threshold"] == 3.0)
            t = af.md_trace(grp, it)
            A = ar.warp_matrix(cam, af.md_scene()[2][0], grp.T_cur_w, it.px_ref, it.f_ref, it.level, it.pt)
            narrow = ar.footprint(A, it.px_ref, it.level, 0, af.W, af.H)
            assert t["search_level"] == 1 and t["footprint"]["ww"] > narrow["ww"] and t["footprint"]["wh"] > narrow["wh"]


def test_warp_sources_cover_both_sides_of_the_window():
    by = {it.name: it.reach for g in af.md_groups() for it in g.items if "source" in it.reach}
    x32, x33, y32, y33 = by["md_far_x/x_32_y_under"], by["md_far_x/x_33_y_under"], by["md_far_y/y_32_x_under"], by["md_far_y/y_33_x_under"]
    assert (x32["ww"], x32["source"]) == (32, "window") and (x33["ww"], x33["source"]) == (33, "direct") and max(x32["wh"], x33["wh"]) <= 32
    assert (y32["wh"], y32["source"]) == (32, "window") and (y33["wh"], y33["source"]) == (33, "direct") and max(y32["ww"], y33["ww"]) <= 32
    assert by["md_far_x/x_over_y_under"]["source"] == by["md_far_y/y_over_x_under"]["source"] == "direct"
    assert by["md_far_roll45/box_fits"]["source"] == by["md_far_roll45/box_32"]["source"] == "window" and by["md_far_roll45/box_outgrows"]["source"] == "direct"
    clipped = [tuple(r["clipped"]) for n, r in by.items() if n.startswith("md_far_clip/L")]
    for side in ("left", "top", "right", "bottom"):
        assert clipped.count((side,)) == 2                  # reference levels 0 and 1
    assert clipped.count(("left", "top")) == clipped.count(("right", "bottom")) == 2
    # a shrinking warp on both sides of about 1/3.2
    cam, _, kf_poses, _ = af.md_scene()
    grp = af.md_group_named("md_far_y")
    scales = [abs(ar.warp_matrix(cam, kf_poses[0], grp.T_cur_w, it.px_ref, it.f_ref, 0, it.pt)[3]) for it in grp.items]
    assert min(scales) < 1 / 3.2 < max(scales) * 1.1, scales


def test_infinite_inverse_warp_zeroes_the_patch():
    """see the module docstring: reachable, so the oracle zeroes NaN sample coordinates as the device does"""
    import ctypes as C
    cam, _, kf_poses, kf_pyr = af.md_scene()
    for name in ("md_singular_0", "md_singular_1"):
        grp = af.md_group_named(name)
        it = grp.items[0]
        A = ar.warp_matrix(cam, kf_poses[0], grp.T_cur_w, it.px_ref, it.f_ref, 0, it.pt)
        assert A[0] * A[3] - A[2] * A[1] == 0.0 and (A != 0).all()
        img = kf_pyr[0][0]
        out = np.full(100, 7, dtype=np.uint8)
        a, p = orc.f64(A), orc.f64(it.px_ref)
        assert orc.lib().svo_orc_warp_affine(orc._p(a, C.c_double), orc._p(img, C.c_uint8), img.shape[1], img.shape[0], orc._p(p, C.c_double), 0, 0, 5,
                                             orc._p(out, C.c_uint8)) == 1
        assert not out.any()
        for item in grp.items:
            ok, px, sl = af.md_oracle(grp, item)
            assert not ok and np.isnan(px).all() and sl == 0


# ---- the comparison has teeth -------------------------------------------------------------------------------------------------------
def rejected_by(mut):
    """the names of the cases on which the GPU comparison tells the stand-in `mut` from the model"""
    out = []
    if mut in ("warp_clamp", "level_cap", "frame_px"):
        for grp in af.md_groups():
            for it in grp.items:
                if 0 <= it.slot < af.N_KF and not same_match(trace_tuple(grp, it, (mut,)), trace_tuple(grp, it)):
                    out.append(it.name)
        return out
    for c in af.align_cases():
        if not same_align(model_tuple(c, (mut,)), model_tuple(c)):
            out.append(c.name)
    return out


# for each stand-in, cases that must reject it (the families built for that decision)
REJECTS = {
    # (an update of about a pixel moves by 1e-7 relative under another summation order: below the f32 spacing of most pixel coordinates,
    # so few cases tell -- which is the share of patches the kernel's header speaks of)
    "jres_tree": ["a2d_leaves/leaves_left", "a2d_exit/b1_spent", "a2d_last/L2", "a1d_rollback/at_2", "a2d_odd/converges_L1"],
    "min_update_le": ["a2d_exit/min_update_equal"],
    "border_right_bottom": ["a2d_border/main_L0_u156", "a2d_border/main_L1_v56", "a2d_border/odd_L2_u21", "a1d_border/main_L0_v116", "a2d_border/cast_u_cols-4-1e-9"],
    "rollback_no_restore": ["a1d_rollback/at_1", "a1d_rollback/at_2", "a1d_rollback/at_4"],
    "rollback_at_0": ["a1d_rollback/large_chi2_at_0", "a1d_exit/b10_inside", "a1d_dir/x"],
    "warp_clamp": ["md_far_clip/L0_left", "md_far_clip/L0_bottom", "md_far_clip/L1_left+top", "md_far_clip/L1_right"],
    "level_cap": ["md_zoom_n1/det_3_L0_over", "md_zoom_n3/det_48_L0_over", "md_zoom_n3/det_large_L2", "md_zoom_n1/det_large_L0"],
    "frame_px": ["md_base/frame_L1_right_in", "md_base/frame_L2_bottom_in", "md_base/frame_L1_left_in", "md_base/frame_L2_top_in"],
    # align1D returns h_inv = 64 / H(0,0), compared by bits: the full-contrast templates tell at once.  align2D returns no part of H, and a
    # quarter off in one term of a sum of 10^6 (2.4e-7 relative) is below what a refined pixel of one short iteration resolves: there the
    # exactness claim is checked on the sums themselves (the "contrast" reach assertions), and longer ordinary runs tell the stand-in.
    "h_half": ["a1d_hinv/checker_diag", "a1d_hinv/checker_oblique", "a1d_hinv/binary_noise", "a1d_hinv/noise_b", "a2d_exit/b10_inside", "a2d_exit/b10_last"],
}


@pytest.mark.parametrize("mut", MUTATIONS)
def test_wrong_stand_in_is_rejected_by_the_named_cases(mut):
    got = rejected_by(mut)
    missing = [n for n in REJECTS[mut] if n not in got]
    assert not missing, (mut, missing, got)


def test_min_update_equality_case():
    """`<` against `<=` in the min_update test differ only where the squared update EQUALS the threshold: af._equal_update_case builds
    that input, and the two differ in nothing but the iteration count (the second iteration's update is 0)"""
    c = af.align_case_named("a2d_exit/min_update_equal")
    m, le = af.model_align(c), af.model_align(c, ("min_update_le",))
    (u0, v0), (u1, v1) = m["trace"][0], m["trace"][1]
    assert u1 - u0 == 0.5 and v1 == v0                      # the first update is exactly (0.5, 0)
    assert m["H"].tolist() == [65536.0, 0, 0, 0, 65536.0, 0, 0, 0, 64.0]
    assert le["ok"] and le["iters"] == 1 and m["ok"] and m["iters"] == 2 and np.array_equal(m["px"], le["px"]) and np.array_equal(m["px"], [121.0, 91.0])
    assert rejected_by("min_update_le") == [c.name]
