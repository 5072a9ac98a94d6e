"""The matcher and the depth filter on images whose pyramid levels have odd widths (346x260 -> 173x130, 86x65;
202x134 -> 101x67, 50x33; 100x68 -> 50x34, 25x17): the row stride is odd, image rows start at every byte alignment, level
offsets are rounded up, and the last row of the last level ends next to the allocation's tail slack -- what the kernels'
unaligned 8- and 12-byte row loads and 32-bit patch staging have to cope with.  The epipolar search, df_align, align2d,
align1d, match_direct and reproject_cells against the CPU oracle exactly as the 640x480 tests compare them.
tests/test_oracle_seed_edges.py proves on the CPU that the depth-filter scenes cover the branches."""
import numpy as np
import pytest

from android_svo_amd import hip, synth
from oracle import orc

import seed_reference as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


def _bits_equal(got, want):
    np.testing.assert_array_equal(np.ascontiguousarray(got, dtype=np.float64).view(np.uint64),
                                  np.ascontiguousarray(want, dtype=np.float64).view(np.uint64))


@pytest.mark.parametrize("size", sr.ODD_SIZES, ids=lambda s: "%dx%d" % s)
def test_depth_filter_on_odd_pyramids(ctx, size):
    """Every branch of updateSeeds / findEpipolarMatchDirect (the recipe of test_depth_filter_all_paths, scaled down) through
    svo_hip_depth_filter_update and through a resident seed batch: statuses, ZMSSD evaluations, align iterations and search
    levels equal to the oracle's, the matched pixel bit for bit, z within 1e-12, the seed state by the rule of
    test_update_seed_kernel_against_the_oracle (99.9 % of the seeds bit-equal, the rest within 3e-6).

    Observed on the MI355X: seeds with a bit-equal state 3000 of 3000 (346x260), 2400 of 2400 (202x134), 1500 of 1500 (100x68)."""
    oc = sr.odd_df_case(*size)
    sc = oc.sc
    n = len(sc.px)
    o, want = sr.oracle_pass(sc, (sc.a, sc.b, sc.mu, sc.sigma2), T_cur_w=oc.T_cur_w)
    counts, n_multi, n_direct = sr.odd_branch_counts(o)
    assert (counts[:4] >= sr.ODD_MIN_STATUS).all() and n_multi >= sr.ODD_MIN_MULTI and n_direct >= sr.ODD_MIN_DIRECT
    kf = hip.Pyramid(ctx, size[0], size[1], 5, 1)
    cf = hip.Pyramid(ctx, size[0], size[1], 5, 1)
    kf.upload(0, sc.ref_pyr)
    cf.upload(0, sc.cur_pyr)
    sb = hip.SeedBatch(ctx, sc.px, sc.f, sc.level, sc.a, sc.b, sc.mu, sc.z_range, sc.sigma2)
    hip.depth_filter_update(ctx, kf, 0, cf, 0, sc.cam, sc.T_ref_w, oc.T_cur_w, sb)
    st = sb.status.download()
    np.testing.assert_array_equal(st, o["status"])
    np.testing.assert_array_equal(sb.n_zmssd.download(), o["n_zmssd"])
    np.testing.assert_array_equal(sb.n_align.download(), o["n_align_iters"])
    np.testing.assert_array_equal(sb.search_level.download(), o["search_level"])
    _bits_equal(sb.px_cur.download(), o["px_cur"])
    upd = st >= hip.SEED_UPDATED
    np.testing.assert_allclose(sb.z.download()[upd], o["z"][upd], rtol=1e-12)
    got = (sb.a.download(), sb.b.download(), sb.mu.download(), sb.sigma2.download())
    same = sr.state_same_bits(got, want)
    print("odd pyramids %dx%d: statuses %s, %d multi-chunk, %d direct-align, %d of %d states bit-equal" %
          (size[0], size[1], counts.tolist(), n_multi, n_direct, same.sum(), n))
    assert same.mean() >= 0.999, same.mean()
    sr.assert_remainder_close(got, want, same, "%dx%d" % size)
    assert same[st <= hip.SEED_NO_MATCH].all()                       # untouched, or b + 1: exact
    # the same pass through a device-resident batch: the same bits as the stateless entry
    rs = hip.ResidentSeeds(ctx, sc.px, sc.f, sc.level, sc.a, sc.b, sc.mu, sc.z_range, sc.sigma2)
    ev, ev_counts = rs.update(kf, 0, cf, 0, sc.cam, sc.T_ref_w, oc.T_cur_w)
    np.testing.assert_array_equal(rs.status(), o["status"])
    d = rs.download()
    assert sr.state_same_bits(tuple(d[k] for k in ("a", "b", "mu", "sigma2")), got).all()
    assert ev_counts[1:].tolist() == counts.tolist() and len(ev) == int(counts[4] + counts[5])
    ev = ev[np.argsort(ev["index"])]
    conv = np.where(st == hip.SEED_CONVERGED)[0]
    np.testing.assert_array_equal(ev["index"][ev["status"] == hip.SEED_CONVERGED], conv)
    _bits_equal(ev["px_cur"][ev["status"] == hip.SEED_CONVERGED], o["px_cur"][conv])
    rs.destroy()
    sb.free(); kf.destroy(); cf.destroy()


@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("size", sr.ODD_SIZES, ids=lambda s: "%dx%d" % s)
def test_align_on_odd_pyramid_levels(ctx, size, level):
    """align2d and align1d on one level of an odd-sized pyramid, 600 patches, a quarter each within 5-8 px of the right
    border, of the bottom border, and an eighth in the bottom-right corner (the end of the level): flags and iteration
    counts equal to the oracle's, pixels and h_inv bit-identical; ragged batch sizes give the same per-patch answers."""
    ac, img, pwb, patch, px_init, dirs = sr.odd_align_case(size[0], size[1], level)
    n = len(px_init)
    assert img.shape == (size[1] >> level, size[0] >> level)
    pyr = hip.Pyramid(ctx, size[0], size[1], 5, 1)
    pyr.upload(0, ac.cur_pyr)
    conv, px, iters = hip.align2d_batch(ctx, pyr, 0, level, pwb, patch, 10, px_init)
    ok_o, px_o, it_o = np.zeros(n, bool), np.zeros((n, 2)), np.zeros(n, np.int32)
    for i in range(n):
        ok_o[i], px_o[i], it_o[i] = orc.align2d(img, pwb[i], patch[i], 10, px_init[i])
    np.testing.assert_array_equal(conv, ok_o)
    np.testing.assert_array_equal(iters, it_o)
    _bits_equal(px, px_o)
    assert ok_o.sum() > n // 4 and (~ok_o).sum() > 10                # converged ones and ones that ran into the border
    c1, p1, h1, i1 = hip.align1d_batch(ctx, pyr, 0, level, pwb, dirs, 10, px_init)
    ok1, px1, hi1, it1 = np.zeros(n, bool), np.zeros((n, 2)), np.zeros(n), np.zeros(n, np.int32)
    for i in range(n):
        ok1[i], px1[i], hi1[i], it1[i] = orc.align1d(img, dirs[i], pwb[i], patch[i], 10, px_init[i])
    np.testing.assert_array_equal(c1, ok1)
    np.testing.assert_array_equal(i1, it1)
    _bits_equal(p1, px1)
    _bits_equal(h1, hi1)
    for m in (1, 63, 65):
        # m patches of the right-border block and m of the corner block
        for sel in (slice(0, m), slice(n // 2, n // 2 + m)):
            c, p, it = hip.align2d_batch(ctx, pyr, 0, level, pwb[sel], patch[sel], 10, px_init[sel])
            np.testing.assert_array_equal(c, ok_o[sel])
            np.testing.assert_array_equal(it, it_o[sel])
            _bits_equal(p, px_o[sel])
            c, p, h, it = hip.align1d_batch(ctx, pyr, 0, level, pwb[sel], dirs[sel], 10, px_init[sel])
            np.testing.assert_array_equal(c, ok1[sel])
            _bits_equal(p, px1[sel])
            _bits_equal(h, hi1[sel])
    pyr.destroy()


@pytest.mark.parametrize("size", sr.ODD_SIZES, ids=lambda s: "%dx%d" % s)
def test_match_direct_on_odd_pyramids(ctx, size):
    """Matcher::findMatchDirect (the scene of test_match_direct_batch at an odd size): map points of 3 keyframes matched into
    a new frame, reference features on levels 0-2 right up to the image border, corners and edgelets."""
    w, h = size
    rng = np.random.default_rng(17 + w)
    cam = synth.Camera.default(w, h)
    scene = synth.PlaneScene(seed=33, depth=2.0, tilt=(0.1, -0.07))
    kf_poses = [synth.se3_from_twist(rng.uniform(-0.03, 0.03, 3) + [0, 0, 0.1 * k], rng.uniform(-0.02, 0.02, 3)) for k in range(3)]
    T_cur_w = synth.se3_from_twist(rng.uniform(-0.02, 0.02, 3) + [0, 0, 0.25], rng.uniform(-0.01, 0.01, 3))
    kf_pyr = [synth.build_pyramid(scene.render(cam, T)) for T in kf_poses]
    cur_pyr = synth.build_pyramid(scene.render(cam, T_cur_w))
    ref = hip.Pyramid(ctx, w, h, 5, 3)
    cur = hip.Pyramid(ctx, w, h, 5, 1)
    for k in range(3):
        ref.upload(k, kf_pyr[k])
    cur.upload(0, cur_pyr)
    n = 600
    slot = rng.integers(0, 3, n).astype(np.int32)
    level = rng.choice([0, 0, 1, 2] if w > 100 else [0, 0, 1], n).astype(np.int32)
    px_ref = np.stack([rng.uniform(2, w - 2, n), rng.uniform(2, h - 2, n)], axis=1)             # some fail the frame test
    f_ref = synth.cam2world(cam, px_ref)
    pt = np.zeros((n, 3))
    for k in range(3):
        m = slot == k
        pt[m] = scene.intersect(cam, kf_poses[k], px_ref[m, 0], px_ref[m, 1])
    Xc = pt @ synth.rot_matrix(T_cur_w[3:]).T + T_cur_w[:3]
    px_cur = np.stack([cam.fx * Xc[:, 0] / Xc[:, 2] + cam.cx, cam.fy * Xc[:, 1] / Xc[:, 2] + cam.cy], axis=1)
    px_cur += rng.uniform(-1.5, 1.5, (n, 2))
    edge = (rng.uniform(size=n) < 0.2).astype(np.uint8)
    grad = rng.normal(size=(n, 2))
    grad /= np.linalg.norm(grad, axis=1, keepdims=True)
    ok, px_out, sl = hip.match_direct_batch(ctx, ref, cur, 0, cam, np.stack(kf_poses), T_cur_w, slot, px_ref, f_ref, level, pt,
                                            px_cur, edgelet=edge, grad=grad)
    ok_o, px_o, sl_o = np.zeros(n, bool), np.zeros((n, 2)), np.zeros(n, np.int32)
    for i in range(n):
        ok_o[i], px_o[i], sl_o[i] = orc.find_match_direct(cam, kf_pyr[slot[i]], cur_pyr, kf_poses[slot[i]], T_cur_w, px_ref[i],
                                                         f_ref[i], int(level[i]), pt[i], px_cur[i], edgelet=bool(edge[i]),
                                                         grad=grad[i])
    framed = np.array([(int(p[0]) // (1 << l) >= 6) and (int(p[0]) // (1 << l) < (w >> l) - 6) and
                       (int(p[1]) // (1 << l) >= 6) and (int(p[1]) // (1 << l) < (h >> l) - 6) for p, l in zip(px_ref, level)])
    assert (~framed).sum() > 10 and not ok[~framed].any()
    np.testing.assert_array_equal(px_out[~framed], px_cur[~framed])        # untouched when the frame test fails
    np.testing.assert_array_equal(sl[framed], sl_o[framed])
    np.testing.assert_array_equal(ok, ok_o)
    _bits_equal(px_out[framed], px_o[framed])
    print("match_direct %dx%d: %d framed, %d corners and %d edgelets matched" %
          (w, h, framed.sum(), (framed & (edge == 0) & ok).sum(), (framed & (edge == 1) & ok).sum()))
    assert (framed & (edge == 0) & ok).sum() > 100 and (framed & (edge == 1) & ok).sum() > 10
    ref.destroy(); cur.destroy()


@pytest.mark.parametrize("max_fts", [1200, 40])
def test_reproject_cells_on_an_odd_pyramid(ctx, max_fts):
    """svo_hip_reproject_cells on a 346x260 frame (cells of 20 px: the last column and row of cells are cut): tried / matched
    flags, search levels, cell winners and counters equal to the oracle's, matched pixels bit-identical."""
    cs = synth.make_reproject_case(width=346, height=260)
    cam = cs["cam"]
    ref = hip.Pyramid(ctx, cam.width, cam.height, 5, 3)
    cur = hip.Pyramid(ctx, cam.width, cam.height, 5, 1)
    for k in range(3):
        ref.upload(k, cs["kf_pyr"][k])
    cur.upload(0, cs["cur_pyr"])
    off, ids = synth.flatten_cells(cs, cs["trial"])
    deleted = (cs["ptype"][ids] == synth.TYPE_DELETED).astype(np.uint8)
    res = hip.reproject_cells(ctx, ref, cur, 0, cam, cs["T_kf_w"], cs["T_cur_w"], off, cs["slot"][ids], cs["px_ref"][ids],
                              cs["f_ref"][ids], cs["level"][ids], cs["pos"][ids], deleted, cs["px_cur"][ids], max_fts=max_fts)
    o = orc.reproject_cells(cam, cs["kf_pyr"], cs["T_kf_w"], cs["cur_pyr"], cs["T_cur_w"], off, cs["slot"][ids], cs["px_ref"][ids],
                            cs["f_ref"][ids], cs["level"][ids], cs["pos"][ids], np.zeros(len(ids), np.uint8),
                            np.tile([1.0, 0.0], (len(ids), 1)), deleted, cs["px_cur"][ids], max_fts=max_fts)
    for key in ("tried", "matched", "cell_winner"):
        np.testing.assert_array_equal(res[key], o[key], err_msg=key)
    hit = o["matched"].astype(bool)
    np.testing.assert_array_equal(res["search_level"][hit], o["search_level"][hit])
    assert res["n_matches"] == o["n_matches"] and res["n_trials"] == o["n_trials"]
    _bits_equal(res["px_cur"][hit], o["px_cur"][hit])
    assert o["n_matches"] >= (40 if max_fts == 40 else 100) and o["n_trials"] > o["n_matches"]
    ref.destroy(); cur.destroy()
