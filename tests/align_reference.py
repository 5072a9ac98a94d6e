"""A plain NumPy f32 model of feature_alignment::align2D / align1D, and a trace of Matcher::findMatchDirect built from the
oracle's own parts -- the definitions tests/test_align_families_cpu.py reads paths from.  No GPU.

The model is scalar np.float32 arithmetic in the reference's order (S/feature_alignment.cpp:35-152 and :167-281, the scalar path):
every product and sum is one f32 operation, the 64 pixels are walked y-then-x, the three weights that contain (1 - subpix) are
formed in f64 and rounded once, Eigen's 3-term dot products are a0 + (a1 + a2).  It must equal oracle/svo_oracle.c
(orc.align2d / orc.align1d) by bits on every case of tests/align_families.py; unlike the C code it returns a trace (the estimate
entering every iteration, the exit reason, chi2) and it can be made wrong on purpose (`mut`), which is how the CPU test shows that the
comparison used on the GPU rejects near-misses.

Behaviour the C code leaves to the platform, defined here: (int)floor(u) of a NaN or an infinity.  x86 gives INT_MIN, gfx950
saturates (NaN -> 0, +inf -> INT_MAX); every one of these values fails the border test, and a NaN additionally the NaN test behind
it.  The only observable result is "loop left, converged false, the non-finite estimate written back"; the model reports it as exit
reason "nonfinite" and never forms an integer from such a value.

Exit reasons: "converged" (at iteration `exit_iter`, counted from 0), "budget" (n_iter iterations ran, none converged), "border"
(the estimate entering iteration `exit_iter` failed the border test; exit_iter == 0: at entry), "nonfinite", "rollback" (align1D:
new_chi2 > chi2 at iteration exit_iter >= 1, the previous step taken back).  `iters` counts the iterations that reached the pixel loop.

Mutations (`mut`, a set of names):
  jres_tree            Jres summed as four partial sums of 16 pixels, then (p0 + p1) + (p2 + p3), instead of serially
  min_update_le        `<=` in the min_update test
  border_right_bottom  the right / bottom border test off by one (`>` for `>=`)
  rollback_no_restore  align1D: the rollback stops without restoring u and v
  rollback_at_0        align1D: the rollback is allowed at iteration 0 (chi2 starts at 0)
  h_half               H(0,0) summed serially in f32 with its first term rounded to a multiple of 1/2
and for the findMatchDirect composition (find_match_direct below):
  warp_clamp           out-of-image warp samples clamped to the image instead of zeroed
  level_cap            the search-level cap off by one (n_pyr_levels instead of n_pyr_levels - 1, bounded by the pyramid)
  frame_px             the reference frame test on px instead of (int)px / (1 << level)
"""
import ctypes as C
import math

import numpy as np

from oracle import orc

F = np.float32
HALF = 4
WIN = 32                # the warp stage's LDS window: WIN_PITCH x WIN_ROWS of csrc/svo_depth_search.h


def _finite(x):
    return bool(np.isfinite(x))


def _jacobians(pwb):
    """(dx, dy) of the 64 pixels in pixel order: 0.5 * central difference, formed in f64 (exact), cast to f32"""
    b = np.asarray(pwb, dtype=np.int64).reshape(10, 10)
    dx = (0.5 * (b[1:9, 2:10] - b[1:9, 0:8])).astype(F).reshape(64)
    dy = (0.5 * (b[2:10, 1:9] - b[0:8, 1:9])).astype(F).reshape(64)
    return dx, dy


def _inverse3f(m):
    """Eigen Matrix3f::inverse(): cofactors / det, the 3-term sums as a0 + (a1 + a2)"""
    M = lambda r, c: m[r * 3 + c]
    cof = lambda i, j: (M((i + 1) % 3, (j + 1) % 3) * M((i + 2) % 3, (j + 2) % 3) -
                        M((i + 1) % 3, (j + 2) % 3) * M((i + 2) % 3, (j + 1) % 3))
    c00, c10, c20 = cof(0, 0), cof(1, 0), cof(2, 0)
    det = c00 * M(0, 0) + (c10 * M(1, 0) + c20 * M(2, 0))
    invdet = F(1.0) / det
    return [c00 * invdet, c10 * invdet, c20 * invdet, cof(0, 1) * invdet, cof(1, 1) * invdet, cof(2, 1) * invdet,
            cof(0, 2) * invdet, cof(1, 2) * invdet, cof(2, 2) * invdet]


def _serial(terms, sub, tree):
    """sum of 64 f32 terms: s -= t (sub) or s += t, serially in pixel order -- or, wrong on purpose, as a 4 x 16 tree"""
    if not tree:
        s = F(0)
        for t in terms:
            s = s - t if sub else s + t
        return s
    p = []
    for k in range(4):
        s = F(0)
        for t in terms[16 * k:16 * k + 16]:
            s = s - t if sub else s + t
        p.append(s)
    return (p[0] + p[1]) + (p[2] + p[3])


def _entry(img, px, mut):
    rows, cols = img.shape
    pad = np.zeros((rows + 2, cols + 2), dtype=np.uint8)          # (only a border test that is wrong on purpose reads the margin)
    pad[:rows, :cols] = img
    return rows, cols, pad, F(np.float64(px[0])), F(np.float64(px[1]))


def _border(u, v, cols, rows, mut):
    """None: inside; else the exit reason"""
    if not (_finite(u) and _finite(v)):
        return "nonfinite"
    u_r, v_r = int(math.floor(u)), int(math.floor(v))
    if "border_right_bottom" in mut:
        out = u_r < HALF or v_r < HALF or u_r > cols - HALF or v_r > rows - HALF
    else:
        out = u_r < HALF or v_r < HALF or u_r >= cols - HALF or v_r >= rows - HALF
    return "border" if out else None


def _weights(u, v):
    u_r, v_r = int(math.floor(u)), int(math.floor(v))
    sx, sy = u - F(u_r), v - F(v_r)
    dsx, dsy = np.float64(sx), np.float64(sy)
    return u_r, v_r, F((1.0 - dsx) * (1.0 - dsy)), F(dsx * (1.0 - dsy)), F((1.0 - dsx) * dsy), sx * sy


def _residuals(pad, u_r, v_r, w, patch, mean_diff):
    wTL, wTR, wBL, wBR = w
    res = []
    for y in range(8):
        r0, r1 = pad[v_r + y - HALF], pad[v_r + y - HALF + 1]
        for x in range(8):
            c = u_r + x - HALF
            sp = wTL * F(r0[c]) + wTR * F(r0[c + 1]) + wBL * F(r1[c]) + wBR * F(r1[c + 1])
            res.append(sp - F(patch[y * 8 + x]) + mean_diff)
    return res


def side_of(px, cols, rows):
    """which border an estimate lies beyond ('' inside): the comparisons of the border test in their order"""
    if not np.isfinite(px).all():
        return "nonfinite"
    u_r, v_r = math.floor(float(F(px[0]))), math.floor(float(F(px[1])))
    return "left" if u_r < HALF else "top" if v_r < HALF else "right" if u_r >= cols - HALF else "bottom" if v_r >= rows - HALF else ""


def align2d(img, pwb, patch, n_iter, px, mut=()):
    """-> dict(ok, px [2] f64, iters, exit, exit_iter, trace [(u, v) entering each iteration that was begun], H [9])"""
    mut = set(mut)
    with np.errstate(all="ignore"):
        rows, cols, pad, u, v = _entry(img, px, mut)
        patch = np.asarray(patch, dtype=np.uint8).reshape(64)
        dx, dy = _jacobians(pwb)
        H = [F(0)] * 9
        for k in range(64):
            J = (dx[k], dy[k], F(1))
            for a in range(3):
                for b in range(3):
                    t = J[a] * J[b]
                    if "h_half" in mut and k == 0 and a == 0 and b == 0:
                        t = F(np.round(np.float64(t) * 2.0) / 2.0)
                    H[a * 3 + b] = H[a * 3 + b] + t
        Hinv = _inverse3f(H)
        mean_diff = F(0)
        trace, ok, iters, reason, exit_iter = [], False, 0, "budget", n_iter
        for it in range(n_iter):
            trace.append((u, v))
            why = _border(u, v, cols, rows, mut)
            if why:
                reason, exit_iter = why, it
                break
            iters += 1
            u_r, v_r, *w = _weights(u, v)
            res = _residuals(pad, u_r, v_r, w, patch, mean_diff)
            tree = "jres_tree" in mut
            J0 = _serial([r * d for r, d in zip(res, dx)], True, tree)
            J1 = _serial([r * d for r, d in zip(res, dy)], True, tree)
            J2 = _serial(res, True, tree)
            up = [Hinv[a * 3] * J0 + (Hinv[a * 3 + 1] * J1 + Hinv[a * 3 + 2] * J2) for a in range(3)]
            u = u + up[0]
            v = v + up[1]
            mean_diff = mean_diff + up[2]
            n2 = up[0] * up[0] + up[1] * up[1]
            if (n2 <= F(0.25)) if "min_update_le" in mut else (n2 < F(0.25)):
                ok, reason, exit_iter = True, "converged", it
                break
    return dict(ok=ok, px=np.array([np.float64(u), np.float64(v)]), iters=iters, exit=reason, exit_iter=exit_iter, trace=trace,
                H=np.array(H, dtype=F))


def align1d(img, direction, pwb, patch, n_iter, px, mut=()):
    """-> dict(ok, px, h_inv (f64), iters, exit, exit_iter, trace, chi2 [new_chi2 of each iteration that ran], H00)"""
    mut = set(mut)
    with np.errstate(all="ignore"):
        rows, cols, pad, u, v = _entry(img, px, mut)
        patch = np.asarray(patch, dtype=np.uint8).reshape(64)
        d0, d1 = F(direction[0]), F(direction[1])
        b = np.asarray(pwb, dtype=np.int64).reshape(10, 10)
        gx = (b[1:9, 2:10] - b[1:9, 0:8]).reshape(64)
        gy = (b[2:10, 1:9] - b[0:8, 1:9]).reshape(64)
        # dir[0] * (int) is an f32 product, the sum of the two an f32 sum, 0.5 * (..) a double product cast to f32 (exact)
        dv = [F(0.5 * np.float64(d0 * F(gx[k]) + d1 * F(gy[k]))) for k in range(64)]
        H00 = H01 = H11 = F(0)
        for k in range(64):
            t = dv[k] * dv[k]
            if "h_half" in mut and k == 0:
                t = F(np.round(np.float64(t) * 2.0) / 2.0)
            H00 = H00 + t
            H01 = H01 + dv[k] * F(1)
            H11 = H11 + F(1) * F(1)
        h_inv = np.float64(1.0) / np.float64(H00) * 8 * 8
        det = H00 * H11 - H01 * H01
        invdet = F(1.0) / det
        Hi = [H11 * invdet, -H01 * invdet, -H01 * invdet, H00 * invdet]
        mean_diff, chi2, up0, up1 = F(0), F(0), F(0), F(0)
        trace, chis, ok, iters, reason, exit_iter = [], [], False, 0, "budget", n_iter
        for it in range(n_iter):
            trace.append((u, v))
            why = _border(u, v, cols, rows, mut)
            if why:
                reason, exit_iter = why, it
                break
            iters += 1
            u_r, v_r, *w = _weights(u, v)
            res = _residuals(pad, u_r, v_r, w, patch, mean_diff)
            tree = "jres_tree" in mut
            J0 = _serial([r * d for r, d in zip(res, dv)], True, tree)
            J1 = _serial(res, True, tree)
            new_chi2 = _serial([r * r for r in res], False, False)
            chis.append(new_chi2)
            if (it > 0 or "rollback_at_0" in mut) and new_chi2 > chi2:
                if "rollback_no_restore" not in mut:
                    u = u - up0
                    v = v - up1
                reason, exit_iter = "rollback", it
                break
            chi2 = new_chi2
            up0 = Hi[0] * J0 + Hi[1] * J1
            up1 = Hi[2] * J0 + Hi[3] * J1
            u = u + up0 * d0
            v = v + up0 * d1
            mean_diff = mean_diff + up1
            n2 = up0 * up0 + up1 * up1
            thr = F(0.03 * 0.03)
            if (n2 <= thr) if "min_update_le" in mut else (n2 < thr):
                ok, reason, exit_iter = True, "converged", it
                break
    return dict(ok=ok, px=np.array([np.float64(u), np.float64(v)]), h_inv=float(h_inv), iters=iters, exit=reason, exit_iter=exit_iter,
                trace=trace, chi2=chis, H00=H00)


# ---- Matcher::findMatchDirect: the oracle's parts, traced -----------------------------------------------------------------------
def _vec(name, n_out, *ins):
    keep = [orc.f64(a) for a in ins]
    out = np.zeros(n_out)
    getattr(orc.lib(), name)(*[orc._p(a, C.c_double) for a in keep], orc._p(out, C.c_double))
    return out


def warp_matrix(cam, T_ref_w, T_cur_w, px_ref, f_ref, level_ref, pt_pos):
    """A_cur_ref of matcher.cpp:171-174 from the oracle's own se3 and warp functions"""
    T_ref_inv = _vec("svo_orc_se3_inverse", 7, T_ref_w)
    T_cur_ref = _vec("svo_orc_se3_mul", 7, T_cur_w, T_ref_inv)
    d = T_ref_inv[:3] - np.asarray(pt_pos, dtype=np.float64)
    depth = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    c = orc.camera(cam)
    A = np.zeros(4)
    p, ff = orc.f64(px_ref), orc.f64(f_ref)
    orc.lib().svo_orc_get_warp_matrix_affine(C.byref(c), C.byref(c), orc._p(p, C.c_double), orc._p(ff, C.c_double), C.c_double(depth),
                                             orc._p(T_cur_ref, C.c_double), C.c_int(level_ref), orc._p(A, C.c_double))
    return A


def frame_test(cam, px_ref, level_ref, mut=()):
    """isInFrame(px.cast<int>() / (1 << level), 6, level): -> (passed, [the four comparisons left, top, right, bottom])"""
    if "frame_px" in mut:
        ox, oy = int(px_ref[0]), int(px_ref[1])
    else:
        ox, oy = int(px_ref[0]) // (1 << level_ref), int(px_ref[1]) // (1 << level_ref)
    w, h = cam.width // (1 << level_ref), cam.height // (1 << level_ref)          # width / (1 << level): abstract_camera.h
    cmp4 = [ox >= 6, oy >= 6, ox < w - 6, oy < h - 6]
    return all(cmp4), cmp4


def inverse_warp(A, px_ref, level_ref):
    """A_ref_cur = A^-1 cast to f32 and the reference pixel on its level, as warp::warpAffine forms them"""
    with np.errstate(all="ignore"):
        det = np.float64(A[0]) * A[3] - np.float64(A[2]) * A[1]
        invdet = np.float64(1.0) / det
        a = [F(A[3] * invdet), F(-A[1] * invdet), F(-A[2] * invdet), F(A[0] * invdet)]
        pr = [F(np.float64(px_ref[0])) / F(1 << level_ref), F(np.float64(px_ref[1])) / F(1 << level_ref)]
    return a, pr


def warp_affine(A, img, px_ref, level_ref, search_level, mut=()):
    """warp::warpAffine of the 10x10 patch (matcher.cpp:83-116) in f32 -> (patch [100] or None where the inverse is NaN, number of
    zeroed samples)"""
    rows, cols = img.shape
    a, pr = inverse_warp(A, px_ref, level_ref)
    if np.isnan(a[0]):
        return None, 100
    out = np.zeros(100, dtype=np.uint8)
    n_zero = 0
    ls = F(1 << search_level)
    with np.errstate(all="ignore"):
        for y in range(10):
            for x in range(10):
                ppx, ppy = F(x - 5) * ls, F(y - 5) * ls
                qx = (a[0] * ppx + a[1] * ppy) + pr[0]
                qy = (a[2] * ppx + a[3] * ppy) + pr[1]
                inside = qx >= 0 and qy >= 0 and qx < cols - 1 and qy < rows - 1       # a NaN coordinate compares false: zeroed
                if not inside:
                    n_zero += 1
                    if "warp_clamp" not in mut or not (_finite(qx) and _finite(qy)):
                        continue
                    qx = min(max(qx, F(0)), np.nextafter(F(cols - 1), F(0)))
                    qy = min(max(qy, F(0)), np.nextafter(F(rows - 1), F(0)))
                ix, iy = int(math.floor(qx)), int(math.floor(qy))
                sx, sy = qx - F(ix), qy - F(iy)
                w00 = (F(1) - sx) * (F(1) - sy)
                w01 = (F(1) - sx) * sy
                w10 = sx * (F(1) - sy)
                w11 = F(1) - w00 - w01 - w10
                val = w00 * F(img[iy, ix]) + w01 * F(img[iy + 1, ix]) + w10 * F(img[iy, ix + 1]) + w11 * F(img[iy + 1, ix + 1])
                out[y * 10 + x] = np.uint8(int(val))
    return out, n_zero


def footprint(A, px_ref, level_ref, search_level, cols, rows):
    """The source footprint of the patch as the warp stage bounds it (the four corners -5 / +4 in f32) and the source its own rule
    then chooses: -> dict(box (xmin, xmax, ymin, ymax) f32, source 'window' | 'direct', ww, wh, clipped [sides])"""
    a, pr = inverse_warp(A, px_ref, level_ref)
    ls = F(1 << search_level)
    with np.errstate(all="ignore"):
        qs = [((a[0] * (F(cx) * ls) + a[1] * (F(cy) * ls)) + pr[0], (a[2] * (F(cx) * ls) + a[3] * (F(cy) * ls)) + pr[1])
              for cy in (-5, 4) for cx in (-5, 4)]
    xs, ys = [q[0] for q in qs], [q[1] for q in qs]
    box = (min(xs), max(xs), min(ys), max(ys))
    out = dict(box=box, source="direct", ww=0, wh=0, clipped=[])
    if np.isnan(a[0]) or not all(_finite(b) and abs(b) < 1e6 for b in box):
        return out
    fx0, fx1, fy0, fy1 = (int(math.floor(b)) for b in box)
    wx0, wy0 = max(fx0, 0), max(fy0, 0)
    wx1, wy1 = min(fx1, cols - 2) + 1, min(fy1, rows - 2) + 1
    out["ww"], out["wh"] = wx1 - wx0 + 1, wy1 - wy0 + 1
    out["clipped"] = [s for s, c in (("left", fx0 < 0), ("top", fy0 < 0), ("right", fx1 > cols - 2), ("bottom", fy1 > rows - 2)) if c]
    if 0 < out["ww"] <= WIN and 0 < out["wh"] <= WIN:
        out["source"] = "window"
    return out


def search_level_of(A, n_pyr_levels, mut=(), n_levels_held=None):
    """-> (det(A), search level): warp::getBestSearchLevel(A, n_pyr_levels - 1)"""
    D = det = float(np.float64(A[0]) * A[3] - np.float64(A[2]) * A[1])
    cap = n_pyr_levels - 1
    if "level_cap" in mut:
        cap = min(n_pyr_levels, (n_levels_held or n_pyr_levels + 1) - 1)
    level = 0
    while D > 3.0 and level < cap:
        level += 1
        D *= 0.25
    return det, level


def find_match_direct(cam, ref_pyr, cur_pyr, T_ref_w, T_cur_w, px_ref, f_ref, level_ref, pt_pos, px_cur, edgelet=False, grad=(1.0, 0.0),
                      n_pyr_levels=3, align_max_iter=10, mut=()):
    """Matcher::findMatchDirect (matcher.cpp:156-202) composed of the oracle's geometry, the f32 warp above and the alignment model,
    with a trace: -> dict(ok, px_cur, search_level, framed, cmp4, det, footprint, n_zero, warp_nan, align (the model's result))"""
    mut = set(mut)
    px_cur = np.array(px_cur, dtype=np.float64)
    framed, cmp4 = (False, [False] * 4) if not 0 <= level_ref < len(ref_pyr) else frame_test(cam, px_ref, level_ref, mut)
    out = dict(ok=False, px_cur=px_cur, search_level=0, framed=framed, cmp4=cmp4)
    if not framed:
        return out
    A = warp_matrix(cam, T_ref_w, T_cur_w, px_ref, f_ref, level_ref, pt_pos)
    det, sl = search_level_of(A, n_pyr_levels, mut, len(cur_pyr))
    img_ref = ref_pyr[level_ref]
    pwb, n_zero = warp_affine(A, img_ref, px_ref, level_ref, sl, mut)
    warp_nan = pwb is None
    if warp_nan:
        pwb = np.zeros(100, dtype=np.uint8)       # (the oracle's and the device's rule; the reference keeps the matcher's last patch)
    patch = pwb.reshape(10, 10)[1:9, 1:9].reshape(64)
    scaled = px_cur / (1 << sl)
    if edgelet:
        d0, d1 = A[0] * grad[0] + A[1] * grad[1], A[2] * grad[0] + A[3] * grad[1]
        n2 = d0 * d0 + d1 * d1
        if n2 > 0.0:
            nn = math.sqrt(n2)
            d0, d1 = d0 / nn, d1 / nn
        al = align1d(cur_pyr[sl], (F(d0), F(d1)), pwb, patch, align_max_iter, scaled, mut)
    else:
        al = align2d(cur_pyr[sl], pwb, patch, align_max_iter, scaled, mut)
    out.update(ok=al["ok"], px_cur=al["px"] * (1 << sl), search_level=sl, det=det, n_zero=n_zero, warp_nan=warp_nan, align=al, pwb=pwb,
               footprint=footprint(A, px_ref, level_ref, sl, img_ref.shape[1], img_ref.shape[0]))
    return out
