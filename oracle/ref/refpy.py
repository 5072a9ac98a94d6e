"""ctypes binding of oracle/_ref/libsvo_ref.so (the reference's own code, built by
`make -C oracle ref` where /root/reference is mounted) -- TEST INFRASTRUCTURE ONLY.
Used to generate tests/golden/* and, when present, for live cross-checks of the
C restatement.  `available()` is False on the GPU box unless the prebuilt .so travelled.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .. import orc

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(os.path.dirname(_HERE), "_ref", "libsvo_ref.so")
_lib = None


def available() -> bool:
    return os.path.exists(_LIB_PATH)


def lib():
    global _lib
    if _lib is None:
        # RTLD_LAZY: sparse_img_align.o keeps unresolved references to OpenCV functions on paths that are never
        # called (see oracle/ref/ref_objects.cpp); ctypes' default mode would insist on resolving them
        _lib = C.CDLL(_LIB_PATH, mode=os.RTLD_LAZY)
        _lib.ref_interpolate_8u.restype = C.c_float
    return _lib


_p = orc._p
f64 = orc.f64
D = C.c_double


def _call_vec(name, n_out, *ins):
    out = np.zeros(n_out)
    args = [_p(f64(a), D) for a in ins]
    keep = [f64(a) for a in ins]
    args = [_p(a, D) for a in keep]
    getattr(lib(), name)(*args, _p(out, D))
    return out


def se3_mul(A, B): return _call_vec("ref_se3_mul", 7, A, B)
def se3_inverse(A): return _call_vec("ref_se3_inverse", 7, A)
def se3_act(A, p): return _call_vec("ref_se3_act", 3, A, p)
def se3_exp(l): return _call_vec("ref_se3_exp", 7, l)
def so3_log(q): return _call_vec("ref_so3_log", 3, q)
def rotation_matrix(A): return _call_vec("ref_se3_rotation_matrix", 9, A)
def jacobian_xyz2uv(p): return _call_vec("ref_jacobian_xyz2uv", 12, p)
def ldlt6_solve(H, b): return _call_vec("ref_ldlt6_solve", 6, np.asarray(H).reshape(36), b)


def driven_sparse_align(fp, max_level=4, min_level=0, n_iter=30, eps=1e-6, T_cur_w_init=None):
    cam = orc.camera(fp.cam)
    rp, cp = orc.pyr_ptrs(fp.ref_pyr), orc.pyr_ptrs(fp.cur_pyr)
    px, f, pos = f64(fp.px), f64(fp.f), f64(fp.pos)
    hp = np.ascontiguousarray(fp.has_point, dtype=np.uint8)
    T_ref = f64(fp.T_ref_w)
    T_init = f64(fp.T_cur_w_init if T_cur_w_init is None else T_cur_w_init)
    T_out = np.zeros(7)
    nt = C.c_size_t(0)
    chi2 = D(0)
    iters = np.zeros(8, dtype=np.int32)
    H = np.zeros(36)
    lib().ref_driven_sparse_align(C.byref(cam), rp, cp, C.c_int(len(px)), _p(px, D), _p(f, D), _p(pos, D),
                                  _p(hp, C.c_uint8), _p(T_ref, D), _p(T_init, D), C.c_int(max_level),
                                  C.c_int(min_level), C.c_int(n_iter), D(eps), _p(T_out, D), C.byref(nt),
                                  C.byref(chi2), _p(iters, C.c_int), _p(H, D))
    return {"T_cur_w": T_out, "n_tracked": nt.value, "chi2": chi2.value, "iters": iters, "H": H}


def align2d(img, pwb, patch, n_iter, px):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    pwb = np.ascontiguousarray(pwb, dtype=np.uint8)
    patch = np.ascontiguousarray(patch, dtype=np.uint8)
    p = f64(px).copy()
    ok = lib().ref_align2d(_p(img, C.c_uint8), img.shape[1], img.shape[0], img.shape[1], _p(pwb, C.c_uint8),
                           _p(patch, C.c_uint8), n_iter, _p(p, D))
    return bool(ok), p


def align1d(img, direction, pwb, patch, n_iter, px):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    pwb = np.ascontiguousarray(pwb, dtype=np.uint8)
    patch = np.ascontiguousarray(patch, dtype=np.uint8)
    d = np.ascontiguousarray(direction, dtype=np.float32)
    p = f64(px).copy()
    hinv = D(0)
    ok = lib().ref_align1d(_p(img, C.c_uint8), img.shape[1], img.shape[0], img.shape[1], _p(d, C.c_float),
                           _p(pwb, C.c_uint8), _p(patch, C.c_uint8), n_iter, _p(p, D), C.byref(hinv))
    return bool(ok), p, hinv.value


def zmssd(ref_patch, img, x0, y0):
    ref_patch = np.ascontiguousarray(ref_patch, dtype=np.uint8)
    img = np.ascontiguousarray(img, dtype=np.uint8)
    ptr = C.cast(img.ctypes.data + y0 * img.shape[1] + x0, C.POINTER(C.c_uint8))
    return lib().ref_zmssd(_p(ref_patch, C.c_uint8), ptr, img.shape[1])


def get_warp_matrix_affine(cam, px_ref, f_ref, depth_ref, T_cur_ref, level_ref):
    A = np.zeros(4)
    p, ff, T = f64(px_ref), f64(f_ref), f64(T_cur_ref)
    lib().ref_get_warp_matrix_affine(C.c_int(cam.width), C.c_int(cam.height), D(cam.fx), D(cam.fy), D(cam.cx),
                                     D(cam.cy), _p(p, D), _p(ff, D), D(depth_ref), _p(T, D),
                                     C.c_int(level_ref), _p(A, D))
    return A


def get_best_search_level(A, max_level):
    a = f64(A)
    return lib().ref_get_best_search_level(_p(a, D), C.c_int(max_level))


def warp_affine(A, img, px_ref, level_ref, search_level, halfpatch_size):
    a, p = f64(A), f64(px_ref)
    img = np.ascontiguousarray(img, dtype=np.uint8)
    n = 2 * halfpatch_size
    patch = np.full(n * n, 7, dtype=np.uint8)
    lib().ref_warp_affine(_p(a, D), _p(img, C.c_uint8), img.shape[1], img.shape[0], _p(p, D),
                          C.c_int(level_ref), C.c_int(search_level), C.c_int(halfpatch_size),
                          _p(patch, C.c_uint8))
    return patch


def patch_from_border(pwb):
    pwb = np.ascontiguousarray(pwb, dtype=np.uint8)
    out = np.zeros(64, dtype=np.uint8)
    lib().ref_patch_from_border(_p(pwb, C.c_uint8), _p(out, C.c_uint8))
    return out


def depth_from_triangulation(T_search_ref, f_ref, f_cur):
    T, a, b = f64(T_search_ref), f64(f_ref), f64(f_cur)
    d = D(0)
    ok = lib().ref_depth_from_triangulation(_p(T, D), _p(a, D), _p(b, D), C.byref(d))
    return bool(ok), d.value


def cam2world(cam, u, v):
    out = np.zeros(3)
    lib().ref_cam2world(C.c_int(cam.width), C.c_int(cam.height), D(cam.fx), D(cam.fy), D(cam.cx), D(cam.cy),
                        D(u), D(v), _p(out, D))
    return out


def interpolate_8u(img, u, v):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    return float(lib().ref_interpolate_8u(_p(img, C.c_uint8), img.shape[1], img.shape[0], C.c_float(u),
                                          C.c_float(v)))


def half_sample(img, force_scalar=False):
    """SSE2 path when the buffer is 16-byte aligned and cols%16==0, else the scalar path."""
    h, w = img.shape
    raw = np.zeros(h * w + 64, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16
    if force_scalar:
        off += 1
    a = raw[off:off + h * w].reshape(h, w)
    a[:] = img
    rawo = np.zeros((h // 2) * (w // 2) + 64, dtype=np.uint8)
    offo = (-rawo.ctypes.data) % 16
    o = rawo[offo:offo + (h // 2) * (w // 2)].reshape(h // 2, w // 2)
    lib().ref_half_sample(_p(a, C.c_uint8), w, h, _p(o, C.c_uint8))
    return o.copy()


# ---- the reference's own SparseImgAlign / Matcher member functions on real objects (ref_objects.cpp) ----
def _cam_args(cam):
    return (C.c_int(cam.width), C.c_int(cam.height), D(cam.fx), D(cam.fy), D(cam.cx), D(cam.cy))


def _set_distortion(fp):
    """radtan coefficients (fp.dist) of the camera of the next SparseImgAlign harness call: the reference's compiled
    vk::PinholeCamera::world2cam on a hand-laid camera object; None / all zero: the distortion-free harness camera"""
    d = getattr(fp, "dist", None) if fp is not None else None
    d5 = f64(d if d is not None else np.zeros(5))
    lib().ref_set_distortion(_p(d5, D))


def sparse_img_align_run(fp, max_level=4, min_level=0, n_iter=30, T_cur_w_init=None, method=0, scale_estimator=0, weight_function=0):
    """method 0 GaussNewton / 1 LevenbergMarquardt, scale_estimator / weight_function: the reference's enums
    (nlls_solver.h:47-48), set through its own setRobustCostFunction."""
    rp, cp = orc.pyr_ptrs(fp.ref_pyr), orc.pyr_ptrs(fp.cur_pyr)
    px, f, pos = f64(fp.px), f64(fp.f), f64(fp.pos)
    n = len(px)
    hp = np.ascontiguousarray(fp.has_point, dtype=np.uint8)
    T_ref = f64(fp.T_ref_w)
    T_init = f64(fp.T_cur_w_init if T_cur_w_init is None else T_cur_w_init)
    T_out, H = np.zeros(7), np.zeros(36)
    nt, chi2, stop = C.c_size_t(0), D(0), C.c_int(0)
    iters = np.zeros(8, dtype=np.int32)
    n_meas = np.zeros(8, dtype=np.uint64)
    cache = np.zeros((max(n, 1), 16), dtype=np.float32)
    jac = np.zeros((max(n, 1) * 16, 6))
    vis = np.zeros(max(n, 1), dtype=np.uint8)
    smn = np.zeros(3)
    _set_distortion(fp)
    lib().ref_sparse_img_align_run_ex(*_cam_args(fp.cam), C.c_int(len(fp.ref_pyr)), rp, cp, C.c_int(n), _p(px, D), _p(f, D),
                                      _p(pos, D), _p(hp, C.c_uint8), _p(T_ref, D), _p(T_init, D), C.c_int(max_level),
                                      C.c_int(min_level), C.c_int(n_iter), C.c_int(method), C.c_int(scale_estimator),
                                      C.c_int(weight_function), _p(T_out, D), C.byref(nt), _p(H, D),
                                      C.byref(chi2), C.byref(stop), _p(iters, C.c_int), _p(n_meas, C.c_size_t),
                                      _p(cache, C.c_float), _p(jac, D), _p(vis, C.c_uint8), _p(smn, D))
    _set_distortion(None)
    return {"scale": np.float32(smn[0]), "mu": smn[1], "nu": smn[2], "T_cur_w": T_out, "n_tracked": nt.value, "H": H, "chi2": chi2.value, "stop": stop.value, "iter": iters,
            "n_meas": n_meas, "ref_patch_cache": cache[:n], "jacobian_cache": jac[:n * 16], "visible": vis[:n]}


def sparse_img_align_fixed_work(fp, max_level=4, min_level=0, n_iter=30, T_cur_w_init=None):
    """Exactly n_iter evaluations per level through the reference's compiled computeResiduals / solve / update (the loop
    around them is the harness's: the reference's own has an unconditional error-increase exit)."""
    rp, cp = orc.pyr_ptrs(fp.ref_pyr), orc.pyr_ptrs(fp.cur_pyr)
    px, f, pos = f64(fp.px), f64(fp.f), f64(fp.pos)
    hp = np.ascontiguousarray(fp.has_point, dtype=np.uint8)
    T_ref = f64(fp.T_ref_w)
    T_init = f64(fp.T_cur_w_init if T_cur_w_init is None else T_cur_w_init)
    T_out, H = np.zeros(7), np.zeros(36)
    nt, chi2 = C.c_size_t(0), D(0)
    _set_distortion(fp)
    lib().ref_sparse_img_align_run_fixed_work(*_cam_args(fp.cam), C.c_int(len(fp.ref_pyr)), rp, cp, C.c_int(len(px)), _p(px, D), _p(f, D),
                                              _p(pos, D), _p(hp, C.c_uint8), _p(T_ref, D), _p(T_init, D), C.c_int(max_level),
                                              C.c_int(min_level), C.c_int(n_iter), _p(T_out, D), C.byref(nt), _p(H, D), C.byref(chi2))
    _set_distortion(None)
    return {"T_cur_w": T_out, "n_tracked": nt.value, "H": H, "chi2": chi2.value}


def find_epipolar_match_direct(cam, ref_pyr, cur_pyr, T_ref_w, T_cur_w, px_ref, f_ref, level_ref, d_estimate, d_min,
                               d_max):
    rp, cp = orc.pyr_ptrs(ref_pyr), orc.pyr_ptrs(cur_pyr)
    Tr, Tc, p, ff = f64(T_ref_w), f64(T_cur_w), f64(px_ref), f64(f_ref)
    depth, epi = D(0), D(0)
    px_cur = np.zeros(2)
    lvl = C.c_int(0)
    pwb = np.zeros(100, dtype=np.uint8)
    ok = lib().ref_find_epipolar_match_direct(*_cam_args(cam), C.c_int(len(ref_pyr)), rp, cp, _p(Tr, D), _p(Tc, D),
                                              _p(p, D), _p(ff, D), C.c_int(level_ref), D(d_estimate), D(d_min),
                                              D(d_max), C.byref(depth), _p(px_cur, D), C.byref(lvl), C.byref(epi),
                                              _p(pwb, C.c_uint8))
    return {"ok": bool(ok), "depth": depth.value, "px_cur": px_cur, "search_level": lvl.value,
            "epi_length": epi.value, "patch_with_border": pwb}


def find_match_direct(cam, ref_pyr, cur_pyr, T_ref_w, T_cur_w, px_ref, f_ref, level_ref, pt_pos, px_cur, edgelet=False,
                      grad=(1.0, 0.0), n_pyr_levels=None):
    """n_pyr_levels: Config::nPyrLevels() for this call (None: the reference's 3)"""
    if n_pyr_levels is not None:
        lib().ref_set_match_n_pyr_levels(C.c_int(int(n_pyr_levels)))
        try:
            return find_match_direct(cam, ref_pyr, cur_pyr, T_ref_w, T_cur_w, px_ref, f_ref, level_ref, pt_pos, px_cur, edgelet, grad)
        finally:
            lib().ref_set_match_n_pyr_levels(C.c_int(0))
    rp, cp = orc.pyr_ptrs(ref_pyr), orc.pyr_ptrs(cur_pyr)
    Tr, Tc, p, ff, pp, g = f64(T_ref_w), f64(T_cur_w), f64(px_ref), f64(f_ref), f64(pt_pos), f64(grad)
    pc = f64(px_cur).copy()
    lvl = C.c_int(0)
    ok = lib().ref_find_match_direct(*_cam_args(cam), C.c_int(len(ref_pyr)), rp, cp, _p(Tr, D), _p(Tc, D), _p(p, D),
                                     _p(ff, D), C.c_int(level_ref), _p(pp, D), C.c_int(1 if edgelet else 0), _p(g, D),
                                     _p(pc, D), C.byref(lvl))
    return {"ok": bool(ok), "px_cur": pc, "search_level": lvl.value}


# ---- next rows f-4 ----
def point_optimize(pos, obs_T, obs_f, n_iter=5):
    p = f64(pos).copy()
    T, ff = f64(obs_T), f64(obs_f)
    lib().ref_point_optimize(C.c_int(n_iter), _p(p, D), C.c_int(len(T)), _p(T, D), _p(ff, D))
    return p


def tukey_weight(x):
    lib().ref_tukey_weight.restype = C.c_float
    return float(lib().ref_tukey_weight(C.c_float(x)))


def mad_scale(errors):
    e = np.ascontiguousarray(errors, dtype=np.float32)
    lib().ref_mad_scale.restype = C.c_float
    return float(lib().ref_mad_scale(_p(e, C.c_float), C.c_int(len(e))))


def median_d(data):
    d = f64(data)
    lib().ref_median_d.restype = D
    return float(lib().ref_median_d(_p(d, D), C.c_int(len(d))))


def inverse6(A): return _call_vec("ref_inverse6", 36, np.asarray(A).reshape(36)).reshape(6, 6)
def ldlt3_solve(A, b): return _call_vec("ref_ldlt3_solve", 3, np.asarray(A).reshape(9), b)


def shi_tomasi_score(img, u, v):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    lib().ref_shi_tomasi_score.restype = C.c_float
    return float(lib().ref_shi_tomasi_score(_p(img, C.c_uint8), img.shape[1], img.shape[0], C.c_int(u), C.c_int(v)))


# ---- next row f-2: the cell loop of Reprojector::reprojectMap on a real Reprojector (ref_objects.cpp) ----
def reproject_cells(cam, kf_pyrs, T_kf_w, cur_pyr, T_cur_w, cell_offset, kf_slot, px_ref, f_ref, level_ref, pt_pos, edgelet,
                    grad, point_type, n_failed, n_succeeded, px_cur, max_fts=1200):
    n_kf, n_cells, n = len(kf_pyrs), len(cell_offset) - 1, int(cell_offset[-1])
    kp = (C.POINTER(C.POINTER(C.c_uint8)) * n_kf)()
    keep = []
    for k in range(n_kf):
        pp = orc.pyr_ptrs(kf_pyrs[k])
        keep.append(pp)
        kp[k] = C.cast(pp, C.POINTER(C.POINTER(C.c_uint8)))
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    co, ks, lr, pt, nf, ns = i32(cell_offset), i32(kf_slot), i32(level_ref), i32(point_type), i32(n_failed), i32(n_succeeded)
    Tk, Tc, pr, fr, pp3, gr, pc = f64(T_kf_w), f64(T_cur_w), f64(px_ref), f64(f_ref), f64(pt_pos), f64(grad), f64(px_cur)
    ed = np.ascontiguousarray(edgelet, dtype=np.uint8)
    nf_o, ns_o, ty_o = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    left = np.zeros(n, np.uint8)
    fc, fpx, fl, ft, fg = np.zeros(n_cells, np.int32), np.zeros((n_cells, 2)), np.zeros(n_cells, np.int32), np.zeros(n_cells, np.int32), np.zeros((n_cells, 2))
    nm, nt = C.c_size_t(0), C.c_size_t(0)
    I = C.c_int
    k = lib().ref_reproject_cells(*_cam_args(cam), C.c_int(len(cur_pyr)), C.c_int(n_kf), kp, _p(Tk, D), orc.pyr_ptrs(cur_pyr), _p(Tc, D),
                                  C.c_int(n_cells), _p(co, I), _p(ks, I), _p(pr, D), _p(fr, D), _p(lr, I), _p(pp3, D),
                                  _p(ed, C.c_uint8), _p(gr, D), _p(pt, I), _p(nf, I), _p(ns, I), _p(pc, D), C.c_int(max_fts),
                                  _p(nf_o, I), _p(ns_o, I), _p(ty_o, I), _p(left, C.c_uint8), _p(fc, I), _p(fpx, D), _p(fl, I),
                                  _p(ft, I), _p(fg, D), C.byref(nm), C.byref(nt))
    assert k >= 0
    return {"n_failed": nf_o, "n_succeeded": ns_o, "type": ty_o, "left_in_cell": left, "feat_cand": fc[:k], "feat_px": fpx[:k],
            "feat_level": fl[:k], "feat_type": ft[:k], "feat_grad": fg[:k], "n_matches": nm.value, "n_trials": nt.value}


# ---- the reference's own compiled vk::PinholeCamera members (ref_camera.cpp) ----
def _cam_d(cam):
    d = np.zeros(5)
    dist = getattr(cam, "dist", None)
    if dist is not None:
        d[:] = dist
    return d


def pinhole_world2cam(cam, xyz):
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    out = np.zeros((len(xyz), 2))
    d = _cam_d(cam)
    rc = lib().ref_pinhole_world2cam(*_cam_args(cam), _p(d, D), C.c_int(len(xyz)), _p(xyz, D), _p(out, D))
    assert rc == 0
    return out


def pinhole_world2cam_uv(cam, uv):
    uv = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2)
    out = np.zeros((len(uv), 2))
    d = _cam_d(cam)
    rc = lib().ref_pinhole_world2cam_uv(*_cam_args(cam), _p(d, D), C.c_int(len(uv)), _p(uv, D), _p(out, D))
    assert rc == 0
    return out


def pinhole_cam2world(cam, px):
    """distortion-free cameras only (the distorted branch calls cv::undistortPoints, absent here)"""
    px = np.ascontiguousarray(px, dtype=np.float64).reshape(-1, 2)
    out = np.zeros((len(px), 3))
    d = _cam_d(cam)
    rc = lib().ref_pinhole_cam2world(*_cam_args(cam), _p(d, D), C.c_int(len(px)), _p(px, D), _p(out, D))
    assert rc == 0
    return out


def camera_is_in_frame(width, height, obs, boundary, level):
    obs = np.ascontiguousarray(obs, dtype=np.int32).reshape(-1, 2)
    plain, lev = np.zeros(len(obs), dtype=np.uint8), np.zeros(len(obs), dtype=np.uint8)
    lib().ref_camera_is_in_frame(C.c_int(width), C.c_int(height), C.c_int(len(obs)), _p(obs, C.c_int), C.c_int(boundary),
                                 C.c_int(level), _p(plain, C.c_uint8), _p(lev, C.c_uint8))
    return plain, lev



# ---- the whole Reprojector::reprojectMap on a real svo::Map (ref_objects.cpp: ref_reproject_map) ----
def reproject_map(cs, max_fts=1200, n_pyr_levels=3, key_override=None, library=None, max_n_kfs=None):
    """cs: a case of android_svo_amd.synth.make_map_case.  library: another build of the same harness (the one linked with
    the PATCHED reprojector of include/svo_dropin/reprojector.patch: tests/test_gpu_dropin_binding.py).  Returns the reference's outputs, incl. the key points its own
    Frame::setKeyPoints chose for every keyframe (an input of the oracle / HIP forms of the call).
    key_override [n_kf][5] (-2: keep the reference's choice, -1: empty slot, else point index): the key features to start
    from; kf_key_point is then what the call started from and kf_key_point_after what Map::safeDeletePoint ->
    Frame::removeKeyPoint left behind.  max_n_kfs: Reprojector::Options::max_n_kfs for this call (None: the reference's 10)."""
    cam, n_kf, n_pts, n_obs = cs["cam"], cs["n_kf"], cs["n_points"], len(cs["obs_point"])
    if max_n_kfs is not None:
        (library or lib()).ref_set_reproj_max_n_kfs(C.c_int(int(max_n_kfs)))
        try:
            return reproject_map(cs, max_fts, n_pyr_levels, key_override, library)
        finally:
            (library or lib()).ref_set_reproj_max_n_kfs(C.c_int(0))
    kp = (C.POINTER(C.POINTER(C.c_uint8)) * n_kf)()
    keep = []
    for k in range(n_kf):
        pp = orc.pyr_ptrs(cs["kf_pyr"][k])
        keep.append(pp)
        kp[k] = C.cast(pp, C.POINTER(C.POINTER(C.c_uint8)))
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    u8 = lambda a: np.ascontiguousarray(a, dtype=np.uint8)
    I, U = C.c_int, C.c_uint8
    n_cells = (-(-cam.width // cs["cell_size"])) * (-(-cam.height // cs["cell_size"]))
    ins = dict(Tk=f64(cs["T_kf_w"]), Tc=f64(cs["T_cur_w"]), pos=f64(cs["pt_pos"]), ty=i32(cs["pt_type"]), nf=i32(cs["pt_n_failed"]),
               ns=i32(cs["pt_n_succeeded"]), op=i32(cs["obs_point"]), ok=i32(cs["obs_kf"]), opx=f64(cs["obs_px"]), of=f64(cs["obs_f"]),
               ol=i32(cs["obs_level"]), oe=u8(cs["obs_edgelet"]), og=f64(cs["obs_grad"]), ko=i32(cs["kf_ftr_offset"]), kb=i32(cs["kf_ftr_obs"]),
               cp=i32(cs["cand_point"]), co=i32(cs["cand_obs"]))
    key = np.zeros((n_kf, 5), np.int32)
    ty_o, nf_o, ns_o, un_o = np.zeros(n_pts, np.int32), np.zeros(n_pts, np.int32), np.zeros(n_pts, np.int32), np.zeros(n_pts, np.uint8)
    n_ov, ov_kf, ov_cnt = C.c_int(0), np.zeros(max(n_kf, 1), np.int32), np.zeros(max(n_kf, 1), np.int32)
    fp, fpx, fl, ft, fg = np.zeros(n_cells, np.int32), np.zeros((n_cells, 2)), np.zeros(n_cells, np.int32), np.zeros(n_cells, np.int32), np.zeros((n_cells, 2))
    nm, nt = C.c_size_t(0), C.c_size_t(0)
    ko = None if key_override is None else i32(key_override)
    key_after = np.zeros((n_kf, 5), np.int32)
    k = (library or lib()).ref_reproject_map_keys(*_cam_args(cam), I(len(cs["cur_pyr"])), I(cs["cell_size"]), I(max_fts), I(n_pyr_levels), I(n_kf), kp,
                                _p(ins["Tk"], D), orc.pyr_ptrs(cs["cur_pyr"]), _p(ins["Tc"], D), I(n_pts), _p(ins["pos"], D), _p(ins["ty"], I),
                                _p(ins["nf"], I), _p(ins["ns"], I), I(n_obs), _p(ins["op"], I), _p(ins["ok"], I), _p(ins["opx"], D),
                                _p(ins["of"], D), _p(ins["ol"], I), _p(ins["oe"], U), _p(ins["og"], D), _p(ins["ko"], I), _p(ins["kb"], I),
                                I(len(ins["cp"])), _p(ins["cp"], I), _p(ins["co"], I),
                                _p(key, I), _p(ty_o, I), _p(nf_o, I), _p(ns_o, I), _p(un_o, U), C.byref(n_ov), _p(ov_kf, I), _p(ov_cnt, I),
                                _p(fp, I), _p(fpx, D), _p(fl, I), _p(ft, I), _p(fg, D), C.byref(nm), C.byref(nt),
                                None if ko is None else _p(ko, I), _p(key_after, I))
    assert k >= 0
    if ko is not None:
        key = np.where(ko == -2, key, ko).astype(np.int32)
    return {"kf_key_point": key, "kf_key_point_after": key_after, "type": ty_o, "n_failed": nf_o, "n_succeeded": ns_o, "unlinked": un_o,
            "overlap_kf": ov_kf[:n_ov.value], "overlap_count": ov_cnt[:n_ov.value], "feat_point": fp[:k], "feat_px": fpx[:k],
            "feat_level": fl[:k], "feat_type": ft[:k], "feat_grad": fg[:k], "n_matches": nm.value, "n_trials": nt.value}
