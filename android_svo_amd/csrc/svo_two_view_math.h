// svo_two_view_math.h -- the arithmetic of the bootstrap's two-view stage (svo_two_view_impl.h), one function per stage of
// tests/two_view_reference.py and held to that model by bits.
//
//   computeFundamental          S/initialization.cpp:260-329  (cv::findFundamentalMat FM_RANSAC and cv::recoverPose restated;
//                                                              vk::computeInliers, Quaterniond(R))
//   addSecondFrame              S/initialization.cpp:85-138   (depth median, map scale, second pose, first points)
//   vk::triangulateFeatureNonLin, vk::reprojError            S/math_utils.cpp:15-64
//
// Every function is host-and-device (SVO_TV_FN, local to this header) so that a plain C++ program can run the same
// arithmetic on the CPU.  All of it is scalar f64 with every operation rounded on its own (-ffp-contract=off); no sum over
// correspondences is a floating-point sum.  Arrays that are indexed by data (the 8 x 9 system) are reached through a stride S:
// the kernels keep them in LDS element-major across the threads of a block, the host uses S = 1.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SVO_TV_FN __host__ __device__ __forceinline__
#else
#define SVO_TV_FN inline
#endif

namespace svo_tv {

constexpr int TV_MAX_HYPOTHESES = 4096;
constexpr int TV_SVD_SWEEPS = 12;
enum { TV_OK = 0, TV_TOO_FEW = 1, TV_NO_MODEL = 2, TV_CHEIRALITY = 3, TV_FEW_INLIERS = 4 };

struct TvPrm {
  double reproj_thresh, map_scale;
  int min_inliers, n_hypotheses;
  unsigned long long seed;
};

// ---- sampling: draw k of hypothesis h is a function of (seed, h, k, n) alone -- a 64-bit mix, its upper word scaled to the
// n - k positions still free, shifted past the earlier picks in ascending order.  s[8] comes back ascending; exactly 8 draws.
SVO_TV_FN uint64_t tv_mix(uint64_t seed, uint32_t h, uint32_t k) {
  uint64_t z = seed * 0x9E3779B97F4A7C15ull + (uint64_t)h * 0xBF58476D1CE4E5B9ull + (uint64_t)k * 0x94D049BB133111EBull;
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
SVO_TV_FN void tv_sample(uint64_t seed, int h, int n, int* s) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint64_t r = tv_mix(seed, (uint32_t)h, (uint32_t)k) >> 32;
    int v = (int)((r * (uint64_t)(n - k)) >> 32);
#pragma unroll
    for (int i = 0; i < k; ++i) v += v >= s[i] ? 1 : 0;
#pragma unroll
    for (int i = 0; i < k; ++i) {
      const int lo = v < s[i] ? v : s[i], hi = v < s[i] ? s[i] : v;
      s[i] = lo; v = hi;
    }
    s[k] = v;
  }
}

// vk::project2d rounded as cv::Point2f rounds it (:274-278)
SVO_TV_FN void tv_normalised(const double* f, float* xy) {
  xy[0] = (float)(f[0] / f[2]);
  xy[1] = (float)(f[1] / f[2]);
}

SVO_TV_FN bool tv_finite_pos(double v) { return v > 0.0 && v < INFINITY; }

// ---- one hypothesis: Hartley normalisation, the 8 x 9 epipolar system x_cur^T F x_ref = 0, its null vector by Gaussian
// elimination with complete pivoting (first maximum in row-major order), de-normalisation.  p[i] = {x_ref, y_ref, x_cur, y_cur}
// of the 8 sampled correspondences; A: 72 doubles at stride S; F row-major.  false: a degenerate sample.  F is not projected
// to rank 2 before scoring.
template <int S>
SVO_TV_FN bool tv_hypothesis(const float (*p)[4], double* A, double* F) {
  double c[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = c[j] + (double)p[i][j];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) c[j] = c[j] * 0.125;
  double d1 = 0.0, d2 = 0.0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const double ax = (double)p[i][0] - c[0], ay = (double)p[i][1] - c[1];
    const double bx = (double)p[i][2] - c[2], by = (double)p[i][3] - c[3];
    d1 = d1 + sqrt(ax * ax + ay * ay);
    d2 = d2 + sqrt(bx * bx + by * by);
  }
  d1 = d1 * 0.125; d2 = d2 * 0.125;
  if (!tv_finite_pos(d1) || !tv_finite_pos(d2)) return false;
  const double s1 = 1.4142135623730951 / d1, s2 = 1.4142135623730951 / d2;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const double u1 = ((double)p[i][0] - c[0]) * s1, v1 = ((double)p[i][1] - c[1]) * s1;
    const double u2 = ((double)p[i][2] - c[2]) * s2, v2 = ((double)p[i][3] - c[3]) * s2;
    double* r = A + (size_t)i * 9 * S;
    r[0 * S] = u2 * u1; r[1 * S] = u2 * v1; r[2 * S] = u2;
    r[3 * S] = v2 * u1; r[4 * S] = v2 * v1; r[5 * S] = v2;
    r[6 * S] = u1;      r[7 * S] = v1;      r[8 * S] = 1.0;
  }
  // perm: nibble j = the unknown that column j holds
  uint64_t perm = 0x876543210ull;
  for (int k = 0; k < 8; ++k) {
    double best = -1.0;
    int pr = k, pc = k;
    for (int r = k; r < 8; ++r)
      for (int cc = k; cc < 9; ++cc) {
        const double a = fabs(A[(r * 9 + cc) * S]);
        if (a > best) { best = a; pr = r; pc = cc; }
      }
    if (!tv_finite_pos(best)) return false;
    if (pr != k)
      for (int cc = k; cc < 9; ++cc) {
        const double t = A[(k * 9 + cc) * S];
        A[(k * 9 + cc) * S] = A[(pr * 9 + cc) * S];
        A[(pr * 9 + cc) * S] = t;
      }
    if (pc != k) {
      for (int r = 0; r < 8; ++r) {
        const double t = A[(r * 9 + k) * S];
        A[(r * 9 + k) * S] = A[(r * 9 + pc) * S];
        A[(r * 9 + pc) * S] = t;
      }
      const uint64_t a = (perm >> (4 * k)) & 15ull, b = (perm >> (4 * pc)) & 15ull;
      perm = (perm & ~((15ull << (4 * k)) | (15ull << (4 * pc)))) | (b << (4 * k)) | (a << (4 * pc));
    }
    const double piv = A[(k * 9 + k) * S];
    for (int r = k + 1; r < 8; ++r) {
      const double m = A[(r * 9 + k) * S] / piv;
      for (int cc = k + 1; cc < 9; ++cc) A[(r * 9 + cc) * S] = A[(r * 9 + cc) * S] - m * A[(k * 9 + cc) * S];
    }
  }
  // back-substitution with x[8] = 1; x[k] takes the pivot's place
  for (int k = 7; k >= 0; --k) {
    double s = A[(k * 9 + 8) * S];
    for (int j = 7; j > k; --j) s = s + A[(k * 9 + j) * S] * A[(j * 9 + j) * S];
    A[(k * 9 + k) * S] = -s / A[(k * 9 + k) * S];
  }
  uint64_t inv = 0;
  for (int j = 0; j < 9; ++j) inv |= (uint64_t)j << (4 * ((perm >> (4 * j)) & 15ull));
  double g[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const int j = (int)((inv >> (4 * i)) & 15ull);
    g[i] = j == 8 ? 1.0 : A[((j & 7) * 10) * S];
  }
  // F = T2^T G T1,  T = [s 0 -s cx; 0 s -s cy; 0 0 1]
  const double t1x = s1 * c[0], t1y = s1 * c[1], t2x = s2 * c[2], t2y = s2 * c[3];
  double m[9];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    m[3 * r] = g[3 * r] * s1;
    m[3 * r + 1] = g[3 * r + 1] * s1;
    m[3 * r + 2] = (g[3 * r + 2] - g[3 * r] * t1x) - g[3 * r + 1] * t1y;
  }
#pragma unroll
  for (int cc = 0; cc < 3; ++cc) {
    F[cc] = s2 * m[cc];
    F[3 + cc] = s2 * m[3 + cc];
    F[6 + cc] = (m[6 + cc] - t2x * m[cc]) - t2y * m[3 + cc];
  }
  return true;
}

// ---- cv::findFundamentalMat's FM_RANSAC error: the larger of the two squared point-to-epipolar-line distances against thr2;
// a NaN is no inlier
SVO_TV_FN bool tv_epi_inlier(const double* F, float xr, float yr, float xc, float yc, double thr2) {
  const double x1 = (double)xr, y1 = (double)yr, x2 = (double)xc, y2 = (double)yc;
  const double a = (F[0] * x1 + F[1] * y1) + F[2], b = (F[3] * x1 + F[4] * y1) + F[5], c = (F[6] * x1 + F[7] * y1) + F[8];
  const double d2 = (x2 * a + y2 * b) + c;
  const double e2 = (d2 * d2) * (1.0 / (a * a + b * b));
  const double a1 = (F[0] * x2 + F[3] * y2) + F[6], b1 = (F[1] * x2 + F[4] * y2) + F[7], c1 = (F[2] * x2 + F[5] * y2) + F[8];
  const double d1 = (x1 * a1 + y1 * b1) + c1;
  const double e1 = (d1 * d1) * (1.0 / (a1 * a1 + b1 * b1));
  return e1 <= thr2 && e2 <= thr2;
}
SVO_TV_FN double tv_thr2(double reproj_thresh, double error_multiplier2) {
  const double t = reproj_thresh / error_multiplier2;
  return t * t;
}

// The orders of Eigen's compiled code, found against tests/golden/two_view_ref.npz.  Vector3d::dot: a packet of two, then the
// third term -- (a0 + a1) + a2.  Matrix3d * Vector3d: rows 0 and 1 as one packet over the columns, (c0 v0 + c1 v1) + c2 v2; row 2
// is the scalar unroller's a0 + (a1 + a2).  R.transpose() * v: no packets, the scalar unroller in every row.
SVO_TV_FN double tv_dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
SVO_TV_FN void tv_matvec(const double* R, const double* v, double* o) {
  const double x = tv_dot3(R, v), y = tv_dot3(R + 3, v), z = R[6] * v[0] + (R[7] * v[1] + R[8] * v[2]);
  o[0] = x; o[1] = y; o[2] = z;
}
SVO_TV_FN void tv_matTvec(const double* R, const double* v, double* o) {
  const double x = R[0] * v[0] + (R[3] * v[1] + R[6] * v[2]);
  const double y = R[1] * v[0] + (R[4] * v[1] + R[7] * v[2]);
  const double z = R[2] * v[0] + (R[5] * v[1] + R[8] * v[2]);
  o[0] = x; o[1] = y; o[2] = z;
}
SVO_TV_FN void tv_cross(const double* a, const double* b, double* o) {
  const double x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
  o[0] = x; o[1] = y; o[2] = z;
}

// ---- cv::recoverPose's decomposition: one-sided Jacobi SVD of F (TV_SVD_SWEEPS sweeps over the column pairs (0,1), (0,2),
// (1,2)), the two largest singular directions, u3 = u1 x u2 and v3 = v1 x v2 (both factors get determinant +1; the smallest
// singular value is dropped, which is the projection to rank 2), then R1 = U W V^T, R2 = U W^T V^T, t = u3.
// w, v: 9 doubles of work space each (column j at [3 j]).
SVO_TV_FN void tv_jacobi_pair(double* wp, double* wq, double* vp, double* vq) {
  const double alpha = tv_dot3(wp, wp), beta = tv_dot3(wq, wq), gamma = tv_dot3(wp, wq);
  if (!(gamma != 0.0)) return;
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double root = sqrt(1.0 + zeta * zeta);
  const double t = zeta >= 0.0 ? 1.0 / (zeta + root) : -1.0 / (root - zeta);
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
  for (int i = 0; i < 3; ++i) {
    const double a = wp[i], b = wq[i];
    wp[i] = c * a - s * b; wq[i] = s * a + c * b;
    const double e = vp[i], f = vq[i];
    vp[i] = c * e - s * f; vq[i] = s * e + c * f;
  }
}
SVO_TV_FN void tv_swap_cols(double* w, double* v, double* sg, int a, int b) {
  if (sg[b] > sg[a]) {
    for (int i = 0; i < 3; ++i) {
      double t = w[3 * a + i]; w[3 * a + i] = w[3 * b + i]; w[3 * b + i] = t;
      t = v[3 * a + i]; v[3 * a + i] = v[3 * b + i]; v[3 * b + i] = t;
    }
    const double t = sg[a]; sg[a] = sg[b]; sg[b] = t;
  }
}
SVO_TV_FN void tv_decompose(const double* F, double* w, double* v, double* R1, double* R2, double* u3) {
  for (int j = 0; j < 3; ++j)
    for (int i = 0; i < 3; ++i) { w[3 * j + i] = F[3 * i + j]; v[3 * j + i] = i == j ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < TV_SVD_SWEEPS; ++sweep) {
    tv_jacobi_pair(w, w + 3, v, v + 3);
    tv_jacobi_pair(w, w + 6, v, v + 6);
    tv_jacobi_pair(w + 3, w + 6, v + 3, v + 6);
  }
  double sg[3];
  for (int j = 0; j < 3; ++j) sg[j] = sqrt(tv_dot3(w + 3 * j, w + 3 * j));
  tv_swap_cols(w, v, sg, 0, 1);
  tv_swap_cols(w, v, sg, 0, 2);
  tv_swap_cols(w, v, sg, 1, 2);
  for (int j = 0; j < 2; ++j)
    for (int i = 0; i < 3; ++i) w[3 * j + i] = w[3 * j + i] / sg[j];
  tv_cross(w, w + 3, w + 6);
  tv_cross(v, v + 3, v + 6);
  for (int i = 0; i < 3; ++i) {
    u3[i] = w[6 + i];
    for (int j = 0; j < 3; ++j) {
      R1[3 * i + j] = (w[3 + i] * v[j] - w[i] * v[3 + j]) + w[6 + i] * v[6 + j];
      R2[3 * i + j] = (w[i] * v[3 + j] - w[3 + i] * v[j]) + w[6 + i] * v[6 + j];
    }
  }
}
// candidate c of (R1, +u3), (R1, -u3), (R2, +u3), (R2, -u3)
SVO_TV_FN void tv_candidate(int c, const double* R1, const double* R2, const double* u3, double* R, double* t) {
  for (int i = 0; i < 9; ++i) R[i] = c < 2 ? R1[i] : R2[i];
  for (int i = 0; i < 3; ++i) t[i] = (c & 1) ? -u3[i] : u3[i];
}

// ---- vk::triangulateFeatureNonLin(R, t, feature1 = f_cur, feature2 = f_ref) (S/math_utils.cpp:15-32): the two ray parameters
// and the point in the current frame.  A.inverse() is Eigen's 2 x 2 formula.
SVO_TV_FN void tv_triangulate(const double* R, const double* t, const double* f1, const double* f_ref, double* lambda, double* xyz) {
  double f2[3];
  tv_matvec(R, f_ref, f2);
  const double b0 = tv_dot3(t, f1), b1 = tv_dot3(t, f2);
  const double a00 = tv_dot3(f1, f1), a10 = tv_dot3(f1, f2), a01 = -a10, a11 = -tv_dot3(f2, f2);
  const double invdet = 1.0 / (a00 * a11 - a10 * a01);
  const double i00 = a11 * invdet, i10 = -a10 * invdet, i01 = -a01 * invdet, i11 = a00 * invdet;
  lambda[0] = i00 * b0 + i01 * b1;
  lambda[1] = i10 * b0 + i11 * b1;
  for (int i = 0; i < 3; ++i) xyz[i] = (lambda[0] * f1[i] + (t[i] + lambda[1] * f2[i])) / 2.0;
}
// vk::reprojError (S/math_utils.cpp:57-64)
SVO_TV_FN double tv_reproj_error(const double* f1, const double* f2, double error_multiplier2) {
  const double ex = f1[0] / f1[2] - f2[0] / f2[2], ey = f1[1] / f1[2] - f2[1] / f2[2];
  return error_multiplier2 * sqrt(ex * ex + ey * ey);
}
// one correspondence of vk::computeInliers (S/math_utils.cpp:66-96); !(e1 > thresh || e2 > thresh): a NaN error is an inlier
SVO_TV_FN bool tv_compute_inlier(const double* R, const double* t, const double* f_cur, const double* f_ref, double reproj_thresh,
                                 double error_multiplier2, double* xyz) {
  double lambda[2], d[3], q[3];
  tv_triangulate(R, t, f_cur, f_ref, lambda, xyz);
  const double e1 = tv_reproj_error(f_cur, xyz, error_multiplier2);
  for (int i = 0; i < 3; ++i) d[i] = xyz[i] - t[i];
  tv_matTvec(R, d, q);
  const double e2 = tv_reproj_error(f_ref, q, error_multiplier2);
  return !(e1 > reproj_thresh || e2 > reproj_thresh);
}

// ---- Eigen's Quaterniond(R) (Quaternion.h, quaternionbase_assign_impl<Other, 3, 3>); q = {x, y, z, w}
SVO_TV_FN void tv_quaternion(const double* R, double* q) {
  double t = R[0] + (R[4] + R[8]);
  if (t > 0.0) {
    t = sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (R[7] - R[5]) * t; q[1] = (R[2] - R[6]) * t; q[2] = (R[3] - R[1]) * t;
  } else {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[4 * i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0);
    q[i] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (R[3 * k + j] - R[3 * j + k]) * t;
    q[j] = (R[3 * j + i] + R[3 * i + j]) * t;
    q[k] = (R[3 * k + i] + R[3 * i + k]) * t;
  }
}

// ---- SE3 arithmetic on T = {tx, ty, tz, qx, qy, qz, qw}, in the operation order of svo_device_math.h
SVO_TV_FN void tv_so3_rotate(const double* q, const double* p, double* o) {
  double uv[3], quv[3];
  tv_cross(q, p, uv);
  uv[0] = uv[0] + uv[0]; uv[1] = uv[1] + uv[1]; uv[2] = uv[2] + uv[2];
  tv_cross(q, uv, quv);
  const double x = (p[0] + q[3] * uv[0]) + quv[0], y = (p[1] + q[3] * uv[1]) + quv[1], z = (p[2] + q[3] * uv[2]) + quv[2];
  o[0] = x; o[1] = y; o[2] = z;
}
SVO_TV_FN void tv_se3_mul(const double* A, const double* B, double* out) {
  const double* a = A + 3;
  const double* b = B + 3;
  const double x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  const double y = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  const double z = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
  const double w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
  double rt[3];
  tv_so3_rotate(a, B, rt);
  out[0] = A[0] + rt[0]; out[1] = A[1] + rt[1]; out[2] = A[2] + rt[2];
  out[3] = x; out[4] = y; out[5] = z; out[6] = w;
}
SVO_TV_FN void tv_se3_inverse(const double* T, double* out) {
  const double qi[4] = {-T[3], -T[4], -T[5], T[6]};
  double rt[3];
  tv_so3_rotate(qi, T, rt);
  out[0] = -rt[0]; out[1] = -rt[1]; out[2] = -rt[2];
  out[3] = qi[0]; out[4] = qi[1]; out[5] = qi[2]; out[6] = qi[3];
}
// row-major 3 x 3 of the rotation (I/SO3.h:391-406, se3_rotation_matrix)
SVO_TV_FN void tv_rotation_matrix(const double* T, double* m) {
  const double x = T[3], y = T[4], z = T[5], w = T[6];
  const double x2 = x * x, y2 = y * y, z2 = z * z;
  const double xy = x * y, xz = x * z, yz = y * z;
  const double wx = w * x, wy = w * y, wz = w * z;
  m[0] = 1.0 - 2.0 * (y2 + z2); m[1] = 2.0 * (xy - wz);       m[2] = 2.0 * (xz + wy);
  m[3] = 2.0 * (xy + wz);       m[4] = 1.0 - 2.0 * (x2 + z2); m[5] = 2.0 * (yz - wx);
  m[6] = 2.0 * (xz - wy);       m[7] = 2.0 * (yz + wx);       m[8] = 1.0 - 2.0 * (x2 + y2);
}
SVO_TV_FN void tv_se3_act(const double* T, const double* p, double* out) {
  double r[3];
  tv_so3_rotate(T + 3, p, r);
  out[0] = T[0] + r[0]; out[1] = T[1] + r[1]; out[2] = T[2] + r[2];
}

// ---- the second frame's pose (:105-118): scale = map_scale / median, T_cur_w = T_cur_from_ref * T_ref_w with the
// translation -R_cur_w (ref_pos + scale (cur_pos - ref_pos)), and T_world_cur for the points
SVO_TV_FN void tv_second_pose(const double* T_cur_from_ref, const double* T_ref_w, double scale, double* T_cur_w, double* T_world_cur) {
  double Ti[7], ref_pos[3], cur_pos[3], p[3], r[3], m[9];
  tv_se3_mul(T_cur_from_ref, T_ref_w, T_cur_w);
  tv_se3_inverse(T_ref_w, Ti);
  for (int i = 0; i < 3; ++i) ref_pos[i] = Ti[i];
  tv_se3_inverse(T_cur_w, Ti);
  for (int i = 0; i < 3; ++i) cur_pos[i] = Ti[i];
  for (int i = 0; i < 3; ++i) p[i] = ref_pos[i] + scale * (cur_pos[i] - ref_pos[i]);
  tv_rotation_matrix(T_cur_w, m);                           // -T_f_w_.rotation_matrix() * (...): an Eigen matrix-vector product
  tv_matvec(m, p, r);
  for (int i = 0; i < 3; ++i) T_cur_w[i] = -r[i];
  tv_se3_inverse(T_cur_w, T_world_cur);
}

// isInFrame(px.cast<int>(), 10) on both pixels and z > 0 (:123); the cast truncates toward zero
SVO_TV_FN bool tv_in_frame(float x, float y, int width, int height) {
  const int ix = (int)(double)x, iy = (int)(double)y;
  return ix >= 10 && ix < width - 10 && iy >= 10 && iy < height - 10;
}

// keys that order doubles as numbers; a NaN's key lies above every number's (positive NaN) -- svo_track_frame_end.h's rule
SVO_TV_FN unsigned long long tv_depth_key(double z) {
  unsigned long long u;
  __builtin_memcpy(&u, &z, 8);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
SVO_TV_FN double tv_depth_from_key(unsigned long long k) {
  const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double z;
  __builtin_memcpy(&z, &u, 8);
  return z;
}

}  // namespace svo_tv
