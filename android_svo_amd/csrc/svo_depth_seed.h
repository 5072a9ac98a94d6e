// svo_depth_seed.h -- the arithmetic of one seed (updateSeed, computeTau, triangulation, the geometry and finalize bodies of
// DepthFilter::updateSeeds) and the thread-per-item kernels around it, findMatchDirect's and the camera batch included.
#pragma once
#include "svo_depth_types.h"
namespace {
// ---- DepthFilter::updateSeed (S/depth_filter.cpp:359-391) -------------------------------------
SVO_DEV double normal_pdf_quirk(double x, double mean, double std_dev) {
  const double SQRT_2_PI = 1.41421356237309505;       // sqrt(2), as in the reference (:360)
  const double q = (x - mean) / std_dev;
  const double exponent = -0.5 * (q * q);              // pow(q, 2)
  return (1 / (std_dev * SQRT_2_PI)) * exp(exponent);
}

SVO_DEV void update_seed(const float x, const float tau2, SeedState* seed) {
  const float norm_scale = sqrtf(seed->sigma2 + tau2);
  if (norm_scale != norm_scale) return;
  const float s2 = (float)(1. / (1. / seed->sigma2 + 1. / tau2));
  const float m = s2 * (seed->mu / seed->sigma2 + x / tau2);
  float C1 = (float)(seed->a / (seed->a + seed->b) * normal_pdf_quirk(x, seed->mu, norm_scale));
  float C2 = (float)(seed->b / (seed->a + seed->b) * 1. / seed->z_range);
  const float normalization_constant = C1 + C2;
  C1 /= normalization_constant;
  C2 /= normalization_constant;
  const float f = (float)(C1 * (seed->a + 1.) / (seed->a + seed->b + 1.) + C2 * seed->a / (seed->a + seed->b + 1.));
  const float e = (float)(C1 * (seed->a + 1.) * (seed->a + 2.) / ((seed->a + seed->b + 1.) * (seed->a + seed->b + 2.)) +
                          C2 * seed->a * (seed->a + 1.0f) / ((seed->a + seed->b + 1.0f) * (seed->a + seed->b + 2.0f)));
  const float mu_new = C1 * m + C2 * seed->mu;
  seed->sigma2 = C1 * (s2 + m * m) + C2 * (seed->sigma2 + seed->mu * seed->mu) - mu_new * mu_new;
  seed->mu = mu_new;
  seed->a = (e - f) / (f - e / f);
  seed->b = seed->a * (1.0f - f) / f;
}

// 44 B/seed of HBM traffic (20 B state + 8 B measurement read, 16 B written): purely HBM-bound
__global__ void update_seed_kernel(int n, const float* __restrict__ x, const float* __restrict__ tau2,
                                   float* __restrict__ a, float* __restrict__ b, float* __restrict__ mu,
                                   const float* __restrict__ z_range, float* __restrict__ sigma2) {
  const int stride = gridDim.x * blockDim.x;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    SeedState s = {a[i], b[i], mu[i], z_range[i], sigma2[i]};
    update_seed(x[i], tau2[i], &s);
    a[i] = s.a; b[i] = s.b; mu[i] = s.mu; sigma2[i] = s.sigma2;
  }
}

// S/depth_filter.cpp:396-416; PI = 3.14159265 (I/global.h:92)
SVO_DEV double compute_tau(const double* t, const double* f, double z, double px_error_angle) {
  const double PI_SVO = 3.14159265;
  const double a[3] = {f[0] * z - t[0], f[1] * z - t[1], f[2] * z - t[2]};
  const double t_norm = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
  const double a_norm = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
  const double alpha = acos(((f[0] * t[0] + f[1] * t[1]) + f[2] * t[2]) / t_norm);
  const double beta = acos(((a[0] * -t[0] + a[1] * -t[1]) + a[2] * -t[2]) / (t_norm * a_norm));
  const double beta_plus = beta + px_error_angle;
  const double gamma_plus = PI_SVO - alpha - beta_plus;
  const double z_plus = t_norm * sin(beta_plus) / sin(gamma_plus);
  return z_plus - z;
}

__global__ void compute_tau_kernel(int n, Vec3 t, const double* __restrict__ f, const double* __restrict__ z,
                                   double px_error_angle, double* __restrict__ tau) {
  const int stride = gridDim.x * blockDim.x;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double fi[3] = {f[3 * (size_t)i], f[3 * (size_t)i + 1], f[3 * (size_t)i + 2]};
    tau[i] = compute_tau(t.v, fi, z[i], px_error_angle);
  }
}

// ---- the camera model exactly as every kernel evaluates it, over a batch (parity tests against the reference's
// ---- compiled vk::PinholeCamera, tests/golden/camera_ref.npz) -------------------------------------------------
__global__ void camera_batch_kernel(Cam cam, int n, const double* __restrict__ xyz, const double* __restrict__ uv,
                                    const double* __restrict__ px, const int32_t* __restrict__ obs, int boundary, int level,
                                    double* __restrict__ px_of_xyz, double* __restrict__ px_of_uv,
                                    double* __restrict__ f_of_px, uint8_t* __restrict__ in_frame) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (xyz && px_of_xyz) {
    const double p[3] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
    world2cam(cam, p, px_of_xyz + 2 * (size_t)i);
  }
  if (uv && px_of_uv) world2cam_uv(cam, uv[2 * (size_t)i], uv[2 * (size_t)i + 1], px_of_uv + 2 * (size_t)i);
  if (px && f_of_px) cam2world(cam, px[2 * (size_t)i], px[2 * (size_t)i + 1], f_of_px + 3 * (size_t)i);
  if (obs && in_frame) {
    const int ox = obs[2 * (size_t)i], oy = obs[2 * (size_t)i + 1];
    in_frame[i] = level < 0 ? (ox >= boundary && ox < cam.width - boundary && oy >= boundary && oy < cam.height - boundary)
                            : is_in_frame_level(cam, ox, oy, boundary, level);
  }
}

// ---- matcher pieces ---------------------------------------------------------------------------
// (get_warp_matrix_affine: svo_device_math.h)

// S/matcher.cpp:123-136
SVO_DEV bool depth_from_triangulation(const double* T_search_ref, const double* f_ref, const double* f_cur,
                                      double* depth) {
  double R[9];
  const double t[3] = {T_search_ref[0], T_search_ref[1], T_search_ref[2]};
  se3_rotation_matrix(T_search_ref, R);
  double a0[3];
  const double a1[3] = {f_cur[0], f_cur[1], f_cur[2]};
  for (int i = 0; i < 3; ++i) a0[i] = (R[3 * i] * f_ref[0] + R[3 * i + 1] * f_ref[1]) + R[3 * i + 2] * f_ref[2];
  const double m00 = (a0[0] * a0[0] + a0[1] * a0[1]) + a0[2] * a0[2];
  const double m01 = (a0[0] * a1[0] + a0[1] * a1[1]) + a0[2] * a1[2];
  const double m11 = (a1[0] * a1[0] + a1[1] * a1[1]) + a1[2] * a1[2];
  const double det = m00 * m11 - m01 * m01;
  if (det < 0.000001) return false;
  const double invdet = 1.0 / det;
  const double n00 = -(m11 * invdet), n01 = -(-m01 * invdet);
  double r0[3];
  for (int k = 0; k < 3; ++k) r0[k] = n00 * a0[k] + n01 * a1[k];
  *depth = fabs((r0[0] * t[0] + r0[1] * t[1]) + r0[2] * t[2]);
  return true;
}

// ---- DepthFilter::updateSeeds as three stages -------------------------------------------------
// G  thread per seed : visibility, epipolar segment, affine warp, search level, search plan  -> SeedRec
// S  wave per seed   : warp the 10x10 patch (LDS), ZMSSD search along the epipolar line, align2D -> SeedRec
// F  thread per seed : triangulation, computeTau, updateSeed, convergence                     -> seed arrays
// The fp64 geometry of a seed runs once (64 seeds per wave instruction) instead of on every lane of
// the seed's wave; only the pixel work is wave-per-seed.
// (SeedRec: svo_match_device.h)

// EXPLICIT_DEPTH = false: the per-seed body of DepthFilter::updateSeeds (visibility test, depth interval from mu/sigma2);
// EXPLICIT_DEPTH = true: Matcher::findEpipolarMatchDirect as a caller would use it directly, with d_estimate / d_min /
// d_max given per item (dep[3][n]) and no visibility test.
// (the per-seed body; `rec_out` = where this seed's record goes, `ref_slot` = its reference keyframe's pyramid slot for
// the search stage when one pass covers several keyframes -- 0 otherwise)
template <bool EXPLICIT_DEPTH>
SVO_DEV void df_geometry_seed(const Cam& cam, const double* T_cur_ref_vis, const double* T_cur_ref_, int n_pyr_levels,
                              int max_epi_search_steps, int ref_slot, int i, int n, const double* __restrict__ px,
                              const double* __restrict__ f, const int32_t* __restrict__ level, const float* __restrict__ smu,
                              const float* __restrict__ ssigma2, const double* __restrict__ dep, double* __restrict__ epi_len_out,
                              SeedRec* __restrict__ rec_out, const uint8_t* __restrict__ alive) {
  SeedRec rc;
  rc.uv0[0] = rc.uv0[1] = rc.step[0] = rc.step[1] = 0.0;
  rc.a00 = rc.a01 = rc.a10 = rc.a11 = rc.prx = rc.pry = 0.0f;
  rc.n_steps = 0; rc.search_level = 0; rc.path = -1; rc.status = SVO_HIP_SEED_NO_MATCH; rc.warp_nan = 0;
  rc.matched = 0; rc.n_zmssd = 0; rc.n_align = 0; rc.pad = ref_slot;
  const double fi[3] = {f[3 * (size_t)i], f[3 * (size_t)i + 1], f[3 * (size_t)i + 2]};
  const double px_ref[2] = {px[2 * (size_t)i], px[2 * (size_t)i + 1]};
  const int level_ref = level[i];
  bool live = true;
  if (alive && !alive[i]) { rc.status = SVO_HIP_SEED_ERASED; live = false; }     // erased from the list (seed batches)
  double d_estimate, d_min, d_max;
  if (EXPLICIT_DEPTH) {
    d_estimate = dep[i]; d_min = dep[(size_t)n + i]; d_max = dep[2 * (size_t)n + i];
    rc.z_inv_min = 0.0f;
  } else {
    const float mu = smu[i], sigma2 = ssigma2[i];
    // ---- visibility in the current frame (depth_filter.cpp:264-275)
    const double inv_mu = 1.0 / mu;
    const double pf[3] = {inv_mu * fi[0], inv_mu * fi[1], inv_mu * fi[2]};
    double xyz_f[3];
    se3_act(T_cur_ref_vis, pf, xyz_f);
    if (live && xyz_f[2] < 0.0) { rc.status = SVO_HIP_SEED_BEHIND; live = false; }
    if (live) {
      double pc[2];
      world2cam(cam, xyz_f, pc);
      const int ox = (int)pc[0], oy = (int)pc[1];
      // A seed whose mu is NaN projects to NaN.  cast<int>() of a NaN is INT_MIN in the x86-64 build the oracle follows
      // (not in frame, the seed is left alone) but 0 on the device (pixel (0,0): in frame, searched, b += 1): spelled out.
      const bool nan_px = pc[0] != pc[0] || pc[1] != pc[1];
      if (nan_px || !(ox >= 0 && ox < cam.width && oy >= 0 && oy < cam.height)) { rc.status = SVO_HIP_SEED_NOT_IN_FRAME; live = false; }
    }
    const float z_inv_min = mu + sqrtf(sigma2);
    rc.z_inv_min = z_inv_min;
    const float z_inv_lo = mu - sqrtf(sigma2);
    const float z_inv_max = (z_inv_lo < 0.00000001f) ? 0.00000001f : z_inv_lo;
    d_estimate = 1.0 / mu; d_min = 1.0 / z_inv_min; d_max = 1.0 / z_inv_max;
  }
  if (live) {
    // ---- Matcher::findEpipolarMatchDirect up to the search plan (matcher.cpp:216-296)
    const double* T_cur_ref = T_cur_ref_;
    double pa[3], pb[3], tmp[3];
    tmp[0] = fi[0] * d_min; tmp[1] = fi[1] * d_min; tmp[2] = fi[2] * d_min;
    se3_act(T_cur_ref, tmp, pa);
    tmp[0] = fi[0] * d_max; tmp[1] = fi[1] * d_max; tmp[2] = fi[2] * d_max;
    se3_act(T_cur_ref, tmp, pb);
    const double Aep[2] = {pa[0] / pa[2], pa[1] / pa[2]};
    const double Bep[2] = {pb[0] / pb[2], pb[1] / pb[2]};
    const double epi_dir[2] = {Aep[0] - Bep[0], Aep[1] - Bep[1]};
    double Acr[4];
    get_warp_matrix_affine(cam, px_ref, fi, d_estimate, T_cur_ref, level_ref, Acr);
    int search_level = 0;
    {
      double D = Acr[0] * Acr[3] - Acr[2] * Acr[1];
      while (D > 3.0 && search_level < n_pyr_levels - 1) { search_level += 1; D *= 0.25; }
    }
    rc.search_level = search_level;
    double px_A[2], px_B[2];
    world2cam_uv(cam, Aep[0], Aep[1], px_A);
    world2cam_uv(cam, Bep[0], Bep[1], px_B);
    double epi_length;
    {
      const double ex = px_A[0] - px_B[0], ey = px_A[1] - px_B[1];
      epi_length = sqrt(ex * ex + ey * ey) / (1 << search_level);
    }
    {
      // warp::warpAffine prologue (matcher.cpp:92-102)
      const double det = Acr[0] * Acr[3] - Acr[2] * Acr[1];
      const double invdet = 1.0 / det;
      rc.a00 = (float)(Acr[3] * invdet); rc.a01 = (float)(-Acr[1] * invdet);
      rc.a10 = (float)(-Acr[2] * invdet); rc.a11 = (float)(Acr[0] * invdet);
      rc.warp_nan = rc.a00 != rc.a00;
      rc.prx = (float)px_ref[0] / (1 << level_ref);
      rc.pry = (float)px_ref[1] / (1 << level_ref);
    }
    if (epi_len_out) epi_len_out[i] = epi_length;
    if (epi_length < 2.0) {
      rc.path = 0;
      rc.uv0[0] = (px_A[0] + px_B[0]) / 2.0;
      rc.uv0[1] = (px_A[1] + px_B[1]) / 2.0;
    } else {
      const size_t n_steps = (size_t)(epi_length / 0.7);
      if (n_steps > (size_t)max_epi_search_steps) {
        rc.path = 2;
      } else {
        rc.path = 1;
        rc.n_steps = (int)n_steps;
        rc.step[0] = epi_dir[0] / n_steps; rc.step[1] = epi_dir[1] / n_steps;
        rc.uv0[0] = Bep[0] - rc.step[0]; rc.uv0[1] = Bep[1] - rc.step[1];
      }
    }
  }
  *rec_out = rc;
}

template <bool EXPLICIT_DEPTH>
__global__ __launch_bounds__(256) void df_geometry_kernel(
    DfFrame fr, int n, const double* __restrict__ px, const double* __restrict__ f, const int32_t* __restrict__ level,
    const float* __restrict__ smu, const float* __restrict__ ssigma2, const double* __restrict__ dep,
    double* __restrict__ epi_len_out, SeedRec* __restrict__ recs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  df_geometry_seed<EXPLICIT_DEPTH>(fr.cam, fr.T.T_cur_ref_vis, fr.T.T_cur_ref, fr.n_pyr_levels, fr.max_epi_search_steps, 0, i, n, px, f,
                                   level, smu, ssigma2, dep, epi_len_out, recs + i, nullptr);
}

// (the per-seed body of the finalize stage: seed i of the arrays, its record `rc`; returns the seed's status)
SVO_DEV int df_finalize_seed(const Cam& cam, const double* T_cur_ref, const double* T_ref_cur, const double* T_ref_inv,
                             double px_error_angle, double conv_thresh, int i, const SeedRec& rc, const double* __restrict__ f,
                             float* __restrict__ sa, float* __restrict__ sb, float* __restrict__ smu,
                             const float* __restrict__ sz_range, float* __restrict__ ssigma2, int32_t* __restrict__ status,
                             double* __restrict__ z_out, double* __restrict__ xyz_world, int32_t* __restrict__ n_zmssd_out,
                             int32_t* __restrict__ n_align_out, double* __restrict__ px_cur_out,
                             int32_t* __restrict__ search_level_out) {
  int st = rc.status;
  {
    double z = 0.0;
    if (rc.path >= 0) {
      const double fi[3] = {f[3 * (size_t)i], f[3 * (size_t)i + 1], f[3 * (size_t)i + 2]};
      SeedState seed = {sa[i], sb[i], smu[i], sz_range[i], ssigma2[i]};
      bool matched = false;
      if (rc.matched) {
        double fc[3];
        cam2world(cam, rc.step[0], rc.step[1], fc);
        matched = depth_from_triangulation(T_cur_ref, fi, fc, &z);
      }
      if (!matched) {
        seed.b += 1.0f;                                   // depth_filter.cpp:286
        st = SVO_HIP_SEED_NO_MATCH;
        z = 0.0;
      } else {
        // ---- computeTau + updateSeed + convergence (depth_filter.cpp:294-337)
        const double tau = compute_tau(T_ref_cur, fi, z, px_error_angle);
        const double zmt = z - tau;
        const double tau_inverse = 0.5 * (1.0 / (0.0000001 < zmt ? zmt : 0.0000001) - 1.0 / (z + tau));
        update_seed((float)(1. / z), (float)(tau_inverse * tau_inverse), &seed);
        if ((double)sqrtf(seed.sigma2) < seed.z_range / conv_thresh) {
          st = SVO_HIP_SEED_CONVERGED;
          if (xyz_world) {
            const double im = 1.0 / seed.mu;
            const double pfw[3] = {fi[0] * im, fi[1] * im, fi[2] * im};
            double xw[3];
            se3_act(T_ref_inv, pfw, xw);
            xyz_world[3 * (size_t)i] = xw[0]; xyz_world[3 * (size_t)i + 1] = xw[1]; xyz_world[3 * (size_t)i + 2] = xw[2];
          }
        } else if (rc.z_inv_min != rc.z_inv_min) {
          st = SVO_HIP_SEED_NAN;
        } else {
          st = SVO_HIP_SEED_UPDATED;
        }
      }
      sa[i] = seed.a; sb[i] = seed.b; smu[i] = seed.mu; ssigma2[i] = seed.sigma2;
    }
    status[i] = st;
    if (z_out) z_out[i] = z;
    if (n_zmssd_out) n_zmssd_out[i] = rc.n_zmssd;
    if (n_align_out) n_align_out[i] = rc.n_align;
    // Matcher::px_cur_ / search_level_ of this seed's findEpipolarMatchDirect call (matcher.cpp:345-346): what
    // DepthFilter::updateSeeds hands to feature_detector_->setGridOccpuancy on keyframes (depth_filter.cpp:302-306)
    if (px_cur_out) {
      const bool updated = st >= SVO_HIP_SEED_UPDATED;
      const double qnan = __longlong_as_double(0x7ff8000000000000ll);
      px_cur_out[2 * (size_t)i] = updated ? rc.step[0] : qnan;
      px_cur_out[2 * (size_t)i + 1] = updated ? rc.step[1] : qnan;
    }
    if (search_level_out) search_level_out[i] = rc.path >= 0 ? rc.search_level : -1;
  }
  return st;
}

__global__ __launch_bounds__(256) void df_finalize_kernel(
    DfFrame fr, int n, const double* __restrict__ f, const SeedRec* __restrict__ recs, float* __restrict__ sa,
    float* __restrict__ sb, float* __restrict__ smu, const float* __restrict__ sz_range, float* __restrict__ ssigma2,
    int32_t* __restrict__ status, double* __restrict__ z_out, double* __restrict__ xyz_world,
    int32_t* __restrict__ n_zmssd_out, int32_t* __restrict__ n_align_out, double* __restrict__ px_cur_out,
    int32_t* __restrict__ search_level_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const SeedRec rc = recs[i];                              // (a copy: the whole record is asked for at once)
  (void)df_finalize_seed(fr.cam, fr.T.T_cur_ref, fr.T.T_ref_cur, fr.T.T_ref_inv, fr.px_error_angle, fr.conv_thresh, i, rc, f, sa, sb,
                         smu, sz_range, ssigma2, status, z_out, xyz_world, n_zmssd_out, n_align_out, px_cur_out, search_level_out);
}

// Matcher::findEpipolarMatchDirect called directly (explicit depth interval): the tail of the function,
// matcher.cpp:340-354 -- cam2world of the refined pixel, depthFromTriangulation.
__global__ __launch_bounds__(256) void epi_finalize_kernel(
    DfFrame fr, int n, const double* __restrict__ f, const SeedRec* __restrict__ recs, uint8_t* __restrict__ ok_out,
    double* __restrict__ depth_out, double* __restrict__ px_cur_out, int32_t* __restrict__ search_level_out,
    int32_t* __restrict__ n_zmssd_out, int32_t* __restrict__ n_align_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const SeedRec rc = recs[i];
  bool ok = false;
  double z = 0.0;
  if (rc.path >= 0 && rc.matched) {
    const double fi[3] = {f[3 * (size_t)i], f[3 * (size_t)i + 1], f[3 * (size_t)i + 2]};
    double fc[3];
    cam2world(fr.cam, rc.step[0], rc.step[1], fc);
    ok = depth_from_triangulation(fr.T.T_cur_ref, fi, fc, &z);
  }
  ok_out[i] = ok ? 1 : 0;
  if (depth_out) depth_out[i] = ok ? z : 0.0;
  if (px_cur_out) {
    const bool have = rc.path >= 0 && rc.matched;        // px_cur_ is assigned when the alignment succeeded (:345)
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    px_cur_out[2 * (size_t)i] = have ? rc.step[0] : qnan;
    px_cur_out[2 * (size_t)i + 1] = have ? rc.step[1] : qnan;
  }
  if (search_level_out) search_level_out[i] = rc.path >= 0 ? rc.search_level : -1;
  if (n_zmssd_out) n_zmssd_out[i] = rc.n_zmssd;
  if (n_align_out) n_align_out[i] = rc.n_align;
}

// ---- Matcher::findMatchDirect over n (map point, reference feature) pairs (S/matcher.cpp:156-202) ----
// (MdFrame, md_geometry_item: svo_match_device.h)
// thread per item: frame test, depth, affine warp, search level -> SeedRec (path 0 = align2D, 3 = align1D)
// (five waves per SIMD, what the kernel reaches with 96 VGPRs: left to itself the scheduler takes 98 and four)
__global__ __launch_bounds__(256, 5) void md_geometry_kernel(
    MdFrame fr, int n, const double* __restrict__ T_ref_w /*[n_kf][7]*/, const int32_t* __restrict__ kf_slot,
    const double* __restrict__ px_ref, const double* __restrict__ f_ref, const int32_t* __restrict__ level,
    const double* __restrict__ pt_pos, const uint8_t* __restrict__ edgelet, const double* __restrict__ grad,
    const double* __restrict__ px_cur, SeedRec* __restrict__ recs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double g[2] = {grad ? grad[2 * (size_t)i] : 1.0, grad ? grad[2 * (size_t)i + 1] : 0.0};
  recs[i] = md_geometry_item(fr, T_ref_w, kf_slot[i], level[i], px_ref + 2 * (size_t)i, f_ref + 3 * (size_t)i, pt_pos + 3 * (size_t)i,
                             edgelet && edgelet[i], g, px_cur + 2 * (size_t)i);
}

__global__ void md_finalize_kernel(int n, const SeedRec* __restrict__ recs, double* __restrict__ px_cur,
                                   uint8_t* __restrict__ success, int32_t* __restrict__ search_level) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const SeedRec& rc = recs[i];
  if (rc.path >= 0) {            // the frame test passed: px_cur is always rewritten (matcher.cpp:200)
    px_cur[2 * (size_t)i] = rc.step[0];
    px_cur[2 * (size_t)i + 1] = rc.step[1];
  }
  success[i] = rc.path >= 0 && rc.matched;
  if (search_level) search_level[i] = rc.search_level;
}
}  // namespace
