// svo_two_view_device.h -- kernels of the bootstrap's two-view stage (svo_two_view_impl.h): the relative pose and the first map
// points from the KLT lists of svo_klt.hip, for every listed camera in one set of launches.
//
//   computeFundamental          S/initialization.cpp:260-329
//   addSecondFrame              S/initialization.cpp:85-138   (without the creation of the host objects)
//
// cv::findFundamentalMat / cv::recoverPose are OpenCV code that is not in the reference's tree: PARITY UNPINNED.  The algorithm
// is restated in tests/two_view_reference.py and these kernels are held to that model by bits; the arithmetic itself is in
// svo_two_view_math.h.  Sums over correspondences are integer counts only.
#pragma once
#include "svo_klt_types.h"
#include "svo_two_view_math.h"

namespace svo_tv {
using svo_klt::KltDev;

constexpr int TV_HYP_THREADS = 64;                   // hypotheses per block: 72 doubles of LDS each
constexpr int TV_STAGE = 1024;                        // correspondences staged in LDS at a time
constexpr int TV_FIN_THREADS = 256;

// one listed camera of a call
struct TvJob {
  int cam, n;
  int width, height;
  double error_multiplier2;
  double T_ref_w[7];
  char* result;                                       // the camera's page-locked result block (device address)
  unsigned long long seq;
};

// the stage's device arrays, [camera][max_features] each but count
struct TvDev {
  int32_t* count;                                     // [camera][TV_MAX_HYPOTHESES]
  double* xyz;                                        // x 3
  uint8_t* mask;
  int32_t* inliers;
  int32_t* pt_index;
  double* pt_pos;                                     // x 3
};

// the result block of a camera in page-locked memory
struct TvResultBlock {
  unsigned long long seq;
  int status, n_in, hypothesis, hypothesis_count, candidate, candidate_count, n_inliers, n_points;
  double depth_median, scale;
  double T_cur_from_ref[7], T_cur_w[7];
};

SVO_DEV void tv_load_xy(const KltDev& d, size_t i, float* xy) {
  double fr[3], fc[3];
  for (int k = 0; k < 3; ++k) { fr[k] = d.f_ref[3 * i + k]; fc[k] = d.f_cur[3 * i + k]; }
  tv_normalised(fr, xy);
  tv_normalised(fc, xy + 2);
}

// ---- one thread per hypothesis: sample, solve, score.  The 8 x 9 systems of a block lie element-major in LDS (entry e of
// thread t at [e * 64 + t]: consecutive lanes, consecutive banks); the correspondences are staged TV_STAGE at a time and every
// lane reads the same one while scoring.
__global__ __launch_bounds__(TV_HYP_THREADS) void tv_hypothesis_kernel(KltDev d, TvDev w, const TvJob* __restrict__ jobs, TvPrm prm) {
  __shared__ float4 s_xy[TV_STAGE];
  __shared__ double s_A[72 * TV_HYP_THREADS];
  const TvJob& job = jobs[blockIdx.y];
  const int n = job.n, t = threadIdx.x;
  if (n < 8) return;                                                              // block-uniform: TOO_FEW is the finish kernel's
  const size_t base = (size_t)job.cam * d.max_features;
  const int h = blockIdx.x * TV_HYP_THREADS + t;
  const bool live = h < prm.n_hypotheses;
  double F[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) F[i] = 0.0;
  bool ok = false;
  if (live) {
    int s[8];
    float p[8][4];
    tv_sample(prm.seed, h, n, s);
#pragma unroll
    for (int i = 0; i < 8; ++i) tv_load_xy(d, base + s[i], p[i]);
    ok = tv_hypothesis<TV_HYP_THREADS>(p, s_A + t, F);
  }
  const double thr2 = tv_thr2(prm.reproj_thresh, job.error_multiplier2);
  int count = 0;
  for (int j0 = 0; j0 < n; j0 += TV_STAGE) {                                       // block-uniform
    const int m = min(TV_STAGE, n - j0);
    __syncthreads();
    for (int j = t; j < m; j += TV_HYP_THREADS) {
      float xy[4];
      tv_load_xy(d, base + j0 + j, xy);
      s_xy[j] = make_float4(xy[0], xy[1], xy[2], xy[3]);
    }
    __syncthreads();
    if (ok)
      for (int j = 0; j < m; ++j) {
        const float4 q = s_xy[j];
        count += tv_epi_inlier(F, q.x, q.y, q.z, q.w, thr2) ? 1 : 0;
      }
  }
  if (live) w.count[(size_t)job.cam * TV_MAX_HYPOTHESES + h] = ok ? count : -1;
}

// ordered compaction of one chunk of TV_FIN_THREADS flags: the rank of a kept entry (ballot ranks, as klt_finish_kernel)
SVO_DEV int tv_chunk_rank(bool keep, int* s_wave, int* s_base) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const unsigned long long m = __ballot(keep);
  if (lane == 0) s_wave[wave] = __popcll(m);
  __syncthreads();
  int off = *s_base;
  for (int v = 0; v < wave; ++v) off += s_wave[v];
  const int rank = off + __popcll(m & ((1ull << lane) - 1ull));
  __syncthreads();
  if (t == 0) *s_base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
  __syncthreads();
  return rank;
}

// ---- everything behind the counts: one workgroup per listed camera
__global__ __launch_bounds__(TV_FIN_THREADS) void tv_finish_kernel(KltDev d, TvDev w, const TvJob* __restrict__ jobs, TvPrm prm) {
  __shared__ unsigned long long s_key[TV_FIN_THREADS];
  __shared__ double s_A[72], s_F[9], s_w[9], s_v[9], s_R1[9], s_R2[9], s_u3[3], s_R[4][9], s_t[4][3];
  __shared__ double s_Tcr[7], s_Tcw[7], s_Twc[7];
  __shared__ int s_cnt[4], s_wave[TV_FIN_THREADS / 64], s_base, s_count, s_nan;
  const TvJob& job = jobs[blockIdx.x];
  const int cam = job.cam, n = job.n, t = threadIdx.x, lane = t & 63;
  const size_t base = (size_t)cam * d.max_features;
  TvResultBlock* res = reinterpret_cast<TvResultBlock*>(job.result);
  int status = TV_OK, best_h = -1, best_count = -1, cand = -1, cand_count = 0, n_inliers = 0, n_points = 0;
  double median = __longlong_as_double(0x7ff8000000000000ll), scale = median;

  if (n < 8) status = TV_TOO_FEW;
  if (status == TV_OK) {
    // 1. arg-max: count descending, index ascending
    unsigned long long key = 0ull;
    for (int h = t; h < prm.n_hypotheses; h += TV_FIN_THREADS) {
      const int c = w.count[(size_t)cam * TV_MAX_HYPOTHESES + h];
      const unsigned long long k = ((unsigned long long)(unsigned)(c + 1) << 32) | (unsigned long long)(0xffffffffu - (unsigned)h);
      key = k > key ? k : key;
    }
    s_key[t] = key;
    __syncthreads();
    if (t == 0) {
      unsigned long long b = 0ull;
      for (int i = 0; i < TV_FIN_THREADS; ++i) b = s_key[i] > b ? s_key[i] : b;
      s_key[0] = b;
    }
    __syncthreads();
    key = s_key[0];
    best_count = (int)(key >> 32) - 1;
    best_h = (int)(0xffffffffu - (unsigned)(key & 0xffffffffull));
    if (best_count < 0) { status = TV_NO_MODEL; best_h = -1; }
  }
  if (status == TV_OK) {                                                           // block-uniform
    // 2. the winner again, its decomposition and the four candidates
    if (t == 0) {
      int s[8];
      float p[8][4];
      double F[9];
      tv_sample(prm.seed, best_h, n, s);
#pragma unroll
      for (int i = 0; i < 8; ++i) tv_load_xy(d, base + s[i], p[i]);
      (void)tv_hypothesis<1>(p, s_A, F);                                            // valid: it has a count
#pragma unroll
      for (int i = 0; i < 9; ++i) s_F[i] = F[i];
      tv_decompose(s_F, s_w, s_v, s_R1, s_R2, s_u3);
      for (int c = 0; c < 4; ++c) tv_candidate(c, s_R1, s_R2, s_u3, s_R[c], s_t[c]);
    }
    if (t < 4) s_cnt[t] = 0;
    __syncthreads();
    // 3. the mask and the cheirality counts
    const double thr2 = tv_thr2(prm.reproj_thresh, job.error_multiplier2);
    int cc[4] = {0, 0, 0, 0};
    for (int j = t; j < n; j += TV_FIN_THREADS) {
      float xy[4];
      double fr[3], fc[3];
      tv_load_xy(d, base + j, xy);
      const bool in = tv_epi_inlier(s_F, xy[0], xy[1], xy[2], xy[3], thr2);
      w.mask[base + j] = in ? 1 : 0;
      if (in) {
        for (int k = 0; k < 3; ++k) { fr[k] = d.f_ref[3 * (base + j) + k]; fc[k] = d.f_cur[3 * (base + j) + k]; }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          double lambda[2], xyz[3];
          tv_triangulate(s_R[c], s_t[c], fc, fr, lambda, xyz);
          cc[c] += (lambda[0] > 0.0 && lambda[1] > 0.0) ? 1 : 0;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int v = svo_dev::group_sum<64>(cc[c]);
      if (lane == 0 && v) atomicAdd(&s_cnt[c], v);
    }
    __syncthreads();
    cand = 0;
    for (int c = 1; c < 4; ++c) cand = s_cnt[c] > s_cnt[cand] ? c : cand;
    cand_count = s_cnt[cand];
    if ((double)cand_count < (double)n * 0.5) status = TV_CHEIRALITY;             // the gate of :305
  }
  if (status == TV_OK) {
    // 4. vk::computeInliers over all n, the inlier list in order
    if (t == 0) {
      s_base = 0; s_nan = 0;
      tv_quaternion(s_R[cand], s_Tcr + 3);                                          // (indexed by data: straight into LDS)
      for (int i = 0; i < 3; ++i) s_Tcr[i] = s_t[cand][i];
    }
    __syncthreads();
    int n_nan = 0;
    for (int k0 = 0; k0 < n; k0 += TV_FIN_THREADS) {                                // block-uniform
      const int j = k0 + t;
      bool keep = false;
      if (j < n) {
        double fr[3], fc[3], xyz[3];
        for (int k = 0; k < 3; ++k) { fr[k] = d.f_ref[3 * (base + j) + k]; fc[k] = d.f_cur[3 * (base + j) + k]; }
        keep = tv_compute_inlier(s_R[cand], s_t[cand], fc, fr, prm.reproj_thresh, job.error_multiplier2, xyz);
        for (int k = 0; k < 3; ++k) w.xyz[3 * (base + j) + k] = xyz[k];
        n_nan += xyz[2] != xyz[2] ? 1 : 0;
      }
      const int rank = tv_chunk_rank(keep, s_wave, &s_base);
      if (keep) w.inliers[base + rank] = j;
    }
    n_inliers = s_base;
    n_nan = svo_dev::group_sum<64>(n_nan);
    if (lane == 0 && n_nan) atomicAdd(&s_nan, n_nan);
    __threadfence_block();
    __syncthreads();
    // 5. the depth median at rank n / 2 over ALL depths: the largest key v with |{key < v}| <= rank, one bit a pass; a NaN
    // among the depths gives a NaN
    if (s_nan == 0) {
      const int rank = n / 2;
      unsigned long long v = 0ull;
      for (int bit = 63; bit >= 0; --bit) {
        const unsigned long long c = v | (1ull << bit);
        if (t == 0) s_count = 0;
        __syncthreads();
        int below = 0;
        for (int j = t; j < n; j += TV_FIN_THREADS) below += tv_depth_key(w.xyz[3 * (base + j) + 2]) < c ? 1 : 0;
        below = svo_dev::group_sum<64>(below);
        if (lane == 0 && below) atomicAdd(&s_count, below);
        __syncthreads();
        if (s_count <= rank) v = c;
        __syncthreads();
      }
      median = tv_depth_from_key(v);
    }
    if (n_inliers < prm.min_inliers) status = TV_FEW_INLIERS;                       // the gate of :85
  }
  if (status == TV_OK) {
    // 6. scale, the second frame's pose, the points in the order of the inlier list
    scale = prm.map_scale / median;
    if (t == 0) {
      tv_second_pose(s_Tcr, job.T_ref_w, scale, s_Tcw, s_Twc);
      s_base = 0;
    }
    __syncthreads();
    for (int k0 = 0; k0 < n_inliers; k0 += TV_FIN_THREADS) {                        // block-uniform
      const int k = k0 + t;
      bool keep = false;
      int j = 0;
      double pos[3] = {0.0, 0.0, 0.0};
      if (k < n_inliers) {
        j = w.inliers[base + k];
        const float* pc = d.px_cur + 2 * (base + j);
        const float* pr = d.px_ref + 2 * (base + j);
        double xyz[3];
        for (int i = 0; i < 3; ++i) xyz[i] = w.xyz[3 * (base + j) + i];
        keep = tv_in_frame(pc[0], pc[1], job.width, job.height) && tv_in_frame(pr[0], pr[1], job.width, job.height) && xyz[2] > 0.0;
        if (keep) {
          for (int i = 0; i < 3; ++i) xyz[i] = xyz[i] * scale;
          tv_se3_act(s_Twc, xyz, pos);
        }
      }
      const int rank = tv_chunk_rank(keep, s_wave, &s_base);
      if (keep) {
        w.pt_index[base + rank] = j;
        for (int i = 0; i < 3; ++i) w.pt_pos[3 * (base + rank) + i] = pos[i];
      }
    }
    n_points = s_base;
  } else {
    n_inliers = 0;                                                                  // a failure leaves no inliers and no points
  }
  if (t == 0) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    res->status = status; res->n_in = n;
    res->hypothesis = best_h; res->hypothesis_count = best_count;
    res->candidate = cand; res->candidate_count = cand_count;
    res->n_inliers = n_inliers; res->n_points = n_points;
    res->depth_median = median; res->scale = scale;
    const bool have_pose = status == TV_OK || status == TV_FEW_INLIERS;
    for (int i = 0; i < 7; ++i) {
      res->T_cur_from_ref[i] = have_pose ? s_Tcr[i] : nan;
      res->T_cur_w[i] = status == TV_OK ? s_Tcw[i] : nan;
    }
    __threadfence_system();
    __hip_atomic_store(&res->seq, job.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
}  // namespace svo_tv
