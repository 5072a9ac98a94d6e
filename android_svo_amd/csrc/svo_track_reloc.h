// svo_track_reloc.h -- relocalisation on the device map: the closest keyframe, and the last frame made from a keyframe.
#pragma once
#include "svo_track_chain.h"
namespace {
// ---- relocalisation: Map::getClosestKeyframe (S/map.cpp:109-151) and last_frame_ = ref_keyframe
// (FrameHandlerMono::relocalizeFrame, S/frame_handler_mono.cpp:337) on the tables.  One workgroup of RELOC_THREADS.
//   choose: every keyframe one of whose key points is visible from T is close (the first visible one decides), its distance is
//           (T.translation_vec() - T_kf_w.translation_vec()).norm(); the answer is the close keyframe other than `exclude` with the
//           smallest distance, the lower index on a tie (std::list::sort is stable over keyframes_ order).  Otherwise kf is given.
//   apply:  the last frame becomes that keyframe when it exists and its features fit: pose = row kf of T_kf_w; features = the
//           entries of its feature row whose point is living and observed in it, in row order, with the px / f of the point's first
//           observation there.  Counted first, written only when the count fits (a refused call changes nothing).  The solver's
//           slot gets the same features with T_ref_w = the keyframe's pose and T_cur_w_init = T (gate) or the keyframe's pose.
// T: the pose of the device's last frame (use_last_pose; read before anything is written) or the one passed by value.
__global__ __launch_bounds__(RELOC_THREADS) void trk_reloc_kernel(TrkMap m, TrkLast last, Cam cam, TrkRelocArgs a, TrkRelocOut* __restrict__ out) {
  static_assert(TRK_LDS_KF <= RELOC_THREADS, "one keyframe per thread");
  __shared__ double s_T[7], s_dist[TRK_LDS_KF];
  __shared__ int s_close[TRK_LDS_KF], s_wave[RELOC_THREADS / 64];
  __shared__ int s_kf, s_n_close, s_count, s_max_point;
  const int t = threadIdx.x, nt = blockDim.x, lane = t & 63, wave = t >> 6;
  if (t < 7) s_T[t] = a.use_last_pose ? last.T_f_w[t] : a.T[t];
  if (t == 0) { s_kf = a.kf; s_n_close = 0; s_count = 0; s_max_point = -1; }
  __syncthreads();
  double T[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) T[i] = s_T[i];
  if (a.choose) {                                                              // block-uniform
    for (int k = t; k < m.n_kf; k += nt) {
      int kp[5];
#pragma unroll
      for (int j = 0; j < 5; ++j) kp[j] = m.kf_key_point[5 * k + j];
      bool close = false;
#pragma unroll
      for (int j = 0; j < 5; ++j)
        if (!close && kp[j] >= 0) close = frame_is_visible(cam, T, m.pt_pos + 3 * (size_t)kp[j]);
      const double* tk = m.T_kf_w + 7 * (size_t)k;
      const double dx = T[0] - tk[0], dy = T[1] - tk[1], dz = T[2] - tk[2];
      s_close[k] = close ? 1 : 0;
      s_dist[k] = sqrt(dx * dx + dy * dy + dz * dz);
    }
    __syncthreads();
    if (t == 0) {                                                              // at most TRK_LDS_KF keyframes: one walk in index order
      int best = -1, n_close = 0;
      for (int k = 0; k < m.n_kf; ++k) {
        if (!s_close[k]) continue;
        ++n_close;
        if (k != a.exclude && (best < 0 || s_dist[k] < s_dist[best])) best = k;
      }
      s_kf = best; s_n_close = n_close;
    }
    __syncthreads();
  }
  const int k = s_kf;
  int n_feat = -1;
  bool apply = false;
  if (a.apply && k >= 0) {                                                     // block-uniform
    const int r0 = m.kf_ftr_offset[k], r1 = m.kf_ftr_offset[k + 1];
    // the point's first observation in keyframe k (-1: none, or the point is not living)
    auto obs_in_kf = [&](int i) {
      const int p = m.kf_ftr_point[i];
      if (p < 0 || m.pt_unlinked[p]) return -1;
      for (int o = m.pt_obs_offset[p]; o < m.pt_obs_offset[p + 1]; ++o)
        if (m.obs_kf[o] == k) return o;
      return -1;
    };
    int mine = 0;
    for (int i = r0 + t; i < r1; i += nt) mine += obs_in_kf(i) >= 0 ? 1 : 0;
    if (mine) atomicAdd(&s_count, mine);
    __syncthreads();
    n_feat = s_count;
    apply = n_feat <= a.max_feat;
    if (apply) {
      // ordered compaction of the row, a chunk of the workgroup's size at a time: ranks inside a wave from the ballot, across
      // the waves through LDS, across the chunks in `base`
      int base = 0;
      for (int c0 = r0; c0 < r1; c0 += nt) {                                   // block-uniform
        const int i = c0 + t;
        const int o = i < r1 ? obs_in_kf(i) : -1;
        const unsigned long long bal = __ballot(o >= 0);
        if (lane == 0) s_wave[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < RELOC_THREADS / 64; ++w) { const int c = s_wave[w]; before += w < wave ? c : 0; total += c; }
        if (o >= 0) {
          const int r = base + before + __popcll(bal & ((1ull << lane) - 1ull));
          const int p = m.kf_ftr_point[i];
          const double x = m.obs_px[2 * (size_t)o], y = m.obs_px[2 * (size_t)o + 1];
          const double f0 = m.obs_f[3 * (size_t)o], f1 = m.obs_f[3 * (size_t)o + 1], f2 = m.obs_f[3 * (size_t)o + 2];
          last.px[2 * r] = x; last.px[2 * r + 1] = y;
          last.f[3 * r] = f0; last.f[3 * r + 1] = f1; last.f[3 * r + 2] = f2;
          last.point[r] = p;
          if (r < last.sia_max_n) {
            last.sia_px[2 * r] = x; last.sia_px[2 * r + 1] = y;
            last.sia_f[3 * r] = f0; last.sia_f[3 * r + 1] = f1; last.sia_f[3 * r + 2] = f2;
            last.sia_pos[3 * r] = m.pt_pos[3 * (size_t)p]; last.sia_pos[3 * r + 1] = m.pt_pos[3 * (size_t)p + 1];
            last.sia_pos[3 * r + 2] = m.pt_pos[3 * (size_t)p + 2];
            last.sia_has_point[r] = 1;
          }
          atomicMax(&s_max_point, p);
        }
        base += total;
        __syncthreads();                                                       // (s_wave is rewritten by the next chunk)
      }
      if (t == 0) {
        *last.n = n_feat;
        FrameConst c;
        c.cam = cam;
        const double* tk = m.T_kf_w + 7 * (size_t)k;
        for (int i = 0; i < 7; ++i) { const double v = tk[i]; last.T_f_w[i] = v; c.T_ref_w[i] = v; c.T_cur_w_init[i] = a.gate ? T[i] : v; }
        double Tinv[7];
        se3_inverse(c.T_ref_w, Tinv);                                          // Frame::pos()
        c.ref_pos[0] = Tinv[0]; c.ref_pos[1] = Tinv[1]; c.ref_pos[2] = Tinv[2];
        c.n_feat = n_feat < last.sia_max_n ? n_feat : last.sia_max_n; c.pad = 0;
        last.sia_fc[0] = c;
      }
    }
  }
  __syncthreads();
  if (t == 0) {
    TrkRelocOut r;
    r.distance = a.choose && k >= 0 ? s_dist[k] : 0.0;
    r.kf = k; r.n_close = s_n_close; r.n_feat = n_feat; r.applied = apply ? 1 : 0; r.max_point = s_max_point; r.pad = 0;
    *out = r;
  }
}
}  // namespace
