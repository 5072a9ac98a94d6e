// svo_track_frame_end.h -- what follows a tracked frame: the structure step, the keyframe decision, both in one launch
// (finish_frame, lone and per camera of a group), and point positions the host optimised scattered into the table.
#pragma once
#include "svo_point_refine.h"
#include "svo_track_chain.h"
namespace {
// ---- FrameHandlerBase::optimizeStructure (S/frame_handler_base.cpp:190-210) on the points the host selected: Point::optimize
// of each of them over its observations as the map tables hold them (keyframe pose + bearing, Point::obs_ order), the new
// positions written into the point table, into the solver's copy of the last frame's points (the next SparseImgAlign::run reads
// point->pos_) and into the page-locked result block.  One workgroup.
// (the body of trk_structure_kernel up to its hand-over: trk_finish_frame_body runs it in front of the keyframe decision)
SVO_DEV void trk_structure_body(const TrkMap& m, double* __restrict__ pt_pos, const TrkLast& last, const TrkStructSel& sel, int n_iter,
                                double* __restrict__ out_pos, int* __restrict__ out_iters) {
  __shared__ double s_new[TRK_MAX_STRUCT][3];
  const int t = threadIdx.x, nt = blockDim.x, n_sel = sel.n;
  if (t < n_sel) {
    const int p = sel.point[t];
    double P[3] = {pt_pos[3 * (size_t)p], pt_pos[3 * (size_t)p + 1], pt_pos[3 * (size_t)p + 2]};
    const int done = point_refine_one(P, m.pt_obs_offset[p], m.pt_obs_offset[p + 1], n_iter, [&](int o, double* T, double* fo) {
      const double* tk = m.T_kf_w + 7 * (size_t)m.obs_kf[o];
      for (int i = 0; i < 7; ++i) T[i] = tk[i];
      fo[0] = m.obs_f[3 * (size_t)o]; fo[1] = m.obs_f[3 * (size_t)o + 1]; fo[2] = m.obs_f[3 * (size_t)o + 2];
    });
    for (int i = 0; i < 3; ++i) { pt_pos[3 * (size_t)p + i] = P[i]; s_new[t][i] = P[i]; out_pos[3 * t + i] = P[i]; }
    out_iters[t] = done;
  }
  __syncthreads();
  const int n_last = *last.n < last.sia_max_n ? *last.n : last.sia_max_n;
  for (int j = t; j < n_last; j += nt) {
    const int p = last.point[j];
    if (p < 0) continue;
    for (int i = 0; i < n_sel; ++i)
      if (sel.point[i] == p) { last.sia_pos[3 * j] = s_new[i][0]; last.sia_pos[3 * j + 1] = s_new[i][1]; last.sia_pos[3 * j + 2] = s_new[i][2]; }
  }
}
__global__ __launch_bounds__(256) void trk_structure_kernel(TrkMap m, double* __restrict__ pt_pos, TrkLast last, TrkStructSel sel, int n_iter,
                                                            double* __restrict__ out_pos, int* __restrict__ out_iters,
                                                            unsigned long long* __restrict__ done_flag, unsigned long long seq) {
  const int t = threadIdx.x;
  trk_structure_body(m, pt_pos, last, sel, n_iter, out_pos, out_iters);
  __threadfence_system();
  __syncthreads();
  if (t == 0) __hip_atomic_store(done_flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- the keyframe decision behind the structure step (FrameHandlerMono::processFrame, S/frame_handler_mono.cpp:258-260, :305):
// frame_utils::getSceneDepth (S/frame.cpp:200-221), needNewKf (:391-403) and Map::getFurthestKeyframe (S/map.cpp:156-169) of the
// device's last frame.  One workgroup of FIN_THREADS; block-uniform call.  pt_pos: the table the structure step has just written
// (read through the same pointer, behind the caller's barrier).
//   depths     every thread walks its features; the numbers become order-preserving 64-bit keys in LDS (any order: what is
//              asked for is an order statistic), the minimum (and the maximum) an integer comparison of the keys
//   median     radix select on the keys, 8 bits a pass from the first byte the keys differ in: a 256-bin histogram of the keys
//              that share the prefix so far, its scan, and the bin that holds the rank extends the prefix -- exact, O(n), no
//              floating-point atomics
//   needNewKf  one thread per overlap keyframe, the first blocking one in list order
//   furthest   one thread per keyframe (TRK_LDS_KF <= FIN_THREADS); "dist > maxdist from 0.0" in index order = the largest
//              distance above zero, the lower index among equals, a NaN never: reduced with that order
constexpr int FIN_THREADS = 256;
constexpr int FIN_MAX_FEAT = 2816;             // svo_hip_tracker_config::max_frame_features <= this (trk_check_config)
SVO_DEV unsigned long long depth_key(double z) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(z);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
SVO_DEV double depth_from_key(unsigned long long k) {
  const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)u);
}
SVO_DEV void trk_decision_body(const TrkMap& m, const double* pt_pos, const TrkLast& last, const int* __restrict__ overlap_kf,
                               const int* __restrict__ counters, int overlap_valid, double min_dist, svo_hip_kf_decision* __restrict__ out) {
  static_assert(TRK_LDS_KF <= FIN_THREADS, "one keyframe per thread");
  static_assert(TRK_MAX_SEL <= FIN_THREADS, "one overlap keyframe per thread");
  __shared__ unsigned long long s_key[FIN_MAX_FEAT];
  __shared__ unsigned long long s_min_key, s_max_key, s_prefix;
  __shared__ int s_hist[256], s_wave[FIN_THREADS / 64];
  __shared__ int s_n, s_n_nan, s_rank, s_block[TRK_MAX_SEL];
  __shared__ double s_T[7], s_pos[3], s_wdist[FIN_THREADS / 64];
  __shared__ int s_wkf[FIN_THREADS / 64];
  const int t = threadIdx.x, nt = blockDim.x, lane = t & 63, wave = t >> 6;
  if (t < 7) s_T[t] = last.T_f_w[t];
  if (t == 0) { s_n = 0; s_n_nan = 0; s_min_key = ~0ull; s_max_key = 0ull; }
  s_hist[t] = 0;
  __syncthreads();
  double T[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) T[i] = s_T[i];
  if (t == 0) {
    double Tinv[7];
    se3_inverse(T, Tinv);                                                      // Frame::pos()
    s_pos[0] = Tinv[0]; s_pos[1] = Tinv[1]; s_pos[2] = Tinv[2];
  }
  // ---- the depths: a wave appends its keys with one atomic (ranks inside the wave from the ballot) and keeps the smallest
  // and the largest key and its NaN count in registers
  const int n_last = *last.n < FIN_MAX_FEAT ? *last.n : FIN_MAX_FEAT;
  unsigned long long kmin = ~0ull, kmax = 0ull;
  int my_nan = 0;
  for (int base = 0; base < n_last; base += nt) {                              // block-uniform
    const int j = base + t;
    const int p = j < n_last ? last.point[j] : -1;
    bool have = false;
    unsigned long long key = 0ull;
    if (p >= 0 && p < m.n_points) {
      double xyz_f[3];
      se3_act(T, pt_pos + 3 * (size_t)p, xyz_f);
      const double z = xyz_f[2];
      if (z != z) ++my_nan;
      else { have = true; key = depth_key(z); }
    }
    const unsigned long long bal = __ballot(have);
    if (bal != 0ull) {                                                         // wave-uniform
      const int first = __ffsll((long long)bal) - 1;
      int slot = 0;
      if (lane == first) slot = atomicAdd(&s_n, __popcll(bal));
      slot = __shfl(slot, first, 64);
      if (have) {
        s_key[slot + __popcll(bal & ((1ull << lane) - 1ull))] = key;
        kmin = key < kmin ? key : kmin; kmax = key > kmax ? key : kmax;
      }
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long a = __shfl_xor(kmin, o, 64), b = __shfl_xor(kmax, o, 64);
    kmin = a < kmin ? a : kmin; kmax = b > kmax ? b : kmax;
    my_nan += __shfl_xor(my_nan, o, 64);
  }
  if (lane == 0) {
    atomicMin(&s_min_key, kmin); atomicMax(&s_max_key, kmax);
    if (my_nan) atomicAdd(&s_n_nan, my_nan);
  }
  __syncthreads();
  const int n = s_n, n_nan = s_n_nan;
  const bool have_median = n > 0 && n_nan == 0;
  // ---- the median: the key of rank n / 2.  The bytes the smallest and the largest key share are every key's: the selection
  // starts at the first byte in which they differ (none: all depths are equal).
  const unsigned long long spread = s_min_key ^ s_max_key;
  const int first_shift = spread == 0ull ? -8 : 56 - (__clzll((long long)spread) & ~7);
  if (t == 0) { s_rank = n / 2; s_prefix = first_shift >= 56 ? 0ull : first_shift < 0 ? s_min_key : s_min_key & (~0ull << (first_shift + 8)); }
  __syncthreads();
  if (have_median) {                                                           // block-uniform
    for (int shift = first_shift; shift >= 0; shift -= 8) {                    // (every bin is zero here)
      const unsigned long long prefix = s_prefix;
      const int rank = s_rank;
      const unsigned long long above = shift == 56 ? 0ull : ~0ull << (shift + 8);
      for (int j = t; j < n; j += nt) {
        const unsigned long long k = s_key[j];
        if ((k & above) == prefix) atomicAdd(&s_hist[(int)((k >> shift) & 255ull)], 1);
      }
      __syncthreads();
      const int c = s_hist[t];
      s_hist[t] = 0;                                                           // (nobody else reads this bin)
      int incl = c;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
      }
      if (lane == 63) s_wave[wave] = incl;
      __syncthreads();
      int before = 0;
      for (int w = 0; w < wave; ++w) before += s_wave[w];
      const int excl = before + incl - c;
      if (rank >= excl && rank < excl + c) {                                   // exactly one bin holds the rank
        s_prefix = prefix | ((unsigned long long)t << shift);
        s_rank = rank - excl;
      }
      __syncthreads();
    }
  }
  // ---- needNewKf: rel = T_f_w * kf->pos() of every overlap keyframe
  const double depth_mean = have_median ? depth_from_key(s_prefix) : __longlong_as_double(0x7ff8000000000000ll);
  const int n_overlap = overlap_valid ? (counters[3] < TRK_MAX_SEL ? counters[3] : TRK_MAX_SEL) : 0;
  if (t < n_overlap) {
    const int k = overlap_kf[t];
    int block = 0;
    if (k >= 0 && k < m.n_kf) {
      const double* tk = m.T_kf_w + 7 * (size_t)k;
      double Tk[7], Tinv[7], rel[3];
#pragma unroll
      for (int i = 0; i < 7; ++i) Tk[i] = tk[i];
      se3_inverse(Tk, Tinv);
      se3_act(T, Tinv, rel);
      block = fabs(rel[0]) / depth_mean < min_dist && fabs(rel[1]) / depth_mean < min_dist * 0.8 && fabs(rel[2]) / depth_mean < min_dist * 1.3;
    }
    s_block[t] = block;
  }
  // ---- Map::getFurthestKeyframe
  double best_d = 0.0;
  int best_k = INT_MAX;
  if (t < m.n_kf && t < TRK_LDS_KF) {
    const double* tk = m.T_kf_w + 7 * (size_t)t;
    double Tk[7], Tinv[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) Tk[i] = tk[i];
    se3_inverse(Tk, Tinv);
    const double dx = Tinv[0] - s_pos[0], dy = Tinv[1] - s_pos[1], dz = Tinv[2] - s_pos[2];
    const double d = sqrt(dx * dx + dy * dy + dz * dz);
    if (d > 0.0) { best_d = d; best_k = t; }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double od = __shfl_xor(best_d, o, 64);
    const int ok = __shfl_xor(best_k, o, 64);
    if (od > best_d || (od == best_d && ok < best_k)) { best_d = od; best_k = ok; }
  }
  if (lane == 0) { s_wdist[wave] = best_d; s_wkf[wave] = best_k; }
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < FIN_THREADS / 64; ++w)
      if (s_wdist[w] > best_d || (s_wdist[w] == best_d && s_wkf[w] < best_k)) { best_d = s_wdist[w]; best_k = s_wkf[w]; }
    svo_hip_kf_decision r;
    r.n_depths = n; r.n_nan_depths = n_nan;
    r.depth_mean = depth_mean;
    r.depth_min = n > 0 ? depth_from_key(s_min_key) : DBL_MAX;
    r.overlap_valid = overlap_valid ? 1 : 0;
    r.need_new_kf = overlap_valid ? 1 : -1;
    r.blocking_kf = -1;
    for (int i = 0; i < n_overlap; ++i)
      if (s_block[i]) { r.need_new_kf = 0; r.blocking_kf = overlap_kf[i]; break; }
    r.furthest_kf = best_k == INT_MAX ? -1 : best_k;
    r.furthest_distance = best_k == INT_MAX ? 0.0 : best_d;
    r.pos[0] = s_pos[0]; r.pos[1] = s_pos[1]; r.pos[2] = s_pos[2];
    *out = r;                              // (out lies in host memory: written, never read back here)
  }
}

// The structure step, a barrier, the decision, the hand-over.  st: the camera's page-locked block [pos 64 x 3][iters 64][flag]
// [decision] (device address).
SVO_DEV void trk_finish_frame_body(const TrkMap& m, double* __restrict__ pt_pos, const TrkLast& last, const TrkStructSel& sel, int n_iter,
                                   const int* __restrict__ overlap_kf, const int* __restrict__ counters, int overlap_valid, double min_dist,
                                   char* st, unsigned long long seq) {
  if (sel.n > 0) {                                                             // block-uniform
    trk_structure_body(m, pt_pos, last, sel, n_iter, reinterpret_cast<double*>(st), reinterpret_cast<int*>(st + ST_O_ITERS));
    __syncthreads();                                                           // the decision reads the new positions
  }
  trk_decision_body(m, pt_pos, last, overlap_kf, counters, overlap_valid, min_dist, reinterpret_cast<svo_hip_kf_decision*>(st + ST_O_DECISION));
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(reinterpret_cast<unsigned long long*>(st + ST_O_FLAG), seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// (one workgroup per camera and nothing beside it: the occupancy bound leaves the structure step's per-thread arrays their place in LDS)
__global__ __launch_bounds__(FIN_THREADS) __attribute__((amdgpu_waves_per_eu(1, 1))) void trk_finish_frame_kernel(TrkMap m, double* __restrict__ pt_pos, TrkLast last, TrkStructSel sel, int n_iter,
                                                                       const int* __restrict__ overlap_kf, const int* __restrict__ counters,
                                                                       int overlap_valid, double min_dist, char* st, unsigned long long seq) {
  trk_finish_frame_body(m, pt_pos, last, sel, n_iter, overlap_kf, counters, overlap_valid, min_dist, st, seq);
}

__global__ __launch_bounds__(FIN_THREADS) __attribute__((amdgpu_waves_per_eu(1, 1))) void trk_finish_frames_cams_kernel(const TrkCamArgs* __restrict__ args, const TrkFinishReq* __restrict__ req,
                                                                             double min_dist) {
  // the request crosses the link once, into LDS (the structure step compares every feature of the last frame with the selection)
  static_assert(sizeof(TrkFinishReq) % 4 == 0 && sizeof(TrkFinishReq) / 4 <= FIN_THREADS, "one word per thread");
  __shared__ TrkFinishReq s_req;
  if (threadIdx.x < sizeof(TrkFinishReq) / 4)
    reinterpret_cast<unsigned*>(&s_req)[threadIdx.x] = reinterpret_cast<const unsigned*>(req + blockIdx.x)[threadIdx.x];
  __syncthreads();
  const TrkFinishReq& r = s_req;
  if (!r.active) return;                                                       // block-uniform
  const TrkCamArgs& a = args[blockIdx.x];
  trk_finish_frame_body(a.m, const_cast<double*>(a.m.pt_pos), a.last, r.sel, r.n_iter, a.pl.overlap_kf, a.pl.counters, r.overlap_valid, min_dist,
                        r.st, r.seq);
}

// Point::pos_ of n points after the host optimised them: one staged block in, one launch
__global__ void trk_scatter_positions_kernel(int n, const int* __restrict__ idx, const double* __restrict__ pos, double* __restrict__ pt_pos) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t p = (size_t)idx[i];
  pt_pos[3 * p] = pos[3 * i]; pt_pos[3 * p + 1] = pos[3 * i + 1]; pt_pos[3 * p + 2] = pos[3 * i + 2];
}
}  // namespace
