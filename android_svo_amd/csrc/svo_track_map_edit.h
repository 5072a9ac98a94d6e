// svo_track_map_edit.h -- the device map edited in place: key points chosen again, candidates appended, the last frame
// promoted to a keyframe, a keyframe removed, the points renumbered.
#pragma once
#include "svo_track_chain.h"
namespace {
// The value of a feature for key-point slot j (0: distance from the centre, smaller is better; 1..4: the quadrant products,
// larger is better, -inf outside the quadrant -- the two left quadrants test x against cv as the reference does,
// S/frame.cpp:133,142).  Shared by the re-selection after deletions and by the selection for a promoted keyframe.
SVO_DEV double key_slot_value(int cu, int cv, int j, double x, double y) {
  if (j == 0) return fmax(fabs(x - cu), fabs(y - cv));
  const bool in = j == 1 ? (x >= cu && y >= cv) : j == 2 ? (x >= cu && y < cv) : j == 3 ? (x < cv && y < cv) : (x < cv && y >= cv);
  return in ? (x - cu) * (y - cv) : -HUGE_VAL;
}
// a thread's running best of the five slots over the features it visits in ascending index: the first best index is kept
struct KeyBest { double v[5]; int i[5]; };
SVO_DEV void key_best_init(KeyBest& b) {
#pragma unroll
  for (int j = 0; j < 5; ++j) { b.v[j] = j == 0 ? HUGE_VAL : -HUGE_VAL; b.i[j] = INT_MAX; }
}
SVO_DEV void key_best_offer(KeyBest& b, int cu, int cv, int idx, double x, double y) {
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const double v = key_slot_value(cu, cv, j, x, y);
    const bool better = j == 0 ? v < b.v[j] : v > b.v[j];
    if (better) { b.v[j] = v; b.i[j] = idx; }
  }
}
// The five slots over the bests of the workgroup's first KEY_THREADS threads: thread j < 5 gets slot j's best value and, on
// ties, the lowest feature index; false: no contender (a feature outside the quadrant is none) or not one of the five threads.
// Block-uniform call with a barrier inside (between the threads' stores to LDS and the five threads' reads).
constexpr int KEY_THREADS = 256;
SVO_DEV bool key_best_select(const KeyBest& best, double* bv_out, int* bi_out) {
  __shared__ int s_idx[5][KEY_THREADS];
  __shared__ double s_val[5][KEY_THREADS];
  const int t = threadIdx.x;
  if (t < KEY_THREADS) {
#pragma unroll
    for (int j = 0; j < 5; ++j) { s_val[j][t] = best.v[j]; s_idx[j][t] = best.i[j]; }
  }
  __syncthreads();
  if (t >= 5) return false;
  double bv = t == 0 ? HUGE_VAL : -HUGE_VAL;
  int bi = INT_MAX;
  for (int q = 0; q < KEY_THREADS; ++q) {
    const double v = s_val[t][q];
    const int i = s_idx[t][q];
    if (i == INT_MAX) continue;
    const bool better = t == 0 ? v < bv : v > bv;
    if (better || (v == bv && i < bi)) { bv = v; bi = i; }
  }
  *bv_out = bv; *bi_out = bi;
  return bi != INT_MAX && (t == 0 || bv > -HUGE_VAL);
}

// ---- Frame::removeKeyPoint / setKeyPoints (S/frame.cpp:83-165) for the keyframes that lost a key feature to a point the
// reprojector deleted in the previous frame (Map::safeDeletePoint, S/map.cpp:78-88): one workgroup per keyframe.
// A keyframe none of whose key features lost its point keeps its key features untouched, as in the reference (they are
// incumbents of the frame's history, not necessarily what a fresh selection would give).  In a keyframe that lost one,
// every slot is contested again by every feature that still has a point, in fts_ order with strict improvement: the
// incumbent stays on a tie, otherwise the first feature that reaches the best value wins.  A feature's pixel is the
// observation of its point in this keyframe.
__global__ __launch_bounds__(KEY_THREADS) void trk_rekey_kernel(TrkMap m, int* __restrict__ kf_key_point, Cam cam) {
  const int k = blockIdx.x, t = threadIdx.x, nt = blockDim.x;        // (nt = KEY_THREADS)
  __shared__ int s_found, s_inc[5];
  __shared__ double s_inc_val[5];
  const int cu = cam.width / 2, cv = cam.height / 2;
  // pixel of point p's observation in keyframe k (false: none)
  auto px_in_kf = [&](int p, double* x, double* y) {
    for (int o = m.pt_obs_offset[p]; o < m.pt_obs_offset[p + 1]; ++o)
      if (m.obs_kf[o] == k) { *x = m.obs_px[2 * (size_t)o]; *y = m.obs_px[2 * (size_t)o + 1]; return true; }
    return false;
  };
  if (t == 0) s_found = 0;
  __syncthreads();
  if (t < 5) {
    int p = kf_key_point[5 * k + t];
    if (p >= 0 && m.pt_unlinked[p]) { p = -1; atomicOr(&s_found, 1); }       // the key feature's point is gone (:85-88, :157-162)
    double x = 0, y = 0;
    const bool has = p >= 0 && px_in_kf(p, &x, &y);
    s_inc[t] = has ? p : -1;
    s_inc_val[t] = has ? key_slot_value(cu, cv, t, x, y) : 0.0;
  }
  __syncthreads();
  if (!s_found) return;                                                        // block-uniform
  KeyBest best;
  key_best_init(best);
  const int f0 = m.kf_ftr_offset[k], f1 = m.kf_ftr_offset[k + 1];
  for (int i = f0 + t; i < f1; i += nt) {                                      // ascending per thread: the first best index is kept
    const int p = m.kf_ftr_point[i];
    if (p < 0 || m.pt_unlinked[p]) continue;                                   // ftr->point == NULL
    double x, y;
    if (!px_in_kf(p, &x, &y)) continue;
    key_best_offer(best, cu, cv, i, x, y);
  }
  double bv;
  int bi;
  const bool challenger = key_best_select(best, &bv, &bi);
  if (t < 5) {
    int winner = s_inc[t];
    if (challenger && (winner < 0 || (t == 0 ? bv < s_inc_val[t] : bv > s_inc_val[t]))) winner = m.kf_ftr_point[bi];
    kf_key_point[5 * k + t] = winner;
  }
}

// ---- one observation (a keyframe's feature that refers to a point) as a value.  The field list of an observation is written
// here, once for reading and once for writing, and once each for the two things a new observation is made from.
struct TrkCandRec { double pos[3], px[2], f[3], grad[2]; int kf, level, edgelet, obs; };    // obs: where its observation goes
struct ObsRow { int kf; double px[2], f[3]; int level; uint8_t edgelet; double grad[2]; };
SVO_DEV ObsRow obs_load(const TrkMap& m, size_t o) {
  return {m.obs_kf[o], {m.obs_px[2 * o], m.obs_px[2 * o + 1]}, {m.obs_f[3 * o], m.obs_f[3 * o + 1], m.obs_f[3 * o + 2]},
          m.obs_level[o], m.obs_edgelet[o], {m.obs_grad[2 * o], m.obs_grad[2 * o + 1]}};
}
SVO_DEV void obs_store(const TrkTables& g, size_t d, const ObsRow& r) {
  g.obs_kf[d] = r.kf;
  g.obs_px[2 * d] = r.px[0]; g.obs_px[2 * d + 1] = r.px[1];
  g.obs_f[3 * d] = r.f[0]; g.obs_f[3 * d + 1] = r.f[1]; g.obs_f[3 * d + 2] = r.f[2];
  g.obs_level[d] = r.level; g.obs_edgelet[d] = r.edgelet;
  g.obs_grad[2 * d] = r.grad[0]; g.obs_grad[2 * d + 1] = r.grad[1];
}
// feature i of the tracked frame, seen from keyframe k
SVO_DEV ObsRow obs_of_feature(const TrkFeat& ft, int i, int k) {
  return {k, {ft.px[2 * i], ft.px[2 * i + 1]}, {ft.f[3 * i], ft.f[3 * i + 1], ft.f[3 * i + 2]}, ft.level[i], ft.edgelet[i],
          {ft.grad[2 * i], ft.grad[2 * i + 1]}};
}
SVO_DEV ObsRow obs_of_record(const TrkCandRec& r) {
  return {r.kf, {r.px[0], r.px[1]}, {r.f[0], r.f[1], r.f[2]}, r.level, (uint8_t)(r.edgelet ? 1 : 0), {r.grad[0], r.grad[1]}};
}

// ---- the map grows in place.  New point candidates (DepthFilter::updateSeeds :310-331 + MapPointCandidates::newCandidatePoint,
// S/map.cpp:226-231): n records from one staged block go to the tails of the point tables and of the current table set (tb);
// no entry that existed before is written.
__global__ void trk_add_candidates_kernel(int n, const TrkCandRec* __restrict__ rec, int n_points, int n_cand, double* __restrict__ pt_pos,
                                          int* __restrict__ pt_type, int* __restrict__ pt_n_failed, int* __restrict__ pt_n_succeeded,
                                          uint8_t* __restrict__ pt_unlinked, TrkTables tb) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const TrkCandRec r = rec[i];
  const size_t p = (size_t)n_points + i;
  pt_pos[3 * p] = r.pos[0]; pt_pos[3 * p + 1] = r.pos[1]; pt_pos[3 * p + 2] = r.pos[2];
  pt_type[p] = TYPE_CANDIDATE; pt_n_failed[p] = 0; pt_n_succeeded[p] = 0; pt_unlinked[p] = 0;
  if (p == 0) tb.pt_obs_offset[0] = 0;                                         // (a map without points has no offsets yet)
  tb.pt_obs_offset[p + 1] = r.obs + (r.kf >= 0 ? 1 : 0);
  tb.cand_point[n_cand + i] = (int)p;
  if (r.kf >= 0) obs_store(tb, (size_t)r.obs, obs_of_record(r));
}

// ---- the rebuild kernels: a promotion, a removal, a renumbering.  Each is one workgroup of TRK_THREADS that reads the current
// table set through m and writes the other set g (the pt_* rows, the keyframe tables and the last frame are edited where they
// lie), with sc and the per-point array mark as scratch, and leaves its counts in sc.out (trk_rebuild_end).
// The tracked frame becomes keyframe n_kf (FrameHandlerMono::processFrame :267-276, map_.addKeyframe :312): the observation CSR
// (Point::addFrameRef pushes the new observation to the FRONT of Point::obs_, S/point.cpp:61-65), the keyframes' feature rows
// (the new keyframe's row, and the seed features MapPointCandidates::addCandidatePointToFrame adds to the END of their
// keyframes' rows, S/map.cpp:236-254) and the candidate list (compacted, order kept).  out[0]: promoted candidates.
constexpr int TRK_MAX_FRAME_FEATURES = 2816;   // trk_check_config
__global__ __launch_bounds__(TRK_THREADS) void trk_promote_kernel(TrkMap m, TrkTables g, TrkScratch sc, double* __restrict__ T_kf_w,
                                                                  double* __restrict__ T_slot_w, int* __restrict__ kf_slot,
                                                                  int* __restrict__ kf_key_point, int* __restrict__ mark, TrkFeat ft, TrkLast last,
                                                                  int n_feat, int slot, Cam cam) {
  __shared__ int s_part[TRK_THREADS];
  __shared__ int s_fscan[TRK_MAX_FRAME_FEATURES + 1];
  __shared__ int s_n_promoted;
  const int t = threadIdx.x, nt = blockDim.x;
  const int k = m.n_kf;
  if (t == 0) s_n_promoted = 0;
  // ---- the frame's features that still have a point (mark[p] = the feature), their rank in creation order
  for (int p = t; p < m.n_points; p += nt) mark[p] = INT_MAX;
  for (int i = t; i < n_feat; i += nt) s_fscan[i] = last.point[i] >= 0 ? 1 : 0;
  __syncthreads();
  for (int i = t; i < n_feat; i += nt) {
    const int p = last.point[i];
    if (p >= 0) atomicMin(&mark[p], i);
  }
  __syncthreads();
  // ---- observations: every point's old range behind its new observation
  for (int p = t; p < m.n_points; p += nt) g.pt_obs_offset[p] = m.pt_obs_offset[p + 1] - m.pt_obs_offset[p] + (mark[p] != INT_MAX ? 1 : 0);
  __syncthreads();
  block_exclusive_scan(g.pt_obs_offset, m.n_points, s_part);
  block_exclusive_scan(s_fscan, n_feat, s_part);
  for (int p = t; p < m.n_points; p += nt) {
    size_t d = (size_t)g.pt_obs_offset[p];
    const int i = mark[p];
    if (i != INT_MAX) obs_store(g, d++, obs_of_feature(ft, i, k));
    for (size_t o = (size_t)m.pt_obs_offset[p]; o < (size_t)m.pt_obs_offset[p + 1]; ++o) obs_store(g, d++, obs_load(m, o));
  }
  // ---- MapPointCandidates::addCandidatePointToFrame: a candidate the frame observes becomes a map point; the others stay
  for (int c = t; c < m.n_candidates; c += nt) {
    const int p = m.cand_point[c];
    int seed = -2;
    if (p >= 0 && mark[p] != INT_MAX) {
      const int o0 = m.pt_obs_offset[p], o1 = m.pt_obs_offset[p + 1];
      seed = o1 > o0 ? m.obs_kf[o1 - 1] : -1;                                  // it->second->frame (none: that keyframe left the map)
      m.pt_type[p] = TYPE_UNKNOWN; m.pt_n_failed[p] = 0;
      atomicAdd(&s_n_promoted, 1);
    }
    sc.cand_seed[c] = seed;                                                    // (read back by this thread in the compaction, by all behind its barriers)
  }
  block_compact(m.n_candidates, sc.cand_scan, s_part, [&](int c) { return m.cand_point[c] >= 0 && sc.cand_seed[c] == -2; },
                [&](int r, int c) { g.cand_point[r] = m.cand_point[c]; });
  // ---- the keyframes' feature rows: the old row, then the promoted seeds of that keyframe in list order; the new keyframe's row
  for (int kk = t; kk <= k; kk += nt) {
    int cnt = s_fscan[n_feat];
    if (kk < k) {
      cnt = m.kf_ftr_offset[kk + 1] - m.kf_ftr_offset[kk];
      for (int c = 0; c < m.n_candidates; ++c) cnt += sc.cand_seed[c] == kk ? 1 : 0;
    }
    g.kf_ftr_offset[kk] = cnt;
  }
  __syncthreads();
  block_exclusive_scan(g.kf_ftr_offset, k + 1, s_part);
  for (int kk = 0; kk < k; ++kk) {
    const int src = m.kf_ftr_offset[kk], len = m.kf_ftr_offset[kk + 1] - src, dst = g.kf_ftr_offset[kk];
    for (int j = t; j < len; j += nt) g.kf_ftr_point[dst + j] = m.kf_ftr_point[src + j];
  }
  for (int kk = t; kk < k; kk += nt) {
    int at = g.kf_ftr_offset[kk] + m.kf_ftr_offset[kk + 1] - m.kf_ftr_offset[kk];
    for (int c = 0; c < m.n_candidates; ++c)
      if (sc.cand_seed[c] == kk) g.kf_ftr_point[at++] = m.cand_point[c];
  }
  const int row_k = g.kf_ftr_offset[k];
  for (int i = t; i < n_feat; i += nt) {
    const int p = last.point[i];
    if (p >= 0) g.kf_ftr_point[row_k + s_fscan[i]] = p;
  }
  // ---- Frame::setKeyPoints (S/frame.cpp:84-146) from five empty slots over the features with a point, in fts_ order
  const int cu = cam.width / 2, cv = cam.height / 2;
  KeyBest best;
  key_best_init(best);
  if (t < KEY_THREADS)
    for (int i = t; i < n_feat; i += KEY_THREADS)
      if (last.point[i] >= 0) key_best_offer(best, cu, cv, i, ft.px[2 * i], ft.px[2 * i + 1]);
  double bv;
  int bi;
  const bool challenger = key_best_select(best, &bv, &bi);
  if (t < 5) kf_key_point[5 * k + t] = challenger ? last.point[bi] : -1;
  if (t < 7) {                                                                  // the pose as the frame left it
    const double v = last.T_f_w[t];
    T_kf_w[7 * (size_t)k + t] = v;
    T_slot_w[7 * (size_t)slot + t] = v;
  }
  if (t == 0) {
    kf_slot[k] = slot;
    sc.out[0] = s_n_promoted;
    sc.out[1] = g.kf_ftr_offset[k + 1];
    sc.out[2] = g.pt_obs_offset[m.n_points];
    sc.out[3] = sc.cand_scan[m.n_candidates];
  }
}

// rows first + 1 .. n_rows - 1 of an [n_rows][W] table move down by one row in place: every element is read, then -- behind
// a barrier -- written.  A thread holds at most two (TRK_LDS_KF rows over TRK_THREADS threads).  Block-uniform call.
template <typename T, int W>
SVO_DEV void rows_move_down(T* a, int first, int n_rows) {
  static_assert(TRK_LDS_KF * W <= 2 * TRK_THREADS, "two elements per thread cover the largest table");
  const int t = threadIdx.x, nt = blockDim.x;
  const int n = (n_rows - 1 - first) * W;
  T* dst = a + (size_t)first * W;
  T v0 = T(), v1 = T();
  if (t < n) v0 = dst[t + W];
  if (t + nt < n) v1 = dst[t + nt + W];
  __syncthreads();
  if (t < n) dst[t] = v0;
  if (t + nt < n) dst[t + nt] = v1;
}

// feature i of the last frame loses its point (Map::safeDeletePoint clears ftr->point of every observation), and the solver
// its copy of it: what it holds of a feature without a point
SVO_DEV void last_feature_loses_point(const TrkLast& last, int i) {
  last.point[i] = -1;
  if (i < last.sia_max_n) {
    last.sia_has_point[i] = 0;
    last.sia_pos[3 * i] = 0.0; last.sia_pos[3 * i + 1] = 0.0; last.sia_pos[3 * i + 2] = 1.0;
  }
}

// ---- keyframe k leaves the map: Map::safeDeleteFrame (S/map.cpp:41-64) on the tables.  removePtFrameRef (:66-80) over the
// keyframe's features that have a point: a point with at most two observations is deleted (safeDeletePoint :82-93, deletePoint
// :95-99), any other loses its observation in k (Point::deleteFrameRef, S/point.cpp:75-86).  A point has one feature per keyframe
// at most, so the decisions are independent.  removeFrameCandidates / deleteCandidate (:271-285, :297-304): the candidates whose
// seed feature (the last observation of their range) lies in k are deleted.  The second set receives the tables in the form a
// host flatten gives them: an unlinked point -- by this call or by an earlier frame -- has no observations, is in no feature
// row and not in the candidate list; row order and observation order are kept, keyframes above k move down by one.  The key
// points of the other keyframes are left to trk_rekey_kernel (the deleted points are unlinked).  A feature of the last frame
// whose point was deleted here loses it.  out[0]: deleted points, out[4]: deleted candidates.
__global__ __launch_bounds__(TRK_THREADS) void trk_remove_kernel(TrkMap m, TrkTables g, TrkScratch sc, double* __restrict__ T_kf_w,
                                                                 int* __restrict__ kf_slot, int* __restrict__ kf_key_point, int* __restrict__ mark,
                                                                 TrkLast last, int k, int n_ftr) {
  __shared__ int s_part[TRK_THREADS];
  __shared__ int s_del_points, s_del_cands;
  const int t = threadIdx.x, nt = blockDim.x;
  const int K = m.n_kf, P = m.n_points;
  if (t == 0) { s_del_points = 0; s_del_cands = 0; }
  for (int p = t; p < P; p += nt) mark[p] = 0;
  __syncthreads();
  // ---- the decisions: mark[p] = 1 deleted as a map point, 2 deleted as a candidate
  const int r0 = m.kf_ftr_offset[k], r1 = m.kf_ftr_offset[k + 1];
  auto linked = [&](int p) { return p >= 0 && !m.pt_unlinked[p]; };             // ftr->point != NULL
  for (int i = r0 + t; i < r1; i += nt) {
    const int p = m.kf_ftr_point[i];
    if (linked(p) && m.pt_obs_offset[p + 1] - m.pt_obs_offset[p] <= 2) mark[p] = 1;      // pt->obs_.size() <= 2
  }
  for (int c = t; c < m.n_candidates; c += nt) {
    const int p = m.cand_point[c];
    if (!linked(p)) continue;
    const int o0 = m.pt_obs_offset[p], o1 = m.pt_obs_offset[p + 1];
    if (o1 > o0 && m.obs_kf[o1 - 1] == k) mark[p] = 2;                           // it->second->frame == frame
  }
  __syncthreads();
  // ---- the points: type and link, and what is left of every observation list
  int n_dp = 0, n_dc = 0;
  for (int p = t; p < P; p += nt) {
    const int mk = mark[p];
    bool gone = m.pt_unlinked[p] != 0;
    if (mk) {
      m.pt_type[p] = TYPE_DELETED; m.pt_unlinked[p] = 1;
      gone = true;
      if (mk == 1) ++n_dp; else ++n_dc;
    }
    int cnt = 0;
    if (!gone)
      for (int o = m.pt_obs_offset[p]; o < m.pt_obs_offset[p + 1]; ++o) cnt += m.obs_kf[o] != k ? 1 : 0;
    g.pt_obs_offset[p] = cnt;
  }
  if (n_dp) atomicAdd(&s_del_points, n_dp);
  if (n_dc) atomicAdd(&s_del_cands, n_dc);
  __syncthreads();
  block_exclusive_scan(g.pt_obs_offset, P, s_part);
  for (int p = t; p < P; p += nt) {
    if (m.pt_unlinked[p]) continue;
    size_t d = (size_t)g.pt_obs_offset[p];
    for (size_t o = (size_t)m.pt_obs_offset[p]; o < (size_t)m.pt_obs_offset[p + 1]; ++o) {
      ObsRow r = obs_load(m, o);
      if (r.kf == k) continue;
      if (r.kf > k) --r.kf;
      obs_store(g, d++, r);
    }
  }
  // ---- the feature rows: row k goes, the others keep the entries that still have a point
  block_compact(n_ftr, sc.ftr_scan, s_part, [&](int i) { return (i < r0 || i >= r1) && linked(m.kf_ftr_point[i]); },
                [&](int r, int i) { g.kf_ftr_point[r] = m.kf_ftr_point[i]; });
  for (int j = t; j < K; j += nt) g.kf_ftr_offset[j] = sc.ftr_scan[m.kf_ftr_offset[j < k ? j : j + 1]];    // (K - 1 rows, K offsets)
  // ---- the candidate list, compacted
  block_compact(m.n_candidates, sc.cand_scan, s_part, [&](int c) { return linked(m.cand_point[c]); },
                [&](int r, int c) { g.cand_point[r] = m.cand_point[c]; });
  // ---- the keyframe tables
  rows_move_down<double, 7>(T_kf_w, k, K);
  rows_move_down<int, 5>(kf_key_point, k, K);
  rows_move_down<int, 1>(kf_slot, k, K);
  // ---- the last frame
  const int n_last = *last.n;
  for (int i = t; i < n_last; i += nt) {
    const int p = last.point[i];
    if (p >= 0 && p < P && mark[p]) last_feature_loses_point(last, i);
  }
  if (t == 0) {
    sc.out[0] = s_del_points;
    sc.out[1] = sc.ftr_scan[n_ftr];
    sc.out[2] = g.pt_obs_offset[P];
    sc.out[3] = sc.cand_scan[m.n_candidates];
    sc.out[4] = s_del_cands;
  }
}

// ---- the points are renumbered in place: the unlinked ones (pt_unlinked: deleted by a tracked frame or by a removal) leave
// the tables, the others keep their order -- a living point's new index is the number of living points below it.  The tables
// end in the form a host flatten under the new numbering writes, the one trk_remove_kernel leaves: no row, no observation, no
// feature-row entry and no candidate entry of a dead point, -1 entries dropped, every order kept.
// What holds a point index, and what becomes of it here:
//   kf_key_point, kf_ftr_point, cand_point        rewritten (the pending re-selection of key points has run before the launch)
//   TrkLast::point (the last frame's features)    rewritten; a feature whose point is dead loses it as in trk_remove_kernel
//                                                 (none after a tracked frame)
//   the solver's slot (sia_pos, sia_has_point)    holds positions and flags by feature, no index
//   the pt_* rows, pt_unlinked, pt_obs_offset     the rows of the living points move down, the offsets are rebuilt
//   TrkPlan::first_seq / item_point / cand_point, TrkFeat::point, TrkStructSel: scratch of one call, rebuilt by the next
//   svo_hip_tracker::last_max_point               host side: set from out[4] (svo_hip_tracker_compact_points)
//   svo_hip_tracker::track_n_points and the page-locked result block: NOT rewritten -- svo_hip_tracker_last_result keeps
//                                                 returning the frame under the numbering it was tracked with
// mark[p] receives old_to_new: the new index, -1 for a dead point; the host copies it out.  out[0]: the points afterwards.
// The observation CSR, the feature rows and the candidate list go to the second set.  The pt_* rows have no second set: they
// move down in place by an ascending walk in chunks of one block -- every thread reads the row of its point of the chunk into
// registers, a barrier, then writes it to its new index.  A new index is never above the old one, so the writes of a chunk land
// on rows of this chunk (read before the barrier) or of earlier chunks (read in earlier rounds), never on a row a later chunk
// has yet to read: one barrier a chunk is enough.
__global__ __launch_bounds__(TRK_THREADS) void trk_compact_kernel(TrkMap m, TrkTables g, TrkScratch sc, double* __restrict__ pt_pos,
                                                                  int* __restrict__ kf_key_point, int* __restrict__ mark, TrkLast last, int n_ftr) {
  __shared__ int s_part[TRK_THREADS];
  __shared__ int s_last_max;
  const int t = threadIdx.x, nt = blockDim.x;
  const int K = m.n_kf, P = m.n_points;
  if (t == 0) s_last_max = -1;
  // ---- the new indices: an exclusive scan over "living" (in the second set's offsets: P + 1 entries)
  for (int p = t; p < P; p += nt) g.pt_obs_offset[p] = m.pt_unlinked[p] ? 0 : 1;
  __syncthreads();
  block_exclusive_scan(g.pt_obs_offset, P, s_part);
  const int N = g.pt_obs_offset[P];
  for (int p = t; p < P; p += nt) mark[p] = m.pt_unlinked[p] ? -1 : g.pt_obs_offset[p];
  __syncthreads();                                                               // (every thread holds N; the offsets are free again)
  // ---- the observations of the living points, by new index
  for (int p = t; p < P; p += nt) {
    const int q = mark[p];
    if (q >= 0) g.pt_obs_offset[q] = m.pt_obs_offset[p + 1] - m.pt_obs_offset[p];
  }
  __syncthreads();
  block_exclusive_scan(g.pt_obs_offset, N, s_part);
  for (int p = t; p < P; p += nt) {
    const int q = mark[p];
    if (q < 0) continue;
    size_t d = (size_t)g.pt_obs_offset[q];
    for (size_t o = (size_t)m.pt_obs_offset[p]; o < (size_t)m.pt_obs_offset[p + 1]; ++o) obs_store(g, d++, obs_load(m, o));
  }
  // ---- the feature rows and the candidate list keep the entries that still have a point, under its new index
  auto living = [&](int p) { return p >= 0 && mark[p] >= 0; };
  block_compact(n_ftr, sc.ftr_scan, s_part, [&](int i) { return living(m.kf_ftr_point[i]); },
                [&](int r, int i) { g.kf_ftr_point[r] = mark[m.kf_ftr_point[i]]; });
  if (K > 0)                                                                     // (a map without keyframes has no offsets)
    for (int j = t; j <= K; j += nt) g.kf_ftr_offset[j] = sc.ftr_scan[m.kf_ftr_offset[j]];
  block_compact(m.n_candidates, sc.cand_scan, s_part, [&](int c) { return living(m.cand_point[c]); },
                [&](int r, int c) { g.cand_point[r] = mark[m.cand_point[c]]; });
  // ---- the key points (none is dead after the re-selection; one that were would become -1)
  for (int j = t; j < 5 * K; j += nt) {
    const int p = kf_key_point[j];
    if (p >= 0) kf_key_point[j] = mark[p];
  }
  // ---- the last frame
  const int n_last = *last.n;
  int last_max = -1;
  for (int i = t; i < n_last; i += nt) {
    const int p = last.point[i];
    if (p < 0 || p >= P) continue;
    const int q = mark[p];
    if (q < 0) { last_feature_loses_point(last, i); continue; }
    last.point[i] = q;
    if (q > last_max) last_max = q;
  }
  if (last_max >= 0) atomicMax(&s_last_max, last_max);
  // ---- the rows of the points move down in place (see above: read, barrier, write, chunk by chunk upwards).  From here on
  // nothing reads pt_unlinked.
  for (int base = 0; base < P; base += nt) {                                     // block-uniform
    const int p = base + t;
    const int q = p < P ? mark[p] : -1;
    double x = 0.0, y = 0.0, z = 0.0;
    int ty = 0, nf = 0, ns = 0;
    if (q >= 0) {
      x = pt_pos[3 * (size_t)p]; y = pt_pos[3 * (size_t)p + 1]; z = pt_pos[3 * (size_t)p + 2];
      ty = m.pt_type[p]; nf = m.pt_n_failed[p]; ns = m.pt_n_succeeded[p];
    }
    __syncthreads();
    if (q >= 0) {
      pt_pos[3 * (size_t)q] = x; pt_pos[3 * (size_t)q + 1] = y; pt_pos[3 * (size_t)q + 2] = z;
      m.pt_type[q] = ty; m.pt_n_failed[q] = nf; m.pt_n_succeeded[q] = ns;
      m.pt_unlinked[q] = 0;
    }
  }
  __syncthreads();
  if (t == 0) {
    sc.out[0] = N;
    sc.out[1] = sc.ftr_scan[n_ftr];
    sc.out[2] = g.pt_obs_offset[N];
    sc.out[3] = sc.cand_scan[m.n_candidates];
    sc.out[4] = s_last_max;
  }
}
}  // namespace
