// svo_track_chain.h -- the kernels of one tracked frame: Reprojector::reprojectMap as plan and replay around the matcher's batch,
// the hand-over of the new frame, and the workgroup scan / compaction helpers every tracker kernel uses.
#pragma once
#include "svo_track_types.h"
namespace {
// Frame::isVisible (S/frame.cpp:162-172)
SVO_DEV bool frame_is_visible(const Cam& cam, const double* T_f_w, const double* xyz_w) {
  double xyz_f[3], px[2];
  se3_act(T_f_w, xyz_w, xyz_f);
  if (xyz_f[2] < 0.0) return false;
  world2cam(cam, xyz_f, px);
  return px[0] >= 0.0 && px[1] >= 0.0 && px[0] < cam.width && px[1] < cam.height;
}

// v.normalize() of Eigen 3.4: divide by the norm when the squared norm is positive
SVO_DEV void normalize3(double* v) {
  const double n2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
  if (n2 > 0.0) { const double nn = sqrt(n2); v[0] = v[0] / nn; v[1] = v[1] / nn; v[2] = v[2] / nn; }
}

// Point::getCloseViewObs (S/point.cpp:101-125): the observation whose viewing direction is closest to the frame's (first
// maximum of the cosine above zero, else the first observation); false when the angle exceeds 60 degrees
SVO_DEV bool close_view_obs(const TrkMap& m, int p, const double* framepos, const double (*kf_pos)[3], int* obs_out) {
  const double* pos = m.pt_pos + 3 * (size_t)p;
  double od[3] = {framepos[0] - pos[0], framepos[1] - pos[1], framepos[2] - pos[2]};
  normalize3(od);
  const int o0 = m.pt_obs_offset[p], o1 = m.pt_obs_offset[p + 1];
  int min_it = o0;
  double min_cos_angle = 0;
  for (int ob = o0; ob < o1; ob += 4) {                                      // the keyframe indices of four observations at once
    int kf[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) kf[e] = ob + e < o1 ? m.obs_kf[ob + e] : -1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (kf[e] < 0) continue;
      double d[3] = {kf_pos[kf[e]][0] - pos[0], kf_pos[kf[e]][1] - pos[1], kf_pos[kf[e]][2] - pos[2]};   // (*it)->frame->pos() - pos_
      normalize3(d);
      const double cos_angle = od[0] * d[0] + od[1] * d[1] + od[2] * d[2];
      if (cos_angle > min_cos_angle) { min_cos_angle = cos_angle; min_it = ob + e; }
    }
  }
  *obs_out = min_it;
  return !(min_cos_angle < 0.5);
}

// exclusive scan of v[0..n) in place by one workgroup, total -> v[n]; s_part: blockDim.x ints of LDS (64 used).
// Thread t owns a contiguous chunk; the thread sums are scanned inside each wave with lane shifts and across the waves
// through LDS: two barriers (a log-step scan over all 1024 threads took twenty).
SVO_DEV void block_exclusive_scan(int* v, int n, int* s_part) {
  const int t = threadIdx.x, nt = blockDim.x;
  const int lane = t & 63, wave = t >> 6, n_waves = nt >> 6;
  const int chunk = (n + nt - 1) / nt;
  const int lo = min(n, t * chunk), hi = min(n, lo + chunk);
  int sum = 0;
  for (int i = lo; i < hi; ++i) sum += v[i];
  int incl = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) s_part[wave] = incl;
  __syncthreads();
  int before = 0;
  for (int w = 0; w < wave; ++w) before += s_part[w];
  int run = before + incl - sum;                          // exclusive prefix of this thread's chunk
  for (int i = lo; i < hi; ++i) { const int c = v[i]; v[i] = run; run += c; }
  if (t == nt - 1) v[n] = before + incl;
  __syncthreads();
  (void)n_waves;
}

// ordered compaction by one workgroup: the elements i of [0, n) with keep(i) get the ranks 0, 1, ... in ascending i, and
// put(rank, i) is called once for each of them, by the thread that owns i.  scan: n + 1 ints of scratch; scan[n] = how many
// were kept.  keep is evaluated twice, before and after the scan.  Block-uniform call with three barriers inside (one behind
// the flags, two in the scan; the last one is behind scan[n], not behind the calls of put).
template <typename Keep, typename Put>
SVO_DEV void block_compact(int n, int* scan, int* s_part, Keep keep, Put put) {
  const int t = threadIdx.x, nt = blockDim.x;
  for (int i = t; i < n; i += nt) scan[i] = keep(i) ? 1 : 0;
  __syncthreads();
  block_exclusive_scan(scan, n, s_part);
  for (int i = t; i < n; i += nt)
    if (keep(i)) put(scan[i], i);
}

// ---- Reprojector::reprojectMap up to the cell loop (S/reprojector.cpp:72-146) + the per-candidate choice of the reference
// feature (Point::getCloseViewObs, the first statement of Matcher::findMatchDirect).  One workgroup.
SVO_DEV void trk_plan_body(const TrkMap& m, const TrkPlan& pl, MdFrame mf, const double* __restrict__ T_slot_w,
                           SeedRec* __restrict__ recs, const FrameState* __restrict__ sia_state) {
  const Cam cam = mf.cam;
  __shared__ int s_part[TRK_THREADS];
  __shared__ int s_sel[TRK_MAX_SEL], s_seq_base[TRK_MAX_SEL + 1], s_ftr_off[TRK_MAX_SEL], s_ftr_cnt[TRK_MAX_SEL];
  __shared__ int s_n_close, s_n_sel, s_n_kept, s_overflow, s_changed;
  __shared__ int s_overlap[TRK_MAX_SEL];
  __shared__ double s_T[7], s_framepos[3];
  // per-keyframe scratch, and -- for frames and grids that fit (block-uniform choice) -- the cell counters and the sort keys
  // in segment order: what one phase writes and the next one reads costs an LDS access instead of a trip to L2
  __shared__ int s_kf_close[TRK_LDS_KF];
  __shared__ double s_kf_dist[TRK_LDS_KF], s_kf_pos[TRK_LDS_KF][3];
  __shared__ int s_cell_count[TRK_LDS_CELLS + 1], s_cell_fill[TRK_LDS_CELLS];
  __shared__ unsigned long long s_seg_key[TRK_LDS_ITEMS];
  const int t = threadIdx.x, nt = blockDim.x;
  int* const cell_count = pl.n_cells <= TRK_LDS_CELLS ? s_cell_count : pl.cell_count;
  int* const cell_fill = pl.n_cells <= TRK_LDS_CELLS ? s_cell_fill : pl.cell_fill;
  if (t < 7) s_T[t] = sia_state->T_cur_w[t];
  if (t == 0) { s_n_close = 0; s_n_kept = 0; s_overflow = 0; s_changed = 0; }
  if (t < TRK_MAX_SEL) { s_sel[t] = -1; s_overlap[t] = 0; }
  __syncthreads();
  double T[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) { T[k] = s_T[k]; mf.T_cur_w[k] = s_T[k]; }
  if (t == 0) {
    double Tinv[7];
    se3_inverse(T, Tinv);                                                  // cur_frame.pos()
    s_framepos[0] = Tinv[0]; s_framepos[1] = Tinv[1]; s_framepos[2] = Tinv[2];
  }
  // ---- Map::getCloseKeyframes (S/map.cpp:109-131): keyframes one of whose key points is visible in the frame
  for (int k = t; k < m.n_kf; k += nt) {
    int kp[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) kp[j] = m.kf_key_point[5 * k + j];
    bool close = false;
#pragma unroll
    for (int j = 0; j < 5; ++j)
      if (!close && kp[j] >= 0) close = frame_is_visible(cam, T, m.pt_pos + 3 * (size_t)kp[j]);
    const double* tk = m.T_kf_w + 7 * (size_t)k;
    double Tk[7], Tinv[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) Tk[i] = tk[i];
    const double dx = T[0] - Tk[0], dy = T[1] - Tk[1], dz = T[2] - Tk[2];
    s_kf_close[k] = close ? 1 : 0;
    s_kf_dist[k] = sqrt(dx * dx + dy * dy + dz * dz);                      // (translation_vec difference).norm()
    se3_inverse(Tk, Tinv);                                                 // Frame::pos() of the keyframe (Point::getCloseViewObs)
    s_kf_pos[k][0] = Tinv[0]; s_kf_pos[k][1] = Tinv[1]; s_kf_pos[k][2] = Tinv[2];
    if (close) atomicAdd(&s_n_close, 1);
  }
  for (int p = t; p < m.n_points; p += nt) pl.first_seq[p] = INT_MAX;
  for (int c = t; c <= pl.n_cells; c += nt) cell_count[c] = 0;
  for (int c = t; c < pl.n_cells; c += nt) cell_fill[c] = 0;
  __syncthreads();
  // ---- close_kfs.sort by distance (stable: std::list::sort), the first max_n_kfs of them (:82-88)
  for (int k = t; k < m.n_kf; k += nt) {
    if (!s_kf_close[k]) continue;
    const double dk = s_kf_dist[k];
    int rank = 0;
    for (int j = 0; j < m.n_kf; ++j)
      if (s_kf_close[j] && (s_kf_dist[j] < dk || (!(dk < s_kf_dist[j]) && j < k))) ++rank;
    if (rank < pl.max_n_kfs) s_sel[rank] = k;
  }
  __syncthreads();
  if (t < TRK_MAX_SEL) {                                                    // the selected keyframes' feature ranges, all at once
    const int n_sel = s_n_close < pl.max_n_kfs ? s_n_close : pl.max_n_kfs;
    if (t < n_sel) {
      const int off = m.kf_ftr_offset[s_sel[t]];
      s_ftr_off[t] = off;
      s_ftr_cnt[t] = m.kf_ftr_offset[s_sel[t] + 1] - off;
    }
  }
  __syncthreads();
  if (t == 0) {
    const int n_sel = s_n_close < pl.max_n_kfs ? s_n_close : pl.max_n_kfs;
    s_n_sel = n_sel;
    int base = 0;
    for (int r = 0; r < n_sel; ++r) { s_seq_base[r] = base; base += s_ftr_cnt[r]; }
    s_seq_base[n_sel] = base;
  }
  __syncthreads();
  const int n_sel = s_n_sel;
  const int m_kf = s_seq_base[n_sel];
  const int m_all = m_kf + m.n_candidates;
  // ---- a point is projected once: the first keyframe feature that refers to it (last_projected_kf_id_, :103-106)
  for (int q = t; q < m_kf; q += nt) {
    int r = 0;
    while (r + 1 < n_sel && q >= s_seq_base[r + 1]) ++r;
    const int p = m.kf_ftr_point[s_ftr_off[r] + (q - s_seq_base[r])];
    if (p >= 0 && !m.pt_unlinked[p]) atomicMin(&pl.first_seq[p], q);
  }
  __syncthreads();
  // ---- reprojectPoint (:246-259) for the keyframe points and the point candidates (:118-138)
  for (int q = t; q < m_all; q += nt) {
    int p, r = -1;
    if (q < m_kf) {
      r = 0;
      while (r + 1 < n_sel && q >= s_seq_base[r + 1]) ++r;
      p = m.kf_ftr_point[s_ftr_off[r] + (q - s_seq_base[r])];
      if (p < 0) continue;
      const int fs = pl.first_seq[p];                                        // (asked for together with the flag)
      if (m.pt_unlinked[p] || fs != q) continue;
    } else {
      p = m.cand_point[q - m_kf];
      if (p < 0 || m.pt_unlinked[p]) continue;
    }
    const int ptype = m.pt_type[p];                                          // (in flight during the projection)
    double xyz_f[3], px[2];
    se3_act(T, m.pt_pos + 3 * (size_t)p, xyz_f);
    world2cam(cam, xyz_f, px);                                             // frame->w2c(point->pos_)
    const int ix = (int)px[0], iy = (int)px[1];                            // px.cast<int>()
    const bool in = px[0] == px[0] && px[1] == px[1] && ix >= 8 && ix < cam.width - 8 && iy >= 8 && iy < cam.height - 8;   // isInFrame(., 8)
    if (in) {
      const int cell = (int)(px[1] / pl.grid_size) * pl.grid_cols + (int)(px[0] / pl.grid_size);
      const int idx = atomicAdd(&s_n_kept, 1);
      if (idx < pl.cap) {
        pl.item_point[idx] = p;
        pl.item_px[2 * idx] = px[0]; pl.item_px[2 * idx + 1] = px[1];
        pl.item_cell[idx] = cell;
        pl.item_key[idx] = ((unsigned long long)(3 - ptype) << 32) | (unsigned)q;   // cell.sort: higher type first, stable
        atomicAdd(&cell_count[cell], 1);
      } else {
        s_overflow = 1;
      }
      if (r >= 0) atomicAdd(&s_overlap[r], 1);                             // overlap_kfs.back().second++ (:112-113)
    } else if (q >= m_kf) {
      // a candidate that is not in the frame (:126-135); the point sits in no cell, nobody else touches it
      const int nf = m.pt_n_failed[p] + 3;
      m.pt_n_failed[p] = nf;
      if (nf > 30) { m.pt_type[p] = TYPE_DELETED; m.pt_unlinked[p] = 1; s_changed = 1; }    // deleteCandidate + erase
    }
  }
  __syncthreads();
  const int n_kept = s_n_kept < pl.cap ? s_n_kept : pl.cap;
  unsigned long long* const seg_key = n_kept <= TRK_LDS_ITEMS ? s_seg_key : pl.seg_key;
  // ---- cell segments
  block_exclusive_scan(cell_count, pl.n_cells, s_part);                    // cell_count[c] = start of cell c, [n_cells] = total
  for (int c = t; c <= pl.n_cells; c += nt) pl.cell_offset[c] = cell_count[c];
  for (int i = t; i < n_kept; i += nt) {
    const int c = pl.item_cell[i];
    const unsigned long long key = pl.item_key[i];
    const int at = cell_count[c] + atomicAdd(&cell_fill[c], 1);
    pl.seg[at] = i;
    seg_key[at] = key;
  }
  __syncthreads();
  // ---- trial order inside the cell, and the reference feature of every candidate
  const double framepos[3] = {s_framepos[0], s_framepos[1], s_framepos[2]};
  for (int s = t; s < n_kept; s += nt) {
    const int i = pl.seg[s];
    const unsigned long long key = seg_key[s];
    const int c = pl.item_cell[i];
    const int p = pl.item_point[i];
    const double pxc[2] = {pl.item_px[2 * i], pl.item_px[2 * i + 1]};
    const int c0 = cell_count[c], c1 = cell_count[c + 1];
    int rank = 0;
    for (int j = c0; j < c1; ++j) rank += seg_key[j] < key ? 1 : 0;
    const int o = c0 + rank;
    const bool deleted = m.pt_type[p] == TYPE_DELETED;
    int obs = -1;
    bool view_ok = false;
    if (!deleted && m.pt_obs_offset[p + 1] > m.pt_obs_offset[p]) view_ok = close_view_obs(m, p, framepos, s_kf_pos, &obs);
    pl.cand_point[o] = p;
    pl.cand_obs[o] = view_ok ? obs : -1;
    pl.cand_deleted[o] = deleted ? 1 : 0;
    // the matcher's record of the candidate (Matcher::findMatchDirect up to the warp, svo_match_device.h): formed here,
    // read by the warp / alignment stages and by the replay
    if (view_ok) {
      pl.cand_level_ref[o] = m.obs_level[obs];
      recs[o] = md_geometry_item(mf, T_slot_w, m.kf_slot[m.obs_kf[obs]], m.obs_level[obs], m.obs_px + 2 * (size_t)obs, m.obs_f + 3 * (size_t)obs,
                                 m.pt_pos + 3 * (size_t)p, m.obs_edgelet[obs] != 0, m.obs_grad + 2 * (size_t)obs, pxc);
    } else {
      // a deleted point is erased from its cell (:190-194), a point without a close view fails the match at once (matcher.cpp:161-162)
      pl.cand_level_ref[o] = 0;
      SeedRec rc = md_dead_record();
      rc.uv0[0] = pxc[0]; rc.uv0[1] = pxc[1];
      recs[o] = rc;
    }
  }
  if (t == 0) {
    pl.counters[0] = n_kept;
    pl.counters[1] = s_overflow;
    pl.counters[2] = s_changed;
    pl.counters[3] = n_sel;
  }
  if (t < TRK_MAX_SEL) { pl.overlap_kf[t] = t < n_sel ? s_sel[t] : -1; pl.overlap_count[t] = t < n_sel ? s_overlap[t] : 0; }
}

// ---- the cell loop of Reprojector::reprojectMap (S/reprojector.cpp:149-166) with reprojectCell (:180-241) replayed over
// the batch results: per cell the first successful candidate wins, the loop stops after the cell that takes n_matches
// beyond max_fts; point bookkeeping (:202-215), the frame's new features (:217-231) and the inputs of the pose refinement.
SVO_DEV void trk_replay_body(const TrkMap& m, const TrkPlan& pl, const TrkFeat& ft, const Cam& cam, const FrameState* __restrict__ sia_state,
                             const SeedRec* __restrict__ recs, int* __restrict__ cell_winner,
                             int* __restrict__ cell_cum, int max_fts, int quality_min_fts) {
  __shared__ int s_part[TRK_THREADS];
  __shared__ int s_cut, s_changed;
  __shared__ unsigned long long s_trials;
  const int t = threadIdx.x, nt = blockDim.x;
  const int n_cells = pl.n_cells;
  if (t == 0) { s_cut = n_cells - 1; s_changed = pl.counters[2]; s_trials = 0ull; }
  // first success per cell
  for (int c = t; c < n_cells; c += nt) {
    int w = -1;
    for (int i = pl.cell_offset[c]; i < pl.cell_offset[c + 1] && w < 0; ++i)
      if (!pl.cand_deleted[i] && recs[i].path >= 0 && recs[i].matched) w = i;      // findMatchDirect returned true
    cell_winner[c] = w;
    cell_cum[c] = w >= 0 ? 1 : 0;
  }
  __syncthreads();
  block_exclusive_scan(cell_cum, n_cells, s_part);                          // cell_cum[c] = matches before cell c
  for (int c = t; c < n_cells; c += nt)
    if (cell_cum[c] + (cell_winner[c] >= 0 ? 1 : 0) > max_fts) atomicMin(&s_cut, c);     // n_matches_ > maxFts after this cell (:164-165)
  __syncthreads();
  const int cut = s_cut;
  double T[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) T[k] = sia_state->T_cur_w[k];
  unsigned long long my_trials = 0ull;
  for (int c = t; c <= cut && c < n_cells; c += nt) {
    const int w = cell_winner[c];
    const int end = w >= 0 ? w + 1 : pl.cell_offset[c + 1];
    for (int i = pl.cell_offset[c]; i < end; ++i) {
      ++my_trials;                                                          // ++n_trials_ (:188)
      if (pl.cand_deleted[i]) continue;                                     // TYPE_DELETED: erased from the cell (:190-194)
      const int p = pl.cand_point[i];
      if (i != w) {                                                         // :202-209
        const int nf = m.pt_n_failed[p] + 1;
        m.pt_n_failed[p] = nf;
        const int ty = m.pt_type[p];
        if ((ty == TYPE_UNKNOWN && nf > 15) || (ty == TYPE_CANDIDATE && nf > 30)) {   // safeDeletePoint / deleteCandidatePoint
          m.pt_type[p] = TYPE_DELETED; m.pt_unlinked[p] = 1; s_changed = 1;
        }
        continue;
      }
      const int ns = m.pt_n_succeeded[p] + 1;                               // :211-214
      m.pt_n_succeeded[p] = ns;
      if (m.pt_type[p] == TYPE_UNKNOWN && ns > 10) m.pt_type[p] = TYPE_GOOD;
      const int fi = cell_cum[c];                                           // creation order = cell order
      if (fi < ft.cap) {
        const SeedRec& rc = recs[i];
        const double u = rc.step[0], v = rc.step[1];                        // px_cur = px_scaled * (1 << search_level_) (matcher.cpp:200)
        const double* pp = m.pt_pos + 3 * (size_t)p;
        ft.px[2 * fi] = u; ft.px[2 * fi + 1] = v;
        double fv[3];
        cam2world(cam, u, v, fv);                                           // Feature(frame, px, level): f = cam2world(px) (I/feature.h:43-51)
        ft.f[3 * fi] = fv[0]; ft.f[3 * fi + 1] = fv[1]; ft.f[3 * fi + 2] = fv[2];
        ft.pos[3 * fi] = pp[0]; ft.pos[3 * fi + 1] = pp[1]; ft.pos[3 * fi + 2] = pp[2];
        ft.level[fi] = rc.search_level;
        ft.point[fi] = p;
        ft.has_point[fi] = 1;
        double g0 = 1.0, g1 = 0.0;
        const int obs = pl.cand_obs[i];
        const bool edge = m.obs_edgelet[obs] != 0;
        if (edge) {                                                         // grad = (A_cur_ref_ * ref_ftr_->grad).normalized() (:224-229)
          const double* Tr = m.T_kf_w + 7 * (size_t)m.obs_kf[obs];
          double T_ref_inv[7], T_cur_ref[7], A[4];
          se3_inverse(Tr, T_ref_inv);
          se3_mul(T, T_ref_inv, T_cur_ref);
          const double dx = T_ref_inv[0] - pp[0], dy = T_ref_inv[1] - pp[1], dz = T_ref_inv[2] - pp[2];
          get_warp_matrix_affine(cam, m.obs_px + 2 * (size_t)obs, m.obs_f + 3 * (size_t)obs, sqrt(dx * dx + dy * dy + dz * dz), T_cur_ref, m.obs_level[obs], A);
          const double gr0 = m.obs_grad[2 * (size_t)obs], gr1 = m.obs_grad[2 * (size_t)obs + 1];
          g0 = A[0] * gr0 + A[1] * gr1;
          g1 = A[2] * gr0 + A[3] * gr1;
          const double n2 = g0 * g0 + g1 * g1;
          if (n2 > 0.0) { const double nn = sqrt(n2); g0 = g0 / nn; g1 = g1 / nn; }
        }
        ft.edgelet[fi] = edge ? 1 : 0;
        ft.grad[2 * fi] = g0; ft.grad[2 * fi + 1] = g1;
      }
    }
  }
  if (my_trials) atomicAdd(&s_trials, my_trials);
  __syncthreads();
  if (t == 0) {
    const int last = cut < n_cells ? cut : n_cells - 1;
    int n_matches = n_cells > 0 ? cell_cum[last] + (cell_winner[last] >= 0 ? 1 : 0) : 0;
    const int n_feat = n_matches < ft.cap ? n_matches : ft.cap;
    pl.counters[2] = s_changed;
    pl.counters[4] = n_feat;
    // processFrame returns before the pose refinement when the reprojector matched too few points (:208-215)
    pl.counters[5] = n_matches < quality_min_fts ? 0 : n_feat;
    pl.counters[6] = (int)(s_trials & 0xffffffffull);
    pl.counters[7] = n_matches;
  }
}

// ---- last_frame_ = new_frame_ (frame_handler_mono.cpp:91) and the result block.  One workgroup.
SVO_DEV void trk_finish_body(const TrkMap& m, const TrkPlan& pl, const TrkFeat& ft, const TrkLast& last, const Cam& cam,
                             const FrameState* __restrict__ sia_state,
                             const svo_hip_pose_opt_result* __restrict__ po, svo_hip_track_result* __restrict__ res,
                             double* __restrict__ out_px, double* __restrict__ out_f, int* __restrict__ out_level,
                             int* __restrict__ out_point, uint8_t* __restrict__ out_edgelet, double* __restrict__ out_grad,
                             int* __restrict__ out_pt_type, int* __restrict__ out_pt_failed, int* __restrict__ out_pt_succeeded,
                             unsigned long long* __restrict__ done_flag, unsigned long long seq) {
  __shared__ double s_Tnew[7];
  const int t = threadIdx.x, nt = blockDim.x;
  const int n_feat = pl.counters[4];
  const int n_po = pl.counters[5];
  const bool refined = n_po > 0 && po->ran != 0;
  if (t == 0) {
    svo_hip_track_result r;
    for (int i = 0; i < 7; ++i) r.T_f_w_sia[i] = sia_state->T_cur_w[i];
    r.sia_n_tracked = sia_state->n_meas / 16;
    for (int i = 0; i < SVO_HIP_MAX_LEVELS; ++i) r.sia_iters[i] = sia_state->iters[i];
    r.sia_stop = sia_state->stop;
    r.n_features = n_feat;
    r.n_matches = (uint64_t)pl.counters[7];
    r.n_trials = (uint64_t)(unsigned)pl.counters[6];
    r.n_overlap = pl.counters[3];
    r.map_changed = pl.counters[2];
    for (int i = 0; i < 16; ++i) { r.overlap_kf[i] = i < TRK_MAX_SEL ? pl.overlap_kf[i] : -1; r.overlap_count[i] = i < TRK_MAX_SEL ? pl.overlap_count[i] : 0; }
    r.n_candidates = pl.counters[0];
    r.items_overflow = pl.counters[1];
    r.pose = *po;
    if (!refined) {                        // the reference did not reach / did not run the refinement: nothing of it is valid
      memset(&r.pose, 0, sizeof(r.pose));
      for (int i = 0; i < 7; ++i) r.pose.T_f_w[i] = sia_state->T_cur_w[i];
    }
    // new_frame_->T_f_w_ when processFrame hands the frame over: the refined pose, or -- too few matches (:211) -- the last frame's
    for (int i = 0; i < 7; ++i) { r.T_f_w[i] = n_po > 0 ? r.pose.T_f_w[i] : last.T_f_w[i]; s_Tnew[i] = r.T_f_w[i]; }
    *res = r;                              // (res lies in host memory: written, never read back here)
  }
  __syncthreads();
  for (int i = t; i < n_feat; i += nt) {
    const int p = ft.has_point[i] ? ft.point[i] : -1;                       // pose_optimizer.cpp:154-157: (*it)->point = NULL
    out_px[2 * i] = ft.px[2 * i]; out_px[2 * i + 1] = ft.px[2 * i + 1];
    out_f[3 * i] = ft.f[3 * i]; out_f[3 * i + 1] = ft.f[3 * i + 1]; out_f[3 * i + 2] = ft.f[3 * i + 2];
    out_level[i] = ft.level[i];
    out_point[i] = p;
    out_edgelet[i] = ft.edgelet[i];
    out_grad[2 * i] = ft.grad[2 * i]; out_grad[2 * i + 1] = ft.grad[2 * i + 1];
    last.px[2 * i] = ft.px[2 * i]; last.px[2 * i + 1] = ft.px[2 * i + 1];
    last.f[3 * i] = ft.f[3 * i]; last.f[3 * i + 1] = ft.f[3 * i + 1]; last.f[3 * i + 2] = ft.f[3 * i + 2];
    last.point[i] = p;
    if (i < last.sia_max_n) {          // the next SparseImgAlign::run walks this frame's features (sparse_img_align.cpp:116-118)
      last.sia_px[2 * i] = ft.px[2 * i]; last.sia_px[2 * i + 1] = ft.px[2 * i + 1];
      last.sia_f[3 * i] = ft.f[3 * i]; last.sia_f[3 * i + 1] = ft.f[3 * i + 1]; last.sia_f[3 * i + 2] = ft.f[3 * i + 2];
      last.sia_pos[3 * i] = ft.pos[3 * i]; last.sia_pos[3 * i + 1] = ft.pos[3 * i + 1]; last.sia_pos[3 * i + 2] = ft.pos[3 * i + 2];
      last.sia_has_point[i] = p >= 0 ? 1 : 0;
    }
  }
  for (int p = t; p < m.n_points; p += nt) {
    out_pt_type[p] = m.pt_type[p]; out_pt_failed[p] = m.pt_n_failed[p]; out_pt_succeeded[p] = m.pt_n_succeeded[p];
  }
  __syncthreads();
  if (t == 0) {
    *last.n = n_feat;
    FrameConst c;
    c.cam = cam;
    for (int i = 0; i < 7; ++i) { const double v = s_Tnew[i]; last.T_f_w[i] = v; c.T_ref_w[i] = v; c.T_cur_w_init[i] = v; }   // :175
    double Tinv[7];
    se3_inverse(c.T_ref_w, Tinv);                                            // Frame::pos()
    c.ref_pos[0] = Tinv[0]; c.ref_pos[1] = Tinv[1]; c.ref_pos[2] = Tinv[2];
    c.n_feat = n_feat < last.sia_max_n ? n_feat : last.sia_max_n; c.pad = 0;
    last.sia_fc[0] = c;
  }
  // the result block lies in page-locked host memory: once every thread's stores have left for the host, the frame's
  // sequence number goes after them and the waiting host thread reads the block
  __threadfence_system();
  __syncthreads();
  if (t == 0) __hip_atomic_store(done_flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- the kernels of the chain: workgroup c takes camera c's TrkCamArgs from a table in device memory (trk_track_all uploads it when it changes)
SVO_DEV void trk_plan_args(const TrkCamArgs& a) { trk_plan_body(a.m, a.pl, a.mf, a.T_slot_w, a.recs, a.sia_state); }
SVO_DEV void trk_replay_args(const TrkCamArgs& a, int max_fts, int quality_min_fts) {
  trk_replay_body(a.m, a.pl, a.ft, a.mf.cam, a.sia_state, a.recs, a.cell_winner, a.cell_cum, max_fts, quality_min_fts);
}
// seq: the frame's sequence number (every camera of the group advances with every call)
SVO_DEV void trk_finish_args(const TrkCamArgs& a, unsigned long long seq) {
  char* rd = a.res;
  int* pt = reinterpret_cast<int*>(rd + a.o_pt);
  trk_finish_body(a.m, a.pl, a.ft, a.last, a.mf.cam, a.sia_state, a.po, reinterpret_cast<svo_hip_track_result*>(rd),
                  reinterpret_cast<double*>(rd + a.o_px), reinterpret_cast<double*>(rd + a.o_f), reinterpret_cast<int*>(rd + a.o_level),
                  reinterpret_cast<int*>(rd + a.o_point), reinterpret_cast<uint8_t*>(rd + a.o_edge), reinterpret_cast<double*>(rd + a.o_grad),
                  pt, pt + a.m.n_points, pt + 2 * (size_t)a.m.n_points, reinterpret_cast<unsigned long long*>(rd + a.o_flag), seq);
}

__global__ __launch_bounds__(TRK_THREADS) void trk_plan_cams_kernel(const TrkCamArgs* __restrict__ args) { trk_plan_args(args[blockIdx.x]); }
__global__ __launch_bounds__(TRK_THREADS) void trk_replay_cams_kernel(const TrkCamArgs* __restrict__ args, int max_fts, int quality_min_fts) {
  trk_replay_args(args[blockIdx.x], max_fts, quality_min_fts);
}
__global__ __launch_bounds__(256) void trk_finish_cams_kernel(const TrkCamArgs* __restrict__ args, unsigned long long seq) {
  trk_finish_args(args[blockIdx.x], seq);
}
// ... over the cameras a list names (svo_hip_tracker_group_track_some): workgroup j takes camera cams[j]'s entry of the table ...
__global__ __launch_bounds__(TRK_THREADS) void trk_plan_listed_kernel(const TrkCamArgs* __restrict__ args, const int* __restrict__ cams) {
  trk_plan_args(args[cams[blockIdx.x]]);
}
__global__ __launch_bounds__(TRK_THREADS) void trk_replay_listed_kernel(const TrkCamArgs* __restrict__ args, const int* __restrict__ cams, int max_fts,
                                                                        int quality_min_fts) {
  trk_replay_args(args[cams[blockIdx.x]], max_fts, quality_min_fts);
}
__global__ __launch_bounds__(256) void trk_finish_listed_kernel(const TrkCamArgs* __restrict__ args, const int* __restrict__ cams, unsigned long long seq) {
  trk_finish_args(args[cams[blockIdx.x]], seq);
}
// ... and the same for a lone tracker with its one entry passed by value, not uploaded: the pointers inside a by-value kernel
// argument address global memory by the ABI, those read from the table are generic pointers, and every memory access of the
// bodies becomes a flat instruction (measured: the lone chain 3 us a frame slower through the table kernels)
__global__ __launch_bounds__(TRK_THREADS) void trk_plan_one_kernel(TrkCamArgs a) { trk_plan_args(a); }
__global__ __launch_bounds__(TRK_THREADS) void trk_replay_one_kernel(TrkCamArgs a, int max_fts, int quality_min_fts) {
  trk_replay_args(a, max_fts, quality_min_fts);
}
__global__ __launch_bounds__(256) void trk_finish_one_kernel(TrkCamArgs a, unsigned long long seq) { trk_finish_args(a, seq); }
}  // namespace
