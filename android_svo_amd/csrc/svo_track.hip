// svo_track.hip -- one tracked frame of FrameHandlerMono::processFrame (S/frame_handler_mono.cpp:171-229) as ONE chain of
// kernels on ONE stream with ONE synchronisation at the end:
//
//   new_frame->T_f_w_ = last_frame->T_f_w_                                   (:175)
//   SparseImgAlign(kltMaxLevel, kltMinLevel, 30, GaussNewton).run(last, new)  (:186-188)   svo_sia.hip, fused kernel
//   Reprojector::reprojectMap(new_frame, overlap_kfs)                         (:203)       trk_plan_cams_kernel -> Matcher::findMatchDirect
//                                                                                          batch (svo_depth.hip) -> trk_replay_cams_kernel
//   pose_optimizer::optimizeGaussNewton(...)                                  (:226-229)   svo_refine.hip
//   last_frame_ = new_frame_                                                  (frame_handler_mono.cpp:91)   trk_finish_cams_kernel
//
// A lone tracker is a group of one: the same launches serve one camera and the N cameras of svo_hip_tracker_group_track.
//
// What stays on the device between the stages: the pose SparseImgAlign leaves (read by the reprojection and by the pose
// refinement straight from the solver's record), the candidates of every grid cell, the matches, and -- across frames --
// the new frame's pyramid and features, which are the next call's reference frame.  The map the reprojector walks
// (keyframe poses / pyramids / feature lists / key points, points with their observation lists, point candidates) is a
// set of index tables the host uploads when the map changes (keyframe rate); the counters the reprojector keeps on the
// points (n_failed_reproj_, n_succeeded_reproj_, type promotions) are advanced on the device and returned with every
// frame.  A point the reprojector deletes changes the pointer graph (Map::safeDeletePoint clears feature references and
// re-selects key points): the device marks it unlinked, the keyframes that lost a key feature choose again before the next
// frame (trk_rekey_kernel), and map_changed tells the host to apply the same deletions to its own objects -- no new upload.
//
// The two serial policies of the reference are kept by construction, not approximated:
//   * cell lists are formed in the reference's push_back order (closest keyframe first, each keyframe's fts_ order, a
//     point only once: last_projected_kf_id_, then the point candidates) and stably ordered by point type
//     (cell.sort(pointQualityComparator)) -- every item gets its sequence number and a rank inside its cell;
//   * all candidates are matched in one batch, then "first success per cell wins, stop once n_matches exceeds maxFts" is
//     replayed over the results (Matcher::findMatchDirect is a pure function of its candidate).
#include <cfloat>
#include <climits>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "svo_internal.h"
#include "svo_match_device.h"
#include "svo_point_refine.h"

using namespace svo_dev;

namespace {

constexpr int TRK_THREADS = 1024;
constexpr int TRK_MAX_SEL = 16;            // >= Reprojector::Options::max_n_kfs
constexpr int TRK_MAX_STRUCT = 64;         // points per structure-optimisation call (Config::structureOptimMaxPts() = 20)
constexpr int TRK_LDS_KF = 256;            // keyframes of the map (svo_hip_tracker_config::max_keyframes <= this): per-keyframe scratch in LDS
constexpr int TRK_LDS_ITEMS = 2048;        // a frame with at most this many candidates keeps their per-cell sort keys in LDS
constexpr int TRK_LDS_CELLS = 2048;        // a grid with at most this many cells keeps the cell counters in LDS
constexpr int TYPE_DELETED = 0, TYPE_CANDIDATE = 1, TYPE_UNKNOWN = 2, TYPE_GOOD = 3;   // Point::PointType (I/point.h:33-38)

// the map as index tables (device pointers)
struct TrkMap {
  int n_kf, n_points, n_candidates;
  const double* T_kf_w;          // [n_kf][7]
  const int* kf_slot;            // [n_kf] pyramid slot
  const int* kf_key_point;       // [n_kf][5]
  const int* kf_ftr_offset;      // [n_kf + 1]
  const int* kf_ftr_point;
  const double* pt_pos;          // [n_points][3]
  int* pt_type;
  int* pt_n_failed;
  int* pt_n_succeeded;
  uint8_t* pt_unlinked;
  const int* pt_obs_offset;      // [n_points + 1]
  const int* obs_kf;
  const double* obs_px;
  const double* obs_f;
  const int* obs_level;
  const uint8_t* obs_edgelet;
  const double* obs_grad;
  const int* cand_point;
};

// The tables whose entries move when the map is rebuilt in place (a keyframe joins or leaves, the points are renumbered): the
// observation CSR, the keyframes' feature rows and the candidate list.  A tracker holds two such sets, each at the capacities of
// its configuration; a rebuild reads the current one (through TrkMap) and writes the other, which is the current one afterwards.
struct TrkTables {
  int* pt_obs_offset;            // [max_points + 1]
  int* obs_kf; double* obs_px; double* obs_f; int* obs_level; uint8_t* obs_edgelet; double* obs_grad;   // [max_obs] rows, as in TrkMap
  int* kf_ftr_offset;            // [max_keyframes + 1]
  int* kf_ftr_point;             // [max_kf_features]
  int* cand_point;               // [max_candidates]
};

// scratch of the rebuild kernels (one workgroup each), and what they report to the host
struct TrkScratch {
  int* cand_seed;                // [max_candidates] trk_promote_kernel: -2 stays, -1 promoted without a seed observation, else its seed keyframe
  int* cand_scan;                // [max_candidates + 1]
  int* ftr_scan;                 // [max_kf_features + 1]
  int* out;                      // [8]: 0 the call's own count, 1 n_ftr, 2 n_obs, 3 n_candidates afterwards (trk_rebuild_end), 4 the call's own
};

// scratch and outputs of the planning kernel; cap = capacity of the candidate arrays
struct TrkPlan {
  int cap, n_cells, grid_cols, grid_size, max_n_kfs;
  int* first_seq;                // [n_points]
  int* item_point;               // [cap] kept items in arrival order
  double* item_px;               // [cap][2]
  int* item_cell;                // [cap]
  unsigned long long* item_key;  // [cap]
  int* seg;                      // [cap]
  unsigned long long* seg_key;   // [cap] item_key in segment order (frames beyond TRK_LDS_ITEMS candidates)
  int* cell_count;               // [n_cells + 1]
  int* cell_fill;                // [n_cells]
  // outputs (the candidates of every cell in trial order)
  int* counters;                 // [8]: 0 n_cand, 1 overflow, 2 map_changed, 3 n_overlap, 4 n_features, 5 n_pose_opt, 6.. n_trials (64 bit)
  int* cell_offset;              // [n_cells + 1]
  int* overlap_kf;               // [TRK_MAX_SEL]
  int* overlap_count;            // [TRK_MAX_SEL]
  int* cand_point;               // [cap]
  int* cand_obs;                 // [cap] (-1: Point::getCloseViewObs failed)
  int* cand_level_ref;           // [cap] pyramid level of the reference feature (read by the warp stage)
  uint8_t* cand_deleted;         // [cap]
};

// the new frame's features (what Reprojector::reprojectCell adds to frame->fts_, in creation order) + pose-refinement inputs
struct TrkFeat {
  int cap;
  double* px;        // [cap][2]
  double* f;         // [cap][3]
  double* pos;       // [cap][3]
  int* level;        // [cap]
  int* point;        // [cap]
  uint8_t* edgelet;  // [cap]
  double* grad;      // [cap][2]
  uint8_t* has_point;   // [cap] in/out of the pose refinement
};

// the last frame (reference of the next SparseImgAlign)
struct TrkLast {
  int* n;            // [1]
  double* T_f_w;     // [7]
  double* px;        // [cap][2]
  double* f;         // [cap][3]
  int* point;        // [cap]
  // slot 0 of the SparseImgAlign solver: the hand-over kernel writes the next solve's inputs there directly
  FrameConst* sia_fc;
  double *sia_px, *sia_f, *sia_pos;
  uint8_t* sia_has_point;
  int sia_max_n;
};

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

// ---- FrameHandlerBase::optimizeStructure (S/frame_handler_base.cpp:190-210) on the points the host selected: Point::optimize
// of each of them over its observations as the map tables hold them (keyframe pose + bearing, Point::obs_ order), the new
// positions written into the point table, into the solver's copy of the last frame's points (the next SparseImgAlign::run reads
// point->pos_) and into the page-locked result block.  One workgroup.
struct TrkStructSel { int n; int point[TRK_MAX_STRUCT]; };
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
constexpr size_t ST_O_ITERS = TRK_MAX_STRUCT * 24, ST_O_FLAG = ST_O_ITERS + TRK_MAX_STRUCT * 4, ST_O_DECISION = ST_O_FLAG + 64;
constexpr size_t ST_BYTES = ST_O_DECISION + 128;
static_assert(sizeof(svo_hip_kf_decision) <= 128, "the decision fits its part of the block");
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

// ---- the kernels of the chain: workgroup c of a launch takes camera c's arguments from a table in device memory (a lone
// tracker is a group of one; trk_track_all uploads the table when it changes)
struct TrkCamArgs {
  TrkMap m;
  TrkPlan pl;
  TrkFeat ft;
  TrkLast last;
  MdFrame mf;
  const double* T_slot_w;
  SeedRec* recs;
  const FrameState* sia_state;
  int *cell_winner, *cell_cum;
  const svo_hip_pose_opt_result* po;
  char* res;                           // the camera's result block (device address of page-locked memory)
  size_t o_px, o_f, o_level, o_point, o_edge, o_grad, o_pt, o_flag;
};

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
// ... and the same for a lone tracker with its one entry passed by value, not uploaded: the pointers inside a by-value kernel
// argument address global memory by the ABI, those read from the table are generic pointers, and every memory access of the
// bodies becomes a flat instruction (measured: the lone chain 3 us a frame slower through the table kernels)
__global__ __launch_bounds__(TRK_THREADS) void trk_plan_one_kernel(TrkCamArgs a) { trk_plan_args(a); }
__global__ __launch_bounds__(TRK_THREADS) void trk_replay_one_kernel(TrkCamArgs a, int max_fts, int quality_min_fts) {
  trk_replay_args(a, max_fts, quality_min_fts);
}
__global__ __launch_bounds__(256) void trk_finish_one_kernel(TrkCamArgs a, unsigned long long seq) { trk_finish_args(a, seq); }

// svo_hip_tracker_group_finish_frames: workgroup c finishes camera c's frame.  The tables come from the chain's argument table, what
// changes with every call from a page-locked array the kernel reads directly (a camera that sits out: active == 0).
struct TrkFinishReq {
  TrkStructSel sel;
  int n_iter, active, overlap_valid, pad;
  char* st;                            // the camera's page-locked block (device address)
  unsigned long long seq;
};
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
constexpr int RELOC_THREADS = 256;
struct TrkRelocArgs {
  int kf, exclude, choose, apply, gate, use_last_pose, max_feat, pad;
  double T[7];
};
struct TrkRelocOut {
  double distance;               // of the chosen keyframe (choose)
  int kf;                        // the keyframe, -1: none
  int n_close;                   // close keyframes before the exclusion (choose)
  int n_feat;                    // its features (apply), -1: not counted
  int applied;                   // 1: the last frame is the keyframe now
  int max_point;                 // largest point index among the features, -1: none
  int pad;
};
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

// device memory for count elements, recorded in got (whose owner frees it); a no-op once *rc holds an error
template <typename T>
void trk_alloc(svo_hip_ctx* ctx, std::vector<void*>* got, int* rc, T** p, size_t count) {
  if (*rc != SVO_HIP_OK) return;
  void* d = nullptr;
  *rc = svo_hip_malloc(ctx, &d, (count ? count : 1) * sizeof(T));
  *p = (T*)d;
  if (*rc == SVO_HIP_OK) got->push_back(d);
}

}  // namespace

// What the cameras of a tracker group share (a lone tracker is a group of one): the pyramid batches, the SparseImgAlign solver
// (camera c = slot c), the arrays the batched stages index by camera with a fixed stride, and the page-locked image block.
struct svo_hip_tracker_shared {
  svo_hip_ctx* ctx = nullptr;
  int n_cams = 1;
  svo_hip_pyramid* kf_pyr = nullptr;        // n_cams x max_keyframes slots: camera c's keyframe slot s is slot c * max_keyframes + s
  svo_hip_pyramid* frame_pyr[2] = {nullptr, nullptr};   // n_cams slots each
  int last_idx = 0;                         // frame_pyr[last_idx] holds the cameras' last frames (they advance together)
  svo_hip_sia* sia = nullptr;               // batch n_cams
  uint8_t* img_host = nullptr;              // page-locked, mapped: n_cams images, img_stride apart
  uint8_t* img_dev = nullptr;
  size_t img_stride = 0;
  // [n_cams][...] arrays of the stages that run over all cameras at once
  int rec_stride = 0;                       // a camera's candidate records / levels: max_items rounded up to the 16 a block takes
  int* counters = nullptr;                  // [n_cams][8]
  int* cand_level_ref = nullptr;            // [n_cams][rec_stride]
  double *ft_f = nullptr, *ft_pos = nullptr;   // [n_cams][NF][3]
  int* ft_level = nullptr;                  // [n_cams][NF]
  uint8_t* ft_has_point = nullptr;          // [n_cams][NF]
  svo_hip_pose_opt_result* po = nullptr;    // [n_cams]
  // the argument table of the chain's kernels (TrkCamArgs per camera): built on the host every call, uploaded when it changed
  std::vector<TrkCamArgs> args_next;
  TrkCamArgs* args_host = nullptr;          // page-locked: the bytes of the last upload
  TrkCamArgs* args_dev = nullptr;
  bool args_valid = false;                  // args_dev holds args_host
  TrkFinishReq* fin_host = nullptr;         // page-locked, mapped: the cameras' requests of svo_hip_tracker_group_finish_frames
  TrkFinishReq* fin_dev = nullptr;
  unsigned long long seq = 0;               // frames tracked: the hand-over kernel stores it behind every camera's block (o_flag)
  std::vector<svo_hip_tracker*> members;
  std::vector<void*> dev_allocs;
};

struct svo_hip_tracker {
  svo_hip_ctx* ctx = nullptr;
  svo_hip_camera cam{};
  svo_hip_tracker_config cfg{};
  int n_cells = 0, grid_cols = 0, grid_rows = 0;
  svo_hip_tracker_shared* sh = nullptr;     // owned by the tracker itself (a lone tracker) or by its group
  bool owns_shared = false;
  int cam_index = 0;                        // this camera's slot in the shared solver / frame pyramids / per-camera arrays
  // map tables: the ones that are edited where they lie ...
  double *T_kf_w = nullptr, *T_slot_w = nullptr, *pt_pos = nullptr;
  int *kf_slot = nullptr, *kf_key_point = nullptr, *pt_type = nullptr, *pt_n_failed = nullptr, *pt_n_succeeded = nullptr;
  uint8_t* pt_unlinked = nullptr;
  // ... and the ones a rebuild (promotion, removal, renumbering) writes anew: tables[cur] is the map's set, the other one and
  // the kernels' scratch are allocated by whichever rebuild runs first (trk_rebuild_begin)
  TrkTables tables[2]{};
  int cur = 0;
  TrkScratch scratch{};
  bool have_second = false;
  int n_kf = 0, n_points = 0, n_candidates = 0;
  int n_ftr = 0, n_obs = 0;                 // entries of kf_ftr_point / of the observation tables
  std::vector<int> kf_slot_host;            // kf_slot as the device holds it (svo_hip_tracker_promote_last_frame checks against it)
  int track_n_points = 0;                   // n_points when the last frame was tracked: the layout of the counters in the result block
  bool have_map = false, have_last = false;
  bool overlap_valid = false;               // pl.overlap_kf / counters[3] are the last frame's and still name keyframes of the map (svo_hip_tracker_finish_frame)
  bool rekey_pending = false;               // the last frame deleted points: keyframes that lost a key feature choose again before the next frame
  int last_n_host = 0;
  int last_max_point = -1;                  // largest map point index the last frame's features refer to (set_last_frame input)
  bool last_from_track = false;             // ... or: the last frame is the previous call's new frame, its features are in the result block
  bool last_renumbered = false;             // ... whose point indices a compaction has outdated since: last_max_point holds the bound again
  // plan / replay scratch
  TrkPlan pl{};
  TrkFeat ft{};
  TrkLast last{};
  int *cell_winner = nullptr, *cell_cum = nullptr;
  bool need_gather = true;                  // the solver's slot 0 does not hold the last frame yet (a host upload came in between)
  bool any_edgelet = false;                 // the map holds EDGELET reference features (align1D stage needed)
  svo_hip_pose_opt_result* po = nullptr;    // (its entry of the shared array)
  TrkRelocOut* reloc_out = nullptr;         // what trk_reloc_kernel reports
  // result block: [svo_hip_track_result][px][f][level][point][edgelet][grad][pt_type][pt_failed][pt_succeeded]
  char* res_dev = nullptr;                  // device address of res_host
  char* res_host = nullptr;                 // page-locked, mapped into the device: the hand-over kernel writes it directly
  size_t o_flag = 0;
  uint8_t* img_dev = nullptr;               // device address of img_host (this camera's part of the shared image block)
  char* st_host = nullptr;                  // page-locked result of svo_hip_tracker_optimize_structure / _finish_frame: [pos 64 x 3][iters 64][flag][decision]
  char* st_dev = nullptr;
  unsigned long long st_seq = 0;
  size_t o_px = 0, o_f = 0, o_level = 0, o_point = 0, o_edge = 0, o_grad = 0, o_pt = 0, res_bytes = 0;
  // page-locked staging: one frame image (inside the shared block), the map tables
  uint8_t* img_host = nullptr;
  char* map_host = nullptr;
  size_t map_host_bytes = 0;
  std::vector<void*> dev_allocs;
};

namespace {

TrkMap make_map(const svo_hip_tracker* t) {
  TrkMap m;
  memset(&m, 0, sizeof(m));                 // (no stray padding bytes: trk_track_all compares argument tables byte by byte)
  m.n_kf = t->n_kf; m.n_points = t->n_points; m.n_candidates = t->n_candidates;
  m.T_kf_w = t->T_kf_w; m.kf_slot = t->kf_slot; m.kf_key_point = t->kf_key_point; m.pt_pos = t->pt_pos; m.pt_type = t->pt_type;
  m.pt_n_failed = t->pt_n_failed; m.pt_n_succeeded = t->pt_n_succeeded; m.pt_unlinked = t->pt_unlinked;
  const TrkTables& tb = t->tables[t->cur];
  m.kf_ftr_offset = tb.kf_ftr_offset; m.kf_ftr_point = tb.kf_ftr_point; m.pt_obs_offset = tb.pt_obs_offset; m.obs_kf = tb.obs_kf;
  m.obs_px = tb.obs_px; m.obs_f = tb.obs_f; m.obs_level = tb.obs_level; m.obs_edgelet = tb.obs_edgelet; m.obs_grad = tb.obs_grad;
  m.cand_point = tb.cand_point;
  return m;
}

// a set of tables at the capacities of the configuration (the one place that states them); what was allocated is appended to
// got, also when a later allocation fails.  kf_ftr_offset: max_keyframes + 1 entries hold the largest index a kernel writes --
// the total of trk_promote_kernel's scan over n_kf + 1 <= max_keyframes rows, trk_compact_kernel's entry n_kf.
int trk_tables_alloc(svo_hip_ctx* ctx, const svo_hip_tracker_config& c, TrkTables* tb, std::vector<void*>* got) {
  int rc = SVO_HIP_OK;
  auto D = [&](auto** p, size_t count) { trk_alloc(ctx, got, &rc, p, count); };
  const size_t K = c.max_keyframes, P = c.max_points, O = c.max_obs, F = c.max_kf_features, CN = c.max_candidates > 0 ? c.max_candidates : 1;
  D(&tb->pt_obs_offset, P + 1); D(&tb->obs_kf, O); D(&tb->obs_px, O * 2); D(&tb->obs_f, O * 3); D(&tb->obs_level, O); D(&tb->obs_edgelet, O);
  D(&tb->obs_grad, O * 2); D(&tb->kf_ftr_offset, K + 1); D(&tb->kf_ftr_point, F); D(&tb->cand_point, CN);
  return rc;
}

// the pending re-selection of key points (the last frame deleted points), before anything reads or extends the feature rows
int trk_rekey_now(svo_hip_tracker* t) {
  svo_hip_ctx* ctx = t->ctx;
  if (t->rekey_pending && t->n_kf > 0) {
    hipLaunchKernelGGL(trk_rekey_kernel, dim3(t->n_kf), dim3(KEY_THREADS), 0, ctx->stream, make_map(t), t->kf_key_point, svo_make_cam(t->cam));
    SVO_CHECK_HIP(ctx, hipGetLastError());
  }
  t->rekey_pending = false;
  return SVO_HIP_OK;
}

// What a promotion, a removal and a renumbering have in common around their launch.  Before it: the map has to be there, then
// the caller's own checks (a refused call changes nothing and enqueues nothing); the second table set and the scratch exist
// from the first rebuild on; the re-selection owed to the last frame's deletions sees the rows as they were.
template <typename Checks>
int trk_rebuild_begin(svo_hip_tracker* t, const char* who, Checks own_checks) {
  svo_hip_ctx* ctx = t->ctx;
  if (!t->have_map) return svo_fail(ctx, SVO_HIP_ERR_STATE, who, "no map has been set");
  int rc = own_checks();
  if (rc != SVO_HIP_OK) return rc;
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  if (!t->have_second) {
    const size_t F = t->cfg.max_kf_features, CN = t->cfg.max_candidates > 0 ? t->cfg.max_candidates : 1;
    TrkTables tb{};
    TrkScratch sc{};
    std::vector<void*> got;
    rc = trk_tables_alloc(ctx, t->cfg, &tb, &got);
    auto D = [&](int** p, size_t count) { trk_alloc(ctx, &got, &rc, p, count); };
    D(&sc.cand_seed, CN); D(&sc.cand_scan, CN + 1); D(&sc.ftr_scan, F + 1); D(&sc.out, 8);
    if (rc != SVO_HIP_OK) { for (void* p : got) (void)hipFree(p); return rc; }
    t->dev_allocs.insert(t->dev_allocs.end(), got.begin(), got.end());
    t->tables[1 - t->cur] = tb; t->scratch = sc; t->have_second = true;
  }
  return trk_rekey_now(t);
}

// After it: the first n_out counts of the kernel come back (out[1..3]: the entries of the feature rows, of the observation
// tables and of the candidate list), and the set the kernel wrote is the map's from here on.
int trk_rebuild_end(svo_hip_tracker* t, int* out, int n_out) {
  svo_hip_ctx* ctx = t->ctx;
  SVO_CHECK_HIP(ctx, hipMemcpyAsync(out, t->scratch.out, (size_t)n_out * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  SVO_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  t->cur = 1 - t->cur;
  t->n_ftr = out[1]; t->n_obs = out[2]; t->n_candidates = out[3];
  return SVO_HIP_OK;
}

}  // namespace

extern "C" {

int svo_hip_tracker_default_config(svo_hip_tracker_config* c) {
  if (!c) return SVO_HIP_ERR_INVALID;
  memset(c, 0, sizeof(*c));
  c->max_keyframes = 64; c->max_points = 1 << 16; c->max_obs = 1 << 18; c->max_kf_features = 1 << 17; c->max_candidates = 1 << 14;
  c->max_items = 1 << 14; c->max_frame_features = 2048;
  c->n_levels = 5;                 // max(Config::nPyrLevels(), Config::kltMaxLevel() + 1) (frame.cpp:63)
  c->klt_max_level = 4; c->klt_min_level = 2; c->sia_n_iter = 30; c->sia_eps = 1e-6;       // config.cpp:62-63, frame_handler_mono.cpp:186-187
  c->grid_size = 20; c->max_fts = 1200; c->quality_min_fts = 40;                            // config.cpp:61,82,83
  c->reproj_max_n_kfs = 10;        // Reprojector::Options::max_n_kfs (I/reprojector.h:41)
  c->n_pyr_levels = 3; c->align_max_iter = 10;                                              // config.cpp:59, I/matcher.h:86
  c->pose_optim_thresh = 2.0; c->pose_optim_num_iter = 10;                                  // config.cpp:66-67
  return SVO_HIP_OK;
}

static void trk_shared_destroy(svo_hip_tracker_shared* sh) {
  if (!sh) return;
  if (sh->sia) svo_hip_sia_destroy(sh->sia);
  if (sh->kf_pyr) svo_hip_pyramid_destroy(sh->kf_pyr);
  for (int i = 0; i < 2; ++i) if (sh->frame_pyr[i]) svo_hip_pyramid_destroy(sh->frame_pyr[i]);
  for (void* p : sh->dev_allocs) if (p) (void)hipFree(p);
  if (sh->img_host) (void)hipHostFree(sh->img_host);
  if (sh->args_host) (void)hipHostFree(sh->args_host);
  if (sh->fin_host) (void)hipHostFree(sh->fin_host);
  delete sh;
}

// one camera's own objects (everything but what svo_hip_tracker_shared holds)
static void trk_member_destroy(svo_hip_tracker* t) {
  for (void* p : t->dev_allocs) if (p) (void)hipFree(p);
  if (t->res_host) (void)hipHostFree(t->res_host);
  if (t->st_host) (void)hipHostFree(t->st_host);
  if (t->map_host) (void)hipHostFree(t->map_host);
  delete t;
}

int svo_hip_tracker_destroy(svo_hip_tracker* t) {
  if (!t) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = t->ctx;
  if (t->sh && !t->owns_shared) return svo_fail(ctx, SVO_HIP_ERR_STATE, "svo_hip_tracker_destroy", "a camera of a tracker group goes with its group (svo_hip_tracker_group_destroy)");
  (void)hipStreamSynchronize(ctx->stream);
  svo_hip_tracker_shared* sh = t->sh;
  trk_member_destroy(t);
  trk_shared_destroy(sh);
  return SVO_HIP_OK;
}

static int trk_check_config(svo_hip_ctx* ctx, const svo_hip_camera* cam, const svo_hip_tracker_config* cfg) {
  SVO_REQUIRE(ctx, cfg->max_keyframes <= TRK_LDS_KF);
  SVO_REQUIRE(ctx, cfg->max_keyframes >= 1 && cfg->max_points >= 1 && cfg->max_obs >= 1 && cfg->max_kf_features >= 1 && cfg->max_candidates >= 0);
  SVO_REQUIRE(ctx, cfg->max_items >= 1 && cfg->max_frame_features >= 1 && cfg->max_frame_features <= 2816);
  // the cell loop stops AFTER the match that exceeds max_fts (reprojector.cpp:164-165): a frame can gain max_fts + 1 features
  SVO_REQUIRE(ctx, cfg->max_frame_features >= cfg->max_fts + 1);
  SVO_REQUIRE(ctx, cfg->n_levels >= 1 && cfg->n_levels <= SVO_HIP_MAX_LEVELS && cfg->klt_max_level < cfg->n_levels && cfg->klt_min_level >= 0 &&
                       cfg->klt_min_level <= cfg->klt_max_level && cfg->sia_n_iter >= 0);
  SVO_REQUIRE(ctx, cfg->grid_size >= 1 && cfg->max_fts >= 0 && cfg->reproj_max_n_kfs >= 1 && cfg->reproj_max_n_kfs <= TRK_MAX_SEL);
  SVO_REQUIRE(ctx, cfg->n_pyr_levels >= 1 && cfg->n_pyr_levels <= cfg->n_levels && cfg->align_max_iter >= 0 && cfg->pose_optim_num_iter >= 0);
  SVO_REQUIRE(ctx, cam->width > 16 && cam->height > 16);
  return SVO_HIP_OK;
}

// the shared part of n_cams cameras with one camera model and one configuration
static int trk_shared_create(svo_hip_ctx* ctx, const svo_hip_camera* cam, const svo_hip_tracker_config* cfg, int n_cams, svo_hip_tracker_shared** out) {
  *out = nullptr;
  svo_hip_tracker_shared* sh = new (std::nothrow) svo_hip_tracker_shared();
  if (!sh) return SVO_HIP_ERR_NOMEM;
  sh->ctx = ctx; sh->n_cams = n_cams;
  int rc = SVO_HIP_OK;
  auto A = [&](int r) { if (rc == SVO_HIP_OK) rc = r; };
  auto D = [&](auto** p, size_t count) { trk_alloc(ctx, &sh->dev_allocs, &rc, p, count); };
  A(svo_hip_pyramid_create(ctx, cam->width, cam->height, cfg->n_levels, n_cams * cfg->max_keyframes, &sh->kf_pyr));
  for (int i = 0; i < 2; ++i) A(svo_hip_pyramid_create(ctx, cam->width, cam->height, cfg->n_levels, n_cams, &sh->frame_pyr[i]));
  A(svo_hip_sia_create(ctx, n_cams, cfg->max_frame_features, &sh->sia));
  // (the library default, pinned here: the chain's decisions -- matches per cell, frame by frame -- equal the CPU chain's)
  if (rc == SVO_HIP_OK) rc = svo_hip_sia_set_option(sh->sia, SVO_HIP_SIA_OPT_ARITH, SVO_HIP_SIA_ARITH_EXACT);
  sh->rec_stride = (cfg->max_items + 15) / 16 * 16;
  const size_t N = (size_t)n_cams, NF = cfg->max_frame_features;
  D(&sh->counters, N * 8); D(&sh->cand_level_ref, N * sh->rec_stride);
  D(&sh->ft_f, N * NF * 3); D(&sh->ft_pos, N * NF * 3); D(&sh->ft_level, N * NF); D(&sh->ft_has_point, N * NF); D(&sh->po, N);
  sh->img_stride = ((size_t)cam->width * cam->height + 64 + 255) & ~(size_t)255;
  if (rc == SVO_HIP_OK && hipHostMalloc((void**)&sh->img_host, N * sh->img_stride, hipHostMallocMapped) != hipSuccess) rc = SVO_HIP_ERR_NOMEM;
  if (rc == SVO_HIP_OK && hipHostGetDevicePointer((void**)&sh->img_dev, sh->img_host, 0) != hipSuccess) rc = SVO_HIP_ERR_DEVICE;
  if (rc == SVO_HIP_OK && hipHostMalloc((void**)&sh->args_host, N * sizeof(TrkCamArgs), hipHostMallocDefault) != hipSuccess) rc = SVO_HIP_ERR_NOMEM;
  D(&sh->args_dev, N);
  if (rc == SVO_HIP_OK && hipHostMalloc((void**)&sh->fin_host, N * sizeof(TrkFinishReq), hipHostMallocMapped) != hipSuccess) rc = SVO_HIP_ERR_NOMEM;
  if (rc == SVO_HIP_OK && hipHostGetDevicePointer((void**)&sh->fin_dev, sh->fin_host, 0) != hipSuccess) rc = SVO_HIP_ERR_DEVICE;
  if (rc == SVO_HIP_OK) sh->args_next.resize(N);
  if (rc != SVO_HIP_OK) { trk_shared_destroy(sh); return rc; }
  *out = sh;
  return SVO_HIP_OK;
}

// camera `index` of the shared part: its own map tables, plan scratch, result block
static int trk_member_create(svo_hip_tracker_shared* sh, int index, const svo_hip_camera* cam, const svo_hip_tracker_config* cfg, svo_hip_tracker** out) {
  svo_hip_ctx* ctx = sh->ctx;
  *out = nullptr;
  svo_hip_tracker* t = new (std::nothrow) svo_hip_tracker();
  if (!t) return SVO_HIP_ERR_NOMEM;
  t->ctx = ctx; t->cam = *cam; t->cfg = *cfg; t->sh = sh; t->cam_index = index;
  t->grid_cols = (cam->width + cfg->grid_size - 1) / cfg->grid_size;        // ceil(width / cell_size) (reprojector.cpp:46-47)
  t->grid_rows = (cam->height + cfg->grid_size - 1) / cfg->grid_size;
  t->n_cells = t->grid_cols * t->grid_rows;
  int rc = SVO_HIP_OK;
  auto D = [&](auto** p, size_t count) { trk_alloc(ctx, &t->dev_allocs, &rc, p, count); };
  const size_t K = cfg->max_keyframes, P = cfg->max_points, O = cfg->max_obs, F = cfg->max_kf_features, CN = cfg->max_candidates > 0 ? cfg->max_candidates : 1;
  D(&t->T_kf_w, K * 7); D(&t->T_slot_w, K * 7); D(&t->kf_slot, K); D(&t->kf_key_point, K * 5);
  D(&t->pt_pos, P * 3); D(&t->pt_type, P); D(&t->pt_n_failed, P); D(&t->pt_n_succeeded, P); D(&t->pt_unlinked, P);
  if (rc == SVO_HIP_OK) rc = trk_tables_alloc(ctx, *cfg, &t->tables[0], &t->dev_allocs);
  TrkPlan& pl = t->pl;
  const size_t C = cfg->max_items, NC = t->n_cells;
  pl.cap = cfg->max_items; pl.n_cells = t->n_cells; pl.grid_cols = t->grid_cols; pl.grid_size = cfg->grid_size; pl.max_n_kfs = cfg->reproj_max_n_kfs;
  D(&pl.first_seq, P); D(&pl.item_point, C); D(&pl.item_px, C * 2); D(&pl.item_cell, C); D(&pl.item_key, C);
  D(&pl.seg, C); D(&pl.seg_key, C); D(&pl.cell_count, NC + 1); D(&pl.cell_fill, NC); D(&pl.cell_offset, NC + 1); D(&pl.overlap_kf, TRK_MAX_SEL);
  D(&pl.overlap_count, TRK_MAX_SEL); D(&pl.cand_point, C); D(&pl.cand_obs, C); D(&pl.cand_deleted, C);
  pl.counters = sh->counters + 8 * (size_t)index;                              // (per-camera entries of the shared arrays)
  pl.cand_level_ref = sh->cand_level_ref + sh->rec_stride * (size_t)index;
  D(&t->cell_winner, NC + 1); D(&t->cell_cum, NC + 1);
  t->po = sh->po + index;
  const size_t NF = cfg->max_frame_features;
  TrkFeat& ft = t->ft;
  ft.cap = cfg->max_frame_features;
  D(&ft.px, NF * 2); D(&ft.point, NF); D(&ft.edgelet, NF); D(&ft.grad, NF * 2);
  ft.f = sh->ft_f + 3 * NF * (size_t)index; ft.pos = sh->ft_pos + 3 * NF * (size_t)index;
  ft.level = sh->ft_level + NF * (size_t)index; ft.has_point = sh->ft_has_point + NF * (size_t)index;
  D(&t->last.n, 1); D(&t->last.T_f_w, 7); D(&t->last.px, NF * 2); D(&t->last.f, NF * 3); D(&t->last.point, NF);
  D(&t->reloc_out, 1);
  // result block
  auto al = [](size_t v) { return (v + 15) & ~(size_t)15; };
  t->o_px = al(sizeof(svo_hip_track_result)); t->o_f = al(t->o_px + NF * 16); t->o_level = al(t->o_f + NF * 24); t->o_point = al(t->o_level + NF * 4);
  t->o_edge = al(t->o_point + NF * 4); t->o_grad = al(t->o_edge + NF); t->o_pt = al(t->o_grad + NF * 16); t->o_flag = al(t->o_pt + P * 12);
  t->res_bytes = t->o_flag + 64;
  if (rc == SVO_HIP_OK && hipHostMalloc((void**)&t->res_host, t->res_bytes, hipHostMallocMapped) != hipSuccess) rc = SVO_HIP_ERR_NOMEM;
  if (rc == SVO_HIP_OK && hipHostGetDevicePointer((void**)&t->res_dev, t->res_host, 0) != hipSuccess) rc = SVO_HIP_ERR_DEVICE;
  if (rc == SVO_HIP_OK) memset(t->res_host, 0, t->res_bytes);
  t->img_host = sh->img_host + sh->img_stride * (size_t)index;
  t->img_dev = sh->img_dev + sh->img_stride * (size_t)index;
  const size_t st_bytes = ST_BYTES;
  if (rc == SVO_HIP_OK && hipHostMalloc((void**)&t->st_host, st_bytes, hipHostMallocMapped) != hipSuccess) rc = SVO_HIP_ERR_NOMEM;
  if (rc == SVO_HIP_OK) memset(t->st_host, 0, st_bytes);
  if (rc == SVO_HIP_OK && hipHostGetDevicePointer((void**)&t->st_dev, t->st_host, 0) != hipSuccess) rc = SVO_HIP_ERR_DEVICE;
  // staging area of svo_hip_tracker_set_map: every table at its capacity (T_kf_w and T_slot_w: two pose tables), 16 bytes of
  // alignment slack per table
  t->map_host_bytes = K * (56 + 56 + 4 + 20 + 4) + 8 + F * 4 + P * (24 + 12 + 4) + 8 + O * (4 + 16 + 24 + 4 + 1 + 16) + CN * 4 + 32 * 16;
  if (rc == SVO_HIP_OK && hipHostMalloc((void**)&t->map_host, t->map_host_bytes, hipHostMallocDefault) != hipSuccess) rc = SVO_HIP_ERR_NOMEM;
  if (rc != SVO_HIP_OK) { trk_member_destroy(t); return rc; }
  (void)hipMemsetAsync(t->last.n, 0, sizeof(int), ctx->stream);
  svo_sia_slot_arrays(sh->sia, index, &t->last.sia_fc, &t->last.sia_px, &t->last.sia_f, &t->last.sia_pos, &t->last.sia_has_point, &t->last.sia_max_n);
  *out = t;
  return SVO_HIP_OK;
}

int svo_hip_tracker_create(svo_hip_ctx* ctx, const svo_hip_camera* cam, const svo_hip_tracker_config* cfg, svo_hip_tracker** out) {
  if (!ctx || !cam || !cfg || !out) return SVO_HIP_ERR_INVALID;
  *out = nullptr;
  int rc = trk_check_config(ctx, cam, cfg);
  if (rc != SVO_HIP_OK) return rc;
  svo_hip_tracker_shared* sh = nullptr;
  rc = trk_shared_create(ctx, cam, cfg, 1, &sh);
  if (rc != SVO_HIP_OK) return rc;
  svo_hip_tracker* t = nullptr;
  rc = trk_member_create(sh, 0, cam, cfg, &t);
  if (rc != SVO_HIP_OK) { trk_shared_destroy(sh); return rc; }
  t->owns_shared = true;
  sh->members.push_back(t);
  *out = t;
  return SVO_HIP_OK;
}

int svo_hip_tracker_upload_keyframe(svo_hip_tracker* t, int slot, const uint8_t* level0) {
  if (!t || !level0) return SVO_HIP_ERR_INVALID;
  SVO_REQUIRE(t->ctx, slot >= 0 && slot < t->cfg.max_keyframes);
  return svo_hip_pyramid_upload_level0_and_build(t->sh->kf_pyr, t->cam_index * t->cfg.max_keyframes + slot, level0);
}

int svo_hip_tracker_keyframe_from_last_frame(svo_hip_tracker* t, int slot) {
  if (!t) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = t->ctx;
  SVO_REQUIRE(ctx, slot >= 0 && slot < t->cfg.max_keyframes);
  if (!t->have_last) return svo_fail(ctx, SVO_HIP_ERR_STATE, "svo_hip_tracker_keyframe_from_last_frame", "no frame has been tracked or set yet");
  const svo_hip_pyramid* src = t->sh->frame_pyr[t->sh->last_idx];
  const svo_hip_pyramid* kf = t->sh->kf_pyr;
  return svo_hip_copy_d2d(ctx, kf->base + ((size_t)t->cam_index * t->cfg.max_keyframes + slot) * kf->pyr_bytes,
                          src->base + (size_t)t->cam_index * src->pyr_bytes, src->pyr_bytes);
}

int svo_hip_tracker_set_map(svo_hip_tracker* t, const svo_hip_tracker_map* mp) {
  if (!t || !mp) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = t->ctx;
  const svo_hip_tracker_config& c = t->cfg;
  SVO_REQUIRE(ctx, mp->n_kf >= 0 && mp->n_kf <= c.max_keyframes && mp->n_points >= 0 && mp->n_points <= c.max_points);
  SVO_REQUIRE(ctx, mp->n_candidates >= 0 && mp->n_candidates <= c.max_candidates);
  SVO_REQUIRE(ctx, mp->n_kf == 0 || (mp->kf_slot && mp->T_kf_w && mp->kf_key_point && mp->kf_ftr_offset));
  SVO_REQUIRE(ctx, mp->n_points == 0 || (mp->pt_pos && mp->pt_type && mp->pt_n_failed && mp->pt_n_succeeded && mp->pt_obs_offset));
  SVO_REQUIRE(ctx, mp->n_candidates == 0 || mp->cand_point);
  const int n_ftr = mp->n_kf > 0 ? mp->kf_ftr_offset[mp->n_kf] : 0;
  const int n_obs = mp->n_points > 0 ? mp->pt_obs_offset[mp->n_points] : 0;
  SVO_REQUIRE(ctx, n_ftr >= 0 && n_ftr <= c.max_kf_features && n_obs >= 0 && n_obs <= c.max_obs);
  SVO_REQUIRE(ctx, n_ftr == 0 || mp->kf_ftr_point);
  SVO_REQUIRE(ctx, n_obs == 0 || (mp->obs_kf && mp->obs_px && mp->obs_f && mp->obs_level));
  // every index the kernels follow is checked here, once, on the host
  for (int k = 0; k < mp->n_kf; ++k) {
    SVO_REQUIRE(ctx, mp->kf_slot[k] >= 0 && mp->kf_slot[k] < c.max_keyframes && mp->kf_ftr_offset[k] <= mp->kf_ftr_offset[k + 1] && mp->kf_ftr_offset[k] >= 0);
    for (int j = 0; j < 5; ++j) SVO_REQUIRE(ctx, mp->kf_key_point[5 * k + j] >= -1 && mp->kf_key_point[5 * k + j] < mp->n_points);
  }
  for (int j = 0; j < n_ftr; ++j) SVO_REQUIRE(ctx, mp->kf_ftr_point[j] >= -1 && mp->kf_ftr_point[j] < mp->n_points);
  for (int p = 0; p < mp->n_points; ++p) SVO_REQUIRE(ctx, mp->pt_obs_offset[p] >= 0 && mp->pt_obs_offset[p] <= mp->pt_obs_offset[p + 1] && mp->pt_type[p] >= 0 && mp->pt_type[p] <= 3);
  for (int o = 0; o < n_obs; ++o) SVO_REQUIRE(ctx, mp->obs_kf[o] >= 0 && mp->obs_kf[o] < mp->n_kf && mp->obs_level[o] >= 0 && mp->obs_level[o] < c.n_levels);
  for (int i = 0; i < mp->n_candidates; ++i) SVO_REQUIRE(ctx, mp->cand_point[i] >= -1 && mp->cand_point[i] < mp->n_points);
  {
    // what the tables below take in the staging area (each starts on a 16-byte boundary): checked before anything is written
    const size_t K_ = (size_t)mp->n_kf, P_ = (size_t)mp->n_points, O_ = (size_t)n_obs;
    const size_t need = K_ * (56 + 4 + 20) + (K_ + 1) * 4 + (size_t)n_ftr * 4 + P_ * (24 + 12) + (P_ + 1) * 4 + O_ * (4 + 16 + 24 + 4 + 1 + 16) +
                        (size_t)mp->n_candidates * 4 + (size_t)c.max_keyframes * 56 + 32 * 16;
    if (need > t->map_host_bytes) return svo_fail(ctx, SVO_HIP_ERR_NOMEM, "svo_hip_tracker_set_map", "staging area too small");
  }
  if (t->have_last) {                       // (after the checks: a refused map changes nothing)
    // the last frame's features keep referring to map points by index: a map with fewer points than the largest of them
    // needs svo_hip_tracker_set_last_frame again (the result block still holds the features of a tracked frame)
    int max_point = t->last_max_point;
    if (t->last_from_track && !t->last_renumbered) {
      const int32_t* fp = reinterpret_cast<const int32_t*>(t->res_host + t->o_point);
      max_point = -1;
      for (int i = 0; i < t->last_n_host; ++i) if (fp[i] > max_point) max_point = fp[i];
    }
    if (max_point >= mp->n_points) t->have_last = false;     // svo_hip_tracker_track will ask for svo_hip_tracker_set_last_frame
  }
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  // the staging area may still feed the copies of the previous upload
  SVO_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  char* hs = t->map_host;
  size_t off = 0;
  hipError_t e = hipSuccess;
  auto put = [&](void* dst, const void* src, size_t bytes) {
    if (!bytes || e != hipSuccess) return;
    off = (off + 15) & ~(size_t)15;
    memcpy(hs + off, src, bytes);
    e = hipMemcpyAsync(dst, hs + off, bytes, hipMemcpyHostToDevice, ctx->stream);
    off += bytes;
  };
  const size_t K = mp->n_kf, P = mp->n_points;
  const TrkTables& tb = t->tables[t->cur];
  put(t->T_kf_w, mp->T_kf_w, K * 56); put(t->kf_slot, mp->kf_slot, K * 4); put(t->kf_key_point, mp->kf_key_point, K * 20);
  if (K) put(tb.kf_ftr_offset, mp->kf_ftr_offset, (K + 1) * 4);
  put(tb.kf_ftr_point, mp->kf_ftr_point, (size_t)n_ftr * 4);
  put(t->pt_pos, mp->pt_pos, P * 24); put(t->pt_type, mp->pt_type, P * 4); put(t->pt_n_failed, mp->pt_n_failed, P * 4);
  put(t->pt_n_succeeded, mp->pt_n_succeeded, P * 4);
  if (P) put(tb.pt_obs_offset, mp->pt_obs_offset, (P + 1) * 4);
  put(tb.obs_kf, mp->obs_kf, (size_t)n_obs * 4); put(tb.obs_px, mp->obs_px, (size_t)n_obs * 16); put(tb.obs_f, mp->obs_f, (size_t)n_obs * 24);
  put(tb.obs_level, mp->obs_level, (size_t)n_obs * 4);
  put(tb.cand_point, mp->cand_point, (size_t)mp->n_candidates * 4);
  // T_slot_w: the keyframe poses indexed by pyramid slot (what the matcher's batch indexes)
  {
    off = (off + 15) & ~(size_t)15;
    double* ts = reinterpret_cast<double*>(hs + off);
    memset(ts, 0, (size_t)c.max_keyframes * 56);
    for (int s = 0; s < c.max_keyframes; ++s) ts[7 * s + 6] = 1.0;
    for (int k = 0; k < mp->n_kf; ++k) memcpy(ts + 7 * (size_t)mp->kf_slot[k], mp->T_kf_w + 7 * (size_t)k, 56);
    if (e == hipSuccess) e = hipMemcpyAsync(t->T_slot_w, ts, (size_t)c.max_keyframes * 56, hipMemcpyHostToDevice, ctx->stream);
    off += (size_t)c.max_keyframes * 56;
  }
  if (n_obs) {
    off = (off + 15) & ~(size_t)15;
    uint8_t* ed = reinterpret_cast<uint8_t*>(hs + off);
    if (mp->obs_edgelet) memcpy(ed, mp->obs_edgelet, (size_t)n_obs); else memset(ed, 0, (size_t)n_obs);
    if (e == hipSuccess) e = hipMemcpyAsync(tb.obs_edgelet, ed, (size_t)n_obs, hipMemcpyHostToDevice, ctx->stream);
    off += (size_t)n_obs;
    off = (off + 15) & ~(size_t)15;
    double* gr = reinterpret_cast<double*>(hs + off);
    if (mp->obs_grad) memcpy(gr, mp->obs_grad, (size_t)n_obs * 16);
    else for (int o = 0; o < n_obs; ++o) { gr[2 * o] = 1.0; gr[2 * o + 1] = 0.0; }
    if (e == hipSuccess) e = hipMemcpyAsync(tb.obs_grad, gr, (size_t)n_obs * 16, hipMemcpyHostToDevice, ctx->stream);
    off += (size_t)n_obs * 16;
  }
  if (e == hipSuccess && P) e = hipMemsetAsync(t->pt_unlinked, 0, P, ctx->stream);
  if (e != hipSuccess) return svo_fail(ctx, SVO_HIP_ERR_DEVICE, "svo_hip_tracker_set_map", hipGetErrorString(e));
  t->n_kf = mp->n_kf; t->n_points = mp->n_points; t->n_candidates = mp->n_candidates;
  t->n_ftr = n_ftr; t->n_obs = n_obs;
  t->kf_slot_host.assign(mp->kf_slot, mp->kf_slot + mp->n_kf);
  t->any_edgelet = false;
  if (mp->obs_edgelet) for (int o = 0; o < n_obs && !t->any_edgelet; ++o) t->any_edgelet = mp->obs_edgelet[o] != 0;
  t->have_map = true; t->rekey_pending = false;
  t->overlap_valid = false;                 // the keyframes may be others now
  t->need_gather = true;                    // point positions may have changed
  return SVO_HIP_OK;
}

int svo_hip_tracker_update_point_positions(svo_hip_tracker* t, int n, const int32_t* point, const double* pos) {
  if (!t) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = t->ctx;
  SVO_REQUIRE(ctx, n >= 0 && (n == 0 || (point && pos)));
  if (!t->have_map) return svo_fail(ctx, SVO_HIP_ERR_STATE, "svo_hip_tracker_update_point_positions", "no map has been set");
  if (n == 0) return SVO_HIP_OK;
  for (int i = 0; i < n; ++i) SVO_REQUIRE(ctx, point[i] >= 0 && point[i] < t->n_points);
  // [pos n x 3 doubles][index n ints] gathered in page-locked memory: one transfer, one scatter launch
  const size_t o_idx = (size_t)n * 24, bytes = o_idx + (size_t)n * 4;
  char* d = nullptr;
  char* hs = nullptr;
  int rc = svo_ctx_staging(ctx, bytes, &d);
  if (rc == SVO_HIP_OK) rc = svo_ctx_host_staging(ctx, bytes, &hs);
  if (rc != SVO_HIP_OK) return rc;
  SVO_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the staging area may still feed an earlier transfer
  memcpy(hs, pos, (size_t)n * 24);
  memcpy(hs + o_idx, point, (size_t)n * 4);
  SVO_CHECK_HIP(ctx, hipMemcpyAsync(d, hs, bytes, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(trk_scatter_positions_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, reinterpret_cast<const int*>(d + o_idx),
                     reinterpret_cast<const double*>(d), t->pt_pos);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  t->need_gather = true;                    // the solver's copy of the last frame's point positions is stale
  return SVO_HIP_OK;
}

int svo_hip_tracker_optimize_structure(svo_hip_tracker* t, int n, const int32_t* point, int n_iter, double* pos_out, int32_t* iters_out) {
  if (!t) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = t->ctx;
  SVO_REQUIRE(ctx, n >= 0 && n <= TRK_MAX_STRUCT && n_iter >= 0 && (n == 0 || (point && pos_out)));
  if (!t->have_map) return svo_fail(ctx, SVO_HIP_ERR_STATE, "svo_hip_tracker_optimize_structure", "no map has been set");
  if (n == 0) return SVO_HIP_OK;
  TrkStructSel sel;
  memset(&sel, 0, sizeof(sel));
  sel.n = n;
  for (int i = 0; i < n; ++i) {
    SVO_REQUIRE(ctx, point[i] >= 0 && point[i] < t->n_points);
    for (int j = 0; j < i; ++j) SVO_REQUIRE(ctx, point[j] != point[i]);         // a point is optimised once per call
    sel.point[i] = point[i];
  }
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t o_it = TRK_MAX_STRUCT * 24, o_flag = o_it + TRK_MAX_STRUCT * 4;
  const unsigned long long seq = ++t->st_seq;
  hipLaunchKernelGGL(trk_structure_kernel, dim3(1), dim3(256), 0, ctx->stream, make_map(t), t->pt_pos, t->last, sel, n_iter,
                     reinterpret_cast<double*>(t->st_dev), reinterpret_cast<int*>(t->st_dev + o_it),
                     reinterpret_cast<unsigned long long*>(t->st_dev + o_flag), seq);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  {
    volatile unsigned long long* flag = reinterpret_cast<volatile unsigned long long*>(t->st_host + o_flag);
    bool seen = false;
    for (long spins = 0; spins < 4000000L; ++spins) {
      if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) { seen = true; break; }
      __builtin_ia32_pause();
    }
    if (!seen) SVO_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != seq)
      return svo_fail(ctx, SVO_HIP_ERR_DEVICE, "svo_hip_tracker_optimize_structure", "the kernel did not complete");
  }
  memcpy(pos_out, t->st_host, (size_t)n * 24);
  if (iters_out) memcpy(iters_out, t->st_host + o_it, (size_t)n * 4);
  // (the point table and the solver's copy of the last frame's points were updated by the kernel: nothing to gather)
  return SVO_HIP_OK;
}

int svo_hip_tracker_set_last_frame(svo_hip_tracker* t, const uint8_t* level0, int kf_slot, const double T_f_w[7], int n, const double* px,
                                   const double* f, const int32_t* point) {
  if (!t || !T_f_w) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = t->ctx;
  SVO_REQUIRE(ctx, n >= 0 && n <= t->cfg.max_frame_features && (n == 0 || (px && f && point)));
  SVO_REQUIRE(ctx, level0 || (kf_slot >= 0 && kf_slot < t->cfg.max_keyframes));
  int max_point = -1;
  for (int i = 0; i < n; ++i) {                               // the alignment reads pt_pos[point]: every index is checked here
    SVO_REQUIRE(ctx, point[i] >= -1 && point[i] < (t->have_map ? t->n_points : 0));
    if (point[i] > max_point) max_point = point[i];
  }
  svo_hip_pyramid* dst = t->sh->frame_pyr[t->sh->last_idx];
  const svo_hip_pyramid* kf = t->sh->kf_pyr;
  int rc;
  if (level0) rc = svo_hip_pyramid_upload_level0_and_build(dst, t->cam_index, level0);
  else rc = svo_hip_copy_d2d(ctx, dst->base + (size_t)t->cam_index * dst->pyr_bytes,
                             kf->base + ((size_t)t->cam_index * t->cfg.max_keyframes + kf_slot) * kf->pyr_bytes, dst->pyr_bytes);
  if (rc != SVO_HIP_OK) return rc;
  const int32_t n32 = n;
  SVO_CHECK_HIP(ctx, hipMemcpyAsync(t->last.n, &n32, 4, hipMemcpyHostToDevice, ctx->stream));
  SVO_CHECK_HIP(ctx, hipMemcpyAsync(t->last.T_f_w, T_f_w, 56, hipMemcpyHostToDevice, ctx->stream));
  if (n > 0) {
    SVO_CHECK_HIP(ctx, hipMemcpyAsync(t->last.px, px, (size_t)n * 16, hipMemcpyHostToDevice, ctx->stream));
    SVO_CHECK_HIP(ctx, hipMemcpyAsync(t->last.f, f, (size_t)n * 24, hipMemcpyHostToDevice, ctx->stream));
    SVO_CHECK_HIP(ctx, hipMemcpyAsync(t->last.point, point, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  }
  t->last_n_host = n;
  t->last_max_point = max_point;
  t->last_from_track = false;
  t->last_renumbered = false;
  t->have_last = true;
  t->overlap_valid = false;
  t->need_gather = true;
  return SVO_HIP_OK;
}

// a tracked frame's outcome from the camera's page-locked result block (valid until the camera's next frame)
static void trk_copy_out(svo_hip_tracker* t, svo_hip_track_result* result, double* feat_px, double* feat_f, int32_t* feat_level, int32_t* feat_point,
                         uint8_t* feat_edgelet, double* feat_grad, int32_t* pt_type, int32_t* pt_n_failed, int32_t* pt_n_succeeded) {
  const char* rh = t->res_host;
  svo_hip_track_result r;
  memcpy(&r, rh, sizeof(r));
  if (result) *result = r;
  const size_t nf = (size_t)(r.n_features > 0 ? r.n_features : 0);
  if (feat_px) memcpy(feat_px, rh + t->o_px, nf * 16);
  if (feat_f) memcpy(feat_f, rh + t->o_f, nf * 24);
  if (feat_level) memcpy(feat_level, rh + t->o_level, nf * 4);
  if (feat_point) memcpy(feat_point, rh + t->o_point, nf * 4);
  if (feat_edgelet) memcpy(feat_edgelet, rh + t->o_edge, nf);
  if (feat_grad) memcpy(feat_grad, rh + t->o_grad, nf * 16);
  const size_t np4 = (size_t)t->track_n_points * 4;    // (the map may have gained points since: svo_hip_tracker_add_candidates)
  if (pt_type) memcpy(pt_type, rh + t->o_pt, np4);
  if (pt_n_failed) memcpy(pt_n_failed, rh + t->o_pt + np4, np4);
  if (pt_n_succeeded) memcpy(pt_n_succeeded, rh + t->o_pt + 2 * np4, np4);
}

// The cameras' arguments of the chain's kernels: one table, uploaded only when it differs from the last upload (the map, the
// scratch behind the records); the previous call's kernels are through with the staging copy: the host waited for them.  A lone
// tracker passes its entry by value instead (trk_plan_one_kernel) and uploads nothing.
static int trk_args_table(svo_hip_tracker_shared* sh, SeedRec* recs) {
  svo_hip_ctx* ctx = sh->ctx;
  const int N = sh->n_cams;
  svo_hip_tracker* t0 = sh->members[0];
  const svo_hip_tracker_config& c = t0->cfg;
  const int stride = sh->rec_stride;
  MdFrame mf;
  memset(&mf, 0, sizeof(mf));
  mf.cam = svo_make_cam(t0->cam); mf.n_pyr_levels = c.n_pyr_levels; mf.n_kf = c.max_keyframes; mf.n_ref_levels = c.n_levels;
  TrkCamArgs* an = sh->args_next.data();
  memset(an, 0, (size_t)N * sizeof(TrkCamArgs));
  for (int k = 0; k < N; ++k) {
    svo_hip_tracker* t = sh->members[(size_t)k];
    TrkCamArgs& a = an[k];
    a.m = make_map(t); a.pl = t->pl; a.ft = t->ft; a.last = t->last;
    a.mf = mf; a.mf.slot_base = k * c.max_keyframes;
    a.T_slot_w = t->T_slot_w;
    a.recs = recs + (size_t)k * stride;
    a.sia_state = svo_sia_state_dev(sh->sia, k);
    a.cell_winner = t->cell_winner; a.cell_cum = t->cell_cum;
    a.po = t->po;
    a.res = t->res_dev;
    a.o_px = t->o_px; a.o_f = t->o_f; a.o_level = t->o_level; a.o_point = t->o_point; a.o_edge = t->o_edge; a.o_grad = t->o_grad; a.o_pt = t->o_pt;
    a.o_flag = t->o_flag;
  }
  const size_t args_bytes = (size_t)N * sizeof(TrkCamArgs);
  if (N > 1 && (!sh->args_valid || memcmp(sh->args_host, an, args_bytes) != 0)) {
    sh->args_valid = false;
    memcpy(sh->args_host, an, args_bytes);
    SVO_CHECK_HIP(ctx, hipMemcpyAsync(sh->args_dev, sh->args_host, args_bytes, hipMemcpyHostToDevice, ctx->stream));
    sh->args_valid = true;
  }
  return SVO_HIP_OK;
}

// One frame for every camera of the shared part: ONE chain of launches whatever the number of cameras.  level0[c]: camera c's
// new image (its own page-locked buffer: no copy).
// image_ready: the new frames' pyramids are built already (svo_hip_tracker_relocalize, whose gate ran on them).
static int trk_track_all(svo_hip_tracker_shared* sh, const uint8_t* const* level0, const char* who, bool image_ready = false) {
  svo_hip_ctx* ctx = sh->ctx;
  const int N = sh->n_cams;
  svo_hip_tracker* t0 = sh->members[0];
  const svo_hip_tracker_config& c = t0->cfg;
  for (int k = 0; k < N; ++k) {
    svo_hip_tracker* t = sh->members[(size_t)k];
    if (!t->have_map || !t->have_last)
      return svo_fail(ctx, SVO_HIP_ERR_STATE, who, "svo_hip_tracker_set_map and svo_hip_tracker_set_last_frame come first (every camera)");
  }
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  for (int k = 0; k < N; ++k) sh->members[(size_t)k]->overlap_valid = false;    // (until the chain has completed: its plan rewrites the list)
  const size_t l0 = (size_t)t0->cam.width * t0->cam.height;
  svo_hip_pyramid* ref = sh->frame_pyr[sh->last_idx];
  svo_hip_pyramid* cur = sh->frame_pyr[1 - sh->last_idx];
  // ---- new Frame(cam, img, t): the images cross the link once, from page-locked memory; the pyramids are built on the device
  for (int k = 0; k < N && !image_ready; ++k) {
    svo_hip_tracker* t = sh->members[(size_t)k];
    if (level0[k] != reinterpret_cast<const uint8_t*>(t->img_host)) memcpy(t->img_host, level0[k], l0);      // (svo_hip_tracker_image_buffer: already there)
  }
  int rc = image_ready ? SVO_HIP_OK : svo_pyramid_build_levels(cur, 0, N, sh->img_dev, sh->img_stride);
  if (rc != SVO_HIP_OK) return rc;
  // ---- SparseImgAlign(kltMaxLevel, kltMinLevel, 30, GaussNewton, false, false).run(last_frame_, new_frame_)
  rc = svo_hip_sia_set_frames(sh->sia, ref, cur);
  if (rc != SVO_HIP_OK) return rc;
  // the previous call's hand-over kernel has written the solver's inputs already, unless the host changed the last frame,
  // the map or point positions since
  for (int k = 0; k < N; ++k) {
    svo_hip_tracker* t = sh->members[(size_t)k];
    if (t->need_gather) rc = svo_sia_prepare_from_device(sh->sia, k, &t->cam, t->last_n_host, t->last.n, t->last.T_f_w, t->last.px, t->last.f, t->last.point, t->pt_pos);
    else rc = svo_sia_note_device_slot(sh->sia, k, &t->cam, t->last_n_host);
    if (rc != SVO_HIP_OK) return rc;
  }
  svo_hip_sia_params sp;
  sp.max_level = c.klt_max_level; sp.min_level = c.klt_min_level; sp.n_iter = c.sia_n_iter; sp.eps = c.sia_eps; sp.early_stop = 1;
  rc = svo_hip_sia_run(sh->sia, N, &sp);
  if (rc != SVO_HIP_OK) return rc;
  // ---- Reprojector::reprojectMap
  const Cam cam = svo_make_cam(t0->cam);
  bool any_edgelet = false;
  for (int k = 0; k < N; ++k) {
    svo_hip_tracker* t = sh->members[(size_t)k];
    if (t->rekey_pending && t->n_kf > 0) {    // Map::safeDeletePoint of the previous frame: Frame::removeKeyPoint on the keyframes
      hipLaunchKernelGGL(trk_rekey_kernel, dim3(t->n_kf), dim3(KEY_THREADS), 0, ctx->stream, make_map(t), t->kf_key_point, cam);
      SVO_CHECK_HIP(ctx, hipGetLastError());
    }
    t->rekey_pending = false;
    any_edgelet = any_edgelet || t->any_edgelet;
  }
  SeedRec* recs = nullptr;
  uint32_t* pwb_t = nullptr;
  int n_pad = 0;
  const int stride = sh->rec_stride;
  rc = svo_match_scratch(ctx, N * stride, &recs, &pwb_t, &n_pad);
  if (rc != SVO_HIP_OK) return rc;
  rc = trk_args_table(sh, recs);
  if (rc != SVO_HIP_OK) return rc;
  const TrkCamArgs* an = sh->args_next.data();
  const TrkCamArgs* ad = sh->args_dev;
  if (N == 1) hipLaunchKernelGGL(trk_plan_one_kernel, dim3(1), dim3(TRK_THREADS), 0, ctx->stream, an[0]);
  else hipLaunchKernelGGL(trk_plan_cams_kernel, dim3(N), dim3(TRK_THREADS), 0, ctx->stream, ad);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  // warp + align2D (+ align1D when a map holds edgelets) over every camera's candidates
  rc = svo_match_stages_cams(ctx, sh->kf_pyr, cur, &t0->cam, N, stride, sh->counters, 8, sh->cand_level_ref, recs, pwb_t, n_pad, c.n_pyr_levels,
                             c.align_max_iter, any_edgelet);
  if (rc != SVO_HIP_OK) return rc;
  if (N == 1) hipLaunchKernelGGL(trk_replay_one_kernel, dim3(1), dim3(TRK_THREADS), 0, ctx->stream, an[0], c.max_fts, c.quality_min_fts);
  else hipLaunchKernelGGL(trk_replay_cams_kernel, dim3(N), dim3(TRK_THREADS), 0, ctx->stream, ad, c.max_fts, c.quality_min_fts);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  // ---- pose_optimizer::optimizeGaussNewton(poseOptimThresh, poseOptimNumIter, ...) on the matched features, from the aligned pose
  const FrameState* st0 = svo_sia_state_dev(sh->sia, 0);
  static_assert(sizeof(FrameState) % sizeof(double) == 0, "the solver records are a whole number of doubles apart");
  rc = svo_pose_optimize_batch_strided(ctx, N, c.max_frame_features, sh->counters + 5, 8, st0->T_cur_w, (int)(sizeof(FrameState) / sizeof(double)),
                                       sh->ft_f, sh->ft_pos, sh->ft_level, sh->ft_has_point, fabs(t0->cam.fx), c.pose_optim_thresh,
                                       c.pose_optim_num_iter, sh->po);
  if (rc != SVO_HIP_OK) return rc;
  // ---- hand-over + result: written straight into the page-locked blocks, the frame's sequence number last
  const unsigned long long seq = ++sh->seq;
  if (N == 1) hipLaunchKernelGGL(trk_finish_one_kernel, dim3(1), dim3(256), 0, ctx->stream, an[0], seq);
  else hipLaunchKernelGGL(trk_finish_cams_kernel, dim3(N), dim3(256), 0, ctx->stream, ad, seq);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  // the one synchronisation of the frame: wait for every camera's sequence number (a spin on host memory: no driver call on the
  // way back), with the stream's own synchronisation as the fall-back and the error check
  {
    bool all = false;
    for (long spins = 0; spins < 4000000L && !all; ++spins) {                 // a few hundred milliseconds at most
      all = true;
      for (int k = 0; k < N && all; ++k) {
        svo_hip_tracker* t = sh->members[(size_t)k];
        volatile unsigned long long* flag = reinterpret_cast<volatile unsigned long long*>(t->res_host + t->o_flag);
        all = __atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq;
      }
      if (!all) __builtin_ia32_pause();
    }
    if (!all) SVO_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < N; ++k) {
      svo_hip_tracker* t = sh->members[(size_t)k];
      volatile unsigned long long* flag = reinterpret_cast<volatile unsigned long long*>(t->res_host + t->o_flag);
      if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != seq) return svo_fail(ctx, SVO_HIP_ERR_DEVICE, who, "the frame's kernels did not complete");
    }
  }
  sh->last_idx = 1 - sh->last_idx;          // the new frames' pyramids are the next call's references
  for (int k = 0; k < N; ++k) {
    svo_hip_tracker* t = sh->members[(size_t)k];
    const svo_hip_track_result* r = reinterpret_cast<const svo_hip_track_result*>(t->res_host);
    t->last_n_host = r->n_features;
    t->track_n_points = t->n_points;
    t->last_from_track = true;
    t->last_renumbered = false;
    t->need_gather = false;
    t->overlap_valid = true;
    if (r->map_changed) t->rekey_pending = true;
  }
  return SVO_HIP_OK;
}

int svo_hip_tracker_track(svo_hip_tracker* t, const uint8_t* level0, svo_hip_track_result* result, double* feat_px, double* feat_f,
                          int32_t* feat_level, int32_t* feat_point, uint8_t* feat_edgelet, double* feat_grad, int32_t* pt_type,
                          int32_t* pt_n_failed, int32_t* pt_n_succeeded) {
  if (!t || !level0 || !result) return SVO_HIP_ERR_INVALID;
  if (t->sh->n_cams != 1)
    return svo_fail(t->ctx, SVO_HIP_ERR_STATE, "svo_hip_tracker_track", "a camera of a tracker group is tracked with its group (svo_hip_tracker_group_track)");
  const int rc = trk_track_all(t->sh, &level0, "svo_hip_tracker_track");
  if (rc != SVO_HIP_OK) return rc;
  trk_copy_out(t, result, feat_px, feat_f, feat_level, feat_point, feat_edgelet, feat_grad, pt_type, pt_n_failed, pt_n_succeeded);
  return SVO_HIP_OK;
}

// ---- a group of cameras: N trackers with one camera model and one configuration whose frames are tracked TOGETHER -- one
// chain of launches per call whatever N (every kernel of the chain takes one workgroup, or one slice of its grid, per camera).
// Every camera keeps its own map, last frame and result block and is set up with the svo_hip_tracker_* functions of its
// handle (svo_hip_tracker_group_camera); only the per-frame call is the group's.
struct svo_hip_tracker_group {
  svo_hip_tracker_shared* sh = nullptr;
};

int svo_hip_tracker_group_create(svo_hip_ctx* ctx, const svo_hip_camera* cam, const svo_hip_tracker_config* cfg, int n_cameras,
                                 svo_hip_tracker_group** out) {
  if (!ctx || !cam || !cfg || !out) return SVO_HIP_ERR_INVALID;
  *out = nullptr;
  SVO_REQUIRE(ctx, n_cameras >= 1 && n_cameras <= 1024);
  int rc = trk_check_config(ctx, cam, cfg);
  if (rc != SVO_HIP_OK) return rc;
  // a block of the batched warp / alignment stages takes 16 candidates and must not straddle two cameras
  SVO_REQUIRE(ctx, n_cameras == 1 || cfg->max_items % 16 == 0);
  svo_hip_tracker_group* g = new (std::nothrow) svo_hip_tracker_group();
  if (!g) return SVO_HIP_ERR_NOMEM;
  rc = trk_shared_create(ctx, cam, cfg, n_cameras, &g->sh);
  for (int k = 0; k < n_cameras && rc == SVO_HIP_OK; ++k) {
    svo_hip_tracker* t = nullptr;
    rc = trk_member_create(g->sh, k, cam, cfg, &t);
    if (rc == SVO_HIP_OK) g->sh->members.push_back(t);
  }
  if (rc != SVO_HIP_OK) { svo_hip_tracker_group_destroy(g); return rc; }
  *out = g;
  return SVO_HIP_OK;
}

int svo_hip_tracker_group_destroy(svo_hip_tracker_group* g) {
  if (!g) return SVO_HIP_ERR_INVALID;
  if (g->sh) {
    (void)hipStreamSynchronize(g->sh->ctx->stream);
    for (svo_hip_tracker* t : g->sh->members) trk_member_destroy(t);
    trk_shared_destroy(g->sh);
  }
  delete g;
  return SVO_HIP_OK;
}

int svo_hip_tracker_group_camera(svo_hip_tracker_group* g, int index, svo_hip_tracker** camera) {
  if (!g || !g->sh || !camera) return SVO_HIP_ERR_INVALID;
  SVO_REQUIRE(g->sh->ctx, index >= 0 && index < g->sh->n_cams);
  *camera = g->sh->members[(size_t)index];
  return SVO_HIP_OK;
}

int svo_hip_tracker_group_track(svo_hip_tracker_group* g, const uint8_t* const* level0, svo_hip_track_result* results) {
  if (!g || !g->sh || !level0) return SVO_HIP_ERR_INVALID;
  for (int k = 0; k < g->sh->n_cams; ++k) if (!level0[k]) return SVO_HIP_ERR_INVALID;
  const int rc = trk_track_all(g->sh, level0, "svo_hip_tracker_group_track");
  if (rc != SVO_HIP_OK) return rc;
  if (results) for (int k = 0; k < g->sh->n_cams; ++k) trk_copy_out(g->sh->members[(size_t)k], results + k, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  return SVO_HIP_OK;
}

int svo_hip_tracker_last_result(svo_hip_tracker* t, svo_hip_track_result* result, double* feat_px, double* feat_f, int32_t* feat_level,
                                int32_t* feat_point, uint8_t* feat_edgelet, double* feat_grad, int32_t* pt_type, int32_t* pt_n_failed,
                                int32_t* pt_n_succeeded) {
  if (!t) return SVO_HIP_ERR_INVALID;
  if (!t->last_from_track) return svo_fail(t->ctx, SVO_HIP_ERR_STATE, "svo_hip_tracker_last_result", "no frame has been tracked since the last frame was set");
  trk_copy_out(t, result, feat_px, feat_f, feat_level, feat_point, feat_edgelet, feat_grad, pt_type, pt_n_failed, pt_n_succeeded);
  return SVO_HIP_OK;
}

int svo_hip_tracker_set_sia_option(svo_hip_tracker* t, int option, int value) {
  if (!t) return SVO_HIP_ERR_INVALID;
  // the one option that changes no decision of the chain, only the grouping of the solver's sums; the solver is the
  // shared one: a camera of a group sets it for the group
  if (option != SVO_HIP_SIA_OPT_REDUCTION)
    return svo_fail(t->ctx, SVO_HIP_ERR_INVALID, "svo_hip_tracker_set_sia_option", "only SVO_HIP_SIA_OPT_REDUCTION can be set on a tracker's solver");
  return svo_hip_sia_set_option(t->sh->sia, option, value);
}

int svo_hip_tracker_image_buffer(svo_hip_tracker* t, uint8_t** buffer) {
  if (!t || !buffer) return SVO_HIP_ERR_INVALID;
  *buffer = reinterpret_cast<uint8_t*>(t->img_host);
  return SVO_HIP_OK;
}

int svo_hip_tracker_download_key_points(svo_hip_tracker* t, int32_t* kf_key_point) {
  if (!t || !kf_key_point) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = t->ctx;
  if (!t->have_map) return svo_fail(ctx, SVO_HIP_ERR_STATE, "svo_hip_tracker_download_key_points", "no map has been set");
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  const int rc = trk_rekey_now(t);
  if (rc != SVO_HIP_OK) return rc;
  if (t->n_kf > 0) {
    SVO_CHECK_HIP(ctx, hipMemcpyAsync(kf_key_point, t->kf_key_point, (size_t)t->n_kf * 5 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    SVO_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return SVO_HIP_OK;
}

int svo_hip_tracker_add_candidates(svo_hip_tracker* t, int n, const double* pos, const int32_t* kf_index, const double* px, const double* f,
                                   const int32_t* level, const uint8_t* edgelet, const double* grad, int32_t* first_point) {
  if (!t) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = t->ctx;
  const svo_hip_tracker_config& c = t->cfg;
  SVO_REQUIRE(ctx, n >= 0 && (n == 0 || (pos && kf_index && px && f && level)));
  if (!t->have_map) return svo_fail(ctx, SVO_HIP_ERR_STATE, "svo_hip_tracker_add_candidates", "no map has been set");
  // every index and every capacity, before anything is enqueued
  SVO_REQUIRE(ctx, n <= c.max_points - t->n_points && n <= c.max_candidates - t->n_candidates);
  int n_new_obs = 0;
  bool edge = false;
  for (int i = 0; i < n; ++i) {
    SVO_REQUIRE(ctx, kf_index[i] >= -1 && kf_index[i] < t->n_kf && level[i] >= 0 && level[i] < c.n_levels);
    if (kf_index[i] >= 0) { ++n_new_obs; edge = edge || (edgelet && edgelet[i]); }
  }
  SVO_REQUIRE(ctx, n_new_obs <= c.max_obs - t->n_obs);
  if (first_point) *first_point = t->n_points;
  if (n == 0) return SVO_HIP_OK;
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t bytes = (size_t)n * sizeof(TrkCandRec);
  char* d = nullptr;
  char* hs = nullptr;
  int rc = svo_ctx_staging(ctx, bytes, &d);
  if (rc == SVO_HIP_OK) rc = svo_ctx_host_staging(ctx, bytes, &hs);
  if (rc != SVO_HIP_OK) return rc;
  SVO_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the staging area may still feed an earlier transfer
  TrkCandRec* rec = reinterpret_cast<TrkCandRec*>(hs);
  int at = t->n_obs;
  for (int i = 0; i < n; ++i) {
    TrkCandRec r;
    memset(&r, 0, sizeof(r));
    memcpy(r.pos, pos + 3 * (size_t)i, 24); memcpy(r.px, px + 2 * (size_t)i, 16); memcpy(r.f, f + 3 * (size_t)i, 24);
    if (grad) memcpy(r.grad, grad + 2 * (size_t)i, 16); else { r.grad[0] = 1.0; r.grad[1] = 0.0; }
    r.kf = kf_index[i]; r.level = level[i]; r.edgelet = edgelet && edgelet[i] ? 1 : 0; r.obs = at;
    if (r.kf >= 0) ++at;
    rec[i] = r;
  }
  SVO_CHECK_HIP(ctx, hipMemcpyAsync(d, hs, bytes, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(trk_add_candidates_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, reinterpret_cast<const TrkCandRec*>(d),
                     t->n_points, t->n_candidates, t->pt_pos, t->pt_type, t->pt_n_failed, t->pt_n_succeeded, t->pt_unlinked, t->tables[t->cur]);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  // existing indices keep their meaning: the last frame, the solver's copy of it and a pending re-selection stay as they are
  t->n_points += n; t->n_candidates += n; t->n_obs = at;
  t->any_edgelet = t->any_edgelet || edge;
  return SVO_HIP_OK;
}

int svo_hip_tracker_promote_last_frame(svo_hip_tracker* t, int slot, int* kf_index, int* n_promoted_candidates) {
  if (!t) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = t->ctx;
  const svo_hip_tracker_config& c = t->cfg;
  const char* who = "svo_hip_tracker_promote_last_frame";
  const int n_feat = t->last_n_host;
  const int32_t* fp = reinterpret_cast<const int32_t*>(t->res_host + t->o_point);
  int rc = trk_rebuild_begin(t, who, [&]() -> int {
    // a frame from svo_hip_tracker_set_last_frame has no levels, edgelet flags or gradients
    if (!t->have_last || !t->last_from_track) return svo_fail(ctx, SVO_HIP_ERR_STATE, who, "the last frame has to be a tracked one");
    SVO_REQUIRE(ctx, slot >= 0 && slot < c.max_keyframes && t->n_kf < c.max_keyframes);
    for (int k = 0; k < t->n_kf; ++k) SVO_REQUIRE(ctx, t->kf_slot_host[(size_t)k] != slot);
    // the frame's features with a point, from the page-locked result block; every one is a new observation and a row entry of
    // the new keyframe.  The promoted candidates add one row entry each at most, and each of them is one of those features:
    // min(features with a point, candidates) bounds what the rows can gain beyond that.
    int n_with_point = 0;
    for (int i = 0; i < n_feat; ++i) n_with_point += fp[i] >= 0 ? 1 : 0;
    const int seeds_bound = n_with_point < t->n_candidates ? n_with_point : t->n_candidates;
    SVO_REQUIRE(ctx, n_with_point <= c.max_obs - t->n_obs && n_with_point + seeds_bound <= c.max_kf_features - t->n_ftr);
    return SVO_HIP_OK;
  });
  if (rc != SVO_HIP_OK) return rc;
  rc = svo_hip_tracker_keyframe_from_last_frame(t, slot);
  if (rc != SVO_HIP_OK) return rc;
  hipLaunchKernelGGL(trk_promote_kernel, dim3(1), dim3(TRK_THREADS), 0, ctx->stream, make_map(t), t->tables[1 - t->cur], t->scratch, t->T_kf_w,
                     t->T_slot_w, t->kf_slot, t->kf_key_point, t->pl.first_seq, t->ft, t->last, n_feat, slot, svo_make_cam(t->cam));
  SVO_CHECK_HIP(ctx, hipGetLastError());
  int out[4] = {0, 0, 0, 0};
  rc = trk_rebuild_end(t, out, 4);
  if (rc != SVO_HIP_OK) return rc;
  if (kf_index) *kf_index = t->n_kf;
  if (n_promoted_candidates) *n_promoted_candidates = out[0];
  t->kf_slot_host.push_back(slot);
  t->n_kf += 1;
  t->overlap_valid = false;                 // the frame is a keyframe of the map now
  if (!t->any_edgelet) {                    // the new observations carry the frame's edgelet flags
    const uint8_t* fe = reinterpret_cast<const uint8_t*>(t->res_host + t->o_edge);
    for (int i = 0; i < n_feat && !t->any_edgelet; ++i) t->any_edgelet = fp[i] >= 0 && fe[i] != 0;
  }
  return SVO_HIP_OK;
}

int svo_hip_tracker_remove_keyframe(svo_hip_tracker* t, int kf_index, int* slot_freed, int* n_deleted_points, int* n_deleted_candidates) {
  if (!t) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = t->ctx;
  int rc = trk_rebuild_begin(t, "svo_hip_tracker_remove_keyframe", [&]() -> int {
    // (the reference removes a keyframe only when Config::maxNKfs() > 2: the map never loses its only one)
    SVO_REQUIRE(ctx, kf_index >= 0 && kf_index < t->n_kf && t->n_kf > 1);
    return SVO_HIP_OK;
  });
  if (rc != SVO_HIP_OK) return rc;
  hipLaunchKernelGGL(trk_remove_kernel, dim3(1), dim3(TRK_THREADS), 0, ctx->stream, make_map(t), t->tables[1 - t->cur], t->scratch, t->T_kf_w,
                     t->kf_slot, t->kf_key_point, t->pl.first_seq, t->last, kf_index, t->n_ftr);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  int out[5] = {0, 0, 0, 0, 0};
  rc = trk_rebuild_end(t, out, 5);
  if (rc != SVO_HIP_OK) return rc;
  if (slot_freed) *slot_freed = t->kf_slot_host[(size_t)kf_index];
  if (n_deleted_points) *n_deleted_points = out[0];
  if (n_deleted_candidates) *n_deleted_candidates = out[4];
  t->kf_slot_host.erase(t->kf_slot_host.begin() + kf_index);
  t->n_kf -= 1;
  t->overlap_valid = false;                 // the keyframes are renumbered
  // the keyframes that lost a key feature to a point deleted here choose again (Frame::removeKeyPoint), on the new rows,
  // before anything reads the key points
  if (out[0] > 0) t->rekey_pending = true;
  return SVO_HIP_OK;
}

int svo_hip_tracker_compact_points(svo_hip_tracker* t, int* n_points_after, int32_t* old_to_new) {
  if (!t) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = t->ctx;
  int rc = trk_rebuild_begin(t, "svo_hip_tracker_compact_points", []() -> int { return SVO_HIP_OK; });
  if (rc != SVO_HIP_OK) return rc;
  const int n_before = t->n_points;
  hipLaunchKernelGGL(trk_compact_kernel, dim3(1), dim3(TRK_THREADS), 0, ctx->stream, make_map(t), t->tables[1 - t->cur], t->scratch, t->pt_pos,
                     t->kf_key_point, t->pl.first_seq, t->last, t->n_ftr);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  if (old_to_new && n_before > 0)           // (enqueued before trk_rebuild_end synchronises)
    SVO_CHECK_HIP(ctx, hipMemcpyAsync(old_to_new, t->pl.first_seq, (size_t)n_before * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  int out[5] = {0, 0, 0, 0, -1};
  rc = trk_rebuild_end(t, out, 5);
  if (rc != SVO_HIP_OK) return rc;
  t->n_points = out[0];
  // the last frame's features refer to the new numbering on the device; the result block (and track_n_points, its layout)
  // stays the tracked frame's under the old one
  t->last_max_point = out[4];
  t->last_renumbered = t->last_from_track;
  if (n_points_after) *n_points_after = t->n_points;
  return SVO_HIP_OK;
}

// ---- relocalisation against a keyframe of the device map (FrameHandlerMono::relocalizeFrame, S/frame_handler_mono.cpp:317-349)

// trk_reloc_kernel and its report: one launch, one synchronisation.  The owed re-selection of key points runs first.
static int trk_reloc_run(svo_hip_tracker* t, const TrkRelocArgs& a, TrkRelocOut* out) {
  svo_hip_ctx* ctx = t->ctx;
  int rc = trk_rekey_now(t);
  if (rc == SVO_HIP_OK) {
    hipLaunchKernelGGL(trk_reloc_kernel, dim3(1), dim3(RELOC_THREADS), 0, ctx->stream, make_map(t), t->last, svo_make_cam(t->cam), a, t->reloc_out);
    if (hipGetLastError() != hipSuccess) rc = svo_fail(ctx, SVO_HIP_ERR_DEVICE, "trk_reloc_kernel", "launch failed");
  }
  hipError_t e = rc == SVO_HIP_OK ? hipMemcpyAsync(out, t->reloc_out, sizeof(TrkRelocOut), hipMemcpyDeviceToHost, ctx->stream) : hipSuccess;
  const hipError_t es = hipStreamSynchronize(ctx->stream);                      // (on the error paths too)
  if (rc != SVO_HIP_OK) return rc;
  if (e != hipSuccess || es != hipSuccess) return svo_fail(ctx, SVO_HIP_ERR_DEVICE, "trk_reloc_kernel", hipGetErrorString(e != hipSuccess ? e : es));
  return SVO_HIP_OK;
}

static TrkRelocArgs trk_reloc_args(const svo_hip_tracker* t, int kf, int exclude, const double* T) {
  TrkRelocArgs a;
  memset(&a, 0, sizeof(a));
  a.kf = kf; a.exclude = exclude; a.choose = kf < 0 ? 1 : 0; a.max_feat = t->cfg.max_frame_features;
  a.use_last_pose = T ? 0 : 1;
  if (T) memcpy(a.T, T, sizeof(a.T)); else a.T[6] = 1.0;
  return a;
}

// the host's side of "the last frame is keyframe k now" (the kernel has written the device's): the keyframe's pyramid becomes
// the last frame's, and the tracker is where svo_hip_tracker_set_last_frame leaves it
static int trk_last_is_keyframe(svo_hip_tracker* t, int k, const TrkRelocOut& o) {
  svo_hip_pyramid* dst = t->sh->frame_pyr[t->sh->last_idx];
  const svo_hip_pyramid* kf = t->sh->kf_pyr;
  const int rc = svo_hip_copy_d2d(t->ctx, dst->base + (size_t)t->cam_index * dst->pyr_bytes,
                                  kf->base + ((size_t)t->cam_index * t->cfg.max_keyframes + t->kf_slot_host[(size_t)k]) * kf->pyr_bytes, dst->pyr_bytes);
  t->last_n_host = o.n_feat;
  t->last_max_point = o.max_point;
  t->last_from_track = false;
  t->last_renumbered = false;
  t->have_last = true;
  t->overlap_valid = false;
  t->need_gather = true;
  return rc;
}

int svo_hip_tracker_closest_keyframe(svo_hip_tracker* t, const double T_f_w[7], int exclude_kf, int* kf_index, int* n_close, double* distance) {
  if (!t || !kf_index) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = t->ctx;
  const char* who = "svo_hip_tracker_closest_keyframe";
  if (!t->have_map) return svo_fail(ctx, SVO_HIP_ERR_STATE, who, "no map has been set");
  if (!T_f_w && !t->have_last) return svo_fail(ctx, SVO_HIP_ERR_STATE, who, "no pose given and the device holds no last frame");
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  TrkRelocOut o;
  const int rc = trk_reloc_run(t, trk_reloc_args(t, -1, exclude_kf, T_f_w), &o);
  if (rc != SVO_HIP_OK) return rc;
  *kf_index = o.kf;
  if (n_close) *n_close = o.n_close;
  if (distance) *distance = o.distance;
  return SVO_HIP_OK;
}

int svo_hip_tracker_last_frame_from_keyframe(svo_hip_tracker* t, int kf_index, int* n_features) {
  if (!t) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = t->ctx;
  const char* who = "svo_hip_tracker_last_frame_from_keyframe";
  if (!t->have_map) return svo_fail(ctx, SVO_HIP_ERR_STATE, who, "no map has been set");
  SVO_REQUIRE(ctx, kf_index >= 0 && kf_index < t->n_kf);
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  TrkRelocArgs a = trk_reloc_args(t, kf_index, -1, nullptr);
  a.apply = 1; a.use_last_pose = 0;                                             // (no pose is read: nothing is chosen, no gate follows)
  TrkRelocOut o;
  int rc = trk_reloc_run(t, a, &o);
  if (rc != SVO_HIP_OK) return rc;
  if (!o.applied) return svo_fail(ctx, SVO_HIP_ERR_INVALID, who, "the keyframe has more living features than max_frame_features");
  rc = trk_last_is_keyframe(t, kf_index, o);
  if (rc != SVO_HIP_OK) return rc;
  if (n_features) *n_features = o.n_feat;
  return SVO_HIP_OK;
}

int svo_hip_tracker_relocalize(svo_hip_tracker* t, const uint8_t* level0, int kf_index, int exclude_kf, const double T_f_w_init[7], int min_tracked,
                               svo_hip_reloc_result* reloc, svo_hip_track_result* result, double* feat_px, double* feat_f, int32_t* feat_level,
                               int32_t* feat_point, uint8_t* feat_edgelet, double* feat_grad, int32_t* pt_type, int32_t* pt_n_failed,
                               int32_t* pt_n_succeeded) {
  if (!t) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = t->ctx;
  svo_hip_tracker_shared* sh = t->sh;
  const char* who = "svo_hip_tracker_relocalize";
  if (!t->have_map) return svo_fail(ctx, SVO_HIP_ERR_STATE, who, "no map has been set");
  if (!T_f_w_init && !t->have_last) return svo_fail(ctx, SVO_HIP_ERR_STATE, who, "no pose given and the device holds no last frame");
  if (sh->n_cams != 1)
    return svo_fail(ctx, SVO_HIP_ERR_STATE, who, "a camera of a tracker group relocalises with svo_hip_tracker_last_frame_from_keyframe and svo_hip_tracker_group_track");
  SVO_REQUIRE(ctx, level0 && reloc && kf_index < t->n_kf && min_tracked >= 0);
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  memset(reloc, 0, sizeof(*reloc));
  reloc->kf_index = -1;
  // whatever fails from here on: the stream is through with the staging areas before the call returns
  auto fail = [&](int rc) { (void)hipStreamSynchronize(ctx->stream); t->need_gather = true; return rc; };
  // ---- new Frame(cam, img, t): the image and its pyramid, as in svo_hip_tracker_track (the pyramid batch that is not the last frame's)
  svo_hip_pyramid* cur = sh->frame_pyr[1 - sh->last_idx];
  if (level0 != reinterpret_cast<const uint8_t*>(t->img_host)) memcpy(t->img_host, level0, (size_t)t->cam.width * t->cam.height);
  int rc = svo_pyramid_build_levels(cur, 0, 1, sh->img_dev, sh->img_stride);
  if (rc != SVO_HIP_OK) return fail(rc);
  // ---- the keyframe (Map::getClosestKeyframe unless given), and last_frame_ = ref_keyframe with the gate's poses in the solver
  TrkRelocArgs a = trk_reloc_args(t, kf_index < 0 ? -1 : kf_index, exclude_kf, T_f_w_init);
  a.apply = 1; a.gate = 1;
  TrkRelocOut o;
  rc = trk_reloc_run(t, a, &o);
  if (rc != SVO_HIP_OK) return fail(rc);
  reloc->kf_index = o.kf;
  reloc->n_close = kf_index < 0 ? o.n_close : 0;
  if (o.kf < 0) return SVO_HIP_OK;                                               // no keyframe is close: the last frame is kept
  if (!o.applied) return svo_fail(ctx, SVO_HIP_ERR_INVALID, who, "the keyframe has more living features than max_frame_features");
  rc = trk_last_is_keyframe(t, o.kf, o);
  if (rc != SVO_HIP_OK) return fail(rc);
  // ---- SparseImgAlign(kltMaxLevel, kltMinLevel, 30, GaussNewton).run(ref_keyframe, new_frame) from T_f_w_init (:329-333)
  const svo_hip_tracker_config& c = t->cfg;
  svo_hip_sia_params sp;
  sp.max_level = c.klt_max_level; sp.min_level = c.klt_min_level; sp.n_iter = c.sia_n_iter; sp.eps = c.sia_eps; sp.early_stop = 1;
  svo_hip_sia_result gate;
  rc = svo_hip_sia_set_frames(sh->sia, sh->frame_pyr[sh->last_idx], cur);
  if (rc == SVO_HIP_OK) rc = svo_sia_note_device_slot(sh->sia, 0, &t->cam, o.n_feat);
  if (rc == SVO_HIP_OK) rc = svo_hip_sia_run(sh->sia, 1, &sp);
  if (rc == SVO_HIP_OK) rc = svo_hip_sia_download(sh->sia, 0, &gate);             // (synchronises: the outcome steers the host)
  if (rc != SVO_HIP_OK) return fail(rc);
  reloc->gate_stop = gate.stop;
  reloc->gate_n_tracked = gate.n_tracked;
  for (int i = 0; i < SVO_HIP_MAX_LEVELS; ++i) reloc->gate_iters[i] = gate.iters[i];
  memcpy(reloc->T_f_w_gate, gate.T_cur_w, sizeof(reloc->T_f_w_gate));
  if (gate.n_tracked > (uint64_t)min_tracked) {
    // ---- processFrame (:338) with last_frame_ = ref_keyframe: the chain starts SparseImgAlign again from the keyframe's pose (:175)
    reloc->accepted = 1;
    rc = trk_track_all(sh, &level0, who, true);
    if (rc != SVO_HIP_OK) return fail(rc);
    trk_copy_out(t, result, feat_px, feat_f, feat_level, feat_point, feat_edgelet, feat_grad, pt_type, pt_n_failed, pt_n_succeeded);
    return SVO_HIP_OK;
  }
  // ---- refused: last_frame_ = new_frame_ (FrameHandlerMono::addImage :90) -- the new image, no features, the pose the gate left
  hipError_t e = hipMemsetAsync(t->last.n, 0, sizeof(int), ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(t->last.T_f_w, svo_sia_state_dev(sh->sia, 0)->T_cur_w, 7 * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream);
  if (e != hipSuccess) return fail(svo_fail(ctx, SVO_HIP_ERR_DEVICE, who, hipGetErrorString(e)));
  sh->last_idx = 1 - sh->last_idx;
  t->last_n_host = 0;
  t->last_max_point = -1;
  return SVO_HIP_OK;
}

// ---- the structure step and the keyframe decision in one call (svo_hip_tracker_finish_frame, svo_hip_tracker_group_finish_frames)

// what svo_hip_tracker_optimize_structure checks of a selection (the map has to be there), and the selection as the kernel takes it
static int trk_finish_check(svo_hip_tracker* t, int n, const int32_t* point, int n_iter, const double* pos_out, TrkStructSel* sel) {
  svo_hip_ctx* ctx = t->ctx;
  SVO_REQUIRE(ctx, n >= 0 && n <= TRK_MAX_STRUCT && n_iter >= 0 && (n == 0 || (point && pos_out)));
  memset(sel, 0, sizeof(*sel));
  sel->n = n;
  for (int i = 0; i < n; ++i) {
    SVO_REQUIRE(ctx, point[i] >= 0 && point[i] < t->n_points);
    for (int j = 0; j < i; ++j) SVO_REQUIRE(ctx, point[j] != point[i]);         // a point is optimised once per call
    sel->point[i] = point[i];
  }
  return SVO_HIP_OK;
}

// the one wait: every listed camera's flag shows its sequence number (a spin on page-locked memory, the stream's own
// synchronisation as the fall-back and the error check)
static int trk_finish_wait(svo_hip_ctx* ctx, svo_hip_tracker* const* cams, int n_cams, const char* who) {
  auto done = [&](int k) {
    volatile unsigned long long* flag = reinterpret_cast<volatile unsigned long long*>(cams[k]->st_host + ST_O_FLAG);
    return __atomic_load_n(flag, __ATOMIC_ACQUIRE) == cams[k]->st_seq;
  };
  bool all = false;
  for (long spins = 0; spins < 4000000L && !all; ++spins) {
    all = true;
    for (int k = 0; k < n_cams && all; ++k) all = done(k);
    if (!all) __builtin_ia32_pause();
  }
  if (!all) SVO_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < n_cams; ++k)
    if (!done(k)) return svo_fail(ctx, SVO_HIP_ERR_DEVICE, who, "the kernel did not complete");
  return SVO_HIP_OK;
}

static void trk_finish_copy_out(const svo_hip_tracker* t, int n, double* pos_out, int32_t* iters_out, svo_hip_kf_decision* decision) {
  if (n > 0) memcpy(pos_out, t->st_host, (size_t)n * 24);
  if (n > 0 && iters_out) memcpy(iters_out, t->st_host + ST_O_ITERS, (size_t)n * 4);
  memcpy(decision, t->st_host + ST_O_DECISION, sizeof(*decision));
}

int svo_hip_tracker_finish_frame(svo_hip_tracker* t, int n, const int32_t* point, int n_iter, double* pos_out, int32_t* iters_out,
                                 double kf_select_min_dist, svo_hip_kf_decision* decision) {
  if (!t) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = t->ctx;
  const char* who = "svo_hip_tracker_finish_frame";
  SVO_REQUIRE(ctx, decision != nullptr && kf_select_min_dist >= 0.0);          // (a NaN compares false)
  TrkStructSel sel;
  int rc = trk_finish_check(t, n, point, n_iter, pos_out, &sel);
  if (rc != SVO_HIP_OK) return rc;
  if (!t->have_map) return svo_fail(ctx, SVO_HIP_ERR_STATE, who, "no map has been set");
  if (!t->have_last) return svo_fail(ctx, SVO_HIP_ERR_STATE, who, "the device holds no last frame");
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  const unsigned long long seq = ++t->st_seq;
  hipLaunchKernelGGL(trk_finish_frame_kernel, dim3(1), dim3(FIN_THREADS), 0, ctx->stream, make_map(t), t->pt_pos, t->last, sel, n_iter,
                     t->pl.overlap_kf, t->pl.counters, t->overlap_valid ? 1 : 0, kf_select_min_dist, t->st_dev, seq);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  rc = trk_finish_wait(ctx, &t, 1, who);
  if (rc != SVO_HIP_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }
  trk_finish_copy_out(t, n, pos_out, iters_out, decision);
  // (the point table and the solver's copy of the last frame's points were updated by the kernel: nothing to gather)
  return SVO_HIP_OK;
}

int svo_hip_tracker_group_finish_frames(svo_hip_tracker_group* g, const svo_hip_structure_request* req, double kf_select_min_dist,
                                        svo_hip_kf_decision* decisions, int32_t* camera_ok) {
  if (!g || !g->sh) return SVO_HIP_ERR_INVALID;
  svo_hip_tracker_shared* sh = g->sh;
  svo_hip_ctx* ctx = sh->ctx;
  const char* who = "svo_hip_tracker_group_finish_frames";
  const int N = sh->n_cams;
  SVO_REQUIRE(ctx, decisions != nullptr && camera_ok != nullptr && kf_select_min_dist >= 0.0);
  // every camera's request, before anything is enqueued or written
  std::vector<TrkStructSel> sels((size_t)N);
  std::vector<svo_hip_tracker*> active;
  for (int k = 0; k < N; ++k) {
    svo_hip_tracker* t = sh->members[(size_t)k];
    const svo_hip_structure_request none = {0, nullptr, 0, nullptr, nullptr};
    const svo_hip_structure_request& r = req ? req[k] : none;
    if (!t->have_map || !t->have_last) {                                       // the camera sits out
      SVO_REQUIRE(ctx, r.n == 0);
      memset(&sels[(size_t)k], 0, sizeof(TrkStructSel));
      continue;
    }
    const int rc = trk_finish_check(t, r.n, r.point, r.n_iter, r.pos_out, &sels[(size_t)k]);
    if (rc != SVO_HIP_OK) return rc;
    active.push_back(t);
  }
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  for (int k = 0; k < N; ++k) { camera_ok[k] = 0; memset(&decisions[k], 0, sizeof(svo_hip_kf_decision)); }
  if (active.empty()) return SVO_HIP_OK;
  // (the previous call's kernel is through with the requests: the host waited for it)
  for (int k = 0; k < N; ++k) {
    svo_hip_tracker* t = sh->members[(size_t)k];
    TrkFinishReq r;
    memset(&r, 0, sizeof(r));
    r.sel = sels[(size_t)k];
    r.active = t->have_map && t->have_last ? 1 : 0;
    if (r.active) {
      r.n_iter = req ? req[k].n_iter : 0;
      r.overlap_valid = t->overlap_valid ? 1 : 0;
      r.st = t->st_dev;
      r.seq = ++t->st_seq;
    }
    sh->fin_host[k] = r;
  }
  // a failure from here on: the stream is through with the staging areas before the call returns
  auto fail = [&](int rc) { (void)hipStreamSynchronize(ctx->stream); return rc; };
  SeedRec* recs = nullptr;
  uint32_t* pwb_t = nullptr;
  int n_pad = 0;
  int rc = svo_match_scratch(ctx, N * sh->rec_stride, &recs, &pwb_t, &n_pad);      // (the records' address is part of the table)
  if (rc == SVO_HIP_OK) rc = trk_args_table(sh, recs);
  if (rc != SVO_HIP_OK) return fail(rc);
  if (N == 1) {
    svo_hip_tracker* t = sh->members[0];
    const TrkFinishReq& r = sh->fin_host[0];
    hipLaunchKernelGGL(trk_finish_frame_kernel, dim3(1), dim3(FIN_THREADS), 0, ctx->stream, make_map(t), t->pt_pos, t->last, r.sel, r.n_iter,
                       t->pl.overlap_kf, t->pl.counters, r.overlap_valid, kf_select_min_dist, r.st, r.seq);
  } else {
    hipLaunchKernelGGL(trk_finish_frames_cams_kernel, dim3(N), dim3(FIN_THREADS), 0, ctx->stream, sh->args_dev, sh->fin_dev, kf_select_min_dist);
  }
  if (hipGetLastError() != hipSuccess) return fail(svo_fail(ctx, SVO_HIP_ERR_DEVICE, who, "launch failed"));
  rc = trk_finish_wait(ctx, active.data(), (int)active.size(), who);
  if (rc != SVO_HIP_OK) return fail(rc);
  for (int k = 0; k < N; ++k) {
    svo_hip_tracker* t = sh->members[(size_t)k];
    if (!sh->fin_host[k].active) continue;
    camera_ok[k] = 1;
    trk_finish_copy_out(t, sels[(size_t)k].n, req ? req[k].pos_out : nullptr, req ? req[k].iters_out : nullptr, &decisions[k]);
  }
  return SVO_HIP_OK;
}

int svo_hip_tracker_map_sizes(const svo_hip_tracker* t, int* n_kf, int* n_ftr, int* n_points, int* n_obs, int* n_candidates) {
  if (!t) return SVO_HIP_ERR_INVALID;
  if (!t->have_map) return svo_fail(t->ctx, SVO_HIP_ERR_STATE, "svo_hip_tracker_map_sizes", "no map has been set");
  if (n_kf) *n_kf = t->n_kf;
  if (n_ftr) *n_ftr = t->n_ftr;
  if (n_points) *n_points = t->n_points;
  if (n_obs) *n_obs = t->n_obs;
  if (n_candidates) *n_candidates = t->n_candidates;
  return SVO_HIP_OK;
}

int svo_hip_tracker_download_map(svo_hip_tracker* t, svo_hip_tracker_map_out* out) {
  if (!t || !out) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = t->ctx;
  if (!t->have_map) return svo_fail(ctx, SVO_HIP_ERR_STATE, "svo_hip_tracker_download_map", "no map has been set");
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  const int rc = trk_rekey_now(t);
  if (rc != SVO_HIP_OK) return rc;
  hipError_t e = hipSuccess;
  auto get = [&](void* dst, const void* src, size_t bytes) {
    if (dst && bytes && e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream);
  };
  const size_t K = (size_t)t->n_kf, P = (size_t)t->n_points, O = (size_t)t->n_obs;
  const TrkTables& tb = t->tables[t->cur];
  out->n_kf = t->n_kf; out->n_points = t->n_points; out->n_candidates = t->n_candidates;
  get(out->kf_slot, t->kf_slot, K * 4); get(out->T_kf_w, t->T_kf_w, K * 56); get(out->kf_key_point, t->kf_key_point, K * 20);
  if (K) get(out->kf_ftr_offset, tb.kf_ftr_offset, (K + 1) * 4);
  get(out->kf_ftr_point, tb.kf_ftr_point, (size_t)t->n_ftr * 4);
  get(out->pt_pos, t->pt_pos, P * 24); get(out->pt_type, t->pt_type, P * 4); get(out->pt_n_failed, t->pt_n_failed, P * 4);
  get(out->pt_n_succeeded, t->pt_n_succeeded, P * 4);
  if (P) get(out->pt_obs_offset, tb.pt_obs_offset, (P + 1) * 4);
  get(out->obs_kf, tb.obs_kf, O * 4); get(out->obs_px, tb.obs_px, O * 16); get(out->obs_f, tb.obs_f, O * 24); get(out->obs_level, tb.obs_level, O * 4);
  get(out->obs_edgelet, tb.obs_edgelet, O); get(out->obs_grad, tb.obs_grad, O * 16);
  get(out->cand_point, tb.cand_point, (size_t)t->n_candidates * 4);
  if (e != hipSuccess) return svo_fail(ctx, SVO_HIP_ERR_DEVICE, "svo_hip_tracker_download_map", hipGetErrorString(e));
  SVO_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SVO_HIP_OK;
}

int svo_hip_tracker_info(const svo_hip_tracker* t, int* n_cells, int* grid_cols, int* grid_rows, svo_hip_pyramid** keyframe_pyramids) {
  if (!t) return SVO_HIP_ERR_INVALID;
  if (n_cells) *n_cells = t->n_cells;
  if (grid_cols) *grid_cols = t->grid_cols;
  if (grid_rows) *grid_rows = t->grid_rows;
  if (keyframe_pyramids) *keyframe_pyramids = t->sh->kf_pyr;      // (a group member's keyframe slot s is slot cam_index * max_keyframes + s of it)
  return SVO_HIP_OK;
}

}  // extern "C"
