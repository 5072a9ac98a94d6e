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

#include "svo_track_types.h"
#include "svo_track_chain.h"
#include "svo_track_map_edit.h"
#include "svo_track_frame_end.h"
#include "svo_track_reloc.h"

namespace {

// device memory for count elements, recorded in got (whose owner frees it); a no-op once *rc holds an error
template <typename T>
void trk_alloc(svo_hip_ctx* ctx, std::vector<void*>* got, int* rc, T** p, size_t count) {
  if (*rc != SVO_HIP_OK) return;
  void* d = nullptr;
  *rc = svo_hip_malloc(ctx, &d, (count ? count : 1) * sizeof(T));
  *p = (T*)d;
  if (*rc == SVO_HIP_OK) got->push_back(d);
}

// The one wait of a call: every listed flag (page-locked memory, a kernel's last store) shows its sequence number.  A spin on host
// memory (no driver call on the way back; a few hundred milliseconds at most), then the stream's own synchronisation and the check.
struct TrkFlagWait { const char* flag; unsigned long long seq; };
int trk_wait_flags(svo_hip_ctx* ctx, const TrkFlagWait* w, int n, const char* who, const char* what) {
  auto done = [&](int k) {
    return __atomic_load_n(reinterpret_cast<const volatile unsigned long long*>(w[k].flag), __ATOMIC_ACQUIRE) == w[k].seq;
  };
  bool all = false;
  for (long spins = 0; spins < 4000000L && !all; ++spins) {
    all = true;
    for (int k = 0; k < n && all; ++k) all = done(k);
    if (!all) __builtin_ia32_pause();
  }
  if (!all) SVO_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < n; ++k)
    if (!done(k)) return svo_fail(ctx, SVO_HIP_ERR_DEVICE, who, what);
  return SVO_HIP_OK;
}

// feature_detector_->setExistingFeatures(frame->fts_) (S/depth_filter.cpp:132, feature_detection.cpp:47-56) for the device's last
// frame: every feature's cell, with or without a point (the pose refinement drops points, not features: pose_optimizer.cpp:154-157).
// The count is the one the device holds; one workgroup strides over it.
__global__ __launch_bounds__(256) void trk_mark_last_kernel(const int* __restrict__ n_last, const double* __restrict__ px, int cap,
                                                            int cell_size, int grid_cols, int n_cells, uint8_t* __restrict__ occupancy) {
  int n = n_last[0];
  if (n > cap) n = cap;
  for (int i = threadIdx.x; i < n; i += 256)
    svo_dev::grid_mark_cell(px[2 * (size_t)i], px[2 * (size_t)i + 1], cell_size, grid_cols, n_cells, occupancy);
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
  double* err_mult = nullptr;               // [n_cams] |fx| of every camera: the pose refinement's error multiplier (groups only)
  // the argument table of the chain's kernels (TrkCamArgs per camera): built on the host every call, uploaded when it changed
  std::vector<TrkCamArgs> args_next;
  TrkCamArgs* args_host = nullptr;          // page-locked: the bytes of the last upload
  TrkCamArgs* args_dev = nullptr;
  bool args_valid = false;                  // args_dev holds args_host
  // svo_hip_tracker_group_track_some: [0, n_cams) the cameras of the call, [n_cams, 2 n_cams) the ones that sit it out; sent with
  // every such call (the previous call's kernels are through with both copies: the host waited for them)
  int* list_host = nullptr;                 // page-locked
  int* list_dev = nullptr;
  TrkFinishReq* fin_host = nullptr;         // page-locked, mapped: the cameras' requests of svo_hip_tracker_group_finish_frames
  TrkFinishReq* fin_dev = nullptr;
  unsigned long long seq = 0;               // frames tracked: the hand-over kernel stores it behind every camera's block (o_flag)
  std::vector<svo_hip_tracker*> members;
  std::vector<TrkFlagWait> waits;           // [n_cams] the flags a call waits for (no allocation per frame)
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
  bool have_map = false;
  bool any_edgelet = false;                 // the map holds EDGELET reference features (align1D stage needed)
  // plan / replay scratch
  TrkPlan pl{};
  TrkFeat ft{};
  TrkLast last{};
  int *cell_winner = nullptr, *cell_cum = nullptr;

  // ---- What the host knows about the device's last frame.  Entry points read these fields; only the transitions below, each named
  // after what happened, write them (behind every field: the transitions that set it / that clear it).
  bool have_last = false;        // the device holds a last frame whose point indices fit the map.  host_set_last; map_accepted may clear it
  int last_n_host = 0;           // its number of features.  host_set_last, frame_tracked
  bool last_from_track = false;  // it is the previous call's new frame, its features are in the result block.  frame_tracked / host_set_last
  bool last_renumbered = false;  // ... under the numbering a compaction has replaced since.  points_renumbered; cleared with last_from_track
  int last_max_point = -1;       // largest map point it refers to where the block does not say it (last_point_bound).  host_set_last, points_renumbered
  int track_n_points = 0;        // n_points when it was tracked: the layout of the counters in the result block.  frame_tracked
  bool need_gather = true;       // the solver's slot holds something else.  host_set_last, map_replaced, positions_changed, call_failed / frame_tracked
  bool overlap_valid = false;    // pl.overlap_kf / counters[3] are the last frame's and still name keyframes of the map (the keyframe decision).
                                 // frame_tracked / frame_begins, host_set_last, map_replaced, keyframes_renumbered
  bool rekey_pending = false;    // deleted points took key features along: the keyframes choose again before the tables are read.
                                 // frame_tracked, keyframes_renumbered / rekeyed (trk_rekey_now), map_replaced
  // the host gave the last frame, or made it from a keyframe: n features, none above map point max_point
  void host_set_last(int n, int max_point) {
    have_last = true; last_n_host = n; last_max_point = max_point; last_from_track = false; last_renumbered = false;
    need_gather = true; overlap_valid = false;
  }
  void gate_refused() { host_set_last(0, -1); }    // a relocalisation's gate turned the keyframe down: the new image, no features
  void frame_begins() { overlap_valid = false; }   // a chain is being enqueued: its plan rewrites the overlap list
  // the chain has completed: the new frame is the last one, the hand-over kernel has written the solver's slot
  void frame_tracked(const svo_hip_track_result& r) {
    last_n_host = r.n_features; track_n_points = n_points; last_from_track = true; last_renumbered = false;
    need_gather = false; overlap_valid = true;
    if (r.map_changed) rekey_pending = true;
  }
  // largest map point the last frame refers to: from the features of a tracked frame while their numbering holds
  int last_point_bound() const {
    if (!last_from_track || last_renumbered) return last_max_point;
    const int32_t* fp = reinterpret_cast<const int32_t*>(res_host + o_point);
    int max_point = -1;
    for (int i = 0; i < last_n_host; ++i) if (fp[i] > max_point) max_point = fp[i];
    return max_point;
  }
  // svo_hip_tracker_set_map, before its uploads: the last frame's features keep referring to map points by index, so a map with
  // fewer points than the largest of them needs svo_hip_tracker_set_last_frame again ...
  void map_accepted(int n_points_new) { if (have_last && last_point_bound() >= n_points_new) have_last = false; }
  // ... and behind them: the keyframes may be others now, point positions may have changed
  void map_replaced() { need_gather = true; overlap_valid = false; rekey_pending = false; }
  // a compaction: the device's last frame follows the new numbering; the result block (and track_n_points, its layout) keeps the old
  void points_renumbered(int max_point) { last_max_point = max_point; last_renumbered = last_from_track; }
  // a promotion (the frame is a keyframe of the map now) or a removal, which may delete points
  void keyframes_renumbered(bool points_deleted) { overlap_valid = false; if (points_deleted) rekey_pending = true; }
  void positions_changed() { need_gather = true; }   // the host wrote point positions: the solver's copy of the last frame's is stale
  void call_failed() { need_gather = true; }         // a relocalisation failed midway: whatever the slot holds is gathered again
  void rekeyed() { rekey_pending = false; }
  // the other per-camera objects
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
  t->rekeyed();
  return SVO_HIP_OK;
}

// SparseImgAlign(kltMaxLevel, kltMinLevel, 30, GaussNewton, false, false) (frame_handler_mono.cpp:186-187, :329-330)
svo_hip_sia_params trk_sia_params(const svo_hip_tracker_config& c) {
  svo_hip_sia_params sp;
  sp.max_level = c.klt_max_level; sp.min_level = c.klt_min_level; sp.n_iter = c.sia_n_iter; sp.eps = c.sia_eps; sp.early_stop = 1;
  return sp;
}

// the slot of the shared keyframe pyramids that holds this camera's keyframe slot
int trk_kf_slot(const svo_hip_tracker* t, int slot) { return t->cam_index * t->cfg.max_keyframes + slot; }

// the last frame's pyramid becomes a copy of that keyframe slot's
int trk_last_pyramid_from_keyframe(svo_hip_tracker* t, int slot) {
  svo_hip_pyramid* dst = t->sh->frame_pyr[t->sh->last_idx];
  const svo_hip_pyramid* kf = t->sh->kf_pyr;
  return svo_hip_copy_d2d(t->ctx, dst->base + (size_t)t->cam_index * dst->pyr_bytes, kf->base + (size_t)trk_kf_slot(t, slot) * kf->pyr_bytes,
                          dst->pyr_bytes);
}

// the context's two staging areas at `bytes`, free to be filled: the stream is through with whatever it still read from them
int trk_stage_upload(svo_hip_ctx* ctx, size_t bytes, char** dev, char** host) {
  int rc = svo_ctx_staging(ctx, bytes, dev);
  if (rc == SVO_HIP_OK) rc = svo_ctx_host_staging(ctx, bytes, host);
  if (rc != SVO_HIP_OK) return rc;
  SVO_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
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
  if (sh->list_host) (void)hipHostFree(sh->list_host);
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

// the shared part of n_cams cameras with one image size (`cam`: any of them) and one configuration
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
  if (rc == SVO_HIP_OK && hipHostMalloc((void**)&sh->list_host, 2 * N * sizeof(int), hipHostMallocDefault) != hipSuccess) rc = SVO_HIP_ERR_NOMEM;
  D(&sh->list_dev, 2 * N);
  if (rc == SVO_HIP_OK && hipHostMalloc((void**)&sh->fin_host, N * sizeof(TrkFinishReq), hipHostMallocMapped) != hipSuccess) rc = SVO_HIP_ERR_NOMEM;
  if (rc == SVO_HIP_OK && hipHostGetDevicePointer((void**)&sh->fin_dev, sh->fin_host, 0) != hipSuccess) rc = SVO_HIP_ERR_DEVICE;
  if (rc == SVO_HIP_OK) { sh->args_next.resize(N); sh->waits.resize(N); }
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
  if (rc == SVO_HIP_OK && hipHostMalloc((void**)&t->st_host, ST_BYTES, hipHostMallocMapped) != hipSuccess) rc = SVO_HIP_ERR_NOMEM;
  if (rc == SVO_HIP_OK) memset(t->st_host, 0, ST_BYTES);
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
  return svo_hip_pyramid_upload_level0_and_build(t->sh->kf_pyr, trk_kf_slot(t, slot), level0);
}

int svo_hip_tracker_keyframe_from_last_frame(svo_hip_tracker* t, int slot) {
  if (!t) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = t->ctx;
  SVO_REQUIRE(ctx, slot >= 0 && slot < t->cfg.max_keyframes);
  if (!t->have_last) return svo_fail(ctx, SVO_HIP_ERR_STATE, "svo_hip_tracker_keyframe_from_last_frame", "no frame has been tracked or set yet");
  const svo_hip_pyramid* src = t->sh->frame_pyr[t->sh->last_idx];
  const svo_hip_pyramid* kf = t->sh->kf_pyr;
  return svo_hip_copy_d2d(ctx, kf->base + (size_t)trk_kf_slot(t, slot) * kf->pyr_bytes, src->base + (size_t)t->cam_index * src->pyr_bytes,
                          src->pyr_bytes);
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
  // what the tables below take in the staging area (each starts on a 16-byte boundary): checked before anything is written
  const size_t K = mp->n_kf, P = mp->n_points, O = (size_t)n_obs;
  const size_t need = K * (56 + 4 + 20) + (K + 1) * 4 + (size_t)n_ftr * 4 + P * (24 + 12) + (P + 1) * 4 + O * (4 + 16 + 24 + 4 + 1 + 16) +
                      (size_t)mp->n_candidates * 4 + (size_t)c.max_keyframes * 56 + 32 * 16;
  if (need > t->map_host_bytes) return svo_fail(ctx, SVO_HIP_ERR_NOMEM, "svo_hip_tracker_set_map", "staging area too small");
  t->map_accepted(mp->n_points);            // (after the checks: a refused map changes nothing)
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  // the staging area may still feed the copies of the previous upload
  SVO_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  char* hs = t->map_host;
  size_t off = 0;
  hipError_t e = hipSuccess;
  // the next `bytes` of the staging area (on a 16-byte boundary) to be filled, then sent
  auto stage = [&](size_t bytes) { off = (off + 15) & ~(size_t)15; char* p = hs + off; off += bytes; return p; };
  auto send = [&](void* dst, const void* p, size_t bytes) { if (e == hipSuccess) e = hipMemcpyAsync(dst, p, bytes, hipMemcpyHostToDevice, ctx->stream); };
  auto put = [&](void* dst, const void* src, size_t bytes) { if (bytes) { char* p = stage(bytes); memcpy(p, src, bytes); send(dst, p, bytes); } };
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
  double* ts = reinterpret_cast<double*>(stage((size_t)c.max_keyframes * 56));
  memset(ts, 0, (size_t)c.max_keyframes * 56);
  for (int s = 0; s < c.max_keyframes; ++s) ts[7 * s + 6] = 1.0;
  for (int k = 0; k < mp->n_kf; ++k) memcpy(ts + 7 * (size_t)mp->kf_slot[k], mp->T_kf_w + 7 * (size_t)k, 56);
  send(t->T_slot_w, ts, (size_t)c.max_keyframes * 56);
  if (n_obs) {
    uint8_t* ed = reinterpret_cast<uint8_t*>(stage((size_t)n_obs));
    if (mp->obs_edgelet) memcpy(ed, mp->obs_edgelet, (size_t)n_obs); else memset(ed, 0, (size_t)n_obs);
    send(tb.obs_edgelet, ed, (size_t)n_obs);
    double* gr = reinterpret_cast<double*>(stage((size_t)n_obs * 16));
    if (mp->obs_grad) memcpy(gr, mp->obs_grad, (size_t)n_obs * 16);
    else for (int o = 0; o < n_obs; ++o) { gr[2 * o] = 1.0; gr[2 * o + 1] = 0.0; }
    send(tb.obs_grad, gr, (size_t)n_obs * 16);
  }
  if (e == hipSuccess && P) e = hipMemsetAsync(t->pt_unlinked, 0, P, ctx->stream);
  if (e != hipSuccess) return svo_fail(ctx, SVO_HIP_ERR_DEVICE, "svo_hip_tracker_set_map", hipGetErrorString(e));
  t->n_kf = mp->n_kf; t->n_points = mp->n_points; t->n_candidates = mp->n_candidates;
  t->n_ftr = n_ftr; t->n_obs = n_obs;
  t->kf_slot_host.assign(mp->kf_slot, mp->kf_slot + mp->n_kf);
  t->any_edgelet = false;
  if (mp->obs_edgelet) for (int o = 0; o < n_obs && !t->any_edgelet; ++o) t->any_edgelet = mp->obs_edgelet[o] != 0;
  t->have_map = true;
  t->map_replaced();
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
  const int rc = trk_stage_upload(ctx, bytes, &d, &hs);
  if (rc != SVO_HIP_OK) return rc;
  memcpy(hs, pos, (size_t)n * 24);
  memcpy(hs + o_idx, point, (size_t)n * 4);
  SVO_CHECK_HIP(ctx, hipMemcpyAsync(d, hs, bytes, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(trk_scatter_positions_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, reinterpret_cast<const int*>(d + o_idx),
                     reinterpret_cast<const double*>(d), t->pt_pos);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  t->positions_changed();
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
  const int rc = level0 ? svo_hip_pyramid_upload_level0_and_build(t->sh->frame_pyr[t->sh->last_idx], t->cam_index, level0)
                        : trk_last_pyramid_from_keyframe(t, kf_slot);
  if (rc != SVO_HIP_OK) return rc;
  const int32_t n32 = n;
  SVO_CHECK_HIP(ctx, hipMemcpyAsync(t->last.n, &n32, 4, hipMemcpyHostToDevice, ctx->stream));
  SVO_CHECK_HIP(ctx, hipMemcpyAsync(t->last.T_f_w, T_f_w, 56, hipMemcpyHostToDevice, ctx->stream));
  if (n > 0) {
    SVO_CHECK_HIP(ctx, hipMemcpyAsync(t->last.px, px, (size_t)n * 16, hipMemcpyHostToDevice, ctx->stream));
    SVO_CHECK_HIP(ctx, hipMemcpyAsync(t->last.f, f, (size_t)n * 24, hipMemcpyHostToDevice, ctx->stream));
    SVO_CHECK_HIP(ctx, hipMemcpyAsync(t->last.point, point, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  }
  t->host_set_last(n, max_point);
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
  mf.n_pyr_levels = c.n_pyr_levels; mf.n_kf = c.max_keyframes; mf.n_ref_levels = c.n_levels;
  TrkCamArgs* an = sh->args_next.data();
  memset(an, 0, (size_t)N * sizeof(TrkCamArgs));
  for (int k = 0; k < N; ++k) {
    svo_hip_tracker* t = sh->members[(size_t)k];
    TrkCamArgs& a = an[k];
    a.m = make_map(t); a.pl = t->pl; a.ft = t->ft; a.last = t->last;
    a.mf = mf; a.mf.cam = svo_make_cam(t->cam); a.mf.slot_base = k * c.max_keyframes;
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
  for (int k = 0; k < N; ++k) sh->members[(size_t)k]->frame_begins();
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
  const svo_hip_sia_params sp = trk_sia_params(c);
  rc = svo_hip_sia_run(sh->sia, N, &sp);
  if (rc != SVO_HIP_OK) return rc;
  // ---- Reprojector::reprojectMap
  bool any_edgelet = false;
  for (int k = 0; k < N; ++k) {
    svo_hip_tracker* t = sh->members[(size_t)k];
    rc = trk_rekey_now(t);                    // Map::safeDeletePoint of the previous frame: Frame::removeKeyPoint on the keyframes
    if (rc != SVO_HIP_OK) return rc;
    any_edgelet = any_edgelet || t->any_edgelet;
  }
  SeedRec* recs = nullptr; uint32_t* pwb_t = nullptr; int n_pad = 0;           // the matcher's scratch
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
  // warp + align2D (+ align1D when a map holds edgelets) over every camera's candidates (these stages read the image size only)
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
                                       sh->ft_f, sh->ft_pos, sh->ft_level, sh->ft_has_point, fabs(t0->cam.fx), sh->err_mult, 1,
                                       c.pose_optim_thresh, c.pose_optim_num_iter, sh->po);
  if (rc != SVO_HIP_OK) return rc;
  // ---- hand-over + result: written straight into the page-locked blocks, the frame's sequence number last
  const unsigned long long seq = ++sh->seq;
  if (N == 1) hipLaunchKernelGGL(trk_finish_one_kernel, dim3(1), dim3(256), 0, ctx->stream, an[0], seq);
  else hipLaunchKernelGGL(trk_finish_cams_kernel, dim3(N), dim3(256), 0, ctx->stream, ad, seq);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  // the one synchronisation of the frame: every camera's sequence number
  for (int k = 0; k < N; ++k) {
    const svo_hip_tracker* t = sh->members[(size_t)k];
    sh->waits[(size_t)k] = {t->res_host + t->o_flag, seq};
  }
  rc = trk_wait_flags(ctx, sh->waits.data(), N, who, "the frame's kernels did not complete");
  if (rc != SVO_HIP_OK) return rc;
  sh->last_idx = 1 - sh->last_idx;          // the new frames' pyramids are the next call's references
  for (int k = 0; k < N; ++k) {
    svo_hip_tracker* t = sh->members[(size_t)k];
    t->frame_tracked(*reinterpret_cast<const svo_hip_track_result*>(t->res_host));
  }
  return SVO_HIP_OK;
}

// One frame for the n cameras cam[0..n) of the shared part (strictly increasing, in range, 0 < n < n_cams: the caller has checked);
// level0[j]: camera cam[j]'s new image.  The chain of trk_track_all with every stage launched n cameras wide: workgroup j, or
// slice j of a grid, takes camera cam[j] from the list in device memory, and no stage reads or writes anything of a camera that
// is not listed -- its counters row still holds its own last frame's counts, which the keyframe decision reads.
// The two frame batches: the new pyramids are built in the batch that is not the last frames'.  When at least half of the cameras
// track, the batches change roles as always and the pyramids of the cameras that sit out are copied forward (one launch);
// otherwise they keep their roles and the new pyramids are copied back behind the alignment and the matching, which read them.
// Either way every camera's last frame lies in frame_pyr[last_idx] afterwards, and the smaller side is what gets copied.
static int trk_track_some(svo_hip_tracker_shared* sh, int n, const int32_t* cam, const uint8_t* const* level0, const char* who) {
  svo_hip_ctx* ctx = sh->ctx;
  const int N = sh->n_cams;
  svo_hip_tracker* t0 = sh->members[0];
  const svo_hip_tracker_config& c = t0->cfg;
  for (int j = 0; j < n; ++j) {
    const svo_hip_tracker* t = sh->members[(size_t)cam[j]];
    if (!t->have_map || !t->have_last)
      return svo_fail(ctx, SVO_HIP_ERR_STATE, who, "svo_hip_tracker_set_map and svo_hip_tracker_set_last_frame come first (every camera of the call)");
  }
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  int* act = sh->list_host;
  int* rest = sh->list_host + N;
  int n_rest = 0;
  for (int k = 0, j = 0; k < N; ++k) {
    if (j < n && cam[j] == k) act[j++] = k;
    else rest[n_rest++] = k;
  }
  const int* act_dev = sh->list_dev;
  const int* rest_dev = sh->list_dev + N;
  const size_t l0 = (size_t)t0->cam.width * t0->cam.height;
  for (int j = 0; j < n; ++j) {
    svo_hip_tracker* t = sh->members[(size_t)act[j]];
    t->frame_begins();
    if (level0[j] != reinterpret_cast<const uint8_t*>(t->img_host)) memcpy(t->img_host, level0[j], l0);
  }
  // a failure from the first enqueue on: the stream is through with the list and the images before the call returns, and whatever
  // the half-run chain left in the solver's slots is gathered again
  auto fail = [&](int rc) {
    (void)hipStreamSynchronize(ctx->stream);
    for (int j = 0; j < n; ++j) sh->members[(size_t)act[j]]->call_failed();
    return rc;
  };
  if (hipMemcpyAsync(sh->list_dev, sh->list_host, 2 * (size_t)N * sizeof(int), hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
    return fail(svo_fail(ctx, SVO_HIP_ERR_DEVICE, who, "upload of the camera list failed"));
  svo_hip_pyramid* ref = sh->frame_pyr[sh->last_idx];
  svo_hip_pyramid* cur = sh->frame_pyr[1 - sh->last_idx];
  const bool flip = 2 * n >= N;
  int rc = svo_pyramid_build_slots(cur, n, act, act_dev, sh->img_dev, sh->img_stride);
  if (rc == SVO_HIP_OK && flip) rc = svo_pyramid_copy_slots(cur, ref, n_rest, rest, rest_dev);
  if (rc == SVO_HIP_OK) rc = svo_hip_sia_set_frames(sh->sia, ref, cur);
  bool any_edgelet = false;
  for (int j = 0; j < n && rc == SVO_HIP_OK; ++j) {
    svo_hip_tracker* t = sh->members[(size_t)act[j]];
    if (t->need_gather) rc = svo_sia_prepare_from_device(sh->sia, act[j], &t->cam, t->last_n_host, t->last.n, t->last.T_f_w, t->last.px, t->last.f, t->last.point, t->pt_pos);
    else rc = svo_sia_note_device_slot(sh->sia, act[j], &t->cam, t->last_n_host);
  }
  const svo_hip_sia_params sp = trk_sia_params(c);
  if (rc == SVO_HIP_OK) rc = svo_sia_run_slots(sh->sia, n, act, act_dev, &sp);
  // (a re-selection owed by a camera that sits out stays owed)
  for (int j = 0; j < n && rc == SVO_HIP_OK; ++j) {
    svo_hip_tracker* t = sh->members[(size_t)act[j]];
    rc = trk_rekey_now(t);
    any_edgelet = any_edgelet || t->any_edgelet;
  }
  SeedRec* recs = nullptr; uint32_t* pwb_t = nullptr; int n_pad = 0;
  const int stride = sh->rec_stride;
  if (rc == SVO_HIP_OK) rc = svo_match_scratch(ctx, N * stride, &recs, &pwb_t, &n_pad);     // (every camera keeps its own part: the table stays as it is)
  if (rc == SVO_HIP_OK) rc = trk_args_table(sh, recs);
  if (rc != SVO_HIP_OK) return fail(rc);
  const TrkCamArgs* ad = sh->args_dev;
  hipLaunchKernelGGL(trk_plan_listed_kernel, dim3(n), dim3(TRK_THREADS), 0, ctx->stream, ad, act_dev);
  if (hipGetLastError() != hipSuccess) return fail(svo_fail(ctx, SVO_HIP_ERR_DEVICE, who, "launch failed"));
  rc = svo_match_stages_cams(ctx, sh->kf_pyr, cur, &t0->cam, N, stride, sh->counters, 8, sh->cand_level_ref, recs, pwb_t, n_pad, c.n_pyr_levels,
                             c.align_max_iter, any_edgelet, act_dev, n);
  if (rc != SVO_HIP_OK) return fail(rc);
  hipLaunchKernelGGL(trk_replay_listed_kernel, dim3(n), dim3(TRK_THREADS), 0, ctx->stream, ad, act_dev, c.max_fts, c.quality_min_fts);
  if (hipGetLastError() != hipSuccess) return fail(svo_fail(ctx, SVO_HIP_ERR_DEVICE, who, "launch failed"));
  const FrameState* st0 = svo_sia_state_dev(sh->sia, 0);
  rc = svo_pose_optimize_batch_strided(ctx, N, c.max_frame_features, sh->counters + 5, 8, st0->T_cur_w, (int)(sizeof(FrameState) / sizeof(double)),
                                       sh->ft_f, sh->ft_pos, sh->ft_level, sh->ft_has_point, fabs(t0->cam.fx), sh->err_mult, 1,
                                       c.pose_optim_thresh, c.pose_optim_num_iter, sh->po, act_dev, n);
  if (rc == SVO_HIP_OK && !flip) rc = svo_pyramid_copy_slots(ref, cur, n, act, act_dev);
  if (rc != SVO_HIP_OK) return fail(rc);
  const unsigned long long seq = ++sh->seq;
  hipLaunchKernelGGL(trk_finish_listed_kernel, dim3(n), dim3(256), 0, ctx->stream, ad, act_dev, seq);
  if (hipGetLastError() != hipSuccess) return fail(svo_fail(ctx, SVO_HIP_ERR_DEVICE, who, "launch failed"));
  // the one synchronisation: the sequence number of the cameras of the call (the others keep an older one)
  for (int j = 0; j < n; ++j) {
    const svo_hip_tracker* t = sh->members[(size_t)act[j]];
    sh->waits[(size_t)j] = {t->res_host + t->o_flag, seq};
  }
  rc = trk_wait_flags(ctx, sh->waits.data(), n, who, "the frame's kernels did not complete");
  if (rc != SVO_HIP_OK) return fail(rc);
  if (flip) sh->last_idx = 1 - sh->last_idx;
  for (int j = 0; j < n; ++j) {
    svo_hip_tracker* t = sh->members[(size_t)act[j]];
    t->frame_tracked(*reinterpret_cast<const svo_hip_track_result*>(t->res_host));
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

// ---- a group of cameras: N trackers with one image size and one configuration, each with its own camera model, whose frames
// are tracked TOGETHER -- one chain of launches per call whatever N (every kernel of the chain takes one workgroup, or one slice
// of its grid, per camera, and reads the camera model of its entry of the argument table).
// Every camera keeps its own map, last frame and result block and is set up with the svo_hip_tracker_* functions of its
// handle (svo_hip_tracker_group_camera); only the per-frame call is the group's.
struct svo_hip_tracker_group {
  svo_hip_tracker_shared* sh = nullptr;
};

// camera k's model is cams[k * cam_stride]: stride 1 for a rig, 0 for the one model svo_hip_tracker_group_create repeats
static int trk_group_create(svo_hip_ctx* ctx, const svo_hip_camera* cams, int cam_stride, const svo_hip_tracker_config* cfg, int n_cameras,
                            svo_hip_tracker_group** out) {
  if (!ctx || !cfg || !out) return SVO_HIP_ERR_INVALID;
  *out = nullptr;
  // every refusal comes before the first allocation
  SVO_REQUIRE(ctx, cams != nullptr);
  SVO_REQUIRE(ctx, n_cameras >= 1 && n_cameras <= 1024);
  for (int k = 0; k < (cam_stride ? n_cameras : 1); ++k) {
    const int rc = trk_check_config(ctx, &cams[k], cfg);
    if (rc != SVO_HIP_OK) return rc;
    // the pyramid batches, the detector grid and the page-locked image blocks are shared and sized once
    SVO_REQUIRE(ctx, cams[k].width == cams[0].width && cams[k].height == cams[0].height);
  }
  // a block of the batched warp / alignment stages takes 16 candidates and must not straddle two cameras
  SVO_REQUIRE(ctx, n_cameras == 1 || cfg->max_items % 16 == 0);
  svo_hip_tracker_group* g = new (std::nothrow) svo_hip_tracker_group();
  if (!g) return SVO_HIP_ERR_NOMEM;
  int rc = trk_shared_create(ctx, &cams[0], cfg, n_cameras, &g->sh);
  for (int k = 0; k < n_cameras && rc == SVO_HIP_OK; ++k) {
    svo_hip_tracker* t = nullptr;
    rc = trk_member_create(g->sh, k, &cams[(size_t)k * cam_stride], cfg, &t);
    if (rc == SVO_HIP_OK) g->sh->members.push_back(t);
  }
  if (rc == SVO_HIP_OK && n_cameras > 1) {                 // (a group of one runs the lone tracker's chain: the scalar |fx|)
    std::vector<double> em((size_t)n_cameras);
    for (int k = 0; k < n_cameras; ++k) em[(size_t)k] = fabs(cams[(size_t)k * cam_stride].fx);
    trk_alloc(ctx, &g->sh->dev_allocs, &rc, &g->sh->err_mult, (size_t)n_cameras);
    if (rc == SVO_HIP_OK && (hipMemcpyAsync(g->sh->err_mult, em.data(), em.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
                             hipStreamSynchronize(ctx->stream) != hipSuccess))
      rc = svo_fail(ctx, SVO_HIP_ERR_DEVICE, "svo_hip_tracker_group_create", "upload of the cameras' error multipliers failed");
  }
  if (rc != SVO_HIP_OK) { svo_hip_tracker_group_destroy(g); return rc; }
  *out = g;
  return SVO_HIP_OK;
}

int svo_hip_tracker_group_create_rig(svo_hip_ctx* ctx, const svo_hip_camera* cams, const svo_hip_tracker_config* cfg, int n_cameras,
                                     svo_hip_tracker_group** out) {
  return trk_group_create(ctx, cams, 1, cfg, n_cameras, out);
}

// one camera model for all cameras: the rig with that model repeated
int svo_hip_tracker_group_create(svo_hip_ctx* ctx, const svo_hip_camera* cam, const svo_hip_tracker_config* cfg, int n_cameras,
                                 svo_hip_tracker_group** out) {
  return trk_group_create(ctx, cam, 0, cfg, n_cameras, out);
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

int svo_hip_tracker_group_track_some(svo_hip_tracker_group* g, int n_active, const int32_t* camera, const uint8_t* const* level0,
                                     svo_hip_track_result* results) {
  if (!g || !g->sh) return SVO_HIP_ERR_INVALID;
  svo_hip_tracker_shared* sh = g->sh;
  svo_hip_ctx* ctx = sh->ctx;
  const char* who = "svo_hip_tracker_group_track_some";
  const int N = sh->n_cams;
  // every refusal before anything is enqueued or changed
  SVO_REQUIRE(ctx, n_active >= 0 && n_active <= N);
  if (n_active == 0) return SVO_HIP_OK;
  SVO_REQUIRE(ctx, camera != nullptr && level0 != nullptr);
  for (int j = 0; j < n_active; ++j)
    SVO_REQUIRE(ctx, camera[j] >= 0 && camera[j] < N && (j == 0 || camera[j] > camera[j - 1]) && level0[j] != nullptr);
  // every camera (the list can only be the identity then): svo_hip_tracker_group_track's own launches
  const int rc = n_active == N ? trk_track_all(sh, level0, who) : trk_track_some(sh, n_active, camera, level0, who);
  if (rc != SVO_HIP_OK) return rc;
  if (results)
    for (int j = 0; j < n_active; ++j)
      trk_copy_out(sh->members[(size_t)camera[j]], results + j, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
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
  const int rc = trk_stage_upload(ctx, bytes, &d, &hs);
  if (rc != SVO_HIP_OK) return rc;
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
  t->keyframes_renumbered(false);
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
  // the keyframes that lost a key feature to a point deleted here choose again (Frame::removeKeyPoint), on the new rows,
  // before anything reads the key points
  t->keyframes_renumbered(out[0] > 0);
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
  t->points_renumbered(out[4]);
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
  const int rc = trk_last_pyramid_from_keyframe(t, t->kf_slot_host[(size_t)k]);
  t->host_set_last(o.n_feat, o.max_point);
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
  auto fail = [&](int rc) { (void)hipStreamSynchronize(ctx->stream); t->call_failed(); return rc; };
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
  const svo_hip_sia_params sp = trk_sia_params(t->cfg);
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
  t->gate_refused();
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

// the camera's block after the wait (decision: nullptr for the structure step alone)
static void trk_finish_copy_out(const svo_hip_tracker* t, int n, double* pos_out, int32_t* iters_out, svo_hip_kf_decision* decision) {
  if (n > 0) memcpy(pos_out, t->st_host, (size_t)n * 24);
  if (n > 0 && iters_out) memcpy(iters_out, t->st_host + ST_O_ITERS, (size_t)n * 4);
  if (decision) memcpy(decision, t->st_host + ST_O_DECISION, sizeof(*decision));
}

// trk_finish_frame_kernel for a lone camera (the tables by value: trk_plan_one_kernel says why)
static void trk_finish_frame_launch(svo_hip_tracker* t, const TrkStructSel& sel, int n_iter, int overlap_valid, double min_dist, unsigned long long seq) {
  hipLaunchKernelGGL(trk_finish_frame_kernel, dim3(1), dim3(FIN_THREADS), 0, t->ctx->stream, make_map(t), t->pt_pos, t->last, sel, n_iter,
                     t->pl.overlap_kf, t->pl.counters, overlap_valid, min_dist, t->st_dev, seq);
}

int svo_hip_tracker_optimize_structure(svo_hip_tracker* t, int n, const int32_t* point, int n_iter, double* pos_out, int32_t* iters_out) {
  if (!t) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = t->ctx;
  const char* who = "svo_hip_tracker_optimize_structure";
  // (the shape of the request, then the state, then the indices: the order this call has always refused in)
  SVO_REQUIRE(ctx, n >= 0 && n <= TRK_MAX_STRUCT && n_iter >= 0 && (n == 0 || (point && pos_out)));
  if (!t->have_map) return svo_fail(ctx, SVO_HIP_ERR_STATE, who, "no map has been set");
  if (n == 0) return SVO_HIP_OK;
  TrkStructSel sel;
  int rc = trk_finish_check(t, n, point, n_iter, pos_out, &sel);
  if (rc != SVO_HIP_OK) return rc;
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  const unsigned long long seq = ++t->st_seq;
  hipLaunchKernelGGL(trk_structure_kernel, dim3(1), dim3(256), 0, ctx->stream, make_map(t), t->pt_pos, t->last, sel, n_iter,
                     reinterpret_cast<double*>(t->st_dev), reinterpret_cast<int*>(t->st_dev + ST_O_ITERS),
                     reinterpret_cast<unsigned long long*>(t->st_dev + ST_O_FLAG), seq);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  const TrkFlagWait w = {t->st_host + ST_O_FLAG, t->st_seq};
  rc = trk_wait_flags(ctx, &w, 1, who, "the kernel did not complete");
  if (rc != SVO_HIP_OK) return rc;
  trk_finish_copy_out(t, n, pos_out, iters_out, nullptr);
  // (the point table and the solver's copy of the last frame's points were updated by the kernel: nothing to gather)
  return SVO_HIP_OK;
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
  trk_finish_frame_launch(t, sel, n_iter, t->overlap_valid ? 1 : 0, kf_select_min_dist, ++t->st_seq);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  const TrkFlagWait w = {t->st_host + ST_O_FLAG, t->st_seq};
  rc = trk_wait_flags(ctx, &w, 1, who, "the kernel did not complete");
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
  // every camera's request as the kernel takes it, before anything is enqueued or written
  std::vector<TrkFinishReq> reqs((size_t)N);
  int n_active = 0;
  for (int k = 0; k < N; ++k) {
    svo_hip_tracker* t = sh->members[(size_t)k];
    const svo_hip_structure_request none = {0, nullptr, 0, nullptr, nullptr};
    const svo_hip_structure_request& r = req ? req[k] : none;
    TrkFinishReq& q = reqs[(size_t)k];
    memset(&q, 0, sizeof(q));
    if (!t->have_map || !t->have_last) {                                       // the camera sits out
      SVO_REQUIRE(ctx, r.n == 0);
      continue;
    }
    const int rc = trk_finish_check(t, r.n, r.point, r.n_iter, r.pos_out, &q.sel);
    if (rc != SVO_HIP_OK) return rc;
    q.active = 1; q.n_iter = r.n_iter; q.overlap_valid = t->overlap_valid ? 1 : 0; q.st = t->st_dev;
    ++n_active;
  }
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  for (int k = 0; k < N; ++k) { camera_ok[k] = 0; memset(&decisions[k], 0, sizeof(svo_hip_kf_decision)); }
  if (n_active == 0) return SVO_HIP_OK;
  // (the previous call's kernel is through with the requests: the host waited for it)
  for (int k = 0, w = 0; k < N; ++k) {
    svo_hip_tracker* t = sh->members[(size_t)k];
    if (reqs[(size_t)k].active) { reqs[(size_t)k].seq = ++t->st_seq; sh->waits[(size_t)w++] = {t->st_host + ST_O_FLAG, t->st_seq}; }
    sh->fin_host[k] = reqs[(size_t)k];
  }
  // a failure from here on: the stream is through with the staging areas before the call returns
  auto fail = [&](int rc) { (void)hipStreamSynchronize(ctx->stream); return rc; };
  SeedRec* recs = nullptr; uint32_t* pwb_t = nullptr; int n_pad = 0;           // the matcher's scratch
  int rc = svo_match_scratch(ctx, N * sh->rec_stride, &recs, &pwb_t, &n_pad);      // (the records' address is part of the table)
  if (rc == SVO_HIP_OK) rc = trk_args_table(sh, recs);
  if (rc != SVO_HIP_OK) return fail(rc);
  if (N == 1) {
    const TrkFinishReq& r = sh->fin_host[0];
    trk_finish_frame_launch(sh->members[0], r.sel, r.n_iter, r.overlap_valid, kf_select_min_dist, r.seq);
  } else {
    hipLaunchKernelGGL(trk_finish_frames_cams_kernel, dim3(N), dim3(FIN_THREADS), 0, ctx->stream, sh->args_dev, sh->fin_dev, kf_select_min_dist);
  }
  if (hipGetLastError() != hipSuccess) return fail(svo_fail(ctx, SVO_HIP_ERR_DEVICE, who, "launch failed"));
  rc = trk_wait_flags(ctx, sh->waits.data(), n_active, who, "the kernel did not complete");
  if (rc != SVO_HIP_OK) return fail(rc);
  for (int k = 0; k < N; ++k) {
    svo_hip_tracker* t = sh->members[(size_t)k];
    if (!sh->fin_host[k].active) continue;
    camera_ok[k] = 1;
    trk_finish_copy_out(t, sh->fin_host[k].sel.n, req ? req[k].pos_out : nullptr, req ? req[k].iters_out : nullptr, &decisions[k]);
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

int svo_hip_tracker_mark_last_frame(svo_hip_tracker* t, int cell_size, int grid_cols, int grid_rows, uint8_t* occupancy_dev) {
  if (!t) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = t->ctx;
  const char* who = "svo_hip_tracker_mark_last_frame";
  SVO_REQUIRE(ctx, occupancy_dev && cell_size > 0 && grid_cols > 0 && grid_rows > 0);
  SVO_REQUIRE(ctx, (long long)grid_cols * grid_rows < (1ll << 31));
  if (!t->have_last) return svo_fail(ctx, SVO_HIP_ERR_STATE, who, "the device holds no last frame");
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(trk_mark_last_kernel, dim3(1), dim3(256), 0, ctx->stream, t->last.n, t->last.px, t->cfg.max_frame_features, cell_size,
                     grid_cols, grid_cols * grid_rows, occupancy_dev);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  // the grid usually belongs to the depth filter's context: its stream may read the marks once this call has returned
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

int svo_hip_tracker_last_frame_pyramid(svo_hip_tracker* t, const svo_hip_pyramid** pyr, int* slot) {
  if (!t) return SVO_HIP_ERR_INVALID;
  SVO_REQUIRE(t->ctx, pyr && slot);
  if (!t->have_last) return svo_fail(t->ctx, SVO_HIP_ERR_STATE, "svo_hip_tracker_last_frame_pyramid", "the tracker has no last frame");
  *pyr = t->sh->frame_pyr[t->sh->last_idx];
  *slot = t->cam_index;
  return SVO_HIP_OK;
}

}  // extern "C"
