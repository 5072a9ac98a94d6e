// svo_track_types.h -- the tracking chain's constants and the structs its kernels and the host half of svo_track.hip share:
// the map as index tables, the scratch of the stages, the last frame, a camera's kernel arguments.  The svo_track_*.h headers are the
// parts of that ONE translation unit (anonymous namespace, `using namespace` at header scope): nothing else may include them.
#pragma once
#include "svo_internal.h"
#include "svo_match_device.h"
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

struct TrkStructSel { int n; int point[TRK_MAX_STRUCT]; };   // the points the host selected for the structure step
// a camera's page-locked block of the structure step and the keyframe decision: [pos 64 x 3][iters 64][flag][decision]
constexpr size_t ST_O_ITERS = TRK_MAX_STRUCT * 24, ST_O_FLAG = ST_O_ITERS + TRK_MAX_STRUCT * 4, ST_O_DECISION = ST_O_FLAG + 64;
constexpr size_t ST_BYTES = ST_O_DECISION + 128;
static_assert(sizeof(svo_hip_kf_decision) <= 128, "the decision fits its part of the block");

// one camera's arguments of the chain's kernels: an entry of the table in device memory, or passed by value (a lone tracker)
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

// svo_hip_tracker_group_finish_frames: workgroup c finishes camera c's frame.  The tables come from the chain's argument table, what
// changes with every call from a page-locked array the kernel reads directly (a camera that sits out: active == 0).
struct TrkFinishReq {
  TrkStructSel sel;
  int n_iter, active, overlap_valid, pad;
  char* st;                            // the camera's page-locked block (device address)
  unsigned long long seq;
};

constexpr int RELOC_THREADS = 256;      // trk_reloc_kernel, what it is asked and what it reports
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
}  // namespace
