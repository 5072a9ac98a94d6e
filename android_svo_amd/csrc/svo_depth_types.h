// svo_depth_types.h -- the depth filter's constants and the structs its kernels and the host half of svo_depth.hip share: the
// frame-level constants of a pass, a keyframe's transforms, the jobs of a grouped pass in their two forms (DfGroup for the kernel
// arguments, DfCamJob / DfCamModel for a table in device memory; the job sources over them, DfGroupJobs and DfTableJobs, are in
// svo_depth_events.h beside the kernels written over them), the header of the event block.  The
// svo_depth_*.h headers are the parts of that ONE translation unit (anonymous namespace, `using namespace` at header scope):
// nothing else may include them.
#pragma once
#include "svo_align_device.h"
#include <cstddef>

#include "svo_internal.h"
#include "svo_match_device.h"
using namespace svo_dev;
namespace {
constexpr int ZMSSD_THRESHOLD = 2000 * 64;     // I/patch_score.h:46

// align2D / align1D: one DPP quad per patch, 16 patches per single-wave workgroup (svo_depth_align.h)
constexpr int ALIGN_BLOCK = 64;
constexpr int ALIGN_PATCHES = ALIGN_BLOCK / ALIGN_LANES_PER_PATCH;     // patches per workgroup
constexpr int ALIGN_STAGE_ROUNDS = (ALIGN_PATCHES * 25 + ALIGN_BLOCK - 1) / ALIGN_BLOCK;
constexpr int ALIGN_STAGE_WORDS = ALIGN_STAGE_ROUNDS * ALIGN_BLOCK;   // >= ALIGN_PATCHES * 25: no bounds test while staging

// the search stage: four seeds per wave, 16 per 256-thread block (svo_depth_search.h)
constexpr int SEEDS_PER_WAVE = 4;
constexpr int SEEDS_PER_BLOCK = 16;

struct SeedState { float a, b, mu, z_range, sigma2; };

struct Vec3 { double v[3]; };

// the transforms between one reference keyframe and the current frame
struct DfPoses {
  double T_ref_cur[7];       // it->ftr->frame->T_f_w_ * frame->T_f_w_.inverse()   (depth_filter.cpp:264)
  double T_cur_ref_vis[7];   // T_ref_cur.inverse()                                (:265)
  double T_cur_ref[7];       // cur.T_f_w_ * ref.T_f_w_.inverse()                  (matcher.cpp:216)
  double T_ref_inv[7];       // ref.T_f_w_.inverse()                                (:314)
};

struct DfFrame {
  Cam cam;
  DfPoses T;
  double px_error_angle;
  size_t ref_level_off[SVO_HIP_MAX_LEVELS];
  size_t cur_level_off[SVO_HIP_MAX_LEVELS];
  int n_pyr_levels, align_max_iter, max_epi_search_steps;
  int keep_px_on_failure;    // findMatchDirect writes px_scaled back even when align fails (matcher.cpp:200)
  double conv_thresh;
};

struct EvHeader { int32_t n_events; int32_t counts[7]; };

// The events, ascending seed index (56 B records).  A handful of them -- every frame but a keyframe's -- goes straight into
// the page-locked host block (no copy, no second wait); more than EV_DIRECT_MAX are packed in device memory and fetched
// with one transfer after the wait (scattered 56-byte stores over the link run at a few GB/s: 100 k events took 1.4 ms).
constexpr int EV_DIRECT_MAX = 512;

// ---- one launch set for one or SEVERAL batches (svo_hip_seed_batch_update[_group]_async; a single batch is a group of one) --
// A frame of the reference's depth filter updates the seeds of a few keyframes, a few hundred each: one launch set per batch
// is six launches of a handful of workgroups -- launch-bound (4 x 500 seeds: 105 us, profiles/r04_df_realistic_sizes.txt).  Here
// the batches of a frame go through the stages together: batch j owns the blocks [first_block, first_block + n_blocks) of the
// thread-per-seed stages (a block never straddles two batches, so the batch -- its arrays, its keyframe's transforms -- is
// block-uniform and lives in scalar registers), its records sit at first_block * 256 of the pass's scratch, the tail of its
// last block is filled with inert records, and the pixel stages (search, align) run over the concatenation unchanged: a
// record carries its keyframe's pyramid slot (SeedRec::pad).
constexpr int DF_GROUP_MAX = 8;
struct DfJob {
  DfPoses T;                 // of this batch's keyframe
  const double *px, *f;
  const int32_t* level;
  float *a, *b, *mu;
  const float* z_range;
  float* sigma2;
  int32_t* status;
  double *xyz, *px_cur;
  uint8_t* alive;
  int *block_count, *hist;
  EvHeader* header;
  svo_hip_seed_event *events_host, *events_dev;
  int n, n_blocks, first_block, ref_slot;
};
struct DfGroup {
  DfJob job[DF_GROUP_MAX];
  int n_jobs, report_updated;
};
// DfPoses sits where the four double[7] sat: the layout of the kernel arguments is what it was
static_assert(sizeof(DfPoses) == 4 * 7 * sizeof(double) && offsetof(DfPoses, T_cur_ref_vis) == 56 && offsetof(DfPoses, T_cur_ref) == 112 &&
              offsetof(DfPoses, T_ref_inv) == 168, "four transforms back to back");
static_assert(offsetof(DfFrame, T) == sizeof(Cam) && offsetof(DfFrame, px_error_angle) == sizeof(Cam) + sizeof(DfPoses) &&
              sizeof(DfFrame) == sizeof(Cam) + sizeof(DfPoses) + 8 + 2 * 8 * SVO_HIP_MAX_LEVELS + 4 * 4 + 8, "DfFrame layout");
static_assert(offsetof(DfJob, T) == 0 && offsetof(DfJob, px) == sizeof(DfPoses) && sizeof(DfJob) == sizeof(DfPoses) + 17 * 8 + 4 * 4,
              "DfJob layout");

// ---- one launch set for the batches of SEVERAL cameras (svo_hip_seed_batch_update_cameras_async) ---------------------------
// The jobs do not travel as kernel arguments: a table of them lies in device memory, and beside it a map from every 256-record
// block of the pass to its job.  A job is a DfJob plus what a DfGroup holds once for all its jobs and a pass holds once for all
// its batches: whether the job's camera reports its updated seeds, and the slot of its camera's current image.  Job
// boundaries are multiples of 256 records, so a 16-record search block or a 16-patch align block lies inside one job too.
// The cameras of the pass may each have their own model (svo_hip_seed_batch_update_rig_async; the image size is common): a table
// of them lies behind the block map, and a job names its camera's entry.  What a pass derives from the camera model travels
// with it, so the kernels read `cam` and `px_error_angle` of their job's entry where the other passes read them from the
// DfFrame; the entry is block-uniform like the job.
struct DfCamJob {
  DfJob job;
  int cur_slot, report_updated;
  int cam, pad_;             // entry of the pass's camera table
};
struct DfCamModel {
  Cam cam;
  double px_error_angle;     // 2 atan(1 / (2 |fx|))   (depth_filter.cpp:245-247)
};
static_assert(sizeof(DfCamJob) == sizeof(DfJob) + 16 && sizeof(DfCamJob) % 8 == 0, "DfCamJob layout");
static_assert(sizeof(DfCamModel) == sizeof(Cam) + 8 && sizeof(DfCamModel) % 8 == 0, "DfCamModel layout");

constexpr int DF_SMALL_MAX = 16384;                      // upper limit of svo_hip_df_set_small_pass_limit

// the batches of one svo_hip_seed_batch_mark_updated launch: batch j owns the blocks [first_block, first_block + ceil(n / 256))
struct MarkJob { const int32_t* status; const double* px_cur; int n, first_block; };
struct MarkGroup { MarkJob job[DF_GROUP_MAX]; int n_jobs; };
}  // namespace
