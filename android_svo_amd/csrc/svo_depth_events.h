// svo_depth_events.h -- what the host hears of a pass, in seed order: the converged-seed records of the multi-GPU gather and the
// events of a device-resident seed batch, with the grouped and small-pass kernels that produce them.  One block scan, one
// ordered rank, one event rule and one event record, shared by the large-pass and small-pass forms; each of those kernels is
// written once over a job source (DfGroupJobs: the jobs in the kernel arguments; DfTableJobs: a job table in device memory).
#pragma once
#include "svo_depth_seed.h"
#include "svo_depth_search.h"
#include "svo_depth_align.h"
namespace {
// ---- ordered compaction: count per 256-item block, scan the counts, scatter by rank ----------------------------------------
// inclusive scan of v over the lanes of a wave
SVO_DEV int wave_scan_inclusive(int v) {
  int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if ((int)(threadIdx.x & 63) >= o) incl += t; }
  return incl;
}

// exclusive scan of the block counts in place, one workgroup of 1024; every thread gets the total.  Wave-level scans by lane
// shuffles and one pass over the 16 wave totals per 1024 counts (round 3: a Hillis-Steele scan in LDS, 20 barriers per 1024
// counts: 8.3 us for the 3 907 blocks of 1 M seeds)
SVO_DEV void block_scan_counts(int n_blocks, int* __restrict__ block_count, int* total) {
  __shared__ int s_part[16];
  __shared__ int s_carry;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  for (int base = 0; base < n_blocks; base += 1024) {
    const int k = base + threadIdx.x;
    const int v = k < n_blocks ? block_count[k] : 0;
    const int incl = wave_scan_inclusive(v);
    if ((threadIdx.x & 63) == 63) s_part[threadIdx.x >> 6] = incl;
    __syncthreads();
    int wave_off = 0;
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) wave_off += s_part[w];
    const int carry = s_carry;
    if (k < n_blocks) block_count[k] = carry + wave_off + incl - v;
    __syncthreads();
    if (threadIdx.x == 1023) s_carry = carry + wave_off + incl;
    __syncthreads();
  }
  *total = s_carry;
}

// rank of this thread among the flagged threads of its block, in thread order; every thread of the block calls it (one barrier).
// s_w: one int per wave of the block.  A workgroup that holds several 256-item blocks passes the first wave of the thread's
// own block as wave0.
SVO_DEV int ordered_rank_in_block(bool flag, int* s_w, int wave0 = 0) {
  const unsigned long long m = __ballot(flag);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s_w[wave] = __popcll(m);
  __syncthreads();
  int rank = __popcll(m & ((1ull << lane) - 1ull));
  for (int w = wave0; w < wave; ++w) rank += s_w[w];
  return rank;
}

// the batch that owns block `block` of a grouped launch (DfGroup, MarkGroup: batch j owns the blocks from job[j].first_block on)
template <class Group>
SVO_DEV int job_of_block(const Group& g, int block) {
  int j = 0;
#pragma unroll
  for (int k = 1; k < DF_GROUP_MAX; ++k) if (k < g.n_jobs && block >= g.job[k].first_block) j = k;
  return j;
}

// ---- the events of a device-resident seed batch (svo_hip_seed_batch_*) -----------------------------------------------------
// The HOST has to hear about converged and NaN seeds (callback / erase, depth_filter.cpp:310-337: the reference erases these,
// :330, :336) and, on keyframes (report_updated), about every updated seed (its px_cur marks the detector grid, :302-306).
SVO_DEV bool seed_gone(int st) { return st == SVO_HIP_SEED_CONVERGED || st == SVO_HIP_SEED_NAN; }
SVO_DEV bool seed_event_wanted(int st, int report_updated) { return seed_gone(st) || (report_updated && st >= SVO_HIP_SEED_UPDATED); }

SVO_DEV svo_hip_seed_event make_seed_event(int i, int st, const float* __restrict__ mu, const float* __restrict__ sigma2,
                                           const double* __restrict__ xyz, const double* __restrict__ px_cur) {
  svo_hip_seed_event e;
  e.index = i; e.status = st; e.mu = mu[i]; e.sigma2 = sigma2[i];
  const bool conv = st == SVO_HIP_SEED_CONVERGED;
  e.xyz_world[0] = conv ? xyz[3 * (size_t)i] : 0.0; e.xyz_world[1] = conv ? xyz[3 * (size_t)i + 1] : 0.0; e.xyz_world[2] = conv ? xyz[3 * (size_t)i + 2] : 0.0;
  e.px_cur[0] = px_cur[2 * (size_t)i]; e.px_cur[1] = px_cur[2 * (size_t)i + 1];
  return e;
}

// The finalize stage also counts, per block, the seeds with an event, clears their `alive` flag where the reference erases
// them, and adds the block's status histogram to ev_hist[8] (slot status + 1; slot 0 = erased).
// (every thread of the 256-thread block calls it; `block` = the block's index within the batch)
SVO_DEV void df_finalize_events(int st, int i, int n, int block, uint8_t* __restrict__ alive, int report_updated,
                                int* __restrict__ ev_block_count, int* __restrict__ ev_hist) {
  const bool ev = seed_event_wanted(st, report_updated);
  if (seed_gone(st)) alive[i] = 0;
  __shared__ int s_ev[4];
  __shared__ int s_hist[8];
  if (threadIdx.x < 8) s_hist[threadIdx.x] = 0;
  __syncthreads();
  const unsigned long long m = __ballot(ev);
  if ((threadIdx.x & 63) == 0) s_ev[threadIdx.x >> 6] = __popcll(m);
  if (i < n) atomicAdd(&s_hist[st + 1], 1);
  __syncthreads();
  if (threadIdx.x == 0) ev_block_count[block] = s_ev[0] + s_ev[1] + s_ev[2] + s_ev[3];
  if (threadIdx.x < 8 && s_hist[threadIdx.x]) atomicAdd(&ev_hist[threadIdx.x], s_hist[threadIdx.x]);
}

// ---- ordered compaction of the converged seeds into packed records (the payload of the multi-GPU gather) ----
// record = {seed id, mu, sigma2, x, y, z} as f64; order = ascending seed index (the order of the reference's callbacks)
__global__ __launch_bounds__(256) void conv_count_kernel(int n, const int32_t* __restrict__ status, int* __restrict__ block_count) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool c = i < n && status[i] == SVO_HIP_SEED_CONVERGED;
  const unsigned long long m = __ballot(c);
  __shared__ int s_w[4];
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) block_count[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// the block counts become block offsets, one workgroup; total -> *count
__global__ __launch_bounds__(1024) void conv_scan_kernel(int n_blocks, int* __restrict__ block_count, int* __restrict__ count) {
  int total;
  block_scan_counts(n_blocks, block_count, &total);
  if (threadIdx.x == 0) *count = total;
}

__global__ __launch_bounds__(256) void conv_scatter_kernel(int n, long long id_offset, const int32_t* __restrict__ status,
                                                           const float* __restrict__ mu, const float* __restrict__ sigma2,
                                                           const double* __restrict__ xyz, const int* __restrict__ block_offset,
                                                           double* __restrict__ records) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool c = i < n && status[i] == SVO_HIP_SEED_CONVERGED;
  __shared__ int s_w[4];
  const int rank = ordered_rank_in_block(c, s_w);
  if (!c) return;
  const int off = block_offset[blockIdx.x] + rank;
  double* r = records + 6 * (size_t)off;
  r[0] = (double)(id_offset + i); r[1] = (double)mu[i]; r[2] = (double)sigma2[i];
  r[3] = xyz[3 * (size_t)i]; r[4] = xyz[3 * (size_t)i + 1]; r[5] = xyz[3 * (size_t)i + 2];
}
// up to `cap` of the packed records and the clamped count into this rank's block of the gather buffers
__global__ void records_clamp_copy_kernel(const double* __restrict__ rec, const int* __restrict__ count, int cap,
                                          double* __restrict__ dst, int32_t* __restrict__ dst_count) {
  const int n = min(*count, cap);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 6 * n; i += gridDim.x * blockDim.x) dst[i] = rec[i];
  if (blockIdx.x == 0 && threadIdx.x == 0) *dst_count = *count;      // the true count: > cap tells the caller about the overflow
}

// the geometry of seed i of batch J into record r of the pass
SVO_DEV void df_geometry_job_seed(const DfFrame& fr, const Cam& cam, const DfJob& J, int i, size_t r, SeedRec* __restrict__ recs,
                                  int32_t* __restrict__ level_cat) {
  if (i < J.n) {
    level_cat[r] = J.level[i];
    df_geometry_seed<false>(cam, J.T.T_cur_ref_vis, J.T.T_cur_ref, fr.n_pyr_levels, fr.max_epi_search_steps, J.ref_slot, i, J.n, J.px, J.f,
                            J.level, J.mu, J.sigma2, nullptr, nullptr, recs + r, J.alive);
  } else {                                                 // the tail of the batch's last block: records no stage touches
    SeedRec rc = md_dead_record();
    rc.status = SVO_HIP_SEED_ERASED;
    recs[r] = rc;
    level_cat[r] = 0;
  }
}

// ---- where a block of a resident-batch pass finds its job ------------------------------------------------------------------
// The grouped and small-pass kernels below are written once over a job source, and instantiated for the two there are.  A
// source answers, for a 256-record block or a job index: which job, its DfJob, its report_updated, its camera's model and
// px_error_angle, its current image.  All of it is block-uniform; the kernels take what they need of it BEFORE THEIR FIRST
// STORE, so that it is read on the scalar side.
// DfGroupJobs: the jobs travel in the kernel arguments (svo_hip_seed_batch_update[_group]_async): at most DF_GROUP_MAX batches of
// one camera, whose model is the DfFrame's and whose current image is one pointer.
struct DfGroupJobs {
  DfGroup g;
  const uint8_t* cur_pyr;
  SVO_DEV int of_block(int block) const { return job_of_block(g, block); }
  SVO_DEV const DfJob& job(int j) const { return g.job[j]; }
  SVO_DEV int report_updated(int) const { return g.report_updated; }
  SVO_DEV const Cam& cam(const DfFrame& fr, int) const { return fr.cam; }
  SVO_DEV double px_error_angle(const DfFrame& fr, int) const { return fr.px_error_angle; }
  SVO_DEV const uint8_t* cur_image(int) const { return cur_pyr; }
};
static_assert(sizeof(DfFrame) + sizeof(DfGroupJobs) + 64 <= 4096, "kernel arguments of the grouped stages");
// DfTableJobs: the jobs lie in a table in device memory (svo_hip_seed_batch_update_cameras_async / _rig_async, DfCamJob in
// svo_depth_types.h): a block finds its job with one load from the block -> job map; the job names its camera's entry of the
// camera table and the slot of its camera's current image.  DfFrame::T, ::cam and ::px_error_angle are not read.  With one
// model in every entry that is a grouped pass per camera, bit for bit (tests/test_gpu_seed_cameras.py); with a model per camera
// every batch equals a grouped pass with its camera's model (tests/test_gpu_seed_rig.py).
// No kernel writes the table, so its pointers are to the constant address space: the table's entries stay scalar-side loads after
// a kernel's stores, which a plain pointer inside a struct (it cannot be __restrict__) would not give.
template <class T> using DfFixed = const __attribute__((address_space(4))) T*;
struct DfTableJobs {
  DfFixed<DfCamJob> jobs;
  DfFixed<int> block_job;
  DfFixed<DfCamModel> cams;
  const uint8_t* cur_base;
  size_t cur_pyr_bytes;
  SVO_DEV const DfCamJob& entry(int j) const { return *(const DfCamJob*)(jobs + j); }
  SVO_DEV const DfCamModel& model(int j) const { return *(const DfCamModel*)(cams + jobs[j].cam); }
  SVO_DEV int of_block(int block) const { return block_job[block]; }
  SVO_DEV const DfJob& job(int j) const { return entry(j).job; }
  SVO_DEV int report_updated(int j) const { return jobs[j].report_updated; }
  SVO_DEV const Cam& cam(const DfFrame&, int j) const { return model(j).cam; }
  SVO_DEV double px_error_angle(const DfFrame&, int j) const { return model(j).px_error_angle; }
  SVO_DEV const uint8_t* cur_image(int j) const { return cur_base + (size_t)jobs[j].cur_slot * cur_pyr_bytes; }
};

template <class Jobs>
__global__ __launch_bounds__(256) void df_geometry_jobs_kernel(DfFrame fr, Jobs jobs, SeedRec* __restrict__ recs, int32_t* __restrict__ level_cat) {
  const int j = jobs.of_block(blockIdx.x);
  const DfJob& J = jobs.job(j);
  const Cam cam = jobs.cam(fr, j);
  const int i = (blockIdx.x - J.first_block) * 256 + threadIdx.x;       // seed of its batch
  if (i < 8) J.hist[i] = 0;
  df_geometry_job_seed(fr, cam, J, i, (size_t)blockIdx.x * 256 + threadIdx.x, recs, level_cat);
}

template <class Jobs>
__global__ __launch_bounds__(256) void df_finalize_jobs_kernel(DfFrame fr, Jobs jobs, const SeedRec* __restrict__ recs) {
  const int j = jobs.of_block(blockIdx.x);
  const DfJob& J = jobs.job(j);
  const Cam cam = jobs.cam(fr, j);
  const double px_error_angle = jobs.px_error_angle(fr, j);
  const int report_updated = jobs.report_updated(j);
  const int block = blockIdx.x - J.first_block;
  const int i = block * 256 + threadIdx.x;
  int st = SVO_HIP_SEED_ERASED;
  if (i < J.n) {
    const SeedRec rc = recs[(size_t)blockIdx.x * 256 + threadIdx.x];
    st = df_finalize_seed(cam, J.T.T_cur_ref, J.T.T_ref_cur, J.T.T_ref_inv, px_error_angle, fr.conv_thresh, i, rc, J.f, J.a, J.b, J.mu,
                          J.z_range, J.sigma2, J.status, nullptr, J.xyz, nullptr, nullptr, J.px_cur, nullptr);
  }
  df_finalize_events(st, i, J.n, block, J.alive, report_updated, J.block_count, J.hist);
}

// exclusive scan of a batch's per-block event counts (one workgroup of 1024 per batch) + the header of its page-locked event
// block (host memory); the total also to hist[8], where the scatter reads it
template <class Jobs>
__global__ __launch_bounds__(1024) void ev_scan_jobs_kernel(Jobs jobs) {
  const DfJob& J = jobs.job(blockIdx.x);
  int total;
  block_scan_counts(J.n_blocks, J.block_count, &total);
  if (threadIdx.x == 0) { J.header->n_events = total; J.hist[8] = total; }
  if (threadIdx.x < 7) J.header->counts[threadIdx.x] = J.hist[threadIdx.x];
}

// the events of one 256-seed block, ascending seed index, into the host block or the packed device array (EV_DIRECT_MAX)
template <class Jobs>
__global__ __launch_bounds__(256) void ev_scatter_jobs_kernel(Jobs jobs) {
  const int j = jobs.of_block(blockIdx.x);
  const DfJob& J = jobs.job(j);
  const int report_updated = jobs.report_updated(j);
  svo_hip_seed_event* events = J.hist[8] <= EV_DIRECT_MAX ? J.events_host : J.events_dev;
  const int block = blockIdx.x - J.first_block, i = block * 256 + threadIdx.x;
  const int st = i < J.n ? J.status[i] : SVO_HIP_SEED_ERASED;
  const bool ev = seed_event_wanted(st, report_updated);
  __shared__ int s_w[4];
  const int rank = ordered_rank_in_block(ev, s_w);
  if (ev) events[J.block_count[block] + rank] = make_seed_event(i, st, J.mu, J.sigma2, J.xyz, J.px_cur);
}

// ---- small passes: two launches ------------------------------------------------------------------------------------------
// Below a few thousand seeds every stage is a handful of workgroups whose time is its launch and a chain of dependent memory
// trips (4 keyframes x 500 seeds: geometry 11, search 10, align 18, finalize 12 us with events between them), six launches a
// frame.  Here ONE wave takes its four seeds through all four stages -- geometry on lanes 0-3, the search stage as it is (it
// never had a block-level barrier: a wave works on its own four seeds), alignment on lanes 0-15 (a quad per seed), the update
// on lanes 0-3 -- handing the records and warped patches from stage to stage through the same scratch as the large pass
// (same wave, same CU: a workgroup-scope fence orders them), and a second launch of one workgroup per batch does what the
// finalize stage's bookkeeping, ev_scan and ev_scatter do: outcome counts, `alive`, the scan and the ordered events.
// The lanes that idle through the f64 stages cost nothing here: the chip is empty.  Same device functions as the large pass,
// so every per-seed result is bit-identical (tests/test_gpu_seed_batch.py).
// 16 of these workgroups per 256-record block; a wave wholly behind its job's last seed has nothing to do: no later stage reads
// the records there.
template <class Jobs>
__global__ __launch_bounds__(256) void df_small_pass_kernel(DfFrame fr, Jobs jobs, const uint8_t* __restrict__ ref_base, size_t ref_pyr_bytes,
                                                            SeedRec* __restrict__ recs, uint32_t* __restrict__ pwb_t,
                                                            int32_t* __restrict__ level_cat, int n_pad) {
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int r0 = (blockIdx.x * 4 + wib) * SEEDS_PER_WAVE;   // the wave's first record
  const int j = jobs.of_block(blockIdx.x >> 4);
  const DfJob& J = jobs.job(j);
  const int n_end = J.first_block * 256 + J.n;             // the end of the job's records
  if (r0 >= n_end) return;                                 // wave-uniform; no block-level barrier below
  const Cam cam = jobs.cam(fr, j);
  const double px_error_angle = jobs.px_error_angle(fr, j);
  const uint8_t* cur_pyr = jobs.cur_image(j);
  const int i0 = r0 - J.first_block * 256;                 // the wave's first seed within its batch
  // ---- geometry
  if (lane < SEEDS_PER_WAVE) df_geometry_job_seed(fr, cam, J, i0 + lane, (size_t)r0 + lane, recs, level_cat);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
  // ---- warp + epipolar search
  df_search_block(fr, cam, ref_base, ref_pyr_bytes, cur_pyr, n_end, level_cat, recs, pwb_t, n_pad, blockIdx.x);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
  // ---- align2D
  {
    const int r = r0 + (lane >> 2);
    df_align_quad<false>(fr, cur_pyr, n_pad, pwb_t, recs, r, lane < 4 * SEEDS_PER_WAVE && r < n_end);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
  // ---- triangulation, computeTau, updateSeed
  if (lane < SEEDS_PER_WAVE && i0 + lane < J.n) {
    const SeedRec rc = recs[(size_t)r0 + lane];
    (void)df_finalize_seed(cam, J.T.T_cur_ref, J.T.T_ref_cur, J.T.T_ref_inv, px_error_angle, fr.conv_thresh, i0 + lane, rc, J.f, J.a, J.b,
                           J.mu, J.z_range, J.sigma2, J.status, nullptr, J.xyz, nullptr, nullptr, J.px_cur, nullptr);
  }
}

// one workgroup of 1024 per batch: what df_finalize_events, ev_scan_jobs_kernel and ev_scatter_jobs_kernel do, for a batch of at
// most DF_SMALL_MAX seeds
template <class Jobs>
__global__ __launch_bounds__(1024) void ev_small_kernel(Jobs jobs) {
  const DfJob& J = jobs.job(blockIdx.x);
  const int n = J.n, report_updated = jobs.report_updated(blockIdx.x);
  __shared__ int s_cnt[DF_SMALL_MAX / 256], s_off[DF_SMALL_MAX / 256], s_hist[8], s_w[16], s_total;
  if (threadIdx.x < DF_SMALL_MAX / 256) s_cnt[threadIdx.x] = 0;
  if (threadIdx.x < 8) s_hist[threadIdx.x] = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += 1024) {
    const int st = J.status[i];
    if (seed_gone(st)) J.alive[i] = 0;
    atomicAdd(&s_hist[st + 1], 1);
    if (seed_event_wanted(st, report_updated)) atomicAdd(&s_cnt[i >> 8], 1);
  }
  __syncthreads();
  if (threadIdx.x < 64) {                                  // exclusive scan of the (at most 64) block counts
    const int v = threadIdx.x < J.n_blocks ? s_cnt[threadIdx.x] : 0;
    const int incl = wave_scan_inclusive(v);
    s_off[threadIdx.x] = incl - v;
    if (threadIdx.x == 63) s_total = incl;
  }
  __syncthreads();
  const int total = s_total;
  if (threadIdx.x == 0) { J.header->n_events = total; J.hist[8] = total; }
  if (threadIdx.x < 7) J.header->counts[threadIdx.x] = s_hist[threadIdx.x];
  svo_hip_seed_event* events = total <= EV_DIRECT_MAX ? J.events_host : J.events_dev;
  for (int base = 0; base < n; base += 1024) {
    const int i = base + threadIdx.x;
    const int st = i < n ? J.status[i] : SVO_HIP_SEED_ERASED;
    const bool ev = seed_event_wanted(st, report_updated);
    const int rank = ordered_rank_in_block(ev, s_w, (threadIdx.x >> 6) & ~3);   // four waves per 256-seed block
    if (ev) events[s_off[i >> 8] + rank] = make_seed_event(i, st, J.mu, J.sigma2, J.xyz, J.px_cur);
    __syncthreads();
  }
}

// DepthFilter::updateSeeds on a keyframe (S/depth_filter.cpp:302-306): feature_detector_->setGridOccpuancy(matcher_.px_cur_)
// for every seed the pass updated -- status UPDATED, CONVERGED or NaN, the seeds a report_updated pass reports.  The status
// is the gate: px_cur of a seed without a match is not finite, that of an erased seed is stale.  Batch j owns the blocks
// [first_block, first_block + ceil(n / 256)) of the launch, as in the grouped pass.
__global__ __launch_bounds__(256) void seed_mark_updated_kernel(MarkGroup g, int cell_size, int grid_cols, int n_cells,
                                                                uint8_t* __restrict__ occupancy) {
  const MarkJob& J = g.job[job_of_block(g, (int)blockIdx.x)];
  const int i = ((int)blockIdx.x - J.first_block) * 256 + threadIdx.x;
  if (i >= J.n) return;
  if (J.status[i] < SVO_HIP_SEED_UPDATED) return;
  grid_mark_cell(J.px_cur[2 * (size_t)i], J.px_cur[2 * (size_t)i + 1], cell_size, grid_cols, n_cells, occupancy);
}
}  // namespace
