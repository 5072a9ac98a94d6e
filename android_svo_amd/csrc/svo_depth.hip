// svo_depth.hip -- align2D batch, DepthFilter::updateSeed / computeTau batches and the
// full per-seed DepthFilter::updateSeeds body (visibility, epipolar ZMSSD search, align2D,
// triangulation, tau, Bayes update, convergence test) on gfx950.
//
// Reference: S/depth_filter.cpp:237-416, S/matcher.cpp:36-147,207-355,
// I/patch_score.h:40-220, S/feature_alignment.cpp:154-282.
//
// Mapping: three stages (thread-per-seed geometry, wave-per-seed pixel work, thread-per-seed update);
// the fp64 geometry of a seed is evaluated once, 64 seeds per wave instruction;
// the 10x10 warped reference patch is built by lanes 0..99 (two passes) into LDS; the
// epipolar search assigns one candidate position per lane (64 candidates per pass), each
// lane computing a whole 8x8 ZMSSD with packed u8 dot products against the LDS patch;
// the best candidate is an order-preserving wave arg-min (first minimum wins, exactly the
// serial `zmssd < zmssd_best` scan); the sub-pixel refinement is the wave-per-patch
// align2D of svo_align_device.h.
//
// Exactness: all integer/index work (candidate pixel, search level, warped patch bytes,
// ZMSSD, arg-min) is bit-exact against the CPU path: the fp64 chains that feed integer
// conversions use the same operation order (built with -ffp-contract=off), and the
// epipolar abscissa uv_i is produced by the same repeated addition uv += step as
// S/matcher.cpp:299 (each lane replays its prefix).
//
// The device code is in the svo_depth_*.h headers of this translation unit (types, align, seed, search, events); this file is
// the host half: pose helpers, launchers, the device-resident seed batches and the C-ABI.
#include <vector>

#include "svo_depth_types.h"
#include "svo_depth_align.h"
#include "svo_depth_seed.h"
#include "svo_depth_search.h"
#include "svo_depth_events.h"

namespace {
int grid_for(int n, int block) {
  long long g = ((long long)n + block - 1) / block;
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
  return (int)g;
}

}  // namespace

extern "C" {

int svo_hip_align2d_batch_dev(svo_hip_ctx* ctx, const svo_hip_pyramid* cur, int slot, int level, int n,
                              const uint8_t* pwb_dev, const uint8_t* ref_patch_dev, int n_iter, double* px_dev,
                              uint8_t* converged_dev, int32_t* iters_dev) {
  if (!ctx || !cur) return SVO_HIP_ERR_INVALID;
  SVO_REQUIRE(ctx, slot >= 0 && slot < cur->batch && level >= 0 && level < cur->n_levels);
  SVO_REQUIRE(ctx, n >= 0 && n_iter >= 0);
  if (n == 0) return SVO_HIP_OK;
  SVO_REQUIRE(ctx, pwb_dev && px_dev && converged_dev);
  // ref_patch_dev == NULL: the 8x8 patch is the interior of the bordered one (createPatchFromPatchWithBorder,
  // matcher.cpp:138-147), which is how every caller of the reference fills it
  SVO_REQUIRE(ctx, ((uintptr_t)pwb_dev & 3) == 0 && ((uintptr_t)ref_patch_dev & 3) == 0);
  const uint8_t* img = cur->base + (size_t)slot * cur->pyr_bytes + cur->level_offset[level];
  hipLaunchKernelGGL(align2d_kernel, dim3((n + ALIGN_PATCHES - 1) / ALIGN_PATCHES), dim3(ALIGN_BLOCK), 0, ctx->stream, img,
                     cur->width >> level, cur->height >> level, n, pwb_dev, ref_patch_dev, n_iter, px_dev, converged_dev,
                     iters_dev);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  return SVO_HIP_OK;
}

int svo_hip_align1d_batch_dev(svo_hip_ctx* ctx, const svo_hip_pyramid* cur, int slot, int level, int n,
                              const uint8_t* pwb_dev, const float* dir_dev, int n_iter, double* px_dev,
                              uint8_t* converged_dev, double* h_inv_dev, int32_t* iters_dev) {
  if (!ctx || !cur) return SVO_HIP_ERR_INVALID;
  SVO_REQUIRE(ctx, slot >= 0 && slot < cur->batch && level >= 0 && level < cur->n_levels);
  SVO_REQUIRE(ctx, n >= 0 && n_iter >= 0);
  if (n == 0) return SVO_HIP_OK;
  SVO_REQUIRE(ctx, pwb_dev && dir_dev && px_dev && converged_dev);
  const uint8_t* img = cur->base + (size_t)slot * cur->pyr_bytes + cur->level_offset[level];
  SVO_REQUIRE(ctx, ((uintptr_t)pwb_dev & 3) == 0);
  hipLaunchKernelGGL(align1d_kernel, dim3((n + ALIGN_PATCHES - 1) / ALIGN_PATCHES), dim3(ALIGN_BLOCK), 0, ctx->stream, img,
                     cur->width >> level, cur->height >> level, n, pwb_dev, (const uint8_t*)nullptr, dir_dev, n_iter, px_dev,
                     converged_dev, h_inv_dev, iters_dev);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  return SVO_HIP_OK;
}

int svo_hip_align2d_batch(svo_hip_ctx* ctx, const svo_hip_pyramid* cur, int slot, int level, int n,
                          const uint8_t* pwb, const uint8_t* ref_patch, int n_iter, double* px, uint8_t* converged,
                          int32_t* iters) {
  if (!ctx || !cur) return SVO_HIP_ERR_INVALID;
  if (n == 0) return SVO_HIP_OK;
  SVO_REQUIRE(ctx, n > 0 && pwb && px && converged);
  // one device block from the context's staging area: px(16) pwb(100) patch(64) iters(4) converged(1) per patch
  const size_t N = (size_t)n;
  const size_t o_px = 0, o_pwb = o_px + 16 * N, o_rp = o_pwb + 100 * N, o_it = o_rp + 64 * N, o_cv = o_it + 4 * N,
               total = o_cv + N;
  char* d = nullptr;
  int rc = svo_ctx_staging(ctx, total, &d);
  if (rc == SVO_HIP_OK) rc = svo_hip_memcpy_h2d(ctx, d + o_pwb, pwb, 100 * N);
  if (rc == SVO_HIP_OK && ref_patch) rc = svo_hip_memcpy_h2d(ctx, d + o_rp, ref_patch, 64 * N);
  if (rc == SVO_HIP_OK) rc = svo_hip_memcpy_h2d(ctx, d + o_px, px, 16 * N);
  if (rc == SVO_HIP_OK)
    rc = svo_hip_align2d_batch_dev(ctx, cur, slot, level, n, (const uint8_t*)(d + o_pwb),
                                   ref_patch ? (const uint8_t*)(d + o_rp) : nullptr, n_iter, (double*)(d + o_px),
                                   (uint8_t*)(d + o_cv), (int32_t*)(d + o_it));
  if (rc == SVO_HIP_OK) rc = svo_hip_memcpy_d2h(ctx, px, d + o_px, 16 * N);
  if (rc == SVO_HIP_OK) rc = svo_hip_memcpy_d2h(ctx, converged, d + o_cv, N);
  if (rc == SVO_HIP_OK && iters) rc = svo_hip_memcpy_d2h(ctx, iters, d + o_it, 4 * N);
  return rc;
}

int svo_hip_camera_batch(svo_hip_ctx* ctx, const svo_hip_camera* cam, int n, const double* xyz, const double* uv,
                         const double* px, const int32_t* obs, int boundary, int level, double* px_of_xyz,
                         double* px_of_uv, double* f_of_px, uint8_t* in_frame) {
  if (!ctx || !cam) return SVO_HIP_ERR_INVALID;
  SVO_REQUIRE(ctx, n >= 0 && boundary >= 0 && level < SVO_HIP_MAX_LEVELS);
  if (n == 0) return SVO_HIP_OK;
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t N = (size_t)n;
  // one staging block: xyz(24) uv(16) px(16) px_of_xyz(16) px_of_uv(16) f_of_px(24) obs(8) in_frame(1)
  const size_t o_xyz = 0, o_uv = o_xyz + 24 * N, o_px = o_uv + 16 * N, o_a = o_px + 16 * N, o_b = o_a + 16 * N,
               o_f = o_b + 16 * N, o_obs = o_f + 24 * N, o_in = o_obs + 8 * N, total = o_in + N;
  char* d = nullptr;
  int rc = svo_ctx_staging(ctx, total, &d);
  if (rc != SVO_HIP_OK) return rc;
  if (xyz && rc == SVO_HIP_OK) rc = svo_hip_memcpy_h2d(ctx, d + o_xyz, xyz, 24 * N);
  if (uv && rc == SVO_HIP_OK) rc = svo_hip_memcpy_h2d(ctx, d + o_uv, uv, 16 * N);
  if (px && rc == SVO_HIP_OK) rc = svo_hip_memcpy_h2d(ctx, d + o_px, px, 16 * N);
  if (obs && rc == SVO_HIP_OK) rc = svo_hip_memcpy_h2d(ctx, d + o_obs, obs, 8 * N);
  if (rc != SVO_HIP_OK) return rc;
  hipLaunchKernelGGL(camera_batch_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, svo_make_cam(*cam), n,
                     xyz ? (const double*)(d + o_xyz) : nullptr, uv ? (const double*)(d + o_uv) : nullptr,
                     px ? (const double*)(d + o_px) : nullptr, obs ? (const int32_t*)(d + o_obs) : nullptr, boundary, level,
                     px_of_xyz ? (double*)(d + o_a) : nullptr, px_of_uv ? (double*)(d + o_b) : nullptr,
                     f_of_px ? (double*)(d + o_f) : nullptr, in_frame ? (uint8_t*)(d + o_in) : nullptr);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  if (xyz && px_of_xyz && rc == SVO_HIP_OK) rc = svo_hip_memcpy_d2h(ctx, px_of_xyz, d + o_a, 16 * N);
  if (uv && px_of_uv && rc == SVO_HIP_OK) rc = svo_hip_memcpy_d2h(ctx, px_of_uv, d + o_b, 16 * N);
  if (px && f_of_px && rc == SVO_HIP_OK) rc = svo_hip_memcpy_d2h(ctx, f_of_px, d + o_f, 24 * N);
  if (obs && in_frame && rc == SVO_HIP_OK) rc = svo_hip_memcpy_d2h(ctx, in_frame, d + o_in, N);
  return rc;
}

int svo_hip_update_seed_batch_dev(svo_hip_ctx* ctx, int n, const float* x, const float* tau2, float* a, float* b,
                                  float* mu, const float* z_range, float* sigma2) {
  if (!ctx) return SVO_HIP_ERR_INVALID;
  SVO_REQUIRE(ctx, n >= 0);
  if (n == 0) return SVO_HIP_OK;
  SVO_REQUIRE(ctx, x && tau2 && a && b && mu && z_range && sigma2);
  hipLaunchKernelGGL(update_seed_kernel, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, n, x, tau2, a, b, mu,
                     z_range, sigma2);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  return SVO_HIP_OK;
}

int svo_hip_compute_tau_batch_dev(svo_hip_ctx* ctx, int n, const double T_ref_cur[7], const double* f,
                                  const double* z, double px_error_angle, double* tau) {
  if (!ctx || !T_ref_cur) return SVO_HIP_ERR_INVALID;
  SVO_REQUIRE(ctx, n >= 0);
  if (n == 0) return SVO_HIP_OK;
  SVO_REQUIRE(ctx, f && z && tau);
  Vec3 t = {{T_ref_cur[0], T_ref_cur[1], T_ref_cur[2]}};
  hipLaunchKernelGGL(compute_tau_kernel, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, n, t, f, z,
                     px_error_angle, tau);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  return SVO_HIP_OK;
}

}  // extern "C"

// host-side SE3 helpers (same arithmetic as the device ones; this TU is built with -ffp-contract=off)
static void h_cross(const double* a, const double* b, double* o) {
  double x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
  o[0] = x; o[1] = y; o[2] = z;
}
static void h_rot(const double* q, const double* p, double* o) {
  double uv[3], quv[3];
  h_cross(q, p, uv);
  uv[0] = uv[0] + uv[0]; uv[1] = uv[1] + uv[1]; uv[2] = uv[2] + uv[2];
  h_cross(q, uv, quv);
  double x = (p[0] + q[3] * uv[0]) + quv[0], y = (p[1] + q[3] * uv[1]) + quv[1], z = (p[2] + q[3] * uv[2]) + quv[2];
  o[0] = x; o[1] = y; o[2] = z;
}
static void h_inv(const double* T, double* o) {
  double qi[4] = {-T[3], -T[4], -T[5], T[6]}, rt[3];
  h_rot(qi, T, rt);
  o[0] = -rt[0]; o[1] = -rt[1]; o[2] = -rt[2]; o[3] = qi[0]; o[4] = qi[1]; o[5] = qi[2]; o[6] = qi[3];
}
static void h_mul(const double* A, const double* B, double* o) {
  const double* a = A + 3; const double* b = B + 3;
  double q[4] = {a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                 a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]};
  double rt[3];
  h_rot(a, B, rt);
  double t0 = A[0] + rt[0], t1 = A[1] + rt[1], t2 = A[2] + rt[2];
  o[0] = t0; o[1] = t1; o[2] = t2; o[3] = q[0]; o[4] = q[1]; o[5] = q[2]; o[6] = q[3];
}

// the transforms between a reference keyframe and the current frame
static DfPoses df_make_poses(const double T_ref_w[7], const double T_cur_w[7]) {
  DfPoses P;
  double T_cur_inv[7];
  h_inv(T_cur_w, T_cur_inv);
  h_mul(T_ref_w, T_cur_inv, P.T_ref_cur);
  h_inv(P.T_ref_cur, P.T_cur_ref_vis);
  h_inv(T_ref_w, P.T_ref_inv);
  h_mul(T_cur_w, P.T_ref_inv, P.T_cur_ref);
  return P;
}

// the pose-free fields of a DfFrame: all the pixel stages (search, align) read
static void df_pixel_frame(const svo_hip_pyramid* ref, const svo_hip_pyramid* cur, const svo_hip_camera* cam, int n_pyr_levels,
                           int align_max_iter, int keep_px_on_failure, DfFrame& fr) {
  memset(&fr, 0, sizeof(fr));
  fr.cam = svo_make_cam(*cam);
  for (int l = 0; l < ref->n_levels; ++l) fr.ref_level_off[l] = ref->level_offset[l];
  for (int l = 0; l < cur->n_levels; ++l) fr.cur_level_off[l] = cur->level_offset[l];
  fr.n_pyr_levels = n_pyr_levels;
  fr.align_max_iter = align_max_iter;
  fr.keep_px_on_failure = keep_px_on_failure;
}

// frame-level constants of an updateSeeds pass without the transforms (fr.T stays zero): what the batches of several cameras
// share, whose jobs carry their own
static void df_make_pass_frame(const svo_hip_pyramid* ref, const svo_hip_pyramid* cur, const svo_hip_camera* cam, const svo_hip_df_params* prm,
                               DfFrame& fr) {
  df_pixel_frame(ref, cur, cam, prm->n_pyr_levels, prm->align_max_iter, 0, fr);
  const double focal_length = fabs(cam->fx);
  fr.px_error_angle = atan(1.0 / (2.0 * focal_length)) * 2.0;       // depth_filter.cpp:245-247
  fr.max_epi_search_steps = prm->max_epi_search_steps;
  fr.conv_thresh = prm->seed_convergence_sigma2_thresh;
}

// frame-level constants of one updateSeeds / findEpipolarMatchDirect batch
static void df_make_frame(const svo_hip_pyramid* ref, const svo_hip_pyramid* cur, const svo_hip_camera* cam,
                          const double T_ref_w[7], const double T_cur_w[7], const svo_hip_df_params* prm, DfFrame& fr) {
  df_make_pass_frame(ref, cur, cam, prm, fr);
  fr.T = df_make_poses(T_ref_w, T_cur_w);
}

// what every pass refuses before it enqueues anything: the slots, the image sizes, the parameters.  (The grouped entry point
// checks its reference slots batch by batch and passes none.)
static int df_check_pass_args(svo_hip_ctx* ctx, const svo_hip_pyramid* ref, int n_ref_slots, const int* ref_slots, const svo_hip_pyramid* cur,
                              int cur_slot, const svo_hip_camera* cam, const svo_hip_df_params* prm) {
  for (int k = 0; k < n_ref_slots; ++k) SVO_REQUIRE(ctx, ref_slots[k] >= 0 && ref_slots[k] < ref->batch);
  SVO_REQUIRE(ctx, cur_slot >= 0 && cur_slot < cur->batch);
  SVO_REQUIRE(ctx, ref->width == cam->width && ref->height == cam->height);
  SVO_REQUIRE(ctx, cur->width == cam->width && cur->height == cam->height);
  SVO_REQUIRE(ctx, prm->n_pyr_levels >= 1 && prm->n_pyr_levels <= ref->n_levels && prm->n_pyr_levels <= cur->n_levels);
  SVO_REQUIRE(ctx, prm->align_max_iter >= 0 && prm->max_epi_search_steps >= 0);
  return SVO_HIP_OK;
}

// per-seed records between the stages + the word-transposed warped patches: grow-only scratch owned by the context
struct DfScratch { SeedRec* recs; uint32_t* pwb_t; int n_pad; };
static int df_scratch(svo_hip_ctx* ctx, int n, DfScratch* s) {
  s->n_pad = (n + 63) / 64 * 64;
  const size_t rec_bytes = ((size_t)n * sizeof(SeedRec) + 255) & ~(size_t)255;
  void* ws = nullptr;
  const int rc = svo_ctx_scratch(ctx, rec_bytes + (size_t)25 * s->n_pad * sizeof(uint32_t), &ws);
  if (rc != SVO_HIP_OK) return rc;
  s->recs = (SeedRec*)ws;
  s->pwb_t = reinterpret_cast<uint32_t*>(static_cast<char*>(ws) + rec_bytes);
  return SVO_HIP_OK;
}

// diagnostic: an event at a stage boundary of a pass (svo_hip_df_set_profiling)
static void df_stamp(svo_hip_ctx* ctx, int k) { if (ctx->df_profile) (void)hipEventRecord(ctx->df_ev[k], ctx->stream); }

// The pixel stages over records [0, n): warp + epipolar search, align2D and, for edgelet reference features, align1D.
// The profiled paths (`stamps`) mark the end of the search stage and of the alignment.
static void df_launch_pixel_stages(svo_hip_ctx* ctx, const DfFrame& fr, const uint8_t* ref_base, size_t ref_pyr_bytes, const uint8_t* cur_img,
                                   int n, const int32_t* level, const DfScratch& s, bool align_1d, bool stamps) {
  const dim3 align_grid((n + ALIGN_PATCHES - 1) / ALIGN_PATCHES);
  hipLaunchKernelGGL(df_search_kernel, dim3((n + SEEDS_PER_BLOCK - 1) / SEEDS_PER_BLOCK), dim3(256), 0, ctx->stream, fr, ref_base, ref_pyr_bytes,
                     cur_img, n, level, s.recs, s.pwb_t, s.n_pad);
  if (stamps) df_stamp(ctx, 2);
  hipLaunchKernelGGL(df_align_kernel<false>, align_grid, dim3(ALIGN_BLOCK), 0, ctx->stream, fr, cur_img, n, s.n_pad, (const uint32_t*)s.pwb_t, s.recs);
  if (align_1d) hipLaunchKernelGGL(df_align_kernel<true>, align_grid, dim3(ALIGN_BLOCK), 0, ctx->stream, fr, cur_img, n, s.n_pad, (const uint32_t*)s.pwb_t, s.recs);
  if (stamps) df_stamp(ctx, 3);
}

// scratch of a resident-batch pass of n_blocks 256-record blocks: records (every block of the thread-per-seed stages whole), the
// transposed patches, the levels
struct DfPassScratch { DfScratch s; int32_t* level_cat; };
static int df_pass_scratch(svo_hip_ctx* ctx, int n_blocks, DfPassScratch* p) {
  const int n_rec = n_blocks * 256;
  const size_t rec_bytes = (size_t)n_rec * sizeof(SeedRec), pwb_bytes = (size_t)25 * n_rec * sizeof(uint32_t);
  void* ws = nullptr;
  if (const int rc = svo_ctx_scratch(ctx, rec_bytes + pwb_bytes + (size_t)n_rec * sizeof(int32_t), &ws); rc != SVO_HIP_OK) return rc;
  p->s = {(SeedRec*)ws, reinterpret_cast<uint32_t*>(static_cast<char*>(ws) + rec_bytes), n_rec};
  p->level_cat = reinterpret_cast<int32_t*>(static_cast<char*>(ws) + rec_bytes + pwb_bytes);
  return SVO_HIP_OK;
}

// the pixel stages of a large resident-batch pass, n_fine workgroups of 16 records (search) or 16 patches (align): over the
// concatenation up to the last job's last record where the jobs are a group's, job by job where they are a table's
static_assert(SEEDS_PER_BLOCK == ALIGN_PATCHES && 256 % SEEDS_PER_BLOCK == 0, "one fine grid for both pixel stages");
static void df_launch_jobs_pixel_stages(svo_hip_ctx* ctx, const DfFrame& fr, const DfGroupJobs& jobs, const svo_hip_pyramid* ref, int,
                                        const DfPassScratch& p) {
  const DfJob& last = jobs.g.job[jobs.g.n_jobs - 1];
  df_launch_pixel_stages(ctx, fr, ref->base, ref->pyr_bytes, jobs.cur_pyr, last.first_block * 256 + last.n, p.level_cat, p.s, false, true);
}
static void df_launch_jobs_pixel_stages(svo_hip_ctx* ctx, const DfFrame& fr, const DfTableJobs& jobs, const svo_hip_pyramid* ref, int n_fine,
                                        const DfPassScratch& p) {
  const DfCamJob* table = (const DfCamJob*)jobs.jobs;      // (these two kernels take the table's addresses one by one)
  const int* block_job = (const int*)jobs.block_job;
  hipLaunchKernelGGL(df_search_jobs_kernel, dim3(n_fine), dim3(256), 0, ctx->stream, fr, table, block_job, (const DfCamModel*)jobs.cams, ref->base,
                     ref->pyr_bytes, jobs.cur_base, jobs.cur_pyr_bytes, (const int32_t*)p.level_cat, p.s.recs, p.s.pwb_t, p.s.n_pad);
  df_stamp(ctx, 2);
  hipLaunchKernelGGL(df_align_jobs_kernel, dim3(n_fine), dim3(ALIGN_BLOCK), 0, ctx->stream, fr, table, block_job, jobs.cur_base, jobs.cur_pyr_bytes,
                     p.s.n_pad, (const uint32_t*)p.s.pwb_t, p.s.recs);
  df_stamp(ctx, 3);
}

// The launches of a resident-batch pass over n_jobs jobs of n_blocks 256-record blocks together, from either job source: two for a
// small pass (a wave takes its four seeds through every stage, then one workgroup per job does the events), six otherwise.
template <class Jobs>
static void df_launch_jobs_pass(svo_hip_ctx* ctx, const DfFrame& fr, const Jobs& jobs, int n_jobs, int n_blocks, int n_fine,
                                const svo_hip_pyramid* ref, const DfPassScratch& p) {
  const auto last = [ctx] { if (ctx->df_profile) { (void)hipEventRecord(ctx->df_ev[4], ctx->stream); ctx->df_ev_recorded = true; } };
  df_stamp(ctx, 0);
  if (n_blocks * 256 <= ctx->df_small_max) {
    hipLaunchKernelGGL(df_small_pass_kernel<Jobs>, dim3(n_fine), dim3(256), 0, ctx->stream, fr, jobs, ref->base, ref->pyr_bytes, p.s.recs,
                       p.s.pwb_t, p.level_cat, p.s.n_pad);
    df_stamp(ctx, 1); df_stamp(ctx, 2); df_stamp(ctx, 3);
    last();
    hipLaunchKernelGGL(ev_small_kernel<Jobs>, dim3(n_jobs), dim3(1024), 0, ctx->stream, jobs);
  } else {
    hipLaunchKernelGGL(df_geometry_jobs_kernel<Jobs>, dim3(n_blocks), dim3(256), 0, ctx->stream, fr, jobs, p.s.recs, p.level_cat);
    df_stamp(ctx, 1);
    df_launch_jobs_pixel_stages(ctx, fr, jobs, ref, n_fine, p);
    hipLaunchKernelGGL(df_finalize_jobs_kernel<Jobs>, dim3(n_blocks), dim3(256), 0, ctx->stream, fr, jobs, (const SeedRec*)p.s.recs);
    last();
    hipLaunchKernelGGL(ev_scan_jobs_kernel<Jobs>, dim3(n_jobs), dim3(1024), 0, ctx->stream, jobs);
    hipLaunchKernelGGL(ev_scatter_jobs_kernel<Jobs>, dim3(n_blocks), dim3(256), 0, ctx->stream, jobs);
  }
}

// One DepthFilter::updateSeeds pass over n seeds in device SoA arrays: geometry -> search -> align -> finalize on the
// context stream (the stateless entries svo_hip_depth_filter_update[_dev]; the seed batches have their own launches below).
static int df_run_pass(svo_hip_ctx* ctx, const svo_hip_pyramid* ref, int ref_slot, const svo_hip_pyramid* cur, int cur_slot,
                       const svo_hip_camera* cam, const double T_ref_w[7], const double T_cur_w[7], int n, const double* px,
                       const double* f, const int32_t* level, float* a, float* b, float* mu, const float* z_range, float* sigma2,
                       const svo_hip_df_params* prm, int32_t* status, double* z, double* xyz_world, int32_t* n_zmssd,
                       int32_t* n_align_iters, double* px_cur, int32_t* search_level) {
  if (!ctx || !ref || !cur || !cam || !T_ref_w || !T_cur_w || !prm) return SVO_HIP_ERR_INVALID;
  if (const int rc = df_check_pass_args(ctx, ref, 1, &ref_slot, cur, cur_slot, cam, prm); rc != SVO_HIP_OK) return rc;
  SVO_REQUIRE(ctx, n >= 0);
  if (n == 0) return SVO_HIP_OK;
  SVO_REQUIRE(ctx, px && f && level && a && b && mu && z_range && sigma2 && status);
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  DfFrame fr;
  df_make_frame(ref, cur, cam, T_ref_w, T_cur_w, prm, fr);
  DfScratch s;
  if (const int rc = df_scratch(ctx, n, &s); rc != SVO_HIP_OK) return rc;
  const uint8_t* ref_img = ref->base + (size_t)ref_slot * ref->pyr_bytes;
  const uint8_t* cur_img = cur->base + (size_t)cur_slot * cur->pyr_bytes;
  df_stamp(ctx, 0);
  hipLaunchKernelGGL(df_geometry_kernel<false>, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, fr, n, px, f, level, mu, sigma2,
                     (const double*)nullptr, (double*)nullptr, s.recs);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  df_stamp(ctx, 1);
  df_launch_pixel_stages(ctx, fr, ref_img, 0, cur_img, n, level, s, false, true);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  struct Last { const bool on; svo_hip_ctx* c; ~Last() { if (on) { (void)hipEventRecord(c->df_ev[4], c->stream); c->df_ev_recorded = true; } } } last{ctx->df_profile, ctx};
  hipLaunchKernelGGL(df_finalize_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, fr, n, f, s.recs, a, b, mu, z_range, sigma2,
                     status, z, xyz_world, n_zmssd, n_align_iters, px_cur, search_level);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  return SVO_HIP_OK;
}

extern "C" {

// Diagnostic: time the four stages of every following depth-filter pass of this context with HIP events on its stream
// (geometry, search, align, finalize); svo_hip_df_get_profile waits for the last pass and returns their durations.
int svo_hip_df_set_profiling(svo_hip_ctx* ctx, int enable) {
  if (!ctx) return SVO_HIP_ERR_INVALID;
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  if (enable) for (hipEvent_t& e : ctx->df_ev) if (!e) SVO_CHECK_HIP(ctx, hipEventCreate(&e));
  ctx->df_profile = enable != 0;
  ctx->df_ev_recorded = false;
  return SVO_HIP_OK;
}

int svo_hip_df_get_profile(svo_hip_ctx* ctx, double stage_us[4]) {
  if (!ctx || !stage_us) return SVO_HIP_ERR_INVALID;
  if (!ctx->df_ev_recorded) return svo_fail(ctx, SVO_HIP_ERR_STATE, "svo_hip_df_get_profile", "no profiled pass yet");
  SVO_CHECK_HIP(ctx, hipEventSynchronize(ctx->df_ev[4]));
  for (int k = 0; k < 4; ++k) {
    float ms = 0.0f;
    SVO_CHECK_HIP(ctx, hipEventElapsedTime(&ms, ctx->df_ev[k], ctx->df_ev[k + 1]));
    stage_us[k] = 1e3 * (double)ms;
  }
  return SVO_HIP_OK;
}

int svo_hip_depth_filter_update_dev(svo_hip_ctx* ctx, const svo_hip_pyramid* ref, int ref_slot,
                                    const svo_hip_pyramid* cur, int cur_slot, const svo_hip_camera* cam,
                                    const double T_ref_w[7], const double T_cur_w[7], int n, const double* px,
                                    const double* f, const int32_t* level, float* a, float* b, float* mu,
                                    const float* z_range, float* sigma2, const svo_hip_df_params* prm,
                                    int32_t* status, double* z, double* xyz_world, int32_t* n_zmssd,
                                    int32_t* n_align_iters, double* px_cur, int32_t* search_level) {
  return df_run_pass(ctx, ref, ref_slot, cur, cur_slot, cam, T_ref_w, T_cur_w, n, px, f, level, a, b, mu, z_range, sigma2, prm, status, z,
                     xyz_world, n_zmssd, n_align_iters, px_cur, search_level);
}

int svo_hip_epipolar_match_batch_dev(svo_hip_ctx* ctx, const svo_hip_pyramid* ref, int ref_slot,
                                     const svo_hip_pyramid* cur, int cur_slot, const svo_hip_camera* cam,
                                     const double T_ref_w[7], const double T_cur_w[7], int n, const double* px,
                                     const double* f, const int32_t* level, const double* depth_est_min_max,
                                     const svo_hip_df_params* prm, uint8_t* ok, double* depth, double* px_cur,
                                     int32_t* search_level, double* epi_length, int32_t* n_zmssd,
                                     int32_t* n_align_iters) {
  if (!ctx || !ref || !cur || !cam || !T_ref_w || !T_cur_w || !prm) return SVO_HIP_ERR_INVALID;
  if (const int rc = df_check_pass_args(ctx, ref, 1, &ref_slot, cur, cur_slot, cam, prm); rc != SVO_HIP_OK) return rc;
  SVO_REQUIRE(ctx, n >= 0);
  if (n == 0) return SVO_HIP_OK;
  SVO_REQUIRE(ctx, px && f && level && depth_est_min_max && ok);
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  DfFrame fr;
  df_make_frame(ref, cur, cam, T_ref_w, T_cur_w, prm, fr);
  DfScratch s;
  if (const int rc = df_scratch(ctx, n, &s); rc != SVO_HIP_OK) return rc;
  const uint8_t* ref_img = ref->base + (size_t)ref_slot * ref->pyr_bytes;
  const uint8_t* cur_img = cur->base + (size_t)cur_slot * cur->pyr_bytes;
  hipLaunchKernelGGL(df_geometry_kernel<true>, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, fr, n, px, f, level,
                     (const float*)nullptr, (const float*)nullptr, depth_est_min_max, epi_length, s.recs);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  df_launch_pixel_stages(ctx, fr, ref_img, 0, cur_img, n, level, s, false, false);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(epi_finalize_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, fr, n, f, s.recs, ok, depth, px_cur,
                     search_level, n_zmssd, n_align_iters);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  return SVO_HIP_OK;
}

}  // extern "C"

// The middle stages of the findMatchDirect pipeline for callers that form the records themselves (svo_track.hip): scratch
// for n_cap records + word-transposed patches, then warp / align2D (/ align1D) over the records of n_cams cameras in one set
// of launches (see df_search_cams_kernel)
int svo_match_scratch(svo_hip_ctx* ctx, int n_cap, svo_dev::SeedRec** recs, uint32_t** pwb_t, int* n_pad) {
  DfScratch s;
  const int rc = df_scratch(ctx, n_cap, &s);
  if (rc == SVO_HIP_OK) { *recs = s.recs; *pwb_t = s.pwb_t; *n_pad = s.n_pad; }
  return rc;
}

int svo_match_stages_cams(svo_hip_ctx* ctx, const svo_hip_pyramid* ref, const svo_hip_pyramid* cur, const svo_hip_camera* cam, int n_cams,
                          int cap, const int* counters_dev, int counter_stride, const int32_t* level_ref_dev, svo_dev::SeedRec* recs,
                          uint32_t* pwb_t, int n_pad, int n_pyr_levels, int align_max_iter, bool edgelets, const int* cam_list_dev, int n_listed) {
  if (!ctx || !ref || !cur || !cam || !recs || !pwb_t || !level_ref_dev || !counters_dev) return SVO_HIP_ERR_INVALID;
  SVO_REQUIRE(ctx, n_cams >= 1 && n_cams <= cur->batch && cap > 0 && cap % SEEDS_PER_BLOCK == 0 && cap % ALIGN_PATCHES == 0 && counter_stride >= 1);
  SVO_REQUIRE(ctx, n_pad >= n_cams * cap);
  SVO_REQUIRE(ctx, !cam_list_dev || (n_listed >= 1 && n_listed <= n_cams));
  DfFrame fr;
  df_pixel_frame(ref, cur, cam, n_pyr_levels, align_max_iter, 1, fr);
  if (cam_list_dev) {                // the listed cameras' slices only: the grid is n_listed cameras wide
    const int n_some = n_listed * cap;
    hipLaunchKernelGGL(df_search_listed_kernel, dim3(n_some / SEEDS_PER_BLOCK), dim3(256), 0, ctx->stream, fr, ref->base, ref->pyr_bytes, cur->base,
                       cur->pyr_bytes, cap, counters_dev, counter_stride, level_ref_dev, recs, pwb_t, n_pad, cam_list_dev);
    SVO_CHECK_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(df_align_listed_kernel<false>, dim3(n_some / ALIGN_PATCHES), dim3(ALIGN_BLOCK), 0, ctx->stream, fr, cur->base, cur->pyr_bytes, cap,
                       counters_dev, counter_stride, n_pad, pwb_t, recs, cam_list_dev);
    SVO_CHECK_HIP(ctx, hipGetLastError());
    if (edgelets) {
      hipLaunchKernelGGL(df_align_listed_kernel<true>, dim3(n_some / ALIGN_PATCHES), dim3(ALIGN_BLOCK), 0, ctx->stream, fr, cur->base, cur->pyr_bytes, cap,
                         counters_dev, counter_stride, n_pad, pwb_t, recs, cam_list_dev);
      SVO_CHECK_HIP(ctx, hipGetLastError());
    }
    return SVO_HIP_OK;
  }
  const int n_all = n_cams * cap;
  hipLaunchKernelGGL(df_search_cams_kernel, dim3(n_all / SEEDS_PER_BLOCK), dim3(256), 0, ctx->stream, fr, ref->base, ref->pyr_bytes, cur->base,
                     cur->pyr_bytes, cap, counters_dev, counter_stride, level_ref_dev, recs, pwb_t, n_pad);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(df_align_cams_kernel<false>, dim3(n_all / ALIGN_PATCHES), dim3(ALIGN_BLOCK), 0, ctx->stream, fr, cur->base, cur->pyr_bytes, cap,
                     counters_dev, counter_stride, n_pad, pwb_t, recs);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  if (edgelets) {
    hipLaunchKernelGGL(df_align_cams_kernel<true>, dim3(n_all / ALIGN_PATCHES), dim3(ALIGN_BLOCK), 0, ctx->stream, fr, cur->base, cur->pyr_bytes, cap,
                       counters_dev, counter_stride, n_pad, pwb_t, recs);
    SVO_CHECK_HIP(ctx, hipGetLastError());
  }
  return SVO_HIP_OK;
}

extern "C" {

int svo_hip_match_direct_batch_dev(svo_hip_ctx* ctx, const svo_hip_pyramid* ref, const svo_hip_pyramid* cur, int cur_slot,
                                   const svo_hip_camera* cam, int n_kf, const double* T_ref_w_dev,
                                   const double T_cur_w[7], int n, const int32_t* kf_slot_dev, const double* px_ref_dev,
                                   const double* f_ref_dev, const int32_t* level_ref_dev, const double* pt_pos_dev,
                                   const uint8_t* edgelet_dev, const double* grad_dev, int n_pyr_levels,
                                   int align_max_iter, double* px_cur_dev, uint8_t* success_dev,
                                   int32_t* search_level_dev) {
  if (!ctx || !ref || !cur || !cam || !T_cur_w) return SVO_HIP_ERR_INVALID;
  SVO_REQUIRE(ctx, cur_slot >= 0 && cur_slot < cur->batch && n_kf >= 1 && n_kf <= ref->batch);
  SVO_REQUIRE(ctx, ref->width == cam->width && ref->height == cam->height && cur->width == cam->width && cur->height == cam->height);
  SVO_REQUIRE(ctx, n_pyr_levels >= 1 && n_pyr_levels <= ref->n_levels && n_pyr_levels <= cur->n_levels && align_max_iter >= 0);
  SVO_REQUIRE(ctx, n >= 0);
  if (n == 0) return SVO_HIP_OK;
  SVO_REQUIRE(ctx, T_ref_w_dev && kf_slot_dev && px_ref_dev && f_ref_dev && level_ref_dev && pt_pos_dev && px_cur_dev && success_dev);
  SVO_REQUIRE(ctx, !edgelet_dev || grad_dev);
  DfScratch s;
  if (const int rc = df_scratch(ctx, n, &s); rc != SVO_HIP_OK) return rc;
  MdFrame mf;
  mf.cam = svo_make_cam(*cam);
  memcpy(mf.T_cur_w, T_cur_w, sizeof(double) * 7);
  mf.n_pyr_levels = n_pyr_levels;
  mf.n_kf = n_kf; mf.n_ref_levels = ref->n_levels; mf.slot_base = 0;
  DfFrame fr;
  df_pixel_frame(ref, cur, cam, n_pyr_levels, align_max_iter, 1, fr);
  hipLaunchKernelGGL(md_geometry_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, mf, n, T_ref_w_dev, kf_slot_dev,
                     px_ref_dev, f_ref_dev, level_ref_dev, pt_pos_dev, edgelet_dev, grad_dev, px_cur_dev, s.recs);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  df_launch_pixel_stages(ctx, fr, ref->base, ref->pyr_bytes, cur->base + (size_t)cur_slot * cur->pyr_bytes, n, level_ref_dev, s, edgelet_dev != nullptr, false);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(md_finalize_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, s.recs, px_cur_dev, success_dev,
                     search_level_dev);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  return SVO_HIP_OK;
}

// host-buffer convenience form: copies the SoA arrays in, runs, copies the results out, synchronises
int svo_hip_depth_filter_update(svo_hip_ctx* ctx, const svo_hip_pyramid* ref, int ref_slot, const svo_hip_pyramid* cur,
                                int cur_slot, const svo_hip_camera* cam, const double T_ref_w[7], const double T_cur_w[7],
                                int n, const double* px, const double* f, const int32_t* level, float* a, float* b,
                                float* mu, const float* z_range, float* sigma2, const svo_hip_df_params* prm,
                                int32_t* status, double* z, double* xyz_world, int32_t* n_zmssd, int32_t* n_align_iters,
                                double* px_cur, int32_t* search_level) {
  if (!ctx) return SVO_HIP_ERR_INVALID;
  SVO_REQUIRE(ctx, n >= 0);
  if (n == 0) return SVO_HIP_OK;
  SVO_REQUIRE(ctx, px && f && level && a && b && mu && z_range && sigma2 && status);
  const size_t N = (size_t)n;
  // One staging layout on both sides, the pageable arguments gathered in page-locked memory: one transfer each way.
  // inputs  : px(16) f(24) level(4) z_range(4) | in/out: a b mu sigma2 (4x4) | outputs: z(8) xyz(24) px_cur(16) status nz na sl (4x4)
  const size_t o_px = 0, o_f = o_px + 16 * N, o_z = o_f + 24 * N, o_xyz = o_z + 8 * N, o_pc = o_xyz + 24 * N,
               o_lvl = o_pc + 16 * N, o_zr = o_lvl + 4 * N, o_a = o_zr + 4 * N, o_b = o_a + 4 * N, o_mu = o_b + 4 * N,
               o_s2 = o_mu + 4 * N, o_st = o_s2 + 4 * N, o_nz = o_st + 4 * N, o_na = o_nz + 4 * N, o_sl = o_na + 4 * N,
               total = o_sl + 4 * N;
  char* blk = nullptr;
  char* hs = nullptr;
  int rc = svo_ctx_staging(ctx, total, &blk);
  if (rc != SVO_HIP_OK) return rc;
  rc = svo_ctx_host_staging(ctx, total, &hs);
  if (rc != SVO_HIP_OK) return rc;
  uint8_t* d = (uint8_t*)blk;
  memcpy(hs + o_px, px, 16 * N); memcpy(hs + o_f, f, 24 * N); memcpy(hs + o_lvl, level, 4 * N);
  memcpy(hs + o_zr, z_range, 4 * N); memcpy(hs + o_a, a, 4 * N); memcpy(hs + o_b, b, 4 * N);
  memcpy(hs + o_mu, mu, 4 * N); memcpy(hs + o_s2, sigma2, 4 * N);
  // two uploads (the output block in the middle does not cross the link): [px f] and [level .. sigma2]
  hipError_t e = hipMemcpyAsync(d + o_px, hs + o_px, 40 * N, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d + o_lvl, hs + o_lvl, o_st - o_lvl, hipMemcpyHostToDevice, ctx->stream);
  if (e != hipSuccess) return svo_fail(ctx, SVO_HIP_ERR_DEVICE, "svo_hip_depth_filter_update", hipGetErrorString(e));
  rc = svo_hip_depth_filter_update_dev(ctx, ref, ref_slot, cur, cur_slot, cam, T_ref_w, T_cur_w, n, (double*)(d + o_px),
                                       (double*)(d + o_f), (int32_t*)(d + o_lvl), (float*)(d + o_a), (float*)(d + o_b),
                                       (float*)(d + o_mu), (float*)(d + o_zr), (float*)(d + o_s2), prm,
                                       (int32_t*)(d + o_st), (double*)(d + o_z), (double*)(d + o_xyz),
                                       (int32_t*)(d + o_nz), (int32_t*)(d + o_na), (double*)(d + o_pc), (int32_t*)(d + o_sl));
  if (rc != SVO_HIP_OK) return rc;
  e = hipMemcpyAsync(hs + o_z, d + o_z, o_lvl - o_z, hipMemcpyDeviceToHost, ctx->stream);                 // z xyz px_cur
  if (e == hipSuccess) e = hipMemcpyAsync(hs + o_a, d + o_a, total - o_a, hipMemcpyDeviceToHost, ctx->stream);   // a .. search level
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return svo_fail(ctx, SVO_HIP_ERR_DEVICE, "svo_hip_depth_filter_update", hipGetErrorString(e));
  memcpy(a, hs + o_a, 4 * N); memcpy(b, hs + o_b, 4 * N); memcpy(mu, hs + o_mu, 4 * N); memcpy(sigma2, hs + o_s2, 4 * N);
  memcpy(status, hs + o_st, 4 * N);
  if (z) memcpy(z, hs + o_z, 8 * N);
  if (xyz_world) memcpy(xyz_world, hs + o_xyz, 24 * N);
  if (px_cur) memcpy(px_cur, hs + o_pc, 16 * N);
  if (n_zmssd) memcpy(n_zmssd, hs + o_nz, 4 * N);
  if (n_align_iters) memcpy(n_align_iters, hs + o_na, 4 * N);
  if (search_level) memcpy(search_level, hs + o_sl, 4 * N);
  return SVO_HIP_OK;
}

int svo_hip_seed_compact_converged_dev(svo_hip_ctx* ctx, int n, long long id_offset, const int32_t* status_dev,
                                       const float* mu_dev, const float* sigma2_dev, const double* xyz_world_dev,
                                       double* records_dev, int32_t* count_dev) {
  if (!ctx) return SVO_HIP_ERR_INVALID;
  SVO_REQUIRE(ctx, n >= 0 && count_dev);
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  if (n == 0) {
    SVO_CHECK_HIP(ctx, hipMemsetAsync(count_dev, 0, sizeof(int32_t), ctx->stream));
    return SVO_HIP_OK;
  }
  SVO_REQUIRE(ctx, status_dev && mu_dev && sigma2_dev && xyz_world_dev && records_dev);
  const int n_blocks = (n + 255) / 256;
  void* ws = nullptr;
  const int rc = svo_ctx_scratch(ctx, sizeof(int) * (size_t)n_blocks + 64, &ws);
  if (rc != SVO_HIP_OK) return rc;
  int* block_count = reinterpret_cast<int*>(ws);
  hipLaunchKernelGGL(conv_count_kernel, dim3(n_blocks), dim3(256), 0, ctx->stream, n, status_dev, block_count);
  hipLaunchKernelGGL(conv_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, n_blocks, block_count, reinterpret_cast<int*>(count_dev));
  hipLaunchKernelGGL(conv_scatter_kernel, dim3(n_blocks), dim3(256), 0, ctx->stream, n, id_offset, status_dev, mu_dev, sigma2_dev,
                     xyz_world_dev, block_count, records_dev);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  return SVO_HIP_OK;
}

// The exchange step of the seed-sharded depth filter (BASELINE config C4): this rank's converged seeds are
// packed on the device in seed order, clamped to `cap` records, and all-gathered together with the per-rank counts:
// records_all[world][cap][6] f64, counts_all[world] i32 (a count above cap = that rank had more: raise cap).
// Two collectives of fixed size, no host round trip in between.
int svo_hip_seed_gather_converged_dev(svo_hip_ctx* ctx, svo_hip_comm* comm, int n, long long id_offset, const int32_t* status_dev,
                                      const float* mu_dev, const float* sigma2_dev, const double* xyz_world_dev, int cap,
                                      double* records_all_dev, int32_t* counts_all_dev) {
  if (!ctx || !comm) return SVO_HIP_ERR_INVALID;
  SVO_REQUIRE(ctx, n >= 0 && cap >= 1 && records_all_dev && counts_all_dev);
  int rank = 0, world = 1;
  svo_hip_comm_info(comm, &rank, &world, nullptr);
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  // scratch: [block counts of the compaction][n records][count]
  const int n_blocks = (n + 255) / 256;
  const size_t o_rec = ((sizeof(int) * (size_t)n_blocks + 64) + 255) & ~(size_t)255;
  const size_t o_cnt = o_rec + (size_t)(n > 0 ? n : 1) * 6 * sizeof(double);
  void* ws = nullptr;
  int rc = svo_ctx_scratch(ctx, o_cnt + 64, &ws);
  if (rc != SVO_HIP_OK) return rc;
  // (svo_hip_seed_compact_converged_dev takes its block counts from the start of the same scratch area)
  double* rec = reinterpret_cast<double*>(static_cast<char*>(ws) + o_rec);
  int32_t* cnt = reinterpret_cast<int32_t*>(static_cast<char*>(ws) + o_cnt);
  rc = svo_hip_seed_compact_converged_dev(ctx, n, id_offset, status_dev, mu_dev, sigma2_dev, xyz_world_dev, rec, cnt);
  if (rc != SVO_HIP_OK) return rc;
  hipLaunchKernelGGL(records_clamp_copy_kernel, dim3(64), dim3(256), 0, ctx->stream, rec, reinterpret_cast<const int*>(cnt), cap,
                     records_all_dev + (size_t)rank * cap * 6, counts_all_dev + rank);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  rc = svo_comm_all_gather(comm, records_all_dev, (size_t)cap * 6 * sizeof(double));
  if (rc != SVO_HIP_OK) return rc;
  return svo_comm_all_gather(comm, counts_all_dev, sizeof(int32_t));
}

// The cell loop of Reprojector::reprojectMap (reprojector.cpp:149-166, 180-241) over candidates bucketed per cell in
// trial order: every live candidate is matched in ONE batch on the device, then the serial policy (first success per
// cell wins, later candidates untouched, stop once n_matches exceeds max_fts) is replayed on the host over the
// results.  findMatchDirect is a pure function of its candidate, so this equals the sequential evaluation.
int svo_hip_reproject_cells(svo_hip_ctx* ctx, const svo_hip_pyramid* ref, const svo_hip_pyramid* cur, int cur_slot,
                            const svo_hip_camera* cam, int n_kf, const double* T_kf_w, const double T_cur_w[7], int n_cells,
                            const int32_t* cell_offset, const int32_t* kf_slot, const double* px_ref, const double* f_ref,
                            const int32_t* level_ref, const double* pt_pos, const uint8_t* edgelet, const double* grad,
                            const uint8_t* deleted, double* px_cur, int max_fts, int n_pyr_levels, int align_max_iter,
                            uint8_t* tried, uint8_t* matched, int32_t* search_level, int32_t* cell_winner,
                            uint64_t* n_matches_out, uint64_t* n_trials_out) {
  if (!ctx) return SVO_HIP_ERR_INVALID;
  SVO_REQUIRE(ctx, n_cells >= 0 && cell_offset && tried && matched && cell_winner && n_matches_out && n_trials_out);
  const int n = cell_offset[n_cells];
  SVO_REQUIRE(ctx, n >= 0 && (n == 0 || (kf_slot && px_ref && f_ref && level_ref && pt_pos && deleted && px_cur && T_kf_w)));
  SVO_REQUIRE(ctx, !edgelet || grad);
  for (int c = 0; c < n_cells; ++c) cell_winner[c] = -1;
  *n_matches_out = 0; *n_trials_out = 0;
  if (n == 0) return SVO_HIP_OK;
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t N = (size_t)n;
  // one device block: px_ref(16) f(24) pos(24) px_cur(16) grad(16) T_kf(56*n_kf) kf_slot(4) level(4) sl(4) edgelet(1) ok(1)
  // one staging layout on both sides: [inputs ...][px_cur (in/out)][search level][matched]; the pageable arguments are
  // gathered in page-locked memory and cross the link in one transfer each way (nine + three transfers of ~10 us before)
  const size_t o_pr = 0, o_f = o_pr + 16 * N, o_pos = o_f + 24 * N, o_g = o_pos + 24 * N, o_T = o_g + 16 * N,
               o_k = o_T + 56 * (size_t)n_kf, o_l = o_k + 4 * N, o_e = o_l + 4 * N, o_pc = (o_e + N + 15) & ~(size_t)15,
               o_sl = o_pc + 16 * N, o_ok = o_sl + 4 * N, total = o_ok + N + 64;
  char* d = nullptr;
  char* hs = nullptr;
  {
    const int rc_st = svo_ctx_staging(ctx, total, &d);
    if (rc_st != SVO_HIP_OK) return rc_st;
    const int rc_hs = svo_ctx_host_staging(ctx, total, &hs);
    if (rc_hs != SVO_HIP_OK) return rc_hs;
  }
  auto put = [&](size_t off, const void* src, size_t bytes) { if (src) memcpy(hs + off, src, bytes); };
  put(o_pr, px_ref, 16 * N); put(o_f, f_ref, 24 * N); put(o_pos, pt_pos, 24 * N); put(o_g, grad, 16 * N);
  put(o_T, T_kf_w, 56 * (size_t)n_kf); put(o_k, kf_slot, 4 * N); put(o_l, level_ref, 4 * N); put(o_e, edgelet, N);
  put(o_pc, px_cur, 16 * N);
  hipError_t e = hipMemcpyAsync(d, hs, o_pc + 16 * N, hipMemcpyHostToDevice, ctx->stream);
  int rc = SVO_HIP_OK;
  const uint8_t* ok = reinterpret_cast<const uint8_t*>(hs + o_ok);
  const int32_t* sl = reinterpret_cast<const int32_t*>(hs + o_sl);
  if (e == hipSuccess) {
    rc = svo_hip_match_direct_batch_dev(ctx, ref, cur, cur_slot, cam, n_kf, reinterpret_cast<const double*>(d + o_T), T_cur_w, n,
                                        reinterpret_cast<const int32_t*>(d + o_k), reinterpret_cast<const double*>(d + o_pr),
                                        reinterpret_cast<const double*>(d + o_f), reinterpret_cast<const int32_t*>(d + o_l),
                                        reinterpret_cast<const double*>(d + o_pos),
                                        edgelet ? reinterpret_cast<const uint8_t*>(d + o_e) : nullptr,
                                        edgelet ? reinterpret_cast<const double*>(d + o_g) : nullptr, n_pyr_levels, align_max_iter,
                                        reinterpret_cast<double*>(d + o_pc), reinterpret_cast<uint8_t*>(d + o_ok),
                                        reinterpret_cast<int32_t*>(d + o_sl));
    if (rc == SVO_HIP_OK) {
      e = hipMemcpyAsync(hs + o_pc, d + o_pc, o_ok + N - o_pc, hipMemcpyDeviceToHost, ctx->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
  }
  if (e != hipSuccess) return svo_fail(ctx, SVO_HIP_ERR_DEVICE, "svo_hip_reproject_cells", hipGetErrorString(e));
  if (rc != SVO_HIP_OK) return rc;
  // ---- the serial policy (reprojector.cpp:149-166 with reprojectCell :180-241)
  memset(tried, 0, N);
  memset(matched, 0, N);
  uint64_t n_matches = 0, n_trials = 0;
  for (int c = 0; c < n_cells; ++c) {
    for (int i = cell_offset[c]; i < cell_offset[c + 1]; ++i) {
      ++n_trials;
      tried[i] = 1;
      if (deleted[i]) continue;                              // TYPE_DELETED: erased from the cell (:190-194)
      // findMatchDirect ran for this candidate: its px_cur is rewritten (matcher.cpp:200); candidates the serial
      // loop never reaches keep the caller's values
      memcpy(px_cur + 2 * (size_t)i, hs + o_pc + 16 * (size_t)i, 16);
      if (search_level) search_level[i] = sl[i];
      if (!ok[i]) continue;                                  // the caller counts the failure on the point (:202-209)
      matched[i] = 1;
      cell_winner[c] = i;
      ++n_matches;
      break;                                                 // maximum one point per cell (:238-239)
    }
    if (n_matches > (uint64_t)max_fts) break;                // :164-165
  }
  *n_matches_out = n_matches;
  *n_trials_out = n_trials;
  return SVO_HIP_OK;
}

}  // extern "C"

// ---- device-resident seed batches (include/svo_hip.h: svo_hip_seed_batch_*) -----------------------------------------
struct svo_hip_seed_batch {
  svo_hip_ctx* ctx = nullptr;
  int n = 0, n_alive = 0, n_blocks = 0;
  char* dev = nullptr;                  // one allocation: the arrays below
  double *px = nullptr, *f = nullptr, *xyz = nullptr, *px_cur = nullptr;
  int32_t *level = nullptr, *status = nullptr;
  float *a = nullptr, *b = nullptr, *mu = nullptr, *z_range = nullptr, *sigma2 = nullptr;
  uint8_t* alive = nullptr;
  int *block_count = nullptr, *hist = nullptr;
  svo_hip_seed_event* events_dev = nullptr;    // where the pass packs its events when there are many
  char* host = nullptr;                 // page-locked, mapped: EvHeader + n events, written by the kernels
  char* host_dev = nullptr;             // its device address
  bool pending = false;                 // a pass is enqueued and not collected yet
  int report_updated = 0;
  unsigned long long call_serial = 0;   // the last svo_hip_seed_batch_update_cameras_async call that named the batch (a batch named twice)
  svo_seed_block blk;                   // the pool block behind dev / host (returned to the context on destroy)
};

static size_t sb_align(size_t v) { return (v + 255) & ~(size_t)255; }
static constexpr size_t kEvHeaderBytes = 64;
static_assert(sizeof(svo_hip_seed_event) == 56, "event record layout (include/svo_hip.h)");

// The arrays of a block laid out for N seeds: the uploaded part first (px f level a b mu z_range sigma2), then outputs and
// bookkeeping
struct SbLayout { size_t o_px, o_f, o_lvl, o_a, o_b, o_mu, o_zr, o_s2, upload_bytes, o_xyz, o_pc, o_st, o_al, o_bc, o_h, o_ev, total; };
static SbLayout sb_layout(size_t N) {
  SbLayout L;
  size_t o = 0;
  L.o_px = o; o = sb_align(o + 16 * N);
  L.o_f = o; o = sb_align(o + 24 * N);
  L.o_lvl = o; o = sb_align(o + 4 * N);
  L.o_a = o; o = sb_align(o + 4 * N);
  L.o_b = o; o = sb_align(o + 4 * N);
  L.o_mu = o; o = sb_align(o + 4 * N);
  L.o_zr = o; o = sb_align(o + 4 * N);
  L.o_s2 = o; o = sb_align(o + 4 * N);
  L.upload_bytes = o;
  L.o_xyz = o; o = sb_align(o + 24 * N);
  L.o_pc = o; o = sb_align(o + 16 * N);
  L.o_st = o; o = sb_align(o + 4 * N);
  L.o_al = o; o = sb_align(o + N);
  L.o_bc = o; o = sb_align(o + 4 * ((N + 255) / 256));
  L.o_h = o; o = sb_align(o + 64);
  L.o_ev = o; o = sb_align(o + N * sizeof(svo_hip_seed_event));
  L.total = o;
  return L;
}
static void sb_point(svo_hip_seed_batch* sb, const SbLayout& L) {
  char* d = sb->dev;
  sb->px = (double*)(d + L.o_px); sb->f = (double*)(d + L.o_f); sb->level = (int32_t*)(d + L.o_lvl);
  sb->a = (float*)(d + L.o_a); sb->b = (float*)(d + L.o_b); sb->mu = (float*)(d + L.o_mu); sb->z_range = (float*)(d + L.o_zr);
  sb->sigma2 = (float*)(d + L.o_s2); sb->xyz = (double*)(d + L.o_xyz); sb->px_cur = (double*)(d + L.o_pc);
  sb->status = (int32_t*)(d + L.o_st); sb->alive = (uint8_t*)(d + L.o_al); sb->block_count = (int*)(d + L.o_bc); sb->hist = (int*)(d + L.o_h);
  sb->events_dev = (svo_hip_seed_event*)(d + L.o_ev);
}

// Capacity classes of the context's seed-batch pool: powers of two from 256 seeds (the drop-in's batches are <= 4096 seeds).
static int sb_capacity_class(int n) {
  int c = 256;
  while (c < n && c < (1 << 30)) c <<= 1;
  return c;
}

// A block for a batch of n seeds: a free block of n's capacity class, else a new one sized for the class (so that the next
// keyframe of about this size reuses it).  dev_need / host_need are the bytes a batch of n seeds lays out; both grow with n.
static int sb_take_block(svo_hip_ctx* ctx, int n, size_t dev_need, size_t host_need, svo_seed_block* out) {
  const int cap = sb_capacity_class(n);
  for (size_t i = 0; i < ctx->seed_pool.size(); ++i) {
    const svo_seed_block& b = ctx->seed_pool[i];
    if (b.cap == cap && b.dev_bytes >= dev_need && b.host_bytes >= host_need) {
      *out = b;
      ctx->seed_pool[i] = ctx->seed_pool.back();
      ctx->seed_pool.pop_back();
      ++ctx->seed_blocks_in_use;
      return SVO_HIP_OK;
    }
  }
  svo_seed_block b;
  b.cap = cap;
  // the layout of `cap` seeds bounds that of any n <= cap: per seed 16+24+4*6 uploaded, 24+16+4+1 outputs, one event record;
  // 15 sections rounded up to 256 bytes each, the block counts and the histogram
  const size_t C = (size_t)cap;
  b.dev_bytes = C * (16 + 24 + 4 * 6 + 24 + 16 + 4 + 1 + sizeof(svo_hip_seed_event)) + 4 * ((C + 255) / 256) + 64 + 16 * 256;
  if (b.dev_bytes < dev_need) b.dev_bytes = dev_need;
  b.host_bytes = kEvHeaderBytes + C * sizeof(svo_hip_seed_event);
  if (b.host_bytes < host_need) b.host_bytes = host_need;
  if (hipMalloc((void**)&b.dev, b.dev_bytes) != hipSuccess) return svo_fail(ctx, SVO_HIP_ERR_NOMEM, "svo_hip_seed_batch_create", "hipMalloc failed");
  ++ctx->n_allocs;
  if (hipHostMalloc((void**)&b.host, b.host_bytes, hipHostMallocMapped) != hipSuccess) {
    (void)hipFree(b.dev);
    return svo_fail(ctx, SVO_HIP_ERR_NOMEM, "svo_hip_seed_batch_create", "hipHostMalloc failed");
  }
  ++ctx->n_allocs;
  if (hipHostGetDevicePointer((void**)&b.host_dev, b.host, 0) != hipSuccess) {
    (void)hipFree(b.dev); (void)hipHostFree(b.host);
    return svo_fail(ctx, SVO_HIP_ERR_DEVICE, "svo_hip_seed_batch_create", "hipHostGetDevicePointer failed");
  }
  *out = b;
  ++ctx->seed_blocks_in_use;
  return SVO_HIP_OK;
}

// a block goes back to the pool (svo_hip_seed_batch_destroy; a detection that found nothing)
static void sb_return_block(svo_hip_ctx* ctx, const svo_seed_block& b) {
  ctx->seed_pool.push_back(b);
  --ctx->seed_blocks_in_use;
}

// a batch object over a pool block laid out for n_layout seeds, its event header cleared; no seeds yet (`who`: the entry point,
// for the error text)
static int sb_new(svo_hip_ctx* ctx, size_t n_layout, const char* who, svo_hip_seed_batch** out) {
  svo_hip_seed_batch* sb = new (std::nothrow) svo_hip_seed_batch;
  if (!sb) return svo_fail(ctx, SVO_HIP_ERR_NOMEM, who, "out of host memory");
  sb->ctx = ctx;
  const SbLayout L = sb_layout(n_layout);
  const int rc = sb_take_block(ctx, (int)n_layout, L.total, kEvHeaderBytes + n_layout * sizeof(svo_hip_seed_event), &sb->blk);
  if (rc != SVO_HIP_OK) { delete sb; return rc; }
  sb->dev = sb->blk.dev; sb->host = sb->blk.host; sb->host_dev = sb->blk.host_dev;
  sb_point(sb, L);
  memset(sb->host, 0, kEvHeaderBytes);
  *out = sb;
  return SVO_HIP_OK;
}


extern "C" {

int svo_hip_seed_batch_create(svo_hip_ctx* ctx, int n, const double* px, const double* f, const int32_t* level, const float* a,
                              const float* b, const float* mu, const float* z_range, const float* sigma2, svo_hip_seed_batch** out) {
  if (!ctx || !out) return SVO_HIP_ERR_INVALID;
  *out = nullptr;
  SVO_REQUIRE(ctx, n > 0 && px && f && level && a && b && mu && z_range && sigma2);
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t N = (size_t)n;
  svo_hip_seed_batch* sb = nullptr;
  int rc = sb_new(ctx, N, "svo_hip_seed_batch_create", &sb);
  if (rc != SVO_HIP_OK) return rc;
  sb->n = n; sb->n_alive = n; sb->n_blocks = (n + 255) / 256;
  const SbLayout L = sb_layout(N);
  // the uploaded arrays gathered in the context's page-locked staging area: one transfer
  char* hs = nullptr;
  rc = svo_ctx_host_staging(ctx, L.upload_bytes, &hs);
  if (rc == SVO_HIP_OK) {
    memcpy(hs + L.o_px, px, 16 * N); memcpy(hs + L.o_f, f, 24 * N); memcpy(hs + L.o_lvl, level, 4 * N); memcpy(hs + L.o_a, a, 4 * N);
    memcpy(hs + L.o_b, b, 4 * N); memcpy(hs + L.o_mu, mu, 4 * N); memcpy(hs + L.o_zr, z_range, 4 * N); memcpy(hs + L.o_s2, sigma2, 4 * N);
    hipError_t e = hipMemcpyAsync(sb->dev, hs, L.upload_bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(sb->alive, 1, N, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(sb->status, 0xff, 4 * N, ctx->stream);       // SVO_HIP_SEED_ERASED until the first pass
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);                          // the staging area is free again
    if (e != hipSuccess) rc = svo_fail(ctx, SVO_HIP_ERR_DEVICE, "svo_hip_seed_batch_create", hipGetErrorString(e));
  }
  if (rc != SVO_HIP_OK) { svo_hip_seed_batch_destroy(sb); return rc; }
  *out = sb;
  return SVO_HIP_OK;
}

int svo_hip_seed_batch_destroy(svo_hip_seed_batch* sb) {
  if (!sb) return SVO_HIP_OK;
  if (sb->ctx) { (void)hipSetDevice(sb->ctx->device); if (sb->pending) (void)hipStreamSynchronize(sb->ctx->stream); }
  // the block goes back to the context's pool: no hipFree (a device-wide synchronisation) at keyframe rate
#ifndef SVO_NO_SEED_POOL          // (the A/B build of tools/ab_churn.sh frees every block: what rounds 3-4 did)
  if (sb->ctx && sb->blk.dev && sb->blk.host) sb_return_block(sb->ctx, sb->blk);
  else
#else
  if (sb->ctx && sb->blk.dev) { --sb->ctx->seed_blocks_in_use; sb->ctx->n_frees += 2; }
#endif
  {
    if (sb->blk.dev) (void)hipFree(sb->blk.dev);
    if (sb->blk.host) (void)hipHostFree(sb->blk.host);
  }
  delete sb;
  return SVO_HIP_OK;
}

int svo_hip_seed_batch_size(const svo_hip_seed_batch* sb, int* n, int* n_alive) {
  if (!sb) return SVO_HIP_ERR_INVALID;
  if (n) *n = sb->n;
  if (n_alive) *n_alive = sb->n_alive;
  return SVO_HIP_OK;
}

// the job of a batch in a pass: its arrays, its keyframe's transforms against the current frame, the first of its 256-record blocks
static void sb_fill_job(DfJob& J, const svo_hip_seed_batch* sb, const double T_ref_w[7], const double T_cur_w[7], int first_block, int ref_slot) {
  J.T = df_make_poses(T_ref_w, T_cur_w);
  J.px = sb->px; J.f = sb->f; J.level = sb->level; J.a = sb->a; J.b = sb->b; J.mu = sb->mu; J.z_range = sb->z_range; J.sigma2 = sb->sigma2;
  J.status = sb->status; J.xyz = sb->xyz; J.px_cur = sb->px_cur; J.alive = sb->alive; J.block_count = sb->block_count; J.hist = sb->hist;
  J.header = reinterpret_cast<EvHeader*>(sb->host_dev);
  J.events_host = reinterpret_cast<svo_hip_seed_event*>(sb->host_dev + kEvHeaderBytes);
  J.events_dev = sb->events_dev;
  J.n = sb->n; J.n_blocks = sb->n_blocks; J.first_block = first_block; J.ref_slot = ref_slot;
}

// one launch set over at most DF_GROUP_MAX batches (arguments checked by the callers)
static int sb_enqueue_jobs(svo_hip_ctx* ctx, int n_jobs, svo_hip_seed_batch* const* batches, const svo_hip_pyramid* ref, const int* ref_slots,
                           const svo_hip_pyramid* cur, int cur_slot, const svo_hip_camera* cam, const double* T_ref_w,
                           const double T_cur_w[7], const svo_hip_df_params* prm, int report_updated) {
  DfFrame fr;
  df_make_frame(ref, cur, cam, T_ref_w, T_cur_w, prm, fr);
  DfGroupJobs jobs;
  memset(&jobs, 0, sizeof(jobs));
  jobs.cur_pyr = cur->base + (size_t)cur_slot * cur->pyr_bytes;
  DfGroup& g = jobs.g;
  g.n_jobs = n_jobs;
  g.report_updated = report_updated ? 1 : 0;
  int n_blocks = 0, n_cat = 0;
  for (int j = 0; j < n_jobs; ++j) {
    svo_hip_seed_batch* sb = batches[j];
    sb_fill_job(g.job[j], sb, T_ref_w + 7 * (size_t)j, T_cur_w, n_blocks, ref_slots[j]);
    n_cat = n_blocks * 256 + sb->n;
    n_blocks += sb->n_blocks;
  }
  DfPassScratch p;
  if (const int rc = df_pass_scratch(ctx, n_blocks, &p); rc != SVO_HIP_OK) return rc;
  df_launch_jobs_pass(ctx, fr, jobs, n_jobs, n_blocks, (n_cat + SEEDS_PER_BLOCK - 1) / SEEDS_PER_BLOCK, ref, p);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  for (int j = 0; j < n_jobs; ++j) { batches[j]->pending = true; batches[j]->report_updated = g.report_updated; }
  return SVO_HIP_OK;
}

int svo_hip_seed_batch_update_group_async(int n_batches, svo_hip_seed_batch* const* batches, const svo_hip_pyramid* ref,
                                          const int* ref_slots, const svo_hip_pyramid* cur, int cur_slot, const svo_hip_camera* cam,
                                          const double* T_ref_w, const double T_cur_w[7], const svo_hip_df_params* prm,
                                          int report_updated) {
  if (n_batches < 1 || !batches || !batches[0]) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = batches[0]->ctx;
  if (!ref || !ref_slots || !cur || !cam || !T_ref_w || !T_cur_w || !prm) return svo_fail(ctx, SVO_HIP_ERR_INVALID, "svo_hip_seed_batch_update_group_async", "null argument");
  // every batch's arguments are checked before anything is enqueued; up to DF_GROUP_MAX batches per set of launches
  for (int k = 0; k < n_batches; ++k) {
    svo_hip_seed_batch* sb = batches[k];
    SVO_REQUIRE(ctx, sb && sb->ctx == ctx);
    if (sb->pending) return svo_fail(ctx, SVO_HIP_ERR_STATE, "svo_hip_seed_batch_update_group_async", "the previous pass has not been collected");
    for (int m = 0; m < k; ++m) SVO_REQUIRE(ctx, batches[m] != sb);
    SVO_REQUIRE(ctx, ref_slots[k] >= 0 && ref_slots[k] < ref->batch);
  }
  if (const int rc = df_check_pass_args(ctx, ref, 0, nullptr, cur, cur_slot, cam, prm); rc != SVO_HIP_OK) return rc;
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  for (int first = 0; first < n_batches; first += DF_GROUP_MAX) {
    const int n_jobs = n_batches - first < DF_GROUP_MAX ? n_batches - first : DF_GROUP_MAX;
    const int rc = sb_enqueue_jobs(ctx, n_jobs, batches + first, ref, ref_slots + first, cur, cur_slot, cam, T_ref_w + 7 * (size_t)first, T_cur_w,
                                   prm, report_updated);
    if (rc != SVO_HIP_OK) return rc;
  }
  return SVO_HIP_OK;
}

// a single batch is a group of one
int svo_hip_seed_batch_update_async(svo_hip_seed_batch* sb, const svo_hip_pyramid* ref, int ref_slot, const svo_hip_pyramid* cur,
                                    int cur_slot, const svo_hip_camera* cam, const double T_ref_w[7], const double T_cur_w[7],
                                    const svo_hip_df_params* prm, int report_updated) {
  return svo_hip_seed_batch_update_group_async(1, &sb, ref, &ref_slot, cur, cur_slot, cam, T_ref_w, T_cur_w, prm, report_updated);
}

// The context's job table of a pass over several cameras: `need` bytes of device memory and of page-locked memory beside it,
// grown together; the page-locked area is free to be rewritten when this returns.
static int df_jobs_area(svo_hip_ctx* ctx, size_t need) {
  if (ctx->df_jobs_in_flight) {                            // the previous call's transfer may still read the area
    SVO_CHECK_HIP(ctx, hipEventSynchronize(ctx->df_jobs_ev));
    ctx->df_jobs_in_flight = false;
  }
  if (!ctx->df_jobs_ev) SVO_CHECK_HIP(ctx, hipEventCreateWithFlags(&ctx->df_jobs_ev, hipEventDisableTiming));
  if (ctx->df_jobs_bytes >= need) return SVO_HIP_OK;
  if (ctx->df_jobs_dev || ctx->df_jobs_host) {
    SVO_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // kernels of an earlier pass read the table
    if (ctx->df_jobs_dev) { (void)hipFree(ctx->df_jobs_dev); ++ctx->n_frees; }
    if (ctx->df_jobs_host) { (void)hipHostFree(ctx->df_jobs_host); ++ctx->n_frees; }
    ctx->df_jobs_dev = ctx->df_jobs_host = nullptr;
    ctx->df_jobs_bytes = 0;
  }
  const size_t bytes = need + need / 4;
  SVO_CHECK_HIP(ctx, hipMalloc(&ctx->df_jobs_dev, bytes));
  ++ctx->n_allocs;
  SVO_CHECK_HIP(ctx, hipHostMalloc(&ctx->df_jobs_host, bytes, hipHostMallocDefault));
  ++ctx->n_allocs;
  ctx->df_jobs_bytes = bytes;
  return SVO_HIP_OK;
}

// what a pass takes from a camera's model, for the pass's camera table
static DfCamModel df_cam_model(const svo_hip_camera* cam) {
  DfCamModel m;
  memset(&m, 0, sizeof(m));
  m.cam = svo_make_cam(*cam);
  m.px_error_angle = atan(1.0 / (2.0 * fabs(cam->fx))) * 2.0;        // depth_filter.cpp:245-247
  return m;
}

// The pass over the batches of several cameras: camera c's model is cams[c * cam_stride] -- stride 1 for a rig, 0 for the one
// model all cameras of svo_hip_seed_batch_update_cameras_async share (its camera table then has one entry).
static int df_cameras_pass(svo_hip_ctx* ctx, const char* who, int n_cameras, const svo_hip_seed_camera_pass* passes, const svo_hip_pyramid* ref,
                           const svo_hip_pyramid* cur, const svo_hip_camera* cams, int cam_stride, const svo_hip_df_params* prm) {
  if (!ctx) return SVO_HIP_ERR_INVALID;
  if (!passes || !ref || !cur || !cams || !prm) return svo_fail(ctx, SVO_HIP_ERR_INVALID, who, "null argument");
  SVO_REQUIRE(ctx, n_cameras >= 0);
  // ---- every camera's and every batch's arguments are checked before anything is enqueued
  const int n_models = cam_stride ? n_cameras : 1;
  for (int m = 1; m < n_models; ++m) SVO_REQUIRE(ctx, cams[m].width == cams[0].width && cams[m].height == cams[0].height);
  // (the call's serial, stamped on the batches the walk has passed, is how a batch named twice is found; it is the one thing a
  // refused call leaves behind, and it means nothing to the next call, which has a serial of its own)
  const unsigned long long serial = ++ctx->df_jobs_serial;
  long long n_jobs_ll = 0, n_blocks_ll = 0;
  for (int c = 0; c < n_cameras; ++c) {
    const svo_hip_seed_camera_pass& P = passes[c];
    SVO_REQUIRE(ctx, P.n_batches >= 0);
    if (P.n_batches == 0) continue;                        // the camera sits this pass out
    SVO_REQUIRE(ctx, P.batches && P.ref_slots && P.T_ref_w);
    SVO_REQUIRE(ctx, P.cur_slot >= 0 && P.cur_slot < cur->batch);
    for (int k = 0; k < P.n_batches; ++k) {
      svo_hip_seed_batch* sb = P.batches[k];
      SVO_REQUIRE(ctx, sb && sb->ctx == ctx);
      if (sb->pending) return svo_fail(ctx, SVO_HIP_ERR_STATE, who, "the previous pass has not been collected");
      if (sb->call_serial == serial) return svo_fail(ctx, SVO_HIP_ERR_INVALID, who, "a batch is named twice");
      sb->call_serial = serial;
      SVO_REQUIRE(ctx, P.ref_slots[k] >= 0 && P.ref_slots[k] < ref->batch);
      n_blocks_ll += sb->n_blocks;
    }
    n_jobs_ll += P.n_batches;
  }
  if (n_models > 0)                                        // (all models have the size of the first)
    if (const int rc = df_check_pass_args(ctx, ref, 0, nullptr, cur, 0, &cams[0], prm); rc != SVO_HIP_OK) return rc;
  SVO_REQUIRE(ctx, n_jobs_ll <= SVO_HIP_DF_CAMERAS_MAX_JOBS && n_blocks_ll * 256 <= SVO_HIP_DF_CAMERAS_MAX_RECORDS);
  if (n_jobs_ll == 0) return SVO_HIP_OK;
  const int n_jobs = (int)n_jobs_ll, n_blocks = (int)n_blocks_ll;
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  // ---- memory: the pass's scratch and the job table; nothing is enqueued yet
  DfPassScratch p;
  if (const int rc = df_pass_scratch(ctx, n_blocks, &p); rc != SVO_HIP_OK) return rc;
  const size_t jobs_bytes = (size_t)n_jobs * sizeof(DfCamJob), cams_off = (jobs_bytes + (size_t)n_blocks * sizeof(int) + 7) & ~(size_t)7,
               table_bytes = cams_off + (size_t)n_models * sizeof(DfCamModel);
  if (const int rc = df_jobs_area(ctx, table_bytes); rc != SVO_HIP_OK) return rc;
  // ---- the table, packed: [jobs][block -> job][camera models]
  DfCamJob* jobs_host = static_cast<DfCamJob*>(ctx->df_jobs_host);
  int* block_job_host = reinterpret_cast<int*>(static_cast<char*>(ctx->df_jobs_host) + jobs_bytes);
  DfCamModel* cams_host = reinterpret_cast<DfCamModel*>(static_cast<char*>(ctx->df_jobs_host) + cams_off);
  memset(jobs_host, 0, cams_off);
  for (int m = 0; m < n_models; ++m) cams_host[m] = df_cam_model(&cams[m]);
  int j = 0, first_block = 0;
  for (int c = 0; c < n_cameras; ++c) {
    const svo_hip_seed_camera_pass& P = passes[c];
    for (int k = 0; k < P.n_batches; ++k, ++j) {
      const svo_hip_seed_batch* sb = P.batches[k];
      sb_fill_job(jobs_host[j].job, sb, P.T_ref_w + 7 * (size_t)k, P.T_cur_w, first_block, P.ref_slots[k]);
      jobs_host[j].cur_slot = P.cur_slot;
      jobs_host[j].report_updated = P.report_updated ? 1 : 0;
      jobs_host[j].cam = c * cam_stride;
      for (int b = 0; b < sb->n_blocks; ++b) block_job_host[first_block + b] = j;
      first_block += sb->n_blocks;
    }
  }
  const char* table = static_cast<const char*>(ctx->df_jobs_dev);
  const DfTableJobs jobs = {(DfFixed<DfCamJob>)table, (DfFixed<int>)(table + jobs_bytes), (DfFixed<DfCamModel>)(table + cams_off), cur->base,
                            cur->pyr_bytes};
  DfFrame fr;                                              // (its cam gives the kernels the common image size and nothing else)
  df_make_pass_frame(ref, cur, &cams[0], prm, fr);
  // ---- the transfer and the launches; from here on an error path waits for the stream before it returns
  hipError_t e = hipMemcpyAsync(ctx->df_jobs_dev, ctx->df_jobs_host, table_bytes, hipMemcpyHostToDevice, ctx->stream);
  if (e != hipSuccess) return svo_fail(ctx, SVO_HIP_ERR_DEVICE, who, hipGetErrorString(e));
  e = hipEventRecord(ctx->df_jobs_ev, ctx->stream);
  if (e == hipSuccess) {
    ctx->df_jobs_in_flight = true;
    df_launch_jobs_pass(ctx, fr, jobs, n_jobs, n_blocks, n_blocks * (256 / SEEDS_PER_BLOCK), ref, p);
    e = hipGetLastError();
  }
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(ctx->stream);               // nothing of the call is in flight when the caller unwinds
    ctx->df_jobs_in_flight = false;
    return svo_fail(ctx, SVO_HIP_ERR_DEVICE, who, hipGetErrorString(e));
  }
  for (int c = 0; c < n_cameras; ++c)
    for (int k = 0; k < passes[c].n_batches; ++k) { passes[c].batches[k]->pending = true; passes[c].batches[k]->report_updated = passes[c].report_updated ? 1 : 0; }
  return SVO_HIP_OK;
}

int svo_hip_seed_batch_update_rig_async(svo_hip_ctx* ctx, int n_cameras, const svo_hip_seed_camera_pass* passes, const svo_hip_pyramid* ref,
                                        const svo_hip_pyramid* cur, const svo_hip_camera* cams, const svo_hip_df_params* prm) {
  return df_cameras_pass(ctx, "svo_hip_seed_batch_update_rig_async", n_cameras, passes, ref, cur, cams, 1, prm);
}

// one camera model for all cameras: the rig pass with that model repeated
int svo_hip_seed_batch_update_cameras_async(svo_hip_ctx* ctx, int n_cameras, const svo_hip_seed_camera_pass* passes, const svo_hip_pyramid* ref,
                                            const svo_hip_pyramid* cur, const svo_hip_camera* cam, const svo_hip_df_params* prm) {
  return df_cameras_pass(ctx, "svo_hip_seed_batch_update_cameras_async", n_cameras, passes, ref, cur, cam, 0, prm);
}

int svo_hip_df_set_small_pass_limit(svo_hip_ctx* ctx, int max_seeds) {
  if (!ctx) return SVO_HIP_ERR_INVALID;
  SVO_REQUIRE(ctx, max_seeds >= 0 && max_seeds <= DF_SMALL_MAX);
  ctx->df_small_max = max_seeds;
  return SVO_HIP_OK;
}

int svo_hip_seed_batch_pending(const svo_hip_seed_batch* sb) { return sb && sb->pending ? 1 : 0; }

int svo_hip_seed_batch_collect(svo_hip_seed_batch* sb, const svo_hip_seed_event** events, int* n_events, int32_t status_counts[7]) {
  if (!sb) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = sb->ctx;
  if (!sb->pending) return svo_fail(ctx, SVO_HIP_ERR_STATE, "svo_hip_seed_batch_collect", "no pass has been enqueued");
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  SVO_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  sb->pending = false;
  const EvHeader* h = reinterpret_cast<const EvHeader*>(sb->host);
  if (h->n_events > EV_DIRECT_MAX) {                      // many events (a keyframe): packed on the device, one transfer
    SVO_CHECK_HIP(ctx, hipMemcpyAsync(sb->host + kEvHeaderBytes, sb->events_dev, (size_t)h->n_events * sizeof(svo_hip_seed_event),
                                      hipMemcpyDeviceToHost, ctx->stream));
    SVO_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (events) *events = reinterpret_cast<const svo_hip_seed_event*>(sb->host + kEvHeaderBytes);
  if (n_events) *n_events = h->n_events;
  if (status_counts) for (int k = 0; k < 7; ++k) status_counts[k] = h->counts[k];
  sb->n_alive -= h->counts[SVO_HIP_SEED_CONVERGED + 1] + h->counts[SVO_HIP_SEED_NAN + 1];
  return SVO_HIP_OK;
}

int svo_hip_seed_batch_erase(svo_hip_seed_batch* sb, int n, const int32_t* indices) {
  if (!sb) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = sb->ctx;
  SVO_REQUIRE(ctx, n >= 0 && (n == 0 || indices));
  if (sb->pending) return svo_fail(ctx, SVO_HIP_ERR_STATE, "svo_hip_seed_batch_erase", "collect the enqueued pass first");
  if (n == 0) return SVO_HIP_OK;
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  // the alive flags come down, are edited and go back: erasures are rare (removeKeyframe) and this keeps n_alive exact
  std::vector<uint8_t> al((size_t)sb->n);
  SVO_CHECK_HIP(ctx, hipMemcpyAsync(al.data(), sb->alive, (size_t)sb->n, hipMemcpyDeviceToHost, ctx->stream));
  SVO_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < n; ++k) {
    SVO_REQUIRE(ctx, indices[k] >= 0 && indices[k] < sb->n);
    if (al[(size_t)indices[k]]) { al[(size_t)indices[k]] = 0; --sb->n_alive; }
  }
  SVO_CHECK_HIP(ctx, hipMemcpyAsync(sb->alive, al.data(), (size_t)sb->n, hipMemcpyHostToDevice, ctx->stream));
  SVO_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SVO_HIP_OK;
}

int svo_hip_seed_batch_download(svo_hip_seed_batch* sb, float* a, float* b, float* mu, float* sigma2, uint8_t* alive) {
  if (!sb) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = sb->ctx;
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t N = (size_t)sb->n;
  if (a) SVO_CHECK_HIP(ctx, hipMemcpyAsync(a, sb->a, 4 * N, hipMemcpyDeviceToHost, ctx->stream));
  if (b) SVO_CHECK_HIP(ctx, hipMemcpyAsync(b, sb->b, 4 * N, hipMemcpyDeviceToHost, ctx->stream));
  if (mu) SVO_CHECK_HIP(ctx, hipMemcpyAsync(mu, sb->mu, 4 * N, hipMemcpyDeviceToHost, ctx->stream));
  if (sigma2) SVO_CHECK_HIP(ctx, hipMemcpyAsync(sigma2, sb->sigma2, 4 * N, hipMemcpyDeviceToHost, ctx->stream));
  if (alive) SVO_CHECK_HIP(ctx, hipMemcpyAsync(alive, sb->alive, N, hipMemcpyDeviceToHost, ctx->stream));
  SVO_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SVO_HIP_OK;
}

int svo_hip_seed_batch_arrays(svo_hip_seed_batch* sb, float** a_dev, float** b_dev, float** mu_dev, float** sigma2_dev, int32_t** status_dev) {
  if (!sb) return SVO_HIP_ERR_INVALID;
  if (a_dev) *a_dev = sb->a;
  if (b_dev) *b_dev = sb->b;
  if (mu_dev) *mu_dev = sb->mu;
  if (sigma2_dev) *sigma2_dev = sb->sigma2;
  if (status_dev) *status_dev = sb->status;
  return SVO_HIP_OK;
}

int svo_hip_seed_batch_mark_updated(int n_batches, svo_hip_seed_batch* const* batches, int cell_size, int grid_cols, int grid_rows,
                                    uint8_t* occupancy_dev) {
  if (n_batches < 1 || !batches || !batches[0]) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = batches[0]->ctx;
  // everything is checked before anything is enqueued
  for (int k = 0; k < n_batches; ++k) SVO_REQUIRE(ctx, batches[k] && batches[k]->ctx == ctx);
  SVO_REQUIRE(ctx, occupancy_dev && cell_size > 0 && grid_cols > 0 && grid_rows > 0);
  SVO_REQUIRE(ctx, (long long)grid_cols * grid_rows < (1ll << 31));
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  for (int first = 0; first < n_batches; first += DF_GROUP_MAX) {
    MarkGroup g;
    memset(&g, 0, sizeof(g));
    g.n_jobs = n_batches - first < DF_GROUP_MAX ? n_batches - first : DF_GROUP_MAX;
    int n_blocks = 0;
    for (int j = 0; j < g.n_jobs; ++j) {
      const svo_hip_seed_batch* sb = batches[first + j];
      g.job[j].status = sb->status; g.job[j].px_cur = sb->px_cur; g.job[j].n = sb->n; g.job[j].first_block = n_blocks;
      n_blocks += sb->n_blocks;
    }
    hipLaunchKernelGGL(seed_mark_updated_kernel, dim3(n_blocks), dim3(256), 0, ctx->stream, g, cell_size, grid_cols, grid_cols * grid_rows,
                       occupancy_dev);
  }
  SVO_CHECK_HIP(ctx, hipGetLastError());
  return SVO_HIP_OK;
}

int svo_hip_seed_batch_create_detected(svo_hip_ctx* ctx, const svo_hip_pyramid* pyr, int slot, const svo_hip_camera* cam, int n_pyr_levels,
                                       int cell_size, uint8_t* occupancy_dev, int clear_occupancy, double detection_threshold,
                                       double depth_mean, double depth_min, svo_hip_seed_batch** out, int32_t* n_out, double* px,
                                       double* f, int32_t* level, float* score) {
  if (!ctx || !out) return SVO_HIP_ERR_INVALID;
  *out = nullptr;
  SVO_REQUIRE(ctx, n_out != nullptr);
  *n_out = 0;
  {
    // the detection's refusals come first: a refused call takes no block
    const int rc = svo_detect_check_args(ctx, pyr, slot, cam, n_pyr_levels, cell_size, detection_threshold);
    if (rc != SVO_HIP_OK) return rc;
  }
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  int gc = 0, gr = 0;
  svo_hip_detect_grid(pyr->width, pyr->height, cell_size, &gc, &gr);
  const size_t NC = (size_t)gc * gr;                       // one feature per cell at most: the block is laid out for NC seeds
  svo_hip_seed_batch* sb = nullptr;
  int rc = sb_new(ctx, NC, "svo_hip_seed_batch_create_detected", &sb);
  if (rc != SVO_HIP_OK) return rc;
  // The features for the host go into the batch's page-locked event area, which nothing uses before the first pass:
  // [px NC x 2 f64][f NC x 3 f64][level NC i32][score NC f32] = 48 bytes a cell of the 56 an event takes; the count into the header
  const size_t o_hpx = kEvHeaderBytes, o_hf = o_hpx + 16 * NC, o_hl = o_hf + 24 * NC, o_hs = o_hl + 4 * NC;
  svo_detect_seed_out o;
  o.px = sb->px; o.f = sb->f; o.level = sb->level; o.a = sb->a; o.b = sb->b; o.mu = sb->mu; o.z_range = sb->z_range; o.sigma2 = sb->sigma2;
  o.alive = sb->alive; o.status = sb->status;
  o.n_host = reinterpret_cast<int32_t*>(sb->host_dev);
  o.px_host = reinterpret_cast<double*>(sb->host_dev + o_hpx); o.f_host = reinterpret_cast<double*>(sb->host_dev + o_hf);
  o.level_host = reinterpret_cast<int32_t*>(sb->host_dev + o_hl); o.score_host = reinterpret_cast<float*>(sb->host_dev + o_hs);
  rc = svo_detect_into_seeds(ctx, pyr, slot, cam, n_pyr_levels, cell_size, occupancy_dev, detection_threshold, depth_mean, depth_min, &o);
  hipError_t e = hipSuccess;
  // resetGrid() (feature_detection.cpp:121), behind the detection on the stream
  if (rc == SVO_HIP_OK && occupancy_dev && clear_occupancy) e = hipMemsetAsync(occupancy_dev, 0, NC, ctx->stream);
  const hipError_t e_sync = hipStreamSynchronize(ctx->stream);                 // the one wait; also before the block may go back
  if (e == hipSuccess) e = e_sync;
  if (rc == SVO_HIP_OK && e != hipSuccess) rc = svo_fail(ctx, SVO_HIP_ERR_DEVICE, "svo_hip_seed_batch_create_detected", hipGetErrorString(e));
  const int n = rc == SVO_HIP_OK ? *reinterpret_cast<const int32_t*>(sb->host) : 0;
  if (rc == SVO_HIP_OK && n > 0) {
    const size_t N = (size_t)n;
    if (px) memcpy(px, sb->host + o_hpx, 16 * N);
    if (f) memcpy(f, sb->host + o_hf, 24 * N);
    if (level) memcpy(level, sb->host + o_hl, 4 * N);
    if (score) memcpy(score, sb->host + o_hs, 4 * N);
  }
  memset(sb->host, 0, kEvHeaderBytes);                     // the header as svo_hip_seed_batch_create leaves it
  if (rc != SVO_HIP_OK || n == 0) {                        // no seeds: no batch, the block back in the pool
    sb_return_block(ctx, sb->blk);
    delete sb;
    return rc;
  }
  sb->n = n; sb->n_alive = n; sb->n_blocks = (n + 255) / 256;
  *n_out = n;
  *out = sb;
  return SVO_HIP_OK;
}

}  // extern "C"
