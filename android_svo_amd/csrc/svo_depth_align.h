// svo_depth_align.h -- the sub-pixel alignment kernels: align2D / align1D over a batch of patches, and the alignment stage of the
// depth-filter and findMatchDirect pipelines over the records the search stage left.
#pragma once
#include "svo_depth_types.h"
namespace {
// ---- align2D / align1D over n patches: one DPP quad per patch, 16 patches per single-wave workgroup ------------
// The [n][100] (and optional [n][64]) patch arrays are read with coalesced word loads into LDS and handed to the
// lanes from there: lane q of a patch takes the ten words of border rows 2q .. 2q+3 (svo_align_device.h).
// One wave per workgroup: a wave leaves as soon as its own 16 patches are done and its slot is refilled at once
// (with 4-wave workgroups the next workgroup waited for the slowest of 64 patches: measured average residency 2.0 of
// 4 waves per SIMD at 200 000 patches).
SVO_DEV void stage_patch_words(const uint8_t* __restrict__ pwb, const uint8_t* __restrict__ ref_patch, int first, int n,
                               uint32_t* s_words, QuadPatch& qp) {
  const int tid = threadIdx.x;
  const int pl = tid >> 2, q = tid & 3;
  const int n_here = min(ALIGN_PATCHES, n - first);
  const uint32_t* src = reinterpret_cast<const uint32_t*>(pwb + (size_t)first * 100);
  // unconditional loads at a clamped index: all of a thread's loads are in flight together (words beyond the last
  // patch are never used)
  const int last = n_here * 25 - 1;
  uint32_t stage[ALIGN_STAGE_ROUNDS];
#pragma unroll
  for (int k = 0; k < ALIGN_STAGE_ROUNDS; ++k) stage[k] = src[min(k * ALIGN_BLOCK + tid, last)];      // all in flight together
#pragma unroll
  for (int k = 0; k < ALIGN_STAGE_ROUNDS; ++k) s_words[k * ALIGN_BLOCK + tid] = stage[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 10; ++k) qp.b[k] = s_words[pl * 25 + 5 * q + k];
  if (ref_patch) {
    __syncthreads();
    const uint32_t* src2 = reinterpret_cast<const uint32_t*>(ref_patch + (size_t)first * 64);
    const int last2 = n_here * 16 - 1;
#pragma unroll
    for (int k = 0; k < ALIGN_PATCHES * 16 / ALIGN_BLOCK; ++k) {
      const int w = k * ALIGN_BLOCK + tid;
      s_words[w + (w >> 4)] = src2[min(w, last2)];                 // row stride 17 words: conflict-free reads
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) qp.p[k] = s_words[pl * 17 + 4 * q + k];
  } else {
    patch_from_border(qp);
  }
}

__global__ __launch_bounds__(ALIGN_BLOCK) void align2d_kernel(const uint8_t* __restrict__ img, int cols, int rows, int n,
                                                              const uint8_t* __restrict__ pwb,
                                                              const uint8_t* __restrict__ ref_patch, int n_iter,
                                                              double* __restrict__ px, uint8_t* __restrict__ converged,
                                                              int32_t* __restrict__ iters) {
  __shared__ uint32_t s_words[ALIGN_STAGE_WORDS];
  const int first = blockIdx.x * ALIGN_PATCHES;
  const int w = first + (threadIdx.x >> 2);
  const bool have = w < n;
  QuadPatch qp;
  stage_patch_words(pwb, ref_patch, first, n, s_words, qp);
  double u = 0.0, v = 0.0;
  if (have) { u = px[2 * (size_t)w]; v = px[2 * (size_t)w + 1]; }
  int it = 0;
  const bool ok = align2d_quad(img, cols, rows, cols, qp, n_iter, have, &u, &v, &it);
  if (have && (threadIdx.x & 3) == 0) {
    px[2 * (size_t)w] = u;
    px[2 * (size_t)w + 1] = v;
    converged[w] = ok ? 1 : 0;
    if (iters) iters[w] = it;
  }
}

// align1D over n patches (edgelets / Matcher::Options::align_1d; secondary)
__global__ __launch_bounds__(ALIGN_BLOCK) void align1d_kernel(const uint8_t* __restrict__ img, int cols, int rows, int n,
                                                              const uint8_t* __restrict__ pwb,
                                                              const uint8_t* __restrict__ ref_patch,
                                                              const float* __restrict__ dir, int n_iter,
                                                              double* __restrict__ px, uint8_t* __restrict__ converged,
                                                              double* __restrict__ h_inv, int32_t* __restrict__ iters) {
  __shared__ uint32_t s_words[ALIGN_STAGE_WORDS];
  const int first = blockIdx.x * ALIGN_PATCHES;
  const int w = first + (threadIdx.x >> 2);
  const bool have = w < n;
  QuadPatch qp;
  stage_patch_words(pwb, ref_patch, first, n, s_words, qp);
  double u = 0.0, v = 0.0, hi = 0.0;
  float d0 = 0.0f, d1 = 0.0f;
  if (have) { u = px[2 * (size_t)w]; v = px[2 * (size_t)w + 1]; d0 = dir[2 * (size_t)w]; d1 = dir[2 * (size_t)w + 1]; }
  int it = 0;
  const bool ok = align1d_quad(img, cols, rows, cols, d0, d1, qp, n_iter, have, &u, &v, &hi, &it);
  if (have && (threadIdx.x & 3) == 0) {
    px[2 * (size_t)w] = u;
    px[2 * (size_t)w + 1] = v;
    converged[w] = ok ? 1 : 0;
    if (h_inv) h_inv[w] = hi;
    if (iters) iters[w] = it;
  }
}

// Sub-pixel refinement of every seed the search stage flagged: one quad per seed, the reference's serial pixel order
// (svo_align_device.h), so `converged`, the refined pixel and the iteration count equal the CPU path's bit for bit.
// ONE_D = false refines the corner features with align2D; ONE_D = true the EDGELET reference features of
// findMatchDirect with align1D (matcher.cpp:183-191; the depth filter never produces them).
// (the body: this lane is lane q = threadIdx.x & 3 of the quad of seed i; `have` = the seed exists)
template <bool ONE_D>
SVO_DEV void df_align_quad(const DfFrame& fr, const uint8_t* __restrict__ cur_pyr, int n_pad, const uint32_t* __restrict__ pwb_t,
                           SeedRec* __restrict__ recs, int i, bool have) {
  const int q = threadIdx.x & 3;
  if (__builtin_amdgcn_ballot_w64(have) == 0ull) return;
  SeedRec* rp = recs + (have ? i : 0);
  // ONE trip to memory for everything the quad needs: lane q takes one 16-byte word of the seed's record -- {step}, {search
  // level, path, status, warp_nan}, {matched, counters}, {uv0} -- and its ten words of the warped patch, all asked for at
  // once; the fields then go round the quad by DPP.  (Round 3 read `path` and `matched` first, the other fields and the
  // patch words -- only where the seed is to be aligned -- after them: two dependent trips to HBM at the head of every
  // wave, in a stage whose set-up part is a third of its time: 79 of 264 us at 1 M seeds, tools/df_iter_probe.py.)
  static_assert(offsetof(SeedRec, step) == 16 && offsetof(SeedRec, search_level) == 64 && offsetof(SeedRec, path) == 68 &&
                offsetof(SeedRec, matched) == 80 && offsetof(SeedRec, uv0) == 0, "record words read below");
  const int word = q == 0 ? 1 : (q == 1 ? 4 : (q == 2 ? 5 : 0));
  const uint4 mine_w = reinterpret_cast<const uint4*>(rp)[word];
  QuadPatch qp;
#pragma unroll
  for (int k = 0; k < 10; ++k) qp.b[k] = pwb_t[(size_t)(5 * q + k) * n_pad + (have ? i : 0)];     // (read-only scratch: any content is valid)
  const int search_level_r = quad_bcast<1>((int)mine_w.x);
  const int path = have ? quad_bcast<1>((int)mine_w.y) : -1;
  const int matched_r = quad_bcast<2>((int)mine_w.x);
  const bool mine = ONE_D ? path == 3 : (path == 0 || path == 1);
  const bool do_align = mine && matched_r == 2;
  const double step0 = __hiloint2double(quad_bcast<0>((int)mine_w.y), quad_bcast<0>((int)mine_w.x));
  const double step1 = __hiloint2double(quad_bcast<0>((int)mine_w.w), quad_bcast<0>((int)mine_w.z));
  const double uv00 = __hiloint2double(quad_bcast<3>((int)mine_w.y), quad_bcast<3>((int)mine_w.x));
  const double uv01 = __hiloint2double(quad_bcast<3>((int)mine_w.w), quad_bcast<3>((int)mine_w.z));
  if (__builtin_amdgcn_ballot_w64(do_align) == 0ull) return;      // wave-uniform
  const int search_level = do_align ? search_level_r : 0;
  const int ccols = fr.cam.width >> search_level, crows = fr.cam.height >> search_level;
  const uint8_t* cur_img = cur_pyr + fr.cur_level_off[search_level];
  patch_from_border(qp);
  double px_cur[2] = {0.0, 0.0};
  float dir0 = 0.0f, dir1 = 0.0f;
  if (do_align) {
    if (ONE_D) { px_cur[0] = uv00; px_cur[1] = uv01; dir0 = (float)step0; dir1 = (float)step1; }
    else { px_cur[0] = step0; px_cur[1] = step1; }
  }
  const double inv_scale = 1.0 / (1 << search_level);    // exact: a power of two
  double us = px_cur[0] * inv_scale, vs = px_cur[1] * inv_scale;
  int n_align = 0;
  bool res;
  if (ONE_D) {
    double h_inv;
    res = align1d_quad(cur_img, ccols, crows, ccols, dir0, dir1, qp, fr.align_max_iter, do_align, &us, &vs, &h_inv, &n_align);
  } else {
    res = align2d_quad(cur_img, ccols, crows, ccols, qp, fr.align_max_iter, do_align, &us, &vs, &n_align);
  }
  if (do_align && q == 0) {
    if (res || fr.keep_px_on_failure) {
      px_cur[0] = us * (1 << search_level);
      px_cur[1] = vs * (1 << search_level);
    }
    rp->matched = res ? 1 : 0;
    rp->step[0] = px_cur[0]; rp->step[1] = px_cur[1];
    rp->n_align = n_align;
  }
}

template <bool ONE_D>
__global__ __launch_bounds__(ALIGN_BLOCK) void df_align_kernel(DfFrame fr, const uint8_t* __restrict__ cur_pyr, int n, int n_pad,
                                                               const uint32_t* __restrict__ pwb_t, SeedRec* __restrict__ recs) {
  const int i = blockIdx.x * ALIGN_PATCHES + (threadIdx.x >> 2);
  df_align_quad<ONE_D>(fr, cur_pyr, n_pad, pwb_t, recs, i, i < n);
}

// (the alignment stage over the candidates of the cameras of a tracker: the layout of df_search_cams_kernel, svo_depth_search.h)
template <bool ONE_D>
__global__ __launch_bounds__(ALIGN_BLOCK) void df_align_cams_kernel(DfFrame fr, const uint8_t* __restrict__ cur_base, size_t cur_pyr_bytes, int cap,
                                                                    const int* __restrict__ counters, int counter_stride, int n_pad,
                                                                    const uint32_t* __restrict__ pwb_t, SeedRec* __restrict__ recs) {
  const int i = blockIdx.x * ALIGN_PATCHES + (threadIdx.x >> 2);
  const int c = (int)(((long long)blockIdx.x * ALIGN_PATCHES) / cap);
  int n_c = counters[(size_t)c * counter_stride];
  n_c = n_c < cap ? n_c : cap;
  df_align_quad<ONE_D>(fr, cur_base + (size_t)c * cur_pyr_bytes, n_pad, pwb_t, recs, i, i < c * cap + n_c);
}

// (the same over the cameras a list names: the layout of df_search_listed_kernel, svo_depth_search.h)
template <bool ONE_D>
__global__ __launch_bounds__(ALIGN_BLOCK) void df_align_listed_kernel(DfFrame fr, const uint8_t* __restrict__ cur_base, size_t cur_pyr_bytes, int cap,
                                                                      const int* __restrict__ counters, int counter_stride, int n_pad,
                                                                      const uint32_t* __restrict__ pwb_t, SeedRec* __restrict__ recs,
                                                                      const int* __restrict__ cam_list) {
  const int per_cam = cap / ALIGN_PATCHES;
  const int j = (int)blockIdx.x / per_cam;
  const int c = cam_list[j];
  const int i = (c * per_cam + ((int)blockIdx.x - j * per_cam)) * ALIGN_PATCHES + (threadIdx.x >> 2);
  int n_c = counters[(size_t)c * counter_stride];
  n_c = n_c < cap ? n_c : cap;
  df_align_quad<ONE_D>(fr, cur_base + (size_t)c * cur_pyr_bytes, n_pad, pwb_t, recs, i, i < c * cap + n_c);
}

// (the alignment stage over the batches of several cameras: the layout of df_search_jobs_kernel, svo_depth_search.h)
__global__ __launch_bounds__(ALIGN_BLOCK) void df_align_jobs_kernel(DfFrame fr, const DfCamJob* __restrict__ jobs, const int* __restrict__ block_job,
                                                                    const uint8_t* __restrict__ cur_base, size_t cur_pyr_bytes, int n_pad,
                                                                    const uint32_t* __restrict__ pwb_t, SeedRec* __restrict__ recs) {
  const int i = blockIdx.x * ALIGN_PATCHES + (threadIdx.x >> 2);
  const DfCamJob& C = jobs[block_job[blockIdx.x / (256 / ALIGN_PATCHES)]];
  df_align_quad<false>(fr, cur_base + (size_t)C.cur_slot * cur_pyr_bytes, n_pad, pwb_t, recs, i, i < C.job.first_block * 256 + C.job.n);
}
}  // namespace
