// svo_two_view_impl.h -- the bootstrap on the device, second half: the relative pose, the gates, the map scale, the second
// frame's pose and the first map points from the KLT lists a svo_hip_klt handle holds, for any subset of its cameras in one
// set of launches.
//
//   computeFundamental                  S/initialization.cpp:260-329  (svo_hip_klt_two_view)
//   KltHomographyInit::addSecondFrame   S/initialization.cpp:77-138   (svo_hip_klt_two_view; the Point / Feature objects are the host's)
//
// The kernels are in svo_two_view_device.h, the arithmetic in svo_two_view_math.h.  This file holds the stage's host side and
// entry points and is compiled as part of svo_klt.hip's translation unit (included at its end, nowhere else): the Makefile's
// source list is one of the files the committed counter profiles under profiles/ are keyed to, and a unit of its own would
// have put every one of them out of date for a stage that changes none of the profiled kernels.
#pragma once
#include "svo_two_view_device.h"

using namespace svo_tv;

// the stage's memory: taken by a handle's first two-view call, released with the handle
struct svo_tv_state {
  TvDev dev;
  char* dev_block = nullptr;
  TvJob* jobs_dev = nullptr;
  char* host_block = nullptr;             // page-locked: [jobs][result blocks]
  TvJob* jobs_host = nullptr;
  TvResultBlock* res_host = nullptr;
  TvResultBlock* res_host_dev = nullptr;
  std::vector<char> has_result;           // the camera has a result block for its present lists
  std::vector<int> n_hyp;                 // the hypotheses of that call
};

void svo_tv_release(svo_hip_klt* k) {
  if (!k->tv) return;
  (void)hipFree(k->tv->dev_block); ++k->ctx->n_frees;
  (void)hipHostFree(k->tv->host_block); ++k->ctx->n_frees;
  delete k->tv;
  k->tv = nullptr;
}

namespace {
size_t tv_align16(size_t v) { return (v + 15) & ~(size_t)15; }

int tv_state(svo_hip_klt* k) {
  if (k->tv) return SVO_HIP_OK;
  svo_hip_ctx* ctx = k->ctx;
  const size_t nc = (size_t)k->n_cameras, mf = (size_t)k->max_features;
  size_t o = 0;
  const size_t o_count = o; o += tv_align16(nc * TV_MAX_HYPOTHESES * sizeof(int32_t));
  const size_t o_xyz = o; o += tv_align16(nc * mf * 3 * sizeof(double));
  const size_t o_pos = o; o += tv_align16(nc * mf * 3 * sizeof(double));
  const size_t o_inl = o; o += tv_align16(nc * mf * sizeof(int32_t));
  const size_t o_pti = o; o += tv_align16(nc * mf * sizeof(int32_t));
  const size_t o_jobs = o; o += tv_align16(nc * sizeof(TvJob));
  const size_t o_mask = o; o += tv_align16(nc * mf);
  svo_tv_state* s = new svo_tv_state;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&s->dev_block), o);
  if (e == hipSuccess) {
    ++ctx->n_allocs;
    e = hipMemsetAsync(s->dev_block, 0, o, ctx->stream);
  }
  const size_t h_jobs = tv_align16(nc * sizeof(TvJob)), h_res = tv_align16(nc * sizeof(TvResultBlock));
  if (e == hipSuccess) {
    e = hipHostMalloc(reinterpret_cast<void**>(&s->host_block), h_jobs + h_res, hipHostMallocDefault);
    if (e == hipSuccess) ++ctx->n_allocs;
  }
  char* host_dev = nullptr;
  if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void**>(&host_dev), s->host_block, 0);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    if (s->dev_block) { (void)hipFree(s->dev_block); ++ctx->n_frees; }
    if (s->host_block) { (void)hipHostFree(s->host_block); ++ctx->n_frees; }
    delete s;
    return svo_fail(ctx, e == hipErrorOutOfMemory ? SVO_HIP_ERR_NOMEM : SVO_HIP_ERR_DEVICE, "svo_hip_klt_two_view", hipGetErrorString(e));
  }
  memset(s->host_block, 0, h_jobs + h_res);
  char* b = s->dev_block;
  s->dev.count = reinterpret_cast<int32_t*>(b + o_count);
  s->dev.xyz = reinterpret_cast<double*>(b + o_xyz); s->dev.pt_pos = reinterpret_cast<double*>(b + o_pos);
  s->dev.inliers = reinterpret_cast<int32_t*>(b + o_inl); s->dev.pt_index = reinterpret_cast<int32_t*>(b + o_pti);
  s->dev.mask = reinterpret_cast<uint8_t*>(b + o_mask);
  s->jobs_dev = reinterpret_cast<TvJob*>(b + o_jobs);
  s->jobs_host = reinterpret_cast<TvJob*>(s->host_block);
  s->res_host = reinterpret_cast<TvResultBlock*>(s->host_block + h_jobs);
  s->res_host_dev = reinterpret_cast<TvResultBlock*>(host_dev + h_jobs);
  s->has_result.assign(nc, 0);
  s->n_hyp.assign(nc, 0);
  k->tv = s;
  return SVO_HIP_OK;
}
}  // namespace

extern "C" {

int svo_hip_two_view_default_params(svo_hip_two_view_params* p) {
  if (!p) return SVO_HIP_ERR_INVALID;
  p->reproj_thresh = 2.0;               // Config::poseOptimThresh() (:81)
  p->min_inliers = 40;                  // Config::initMinInliers() (:85)
  p->map_scale = 1.0;                   // Config::mapScale() (:105)
  p->n_hypotheses = 1024;
  p->seed = 0;
  return SVO_HIP_OK;
}

int svo_hip_klt_set_lists(svo_hip_klt* k, int camera, int n, const float* px_ref, const float* px_cur, const double* f_ref, const double* f_cur) {
  if (!k) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = k->ctx;
  SVO_REQUIRE(ctx, camera >= 0 && camera < k->n_cameras);
  if (!k->has_ref[camera]) return svo_fail(ctx, SVO_HIP_ERR_STATE, "svo_hip_klt_set_lists", "the camera has no reference");
  SVO_REQUIRE(ctx, n >= 0 && n <= k->max_features && (n == 0 || (px_ref && px_cur && f_ref && f_cur)));
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t m = (size_t)n, per = 4 * sizeof(float) + 6 * sizeof(double) + sizeof(int32_t);
  char* hs = nullptr;
  {
    const int rc = svo_ctx_host_staging(ctx, m * per + 64, &hs);
    if (rc != SVO_HIP_OK) return rc;
  }
  const size_t base = (size_t)camera * k->max_features;
  double* hfr = reinterpret_cast<double*>(hs);
  double* hfc = hfr + 3 * m;
  float* hpr = reinterpret_cast<float*>(hfc + 3 * m);
  float* hpc = hpr + 2 * m;
  int32_t* hi = reinterpret_cast<int32_t*>(hpc + 2 * m);
  int32_t* hn = hi + m;
  if (n) {
    memcpy(hfr, f_ref, 3 * m * sizeof(double)); memcpy(hfc, f_cur, 3 * m * sizeof(double));
    memcpy(hpr, px_ref, 2 * m * sizeof(float)); memcpy(hpc, px_cur, 2 * m * sizeof(float));
    for (int i = 0; i < n; ++i) hi[i] = i;
    SVO_CHECK_HIP(ctx, hipMemcpyAsync(k->dev.f_ref + 3 * base, hfr, 3 * m * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    SVO_CHECK_HIP(ctx, hipMemcpyAsync(k->dev.f_cur + 3 * base, hfc, 3 * m * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    SVO_CHECK_HIP(ctx, hipMemcpyAsync(k->dev.px_ref + 2 * base, hpr, 2 * m * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    SVO_CHECK_HIP(ctx, hipMemcpyAsync(k->dev.px_cur + 2 * base, hpc, 2 * m * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    SVO_CHECK_HIP(ctx, hipMemcpyAsync(k->dev.index + base, hi, m * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  }
  *hn = n;
  SVO_CHECK_HIP(ctx, hipMemcpyAsync(k->dev.n + camera, hn, sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  SVO_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  k->n_host[camera] = n;
  k->has_cur[camera] = 1;
  if (k->tv) k->tv->has_result[camera] = 0;
  return SVO_HIP_OK;
}

int svo_hip_klt_two_view(svo_hip_klt* k, int n, const int* cameras, const svo_hip_camera* cams, const double* T_ref_w,
                         const svo_hip_two_view_params* params, svo_hip_two_view_result* results) {
  if (!k) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = k->ctx;
  SVO_REQUIRE(ctx, n >= 1 && n <= k->n_cameras && cameras && cams && results);
  svo_hip_two_view_params prm;
  svo_hip_two_view_default_params(&prm);
  if (params) prm = *params;
  SVO_REQUIRE(ctx, prm.reproj_thresh > 0.0 && prm.reproj_thresh < INFINITY && prm.map_scale > 0.0 && prm.map_scale < INFINITY);
  SVO_REQUIRE(ctx, prm.min_inliers >= 0 && prm.n_hypotheses >= 1 && prm.n_hypotheses <= TV_MAX_HYPOTHESES);
  for (int i = 0; i < n; ++i) {
    SVO_REQUIRE(ctx, cameras[i] >= 0 && cameras[i] < k->n_cameras);
    for (int j = 0; j < i; ++j) SVO_REQUIRE(ctx, cameras[j] != cameras[i]);
    SVO_REQUIRE(ctx, cams[i].width > 0 && cams[i].height > 0 && fabs(cams[i].fx) > 0.0 && fabs(cams[i].fx) < INFINITY);
  }
  for (int i = 0; i < n; ++i) {
    if (!k->has_ref[cameras[i]]) return svo_fail(ctx, SVO_HIP_ERR_STATE, "svo_hip_klt_two_view", "a listed camera has no reference");
    if (!k->has_cur[cameras[i]])
      return svo_fail(ctx, SVO_HIP_ERR_STATE, "svo_hip_klt_two_view", "a listed camera has not been tracked since its reference was set");
  }
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  {
    const int rc = tv_state(k);
    if (rc != SVO_HIP_OK) return rc;
  }
  svo_tv_state* s = k->tv;
  const unsigned long long seq = ++k->seq;
  for (int i = 0; i < n; ++i) {
    const int c = cameras[i];
    TvJob& j = s->jobs_host[i];
    j.cam = c; j.n = k->n_host[c];
    j.width = cams[i].width; j.height = cams[i].height;
    j.error_multiplier2 = fabs(cams[i].fx);                                        // PinholeCamera::errorMultiplier2()
    for (int q = 0; q < 7; ++q) j.T_ref_w[q] = T_ref_w ? T_ref_w[7 * i + q] : (q == 6 ? 1.0 : 0.0);
    j.result = reinterpret_cast<char*>(s->res_host_dev + c);
    j.seq = seq;
    s->has_result[c] = 0;
  }
  TvPrm dp;
  dp.reproj_thresh = prm.reproj_thresh; dp.map_scale = prm.map_scale; dp.min_inliers = prm.min_inliers;
  dp.n_hypotheses = prm.n_hypotheses; dp.seed = prm.seed;
  SVO_CHECK_HIP(ctx, hipMemcpyAsync(s->jobs_dev, s->jobs_host, (size_t)n * sizeof(TvJob), hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(tv_hypothesis_kernel, dim3((prm.n_hypotheses + TV_HYP_THREADS - 1) / TV_HYP_THREADS, n), dim3(TV_HYP_THREADS), 0,
                     ctx->stream, k->dev, s->dev, (const TvJob*)s->jobs_dev, dp);
  hipLaunchKernelGGL(tv_finish_kernel, dim3(n), dim3(TV_FIN_THREADS), 0, ctx->stream, k->dev, s->dev, (const TvJob*)s->jobs_dev, dp);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  SVO_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));                          // the call's one synchronisation
  for (int i = 0; i < n; ++i) {
    const int c = cameras[i];
    const TvResultBlock& r = s->res_host[c];
    if (__atomic_load_n(&r.seq, __ATOMIC_ACQUIRE) != seq) return svo_fail(ctx, SVO_HIP_ERR_DEVICE, "svo_hip_klt_two_view", "result block not written");
    svo_hip_two_view_result& o = results[i];
    o.status = r.status; o.n_in = r.n_in;
    o.hypothesis = r.hypothesis; o.hypothesis_count = r.hypothesis_count;
    o.candidate = r.candidate; o.candidate_count = r.candidate_count;
    o.n_inliers = r.n_inliers; o.n_points = r.n_points;
    o.depth_median = r.depth_median; o.scale = r.scale;
    for (int q = 0; q < 7; ++q) { o.T_cur_from_ref[q] = r.T_cur_from_ref[q]; o.T_cur_w[q] = r.T_cur_w[q]; }
    s->has_result[c] = 1;
    s->n_hyp[c] = prm.n_hypotheses;
  }
  return SVO_HIP_OK;
}

int svo_hip_klt_download_two_view(svo_hip_klt* k, int camera, int32_t* status, int32_t* n, double* xyz_in_cur, uint8_t* mask, int32_t* n_inliers,
                                  int32_t* inliers, int32_t* n_points, int32_t* point_index, double* point_pos, int32_t* n_hypotheses,
                                  int32_t* hypothesis_count) {
  if (!k) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = k->ctx;
  SVO_REQUIRE(ctx, camera >= 0 && camera < k->n_cameras);
  if (!k->tv || !k->tv->has_result[camera])
    return svo_fail(ctx, SVO_HIP_ERR_STATE, "svo_hip_klt_download_two_view", "the camera has no two-view result for its lists");
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  svo_tv_state* s = k->tv;
  const TvResultBlock& r = s->res_host[camera];
  const size_t base = (size_t)camera * k->max_features;
  // what the call computed: nothing before the hypotheses, the mask behind a model, xyz behind the cheirality gate
  const bool have_counts = r.status != TV_TOO_FEW, have_mask = have_counts && r.status != TV_NO_MODEL;
  const bool have_xyz = r.status == TV_OK || r.status == TV_FEW_INLIERS;
  const size_t m = (size_t)r.n_in, ni = (size_t)r.n_inliers, np = (size_t)r.n_points;
  if (status) *status = r.status;
  if (n) *n = r.n_in;
  if (n_inliers) *n_inliers = r.n_inliers;
  if (n_points) *n_points = r.n_points;
  if (n_hypotheses) *n_hypotheses = have_counts ? s->n_hyp[camera] : 0;
  if (xyz_in_cur && have_xyz && m)
    SVO_CHECK_HIP(ctx, hipMemcpyAsync(xyz_in_cur, s->dev.xyz + 3 * base, 3 * m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (mask && m) {
    if (have_mask) SVO_CHECK_HIP(ctx, hipMemcpyAsync(mask, s->dev.mask + base, m, hipMemcpyDeviceToHost, ctx->stream));
    else memset(mask, 0, m);
  }
  if (inliers && ni) SVO_CHECK_HIP(ctx, hipMemcpyAsync(inliers, s->dev.inliers + base, ni * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (point_index && np)
    SVO_CHECK_HIP(ctx, hipMemcpyAsync(point_index, s->dev.pt_index + base, np * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (point_pos && np)
    SVO_CHECK_HIP(ctx, hipMemcpyAsync(point_pos, s->dev.pt_pos + 3 * base, 3 * np * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (hypothesis_count && have_counts)
    SVO_CHECK_HIP(ctx, hipMemcpyAsync(hypothesis_count, s->dev.count + (size_t)camera * TV_MAX_HYPOTHESES,
                                      (size_t)s->n_hyp[camera] * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  SVO_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SVO_HIP_OK;
}

}  // extern "C"
