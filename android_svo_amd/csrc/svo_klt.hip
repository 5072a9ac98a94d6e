// svo_klt.hip -- the bootstrap on the device: KLT tracking of the first frame's features for up to every camera of a group
// in one set of launches.
//
//   KltHomographyInit::addFirstFrame    S/initialization.cpp:32-51    (svo_hip_klt_set_reference / _set_reference_detected)
//   KltHomographyInit::addSecondFrame   S/initialization.cpp:61-75    (the tracking and the median; the gates are the host's)
//   trackKlt                            S/initialization.cpp:180-226  (svo_hip_klt_track)
//
// computeFundamental (:260-329) and the rest of addSecondFrame (:77-138) are svo_two_view_impl.h; computeHomography (:232-258, the
// path the reference has switched off) is not built.  The kernels are in svo_klt_device.h.
#include "svo_klt_device.h"

using namespace svo_klt;

namespace {
size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

KltPrm klt_prm(const svo_hip_klt_params& p) {
  KltPrm k;
  k.win = p.win_size; k.max_level = p.max_level; k.max_iter = p.max_iter;
  k.eps2 = p.eps * p.eps;
  k.min_eig = (float)p.min_eig_threshold;
  return k;
}

// levels 1.. of the previous image's pyramid of one camera (level 0 is in place)
void klt_build_prev(svo_hip_klt* k, int camera) {
  uint8_t* base = k->dev.prev_pyr + (size_t)camera * k->dev.pyr_bytes;
  for (int l = 0; l + 1 < k->lv.n_levels; ++l) {
    const int dw = k->lv.w[l + 1], dh = k->lv.h[l + 1];
    hipLaunchKernelGGL(klt_pyr_down_kernel, dim3((dw + 63) / 64, (dh + 3) / 4, 1), dim3(256), 0, k->ctx->stream, (const KltJob*)nullptr,
                       base + k->lv.off[l], (size_t)0, base + k->lv.off[l + 1], (size_t)0, k->lv.w[l], k->lv.h[l], dw, dh, 0);
  }
}

int klt_check_pyramid(svo_hip_klt* k, const svo_hip_pyramid* pyr, int slot) {
  SVO_REQUIRE(k->ctx, pyr && pyr->ctx == k->ctx && pyr->width == k->width && pyr->height == k->height);
  SVO_REQUIRE(k->ctx, slot >= 0 && slot < pyr->batch);
  return SVO_HIP_OK;
}
}  // namespace

extern "C" {

int svo_hip_klt_default_params(svo_hip_klt_params* p) {
  if (!p) return SVO_HIP_ERR_INVALID;
  p->win_size = 30; p->max_level = 4; p->max_iter = 30;           // trackKlt, S/initialization.cpp:189-201
  p->eps = 0.001; p->min_eig_threshold = 1e-4;
  return SVO_HIP_OK;
}

int svo_hip_klt_create(svo_hip_ctx* ctx, int width, int height, int n_cameras, int max_features, const svo_hip_klt_params* params,
                       svo_hip_klt** out) {
  if (!ctx) return SVO_HIP_ERR_INVALID;
  SVO_REQUIRE(ctx, out != nullptr);
  svo_hip_klt_params prm;
  svo_hip_klt_default_params(&prm);
  if (params) prm = *params;
  SVO_REQUIRE(ctx, prm.win_size >= 3 && prm.win_size <= KLT_MAX_WIN);              // the template's place in LDS
  SVO_REQUIRE(ctx, prm.max_level >= 0 && prm.max_level < SVO_HIP_MAX_LEVELS && prm.max_iter >= 0);
  SVO_REQUIRE(ctx, prm.eps >= 0.0 && prm.min_eig_threshold == prm.min_eig_threshold);
  // a window may hang off the image by its own size: one reflection reaches back only if the image exceeds the window
  SVO_REQUIRE(ctx, width > prm.win_size && height > prm.win_size && width <= 16384 && height <= 16384);
  SVO_REQUIRE(ctx, n_cameras >= 1 && n_cameras <= 1024 && max_features >= 1 && max_features <= (1 << 20));
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  svo_hip_klt* k = new svo_hip_klt;
  k->ctx = ctx; k->width = width; k->height = height; k->n_cameras = n_cameras; k->max_features = max_features; k->prm = prm;
  memset(&k->lv, 0, sizeof(k->lv));
  {
    // cv::buildOpticalFlowPyramid: level l + 1 is ((w + 1) / 2, (h + 1) / 2) and exists only while both exceed the window
    int w = width, h = height;
    size_t off = 0;
    int n = 0;
    for (;;) {
      k->lv.w[n] = w; k->lv.h[n] = h; k->lv.off[n] = (unsigned)off;
      off += align16((size_t)w * h);
      ++n;
      if (n > prm.max_level) break;
      w = (w + 1) / 2; h = (h + 1) / 2;
      if (!(w > prm.win_size && h > prm.win_size)) break;
    }
    k->lv.n_levels = n;
    k->dev.pyr_bytes = off;
  }
  const size_t nc = (size_t)n_cameras, mf = (size_t)max_features;
  size_t o = 0;
  const size_t o_prev = o; o += align16(nc * k->dev.pyr_bytes);
  const size_t o_cur = o; o += align16(nc * k->dev.pyr_bytes);
  const size_t o_fref = o; o += align16(nc * mf * 3 * sizeof(double));
  const size_t o_fcur = o; o += align16(nc * mf * 3 * sizeof(double));
  const size_t o_disp = o; o += align16(nc * mf * sizeof(double));
  const size_t o_pref = o; o += align16(nc * mf * 2 * sizeof(float));
  const size_t o_pcur = o; o += align16(nc * mf * 2 * sizeof(float));
  const size_t o_idx = o; o += align16(nc * mf * sizeof(int32_t));
  const size_t o_n = o; o += align16(nc * sizeof(int32_t));
  const size_t o_jobs = o; o += align16(nc * sizeof(KltJob));
  const size_t o_status = o; o += align16(nc * mf);
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&k->dev_block), o);
  if (e == hipSuccess) {
    ++ctx->n_allocs;
    e = hipMemsetAsync(k->dev_block, 0, o, ctx->stream);
  }
  const size_t h_jobs = align16(nc * sizeof(KltJob)), h_res = align16(nc * sizeof(KltResultBlock));
  if (e == hipSuccess) {
    e = hipHostMalloc(reinterpret_cast<void**>(&k->host_block), h_jobs + h_res + 16, hipHostMallocDefault);
    if (e == hipSuccess) ++ctx->n_allocs;
  }
  char* host_dev = nullptr;
  if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void**>(&host_dev), k->host_block, 0);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    if (k->dev_block) { (void)hipFree(k->dev_block); ++ctx->n_frees; }
    if (k->host_block) { (void)hipHostFree(k->host_block); ++ctx->n_frees; }
    delete k;
    return svo_fail(ctx, e == hipErrorOutOfMemory ? SVO_HIP_ERR_NOMEM : SVO_HIP_ERR_DEVICE, "svo_hip_klt_create", hipGetErrorString(e));
  }
  memset(k->host_block, 0, h_jobs + h_res + 16);
  char* b = k->dev_block;
  k->dev.prev_pyr = reinterpret_cast<uint8_t*>(b + o_prev); k->dev.cur_pyr = reinterpret_cast<uint8_t*>(b + o_cur);
  k->dev.f_ref = reinterpret_cast<double*>(b + o_fref); k->dev.f_cur = reinterpret_cast<double*>(b + o_fcur);
  k->dev.disparity = reinterpret_cast<double*>(b + o_disp);
  k->dev.px_ref = reinterpret_cast<float*>(b + o_pref); k->dev.px_cur = reinterpret_cast<float*>(b + o_pcur);
  k->dev.index = reinterpret_cast<int32_t*>(b + o_idx); k->dev.n = reinterpret_cast<int32_t*>(b + o_n);
  k->dev.status = reinterpret_cast<uint8_t*>(b + o_status);
  k->dev.max_features = max_features;
  k->jobs_dev = reinterpret_cast<KltJob*>(b + o_jobs);
  k->jobs_host = reinterpret_cast<KltJob*>(k->host_block);
  k->res_host = reinterpret_cast<KltResultBlock*>(k->host_block + h_jobs);
  k->res_host_dev = reinterpret_cast<KltResultBlock*>(host_dev + h_jobs);
  k->det_n_host = reinterpret_cast<int32_t*>(k->host_block + h_jobs + h_res);
  k->det_n_host_dev = reinterpret_cast<int32_t*>(host_dev + h_jobs + h_res);
  k->n_host.assign(nc, 0);
  k->has_ref.assign(nc, 0);
  k->has_cur.assign(nc, 0);
  *out = k;
  return SVO_HIP_OK;
}

int svo_hip_klt_destroy(svo_hip_klt* k) {
  if (!k) return SVO_HIP_ERR_INVALID;
  (void)hipSetDevice(k->ctx->device);
  (void)hipStreamSynchronize(k->ctx->stream);
  svo_tv_release(k);
  (void)hipFree(k->dev_block); ++k->ctx->n_frees;
  (void)hipHostFree(k->host_block); ++k->ctx->n_frees;
  delete k;
  return SVO_HIP_OK;
}

int svo_hip_klt_info(const svo_hip_klt* k, int* n_levels, int* level_width, int* level_height) {
  if (!k) return SVO_HIP_ERR_INVALID;
  if (n_levels) *n_levels = k->lv.n_levels;
  for (int l = 0; l < k->lv.n_levels; ++l) {
    if (level_width) level_width[l] = k->lv.w[l];
    if (level_height) level_height[l] = k->lv.h[l];
  }
  return SVO_HIP_OK;
}

int svo_hip_klt_set_reference(svo_hip_klt* k, int camera, const svo_hip_pyramid* pyr, int slot, int n, const float* px, const double* f) {
  if (!k) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = k->ctx;
  SVO_REQUIRE(ctx, camera >= 0 && camera < k->n_cameras);
  {
    const int rc = klt_check_pyramid(k, pyr, slot);
    if (rc != SVO_HIP_OK) return rc;
  }
  SVO_REQUIRE(ctx, n >= 0 && n <= k->max_features && (n == 0 || (px && f)));
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t per = 2 * sizeof(float) + 3 * sizeof(double) + sizeof(int32_t);
  char* hs = nullptr;
  {
    const int rc = svo_ctx_host_staging(ctx, (size_t)n * per + 64, &hs);
    if (rc != SVO_HIP_OK) return rc;
  }
  const size_t base = (size_t)camera * k->max_features;
  SVO_CHECK_HIP(ctx, hipMemcpyAsync(k->dev.prev_pyr + (size_t)camera * k->dev.pyr_bytes, pyr->base + (size_t)slot * pyr->pyr_bytes + pyr->level_offset[0],
                                    (size_t)k->width * k->height, hipMemcpyDeviceToDevice, ctx->stream));
  klt_build_prev(k, camera);
  double* hf = reinterpret_cast<double*>(hs);
  float* hp = reinterpret_cast<float*>(hf + 3 * (size_t)n);
  int32_t* hi = reinterpret_cast<int32_t*>(hp + 2 * (size_t)n);
  int32_t* hn = hi + n;
  if (n) {
    memcpy(hf, f, 3 * (size_t)n * sizeof(double));
    memcpy(hp, px, 2 * (size_t)n * sizeof(float));
    for (int i = 0; i < n; ++i) hi[i] = i;
    SVO_CHECK_HIP(ctx, hipMemcpyAsync(k->dev.f_ref + 3 * base, hf, 3 * (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    SVO_CHECK_HIP(ctx, hipMemcpyAsync(k->dev.px_ref + 2 * base, hp, 2 * (size_t)n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    // px_cur_.insert(px_cur_.begin(), px_ref_.begin(), px_ref_.end()) (:49): the first call's initial flow
    SVO_CHECK_HIP(ctx, hipMemcpyAsync(k->dev.px_cur + 2 * base, hp, 2 * (size_t)n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    SVO_CHECK_HIP(ctx, hipMemcpyAsync(k->dev.index + base, hi, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  }
  *hn = n;
  SVO_CHECK_HIP(ctx, hipMemcpyAsync(k->dev.n + camera, hn, sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  SVO_CHECK_HIP(ctx, hipGetLastError());
  SVO_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  k->n_host[camera] = n;
  k->has_ref[camera] = 1;
  k->has_cur[camera] = 0;
  return SVO_HIP_OK;
}

int svo_hip_klt_set_reference_detected(svo_hip_klt* k, int camera, const svo_hip_pyramid* pyr, int slot, const svo_hip_camera* cam,
                                       int n_pyr_levels, int cell_size, double detection_threshold, int32_t* n) {
  if (!k) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = k->ctx;
  SVO_REQUIRE(ctx, camera >= 0 && camera < k->n_cameras && n != nullptr);
  {
    int rc = klt_check_pyramid(k, pyr, slot);
    if (rc == SVO_HIP_OK) rc = svo_detect_check_args(ctx, pyr, slot, cam, n_pyr_levels, cell_size, detection_threshold);
    if (rc != SVO_HIP_OK) return rc;
  }
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  int gc = 0, gr = 0;
  svo_hip_detect_grid(pyr->width, pyr->height, cell_size, &gc, &gr);
  const size_t nc = (size_t)gc * gr;
  char* d = nullptr;
  {
    const int rc = svo_ctx_staging(ctx, nc * (5 * sizeof(double) + sizeof(int32_t)) + 64, &d);
    if (rc != SVO_HIP_OK) return rc;
  }
  double* dpx = reinterpret_cast<double*>(d);
  double* df = dpx + 2 * nc;
  int32_t* dl = reinterpret_cast<int32_t*>(df + 3 * nc);
  int32_t* dn = dl + nc;
  {
    const int rc = svo_hip_detect_features_dev(ctx, pyr, slot, cam, n_pyr_levels, cell_size, nullptr, detection_threshold, dn, dpx, df, dl, nullptr);
    if (rc != SVO_HIP_OK) return rc;
  }
  const int blocks = (int)((nc + 255) / 256) < 32 ? (int)((nc + 255) / 256) : 32;
  hipLaunchKernelGGL(klt_take_detection_kernel, dim3(blocks > 0 ? blocks : 1), dim3(256), 0, ctx->stream, k->dev, camera, dn, dpx, df, k->det_n_host_dev);
  SVO_CHECK_HIP(ctx, hipMemcpyAsync(k->dev.prev_pyr + (size_t)camera * k->dev.pyr_bytes, pyr->base + (size_t)slot * pyr->pyr_bytes + pyr->level_offset[0],
                                    (size_t)k->width * k->height, hipMemcpyDeviceToDevice, ctx->stream));
  klt_build_prev(k, camera);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  SVO_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int n_det = *k->det_n_host;
  *n = n_det;
  if (n_det > k->max_features) {                       // known only now: the camera is left WITHOUT a reference
    k->n_host[camera] = 0; k->has_ref[camera] = 0; k->has_cur[camera] = 0;
    return svo_fail(ctx, SVO_HIP_ERR_INVALID, "svo_hip_klt_set_reference_detected", "more features than max_features");
  }
  k->n_host[camera] = n_det;
  k->has_ref[camera] = 1;
  k->has_cur[camera] = 0;
  return SVO_HIP_OK;
}

int svo_hip_klt_set_flow(svo_hip_klt* k, int camera, int n, const float* px_cur) {
  if (!k) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = k->ctx;
  SVO_REQUIRE(ctx, camera >= 0 && camera < k->n_cameras);
  if (!k->has_ref[camera]) return svo_fail(ctx, SVO_HIP_ERR_STATE, "svo_hip_klt_set_flow", "the camera has no reference");
  SVO_REQUIRE(ctx, n == k->n_host[camera] && (n == 0 || px_cur));
  if (n == 0) return SVO_HIP_OK;
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  char* hs = nullptr;
  {
    const int rc = svo_ctx_host_staging(ctx, (size_t)n * 2 * sizeof(float), &hs);
    if (rc != SVO_HIP_OK) return rc;
  }
  memcpy(hs, px_cur, (size_t)n * 2 * sizeof(float));
  SVO_CHECK_HIP(ctx, hipMemcpyAsync(k->dev.px_cur + 2 * (size_t)camera * k->max_features, hs, (size_t)n * 2 * sizeof(float), hipMemcpyHostToDevice,
                                    ctx->stream));
  SVO_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SVO_HIP_OK;
}

int svo_hip_klt_track(svo_hip_klt* k, int n, const int* cameras, const svo_hip_pyramid* cur, const int* slots, const svo_hip_camera* cams,
                      svo_hip_klt_result* results) {
  if (!k) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = k->ctx;
  SVO_REQUIRE(ctx, n >= 1 && n <= k->n_cameras && cameras && slots && cams && results);
  SVO_REQUIRE(ctx, cur && cur->ctx == ctx && cur->width == k->width && cur->height == k->height);
  for (int i = 0; i < n; ++i) {
    SVO_REQUIRE(ctx, cameras[i] >= 0 && cameras[i] < k->n_cameras);
    SVO_REQUIRE(ctx, slots[i] >= 0 && slots[i] < cur->batch);
    for (int j = 0; j < i; ++j) SVO_REQUIRE(ctx, cameras[j] != cameras[i]);
  }
  for (int i = 0; i < n; ++i)
    if (!k->has_ref[cameras[i]]) return svo_fail(ctx, SVO_HIP_ERR_STATE, "svo_hip_klt_track", "a listed camera has no reference");
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  const unsigned long long seq = ++k->seq;
  int max_n = 0;
  for (int i = 0; i < n; ++i) {
    const int c = cameras[i];
    KltJob& j = k->jobs_host[i];
    j.cam = c; j.pad = 0;
    j.cur_l0 = cur->base + (size_t)slots[i] * cur->pyr_bytes + cur->level_offset[0];
    j.result = reinterpret_cast<char*>(k->res_host_dev + c);
    j.seq = seq;
    j.model = svo_make_cam(cams[i]);
    if (k->n_host[c] > max_n) max_n = k->n_host[c];
  }
  SVO_CHECK_HIP(ctx, hipMemcpyAsync(k->jobs_dev, k->jobs_host, (size_t)n * sizeof(KltJob), hipMemcpyHostToDevice, ctx->stream));
  if (max_n > 0) {
    for (int l = 0; l + 1 < k->lv.n_levels; ++l) {
      const int dw = k->lv.w[l + 1], dh = k->lv.h[l + 1];
      hipLaunchKernelGGL(klt_pyr_down_kernel, dim3((dw + 63) / 64, (dh + 3) / 4, n), dim3(256), 0, ctx->stream, (const KltJob*)k->jobs_dev,
                         (const uint8_t*)k->dev.cur_pyr + k->lv.off[l], k->dev.pyr_bytes, k->dev.cur_pyr + k->lv.off[l + 1], k->dev.pyr_bytes,
                         k->lv.w[l], k->lv.h[l], dw, dh, l == 0 ? 1 : 0);
    }
    hipLaunchKernelGGL(klt_track_kernel, dim3((max_n + KLT_WAVES - 1) / KLT_WAVES, n), dim3(256), 0, ctx->stream, k->dev, k->lv,
                       (const KltJob*)k->jobs_dev, klt_prm(k->prm));
  }
  hipLaunchKernelGGL(klt_finish_kernel, dim3(n), dim3(KLT_FIN_THREADS), 0, ctx->stream, k->dev, (const KltJob*)k->jobs_dev);
  SVO_CHECK_HIP(ctx, hipGetLastError());
  SVO_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));                          // the call's one synchronisation
  for (int i = 0; i < n; ++i) {
    const int c = cameras[i];
    const KltResultBlock& r = k->res_host[c];
    if (__atomic_load_n(&r.seq, __ATOMIC_ACQUIRE) != seq) return svo_fail(ctx, SVO_HIP_ERR_DEVICE, "svo_hip_klt_track", "result block not written");
    results[i].n_in = r.n_in; results[i].n_tracked = r.n_tracked; results[i].n_levels = k->lv.n_levels;
    results[i].disparity_median = r.median;
    k->n_host[c] = r.n_tracked;
    k->has_cur[c] = 1;
  }
  return SVO_HIP_OK;
}

int svo_hip_klt_download(svo_hip_klt* k, int camera, int32_t* n, float* px_ref, float* px_cur, double* f_ref, double* f_cur, double* disparity,
                         int32_t* index) {
  if (!k) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = k->ctx;
  SVO_REQUIRE(ctx, camera >= 0 && camera < k->n_cameras);
  if (!k->has_ref[camera]) return svo_fail(ctx, SVO_HIP_ERR_STATE, "svo_hip_klt_download", "the camera has no reference");
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t m = (size_t)k->n_host[camera], base = (size_t)camera * k->max_features;
  if (n) *n = (int32_t)m;
  if (m) {
    if (px_ref) SVO_CHECK_HIP(ctx, hipMemcpyAsync(px_ref, k->dev.px_ref + 2 * base, 2 * m * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (px_cur) SVO_CHECK_HIP(ctx, hipMemcpyAsync(px_cur, k->dev.px_cur + 2 * base, 2 * m * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (f_ref) SVO_CHECK_HIP(ctx, hipMemcpyAsync(f_ref, k->dev.f_ref + 3 * base, 3 * m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (f_cur) SVO_CHECK_HIP(ctx, hipMemcpyAsync(f_cur, k->dev.f_cur + 3 * base, 3 * m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (disparity) SVO_CHECK_HIP(ctx, hipMemcpyAsync(disparity, k->dev.disparity + base, m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (index) SVO_CHECK_HIP(ctx, hipMemcpyAsync(index, k->dev.index + base, m * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    SVO_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return SVO_HIP_OK;
}

int svo_hip_klt_download_level(svo_hip_klt* k, int camera, int current, int level, uint8_t* out) {
  if (!k) return SVO_HIP_ERR_INVALID;
  svo_hip_ctx* ctx = k->ctx;
  SVO_REQUIRE(ctx, camera >= 0 && camera < k->n_cameras && out);
  SVO_REQUIRE(ctx, level >= (current ? 1 : 0) && level < k->lv.n_levels);
  SVO_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  const uint8_t* src = (current ? k->dev.cur_pyr : k->dev.prev_pyr) + (size_t)camera * k->dev.pyr_bytes + k->lv.off[level];
  SVO_CHECK_HIP(ctx, hipMemcpyAsync(out, src, (size_t)k->lv.w[level] * k->lv.h[level], hipMemcpyDeviceToHost, ctx->stream));
  SVO_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SVO_HIP_OK;
}

}  // extern "C"

// the two-view stage on the same handle: svo_hip_klt_two_view / _download_two_view / _set_lists
#include "svo_two_view_impl.h"
