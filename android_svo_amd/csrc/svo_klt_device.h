// svo_klt_device.h -- kernels of the bootstrap's KLT tracker (svo_klt.hip).
//
//   trackKlt                    S/initialization.cpp:180-226  (cv::calcOpticalFlowPyrLK, 30 x 30 window, 4 levels, 30 iterations,
//                                                              OPTFLOW_USE_INITIAL_FLOW; erasures, bearings, disparities)
//   vk::getMedian               the upper median of the disparities (addSecondFrame, :72)
//
// cv::calcOpticalFlowPyrLK / cv::buildOpticalFlowPyramid / cv::pyrDown are OpenCV 4.5.4 code that is not in the reference's
// tree: PARITY UNPINNED.  The algorithm is restated in tests/klt_reference.py, and these kernels are held to that model by bits:
// integer pyramid, integer Scharr derivatives, integer bilinear window samples, exact integer window sums converted to f32
// once, and an f32 chain in which every operation is rounded on its own (-ffp-contract=off; roots and quotients through f64,
// which rounds to the correctly rounded f32 result).
#pragma once
#include "svo_klt_types.h"

namespace svo_klt {

// BORDER_REFLECT_101 for an index at most n - 1 beyond the image (what a window and its derivative neighbourhood reach);
// clamped behind it, so that no read leaves the image whatever the index
SVO_DEV int reflect101(int i, int n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * n - 2 - i : i;
  return min(max(i, 0), n - 1);
}

// ---- cv::pyrDown: dst(x, y) = (sum k_i k_j src(r(2x + j), r(2y + i)) + 128) >> 8, k = [1 4 6 4 1].  One thread per pixel, one
// grid slice per image: slice z reads src0 + z * src_stride (jobs == nullptr) or the listed camera's image.
__global__ __launch_bounds__(256) void klt_pyr_down_kernel(const KltJob* __restrict__ jobs, const uint8_t* src0, size_t src_stride,
                                                           uint8_t* dst0, size_t dst_stride, int sw, int sh, int dw, int dh,
                                                           int from_job_l0) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= dw || y >= dh) return;
  const size_t z = jobs ? (size_t)jobs[blockIdx.z].cam : (size_t)blockIdx.z;
  const uint8_t* src = (jobs && from_job_l0) ? jobs[blockIdx.z].cur_l0 : src0 + z * src_stride;
  uint8_t* dst = dst0 + z * dst_stride;
  int cx[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) cx[j] = reflect101(2 * x + j - 2, sw);
  const int k[5] = {1, 4, 6, 4, 1};
  int acc = 0;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const uint8_t* row = src + (size_t)reflect101(2 * y + i - 2, sh) * sw;
    acc += k[i] * ((int)row[cx[0]] + 4 * (int)row[cx[1]] + 6 * (int)row[cx[2]] + 4 * (int)row[cx[3]] + (int)row[cx[4]]);
  }
  dst[(size_t)y * dw + x] = (uint8_t)((acc + 128) >> 8);
}

// the four bilinear weights of a sub-pixel offset, 14 fractional bits
struct KltW { int w00, w01, w10, w11; };
SVO_DEV KltW klt_weights(float a, float b) {
  KltW w;
  w.w00 = (int)rintf((1.f - a) * (1.f - b) * 16384.f);
  w.w01 = (int)rintf(a * (1.f - b) * 16384.f);
  w.w10 = (int)rintf((1.f - a) * b * 16384.f);
  w.w11 = 16384 - w.w00 - w.w01 - w.w10;
  return w;
}
SVO_DEV bool klt_in_range(float fx, float fy, int win, int cols, int rows) {      // on the floats: a NaN is out of range
  return fx >= (float)-win && fx < (float)cols && fy >= (float)-win && fy < (float)rows;
}
SVO_DEV float klt_div(float a, float b) { return (float)((double)a / (double)b); }    // the correctly rounded f32 quotient

// Exact sum of a per-lane integer (|v| < 2^31) over the wave, every lane gets it: the low 16 bits and the rest are summed
// apart (each sum fits 32 bits), 16 lanes by DPP, the four rows by two exchanges.
SVO_DEV int klt_wave_sum_i32(int v) {
  v = row16_sum(v);
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}
SVO_DEV long long klt_wave_sum(int v) {
  const int lo = v & 0xffff, hi = v >> 16;
  return (long long)klt_wave_sum_i32(hi) * 65536ll + (long long)klt_wave_sum_i32(lo);
}
SVO_DEV float klt_sum_f32(long long s) { return (float)(double)s * 9.5367431640625e-07f; }      // (float)sum * 2^-20

// ---- calcOpticalFlowPyrLK of one feature per wave, all levels, all listed cameras in one launch.  No barrier: a lane reads
// back only the template entries it wrote itself.
__global__ __launch_bounds__(256) void klt_track_kernel(KltDev d, KltLevels lv, const KltJob* __restrict__ jobs, KltPrm prm) {
  __shared__ short s_tpl[KLT_WAVES][3][KLT_TPL];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cam = jobs[blockIdx.y].cam;
  const int k = __builtin_amdgcn_readfirstlane(blockIdx.x * KLT_WAVES + wave);
  if (k >= d.n[cam]) return;                                                      // wave-uniform
  const size_t fi = (size_t)cam * d.max_features + k;
  const float rx = d.px_ref[2 * fi], ry = d.px_ref[2 * fi + 1];
  float cx = d.px_cur[2 * fi], cy = d.px_cur[2 * fi + 1];
  const int W = prm.win, WW = W * W;
  const float half = (float)(W - 1) * 0.5f;
  const int L = min(prm.max_level, lv.n_levels - 1);
  short* tI = s_tpl[wave][0];
  short* tX = s_tpl[wave][1];
  short* tY = s_tpl[wave][2];
  int status = 1;
  for (int level = L; level >= 0; --level) {
    const int cols = lv.w[level], rows = lv.h[level];
    const uint8_t* I = d.prev_pyr + (size_t)cam * d.pyr_bytes + lv.off[level];
    const uint8_t* J = level == 0 ? jobs[blockIdx.y].cur_l0 : d.cur_pyr + (size_t)cam * d.pyr_bytes + lv.off[level];
    const float sc = (float)(1.0 / (double)(1 << level));
    float px = rx * sc, py = ry * sc;
    float nx, ny;
    if (level == L) { nx = cx * sc; ny = cy * sc; }
    else { nx = cx * 2.f; ny = cy * 2.f; }
    cx = nx; cy = ny;
    px -= half; py -= half;
    float fx = floorf(px), fy = floorf(py);
    if (!klt_in_range(fx, fy, W, cols, rows)) {
      if (level == 0) status = 0;
      continue;
    }
    const int ipx = (int)fx, ipy = (int)fy;
    {
      // the template: I, Ix, Iy of the window; the derivatives of the four corners of a sample from its 4 x 4 neighbourhood
      const KltW w = klt_weights(px - fx, py - fy);
      int sxx = 0, sxy = 0, syy = 0;
      for (int p = lane; p < WW; p += 64) {
        const int y = p / W, x = p - y * W;
        const int gx = ipx + x, gy = ipy + y;
        int c[4], v[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) c[i] = reflect101(gx - 1 + i, cols);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint8_t* row = I + (size_t)reflect101(gy - 1 + j, rows) * cols;
#pragma unroll
          for (int i = 0; i < 4; ++i) v[j][i] = row[c[i]];
        }
        const int iv = (w.w00 * v[1][1] + w.w01 * v[1][2] + w.w10 * v[2][1] + w.w11 * v[2][2] + 256) >> 9;
        int dx[2][2], dy[2][2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          int t0[4], t1[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) { t0[i] = 3 * (v[j][i] + v[j + 2][i]) + 10 * v[j + 1][i]; t1[i] = v[j + 2][i] - v[j][i]; }
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            // outside the image a derivative is zero
            const bool in = gx + i >= 0 && gx + i < cols && gy + j >= 0 && gy + j < rows;
            dx[j][i] = in ? t0[i + 2] - t0[i] : 0;
            dy[j][i] = in ? 3 * (t1[i + 2] + t1[i]) + 10 * t1[i + 1] : 0;
          }
        }
        const int ix = (w.w00 * dx[0][0] + w.w01 * dx[0][1] + w.w10 * dx[1][0] + w.w11 * dx[1][1] + 8192) >> 14;
        const int iy = (w.w00 * dy[0][0] + w.w01 * dy[0][1] + w.w10 * dy[1][0] + w.w11 * dy[1][1] + 8192) >> 14;
        tI[p] = (short)iv; tX[p] = (short)ix; tY[p] = (short)iy;
        sxx += ix * ix; sxy += ix * iy; syy += iy * iy;
      }
      // (no lane is masked off here: the sums exchange registers across the whole wave)
      const float A11 = klt_sum_f32(klt_wave_sum(sxx)), A12 = klt_sum_f32(klt_wave_sum(sxy)), A22 = klt_sum_f32(klt_wave_sum(syy));
      float D = A11 * A22 - A12 * A12;
      const float t = A11 - A22;
      const float root = (float)sqrt((double)(t * t + 4.f * A12 * A12));
      const float min_eig = klt_div(A22 + A11 - root, (float)(2 * WW));
      if (min_eig < prm.min_eig || D < 1.1920929e-07f) {
        if (level == 0) status = 0;
        continue;
      }
      D = klt_div(1.f, D);
      nx -= half; ny -= half;
      float pdx = 0.f, pdy = 0.f;
      for (int j = 0; j < prm.max_iter; ++j) {
        fx = floorf(nx); fy = floorf(ny);
        if (!klt_in_range(fx, fy, W, cols, rows)) {
          if (level == 0) status = 0;
          break;
        }
        const int inx = (int)fx, iny = (int)fy;
        const KltW wj = klt_weights(nx - fx, ny - fy);
        int sb1 = 0, sb2 = 0;
        for (int p = lane; p < WW; p += 64) {
          const int y = p / W, x = p - y * W;
          const int c0 = reflect101(inx + x, cols), c1 = reflect101(inx + x + 1, cols);
          const uint8_t* r0 = J + (size_t)reflect101(iny + y, rows) * cols;
          const uint8_t* r1 = J + (size_t)reflect101(iny + y + 1, rows) * cols;
          const int diff = ((wj.w00 * (int)r0[c0] + wj.w01 * (int)r0[c1] + wj.w10 * (int)r1[c0] + wj.w11 * (int)r1[c1] + 256) >> 9) - (int)tI[p];
          sb1 += diff * (int)tX[p]; sb2 += diff * (int)tY[p];
        }
        const float b1 = klt_sum_f32(klt_wave_sum(sb1)), b2 = klt_sum_f32(klt_wave_sum(sb2));
        const float dlx = (A12 * b2 - A22 * b1) * D, dly = (A12 * b1 - A11 * b2) * D;
        nx += dlx; ny += dly;
        cx = nx + half; cy = ny + half;
        if ((double)dlx * (double)dlx + (double)dly * (double)dly <= prm.eps2) break;
        if (j > 0 && fabsf(dlx + pdx) < 0.01f && fabsf(dly + pdy) < 0.01f) {
          cx -= dlx * 0.5f; cy -= dly * 0.5f;
          break;
        }
        pdx = dlx; pdy = dly;
      }
    }
    if (status && level == 0) {
      const float qx = rintf(cx - half), qy = rintf(cy - half);
      if (!klt_in_range(qx, qy, W, cols, rows)) status = 0;
    }
  }
  if (lane == 0) {
    d.px_cur[2 * fi] = cx; d.px_cur[2 * fi + 1] = cy;
    d.status[fi] = (uint8_t)status;
  }
}

// ---- what follows the tracker (trackKlt :203-225, addSecondFrame :72): one workgroup per listed camera.  The survivors move
// to the front of px_ref / px_cur / f_ref / index in order (a chunk is read into registers, a barrier, then written: a target
// never lies behind its source), f_cur and the disparities are formed, and the upper median is selected on the disparities'
// bit patterns (non-negative doubles order as their bits do): the largest v with |{d < v}| <= rank, one bit a pass -- exact,
// no sorting, no floating-point atomics.
constexpr int KLT_FIN_THREADS = 256;
__global__ __launch_bounds__(KLT_FIN_THREADS) void klt_finish_kernel(KltDev d, const KltJob* __restrict__ jobs) {
  __shared__ int s_wave[KLT_FIN_THREADS / 64];
  __shared__ int s_base, s_count;
  const KltJob& job = jobs[blockIdx.x];
  const int cam = job.cam, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const size_t base = (size_t)cam * d.max_features;
  const int n_in = d.n[cam];
  if (t == 0) s_base = 0;
  __syncthreads();
  for (int k0 = 0; k0 < n_in; k0 += KLT_FIN_THREADS) {                              // block-uniform
    const int k = k0 + t;
    const bool keep = k < n_in && d.status[base + k] != 0;
    float pr[2] = {0.f, 0.f}, pc[2] = {0.f, 0.f};
    double fr[3] = {0.0, 0.0, 0.0};
    int idx = 0;
    if (keep) {
      pr[0] = d.px_ref[2 * (base + k)]; pr[1] = d.px_ref[2 * (base + k) + 1];
      pc[0] = d.px_cur[2 * (base + k)]; pc[1] = d.px_cur[2 * (base + k) + 1];
      for (int i = 0; i < 3; ++i) fr[i] = d.f_ref[3 * (base + k) + i];
      idx = d.index[base + k];
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int off = s_base;
    for (int w = 0; w < wave; ++w) off += s_wave[w];
    if (keep) {
      const size_t o = base + off + __popcll(m & ((1ull << lane) - 1ull));
      d.px_ref[2 * o] = pr[0]; d.px_ref[2 * o + 1] = pr[1];
      d.px_cur[2 * o] = pc[0]; d.px_cur[2 * o + 1] = pc[1];
      for (int i = 0; i < 3; ++i) d.f_ref[3 * o + i] = fr[i];
      d.index[o] = idx;
      double f[3];
      cam2world(job.model, (double)pc[0], (double)pc[1], f);                       // frame_cur->c2f(px_cur.x, px_cur.y)
      for (int i = 0; i < 3; ++i) d.f_cur[3 * o + i] = f[i];
      const double dx = (double)(pr[0] - pc[0]), dy = (double)(pr[1] - pc[1]);     // float differences, a double norm
      d.disparity[o] = sqrt(dx * dx + dy * dy);
    }
    __syncthreads();
    if (t == 0) s_base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
  }
  const int n = s_base;
  __syncthreads();
  // the median: rank n / 2
  unsigned long long v = 0ull;
  if (n > 0) {
    const unsigned long long* key = reinterpret_cast<const unsigned long long*>(d.disparity + base);
    const int rank = n / 2;
    for (int bit = 62; bit >= 0; --bit) {                                          // (the sign bit of a norm is clear)
      const unsigned long long cand = v | (1ull << bit);
      if (t == 0) s_count = 0;
      __syncthreads();
      int c = 0;
      for (int j = t; j < n; j += KLT_FIN_THREADS) c += key[j] < cand ? 1 : 0;
      c = group_sum<64>(c);
      if (lane == 0 && c) atomicAdd(&s_count, c);
      __syncthreads();
      if (s_count <= rank) v = cand;
      __syncthreads();
    }
  }
  if (t == 0) {
    d.n[cam] = n;
    KltResultBlock* r = reinterpret_cast<KltResultBlock*>(job.result);
    r->n_in = n_in; r->n_tracked = n;
    r->median = n > 0 ? __longlong_as_double((long long)v) : __longlong_as_double(0x7ff8000000000000ll);
    __threadfence_system();
    __hip_atomic_store(&r->seq, job.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// addFirstFrame with the detector's features (detectFeatures, S/initialization.cpp:154-174): cv::Point2f(ftr->px[0], ftr->px[1])
// and ftr->f of the n features the detection left in device memory
__global__ __launch_bounds__(256) void klt_take_detection_kernel(KltDev d, int cam, const int32_t* __restrict__ n_det, const double* __restrict__ px,
                                                                 const double* __restrict__ f, int32_t* __restrict__ n_host) {
  const int n = min(*n_det, d.max_features);
  const size_t base = (size_t)cam * d.max_features;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const float x = (float)px[2 * i], y = (float)px[2 * i + 1];
    d.px_ref[2 * (base + i)] = x; d.px_ref[2 * (base + i) + 1] = y;
    d.px_cur[2 * (base + i)] = x; d.px_cur[2 * (base + i) + 1] = y;
    for (int j = 0; j < 3; ++j) d.f_ref[3 * (base + i) + j] = f[3 * i + j];
    d.index[base + i] = i;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { d.n[cam] = n; *n_host = *n_det; }
}
}  // namespace svo_klt
