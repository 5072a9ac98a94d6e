// svo_klt_types.h -- the bootstrap's handle and the structures its kernels share (svo_klt.hip / svo_klt_device.h: the KLT
// tracker; svo_two_view_impl.h / svo_two_view_device.h: the two-view stage on the same device-resident lists).
#pragma once
#include <vector>

#include "svo_internal.h"

namespace svo_klt {
using namespace svo_dev;

constexpr int KLT_MAX_WIN = 30;                       // the template of a wave: 3 x 900 int16 in LDS
constexpr int KLT_TPL = 15 * 64;                      // 900 rounded up to whole waves
constexpr int KLT_WAVES = 4;                          // features per 256-thread block

// the Gaussian pyramid of one image: level l is w[l] x h[l] bytes at off[l] (level 0 of the current image is read where the
// caller's svo_hip_pyramid holds it)
struct KltLevels {
  int n_levels;
  int w[SVO_HIP_MAX_LEVELS], h[SVO_HIP_MAX_LEVELS];
  unsigned off[SVO_HIP_MAX_LEVELS];
};

// one listed camera of a call
struct KltJob {
  int cam, pad;
  const uint8_t* cur_l0;                              // level 0 of the current image
  char* result;                                       // the camera's page-locked result block (device address)
  unsigned long long seq;
  Cam model;
};

// the handle's device arrays, [camera][max_features] each
struct KltDev {
  float *px_ref, *px_cur;                             // x 2
  double *f_ref, *f_cur;                              // x 3
  double* disparity;
  int32_t* index;
  uint8_t* status;
  int32_t* n;                                         // [camera]
  uint8_t *prev_pyr, *cur_pyr;                        // [camera][pyr_bytes]
  size_t pyr_bytes;
  int max_features;
};

struct KltPrm {
  int win, max_level, max_iter;
  double eps2;
  float min_eig;
};

// the result block of a camera in page-locked memory
struct KltResultBlock {
  unsigned long long seq;
  int n_in, n_tracked;
  double median;
};
}  // namespace svo_klt

// the handle (svo_klt.hip, svo_two_view_impl.h)
void svo_tv_release(struct svo_hip_klt* k);
struct svo_hip_klt {
  svo_hip_ctx* ctx = nullptr;
  int width = 0, height = 0, n_cameras = 0, max_features = 0;
  svo_hip_klt_params prm;
  svo_klt::KltLevels lv;
  svo_klt::KltDev dev;
  char* dev_block = nullptr;
  svo_klt::KltJob* jobs_dev = nullptr;
  char* host_block = nullptr;             // page-locked: [jobs][result blocks][detection count]
  svo_klt::KltJob* jobs_host = nullptr;
  svo_klt::KltResultBlock* res_host = nullptr;
  svo_klt::KltResultBlock* res_host_dev = nullptr;
  int32_t* det_n_host = nullptr;
  int32_t* det_n_host_dev = nullptr;
  std::vector<int> n_host;                // features a camera holds
  std::vector<char> has_ref;
  unsigned long long seq = 0;
  std::vector<char> has_cur;              // f_cur is defined: a track or a set_lists since the reference was set
  struct svo_tv_state* tv = nullptr;      // the two-view stage's memory (svo_two_view_impl.h), taken by its first call
};
