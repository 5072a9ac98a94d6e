// The host twin of the two-view kernels: the arithmetic of android_svo_amd/csrc/svo_two_view_math.h (the functions the kernels
// call) run serially on the CPU in the order the kernels decide things.  tests/test_two_view_twin_cpu.py feeds it the families
// of tests/test_two_view_model_cpu.py and requires the model's numbers bit for bit.  Build with -ffp-contract=off.
//
//   two_view_twin <case.bin> <result.bin> [...]     one pair per case; prints the single-core time of each
//
// case.bin:   int32 n, width, height, n_hypotheses, min_inliers, pad; uint64 seed; f64 error_multiplier2, reproj_thresh,
//             map_scale, T_ref_w[7]; f64 f_ref[n][3], f_cur[n][3]; f32 px_ref[n][2], px_cur[n][2]
// result.bin: int32 status, n_in, hypothesis, hypothesis_count, candidate, candidate_count, n_inliers, n_points;
//             f64 depth_median, scale, T_cur_from_ref[7], T_cur_w[7]; int32 counts[n_hypotheses] (status != TOO_FEW);
//             uint8 mask[n]; int32 inliers[n_inliers]; f64 xyz[n][3] (status OK or FEW_INLIERS); int32 point_index[n_points];
//             f64 point_pos[n_points][3]
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../android_svo_amd/csrc/svo_two_view_math.h"

using namespace svo_tv;

namespace {
struct Case {
  int32_t n, width, height, n_hypotheses, min_inliers, pad;
  uint64_t seed;
  double em2, reproj_thresh, map_scale, T_ref_w[7];
  std::vector<double> f_ref, f_cur;
  std::vector<float> px_ref, px_cur;
};
struct Result {
  int32_t status = TV_OK, n_in = 0, hypothesis = -1, hypothesis_count = -1, candidate = -1, candidate_count = 0, n_inliers = 0, n_points = 0;
  double depth_median, scale, T_cur_from_ref[7], T_cur_w[7];
  std::vector<int32_t> counts, inliers, point_index;
  std::vector<uint8_t> mask;
  std::vector<double> xyz, point_pos;
  bool have_xyz = false;
};

bool read_case(const char* path, Case& c) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  bool ok = fread(&c.n, 4, 6, f) == 6 && fread(&c.seed, 8, 1, f) == 1 && fread(&c.em2, 8, 10, f) == 10;
  if (ok && c.n >= 0 && c.n <= (1 << 20)) {
    const size_t n = (size_t)c.n;
    c.f_ref.resize(3 * n); c.f_cur.resize(3 * n); c.px_ref.resize(2 * n); c.px_cur.resize(2 * n);
    ok = fread(c.f_ref.data(), 8, 3 * n, f) == 3 * n && fread(c.f_cur.data(), 8, 3 * n, f) == 3 * n &&
         fread(c.px_ref.data(), 4, 2 * n, f) == 2 * n && fread(c.px_cur.data(), 4, 2 * n, f) == 2 * n;
  } else {
    ok = false;
  }
  fclose(f);
  return ok && c.n_hypotheses >= 1 && c.n_hypotheses <= TV_MAX_HYPOTHESES;
}

void load_xy(const Case& c, int i, float* xy) {
  tv_normalised(&c.f_ref[3 * (size_t)i], xy);
  tv_normalised(&c.f_cur[3 * (size_t)i], xy + 2);
}

bool hypothesis(const Case& c, int h, double* F) {
  int s[8];
  float p[8][4];
  double A[72];
  tv_sample(c.seed, h, c.n, s);
  for (int i = 0; i < 8; ++i) load_xy(c, s[i], p[i]);
  return tv_hypothesis<1>(p, A, F);
}

void run(const Case& c, Result& r) {
  const double nan = __builtin_nan("");
  const int n = c.n;
  r.n_in = n;
  r.depth_median = r.scale = nan;
  for (int i = 0; i < 7; ++i) r.T_cur_from_ref[i] = r.T_cur_w[i] = nan;
  r.mask.assign((size_t)n, 0);
  if (n < 8) { r.status = TV_TOO_FEW; return; }
  std::vector<float> xy(4 * (size_t)n);
  for (int j = 0; j < n; ++j) load_xy(c, j, &xy[4 * (size_t)j]);
  const double thr2 = tv_thr2(c.reproj_thresh, c.em2);
  // the hypothesis kernel
  r.counts.assign((size_t)c.n_hypotheses, -1);
  for (int h = 0; h < c.n_hypotheses; ++h) {
    double F[9];
    if (!hypothesis(c, h, F)) continue;
    int count = 0;
    for (int j = 0; j < n; ++j) count += tv_epi_inlier(F, xy[4 * j], xy[4 * j + 1], xy[4 * j + 2], xy[4 * j + 3], thr2) ? 1 : 0;
    r.counts[h] = count;
  }
  // the finish kernel
  int best = -1;
  for (int h = 0; h < c.n_hypotheses; ++h)
    if (r.counts[h] > (best < 0 ? -1 : r.counts[best])) best = h;
  if (best < 0) { r.status = TV_NO_MODEL; return; }
  r.hypothesis = best; r.hypothesis_count = r.counts[best];
  double F[9], w[9], v[9], R1[9], R2[9], u3[3], R[4][9], t[4][3];
  hypothesis(c, best, F);
  tv_decompose(F, w, v, R1, R2, u3);
  int cc[4] = {0, 0, 0, 0};
  for (int k = 0; k < 4; ++k) tv_candidate(k, R1, R2, u3, R[k], t[k]);
  for (int j = 0; j < n; ++j) {
    const bool in = tv_epi_inlier(F, xy[4 * j], xy[4 * j + 1], xy[4 * j + 2], xy[4 * j + 3], thr2);
    r.mask[j] = in ? 1 : 0;
    if (!in) continue;
    for (int k = 0; k < 4; ++k) {
      double lambda[2], xyz[3];
      tv_triangulate(R[k], t[k], &c.f_cur[3 * (size_t)j], &c.f_ref[3 * (size_t)j], lambda, xyz);
      cc[k] += (lambda[0] > 0.0 && lambda[1] > 0.0) ? 1 : 0;
    }
  }
  int cand = 0;
  for (int k = 1; k < 4; ++k) cand = cc[k] > cc[cand] ? k : cand;
  r.candidate = cand; r.candidate_count = cc[cand];
  if ((double)cc[cand] < (double)n * 0.5) { r.status = TV_CHEIRALITY; return; }
  r.xyz.resize(3 * (size_t)n);
  r.have_xyz = true;
  std::vector<int32_t> inliers;
  bool any_nan = false;
  for (int j = 0; j < n; ++j) {
    double* xyz = &r.xyz[3 * (size_t)j];
    if (tv_compute_inlier(R[cand], t[cand], &c.f_cur[3 * (size_t)j], &c.f_ref[3 * (size_t)j], c.reproj_thresh, c.em2, xyz)) inliers.push_back(j);
    any_nan = any_nan || xyz[2] != xyz[2];
  }
  for (int i = 0; i < 3; ++i) r.T_cur_from_ref[i] = t[cand][i];
  tv_quaternion(R[cand], r.T_cur_from_ref + 3);
  if (!any_nan) {
    std::vector<unsigned long long> keys((size_t)n);
    for (int j = 0; j < n; ++j) keys[j] = tv_depth_key(r.xyz[3 * (size_t)j + 2]);
    std::nth_element(keys.begin(), keys.begin() + n / 2, keys.end());
    r.depth_median = tv_depth_from_key(keys[n / 2]);
  }
  if ((int)inliers.size() < c.min_inliers) { r.status = TV_FEW_INLIERS; return; }
  r.inliers = inliers; r.n_inliers = (int32_t)inliers.size();
  r.scale = c.map_scale / r.depth_median;
  double Twc[7];
  tv_second_pose(r.T_cur_from_ref, c.T_ref_w, r.scale, r.T_cur_w, Twc);
  for (int j : inliers) {
    double xyz[3], pos[3];
    for (int i = 0; i < 3; ++i) xyz[i] = r.xyz[3 * (size_t)j + i];
    if (!(tv_in_frame(c.px_cur[2 * j], c.px_cur[2 * j + 1], c.width, c.height) && tv_in_frame(c.px_ref[2 * j], c.px_ref[2 * j + 1], c.width, c.height) &&
          xyz[2] > 0.0))
      continue;
    for (int i = 0; i < 3; ++i) xyz[i] = xyz[i] * r.scale;
    tv_se3_act(Twc, xyz, pos);
    r.point_index.push_back(j);
    r.point_pos.insert(r.point_pos.end(), pos, pos + 3);
  }
  r.n_points = (int32_t)r.point_index.size();
}

bool write_result(const char* path, const Result& r) {
  FILE* f = fopen(path, "wb");
  if (!f) return false;
  fwrite(&r.status, 4, 8, f);
  fwrite(&r.depth_median, 8, 16, f);
  if (!r.counts.empty()) fwrite(r.counts.data(), 4, r.counts.size(), f);
  if (!r.mask.empty()) fwrite(r.mask.data(), 1, r.mask.size(), f);
  if (!r.inliers.empty()) fwrite(r.inliers.data(), 4, r.inliers.size(), f);
  if (r.have_xyz) fwrite(r.xyz.data(), 8, r.xyz.size(), f);
  if (!r.point_index.empty()) fwrite(r.point_index.data(), 4, r.point_index.size(), f);
  if (!r.point_pos.empty()) fwrite(r.point_pos.data(), 8, r.point_pos.size(), f);
  return fclose(f) == 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3 || (argc - 1) % 2 != 0) {
    fprintf(stderr, "usage: two_view_twin <case.bin> <result.bin> [...]\n");
    return 2;
  }
  for (int a = 1; a + 1 < argc; a += 2) {
    Case c;
    if (!read_case(argv[a], c)) { fprintf(stderr, "cannot read %s\n", argv[a]); return 1; }
    Result r;
    const auto t0 = std::chrono::steady_clock::now();
    run(c, r);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (!write_result(argv[a + 1], r)) { fprintf(stderr, "cannot write %s\n", argv[a + 1]); return 1; }
    printf("%s: n %d hypotheses %d status %d time_ms %.3f\n", argv[a], c.n, c.n_hypotheses, r.status, ms);
  }
  printf("two view twin OK\n");
  return 0;
}
