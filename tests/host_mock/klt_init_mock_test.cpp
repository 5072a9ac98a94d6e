// CPU-only test of hip_bridge::KltInitT (include/svo_dropin/klt_init_hip.h) against a MOCK of the svo_hip_klt_* entry points that
// records every call and drops the features it is told to drop.  Checked: the call sequences (addFirstFrame below the gate
// sends nothing; one svo_hip_klt_track per trackSecondFrames, whatever the number of cameras); FAILURE / NO_KEYFRAME / SUCCESS
// exactly at the gates' boundaries (n_tracked == min_tracked passes, median == min_disparity passes); px_ref_ / px_cur_ /
// f_ref_ / f_cur_ / disparities_ / index_ after erasures over several frames; a camera without a reference and a refused
// device call leave every list as it was.  Built and run by tests/test_host_klt_mock.py, plain and with
// -fsanitize=address,undefined.  C++11, the reference's language level.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

#include "svo_hip.h"
#include "svo_dropin/klt_init_hip.h"

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

// ---------------------------------------------------------------- mock device
struct svo_hip_ctx { int unused; };
struct svo_hip_pyramid { int unused; };
struct MockCam {
  bool has_ref;
  std::vector<float> px_ref, px_cur;
  std::vector<double> f_ref, f_cur, disp;
  std::vector<int32_t> index;
  MockCam() : has_ref(false) {}
};
struct svo_hip_klt { std::vector<MockCam> cams; int max_features; };
static std::vector<std::string> g_calls;
static std::set<int> g_drop;             // original indices the next track loses
static float g_move = 0.f;               // px_cur.x of every survivor moves by this much in the next track
static bool g_refuse = false;
static int g_detect_n = 0;

extern "C" {
int svo_hip_klt_create(svo_hip_ctx*, int, int, int n_cameras, int max_features, const svo_hip_klt_params*, svo_hip_klt** out) {
  g_calls.push_back("create");
  *out = new svo_hip_klt();
  (*out)->cams.resize((size_t)n_cameras);
  (*out)->max_features = max_features;
  return SVO_HIP_OK;
}
int svo_hip_klt_destroy(svo_hip_klt* k) { g_calls.push_back("destroy"); delete k; return SVO_HIP_OK; }
int svo_hip_klt_set_reference(svo_hip_klt* k, int camera, const svo_hip_pyramid* pyr, int, int n, const float* px, const double* f) {
  g_calls.push_back("set_reference");
  if (g_refuse || !pyr || camera < 0 || camera >= (int)k->cams.size() || n > k->max_features) return SVO_HIP_ERR_INVALID;
  MockCam& c = k->cams[(size_t)camera];
  c.px_ref.assign(px, px + 2 * n); c.px_cur = c.px_ref; c.f_ref.assign(f, f + 3 * n);
  c.index.resize((size_t)n);
  for (int i = 0; i < n; ++i) c.index[(size_t)i] = i;
  c.f_cur.clear(); c.disp.clear();
  c.has_ref = true;
  return SVO_HIP_OK;
}
int svo_hip_klt_set_reference_detected(svo_hip_klt* k, int camera, const svo_hip_pyramid* pyr, int slot, const svo_hip_camera* cam, int, int, double,
                                       int32_t* n) {
  g_calls.push_back("set_reference_detected");
  if (g_refuse || !cam) return SVO_HIP_ERR_INVALID;
  std::vector<float> px;
  std::vector<double> f;
  for (int i = 0; i < g_detect_n; ++i) { px.push_back(10.f + i); px.push_back(20.f + 2 * i); f.push_back(0.1 * i); f.push_back(0.2); f.push_back(0.9); }
  g_calls.pop_back();
  const int rc = svo_hip_klt_set_reference(k, camera, pyr, slot, g_detect_n, px.data(), f.data());
  g_calls.back() = "set_reference_detected";
  *n = g_detect_n;
  return rc;
}
int svo_hip_klt_track(svo_hip_klt* k, int n, const int* cameras, const svo_hip_pyramid* cur, const int*, const svo_hip_camera* cams, svo_hip_klt_result* res) {
  g_calls.push_back("track");
  if (g_refuse || !cur || !cams) return SVO_HIP_ERR_INVALID;
  for (int i = 0; i < n; ++i)
    if (!k->cams[(size_t)cameras[i]].has_ref) return SVO_HIP_ERR_STATE;
  for (int i = 0; i < n; ++i) {
    MockCam& c = k->cams[(size_t)cameras[i]];
    MockCam o;
    o.has_ref = true;
    res[i].n_in = (int)c.index.size();
    for (size_t j = 0; j < c.index.size(); ++j) {
      if (g_drop.count(c.index[j])) continue;
      o.index.push_back(c.index[j]);
      o.px_ref.push_back(c.px_ref[2 * j]); o.px_ref.push_back(c.px_ref[2 * j + 1]);
      o.px_cur.push_back(c.px_cur[2 * j] + g_move); o.px_cur.push_back(c.px_cur[2 * j + 1]);
      for (int d = 0; d < 3; ++d) { o.f_ref.push_back(c.f_ref[3 * j + d]); o.f_cur.push_back(1000.0 * cameras[i] + c.index[j] + 0.25 * d); }
      const double dx = (double)(o.px_ref[o.px_ref.size() - 2] - o.px_cur[o.px_cur.size() - 2]);
      o.disp.push_back(std::sqrt(dx * dx));
    }
    c = o;
    res[i].n_tracked = (int)c.index.size(); res[i].n_levels = 4;
    std::vector<double> s(c.disp);
    for (size_t a = 0; a < s.size(); ++a) for (size_t b = a + 1; b < s.size(); ++b) if (s[b] < s[a]) std::swap(s[a], s[b]);
    res[i].disparity_median = s.empty() ? std::nan("") : s[s.size() / 2];
  }
  return SVO_HIP_OK;
}
int svo_hip_klt_download(svo_hip_klt* k, int camera, int32_t* n, float* px_ref, float* px_cur, double* f_ref, double* f_cur, double* disp, int32_t* index) {
  g_calls.push_back("download");
  const MockCam& c = k->cams[(size_t)camera];
  if (!c.has_ref) return SVO_HIP_ERR_STATE;
  *n = (int32_t)c.index.size();
  for (size_t i = 0; i < c.px_ref.size(); ++i) { px_ref[i] = c.px_ref[i]; px_cur[i] = c.px_cur[i]; }
  for (size_t i = 0; i < c.f_ref.size(); ++i) f_ref[i] = c.f_ref[i];
  if (f_cur) for (size_t i = 0; i < c.f_cur.size(); ++i) f_cur[i] = c.f_cur[i];
  if (disp) for (size_t i = 0; i < c.disp.size(); ++i) disp[i] = c.disp[i];
  for (size_t i = 0; i < c.index.size(); ++i) index[i] = c.index[i];
  return SVO_HIP_OK;
}
}  // extern "C"

// ---------------------------------------------------------------- the host's types
struct Point2f { float x, y; Point2f() : x(0), y(0) {} Point2f(float a, float b) : x(a), y(b) {} };
struct Vector3d { double v[3]; Vector3d() { v[0] = v[1] = v[2] = 0; } double& operator[](int i) { return v[i]; } const double& operator[](int i) const { return v[i]; } };
struct Types { typedef ::Point2f Point2f; typedef ::Vector3d Vector3d; };
namespace hip_bridge = svo::hip_bridge;
typedef hip_bridge::KltInitT<Types> KltInit;
using hip_bridge::KLT_FAILURE;
using hip_bridge::KLT_NO_KEYFRAME;
using hip_bridge::KLT_SUCCESS;

static void features(int n, std::vector<Point2f>& px, std::vector<Vector3d>& f) {
  px.clear(); f.clear();
  for (int i = 0; i < n; ++i) {
    px.push_back(Point2f(5.f + i, 7.f + 0.5f * i));
    Vector3d v; v[0] = 0.01 * i; v[1] = -0.02 * i; v[2] = 1.0;
    f.push_back(v);
  }
}
static size_t count(const std::string& what) {
  size_t n = 0;
  for (size_t i = 0; i < g_calls.size(); ++i) n += g_calls[i] == what;
  return n;
}

int main() {
  svo_hip_ctx ctx;
  svo_hip_pyramid pyr;
  svo_hip_camera cam = svo_hip_camera();
  hip_bridge::KltInitGates gates;
  gates.min_features = 100; gates.min_tracked = 50; gates.min_disparity = 4.0;
  std::vector<Point2f> px;
  std::vector<Vector3d> f;
  {
    KltInit init(&ctx, 640, 480, 3, 256, gates);
    CHECK(init.ok() && init.cameras() == 3 && count("create") == 1);
    // ---- the first frame's gate: 99 features fail and nothing is sent, 100 pass
    features(99, px, f);
    CHECK(init.addFirstFrame(0, &pyr, 0, px, f) == KLT_FAILURE && count("set_reference") == 0 && !init.lists(0).has_ref_);
    CHECK(init.trackSecondFrame(0, &pyr, 1, cam) == KLT_FAILURE && count("track") == 0);          // no reference: nothing is sent
    features(100, px, f);
    CHECK(init.addFirstFrame(0, &pyr, 0, px, f) == KLT_SUCCESS && count("set_reference") == 1);
    {
      const KltInit::Lists& l = init.lists(0);
      CHECK(l.has_ref_ && l.px_ref_.size() == 100 && l.px_cur_.size() == 100 && l.f_ref_.size() == 100 && l.f_cur_.empty() && l.disparities_.empty());
      CHECK(l.px_cur_[37].x == px[37].x && l.px_cur_[37].y == px[37].y && l.index_[99] == 99);
    }
    CHECK(init.addFirstFrame(3, &pyr, 0, px, f) == KLT_FAILURE && init.addFirstFrame(-1, &pyr, 0, px, f) == KLT_FAILURE);
    // ---- frame 2: features 3, 50 and 99 are lost, the rest moves by 2 px: below the disparity gate
    g_drop.clear(); g_drop.insert(3); g_drop.insert(50); g_drop.insert(99);
    g_move = 2.f;
    CHECK(init.trackSecondFrame(0, &pyr, 1, cam) == KLT_NO_KEYFRAME && count("track") == 1);
    {
      const KltInit::Lists& l = init.lists(0);
      CHECK(l.px_ref_.size() == 97 && l.px_cur_.size() == 97 && l.f_ref_.size() == 97 && l.f_cur_.size() == 97 && l.disparities_.size() == 97);
      CHECK(l.index_[2] == 2 && l.index_[3] == 4 && l.index_[48] == 49 && l.index_[49] == 51 && l.index_[96] == 98);
      CHECK(l.px_ref_[3].x == px[4].x && l.px_cur_[3].x == px[4].x + 2.f && l.px_cur_[3].y == px[4].y);
      CHECK(l.f_ref_[49][1] == f[51][1] && l.f_cur_[49][2] == 51 + 0.5 && l.disparities_[10] == 2.0 && l.disparity_median_ == 2.0);
    }
    // ---- frame 3: the flow is carried (another 2 px: 4 px in all), the median sits exactly on the gate -> on to computeFundamental
    g_drop.clear(); g_drop.insert(0);
    CHECK(init.trackSecondFrame(0, &pyr, 2, cam) == KLT_SUCCESS);
    CHECK(init.lists(0).px_ref_.size() == 96 && init.lists(0).index_[0] == 1 && init.lists(0).disparity_median_ == 4.0);
    CHECK(init.lists(0).px_cur_[0].x == px[1].x + 4.f);
    // ---- the survivor gate: exactly min_tracked passes, one fewer fails
    g_drop.clear();
    for (int i = 1; i <= 47; ++i) g_drop.insert(i == 3 ? 0 : i);                                  // 96 - 46 = 50 left (0, 3, 50 are gone already)
    g_move = 0.f;
    CHECK(init.trackSecondFrame(0, &pyr, 1, cam) == KLT_SUCCESS && init.lists(0).disparities_.size() == 50);
    g_drop.clear(); g_drop.insert(98);
    CHECK(init.trackSecondFrame(0, &pyr, 1, cam) == KLT_FAILURE && init.lists(0).disparities_.size() == 49 && init.lists(0).px_ref_.size() == 49);
    // ---- a refused device call: false / FAILURE, the lists as they were
    g_refuse = true;
    CHECK(init.trackSecondFrame(0, &pyr, 1, cam) == KLT_FAILURE && init.lists(0).px_ref_.size() == 49 && init.lists(0).index_.back() == 97);
    features(120, px, f);
    CHECK(init.addFirstFrame(1, &pyr, 0, px, f) == KLT_FAILURE && !init.lists(1).has_ref_);
    g_refuse = false;
    // ---- three cameras, one device call; the detected form for one of them
    g_detect_n = 99;
    CHECK(init.addFirstFrameDetected(2, &pyr, 0, cam, 3, 20, 10.0) == KLT_FAILURE && !init.lists(2).has_ref_ && init.lists(2).px_ref_.empty());
    g_detect_n = 130;
    CHECK(init.addFirstFrameDetected(2, &pyr, 0, cam, 3, 20, 10.0) == KLT_SUCCESS && init.lists(2).px_ref_.size() == 130);
    CHECK(init.lists(2).px_cur_[7].y == 34.f && init.lists(2).f_ref_[7][0] == 0.1 * 7 && init.lists(2).f_cur_.empty() && init.lists(2).index_[129] == 129);
    CHECK(init.addFirstFrame(1, &pyr, 0, px, f) == KLT_SUCCESS);
    features(100, px, f);
    CHECK(init.addFirstFrame(0, &pyr, 0, px, f) == KLT_SUCCESS && init.lists(0).f_cur_.empty());  // a new first frame resets the camera
    const size_t tracks = count("track");
    g_drop.clear(); g_drop.insert(5);
    g_move = 9.f;
    const int cams_listed[3] = {2, 0, 1}, slots[3] = {1, 2, 3};
    const svo_hip_camera models[3] = {cam, cam, cam};
    hip_bridge::KltInitResult res[3];
    CHECK(init.trackSecondFrames(3, cams_listed, &pyr, slots, models, res) && count("track") == tracks + 1);
    CHECK(res[0] == KLT_SUCCESS && res[1] == KLT_SUCCESS && res[2] == KLT_SUCCESS);
    CHECK(init.lists(2).px_ref_.size() == 129 && init.lists(0).px_ref_.size() == 99 && init.lists(1).px_ref_.size() == 119);
    CHECK(init.lists(2).f_cur_[5][0] == 2000.0 + 6 && init.lists(1).f_cur_[4][0] == 1000.0 + 4);
    // a listed camera without a reference: nothing is sent, nothing changes
    init.reset(1);
    CHECK(!init.trackSecondFrames(3, cams_listed, &pyr, slots, models, res) && count("track") == tracks + 1 && init.lists(2).px_ref_.size() == 129);
  }
  CHECK(count("destroy") == 1);
  std::printf("klt init mock test OK\n");
  return 0;
}
