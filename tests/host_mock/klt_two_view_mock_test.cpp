// CPU-only test of hip_bridge::KltInitT::computeTwoViews / computeTwoView (include/svo_dropin/klt_init_hip.h) against a MOCK of its
// own of the svo_hip_klt_* entry points.  Checked: the call sequences (one svo_hip_klt_two_view per computeTwoViews whatever the
// number of cameras, one download per camera that passed the cheirality gate, nothing sent for a camera without tracked
// lists); SUCCESS only for status OK, FAILURE for every other status with no inliers and no points held; inliers_,
// xyz_in_cur_, T_cur_from_ref_, T_cur_w_ and the point list as the device returned them; a new track forgets the result; a
// refused call leaves lists and results as they were.  Then the C++ twin (android_svo_amd/host/svo_host.h):
// svo::initialization::KltInit::setLists / addSecondFrame on the twin types -- the second frame's pose, one Point per entry of the
// point list in its order, its Feature in the current frame created first and in the reference frame second, Point::obs_
// reading [ref, cur], level 0 -- and flattenMap's tables of that map; a failure changes neither frame.  Built and run by
// tests/test_host_two_view_mock.py, plain and with -fsanitize=address,undefined.  C++17, the host layer's language level.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "svo_hip.h"
#include "svo_dropin/klt_init_hip.h"
#include "../../android_svo_amd/host/svo_host.h"

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

// ---------------------------------------------------------------- mock device
struct svo_hip_ctx { int unused; };
struct svo_hip_pyramid { int unused; };
static int g_set_lists_n = -1;
struct MockCam {
  bool has_ref, has_cur, has_result;
  int n;
  svo_hip_two_view_result res;
  MockCam() : has_ref(false), has_cur(false), has_result(false), n(0), res() {}
};
struct svo_hip_klt { std::vector<MockCam> cams; };
static std::vector<std::string> g_calls;
static std::vector<int> g_status;        // the status the next two-view call gives its i-th listed camera
static bool g_refuse = false;
static int g_last_n = 0;
static const double* g_last_T = NULL;

extern "C" {
int svo_hip_klt_create(svo_hip_ctx*, int, int, int n_cameras, int, const svo_hip_klt_params*, svo_hip_klt** out) {
  *out = new svo_hip_klt();
  (*out)->cams.resize((size_t)n_cameras);
  return SVO_HIP_OK;
}
int svo_hip_klt_destroy(svo_hip_klt* k) { delete k; return SVO_HIP_OK; }
int svo_hip_klt_set_reference(svo_hip_klt* k, int camera, const svo_hip_pyramid*, int, int n, const float*, const double*) {
  g_calls.push_back("set_reference");
  MockCam& c = k->cams[(size_t)camera];
  c = MockCam(); c.has_ref = true; c.n = n;
  return SVO_HIP_OK;
}
int svo_hip_klt_track(svo_hip_klt* k, int n, const int* cameras, const svo_hip_pyramid*, const int*, const svo_hip_camera*, svo_hip_klt_result* res) {
  g_calls.push_back("track");
  for (int i = 0; i < n; ++i) {
    MockCam& c = k->cams[(size_t)cameras[i]];
    c.has_cur = true; c.has_result = false;
    res[i].n_in = c.n; res[i].n_tracked = c.n; res[i].n_levels = 4; res[i].disparity_median = 60.0;
  }
  return SVO_HIP_OK;
}
int svo_hip_klt_download(svo_hip_klt* k, int camera, int32_t* n, float* px_ref, float* px_cur, double* f_ref, double* f_cur, double* disp, int32_t* index) {
  g_calls.push_back("download");
  const MockCam& c = k->cams[(size_t)camera];
  *n = c.n;
  for (int i = 0; i < c.n; ++i) {
    px_ref[2 * i] = 20.f + i; px_ref[2 * i + 1] = 30.f; px_cur[2 * i] = 80.f + i; px_cur[2 * i + 1] = 30.f;
    for (int j = 0; j < 3; ++j) { f_ref[3 * i + j] = 0.1 * j; if (f_cur) f_cur[3 * i + j] = 0.2 * j; }
    if (disp) disp[i] = 60.0;
    index[i] = i;
  }
  return SVO_HIP_OK;
}
int svo_hip_klt_set_lists(svo_hip_klt* k, int camera, int n, const float*, const float*, const double*, const double*) {
  g_calls.push_back("set_lists");
  MockCam& c = k->cams[(size_t)camera];
  if (g_refuse || !c.has_ref) return SVO_HIP_ERR_STATE;
  c.n = n; c.has_cur = true; c.has_result = false;
  g_set_lists_n = n;
  return SVO_HIP_OK;
}
int svo_hip_klt_two_view(svo_hip_klt* k, int n, const int* cameras, const svo_hip_camera* cams, const double* T_ref_w, const svo_hip_two_view_params*,
                         svo_hip_two_view_result* results) {
  g_calls.push_back("two_view");
  g_last_n = n; g_last_T = T_ref_w;
  if (g_refuse || !cams) return SVO_HIP_ERR_INVALID;
  for (int i = 0; i < n; ++i)
    if (!k->cams[(size_t)cameras[i]].has_cur) return SVO_HIP_ERR_STATE;
  for (int i = 0; i < n; ++i) {
    MockCam& c = k->cams[(size_t)cameras[i]];
    svo_hip_two_view_result r = svo_hip_two_view_result();
    r.status = g_status[(size_t)i]; r.n_in = c.n;
    const bool ok = r.status == SVO_HIP_TWO_VIEW_OK;
    r.n_inliers = ok ? c.n - 2 : 0;                      // every correspondence but the first two
    r.n_points = ok ? c.n - 3 : 0;                       // ... and the last inlier fails the gate of :123
    r.depth_median = 4.0 + cameras[i]; r.scale = ok ? 1.0 / r.depth_median : std::nan("");
    for (int j = 0; j < 7; ++j) { r.T_cur_from_ref[j] = 10.0 * cameras[i] + j; r.T_cur_w[j] = ok ? 100.0 * cameras[i] + j : std::nan(""); }
    c.res = r; c.has_result = true;
    results[i] = r;
  }
  return SVO_HIP_OK;
}
int svo_hip_klt_download_two_view(svo_hip_klt* k, int camera, int32_t*, int32_t* n, double* xyz, uint8_t*, int32_t* n_inliers, int32_t* inliers, int32_t* n_points,
                                  int32_t* point_index, double* point_pos, int32_t*, int32_t*) {
  g_calls.push_back("download_two_view");
  const MockCam& c = k->cams[(size_t)camera];
  if (!c.has_result) return SVO_HIP_ERR_STATE;
  *n = c.n; *n_inliers = c.res.n_inliers; *n_points = c.res.n_points;
  for (int i = 0; i < 3 * c.n; ++i) xyz[i] = 1000.0 * camera + i;
  for (int i = 0; i < c.res.n_inliers; ++i) inliers[i] = i + 2;
  for (int i = 0; i < c.res.n_points; ++i) { point_index[i] = i + 2; for (int j = 0; j < 3; ++j) point_pos[3 * i + j] = -1000.0 * camera - (3 * i + j); }
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
using hip_bridge::KLT_SUCCESS;

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
  gates.min_features = 10; gates.min_tracked = 5; gates.min_disparity = 4.0;
  KltInit init(&ctx, 640, 480, 4, 64, gates);
  CHECK(init.ok());
  std::vector<Point2f> px;
  std::vector<Vector3d> f;
  for (int i = 0; i < 12; ++i) { px.push_back(Point2f(20.f + i, 30.f)); f.push_back(Vector3d()); }
  const int cams3[3] = {2, 0, 3};
  const int slots[3] = {0, 0, 0};
  const svo_hip_camera cm[3] = {cam, cam, cam};
  hip_bridge::KltInitResult r[3];
  for (int i = 0; i < 3; ++i) CHECK(init.addFirstFrame(cams3[i], &pyr, 0, px, f) == KLT_SUCCESS);
  // ---- no tracked lists yet: nothing is sent
  CHECK(!init.computeTwoViews(3, cams3, cm, NULL, NULL, r) && count("two_view") == 0);
  CHECK(init.computeTwoView(1, cam) == KLT_FAILURE && count("two_view") == 0);                      // no reference at all
  CHECK(init.trackSecondFrames(3, cams3, &pyr, slots, cm, r) && r[0] == KLT_SUCCESS && r[2] == KLT_SUCCESS);
  CHECK(init.twoView(2).status_ == -1 && init.twoView(2).inliers_.empty());
  // ---- one device call for three cameras: OK, FEW_INLIERS, CHEIRALITY
  const int st[3] = {SVO_HIP_TWO_VIEW_OK, SVO_HIP_TWO_VIEW_FEW_INLIERS, SVO_HIP_TWO_VIEW_CHEIRALITY};
  g_status.assign(st, st + 3);
  double T[21];
  for (int i = 0; i < 21; ++i) T[i] = i;
  g_calls.clear();
  CHECK(init.computeTwoViews(3, cams3, cm, T, NULL, r));
  CHECK(count("two_view") == 1 && g_last_n == 3 && g_last_T == T);
  CHECK(count("download_two_view") == 2 && count("download") == 0);                                 // OK and FEW_INLIERS have xyz, CHEIRALITY nothing
  CHECK(r[0] == KLT_SUCCESS && r[1] == KLT_FAILURE && r[2] == KLT_FAILURE);
  {
    const KltInit::TwoView& a = init.twoView(2);
    CHECK(a.status_ == SVO_HIP_TWO_VIEW_OK && a.inliers_.size() == 10 && a.inliers_[0] == 2 && a.inliers_[9] == 11);
    CHECK(a.xyz_in_cur_.size() == 12 && a.xyz_in_cur_[0][0] == 2000.0 && a.xyz_in_cur_[11][2] == 2035.0);
    CHECK(a.point_index_.size() == 9 && a.point_index_[8] == 10 && a.point_pos_.size() == 9 && a.point_pos_[8][2] == -2026.0);
    CHECK(a.T_cur_from_ref_[6] == 26.0 && a.T_cur_w_[0] == 200.0 && a.depth_median_ == 6.0 && a.scale_ == 1.0 / 6.0);
    const KltInit::TwoView& b = init.twoView(0);
    CHECK(b.status_ == SVO_HIP_TWO_VIEW_FEW_INLIERS && b.inliers_.empty() && b.point_index_.empty() && b.xyz_in_cur_.size() == 12);
    CHECK(b.T_cur_from_ref_[3] == 3.0 && b.T_cur_w_[0] != b.T_cur_w_[0] && b.scale_ != b.scale_);
    const KltInit::TwoView& c = init.twoView(3);
    CHECK(c.status_ == SVO_HIP_TWO_VIEW_CHEIRALITY && c.inliers_.empty() && c.xyz_in_cur_.empty() && c.point_pos_.empty());
  }
  // ---- the other statuses are failures too
  const int st2[2] = {SVO_HIP_TWO_VIEW_TOO_FEW, SVO_HIP_TWO_VIEW_NO_MODEL};
  g_status.assign(st2, st2 + 2);
  CHECK(init.computeTwoViews(2, cams3, cm, NULL, NULL, r) && r[0] == KLT_FAILURE && r[1] == KLT_FAILURE && g_last_T == NULL);
  CHECK(init.twoView(2).status_ == SVO_HIP_TWO_VIEW_TOO_FEW && init.twoView(2).inliers_.empty() && init.twoView(2).xyz_in_cur_.empty());
  // ---- a refused call leaves lists and results as they were
  g_status.assign(1, SVO_HIP_TWO_VIEW_OK);
  CHECK(init.computeTwoView(3, cam) == KLT_SUCCESS && init.twoView(3).inliers_.size() == 10);
  g_refuse = true;
  CHECK(init.computeTwoView(3, cam) == KLT_FAILURE);
  CHECK(init.twoView(3).status_ == SVO_HIP_TWO_VIEW_OK && init.twoView(3).inliers_.size() == 10 && init.lists(3).px_ref_.size() == 12);
  g_refuse = false;
  // ---- a new track forgets the result; a new first frame too
  const int one = 3;
  CHECK(init.trackSecondFrames(1, &one, &pyr, slots, cm, r) && init.twoView(3).status_ == -1 && init.twoView(3).inliers_.empty());
  CHECK(init.computeTwoView(2, cam) == KLT_SUCCESS);
  CHECK(init.addFirstFrame(2, &pyr, 0, px, f) == KLT_SUCCESS && init.twoView(2).status_ == -1);
  CHECK(init.computeTwoView(2, cam) == KLT_FAILURE);                                                // no track since the new reference
  // ---- the C++ twin: lists from a matcher, then addSecondFrame's second half on Frame / Point / Feature
  {
    namespace si = svo::initialization;
    si::KltInit twin(&ctx, 640, 480, 2, 64, gates);
    std::vector<si::Point2f> pr, pc;
    std::vector<svo::Vector3d> fr, fc;
    for (int i = 0; i < 12; ++i) {
      pr.push_back(si::Point2f(20.f + i, 30.f)); pc.push_back(si::Point2f(80.f + i, 31.f));
      fr.push_back(svo::Vector3d{{0.1 * i, 0.2, 1.0}}); fc.push_back(svo::Vector3d{{0.3 * i, 0.4, 1.0}});
    }
    svo::PinholeCamera pcam;
    pcam.width = 640; pcam.height = 480; pcam.fx = pcam.fy = 300.0; pcam.cx = 320.0; pcam.cy = 240.0;
    svo::Frame ref(&pcam, {}), cur(&pcam, {});
    ref.T_f_w_.p[0] = 0.5;
    CHECK(!twin.setLists(1, pr, pc, fr, fc) && count("set_lists") == 0);                              // no reference: nothing is sent
    CHECK(twin.addFirstFrame(1, &pyr, 0, pr, fr) == KLT_SUCCESS);
    CHECK(twin.addSecondFrame(1, &ref, &cur) == KLT_FAILURE && ref.fts_.empty());                      // no tracked lists
    pc.pop_back();
    CHECK(!twin.setLists(1, pr, pc, fr, fc) && count("set_lists") == 0);                              // sizes differ
    pc.push_back(si::Point2f(91.f, 31.f));
    CHECK(twin.setLists(1, pr, pc, fr, fc) && g_set_lists_n == 12 && twin.lists(1).f_cur_.size() == 12 && twin.lists(1).index_[11] == 11);
    CHECK(twin.lists(1).disparities_.size() == 12 && twin.lists(1).disparities_[0] != twin.lists(1).disparities_[0]);
    // a failure changes neither frame
    g_status.assign(1, SVO_HIP_TWO_VIEW_FEW_INLIERS);
    CHECK(twin.addSecondFrame(1, &ref, &cur) == KLT_FAILURE && ref.fts_.empty() && cur.fts_.empty() && cur.T_f_w_.p[0] == 0.0 && cur.T_f_w_.p[6] == 1.0);
    g_status.assign(1, SVO_HIP_TWO_VIEW_OK);
    CHECK(twin.addSecondFrame(1, &ref, &cur) == KLT_SUCCESS && g_last_T == ref.T_f_w_.p);
    CHECK(cur.T_f_w_.p[0] == 100.0 && cur.T_f_w_.p[6] == 106.0 && ref.T_f_w_.p[0] == 0.5);          // :108-115: the mock's T_cur_w of camera 1
    CHECK(ref.fts_.size() == 9 && cur.fts_.size() == 9);                                               // the mock's point list: features 2..10
    std::list<svo::Feature*>::const_iterator ir = ref.fts_.begin(), ic = cur.fts_.begin();
    for (int k = 0; k < 9; ++k, ++ir, ++ic) {
      const svo::Feature *a = *ir, *b = *ic;
      CHECK(a->point != NULL && a->point == b->point && a->frame == &ref && b->frame == &cur && a->level == 0 && b->level == 0);
      CHECK(a->point->obs_.size() == 2 && a->point->obs_.front() == a && a->point->obs_.back() == b);   // obs_ reads [ref, cur]
      CHECK(a->point->type_ == svo::Point::TYPE_UNKNOWN && a->point->pos_[2] == -1000.0 - (3 * k + 2));
      CHECK(a->px[0] == 20.0 + (k + 2) && a->px[1] == 30.0 && b->px[0] == 80.0 + (k + 2) && b->px[1] == 31.0);
      CHECK(a->f[0] == 0.1 * (k + 2) && b->f[0] == 0.3 * (k + 2) && a->type == svo::Feature::CORNER);
    }
    // ... and its flatten: two keyframes (ref, cur), creation order, no candidates
    svo::Map map;
    svo::FramePtr kref(&ref, [](svo::Frame*) {}), kcur(&cur, [](svo::Frame*) {});
    map.addKeyframe(kref); map.addKeyframe(kcur);
    const si::MapTables t = si::flattenMap(map);
    CHECK(t.kf_slot.size() == 2 && t.kf_ftr_offset[1] == 9 && t.kf_ftr_offset[2] == 18 && t.pt_type.size() == 9 && t.cand_point.empty());
    for (int k = 0; k < 9; ++k) {
      CHECK(t.kf_ftr_point[(size_t)k] == k && t.kf_ftr_point[(size_t)(9 + k)] == k && t.pt_obs_offset[(size_t)k + 1] == 2 * (k + 1));
      CHECK(t.obs_kf[(size_t)(2 * k)] == 0 && t.obs_kf[(size_t)(2 * k + 1)] == 1 && t.obs_level[(size_t)(2 * k)] == 0 && t.obs_edgelet[(size_t)(2 * k)] == 0);
      CHECK(t.obs_px[(size_t)(4 * k)] == 20.0 + (k + 2) && t.obs_px[(size_t)(4 * k + 2)] == 80.0 + (k + 2) && t.pt_type[(size_t)k] == 2);
    }
    CHECK(t.T_kf_w[0] == 0.5 && t.T_kf_w[7] == 100.0 && t.kf_key_point.size() == 10 && t.kf_key_point[0] == -1);
    for (svo::Feature* ftr : ref.fts_) delete ftr->point;
  }
  std::printf("klt two view mock test OK\n");
  return 0;
}
