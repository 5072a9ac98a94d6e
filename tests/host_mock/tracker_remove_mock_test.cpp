// CPU-only test of hip_bridge::FrameTrackerT::keyframeRemoved (include/svo_dropin/frame_tracker_batch.h) and of the removal
// functions of the twins (android_svo_amd/host/svo_host.h: Map::safeDeleteFrame, removePtFrameRef, getFurthestKeyframe,
// MapPointCandidates::removeFrameCandidates, Point::deleteFrameRef) against a MOCK of the svo_hip_tracker_* entry points that
// records every call, as tests/host_mock/tracker_mock_test.cpp does for the map's growth.  Checked: with setIncrementalMap a
// removed keyframe goes down as exactly one svo_hip_tracker_remove_keyframe with its index and no svo_hip_tracker_set_map; the
// keyframes behind it are renumbered (overlap_kfs, the kf_index of later candidates, -1 for a seed of the keyframe that left);
// its pyramid slot is the next promotion's; a refusal, or counts that differ from what the host deleted, or the mode off, end
// in one full upload.  Built and run by tests/test_tracker_bridge_remove_mock.py, plain and with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

#include "svo_hip.h"
#include "../../android_svo_amd/host/svo_host.h"

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

// ---------------------------------------------------------------- mock device
struct svo_hip_ctx { int unused; };
struct svo_hip_tracker {
  std::vector<int32_t> type;                   // the point table's types as uploaded / appended
  int n_kf = 0, n_candidates = 0;
  std::vector<int> kf_slot;
  std::vector<uint8_t> image;
  int frame_features = 0;                      // features of the last tracked frame
};
static std::vector<std::string> g_calls;
static bool g_fail_add = false, g_fail_promote = false;
struct AddRecord { std::vector<double> pos, px, f, grad; std::vector<int32_t> kf, level; std::vector<uint8_t> edge; int first = -1; };
static AddRecord g_add;
static int g_promoted_slot = -1;
static bool g_fail_remove = false;
static int g_removed_index = -1, g_report_points = 0, g_report_cands = 0;     // what the mock device says it deleted
static svo_hip_tracker_map g_last_map;         // the scalars of the last upload (its pointers are stale)

extern "C" {
int svo_hip_ctx_create(svo_hip_ctx** out, int, void*) { *out = new svo_hip_ctx(); return SVO_HIP_OK; }
int svo_hip_ctx_destroy(svo_hip_ctx* c) { delete c; return SVO_HIP_OK; }
const char* svo_hip_last_error(svo_hip_ctx*) { return "mock"; }
int svo_hip_tracker_create(svo_hip_ctx*, const svo_hip_camera* cam, const svo_hip_tracker_config*, svo_hip_tracker** out) {
  *out = new svo_hip_tracker();
  (*out)->image.resize((size_t)cam->width * cam->height);
  return SVO_HIP_OK;
}
int svo_hip_tracker_destroy(svo_hip_tracker* t) { delete t; return SVO_HIP_OK; }
int svo_hip_tracker_image_buffer(svo_hip_tracker* t, uint8_t** b) { *b = t->image.data(); return SVO_HIP_OK; }
int svo_hip_tracker_upload_keyframe(svo_hip_tracker*, int, const uint8_t*) { g_calls.push_back("upload_keyframe"); return SVO_HIP_OK; }
int svo_hip_tracker_keyframe_from_last_frame(svo_hip_tracker*, int) { g_calls.push_back("keyframe_from_last_frame"); return SVO_HIP_OK; }
int svo_hip_tracker_set_map(svo_hip_tracker* t, const svo_hip_tracker_map* m) {
  g_calls.push_back("set_map");
  t->type.assign(m->pt_type, m->pt_type + m->n_points);
  t->n_kf = m->n_kf; t->n_candidates = m->n_candidates;
  t->kf_slot.assign(m->kf_slot, m->kf_slot + m->n_kf);
  g_last_map = *m;
  return SVO_HIP_OK;
}
int svo_hip_tracker_update_point_positions(svo_hip_tracker*, int, const int32_t*, const double*) { g_calls.push_back("update_point_positions"); return SVO_HIP_OK; }
int svo_hip_tracker_optimize_structure(svo_hip_tracker*, int, const int32_t*, int, double*, int32_t*) { g_calls.push_back("optimize_structure"); return SVO_HIP_OK; }
int svo_hip_tracker_set_last_frame(svo_hip_tracker*, const uint8_t*, int, const double*, int, const double*, const double*, const int32_t*) {
  g_calls.push_back("set_last_frame");
  return SVO_HIP_OK;
}
int svo_hip_tracker_add_candidates(svo_hip_tracker* t, int n, const double* pos, const int32_t* kf, const double* px, const double* f, const int32_t* level,
                                   const uint8_t* edge, const double* grad, int32_t* first) {
  g_calls.push_back("add_candidates");
  if (g_fail_add) return SVO_HIP_ERR_INVALID;
  for (int i = 0; i < n; ++i) if (kf[i] < -1 || kf[i] >= t->n_kf) return SVO_HIP_ERR_INVALID;
  g_add = AddRecord();
  g_add.pos.assign(pos, pos + 3 * n); g_add.px.assign(px, px + 2 * n); g_add.f.assign(f, f + 3 * n); g_add.grad.assign(grad, grad + 2 * n);
  g_add.kf.assign(kf, kf + n); g_add.level.assign(level, level + n); g_add.edge.assign(edge, edge + n);
  g_add.first = (int)t->type.size();
  if (first) *first = g_add.first;
  t->type.insert(t->type.end(), (size_t)n, 1);
  t->n_candidates += n;
  return SVO_HIP_OK;
}
int svo_hip_tracker_promote_last_frame(svo_hip_tracker* t, int slot, int* kf_index, int* n_promoted) {
  g_calls.push_back("promote_last_frame");
  if (g_fail_promote) return SVO_HIP_ERR_INVALID;
  g_promoted_slot = slot;
  *kf_index = t->n_kf++;
  t->kf_slot.push_back(slot);
  *n_promoted = 0;
  return SVO_HIP_OK;
}
int svo_hip_tracker_remove_keyframe(svo_hip_tracker* t, int k, int* slot, int* n_points, int* n_cands) {
  g_calls.push_back("remove_keyframe");
  if (g_fail_remove || k < 0 || k >= t->n_kf || t->n_kf == 1) return SVO_HIP_ERR_INVALID;
  g_removed_index = k;
  *slot = t->kf_slot[(size_t)k]; *n_points = g_report_points; *n_cands = g_report_cands;
  t->kf_slot.erase(t->kf_slot.begin() + k);
  t->n_kf -= 1; t->n_candidates -= g_report_cands;
  return SVO_HIP_OK;
}
// a frame: three features on the first three points, every counter as it was
int svo_hip_tracker_track(svo_hip_tracker* t, const uint8_t*, svo_hip_track_result* r, double* px, double* f, int32_t* level, int32_t* point, uint8_t* edge,
                          double* grad, int32_t* pt_type, int32_t* pt_failed, int32_t* pt_succ) {
  g_calls.push_back("track");
  std::memset(r, 0, sizeof(*r));
  r->T_f_w[6] = 1.0;
  r->n_features = 3; r->n_matches = 3; r->n_overlap = 1; r->overlap_kf[0] = 0; r->overlap_count[0] = 3;
  for (int i = 0; i < 3; ++i) {
    px[2 * i] = 10.0 + i; px[2 * i + 1] = 12.0; f[3 * i] = 0.0; f[3 * i + 1] = 0.0; f[3 * i + 2] = 1.0;
    level[i] = 0; point[i] = i; edge[i] = 0; grad[2 * i] = 1.0; grad[2 * i + 1] = 0.0;
  }
  for (size_t p = 0; p < t->type.size(); ++p) { pt_type[p] = t->type[p]; pt_failed[p] = 0; pt_succ[p] = 0; }
  t->frame_features = 3;
  return SVO_HIP_OK;
}
int svo_hip_tracker_last_result(svo_hip_tracker*, svo_hip_track_result*, double*, double*, int32_t*, int32_t*, uint8_t*, double*, int32_t*, int32_t*,
                                int32_t*) { return SVO_HIP_ERR_STATE; }
int svo_hip_tracker_default_config(svo_hip_tracker_config* c) {
  std::memset(c, 0, sizeof(*c));
  c->max_keyframes = 8; c->max_frame_features = 16;
  return SVO_HIP_OK;
}
}  // extern "C"

// ---------------------------------------------------------------- a small world on the twins
using namespace svo;
static const int W = 32, H = 24;

struct World {
  PinholeCamera cam{W, H, 30.0, 30.0, 16.0, 12.0};
  Map map;
  std::vector<std::unique_ptr<Point>> points;
  std::vector<FramePtr> kfs;                   // every keyframe there ever was, in order of creation
  FramePtr last;
  FramePtr newFrame(double x = 0.0) {
    std::vector<std::vector<uint8_t>> pyr(1, std::vector<uint8_t>((size_t)W * H, 7));
    FramePtr f = std::make_shared<Frame>(&cam, std::move(pyr));
    const double T[7] = {-x, 0, 0, 0, 0, 0, 1};                                   // camera centre (x, 0, 0)
    f->T_f_w_ = SE3(T);
    return f;
  }
  // two keyframes, six points: the even ones seen by keyframe 0, the odd ones by keyframe 1, point 5 by both; a candidate of each
  World() {
    for (int k = 0; k < 2; ++k) kfs.push_back(newFrame(1.0 * k));
    for (int p = 0; p < 6; ++p) {
      points.emplace_back(new Point(Vector3d{{0.1 * p, 0.2, 2.0}}));
      observe(kfs[(size_t)(p % 2)], p);
    }
    observe(kfs[0], 5);
    for (FramePtr& kf : kfs) { kf->setKeyframe(); map.addKeyframe(kf); }
    addCandidate(kfs[0].get(), 1.0);
    addCandidate(kfs[1].get(), 2.0);
    last = kfs[1];
  }
  void observe(const FramePtr& kf, int p) {
    Feature* ftr = new Feature(kf.get(), Vector2d{{5.0 + p, 6.0}}, Vector3d{{0.0, 0.0, 1.0}}, 0);
    ftr->point = points[(size_t)p].get();
    ftr->point->addFrameRef(ftr);
    kf->addFeature(ftr);
  }
  Point* addCandidate(Frame* frame, double x) {
    Feature* ftr = new Feature(frame, Vector2d{{x, x + 1.0}}, Vector3d{{x, 0.5, 1.0}}, 2);
    points.emplace_back(new Point(Vector3d{{x, -x, 3.0}}, ftr));
    ftr->point = points.back().get();
    points.back()->type_ = Point::TYPE_CANDIDATE;
    std::unique_lock<std::mutex> lock(map.point_candidates_.mut_);
    map.point_candidates_.candidates_.push_back(MapPointCandidates::PointCandidate(points.back().get(), ftr));
    return points.back().get();
  }
  /// one frame through the tracker (the mock matches points 0, 1, 2 and names keyframe 0 as the overlap); returns the frame
  FramePtr frame(FrameTracker& trk, const FramePtr& first_keyframe, double x) {
    FramePtr cur = newFrame(x);
    std::vector<std::pair<FramePtr, size_t>> overlap;
    FrameTracker::Outcome oc;
    CHECK(trk.track(last, cur, map, overlap, oc));
    CHECK(cur->fts_.size() == 3 && overlap.size() == 1 && overlap[0].first == first_keyframe);
    cur->T_f_w_ = newFrame(x)->T_f_w_;                                           // (the mock reports the identity pose: the world knows better)
    last = cur;
    return cur;
  }
  /// processFrame :267-276 and :303-312 on the objects: the frame becomes a keyframe; a full map loses its furthest one
  FramePtr makeKeyframe(FrameTracker& trk, const FramePtr& cur, size_t max_kfs) {
    cur->setKeyframe();
    for (Feature* ftr : cur->fts_) if (ftr->point != nullptr) ftr->point->addFrameRef(ftr);
    map.point_candidates_.addCandidatePointToFrame(cur);
    FramePtr furthest;
    if (map.size() >= max_kfs) furthest = map.getFurthestKeyframe(cur->pos());
    map.addKeyframe(cur);
    kfs.push_back(cur);
    CHECK(trk.lastFrameBecameKeyframe(cur, map));
    if (furthest) CHECK(map.safeDeleteFrame(furthest));
    return furthest;
  }
};

static std::string take() {
  std::string s;
  for (const std::string& c : g_calls) s += (s.empty() ? "" : " ") + c;
  g_calls.clear();
  return s;
}
#define CALLS(expected) do { const std::string got_ = take(); if (got_ != (expected)) { \
  std::fprintf(stderr, "line %d: calls were [%s], expected [%s]\n", __LINE__, got_.c_str(), (expected)); std::exit(1); } } while (0)

static svo_hip_tracker_config config() {
  svo_hip_tracker_config cfg;
  svo_hip_tracker_default_config(&cfg);
  return cfg;
}

// the twins' own removal, no tracker involved
static void test_twin_objects() {
  World w;
  Point* cand0 = w.map.point_candidates_.candidates_.front().first;
  Point* cand1 = w.map.point_candidates_.candidates_.back().first;
  CHECK(w.map.getFurthestKeyframe(Vector3d{{3.0, 0.0, 0.0}}) == w.kfs[0] && w.map.getFurthestKeyframe(Vector3d{{-1.0, 0.0, 0.0}}) == w.kfs[1]);
  CHECK(w.map.getFurthestKeyframe(w.kfs[0]->pos()) == w.kfs[1]);
  Feature* key_of_5 = nullptr;                                                  // point 5's feature in keyframe 1
  for (Feature* ftr : w.kfs[1]->fts_) if (ftr->point == w.points[5].get()) key_of_5 = ftr;
  CHECK(key_of_5 != nullptr);
  FramePtr third = w.newFrame(2.0);                                             // a third keyframe that sees point 5 too: three observations
  w.observe(third, 5);
  third->setKeyframe();
  w.map.addKeyframe(third);
  CHECK(w.points[5]->obs_.size() == 3);
  CHECK(w.map.safeDeleteFrame(w.kfs[0]) && !w.map.safeDeleteFrame(w.kfs[0]));   // (the second time it is not there)
  CHECK(w.map.size() == 2 && w.map.keyframes_.front() == w.kfs[1]);
  for (int p : {0, 2, 4}) CHECK(w.points[(size_t)p]->type_ == Point::TYPE_DELETED && w.points[(size_t)p]->obs_.empty());
  for (int p : {1, 3}) CHECK(w.points[(size_t)p]->type_ == Point::TYPE_UNKNOWN && w.points[(size_t)p]->obs_.size() == 1);
  CHECK(w.points[5]->type_ == Point::TYPE_UNKNOWN && w.points[5]->obs_.size() == 2);   // it forgot the keyframe, kept the others in order
  CHECK(w.points[5]->obs_.front()->frame == third.get() && w.points[5]->obs_.back() == key_of_5 && key_of_5->point == w.points[5].get());
  for (Feature* ftr : w.kfs[0]->fts_) CHECK(ftr->point == nullptr);
  CHECK(cand0->type_ == Point::TYPE_DELETED && cand1->type_ == Point::TYPE_CANDIDATE);
  CHECK(w.map.point_candidates_.candidates_.size() == 1 && w.map.point_candidates_.candidates_.front().first == cand1);
  CHECK(w.map.trash_points_.size() == 3 && w.map.point_candidates_.trash_points_.size() == 1);
  // two observations left: the next removal takes the point, and keyframe `third` loses it as a key feature and chooses again
  CHECK(w.map.safeDeleteFrame(w.kfs[1]));
  CHECK(w.points[5]->type_ == Point::TYPE_DELETED && third->fts_.front()->point == nullptr);
  for (const Feature* k : third->key_pts_) CHECK(k == nullptr);
}

static void test_removal_in_place() {
  World w;
  FrameTracker trk(w.cam, config());
  trk.setIncrementalMap(true);
  w.frame(trk, w.kfs[0], 1.5);
  CALLS("upload_keyframe upload_keyframe set_map set_last_frame track");
  CHECK(g_last_map.n_kf == 2 && g_last_map.n_points == 8 && g_last_map.n_candidates == 2);
  // ---- a third keyframe near keyframe 1: keyframe 0 is the furthest and leaves.  The new keyframe sees the first three points
  // of the tables, which are keyframe 0's 0, 2 and 4: two observations each, so they go with it, as do point 5 (seen by keyframes 0
  // and 1) and the candidate seeded there
  FramePtr cur = w.frame(trk, w.kfs[0], 2.0);
  g_report_points = 4; g_report_cands = 1;
  FramePtr gone = w.makeKeyframe(trk, cur, 2);
  CHECK(gone == w.kfs[0] && trk.keyframeRemoved(gone, w.map));
  CALLS("track promote_last_frame remove_keyframe");
  CHECK(g_promoted_slot == 2 && g_removed_index == 0);
  for (int p : {0, 2, 4, 5}) CHECK(w.points[(size_t)p]->type_ == Point::TYPE_DELETED);
  CHECK(w.points[1]->type_ == Point::TYPE_UNKNOWN && w.map.point_candidates_.candidates_.size() == 1);
  w.frame(trk, w.kfs[1], 2.5);                                                  // keyframe 1 is index 0 now
  CALLS("track");                                                               // no set_map, no set_last_frame
  CHECK(trk.mapUploads() == 1);
  CHECK(w.last->fts_.front()->point == nullptr);                                // (a feature on the deleted point 0: the object is forgotten)
  // ---- later candidates: seeds of the keyframes that moved down get their new index, a seed of the one that left gets none
  w.addCandidate(w.kfs[1].get(), 3.0);
  w.addCandidate(w.kfs[2].get(), 4.0);
  w.addCandidate(w.kfs[0].get(), 5.0);
  w.frame(trk, w.kfs[1], 3.0);
  CALLS("add_candidates track");
  CHECK(g_add.first == 8 && g_add.kf == (std::vector<int32_t>{0, 1, -1}));
  // ---- the freed slot takes the next keyframe; now keyframe 1 is the furthest.  Points 1 and 3 (one observation each) and its
  // two candidates go with it
  cur = w.frame(trk, w.kfs[1], 4.0);
  g_report_points = 2; g_report_cands = 2;
  gone = w.makeKeyframe(trk, cur, 2);
  CHECK(gone == w.kfs[1] && trk.keyframeRemoved(gone, w.map));
  CALLS("track promote_last_frame remove_keyframe");
  CHECK(g_promoted_slot == 0 && g_removed_index == 0);
  CHECK(w.points[1]->type_ == Point::TYPE_DELETED && w.points[3]->type_ == Point::TYPE_DELETED);
  w.frame(trk, w.kfs[2], 4.5);
  CALLS("track");
  CHECK(trk.mapUploads() == 1);
  // ---- the device reports other counts than the host deleted: one full upload puts it right
  cur = w.frame(trk, w.kfs[2], 6.0);
  g_report_points = 0; g_report_cands = 0;                                      // (the host deletes the candidate of keyframe 2)
  gone = w.makeKeyframe(trk, cur, 2);
  CHECK(gone == w.kfs[2] && trk.keyframeRemoved(gone, w.map));
  CALLS("track promote_last_frame remove_keyframe");
  w.frame(trk, w.kfs[3], 6.5);
  CALLS("set_map set_last_frame track");
  CHECK(trk.mapUploads() == 2 && g_last_map.n_kf == 2 && g_last_map.n_candidates == 1);
  // ---- a refusal: the same
  cur = w.frame(trk, w.kfs[3], 8.0);
  g_fail_remove = true;
  gone = w.makeKeyframe(trk, cur, 2);
  CHECK(gone == w.kfs[3] && trk.keyframeRemoved(gone, w.map));
  CALLS("track promote_last_frame remove_keyframe");
  g_fail_remove = false;
  w.frame(trk, w.kfs[4], 8.5);
  CALLS("set_map set_last_frame track");
  CHECK(trk.mapUploads() == 3 && g_last_map.n_kf == 2);
  // ---- a keyframe the tables do not hold, and a dirty map: no device call
  CHECK(trk.keyframeRemoved(w.kfs[0], w.map));
  CALLS("");
  w.frame(trk, w.kfs[4], 9.0);
  CALLS("set_map set_last_frame track");
}

static void test_mode_off() {
  World w;
  FrameTracker trk(w.cam, config());
  w.frame(trk, w.kfs[0], 1.5);
  FramePtr cur = w.frame(trk, w.kfs[0], 2.0);
  take();
  FramePtr gone = w.makeKeyframe(trk, cur, 2);
  CHECK(gone == w.kfs[0] && trk.keyframeRemoved(gone, w.map));
  CALLS("keyframe_from_last_frame");
  w.frame(trk, w.kfs[1], 2.5);
  CALLS("set_map set_last_frame track");
  CHECK(g_last_map.n_kf == 2 && g_last_map.n_candidates == 1);
}

// Config::maxNKfs()'s own bound: ten keyframes (eleven pyramid slots), forty promotions along a line and along a path that turns
// back, each past the ninth followed by the removal of the furthest keyframe -- one upload, no slot runs out, every removal in place
static void test_bound_of_ten(bool turns_back) {
  World w;
  svo_hip_tracker_config cfg = config();
  cfg.max_keyframes = 11;
  FrameTracker trk(w.cam, cfg);
  trk.setIncrementalMap(true);
  std::set<const Point*> dead;
  int n_removed = 0;
  for (int k = 0; k < 80; ++k) {
    const int r = k % 38;
    const double x = 2.0 + 0.3 * (turns_back ? (r <= 19 ? r : 38 - r) : k);
    FramePtr cur = w.frame(trk, w.map.keyframes_.front(), x);
    if (k % 2 == 0) continue;
    const size_t n_list = w.map.point_candidates_.candidates_.size();
    FramePtr gone = w.makeKeyframe(trk, cur, 10);
    CHECK((gone != nullptr) == (w.kfs.size() > 10));
    if (!gone) continue;
    int n_dead = 0;                                                             // what the host's safeDeleteFrame deleted: the mock device agrees
    for (const auto& p : w.points) if (p->type_ == Point::TYPE_DELETED && dead.insert(p.get()).second) ++n_dead;
    g_report_cands = (int)(n_list - w.map.point_candidates_.candidates_.size());
    g_report_points = n_dead - g_report_cands;
    CHECK(trk.keyframeRemoved(gone, w.map));
    CHECK(w.map.size() == 10);
    ++n_removed;
  }
  CHECK(n_removed >= 30 && trk.mapUploads() == 1);
  int n_set_map = 0, n_remove = 0, n_promote = 0;
  for (const std::string& c : g_calls) { n_set_map += c == "set_map"; n_remove += c == "remove_keyframe"; n_promote += c == "promote_last_frame"; }
  CHECK(n_set_map == 1 && n_remove == n_removed && n_promote == 40);
  g_calls.clear();
}

int main() {
  test_twin_objects();
  test_removal_in_place();
  test_mode_off();
  test_bound_of_ten(false);
  test_bound_of_ten(true);
  std::printf("tracker removal mock test OK\n");
  return 0;
}
