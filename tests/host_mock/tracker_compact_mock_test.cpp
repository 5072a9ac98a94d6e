// CPU-only test of hip_bridge::FrameTrackerT::setPointCompaction (include/svo_dropin/frame_tracker_batch.h) against a MOCK of the
// svo_hip_tracker_* entry points that records every call and keeps a point table with a capacity, as
// tests/host_mock/tracker_remove_mock_test.cpp does for the removal.  Checked: with the option off a capacity refusal of
// svo_hip_tracker_add_candidates ends in one full upload, as before; with it on the bridge calls svo_hip_tracker_compact_points
// once, repeats the refused call once and uploads nothing, and its own index tables follow old_to_new (the indices it sends
// afterwards are the new ones); a second refusal ends in the full upload; a device that kept another set of points than the host
// holds ends in mapChanged(); a refused promotion takes the same path.  Built and run by
// tests/test_tracker_bridge_compact_mock.py, plain and with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "svo_hip.h"
#include "../../android_svo_amd/host/svo_host.h"

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

// ---------------------------------------------------------------- mock device
struct svo_hip_ctx { int unused; };
struct svo_hip_tracker {
  std::vector<int32_t> type;                   // the point table's types as uploaded / appended
  std::vector<uint8_t> dead;                   // ... and which of them a frame has deleted (the device's pt_unlinked)
  int max_points = 0;
  int n_kf = 0;
  std::vector<uint8_t> image;
};
static std::vector<std::string> g_calls;
static int g_fail_add = 0, g_fail_promote = 0;   // how many of the next calls are refused whatever the capacity
static bool g_fail_compact = false;
static int g_revive = -1;                        // the next compaction keeps this dead point: the device and the host disagree
static std::vector<int> g_delete_next;           // table indices the next tracked frame deletes
static std::vector<int32_t> g_add_kf, g_moved;   // kf_index of the last accepted append; the indices of the last update_point_positions
static int g_add_first = -1, g_add_n = 0;
static svo_hip_tracker_map g_last_map;           // the scalars of the last upload (its pointers are stale)

extern "C" {
int svo_hip_ctx_create(svo_hip_ctx** out, int, void*) { *out = new svo_hip_ctx(); return SVO_HIP_OK; }
int svo_hip_ctx_destroy(svo_hip_ctx* c) { delete c; return SVO_HIP_OK; }
const char* svo_hip_last_error(svo_hip_ctx*) { return "mock"; }
int svo_hip_tracker_create(svo_hip_ctx*, const svo_hip_camera* cam, const svo_hip_tracker_config* cfg, svo_hip_tracker** out) {
  *out = new svo_hip_tracker();
  (*out)->image.resize((size_t)cam->width * cam->height);
  (*out)->max_points = cfg->max_points;
  return SVO_HIP_OK;
}
int svo_hip_tracker_destroy(svo_hip_tracker* t) { delete t; return SVO_HIP_OK; }
int svo_hip_tracker_image_buffer(svo_hip_tracker* t, uint8_t** b) { *b = t->image.data(); return SVO_HIP_OK; }
int svo_hip_tracker_upload_keyframe(svo_hip_tracker*, int, const uint8_t*) { g_calls.push_back("upload_keyframe"); return SVO_HIP_OK; }
int svo_hip_tracker_keyframe_from_last_frame(svo_hip_tracker*, int) { g_calls.push_back("keyframe_from_last_frame"); return SVO_HIP_OK; }
int svo_hip_tracker_set_map(svo_hip_tracker* t, const svo_hip_tracker_map* m) {
  g_calls.push_back("set_map");
  if (m->n_points > t->max_points) return SVO_HIP_ERR_INVALID;
  t->type.assign(m->pt_type, m->pt_type + m->n_points);
  t->dead.assign((size_t)m->n_points, 0);        // (an upload unlinks nothing)
  t->n_kf = m->n_kf;
  g_last_map = *m;
  return SVO_HIP_OK;
}
int svo_hip_tracker_update_point_positions(svo_hip_tracker* t, int n, const int32_t* idx, const double*) {
  g_calls.push_back("update_point_positions");
  g_moved.assign(idx, idx + n);
  for (int i = 0; i < n; ++i) if (idx[i] < 0 || idx[i] >= (int)t->type.size()) return SVO_HIP_ERR_INVALID;
  return SVO_HIP_OK;
}
int svo_hip_tracker_optimize_structure(svo_hip_tracker*, int, const int32_t*, int, double*, int32_t*) { g_calls.push_back("optimize_structure"); return SVO_HIP_OK; }
int svo_hip_tracker_set_last_frame(svo_hip_tracker*, const uint8_t*, int, const double*, int, const double*, const double*, const int32_t*) {
  g_calls.push_back("set_last_frame");
  return SVO_HIP_OK;
}
int svo_hip_tracker_add_candidates(svo_hip_tracker* t, int n, const double*, const int32_t* kf, const double*, const double*, const int32_t*,
                                   const uint8_t*, const double*, int32_t* first) {
  g_calls.push_back("add_candidates");
  if (g_fail_add > 0) { --g_fail_add; return SVO_HIP_ERR_INVALID; }
  if (n > t->max_points - (int)t->type.size()) return SVO_HIP_ERR_INVALID;     // the capacity: dead rows count until they are compacted
  for (int i = 0; i < n; ++i) if (kf[i] < -1 || kf[i] >= t->n_kf) return SVO_HIP_ERR_INVALID;
  g_add_kf.assign(kf, kf + n);
  g_add_first = (int)t->type.size(); g_add_n = n;
  if (first) *first = g_add_first;
  t->type.insert(t->type.end(), (size_t)n, 1);
  t->dead.insert(t->dead.end(), (size_t)n, 0);
  return SVO_HIP_OK;
}
int svo_hip_tracker_promote_last_frame(svo_hip_tracker* t, int, int* kf_index, int* n_promoted) {
  g_calls.push_back("promote_last_frame");
  if (g_fail_promote > 0) { --g_fail_promote; return SVO_HIP_ERR_INVALID; }
  *kf_index = t->n_kf++;
  *n_promoted = 0;
  return SVO_HIP_OK;
}
int svo_hip_tracker_remove_keyframe(svo_hip_tracker*, int, int*, int*, int*) { g_calls.push_back("remove_keyframe"); return SVO_HIP_ERR_INVALID; }
int svo_hip_tracker_compact_points(svo_hip_tracker* t, int* n_after, int32_t* old_to_new) {
  g_calls.push_back("compact_points");
  if (g_fail_compact) return SVO_HIP_ERR_STATE;
  std::vector<int32_t> type;
  for (size_t p = 0; p < t->type.size(); ++p) {
    const bool alive = !t->dead[p] || (int)p == g_revive;
    if (old_to_new) old_to_new[p] = alive ? (int32_t)type.size() : -1;
    if (alive) type.push_back(t->type[p]);
  }
  g_revive = -1;
  t->type.swap(type);
  t->dead.assign(t->type.size(), 0);
  if (n_after) *n_after = (int)t->type.size();
  return SVO_HIP_OK;
}
// a frame: three features on the first three points; the points of g_delete_next are deleted, every other counter as it was
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
  for (int p : g_delete_next) { t->type[(size_t)p] = 0; t->dead[(size_t)p] = 1; r->map_changed = 1; }
  g_delete_next.clear();
  for (size_t p = 0; p < t->type.size(); ++p) { pt_type[p] = t->type[p]; pt_failed[p] = 0; pt_succ[p] = 0; }
  return SVO_HIP_OK;
}
int svo_hip_tracker_last_result(svo_hip_tracker*, svo_hip_track_result*, double*, double*, int32_t*, int32_t*, uint8_t*, double*, int32_t*, int32_t*,
                                int32_t*) { return SVO_HIP_ERR_STATE; }
int svo_hip_tracker_default_config(svo_hip_tracker_config* c) {
  std::memset(c, 0, sizeof(*c));
  c->max_keyframes = 8; c->max_frame_features = 16; c->max_points = 9;
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

/// a frame that is tracked nowhere, with one feature on each of the given points: what pointsOptimised sends are their table indices
static FramePtr probe(World& w, const std::vector<Point*>& pts) {
  FramePtr fr = w.newFrame(0.5);
  for (Point* pt : pts) {
    Feature* ftr = new Feature(fr.get(), Vector2d{{3.0, 4.0}}, Vector3d{{0.0, 0.0, 1.0}}, 0);
    ftr->point = pt;
    fr->addFeature(ftr);
  }
  return fr;
}

// The tables of the first upload, in the order the bridge flattens the world: keyframe 0's points 0, 2, 4, 5 (indices 0-3), keyframe
// 1's points 1, 3 (4, 5), the candidates of keyframe 0 and of keyframe 1 (6, 7).  The mock's frames match the indices 0, 1, 2.
static void start(World& w, FrameTracker& trk) {
  w.frame(trk, w.kfs[0], 1.5);
  CALLS("upload_keyframe upload_keyframe set_map set_last_frame track");
  CHECK(g_last_map.n_points == 8 && g_last_map.n_candidates == 2 && trk.mapUploads() == 1);
  // a frame deletes point 1 (index 4) and the candidate of keyframe 0 (index 6): the host forgets the objects, the rows stay
  g_delete_next = {4, 6};
  w.frame(trk, w.kfs[0], 1.6);
  CALLS("track");
  CHECK(w.points[1]->type_ == Point::TYPE_DELETED && w.points[6]->type_ == Point::TYPE_DELETED && w.map.point_candidates_.candidates_.size() == 1);
}

static void test_option_off() {
  World w;
  FrameTracker trk(w.cam, config());
  trk.setIncrementalMap(true);
  CHECK(!trk.pointCompaction());
  start(w, trk);
  w.addCandidate(w.kfs[0].get(), 3.0);
  w.addCandidate(w.kfs[1].get(), 4.0);                                          // 8 rows + 2 > max_points 9
  w.frame(trk, w.kfs[0], 1.7);
  CALLS("add_candidates set_map set_last_frame track");                         // refused: the full upload, as before
  CHECK(trk.mapUploads() == 2 && trk.pointCompactions() == 0 && g_last_map.n_points == 8 && g_last_map.n_candidates == 3);
}

static void test_option_on() {
  World w;
  FrameTracker trk(w.cam, config());
  trk.setIncrementalMap(true);
  trk.setPointCompaction(true);
  CHECK(trk.pointCompaction());
  start(w, trk);
  // ---- compact, retry, no upload
  Point* c0 = w.addCandidate(w.kfs[0].get(), 3.0);
  Point* c1 = w.addCandidate(w.kfs[1].get(), 4.0);
  w.frame(trk, w.kfs[0], 1.7);
  CALLS("add_candidates compact_points add_candidates track");
  CHECK(trk.mapUploads() == 1 && trk.pointCompactions() == 1);
  CHECK(g_add_first == 6 && g_add_n == 2 && g_add_kf == (std::vector<int32_t>{0, 1}));
  // the index tables were rewritten: point 3 was 5 and is 4, keyframe 1's candidate was 7 and is 5, the new ones are 6 and 7; a
  // forgotten point is sent nowhere
  CHECK(trk.pointsOptimised(*probe(w, {w.points[3].get(), w.points[7].get(), c0, c1, w.points[0].get(), w.points[1].get()})));
  CALLS("update_point_positions");
  CHECK(g_moved == (std::vector<int32_t>{4, 5, 6, 7, 0}));
  // the next frame's counters are for the eight rows the device holds now; a deletion finds its object under the new index
  g_delete_next = {4};
  w.frame(trk, w.kfs[0], 1.8);
  CALLS("track");
  CHECK(w.points[3]->type_ == Point::TYPE_DELETED && w.points[5]->type_ != Point::TYPE_DELETED);
  // ---- room again: one more candidate fits without anything (8 rows, max_points 9)
  w.addCandidate(w.kfs[0].get(), 5.0);
  w.frame(trk, w.kfs[0], 1.9);
  CALLS("add_candidates track");
  CHECK(g_add_first == 8 && trk.pointCompactions() == 1);
  // ---- a second refusal after the compaction: the full upload
  w.addCandidate(w.kfs[0].get(), 6.0);
  g_fail_add = 2;
  w.frame(trk, w.kfs[0], 2.0);
  CALLS("add_candidates compact_points add_candidates set_map set_last_frame track");
  CHECK(trk.mapUploads() == 2 && trk.pointCompactions() == 2 && g_fail_add == 0);
  CHECK(g_last_map.n_points == 9 && g_last_map.n_candidates == 5);              // points 0, 2, 4, 5 and five candidates
  // ---- the device kept a point the host has forgotten: mapChanged(), no second attempt
  g_delete_next = {3};                                                          // point 5
  w.frame(trk, w.kfs[0], 2.1);
  CALLS("track");
  CHECK(w.points[5]->type_ == Point::TYPE_DELETED);
  w.addCandidate(w.kfs[1].get(), 7.0);                                          // 9 rows + 1 > 9
  g_revive = 3;
  w.frame(trk, w.kfs[0], 2.2);
  CALLS("add_candidates compact_points set_map set_last_frame track");
  CHECK(trk.mapUploads() == 3 && trk.pointCompactions() == 3 && g_last_map.n_points == 9);
  // ---- a compaction the device refuses changes nothing: the full upload
  g_delete_next = {3};
  w.frame(trk, w.kfs[0], 2.3);
  w.addCandidate(w.kfs[1].get(), 8.0);
  g_fail_compact = true;
  take();
  w.frame(trk, w.kfs[0], 2.4);
  CALLS("add_candidates compact_points set_map set_last_frame track");
  g_fail_compact = false;
  CHECK(trk.mapUploads() == 4 && trk.pointCompactions() == 3);
}

// a refused promotion takes the same path: compact, promote again, no upload
static void test_refused_promotion() {
  World w;
  FrameTracker trk(w.cam, config());
  trk.setIncrementalMap(true);
  trk.setPointCompaction(true);
  start(w, trk);
  FramePtr cur = w.frame(trk, w.kfs[0], 2.0);
  take();
  g_fail_promote = 1;
  CHECK(w.makeKeyframe(trk, cur, 10) == nullptr);
  CALLS("promote_last_frame compact_points promote_last_frame");
  CHECK(trk.pointCompactions() == 1 && trk.mapUploads() == 1);
  CHECK(trk.pointsOptimised(*probe(w, {w.points[3].get(), w.points[7].get()})));
  CALLS("update_point_positions");
  CHECK(g_moved == (std::vector<int32_t>{4, 5}));
  w.frame(trk, w.kfs[0], 2.5);
  CALLS("track");
  // refused twice: the keyframe goes up with the next full upload, as it did before
  cur = w.frame(trk, w.kfs[0], 3.0);
  take();
  g_fail_promote = 2;
  CHECK(w.makeKeyframe(trk, cur, 10) == nullptr);
  CALLS("promote_last_frame compact_points promote_last_frame keyframe_from_last_frame");
  w.frame(trk, w.kfs[0], 3.5);
  CALLS("set_map set_last_frame track");
  CHECK(trk.mapUploads() == 2 && trk.pointCompactions() == 2 && g_last_map.n_kf == 4);
  // without the incremental mode the option does nothing
  World w2;
  FrameTracker off(w2.cam, config());
  off.setPointCompaction(true);
  w2.frame(off, w2.kfs[0], 1.5);
  w2.addCandidate(w2.kfs[0].get(), 3.0);
  take();
  w2.frame(off, w2.kfs[0], 1.6);
  CALLS("set_map set_last_frame track");
  CHECK(off.pointCompactions() == 0);
}

int main() {
  test_option_off();
  test_option_on();
  test_refused_promotion();
  std::printf("tracker compaction mock test OK\n");
  return 0;
}
