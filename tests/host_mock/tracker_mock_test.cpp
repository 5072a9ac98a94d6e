// CPU-only test of hip_bridge::FrameTrackerT (include/svo_dropin/frame_tracker_batch.h) on the self-contained twins of
// android_svo_amd/host/svo_host.h against a MOCK of the svo_hip_tracker_* entry points that records every call (no GPU, no
// oracle: the mock "tracks" a frame by matching the first three points it knows).  What is checked is the host logic of
// setIncrementalMap: a grown candidate list goes down as exactly one svo_hip_tracker_add_candidates with the right arrays and
// no svo_hip_tracker_set_map, a promoted keyframe as one svo_hip_tracker_promote_last_frame, a failing incremental call is
// followed by one full upload -- and with the mode off the sequence of calls is what it was before the mode existed.
// Built and run by tests/test_tracker_bridge_mock.py with g++ -std=c++17, plain and with -fsanitize=address,undefined.
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
  int n_kf = 0, n_candidates = 0;
  std::vector<uint8_t> image;
  int frame_features = 0;                      // features of the last tracked frame
};
static std::vector<std::string> g_calls;
static bool g_fail_add = false, g_fail_promote = false;
struct AddRecord { std::vector<double> pos, px, f, grad; std::vector<int32_t> kf, level; std::vector<uint8_t> edge; int first = -1; };
static AddRecord g_add;
static int g_promoted_slot = -1;
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
  *n_promoted = 0;
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
  std::vector<FramePtr> kfs;
  FramePtr last;
  FramePtr stray;                              // a frame that is no keyframe of the map (a seed's keyframe that has left it)
  FramePtr newFrame() {
    std::vector<std::vector<uint8_t>> pyr(1, std::vector<uint8_t>((size_t)W * H, 7));
    return std::make_shared<Frame>(&cam, std::move(pyr));
  }
  World() {
    for (int k = 0; k < 2; ++k) kfs.push_back(newFrame());
    for (int p = 0; p < 6; ++p) {
      points.emplace_back(new Point(Vector3d{{0.1 * p, 0.2, 2.0}}));
      Feature* ftr = new Feature(kfs[(size_t)(p % 2)].get(), Vector2d{{5.0 + p, 6.0}}, Vector3d{{0.0, 0.0, 1.0}}, 0);
      ftr->point = points.back().get();
      points.back()->obs_.push_front(ftr);
      kfs[(size_t)(p % 2)]->addFeature(ftr);
    }
    for (FramePtr& kf : kfs) { kf->setKeyframe(); map.addKeyframe(kf); }
    stray = newFrame();
    addCandidate(kfs[0].get(), 1.0, false);
    last = kfs[1];
  }
  /// MapPointCandidates::newCandidatePoint for a seed of `frame` that converged
  Point* addCandidate(Frame* frame, double x, bool edgelet) {
    Feature* ftr = new Feature(frame, Vector2d{{x, x + 1.0}}, Vector3d{{x, 0.5, 1.0}}, 2);
    if (edgelet) { ftr->type = Feature::EDGELET; ftr->grad = Vector2d{{0.6, 0.8}}; }
    points.emplace_back(new Point(Vector3d{{x, -x, 3.0}}, ftr));
    ftr->point = points.back().get();
    points.back()->type_ = Point::TYPE_CANDIDATE;
    std::unique_lock<std::mutex> lock(map.point_candidates_.mut_);
    map.point_candidates_.candidates_.push_back(MapPointCandidates::PointCandidate(points.back().get(), ftr));
    return points.back().get();
  }
  /// one frame through the tracker; returns the frame
  FramePtr frame(FrameTracker& trk) {
    FramePtr cur = newFrame();
    std::vector<std::pair<FramePtr, size_t>> overlap;
    FrameTracker::Outcome oc;
    CHECK(trk.track(last, cur, map, overlap, oc));
    CHECK(cur->fts_.size() == 3 && overlap.size() == 1 && overlap[0].first == kfs[0]);
    last = cur;
    return cur;
  }
  /// processFrame :267-276 + map_.addKeyframe on the objects
  void makeKeyframe(const FramePtr& cur) {
    cur->setKeyframe();
    for (Feature* ftr : cur->fts_) if (ftr->point != nullptr) ftr->point->addFrameRef(ftr);
    map.point_candidates_.addCandidatePointToFrame(cur);
    map.addKeyframe(cur);
    kfs.push_back(cur);
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

// the mode off: today's sequence of calls
static void test_default_mode() {
  World w;
  FrameTracker trk(w.cam, config());
  CHECK(trk.ok() && !trk.incrementalMap());
  w.frame(trk);
  CALLS("upload_keyframe upload_keyframe set_map set_last_frame track");
  CHECK(g_last_map.n_kf == 2 && g_last_map.n_points == 7 && g_last_map.n_candidates == 1);
  w.frame(trk);
  CALLS("track");
  w.addCandidate(w.kfs[1].get(), 2.0, false);
  w.frame(trk);
  CALLS("set_map set_last_frame track");                                        // one new candidate: the whole map again, and the last frame
  CHECK(g_last_map.n_points == 8 && g_last_map.n_candidates == 2 && trk.mapUploads() == 2);
  FramePtr cur = w.frame(trk);
  CALLS("track");
  w.makeKeyframe(cur);
  CHECK(trk.lastFrameBecameKeyframe(*cur));
  CALLS("keyframe_from_last_frame");
  w.frame(trk);
  CALLS("set_map set_last_frame track");
  CHECK(g_last_map.n_kf == 3 && trk.mapUploads() == 3);
  // the overload that takes the map does the same while the mode is off
  cur = w.frame(trk);
  w.makeKeyframe(cur);
  CHECK(trk.lastFrameBecameKeyframe(cur, w.map));
  w.frame(trk);
  CALLS("track keyframe_from_last_frame set_map set_last_frame track");
}

static void test_incremental_mode() {
  World w;
  FrameTracker trk(w.cam, config());
  trk.setIncrementalMap(true);
  w.frame(trk);
  CALLS("upload_keyframe upload_keyframe set_map set_last_frame track");
  // ---- the list grows by three: a corner of keyframe 1, an edgelet of keyframe 0, a seed whose keyframe the map no longer holds
  Point* a = w.addCandidate(w.kfs[1].get(), 2.0, false);
  Point* b = w.addCandidate(w.kfs[0].get(), 3.0, true);
  Point* c = w.addCandidate(w.stray.get(), 4.0, false);
  w.frame(trk);
  CALLS("add_candidates track");                                                // no set_map, no set_last_frame
  CHECK(trk.mapUploads() == 1);
  CHECK(g_add.first == 7 && g_add.kf == (std::vector<int32_t>{1, 0, -1}) && g_add.level == (std::vector<int32_t>{2, 2, 2}));
  CHECK(g_add.edge == (std::vector<uint8_t>{0, 1, 0}));
  CHECK(g_add.pos == (std::vector<double>{2.0, -2.0, 3.0, 3.0, -3.0, 3.0, 4.0, -4.0, 3.0}));
  CHECK(g_add.px == (std::vector<double>{2.0, 3.0, 3.0, 4.0, 4.0, 5.0}));
  CHECK(g_add.f == (std::vector<double>{2.0, 0.5, 1.0, 3.0, 0.5, 1.0, 4.0, 0.5, 1.0}));
  CHECK(g_add.grad == (std::vector<double>{1.0, 0.0, 0.6, 0.8, 1.0, 0.0}));
  CHECK(a->type_ == Point::TYPE_CANDIDATE && b->type_ == Point::TYPE_CANDIDATE && c->type_ == Point::TYPE_CANDIDATE);   // (apply reached the new points)
  w.frame(trk);
  CALLS("track");                                                               // the list is as long as the tables know it
  // ---- the tracked frame becomes a keyframe
  FramePtr cur = w.frame(trk);
  w.makeKeyframe(cur);
  CHECK(trk.lastFrameBecameKeyframe(cur, w.map));
  CALLS("track promote_last_frame");
  CHECK(g_promoted_slot == 2);                                                  // the lowest slot no keyframe holds
  cur = w.frame(trk);
  CALLS("track");
  CHECK(trk.mapUploads() == 1);
  // a candidate of the promoted keyframe's own: its index in the tables is known
  w.addCandidate(w.kfs[2].get(), 5.0, false);
  w.frame(trk);
  CALLS("add_candidates track");
  CHECK(g_add.first == 10 && g_add.kf == (std::vector<int32_t>{2}));
  // ---- a refused append: one full upload follows, the frame is not lost
  g_fail_add = true;
  w.addCandidate(w.kfs[0].get(), 6.0, false);
  w.frame(trk);
  CALLS("add_candidates set_map set_last_frame track");
  CHECK(trk.mapUploads() == 2 && g_last_map.n_kf == 3 && g_last_map.n_candidates == 6);
  g_fail_add = false;
  w.frame(trk);
  CALLS("track");
  // ---- a refused promotion: the pyramid is kept the old way and the next frame flattens the map
  g_fail_promote = true;
  cur = w.frame(trk);
  w.makeKeyframe(cur);
  CHECK(trk.lastFrameBecameKeyframe(cur, w.map));
  CALLS("track promote_last_frame keyframe_from_last_frame");
  w.frame(trk);
  CALLS("set_map set_last_frame track");
  CHECK(trk.mapUploads() == 3 && g_last_map.n_kf == 4);
  g_fail_promote = false;
  // ---- a list that SHRANK behind the tracker's back is no append
  w.map.point_candidates_.deleteCandidatePoint(a);
  w.frame(trk);
  CALLS("set_map set_last_frame track");
  // ---- something else dirty: the promotion waits for the upload too
  trk.mapChanged();
  cur = w.frame(trk);
  CALLS("set_map set_last_frame track");
  trk.mapChanged();
  w.makeKeyframe(cur);
  CHECK(trk.lastFrameBecameKeyframe(cur, w.map));
  CALLS("keyframe_from_last_frame");
}

int main() {
  test_default_mode();
  test_incremental_mode();
  std::printf("tracker mock test OK\n");
  return 0;
}
