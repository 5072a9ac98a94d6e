// CPU-only test of hip_bridge::FrameTrackerT::finishFrame (include/svo_dropin/frame_tracker_batch.h) against a MOCK of the
// svo_hip_tracker_* entry points that records every call, as its siblings under tests/host_mock/ do for the other bridge calls.
// Checked: the structure step and the decision are ONE device call and svo_hip_tracker_optimize_structure is not called; the
// positions and Point::last_structure_optim_ are applied as optimiseStructure applies them; the furthest keyframe's index is
// translated through the tracker's own keyframe list, before and after a keyframeRemoved; need_new_kf = -1 surfaces as
// overlap_valid == false; a refused device call returns false with the host's objects untouched.  Built and run by
// tests/test_tracker_bridge_decision_mock.py, plain and with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "svo_hip.h"
#include "../../android_svo_amd/host/svo_host.h"

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

// ---------------------------------------------------------------- mock device
struct svo_hip_ctx { int unused; };
struct svo_hip_tracker {
  std::vector<int32_t> type;
  int n_kf = 0;
  std::vector<uint8_t> image;
};
static std::vector<std::string> g_calls;
static svo_hip_kf_decision g_decision;           // what the device reports
static bool g_refuse = false;                    // the device refuses svo_hip_tracker_finish_frame
static std::vector<int32_t> g_points;            // the selection of the last call
static int g_n_iter = -1;
static double g_min_dist = -1.0;

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
  t->n_kf = m->n_kf;
  return SVO_HIP_OK;
}
int svo_hip_tracker_update_point_positions(svo_hip_tracker*, int, const int32_t*, const double*) { g_calls.push_back("update_point_positions"); return SVO_HIP_OK; }
int svo_hip_tracker_optimize_structure(svo_hip_tracker*, int, const int32_t*, int, double*, int32_t*) { g_calls.push_back("optimize_structure"); return SVO_HIP_OK; }
int svo_hip_tracker_set_last_frame(svo_hip_tracker*, const uint8_t*, int, const double*, int, const double*, const double*, const int32_t*) {
  g_calls.push_back("set_last_frame");
  return SVO_HIP_OK;
}
int svo_hip_tracker_add_candidates(svo_hip_tracker*, int, const double*, const int32_t*, const double*, const double*, const int32_t*, const uint8_t*,
                                   const double*, int32_t*) { g_calls.push_back("add_candidates"); return SVO_HIP_ERR_INVALID; }
int svo_hip_tracker_promote_last_frame(svo_hip_tracker*, int, int*, int*) { g_calls.push_back("promote_last_frame"); return SVO_HIP_ERR_INVALID; }
// the keyframe holds nothing in this test: its slot is its index (slots were handed out in map order), nothing is deleted
int svo_hip_tracker_remove_keyframe(svo_hip_tracker* t, int k, int* slot, int* n_points, int* n_cands) {
  g_calls.push_back("remove_keyframe");
  if (k < 0 || k >= t->n_kf) return SVO_HIP_ERR_INVALID;
  *slot = k; *n_points = 0; *n_cands = 0;
  t->n_kf -= 1;
  return SVO_HIP_OK;
}
int svo_hip_tracker_track(svo_hip_tracker* t, const uint8_t*, svo_hip_track_result* r, double* px, double* f, int32_t* level, int32_t* point, uint8_t* edge,
                          double* grad, int32_t* pt_type, int32_t* pt_failed, int32_t* pt_succ) {
  g_calls.push_back("track");
  std::memset(r, 0, sizeof(*r));
  r->T_f_w[0] = -1.25; r->T_f_w[6] = 1.0;
  r->n_features = 4; r->n_matches = 4; r->n_overlap = 1; r->overlap_kf[0] = 0; r->overlap_count[0] = 4; r->sia_n_tracked = 4;
  for (int i = 0; i < 4; ++i) {
    px[2 * i] = 10.0 + i; px[2 * i + 1] = 12.0; f[3 * i] = 0.0; f[3 * i + 1] = 0.0; f[3 * i + 2] = 1.0;
    level[i] = 0; point[i] = i == 3 ? -1 : 2 * i; edge[i] = 0; grad[2 * i] = 1.0; grad[2 * i + 1] = 0.0;     // points 0, 2, 4 and a feature without one
  }
  for (size_t p = 0; p < t->type.size(); ++p) { pt_type[p] = t->type[p]; pt_failed[p] = 0; pt_succ[p] = 0; }
  return SVO_HIP_OK;
}
// svo_hip_tracker_finish_frame as include/svo_hip.h states it, on made-up numbers: point p moves to (100 + p, 200 + p, 300 + p)
int svo_hip_tracker_finish_frame(svo_hip_tracker* t, int n, const int32_t* point, int n_iter, double* pos_out, int32_t* iters_out, double min_dist,
                                 svo_hip_kf_decision* decision) {
  g_calls.push_back("finish_frame");
  g_points.assign(point, point + n);
  g_n_iter = n_iter; g_min_dist = min_dist;
  if (g_refuse || !decision || n > 64 || !(min_dist >= 0.0)) return SVO_HIP_ERR_INVALID;
  for (int i = 0; i < n; ++i) {
    if (point[i] < 0 || point[i] >= (int)t->type.size()) return SVO_HIP_ERR_INVALID;
    for (int k = 0; k < 3; ++k) pos_out[3 * i + k] = 100.0 * (k + 1) + point[i];
    if (iters_out) iters_out[i] = n_iter;
  }
  *decision = g_decision;
  return SVO_HIP_OK;
}
int svo_hip_tracker_last_result(svo_hip_tracker*, svo_hip_track_result*, double*, double*, int32_t*, int32_t*, uint8_t*, double*, int32_t*, int32_t*,
                                int32_t*) { return SVO_HIP_ERR_STATE; }
int svo_hip_tracker_default_config(svo_hip_tracker_config* c) {
  std::memset(c, 0, sizeof(*c));
  c->max_keyframes = 8; c->max_frame_features = 16; c->max_points = 64;
  return SVO_HIP_OK;
}
}  // extern "C"

// ---------------------------------------------------------------- a small world on the twins
using namespace svo;
static const int W = 32, H = 24;

static std::string take() {
  std::string s;
  for (const std::string& c : g_calls) s += (s.empty() ? "" : " ") + c;
  g_calls.clear();
  return s;
}
#define CALLS(expected) do { const std::string got_ = take(); if (got_ != (expected)) { \
  std::fprintf(stderr, "line %d: calls were [%s], expected [%s]\n", __LINE__, got_.c_str(), (expected)); std::exit(1); } } while (0)

// three keyframes in map order: A sees the even points, E sees nothing, B the odd ones
struct World {
  PinholeCamera cam{W, H, 30.0, 30.0, 16.0, 12.0};
  Map map;
  std::vector<std::unique_ptr<Point>> points;
  FramePtr A, E, B, last;
  FramePtr newFrame(double x) {
    std::vector<std::vector<uint8_t>> pyr(1, std::vector<uint8_t>((size_t)W * H, 7));
    FramePtr f = std::make_shared<Frame>(&cam, std::move(pyr));
    const double T[7] = {-x, 0, 0, 0, 0, 0, 1};
    f->T_f_w_ = SE3(T);
    return f;
  }
  World() {
    A = newFrame(0.0); E = newFrame(0.5); B = newFrame(1.0);
    for (int p = 0; p < 6; ++p) {                                                  // table order of the flatten: 0, 2, 4 (A's row), then 1, 3, 5
      points.emplace_back(new Point(Vector3d{{0.1 * p, 0.2, 2.0}}));
      observe(p % 2 == 0 ? A : B, p);
    }
    for (const FramePtr& kf : {A, E, B}) { kf->setKeyframe(); map.addKeyframe(kf); }
    last = B;
  }
  void observe(const FramePtr& kf, int p) {
    Feature* ftr = new Feature(kf.get(), Vector2d{{5.0 + p, 6.0}}, Vector3d{{0.0, 0.0, 1.0}}, 0);
    ftr->point = points[(size_t)p].get();
    ftr->point->addFrameRef(ftr);
    kf->addFeature(ftr);
  }
};

static svo_hip_kf_decision decision(int need, int furthest) {
  svo_hip_kf_decision d;
  std::memset(&d, 0, sizeof(d));
  d.n_depths = 3; d.depth_mean = 2.5; d.depth_min = 1.75; d.overlap_valid = need >= 0 ? 1 : 0; d.need_new_kf = need; d.blocking_kf = need == 0 ? 0 : -1;
  d.furthest_kf = furthest; d.furthest_distance = furthest >= 0 ? 3.0 : 0.0;
  return d;
}

int main() {
  World w;
  svo_hip_tracker_config cfg;
  svo_hip_tracker_default_config(&cfg);
  FrameTracker trk(w.cam, cfg);
  trk.setIncrementalMap(true);
  // ---- one tracked frame: the mock matches the table's points 0, 2, 4 (the world's points 0, 4 and 3: rows are 0 2 4 | 1 3 5)
  FramePtr cur = w.newFrame(1.5);
  std::vector<std::pair<FramePtr, size_t>> overlap;
  FrameTracker::Outcome oc;
  CHECK(trk.track(w.last, cur, w.map, overlap, oc));
  CALLS("upload_keyframe upload_keyframe upload_keyframe set_map set_last_frame track");
  CHECK(cur->fts_.size() == 4 && overlap.size() == 1 && overlap[0].first == w.A);
  std::vector<Point*> seen;
  for (Feature* f : cur->fts_) if (f->point) seen.push_back(f->point);
  CHECK(seen.size() == 3);
  // ---- the structure step and the decision: ONE device call, no optimize_structure; two of the three points are selected
  seen[1]->last_structure_optim_ = 7;                                              // optimised more recently than the other two
  const Vector3d kept = seen[1]->pos_;
  g_decision = decision(1, 2);
  FrameTracker::Decision dec;
  CHECK(trk.finishFrame(cur, w.map, 2, 5, 0.125, dec));
  CALLS("finish_frame");
  CHECK(trk.deviceDecisions() == 1 && g_points.size() == 2 && g_n_iter == 5 && g_min_dist == 0.125);
  CHECK(dec.have_depth && dec.depth_mean == 2.5 && dec.depth_min == 1.75 && dec.overlap_valid && dec.need_new_kf);
  CHECK(dec.furthest == w.B);                                                      // keyframe index 2 of A, E, B
  for (int i = 0; i < 2; ++i) {
    Point* pt = seen[i == 0 ? 0 : 2];
    bool found = false;
    for (int32_t p : g_points) found = found || (pt->pos_[0] == 100.0 + p && pt->pos_[1] == 200.0 + p && pt->pos_[2] == 300.0 + p);
    CHECK(found && pt->last_structure_optim_ == cur->id_);
  }
  CHECK(seen[1]->last_structure_optim_ == 7 && seen[1]->pos_[0] == kept[0] && seen[1]->pos_[2] == kept[2]);
  // ---- needNewKf says no; no furthest keyframe
  g_decision = decision(0, -1);
  CHECK(trk.finishFrame(cur, w.map, 0, 5, 0.125, dec));
  CALLS("finish_frame");
  CHECK(g_points.empty() && dec.overlap_valid && !dec.need_new_kf && dec.furthest == nullptr && trk.deviceDecisions() == 2);
  // ---- need_new_kf = -1: no answer
  g_decision = decision(-1, 0);
  CHECK(trk.finishFrame(cur, w.map, 0, 5, 0.125, dec));
  CALLS("finish_frame");
  CHECK(!dec.overlap_valid && !dec.need_new_kf && dec.furthest == w.A && dec.raw.need_new_kf == -1);
  // ---- a frame without depths
  g_decision = decision(1, 0);
  g_decision.n_depths = 0; g_decision.depth_mean = std::numeric_limits<double>::quiet_NaN(); g_decision.depth_min = std::numeric_limits<double>::max();
  CHECK(trk.finishFrame(cur, w.map, 0, 5, 0.125, dec) && !dec.have_depth);
  CALLS("finish_frame");
  // ---- the device refuses: false, the objects untouched, the host path is the caller's
  g_refuse = true;
  const int optim_before = seen[0]->last_structure_optim_;
  const Vector3d pos_before = seen[0]->pos_;
  seen[0]->last_structure_optim_ = -5;                                             // (the oldest: it would be selected)
  FrameTracker::Decision untouched = dec;
  CHECK(!trk.finishFrame(cur, w.map, 1, 5, 0.125, dec));
  CALLS("finish_frame");
  CHECK(seen[0]->last_structure_optim_ == -5 && seen[0]->pos_[0] == pos_before[0] && seen[0]->pos_[1] == pos_before[1] && trk.deviceDecisions() == 4);
  CHECK(dec.furthest == untouched.furthest && dec.have_depth == untouched.have_depth);
  seen[0]->last_structure_optim_ = optim_before;
  g_refuse = false;
  // ---- a keyframe leaves: index 1 names B afterwards, and 2 is no keyframe any more
  CHECK(w.map.safeDeleteFrame(w.E));
  CHECK(trk.keyframeRemoved(w.E, w.map));
  CALLS("remove_keyframe");
  g_decision = decision(1, 1);
  CHECK(trk.finishFrame(cur, w.map, 0, 5, 0.125, dec) && dec.furthest == w.B);
  g_decision = decision(1, 0);
  CHECK(trk.finishFrame(cur, w.map, 0, 5, 0.125, dec) && dec.furthest == w.A);
  g_decision = decision(1, 2);
  CHECK(!trk.finishFrame(cur, w.map, 0, 5, 0.125, dec));                           // an index the tracker's list does not hold
  CALLS("finish_frame finish_frame finish_frame");
  CHECK(trk.mapUploads() == 1);
  // ---- a map that changed behind the tracker is flattened first; the device's last frame is gone with it: the host path
  trk.mapChanged();
  CHECK(!trk.finishFrame(cur, w.map, 1, 5, 0.125, dec));
  CALLS("set_map");
  std::printf("tracker decision mock test OK\n");
  return 0;
}
