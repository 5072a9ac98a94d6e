// CPU-only test of hip_bridge::FrameTrackerT::relocalize / setDeviceRelocalisation (include/svo_dropin/frame_tracker_batch.h)
// against a MOCK of the svo_hip_tracker_* entry points that records every call, as tests/host_mock/tracker_compact_mock_test.cpp
// does for the compaction.  Checked: an accepted relocalisation makes one device call, no upload, and leaves the frame's outcome
// on the host's objects; a refused gate leaves the gate's pose on the new frame and the next frame uploads no last frame; no close
// keyframe changes nothing; a keyframe given by the caller is passed by its index, the excluded one too; a refusal of the device
// ends in the upload of the keyframe as last frame, as before; with the switch off the new entry point is never called.  Built
// and run by tests/test_tracker_bridge_reloc_mock.py, plain and with -fsanitize=address,undefined.
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
  std::vector<int32_t> type;
  int n_kf = 0;
  std::vector<uint8_t> image;
};
static std::vector<std::string> g_calls;
static int g_closest = 1;                        // the keyframe the device finds closest (-1: none is close)
static uint64_t g_gate_tracked = 50;             // what the gate's SparseImgAlign tracks
static bool g_fail_reloc = false;                // the device refuses the call
static int g_kf_arg = -9, g_excl_arg = -9, g_min_arg = -9;
static double g_init_arg[7];
static int g_last_n = -1;                        // features of the last upload of a last frame
static svo_hip_tracker_map g_last_map;           // the scalars of the last upload (its pointers are stale)

static void fill_frame(svo_hip_tracker* t, svo_hip_track_result* r, double* px, double* f, int32_t* level, int32_t* point, uint8_t* edge, double* grad,
                       int32_t* pt_type, int32_t* pt_failed, int32_t* pt_succ) {
  std::memset(r, 0, sizeof(*r));
  r->T_f_w[0] = -1.25; r->T_f_w[6] = 1.0;
  r->n_features = 3; r->n_matches = 3; r->n_overlap = 1; r->overlap_kf[0] = 0; r->overlap_count[0] = 3; r->sia_n_tracked = 3;
  for (int i = 0; i < 3; ++i) {
    px[2 * i] = 10.0 + i; px[2 * i + 1] = 12.0; f[3 * i] = 0.0; f[3 * i + 1] = 0.0; f[3 * i + 2] = 1.0;
    level[i] = 0; point[i] = i; edge[i] = 0; grad[2 * i] = 1.0; grad[2 * i + 1] = 0.0;
  }
  for (size_t p = 0; p < t->type.size(); ++p) { pt_type[p] = t->type[p]; pt_failed[p] = 0; pt_succ[p] = 0; }
}

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
  g_last_map = *m;
  return SVO_HIP_OK;
}
int svo_hip_tracker_update_point_positions(svo_hip_tracker*, int, const int32_t*, const double*) { g_calls.push_back("update_point_positions"); return SVO_HIP_OK; }
int svo_hip_tracker_optimize_structure(svo_hip_tracker*, int, const int32_t*, int, double*, int32_t*) { g_calls.push_back("optimize_structure"); return SVO_HIP_OK; }
int svo_hip_tracker_set_last_frame(svo_hip_tracker*, const uint8_t*, int, const double*, int n, const double*, const double*, const int32_t*) {
  g_calls.push_back("set_last_frame");
  g_last_n = n;
  return SVO_HIP_OK;
}
int svo_hip_tracker_add_candidates(svo_hip_tracker*, int, const double*, const int32_t*, const double*, const double*, const int32_t*, const uint8_t*,
                                   const double*, int32_t*) { g_calls.push_back("add_candidates"); return SVO_HIP_ERR_INVALID; }
int svo_hip_tracker_promote_last_frame(svo_hip_tracker*, int, int*, int*) { g_calls.push_back("promote_last_frame"); return SVO_HIP_ERR_INVALID; }
int svo_hip_tracker_remove_keyframe(svo_hip_tracker*, int, int*, int*, int*) { g_calls.push_back("remove_keyframe"); return SVO_HIP_ERR_INVALID; }
int svo_hip_tracker_compact_points(svo_hip_tracker*, int*, int32_t*) { g_calls.push_back("compact_points"); return SVO_HIP_ERR_STATE; }
int svo_hip_tracker_track(svo_hip_tracker* t, const uint8_t*, svo_hip_track_result* r, double* px, double* f, int32_t* level, int32_t* point, uint8_t* edge,
                          double* grad, int32_t* pt_type, int32_t* pt_failed, int32_t* pt_succ) {
  g_calls.push_back("track");
  fill_frame(t, r, px, f, level, point, edge, grad, pt_type, pt_failed, pt_succ);
  return SVO_HIP_OK;
}
// svo_hip_tracker_relocalize as include/svo_hip.h states it: the keyframe given or g_closest (unless excluded), the gate against
// min_tracked, the frame's outcome only when the gate accepted
int svo_hip_tracker_relocalize(svo_hip_tracker* t, const uint8_t* level0, int kf_index, int exclude_kf, const double* T_init, int min_tracked,
                               svo_hip_reloc_result* rel, svo_hip_track_result* r, double* px, double* f, int32_t* level, int32_t* point, uint8_t* edge,
                               double* grad, int32_t* pt_type, int32_t* pt_failed, int32_t* pt_succ) {
  g_calls.push_back("relocalize");
  g_kf_arg = kf_index; g_excl_arg = exclude_kf; g_min_arg = min_tracked;
  if (g_fail_reloc) return SVO_HIP_ERR_INVALID;
  if (!level0 || !rel || !T_init || kf_index >= t->n_kf) return SVO_HIP_ERR_INVALID;
  std::memcpy(g_init_arg, T_init, sizeof(g_init_arg));
  std::memset(rel, 0, sizeof(*rel));
  rel->kf_index = kf_index >= 0 ? kf_index : (g_closest == exclude_kf ? -1 : g_closest);
  rel->n_close = kf_index >= 0 ? 0 : (g_closest >= 0 ? 1 : 0);
  if (rel->kf_index < 0) return SVO_HIP_OK;
  rel->gate_n_tracked = g_gate_tracked;
  rel->T_f_w_gate[0] = -7.5; rel->T_f_w_gate[6] = 1.0;
  if (g_gate_tracked <= (uint64_t)min_tracked) return SVO_HIP_OK;
  rel->accepted = 1;
  fill_frame(t, r, px, f, level, point, edge, grad, pt_type, pt_failed, pt_succ);
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


static void pose_of(const FramePtr& f, double T[7]) { HostTrackerPolicy::pose7(*f, T); }

struct Reloc {
  bool ok, accepted;
  FramePtr ref, cur;
  std::vector<std::pair<FramePtr, size_t>> overlap;
  FrameTracker::Outcome oc;
};
static Reloc relocalise(World& w, FrameTracker& trk, const FramePtr& ref, int min_tracked = 30, const FramePtr& exclude = FramePtr()) {
  Reloc r;
  r.cur = w.newFrame(2.0);
  double T[7];
  pose_of(w.last, T);
  r.accepted = true;
  r.ref = w.kfs[0];
  r.ok = trk.relocalize(ref, T, r.cur, w.map, r.overlap, r.oc, &r.accepted, &r.ref, min_tracked, exclude);
  return r;
}

// the first frame uploads the map (two keyframes, eight points) and the last frame
static void start(World& w, FrameTracker& trk) {
  w.frame(trk, w.kfs[0], 1.5);
  CALLS("upload_keyframe upload_keyframe set_map set_last_frame track");
  CHECK(trk.mapUploads() == 1 && g_last_map.n_kf == 2);
}

static void test_switch_on() {
  World w;
  FrameTracker trk(w.cam, config());
  CHECK(!trk.deviceRelocalisation());
  trk.setDeviceRelocalisation(true);
  CHECK(trk.deviceRelocalisation());
  start(w, trk);
  // ---- accepted, the device chooses: one call, no upload, the outcome on the host's objects
  g_closest = 1; g_gate_tracked = 50;
  Reloc r = relocalise(w, trk, FramePtr());
  CALLS("relocalize");
  CHECK(r.ok && r.accepted && r.ref == w.kfs[1] && g_kf_arg == -1 && g_excl_arg == -1 && g_min_arg == 30);
  double T[7];
  pose_of(w.last, T);
  CHECK(std::memcmp(T, g_init_arg, sizeof(T)) == 0);                            // T_f_w_init = last_frame_->T_f_w_
  CHECK(r.cur->fts_.size() == 3 && r.overlap.size() == 1 && r.overlap[0].first == w.kfs[0] && r.oc.repr_n_matches == 3);
  pose_of(r.cur, T);
  CHECK(T[0] == -1.25);
  CHECK(trk.deviceRelocalisations() == 1 && trk.lastRelocalisation().gate_n_tracked == 50 && trk.mapUploads() == 1);
  w.last = r.cur;                                                               // addImage: last_frame_ = new_frame_
  w.frame(trk, w.kfs[0], 2.1);
  CALLS("track");                                                               // the device handed the frame over to itself
  // ---- the keyframe given by the caller goes by its index; so does the excluded one
  r = relocalise(w, trk, w.kfs[0], 40, w.kfs[1]);
  CALLS("relocalize");
  CHECK(r.ok && r.accepted && r.ref == w.kfs[0] && g_kf_arg == 0 && g_excl_arg == 1 && g_min_arg == 40);
  r = relocalise(w, trk, FramePtr(), 30, w.kfs[1]);                             // the closest one is the excluded one: none is left
  CALLS("relocalize");
  CHECK(r.ok && !r.accepted && r.ref == nullptr && r.cur->fts_.empty());
  // ---- the gate refuses: the gate's pose on the new frame, nothing else; the next frame uploads nothing
  g_gate_tracked = 30;
  r = relocalise(w, trk, FramePtr());
  CALLS("relocalize");
  CHECK(r.ok && !r.accepted && r.ref == w.kfs[1] && r.cur->fts_.empty() && r.overlap.empty());
  pose_of(r.cur, T);
  CHECK(T[0] == -7.5);
  w.last = r.cur;
  w.frame(trk, w.kfs[0], 2.2);
  CALLS("track");
  CHECK(trk.mapUploads() == 1);
  // ---- no keyframe is close: nothing changes, on either side
  g_closest = -1; g_gate_tracked = 50;
  FramePtr last = w.last;
  double before[7];
  r = relocalise(w, trk, FramePtr());
  CALLS("relocalize");
  pose_of(r.cur, T);
  pose_of(w.newFrame(2.0), before);
  CHECK(r.ok && !r.accepted && r.ref == nullptr && r.cur->fts_.empty() && std::memcmp(T, before, sizeof(T)) == 0);
  w.frame(trk, w.kfs[0], 2.3);
  CALLS("track");                                                               // the device's last frame was kept
  // ---- the device refuses: the keyframe goes up as last frame and the frame is tracked from it, as before
  g_closest = 1; g_fail_reloc = true;
  r = relocalise(w, trk, w.kfs[1]);
  CALLS("relocalize set_last_frame track");
  CHECK(r.ok && r.accepted && r.ref == w.kfs[1] && r.cur->fts_.size() == 3 && g_last_n == (int)w.kfs[1]->fts_.size());
  r = relocalise(w, trk, FramePtr());                                           // ... which needs a keyframe to start from
  CALLS("relocalize");
  CHECK(!r.ok && !r.accepted && r.ref == nullptr);
  g_fail_reloc = false;
  // ---- a keyframe the tables do not hold: the old path, without asking the device
  FramePtr stranger = w.newFrame(3.0);
  w.observe(stranger, 0);
  r = relocalise(w, trk, stranger);
  CALLS("set_last_frame track");
  CHECK(r.ok && r.accepted && r.ref == stranger && g_last_n == 1);
  // ---- a map that changed is flattened before the device looks at it
  trk.mapChanged();
  r = relocalise(w, trk, FramePtr());
  CALLS("set_map relocalize");
  CHECK(r.ok && r.accepted && trk.mapUploads() == 2 && trk.deviceRelocalisations() == 6);
}

static void test_switch_off() {
  World w;
  FrameTracker trk(w.cam, config());
  start(w, trk);
  Reloc r = relocalise(w, trk, w.kfs[1]);
  CALLS("set_last_frame track");                                                // no new entry point is called
  CHECK(r.ok && r.accepted && r.ref == w.kfs[1] && r.cur->fts_.size() == 3 && trk.deviceRelocalisations() == 0);
  r = relocalise(w, trk, FramePtr());
  CALLS("");
  CHECK(!r.ok && !r.accepted && r.ref == nullptr);
  w.frame(trk, w.kfs[0], 2.5);
  CALLS("set_last_frame track");                                                // (lastFrameChanged: the last frame goes up again)
}

int main() {
  test_switch_on();
  test_switch_off();
  std::printf("tracker relocalisation mock test OK\n");
  return 0;
}
