// CPU-only test of hip_bridge::FrameTrackerGroupT::trackSome (include/svo_dropin/frame_tracker_batch.h) on the twins of
// android_svo_amd/host/svo_host.h against a MOCK device: the mock tracker and the small world of tests/host_mock/tracker_mock_test.cpp,
// reused by inclusion, plus the group entry points defined below, which RECORD what they were given.  What is checked:
//   1. trackSome makes exactly ONE svo_hip_tracker_group_track_some call, with the active list and the images in its order
//      (image j is level 0 of the new frame of camera active[j]), and never svo_hip_tracker_group_track;
//   2. prepare (the map upload of a camera's first frame), fetch and apply run on the cameras of the call only: a camera that sits
//      out gets no device call at all, its fresh frame gains no feature, and its entries of `out` and `overlap_kfs` keep the
//      sentinels put there; entries of last / fresh / maps of such cameras may be null;
//   3. a camera that joins later is prepared then (its uploads happen in that call), the full list goes through the same entry,
//      an empty list makes the call with n_active = 0, a bad list or a refusal of the device returns false and applies nothing.
// Built plain (g++ -std=c++17) and with -fsanitize=address,undefined by tests/test_host_group_subset_mock.py.
#include <memory>
#include <string>

#include "svo_hip.h"
#include "../../android_svo_amd/host/svo_host.h"

// the lone-tracker mock answers svo_hip_tracker_last_result with SVO_HIP_ERR_STATE; a group's cameras read their frames through it
#define svo_hip_tracker_last_result lone_mock_last_result
#define main tracker_mock_main
#include "../host_mock/tracker_mock_test.cpp"
#undef main
#undef svo_hip_tracker_last_result

struct GroupCall { int n; std::vector<int32_t> camera; std::vector<const uint8_t*> image; };
static std::vector<GroupCall> g_group_calls;
static int g_full_calls = 0, g_fetches = 0;
static bool g_refuse = false;
static std::vector<int> g_fetched;                   // the cameras whose result block was read, in order

struct svo_hip_tracker_group { std::vector<svo_hip_tracker*> members; };
static svo_hip_tracker_group* g_group = nullptr;

extern "C" {
int svo_hip_tracker_group_create(svo_hip_ctx*, const svo_hip_camera* cam, const svo_hip_tracker_config*, int n, svo_hip_tracker_group** out) {
  svo_hip_tracker_group* g = new svo_hip_tracker_group();
  for (int k = 0; k < n; ++k) {
    g->members.push_back(new svo_hip_tracker());
    g->members.back()->image.resize((size_t)cam->width * cam->height);
  }
  g_group = g;
  *out = g;
  return SVO_HIP_OK;
}
int svo_hip_tracker_group_create_rig(svo_hip_ctx* c, const svo_hip_camera* cams, const svo_hip_tracker_config* cfg, int n, svo_hip_tracker_group** out) {
  return svo_hip_tracker_group_create(c, cams, cfg, n, out);
}
int svo_hip_tracker_group_destroy(svo_hip_tracker_group* g) {
  for (svo_hip_tracker* t : g->members) delete t;
  delete g;
  g_group = nullptr;
  return SVO_HIP_OK;
}
int svo_hip_tracker_group_camera(svo_hip_tracker_group* g, int index, svo_hip_tracker** camera) { *camera = g->members[(size_t)index]; return SVO_HIP_OK; }
int svo_hip_tracker_group_track(svo_hip_tracker_group*, const uint8_t* const*, svo_hip_track_result*) { ++g_full_calls; return SVO_HIP_ERR_STATE; }
int svo_hip_tracker_group_track_some(svo_hip_tracker_group* g, int n_active, const int32_t* camera, const uint8_t* const* level0,
                                     svo_hip_track_result* results) {
  g_calls.push_back("group_track_some");
  GroupCall c;
  c.n = n_active;
  for (int j = 0; j < n_active; ++j) { c.camera.push_back(camera[j]); c.image.push_back(level0[j]); }
  g_group_calls.push_back(c);
  if (g_refuse) return SVO_HIP_ERR_STATE;
  for (int j = 0; j < n_active; ++j) {
    std::memset(&results[j], 0, sizeof(results[j]));
    results[j].T_f_w[6] = 1.0; results[j].T_f_w[0] = 100.0 + camera[j];          // (which camera the record belongs to)
    results[j].n_features = 3; results[j].n_matches = 3; results[j].n_overlap = 1; results[j].overlap_kf[0] = 0; results[j].overlap_count[0] = 3;
    g->members[(size_t)camera[j]]->frame_features = 3;
  }
  return SVO_HIP_OK;
}
// a camera's frame as the lone mock's svo_hip_tracker_track leaves it: three features on the first three points
int svo_hip_tracker_last_result(svo_hip_tracker* t, svo_hip_track_result* r, double* px, double* f, int32_t* level, int32_t* point, uint8_t* edge,
                                double* grad, int32_t* pt_type, int32_t* pt_failed, int32_t* pt_succ) {
  ++g_fetches;
  for (size_t k = 0; g_group && k < g_group->members.size(); ++k) if (g_group->members[k] == t) g_fetched.push_back((int)k);
  if (t->frame_features != 3) return SVO_HIP_ERR_STATE;
  (void)r;                                            // (the record comes from the group call)
  for (int i = 0; i < 3; ++i) {
    px[2 * i] = 10.0 + i; px[2 * i + 1] = 12.0; f[3 * i] = 0.0; f[3 * i + 1] = 0.0; f[3 * i + 2] = 1.0;
    level[i] = 0; point[i] = i; edge[i] = 0; grad[2 * i] = 1.0; grad[2 * i + 1] = 0.0;
  }
  for (size_t p = 0; p < t->type.size(); ++p) { pt_type[p] = t->type[p]; pt_failed[p] = 0; pt_succ[p] = 0; }
  return SVO_HIP_OK;
}
}  // extern "C"

typedef FrameTrackerGroup Group;
typedef Group::Outcome Outcome;
typedef std::vector<std::vector<std::pair<FramePtr, size_t>>> Overlaps;

static const size_t SENTINEL = 4242;

// one frame of the cameras `active` of `worlds`; the entries of the others are null / sentinels and must stay so
static bool step(Group& grp, std::vector<World>& worlds, const std::vector<int>& active, Overlaps& overlap, std::vector<Outcome>& out,
                 std::vector<FramePtr>* fresh_out = nullptr) {
  const size_t n = worlds.size();
  std::vector<bool> in(n, false);
  for (int c : active) if (c >= 0 && (size_t)c < n) in[(size_t)c] = true;
  std::vector<FramePtr> last(n), fresh(n);
  std::vector<Map*> maps(n, nullptr);
  for (size_t c = 0; c < n; ++c) {
    if (!in[c]) continue;
    last[c] = worlds[c].last; fresh[c] = worlds[c].newFrame(); maps[c] = &worlds[c].map;
  }
  const bool ok = grp.trackSome(active, last, fresh, maps, overlap, out);
  for (size_t c = 0; c < n && ok; ++c) if (in[c]) worlds[c].last = fresh[c];
  if (fresh_out) *fresh_out = fresh;
  return ok;
}

static void fill_sentinels(const std::vector<World>& worlds, Overlaps& overlap, std::vector<Outcome>& out) {
  overlap.assign(worlds.size(), std::vector<std::pair<FramePtr, size_t>>(1, std::make_pair(FramePtr(), SENTINEL)));
  Outcome o = Outcome();
  o.repr_n_matches = SENTINEL;
  out.assign(worlds.size(), o);
}

static void test_track_some() {
  const int N = 4;
  std::vector<World> worlds(N);
  Group grp(worlds[0].cam, config(), N);
  CHECK(grp.ok() && grp.size() == (size_t)N);
  g_calls.clear();
  Overlaps overlap;
  std::vector<Outcome> out;
  std::vector<FramePtr> fresh;
  // ---- cameras 1 and 3: their uploads, ONE group call with the list and the images in order, nothing for cameras 0 and 2
  fill_sentinels(worlds, overlap, out);
  CHECK(step(grp, worlds, {1, 3}, overlap, out, &fresh));
  CALLS("upload_keyframe upload_keyframe set_map set_last_frame upload_keyframe upload_keyframe set_map set_last_frame group_track_some");
  CHECK(g_group_calls.size() == 1 && g_full_calls == 0);
  CHECK(g_group_calls[0].n == 2 && g_group_calls[0].camera == (std::vector<int32_t>{1, 3}));
  CHECK(g_group_calls[0].image[0] == fresh[1]->img_pyr_[0].data() && g_group_calls[0].image[1] == fresh[3]->img_pyr_[0].data());
  CHECK(g_fetched == (std::vector<int>{1, 3}));
  for (int c = 0; c < N; ++c) {
    const bool in = c == 1 || c == 3;
    CHECK(grp.camera((size_t)c).mapUploads() == (in ? 1u : 0u));
    if (in) {
      CHECK(fresh[(size_t)c]->fts_.size() == 3 && overlap[(size_t)c].size() == 1 && overlap[(size_t)c][0].first == worlds[(size_t)c].kfs[0]);
      CHECK(out[(size_t)c].repr_n_matches == 3);
    } else {
      CHECK(!fresh[(size_t)c] && overlap[(size_t)c].size() == 1 && overlap[(size_t)c][0].second == SENTINEL && out[(size_t)c].repr_n_matches == SENTINEL);
    }
  }
  // ---- camera 0 joins, camera 3 sits out: camera 0's uploads happen now, camera 1 has nothing to upload
  fill_sentinels(worlds, overlap, out);
  g_fetched.clear();
  CHECK(step(grp, worlds, {0, 1}, overlap, out, &fresh));
  CALLS("upload_keyframe upload_keyframe set_map set_last_frame group_track_some");
  CHECK(g_group_calls.size() == 2 && g_group_calls[1].camera == (std::vector<int32_t>{0, 1}) && g_fetched == (std::vector<int>{0, 1}));
  CHECK(fresh[0]->fts_.size() == 3 && fresh[1]->fts_.size() == 3 && !fresh[2] && !fresh[3]);
  CHECK(out[3].repr_n_matches == SENTINEL && overlap[3][0].second == SENTINEL && out[2].repr_n_matches == SENTINEL && out[0].repr_n_matches == 3);
  CHECK(grp.camera(2).mapUploads() == 0 && grp.camera(3).mapUploads() == 1);
  // ---- the full list: the same entry point, every camera; short vectors grow to the group's size
  overlap.clear(); out.clear();
  g_fetched.clear();
  CHECK(step(grp, worlds, {0, 1, 2, 3}, overlap, out, &fresh));
  CALLS("upload_keyframe upload_keyframe set_map set_last_frame group_track_some");              // (camera 2's first frame)
  CHECK(g_group_calls.size() == 3 && g_group_calls[2].n == 4 && g_full_calls == 0 && overlap.size() == 4 && out.size() == 4);
  for (int c = 0; c < N; ++c) CHECK(fresh[(size_t)c]->fts_.size() == 3 && out[(size_t)c].repr_n_matches == 3);
  // ---- nobody: the call is made with n_active = 0 and touches nothing
  fill_sentinels(worlds, overlap, out);
  CHECK(step(grp, worlds, {}, overlap, out));
  CALLS("group_track_some");
  CHECK(g_group_calls.back().n == 0);
  for (int c = 0; c < N; ++c) CHECK(out[(size_t)c].repr_n_matches == SENTINEL);
  // ---- lists the bridge itself turns down: no device call
  const size_t calls = g_group_calls.size();
  g_fetches = 0;
  CHECK(!step(grp, worlds, {2, 1}, overlap, out) && !step(grp, worlds, {1, 1}, overlap, out) && !step(grp, worlds, {4}, overlap, out) &&
        !step(grp, worlds, {-1}, overlap, out));
  CHECK(g_group_calls.size() == calls && g_fetches == 0);
  g_calls.clear();
  // ---- a refusal of the device: false, nothing fetched or applied
  g_refuse = true;
  CHECK(!step(grp, worlds, {2}, overlap, out, &fresh));
  g_refuse = false;
  CALLS("group_track_some");
  CHECK(g_fetches == 0 && fresh[2]->fts_.empty() && out[2].repr_n_matches == SENTINEL);
}

int main() {
  test_track_some();
  std::printf("group subset mock test OK: %zu group calls\n", g_group_calls.size());
  return 0;
}
