// CPU-only test of the camera-rig paths of the bridges against a MOCK device: hip_bridge::updateCameraRig
// (include/svo_dropin/depth_filter_batch.h) and hip_bridge::FrameTrackerGroupT (include/svo_dropin/frame_tracker_batch.h) with a
// camera model per camera.  The mock seed batches and host types are those of tests/host_mock/mirror_mock_test.cpp, reused by
// inclusion; the two rig entry points of svo_hip.h and the calls they stand beside are defined below and RECORD what they were
// given.  What is checked:
//   1. updateCameraRig() over three cameras with three distinct models makes exactly ONE device call per pass, the rig call, and
//      camera c's model travels with camera c's pass (a camera that sits the pass out is given a model of the common size); every
//      camera ends as its twin does through update();
//   2. with three equal models the same function makes the call updateCameras() makes, never the rig call;
//   3. FrameTrackerGroupT built from three distinct models creates its group with the rig call, member c given cams[c]; from
//      equal models, and through the one-model constructor, with svo_hip_tracker_group_create.
// Built plain (g++ -std=c++11) and run by tests/test_host_rig_mock.py.
#include <memory>
#include <string>

#include "svo_hip.h"
#include "svo_dropin/slot_table.h"
#include "svo_dropin/depth_filter_batch.h"
#include "svo_dropin/frame_tracker_batch.h"

#define main mirror_mock_main
#include "../host_mock/mirror_mock_test.cpp"
#undef main

// ---------------------------------------------------------------- the record
struct PassRecord { int camera; int n_batches; svo_hip_camera model; };
struct CallRecord { std::string call; std::vector<PassRecord> passes; };
static std::vector<CallRecord> g_calls;
static std::vector<std::string> g_group_calls;
static std::vector<svo_hip_camera> g_member_models;          // of the last group created

struct svo_hip_ctx { int unused; };
struct svo_hip_tracker { int index; };
struct svo_hip_tracker_group { std::vector<svo_hip_tracker> members; };

static int run_passes(const char* call, int n_cameras, const svo_hip_seed_camera_pass* p, const svo_hip_pyramid* ref, const svo_hip_pyramid* cur,
                      const svo_hip_camera* cams, int cam_stride, const svo_hip_df_params* prm) {
  for (int c = 0; c < n_cameras; ++c)
    for (int k = 0; k < p[c].n_batches; ++k) if (p[c].batches[k]->pending) return SVO_HIP_ERR_STATE;     // checked before anything is enqueued
  for (int c = 1; c < n_cameras && cam_stride; ++c)
    if (cams[c].width != cams[0].width || cams[c].height != cams[0].height) return SVO_HIP_ERR_INVALID;  // also for a camera that sits out
  CallRecord r;
  r.call = call;
  for (int c = 0; c < n_cameras; ++c) {
    PassRecord pr = {c, p[c].n_batches, cams[c * cam_stride]};
    r.passes.push_back(pr);
    for (int k = 0; k < p[c].n_batches; ++k)
      svo_hip_seed_batch_update_async(p[c].batches[k], ref, p[c].ref_slots[k], cur, p[c].cur_slot, &cams[c * cam_stride], p[c].T_ref_w + 7 * k, p[c].T_cur_w,
                                      prm, p[c].report_updated);
  }
  g_calls.push_back(r);
  return SVO_HIP_OK;
}

extern "C" {
int svo_hip_seed_batch_update_cameras_async(svo_hip_ctx*, int n_cameras, const svo_hip_seed_camera_pass* p, const svo_hip_pyramid* ref,
                                            const svo_hip_pyramid* cur, const svo_hip_camera* cam, const svo_hip_df_params* prm) {
  return run_passes("cameras", n_cameras, p, ref, cur, cam, 0, prm);
}
int svo_hip_seed_batch_update_rig_async(svo_hip_ctx*, int n_cameras, const svo_hip_seed_camera_pass* p, const svo_hip_pyramid* ref,
                                        const svo_hip_pyramid* cur, const svo_hip_camera* cams, const svo_hip_df_params* prm) {
  return run_passes("rig", n_cameras, p, ref, cur, cams, 1, prm);
}
int svo_hip_ctx_create(svo_hip_ctx** out, int, void*) { *out = new svo_hip_ctx(); return SVO_HIP_OK; }
int svo_hip_ctx_destroy(svo_hip_ctx* c) { delete c; return SVO_HIP_OK; }
int svo_hip_tracker_destroy(svo_hip_tracker*) { return SVO_HIP_ERR_STATE; }                              // a group's camera goes with its group
static int make_group(const char* call, const svo_hip_camera* cams, int cam_stride, int n, svo_hip_tracker_group** out) {
  g_group_calls.push_back(call);
  g_member_models.clear();
  svo_hip_tracker_group* g = new svo_hip_tracker_group();
  for (int k = 0; k < n; ++k) { svo_hip_tracker t = {k}; g->members.push_back(t); g_member_models.push_back(cams[k * cam_stride]); }
  *out = g;
  return SVO_HIP_OK;
}
int svo_hip_tracker_group_create(svo_hip_ctx*, const svo_hip_camera* cam, const svo_hip_tracker_config*, int n, svo_hip_tracker_group** out) {
  return make_group("group_create", cam, 0, n, out);
}
int svo_hip_tracker_group_create_rig(svo_hip_ctx*, const svo_hip_camera* cams, const svo_hip_tracker_config*, int n, svo_hip_tracker_group** out) {
  return make_group("group_create_rig", cams, 1, n, out);
}
int svo_hip_tracker_group_destroy(svo_hip_tracker_group* g) { g_group_calls.push_back("group_destroy"); delete g; return SVO_HIP_OK; }
int svo_hip_tracker_group_camera(svo_hip_tracker_group* g, int index, svo_hip_tracker** camera) { *camera = &g->members[(size_t)index]; return SVO_HIP_OK; }
}  // extern "C"

// ---------------------------------------------------------------- hosts whose frames carry a camera model of their own
struct RigHost : Host {
  svo_hip_camera model;
  svo_hip_camera camera(const Frame&) const { return model; }
};

static svo_hip_camera model_of(int c, bool distinct) {
  svo_hip_camera m = svo_hip_camera();
  m.width = 640; m.height = 480;
  m.fx = distinct ? 430.0 + 65.0 * c : 500.0; m.fy = distinct ? 445.0 + 50.0 * c : 500.0; m.cx = 319.5 + (distinct ? 7.25 * c : 0.0); m.cy = 239.5;
  if (distinct && c == 2) { m.d[0] = -0.12; m.d[1] = 0.03; m.distortion = 1; }
  return m;
}

typedef svo::hip_bridge::DeviceSeedMirror<SeedList> Mirror;
struct Rig {                      // one camera: a list, a mirror, a host, its keyframes
  SeedList seeds;
  Mirror mirror;
  RigHost host;
  std::vector<Frame> kfs;
  Rig() : kfs(2) {}
};

// camera 1 has no seeds in the first two frames: it sits those passes out
static void feed(Rig* r, int n_cams, int frame) {
  for (int c = 0; c < n_cams; ++c) {
    if (frame == 0 && c != 1) { r[c].kfs[0].id = 10 * c; r[c].kfs[0].keyframe = true; add_keyframe(r[c].seeds, &r[c].kfs[0], 30 + 25 * c, 2); }
    if (frame == 2) { r[c].kfs[1].id = 10 * c + 1; r[c].kfs[1].keyframe = true; add_keyframe(r[c].seeds, &r[c].kfs[1], 12 + c, 3); }
  }
}

static void seed_passes(bool distinct) {
  const int N = 3, FRAMES = 5;
  svo_hip_df_params prm = svo_hip_df_params();
  volatile bool halt = false;
  Rig one[N], all[N];
  for (int c = 0; c < N; ++c) one[c].host.model = all[c].host.model = model_of(c, distinct);
  Frame cur[N], cur_kf[N];
  for (int c = 0; c < N; ++c) { cur[c].id = 900 + c; cur[c].keyframe = false; cur_kf[c].id = 950 + c; cur_kf[c].keyframe = true; }
  const int counter0 = Seed::batch_counter;
  int n_rig = 0, n_cameras = 0;
  for (int frame = 0; frame < FRAMES; ++frame) {
    Frame* fr[N];
    for (int c = 0; c < N; ++c) fr[c] = (frame == 3 && c != 2) ? &cur_kf[c] : &cur[c];
    Seed::batch_counter = counter0 + 4 * frame;
    feed(one, N, frame);
    const int bc = Seed::batch_counter;
    svo::hip_bridge::SeedBatchStats want[N], got[N];
    for (int c = 0; c < N; ++c) want[c] = one[c].mirror.update(one[c].host, NULL, one[c].seeds, *fr[c], prm, bc, 12, halt, 40);
    Seed::batch_counter = counter0 + 4 * frame;
    feed(all, N, frame);
    Mirror* mirrors[N]; RigHost* hosts[N]; SeedList* lists[N]; int counters[N];
    for (int c = 0; c < N; ++c) { mirrors[c] = &all[c].mirror; hosts[c] = &all[c].host; lists[c] = &all[c].seeds; counters[c] = bc; }
    const size_t calls0 = g_calls.size();
    svo::hip_bridge::updateCameraRig(N, mirrors, hosts, (svo_hip_ctx*)NULL, lists, fr, prm, counters, 12, halt, got, 40);
    // ---- the call sequence: one call for the pass
    CHECK(g_calls.size() == calls0 + 1);
    const CallRecord& r = g_calls.back();
    CHECK(r.call == (distinct ? "rig" : "cameras") && r.passes.size() == (size_t)N);
    n_rig += r.call == "rig"; n_cameras += r.call == "cameras";
    // ---- the camera that travels with each pass
    for (int c = 0; c < N; ++c) {
      const PassRecord& p = r.passes[(size_t)c];
      CHECK(p.camera == c && (p.n_batches > 0) == (want[c].n_seeds > 0));
      if (p.n_batches > 0) CHECK(svo::hip_bridge::sameCamera(p.model, all[c].host.model));
      else CHECK(p.model.width == 640 && p.model.height == 480);                   // sits out: a model of the common size
    }
    if (frame < 2) CHECK(r.passes[1].n_batches == 0);
    // ---- every camera as its twin through update()
    for (int c = 0; c < N; ++c) {
      CHECK(got[c].n_seeds == want[c].n_seeds && got[c].n_updated == want[c].n_updated && got[c].n_converged == want[c].n_converged);
      CHECK(got[c].n_nan == want[c].n_nan && got[c].n_uploaded == want[c].n_uploaded && got[c].n_device_calls == want[c].n_device_calls);
      CHECK(got[c].n_device_errors == 0 && all[c].seeds.size() == one[c].seeds.size());
      CHECK(all[c].host.converged_log.size() == one[c].host.converged_log.size() && all[c].host.grid_log == one[c].host.grid_log);
    }
  }
  CHECK(distinct ? (n_rig == FRAMES && n_cameras == 0) : (n_rig == 0 && n_cameras == FRAMES));
  // a model of another size is refused by the device call as a whole: every camera with a pass counts the error, nothing stays pending
  if (distinct) {
    all[2].host.model.width = 656;
    Frame* fr[N] = {&cur[0], &cur[1], &cur[2]};
    Mirror* mirrors[N]; RigHost* hosts[N]; SeedList* lists[N]; int counters[N];
    for (int c = 0; c < N; ++c) { mirrors[c] = &all[c].mirror; hosts[c] = &all[c].host; lists[c] = &all[c].seeds; counters[c] = Seed::batch_counter; }
    svo::hip_bridge::SeedBatchStats got[N];
    const size_t calls0 = g_calls.size();
    svo::hip_bridge::updateCameraRig(N, mirrors, hosts, (svo_hip_ctx*)NULL, lists, fr, prm, counters, 12, halt, got, 40);
    CHECK(g_calls.size() == calls0);
    for (int c = 0; c < N; ++c) CHECK(got[c].n_device_errors == (got[c].n_device_calls > 0 ? 1 : 0) && got[c].n_updated == 0);
  }
  for (int c = 0; c < N; ++c) { one[c].mirror.clear(); all[c].mirror.clear(); }
}

// ---------------------------------------------------------------- the tracker group
struct TrackerTypes {             // FrameTrackerGroupT is only created and destroyed here: the policy's types, no behaviour
  struct Frame {};
  typedef std::shared_ptr<Frame> FramePtr;
  struct Feature {};
  struct Point {};
  struct Map {};
};
typedef svo::hip_bridge::FrameTrackerGroupT<TrackerTypes> Group;

static void tracker_groups() {
  svo_hip_tracker_config cfg = svo_hip_tracker_config();
  for (int distinct = 0; distinct < 2; ++distinct) {
    std::vector<svo_hip_camera> cams;
    for (int c = 0; c < 3; ++c) cams.push_back(model_of(c, distinct != 0));
    g_group_calls.clear();
    {
      Group g(cams, cfg);
      CHECK(g.ok() && g.size() == 3);
      CHECK(g_group_calls.size() == 1 && g_group_calls[0] == (distinct ? "group_create_rig" : "group_create"));
      CHECK(g_member_models.size() == 3);
      for (int c = 0; c < 3; ++c) CHECK(svo::hip_bridge::sameCamera(g_member_models[(size_t)c], cams[(size_t)c]));       // member c: cams[c]
    }
    CHECK(g_group_calls.size() == 2 && g_group_calls[1] == "group_destroy");
  }
  g_group_calls.clear();
  {
    Group g(model_of(1, true), cfg, 4);                                          // the one-model constructor: the old call
    CHECK(g.ok() && g.size() == 4 && g_group_calls.size() == 1 && g_group_calls[0] == "group_create");
    for (int c = 0; c < 4; ++c) CHECK(svo::hip_bridge::sameCamera(g_member_models[(size_t)c], model_of(1, true)));
  }
  {
    Group g(std::vector<svo_hip_camera>(), cfg);                                 // no cameras: no group, no device call
    CHECK(!g.ok() && g.size() == 0 && g_group_calls.size() == 2);
  }
}

int main() {
  seed_passes(true);
  seed_passes(false);
  CHECK(g_created == g_destroyed);
  tracker_groups();
  std::printf("rig mock test OK: %zu passes\n", g_calls.size());
  return 0;
}
