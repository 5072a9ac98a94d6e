// CPU-only test of the split hip_bridge::DeviceSeedMirror (include/svo_dropin/depth_filter_batch.h) and of updateCameras(), the
// several-mirror function, against the MOCK device of tests/host_mock/mirror_mock_test.cpp, reused here by inclusion: its
// svo_hip_seed_batch_* definitions are renamed to inner_* while that file is read, and the entry points the header calls are
// defined below as wrappers that LOG every call before they forward it.
//   1. the whole scenario of mirror_mock_test.cpp runs through update(): the sequence of device calls it makes hashes to the
//      value recorded with the header as it was before update() was split into phases (same calls, same order, same sizes);
//   2. updateCameras() over three cameras makes exactly ONE device call (svo_hip_seed_batch_update_cameras_async, no call per
//      camera), its collects come in camera order, and every camera's callbacks and list equal those of a twin run through
//      update().
// Built plain (g++ -std=c++11) and run by tests/test_host_mirror_cameras_mock.py.
#include <string>

#include "svo_hip.h"
#include "svo_dropin/slot_table.h"
#include "svo_dropin/depth_filter_batch.h"     // (the template's calls keep their names: read before the renaming below)

#define svo_hip_seed_batch_create inner_create
#define svo_hip_seed_batch_destroy inner_destroy
#define svo_hip_seed_batch_size inner_size
#define svo_hip_seed_batch_update_async inner_update_async
#define svo_hip_seed_batch_update_group_async inner_update_group_async
#define svo_hip_seed_batch_pending inner_pending
#define svo_hip_seed_batch_collect inner_collect
#define svo_hip_seed_batch_erase inner_erase
#define svo_hip_seed_batch_download inner_download
#define main mirror_mock_main
#include "../host_mock/mirror_mock_test.cpp"
#undef main
#undef svo_hip_seed_batch_create
#undef svo_hip_seed_batch_destroy
#undef svo_hip_seed_batch_size
#undef svo_hip_seed_batch_update_async
#undef svo_hip_seed_batch_update_group_async
#undef svo_hip_seed_batch_pending
#undef svo_hip_seed_batch_collect
#undef svo_hip_seed_batch_erase
#undef svo_hip_seed_batch_download

// ---------------------------------------------------------------- the log
static std::vector<std::string> g_log;
static std::map<const svo_hip_seed_batch*, int> g_name;      // batches are named in creation order (addresses may be recycled)
static int g_next_name = 0;
static int g_camera_calls = 0;
static std::map<const svo_hip_seed_batch*, int> g_camera_of;  // the camera under which the last several-camera call named a batch
static std::vector<int> g_collect_cameras;                    // ... of every collect since, in order
static std::string num(long long v) { char b[32]; std::snprintf(b, sizeof(b), "%lld", v); return b; }
static std::string name_of(const svo_hip_seed_batch* s) { return "#" + num(g_name.count(s) ? g_name[s] : -1); }
static unsigned long long log_hash() {
  unsigned long long h = 1469598103934665603ull;               // FNV-1a over the lines
  for (size_t k = 0; k < g_log.size(); ++k) {
    for (size_t i = 0; i < g_log[k].size(); ++i) { h ^= (unsigned char)g_log[k][i]; h *= 1099511628211ull; }
    h ^= '\n'; h *= 1099511628211ull;
  }
  return h;
}

extern "C" {
int svo_hip_seed_batch_create(svo_hip_ctx* c, int n, const double* px, const double* f, const int32_t* l, const float* a, const float* b,
                              const float* mu, const float* zr, const float* s2, svo_hip_seed_batch** out) {
  const int rc = inner_create(c, n, px, f, l, a, b, mu, zr, s2, out);
  g_name[*out] = g_next_name++;
  g_log.push_back("create " + name_of(*out) + " n=" + num(n));
  return rc;
}
int svo_hip_seed_batch_destroy(svo_hip_seed_batch* s) {
  g_log.push_back("destroy " + name_of(s));
  g_name.erase(s);
  return inner_destroy(s);
}
int svo_hip_seed_batch_update_group_async(int n, svo_hip_seed_batch* const* sbs, const svo_hip_pyramid* ref, const int* slots,
                                          const svo_hip_pyramid* cur, int cur_slot, const svo_hip_camera* cam, const double* T_ref_w,
                                          const double* T_cur_w, const svo_hip_df_params* prm, int report_updated) {
  std::string line = "group report=" + num(report_updated) + " cur=" + num(cur_slot);
  for (int k = 0; k < n; ++k) line += " " + name_of(sbs[k]) + "@" + num(slots[k]);
  g_log.push_back(line);
  return inner_update_group_async(n, sbs, ref, slots, cur, cur_slot, cam, T_ref_w, T_cur_w, prm, report_updated);
}
int svo_hip_seed_batch_update_cameras_async(svo_hip_ctx*, int n_cameras, const svo_hip_seed_camera_pass* p, const svo_hip_pyramid* ref,
                                            const svo_hip_pyramid* cur, const svo_hip_camera* cam, const svo_hip_df_params* prm) {
  ++g_camera_calls;
  std::string line = "cameras n=" + num(n_cameras);
  for (int c = 0; c < n_cameras; ++c)
    for (int k = 0; k < p[c].n_batches; ++k) if (p[c].batches[k]->pending) return SVO_HIP_ERR_STATE;     // checked before anything is enqueued
  for (int c = 0; c < n_cameras; ++c) {
    line += " | cam" + num(c) + " report=" + num(p[c].report_updated) + " cur=" + num(p[c].cur_slot);
    for (int k = 0; k < p[c].n_batches; ++k) {
      line += " " + name_of(p[c].batches[k]) + "@" + num(p[c].ref_slots[k]);
      g_camera_of[p[c].batches[k]] = c;
      inner_update_async(p[c].batches[k], ref, p[c].ref_slots[k], cur, p[c].cur_slot, cam, p[c].T_ref_w + 7 * k, p[c].T_cur_w, prm, p[c].report_updated);
    }
  }
  g_log.push_back(line);
  return SVO_HIP_OK;
}
int svo_hip_seed_batch_pending(const svo_hip_seed_batch* s) { return inner_pending(s); }
int svo_hip_seed_batch_collect(svo_hip_seed_batch* s, const svo_hip_seed_event** ev, int* n_ev, int32_t counts[7]) {
  const int rc = inner_collect(s, ev, n_ev, counts);
  if (g_camera_of.count(s)) g_collect_cameras.push_back(g_camera_of[s]);
  g_log.push_back("collect " + name_of(s) + " rc=" + num(rc) + " events=" + num(rc == SVO_HIP_OK && n_ev ? *n_ev : -1));
  return rc;
}
int svo_hip_seed_batch_erase(svo_hip_seed_batch* s, int n, const int32_t* idx) {
  g_log.push_back("erase " + name_of(s) + " n=" + num(n));
  return inner_erase(s, n, idx);
}
int svo_hip_seed_batch_download(svo_hip_seed_batch* s, float* a, float* b, float* mu, float* sigma2, uint8_t* alive) {
  g_log.push_back("download " + name_of(s));
  return inner_download(s, a, b, mu, sigma2, alive);
}
}  // extern "C"

// the device calls of mirror_mock_test.cpp's scenario through update(), recorded with the header of the parent commit (one
// update() body): line count and FNV-1a hash of the log above
static const size_t kUpdateLogLines = 197;
static const unsigned long long kUpdateLogHash = 12123843149330504597ull;

typedef svo::hip_bridge::DeviceSeedMirror<SeedList> Mirror;

struct Rig {                      // one camera: a list, a mirror, a host, its frames
  SeedList seeds;
  Mirror mirror;
  Host host;
  std::vector<Frame> kfs;
  Rig() : kfs(3) {}
};

// three cameras with different keyframes and seed counts; camera 1 has no seeds at all in the first frames
static void feed(Rig* r, int n_cams, int frame) {
  for (int c = 0; c < n_cams; ++c) {
    if (frame == 0 && c != 1) { r[c].kfs[0].id = 10 * c; r[c].kfs[0].keyframe = true; add_keyframe(r[c].seeds, &r[c].kfs[0], 30 + 25 * c, 2); }
    if (frame == 2) { r[c].kfs[1].id = 10 * c + 1; r[c].kfs[1].keyframe = true; add_keyframe(r[c].seeds, &r[c].kfs[1], 12 + c, 3); }
  }
}

int main() {
  // ---- 1. update() over the old scenario
  if (mirror_mock_main() != 0) return 1;
  std::printf("update() log: %zu lines, hash %llu\n", g_log.size(), log_hash());
  CHECK(g_camera_calls == 0);                                                     // update() never makes the several-camera call
#ifdef MIRROR_LOG_RECORD            // (how the two constants were made: this part alone, built against the header to compare with)
  return 0;
#else
  CHECK(g_log.size() == kUpdateLogLines && log_hash() == kUpdateLogHash);

  // ---- 2. updateCameras() against twins run through update()
  const int N = 3, FRAMES = 6;
  svo_hip_df_params prm = svo_hip_df_params();
  volatile bool halt = false;
  Rig one[N], all[N];
  Frame cur[N], cur_kf[N];
  for (int c = 0; c < N; ++c) { cur[c].id = 900 + c; cur[c].keyframe = false; cur_kf[c].id = 950 + c; cur_kf[c].keyframe = true; }
  const int counter0 = Seed::batch_counter;
  for (int frame = 0; frame < FRAMES; ++frame) {
    Frame* fr[N];
    for (int c = 0; c < N; ++c) fr[c] = (frame == 3 && c != 2) ? &cur_kf[c] : &cur[c];     // frame 3: cameras 0 and 1 are keyframes
    // the twins, one update() per camera
    Seed::batch_counter = counter0 + 4 * frame;
    feed(one, N, frame);
    const int bc = Seed::batch_counter;
    svo::hip_bridge::SeedBatchStats want[N], got[N];
    for (int c = 0; c < N; ++c) want[c] = one[c].mirror.update(one[c].host, NULL, one[c].seeds, *fr[c], prm, bc, 12, halt, 40);
    // the one call
    Seed::batch_counter = counter0 + 4 * frame;
    feed(all, N, frame);
    CHECK(Seed::batch_counter == bc);
    Mirror* mirrors[N]; Host* hosts[N]; SeedList* lists[N]; int counters[N];
    for (int c = 0; c < N; ++c) { mirrors[c] = &all[c].mirror; hosts[c] = &all[c].host; lists[c] = &all[c].seeds; counters[c] = bc; }
    const size_t log0 = g_log.size();
    const int calls0 = g_camera_calls;
    g_camera_of.clear(); g_collect_cameras.clear();
    svo::hip_bridge::updateCameras(N, mirrors, hosts, (svo_hip_ctx*)NULL, lists, fr, prm, counters, 12, halt, got, 40);
    // exactly one device call for the pass, none per camera; then the collects, camera by camera
    int n_group = 0, n_cameras_lines = 0, n_collects = 0;
    for (size_t k = log0; k < g_log.size(); ++k) {
      if (g_log[k].compare(0, 6, "group ") == 0) ++n_group;
      if (g_log[k].compare(0, 8, "cameras ") == 0) { ++n_cameras_lines; CHECK(n_collects == 0); }     // in front of every collect
      if (g_log[k].compare(0, 8, "collect ") == 0) ++n_collects;
    }
    CHECK((size_t)n_collects == g_collect_cameras.size() && std::is_sorted(g_collect_cameras.begin(), g_collect_cameras.end()));
    int n_with_seeds = 0;
    for (int c = 0; c < N; ++c) n_with_seeds += want[c].n_seeds > 0;
    CHECK(n_group == 0 && g_camera_calls - calls0 == (n_with_seeds ? 1 : 0) && n_cameras_lines == g_camera_calls - calls0);
    for (int c = 0; c < N; ++c) {
      CHECK(got[c].n_seeds == want[c].n_seeds && got[c].n_updated == want[c].n_updated && got[c].n_converged == want[c].n_converged);
      CHECK(got[c].n_nan == want[c].n_nan && got[c].n_aged_out == want[c].n_aged_out && got[c].n_uploaded == want[c].n_uploaded);
      CHECK(got[c].n_device_calls == want[c].n_device_calls && got[c].n_device_errors == 0 && want[c].n_device_errors == 0);
      CHECK(all[c].seeds.size() == one[c].seeds.size() && all[c].mirror.deviceBatches() == one[c].mirror.deviceBatches());
      CHECK(all[c].host.converged_log.size() == one[c].host.converged_log.size() && all[c].host.grid_log == one[c].host.grid_log);
      for (size_t k = 0; k < all[c].host.converged_log.size(); ++k)
        CHECK(all[c].host.converged_log[k].second == one[c].host.converged_log[k].second);          // sigma2 at the callback, in order
    }
  }
  int n_conv = 0, n_marks = 0;
  for (int c = 0; c < N; ++c) { n_conv += (int)all[c].host.converged_log.size(); n_marks += (int)all[c].host.grid_log.size(); }
  CHECK(n_conv > 20 && n_marks > 20 && all[2].host.grid_log.empty());             // camera 2 never had a keyframe frame
  for (int c = 0; c < N; ++c) { one[c].mirror.clear(); all[c].mirror.clear(); }
  CHECK(g_created == g_destroyed);
  std::printf("mirror cameras mock test OK: %d calls for all cameras\n", g_camera_calls);
  return 0;
#endif
}
