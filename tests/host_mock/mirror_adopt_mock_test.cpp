// CPU-only test of hip_bridge::DeviceSeedMirror::adopt and of the device-grid mode of update() (include/svo_dropin/
// depth_filter_batch.h) against a MOCK of the svo_hip_seed_batch_* entry points, in the manner of mirror_mock_test.cpp: the mock
// "device" gives every seed a countdown -- it is "updated" every pass and "converges" when the countdown reaches zero.
// A batch "created from a detection" is made by the mock directly (mock_detected_batch) and handed to adopt() with the list
// entries the host pushed for it.  Checked: adopted seeds are never uploaded; their events reach the right list entries; age-out,
// a foreign removeKeyframe, recycled list nodes and syncToHost work on adopted batches as on uploaded ones; in the device-grid
// mode a keyframe's pass runs with report_updated = 0, one svo_hip_seed_batch_mark_updated call follows it for the frame's set
// of batches, and Host::setGridOccupancy is not called.
// Built and run by tests/test_host_mirror_adopt_mock.py with g++ -std=c++11, once more with -fsanitize=address,undefined.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <list>
#include <vector>

#include "svo_hip.h"
#include "svo_dropin/depth_filter_batch.h"

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

// ---------------------------------------------------------------- mock device
struct svo_hip_seed_batch {
  std::vector<float> a, b, mu, sigma2;
  std::vector<int> countdown;
  std::vector<uint8_t> alive;
  std::vector<svo_hip_seed_event> events;
  int32_t counts[7];
  bool pending;
};
struct svo_hip_pyramid { int unused; };
static int g_created = 0, g_destroyed = 0, g_uploaded_seeds = 0, g_updates = 0;
static int g_fail_group_after = -1;
static std::vector<int> g_report_updated;                // per grouped call
struct MarkCall { std::vector<svo_hip_seed_batch*> batches; std::vector<int> pending; int cell, cols, rows; uint8_t* grid; };
static std::vector<MarkCall> g_marks;

static svo_hip_seed_batch* mock_batch(int n, int countdown_base) {
  svo_hip_seed_batch* s = new svo_hip_seed_batch;
  s->a.assign((size_t)n, 10.f); s->b.assign((size_t)n, 10.f); s->mu.assign((size_t)n, 0.5f); s->sigma2.assign((size_t)n, 1.f);
  s->countdown.resize((size_t)n); s->alive.assign((size_t)n, 1);
  for (int i = 0; i < n; ++i) s->countdown[(size_t)i] = countdown_base + (i % 5);
  s->pending = false;
  ++g_created;
  return s;
}
// svo_hip_seed_batch_create_detected in miniature: the batch exists on the "device", nothing came from the host
static svo_hip_seed_batch* mock_detected_batch(int n, int countdown_base) { return mock_batch(n, countdown_base); }

extern "C" {
int svo_hip_seed_batch_create(svo_hip_ctx*, int n, const double* px, const double*, const int32_t*, const float*, const float*,
                              const float*, const float*, const float*, svo_hip_seed_batch** out) {
  *out = mock_batch(n, (int)px[0]);                      // the test encodes the countdown base in px[0] of the first seed
  g_uploaded_seeds += n;
  return SVO_HIP_OK;
}
int svo_hip_seed_batch_destroy(svo_hip_seed_batch* s) { if (s) { ++g_destroyed; delete s; } return SVO_HIP_OK; }
int svo_hip_seed_batch_update_group_async(int n, svo_hip_seed_batch* const* sbs, const svo_hip_pyramid*, const int*, const svo_hip_pyramid*, int,
                                          const svo_hip_camera*, const double*, const double*, const svo_hip_df_params*, int report_updated) {
  for (int k = 0; k < n; ++k) if (sbs[k]->pending) return SVO_HIP_ERR_STATE;
  g_report_updated.push_back(report_updated);
  for (int k = 0; k < n; ++k) {
    if (g_fail_group_after >= 0 && k == g_fail_group_after) return SVO_HIP_ERR_DEVICE;
    svo_hip_seed_batch* s = sbs[k];
    ++g_updates;
    s->events.clear();
    for (int c = 0; c < 7; ++c) s->counts[c] = 0;
    for (size_t i = 0; i < s->alive.size(); ++i) {
      if (!s->alive[i]) { ++s->counts[SVO_HIP_SEED_ERASED + 1]; continue; }
      --s->countdown[i];
      s->mu[i] += 1.0f; s->sigma2[i] *= 0.5f;
      const int st = s->countdown[i] <= 0 ? SVO_HIP_SEED_CONVERGED : SVO_HIP_SEED_UPDATED;
      ++s->counts[st + 1];
      if (st != SVO_HIP_SEED_UPDATED || report_updated) {
        svo_hip_seed_event e;
        e.index = (int32_t)i; e.status = st; e.mu = s->mu[i]; e.sigma2 = s->sigma2[i];
        e.xyz_world[0] = (double)i; e.xyz_world[1] = s->mu[i]; e.xyz_world[2] = 0.0;
        e.px_cur[0] = (double)i; e.px_cur[1] = 0.0;
        s->events.push_back(e);
      }
      if (st != SVO_HIP_SEED_UPDATED) s->alive[i] = 0;
    }
    s->pending = true;
  }
  return SVO_HIP_OK;
}
int svo_hip_seed_batch_pending(const svo_hip_seed_batch* s) { return s && s->pending ? 1 : 0; }
int svo_hip_seed_batch_collect(svo_hip_seed_batch* s, const svo_hip_seed_event** ev, int* n_ev, int32_t counts[7]) {
  if (!s->pending) return SVO_HIP_ERR_STATE;
  s->pending = false;
  if (ev) *ev = s->events.empty() ? NULL : &s->events[0];
  if (n_ev) *n_ev = (int)s->events.size();
  if (counts) for (int k = 0; k < 7; ++k) counts[k] = s->counts[k];
  return SVO_HIP_OK;
}
int svo_hip_seed_batch_erase(svo_hip_seed_batch* s, int n, const int32_t* idx) {
  for (int k = 0; k < n; ++k) s->alive[(size_t)idx[k]] = 0;
  return SVO_HIP_OK;
}
int svo_hip_seed_batch_download(svo_hip_seed_batch* s, float* a, float* b, float* mu, float* sigma2, uint8_t* alive) {
  if (a) std::copy(s->a.begin(), s->a.end(), a);
  if (b) std::copy(s->b.begin(), s->b.end(), b);
  if (mu) std::copy(s->mu.begin(), s->mu.end(), mu);
  if (sigma2) std::copy(s->sigma2.begin(), s->sigma2.end(), sigma2);
  if (alive) std::copy(s->alive.begin(), s->alive.end(), alive);
  return SVO_HIP_OK;
}
int svo_hip_seed_batch_mark_updated(int n, svo_hip_seed_batch* const* sbs, int cell_size, int grid_cols, int grid_rows, uint8_t* occupancy_dev) {
  MarkCall c;
  c.batches.assign(sbs, sbs + n);
  for (int k = 0; k < n; ++k) c.pending.push_back(sbs[k]->pending ? 1 : 0);
  c.cell = cell_size; c.cols = grid_cols; c.rows = grid_rows; c.grid = occupancy_dev;
  g_marks.push_back(c);
  return SVO_HIP_OK;
}
}  // extern "C"

// ---------------------------------------------------------------- minimal host types (the shape of the reference's)
struct Frame { int id; bool keyframe; };
struct Feature { Frame* frame; double px[2]; };
struct Seed {
  static int batch_counter, seed_counter;
  int batch_id, id;
  Feature* ftr;
  float a, b, mu, z_range, sigma2;
  Seed(Feature* f) : batch_id(batch_counter), id(seed_counter++), ftr(f), a(10), b(10), mu(0.5f), z_range(1), sigma2(1) {}
};
int Seed::batch_counter = 0;
int Seed::seed_counter = 0;

struct Host {
  std::vector<int> converged_log;                         // seed ids in callback order
  std::vector<double> grid_log;
  svo_hip_pyramid pyr;
  Frame* keyframeOf(const Seed& s) const { return s.ftr->frame; }
  void feature(const Seed& s, double px[2], double f[3], int* level) const { px[0] = s.ftr->px[0]; px[1] = s.ftr->px[1]; f[0] = f[1] = 0; f[2] = 1; *level = 0; }
  void pose7(const Frame&, double T[7]) const { for (int k = 0; k < 7; ++k) T[k] = k == 6 ? 1.0 : 0.0; }
  bool keyframeSlots(const std::vector<Frame*>& kfs, std::vector<int>& slots) { slots.assign(kfs.size(), 0); return true; }
  int currentSlot(Frame&) { return 0; }
  svo_hip_pyramid* keyframePyramids() { return &pyr; }
  svo_hip_pyramid* currentPyramids() { return &pyr; }
  svo_hip_camera camera(const Frame&) const { svo_hip_camera c = svo_hip_camera(); c.width = 640; c.height = 480; return c; }
  bool isKeyframe(const Frame& f) const { return f.keyframe; }
  void setGridOccupancy(const double px_cur[2]) { grid_log.push_back(px_cur[0]); }
  void converged(Seed& s, const double*) { converged_log.push_back(s.id); }
};

typedef std::list<Seed> SeedList;
typedef svo::hip_bridge::DeviceSeedMirror<SeedList> Mirror;
static std::vector<Feature*> g_features;                  // freed at the end

// initializeSeeds with handed-in features: list entries only, the mirror uploads them at its next update
static void push_keyframe(SeedList& seeds, Frame* kf, int n, int countdown_base) {
  ++Seed::batch_counter;
  for (int i = 0; i < n; ++i) {
    Feature* f = new Feature; f->frame = kf; f->px[0] = countdown_base; f->px[1] = 0;
    g_features.push_back(f);
    seeds.push_back(Seed(f));
  }
}
// initializeSeeds on the device: the batch exists, one list entry per seed, adopt
static void adopt_keyframe(Mirror& mirror, SeedList& seeds, Frame* kf, int n, int countdown_base) {
  svo_hip_seed_batch* batch = mock_detected_batch(n, countdown_base);
  ++Seed::batch_counter;
  SeedList::iterator first = seeds.end();
  for (int i = 0; i < n; ++i) {
    Feature* f = new Feature; f->frame = kf; f->px[0] = -1; f->px[1] = 0;
    g_features.push_back(f);
    seeds.push_back(Seed(f));
    if (i == 0) { first = seeds.end(); --first; }
  }
  mirror.adopt(batch, first, (size_t)n, Seed::batch_counter, kf);
}

int main() {
  svo_hip_df_params prm = svo_hip_df_params();
  volatile bool halt = false;
  Host host;
  SeedList seeds;
  Mirror mirror;
  Frame kfA = {0, true}, kfB = {1, true}, kfC = {2, true}, kfD = {3, true}, cur = {9, false}, cur_kf = {10, true};
  uint8_t grid_bytes[4] = {0, 0, 0, 0};
  const svo::hip_bridge::DeviceGrid grid = {30, 22, 16, grid_bytes};
  svo::hip_bridge::SeedBatchStats st;

  // ---- an adopted batch is never uploaded; the next update finds nothing fresh and does not re-read the list
  adopt_keyframe(mirror, seeds, &kfA, 50, 2);                       // ids 0..49, countdowns 2..6
  CHECK(mirror.deviceBatches() == 1 && g_created == 1 && g_uploaded_seeds == 0);
  st = mirror.update(host, NULL, seeds, cur, prm, Seed::batch_counter, 3, halt, 4096);
  CHECK(st.n_uploaded == 0 && !st.resynced && g_uploaded_seeds == 0 && g_created == 1);
  CHECK(st.n_seeds == 50 && st.n_updated == 50 && st.n_converged == 0 && st.n_device_calls == 1);
  st = mirror.update(host, NULL, seeds, cur, prm, Seed::batch_counter, 3, halt, 4096);
  CHECK(st.n_uploaded == 0 && !st.resynced && st.n_converged == 10 && seeds.size() == 40);
  for (size_t k = 0; k < host.converged_log.size(); ++k) CHECK(host.converged_log[k] == (int)(5 * k));   // device index -> list entry
  for (SeedList::iterator it = seeds.begin(); it != seeds.end(); ++it) CHECK(it->id % 5 != 0);
  CHECK(g_report_updated.size() == 2 && g_report_updated[0] == 0 && g_report_updated[1] == 0 && g_marks.empty());

  // ---- the device-grid mode on a frame that is no keyframe: an ordinary pass, no mark call
  st = mirror.update(host, NULL, seeds, cur, prm, Seed::batch_counter, 3, halt, 4096, &grid);
  CHECK(g_marks.empty() && g_report_updated.back() == 0 && host.grid_log.empty() && st.n_converged == 10 && seeds.size() == 30);

  // ---- a second keyframe the old way (uploaded at the next update) and a third one adopted: one pass over all three
  push_keyframe(seeds, &kfB, 20, 50);                               // ids 50..69
  st = mirror.update(host, NULL, seeds, cur, prm, Seed::batch_counter, 3, halt, 4096);
  CHECK(st.n_uploaded == 20 && g_uploaded_seeds == 20 && mirror.deviceBatches() == 2 && !st.resynced);
  adopt_keyframe(mirror, seeds, &kfC, 25, 60);                      // ids 70..94
  CHECK(mirror.deviceBatches() == 3 && g_uploaded_seeds == 20);

  // ---- the device-grid mode on a keyframe: report_updated = 0, ONE mark call for the frame's set, behind the pass (the batches
  // ---- still have it pending), no host grid mark; convergence events are handled as ever
  const size_t conv_before = host.converged_log.size();
  st = mirror.update(host, NULL, seeds, cur_kf, prm, Seed::batch_counter, 3, halt, 4096, &grid);
  CHECK(st.n_uploaded == 0 && !st.resynced && g_uploaded_seeds == 20);
  CHECK(g_report_updated.back() == 0 && host.grid_log.empty());
  CHECK(g_marks.size() == 1 && g_marks[0].batches.size() == 3 && g_marks[0].cell == 30 && g_marks[0].cols == 22 && g_marks[0].rows == 16 &&
        g_marks[0].grid == grid_bytes);
  for (size_t k = 0; k < 3; ++k) CHECK(g_marks[0].pending[k] == 1);
  CHECK(st.n_converged == 10 && host.converged_log.size() == conv_before + 10);     // A's countdown-5 seeds, after five passes
  CHECK(st.n_updated == 20 + 20 + 25);                                              // A has 20 seeds left after four passes
  // the plain form on a keyframe reports and marks on the host, as ever
  st = mirror.update(host, NULL, seeds, cur_kf, prm, Seed::batch_counter, 3, halt, 4096);
  CHECK(g_report_updated.back() == 1 && g_marks.size() == 1 && host.grid_log.size() == 10 + 20 + 25);
  // a NULL grid given to the grid form: the plain form
  host.grid_log.clear();
  st = mirror.update(host, NULL, seeds, cur_kf, prm, Seed::batch_counter, 3, halt, 4096, NULL);
  CHECK(g_report_updated.back() == 1 && g_marks.size() == 1 && !host.grid_log.empty());
  CHECK(mirror.deviceBatches() == 2 && st.n_seeds == 45);           // (A's last seeds converged in the pass before: its batch is gone)

  // ---- syncToHost on an adopted batch
  SeedList::iterator c0 = seeds.begin();
  while (c0->ftr->frame != &kfC) ++c0;
  CHECK(c0->mu == 0.5f);
  CHECK(mirror.syncToHost());
  CHECK(c0->mu == 3.5f && c0->sigma2 == 0.125f);                    // three passes since it was adopted

  // ---- a grouped pass that fails half-way in the device-grid mode: only the batches whose pass was enqueued are marked
  g_fail_group_after = 1;
  st = mirror.update(host, NULL, seeds, cur_kf, prm, Seed::batch_counter, 3, halt, 4096, &grid);
  CHECK(st.n_device_errors == 1 && g_marks.size() == 2 && g_marks[1].batches.size() == 1 && st.n_updated == 20);
  g_fail_group_after = -1;

  // ---- removeKeyframe behind the mirror's back takes an adopted keyframe's seeds; a new adopted keyframe follows, whose list
  // ---- nodes may reuse the freed addresses
  for (SeedList::iterator it = seeds.begin(); it != seeds.end();) it = (it->ftr->frame == &kfC) ? seeds.erase(it) : ++it;
  CHECK(seeds.size() == 20);
  adopt_keyframe(mirror, seeds, &kfD, 30, 70);                      // ids 95..124
  const int uploaded_before = g_uploaded_seeds;
  st = mirror.update(host, NULL, seeds, cur, prm, Seed::batch_counter, 3, halt, 4096);
  CHECK(st.resynced && st.n_uploaded == 0 && g_uploaded_seeds == uploaded_before);  // the list was re-read; the adopted seeds were known
  CHECK(st.n_seeds == 50 && st.n_updated == 50 && mirror.deviceBatches() == 2);
  CHECK(mirror.syncToHost());
  for (SeedList::iterator it = seeds.begin(); it != seeds.end(); ++it)
    CHECK(it->mu == (it->ftr->frame == &kfD ? 1.5f : 0.5f + 6.0f));                // D: one pass; B: six -- no state mixed up by recycled nodes
  st = mirror.update(host, NULL, seeds, cur, prm, Seed::batch_counter, 3, halt, 4096);
  CHECK(!st.resynced && st.n_uploaded == 0);

  // ---- age-out of an adopted batch: batch_counter - batch_id > max_n_kfs
  Seed::batch_counter += 3;                                         // B (batch id 2) is 5 keyframes old, D (4) is 3
  st = mirror.update(host, NULL, seeds, cur, prm, Seed::batch_counter, 3, halt, 4096);
  CHECK(st.n_aged_out == 20 && seeds.size() == 30 && mirror.deviceBatches() == 1);
  Seed::batch_counter += 1;
  st = mirror.update(host, NULL, seeds, cur, prm, Seed::batch_counter, 3, halt, 4096);
  CHECK(st.n_aged_out == 30 && seeds.empty() && mirror.deviceBatches() == 0);

  // ---- adopt of nothing: a NULL batch (the detection found no feature) changes nothing
  mirror.adopt((svo_hip_seed_batch*)NULL, seeds.end(), 0, Seed::batch_counter, &kfA);
  st = mirror.update(host, NULL, seeds, cur, prm, Seed::batch_counter, 3, halt, 4096);
  CHECK(mirror.deviceBatches() == 0 && !st.resynced && st.n_seeds == 0);
  mirror.clear();
  CHECK(g_created == g_destroyed && g_uploaded_seeds == 20);
  for (size_t k = 0; k < g_features.size(); ++k) delete g_features[k];
  std::printf("mirror adopt mock test OK: %d device batches, %d seeds uploaded, %d passes, %d mark calls\n", g_created, g_uploaded_seeds,
              g_updates, (int)g_marks.size());
  return 0;
}
