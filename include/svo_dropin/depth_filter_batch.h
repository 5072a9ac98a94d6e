// depth_filter_batch.h -- DepthFilter::updateSeeds (S/depth_filter.cpp:237-341) with the seeds RESIDENT ON THE DEVICE,
// written ONCE against a small Host policy so that the drop-in for the reference's own types (depth_filter_hip.cpp) and
// the executable host layer on minimal types (android_svo_amd/host/svo_host.h, run on the GPU by
// tests/test_gpu_host_cpp.py) execute the same code.  Depends on svo_hip.h and the standard library only.
//
// The reference keeps its seeds in a std::list<Seed> and walks it once per frame.  Here every keyframe's seeds are
// mirrored on the device when they are first seen (svo_hip_seed_batch_create: Feature px / f / level and the Seed
// constructor's state, uploaded ONCE, in chunks of at most `sub_batch` seeds), and a frame costs two poses down and the
// seeds the host has to act on back (round 3 moved 144 B per seed over the link every frame):
//   * age-out of old seeds (:256-261)                     -> whole device batches dropped, their list entries erased
//   * visibility test, findEpipolarMatchDirect, computeTau, updateSeed (:264-299)
//                                                         -> device, all batches of the frame through one set of launches
//     (svo_hip_seed_batch_update_group_async), awaited once; the halt flag (:253) is polled before the frame's pass is
//     enqueued (a seed is either updated by this frame or not, as in the reference, where the prefix that got updated
//     also depends on when the flag rises: here the prefix is everything or nothing)
//   * on keyframes feature_detector_->setGridOccpuancy(matcher_.px_cur_) for every updated seed (:302-306),
//     convergence -> new Point + seed_converged_cb_ + erase (:310-331), NaN -> erase (:333-337)
//                                                         -> the batch's EVENTS, ascending seed index, batches in list
//     order: the callbacks (candidate-list insertion order), grid marks and erasures happen in the reference's order.
// The list entries of live seeds keep their CONSTRUCTION-time a / b / mu / sigma2 until syncToHost() copies the device
// state back (getSeeds() / getSeedsCopy() callers; the reference app has none) -- a converged seed's mu / sigma2 are
// written before its callback, which is all the reference's callback reads.
// Erasures behind the mirror's back (DepthFilter::removeKeyframe, reset: non-virtual in the reference) are noticed at the
// next call -- the list's size or its last seed id no longer match -- and the mirror is re-built from the list: seeds
// still there keep their device state, the others are erased on the device too.
//
// A keyframe's seeds may also be BORN on the device (svo_hip_seed_batch_create_detected: DepthFilter::initializeSeeds as one
// device call).  The host then pushes one list entry per returned feature and hands the batch over with adopt(): nothing is
// uploaded for those seeds.  With a DeviceGrid given to update(), a keyframe's pass does not report its updated seeds
// (report_updated = 0): svo_hip_seed_batch_mark_updated marks the device grid behind the pass on the stream instead of
// Host::setGridOccupancy (:302-306); convergence and NaN events are handled as ever.
//
// Host policy (duck-typed; see the two users):
//   Frame*  keyframeOf(const Seed&)                       it->ftr->frame
//   void    feature(const Seed&, double px[2], double f[3], int* level)
//   void    pose7(const Frame&, double T[7])              {t, q(xyzw)} of T_f_w_
//   bool    keyframeSlots(const std::vector<Frame*>&, std::vector<int>&)   device pyramid slots of ALL the frame's keyframes,
//                                                         resolved together (slot_table.h); false: unavailable
//   int     currentSlot(Frame&)                           device pyramid slot of the current frame (negative: unavailable)
//   svo_hip_pyramid* keyframePyramids(), currentPyramids()
//   svo_hip_camera camera(const Frame&)
//   bool    isKeyframe(const Frame&)
//   void    setGridOccupancy(const double px_cur[2])      feature_detector_->setGridOccpuancy
//   void    converged(Seed&, const double xyz_world[3])   new Point, ftr->point, seed_converged_cb_(point, sigma2)
#ifndef SVO_DROPIN_DEPTH_FILTER_BATCH_H_
#define SVO_DROPIN_DEPTH_FILTER_BATCH_H_

#include <cstddef>
#include <cstdint>
#include <unordered_map>
#include <vector>

#include "svo_hip.h"
#include "svo_dropin/camera_rig.h"

namespace svo {
namespace hip_bridge {

struct SeedBatchStats {
  int n_seeds = 0, n_aged_out = 0, n_updated = 0, n_failed_matches = 0, n_converged = 0, n_nan = 0;
  int n_device_calls = 0, n_device_errors = 0;
  int n_uploaded = 0;                  // seeds mirrored on the device by this call (0 on every frame but a keyframe's next)
  bool resynced = false;               // the list had changed behind the mirror's back
  bool halted = false;
};

/// The detector's occupancy grid as a device buffer (svo_hip_detect_grid, svo_hip_malloc) of the depth filter's context
struct DeviceGrid {
  int cell_size, grid_cols, grid_rows;
  uint8_t* occupancy_dev;
};

/// The device mirror of a std::list<Seed>: owned by the depth filter object, used under its seeds mutex.
template <class SeedList>
class DeviceSeedMirror {
 public:
  typedef typename SeedList::iterator It;
  typedef typename SeedList::value_type SeedT;

  DeviceSeedMirror() {}
  ~DeviceSeedMirror() { clear(); }
  DeviceSeedMirror(const DeviceSeedMirror&) = delete;
  DeviceSeedMirror& operator=(const DeviceSeedMirror&) = delete;

  void clear() {
    for (size_t k = 0; k < batches_.size(); ++k) svo_hip_seed_batch_destroy(batches_[k].dev);
    batches_.clear();
    where_.clear();
    known_size_ = 0; known_back_id_ = -1;
  }
  size_t deviceBatches() const { return batches_.size(); }
  struct Pass;                           // what the phases of update() hand on (below)

  /// DepthFilter::updateSeeds(frame).  `sub_batch`: seeds per device batch (an upload unit; one frame's pass covers all).
  template <class Host, class Frame>
  SeedBatchStats update(Host& host, svo_hip_ctx* ctx, SeedList& seeds, Frame& frame, const svo_hip_df_params& prm, int batch_counter,
                        int max_n_kfs, const volatile bool& halt, int sub_batch = 4096) {
    return updateImpl(NoGrid(), host, ctx, seeds, frame, prm, batch_counter, max_n_kfs, halt, sub_batch, NULL);
  }
  /// The device-grid mode: on a keyframe the pass runs with report_updated = 0, svo_hip_seed_batch_mark_updated marks
  /// *device_grid behind it on the stream, and Host::setGridOccupancy is not called.  (An overload of its own, so that users of
  /// the plain form need not link svo_hip_seed_batch_mark_updated.)  device_grid == NULL: the plain form.
  template <class Host, class Frame>
  SeedBatchStats update(Host& host, svo_hip_ctx* ctx, SeedList& seeds, Frame& frame, const svo_hip_df_params& prm, int batch_counter,
                        int max_n_kfs, const volatile bool& halt, int sub_batch, const DeviceGrid* device_grid) {
    return updateImpl(WithGrid(), host, ctx, seeds, frame, prm, batch_counter, max_n_kfs, halt, sub_batch, device_grid);
  }

 private:
  struct NoGrid {};
  struct WithGrid {};
  static int markUpdated(NoGrid, const std::vector<svo_hip_seed_batch*>&, const DeviceGrid*) { return SVO_HIP_OK; }
  static int markUpdated(WithGrid, const std::vector<svo_hip_seed_batch*>& passed, const DeviceGrid* g) {
    return svo_hip_seed_batch_mark_updated((int)passed.size(), passed.data(), g->cell_size, g->grid_cols, g->grid_rows, g->occupancy_dev);
  }

  /// update() is the composition of the three phases below (unchanged in behaviour); updateCameras() at the end of this header runs
  /// phase 1 for several mirrors, makes ONE device call for all of them and runs phase 3 per mirror.
  template <class Mode, class Host, class Frame>
  SeedBatchStats updateImpl(Mode mode, Host& host, svo_hip_ctx* ctx, SeedList& seeds, Frame& frame, const svo_hip_df_params& prm,
                            int batch_counter, int max_n_kfs, const volatile bool& halt, int sub_batch, const DeviceGrid* device_grid) {
    Pass p;
    if (!preparePass(host, ctx, seeds, frame, batch_counter, max_n_kfs, halt, sub_batch, device_grid, p)) return p.st;
    launchPass(mode, host, prm, device_grid, p);
    collectPass(host, seeds, p);
    return p.st;
  }

  /// phase 2, one mirror: the batches of the frame through ONE set of launches (svo_hip_seed_batch_update_group_async)
  template <class Mode, class Host>
  void launchPass(Mode mode, Host& host, const svo_hip_df_params& prm, const DeviceGrid* device_grid, Pass& p) {
    SeedBatchStats& st = p.st;
    if (p.devs.empty()) return;
    st.n_device_calls += (int)p.devs.size();
    const int rc = svo_hip_seed_batch_update_group_async((int)p.devs.size(), p.devs.data(), host.keyframePyramids(), p.slots.data(),
                                                         host.currentPyramids(), p.cur_slot, &p.cam, p.T_refs.data(), p.T_cur, &prm,
                                                         p.is_keyframe && !p.mark_on_device ? 1 : 0);
    // A failure leaves up to 8 batches at a time either enqueued or not (svo_hip.h): the collect loop takes
    // every batch that has a pass pending -- its seeds WERE updated -- and skips the others, so nothing stays
    // pending into the next frame.
    if (rc != SVO_HIP_OK) ++st.n_device_errors;
    if (p.mark_on_device) {
      // behind the pass on the stream, one call for the frame's set: the batches whose pass was enqueued
      std::vector<svo_hip_seed_batch*> passed;
      for (size_t j = 0; j < p.devs.size(); ++j)
        if (svo_hip_seed_batch_pending(p.devs[j])) passed.push_back(p.devs[j]);
      if (!passed.empty() && markUpdated(mode, passed, device_grid) != SVO_HIP_OK) ++st.n_device_errors;
    }
  }

 public:
  /// What phase 1 hands to the device call and to the collect loop of one frame
  struct Pass {
    SeedBatchStats st;
    svo_hip_camera cam;
    int cur_slot = -1;
    double T_cur[7];
    bool is_keyframe = false, mark_on_device = false;
    std::vector<svo_hip_seed_batch*> devs;     // the batches of the pass, list order ...
    std::vector<int> slots;                    // ... their keyframes' pyramid slots ...
    std::vector<double> T_refs;                // ... and poses [7] each
    std::vector<size_t> enqueued;              // their positions in the mirror
  };

  /// Phase 1: the list against the mirror (new seeds, foreign erasures), age-out (:256-261), and the batches, slots and poses of
  /// the frame's pass.  false: update() ends here with p.st (halted, nothing to update, no slot for the frame, a device error).
  template <class Host, class Frame>
  bool preparePass(Host& host, svo_hip_ctx* ctx, SeedList& seeds, Frame& frame, int batch_counter, int max_n_kfs, const volatile bool& halt,
                   int sub_batch, const DeviceGrid* device_grid, Pass& p) {
    SeedBatchStats& st = p.st;
    if (sub_batch < 1) sub_batch = 1;
    if (halt) { st.halted = true; return false; }
    // ---- the list against the mirror: new seeds (initializeSeeds pushed a keyframe's batch) or foreign erasures
    const int back_id = seeds.empty() ? -1 : seeds.back().id;
    if (seeds.size() != known_size_ || back_id != known_back_id_) {
      if (!reconcile(host, ctx, seeds, sub_batch, st)) { ++st.n_device_errors; return false; }
    }
    // ---- age-out (:256-261): batches older than max_n_kfs keyframes leave the list and the device
    for (size_t k = 0; k < batches_.size();) {
      if (halt) { st.halted = true; remember(seeds); return false; }
      Batch& b = batches_[k];
      if ((batch_counter - b.batch_id) > max_n_kfs) {
        for (size_t i = 0; i < b.its.size(); ++i)
          if (b.alive[i]) { where_.erase(&*b.its[i]); seeds.erase(b.its[i]); ++st.n_aged_out; }
        svo_hip_seed_batch_destroy(b.dev);
        batches_.erase(batches_.begin() + (std::ptrdiff_t)k);
      } else {
        ++k;
      }
    }
    for (size_t k = 0; k < batches_.size(); ++k) st.n_seeds += batches_[k].n_alive;
    remember(seeds);
    if (batches_.empty()) return false;

    p.cam = host.camera(frame);
    p.cur_slot = host.currentSlot(frame);
    if (p.cur_slot < 0) return false;
    host.pose7(frame, p.T_cur);
    p.is_keyframe = host.isKeyframe(frame);
    p.mark_on_device = p.is_keyframe && device_grid != NULL;    // the grid marks of :302-306 stay on the device

    if (halt) { st.halted = true; return false; }
    // the keyframes of every batch with live seeds, resolved TOGETHER: a slot handed out for one keyframe of this pass must
    // not be recycled for another (with more keyframes alive than the cache had slots, a one-at-a-time look-up did that,
    // and the first keyframe's seeds were matched against the second one's image)
    typedef decltype(((SeedT*)0)->ftr->frame) FramePtrT;
    std::vector<FramePtrT> kfs;
    std::vector<size_t> which;
    for (size_t k = 0; k < batches_.size(); ++k)
      if (batches_[k].n_alive != 0) { kfs.push_back(batches_[k].kf); which.push_back(k); }
    std::vector<int> kf_slots;
    if (!kfs.empty() && !host.keyframeSlots(kfs, kf_slots)) { ++st.n_device_errors; return false; }
    for (size_t j = 0; j < which.size(); ++j) {
      Batch& b = batches_[which[j]];
      if (kf_slots[j] < 0) continue;
      double T_ref[7];
      host.pose7(*b.kf, T_ref);
      p.devs.push_back(b.dev); p.slots.push_back(kf_slots[j]); p.T_refs.insert(p.T_refs.end(), T_ref, T_ref + 7);
      p.enqueued.push_back(which[j]);
    }
    return true;
  }

  /// Phase 3: the events of the batches whose pass was enqueued, in list order: grid marks, callbacks, erasures (:302-337); batches
  /// without a live seed are dropped.
  template <class Host>
  void collectPass(Host& host, SeedList& seeds, Pass& p) {
    SeedBatchStats& st = p.st;
    for (size_t e = 0; e < p.enqueued.size(); ++e) {
      Batch& b = batches_[p.enqueued[e]];
      const svo_hip_seed_event* ev = NULL;
      int n_ev = 0;
      int32_t counts[7];
      if (st.n_device_errors && !svo_hip_seed_batch_pending(b.dev)) continue;      // (not reached by a failed group call)
      if (svo_hip_seed_batch_collect(b.dev, &ev, &n_ev, counts) != SVO_HIP_OK) { ++st.n_device_errors; continue; }
      st.n_failed_matches += counts[SVO_HIP_SEED_NO_MATCH + 1];
      st.n_updated += counts[SVO_HIP_SEED_UPDATED + 1] + counts[SVO_HIP_SEED_CONVERGED + 1] + counts[SVO_HIP_SEED_NAN + 1];
      for (int j = 0; j < n_ev; ++j) {
        const svo_hip_seed_event& x = ev[j];
        if (x.index < 0 || (size_t)x.index >= b.its.size() || !b.alive[(size_t)x.index]) continue;
        It it = b.its[(size_t)x.index];
        if (p.is_keyframe && !p.mark_on_device) host.setGridOccupancy(x.px_cur);   // :302-306
        if (x.status == SVO_HIP_SEED_CONVERGED) {                   // :310-331
          it->mu = x.mu; it->sigma2 = x.sigma2;
          host.converged(*it, x.xyz_world);
          forget(b, (size_t)x.index, seeds);
          ++st.n_converged;
        } else if (x.status == SVO_HIP_SEED_NAN) {                  // :333-337
          forget(b, (size_t)x.index, seeds);
          ++st.n_nan;
        }
      }
    }
    // batches without a live seed are of no further use
    for (size_t k = 0; k < batches_.size();) {
      if (batches_[k].n_alive == 0) { svo_hip_seed_batch_destroy(batches_[k].dev); batches_.erase(batches_.begin() + (std::ptrdiff_t)k); }
      else ++k;
    }
    remember(seeds);
  }

  /// A batch that was created on the device from a detection (svo_hip_seed_batch_create_detected) joins the mirror: the n
  /// list entries the host has just pushed for it, `first` onwards, are its seeds 0..n-1 (batch id `batch_id`, keyframe `kf`).
  /// The mirror owns the batch from here on.  As after reconcile(): the entries are known (where_), the batch stands at the end
  /// of the batches -- the entries stand at the end of the list -- and the list's size and last id are remembered, so the next
  /// update() finds nothing fresh and uploads nothing.  To be called with the mirror in line with the list as it was before
  /// the n entries were pushed (update() leaves it so; an erasure behind the mirror's back in between is still noticed by the
  /// next update(), which then re-reads the list).
  template <class FramePtrT>
  void adopt(svo_hip_seed_batch* batch, It first, size_t n, int batch_id, FramePtrT kf) {
    if (batch == NULL) return;
    if (n == 0) { svo_hip_seed_batch_destroy(batch); return; }
    Batch nb;
    nb.serial = next_serial_++;
    nb.batch_id = batch_id;
    nb.kf = kf;
    nb.dev = batch;
    nb.its.reserve(n);
    It it = first;
    for (size_t i = 0; i < n; ++i, ++it) {
      nb.its.push_back(it);
      Where w; w.batch_serial = nb.serial; w.index = (int)i; w.id = it->id;
      where_[&*it] = w;
    }
    nb.alive.assign(n, 1);
    nb.n_alive = (int)n;
    known_size_ += n;
    known_back_id_ = nb.its.back()->id;
    batches_.push_back(nb);
  }

  /// Copy the device state (a, b, mu, sigma2) of every live seed into its list entry: before the host reads the list
  /// (getSeeds() / getSeedsCopy()).  Returns false on a device error.
  bool syncToHost() {
    std::vector<float> a, b, mu, s2;
    for (size_t k = 0; k < batches_.size(); ++k) {
      Batch& bt = batches_[k];
      const size_t n = bt.its.size();
      a.resize(n); b.resize(n); mu.resize(n); s2.resize(n);
      if (svo_hip_seed_batch_download(bt.dev, a.data(), b.data(), mu.data(), s2.data(), NULL) != SVO_HIP_OK) return false;
      for (size_t i = 0; i < n; ++i)
        if (bt.alive[i]) { It it = bt.its[i]; it->a = a[i]; it->b = b[i]; it->mu = mu[i]; it->sigma2 = s2[i]; }
    }
    return true;
  }

 private:
  struct Batch {
    size_t serial;                       // never reused: what where_ refers to
    int batch_id;                        // Seed::batch_id of its seeds (age-out)
    decltype(((SeedT*)0)->ftr->frame) kf;   // the reference keyframe (Frame*)
    svo_hip_seed_batch* dev;
    std::vector<It> its;                 // device index -> list entry
    std::vector<uint8_t> alive;          // ... still in the list
    int n_alive;
  };
  struct Where { size_t batch_serial; int index; int id; };   // id: Seed::id (a recycled list node is another seed)

  std::vector<Batch> batches_;                           // list order (= creation order of the keyframes' seed batches)
  std::unordered_map<const SeedT*, Where> where_;        // list node -> (its batch, index): the re-build after foreign erasures
  size_t next_serial_ = 0;
  size_t known_size_ = 0;
  int known_back_id_ = -1;

  void remember(const SeedList& seeds) {
    known_size_ = seeds.size();
    known_back_id_ = seeds.empty() ? -1 : seeds.back().id;
  }
  void forget(Batch& b, size_t index, SeedList& seeds) {
    where_.erase(&*b.its[index]);
    seeds.erase(b.its[index]);
    b.alive[index] = 0;
    --b.n_alive;
  }

  /// Bring the mirror in line with the list: seeds the mirror does not know become new device batches (per keyframe batch
  /// id, chunks of at most sub_batch, list order); mirrored seeds that left the list are erased on the device.
  template <class Host>
  bool reconcile(Host& host, svo_hip_ctx* ctx, SeedList& seeds, int sub_batch, SeedBatchStats& st) {
    // present[k][i]: list entries found for batch k
    std::vector<std::vector<uint8_t> > present(batches_.size());
    for (size_t k = 0; k < batches_.size(); ++k) present[k].assign(batches_[k].its.size(), 0);
    std::unordered_map<size_t, size_t> pos_of_serial;
    for (size_t k = 0; k < batches_.size(); ++k) pos_of_serial[batches_[k].serial] = k;
    std::vector<It> fresh;                                         // list entries without a mirror, list order
    for (It it = seeds.begin(); it != seeds.end(); ++it) {
      typename std::unordered_map<const SeedT*, Where>::const_iterator w = where_.find(&*it);
      if (w == where_.end() || w->second.id != it->id) { fresh.push_back(it); continue; }
      present[pos_of_serial[w->second.batch_serial]][(size_t)w->second.index] = 1;
    }
    // foreign erasures
    std::vector<int32_t> gone;
    for (size_t k = 0; k < batches_.size(); ++k) {
      Batch& b = batches_[k];
      gone.clear();
      for (size_t i = 0; i < b.its.size(); ++i)
        if (b.alive[i] && !present[k][i]) { gone.push_back((int32_t)i); b.alive[i] = 0; --b.n_alive; }
      if (!gone.empty()) {
        st.resynced = true;
        if (svo_hip_seed_batch_erase(b.dev, (int)gone.size(), gone.data()) != SVO_HIP_OK) return false;
      }
    }
    if (st.resynced) {                                             // stale node addresses must not alias new seeds
      for (typename std::unordered_map<const SeedT*, Where>::iterator w = where_.begin(); w != where_.end();) {
        const Batch& b = batches_[pos_of_serial[w->second.batch_serial]];
        if (!b.alive[(size_t)w->second.index]) w = where_.erase(w); else ++w;
      }
    }
    for (size_t k = 0; k < batches_.size();) {
      if (batches_[k].n_alive == 0) { svo_hip_seed_batch_destroy(batches_[k].dev); batches_.erase(batches_.begin() + (std::ptrdiff_t)k); }
      else ++k;
    }
    // new seeds: runs of equal (batch id, keyframe), chunked
    std::vector<double> px, f;
    std::vector<int32_t> level;
    std::vector<float> a, b, mu, zr, s2;
    size_t first = 0;
    while (first < fresh.size()) {
      size_t last = first + 1;
      while (last < fresh.size() && last - first < (size_t)sub_batch && fresh[last]->batch_id == fresh[first]->batch_id &&
             host.keyframeOf(*fresh[last]) == host.keyframeOf(*fresh[first])) ++last;
      const size_t n = last - first;
      px.resize(2 * n); f.resize(3 * n); level.resize(n); a.resize(n); b.resize(n); mu.resize(n); zr.resize(n); s2.resize(n);
      for (size_t i = 0; i < n; ++i) {
        const It it = fresh[first + i];
        int lvl = 0;
        host.feature(*it, &px[2 * i], &f[3 * i], &lvl);
        level[i] = lvl;
        a[i] = it->a; b[i] = it->b; mu[i] = it->mu; zr[i] = it->z_range; s2[i] = it->sigma2;
      }
      Batch nb;
      nb.batch_id = fresh[first]->batch_id;
      nb.kf = host.keyframeOf(*fresh[first]);
      nb.dev = NULL;
      if (svo_hip_seed_batch_create(ctx, (int)n, px.data(), f.data(), level.data(), a.data(), b.data(), mu.data(), zr.data(), s2.data(),
                                    &nb.dev) != SVO_HIP_OK) return false;
      nb.its.assign(fresh.begin() + (std::ptrdiff_t)first, fresh.begin() + (std::ptrdiff_t)last);
      nb.alive.assign(n, 1);
      nb.n_alive = (int)n;
      nb.serial = next_serial_++;
      for (size_t i = 0; i < n; ++i) { Where w; w.batch_serial = nb.serial; w.index = (int)i; w.id = nb.its[i]->id; where_[&*nb.its[i]] = w; }
      // batches_ stays in list order: new seeds are pushed to the back of the list, so a new batch goes to the end
      batches_.push_back(nb);
      st.n_uploaded += (int)n;
      first = last;
    }
    return true;
  }
};

/// DepthFilter::updateSeeds for SEVERAL cameras of one context -- camera c: mirror, host policy, seed list, frame and batch
/// counter number c -- with ONE device call for all of them (svo_hip_seed_batch_update_cameras_async): phase 1 per mirror in
/// camera order, the call, phase 3 per mirror in camera order, so that every camera's callbacks, grid marks and erasures come in
/// the order of its own update().  One pair of pyramid batches for all cameras (those of camera 0's host); a keyframe's updated
/// seeds are reported to Host::setGridOccupancy (no device grid here).
/// updateCameras() is for cameras that share ONE camera model (that of the first camera with a pass); updateCameraRig() below takes
/// every camera's own model from its host (Host::camera of its frame: same image size, own intrinsics and distortion).
/// The hosts must SHARE their two pyramid caches: the call takes the batches of hosts[0] for every camera's slots, and nothing here
/// can check that.  With shared caches a later camera's keyframeSlots() / currentSlot() must not recycle a slot an earlier camera of
/// the same pass was given: the caller makes every frame of the pass resident TOGETHER before this call, so that the cameras'
/// look-ups only find resident frames (svo::DepthFilterGroup::addFrames does; slot_table.h: a resident frame keeps its slot).  stats[c]: as update() returns them;
/// n_device_calls counts the camera's batches in the call.  (The only users of the two entry points in this header: code that
/// never instantiates a template need not link what it calls.)
// the device call of a pass: RIG = false knows one model only; RIG = true takes the rig call when the models differ
template <bool RIG> struct CamerasCall;
template <> struct CamerasCall<false> {
  static int run(svo_hip_ctx* ctx, int n, const svo_hip_seed_camera_pass* passes, const svo_hip_pyramid* ref, const svo_hip_pyramid* cur,
                 const svo_hip_camera* models, const svo_hip_camera* first, const svo_hip_df_params* prm) {
    (void)models;
    return svo_hip_seed_batch_update_cameras_async(ctx, n, passes, ref, cur, first, prm);
  }
};
template <> struct CamerasCall<true> {
  static int run(svo_hip_ctx* ctx, int n, const svo_hip_seed_camera_pass* passes, const svo_hip_pyramid* ref, const svo_hip_pyramid* cur,
                 const svo_hip_camera* models, const svo_hip_camera* first, const svo_hip_df_params* prm) {
    if (oneCameraModel(models, (size_t)n)) return svo_hip_seed_batch_update_cameras_async(ctx, n, passes, ref, cur, first, prm);
    return svo_hip_seed_batch_update_rig_async(ctx, n, passes, ref, cur, models, prm);
  }
};

template <bool RIG, class Mirror, class Host, class SeedList, class Frame>
void updateCamerasWith(size_t n_cameras, Mirror* const* mirrors, Host* const* hosts, svo_hip_ctx* ctx, SeedList* const* seeds, Frame* const* frames,
                       const svo_hip_df_params& prm, const int* batch_counters, int max_n_kfs, const volatile bool& halt, SeedBatchStats* stats,
                       int sub_batch) {
  std::vector<typename Mirror::Pass> passes(n_cameras);
  std::vector<svo_hip_seed_camera_pass> cams(n_cameras);
  std::vector<svo_hip_camera> models(n_cameras);             // camera c's model; a camera that sits out gets the first one's (its size)
  std::vector<uint8_t> runs(n_cameras, 0);
  const svo_hip_camera* cam = NULL;
  for (size_t c = 0; c < n_cameras; ++c) {
    typename Mirror::Pass& p = passes[c];
    svo_hip_seed_camera_pass& cp = cams[c];
    cp.n_batches = 0; cp.batches = NULL; cp.ref_slots = NULL; cp.T_ref_w = NULL; cp.cur_slot = 0; cp.report_updated = 0;
    for (int i = 0; i < 7; ++i) cp.T_cur_w[i] = 0.0;
    runs[c] = mirrors[c]->preparePass(*hosts[c], ctx, *seeds[c], *frames[c], batch_counters[c], max_n_kfs, halt, sub_batch, NULL, p) ? 1 : 0;
    if (!runs[c] || p.devs.empty()) continue;
    cp.n_batches = (int)p.devs.size(); cp.batches = p.devs.data(); cp.ref_slots = p.slots.data(); cp.T_ref_w = p.T_refs.data();
    cp.cur_slot = p.cur_slot; cp.report_updated = p.is_keyframe ? 1 : 0;
    for (int i = 0; i < 7; ++i) cp.T_cur_w[i] = p.T_cur[i];
    p.st.n_device_calls += cp.n_batches;
    if (!cam) cam = &p.cam;
  }
  if (cam) {
    for (size_t c = 0; c < n_cameras; ++c) models[c] = cams[c].n_batches ? passes[c].cam : *cam;
    const int rc = CamerasCall<RIG>::run(ctx, (int)n_cameras, cams.data(), hosts[0]->keyframePyramids(), hosts[0]->currentPyramids(), models.data(),
                                         cam, &prm);
    // a refused or failed call has enqueued nothing or has waited for what it had: the collect loops skip batches without a pass
    if (rc != SVO_HIP_OK)
      for (size_t c = 0; c < n_cameras; ++c) if (cams[c].n_batches) ++passes[c].st.n_device_errors;
  }
  for (size_t c = 0; c < n_cameras; ++c) {
    if (runs[c]) mirrors[c]->collectPass(*hosts[c], *seeds[c], passes[c]);
    stats[c] = passes[c].st;
  }
}

template <class Mirror, class Host, class SeedList, class Frame>
void updateCameras(size_t n_cameras, Mirror* const* mirrors, Host* const* hosts, svo_hip_ctx* ctx, SeedList* const* seeds, Frame* const* frames,
                   const svo_hip_df_params& prm, const int* batch_counters, int max_n_kfs, const volatile bool& halt, SeedBatchStats* stats,
                   int sub_batch = 4096) {
  updateCamerasWith<false>(n_cameras, mirrors, hosts, ctx, seeds, frames, prm, batch_counters, max_n_kfs, halt, stats, sub_batch);
}

/// updateCameras() for a camera rig: camera c's pass goes with the model its host gives for its frame.  Equal models make the
/// call updateCameras() makes (svo_hip_seed_batch_update_cameras_async); models that differ make ONE
/// svo_hip_seed_batch_update_rig_async call.
template <class Mirror, class Host, class SeedList, class Frame>
void updateCameraRig(size_t n_cameras, Mirror* const* mirrors, Host* const* hosts, svo_hip_ctx* ctx, SeedList* const* seeds, Frame* const* frames,
                     const svo_hip_df_params& prm, const int* batch_counters, int max_n_kfs, const volatile bool& halt, SeedBatchStats* stats,
                     int sub_batch = 4096) {
  updateCamerasWith<true>(n_cameras, mirrors, hosts, ctx, seeds, frames, prm, batch_counters, max_n_kfs, halt, stats, sub_batch);
}

}  // namespace hip_bridge
}  // namespace svo

#endif  // SVO_DROPIN_DEPTH_FILTER_BATCH_H_
