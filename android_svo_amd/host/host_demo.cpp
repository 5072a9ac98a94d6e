// host_demo.cpp -- runs the C++ host layer (svo_host.h) end to end on the GPU: one SparseImgAlign::run,
// the DepthFilter protocol synchronously, then again with its worker thread while the main thread keeps
// aligning frames (two host threads, two svo_hip contexts, as in the reference: SURVEY 8b "Threading").
// Usage: svo_host_demo <case_dir> <out_dir>      (inputs written by tests/test_gpu_host_cpp.py)
//        svo_host_demo <case_dir> <out_dir> track   the tracking chain: svo::FrameTracker (hip_bridge::FrameTrackerT on this
//                                                   file's data model) over a map built as an object graph from index tables
//        svo_host_demo <case_dir> <out_dir> trackgroup [n]   the same tracking chain for n (default 2) copies of the world at once through
//                                                   svo::FrameTrackerGroup (hip_bridge::FrameTrackerGroupT, svo_hip_tracker_group): outputs of
//                                                   world w under <out_dir>/g<w>/, each equal to the lone tracker's
//        svo_host_demo <case_dir> <out_dir> trackgroup n rig   a camera rig: world w is the case <case_dir>/cam<w> with a camera model of its
//                                                   own (track_manifest.bin, optional track_dist.bin: k1 k2 p1 p2 k3); outputs under
//                                                   <out_dir>/g<w>/, each equal to `track` on <case_dir>/cam<w>
//        svo_host_demo <case_dir> <out_dir> keyframes [device_seeds] [threaded]   keyframes whose seeds the filter detects and creates
//                                                   on the device, or (without device_seeds) are detected by the caller and handed in
//        svo_host_demo <case_dir> <out_dir> trackgroup n staggered   the worlds of the group do not advance together: world w takes part in
//                                                   every (w + 1)-th call of the group (FrameTrackerGroup::trackSome, svo_hip_tracker_group_track_some)
//                                                   and sits the others out; the same outputs as trackgroup, and group_schedule.bin
//        svo_host_demo <case_dir> <out_dir> filtergroup   svo::DepthFilterGroup: the depth filters of n cameras as one device pass per
//                                                   step, and a lone DepthFilter per camera over the same frames (filter_group_demo);
//                                                   `filtergroup rig`: every camera with the model of <case_dir>/cam<c>/camera.bin
//        svo_host_demo <case_dir> <out_dir> churn   SURVEY 8(b) "Threading": latency of SparseImgAlign::run on the tracking
//                                                   thread while a second thread (own context) creates seed batches, runs a
//                                                   pass and drops them at keyframe rate -- and with that thread idle
//        svo_host_demo <case_dir> <out_dir> klt     the bootstrap of n cameras: svo::initialization::KltInit (hip_bridge::KltInitT,
//                                                   svo_hip_klt_*) over klt_meta.bin / klt_images.bin / klt_px.bin -- camera 0's first
//                                                   frame detected on the device, the others from the given features -- then three
//                                                   frames, each ONE device call for all cameras; the lists of camera c after frame k
//                                                   under <out_dir>/klt_c<c>_k<k>_*.bin, the return codes in klt_results.bin
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <map>
#include <string>
#include <sys/stat.h>

#include "svo_host.h"

using namespace svo;

template <typename T>
static std::vector<T> read_bin(const std::string& path) {
  std::ifstream f(path, std::ios::binary | std::ios::ate);
  if (!f) throw std::runtime_error("cannot open " + path);
  const std::streamsize n = f.tellg();
  f.seekg(0);
  std::vector<T> v((size_t)n / sizeof(T));
  f.read(reinterpret_cast<char*>(v.data()), n);
  return v;
}
template <typename T>
static void write_bin(const std::string& path, const std::vector<T>& v) {
  std::ofstream f(path, std::ios::binary);
  f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

struct Case {
  PinholeCamera cam;
  int n_levels, n_frames;
  std::vector<FramePtr> frames;
};

static FramePtr load_frame(const std::string& dir, const PinholeCamera* cam, int k, int n_levels) {
  std::vector<std::vector<uint8_t>> pyr;
  for (int l = 0; l < n_levels; ++l) pyr.push_back(read_bin<uint8_t>(dir + "/frame_" + std::to_string(k) + "_L" + std::to_string(l) + ".bin"));
  FramePtr f = std::make_shared<Frame>(cam, std::move(pyr));
  f->T_f_w_ = SE3(read_bin<double>(dir + "/frame_" + std::to_string(k) + "_pose.bin").data());
  return f;
}

static void dump_filter(DepthFilter& df, const std::map<Feature*, int>& index, const std::vector<double>& conv,
                        const std::string& out, const std::string& tag) {
  std::vector<double> rows;
  for (const Seed& s : df.getSeeds()) {
    rows.push_back((double)index.at(s.ftr)); rows.push_back(s.a); rows.push_back(s.b); rows.push_back(s.mu); rows.push_back(s.sigma2);
  }
  write_bin(out + "/" + tag + "_seeds.bin", rows);
  write_bin(out + "/" + tag + "_conv.bin", conv);
}

// ---- svo::FrameTracker over a svo::Map: the object graph (frames, features, points with their observation lists,
// point candidates) is built from the index tables the test wrote, the frames are tracked one after the other (each
// tracked frame is the next one's last frame), and what the tracker left on the objects is written out as tables again.
// What track_demo tracks through: a lone svo::FrameTracker, or camera w of a svo::FrameTrackerGroup.  In a group the worlds run on
// one thread each but in lockstep: a thread only runs while it holds the rendezvous' mutex (the C-ABI context is one host thread's
// at a time), gives it up inside track() and goes on when the group call -- made by the last world to arrive -- has returned.
typedef hip_bridge::FrameTrackerT<HostTrackerPolicy> TrackerCamera;
struct GroupRendezvous {
  std::mutex mu;
  std::condition_variable cv;
  FrameTrackerGroup* group = nullptr;
  size_t n = 0, arrived = 0, failed = 0;                // failed: worlds that gave up (the others must not wait for them)
  unsigned long generation = 0;
  bool ok = true;
  std::vector<FramePtr> last, cur;
  std::vector<Map*> maps;
  std::vector<std::vector<std::pair<FramePtr, size_t>>> overlap;
  std::vector<TrackerCamera::Outcome> out;
  // a staggered schedule (trackgroup n staggered): the group's calls are numbered, world w takes part in call t when t is a multiple
  // of w + 1 -- world 0 in every call, world 1 in every other one, ... -- until it has run out of frames; the cameras of a call go
  // through FrameTrackerGroup::trackSome, the others sit it out
  bool staggered = false;
  unsigned long tick = 0;
  std::vector<char> waiting, finished;                  // per world: its frame waits for its call / it has no frame left
  std::vector<double> schedule;                         // the calls made: per call the tick and the worlds' membership (n entries of 0 / 1)
  bool inCall(size_t w) const { return !finished[w] && tick % (w + 1) == 0; }
  /// make every call whose worlds have all arrived (called with the mutex held, by whichever world moved last)
  void fire() {
    while (ok && !failed) {
      std::vector<int> active;
      bool all_here = true, anybody_left = false;
      for (size_t w = 0; w < n; ++w) {
        anybody_left = anybody_left || !finished[w];
        if (!inCall(w)) continue;
        active.push_back((int)w);
        all_here = all_here && waiting[w];
      }
      if (!anybody_left || !all_here) return;
      if (!active.empty()) {
        ok = group->trackSome(active, last, cur, maps, overlap, out);
        schedule.push_back((double)tick);
        for (size_t w = 0; w < n; ++w) schedule.push_back(std::find(active.begin(), active.end(), (int)w) != active.end() ? 1.0 : 0.0);
        for (int w : active) waiting[(size_t)w] = 0;
        cv.notify_all();
      }
      ++tick;
    }
  }
};
struct TrackerPort {
  FrameTracker* lone = nullptr;
  GroupRendezvous* rz = nullptr;
  std::unique_lock<std::mutex>* baton = nullptr;       // the world thread's hold on rz->mu
  size_t w = 0;
  TrackerCamera& camera() { return lone ? static_cast<TrackerCamera&>(*lone) : rz->group->camera(w); }
  bool track(const FramePtr& last, const FramePtr& cur, Map& map, std::vector<std::pair<FramePtr, size_t>>& overlap, TrackerCamera::Outcome& oc) {
    if (lone) return lone->track(last, cur, map, overlap, oc);
    GroupRendezvous& r = *rz;
    if (r.failed) return false;
    r.last[w] = last; r.cur[w] = cur; r.maps[w] = &map;
    if (r.staggered) {
      r.waiting[w] = 1;
      r.fire();
      r.cv.wait(*baton, [&]() { return !r.waiting[w] || r.failed || !r.ok; });
      if (r.failed || !r.ok) return false;
      overlap = r.overlap[w]; oc = r.out[w];
      return true;
    }
    const unsigned long my_gen = r.generation;
    if (++r.arrived == r.n) {
      r.ok = r.group->trackAll(r.last, r.cur, r.maps, r.overlap, r.out);
      r.arrived = 0;
      ++r.generation;
      r.cv.notify_all();
    } else {
      r.cv.wait(*baton, [&]() { return r.generation != my_gen; });
      if (r.failed) return false;
    }
    if (r.ok) { overlap = r.overlap[w]; oc = r.out[w]; }
    return r.ok;
  }
};

static svo_hip_tracker_config track_config(const std::vector<double>& m, int max_kfs = 0, int max_points = 0) {
  svo_hip_tracker_config cfg;
  svo_hip_tracker_default_config(&cfg);
  cfg.max_keyframes = (int)m[6] + 2;                                          // room for a frame that becomes a keyframe
  if (cfg.max_keyframes < max_kfs + 1) cfg.max_keyframes = max_kfs + 1;      // (the new keyframe joins before the furthest one leaves)
  cfg.grid_size = (int)m[12]; cfg.max_fts = (int)m[13]; cfg.quality_min_fts = (int)m[14];
  cfg.klt_min_level = (int)m[15]; cfg.max_frame_features = (int)m[16];
  if (max_points > 0) cfg.max_points = max_points;
  return cfg;
}

// incremental: FrameTracker::setIncrementalMap -- new candidates and a promoted keyframe reach the device in place, and the
// promotion also runs MapPointCandidates::addCandidatePointToFrame (processFrame :276) on the objects.  times: the host-side
// duration of every track() call in microseconds goes to times_track.bin.  kf_every E: not only the manifest's frame
// keyframe_at becomes a keyframe but every E-th frame from it on.  max_kfs N (Config::maxNKfs(), > 2): once the map holds N
// keyframes the one furthest from the new keyframe leaves first (processFrame :303-308: getFurthestKeyframe, safeDeleteFrame),
// which reaches the device through FrameTracker::keyframeRemoved; full_remove: through mapChanged() instead (a full upload, the
// yardstick).  A frame whose pose is NaN (tracking was lost) has no furthest keyframe, and the reference would let the map grow:
// the demo stops there.  track_removed.bin: per frame, which keyframe left (in order of creation), or -1; track_map_size.bin: the map at the end.
// new_seeds S: every frame that becomes a keyframe seeds S point candidates behind the tracker's back, as the depth filter's thread
// does when seeds of that keyframe converge: twins of the first S of its features that have a point, a tenth of a millimetre
// off.  They reach the device with the next frame; those that are not matched and promoted go with their keyframe, so with max_kfs
// the living points stay bounded while the rows of the device's point tables grow.  max_points N: svo_hip_tracker_config::max_points.
// compact: FrameTracker::setPointCompaction.  map_compactions.bin: per frame, the compactions so far (beside track_uploads.bin);
// map_points_room.bin: the largest (living points + candidates waiting to be appended) at the end of a frame, and the rows of
// the device's point tables at the end.
// reloc_at K: frame K is not tracked from the last frame but relocalised (svo::relocalizeFrame: FrameHandlerMono::relocalizeFrame
// against Map::getClosestKeyframe(last_frame_)) with FrameTracker::setDeviceRelocalisation -- keyframe choice, gate and tracking in
// one device call.  track_reloc.bin: the result (UpdateResult), the reference keyframe (in order of creation, -1: none), how many
// device relocalisations the bridge made, gate_n_tracked, accepted, n_close, the gate's pose.
// Manifest field 21 (optional), kf_select_min_dist > 0 (Config::kfSelectMinDist()): every tracked frame is finished with
// FrameTracker::finishFrame -- optimizeStructure(frame, field 18 or 20 points, 5 iterations) and the keyframe decision in one device
// call -- and the host twins (frame_utils::getSceneDepth, needNewKf, Map::getFurthestKeyframe) decide again on the objects, which
// hold the positions the call wrote.  track_decision.bin, 13 doubles per frame: the device's have_depth, depth_mean, depth_min,
// overlap_valid, need_new_kf, furthest keyframe (in order of creation, -1: none), the host's six, and the device decisions so far.
// With max_kfs the keyframe that leaves is the one the device named; the run throws if the host names another.
// the camera of a tracking case: the manifest's size and intrinsics, and the radtan coefficients of track_dist.bin where the case has one
static PinholeCamera track_camera(const std::string& dir, const std::vector<double>& m) {
  PinholeCamera cam{(int)m[0], (int)m[1], m[2], m[3], m[4], m[5]};
  struct stat st;
  if (::stat((dir + "/track_dist.bin").c_str(), &st) == 0) {
    const std::vector<double> d = read_bin<double>(dir + "/track_dist.bin");
    for (size_t k = 0; k < 5 && k < d.size(); ++k) cam.d[k] = d[k];
  }
  return cam;
}

static int track_demo(const std::string& dir, const std::string& out, TrackerPort& port, bool incremental = false, bool times = false,
                      int max_kfs = 0, bool full_remove = false, int kf_every = 0, bool compact = false, int new_seeds = 0, int reloc_at = -1) {
  const std::vector<double> m = read_bin<double>(dir + "/track_manifest.bin");
  PinholeCamera cam = track_camera(dir, m);
  const int n_kf = (int)m[6], n_points = (int)m[7], n_obs = (int)m[8], n_cand = (int)m[10], n_frames = (int)m[11];
  const auto kf_pose = read_bin<double>(dir + "/kf_pose.bin"), pt_pos = read_bin<double>(dir + "/pt_pos.bin");
  const auto pt_type = read_bin<int32_t>(dir + "/pt_type.bin"), pt_failed = read_bin<int32_t>(dir + "/pt_n_failed.bin"),
             pt_succ = read_bin<int32_t>(dir + "/pt_n_succeeded.bin"), pt_obs_offset = read_bin<int32_t>(dir + "/pt_obs_offset.bin"),
             obs_point = read_bin<int32_t>(dir + "/obs_point.bin"), obs_kf = read_bin<int32_t>(dir + "/obs_kf.bin"),
             obs_level = read_bin<int32_t>(dir + "/obs_level.bin"), kf_ftr_offset = read_bin<int32_t>(dir + "/kf_ftr_offset.bin"),
             kf_ftr_obs = read_bin<int32_t>(dir + "/kf_ftr_obs.bin"), cand_obs = read_bin<int32_t>(dir + "/cand_obs.bin");
  const auto obs_px = read_bin<double>(dir + "/obs_px.bin"), obs_f = read_bin<double>(dir + "/obs_f.bin"), obs_grad = read_bin<double>(dir + "/obs_grad.bin");
  const auto obs_edgelet = read_bin<uint8_t>(dir + "/obs_edgelet.bin");
  if ((int)obs_point.size() != n_obs || (int)pt_type.size() != n_points || (int)cand_obs.size() != n_cand) throw std::runtime_error("track case: table sizes");

  Map map;
  std::vector<std::unique_ptr<Point>> points;
  std::map<const Point*, int> index_of_point;
  for (int p = 0; p < n_points; ++p) {
    points.emplace_back(new Point(Vector3d{{pt_pos[3 * p], pt_pos[3 * p + 1], pt_pos[3 * p + 2]}}));
    points.back()->type_ = (Point::PointType)pt_type[p];
    points.back()->n_failed_reproj_ = pt_failed[p];
    points.back()->n_succeeded_reproj_ = pt_succ[p];
    index_of_point[points.back().get()] = p;
  }
  std::vector<FramePtr> kfs;
  for (int k = 0; k < n_kf; ++k) {
    std::vector<std::vector<uint8_t>> pyr;
    pyr.push_back(read_bin<uint8_t>(dir + "/kf_" + std::to_string(k) + "_img.bin"));
    kfs.push_back(std::make_shared<Frame>(&cam, std::move(pyr)));
    kfs.back()->T_f_w_ = SE3(&kf_pose[7 * (size_t)k]);
  }
  std::vector<Feature*> feature_of_obs((size_t)n_obs, nullptr);
  auto make_obs_feature = [&](int o) {
    Feature* ftr = new Feature(kfs[obs_kf[o]].get(), Vector2d{{obs_px[2 * o], obs_px[2 * o + 1]}},
                               Vector3d{{obs_f[3 * o], obs_f[3 * o + 1], obs_f[3 * o + 2]}}, obs_level[o]);
    if (obs_edgelet[o]) { ftr->type = Feature::EDGELET; ftr->grad = Vector2d{{obs_grad[2 * o], obs_grad[2 * o + 1]}}; }
    ftr->point = points[obs_point[o]].get();
    feature_of_obs[o] = ftr;
    return ftr;
  };
  for (int k = 0; k < n_kf; ++k)                                               // Frame::fts_ in the keyframe's own order
    for (int j = kf_ftr_offset[k]; j < kf_ftr_offset[k + 1]; ++j) kfs[k]->addFeature(make_obs_feature(kf_ftr_obs[j]));
  for (int c = 0; c < n_cand; ++c) {                                           // candidates: one feature each, in no fts_
    Feature* ftr = make_obs_feature(cand_obs[c]);
    map.point_candidates_.candidates_.push_back(MapPointCandidates::PointCandidate(ftr->point, ftr));
  }
  for (int p = 0; p < n_points; ++p)                                           // Point::obs_ in table order
    for (int o = pt_obs_offset[p]; o < pt_obs_offset[p + 1]; ++o)
      if (feature_of_obs[o]) points[p]->obs_.push_back(feature_of_obs[o]);
  for (int k = 0; k < n_kf; ++k) { kfs[k]->setKeyframe(); map.addKeyframe(kfs[k]); }
  auto key_table = [&]() {
    std::vector<int32_t> key;
    for (int k = 0; k < n_kf; ++k)
      for (int j = 0; j < 5; ++j) { const Feature* kp = kfs[k]->key_pts_[j]; key.push_back(kp && kp->point ? index_of_point.at(kp->point) : -1); }
    return key;
  };
  write_bin(out + "/track_key_before.bin", key_table());

  TrackerCamera& tracker = port.camera();
  if (!tracker.ok()) throw std::runtime_error("svo::FrameTracker: no device tracker");
  tracker.setIncrementalMap(incremental);
  if (compact) tracker.setPointCompaction(true);
  if (reloc_at >= 0) tracker.setDeviceRelocalisation(true);
  std::vector<double> track_us;

  // the last frame: a keyframe of the map, or a frame of its own without features (SparseImgAlign::run then returns at once)
  const int last_kf = (int)m[17];
  FramePtr last;
  if (last_kf >= 0) {
    last = kfs[last_kf];
  } else {
    std::vector<std::vector<uint8_t>> pyr;
    pyr.push_back(read_bin<uint8_t>(dir + "/last_img.bin"));
    last = std::make_shared<Frame>(&cam, std::move(pyr));
    last->T_f_w_ = SE3(read_bin<double>(dir + "/last_pose.bin").data());
  }
  std::vector<double> poses, stats, overlap, uploads, removed, compactions;
  size_t room_needed = 0;
  const int keyframe_at = m.size() > 19 ? (int)m[19] : -1;
  const double kf_select_min_dist = m.size() > 21 ? m[21] : 0.0;
  const bool decide = kf_select_min_dist > 0.0;
  std::vector<double> decisions;
  for (int k = 0; k < n_frames; ++k) {
    std::vector<std::vector<uint8_t>> pyr;
    pyr.push_back(read_bin<uint8_t>(dir + "/trk_frame_" + std::to_string(k) + ".bin"));
    FramePtr cur = std::make_shared<Frame>(&cam, std::move(pyr));
    std::vector<std::pair<FramePtr, size_t>> overlap_kfs;
    FrameTracker::Outcome oc;
    const auto t0 = std::chrono::steady_clock::now();
    if (k == reloc_at) {
      oc = FrameTracker::Outcome();
      const UpdateResult res = relocalizeFrame(tracker, map, last, cur, FramePtr(), overlap_kfs, oc, (size_t)m[14]);
      const svo_hip_reloc_result& rr = tracker.lastRelocalisation();
      double ref = -1.0;
      for (size_t j = 0; j < kfs.size(); ++j) if (res != RESULT_FAILURE && kfs[j] == last) ref = (double)j;
      std::vector<double> rel{(double)res, ref, (double)tracker.deviceRelocalisations(), (double)rr.gate_n_tracked, (double)rr.accepted, (double)rr.n_close};
      rel.insert(rel.end(), rr.T_f_w_gate, rr.T_f_w_gate + 7);
      write_bin(out + "/track_reloc.bin", rel);
    } else
    if (!port.track(last, cur, map, overlap_kfs, oc)) throw std::runtime_error("svo::FrameTracker::track failed at frame " + std::to_string(k));
    track_us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    poses.insert(poses.end(), cur->T_f_w_.p, cur->T_f_w_.p + 7);
    stats.insert(stats.end(), {(double)cur->fts_.size(), (double)oc.repr_n_matches, (double)oc.repr_n_trials, (double)oc.img_align_n_tracked,
                               oc.pose_optimised ? 1.0 : 0.0, (double)oc.sfba_n_edges_final, oc.sfba_error_init, oc.sfba_error_final, (double)overlap_kfs.size()});
    std::vector<double> fpx, fgrad;
    std::vector<int32_t> flevel, fpoint;
    std::vector<uint8_t> fedge;
    for (const Feature* ftr : cur->fts_) {
      fpx.push_back(ftr->px[0]); fpx.push_back(ftr->px[1]);
      fgrad.push_back(ftr->grad[0]); fgrad.push_back(ftr->grad[1]);
      flevel.push_back(ftr->level);
      fpoint.push_back(ftr->point ? index_of_point.at(ftr->point) : -1);
      fedge.push_back(ftr->type == Feature::EDGELET ? 1 : 0);
    }
    const std::string tag = out + "/track_feat_" + std::to_string(k);
    write_bin(tag + "_px.bin", fpx); write_bin(tag + "_grad.bin", fgrad); write_bin(tag + "_level.bin", flevel);
    write_bin(tag + "_point.bin", fpoint); write_bin(tag + "_edgelet.bin", fedge);
    if (k == 0)
      for (const auto& ov : overlap_kfs) {
        int idx = -1;
        for (int j = 0; j < n_kf; ++j) if (kfs[j] == ov.first) idx = j;
        overlap.push_back((double)idx); overlap.push_back((double)ov.second);
      }
    FrameTracker::Decision dec = FrameTracker::Decision();
    if (decide) {
      // processFrame :242-260 and :305 in one device call, then the same decision by the host twins on the objects as the call left them
      auto created = [&](const FramePtr& f) { double j = -1.0; for (size_t i = 0; i < kfs.size(); ++i) if (kfs[i] == f) j = (double)i; return j; };
      if (!tracker.finishFrame(cur, map, m.size() > 18 && m[18] > 0 ? (size_t)m[18] : (size_t)20, 5, kf_select_min_dist, dec))
        throw std::runtime_error("svo::FrameTracker::finishFrame failed at frame " + std::to_string(k));
      double depth_mean = std::numeric_limits<double>::quiet_NaN(), depth_min = 0.0;
      const bool have = frame_utils::getSceneDepth(*cur, depth_mean, depth_min);
      const bool need = needNewKf(*cur, overlap_kfs, depth_mean, kf_select_min_dist);
      const FramePtr far = map.getFurthestKeyframe(cur->pos());
      decisions.insert(decisions.end(), {dec.have_depth ? 1.0 : 0.0, dec.depth_mean, dec.depth_min, dec.overlap_valid ? 1.0 : 0.0, dec.need_new_kf ? 1.0 : 0.0,
                                         created(dec.furthest), have ? 1.0 : 0.0, depth_mean, depth_min, 1.0, need ? 1.0 : 0.0, created(far),
                                         (double)tracker.deviceDecisions()});
    }
    if (!decide && k == 0 && m.size() > 18 && m[18] > 0) {
      // FrameHandlerBase::optimizeStructure(new_frame, 20, 5) as processFrame calls it behind the pose refinement (:242-244)
      std::vector<const Point*> had;
      for (const Feature* ftr : cur->fts_) if (ftr->point) had.push_back(ftr->point);
      if (!tracker.optimiseStructure(cur, map, (size_t)m[18], 5)) throw std::runtime_error("svo::FrameTracker::optimiseStructure failed");
      std::vector<double> so;                                                  // point index, x, y, z of every point that was optimised
      for (int p = 0; p < n_points; ++p)
        if (points[p]->last_structure_optim_ == cur->id_) so.insert(so.end(), {(double)p, points[p]->pos_[0], points[p]->pos_[1], points[p]->pos_[2]});
      write_bin(out + "/track_structure_first.bin", so);
    }
    if (k == 0) {                                                              // the map's points as the first frame left them
      std::vector<int32_t> st;
      for (int p = 0; p < n_points; ++p) { st.push_back((int32_t)points[p]->type_); st.push_back(points[p]->n_failed_reproj_); st.push_back(points[p]->n_succeeded_reproj_); }
      write_bin(out + "/track_points_after_first.bin", st);
      write_bin(out + "/track_key_after_first.bin", key_table());
      std::vector<int32_t> linked;                                             // features that still refer to their point, per observation
      for (int o = 0; o < n_obs; ++o) {
        // (a deleted candidate's feature is gone: its observation counts as unlinked)
        bool cand_alive = true;
        if (points[obs_point[o]]->type_ == Point::TYPE_DELETED && pt_type[obs_point[o]] == (int)Point::TYPE_CANDIDATE) cand_alive = false;
        linked.push_back(cand_alive && feature_of_obs[o] && feature_of_obs[o]->point != nullptr ? 1 : 0);
      }
      write_bin(out + "/track_obs_linked_after_first.bin", linked);
    }
    uploads.push_back((double)tracker.mapUploads());
    compactions.push_back((double)tracker.pointCompactions());
    if (m.size() > 20 && (int)m[20] == k && !map.point_candidates_.candidates_.empty()) {
      // what the depth filter's thread does when a seed converges (MapPointCandidates::newCandidatePoint): a new candidate
      // appears in the list behind the tracker's back -- here a twin of the list's first one
      const MapPointCandidates::PointCandidate& c0 = map.point_candidates_.candidates_.front();
      points.emplace_back(new Point(c0.first->pos_));
      Point* np_ = points.back().get();
      np_->type_ = Point::TYPE_CANDIDATE;
      Feature* nf = new Feature(c0.second->frame, c0.second->px, c0.second->f, c0.second->level);
      nf->point = np_;
      np_->obs_.push_front(nf);
      index_of_point[np_] = (int)points.size() - 1;
      std::unique_lock<std::mutex> lock(map.point_candidates_.mut_);
      map.point_candidates_.candidates_.push_back(MapPointCandidates::PointCandidate(np_, nf));
    }
    removed.push_back(-1.0);
    if (keyframe_at >= 0 && (k == keyframe_at || (kf_every > 0 && k > keyframe_at && (k - keyframe_at) % kf_every == 0))) {
      // FrameHandlerMono::processFrame :284-330: the tracked frame becomes a keyframe -- setKeyframe (key points), every feature
      // with a point becomes an observation of it (Point::addFrameRef: front of obs_), the map takes the frame, the device
      // keeps its pyramid; the tracker flattens the grown map before the next frame
      cur->setKeyframe();
      for (Feature* ftr : cur->fts_) if (ftr->point != nullptr) ftr->point->addFrameRef(ftr);
      if (incremental) map.point_candidates_.addCandidatePointToFrame(cur);
      // a map that is full loses the keyframe furthest from the new one: chosen before the new one joins, as the reference does
      FramePtr furthest;
      if (max_kfs > 2 && (int)map.size() >= max_kfs) {
        furthest = map.getFurthestKeyframe(cur->pos());
        if (decide) {                                                            // the device named it; the objects have to agree
          if (dec.furthest != furthest) throw std::runtime_error("the device and Map::getFurthestKeyframe name different keyframes at frame " + std::to_string(k));
          furthest = dec.furthest;
        }
        if (!furthest) throw std::runtime_error("no furthest keyframe at frame " + std::to_string(k) + ": the frame's pose is not a number, tracking was lost");
      }
      map.addKeyframe(cur);
      kfs.push_back(cur);
      if (!(incremental ? tracker.lastFrameBecameKeyframe(cur, map) : tracker.lastFrameBecameKeyframe(*cur)))
        throw std::runtime_error("svo::FrameTracker::lastFrameBecameKeyframe failed");
      if (furthest) {
        for (size_t j = 0; j < kfs.size(); ++j) if (kfs[j] == furthest) removed.back() = (double)j;
        map.safeDeleteFrame(furthest);
        if (full_remove || !incremental) tracker.mapChanged();
        else if (!tracker.keyframeRemoved(furthest, map)) throw std::runtime_error("svo::FrameTracker::keyframeRemoved failed");
      }
    }
    size_t n_seeded = 0;
    if (new_seeds > 0 && cur->is_keyframe_) {
      // the depth filter's thread: seeds of the new keyframe converge (DepthFilter::updateSeeds :310-331, newCandidatePoint)
      std::unique_lock<std::mutex> lock(map.point_candidates_.mut_);
      for (const Feature* ftr : cur->fts_) {
        if ((int)n_seeded == new_seeds) break;
        if (ftr->point == nullptr) continue;
        points.emplace_back(new Point(Vector3d{{ftr->point->pos_[0] + 1e-4, ftr->point->pos_[1] + 1e-4, ftr->point->pos_[2] + 1e-4}}));
        Point* np_ = points.back().get();
        np_->type_ = Point::TYPE_CANDIDATE;
        Feature* nf = new Feature(cur.get(), ftr->px, ftr->f, ftr->level);
        nf->point = np_;
        np_->obs_.push_front(nf);
        index_of_point[np_] = (int)points.size() - 1;
        map.point_candidates_.candidates_.push_back(MapPointCandidates::PointCandidate(np_, nf));
        ++n_seeded;
      }
    }
    room_needed = std::max(room_needed, tracker.livingPoints() + n_seeded);
    last = cur;
  }
  write_bin(out + "/track_poses.bin", poses);
  write_bin(out + "/map_compactions.bin", compactions);
  write_bin(out + "/map_points_room.bin", std::vector<double>{(double)room_needed, (double)tracker.tablePoints()});
  write_bin(out + "/track_stats.bin", stats);
  write_bin(out + "/track_uploads.bin", uploads);
  if (max_kfs > 0) {
    write_bin(out + "/track_removed.bin", removed);
    std::set<const Point*> seen;                                               // the map at the end: keyframes, features with a point, points, candidates
    double n_ftr = 0;
    for (const FramePtr& kf : map.keyframes_)
      for (const Feature* ftr : kf->fts_) if (ftr->point) { ++n_ftr; seen.insert(ftr->point); }
    write_bin(out + "/track_map_size.bin", std::vector<double>{(double)map.size(), n_ftr, (double)seen.size(), (double)map.point_candidates_.candidates_.size()});
  }
  write_bin(out + "/track_overlap_first.bin", overlap);
  if (decide) write_bin(out + "/track_decision.bin", decisions);
  if (times) write_bin(out + "/times_track.bin", track_us);
  if (port.lone) std::printf("svo_host_demo track OK\n");
  return 0;
}

static int track_lone(const std::string& dir, const std::string& out, bool incremental, bool times, int max_kfs, bool full_remove, int kf_every,
                      int max_points, bool compact, int new_seeds, int reloc_at) {
  const std::vector<double> m = read_bin<double>(dir + "/track_manifest.bin");
  PinholeCamera cam = track_camera(dir, m);
  FrameTracker tracker(cam, track_config(m, max_kfs, max_points));
  TrackerPort port;
  port.lone = &tracker;
  return track_demo(dir, out, port, incremental, times, max_kfs, full_remove, kf_every, compact, new_seeds, reloc_at);
}

// n copies of the world, one svo::FrameTrackerGroup: every world's outputs must equal the lone tracker's.  rig: n worlds of their
// own (<dir>/cam<w>), every camera with its own model (one image size, one configuration: that of cam0's manifest)
// staggered: the worlds do not advance together (GroupRendezvous::staggered); group_schedule.bin lists the calls that were made
static int track_group(const std::string& dir, const std::string& out, int n, bool rig, bool staggered = false) {
  auto world_dir = [&](int w) { return rig ? dir + "/cam" + std::to_string(w) : dir; };
  const std::vector<double> m = read_bin<double>(world_dir(0) + "/track_manifest.bin");
  std::vector<PinholeCamera> cams;
  for (int w = 0; w < n; ++w) cams.push_back(track_camera(world_dir(w), read_bin<double>(world_dir(w) + "/track_manifest.bin")));
  std::vector<const PinholeCamera*> cam_ptrs;
  for (const PinholeCamera& c : cams) cam_ptrs.push_back(&c);
  svo_hip_tracker_config cfg = track_config(m);
  cfg.max_items = (cfg.max_items + 15) / 16 * 16;
  FrameTrackerGroup group(cam_ptrs, cfg);
  if (!group.ok()) throw std::runtime_error("svo::FrameTrackerGroup: no device tracker group");
  GroupRendezvous rz;
  rz.group = &group; rz.n = (size_t)n;
  rz.last.resize((size_t)n); rz.cur.resize((size_t)n); rz.maps.resize((size_t)n); rz.overlap.resize((size_t)n); rz.out.resize((size_t)n);
  rz.staggered = staggered; rz.waiting.assign((size_t)n, 0); rz.finished.assign((size_t)n, 0);
  std::vector<std::string> errors((size_t)n);
  for (int w = 0; w < n; ++w) (void)::mkdir((out + "/g" + std::to_string(w)).c_str(), 0755);
  std::vector<std::thread> worlds;
  for (int w = 0; w < n; ++w)
    worlds.emplace_back([&, w]() {
      std::unique_lock<std::mutex> baton(rz.mu);                               // this world runs only while it holds the baton
      TrackerPort port;
      port.rz = &rz; port.baton = &baton; port.w = (size_t)w;
      try {
        track_demo(world_dir(w), out + "/g" + std::to_string(w), port);
        if (staggered) { rz.finished[(size_t)w] = 1; rz.fire(); }               // (the others no longer wait for this world)
      } catch (const std::exception& e) {
        errors[(size_t)w] = e.what();
        rz.ok = false; ++rz.failed; ++rz.generation; rz.cv.notify_all();      // let the others go (they fail at their next frame)
      }
    });
  for (std::thread& t : worlds) t.join();
  for (const std::string& e : errors) if (!e.empty()) throw std::runtime_error(e);
  if (staggered) write_bin(out + "/group_schedule.bin", rz.schedule);
  std::printf("svo_host_demo trackgroup OK (%d worlds%s%s)\n", n, rig ? ", a rig" : "", staggered ? ", staggered" : "");
  return 0;
}

// ---- the tracking thread's SparseImgAlign::run while the depth-filter thread creates and drops device seed batches.
// A keyframe's seeds are a svo_hip_seed_batch created when the keyframe is first seen and destroyed when its seeds age out
// or are used up (S/depth_filter.cpp:129-151,256-261): allocator traffic on the depth-filter thread at keyframe rate.
// hipFree synchronises the whole device; with the per-context pool (svo_hip_ctx_info) nothing is allocated or freed after
// warm-up.  Prints median / 99th percentile / worst latency of run() with the second thread idle and busy.
static int churn_demo(const std::string& dir, const std::string& out) {
  const std::vector<double> m = read_bin<double>(dir + "/manifest.bin");
  PinholeCamera cam{(int)m[0], (int)m[1], m[2], m[3], m[4], m[5]};
  const int n_levels = (int)m[6];
  const auto px = read_bin<double>(dir + "/sia_px.bin"), f = read_bin<double>(dir + "/sia_f.bin"), pos = read_bin<double>(dir + "/sia_pos.bin");
  const auto has = read_bin<uint8_t>(dir + "/sia_has.bin");
  FramePtr ref = load_frame(dir, &cam, 0, n_levels);
  std::vector<std::unique_ptr<Point>> points;
  for (size_t i = 0; i < has.size(); ++i) {
    Feature* ftr = new Feature(ref.get(), Vector2d{{px[2 * i], px[2 * i + 1]}}, Vector3d{{f[3 * i], f[3 * i + 1], f[3 * i + 2]}}, 0);
    if (has[i]) { points.emplace_back(new Point(Vector3d{{pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]}})); ftr->point = points.back().get(); }
    ref->fts_.push_back(ftr);
  }
  FramePtr cur = load_frame(dir, &cam, 1, n_levels);
  const SE3 T_start = ref->T_f_w_;
  SparseImgAlign align(4, 2, 30, SparseImgAlign::GaussNewton, false, false);      // the shipping range L4..L2
  auto one_run = [&]() {
    cur->T_f_w_ = T_start;
    const auto t0 = std::chrono::steady_clock::now();
    align.run(ref, cur);
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  };
  for (int k = 0; k < 20; ++k) one_run();
  const auto spx = read_bin<double>(dir + "/seed_px.bin"), sf = read_bin<double>(dir + "/seed_f.bin");
  const auto slevel = read_bin<int32_t>(dir + "/seed_level.bin");
  const int n_all = (int)slevel.size();
  std::atomic<int> mode{0};                  // 0 idle, 1 churn, 2 stop
  std::atomic<long> n_created{0};
  svo_hip_ctx_stats st_before{}, st_after{};
  std::vector<double> create_us;            // per keyframe on the second thread: svo_hip_seed_batch_create (+ the drop of the oldest batch)
  std::thread filter([&]() {
    svo_hip_ctx* ctx = nullptr;
    if (svo_hip_ctx_create(&ctx, 0, nullptr) != SVO_HIP_OK) return;
    std::vector<float> a((size_t)n_all, 10.f), b((size_t)n_all, 10.f), mu((size_t)n_all, 0.5f), zr((size_t)n_all, 1.f), s2((size_t)n_all, 1.f / 36.f);
    std::vector<svo_hip_seed_batch*> alive;
    unsigned rng = 12345u;
    auto keyframe = [&]() {                  // a new keyframe's seeds come, the oldest keyframe's go
      rng = rng * 1664525u + 1013904223u;
      const int n = 300 + (int)((rng >> 8) % 700u);
      svo_hip_seed_batch* sb = nullptr;
      const auto t0 = std::chrono::steady_clock::now();
      if (svo_hip_seed_batch_create(ctx, n < n_all ? n : n_all, spx.data(), sf.data(), slevel.data(), a.data(), b.data(), mu.data(), zr.data(), s2.data(), &sb) == SVO_HIP_OK) {
        alive.push_back(sb);
        ++n_created;
      }
      if (alive.size() > 3) { svo_hip_seed_batch_destroy(alive.front()); alive.erase(alive.begin()); }
      if (mode.load() == 1) create_us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    };
    for (int k = 0; k < 64; ++k) keyframe(); // warm-up: the pool has seen the working set (both capacity classes, every size)
    svo_hip_ctx_info(ctx, &st_before);
    while (mode.load() != 2) {
      if (mode.load() == 1) keyframe();
      else std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
    svo_hip_ctx_info(ctx, &st_after);
    for (svo_hip_seed_batch* sb : alive) svo_hip_seed_batch_destroy(sb);
    svo_hip_ctx_destroy(ctx);
  });
  auto measure = [&](int n) {
    std::vector<double> us;
    for (int k = 0; k < n; ++k) us.push_back(one_run());
    std::sort(us.begin(), us.end());
    return std::vector<double>{us[us.size() / 2], us[us.size() * 99 / 100], us.back()};
  };
  std::this_thread::sleep_for(std::chrono::milliseconds(300));     // the filter thread's warm-up is over
  const std::vector<double> idle = measure(2000);
  const long c0 = n_created.load();
  mode = 1;
  const std::vector<double> busy = measure(2000);
  const long c1 = n_created.load();
  mode = 2;
  filter.join();
  std::printf("churn: SparseImgAlign::run (L4-L2, %zu features) on the tracking thread, us: median / p99 / worst\n", has.size());
  std::printf("churn:   second thread idle:                          %8.1f %8.1f %8.1f\n", idle[0], idle[1], idle[2]);
  std::printf("churn:   second thread creating + dropping batches:   %8.1f %8.1f %8.1f   (%ld batches created meanwhile)\n", busy[0], busy[1], busy[2], c1 - c0);
  std::printf("churn:   allocator calls of the second context during the measurement: %llu, free calls: %llu\n",
              st_after.allocator_calls - st_before.allocator_calls, st_after.free_calls - st_before.free_calls);
  std::sort(create_us.begin(), create_us.end());
  if (!create_us.empty())
    std::printf("churn:   a keyframe on the second thread (create a batch of 300-1000 seeds incl. its upload, drop the oldest), us: median %.1f  p99 %.1f\n",
                create_us[create_us.size() / 2], create_us[create_us.size() * 99 / 100]);
  write_bin(out + "/churn.bin", std::vector<double>{idle[0], idle[1], idle[2], busy[0], busy[1], busy[2], (double)(c1 - c0),
                                                    (double)(st_after.allocator_calls - st_before.allocator_calls),
                                                    (double)(st_after.free_calls - st_before.free_calls)});
  return 0;
}

// ---- keyframes [device_seeds] [threaded]: N frames through the DepthFilter protocol, some of them keyframes, each keyframe with a
// list of existing features.  With device_seeds the filter makes a keyframe's seeds itself (enableDeviceSeedInit, addKeyframe
// without features: grid marks, detection and seed construction on the device, nothing uploaded).  Without it the demo does what
// a host has to do today: on the threaded path the keyframe's update comes first (it marks the host DetectorGrid), then the
// existing features are marked, svo_hip_detect_features runs on that grid, and the features are handed in.
// Inputs: manifest.bin, frame_<k>_*.bin, depth_mean_min.bin, kf_params.bin (n_pyr_levels, cell_size, detection_threshold),
// kf_list.bin (frame indices, ascending, the first one 0), kf_existing_<j>.bin (px of keyframe j's existing features).
// Outputs: kf<j>_grid.bin (the grid as the detector saw it), kf<j>_px.bin / kf<j>_level.bin (the new seeds), kf_counts.bin;
// conv.bin, per convergence callback: seed id, xyz_world (bits), sigma2; frames.bin, per frame that is not a keyframe: its
// index, seeds on the device, seeds uploaded by its update.
struct KeyframeDemoFilter : DepthFilter {
  using DepthFilter::DepthFilter;
  /// the features of a keyframe whose update has already run (the threaded path of the leg without device_seeds)
  void seedKeyframe(FramePtr frame, double depth_mean, double depth_min, const std::vector<Feature*>& fts) {
    new_keyframe_min_depth_ = depth_min;
    new_keyframe_mean_depth_ = depth_mean;
    initializeSeeds(frame, fts);
  }
};

static int keyframes_demo(const std::string& dir, const std::string& out, bool device_seeds, bool threaded) {
  const std::vector<double> m = read_bin<double>(dir + "/manifest.bin");
  PinholeCamera cam{(int)m[0], (int)m[1], m[2], m[3], m[4], m[5]};
  const int n_levels = (int)m[6], n_frames = (int)m[7];
  const auto dm = read_bin<double>(dir + "/depth_mean_min.bin");
  const auto prm = read_bin<double>(dir + "/kf_params.bin");
  const int n_pyr_levels = (int)prm[0], cell = (int)prm[1];
  const double threshold = prm[2];
  const auto kf_list = read_bin<double>(dir + "/kf_list.bin");
  std::vector<FramePtr> frames;
  for (int k = 0; k < n_frames; ++k) frames.push_back(load_frame(dir, &cam, k, n_levels));
  Seed::batch_counter = 0;
  Seed::seed_counter = 0;
  std::map<Feature*, int> seed_id;
  std::vector<double> conv, frame_rows, counts;
  std::vector<Feature*> seed_features;
  DetectorGrid grid(cam.width, cam.height, cell);
  // the detector of the leg without device_seeds: the main thread's own context and pyramid
  svo_hip_ctx* dctx = nullptr;
  svo_hip_pyramid* dpyr = nullptr;
  hip_bridge::check(svo_hip_ctx_create(&dctx, 0, nullptr), nullptr, "ctx_create");
  hip_bridge::check(svo_hip_pyramid_create(dctx, cam.width, cam.height, n_levels, 1, &dpyr), dctx, "pyramid_create");
  {
    KeyframeDemoFilter df([&](Point* p, double s2) {
      double row[5] = {(double)seed_id.at(p->obs_.front()), p->pos_[0], p->pos_[1], p->pos_[2], s2};
      conv.insert(conv.end(), row, row + 5);
      delete p;
    }, &grid);
    if (device_seeds) { df.enableDeviceSeedInit(n_pyr_levels, cell, threshold); df.record_detector_grid_ = true; }
    auto wait_idle = [&]() { while (threaded && !df.idle()) std::this_thread::yield(); };
    if (threaded) df.startThread();
    size_t j = 0;
    for (int k = 0; k < n_frames; ++k) {
      FramePtr fr = frames[(size_t)k];
      if (j < kf_list.size() && (int)kf_list[j] == k) {
        const auto ex = read_bin<double>(dir + "/kf_existing_" + std::to_string(j) + ".bin");
        for (size_t i = 0; i + 1 < ex.size(); i += 2)
          fr->addFeature(new Feature(fr.get(), Vector2d{{ex[i], ex[i + 1]}}, Vector3d{{0.0, 0.0, 1.0}}, 0));
        fr->setKeyframe();
        std::vector<Feature*> fts;
        std::vector<uint8_t> seen;
        if (device_seeds) {
          df.addKeyframe(fr, dm[0], dm[1]);
          wait_idle();
          fts = df.takeDeviceFeatures();
          seen = df.last_detector_grid_;
        } else {
          if (threaded) { df.addFrame(fr); wait_idle(); }                       // updateSeeds(kf): the grid marks of :302-306
          for (const Feature* f : fr->fts_) grid.setGridOccpuancy(f->px);       // setExistingFeatures
          seen.assign(grid.grid_occupancy_.begin(), grid.grid_occupancy_.end());
          const uint8_t* lv[SVO_HIP_MAX_LEVELS] = {nullptr};
          for (size_t l = 0; l < fr->img_pyr_.size(); ++l) lv[l] = fr->img_pyr_[l].data();
          hip_bridge::check(svo_hip_pyramid_upload(dpyr, 0, lv), dctx, "pyramid_upload");
          hip_bridge::check(svo_hip_ctx_sync(dctx), dctx, "sync");
          const size_t nc = seen.size();
          std::vector<double> px(2 * nc), f(3 * nc);
          std::vector<int32_t> level(nc);
          int32_t n = 0;
          const svo_hip_camera c = cam.toC();
          hip_bridge::check(svo_hip_detect_features(dctx, dpyr, 0, &c, n_pyr_levels, cell, seen.data(), threshold, &n, px.data(), f.data(),
                                                    level.data(), nullptr), dctx, "detect_features");
          grid.resetGrid();
          for (int32_t i = 0; i < n; ++i)
            fts.push_back(new Feature(fr.get(), Vector2d{{px[2 * (size_t)i], px[2 * (size_t)i + 1]}},
                                      Vector3d{{f[3 * (size_t)i], f[3 * (size_t)i + 1], f[3 * (size_t)i + 2]}}, level[(size_t)i]));
          if (threaded) df.seedKeyframe(fr, dm[0], dm[1], fts);
          else df.addKeyframe(fr, dm[0], dm[1], fts);
        }
        std::vector<double> px;
        std::vector<int32_t> level;
        for (Feature* f : fts) {
          seed_id[f] = (int)seed_features.size();                             // = Seed::id: seeds are numbered as they are made
          seed_features.push_back(f);
          px.push_back(f->px[0]); px.push_back(f->px[1]); level.push_back(f->level);
        }
        write_bin(out + "/kf" + std::to_string(j) + "_grid.bin", seen);
        write_bin(out + "/kf" + std::to_string(j) + "_px.bin", px);
        write_bin(out + "/kf" + std::to_string(j) + "_level.bin", level);
        counts.push_back((double)fts.size());
        ++j;
      } else {
        df.addFrame(fr);
        wait_idle();
        const svo::hip_bridge::SeedBatchStats& ls = df.last_stats_;
        frame_rows.insert(frame_rows.end(), {(double)k, (double)ls.n_seeds, (double)ls.n_uploaded});
      }
    }
    if (threaded) df.stopThread();
  }
  write_bin(out + "/kf_counts.bin", counts);
  write_bin(out + "/conv.bin", conv);
  write_bin(out + "/frames.bin", frame_rows);
  for (Feature* f : seed_features) delete f;
  svo_hip_pyramid_destroy(dpyr);
  svo_hip_ctx_destroy(dctx);
  std::printf("svo_host_demo OK\n");
  return 0;
}

// ---- svo::DepthFilterGroup: n cameras, each with its own frames (<case_dir>/cam<c>/frame_*), keyframes (cam<c>/keyframes.bin: the
// frame numbers, the first is 0) and seeds per keyframe (cam<c>/kf<j>_{px,f,level}.bin); options.bin: max_n_kfs and the convergence threshold.  Step k: a camera whose frame k is a
// keyframe updates its seeds with it (the pass reports the updated seeds, the grid is marked) and then gets the keyframe's new
// seeds, as DepthFilter's thread does (depth_filter.cpp:191-229); the other cameras update with frame k.  Run twice: through the
// group (one device pass per step for all cameras) and through one lone unthreaded DepthFilter per camera.  Per camera the
// sequence of convergence callbacks, the final seeds and the detector grid go to <out_dir>/{group,lone}_cam<c>_*.bin.
// rig: camera c's model is cam<c>/camera.bin (fx fy cx cy k1 k2 p1 p2 k3; the manifest's image size)
static int filter_group_demo(const std::string& dir, const std::string& out, bool rig) {
  const std::vector<double> m = read_bin<double>(dir + "/manifest.bin");      // w h fx fy cx cy n_levels n_frames n_cameras
  PinholeCamera pc{(int)m[0], (int)m[1], m[2], m[3], m[4], m[5]};
  const int n_levels = (int)m[6], n_frames = (int)m[7], n_cams = (int)m[8];
  std::vector<PinholeCamera> pcs((size_t)n_cams, pc);         // (the frames keep pointers into it)
  for (int c = 0; c < n_cams && rig; ++c) {
    const std::vector<double> k = read_bin<double>(dir + "/cam" + std::to_string(c) + "/camera.bin");
    if (k.size() != 9) throw std::runtime_error("filtergroup rig: camera.bin holds fx fy cx cy and five distortion coefficients");
    PinholeCamera& q = pcs[(size_t)c];
    q.fx = k[0]; q.fy = k[1]; q.cx = k[2]; q.cy = k[3];
    for (int i = 0; i < 5; ++i) q.d[i] = k[4 + (size_t)i];
  }
  const auto dm = read_bin<double>(dir + "/depth_mean_min.bin");
  const auto opt = read_bin<double>(dir + "/options.bin");                    // Options: max_n_kfs, seed_convergence_sigma2_thresh
  struct SeedSet { std::vector<double> px, f; std::vector<int32_t> level; };
  struct Cam {
    std::vector<FramePtr> frames;
    std::vector<int> keyframes;
    std::vector<SeedSet> sets;
  };
  std::vector<Cam> cams((size_t)n_cams);
  for (int c = 0; c < n_cams; ++c) {
    const std::string cd = dir + "/cam" + std::to_string(c);
    for (int k = 0; k < n_frames; ++k) cams[(size_t)c].frames.push_back(load_frame(cd, &pcs[(size_t)c], k, n_levels));
    for (double k : read_bin<double>(cd + "/keyframes.bin")) {
      const std::string kd = cd + "/kf" + std::to_string(cams[(size_t)c].keyframes.size());
      cams[(size_t)c].keyframes.push_back((int)k);
      cams[(size_t)c].frames[(size_t)k]->setKeyframe();
      cams[(size_t)c].sets.push_back(SeedSet{read_bin<double>(kd + "_px.bin"), read_bin<double>(kd + "_f.bin"), read_bin<int32_t>(kd + "_level.bin")});
    }
  }
  // per run and camera: the features of its keyframes (feature -> running number), the callbacks, the grid
  struct Side {
    std::map<Feature*, int> index;
    std::vector<std::vector<Feature*>> fts;     // per keyframe
    std::vector<double> conv;                    // per callback: feature number, x, y, z, sigma2
    std::unique_ptr<DetectorGrid> grid;
  };
  auto make_side = [&](const Cam& cam, Side& s) {
    int id = 0;
    for (size_t j = 0; j < cam.sets.size(); ++j) {
      const SeedSet& ss = cam.sets[j];
      Frame* kf = cam.frames[(size_t)cam.keyframes[j]].get();
      s.fts.emplace_back();
      for (size_t i = 0; i < ss.level.size(); ++i) {
        s.fts.back().push_back(new Feature(kf, Vector2d{{ss.px[2 * i], ss.px[2 * i + 1]}}, Vector3d{{ss.f[3 * i], ss.f[3 * i + 1], ss.f[3 * i + 2]}}, ss.level[i]));
        s.index[s.fts.back().back()] = id++;
      }
    }
    s.grid.reset(new DetectorGrid(pc.width, pc.height, 30));
  };
  auto keyframe_no = [&](const Cam& cam, int k) {
    for (size_t j = 0; j < cam.keyframes.size(); ++j) if (cam.keyframes[j] == k) return (int)j;
    return -1;
  };
  auto dump = [&](Side& s, std::list<Seed>& seeds, const std::string& tag) {
    std::vector<double> rows;
    for (const Seed& sd : seeds) { rows.push_back((double)s.index.at(sd.ftr)); rows.push_back(sd.a); rows.push_back(sd.b); rows.push_back(sd.mu); rows.push_back(sd.sigma2); }
    write_bin(out + "/" + tag + "_seeds.bin", rows);
    write_bin(out + "/" + tag + "_conv.bin", s.conv);
    write_bin(out + "/" + tag + "_grid.bin", std::vector<uint8_t>(s.grid->grid_occupancy_.begin(), s.grid->grid_occupancy_.end()));
    for (auto& v : s.fts) for (Feature* f : v) delete f;
  };
  auto callback = [](Side* s) {
    return [s](Point* p, double s2) {
      s->conv.insert(s->conv.end(), {(double)s->index.at(p->obs_.front()), p->pos_[0], p->pos_[1], p->pos_[2], s2});
      delete p;
    };
  };
  // ---- the group
  {
    std::vector<Side> sides((size_t)n_cams);
    std::vector<DepthFilterGroup::callback_t> cbs;
    std::vector<DetectorGrid*> grids;
    for (int c = 0; c < n_cams; ++c) { make_side(cams[(size_t)c], sides[(size_t)c]); cbs.push_back(callback(&sides[(size_t)c])); grids.push_back(sides[(size_t)c].grid.get()); }
    DepthFilterGroup group(cbs, grids);
    group.options_.max_n_kfs = (int)opt[0]; group.options_.seed_convergence_sigma2_thresh = opt[1];
    int n_passes = 0, n_batches = 0;
    for (int k = 0; k < n_frames; ++k) {
      std::vector<FramePtr> frames;
      for (int c = 0; c < n_cams; ++c) frames.push_back(cams[(size_t)c].frames[(size_t)k]);
      group.addFrames(frames);
      for (int c = 0; c < n_cams; ++c) { n_batches += group.last_stats_[(size_t)c].n_device_calls; }
      ++n_passes;
      for (int c = 0; c < n_cams; ++c) {
        const int j = keyframe_no(cams[(size_t)c], k);
        if (j >= 0) group.addKeyframe((size_t)c, cams[(size_t)c].frames[(size_t)k], dm[0], dm[1], sides[(size_t)c].fts[(size_t)j]);
      }
    }
    for (int c = 0; c < n_cams; ++c) dump(sides[(size_t)c], group.getSeeds((size_t)c), "group_cam" + std::to_string(c));
    write_bin(out + "/group_summary.bin", std::vector<double>{(double)n_passes, (double)n_batches, (double)group.keyframeUploads()});
  }
  // ---- a lone filter per camera
  for (int c = 0; c < n_cams; ++c) {
    Side side;
    make_side(cams[(size_t)c], side);
    Seed::batch_counter = 0;
    DepthFilter df(callback(&side), side.grid.get());
    df.options_.max_n_kfs = (int)opt[0]; df.options_.seed_convergence_sigma2_thresh = opt[1];
    for (int k = 0; k < n_frames; ++k) {
      df.addFrame(cams[(size_t)c].frames[(size_t)k]);
      const int j = keyframe_no(cams[(size_t)c], k);
      if (j >= 0) df.addKeyframe(cams[(size_t)c].frames[(size_t)k], dm[0], dm[1], side.fts[(size_t)j]);
    }
    dump(side, df.getSeeds(), "lone_cam" + std::to_string(c));
  }
  std::printf("svo_host_demo filtergroup OK%s\n", rig ? " (a rig)" : "");
  return 0;
}

// ---- the bootstrap: klt_meta.bin = [width, height, n_cameras, n_images, n_features, min_features, min_tracked, min_disparity,
// then per camera fx fy cx cy k1 k2 p1 p2 k3] (doubles), klt_images.bin = n_images level-0 images back to back (image 0: the
// first frame), klt_px.bin = n_features x 2 floats.  Camera c tracks image 1 + (k + c) % (n_images - 1) in frame k.
static int klt_demo(const std::string& dir, const std::string& out) {
  using namespace svo::initialization;
  const std::vector<double> m = read_bin<double>(dir + "/klt_meta.bin");
  const int w = (int)m[0], h = (int)m[1], nc = (int)m[2], ni = (int)m[3], nf = (int)m[4];
  hip_bridge::KltInitGates gates;
  gates.min_features = (size_t)m[5]; gates.min_tracked = (size_t)m[6]; gates.min_disparity = m[7];
  std::vector<svo_hip_camera> cams((size_t)nc);
  for (int c = 0; c < nc; ++c) {
    PinholeCamera pc;
    pc.width = w; pc.height = h; pc.fx = m[8 + 9 * c]; pc.fy = m[9 + 9 * c]; pc.cx = m[10 + 9 * c]; pc.cy = m[11 + 9 * c];
    for (int k = 0; k < 5; ++k) pc.d[k] = m[12 + 9 * c + k];
    cams[(size_t)c] = pc.toC();
  }
  const std::vector<uint8_t> images = read_bin<uint8_t>(dir + "/klt_images.bin");
  const std::vector<float> pxf = read_bin<float>(dir + "/klt_px.bin");
  if (images.size() != (size_t)w * h * ni || pxf.size() != (size_t)2 * nf) throw std::runtime_error("klt case: sizes");
  svo_hip_ctx* ctx = nullptr;
  hip_bridge::check(svo_hip_ctx_create(&ctx, 0, nullptr), nullptr, "ctx_create");
  svo_hip_pyramid* pyr = nullptr;
  hip_bridge::check(svo_hip_pyramid_create(ctx, w, h, 3, ni, &pyr), ctx, "pyramid_create");
  hip_bridge::check(svo_hip_pyramid_upload_level0_batch_and_build(pyr, 0, ni, images.data()), ctx, "pyramid_build");
  hip_bridge::check(svo_hip_ctx_sync(ctx), ctx, "sync");
  std::vector<double> results;
  {
    KltInit init(ctx, w, h, nc, 1024, gates);
    if (!init.ok()) throw std::runtime_error("klt_create");
    std::vector<Point2f> px;
    std::vector<Vector3d> f;
    for (int i = 0; i < nf; ++i) {
      px.push_back(Point2f(pxf[2 * i], pxf[2 * i + 1]));
      f.push_back(Vector3d{{0.001 * pxf[2 * i], 0.001 * pxf[2 * i + 1], 1.0}});
    }
    for (int c = 0; c < nc; ++c)
      results.push_back(c == 0 ? init.addFirstFrameDetected(0, pyr, 0, cams[0], 3, 20, 10.0) : init.addFirstFrame(c, pyr, 0, px, f));
    std::vector<int> listed((size_t)nc), slots((size_t)nc);
    std::vector<InitResult> res((size_t)nc);
    for (int k = 0; k < 3; ++k) {
      for (int c = 0; c < nc; ++c) { listed[(size_t)c] = c; slots[(size_t)c] = 1 + (k + c) % (ni - 1); }
      if (!init.trackSecondFrames(nc, listed.data(), pyr, slots.data(), cams.data(), res.data())) throw std::runtime_error("klt_track");
      for (int c = 0; c < nc; ++c) {
        const KltInit::Lists& l = init.lists(c);
        std::vector<float> a, b;
        std::vector<double> fr, fc;
        for (size_t i = 0; i < l.px_ref_.size(); ++i) {
          a.push_back(l.px_ref_[i].x); a.push_back(l.px_ref_[i].y); b.push_back(l.px_cur_[i].x); b.push_back(l.px_cur_[i].y);
          for (int j = 0; j < 3; ++j) { fr.push_back(l.f_ref_[i][j]); fc.push_back(l.f_cur_[i][j]); }
        }
        const std::string base = out + "/klt_c" + std::to_string(c) + "_k" + std::to_string(k);
        write_bin(base + "_px_ref.bin", a); write_bin(base + "_px_cur.bin", b); write_bin(base + "_f_ref.bin", fr); write_bin(base + "_f_cur.bin", fc);
        write_bin(base + "_disparity.bin", l.disparities_); write_bin(base + "_index.bin", l.index_);
        results.push_back((double)res[(size_t)c]); results.push_back(l.disparity_median_);
        std::printf("klt camera %d frame %d: %zu tracked, median disparity %.3f px, result %d\n", c, k, l.px_ref_.size(), l.disparity_median_, (int)res[(size_t)c]);
      }
    }
  }
  write_bin(out + "/klt_results.bin", results);
  svo_hip_pyramid_destroy(pyr);
  svo_hip_ctx_destroy(ctx);
  std::printf("klt OK (%d cameras)\n", nc);
  return 0;
}

// ---- the bootstrap's second half: boot_meta.bin = [width, height, fx, fy, cx, cy, n, reproj_thresh, min_inliers, map_scale,
// n_hypotheses, seed, T_ref_w[7]] (doubles); boot_px_ref.bin / boot_px_cur.bin = n x 2 floats, boot_f_ref.bin / boot_f_cur.bin =
// n x 3 doubles: the lists of a matcher.  Lists -> two-view on the device -> the twin's first map -> its flatten written out.
static int bootstrap_demo(const std::string& dir, const std::string& out) {
  using namespace svo::initialization;
  const std::vector<double> m = read_bin<double>(dir + "/boot_meta.bin");
  if (m.size() != 19) throw std::runtime_error("bootstrap case: boot_meta.bin");
  PinholeCamera cam;
  cam.width = (int)m[0]; cam.height = (int)m[1]; cam.fx = m[2]; cam.fy = m[3]; cam.cx = m[4]; cam.cy = m[5];
  const size_t n = (size_t)m[6];
  svo_hip_two_view_params prm;
  svo_hip_two_view_default_params(&prm);
  prm.reproj_thresh = m[7]; prm.min_inliers = (int)m[8]; prm.map_scale = m[9]; prm.n_hypotheses = (int)m[10]; prm.seed = (unsigned long long)m[11];
  const auto pr = read_bin<float>(dir + "/boot_px_ref.bin"), pc = read_bin<float>(dir + "/boot_px_cur.bin");
  const auto fr = read_bin<double>(dir + "/boot_f_ref.bin"), fc = read_bin<double>(dir + "/boot_f_cur.bin");
  if (pr.size() != 2 * n || pc.size() != 2 * n || fr.size() != 3 * n || fc.size() != 3 * n) throw std::runtime_error("bootstrap case: sizes");
  std::vector<Point2f> px_ref, px_cur;
  std::vector<Vector3d> f_ref, f_cur;
  for (size_t i = 0; i < n; ++i) {
    px_ref.push_back(Point2f(pr[2 * i], pr[2 * i + 1])); px_cur.push_back(Point2f(pc[2 * i], pc[2 * i + 1]));
    f_ref.push_back(Vector3d{{fr[3 * i], fr[3 * i + 1], fr[3 * i + 2]}}); f_cur.push_back(Vector3d{{fc[3 * i], fc[3 * i + 1], fc[3 * i + 2]}});
  }
  svo_hip_ctx* ctx = nullptr;
  hip_bridge::check(svo_hip_ctx_create(&ctx, 0, nullptr), nullptr, "ctx_create");
  svo_hip_pyramid* pyr = nullptr;
  const std::vector<uint8_t> blank((size_t)cam.width * cam.height, 0);                // the two-view stage reads no image
  hip_bridge::check(svo_hip_pyramid_create(ctx, cam.width, cam.height, 1, 1, &pyr), ctx, "pyramid_create");
  hip_bridge::check(svo_hip_pyramid_upload_level0_batch_and_build(pyr, 0, 1, blank.data()), ctx, "pyramid_build");
  hip_bridge::check(svo_hip_ctx_sync(ctx), ctx, "sync");
  std::vector<double> results;
  {
    hip_bridge::KltInitGates gates;
    gates.min_features = 0;
    KltInit init(ctx, cam.width, cam.height, 1, 1024, gates);
    if (!init.ok()) throw std::runtime_error("klt_create");
    if (init.addFirstFrame(0, pyr, 0, px_ref, f_ref) != hip_bridge::KLT_SUCCESS) throw std::runtime_error("addFirstFrame");
    if (!init.setLists(0, px_ref, px_cur, f_ref, f_cur)) throw std::runtime_error("setLists");
    FramePtr frame_ref(new Frame(&cam, {blank})), frame_cur(new Frame(&cam, {blank}));
    frame_ref->T_f_w_ = SE3(m.data() + 12);
    const InitResult r = init.addSecondFrame(0, frame_ref.get(), frame_cur.get(), &prm);
    const KltInit::TwoView& tv = init.twoView(0);
    results = {(double)r, (double)tv.status_, (double)tv.inliers_.size(), (double)tv.point_index_.size(), tv.depth_median_, tv.scale_};
    results.insert(results.end(), tv.T_cur_from_ref_, tv.T_cur_from_ref_ + 7);
    results.insert(results.end(), tv.T_cur_w_, tv.T_cur_w_ + 7);
    Map map;
    if (r == hip_bridge::KLT_SUCCESS) { map.addKeyframe(frame_ref); map.addKeyframe(frame_cur); }
    const MapTables t = flattenMap(map);
    write_bin(out + "/boot_kf_slot.bin", t.kf_slot); write_bin(out + "/boot_T_kf_w.bin", t.T_kf_w); write_bin(out + "/boot_kf_key_point.bin", t.kf_key_point);
    write_bin(out + "/boot_kf_ftr_offset.bin", t.kf_ftr_offset); write_bin(out + "/boot_kf_ftr_point.bin", t.kf_ftr_point);
    write_bin(out + "/boot_pt_pos.bin", t.pt_pos); write_bin(out + "/boot_pt_type.bin", t.pt_type); write_bin(out + "/boot_pt_n_failed.bin", t.pt_n_failed);
    write_bin(out + "/boot_pt_n_succeeded.bin", t.pt_n_succeeded); write_bin(out + "/boot_pt_obs_offset.bin", t.pt_obs_offset);
    write_bin(out + "/boot_obs_kf.bin", t.obs_kf); write_bin(out + "/boot_obs_px.bin", t.obs_px); write_bin(out + "/boot_obs_f.bin", t.obs_f);
    write_bin(out + "/boot_obs_level.bin", t.obs_level); write_bin(out + "/boot_obs_edgelet.bin", t.obs_edgelet); write_bin(out + "/boot_obs_grad.bin", t.obs_grad);
    write_bin(out + "/boot_cand_point.bin", t.cand_point);
    std::vector<int32_t> inl(tv.inliers_.begin(), tv.inliers_.end());
    std::vector<double> xyz;
    for (const Vector3d& v : tv.xyz_in_cur_) xyz.insert(xyz.end(), v.v, v.v + 3);
    write_bin(out + "/boot_inliers.bin", inl); write_bin(out + "/boot_xyz_in_cur.bin", xyz);
    std::printf("bootstrap: %zu correspondences, status %d, %zu inliers, %zu points, result %d\n", n, tv.status_, tv.inliers_.size(), tv.point_index_.size(), (int)r);
  }
  write_bin(out + "/boot_results.bin", results);
  svo_hip_pyramid_destroy(pyr);
  svo_hip_ctx_destroy(ctx);
  std::printf("bootstrap OK\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 3 && std::string(argv[3]) == "bootstrap") {
    try {
      return bootstrap_demo(argv[1], argv[2]);
    } catch (const std::exception& e) {
      std::fprintf(stderr, "bootstrap demo failed: %s\n", e.what());
      return 1;
    }
  }
  if (argc > 3 && std::string(argv[3]) == "klt") {
    try {
      return klt_demo(argv[1], argv[2]);
    } catch (const std::exception& e) {
      std::fprintf(stderr, "klt demo failed: %s\n", e.what());
      return 1;
    }
  }
  if (argc > 3 && std::string(argv[3]) == "filtergroup") {
    try {
      return filter_group_demo(argv[1], argv[2], argc > 4 && std::string(argv[4]) == "rig");
    } catch (const std::exception& e) {
      std::fprintf(stderr, "svo_host_demo FAILED: %s\n", e.what());
      return 1;
    }
  }
  if (argc > 3 && std::string(argv[3]) == "keyframes") {
    try {
      bool device_seeds = false, threaded = false;
      for (int a = 4; a < argc; ++a) {
        device_seeds = device_seeds || std::string(argv[a]) == "device_seeds";
        threaded = threaded || std::string(argv[a]) == "threaded";
      }
      return keyframes_demo(argv[1], argv[2], device_seeds, threaded);
    } catch (const std::exception& e) {
      std::fprintf(stderr, "svo_host_demo FAILED: %s\n", e.what());
      return 1;
    }
  }
  if (argc < 3) { std::fprintf(stderr, "usage: %s case_dir out_dir [track [incremental] [times] [kf_every E] [max_kfs N] [full_remove] [new_seeds S] [max_points N] [compact] [reloc_at K]|trackgroup n [rig] [staggered]|filtergroup [rig]|churn|keyframes [device_seeds] [threaded]|klt|bootstrap]\n", argv[0]); return 2; }
  const std::string dir = argv[1], out = argv[2];
  if (argc > 3 && std::string(argv[3]) == "trackgroup") {
    try {
      bool rig = false, staggered = false;
      for (int a = 5; a < argc; ++a) { rig = rig || std::string(argv[a]) == "rig"; staggered = staggered || std::string(argv[a]) == "staggered"; }
      return track_group(dir, out, argc > 4 ? std::atoi(argv[4]) : 2, rig, staggered);
    } catch (const std::exception& e) {
      std::fprintf(stderr, "svo_host_demo FAILED: %s\n", e.what());
      return 1;
    }
  }
  if (argc > 3 && std::string(argv[3]) == "churn") {
    try {
      return churn_demo(dir, out);
    } catch (const std::exception& e) {
      std::fprintf(stderr, "svo_host_demo FAILED: %s\n", e.what());
      return 1;
    }
  }
  if (argc > 3 && std::string(argv[3]) == "track") {
    try {
      bool incremental = false, times = false, full_remove = false, compact = false;     // optional trailing arguments
      int max_kfs = 0, kf_every = 0, max_points = 0, new_seeds = 0, reloc_at = -1;
      for (int a = 4; a < argc; ++a) {
        incremental = incremental || std::string(argv[a]) == "incremental";
        times = times || std::string(argv[a]) == "times";
        full_remove = full_remove || std::string(argv[a]) == "full_remove";
        if (std::string(argv[a]) == "max_kfs" && a + 1 < argc) max_kfs = std::atoi(argv[++a]);
        else if (std::string(argv[a]) == "kf_every" && a + 1 < argc) kf_every = std::atoi(argv[++a]);
        else if (std::string(argv[a]) == "max_points" && a + 1 < argc) max_points = std::atoi(argv[++a]);
        else if (std::string(argv[a]) == "new_seeds" && a + 1 < argc) new_seeds = std::atoi(argv[++a]);
        else if (std::string(argv[a]) == "reloc_at" && a + 1 < argc) reloc_at = std::atoi(argv[++a]);
        else if (std::string(argv[a]) == "compact") compact = true;
      }
      return track_lone(dir, out, incremental, times, max_kfs, full_remove, kf_every, max_points, compact, new_seeds, reloc_at);
    } catch (const std::exception& e) {
      std::fprintf(stderr, "svo_host_demo FAILED: %s\n", e.what());
      return 1;
    }
  }
  try {
    const std::vector<double> m = read_bin<double>(dir + "/manifest.bin");   // w h fx fy cx cy n_levels n_frames
    Case c;
    c.cam = PinholeCamera{(int)m[0], (int)m[1], m[2], m[3], m[4], m[5]};
    c.n_levels = (int)m[6]; c.n_frames = (int)m[7];
    if (m.size() >= 13) for (int k = 0; k < 5; ++k) c.cam.d[k] = m[8 + (size_t)k];      // radtan coefficients k1 k2 p1 p2 k3
    for (int k = 0; k < c.n_frames; ++k) c.frames.push_back(load_frame(dir, &c.cam, k, c.n_levels));

    // ---- SparseImgAlign: frame 0 (with features + points) -> frame 1 starting from frame 0's pose
    {
      const auto px = read_bin<double>(dir + "/sia_px.bin"), f = read_bin<double>(dir + "/sia_f.bin"), pos = read_bin<double>(dir + "/sia_pos.bin");
      const auto has = read_bin<uint8_t>(dir + "/sia_has.bin");
      FramePtr ref = c.frames[0];
      std::vector<std::unique_ptr<Point>> points;
      for (size_t i = 0; i < has.size(); ++i) {
        Feature* ftr = new Feature(ref.get(), Vector2d{{px[2 * i], px[2 * i + 1]}}, Vector3d{{f[3 * i], f[3 * i + 1], f[3 * i + 2]}}, 0);
        if (has[i]) { points.emplace_back(new Point(Vector3d{{pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]}})); ftr->point = points.back().get(); }
        ref->fts_.push_back(ftr);
      }
      FramePtr cur = load_frame(dir, &c.cam, 1, c.n_levels);
      cur->T_f_w_ = ref->T_f_w_;                                    // processFrame: new pose starts at the last one (:175)
      SparseImgAlign align(4, 0, 30, SparseImgAlign::GaussNewton, false, false);
      const size_t n_tracked = align.run(ref, cur);
      std::vector<double> res(cur->T_f_w_.p, cur->T_f_w_.p + 7);
      res.push_back((double)n_tracked);
      const auto I = align.getFisherInformation();
      res.insert(res.end(), I.begin(), I.end());
      write_bin(out + "/sia.bin", res);
      // the same pair through NLLSSolver's other branches: Levenberg-Marquardt with setRobustCostFunction(MADScale, HuberWeight)
      {
        FramePtr cur_lm = load_frame(dir, &c.cam, 1, c.n_levels);
        cur_lm->T_f_w_ = ref->T_f_w_;
        SparseImgAlign lm(4, 0, 30, SparseImgAlign::LevenbergMarquardt, false, false);
        lm.setRobustCostFunction(SparseImgAlign::MADScale, SparseImgAlign::HuberWeight);
        const size_t n_lm = lm.run(ref, cur_lm);
        std::vector<double> r2(cur_lm->T_f_w_.p, cur_lm->T_f_w_.p + 7);
        r2.push_back((double)n_lm);
        r2.push_back(lm.getChi2()); r2.push_back((double)lm.scale_); r2.push_back(lm.mu_); r2.push_back(lm.nu_); r2.push_back(lm.stop_ ? 1.0 : 0.0);
        write_bin(out + "/sia_lm.bin", r2);
      }
      // an empty reference frame returns 0 and leaves the pose alone
      FramePtr empty_ref = load_frame(dir, &c.cam, 0, c.n_levels);
      FramePtr cur2 = load_frame(dir, &c.cam, 1, c.n_levels);
      const SE3 before = cur2->T_f_w_;
      if (align.run(empty_ref, cur2) != 0 || std::memcmp(before.p, cur2->T_f_w_.p, sizeof(before.p)) != 0) throw std::runtime_error("empty-frame contract violated");

      // ---- DepthFilter: keyframe 0 with seed batch A, frames 1..kf2-1, keyframe kf2 with seed batch B (the update on a
      // ---- keyframe marks the detector grid), then the remaining frames update seeds of BOTH keyframes
      const auto dm = read_bin<double>(dir + "/depth_mean_min.bin");
      const int kf2 = (int)read_bin<double>(dir + "/second_keyframe.bin")[0];
      struct SeedSet { std::vector<double> px, f; std::vector<int32_t> level; };
      SeedSet setA{read_bin<double>(dir + "/seed_px.bin"), read_bin<double>(dir + "/seed_f.bin"), read_bin<int32_t>(dir + "/seed_level.bin")};
      SeedSet setB{read_bin<double>(dir + "/seedB_px.bin"), read_bin<double>(dir + "/seedB_f.bin"), read_bin<int32_t>(dir + "/seedB_level.bin")};
      auto make_features = [&](const SeedSet& ss, Frame* kf, int id0, std::map<Feature*, int>& index) {
        std::vector<Feature*> fts;
        for (size_t i = 0; i < ss.level.size(); ++i) {
          fts.push_back(new Feature(kf, Vector2d{{ss.px[2 * i], ss.px[2 * i + 1]}}, Vector3d{{ss.f[3 * i], ss.f[3 * i + 1], ss.f[3 * i + 2]}}, ss.level[i]));
          index[fts.back()] = id0 + (int)i;
        }
        return fts;
      };
      const int nA = (int)setA.level.size();
      c.frames[0]->setKeyframe();
      c.frames[kf2]->setKeyframe();
      size_t align_runs = 0;
      std::vector<double> conv_count;
      auto run_protocol = [&](bool threaded, int sub_batch, const std::string& tag, int remove_a_after = -1) {
        Seed::batch_counter = 0;
        std::vector<double> conv;                 // per callback, in callback order: seed id, x, y, z, sigma2
        std::map<Feature*, int> index;
        DetectorGrid grid(c.cam.width, c.cam.height, 30);
        std::vector<Feature*> fa, fb;
        {
          DepthFilter df([&](Point* p, double s2) {
            conv.insert(conv.end(), {(double)index.at(p->obs_.front()), p->pos_[0], p->pos_[1], p->pos_[2], s2});
            delete p;
          }, &grid);
          df.sub_batch_ = sub_batch;
          fa = make_features(setA, c.frames[0].get(), 0, index);
          fb = make_features(setB, c.frames[kf2].get(), nA, index);
          auto wait_idle = [&]() {
            if (!threaded) return;
            while (!df.idle()) {
              FramePtr cur3 = load_frame(dir, &c.cam, 1, c.n_levels);
              cur3->T_f_w_ = ref->T_f_w_;
              if (align.run(ref, cur3) != n_tracked) throw std::runtime_error("alignment changed under concurrency");
              if (std::memcmp(cur3->T_f_w_.p, cur->T_f_w_.p, sizeof(double) * 7) != 0) throw std::runtime_error("pose changed under concurrency");
              ++align_runs;
            }
          };
          if (threaded) df.startThread();
          df.addKeyframe(c.frames[0], dm[0], dm[1], fa);
          wait_idle();
          std::vector<double> frame_us;           // synchronous protocols: what DepthFilter::addFrame (= updateSeeds) took, per frame
          for (int k = 1; k < c.n_frames; ++k) {
            const auto t0 = std::chrono::steady_clock::now();
            if (k == kf2) df.addKeyframe(c.frames[k], dm[0], dm[1], fb);
            else df.addFrame(c.frames[k]);
            if (!threaded) {                      // rows of: us, seeds on the device, uploaded by this call, converged, NaN, list re-read
              frame_us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
              const svo::hip_bridge::SeedBatchStats& ls = df.last_stats_;
              frame_us.insert(frame_us.end(), {(double)ls.n_seeds, (double)ls.n_uploaded, (double)ls.n_converged, (double)ls.n_nan, ls.resynced ? 1.0 : 0.0});
            }
            wait_idle();
            if (k == remove_a_after) {
              // Map::removeKeyframe path (depth_filter.cpp:153-170): every seed of the SECOND keyframe leaves the list BEHIND the
              // device mirror's back (removeKeyframe is not virtual in the reference); a copy taken just before shows the synced state
              std::list<Seed> copy_a;
              df.getSeedsCopy(c.frames[kf2], copy_a);
              std::vector<double> rows;
              for (const Seed& s : copy_a) { rows.push_back((double)index.at(s.ftr)); rows.push_back(s.a); rows.push_back(s.b); rows.push_back(s.mu); rows.push_back(s.sigma2); }
              write_bin(out + "/" + tag + "_copy_b.bin", rows);
              df.removeKeyframe(c.frames[kf2]);
            }
          }
          if (threaded) df.stopThread();
          if (!threaded) write_bin(out + "/" + tag + "_frame_us.bin", frame_us);
          dump_filter(df, index, conv, out, tag);
        }
        std::vector<uint8_t> occ(grid.grid_occupancy_.begin(), grid.grid_occupancy_.end());
        write_bin(out + "/" + tag + "_grid.bin", occ);
        conv_count.push_back((double)conv.size() / 5);
        for (Feature* f2 : fa) delete f2;
        for (Feature* f2 : fb) delete f2;
      };
      run_protocol(false, 4096, "sync");          // (a) synchronous protocol (no thread)
      run_protocol(false, 700, "sync_small");     // (b) the same with small device sub-batches: identical results
      run_protocol(true, 4096, "thread");         // (c) worker thread, while this thread keeps running SparseImgAlign
      run_protocol(false, 1000, "remove", kf2 + 1);   // (d) the second keyframe removed one frame after it came: its seeds vanish from the list
      write_bin(out + "/summary.bin", std::vector<double>{(double)align_runs, conv_count[0], conv_count[1], conv_count[2], conv_count[3]});
    }
    std::printf("svo_host_demo OK\n");
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "svo_host_demo FAILED: %s\n", e.what());
    return 1;
  }
}
