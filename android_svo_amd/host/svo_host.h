// svo_host.h -- self-contained C++ host layer over the C-ABI (include/svo_hip.h).
//
// The reference's public classes (svo::SparseImgAlign, svo::DepthFilter, svo::Seed, Frame/Feature/Point)
// with the same names, methods and protocol, but on minimal own data types (no Eigen, no OpenCV), so that
// the host side can be built and RUN wherever libsvo_hip.so runs.  The bindings that plug into the
// reference's real headers are include/svo_dropin/ (compile-checked only); this file is
// their executable counterpart.  DepthFilter::updateSeeds is NOT a second copy: both sides instantiate
// hip_bridge::DeviceSeedMirror (include/svo_dropin/depth_filter_batch.h) with a small Host policy, so the
// batching / ordering / halt logic the GPU tests exercise is the code the drop-in ships.  The same holds for the tracking
// chain: svo::FrameTracker here and in include/svo_dropin/frame_tracker_hip.h are both hip_bridge::FrameTrackerT
// (frame_tracker_batch.h) -- the flattening of svo::Map's pointer graph into the tracker's index tables and the write-back
// of a frame's outcome (features, counters, Map::safeDeletePoint) run on the GPU from this file's Map / Frame / Point.
// Host logic here:
//   * SparseImgAlign::run       S/sparse_img_align.cpp:51-92   (flatten fts_, upload, run, read back)
//   * DepthFilter protocol      S/depth_filter.cpp:47-229,237-357 (thread, 3-deep frame queue, keyframe
//                               hand-off with the halt flag, std::list<Seed>, age-out, convergence callback)
//   * Map / Frame bookkeeping   S/map.cpp:78-99,256-304 (safeDeletePoint, deleteCandidatePoint), S/frame.cpp:67-165
//                               (setKeyframe, addFeature, setKeyPoints / checkKeyPoints / removeKeyPoint)
// Host threads: the tracking thread and the depth-filter thread each own a svo_hip_ctx (one stream each).
#ifndef SVO_HOST_H_
#define SVO_HOST_H_

#include <algorithm>
#include <array>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <functional>
#include <limits>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <queue>
#include <set>
#include <stdexcept>
#include <thread>
#include <vector>

#include "svo_hip.h"
#include "svo_dropin/slot_table.h"
#include "svo_dropin/depth_filter_batch.h"
#include "svo_dropin/frame_tracker_batch.h"
#include "svo_dropin/klt_init_hip.h"

namespace svo {

struct Vector2d { double v[2]; double& operator[](int i) { return v[i]; } const double& operator[](int i) const { return v[i]; } };
struct Vector3d { double v[3]; double& operator[](int i) { return v[i]; } const double& operator[](int i) const { return v[i]; } };

/// {t, q(xyzw)} with the reference's composition rules (I/SE3.h:35-61, I/SO3.h:468-488,523-526)
struct SE3 {
  double p[7];
  SE3() : p{0, 0, 0, 0, 0, 0, 1} {}
  explicit SE3(const double* s) { std::memcpy(p, s, sizeof(p)); }
  static void rot(const double* q, const double* x, double* o) {
    double uv[3] = {q[1] * x[2] - q[2] * x[1], q[2] * x[0] - q[0] * x[2], q[0] * x[1] - q[1] * x[0]};
    uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
    const double c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
    for (int i = 0; i < 3; ++i) o[i] = (x[i] + q[3] * uv[i]) + c[i];
  }
  SE3 inverse() const {
    SE3 r;
    const double qi[4] = {-p[3], -p[4], -p[5], p[6]};
    double t[3];
    rot(qi, p, t);
    r.p[0] = -t[0]; r.p[1] = -t[1]; r.p[2] = -t[2];
    r.p[3] = qi[0]; r.p[4] = qi[1]; r.p[5] = qi[2]; r.p[6] = qi[3];
    return r;
  }
  Vector3d operator*(const Vector3d& x) const {
    double t[3];
    rot(p + 3, x.v, t);
    return Vector3d{{p[0] + t[0], p[1] + t[1], p[2] + t[2]}};
  }
};

struct PinholeCamera {            // vk::PinholeCamera: pinhole + optional 5-coefficient radtan distortion (S/pinhole_camera.cpp:19-38)
  int width, height;
  double fx, fy, cx, cy;
  double d[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  svo_hip_camera toC() const {
    svo_hip_camera c;
    c.width = width; c.height = height; c.fx = fx; c.fy = fy; c.cx = cx; c.cy = cy;
    for (int k = 0; k < 5; ++k) c.d[k] = d[k];
    c.distortion = std::fabs(d[0]) > 0.0000001 ? 1 : 0;       // distortion_(fabs(d0) > 0.0000001), S/pinhole_camera.cpp:26
    return c;
  }
  /// vk::PinholeCamera::world2cam (S/pinhole_camera.cpp:80-107): the pixel of a point in the camera frame
  Vector2d world2cam(const Vector3d& xyz) const {
    const double x = xyz[0] / xyz[2], y = xyz[1] / xyz[2];
    if (!(std::fabs(d[0]) > 0.0000001)) return Vector2d{{fx * x + cx, fy * y + cy}};
    const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
    const double a1 = 2 * x * y, a2 = r2 + 2 * x * x, a3 = r2 + 2 * y * y;
    const double cdist = 1 + d[0] * r2 + d[1] * r4 + d[4] * r6;
    const double xd = x * cdist + d[2] * a1 + d[3] * a2, yd = y * cdist + d[2] * a3 + d[3] * a1;
    return Vector2d{{xd * fx + cx, yd * fy + cy}};
  }
};

struct Feature;
struct Frame;
struct Point {                                      // I/point.h: position + the features that observe it
  enum PointType { TYPE_DELETED, TYPE_CANDIDATE, TYPE_UNKNOWN, TYPE_GOOD };      // I/point.h:33-38
  Vector3d pos_;
  std::list<Feature*> obs_;
  PointType type_ = TYPE_UNKNOWN;
  int n_failed_reproj_ = 0, n_succeeded_reproj_ = 0;                             // the reprojector's counters (I/point.h:49-50)
  int last_structure_optim_ = 0;                                                 // id of the frame that optimised it last (:51)
  explicit Point(const Vector3d& p) : pos_(p) {}
  Point(const Vector3d& p, Feature* ftr) : pos_(p) { obs_.push_front(ftr); }     // S/point.cpp:39-48
  void addFrameRef(Feature* ftr) { obs_.push_front(ftr); }                       // S/point.cpp:52-55
  bool deleteFrameRef(const Frame* frame);                                       // S/point.cpp:75-86
};
struct Feature {
  enum FeatureType { CORNER, EDGELET };                                          // I/feature.h:26-29
  FeatureType type = CORNER;
  Frame* frame; Vector2d px; Vector3d f; int level; Point* point;
  Vector2d grad{{1.0, 0.0}};                                                     // edgelets: direction of the gradient, normalised
  Feature(Frame* fr, const Vector2d& px_, const Vector3d& f_, int lvl) : frame(fr), px(px_), f(f_), level(lvl), point(nullptr) {}
};
/// the point's observation made in `frame` leaves the list (false: it had none there)
inline bool Point::deleteFrameRef(const Frame* frame) {
  for (auto it = obs_.begin(); it != obs_.end(); ++it)
    if ((*it)->frame == frame) { obs_.erase(it); return true; }
  return false;
}

struct Frame {
  static int frame_counter_;
  int id_;
  const PinholeCamera* cam_;
  SE3 T_f_w_;
  std::vector<std::vector<uint8_t>> img_pyr_;      // level l: (w>>l) x (h>>l), stride == cols
  std::list<Feature*> fts_;
  std::vector<Feature*> key_pts_ = std::vector<Feature*>(5, nullptr);   // five features spread over the image: the keyframe's overlap test
  std::array<double, 36> Cov_{};                   // covariance of the refined pose (pose_optimizer.cpp:141)
  bool is_keyframe_ = false;
  Frame(const PinholeCamera* cam, std::vector<std::vector<uint8_t>> pyr) : id_(frame_counter_++), cam_(cam), img_pyr_(std::move(pyr)) {}
  ~Frame() { for (Feature* f : fts_) delete f; }
  bool isKeyframe() const { return is_keyframe_; }
  Vector3d pos() const { const SE3 T_w_f = T_f_w_.inverse(); return Vector3d{{T_w_f.p[0], T_w_f.p[1], T_w_f.p[2]}}; }   // I/frame.h: the camera centre
  void setKeyframe() { is_keyframe_ = true; setKeyPoints(); }                    // S/frame.cpp:67-71
  void addFeature(Feature* ftr) { fts_.push_back(ftr); }                         // :75-78
  /// S/frame.cpp:162-172: the world point lies in front of the camera and projects into the image
  bool isVisible(const Vector3d& xyz_w) const {
    const Vector3d xyz_f = T_f_w_ * xyz_w;
    if (xyz_f[2] < 0.0) return false;
    const Vector2d px = cam_->world2cam(xyz_f);
    return px[0] >= 0.0 && px[1] >= 0.0 && px[0] < cam_->width && px[1] < cam_->height;
  }

  /// S/frame.cpp:83-92: key features whose point is gone are dropped, then every feature with a point competes again
  void setKeyPoints() {
    for (Feature*& k : key_pts_) if (k != nullptr && k->point == nullptr) k = nullptr;
    for (Feature* ftr : fts_) if (ftr->point != nullptr) checkKeyPoints(ftr);
  }
  /// :98-149.  Slot 0: the feature closest to the image centre (max norm).  Slots 1..4: per quadrant the feature with the
  /// largest product (x - cu)(y - cv); the two left quadrants test x against cv, not cu, as the reference does (:133,142).
  void checkKeyPoints(Feature* ftr) {
    const int cu = cam_->width / 2, cv = cam_->height / 2;
    const double x = ftr->px[0], y = ftr->px[1];
    auto off_centre = [&](const Feature* g) { return std::max(std::fabs(g->px[0] - cu), std::fabs(g->px[1] - cv)); };
    auto product = [&](const Feature* g) { return (g->px[0] - cu) * (g->px[1] - cv); };
    if (key_pts_[0] == nullptr || off_centre(ftr) < off_centre(key_pts_[0])) key_pts_[0] = ftr;
    const bool in_quadrant[4] = {x >= cu && y >= cv, x >= cu && y < cv, x < cv && y < cv, x < cv && y >= cv};
    for (int q = 0; q < 4; ++q) {
      if (!in_quadrant[q]) continue;
      Feature*& slot = key_pts_[1 + q];
      if (slot == nullptr || product(ftr) > product(slot)) slot = ftr;
    }
  }
  /// :154-165
  void removeKeyPoint(Feature* ftr) {
    bool found = false;
    for (Feature*& k : key_pts_) if (k == ftr) { k = nullptr; found = true; }
    if (found) setKeyPoints();
  }
};
inline int Frame::frame_counter_ = 0;
typedef std::shared_ptr<Frame> FramePtr;

namespace hip_bridge {
inline void check(int rc, svo_hip_ctx* ctx, const char* what) {
  if (rc != SVO_HIP_OK) throw std::runtime_error(std::string(what) + ": " + (ctx ? svo_hip_last_error(ctx) : "no context"));
}
/// device copies of frame pyramids, cached by Frame::id_ (the slot bookkeeping is the drop-in's: include/svo_dropin/slot_table.h)
class PyramidCache {
 public:
  PyramidCache(svo_hip_ctx* ctx, int capacity) : ctx_(ctx), table_(capacity) {}
  ~PyramidCache() { if (pyr_) svo_hip_pyramid_destroy(pyr_); }
  int slotOf(const Frame& f) {
    std::vector<const Frame*> one(1, &f);
    std::vector<int> slots;
    acquire(one, slots);
    return slots[0];
  }
  /// all frames of one device call at once: a slot handed out for one of them is not recycled for another
  bool acquire(const std::vector<const Frame*>& frames, std::vector<int>& slots) {
    slots.assign(frames.size(), -1);
    if (frames.empty()) return true;
    std::vector<int> ids;
    std::set<int> distinct;
    for (const Frame* f : frames) { ids.push_back(f->id_); distinct.insert(f->id_); }
    const int need = table_.capacityFor((int)distinct.size());
    // (every frame of a call has the geometry of the first; a cache that holds another geometry starts again)
    const Frame& f = *frames[0];
    const int n_levels = (int)f.img_pyr_.size();
    for (const Frame* g : frames)
      if (g->cam_->width != f.cam_->width || g->cam_->height != f.cam_->height || (int)g->img_pyr_.size() != n_levels) return false;
    if (need != table_.capacity() || !pyr_ || f.cam_->width != width_ || f.cam_->height != height_ || n_levels != n_levels_) {
      if (pyr_) { svo_hip_pyramid_destroy(pyr_); pyr_ = nullptr; }
      check(svo_hip_pyramid_create(ctx_, f.cam_->width, f.cam_->height, n_levels, need, &pyr_), ctx_, "pyramid_create");
      width_ = f.cam_->width; height_ = f.cam_->height; n_levels_ = n_levels;
      table_.reset(need);
      ++n_created_;
    }
    return table_.acquire(ids, slots, [&](size_t k, int s) {
      const Frame& f = *frames[k];
      const uint8_t* lv[SVO_HIP_MAX_LEVELS] = {nullptr};
      for (size_t l = 0; l < f.img_pyr_.size(); ++l) lv[l] = f.img_pyr_[l].data();
      check(svo_hip_pyramid_upload(pyr_, s, lv), ctx_, "pyramid_upload");
      check(svo_hip_ctx_sync(ctx_), ctx_, "sync");
      ++n_uploads_;
      return true;
    });
  }
  svo_hip_pyramid* pyramid() const { return pyr_; }
  int capacity() const { return table_.capacity(); }
  int uploads() const { return n_uploads_; }
 private:
  svo_hip_ctx* ctx_; svo_hip_pyramid* pyr_ = nullptr; int width_ = 0, height_ = 0, n_levels_ = 0; SlotTable table_; int n_uploads_ = 0, n_created_ = 0;
};
}  // namespace hip_bridge

/// I/map.h:34-66, S/map.cpp:256-304: converged seeds that no keyframe holds yet
struct MapPointCandidates {
  typedef std::pair<Point*, Feature*> PointCandidate;
  typedef std::list<PointCandidate> PointCandidateList;
  std::mutex mut_;
  PointCandidateList candidates_;
  std::list<Point*> trash_points_;
  ~MapPointCandidates() {
    for (PointCandidate& c : candidates_) delete c.second;
  }
  /// S/map.cpp:236-254: the candidates the new keyframe observes first become map points; their seed features join the
  /// keyframes they were made in
  template <class FramePtrT>
  void addCandidatePointToFrame(const FramePtrT& frame) {
    std::unique_lock<std::mutex> lock(mut_);
    for (auto it = candidates_.begin(); it != candidates_.end();) {
      if (!it->first->obs_.empty() && it->first->obs_.front()->frame == frame.get()) {
        it->first->type_ = Point::TYPE_UNKNOWN;
        it->first->n_failed_reproj_ = 0;
        it->second->frame->addFeature(it->second);
        it = candidates_.erase(it);
      } else {
        ++it;
      }
    }
  }
  bool deleteCandidatePoint(Point* point) {                                      // S/map.cpp:256-269, :297-304
    std::unique_lock<std::mutex> lock(mut_);
    for (auto it = candidates_.begin(); it != candidates_.end(); ++it) {
      if (it->first != point) continue;
      delete it->second;                           // the candidate's only feature
      it->first->type_ = Point::TYPE_DELETED;
      trash_points_.push_back(it->first);
      candidates_.erase(it);
      return true;
    }
    return false;
  }
  /// S/map.cpp:271-285, :297-304: the candidates whose seed feature was made in `frame` go with it
  template <class FramePtrT>
  void removeFrameCandidates(const FramePtrT& frame) {
    std::unique_lock<std::mutex> lock(mut_);
    for (auto it = candidates_.begin(); it != candidates_.end();) {
      if (it->second->frame != frame.get()) { ++it; continue; }
      delete it->second;
      it->first->type_ = Point::TYPE_DELETED;
      trash_points_.push_back(it->first);
      it = candidates_.erase(it);
    }
  }
};

/// I/map.h:69-130: keyframes + the candidates; points are owned through the features that refer to them
struct Map {
  std::list<FramePtr> keyframes_;
  std::list<Point*> trash_points_;
  MapPointCandidates point_candidates_;
  void addKeyframe(FramePtr kf) { keyframes_.push_back(kf); }                    // S/map.cpp:96-99
  void deletePoint(Point* pt) { pt->type_ = Point::TYPE_DELETED; trash_points_.push_back(pt); }   // :90-94
  /// :78-88: every observation lets go of the point (a keyframe that loses a key feature picks its key features again)
  void safeDeletePoint(Point* pt) {
    for (Feature* ftr : pt->obs_) { ftr->point = nullptr; ftr->frame->removeKeyPoint(ftr); }
    pt->obs_.clear();
    deletePoint(pt);
  }
  size_t size() const { return keyframes_.size(); }
  /// :66-80: a feature of a keyframe that leaves lets go of its point; a point that two features saw at most goes with it,
  /// any other forgets the keyframe
  void removePtFrameRef(Frame* frame, Feature* ftr) {
    Point* pt = ftr->point;
    if (pt == nullptr) return;                     // (gone with an earlier deletion)
    ftr->point = nullptr;
    if (pt->obs_.size() <= 2) { safeDeletePoint(pt); return; }
    pt->deleteFrameRef(frame);
    frame->removeKeyPoint(ftr);
  }
  /// :41-64: the keyframe leaves the map, its candidates with it (false: the map did not hold it)
  bool safeDeleteFrame(FramePtr frame) {
    bool found = false;
    for (auto it = keyframes_.begin(); it != keyframes_.end(); ++it) {
      if (*it != frame) continue;
      for (Feature* ftr : frame->fts_) removePtFrameRef(frame.get(), ftr);
      keyframes_.erase(it);
      found = true;
      break;
    }
    point_candidates_.removeFrameCandidates(frame);
    return found;
  }
  /// :109-131: the keyframes one of whose key points the frame sees, each with the distance between the two translation_vec()
  void getCloseKeyframes(const FramePtr& frame, std::list<std::pair<FramePtr, double>>& close_kfs) const {
    for (const FramePtr& kf : keyframes_)
      for (const Feature* keypoint : kf->key_pts_) {
        if (keypoint == nullptr) continue;
        if (frame->isVisible(keypoint->point->pos_)) {
          const double d[3] = {frame->T_f_w_.p[0] - kf->T_f_w_.p[0], frame->T_f_w_.p[1] - kf->T_f_w_.p[1], frame->T_f_w_.p[2] - kf->T_f_w_.p[2]};
          close_kfs.push_back(std::make_pair(kf, std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])));
          break;                                     // this keyframe has an overlapping field of view
        }
      }
  }
  /// :133-151: the closest of them that is not the frame itself (none: no keyframe is close -- where the reference reads front()
  /// of an empty list after the pop, the twin returns none, as the device does)
  FramePtr getClosestKeyframe(const FramePtr& frame) const {
    std::list<std::pair<FramePtr, double>> close_kfs;
    getCloseKeyframes(frame, close_kfs);
    if (close_kfs.empty()) return nullptr;
    close_kfs.sort([](const std::pair<FramePtr, double>& l, const std::pair<FramePtr, double>& r) { return l.second < r.second; });
    if (close_kfs.front().first != frame) return close_kfs.front().first;
    close_kfs.pop_front();
    return close_kfs.empty() ? nullptr : close_kfs.front().first;
  }
  /// :156-169: the keyframe whose camera centre is furthest from pos (none: no keyframe lies away from it)
  FramePtr getFurthestKeyframe(const Vector3d& pos) const {
    FramePtr furthest;
    double maxdist = 0.0;
    for (const FramePtr& kf : keyframes_) {
      const Vector3d c = kf->pos();
      const double d[3] = {c[0] - pos[0], c[1] - pos[1], c[2] - pos[2]};
      const double dist = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
      if (dist > maxdist) { maxdist = dist; furthest = kf; }
    }
    return furthest;
  }
};

namespace frame_utils {
/// S/frame.cpp:200-221: the depths (T_f_w * pos_).z() of the features that have a point; their median as vk::getMedian takes it
/// (I/math_utils.h:125-131: std::nth_element at size / 2) and their minimum by fmin from the largest double.  false, with
/// depth_mean untouched, for a frame without such a feature.  The host twin of svo_hip_kf_decision's depth pair.
inline bool getSceneDepth(const Frame& frame, double& depth_mean, double& depth_min) {
  std::vector<double> depth_vec;
  depth_vec.reserve(frame.fts_.size());
  depth_min = std::numeric_limits<double>::max();
  for (const Feature* ftr : frame.fts_) {
    if (ftr->point == nullptr) continue;
    const double z = (frame.T_f_w_ * ftr->point->pos_)[2];
    depth_vec.push_back(z);
    depth_min = std::fmin(z, depth_min);
  }
  if (depth_vec.empty()) return false;
  std::vector<double>::iterator it = depth_vec.begin() + depth_vec.size() / 2;
  std::nth_element(depth_vec.begin(), it, depth_vec.end());
  depth_mean = *it;
  return true;
}
}  // namespace frame_utils

/// FrameHandlerMono::needNewKf (S/frame_handler_mono.cpp:391-403) as a free function: no new keyframe while one of the overlap
/// keyframes lies within min_dist (Config::kfSelectMinDist()) scene depths of the frame, the box 1 : 0.8 : 1.3 in the frame's
/// axes.  *blocking (may be NULL): the first keyframe that says so.
inline bool needNewKf(const Frame& frame, const std::vector<std::pair<FramePtr, size_t>>& overlap_kfs, double scene_depth_mean, double min_dist,
                      FramePtr* blocking = nullptr) {
  for (const std::pair<FramePtr, size_t>& kf : overlap_kfs) {
    const Vector3d relpos = frame.T_f_w_ * kf.first->pos();
    if (std::fabs(relpos[0]) / scene_depth_mean < min_dist && std::fabs(relpos[1]) / scene_depth_mean < min_dist * 0.8 &&
        std::fabs(relpos[2]) / scene_depth_mean < min_dist * 1.3) {
      if (blocking) *blocking = kf.first;
      return false;
    }
  }
  return true;
}

/// Host policy of hip_bridge::FrameTrackerT on this file's data model (the drop-in instantiates the same template on the
/// reference's types: include/svo_dropin/frame_tracker_hip.h)
struct HostTrackerPolicy {
  typedef svo::Frame Frame;
  typedef svo::FramePtr FramePtr;
  typedef svo::Feature Feature;
  typedef svo::Point Point;
  typedef svo::Map Map;
  typedef std::list<svo::Feature*> FeatureList;
  typedef MapPointCandidates::PointCandidateList CandidateList;
  static void pose7(const Frame& fr, double T[7]) { std::memcpy(T, fr.T_f_w_.p, sizeof(double) * 7); }
  static void setPose(Frame& fr, const double T[7]) { fr.T_f_w_ = SE3(T); }
  static const uint8_t* level0(const Frame& fr, int* stride, int* cols, int* rows) {
    *stride = fr.cam_->width; *cols = fr.cam_->width; *rows = fr.cam_->height;
    return fr.img_pyr_[0].data();
  }
  static Feature* makeFeature(Frame* fr, const double px[2], const double f[3], int level) {
    return new Feature(fr, Vector2d{{px[0], px[1]}}, Vector3d{{f[0], f[1], f[2]}}, level);
  }
  static void setEdgelet(Feature& ftr, const double g[2]) { ftr.type = Feature::EDGELET; ftr.grad = Vector2d{{g[0], g[1]}}; }
  static bool isEdgelet(const Feature& ftr) { return ftr.type == Feature::EDGELET; }
  static void setCov(Frame& fr, const double cov[36]) { std::memcpy(fr.Cov_.data(), cov, sizeof(double) * 36); }
};

/// The first half of FrameHandlerMono::processFrame (frame_handler_mono.cpp:171-229) in one device call per frame: the
/// executable twin of include/svo_dropin/frame_tracker_hip.h.  cfg: svo_hip_tracker_default_config + the caller's values.
class FrameTracker : public hip_bridge::FrameTrackerT<HostTrackerPolicy> {
 public:
  FrameTracker(const PinholeCamera& cam, const svo_hip_tracker_config& cfg) : hip_bridge::FrameTrackerT<HostTrackerPolicy>(cam.toC(), cfg) {}
};

/// FrameHandlerMono::relocalizeFrame (frame_handler_mono.cpp:317-349) as addImage calls it (:80-82: against
/// map_.getClosestKeyframe(last_frame_)), on the bridge: with FrameTrackerT::setDeviceRelocalisation(true) the keyframe is chosen,
/// the gate is run and the frame is tracked by ONE device call and the map is not flattened; otherwise, or when the device
/// refuses, the keyframe is chosen on the objects and goes up as the last frame (the path there was before, without a gate).
/// last_frame: the caller's last_frame_, set to the reference keyframe when the gate accepted (:337).  ref_keyframe: NULL = the
/// closest one.  quality_min_fts: Config::qualityMinFts() (processFrame :208-215; :231-232 asks for 20 edges).
enum UpdateResult { RESULT_NO_KEYFRAME, RESULT_IS_KEYFRAME, RESULT_FAILURE };      // I/frame_handler_base.h:60-64
template <class Tracker>
inline UpdateResult relocalizeFrame(Tracker& tracker, Map& map, FramePtr& last_frame, const FramePtr& new_frame, FramePtr ref_keyframe,
                                    std::vector<std::pair<FramePtr, size_t>>& overlap_kfs, typename Tracker::Outcome& out, size_t quality_min_fts,
                                    int min_tracked = 30) {
  bool accepted = false;
  FramePtr ref_used;
  const FramePtr exclude = last_frame->isKeyframe() ? last_frame : FramePtr();
  bool ok = tracker.relocalize(ref_keyframe, last_frame->T_f_w_.p, new_frame, map, overlap_kfs, out, &accepted, &ref_used, min_tracked, exclude);
  if (!ok && ref_keyframe == nullptr) {                     // (the old path has nothing to start from: choose on the objects)
    ref_keyframe = map.getClosestKeyframe(last_frame);
    if (ref_keyframe == nullptr) return RESULT_FAILURE;     // "No reference keyframe." (:322-326)
    ok = tracker.relocalize(ref_keyframe, last_frame->T_f_w_.p, new_frame, map, overlap_kfs, out, &accepted, &ref_used, min_tracked, exclude);
  }
  if (!ok || ref_used == nullptr || !accepted) return RESULT_FAILURE;
  const SE3 T_f_w_last = last_frame->T_f_w_;
  last_frame = ref_used;                                    // :337
  if (out.repr_n_matches < quality_min_fts || out.sfba_n_edges_final < 20) {     // processFrame returned RESULT_FAILURE
    new_frame->T_f_w_ = T_f_w_last;                         // reset to last well localized pose (:345)
    tracker.lastFrameChanged();
    return RESULT_FAILURE;
  }
  return RESULT_NO_KEYFRAME;
}

/// N cameras with a map each, tracked together (hip_bridge::FrameTrackerGroupT on this file's data model; svo_hip_tracker_group)
class FrameTrackerGroup : public hip_bridge::FrameTrackerGroupT<HostTrackerPolicy> {
 public:
  FrameTrackerGroup(const PinholeCamera& cam, const svo_hip_tracker_config& cfg, int n_cameras)
      : hip_bridge::FrameTrackerGroupT<HostTrackerPolicy>(cam.toC(), cfg, n_cameras) {}
  /// a rig: camera c tracks with cams[c] (one image size; a device group of per-camera models when they differ)
  FrameTrackerGroup(const std::vector<const PinholeCamera*>& cams, const svo_hip_tracker_config& cfg)
      : hip_bridge::FrameTrackerGroupT<HostTrackerPolicy>(toC(cams), cfg) {}

 private:
  static std::vector<svo_hip_camera> toC(const std::vector<const PinholeCamera*>& cams) {
    std::vector<svo_hip_camera> out;
    for (const PinholeCamera* c : cams) out.push_back(c->toC());
    return out;
  }
};

/// I/sparse_img_align.h:33-79
class SparseImgAlign {
 public:
  enum Method { GaussNewton, LevenbergMarquardt };                             // I/nlls_solver.h:46-48
  enum ScaleEstimatorType { UnitScale, TDistScale, MADScale, NormalScale };
  enum WeightFunctionType { UnitWeight, TDistWeight, TukeyWeight, HuberWeight };
  size_t n_iter_; double eps_; bool stop_ = false; size_t n_meas_ = 0;
  Method method_;
  double mu_ = 0.01f, nu_ = 2.0;
  float scale_ = 0.0f;
  SparseImgAlign(int n_levels, int min_level, int n_iter, Method method, bool display, bool verbose)
      : n_iter_(n_iter), eps_(0.000001), method_(method), max_level_(n_levels), min_level_(min_level) {
    (void)display; (void)verbose;
    hip_bridge::check(svo_hip_ctx_create(&ctx_, 0, nullptr), nullptr, "ctx_create");
    ref_.reset(new hip_bridge::PyramidCache(ctx_, 1));
    cur_.reset(new hip_bridge::PyramidCache(ctx_, 1));
  }
  ~SparseImgAlign() { if (sia_) svo_hip_sia_destroy(sia_); ref_.reset(); cur_.reset(); svo_hip_ctx_destroy(ctx_); }

  /// NLLSSolver::setRobustCostFunction (I/nlls_solver_impl.hpp:229-281): UnitScale switches the weights off
  void setRobustCostFunction(ScaleEstimatorType scale_estimator, WeightFunctionType weight_function) {
    scale_kind_ = (int)scale_estimator; weight_kind_ = (int)weight_function;
  }

  size_t run(FramePtr ref_frame, FramePtr cur_frame) {
    stop_ = false; n_meas_ = 0; chi2_ = 1e10;
    if (ref_frame->fts_.empty()) return 0;                                   // :55-59
    const int n = (int)ref_frame->fts_.size();
    std::vector<double> px(2 * (size_t)n), f(3 * (size_t)n), pos(3 * (size_t)n, 0.0);
    std::vector<uint8_t> hp((size_t)n, 0);
    size_t i = 0;
    for (Feature* ftr : ref_frame->fts_) {                                    // list order defines the patch order
      px[2 * i] = ftr->px[0]; px[2 * i + 1] = ftr->px[1];
      for (int k = 0; k < 3; ++k) f[3 * i + k] = ftr->f[k];
      if (ftr->point) { hp[i] = 1; for (int k = 0; k < 3; ++k) pos[3 * i + k] = ftr->point->pos_[k]; }
      ++i;
    }
    if (!sia_ || cap_ < n) {
      if (sia_) svo_hip_sia_destroy(sia_);
      cap_ = n > 2048 ? n : 2048;
      hip_bridge::check(svo_hip_sia_create(ctx_, 1, cap_, &sia_), ctx_, "sia_create");
    }
    const int rs = ref_->slotOf(*ref_frame), cs = cur_->slotOf(*cur_frame);
    (void)rs; (void)cs;
    const svo_hip_camera cam = cur_frame->cam_->toC();
    svo_hip_sia_params prm{max_level_, min_level_, (int)n_iter_, eps_, 1};
    svo_hip_sia_result res;
    hip_bridge::check(svo_hip_sia_set_option(sia_, SVO_HIP_SIA_OPT_METHOD, method_ == LevenbergMarquardt ? SVO_HIP_SIA_METHOD_LEVENBERG_MARQUARDT
                                                                                                         : SVO_HIP_SIA_METHOD_GAUSS_NEWTON), ctx_, "set_option");
    hip_bridge::check(svo_hip_sia_set_option(sia_, SVO_HIP_SIA_OPT_SCALE_ESTIMATOR, scale_kind_), ctx_, "set_option");
    hip_bridge::check(svo_hip_sia_set_option(sia_, SVO_HIP_SIA_OPT_WEIGHT_FUNCTION, weight_kind_), ctx_, "set_option");
    hip_bridge::check(svo_hip_sia_set_frames(sia_, ref_->pyramid(), cur_->pyramid()), ctx_, "set_frames");
    hip_bridge::check(svo_hip_sia_upload_features(sia_, 0, n, px.data(), f.data(), pos.data(), hp.data()), ctx_, "upload_features");
    hip_bridge::check(svo_hip_sia_upload_poses(sia_, 0, &cam, ref_frame->T_f_w_.p, cur_frame->T_f_w_.p), ctx_, "upload_poses");
    hip_bridge::check(svo_hip_sia_run(sia_, 1, &prm), ctx_, "run");
    hip_bridge::check(svo_hip_sia_download(sia_, 0, &res), ctx_, "download");
    cur_frame->T_f_w_ = SE3(res.T_cur_w);                                     // :89
    std::memcpy(H_.data(), res.H, sizeof(res.H));
    chi2_ = res.chi2; stop_ = res.stop != 0; n_meas_ = (size_t)res.n_tracked * 16;
    if (method_ == LevenbergMarquardt || scale_kind_ != SVO_HIP_SIA_SCALE_UNIT)
      hip_bridge::check(svo_hip_sia_solver_state(sia_, 0, &scale_, &mu_, &nu_), ctx_, "solver_state");
    return (size_t)res.n_tracked;                                             // :91
  }
  std::array<double, 36> getFisherInformation() const {                       // :94-99
    std::array<double, 36> I = H_;
    const double sigma_i_sq = 5e-4 * 255 * 255;
    for (double& v : I) v /= sigma_i_sq;
    return I;
  }
  double getChi2() const { return chi2_; }

 private:
  int max_level_, min_level_;
  int scale_kind_ = SVO_HIP_SIA_SCALE_UNIT, weight_kind_ = SVO_HIP_SIA_WEIGHT_UNIT;
  svo_hip_ctx* ctx_ = nullptr;
  svo_hip_sia* sia_ = nullptr;
  int cap_ = 0;
  std::unique_ptr<hip_bridge::PyramidCache> ref_, cur_;
  std::array<double, 36> H_{};
  double chi2_ = 1e10;
};

/// The detector grid of feature_detection::AbstractDetector (S/feature_detection.cpp:24-64): cells the depth filter
/// marks on keyframes so that initializeSeeds does not seed again where a live seed was just matched.
struct DetectorGrid {
  int cell_size_, grid_n_cols_, grid_n_rows_;
  std::vector<bool> grid_occupancy_;
  DetectorGrid(int img_width, int img_height, int cell_size)
      : cell_size_(cell_size), grid_n_cols_((int)std::ceil((double)img_width / cell_size)),
        grid_n_rows_((int)std::ceil((double)img_height / cell_size)), grid_occupancy_((size_t)grid_n_cols_ * grid_n_rows_, false) {}
  void resetGrid() { std::fill(grid_occupancy_.begin(), grid_occupancy_.end(), false); }
  void setGridOccpuancy(const Vector2d& px) {                                   // :58-64 (spelling as in the reference)
    grid_occupancy_.at((size_t)((int)(px[1] / cell_size_) * grid_n_cols_ + (int)(px[0] / cell_size_))) = true;
  }
};

/// I/depth_filter.h:36-52
struct Seed {
  static int batch_counter, seed_counter;
  int batch_id, id;
  Feature* ftr;
  float a, b, mu, z_range, sigma2;
  Seed(Feature* ftr_, float depth_mean, float depth_min)
      : batch_id(batch_counter), id(seed_counter++), ftr(ftr_), a(10), b(10), mu((float)(1.0 / depth_mean)),
        z_range((float)(1.0 / depth_min)), sigma2(z_range * z_range / 36) {}
};
inline int Seed::batch_counter = 0;
inline int Seed::seed_counter = 0;

/// I/depth_filter.h:60-166.  The detector is out of scope: the new keyframe's features are handed in.
class DepthFilter {
 public:
  typedef std::unique_lock<std::mutex> lock_t;
  typedef std::function<void(Point*, double)> callback_t;
  struct Options {
    int max_n_kfs = 3;
    double seed_convergence_sigma2_thresh = 100.0;
    bool verbose = false;
  } options_;

  explicit DepthFilter(callback_t seed_converged_cb, DetectorGrid* feature_detector = nullptr)
      : feature_detector_(feature_detector), seed_converged_cb_(std::move(seed_converged_cb)) {
    hip_bridge::check(svo_hip_ctx_create(&ctx_, 0, nullptr), nullptr, "ctx_create");   // the filter thread's own stream
    kf_pyr_.reset(new hip_bridge::PyramidCache(ctx_, 8));
    cur_pyr_.reset(new hip_bridge::PyramidCache(ctx_, 2));
  }
  virtual ~DepthFilter() {
    stopThread(); mirror_.clear(); kf_pyr_.reset(); cur_pyr_.reset();
    if (grid_dev_) svo_hip_free(ctx_, grid_dev_);
    svo_hip_ctx_destroy(ctx_);
  }

  /// initializeSeeds on the device (svo_hip_seed_batch_create_detected) for the keyframes queued with
  /// addKeyframe(frame, depth_mean, depth_min): FastDetector(img_width, img_height, cell_size, n_pyr_levels) and
  /// Config::triangMinCornerScore() of the reference's constructor arguments (depth_filter.cpp:129-151)
  void enableDeviceSeedInit(int n_pyr_levels, int cell_size, double detection_threshold) {
    if (n_pyr_levels < 1 || cell_size < 1) throw std::invalid_argument("enableDeviceSeedInit");
    dev_n_pyr_levels_ = n_pyr_levels; dev_cell_size_ = cell_size; dev_detection_threshold_ = detection_threshold;
    device_seed_init_ = true;
  }

  void startThread() { thread_stop_ = false; thread_ = new std::thread(&DepthFilter::updateSeedsLoop, this); }
  void stopThread() {
    if (thread_ != nullptr) {
      seeds_updating_halt_ = true;
      { lock_t lock(frame_queue_mut_); thread_stop_ = true; }
      frame_queue_cond_.notify_one();
      if (thread_->joinable()) thread_->join();
      delete thread_;
      thread_ = nullptr;
    }
  }
  void addFrame(FramePtr frame) {                                              // depth_filter.cpp:87-104
    if (thread_ != nullptr) {
      {
        lock_t lock(frame_queue_mut_);
        if (frame_queue_.size() > 2) frame_queue_.pop();
        frame_queue_.push(frame);
      }
      seeds_updating_halt_ = false;
      frame_queue_cond_.notify_one();
    } else {
      updateSeeds(frame);
    }
  }
  void addKeyframe(FramePtr frame, double depth_mean, double depth_min, std::vector<Feature*> new_features) {   // :109-123
    new_keyframe_min_depth_ = depth_min;
    new_keyframe_mean_depth_ = depth_mean;
    if (thread_ != nullptr) {
      lock_t lock(frame_queue_mut_);
      new_keyframe_ = frame;
      new_keyframe_features_ = std::move(new_features);
      new_keyframe_on_device_ = false;
      new_keyframe_set_ = true;
      seeds_updating_halt_ = true;
      frame_queue_cond_.notify_one();
    } else {
      initializeSeeds(frame, new_features);
    }
  }
  /// :109-123 with the detector inside the filter, as in the reference: no feature list.  The keyframe's existing features
  /// (frame->fts_) and, on the threaded path, the seeds its update has just matched occupy the grid; the new features are detected
  /// on the filter's own copy of the keyframe's pyramid and their seeds are born on the device.  The Feature objects the filter
  /// creates belong to the caller, like handed-in ones: takeDeviceFeatures() returns those made since its last call.
  void addKeyframe(FramePtr frame, double depth_mean, double depth_min) {
    if (!device_seed_init_) throw std::logic_error("addKeyframe without features: enableDeviceSeedInit comes first");
    new_keyframe_min_depth_ = depth_min;
    new_keyframe_mean_depth_ = depth_mean;
    if (thread_ != nullptr) {
      lock_t lock(frame_queue_mut_);
      new_keyframe_ = frame;
      new_keyframe_features_.clear();
      new_keyframe_on_device_ = true;
      new_keyframe_set_ = true;
      seeds_updating_halt_ = true;
      frame_queue_cond_.notify_one();
    } else {
      initializeSeedsOnDevice(frame);
    }
  }
  std::vector<Feature*> takeDeviceFeatures() {
    lock_t lock(seeds_mut_);
    std::vector<Feature*> out;
    out.swap(device_features_);
    return out;
  }
  void removeKeyframe(FramePtr frame) {                                        // :153-170
    seeds_updating_halt_ = true;
    lock_t lock(seeds_mut_);
    for (auto it = seeds_.begin(); it != seeds_.end();) it = (it->ftr->frame == frame.get()) ? seeds_.erase(it) : std::next(it);
    seeds_updating_halt_ = false;
  }
  void reset() {                                                               // :172-186
    seeds_updating_halt_ = true;
    { lock_t lock(seeds_mut_); seeds_.clear(); }
    lock_t lock(frame_queue_mut_);
    while (!frame_queue_.empty()) frame_queue_.pop();
    seeds_updating_halt_ = false;
  }
  /// The seeds' state lives on the device between frames (hip_bridge::DeviceSeedMirror): bring it into the list
  void syncSeeds() {
    lock_t lock(seeds_mut_);
    if (!mirror_.syncToHost()) throw std::runtime_error(std::string("seed_batch_download: ") + svo_hip_last_error(ctx_));
  }
  std::list<Seed>& getSeeds() { syncSeeds(); return seeds_; }
  void getSeedsCopy(const FramePtr& frame, std::list<Seed>& seeds) {           // :349-357
    lock_t lock(seeds_mut_);
    if (!mirror_.syncToHost()) throw std::runtime_error(std::string("seed_batch_download: ") + svo_hip_last_error(ctx_));
    for (const Seed& s : seeds_) if (s.ftr->frame == frame.get()) seeds.push_back(s);
  }
  bool idle() {
    lock_t lock(frame_queue_mut_);
    return frame_queue_.empty() && !new_keyframe_set_ && !busy_;
  }

 protected:
  void initializeSeeds(FramePtr frame, const std::vector<Feature*>& new_features) {   // :129-151
    (void)frame;
    seeds_updating_halt_ = true;
    lock_t lock(seeds_mut_);
    ++Seed::batch_counter;
    for (Feature* ftr : new_features) seeds_.push_back(Seed(ftr, (float)new_keyframe_mean_depth_, (float)new_keyframe_min_depth_));
    seeds_updating_halt_ = false;
  }

  /// initializeSeeds (:129-151) as one device call: setExistingFeatures(frame->fts_) on the device grid, detection and seed
  /// construction into a pool block, the grid reset behind it; one Feature and one list entry per returned feature; the batch
  /// joins the mirror without an upload
  void initializeSeedsOnDevice(FramePtr frame) {
    seeds_updating_halt_ = true;
    lock_t lock(seeds_mut_);
    const hip_bridge::DeviceGrid grid = deviceGrid(*frame);
    std::vector<double> px;
    for (const Feature* ftr : frame->fts_) { px.push_back(ftr->px[0]); px.push_back(ftr->px[1]); }
    hip_bridge::check(svo_hip_grid_mark_px(ctx_, (int)(px.size() / 2), px.data(), grid.cell_size, grid.grid_cols, grid.grid_rows,
                                           grid.occupancy_dev), ctx_, "grid_mark_px");
    if (record_detector_grid_) {
      last_detector_grid_.resize((size_t)grid.grid_cols * grid.grid_rows);
      hip_bridge::check(svo_hip_memcpy_d2h(ctx_, last_detector_grid_.data(), grid.occupancy_dev, last_detector_grid_.size()), ctx_, "grid d2h");
    }
    const int slot = kf_pyr_->slotOf(*frame);
    const svo_hip_camera cam = frame->cam_->toC();
    const size_t n_cells = (size_t)grid.grid_cols * grid.grid_rows;
    std::vector<double> fpx(2 * n_cells), ff(3 * n_cells);
    std::vector<int32_t> level(n_cells);
    svo_hip_seed_batch* batch = nullptr;
    int32_t n = 0;
    hip_bridge::check(svo_hip_seed_batch_create_detected(ctx_, kf_pyr_->pyramid(), slot, &cam, dev_n_pyr_levels_, grid.cell_size,
                                                         grid.occupancy_dev, 1, dev_detection_threshold_, (float)new_keyframe_mean_depth_,
                                                         (float)new_keyframe_min_depth_, &batch, &n, fpx.data(), ff.data(), level.data(),
                                                         nullptr), ctx_, "seed_batch_create_detected");
    ++Seed::batch_counter;
    std::list<Seed>::iterator first = seeds_.end();
    for (int32_t i = 0; i < n; ++i) {
      Feature* ftr = new Feature(frame.get(), Vector2d{{fpx[2 * (size_t)i], fpx[2 * (size_t)i + 1]}},
                                 Vector3d{{ff[3 * (size_t)i], ff[3 * (size_t)i + 1], ff[3 * (size_t)i + 2]}}, level[(size_t)i]);
      device_features_.push_back(ftr);
      seeds_.push_back(Seed(ftr, (float)new_keyframe_mean_depth_, (float)new_keyframe_min_depth_));
      if (i == 0) first = std::prev(seeds_.end());
    }
    mirror_.adopt(batch, first, (size_t)n, Seed::batch_counter, frame.get());
    seeds_updating_halt_ = false;
  }

  /// the device grid of enableDeviceSeedInit for this frame's image size (allocated and zeroed when first needed)
  hip_bridge::DeviceGrid deviceGrid(const Frame& frame) {
    int gc = 0, gr = 0;
    hip_bridge::check(svo_hip_detect_grid(frame.cam_->width, frame.cam_->height, dev_cell_size_, &gc, &gr), ctx_, "detect_grid");
    if (grid_dev_ == nullptr || gc != grid_cols_ || gr != grid_rows_) {
      if (grid_dev_) { hip_bridge::check(svo_hip_ctx_sync(ctx_), ctx_, "sync"); svo_hip_free(ctx_, grid_dev_); grid_dev_ = nullptr; }
      void* p = nullptr;
      hip_bridge::check(svo_hip_malloc(ctx_, &p, (size_t)gc * gr), ctx_, "malloc");
      grid_dev_ = static_cast<uint8_t*>(p);
      grid_cols_ = gc; grid_rows_ = gr;
      const std::vector<uint8_t> zero((size_t)gc * gr, 0);
      hip_bridge::check(svo_hip_memcpy_h2d(ctx_, grid_dev_, zero.data(), zero.size()), ctx_, "grid h2d");
      hip_bridge::check(svo_hip_ctx_sync(ctx_), ctx_, "sync");
    }
    return hip_bridge::DeviceGrid{dev_cell_size_, grid_cols_, grid_rows_, grid_dev_};
  }

  void updateSeedsLoop() {                                                      // :191-229
    while (true) {
      FramePtr frame;
      std::vector<Feature*> feats;
      bool is_kf = false, on_device = false;
      {
        lock_t lock(frame_queue_mut_);
        while (frame_queue_.empty() && !new_keyframe_set_ && !thread_stop_) frame_queue_cond_.wait(lock);
        if (thread_stop_) return;
        if (new_keyframe_set_) {
          new_keyframe_set_ = false;
          seeds_updating_halt_ = false;
          while (!frame_queue_.empty()) frame_queue_.pop();
          frame = new_keyframe_;
          feats = std::move(new_keyframe_features_);
          is_kf = true;
          on_device = new_keyframe_on_device_;
        } else {
          frame = frame_queue_.front();
          frame_queue_.pop();
        }
        busy_ = true;
      }
      // (a keyframe whose seeds are made on the device: its update marks the device grid, :302-306)
      grid_pass_ = is_kf && on_device;
      updateSeeds(frame);
      grid_pass_ = false;
      if (is_kf && on_device) initializeSeedsOnDevice(frame);
      else if (is_kf) initializeSeeds(frame, feats);
      { lock_t lock(frame_queue_mut_); busy_ = false; }
    }
  }

  /// Host policy of hip_bridge::DeviceSeedMirror on this file's data model
  struct BatchHost {
    DepthFilter* df;
    Frame* keyframeOf(const Seed& s) const { return s.ftr->frame; }
    void feature(const Seed& s, double px[2], double f[3], int* level) const {
      px[0] = s.ftr->px[0]; px[1] = s.ftr->px[1];
      for (int k = 0; k < 3; ++k) f[k] = s.ftr->f[k];
      *level = s.ftr->level;
    }
    void pose7(const Frame& fr, double T[7]) const { std::memcpy(T, fr.T_f_w_.p, sizeof(double) * 7); }
    bool keyframeSlots(const std::vector<Frame*>& kfs, std::vector<int>& slots) {
      std::vector<const Frame*> c(kfs.begin(), kfs.end());
      return df->kf_pyr_->acquire(c, slots);
    }
    int currentSlot(Frame& fr) { return df->cur_pyr_->slotOf(fr); }
    svo_hip_pyramid* keyframePyramids() const { return df->kf_pyr_->pyramid(); }
    svo_hip_pyramid* currentPyramids() const { return df->cur_pyr_->pyramid(); }
    svo_hip_camera camera(const Frame& fr) const { return fr.cam_->toC(); }
    bool isKeyframe(const Frame& fr) const { return fr.isKeyframe(); }
    void setGridOccupancy(const double px_cur[2]) {                              // depth_filter.cpp:302-306
      if (df->feature_detector_) df->feature_detector_->setGridOccpuancy(Vector2d{{px_cur[0], px_cur[1]}});
    }
    void converged(Seed& s, const double xyz[3]) {                               // :310-331
      Point* point = new Point(Vector3d{{xyz[0], xyz[1], xyz[2]}}, s.ftr);
      s.ftr->point = point;
      df->seed_converged_cb_(point, s.sigma2);
    }
  };

  /// depth_filter.cpp:237-341 through the shared batched implementation
  virtual void updateSeeds(FramePtr frame) {
    lock_t lock(seeds_mut_);
    if (seeds_.empty()) return;
    svo_hip_df_params prm{3, 10, 1000, options_.seed_convergence_sigma2_thresh};
    BatchHost host{this};
    hip_bridge::DeviceGrid grid{0, 0, 0, nullptr};
    if (grid_pass_) grid = deviceGrid(*frame);
    last_stats_ = mirror_.update(host, ctx_, seeds_, *frame, prm, Seed::batch_counter, options_.max_n_kfs, seeds_updating_halt_, sub_batch_,
                                 grid_pass_ ? &grid : nullptr);
    total_uploaded_ += last_stats_.n_uploaded;
    if (last_stats_.n_device_errors) throw std::runtime_error(std::string("depth_filter_update: ") + svo_hip_last_error(ctx_));
  }

 public:
  int sub_batch_ = 4096;                         ///< seeds per device batch (the halt flag is polled in between)
  hip_bridge::SeedBatchStats last_stats_;
  long total_uploaded_ = 0;                      ///< seeds ever uploaded to the device mirror (seeds born on the device: never)
  bool record_detector_grid_ = false;            ///< tests: keep the grid as the device detector saw it (one more transfer a keyframe)
  std::vector<uint8_t> last_detector_grid_;
 protected:
  DetectorGrid* feature_detector_ = nullptr;
  callback_t seed_converged_cb_;
  std::list<Seed> seeds_;
  hip_bridge::DeviceSeedMirror<std::list<Seed> > mirror_;    // the seeds' device-resident state
  std::mutex seeds_mut_;
  volatile bool seeds_updating_halt_ = false;
  bool thread_stop_ = false;
  std::thread* thread_ = nullptr;
  std::queue<FramePtr> frame_queue_;
  std::mutex frame_queue_mut_;
  std::condition_variable frame_queue_cond_;
  FramePtr new_keyframe_;
  std::vector<Feature*> new_keyframe_features_;
  bool new_keyframe_set_ = false, busy_ = false;
  bool new_keyframe_on_device_ = false;          // the queued keyframe came without features (enableDeviceSeedInit)
  bool device_seed_init_ = false, grid_pass_ = false;
  int dev_n_pyr_levels_ = 3, dev_cell_size_ = 30;
  double dev_detection_threshold_ = 10.0;
  uint8_t* grid_dev_ = nullptr;                  // the detector grid on the filter's context
  int grid_cols_ = 0, grid_rows_ = 0;
  std::vector<Feature*> device_features_;        // made by initializeSeedsOnDevice, not yet taken by the caller
  double new_keyframe_min_depth_ = 0.0, new_keyframe_mean_depth_ = 0.0;
  svo_hip_ctx* ctx_ = nullptr;
  std::unique_ptr<hip_bridge::PyramidCache> kf_pyr_, cur_pyr_;
};

/// The depth filters of N cameras (one image size, every camera with the model of its frames) on ONE context, unthreaded: the
/// counterpart of FrameTrackerGroup.  One
/// keyframe PyramidCache and one current-frame cache are shared by the cameras; every camera has its own seed list, device mirror,
/// convergence callback, detector grid and keyframe-batch counter.  addFrames() is DepthFilter::updateSeeds of all cameras as ONE
/// device pass (hip_bridge::updateCameraRig -> svo_hip_seed_batch_update_cameras_async, or svo_hip_seed_batch_update_rig_async when the
/// cameras' models differ); each camera's callbacks, grid marks and
/// erasures come in the order of a lone DepthFilter fed the same frames (tests/test_gpu_depth_filter_group_cpp.py).
/// Frame ids are what the shared caches know a pyramid by: they must be unique across the cameras (Frame::frame_counter_ is).
class DepthFilterGroup {
 public:
  typedef DepthFilter::callback_t callback_t;
  DepthFilter::Options options_;
  int sub_batch_ = 4096;
  std::vector<hip_bridge::SeedBatchStats> last_stats_;        ///< per camera, of the last addFrames (a camera that sat out: zeros)

  /// cbs[c]: seed_converged_cb of camera c; detectors[c] (optional): its feature detector's grid
  explicit DepthFilterGroup(std::vector<callback_t> cbs, std::vector<DetectorGrid*> detectors = std::vector<DetectorGrid*>()) {
    hip_bridge::check(svo_hip_ctx_create(&ctx_, 0, nullptr), nullptr, "ctx_create");
    kf_pyr_.reset(new hip_bridge::PyramidCache(ctx_, 16));
    cur_pyr_.reset(new hip_bridge::PyramidCache(ctx_, (int)std::max<size_t>(cbs.size(), 1)));
    for (size_t c = 0; c < cbs.size(); ++c) {
      cams_.emplace_back(new Camera);
      cams_.back()->cb = std::move(cbs[c]);
      cams_.back()->detector = c < detectors.size() ? detectors[c] : nullptr;
    }
    last_stats_.resize(cams_.size());
  }
  ~DepthFilterGroup() {
    for (auto& cam : cams_) cam->mirror.clear();
    kf_pyr_.reset(); cur_pyr_.reset();
    svo_hip_ctx_destroy(ctx_);
  }
  size_t cameras() const { return cams_.size(); }

  /// DepthFilter::addKeyframe of camera c without a thread: initializeSeeds (depth_filter.cpp:129-151) under the camera's own batch
  /// counter (the reference's is one static for its one filter; age-out compares it with a seed's batch id)
  void addKeyframe(size_t c, FramePtr frame, double depth_mean, double depth_min, const std::vector<Feature*>& new_features) {
    (void)frame;
    Camera& cam = *cams_.at(c);
    Seed::batch_counter = ++cam.batch_counter;
    for (Feature* ftr : new_features) cam.seeds.push_back(Seed(ftr, (float)depth_mean, (float)depth_min));
  }

  /// DepthFilter::addFrame for every camera, frames[c] camera c's new frame (null: the camera sits this pass out): ONE device pass
  void addFrames(const std::vector<FramePtr>& frames) {
    if (frames.size() != cams_.size()) throw std::invalid_argument("addFrames: one frame (or null) per camera");
    std::vector<Mirror*> mirrors;
    std::vector<GroupHost> host_objs;
    std::vector<std::list<Seed>*> lists;
    std::vector<Frame*> frs;
    std::vector<int> counters;
    std::vector<size_t> who;
    std::vector<const Frame*> all_kfs, all_cur;
    for (size_t c = 0; c < cams_.size(); ++c) {
      last_stats_[c] = hip_bridge::SeedBatchStats();
      Camera& cam = *cams_[c];
      if (!frames[c] || cam.seeds.empty()) continue;
      who.push_back(c);
      mirrors.push_back(&cam.mirror); lists.push_back(&cam.seeds); frs.push_back(frames[c].get()); counters.push_back(cam.batch_counter);
      host_objs.push_back(GroupHost{this, &cam});
      all_cur.push_back(frames[c].get());
      const Frame* prev = nullptr;
      for (const Seed& s : cam.seeds)
        if (s.ftr->frame != prev) { prev = s.ftr->frame; if (std::find(all_kfs.begin(), all_kfs.end(), prev) == all_kfs.end()) all_kfs.push_back(prev); }
    }
    if (who.empty()) return;
    // The caches are shared: every keyframe that owns a seed of ANY camera and every current frame of the pass is made resident
    // here, together, before the first camera resolves its slots.  The cameras' own look-ups in phase 1 then only find resident
    // frames -- a resident frame keeps its slot (slot_table.h) -- so no camera's look-up can recycle a slot that another camera of
    // the same pass was given.
    std::vector<int> slots;
    if (!kf_pyr_->acquire(all_kfs, slots) || !cur_pyr_->acquire(all_cur, slots)) throw std::runtime_error("DepthFilterGroup: frames of different geometry");
    std::vector<GroupHost*> hosts;
    for (GroupHost& h : host_objs) hosts.push_back(&h);
    std::vector<hip_bridge::SeedBatchStats> st(who.size());
    svo_hip_df_params prm{3, 10, 1000, options_.seed_convergence_sigma2_thresh};
    hip_bridge::updateCameraRig(who.size(), mirrors.data(), hosts.data(), ctx_, lists.data(), frs.data(), prm, counters.data(), options_.max_n_kfs,
                                halt_, st.data(), sub_batch_);
    bool failed = false;
    for (size_t k = 0; k < who.size(); ++k) { last_stats_[who[k]] = st[k]; failed = failed || st[k].n_device_errors != 0; }
    if (failed) throw std::runtime_error(std::string("depth_filter_group_update: ") + svo_hip_last_error(ctx_));
  }

  /// camera c's seeds with the device state copied in (DepthFilter::getSeeds)
  std::list<Seed>& getSeeds(size_t c) {
    Camera& cam = *cams_.at(c);
    if (!cam.mirror.syncToHost()) throw std::runtime_error(std::string("seed_batch_download: ") + svo_hip_last_error(ctx_));
    return cam.seeds;
  }
  int keyframeUploads() const { return kf_pyr_->uploads(); }

 private:
  typedef hip_bridge::DeviceSeedMirror<std::list<Seed> > Mirror;
  struct Camera {
    callback_t cb;
    DetectorGrid* detector = nullptr;
    std::list<Seed> seeds;
    Mirror mirror;
    int batch_counter = 0;
  };
  /// Host policy of hip_bridge::DeviceSeedMirror for one camera of the group: the caches are the group's
  struct GroupHost {
    DepthFilterGroup* g;
    Camera* cam;
    Frame* keyframeOf(const Seed& s) const { return s.ftr->frame; }
    void feature(const Seed& s, double px[2], double f[3], int* level) const {
      px[0] = s.ftr->px[0]; px[1] = s.ftr->px[1];
      for (int k = 0; k < 3; ++k) f[k] = s.ftr->f[k];
      *level = s.ftr->level;
    }
    void pose7(const Frame& fr, double T[7]) const { std::memcpy(T, fr.T_f_w_.p, sizeof(double) * 7); }
    bool keyframeSlots(const std::vector<Frame*>& kfs, std::vector<int>& slots) {
      std::vector<const Frame*> c(kfs.begin(), kfs.end());
      return g->kf_pyr_->acquire(c, slots);
    }
    int currentSlot(Frame& fr) { return g->cur_pyr_->slotOf(fr); }
    svo_hip_pyramid* keyframePyramids() const { return g->kf_pyr_->pyramid(); }
    svo_hip_pyramid* currentPyramids() const { return g->cur_pyr_->pyramid(); }
    svo_hip_camera camera(const Frame& fr) const { return fr.cam_->toC(); }
    bool isKeyframe(const Frame& fr) const { return fr.isKeyframe(); }
    void setGridOccupancy(const double px_cur[2]) { if (cam->detector) cam->detector->setGridOccpuancy(Vector2d{{px_cur[0], px_cur[1]}}); }
    void converged(Seed& s, const double xyz[3]) {
      Point* point = new Point(Vector3d{{xyz[0], xyz[1], xyz[2]}}, s.ftr);
      s.ftr->point = point;
      cam->cb(point, s.sigma2);
    }
  };

  std::vector<std::unique_ptr<Camera> > cams_;
  volatile bool halt_ = false;
  svo_hip_ctx* ctx_ = nullptr;
  std::unique_ptr<hip_bridge::PyramidCache> kf_pyr_, cur_pyr_;
};

/// svo::initialization::KltHomographyInit's KLT half (I/initialization.h:30-57, S/initialization.cpp:32-75,180-226) over
/// hip_bridge::KltInitT: addFirstFrame / addFirstFrameDetected, trackSecondFrame(s) with the reference's gates, and the lists
/// px_ref_, px_cur_, f_ref_, f_cur_, disparities_ as trackKlt leaves them, for one camera or for all cameras of a group in
/// one device call.  computeFundamental and what follows (:79-140) stay the caller's.
namespace initialization {
struct Point2f { float x, y; Point2f() : x(0.f), y(0.f) {} Point2f(float a, float b) : x(a), y(b) {} };     // cv::Point2f
struct KltTypes { typedef initialization::Point2f Point2f; typedef svo::Vector3d Vector3d; };
typedef hip_bridge::KltInitResult InitResult;

/// KltHomographyInit on the twin types: the bridge's lists and device calls, and addSecondFrame's second half (:77-138).
class KltInit : public hip_bridge::KltInitT<KltTypes> {
 public:
  typedef hip_bridge::KltInitT<KltTypes> Base;
  KltInit(svo_hip_ctx* ctx, int width, int height, int n_cameras, int max_features, const hip_bridge::KltInitGates& gates = hip_bridge::KltInitGates())
      : Base(ctx, width, height, n_cameras, max_features, gates) {}

  /// :117-138 for one camera: for every feature of the point list, in its order, a Point at `pos` with its Feature in the
  /// current frame (added first) and in the reference frame (added second: Point::obs_ reads [ref, cur]), level 0.  Returns
  /// the number of points created.
  static size_t createFirstPoints(const Lists& l, const TwoView& tv, Frame* frame_ref, Frame* frame_cur) {
    for (size_t k = 0; k < tv.point_index_.size(); ++k) {
      const size_t i = (size_t)tv.point_index_[k];
      Point* new_point = new Point(tv.point_pos_[k]);                                                   // :125-126
      Feature* ftr_cur = new Feature(frame_cur, Vector2d{{(double)l.px_cur_[i].x, (double)l.px_cur_[i].y}}, l.f_cur_[i], 0);   // :121, :129
      ftr_cur->point = new_point;
      frame_cur->addFeature(ftr_cur);
      new_point->addFrameRef(ftr_cur);
      Feature* ftr_ref = new Feature(frame_ref, Vector2d{{(double)l.px_ref_[i].x, (double)l.px_ref_[i].y}}, l.f_ref_[i], 0);   // :122, :134
      ftr_ref->point = new_point;
      frame_ref->addFeature(ftr_ref);
      new_point->addFrameRef(ftr_ref);
    }
    return tv.point_index_.size();
  }

  /// addSecondFrame from :77 on, for a camera whose lists the last trackSecondFrames (or setLists) left: computeFundamental, the
  /// gates, scale and pose on the device (computeTwoView with the reference frame's camera and pose), then frame_cur->T_f_w_
  /// (:108-115) and the first points (:117-138).  FAILURE (:89, :307, or a refused call) changes neither frame.
  InitResult addSecondFrame(int camera, Frame* frame_ref, Frame* frame_cur, const svo_hip_two_view_params* params = nullptr) {
    const InitResult r = computeTwoView(camera, frame_ref->cam_->toC(), frame_ref->T_f_w_.p, params);
    if (r != hip_bridge::KLT_SUCCESS) return hip_bridge::KLT_FAILURE;
    frame_cur->T_f_w_ = SE3(twoView(camera).T_cur_w_);
    createFirstPoints(lists(camera), twoView(camera), frame_ref, frame_cur);
    return hip_bridge::KLT_SUCCESS;
  }
};

/// svo::Map as the index tables of svo_hip_tracker_map, in the order FrameTrackerT::uploadMap walks it (keyframes_, fts_,
/// Point::obs_, candidates_); kf_slot is the keyframe's position.  What a freshly bootstrapped map looks like to the tracker.
struct MapTables {
  std::vector<int32_t> kf_slot, kf_key_point, kf_ftr_offset, kf_ftr_point, pt_type, pt_n_failed, pt_n_succeeded, pt_obs_offset, obs_kf, obs_level,
      cand_point;
  std::vector<double> T_kf_w, pt_pos, obs_px, obs_f, obs_grad;
  std::vector<uint8_t> obs_edgelet;
};
inline MapTables flattenMap(Map& map) {
  MapTables t;
  std::map<const Point*, int> index_of_point;
  std::vector<const Point*> points;
  std::map<int, int> index_of_frame;
  auto point_index = [&](const Point* p) {
    auto it = index_of_point.find(p);
    if (it != index_of_point.end()) return it->second;
    const int i = (int)points.size();
    points.push_back(p); index_of_point[p] = i;
    return i;
  };
  t.kf_ftr_offset.push_back(0); t.pt_obs_offset.push_back(0);
  int k = 0;
  for (const FramePtr& kf : map.keyframes_) {
    index_of_frame[kf->id_] = k;
    t.kf_slot.push_back(k++);
    t.T_kf_w.insert(t.T_kf_w.end(), kf->T_f_w_.p, kf->T_f_w_.p + 7);
    for (const Feature* ftr : kf->fts_) if (ftr->point != nullptr) t.kf_ftr_point.push_back(point_index(ftr->point));
    t.kf_ftr_offset.push_back((int32_t)t.kf_ftr_point.size());
    for (size_t j = 0; j < 5; ++j) {
      const Feature* kp = j < kf->key_pts_.size() ? kf->key_pts_[j] : nullptr;
      t.kf_key_point.push_back(kp && kp->point ? point_index(kp->point) : -1);
    }
  }
  for (auto& c : map.point_candidates_.candidates_) t.cand_point.push_back(point_index(c.first));
  for (size_t p = 0; p < points.size(); ++p) {
    const Point* pt = points[p];
    for (int j = 0; j < 3; ++j) t.pt_pos.push_back(pt->pos_[j]);
    t.pt_type.push_back((int)pt->type_); t.pt_n_failed.push_back(pt->n_failed_reproj_); t.pt_n_succeeded.push_back(pt->n_succeeded_reproj_);
    for (const Feature* o : pt->obs_) {
      auto fi = index_of_frame.find(o->frame->id_);
      if (fi == index_of_frame.end()) continue;
      t.obs_kf.push_back(fi->second);
      t.obs_px.push_back(o->px[0]); t.obs_px.push_back(o->px[1]);
      for (int j = 0; j < 3; ++j) t.obs_f.push_back(o->f[j]);
      t.obs_level.push_back(o->level);
      t.obs_edgelet.push_back(o->type == Feature::EDGELET ? 1 : 0);
      t.obs_grad.push_back(o->grad[0]); t.obs_grad.push_back(o->grad[1]);
    }
    t.pt_obs_offset.push_back((int32_t)t.obs_kf.size());
  }
  return t;
}
}  // namespace initialization

}  // namespace svo

#endif  // SVO_HOST_H_
