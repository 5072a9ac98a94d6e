// klt_init_hip.h -- hip_bridge::KltInitT: the KLT half of svo::initialization::KltHomographyInit (I/initialization.h,
// S/initialization.cpp) on the device, for one camera or for every camera of a group in one call.
//
//   addFirstFrame    :32-51    detectFeatures (:154-174) or features the caller already has; the `< 100 features` gate
//   addSecondFrame   :61-75    trackKlt (:180-226) + the two gates: FAILURE below Config::initMinTracked() survivors,
//                              NO_KEYFRAME while the median disparity is below Config::initMinDisparity()
//
//   addSecondFrame   :77-125   computeTwoViews: computeFundamental (:260-329), the init_min_inliers gate, the depth median, the
//                              map scale, the second frame's pose and the positions of the first points (svo_hip_klt_two_view)
//
// trackSecondFrame returns SUCCESS where the reference goes on to computeFundamental (:79); computeTwoViews is that step, on
// the lists this class fills exactly as trackKlt leaves them -- px_ref_, px_cur_, f_ref_, f_cur_, disparities_ (erased
// features gone for good, order kept, px_cur_ carried to the next frame as its initial flow).  index_ adds each survivor's
// position in the first frame's list.  The Point and Feature objects of :126-136 stay the caller's: TwoView lists, in the
// reference's order, the feature and the position of each.
//
// Types::Point2f: a type with float members x, y (cv::Point2f); Types::Vector3d: default-constructible, operator[] on doubles
// (Eigen::Vector3d).  The image of a frame is level 0 of a slot of any svo_hip_pyramid of the context: the drop-in's
// PyramidCache, or a tracker group's frame batch (svo_hip_tracker_last_frame_pyramid).  C++11, header only.
#ifndef SVO_KLT_INIT_HIP_H_
#define SVO_KLT_INIT_HIP_H_

#include <cstddef>
#include <limits>
#include <vector>

#include "../svo_hip.h"

namespace svo {
namespace hip_bridge {

/// svo::initialization::InitResult (I/initialization.h:27), same order
enum KltInitResult { KLT_FAILURE = 0, KLT_NO_KEYFRAME = 1, KLT_SUCCESS = 2 };

struct KltInitGates {
  size_t min_features;      ///< addFirstFrame fails below this many features (:42)
  size_t min_tracked;       ///< Config::initMinTracked() (:68)
  double min_disparity;     ///< Config::initMinDisparity() (:74)
  KltInitGates() : min_features(100), min_tracked(50), min_disparity(50.0) {}
};

template <class Types>
class KltInitT {
 public:
  typedef typename Types::Point2f Point2f;
  typedef typename Types::Vector3d Vector3d;

  /// what KltHomographyInit holds between frames, per camera
  struct Lists {
    std::vector<Point2f> px_ref_, px_cur_;
    std::vector<Vector3d> f_ref_, f_cur_;
    std::vector<double> disparities_;
    std::vector<int32_t> index_;
    double disparity_median_;
    bool has_ref_;              ///< frame_ref_ is set
    Lists() : disparity_median_(std::numeric_limits<double>::quiet_NaN()), has_ref_(false) {}
  };

  /// what computeFundamental and addSecondFrame :85-125 leave, per camera, as KltHomographyInit holds it
  struct TwoView {
    int status_;                          ///< SVO_HIP_TWO_VIEW_*; -1: no attempt since the lists changed
    std::vector<int> inliers_;            ///< (:82) empty unless status_ is OK: a failure leaves no inliers
    std::vector<Vector3d> xyz_in_cur_;    ///< (:82) one per correspondence; empty before the cheirality gate is passed
    double T_cur_from_ref_[7];            ///< (:82) T_f_w[7] layout
    double T_cur_w_[7];                   ///< frame_cur->T_f_w_ with the rescaled translation (:108-115)
    double depth_median_, scale_;         ///< (:96, :105)
    std::vector<int32_t> point_index_;    ///< the features that get a point (:123), positions in the camera's lists, inlier order
    std::vector<Vector3d> point_pos_;     ///< `pos` of :125 for each
    TwoView() : status_(-1), depth_median_(std::numeric_limits<double>::quiet_NaN()), scale_(depth_median_) {
      for (int i = 0; i < 7; ++i) T_cur_from_ref_[i] = T_cur_w_[i] = depth_median_;
    }
  };

  KltInitT(svo_hip_ctx* ctx, int width, int height, int n_cameras, int max_features, const KltInitGates& gates = KltInitGates())
      : klt_(NULL), max_features_(max_features), gates_(gates), lists_(n_cameras > 0 ? n_cameras : 0), two_view_(n_cameras > 0 ? n_cameras : 0) {
    if (svo_hip_klt_create(ctx, width, height, n_cameras, max_features, NULL, &klt_) != SVO_HIP_OK) klt_ = NULL;
  }
  ~KltInitT() { if (klt_) svo_hip_klt_destroy(klt_); }
  bool ok() const { return klt_ != NULL; }
  int cameras() const { return (int)lists_.size(); }
  const Lists& lists(int camera) const { return lists_[camera]; }
  const TwoView& twoView(int camera) const { return two_view_[camera]; }
  svo_hip_klt* handle() { return klt_; }

  /// KltHomographyInit::reset (:143-147)
  void reset(int camera) { lists_[camera] = Lists(); two_view_[camera] = TwoView(); }

  /// addFirstFrame with features the caller has (the reference's detectFeatures output)
  KltInitResult addFirstFrame(int camera, const svo_hip_pyramid* pyr, int slot, const std::vector<Point2f>& px, const std::vector<Vector3d>& f) {
    if (!inRange(camera)) return KLT_FAILURE;
    reset(camera);
    if (px.size() != f.size() || px.size() < gates_.min_features || !klt_) return KLT_FAILURE;         // :42-46, nothing is sent
    std::vector<float> p(2 * px.size());
    std::vector<double> ff(3 * px.size());
    for (size_t i = 0; i < px.size(); ++i) {
      p[2 * i] = px[i].x; p[2 * i + 1] = px[i].y;
      for (int j = 0; j < 3; ++j) ff[3 * i + j] = f[i][j];
    }
    if (svo_hip_klt_set_reference(klt_, camera, pyr, slot, (int)px.size(), p.data(), ff.data()) != SVO_HIP_OK) return KLT_FAILURE;
    Lists& l = lists_[camera];
    l.px_ref_ = px; l.px_cur_ = px; l.f_ref_ = f;                                                      // :49
    l.index_.resize(px.size());
    for (size_t i = 0; i < px.size(); ++i) l.index_[i] = (int32_t)i;
    l.has_ref_ = true;
    return KLT_SUCCESS;
  }

  /// addFirstFrame as one device call: the detection runs where the image lies, the lists come back once
  KltInitResult addFirstFrameDetected(int camera, const svo_hip_pyramid* pyr, int slot, const svo_hip_camera& cam, int n_pyr_levels, int cell_size,
                                      double detection_threshold) {
    if (!inRange(camera)) return KLT_FAILURE;
    reset(camera);
    int32_t n = 0;
    if (!klt_ || svo_hip_klt_set_reference_detected(klt_, camera, pyr, slot, &cam, n_pyr_levels, cell_size, detection_threshold, &n) != SVO_HIP_OK)
      return KLT_FAILURE;
    if (!fetch(camera, false)) return KLT_FAILURE;
    Lists& l = lists_[camera];
    if (l.px_ref_.size() < gates_.min_features) { reset(camera); return KLT_FAILURE; }                  // :42-46
    l.has_ref_ = true;
    return KLT_SUCCESS;
  }

  /// addSecondFrame's KLT half for the listed cameras in one device call; results[i] for cameras[i].  A camera without a
  /// reference makes the whole call fail (nothing is sent).  false: the device refused, every list is as it was.
  bool trackSecondFrames(int n, const int* cameras, const svo_hip_pyramid* cur, const int* slots, const svo_hip_camera* cams, KltInitResult* results) {
    if (!klt_ || n <= 0) return false;
    for (int i = 0; i < n; ++i)
      if (!inRange(cameras[i]) || !lists_[cameras[i]].has_ref_) return false;
    std::vector<svo_hip_klt_result> res((size_t)n);
    if (svo_hip_klt_track(klt_, n, cameras, cur, slots, cams, res.data()) != SVO_HIP_OK) return false;
    bool all = true;
    for (int i = 0; i < n; ++i) {
      Lists& l = lists_[cameras[i]];
      two_view_[cameras[i]] = TwoView();                                                                 // the lists change
      if (!fetch(cameras[i], true)) { all = false; results[i] = KLT_FAILURE; continue; }
      l.disparity_median_ = res[i].disparity_median;
      if (l.disparities_.size() < gates_.min_tracked) results[i] = KLT_FAILURE;                         // :68-69
      else if (l.disparity_median_ < gates_.min_disparity) results[i] = KLT_NO_KEYFRAME;                // :72-75
      else results[i] = KLT_SUCCESS;                                                                    // on to computeFundamental (:79)
    }
    return all;
  }

  KltInitResult trackSecondFrame(int camera, const svo_hip_pyramid* cur, int slot, const svo_hip_camera& cam) {
    KltInitResult r = KLT_FAILURE;
    return trackSecondFrames(1, &camera, cur, &slot, &cam, &r) ? r : KLT_FAILURE;
  }

  /// The camera's lists from a matcher of the caller's own (svo_hip_klt_set_lists) in place of what trackKlt left: index_ becomes
  /// 0..n-1, the disparities are undefined (NaN) until the next track.  The camera must have a reference.  false: refused, every
  /// list as it was.
  bool setLists(int camera, const std::vector<Point2f>& px_ref, const std::vector<Point2f>& px_cur, const std::vector<Vector3d>& f_ref,
                const std::vector<Vector3d>& f_cur) {
    const size_t m = px_ref.size();
    if (!klt_ || !inRange(camera) || !lists_[camera].has_ref_ || px_cur.size() != m || f_ref.size() != m || f_cur.size() != m) return false;
    std::vector<float> pr(2 * m + 1), pc(2 * m + 1);
    std::vector<double> fr(3 * m + 1), fc(3 * m + 1);
    for (size_t i = 0; i < m; ++i) {
      pr[2 * i] = px_ref[i].x; pr[2 * i + 1] = px_ref[i].y; pc[2 * i] = px_cur[i].x; pc[2 * i + 1] = px_cur[i].y;
      for (int j = 0; j < 3; ++j) { fr[3 * i + j] = f_ref[i][j]; fc[3 * i + j] = f_cur[i][j]; }
    }
    if (svo_hip_klt_set_lists(klt_, camera, (int)m, pr.data(), pc.data(), fr.data(), fc.data()) != SVO_HIP_OK) return false;
    Lists& l = lists_[camera];
    l.px_ref_ = px_ref; l.px_cur_ = px_cur; l.f_ref_ = f_ref; l.f_cur_ = f_cur;
    l.disparities_.assign(m, std::numeric_limits<double>::quiet_NaN());
    l.disparity_median_ = std::numeric_limits<double>::quiet_NaN();
    l.index_.resize(m);
    for (size_t i = 0; i < m; ++i) l.index_[i] = (int32_t)i;
    two_view_[camera] = TwoView();
    return true;
  }

  /// The rest of addSecondFrame (:77-125) for the listed cameras in one device call, on the lists the last trackSecondFrames
  /// left: results[i] is SUCCESS where the reference reaches :140, FAILURE where it returns at :89 (or leaves computeFundamental
  /// at :307); twoView(camera) holds what the class holds then.  cams[i]: errorMultiplier2 and the image size of the gate of
  /// :123; T_ref_w: [n][7] or NULL (identity); params: NULL for the reference's Config values.  A camera without tracked lists
  /// makes the whole call fail (nothing is sent).  false: the device refused, every list and result is as it was.
  bool computeTwoViews(int n, const int* cameras, const svo_hip_camera* cams, const double* T_ref_w, const svo_hip_two_view_params* params,
                       KltInitResult* results) {
    if (!klt_ || n <= 0) return false;
    for (int i = 0; i < n; ++i)
      if (!inRange(cameras[i]) || !lists_[cameras[i]].has_ref_ || lists_[cameras[i]].f_cur_.size() != lists_[cameras[i]].px_ref_.size() ||
          lists_[cameras[i]].disparities_.size() != lists_[cameras[i]].px_ref_.size())
        return false;
    std::vector<svo_hip_two_view_result> res((size_t)n);
    if (svo_hip_klt_two_view(klt_, n, cameras, cams, T_ref_w, params, res.data()) != SVO_HIP_OK) return false;
    bool all = true;
    for (int i = 0; i < n; ++i) {
      TwoView tv;
      tv.status_ = res[i].status;
      tv.depth_median_ = res[i].depth_median; tv.scale_ = res[i].scale;
      for (int j = 0; j < 7; ++j) { tv.T_cur_from_ref_[j] = res[i].T_cur_from_ref[j]; tv.T_cur_w_[j] = res[i].T_cur_w[j]; }
      results[i] = res[i].status == SVO_HIP_TWO_VIEW_OK ? KLT_SUCCESS : KLT_FAILURE;                     // :85-89, :305-308
      const bool have_xyz = res[i].status == SVO_HIP_TWO_VIEW_OK || res[i].status == SVO_HIP_TWO_VIEW_FEW_INLIERS;
      if (have_xyz && !fetchTwoView(cameras[i], res[i], tv)) { all = false; results[i] = KLT_FAILURE; tv = TwoView(); }
      two_view_[cameras[i]] = tv;
    }
    return all;
  }

  KltInitResult computeTwoView(int camera, const svo_hip_camera& cam, const double* T_ref_w = NULL, const svo_hip_two_view_params* params = NULL) {
    KltInitResult r = KLT_FAILURE;
    return computeTwoViews(1, &camera, &cam, T_ref_w, params, &r) ? r : KLT_FAILURE;
  }

 private:
  bool inRange(int camera) const { return camera >= 0 && camera < (int)lists_.size(); }

  /// the camera's lists from the device (tracked: f_cur_ and disparities_ are defined)
  bool fetch(int camera, bool tracked) {
    const size_t cap = (size_t)max_features_;
    std::vector<float> pr(2 * cap), pc(2 * cap);
    std::vector<double> fr(3 * cap), fc(3 * cap), d(cap);
    std::vector<int32_t> idx(cap);
    int32_t n = 0;
    if (svo_hip_klt_download(klt_, camera, &n, pr.data(), pc.data(), fr.data(), tracked ? fc.data() : NULL, tracked ? d.data() : NULL, idx.data()) !=
        SVO_HIP_OK)
      return false;
    Lists& l = lists_[camera];
    const size_t m = (size_t)n;
    l.px_ref_.resize(m); l.px_cur_.resize(m); l.f_ref_.resize(m); l.index_.assign(idx.begin(), idx.begin() + m);
    l.f_cur_.clear(); l.disparities_.clear();
    if (tracked) { l.f_cur_.resize(m); l.disparities_.assign(d.begin(), d.begin() + m); }
    for (size_t i = 0; i < m; ++i) {
      l.px_ref_[i].x = pr[2 * i]; l.px_ref_[i].y = pr[2 * i + 1];
      l.px_cur_[i].x = pc[2 * i]; l.px_cur_[i].y = pc[2 * i + 1];
      for (int j = 0; j < 3; ++j) {
        l.f_ref_[i][j] = fr[3 * i + j];
        if (tracked) l.f_cur_[i][j] = fc[3 * i + j];
      }
    }
    return true;
  }

  /// xyz_in_cur_, inliers_ and the point list of a camera from the device
  bool fetchTwoView(int camera, const svo_hip_two_view_result& r, TwoView& tv) {
    const size_t m = (size_t)r.n_in, ni = (size_t)r.n_inliers, np = (size_t)r.n_points;
    std::vector<double> xyz(3 * m + 1), pos(3 * np + 1);
    std::vector<int32_t> inl(ni + 1), idx(np + 1);
    int32_t n = 0, n_inl = 0, n_pts = 0;
    if (svo_hip_klt_download_two_view(klt_, camera, NULL, &n, xyz.data(), NULL, &n_inl, inl.data(), &n_pts, idx.data(), pos.data(), NULL, NULL) != SVO_HIP_OK)
      return false;
    if ((size_t)n != m || (size_t)n_inl != ni || (size_t)n_pts != np || m != lists_[camera].px_ref_.size()) return false;
    tv.xyz_in_cur_.resize(m); tv.inliers_.assign(inl.begin(), inl.begin() + ni);
    tv.point_index_.assign(idx.begin(), idx.begin() + np); tv.point_pos_.resize(np);
    for (size_t i = 0; i < m; ++i)
      for (int j = 0; j < 3; ++j) tv.xyz_in_cur_[i][j] = xyz[3 * i + j];
    for (size_t i = 0; i < np; ++i)
      for (int j = 0; j < 3; ++j) tv.point_pos_[i][j] = pos[3 * i + j];
    return true;
  }

  KltInitT(const KltInitT&);
  KltInitT& operator=(const KltInitT&);

  svo_hip_klt* klt_;
  int max_features_;
  KltInitGates gates_;
  std::vector<Lists> lists_;
  std::vector<TwoView> two_view_;
};

}  // namespace hip_bridge
}  // namespace svo

#endif  // SVO_KLT_INIT_HIP_H_
