// camera_rig.h -- the cameras of a rig each have their own svo_hip_camera (same image size, own intrinsics and distortion).  The
// many-camera bridges (FrameTrackerGroupT, updateCameraRig) take one model per camera and use the rig entry points of
// svo_hip.h only when the models really differ: a set of equal models goes through the calls it always went through.
#ifndef SVO_DROPIN_CAMERA_RIG_H_
#define SVO_DROPIN_CAMERA_RIG_H_

#include <cstddef>

#include "svo_hip.h"

namespace svo {
namespace hip_bridge {

/// the same camera model: image size, intrinsics, distortion
inline bool sameCamera(const svo_hip_camera& a, const svo_hip_camera& b) {
  if (a.width != b.width || a.height != b.height || a.fx != b.fx || a.fy != b.fy || a.cx != b.cx || a.cy != b.cy || a.distortion != b.distortion)
    return false;
  for (int i = 0; i < 5; ++i)
    if (a.d[i] != b.d[i]) return false;
  return true;
}

/// every one of the n models equals the first
inline bool oneCameraModel(const svo_hip_camera* cams, size_t n) {
  for (size_t c = 1; c < n; ++c)
    if (!sameCamera(cams[c], cams[0])) return false;
  return true;
}

}  // namespace hip_bridge
}  // namespace svo

#endif  // SVO_DROPIN_CAMERA_RIG_H_
