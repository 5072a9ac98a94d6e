// Generator of tests/golden/two_view_ref.npz, the pin of tests/two_view_reference.py to the reference's COMPILED code
// (tools/gen_two_view_golden.py drives it; built on a machine that has the reference tree, never by the tests).  A harness of
// this project's own: it includes the reference's headers, links oracle/_ref/math_utils.o and records, for the (R, t) and the
// inputs the numpy model hands it, what the reference's own functions compute:
//   vk::computeInliers (xyz, inliers, outliers), vk::getMedian of the depths, Eigen's Quaterniond(R), and the SE3 products
//   and inverse of S/initialization.cpp:108-125 with the point positions.
//
//   gen_two_view_golden <in.bin> <out.bin>
//   in.bin:  int32 n, n_points; f64 R[9] (row-major), t[3], error_multiplier2, reproj_thresh, map_scale, T_ref_w[7];
//            f64 f_cur[n][3], f_ref[n][3]; int32 point_index[n_points]
//   out.bin: f64 xyz[n][3]; int32 n_inliers, inliers[..], n_outliers, outliers[..]; f64 median (absent when a depth is NaN:
//            nth_element has no defined answer there), quaternion[4] (x y z w), T_cur_w[7], T_world_cur[7], pos[n_points][3]
#include <cstdio>
#include <vector>

#include <svo/SE3.h>
#include <svo/math_utils.h>

static void put_se3(FILE* f, const SE3& T) {
  const double v[7] = {T.get_translation().x, T.get_translation().y, T.get_translation().z, T.get_rotation().x, T.get_rotation().y,
                       T.get_rotation().z, T.get_rotation().w};
  fwrite(v, 8, 7, f);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 1;
  int32_t hd[2];
  double s[22];
  if (fread(hd, 4, 2, f) != 2 || fread(s, 8, 22, f) != 22) return 1;
  const int n = hd[0], np = hd[1];
  std::vector<double> fc(3 * (size_t)n), fr(3 * (size_t)n);
  std::vector<int32_t> pts((size_t)np);
  if (fread(fc.data(), 8, fc.size(), f) != fc.size() || fread(fr.data(), 8, fr.size(), f) != fr.size()) return 1;
  if (np && fread(pts.data(), 4, pts.size(), f) != pts.size()) return 1;
  fclose(f);
  Eigen::Matrix3d R;
  Eigen::Vector3d t(s[9], s[10], s[11]);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R(i, j) = s[3 * i + j];
  const double em2 = s[12], thresh = s[13], map_scale = s[14];
  std::vector<Eigen::Vector3d> f_cur, f_ref, xyz;
  for (int i = 0; i < n; ++i) {
    f_cur.push_back(Eigen::Vector3d(fc[3 * i], fc[3 * i + 1], fc[3 * i + 2]));
    f_ref.push_back(Eigen::Vector3d(fr[3 * i], fr[3 * i + 1], fr[3 * i + 2]));
  }
  std::vector<int> inliers, outliers;
  vk::computeInliers(f_cur, f_ref, R, t, thresh, em2, xyz, inliers, outliers);                 // S/initialization.cpp:320
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 1;
  bool any_nan = false;
  std::vector<double> depth;
  for (int i = 0; i < n; ++i) {
    const double v[3] = {xyz[i].x(), xyz[i].y(), xyz[i].z()};
    fwrite(v, 8, 3, o);
    depth.push_back(v[2]);
    any_nan = any_nan || v[2] != v[2];
  }
  int32_t c = (int32_t)inliers.size();
  fwrite(&c, 4, 1, o);
  for (int v : inliers) { int32_t w = v; fwrite(&w, 4, 1, o); }
  c = (int32_t)outliers.size();
  fwrite(&c, 4, 1, o);
  for (int v : outliers) { int32_t w = v; fwrite(&w, 4, 1, o); }
  double median = 0.0;
  if (!any_nan) {
    median = vk::getMedian(depth);                                                              // :96
    fwrite(&median, 8, 1, o);
  }
  Eigen::Quaterniond quat(R);                                                                   // :324
  const double q[4] = {quat.x(), quat.y(), quat.z(), quat.w()};
  fwrite(q, 8, 4, o);
  if (!any_nan) {
    const SE3 T_cur_from_ref(t.x(), t.y(), t.z(), quat.x(), quat.y(), quat.z(), quat.w());     // :325
    const SE3 T_ref_w(s[15], s[16], s[17], s[18], s[19], s[20], s[21]);
    const double scale = map_scale / median;                                                    // :105
    SE3 T_cur_w = T_cur_from_ref * T_ref_w;                                                     // :108
    const Eigen::Vector3d ref_pos = T_ref_w.inverse().translation_vec(), cur_pos = T_cur_w.inverse().translation_vec();   // Frame::pos()
    Eigen::Vector3d translation = -T_cur_w.rotation_matrix() * (ref_pos + scale * (cur_pos - ref_pos));                   // :110-111
    T_cur_w.get_translation().x = translation.x();
    T_cur_w.get_translation().y = translation.y();
    T_cur_w.get_translation().z = translation.z();
    const SE3 T_world_cur = T_cur_w.inverse();                                                  // :118
    put_se3(o, T_cur_w);
    put_se3(o, T_world_cur);
    for (int k = 0; k < np; ++k) {
      const Eigen::Vector3d pos = T_world_cur * (xyz[pts[k]] * scale);                          // :125
      const double v[3] = {pos.x(), pos.y(), pos.z()};
      fwrite(v, 8, 3, o);
    }
  }
  return fclose(o) == 0 ? 0 : 1;
}
