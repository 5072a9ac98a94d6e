// The host twins of the keyframe decision -- svo::frame_utils::getSceneDepth (std::nth_element, as vk::getMedian), svo::needNewKf
// and svo::Map::getFurthestKeyframe of android_svo_amd/host/svo_host.h -- over cases read from a text file, for
// tests/test_keyframe_decision_model.py: the numpy models of tests/keyframe_decision_reference.py have to give exactly what this
// program prints.  Plain host code, no device.
//
// input, one case after another (doubles as C99 hex floats or "nan"):
//   case <name without blanks>
//   T <7 doubles>                     the frame's T_f_w
//   points <P> <3 P doubles>
//   features <F> <F point indices, -1: none>
//   keyframes <K> <7 K doubles>       T_kf_w rows
//   overlap <M> <M keyframe indices>
//   decide <depth_mean> <min_dist>    what needNewKf is asked with
// output, one line per case: name ok n_features_with_point bits(depth_mean) bits(depth_min) need blocking furthest bits(distance)
// With a repetition count as second argument the decision of every case is also timed (tools/finish_frame_probe.py): the line
// gains the median microseconds of one getSceneDepth + needNewKf + getFurthestKeyframe.
#include <algorithm>
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "svo_hip.h"
#include "../../android_svo_amd/host/svo_host.h"

using namespace svo;

static double number(std::istream& in) {
  std::string tok;
  in >> tok;
  return std::strtod(tok.c_str(), nullptr);
}
static unsigned long long bits(double v) {
  unsigned long long u;
  std::memcpy(&u, &v, sizeof(u));
  return u;
}

int main(int argc, char** argv) {
  if (argc != 2 && argc != 3) { std::fprintf(stderr, "usage: %s cases.txt [repetitions]\n", argv[0]); return 2; }
  const int reps = argc == 3 ? std::atoi(argv[2]) : 0;
  std::ifstream in(argv[1]);
  const PinholeCamera cam{64, 48, 60.0, 60.0, 32.0, 24.0};
  std::string word, name;
  while (in >> word) {
    if (word != "case") { std::fprintf(stderr, "expected 'case', got '%s'\n", word.c_str()); return 2; }
    in >> name;
    double T[7];
    in >> word;
    for (double& v : T) v = number(in);
    Frame frame(&cam, std::vector<std::vector<uint8_t>>());
    frame.T_f_w_ = SE3(T);
    size_t P = 0, F = 0, K = 0, M = 0;
    in >> word >> P;
    std::vector<std::unique_ptr<Point>> points;
    for (size_t p = 0; p < P; ++p) {
      Vector3d x;
      for (int i = 0; i < 3; ++i) x[i] = number(in);
      points.emplace_back(new Point(x));
    }
    in >> word >> F;
    size_t with_point = 0;
    for (size_t i = 0; i < F; ++i) {
      long p = -1;
      in >> p;
      Feature* ftr = new Feature(&frame, Vector2d{{0.0, 0.0}}, Vector3d{{0.0, 0.0, 1.0}}, 0);
      if (p >= 0) { ftr->point = points[(size_t)p].get(); ++with_point; }
      frame.addFeature(ftr);
    }
    in >> word >> K;
    Map map;
    std::vector<FramePtr> kfs;
    for (size_t k = 0; k < K; ++k) {
      double Tk[7];
      for (double& v : Tk) v = number(in);
      kfs.push_back(std::make_shared<Frame>(&cam, std::vector<std::vector<uint8_t>>()));
      kfs.back()->T_f_w_ = SE3(Tk);
      map.addKeyframe(kfs.back());
    }
    in >> word >> M;
    std::vector<std::pair<FramePtr, size_t>> overlap;
    for (size_t i = 0; i < M; ++i) {
      size_t k = 0;
      in >> k;
      overlap.push_back(std::make_pair(kfs[k], (size_t)1));
    }
    in >> word;
    const double ask_depth = number(in), min_dist = number(in);
    if (!in) { std::fprintf(stderr, "case %s is incomplete\n", name.c_str()); return 2; }

    double depth_mean = 0.0, depth_min = 0.0;
    const bool ok = frame_utils::getSceneDepth(frame, depth_mean, depth_min);
    FramePtr blocking;
    const bool need = needNewKf(frame, overlap, ask_depth, min_dist, &blocking);
    const FramePtr furthest = map.getFurthestKeyframe(frame.pos());
    long blocking_k = -1, furthest_k = -1;
    for (size_t k = 0; k < K; ++k) {
      if (blocking_k < 0 && kfs[k] == blocking) blocking_k = (long)k;       // (the first: a list may name a keyframe twice)
      if (kfs[k] == furthest) furthest_k = (long)k;
    }
    double distance = 0.0;
    if (furthest) {
      const Vector3d c = furthest->pos(), o = frame.pos();
      const double d[3] = {c[0] - o[0], c[1] - o[1], c[2] - o[2]};
      distance = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    }
    std::printf("%s %d %zu %016llx %016llx %d %ld %ld %016llx", name.c_str(), ok ? 1 : 0, with_point, bits(ok ? depth_mean : 0.0), bits(depth_min),
                need ? 1 : 0, blocking_k, furthest_k, bits(distance));
    if (reps > 0) {
      std::vector<double> us;
      volatile double sink = 0.0;
      for (int r = 0; r < reps; ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        double mean = 0.0, dmin = 0.0;
        const bool have = frame_utils::getSceneDepth(frame, mean, dmin);
        const bool nk = needNewKf(frame, overlap, have ? mean : ask_depth, min_dist);
        const FramePtr far = map.getFurthestKeyframe(frame.pos());
        us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
        sink = sink + mean + dmin + (nk ? 1.0 : 0.0) + (far ? 1.0 : 0.0);
      }
      std::sort(us.begin(), us.end());
      std::printf(" %.3f", us[us.size() / 2]);
    }
    std::printf("\n");
  }
  return 0;
}
