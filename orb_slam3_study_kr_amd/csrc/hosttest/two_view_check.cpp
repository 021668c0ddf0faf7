// two_view_check.cpp -- csrc/two_view.h as plain C++ under AddressSanitizer and UBSan: a program of its own (make two-view-check)
// that makes no HIP call and needs no device.  It runs the host build of TwoViewReconstruction (tv_reconstruct_host, the statements
// of two_view_device.hip) on exactly-sized arrays at the extremes of a valid call: 8 matches with 1 iteration, every match an
// outlier, coincident points, no iterations, no matches, and the largest counts osh_orb_two_view_reconstruct accepts.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../two_view.h"

namespace {

struct Rng {
  uint64_t s;
  double next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; }
};

// kind 0: a general scene, 1: every second-frame pixel random (all outliers), 2: four correspondences repeated
long run(int n, int iterations, int kind, uint64_t seed) {
  Rng rng{seed};
  const int n1 = n + 5, n2 = n + 9;   // more keypoints than matches
  std::vector<float> xy1(2 * (size_t)n1), xy2(2 * (size_t)n2), pn1(2 * (size_t)n1), pn2(2 * (size_t)n2);
  for (int i = 0; i < n2; ++i) {
    const int j = kind == 2 ? i % 4 : i;
    Rng point{seed * 977 + (uint64_t)j};
    const double X = point.next() * 6 - 3, Y = point.next() * 4 - 2, Z = 2.5 + point.next() * 6;
    if (i < n1) { xy1[2 * i] = (float)(500 * X / Z + 320); xy1[2 * i + 1] = (float)(500 * Y / Z + 240); }
    const double X2 = X + 0.6, Z2 = Z + 0.1;
    xy2[2 * i] = (float)(500 * X2 / Z2 + 320 + (kind == 0 ? rng.next() - 0.5 : 0)); xy2[2 * i + 1] = (float)(500 * Y / Z2 + 240);
    if (kind == 1) { xy2[2 * i] = (float)(rng.next() * 640); xy2[2 * i + 1] = (float)(rng.next() * 480); }
  }
  osh_two_view_problem p{};
  const float K[9] = {500, 0, 320, 0, 500, 240, 0, 0, 1};
  for (int k = 0; k < 9; ++k) p.K[k] = K[k];
  if (n1) osh::tv_normalize(xy1.data(), n1, pn1.data(), p.T1);
  if (n2) osh::tv_normalize(xy2.data(), n2, pn2.data(), p.T2);
  // heap arrays of exactly the sizes the entry names, so that one element too far is caught
  std::unique_ptr<int32_t[]> idx1(new int32_t[n]), idx2(new int32_t[n]), sets(new int32_t[8 * (size_t)iterations]);
  std::unique_ptr<float[]> pt1(new float[2 * (size_t)n]), pt2(new float[2 * (size_t)n]), q1(new float[2 * (size_t)n]), q2(new float[2 * (size_t)n]);
  for (int i = 0; i < n; ++i) {
    idx1[i] = i; idx2[i] = n - 1 - i;
    for (int k = 0; k < 2; ++k) { pt1[2 * i + k] = xy1[2 * i + k]; pt2[2 * i + k] = xy2[2 * idx2[i] + k]; q1[2 * i + k] = pn1[2 * i + k]; q2[2 * i + k] = pn2[2 * idx2[i] + k]; }
  }
  if (kind != 1)   // match i of the general and the repeated scene is a true correspondence
    for (int i = 0; i < n; ++i) for (int k = 0; k < 2; ++k) { pt2[2 * i + k] = xy2[2 * i + k]; q2[2 * i + k] = pn2[2 * i + k]; idx2[i] = i; }
  for (int it = 0; it < iterations; ++it) {
    std::vector<int> avail(n);
    for (int i = 0; i < n; ++i) avail[i] = i;
    for (int j = 0; j < 8; ++j) {
      const int r = (int)(rng.next() * avail.size());
      sets[8 * (size_t)it + j] = avail[r];
      avail[r] = avail.back(); avail.pop_back();
    }
  }
  p.sigma = 1.f; p.n_iterations = iterations; p.n_matches = n; p.n_keys1 = n1; p.n_keys2 = n2;
  p.idx1 = idx1.get(); p.idx2 = idx2.get(); p.pt1 = pt1.get(); p.pt2 = pt2.get(); p.pn1 = q1.get(); p.pn2 = q2.get(); p.sets = sets.get();
  int32_t status = -1, best[2], info[4], n_good[8];
  float T21[12], s[2], M[18], parallax[8], dR[72], dt[24];
  std::unique_ptr<uint8_t[]> inl(new uint8_t[n]), tri(new uint8_t[n]);
  std::unique_ptr<float[]> x3d(new float[3 * (size_t)n]), mn(new float[18 * (size_t)iterations]), m(new float[18 * (size_t)iterations]),
      score(new float[2 * (size_t)iterations]);
  const osh_two_view_result r{&status, T21, &s[0], &s[1], M, M + 9, &best[0], &best[1], info, inl.get(), x3d.get(), tri.get(), n_good, parallax,
                              mn.get(), m.get(), score.get(), dR, dt};
  osh::tv_reconstruct_host(p, r);
  if (status < OSH_TWOVIEW_ACCEPTED_H || status > OSH_TWOVIEW_LOW_PARALLAX) { std::printf("two_view_check: status %d\n", status); std::exit(1); }
  for (int k = 0; k < 12; ++k) if (!std::isfinite(T21[k])) { std::printf("two_view_check: T21 not finite (n %d, kind %d)\n", n, kind); std::exit(1); }
  for (int i = 0; i < 3 * n; ++i) if (!std::isfinite(x3d[i])) { std::printf("two_view_check: x3d not finite\n"); std::exit(1); }
  for (int i = 0; i < 2 * iterations; ++i) if (!std::isfinite(score[i])) { std::printf("two_view_check: score not finite\n"); std::exit(1); }
  if (kind == 0 && n >= 100 && iterations >= 100 && status != OSH_TWOVIEW_ACCEPTED_F) { std::printf("two_view_check: the general scene ended with status %d\n", status); std::exit(1); }
  return status;
}

}  // namespace

int main() {
  long seen[7] = {0};
  int runs = 0;
  for (int kind = 0; kind < 3; ++kind) {
    const int sizes[][2] = {{8, 1}, {9, 3}, {64, 200}, {300, 200}, {300, 0}, {0, 0}};
    for (const auto& sz : sizes) { ++seen[run(sz[0], sz[1], kind, 17 + kind)]; ++runs; }
  }
  ++seen[run(OSH_TWOVIEW_MAX_MATCHES, OSH_TWOVIEW_MAX_ITERATIONS, 0, 5)]; ++runs;
  std::printf("two_view_check: %d runs, statuses", runs);
  for (int k = 0; k < 7; ++k) std::printf(" %ld", seen[k]);
  std::printf("\n");
  return 0;
}
