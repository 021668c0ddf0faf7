// sim3_ransac_check.cpp -- csrc/sim3_ransac.h as plain C++ under AddressSanitizer and UBSan: a program of its own (make
// sim3-ransac-check) that makes no HIP call and needs no device.  It runs the host build of ComputeSim3 on three fixed minimal sets
// (a free scale, a fixed scale, and both sets equal, where the quaternion is the identity) and compares the transforms with constants
// produced by the numpy restatement (tests/sim3_ransac_numpy.py) for the same inputs, then runs the whole pipeline (s3r_solve_host,
// the statements of sim3_ransac_device.hip) on exactly-sized arrays at the extremes of a valid call: 3 correspondences with 1
// iteration, no iterations, a NaN coordinate, coincident set members, and the largest counts osh_orb_sim3_ransac accepts.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../sim3_ransac.h"

namespace {

const float kA[9] = {0.f, 0.f, 4.f, 1.5f, 0.f, 4.5f, 0.25f, 1.25f, 5.f};
const float kB[9] = {0.5f, -0.25f, 5.f, 1.75f, 0.5f, 5.25f, 0.f, 1.f, 6.f};
const float kC[9] = {-1.f, 0.5f, 3.f, 0.75f, -0.5f, 3.5f, 0.25f, 1.5f, 4.25f};

int check_sim3(const char* name, const float* P1, const float* P2, bool fix_scale, const float want[13]) {
  float T[13];
  osh::s3r_compute_sim3(P1, P2, fix_scale, T);
  double worst = 0;
  for (int k = 0; k < 13; ++k) worst = std::fmax(worst, std::fabs((double)T[k] - (double)want[k]));
  std::printf("ComputeSim3, %s: s = %.9g, largest difference from numpy %.3e\n", name, (double)T[12], worst);
  // the host build equals numpy in every float32 bit on the test cases; 4 units in the last place of entries up to 2 in size
  if (!(worst <= 4 * 2 * 1.1920929e-7)) { std::printf("  FAILED\n"); return 1; }
  return 0;
}

struct Rng {
  uint64_t s;
  double next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; }
};

// X1 = s R X2 + t of the fixed scenes: the transform of check A
const float kT[13] = {0.833028555f, 0.537696064f, -0.130178109f, -0.541547298f, 0.84064275f, 0.00680554332f, 0.113092601f,
                      0.0648283958f, 0.991467297f, 0.443159342f, 0.435231596f, -0.848503113f, 0.975598514f};

// the whole pipeline on heap arrays of exactly the sizes the entry names, so that one element too far is caught
long run(int n, int iterations, bool with_nan, bool coincident, bool fix_scale, uint64_t seed) {
  Rng rng{seed};
  const size_t sn = (size_t)n, ni = (size_t)iterations, words = (size_t)OSH_SIM3R_MASK_WORDS(n);
  std::unique_ptr<float[]> x1(new float[3 * sn]), x2(new float[3 * sn]), p1(new float[2 * sn]), p2(new float[2 * sn]), e1(new float[sn]), e2(new float[sn]);
  std::unique_ptr<int32_t[]> sets(new int32_t[3 * ni]);
  const float cam1[4] = {458.f, 457.f, 367.f, 248.f}, cam2[8] = {191.f, 191.f, 255.f, 257.f, 0.0035f, 0.0007f, -0.002f, 0.0002f};
  for (int i = 0; i < n; ++i) {
    float* a = &x2[3 * (size_t)i];
    a[0] = (float)(rng.next() * 3 - 1.5); a[1] = (float)(rng.next() * 2 - 1); a[2] = (float)(rng.next() * 4 + 3);
    const bool outlier = i % 3 == 2;
    for (int r = 0; r < 3; ++r)
      x1[3 * (size_t)i + r] = kT[12] * (kT[3 * r] * a[0] + kT[3 * r + 1] * a[1] + kT[3 * r + 2] * a[2]) + kT[9 + r] + (outlier ? 0.5f : 0.f) * (float)rng.next();
    const float* b = &x1[3 * (size_t)i];
    p1[2 * i] = cam1[0] * b[0] / b[2] + cam1[2]; p1[2 * i + 1] = cam1[1] * b[1] / b[2] + cam1[3];
    float uv[2];
    osh::kb8_project(cam2, a, uv);
    p2[2 * i] = uv[0]; p2[2 * i + 1] = uv[1];
    e1[i] = 9.f; e2[i] = 13.f;
  }
  if (with_nan && n) x2[1] = std::nanf("");
  if (coincident && n > 1) for (int k = 0; k < 3; ++k) { x1[3 + k] = x1[k]; x2[3 + k] = x2[k]; }
  for (int it = 0; it < iterations; ++it) {   // three distinct indices; with_nan or coincident: correspondences 0 and 1 in every set
    int s[3];
    for (int j = 0; j < 3; ++j) {
      bool fresh;
      do {
        s[j] = (j < 2 && (with_nan || coincident)) ? j : (int)(rng.next() * n) % n;
        fresh = true;
        for (int k = 0; k < j; ++k) fresh = fresh && s[k] != s[j];
      } while (!fresh);
      sets[3 * (size_t)it + j] = s[j];
    }
  }
  osh_sim3r_problem P{};
  P.camera_type1 = OSH_SIM3R_PINHOLE; P.camera_type2 = OSH_SIM3R_KB8;
  for (int k = 0; k < 4; ++k) P.camera1[k] = cam1[k];
  for (int k = 0; k < 8; ++k) P.camera2[k] = cam2[k];
  P.fix_scale = fix_scale ? 1 : 0;
  P.n = n; P.x3dc1 = x1.get(); P.x3dc2 = x2.get(); P.p1im1 = p1.get(); P.p2im2 = p2.get(); P.max_error1 = e1.get(); P.max_error2 = e2.get();
  P.n_iterations = iterations; P.sets = sets.get(); P.min_inliers = 6;
  int32_t head[4] = {0, 0, 0, 0};
  std::unique_ptr<int32_t[]> record(new int32_t[ni]), rcount(new int32_t[ni]), dcount(new int32_t[ni]);
  std::unique_ptr<float[]> rT(new float[13 * ni]), dT(new float[13 * ni]);
  std::unique_ptr<uint32_t[]> rmask(new uint32_t[words * ni]);
  osh_sim3r_result r{};
  r.first_hit = &head[0]; r.n_records = &head[1]; r.best_iteration = &head[2]; r.best_count = &head[3];
  r.record = record.get(); r.record_count = rcount.get(); r.record_T = rT.get(); r.record_mask = rmask.get(); r.debug_count = dcount.get();
  r.debug_T = dT.get();
  osh::s3r_solve_host(P, r);
  long bits = 0;
  for (size_t q = 0; q < (size_t)head[1]; ++q)
    for (size_t w = 0; w < words; ++w) bits += __builtin_popcount(rmask[q * words + w]);
  std::printf("solve, %4d correspondences x %4d iterations%s%s: first_hit %d, records %d, best_count %d\n", n, iterations,
              with_nan ? ", a NaN in every set" : "", coincident ? ", two coincident members in every set" : "", head[0], head[1], head[3]);
  if (with_nan) for (size_t k = 0; k < ni; ++k) if (dcount[k] != 0) { std::printf("  FAILED: %d inliers from a NaN\n", dcount[k]); std::exit(1); }
  return (long)head[0] + head[3] + bits;
}

}  // namespace

int main() {
  const float wantA[13] = {0.833028555f, 0.537696064f, -0.130178109f, -0.541547298f, 0.84064275f, 0.00680554332f, 0.113092601f,
                           0.0648283958f, 0.991467297f, 0.443159342f, 0.435231596f, -0.848503113f, 0.975598514f};
  const float wantB[13] = {0.853185952f, 0.516461968f, 0.0730807856f, -0.512199819f, 0.856024027f, -0.069815658f, -0.0986160412f,
                           0.0221337732f, 0.994879365f, -1.04174781f, 0.756276965f, -0.845320463f, 1.f};
  const float wantC[13] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  int failed = 0;
  failed += check_sim3("a free scale", kA, kB, false, wantA);
  failed += check_sim3("a fixed scale", kC, kA, true, wantB);
  failed += check_sim3("both sets equal", kB, kB, false, wantC);
  long sum = 0;
  sum += run(3, 1, false, false, false, 1);
  sum += run(65, 3, false, false, true, 2);
  sum += run(300, 0, false, false, false, 3);
  sum += run(64, 5, true, false, false, 4);
  sum += run(64, 5, false, true, false, 5);
  sum += run(OSH_SIM3R_MAX_POINTS, 3, false, false, false, 6);
  sum += run(130, OSH_SIM3R_MAX_ITERATIONS, false, false, true, 7);
  std::printf("sim3_ransac_check: %s (%ld)\n", failed ? "FAILED" : "ok", sum);
  return failed ? 1 : 0;
}
