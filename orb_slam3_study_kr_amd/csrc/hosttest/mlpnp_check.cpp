// mlpnp_check.cpp -- csrc/mlpnp.h as plain C++ under AddressSanitizer and UBSan: a program of its own (make mlpnp-check) that makes no
// HIP call and needs no device.  It runs the host build of computePose on three fixed problems (6 and 40 correspondences of a general
// scene, 8 on the plane z = 0) and compares the poses with constants produced by the numpy restatement (tests/mlpnp_numpy.py) for
// the same inputs, then runs the whole pipeline (ml_solve_host, the statements of mlpnp_device.hip) on exactly-sized arrays at the
// extremes of a valid call: 6 correspondences with 1 iteration, no iterations, a NaN coordinate, and the largest counts
// osh_orb_mlpnp_solve accepts.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../mlpnp.h"

namespace {

// Rcw (row-major) and tcw of the fixed problems: rodrigues2rot(0.11, -0.07, 0.05), (0.15, -0.25, 5)
const double kPose[12] = {0.99630600859323559, -0.053681406179106439, -0.067027187555867243, 0.045993910548812855, 0.99271185479205937,
                          -0.11139000649850522, 0.072518255863219791, 0.10789569030291724, 0.99151380352500063, 0.14999999999999999, -0.25, 5};

// point i of a fixed problem, and its bearing vector (R p + t) / z with a small fixed perturbation of x
void fixed_scene(int n, bool planar, std::vector<double>& f, std::vector<double>& p) {
  f.resize(3 * (size_t)n); p.resize(3 * (size_t)n);
  for (int i = 0; i < n; ++i) {
    double* q = &p[3 * (size_t)i];
    q[0] = (double)((i * 37) % 23) / 23 * 3 - 1.5;
    q[1] = (double)((i * 53) % 19) / 19 * 2 - 1.0;
    q[2] = planar ? 0.0 : (double)((i * 29) % 17) / 17 * 1.6 - 0.8;
    double y[3];
    for (int r = 0; r < 3; ++r) y[r] = kPose[3 * r] * q[0] + kPose[3 * r + 1] * q[1] + kPose[3 * r + 2] * q[2] + kPose[9 + r];
    f[3 * (size_t)i] = y[0] / y[2] + 1e-4 * (double)(((i * 7) % 5) - 2); f[3 * (size_t)i + 1] = y[1] / y[2]; f[3 * (size_t)i + 2] = 1.0;
  }
}

int check_pose(int n, bool planar, const double want[12], double tolerance) {
  std::vector<double> f, p;
  fixed_scene(n, planar, f, p);
  std::vector<int> idx((size_t)n);
  for (int i = 0; i < n; ++i) idx[i] = i;
  double pose[12];
  int info[3] = {-1, -1, -1};
  osh::ml_compute_pose_host(n, idx.data(), f.data(), p.data(), pose, info);
  double worst = 0;
  for (int k = 0; k < 12; ++k) worst = std::fmax(worst, std::fabs(pose[k] - want[k]));
  std::printf("computePose, %d correspondences%s: planar %d, %d Gauss-Newton updates (end %d), largest difference from numpy %.3e\n", n,
              planar ? " on z = 0" : "", info[0], info[1], info[2], worst);
  if (info[0] != (planar ? 1 : 0) || !(worst <= tolerance)) { std::printf("  FAILED (tolerance %.1e)\n", tolerance); return 1; }
  return 0;
}

struct Rng {
  uint64_t s;
  double next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; }
};

// the whole pipeline on heap arrays of exactly the sizes the entry names, so that one element too far is caught
long run(int n, int iterations, bool with_nan, uint64_t seed) {
  Rng rng{seed};
  std::unique_ptr<double[]> bearing(new double[3 * (size_t)n + 1]), p3d(new double[3 * (size_t)n + 1]);
  std::unique_ptr<float[]> p2d(new float[2 * (size_t)n + 1]), err(new float[(size_t)n + 1]);
  std::unique_ptr<int32_t[]> sets(new int32_t[6 * (size_t)iterations + 1]);
  for (int i = 0; i < n; ++i) {
    double q[3] = {rng.next() * 3 - 1.5, rng.next() * 2 - 1, rng.next() * 1.6 - 0.8}, y[3];
    for (int k = 0; k < 3; ++k) q[k] = (double)(float)q[k];
    for (int r = 0; r < 3; ++r) y[r] = kPose[3 * r] * q[0] + kPose[3 * r + 1] * q[1] + kPose[3 * r + 2] * q[2] + kPose[9 + r];
    const bool outlier = i % 3 == 2;
    const double u = 458.0 * y[0] / y[2] + 367.0 + (outlier ? 30.0 + 20.0 * rng.next() : rng.next() - 0.5), v = 457.0 * y[1] / y[2] + 248.0;
    p2d[2 * i] = (float)u; p2d[2 * i + 1] = (float)v;
    bearing[3 * i] = (double)(float)((u - 367.0) / 458.0); bearing[3 * i + 1] = (double)(float)((v - 248.0) / 457.0); bearing[3 * i + 2] = 1.0;
    for (int k = 0; k < 3; ++k) p3d[3 * i + k] = q[k];
    err[i] = 5.991f;
  }
  if (with_nan && n) p3d[1] = std::nan("");
  for (int it = 0; it < iterations; ++it) {   // six distinct indices; with_nan: correspondence 0 in every set
    int s[6];
    for (int j = 0; j < 6; ++j) {
      bool fresh;
      do {
        s[j] = (j == 0 && with_nan) ? 0 : (int)(rng.next() * n) % n;
        fresh = true;
        for (int k = 0; k < j; ++k) fresh = fresh && s[k] != s[j];
      } while (!fresh);
      sets[6 * (size_t)it + j] = s[j];
    }
  }
  osh_mlpnp_problem P{};
  P.camera_type = OSH_MLPNP_PINHOLE;
  P.camera[0] = 458.f; P.camera[1] = 457.f; P.camera[2] = 367.f; P.camera[3] = 248.f;
  P.n = n; P.bearing = bearing.get(); P.p3d = p3d.get(); P.p2d = p2d.get(); P.max_error = err.get();
  P.n_iterations = iterations; P.sets = sets.get(); P.min_inliers = 6;
  const size_t words = (size_t)OSH_MLPNP_MASK_WORDS(n), ni = (size_t)iterations;
  int32_t head[7];
  std::unique_ptr<double[]> hit_pose(new double[12]), best_pose(new double[12]), dpose(new double[12 * ni + 1]), rpose(new double[12 * ni + 1]);
  std::unique_ptr<uint32_t[]> hit_mask(new uint32_t[words + 1]), best_mask(new uint32_t[words + 1]);
  std::unique_ptr<int32_t[]> dcount(new int32_t[ni + 1]), drec(new int32_t[ni + 1]), drcount(new int32_t[ni + 1]);
  osh_mlpnp_result r{};
  r.first_hit = &head[0]; r.hit_record = &head[1]; r.hit_count = &head[2]; r.best_iteration = &head[3]; r.best_count = &head[4];
  r.best_refine_ok = &head[5]; r.n_records = &head[6];
  r.hit_pose = hit_pose.get(); r.best_pose = best_pose.get(); r.hit_mask = hit_mask.get(); r.best_mask = best_mask.get();
  r.debug_pose = dpose.get(); r.debug_count = dcount.get(); r.debug_record = drec.get(); r.debug_record_count = drcount.get();
  r.debug_record_pose = rpose.get();
  osh::ml_solve_host(P, r);
  std::printf("solve, %4d correspondences x %4d iterations%s: first_hit %d, hit_count %d, best_count %d, records %d\n", n, iterations,
              with_nan ? ", a NaN in every set" : "", head[0], head[2], head[4], head[6]);
  return (long)head[0] + head[2];
}

}  // namespace

int main() {
  const double want6[12] = {0.99634408122292739, -0.053725119946743422, -0.0664235146521817, 0.046104604989260389, 0.99270931913303107,
                            -0.1113668402407918, 0.071922438854816598, 0.10789726221337503, 0.991557029926183, 0.14987616750957178,
                            -0.24993658055178652, 4.9994483879600464};
  const double want40[12] = {0.99629138453204846, -0.053738657605859073, -0.067198465651636785, 0.046033212650374862, 0.99271129889246079,
                             -0.11137872500764542, 0.072694019288379791, 0.10787230288616062, 0.99150347746729406, 0.15001301493906449,
                             -0.24994322602269553, 4.9992187124191263};
  const double want8[12] = {0.99608309407105411, -0.053819853495646872, -0.070156204825678428, 0.04577535641996186, 0.99269632107235684,
                            -0.11161823719282443, 0.075651083604009892, 0.10796961377681807, 0.99127164594293915, 0.31365179104390495,
                            -0.52111385469457283, 10.425085680249579};
  int failed = 0;
  // the spread between the host build and numpy measured over the test cases is 5e-15 (general) and 8e-11 (planar); 100 x that
  failed += check_pose(6, false, want6, 5e-13);
  failed += check_pose(40, false, want40, 5e-13);
  failed += check_pose(8, true, want8, 8e-9);
  long sum = 0;
  sum += run(6, 1, false, 1);
  sum += run(65, 3, false, 2);
  sum += run(300, 0, false, 3);
  sum += run(64, 5, true, 4);
  sum += run(OSH_MLPNP_MAX_POINTS, 3, false, 5);
  sum += run(130, OSH_MLPNP_MAX_ITERATIONS, false, 6);
  std::printf("mlpnp_check: %s (%ld)\n", failed ? "FAILED" : "ok", sum);
  return failed ? 1 : 0;
}
