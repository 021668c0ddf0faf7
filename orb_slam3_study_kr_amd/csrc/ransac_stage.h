// ransac_stage.h -- what the minimal-set RANSAC entries share beside orb_stage.h: osh_orb_two_view_reconstruct (two_view_device.hip,
// sets of 8), osh_orb_mlpnp_solve (mlpnp_device.hip, sets of 6) and osh_orb_sim3_ransac (sim3_ransac_device.hip, sets of 3) with their
// two check_inliers entries.  Each takes a batch of problems (n correspondences and n_iterations minimal sets drawn by the caller),
// lays their arrays one after another, scores every hypothesis over all correspondences of its problem and, for MLPnP and Sim3,
// keeps one inlier mask per hypothesis.  Here: the layout of a mask and the camera projection of CheckInliers, which the statement
// headers mlpnp.h and sim3_ransac.h use; validate_minimal_sets and RansacBatch, the host side of an entry before its upload;
// wave_score and wave_compact, the two ballot loops of the kernels.
// The statements of a hypothesis, the problem structs, views, kernels, outputs and whatever a validator checks beyond the sets stay
// with their solver.  Apart from the device helpers this is plain C++ that needs no HIP header (`make ransac-stage-check`).
#pragma once
#include "kb8_triangulate.h"
#include "../../include/orbslam3_hip.h"
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace osh {

void set_error(const char* fmt, ...);   // common.cpp

// ---------------------------------------------------------------------------------------------------- masks and cameras
// Words of one inlier mask over n correspondences: bit i % 32 of word i / 32 is correspondence i, two words per 64 (one ballot)
constexpr int ransac_mask_words(int n) { return 2 * ((n + 63) / 64); }
static_assert(OSH_MLPNP_MASK_WORDS(0) == ransac_mask_words(0) && OSH_MLPNP_MASK_WORDS(64) == ransac_mask_words(64) &&
              OSH_MLPNP_MASK_WORDS(65) == ransac_mask_words(65) && OSH_SIM3R_MASK_WORDS(0) == ransac_mask_words(0) &&
              OSH_SIM3R_MASK_WORDS(64) == ransac_mask_words(64) && OSH_SIM3R_MASK_WORDS(65) == ransac_mask_words(65),
              "OSH_MLPNP_MASK_WORDS and OSH_SIM3R_MASK_WORDS are the layout of ransac_mask_words");

enum { kRansacPinhole = 0, kRansacKb8 = 1 };   // camera: fx fy cx cy, and k1 k2 k3 k4 for KannalaBrandt8
static_assert(OSH_MLPNP_PINHOLE == kRansacPinhole && OSH_MLPNP_KB8 == kRansacKb8 && OSH_SIM3R_PINHOLE == kRansacPinhole &&
              OSH_SIM3R_KB8 == kRansacKb8, "the camera types of osh_mlpnp_problem and osh_sim3r_problem");

// GeometricCamera::project of a float point v in the camera: Pinhole fx * x / z + cx, KannalaBrandt8 kb8_project.  By value: the
// pixel aliases neither cam nor v
struct Pixel { float u, v; };
OSH_KB8_HD Pixel ransac_project(int camera_type, const float* cam, const float v[3]) {
#pragma clang fp contract(off)
  float uv[2];
  if (camera_type == kRansacKb8) kb8_project(cam, v, uv);
  else { uv[0] = cam[0] * v[0] / v[2] + cam[2]; uv[1] = cam[1] * v[1] / v[2] + cam[3]; }
  return {uv[0], uv[1]};
}

// A result array the caller may leave out
template <class T>
inline void copy_if(T* dst, const T* src, size_t n) { if (dst && n) std::memcpy(dst, src, n * sizeof(T)); }

// ---------------------------------------------------------------------------------------------------- the host side of an entry
// The minimal sets of problem k: n_iterations sets of K distinct indices into its n correspondences (`what` the entry calls them);
// K is a template argument so that the pair loop is unrolled (a batch of two-view problems has 12800 sets to check)
template <int K>
int validate_minimal_sets(const char* entry, int k, const int32_t* sets, int n_iterations, int n, const char* what = "correspondences") {
  if (n_iterations && !sets) { set_error("%s: problem %d: NULL sets with n_iterations = %d", entry, k, n_iterations); return OSH_ERR_INVALID; }
  if (n_iterations && n < K) { set_error("%s: problem %d: %d %s cannot fill a minimal set of %d", entry, k, n, what, K); return OSH_ERR_INVALID; }
  for (int it = 0; it < n_iterations; ++it) {
    const int32_t* s = sets + (size_t)K * it;
    for (int a = 0; a < K; ++a) {
      if (s[a] < 0 || s[a] >= n) { set_error("%s: problem %d: set %d: index %d outside [0, %d)", entry, k, it, s[a], n); return OSH_ERR_INVALID; }
      for (int b = 0; b < a; ++b)
        if (s[a] == s[b]) { set_error("%s: problem %d: set %d repeats index %d", entry, k, it, s[a]); return OSH_ERR_INVALID; }
    }
  }
  return OSH_OK;
}

// Where the problems of a call lie in the arrays of the batch, and how much the batch holds
struct RansacBatch {
  struct Base { size_t p, h, w; };   // first correspondence, first iteration, first mask word of the iterations
  std::vector<Base> base;
  size_t N = 0, I = 0, W = 0;        // correspondences, iterations, mask words of all iterations
  int max_iter = 0;
  // The next problem: n correspondences, n_iterations sets, `words` mask words per iteration (0: the entry keeps no masks)
  void add(int n, int n_iterations, int words) {
    base.push_back({N, I, W});
    N += (size_t)n; I += (size_t)n_iterations; W += (size_t)words * (size_t)n_iterations;
    max_iter = std::max(max_iter, n_iterations);
  }
  // The sets of all problems one after another at dst [I * K]
  template <int K, class Problem>
  void stage_sets(int32_t* dst, const Problem* ps) const {
    for (size_t k = 0; k < base.size(); ++k)
      if (ps[k].n_iterations) std::memcpy(dst + base[k].h * K, ps[k].sets, (size_t)ps[k].n_iterations * K * sizeof(int32_t));
  }
};

// ---------------------------------------------------------------------------------------------------- the ballot loops
#ifdef __HIPCC__
// One wavefront scores the correspondences [0, n) 64 at a time: pred(i) is the test of correspondence i, the ballot of 64 tests is
// two words of mask_row [ransac_mask_words(n)] (bits beyond n are 0).  Returns the number of correspondences that passed.
template <class Pred>
__device__ __forceinline__ int wave_score(int lane, int n, unsigned* mask_row, Pred pred) {
  int c = 0;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    bool in = false;
    if (i < n) in = pred(i);
    const unsigned long long b = __ballot(in);
    if (lane < 2) mask_row[(base >> 5) + lane] = (unsigned)(b >> (32 * lane));
    c += __popcll(b);
  }
  return c;
}
// One wavefront lists the i in [0, n) with flag_of(i) in ascending order in out (the lanes' ranks from the ballot).  flag_of is
// called by all 64 lanes together, also for i >= n, where it must answer false; it may use cross-lane steps.  Returns the count.
template <class Flag>
__device__ __forceinline__ int wave_compact(int lane, int n, Flag flag_of, int* out) {
  int c = 0;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    const bool in = flag_of(i);
    const unsigned long long b = __ballot(in);
    if (in) out[c + __popcll(b & ((1ull << lane) - 1ull))] = i;
    c += __popcll(b);
  }
  return c;
}
#endif

}  // namespace osh
