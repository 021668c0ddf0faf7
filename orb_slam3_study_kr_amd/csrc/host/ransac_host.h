// ransac_host.h -- what the drop-in RANSAC classes share (TwoViewReconstruction.cc, MLPnPsolver.cc, Sim3Solver.cc): the reference's
// minimal-set draw, the conversion of an entry's inlier mask, and the batched call of an entry for many solvers.  Which solvers fit
// the device, what a refusal means for a solver and every message on stderr stay with the class.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "orbslam3_hip.h"

namespace ORB_SLAM3 {

osh_orb_ctx* HostMatcherContext();   // csrc/host/ORBmatcher.cc

// DUtils::Random::RandomInt (Thirdparty/DBoW2/DUtils/Random.cpp:44-50) on the process-wide rand() stream
inline int RandomInt(int min, int max) {
  int d = max - min + 1;
  return int(((double)rand() / ((double)RAND_MAX + 1.0)) * d) + min;
}

// One minimal set as the reference's loops draw it, appended to out: a fresh copy of all indices, K times a RandomInt over what is
// left and the swap-with-back removal.  The copy is kept between calls, so a draw allocates nothing.
inline void DrawMinimalSet(const std::vector<size_t>& all, int K, std::vector<int32_t>& out) {
  static thread_local std::vector<size_t> vAvailableIndices;
  vAvailableIndices = all;
  for (int i = 0; i < K; ++i) {
    int randi = RandomInt(0, vAvailableIndices.size() - 1);
    out.push_back((int32_t)vAvailableIndices[randi]);
    vAvailableIndices[randi] = vAvailableIndices.back();
    vAvailableIndices.pop_back();
  }
}

// The flags of the n correspondences from the mask words of an entry (bit i % 32 of word i / 32)
inline void MaskToFlags(const uint32_t* mask, int n, std::vector<bool>& flags) {
  flags.assign(n, false);
  for (int i = 0; i < n; ++i) flags[i] = (mask[i >> 5] >> (i & 31)) & 1u;
}

// The problems of the solvers listed in `device` (indices into problems / results) through `entry`, max_problems of them per call.
// Returns, per solver, the return code of its call (OSH_OK: the device filled its result); OSH_ERR_UNSUPPORTED for a solver that is
// not listed and for all without a context.  on_failure(rc) is called right after a failed call, while osh_last_error() is its message.
template <class Problem, class Result, class Entry, class OnFailure>
std::vector<int> RunOnDevice(osh_orb_ctx* ctx, Entry entry, size_t max_problems, const std::vector<Problem>& problems,
                             const std::vector<Result>& results, const std::vector<size_t>& device, OnFailure on_failure) {
  std::vector<int> rc(problems.size(), OSH_ERR_UNSUPPORTED);
  for (size_t b = 0; ctx && b < device.size(); b += max_problems) {
    const size_t n = std::min(device.size() - b, max_problems);
    std::vector<Problem> ps(n);
    std::vector<Result> rs(n);
    for (size_t i = 0; i < n; ++i) { ps[i] = problems[device[b + i]]; rs[i] = results[device[b + i]]; }
    const int r = entry(ctx, (int32_t)n, ps.data(), rs.data());
    for (size_t i = 0; i < n; ++i) rc[device[b + i]] = r;
    if (r != OSH_OK) on_failure(r);
  }
  return rc;
}

}  // namespace ORB_SLAM3
