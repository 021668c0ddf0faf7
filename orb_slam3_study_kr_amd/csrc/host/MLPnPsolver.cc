// MLPnPsolver.cc -- drop-in for src/MLPnPsolver.cpp: the constructor (:55-97) and SetRansacParameters (:225-260) as the reference's,
// iterate (:100-223) as ONE osh_orb_mlpnp_solve call (csrc/mlpnp_device.hip): Prepare draws the minimal sets the reference's loop
// would draw, the device runs computePose, CheckInliers and Refine for all of them, Replay walks the answer as :169-222 would.
//
// Kept from the reference:
//   * the loop condition mnIterations < mRansacMaxIts || nCurrentIterations < nIterations (:115): one call runs up to
//     max(mRansacMaxIts - mnIterations, nIterations) iterations;
//   * DUtils::Random::SeedRandOnce(0) is the caller's business as in the reference (MLPnPsolver never seeds); RandomInt
//     (Thirdparty/DBoW2/DUtils/Random.cpp:44-50) and the swap-with-back removal (:128-140);
//   * Refine of the unchanged best is a function of the best mask alone: its outcome is kept with the best and answers again when a
//     later iteration with enough inliers is no record (the reference recomputes it);
//   * Tout is the float conversion of the double pose (:338-345), vbInliers is scattered through mvKeyPointIndices (:192-197).
// Deviations, all intended:
//   * the arithmetic defined in csrc/mlpnp.h;
//   * all sets of a call are drawn before the device call.  Sets that an early return leaves unused stay queued in the solver and are
//     used first by its next call, so the solver sees the sets the reference would; the process-wide rand() stream is advanced
//     further than the reference advances it;
//   * a minimal set other than 6 is refused (bNoMore, false) after a message: the entry's kernels are written for 6;
//   * beyond the device limits (OSH_MLPNP_MAX_POINTS, OSH_MLPNP_MAX_ITERATIONS), without a device context or on a device error the
//     same statements run on the host (ml_solve_host of csrc/mlpnp.h) after a message on stderr.
#include "MLPnPsolver.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../mlpnp.h"
#include "orbslam3_hip.h"
#include "ransac_host.h"

namespace ORB_SLAM3 {

MLPnPsolver::MLPnPsolver(const Frame& F, const std::vector<MapPoint*>& vpMapPointMatches) : mpCamera(F.mpCamera) {
  mvpMapPointMatches = vpMapPointMatches;
  mvBearingVecs.reserve(F.mvpMapPoints.size());
  mvP2D.reserve(F.mvpMapPoints.size());
  mvSigma2.reserve(F.mvpMapPoints.size());
  mvP3Dw.reserve(F.mvpMapPoints.size());
  mvKeyPointIndices.reserve(F.mvpMapPoints.size());
  mvAllIndices.reserve(F.mvpMapPoints.size());
  mBestTcw.setIdentity();
  mRefinedTcw.setIdentity();
  int idx = 0;
  for (size_t i = 0, iend = mvpMapPointMatches.size(); i < iend; i++) {
    MapPoint* pMP = vpMapPointMatches[i];
    if (pMP) {
      if (!pMP->isBad()) {
        if (i >= F.mvKeysUn.size()) continue;
        const cv::KeyPoint& kp = F.mvKeysUn[i];
        mvP2D.push_back(kp.pt);
        mvSigma2.push_back(F.mvLevelSigma2[kp.octave]);
        // Bearing vector should be normalized
        cv::Point3f cv_br = mpCamera->unproject(kp.pt);
        cv_br.x /= cv_br.z; cv_br.y /= cv_br.z; cv_br.z /= cv_br.z;
        mvBearingVecs.push_back({(double)cv_br.x, (double)cv_br.y, (double)cv_br.z});
        // 3D coordinates
        Eigen::Vector3f posEig = pMP->GetWorldPos();
        mvP3Dw.push_back({(double)posEig(0), (double)posEig(1), (double)posEig(2)});
        mvKeyPointIndices.push_back(i);
        mvAllIndices.push_back(idx);
        idx++;
      }
    }
  }
  SetRansacParameters();
}

void MLPnPsolver::SetRansacParameters(double probability, int minInliers, int maxIterations, int minSet, float epsilon, float th2) {
  mRansacProb = probability;
  mRansacEpsilon = epsilon;
  mRansacMinSet = minSet;
  N = (int)mvP2D.size();   // number of correspondences
  osh::ml_ransac_parameters(N, probability, minInliers, maxIterations, minSet, epsilon, &mRansacMinInliers, &mRansacMaxIts);
  if (N > 0 && mRansacEpsilon < (float)mRansacMinInliers / N) mRansacEpsilon = (float)mRansacMinInliers / N;
  mvMaxError.resize(mvSigma2.size());
  for (size_t i = 0; i < mvSigma2.size(); i++) mvMaxError[i] = mvSigma2[i] * th2;
}

MLPnPsolver::Round MLPnPsolver::Prepare(int nIterations) {
  Round r;
  if (N < mRansacMinInliers) { r.skip = true; return r; }
  // while (mnIterations < mRansacMaxIts || nCurrentIterations < nIterations)
  r.iterations = std::max(std::max(mRansacMaxIts - mnIterations, nIterations), 0);
  r.sets.reserve(6 * (size_t)r.iterations);
  for (int it = 0; it < r.iterations; ++it) {
    if (!mvQueuedSets.empty()) {
      for (int j = 0; j < 6; ++j) r.sets.push_back(mvQueuedSets.front()[j]);
      mvQueuedSets.pop_front();
      continue;
    }
    DrawMinimalSet(mvAllIndices, 6, r.sets);   // Get min set of points
  }
  return r;
}

bool MLPnPsolver::Replay(const Round& round, const Outcome& o, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, Eigen::Matrix4f& Tout) {
  Tout.setIdentity();
  bNoMore = false;
  vbInliers.clear();
  nInliers = 0;
  if (round.skip) { bNoMore = true; return false; }
  const int consumed = o.first_hit >= 0 ? o.first_hit + 1 : round.iterations;
  mnIterations += consumed;
  for (int it = consumed; it < round.iterations; ++it) {   // the sets an early return leaves unused, in order
    std::array<int32_t, 6> s;
    for (int j = 0; j < 6; ++j) s[j] = round.sets[6 * (size_t)it + j];
    mvQueuedSets.push_back(s);
  }
  auto to_matrix = [](const double* pose, Eigen::Matrix4f& T) {
    T.setIdentity();
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) T(i, j) = (float)pose[3 * i + j]; T(i, 3) = (float)pose[9 + i]; }
  };
  if (o.best_iteration >= 0) {   // a record of this call is the running best now (:172-187)
    mnBestInliers = o.best_count;
    MaskToFlags(o.best_mask.data(), N, mvbBestInliers);
    to_matrix(o.best_pose, mBestTcw);
    mbBestRefineOk = o.best_refine_ok != 0;
    if (o.hit_record >= 0) {
      mnRefinedInliers = o.hit_count;
      MaskToFlags(o.hit_mask.data(), N, mvbRefinedInliers);
      to_matrix(o.hit_pose, mRefinedTcw);
    }
  }
  if (o.first_hit >= 0) {   // Refine() of the running best returned true (:189-200)
    nInliers = mnRefinedInliers;
    vbInliers = std::vector<bool>(mvpMapPointMatches.size(), false);
    for (int i = 0; i < N; i++)
      if (mvbRefinedInliers[i]) vbInliers[mvKeyPointIndices[i]] = true;
    Tout = mRefinedTcw;
    return true;
  }
  if (mnIterations >= mRansacMaxIts) {
    bNoMore = true;
    if (mnBestInliers >= mRansacMinInliers) {
      nInliers = mnBestInliers;
      vbInliers = std::vector<bool>(mvpMapPointMatches.size(), false);
      for (int i = 0; i < N; i++)
        if (mvbBestInliers[i]) vbInliers[mvKeyPointIndices[i]] = true;
      Tout = mBestTcw;
      return true;
    }
  }
  return false;
}

bool MLPnPsolver::iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, Eigen::Matrix4f& Tout) {
  std::vector<bool> found, noMore;
  std::vector<std::vector<bool> > inliers;
  std::vector<int> n;
  std::vector<Eigen::Matrix4f> T;
  IterateBatch(std::vector<MLPnPsolver*>(1, this), nIterations, found, noMore, inliers, n, T);
  bNoMore = noMore[0]; vbInliers = inliers[0]; nInliers = n[0]; Tout = T[0];
  return found[0];
}

void MLPnPsolver::IterateBatch(const std::vector<MLPnPsolver*>& solvers, int nIterations, std::vector<bool>& vbFound, std::vector<bool>& vbNoMore,
                               std::vector<std::vector<bool> >& vvbInliers, std::vector<int>& vnInliers, std::vector<Eigen::Matrix4f>& vTout) {
  const size_t S = solvers.size();
  vbFound.assign(S, false); vbNoMore.assign(S, false); vvbInliers.assign(S, std::vector<bool>()); vnInliers.assign(S, 0); vTout.assign(S, Eigen::Matrix4f());
  std::vector<Round> rounds(S);
  std::vector<Outcome> outcomes(S);
  std::vector<osh_mlpnp_problem> problems(S);
  std::vector<osh_mlpnp_result> results(S);
  std::vector<std::vector<float> > p2d(S);
  std::vector<bool> invalid(S, false);
  std::vector<size_t> device;   // the solvers whose round fits the entry
  for (size_t k = 0; k < S; ++k) {
    MLPnPsolver& s = *solvers[k];
    if (s.mRansacMinSet != 6) {
      std::fprintf(stderr, "MLPnPsolver::iterate: a minimal set of %d is not supported\n", s.mRansacMinSet);
      invalid[k] = true; rounds[k].skip = true;
      continue;
    }
    rounds[k] = s.Prepare(nIterations);
    if (rounds[k].skip) continue;
    osh_mlpnp_problem& p = problems[k];
    p.camera_type = s.mpCamera->GetType() == GeometricCamera::CAM_FISHEYE ? OSH_MLPNP_KB8 : OSH_MLPNP_PINHOLE;
    for (int i = 0; i < (p.camera_type == OSH_MLPNP_KB8 ? 8 : 4); ++i) p.camera[i] = s.mpCamera->getParameter(i);
    p2d[k].resize(2 * (size_t)s.N);
    for (int i = 0; i < s.N; ++i) { p2d[k][2 * i] = s.mvP2D[i].x; p2d[k][2 * i + 1] = s.mvP2D[i].y; }
    p.n = s.N; p.bearing = s.mvBearingVecs.empty() ? nullptr : s.mvBearingVecs[0].data(); p.p3d = s.mvP3Dw.empty() ? nullptr : s.mvP3Dw[0].data();
    p.p2d = p2d[k].data(); p.max_error = s.mvMaxError.data();
    p.n_iterations = rounds[k].iterations; p.sets = rounds[k].sets.data();
    p.min_inliers = s.mRansacMinInliers; p.best_inliers_in = s.mnBestInliers; p.best_refine_ok_in = s.mbBestRefineOk ? 1 : 0;
    Outcome& o = outcomes[k];
    const size_t words = (size_t)OSH_MLPNP_MASK_WORDS(s.N);
    o.hit_mask.assign(words, 0u); o.best_mask.assign(words, 0u);
    osh_mlpnp_result& r = results[k];
    r.first_hit = &o.first_hit; r.hit_record = &o.hit_record; r.hit_pose = o.hit_pose; r.hit_count = &o.hit_count; r.hit_mask = o.hit_mask.data();
    r.best_iteration = &o.best_iteration; r.best_count = &o.best_count; r.best_mask = o.best_mask.data(); r.best_pose = o.best_pose;
    r.best_refine_ok = &o.best_refine_ok;
    if (s.N <= OSH_MLPNP_MAX_POINTS && p.n_iterations <= OSH_MLPNP_MAX_ITERATIONS) device.push_back(k);
  }
  osh_orb_ctx* ctx = device.empty() ? nullptr : HostMatcherContext();
  const std::vector<int> rc = RunOnDevice(ctx, osh_orb_mlpnp_solve, OSH_MLPNP_MAX_PROBLEMS, problems, results, device, [](int r) {
    if (r == OSH_ERR_INVALID) std::fprintf(stderr, "MLPnPsolver::iterate: %s\n", osh_last_error());
    else std::fprintf(stderr, "MLPnPsolver::iterate: %s; running on the host\n", osh_last_error());
  });
  for (size_t k = 0; k < S; ++k) {
    MLPnPsolver& s = *solvers[k];
    bool noMore = false;
    int n = 0;
    s.mbLastOnDevice = !rounds[k].skip && rc[k] == OSH_OK;
    if (invalid[k] || (!rounds[k].skip && rc[k] == OSH_ERR_INVALID)) {   // refused: nothing was run, the solver gives up
      vTout[k].setIdentity(); vbNoMore[k] = true;
      continue;
    }
    if (!rounds[k].skip && rc[k] != OSH_OK) {
      if (s.N > OSH_MLPNP_MAX_POINTS || rounds[k].iterations > OSH_MLPNP_MAX_ITERATIONS)
        std::fprintf(stderr, "MLPnPsolver::iterate: beyond the device limits; running on the host\n");
      osh::ml_solve_host(problems[k], results[k]);
    }
    vbFound[k] = s.Replay(rounds[k], outcomes[k], noMore, vvbInliers[k], n, vTout[k]);
    vbNoMore[k] = noMore; vnInliers[k] = n;
  }
}

}  // namespace ORB_SLAM3
