// Sim3Solver.cc -- drop-in for src/Sim3Solver.cc: the constructor (:35-121) and SetRansacParameters (:123-147) as the reference's,
// iterate (:149-294) and find (:296-300) as ONE osh_orb_sim3_ransac call (csrc/sim3_ransac_device.hip) per SetRansacParameters: on
// its first call after a reset iterate draws the minimal sets of all remaining iterations, the device runs ComputeSim3 and
// CheckInliers for all of them and lists the records, and that call and every later one replay nIterations iterations from the kept
// answer as :167-210 / :240-288 would have run them.  The caller's while(!bConverge && !bNoMore) iterate(20, ..) stays as it is.
//
// Kept from the reference:
//   * the constructor statement by statement: null, bad and index < 0 entries are skipped; pKFm is taken from vpKeyFrameMatchedMP
//     only when that vector was passed EMPTY and filled with pKF2 (the flag bDifferentKFs is named the wrong way round, :40-45, :84);
//     mvX3Dc2 uses pKF2's pose even for a point matched in another keyframe, sigmaSquare2 and kp2 come from pKFm;
//   * mvnMaxError1/2 are std::vector<size_t> (include/Sim3Solver.h:78-79): 9.210 * sigma2 is truncated towards zero and compared as
//     (float)(size_t);
//   * SetRansacParameters keeps pow(epsilon, 3), max(1, min(nIterations, mRansacMaxIts)) and the reset of mnIterations, and does not
//     reset mnBestInliers;
//   * DUtils::Random::RandomInt (Thirdparty/DBoW2/DUtils/Random.cpp:44-50) and the swap-with-back removal over a fresh copy of
//     mvAllIndices per iteration (:172-186); seeding is the caller's business.
// Deviations, all intended:
//   * the arithmetic defined in csrc/sim3_ransac.h;
//   * all sets are drawn before the device call, so the process-wide rand() stream is advanced further than the reference advances it
//     when a hit ends the search early;
//   * the five-argument iterate returns the identity when no iteration of the call became the best (the reference returns an
//     uninitialised matrix);
//   * N < 3 sets bNoMore and returns the identity (the reference draws from an empty vector);
//   * beyond the device limits (OSH_SIM3R_MAX_POINTS, OSH_SIM3R_MAX_ITERATIONS), without a device context or on a device error the
//     same statements run on the host (s3r_solve_host of csrc/sim3_ransac.h) after a message on stderr.
#include "Sim3Solver.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <tuple>

#include "../sim3_ransac.h"
#include "orbslam3_hip.h"
#include "ransac_host.h"

namespace ORB_SLAM3 {

Sim3Solver::Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatched12, const bool bFixScale,
                       std::vector<KeyFrame*> vpKeyFrameMatchedMP)
    : mbFixScale(bFixScale), pCamera1(pKF1->mpCamera), pCamera2(pKF2->mpCamera) {
  bool bDifferentKFs = false;
  if (vpKeyFrameMatchedMP.empty()) {
    bDifferentKFs = true;
    vpKeyFrameMatchedMP = std::vector<KeyFrame*>(vpMatched12.size(), pKF2);
  }
  mpKF1 = pKF1;
  mpKF2 = pKF2;
  mBestT12.setIdentity();
  mBestRotation.setIdentity();
  std::vector<MapPoint*> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
  mN1 = (int)vpMatched12.size();
  mvpMapPoints1.reserve(mN1);
  mvpMapPoints2.reserve(mN1);
  mvpMatches12 = vpMatched12;
  mvnIndices1.reserve(mN1);
  mvX3Dc1.reserve(3 * (size_t)mN1);
  mvX3Dc2.reserve(3 * (size_t)mN1);
  const Eigen::Matrix3f Rcw1 = pKF1->GetRotation();
  const Eigen::Vector3f tcw1 = pKF1->GetTranslation();
  const Eigen::Matrix3f Rcw2 = pKF2->GetRotation();
  const Eigen::Vector3f tcw2 = pKF2->GetTranslation();
  mvAllIndices.reserve(mN1);
  size_t idx = 0;
  KeyFrame* pKFm = pKF2;   // Default variable
  auto to_camera = [](const Eigen::Matrix3f& R, const Eigen::Vector3f& t, const Eigen::Vector3f& X, std::vector<float>& out) {
    for (int i = 0; i < 3; ++i) out.push_back(((R(i, 0) * X(0) + R(i, 1) * X(1)) + R(i, 2) * X(2)) + t(i));
  };
  for (int i1 = 0; i1 < mN1; i1++) {
    if (vpMatched12[i1]) {
      MapPoint* pMP1 = i1 < (int)vpKeyFrameMP1.size() ? vpKeyFrameMP1[i1] : nullptr;
      MapPoint* pMP2 = vpMatched12[i1];
      if (!pMP1) continue;
      if (pMP1->isBad() || pMP2->isBad()) continue;
      if (bDifferentKFs) pKFm = vpKeyFrameMatchedMP[i1];
      int indexKF1 = std::get<0>(pMP1->GetIndexInKeyFrame(pKF1));
      int indexKF2 = std::get<0>(pMP2->GetIndexInKeyFrame(pKFm));
      if (indexKF1 < 0 || indexKF2 < 0) continue;
      const cv::KeyPoint& kp1 = pKF1->mvKeysUn[indexKF1];
      const cv::KeyPoint& kp2 = pKFm->mvKeysUn[indexKF2];
      const float sigmaSquare1 = pKF1->mvLevelSigma2[kp1.octave];
      const float sigmaSquare2 = pKFm->mvLevelSigma2[kp2.octave];
      mvnMaxError1.push_back(9.210 * sigmaSquare1);
      mvnMaxError2.push_back(9.210 * sigmaSquare2);
      mvpMapPoints1.push_back(pMP1);
      mvpMapPoints2.push_back(pMP2);
      mvnIndices1.push_back(i1);
      to_camera(Rcw1, tcw1, pMP1->GetWorldPos(), mvX3Dc1);
      to_camera(Rcw2, tcw2, pMP2->GetWorldPos(), mvX3Dc2);
      mvAllIndices.push_back(idx);
      idx++;
    }
  }
  // FromCameraToImage (:477-487)
  auto to_image = [](const std::vector<float>& X, GeometricCamera* pCamera, std::vector<float>& out) {
    out.clear();
    out.reserve(X.size() / 3 * 2);
    for (size_t i = 0; i + 2 < X.size(); i += 3) {
      const Eigen::Vector2f pt2D = pCamera->project(Eigen::Vector3f(X[i], X[i + 1], X[i + 2]));
      out.push_back(pt2D[0]); out.push_back(pt2D[1]);
    }
  };
  to_image(mvX3Dc1, pCamera1, mvP1im1);
  to_image(mvX3Dc2, pCamera2, mvP2im2);
  mvMaxError1.resize(mvnMaxError1.size());
  mvMaxError2.resize(mvnMaxError2.size());
  for (size_t i = 0; i < mvnMaxError1.size(); ++i) { mvMaxError1[i] = (float)mvnMaxError1[i]; mvMaxError2[i] = (float)mvnMaxError2[i]; }
  SetRansacParameters();
}

void Sim3Solver::SetRansacParameters(double probability, int minInliers, int maxIterations) {
  mRansacProb = probability;
  mRansacMinInliers = minInliers;
  N = (int)mvpMapPoints1.size();   // number of correspondences
  // Set RANSAC iterations according to probability, epsilon, and max iterations
  mRansacMaxIts = osh::s3r_max_iterations(N, probability, minInliers, maxIterations);
  mnIterations = 0;
  mbAnswer = false;   // the kept answer belongs to the iterations before the reset
}

Sim3Solver::Round Sim3Solver::Prepare() {
  Round r;
  if (mbAnswer || N < mRansacMinInliers || N < 3) return r;
  r.iterations = std::max(mRansacMaxIts - mnIterations, 0);
  if (r.iterations == 0) return r;
  r.pending = true;
  r.sets.reserve(3 * (size_t)r.iterations);
  for (int it = 0; it < r.iterations; ++it) DrawMinimalSet(mvAllIndices, 3, r.sets);   // Get min set of points
  return r;
}

void Sim3Solver::Keep(const Round& round, const Answer& a) {
  mAnswer = a;
  mbAnswer = true;
  mnAnswerBase = mnIterations;
  mnAnswerIterations = round.iterations;
  mvRecordOf.assign((size_t)round.iterations, -1);
  for (int q = 0; q < a.n_records && q < (int)a.record.size(); ++q)
    if (a.record[q] >= 0 && a.record[q] < round.iterations) mvRecordOf[a.record[q]] = q;
}

Eigen::Matrix4f Sim3Solver::Replay(int nIterations, bool five, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, bool& bConverge) {
  bNoMore = false;
  bConverge = false;
  vbInliers = std::vector<bool>(mN1, false);
  nInliers = 0;
  Eigen::Matrix4f identity;
  identity.setIdentity();
  if (N < mRansacMinInliers || N < 3) {
    bNoMore = true;
    return identity;
  }
  const size_t words = (size_t)OSH_SIM3R_MASK_WORDS(N);
  Eigen::Matrix4f bestSim3 = identity;
  int nCurrentIterations = 0;
  while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations) {
    nCurrentIterations++;
    mnIterations++;
    const int i = mnIterations - 1 - mnAnswerBase;
    const int q = mbAnswer && i >= 0 && i < mnAnswerIterations ? mvRecordOf[i] : -1;
    if (q < 0) continue;   // mnInliersi < mnBestInliers
    const int mnInliersi = mAnswer.record_count[q];
    const uint32_t* mask = &mAnswer.record_mask[(size_t)q * words];
    const float* T = &mAnswer.record_T[13 * (size_t)q];
    MaskToFlags(mask, N, mvbBestInliers);
    mnBestInliers = mnInliersi;
    mBestT12.setIdentity();
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) { mBestRotation(r, c) = T[3 * r + c]; mBestT12(r, c) = T[12] * T[3 * r + c]; }
      mBestTranslation(r) = T[9 + r];
      mBestT12(r, 3) = T[9 + r];
    }
    mBestScale = T[12];
    if (mnInliersi > mRansacMinInliers) {
      nInliers = mnInliersi;
      for (int k = 0; k < N; k++)
        if (mvbBestInliers[k]) vbInliers[mvnIndices1[k]] = true;
      bConverge = true;
      return mBestT12;
    }
    bestSim3 = mBestT12;
  }
  if (mnIterations >= mRansacMaxIts) bNoMore = true;
  return five ? bestSim3 : identity;
}

namespace {
// The pending device calls of the solvers as one call (or the host build): every solver with a pending round keeps its answer
void RunPending(const std::vector<Sim3Solver*>& solvers, const std::vector<Sim3Solver::Round>& rounds) {
  const size_t S = solvers.size();
  std::vector<osh_sim3r_problem> problems(S);
  std::vector<osh_sim3r_result> results(S);
  std::vector<Sim3Solver::Answer> answers(S);
  std::vector<size_t> device;   // the solvers whose round fits the entry
  for (size_t k = 0; k < S; ++k) {
    if (!rounds[k].pending) continue;
    osh_sim3r_problem& p = problems[k];
    solvers[k]->FillProblem(p);
    p.n_iterations = rounds[k].iterations; p.sets = rounds[k].sets.data();
    Sim3Solver::Answer& a = answers[k];
    const size_t ni = (size_t)rounds[k].iterations, words = (size_t)OSH_SIM3R_MASK_WORDS(p.n);
    a.record.assign(ni, -1); a.record_count.assign(ni, 0); a.record_T.assign(ni * 13, 0.f); a.record_mask.assign(ni * words, 0u);
    osh_sim3r_result& r = results[k];
    r.n_records = &a.n_records; r.record = a.record.data(); r.record_count = a.record_count.data(); r.record_T = a.record_T.data();
    r.record_mask = a.record_mask.data();
    if (p.n <= OSH_SIM3R_MAX_POINTS && p.n_iterations <= OSH_SIM3R_MAX_ITERATIONS) device.push_back(k);
    else std::fprintf(stderr, "Sim3Solver::iterate: beyond the device limits; running on the host\n");
  }
  osh_orb_ctx* ctx = device.empty() ? nullptr : HostMatcherContext();
  if (!device.empty() && !ctx) std::fprintf(stderr, "Sim3Solver::iterate: no device context; running on the host\n");
  const std::vector<int> rc = RunOnDevice(ctx, osh_orb_sim3_ransac, OSH_SIM3R_MAX_PROBLEMS, problems, results, device, [](int) {
    std::fprintf(stderr, "Sim3Solver::iterate: %s; running on the host\n", osh_last_error());
  });
  for (size_t k = 0; k < S; ++k) {
    if (!rounds[k].pending) continue;
    solvers[k]->mbLastOnDevice = rc[k] == OSH_OK;
    if (rc[k] != OSH_OK) osh::s3r_solve_host(problems[k], results[k]);
    solvers[k]->Keep(rounds[k], answers[k]);
  }
}
}  // namespace

void Sim3Solver::FillProblem(osh_sim3r_problem& p) const {
  p.camera_type1 = pCamera1->GetType() == GeometricCamera::CAM_FISHEYE ? OSH_SIM3R_KB8 : OSH_SIM3R_PINHOLE;
  p.camera_type2 = pCamera2->GetType() == GeometricCamera::CAM_FISHEYE ? OSH_SIM3R_KB8 : OSH_SIM3R_PINHOLE;
  for (int i = 0; i < (p.camera_type1 == OSH_SIM3R_KB8 ? 8 : 4); ++i) p.camera1[i] = pCamera1->getParameter(i);
  for (int i = 0; i < (p.camera_type2 == OSH_SIM3R_KB8 ? 8 : 4); ++i) p.camera2[i] = pCamera2->getParameter(i);
  p.fix_scale = mbFixScale ? 1 : 0;
  p.n = N;
  p.x3dc1 = mvX3Dc1.data(); p.x3dc2 = mvX3Dc2.data(); p.p1im1 = mvP1im1.data(); p.p2im2 = mvP2im2.data();
  p.max_error1 = mvMaxError1.data(); p.max_error2 = mvMaxError2.data();
  p.min_inliers = mRansacMinInliers; p.best_inliers_in = mnBestInliers;
}

Eigen::Matrix4f Sim3Solver::iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
  RunPending(std::vector<Sim3Solver*>(1, this), std::vector<Round>(1, Prepare()));
  bool bConverge = false;
  return Replay(nIterations, false, bNoMore, vbInliers, nInliers, bConverge);
}

Eigen::Matrix4f Sim3Solver::iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, bool& bConverge) {
  RunPending(std::vector<Sim3Solver*>(1, this), std::vector<Round>(1, Prepare()));
  return Replay(nIterations, true, bNoMore, vbInliers, nInliers, bConverge);
}

Eigen::Matrix4f Sim3Solver::find(std::vector<bool>& vbInliers12, int& nInliers) {
  bool bFlag;
  return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
}

void Sim3Solver::IterateBatch(const std::vector<Sim3Solver*>& solvers, int nIterations, std::vector<bool>& vbNoMore,
                              std::vector<std::vector<bool> >& vvbInliers, std::vector<int>& vnInliers, std::vector<bool>& vbConverge,
                              std::vector<Eigen::Matrix4f>& vT12) {
  const size_t S = solvers.size();
  vbNoMore.assign(S, false); vvbInliers.assign(S, std::vector<bool>()); vnInliers.assign(S, 0); vbConverge.assign(S, false);
  vT12.assign(S, Eigen::Matrix4f());
  std::vector<Round> rounds(S);
  for (size_t k = 0; k < S; ++k) rounds[k] = solvers[k]->Prepare();
  RunPending(solvers, rounds);
  for (size_t k = 0; k < S; ++k) {
    bool noMore = false, converge = false;
    int n = 0;
    vT12[k] = solvers[k]->Replay(nIterations, true, noMore, vvbInliers[k], n, converge);
    vbNoMore[k] = noMore; vnInliers[k] = n; vbConverge[k] = converge;
  }
}

}  // namespace ORB_SLAM3
