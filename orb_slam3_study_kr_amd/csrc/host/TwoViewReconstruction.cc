// TwoViewReconstruction.cc -- drop-in for src/TwoViewReconstruction.cc: Reconstruct (:41-129) builds mvMatches12, draws mvSets as the
// reference does (:68-98), normalises both frames (Normalize, :737-784, over all keypoints) and hands FindHomography, FindFundamental,
// ReconstructH / ReconstructF and CheckRT to the device in ONE osh_orb_two_view_reconstruct call (csrc/two_view_device.hip), then
// scatters the winner's points from match order into vKeys1 order (:796-797,883,887).
//
// Kept from the reference:
//   * DUtils::Random::SeedRandOnce(0) and RandomInt (Thirdparty/DBoW2/DUtils/Random.cpp:38-50): srand(0) once per process, then
//     RandomInt on rand() and the swap-with-back removal (DrawMinimalSet of ransac_host.h).  The once-flag lives here; an integrator whose other code also calls DUtils::Random::SeedRandOnce replaces SeedRandOnce below and
//     RandomInt there by DUtils' own.
//   * ReconstructH returns true without assigning vP3D (:725-731): on the H branch vP3D is left as passed.  The C-ABI result carries
//     the points in both branches (INTEGRATION.md section 5 says how to use them).
// Deviations, all intended:
//   * the arithmetic defined in csrc/two_view.h (FP64 Jacobi singular vectors, cofactor inverses);
//   * fewer than 8 matches with iterations > 0 returns false; the reference draws from an empty vector there (:90);
//   * a non-finite K, sigma or matched keypoint, or fx, fy or sigma of 0, returns false after a message, with or without a device
//     (what osh_orb_two_view_reconstruct refuses as invalid);
//   * beyond the device limits (OSH_TWOVIEW_MAX_MATCHES, OSH_TWOVIEW_MAX_ITERATIONS), without a device context or on a device error
//     the same statements run on the host (tv_reconstruct_host of csrc/two_view.h) after a message on stderr: initialisation does
//     not depend on the device being healthy.
#include "TwoViewReconstruction.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../two_view.h"
#include "orbslam3_hip.h"
#include "ransac_host.h"

namespace ORB_SLAM3 {

namespace {
bool already_seeded = false;
void SeedRandOnce(int seed) {
  if (!already_seeded) { srand(seed); already_seeded = true; }
}
}  // namespace

TwoViewReconstruction::TwoViewReconstruction(const Eigen::Matrix3f& k, float sigma, int iterations) {
  mK = k;
  mSigma = sigma;
  mSigma2 = sigma * sigma;
  mMaxIterations = iterations;
}

bool TwoViewReconstruction::Reconstruct(const std::vector<cv::KeyPoint>& vKeys1, const std::vector<cv::KeyPoint>& vKeys2, const std::vector<int>& vMatches12,
                                        Sophus::SE3f& T21, std::vector<cv::Point3f>& vP3D, std::vector<bool>& vbTriangulated) {
  // Fill structures with current keypoints and matches with reference frame
  // Reference Frame: 1, Current Frame: 2
  mvMatches12.clear();
  mvMatches12.reserve(vKeys2.size());
  for (size_t i = 0, iend = vMatches12.size(); i < iend; i++)
    if (vMatches12[i] >= 0) mvMatches12.push_back(std::make_pair((int)i, vMatches12[i]));
  const int N = (int)mvMatches12.size();
  mnLastStatus = OSH_TWOVIEW_NO_MODEL;
  mbLastOnDevice = false;
  if (mMaxIterations > 0 && N < 8) { mvSets.clear(); return false; }

  // Generate sets of 8 points for each RANSAC iteration
  std::vector<size_t> vAllIndices;
  vAllIndices.reserve(N);
  for (int i = 0; i < N; i++) vAllIndices.push_back(i);
  std::vector<int32_t> sets;
  SeedRandOnce(0);
  for (int it = 0; it < mMaxIterations; it++) DrawMinimalSet(vAllIndices, 8, sets);   // Select a minimum set
  mvSets = std::vector<std::vector<size_t> >(mMaxIterations > 0 ? mMaxIterations : 0, std::vector<size_t>(8, 0));
  for (size_t it = 0; it < mvSets.size(); ++it) for (int j = 0; j < 8; ++j) mvSets[it][j] = sets[8 * it + j];

  // Normalize coordinates, over all keypoints of each frame
  const size_t n1 = vKeys1.size(), n2 = vKeys2.size();
  std::vector<float> xy1(2 * n1), xy2(2 * n2), vPn1(2 * n1), vPn2(2 * n2);
  for (size_t i = 0; i < n1; ++i) { xy1[2 * i] = vKeys1[i].pt.x; xy1[2 * i + 1] = vKeys1[i].pt.y; }
  for (size_t i = 0; i < n2; ++i) { xy2[2 * i] = vKeys2[i].pt.x; xy2[2 * i + 1] = vKeys2[i].pt.y; }
  osh_two_view_problem p{};
  osh::tv_normalize(xy1.data(), (int)n1, vPn1.data(), p.T1);
  osh::tv_normalize(xy2.data(), (int)n2, vPn2.data(), p.T2);
  std::vector<int32_t> idx1(N), idx2(N);
  std::vector<float> pt1(2 * (size_t)N), pt2(2 * (size_t)N), pn1(2 * (size_t)N), pn2(2 * (size_t)N);
  bool valid = true;
  for (int i = 0; i < N; ++i) {
    const int a = mvMatches12[i].first, b = mvMatches12[i].second;
    if ((size_t)b >= n2) { valid = false; break; }
    idx1[i] = a; idx2[i] = b;
    for (int k = 0; k < 2; ++k) { pt1[2 * i + k] = xy1[2 * a + k]; pt2[2 * i + k] = xy2[2 * b + k]; pn1[2 * i + k] = vPn1[2 * a + k]; pn2[2 * i + k] = vPn2[2 * b + k]; }
  }
  if (!valid) { std::fprintf(stderr, "TwoViewReconstruction::Reconstruct: a match names a keypoint outside vKeys2\n"); return false; }
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) p.K[3 * r + c] = mK(r, c);
  p.sigma = mSigma; p.n_iterations = (int32_t)mvSets.size(); p.n_matches = N; p.n_keys1 = (int32_t)n1; p.n_keys2 = (int32_t)n2;
  p.idx1 = idx1.data(); p.idx2 = idx2.data(); p.pt1 = pt1.data(); p.pt2 = pt2.data(); p.pn1 = pn1.data(); p.pn2 = pn2.data(); p.sets = sets.data();

  // what osh_orb_two_view_reconstruct refuses as OSH_ERR_INVALID is refused here too, so that the answer does not depend on
  // whether a device is there: the host build is not run on input the entry would not take
  bool finite = std::isfinite(mSigma) && mSigma != 0.f && p.K[0] != 0.f && p.K[4] != 0.f;
  for (int k = 0; k < 9; ++k) finite = finite && std::isfinite(p.K[k]) && std::isfinite(p.T1[k]) && std::isfinite(p.T2[k]);
  for (size_t i = 0; i < 2 * (size_t)N; ++i) finite = finite && std::isfinite(pt1[i]) && std::isfinite(pt2[i]) && std::isfinite(pn1[i]) && std::isfinite(pn2[i]);
  if (!finite) {
    std::fprintf(stderr, "TwoViewReconstruction::Reconstruct: K, sigma or a keypoint coordinate is not finite, or fx, fy or sigma is 0\n");
    return false;
  }

  int32_t status = OSH_TWOVIEW_NO_MODEL;
  float t21[12];
  std::vector<float> x3d(3 * (size_t)N);
  std::vector<uint8_t> tri(N);
  osh_two_view_result r{};
  r.status = &status; r.T21 = t21; r.x3d = x3d.data(); r.triangulated = tri.data();
  const bool fits = N <= OSH_TWOVIEW_MAX_MATCHES && p.n_iterations <= OSH_TWOVIEW_MAX_ITERATIONS;
  osh_orb_ctx* ctx = fits ? HostMatcherContext() : nullptr;
  int rc = OSH_ERR_UNSUPPORTED;
  if (ctx) rc = osh_orb_two_view_reconstruct(ctx, 1, &p, &r);
  if (rc == OSH_ERR_INVALID) {   // not reached with the checks above; kept so that a refusal never runs the host build
    std::fprintf(stderr, "TwoViewReconstruction::Reconstruct: %s\n", osh_last_error());
    return false;
  }
  mbLastOnDevice = rc == OSH_OK;
  if (rc != OSH_OK) {
    std::fprintf(stderr, "TwoViewReconstruction::Reconstruct: %s; running on the host\n",
                 !fits ? "beyond the device limits" : osh_last_error());
    osh::tv_reconstruct_host(p, r);
  }
  mnLastStatus = status;
  if (status != OSH_TWOVIEW_ACCEPTED_H && status != OSH_TWOVIEW_ACCEPTED_F) return false;

  Eigen::Matrix3f R;
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) R(i, j) = t21[3 * i + j];
  T21 = Sophus::SE3f(R, Eigen::Vector3f(t21[9], t21[10], t21[11]));
  // CheckRT sizes both by vKeys1 (:796-797) and writes at vMatches12[i].first (:883,887)
  vbTriangulated = std::vector<bool>(n1, false);
  for (int i = 0; i < N; ++i) if (tri[i]) vbTriangulated[idx1[i]] = true;
  if (status == OSH_TWOVIEW_ACCEPTED_F) {
    vP3D = std::vector<cv::Point3f>(n1);
    for (int i = 0; i < N; ++i) vP3D[idx1[i]] = cv::Point3f(x3d[3 * i], x3d[3 * i + 1], x3d[3 * i + 2]);
  }
  return true;
}

}  // namespace ORB_SLAM3
