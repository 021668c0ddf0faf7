// OptimizerSim3.cc -- ORB_SLAM3::Optimizer::OptimizeSim3 on MI355X: the relative Sim3 of a loop or merge candidate.
//
// Host side: the pair walk of src/Optimizer.cc:2118-2277 flattened into an osh_sim3_problem (PackOptimizeSim3, also called by
// the test library without a device), the device runs both optimisation rounds and the classifications (:2279-2378,
// csrc/sim3opt_device.hip), the host nulls the outliers' vpMatches1 entries and writes g2oS12 and mAcumHessian back (:2301, :2348-2384).
#include <cmath>
#include <cstdio>
#include <tuple>
#include <vector>

#include "Optimizer.h"
#include "host_pack.h"
#include "orbslam3_hip.h"

namespace ORB_SLAM3 {

// pMP->GetWorldPos() in the camera of pKF, in float as the reference computes it (R1w*P3D1w + t1w); the pose is applied as the
// other host walks apply a keyframe pose (SE3f * Vector3f, e.g. SearchBySim3's T1w * p3Dw)
static Eigen::Vector3f sim3_camera_point(const Sophus::SE3f& Tcw, MapPoint* pMP) { return Tcw * pMP->GetWorldPos(); }

static bool sim3_camera(GeometricCamera* cam, double* p, int32_t& kb8, const char*& unsupported) {
  for (int k = 0; k < 8; ++k) p[k] = 0.0;
  if (!cam) { unsupported = "keyframe without a camera"; return false; }
  if (cam->GetType() == GeometricCamera::CAM_PINHOLE) { kb8 = 0; for (int k = 0; k < 4; ++k) p[k] = cam->getParameter(k); return true; }
  if (cam->GetType() == GeometricCamera::CAM_FISHEYE) { kb8 = 1; for (int k = 0; k < 8; ++k) p[k] = cam->getParameter(k); return true; }
  unsupported = "unknown camera model";
  return false;
}

bool PackOptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatches1, const bool bAllPoints, Sim3OptPack& pk) {
  pk = Sim3OptPack();
  if (!sim3_camera(pKF1->mpCamera, pk.cam1, pk.kb8_1, pk.unsupported) || !sim3_camera(pKF2->mpCamera, pk.cam2, pk.kb8_2, pk.unsupported)) return false;
  const Sophus::SE3f T1w = pKF1->GetPose(), T2w = pKF2->GetPose();
  const int N = (int)vpMatches1.size();
  const std::vector<MapPoint*> vpMapPoints1 = pKF1->GetMapPointMatches();
  for (int i = 0; i < N; i++) {
    if (!vpMatches1[i]) continue;
    MapPoint* pMP1 = i < (int)vpMapPoints1.size() ? vpMapPoints1[i] : nullptr;
    MapPoint* pMP2 = vpMatches1[i];
    const int i2 = std::get<0>(pMP2->GetIndexInKeyFrame(pKF2));
    Eigen::Vector3f P3D1c, P3D2c;
    if (pMP1 && pMP2) {
      if (pMP1->isBad() || pMP2->isBad()) continue;   // :2199-2203
      P3D1c = sim3_camera_point(T1w, pMP1);
      P3D2c = sim3_camera_point(T2w, pMP2);
    } else {
      (void)pMP2->isBad();   // the reference adds pMP2's vertex only (:2205-2222): no edge
      continue;
    }
    if (i2 < 0 && !bAllPoints) continue;   // :2224-2228
    if (P3D2c(2) < 0) continue;            // :2230-2234
    // e12: x1 = S12 * X2 through pKF1's camera (:2238-2253)
    const cv::KeyPoint& kpUn1 = pKF1->mvKeysUn[i];
    pk.index.push_back(i);
    pk.X1c.push_back(P3D1c(0)); pk.X1c.push_back(P3D1c(1)); pk.X1c.push_back(P3D1c(2));
    pk.X2c.push_back(P3D2c(0)); pk.X2c.push_back(P3D2c(1)); pk.X2c.push_back(P3D2c(2));
    pk.obs1.push_back(kpUn1.pt.x); pk.obs1.push_back(kpUn1.pt.y);
    pk.info1.push_back(pKF1->mvInvLevelSigma2[kpUn1.octave]);
    // e21: x2 = S12^-1 * X1 through pKF2's camera (:2255-2292).  Without an observation in pKF2 the measurement is the normalised
    // float (x/z, y/z) of P3D2c, and the keypoint is cv::KeyPoint(Point2f(x, y), pMP2->mnTrackScaleLevel): that constructor's
    // second argument is the SIZE, so the octave -- the information's level -- is KeyPoint's default 0.
    float ox, oy;
    int octave2;
    if (i2 >= 0) {
      const cv::KeyPoint& kpUn2 = pKF2->mvKeysUn[i2];
      ox = kpUn2.pt.x; oy = kpUn2.pt.y; octave2 = kpUn2.octave;
    } else {
      const float invz = 1 / P3D2c(2);
      ox = P3D2c(0) * invz; oy = P3D2c(1) * invz; octave2 = 0;
    }
    pk.obs2.push_back(ox); pk.obs2.push_back(oy);
    pk.info2.push_back(pKF2->mvInvLevelSigma2[octave2]);
  }
  return true;
}

int Optimizer::OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12, const float th2,
                            const bool bFixScale, Eigen::Matrix<double, 7, 7>& mAcumHessian, const bool bAllPoints) {
  Sim3OptPack pk;
  if (!PackOptimizeSim3(pKF1, pKF2, vpMatches1, bAllPoints, pk)) {
    std::fprintf(stderr, "OptimizeSim3: %s; not supported\n", pk.unsupported);
    return 0;
  }
  osh_lba_ctx* ctx = HostSolverContext();
  if (!ctx) return 0;
  osh_sim3_problem prob;
  pk.fill(prob, g2oS12, th2, bFixScale);
  const size_t n = pk.index.size();
  std::vector<uint8_t> outlier(n);
  osh_sim3_result res;
  res.outlier1 = nullptr; res.outlier = outlier.data(); res.chi2_12 = nullptr; res.chi2_21 = nullptr;
  if (osh_sim3_optimize(ctx, 1, &prob, &res) != OSH_OK) {
    std::fprintf(stderr, "OptimizeSim3: device solve failed (%s); matches and Sim3 left untouched\n", osh_last_error());
    return 0;
  }
  for (size_t k = 0; k < n; ++k)
    if (outlier[k]) vpMatches1[pk.index[k]] = static_cast<MapPoint*>(NULL);   // :2301, :2373
  if (!res.round2) return 0;   // nCorrespondences - nBad < 10 (:2321-2322): g2oS12 and mAcumHessian untouched
  for (int r = 0; r < 7; ++r)
    for (int c = 0; c < 7; ++c) mAcumHessian(r, c) = 0.0;   // :2329, never accumulated
  const double* S = res.S12;
  g2oS12 = g2o::Sim3(Eigen::Quaterniond(S[3], S[0], S[1], S[2]), Eigen::Vector3d(S[4], S[5], S[6]), S[7]);
  return res.n_in;
}

}  // namespace ORB_SLAM3
