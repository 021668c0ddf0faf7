// LocalMapping.cc -- LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:398-741) on MI355X (host side).
//
// The neighbour list, the baseline test and ORBmatcher::SearchForTriangulation (itself on the device, ORBmatcher.cc) stay in the
// reference's order, one neighbour after another: a point created for neighbour i takes its feature out of the search of
// neighbour i + 1.  The loop over the matched pairs (:495-739) is split: everything up to the decision "a new map point"
// (:503-720) runs for all pairs of the neighbour in ONE osh_orb_triangulate_new_points call (csrc/newpoint_device.hip), and the
// part that changes the map (:722-738) is replayed on the host for the accepted pairs in match order.
//
// Deviations from the reference, all intended:
//   * the null vector of GeometricTools::Triangulate comes from an FP64 Jacobi method on the device, and x3D is rounded to float32
//     once (include/orbslam3_hip.h);
//   * in the monocular median-depth test a neighbour without map points is skipped; the reference indexes an empty vector there
//     (KeyFrame::ComputeSceneMedianDepth, src/KeyFrame.cc:806);
//   * on a device error (or keyframes the pack refuses) no point is created for that neighbour and a message goes to stderr.
#include "LocalMapping.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "ORBmatcher.h"
#include "host_pack.h"
#include "orbslam3_hip.h"

namespace ORB_SLAM3 {

osh_orb_ctx* HostMatcherContext();   // csrc/host/ORBmatcher.cc

void LocalMapping::CreateNewMapPoints() {
  // Retrieve neighbor keyframes in covisibility graph (:400-419)
  int nn = 10;
  if (mbMonocular) nn = 30;
  std::vector<KeyFrame*> vpNeighKFs = mpCurrentKeyFrame->GetBestCovisibilityKeyFrames(nn);
  if (mbInertial) {
    KeyFrame* pKF = mpCurrentKeyFrame;
    int count = 0;
    while (((int)vpNeighKFs.size() <= nn) && (pKF->mPrevKF) && (count++ < nn)) {
      if (std::find(vpNeighKFs.begin(), vpNeighKFs.end(), pKF->mPrevKF) == vpNeighKFs.end()) vpNeighKFs.push_back(pKF->mPrevKF);
      pKF = pKF->mPrevKF;
    }
  }

  ORBmatcher matcher(0.6f, false);
  // Ow1 is set here and, on a rig, again by every matched pair (:527-558): the baseline test of the next neighbour reads what
  // the last pair of the previous one left
  Eigen::Vector3f Ow1 = mpCurrentKeyFrame->GetCameraCenter();
  const float ratioFactor = 1.5f * mpCurrentKeyFrame->mfScaleFactor;

  for (size_t i = 0; i < vpNeighKFs.size(); i++) {
    if (i > 0 && CheckNewKeyFrames()) return;
    KeyFrame* pKF2 = vpNeighKFs[i];

    // Check first that baseline is not too short (:454-471)
    const Eigen::Vector3f Ow2 = pKF2->GetCameraCenter();
    const float bx = Ow2(0) - Ow1(0), by = Ow2(1) - Ow1(1), bz = Ow2(2) - Ow1(2);
    const float baseline = std::sqrt(bx * bx + (by * by + bz * bz));
    if (!mbMonocular) {
      if (baseline < pKF2->mb) continue;
    } else {
      bool any = false;
      for (MapPoint* pMP : pKF2->GetMapPointMatches()) if (pMP) { any = true; break; }
      if (!any) continue;                                   // the reference reads vDepths[0] of an empty vector here
      const float medianDepthKF2 = pKF2->ComputeSceneMedianDepth(2);
      const float ratioBaselineDepth = baseline / medianDepthKF2;
      if (ratioBaselineDepth < 0.01) continue;
    }

    // Search matches that fullfil epipolar constraint (:473-478)
    std::vector<std::pair<size_t, size_t>> vMatchedIndices;
    const bool bCoarse = mbInertial && mpTracker->mState == Tracking::RECENTLY_LOST && mpCurrentKeyFrame->GetMap()->GetIniertialBA2();
    matcher.SearchForTriangulation(mpCurrentKeyFrame, pKF2, vMatchedIndices, false, bCoarse);
    const int nmatches = (int)vMatchedIndices.size();
    if (nmatches == 0) continue;

    // Triangulate each match (:495-720) on the device
    NewPointPack pk;
    if (!PackNewMapPoints(mpCurrentKeyFrame, pKF2, vMatchedIndices, pk)) {
      std::fprintf(stderr, "LocalMapping::CreateNewMapPoints: %s\n", pk.unsupported);
      continue;
    }
    osh_orb_ctx* ctx = HostMatcherContext();
    if (!ctx) {
      std::fprintf(stderr, "LocalMapping::CreateNewMapPoints: %s\n", osh_last_error());
      continue;
    }
    osh_newpoint_segment seg;
    pk.fill(seg, mpCurrentKeyFrame, pKF2, ratioFactor, mbInertial, mbFarPoints, mThFarPoints);
    std::vector<uint8_t> stage(nmatches);
    std::vector<float> x3d((size_t)nmatches * 3);
    const osh_newpoint_result res{stage.data(), nullptr, nullptr, x3d.data()};
    if (osh_orb_triangulate_new_points(ctx, 1, &seg, &res) != OSH_OK) {
      std::fprintf(stderr, "LocalMapping::CreateNewMapPoints: %s\n", osh_last_error());
      continue;
    }
    if (mpCurrentKeyFrame->mpCamera2 && pKF2->mpCamera2) {   // what the last pair leaves in Ow1 (:527-558)
      const int last1 = (int)vMatchedIndices[nmatches - 1].first;
      const bool bRight1 = !(mpCurrentKeyFrame->NLeft == -1 || last1 < mpCurrentKeyFrame->NLeft);
      Ow1 = bRight1 ? mpCurrentKeyFrame->GetRightCameraCenter() : mpCurrentKeyFrame->GetCameraCenter();
    }

    // Triangulation is succesfull (:722-738), in match order
    for (int ikp = 0; ikp < nmatches; ikp++) {
      if (stage[ikp] != OSH_NEWPOINT_ACCEPTED) continue;
      const int idx1 = (int)vMatchedIndices[ikp].first, idx2 = (int)vMatchedIndices[ikp].second;
      const Eigen::Vector3f x3D(x3d[3 * (size_t)ikp], x3d[3 * (size_t)ikp + 1], x3d[3 * (size_t)ikp + 2]);
      MapPoint* pMP = new MapPoint(x3D, mpCurrentKeyFrame, mpAtlas->GetCurrentMap());
      pMP->AddObservation(mpCurrentKeyFrame, idx1);
      pMP->AddObservation(pKF2, idx2);
      mpCurrentKeyFrame->AddMapPoint(pMP, idx1);
      pKF2->AddMapPoint(pMP, idx2);
      pMP->ComputeDistinctiveDescriptors();
      pMP->UpdateNormalAndDepth();
      mpAtlas->AddMapPoint(pMP);
      mlpRecentAddedMapPoints.push_back(pMP);
    }
  }
}

}  // namespace ORB_SLAM3
