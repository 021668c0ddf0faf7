// LocalMapping.cc -- LocalMapping::ProcessNewKeyFrame (reference src/LocalMapping.cc:306-346), CreateNewMapPoints (:398-741) and
// SearchInNeighbors (:743-853) on MI355X (host side).
//
// ProcessNewKeyFrame and SearchInNeighbors follow the reference statement for statement: the order of vpTargetKFs, the
// mnFuseTargetForKF / mnFuseCandidateForKF marks, the mbAbortBA exits, one ORBmatcher::Fuse per target keyframe (and one more for
// the right camera of a rig), each of them on the device (ORBmatcher.cc).  Their loops over MapPoint::ComputeDistinctiveDescriptors
// and UpdateNormalAndDepth (:328-331 and :843-846) are ONE MapPoint::RefreshBatch (MapPoint.cc) over the same points in the same
// order.  That is the same computation: neither function reads another point's state, and nothing between the pairs of two points
// changes what either reads (in ProcessNewKeyFrame the AddObservation calls of all points come first; each touches its own point).
// The rig calls are kept as the reference writes them, Fuse(pKF, points, true): with the signature Fuse(KeyFrame*, const
// vector<MapPoint*>&, const float th = 3.0, const bool bRight = false) the `true` is th = 1.0f and bRight stays false, so the
// second call searches the left camera again with a narrower radius (:803,833).
//
// CreateNewMapPoints:
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

// src/LocalMapping.cc:306-346
void LocalMapping::ProcessNewKeyFrame() {
  {
    std::unique_lock<std::mutex> lock(mMutexNewKFs);
    mpCurrentKeyFrame = mlNewKeyFrames.front();
    mlNewKeyFrames.pop_front();
  }

  // Compute Bags of Words structures
  mpCurrentKeyFrame->ComputeBoW();

  // Associate MapPoints to the new keyframe and update normal and descriptor
  const std::vector<MapPoint*> vpMapPointMatches = mpCurrentKeyFrame->GetMapPointMatches();
  std::vector<MapPoint*> vpRefresh;
  for (size_t i = 0; i < vpMapPointMatches.size(); i++) {
    MapPoint* pMP = vpMapPointMatches[i];
    if (pMP) {
      if (!pMP->isBad()) {
        if (!pMP->IsInKeyFrame(mpCurrentKeyFrame)) {
          pMP->AddObservation(mpCurrentKeyFrame, i);
          vpRefresh.push_back(pMP);   // UpdateNormalAndDepth, ComputeDistinctiveDescriptors (:330-331)
        } else {                      // this can only happen for new stereo points inserted by the Tracking
          mlpRecentAddedMapPoints.push_back(pMP);
        }
      }
    }
  }
  MapPoint::RefreshBatch(vpRefresh);

  // Update links in the Covisibility Graph
  mpCurrentKeyFrame->UpdateConnections();

  // Insert Keyframe in Map
  mpAtlas->AddKeyFrame(mpCurrentKeyFrame);
}

// src/LocalMapping.cc:743-853
void LocalMapping::SearchInNeighbors() {
  // Retrieve neighbor keyframes
  int nn = 10;
  if (mbMonocular) nn = 30;
  const std::vector<KeyFrame*> vpNeighKFs = mpCurrentKeyFrame->GetBestCovisibilityKeyFrames(nn);
  std::vector<KeyFrame*> vpTargetKFs;
  for (std::vector<KeyFrame*>::const_iterator vit = vpNeighKFs.begin(), vend = vpNeighKFs.end(); vit != vend; vit++) {
    KeyFrame* pKFi = *vit;
    if (pKFi->isBad() || pKFi->mnFuseTargetForKF == mpCurrentKeyFrame->mnId) continue;
    vpTargetKFs.push_back(pKFi);
    pKFi->mnFuseTargetForKF = mpCurrentKeyFrame->mnId;
  }

  // Add some covisible of covisible; extend to some second neighbors if abort is not requested
  for (int i = 0, imax = vpTargetKFs.size(); i < imax; i++) {
    const std::vector<KeyFrame*> vpSecondNeighKFs = vpTargetKFs[i]->GetBestCovisibilityKeyFrames(20);
    for (std::vector<KeyFrame*>::const_iterator vit2 = vpSecondNeighKFs.begin(), vend2 = vpSecondNeighKFs.end(); vit2 != vend2; vit2++) {
      KeyFrame* pKFi2 = *vit2;
      if (pKFi2->isBad() || pKFi2->mnFuseTargetForKF == mpCurrentKeyFrame->mnId || pKFi2->mnId == mpCurrentKeyFrame->mnId) continue;
      vpTargetKFs.push_back(pKFi2);
      pKFi2->mnFuseTargetForKF = mpCurrentKeyFrame->mnId;
    }
    if (mbAbortBA) break;
  }

  // Extend to temporal neighbors
  if (mbInertial) {
    KeyFrame* pKFi = mpCurrentKeyFrame->mPrevKF;
    while (vpTargetKFs.size() < 20 && pKFi) {
      if (pKFi->isBad() || pKFi->mnFuseTargetForKF == mpCurrentKeyFrame->mnId) {
        pKFi = pKFi->mPrevKF;
        continue;
      }
      vpTargetKFs.push_back(pKFi);
      pKFi->mnFuseTargetForKF = mpCurrentKeyFrame->mnId;
      pKFi = pKFi->mPrevKF;
    }
  }

  // Search matches by projection from current KF in target KFs
  ORBmatcher matcher;
  std::vector<MapPoint*> vpMapPointMatches = mpCurrentKeyFrame->GetMapPointMatches();
  for (std::vector<KeyFrame*>::iterator vit = vpTargetKFs.begin(), vend = vpTargetKFs.end(); vit != vend; vit++) {
    KeyFrame* pKFi = *vit;
    matcher.Fuse(pKFi, vpMapPointMatches);
    if (pKFi->NLeft != -1) matcher.Fuse(pKFi, vpMapPointMatches, true);
  }

  if (mbAbortBA) return;

  // Search matches by projection from target KFs in current KF
  std::vector<MapPoint*> vpFuseCandidates;
  vpFuseCandidates.reserve(vpTargetKFs.size() * vpMapPointMatches.size());
  for (std::vector<KeyFrame*>::iterator vitKF = vpTargetKFs.begin(), vendKF = vpTargetKFs.end(); vitKF != vendKF; vitKF++) {
    KeyFrame* pKFi = *vitKF;
    std::vector<MapPoint*> vpMapPointsKFi = pKFi->GetMapPointMatches();
    for (std::vector<MapPoint*>::iterator vitMP = vpMapPointsKFi.begin(), vendMP = vpMapPointsKFi.end(); vitMP != vendMP; vitMP++) {
      MapPoint* pMP = *vitMP;
      if (!pMP) continue;
      if (pMP->isBad() || pMP->mnFuseCandidateForKF == mpCurrentKeyFrame->mnId) continue;
      pMP->mnFuseCandidateForKF = mpCurrentKeyFrame->mnId;
      vpFuseCandidates.push_back(pMP);
    }
  }

  matcher.Fuse(mpCurrentKeyFrame, vpFuseCandidates);
  if (mpCurrentKeyFrame->NLeft != -1) matcher.Fuse(mpCurrentKeyFrame, vpFuseCandidates, true);

  // Update points (:837-849): the pairs of all non-bad matches as one batch
  vpMapPointMatches = mpCurrentKeyFrame->GetMapPointMatches();
  std::vector<MapPoint*> vpRefresh;
  for (size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {
    MapPoint* pMP = vpMapPointMatches[i];
    if (pMP) {
      if (!pMP->isBad()) vpRefresh.push_back(pMP);
    }
  }
  MapPoint::RefreshBatch(vpRefresh);

  // Update connections in covisibility graph
  mpCurrentKeyFrame->UpdateConnections();
}

}  // namespace ORB_SLAM3
