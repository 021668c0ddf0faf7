// LocalMapping.cc -- LocalMapping::ProcessNewKeyFrame (reference src/LocalMapping.cc:306-346), MapPointCulling (:354-395),
// CreateNewMapPoints (:398-741), SearchInNeighbors (:743-853) and KeyFrameCulling (:932-1089) on MI355X (host side).
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
// KeyFrameCulling:
// Everything but the counting loop (:976-1042) is the reference's statement for statement: the candidate list, redundant_th, the
// last_ID walk, count++ and the skip of the initial and of bad keyframes, the decision, the inertial guards and both cull branches
// with MergePrevious and the re-linking, the two exits.  The counting is osh_orb_keyframe_cull_count on a problem that
// PackKeyFrameCull (host_pack.h) builds and osh_orb_keyframe_cull_stage uploads ONCE per call: the first count, with the empty
// removed set, gives nMPs and nRedundantObservations of every candidate; whenever SetBadFlag has actually made a keyframe bad
// (isBad() afterwards: one with mbNotErase only gets mbToBeErased) it joins the removed set and one more count gives the values
// of the candidates after it.  So a call that culls n keyframes makes n + 1 device calls.  The host never recounts: that a culled
// keyframe's points lose an observer and may go bad is the state rule of csrc/keyframe_cull.h, evaluated on the device.  Without a
// device, on a device error or beyond the limits of the entry the same counts come from the host build of that header.
// The loop leaves after the 101st keyframe of the list (:1084) unless that one is skipped by a `continue`, which passes the exit
// test as well; the first OSH_KFCULL_MAX_CANDIDATES = 128 keyframes of the list are packed, and a keyframe the loop reaches beyond
// them is counted alone on the host from the map as it is then.
//
// Deviations from the reference, all intended:
//   * KeyFrameCulling reads the level of a right slot i of a rig from mvKeysRight[i - NLeft]; the reference reads mvKeysRight[i]
//     (:1003), the wrong key or one past the end;
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

#include "../keyframe_cull.h"
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

// src/LocalMapping.cc:354-395
void LocalMapping::MapPointCulling() {
  // Check Recent Added MapPoints
  std::list<MapPoint*>::iterator lit = mlpRecentAddedMapPoints.begin();
  const unsigned long int nCurrentKFid = mpCurrentKeyFrame->mnId;

  int nThObs;
  if (mbMonocular) nThObs = 2;
  else nThObs = 3;
  const int cnThObs = nThObs;

  while (lit != mlpRecentAddedMapPoints.end()) {
    MapPoint* pMP = *lit;
    if (pMP->isBad()) {
      lit = mlpRecentAddedMapPoints.erase(lit);
    } else if (pMP->GetFoundRatio() < 0.25f) {
      pMP->SetBadFlag();
      lit = mlpRecentAddedMapPoints.erase(lit);
    } else if (((int)nCurrentKFid - (int)pMP->mnFirstKFid) >= 2 && pMP->Observations() <= cnThObs) {
      pMP->SetBadFlag();
      lit = mlpRecentAddedMapPoints.erase(lit);
    } else if (((int)nCurrentKFid - (int)pMP->mnFirstKFid) >= 3) {
      lit = mlpRecentAddedMapPoints.erase(lit);
    } else {
      lit++;
    }
  }
}

namespace {

// nMPs, nRedundantObservations and the decision of the candidates from `first` on under a removed set, on the device (a staged
// problem) or by the host build of csrc/keyframe_cull.h
struct KeyFrameCullCounter {
  const KeyFrameCullPack& pk;
  float redundant_th;
  osh_orb_ctx* ctx = nullptr;   // null: the host path
  int device_calls = 0;
  int base = 0;                 // the candidate entry 0 of the arrays belongs to
  std::vector<int32_t> n_mps, n_redundant;
  std::vector<uint8_t> redundant;
  std::vector<osh::KcPoint> h_point;   // the host path's records, built on first use
  std::vector<uint32_t> h_obs;

  KeyFrameCullCounter(const KeyFrameCullPack& pack, float th) : pk(pack), redundant_th(th), n_mps(pack.n_candidates), n_redundant(pack.n_candidates), redundant(pack.n_candidates) {}

  void Stage() {
    if (!pk.within_device_limits()) return;
    ctx = HostMatcherContext();
    if (!ctx) return;
    osh_kfcull_problem b;
    pk.fill(b, redundant_th);
    if (osh_orb_keyframe_cull_stage(ctx, &b) != OSH_OK) {
      std::fprintf(stderr, "LocalMapping::KeyFrameCulling: %s; counted on the host\n", osh_last_error());
      ctx = nullptr;
    }
  }
  void Count(const std::vector<int32_t>& removed, int first) {
    base = first;
    if (ctx) {
      const osh_kfcull_result r{n_mps.data(), n_redundant.data(), redundant.data()};
      ++device_calls;
      if (osh_orb_keyframe_cull_count(ctx, (int32_t)removed.size(), removed.data(), first, &r) == OSH_OK) return;
      std::fprintf(stderr, "LocalMapping::KeyFrameCulling: %s; counted on the host\n", osh_last_error());
      ctx = nullptr;
    }
    if (h_point.size() != pk.points.size() || h_obs.size() != pk.obs_kf.size()) {
      h_point.resize(pk.points.size()); h_obs.resize(pk.obs_kf.size());
      for (size_t p = 0; p < pk.points.size(); ++p)
        h_point[p] = osh::KcPoint{pk.point_obs_off[p], pk.point_obs_off[p + 1] - pk.point_obs_off[p], pk.point_n_obs[p], (int)pk.point_bad[p]};
      for (size_t e = 0; e < pk.obs_kf.size(); ++e) h_obs[e] = osh::kc_obs_word(pk.obs_kf[e], pk.obs_level[e], pk.obs_weight[e]);
    }
    std::vector<uint32_t> mask((pk.table.size() + 31) / 32 + 1, 0u);
    for (const int32_t k : removed) mask[k >> 5] |= 1u << (k & 31);
    const osh::KcView v{pk.cand_slot_off.data(), pk.slot_point.data(), pk.slot_level.data(), h_point.data(), h_obs.data()};
    for (int k = first; k < pk.n_candidates; ++k) {
      int a, b;
      osh::kc_count_candidate(v, mask.data(), k, a, b);
      n_mps[k - first] = a; n_redundant[k - first] = b; redundant[k - first] = (uint8_t)osh::kc_decide(b, a, redundant_th);
    }
  }
};

}  // namespace

// src/LocalMapping.cc:932-1089
void LocalMapping::KeyFrameCulling() {
  // Check redundant keyframes (only local keyframes): a keyframe is considered redundant if 90% of the MapPoints it sees are seen
  // in at least other 3 keyframes (in the same or finer scale); only close stereo points are considered
  const int Nd = 21;
  mpCurrentKeyFrame->UpdateBestCovisibles();
  std::vector<KeyFrame*> vpLocalKeyFrames = mpCurrentKeyFrame->GetVectorCovisibleKeyFrames();

  float redundant_th;
  if (!mbInertial) redundant_th = 0.9;
  else if (mbMonocular) redundant_th = 0.9;
  else redundant_th = 0.5;

  const bool bInitImu = mpAtlas->isImuInitialized();
  int count = 0;

  // Compute last KF from optimizable window:
  unsigned int last_ID = 0;
  if (mbInertial) {
    int count = 0;
    KeyFrame* aux_KF = mpCurrentKeyFrame;
    while (count < Nd && aux_KF->mPrevKF) {
      aux_KF = aux_KF->mPrevKF;
      count++;
    }
    last_ID = aux_KF->mnId;
  }

  // the counting of :976-1042 for all candidates at once
  mnKeyFrameCullDeviceCalls = 0;
  const std::vector<KeyFrame*> vpCandidates(vpLocalKeyFrames.begin(), vpLocalKeyFrames.begin() + std::min<size_t>(vpLocalKeyFrames.size(), OSH_KFCULL_MAX_CANDIDATES));
  KeyFrameCullPack pk;
  PackKeyFrameCull(vpCandidates, mbMonocular, pk);
  KeyFrameCullCounter counter(pk, redundant_th);
  std::vector<int32_t> removed;
  counter.Stage();
  counter.Count(removed, 0);

  int at = -1;   // the candidate's place in the list
  for (std::vector<KeyFrame*>::iterator vit = vpLocalKeyFrames.begin(), vend = vpLocalKeyFrames.end(); vit != vend; vit++) {
    count++;
    at++;
    KeyFrame* pKF = *vit;

    if ((pKF->mnId == pKF->GetMap()->GetInitKFid()) || pKF->isBad()) continue;

    bool bRedundant;   // nRedundantObservations > redundant_th * nMPs
    if (at < pk.n_candidates) {
      bRedundant = counter.redundant[at - counter.base] != 0;
    } else {           // past the packed candidates: this keyframe alone, from the map as it is now, on the host
      KeyFrameCullPack one;
      PackKeyFrameCull(std::vector<KeyFrame*>(1, pKF), mbMonocular, one);
      KeyFrameCullCounter single(one, redundant_th);
      single.Count(std::vector<int32_t>(), 0);
      bRedundant = single.redundant[0] != 0;
    }
    if (bRedundant) {
      if (mbInertial) {
        if (mpAtlas->KeyFramesInMap() <= Nd) continue;

        if (pKF->mnId > (mpCurrentKeyFrame->mnId - 2)) continue;

        if (pKF->mPrevKF && pKF->mNextKF) {
          const float t = pKF->mNextKF->mTimeStamp - pKF->mPrevKF->mTimeStamp;

          if ((bInitImu && (pKF->mnId < last_ID) && t < 3.) || (t < 0.5)) {
            pKF->mNextKF->mpImuPreintegrated->MergePrevious(pKF->mpImuPreintegrated);
            pKF->mNextKF->mPrevKF = pKF->mPrevKF;
            pKF->mPrevKF->mNextKF = pKF->mNextKF;
            pKF->mNextKF = NULL;
            pKF->mPrevKF = NULL;
            pKF->SetBadFlag();
          } else if (!mpCurrentKeyFrame->GetMap()->GetIniertialBA2() && ((pKF->GetImuPosition() - pKF->mPrevKF->GetImuPosition()).norm() < 0.02) && (t < 3)) {
            pKF->mNextKF->mpImuPreintegrated->MergePrevious(pKF->mpImuPreintegrated);
            pKF->mNextKF->mPrevKF = pKF->mPrevKF;
            pKF->mPrevKF->mNextKF = pKF->mNextKF;
            pKF->mNextKF = NULL;
            pKF->mPrevKF = NULL;
            pKF->SetBadFlag();
          }
        }
      } else {
        pKF->SetBadFlag();
      }
      // a keyframe that is gone takes an observer from its points: the candidates after it are counted again
      if (pKF->isBad() && at < pk.n_candidates) {
        removed.push_back(at);
        counter.Count(removed, at + 1);
      }
    }
    if ((count > 20 && mbAbortBA) || count > 100) break;
  }
  mnKeyFrameCullDeviceCalls = counter.device_calls;
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
  // one batch for all targets (ORBmatcher::FuseBatch): the map it leaves is the one of the reference's loop of Fuse calls.  On a rig
  // the second call is Fuse(pKFi, vpMapPointMatches, true), whose `true` binds to th: th = 1, the left camera again
  std::vector<ORBmatcher::FuseTarget> vFuseTargets;
  for (std::vector<KeyFrame*>::iterator vit = vpTargetKFs.begin(), vend = vpTargetKFs.end(); vit != vend; vit++) {
    KeyFrame* pKFi = *vit;
    vFuseTargets.push_back(ORBmatcher::FuseTarget{pKFi, 3.0f, false});
    if (pKFi->NLeft != -1) vFuseTargets.push_back(ORBmatcher::FuseTarget{pKFi, 1.0f, false});
  }
  matcher.FuseBatch(vFuseTargets, vpMapPointMatches);

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

  vFuseTargets.assign(1, ORBmatcher::FuseTarget{mpCurrentKeyFrame, 3.0f, false});
  if (mpCurrentKeyFrame->NLeft != -1) vFuseTargets.push_back(ORBmatcher::FuseTarget{mpCurrentKeyFrame, 1.0f, false});
  matcher.FuseBatch(vFuseTargets, vpFuseCandidates);

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
