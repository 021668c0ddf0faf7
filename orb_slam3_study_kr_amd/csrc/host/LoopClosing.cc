// LoopClosing.cc -- LoopClosing::SearchAndFuse, both overloads (reference src/LoopClosing.cc:2120-2201): the map points of the loop
// or of the merged map are fused into every keyframe on the list.  The reference calls the Sim3 overload of ORBmatcher::Fuse once per
// keyframe, each followed by the Replace loop over vpReplacePoints; here all keyframes go through ONE ORBmatcher::FuseBatch and the
// Replace loop of keyframe k runs in its `after(k)`, between the replays of keyframes k and k + 1, where the reference has it.
#include "LoopClosing.h"

#include <mutex>

#include "KeyFrame.h"
#include "Map.h"
#include "MapPoint.h"
#include "ORBmatcher.h"

namespace ORB_SLAM3 {

namespace {

// Converter::toSophus(const g2o::Sim3&) (src/Converter.cc): rotation, translation and scale cast to float
Sophus::Sim3f to_sophus(const g2o::Sim3& S) {
  const Eigen::Vector3d& t = S.translation();
  return Sophus::Sim3f(S.rotation().cast<float>(), Eigen::Vector3f((float)t(0), (float)t(1), (float)t(2)), (float)S.scale());
}

void search_and_fuse(LoopClosing* lc, const std::vector<std::pair<KeyFrame*, Sophus::Sim3f>>& targets, std::vector<MapPoint*>& vpMapPoints) {
  ORBmatcher matcher(0.8);
  matcher.mbFuseBatchSearchOnHost = lc->mbFuseSearchOnHost;
  int total_replaces = 0;
  std::vector<std::vector<MapPoint*>> vvpReplacePoints;
  matcher.FuseBatch(targets, vpMapPoints, 4, vvpReplacePoints, [&](int k) {
    Map* pMap = targets[k].first->GetMap();
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);   // Get Map Mutex
    const std::vector<MapPoint*>& vpReplacePoints = vvpReplacePoints[k];
    const int nLP = (int)vpMapPoints.size();
    for (int i = 0; i < nLP; i++) {
      MapPoint* pRep = vpReplacePoints[i];
      if (pRep) {
        total_replaces += 1;
        pRep->Replace(vpMapPoints[i]);
      }
    }
  });
  lc->mnLastFuseReplaces = total_replaces;
  lc->mnLastFuseResearched = matcher.mnFuseBatchResearched;
  lc->mnLastFuseResearchedChanged = matcher.mnFuseBatchResearchedChanged;
}

}  // namespace

void LoopClosing::SearchAndFuse(const KeyFrameAndPose& CorrectedPosesMap, std::vector<MapPoint*>& vpMapPoints) {
  std::vector<std::pair<KeyFrame*, Sophus::Sim3f>> targets;
  for (KeyFrameAndPose::const_iterator mit = CorrectedPosesMap.begin(), mend = CorrectedPosesMap.end(); mit != mend; mit++)   // the map's own order
    targets.push_back(std::make_pair(mit->first, to_sophus(mit->second)));
  search_and_fuse(this, targets, vpMapPoints);
}

void LoopClosing::SearchAndFuse(const std::vector<KeyFrame*>& vConectedKFs, std::vector<MapPoint*>& vpMapPoints) {
  std::vector<std::pair<KeyFrame*, Sophus::Sim3f>> targets;
  for (auto mit = vConectedKFs.begin(), mend = vConectedKFs.end(); mit != mend; mit++) {
    KeyFrame* pKF = (*mit);
    const Sophus::SE3f Tcw = pKF->GetPose();
    targets.push_back(std::make_pair(pKF, Sophus::Sim3f(Tcw.unit_quaternion(), Tcw.translation(), 1.f)));   // Scw.setScale(1.f)
  }
  search_and_fuse(this, targets, vpMapPoints);
}

}  // namespace ORB_SLAM3
