/* LoopClosing.h -- what the hot path names of ORB_SLAM3::LoopClosing: the keyframe -> corrected Sim3 map that
 * Optimizer::MergeInertialBA fills (reference include/LoopClosing.h:49-51) and the two SearchAndFuse overloads
 * (src/LoopClosing.cc:2120-2201; private there, public in this stand-in), csrc/host/LoopClosing.cc. */
#ifndef LOOPCLOSING_H
#define LOOPCLOSING_H
#include <functional>
#include <map>
#include <set>
#include <utility>
#include <vector>
#include "orbslam3_compat.h"
namespace ORB_SLAM3 {
class KeyFrame;
class MapPoint;
class LoopClosing {
 public:
  typedef std::pair<std::set<KeyFrame*>, int> ConsistentGroup;
  typedef std::map<KeyFrame*, g2o::Sim3, std::less<KeyFrame*>, Eigen::aligned_allocator<std::pair<KeyFrame* const, g2o::Sim3>>> KeyFrameAndPose;
  // The loop's map points fused into every keyframe of the map through its corrected Sim3 (CorrectLoop), or through its own pose
  // (MergeLocal, MergeLocal2): ONE ORBmatcher::FuseBatch, the Replace loop of each keyframe between the targets' replays.
  void SearchAndFuse(const KeyFrameAndPose& CorrectedPosesMap, std::vector<MapPoint*>& vpMapPoints);
  void SearchAndFuse(const std::vector<KeyFrame*>& vConectedKFs, std::vector<MapPoint*>& vpMapPoints);
  // stand-in only, not for the reference's class: what the last SearchAndFuse did (the reference keeps total_replaces in a local)
  int mnLastFuseReplaces = 0, mnLastFuseResearched = 0, mnLastFuseResearchedChanged = 0;
  bool mbFuseSearchOnHost = false;   // test aid: ORBmatcher::mbFuseBatchSearchOnHost of the matcher it makes
};
}  // namespace ORB_SLAM3
#endif
