/* LocalMapping.h -- members of ORB_SLAM3::LocalMapping used by LocalMapping::ProcessNewKeyFrame, MapPointCulling, CreateNewMapPoints,
 * SearchInNeighbors and KeyFrameCulling (reference include/LocalMapping.h:111-112,134,144-145,164-172; src/LocalMapping.cc:306-395,398-853,932-1089).  Minimal test double: the members the method reads, public, and no
 * thread. */
#ifndef LOCALMAPPING_H
#define LOCALMAPPING_H
#include <list>
#include <mutex>
#include "Atlas.h"
#include "KeyFrame.h"
#include "MapPoint.h"
#include "Tracking.h"
namespace ORB_SLAM3 {
class LocalMapping {
 public:
  // src/LocalMapping.cc:398-741: the neighbour list, the baseline test and ORBmatcher::SearchForTriangulation per neighbour on the
  // host side, the per-match body (:503-720) in one osh_orb_triangulate_new_points call per neighbour, the map points created from
  // its results in match order (csrc/host/LocalMapping.cc)
  void CreateNewMapPoints();
  // src/LocalMapping.cc:306-346 and :743-853, statement for statement; the per-point ComputeDistinctiveDescriptors /
  // UpdateNormalAndDepth pairs (:328-331, :843-846) are one MapPoint::RefreshBatch each (csrc/host/LocalMapping.cc)
  void ProcessNewKeyFrame();
  void SearchInNeighbors();
  // src/LocalMapping.cc:354-395, a plain host body (csrc/host/LocalMapping.cc)
  void MapPointCulling();
  // src/LocalMapping.cc:932-1089, statement for statement with the counting of :976-1042 on the device: the candidates, their
  // points and the points' observations are packed and staged ONCE (PackKeyFrameCull, osh_orb_keyframe_cull_stage), one
  // osh_orb_keyframe_cull_count gives nMPs / nRedundantObservations of every candidate, and after every keyframe that SetBadFlag
  // has actually made bad one more count gives those of the candidates after it: the number of device calls is one more than the
  // number of keyframes culled.  mnKeyFrameCullDeviceCalls (ADD THIS MEMBER; it is only read by tests) counts them, 0 on the
  // host path.
  void KeyFrameCulling();
  int mnKeyFrameCullDeviceCalls = 0;
  bool CheckNewKeyFrames() { std::unique_lock<std::mutex> lock(mMutexNewKFs); return !mlNewKeyFrames.empty(); }   // :342-346

  bool mbFarPoints = false;
  float mThFarPoints = 0;
  bool mbMonocular = false;
  bool mbInertial = false;
  bool mbAbortBA = false;   // include/LocalMapping.h:172
  Atlas* mpAtlas = nullptr;
  Tracking* mpTracker = nullptr;
  KeyFrame* mpCurrentKeyFrame = nullptr;
  std::list<KeyFrame*> mlNewKeyFrames;
  std::list<MapPoint*> mlpRecentAddedMapPoints;
  std::mutex mMutexNewKFs;
};
}  // namespace ORB_SLAM3
#endif
