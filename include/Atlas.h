/* Atlas.h -- members of ORB_SLAM3::Atlas used by LocalMapping::CreateNewMapPoints, ProcessNewKeyFrame and KeyFrameCulling (reference
 * include/Atlas.h; src/Atlas.cc:103-113,185-189,249-258,296-300).  Minimal test double: one current map, no locking. */
#ifndef ATLAS_H
#define ATLAS_H
#include "KeyFrame.h"
#include "Map.h"
#include "MapPoint.h"
namespace ORB_SLAM3 {
class Atlas {
 public:
  Map* GetCurrentMap() { return mpCurrentMap; }
  void AddMapPoint(MapPoint* pMP) { pMP->GetMap()->AddMapPoint(pMP); }
  void AddKeyFrame(KeyFrame* pKF) { pKF->GetMap()->AddKeyFrame(pKF); }   // src/Atlas.cc:103-107
  bool isImuInitialized() { return mpCurrentMap->isImuInitialized(); }     // src/Atlas.cc:296-300
  long unsigned int KeyFramesInMap() { return mpCurrentMap->KeyFramesInMap(); }   // src/Atlas.cc:185-189
  // test-double state
  Map* mpCurrentMap = nullptr;
};
}  // namespace ORB_SLAM3
#endif
