/* Atlas.h -- members of ORB_SLAM3::Atlas used by LocalMapping::CreateNewMapPoints (reference include/Atlas.h;
 * src/Atlas.cc:109-113,249-258).  Minimal test double: one current map, no locking. */
#ifndef ATLAS_H
#define ATLAS_H
#include "Map.h"
#include "MapPoint.h"
namespace ORB_SLAM3 {
class Atlas {
 public:
  Map* GetCurrentMap() { return mpCurrentMap; }
  void AddMapPoint(MapPoint* pMP) { pMP->GetMap()->AddMapPoint(pMP); }
  // test-double state
  Map* mpCurrentMap = nullptr;
};
}  // namespace ORB_SLAM3
#endif
