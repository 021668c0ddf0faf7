/* Tracking.h -- members of ORB_SLAM3::Tracking used by LocalMapping::CreateNewMapPoints (reference include/Tracking.h:121-131).
 * Minimal test double. */
#ifndef TRACKING_H
#define TRACKING_H
namespace ORB_SLAM3 {
class Tracking {
 public:
  enum eTrackingState { SYSTEM_NOT_READY = -1, NO_IMAGES_YET = 0, NOT_INITIALIZED = 1, OK = 2, RECENTLY_LOST = 3, LOST = 4, OK_KLT = 5 };
  eTrackingState mState = NO_IMAGES_YET;
};
}  // namespace ORB_SLAM3
#endif
