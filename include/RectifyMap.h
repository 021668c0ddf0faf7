/* RectifyMap.h -- ADD THIS CLASS to the reference's tree: the two CV_32F maps Settings::precomputeRectificationMaps
 * (src/Settings.cc:485-509) leaves in M1l / M2l (or M1r / M2r), as the resident rectify map of include/orbslam3_hip.h.  Built once
 * at start-up, for example RectifyMap(M1l.ptr<float>(), M1l.step, M2l.ptr<float>(), M2l.step, M1l.rows, M1l.cols, rows and cols of
 * the camera images); ORBextractor::ExtractBatchRaw reads it through ImagePrep::pMap.  The maps are copied, so the cv::Mat may go.
 * The copy on the device is made on the first use on that device and destroyed with the object; every thread may use it. */
#ifndef RECTIFYMAP_H
#define RECTIFYMAP_H
#include <cstddef>
#include <map>
#include <mutex>
#include <vector>
#include "orbslam3_hip.h"
namespace ORB_SLAM3 {
class RectifyMap {
 public:
  /* pMapX / pMapY: the source x / y of every destination pixel, nRows rows of nCols floats, nStepX / nStepY bytes apart;
   * nSrcRows x nSrcCols: the images the maps were made for */
  RectifyMap(const float* pMapX, size_t nStepX, const float* pMapY, size_t nStepY, int nRows, int nCols, int nSrcRows, int nSrcCols);
  ~RectifyMap();
  RectifyMap(const RectifyMap&) = delete;
  RectifyMap& operator=(const RectifyMap&) = delete;

  /* The map on `device`, made on the first call for that device; null (the reason is osh_last_error()) when it cannot be made */
  const osh_rectify_map* OnDevice(int device) const;

  int rows() const { return mnRows; }
  int cols() const { return mnCols; }
  int srcRows() const { return mnSrcRows; }
  int srcCols() const { return mnSrcCols; }

 private:
  int mnRows, mnCols, mnSrcRows, mnSrcCols;
  std::vector<float> mvMapX, mvMapY;   /* rows packed */
  mutable std::mutex mMutexDevice;
  mutable std::map<int, osh_rectify_map*> mDeviceMap;
};

/* How ORBextractor::ExtractBatchRaw turns a raw camera image into the grey image operator() reads: what System::Track* and
 * Tracking::GrabImage* do with mbRGB, the rectification maps and newImSize */
struct ImagePrep {
  bool bRGB = true;                   /* mbRGB: the channel order of a 3- or 4-channel image */
  const RectifyMap* pMap = nullptr;   /* settings_->needToRectify(): the camera's map; null: no remap */
  int newRows = 0, newCols = 0;       /* settings_->needToResize(): newImSize; 0, 0: the map's size, else the image's */
};
}  // namespace ORB_SLAM3
#endif
