// RectifyMap.cc -- ORB_SLAM3::RectifyMap (include/RectifyMap.h, a class to ADD): the rectification maps of a camera, copied at
// construction and made resident with osh_rectify_map_create (csrc/orb_prepare_device.hip) on the first use on a device, under a
// mutex, as ORBVocabulary keeps its device vocabulary.  The destructor destroys the device copies: the object must outlive the
// calls that use it.
#include "RectifyMap.h"

#include <cstring>

namespace ORB_SLAM3 {

RectifyMap::RectifyMap(const float* pMapX, size_t nStepX, const float* pMapY, size_t nStepY, int nRows, int nCols, int nSrcRows, int nSrcCols)
    : mnRows(nRows), mnCols(nCols), mnSrcRows(nSrcRows), mnSrcCols(nSrcCols) {
  if (!pMapX || !pMapY || nRows <= 0 || nCols <= 0 || nStepX < sizeof(float) * (size_t)nCols || nStepY < sizeof(float) * (size_t)nCols) {
    mnRows = mnCols = 0;   // osh_rectify_map_create refuses it at the first use, with its message
    return;
  }
  mvMapX.resize((size_t)nRows * nCols); mvMapY.resize((size_t)nRows * nCols);
  for (int r = 0; r < nRows; ++r) {
    std::memcpy(&mvMapX[(size_t)r * nCols], reinterpret_cast<const char*>(pMapX) + (size_t)r * nStepX, sizeof(float) * (size_t)nCols);
    std::memcpy(&mvMapY[(size_t)r * nCols], reinterpret_cast<const char*>(pMapY) + (size_t)r * nStepY, sizeof(float) * (size_t)nCols);
  }
}

RectifyMap::~RectifyMap() {
  std::lock_guard<std::mutex> lock(mMutexDevice);
  for (auto& dm : mDeviceMap) osh_rectify_map_destroy(dm.second);
  mDeviceMap.clear();
}

const osh_rectify_map* RectifyMap::OnDevice(int device) const {
  std::lock_guard<std::mutex> lock(mMutexDevice);
  const auto it = mDeviceMap.find(device);
  if (it != mDeviceMap.end()) return it->second;
  osh_rectify_map_desc desc{};
  desc.rows = mnRows; desc.cols = mnCols; desc.src_rows = mnSrcRows; desc.src_cols = mnSrcCols;
  desc.map_x = mvMapX.empty() ? nullptr : mvMapX.data(); desc.map_y = mvMapY.empty() ? nullptr : mvMapY.data();
  desc.map_x_stride = desc.map_y_stride = (int64_t)sizeof(float) * mnCols;
  osh_rectify_map* map = nullptr;
  if (osh_rectify_map_create(device, &desc, &map) != OSH_OK) return nullptr;
  mDeviceMap[device] = map;
  return map;
}

}  // namespace ORB_SLAM3
