// host_graph.h -- osh_host_graph (include/orbslam3_hip_host.h): the stand-in map the wrappers of harness.cc and mappoints.cc share.
#pragma once
#include <memory>
#include <new>
#include <type_traits>
#include <vector>

#include "KeyFrame.h"
#include "Map.h"
#include "MapPoint.h"
#include "host_pack.h"

using namespace ORB_SLAM3;

// The keyframes of a stand-in map live in one block, in array order: containers the reference keys by KeyFrame* (LoopConnections
// of the essential graphs, std::set<KeyFrame*>) then iterate in the same order for every construction of the same map, as they
// would not with one heap allocation per keyframe, whose addresses depend on what the thread freed before.
struct KfDestroy { void operator()(KeyFrame* k) const { k->~KeyFrame(); } };
using KfSlot = std::aligned_storage_t<sizeof(KeyFrame), alignof(KeyFrame)>;

struct osh_host_graph {
  Map map;
  std::unique_ptr<GeometricCamera> cam, cam2;
  std::unique_ptr<KfSlot[]> kf_block;   // declared before kfs: released after the keyframes in it are destroyed
  std::vector<std::unique_ptr<KeyFrame, KfDestroy>> kfs;
  std::vector<std::unique_ptr<MapPoint>> mps;
  std::vector<std::unique_ptr<IMU::Preintegrated>> preints;
  LibaPack liba;   // storage behind osh_host_pack_liba
  bool last_has_kb8 = false;   // camera model of the last osh_host_pack_lba / _gba / _welding
  double last_kb8[4] = {0, 0, 0, 0};
  bool last_has_rig = false;
  double last_cam2[8] = {0, 0, 0, 0, 0, 0, 0, 0}, last_trl[7] = {0, 0, 0, 1, 0, 0, 0};
};
