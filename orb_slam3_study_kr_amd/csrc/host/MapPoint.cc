// MapPoint.cc -- MapPoint::RefreshBatch: MapPoint::ComputeDistinctiveDescriptors (reference src/MapPoint.cc:329-403) and
// MapPoint::UpdateNormalAndDepth (:426-494) for a list of map points on MI355X (host side).
//
// The reference runs that pair point by point (LocalMapping::ProcessNewKeyFrame, src/LocalMapping.cc:320-339, and
// SearchInNeighbors, :837-849).  Neither function reads another point's state, so a loop of pairs over a list equals one batch over
// the same list in the same order.  RefreshBatch walks the observations of every non-bad point in map order (PackMapPointRefresh,
// host_pack.h), makes ONE osh_orb_refresh_map_points call (csrc/mappoint_device.hip) and writes mDescriptor, mNormalVector,
// mfMinDistance and mfMaxDistance.  A point occurring twice in the list is computed and written twice, as two calls would.
//
// The two single-point members are not replaced: every existing call site keeps the reference's (in this repository's stand-in:
// the counters of include/MapPoint.h).
//
// Deviations from the reference, all intended:
//   * the float32 statements of the normal and the distances are those of csrc/mappoint_refresh.h (single operations, norm as
//     sqrt(x*x + (y*y + z*z))); parity with the code Eigen generates for them is not pinned;
//   * a point without a reference keyframe is left alone (the reference dereferences the null pointer);
//   * a point with more than OSH_MAPPOINT_MAX_DESCRIPTORS entries is computed by the same statements on the host, inside this
//     function;
//   * on a device error a message goes to stderr and the whole list is computed by those statements on the host.
#include "MapPoint.h"

#include <cstdio>
#include <cstring>
#include <vector>

#include "../mappoint_refresh.h"
#include "KeyFrame.h"
#include "host_pack.h"
#include "orbslam3_hip.h"

namespace ORB_SLAM3 {

osh_orb_ctx* HostMatcherContext();   // csrc/host/ORBmatcher.cc

namespace {

// point k of the pack by the statements of csrc/mappoint_refresh.h on this thread
void RefreshOnHost(const MapPointRefreshPack& pk, size_t k, std::vector<uint16_t>& table, osh::MpOut& o) {
  const int e0 = pk.entry_off[k], n = pk.entry_off[k + 1] - e0;
  const osh::MpPoint p{0, n, {pk.pos[3 * k], pk.pos[3 * k + 1], pk.pos[3 * k + 2]}, pk.ref_centre[k], pk.level_scale[k], pk.top_scale[k]};
  if (table.size() < (size_t)n * n) table.resize((size_t)n * n);
  osh::mappoint_refresh_point(p, reinterpret_cast<const uint32_t*>(pk.desc.data()) + 8 * (size_t)e0, pk.centre.data() + e0, pk.use_desc.data() + e0,
                              pk.centres.data(), table.data(), o);
}

}  // namespace

void MapPoint::RefreshBatch(const std::vector<MapPoint*>& vpMPs) {
  MapPointRefreshPack pk;
  PackMapPointRefresh(vpMPs, pk);
  const size_t P = pk.points.size();
  if (P == 0) return;

  // the points the device takes: all but those above its limit, as a batch of their own
  std::vector<size_t> on_device;
  for (size_t k = 0; k < P; ++k)
    if (pk.entry_off[k + 1] - pk.entry_off[k] <= OSH_MAPPOINT_MAX_DESCRIPTORS) on_device.push_back(k);
  std::vector<osh::MpOut> out(P);
  std::vector<uint8_t> done(P, 0);
  if (!on_device.empty()) {
    osh_mappoint_batch b;
    pk.fill(b);
    MapPointRefreshPack sub;   // only when a point is over the limit: offsets, positions and per-point values of the others
    if (on_device.size() != P) {
      sub.entry_off.assign(1, 0);
      for (const size_t k : on_device) {
        const int e0 = pk.entry_off[k], e1 = pk.entry_off[k + 1];
        sub.desc.insert(sub.desc.end(), pk.desc.begin() + 32 * (size_t)e0, pk.desc.begin() + 32 * (size_t)e1);
        sub.centre.insert(sub.centre.end(), pk.centre.begin() + e0, pk.centre.begin() + e1);
        sub.use_desc.insert(sub.use_desc.end(), pk.use_desc.begin() + e0, pk.use_desc.begin() + e1);
        sub.entry_off.push_back((int32_t)sub.centre.size());
        sub.pos.insert(sub.pos.end(), pk.pos.begin() + 3 * k, pk.pos.begin() + 3 * k + 3);
        sub.ref_centre.push_back(pk.ref_centre[k]); sub.level_scale.push_back(pk.level_scale[k]); sub.top_scale.push_back(pk.top_scale[k]);
        sub.points.push_back(pk.points[k]);
      }
      sub.centres = pk.centres;
      sub.fill(b);
    }
    const size_t n = on_device.size();
    std::vector<int32_t> best_entry(n), best_median(n);
    std::vector<float> normal(3 * n), min_distance(n), max_distance(n);
    const osh_mappoint_result r{best_entry.data(), best_median.data(), normal.data(), min_distance.data(), max_distance.data()};
    osh_orb_ctx* ctx = HostMatcherContext();
    if (ctx && osh_orb_refresh_map_points(ctx, 1, &b, &r) == OSH_OK) {
      for (size_t i = 0; i < n; ++i) {
        osh::MpOut& o = out[on_device[i]];
        o.best_entry = best_entry[i]; o.best_median = best_median[i];
        o.normal[0] = normal[3 * i]; o.normal[1] = normal[3 * i + 1]; o.normal[2] = normal[3 * i + 2];
        o.min_distance = min_distance[i]; o.max_distance = max_distance[i];
        done[on_device[i]] = 1;
      }
    } else {
      std::fprintf(stderr, "MapPoint::RefreshBatch: %s; the list is computed on the host\n", osh_last_error());
    }
  }
  std::vector<uint16_t> table;
  for (size_t k = 0; k < P; ++k)
    if (!done[k]) RefreshOnHost(pk, k, table, out[k]);

  // write-back, one occurrence after another (src/MapPoint.cc:399-402,488-493)
  for (size_t k = 0; k < P; ++k) {
    MapPoint* pMP = pk.points[k];
    const osh::MpOut& o = out[k];
    const int e0 = pk.entry_off[k], n = pk.entry_off[k + 1] - e0;
    if (n == 0) continue;   // observations without an index: nothing to apply
#ifdef ORBSLAM3_HIP_USE_REAL_HEADERS
    std::unique_lock<std::mutex> lock1(pMP->mMutexFeatures);
    std::unique_lock<std::mutex> lock2(pMP->mMutexPos);
#endif
    if (o.best_entry >= 0) {
      const std::pair<KeyFrame*, int>& row = pk.entry_row[(size_t)e0 + o.best_entry];
      pMP->mDescriptor = row.first->mDescriptors.row(row.second).clone();
    }
    pMP->mfMaxDistance = o.max_distance;
    pMP->mfMinDistance = o.min_distance;
    pMP->mNormalVector = Eigen::Vector3f(o.normal[0], o.normal[1], o.normal[2]);
#ifndef ORBSLAM3_HIP_USE_REAL_HEADERS
    ++pMP->mnDescriptorUpdates; ++pMP->mnNormalUpdates;   // the stand-in's call counters keep their meaning
#endif
  }
}

}  // namespace ORB_SLAM3
