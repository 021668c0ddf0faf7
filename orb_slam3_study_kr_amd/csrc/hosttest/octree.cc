// octree.cc -- the C wrappers around csrc/orb_octree.h and ORBextractor::DistributeOctTreeDevice (include/orbslam3_hip_host.h):
// osh_host_orb_octree_cpu, the host build of the rule on one thread (what tests/test_octree_cpu.py pins to the numpy restatement and
// the CPU baseline of profiles/extract_timing.py), and osh_host_orbextractor_distribute_device.  Test library only.
#include <chrono>
#include <cstdint>
#include <vector>

#include "ORBextractor.h"
#include "../orb_octree.h"
#include "orbslam3_hip.h"
#include "orbslam3_hip_host.h"

extern "C" int osh_host_orb_octree_cpu(int32_t n_lists, const osh_octree_list* lists, osh_octree_result* results, double* ms) {
  if (n_lists < 0 || (n_lists && (!lists || !results))) return OSH_ERR_INVALID;
  for (int k = 0; k < n_lists; ++k) {
    const osh_octree_list& l = lists[k];
    const char* why = "";
    const int rc = osh::oct_validate_list(l.n, l.xy, l.response, l.width, l.height, l.n_features, &why);
    if (rc != osh::kOctOk) return rc;
    if (results[k].capacity < 0 || (results[k].capacity && !results[k].index)) return OSH_ERR_INVALID;
  }
  const auto t0 = std::chrono::steady_clock::now();
  int rc = OSH_OK;
  std::vector<int> kept;
  for (int k = 0; k < n_lists; ++k) {
    const osh_octree_list& l = lists[k];
    osh_octree_result& r = results[k];
    r.status = osh::octree_distribute_host(l.n, l.xy, l.response, l.width, l.height, l.n_features, kept);
    r.n_out = r.status == OSH_OK ? (int32_t)kept.size() : 0;
    if (r.status != OSH_OK && rc == OSH_OK) rc = r.status;
    if (r.status != OSH_OK || r.n_out > r.capacity) continue;
    for (int i = 0; i < r.n_out; ++i) r.index[i] = kept[i];
  }
  if (ms) *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

extern "C" int osh_host_orbextractor_distribute_device(const osh_octree_list* list, int32_t capacity, int32_t* index, float* xy, float* response,
                                                       int32_t* distribute_calls) {
  if (!list || list->n < 0 || (list->n && (!list->xy || !list->response)) || capacity < 0 || (capacity && !index) || !distribute_calls) return -1;
  ORB_SLAM3::ORBextractor ex(1000, 1.2f, 1, 20, 7);
  std::vector<cv::KeyPoint> keys((size_t)list->n);
  for (int k = 0; k < list->n; ++k) {
    cv::KeyPoint& c = keys[k];
    c.pt.x = list->xy[2 * k]; c.pt.y = list->xy[2 * k + 1]; c.response = list->response[k];
    c.size = 7.f; c.angle = -1.f; c.octave = 0; c.class_id = k;
  }
  const std::vector<cv::KeyPoint> kept = ex.DistributeOctTreeDevice(keys, 16, 16 + list->width, 16, 16 + list->height, list->n_features, 0);
  *distribute_calls = (int32_t)ex.mvDistributeCalls.size();
  for (size_t i = 0; i < kept.size() && i < (size_t)capacity; ++i) {
    index[i] = kept[i].class_id;
    if (xy) { xy[2 * i] = kept[i].pt.x; xy[2 * i + 1] = kept[i].pt.y; }
    if (response) response[i] = kept[i].response;
  }
  return (int)kept.size();
}
