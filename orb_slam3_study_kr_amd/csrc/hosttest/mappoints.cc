// mappoints.cc -- osh_host_mappoint_refresh_cpu (include/orbslam3_hip_host.h): csrc/mappoint_refresh.h, the statements of
// k_mappoint_wave / k_mappoint_block, on the host in one thread (the CPU side of tests/test_mappoint_refresh_cpu.py and of
// profiles/mappoint_refresh_timing.py); the wrappers that prepare a stand-in graph for the local-mapping steps, drive
// MapPoint::RefreshBatch, LocalMapping::SearchInNeighbors and LocalMapping::ProcessNewKeyFrame on it and read the map back.
// Test library only.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../mappoint_refresh.h"
#include "LocalMapping.h"
#include "ORBmatcher.h"
#include "host_graph.h"
#include "host_pack.h"
#include "orbslam3_hip.h"
#include "orbslam3_hip_host.h"

namespace {

bool kf_ok(osh_host_graph* g, int32_t k) { return g && k >= 0 && k < (int)g->kfs.size(); }
bool mp_ok(osh_host_graph* g, int32_t j) { return g && j >= 0 && j < (int)g->mps.size(); }
int kf_index(osh_host_graph* g, KeyFrame* pKF) {
  for (size_t k = 0; k < g->kfs.size(); ++k) if (g->kfs[k].get() == pKF) return (int)k;
  return -1;
}
int mp_index(osh_host_graph* g, MapPoint* pMP) {
  for (size_t j = 0; j < g->mps.size(); ++j) if (g->mps[j].get() == pMP) return (int)j;
  return -1;
}
// the list a wrapper hands to the product: -1 is a null entry
bool point_list(osh_host_graph* g, int32_t n, const int32_t* mp, std::vector<MapPoint*>& out) {
  if (!g || n < 0 || (n && !mp)) return false;
  for (int i = 0; i < n; ++i) {
    if (mp[i] != -1 && !mp_ok(g, mp[i])) return false;
    out.push_back(mp[i] < 0 ? nullptr : g->mps[mp[i]].get());
  }
  return true;
}
// the slots of a keyframe that hold the point, and the observation taken out of the point without the bookkeeping of
// MapPoint::EraseObservation (no bad flag, no new reference keyframe)
void forget_observation(KeyFrame* kf, MapPoint* mp, bool keep_match) {
  const auto it = mp->mObservations.find(kf);
  if (it == mp->mObservations.end()) return;
  const int idx[2] = {std::get<0>(it->second), std::get<1>(it->second)};
  for (int s = 0; s < 2; ++s) {
    if (idx[s] == -1) continue;
    mp->nObs -= (s == 0 && !kf->mpCamera2 && kf->mvuRight[idx[s]] >= 0) ? 2 : 1;
    if (!keep_match) kf->mvpMapPoints[idx[s]] = nullptr;
  }
  mp->mObservations.erase(it);
}

}  // namespace

extern "C" int osh_host_mappoint_refresh_cpu(int32_t n_batches, const osh_mappoint_batch* batches, const osh_mappoint_result* results, double* ms) {
  if (n_batches < 0 || (n_batches && (!batches || !results))) return -1;
  double total = 0;
  std::vector<uint16_t> table((size_t)OSH_MAPPOINT_MAX_DESCRIPTORS * OSH_MAPPOINT_MAX_DESCRIPTORS);
  for (int b = 0; b < n_batches; ++b) {
    const osh_mappoint_batch& g = batches[b];
    const osh_mappoint_result& r = results[b];
    if (g.n_points < 0) return -1;
    const auto t0 = std::chrono::steady_clock::now();
    for (int p = 0; p < g.n_points; ++p) {
      const int e0 = g.entry_off[p], n = g.entry_off[p + 1] - e0;
      if ((size_t)n * n > table.size()) table.resize((size_t)n * n);
      const osh::MpPoint q{0, n, {g.pos[3 * (size_t)p], g.pos[3 * (size_t)p + 1], g.pos[3 * (size_t)p + 2]}, n ? g.ref_centre[p] : 0, g.level_scale[p], g.top_scale[p]};
      osh::MpOut o;
      osh::mappoint_refresh_point(q, reinterpret_cast<const uint32_t*>(g.desc) + 8 * (size_t)e0, g.centre + e0, g.use_desc + e0, g.centres, table.data(), o);
      if (r.best_entry) r.best_entry[p] = o.best_entry;
      if (r.best_median) r.best_median[p] = o.best_median;
      if (r.normal) { r.normal[3 * (size_t)p] = o.normal[0]; r.normal[3 * (size_t)p + 1] = o.normal[1]; r.normal[3 * (size_t)p + 2] = o.normal[2]; }
      if (r.min_distance) r.min_distance[p] = o.min_distance;
      if (r.max_distance) r.max_distance[p] = o.max_distance;
    }
    total += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  if (ms) *ms = total;
  return 0;
}

extern "C" int osh_host_graph_set_mapping(osh_host_graph* g, float scale_factor, int32_t n_levels, const float bounds[4], float mb,
                                          const int32_t* kf_rows, const uint8_t* desc) {
  if (!g || n_levels < 1 || !bounds || !kf_rows || !desc) return -1;
  size_t row0 = 0;
  for (size_t k = 0; k < g->kfs.size(); ++k) {
    KeyFrame& kf = *g->kfs[k];
    const int rows = (int)kf.mvpMapPoints.size();
    if (kf_rows[k] != rows) return -1;
    kf.N = rows;
    if ((int)kf.mvInvLevelSigma2.size() < n_levels) return -1;
    kf.mfScaleFactor = scale_factor; kf.mfLogScaleFactor = std::log(scale_factor); kf.mnScaleLevels = n_levels;
    kf.mvScaleFactors.assign(n_levels, 1.0f); kf.mvLevelSigma2.assign(n_levels, 1.0f);
    for (int l = 1; l < n_levels; ++l) { kf.mvScaleFactors[l] = kf.mvScaleFactors[l - 1] * scale_factor; kf.mvLevelSigma2[l] = kf.mvScaleFactors[l] * kf.mvScaleFactors[l]; }
    kf.invfx = 1.0f / kf.fx; kf.invfy = 1.0f / kf.fy; kf.mb = mb;
    kf.mvKeys = kf.mvKeysUn;   // the left keypoints of a rig keyframe are read from mvKeys
    kf.mvuRight.resize(rows, -1.f);
    kf.mvDepth.assign(rows, -1.f);
    kf.mDescriptors = cv::Mat(rows, 32);
    for (int i = 0; i < rows; ++i) std::memcpy(kf.mDescriptors.ptr<uint8_t>(i), desc + 32 * (row0 + i), 32);
    row0 += (size_t)rows;
    kf.mnMinX = (int)bounds[0]; kf.mnMinY = (int)bounds[1]; kf.mnMaxX = (int)bounds[2]; kf.mnMaxY = (int)bounds[3];
    kf.mnGridCols = FRAME_GRID_COLS; kf.mnGridRows = FRAME_GRID_ROWS;
    kf.mfGridElementWidthInv = (float)FRAME_GRID_COLS / (bounds[2] - bounds[0]);
    kf.mfGridElementHeightInv = (float)FRAME_GRID_ROWS / (bounds[3] - bounds[1]);
    kf.mGrid.assign(FRAME_GRID_COLS, std::vector<std::vector<size_t>>(FRAME_GRID_ROWS));
    for (size_t i = 0; i < kf.mvKeysUn.size(); ++i) {   // src/Frame.cc:397-417: the left / only camera
      const cv::KeyPoint& kp = kf.mvKeysUn[i];
      const int posX = (int)std::round((kp.pt.x - kf.mnMinX) * kf.mfGridElementWidthInv);
      const int posY = (int)std::round((kp.pt.y - kf.mnMinY) * kf.mfGridElementHeightInv);
      if (posX < 0 || posX >= FRAME_GRID_COLS || posY < 0 || posY >= FRAME_GRID_ROWS) continue;
      kf.mGrid[posX][posY].push_back(i);
    }
  }
  return 0;
}

extern "C" int osh_host_graph_set_ref_kf(osh_host_graph* g, int32_t n, const int32_t* mp, const int32_t* kf) {
  if (!g || n < 0 || (n && (!mp || !kf))) return -1;
  for (int i = 0; i < n; ++i) {
    if (!mp_ok(g, mp[i]) || (kf[i] != -1 && !kf_ok(g, kf[i]))) return -1;
    g->mps[mp[i]]->mpRefKF = kf[i] < 0 ? nullptr : g->kfs[kf[i]].get();
  }
  return 0;
}

extern "C" int osh_host_graph_unlink(osh_host_graph* g, int32_t kf, int32_t mp, int32_t keep_match) {
  if (!kf_ok(g, kf) || !mp_ok(g, mp)) return -1;
  forget_observation(g->kfs[kf].get(), g->mps[mp].get(), keep_match != 0);
  return 0;
}

extern "C" int osh_host_graph_clone_point(osh_host_graph* g, int32_t mp, int64_t new_id, int32_t n_kf, const int32_t* kf) {
  if (!mp_ok(g, mp) || n_kf < 0 || (n_kf && !kf)) return -1;
  MapPoint* src = g->mps[mp].get();
  g->mps.emplace_back(new MapPoint((unsigned long)new_id, src->GetWorldPos(), &g->map));
  MapPoint* dup = g->mps.back().get();
  g->map.mvpMapPoints.push_back(dup);
  for (int a = 0; a < n_kf; ++a) {
    if (!kf_ok(g, kf[a])) return -1;
    KeyFrame* pKF = g->kfs[kf[a]].get();
    const auto it = src->mObservations.find(pKF);
    if (it == src->mObservations.end()) continue;
    const int idx[2] = {std::get<0>(it->second), std::get<1>(it->second)};
    forget_observation(pKF, src, false);
    for (int s = 0; s < 2; ++s)
      if (idx[s] != -1) { pKF->mvpMapPoints[idx[s]] = dup; dup->AddObservation(pKF, idx[s]); }
    if (!dup->mpRefKF) dup->mpRefKF = pKF;
  }
  return (int)g->mps.size() - 1;
}

extern "C" int osh_host_mp_refresh_batch(osh_host_graph* g, int32_t n, const int32_t* mp) {
  std::vector<MapPoint*> list;
  if (!point_list(g, n, mp, list)) return -1;
  MapPoint::RefreshBatch(list);
  return 0;
}

extern "C" int osh_host_mp_refresh_pack(osh_host_graph* g, int32_t n, const int32_t* mp, int32_t sizes[3], int32_t* point_mp, int32_t* entry_off,
                                        int32_t* entry_kf, int32_t* entry_row, uint8_t* desc, int32_t* centre, uint8_t* use_desc, float* centres,
                                        float* pos, int32_t* ref_centre, float* level_scale, float* top_scale) {
  std::vector<MapPoint*> list;
  if (!point_list(g, n, mp, list) || !sizes) return -1;
  MapPointRefreshPack pk;
  PackMapPointRefresh(list, pk);
  const size_t P = pk.points.size(), E = pk.centre.size();
  sizes[0] = (int32_t)P; sizes[1] = (int32_t)E; sizes[2] = (int32_t)(pk.centres.size() / 3);
  if (point_mp) for (size_t k = 0; k < P; ++k) point_mp[k] = mp_index(g, pk.points[k]);
  if (entry_off) std::memcpy(entry_off, pk.entry_off.data(), (P + 1) * 4);
  if (entry_kf) for (size_t e = 0; e < E; ++e) entry_kf[e] = kf_index(g, pk.entry_row[e].first);
  if (entry_row) for (size_t e = 0; e < E; ++e) entry_row[e] = pk.entry_row[e].second;
  if (desc && E) std::memcpy(desc, pk.desc.data(), E * 32);
  if (centre && E) std::memcpy(centre, pk.centre.data(), E * 4);
  if (use_desc && E) std::memcpy(use_desc, pk.use_desc.data(), E);
  if (centres && !pk.centres.empty()) std::memcpy(centres, pk.centres.data(), pk.centres.size() * 4);
  if (pos && P) std::memcpy(pos, pk.pos.data(), P * 12);
  if (ref_centre && P) std::memcpy(ref_centre, pk.ref_centre.data(), P * 4);
  if (level_scale && P) std::memcpy(level_scale, pk.level_scale.data(), P * 4);
  if (top_scale && P) std::memcpy(top_scale, pk.top_scale.data(), P * 4);
  return 0;
}

extern "C" int osh_host_mp_get_refresh(osh_host_graph* g, int32_t mp, uint8_t desc[32], float normal[3], float min_max[2], int32_t counts[2]) {
  if (!mp_ok(g, mp)) return -1;
  MapPoint* p = g->mps[mp].get();
  const bool has = !p->mDescriptor.empty();
  if (desc) { if (has) std::memcpy(desc, p->mDescriptor.ptr<uint8_t>(0), 32); else std::memset(desc, 0, 32); }
  if (normal) { normal[0] = p->mNormalVector(0); normal[1] = p->mNormalVector(1); normal[2] = p->mNormalVector(2); }
  if (min_max) { min_max[0] = p->mfMinDistance; min_max[1] = p->mfMaxDistance; }
  if (counts) { counts[0] = p->mnDescriptorUpdates; counts[1] = p->mnNormalUpdates; }
  return has ? 1 : 0;
}

extern "C" int osh_host_mp_observations(osh_host_graph* g, int32_t mp, int32_t capacity, int32_t* kf, int32_t* left, int32_t* right) {
  if (!mp_ok(g, mp) || capacity < 0) return -1;
  int n = 0;
  for (const auto& ob : g->mps[mp]->mObservations) {   // the order both reference functions walk: by pointer value
    if (n < capacity) {
      if (kf) kf[n] = kf_index(g, ob.first);
      if (left) left[n] = std::get<0>(ob.second);
      if (right) right[n] = std::get<1>(ob.second);
    }
    ++n;
  }
  return n;
}

extern "C" int osh_host_mp_state(osh_host_graph* g, int32_t mp, int64_t out[4]) {
  if (!mp_ok(g, mp) || !out) return -1;
  MapPoint* p = g->mps[mp].get();
  out[0] = p->isBad() ? 1 : 0; out[1] = p->GetReplaced() ? mp_index(g, p->GetReplaced()) : -1;
  out[2] = (int64_t)p->mnFuseCandidateForKF; out[3] = p->GetReferenceKeyFrame() ? kf_index(g, p->GetReferenceKeyFrame()) : -1;
  return 0;
}

extern "C" int osh_host_kf_matches(osh_host_graph* g, int32_t kf, int32_t capacity, int32_t* mp) {
  if (!kf_ok(g, kf) || capacity < 0) return -1;
  const std::vector<MapPoint*>& v = g->kfs[kf]->mvpMapPoints;
  for (size_t i = 0; i < v.size() && (int)i < capacity; ++i) mp[i] = v[i] ? mp_index(g, v[i]) : -1;
  return (int)v.size();
}

extern "C" int osh_host_kf_state(osh_host_graph* g, int32_t kf, int64_t marks[3], float centres[6]) {
  if (!kf_ok(g, kf)) return -1;
  KeyFrame* k = g->kfs[kf].get();
  if (marks) { marks[0] = (int64_t)k->mnFuseTargetForKF; marks[1] = k->mnConnectionUpdates; marks[2] = k->NLeft; }
  if (centres) {
    const Eigen::Vector3f a = k->GetCameraCenter(), b = k->NLeft != -1 ? k->GetRightCameraCenter() : a;
    for (int i = 0; i < 3; ++i) { centres[i] = a(i); centres[3 + i] = b(i); }
  }
  return 0;
}

extern "C" int osh_host_graph_fuse(osh_host_graph* g, int32_t kf, int32_t n, const int32_t* mp, float th, int32_t right) {
  std::vector<MapPoint*> list;
  if (!kf_ok(g, kf) || !point_list(g, n, mp, list)) return -1;
  ORBmatcher matcher;
  return matcher.Fuse(g->kfs[kf].get(), list, th, right != 0);
}

extern "C" int osh_host_local_mapping_search_in_neighbors(osh_host_graph* g, int32_t kf, int32_t monocular, int32_t inertial, int32_t abort_ba) {
  if (!kf_ok(g, kf)) return -1;
  Atlas atlas;
  atlas.mpCurrentMap = &g->map;
  LocalMapping lm;
  lm.mbMonocular = monocular != 0; lm.mbInertial = inertial != 0; lm.mbAbortBA = abort_ba != 0;
  lm.mpAtlas = &atlas; lm.mpCurrentKeyFrame = g->kfs[kf].get();
  lm.SearchInNeighbors();
  return 0;
}

extern "C" int osh_host_local_mapping_process_new_keyframe(osh_host_graph* g, int32_t kf, int32_t capacity, int32_t* recent, int32_t* in_map) {
  if (!kf_ok(g, kf) || capacity < 0) return -1;
  KeyFrame* pKF = g->kfs[kf].get();
  pKF->mBowVec[0u] = 1.0;                      // ComputeBoW (src/KeyFrame.cc:92-102) finds both filled: no vocabulary is needed
  pKF->mFeatVec[0u] = std::vector<unsigned int>();
  Atlas atlas;
  atlas.mpCurrentMap = &g->map;
  LocalMapping lm;
  lm.mpAtlas = &atlas;
  lm.mlNewKeyFrames.push_back(pKF);
  const long before = std::count(g->map.mvpKeyFrames.begin(), g->map.mvpKeyFrames.end(), pKF);
  lm.ProcessNewKeyFrame();
  if (in_map) *in_map = (int32_t)(std::count(g->map.mvpKeyFrames.begin(), g->map.mvpKeyFrames.end(), pKF) - before);
  if (lm.mpCurrentKeyFrame != pKF || !lm.mlNewKeyFrames.empty()) return -1;
  int n = 0;
  for (MapPoint* pMP : lm.mlpRecentAddedMapPoints) { if (n < capacity && recent) recent[n] = mp_index(g, pMP); ++n; }
  return n;
}
