// kfcull.cc -- the stand-in bodies LocalMapping::KeyFrameCulling and MapPointCulling call (KeyFrame::SetBadFlag,
// MapPoint::SetBadFlag), a stand-in map built from flat arrays for them (osh_host_cull_graph_create), the wrappers that drive the
// two bodies and PackKeyFrameCull on it and read the map back, and osh_host_keyframe_cull_cpu: csrc/keyframe_cull.h, the statements
// of k_keyframe_cull_count, on the host in one thread (include/orbslam3_hip_host.h).  Test library only.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../keyframe_cull.h"
#include "LocalMapping.h"
#include "host_graph.h"
#include "host_pack.h"
#include "orbslam3_hip.h"
#include "orbslam3_hip_host.h"

namespace ORB_SLAM3 {

// src/KeyFrame.cc:573-680: nothing for the map's initial keyframe, mbToBeErased alone under mbNotErase; else every matched point
// loses this observer and the keyframe is bad.  The connection and spanning-tree updates are counted, not performed.
void KeyFrame::SetBadFlag() {
  if (mnId == mpMap->GetInitKFid()) return;
  else if (mbNotErase) { mbToBeErased = true; return; }
  ++mnConnectionErasures;
  for (size_t i = 0; i < mvpMapPoints.size(); i++)
    if (mvpMapPoints[i]) mvpMapPoints[i]->EraseObservation(this);
  ++mnSpanningTreeUpdates;
  mbBad = true;
}

// src/MapPoint.cc:216-240: the point is bad, forgets its observers and leaves their match tables (the map's own list is kept)
void MapPoint::SetBadFlag() {
  std::map<KeyFrame*, std::tuple<int, int>> obs;
  mbBad = true;
  obs = mObservations;
  mObservations.clear();
  for (auto& ob : obs) {
    KeyFrame* pKF = ob.first;
    const int leftIndex = std::get<0>(ob.second), rightIndex = std::get<1>(ob.second);
    if (leftIndex != -1) pKF->EraseMapPointMatch(leftIndex);
    if (rightIndex != -1) pKF->EraseMapPointMatch(rightIndex);
  }
}

}  // namespace ORB_SLAM3

namespace {

bool kf_ok(osh_host_graph* g, int32_t k) { return g && k >= 0 && k < (int)g->kfs.size(); }
bool mp_ok(osh_host_graph* g, int32_t j) { return g && j >= 0 && j < (int)g->mps.size(); }
int kf_index(osh_host_graph* g, KeyFrame* pKF) {
  if (!pKF) return -1;
  for (size_t k = 0; k < g->kfs.size(); ++k) if (g->kfs[k].get() == pKF) return (int)k;
  return -1;
}
int mp_index(osh_host_graph* g, MapPoint* pMP) {
  for (size_t j = 0; j < g->mps.size(); ++j) if (g->mps[j].get() == pMP) return (int)j;
  return -1;
}

}  // namespace

extern "C" osh_host_graph* osh_host_cull_graph_create(const osh_host_cull_scene* sc) {
  if (!sc || sc->n_kf < 0 || sc->n_mp < 0) return nullptr;
  {   // the counts and the points of the slots, before anything is built
    size_t s = 0;
    for (int i = 0; i < sc->n_kf; ++i) {
      const int n = sc->kf_n_slots[i], n_left = sc->kf_n_left[i];
      if (n < 0 || n_left < -1 || n_left > n) return nullptr;
      for (int j = 0; j < n; ++j, ++s)
        if (sc->slot_point[s] < -1 || sc->slot_point[s] >= sc->n_mp) return nullptr;
    }
  }
  osh_host_graph* g = new osh_host_graph();
  g->map.mnInitKFid = (unsigned long)sc->init_kf_id;
  g->map.mnKeyFrames = (unsigned long)sc->keyframes_in_map;
  g->map.mbImuInitialized = sc->imu_initialized != 0;
  g->map.mbIMU_BA2 = sc->inertial_ba2 != 0;
  g->cam.reset(new Pinhole(std::vector<float>{500.f, 500.f, 320.f, 240.f}));
  g->cam2.reset(new Pinhole(std::vector<float>{500.f, 500.f, 320.f, 240.f}));
  g->kf_block.reset(new KfSlot[std::max(sc->n_kf, 1)]);
  for (int j = 0; j < sc->n_mp; ++j) g->mps.emplace_back(new MapPoint((unsigned long)j, Eigen::Vector3f(0.f, 0.f, 1.f), &g->map));
  size_t s0 = 0;
  for (int i = 0; i < sc->n_kf; ++i) {
    std::unique_ptr<KeyFrame, KfDestroy> kf(new (&g->kf_block[i]) KeyFrame((unsigned long)sc->kf_id[i], &g->map));
    const int n = sc->kf_n_slots[i], n_left = sc->kf_n_left[i];
    kf->mpCamera = g->cam.get();
    kf->mpCamera2 = sc->kf_camera2[i] ? g->cam2.get() : nullptr;
    kf->N = n; kf->NLeft = n_left;
    kf->mThDepth = sc->kf_th_depth[i]; kf->mTimeStamp = sc->kf_timestamp[i];
    kf->mbNotErase = sc->kf_not_erase[i] != 0;
    kf->mOwb = Eigen::Vector3f(sc->kf_imu_pos[3 * i], sc->kf_imu_pos[3 * i + 1], sc->kf_imu_pos[3 * i + 2]);
    kf->mvpMapPoints.assign(n, nullptr); kf->mvuRight.assign(n, -1.f); kf->mvDepth.assign(n, -1.f);
    const int n_first = n_left == -1 ? n : n_left;   // the keys of mvKeysUn / mvKeys; the rest are mvKeysRight
    for (int s = 0; s < n; ++s) {
      cv::KeyPoint kp;
      kp.octave = sc->slot_octave[s0 + s];
      if (s < n_first) kf->mvKeysUn.push_back(kp); else kf->mvKeysRight.push_back(kp);
      kf->mvuRight[s] = sc->slot_u_right[s0 + s]; kf->mvDepth[s] = sc->slot_depth[s0 + s];
    }
    kf->mvKeys = kf->mvKeysUn;
    if (sc->kf_has_preint[i]) {
      g->preints.emplace_back(new IMU::Preintegrated(IMU::Bias(), IMU::Calib()));
      kf->mpImuPreintegrated = g->preints.back().get();
    }
    for (int s = 0; s < n; ++s) {
      const int p = sc->slot_point[s0 + s];
      if (p == -1) continue;
      kf->mvpMapPoints[s] = g->mps[p].get();
      g->mps[p]->AddObservation(kf.get(), s);
    }
    s0 += (size_t)n;
    g->kfs.push_back(std::move(kf));
  }
  for (int i = 0; i < sc->n_kf; ++i) {
    KeyFrame* kf = g->kfs[i].get();
    if (sc->kf_prev[i] >= 0 && sc->kf_prev[i] < sc->n_kf) kf->mPrevKF = g->kfs[sc->kf_prev[i]].get();
    if (sc->kf_next[i] >= 0 && sc->kf_next[i] < sc->n_kf) kf->mNextKF = g->kfs[sc->kf_next[i]].get();
    kf->mbBad = sc->kf_bad[i] != 0;
    g->map.mvpKeyFrames.push_back(kf);
    g->map.mnMaxKFid = std::max(g->map.mnMaxKFid, kf->mnId);
    if (kf->mnId == g->map.mnInitKFid) g->map.mpKFinitial = kf;
  }
  for (int j = 0; j < sc->n_mp; ++j) {
    MapPoint* mp = g->mps[j].get();
    if (sc->mp_n_obs[j] >= 0) mp->nObs = sc->mp_n_obs[j];
    mp->mbBad = sc->mp_bad[j] != 0;
    g->map.mvpMapPoints.push_back(mp);
  }
  return g;
}

extern "C" int osh_host_kfcull_pack(osh_host_graph* g, int32_t n, const int32_t* kf, int32_t monocular, int32_t sizes[4], int32_t* table_kf,
                                    int32_t* cand_slot_off, int32_t* slot_point, int32_t* slot_level, int32_t* slot_index, int32_t* point_mp,
                                    int32_t* point_n_obs, uint8_t* point_bad, int32_t* point_obs_off, int32_t* obs_kf, int32_t* obs_level,
                                    int32_t* obs_weight) {
  if (!g || n < 0 || (n && !kf) || !sizes) return -1;
  std::vector<KeyFrame*> list;
  for (int i = 0; i < n; ++i) { if (!kf_ok(g, kf[i])) return -1; list.push_back(g->kfs[kf[i]].get()); }
  KeyFrameCullPack pk;
  PackKeyFrameCull(list, monocular != 0, pk);
  const size_t T = pk.table.size(), S = pk.slot_point.size(), P = pk.points.size(), E = pk.obs_kf.size();
  sizes[0] = (int32_t)T; sizes[1] = (int32_t)S; sizes[2] = (int32_t)P; sizes[3] = (int32_t)E;
  if (table_kf) for (size_t t = 0; t < T; ++t) table_kf[t] = kf_index(g, pk.table[t]);
  if (cand_slot_off) std::memcpy(cand_slot_off, pk.cand_slot_off.data(), ((size_t)n + 1) * 4);
  if (slot_point && S) std::memcpy(slot_point, pk.slot_point.data(), S * 4);
  if (slot_level && S) std::memcpy(slot_level, pk.slot_level.data(), S * 4);
  if (slot_index && S) std::memcpy(slot_index, pk.slot_index.data(), S * 4);
  if (point_mp) for (size_t p = 0; p < P; ++p) point_mp[p] = mp_index(g, pk.points[p]);
  if (point_n_obs && P) std::memcpy(point_n_obs, pk.point_n_obs.data(), P * 4);
  if (point_bad && P) std::memcpy(point_bad, pk.point_bad.data(), P);
  if (point_obs_off) std::memcpy(point_obs_off, pk.point_obs_off.data(), (P + 1) * 4);
  if (obs_kf && E) std::memcpy(obs_kf, pk.obs_kf.data(), E * 4);
  if (obs_level && E) std::memcpy(obs_level, pk.obs_level.data(), E * 4);
  if (obs_weight && E) std::memcpy(obs_weight, pk.obs_weight.data(), E * 4);
  return 0;
}

extern "C" int osh_host_keyframe_cull_cpu(const osh_kfcull_problem* g, int32_t n_removed, const int32_t* removed_kf, int32_t first_candidate,
                                          const osh_kfcull_result* r, double* ms) {
  if (!g || !r || n_removed < 0 || (n_removed && !removed_kf) || first_candidate < 0 || first_candidate > g->n_candidates) return -1;
  const size_t P = (size_t)g->n_points, E = P ? (size_t)g->point_obs_off[P] : 0;
  std::vector<osh::KcPoint> point(P);
  std::vector<uint32_t> obs(E);
  for (size_t p = 0; p < P; ++p) point[p] = osh::KcPoint{g->point_obs_off[p], g->point_obs_off[p + 1] - g->point_obs_off[p], g->point_n_obs[p], (int)g->point_bad[p]};
  for (size_t e = 0; e < E; ++e) obs[e] = osh::kc_obs_word(g->obs_kf[e], g->obs_level[e], g->obs_weight[e]);
  std::vector<uint32_t> mask((size_t)g->n_keyframes / 32 + 1, 0u);
  for (int i = 0; i < n_removed; ++i) {
    if (removed_kf[i] < 0 || removed_kf[i] >= g->n_keyframes) return -1;
    mask[removed_kf[i] >> 5] |= 1u << (removed_kf[i] & 31);
  }
  const osh::KcView v{g->cand_slot_off, g->slot_point, g->slot_level, point.data(), obs.data()};
  const auto t0 = std::chrono::steady_clock::now();
  for (int k = first_candidate; k < g->n_candidates; ++k) {
    int a, b;
    osh::kc_count_candidate(v, mask.data(), k, a, b);
    const int i = k - first_candidate;
    if (r->n_mps) r->n_mps[i] = a;
    if (r->n_redundant) r->n_redundant[i] = b;
    if (r->redundant) r->redundant[i] = (uint8_t)osh::kc_decide(b, a, g->redundant_th);
  }
  if (ms) *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

extern "C" int osh_host_local_mapping_keyframe_culling(osh_host_graph* g, int32_t kf, int32_t monocular, int32_t inertial, int32_t abort_ba,
                                                       int32_t capacity, int32_t* culled, int32_t* n_device_calls) {
  if (!kf_ok(g, kf) || capacity < 0) return -1;
  Atlas atlas;
  atlas.mpCurrentMap = &g->map;
  LocalMapping lm;
  lm.mbMonocular = monocular != 0; lm.mbInertial = inertial != 0; lm.mbAbortBA = abort_ba != 0;
  lm.mpAtlas = &atlas; lm.mpCurrentKeyFrame = g->kfs[kf].get();
  // what the body packs, taken before it runs: the state rule of csrc/keyframe_cull.h is checked against the objects afterwards
  const std::vector<KeyFrame*> list = lm.mpCurrentKeyFrame->GetVectorCovisibleKeyFrames();
  const std::vector<KeyFrame*> cand(list.begin(), list.begin() + std::min<size_t>(list.size(), OSH_KFCULL_MAX_CANDIDATES));
  KeyFrameCullPack pk;
  PackKeyFrameCull(cand, lm.mbMonocular, pk);
  std::vector<uint8_t> was_bad(list.size());
  for (size_t i = 0; i < list.size(); ++i) was_bad[i] = list[i]->isBad() ? 1 : 0;

  lm.KeyFrameCulling();

  if (n_device_calls) *n_device_calls = lm.mnKeyFrameCullDeviceCalls;
  int n = 0;
  std::vector<uint32_t> mask(pk.table.size() / 32 + 1, 0u);
  for (size_t i = 0; i < list.size(); ++i) {
    if (was_bad[i] || !list[i]->isBad()) continue;
    if (std::find(list.begin(), list.begin() + i, list[i]) != list.begin() + i) continue;   // a second occurrence
    if (n < capacity && culled) culled[n] = kf_index(g, list[i]);
    ++n;
    if (i < cand.size()) mask[i >> 5] |= 1u << (i & 31);
    else return -3;   // culled beyond the packed candidates: the check below does not cover it
  }
  for (size_t p = 0; p < pk.points.size(); ++p) {
    int lost = 0;
    for (int e = pk.point_obs_off[p]; e < pk.point_obs_off[p + 1]; ++e)
      if (osh::kc_removed(mask.data(), pk.obs_kf[e])) lost += pk.obs_weight[e];
    int is_mp, is_redundant;
    osh::kc_slot_verdict(pk.point_n_obs[p], pk.point_bad[p], lost, 0, is_mp, is_redundant);
    if (pk.points[p]->Observations() != pk.point_n_obs[p] - lost || pk.points[p]->isBad() != (is_mp == 0)) return -2;
  }
  return n;
}

extern "C" int osh_host_local_mapping_map_point_culling(osh_host_graph* g, int32_t kf, int32_t monocular, int32_t n, const int32_t* mp,
                                                        int32_t capacity, int32_t* remaining) {
  if (!kf_ok(g, kf) || n < 0 || (n && !mp) || capacity < 0) return -1;
  LocalMapping lm;
  lm.mbMonocular = monocular != 0;
  lm.mpCurrentKeyFrame = g->kfs[kf].get();
  for (int i = 0; i < n; ++i) { if (!mp_ok(g, mp[i])) return -1; lm.mlpRecentAddedMapPoints.push_back(g->mps[mp[i]].get()); }
  lm.MapPointCulling();
  int m = 0;
  for (MapPoint* pMP : lm.mlpRecentAddedMapPoints) { if (m < capacity && remaining) remaining[m] = mp_index(g, pMP); ++m; }
  return m;
}

extern "C" int osh_host_mp_set_culling(osh_host_graph* g, int32_t mp, int64_t first_kf_id, int32_t n_visible, int32_t n_found) {
  if (!mp_ok(g, mp)) return -1;
  MapPoint* p = g->mps[mp].get();
  p->mnFirstKFid = (long)first_kf_id; p->mnVisible = n_visible; p->mnFound = n_found;
  return 0;
}

extern "C" int osh_host_kf_cull_state(osh_host_graph* g, int32_t kf, int64_t out[9]) {
  if (!kf_ok(g, kf) || !out) return -1;
  KeyFrame* k = g->kfs[kf].get();
  out[0] = k->isBad() ? 1 : 0; out[1] = k->mbToBeErased ? 1 : 0;
  out[2] = kf_index(g, k->mPrevKF); out[3] = kf_index(g, k->mNextKF);
  out[4] = k->mnBestCovisibleUpdates; out[5] = k->mnConnectionErasures; out[6] = k->mnSpanningTreeUpdates;
  out[7] = -1; out[8] = 0;
  if (k->mpImuPreintegrated) {
    out[8] = k->mpImuPreintegrated->mnMerges;
    for (size_t i = 0; i < g->kfs.size(); ++i)
      if (k->mpImuPreintegrated->mpMergedPrevious && g->kfs[i]->mpImuPreintegrated == k->mpImuPreintegrated->mpMergedPrevious) out[7] = (int64_t)i;
  }
  return 0;
}

extern "C" int osh_host_mp_cull_state(osh_host_graph* g, int32_t mp, int64_t out[3]) {
  if (!mp_ok(g, mp) || !out) return -1;
  MapPoint* p = g->mps[mp].get();
  out[0] = p->Observations(); out[1] = p->isBad() ? 1 : 0; out[2] = (int64_t)p->mObservations.size();
  return 0;
}

// For profiles/keyframe_cull_timing.py.  ms[0]: PackKeyFrameCull for the list.  ms[1]: the counting loop in the reference's shape on
// the same objects, one thread: per candidate and slot a copy of GetObservations() and a walk over the copy with the exit at the
// fourth hit (src/LocalMapping.cc:976-1042, the right key of a rig slot at i - NLeft); totals = the sums of nMPs and
// nRedundantObservations it finds, to compare with the packed counts.
extern "C" int osh_host_kfcull_time(osh_host_graph* g, int32_t n, const int32_t* kf, int32_t monocular, double ms[2], int64_t totals[2]) {
  if (!g || n < 0 || (n && !kf) || !ms || !totals) return -1;
  std::vector<KeyFrame*> list;
  for (int i = 0; i < n; ++i) { if (!kf_ok(g, kf[i])) return -1; list.push_back(g->kfs[kf[i]].get()); }
  auto t0 = std::chrono::steady_clock::now();
  {
    KeyFrameCullPack pk;
    PackKeyFrameCull(list, monocular != 0, pk);
    ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  totals[0] = totals[1] = 0;
  t0 = std::chrono::steady_clock::now();
  for (KeyFrame* pKF : list) {
    if (pKF->mnId == pKF->GetMap()->GetInitKFid() || pKF->isBad()) continue;
    const std::vector<MapPoint*> vpMapPoints = pKF->GetMapPointMatches();
    const int thObs = 3;
    for (size_t i = 0, iend = vpMapPoints.size(); i < iend; i++) {
      MapPoint* pMP = vpMapPoints[i];
      if (!pMP || pMP->isBad()) continue;
      if (!monocular && (pKF->mvDepth[i] > pKF->mThDepth || pKF->mvDepth[i] < 0)) continue;
      totals[0]++;
      if (pMP->Observations() > thObs) {
        const int scaleLevel = (pKF->NLeft == -1) ? pKF->mvKeysUn[i].octave : ((int)i < pKF->NLeft) ? pKF->mvKeys[i].octave : pKF->mvKeysRight[i - pKF->NLeft].octave;
        const std::map<KeyFrame*, std::tuple<int, int>> observations = pMP->GetObservations();
        int nObs = 0;
        for (const auto& ob : observations) {
          KeyFrame* pKFi = ob.first;
          if (pKFi == pKF) continue;
          const int leftIndex = std::get<0>(ob.second), rightIndex = std::get<1>(ob.second);
          int scaleLeveli = -1;
          if (pKFi->NLeft == -1) scaleLeveli = pKFi->mvKeysUn[leftIndex].octave;
          else {
            if (leftIndex != -1) scaleLeveli = pKFi->mvKeys[leftIndex].octave;
            if (rightIndex != -1) {
              const int rightLevel = pKFi->mvKeysRight[rightIndex - pKFi->NLeft].octave;
              scaleLeveli = (scaleLeveli == -1 || scaleLeveli > rightLevel) ? rightLevel : scaleLeveli;
            }
          }
          if (scaleLeveli <= scaleLevel + 1) {
            nObs++;
            if (nObs > thObs) break;
          }
        }
        if (nObs > thObs) totals[1]++;
      }
    }
  }
  ms[1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}
