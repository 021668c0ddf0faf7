// OptimizerEssentialGraph.cc -- drop-in ORB_SLAM3::Optimizer::OptimizeEssentialGraph, both Sim3 overloads
// (reference src/Optimizer.cc:1501-1784 and :1786-2117).  The graph walk is restated edge rule by edge rule into an
// osh_pgo_problem (PackEssentialGraph / PackEssentialGraphMerge); optimize(20) runs on the device (csrc/pgo_device.hip);
// the write-back is the reference's.
#include <algorithm>
#include <cstdio>
#include <iostream>
#include <map>
#include <mutex>
#include <set>
#include <vector>

#include "Optimizer.h"
#include "host_pack.h"
#include "orbslam3_hip.h"

namespace ORB_SLAM3 {

namespace {

void PutSim3(const g2o::Sim3& S, std::vector<double>& out) {
  const Eigen::Quaterniond& q = S.rotation();
  const double v[8] = {q.x(), q.y(), q.z(), q.w(), S.translation()(0), S.translation()(1), S.translation()(2), S.scale()};
  out.insert(out.end(), v, v + 8);
}

g2o::Sim3 GetSim3(const double* v) {
  return g2o::Sim3(Eigen::Quaterniond(v[3], v[0], v[1], v[2]), Eigen::Vector3d(v[4], v[5], v[6]), v[7]);
}

// vertices in keyframe-id order (the order of g2o's index mapping, and the order the device factors the system in)
struct VertexList {
  struct V { KeyFrame* kf; g2o::Sim3 est; bool fixed, fix_scale; };
  std::vector<V> v;
  void add(KeyFrame* kf, const g2o::Sim3& est, bool fixed, bool fix_scale) { v.push_back({kf, est, fixed, fix_scale}); }
  void finish(size_t nIds, PgoPack& pk) {
    std::stable_sort(v.begin(), v.end(), [](const V& a, const V& b) { return a.kf->mnId < b.kf->mnId; });
    pk.vertexOfId.assign(nIds, -1);
    pk.nFree = 0;
    for (const V& x : v) {
      if (pk.vertexOfId[x.kf->mnId] >= 0) continue;   // g2o's addVertex refuses a second vertex with the same id
      pk.vertexOfId[x.kf->mnId] = (int)pk.vpVertexKF.size();
      pk.vpVertexKF.push_back(x.kf);
      PutSim3(x.est, pk.estimate);
      pk.fixed.push_back(x.fixed ? 1 : 0);
      pk.fix_scale.push_back(x.fix_scale ? 1 : 0);
      if (!x.fixed) ++pk.nFree;
    }
  }
};

// EdgeSim3 with vertex 0 = keyframe id i, vertex 1 = keyframe id j; an edge to a keyframe without a vertex is not added
void AddEdge(PgoPack& pk, unsigned long i, unsigned long j, const g2o::Sim3& Sji) {
  if (i >= pk.vertexOfId.size() || j >= pk.vertexOfId.size()) return;
  const int vi = pk.vertexOfId[i], vj = pk.vertexOfId[j];
  if (vi < 0 || vj < 0) return;
  pk.edge_ij.push_back(vi);
  pk.edge_ij.push_back(vj);
  PutSim3(Sji, pk.measurement);
}

// Runs the packed problem; false (map left as it is) when the graph is over the device limits or the device fails.
bool SolvePgo(const char* who, PgoPack& pk, std::vector<double>& out) {
  if (pk.nFree > OSH_PGO_MAX_VERTICES) {   // before any device call
    std::fprintf(stderr, "%s: %d keyframes to optimise, the MI355X path takes up to %d; map left untouched\n", who, pk.nFree,
                 OSH_PGO_MAX_VERTICES);
    return false;
  }
  osh_lba_ctx* ctx = HostSolverContext();
  if (!ctx) return false;
  osh_pgo_problem prob;
  pk.fill(prob);
  out.assign(pk.estimate.size(), 0.0);
  osh_pgo_result res;
  res.estimate = out.data();
  if (osh_pgo_solve(ctx, &prob, &res) != OSH_OK) {
    std::fprintf(stderr, "%s: device solve failed (%s); map left untouched\n", who, osh_last_error());
    return false;
  }
  return true;
}

}  // namespace

// src/Optimizer.cc:1501-1711
void PackEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const LoopClosing::KeyFrameAndPose& NonCorrectedSim3,
                        const LoopClosing::KeyFrameAndPose& CorrectedSim3, const std::map<KeyFrame*, std::set<KeyFrame*>>& LoopConnections,
                        const bool& bFixScale, PgoPack& pk) {
  pk = PgoPack();
  const std::vector<KeyFrame*> vpKFs = pMap->GetAllKeyFrames();
  const unsigned int nMaxKFid = pMap->GetMaxKFid();
  pk.vScw.assign(nMaxKFid + 1, g2o::Sim3());
  pk.vCorrectedSwc.assign(nMaxKFid + 1, g2o::Sim3());
  const int minFeat = 100;
  // KeyFrame vertices (:1533-1570)
  VertexList vl;
  for (KeyFrame* pKF : vpKFs) {
    if (pKF->isBad()) continue;
    const int nIDi = pKF->mnId;
    const auto it = CorrectedSim3.find(pKF);
    if (it != CorrectedSim3.end()) pk.vScw[nIDi] = it->second;
    else pk.vScw[nIDi] = Sim3FromPose(pKF->GetPose());
    vl.add(pKF, pk.vScw[nIDi], pKF->mnId == pMap->GetInitKFid(), bFixScale);
  }
  vl.finish(nMaxKFid + 1, pk);
  auto nonCorrectedOr = [&](KeyFrame* pKF) { const auto it = NonCorrectedSim3.find(pKF); return it != NonCorrectedSim3.end() ? it->second : pk.vScw[pKF->mnId]; };
  std::set<std::pair<long unsigned int, long unsigned int>> sInsertedEdges;
  // loop edges (:1577-1610); the weight rule does not apply to the (pCurKF, pLoopKF) pair
  for (const auto& kv : LoopConnections) {
    KeyFrame* pKF = kv.first;
    const long unsigned int nIDi = pKF->mnId;
    const g2o::Sim3 Swi = pk.vScw[nIDi].inverse();
    for (KeyFrame* pKFj : kv.second) {
      const long unsigned int nIDj = pKFj->mnId;
      if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(pKFj) < minFeat) continue;
      const g2o::Sim3 Sji = pk.vScw[nIDj] * Swi;
      AddEdge(pk, nIDi, nIDj, Sji);
      sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
    }
  }
  // normal edges (:1612-1711)
  for (KeyFrame* pKF : vpKFs) {
    const int nIDi = pKF->mnId;
    const auto iti = NonCorrectedSim3.find(pKF);
    const g2o::Sim3 Swi = iti != NonCorrectedSim3.end() ? iti->second.inverse() : pk.vScw[nIDi].inverse();
    KeyFrame* pParentKF = pKF->GetParent();
    // spanning tree edge
    if (pParentKF) AddEdge(pk, nIDi, pParentKF->mnId, nonCorrectedOr(pParentKF) * Swi);
    // loop edges of earlier loop closures, from the newer keyframe only
    for (KeyFrame* pLKF : pKF->GetLoopEdges())
      if (pLKF->mnId < pKF->mnId) AddEdge(pk, nIDi, pLKF->mnId, nonCorrectedOr(pLKF) * Swi);
    // covisibility graph edges
    const std::vector<KeyFrame*> vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);
    for (KeyFrame* pKFn : vpConnectedKFs) {
      if (pKFn && pKFn != pParentKF && !pKF->hasChild(pKFn)) {
        if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
          if (sInsertedEdges.count(std::make_pair(std::min(pKF->mnId, pKFn->mnId), std::max(pKF->mnId, pKFn->mnId)))) continue;
          AddEdge(pk, nIDi, pKFn->mnId, nonCorrectedOr(pKFn) * Swi);
        }
      }
    }
    // inertial edge
    if (pKF->bImu && pKF->mPrevKF) AddEdge(pk, nIDi, pKF->mPrevKF->mnId, nonCorrectedOr(pKF->mPrevKF) * Swi);
  }
}

void Optimizer::OptimizeEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const LoopClosing::KeyFrameAndPose& NonCorrectedSim3,
                                       const LoopClosing::KeyFrameAndPose& CorrectedSim3,
                                       const std::map<KeyFrame*, std::set<KeyFrame*>>& LoopConnections, const bool& bFixScale) {
  PgoPack pk;
  PackEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale, pk);
  std::vector<double> est;
  if (!SolvePgo("OptimizeEssentialGraph", pk, est)) return;
  const std::vector<KeyFrame*> vpKFs = pMap->GetAllKeyFrames();
  const std::vector<MapPoint*> vpMPs = pMap->GetAllMapPoints();
  std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
  // SE3 pose recovering, Sim3 [sR t; 0 1] -> SE3 [R t/s; 0 1] (:1717-1731); the reference reads a vertex for every keyframe of the
  // map, a bad one included (it has none there): bad keyframes are skipped here
  for (KeyFrame* pKFi : vpKFs) {
    const int v = pk.vertexOfId[pKFi->mnId];
    if (v < 0) continue;
    const g2o::Sim3 CorrectedSiw = GetSim3(&est[8 * (size_t)v]);
    pk.vCorrectedSwc[pKFi->mnId] = CorrectedSiw.inverse();
    const double s = CorrectedSiw.scale();
    const Eigen::Vector3f tf = CorrectedSiw.translation().cast<float>();
    const float sf = (float)s;   // Eigen converts the double scalar of `Vector3f / double` to float
    Sophus::SE3f Tiw(CorrectedSiw.rotation().cast<float>(), Eigen::Vector3f(tf(0) / sf, tf(1) / sf, tf(2) / sf));
    pKFi->SetPose(Tiw);
  }
  // map points: to the non-optimised pose of their reference keyframe and back with the optimised one (:1733-1762)
  for (MapPoint* pMP : vpMPs) {
    if (pMP->isBad()) continue;
    int nIDr;
    if (pMP->mnCorrectedByKF == pCurKF->mnId) {
      nIDr = pMP->mnCorrectedReference;
    } else {
      KeyFrame* pRefKF = pMP->GetReferenceKeyFrame();
      nIDr = pRefKF->mnId;
    }
    const g2o::Sim3 Srw = pk.vScw[nIDr];
    const g2o::Sim3 correctedSwr = pk.vCorrectedSwc[nIDr];
    const Eigen::Vector3d eigP3Dw = pMP->GetWorldPos().cast<double>();
    const Eigen::Vector3d eigCorrectedP3Dw = correctedSwr.map(Srw.map(eigP3Dw));
    pMP->SetWorldPos(eigCorrectedP3Dw.cast<float>());
    pMP->UpdateNormalAndDepth();
  }
  pMap->IncreaseChangeIndex();
}

// src/Optimizer.cc:1786-2040
void PackEssentialGraphMerge(KeyFrame* pCurKF, std::vector<KeyFrame*>& vpFixedKFs, std::vector<KeyFrame*>& vpFixedCorrectedKFs,
                             std::vector<KeyFrame*>& vpNonFixedKFs, PgoPack& pk) {
  pk = PgoPack();
  Map* pMap = pCurKF->GetMap();
  unsigned long nIds = pMap->GetMaxKFid() + 1;
  for (const auto* l : {&vpFixedKFs, &vpFixedCorrectedKFs, &vpNonFixedKFs})
    for (KeyFrame* k : *l) nIds = std::max(nIds, k->mnId + 1);   // the reference sizes these by the current map's max id alone
  pk.vScw.assign(nIds, g2o::Sim3());
  pk.vCorrectedSwc.assign(nIds, g2o::Sim3());
  pk.vpGoodPose.assign(nIds, false);
  pk.vpBadPose.assign(nIds, false);
  const int minFeat = 100;
  VertexList vl;
  // fixed keyframes of the merged map: corrected pose = current pose, vScw left at its default (identity) as in the reference
  for (KeyFrame* pKFi : vpFixedKFs) {
    if (pKFi->isBad()) continue;
    const int nIDi = pKFi->mnId;
    const g2o::Sim3 Siw = Sim3FromPose(pKFi->GetPose());
    pk.vCorrectedSwc[nIDi] = Siw.inverse();
    vl.add(pKFi, Siw, true, true);
    pk.vpGoodPose[nIDi] = true;
    pk.vpBadPose[nIDi] = false;
  }
  std::set<unsigned long> sIdKF;
  for (KeyFrame* pKFi : vpFixedCorrectedKFs) {
    if (pKFi->isBad()) continue;
    const int nIDi = pKFi->mnId;
    const g2o::Sim3 Siw = Sim3FromPose(pKFi->GetPose());
    pk.vCorrectedSwc[nIDi] = Siw.inverse();
    pk.vScw[nIDi] = Sim3FromPose(pKFi->mTcwBefMerge);
    vl.add(pKFi, Siw, true, false);
    sIdKF.insert(nIDi);
    pk.vpGoodPose[nIDi] = true;
    pk.vpBadPose[nIDi] = true;
  }
  for (KeyFrame* pKFi : vpNonFixedKFs) {
    if (pKFi->isBad()) continue;
    const int nIDi = pKFi->mnId;
    if (sIdKF.count(nIDi)) continue;   // already added with the corrected merge keyframes
    const g2o::Sim3 Siw = Sim3FromPose(pKFi->GetPose());
    pk.vScw[nIDi] = Siw;
    vl.add(pKFi, Siw, false, false);
    sIdKF.insert(nIDi);
    pk.vpGoodPose[nIDi] = false;
    pk.vpBadPose[nIDi] = true;
  }
  vl.finish(nIds, pk);
  std::vector<KeyFrame*> vpKFs;
  vpKFs.insert(vpKFs.end(), vpFixedKFs.begin(), vpFixedKFs.end());
  vpKFs.insert(vpKFs.end(), vpFixedCorrectedKFs.begin(), vpFixedCorrectedKFs.end());
  vpKFs.insert(vpKFs.end(), vpNonFixedKFs.begin(), vpNonFixedKFs.end());
  const std::set<KeyFrame*> spKFs(vpKFs.begin(), vpKFs.end());
  // the measurement's Sjw: corrected when both poses are good, original when both are bad, no edge otherwise
  auto relation = [&](int nIDi, int nIDj, g2o::Sim3& Sjw) {
    if (pk.vpGoodPose[nIDi] && pk.vpGoodPose[nIDj]) { Sjw = pk.vCorrectedSwc[nIDj].inverse(); return true; }
    if (pk.vpBadPose[nIDi] && pk.vpBadPose[nIDj]) { Sjw = pk.vScw[nIDj]; return true; }
    return false;
  };
  for (KeyFrame* pKFi : vpKFs) {
    const int nIDi = pKFi->mnId;
    // Swi stays the identity (default-constructed) for a keyframe whose pose is not bad, as in the reference: correctedSwi is
    // computed there but never used
    g2o::Sim3 Swi;
    if (pk.vpBadPose[nIDi]) Swi = pk.vScw[nIDi].inverse();
    KeyFrame* pParentKFi = pKFi->GetParent();
    if (pParentKFi && spKFs.find(pParentKFi) != spKFs.end()) {
      g2o::Sim3 Sjw;
      if (relation(nIDi, pParentKFi->mnId, Sjw)) AddEdge(pk, nIDi, pParentKFi->mnId, Sjw * Swi);
    }
    const std::set<KeyFrame*> sLoopEdges = pKFi->GetLoopEdges();
    for (KeyFrame* pLKF : sLoopEdges) {
      if (spKFs.find(pLKF) != spKFs.end() && pLKF->mnId < pKFi->mnId) {
        g2o::Sim3 Slw;
        if (relation(nIDi, pLKF->mnId, Slw)) AddEdge(pk, nIDi, pLKF->mnId, Slw * Swi);
      }
    }
    const std::vector<KeyFrame*> vpConnectedKFs = pKFi->GetCovisiblesByWeight(minFeat);
    for (KeyFrame* pKFn : vpConnectedKFs) {
      if (pKFn && pKFn != pParentKFi && !pKFi->hasChild(pKFn) && !sLoopEdges.count(pKFn) && spKFs.find(pKFn) != spKFs.end()) {
        if (!pKFn->isBad() && pKFn->mnId < pKFi->mnId) {
          g2o::Sim3 Snw = pk.vScw[pKFn->mnId];
          if (relation(nIDi, pKFn->mnId, Snw)) AddEdge(pk, nIDi, pKFn->mnId, Snw * Swi);
        }
      }
    }
  }
}

void Optimizer::OptimizeEssentialGraph(KeyFrame* pCurKF, std::vector<KeyFrame*>& vpFixedKFs, std::vector<KeyFrame*>& vpFixedCorrectedKFs,
                                       std::vector<KeyFrame*>& vpNonFixedKFs, std::vector<MapPoint*>& vpNonCorrectedMPs) {
  PgoPack pk;
  PackEssentialGraphMerge(pCurKF, vpFixedKFs, vpFixedCorrectedKFs, vpNonFixedKFs, pk);
  std::vector<double> est;
  if (!SolvePgo("OptimizeEssentialGraph", pk, est)) return;
  Map* pMap = pCurKF->GetMap();
  std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
  // SE3 pose recovering (:2046-2064)
  for (KeyFrame* pKFi : vpNonFixedKFs) {
    if (pKFi->isBad()) continue;
    const int nIDi = pKFi->mnId;
    const g2o::Sim3 CorrectedSiw = GetSim3(&est[8 * (size_t)pk.vertexOfId[nIDi]]);
    pk.vCorrectedSwc[nIDi] = CorrectedSiw.inverse();
    const double s = CorrectedSiw.scale();
    const Eigen::Vector3d& t = CorrectedSiw.translation();
    const Sophus::SE3d Tiw(CorrectedSiw.rotation(), Eigen::Vector3d(t(0) / s, t(1) / s, t(2) / s));
    pKFi->mTcwBefMerge = pKFi->GetPose();
    pKFi->mTwcBefMerge = pKFi->GetPoseInverse();
    pKFi->SetPose(Tiw.cast<float>());
  }
  // map points through the pose change of their reference keyframe (:2066-2102)
  for (MapPoint* pMPi : vpNonCorrectedMPs) {
    if (pMPi->isBad()) continue;
    KeyFrame* pRefKF = pMPi->GetReferenceKeyFrame();
    while (pRefKF && pRefKF->isBad()) {
      pMPi->EraseObservation(pRefKF);
      KeyFrame* pNext = pMPi->GetReferenceKeyFrame();
      if (pNext == pRefKF) { pRefKF = nullptr; break; }   // no observation left to take over the reference
      pRefKF = pNext;
    }
    if (!pRefKF) continue;   // "MP without a valid reference KF"
    if (pRefKF->mnId < pk.vpBadPose.size() && pk.vpBadPose[pRefKF->mnId]) {
      const Sophus::SE3f TNonCorrectedwr = pRefKF->mTwcBefMerge;
      const Sophus::SE3f Twr = pRefKF->GetPoseInverse();
      const Eigen::Vector3f eigCorrectedP3Dw = Twr * TNonCorrectedwr.inverse() * pMPi->GetWorldPos();
      pMPi->SetWorldPos(eigCorrectedP3Dw);
      pMPi->UpdateNormalAndDepth();
    } else {
      std::cout << "ERROR: MapPoint has a reference KF from another map" << std::endl;
    }
  }
}

}  // namespace ORB_SLAM3
