// OptimizerEssentialGraph4DoF.cc -- drop-in ORB_SLAM3::Optimizer::OptimizeEssentialGraph4DoF, the pose graph of an inertial loop
// correction (reference src/Optimizer.cc:5300-5596).  The graph walk is restated edge rule by edge rule into an osh_pgo4_problem
// (PackEssentialGraph4DoF); optimize(20) runs on the device (csrc/pgo4_device.hip); the write-back is the reference's.
//
// One intended deviation: the reference creates no vertex for a bad keyframe but still adds edges to it and reads its vertex in
// the write-back (a null dereference).  Here edges to a keyframe without a vertex are skipped and bad keyframes are not written.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <map>
#include <mutex>
#include <set>
#include <vector>

#include "Optimizer.h"
#include "host_pack.h"
#include "orbslam3_hip.h"

namespace ORB_SLAM3 {

namespace {

// Eigen's Quaternion::toRotationMatrix, row-major
void QuatToR(const Eigen::Quaterniond& q, double R[9]) {
  const double x = q.x(), y = q.y(), z = q.z(), w = q.w();
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
  R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}

// Eigen's Quaterniond(const Matrix3d&) (no normalisation)
Eigen::Quaterniond RToQuat(const double* R) {
  double q[4];   // x y z w
  const double tr = R[0] + R[4] + R[8];
  if (tr > 0.0) {
    double t = std::sqrt(tr + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (R[7] - R[5]) * t; q[1] = (R[2] - R[6]) * t; q[2] = (R[3] - R[1]) * t;
  } else {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[i * 4]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    double t = std::sqrt(R[i * 4] - R[j * 4] - R[k * 4] + 1.0);
    q[i] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (R[k * 3 + j] - R[j * 3 + k]) * t;
    q[j] = (R[j * 3 + i] + R[i * 3 + j]) * t;
    q[k] = (R[k * 3 + i] + R[i * 3 + k]) * t;
  }
  return Eigen::Quaterniond(q[3], q[0], q[1], q[2]);
}

void PutM3f(const Eigen::Matrix3f& M, std::vector<double>& out) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) out.push_back((double)M(r, c));
}
void PutV3f(const Eigen::Vector3f& v, std::vector<double>& out) {
  for (int r = 0; r < 3; ++r) out.push_back((double)v(r));
}

struct Vertex4 {
  KeyFrame* kf;
  double Rwb[9], twb[3], Rcw[9], tcw[3], Rcb[9], tcb[3];
  bool fixed;
};

// Edge4DoF with vertex 0 = keyframe id i, vertex 1 = keyframe id j, Tij from Sij; an edge to a keyframe without a vertex is skipped
void AddEdge4(Pgo4Pack& pk, unsigned long i, unsigned long j, const g2o::Sim3& Sij) {
  if (i >= pk.vertexOfId.size() || j >= pk.vertexOfId.size()) return;
  const int vi = pk.vertexOfId[i], vj = pk.vertexOfId[j];
  if (vi < 0 || vj < 0) return;
  pk.edge_ij.push_back(vi);
  pk.edge_ij.push_back(vj);
  double R[9];
  QuatToR(Sij.rotation(), R);
  pk.dR.insert(pk.dR.end(), R, R + 9);
  for (int k = 0; k < 3; ++k) pk.dt.push_back(Sij.translation()(k));
}

}  // namespace

// src/Optimizer.cc:5300-5470
void PackEssentialGraph4DoF(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const LoopClosing::KeyFrameAndPose& NonCorrectedSim3,
                            const LoopClosing::KeyFrameAndPose& CorrectedSim3,
                            const std::map<KeyFrame*, std::set<KeyFrame*>>& LoopConnections, Pgo4Pack& pk) {
  pk = Pgo4Pack();
  const std::vector<KeyFrame*> vpKFs = pMap->GetAllKeyFrames();
  const unsigned int nMaxKFid = pMap->GetMaxKFid();
  pk.vScw.assign(nMaxKFid + 1, g2o::Sim3());
  const int minFeat = 100;
  // KeyFrame vertices (:5329-5368): ImuCamPose(Rwc, twc, pKF) from CorrectedSim3, else ImuCamPose(pKF)
  std::vector<Vertex4> vv;
  for (KeyFrame* pKF : vpKFs) {
    if (pKF->isBad()) continue;
    const int nIDi = pKF->mnId;
    Vertex4 x;
    x.kf = pKF;
    x.fixed = pKF == pLoopKF;
    const Eigen::Matrix3f Rcbf = pKF->mImuCalib.mTcb.rotationMatrix();
    const Eigen::Vector3f tcbf = pKF->mImuCalib.mTcb.translation();
    for (int k = 0; k < 9; ++k) x.Rcb[k] = (double)Rcbf(k / 3, k % 3);
    for (int k = 0; k < 3; ++k) x.tcb[k] = (double)tcbf(k);
    const auto it = CorrectedSim3.find(pKF);
    if (it != CorrectedSim3.end()) {
      pk.vScw[nIDi] = it->second;
      const g2o::Sim3 Swc = it->second.inverse();
      double Rwc[9];
      QuatToR(Swc.rotation(), Rwc);
      const Eigen::Vector3d twc = Swc.translation();
      for (int r = 0; r < 3; ++r) {
        x.twb[r] = Rwc[3 * r] * x.tcb[0] + Rwc[3 * r + 1] * x.tcb[1] + Rwc[3 * r + 2] * x.tcb[2] + twc(r);
        for (int c = 0; c < 3; ++c) {
          x.Rwb[3 * r + c] = Rwc[3 * r] * x.Rcb[c] + Rwc[3 * r + 1] * x.Rcb[3 + c] + Rwc[3 * r + 2] * x.Rcb[6 + c];
          x.Rcw[3 * r + c] = Rwc[3 * c + r];
        }
      }
      for (int r = 0; r < 3; ++r) x.tcw[r] = -x.Rcw[3 * r] * twc(0) + -x.Rcw[3 * r + 1] * twc(1) + -x.Rcw[3 * r + 2] * twc(2);
    } else {
      pk.vScw[nIDi] = Sim3FromPose(pKF->GetPose());
      const Eigen::Vector3f twb = pKF->GetImuPosition(), tcw = pKF->GetTranslation();
      const Eigen::Matrix3f Rwb = pKF->GetImuRotation(), Rcw = pKF->GetRotation();
      for (int k = 0; k < 9; ++k) { x.Rwb[k] = (double)Rwb(k / 3, k % 3); x.Rcw[k] = (double)Rcw(k / 3, k % 3); }
      for (int k = 0; k < 3; ++k) { x.twb[k] = (double)twb(k); x.tcw[k] = (double)tcw(k); }
    }
    vv.push_back(x);
  }
  // vertices in keyframe-id order (g2o's index mapping; the order the device factors the system in)
  std::stable_sort(vv.begin(), vv.end(), [](const Vertex4& a, const Vertex4& b) { return a.kf->mnId < b.kf->mnId; });
  pk.vertexOfId.assign(nMaxKFid + 1, -1);
  for (const Vertex4& x : vv) {
    if (pk.vertexOfId[x.kf->mnId] >= 0) continue;
    pk.vertexOfId[x.kf->mnId] = (int)pk.vpVertexKF.size();
    pk.vpVertexKF.push_back(x.kf);
    pk.Rwb.insert(pk.Rwb.end(), x.Rwb, x.Rwb + 9); pk.twb.insert(pk.twb.end(), x.twb, x.twb + 3);
    pk.Rcw.insert(pk.Rcw.end(), x.Rcw, x.Rcw + 9); pk.tcw.insert(pk.tcw.end(), x.tcw, x.tcw + 3);
    pk.Rcb.insert(pk.Rcb.end(), x.Rcb, x.Rcb + 9); pk.tcb.insert(pk.tcb.end(), x.tcb, x.tcb + 3);
    pk.fixed.push_back(x.fixed ? 1 : 0);
    if (!x.fixed) ++pk.nFree;
  }
  auto nonCorrectedOr = [&](KeyFrame* pKF) { const auto it = NonCorrectedSim3.find(pKF); return it != NonCorrectedSim3.end() ? it->second : pk.vScw[pKF->mnId]; };
  std::set<std::pair<long unsigned int, long unsigned int>> sInsertedEdges;
  // loop edges (:5377-5406); the weight rule does not apply to the (pCurKF, pLoopKF) pair
  for (const auto& kv : LoopConnections) {
    KeyFrame* pKF = kv.first;
    const long unsigned int nIDi = pKF->mnId;
    const g2o::Sim3 Siw = pk.vScw[nIDi];
    for (KeyFrame* pKFj : kv.second) {
      const long unsigned int nIDj = pKFj->mnId;
      if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(pKFj) < minFeat) continue;
      AddEdge4(pk, nIDi, nIDj, Siw * pk.vScw[nIDj].inverse());
      sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
    }
  }
  // normal edges (:5408-5536); the spanning-tree edge is dead code there (pParentKF is NULL)
  for (KeyFrame* pKF : vpKFs) {
    const int nIDi = pKF->mnId;
    const g2o::Sim3 Siw = nonCorrectedOr(pKF);
    KeyFrame* prevKF = pKF->mPrevKF;
    if (prevKF) AddEdge4(pk, nIDi, prevKF->mnId, Siw * nonCorrectedOr(prevKF).inverse());
    const std::set<KeyFrame*> sLoopEdges = pKF->GetLoopEdges();
    for (KeyFrame* pLKF : sLoopEdges)
      if (pLKF->mnId < pKF->mnId) AddEdge4(pk, nIDi, pLKF->mnId, Siw * nonCorrectedOr(pLKF).inverse());
    const std::vector<KeyFrame*> vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);
    for (KeyFrame* pKFn : vpConnectedKFs) {
      if (pKFn && pKFn != prevKF && pKFn != pKF->mNextKF && !pKF->hasChild(pKFn) && !sLoopEdges.count(pKFn)) {
        if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
          if (sInsertedEdges.count(std::make_pair(std::min(pKF->mnId, pKFn->mnId), std::max(pKF->mnId, pKFn->mnId)))) continue;
          AddEdge4(pk, nIDi, pKFn->mnId, Siw * nonCorrectedOr(pKFn).inverse());
        }
      }
    }
  }
}

void Optimizer::OptimizeEssentialGraph4DoF(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const LoopClosing::KeyFrameAndPose& NonCorrectedSim3,
                                           const LoopClosing::KeyFrameAndPose& CorrectedSim3,
                                           const std::map<KeyFrame*, std::set<KeyFrame*>>& LoopConnections) {
  Pgo4Pack pk;
  PackEssentialGraph4DoF(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, pk);
  if (pk.nFree > OSH_PGO_MAX_VERTICES) {   // before any device call
    std::fprintf(stderr, "OptimizeEssentialGraph4DoF: %d keyframes to optimise, the MI355X path takes up to %d; map left untouched\n",
                 pk.nFree, OSH_PGO_MAX_VERTICES);
    return;
  }
  osh_lba_ctx* ctx = HostSolverContext();
  if (!ctx) return;
  osh_pgo4_problem prob;
  pk.fill(prob);
  const size_t n = pk.vpVertexKF.size();
  std::vector<double> Rcw(9 * n), tcw(3 * n);
  osh_pgo4_result res;
  res.Rcw = Rcw.data();
  res.tcw = tcw.data();
  res.Rwb = nullptr;
  res.twb = nullptr;
  if (osh_pgo4_solve(ctx, &prob, &res) != OSH_OK) {
    std::fprintf(stderr, "OptimizeEssentialGraph4DoF: device solve refused or failed (%s); map left untouched\n", osh_last_error());
    return;
  }
  const std::vector<KeyFrame*> vpKFs = pMap->GetAllKeyFrames();
  const std::vector<MapPoint*> vpMPs = pMap->GetAllMapPoints();
  std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
  std::vector<g2o::Sim3> vCorrectedSwc(pk.vScw.size());
  // SE3 pose recovering (:5542-5557): CorrectedSiw = Sim3(Rcw, tcw, 1), the pose SE3d(Rcw, tcw) cast to float
  for (KeyFrame* pKFi : vpKFs) {
    const int v = pk.vertexOfId[pKFi->mnId];
    if (v < 0) continue;
    const Eigen::Quaterniond q = RToQuat(&Rcw[9 * (size_t)v]);
    const Eigen::Vector3d ti(tcw[3 * v], tcw[3 * v + 1], tcw[3 * v + 2]);
    const g2o::Sim3 CorrectedSiw(q, ti, 1.);
    vCorrectedSwc[pKFi->mnId] = CorrectedSiw.inverse();
    Eigen::Quaterniond qn = q;
    qn.normalize();   // Sophus' SO3 constructor
    pKFi->SetPose(Sophus::SE3f(qn.cast<float>(), ti.cast<float>()));
  }
  // map points (:5560-5591): through the reference keyframe, Srw = vScw (the corrected Sim3 for a keyframe of CorrectedSim3)
  for (MapPoint* pMP : vpMPs) {
    if (pMP->isBad()) continue;
    const int nIDr = pMP->GetReferenceKeyFrame()->mnId;
    const g2o::Sim3 Srw = pk.vScw[nIDr];
    const g2o::Sim3 correctedSwr = vCorrectedSwc[nIDr];
    const Eigen::Vector3d eigP3Dw = pMP->GetWorldPos().cast<double>();
    const Eigen::Vector3d eigCorrectedP3Dw = correctedSwr.map(Srw.map(eigP3Dw));
    pMP->SetWorldPos(eigCorrectedP3Dw.cast<float>());
    pMP->UpdateNormalAndDepth();
  }
  pMap->IncreaseChangeIndex();
}

}  // namespace ORB_SLAM3
