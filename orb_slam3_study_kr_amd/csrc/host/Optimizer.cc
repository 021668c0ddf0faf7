// Optimizer.cc -- ORB_SLAM3::Optimizer::LocalBundleAdjustment on MI355X.
//
// Host side of the drop-in: walks the KeyFrame/MapPoint graph exactly like the reference
// (src/Optimizer.cc:1116-1498), packs it into the flat arrays of osh_lba_problem, lets the HIP
// path run optimizer.optimize(10) (src/Optimizer.cc:1410-1411) and applies the reference's outlier
// test, observation erasure and write-back (:1413-1497).  No g2o, no Eigen.
#include "Optimizer.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <list>
#include <mutex>
#include <set>

#include "host_pack.h"
#include "orbslam3_hip.h"

namespace ORB_SLAM3 {

namespace {

// One solver context (HIP stream + reusable device buffers) per calling thread, destroyed when the thread exits: the reference
// runs every GlobalBundleAdjustment in a freshly created std::thread (LoopClosing), so a context that outlived its thread would
// leak a stream, pinned memory and the largest device buffers of the process per loop closure.
struct ThreadCtx {
  osh_lba_ctx* ctx = nullptr;
  ~ThreadCtx() { if (ctx) osh_lba_destroy(ctx); }
};

osh_lba_ctx* thread_ctx() {
  static thread_local ThreadCtx holder;
  if (!holder.ctx) {
    const char* dev = std::getenv("ORBSLAM3_HIP_DEVICE");
    if (osh_lba_create(dev ? std::atoi(dev) : 0, &holder.ctx) != OSH_OK) {
      std::fprintf(stderr, "LM-LBA: cannot create the HIP solver context: %s\n", osh_last_error());
      holder.ctx = nullptr;
    }
  }
  return holder.ctx;
}

}  // namespace

osh_lba_ctx* HostSolverContext() { return thread_ctx(); }

// Steps 1-6 of src/Optimizer.cc:1118-1404: select the window and flatten it.
bool PackLocalBA(KeyFrame* pKF, Map* pMap, LbaPack& pk) {
  pk = LbaPack();
  // 1. local keyframes: pKF + its covisibles (:1118-1132)
  pk.lLocalKeyFrames.push_back(pKF);
  pKF->mnBALocalForKF = pKF->mnId;
  Map* pCurrentMap = pKF->GetMap();
  const std::vector<KeyFrame*> vNeighKFs = pKF->GetVectorCovisibleKeyFrames();
  for (KeyFrame* pKFi : vNeighKFs) {
    pKFi->mnBALocalForKF = pKF->mnId;
    if (!pKFi->isBad() && pKFi->GetMap() == pCurrentMap) pk.lLocalKeyFrames.push_back(pKFi);
  }
  // 2. local map points (:1134-1160)
  pk.num_fixedKF = 0;
  for (KeyFrame* pKFi : pk.lLocalKeyFrames) {
    if (pKFi->mnId == pMap->GetInitKFid()) pk.num_fixedKF = 1;
    const std::vector<MapPoint*> vpMPs = pKFi->GetMapPointMatches();
    for (MapPoint* pMP : vpMPs) {
      if (!pMP) continue;
      if (pMP->isBad() || pMP->GetMap() != pCurrentMap) continue;
      if (pMP->mnBALocalForKF != pKF->mnId) {
        pk.lLocalMapPoints.push_back(pMP);
        pMP->mnBALocalForKF = pKF->mnId;
      }
    }
  }
  // 3. fixed keyframes: observers of local points that are not local (:1162-1179)
  for (MapPoint* pMP : pk.lLocalMapPoints) {
    const std::map<KeyFrame*, std::tuple<int, int>> observations = pMP->GetObservations();
    for (const auto& ob : observations) {
      KeyFrame* pKFi = ob.first;
      if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) {
        pKFi->mnBAFixedForKF = pKF->mnId;
        if (!pKFi->isBad() && pKFi->GetMap() == pCurrentMap) pk.lFixedCameras.push_back(pKFi);
      }
    }
  }
  pk.num_fixedKF += (int)pk.lFixedCameras.size();
  if (pk.num_fixedKF == 0) return false;  // caller prints the reference's message and returns (:1182-1186)

  // 4./5. vertices; the map's initial keyframe is a fixed vertex (:1220)
  std::vector<KeyFrame*> vFree, vFixed;
  for (KeyFrame* pKFi : pk.lLocalKeyFrames) (pKFi->mnId == pMap->GetInitKFid() ? vFixed : vFree).push_back(pKFi);
  vFixed.insert(vFixed.end(), pk.lFixedCameras.begin(), pk.lFixedCameras.end());
  const std::map<KeyFrame*, int> poseIndex = pk.set_poses(vFree, vFixed);
  const std::map<MapPoint*, int> pointIndex = pk.set_points(std::vector<MapPoint*>(pk.lLocalMapPoints.begin(), pk.lLocalMapPoints.end()));   // :1286
  // 6. edges in g2o insertion order: landmark list order x observation-map order (:1293-1402)
  for (MapPoint* pMP : pk.lLocalMapPoints) {
    const std::map<KeyFrame*, std::tuple<int, int>> observations = pMP->GetObservations();
    for (const auto& ob : observations) {
      KeyFrame* pKFi = ob.first;
      if (pKFi->isBad() || pKFi->GetMap() != pCurrentMap) continue;
      const int leftIndex = std::get<0>(ob.second);
      if (leftIndex != -1) {
        const cv::KeyPoint& kpUn = pKFi->mvKeysUn[leftIndex];
        const float kp_ur = pKFi->mvuRight[leftIndex];
        const bool stereo = kp_ur >= 0;   // mono if mvuRight < 0 (:1305), stereo otherwise (:1332)
        if (!stereo) {
          // the mono edge projects through pKFi->mpCamera (:1323); the device keeps ONE intrinsics row per keyframe
          if (!pk.mono_camera(pKFi->mpCamera, pKFi->fx, pKFi->fy, pKFi->cx, pKFi->cy)) return true;
        }
        pk.add_edge(poseIndex.at(pKFi), pointIndex.at(pMP), stereo ? OSH_EDGE_STEREO : OSH_EDGE_MONO, kpUn, kp_ur, pKFi->mvInvLevelSigma2[kpUn.octave], pKFi, pMP);
      }
      if (pKFi->mpCamera2 && std::get<1>(ob.second) != -1) {
        // EdgeSE3ProjectXYZToBody (:1365-1399): the right-camera observation, a second edge on the pair's Hessian block
        if (!pk.add_body_edge(pKFi, pMP, std::get<1>(ob.second), poseIndex.at(pKFi), pointIndex.at(pMP))) return true;
      }
    }
  }
  pk.camera_models_ok();
  return true;
}

void Optimizer::LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Map* pMap, int& num_fixedKF, int& num_OptKF,
                                      int& num_MPs, int& num_edges) {
  (void)num_MPs;  // never assigned by the reference
  LbaPack pk;
  const bool haveFixed = PackLocalBA(pKF, pMap, pk);
  num_fixedKF = pk.num_fixedKF;
  if (!haveFixed) {
    std::fprintf(stderr, "LM-LBA: There are 0 fixed KF in the optimizations, LBA aborted\n");
    return;
  }
  Map* pCurrentMap = pKF->GetMap();
  // DEBUG LBA sets (:1209-1210,1225,1242)
  pCurrentMap->msOptKFs.clear();
  pCurrentMap->msFixedKFs.clear();
  for (KeyFrame* pKFi : pk.lLocalKeyFrames) pCurrentMap->msOptKFs.insert(pKFi->mnId);
  for (KeyFrame* pKFi : pk.lFixedCameras) pCurrentMap->msFixedKFs.insert(pKFi->mnId);
  num_OptKF = (int)pk.lLocalKeyFrames.size();
  if (pk.unsupported) {
    std::fprintf(stderr, "LM-LBA: %s is not supported by the MI355X path yet; map left untouched\n", pk.unsupported);
    return;
  }
  num_edges = (int)pk.edge_pose.size();
  if (pbStopFlag && *pbStopFlag) return;  // :1406-1408

  osh_lba_ctx* ctx = thread_ctx();
  if (!ctx) return;  // device error: map stays consistent (SURVEY.md 8b "Errors")
  osh_lba_problem prob;
  pk.fill(prob);
  prob.huber_mono = kHuberMono;
  prob.huber_stereo = kHuberStereo;
  prob.lambda_init = pMap->IsInertial() ? 100.0 : 0.0;  // solver->setUserLambdaInit(100.0) (:1197-1198)
  prob.max_iterations = 10;                             // optimizer.optimize(10) (:1411)
  prob.stop_flag = reinterpret_cast<const volatile unsigned char*>(pbStopFlag);
  LbaOutput out(pk.n_free, pk.vPointMPs.size(), pk.edge_pose.size());
  if (osh_lba_solve(ctx, 1, &prob, &out.res) != OSH_OK) {
    std::fprintf(stderr, "LM-LBA: device solve failed (%s); map left untouched\n", osh_last_error());
    return;
  }

  // 9. outlier observations (:1413-1460): mono edges first, then the right-camera (body) edges, then stereo, each in insertion order
  std::vector<std::pair<KeyFrame*, MapPoint*>> vToErase;
  vToErase.reserve(pk.edge_pose.size());
  for (int pass = 0; pass < 3; ++pass) {
    const int kind = pass == 0 ? OSH_EDGE_MONO : (pass == 1 ? OSH_EDGE_BODY : OSH_EDGE_STEREO);
    const double th = pass == 2 ? 7.815 : 5.991;
    for (size_t e = 0; e < pk.edge_kind.size(); ++e) {
      if (pk.edge_kind[e] != kind) continue;
      MapPoint* pMP = pk.vEdgeMP[e];
      if (pMP->isBad()) continue;
      if (out.chi[e] > th || !out.dep[e]) vToErase.push_back(std::make_pair(pk.vEdgeKF[e], pMP));
    }
  }
  // 10. commit under the map mutex (:1464-1475)
  std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
  EraseObservations(vToErase);
  // 11. recover optimised data (:1477-1497); poses of the map's initial keyframe were fixed and stay as they are
  for (KeyFrame* pKFi : pk.lLocalKeyFrames) {
    const int idx = (int)(std::find(pk.vPoseKFs.begin(), pk.vPoseKFs.end(), pKFi) - pk.vPoseKFs.begin());
    pKFi->SetPose(pk.pose(idx, out.pose.data()));
  }
  for (MapPoint* pMP : pk.lLocalMapPoints) {
    pMP->SetWorldPos(out.point(pk.point_of(pMP)));
    pMP->UpdateNormalAndDepth();
  }
  pMap->IncreaseChangeIndex();
}

}  // namespace ORB_SLAM3
