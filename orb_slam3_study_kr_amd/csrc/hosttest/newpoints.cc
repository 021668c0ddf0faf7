// newpoints.cc -- osh_host_newpoint_triangulate_cpu (include/orbslam3_hip_host.h): csrc/newpoint_triangulate.h, the statements
// k_newpoint_triangulate runs per match, on the host in one thread (the CPU side of tests/test_newpoints_cpu.py and of
// profiles/newpoints_timing.py); osh_host_create_new_map_points drives LocalMapping::CreateNewMapPoints on stand-in keyframes built
// from flat arrays; the stand-in bodies of KeyFrame::UnprojectStereo / ComputeSceneMedianDepth.  Test library only.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "../newpoint_triangulate.h"
#include "LocalMapping.h"
#include "host_pack.h"
#include "orbslam3_hip.h"
#include "orbslam3_hip_host.h"

namespace ORB_SLAM3 {

long unsigned int MapPoint::nNextId = 0;

// src/KeyFrame.cc:755-772
bool KeyFrame::UnprojectStereo(int i, Eigen::Vector3f& x3D) {
  const float z = mvDepth[i];
  if (!(z > 0)) return false;
  const float u = mvKeys[i].pt.x, v = mvKeys[i].pt.y;
  x3D = mTwc * Eigen::Vector3f((u - cx) * z * invfx, (v - cy) * z * invfy, z);
  return true;
}

// src/KeyFrame.cc:774-807: the depth, in this keyframe, of the map point at position (size - 1) / q of the sorted depths
float KeyFrame::ComputeSceneMedianDepth(const int q) {
  if (N == 0) return -1.0;
  std::vector<float> vDepths;
  vDepths.reserve(N);
  const Eigen::Vector3f tcw = mTcw.translation();
  for (int i = 0; i < N; i++) {
    MapPoint* pMP = mvpMapPoints[i];
    if (!pMP) continue;
    const Eigen::Vector3f x3Dw = pMP->GetWorldPos();
    vDepths.push_back(mRcw(2, 0) * x3Dw(0) + (mRcw(2, 1) * x3Dw(1) + mRcw(2, 2) * x3Dw(2)) + tcw(2));
  }
  std::sort(vDepths.begin(), vDepths.end());
  return vDepths[(vDepths.size() - 1) / q];
}

}  // namespace ORB_SLAM3

using namespace ORB_SLAM3;

extern "C" int osh_host_newpoint_triangulate_cpu(int32_t n_segments, const osh_newpoint_segment* segments, const osh_newpoint_result* results,
                                                 double* ms) {
  if (n_segments < 0 || (n_segments && (!segments || !results))) return -1;
  double total = 0;
  for (int k = 0; k < n_segments; ++k) {
    const osh_newpoint_segment& s = segments[k];
    const osh_newpoint_result& r = results[k];
    if (s.n_matches < 0) return -1;
    osh::NpSegment seg;
    osh::np_fill_segment(seg, s, 0);
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < s.n_matches; ++i) {
      osh::NpOut o;
      osh::newpoint_triangulate(seg, osh::np_match_of(s, i), o);
      if (r.stage) r.stage[i] = (uint8_t)o.stage;
      if (r.source) r.source[i] = (uint8_t)o.source;
      if (r.cos_parallax) r.cos_parallax[i] = o.cosp;
      if (r.x3d) { r.x3d[3 * (size_t)i] = o.x3D[0]; r.x3d[3 * (size_t)i + 1] = o.x3D[1]; r.x3d[3 * (size_t)i + 2] = o.x3D[2]; }
    }
    total += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  if (ms) *ms = total;
  return 0;
}

extern "C" int osh_host_create_new_map_points(const osh_host_newpoint_scene* sc, int32_t capacity, int32_t* neighbour, int32_t* idx1, int32_t* idx2,
                                              float* x3d, int32_t* n_obs, int32_t* flags, float* poses) {
  if (!sc || sc->n_kf < 1 || !sc->kf || sc->n_neighbours < 0 || (sc->n_neighbours && !sc->neighbours) || capacity < 0) return -1;
  Map map;
  map.mbIMU_BA2 = sc->inertial_ba2 != 0;
  Atlas atlas;
  atlas.mpCurrentMap = &map;
  Tracking tracker;
  tracker.mState = sc->recently_lost ? Tracking::RECENTLY_LOST : Tracking::OK;
  std::vector<std::unique_ptr<KeyFrame>> kfs;
  std::vector<std::unique_ptr<GeometricCamera>> cams;
  std::vector<std::unique_ptr<MapPoint>> held;
  for (int k = 0; k < sc->n_kf; ++k) {
    const osh_host_newpoint_kf& in = sc->kf[k];
    if (in.n < 0 || in.n_left > in.n || in.n_levels < 1) return -1;
    kfs.emplace_back(new KeyFrame((unsigned long)k, &map));
    KeyFrame& kf = *kfs.back();
    const std::vector<float> p1(in.camera, in.camera + (in.camera_kb8 ? 8 : 4));
    cams.emplace_back(in.camera_kb8 ? static_cast<GeometricCamera*>(new KannalaBrandt8(p1)) : new Pinhole(p1));
    kf.mpCamera = cams.back().get();
    if (in.has_camera2) {
      cams.emplace_back(new KannalaBrandt8(std::vector<float>(in.camera2, in.camera2 + 8)));
      kf.mpCamera2 = cams.back().get();
      kf.mTrl = Sophus::SE3f(Eigen::Quaternionf(in.trl_qt[3], in.trl_qt[0], in.trl_qt[1], in.trl_qt[2]), Eigen::Vector3f(in.trl_qt[4], in.trl_qt[5], in.trl_qt[6]));
    }
    kf.fx = in.camera[0]; kf.fy = in.camera[1]; kf.cx = in.camera[2]; kf.cy = in.camera[3];
    kf.invfx = 1.0f / kf.fx; kf.invfy = 1.0f / kf.fy; kf.mbf = in.mbf; kf.mb = in.mb;
    kf.N = in.n; kf.NLeft = in.n_left < 0 ? -1 : in.n_left;
    kf.mfScaleFactor = in.scale_factor; kf.mnScaleLevels = in.n_levels;
    kf.mvScaleFactors.assign(in.n_levels, 1.0f); kf.mvLevelSigma2.assign(in.n_levels, 1.0f);
    for (int l = 1; l < in.n_levels; ++l) { kf.mvScaleFactors[l] = kf.mvScaleFactors[l - 1] * in.scale_factor; kf.mvLevelSigma2[l] = kf.mvScaleFactors[l] * kf.mvScaleFactors[l]; }
    kf.mDescriptors = cv::Mat(in.n, 32);
    kf.mvpMapPoints.assign(in.n, nullptr);
    kf.mvuRight.assign(in.u_right, in.u_right + in.n);
    kf.mvDepth.assign(in.depth, in.depth + in.n);
    for (int i = 0; i < in.n; ++i) {
      cv::KeyPoint kp;
      kp.pt.x = in.xy[2 * i]; kp.pt.y = in.xy[2 * i + 1]; kp.octave = in.octave[i]; kp.angle = 0.f;
      if (kf.NLeft == -1) { kf.mvKeysUn.push_back(kp); kf.mvKeys.push_back(kp); }
      else if (i < kf.NLeft) kf.mvKeys.push_back(kp);
      else kf.mvKeysRight.push_back(kp);
      std::memcpy(kf.mDescriptors.ptr<uint8_t>(i), in.desc + 32 * (size_t)i, 32);
      if (in.has_mp[i]) {
        held.emplace_back(new MapPoint(1000000ul + held.size(), Eigen::Vector3f(in.mp_pos[3 * i], in.mp_pos[3 * i + 1], in.mp_pos[3 * i + 2]), &map));
        kf.mvpMapPoints[i] = held.back().get();
      }
    }
    for (int a = 0; a < in.n_nodes; ++a)
      kf.mFeatVec[(unsigned)in.node_id[a]] = std::vector<unsigned int>(in.node_feat + in.node_off[a], in.node_feat + in.node_off[a + 1]);
    kf.SetPose(Sophus::SE3f(Eigen::Quaternionf(in.pose_qt[3], in.pose_qt[0], in.pose_qt[1], in.pose_qt[2]), Eigen::Vector3f(in.pose_qt[4], in.pose_qt[5], in.pose_qt[6])));
  }
  for (int k = 0; k < sc->n_kf; ++k) {
    const int p = sc->kf[k].prev;
    if (p >= sc->n_kf) return -1;
    if (p >= 0) kfs[k]->mPrevKF = kfs[p].get();
  }
  KeyFrame* cur = kfs[0].get();
  for (int a = 0; a < sc->n_neighbours; ++a) {
    if (sc->neighbours[a] < 1 || sc->neighbours[a] >= sc->n_kf) return -1;
    cur->mvpOrderedConnectedKeyFrames.push_back(kfs[sc->neighbours[a]].get());
  }
  if (poses)
    for (int k = 0; k < sc->n_kf; ++k) {
      osh_newpoint_pose p[2];
      FillNewPointPose(p[0], kfs[k]->GetPose(), kfs[k]->GetCameraCenter());
      p[1] = p[0];
      if (kfs[k]->mpCamera2) FillNewPointPose(p[1], kfs[k]->GetRightPose(), kfs[k]->GetRightCameraCenter());
      for (int s = 0; s < 2; ++s) {
        float* o = poses + 48 * (size_t)k + 24 * s;
        std::memcpy(o, p[s].Rcw, 36); std::memcpy(o + 9, p[s].tcw, 12); std::memcpy(o + 12, p[s].Rwc, 36); std::memcpy(o + 21, p[s].Ow, 12);
      }
    }
  LocalMapping lm;
  lm.mbMonocular = sc->monocular != 0; lm.mbInertial = sc->inertial != 0; lm.mbFarPoints = sc->far_points != 0; lm.mThFarPoints = sc->th_far_points;
  lm.mpAtlas = &atlas; lm.mpTracker = &tracker; lm.mpCurrentKeyFrame = cur;
  if (sc->new_keyframe_waiting) lm.mlNewKeyFrames.push_back(cur);
  lm.CreateNewMapPoints();
  int n = 0;
  for (MapPoint* pMP : lm.mlpRecentAddedMapPoints) {
    if (n < capacity) {
      KeyFrame* other = nullptr;
      int i1 = -1, i2 = -1, nb = -1, f = 0;
      for (const auto& ob : pMP->GetObservations()) {
        KeyFrame* pKF = ob.first;
        const int left = std::get<0>(ob.second), right = std::get<1>(ob.second);
        if (pKF == cur) continue;
        other = pKF;
        i2 = left != -1 ? left : right;
      }
      for (size_t i = 0; i < cur->mvpMapPoints.size(); ++i) if (cur->mvpMapPoints[i] == pMP) i1 = (int)i;
      if (other) for (int k = 0; k < sc->n_kf; ++k) if (kfs[k].get() == other) nb = k;
      auto names = [&](KeyFrame* pKF, int idx) {
        if (!pKF || idx < 0) return false;
        const std::tuple<int, int> t = pMP->GetIndexInKeyFrame(pKF);
        const bool right = pKF->NLeft != -1 && idx >= pKF->NLeft;
        return right ? (std::get<1>(t) == idx && std::get<0>(t) == -1) : (std::get<0>(t) == idx && std::get<1>(t) == -1);
      };
      if (i1 >= 0) f |= 1;
      if (other && i2 >= 0 && other->mvpMapPoints[i2] == pMP) f |= 2;
      if (names(cur, i1)) f |= 4;
      if (names(other, i2)) f |= 8;
      if (pMP->mnDescriptorUpdates == 1 && pMP->mnNormalUpdates == 1) f |= 16;
      if (std::count(map.mvpMapPoints.begin(), map.mvpMapPoints.end(), pMP) == 1) f |= 32;
      if (pMP->GetReferenceKeyFrame() == cur) f |= 64;
      if (neighbour) neighbour[n] = nb;
      if (idx1) idx1[n] = i1;
      if (idx2) idx2[n] = i2;
      if (x3d) { const Eigen::Vector3f X = pMP->GetWorldPos(); x3d[3 * n] = X(0); x3d[3 * n + 1] = X(1); x3d[3 * n + 2] = X(2); }
      if (n_obs) n_obs[n] = pMP->Observations();
      if (flags) flags[n] = f;
    }
    ++n;
    delete pMP;
  }
  return n;
}
