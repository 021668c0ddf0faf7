// host_pack.h -- the flat problems the host layer hands to the device (one struct per solver) and the packing and write-back
// steps the Optimizer:: bodies of csrc/host/ share.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <list>
#include <map>
#include <set>
#include <unordered_map>
#include <vector>
#include "CameraModels/GeometricCamera.h"
#include "Frame.h"
#include "ImuTypes.h"
#include "KeyFrame.h"
#include "LoopClosing.h"
#include "Map.h"
#include "MapPoint.h"
#include "orbslam3_hip.h"

namespace ORB_SLAM3 {
bool InvertDense(int n, const double* A, double* inv);             // Gauss-Jordan, partial pivoting (OptimizerInertial.cc)
void SymmetricEigen(int n, const double* A, double* w, double* V);  // cyclic Jacobi: A = V diag(w) V^T (OptimizerInertial.cc)
void InertialInformation(const Eigen::Matrix<float, 15, 15>& C, double* info81);

// Huber deltas of the reference, each the float constant it declares, widened
inline const double kHuberMono = (double)(float)std::sqrt(5.991);     // const float thHuberMono = sqrt(5.991) (src/Optimizer.cc:1275)
inline const double kHuberStereo = (double)(float)std::sqrt(7.815);   // const float thHuberStereo = sqrt(7.815) (:1276)
inline const double kHuber2D = (double)(float)std::sqrt(5.99);        // const float thHuber2D = sqrt(5.99) (:130, 3625)
inline const double kHuberInertial = std::sqrt(16.92);                // rki->setDelta(sqrt(16.92)) (:2646)

// [qx qy qz qw tx ty tz] of a pose, float members widened to double (src/Optimizer.cc:1217-1218), and back
inline void PoseToQt(const Sophus::SE3f& T, double* qt) {
  const Eigen::Quaterniond q = T.unit_quaternion().cast<double>();
  const Eigen::Vector3d t = T.translation().cast<double>();
  qt[0] = q.x(); qt[1] = q.y(); qt[2] = q.z(); qt[3] = q.w(); qt[4] = t[0]; qt[5] = t[1]; qt[6] = t[2];
}
inline Sophus::SE3f PoseFromQt(const double* qt) {
  return Sophus::SE3f(Eigen::Quaterniond(qt[3], qt[0], qt[1], qt[2]).cast<float>(), Eigen::Vector3d(qt[4], qt[5], qt[6]).cast<float>());
}
// Trl as the 3x4 row-major [R | t] of ImuCamPose (Trl.matrix().cast<double>(), src/G2oTypes.cc:58, 104)
inline void PoseTo3x4(const Sophus::SE3f& T, double* m) {
  const Eigen::Matrix3f R = T.rotationMatrix();
  for (int a = 0; a < 3; ++a) { for (int b = 0; b < 3; ++b) m[a * 4 + b] = (double)R(a, b); m[a * 4 + 3] = (double)T.translation()(a); }
}
inline g2o::Sim3 Sim3FromPose(const Sophus::SE3f& T) {
  const Sophus::SE3d Tcw = T.cast<double>();
  return g2o::Sim3(Tcw.unit_quaternion(), Tcw.translation(), 1.0);
}
// the camera's pinhole part is (fx, fy, cx, cy)
inline bool HasIntrinsics(GeometricCamera* c, float fx, float fy, float cx, float cy) {
  return c->getParameter(0) == fx && c->getParameter(1) == fy && c->getParameter(2) == cx && c->getParameter(3) == cy;
}
inline bool ByMnId(const MapPoint* a, const MapPoint* b) { return a->mnId < b->mnId; }
inline void PushPosition(MapPoint* pMP, std::vector<double>& points) {
  const Eigen::Vector3d X = pMP->GetWorldPos().cast<double>();
  points.push_back(X[0]); points.push_back(X[1]); points.push_back(X[2]);
}
// The 67-float IMU::Preintegrated record of osh_liba_problem / osh_posei_problem: dT, dR, dV, dP, JRg, JVg, JVa, JPg, JPa, b
inline void PackPreintegration(const IMU::Preintegrated* P, float* rec) {
  for (int a = 0; a < OSH_PREINT_FLOATS; ++a) rec[a] = 0.f;
  rec[0] = P->dT;
  for (int a = 0; a < 9; ++a) {
    const int r = a / 3, c = a % 3;
    rec[1 + a] = P->dR(r, c); rec[16 + a] = P->JRg(r, c); rec[25 + a] = P->JVg(r, c); rec[34 + a] = P->JVa(r, c); rec[43 + a] = P->JPg(r, c); rec[52 + a] = P->JPa(r, c);
  }
  for (int a = 0; a < 3; ++a) { rec[10 + a] = P->dV(a); rec[13 + a] = P->dP(a); }
  rec[61] = P->b.bax; rec[62] = P->b.bay; rec[63] = P->b.baz; rec[64] = P->b.bwx; rec[65] = P->b.bwy; rec[66] = P->b.bwz;
}
// the reference's erase step for the selected outlier observations (caller holds mMutexMapUpdate)
inline void EraseObservations(const std::vector<std::pair<KeyFrame*, MapPoint*>>& vToErase) {
  for (const auto& er : vToErase) {
    er.first->EraseMapPointMatch(er.second);
    er.second->EraseObservation(er.first);
  }
}

// Map points and visual edges, as both bundle-adjustment packs carry them
struct VisualPack {
  std::vector<MapPoint*> vPointMPs;                      // ascending id
  std::vector<KeyFrame*> vEdgeKF;                        // per edge, insertion order
  std::vector<MapPoint*> vEdgeMP;
  std::vector<double> points, edge_obs, edge_info;
  std::vector<int32_t> edge_pose, edge_point;
  std::vector<uint8_t> edge_kind;
  const char* unsupported = nullptr;
  bool has_kb8 = false;       // the keyframes' camera is a KannalaBrandt8 (monocular fisheye)
  double kb8[4] = {0, 0, 0, 0};
  bool has_rig = false;       // fisheye stereo rig: right-camera edges through cam2 / trl
  double cam2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  // point vertices in ascending mnId (their Hessian order): vPointMPs and their positions; returns each point's index
  std::map<MapPoint*, int> set_points(std::vector<MapPoint*> vMPs) {
    std::sort(vMPs.begin(), vMPs.end(), ByMnId);
    vPointMPs = std::move(vMPs);
    std::map<MapPoint*, int> index;
    for (size_t j = 0; j < vPointMPs.size(); ++j) {
      index[vPointMPs[j]] = (int)j;
      PushPosition(vPointMPs[j], points);
    }
    return index;
  }
  // index of a point of vPointMPs
  int point_of(MapPoint* pMP) const { return (int)(std::lower_bound(vPointMPs.begin(), vPointMPs.end(), pMP, ByMnId) - vPointMPs.begin()); }
  // one visual edge: keypoint kp of pKF observing pMP (an index already checked by the caller), information invSigma2
  void add_edge(int pose, int point, uint8_t kind, const cv::KeyPoint& kp, float ur, float invSigma2, KeyFrame* pKF, MapPoint* pMP) {
    edge_pose.push_back(pose);
    edge_point.push_back(point);
    edge_kind.push_back(kind);
    edge_obs.push_back(kp.pt.x); edge_obs.push_back(kp.pt.y); edge_obs.push_back(kind == OSH_EDGE_STEREO ? ur : -1.0);
    edge_info.push_back(invSigma2);
    vEdgeKF.push_back(pKF);
    vEdgeMP.push_back(pMP);
  }
  // a fisheye problem is monocular on the device (no rectified-stereo edges next to KannalaBrandt8 ones)
  bool no_stereo_with_kb8(const char* msg) {
    if (has_kb8)
      for (uint8_t k : edge_kind) if (k == OSH_EDGE_STEREO) { unsupported = msg; return false; }
    return true;
  }
};

struct LbaPack : VisualPack {
  std::list<KeyFrame*> lLocalKeyFrames, lFixedCameras;   // same containers / order as src/Optimizer.cc:1119,1163
  std::list<MapPoint*> lLocalMapPoints;                  // :1136
  std::vector<KeyFrame*> vPoseKFs;                       // pose order of the problem: optimisable (ascending id), then fixed
  int n_free = 0, n_fixed = 0, num_fixedKF = 0;
  std::vector<double> pose_qt, pose_cam;
  int n_pinhole_mono = 0;
  double trl[7] = {0, 0, 0, 1, 0, 0, 0};
  // pose vertices: vFree in ascending id (the Hessian order of the non-fixed vertices, g2o/core/sparse_optimizer.cpp:166-190),
  // then vFixed; the estimate (:1217-1218) and the camera row (:1352-1356) of each.  Returns each keyframe's pose index.
  std::map<KeyFrame*, int> set_poses(std::vector<KeyFrame*> vFree, const std::vector<KeyFrame*>& vFixed) {
    std::sort(vFree.begin(), vFree.end(), [](KeyFrame* a, KeyFrame* b) { return a->mnId < b->mnId; });
    vPoseKFs = vFree;
    vPoseKFs.insert(vPoseKFs.end(), vFixed.begin(), vFixed.end());
    n_free = (int)vFree.size();
    n_fixed = (int)vFixed.size();
    std::map<KeyFrame*, int> index;
    for (size_t i = 0; i < vPoseKFs.size(); ++i) {
      KeyFrame* pKF = vPoseKFs[i];
      index[pKF] = (int)i;
      double qt[7];
      PoseToQt(pKF->GetPose(), qt);
      pose_qt.insert(pose_qt.end(), qt, qt + 7);
      const double cam[5] = {pKF->fx, pKF->fy, pKF->cx, pKF->cy, pKF->mbf};
      pose_cam.insert(pose_cam.end(), cam, cam + 5);
    }
    return index;
  }
  // Right camera of a keyframe with a right-camera observation (e->pCamera = pKFi->mpCamera2, e->mTrl = GetRelativePoseTrl(),
  // src/Optimizer.cc:1389-1392): one KannalaBrandt8 model and one Trl shared by the whole window (a rig is rigid).
  bool rig_camera(KeyFrame* pKF) {
    GeometricCamera* cam = pKF->mpCamera2;
    if (!cam || cam->GetType() != GeometricCamera::CAM_FISHEYE) { unsupported = "right camera that is not a KannalaBrandt8"; return false; }
    double c[8], t[7];
    for (int i = 0; i < 8; ++i) c[i] = cam->getParameter(i);
    PoseToQt(pKF->GetRelativePoseTrl(), t);
    if (has_rig) {
      for (int i = 0; i < 8; ++i) if (c[i] != cam2[i]) { unsupported = "keyframes with different right cameras in one window"; return false; }
      for (int i = 0; i < 7; ++i) if (t[i] != trl[i]) { unsupported = "keyframes with different Trl in one window"; return false; }
    }
    has_rig = true;
    for (int i = 0; i < 8; ++i) cam2[i] = c[i];
    for (int i = 0; i < 7; ++i) trl[i] = t[i];
    return true;
  }
  // the right-camera edge of (pKF, pMP): appended right after the pair's left edge, as the reference inserts it
  bool add_body_edge(KeyFrame* pKF, MapPoint* pMP, int rightIndex, int pose, int point) {
    if (!rig_camera(pKF)) return false;
    rightIndex -= pKF->NLeft;                                   // :1369
    if (rightIndex < 0 || rightIndex >= (int)pKF->mvKeysRight.size()) { unsupported = "right-camera index outside mvKeysRight"; return false; }
    const cv::KeyPoint& kp = pKF->mvKeysRight[rightIndex];      // :1372
    add_edge(pose, point, OSH_EDGE_BODY, kp, -1.f, pKF->mvInvLevelSigma2[kp.octave], pKF, pMP);   // :1380-1381
    return true;
  }
  // Camera of a monocular observation (the edge projects through pKF->mpCamera, src/Optimizer.cc:1323): the keyframe's own
  // pinhole model, or one KannalaBrandt8 model shared by the whole window.  Anything else sets `unsupported`.
  bool mono_camera(GeometricCamera* cam, float fx, float fy, float cx, float cy) {
    if (!cam || !HasIntrinsics(cam, fx, fy, cx, cy)) {
      unsupported = "monocular observation through a camera that is not the keyframe's own model";
      return false;
    }
    if (cam->GetType() == GeometricCamera::CAM_PINHOLE) { ++n_pinhole_mono; }
    else if (cam->GetType() == GeometricCamera::CAM_FISHEYE) {
      double k[4];
      for (int i = 0; i < 4; ++i) k[i] = cam->getParameter(4 + i);
      if (has_kb8 && (k[0] != kb8[0] || k[1] != kb8[1] || k[2] != kb8[2] || k[3] != kb8[3])) {
        unsupported = "keyframes with different KannalaBrandt8 coefficients in one window";
        return false;
      }
      has_kb8 = true;
      for (int i = 0; i < 4; ++i) kb8[i] = k[i];
    } else { unsupported = "unknown camera model"; return false; }
    if (has_kb8 && n_pinhole_mono > 0) { unsupported = "pinhole and KannalaBrandt8 monocular observations in one window"; return false; }
    return true;
  }
  bool camera_models_ok() {
    if (!no_stereo_with_kb8("rectified-stereo observation in a KannalaBrandt8 window")) return false;
    if (has_rig && !has_kb8) { unsupported = "right-camera observations without a KannalaBrandt8 left camera"; return false; }
    return true;
  }
  // the pose of vPoseKFs[i] after a solve: optimised for a free one, as packed for a fixed one
  Sophus::SE3f pose(int i, const double* out_pose) const { return PoseFromQt(i < n_free ? &out_pose[(size_t)i * 7] : &pose_qt[(size_t)i * 7]); }
  void fill(osh_lba_problem& p) const {
    p.n_free = n_free; p.n_fixed = n_fixed; p.n_points = (int32_t)vPointMPs.size(); p.n_edges = (int32_t)edge_pose.size();
    p.pose_qt = pose_qt.data(); p.pose_cam = pose_cam.data(); p.points = points.data();
    p.edge_pose = edge_pose.data(); p.edge_point = edge_point.data(); p.edge_kind = edge_kind.data();
    p.edge_obs = edge_obs.data(); p.edge_info = edge_info.data();
    p.huber_mono = p.huber_stereo = 0; p.lambda_init = 0; p.max_iterations = 10; p.stop_flag = nullptr;
    p.kb8 = has_kb8 ? kb8 : nullptr;
    p.cam2 = has_rig ? cam2 : nullptr; p.trl = has_rig ? trl : nullptr;
  }
};
// The result buffers of one osh_lba_solve; no per-edge outputs when n_edges is 0
struct LbaOutput {
  std::vector<double> pose, pts, chi;
  std::vector<uint8_t> dep;
  osh_lba_result res;
  LbaOutput(int n_free, size_t n_points, size_t n_edges) : pose((size_t)n_free * 7), pts(n_points * 3), chi(n_edges), dep(n_edges) {
    res.pose_qt = pose.data(); res.points = pts.data();
    res.edge_chi2 = n_edges ? chi.data() : nullptr; res.edge_depth_pos = n_edges ? dep.data() : nullptr;
  }
  Eigen::Vector3f point(size_t j) const { return Eigen::Vector3d(pts[3 * j], pts[3 * j + 1], pts[3 * j + 2]).cast<float>(); }
};

struct LibaPack : VisualPack {
  std::vector<KeyFrame*> vpOptimizableKFs;              // newest first, as the reference builds it (:2402-2417)
  std::list<KeyFrame*> lFixedKeyFrames;
  std::list<MapPoint*> lLocalMapPoints;
  std::vector<KeyFrame*> vPoseKFs;                       // problem order: temporal (ascending id), fixed predecessor, fixed observers
  int n_opt = 0, n_fixed_imu = 0, n_fixed = 0, opt_it = 10;
  std::vector<double> pose_Rcw, pose_tcw, pose_Rwb, pose_twb, vel, bias_g, bias_a, link_info, link_info_g, link_info_a;
  double Rcb[9], tcb[3], tbc[3], cam[5];
  double trl[12] = {0};
  std::vector<int32_t> link_prev, link_cur;
  std::vector<int32_t> link_bias;   // empty, or per link the keyframe that stores the edge's bias vertices (FullInertialBA with bInit)
  std::vector<uint8_t> link_robust;
  std::vector<float> link_preint;
  // ImuCamPose(KeyFrame*) (src/G2oTypes.cc:25-71) of every keyframe of vPoseKFs, float members widened to double; velocity and
  // biases of the first n_opt + n_fixed_imu; body-camera calibration and camera row of pCalibKF
  void set_states(KeyFrame* pCalibKF) {
    for (size_t i = 0; i < vPoseKFs.size(); ++i) {
      KeyFrame* k = vPoseKFs[i];
      const Eigen::Matrix3f Rcw = k->GetRotation(), Rwb = k->GetImuRotation();
      const Eigen::Vector3f tcw = k->GetTranslation(), twb = k->GetImuPosition();
      for (int a = 0; a < 9; ++a) { pose_Rcw.push_back((double)Rcw(a / 3, a % 3)); pose_Rwb.push_back((double)Rwb(a / 3, a % 3)); }
      for (int a = 0; a < 3; ++a) { pose_tcw.push_back((double)tcw(a)); pose_twb.push_back((double)twb(a)); }
      if ((int)i < n_opt + n_fixed_imu) {
        const Eigen::Vector3f v = k->GetVelocity(), bg = k->GetGyroBias(), ba = k->GetAccBias();
        for (int a = 0; a < 3; ++a) { vel.push_back((double)v(a)); bias_g.push_back((double)bg(a)); bias_a.push_back((double)ba(a)); }
      }
    }
    const IMU::Calib& cal = pCalibKF->mImuCalib;
    const Eigen::Matrix3f R = cal.mTcb.rotationMatrix();
    for (int a = 0; a < 9; ++a) Rcb[a] = (double)R(a / 3, a % 3);
    for (int a = 0; a < 3; ++a) { tcb[a] = (double)cal.mTcb.translation()(a); tbc[a] = (double)cal.mTbc.translation()(a); }
    cam[0] = pCalibKF->fx; cam[1] = pCalibKF->fy; cam[2] = pCalibKF->cx; cam[3] = pCalibKF->cy; cam[4] = pCalibKF->mbf;
  }
  // EdgeInertial + EdgeGyroRW + EdgeAccRW between pKFi->mPrevKF (pose prev) and pKFi (pose cur) (src/Optimizer.cc:523-568,
  // 2600-2667, 4226-4257); the inertial information is scaled by infoScale
  void add_link(KeyFrame* pKFi, int prev, int cur, bool robust, double infoScale) {
    IMU::Preintegrated* P = pKFi->mpImuPreintegrated;
    link_prev.push_back(prev);
    link_cur.push_back(cur);
    float rec[OSH_PREINT_FLOATS];
    PackPreintegration(P, rec);
    link_preint.insert(link_preint.end(), rec, rec + OSH_PREINT_FLOATS);
    double info[81];
    InertialInformation(P->C, info);
    for (double& x : info) x *= infoScale;
    link_info.insert(link_info.end(), info, info + 81);
    link_robust.push_back(robust ? 1 : 0);
    for (int which = 0; which < 2; ++which) {
      double Cb[9], inv[9];
      for (int a = 0; a < 3; ++a) for (int c = 0; c < 3; ++c) Cb[a * 3 + c] = (double)P->C(9 + 3 * which + a, 9 + 3 * which + c);
      InvertDense(3, Cb, inv);
      std::vector<double>& dst = which == 0 ? link_info_g : link_info_a;
      dst.insert(dst.end(), inv, inv + 9);
    }
  }
  // one KannalaBrandt8 per problem (ImuCamPose::Project goes through pKFi->mpCamera, src/G2oTypes.cc:166-171); notOwnModel is the
  // message for a camera whose pinhole part is not cam
  bool note_fisheye(KeyFrame* pKFi, const char* notOwnModel) {
    GeometricCamera* c = pKFi->mpCamera;
    if (!HasIntrinsics(c, (float)cam[0], (float)cam[1], (float)cam[2], (float)cam[3])) { unsupported = notOwnModel; return false; }
    for (int k = 0; k < 4; ++k) {
      if (has_kb8 && kb8[k] != (double)c->getParameter(4 + k)) { unsupported = "keyframes with different KannalaBrandt8 coefficients"; return false; }
      kb8[k] = c->getParameter(4 + k);
    }
    has_kb8 = true;
    return true;
  }
  // the KannalaBrandt8 pair and Trl of a keyframe with a right-camera observation (EdgeMono(1)): one rig per problem
  bool note_rig(KeyFrame* pKFi, const char* notOwnModel) {
    if (pKFi->mpCamera->GetType() != GeometricCamera::CAM_FISHEYE || pKFi->mpCamera2->GetType() != GeometricCamera::CAM_FISHEYE) {
      unsupported = "right-camera observation of a rig that is not a KannalaBrandt8 pair"; return false;
    }
    if (!note_fisheye(pKFi, notOwnModel)) return false;
    double c2[8], T[12];
    for (int k = 0; k < 8; ++k) c2[k] = pKFi->mpCamera2->getParameter(k);
    PoseTo3x4(pKFi->GetRelativePoseTrl(), T);
    if (has_rig) {
      for (int k = 0; k < 8; ++k) if (cam2[k] != c2[k]) { unsupported = "keyframes with different right cameras"; return false; }
      for (int k = 0; k < 12; ++k) if (trl[k] != T[k]) { unsupported = "keyframes with different left-to-right transforms"; return false; }
    }
    std::copy(c2, c2 + 8, cam2); std::copy(T, T + 12, trl);
    has_rig = true;
    return true;
  }
  // keeps the points of `all` (ascending id) that an edge refers to (g2o never activates the others) and renumbers edge_point
  void drop_unobserved_points(const std::vector<MapPoint*>& all) {
    std::vector<int> count(all.size(), 0), remap(all.size(), -1);
    for (int32_t j : edge_point) ++count[j];
    vPointMPs.clear(); points.clear();
    for (size_t j = 0; j < all.size(); ++j)
      if (count[j]) {
        remap[j] = (int)vPointMPs.size();
        vPointMPs.push_back(all[j]);
        PushPosition(all[j], points);
      }
    for (int32_t& j : edge_point) j = remap[j];
  }
  // the pose index is an end of some inertial link
  bool linked(int i) const {
    return std::find(link_prev.begin(), link_prev.end(), i) != link_prev.end() || std::find(link_cur.begin(), link_cur.end(), i) != link_cur.end();
  }
  void fill(osh_liba_problem& p) const {
    p.n_opt = n_opt; p.n_fixed_imu = n_fixed_imu; p.n_fixed = n_fixed;
    p.n_points = (int32_t)vPointMPs.size(); p.n_edges = (int32_t)edge_pose.size(); p.n_links = (int32_t)link_prev.size();
    p.pose_Rcw = pose_Rcw.data(); p.pose_tcw = pose_tcw.data(); p.pose_Rwb = pose_Rwb.data(); p.pose_twb = pose_twb.data();
    p.Rcb = Rcb; p.tcb = tcb; p.tbc = tbc; p.cam = cam; p.vel = vel.data(); p.bias_g = bias_g.data(); p.bias_a = bias_a.data();
    p.points = points.data(); p.edge_pose = edge_pose.data(); p.edge_point = edge_point.data(); p.edge_kind = edge_kind.data();
    p.edge_obs = edge_obs.data(); p.edge_info = edge_info.data(); p.link_prev = link_prev.data(); p.link_cur = link_cur.data();
    p.link_preint = link_preint.data(); p.link_info = link_info.data(); p.link_info_g = link_info_g.data(); p.link_info_a = link_info_a.data();
    p.link_robust = link_robust.data();
    p.huber_mono = p.huber_stereo = p.huber_inertial = 0; p.lambda_init = 1.0; p.max_iterations = opt_it;
    p.kb8 = has_kb8 ? kb8 : nullptr;
    p.cam2 = has_rig ? cam2 : nullptr; p.trl = has_rig ? trl : nullptr;
    p.link_bias = link_bias.empty() ? nullptr : link_bias.data();
  }
};
// The result buffers of one osh_liba_solve and the map types its rows become
struct LibaOutput {
  std::vector<double> Rcw, tcw, Rwb, twb, v, bg, ba, pts, chi;
  std::vector<uint8_t> dep;
  osh_liba_result res;
  LibaOutput(int N, int L, int E) : Rcw((size_t)N * 9), tcw((size_t)N * 3), Rwb((size_t)N * 9), twb((size_t)N * 3), v((size_t)N * 3), bg((size_t)N * 3), ba((size_t)N * 3),
                                    pts((size_t)L * 3), chi(E), dep(E) {
    res.pose_Rcw = Rcw.data(); res.pose_tcw = tcw.data(); res.pose_Rwb = Rwb.data(); res.pose_twb = twb.data();
    res.vel = v.data(); res.bias_g = bg.data(); res.bias_a = ba.data(); res.points = pts.data(); res.edge_chi2 = chi.data(); res.edge_depth_pos = dep.data();
  }
  Sophus::SE3f pose(int i) const {
    Eigen::Matrix3f R; Eigen::Vector3f t;
    for (int a = 0; a < 9; ++a) R(a / 3, a % 3) = (float)Rcw[(size_t)i * 9 + a];
    for (int a = 0; a < 3; ++a) t(a) = (float)tcw[(size_t)i * 3 + a];
    return Sophus::SE3f(R, t);
  }
  Eigen::Vector3f velocity(int i) const { return Eigen::Vector3f((float)v[(size_t)i * 3], (float)v[(size_t)i * 3 + 1], (float)v[(size_t)i * 3 + 2]); }
  IMU::Bias bias(int i) const { return IMU::Bias(ba[(size_t)i * 3], ba[(size_t)i * 3 + 1], ba[(size_t)i * 3 + 2], bg[(size_t)i * 3], bg[(size_t)i * 3 + 1], bg[(size_t)i * 3 + 2]); }
  Eigen::Vector3f point(int j) const { return Eigen::Vector3d(pts[3 * (size_t)j], pts[3 * (size_t)j + 1], pts[3 * (size_t)j + 2]).cast<float>(); }
};
// Flat problem of Optimizer::PoseInertialOptimizationLastKeyFrame (mode 0) / LastFrame (mode 1), src/Optimizer.cc:4499-5299
struct PoseiPack {
  int mode = 0;
  bool rec_init = false;
  const char* unsupported = nullptr;
  int n_mono = 0, n_stereo = 0;                 // nInitialMonoCorrespondences / nInitialStereoCorrespondences
  std::vector<int> index;                       // keypoint of every edge
  std::vector<double> points, edge_obs, edge_info;
  std::vector<uint8_t> edge_kind, edge_close;
  double Rcw[9], tcw[3], Rwb[9], twb[3], vel[3], bias_g[3], bias_a[3];
  double prev_Rwb[9], prev_twb[3], prev_vel[3], prev_bias_g[3], prev_bias_a[3];
  double Rcb[9], tcb[3], tbc[3], cam[5];
  bool has_kb8 = false, has_rig = false;
  double kb8[4] = {0, 0, 0, 0}, cam2[8] = {0, 0, 0, 0, 0, 0, 0, 0}, trl[12] = {0};
  float preint[OSH_PREINT_FLOATS];
  double info_inertial[81], info_g[9], info_a[9];
  double prior_Rwb[9], prior_twb[3], prior_vel[3], prior_bg[3], prior_ba[3], prior_H[225];
  void fill(osh_posei_problem& p) const {
    p.mode = mode; p.n_edges = (int32_t)index.size(); p.rec_init = rec_init ? 1 : 0;
    p.Rcw = Rcw; p.tcw = tcw; p.Rwb = Rwb; p.twb = twb; p.vel = vel; p.bias_g = bias_g; p.bias_a = bias_a;
    p.prev_Rwb = prev_Rwb; p.prev_twb = prev_twb; p.prev_vel = prev_vel; p.prev_bias_g = prev_bias_g; p.prev_bias_a = prev_bias_a;
    p.Rcb = Rcb; p.tcb = tcb; p.tbc = tbc; p.cam = cam;
    p.kb8 = has_kb8 ? kb8 : nullptr; p.cam2 = has_rig ? cam2 : nullptr; p.trl = has_rig ? trl : nullptr;
    p.preint = preint; p.info_inertial = info_inertial; p.info_g = info_g; p.info_a = info_a;
    const bool pr = mode == 1;
    p.prior_Rwb = pr ? prior_Rwb : nullptr; p.prior_twb = pr ? prior_twb : nullptr; p.prior_vel = pr ? prior_vel : nullptr;
    p.prior_bg = pr ? prior_bg : nullptr; p.prior_ba = pr ? prior_ba : nullptr; p.prior_H = pr ? prior_H : nullptr;
    p.points = points.data(); p.edge_kind = edge_kind.data(); p.edge_obs = edge_obs.data(); p.edge_info = edge_info.data();
    p.edge_close = edge_close.data();
    p.huber_mono = kHuberMono;                           // const float thHuberMono = sqrt(5.991) (:4552)
    p.huber_stereo = kHuberStereo;
    p.huber_prior = 5.0;                                 // rkp->setDelta(5) (:5117)
    const float m0[4] = {12.f, 7.5f, 5.991f, 5.991f}, m1[4] = {5.991f, 5.991f, 5.991f, 5.991f}, st[4] = {15.6f, 9.8f, 7.815f, 7.815f};
    for (int k = 0; k < 4; ++k) { p.chi2_mono[k] = mode == 0 ? m0[k] : m1[k]; p.chi2_stereo[k] = st[k]; p.iterations[k] = 10; }   // :4714-4716 / :5121-5123
  }
};
class Frame;
bool PackPoseInertial(Frame* pFrame, bool bRecInit, int mode, PoseiPack& pk);
bool PackLocalInertialBA(KeyFrame* pKF, Map* pMap, bool bLarge, bool bRecInit, LibaPack& pk);
// Optimizer::FullInertialBA / MergeInertialBA as the same flat problem (OptimizerInertialMap.cc).  vpIdle: keyframes no edge touches;
// vpCovKFs: the merge's covisible keyframes in the reference's order
// *sharedBiasSlot: with bInit the keyframe (pose index) whose bias slot holds the one optimised bias pair, else -1
bool PackFullInertialBA(Map* pMap, int its, bool bFixLocal, bool bInit, float priorG, float priorA, LibaPack& pk, std::vector<KeyFrame*>& vpIdle,
                        std::vector<MapPoint*>& vpAllMPs, int* sharedBiasSlot);
bool PackMergeInertialBA(KeyFrame* pCurrKF, KeyFrame* pMergeKF, LibaPack& pk, std::vector<KeyFrame*>& vpCovKFs);
osh_lba_ctx* HostSolverContext();   // one solver context per calling thread (Optimizer.cc)

// Optimizer::OptimizeEssentialGraph as an osh_pgo_problem (OptimizerEssentialGraph.cc): vertices in keyframe-id order, edges in
// the order the reference adds them; vScw / vCorrectedSwc / vpGoodPose / vpBadPose indexed by mnId as there.
struct PgoPack {
  std::vector<KeyFrame*> vpVertexKF;         // keyframe of every vertex
  std::vector<int> vertexOfId;               // mnId -> vertex (-1: none)
  std::vector<double> estimate, measurement; // [n*8], [E*8]
  std::vector<uint8_t> fixed, fix_scale;
  std::vector<int32_t> edge_ij;
  std::vector<g2o::Sim3> vScw, vCorrectedSwc;
  std::vector<bool> vpGoodPose, vpBadPose;   // merge overload only
  int nFree = 0;
  void fill(osh_pgo_problem& p) const {
    p.n_vertices = (int32_t)vpVertexKF.size(); p.estimate = estimate.data(); p.fixed = fixed.data(); p.fix_scale = fix_scale.data();
    p.n_edges = (int32_t)(edge_ij.size() / 2); p.edge_ij = edge_ij.data(); p.measurement = measurement.data();
    p.iterations = 20; p.lambda_init = 1e-16; p.solve_mode = OSH_PGO_SOLVE_ENVELOPE;   // setUserLambdaInit(1e-16), optimize(20)
  }
};
void PackEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const LoopClosing::KeyFrameAndPose& NonCorrectedSim3,
                        const LoopClosing::KeyFrameAndPose& CorrectedSim3, const std::map<KeyFrame*, std::set<KeyFrame*>>& LoopConnections,
                        const bool& bFixScale, PgoPack& pk);
// The 4-DoF graph of Optimizer::OptimizeEssentialGraph4DoF: 3x3 matrices row-major, vertices in keyframe-id order.
struct Pgo4Pack {
  std::vector<KeyFrame*> vpVertexKF;
  std::vector<int> vertexOfId;                               // mnId -> vertex (-1: none)
  std::vector<double> Rwb, twb, Rcw, tcw, Rcb, tcb, dR, dt;  // [n*9], [n*3], ... [E*9], [E*3]
  std::vector<uint8_t> fixed;
  std::vector<int32_t> edge_ij;
  std::vector<g2o::Sim3> vScw;                               // by mnId
  int nFree = 0;
  void fill(osh_pgo4_problem& p) const {
    p.n_vertices = (int32_t)vpVertexKF.size(); p.Rwb = Rwb.data(); p.twb = twb.data(); p.Rcw = Rcw.data(); p.tcw = tcw.data();
    p.Rcb = Rcb.data(); p.tcb = tcb.data(); p.fixed = fixed.data();
    p.n_edges = (int32_t)(edge_ij.size() / 2); p.edge_ij = edge_ij.data(); p.dR = dR.data(); p.dt = dt.data();
    // matLambda of src/Optimizer.cc:5372-5375: (0, 0) is set twice, (2, 2) never
    const double info[6] = {1e3, 1e3, 1.0, 1.0, 1.0, 1.0};
    for (int k = 0; k < 6; ++k) p.info_diag[k] = info[k];
    p.iterations = 20; p.lambda_init = 0.0; p.solve_mode = OSH_PGO_SOLVE_ENVELOPE;   // no setUserLambdaInit: computeLambdaInit
  }
};
void PackEssentialGraph4DoF(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const LoopClosing::KeyFrameAndPose& NonCorrectedSim3,
                            const LoopClosing::KeyFrameAndPose& CorrectedSim3,
                            const std::map<KeyFrame*, std::set<KeyFrame*>>& LoopConnections, Pgo4Pack& pk);
void PackEssentialGraphMerge(KeyFrame* pCurKF, std::vector<KeyFrame*>& vpFixedKFs, std::vector<KeyFrame*>& vpFixedCorrectedKFs,
                             std::vector<KeyFrame*>& vpNonFixedKFs, PgoPack& pk);

// The pairs of Optimizer::OptimizeSim3 (OptimizerSim3.cc): one entry per edge pair in the reference's order, index = i of
// vpMatches1 (vnIndexEdge).  False (with `unsupported`) when a keyframe's camera is neither a Pinhole nor a KannalaBrandt8.
struct Sim3OptPack {
  std::vector<int> index;
  std::vector<double> X1c, X2c, obs1, obs2, info1, info2;
  double cam1[8], cam2[8];
  int32_t kb8_1 = 0, kb8_2 = 0;
  const char* unsupported = nullptr;
  void fill(osh_sim3_problem& p, const g2o::Sim3& S12, float th2, bool bFixScale) const {
    p.n_pairs = (int32_t)index.size();
    const Eigen::Quaterniond& q = S12.rotation();
    const Eigen::Vector3d& t = S12.translation();
    const double S[8] = {q.x(), q.y(), q.z(), q.w(), t(0), t(1), t(2), S12.scale()};
    for (int k = 0; k < 8; ++k) { p.S12[k] = S[k]; p.cam1[k] = cam1[k]; p.cam2[k] = cam2[k]; }
    p.fix_scale = bFixScale ? 1 : 0; p.th2 = th2; p.kb8_1 = kb8_1; p.kb8_2 = kb8_2;
    p.iterations[0] = 5; p.iterations[1] = 10; p.iterations[2] = 5;   // optimize(5), optimize(nBad > 0 ? 10 : 5) (src/Optimizer.cc:2287, :2325-2331)
    p.X1c = X1c.data(); p.X2c = X2c.data(); p.obs1 = obs1.data(); p.obs2 = obs2.data(); p.info1 = info1.data(); p.info2 = info2.data();
  }
};
bool PackOptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatches1, const bool bAllPoints, Sim3OptPack& pk);

// Steps 1-6 of Optimizer::LocalBundleAdjustment; false when the window has no fixed keyframe.
bool PackLocalBA(KeyFrame* pKF, Map* pMap, LbaPack& pk);
// Vertex / edge construction of the welding Optimizer::LocalBundleAdjustment(pMainKF, vpAdjustKF, vpFixedKF, ...) (src/Optimizer.cc:3524-3705);
// vpMPs = the map points of the problem in the reference's insertion order.
void PackWeldingBA(KeyFrame* pMainKF, const std::vector<KeyFrame*>& vpAdjustKF, const std::vector<KeyFrame*>& vpFixedKF, LbaPack& pk,
                   std::vector<MapPoint*>& vpMPs);
// Vertex / edge construction of Optimizer::BundleAdjustment (src/Optimizer.cc:112-300); vbNotIncludedMP as there.
void PackBundleAdjustment(const std::vector<KeyFrame*>& vpKFs, const std::vector<MapPoint*>& vpMP, LbaPack& pk,
                          std::vector<bool>& vbNotIncludedMP);

// The keypoints of a stereo Frame as both stereo entries take them: positions, octaves and descriptor rows copied into flat arrays.
struct KeypointArrays {
  std::vector<float> left_xy, right_xy;
  std::vector<int32_t> left_octave, right_octave;
  std::vector<uint8_t> left_desc, right_desc;
};
// False (with `unsupported`) when the descriptor matrices do not fit the keypoints.
inline bool pack_keypoints(const Frame& F, KeypointArrays& a, const char*& unsupported) {
  const size_t nl = F.mvKeys.size(), nr = F.mvKeysRight.size();
  if ((size_t)F.mDescriptors.rows < nl || (size_t)F.mDescriptorsRight.rows < nr || (nl && F.mDescriptors.cols != 32) || (nr && F.mDescriptorsRight.cols != 32)) {
    unsupported = "descriptor matrices do not match the keypoints"; return false;
  }
  auto keys = [](const std::vector<cv::KeyPoint>& k, const cv::Mat& D, std::vector<float>& xy, std::vector<int32_t>& oct, std::vector<uint8_t>& desc) {
    xy.resize(k.size() * 2); oct.resize(k.size()); desc.resize(k.size() * 32);
    for (size_t i = 0; i < k.size(); ++i) {
      xy[2 * i] = k[i].pt.x; xy[2 * i + 1] = k[i].pt.y; oct[i] = k[i].octave;
      std::copy(D.ptr<uint8_t>((int)i), D.ptr<uint8_t>((int)i) + 32, &desc[32 * i]);
    }
  };
  keys(F.mvKeys, F.mDescriptors, a.left_xy, a.left_octave, a.left_desc);
  keys(F.mvKeysRight, F.mDescriptorsRight, a.right_xy, a.right_octave, a.right_desc);
  return true;
}
// the eight keypoint fields of osh_stereo_frame / osh_fisheye_stereo_frame
template <class FrameStruct>
void fill_keypoints(FrameStruct& f, const KeypointArrays& a) {
  f.n_left = (int32_t)a.left_octave.size(); f.n_right = (int32_t)a.right_octave.size();
  f.left_xy = a.left_xy.data(); f.left_octave = a.left_octave.data(); f.left_desc = a.left_desc.data();
  f.right_xy = a.right_xy.data(); f.right_octave = a.right_octave.data(); f.right_desc = a.right_desc.data();
}

// The frame Frame::ComputeStereoMatches (Frame.cc) hands to osh_orb_stereo_match: the keypoint arrays, and the pyramid levels
// referenced in place through ptr<uchar>(0) and step (a level is a view into a bordered image: its rows are `step` bytes apart,
// never `cols`).  False (with `unsupported`) when the frame's members do not fit together.
struct StereoPack {
  KeypointArrays keys;
  std::vector<osh_stereo_image> left_pyramid, right_pyramid;
  const char* unsupported = nullptr;
  void fill(osh_stereo_frame& f, const Frame& F) const {
    fill_keypoints(f, keys);
    f.n_levels = (int32_t)left_pyramid.size();
    f.scale_factors = F.mvScaleFactors.data(); f.inv_scale_factors = F.mvInvScaleFactors.data();
    f.left_pyramid = left_pyramid.data(); f.right_pyramid = right_pyramid.data();
    f.bf = F.mbf; f.b = F.mb;
  }
};
inline bool PackStereoMatches(const Frame& F, StereoPack& pk) {
  if (!F.mpORBextractorLeft || !F.mpORBextractorRight) { pk.unsupported = "no ORB extractors"; return false; }
  const std::vector<cv::Mat>& pl = F.mpORBextractorLeft->mvImagePyramid;
  const std::vector<cv::Mat>& pr = F.mpORBextractorRight->mvImagePyramid;
  if (pl.empty() || pl.size() != pr.size() || F.mvScaleFactors.size() < pl.size() || F.mvInvScaleFactors.size() < pl.size()) {
    pk.unsupported = "image pyramids and scale factors differ in their number of levels"; return false;
  }
  if (!pack_keypoints(F, pk.keys, pk.unsupported)) return false;
  auto levels = [](const std::vector<cv::Mat>& pyr, std::vector<osh_stereo_image>& out) {
    out.resize(pyr.size());
    for (size_t l = 0; l < pyr.size(); ++l) {
      const cv::Mat& m = pyr[l];
      out[l].data = m.empty() ? nullptr : m.ptr<uint8_t>(0);
      out[l].rows = m.rows; out[l].cols = m.cols; out[l].stride = (int64_t)(size_t)m.step;
    }
  };
  levels(pl, pk.left_pyramid); levels(pr, pk.right_pyramid);
  return true;
}

// The frame Frame::ComputeStereoFishEyeMatches (Frame.cc) hands to osh_orb_fisheye_stereo_match, all but Rlr / tlr: mRlr and mtlr
// are private members of Frame, so the member function fills those itself.  False (with `unsupported`) when
// the cameras are not a KannalaBrandt8 pair or the frame's members do not fit together.
struct FisheyeStereoPack {
  KeypointArrays keys;
  const char* unsupported = nullptr;
  void fill(osh_fisheye_stereo_frame& f, const Frame& F) const {
    fill_keypoints(f, keys);
    f.mono_left = F.monoLeft; f.mono_right = F.monoRight;
    f.n_levels = (int32_t)F.mvLevelSigma2.size(); f.level_sigma2 = F.mvLevelSigma2.data();
    for (int k = 0; k < 8; ++k) { f.cam1[k] = F.mpCamera->getParameter(k); f.cam2[k] = F.mpCamera2->getParameter(k); }
    f.precision1 = static_cast<KannalaBrandt8*>(F.mpCamera)->GetPrecision();
    f.precision2 = static_cast<KannalaBrandt8*>(F.mpCamera2)->GetPrecision();
  }
};
inline bool PackStereoFishEyeMatches(const Frame& F, FisheyeStereoPack& pk) {
  if (!F.mpCamera || !F.mpCamera2 || F.mpCamera->GetType() != GeometricCamera::CAM_FISHEYE || F.mpCamera2->GetType() != GeometricCamera::CAM_FISHEYE) {
    pk.unsupported = "the cameras are not a KannalaBrandt8 (CAM_FISHEYE) pair"; return false;
  }
  const size_t nl = F.mvKeys.size(), nr = F.mvKeysRight.size();
  if (F.monoLeft < 0 || (size_t)F.monoLeft > nl || F.monoRight < 0 || (size_t)F.monoRight > nr) { pk.unsupported = "monoLeft / monoRight outside the keypoints"; return false; }
  if (!pack_keypoints(F, pk.keys, pk.unsupported)) return false;
  if (F.mvLevelSigma2.empty()) { pk.unsupported = "mvLevelSigma2 is empty"; return false; }
  return true;
}

// ---- LocalMapping::CreateNewMapPoints: one (current keyframe, neighbour) segment of osh_orb_triangulate_new_points
// The poses as the reference forms them (src/LocalMapping.cc:425-430,480-484,566-574): Rcw of the pose's 3x4 matrix, its transpose,
// the translation and the camera centre.
inline void FillNewPointPose(osh_newpoint_pose& p, const Sophus::SE3f& Tcw, const Eigen::Vector3f& Ow) {
  const Eigen::Matrix3f R = Tcw.rotationMatrix();
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) { p.Rcw[3 * r + c] = R(r, c); p.Rwc[3 * c + r] = R(r, c); }
    p.tcw[r] = Tcw.translation()(r); p.Ow[r] = Ow(r);
  }
}
inline bool FillNewPointCamera(osh_newpoint_camera& c, GeometricCamera* cam) {
  const bool kb8 = cam->GetType() == GeometricCamera::CAM_FISHEYE;
  if (!kb8 && cam->GetType() != GeometricCamera::CAM_PINHOLE) return false;
  c.type = kb8 ? OSH_NEWPOINT_KB8 : OSH_NEWPOINT_PINHOLE;
  c.precision = kb8 ? static_cast<KannalaBrandt8*>(cam)->GetPrecision() : 0.f;
  for (int k = 0; k < 8; ++k) c.params[k] = k < (kb8 ? 8 : 4) ? cam->getParameter(k) : 0.f;
  return true;
}
struct NewPointPack {
  std::vector<int32_t> idx1, idx2, octave1, octave2;
  std::vector<float> pt1, pt2, u_right1, u_right2, depth1, depth2;
  const char* unsupported = nullptr;
  // the segment record; the arrays it points at live in this pack and in the two keyframes
  void fill(osh_newpoint_segment& s, KeyFrame* pKF1, KeyFrame* pKF2, float ratioFactor, bool bInertial, bool bFarPoints, float thFarPoints) const {
    KeyFrame* kfs[2] = {pKF1, pKF2};
    osh_newpoint_keyframe* out[2] = {&s.kf1, &s.kf2};
    for (int a = 0; a < 2; ++a) {
      KeyFrame* k = kfs[a];
      osh_newpoint_keyframe& o = *out[a];
      FillNewPointPose(o.pose, k->GetPose(), k->GetCameraCenter());
      FillNewPointCamera(o.camera, k->mpCamera);
      o.has_camera2 = k->mpCamera2 ? 1 : 0;
      if (k->mpCamera2) {
        FillNewPointPose(o.right_pose, k->GetRightPose(), k->GetRightCameraCenter());
        FillNewPointCamera(o.camera2, k->mpCamera2);
      } else {
        o.right_pose = o.pose; o.camera2 = o.camera;
      }
      o.fx = k->fx; o.fy = k->fy; o.cx = k->cx; o.cy = k->cy; o.invfx = k->invfx; o.invfy = k->invfy; o.mbf = k->mbf; o.mb = k->mb;
      o.n_left = k->NLeft; o.n_keys = k->N;
      o.n_levels = (int32_t)k->mvLevelSigma2.size();
      o.level_sigma2 = k->mvLevelSigma2.data(); o.scale_factors = k->mvScaleFactors.data();
    }
    s.ratio_factor = ratioFactor; s.inertial = bInertial ? 1 : 0; s.far_points = bFarPoints ? 1 : 0; s.th_far_points = thFarPoints;
    s.n_matches = (int32_t)idx1.size();
    s.idx1 = idx1.data(); s.idx2 = idx2.data(); s.pt1 = pt1.data(); s.pt2 = pt2.data(); s.octave1 = octave1.data(); s.octave2 = octave2.data();
    s.u_right1 = u_right1.data(); s.u_right2 = u_right2.data(); s.depth1 = depth1.data(); s.depth2 = depth2.data();
  }
};
// What the loop over vMatchedIndices reads per match (:497-519): the keypoint :503-505 / :515-517 choose, mvuRight and mvDepth.
// False (with pk.unsupported) for keyframes whose arrays do not fit together; the device entry checks the values.
inline bool PackNewMapPoints(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<std::pair<size_t, size_t>>& vMatchedIndices, NewPointPack& pk) {
  KeyFrame* kfs[2] = {pKF1, pKF2};
  for (KeyFrame* k : kfs) {
    if (!k->mpCamera) { pk.unsupported = "a keyframe has no camera"; return false; }
    osh_newpoint_camera c;
    if (!FillNewPointCamera(c, k->mpCamera) || (k->mpCamera2 && !FillNewPointCamera(c, k->mpCamera2))) { pk.unsupported = "a camera is neither a Pinhole nor a KannalaBrandt8"; return false; }
    if (k->mvLevelSigma2.empty() || k->mvLevelSigma2.size() != k->mvScaleFactors.size()) { pk.unsupported = "mvLevelSigma2 and mvScaleFactors do not fit together"; return false; }
    if ((int)k->mvuRight.size() < k->N || (int)k->mvDepth.size() < k->N) { pk.unsupported = "mvuRight or mvDepth is shorter than N"; return false; }
    const size_t keys = k->NLeft == -1 ? k->mvKeysUn.size() : k->mvKeys.size() + k->mvKeysRight.size();
    if ((int)keys < k->N || (k->NLeft != -1 && (int)k->mvKeys.size() != k->NLeft)) { pk.unsupported = "the keypoint arrays are shorter than N"; return false; }
  }
  const size_t n = vMatchedIndices.size();
  pk.idx1.resize(n); pk.idx2.resize(n); pk.octave1.resize(n); pk.octave2.resize(n);
  pk.pt1.resize(2 * n); pk.pt2.resize(2 * n); pk.u_right1.resize(n); pk.u_right2.resize(n); pk.depth1.resize(n); pk.depth2.resize(n);
  for (size_t i = 0; i < n; ++i) {
    const int idx1 = (int)vMatchedIndices[i].first, idx2 = (int)vMatchedIndices[i].second;
    if (idx1 < 0 || idx1 >= pKF1->N || idx2 < 0 || idx2 >= pKF2->N) { pk.unsupported = "a matched index lies outside its keyframe"; return false; }
    const cv::KeyPoint& kp1 = (pKF1->NLeft == -1) ? pKF1->mvKeysUn[idx1] : (idx1 < pKF1->NLeft) ? pKF1->mvKeys[idx1] : pKF1->mvKeysRight[idx1 - pKF1->NLeft];
    const cv::KeyPoint& kp2 = (pKF2->NLeft == -1) ? pKF2->mvKeysUn[idx2] : (idx2 < pKF2->NLeft) ? pKF2->mvKeys[idx2] : pKF2->mvKeysRight[idx2 - pKF2->NLeft];
    pk.idx1[i] = idx1; pk.idx2[i] = idx2;
    pk.pt1[2 * i] = kp1.pt.x; pk.pt1[2 * i + 1] = kp1.pt.y; pk.pt2[2 * i] = kp2.pt.x; pk.pt2[2 * i + 1] = kp2.pt.y;
    pk.octave1[i] = kp1.octave; pk.octave2[i] = kp2.octave;
    pk.u_right1[i] = pKF1->mvuRight[idx1]; pk.u_right2[i] = pKF2->mvuRight[idx2];
    pk.depth1[i] = pKF1->mvDepth[idx1]; pk.depth2[i] = pKF2->mvDepth[idx2];
  }
  return true;
}

// ---- MapPoint::RefreshBatch: one batch of osh_orb_refresh_map_points
// What MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:329-403) and UpdateNormalAndDepth (:426-494) read of each point
// of a list: its observations in map order (a left and a right index of one keyframe are two entries, left first), the descriptor
// row and the camera centre of each, whether the keyframe is bad, and the level of the reference keyframe's keypoint.
struct MapPointRefreshPack {
  std::vector<MapPoint*> points;                        // the occurrences that are refreshed, in list order
  std::vector<std::pair<KeyFrame*, int>> entry_row;     // per entry: the keyframe and the row of its mDescriptors
  std::vector<int32_t> entry_off{0}, centre, ref_centre;
  std::vector<uint8_t> desc, use_desc;
  std::vector<float> centres, pos, level_scale, top_scale;
  std::map<KeyFrame*, int> centre_of;                   // the keyframe's left centre in `centres`; the right one follows it on a rig
  void fill(osh_mappoint_batch& b) const {
    b.n_points = (int32_t)points.size(); b.entry_off = entry_off.data(); b.desc = desc.data(); b.centre = centre.data();
    b.use_desc = use_desc.data(); b.n_centres = (int32_t)(centres.size() / 3); b.centres = centres.data(); b.pos = pos.data();
    b.ref_centre = ref_centre.data(); b.level_scale = level_scale.data(); b.top_scale = top_scale.data();
  }
  int centre_index(KeyFrame* pKF) {
    const auto it = centre_of.find(pKF);
    if (it != centre_of.end()) return it->second;
    const int at = (int)(centres.size() / 3);
    const Eigen::Vector3f Ow = pKF->GetCameraCenter();
    centres.insert(centres.end(), {Ow(0), Ow(1), Ow(2)});
    if (pKF->NLeft != -1) {
      const Eigen::Vector3f Owr = pKF->GetRightCameraCenter();
      centres.insert(centres.end(), {Owr(0), Owr(1), Owr(2)});
    }
    centre_of[pKF] = at;
    return at;
  }
  void add_entry(KeyFrame* pKF, int row, int centre_at) {
    const uint8_t* d = pKF->mDescriptors.ptr<uint8_t>(row);
    desc.insert(desc.end(), d, d + 32);
    entry_row.emplace_back(pKF, row);
    centre.push_back(centre_at);
    use_desc.push_back(pKF->isBad() ? 0 : 1);
  }
};
// A bad point, a point without observations (both reference functions return early) and a point without a reference keyframe
// (the reference dereferences it) are left out.
inline void PackMapPointRefresh(const std::vector<MapPoint*>& vpMPs, MapPointRefreshPack& pk) {
  for (MapPoint* pMP : vpMPs) {
    if (!pMP || pMP->isBad()) continue;
    std::map<KeyFrame*, std::tuple<int, int>> observations = pMP->GetObservations();
    KeyFrame* pRefKF = pMP->GetReferenceKeyFrame();
    if (observations.empty() || !pRefKF) continue;
    for (const auto& ob : observations) {
      KeyFrame* pKF = ob.first;
      const int leftIndex = std::get<0>(ob.second), rightIndex = std::get<1>(ob.second);
      if (leftIndex == -1 && rightIndex == -1) continue;
      const int at = pk.centre_index(pKF);
      if (leftIndex != -1) pk.add_entry(pKF, leftIndex, at);
      if (rightIndex != -1) pk.add_entry(pKF, rightIndex, at + 1);
    }
    // :471-482; observations[pRefKF] default-constructs (0, 0) in the copy when the reference keyframe is not an observer
    const std::tuple<int, int> indexes = observations[pRefKF];
    const int leftIndex = std::get<0>(indexes), rightIndex = std::get<1>(indexes);
    int level;
    if (pRefKF->NLeft == -1) level = pRefKF->mvKeysUn[leftIndex].octave;
    else if (leftIndex != -1) level = pRefKF->mvKeys[leftIndex].octave;
    else level = pRefKF->mvKeysRight[rightIndex - pRefKF->NLeft].octave;
    const Eigen::Vector3f Pos = pMP->GetWorldPos();
    pk.points.push_back(pMP);
    pk.entry_off.push_back((int32_t)pk.centre.size());
    pk.pos.insert(pk.pos.end(), {Pos(0), Pos(1), Pos(2)});
    pk.ref_centre.push_back(pk.centre_index(pRefKF));
    pk.level_scale.push_back(pRefKF->mvScaleFactors[level]);
    pk.top_scale.push_back(pRefKF->mvScaleFactors[pRefKF->mnScaleLevels - 1]);
  }
}

// ---- LocalMapping::KeyFrameCulling: the problem of osh_orb_keyframe_cull_stage
// What the counting loop of LocalMapping::KeyFrameCulling (src/LocalMapping.cc:976-1042) reads, as the records of
// csrc/keyframe_cull.h.  The keyframe table starts with the candidates in list order (candidate c is entry c); every other observer
// follows in the order it is first met.  A candidate that is the map's initial keyframe or bad (:974) or that occurs a second time
// in the list keeps its entry and gets no slots.  A slot is packed when it holds a point and passes the depth test of :989-993; a
// bad point is packed too, its state is evaluated with the removed set.  The observations of each DISTINCT point are walked once.
// An observation with neither index (no keypoint to take a level from) is left out.
struct KeyFrameCullPack {
  std::vector<KeyFrame*> table;    // candidates first
  std::vector<MapPoint*> points;
  int32_t n_candidates = 0;
  std::vector<int32_t> cand_slot_off{0}, slot_point, slot_level, slot_index, point_n_obs, point_obs_off{0}, obs_kf, obs_level, obs_weight;
  std::vector<uint8_t> point_bad;
  void fill(osh_kfcull_problem& b, float redundant_th) const {
    b.n_keyframes = (int32_t)table.size(); b.n_candidates = n_candidates; b.redundant_th = redundant_th;
    b.cand_slot_off = cand_slot_off.data(); b.slot_point = slot_point.data(); b.slot_level = slot_level.data();
    b.n_points = (int32_t)points.size(); b.point_n_obs = point_n_obs.data(); b.point_bad = point_bad.data();
    b.point_obs_off = point_obs_off.data(); b.obs_kf = obs_kf.data(); b.obs_level = obs_level.data(); b.obs_weight = obs_weight.data();
  }
  bool within_device_limits() const {
    return n_candidates <= OSH_KFCULL_MAX_CANDIDATES && table.size() <= (size_t)OSH_KFCULL_MAX_KEYFRAMES &&
           slot_point.size() <= (size_t)OSH_KFCULL_MAX_SLOTS && points.size() <= (size_t)OSH_KFCULL_MAX_POINTS &&
           obs_kf.size() <= (size_t)OSH_KFCULL_MAX_OBSERVATIONS;
  }
};
inline void PackKeyFrameCull(const std::vector<KeyFrame*>& vpCandidates, bool bMonocular, KeyFrameCullPack& pk) {
  std::unordered_map<KeyFrame*, int> table_of;
  std::unordered_map<MapPoint*, int> point_of;
  pk.n_candidates = (int32_t)vpCandidates.size();
  std::vector<uint8_t> first(vpCandidates.size(), 0);
  for (size_t c = 0; c < vpCandidates.size(); ++c) {
    pk.table.push_back(vpCandidates[c]);
    first[c] = table_of.emplace(vpCandidates[c], (int)c).second ? 1 : 0;
  }
  for (size_t c = 0; c < vpCandidates.size(); ++c) {
    KeyFrame* pKF = vpCandidates[c];
    if (first[c] && !(pKF->mnId == pKF->GetMap()->GetInitKFid()) && !pKF->isBad()) {
      const std::vector<MapPoint*> vpMapPoints = pKF->GetMapPointMatches();
      for (size_t i = 0, iend = vpMapPoints.size(); i < iend; i++) {
        MapPoint* pMP = vpMapPoints[i];
        if (!pMP) continue;
        if (!bMonocular) {
          if (pKF->mvDepth[i] > pKF->mThDepth || pKF->mvDepth[i] < 0) continue;
        }
        // :1001-1003, with the right keypoint of a rig slot at i - NLeft (the reference reads mvKeysRight[i])
        const int scaleLevel = (pKF->NLeft == -1) ? pKF->mvKeysUn[i].octave
                               : ((int)i < pKF->NLeft) ? pKF->mvKeys[i].octave : pKF->mvKeysRight[i - pKF->NLeft].octave;
        auto at = point_of.find(pMP);
        if (at == point_of.end()) {
          at = point_of.emplace(pMP, (int)pk.points.size()).first;
          pk.points.push_back(pMP);
          pk.point_n_obs.push_back(pMP->Observations());
          pk.point_bad.push_back(pMP->isBad() ? 1 : 0);
          const std::map<KeyFrame*, std::tuple<int, int>> observations = pMP->GetObservations();
          for (const auto& ob : observations) {
            KeyFrame* pKFi = ob.first;
            const int leftIndex = std::get<0>(ob.second), rightIndex = std::get<1>(ob.second);
            if (leftIndex == -1 && rightIndex == -1) continue;
            int scaleLeveli = -1;   // :1013-1026
            if (pKFi->NLeft == -1) {
              scaleLeveli = pKFi->mvKeysUn[leftIndex == -1 ? rightIndex : leftIndex].octave;
            } else {
              if (leftIndex != -1) scaleLeveli = pKFi->mvKeys[leftIndex].octave;
              if (rightIndex != -1) {
                const int rightLevel = pKFi->mvKeysRight[rightIndex - pKFi->NLeft].octave;
                scaleLeveli = (scaleLeveli == -1 || scaleLeveli > rightLevel) ? rightLevel : scaleLeveli;
              }
            }
            int weight = 0;         // src/MapPoint.cc:178-186
            if (leftIndex != -1) weight += (!pKFi->mpCamera2 && pKFi->mvuRight[leftIndex] >= 0) ? 2 : 1;
            if (rightIndex != -1) weight += 1;
            auto kf_at = table_of.find(pKFi);
            if (kf_at == table_of.end()) {
              kf_at = table_of.emplace(pKFi, (int)pk.table.size()).first;
              pk.table.push_back(pKFi);
            }
            pk.obs_kf.push_back(kf_at->second); pk.obs_level.push_back(scaleLeveli); pk.obs_weight.push_back(weight);
          }
          pk.point_obs_off.push_back((int32_t)pk.obs_kf.size());
        }
        pk.slot_point.push_back(at->second); pk.slot_level.push_back(scaleLevel); pk.slot_index.push_back((int32_t)i);
      }
    }
    pk.cand_slot_off.push_back((int32_t)pk.slot_point.size());
  }
}
}  // namespace ORB_SLAM3
