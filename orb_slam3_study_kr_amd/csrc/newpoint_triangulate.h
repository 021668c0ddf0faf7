// newpoint_triangulate.h -- the body of LocalMapping::CreateNewMapPoints for one matched pair (src/LocalMapping.cc:503-720: the
// right / left choice of a rig, the ray parallax test, the choice between GeometricTools::Triangulate (src/GeometricTools.cc:47-66),
// KeyFrame::UnprojectStereo (src/KeyFrame.cc:755-772) of either keyframe and giving up, the depth tests, the two re-projection tests,
// the far-point limit and the scale consistency), with Pinhole::unprojectEig / project (src/CameraModels/Pinhole.cpp:30-33,61-64) and
// the KannalaBrandt8 pair of kb8_triangulate.h.  Device code of newpoint_device.hip; plain C++ as well, so the test library can run
// the same statements on the host.
//
// The parity rules of kb8_triangulate.h hold: single float32 operations in the reference's order with contraction off, Eigen's
// three-term reductions as a0 + (a1 + a2), sqrt, atan2 and cos as the FP64 function rounded once (cos(2 * atan2(mb / 2, depth))
// included), double comparisons where the reference compares with a double literal, invz = 1.0 / z as written.  The one deviation is
// the same as there: the null vector of A comes from the FP64 Jacobi method and x3D is rounded to float32 once after the division.
// UnprojectStereo reads mvKeys[i].pt; the match carries one pt per side (mvKeysUn on a keyframe with NLeft == -1), which is the same
// pixel on a rectified keyframe, the only kind that has mvuRight >= 0.
#pragma once
#include "kb8_triangulate.h"
#include "../../include/orbslam3_hip.h"

namespace osh {

struct NpPose { float Rcw[9], tcw[3], Rwc[9], Ow[3]; };   // row-major; GetPose / GetRotation^T / GetCameraCenter (or the Right ones)
struct NpCamera {
  int type;            // OSH_NEWPOINT_PINHOLE / OSH_NEWPOINT_KB8
  float precision;     // KannalaBrandt8::precision
  float p[8];          // mvParameters: fx fy cx cy (k1 k2 k3 k4)
};
struct NpKeyFrame {
  NpPose pose[2];      // [1]: the right camera of a rig
  NpCamera cam[2];     // mpCamera, mpCamera2
  int has_cam2;        // mpCamera2 != nullptr
  float fx, fy, cx, cy, invfx, invfy, mbf, mb;
  int n_left;          // NLeft (-1: no rig layout)
  int n_levels;
  float sigma2[OSH_NEWPOINT_MAX_LEVELS], scale[OSH_NEWPOINT_MAX_LEVELS];   // mvLevelSigma2, mvScaleFactors
};
struct NpSegment {
  NpKeyFrame kf1, kf2;  // mpCurrentKeyFrame, pKF2
  float ratio_factor;   // 1.5f * mpCurrentKeyFrame->mfScaleFactor
  int inertial, far_points;
  float th_far;
  int n_matches, base;  // base: offset of the segment's matches in the arrays of the batch
};
struct NpMatch {
  int idx1, idx2;
  float x1, y1, x2, y2;   // kp1.pt, kp2.pt
  int oct1, oct2;
  float ur1, ur2, d1, d2; // mvuRight[idx], mvDepth[idx]
};
struct NpOut {
  int stage, source;
  float cosp, x3D[3];
};

OSH_KB8_HD void np_unproject(const NpCamera& c, float x, float y, float r[3]) {
#pragma clang fp contract(off)
  if (c.type == OSH_NEWPOINT_KB8) { kb8_unproject(c.p, c.precision, x, y, r); return; }
  r[0] = (x - c.p[2]) / c.p[0]; r[1] = (y - c.p[3]) / c.p[1]; r[2] = 1.f;
}
OSH_KB8_HD void np_project(const NpCamera& c, const float v[3], float uv[2]) {
#pragma clang fp contract(off)
  if (c.type == OSH_NEWPOINT_KB8) { kb8_project(c.p, v, uv); return; }
  uv[0] = c.p[0] * v[0] / v[2] + c.p[2];
  uv[1] = c.p[1] * v[1] / v[2] + c.p[3];
}
OSH_KB8_HD float np_row_dot(const float* R, int row, const float v[3]) {
#pragma clang fp contract(off)
  return kb8_sum3(R[3 * row] * v[0], R[3 * row + 1] * v[1], R[3 * row + 2] * v[2]);
}
OSH_KB8_HD float np_norm(const float v[3]) {
#pragma clang fp contract(off)
  return kb8_sqrt(kb8_sum3(v[0] * v[0], v[1] * v[1], v[2] * v[2]));
}
// cos(2*atan2(mb/2, mvDepth[idx])) (:590,592): atan2(float, float) and cos(float) are the float overloads
OSH_KB8_HD float np_cos_stereo(float mb, float depth) {
#pragma clang fp contract(off)
  const float half = mb / 2.f;
  const float angle = 2.f * (float)atan2((double)half, (double)depth);
  return (float)cos((double)angle);
}
// KeyFrame::UnprojectStereo (src/KeyFrame.cc:755-772): mRwc and mTwc.translation() are the left camera's
OSH_KB8_HD bool np_unproject_stereo(const NpKeyFrame& k, float u, float v, float z, float x3D[3]) {
#pragma clang fp contract(off)
  if (!(z > 0)) return false;
  float c[3];
  c[0] = (u - k.cx) * z * k.invfx;
  c[1] = (v - k.cy) * z * k.invfy;
  c[2] = z;
#pragma unroll
  for (int i = 0; i < 3; ++i) x3D[i] = np_row_dot(k.pose[0].Rwc, i, c) + k.pose[0].Ow[i];
  return true;
}

// One side's re-projection test (:646-697).  mbf is mpCurrentKeyFrame's for both keyframes (:665,690).  True: the pair goes on.
OSH_KB8_HD bool np_reproject(const NpPose& P, const NpCamera& C, const NpKeyFrame& k, bool stereo, float mbf_current, const float x3D[3], float z,
                             float px, float py, float ur, float sigma2) {
#pragma clang fp contract(off)
  const float x = np_row_dot(P.Rcw, 0, x3D) + P.tcw[0];
  const float y = np_row_dot(P.Rcw, 1, x3D) + P.tcw[1];
  const float invz = (float)(1.0 / (double)z);
  if (!stereo) {
    const float v[3] = {x, y, z};
    float uv[2];
    np_project(C, v, uv);
    const float errX = uv[0] - px, errY = uv[1] - py;
    return !((double)(errX * errX + errY * errY) > 5.991 * (double)sigma2);
  }
  const float u = k.fx * x * invz + k.cx;
  const float u_r = u - mbf_current * invz;
  const float v = k.fy * y * invz + k.cy;
  const float errX = u - px, errY = v - py, errX_r = u_r - ur;
  return !((double)(errX * errX + errY * errY + errX_r * errX_r) > 7.8 * (double)sigma2);
}

OSH_KB8_HD void newpoint_triangulate(const NpSegment& s, const NpMatch& m, NpOut& o) {
#pragma clang fp contract(off)
  const NpKeyFrame& k1 = s.kf1;
  const NpKeyFrame& k2 = s.kf2;
  o.source = OSH_NEWPOINT_NO_SOURCE;
  o.x3D[0] = o.x3D[1] = o.x3D[2] = 0.f;
  // :503-575
  const bool bStereo1 = !k1.has_cam2 && m.ur1 >= 0;
  const bool bStereo2 = !k2.has_cam2 && m.ur2 >= 0;
  const bool bRight1 = !(k1.n_left == -1 || m.idx1 < k1.n_left);
  const bool bRight2 = !(k2.n_left == -1 || m.idx2 < k2.n_left);
  const bool rig = k1.has_cam2 && k2.has_cam2;
  const int side1 = rig && bRight1 ? 1 : 0, side2 = rig && bRight2 ? 1 : 0;
  const NpPose& P1 = k1.pose[side1];
  const NpPose& P2 = k2.pose[side2];
  const NpCamera& C1 = k1.cam[side1];
  const NpCamera& C2 = k2.cam[side2];
  // :577-597
  float xn1[3], xn2[3], ray1[3], ray2[3];
  np_unproject(C1, m.x1, m.y1, xn1);
  np_unproject(C2, m.x2, m.y2, xn2);
#pragma unroll
  for (int i = 0; i < 3; ++i) { ray1[i] = np_row_dot(P1.Rwc, i, xn1); ray2[i] = np_row_dot(P2.Rwc, i, xn2); }
  const float cosParallaxRays = kb8_sum3(ray1[0] * ray2[0], ray1[1] * ray2[1], ray1[2] * ray2[2]) / (np_norm(ray1) * np_norm(ray2));
  o.cosp = cosParallaxRays;
  float cosParallaxStereo = cosParallaxRays + 1.f;
  float cosParallaxStereo1 = cosParallaxStereo, cosParallaxStereo2 = cosParallaxStereo;
  if (bStereo1) cosParallaxStereo1 = np_cos_stereo(k1.mb, m.d1);
  else if (bStereo2) cosParallaxStereo2 = np_cos_stereo(k2.mb, m.d2);
  cosParallaxStereo = cosParallaxStereo2 < cosParallaxStereo1 ? cosParallaxStereo2 : cosParallaxStereo1;   // std::min
  // :599-635
  float x3D[3];
  const double cosd = (double)cosParallaxRays;
  if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0.f &&
      (bStereo1 || bStereo2 || (cosd < 0.9996 && s.inertial) || (cosd < 0.9998 && !s.inertial))) {
    o.source = OSH_NEWPOINT_TRIANGULATED;
    float A[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float t1_0 = j < 3 ? P1.Rcw[j] : P1.tcw[0], t1_1 = j < 3 ? P1.Rcw[3 + j] : P1.tcw[1], t1_2 = j < 3 ? P1.Rcw[6 + j] : P1.tcw[2];
      const float t2_0 = j < 3 ? P2.Rcw[j] : P2.tcw[0], t2_1 = j < 3 ? P2.Rcw[3 + j] : P2.tcw[1], t2_2 = j < 3 ? P2.Rcw[6 + j] : P2.tcw[2];
      A[0][j] = xn1[0] * t1_2 - t1_0;
      A[1][j] = xn1[1] * t1_2 - t1_1;
      A[2][j] = xn2[0] * t2_2 - t2_0;
      A[3][j] = xn2[1] * t2_2 - t2_1;
    }
    double h[4];
    kb8_null_vector_h(A, h);
    if (h[3] == 0.0) { o.stage = OSH_NEWPOINT_W_ZERO; return; }
    x3D[0] = (float)(h[0] / h[3]); x3D[1] = (float)(h[1] / h[3]); x3D[2] = (float)(h[2] / h[3]);
  } else if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2) {
    o.source = OSH_NEWPOINT_STEREO_1;
    if (!np_unproject_stereo(k1, m.x1, m.y1, m.d1, x3D)) { o.stage = OSH_NEWPOINT_NO_DEPTH; return; }
  } else if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1) {
    o.source = OSH_NEWPOINT_STEREO_2;
    if (!np_unproject_stereo(k2, m.x2, m.y2, m.d2, x3D)) { o.stage = OSH_NEWPOINT_NO_DEPTH; return; }
  } else {
    o.stage = OSH_NEWPOINT_LOW_PARALLAX;
    return;
  }
  o.x3D[0] = x3D[0]; o.x3D[1] = x3D[1]; o.x3D[2] = x3D[2];
  // :637-697
  const float z1 = np_row_dot(P1.Rcw, 2, x3D) + P1.tcw[2];
  if (z1 <= 0) { o.stage = OSH_NEWPOINT_BEHIND_1; return; }
  const float z2 = np_row_dot(P2.Rcw, 2, x3D) + P2.tcw[2];
  if (z2 <= 0) { o.stage = OSH_NEWPOINT_BEHIND_2; return; }
  if (!np_reproject(P1, C1, k1, bStereo1, k1.mbf, x3D, z1, m.x1, m.y1, m.ur1, k1.sigma2[m.oct1])) { o.stage = OSH_NEWPOINT_REPROJ_1; return; }
  if (!np_reproject(P2, C2, k2, bStereo2, k1.mbf, x3D, z2, m.x2, m.y2, m.ur2, k2.sigma2[m.oct2])) { o.stage = OSH_NEWPOINT_REPROJ_2; return; }
  // :699-720
  const float normal1[3] = {x3D[0] - P1.Ow[0], x3D[1] - P1.Ow[1], x3D[2] - P1.Ow[2]};
  const float normal2[3] = {x3D[0] - P2.Ow[0], x3D[1] - P2.Ow[1], x3D[2] - P2.Ow[2]};
  const float dist1 = np_norm(normal1), dist2 = np_norm(normal2);
  if (dist1 == 0 || dist2 == 0) { o.stage = OSH_NEWPOINT_ZERO_DIST; return; }
  if (s.far_points && (dist1 >= s.th_far || dist2 >= s.th_far)) { o.stage = OSH_NEWPOINT_FAR; return; }
  const float ratioDist = dist2 / dist1;
  const float ratioOctave = k1.scale[m.oct1] / k2.scale[m.oct2];
  if (ratioDist * s.ratio_factor < ratioOctave || ratioDist > ratioOctave * s.ratio_factor) { o.stage = OSH_NEWPOINT_SCALE; return; }
  o.stage = OSH_NEWPOINT_ACCEPTED;
}

// ---- host side: the device records of a segment of the C-ABI (the segment must have passed the entry's validation)
inline void np_fill_pose(NpPose& d, const osh_newpoint_pose& p) {
  for (int i = 0; i < 9; ++i) { d.Rcw[i] = p.Rcw[i]; d.Rwc[i] = p.Rwc[i]; }
  for (int i = 0; i < 3; ++i) { d.tcw[i] = p.tcw[i]; d.Ow[i] = p.Ow[i]; }
}
inline void np_fill_camera(NpCamera& d, const osh_newpoint_camera& c) {
  d.type = c.type; d.precision = c.precision;
  for (int i = 0; i < 8; ++i) d.p[i] = c.params[i];
}
inline void np_fill_keyframe(NpKeyFrame& d, const osh_newpoint_keyframe& k) {
  d = NpKeyFrame{};
  np_fill_pose(d.pose[0], k.pose); np_fill_camera(d.cam[0], k.camera);
  d.has_cam2 = k.has_camera2 ? 1 : 0;
  if (d.has_cam2) { np_fill_pose(d.pose[1], k.right_pose); np_fill_camera(d.cam[1], k.camera2); }
  d.fx = k.fx; d.fy = k.fy; d.cx = k.cx; d.cy = k.cy; d.invfx = k.invfx; d.invfy = k.invfy; d.mbf = k.mbf; d.mb = k.mb;
  d.n_left = k.n_left; d.n_levels = k.n_levels;
  for (int l = 0; l < OSH_NEWPOINT_MAX_LEVELS; ++l) {
    d.sigma2[l] = l < k.n_levels ? k.level_sigma2[l] : 1.f;
    d.scale[l] = l < k.n_levels ? k.scale_factors[l] : 1.f;
  }
}
inline void np_fill_segment(NpSegment& d, const osh_newpoint_segment& s, int base) {
  np_fill_keyframe(d.kf1, s.kf1); np_fill_keyframe(d.kf2, s.kf2);
  d.ratio_factor = s.ratio_factor; d.inertial = s.inertial ? 1 : 0; d.far_points = s.far_points ? 1 : 0; d.th_far = s.th_far_points;
  d.n_matches = s.n_matches; d.base = base;
}
inline NpMatch np_match_of(const osh_newpoint_segment& s, int i) {
  return NpMatch{s.idx1[i], s.idx2[i], s.pt1[2 * i], s.pt1[2 * i + 1], s.pt2[2 * i], s.pt2[2 * i + 1], s.octave1[i], s.octave2[i],
                 s.u_right1[i], s.u_right2[i], s.depth1[i], s.depth2[i]};
}

}  // namespace osh
