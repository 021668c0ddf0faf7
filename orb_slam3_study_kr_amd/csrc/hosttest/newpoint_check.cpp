// newpoint_check.cpp -- csrc/newpoint_triangulate.h as plain C++ under AddressSanitizer and UBSan: a program of its own (make
// newpoint-check) that makes no HIP call and needs no device.  It runs the per-match statements of LocalMapping::CreateNewMapPoints
// over a grid of pixel pairs for every camera kind (pinhole mono, rectified stereo, KannalaBrandt8, rig with its four left / right
// combinations), with the values a validated call can still carry at their extremes (zero and negative depths, keypoints far outside
// the image, identical keypoints, the highest octave), and checks that every pair ends with a stage and a source of the C-ABI and
// that x3D is 0 where no point was computed.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../newpoint_triangulate.h"

static void pose(osh_newpoint_pose& p, float yaw, float tx, float ty, float tz) {
  const float c = std::cos(yaw), s = std::sin(yaw);
  const float R[9] = {c, 0, s, 0, 1, 0, -s, 0, c};
  for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) { p.Rcw[3 * r + k] = R[3 * r + k]; p.Rwc[3 * k + r] = R[3 * r + k]; }
  p.tcw[0] = tx; p.tcw[1] = ty; p.tcw[2] = tz;
  for (int r = 0; r < 3; ++r) p.Ow[r] = -(p.Rwc[3 * r] * tx + p.Rwc[3 * r + 1] * ty + p.Rwc[3 * r + 2] * tz);
}

int main() {
  static const float sigma2[OSH_NEWPOINT_MAX_LEVELS] = {1, 1.44f, 2.07f, 2.99f, 4.3f, 6.19f, 8.92f, 12.8f, 18.5f, 26.6f, 38.3f, 55.2f, 79.5f, 114.f, 165.f, 237.f};
  static const float scale[OSH_NEWPOINT_MAX_LEVELS] = {1, 1.2f, 1.44f, 1.73f, 2.07f, 2.49f, 2.99f, 3.58f, 4.3f, 5.16f, 6.19f, 7.43f, 8.92f, 10.7f, 12.8f, 15.4f};
  const float kb8[8] = {190.978f, 190.973f, 254.931f, 256.897f, 0.0034824f, 0.00071503f, -0.0020532f, 0.00020294f};
  const float pin[8] = {458.654f, 457.296f, 367.215f, 248.375f, 0, 0, 0, 0};
  long pairs = 0, stages[11] = {0};
  for (int kind = 0; kind < 4; ++kind) {          // 0 pinhole mono, 1 rectified stereo, 2 KannalaBrandt8, 3 rig
    osh_newpoint_segment s{};
    osh_newpoint_keyframe* kfs[2] = {&s.kf1, &s.kf2};
    for (int a = 0; a < 2; ++a) {
      osh_newpoint_keyframe& k = *kfs[a];
      pose(k.pose, 0.03f * a, -0.4f * a, 0.01f * a, 0.05f * a);
      pose(k.right_pose, 0.03f * a + 0.01f, -0.4f * a - 0.1f, 0.01f * a, 0.05f * a);
      const float* cam = kind >= 2 ? kb8 : pin;
      k.camera.type = k.camera2.type = kind >= 2 ? OSH_NEWPOINT_KB8 : OSH_NEWPOINT_PINHOLE;
      k.camera.precision = k.camera2.precision = 1e-6f;
      for (int i = 0; i < 8; ++i) k.camera.params[i] = k.camera2.params[i] = cam[i];
      k.has_camera2 = kind == 3;
      k.fx = cam[0]; k.fy = cam[1]; k.cx = cam[2]; k.cy = cam[3]; k.invfx = 1.f / k.fx; k.invfy = 1.f / k.fy;
      k.mb = kind == 1 ? 0.1f : 0.f; k.mbf = k.mb * k.fx;
      k.n_left = kind == 3 ? 2 : -1; k.n_keys = 4; k.n_levels = OSH_NEWPOINT_MAX_LEVELS;
      k.level_sigma2 = sigma2; k.scale_factors = scale;
    }
    s.ratio_factor = 1.8f;
    const float xs[] = {-1.0e6f, -50.f, 0.f, 120.f, 254.931f, 367.215f, 400.f, 700.f, 1.0e6f};
    const float depths[] = {-1.f, 0.f, 1e-30f, 0.3f, 2.f, 1.0e6f};
    std::vector<int32_t> idx1, idx2, o1, o2;
    std::vector<float> p1, p2, ur1, ur2, d1, d2;
    for (float x1 : xs) for (float y1 : {0.f, 248.375f, 500.f}) for (float x2 : xs) for (float y2 : {10.f, 256.897f})
      for (float da : depths) for (int v = 0; v < 4; ++v) {
        idx1.push_back(v & 1 ? 3 : 0); idx2.push_back(v & 2 ? 3 : 0);
        o1.push_back(v == 0 ? 0 : OSH_NEWPOINT_MAX_LEVELS - 1); o2.push_back(v == 3 ? 0 : 7);
        p1.push_back(x1); p1.push_back(y1); p2.push_back(x2); p2.push_back(y2);
        ur1.push_back(v & 1 ? x1 - 5.f : -1.f); ur2.push_back(v & 2 ? x2 - 5.f : -1.f);
        d1.push_back(da); d2.push_back(v == 1 ? -1.f : da);
      }
    s.n_matches = (int32_t)idx1.size();
    s.idx1 = idx1.data(); s.idx2 = idx2.data(); s.pt1 = p1.data(); s.pt2 = p2.data(); s.octave1 = o1.data(); s.octave2 = o2.data();
    s.u_right1 = ur1.data(); s.u_right2 = ur2.data(); s.depth1 = d1.data(); s.depth2 = d2.data();
    for (int flags = 0; flags < 4; ++flags) {
      s.inertial = flags & 1; s.far_points = flags >> 1; s.th_far_points = 3.f;
      osh::NpSegment seg;
      osh::np_fill_segment(seg, s, 0);
      for (int i = 0; i < s.n_matches; ++i) {
        osh::NpOut o;
        osh::newpoint_triangulate(seg, osh::np_match_of(s, i), o);
        const bool source_ok = o.source == OSH_NEWPOINT_NO_SOURCE ? o.stage == OSH_NEWPOINT_LOW_PARALLAX : (o.source >= 0 && o.source <= OSH_NEWPOINT_STEREO_2);
        if (o.stage < 0 || o.stage > OSH_NEWPOINT_ACCEPTED || !source_ok) { std::printf("kind %d pair %d: stage %d source %d\n", kind, i, o.stage, o.source); return 1; }
        if (o.stage < OSH_NEWPOINT_BEHIND_1 && (o.x3D[0] != 0 || o.x3D[1] != 0 || o.x3D[2] != 0)) { std::printf("kind %d pair %d: x3D without a point\n", kind, i); return 1; }
        if (kind == 3 && o.source != OSH_NEWPOINT_NO_SOURCE && o.source != OSH_NEWPOINT_TRIANGULATED) { std::printf("rig pair %d took a stereo source\n", i); return 1; }
        ++stages[o.stage]; ++pairs;
      }
    }
  }
  std::printf("newpoint_check: %ld pairs, stages", pairs);
  for (long n : stages) std::printf(" %ld", n);
  std::printf("\n");
  return 0;
}
