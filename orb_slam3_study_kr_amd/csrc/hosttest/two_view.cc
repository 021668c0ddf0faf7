// two_view.cc -- the C wrappers of include/orbslam3_hip_host.h for the monocular initialisation: osh_host_two_view_cpu runs the host
// build of csrc/two_view.h (tv_reconstruct_host, the statements of two_view_device.hip on one thread; the CPU side of
// tests/test_two_view_cpu.py and of profiles/two_view_timing.py), osh_host_two_view_normalize and osh_host_two_view_decide expose its
// Normalize and its decision tables, osh_host_two_view_motion its motion hypotheses, osh_host_two_view_reconstruct drives TwoViewReconstruction::Reconstruct or a camera's
// ReconstructWithTwoViews on flat arrays; and the bodies of the stand-in cameras' ReconstructWithTwoViews.  Test library only.
#include <chrono>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "../two_view.h"
#include "CameraModels/GeometricCamera.h"
#include "TwoViewReconstruction.h"
#include "orbslam3_hip.h"
#include "orbslam3_hip_host.h"

namespace ORB_SLAM3 {

namespace {
Eigen::Matrix3f toK_(GeometricCamera& c) {
  Eigen::Matrix3f K;
  K(0, 0) = c.getParameter(0); K(0, 2) = c.getParameter(2); K(1, 1) = c.getParameter(1); K(1, 2) = c.getParameter(3); K(2, 2) = 1.f;
  return K;
}
}  // namespace

Pinhole::~Pinhole() { delete tvr; }
KannalaBrandt8::~KannalaBrandt8() { delete tvr; }

// src/CameraModels/Pinhole.cpp:83-91
bool Pinhole::ReconstructWithTwoViews(const std::vector<cv::KeyPoint>& vKeys1, const std::vector<cv::KeyPoint>& vKeys2, const std::vector<int>& vMatches12,
                                      Sophus::SE3f& T21, std::vector<cv::Point3f>& vP3D, std::vector<bool>& vbTriangulated) {
  if (!tvr) tvr = new TwoViewReconstruction(toK_(*this));
  return tvr->Reconstruct(vKeys1, vKeys2, vMatches12, T21, vP3D, vbTriangulated);
}

// src/CameraModels/KannalaBrandt8.cpp:177-201.  The reference undistorts with cv::fisheye::undistortPoints(pts, pts, K, D, I, K),
// whose arithmetic is not pinned; here a keypoint goes through unproject (:116-143, kb8_unproject) and then K: u = fx * x + cx.
bool KannalaBrandt8::ReconstructWithTwoViews(const std::vector<cv::KeyPoint>& vKeys1, const std::vector<cv::KeyPoint>& vKeys2, const std::vector<int>& vMatches12,
                                             Sophus::SE3f& T21, std::vector<cv::Point3f>& vP3D, std::vector<bool>& vbTriangulated) {
  if (!tvr) tvr = new TwoViewReconstruction(toK_(*this));
  std::vector<cv::KeyPoint> vKeysUn1 = vKeys1, vKeysUn2 = vKeys2;
  for (std::vector<cv::KeyPoint>* keys : {&vKeysUn1, &vKeysUn2})
    for (cv::KeyPoint& kp : *keys) {
      float r[3];
      osh::kb8_unproject(mvParameters.data(), precision, kp.pt.x, kp.pt.y, r);
      kp.pt.x = mvParameters[0] * r[0] + mvParameters[2];
      kp.pt.y = mvParameters[1] * r[1] + mvParameters[3];
    }
  return tvr->Reconstruct(vKeysUn1, vKeysUn2, vMatches12, T21, vP3D, vbTriangulated);
}

}  // namespace ORB_SLAM3

using namespace ORB_SLAM3;

extern "C" int osh_host_two_view_cpu(int32_t n_problems, const osh_two_view_problem* problems, const osh_two_view_result* results, double* ms) {
  if (n_problems < 0 || (n_problems && (!problems || !results))) return -1;
  const auto t0 = std::chrono::steady_clock::now();
  for (int k = 0; k < n_problems; ++k) {
    if (problems[k].n_matches < 0 || problems[k].n_iterations < 0) return -1;
    osh::tv_reconstruct_host(problems[k], results[k]);
  }
  if (ms) *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

extern "C" int osh_host_two_view_normalize(int32_t n, const float* xy, float* pn, float* T) {
  if (n < 0 || !pn || !T || (n && !xy)) return -1;
  osh::tv_normalize(xy, n, pn, T);
  return 0;
}

extern "C" int osh_host_two_view_decide(int32_t branch, int32_t n_inliers, const int32_t* n_good, const float* parallax, int32_t* winner) {
  if ((branch != 0 && branch != 1) || !n_good || !parallax || !winner) return -1;
  int w = -1;
  const int status = osh::tv_decide(branch, n_inliers, n_good, parallax, &w);
  *winner = w;
  return status;
}

extern "C" int osh_host_two_view_motion(int32_t branch, const float* model, const float* K, float* R, float* t) {
  if ((branch != 0 && branch != 1) || !model || !K || !R || !t) return -1;
  osh::TvHead h;
  osh::tv_head_clear(h);
  h.branch = branch;
  for (int k = 0; k < 9; ++k) (branch == 1 ? h.H21 : h.F21)[k] = model[k];
  osh::tv_motion(K, h);
  std::memcpy(R, h.R, sizeof(h.R));
  std::memcpy(t, h.t, sizeof(h.t));
  return h.n_hyp;
}

extern "C" int osh_host_two_view_reconstruct(int32_t camera, const float* params, float sigma, int32_t iterations, int32_t n1, const float* xy1,
                                             int32_t n2, const float* xy2, const int32_t* matches12, float* T21, float* p3d, int32_t* n_p3d,
                                             uint8_t* triangulated, int32_t* n_triangulated, int32_t* sets, int32_t* info) {
  if (camera < 0 || camera > 2 || !params || n1 < 0 || n2 < 0 || (n1 && (!xy1 || !matches12)) || (n2 && !xy2) || !n_p3d || !n_triangulated) return -1;
  std::vector<cv::KeyPoint> k1(n1), k2(n2);
  for (int i = 0; i < n1; ++i) { k1[i].pt.x = xy1[2 * i]; k1[i].pt.y = xy1[2 * i + 1]; }
  for (int i = 0; i < n2; ++i) { k2[i].pt.x = xy2[2 * i]; k2[i].pt.y = xy2[2 * i + 1]; }
  const std::vector<int> m12(matches12, matches12 + n1);
  std::vector<cv::Point3f> vP3D((size_t)*n_p3d);
  for (int i = 0; i < *n_p3d; ++i) vP3D[i] = cv::Point3f(p3d[3 * i], p3d[3 * i + 1], p3d[3 * i + 2]);
  std::vector<bool> vbTriangulated((size_t)*n_triangulated, false);
  Sophus::SE3f T;
  bool ok;
  std::unique_ptr<TwoViewReconstruction> own;
  std::unique_ptr<GeometricCamera> cam;
  TwoViewReconstruction* tvr;
  if (camera == 0) {
    Eigen::Matrix3f K;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) K(r, c) = params[3 * r + c];
    own.reset(new TwoViewReconstruction(K, sigma, iterations));
    tvr = own.get();
    ok = tvr->Reconstruct(k1, k2, m12, T, vP3D, vbTriangulated);
  } else if (camera == 1) {
    Pinhole* c = new Pinhole(std::vector<float>(params, params + 4));
    cam.reset(c);
    ok = c->ReconstructWithTwoViews(k1, k2, m12, T, vP3D, vbTriangulated);
    tvr = c->tvr;
  } else {
    KannalaBrandt8* c = new KannalaBrandt8(std::vector<float>(params, params + 8));
    cam.reset(c);
    ok = c->ReconstructWithTwoViews(k1, k2, m12, T, vP3D, vbTriangulated);
    tvr = c->tvr;
  }
  if (T21) {
    const Eigen::Matrix3f R = T.rotationMatrix();
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) T21[3 * r + c] = R(r, c); T21[9 + r] = T.translation()(r); }
  }
  // the vectors as Reconstruct left them, cut to what the caller's arrays hold (n1 entries each)
  *n_p3d = (int32_t)vP3D.size(); *n_triangulated = (int32_t)vbTriangulated.size();
  for (int i = 0; i < n1 && i < (int)vP3D.size(); ++i) if (p3d) { p3d[3 * i] = vP3D[i].x; p3d[3 * i + 1] = vP3D[i].y; p3d[3 * i + 2] = vP3D[i].z; }
  for (int i = 0; i < n1 && i < (int)vbTriangulated.size(); ++i) if (triangulated) triangulated[i] = vbTriangulated[i];
  const auto& vs = tvr->GetSets();
  if (sets) for (size_t it = 0; it < vs.size() && (int)it < iterations; ++it) for (int j = 0; j < 8; ++j) sets[8 * it + j] = (int32_t)vs[it][j];
  if (info) { info[0] = tvr->mnLastStatus; info[1] = tvr->mbLastOnDevice ? 1 : 0; info[2] = (int32_t)vs.size(); }
  return ok ? 1 : 0;
}
